"""_lib.ABI, the one table of the C ABI: every public header is in it, each header declares exactly its
table's functions with the table's number of parameters, no name is in two tables, every name is bound on the loaded library
as its table says, and the file lists the build compiles and watches are all of csrc/.  No device is needed."""
import glob
import os
import re

import pytest

from control_pcgrl_amd import _lib

INCLUDE = os.path.join(os.path.dirname(_lib.CSRC), os.pardir, "include")


def _declarations(header):
    """{function: number of parameters} of a header, comments stripped as the family tests strip them"""
    text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    found = {}
    for name, params in re.findall(r"\b(pcgrl_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        assert name not in found, f"{name} is declared twice in {header}"
        found[name] = 0 if params.strip() in ("", "void") else len(params.split(","))
    return found


def test_every_public_header_is_in_the_table_once():
    names = [name for name, _ in _lib.ABI]
    assert len(set(names)) == len(names) and len({id(table) for _, table in _lib.ABI}) == len(names)
    for name in names:
        assert os.path.exists(os.path.join(INCLUDE, name)), name
    on_disk = {os.path.basename(p) for p in glob.glob(os.path.join(INCLUDE, "pcgrl_amd*.h"))}
    assert on_disk and on_disk == set(names)
    # the module attributes the family tests read are the table's entries
    headers = {v for k, v in vars(_lib).items() if k == "HEADER" or k.endswith("_HEADER")}
    assert {os.path.realpath(h) for h in headers} == {os.path.realpath(os.path.join(INCLUDE, n)) for n in names}
    tables = [v for k, v in vars(_lib).items() if k == "SYMBOLS" or k.endswith("_SYMBOLS")]
    assert sorted(map(id, tables)) == sorted(id(table) for _, table in _lib.ABI)


@pytest.mark.parametrize("name,table", _lib.ABI, ids=[name for name, _ in _lib.ABI])
def test_header_declares_exactly_its_table(name, table):
    declared = _declarations(os.path.join(INCLUDE, name))
    assert set(declared) == set(table)
    for fn, n_params in declared.items():
        assert n_params == len(table[fn][1]), fn


def test_tables_are_pairwise_disjoint():
    seen = {}
    for name, table in _lib.ABI:
        for fn in table:
            assert fn not in seen, f"{fn} is in the tables of {seen.get(fn)} and {name}"
            seen[fn] = name


def test_every_name_is_bound_as_its_table_says():
    _lib.build()
    L = _lib.lib()
    for name, table in _lib.ABI:
        for fn, (restype, argtypes) in table.items():
            bound = getattr(L, fn)  # exported by the library
            assert bound.restype == restype and bound.argtypes == argtypes, (name, fn)


def test_units_and_headers_are_all_of_csrc():
    on_disk = {".hip": [], ".h": []}
    for root, dirs, files in os.walk(_lib.CSRC):
        dirs[:] = [d for d in dirs if not d.startswith("_obj")]
        for f in files:
            ext = os.path.splitext(f)[1]
            if ext in on_disk:
                on_disk[ext].append(os.path.relpath(os.path.join(root, f), _lib.CSRC).replace(os.sep, "/"))
    assert _lib.UNITS == sorted(on_disk[".hip"]) and _lib.HEADERS == sorted(on_disk[".h"])
    assert "pcgrl_engine.hip" in _lib.UNITS and "smb/pcgrl_smb_ctrl.h" in _lib.HEADERS
    objects = [os.path.basename(u) for u in _lib.UNITS]  # build() names a unit's object by its base name
    assert len(set(objects)) == len(objects)
