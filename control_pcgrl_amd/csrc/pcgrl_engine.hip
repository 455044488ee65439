// pcgrl_engine.hip -- host side of libpcgrl_amd.so: the C ABI declared in include/pcgrl_amd.h.
//
// Owns the per-env state in HBM, seeds the numpy-compatible RNG streams, validates configs and launches the
// gfx950 kernels of pcgrl_kernels2d.h / pcgrl_kernels3d.h on the caller's HIP stream.  No torch types, no
// hidden synchronisation in reset/step/observe.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include <map>
#include <mutex>
#include <tuple>

#include "pcgrl_common.h"
#include "pcgrl_dispatch.h"
#include "pcgrl_kernels2d.h"  // U128 / Pcg (host side of the RNG), the small engine-level kernels
#include "pcgrl_sokoban.h"    // sokoban_alloc
#include "pcgrl_kernels3d.h"  // M3_* limits
#include "codes/pcgrl_codes.h"
#include "reps3d/pcgrl_reps3d.h"  // the 3-D maze under turtle / wide
#include "async3d/pcgrl_async3d.h"  // the 3-D maze (narrow) under a solver budget
#include "paths/pcgrl_paths.h"      // solution paths of binary / zelda maps
#include "solutions/pcgrl_solutions.h"  // sokoban solutions (the move list behind sol-length)
#include "multiagent/pcgrl_multiagent.h"  // multi-agent turtle stepping (binary, zelda)
#include "measures/pcgrl_measures.h"  // level measures and pairwise Hamming diversity of 2-D maps
#include "smb/pcgrl_smb.h"            // Super Mario Bros levels: statistics and A* play-through
#include "../../include/pcgrl_amd_codes.h"
#include "../../include/pcgrl_amd_async3d.h"
#include "../../include/pcgrl_amd_paths.h"
#include "../../include/pcgrl_amd_solutions.h"
#include "../../include/pcgrl_amd_multiagent.h"
#include "../../include/pcgrl_amd_measures.h"
#include "../../include/pcgrl_amd_smb.h"
#include "../../include/pcgrl_amd_smb_env.h"
#include "smb/pcgrl_smb_env.h"
#include "../../include/pcgrl_amd_smb_ready.h"
#include "smb/pcgrl_smb_ready.h"  // the same envs under a solver budget
#include "../../include/pcgrl_amd_smb_state.h"
#include "smb/pcgrl_smb_state.h"  // their checkpoint and restore
#include "../../include/pcgrl_amd_smb_rollout.h"
#include "smb/pcgrl_smb_rollout.h"  // K steps in one launch, device-drawn actions
#include "../../include/pcgrl_amd_smb_ctrl.h"
#include "smb/pcgrl_smb_ctrl.h"  // controllable generation: per-env targets
#include "../../include/pcgrl_amd_smb_vector.h"
#include "smb/pcgrl_smb_vector.h"  // the float32 hand-out (RLlib's Box form)
#include "../../include/pcgrl_amd_smb_measures.h"
#include "smb/pcgrl_smb_measures.h"  // level measures and pairwise Hamming diversity of smb maps
#include "../../include/pcgrl_amd_loderunner.h"
#include "loderunner/pcgrl_loderunner.h"  // Lode Runner levels: statistics, win score and gold searches
#include "../../include/pcgrl_amd_loderunner_routes.h"
#include "loderunner/pcgrl_loderunner_routes.h"  // the routes behind path-length
#include "../../include/pcgrl_amd_loderunner_measures.h"
#include "loderunner/pcgrl_loderunner_measures.h"  // level measures and pairwise Hamming diversity of Lode Runner maps
#include "../../include/pcgrl_amd_microstructure.h"
#include "microstructure/pcgrl_microstructure.h"  // microstructure levels: path-length, tortuosity, measures
#include "../../include/pcgrl_amd_ddave.h"
#include "ddave/pcgrl_ddave.h"  // Dangerous Dave levels: statistics and the four-stage play-through, measures
#include "../../include/pcgrl_amd_mdungeon.h"
#include "mdungeon/pcgrl_mdungeon.h"  // MiniDungeon levels: statistics and the four-stage play-through, measures
#include "../../include/pcgrl_amd_mc3d_holey.h"
#include "mc3d_holey/pcgrl_mc3d_holey.h"  // 3-D holey dungeon and maze levels: statistics, loss and routes
#include "step16/pcgrl_step16.h"  // the binary 16x16 step (narrow / turtle, 32x32 window) as a kernel of its own

using namespace pcgrl;

static thread_local std::string g_err;
static int fail(int code, const std::string &msg) {
  g_err = msg;
  return code;
}
#define HIPCHK(x)                                                                                   \
  do {                                                                                              \
    hipError_t _e = (x);                                                                            \
    if (_e != hipSuccess) return fail(PCGRL_EHIP, std::string(#x) + ": " + hipGetErrorString(_e)); \
  } while (0)

namespace pcgrl {
struct RedScratch;
struct SampleState;
}
struct pcgrl_engine {
  Params p;
  int device = 0;
  int lpe = 16;
  size_t lds_bytes = 0;
  int cpl = 0;  // 3-D: cells per lane of the reset RNG split
  int32_t *seen_host = nullptr;  // sokoban: host-mapped counter of device solver runs
  int soko_slots = 0;            // sokoban: workspace slots of the current pool (p.soko)
  int32_t seen_last = 0, spread_left = 0;
  bool soko_lazy = true;         // grow the solver pool by itself the first time the solver has been seen running
  int sk_budget = 0;             // sokoban, asynchronous stepping: solver iteration units per env and launch (0 = synchronous)
  void *a3_park = nullptr;       // 3-D maze (narrow), asynchronous stepping: one park record per env (async3d/pcgrl_async3d.h)
  void *sk_ws = nullptr, *sk_park = nullptr;  // ... and its per-env stage workspaces / park records (also in the device SokoPool)
  bool soko_grow_failed = false; // the last growth attempt failed (message in soko_grow_msg): not retried by itself
  std::string soko_grow_msg;
  uint8_t *hdr_host = nullptr;   // pinned: the 256-byte header of pcgrl_export_state images (rebuilt by pcgrl_set_static)
  // development switches, read ONCE at pcgrl_create (never getenv() in a stepping call: not thread-safe against a host's
  // putenv, and a stray variable must not steer a running engine): PCGRL_ROLLOUT_KERNEL 1 = always the one-launch rollout
  // kernel, 0 = always step launches, unset = by shape; PCGRL_OBS_NT_MB = observation bytes per launch (MB) from which the
  // stores are non-temporal (default 384, 0 = never)
  int rollout_form = -1;
  bool step16 = true;  // PCGRL_STEP16=0: the binary 16x16 step stays on step_kernel (A/B runs against step16_kernel, the parity test)
  int rollout_epw = -1;  // PCGRL_ROLLOUT_EPW (development): envs per wavefront of the rollout's simulate role, -1 = chosen by batch size
  // pcgrl_rollout as two kernels (16x16 compile-time kernels, plain mode): the observe role runs on this stream from a
  // snapshot of the pre-call state (tile planes, the scalars of the hot state line, both RNG streams)
  bool split_ok = false;
  int64_t two_role_resident = 0;  // workgroups of the two-role rollout kernel the device holds at once (occupancy x CUs)
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  void *snap_planes = nullptr;
  EnvState *snap_st = nullptr;
  RngState *snap_rng = nullptr;
  long obs_nt_mb = 384;
  bool maybe_stale = false;  // pcgrl_update ran since the last refresh / full reset: some env may carry ENV_STATS_DIRTY
  int64_t obs_bytes = 0;
  int obs_ndim = 0;
  int32_t obs_shape[4] = {0, 0, 0, 0};
  RedScratch *red = nullptr;  // pcgrl_reduce_episodes block partials
  SampleState *sample = nullptr;  // pcgrl_sample_actions: draw counter + ticket
  // multi-agent turtle stepping (pcgrl_ma_attach): the side arrays and the shape of one agent's observation
  bool ma_on = false;
  MaArgs ma = {};
  size_t ma_lds = 0;
  int64_t ma_obs_bytes = 0;
  int32_t ma_obs_shape[3] = {0, 0, 0};
  std::vector<void *> allocs;
  // the persistent per-env arrays (pointer, bytes per env): what pcgrl_export_state / pcgrl_import_state carry
  std::vector<std::pair<void *, size_t>> state_arrays;
};

extern "C" {
static void state_header_build(pcgrl_engine *h);
}

// ---------------------------------------------------------------------------------------------- RNG seeding (host)
// numpy.random.SeedSequence(seed).generate_state(4, uint64) -> PCG64 state/inc (numpy/random/bit_generator.pyx,
// _pcg64.pyx, src/pcg64/pcg64.h); reached in the reference through gymnasium.utils.seeding.np_random
// (envs/reps/representation.py:50-53, envs/probs/problem.py:79-81).
static void seedseq_words(uint64_t seed, uint64_t out[4]) {
  const uint32_t INIT_A = 0x43b0d7e5u, MULT_A = 0x931e8875u, INIT_B = 0x8b51f9ddu, MULT_B = 0x58f38dedu;
  const uint32_t MIX_L = 0xca01f9ddu, MIX_R = 0x4973f715u;
  uint32_t ent[4] = {(uint32_t)seed, (uint32_t)(seed >> 32), 0, 0};
  int n_ent = ent[1] ? 2 : 1;
  uint32_t pool[4], hc = INIT_A;
  auto hashmix = [&](uint32_t v) {
    v ^= hc;
    hc *= MULT_A;
    v *= hc;
    v ^= v >> 16;
    return v;
  };
  for (int i = 0; i < 4; i++) pool[i] = hashmix(i < n_ent ? ent[i] : 0u);
  for (int s = 0; s < 4; s++)
    for (int d = 0; d < 4; d++)
      if (s != d) {
        uint32_t r = MIX_L * pool[d] - MIX_R * hashmix(pool[s]);
        r ^= r >> 16;
        pool[d] = r;
      }
  uint32_t w[8], hb = INIT_B;
  for (int i = 0; i < 8; i++) {
    uint32_t v = pool[i & 3] ^ hb;
    hb *= MULT_B;
    v *= hb;
    v ^= v >> 16;
    w[i] = v;
  }
  for (int i = 0; i < 4; i++) out[i] = (uint64_t)w[2 * i] | ((uint64_t)w[2 * i + 1] << 32);
}

static void pcg64_seed_state(uint64_t seed, uint64_t st[4]) {
  uint64_t w[4];
  seedseq_words(seed, w);
  const U128 mult{PCG_MULT_HI, PCG_MULT_LO};
  U128 initstate{w[0], w[1]}, initseq{w[2], w[3]};
  U128 inc{(initseq.hi << 1) | (initseq.lo >> 63), (initseq.lo << 1) | 1ull};
  U128 s{0, 0};
  s = add128(mul128(s, mult), inc);
  s = add128(s, initstate);
  s = add128(mul128(s, mult), inc);
  st[0] = s.hi;
  st[1] = s.lo;
  st[2] = inc.hi;
  st[3] = inc.lo;
}

// ---------------------------------------------------------------------------------------------- config
static int n_tiles_of(int prob) {
  switch (prob) {
    case PCGRL_PROB_BINARY: return 2;
    case PCGRL_PROB_ZELDA: return 8;
    case PCGRL_PROB_SOKOBAN: return 5;
    case PCGRL_PROB_MC3DMAZE: return 2;
  }
  return 0;
}
static int n_stats_of(int prob) {
  switch (prob) {
    case PCGRL_PROB_BINARY: return 2;
    case PCGRL_PROB_ZELDA: return 7;
    case PCGRL_PROB_SOKOBAN: return 7;
    case PCGRL_PROB_MC3DMAZE: return 3;
  }
  return 0;
}

static int validate(const pcgrl_config &c, int &lpe, int64_t &obs_bytes, int &obs_chunks, int32_t shape[4], int &ndim) {
  if (c.problem < 0 || c.problem > PCGRL_PROB_MC3DMAZE) return fail(PCGRL_EINVAL, "unknown problem");
  if (c.representation < 0 || c.representation > PCGRL_REP_WIDE) return fail(PCGRL_EINVAL, "unknown representation");
  if (c.n_stats != n_stats_of(c.problem)) return fail(PCGRL_EINVAL, "n_stats does not match the problem");
  if (c.n_ctrl < 0 || c.n_ctrl > c.n_stats) return fail(PCGRL_EINVAL, "n_ctrl out of range");
  for (int j = 0; j < c.n_ctrl; j++)
    if (c.ctrl_idx[j] < 0 || c.ctrl_idx[j] >= c.n_stats || !(c.ctrl_range[j] > 0.0) || !c.has_trg[c.ctrl_idx[j]])
      return fail(PCGRL_EINVAL, "control metric: bad stat index, non-positive range, or a stat without a target");
  const int nt = n_tiles_of(c.problem);
  if (c.problem == PCGRL_PROB_MC3DMAZE) {
    if (c.ndim != 3) return fail(PCGRL_EINVAL, "minecraft_3D_maze needs ndim == 3");
    if (c.static_tiles || c.act_window[0] != 0)
      return fail(PCGRL_EUNSUPPORTED, "static tiles / act_window are only on the accelerated path for 2-D problems");
    const int Z = c.dims[0], Y = c.dims[1], X = c.dims[2];
    if (!m3_supported(Z, Y, X))
      return fail(PCGRL_EUNSUPPORTED, "minecraft_3D_maze: need 1 <= Z, Y, X <= 16 (the reference's stock map is 15 x 15 x 15)");
    if (c.representation == PCGRL_REP_WIDE) {  // wide_rep.py: the observation is the whole map, not a crop
      if (c.obs_window[0] != Z || c.obs_window[1] != Y || c.obs_window[2] != X)
        return fail(PCGRL_EINVAL, "wide representation needs obs_window == map_shape");
      lpe = 64;
      obs_chunks = 0;
      obs_bytes = (int64_t)Z * Y * X * 3;
      shape[0] = Z;
      shape[1] = Y;
      shape[2] = X;
      shape[3] = 3;  // AIR, DIRT, path overlay
      ndim = 4;
      return PCGRL_OK;
    }
    const int64_t cells = (int64_t)c.obs_window[0] * c.obs_window[1] * c.obs_window[2];
    if (cells < 1 || cells % 4) return fail(PCGRL_EUNSUPPORTED, "3-D obs_window volume must be a positive multiple of 4");
    lpe = 64;
    obs_chunks = 0;
    obs_bytes = cells * 4;
    shape[0] = c.obs_window[0];
    shape[1] = c.obs_window[1];
    shape[2] = c.obs_window[2];
    shape[3] = 4;  // out-of-bounds, AIR, DIRT, path overlay
    ndim = 4;
    return PCGRL_OK;
  }
  if (c.ndim != 2) return fail(PCGRL_EINVAL, "2-D problem needs ndim == 2");
  const int H = c.dims[0], W = c.dims[1];
  if (c.act_window[0] != 0 || c.act_window[1] != 0) {  // reps/wrappers.py:397-545; turtle / wide raise in the reference
    if (c.representation != PCGRL_REP_NARROW)
      return fail(PCGRL_EUNSUPPORTED, "act_window: the reference's MultiActionRepresentation only runs on narrow");
    if (c.act_window[0] < 1 || c.act_window[1] < 1 || c.act_window[0] > H || c.act_window[1] > W)
      return fail(PCGRL_EINVAL, "act_window must fit inside map_shape");
  }
  if (c.static_tiles) {  // reps/wrappers.py:234-376; wide raises in the reference (update() got an unexpected 'pos')
    if (c.representation == PCGRL_REP_WIDE)
      return fail(PCGRL_EUNSUPPORTED, "static tiles: the reference's StaticTileRepresentation does not run on wide");
    if (!(c.static_prob >= 0.0 && c.static_prob <= 1.0) || c.n_static_walls < 0)
      return fail(PCGRL_EINVAL, "static_prob must be in [0, 1] and n_static_walls >= 0");
    if (c.n_static_walls > 0 && (H < 3 || W < 3)) return fail(PCGRL_EINVAL, "static walls need a map of at least 3x3");
  } else if (c.static_prob != 0.0 || c.n_static_walls != 0) {
    return fail(PCGRL_EINVAL, "static_prob / n_static_walls need static_tiles = 1");
  }
  if (H < 1 || W < 1 || H > 64 || W > 64) return fail(PCGRL_EUNSUPPORTED, "map_shape: need 1 <= H <= 64, 1 <= W <= 64");
  if (c.problem == PCGRL_PROB_SOKOBAN && (W + 2 > SK_MAXDIM || H + 2 > SK_MAXDIM))
    return fail(PCGRL_EUNSUPPORTED, "sokoban: the device solver's level (map + border) is at most 64 x 64: need H, W <= 62");
  if (c.problem == PCGRL_PROB_SOKOBAN && (c.solver_power < 1 || c.solver_power > SK_MAX_POWER))
    return fail(PCGRL_EUNSUPPORTED, "sokoban: solver_power must be in [1, " + std::to_string(SK_MAX_POWER) +
                                        "] (the device solver's visited table and node ids are sized for that)");
  lpe = H <= 8 ? 8 : (H <= 16 ? 16 : (H <= 32 ? 32 : 64));
  if (W > 32 && lpe < 32) lpe = 32;  // the 64-bit row-mask kernels are built for 32 and 64 lanes per env: short maps leave rows idle
  if (c.representation == PCGRL_REP_WIDE) {
    if (c.obs_window[0] != H || c.obs_window[1] != W)
      return fail(PCGRL_EINVAL, "wide representation needs obs_window == map_shape (reference wrappers.py:140-150 reshape)");
    if (H != W) return fail(PCGRL_EUNSUPPORTED, "wide representation: the reference's transposed write needs a square map");
    obs_chunks = (W * nt + 15) / 16;  // rows that are not a multiple of 16 bytes take the byte-string store path
    obs_bytes = (int64_t)H * W * nt;
    shape[0] = H;
    shape[1] = W;
    shape[2] = nt;
    ndim = 3;
  } else {
    const int OH = c.obs_window[0], OW = c.obs_window[1], C = nt + 1 + (c.static_tiles ? 1 : 0);
    if (OH < 1 || OW < 1) return fail(PCGRL_EINVAL, "obs_window must be positive");
    obs_chunks = (OW * C + 15) / 16;
    obs_bytes = (int64_t)OH * OW * C;
    shape[0] = OH;
    shape[1] = OW;
    shape[2] = C;
    ndim = 3;
  }
  return PCGRL_OK;
}

static std::vector<JumpEntry> make_jump_table(int H, int W, int last = -1) {
  // A_k = a^k, G_k = 1 + a + ... + a^(k-1)  (mod 2^128); entry r = skip r*W draws, entry H = H*W draws
  // (or `last` draws when given: 3-D uses H = 64 lanes, W = cells per lane, last = n_cells)
  std::vector<JumpEntry> t(H + 1);
  U128 A{0, 1}, G{0, 0};
  const U128 a{PCG_MULT_HI, PCG_MULT_LO};
  int k = 0;
  for (int r = 0; r <= H; r++) {
    const int want = (r == H && last >= 0) ? last : r * W;
    if (want < k) {  // only for the final entry when last < H*W: restart
      A = U128{0, 1};
      G = U128{0, 0};
      k = 0;
    }
    while (k < want) {
      G = add128(mul128(G, a), U128{0, 1});
      A = mul128(A, a);
      k++;
    }
    t[r] = JumpEntry{A.hi, A.lo, G.hi, G.lo};
  }
  return t;
}

// observation bytes of one launch from which the 16x16 / 3-D kernels store non-temporally (profiles/r05_dev_traces.md)
static bool obs_nt_for(const pcgrl_engine *e, int64_t bytes_per_launch) {
  return e->obs_nt_mb > 0 && bytes_per_launch >= (int64_t)e->obs_nt_mb * 1000000;
}

// ---------------------------------------------------------------------------------------------- dispatch
// The kernels live in their own translation units (pcgrl_k_*.hip, see pcgrl_dispatch.h).
// step16: the engine has not switched step16_kernel off (pcgrl_engine::step16); only the stepping entry points pass it.
static hipError_t launch(KernelId id, int lpe, const Params &p, size_t lds, hipStream_t s, int cpl = 0, bool step16 = false) {
  const bool wide64 = p.cfg.dims[1] > 32;  // 64-bit row masks (W <= 64); validate() guarantees lpe >= 32 there
  if (id == K_STEP && step16 && step16_applies(p, lpe)) return launch_step16(p, lds, s);
  switch (p.cfg.problem) {
    case PCGRL_PROB_MC3DMAZE:
      if (p.cfg.representation == PCGRL_REP_TURTLE) return launch_3d_turtle(id, p, cpl, s);
      if (p.cfg.representation == PCGRL_REP_WIDE) return launch_3d_wide(id, p, cpl, s);
      // asynchronous stepping: the resumable kernels, the park records in Params::soko (with_budget)
      if (p.sk_budget > 0 && (id == K_STEP || id == K_RESET)) return launch_3d_async(id, p, cpl, s);
      return launch_3d(id, p, cpl, s);
    case PCGRL_PROB_BINARY: return wide64 ? launch_binary64(id, lpe, p, lds, s) : launch_binary32(id, lpe, p, lds, s);
    case PCGRL_PROB_ZELDA: return wide64 ? launch_zelda64(id, lpe, p, lds, s) : launch_zelda32(id, lpe, p, lds, s);
    default: return wide64 ? launch_sokoban64(id, lpe, p, lds, s) : launch_sokoban32(id, lpe, p, lds, s);
  }
}

// Every entry point runs on the engine's device whatever the caller's current device is, and leaves the caller's
// current device as it found it.
struct DeviceGuard {
  int prev = -1;
  hipError_t err;
  explicit DeviceGuard(int device) {
    err = hipGetDevice(&prev);
    if (err == hipSuccess && prev != device) err = hipSetDevice(device);
    else if (err == hipSuccess) prev = -1;  // nothing to restore
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};
#define ON_DEVICE(dev)                                                                            \
  DeviceGuard _guard(dev);                                                                        \
  if (_guard.err != hipSuccess) return fail(PCGRL_EHIP, std::string("hipSetDevice: ") + hipGetErrorString(_guard.err))

// ---------------------------------------------------------------------------------------------- engine-level kernels
namespace pcgrl {

__global__ __launch_bounds__(64) void queue_targets_kernel(Params p, const double *lo, const double *hi) {
  const int env = blockIdx.x * 64 + threadIdx.x;
  if (env >= p.n_envs || (p.mask != nullptr && p.mask[env] == 0)) return;
  double *q = p.trg_pending + (size_t)env * PCGRL_MAX_STATS * 2;
  for (int k = 0; k < p.cfg.n_stats; k++) {
    q[2 * k] = lo[(size_t)env * p.cfg.n_stats + k];
    q[2 * k + 1] = hi[(size_t)env * p.cfg.n_stats + k];
  }
  p.trg_flag[env] |= 1;  // (bits 1..: the env's resampling draw counter)
}

// pcgrl_reduce_episodes: sum of the per-env episode totals in a FIXED order (block b owns envs [b*chunk, (b+1)*chunk),
// the last block to finish adds the block partials in block order), so the result does not depend on timing.
constexpr int RED_BLOCKS = 64, RED_THREADS = 256, RED_W = 3 + PCGRL_MAX_STATS;
struct RedScratch {
  double part[RED_BLOCKS][RED_W];
  unsigned int ticket;
};
__global__ __launch_bounds__(RED_THREADS) void reduce_episodes_kernel(Params p, RedScratch *scr, double *out, int n_blocks, int clear) {
  __shared__ double sh[RED_THREADS / 64][RED_W];
  __shared__ bool last;
  const int chunk = (p.n_envs + n_blocks - 1) / n_blocks;
  const int lo = blockIdx.x * chunk, hi = min(p.n_envs, lo + chunk);
  double ret = 0.0;
  int64_t v[RED_W - 1];
  for (int k = 0; k < RED_W - 1; k++) v[k] = 0;
  for (int e = lo + (int)threadIdx.x; e < hi; e += RED_THREADS) {  // fixed env -> thread assignment
    EpAcc *A = &p.st[e].acc;
    ret += A->sum_return;
    v[0] += A->sum_len;
    v[1] += A->n;
    for (int k = 0; k < PCGRL_MAX_STATS; k++) v[2 + k] += A->sum_stats[k];
    if (clear) {
      A->sum_return = 0.0;
      A->sum_len = 0;
      A->n = 0;
      for (int k = 0; k < PCGRL_MAX_STATS; k++) A->sum_stats[k] = 0;
    }
  }
  // lanes -> wave (xor butterfly: a fixed tree), waves -> block (in wave order)
  double w[RED_W];
  w[0] = ret;
  for (int k = 1; k < RED_W; k++) w[k] = (double)v[k - 1];  // integer totals < 2^53: exact in double from here on
  for (int k = 0; k < RED_W; k++)
    for (int o = 32; o >= 1; o >>= 1) w[k] += __shfl_xor(w[k], o, 64);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0)
    for (int k = 0; k < RED_W; k++) sh[wave][k] = w[k];
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 0; k < RED_W; k++) {
      double s = 0.0;
      for (int i = 0; i < RED_THREADS / 64; i++) s += sh[i][k];
      scr->part[blockIdx.x][k] = s;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    last = atomicAdd(&scr->ticket, 1u) == (unsigned)n_blocks - 1u;
  }
  __syncthreads();
  if (!last) return;
  if (threadIdx.x == 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  __syncthreads();
  if (threadIdx.x < RED_W) {
    double s = 0.0;
    for (int b = 0; b < n_blocks; b++) s += __hip_atomic_load(&scr->part[b][threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // out = sum_return, sum_len, n_episodes, sum_final_stats[n_stats]
    if ((int)threadIdx.x < 3 + p.cfg.n_stats) out[threadIdx.x] = s;
  }
  if (threadIdx.x == 0) scr->ticket = 0;  // ready for the next call on the same stream
}

// small batches: one block, no cross-block hand-off (same fixed summation order: thread t owns envs t, t + 1024, ...;
// lanes -> wave by an xor butterfly, waves in wave order)
__global__ __launch_bounds__(1024) void reduce_episodes_small_kernel(Params p, double *out, int clear) {
  __shared__ double sh[16][RED_W];
  const int cols = 3 + p.cfg.n_stats;
  // The totals sit in the envs' second state line, which only episode ends touch: cold in HBM.  All of a thread's
  // counters are requested before the first is looked at, so their latencies overlap (n_envs <= 16384: 16 per thread).
  int64_t cnt[16];
#pragma unroll
  for (int i = 0; i < 16; i++) {
    const int e = (int)threadIdx.x + 1024 * i;
    cnt[i] = e < p.n_envs ? p.st[e].acc.n : 0;
  }
  double ret = 0.0;
  int64_t v[RED_W - 1];
  for (int k = 0; k < RED_W - 1; k++) v[k] = 0;
#pragma unroll
  for (int i = 0; i < 16; i++) {
    if (cnt[i] == 0) continue;  // nothing finished in this env since the last clearing call
    EpAcc *A = &p.st[(int)threadIdx.x + 1024 * i].acc;
    ret += A->sum_return;
    v[0] += A->sum_len;
    v[1] += cnt[i];
    for (int k = 0; k < PCGRL_MAX_STATS; k++) v[2 + k] += A->sum_stats[k];
    if (clear) {
      A->sum_return = 0.0;
      A->sum_len = 0;
      A->n = 0;
      for (int k = 0; k < PCGRL_MAX_STATS; k++) A->sum_stats[k] = 0;
    }
  }
  double w[RED_W];
  w[0] = ret;
  for (int k = 1; k < RED_W; k++) w[k] = (double)v[k - 1];
#pragma unroll
  for (int k = 0; k < RED_W; k++) {
    if (k >= cols) break;  // (uniform: only the problem's own statistics are summed)
    for (int o = 32; o >= 1; o >>= 1) w[k] += __shfl_xor(w[k], o, 64);
  }
  if ((threadIdx.x & 63) == 0)
    for (int k = 0; k < RED_W; k++) sh[threadIdx.x >> 6][k] = w[k];
  __syncthreads();
  if ((int)threadIdx.x < cols) {
    double s = 0.0;
    for (int i = 0; i < 16; i++) s += sh[i][threadIdx.x];
    out[threadIdx.x] = s;
  }
}

// pcgrl_sample_actions: action_space.sample() for every env.  Counter-based (entry i of draw c under seed s is a pure
// function of (s, c, i)); the draw counter lives in device memory and is advanced by the last block to finish, after every
// block has read it, so a launch captured in a HIP graph draws new actions at every replay.
struct SampleState {
  unsigned long long counter;
  unsigned int ticket;
};
__device__ __forceinline__ uint64_t mix64(uint64_t z) {  // splitmix64 finaliser
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
__global__ __launch_bounds__(256) void sample_actions_kernel(int32_t *out, int32_t n, uint32_t n_actions, uint64_t seed, SampleState *st) {
  __shared__ unsigned long long c_sh;
  if (threadIdx.x == 0) c_sh = __hip_atomic_load(&st->counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  const uint64_t c = c_sh;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    const uint64_t r = mix64(mix64(seed + c * 0x9e3779b97f4a7c15ull) ^ ((uint64_t)i * 0xd1b54a32d192ed03ull + 0x8cb92ba72f3d8dd7ull));
    out[i] = (int32_t)__umul64hi(r, (uint64_t)n_actions);  // floor(r * n / 2^64): bias < n / 2^64
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (atomicAdd(&st->ticket, 1u) == gridDim.x - 1u) {  // every block has read the counter before its ticket
      st->ticket = 0;
      __hip_atomic_store(&st->counter, c + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// pcgrl_get_rng_state / pcgrl_set_rng_state: [N][10] = rep state hi, lo, inc hi, lo; prob state hi, lo, inc hi, lo;
// representation-wrapper flags | has32 << 32, val32
__global__ __launch_bounds__(64) void rng_state_kernel(Params p, uint64_t *out, const uint64_t *in) {
  const int env = blockIdx.x * 64 + threadIdx.x;
  if (env >= p.n_envs || (p.mask != nullptr && p.mask[env] == 0)) return;
  RngState *r = &p.rng[env];
  uint32_t *xs = p.xstate ? p.xstate + (size_t)env * 4 : nullptr;
  if (out) {
    uint64_t *o = out + (size_t)env * 10;
    for (int k = 0; k < 4; k++) {
      o[k] = r->rep[k];
      o[4 + k] = r->prob[k];
    }
    o[8] = xs ? ((uint64_t)xs[0] | ((uint64_t)xs[1] << 32)) : 0ull;
    o[9] = xs ? (uint64_t)xs[2] : 0ull;
  }
  if (in) {
    const uint64_t *i = in + (size_t)env * 10;
    for (int k = 0; k < 4; k++) {
      r->rep[k] = i[k];
      r->prob[k] = i[4 + k];
    }
    if (xs) {
      xs[0] = (uint32_t)i[8];
      xs[1] = (uint32_t)(i[8] >> 32);
      xs[2] = (uint32_t)i[9];
    }
  }
}

// pcgrl_rollout in its two-kernel form: what the observe kernel needs of the state as it is BEFORE the call -- the tile planes,
// the first 32 bytes of the hot state line (position, counters, flags) and both RNG streams -- copied in 16-byte pieces
__global__ __launch_bounds__(256) void rollout_snapshot_kernel(const uint4 *planes, uint4 *s_planes, int64_t plane_q, const uint4 *st, uint4 *s_st,
                                                               const uint4 *rng, uint4 *s_rng, int32_t n_envs) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t n_st = (int64_t)n_envs * 2, n_rng = (int64_t)n_envs * (int64_t)(sizeof(RngState) / 16);
  if (i < plane_q) {
    s_planes[i] = planes[i];
  } else if (i < plane_q + n_st) {
    const int64_t j = i - plane_q, e = j >> 1, q = j & 1;
    s_st[e * (int64_t)(sizeof(EnvState) / 16) + q] = st[e * (int64_t)(sizeof(EnvState) / 16) + q];
  } else if (i < plane_q + n_st + n_rng) {
    const int64_t j = i - plane_q - n_st;
    s_rng[j] = rng[j];
  }
}

// pcgrl_env_busy: 1 = the env waits for a parked search (asynchronous stepping)
__global__ __launch_bounds__(256) void env_busy_kernel(Params p, uint8_t *out) {
  const int env = blockIdx.x * 256 + threadIdx.x;
  if (env < p.n_envs) out[env] = (p.st[env].flags & (ENV_PENDING_STEP | ENV_PENDING_STATS)) != 0 ? 1 : 0;
}

// pcgrl_import_state with a mask: rows (envs) of one state array, 4 bytes per thread
__global__ __launch_bounds__(256) void masked_rows_copy_kernel(uint32_t *dst, const uint32_t *src, int64_t words_per_env, int32_t n_envs,
                                                              const uint8_t *mask) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= words_per_env * n_envs) return;
  if (mask[i / words_per_env]) dst[i] = src[i];
}

}  // namespace pcgrl

// sokoban: while the device solver has been running in recent launches, step with one env per wavefront (every search gets
// a wave of its own); otherwise 64 / LPE envs share a wave.  The counter lives in host-mapped memory: reading it costs
// nothing and may lag a launch or two, which only delays the switch.
// sokoban: the solver's workspace pool is allocated at full size (one slot per four envs, sokoban_slots_for) the first time
// the solver has been SEEN running, not at pcgrl_create: until then at most SK_SLOTS_AT_CREATE slots exist (searches
// beyond the pool wait for a slot: speed, not results).  Synchronous (hipMalloc + a device synchronise), once per engine,
// never while `stream` is being captured; launches issued earlier (or frozen in a HIP graph) keep using the pool they were
// issued with, which stays allocated until pcgrl_destroy.
static int soko_pool_for(pcgrl_engine *h, Params &p, int want, hipStream_t stream, bool lazy = true) {
  if (!h->p.soko || h->soko_slots >= want) return PCGRL_OK;
  if (lazy && (!h->soko_lazy || h->soko_grow_failed)) return PCGRL_OK;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (stream != nullptr && (hipStreamIsCapturing(stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone)) {
    (void)hipGetLastError();
    return lazy ? PCGRL_OK : fail(PCGRL_EINVAL, "solver pool: `stream` is being captured (hipMalloc is not capturable)");
  }
  Params grown = h->p;
  int got = 0;
  const hipError_t e = sokoban_alloc(grown, h->allocs, want, &got, h->sk_ws, h->sk_park);
  if (e == hipSuccess) {
    h->p.soko = grown.soko;
    p.soko = grown.soko;
    h->soko_slots = got;
    h->soko_grow_failed = false;
    h->soko_grow_msg.clear();
    return PCGRL_OK;
  }
  (void)hipGetLastError();
  // (out of memory: sokoban_alloc handed back what it had taken; the engine keeps the pool it has -- searches beyond it wait
  // for a slot: speed, not results -- and does not try again by itself; pcgrl_solver_pool_slots reports it,
  // pcgrl_reserve_solver_pool retries on request)
  h->soko_grow_failed = true;
  h->soko_grow_msg = std::string("solver pool: growing from ") + std::to_string(h->soko_slots) + " to " + std::to_string(want) +
                     " slots failed: " + hipGetErrorString(e);
  return lazy ? PCGRL_OK : fail(PCGRL_EHIP, h->soko_grow_msg);
}

static void soko_pool_lazy(pcgrl_engine *h, Params &p, hipStream_t stream) {
  if (!h->seen_host || h->soko_slots >= sokoban_slots_for(h->p.n_envs)) return;
  if (*(volatile int32_t *)h->seen_host != 0) soko_pool_for(h, p, sokoban_slots_for(h->p.n_envs), stream);
}

static void choose_spread(pcgrl_engine *h, Params &p) {
  if (!h->seen_host || h->p.ext) return;
  static const int force = getenv("PCGRL_FORCE_SPREAD") ? atoi(getenv("PCGRL_FORCE_SPREAD")) : 0;  // development: 1 = spread, 2 = + helpers
  if (force) {
    p.spread = 1;
    p.sk_helpers = force == 2 ? 3 : 0;
    return;
  }
  // (a workgroup per env only pays while the launch is short of wavefronts: at 32 768 envs it is 32 768 workgroups of eight
  // waves and the step launch goes from 10 to 74 us)
  if (h->p.n_envs > 8192) return;
  const int32_t seen = *(volatile int32_t *)h->seen_host;
  if (seen != h->seen_last) {
    h->seen_last = seen;
    h->spread_left = 16;
  }
  if (h->spread_left > 0) {
    h->spread_left--;
    p.spread = 1;
    // ... and three more wavefronts per env run the A* stages next to the BFS stage, when their heaps fit the CU's 160 KiB
    // of LDS next to the observation staging rows (they do for every window up to about 2 x 62 cells per row)
    p.sk_helpers = h->lds_bytes + 3 * (size_t)SK_HELPER_LDS + 4096 <= 160 * 1024 ? 3 : 0;
  }
}

// ---------------------------------------------------------------------------------------------- C ABI
extern "C" {

const char *pcgrl_last_error(void) { return g_err.c_str(); }
const char *pcgrl_version(void) { return "pcgrl_amd 0.7.0 (gfx950)"; }

int pcgrl_create(const pcgrl_config *cfg, int32_t n_envs, int32_t device, pcgrl_handle *out) {
  if (!cfg || !out || n_envs < 1) return fail(PCGRL_EINVAL, "pcgrl_create: bad arguments");
  int lpe = 16, obs_chunks = 0, ndim = 0;
  int64_t obs_bytes = 0;
  int32_t shape[4] = {0, 0, 0, 0};
  int rc = validate(*cfg, lpe, obs_bytes, obs_chunks, shape, ndim);
  if (rc) return rc;
  ON_DEVICE(device);
  pcgrl_engine *e = new pcgrl_engine();
  {
    const char *f = getenv("PCGRL_ROLLOUT_KERNEL");
    if (f != nullptr && (f[0] == '0' || f[0] == '1')) e->rollout_form = f[0] - '0';
    if (getenv("PCGRL_OBS_NT_MB")) e->obs_nt_mb = atol(getenv("PCGRL_OBS_NT_MB"));
    if (getenv("PCGRL_ROLLOUT_EPW")) e->rollout_epw = atoi(getenv("PCGRL_ROLLOUT_EPW"));
    const char *s16 = getenv("PCGRL_STEP16");
    if (s16 != nullptr && s16[0] == '0') e->step16 = false;
  }
  e->device = device;
  e->lpe = lpe;
  e->obs_bytes = obs_bytes;
  e->obs_ndim = ndim;
  memcpy(e->obs_shape, shape, sizeof(shape));
  Params &p = e->p;
  memset(&p, 0, sizeof(p));
  p.cfg = *cfg;
  {  // integer form of the static targets (get_loss): statistics are far below 2^29 in magnitude, so infinite bounds clamp there
    bool integral = true;
    for (int k = 0; k < PCGRL_MAX_STATS; k++) {
      const double lo = cfg->trg_lo[k], hi = cfg->trg_hi[k];
      const int32_t big = 1 << 29;
      int32_t lo_i = 0, hi_i = 0;
      if (k < cfg->n_stats && cfg->has_trg[k]) {
        if (lo != lo || hi != hi || lo > hi) integral = false;  // (NaN, or an empty interval: the float64 form decides)
        else {
          if (lo <= -(double)big) lo_i = -big;
          else if (lo >= (double)big) lo_i = big;
          else if (lo == (double)(int32_t)lo) lo_i = (int32_t)lo;
          else integral = false;
          if (hi >= (double)big) hi_i = big;
          else if (hi <= -(double)big) hi_i = -big;
          else if (hi == (double)(int32_t)hi) hi_i = (int32_t)hi;
          else integral = false;
        }
      }
      p.trg_lo_i[k] = lo_i;
      p.trg_hi_i[k] = hi_i;
    }
    p.int_targets = integral ? 1 : 0;
  }
  p.n_envs = n_envs;
  p.n_tiles = n_tiles_of(cfg->problem);
  const bool is3d = cfg->problem == PCGRL_PROB_MC3DMAZE;
  p.n_cells = cfg->dims[0] * cfg->dims[1] * (is3d ? cfg->dims[2] : 1);
  p.obs_chunks = obs_chunks;
  if (is3d) m3_edge_masks_host(cfg->dims[1], cfg->dims[2], p.m3_notx0, p.m3_notxl);
  p.ext = (!is3d && (cfg->static_tiles || cfg->act_window[0] > 0)) ? 1 : 0;
  p.n_act = (!is3d && cfg->act_window[0] > 0) ? cfg->act_window[0] * cfg->act_window[1] : 1;
  // one padded observation row per lane + the OOB row (+ 2 rows per env of the wave with the static_builds plane)
  // (+ 64 bytes per env of the wave: the observe wave's copy of the RNG streams, see step_kernel)
  e->lds_bytes = (size_t)(obs_chunks * 16 + 32) * (65 + (cfg->static_tiles ? 16 : 0)) + 64 * 8;  // (+32: lds_row_stride may add a chunk)
  {
    // Cropped windows whose rows are whole 16-byte chunks, off the compile-time 16x16 / 32x32 point, without the static
    // tiles' extra channel: the general kernels compute the observation chunks from one code byte per cell
    // (encode_obs_codes) -- per env H rows of W + 20 bytes (rounded to 16) instead of H one-hot rows
    const int Hc = cfg->dims[0], Wc = cfg->dims[1], OWc = cfg->obs_window[1], Cc = p.n_tiles + 1;
    const bool fast_cfg = Hc == 16 && Wc == 16 && cfg->obs_window[0] == 32 && OWc == 32;
    p.obs16 = (!is3d && fast_cfg) ? 1 : 0;
    // non-temporal observation stores where a launch writes far more than the 256 MB last-level cache holds (store_obs16_nt)
    if ((p.obs16 || is3d) && obs_nt_for(e, (int64_t)n_envs * obs_bytes)) p.obs16 |= 2;  // (3-D: bit 1 alone)
    // (only where the one-hot rows are what limits occupancy: at 13 KB per workgroup -- binary 32 x 32 -- the rows are
    // cheaper: 14.0 vs 15.6 us per launch; at 26 KB -- binary 64 x 64 -- 67 vs 47.5; at 38 KB -- zelda 32 x 32 -- 44 vs 27.6)
    if (!is3d && cfg->representation != PCGRL_REP_WIDE && !cfg->static_tiles && !fast_cfg && (OWc * Cc) % 16 == 0 &&
        e->lds_bytes > 20000) {
      const int rs = (Wc + 8 + 12 + 15) & ~15;
      const int epw = 64 / lpe;
      p.obs_codes = rs;
      e->lds_bytes = (size_t)epw * Hc * rs + rs + (size_t)Cc * 48 + 64 * 8;
      e->lds_bytes = (e->lds_bytes + 15) & ~(size_t)15;
    }
  }
  p.lds_pair_bytes = (int32_t)e->lds_bytes;
  e->cpl = is3d ? (p.n_cells + 63) / 64 : 0;
  const int H = cfg->dims[0], W = cfg->dims[1];
  auto dalloc = [&](void **ptr, size_t bytes) -> hipError_t {
    hipError_t err = hipMalloc(ptr, bytes);
    if (err == hipSuccess) {
      e->allocs.push_back(*ptr);
      err = hipMemset(*ptr, 0, bytes);
    }
    return err;
  };
#define CREATE_CHK(x)                                                                                \
  do {                                                                                               \
    hipError_t _e = (x);                                                                             \
    if (_e != hipSuccess) {                                                                          \
      pcgrl_destroy(e);                                                                              \
      return fail(PCGRL_EHIP, std::string(#x) + ": " + hipGetErrorString(_e));                       \
    }                                                                                                \
  } while (0)
  if (is3d) {
    // one record per env: tile bits, overlay bits, column masks, cached start-plane results, move table (M3Lay)
    CREATE_CHK(dalloc(&p.planes, (size_t)n_envs * m3_layout(cfg->dims[0], cfg->dims[1], cfg->dims[2]).rec_words * sizeof(uint32_t)));
  } else
    CREATE_CHK(dalloc(&p.planes, (size_t)n_envs * ROW_WORDS * H * (W > 32 ? sizeof(uint64_t) : sizeof(uint32_t))));
  CREATE_CHK(dalloc((void **)&p.st, (size_t)n_envs * sizeof(EnvState)));
  CREATE_CHK(dalloc((void **)&p.rng, (size_t)n_envs * sizeof(RngState)));
  CREATE_CHK(dalloc((void **)&e->red, sizeof(RedScratch)));
  CREATE_CHK(dalloc((void **)&e->sample, sizeof(SampleState)));
  // [0..3] error flags; from int 64 on: per-workgroup phase-timing accumulators (PCGRL_PHASE_TIMING builds)
  CREATE_CHK(dalloc((void **)&p.err, sizeof(int32_t) * 64 + sizeof(uint64_t) * 8 * (size_t)(n_envs + 64)));
  std::vector<JumpEntry> jt = is3d ? make_jump_table(64, e->cpl, p.n_cells) : make_jump_table(H, W);
  JumpEntry *djt = nullptr;
  CREATE_CHK(dalloc((void **)&djt, jt.size() * sizeof(JumpEntry)));
  CREATE_CHK(hipMemcpy(djt, jt.data(), jt.size() * sizeof(JumpEntry), hipMemcpyHostToDevice));
  p.jump = djt;
  if (p.ext) {
    const size_t mbytes = W > 32 ? sizeof(uint64_t) : sizeof(uint32_t);
    const int nb = p.n_tiles <= 2 ? 1 : 3;
    CREATE_CHK(dalloc(&p.xplanes, (size_t)n_envs * (1 + nb) * H * mbytes));
    CREATE_CHK(dalloc((void **)&p.xstate, (size_t)n_envs * 4 * sizeof(uint32_t)));
    std::vector<JumpEntry> jb = make_jump_table(H + 2, W + 2);
    JumpEntry *djb = nullptr;
    CREATE_CHK(dalloc((void **)&djb, jb.size() * sizeof(JumpEntry)));
    CREATE_CHK(hipMemcpy(djb, jb.data(), jb.size() * sizeof(JumpEntry), hipMemcpyHostToDevice));
    p.jump_b = djb;
  }
  if (cfg->problem == PCGRL_PROB_SOKOBAN) {
    CREATE_CHK(sokoban_alloc(p, e->allocs, std::min(SK_SLOTS_AT_CREATE, sokoban_slots_for(n_envs)), &e->soko_slots));
    CREATE_CHK(hipHostMalloc((void **)&e->seen_host, sizeof(int32_t), hipHostMallocMapped));
    *e->seen_host = 0;
    CREATE_CHK(hipHostGetDevicePointer((void **)&p.solver_seen, e->seen_host, 0));
  }
  if (cfg->n_ctrl > 0) {  // controllable mode: per-env targets, initialised with the static ones
    std::vector<double> init((size_t)n_envs * PCGRL_MAX_STATS * 2, 0.0);
    for (int i = 0; i < n_envs; i++)
      for (int k = 0; k < PCGRL_MAX_STATS; k++) {
        init[((size_t)i * PCGRL_MAX_STATS + k) * 2] = cfg->trg_lo[k];
        init[((size_t)i * PCGRL_MAX_STATS + k) * 2 + 1] = cfg->trg_hi[k];
      }
    // (the engine-wide resampling record sits right in front of the targets: TrgResample, pcgrl_common.h)
    uint8_t *trg_block = nullptr;
    CREATE_CHK(dalloc((void **)&trg_block, sizeof(TrgResample) + init.size() * sizeof(double)));
    p.trg = (double *)(trg_block + sizeof(TrgResample));
    CREATE_CHK(dalloc((void **)&p.trg_pending, init.size() * sizeof(double)));
    CREATE_CHK(dalloc((void **)&p.trg_flag, (size_t)n_envs * sizeof(int32_t)));
    CREATE_CHK(hipMemcpy(p.trg, init.data(), init.size() * sizeof(double), hipMemcpyHostToDevice));
  }
#undef CREATE_CHK
  {
    const size_t plane_bytes = is3d ? (size_t)m3_layout(cfg->dims[0], cfg->dims[1], cfg->dims[2]).rec_words * sizeof(uint32_t)
                                    : (size_t)ROW_WORDS * H * (W > 32 ? sizeof(uint64_t) : sizeof(uint32_t));
    e->state_arrays.push_back({p.planes, plane_bytes});
    e->state_arrays.push_back({p.st, sizeof(EnvState)});
    e->state_arrays.push_back({p.rng, sizeof(RngState)});
    if (p.xplanes) {
      const size_t mbytes = W > 32 ? sizeof(uint64_t) : sizeof(uint32_t);
      e->state_arrays.push_back({p.xplanes, (size_t)(1 + (p.n_tiles <= 2 ? 1 : 3)) * H * mbytes});
      e->state_arrays.push_back({p.xstate, 4 * sizeof(uint32_t)});
    }
    if (p.trg) {
      e->state_arrays.push_back({p.trg, PCGRL_MAX_STATS * 2 * sizeof(double)});
      e->state_arrays.push_back({p.trg_pending, PCGRL_MAX_STATS * 2 * sizeof(double)});
      e->state_arrays.push_back({p.trg_flag, sizeof(int32_t)});
    }
  }
  // the two-kernel rollout exists for the compile-time 16x16 kernels in plain mode (no wrappers, no control metrics)
  if (!is3d && H == 16 && W == 16 && !p.ext && cfg->n_ctrl == 0 &&
      (cfg->representation == PCGRL_REP_WIDE || (cfg->obs_window[0] == 32 && cfg->obs_window[1] == 32))) {
    hipError_t he = hipStreamCreateWithFlags(&e->side, hipStreamNonBlocking);
    if (he == hipSuccess) he = hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming);
    if (he == hipSuccess) he = hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming);
    if (he == hipSuccess) he = dalloc(&e->snap_planes, (size_t)n_envs * ROW_WORDS * H * sizeof(uint32_t));
    if (he == hipSuccess) he = dalloc((void **)&e->snap_st, (size_t)n_envs * sizeof(EnvState));
    if (he == hipSuccess) he = dalloc((void **)&e->snap_rng, (size_t)n_envs * sizeof(RngState));
    if (he != hipSuccess) {
      pcgrl_destroy(e);
      return fail(PCGRL_EHIP, std::string("pcgrl_create (rollout side stream / snapshot): ") + hipGetErrorString(he));
    }
    e->split_ok = true;
    int cus = 0;
    rollout_resident_per_cu = 0;
    if (launch(K_ROLLOUT_RESIDENT, e->lpe, e->p, e->lds_bytes, nullptr, e->cpl) == hipSuccess &&
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, e->device) == hipSuccess)
      e->two_role_resident = (int64_t)rollout_resident_per_cu * cus;
    // (development / tests: PCGRL_ROLLOUT_RESIDENT=<workgroups> stands in for the device's figure, so that small batches take
    // the forms of large ones)
    if (getenv("PCGRL_ROLLOUT_RESIDENT")) e->two_role_resident = atol(getenv("PCGRL_ROLLOUT_RESIDENT"));
    (void)hipGetLastError();
  }
  {
    const hipError_t he = hipHostMalloc((void **)&e->hdr_host, 256, hipHostMallocDefault);
    if (he != hipSuccess) {
      pcgrl_destroy(e);
      return fail(PCGRL_EHIP, std::string("hipHostMalloc (state header): ") + hipGetErrorString(he));
    }
    memset(e->hdr_host, 0, 256);
    state_header_build(e);
  }
  *out = e;
  // default seeding: env i gets seed i (callers normally call pcgrl_seed)
  std::vector<uint64_t> seeds(n_envs);
  for (int i = 0; i < n_envs; i++) seeds[i] = (uint64_t)i;
  return pcgrl_seed(e, seeds.data());
}

void pcgrl_destroy(pcgrl_handle h) {
  if (!h) return;
  DeviceGuard guard(h->device);
  if (h->seen_host) (void)hipHostFree(h->seen_host);
  if (h->hdr_host) (void)hipHostFree(h->hdr_host);
  if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
  if (h->ev_join) (void)hipEventDestroy(h->ev_join);
  if (h->side) (void)hipStreamDestroy(h->side);
  for (void *a : h->allocs) (void)hipFree(a);
  delete h;
}

int pcgrl_seed(pcgrl_handle h, const uint64_t *seeds) {
  if (!h || !seeds) return fail(PCGRL_EINVAL, "pcgrl_seed: bad arguments");
  ON_DEVICE(h->device);
  std::vector<RngState> r(h->p.n_envs);
  for (int i = 0; i < h->p.n_envs; i++) {
    pcg64_seed_state(seeds[i], r[i].rep);
    memcpy(r[i].prob, r[i].rep, sizeof(r[i].rep));  // envs/pcgrl_env.py:142-146: same seed for both streams
  }
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(h->p.rng, r.data(), r.size() * sizeof(RngState), hipMemcpyHostToDevice));
  // seeding a numpy bit generator drops the spare 32 bits of its last draw
  if (h->p.xstate) HIPCHK(hipMemset(h->p.xstate, 0, (size_t)h->p.n_envs * 4 * sizeof(uint32_t)));
  if (h->ma_on) HIPCHK(hipMemset2D(h->ma.side + 1, 4 * sizeof(uint32_t), 0, 2 * sizeof(uint32_t), (size_t)h->p.n_envs));
  return PCGRL_OK;
}

// the per-launch parameters of asynchronous stepping: the budget and, on a 3-D maze engine, the park records (Params::soko is
// null there otherwise and stays null in h->p: the engine reads h->p.soko as "this engine has the sokoban solver")
static void with_budget(const pcgrl_engine *h, Params &p) {
  p.sk_budget = h->sk_budget;
  if (h->sk_budget > 0 && h->a3_park) p.soko = h->a3_park;
}
static bool async_capable(const pcgrl_engine *h) {
  return h->p.soko != nullptr || (h->p.cfg.problem == PCGRL_PROB_MC3DMAZE && h->p.cfg.representation == PCGRL_REP_NARROW);
}

// the single-agent stepping entry points on an engine that pcgrl_ma_attach has made a multi-agent one
#define NOT_ATTACHED(h, what)                                                                                             \
  if ((h)->ma_on)                                                                                                         \
  return fail(PCGRL_EINVAL, std::string(what) + ": the engine steps several agents (pcgrl_ma_attach): use the pcgrl_ma_* entry " \
                                                "points of pcgrl_amd_multiagent.h")

int pcgrl_reset(pcgrl_handle h, const uint8_t *d_mask, const uint8_t *d_init_grids, const int32_t *d_init_pos, void *stream) {
  if (!h) return fail(PCGRL_EINVAL, "pcgrl_reset: null handle");
  NOT_ATTACHED(h, "pcgrl_reset");
  ON_DEVICE(h->device);
  Params p = h->p;
  soko_pool_lazy(h, p, (hipStream_t)stream);
  p.mask = d_mask;
  p.init_grids = d_init_grids;
  p.init_pos = d_init_pos;
  with_budget(h, p);  // (asynchronous stepping: a search may stay parked, the env busy)
  HIPCHK(launch(K_RESET, h->lpe, p, h->lds_bytes, (hipStream_t)stream, h->cpl));
  if (d_mask == nullptr) h->maybe_stale = false;
  return PCGRL_OK;
}

#define NOT_WITH_BUDGET(h, what)                                                                                         \
  if ((h)->sk_budget > 0)                                                                                                \
  return fail(PCGRL_EINVAL, std::string(what) + ": a solver budget is set (pcgrl_set_solver_budget): envs may be busy, which only " \
                                                "pcgrl_step_ready can report")

int pcgrl_step(pcgrl_handle h, const int32_t *d_actions, int32_t auto_reset, uint8_t *d_obs, float *d_reward, uint8_t *d_done,
               int32_t *d_stats, void *stream) {
  if (!h || !d_actions) return fail(PCGRL_EINVAL, "pcgrl_step: bad arguments");
  NOT_WITH_BUDGET(h, "pcgrl_step");
  NOT_ATTACHED(h, "pcgrl_step");
  ON_DEVICE(h->device);
  Params p = h->p;
  p.no_fast = h->maybe_stale ? 1 : 0;
  soko_pool_lazy(h, p, (hipStream_t)stream);
  choose_spread(h, p);
  p.actions = d_actions;
  p.auto_reset = auto_reset;
  p.obs = d_obs;
  p.reward = d_reward;
  p.done = d_done;
  p.stats_out = d_stats;
  HIPCHK(launch(K_STEP, h->lpe, p, h->lds_bytes, (hipStream_t)stream, h->cpl, h->step16));
  return PCGRL_OK;
}

int pcgrl_step_seq(pcgrl_handle h, const int32_t *d_action_rows, int64_t row_stride, int32_t n_rows, int32_t first_row,
                   int32_t n_steps, int32_t auto_reset, uint8_t *d_obs, float *d_reward, uint8_t *d_done, int32_t *d_stats,
                   void *stream) {
  if (!h || !d_action_rows || n_rows < 1 || n_steps < 0 || first_row < 0 || row_stride < 0)
    return fail(PCGRL_EINVAL, "pcgrl_step_seq: bad arguments");
  for (int32_t k = 0; k < n_steps; k++) {
    const int rc = pcgrl_step(h, d_action_rows + (size_t)((first_row + k) % n_rows) * (size_t)row_stride, auto_reset, d_obs, d_reward,
                              d_done, d_stats, stream);
    if (rc != PCGRL_OK) return rc;
  }
  return PCGRL_OK;
}

int pcgrl_step_ex(pcgrl_handle h, const int32_t *d_actions, int32_t auto_reset, uint8_t *d_obs, float *d_reward,
                  double *d_reward64, uint8_t *d_done, int32_t *d_stats, float *d_ctrl_obs, void *stream) {
  if (!h || !d_actions) return fail(PCGRL_EINVAL, "pcgrl_step_ex: bad arguments");
  NOT_WITH_BUDGET(h, "pcgrl_step_ex");
  NOT_ATTACHED(h, "pcgrl_step_ex");
  ON_DEVICE(h->device);
  if (d_ctrl_obs && h->p.cfg.n_ctrl == 0) return fail(PCGRL_EINVAL, "pcgrl_step_ex: d_ctrl_obs needs cfg.n_ctrl > 0");
  Params p = h->p;
  p.no_fast = h->maybe_stale ? 1 : 0;
  soko_pool_lazy(h, p, (hipStream_t)stream);
  choose_spread(h, p);
  p.actions = d_actions;
  p.auto_reset = auto_reset;
  p.obs = d_obs;
  p.reward = d_reward;
  p.reward64 = d_reward64;
  p.done = d_done;
  p.stats_out = d_stats;
  p.ctrl_obs = d_ctrl_obs;
  HIPCHK(launch(K_STEP, h->lpe, p, h->lds_bytes, (hipStream_t)stream, h->cpl, h->step16));
  return PCGRL_OK;
}

// pcgrl_rollout where the rollout kernel loses to stepping.  That kernel keeps the env in registers and does both roles on
// one wave: it pays where a step is short or its launches wait for their slowest env (16-row maps: 3.5 vs 5.9 us per step
// for binary; the 3-D mazes, whose waves then advance independently: 10 vs 21 us at 7^3, 112 vs 126 at 15^3 over the same
// steps) and costs on the 2-D maps of more than 16 rows, where the observation is large (or computed chunk by chunk from tile
// codes, Params::obs_codes) and wants a wave of its own next to the statistics -- zelda_big 49.7 vs 34 us per step,
// zelda_bigger 217 vs 126, binary_bigger 60 vs 51, binary_big 16.7 vs 15.5 (bench lines of rounds 4 / 5).  There the call
// issues its n_steps as step launches: same results by the entry point's own definition.
static bool rollout_as_steps(const pcgrl_engine *h) {
  if (h->rollout_form >= 0) return h->rollout_form == 0;  // (pcgrl_set_rollout_form; PCGRL_ROLLOUT_KERNEL at pcgrl_create)
  // (maps of more than 16 rows without tile codes, e.g. binary_big 32 x 32: 16.7 us per step in one launch -- its kernel sits at
  // 256 VGPRs -- against 15.0-15.5 as step launches)
  // lpe > 16: a 2-D map of more than 16 rows OR more than 32 columns (64-bit row masks run on 32 / 64 lanes per env)
  return h->p.cfg.problem != PCGRL_PROB_MC3DMAZE && (h->p.obs_codes > 0 || h->lpe > 16);
}

int32_t pcgrl_rollout_is_one_launch(pcgrl_handle h) { return h ? (rollout_as_steps(h) ? 0 : 1) : -1; }  // (1 also for the two-kernel form)

int pcgrl_set_rollout_form(pcgrl_handle h, int32_t form) {
  if (!h || form < -1 || form > 2)
    return fail(PCGRL_EINVAL, "pcgrl_set_rollout_form: form must be -1 (by shape), 0 (step launches), 1 (one kernel) or 2 (two kernels)");
  if (form == 2 && !h->split_ok)
    return fail(PCGRL_EUNSUPPORTED, "pcgrl_set_rollout_form(2): the two-kernel rollout exists for 16 x 16 maps with the default window, plain mode");
  h->rollout_form = form;
  return PCGRL_OK;
}

int pcgrl_rollout_ex(pcgrl_handle h, const int32_t *d_actions, int32_t n_steps, int32_t auto_reset, uint8_t *d_obs,
                     int32_t obs_last_only, float *d_reward, double *d_reward64, uint8_t *d_done, int32_t *d_stats, float *d_ctrl_obs,
                     void *stream) {
  if (!h || !d_actions || n_steps < 1) return fail(PCGRL_EINVAL, "pcgrl_rollout: bad arguments");
  NOT_WITH_BUDGET(h, "pcgrl_rollout");
  NOT_ATTACHED(h, "pcgrl_rollout");
  if (d_ctrl_obs && h->p.cfg.n_ctrl == 0) return fail(PCGRL_EINVAL, "pcgrl_rollout_ex: d_ctrl_obs needs cfg.n_ctrl > 0");
  if (rollout_as_steps(h)) {
    const size_t N = (size_t)h->p.n_envs;
    for (int32_t k = 0; k < n_steps; k++) {
      const bool last = k == n_steps - 1;
      uint8_t *obs_k = d_obs == nullptr ? nullptr : (obs_last_only ? (last ? d_obs : nullptr) : d_obs + (size_t)k * N * (size_t)h->obs_bytes);
      const int rc = pcgrl_step_ex(h, d_actions + (size_t)k * N * (size_t)h->p.n_act, auto_reset, obs_k, d_reward ? d_reward + (size_t)k * N : nullptr,
                                   d_reward64 ? d_reward64 + (size_t)k * N : nullptr, d_done ? d_done + (size_t)k * N : nullptr,
                                   d_stats ? d_stats + (size_t)k * N * (size_t)h->p.cfg.n_stats : nullptr, last ? d_ctrl_obs : nullptr, stream);
      if (rc != PCGRL_OK) return rc;
    }
    return PCGRL_OK;
  }
  ON_DEVICE(h->device);
  Params p = h->p;
  p.no_fast = h->maybe_stale ? 1 : 0;
  soko_pool_lazy(h, p, (hipStream_t)stream);
  p.actions = d_actions;
  p.n_steps = n_steps;
  p.spread = 0;
  // The roles as kernels of their own (16 x 16 compile-time kernels, plain mode; not while statistics may be stale and not in the
  // controllable-output form), see rollout_kernel's ROLE.  The simulate kernel takes 103 / 114 / 157 VGPRs (binary / zelda /
  // sokoban) against the two-role kernel's 224 / 323 / 335, whose workgroups are all resident at once only up to
  // two_role_resident of them (binary 1024 = 4096 envs, zelda and sokoban 512 = 2048 envs); beyond that it runs in rounds and the
  // roles are better off apart.  By shape (form -1), measured in profiles/r06_dev_traces.md section 3:
  //   no observation asked for    the simulate kernel alone, always (never slower; binary-narrow 16 384 envs 9.3 -> 6.1 us per
  //                               step, zelda-turtle 4096 envs 4.4 -> 2.1)
  //   only the last observation   when the two-role kernel would run in rounds: the simulate kernel, then pcgrl_observe's kernel
  //                               on the state it left, same stream (zelda-turtle 4096 envs 4.2 -> 2.2; one launch more per call,
  //                               which costs binary-narrow at 4096 envs 4.04 -> 4.32 at 8 steps per call: not below the bound)
  //   every observation           when the two-role kernel would run in rounds and the call has >= 16 steps: both kernels, the
  //                               observe one on the engine's side stream from a snapshot of the pre-call state (form 2).
  //                               Snapshot + fork + join cost 15-25 us per CALL (binary-narrow 4096 envs, 8 steps: 5.97 vs 4.10 us
  //                               per step; 64 steps: 3.42 vs 3.21), the gain is the simulate role's occupancy (binary-narrow
  //                               8192 envs 7.86 -> 5.87, zelda-turtle 4096 envs 8.64 -> 7.51, 16 384 envs 33.4 -> 28.4).
  // Fewer envs per simulate wave (PCGRL_ROLLOUT_EPW) do NOT pay: a wave64 instruction occupies its SIMD for four cycles whatever
  // the number of active lanes, and two waves per SIMD already issue back to back (binary-narrow, 1 / 2 envs per wave: 4.59 / 3.54).
  const bool roles_ok = h->split_ok && !h->maybe_stale && d_reward64 == nullptr && d_ctrl_obs == nullptr && h->rollout_form != 1;
  const int64_t two_role_wgs = ((int64_t)h->p.n_envs + 64 / h->lpe - 1) / (64 / h->lpe);
  const bool in_rounds = h->two_role_resident > 0 && two_role_wgs > h->two_role_resident;
  const bool split = roles_ok && d_obs != nullptr && (h->rollout_form == 2 || (in_rounds && !obs_last_only && n_steps >= 16));
  const bool sim_then_observe = roles_ok && !split && d_obs != nullptr && obs_last_only && in_rounds;
  const bool sim_only = (roles_ok && d_obs == nullptr) || sim_then_observe;
  if (h->p.cfg.problem != PCGRL_PROB_MC3DMAZE) {
    const int full = 64 / h->lpe;
    int epw = h->rollout_epw;
    if (epw > full) epw = full;
    p.spread = epw > 0 ? epw : 0;
  }
  p.auto_reset = auto_reset;
  p.obs = d_obs;
  p.obs_last_only = obs_last_only;
  p.obs_env_bytes = h->obs_bytes;
  // (a rollout that keeps every step's observation writes n_steps times a step launch's bytes: 805 MB for 64 steps of 4096 binary envs)
  if ((p.obs16 || h->p.cfg.problem == PCGRL_PROB_MC3DMAZE) && d_obs && !obs_last_only && obs_nt_for(h, (int64_t)n_steps * h->p.n_envs * h->obs_bytes)) p.obs16 |= 2;
  p.reward = d_reward;
  p.reward64 = d_reward64;
  p.done = d_done;
  p.stats_out = d_stats;
  p.ctrl_obs = d_ctrl_obs;
  if (split || sim_only) {
    hipStream_t s0 = (hipStream_t)stream;
    if (split) {  // the observe kernel: from a snapshot of the pre-call state, on the side stream
      const int64_t plane_q = (int64_t)h->p.n_envs * ROW_WORDS * h->p.cfg.dims[0] * (int64_t)sizeof(uint32_t) / 16;
      const int64_t total = plane_q + (int64_t)h->p.n_envs * 2 + (int64_t)h->p.n_envs * (int64_t)(sizeof(RngState) / 16);
      hipLaunchKernelGGL(rollout_snapshot_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s0, (const uint4 *)h->p.planes,
                         (uint4 *)h->snap_planes, plane_q, (const uint4 *)h->p.st, (uint4 *)h->snap_st, (const uint4 *)h->p.rng, (uint4 *)h->snap_rng,
                         h->p.n_envs);
      HIPCHK(hipGetLastError());
      HIPCHK(hipEventRecord(h->ev_fork, s0));
      HIPCHK(hipStreamWaitEvent(h->side, h->ev_fork, 0));
      Params po = p;
      po.planes = h->snap_planes;
      po.st = h->snap_st;
      po.rng = h->snap_rng;
      po.spread = 0;
      po.reward = nullptr;
      po.done = nullptr;
      po.stats_out = nullptr;
      HIPCHK(launch(K_ROLLOUT_OBS, h->lpe, po, h->lds_bytes, h->side, h->cpl));
    }
    Params ps = p;
    ps.obs = nullptr;
    HIPCHK(launch(K_ROLLOUT_SIM, h->lpe, ps, 0, s0, h->cpl));
    if (split) {
      HIPCHK(hipEventRecord(h->ev_join, h->side));
      HIPCHK(hipStreamWaitEvent(s0, h->ev_join, 0));
    }
    if (sim_then_observe) {
      Params po = h->p;
      po.obs = d_obs;
      HIPCHK(launch(K_OBSERVE, h->lpe, po, h->lds_bytes, s0, h->cpl));
    }
    return PCGRL_OK;
  }
  HIPCHK(launch(K_ROLLOUT, h->lpe, p, h->lds_bytes, (hipStream_t)stream, h->cpl));
  return PCGRL_OK;
}

int pcgrl_rollout(pcgrl_handle h, const int32_t *d_actions, int32_t n_steps, int32_t auto_reset, uint8_t *d_obs,
                  int32_t obs_last_only, float *d_reward, uint8_t *d_done, int32_t *d_stats, void *stream) {
  return pcgrl_rollout_ex(h, d_actions, n_steps, auto_reset, d_obs, obs_last_only, d_reward, nullptr, d_done, d_stats, nullptr, stream);
}

int pcgrl_update(pcgrl_handle h, const int32_t *d_actions, uint8_t *d_obs, void *stream) {
  if (!h || !d_actions) return fail(PCGRL_EINVAL, "pcgrl_update: bad arguments");
  NOT_WITH_BUDGET(h, "pcgrl_update");
  NOT_ATTACHED(h, "pcgrl_update");
  ON_DEVICE(h->device);
  Params p = h->p;
  p.actions = d_actions;
  p.obs = d_obs;
  p.update_only = 1;
  h->maybe_stale = true;
  HIPCHK(launch(K_STEP, h->lpe, p, h->lds_bytes, (hipStream_t)stream, h->cpl, h->step16));
  return PCGRL_OK;
}

int pcgrl_refresh_stats(pcgrl_handle h, int32_t *d_stats, void *stream) {
  if (!h) return fail(PCGRL_EINVAL, "pcgrl_refresh_stats: null handle");
  ON_DEVICE(h->device);
  Params p = h->p;
  p.refresh_only = 1;
  p.stats_out = d_stats;
  with_budget(h, p);
  HIPCHK(launch(K_RESET, h->lpe, p, h->lds_bytes, (hipStream_t)stream, h->cpl));
  h->maybe_stale = false;
  return PCGRL_OK;
}

int pcgrl_queue_targets(pcgrl_handle h, const uint8_t *d_mask, const double *d_trg_lo, const double *d_trg_hi, void *stream) {
  if (!h || !d_trg_lo || !d_trg_hi) return fail(PCGRL_EINVAL, "pcgrl_queue_targets: bad arguments");
  ON_DEVICE(h->device);
  if (h->p.cfg.n_ctrl == 0) return fail(PCGRL_EINVAL, "pcgrl_queue_targets: the engine was created without control metrics");
  Params p = h->p;
  p.mask = d_mask;
  hipLaunchKernelGGL(queue_targets_kernel, dim3((p.n_envs + 63) / 64), dim3(64), 0, (hipStream_t)stream, p, d_trg_lo, d_trg_hi);
  HIPCHK(hipGetLastError());
  return PCGRL_OK;
}

int pcgrl_set_target_resampling(pcgrl_handle h, int32_t enable, uint64_t seed, const double *lo, const double *hi) {
  if (!h) return fail(PCGRL_EINVAL, "pcgrl_set_target_resampling: null handle");
  if (h->p.cfg.n_ctrl == 0) return fail(PCGRL_EINVAL, "pcgrl_set_target_resampling: the engine was created without control metrics");
  if (enable && (!lo || !hi)) return fail(PCGRL_EINVAL, "pcgrl_set_target_resampling: bounds missing");
  ON_DEVICE(h->device);
  TrgResample r;
  memset(&r, 0, sizeof(r));
  r.enable = enable ? 1 : 0;
  r.seed = seed;
  for (int j = 0; j < h->p.cfg.n_ctrl && enable; j++) {
    if (!(lo[j] <= hi[j])) return fail(PCGRL_EINVAL, "pcgrl_set_target_resampling: need lo <= hi for every control metric");
    r.lo[j] = lo[j];
    r.hi[j] = hi[j];
  }
  HIPCHK(hipDeviceSynchronize());  // (launches in flight keep the parameters they were issued under)
  HIPCHK(hipMemcpy((TrgResample *)h->p.trg - 1, &r, sizeof(r), hipMemcpyHostToDevice));
  return PCGRL_OK;
}

int pcgrl_ctrl_observe(pcgrl_handle h, float *d_ctrl_obs, void *stream) {
  if (!h || !d_ctrl_obs) return fail(PCGRL_EINVAL, "pcgrl_ctrl_observe: bad arguments");
  ON_DEVICE(h->device);
  if (h->p.cfg.n_ctrl == 0) return fail(PCGRL_EINVAL, "pcgrl_ctrl_observe: the engine was created without control metrics");
  Params p = h->p;
  p.ctrl_obs = d_ctrl_obs;
  dim3 grid((p.n_envs + 63) / 64), block(64);
  switch (p.cfg.n_stats) {
    case 2: hipLaunchKernelGGL((ctrl_observe_kernel<2>), grid, block, 0, (hipStream_t)stream, p); break;
    case 3: hipLaunchKernelGGL((ctrl_observe_kernel<3>), grid, block, 0, (hipStream_t)stream, p); break;
    default: hipLaunchKernelGGL((ctrl_observe_kernel<7>), grid, block, 0, (hipStream_t)stream, p); break;
  }
  HIPCHK(hipGetLastError());
  return PCGRL_OK;
}

int pcgrl_observe(pcgrl_handle h, uint8_t *d_obs, void *stream) {
  if (!h || !d_obs) return fail(PCGRL_EINVAL, "pcgrl_observe: bad arguments");
  NOT_ATTACHED(h, "pcgrl_observe");
  ON_DEVICE(h->device);
  Params p = h->p;
  p.obs = d_obs;
  HIPCHK(launch(K_OBSERVE, h->lpe, p, h->lds_bytes, (hipStream_t)stream, h->cpl));
  return PCGRL_OK;
}

int pcgrl_get_static(pcgrl_handle h, uint8_t *d_static, void *stream) {
  if (!h || !d_static) return fail(PCGRL_EINVAL, "pcgrl_get_static: bad arguments");
  ON_DEVICE(h->device);
  if (!h->p.cfg.static_tiles) return fail(PCGRL_EINVAL, "pcgrl_get_static: the engine was created without static tiles");
  Params p = h->p;
  p.out_static = d_static;
  const int nb = p.n_tiles <= 2 ? 1 : 3;
  if (p.cfg.dims[1] > 32)
    hipLaunchKernelGGL((get_static_kernel<uint64_t>), dim3(p.n_envs), dim3(64), 0, (hipStream_t)stream, p, nb);
  else
    hipLaunchKernelGGL((get_static_kernel<uint32_t>), dim3(p.n_envs), dim3(64), 0, (hipStream_t)stream, p, nb);
  HIPCHK(hipGetLastError());
  return PCGRL_OK;
}

int pcgrl_set_static(pcgrl_handle h, double static_prob, int32_t n_static_walls, int32_t eval_mode) {
  if (!h) return fail(PCGRL_EINVAL, "pcgrl_set_static: null handle");
  if (!h->p.cfg.static_tiles) return fail(PCGRL_EINVAL, "pcgrl_set_static: the engine was created without static tiles");
  if (static_prob > 1.0) return fail(PCGRL_EINVAL, "pcgrl_set_static: static_prob must be <= 1");
  if (n_static_walls > 0 && (h->p.cfg.dims[0] < 3 || h->p.cfg.dims[1] < 3))
    return fail(PCGRL_EINVAL, "pcgrl_set_static: static walls need a map of at least 3x3");
  if (static_prob >= 0.0) h->p.cfg.static_prob = static_prob;
  if (n_static_walls >= 0) h->p.cfg.n_static_walls = n_static_walls;
  if (eval_mode >= 0) h->p.cfg.static_eval = eval_mode ? 1 : 0;
  state_header_build(h);
  return PCGRL_OK;
}

int64_t pcgrl_obs_bytes(pcgrl_handle h) { return h ? h->obs_bytes : -1; }

int pcgrl_obs_shape(pcgrl_handle h, int32_t shape_out[4], int32_t *ndim_out) {
  if (!h) return fail(PCGRL_EINVAL, "pcgrl_obs_shape: null handle");
  memcpy(shape_out, h->obs_shape, sizeof(h->obs_shape));
  *ndim_out = h->obs_ndim;
  return PCGRL_OK;
}

int pcgrl_get_state(pcgrl_handle h, uint8_t *d_grids, int32_t *d_pos, int32_t *d_counters, int32_t *d_stats, double *d_last_loss,
                    double *d_ep_return, void *stream) {
  if (!h) return fail(PCGRL_EINVAL, "pcgrl_get_state: null handle");
  ON_DEVICE(h->device);
  Params p = h->p;
  p.out_grids = d_grids;
  p.out_pos = d_pos;
  p.out_counters = d_counters;
  p.stats_out = d_stats;
  p.out_last_loss = d_last_loss;
  p.out_ep_return = d_ep_return;
  HIPCHK(launch(K_GET_STATE, h->lpe, p, 0, (hipStream_t)stream, h->cpl));
  return PCGRL_OK;
}

int pcgrl_get_last_episode(pcgrl_handle h, double *d_ep_return, int32_t *d_ep_len, int32_t *d_final_stats, int64_t *d_n_episodes,
                           void *stream) {
  if (!h) return fail(PCGRL_EINVAL, "pcgrl_get_last_episode: null handle");
  ON_DEVICE(h->device);
  Params p = h->p;
  p.out_ep_return = d_ep_return;
  p.out_ep_len = d_ep_len;
  p.stats_out = d_final_stats;
  p.out_n_episodes = d_n_episodes;
  HIPCHK(launch(K_LAST_EPISODE, h->lpe, p, 0, (hipStream_t)stream, h->cpl));
  return PCGRL_OK;
}

// Scratch engines of the handle-less pcgrl_stats_for_grids: one per (problem, map shape, solver_power, device), created
// on first use and kept until pcgrl_stats_cache_clear() / process exit.  The statistics kernel needs no per-env state,
// only the engine's error word and (sokoban) solver workspace pool, so one engine serves any batch size.
static std::mutex g_stats_mu;
static std::map<std::tuple<int, int, int, int, int, int>, pcgrl_handle> g_stats_engines;

static int stats_engine_for(const pcgrl_config &cfg, int device, pcgrl_handle *out) {
  pcgrl_config c = cfg;
  c.representation = PCGRL_REP_NARROW;
  c.obs_window[0] = 2 * c.dims[0];
  c.obs_window[1] = c.ndim == 3 ? 2 * c.dims[1] : 32;  // unused by the statistics; any legal value
  c.obs_window[2] = c.ndim == 3 ? 2 * c.dims[2] : 1;
  c.n_ctrl = 0;
  c.static_tiles = 0;
  c.static_prob = 0.0;
  c.n_static_walls = 0;
  c.act_window[0] = c.act_window[1] = c.act_window[2] = 0;
  const auto key = std::make_tuple((int)c.problem, (int)c.dims[0], (int)c.dims[1], (int)(c.ndim == 3 ? c.dims[2] : 1),
                                   (int)c.solver_power, device);
  std::lock_guard<std::mutex> lock(g_stats_mu);
  auto it = g_stats_engines.find(key);
  if (it == g_stats_engines.end()) {
    pcgrl_handle h = nullptr;
    int rc = pcgrl_create(&c, 256, device, &h);  // 256 "envs": sizes the sokoban solver's workspace pool (64 slots)
    if (rc) return rc;
    it = g_stats_engines.emplace(key, h).first;
  }
  *out = it->second;
  return PCGRL_OK;
}

int pcgrl_stats_for_grids_h(pcgrl_handle h, int32_t n, const uint8_t *d_grids, int32_t *d_stats, void *stream) {
  if (!h || n < 1 || !d_grids || !d_stats) return fail(PCGRL_EINVAL, "pcgrl_stats_for_grids_h: bad arguments");
  ON_DEVICE(h->device);
  Params p;
  {
    // One level per workgroup, at most one such workgroup per CU: up to 256 searches run at once, each in a workspace
    // slot.  A batch that is much larger than the pool gets a larger pool the first time (synchronous, up to 256 slots =
    // 11.8 GB at the default solver_power; the old pool stays allocated until destroy: launches in flight on other streams
    // keep using it).  The handle-less entry point shares its hidden engines between threads: the pool is grown and the
    // launch parameters are read under one lock.
    static std::mutex grow_mu;
    std::lock_guard<std::mutex> lock(grow_mu);
    p = h->p;
    if (h->p.soko) soko_pool_for(h, p, std::min(256, sokoban_slots_for(n)), (hipStream_t)stream);
  }
  p.n_envs = n;  // the kernel touches no per-env engine state
  p.init_grids = d_grids;
  p.stats_out = d_stats;
  p.sk_helpers = h->p.soko ? 3 : 0;  // sokoban: one map per workgroup, the solver's stages side by side
  HIPCHK(launch(K_STATS_FOR_GRIDS, h->lpe, p, 0, (hipStream_t)stream, h->cpl));
  return PCGRL_OK;
}

int pcgrl_stats_for_grids(const pcgrl_config *cfg, int32_t n, const uint8_t *d_grids, int32_t *d_stats, int32_t device, void *stream) {
  if (!cfg || n < 1 || !d_grids || !d_stats) return fail(PCGRL_EINVAL, "pcgrl_stats_for_grids: bad arguments");
  pcgrl_handle h = nullptr;
  int rc = stats_engine_for(*cfg, device, &h);
  if (rc) return rc;
  return pcgrl_stats_for_grids_h(h, n, d_grids, d_stats, stream);
}

int pcgrl_stats_poll_error(const pcgrl_config *cfg, int32_t device) {
  if (!cfg) return fail(PCGRL_EINVAL, "pcgrl_stats_poll_error: bad arguments");
  pcgrl_handle h = nullptr;
  int rc = stats_engine_for(*cfg, device, &h);
  if (rc) return rc;
  return pcgrl_poll_error(h);
}

void pcgrl_stats_cache_clear(void) {
  std::lock_guard<std::mutex> lock(g_stats_mu);
  for (auto &kv : g_stats_engines) pcgrl_destroy(kv.second);
  g_stats_engines.clear();
}

int pcgrl_reduce_episodes(pcgrl_handle h, double *d_out, int32_t clear, void *stream) {
  if (!h || !d_out) return fail(PCGRL_EINVAL, "pcgrl_reduce_episodes: bad arguments");
  ON_DEVICE(h->device);
  if (h->p.n_envs <= 16384) {
    hipLaunchKernelGGL(reduce_episodes_small_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, h->p, d_out, clear ? 1 : 0);
    HIPCHK(hipGetLastError());
    return PCGRL_OK;
  }
  const int n_blocks = std::min(RED_BLOCKS, (h->p.n_envs + RED_THREADS - 1) / RED_THREADS);
  hipLaunchKernelGGL(reduce_episodes_kernel, dim3(n_blocks), dim3(RED_THREADS), 0, (hipStream_t)stream, h->p, h->red, d_out, n_blocks,
                     clear ? 1 : 0);
  HIPCHK(hipGetLastError());
  return PCGRL_OK;
}

int pcgrl_set_state(pcgrl_handle h, const uint8_t *d_mask, const uint8_t *d_grids, const int32_t *d_pos, const int32_t *d_counters,
                    const double *d_ep_return, void *stream) {
  if (!h || !d_grids) return fail(PCGRL_EINVAL, "pcgrl_set_state: bad arguments");
  if (h->p.ext) return fail(PCGRL_EUNSUPPORTED, "pcgrl_set_state: not with static tiles / action patches (their masks are drawn at reset)");
  ON_DEVICE(h->device);
  Params p = h->p;
  p.mask = d_mask;
  p.init_grids = d_grids;
  p.init_pos = d_pos;
  p.in_counters = d_counters;
  p.in_ep_return = d_ep_return;
  p.set_state = 1;
  with_budget(h, p);
  HIPCHK(launch(K_RESET, h->lpe, p, h->lds_bytes, (hipStream_t)stream, h->cpl));
  if (d_mask == nullptr) h->maybe_stale = false;
  return PCGRL_OK;
}

static size_t state_section(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// The image starts with one 256-byte header section: what it was exported from.  pcgrl_import_state refuses an image whose
// header does not match the importing engine (another config -- even one with the same byte size, e.g. other weights or
// targets --, another batch size, another per-env layout / library version) instead of importing it silently.
struct StateHeader {
  uint64_t magic;        // "PCGRLST2"
  uint64_t fingerprint;  // FNV-1a over the create-time config fields, n_envs, the library version string and every array's bytes per env
  int32_t n_envs, n_arrays;
  uint64_t total_bytes;
  // the three static-tile parameters pcgrl_set_static changes at run time (the reference's set_static_prob /
  // set_n_static_walls / set_eval_mode, reps/wrappers.py:256-263): state, not identity -- a full import applies them
  double static_prob;
  int32_t n_static_walls, static_eval;
};
static constexpr uint64_t STATE_MAGIC = 0x3254534c52474350ull;  // "PCGRLST2", little endian
static constexpr size_t STATE_HDR_BYTES = 256;
static_assert(sizeof(StateHeader) <= STATE_HDR_BYTES, "state header section");

static uint64_t state_fingerprint(pcgrl_handle h) {
  uint64_t x = 1469598103934665603ull;
  auto mix = [&](const void *p, size_t n) {
    for (size_t i = 0; i < n; i++) x = (x ^ ((const uint8_t *)p)[i]) * 1099511628211ull;
  };
  const pcgrl_config &c = h->p.cfg;  // field by field: the struct's padding bytes are not part of the config
#define MIX(f) mix(&c.f, sizeof(c.f))
  MIX(problem); MIX(representation); MIX(ndim); MIX(dims); MIX(obs_window); MIX(max_iterations); MIX(max_changes); MIX(n_stats);
  MIX(has_trg); MIX(weights); MIX(trg_lo); MIX(trg_hi); MIX(solver_power); MIX(n_ctrl); MIX(ctrl_idx); MIX(ctrl_range);
  MIX(act_window); MIX(static_tiles);  // (not static_prob / n_static_walls / static_eval: pcgrl_set_static moves them)
#undef MIX
  const int32_t n = h->p.n_envs;
  mix(&n, sizeof(n));
  const char *v = pcgrl_version();
  mix(v, strlen(v));
  for (auto &a : h->state_arrays) mix(&a.second, sizeof(a.second));
  return x;
}

// The header lives in pinned host memory owned by the engine: pcgrl_export_state copies it from there, so a captured export
// keeps a pointer that stays valid and every replay writes the header of the engine's CURRENT static-tile parameters.
static void state_header_build(pcgrl_handle h) {
  if (!h->hdr_host) return;
  StateHeader hdr{};
  hdr.magic = STATE_MAGIC;
  hdr.fingerprint = state_fingerprint(h);
  hdr.n_envs = h->p.n_envs;
  hdr.n_arrays = (int32_t)h->state_arrays.size();
  hdr.total_bytes = (uint64_t)pcgrl_state_bytes(h);
  hdr.static_prob = h->p.cfg.static_prob;
  hdr.n_static_walls = h->p.cfg.n_static_walls;
  hdr.static_eval = h->p.cfg.static_eval;
  // (no memset: the bytes behind the struct were zeroed once at create, and an export issued earlier may still be copying
  // from this pinned block -- magic / fingerprint / sizes are rewritten with the values they already hold, only the three
  // static-tile fields really change.  pcgrl_set_static must still be ordered after exports that are to carry the OLD
  // parameters: include/pcgrl_amd.h)
  memcpy(h->hdr_host, &hdr, sizeof(hdr));
}

int64_t pcgrl_state_bytes(pcgrl_handle h) {
  if (!h) return -1;
  size_t total = STATE_HDR_BYTES;
  for (auto &a : h->state_arrays) total += state_section(a.second * (size_t)h->p.n_envs);
  return (int64_t)total;
}

int pcgrl_export_state(pcgrl_handle h, uint8_t *d_buf, int32_t *maybe_stale_out, void *stream) {
  if (!h || !d_buf) return fail(PCGRL_EINVAL, "pcgrl_export_state: bad arguments");
  ON_DEVICE(h->device);
  // (pinned, engine-owned source: capturable, and no stack frame for the runtime to read later)
  HIPCHK(hipMemcpyAsync(d_buf, h->hdr_host, STATE_HDR_BYTES, hipMemcpyHostToDevice, (hipStream_t)stream));
  size_t off = STATE_HDR_BYTES;
  for (auto &a : h->state_arrays) {
    const size_t bytes = a.second * (size_t)h->p.n_envs;
    HIPCHK(hipMemcpyAsync(d_buf + off, a.first, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    off += state_section(bytes);
  }
  if (maybe_stale_out) *maybe_stale_out = h->maybe_stale ? 1 : 0;
  return PCGRL_OK;
}

int pcgrl_import_state(pcgrl_handle h, const uint8_t *d_mask, const uint8_t *d_buf, int32_t maybe_stale, void *stream) {
  if (!h || !d_buf) return fail(PCGRL_EINVAL, "pcgrl_import_state: bad arguments");
  ON_DEVICE(h->device);
  // the header is checked on the host before anything is overwritten: one small copy and a wait for `stream`
  StateHeader hdr{};
  HIPCHK(hipMemcpyAsync(&hdr, d_buf, sizeof(hdr), hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  if (hdr.magic != STATE_MAGIC) return fail(PCGRL_EINVAL, "pcgrl_import_state: not a pcgrl_export_state image (bad magic)");
  if (hdr.n_envs != h->p.n_envs || hdr.n_arrays != (int32_t)h->state_arrays.size() || hdr.total_bytes != (uint64_t)pcgrl_state_bytes(h) ||
      hdr.fingerprint != state_fingerprint(h))
    return fail(PCGRL_EINVAL, "pcgrl_import_state: the image was exported by an engine with another config, batch size or library version");
  // asynchronous stepping and the synchronous kernels each lack the other's per-env states: the resumable kernels carry no
  // code for statistics left stale by pcgrl_update, the synchronous ones none for a parked search (ENV_PENDING_STEP /
  // ENV_PENDING_STATS and pend_action would be ignored, not played).  Refused as pcgrl_set_solver_budget refuses them.
  if (h->sk_budget > 0 && maybe_stale != 0)
    return fail(PCGRL_EINVAL, "pcgrl_import_state: the image may carry statistics left stale by pcgrl_update, which the asynchronous "
                              "kernels have no code for (a solver budget is set): call pcgrl_refresh_stats before exporting");
  if (h->sk_budget == 0 && async_capable(h)) {  // (the mode, whatever the problem: every engine that can leave envs busy)
    const int32_t n = h->p.n_envs;
    size_t st_off = STATE_HDR_BYTES;
    for (auto &a : h->state_arrays) {
      if (a.first == (void *)h->p.st) break;
      st_off += state_section(a.second * (size_t)n);
    }
    std::vector<EnvState> st(n);
    std::vector<uint8_t> m(d_mask != nullptr ? n : 0);
    HIPCHK(hipMemcpyAsync(st.data(), d_buf + st_off, (size_t)n * sizeof(EnvState), hipMemcpyDeviceToHost, (hipStream_t)stream));
    if (d_mask != nullptr) HIPCHK(hipMemcpyAsync(m.data(), d_mask, (size_t)n, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    for (int32_t i = 0; i < n; i++)
      if ((d_mask == nullptr || m[i] != 0) && (st[i].flags & (ENV_PENDING_STEP | ENV_PENDING_STATS)) != 0)
        return fail(PCGRL_EINVAL, "pcgrl_import_state: env " + std::to_string(i) + " of the image is busy (a parked search of an engine "
                                  "with a solver budget), which only pcgrl_step_ready can finish: set a solver budget first");
  }
  // 3-D maze: searches parked in THIS engine belong to the states about to be replaced (parked searches are not in the image)
  if (h->a3_park)
    HIPCHK(launch_3d_async_unpark(h->a3_park, h->p.cfg.dims[0], h->p.cfg.dims[1], h->p.cfg.dims[2], h->p.n_envs, d_mask, (hipStream_t)stream));
  if (d_mask == nullptr && h->p.cfg.static_tiles) {
    // the exporter's run-time static-tile parameters (a curriculum's set_static_prob, evaluation mode) come with the image;
    // a masked import leaves the engine-wide parameters as they are
    if (!(hdr.static_prob >= 0.0 && hdr.static_prob <= 1.0) || hdr.n_static_walls < 0)
      return fail(PCGRL_EINVAL, "pcgrl_import_state: corrupt static-tile parameters in the image header");
    h->p.cfg.static_prob = hdr.static_prob;
    h->p.cfg.n_static_walls = hdr.n_static_walls;
    h->p.cfg.static_eval = hdr.static_eval ? 1 : 0;
    state_header_build(h);
  }
  size_t off = STATE_HDR_BYTES;
  for (auto &a : h->state_arrays) {
    const size_t bytes = a.second * (size_t)h->p.n_envs;
    if (d_mask == nullptr) {
      HIPCHK(hipMemcpyAsync(a.first, d_buf + off, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    } else {
      const int64_t wpe = (int64_t)(a.second / 4), total = wpe * h->p.n_envs;  // (every array's row is a multiple of 4 bytes)
      hipLaunchKernelGGL(masked_rows_copy_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                         (uint32_t *)a.first, (const uint32_t *)(d_buf + off), wpe, h->p.n_envs, d_mask);
      HIPCHK(hipGetLastError());
    }
    off += state_section(bytes);
  }
  // the imported envs may carry statistics left stale by pcgrl_update: the host-side kernel choice follows the exporter's
  h->maybe_stale = d_mask == nullptr ? (maybe_stale != 0) : (h->maybe_stale || maybe_stale != 0);
  return PCGRL_OK;
}

int pcgrl_get_rng_state(pcgrl_handle h, uint64_t *d_out, void *stream) {
  if (!h || !d_out) return fail(PCGRL_EINVAL, "pcgrl_get_rng_state: bad arguments");
  ON_DEVICE(h->device);
  hipLaunchKernelGGL(rng_state_kernel, dim3((h->p.n_envs + 63) / 64), dim3(64), 0, (hipStream_t)stream, h->p, d_out, (const uint64_t *)nullptr);
  HIPCHK(hipGetLastError());
  return PCGRL_OK;
}

int pcgrl_set_rng_state(pcgrl_handle h, const uint8_t *d_mask, const uint64_t *d_in, void *stream) {
  if (!h || !d_in) return fail(PCGRL_EINVAL, "pcgrl_set_rng_state: bad arguments");
  ON_DEVICE(h->device);
  Params p = h->p;
  p.mask = d_mask;
  hipLaunchKernelGGL(rng_state_kernel, dim3((p.n_envs + 63) / 64), dim3(64), 0, (hipStream_t)stream, p, (uint64_t *)nullptr, d_in);
  HIPCHK(hipGetLastError());
  return PCGRL_OK;
}

static int32_t num_actions_of(const pcgrl_engine *h) {
  const pcgrl_config &c = h->p.cfg;
  if (c.act_window[0] > 0) return h->p.n_tiles;  // MultiDiscrete([n_tiles] * prod(act_window)), reps/wrappers.py:475-478
  switch (c.representation) {
    case PCGRL_REP_NARROW: return h->p.n_tiles;      // narrow_rep.py: Discrete(n_tiles)
    case PCGRL_REP_TURTLE: return h->p.n_tiles + 4;  // turtle_rep.py: 4 moves + n_tiles (A6)
    default: return h->p.n_cells * h->p.n_tiles;     // wide: ActionMap's flat (cell, tile) index (A7)
  }
}

int32_t pcgrl_num_actions(pcgrl_handle h) { return h ? num_actions_of(h) : -1; }

int pcgrl_sample_actions(pcgrl_handle h, int32_t *d_actions, uint64_t seed, void *stream) {
  if (!h || !d_actions) return fail(PCGRL_EINVAL, "pcgrl_sample_actions: bad arguments");
  ON_DEVICE(h->device);
  const int32_t n = h->p.n_envs * h->p.n_act;
  hipLaunchKernelGGL(sample_actions_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_actions, n,
                     (uint32_t)num_actions_of(h), seed, h->sample);
  HIPCHK(hipGetLastError());
  return PCGRL_OK;
}

int pcgrl_set_solver_budget(pcgrl_handle h, int32_t budget) {
  if (!h || budget < 0) return fail(PCGRL_EINVAL, "pcgrl_set_solver_budget: bad arguments");
  NOT_ATTACHED(h, "pcgrl_set_solver_budget");
  const bool maze3d = h->p.cfg.problem == PCGRL_PROB_MC3DMAZE;
  if (maze3d && h->p.cfg.representation != PCGRL_REP_NARROW)
    return fail(PCGRL_EUNSUPPORTED, "pcgrl_set_solver_budget: minecraft_3D_maze steps asynchronously under the narrow representation only "
                                    "(the turtle and wide kernels are synchronous)");
  if (!maze3d && (h->p.cfg.problem != PCGRL_PROB_SOKOBAN || !h->p.soko))
    return fail(PCGRL_EUNSUPPORTED, "pcgrl_set_solver_budget: only sokoban (device solver) and minecraft_3D_maze narrow (path searches) "
                                    "have resumable searches");
  if (h->p.ext || h->p.cfg.n_ctrl > 0)
    return fail(PCGRL_EUNSUPPORTED, "pcgrl_set_solver_budget: asynchronous stepping is built for sokoban and the 3-D maze without static "
                                    "tiles, action patches or control metrics");
  if (budget > 0 && h->maybe_stale)
    return fail(PCGRL_EINVAL, "pcgrl_set_solver_budget: statistics left stale by pcgrl_update may exist (the asynchronous kernels carry no "
                              "code for them): call pcgrl_refresh_stats or reset the envs first");
  ON_DEVICE(h->device);
  if (maze3d && budget > 0 && h->a3_park == nullptr) {  // one park record per env, once (12 320 / 105 760 bytes by size class)
    HIPCHK(hipDeviceSynchronize());
    const size_t bytes = a3_park_bytes(h->p.cfg.dims[0], h->p.cfg.dims[1], h->p.cfg.dims[2]) * (size_t)h->p.n_envs;
    void *pool = nullptr;
    hipError_t e = hipMalloc(&pool, bytes);
    if (e == hipSuccess) {
      h->allocs.push_back(pool);
      e = hipMemset(pool, 0, bytes);
    }
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return fail(PCGRL_EHIP, std::string("pcgrl_set_solver_budget: allocating one park record per env: ") + hipGetErrorString(e));
    }
    h->a3_park = pool;
  }
  if (!maze3d && budget > 0 && h->sk_ws == nullptr) {  // one stage workspace + one park record per env, once
    HIPCHK(hipDeviceSynchronize());
    const hipError_t e = sokoban_alloc_async(h->p, h->allocs, h->p.n_envs, &h->sk_ws, &h->sk_park);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return fail(PCGRL_EHIP, std::string("pcgrl_set_solver_budget: allocating one solver workspace per env: ") + hipGetErrorString(e));
    }
  }
  if (budget == 0 && h->sk_budget > 0) {  // back to synchronous stepping: nobody may be waiting for a parked search
    HIPCHK(hipDeviceSynchronize());
    std::vector<EnvState> st(h->p.n_envs);
    HIPCHK(hipMemcpy(st.data(), h->p.st, st.size() * sizeof(EnvState), hipMemcpyDeviceToHost));
    for (auto &e : st)
      if (e.flags & (ENV_PENDING_STEP | ENV_PENDING_STATS))
        return fail(PCGRL_EINVAL, "pcgrl_set_solver_budget(0): an env is still busy (a parked search): keep stepping with pcgrl_step_ready "
                                  "or reset the envs first");
  }
  h->sk_budget = budget;
  return PCGRL_OK;
}

int32_t pcgrl_get_solver_budget(pcgrl_handle h) { return h ? h->sk_budget : -1; }

// include/pcgrl_amd_async3d.h
int64_t pcgrl_park_bytes_per_env(pcgrl_handle h) {
  if (!h) return -1;
  if (h->p.cfg.problem != PCGRL_PROB_MC3DMAZE || h->p.cfg.representation != PCGRL_REP_NARROW) return 0;
  return (int64_t)a3_park_bytes(h->p.cfg.dims[0], h->p.cfg.dims[1], h->p.cfg.dims[2]);
}

int pcgrl_step_ready(pcgrl_handle h, const int32_t *d_actions, int32_t auto_reset, uint8_t *d_obs, float *d_reward, uint8_t *d_done,
                     int32_t *d_stats, uint8_t *d_status, void *stream) {
  if (!h || !d_actions || !d_status) return fail(PCGRL_EINVAL, "pcgrl_step_ready: bad arguments");
  if (h->sk_budget <= 0) return fail(PCGRL_EINVAL, "pcgrl_step_ready: no solver budget set (pcgrl_set_solver_budget)");
  ON_DEVICE(h->device);
  Params p = h->p;
  p.no_fast = h->maybe_stale ? 1 : 0;
  soko_pool_lazy(h, p, (hipStream_t)stream);  // (levels of more than SK_MAXC pairs run the synchronous solver on the pool)
  p.spread = 1;  // one env per workgroup: every search has a wavefront of its own
  p.sk_helpers = 0;
  with_budget(h, p);
  p.actions = d_actions;
  p.auto_reset = auto_reset;
  p.obs = d_obs;
  p.reward = d_reward;
  p.done = d_done;
  p.stats_out = d_stats;
  p.ready = d_status;
  HIPCHK(launch(K_STEP, h->lpe, p, h->lds_bytes, (hipStream_t)stream, h->cpl, h->step16));
  return PCGRL_OK;
}

int pcgrl_env_busy(pcgrl_handle h, uint8_t *d_busy, void *stream) {
  if (!h || !d_busy) return fail(PCGRL_EINVAL, "pcgrl_env_busy: bad arguments");
  ON_DEVICE(h->device);
  hipLaunchKernelGGL(env_busy_kernel, dim3((h->p.n_envs + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->p, d_busy);
  HIPCHK(hipGetLastError());
  return PCGRL_OK;
}

int pcgrl_reserve_solver_pool(pcgrl_handle h, int32_t n_slots, int32_t allow_lazy_growth) {
  if (!h) return fail(PCGRL_EINVAL, "pcgrl_reserve_solver_pool: null handle");
  if (!h->p.soko) return fail(PCGRL_EINVAL, "pcgrl_reserve_solver_pool: the engine has no device solver (sokoban only)");
  ON_DEVICE(h->device);
  h->soko_lazy = allow_lazy_growth != 0;
  const int full = sokoban_slots_for(h->p.n_envs);
  const int want = n_slots < 0 ? h->soko_slots : (n_slots == 0 ? full : std::min((int)n_slots, 512));
  Params scratch = h->p;
  return soko_pool_for(h, scratch, want, nullptr, /*lazy=*/false);
}

int32_t pcgrl_solver_pool_slots(pcgrl_handle h, int32_t *full_size_out, int32_t *grow_failed_out) {
  if (!h || !h->p.soko) return 0;
  if (full_size_out) *full_size_out = sokoban_slots_for(h->p.n_envs);
  if (grow_failed_out) *grow_failed_out = h->soko_grow_failed ? 1 : 0;
  if (h->soko_grow_failed) g_err = h->soko_grow_msg;
  return h->soko_slots;
}

// Host utilities for a foreign-language host (ctypes): the HIP runtime THIS library is linked against -- the one that owns
// the handles the caller passes -- instead of a second dlopen of libamdhip64 by name.
int pcgrl_copy_to_host(void *dst_host, const void *d_src, int64_t bytes, void *stream) {
  if (!dst_host || !d_src || bytes < 0) return fail(PCGRL_EINVAL, "pcgrl_copy_to_host: bad arguments");
  HIPCHK(hipMemcpyAsync(dst_host, d_src, (size_t)bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
  return PCGRL_OK;
}

int pcgrl_stream_synchronize(void *stream) {
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  return PCGRL_OK;
}

int pcgrl_graph_upload(void *graph_exec, void *stream) {
  if (!graph_exec) return fail(PCGRL_EINVAL, "pcgrl_graph_upload: null graph");
  HIPCHK(hipGraphUpload((hipGraphExec_t)graph_exec, (hipStream_t)stream));
  return PCGRL_OK;
}

int pcgrl_debug_counters(pcgrl_handle h, uint64_t *out, int32_t n) {
  if (!h || !out || n < 1 || n > 8 * (h->p.n_envs + 64)) return fail(PCGRL_EINVAL, "pcgrl_debug_counters: bad arguments");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(out, h->p.err + 64, sizeof(uint64_t) * n, hipMemcpyDeviceToHost));
  HIPCHK(hipMemset(h->p.err + 64, 0, sizeof(uint64_t) * n));
  return PCGRL_OK;
}

int pcgrl_poll_error(pcgrl_handle h) {
  if (!h) return fail(PCGRL_EINVAL, "pcgrl_poll_error: null handle");
  ON_DEVICE(h->device);
  HIPCHK(hipDeviceSynchronize());
  int32_t flags[4] = {0, 0, 0, 0};
  HIPCHK(hipMemcpy(flags, h->p.err, sizeof(flags), hipMemcpyDeviceToHost));
  if (flags[0]) {
    HIPCHK(hipMemset(h->p.err, 0, sizeof(flags)));
    if (flags[0] & 1) return fail(PCGRL_EACTION, "an action was outside the action space (the reference raises IndexError)");
    if (flags[0] & 2) return fail(PCGRL_EUNSUPPORTED, "sokoban solver: level exceeds the device solver's limits");
    if (flags[0] & 4) return fail(PCGRL_EUNSUPPORTED, "3-D maze path search: more live queue entries than the search ring holds (512 for planes of <= 64 cells, else 4096); the statistics of that step were kept at their previous values and are recomputed from scratch at the env's next changing step");
    if (flags[0] & 8)
      return fail(PCGRL_ESTALE, "a step launch issued before pcgrl_update (a replayed HIP graph?) met statistics that pcgrl_update "
                                "left stale: re-capture after pcgrl_update or call pcgrl_refresh_stats first (include/pcgrl_amd.h, HIP graphs)");
    return fail(PCGRL_EINVAL, "device error flag set");
  }
  return PCGRL_OK;
}

// ---------------------------------------------------------------------------------------------- tile-code observations
// include/pcgrl_amd_codes.h; the kernels live in codes/pcgrl_codes.hip
static void codes_layout(const pcgrl_engine *h, int32_t shape[4], int *ndim, int *C, int *CS) {
  const pcgrl_config &c = h->p.cfg;
  const int nt = h->p.n_tiles;
  shape[0] = shape[1] = shape[2] = shape[3] = 0;
  if (c.problem == PCGRL_PROB_MC3DMAZE && c.representation == PCGRL_REP_WIDE) {
    shape[0] = c.dims[0];  // obs["map"] itself: 0 AIR, 1 DIRT, 2 path overlay
    shape[1] = c.dims[1];
    shape[2] = c.dims[2];
    shape[3] = 1;
    *ndim = 4;
    *C = *CS = 3;
  } else if (c.problem == PCGRL_PROB_MC3DMAZE) {
    shape[0] = c.obs_window[0];
    shape[1] = c.obs_window[1];
    shape[2] = c.obs_window[2];
    shape[3] = 1;
    *ndim = 4;
    *C = *CS = 4;
  } else if (c.representation == PCGRL_REP_WIDE) {
    shape[0] = c.dims[0];
    shape[1] = c.dims[1];
    shape[2] = 1;
    *ndim = 3;
    *C = *CS = nt;
  } else {
    shape[0] = c.obs_window[0];
    shape[1] = c.obs_window[1];
    shape[2] = 1 + (c.static_tiles ? 1 : 0);
    *ndim = 3;
    *CS = nt + 1;
    *C = nt + 1 + (c.static_tiles ? 1 : 0);
  }
}

static int64_t codes_bytes_of(const pcgrl_engine *h) {
  int32_t shape[4];
  int nd = 0, C = 0, CS = 0;
  codes_layout(h, shape, &nd, &C, &CS);
  int64_t n = 1;
  for (int i = 0; i < nd; i++) n *= shape[i];
  return n;
}

int pcgrl_codes_shape(pcgrl_handle h, int32_t shape_out[4], int32_t *ndim_out) {
  if (!h || !shape_out || !ndim_out) return fail(PCGRL_EINVAL, "pcgrl_codes_shape: bad arguments");
  int nd = 0, C = 0, CS = 0;
  codes_layout(h, shape_out, &nd, &C, &CS);
  *ndim_out = nd;
  return PCGRL_OK;
}

int64_t pcgrl_codes_bytes(pcgrl_handle h) { return h ? codes_bytes_of(h) : -1; }

int pcgrl_observe_codes(pcgrl_handle h, uint8_t *d_codes, void *stream) {
  if (!h || !d_codes) return fail(PCGRL_EINVAL, "pcgrl_observe_codes: bad arguments");
  if (h->p.cfg.problem == PCGRL_PROB_MC3DMAZE)
    return fail(PCGRL_EUNSUPPORTED, "pcgrl_observe_codes: the 3-D observation shows the overlay of the last statistics update: "
                                    "pcgrl_observe into a one-hot buffer, then pcgrl_onehot_to_codes");
  ON_DEVICE(h->device);
  int32_t shape[4];
  int nd = 0, C = 0, CS = 0;
  codes_layout(h, shape, &nd, &C, &CS);
  CodesArgs a;
  a.out = d_codes;
  a.T = (int32_t)codes_bytes_of(h);
  a.P = 1 + C - CS;
  a.wide = h->p.cfg.representation == PCGRL_REP_WIDE ? 1 : 0;
  a.nt = obs_nt_for(h, (int64_t)h->p.n_envs * a.T) ? 1 : 0;  // (the one-hot kernels' rule, Params::obs16 bit 1)
  HIPCHK(launch_codes_observe(h->p, h->lpe, a, (hipStream_t)stream));
  return PCGRL_OK;
}

static int onehot_to_codes(pcgrl_handle h, const uint8_t *d_onehot, int64_t n_rows, uint8_t *d_codes, void *stream) {
  int32_t shape[4];
  int nd = 0, C = 0, CS = 0;
  codes_layout(h, shape, &nd, &C, &CS);
  const int cells = (int)(h->obs_bytes / C);
  HIPCHK(launch_onehot_to_codes(d_onehot, n_rows, cells, C, CS, d_codes, (hipStream_t)stream));
  return PCGRL_OK;
}

int pcgrl_onehot_to_codes(pcgrl_handle h, const uint8_t *d_onehot, int64_t n_rows, uint8_t *d_codes, void *stream) {
  if (!h || !d_onehot || !d_codes || n_rows < 0) return fail(PCGRL_EINVAL, "pcgrl_onehot_to_codes: bad arguments");
  ON_DEVICE(h->device);
  return onehot_to_codes(h, d_onehot, n_rows, d_codes, stream);
}

int pcgrl_step_ready_codes(pcgrl_handle h, const int32_t *d_actions, int32_t auto_reset, uint8_t *d_scratch, uint8_t *d_codes,
                           float *d_reward, uint8_t *d_done, int32_t *d_stats, uint8_t *d_status, void *stream) {
  if (!h || !d_actions || !d_scratch || !d_codes || !d_status) return fail(PCGRL_EINVAL, "pcgrl_step_ready_codes: bad arguments");
  const int rc = pcgrl_step_ready(h, d_actions, auto_reset, d_scratch, d_reward, d_done, d_stats, d_status, stream);
  if (rc != PCGRL_OK) return rc;
  ON_DEVICE(h->device);
  return onehot_to_codes(h, d_scratch, h->p.n_envs, d_codes, stream);
}

// ---------------------------------------------------------------------------------------------- solution paths
// include/pcgrl_amd_paths.h; kernels in paths/pcgrl_paths.h
int32_t pcgrl_path_capacity(pcgrl_handle h) {
  if (!h) return -1;
  const int cells = h->p.cfg.dims[0] * h->p.cfg.dims[1];
  switch (h->p.cfg.problem) {
    case PCGRL_PROB_BINARY: return cells;
    case PCGRL_PROB_ZELDA: return 2 * cells;
    default: return 0;  // (no path to hand out)
  }
}

// n maps -- the engine's own (d_grids == nullptr, own) or the caller's -- through the path kernel
static int paths_launch(pcgrl_handle h, const char *who, bool own, int32_t n, const uint8_t *d_grids, int32_t cap, int16_t *d_path,
                        int32_t *d_len, void *d_overlay, void *stream) {
  if (!h || cap < 1 || n < 0 || (n > 0 && (!d_path || !d_len || (!own && !d_grids))))
    return fail(PCGRL_EINVAL, std::string(who) + ": bad arguments");
  const int prob = h->p.cfg.problem;
  if (prob != PCGRL_PROB_BINARY && prob != PCGRL_PROB_ZELDA)
    return fail(PCGRL_EUNSUPPORTED, std::string(who) + (prob == PCGRL_PROB_SOKOBAN
                                        ? ": sokoban's solution is an action list out of a transient search, not a path"
                                        : ": the 3-D maze shows its path as the overlay channel of the observation"));
  if (n == 0) return PCGRL_OK;
  ON_DEVICE(h->device);
  Params p = h->p;
  p.n_envs = n;  // the kernel touches no per-env engine state but the tile planes
  p.init_grids = d_grids;
  PathArgs a;
  a.path = d_path;
  a.len = d_len;
  a.overlay = (uint8_t *)d_overlay;
  a.cap = cap;
  a.from_grids = own ? 0 : 1;
  a.ts = 0;
  HIPCHK(launch_paths(p, h->lpe, a, (hipStream_t)stream));
  return PCGRL_OK;
}

int pcgrl_paths(pcgrl_handle h, int32_t cap, int16_t *d_path, int32_t *d_len, uint8_t *d_overlay, void *stream) {
  return paths_launch(h, "pcgrl_paths", true, h ? h->p.n_envs : 0, nullptr, cap, d_path, d_len, d_overlay, stream);
}

int pcgrl_paths_for_grids(pcgrl_handle h, int32_t n, const uint8_t *d_grids, int32_t cap, int16_t *d_path, int32_t *d_len,
                          uint8_t *d_overlay, void *stream) {
  return paths_launch(h, "pcgrl_paths_for_grids", false, n, d_grids, cap, d_path, d_len, d_overlay, stream);
}

// ---------------------------------------------------------------------------------------------- sokoban solutions
// include/pcgrl_amd_solutions.h; kernel in solutions/pcgrl_solutions.h
int32_t pcgrl_solution_capacity(pcgrl_handle h) {
  if (!h) return -1;
  return h->p.cfg.problem == PCGRL_PROB_SOKOBAN ? h->p.cfg.solver_power : 0;  // (no solver, no solution)
}

// n maps -- the engine's own (d_grids == nullptr, own) or the caller's -- through the solution kernel
static int solutions_launch(pcgrl_handle h, const char *who, bool own, int32_t n, const uint8_t *d_grids, int32_t cap, int8_t *d_moves,
                            int32_t *d_len, int32_t *d_dist_win, void *stream) {
  if (!h || cap < 1 || n < 0 || (n > 0 && (!d_moves || !d_len || (!own && !d_grids))))
    return fail(PCGRL_EINVAL, std::string(who) + ": bad arguments");
  if (h->p.cfg.problem != PCGRL_PROB_SOKOBAN || !h->p.soko)
    return fail(PCGRL_EUNSUPPORTED, std::string(who) + ": only sokoban has a solver and a solution (paths: pcgrl_amd_paths.h)");
  if (n == 0) return PCGRL_OK;
  ON_DEVICE(h->device);
  Params p = h->p;
  // one search per workgroup, each on a slot of the synchronous pool -- also under a solver budget: the per-env workspaces of
  // asynchronous stepping and their park records are not touched.  A batch much larger than the pool gets a larger pool the
  // first time, as in pcgrl_stats_for_grids_h (never while `stream` is being captured: searches then wait for a slot)
  soko_pool_for(h, p, std::min(256, sokoban_slots_for(n)), (hipStream_t)stream);
  p.n_envs = n;  // the kernel touches no per-env engine state but the tile planes
  p.init_grids = d_grids;
  SolArgs a;
  a.moves = d_moves;
  a.len = d_len;
  a.dist_win = d_dist_win;
  a.cap = cap;
  a.from_grids = own ? 0 : 1;
  HIPCHK(launch_solutions(p, h->lpe, a, (hipStream_t)stream));
  return PCGRL_OK;
}

int pcgrl_solutions(pcgrl_handle h, int32_t cap, int8_t *d_moves, int32_t *d_len, int32_t *d_dist_win, void *stream) {
  return solutions_launch(h, "pcgrl_solutions", true, h ? h->p.n_envs : 0, nullptr, cap, d_moves, d_len, d_dist_win, stream);
}

int pcgrl_solutions_for_grids(pcgrl_handle h, int32_t n, const uint8_t *d_grids, int32_t cap, int8_t *d_moves, int32_t *d_len,
                              int32_t *d_dist_win, void *stream) {
  return solutions_launch(h, "pcgrl_solutions_for_grids", false, n, d_grids, cap, d_moves, d_len, d_dist_win, stream);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------- measures and diversity
// The measure / pack step and the pairwise step are the same for every problem: one host path, composed by the entry points of
// include/pcgrl_amd_measures.h (below), include/pcgrl_amd_loderunner_measures.h and include/pcgrl_amd_smb_measures.h (further
// down).  An entry point checks its own preconditions (a null handle, the 3-D refusal, its shape range), calls the pointer
// check here before any HIP call, and hands the arguments and its measure / pack launch to an enqueue.  Kernels in
// measures/pcgrl_measures.h and, the per-map wave body, measures/pcgrl_measures_wave.h.

// map e at d_grids + e * stride (null: the 2-D engine's own planes), h x w cells each
static MeasWaveArgs meas_args(const uint8_t *d_grids, int32_t stride, int32_t h, int32_t w, int32_t n) {
  MeasWaveArgs a{};
  a.grids = d_grids;
  a.stride = stride;
  a.h = h;
  a.w = w;
  a.n = n;
  a.NW = (h * w + 63) / 64;
  a.group = 1;
  return a;
}

// the pointer checks of a measures call (`caller`: the call takes caller maps, so it needs d_grids)
static int measures_check(const char *who, bool caller, int32_t n, const uint8_t *d_grids, const int32_t *d_counts,
                          const int32_t *d_match, const double *d_entropy, const double *d_tab) {
  if (n < 0 || (n > 0 && (!d_counts || !d_match || (d_entropy && !d_tab) || (caller && !d_grids))))
    return fail(PCGRL_EINVAL, std::string(who) + ": bad arguments");
  return PCGRL_OK;
}

// the pointer checks of a diversity call, then the group
static int diversity_check(const char *who, bool caller, int32_t n, const uint8_t *d_grids, int32_t group, const void *d_scratch,
                           const int64_t *d_sum) {
  if (n < 0 || (n > 0 && (!d_scratch || ((uintptr_t)d_scratch & 7u) || !d_sum || (caller && !d_grids))))
    return fail(PCGRL_EINVAL, std::string(who) + ": bad arguments");
  if (group < 2 || n % group != 0)
    return fail(PCGRL_EINVAL, std::string(who) + ": group must be at least 2 and divide the number of maps");
  return PCGRL_OK;
}

// `launch(a, stream)` is the problem's measure / pack kernel (launch_smb_measures, launch_lr_measures, or launch_measures
// bound to an engine's Params)
template <class Launch>
static int measures_enqueue(MeasWaveArgs a, Launch launch, int32_t *d_counts, int32_t *d_match, double *d_forms,
                            double *d_entropy, const double *d_tab, void *stream) {
  a.counts = d_counts;
  a.match = d_match;
  a.forms = d_forms;
  a.entropy = d_entropy;
  a.tab = d_tab;
  HIPCHK(launch(a, (hipStream_t)stream));
  return PCGRL_OK;
}

// the bit-plane image of n maps of P planes, then one nearest-map key per map
static size_t diversity_scratch_bytes(int P, int32_t h, int32_t w, int32_t n) {
  return (size_t)n * (P * ((h * w + 63) / 64) + 1) * sizeof(uint64_t);
}

// pack the n maps into d_scratch, then the all-pairs kernel per group and the finish
template <class Launch>
static int diversity_enqueue(MeasWaveArgs a, int P, Launch launch, int32_t group, void *d_scratch, int64_t *d_sum,
                             double *d_scores, int32_t *d_nearest, int32_t *d_nearest_idx, int32_t *d_pairwise, void *stream) {
  a.pack = (uint64_t *)d_scratch;
  a.sum = (unsigned long long *)d_sum;
  a.near_key = (unsigned long long *)(a.pack + (size_t)a.n * P * a.NW);
  a.group = group;
  HIPCHK(launch(a, (hipStream_t)stream));
  DivArgs d;
  d.pack = a.pack;
  d.n = a.n;
  d.K = group;
  d.P = P;
  d.NW = a.NW;
  div_splits(a.n, group, d.splits, d.tiles_per_split);
  d.sum = a.sum;
  d.near_key = a.near_key;
  d.pairwise = d_pairwise;
  HIPCHK(launch_diversity(d, (hipStream_t)stream));
  if (d_scores || d_nearest || d_nearest_idx)
    HIPCHK(launch_diversity_finish(d, a.h * a.w, d_nearest, d_nearest_idx, d_scores, (hipStream_t)stream));
  return PCGRL_OK;
}

// The caller-map entry points of a level family (<family>_measures_for_grids, <family>_diversity_for_grids): `check_shape` is
// the family's shape refusal, P its plane count and `launch` its measure / pack kernel.  The pointer checks come first.
typedef int (*ShapeCheck)(const char *who, int32_t h, int32_t w);

template <class Launch>
static int measures_for_grids(const char *who, ShapeCheck check_shape, Launch launch, int32_t h, int32_t w, int32_t n,
                              const uint8_t *d_grids, int32_t *d_counts, int32_t *d_match, double *d_forms, double *d_entropy,
                              const double *d_tab, void *stream) {
  int rc = measures_check(who, true, n, d_grids, d_counts, d_match, d_entropy, d_tab);
  if (rc == PCGRL_OK) rc = check_shape(who, h, w);
  if (rc != PCGRL_OK || n == 0) return rc;
  return measures_enqueue(meas_args(d_grids, h * w, h, w, n), launch, d_counts, d_match, d_forms, d_entropy, d_tab, stream);
}

template <class Launch>
static int diversity_for_grids(const char *who, ShapeCheck check_shape, int P, Launch launch, int32_t h, int32_t w, int32_t n,
                               const uint8_t *d_grids, int32_t group, void *d_scratch, int64_t *d_sum, double *d_scores,
                               int32_t *d_nearest, int32_t *d_nearest_idx, int32_t *d_pairwise, void *stream) {
  int rc = diversity_check(who, true, n, d_grids, group, d_scratch, d_sum);
  if (rc == PCGRL_OK) rc = check_shape(who, h, w);
  if (rc != PCGRL_OK || n == 0) return rc;
  return diversity_enqueue(meas_args(d_grids, h * w, h, w, n), P, launch, group, d_scratch, d_sum, d_scores, d_nearest,
                           d_nearest_idx, d_pairwise, stream);
}

// ---------------------------------------------------------------------------------------------- level families: shared checks
// What the entry points of the level families below share besides the measures.

// a config's per-statistic targets and weights into the kernel's arguments, K statistics
template <int K, class Args, class Config>
static void copy_targets(Args &a, const Config *cfg) {
  for (int k = 0; k < K; k++) {
    a.has_trg[k] = cfg->has_trg[k];
    a.weight[k] = cfg->weight[k];
    a.trg_lo[k] = cfg->trg_lo[k];
    a.trg_hi[k] = cfg->trg_hi[k];
  }
}

// the caller's workspace: `align` a power of two, `needed` what `sized_by` (the function the text names) gives for the call
static int workspace_check(const char *who, const void *d_workspace, unsigned align, int64_t given, int64_t needed,
                           const char *sized_by) {
  if (!d_workspace || ((uintptr_t)d_workspace & (align - 1)) || given < needed)
    return fail(PCGRL_EINVAL, std::string(who) + ": the workspace is null, not " + std::to_string(align) +
                                  "-byte aligned or smaller than " + sized_by);
  return PCGRL_OK;
}

// include/pcgrl_amd_measures.h: the 2-D engine's maps (`own`) or caller maps of its problem and shape
static const char *MEASURES_3D =
    ": 2-D problems only (the reference's get_counts reads an attribute the 3-D maze does not have and get_co looks at two "
    "axes only)";

static int measures_2d_refuse(pcgrl_handle h, const char *who) {
  if (!h) return fail(PCGRL_EINVAL, std::string(who) + ": bad arguments");
  if (h->p.cfg.ndim != 2) return fail(PCGRL_EUNSUPPORTED, std::string(who) + MEASURES_3D);
  return PCGRL_OK;
}

static MeasWaveArgs meas_args_2d(pcgrl_handle h, bool own, int32_t n, const uint8_t *d_grids) {
  const int32_t H = h->p.cfg.dims[0], W = h->p.cfg.dims[1];
  return meas_args(own ? nullptr : d_grids, H * W, H, W, n);
}

static int measures_2d(pcgrl_handle h, const char *who, bool own, int32_t n, const uint8_t *d_grids, int32_t *d_counts,
                       int32_t *d_match, double *d_forms, double *d_entropy, const double *d_tab, void *stream) {
  int rc = measures_2d_refuse(h, who);
  if (rc == PCGRL_OK) rc = measures_check(who, !own, n, d_grids, d_counts, d_match, d_entropy, d_tab);
  if (rc != PCGRL_OK || n == 0) return rc;
  ON_DEVICE(h->device);
  return measures_enqueue(meas_args_2d(h, own, n, d_grids),
                          [h](const MeasWaveArgs &a, hipStream_t s) { return launch_measures(h->p, a, s); }, d_counts, d_match,
                          d_forms, d_entropy, d_tab, stream);
}

static int diversity_2d(pcgrl_handle h, const char *who, bool own, int32_t n, const uint8_t *d_grids, int32_t group,
                        void *d_scratch, int64_t *d_sum, double *d_scores, int32_t *d_nearest, int32_t *d_nearest_idx,
                        int32_t *d_pairwise, void *stream) {
  int rc = measures_2d_refuse(h, who);
  if (rc == PCGRL_OK) rc = diversity_check(who, !own, n, d_grids, group, d_scratch, d_sum);
  if (rc != PCGRL_OK || n == 0) return rc;
  ON_DEVICE(h->device);
  return diversity_enqueue(meas_args_2d(h, own, n, d_grids), meas_planes(h->p.n_tiles),
                           [h](const MeasWaveArgs &a, hipStream_t s) { return launch_measures(h->p, a, s); }, group, d_scratch,
                           d_sum, d_scores, d_nearest, d_nearest_idx, d_pairwise, stream);
}

extern "C" {

int32_t pcgrl_measures_tiles(pcgrl_handle h) {
  if (!h) return -1;
  return h->p.cfg.ndim == 2 ? h->p.n_tiles : 0;
}

int pcgrl_measures(pcgrl_handle h, int32_t *d_counts, int32_t *d_match, double *d_forms, double *d_entropy,
                   const double *d_entropy_tab, void *stream) {
  return measures_2d(h, "pcgrl_measures", true, h ? h->p.n_envs : 0, nullptr, d_counts, d_match, d_forms, d_entropy,
                     d_entropy_tab, stream);
}

int pcgrl_measures_for_grids(pcgrl_handle h, int32_t n, const uint8_t *d_grids, int32_t *d_counts, int32_t *d_match,
                             double *d_forms, double *d_entropy, const double *d_entropy_tab, void *stream) {
  return measures_2d(h, "pcgrl_measures_for_grids", false, n, d_grids, d_counts, d_match, d_forms, d_entropy, d_entropy_tab,
                     stream);
}

size_t pcgrl_diversity_scratch_bytes(pcgrl_handle h, int32_t n) {
  if (!h || n <= 0 || h->p.cfg.ndim != 2) return 0;
  return diversity_scratch_bytes(meas_planes(h->p.n_tiles), h->p.cfg.dims[0], h->p.cfg.dims[1], n);
}

int pcgrl_diversity(pcgrl_handle h, int32_t group, void *d_scratch, int64_t *d_sum, double *d_scores, int32_t *d_nearest,
                    int32_t *d_nearest_idx, int32_t *d_pairwise, void *stream) {
  return diversity_2d(h, "pcgrl_diversity", true, h ? h->p.n_envs : 0, nullptr, group, d_scratch, d_sum, d_scores, d_nearest,
                      d_nearest_idx, d_pairwise, stream);
}

int pcgrl_diversity_for_grids(pcgrl_handle h, int32_t n, const uint8_t *d_grids, int32_t group, void *d_scratch, int64_t *d_sum,
                              double *d_scores, int32_t *d_nearest, int32_t *d_nearest_idx, int32_t *d_pairwise, void *stream) {
  return diversity_2d(h, "pcgrl_diversity_for_grids", false, n, d_grids, group, d_scratch, d_sum, d_scores, d_nearest,
                      d_nearest_idx, d_pairwise, stream);
}

// ---------------------------------------------------------------------------------------------- multi-agent turtle stepping
// include/pcgrl_amd_multiagent.h; kernels in multiagent/pcgrl_multiagent.h
int pcgrl_ma_attach(pcgrl_handle h, int32_t n_agents, int32_t show_agents) {
  if (!h) return fail(PCGRL_EINVAL, "pcgrl_ma_attach: null handle");
  if (h->ma_on) return fail(PCGRL_EINVAL, "pcgrl_ma_attach: the engine is attached already");
  if (n_agents < 1 || n_agents > PCGRL_MA_MAX_AGENTS)
    return fail(PCGRL_EINVAL, "pcgrl_ma_attach: n_agents must be in [1, " + std::to_string(PCGRL_MA_MAX_AGENTS) + "]");
  const pcgrl_config &c = h->p.cfg;
  if (c.representation != PCGRL_REP_TURTLE)
    return fail(PCGRL_EUNSUPPORTED, "pcgrl_ma_attach: the turtle representation only (the reference's multi-agent narrow raises "
                                    "'Busted for now' and its multi-agent wide a TypeError)");
  if (c.problem != PCGRL_PROB_BINARY && c.problem != PCGRL_PROB_ZELDA)
    return fail(PCGRL_EUNSUPPORTED, "pcgrl_ma_attach: binary and zelda only (sokoban and the 3-D maze need the helper-wave and "
                                    "workspace machinery of their searches, which the multi-agent kernels do not carry)");
  if (c.static_tiles) return fail(PCGRL_EUNSUPPORTED, "pcgrl_ma_attach: not with static tiles");
  if (c.act_window[0] != 0 || c.act_window[1] != 0) return fail(PCGRL_EUNSUPPORTED, "pcgrl_ma_attach: not with an action patch");
  if (c.n_ctrl > 0) return fail(PCGRL_EUNSUPPORTED, "pcgrl_ma_attach: not with control metrics");
  if (h->sk_budget > 0) return fail(PCGRL_EUNSUPPORTED, "pcgrl_ma_attach: not with a solver budget");
  if (show_agents && n_agents == 1)
    return fail(PCGRL_EUNSUPPORTED, "pcgrl_ma_attach: show_agents needs more than one agent (the reference's "
                                    "ShowAgentRepresentation raises with one)");
  if (h->maybe_stale) return fail(PCGRL_EINVAL, "pcgrl_ma_attach: pcgrl_update has left statistics stale (pcgrl_refresh_stats first)");
  const int OH = c.obs_window[0], OW = c.obs_window[1], C = h->p.n_tiles + 1 + (show_agents ? 1 : 0);
  const int chunks = (OW * C + 15) / 16;
  const size_t lds = show_agents ? (size_t)(chunks * 16 + 16) * 65 : h->lds_bytes;
  if (lds > 160 * 1024) return fail(PCGRL_EUNSUPPORTED, "pcgrl_ma_attach: the observation rows with the occupancy channel exceed the LDS");
  ON_DEVICE(h->device);
  const size_t N = (size_t)h->p.n_envs, A = (size_t)n_agents;
  MaArgs a = {};
  a.n_agents = n_agents;
  a.show_agents = show_agents ? 1 : 0;
  a.obs_chunks = chunks;
  void *ptr[3] = {nullptr, nullptr, nullptr};
  const size_t bytes[3] = {N * A * 2 * sizeof(int32_t), N * 4 * sizeof(uint32_t), N * A * PCGRL_MAX_STATS * sizeof(int32_t)};
  for (int i = 0; i < 3; i++) {
    hipError_t err = hipMalloc(&ptr[i], bytes[i]);
    if (err == hipSuccess) {
      h->allocs.push_back(ptr[i]);  // (freed with the engine, also when a later allocation fails)
      err = hipMemset(ptr[i], 0, bytes[i]);
    }
    if (err != hipSuccess) return fail(PCGRL_EHIP, std::string("pcgrl_ma_attach: ") + hipGetErrorString(err));
  }
  a.pos = (int32_t *)ptr[0];
  a.side = (uint32_t *)ptr[1];
  a.last_stats = (int32_t *)ptr[2];
  h->ma = a;
  h->ma_lds = lds;
  h->ma_obs_bytes = (int64_t)OH * OW * C;
  h->ma_obs_shape[0] = OH;
  h->ma_obs_shape[1] = OW;
  h->ma_obs_shape[2] = C;
  h->ma_on = true;
  return PCGRL_OK;
}

int32_t pcgrl_ma_attached(pcgrl_handle h) { return h ? (h->ma_on ? 1 : 0) : -1; }

#define MA_ATTACHED(h, what)                                                                        \
  if (!(h)) return fail(PCGRL_EINVAL, std::string(what) + ": null handle");                         \
  if (!(h)->ma_on) return fail(PCGRL_EINVAL, std::string(what) + ": the engine is not attached (pcgrl_ma_attach)")

int pcgrl_ma_obs_shape(pcgrl_handle h, int32_t shape_out[4], int32_t *ndim_out) {
  MA_ATTACHED(h, "pcgrl_ma_obs_shape");
  if (!shape_out || !ndim_out) return fail(PCGRL_EINVAL, "pcgrl_ma_obs_shape: bad arguments");
  for (int i = 0; i < 4; i++) shape_out[i] = i < 3 ? h->ma_obs_shape[i] : 0;
  *ndim_out = 3;
  return PCGRL_OK;
}

int pcgrl_ma_observe(pcgrl_handle h, uint8_t *d_obs, void *stream) {
  MA_ATTACHED(h, "pcgrl_ma_observe");
  if (!d_obs) return fail(PCGRL_EINVAL, "pcgrl_ma_observe: bad arguments");
  ON_DEVICE(h->device);
  Params p = h->p;
  p.obs = d_obs;
  HIPCHK(launch_ma(MA_OBSERVE, p, h->lpe, h->ma, h->ma_lds, (hipStream_t)stream));
  return PCGRL_OK;
}

int pcgrl_ma_reset(pcgrl_handle h, const uint8_t *d_mask, const uint8_t *d_init_grids, const int32_t *d_init_pos, uint8_t *d_obs,
                   void *stream) {
  MA_ATTACHED(h, "pcgrl_ma_reset");
  if ((d_init_grids == nullptr) != (d_init_pos == nullptr))
    return fail(PCGRL_EINVAL, "pcgrl_ma_reset: injected maps and injected positions come together");
  ON_DEVICE(h->device);
  Params p = h->p;
  p.mask = d_mask;
  p.init_grids = d_init_grids;
  MaArgs a = h->ma;
  a.init_pos = d_init_pos;
  HIPCHK(launch_ma(MA_RESET, p, h->lpe, a, 0, (hipStream_t)stream));
  if (d_obs) {
    p.obs = d_obs;
    HIPCHK(launch_ma(MA_OBSERVE, p, h->lpe, h->ma, h->ma_lds, (hipStream_t)stream));
  }
  return PCGRL_OK;
}

int pcgrl_ma_step(pcgrl_handle h, const int32_t *d_actions, int32_t auto_reset, uint8_t *d_obs, float *d_reward, uint8_t *d_done,
                  int32_t *d_stats, uint8_t *d_done_all, void *stream) {
  MA_ATTACHED(h, "pcgrl_ma_step");
  if (!d_actions) return fail(PCGRL_EINVAL, "pcgrl_ma_step: bad arguments");
  ON_DEVICE(h->device);
  Params p = h->p;
  p.actions = d_actions;
  p.auto_reset = auto_reset;
  p.obs = d_obs;
  p.reward = d_reward;
  p.done = d_done;
  p.stats_out = d_stats;
  MaArgs a = h->ma;
  a.done_all = d_done_all;
  HIPCHK(launch_ma(MA_STEP, p, h->lpe, a, h->ma_lds, (hipStream_t)stream));
  return PCGRL_OK;
}

int pcgrl_ma_get_state(pcgrl_handle h, int32_t *d_pos, uint32_t *d_side, int32_t *d_last_stats, void *stream) {
  MA_ATTACHED(h, "pcgrl_ma_get_state");
  ON_DEVICE(h->device);
  const size_t N = (size_t)h->p.n_envs, A = (size_t)h->ma.n_agents;
  hipStream_t s = (hipStream_t)stream;
  if (d_pos) HIPCHK(hipMemcpyAsync(d_pos, h->ma.pos, N * A * 2 * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  if (d_side) HIPCHK(hipMemcpyAsync(d_side, h->ma.side, N * 4 * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
  if (d_last_stats)
    HIPCHK(hipMemcpyAsync(d_last_stats, h->ma.last_stats, N * A * PCGRL_MAX_STATS * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  return PCGRL_OK;
}

int pcgrl_ma_set_state(pcgrl_handle h, const uint8_t *d_mask, const int32_t *d_pos, const uint32_t *d_side,
                       const int32_t *d_last_stats, void *stream) {
  MA_ATTACHED(h, "pcgrl_ma_set_state");
  if (!d_pos && !d_side && !d_last_stats) return PCGRL_OK;
  ON_DEVICE(h->device);
  Params p = h->p;
  p.mask = d_mask;
  MaArgs a = h->ma;
  a.init_pos = d_pos;
  a.in_side = d_side;
  a.in_stats = d_last_stats;
  HIPCHK(launch_ma(MA_SET_STATE, p, h->lpe, a, 0, (hipStream_t)stream));
  return PCGRL_OK;
}

// ---------------------------------------------------------------------------------------------- Super Mario Bros levels
// include/pcgrl_amd_smb.h; kernel in smb/pcgrl_smb.h.  No handle: the evaluation is a function of the maps and the config.
static bool smb_shape_ok(int32_t h, int32_t w) { return h >= SMB_MIN_H && h <= SMB_MAX_H && w >= 1 && w <= SMB_MAX_W; }

static int smb_check_shape(const char *who, int32_t h, int32_t w, int32_t power) {
  if (!smb_shape_ok(h, w))
    return fail(PCGRL_EUNSUPPORTED, std::string(who) + ": maps of 4..16 rows and 1..128 columns only (with fewer than 4 rows the "
                                                       "reference's level has no exit)");
  if (power < 1 || power > SMB_MAX_POWER)
    return fail(PCGRL_EUNSUPPORTED, std::string(who) + ": solver_power must be in [1, " + std::to_string(SMB_MAX_POWER) + "]");
  return PCGRL_OK;
}

int64_t pcgrl_smb_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t solver_power) {
  if (n < 1 || smb_check_shape("pcgrl_smb_workspace_bytes", h, w, solver_power) != PCGRL_OK) return -1;
  return (int64_t)n * smb_ws_stride(solver_power);
}

int pcgrl_smb_evaluate(const pcgrl_smb_config *cfg, int32_t n, const uint8_t *d_grids, void *d_workspace, int64_t workspace_bytes,
                       int32_t cap, int32_t jump_cap, int32_t *d_stats, double *d_loss, int8_t *d_moves, int32_t *d_length,
                       int16_t *d_jump_locs, int32_t *d_play, uint32_t *d_error, void *stream) {
  const char *who = "pcgrl_smb_evaluate";
  if (!cfg || !d_grids || !d_stats || n < 1) return fail(PCGRL_EINVAL, std::string(who) + ": bad arguments");
  if (cap < 0 || jump_cap < 0 || (d_moves && cap < 1) || (d_jump_locs && jump_cap < 1))
    return fail(PCGRL_EINVAL, std::string(who) + ": cap and jump_cap must be at least 1 where their output is given");
  const int rc = smb_check_shape(who, cfg->h, cfg->w, cfg->solver_power);
  if (rc != PCGRL_OK) return rc;
  const int64_t stride = smb_ws_stride(cfg->solver_power);
  const int ws = workspace_check(who, d_workspace, 8, workspace_bytes, (int64_t)n * stride, "pcgrl_smb_workspace_bytes");
  if (ws != PCGRL_OK) return ws;
  SmbArgs a = {};
  a.h = cfg->h;
  a.w = cfg->w;
  a.power = cfg->solver_power;
  a.n = n;
  a.grids = d_grids;
  a.ws = (uint8_t *)d_workspace;
  a.ws_stride = stride;
  a.cap = cap;
  a.jump_cap = jump_cap;
  a.stats = d_stats;
  a.loss = d_loss;
  a.moves = d_moves;
  a.length = d_length;
  a.jump_locs = d_jump_locs;
  a.play = d_play;
  a.error = d_error;
  copy_targets<SMB_STATS>(a, cfg);
  HIPCHK(launch_smb(a, (hipStream_t)stream));
  return PCGRL_OK;
}

// ---------------------------------------------------------------------------------------------- Lode Runner levels
// include/pcgrl_amd_loderunner.h; kernel in loderunner/pcgrl_loderunner.h.  No handle, as for the Mario levels above.
static bool lr_shape_ok(int32_t h, int32_t w) { return h >= 1 && h <= LR_MAX_H && w >= 1 && w <= LR_MAX_W; }

static int lr_check_shape(const char *who, int32_t h, int32_t w) {
  if (!lr_shape_ok(h, w))
    return fail(PCGRL_EUNSUPPORTED, std::string(who) + ": maps of 1..16 rows and 1..32 columns only");
  return PCGRL_OK;
}

int64_t pcgrl_loderunner_workspace_bytes(int32_t n, int32_t h, int32_t w) {
  if (n < 1 || lr_check_shape("pcgrl_loderunner_workspace_bytes", h, w) != PCGRL_OK) return -1;
  return (int64_t)lr_blocks(n, h, w) * lr_ws_stride(h, w);
}

// the argument checks and the kernel arguments that pcgrl_loderunner_evaluate and pcgrl_loderunner_routes share
static int lr_fill_args(const char *who, LrArgs &a, const pcgrl_loderunner_config *cfg, int32_t n, const uint8_t *d_grids,
                        void *d_workspace, int64_t workspace_bytes, int32_t gold_cap, double *d_stats, double *d_loss,
                        int32_t *d_play, int8_t *d_gold_state, int16_t *d_gold_dist, uint32_t *d_error) {
  if (!cfg || !d_grids || !d_stats || n < 1) return fail(PCGRL_EINVAL, std::string(who) + ": bad arguments");
  if (gold_cap < 0) return fail(PCGRL_EINVAL, std::string(who) + ": gold_cap must not be negative");
  const int rc = lr_check_shape(who, cfg->h, cfg->w);
  if (rc != PCGRL_OK) return rc;
  const int64_t stride = lr_ws_stride(cfg->h, cfg->w);
  const int ws = workspace_check(who, d_workspace, 4, workspace_bytes, (int64_t)lr_blocks(n, cfg->h, cfg->w) * stride,
                                 "pcgrl_loderunner_workspace_bytes");
  if (ws != PCGRL_OK) return ws;
  a = LrArgs{};
  a.h = cfg->h;
  a.w = cfg->w;
  a.n = n;
  a.grids = d_grids;
  a.ws = (uint32_t *)d_workspace;
  a.ws_stride = stride;
  a.gold_cap = gold_cap;
  a.stats = d_stats;
  a.loss = d_loss;
  a.play = d_play;
  a.gold_state = d_gold_state;
  a.gold_dist = d_gold_dist;
  a.error = d_error;
  copy_targets<LR_STATS>(a, cfg);
  return PCGRL_OK;
}

int pcgrl_loderunner_evaluate(const pcgrl_loderunner_config *cfg, int32_t n, const uint8_t *d_grids, void *d_workspace,
                              int64_t workspace_bytes, int32_t gold_cap, double *d_stats, double *d_loss, int32_t *d_play,
                              int8_t *d_gold_state, int16_t *d_gold_dist, uint32_t *d_error, void *stream) {
  LrArgs a;
  const int rc = lr_fill_args("pcgrl_loderunner_evaluate", a, cfg, n, d_grids, d_workspace, workspace_bytes, gold_cap, d_stats,
                              d_loss, d_play, d_gold_state, d_gold_dist, d_error);
  if (rc != PCGRL_OK) return rc;
  HIPCHK(launch_loderunner(a, (hipStream_t)stream));
  return PCGRL_OK;
}

// include/pcgrl_amd_loderunner_routes.h; kernel in loderunner/pcgrl_loderunner_routes.h
int pcgrl_loderunner_routes(const pcgrl_loderunner_config *cfg, int32_t n, const uint8_t *d_grids, void *d_workspace,
                            int64_t workspace_bytes, int32_t gold_cap, int32_t route_cap, double *d_stats, double *d_loss,
                            int32_t *d_play, int8_t *d_gold_state, int16_t *d_gold_dist, int32_t *d_gold_off,
                            int16_t *d_gold_back, int16_t *d_coords, int8_t *d_moves, int32_t *d_tour_len, uint32_t *d_error,
                            void *stream) {
  const char *who = "pcgrl_loderunner_routes";
  LrRouteArgs a = {};
  const int rc = lr_fill_args(who, a.lr, cfg, n, d_grids, d_workspace, workspace_bytes, gold_cap, d_stats, d_loss, d_play,
                              d_gold_state, d_gold_dist, d_error);
  if (rc != PCGRL_OK) return rc;
  if (route_cap < 0) return fail(PCGRL_EINVAL, std::string(who) + ": route_cap must not be negative");
  if (route_cap > 0 && !d_coords) return fail(PCGRL_EINVAL, std::string(who) + ": route_cap > 0 needs d_coords");
  a.route_cap = route_cap;
  a.coords = d_coords;
  a.moves = d_moves;
  a.tour_len = d_tour_len;
  a.gold_off = d_gold_off;
  a.gold_back = d_gold_back;
  HIPCHK(launch_loderunner_routes(a, (hipStream_t)stream));
  return PCGRL_OK;
}

}  // extern "C"

// ------------------------------------------------------------ Lode Runner maps: level measures and pairwise Hamming diversity
// include/pcgrl_amd_loderunner_measures.h; the measure / pack kernel in loderunner/pcgrl_loderunner_measures.h, the pairwise
// kernels those of measures/pcgrl_measures.h; the host path is the one of "measures and diversity" above.

extern "C" {

int pcgrl_loderunner_measures_for_grids(int32_t h, int32_t w, int32_t n, const uint8_t *d_grids, int32_t *d_counts,
                                        int32_t *d_match, double *d_forms, double *d_entropy, const double *d_entropy_tab,
                                        void *stream) {
  return measures_for_grids("pcgrl_loderunner_measures_for_grids", lr_check_shape, launch_lr_measures, h, w, n, d_grids,
                            d_counts, d_match, d_forms, d_entropy, d_entropy_tab, stream);
}

size_t pcgrl_loderunner_diversity_scratch_bytes(int32_t h, int32_t w, int32_t n) {
  if (n <= 0 || !lr_shape_ok(h, w)) return 0;
  return diversity_scratch_bytes(LR_MEAS_PLANES, h, w, n);
}

int pcgrl_loderunner_diversity_for_grids(int32_t h, int32_t w, int32_t n, const uint8_t *d_grids, int32_t group,
                                         void *d_scratch, int64_t *d_sum, double *d_scores, int32_t *d_nearest,
                                         int32_t *d_nearest_idx, int32_t *d_pairwise, void *stream) {
  return diversity_for_grids("pcgrl_loderunner_diversity_for_grids", lr_check_shape, LR_MEAS_PLANES, launch_lr_measures, h, w,
                             n, d_grids, group, d_scratch, d_sum, d_scores, d_nearest, d_nearest_idx, d_pairwise, stream);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------- microstructure levels
// include/pcgrl_amd_microstructure.h; kernels in microstructure/pcgrl_microstructure.h.  No handle and no workspace.  The
// measures and the diversity are the (2, 1, 4096) instantiation of the wave body through the host path of "measures and
// diversity" above.
static bool ms_shape_ok(int32_t h, int32_t w) { return h >= 1 && h <= MS_MAX_H && w >= 1 && w <= MS_MAX_W; }

static int ms_check_shape(const char *who, int32_t h, int32_t w) {
  if (!ms_shape_ok(h, w))
    return fail(PCGRL_EUNSUPPORTED, std::string(who) + ": maps of 1..64 rows and 1..64 columns only");
  return PCGRL_OK;
}

extern "C" {

int pcgrl_microstructure_evaluate(const pcgrl_microstructure_config *cfg, int32_t n, const uint8_t *d_grids, int32_t region_cap,
                                  double *d_stats, double *d_loss, int32_t *d_regions, int16_t *d_region_rec,
                                  double *d_region_tort, uint32_t *d_error, void *stream) {
  const char *who = "pcgrl_microstructure_evaluate";
  if (!cfg || !d_grids || !d_stats || n < 1) return fail(PCGRL_EINVAL, std::string(who) + ": bad arguments");
  if (region_cap < 0) return fail(PCGRL_EINVAL, std::string(who) + ": region_cap must not be negative");
  const int rc = ms_check_shape(who, cfg->h, cfg->w);
  if (rc != PCGRL_OK) return rc;
  MsArgs a{};
  a.h = cfg->h;
  a.w = cfg->w;
  a.n = n;
  a.grids = d_grids;
  a.region_cap = region_cap;
  a.stats = d_stats;
  a.loss = d_loss;
  a.regions = d_regions;
  a.region_rec = region_cap > 0 ? d_region_rec : nullptr;
  a.region_tort = region_cap > 0 ? d_region_tort : nullptr;
  a.error = d_error;
  copy_targets<MS_STATS>(a, cfg);
  HIPCHK(launch_microstructure(a, (hipStream_t)stream));
  return PCGRL_OK;
}

int pcgrl_microstructure_measures_for_grids(int32_t h, int32_t w, int32_t n, const uint8_t *d_grids, int32_t *d_counts,
                                            int32_t *d_match, double *d_forms, double *d_entropy, const double *d_entropy_tab,
                                            void *stream) {
  return measures_for_grids("pcgrl_microstructure_measures_for_grids", ms_check_shape, launch_ms_measures, h, w, n, d_grids,
                            d_counts, d_match, d_forms, d_entropy, d_entropy_tab, stream);
}

size_t pcgrl_microstructure_diversity_scratch_bytes(int32_t h, int32_t w, int32_t n) {
  if (n <= 0 || !ms_shape_ok(h, w)) return 0;
  return diversity_scratch_bytes(MS_MEAS_PLANES, h, w, n);
}

int pcgrl_microstructure_diversity_for_grids(int32_t h, int32_t w, int32_t n, const uint8_t *d_grids, int32_t group,
                                             void *d_scratch, int64_t *d_sum, double *d_scores, int32_t *d_nearest,
                                             int32_t *d_nearest_idx, int32_t *d_pairwise, void *stream) {
  return diversity_for_grids("pcgrl_microstructure_diversity_for_grids", ms_check_shape, MS_MEAS_PLANES, launch_ms_measures, h,
                             w, n, d_grids, group, d_scratch, d_sum, d_scores, d_nearest, d_nearest_idx, d_pairwise, stream);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------- solver play-throughs
// What the entry points of the Dangerous Dave and MiniDungeon levels below share (playthrough/pcgrl_playthrough.h): `who` names
// the caller in the error text, `ws_name` the function whose size the workspace must have, `launch` is the game's kernel.
static bool pt_shape_ok(int32_t h, int32_t w) { return h >= 1 && h <= PT_MAX_H && w >= 1 && w <= PT_MAX_W; }

static int pt_check_shape(const char *who, int32_t h, int32_t w) {
  if (!pt_shape_ok(h, w))
    return fail(PCGRL_EUNSUPPORTED, std::string(who) + ": maps of 1..16 rows and 1..32 columns only");
  return PCGRL_OK;
}

static int pt_check_power(const char *who, int32_t power) {
  if (power < 1 || power > PT_MAX_POWER)
    return fail(PCGRL_EUNSUPPORTED, std::string(who) + ": solver_power must be in [1, " + std::to_string(PT_MAX_POWER) + "]");
  return PCGRL_OK;
}

static int64_t pt_workspace_bytes(const char *who, int32_t n, int32_t h, int32_t w, int32_t power) {
  if (n < 1) {
    fail(PCGRL_EINVAL, std::string(who) + ": n must be at least 1");
    return -1;
  }
  if (pt_check_shape(who, h, w) != PCGRL_OK || pt_check_power(who, power) != PCGRL_OK) return -1;
  return (int64_t)n * pt_ws_stride(power);
}

static int pt_evaluate(const char *who, const char *ws_name, hipError_t (*launch)(const PtArgs &, hipStream_t), int32_t h,
                       int32_t w, int32_t power, int32_t n, const uint8_t *d_grids, void *d_workspace, int64_t workspace_bytes,
                       int32_t move_cap, int32_t *d_stats, int8_t *d_moves, int32_t *d_length, int32_t *d_play,
                       uint32_t *d_error, void *stream) {
  if (!d_grids || !d_stats || n < 1) return fail(PCGRL_EINVAL, std::string(who) + ": bad arguments");
  if (move_cap < 0) return fail(PCGRL_EINVAL, std::string(who) + ": move_cap must not be negative");
  int rc = pt_check_shape(who, h, w);
  if (rc == PCGRL_OK) rc = pt_check_power(who, power);
  if (rc != PCGRL_OK) return rc;
  const int64_t stride = pt_ws_stride(power);
  rc = workspace_check(who, d_workspace, 16, workspace_bytes, (int64_t)n * stride, ws_name);
  if (rc != PCGRL_OK) return rc;
  PtArgs a{};
  a.h = h;
  a.w = w;
  a.power = power;
  a.n = n;
  a.grids = d_grids;
  a.ws = (uint8_t *)d_workspace;
  a.ws_stride = stride;
  a.hash_cap = pt_hash_cap(power);
  a.cap = move_cap;
  a.stats = d_stats;
  a.moves = move_cap > 0 ? d_moves : nullptr;
  a.length = d_length;
  a.play = d_play;
  a.error = d_error;
  HIPCHK(launch(a, (hipStream_t)stream));
  return PCGRL_OK;
}

// ---------------------------------------------------------------------------------------------- Dangerous Dave levels
// include/pcgrl_amd_ddave.h; kernels in ddave/pcgrl_ddave.h.  No handle, as for the Mario levels above.  The measures and the
// diversity are the (7, 3, 512) instantiation of the wave body through the host path of "measures and diversity" above.
extern "C" {

int64_t pcgrl_ddave_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t solver_power) {
  return pt_workspace_bytes("pcgrl_ddave_workspace_bytes", n, h, w, solver_power);
}

int pcgrl_ddave_evaluate(const pcgrl_ddave_config *cfg, int32_t n, const uint8_t *d_grids, void *d_workspace,
                         int64_t workspace_bytes, int32_t move_cap, int32_t *d_stats, int8_t *d_moves, int32_t *d_length,
                         int32_t *d_play, uint32_t *d_error, void *stream) {
  const char *who = "pcgrl_ddave_evaluate";
  if (!cfg) return fail(PCGRL_EINVAL, std::string(who) + ": bad arguments");
  return pt_evaluate(who, "pcgrl_ddave_workspace_bytes", launch_ddave, cfg->h, cfg->w, cfg->solver_power, n, d_grids,
                     d_workspace, workspace_bytes, move_cap, d_stats, d_moves, d_length, d_play, d_error, stream);
}

int pcgrl_ddave_measures_for_grids(int32_t h, int32_t w, int32_t n, const uint8_t *d_grids, int32_t *d_counts, int32_t *d_match,
                                   double *d_forms, double *d_entropy, const double *d_entropy_tab, void *stream) {
  return measures_for_grids("pcgrl_ddave_measures_for_grids", pt_check_shape, launch_dd_measures, h, w, n, d_grids, d_counts,
                            d_match, d_forms, d_entropy, d_entropy_tab, stream);
}

size_t pcgrl_ddave_diversity_scratch_bytes(int32_t h, int32_t w, int32_t n) {
  if (n <= 0 || !pt_shape_ok(h, w)) return 0;
  return diversity_scratch_bytes(DD_MEAS_PLANES, h, w, n);
}

int pcgrl_ddave_diversity_for_grids(int32_t h, int32_t w, int32_t n, const uint8_t *d_grids, int32_t group, void *d_scratch,
                                    int64_t *d_sum, double *d_scores, int32_t *d_nearest, int32_t *d_nearest_idx,
                                    int32_t *d_pairwise, void *stream) {
  return diversity_for_grids("pcgrl_ddave_diversity_for_grids", pt_check_shape, DD_MEAS_PLANES, launch_dd_measures, h, w, n,
                             d_grids, group, d_scratch, d_sum, d_scores, d_nearest, d_nearest_idx, d_pairwise, stream);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------- MiniDungeon levels
// include/pcgrl_amd_mdungeon.h; kernels in mdungeon/pcgrl_mdungeon.h.  No handle, as for the Dangerous Dave levels above.  The
// measures and the diversity are the (8, 3, 512) instantiation of the wave body through the host path of "measures and
// diversity" above.
extern "C" {

int64_t pcgrl_mdungeon_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t solver_power) {
  return pt_workspace_bytes("pcgrl_mdungeon_workspace_bytes", n, h, w, solver_power);
}

int pcgrl_mdungeon_evaluate(const pcgrl_mdungeon_config *cfg, int32_t n, const uint8_t *d_grids, void *d_workspace,
                            int64_t workspace_bytes, int32_t move_cap, int32_t *d_stats, int8_t *d_moves, int32_t *d_length,
                            int32_t *d_play, uint32_t *d_error, void *stream) {
  const char *who = "pcgrl_mdungeon_evaluate";
  if (!cfg) return fail(PCGRL_EINVAL, std::string(who) + ": bad arguments");
  return pt_evaluate(who, "pcgrl_mdungeon_workspace_bytes", launch_mdungeon, cfg->h, cfg->w, cfg->solver_power, n, d_grids,
                     d_workspace, workspace_bytes, move_cap, d_stats, d_moves, d_length, d_play, d_error, stream);
}

int pcgrl_mdungeon_measures_for_grids(int32_t h, int32_t w, int32_t n, const uint8_t *d_grids, int32_t *d_counts,
                                      int32_t *d_match, double *d_forms, double *d_entropy, const double *d_entropy_tab,
                                      void *stream) {
  return measures_for_grids("pcgrl_mdungeon_measures_for_grids", pt_check_shape, launch_md_measures, h, w, n, d_grids,
                            d_counts, d_match, d_forms, d_entropy, d_entropy_tab, stream);
}

size_t pcgrl_mdungeon_diversity_scratch_bytes(int32_t h, int32_t w, int32_t n) {
  if (n <= 0 || !pt_shape_ok(h, w)) return 0;
  return diversity_scratch_bytes(MD_MEAS_PLANES, h, w, n);
}

int pcgrl_mdungeon_diversity_for_grids(int32_t h, int32_t w, int32_t n, const uint8_t *d_grids, int32_t group, void *d_scratch,
                                       int64_t *d_sum, double *d_scores, int32_t *d_nearest, int32_t *d_nearest_idx,
                                       int32_t *d_pairwise, void *stream) {
  return diversity_for_grids("pcgrl_mdungeon_diversity_for_grids", pt_check_shape, MD_MEAS_PLANES, launch_md_measures, h, w, n,
                             d_grids, group, d_scratch, d_sum, d_scores, d_nearest, d_nearest_idx, d_pairwise, stream);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------- 3-D holey dungeon and maze levels
// include/pcgrl_amd_mc3d_holey.h; kernel in mc3d_holey/pcgrl_mc3d_holey.h.  No handle, as for the MiniDungeon levels above.
static int h3_check_shape(const char *who, int32_t z, int32_t y, int32_t x) {
  if (z < 3 || z > H3_MAX || y < 3 || y > H3_MAX || x < 3 || x > H3_MAX)
    return fail(PCGRL_EUNSUPPORTED, std::string(who) + ": interiors of 3..16 cells along each axis only");
  return PCGRL_OK;
}

extern "C" {

int64_t pcgrl_mc3d_holey_workspace_bytes(int32_t blocks, int32_t z, int32_t y, int32_t x) {
  const char *who = "pcgrl_mc3d_holey_workspace_bytes";
  if (blocks < 1) {
    fail(PCGRL_EINVAL, std::string(who) + ": blocks must be at least 1");
    return -1;
  }
  if (h3_check_shape(who, z, y, x) != PCGRL_OK) return -1;
  return (int64_t)blocks * h3_ws_stride(h3_cells(z, y, x));
}

int pcgrl_mc3d_holey_evaluate(const pcgrl_mc3d_holey_config *cfg, int32_t n, const uint8_t *d_grids, const int32_t *d_holes,
                              void *d_workspace, int64_t workspace_bytes, int32_t route_cap, int32_t *d_stats, double *d_loss,
                              int32_t *d_play, uint32_t *d_error, int16_t *d_coords, int32_t *d_route_len, int32_t *d_leg_len,
                              int16_t *d_coords2, int32_t *d_route2_len, uint8_t *d_overlay, uint8_t *d_overlay2, void *stream) {
  const char *who = "pcgrl_mc3d_holey_evaluate";
  if (!cfg || !d_grids || !d_holes || !d_stats || n < 1) return fail(PCGRL_EINVAL, std::string(who) + ": bad arguments");
  if (route_cap < 0) return fail(PCGRL_EINVAL, std::string(who) + ": route_cap must not be negative");
  if (cfg->problem != PCGRL_MC3D_HOLEY_DUNGEON && cfg->problem != PCGRL_MC3D_HOLEY_MAZE)
    return fail(PCGRL_EINVAL, std::string(who) + ": problem must be 0 (dungeon) or 1 (maze)");
  const int rc = h3_check_shape(who, cfg->z, cfg->y, cfg->x);
  if (rc != PCGRL_OK) return rc;
  const int cells = h3_cells(cfg->z, cfg->y, cfg->x);
  const int64_t stride = h3_ws_stride(cells);
  const int ws =
      workspace_check(who, d_workspace, 16, workspace_bytes, stride, "pcgrl_mc3d_holey_workspace_bytes(1, z, y, x)");
  if (ws != PCGRL_OK) return ws;
  H3Args a{};
  a.problem = cfg->problem;
  a.Z = cfg->z, a.Y = cfg->y, a.X = cfg->x;
  a.n = n;
  a.grids = d_grids;
  a.holes = d_holes;
  a.ws = (uint8_t *)d_workspace;
  a.ws_stride = stride;
  a.qcap = h3_qcap(cells);
  a.route_cap = route_cap;
  a.stats = d_stats;
  a.loss = d_loss;
  a.play = d_play;
  a.error = d_error;
  a.coords = route_cap > 0 ? d_coords : nullptr;
  a.route_len = d_route_len;
  a.leg_len = d_leg_len;
  a.coords2 = route_cap > 0 ? d_coords2 : nullptr;
  a.route2_len = d_route2_len;
  a.overlay = d_overlay;
  a.overlay2 = d_overlay2;
  for (int k = 0; k < H3_MAX_STATS; k++) a.weight[k] = cfg->weight[k], a.trg_lo[k] = cfg->trg_lo[k], a.trg_hi[k] = cfg->trg_hi[k];
  const int64_t slots = workspace_bytes / stride;
  HIPCHK(launch_mc3d_holey(a, (int)(slots < n ? slots : n), (hipStream_t)stream));
  return PCGRL_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------- Super Mario Bros environments
// include/pcgrl_amd_smb_env.h; kernels in smb/pcgrl_smb_env.h.  A handle of its own: the engine above does not know the problem.

struct pcgrl_smb_env {
  pcgrl_smb_env_config cfg;
  int device = 0;
  SmbEnvArgs a = {};
  std::vector<void *> allocs;
  int32_t budget = 0;       // include/pcgrl_amd_smb_ready.h: 0 = synchronous stepping
  SmbPark *park = nullptr;  // [n], allocated by the first pcgrl_smb_ready_set_budget
  uint8_t *state_hdr = nullptr;            // include/pcgrl_amd_smb_state.h: the image's 256-byte header, pinned and mapped
  const uint8_t *state_hdr_dev = nullptr;  // the same block as the device sees it
  SmbDrawState *draw = nullptr;            // include/pcgrl_amd_smb_rollout.h: the draw counter of the device-drawn actions
  SmbCtrlCfg ctrl = {};                    // include/pcgrl_amd_smb_ctrl.h: n_ctrl 0 = not controllable (the host's copy)
  bool touched = false;                    // a reset, a state set or an import has run: too late to attach controls
};

static hipError_t smb_state_header_create(pcgrl_smb_env *e);

static int smb_env_check(const char *who, const pcgrl_smb_env_config *c) {
  if (!c) return fail(PCGRL_EINVAL, std::string(who) + ": null config");
  const int rc = smb_check_shape(who, c->h, c->w, c->solver_power);
  if (rc != PCGRL_OK) return rc;
  if (c->representation == PCGRL_REP_WIDE)
    return fail(PCGRL_EUNSUPPORTED, std::string(who) + ": the wide representation is not stepped for smb (the reference's wide "
                                                       "fails on a non-square map: wide_rep.py:42, IndexError)");
  if (c->representation != PCGRL_REP_NARROW && c->representation != PCGRL_REP_TURTLE)
    return fail(PCGRL_EINVAL, std::string(who) + ": unknown representation");
  for (int k = 0; k < 2; k++)
    if (c->obs_window[k] < 1 || c->obs_window[k] > 255)
      return fail(PCGRL_EUNSUPPORTED, std::string(who) + ": obs_window entries must be in 1..255 (the reference keeps the pad as "
                                                         "int8 and fails above: 'index can't contain negative values')");
  if (c->n_envs < 1 || c->max_iterations < 0 || c->max_changes < -1)
    return fail(PCGRL_EINVAL, std::string(who) + ": n_envs must be at least 1, max_iterations >= 0 and max_changes >= -1");
  return PCGRL_OK;
}

extern "C" {

int64_t pcgrl_smb_env_workspace_bytes(const pcgrl_smb_env_config *cfg) {
  if (smb_env_check("pcgrl_smb_env_workspace_bytes", cfg) != PCGRL_OK) return -1;
  return (int64_t)cfg->n_envs * smb_ws_stride(cfg->solver_power);
}

int64_t pcgrl_smb_env_obs_bytes(const pcgrl_smb_env_config *cfg) {
  if (smb_env_check("pcgrl_smb_env_obs_bytes", cfg) != PCGRL_OK) return -1;
  return (int64_t)cfg->obs_window[0] * cfg->obs_window[1] * (SMB_TILES + 1);
}

int pcgrl_smb_env_create(const pcgrl_smb_env_config *cfg, int32_t device, void *d_workspace, int64_t workspace_bytes,
                         pcgrl_smb_env_handle *out) {
  const char *who = "pcgrl_smb_env_create";
  if (!out) return fail(PCGRL_EINVAL, std::string(who) + ": null out");
  const int rc = smb_env_check(who, cfg);
  if (rc != PCGRL_OK) return rc;
  const int64_t stride = smb_ws_stride(cfg->solver_power);
  const int ws = workspace_check(who, d_workspace, 8, workspace_bytes, (int64_t)cfg->n_envs * stride,
                                 "pcgrl_smb_env_workspace_bytes");
  if (ws != PCGRL_OK) return ws;
  if (device < 0) return fail(PCGRL_EINVAL, std::string(who) + ": bad device");
  ON_DEVICE(device);
  pcgrl_smb_env *e = new pcgrl_smb_env();
  e->cfg = *cfg;
  e->device = device;
  SmbEnvArgs &a = e->a;
  a.h = cfg->h;
  a.w = cfg->w;
  a.rep = cfg->representation;
  a.oh = cfg->obs_window[0];
  a.ow = cfg->obs_window[1];
  a.max_iterations = cfg->max_iterations;
  a.max_changes = cfg->max_changes;
  a.power = cfg->solver_power;
  a.n = cfg->n_envs;
  // H * W rounded up to 16 on hipMalloc's aligned base: what the generic staging of measures/pcgrl_measures_wave.h needs to
  // read an env's rows with no load outside them
  a.map_stride = (cfg->h * cfg->w + 15) / 16 * 16;
  a.ws = (uint8_t *)d_workspace;
  a.ws_stride = stride;
  copy_targets<SMB_STATS>(a, cfg);
  const int cells = cfg->h * cfg->w, cpl = (cells + 63) / 64;
  const std::vector<JumpEntry> jt = make_jump_table(64, cpl, cells);
  const size_t n = (size_t)cfg->n_envs;
  auto alloc = [&](void **ptr, size_t bytes) {
    hipError_t he = hipMalloc(ptr, bytes);
    if (he == hipSuccess) {
      e->allocs.push_back(*ptr);
      he = hipMemset(*ptr, 0, bytes);
    }
    return he;
  };
  hipError_t he = alloc((void **)&a.maps, n * a.map_stride);
  if (he == hipSuccess) he = alloc((void **)&a.st, n * sizeof(SmbEnvState));
  if (he == hipSuccess) he = alloc((void **)&a.rng, n * sizeof(RngState));
  if (he == hipSuccess) he = alloc((void **)&a.jump, jt.size() * sizeof(JumpEntry));
  if (he == hipSuccess) he = alloc((void **)&a.err, 4 * sizeof(int32_t));
  if (he == hipSuccess) he = alloc((void **)&e->draw, sizeof(SmbDrawState));
  if (he == hipSuccess) he = hipMemcpy((void *)a.jump, jt.data(), jt.size() * sizeof(JumpEntry), hipMemcpyHostToDevice);
  if (he == hipSuccess) he = smb_state_header_create(e);
  if (he != hipSuccess) {
    pcgrl_smb_env_destroy(e);
    return fail(PCGRL_EHIP, std::string(who) + ": " + hipGetErrorString(he));
  }
  *out = e;
  std::vector<uint64_t> seeds(n);
  for (size_t i = 0; i < n; i++) seeds[i] = (uint64_t)i;
  return pcgrl_smb_env_seed(e, seeds.data());
}

void pcgrl_smb_env_destroy(pcgrl_smb_env_handle h) {
  if (!h) return;
  DeviceGuard guard(h->device);
  for (void *p : h->allocs) (void)hipFree(p);
  if (h->state_hdr) (void)hipHostFree(h->state_hdr);
  delete h;
}

int pcgrl_smb_env_seed(pcgrl_smb_env_handle h, const uint64_t *seeds) {
  if (!h || !seeds) return fail(PCGRL_EINVAL, "pcgrl_smb_env_seed: bad arguments");
  ON_DEVICE(h->device);
  std::vector<RngState> r(h->a.n);
  for (int i = 0; i < h->a.n; i++) {
    pcg64_seed_state(seeds[i], r[i].rep);
    memcpy(r[i].prob, r[i].rep, sizeof(r[i].rep));  // envs/pcgrl_env.py:142-146: the same seed for both streams
  }
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(h->a.rng, r.data(), r.size() * sizeof(RngState), hipMemcpyHostToDevice));
  return PCGRL_OK;
}

int pcgrl_smb_env_reset(pcgrl_smb_env_handle h, const uint8_t *d_mask, const uint8_t *d_init_grids, const int32_t *d_init_pos,
                        uint8_t *d_obs, void *stream) {
  if (!h) return fail(PCGRL_EINVAL, "pcgrl_smb_env_reset: null handle");
  if ((uintptr_t)d_obs & 15u) return fail(PCGRL_EINVAL, "pcgrl_smb_env_reset: the observation must be 16-byte aligned");
  if (d_init_pos && !d_init_grids) return fail(PCGRL_EINVAL, "pcgrl_smb_env_reset: init_pos needs init_grids");
  ON_DEVICE(h->device);
  SmbEnvArgs a = h->a;
  a.mask = d_mask;
  a.init_grids = d_init_grids;
  a.init_pos = d_init_pos;
  a.obs = d_obs;
  h->touched = true;
  if (h->budget > 0) {  // include/pcgrl_amd_smb_ready.h: the new levels' searches run under the budget
    SmbReadyArgs ra = {a, h->park, h->budget, nullptr};
    HIPCHK(launch_smb_ready_reset(ra, (hipStream_t)stream));
    return PCGRL_OK;
  }
  HIPCHK(launch_smb_env(SMB_ENV_RESET, a, (hipStream_t)stream));
  return PCGRL_OK;
}

int pcgrl_smb_env_step(pcgrl_smb_env_handle h, const int32_t *d_actions, int32_t auto_reset, uint8_t *d_obs, float *d_reward,
                       double *d_reward64, uint8_t *d_done, int32_t *d_stats, void *stream) {
  if (!h || !d_actions) return fail(PCGRL_EINVAL, "pcgrl_smb_env_step: null handle or actions");
  if ((uintptr_t)d_obs & 15u) return fail(PCGRL_EINVAL, "pcgrl_smb_env_step: the observation must be 16-byte aligned");
  if (h->budget > 0)
    return fail(PCGRL_EINVAL, "pcgrl_smb_env_step: a solver budget is set and this call cannot say \"busy\": use "
                              "pcgrl_smb_ready_step, or pcgrl_smb_ready_set_budget(h, 0)");
  ON_DEVICE(h->device);
  SmbEnvArgs a = h->a;
  a.actions = d_actions;
  a.auto_reset = auto_reset ? 1 : 0;
  a.obs = d_obs;
  a.reward = d_reward;
  a.reward64 = d_reward64;
  a.done = d_done;
  a.stats_out = d_stats;
  HIPCHK(launch_smb_env(SMB_ENV_STEP, a, (hipStream_t)stream));
  return PCGRL_OK;
}

int pcgrl_smb_env_observe(pcgrl_smb_env_handle h, uint8_t *d_obs, void *stream) {
  if (!h || !d_obs) return fail(PCGRL_EINVAL, "pcgrl_smb_env_observe: bad arguments");
  if ((uintptr_t)d_obs & 15u) return fail(PCGRL_EINVAL, "pcgrl_smb_env_observe: the observation must be 16-byte aligned");
  ON_DEVICE(h->device);
  SmbEnvArgs a = h->a;
  a.obs = d_obs;
  HIPCHK(launch_smb_env(SMB_ENV_OBSERVE, a, (hipStream_t)stream));
  return PCGRL_OK;
}

static SmbEnvGather smb_env_gather_of(pcgrl_smb_env_handle h) {
  SmbEnvGather g = {};
  g.n = h->a.n;
  g.h = h->a.h;
  g.w = h->a.w;
  g.map_stride = h->a.map_stride;
  g.maps = h->a.maps;
  g.st = h->a.st;
  return g;
}

int pcgrl_smb_env_get_state(pcgrl_smb_env_handle h, uint8_t *d_grids, int32_t *d_pos, int32_t *d_counters, int32_t *d_stats,
                            double *d_last_loss, double *d_ep_return, int64_t *d_iterations, void *stream) {
  if (!h) return fail(PCGRL_EINVAL, "pcgrl_smb_env_get_state: null handle");
  ON_DEVICE(h->device);
  SmbEnvGather g = smb_env_gather_of(h);
  g.grids = d_grids;
  g.pos = d_pos;
  g.counters = d_counters;
  g.stats = d_stats;
  g.last_loss = d_last_loss;
  g.ep_return = d_ep_return;
  g.iters = d_iterations;
  HIPCHK(launch_smb_env_gather(g, (hipStream_t)stream));
  return PCGRL_OK;
}

int pcgrl_smb_env_get_last_episode(pcgrl_smb_env_handle h, double *d_return, int32_t *d_length, int32_t *d_stats,
                                   int32_t *d_count, void *stream) {
  if (!h) return fail(PCGRL_EINVAL, "pcgrl_smb_env_get_last_episode: null handle");
  ON_DEVICE(h->device);
  SmbEnvGather g = smb_env_gather_of(h);
  g.last_return = d_return;
  g.last_len = d_length;
  g.last_stats = d_stats;
  g.last_count = d_count;
  HIPCHK(launch_smb_env_gather(g, (hipStream_t)stream));
  return PCGRL_OK;
}

int pcgrl_smb_env_poll_error(pcgrl_smb_env_handle h) {
  if (!h) return fail(PCGRL_EINVAL, "pcgrl_smb_env_poll_error: null handle");
  ON_DEVICE(h->device);
  HIPCHK(hipDeviceSynchronize());
  int32_t flags = 0;
  HIPCHK(hipMemcpy(&flags, h->a.err, sizeof(flags), hipMemcpyDeviceToHost));
  if (flags) {
    HIPCHK(hipMemset(h->a.err, 0, sizeof(flags)));
    if (flags & 1) return fail(PCGRL_EACTION, "an action was outside the action space (the reference raises IndexError)");
    if (flags & 2) return fail(PCGRL_EINVAL, "smb: a tile id above 6 was seen in init_grids or in the maps of pcgrl_smb_state_set (read as empty)");
    if (flags & 4)
      return fail(PCGRL_EINVAL, "smb: pcgrl_smb_state_import saw an index entry outside 0..n_envs-1 (the env was left as it was)");
  }
  return PCGRL_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------- Super Mario Bros environments under a solver budget
// include/pcgrl_amd_smb_ready.h; kernels in smb/pcgrl_smb_ready.h.

extern "C" {

int64_t pcgrl_smb_ready_park_bytes(const pcgrl_smb_env_config *cfg) {
  if (smb_env_check("pcgrl_smb_ready_park_bytes", cfg) != PCGRL_OK) return -1;
  return (int64_t)sizeof(SmbPark);
}

int32_t pcgrl_smb_ready_get_budget(pcgrl_smb_env_handle h) { return h ? h->budget : -1; }

int pcgrl_smb_ready_set_budget(pcgrl_smb_env_handle h, int32_t budget) {
  const char *who = "pcgrl_smb_ready_set_budget";
  if (!h) return fail(PCGRL_EINVAL, std::string(who) + ": null handle");
  if (budget < 0) return fail(PCGRL_EINVAL, std::string(who) + ": the budget must be at least 0");
  if (budget == h->budget) return PCGRL_OK;
  ON_DEVICE(h->device);
  const size_t n = (size_t)h->a.n;
  if (budget == 0) {  // only when nothing is parked: the synchronous kernels know no park record
    HIPCHK(hipDeviceSynchronize());
    std::vector<int32_t> mode(n);
    HIPCHK(hipMemcpy2D(mode.data(), sizeof(int32_t), h->park, sizeof(SmbPark), sizeof(int32_t), n, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++)
      if (mode[i] != SMB_READY_IDLE)
        return fail(PCGRL_EINVAL, std::string(who) + ": env " + std::to_string(i) + " is busy: step until no env is, or reset");
  } else if (!h->park) {
    void *p = nullptr;
    HIPCHK(hipMalloc(&p, n * sizeof(SmbPark)));
    h->allocs.push_back(p);
    HIPCHK(hipMemset(p, 0, n * sizeof(SmbPark)));  // every env idle
    HIPCHK(hipDeviceSynchronize());
    h->park = (SmbPark *)p;
  }
  h->budget = budget;
  return PCGRL_OK;
}

int pcgrl_smb_ready_step(pcgrl_smb_env_handle h, const int32_t *d_actions, int32_t auto_reset, uint8_t *d_obs, float *d_reward,
                         double *d_reward64, uint8_t *d_done, int32_t *d_stats, uint8_t *d_status, void *stream) {
  if (!h || !d_actions || !d_status) return fail(PCGRL_EINVAL, "pcgrl_smb_ready_step: null handle, actions or status");
  if ((uintptr_t)d_obs & 15u) return fail(PCGRL_EINVAL, "pcgrl_smb_ready_step: the observation must be 16-byte aligned");
  if (h->budget < 1) return fail(PCGRL_EINVAL, "pcgrl_smb_ready_step: no solver budget is set (pcgrl_smb_ready_set_budget)");
  ON_DEVICE(h->device);
  SmbReadyArgs ra = {h->a, h->park, h->budget, d_status};
  ra.e.actions = d_actions;
  ra.e.auto_reset = auto_reset ? 1 : 0;
  ra.e.obs = d_obs;
  ra.e.reward = d_reward;
  ra.e.reward64 = d_reward64;
  ra.e.done = d_done;
  ra.e.stats_out = d_stats;
  HIPCHK(launch_smb_ready_step(ra, (hipStream_t)stream));
  return PCGRL_OK;
}

int pcgrl_smb_ready_busy(pcgrl_smb_env_handle h, uint8_t *d_busy, void *stream) {
  if (!h || !d_busy) return fail(PCGRL_EINVAL, "pcgrl_smb_ready_busy: bad arguments");
  ON_DEVICE(h->device);
  if (!h->park) {  // no budget was ever set: nothing can be busy
    HIPCHK(hipMemsetAsync(d_busy, 0, (size_t)h->a.n, (hipStream_t)stream));
    return PCGRL_OK;
  }
  HIPCHK(launch_smb_ready_busy(h->park, h->a.n, d_busy, (hipStream_t)stream));
  return PCGRL_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------- Super Mario Bros environments: open-loop rollouts
// include/pcgrl_amd_smb_rollout.h; kernels in smb/pcgrl_smb_rollout.h.

extern "C" {

int32_t pcgrl_smb_env_num_actions(pcgrl_smb_env_handle h) {
  return h ? (h->a.rep == PCGRL_REP_NARROW ? SMB_TILES : 4 + SMB_TILES) : -1;
}

int pcgrl_smb_env_rollout(pcgrl_smb_env_handle h, const int32_t *d_actions, uint64_t seed, int32_t n_steps, int32_t auto_reset,
                          uint8_t *d_obs, int32_t obs_mode, float *d_reward, double *d_reward64, uint8_t *d_done,
                          int32_t *d_stats, int32_t *d_actions_out, int32_t *d_ep_count, double *d_ep_return_sum,
                          int64_t *d_ep_length_sum, int64_t *d_ep_stats_sum, void *stream) {
  const char *who = "pcgrl_smb_env_rollout";
  if (!h) return fail(PCGRL_EINVAL, std::string(who) + ": null handle");
  if (n_steps < 1) return fail(PCGRL_EINVAL, std::string(who) + ": n_steps must be at least 1");
  if ((int64_t)n_steps * h->a.n > INT32_MAX)
    return fail(PCGRL_EINVAL, std::string(who) + ": n_steps * n_envs must stay below 2^31");
  if (obs_mode < 0 || obs_mode > 2) return fail(PCGRL_EINVAL, std::string(who) + ": obs_mode must be 0 (none), 1 (last) or 2 (all)");
  if (obs_mode != 0 && (!d_obs || ((uintptr_t)d_obs & 15u)))
    return fail(PCGRL_EINVAL, std::string(who) + ": the observation must be non-null and 16-byte aligned when obs_mode is not 0");
  if (h->budget > 0)
    return fail(PCGRL_EINVAL, std::string(who) + ": a solver budget is set and this call cannot say \"busy\": use "
                                                 "pcgrl_smb_ready_step, or pcgrl_smb_ready_set_budget(h, 0)");
  ON_DEVICE(h->device);
  SmbRolloutArgs ra = {};
  ra.e = h->a;
  ra.e.actions = d_actions;
  ra.e.auto_reset = auto_reset ? 1 : 0;
  ra.e.obs = obs_mode != 0 ? d_obs : nullptr;
  ra.e.reward = d_reward;
  ra.e.reward64 = d_reward64;
  ra.e.done = d_done;
  ra.e.stats_out = d_stats;
  ra.n_steps = n_steps;
  ra.obs_mode = obs_mode;
  ra.n_actions = pcgrl_smb_env_num_actions(h);
  ra.seed = seed;
  ra.draw = h->draw;
  ra.actions_out = d_actions_out;
  ra.ep_count = d_ep_count;
  ra.ep_return_sum = d_ep_return_sum;
  ra.ep_length_sum = d_ep_length_sum;
  ra.ep_stats_sum = d_ep_stats_sum;
  HIPCHK(launch_smb_env_rollout(ra, (hipStream_t)stream));
  return PCGRL_OK;
}

int pcgrl_smb_env_sample_actions(pcgrl_smb_env_handle h, int32_t *d_actions, uint64_t seed, void *stream) {
  if (!h || !d_actions) return fail(PCGRL_EINVAL, "pcgrl_smb_env_sample_actions: null handle or actions");
  ON_DEVICE(h->device);
  HIPCHK(launch_smb_env_sample(d_actions, h->a.n, pcgrl_smb_env_num_actions(h), seed, h->draw, (hipStream_t)stream));
  return PCGRL_OK;
}

}  // extern "C"

// ----------------------------------------------------------------- Super Mario Bros environments: checkpoint and restore
// include/pcgrl_amd_smb_state.h; kernels in smb/pcgrl_smb_state.h.

struct SmbStateHeader {
  uint64_t magic;        // "PCGRLSM1"
  uint64_t fingerprint;  // FNV-1a over the create-time config fields, the library version string and the fields below
  int32_t n_envs, map_stride, record_bytes, rng_bytes, mode_bytes, pad;
  uint64_t total_bytes;
};
static constexpr uint64_t SMB_STATE_MAGIC = 0x314d534c52474350ull;  // "PCGRLSM1", little endian
static_assert(sizeof(SmbStateHeader) <= SMB_STATE_HDR_BYTES, "state header section");

static SmbStateHeader smb_state_header_of(const pcgrl_smb_env *e) {
  SmbStateHeader hdr{};
  hdr.magic = SMB_STATE_MAGIC;
  hdr.n_envs = e->a.n;
  hdr.map_stride = e->a.map_stride;
  hdr.record_bytes = (int32_t)sizeof(SmbEnvState);
  hdr.rng_bytes = SMB_STATE_RNG_WORDS * 8;
  hdr.mode_bytes = 8;
  hdr.total_bytes = (uint64_t)smb_state_layout(e->a.n, e->a.map_stride, e->ctrl.n_ctrl > 0).total;
  uint64_t x = 1469598103934665603ull;
  auto mix = [&](const void *p, size_t n) {
    for (size_t i = 0; i < n; i++) x = (x ^ ((const uint8_t *)p)[i]) * 1099511628211ull;
  };
  const pcgrl_smb_env_config &c = e->cfg;  // field by field: the struct's padding bytes are not part of the config
#define MIX(f) mix(&c.f, sizeof(c.f))
  MIX(h); MIX(w); MIX(representation); MIX(obs_window); MIX(max_iterations); MIX(max_changes); MIX(solver_power); MIX(n_envs);
  MIX(has_trg); MIX(weight); MIX(trg_lo); MIX(trg_hi);
#undef MIX
  const char *v = pcgrl_version();
  mix(v, strlen(v));
  mix(&hdr.n_envs, sizeof(int32_t) * 6);
  mix(&hdr.total_bytes, sizeof(hdr.total_bytes));
  if (e->ctrl.n_ctrl > 0) {  // a controllable env: the control list and ranges (without controls the fingerprint is what it was)
    const int32_t rec_bytes = (int32_t)sizeof(SmbCtrlRec);
    mix("ctrl", 4);
    mix(&rec_bytes, sizeof(rec_bytes));
    mix(&e->ctrl.n_ctrl, sizeof(int32_t));
    mix(e->ctrl.idx, sizeof(int32_t) * e->ctrl.n_ctrl);
    mix(e->ctrl.range, sizeof(double) * e->ctrl.n_ctrl);
  }
  hdr.fingerprint = x;
  return hdr;
}

// The header never changes after the create.  It lives in pinned, mapped host memory owned by the env: the export kernel reads
// it from there, so a captured export keeps a pointer that stays valid.
static hipError_t smb_state_header_create(pcgrl_smb_env *e) {
  hipError_t he = hipHostMalloc((void **)&e->state_hdr, SMB_STATE_HDR_BYTES, hipHostMallocMapped);
  if (he != hipSuccess) {
    e->state_hdr = nullptr;
    return he;
  }
  memset(e->state_hdr, 0, SMB_STATE_HDR_BYTES);
  const SmbStateHeader hdr = smb_state_header_of(e);
  memcpy(e->state_hdr, &hdr, sizeof(hdr));
  return hipHostGetDevicePointer((void **)&e->state_hdr_dev, e->state_hdr, 0);
}

static SmbStateArgs smb_state_args_of(pcgrl_smb_env_handle h) {
  SmbStateArgs sa = {};
  sa.r.e = h->a;
  sa.r.park = h->park;
  sa.r.budget = h->budget;
  return sa;
}

extern "C" {

int64_t pcgrl_smb_state_bytes(pcgrl_smb_env_handle h) {
  if (!h) {
    (void)fail(PCGRL_EINVAL, "pcgrl_smb_state_bytes: null handle");
    return -1;
  }
  return smb_state_layout(h->a.n, h->a.map_stride, h->ctrl.n_ctrl > 0).total;
}

int pcgrl_smb_state_export(pcgrl_smb_env_handle h, uint8_t *d_buf, void *stream) {
  if (!h) return fail(PCGRL_EINVAL, "pcgrl_smb_state_export: null handle");
  if (!d_buf || ((uintptr_t)d_buf & 15u)) return fail(PCGRL_EINVAL, "pcgrl_smb_state_export: the image is null or not 16-byte aligned");
  ON_DEVICE(h->device);
  SmbStateArgs sa = smb_state_args_of(h);
  sa.hdr = h->state_hdr_dev;
  sa.image = d_buf;
  HIPCHK(launch_smb_state(SMB_STATE_EXPORT, sa, (hipStream_t)stream));
  return PCGRL_OK;
}

int pcgrl_smb_state_import(pcgrl_smb_env_handle h, const uint8_t *d_mask, const int32_t *d_index, const uint8_t *d_buf,
                           void *stream) {
  const char *who = "pcgrl_smb_state_import";
  if (!h) return fail(PCGRL_EINVAL, std::string(who) + ": null handle");
  if (!d_buf || ((uintptr_t)d_buf & 15u)) return fail(PCGRL_EINVAL, std::string(who) + ": the image is null or not 16-byte aligned");
  ON_DEVICE(h->device);
  const int32_t n = h->a.n;
  const SmbStateLayout l = smb_state_layout(n, h->a.map_stride, h->ctrl.n_ctrl > 0);
  // the header is checked on the host before anything is overwritten: a small copy and one wait for `stream`.  Where the env
  // has no budget the mask and the index come with it, and the modes once the header has said that the image has them.
  const bool sync_env = h->budget == 0;
  SmbStateHeader got{};
  std::vector<int32_t> mode(sync_env ? (size_t)n * 2 : 0), index(sync_env && d_index ? n : 0);
  std::vector<uint8_t> mask(sync_env && d_mask ? n : 0);
  HIPCHK(hipMemcpyAsync(&got, d_buf, sizeof(got), hipMemcpyDeviceToHost, (hipStream_t)stream));
  if (sync_env) {
    if (d_mask) HIPCHK(hipMemcpyAsync(mask.data(), d_mask, (size_t)n, hipMemcpyDeviceToHost, (hipStream_t)stream));
    if (d_index) HIPCHK(hipMemcpyAsync(index.data(), d_index, (size_t)n * 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
  }
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  const SmbStateHeader want = smb_state_header_of(h);
  if (got.magic != SMB_STATE_MAGIC) return fail(PCGRL_EINVAL, std::string(who) + ": not a pcgrl_smb_state_export image (bad magic)");
  if (memcmp(&got, &want, sizeof(want)) != 0)
    return fail(PCGRL_EINVAL, std::string(who) + ": the image was exported by an env with another config, batch size, layout, "
                                                 "control list or library version");
  h->touched = true;
  if (sync_env) {
    HIPCHK(hipMemcpyAsync(mode.data(), d_buf + l.mode, (size_t)n * 8, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));  // (nothing else is queued: the wait above has drained the stream)
    int busy = 0;
    for (int32_t i = 0; i < n; i++) {
      if (d_mask && mask[i] == 0) continue;
      const int32_t row = d_index ? index[i] : i;
      if (row < 0 || row >= n) continue;  // overwrites nothing (the error bit)
      busy += mode[(size_t)row * 2] != SMB_READY_IDLE ? 1 : 0;
    }
    if (busy)
      return fail(PCGRL_EUNSUPPORTED, std::string(who) + ": " + std::to_string(busy) + " of the rows to import are busy (a parked "
                  "search of an env with a solver budget), which only pcgrl_smb_ready_step can finish: set a solver budget "
                  "first, or mask them out");
  }
  SmbStateArgs sa = smb_state_args_of(h);
  sa.r.e.mask = d_mask;
  sa.index = d_index;
  sa.image = (uint8_t *)d_buf;
  HIPCHK(launch_smb_state(SMB_STATE_IMPORT, sa, (hipStream_t)stream));
  return PCGRL_OK;
}

int pcgrl_smb_state_set(pcgrl_smb_env_handle h, const uint8_t *d_mask, const uint8_t *d_grids, const int32_t *d_pos,
                        const int32_t *d_counters, const double *d_ep_return, void *stream) {
  if (!h) return fail(PCGRL_EINVAL, "pcgrl_smb_state_set: null handle");
  if (!d_grids) return fail(PCGRL_EINVAL, "pcgrl_smb_state_set: null maps");
  ON_DEVICE(h->device);
  h->touched = true;
  SmbStateArgs sa = smb_state_args_of(h);
  sa.r.e.mask = d_mask;
  sa.r.e.init_grids = d_grids;
  sa.pos = d_pos;
  sa.counters = d_counters;
  sa.ep_return = d_ep_return;
  HIPCHK(launch_smb_state(SMB_STATE_SET, sa, (hipStream_t)stream));
  return PCGRL_OK;
}

int pcgrl_smb_state_get_rng(pcgrl_smb_env_handle h, uint64_t *d_rng, void *stream) {
  if (!h) return fail(PCGRL_EINVAL, "pcgrl_smb_state_get_rng: null handle");
  if (!d_rng) return fail(PCGRL_EINVAL, "pcgrl_smb_state_get_rng: null output");
  ON_DEVICE(h->device);
  SmbStateArgs sa = smb_state_args_of(h);
  sa.rng_out = d_rng;
  HIPCHK(launch_smb_state(SMB_STATE_RNG, sa, (hipStream_t)stream));
  return PCGRL_OK;
}

int pcgrl_smb_state_set_rng(pcgrl_smb_env_handle h, const uint8_t *d_mask, const uint64_t *d_rng, void *stream) {
  if (!h) return fail(PCGRL_EINVAL, "pcgrl_smb_state_set_rng: null handle");
  if (!d_rng) return fail(PCGRL_EINVAL, "pcgrl_smb_state_set_rng: null input");
  ON_DEVICE(h->device);
  SmbStateArgs sa = smb_state_args_of(h);
  sa.r.e.mask = d_mask;
  sa.rng_in = d_rng;
  HIPCHK(launch_smb_state(SMB_STATE_RNG, sa, (hipStream_t)stream));
  return PCGRL_OK;
}

}  // extern "C"

// ------------------------------------------------------------ Super Mario Bros environments: controllable generation
// include/pcgrl_amd_smb_ctrl.h; kernels in smb/pcgrl_smb_ctrl.h and, as the controllable instantiations, in every smb kernel file.

extern "C" {

int32_t pcgrl_smb_ctrl_count(pcgrl_smb_env_handle h) { return h ? h->ctrl.n_ctrl : -1; }

int pcgrl_smb_ctrl_attach(pcgrl_smb_env_handle h, int32_t n_ctrl, const int32_t *ctrl_idx, const double *ctrl_range,
                          const double *shown, float *d_ctrl_obs) {
  const char *who = "pcgrl_smb_ctrl_attach";
  if (!h) return fail(PCGRL_EINVAL, std::string(who) + ": null handle");
  if (h->ctrl.n_ctrl > 0) return fail(PCGRL_EINVAL, std::string(who) + ": the env has controls already");
  if (h->touched) return fail(PCGRL_EINVAL, std::string(who) + ": controls are attached before the first reset");
  if (n_ctrl < 1 || n_ctrl > SMB_STATS || !ctrl_idx || !ctrl_range || !shown)
    return fail(PCGRL_EINVAL, std::string(who) + ": n_ctrl must be in 1..9 and the index, range and value arrays non-null");
  if ((uintptr_t)d_ctrl_obs & 7u) return fail(PCGRL_EINVAL, std::string(who) + ": the control observation must be 8-byte aligned");
  uint32_t seen = 0;
  for (int j = 0; j < n_ctrl; j++) {
    if (ctrl_idx[j] < 0 || ctrl_idx[j] >= SMB_STATS)
      return fail(PCGRL_EINVAL, std::string(who) + ": a control index is outside the nine statistics");
    if ((seen >> ctrl_idx[j]) & 1u) return fail(PCGRL_EINVAL, std::string(who) + ": a statistic is listed twice");
    seen |= 1u << ctrl_idx[j];
    if (!(ctrl_range[j] > 0.0) || !std::isfinite(ctrl_range[j]) || !std::isfinite(shown[j]))
      return fail(PCGRL_EINVAL, std::string(who) + ": ranges must be positive and finite, observed values finite");
  }
  ON_DEVICE(h->device);
  SmbCtrlCfg cc = {};
  cc.n_ctrl = n_ctrl;
  SmbCtrlRec rec = {};
  for (int k = 0; k < SMB_STATS; k++) {
    rec.lo[k] = h->a.trg_lo[k];
    rec.hi[k] = h->a.trg_hi[k];
  }
  for (int j = 0; j < n_ctrl; j++) {
    cc.idx[j] = ctrl_idx[j];
    cc.range[j] = ctrl_range[j];
    rec.obs[j] = shown[j];
  }
  const std::vector<SmbCtrlRec> recs((size_t)h->a.n, rec);
  void *d_cfg = nullptr, *d_rec = nullptr;
  hipError_t he = hipMalloc(&d_cfg, sizeof(SmbCtrlCfg));
  if (he == hipSuccess) {
    h->allocs.push_back(d_cfg);
    he = hipMalloc(&d_rec, recs.size() * sizeof(SmbCtrlRec));
  }
  if (he == hipSuccess) {
    h->allocs.push_back(d_rec);
    he = hipMemcpy(d_cfg, &cc, sizeof(cc), hipMemcpyHostToDevice);
  }
  if (he == hipSuccess) he = hipMemcpy(d_rec, recs.data(), recs.size() * sizeof(SmbCtrlRec), hipMemcpyHostToDevice);
  if (he == hipSuccess) he = hipDeviceSynchronize();
  if (he != hipSuccess) return fail(PCGRL_EHIP, std::string(who) + ": " + hipGetErrorString(he));
  h->ctrl = cc;
  h->a.ctrl.cfg = (const SmbCtrlCfg *)d_cfg;
  h->a.ctrl.rec = (SmbCtrlRec *)d_rec;
  h->a.ctrl.obs = d_ctrl_obs;
  const SmbStateHeader hdr = smb_state_header_of(h);  // the image gains the control section: a new size and fingerprint
  memcpy(h->state_hdr, &hdr, sizeof(hdr));
  return PCGRL_OK;
}

int pcgrl_smb_ctrl_queue(pcgrl_smb_env_handle h, const uint8_t *d_mask, int32_t n_named, const int32_t *named,
                         const double *d_lo, const double *d_hi, const double *d_shown, void *stream) {
  const char *who = "pcgrl_smb_ctrl_queue";
  if (!h) return fail(PCGRL_EINVAL, std::string(who) + ": null handle");
  if (h->ctrl.n_ctrl < 1) return fail(PCGRL_EINVAL, std::string(who) + ": the env has no controls (pcgrl_smb_ctrl_attach)");
  if (n_named < 1 || n_named > h->ctrl.n_ctrl || !named || !d_lo || !d_hi || !d_shown)
    return fail(PCGRL_EINVAL, std::string(who) + ": between 1 and n_ctrl named controls, and non-null lo, hi and observed values");
  SmbCtrlQueueArgs qa = {};
  uint32_t seen = 0;
  for (int i = 0; i < n_named; i++) {
    if (named[i] < 0 || named[i] >= h->ctrl.n_ctrl)
      return fail(PCGRL_EINVAL, std::string(who) + ": a named control is outside 0..n_ctrl-1");
    if ((seen >> named[i]) & 1u) return fail(PCGRL_EINVAL, std::string(who) + ": a control is named twice");
    seen |= 1u << named[i];
    qa.named[i] = named[i];
  }
  ON_DEVICE(h->device);
  qa.n = h->a.n;
  qa.n_named = n_named;
  qa.rec = h->a.ctrl.rec;
  qa.mask = d_mask;
  qa.lo = d_lo;
  qa.hi = d_hi;
  qa.obs = d_shown;
  HIPCHK(launch_smb_ctrl_queue(qa, (hipStream_t)stream));
  return PCGRL_OK;
}

int pcgrl_smb_ctrl_observe(pcgrl_smb_env_handle h, float *d_ctrl_obs, void *stream) {
  const char *who = "pcgrl_smb_ctrl_observe";
  if (!h) return fail(PCGRL_EINVAL, std::string(who) + ": null handle");
  if (h->ctrl.n_ctrl < 1) return fail(PCGRL_EINVAL, std::string(who) + ": the env has no controls (pcgrl_smb_ctrl_attach)");
  float *out = d_ctrl_obs ? d_ctrl_obs : h->a.ctrl.obs;
  if (!out) return fail(PCGRL_EINVAL, std::string(who) + ": no output and no attached control observation");
  ON_DEVICE(h->device);
  SmbCtrlObserveArgs oa = {};
  oa.n = h->a.n;
  oa.c = h->a.ctrl;
  oa.c.obs = out;
  oa.stats = (const int32_t *)h->a.st;
  oa.stats_stride = (int64_t)sizeof(SmbEnvState);
  oa.stats_offset = (int64_t)offsetof(SmbEnvState, stats);
  HIPCHK(launch_smb_ctrl_observe(oa, (hipStream_t)stream));
  return PCGRL_OK;
}

int pcgrl_smb_ctrl_set_resampling(pcgrl_smb_env_handle h, int32_t enable, uint64_t seed, const double *lo, const double *hi,
                                  void *stream) {
  const char *who = "pcgrl_smb_ctrl_set_resampling";
  if (!h) return fail(PCGRL_EINVAL, std::string(who) + ": null handle");
  if (h->ctrl.n_ctrl < 1) return fail(PCGRL_EINVAL, std::string(who) + ": the env has no controls (pcgrl_smb_ctrl_attach)");
  if (enable && (!lo || !hi)) return fail(PCGRL_EINVAL, std::string(who) + ": resampling needs lo and hi per control");
  SmbCtrlResampleArgs ra = {};
  for (int j = 0; j < h->ctrl.n_ctrl; j++) {
    ra.lo[j] = lo ? lo[j] : 0.0;
    ra.hi[j] = hi ? hi[j] : 0.0;
    if (!std::isfinite(ra.lo[j]) || !std::isfinite(ra.hi[j]))
      return fail(PCGRL_EINVAL, std::string(who) + ": the bounds must be finite");
  }
  ON_DEVICE(h->device);
  ra.cfg = (SmbCtrlCfg *)h->a.ctrl.cfg;
  ra.enable = enable ? 1 : 0;
  ra.n_ctrl = h->ctrl.n_ctrl;
  ra.seed = seed;
  HIPCHK(launch_smb_ctrl_resample(ra, (hipStream_t)stream));
  return PCGRL_OK;
}

int pcgrl_smb_ctrl_get(pcgrl_smb_env_handle h, double *d_active, double *d_shown, double *d_queued, int32_t *d_flags,
                       void *stream) {
  const char *who = "pcgrl_smb_ctrl_get";
  if (!h) return fail(PCGRL_EINVAL, std::string(who) + ": null handle");
  if (h->ctrl.n_ctrl < 1) return fail(PCGRL_EINVAL, std::string(who) + ": the env has no controls (pcgrl_smb_ctrl_attach)");
  ON_DEVICE(h->device);
  SmbCtrlGetArgs ga = {};
  ga.n = h->a.n;
  ga.rec = h->a.ctrl.rec;
  ga.active = d_active;
  ga.shown = d_shown;
  ga.queued = d_queued;
  ga.flags = d_flags;
  HIPCHK(launch_smb_ctrl_get(ga, (hipStream_t)stream));
  return PCGRL_OK;
}

}  // extern "C"

// ------------------------------------------------------------------- Super Mario Bros environments: the float32 hand-out
// include/pcgrl_amd_smb_vector.h; the kernel in smb/pcgrl_smb_vector.h.

extern "C" {

int64_t pcgrl_smb_env_obs_f32_bytes(pcgrl_smb_env_handle h) {
  if (!h) return -1;
  return (int64_t)h->a.oh * h->a.ow * (2 * h->ctrl.n_ctrl + SMB_TILES + 1) * (int64_t)sizeof(float);
}

int pcgrl_smb_env_observe_f32(pcgrl_smb_env_handle h, float *out, void *stream) {
  const char *who = "pcgrl_smb_env_observe_f32";
  if (!h || !out) return fail(PCGRL_EINVAL, std::string(who) + ": null handle or output");
  if ((uintptr_t)out & 7u) return fail(PCGRL_EINVAL, std::string(who) + ": the output must be 8-byte aligned");
  if (h->budget > 0)
    return fail(PCGRL_EUNSUPPORTED, std::string(who) + ": a solver budget is set: a busy env's committed state is not the state "
                                                       "of the step in flight (pcgrl_smb_ready_set_budget(h, 0) first)");
  if (h->ctrl.n_ctrl > 0 && !h->a.ctrl.obs)
    return fail(PCGRL_EINVAL, std::string(who) + ": the controls were attached without a control observation buffer");
  ON_DEVICE(h->device);
  SmbVectorArgs va = {};
  va.h = h->a.h;
  va.w = h->a.w;
  va.oh = h->a.oh;
  va.ow = h->a.ow;
  va.n = h->a.n;
  va.map_stride = h->a.map_stride;
  va.n_ctrl = h->ctrl.n_ctrl;
  va.maps = h->a.maps;
  va.st = h->a.st;
  va.ctrl_obs = h->a.ctrl.obs;
  va.out = out;
  HIPCHK(launch_smb_vector_obs(va, (hipStream_t)stream));
  return PCGRL_OK;
}

}  // extern "C"

// ------------------------------------------------------- Super Mario Bros maps: level measures and pairwise Hamming diversity
// include/pcgrl_amd_smb_measures.h; the measure / pack kernel in smb/pcgrl_smb_measures.h, the pairwise kernels those of
// measures/pcgrl_measures.h; the host path is the one of "measures and diversity" above.

static int smb_meas_check_shape(const char *who, int32_t h, int32_t w) {
  if (!smb_shape_ok(h, w))
    return fail(PCGRL_EUNSUPPORTED, std::string(who) + ": maps of 4..16 rows and 1..128 columns only (the shapes the smb "
                                                       "evaluator takes)");
  return PCGRL_OK;
}

// an env handle's committed maps: rows of map_stride bytes on a 16-byte aligned base (pcgrl_smb_env_create)
static MeasWaveArgs smb_env_meas_args(const pcgrl_smb_env *e) {
  return meas_args(e->a.maps, e->a.map_stride, e->a.h, e->a.w, e->a.n);
}

extern "C" {

int pcgrl_smb_measures_for_grids(int32_t h, int32_t w, int32_t n, const uint8_t *d_grids, int32_t *d_counts, int32_t *d_match,
                                 double *d_forms, double *d_entropy, const double *d_entropy_tab, void *stream) {
  return measures_for_grids("pcgrl_smb_measures_for_grids", smb_meas_check_shape, launch_smb_measures, h, w, n, d_grids,
                            d_counts, d_match, d_forms, d_entropy, d_entropy_tab, stream);
}

size_t pcgrl_smb_diversity_scratch_bytes(int32_t h, int32_t w, int32_t n) {
  if (n <= 0 || !smb_shape_ok(h, w)) return 0;
  return diversity_scratch_bytes(SMB_MEAS_PLANES, h, w, n);
}

int pcgrl_smb_diversity_for_grids(int32_t h, int32_t w, int32_t n, const uint8_t *d_grids, int32_t group, void *d_scratch,
                                  int64_t *d_sum, double *d_scores, int32_t *d_nearest, int32_t *d_nearest_idx,
                                  int32_t *d_pairwise, void *stream) {
  return diversity_for_grids("pcgrl_smb_diversity_for_grids", smb_meas_check_shape, SMB_MEAS_PLANES, launch_smb_measures, h, w,
                             n, d_grids, group, d_scratch, d_sum, d_scores, d_nearest, d_nearest_idx, d_pairwise, stream);
}

int pcgrl_smb_env_measures(pcgrl_smb_env_handle h, int32_t *d_counts, int32_t *d_match, double *d_forms, double *d_entropy,
                           const double *d_entropy_tab, void *stream) {
  const char *who = "pcgrl_smb_env_measures";
  if (!h) return fail(PCGRL_EINVAL, std::string(who) + ": null handle");
  int rc = measures_check(who, false, h->a.n, nullptr, d_counts, d_match, d_entropy, d_entropy_tab);
  if (rc == PCGRL_OK) rc = smb_meas_check_shape(who, h->a.h, h->a.w);
  if (rc != PCGRL_OK) return rc;
  ON_DEVICE(h->device);
  return measures_enqueue(smb_env_meas_args(h), launch_smb_measures, d_counts, d_match, d_forms, d_entropy, d_entropy_tab,
                          stream);
}

int pcgrl_smb_env_diversity(pcgrl_smb_env_handle h, int32_t group, void *d_scratch, int64_t *d_sum, double *d_scores,
                            int32_t *d_nearest, int32_t *d_nearest_idx, int32_t *d_pairwise, void *stream) {
  const char *who = "pcgrl_smb_env_diversity";
  if (!h) return fail(PCGRL_EINVAL, std::string(who) + ": null handle");
  int rc = diversity_check(who, false, h->a.n, nullptr, group, d_scratch, d_sum);
  if (rc == PCGRL_OK) rc = smb_meas_check_shape(who, h->a.h, h->a.w);
  if (rc != PCGRL_OK) return rc;
  ON_DEVICE(h->device);
  return diversity_enqueue(smb_env_meas_args(h), SMB_MEAS_PLANES, launch_smb_measures, group, d_scratch, d_sum, d_scores,
                           d_nearest, d_nearest_idx, d_pairwise, stream);
}

}  // extern "C"
