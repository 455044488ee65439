// smb/pcgrl_smb_rollout.h -- open-loop rollouts of Super Mario Bros environments (include/pcgrl_amd_smb_rollout.h): K steps of
// every env in one launch, with given actions or with actions drawn on the device.  DESIGN.md section 21 has the rules.
//
// smb_env_rollout_kernel keeps smb_env_step_kernel's layout (smb/pcgrl_smb_env.h): one 64-lane wave per env, the map in SmbLds.
//   once      the map and the SmbEnvState record are loaded; with drawn actions the handle's draw counter is read.
//   per step  the pieces smb_env_step_kernel composes (smb_env_bad_action, _update, _restat, _emit, _latch, _begin), in the same
//             order, on the record in registers and the map in LDS -- the action check, the update, the two exact shortcuts,
//             loss and float64 reward, done, the latch of the finished episode and, with auto_reset, the next episode drawn and
//             searched inside the same iteration -- with row k of reward / reward64 / done / stats as the output row.
//             A launch therefore lasts as long as the largest, over envs, of the env's OWN K steps, not as the sum over steps
//             of the batch's longest search.
//   at the end  the map (if an edit or a new episode touched it) and the record.  The two PCG64 streams stay in HBM between the
//             episode draws, as smb_env_draw keeps them: it loads them, and its lane 0 stores them advanced; the barrier in
//             front of every draw orders the next draw's loads behind those stores.
//   obs       mode 1: [n][obs_bytes] of the last step only, issued before that step's search where the step kernel issues it;
//             mode 2: [K][n][obs_bytes], row k what step() would have returned at step k (smb_env_write_obs with the row index
//             k * n + env).  At an episode end with auto_reset that is the new episode's first observation.
//   bad action  pcgrl_smb_env_step's rule for that step: error bit 0, reward 0, not done, the same statistics, the env as it
//             was; the loop goes on with step k + 1.
//   actions   e.actions int32 [K][n], or drawn: the action of env i at step k is the engine's own function of (seed, c + k, i)
//             (sample_actions_kernel of pcgrl_engine.hip), c the handle's draw counter.  Every block reads c, then takes a
//             ticket; the last ticket stores c + K, so a captured launch draws fresh actions at every replay.
//   episodes  optional caller buffers per env, zeroed by the launch and added to by lane 0 at every latch, in the order the
//             episodes finished.  They are not part of SmbEnvState: the record and the state image do not change.
#pragma once
#include "pcgrl_smb_env.h"

namespace pcgrl {

struct SmbDrawState {
  unsigned long long counter;  // draws taken so far
  unsigned int ticket;
};

struct SmbRolloutArgs {
  SmbEnvArgs e;  // actions [K][n] or null; obs as obs_mode says; reward, reward64, done [K][n]; stats_out [K][n][9]
  int32_t n_steps, obs_mode, n_actions;
  uint64_t seed;
  SmbDrawState *draw;
  int32_t *actions_out;    // [K][n] or null
  int32_t *ep_count;       // [n] or null
  double *ep_return_sum;   // [n] or null
  int64_t *ep_length_sum;  // [n] or null
  int64_t *ep_stats_sum;   // [n][9] or null
};

hipError_t launch_smb_env_rollout(const SmbRolloutArgs &a, hipStream_t s);
hipError_t launch_smb_env_sample(int32_t *out, int n, int n_actions, uint64_t seed, SmbDrawState *draw, hipStream_t s);

#ifdef PCGRL_KERNEL_TU

__device__ __forceinline__ uint64_t smb_mix64(uint64_t z) {  // splitmix64 finaliser
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// entry i of draw c under `seed`: floor(r * n_actions / 2^64)
__device__ __forceinline__ int smb_sampled_action(uint64_t seed, uint64_t c, int i, uint32_t n_actions) {
  const uint64_t r = smb_mix64(smb_mix64(seed + c * 0x9e3779b97f4a7c15ull) ^ ((uint64_t)i * 0xd1b54a32d192ed03ull + 0x8cb92ba72f3d8dd7ull));
  return (int)__umul64hi(r, (uint64_t)n_actions);
}

// Lane 0 of every block calls this once: the draw counter as the launch found it.  The ticket is taken after the read
// (release), and the block with the last ticket -- every block has read by then (acquire) -- advances the counter by `by`.
__device__ __forceinline__ unsigned long long smb_draw_counter(SmbDrawState *d, unsigned long long by) {
  const unsigned long long c = __hip_atomic_load(&d->counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (__hip_atomic_fetch_add(&d->ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1u) {
    __hip_atomic_store(&d->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&d->counter, c + by, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  return c;
}

__global__ __launch_bounds__(256) void smb_env_sample_kernel(int32_t *out, int32_t n, uint32_t n_actions, uint64_t seed,
                                                             SmbDrawState *draw) {
  __shared__ unsigned long long c_sh;
  if (threadIdx.x == 0) c_sh = smb_draw_counter(draw, 1ull);
  __syncthreads();
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = smb_sampled_action(seed, c_sh, i, n_actions);
}

template <bool CTRL>
__global__ __launch_bounds__(64) void smb_env_rollout_kernel(const SmbRolloutArgs ra) {
  __shared__ SmbLds L;
  __shared__ typename SmbCtrlLdsOf<CTRL>::type C;
  const SmbEnvArgs &a = ra.e;
  const int env = blockIdx.x, lane = threadIdx.x;
  if (env >= a.n) return;
  const int N = a.n, K = ra.n_steps;
  smb_env_load_map(L, a, env, lane);
  SmbEnvState S = a.st[env];
  smb_ctrl_load(C, a.ctrl, env, lane);
  uint64_t c0 = 0;
  if (!a.actions) {
    unsigned long long c = 0;
    if (lane == 0) c = smb_draw_counter(ra.draw, (unsigned long long)K);
    c0 = (uint64_t)__shfl(c, 0, 64);
  }
  if (lane == 0) {  // the episode totals of this launch start from nothing
    if (ra.ep_count) ra.ep_count[env] = 0;
    if (ra.ep_return_sum) ra.ep_return_sum[env] = 0.0;
    if (ra.ep_length_sum) ra.ep_length_sum[env] = 0;
    if (ra.ep_stats_sum)
      for (int j = 0; j < SMB_STATS; j++) ra.ep_stats_sum[(size_t)env * SMB_STATS + j] = 0;
  }
  bool dirty = false;  // the map in LDS differs from the stored one
  __syncthreads();
  for (int k = 0; k < K; k++) {
    const size_t row = (size_t)k * N + env;
    const int act = a.actions ? a.actions[row] : smb_sampled_action(ra.seed, c0 + (uint64_t)k, env, (uint32_t)ra.n_actions);
    if (ra.actions_out && lane == 0) ra.actions_out[row] = act;
    const bool want_obs = ra.obs_mode == 2 || (ra.obs_mode == 1 && k == K - 1);
    const int obs_row = ra.obs_mode == 2 ? (int)row : env;
    if (smb_env_bad_action(a, act, ra.n_actions, row, lane, S)) {  // the env as it was; the loop goes on
      if (want_obs) smb_env_write_obs(L, a, obs_row, lane, S.pos[0], S.pos[1]);
      continue;
    }
    SmbEnvEdit e = smb_env_update(L, a, act, lane, S);
    const bool renew = e.done && a.auto_reset != 0;
    if (want_obs && !renew) smb_env_write_obs(L, a, obs_row, lane, e.pos[0], e.pos[1]);  // drains under the search
    if (e.changed) {
      dirty = true;
      smb_env_restat(L, a, env, e.resolid, S);
    }
    smb_env_emit(a, row, lane, e, S, C);
    if (e.done) {
      smb_env_latch(S);
      if (lane == 0) {  // lane 0 wrote the zeros above: its own stores, read back in program order
        if (ra.ep_count) ra.ep_count[env] += 1;
        if (ra.ep_return_sum) ra.ep_return_sum[env] += S.ep_return;
        if (ra.ep_length_sum) ra.ep_length_sum[env] += S.ep_len;
        if (ra.ep_stats_sum)
          for (int j = 0; j < SMB_STATS; j++) ra.ep_stats_sum[(size_t)env * SMB_STATS + j] += S.stats[j];
      }
    }
    if (renew) {  // the next episode inside the same iteration: the observation of this step is its first
      dirty = true;
      __syncthreads();
      smb_env_draw(L, a, env, lane, e.pos);
      __syncthreads();
      if (want_obs) smb_env_write_obs(L, a, obs_row, lane, e.pos[0], e.pos[1]);
      smb_env_begin(L, a, env, S, e.pos, C);
    }
  }
  smb_ctrl_write_obs(C, a.ctrl, env, lane, S.stats);  // the control observation after the last step
  if (dirty) smb_env_store_map(L, a, env, lane);
  if (lane == 0) a.st[env] = S;
}

#endif  // PCGRL_KERNEL_TU

}  // namespace pcgrl
