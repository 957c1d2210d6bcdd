// mgx_step_stats.h — a chosen handful of stats of every env and agent, read out on the device at the end of every step.
//
// Reference: MettaGridPufferEnv takes step_info_keys (python/src/mettagrid/envs/mettagrid_puffer_env.py:81, 132-183) and after
// every sim.step() reads those values — game stats, attributes, per-agent stats, the step and episode rewards — into the
// step's info payload (_build_step_info_payload :230-282, returned by step :402-408).  mgx_get_stats serves one env per call,
// flushes the integer bookkeeping of the whole batch and waits for four copies: nothing to call every step at 65 536 envs.
// Here the host resolves each key ONCE into a column (kind, id) and one kernel behind the step gathers the columns of all
// envs / agents into caller-owned device tensors:
//
//   mgx_step_stats_kernel   one LANE per (row, column) pair, columns fastest: the stores of a wavefront are one contiguous run
//                           of the output, the lanes of one row share that row's lines (its stat row, its 32-byte ag_cnt
//                           record).  Agent pairs [E*A][KA] first, then game pairs [E][KG]; grid-stride over both.
//
// The kernel only READS engine state.  A stat the engine keeps as an integer (MgxDev::shadow: the counters of the per-action
// bookkeeping in ag_cnt, the two coverage stats in ag_unique / ag_maxdist) is converted exactly as mgx_shadow_flush_kernel
// (mgx_episode.h) converts it — its float cell in the stat row may be stale and is neither read nor written here, so the
// step pays no flush (DESIGN.md §4 "Bookkeeping counters as integers").  "Key exists" follows mgx_get_stats and
// mgx_episode_record_kernel: touched bit OR value != 0.
#ifndef MGX_STEP_STATS_H_
#define MGX_STEP_STATS_H_

#include "mgx_device.h"

// A column word: kind (MGX_SSK_*, include/mgx_program.h) | counter word q << 8 | stat id << 16.
#define MGX_SS_COL(kind, q, id) ((uint32_t)(kind) | ((uint32_t)(q) << 8) | ((uint32_t)(id) << 16))
#define MGX_SS_KIND(w) ((int)((w) & 0xFFu))
#define MGX_SS_Q(w) ((int)(((w) >> 8) & 0xFFu))
#define MGX_SS_ID(w) ((int)((w) >> 16))

struct MgxStepStats {
  int KG, KA;                    // game / agent columns (each at most MGX_SS_MAX_COLUMNS)
  const uint32_t* cols;          // device: [KG] game column words, then [KA] agent column words
  float* game_out;               // [E][KG]        caller-owned device memory
  uint8_t* game_exists;          // [E][KG]
  float* agent_out;              // [E*A][KA]
  uint8_t* agent_exists;         // [E*A][KA]
};

#ifndef MGX_CPU_EMU
// k -> (k / K, k % K); pair counts of real batches fit 32 bits, where the division is an order of magnitude cheaper
__device__ __forceinline__ void mgx_ss_split(long long k, int K, long long& row, int& c) {
  if (k < (1ll << 31)) {
    const uint32_t q = (uint32_t)k / (uint32_t)K;
    row = (long long)q;
    c = (int)((uint32_t)k - q * (uint32_t)K);
  } else {
    row = k / K;
    c = (int)(k - row * K);
  }
}

__global__ void __launch_bounds__(256) mgx_step_stats_kernel(const MgxDev* __restrict__ dp, const MgxStepStats s) {
  const MgxDev& d = *dp;
  const long long n_agent = (long long)d.E * d.A * s.KA, total = n_agent + (long long)d.E * s.KG;
  for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += (long long)gridDim.x * blockDim.x) {
    long long row;
    int c;
    float v = 0.f;
    bool t = false;
    if (k < n_agent) {
      mgx_ss_split(k, s.KA, row, c);
      const uint32_t w = s.cols[s.KG + c];
      const int kind = MGX_SS_KIND(w), id = MGX_SS_ID(w);
      const size_t ao = (size_t)row;
      if (kind == MGX_SSK_REWARD_STEP) { v = d.rewards[ao]; t = true; }
      else if (kind == MGX_SSK_REWARD_EPISODE) { v = d.episode_rewards[ao]; t = true; }
      else if (kind != MGX_SSK_ABSENT) {
        if (kind == MGX_SSK_STAT) v = d.ag_stats[ao * d.NSP + id];
        else if (kind == MGX_SSK_COUNTER) {
          const int q = MGX_SS_Q(w);
          const uint32_t n = d.ag_cnt[ao * 8 + q];
          v = (float)(q == 7 ? n : min(n, 1u << 24));   // (the running maximum is not a sum of 1.f: no clamp)
        }
        else if (kind == MGX_SSK_COV_UNIQUE) v = (float)d.ag_unique[ao];
        else v = (float)d.ag_maxdist[ao];
        t = ((d.ag_touched[ao * d.NSW + (id >> 5)] >> (id & 31)) & 1u) || v != 0.f;
      }
      s.agent_out[k] = v;
      s.agent_exists[k] = t ? 1 : 0;
    } else {
      const long long g = k - n_agent;
      mgx_ss_split(g, s.KG, row, c);
      const uint32_t w = s.cols[c];
      const int kind = MGX_SS_KIND(w), id = MGX_SS_ID(w);
      const size_t env = (size_t)row;
      if (kind == MGX_SSK_STEPS) { v = (float)d.step[env]; t = true; }
      else if (kind == MGX_SSK_STAT) {
        v = d.game_stats[env * d.NG + id];
        t = ((d.game_touched[env * d.NGW + (id >> 5)] >> (id & 31)) & 1u) || v != 0.f;
      }
      s.game_out[g] = v;
      s.game_exists[g] = t ? 1 : 0;
    }
  }
}
#endif  // !MGX_CPU_EMU

#endif  // MGX_STEP_STATS_H_
