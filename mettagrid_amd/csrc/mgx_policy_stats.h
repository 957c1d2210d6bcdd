// mgx_policy_stats.h — per-policy episode statistics of a batch of auto-resetting envs, reduced on the device.
//
// Reference: build_multi_episode_rollout_summaries (python/src/mettagrid/simulator/multi_episode/summary.py:38-130) splits a
// finished episode's agents by the policy that drove them (`assignments`): summed_policy_stats[p][key] += float(value) over
// the agents of p in agent order (:60-67), per_policy_totals[p] += float(reward) and per_policy_counts[p] += 1 (:81-94), the
// episode's row of per_episode_per_policy_avg_rewards being totals[p] / counts[p] or None.  The episode records of
// mgx_episode.h fold all agents into one mean, and the per-agent log rows that would allow the split on the host cost A * NS
// words per episode.  Here the split happens behind mgx_episode_record_kernel (whose launcher flushes the integer counters
// into the stat cells first), before the restart wipes the rows:
//
//   mgx_policy_record_kernel    one WAVEFRONT per finished env (ordered done list), lane = agent-stat column.  Per column and
//                               policy p an f64 sum, started at +0.0, of (double)ag_stats[a][c] over the agents a with
//                               assign[env][a] == p in agent order, and a "key exists" bit (some agent of p has the touched
//                               bit or a non-zero value: the rule of mgx_get_stats; one ballot per policy and 64 columns).
//                               An agent of another policy adds +0.0: x + +0.0 == x for every x but -0.0, and a sum that starts
//                               at +0.0 never becomes -0.0 (+0.0 + -0.0 == +0.0 under round-to-nearest), so adding
//                               unconditionally gives the reference's bits.  The P sums of a lane stay in registers (the
//                               policy loop is unrolled over a compile-time bound PP >= P and picks by compare-select, so
//                               nothing is indexed dynamically): no scratch, no LDS, no atomics.  Lane p also sums the
//                               episode rewards of policy p's agents in agent order (f64) and counts them.
//                               One fixed-size RECORD per finished env in done-list order, optionally also into a bounded LOG.
//   mgx_policy_total_kernel     records -> batch totals (f64) in the order of mgx_episode_accum_kernel: list order, chunks of
//                               MGX_EP_CHUNK, chunk sums started at +0.0 and added in chunk order by the last workgroup.
//                               One thread per (policy, column) and per policy header, spread over blockIdx.y.
//                               mgx_request_policy_stats takes the totals with mgx_totals_snapshot_kernel<MgxPsKind>.
//   mgx_policy_assign_kernel    rows of the assignment table of a list of envs <- a packed block (mgx_set_policy_assignments).
//
// The assignment table (u8 [E][A]) is SLOT-owned: agent rows are routed to policies by row index, whichever episode or env
// state occupies the slot, so mgx_save_envs / mgx_load_envs / mgx_copy_envs never touch it and an episode is attributed by the
// table as it stands when the episode ends.
#ifndef MGX_POLICY_STATS_H_
#define MGX_POLICY_STATS_H_

#include "mgx_device.h"
#include "mgx_episode.h"

#define MGX_PS_MAX_POLICIES 16   // include/mgx.h MGX_MAX_POLICIES: 16 f64 sums per lane are 32 VGPRs
#define MGX_PS_HDR 4             // record header words: env, episode, steps, flags (the f64 fields start on an 8-byte boundary)
#define MGX_PS_TOT_HDR 1         // totals header doubles: episodes
#define MGX_PS_TOT_POLICY 5      // per policy: episodes with an agent, agent-episodes, sum / min / max of the per-episode average reward

struct MgxPsLayout {
  int NS, NSW, NSP, A, P;
  int off_rew, off_cnt, off_sum, off_bits, rec_words;   // the record (32-bit words); a log record is the same
  int tot_off_sum, tot_off_cnt, tot_words;              // totals (doubles): header, P * 5 policy words, [P][NS] sums, [P][NS] key counts
};

static inline MgxPsLayout mgx_ps_layout(int NS, int A, int NSP, int P) {
  MgxPsLayout L{};
  L.NS = NS; L.NSW = (NS + 31) / 32; L.NSP = NSP; L.A = A; L.P = P;
  int w = MGX_PS_HDR;
  L.off_rew = w; w += 2 * P;
  L.off_cnt = w; w += P;
  w = (w + 1) & ~1;            // f64 columns on 8-byte boundaries
  L.off_sum = w; w += 2 * P * NS;
  L.off_bits = w; w += P * L.NSW;
  L.rec_words = (w + 3) & ~3;  // records start on 16-byte boundaries
  L.tot_off_sum = MGX_PS_TOT_HDR + MGX_PS_TOT_POLICY * P;
  L.tot_off_cnt = L.tot_off_sum + P * NS;
  L.tot_words = L.tot_off_cnt + P * NS;
  return L;
}

struct MgxPolicyStats {
  MgxPsLayout L;
  uint8_t* assign;    // [E][A] policy index of every agent row
};

#ifndef MGX_CPU_EMU
// log_state: [0] records in the log, [1] records dropped since the last drain (log full).  PP: compile-time bound of L.P.
template <int PP>
__global__ void __launch_bounds__(256) mgx_policy_record_kernel(const MgxDev* __restrict__ dp, const MgxPolicyStats ps,
                                                                const int32_t* __restrict__ list, const uint32_t* __restrict__ list_n,
                                                                uint32_t* __restrict__ rec, uint32_t* __restrict__ log,
                                                                const uint32_t* __restrict__ log_state, int log_cap,
                                                                const uint32_t* __restrict__ early_steps, const uint32_t* __restrict__ episodes) {
  const MgxDev& d = *dp;
  const MgxPsLayout& L = ps.L;
  const int n = (int)*list_n;
  const int P = L.P;
  const int lane = threadIdx.x & (MGX_WAVE - 1);
  const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) / MGX_WAVE), nwaves = (int)(gridDim.x * blockDim.x / MGX_WAVE);
  const uint32_t log_base = log ? log_state[0] : 0u;
  for (int k = wave; k < n; k += nwaves) {
    const int env = list[k];
    uint32_t* R = rec + (size_t)k * L.rec_words;
    uint32_t* G = (log && log_base + (uint32_t)k < (uint32_t)log_cap) ? log + (size_t)(log_base + k) * L.rec_words : nullptr;
    const size_t a0 = (size_t)env * L.A;
    const uint8_t* asg = ps.assign + a0;
    // ---- agent stats: per column and policy the f64 sum over the policy's agents in agent order (summary.py:60-67) ----
    for (int c0 = 0; c0 < L.NS; c0 += MGX_WAVE) {
      const int c = c0 + lane;
      double s[PP];
#pragma unroll
      for (int p = 0; p < PP; p++) s[p] = 0.0;
      uint32_t anym = 0u;   // bit p: some agent of policy p holds the key
      const float* as = d.ag_stats + a0 * L.NSP + (c < L.NS ? c : 0);
      const uint32_t* at = d.ag_touched + a0 * L.NSW + (c < L.NS ? (c >> 5) : 0);
      for (int ab = 0; ab < L.A; ab += 8) {   // eight agents' loads in flight at a time, added in agent order
        float v[8];
        uint32_t tw[8], pa[8];
#pragma unroll
        for (int q = 0; q < 8; q++) {
          const int a = min(ab + q, L.A - 1);
          v[q] = as[(size_t)a * L.NSP];
          tw[q] = at[(size_t)a * L.NSW];
          pa[q] = asg[a];
        }
#pragma unroll
        for (int q = 0; q < 8; q++) {
          if (ab + q >= L.A) break;
          if (c < L.NS) {
            const double x = (double)v[q];
#pragma unroll
            for (int p = 0; p < PP; p++) s[p] += pa[q] == (uint32_t)p ? x : 0.0;   // (+0.0 changes no sum that started at +0.0)
            if (((tw[q] >> (c & 31)) & 1u) || v[q] != 0.f) anym |= 1u << pa[q];
          }
        }
      }
      if (c < L.NS) {
#pragma unroll
        for (int p = 0; p < PP; p++) {
          if (p < P) {
            const unsigned long long b = (unsigned long long)__double_as_longlong(s[p]);
            const int o = L.off_sum + 2 * (p * L.NS + c);
            R[o] = (uint32_t)b; R[o + 1] = (uint32_t)(b >> 32);
            if (G) { G[o] = (uint32_t)b; G[o + 1] = (uint32_t)(b >> 32); }
          }
        }
      }
      for (int p = 0; p < P; p++) {
        const unsigned long long m = __ballot((anym >> p) & 1u);
        if (lane == 0) {
          const int o = L.off_bits + p * L.NSW + (c0 >> 5);
          R[o] = (uint32_t)m;
          if ((c0 >> 5) + 1 < L.NSW) R[o + 1] = (uint32_t)(m >> 32);
          if (G) { G[o] = (uint32_t)m; if ((c0 >> 5) + 1 < L.NSW) G[o + 1] = (uint32_t)(m >> 32); }
        }
      }
    }
    // ---- episode rewards: lane p sums those of policy p's agents in agent order and counts them (summary.py:81-94) ----
    if (lane < P) {
      double r = 0.0;
      uint32_t cnt = 0u;
      for (int ab = 0; ab < L.A; ab += 8) {   // eight agents' loads in flight at a time, added in agent order
        float v[8];
        uint32_t pa[8];
#pragma unroll
        for (int q = 0; q < 8; q++) {
          const int a = min(ab + q, L.A - 1);
          v[q] = d.episode_rewards[a0 + a];
          pa[q] = asg[a];
        }
#pragma unroll
        for (int q = 0; q < 8; q++) {
          if (ab + q >= L.A) break;
          const bool mine = pa[q] == (uint32_t)lane;
          r += mine ? (double)v[q] : 0.0;   // (+0.0 changes no sum that started at +0.0)
          cnt += mine ? 1u : 0u;
        }
      }
      const unsigned long long b = (unsigned long long)__double_as_longlong(r);
      R[L.off_rew + 2 * lane] = (uint32_t)b; R[L.off_rew + 2 * lane + 1] = (uint32_t)(b >> 32); R[L.off_cnt + lane] = cnt;
      if (G) { G[L.off_rew + 2 * lane] = (uint32_t)b; G[L.off_rew + 2 * lane + 1] = (uint32_t)(b >> 32); G[L.off_cnt + lane] = cnt; }
    }
    // ---- flags, header, the record's padding ----
    bool all_term = true, all_trunc = true;
    for (int a = lane; a < L.A; a += MGX_WAVE) {
      all_term = all_term && d.terminals[a0 + a];
      all_trunc = all_trunc && d.truncations[a0 + a];
    }
    const bool at = __ballot(!all_term) == 0ull, au = __ballot(!all_trunc) == 0ull;
    if (lane < MGX_PS_HDR) {
      const uint32_t steps = d.step[env], ep = episodes ? episodes[env] : 0u;
      const bool early = early_steps && ep == 0 && early_steps[env] > 0 && steps >= early_steps[env];
      const uint32_t h = lane == 0 ? (uint32_t)env : lane == 1 ? ep : lane == 2 ? steps : (at ? 1u : 0u) | (au ? 2u : 0u) | (early ? 4u : 0u);
      R[lane] = h;
      if (G) G[lane] = h;
    }
    if ((P & 1) && lane == 0) { R[L.off_cnt + P] = 0u; if (G) G[L.off_cnt + P] = 0u; }
    for (int w = L.off_bits + P * L.NSW + lane; w < L.rec_words; w += MGX_WAVE) { R[w] = 0u; if (G) G[w] = 0u; }
  }
}

// totals / partial layout (doubles): [0] episodes; per policy p at 1 + 5 p: episodes in which p had an agent, agent-episodes,
// sum / min / max of reward_sum / count over those episodes; tot_off_sum: [P][NS] sums; tot_off_cnt: [P][NS] episodes in which
// some agent of p held the key.  Work items: the P * NS columns, then the P policy headers, one thread each; blockIdx.x walks
// the chunks, blockIdx.y the items in groups of blockDim.x, so that every item's serial pass over a chunk runs side by side
// with the others' (the pass is a chain of load latencies: sixteen records' loads in flight at a time).
struct MgxPsKind {   // field 3 of a policy header is a minimum, field 4 a maximum
  int tot_off_sum;
  __device__ int operator()(int c) const {
    const int f = (c >= MGX_PS_TOT_HDR && c < tot_off_sum) ? (c - MGX_PS_TOT_HDR) % MGX_PS_TOT_POLICY : 0;
    return f == 3 ? MGX_TOT_MIN : f == 4 ? MGX_TOT_MAX : MGX_TOT_SUM;
  }
};
__global__ void __launch_bounds__(256) mgx_policy_total_kernel(const MgxPsLayout L, const uint32_t* __restrict__ list_n,
                                                               const uint32_t* __restrict__ rec, double* __restrict__ partial,
                                                               double* __restrict__ totals, uint32_t* __restrict__ ticket,
                                                               uint32_t* __restrict__ log_state, int log_cap, int has_log) {
  const int n = (int)*list_n;
  if (n == 0) return;
  const int nchunks = (n + MGX_EP_CHUNK - 1) / MGX_EP_CHUNK;
  const int TW = L.tot_words, cols = L.P * L.NS;
  const double INF = __longlong_as_double(0x7FF0000000000000ll);
  const int j = (int)(blockIdx.y * blockDim.x + threadIdx.x);   // this thread's item
  for (int ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const int k0 = ch * MGX_EP_CHUNK, k1 = min(n, k0 + MGX_EP_CHUNK);
    double* Pt = partial + (size_t)ch * TW;
    if (j < cols) {
      const int p = j / L.NS, c = j - p * L.NS;
      const int os = L.off_sum + 2 * j, ob = L.off_bits + p * L.NSW + (c >> 5);
      double s = 0.0, cnt = 0.0;
      for (int kb = k0; kb < k1; kb += 16) {   // added in list order
        uint32_t lo[16], hi[16], tb[16];
#pragma unroll
        for (int q = 0; q < 16; q++) {
          const uint32_t* R = rec + (size_t)min(kb + q, k1 - 1) * L.rec_words;
          lo[q] = R[os]; hi[q] = R[os + 1]; tb[q] = R[ob];
        }
#pragma unroll
        for (int q = 0; q < 16; q++) {
          if (kb + q >= k1) break;
          s += __longlong_as_double((long long)((unsigned long long)lo[q] | ((unsigned long long)hi[q] << 32)));   // (a missing key holds +0)
          cnt += ((tb[q] >> (c & 31)) & 1u) ? 1.0 : 0.0;
        }
      }
      Pt[L.tot_off_sum + j] = s; Pt[L.tot_off_cnt + j] = cnt;
    } else if (j < cols + L.P) {   // policy hp's header, in list order
      const int hp = j - cols;
      double eps = 0.0, ag = 0.0, rs = 0.0, rmin = INF, rmax = -INF;
      for (int kb = k0; kb < k1; kb += 16) {
        uint32_t lo[16], hi[16], cn[16];
#pragma unroll
        for (int q = 0; q < 16; q++) {
          const uint32_t* R = rec + (size_t)min(kb + q, k1 - 1) * L.rec_words;
          lo[q] = R[L.off_rew + 2 * hp]; hi[q] = R[L.off_rew + 2 * hp + 1]; cn[q] = R[L.off_cnt + hp];
        }
#pragma unroll
        for (int q = 0; q < 16; q++) {
          if (kb + q >= k1) break;
          if (!cn[q]) continue;   // (summary.py:94: None, in no sum)
          const double r = __longlong_as_double((long long)((unsigned long long)lo[q] | ((unsigned long long)hi[q] << 32))) / (double)cn[q];
          eps += 1.0; ag += (double)cn[q];
          rs += r; rmin = fmin(rmin, r); rmax = fmax(rmax, r);
        }
      }
      double* H = Pt + MGX_PS_TOT_HDR + MGX_PS_TOT_POLICY * hp;
      H[0] = eps; H[1] = ag; H[2] = rs; H[3] = rmin; H[4] = rmax;
      if (hp == 0) Pt[0] = (double)(k1 - k0);
    }
  }
  mgx_totals_fold(MgxPsKind{L.tot_off_sum}, partial, totals, ticket, gridDim.x * gridDim.y, nchunks, TW, log_state, log_cap, has_log, n);
}

// assign[list[i]][0..A) <- rows[i][0..A) for the n listed envs (no env twice).
__global__ void __launch_bounds__(256) mgx_policy_assign_kernel(uint8_t* __restrict__ assign, const int32_t* __restrict__ list, int n,
                                                                const uint8_t* __restrict__ rows, int A) {
  const long long total = (long long)n * A;
  for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += (long long)gridDim.x * blockDim.x) {
    const int i = (int)(k / A), a = (int)(k - (long long)i * A);
    assign[(size_t)list[i] * A + a] = rows[k];
  }
}
#endif  // !MGX_CPU_EMU

#endif  // MGX_POLICY_STATS_H_
