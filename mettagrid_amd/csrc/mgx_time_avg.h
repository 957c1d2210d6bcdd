// mgx_time_avg.h — time-averaged game stats of every episode, accumulated on the device.
//
// Reference: the episode runner attaches a TimeAveragedStatsHandler to every evaluation episode
// (python/src/mettagrid/simulator/time_averaged_stats.py:17-41, used at runner/rollout.py:107-135): after every sim.step() it
// adds each value of episode_stats["game"] into a Python-float (f64) sum and reports sum / steps per key at the end
// (time_averaged_game_stats), which simulator/multi_episode/summary.py:50-77 averages over episodes.  The end-of-episode
// snapshot (mgx_episode.h) cannot give this, and with the on-device auto-reset the sums have to be finished before the restart
// wipes the env:
//
//   mgx_time_avg_accum_kernel    every step: one LANE per (env, column) slot, flat over E * NGP (NGP = NG rounded up to 32, so
//                                that the 32 columns of one `seen` word are one half-wavefront and the word is one ballot: no
//                                atomics, no LDS).  sum += (double)value; seen |= exists (touched bit OR value != 0, the rule of
//                                mgx_get_stats); the lane of column 0 bumps ta_steps.  The padding lanes touch no memory, so
//                                the f32 loads, f64 loads and f64 stores of a wavefront are each one contiguous run.
//                                A key the reference's dict does not hold has value +-0 and x + +-0 == x for the sums that occur
//                                (they start at +0.0): adding unconditionally gives the reference's bits.
//   mgx_time_avg_finish_kernel   one WAVEFRONT per finished env (ordered done list), lane = column: sum / (double)ta_steps
//                                (correctly rounded f64 division) -> one RECORD per finished env in list order, and into a
//                                bounded LOG.  An episode whose ta_steps differs from the env's step is PARTIAL (flag).
//   mgx_time_avg_total_kernel    records -> batch totals in the fixed order of mgx_episode_accum_kernel: list order, chunks of
//                                MGX_EP_CHUNK, chunk sums added in chunk order by the last workgroup.  Partial episodes are
//                                left out and counted.
//   mgx_time_avg_clear_kernel    the three arrays of a list (or mask) of envs -> 0 (episode restart, mgx_load_envs).
//   mgx_time_avg_move_kernel     raw gather / scatter of the accumulators of a list of envs (get / put, mgx_copy_envs).
//
// The state (ta_sum f64 [E][NG], ta_seen u32 [E][NGW], ta_steps u32 [E]) exists only while the feature is on and is NOT part
// of the saved env record (mgx_env_state.h): mgx_copy_envs copies it, mgx_load_envs zeroes it.
#ifndef MGX_TIME_AVG_H_
#define MGX_TIME_AVG_H_

#include "mgx_device.h"
#include "mgx_episode.h"

#define MGX_TA_HDR 8            // record header words: env, episode, step, ta_steps, flags, 3 x 0 (f64 columns on 8-byte boundaries)
#define MGX_TA_TOT_HDR 2        // totals header doubles: episodes, partial episodes
#define MGX_TA_FLAG_PARTIAL 2u  // flags bit 1

struct MgxTaLayout {
  int NG, NGW, NGP;                    // columns, seen words, lane slots per env (NGW * 32)
  int off_avg, off_seen, rec_words;    // the record (32-bit words); a log record is the same
  int tot_words;                       // totals (doubles): header, NG sums of per-episode averages, NG counts of episodes holding the key
};

static inline MgxTaLayout mgx_ta_layout(int NG) {
  MgxTaLayout L{};
  L.NG = NG; L.NGW = (NG + 31) / 32; L.NGP = L.NGW * 32;
  int w = MGX_TA_HDR;
  L.off_avg = w; w += 2 * NG;
  L.off_seen = w; w += L.NGW;
  L.rec_words = (w + 3) & ~3;
  L.tot_words = MGX_TA_TOT_HDR + 2 * NG;
  return L;
}

struct MgxTimeAvg {
  MgxTaLayout L;
  double* sum;        // [E][NG]
  uint32_t* seen;     // [E][NGW]
  uint32_t* steps;    // [E]
};

#ifndef MGX_CPU_EMU
__global__ void __launch_bounds__(256) mgx_time_avg_accum_kernel(const MgxDev* __restrict__ dp, const MgxTimeAvg ta) {
  const MgxDev& d = *dp;
  const int NG = ta.L.NG, NGW = ta.L.NGW, NGP = ta.L.NGP;
  const long long total = (long long)d.E * NGP;   // a multiple of 32: a wavefront's last half may be out of range
  const int lane = threadIdx.x & (MGX_WAVE - 1);
  for (long long base = (long long)blockIdx.x * blockDim.x + (threadIdx.x - lane); base < total; base += (long long)gridDim.x * blockDim.x) {
    const long long k = base + lane;
    long long env = 0;
    int c = NGP;
    if (k < total) {
      if (k < (1ll << 31)) { const uint32_t q = (uint32_t)k / (uint32_t)NGP; env = q; c = (int)((uint32_t)k - q * (uint32_t)NGP); }
      else { env = k / NGP; c = (int)(k - env * NGP); }
    }
    const bool active = c < NG;
    bool t = false;
    if (active) {
      const size_t o = (size_t)env * NG + c;
      const float v = d.game_stats[o];
      const uint32_t tw = d.game_touched[(size_t)env * NGW + (c >> 5)];
      t = ((tw >> (c & 31)) & 1u) || v != 0.f;
      ta.sum[o] += (double)v;
      if (c == 0) ta.steps[env] += 1u;
    }
    const unsigned long long m = __ballot(t);
    if (active && (lane & 31) == 0) {   // c is a multiple of 32 here: the ballot half of this lane is seen word c >> 5
      const uint32_t bits = (uint32_t)(lane ? (m >> 32) : m);
      if (bits) {
        uint32_t* w = ta.seen + (size_t)env * NGW + (c >> 5);
        const uint32_t old = *w;
        if ((old | bits) != old) *w = old | bits;
      }
    }
  }
}

// log_state: [0] records in the log, [1] records dropped since the last drain (log full).
__global__ void __launch_bounds__(256) mgx_time_avg_finish_kernel(const MgxDev* __restrict__ dp, const MgxTimeAvg ta,
                                                                  const int32_t* __restrict__ list, const uint32_t* __restrict__ list_n,
                                                                  uint32_t* __restrict__ rec, uint32_t* __restrict__ log,
                                                                  const uint32_t* __restrict__ log_state, int log_cap,
                                                                  const uint32_t* __restrict__ episodes) {
  const MgxDev& d = *dp;
  const MgxTaLayout& L = ta.L;
  const int n = (int)*list_n;
  const int lane = threadIdx.x & (MGX_WAVE - 1);
  const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) / MGX_WAVE), nwaves = (int)(gridDim.x * blockDim.x / MGX_WAVE);
  const uint32_t log_base = log ? log_state[0] : 0u;
  for (int k = wave; k < n; k += nwaves) {
    const int env = list[k];
    uint32_t* R = rec + (size_t)k * L.rec_words;
    uint32_t* G = (log && log_base + (uint32_t)k < (uint32_t)log_cap) ? log + (size_t)(log_base + k) * L.rec_words : nullptr;
    const uint32_t ts = ta.steps[env];
    const double den = (double)ts;
    for (int c = lane; c < L.NG; c += MGX_WAVE) {
      const double avg = ts ? ta.sum[(size_t)env * L.NG + c] / den : 0.0;
      const unsigned long long b = (unsigned long long)__double_as_longlong(avg);
      R[L.off_avg + 2 * c] = (uint32_t)b; R[L.off_avg + 2 * c + 1] = (uint32_t)(b >> 32);
      if (G) { G[L.off_avg + 2 * c] = (uint32_t)b; G[L.off_avg + 2 * c + 1] = (uint32_t)(b >> 32); }
    }
    for (int w = lane; w < L.rec_words - L.off_seen; w += MGX_WAVE) {   // seen words, then the record's padding
      const uint32_t s = w < L.NGW ? ta.seen[(size_t)env * L.NGW + w] : 0u;
      R[L.off_seen + w] = s;
      if (G) G[L.off_seen + w] = s;
    }
    if (lane < MGX_TA_HDR) {
      const uint32_t step = d.step[env];
      const uint32_t h = lane == 0 ? (uint32_t)env : lane == 1 ? (episodes ? episodes[env] : 0u) : lane == 2 ? step : lane == 3 ? ts
                         : lane == 4 ? (ts != step ? MGX_TA_FLAG_PARTIAL : 0u) : 0u;
      R[lane] = h;
      if (G) G[lane] = h;
    }
  }
}

// totals / partial layout (doubles): [0] episodes (not partial) [1] partial episodes [NG sums of the averages][NG key counts]
struct MgxTaKind {
  __device__ int operator()(int) const { return MGX_TOT_SUM; }
};
__global__ void __launch_bounds__(256) mgx_time_avg_total_kernel(const MgxTaLayout L, const uint32_t* __restrict__ list_n,
                                                                 const uint32_t* __restrict__ rec, double* __restrict__ partial,
                                                                 double* __restrict__ totals, uint32_t* __restrict__ ticket,
                                                                 uint32_t* __restrict__ log_state, int log_cap, int has_log) {
  const int n = (int)*list_n;
  if (n == 0) return;
  const int nchunks = (n + MGX_EP_CHUNK - 1) / MGX_EP_CHUNK;
  const int TW = L.tot_words;
  for (int ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const int k0 = ch * MGX_EP_CHUNK, k1 = min(n, k0 + MGX_EP_CHUNK);
    double* P = partial + (size_t)ch * TW;
    for (int c = threadIdx.x; c < L.NG; c += blockDim.x) {
      double s = 0.0, cnt = 0.0;
      for (int kb = k0; kb < k1; kb += 8) {   // eight records' loads in flight at a time, added in list order
        uint32_t lo[8], hi[8], tb[8], fl[8];
#pragma unroll
        for (int q = 0; q < 8; q++) {
          const uint32_t* R = rec + (size_t)min(kb + q, k1 - 1) * L.rec_words;
          lo[q] = R[L.off_avg + 2 * c]; hi[q] = R[L.off_avg + 2 * c + 1]; tb[q] = R[L.off_seen + (c >> 5)]; fl[q] = R[4];
        }
#pragma unroll
        for (int q = 0; q < 8; q++) {
          if (kb + q >= k1) break;
          if (fl[q] & MGX_TA_FLAG_PARTIAL) continue;
          s += __longlong_as_double((long long)((unsigned long long)lo[q] | ((unsigned long long)hi[q] << 32)));   // (a missing key holds +0)
          cnt += ((tb[q] >> (c & 31)) & 1u) ? 1.0 : 0.0;
        }
      }
      P[MGX_TA_TOT_HDR + c] = s; P[MGX_TA_TOT_HDR + L.NG + c] = cnt;
    }
    if (threadIdx.x == blockDim.x - 1) {
      double full = 0.0, part = 0.0;
      for (int k = k0; k < k1; k++) {
        if (rec[(size_t)k * L.rec_words + 4] & MGX_TA_FLAG_PARTIAL) part += 1.0; else full += 1.0;
      }
      P[0] = full; P[1] = part;
    }
  }
  mgx_totals_fold(MgxTaKind{}, partial, totals, ticket, gridDim.x, nchunks, TW, log_state, log_cap, has_log, n);
}

// The accumulators of the listed envs (n on the device, or n_host >= 0) or of the masked envs (list == nullptr) -> 0.
__global__ void __launch_bounds__(256) mgx_time_avg_clear_kernel(const MgxTimeAvg ta, const int32_t* __restrict__ list,
                                                                 const uint32_t* __restrict__ list_n, int n_host,
                                                                 const uint8_t* __restrict__ mask, int E) {
  const MgxTaLayout& L = ta.L;
  const int n = list ? (n_host >= 0 ? n_host : (int)*list_n) : E;
  for (int k = blockIdx.x; k < n; k += gridDim.x) {
    const int env = list ? list[k] : k;
    if (!list && !mask[env]) continue;
    for (int c = threadIdx.x; c < L.NG; c += blockDim.x) ta.sum[(size_t)env * L.NG + c] = 0.0;
    for (int w = threadIdx.x; w < L.NGW; w += blockDim.x) ta.seen[(size_t)env * L.NGW + w] = 0u;
    if (threadIdx.x == 0) ta.steps[env] = 0u;
  }
}

// Raw accumulators of the n listed envs <-> a packed block [n][NG] f64 sums, [n][NGW] u32 seen, [n] u32 steps.  dir 0: get.
static inline size_t mgx_ta_block_bytes(const MgxTaLayout& L, size_t n) { return n * ((size_t)L.NG * 8 + (size_t)L.NGW * 4 + 4); }
__global__ void __launch_bounds__(256) mgx_time_avg_move_kernel(const MgxTimeAvg ta, const int32_t* __restrict__ list, int n,
                                                                uint8_t* __restrict__ block, int dir) {
  const MgxTaLayout& L = ta.L;
  double* bsum = (double*)block;
  uint32_t* bseen = (uint32_t*)(block + (size_t)n * L.NG * 8);
  uint32_t* bsteps = bseen + (size_t)n * L.NGW;
  const long long stride = (long long)gridDim.x * blockDim.x, t0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (long long k = t0; k < (long long)n * L.NG; k += stride) {
    const int i = (int)(k / L.NG), c = (int)(k - (long long)i * L.NG);
    double* p = ta.sum + (size_t)list[i] * L.NG + c;
    if (dir == 0) bsum[k] = *p; else *p = bsum[k];
  }
  for (long long k = t0; k < (long long)n * L.NGW; k += stride) {
    const int i = (int)(k / L.NGW), w = (int)(k - (long long)i * L.NGW);
    uint32_t* p = ta.seen + (size_t)list[i] * L.NGW + w;
    if (dir == 0) bseen[k] = *p; else *p = bseen[k];
  }
  for (long long k = t0; k < n; k += stride) {
    uint32_t* p = ta.steps + list[k];
    if (dir == 0) bsteps[k] = *p; else *p = bsteps[k];
  }
}
#endif  // !MGX_CPU_EMU

#endif  // MGX_TIME_AVG_H_
