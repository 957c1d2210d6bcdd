// mgx_totals.h — the part the statistics reducers share on the device (mgx_episode.h, mgx_time_avg.h, mgx_policy_stats.h;
// DESIGN.md §7e-1): chunk sums -> batch totals in a fixed order, and totals -> snapshot.
//
// A reducer's total kernel writes one row of f64 chunk sums per chunk of MGX_EP_CHUNK records into `partial` and ends in
// mgx_totals_fold: the workgroup that draws the last ticket adds the rows to `totals` in chunk order, so the totals do not
// depend on which workgroup finishes when.  Whether a totals column is a sum, a minimum or a maximum is the reducer's KIND, a
// functor `int operator()(int c) const` returning MGX_TOT_SUM / _MIN / _MAX; the snapshot kernel clears by the same rule.
#ifndef MGX_TOTALS_H_
#define MGX_TOTALS_H_

#include "mgx_device.h"

#define MGX_TOT_SUM 0
#define MGX_TOT_MIN 1
#define MGX_TOT_MAX 2

#ifndef MGX_CPU_EMU
// The tail of a total kernel, called by every thread of every workgroup once its chunks' rows are written.  n_blocks: the
// workgroups of the launch; n: the step's records (> 0); log_state: [0] records in the log, [1] records dropped since the
// last drain (log full), advanced here because the record kernel of the same step reads [0] as its base.
template <class Kind>
__device__ __forceinline__ void mgx_totals_fold(const Kind kind, const double* __restrict__ partial, double* __restrict__ totals,
                                                uint32_t* __restrict__ ticket, unsigned n_blocks, int nchunks, int TW,
                                                uint32_t* __restrict__ log_state, int log_cap, int has_log, int n) {
  __threadfence();
  __syncthreads();
  __shared__ uint32_t s_last;
  if (threadIdx.x == 0) s_last = atomicAdd(ticket, 1u) == n_blocks - 1 ? 1u : 0u;
  __syncthreads();
  if (!s_last) return;
  __threadfence();
  for (int c = threadIdx.x; c < TW; c += blockDim.x) {   // totals += chunk sums, in chunk order
    double t = totals[c];
    const int k = kind(c);
    for (int ch = 0; ch < nchunks; ch++) {
      const double p = __longlong_as_double((long long)__hip_atomic_load((const unsigned long long*)(partial + (size_t)ch * TW + c),
                                                                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
      t = k == MGX_TOT_MIN ? fmin(t, p) : k == MGX_TOT_MAX ? fmax(t, p) : t + p;
    }
    totals[c] = t;
  }
  if (threadIdx.x == 0) {
    *ticket = 0;
    if (has_log) {
      const uint32_t have = log_state[0], room = (uint32_t)log_cap - have, take = (uint32_t)n < room ? (uint32_t)n : room;
      log_state[0] = have + take;
      log_state[1] += (uint32_t)n - take;
    }
  }
}

// totals -> snapshot, totals cleared (sums 0, minima +inf, maxima -inf).
template <class Kind>
__global__ void __launch_bounds__(256) mgx_totals_snapshot_kernel(const Kind kind, double* __restrict__ totals, double* __restrict__ snap, int TW) {
  const double INF = __longlong_as_double(0x7FF0000000000000ll);
  for (int c = threadIdx.x; c < TW; c += blockDim.x) {
    const int k = kind(c);
    snap[c] = totals[c];
    totals[c] = k == MGX_TOT_MIN ? INF : k == MGX_TOT_MAX ? -INF : 0.0;
  }
}
#endif  // !MGX_CPU_EMU

#endif  // MGX_TOTALS_H_
