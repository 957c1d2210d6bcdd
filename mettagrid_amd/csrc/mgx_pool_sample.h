// mgx_pool_sample.h — weighted draws of the next pool map at restart, and per-map episode statistics (include/mgx.h "Weighted
// map-pool sampling").
//
// Reference: the map cache hands every new episode a uniformly random cached map (python/src/mettagrid/simulator/map_cache.py:
// 207-215, rng.integers(0, len(maps_list))), the trainers' curricula feed per-task returns back into the task distribution, and
// StatsTracker reports per_label_rewards (python/src/mettagrid/envs/stats_tracker.py:59-60).  The rotation rule of
// mgx_clear_rows_env can do neither.  Here:
//
//   the draw     counter-based on numpy's own stream: for env slot e whose episode counter becomes k at the auto-reset bump,
//                u = Generator(PCG64(SeedSequence(sample_seed, spawn_key=(a, k)))).integers(0, 2^32, dtype=uint32) with
//                a = (env_offset + e) mod 2^32 — the low half of the stream's first output.  It depends on (seed, a, k) alone:
//                not on which envs restart together, nor in which order.  SeedSequence mixing, PCG64 seeding, step and XSL-RR
//                output are mgx_mapgen.h's; the two-word key is one more mix round per word (mgx_pcg64_seed_keys<2>).
//   the mapping  weights -> thresholds on the host in f64 (mgx_pool_quantise_host): C_m = C_(m-1) + w_m sequentially,
//                edge[m] = floor(C_m / C_(M-1) * 2^32) for m < M - 1 and edge[M-1] = 2^32; the map is the smallest m with
//                u < edge[m] (binary search).  A zero weight has an empty interval and is never drawn; a positive weight below
//                2^-32 of the total may have one too.
//   mgx_pool_draw_kernel   one thread per listed env, behind the bump of mgx_clear_rows_kernel: d_map_index[env] = the drawn
//                map.  The thresholds are read from global memory (a pool has a few dozen maps: the binary search's loads hit
//                the same few cache lines in every lane).  The same kernel answers mgx_pool_draws for caller-given (env,
//                episode) pairs.
//   mgx_map_stats_kernel   one thread per record of the step's done list, behind mgx_episode_record_kernel: row = the record's
//                map index (word [2]), or row n_maps for -1 (a slot's first episode).  Six unsigned 64-bit vector atomics per
//                record; integer adds, minima and maxima commute, so the table does not depend on arrival order.
//                The return sum is FIXED POINT by definition: q = (int64) rint(r * 2^20), round-half-even, two's complement;
//                minimum and maximum are taken on the total-order key of r (all bits flipped if negative, else sign bit set).
//                r = the record's f64 reward sum / A, the value MGX_EPT_RETURN_SUM sums.
//   mgx_map_stats_snapshot_kernel   table -> snapshot, table cleared (sums 0, minimum key all ones, maximum key 0).
//
// The draw and the pick are __host__ __device__: mgx_pool_draw_words and mgx_pool_draws' checks run this source on the host.
#ifndef MGX_POOL_SAMPLE_H_
#define MGX_POOL_SAMPLE_H_

#include "mgx_mapgen.h"

#define MGX_MS_COLS 6            // include/mgx.h MGX_MS_*
#define MGX_MS_Q_SCALE 1048576.0 // 2^20

#ifndef MGX_CPU_EMU
struct MgxPoolSample {
  const unsigned long long* edges;   // [n_maps] upper edges of the maps' intervals of [0, 2^32), the last one 2^32
  int n_maps;
  uint32_t seed, offset;
};

// The low 32 bits of the first output of PCG64(SeedSequence(seed, spawn_key=(a, k))).
__host__ __device__ __forceinline__ uint32_t mgx_pool_draw_word(uint32_t seed, uint32_t a, uint32_t k) {
  const uint32_t keys[2] = {a, k};
  MgxU128 s, inc;
  mgx_pcg64_seed_keys<2>(seed, s, inc, keys);
  s = mgx_add128(mgx_mul128(s, MGX_PCG_MULT), inc);   // next64: step, then XSL-RR of the new state
  const unsigned long long x = s.hi ^ s.lo;
  const unsigned rot = (unsigned)(s.hi >> 58);
  return (uint32_t)((x >> rot) | (x << ((64u - rot) & 63u)));
}
// The smallest m with u < edges[m] (edges[n - 1] = 2^32 > u: the search never leaves [0, n)).
__host__ __device__ __forceinline__ int mgx_pool_pick(const unsigned long long* __restrict__ edges, int n, uint32_t u) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((unsigned long long)u < edges[mid]) hi = mid; else lo = mid + 1;
  }
  return lo;
}
// Weights -> thresholds (host, f64).  Returns nullptr, or why the weights are refused (edges untouched).
static inline const char* mgx_pool_quantise_host(const double* w, int n, unsigned long long* edges) {
  if (!w || !edges || n <= 0) return "null / empty argument";
  double total = 0.0;
  for (int m = 0; m < n; m++) {
    if (!(w[m] >= 0.0) || w[m] > 1.7976931348623157e308) return "a weight is negative, NaN or infinite";
    total = total + w[m];
  }
  if (!(total > 0.0) || total > 1.7976931348623157e308) return "the weights' total is zero or not finite";
  double c = 0.0;
  for (int m = 0; m < n; m++) {
    c = c + w[m];
    edges[m] = m == n - 1 ? 4294967296ull : (unsigned long long)floor(c / total * 4294967296.0);
  }
  return nullptr;
}

// Entry k of the list (n_dev: its length when only the device knows it, else n): env = list[k]; episode = given[k] when given,
// else episodes[env] (the counter the restart has just bumped); out[given ? k : env] = the drawn map.
__global__ void __launch_bounds__(256) mgx_pool_draw_kernel(const MgxPoolSample s, const int32_t* __restrict__ list,
                                                            const uint32_t* __restrict__ n_dev, int n, const uint32_t* __restrict__ episodes,
                                                            const uint32_t* __restrict__ given, int32_t* __restrict__ out) {
  const int count = n_dev ? (int)*n_dev : n;
  for (int k = (int)(blockIdx.x * blockDim.x + threadIdx.x); k < count; k += (int)(gridDim.x * blockDim.x)) {
    const int env = list[k];
    const uint32_t ep = given ? given[k] : episodes[env];
    const uint32_t u = mgx_pool_draw_word(s.seed, s.offset + (uint32_t)env, ep);
    out[given ? k : env] = mgx_pool_pick(s.edges, s.n_maps, u);
  }
}

__device__ __forceinline__ unsigned long long mgx_ms_key(double r) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(r);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
// rec: the step's episode records (mgx_episode.h: [2] map index, [4] steps, [5] flags, [6..7] f64 reward sum), *list_n of them.
// table: [n_maps + 1][MGX_MS_COLS]; a map index outside [0, n_maps) counts in the last row.
__global__ void __launch_bounds__(256) mgx_map_stats_kernel(const uint32_t* __restrict__ list_n, const uint32_t* __restrict__ rec, int rec_words,
                                                            int A, int n_maps, unsigned long long* __restrict__ table) {
  const int n = (int)*list_n;
  for (int k = (int)(blockIdx.x * blockDim.x + threadIdx.x); k < n; k += (int)(gridDim.x * blockDim.x)) {
    const uint32_t* R = rec + (size_t)k * rec_words;
    const uint32_t mi = R[2];
    const uint4 h = *(const uint4*)(R + 4);   // steps, flags, f64 reward sum (records start on 16-byte boundaries)
    const double r = __longlong_as_double((long long)((unsigned long long)h.z | ((unsigned long long)h.w << 32))) / (double)A;
    const long long q = (long long)rint(r * MGX_MS_Q_SCALE);
    const unsigned long long key = mgx_ms_key(r);
    unsigned long long* T = table + (size_t)(mi < (uint32_t)n_maps ? (int)mi : n_maps) * MGX_MS_COLS;
    atomicAdd(T + 0, 1ull);
    if (h.y & 1u) atomicAdd(T + 1, 1ull);
    atomicAdd(T + 2, (unsigned long long)h.x);
    atomicAdd(T + 3, (unsigned long long)q);
    atomicMin(T + 4, key);
    atomicMax(T + 5, key);
  }
}

__global__ void __launch_bounds__(256) mgx_map_stats_snapshot_kernel(unsigned long long* __restrict__ table, unsigned long long* __restrict__ snap,
                                                                     int words) {
  for (int c = threadIdx.x; c < words; c += blockDim.x) {
    snap[c] = table[c];
    table[c] = (c % MGX_MS_COLS) == 4 ? ~0ull : 0ull;
  }
}
#endif  // MGX_CPU_EMU
#endif  // MGX_POOL_SAMPLE_H_
