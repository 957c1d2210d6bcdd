// mgx_sample.hip — the output side of a policy: from logits to sampled actions, their log-probabilities and entropies, and the
// gradient of both (include/mgx.h mgx_sample_actions / mgx_action_logprob / mgx_action_logprob_backward).
// The reference policies end in Categorical(logits=logits).sample() or pufferlib's sample_logits
// (python/src/mettagrid/policy/lstm.py:232, stateless.py:98, token_encoder.py:149), a trainer re-evaluates log_prob and
// entropy with a gradient: in torch six or more passes over a [N, A] float tensor.  Here every kernel reads the logits once.
//
//   z_a = fl(t * l_a)   m = max z   pt_a = exp(z_a - m)   S = sum pt_a   logp_a = z_a - m - log S
//   H = log S - (sum_{pt_a > 0} pt_a (z_a - m)) / S                      (a term with pt_a = 0 is exactly 0: masked actions)
//   sampled a = the smallest a with c_a > u c_{A-1}, c the running sum of pt in index order, u from Philox4x32-10 keyed by
//   the seed, counter (row, step): a row's draw does not depend on N, on the launch or on how rows are split between calls.
//
// Two forms, chosen on the host (sa_lane_path):
//   lane per row   A <= 64 and the rows back to back (row_stride == A).  A workgroup of 128 threads copies the flat span of
//                  its 128 rows into LDS with 16-byte loads (z as float32, row pitch A | 1 words: a lane's row starts on its
//                  own bank), then lane i walks row i out of LDS: a max pass, a sum pass that leaves pt in place, and for the
//                  sampler a scan pass.  No cross-lane traffic.  The backward kernel writes the gradient over z in LDS and the
//                  workgroup stores the span flat again.
//   wave per row   every other shape (A up to 4096, any row stride): lanes stride the row, wave reductions for m and the
//                  sums, a wave prefix scan per 64-element chunk for c (the same scan code gives S and finds the crossing,
//                  so both see the same bits); the row is read three times, twice out of L2.
// exp / log are the library's (expf / logf, within 2 ulp), not the fast hardware forms.  Plain C++ and vector stores only; the
// bad-row counter is one atomicAdd per workgroup at most.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mgx.h"

#define MGX_SA_ROWS 128        // lane per row: rows (= threads) per workgroup
#define MGX_SA_LANE_MAX_A 64   // lane per row: largest A
#define MGX_SA_BATCH 4         // lane per row: 16-byte loads a thread keeps in flight while staging
#define MGX_SA_WAVES 4         // wave per row: rows (= wavefronts) per workgroup
#define MGX_SA_MAX_A 4096
#define MGX_SA_MAX_ROWS ((int64_t)1 << 25)   // (a wavefront per row: 2^31 threads per launch)
enum { MGX_SA_F32 = 1, MGX_SA_BF16 = 2 };   // the dtype codes of include/mgx.h

__device__ static inline float sa_bf16_float(uint32_t bits) { return __uint_as_float(bits << 16); }
__device__ static inline uint32_t sa_bf16(float v) { return (uint32_t)__builtin_bit_cast(unsigned short, (__bf16)v); }

template <int BF16>
__device__ static inline float sa_elem(const void* __restrict__ p, long long idx) {
  return BF16 ? sa_bf16_float(((const uint16_t*)p)[idx]) : ((const float*)p)[idx];
}

// Philox4x32-10 (Salmon et al., SC'11): the first output word of counter (c0, c1, c2, c3) under key (k0, k1)
__device__ static inline uint32_t sa_philox_x0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; r++) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c0;
}

// u in [0, 1) of output row r at step `step`
__device__ static inline float sa_uniform(unsigned long long seed, unsigned long long step, unsigned long long r) {
  const uint32_t x0 = sa_philox_x0((uint32_t)r, (uint32_t)(r >> 32), (uint32_t)step, (uint32_t)(step >> 32), (uint32_t)seed, (uint32_t)(seed >> 32));
  return (float)(x0 >> 8) * 0x1p-24f;
}

__device__ static inline bool sa_is_bad(float z) { return z != z || z == INFINITY; }   // NaN or +inf

// ---- lane per row -------------------------------------------------------------------------------------------------------

// z = fl(t * l) of the n_el elements behind element e0 (whole rows, back to back) into LDS at row pitch P; reads nothing
// outside [e0, e0 + n_el)
template <int BF16>
__device__ static inline void sa_stage(const void* __restrict__ logits, long long e0, int n_el, int A, int P, float t, float* __restrict__ lds) {
  const int tid = (int)threadIdx.x;
  constexpr int V = BF16 ? 8 : 4;   // elements of a 16-byte load
  const bool vec = (((uintptr_t)logits) & 15) == 0;   // (e0 is a multiple of 128 A elements: the span starts 16-aligned then)
  const int nv = vec ? n_el / V : 0;
  // MGX_SA_BATCH loads per thread are issued before the first is used: with one in flight a workgroup would wait a memory
  // latency per 2 KB
  const uint4* __restrict__ src = (const uint4*)((const uint8_t*)logits + e0 * (BF16 ? 2 : 4));
  for (int v0 = tid; v0 < nv; v0 += MGX_SA_BATCH * MGX_SA_ROWS) {
    uint4 q[MGX_SA_BATCH];
#pragma unroll
    for (int b = 0; b < MGX_SA_BATCH; b++) {
      const int v = v0 + b * MGX_SA_ROWS;
      q[b] = v < nv ? src[v] : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int b = 0; b < MGX_SA_BATCH; b++) {
      const int v = v0 + b * MGX_SA_ROWS;
      if (v < nv) {
        const uint32_t w[4] = {q[b].x, q[b].y, q[b].z, q[b].w};
        float x[V];
#pragma unroll
        for (int j = 0; j < 4; j++) {
          if (!BF16) x[j] = __uint_as_float(w[j]);
          else { x[2 * j] = sa_bf16_float(w[j] & 0xFFFFu); x[2 * j + 1] = sa_bf16_float(w[j] >> 16); }
        }
        int r = (V * v) / A, c = V * v - r * A;
#pragma unroll
        for (int j = 0; j < V; j++) {
          lds[r * P + c] = __fmul_rn(t, x[j]);
          if (++c == A) { c = 0; r++; }
        }
      }
    }
  }
  for (int e = nv * V + tid; e < n_el; e += MGX_SA_ROWS) {
    const int r = e / A, c = e - r * A;
    lds[r * P + c] = __fmul_rn(t, sa_elem<BF16>(logits, e0 + e));
  }
}

struct SaStats {
  float m, S, T;   // max z, sum pt, sum pt (z - m)
  int amax;        // lowest index among the maxima
  bool bad;
};

// a lane's walk over its row z[0 .. A) in LDS; STORE_P leaves pt_a in place of z_a
template <int STORE_P>
__device__ static inline SaStats sa_lane_stats(float* __restrict__ z, int A) {
  SaStats s;
  s.m = -INFINITY; s.amax = 0; s.bad = false;
#pragma unroll 4
  for (int a = 0; a < A; a++) {
    const float v = z[a];
    s.bad |= sa_is_bad(v);
    if (v > s.m) { s.m = v; s.amax = a; }
  }
  s.bad |= s.m == -INFINITY;   // no finite entry
  s.S = 0.f; s.T = 0.f;
  if (s.bad) return s;
#pragma unroll 4
  for (int a = 0; a < A; a++) {
    const float d = z[a] - s.m, p = expf(d);
    s.S = __fadd_rn(s.S, p);
    if (p > 0.f) s.T = fmaf(p, d, s.T);
    if (STORE_P) z[a] = p;
  }
  return s;
}

// one atomic per workgroup at most
__device__ static inline void sa_count_bad(bool bad, unsigned int* __restrict__ bad_rows) {
  const int n = __syncthreads_count(bad ? 1 : 0);
  if (bad_rows && n > 0 && threadIdx.x == 0) atomicAdd(bad_rows, (unsigned int)n);
}

template <int BF16>
__global__ void __launch_bounds__(MGX_SA_ROWS)
mgx_sample_lane_kernel(const void* __restrict__ logits, long long N, int A, const long long* __restrict__ rows, float t, int greedy,
                       unsigned long long seed, unsigned long long step, int* __restrict__ actions, float* __restrict__ logprob,
                       float* __restrict__ entropy, unsigned int* __restrict__ bad_rows) {
  extern __shared__ __align__(16) float sa_lds[];
  const int P = A | 1;
  const long long row0 = (long long)blockIdx.x * MGX_SA_ROWS;
  const int here = N - row0 < MGX_SA_ROWS ? (int)(N - row0) : MGX_SA_ROWS;
  sa_stage<BF16>(logits, row0 * A, here * A, A, P, t, sa_lds);
  __syncthreads();
  const int tid = (int)threadIdx.x;
  bool bad = false;
  if (tid < here) {
    const long long i = row0 + tid, r = rows ? rows[i] : i;
    float* z = sa_lds + tid * P;
    const SaStats s = sa_lane_stats<1>(z, A);
    bad = s.bad;
    int act = 0;
    float lp = NAN, ent = NAN;
    if (!bad) {
      float zd = 0.f;   // z_act - m
      if (greedy) {
        act = s.amax;
      } else {
        const float thr = __fmul_rn(sa_uniform(seed, step, (unsigned long long)r), s.S);
        float c = 0.f;
        int last = 0;
        act = -1;
#pragma unroll 4
        for (int a = 0; a < A; a++) {
          const float p = z[a];
          c = __fadd_rn(c, p);
          if (act < 0 && c > thr) act = a;
          if (p > 0.f) last = a;
        }
        if (act < 0) act = last;
        zd = __fmul_rn(t, sa_elem<BF16>(logits, i * A + act)) - s.m;
      }
      const float ls = logf(s.S);
      lp = zd - ls;
      ent = ls - s.T / s.S;
    }
    actions[r] = act;
    if (logprob) logprob[r] = lp;
    if (entropy) entropy[r] = ent;
  }
  sa_count_bad(bad, bad_rows);
}

template <int BF16>
__global__ void __launch_bounds__(MGX_SA_ROWS)
mgx_logprob_lane_kernel(const void* __restrict__ logits, long long N, int A, const int* __restrict__ actions, float t,
                        float* __restrict__ logprob, float* __restrict__ entropy, float* __restrict__ lse, unsigned int* __restrict__ bad_rows) {
  extern __shared__ __align__(16) float sa_lds[];
  const int P = A | 1;
  const long long row0 = (long long)blockIdx.x * MGX_SA_ROWS;
  const int here = N - row0 < MGX_SA_ROWS ? (int)(N - row0) : MGX_SA_ROWS;
  sa_stage<BF16>(logits, row0 * A, here * A, A, P, t, sa_lds);
  __syncthreads();
  const int tid = (int)threadIdx.x;
  bool bad = false;
  if (tid < here) {
    const long long i = row0 + tid;
    const float* z = sa_lds + tid * P;
    const int act = actions[i];
    const bool in_range = act >= 0 && act < A;
    const float za = in_range ? z[act] : 0.f;
    const SaStats s = sa_lane_stats<0>(sa_lds + tid * P, A);
    bad = s.bad || !in_range;
    float lp = NAN, ent = NAN, l = NAN;
    if (!bad) {
      const float ls = logf(s.S);
      lp = (za - s.m) - ls;
      ent = ls - s.T / s.S;
      l = s.m + ls;
    }
    logprob[i] = lp;
    if (entropy) entropy[i] = ent;
    if (lse) lse[i] = l;
  }
  sa_count_bad(bad, bad_rows);
}

// d_logits[a] = t (dlp ([a = act] - p_a) - dH p_a (logp_a + H)), exactly 0 where z_a = -inf
__device__ static inline float sa_grad(float z, float l, float H, bool is_act, float t, float dlp, float dH) {
  if (z == -INFINITY) return 0.f;
  const float lp = z - l, p = expf(lp);
  return __fmul_rn(t, dlp * ((is_act ? 1.f : 0.f) - p) - dH * (p * (lp + H)));
}

template <int BF16, int D_BF16>
__global__ void __launch_bounds__(MGX_SA_ROWS)
mgx_logprob_bwd_lane_kernel(const void* __restrict__ logits, long long N, int A, const int* __restrict__ actions, float t,
                            const float* __restrict__ lse, const float* __restrict__ d_logprob, const float* __restrict__ d_entropy,
                            void* __restrict__ d_logits) {
  extern __shared__ __align__(16) float sa_lds[];
  const int P = A | 1;
  const long long row0 = (long long)blockIdx.x * MGX_SA_ROWS;
  const int here = N - row0 < MGX_SA_ROWS ? (int)(N - row0) : MGX_SA_ROWS;
  sa_stage<BF16>(logits, row0 * A, here * A, A, P, t, sa_lds);
  __syncthreads();
  const int tid = (int)threadIdx.x;
  if (tid < here) {
    const long long i = row0 + tid;
    float* z = sa_lds + tid * P;
    const float l = lse[i], dlp = d_logprob ? d_logprob[i] : 0.f, dH = d_entropy ? d_entropy[i] : 0.f;
    const int act = actions[i];
    float H = 0.f;   // - sum p logp
    for (int a = 0; a < A; a++) {
      const float lp = z[a] - l, p = expf(lp);
      if (p > 0.f) H = fmaf(-p, lp, H);
    }
    for (int a = 0; a < A; a++) z[a] = sa_grad(z[a], l, H, a == act, t, dlp, dH);
  }
  __syncthreads();
  // the span, flat again
  const long long e0 = row0 * A;
  const int n_el = here * A;
  constexpr int V = D_BF16 ? 8 : 4;
  const bool vec = (((uintptr_t)d_logits) & 15) == 0;
  const int nv = vec ? n_el / V : 0;
  for (int v = tid; v < nv; v += MGX_SA_ROWS) {
    float x[V];
    int r = (V * v) / A, c = V * v - r * A;
#pragma unroll
    for (int j = 0; j < V; j++) {
      x[j] = sa_lds[r * P + c];
      if (++c == A) { c = 0; r++; }
    }
    if (!D_BF16) {
      *(float4*)((float*)d_logits + e0 + (long long)V * v) = make_float4(x[0], x[1], x[2], x[3]);
    } else {
      uint32_t w[4];
#pragma unroll
      for (int j = 0; j < 4; j++) w[j] = sa_bf16(x[2 * j]) | sa_bf16(x[2 * j + 1]) << 16;
      *(uint4*)((uint16_t*)d_logits + e0 + (long long)V * v) = make_uint4(w[0], w[1], w[2], w[3]);
    }
  }
  for (int e = nv * V + tid; e < n_el; e += MGX_SA_ROWS) {
    const int r = e / A, c = e - r * A;
    const float g = sa_lds[r * P + c];
    if (!D_BF16) ((float*)d_logits)[e0 + e] = g;
    else ((uint16_t*)d_logits)[e0 + e] = (uint16_t)sa_bf16(g);
  }
}

// ---- wave per row -------------------------------------------------------------------------------------------------------

__device__ static inline float sa_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// inclusive prefix sum over the 64 lanes
__device__ static inline float sa_wave_scan(float v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float u = __shfl_up(v, o, 64);
    if (lane >= o) v = __fadd_rn(v, u);
  }
  return v;
}

struct SaWaveStats {
  float m, S, T;
  int amax;
  bool bad;
};

// the wavefront's walk over row `z` (element a at z_base + a); every lane returns the same values.  S is the last value of
// the running sum sa_wave_find walks again.
template <int BF16>
__device__ static inline SaWaveStats sa_wave_stats(const void* __restrict__ logits, long long z_base, int A, float t, int lane) {
  SaWaveStats s;
  float m = -INFINITY;
  int am = 0x7FFFFFFF;
  bool bad = false;
  for (int a = lane; a < A; a += 64) {
    const float v = __fmul_rn(t, sa_elem<BF16>(logits, z_base + a));
    bad |= sa_is_bad(v);
    if (v > m) { m = v; am = a; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, 64);
    const int oa = __shfl_xor(am, o, 64);
    if (om > m || (om == m && oa < am)) { m = om; am = oa; }
  }
  s.m = m; s.amax = am;
  s.bad = __any(bad ? 1 : 0) || m == -INFINITY;
  s.S = 0.f; s.T = 0.f;
  if (s.bad) return s;   // (the same in every lane)
  float carry = 0.f, tsum = 0.f;
  for (int base = 0; base < A; base += 64) {
    const int a = base + lane;
    float p = 0.f;
    if (a < A) {
      const float d = __fmul_rn(t, sa_elem<BF16>(logits, z_base + a)) - m;
      p = expf(d);
      if (p > 0.f) tsum = fmaf(p, d, tsum);
    }
    const float c = __fadd_rn(carry, sa_wave_scan(p, lane));
    carry = __shfl(c, 63, 64);
  }
  s.S = carry;
  s.T = sa_wave_sum(tsum);
  return s;
}

// the first a with pt_a > 0 and c_a > thr, else the last a with pt_a > 0; the sums of sa_wave_stats, bit for bit
template <int BF16>
__device__ static inline int sa_wave_find(const void* __restrict__ logits, long long z_base, int A, float t, float m, float thr, int lane) {
  float carry = 0.f;
  int last = 0;
  for (int base = 0; base < A; base += 64) {
    const int a = base + lane;
    float p = 0.f;
    if (a < A) p = expf(__fmul_rn(t, sa_elem<BF16>(logits, z_base + a)) - m);
    const float c = __fadd_rn(carry, sa_wave_scan(p, lane));
    carry = __shfl(c, 63, 64);
    const unsigned long long pos = __ballot(p > 0.f ? 1 : 0), hit = __ballot((p > 0.f && c > thr) ? 1 : 0);
    if (hit) return base + (__ffsll((long long)hit) - 1);
    if (pos) last = base + 63 - __clzll((long long)pos);
  }
  return last;
}

template <int BF16>
__global__ void __launch_bounds__(64 * MGX_SA_WAVES)
mgx_sample_wave_kernel(const void* __restrict__ logits, long long N, int A, long long stride, const long long* __restrict__ rows, float t,
                       int greedy, unsigned long long seed, unsigned long long step, int* __restrict__ actions, float* __restrict__ logprob,
                       float* __restrict__ entropy, unsigned int* __restrict__ bad_rows) {
  const int lane = (int)threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * MGX_SA_WAVES + ((int)threadIdx.x >> 6);
  bool bad = false;
  if (i < N) {   // (the same in every lane of a wavefront)
    const long long r = rows ? rows[i] : i, zb = i * stride;
    const SaWaveStats s = sa_wave_stats<BF16>(logits, zb, A, t, lane);
    bad = s.bad;
    int act = 0;
    float lp = NAN, ent = NAN;
    if (!bad) {
      float zd = 0.f;
      if (greedy) {
        act = s.amax;
      } else {
        const float thr = __fmul_rn(sa_uniform(seed, step, (unsigned long long)r), s.S);
        act = sa_wave_find<BF16>(logits, zb, A, t, s.m, thr, lane);
        zd = __fmul_rn(t, sa_elem<BF16>(logits, zb + act)) - s.m;
      }
      const float ls = logf(s.S);
      lp = zd - ls;
      ent = ls - s.T / s.S;
    }
    if (lane == 0) {
      actions[r] = act;
      if (logprob) logprob[r] = lp;
      if (entropy) entropy[r] = ent;
    }
  }
  sa_count_bad(bad && lane == 0, bad_rows);
}

template <int BF16>
__global__ void __launch_bounds__(64 * MGX_SA_WAVES)
mgx_logprob_wave_kernel(const void* __restrict__ logits, long long N, int A, long long stride, const int* __restrict__ actions, float t,
                        float* __restrict__ logprob, float* __restrict__ entropy, float* __restrict__ lse, unsigned int* __restrict__ bad_rows) {
  const int lane = (int)threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * MGX_SA_WAVES + ((int)threadIdx.x >> 6);
  bool bad = false;
  if (i < N) {
    const long long zb = i * stride;
    const int act = actions[i];
    const bool in_range = act >= 0 && act < A;
    const SaWaveStats s = sa_wave_stats<BF16>(logits, zb, A, t, lane);
    bad = s.bad || !in_range;
    float lp = NAN, ent = NAN, l = NAN;
    if (!bad) {
      const float ls = logf(s.S);
      lp = (__fmul_rn(t, sa_elem<BF16>(logits, zb + act)) - s.m) - ls;
      ent = ls - s.T / s.S;
      l = s.m + ls;
    }
    if (lane == 0) {
      logprob[i] = lp;
      if (entropy) entropy[i] = ent;
      if (lse) lse[i] = l;
    }
  }
  sa_count_bad(bad && lane == 0, bad_rows);
}

template <int BF16, int D_BF16>
__global__ void __launch_bounds__(64 * MGX_SA_WAVES)
mgx_logprob_bwd_wave_kernel(const void* __restrict__ logits, long long N, int A, long long stride, const int* __restrict__ actions, float t,
                            const float* __restrict__ lse, const float* __restrict__ d_logprob, const float* __restrict__ d_entropy,
                            void* __restrict__ d_logits, long long d_stride) {
  const int lane = (int)threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * MGX_SA_WAVES + ((int)threadIdx.x >> 6);
  if (i >= N) return;   // (no barrier in this kernel)
  const long long zb = i * stride, db = i * d_stride;
  const float l = lse[i], dlp = d_logprob ? d_logprob[i] : 0.f, dH = d_entropy ? d_entropy[i] : 0.f;
  const int act = actions[i];
  float h = 0.f;
  for (int a = lane; a < A; a += 64) {
    const float lp = __fmul_rn(t, sa_elem<BF16>(logits, zb + a)) - l, p = expf(lp);
    if (p > 0.f) h = fmaf(-p, lp, h);
  }
  const float H = sa_wave_sum(h);
  for (int a = lane; a < A; a += 64) {
    const float g = sa_grad(__fmul_rn(t, sa_elem<BF16>(logits, zb + a)), l, H, a == act, t, dlp, dH);
    if (!D_BF16) ((float*)d_logits)[db + a] = g;
    else ((uint16_t*)d_logits)[db + a] = (uint16_t)sa_bf16(g);
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------

static bool sa_dtype_ok(int32_t d) { return d == MGX_SA_F32 || d == MGX_SA_BF16; }
static bool sa_aligned(const void* p, int32_t dtype) { return (((uintptr_t)p) & (dtype == MGX_SA_F32 ? 3 : 1)) == 0; }
static bool sa_shape_ok(int32_t dtype, int64_t n_rows, int32_t n_actions, int64_t row_stride, float t) {
  // (NaN fails t > 0)
  return sa_dtype_ok(dtype) && n_rows >= 0 && n_rows <= MGX_SA_MAX_ROWS && n_actions >= 1 && n_actions <= MGX_SA_MAX_A &&
         row_stride >= n_actions && row_stride <= ((int64_t)1 << 32) && t > 0.f && t <= 3.4028235e38f;
}
static bool sa_lane_path(int32_t n_actions, int64_t row_stride) { return n_actions <= MGX_SA_LANE_MAX_A && row_stride == n_actions; }
static size_t sa_lane_lds(int32_t n_actions) { return (size_t)MGX_SA_ROWS * (n_actions | 1) * sizeof(float); }
static unsigned sa_lane_grid(int64_t n) { return (unsigned)((n + MGX_SA_ROWS - 1) / MGX_SA_ROWS); }
static unsigned sa_wave_grid(int64_t n) { return (unsigned)((n + MGX_SA_WAVES - 1) / MGX_SA_WAVES); }

extern "C" {

int mgx_sample_actions(const void* logits, int32_t dtype, int64_t n_rows, int32_t n_actions, int64_t row_stride, const int64_t* rows,
                       float inv_temperature, int32_t mode, uint64_t seed, uint64_t step, int32_t* actions, float* logprob, float* entropy,
                       uint32_t* bad_rows, void* hip_stream) {
  if (!sa_shape_ok(dtype, n_rows, n_actions, row_stride, inv_temperature) || (mode != 0 && mode != 1)) return MGX_ERR_BAD_ARG;
  if (!logits || !actions || !sa_aligned(logits, dtype) || (((uintptr_t)rows) & 7) ||
      (((uintptr_t)actions | (uintptr_t)logprob | (uintptr_t)entropy | (uintptr_t)bad_rows) & 3))
    return MGX_ERR_BAD_ARG;
  if (n_rows == 0) return MGX_OK;
  hipStream_t st = (hipStream_t)hip_stream;
  const long long N = n_rows;
  const int A = n_actions;
  const float t = inv_temperature;
  const bool bf = dtype == MGX_SA_BF16;
  if (sa_lane_path(n_actions, row_stride)) {
    const dim3 grid(sa_lane_grid(n_rows)), block(MGX_SA_ROWS);
    const size_t lds = sa_lane_lds(n_actions);
    if (bf) hipLaunchKernelGGL(mgx_sample_lane_kernel<1>, grid, block, lds, st, logits, N, A, (const long long*)rows, t, (int)mode,
                               (unsigned long long)seed, (unsigned long long)step, (int*)actions, logprob, entropy, (unsigned int*)bad_rows);
    else hipLaunchKernelGGL(mgx_sample_lane_kernel<0>, grid, block, lds, st, logits, N, A, (const long long*)rows, t, (int)mode,
                            (unsigned long long)seed, (unsigned long long)step, (int*)actions, logprob, entropy, (unsigned int*)bad_rows);
  } else {
    const dim3 grid(sa_wave_grid(n_rows)), block(64 * MGX_SA_WAVES);
    if (bf) hipLaunchKernelGGL(mgx_sample_wave_kernel<1>, grid, block, 0, st, logits, N, A, (long long)row_stride, (const long long*)rows, t,
                               (int)mode, (unsigned long long)seed, (unsigned long long)step, (int*)actions, logprob, entropy,
                               (unsigned int*)bad_rows);
    else hipLaunchKernelGGL(mgx_sample_wave_kernel<0>, grid, block, 0, st, logits, N, A, (long long)row_stride, (const long long*)rows, t,
                            (int)mode, (unsigned long long)seed, (unsigned long long)step, (int*)actions, logprob, entropy,
                            (unsigned int*)bad_rows);
  }
  return hipGetLastError() == hipSuccess ? MGX_OK : MGX_ERR_HIP;
}

int mgx_action_logprob(const void* logits, int32_t dtype, int64_t n_rows, int32_t n_actions, int64_t row_stride, const int32_t* actions,
                       float inv_temperature, float* logprob, float* entropy, float* lse, uint32_t* bad_rows, void* hip_stream) {
  if (!sa_shape_ok(dtype, n_rows, n_actions, row_stride, inv_temperature)) return MGX_ERR_BAD_ARG;
  if (!logits || !actions || !logprob || !sa_aligned(logits, dtype) ||
      (((uintptr_t)actions | (uintptr_t)logprob | (uintptr_t)entropy | (uintptr_t)lse | (uintptr_t)bad_rows) & 3))
    return MGX_ERR_BAD_ARG;
  if (n_rows == 0) return MGX_OK;
  hipStream_t st = (hipStream_t)hip_stream;
  const long long N = n_rows;
  const int A = n_actions;
  const float t = inv_temperature;
  const bool bf = dtype == MGX_SA_BF16;
  if (sa_lane_path(n_actions, row_stride)) {
    const dim3 grid(sa_lane_grid(n_rows)), block(MGX_SA_ROWS);
    const size_t lds = sa_lane_lds(n_actions);
    if (bf) hipLaunchKernelGGL(mgx_logprob_lane_kernel<1>, grid, block, lds, st, logits, N, A, (const int*)actions, t, logprob, entropy, lse,
                               (unsigned int*)bad_rows);
    else hipLaunchKernelGGL(mgx_logprob_lane_kernel<0>, grid, block, lds, st, logits, N, A, (const int*)actions, t, logprob, entropy, lse,
                            (unsigned int*)bad_rows);
  } else {
    const dim3 grid(sa_wave_grid(n_rows)), block(64 * MGX_SA_WAVES);
    if (bf) hipLaunchKernelGGL(mgx_logprob_wave_kernel<1>, grid, block, 0, st, logits, N, A, (long long)row_stride, (const int*)actions, t,
                               logprob, entropy, lse, (unsigned int*)bad_rows);
    else hipLaunchKernelGGL(mgx_logprob_wave_kernel<0>, grid, block, 0, st, logits, N, A, (long long)row_stride, (const int*)actions, t,
                            logprob, entropy, lse, (unsigned int*)bad_rows);
  }
  return hipGetLastError() == hipSuccess ? MGX_OK : MGX_ERR_HIP;
}

int mgx_action_logprob_backward(const void* logits, int32_t dtype, int64_t n_rows, int32_t n_actions, int64_t row_stride,
                                const int32_t* actions, float inv_temperature, const float* lse, const float* d_logprob,
                                const float* d_entropy, void* d_logits, int32_t d_dtype, int64_t d_row_stride, void* hip_stream) {
  if (!sa_shape_ok(dtype, n_rows, n_actions, row_stride, inv_temperature) || !sa_dtype_ok(d_dtype) || d_row_stride < n_actions ||
      d_row_stride > ((int64_t)1 << 32))
    return MGX_ERR_BAD_ARG;
  if (!logits || !actions || !lse || !d_logits || !sa_aligned(logits, dtype) || !sa_aligned(d_logits, d_dtype) ||
      (((uintptr_t)actions | (uintptr_t)lse | (uintptr_t)d_logprob | (uintptr_t)d_entropy) & 3))
    return MGX_ERR_BAD_ARG;
  if (n_rows == 0) return MGX_OK;
  hipStream_t st = (hipStream_t)hip_stream;
  const long long N = n_rows;
  const int A = n_actions;
  const float t = inv_temperature;
  const int variant = (dtype == MGX_SA_BF16 ? 2 : 0) | (d_dtype == MGX_SA_BF16 ? 1 : 0);
  if (sa_lane_path(n_actions, row_stride) && d_row_stride == n_actions) {
    const dim3 grid(sa_lane_grid(n_rows)), block(MGX_SA_ROWS);
    const size_t lds = sa_lane_lds(n_actions);
#define SA_BWD(B, D)                                                                                                                      \
  hipLaunchKernelGGL((mgx_logprob_bwd_lane_kernel<B, D>), grid, block, lds, st, logits, N, A, (const int*)actions, t, lse, d_logprob, d_entropy, \
                     d_logits)
    if (variant == 0) SA_BWD(0, 0);
    else if (variant == 1) SA_BWD(0, 1);
    else if (variant == 2) SA_BWD(1, 0);
    else SA_BWD(1, 1);
#undef SA_BWD
  } else {
    const dim3 grid(sa_wave_grid(n_rows)), block(64 * MGX_SA_WAVES);
#define SA_BWD(B, D)                                                                                                                      \
  hipLaunchKernelGGL((mgx_logprob_bwd_wave_kernel<B, D>), grid, block, 0, st, logits, N, A, (long long)row_stride, (const int*)actions, t, lse, \
                     d_logprob, d_entropy, d_logits, (long long)d_row_stride)
    if (variant == 0) SA_BWD(0, 0);
    else if (variant == 1) SA_BWD(0, 1);
    else if (variant == 2) SA_BWD(1, 0);
    else SA_BWD(1, 1);
#undef SA_BWD
  }
  return hipGetLastError() == hipSuccess ? MGX_OK : MGX_ERR_HIP;
}

}  // extern "C"
