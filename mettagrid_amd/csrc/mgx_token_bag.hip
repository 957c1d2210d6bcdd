// mgx_token_bag.hip — token-bag features of the observation rows: what a token policy's front end needs of
// a row, in one pass.  The reference's token baseline (python/src/mettagrid/policy/token_encoder.py:88-114) sums, per row,
// s_t * (Px[x_t] + Py[y_t] + F[f_t]) over the row's tokens, s_t = value_t / (scale[f_t] + 1e-6); that sum is
// bag[row] @ concat(Px[:16], Py[:16], F[:C]) with bag[row] = the per-x-nibble, per-y-nibble and per-feature sums of s_t.
// The bag holds no learned parameter, so it is computed here, once, and everything behind it is a GEMM.
//
// u8 [rows][T][3] (coord, feature, value) -> bag [rows][32 + C] (f32, or bf16 = the f32 sum rounded to nearest even on
// store) and counts int32 [rows].  A token counts when coord != 0xFF and feature < C; coord 0xFE is x = 14, y = 15 as in
// the reference net (NOT the centre cell of the box decode).  Every column of every row is written by every launch.
//
// One wavefront per row, four rows per workgroup, like mgx_decode.hip: the row's tokens are staged in LDS, the sums are
// made in per-wavefront f32 bins in LDS with plain LDS float adds (ds_add_f32: lanes that share a bin are serialised by
// the LDS, no global atomics) and the finished row leaves with coalesced stores.  Private copies of the two 16-bin
// marginals and pre-summing runs of equal coords across lanes were measured and lost to the plain adds.
// A bin that a single token targets holds that token's term bit for bit (0 + s == s).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mgx.h"
#include "mgx_host.h"

#define MGX_BAG_WAVES 4
#define MGX_BAG_WAVE 64

// LDS of one wavefront, in dwords (each part a multiple of 4: the next part stays 16-byte aligned): the padded token row,
// the bins (32 + C), the divisors scale[f] + 1e-6 (C)
__host__ __device__ static inline int bag_tok_pad(int T) { return (((3 * T + 3) / 4) + 3) & ~3; }
__host__ __device__ static inline int bag_bins_pad(int C) { return (32 + C + 3) & ~3; }
__host__ __device__ static inline int bag_den_pad(int C) { return (C + 3) & ~3; }

__device__ static inline uint32_t bag_bf16(float x) {   // round to nearest even; the sums are finite and non-negative
  const uint32_t u = __float_as_uint(x);
  return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}

template <int BF16>
__global__ void __launch_bounds__(MGX_BAG_WAVES* MGX_BAG_WAVE) mgx_token_bag_kernel(const uint8_t* __restrict__ tokens, void* __restrict__ bag,
                                                                                    int32_t* __restrict__ counts, const float* __restrict__ scale,
                                                                                    long long rows, int T, int C) {
  extern __shared__ __align__(16) uint8_t bag_lds[];
  const int wave = (int)threadIdx.x / MGX_BAG_WAVE, lane = (int)threadIdx.x & (MGX_BAG_WAVE - 1);
  const long long row = (long long)blockIdx.x * MGX_BAG_WAVES + wave;
  if (row >= rows) return;   // (the whole wavefront: nothing below synchronises across wavefronts)
  const int NB = 32 + C, nb_pad = bag_bins_pad(C);
  const int tok_words = (3 * T + 3) / 4, tok_pad = bag_tok_pad(T);
  uint8_t* stok = bag_lds + (size_t)wave * 4 * (size_t)(tok_pad + nb_pad + bag_den_pad(C));
  float* bins = (float*)(stok + (size_t)tok_pad * 4);
  float* den = bins + nb_pad;
  // ---- stage the token row, clear the bins, fill the divisors ----
  const uint8_t* src = tokens + row * (long long)T * 3;
  if ((((uintptr_t)src) & 3) == 0) {
    const uint32_t* s32 = (const uint32_t*)src;
    for (int i = lane; i < tok_words; i += MGX_BAG_WAVE) {
      // the last word of a row whose 3T is not a multiple of 4 reaches into the next row (or past the buffer for the
      // last row): read it bytewise
      if (i * 4 + 4 <= 3 * T) ((uint32_t*)stok)[i] = s32[i];
      else for (int b = i * 4; b < 3 * T; b++) stok[b] = src[b];
    }
  } else {
    for (int b = lane; b < 3 * T; b += MGX_BAG_WAVE) stok[b] = src[b];
  }
  for (int i = lane; i < nb_pad; i += MGX_BAG_WAVE) bins[i] = 0.f;
  for (int i = lane; i < C; i += MGX_BAG_WAVE) den[i] = __fadd_rn(scale[i], 1e-6f);   // (no dependent gather per token)
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // one wavefront per row: LDS operations complete in issue order
  // ---- one token per lane and pass: its term into its x bin, its y bin and its feature bin ----
  int count = 0;
  for (int base = 0; base < T; base += MGX_BAG_WAVE) {   // (wavefront-uniform trip count: the ballot sees every lane)
    const int t = base + lane;
    bool valid = false;
    if (t < T) {
      const uint32_t coord = stok[3 * t], fid = stok[3 * t + 1];
      valid = coord != 0xFFu && (int)fid < C;
      if (valid) {
        const float s = __fdiv_rn((float)stok[3 * t + 2], den[fid]);   // the reference's f32 term
        atomicAdd(&bins[coord & 15u], s);
        atomicAdd(&bins[16u + (coord >> 4)], s);
        atomicAdd(&bins[32u + fid], s);
      }
    }
    count += (int)__popcll(__ballot(valid));
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  // ---- the finished row: coalesced stores, 16 bytes per lane when the row stride and the pointer allow it ----
  if (lane == 0) counts[row] = count;
  if (!BF16) {
    float* dst = (float*)bag + row * (long long)NB;
    if ((NB & 3) == 0 && (((uintptr_t)dst) & 15) == 0) {
      for (int i = lane; i < NB / 4; i += MGX_BAG_WAVE) ((uint4*)dst)[i] = ((const uint4*)bins)[i];
    } else {
      for (int i = lane; i < NB; i += MGX_BAG_WAVE) dst[i] = bins[i];
    }
  } else {
    uint16_t* dst = (uint16_t*)bag + row * (long long)NB;
    if ((NB & 7) == 0 && (((uintptr_t)dst) & 15) == 0) {
      for (int i = lane; i < NB / 8; i += MGX_BAG_WAVE) {
        const float4 a = ((const float4*)bins)[2 * i], b = ((const float4*)bins)[2 * i + 1];
        ((uint4*)dst)[i] = make_uint4(bag_bf16(a.x) | bag_bf16(a.y) << 16, bag_bf16(a.z) | bag_bf16(a.w) << 16,
                                      bag_bf16(b.x) | bag_bf16(b.y) << 16, bag_bf16(b.z) | bag_bf16(b.w) << 16);
      }
    } else if ((NB & 1) == 0 && (((uintptr_t)dst) & 3) == 0) {
      for (int i = lane; i < NB / 2; i += MGX_BAG_WAVE) ((uint32_t*)dst)[i] = bag_bf16(bins[2 * i]) | bag_bf16(bins[2 * i + 1]) << 16;
    } else {
      for (int i = lane; i < NB; i += MGX_BAG_WAVE) dst[i] = (uint16_t)bag_bf16(bins[i]);
    }
  }
}

size_t mgx_token_bag_lds_bytes(int T, int C) {
  return (size_t)MGX_BAG_WAVES * 4 * (size_t)(bag_tok_pad(T) + bag_bins_pad(C) + bag_den_pad(C));
}

static MgxLdsLimit g_lds_limit;
int mgx_launch_token_bag(hipStream_t stream, const uint8_t* tokens, void* bag, int bf16, int32_t* counts, const float* scale_dev, long long rows,
                         int T, int C) {
  const size_t lds = mgx_token_bag_lds_bytes(T, C);
  if (lds > 160 * 1024) return -1;
  if (!g_lds_limit.raise_current({(const void*)mgx_token_bag_kernel<0>, (const void*)mgx_token_bag_kernel<1>}, lds)) return -2;
  const long long blocks = (rows + MGX_BAG_WAVES - 1) / MGX_BAG_WAVES;
  if (bf16)
    hipLaunchKernelGGL(mgx_token_bag_kernel<1>, dim3((unsigned)blocks), dim3(MGX_BAG_WAVES * MGX_BAG_WAVE), lds, stream, tokens, bag, counts,
                       scale_dev, rows, T, C);
  else
    hipLaunchKernelGGL(mgx_token_bag_kernel<0>, dim3((unsigned)blocks), dim3(MGX_BAG_WAVES * MGX_BAG_WAVE), lds, stream, tokens, bag, counts,
                       scale_dev, rows, T, C);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
