// mgx_byte_linear.hip — the first Linear of a dense policy, read straight from the u8 observation rows (DESIGN.md §7l;
// include/mgx.h mgx_byte_linear_forward / mgx_byte_linear_wgrad).  The reference's trainable baselines flatten a row and
// feed `observations.view(B, -1).float() / 255.0` to Linear(3T, hidden) (python/src/mettagrid/policy/stateless.py:29,42,
// lstm.py:31-37,73-84, puffer_default.py:57,65).  Every u8 value is exact in bfloat16, so the row itself is a matrix-core
// operand: no float copy of the observations is made and the input is never rounded.
//
//   y[n][h]  = fl( fl( s * sum_k x[n][k] * W[h][k] ) + b[h] )        x u8 [N][K], W bf16 [H][K] (one or two terms), f32 sums
//   dW[h][k] = s * sum_n dy[n][h] * x[n][k]
//
// Both kernels use v_mfma_f32_16x16x32_bf16: H comes in multiples of 16 (a 32-wide tile would idle on H = 16, 144), the
// kernels are bound by their bytes, not by the matrix cores, and four accumulator registers per tile keep a wavefront's
// block of tiles small enough for two wavefronts per SIMD.  Operand maps (lane l, l15 = l & 15, g = l >> 4):
// A[row l15][k = 8 g + j], B[k = 8 g + j][col l15], j = 0..7; D[row 4 g + r][col l15], r = 0..3.
//
// Forward.  A = W (rows = h), B = x^T (cols = n): both fragments are 8 CONSECUTIVE k of one row of their matrix, a plain
// 16-byte (W) or 8-byte (x) LDS read, and a lane's four results are four consecutive h of one row n: one 16-byte (f32) or
// 8-byte (bf16) store.  A workgroup of four wavefronts owns 128 rows x 128 columns; a wavefront 64 rows x 64 columns
// (4 x 4 tiles, 64 accumulator registers).  K runs in steps of 64: the x bytes and the W slice are staged in LDS (zeros
// past K, past row N - 1 and past column H - 1), the bytes are widened to bf16 in registers when a fragment is read.
//
// Weight gradient.  A = dy^T (rows = h), B = x (cols = k), the sum runs over rows n: BOTH operands have n as their slow
// index in memory, so both are transposed while they are staged (x as bytes, [k][64 n]; dy as bf16, [h][64 n], split
// into hi + lo for two terms) and the fragment reads are plain again.  A workgroup reduces one chunk of
// MGX_BL_CHUNK rows for 128 columns h and a slab of at most 16 k-tiles and writes its f32 partial tile to the caller's
// scratch; a second kernel adds the partials of every (h, k) in chunk order and scales.  No atomics: the result of a
// given input is the same bits on every call.
//
// Control flow around the MFMAs is wavefront-uniform (tile counts depend on the wavefront, never on the lane).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mgx.h"
#include "mgx_host.h"

#define MGX_BL_THREADS 256
#define MGX_BL_MT 4        // forward: row tiles per wavefront
#define MGX_BL_BM (32 * MGX_BL_MT)   // forward: rows per workgroup (two wavefronts deep)
#define MGX_BL_BH 128      // columns h per workgroup (both kernels)
#define MGX_BL_KC 64       // forward: k per staging step (two MFMA k-steps)
#define MGX_BL_XP 80       // forward: LDS pitch of an x row (64 bytes + 16: 16 rows x 2 groups of 8 bytes hit 64 distinct banks)
#define MGX_BL_WP 144      // forward: LDS pitch of a W row (64 bf16 + 16 bytes: 16 rows x 16 bytes hit 64 distinct banks)
#define MGX_BL_CHUNK 4096  // weight gradient: rows per partial tile
#define MGX_BL_NC 64       // weight gradient: rows per staging step (two MFMA k-steps)
#define MGX_BL_GXP 68      // weight gradient: LDS pitch of a k row of x^T (64 bytes + 4)
#define MGX_BL_GDP 136     // weight gradient: LDS pitch of an h row of dy^T (64 bf16 + 8 bytes)
#define MGX_BL_SLAB 16     // weight gradient: k-tiles per workgroup at most (four per wavefront)
#define MGX_BL_MAX_H 4096
enum { MGX_BL_F32 = 1, MGX_BL_BF16 = 2 };   // the dtype codes of include/mgx.h (as mgx_token_bag's)

typedef short bl_frag __attribute__((ext_vector_type(8)));   // 8 bf16: one A or B fragment
typedef float bl_acc __attribute__((ext_vector_type(4)));

__device__ static inline uint32_t bl_bf16(float v) {   // round to nearest even (v_cvt_pk_bf16_f32)
  return (uint32_t)__builtin_bit_cast(unsigned short, (__bf16)v);
}
__device__ static inline float bl_bf16_float(uint32_t bits) { return __uint_as_float(bits << 16); }

// 8 bytes -> 8 bf16 (exact)
__device__ static inline bl_frag bl_widen(uint32_t lo, uint32_t hi) {
  bl_frag f;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    f[j] = (short)bl_bf16((float)((lo >> (8 * j)) & 0xFFu));
    f[4 + j] = (short)bl_bf16((float)((hi >> (8 * j)) & 0xFFu));
  }
  return f;
}

// bytes k .. k + 3 of one row of x (`row` points at its first byte), 0 for k' >= K: a dword load where the row is
// 4-aligned and the dword ends inside the row's K bytes, else bytewise — never a byte past the row's K
__device__ static inline uint32_t bl_x_word(const uint8_t* __restrict__ row, int k, int K, bool aligned) {
  if (aligned && k + 4 <= K) return *(const uint32_t*)(row + k);
  uint32_t v = 0;
  for (int b = 0; b < 4; b++)
    if (k + b < K) v |= (uint32_t)row[k + b] << (8 * b);
  return v;
}

template <int TERMS, int BF16>
__global__ void __launch_bounds__(MGX_BL_THREADS, 2)
mgx_byte_linear_fwd_kernel(const uint8_t* __restrict__ x, long long ldx, const uint16_t* __restrict__ w_hi, const uint16_t* __restrict__ w_lo,
                           const float* __restrict__ bias, float scale, void* __restrict__ y, long long ldy, long long N, int K, int H) {
  extern __shared__ __align__(16) uint8_t bl_lds[];
  uint8_t* sx = bl_lds;                                     // [BM][XP]
  uint8_t* sw = bl_lds + MGX_BL_BM * MGX_BL_XP;             // [TERMS][128][WP]
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, g = lane >> 4;
  const long long n0 = (long long)blockIdx.x * MGX_BL_BM;
  const int h0 = (int)blockIdx.y * MGX_BL_BH;
  const int rg = wave >> 1, cg = wave & 1;                  // the wavefront's 16 MT rows and 64 columns
  // valid tiles of this wavefront (wavefront-uniform)
  long long rows_left = N - n0 - rg * (16 * MGX_BL_MT);
  const int mv = rows_left <= 0 ? 0 : rows_left >= 16 * MGX_BL_MT ? MGX_BL_MT : (int)((rows_left + 15) / 16);
  const int cols_left = H - h0 - cg * 64;
  const int nv = cols_left <= 0 ? 0 : cols_left >= 64 ? 4 : cols_left / 16;
  const bool x_aligned = ((((uintptr_t)x) | (uintptr_t)ldx) & 3) == 0;
  const bool w_vec = (K & 7) == 0 && ((((uintptr_t)w_hi) | (TERMS == 2 ? (uintptr_t)w_lo : 0)) & 15) == 0;

  bl_acc acc[MGX_BL_MT][4];
#pragma unroll
  for (int m = 0; m < MGX_BL_MT; m++)
#pragma unroll
    for (int n = 0; n < 4; n++) acc[m][n] = (bl_acc){0.f, 0.f, 0.f, 0.f};

  for (int k0 = 0; k0 < K; k0 += MGX_BL_KC) {
    // ---- stage x: BM rows x 16 dwords, 16 lanes per row ----
    {
      const int cw = tid & 15, r0 = tid >> 4;
      uint32_t v[MGX_BL_BM / 16];
#pragma unroll
      for (int i = 0; i < MGX_BL_BM / 16; i++) {
        const long long n = n0 + i * 16 + r0;
        v[i] = n < N ? bl_x_word(x + n * ldx, k0 + 4 * cw, K, x_aligned) : 0u;
      }
#pragma unroll
      for (int i = 0; i < MGX_BL_BM / 16; i++) *(uint32_t*)(sx + (i * 16 + r0) * MGX_BL_XP + 4 * cw) = v[i];
    }
    // ---- stage W[h0 .. h0+127][k0 .. k0+63], zeros past H and K ----
#pragma unroll
    for (int t = 0; t < TERMS; t++) {
      const uint16_t* __restrict__ w = t ? w_lo : w_hi;
      uint8_t* dst = sw + t * (MGX_BL_BH * MGX_BL_WP);
      if (w_vec) {   // 8 bf16 per lane: K % 8 == 0 keeps every vector inside its row
        const int seg = tid & 7, hr = tid >> 3;
        uint4 v[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int h = h0 + hr + 32 * i, k = k0 + 8 * seg;
          v[i] = (h < H && k < K) ? *(const uint4*)(w + (long long)h * K + k) : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 4; i++) *(uint4*)(dst + (hr + 32 * i) * MGX_BL_WP + 16 * seg) = v[i];
      } else {
        const int kk = tid & 63, hr = tid >> 6;
        for (int i = 0; i < 32; i++) {
          const int h = h0 + hr + 4 * i, k = k0 + kk;
          *(uint16_t*)(dst + (hr + 4 * i) * MGX_BL_WP + 2 * kk) = (h < H && k < K) ? w[(long long)h * K + k] : (uint16_t)0;
        }
      }
    }
    __syncthreads();
    // ---- 2 k-steps x (MT x 4 tiles) ----
#pragma unroll 1
    for (int ks = 0; ks < 2; ks++) {
      bl_frag whi[4], wlo[4];
#pragma unroll
      for (int n = 0; n < 4; n++) {
        const int off = (cg * 64 + n * 16 + l15) * MGX_BL_WP + ks * 64 + g * 16;
        whi[n] = *(const bl_frag*)(sw + off);
        if (TERMS == 2) wlo[n] = *(const bl_frag*)(sw + MGX_BL_BH * MGX_BL_WP + off);
      }
#pragma unroll
      for (int m = 0; m < MGX_BL_MT; m++) {
        if (m < mv) {
          const uint2 xb = *(const uint2*)(sx + (rg * (16 * MGX_BL_MT) + m * 16 + l15) * MGX_BL_XP + ks * 32 + g * 8);
          const bl_frag xf = bl_widen(xb.x, xb.y);
#pragma unroll
          for (int n = 0; n < 4; n++) {
            if (n < nv) {
              acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(whi[n], xf, acc[m][n], 0, 0, 0);
              if (TERMS == 2) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wlo[n], xf, acc[m][n], 0, 0, 0);
            }
          }
        }
      }
    }
    __syncthreads();
  }
  // ---- y = fl(fl(s * acc) + b): a lane holds columns h .. h + 3 of row n ----
  const bool y_vec = BF16 ? ((((uintptr_t)y) & 7) == 0 && (ldy & 3) == 0) : ((((uintptr_t)y) & 15) == 0 && (ldy & 3) == 0);
#pragma unroll
  for (int n = 0; n < 4; n++) {
    if (n < nv) {
      const int h = h0 + cg * 64 + n * 16 + 4 * g;
      float b[4] = {0.f, 0.f, 0.f, 0.f};
      if (bias)
        for (int r = 0; r < 4; r++) b[r] = bias[h + r];
#pragma unroll
      for (int m = 0; m < MGX_BL_MT; m++) {
        const long long row = n0 + rg * (16 * MGX_BL_MT) + m * 16 + l15;
        if (m < mv && row < N) {
          float o[4];
#pragma unroll
          for (int r = 0; r < 4; r++) {
            o[r] = __fmul_rn(scale, acc[m][n][r]);
            if (bias) o[r] = __fadd_rn(o[r], b[r]);
          }
          if (!BF16) {
            float* p = (float*)y + row * ldy + h;
            if (y_vec) *(float4*)p = make_float4(o[0], o[1], o[2], o[3]);
            else for (int r = 0; r < 4; r++) p[r] = o[r];
          } else {
            uint16_t* p = (uint16_t*)y + row * ldy + h;
            if (y_vec) *(uint2*)p = make_uint2(bl_bf16(o[0]) | bl_bf16(o[1]) << 16, bl_bf16(o[2]) | bl_bf16(o[3]) << 16);
            else for (int r = 0; r < 4; r++) p[r] = (uint16_t)bl_bf16(o[r]);
          }
        }
      }
    }
  }
}

// four values dy[n][h .. h + 3] as float (h % 4 == 0, h + 3 < H)
template <int DY_BF16>
__device__ static inline void bl_dy4(const void* __restrict__ dy, long long n, int H, int h, bool vec, float* out) {
  if (!DY_BF16) {
    const float* p = (const float*)dy + n * H + h;
    if (vec) { const float4 v = *(const float4*)p; out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w; }
    else for (int i = 0; i < 4; i++) out[i] = p[i];
  } else {
    const uint16_t* p = (const uint16_t*)dy + n * H + h;
    uint32_t a, b;
    if (vec) { const uint2 v = *(const uint2*)p; a = v.x; b = v.y; }
    else { a = p[0] | (uint32_t)p[1] << 16; b = p[2] | (uint32_t)p[3] << 16; }
    out[0] = bl_bf16_float(a & 0xFFFFu); out[1] = bl_bf16_float(a >> 16);
    out[2] = bl_bf16_float(b & 0xFFFFu); out[3] = bl_bf16_float(b >> 16);
  }
}

// TERMS = 2: dy (f32) is split into bf16 hi + lo; TERMS = 1: hi alone (f32 rounded, or the bf16 values themselves)
template <int TERMS, int DY_BF16>
__global__ void __launch_bounds__(MGX_BL_THREADS, 2)
mgx_byte_linear_wgrad_kernel(const uint8_t* __restrict__ x, long long ldx, const void* __restrict__ dy, long long N, int K, int H,
                             int slab_tiles, float* __restrict__ partial) {
  extern __shared__ __align__(16) uint8_t bl_lds[];
  uint8_t* sxt = bl_lds;                                            // [256 k][GXP]: x^T, bytes
  uint8_t* sdt = bl_lds + MGX_BL_SLAB * 16 * MGX_BL_GXP;            // [TERMS][128 h][GDP]: dy^T, bf16
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, g = lane >> 4;
  const long long chunk = blockIdx.x;
  const int k_base = (int)blockIdx.y * slab_tiles * 16;
  const int h0 = (int)blockIdx.z * MGX_BL_BH;
  const long long n_begin = chunk * MGX_BL_CHUNK;
  const long long n_end = n_begin + MGX_BL_CHUNK < N ? n_begin + MGX_BL_CHUNK : N;
  const int hv = H - h0 >= MGX_BL_BH ? 8 : (H - h0) / 16;           // valid h tiles (wavefront-uniform)
  // this wavefront's k-tiles: wave, wave + 4, wave + 8, wave + 12 while inside the slab and inside K
  int kv = 0;
  for (int j = 0; j < 4; j++)
    if (wave + 4 * j < slab_tiles && k_base + (wave + 4 * j) * 16 < K) kv = j + 1;
  const bool x_aligned = ((((uintptr_t)x) | (uintptr_t)ldx) & 3) == 0;
  const bool dy_vec = (((uintptr_t)dy) & (DY_BF16 ? 7 : 15)) == 0;
  const int words = slab_tiles * 4;                                 // dwords of one row's slab (<= 64)

  bl_acc acc[8][4];
#pragma unroll
  for (int m = 0; m < 8; m++)
#pragma unroll
    for (int n = 0; n < 4; n++) acc[m][n] = (bl_acc){0.f, 0.f, 0.f, 0.f};

  for (long long n0 = n_begin; n0 < n_end; n0 += MGX_BL_NC) {
    // ---- stage x^T: four rows' dwords per thread, their bytes transposed in registers, one dword per k row ----
    {
      const int kw = tid & 63, qq = tid >> 6;
      if (kw < words) {
        const int k = k_base + 4 * kw;
#pragma unroll
        for (int it = 0; it < 4; it++) {
          const int q = qq + 4 * it;
          uint32_t d[4];
#pragma unroll
          for (int r = 0; r < 4; r++) {
            const long long n = n0 + 4 * q + r;
            d[r] = (n < n_end && k < K) ? bl_x_word(x + n * ldx, k, K, x_aligned) : 0u;
          }
#pragma unroll
          for (int j = 0; j < 4; j++) {
            const uint32_t t = ((d[0] >> (8 * j)) & 0xFFu) | ((d[1] >> (8 * j)) & 0xFFu) << 8 | ((d[2] >> (8 * j)) & 0xFFu) << 16 |
                               ((d[3] >> (8 * j)) & 0xFFu) << 24;
            *(uint32_t*)(sxt + (4 * kw + j) * MGX_BL_GXP + 4 * q) = t;
          }
        }
      }
    }
    // ---- stage dy^T: two rows x four columns per thread, one dword (rows n, n + 1) per h row and term ----
    {
      const int hq = tid & 31, pp = tid >> 5;
      const int h = h0 + 4 * hq;
#pragma unroll
      for (int it = 0; it < 4; it++) {
        const int p = pp + 8 * it;
        float v[2][4];
#pragma unroll
        for (int r = 0; r < 2; r++) {
          const long long n = n0 + 2 * p + r;
          if (n < n_end && h < H) bl_dy4<DY_BF16>(dy, n, H, h, dy_vec, v[r]);
          else v[r][0] = v[r][1] = v[r][2] = v[r][3] = 0.f;
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const uint32_t a = bl_bf16(v[0][i]), b = bl_bf16(v[1][i]);
          *(uint32_t*)(sdt + (4 * hq + i) * MGX_BL_GDP + 4 * p) = a | b << 16;
          if (TERMS == 2) {
            const uint32_t al = bl_bf16(__fsub_rn(v[0][i], bl_bf16_float(a))), bl = bl_bf16(__fsub_rn(v[1][i], bl_bf16_float(b)));
            *(uint32_t*)(sdt + MGX_BL_BH * MGX_BL_GDP + (4 * hq + i) * MGX_BL_GDP + 4 * p) = al | bl << 16;
          }
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < 2; ks++) {
      bl_frag xf[4];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        if (j < kv) {
          const uint8_t* p = sxt + ((wave + 4 * j) * 16 + l15) * MGX_BL_GXP + ks * 32 + g * 8;
          xf[j] = bl_widen(*(const uint32_t*)p, *(const uint32_t*)(p + 4));
        }
      }
#pragma unroll
      for (int m = 0; m < 8; m++) {
        if (m < hv) {
          const int off = (m * 16 + l15) * MGX_BL_GDP + ks * 64 + g * 16;
          union { uint2 u[2]; bl_frag f; } dhi, dlo;
          dhi.u[0] = *(const uint2*)(sdt + off);
          dhi.u[1] = *(const uint2*)(sdt + off + 8);
          if (TERMS == 2) {
            dlo.u[0] = *(const uint2*)(sdt + MGX_BL_BH * MGX_BL_GDP + off);
            dlo.u[1] = *(const uint2*)(sdt + MGX_BL_BH * MGX_BL_GDP + off + 8);
          }
#pragma unroll
          for (int j = 0; j < 4; j++) {
            if (j < kv) {
              acc[m][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dhi.f, xf[j], acc[m][j], 0, 0, 0);
              if (TERMS == 2) acc[m][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dlo.f, xf[j], acc[m][j], 0, 0, 0);
            }
          }
        }
      }
    }
    __syncthreads();
  }
  // ---- the partial tile: partial[chunk][h][k], a lane holds rows h .. h + 3 of column k ----
  float* out = partial + chunk * (long long)H * K;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    if (j < kv) {
      const int k = k_base + (wave + 4 * j) * 16 + l15;
      if (k < K) {
#pragma unroll
        for (int m = 0; m < 8; m++) {
          if (m < hv) {
#pragma unroll
            for (int r = 0; r < 4; r++) out[(long long)(h0 + m * 16 + 4 * g + r) * K + k] = acc[m][j][r];
          }
        }
      }
    }
  }
}

// dW[i] = s * (partial[0][i] + partial[1][i] + ...), added in chunk order
__global__ void __launch_bounds__(MGX_BL_THREADS, 2)
mgx_byte_linear_wgrad_sum_kernel(const float* __restrict__ partial, long long chunks, long long elems, float scale, float* __restrict__ dw) {
  const long long i = (long long)blockIdx.x * MGX_BL_THREADS + threadIdx.x;
  if (i >= elems) return;
  float s = partial[i];
  for (long long c = 1; c < chunks; c++) s = __fadd_rn(s, partial[c * elems + i]);
  dw[i] = __fmul_rn(scale, s);
}

static size_t bl_fwd_lds(int terms) { return (size_t)MGX_BL_BM * MGX_BL_XP + (size_t)terms * MGX_BL_BH * MGX_BL_WP; }
static size_t bl_wgrad_lds(int terms) { return (size_t)MGX_BL_SLAB * 16 * MGX_BL_GXP + (size_t)terms * MGX_BL_BH * MGX_BL_GDP; }

static MgxLdsLimit g_fwd_lds_limit, g_wgrad_lds_limit;

static bool bl_shape_ok(int64_t n_rows, int32_t k, int32_t h, int64_t x_stride) {
  return n_rows >= 0 && n_rows <= ((int64_t)1 << 38) && k >= 1 && k <= 65535 && h >= 16 && h <= MGX_BL_MAX_H && (h & 15) == 0 && x_stride >= k;
}

extern "C" {

int32_t mgx_byte_linear_chunk_rows(void) { return MGX_BL_CHUNK; }

int64_t mgx_byte_linear_scratch_bytes(int64_t n_rows, int32_t k, int32_t h) {
  if (n_rows <= 0 || k <= 0 || h <= 0) return 0;
  return (n_rows + MGX_BL_CHUNK - 1) / MGX_BL_CHUNK * (int64_t)h * k * 4;
}

int mgx_byte_linear_forward(const uint8_t* x, int64_t n_rows, int32_t k, int64_t x_stride, const void* w_hi, const void* w_lo, int32_t terms,
                            const float* bias, float scale, void* y, int32_t y_dtype, int64_t y_stride, int32_t h, void* hip_stream) {
  if (!bl_shape_ok(n_rows, k, h, x_stride) || (terms != 1 && terms != 2) || (y_dtype != MGX_BL_F32 && y_dtype != MGX_BL_BF16) || y_stride < h)
    return MGX_ERR_BAD_ARG;
  if (!w_hi || (terms == 2 && !w_lo) || (((uintptr_t)w_hi | (uintptr_t)w_lo) & 1)) return MGX_ERR_BAD_ARG;
  if (n_rows == 0) return MGX_OK;
  if (!x || !y || (((uintptr_t)y) & (y_dtype == MGX_BL_F32 ? 3 : 1)) || (((uintptr_t)bias) & 3)) return MGX_ERR_BAD_ARG;
  const size_t lds = bl_fwd_lds(terms);
  if (lds > 160 * 1024) return MGX_ERR_PROGRAM;
  if (!g_fwd_lds_limit.raise_current({(const void*)mgx_byte_linear_fwd_kernel<1, 0>, (const void*)mgx_byte_linear_fwd_kernel<1, 1>,
                                      (const void*)mgx_byte_linear_fwd_kernel<2, 0>, (const void*)mgx_byte_linear_fwd_kernel<2, 1>}, lds))
    return MGX_ERR_HIP;
  hipStream_t st = (hipStream_t)hip_stream;
  const dim3 grid((unsigned)((n_rows + MGX_BL_BM - 1) / MGX_BL_BM), (unsigned)((h + MGX_BL_BH - 1) / MGX_BL_BH));
  const bool bf = y_dtype == MGX_BL_BF16;
#define BL_FWD(T, B)                                                                                                                     \
  hipLaunchKernelGGL((mgx_byte_linear_fwd_kernel<T, B>), grid, dim3(MGX_BL_THREADS), lds, st, x, (long long)x_stride, (const uint16_t*)w_hi, \
                     (const uint16_t*)w_lo, bias, scale, y, (long long)y_stride, (long long)n_rows, (int)k, (int)h)
  if (terms == 1 && !bf) BL_FWD(1, 0);
  else if (terms == 1) BL_FWD(1, 1);
  else if (!bf) BL_FWD(2, 0);
  else BL_FWD(2, 1);
#undef BL_FWD
  return hipGetLastError() == hipSuccess ? MGX_OK : MGX_ERR_HIP;
}

int mgx_byte_linear_wgrad(const uint8_t* x, int64_t n_rows, int32_t k, int64_t x_stride, const void* dy, int32_t dy_dtype, int32_t h,
                          int32_t terms, float scale, float* dw, void* scratch, void* hip_stream) {
  if (!bl_shape_ok(n_rows, k, h, x_stride) || (terms != 1 && terms != 2) || (dy_dtype != MGX_BL_F32 && dy_dtype != MGX_BL_BF16))
    return MGX_ERR_BAD_ARG;
  if (n_rows == 0) return MGX_OK;
  if (!x || !dy || !dw || !scratch || (((uintptr_t)dy) & (dy_dtype == MGX_BL_F32 ? 3 : 1)) || (((uintptr_t)dw | (uintptr_t)scratch) & 3))
    return MGX_ERR_BAD_ARG;
  const int split = terms == 2 && dy_dtype == MGX_BL_F32 ? 2 : 1;
  const size_t lds = bl_wgrad_lds(split);
  if (lds > 160 * 1024) return MGX_ERR_PROGRAM;
  if (!g_wgrad_lds_limit.raise_current({(const void*)mgx_byte_linear_wgrad_kernel<1, 0>, (const void*)mgx_byte_linear_wgrad_kernel<1, 1>,
                                        (const void*)mgx_byte_linear_wgrad_kernel<2, 0>}, lds))
    return MGX_ERR_HIP;
  hipStream_t st = (hipStream_t)hip_stream;
  const long long chunks = (n_rows + MGX_BL_CHUNK - 1) / MGX_BL_CHUNK;
  const int k_tiles = (k + 15) / 16, slabs = (k_tiles + MGX_BL_SLAB - 1) / MGX_BL_SLAB, slab_tiles = (k_tiles + slabs - 1) / slabs;
  const dim3 grid((unsigned)chunks, (unsigned)slabs, (unsigned)((h + MGX_BL_BH - 1) / MGX_BL_BH));
#define BL_WGRAD(T, B)                                                                                                                \
  hipLaunchKernelGGL((mgx_byte_linear_wgrad_kernel<T, B>), grid, dim3(MGX_BL_THREADS), lds, st, x, (long long)x_stride, dy, (long long)n_rows, \
                     (int)k, (int)h, slab_tiles, (float*)scratch)
  if (dy_dtype == MGX_BL_BF16) BL_WGRAD(1, 1);
  else if (split == 2) BL_WGRAD(2, 0);
  else BL_WGRAD(1, 0);
#undef BL_WGRAD
  const long long elems = (long long)h * k;
  hipLaunchKernelGGL(mgx_byte_linear_wgrad_sum_kernel, dim3((unsigned)((elems + MGX_BL_THREADS - 1) / MGX_BL_THREADS)), dim3(MGX_BL_THREADS), 0, st,
                     (const float*)scratch, chunks, elems, scale, dw);
  return hipGetLastError() == hipSuccess ? MGX_OK : MGX_ERR_HIP;
}

}  // extern "C"
