// mgx_render.h — looking at envs: the cell words a text frame is made of and RGB frames of watched envs, on the device.
//
// The reference renders one env on the host (envs/mettagrid_puffer_env.py:505-524: grid_objects() -> miniscope MapBuffer).
// Here the state is on the device already (grid u16 [E][H*W] -> slot -> obj_cls / obj_agent / obj_vibe), so a frame of any
// listed env is one pass over its cells:
//
//   cell word   u32   0 = empty, else (class + 1) | agent_id << 16 | vibe << 24   (agent_id 0xFF: not an agent)
//
//   mgx_render_cells_kernel   one thread per cell of a listed env: the gather, one coalesced dword store.  The host turns the
//                             words into text (mettagrid_amd/render.py::ansi).
//   mgx_render_rgb_kernel     frames u8 [n][H*s][W*s][3] from a tile atlas (MgxRenderAtlas): store-bound.  One workgroup owns
//                             a BAND of cell rows of one listed env.  It gathers the band's cells once, resolves each to
//                             (tile, vibe marker) and keeps that in LDS (one dword per cell).  The band's pixel rows are one
//                             contiguous byte range of the frame; the workgroup writes it with 16-byte stores per lane between
//                             the first and the last 16-byte boundary, dwords and bytes in front of and behind them.  A pixel
//                             row is W*s*3 bytes, in general no multiple of 4, and the frames may start anywhere: nothing is
//                             assumed about either, and no byte outside the range is touched.  A lane builds its 16 bytes from
//                             a cursor (cell row, pixel row, cell column, pixel, channel) found once by division and then
//                             advanced; the four bytes of a dword that lie in one cell's tile row come from ONE unaligned
//                             dword load of the atlas (global memory: small, read-mostly, cached), the others bytewise.
//
// Both kernels only READ engine state; every output byte has one writer: no atomics, no scratch.
#ifndef MGX_RENDER_H_
#define MGX_RENDER_H_

#include "mgx_device.h"

#define MGX_RENDER_MAX_TILE_PX 32
#define MGX_RENDER_MAX_BAND_ROWS 16   // cell rows per workgroup: at most 16 * 255 dwords of LDS

struct MgxRenderAtlas {          // device pointers into one engine-owned block
  const uint8_t* tiles;          // [n_tiles][s][s][3]
  const uint16_t* class_tile;    // [n_classes]
  const uint16_t* agent_tile;    // [A]
  const uint8_t* vibe_rgb;       // [n_vibes][3] or nullptr: no marker
  int n_tiles, s, n_vibes, n_classes;
};

// Cell rows per workgroup of the RGB kernel: about 32 KB of output each, so that small maps still give several workgroups
// per env and a 255-wide map at s = 8 (48 KB per cell row) takes one row.
inline int mgx_render_band_rows(int H, int W, int s) {
  const long long per_row = (long long)s * s * W * 3;
  long long rows = (32768 + per_row - 1) / per_row;
  if (rows > MGX_RENDER_MAX_BAND_ROWS) rows = MGX_RENDER_MAX_BAND_ROWS;
  if (rows > H) rows = H;
  return rows < 1 ? 1 : (int)rows;
}

#ifdef MGX_RENDER_KERNELS   // the device code: the render unit only (mgx_engine.hip takes the atlas struct and the band rule)
// The word of cell idx of env `env`.  A grid word past the env's slots or a slot without a class — never in a sound env —
// counts as empty: nothing is read outside the env's rows.
__device__ __forceinline__ uint32_t mgx_render_cell_word(const MgxDev& d, int env, int idx) {
  const uint32_t v = d.grid[(size_t)env * (size_t)(d.H * d.W) + idx];
  if (v == 0 || v > (uint32_t)d.S) return 0u;
  const size_t so = (size_t)env * d.S + (v - 1);
  const uint32_t cls = d.obj_cls[so];
  if (cls == MGX_DEAD_CLASS) return 0u;
  return (cls + 1u) | (uint32_t)d.obj_agent[so] << 16 | (uint32_t)d.obj_vibe[so] << 24;
}

// out u32 [n][H*W] (device scratch).  Grid: n * ceil(H*W / 256) workgroups.
__global__ void __launch_bounds__(256) mgx_render_cells_kernel(const MgxDev* __restrict__ dp, const int32_t* __restrict__ envs, int n,
                                                               uint32_t* __restrict__ out) {
  const MgxDev& d = *dp;
  const int HW = d.H * d.W, chunks = (HW + 255) / 256;
  const int k = (int)(blockIdx.x / (unsigned)chunks), idx = (int)(blockIdx.x % (unsigned)chunks) * 256 + (int)threadIdx.x;
  if (k >= n || idx >= HW) return;
  out[(size_t)k * HW + idx] = mgx_render_cell_word(d, envs[k], idx);
}

// Where the next output byte of a band comes from: cell row of the band, pixel row of the cell, cell column, pixel of the
// cell, channel.
struct MgxRgbCursor {
  int cr, py, col, px, ch;
};
struct MgxRgbBand {               // what every byte of a band is looked up in
  const uint32_t* cells;          // LDS: [rows][W] tile | vibe << 16 (vibe 0: no marker on this cell)
  const uint8_t* tiles;
  const uint8_t* vibe_rgb;
  int W, s, q;                    // q = s / 3: the marker is the q x q pixels of the cell's top right corner
  unsigned row_bytes;             // W * s * 3
};
__device__ __forceinline__ void mgx_rgb_seek(const MgxRgbBand& b, unsigned off, MgxRgbCursor& c) {
  const unsigned pr = off / b.row_bytes, xb = off - pr * b.row_bytes;
  c.cr = (int)(pr / (unsigned)b.s);
  c.py = (int)pr - c.cr * b.s;
  const unsigned x = xb / 3u;
  c.ch = (int)(xb - 3u * x);
  c.col = (int)(x / (unsigned)b.s);
  c.px = (int)x - c.col * b.s;
}
__device__ __forceinline__ void mgx_rgb_next_cell(const MgxRgbBand& b, MgxRgbCursor& c) {
  c.px = 0; c.ch = 0;
  if (++c.col == b.W) {
    c.col = 0;
    if (++c.py == b.s) { c.py = 0; c.cr++; }
  }
}
__device__ __forceinline__ uint32_t mgx_rgb_byte(const MgxRgbBand& b, MgxRgbCursor& c) {
  const uint32_t cell = b.cells[c.cr * b.W + c.col], t = cell & 0xFFFFu, vibe = cell >> 16;
  const uint32_t v = (vibe != 0 && c.py < b.q && c.px >= b.s - b.q) ? b.vibe_rgb[vibe * 3u + (uint32_t)c.ch]
                                                                    : b.tiles[(((int)t * b.s + c.py) * b.s + c.px) * 3 + c.ch];
  if (++c.ch == 3) {
    c.ch = 0;
    if (++c.px == b.s) mgx_rgb_next_cell(b, c);
  }
  return v;
}
__device__ __forceinline__ uint32_t mgx_rgb_dword(const MgxRgbBand& b, MgxRgbCursor& c) {
  const uint32_t cell = b.cells[c.cr * b.W + c.col], t = cell & 0xFFFFu, vibe = cell >> 16;
  int lin = c.px * 3 + c.ch;
  if (lin + 4 <= b.s * 3 && !(vibe != 0 && c.py < b.q)) {   // four bytes of one tile row, no marker on this pixel row
    uint32_t v;
    __builtin_memcpy(&v, b.tiles + (((int)t * b.s + c.py) * b.s) * 3 + lin, 4);   // (one unaligned load, inside the atlas)
    lin += 4;
    if (lin == b.s * 3) {
      mgx_rgb_next_cell(b, c);
    } else {
      c.px = lin / 3;
      c.ch = lin - 3 * c.px;
    }
    return v;
  }
  uint32_t v = mgx_rgb_byte(b, c);
  v |= mgx_rgb_byte(b, c) << 8;
  v |= mgx_rgb_byte(b, c) << 16;
  v |= mgx_rgb_byte(b, c) << 24;
  return v;
}

// frames u8 [n][H*s][W*s][3], any alignment.  Grid: n * ceil(H / band_rows) workgroups; dynamic LDS: band_rows * W dwords.
__global__ void __launch_bounds__(256) mgx_render_rgb_kernel(const MgxDev* __restrict__ dp, const MgxRenderAtlas a,
                                                             const int32_t* __restrict__ envs, int n, int band_rows,
                                                             uint8_t* __restrict__ frames) {
  extern __shared__ __align__(16) uint32_t rgb_cells[];
  const MgxDev& d = *dp;
  const int H = d.H, W = d.W, s = a.s, tid = (int)threadIdx.x;
  const int bands = (H + band_rows - 1) / band_rows;
  const int k = (int)(blockIdx.x / (unsigned)bands), y0 = (int)(blockIdx.x % (unsigned)bands) * band_rows;
  if (k >= n) return;                               // (workgroup-uniform)
  const int rows = min(band_rows, H - y0), env = envs[k];
  // ---- the band's cells: gathered once, resolved to (tile, marker) ----
  const bool marker = a.vibe_rgb != nullptr && s >= 3;
  for (int i = tid; i < rows * W; i += 256) {
    const uint32_t w = mgx_render_cell_word(d, env, y0 * W + i);
    uint32_t t = 0, vibe = 0;
    if (w != 0) {
      const uint32_t cls = (w & 0xFFFFu) - 1u, agent = (w >> 16) & 0xFFu;
      // (an agent id past the table — never in a sound env — is drawn by its class: nothing is read outside the tables)
      t = agent != MGX_NO_AGENT && agent < (uint32_t)d.A ? a.agent_tile[agent] : cls < (uint32_t)a.n_classes ? a.class_tile[cls] : 0u;
      vibe = w >> 24;
      if (!marker || vibe >= (uint32_t)a.n_vibes) vibe = 0;
    }
    rgb_cells[i] = t | vibe << 16;
  }
  __syncthreads();
  // ---- the band's bytes: [dst, dst + len) ----
  MgxRgbBand b;
  b.cells = rgb_cells; b.tiles = a.tiles; b.vibe_rgb = a.vibe_rgb; b.W = W; b.s = s; b.q = s / 3;
  b.row_bytes = (unsigned)(W * s * 3);
  const size_t frame_bytes = (size_t)H * (size_t)s * b.row_bytes;
  uint8_t* dst = frames + (size_t)k * frame_bytes + (size_t)y0 * (size_t)s * b.row_bytes;
  const unsigned len = (unsigned)(rows * s) * b.row_bytes;   // (at most 16 * 32 * 255 * 32 * 3: 32 bits)
  const unsigned head_b = min(len, (unsigned)(-(uintptr_t)dst & 3u));                           // bytes up to a dword boundary
  const unsigned head_d = min((len - head_b) / 4u, (unsigned)(-(uintptr_t)(dst + head_b) & 15u) / 4u);   // dwords up to a 16-byte one
  const unsigned body = head_b + 4u * head_d, n16 = (len - body) / 16u;
  const unsigned tail = body + 16u * n16, tail_d = (len - tail) / 4u, tail_b = tail + 4u * tail_d;
  MgxRgbCursor c;
  for (unsigned j = (unsigned)tid; j < n16; j += 256u) {
    mgx_rgb_seek(b, body + 16u * j, c);
    uint4 v;
    v.x = mgx_rgb_dword(b, c); v.y = mgx_rgb_dword(b, c); v.z = mgx_rgb_dword(b, c); v.w = mgx_rgb_dword(b, c);
    *(uint4*)(dst + body + 16u * j) = v;
  }
  // (the few bytes in front of and behind the body, by the last wavefront: it has the fewest body trips)
  const unsigned r = 255u - (unsigned)tid;
  if (r < head_b) { mgx_rgb_seek(b, r, c); dst[r] = (uint8_t)mgx_rgb_byte(b, c); }
  if (r < head_d) { mgx_rgb_seek(b, head_b + 4u * r, c); *(uint32_t*)(dst + head_b + 4u * r) = mgx_rgb_dword(b, c); }
  if (r < tail_d) { mgx_rgb_seek(b, tail + 4u * r, c); *(uint32_t*)(dst + tail + 4u * r) = mgx_rgb_dword(b, c); }
  if (r < len - tail_b) { mgx_rgb_seek(b, tail_b + r, c); dst[tail_b + r] = (uint8_t)mgx_rgb_byte(b, c); }
}
#endif  // MGX_RENDER_KERNELS

#endif  // MGX_RENDER_H_
