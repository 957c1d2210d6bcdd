// mgx_render.hip — the render unit: launchers of the cell-word kernel behind mgx_render_cells and of the RGB
// frame kernel behind mgx_render_rgb.  The kernels and what they compute: mgx_render.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mgx.h"
#include "mgx_host.h"
#define MGX_RENDER_KERNELS
#include "mgx_render.h"

// -1: the launch does not fit a grid, -2: the runtime refused
int mgx_launch_render_cells(hipStream_t stream, const MgxDev* dev_copy, const int32_t* envs_dev, int n, int H, int W, uint32_t* out_dev) {
  const long long blocks = (long long)n * (((long long)H * W + 255) / 256);
  if (blocks < 1 || blocks > 0x7FFFFFFFll) return -1;
  hipLaunchKernelGGL(mgx_render_cells_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, dev_copy, envs_dev, n, out_dev);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

static MgxLdsLimit g_lds_limit;
int mgx_launch_render_rgb(hipStream_t stream, const MgxDev* dev_copy, const MgxRenderAtlas& atlas, const int32_t* envs_dev, int n, int H, int W,
                          uint8_t* frames_dev) {
  const int band_rows = mgx_render_band_rows(H, W, atlas.s);
  const long long blocks = (long long)n * ((H + band_rows - 1) / band_rows);
  if (blocks < 1 || blocks > 0x7FFFFFFFll) return -1;
  const size_t lds = (size_t)band_rows * (size_t)W * 4;
  if (!g_lds_limit.raise_current({(const void*)mgx_render_rgb_kernel}, lds)) return -2;
  hipLaunchKernelGGL(mgx_render_rgb_kernel, dim3((unsigned)blocks), dim3(256), lds, stream, dev_copy, atlas, envs_dev, n, band_rows, frames_dev);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
