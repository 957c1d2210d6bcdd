// mgx_world_fast.hip — the lean world-update kernels (games without rung-4 features: no dynamic tags, queries,
// events, AoE, territory, run-time object creation).  Own translation unit: MgxDev in constant memory (one copy per
// MGX_SLOT), the register handler VM, and MGX_BIG=__forceinline__ — one flat kernel, no calls but mgx_logf.
#define MGX_BIG __forceinline__  // safe here: the lean variant's handler VM is iterative (MgxEnvT::run_handler)
#define MGX_OUTLINE __forceinline__
#define MGX_WORLD_FAST_TU 1
#ifndef MGX_SLOT
#define MGX_SLOT 0  // which constant-memory copy of MgxDev this object file owns (mgx_device.h MGX_CONST_DEV)
#endif
#define MGX_CAT2(a, b) a##b
#define MGX_CAT(a, b) MGX_CAT2(a, b)
#define MGX_TU_NS MGX_CAT(mgx_tu_fast, MGX_SLOT)
#define MGX_CONST_DEV 1
#define MGX_WORLD_IDS 1
#ifndef MGX_NO_WORLD_HELPERS
#define MGX_WORLD_HELPERS 1   // idle upper half-wavefronts take half of the batched per-agent passes (mgx_world.h)
#endif
#ifndef MGX_NO_GEN_HANDLERS
#define MGX_GEN_HANDLERS MgxGenR3   // straight-line handler code of the preset (mgx_handlers_gen.h), used when MgxDev::gen_prog says so
#define MGX_GEN_ID 3
#endif
// Measured on MI355X (rung 3, 65 536 envs): 32 envs per wavefront, two wavefronts per SIMD is the best split —
// 64 lanes serialise more distinct handler paths per wavefront, 16 or 8 multiply the instruction stream.
#ifndef MGX_WORLD_LPW
#define MGX_WORLD_LPW 32
#endif
#ifndef MGX_WORLD_WPE
#define MGX_WORLD_WPE 2
#endif
#include <hip/hip_runtime.h>

#include "mgx_device.h"
#include "mgx_world.h"
#include "mgx_host.h"
#include "mgx_presets_gen.h"   // MgxWorldShapeR3: the preset's shape (mettagrid_amd/gen_presets.py, written at build())

#ifdef MGX_WORLD_WPE
#define MGX_WPE_ATTR __attribute__((amdgpu_waves_per_eu(MGX_WORLD_WPE, MGX_WORLD_WPE)))
#else
#define MGX_WPE_ATTR
#endif
#ifdef MGX_CPU_EMU
#undef MGX_WPE_ATTR
#define MGX_WPE_ATTR
#endif
namespace MGX_TU_NS {
template <bool PROG_LDS>
__global__ void __launch_bounds__(MGX_WORLD_THREADS) MGX_WPE_ATTR mgx_world_kernel_fast(int prog_words) {
  mgx_world_entry<PROG_LDS, false>(g_mgx_dev, prog_words);
}
// The instance compiled for ONE shape (MgxWorldShape, mgx_world.h): every scalar of the table is a constant.  Only the form
// with the program copy in LDS is built — the one the preset launches; each instance takes minutes to compile.  Not in the
// sanitizer build (its planner never chooses it) nor in a unit without the preset's generated handlers.
#if defined(MGX_GEN_HANDLERS) && !defined(MGX_CPU_EMU)
#define MGX_WORLD_PRESET_INSTANCE 1
#endif
#ifdef MGX_WORLD_PRESET_INSTANCE
template <class K>
__global__ void __launch_bounds__(MGX_WORLD_THREADS) MGX_WPE_ATTR mgx_world_kernel_fast_shape(int prog_words) {
  mgx_world_entry<true, false, K>(g_mgx_dev, prog_words);
}
#endif
}  // namespace

static MgxLdsLimit g_lds_limit;
bool MGX_CAT(mgx_world_fast_set_lds_s, MGX_SLOT)(size_t lds) {
  return g_lds_limit.raise_current({(const void*)mgx_world_kernel_fast<true>, (const void*)mgx_world_kernel_fast<false>,
#ifdef MGX_WORLD_PRESET_INSTANCE
                                    (const void*)mgx_world_kernel_fast_shape<MgxWorldShapeR3>,
#endif
                                   }, lds);
}

#if MGX_SLOT == 0
size_t mgx_world_fast_lds_bytes(int A) { return (size_t)mgx_world_lds_fixed(A, false); }
#endif

static MgxConstDev g_const_dev;   // keeps this slot's g_mgx_dev equal to the launching engine's MgxDev
// variant: MgxPlan::world_variant — 3 asks for the preset's instance; the table is compared with its shape once more here, field
// by field (it may have changed since mgx_create: mgx_attach_code), and anything else runs the generic kernels.
void MGX_CAT(mgx_launch_world_fast_s, MGX_SLOT)(bool prog_lds, int variant, size_t lds, hipStream_t stream, const MgxDev& d, int prog_words) {
  const auto lock = g_const_dev.upload(&g_mgx_dev, d, stream, __func__);
  dim3 grid((d.E + MGX_WORLD_EPG - 1) / MGX_WORLD_EPG), block(MGX_WORLD_THREADS);
#ifdef MGX_WORLD_PRESET_INSTANCE
  if (variant == 3 && prog_lds && mgx_world_shape_matches<MgxWorldShapeR3>(d))
    hipLaunchKernelGGL((mgx_world_kernel_fast_shape<MgxWorldShapeR3>), grid, block, lds, stream, prog_words);
  else
#endif
  if (prog_lds) hipLaunchKernelGGL((mgx_world_kernel_fast<true>), grid, block, lds, stream, prog_words);
  else hipLaunchKernelGGL((mgx_world_kernel_fast<false>), grid, block, lds, stream, prog_words);
}

#if defined(MGX_WORLD_TIMING) && MGX_SLOT == 0  // instrumented developer build only (scripts/world_timing.py); not part of the ABI
extern "C" int mgx_debug_world_cycles(unsigned long long* out, int reset) { return mgx_read_cycles(&mgx_dbg_cycles, out, reset); }
// ... and the primary stream's split (mgx_dbg_run, mgx_world.h): out[16]
extern "C" int mgx_debug_world_run_cycles(unsigned long long* out, int reset) { return mgx_read_cycles(&mgx_dbg_run, out, reset, 16); }
#endif
