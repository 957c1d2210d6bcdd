// mgx_host.h — what the host code of the kernel units shares: the dynamic-LDS limit rule, the cached image of a
// device-side MgxDev, the cycle-counter reader of the instrumented builds and the prototypes of the units' launchers.
// Host code only; included by the units, mgx_plan.h and mgx_engine.hip.
#ifndef MGX_HOST_H_
#define MGX_HOST_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <mutex>
#include <vector>

#include "mgx_device.h"

inline int mgx_pow2_at_least(int n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}

// The dynamic-LDS limit of a set of kernels that are launched with the same size (hipFuncAttributeMaxDynamicSharedMemorySize;
// past 64 KB a launch needs it).  The attribute belongs to the kernel and the device, not to an engine, so every engine
// of the process shares it: one maximum per device, only ever raised, never lowered under a live engine that needs more.
struct MgxLdsLimit {
  std::mutex mu;
  size_t max_bytes[64] = {};   // by device ordinal
  // `device` is the CURRENT device's ordinal (the attribute call goes to the current device).  hipErrorInvalidDevice: an
  // ordinal outside the table; any other error is the runtime's, and the maximum stays as it was.
  hipError_t raise(const void* const* kernels, size_t n, int device, size_t bytes) {
    if (device < 0 || device >= 64) return hipErrorInvalidDevice;
    std::lock_guard<std::mutex> lock(mu);
    if (bytes <= max_bytes[device]) return hipSuccess;
    for (size_t i = 0; i < n; i++) {
      const hipError_t err = hipFuncSetAttribute(kernels[i], hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
      if (err != hipSuccess) return err;
    }
    max_bytes[device] = bytes;
    return hipSuccess;
  }
  hipError_t raise(std::initializer_list<const void*> kernels, int device, size_t bytes) {
    return raise(kernels.begin(), kernels.size(), device, bytes);
  }
  // ... on the current device, as the units' *_set_lds functions are called (mgx_create has selected the engine's)
  bool raise_current(std::initializer_list<const void*> kernels, size_t bytes) {
    int device = 0;
    return hipGetDevice(&device) == hipSuccess && raise(kernels, device, bytes) == hipSuccess;
  }
};

// Host image of an MgxDev that lives on the device (a copy in device memory, or a constant-memory symbol): what was
// uploaded last, so that the next launch uploads only a table that differs.
struct MgxDevImage {
  MgxDev host{};
  bool valid = false;
  // Does the device copy differ from `d` (or hold nothing yet)?  If so `d` is remembered as its new content: the caller uploads it.
  bool differs(const MgxDev& d) {
    if (valid && memcmp(&host, &d, sizeof(MgxDev)) == 0) return false;
    memcpy(&host, &d, sizeof(MgxDev));
    valid = true;
    return true;
  }
};

// The constant-memory MgxDev of a lean unit (MGX_CONST_DEV; one object per unit and slot, the symbol exists once per
// device).  upload() keeps the symbol equal to the launching engine's table and returns the lock under which the caller
// launches.  A change of content first waits for the kernels that still read the old content (another engine on the
// same slot, or re-bound buffers).
struct MgxConstDev {
  std::mutex mu;
  MgxDevImage image[16];   // by device ordinal
  bool thrash_warned = false;
  std::unique_lock<std::mutex> upload(const void* symbol, const MgxDev& d, hipStream_t stream, const char* who) {
    std::unique_lock<std::mutex> lock(mu);
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) dev = 0;
    const bool held = image[dev].valid;
    if (image[dev].differs(d)) {
      if (held) {
        (void)hipDeviceSynchronize();
        if (!thrash_warned && getenv("MGX_VERBOSE")) {   // two engines alternating on one slot pay a device-wide wait per step
          fprintf(stderr, "[mgx] %s: the constant-memory engine table of device %d changed (another engine on the same slot, or re-bound "
                          "buffers): device synchronised before the upload\n", who, dev);
          thrash_warned = true;
        }
      }
      (void)hipMemcpyToSymbolAsync(symbol, &d, sizeof(MgxDev), 0, hipMemcpyHostToDevice, stream);
    }
    return lock;
  }
};

#ifdef MGX_WORLD_TIMING  // instrumented developer builds only (scripts/*_timing.py): a unit's mgx_dbg_cycles, optionally cleared
inline int mgx_read_cycles(const void* symbol, unsigned long long* out, int reset, int n = 16) {   // n <= 16 counters
  (void)hipDeviceSynchronize();
  (void)hipMemcpyFromSymbol(out, symbol, sizeof(unsigned long long) * n);
  if (reset) { unsigned long long z[16] = {0}; (void)hipMemcpyToSymbol(symbol, z, sizeof(unsigned long long) * n); }
  return 0;
}
#endif

// ---- the units' launchers ----
// lean world kernels (mgx_world_fast.hip): one copy per constant-memory slot, the unit is compiled with MGX_SLOT = 0 and 1
#define MGX_FAST_SLOTS 2
size_t mgx_world_fast_lds_bytes(int A);   // dynamic LDS of the unit's kernels without the program copy
void mgx_launch_world_fast_s0(bool prog_lds, int variant, size_t lds, hipStream_t stream, const MgxDev& d, int prog_words);
void mgx_launch_world_fast_s1(bool prog_lds, int variant, size_t lds, hipStream_t stream, const MgxDev& d, int prog_words);
bool mgx_world_fast_set_lds_s0(size_t lds);  // raises the kernels' dynamic LDS limit (MgxLdsLimit)
bool mgx_world_fast_set_lds_s1(size_t lds);
// the lane-per-agent action kernels (mgx_act_fast.hip, mgx_act_x.hip; mgx_act.h)
size_t mgx_act_fast_lds_bytes(int A, int extra);
int mgx_act_fast_epg();   // envs per workgroup of the unit
void mgx_launch_act_fast_s0(bool prog_lds, size_t lds, hipStream_t stream, const MgxDev& d, int prog_words);
bool mgx_act_fast_set_lds_s0(size_t lds);
void mgx_launch_act_x(bool prog_lds, size_t lds, hipStream_t stream, const MgxDev& d, const MgxDev* dev_copy, int prog_words);
bool mgx_act_x_set_lds(size_t lds);
size_t mgx_act_x_lds_bytes(int A, bool aoe_lds, int extra);
int mgx_act_x_epg();
// the extended world kernel (mgx_world_x.hip)
void mgx_launch_world_x(bool prog_lds, size_t lds, hipStream_t stream, const MgxDev& d, const MgxDev* dev_copy, int prog_words, int phases);
bool mgx_world_x_set_lds(size_t lds);
size_t mgx_world_x_lds_bytes(int A, bool aoe_lds);
size_t mgx_world_x_private_bytes();
void mgx_launch_values(hipStream_t stream, const MgxDev& d, const MgxDev* dev_copy, int phase, const uint8_t* env_mask);
// lane-per-agent area effects (mgx_aoe.hip) and the host analysis that allows them
// (dev_copy: absolute section offsets, for the source-record kernel; hot_copy + prog_words: the copy whose hot sections are
// relative to the kernel's LDS program copy, or nullptr / 0 when the program stays in HBM / L2)
void mgx_launch_aoe(hipStream_t stream, const MgxDev& d, const MgxDev* dev_copy, const MgxDev* hot_copy, int prog_words);
bool mgx_aoe_is_target_local(const int32_t* program);
bool mgx_aoe_on_tick_local(const int32_t* program);  // + every per-agent on_tick handler is a leaf that only touches its own agent
bool mgx_aoe_set_lds(int nstat, int prog_words);
void mgx_aoe_collect_stats(const int32_t* program, bool with_on_tick, bool with_coverage, std::vector<int16_t>& out);
// token decode kernel (mgx_decode.hip)
int mgx_launch_decode(hipStream_t stream, const uint8_t* tokens, float* box, const float* scale_dev, long long rows, int T, int C, int H, int W);
// token-bag kernel (mgx_token_bag.hip): -1 = T / C do not fit the LDS, -2 = the runtime refused
int mgx_launch_token_bag(hipStream_t stream, const uint8_t* tokens, void* bag, int bf16, int32_t* counts, const float* scale_dev, long long rows,
                         int T, int C);
// render kernels (mgx_render.hip; mgx_render.h): -1 = the launch does not fit a grid, -2 = the runtime refused
struct MgxRenderAtlas;
int mgx_launch_render_cells(hipStream_t stream, const MgxDev* dev_copy, const int32_t* envs_dev, int n, int H, int W, uint32_t* out_dev);
int mgx_launch_render_rgb(hipStream_t stream, const MgxDev* dev_copy, const MgxRenderAtlas& atlas, const int32_t* envs_dev, int n, int H, int W,
                          uint8_t* frames_dev);

#endif  // MGX_HOST_H_
