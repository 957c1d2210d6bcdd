// mgx_obs_box.hip — the dense-output instances of the observation kernel (fused form): mgx_obs_kernel<...,
// BOX = true> writes the policy's [C][H][W] box of every agent straight from its LDS staging row instead of the token rows
// (mgx_obs.h).  Own translation unit so that the token-path build does not wait for these instantiations; all it exports is
// the table of them, which mgx_engine.hip looks up, launches and raises the LDS limit of like its own token-row table.
#define MGX_WORLD_FAST_TU 1   // (no construction / restart kernels in this unit)
#define MGX_TU_NS mgx_tu_box
#include <hip/hip_runtime.h>

#include "mgx_device.h"
#include "mgx_obs_instances.h"

// The generic instance the token path would launch for the same engine: lean with / without the program block in LDS,
// extended with 256 threads or 512 threads and 4 / 3 / 2 encode wavefronts.
const MgxObsInstance* mgx_obs_box_instances(int* n) {
  static const MgxObsInstance rows[] = {
      MGX_OBS_INSTANCE(false, true, MGX_OBS_THREADS, MGX_OBS_THREADS / MGX_WAVE, MgxObsShapeDyn, true),
      MGX_OBS_INSTANCE(false, false, MGX_OBS_THREADS, MGX_OBS_THREADS / MGX_WAVE, MgxObsShapeDyn, true),
      MGX_OBS_INSTANCE(true, false, 512, 4, MgxObsShapeDyn, true),
      MGX_OBS_INSTANCE(true, false, 512, 3, MgxObsShapeDyn, true),
      MGX_OBS_INSTANCE(true, false, 512, 2, MgxObsShapeDyn, true),
      MGX_OBS_INSTANCE(true, false, MGX_OBS_THREADS, MGX_OBS_THREADS / MGX_WAVE, MgxObsShapeDyn, true),
  };
  *n = (int)(sizeof rows / sizeof *rows);
  return rows;
}
