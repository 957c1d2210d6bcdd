// mgx_obs_instances.h — the compiled instances of the observation kernel (mgx_obs.h) as table rows: what the host looks an
// engine's instance up in (mgx_engine.hip launch_obs) and walks to raise the kernels' dynamic LDS limit (raise_obs_lds).
// The token-row rows are in mgx_engine.hip, the dense-output rows in mgx_obs_box.hip.
#pragma once
#include "mgx_obs.h"

struct MgxObsInstance { bool box, x, pl; int threads, ew, variant; const void* fn[2]; };   // fn[with_rewards]

// One row from the template arguments of the instance, so that a row cannot be keyed differently from what it instantiates.
// variant: the MgxPlan::obs_variant the row serves — 0 for the generic shape, else the preset shape's (3: the episode length
// is part of the shape, 5: any length).
#define MGX_OBS_INSTANCE(X, PL, NTH, EW, K, BOX)                                                                      \
  {BOX, X, PL, NTH, EW, !K::fixed ? 0 : K::MAX_STEPS < 0 ? 5 : 3,                                                     \
   {(const void*)mgx_obs_kernel<false, X, PL, NTH, EW, K, BOX>, (const void*)mgx_obs_kernel<true, X, PL, NTH, EW, K, BOX>}}

const MgxObsInstance* mgx_obs_box_instances(int* n);   // mgx_obs_box.hip
