// mgx_engine.hip — host side of libmgx: device state allocation, kernel launches and the C ABI of include/mgx.h.
// gfx950 only.  There is NO CPU fallback in this library: every entry point that computes runs HIP kernels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "mgx.h"
#include "mgx_device.h"
#include "mgx_obs.h"
#include "mgx_obs_instances.h"
#include "mgx_presets_gen.h"   // MgxObsShapeR3 / R4: the benchmark presets' shapes (mettagrid_amd/gen_presets.py, written at build())
#include "mgx_handlers_fp.h"   // fingerprints of the presets' handler tables (mettagrid_amd/gen_handlers.py, written at build())
#include "mgx_world.h"
#include "mgx_host.h"      // what the kernel units' host code shares, and their launchers
#include "mgx_aoe_local.h"
#include "mgx_episode.h"
#include "mgx_plan.h"       // mgx_create's host-only half: validation and every create-time decision
#include "mgx_env_state.h"  // what an env's state is (the one list of its arrays) and the save / load kernel
#include "mgx_replay.h"     // change log of the watched envs (mgx_set_replay)
#include "mgx_mapgen_plan.h"  // the map builders on the device (mgx_mapgen.h) and the host-only half of mgx_set_map_*generator
#include "mgx_step_stats.h" // chosen stats of every env / agent read out behind every step (mgx_set_step_stats)
#include "mgx_time_avg.h"   // time-averaged game stats of every episode (mgx_set_time_averages)
#include "mgx_policy_stats.h"  // per-policy episode statistics (mgx_set_policy_stats)
#include "mgx_pool_sample.h"   // weighted draws of the next pool map, per-map episode statistics (mgx_set_pool_sampling)
#include "mgx_global_state.h"  // every env's objects as one token row, written behind every step (mgx_set_global_state)
#include "mgx_render.h"        // the tile atlas of mgx_render_rgb (the kernels: mgx_render.hip)


// Territory ownership map (TerritoryTracker::compute_cell_ownership, core/territory_tracker.cpp:215-252) of every cell,
// per territory type: one workgroup per env, rebuilt only for envs whose sources moved or changed tags since the last
// build (terr_dirty).  Static sources (flags) make this a once-per-episode cost; the observation kernel's aoe_mask
// token and the per-agent territory effects then read one u16 per cell instead of re-deriving the influence sums.
__global__ void __launch_bounds__(256) mgx_terr_kernel(MgxDev d) {
  MGX_KERNARG_ENTRY(d);
  extern __shared__ __align__(16) uint8_t smem[];
  const int env = blockIdx.x;
  if (!d.terr_dirty[env]) return;
  MgxEnvX e(d, d.P, env);
  e.xl.terr_score = (long long*)smem;
  e.xl.lane = (int)threadIdx.x;
  e.xl.stride = 256;
  const int HW = d.H * d.W;
  for (int ti = 0; ti < d.NT; ti++)
    for (int cellidx = (int)threadIdx.x; cellidx < HW; cellidx += 256) {
      const int owner = e.cell_owner(cellidx / d.W, cellidx % d.W, ti);
      d.terr_owner[((size_t)env * d.NT + ti) * (size_t)HW + cellidx] = owner < 0 ? (uint16_t)0xFFFF : (uint16_t)owner;
    }
  __syncthreads();
  if (threadIdx.x == blockDim.x - 1) d.terr_dirty[env] = 0;
}

// MGX_TRACE=1: name every launch on stderr and wait for it, so that a faulting kernel is the last one named.
static bool g_trace = getenv("MGX_TRACE") != nullptr;
#define MGX_TRACE_POINT(e, what)                                                   \
  do {                                                                             \
    if (g_trace) { (void)hipStreamSynchronize((e)->stream); fprintf(stderr, "[mgx] done: %s\n", what); fflush(stderr); } \
  } while (0)
// Agent::set_inventory (objects/agent.cpp:86-104) for one agent: a single work-item, the same Inventory::update code
// the world kernels use.
__global__ void mgx_set_inventory_kernel(const MgxDev* __restrict__ dp, int env, int agent, const int32_t* items,
                                         const int32_t* amounts, int n) {
  const MgxDev& d = *dp;
  MgxEnvX e(d, d.P, env);
  e.step = d.step[env];
  const int slot = d.ag_obj[e.ao(agent)];
  unsigned long long ord = d.obj_order[e.so(slot)];  // iterate a copy of the current items
  for (int k = 0; k < 16; k++) {
    const int item = (int)((ord >> (4 * k)) & 0xF);
    if (item == 0xF) break;
    e.inv_update<1>(slot, item, -(int)e.inv(slot, item));
    e.astat_set(agent, d.wk[MGX_S_RES_AMOUNT_BASE] + item, 0.f);
  }
  for (int i = 0; i < n; i++) e.inv_update<1>(slot, items[i], amounts[i] - (int)e.inv(slot, items[i]));
}

// ---- batched state digests --------------------------------------------------------------------------
// One 64-bit digest per env over exactly what the episode signature is made of — the mgx_get_objects records, every stat
// value + "key exists" flag, episode rewards, action_success, current_stat_reward, current step — so that the signature of
// all 65 536 envs costs one kernel and one 512 KB copy instead of 65 536 round trips.  FNV-1a over 32-bit words; the
// objects are hashed per slot by the lanes of a wavefront and the slot hashes chained in slot order.
__device__ __forceinline__ unsigned long long mgx_fnv(unsigned long long h, uint32_t w) {
  return (h ^ (unsigned long long)w) * 1099511628211ull;
}
#define MGX_FNV_BASIS 14695981039346656037ull
__global__ void __launch_bounds__(MGX_WAVE) mgx_digest_kernel(const MgxDev* __restrict__ dp, unsigned long long* out) {
  const MgxDev& d = *dp;
  __shared__ unsigned long long slot_hash[MGX_WAVE];
  const int env = blockIdx.x, lane = threadIdx.x;
  MgxEnvX e(d, d.P, env);
  const int n = (int)d.num_objs[env];
  unsigned long long h = MGX_FNV_BASIS;
  h = mgx_fnv(h, d.step[env]);
  h = mgx_fnv(h, (uint32_t)n);
  for (int s0 = 0; s0 < n; s0 += MGX_WAVE) {
    const int s = s0 + lane;
    unsigned long long hs = MGX_FNV_BASIS;
    if (s < n) {   // the 42 words of the slot's mgx_get_objects record
      const size_t o = e.so(s);
      const uint16_t cls = d.obj_cls[o], rc = d.obj_rc[o];
      const uint8_t oflags = d.obj_flags ? d.obj_flags[o] : 0;
      const uint8_t ag = d.obj_agent[o];
      const unsigned long long ord = d.obj_order[o];
      hs = mgx_fnv(hs, (uint32_t)(s + 1)); hs = mgx_fnv(hs, cls); hs = mgx_fnv(hs, rc >> 8); hs = mgx_fnv(hs, rc & 0xFF);
      hs = mgx_fnv(hs, d.obj_vibe[o]); hs = mgx_fnv(hs, (cls != MGX_DEAD_CLASS && !(oflags & 1)) ? 1u : 0u);
      hs = mgx_fnv(hs, ag == MGX_NO_AGENT ? 0xFFFFFFFFu : (uint32_t)ag);
      int cnt = 0;
      uint32_t items[MGX_MAX_RESOURCES];
      bool ended = false;
#pragma unroll
      for (int k = 0; k < MGX_MAX_RESOURCES; k++) {
        const int item = (int)((ord >> (4 * k)) & 0xF);
        ended = ended || item == 0xF;
        items[k] = ended ? 0xFFFFFFFFu : (uint32_t)item;
        cnt += ended ? 0 : 1;
      }
      hs = mgx_fnv(hs, (uint32_t)cnt);
#pragma unroll
      for (int k = 0; k < MGX_MAX_RESOURCES; k++) hs = mgx_fnv(hs, items[k]);
      for (int k = 0; k < MGX_MAX_RESOURCES; k++) hs = mgx_fnv(hs, k < d.R ? (uint32_t)d.obj_inv[o * MGX_INV_PITCH + k] : 0u);
      for (int k = 0; k < MGX_TAG_WORDS; k++)
        hs = mgx_fnv(hs, d.obj_tags ? d.obj_tags[o * MGX_TAG_WORDS + k]
                                     : (cls != MGX_DEAD_CLASS ? (uint32_t)mgx_cls(d, cls)[MGX_C_TAGS + k] : 0u));
    }
    slot_hash[lane] = hs;
    __syncthreads();
    if (lane == 0)
      for (int k = 0; k < MGX_WAVE && s0 + k < n; k++) { h = mgx_fnv(h, (uint32_t)slot_hash[k]); h = mgx_fnv(h, (uint32_t)(slot_hash[k] >> 32)); }
    __syncthreads();
  }
  if (lane != 0) return;
  for (int i = 0; i < d.NG; i++) {   // game stats: value bits + key exists (mgx_get_stats)
    const float v = d.game_stats[(size_t)env * d.NG + i];
    const uint32_t t = ((d.game_touched[(size_t)env * d.NGW + (i >> 5)] >> (i & 31)) & 1u) | (v != 0.f ? 1u : 0u);
    h = mgx_fnv(h, __float_as_uint(v)); h = mgx_fnv(h, t);
  }
  for (int a = 0; a < d.A; a++) {
    for (int i = 0; i < d.NS; i++) {
      const float v = d.ag_stats[e.ao(a) * d.NSP + i];
      const uint32_t t = ((d.ag_touched[e.ao(a) * d.NSW + (i >> 5)] >> (i & 31)) & 1u) | (v != 0.f ? 1u : 0u);
      h = mgx_fnv(h, __float_as_uint(v)); h = mgx_fnv(h, t);
    }
    h = mgx_fnv(h, __float_as_uint(d.episode_rewards[e.ao(a)]));
    h = mgx_fnv(h, (uint32_t)d.success[e.ao(a)]);
    {  // the per-agent mirrors of the object row (MgxDev::ag_rc, ag_cls) against the row itself
      const size_t so = e.so(d.ag_obj[e.ao(a)]);
      if (d.ag_rc[e.ao(a)] != d.obj_rc[so] || d.ag_cls[e.ao(a)] != d.obj_cls[so]) d.err[env] |= MGX_ENV_INTERNAL;
    }
    const uint16_t c = d.obj_cls[e.so(d.ag_obj[e.ao(a)])];   // current_stat_reward (systems/reward.hpp:36-42)
    const int nrw = c == MGX_DEAD_CLASS ? 0 : mgx_cls(d, c)[MGX_C_REWARD_COUNT];
    float tot = 0.f;
    for (int k = 0; k < nrw; k++) tot = __fadd_rn(tot, d.ag_rprev[e.ao(a) * d.NRW + k]);
    h = mgx_fnv(h, __float_as_uint(tot));
    for (int q = 0; q < MGX_INVALID_EXTRA; q++) {   // "action.invalid_index.<k>" keys beyond the stat columns (mgx.h)
      const float nq = d.ag_invn[e.ao(a) * MGX_INVALID_EXTRA + q];
      if (nq != 0.f) { h = mgx_fnv(h, (uint32_t)d.ag_invk[e.ao(a) * MGX_INVALID_EXTRA + q]); h = mgx_fnv(h, __float_as_uint(nq)); }
    }
  }
  out[env] = h;
}

// ---- batched object export (the replay-writer shape of grid_objects(), cpp/bindings/mettagrid_py.cpp:28-139) ----
// One workgroup per LISTED env, one thread per object slot: the slot's mgx_get_objects record (MGX_OBJ_RECORD_WORDS int32,
// layout in include/mgx.h) goes to a packed device buffer [n_envs][S][words] that the host fetches with one copy.
__global__ void __launch_bounds__(256) mgx_objects_kernel(const MgxDev* __restrict__ dp, const int32_t* __restrict__ envs, int32_t* __restrict__ out,
                                                          int32_t* __restrict__ counts) {
  const MgxDev& d = *dp;
  const int env = envs[blockIdx.x];
  MgxEnvX e(d, d.P, env);
  const int n = (int)d.num_objs[env];
  if (threadIdx.x == 0) counts[blockIdx.x] = n;
  for (int s = (int)threadIdx.x; s < n; s += (int)blockDim.x) {
    int32_t* w = out + ((size_t)blockIdx.x * d.S + s) * MGX_OBJ_RECORD_WORDS;
    const size_t o = e.so(s);
    const uint16_t cls = d.obj_cls[o], rc = d.obj_rc[o];
    const uint8_t oflags = d.obj_flags ? d.obj_flags[o] : 0;
    const uint8_t ag = d.obj_agent[o];
    const unsigned long long ord = d.obj_order[o];
    w[0] = s + 1; w[1] = cls; w[2] = rc >> 8; w[3] = rc & 0xFF; w[4] = d.obj_vibe[o];
    w[5] = (cls != MGX_DEAD_CLASS && !(oflags & 1)) ? 1 : 0;
    w[6] = ag == MGX_NO_AGENT ? -1 : (int)ag;
    int cnt = 0;
    bool ended = false;
    for (int k = 0; k < MGX_MAX_RESOURCES; k++) {
      const int item = (int)((ord >> (4 * k)) & 0xF);
      ended = ended || item == 0xF;
      w[8 + k] = ended ? -1 : item;
      cnt += ended ? 0 : 1;
    }
    w[7] = cnt;
    for (int k = 0; k < MGX_MAX_RESOURCES; k++) w[8 + MGX_MAX_RESOURCES + k] = k < d.R ? (int)d.obj_inv[o * MGX_INV_PITCH + k] : 0;
    for (int k = 0; k < MGX_TAG_WORDS; k++)
      w[8 + 2 * MGX_MAX_RESOURCES + k] = d.obj_tags ? (int32_t)d.obj_tags[o * MGX_TAG_WORDS + k]
                                                    : (cls != MGX_DEAD_CLASS ? mgx_cls(d, cls)[MGX_C_TAGS + k] : 0);
  }
}

static thread_local std::string g_err;
static int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t _e = (expr);                                                                        \
    if (_e != hipSuccess)                                                                          \
      return fail(MGX_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));                 \
  } while (0)

// ---- what the statistics reducers share on the host (on the device: csrc/mgx_totals.h) --------------------------
// Totals that live on the device and are read by SNAPSHOT: one kernel launch copies them to d_snap and clears them, an async
// copy brings d_snap to pinned memory, an event says when it has landed.  One snapshot at a time.  Elements are 8 bytes.
struct MgxSnapshot {
  void* d_totals = nullptr;   // [bytes] since the last snapshot
  void* d_snap = nullptr;     // [bytes] the snapshot taken by request()
  void* h_snap = nullptr;     // pinned host copy of the snapshot
  size_t bytes = 0;
  hipEvent_t ev = nullptr;    // recorded behind the snapshot copy
  bool pending = false;       // a snapshot has been requested and not fetched yet

  int create(size_t n_bytes) {
    bytes = n_bytes;
    HIP_TRY(hipMalloc(&d_totals, bytes));
    HIP_TRY(hipMalloc(&d_snap, bytes));
    HIP_TRY(hipHostMalloc(&h_snap, bytes, hipHostMallocDefault));
    HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    return MGX_OK;
  }
  void destroy() {   // (also of a half-created one)
    if (d_totals) (void)hipFree(d_totals);
    if (d_snap) (void)hipFree(d_snap);
    if (h_snap) (void)hipHostFree(h_snap);
    if (ev) (void)hipEventDestroy(ev);
    *this = MgxSnapshot{};
  }
  // launch(): the owner's snapshot kernel, enqueued on `stream`; returns MGX_OK or its failure.
  template <class Launch>
  int request(int device, hipStream_t stream, Launch launch) {
    if (pending) return MGX_OK;   // the snapshot already under way is fetched first; the totals keep accumulating
    HIP_TRY(hipSetDevice(device));
    { int rc = launch(); if (rc) return rc; }
    HIP_TRY(hipMemcpyAsync(h_snap, d_snap, bytes, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipEventRecord(ev, stream));
    pending = true;
    return MGX_OK;
  }
  // *ready (0 on entry) = 1 and `out` filled once the requested snapshot has landed; nothing without a request.
  int fetch(int device, int32_t wait, void* out, int32_t* ready) {
    if (!pending) return MGX_OK;
    HIP_TRY(hipSetDevice(device));
    if (wait) {
      HIP_TRY(hipEventSynchronize(ev));
    } else {
      const hipError_t q = hipEventQuery(ev);
      if (q == hipErrorNotReady) return MGX_OK;
      if (q != hipSuccess) return fail(MGX_ERR_HIP, std::string("hipEventQuery: ") + hipGetErrorString(q));
    }
    memcpy(out, h_snap, bytes);
    pending = false;
    *ready = 1;
    return MGX_OK;
  }
};

// A bounded device log of per-episode records; the total kernel of each step advances d_state (csrc/mgx_totals.h).
struct MgxEpisodeLog {
  uint32_t* d_log = nullptr;     // [cap][words] records kept for the drain, or nullptr (no log)
  uint32_t* d_state = nullptr;   // [2] records in the log, records dropped since the last drain
  int cap = 0, words = 0;

  int create(hipStream_t stream, int log_cap, int log_words) {
    words = log_words;
    HIP_TRY(hipMalloc((void**)&d_state, 8));
    HIP_TRY(hipMemsetAsync(d_state, 0, 8, stream));
    if (log_cap > 0) {
      HIP_TRY(hipMalloc((void**)&d_log, (size_t)log_cap * words * 4));
      cap = log_cap;
    }
    return MGX_OK;
  }
  void destroy() {
    if (d_log) (void)hipFree(d_log);
    if (d_state) (void)hipFree(d_state);
    *this = MgxEpisodeLog{};
  }
  // The log's records -> `records` (room for `cap` of them), the log emptied; waits for the device.
  int drain(int device, hipStream_t stream, uint32_t* records, int32_t* n_records, int32_t* n_dropped) {
    HIP_TRY(hipSetDevice(device));
    uint32_t st[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(st, d_state, 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (st[0]) HIP_TRY(hipMemcpyAsync(records, d_log, (size_t)st[0] * words * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemsetAsync(d_state, 0, 8, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    *n_records = (int32_t)st[0];
    if (n_dropped) *n_dropped = (int32_t)st[1];
    return MGX_OK;
  }
};

// One reducer: the step's records -> chunk sums -> f64 batch totals (read by snapshot) + the log.
struct MgxReducer {
  uint32_t* rec = nullptr;      // [E][rec_words] records of the envs that finished in the last step
  double* partial = nullptr;    // [ceil(E / MGX_EP_CHUNK)][tot_words] chunk sums
  uint32_t* ticket = nullptr;   // [1]
  MgxSnapshot snap;             // [tot_words] doubles
  MgxEpisodeLog log;
  double* totals() const { return (double*)snap.d_totals; }

  // The totals are left as allocated: the owner runs its snapshot kernel once, which leaves them cleared.
  int create(hipStream_t stream, size_t E, int rec_words, int tot_words, int log_cap, int log_words) {
    const size_t nch = (E + MGX_EP_CHUNK - 1) / MGX_EP_CHUNK;
    HIP_TRY(hipMalloc((void**)&rec, E * rec_words * 4));
    HIP_TRY(hipMalloc((void**)&partial, nch * tot_words * 8));
    HIP_TRY(hipMalloc((void**)&ticket, 4));
    HIP_TRY(hipMemsetAsync(ticket, 0, 4, stream));
    { int rc = snap.create((size_t)tot_words * 8); if (rc) return rc; }
    return log.create(stream, log_cap, log_words);
  }
  void destroy() {
    if (rec) (void)hipFree(rec);
    if (partial) (void)hipFree(partial);
    if (ticket) (void)hipFree(ticket);
    snap.destroy();
    log.destroy();
    *this = MgxReducer{};
  }
};

struct mgx_engine : MgxPlan {   // the plan mgx_create made (d, paths, LDS layout) + the resources behind it
  MgxSwitches sw{};            // the create-time switches, for the rest of the engine's life
  MgxDev* d_dev = nullptr;     // copy of `d` in device memory for the kernels that take it by pointer (extended path)
  MgxDevImage d_dev_image;     // what d_dev holds
  MgxDev* d_hot = nullptr;     // the extended world kernel's copy: sec[] of the hot program range relative to its LDS copy
  MgxDevImage d_hot_image;
  int device = 0;
  hipStream_t stream = nullptr;
  std::vector<void*> allocs;
  int64_t state_bytes = 0;
  std::vector<int32_t> prog;
  // internally owned caller-visible buffers (always allocated; bound by default)
  uint8_t *own_obs = nullptr, *own_term = nullptr, *own_trunc = nullptr;
  float* own_rew = nullptr;
  int32_t *own_act = nullptr, *own_vact = nullptr;
  // host-bound buffers (MGX_MEM_HOST)
  int mem_kind = MGX_MEM_DEVICE;
  uint8_t *h_obs = nullptr, *h_term = nullptr, *h_trunc = nullptr;
  float* h_rew = nullptr;
  int32_t *h_act = nullptr, *h_vact = nullptr;
  bool external = false;
  int box_dtype = 0, box_C = 0;   // mgx_set_box_output: the observation kernel writes the dense box instead of token rows
  void* box_out = nullptr;
  bool terr_fresh = false;     // the territory ownership maps were refreshed in this step and nothing behind that can change them
  int slot = 0;                // constant-memory slot of the lean world kernel (mgx_world_fast.hip, MGX_SLOT)
  uint32_t* h_act_err = nullptr;      // pinned + mapped [4]: mgx_set_joint_actions' range check: flags, lowest bad row, its value
  uint32_t* h_act_err_dev = nullptr;
  unsigned long long* d_first_bad = nullptr;   // (row << 32 | value) of the lowest bad row so far, ~0 = none
  int32_t* d_vibe_ids = nullptr;  // mgx_set_joint_actions: action index of each vibe action
  int32_t vibe_ids_host[256] = {};
  int n_vibe_ids = 0;
  uint16_t* dmaps = nullptr;
  uint32_t* dseeds = nullptr;
  uint8_t* dmask = nullptr;
  struct Row { void* base; size_t row_bytes; int fill; };
  std::vector<Row> rows_state;  // per-env state arrays (env-major) that an episode restart clears
  MgxRow* d_rows = nullptr;     // device table: rows_state + the caller-visible terminals / truncations / rewards rows
  int n_rows = 0;
  std::vector<MgxRow> rows_host;
  // device-resident map pool + auto-reset
  uint16_t* d_pool = nullptr;   // [n_pool][H][W]
  int n_pool = 0;
  int32_t* d_map_index = nullptr;   // [E] pool map of each env's current episode
  uint32_t* d_episodes = nullptr;   // [E] episodes started by auto-reset
  uint8_t* d_next_mask = nullptr;   // [E] envs found done at the end of the last step
  uint32_t* d_early = nullptr;      // [E] step at which each env's FIRST episode ends early (desync), or nullptr
  uint32_t* d_counters = nullptr;   // [2] done count, block ticket
  uint32_t* h_flags = nullptr;      // pinned + mapped: [0] sequence number of the last finished step, [1] its done count
  uint32_t* h_flags_dev = nullptr;  // device address of h_flags
  bool auto_reset = false;
  int pool_stride = 1;
  uint32_t step_seq = 0;
  // code objects specialised for this engine's program at run time (mgx_attach_code; mettagrid_amd/jit.py)
  struct Jit {
    hipModule_t mod = nullptr;
    hipFunction_t f0 = nullptr, f1 = nullptr;   // world: the kernel for this engine's prog_in_lds; obs: with / without rewards
    void* dev_sym = nullptr;                     // world: address of the module's g_mgx_dev
    MgxDevImage dev_image;                       // ... and what it holds
    int epg = 0, threads = 0;
  } jit_world, jit_obs, jit_actx;
  int32_t* d_done_list = nullptr;   // [E] the envs of d_next_mask in ascending order (mgx_episode_end_kernel) ...
  uint32_t* d_done_n = nullptr;     // [1] ... and how many: what the restart and episode-statistics kernels walk
  // episode-end statistics (mgx_set_episode_stats; csrc/mgx_episode.h)
  bool ep_stats = false;
  MgxEpLayout ep{};
  MgxReducer ep_red;                // records [E][ep.rec_words], totals [ep_tw()], log records of ep.log_words
  int ep_tw() const { return MGX_EP_TOT_HDR + 2 * (ep.NG + ep.NS); }
  // time-averaged game stats (mgx_set_time_averages; csrc/mgx_time_avg.h): slot-side arrays outside the saved env record
  bool ta_on = false;
  MgxTimeAvg ta{};                  // layout + ta_sum [E][NG], ta_seen [E][NGW], ta_steps [E]
  MgxReducer ta_red;                // records [E][ta.L.rec_words], totals [ta.L.tot_words], log records as the records
  uint8_t* d_ta_block = nullptr;    // staging of mgx_copy_envs / get / put: packed accumulators of a list of envs
  size_t ta_block_bytes = 0;
  // per-policy episode statistics (mgx_set_policy_stats; csrc/mgx_policy_stats.h): the assignment table belongs to the slots
  bool ps_on = false;
  MgxPolicyStats ps{};              // layout + assign u8 [E][A]
  MgxReducer ps_red;                // records [E][ps.L.rec_words], totals [ps.L.tot_words], log records as the records
  uint8_t* d_ps_rows = nullptr;     // [E][A] staging of mgx_set_policy_assignments: the rows of the listed envs
  int32_t* d_ps_list = nullptr;     // [E] ... and the list
  // weighted pool sampling (mgx_set_pool_sampling; csrc/mgx_pool_sample.h): thresholds, seed and offset belong to the slots
  bool smp_on = false;              // (false: the restarts enqueue nothing for it and the rotation rule stands)
  uint32_t smp_seed = 0, smp_offset = 0;
  unsigned long long* d_smp_edges = nullptr;   // [n_pool] thresholds the draw kernel reads
  unsigned long long* h_smp_edges = nullptr;   // pinned [MGX_SMP_RING][n_pool] staging of mgx_set_pool_weights ...
  hipEvent_t smp_ev[4] = {};                   // ... and the event behind each slot's upload: a slot is reused once it has landed
  int smp_slot = 0;
  // per-map episode statistics (mgx_set_map_stats): the table belongs to the slots
  bool ms_on = false;               // (false: nothing is enqueued behind the episode records)
  MgxSnapshot ms_snap;              // the table: uint64 [n_pool + 1][MGX_MS_COLS]
  unsigned long long* d_digest = nullptr;   // [E] mgx_state_digests
  // saved env state (mgx_env_state.h): the record layout, the device segment table, the staging of mgx_copy_envs
  MgxEnvStateLayout es;
  std::vector<MgxSeg> es_segs_host;   // what d_es_segs holds
  MgxSeg* d_es_segs = nullptr;
  uint8_t* d_es_buf = nullptr;        // mgx_copy_envs: records of the sources
  size_t es_buf_bytes = 0;
  std::vector<uint8_t> es_lists;      // host side of the env lists uploaded through d_stage ...
  hipEvent_t es_ev = nullptr;         // ... recorded behind that upload: the vector is reused once it has completed
  bool es_ev_pending = false;
  // replays of watched envs (mgx_set_replay; csrc/mgx_replay.h): slot-owned, never part of an env-state record
  MgxRpl rpl{};                     // device pointers of the watch list, log, cursors, recorder state, shadow, static-class bits
  int rpl_n = 0;                    // watched envs (0: the recorder is off and mgx_step enqueues nothing for it)
  // per-step stat readout (mgx_set_step_stats; csrc/mgx_step_stats.h): the outputs are the caller's, the column table the slot's
  MgxStepStats ss{};                // the kernel's argument: column table (device), the four output tensors
  bool ss_on = false;               // (false: mgx_step enqueues nothing for it)
  int32_t ss_kinds[2 * MGX_SS_MAX_COLUMNS] = {};   // resolved kind of each column, game columns first (mgx_step_stats_columns)
  // global state rows (mgx_set_global_state; csrc/mgx_global_state.h): the rows are the caller's; the previous row lengths, the
  // class filter and the staging of mgx_write_global_state's env mask are the slot's (one device block: used | include | mask)
  MgxGlobalState gs{};              // the kernel's argument
  bool gs_on = false;               // (false: mgx_step enqueues nothing for it)
  uint8_t* d_gs_mask = nullptr;     // [E] inside the block behind gs.used
  // device map generator (mgx_set_map_generator; csrc/mgx_mapgen.h): the recipe and the base seeds belong to the slot, never
  // to a saved env state
  MgxMapRecipe gen{};               // the kind (MGX_GEN_OFF: none) and its kernel's argument: device pointers into d_gen_recipe + the shape
  size_t gen_lds = 0;               // dynamic LDS of the kind's kernel: the inner array (scene: map, indices, symbols)
  void* d_gen_recipe = nullptr;     // inner (scene: symbols) | rename | rename_off
  uint32_t* d_gen_base = nullptr;   // [E] map seed base of each slot
  uint32_t* d_gen_seed = nullptr;   // [E] seed of the map each env's most recent generated restart built
  int32_t* d_objs = nullptr;        // mgx_get_objects_batch: env list | counts | packed records
  size_t objs_cap = 0;              // envs the buffer holds
  // rendering (mgx_render_cells / mgx_set_render_tiles / mgx_render_rgb; csrc/mgx_render.h): slot-owned, in no env record
  MgxRenderAtlas rnd{};             // device pointers into d_rnd_atlas (tiles == nullptr: no atlas)
  void* d_rnd_atlas = nullptr;      // tiles | class_tile | agent_tile | vibe_rgb
  int32_t* d_rnd_envs = nullptr;    // the env list of the last render call ...
  size_t rnd_envs_cap = 0;
  std::vector<int32_t> rnd_envs_host;   // ... as uploaded (an equal list is not uploaded again) ...
  hipEvent_t rnd_ev = nullptr;      // ... recorded behind that upload: the vector is rewritten once it has completed
  bool rnd_ev_pending = false;
  uint32_t* d_rnd_cells = nullptr;  // mgx_render_cells: scratch u32 [rnd_cells_cap]
  size_t rnd_cells_cap = 0;
  float* d_scale = nullptr;         // per-feature scale of the token decode (mgx_decode_obs)
  float scale_host[256] = {};
  bool scale_valid = false;
  void* d_stage = nullptr;          // staging for contiguous uploads of restart arguments
  size_t stage_bytes = 0;
  bool profiling = false;
  bool timing_valid = false;   // a step has been recorded since profiling was switched on
  hipEvent_t out_fence = nullptr;    // mgx_wait_before_outputs: pending, consumed by the next writer of the output buffers
  hipEvent_t world_done = nullptr;   // recorded after the world-update kernels of every step (mgx_chain_world)
  mgx_engine* world_after = nullptr;
  bool world_chained = false;
        // some engine waits on world_done // this engine's world kernels wait for that engine's most recent world_done
  hipEvent_t ev[MGX_T_COUNT + 1] = {};  // boundaries of the timing segments of the most recent step (profiling only)

  int alloc_env_bytes(void** p, size_t per_env, int fill) {  // env-major array: remembered for episode restarts
    int rc = alloc_bytes(p, per_env * (size_t)d.E, fill);
    if (rc == MGX_OK && per_env) rows_state.push_back({*p, per_env, fill});
    return rc;
  }
  template <class T>
  int alloc(T** p, size_t count, int fill = 0) {
    void* q = nullptr;
    int rc = alloc_bytes(&q, count ? count * sizeof(T) : sizeof(T), fill);
    if (rc == MGX_OK) *p = (T*)q;
    return rc;
  }
  int alloc_bytes(void** p, size_t bytes, int fill = 0) {
    void* q = nullptr;
    if (bytes == 0) bytes = 16;
    hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) return fail(MGX_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
    e = hipMemsetAsync(q, fill, bytes, stream);
    if (e != hipSuccess) return fail(MGX_ERR_HIP, std::string("hipMemset: ") + hipGetErrorString(e));
    allocs.push_back(q);
    state_bytes += (int64_t)bytes;
    *p = q;
    return MGX_OK;
  }
};

// The token-row instances of the observation kernel (the dense-output ones: mgx_obs_box.hip): the preset shapes, lean
// without / with the program block in LDS, extended with 256 threads or 512 threads and 4 / 3 / 2 encode wavefronts.
static const MgxObsInstance g_obs_instances[] = {
    MGX_OBS_INSTANCE(false, true, MGX_OBS_THREADS, MGX_OBS_THREADS / MGX_WAVE, MgxObsShapeR3, false),
    MGX_OBS_INSTANCE(false, true, MGX_OBS_THREADS, MGX_OBS_THREADS / MGX_WAVE, MgxObsShapeR3AnyLength, false),
    MGX_OBS_INSTANCE(false, false, MGX_OBS_THREADS, MGX_OBS_THREADS / MGX_WAVE, MgxObsShapeDyn, false),
    MGX_OBS_INSTANCE(false, true, MGX_OBS_THREADS, MGX_OBS_THREADS / MGX_WAVE, MgxObsShapeDyn, false),
    MGX_OBS_INSTANCE(true, false, MGX_OBS_THREADS, MGX_OBS_THREADS / MGX_WAVE, MgxObsShapeDyn, false),
    MGX_OBS_INSTANCE(true, false, 512, 4, MgxObsShapeDyn, false),
    MGX_OBS_INSTANCE(true, false, 512, 3, MgxObsShapeDyn, false),
    MGX_OBS_INSTANCE(true, false, 512, 2, MgxObsShapeDyn, false),
};
// The instance an engine runs, or nullptr.  A program whose shape equals a preset's runs that preset's instance (shape =
// compile-time constants); dense output (mgx_set_box_output) has generic instances only.  Not asked for obs_variant 9.
static const MgxObsInstance* find_obs_instance(const mgx_engine* e) {
  const bool box = e->box_dtype != MGX_BOX_OFF, x = e->d.X != 0, pl = !x && e->obs_blk_lds;
  const int variant = !box && (e->obs_variant == 3 || e->obs_variant == 5) ? e->obs_variant : 0;
  int n = (int)(sizeof g_obs_instances / sizeof *g_obs_instances);
  const MgxObsInstance* t = box ? mgx_obs_box_instances(&n) : g_obs_instances;
  for (const MgxObsInstance* r = t; r < t + n; r++)
    if (r->box == box && r->x == x && r->pl == pl && r->threads == e->obs_threads && r->ew == e->obs_ew && r->variant == variant) return r;
  return nullptr;
}
// A kernel set's dynamic LDS limit on the engine's device (MgxLdsLimit: shared by every engine, only ever raised).
static int raise_lds(MgxLdsLimit& limit, const std::vector<const void*>& kernels, const mgx_engine* e, size_t bytes) {
  HIP_TRY(limit.raise(kernels.data(), kernels.size(), e->device, bytes));
  return MGX_OK;
}
// Raise the observation kernels' dynamic LDS limit to the engine's lds_obs (mgx_create; fit_maps when new maps need a
// larger pool).
static int raise_obs_lds(mgx_engine* e) {
  if (e->sw.verbose)
    fprintf(stderr, "[mgx] obs: lds=%zu B pool=%d tokens (prefix %d) blk_lds=%d rewards_early=%d threads=%d encode wavefronts=%d (4 would need %zu B)\n",
            e->lds_obs, e->pool_tokens, e->pool_prefix, (int)e->obs_blk_lds, e->rmode, e->obs_threads, e->obs_ew, e->obs_lds_bytes(4));
  static MgxLdsLimit limit;
  int nb = 0;
  const MgxObsInstance* box = mgx_obs_box_instances(&nb);
  std::vector<const void*> kernels;   // every instance of both tables
  for (const MgxObsInstance& r : g_obs_instances) kernels.insert(kernels.end(), std::begin(r.fn), std::end(r.fn));
  for (const MgxObsInstance* r = box; r < box + nb; r++) kernels.insert(kernels.end(), std::begin(r->fn), std::end(r->fn));
  return raise_lds(limit, kernels, e, e->lds_obs);
}

// Grid of a restart kernel that walks a device list whose length only the device knows: enough workgroups to fill the chip,
// each taking every grid-th entry.  n_host >= 0: the host knows the length (host-driven restarts) and launches exactly that.
struct MgxList { const int32_t* list = nullptr; const uint32_t* n = nullptr; int n_host = -1; int passes = 1; };   // passes: see mgx_obs.h (token statistics of a restart)
// Launching and retiring idle workgroups is not free (measured: ~3 us per 1 000 wavefronts), so the grid follows the number
// of envs that finished in the most recent step the host has heard of (h_flags, written by mgx_episode_end_kernel): twice
// that, at least `lo` workgroups — a wrong guess only changes how many entries each workgroup walks.
static unsigned list_grid(const mgx_engine* e, const MgxList& l, int lo, int hi) {
  if (l.n_host >= 0) return (unsigned)std::max(1, std::min(l.n_host, e->d.E));
  const int hint = e->h_flags ? (int)std::min<uint32_t>(e->h_flags[1], 1u << 20) : 0;
  return (unsigned)std::max(1, std::min(e->d.E, std::min(hi, std::max(lo, 2 * hint))));
}
// The observation kernel's arguments (mgx_obs_kernel, and the same list for a run-time code object's kernels) and grid for one
// launch.  params[] points into the block itself: filled in place, never copied.
struct MgxObsArgs {
  MgxDev dd;
  int pool_tokens, pool_prefix, blk_start, blk_words, rmode, box_C, box_dtype, passes;
  const uint8_t* mask;
  void* box;
  const float* scale;
  const int32_t* list;
  const uint32_t* list_n;
  unsigned grid;
  void* params[14] = {&dd, &pool_tokens, &pool_prefix, &mask, &blk_start, &blk_words, &rmode, &box, &scale, &box_C, &box_dtype, &list, &list_n, &passes};
  // pl: the instance keeps the interpreted program block in LDS.  A device env list replaces the mask, without rewards only.
  MgxObsArgs(const mgx_engine* e, bool pl, bool with_rewards, const uint8_t* m, const MgxList& l) {
    const bool listed = !with_rewards && l.list, boxed = e->box_dtype != MGX_BOX_OFF;
    dd = e->d;
    if (pl)  // the interpreted sections are addressed relative to their LDS copy
      for (int k = MGX_SEC_INV_FEATURES; k < MGX_SEC_WORDLIST; k++) dd.sec[k] -= e->obs_blk_start;
    pool_tokens = e->pool_tokens; pool_prefix = e->pool_prefix;
    mask = listed ? nullptr : m;
    blk_start = e->obs_blk_start; blk_words = e->obs_blk_words; rmode = e->rmode;
    box = boxed ? e->box_out : nullptr; scale = boxed ? e->d_scale : nullptr;
    box_C = boxed ? e->box_C : 0; box_dtype = boxed ? e->box_dtype : 0;
    list = listed ? l.list : nullptr; list_n = listed ? l.n : nullptr;
    passes = l.passes;
    grid = listed ? list_grid(e, l, 128, 2048) : (unsigned)e->d.E;
  }
  MgxObsArgs(const MgxObsArgs&) = delete;
};
// The lean world unit's launcher and limit function by constant-memory slot (mgx_engine::slot).
static const struct {
  void (*launch)(bool prog_lds, int variant, size_t lds, hipStream_t stream, const MgxDev& d, int prog_words);
  bool (*set_lds)(size_t lds);
} g_world_fast[MGX_FAST_SLOTS] = {{mgx_launch_world_fast_s0, mgx_world_fast_set_lds_s0}, {mgx_launch_world_fast_s1, mgx_world_fast_set_lds_s1}};
// The lean world kernel of a run-time code object: its MgxDev lives in the module's constant memory.
static int launch_world_jit(mgx_engine* e, int prog_words) {
  mgx_engine::Jit& j = e->jit_world;
  if (j.dev_image.differs(e->d))   // (stream-ordered: the kernels still reading the old content are ahead of the copy)
    HIP_TRY(hipMemcpyAsync(j.dev_sym, &j.dev_image.host, sizeof(MgxDev), hipMemcpyHostToDevice, e->stream));
  void* params[] = {&prog_words};
  const unsigned grid = (unsigned)((e->d.E + j.epg - 1) / j.epg);
  HIP_TRY(hipModuleLaunchKernel(j.f0, grid, 1, 1, (unsigned)j.threads, 1, 1, (unsigned)e->lds_world, e->stream, params, nullptr));
  return MGX_OK;
}
// The extended games' lane-per-agent dispatch of a run-time code object (same geometry as mgx_launch_act_x).
static int launch_act_x_jit(mgx_engine* e, const MgxDev* dp, int prog_words) {
  const int ap = mgx_pow2_at_least(e->d.A);
  const int epg = e->jit_actx.epg;
  void* params[] = {&dp, &prog_words};
  HIP_TRY(hipModuleLaunchKernel(e->jit_actx.f0, (unsigned)((e->d.E + epg - 1) / epg), 1, 1, (unsigned)(epg * ap), 1, 1, (unsigned)e->lds_act, e->stream,
                                params, nullptr));
  return MGX_OK;
}
// Device-memory copy of e->d, brought up to date (stream-ordered) whenever the host table changed.
static const MgxDev* dev_copy(mgx_engine* e) {
  if (e->d_dev_image.differs(e->d)) (void)hipMemcpyAsync(e->d_dev, &e->d, sizeof(MgxDev), hipMemcpyHostToDevice, e->stream);
  return e->d_dev;
}
// ... and the extended world kernel's variant of it when that kernel keeps the hot program range in LDS.
static const MgxDev* dev_copy_hot(mgx_engine* e);
static const MgxDev* dev_copy_world_x(mgx_engine* e) { return e->prog_in_lds ? dev_copy_hot(e) : dev_copy(e); }
static const MgxDev* dev_copy_hot(mgx_engine* e) {
  MgxDev h = e->d;
  h.hot_lo = e->hot_lo;
  for (int k = 0; k < MGX_SEC_COUNT; k++)
    if (h.sec[k] >= e->hot_lo && h.sec[k] <= e->hot_hi && k != MGX_SEC_TAG_LISTS && k != MGX_SEC_SCHEDULE && k != MGX_SEC_CLASSES) h.sec[k] -= e->hot_lo;
  if (e->d_hot_image.differs(h)) (void)hipMemcpyAsync(e->d_hot, &h, sizeof(MgxDev), hipMemcpyHostToDevice, e->stream);
  return e->d_hot;
}
// The extended games' world launches of mgx_step: the lane-per-agent dispatch (an attached code object's, else the built-in
// one) and the world kernel's `phases`.
static int launch_act_x(mgx_engine* e, int pw) {
  if (e->jit_actx.mod) return launch_act_x_jit(e, dev_copy_world_x(e), pw);
  mgx_launch_act_x(e->prog_in_lds, e->lds_act, e->stream, e->d, dev_copy_world_x(e), pw);
  return MGX_OK;
}
static void launch_world_x(mgx_engine* e, int pw, int phases) {
  mgx_launch_world_x(e->prog_in_lds, e->lds_world, e->stream, e->d, dev_copy_world_x(e), pw, phases);
}
// mgx_wait_before_outputs: whatever writes the bound output buffers next goes behind the caller's event.
static int consume_out_fence(mgx_engine* e) {
  if (e->out_fence) {
    hipEvent_t ev = e->out_fence;
    e->out_fence = nullptr;
    HIP_TRY(hipStreamWaitEvent(e->stream, ev, 0));
  }
  return MGX_OK;
}
static int launch_terr(mgx_engine* e) {  // refresh the ownership maps of the envs whose territory sources changed
  if (e->d.X && e->d.NT > 0 && e->d.terr_owner) {
    hipLaunchKernelGGL(mgx_terr_kernel, dim3(e->d.E), dim3(256), 8 * 256 * 8, e->stream, e->d);
    HIP_TRY(hipGetLastError());
  }
  return MGX_OK;
}
static int launch_obs(mgx_engine* e, bool with_rewards, const uint8_t* mask = nullptr, const MgxList& l = MgxList()) {
#ifdef MGX_CPU_EMU
  (void)with_rewards; (void)mask; (void)l;
  return launch_terr(e);  // sanitizer build: the wavefront-cooperative observation kernel is not emulated
#endif
  const bool terr_fresh = e->terr_fresh;   // (consumed here whatever happens below: a stale "fresh" would skip a needed refresh)
  e->terr_fresh = false;
  int trc = consume_out_fence(e);
  if (trc) return trc;
  if (!terr_fresh) trc = launch_terr(e);   // (mgx_step already refreshed the maps for the area-effect kernel and nothing since can have changed them)
  if (trc) return trc;
  MGX_TRACE_POINT(e, "terr kernel");
  if (e->d.obsval) mgx_launch_values(e->stream, e->d, dev_copy(e), 0, mask);
  MGX_TRACE_POINT(e, "values kernel");
  if (e->rewards_ext) with_rewards = false;
  // the instance compiled for this program at run time (mgx_attach_code: lean, token rows, program block in LDS), or a row
  // of the instance tables
  const bool box = e->box_dtype != MGX_BOX_OFF, jit = !box && e->obs_variant == 9;
  const MgxObsInstance* row = jit ? nullptr : find_obs_instance(e);
  if (!jit && !row)
    return fail(MGX_ERR_PROGRAM, std::string("mgx_step: no ") + (box ? "dense-output" : "token-row") + " instance of the observation kernel for this configuration");
  MgxObsArgs a(e, jit || row->pl, with_rewards, mask, l);
  if (jit)
    HIP_TRY(hipModuleLaunchKernel(with_rewards ? e->jit_obs.f0 : e->jit_obs.f1, a.grid, 1, 1, (unsigned)e->jit_obs.threads, 1, 1, (unsigned)e->lds_obs,
                                  e->stream, a.params, nullptr));
  else
    (void)hipLaunchKernel(row->fn[with_rewards], dim3(a.grid), dim3((unsigned)row->threads), a.params, e->lds_obs, e->stream);   // (a failure is the last error)
  HIP_TRY(hipGetLastError());
  return MGX_OK;
}

// MgxDev::obs_used: nothing is known about the bound observation rows any more (stream-ordered): the next observation pass
// rewrites every row it touches in full.
static int invalidate_obs(mgx_engine* e) {
  if (e->d.obs_used) HIP_TRY(hipMemsetAsync(e->d.obs_used, 0xFF, (size_t)e->d.E * e->d.A * 2, e->stream));
  return MGX_OK;
}
// MGX_MEM_HOST: the caller-visible rows of envs [env0, env0 + n_envs) -> the bound host buffers (stream-ordered).
static int copy_out(mgx_engine* e, size_t env0, size_t n_envs) {
  if (e->mem_kind != MGX_MEM_HOST) return MGX_OK;
  const MgxDev& d = e->d;
  const size_t r0 = env0 * d.A, rows = n_envs * d.A;
  HIP_TRY(hipMemcpyAsync(e->h_obs + r0 * d.T * 3, d.obs + r0 * d.T * 3, rows * d.T * 3, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipMemcpyAsync(e->h_term + r0, d.terminals + r0, rows, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipMemcpyAsync(e->h_trunc + r0, d.truncations + r0, rows, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipMemcpyAsync(e->h_rew + r0, d.rewards + r0, rows * 4, hipMemcpyDeviceToHost, e->stream));
  return MGX_OK;
}
// The same for a list of envs (any order): one copy_out per run of consecutive envs.
static int copy_out_envs(mgx_engine* e, const int32_t* envs, size_t n) {
  if (e->mem_kind != MGX_MEM_HOST) return MGX_OK;
  std::vector<int32_t> sorted;
  if (!std::is_sorted(envs, envs + n)) {
    sorted.assign(envs, envs + n);
    std::sort(sorted.begin(), sorted.end());
    envs = sorted.data();
  }
  for (size_t k = 0; k < n;) {
    size_t j = k;
    while (j + 1 < n && envs[j + 1] == envs[j] + 1) j++;
    int rc = copy_out(e, (size_t)envs[k], (size_t)(envs[j] - envs[k] + 1));
    if (rc) return rc;
    k = j + 1;
  }
  return MGX_OK;
}
// MettaGrid::_init_buffers (mettagrid_c.cpp:294-319): clear the bound buffers, initial observations (action 0).
static int init_buffers(mgx_engine* e) {
  const MgxDev& d = e->d;
  size_t rows = (size_t)d.E * d.A;
  { int frc = consume_out_fence(e); if (frc) return frc; }
  { int irc = invalidate_obs(e); if (irc) return irc; }   // the buffer may be new and hold anything
  HIP_TRY(hipMemsetAsync(d.terminals, 0, rows, e->stream));
  HIP_TRY(hipMemsetAsync(d.truncations, 0, rows, e->stream));
  HIP_TRY(hipMemsetAsync(d.rewards, 0, rows * 4, e->stream));
  HIP_TRY(hipMemsetAsync(d.episode_rewards, 0, rows * 4, e->stream));
  HIP_TRY(hipMemsetAsync(d.executed, 0, rows * 4, e->stream));
  int rc = launch_obs(e, false);
  if (!rc) rc = copy_out(e, 0, (size_t)d.E);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));
  return MGX_OK;
}

static void free_time_averages(mgx_engine* e) {
  for (void* p : {(void*)e->ta.sum, (void*)e->ta.seen, (void*)e->ta.steps, (void*)e->d_ta_block})
    if (p) (void)hipFree(p);
  e->ta_red.destroy();
  e->ta = MgxTimeAvg{};
  e->d_ta_block = nullptr;
  e->ta_on = false; e->ta_block_bytes = 0;
}
static void free_policy_stats(mgx_engine* e) {
  for (void* p : {(void*)e->ps.assign, (void*)e->d_ps_rows, (void*)e->d_ps_list})
    if (p) (void)hipFree(p);
  e->ps_red.destroy();
  e->ps = MgxPolicyStats{};
  e->d_ps_rows = nullptr; e->d_ps_list = nullptr;
  e->ps_on = false;
}
#define MGX_SMP_RING 4
static void free_pool_sampling(mgx_engine* e) {
  if (e->d_smp_edges) (void)hipFree(e->d_smp_edges);
  if (e->h_smp_edges) (void)hipHostFree(e->h_smp_edges);
  for (hipEvent_t& ev : e->smp_ev) { if (ev) (void)hipEventDestroy(ev); ev = nullptr; }
  e->d_smp_edges = nullptr; e->h_smp_edges = nullptr;
  e->smp_on = false; e->smp_slot = 0;
}
static void free_map_stats(mgx_engine* e) {
  e->ms_snap.destroy();
  e->ms_on = false;
}
static void free_episode_stats(mgx_engine* e) {
  free_time_averages(e);   // (the time averages are finished on the episode statistics' done list)
  free_policy_stats(e);    // (... and so are the per-policy records)
  free_map_stats(e);       // (... and the per-map table reads the episode records)
  e->ep_red.destroy();
  e->ep_stats = false;
}
static void free_replay(mgx_engine* e) {
  for (const void* p : {(const void*)e->rpl.envs, (const void*)e->rpl.log, (const void*)e->rpl.cursor, (const void*)e->rpl.state,
                        (const void*)e->rpl.shadow, (const void*)e->rpl.static_cls})
    if (p) (void)hipFree(const_cast<void*>(p));
  e->rpl = MgxRpl{};
  e->rpl_n = 0;
}

static void free_step_stats(mgx_engine* e) {
  if (e->ss.cols) (void)hipFree(const_cast<uint32_t*>(e->ss.cols));
  e->ss = MgxStepStats{};
  e->ss_on = false;
}

static void free_global_state(mgx_engine* e) {
  if (e->gs.used) (void)hipFree(e->gs.used);
  e->gs = MgxGlobalState{};
  e->d_gs_mask = nullptr;
  e->gs_on = false;
}

#ifdef MGX_CPU_EMU   // the sanitizer build has no episode statistics, no replay recorder, no map generator and no step stats
static int launch_step_stats(mgx_engine*) { return MGX_OK; }
static int launch_global_state(mgx_engine*, const uint8_t*) { return MGX_OK; }
static int flush_shadow(mgx_engine*, const int32_t*, const uint32_t*, unsigned) { return MGX_OK; }
static int launch_episode_stats(mgx_engine*) { return MGX_OK; }
static int launch_time_avg_accum(mgx_engine*) { return MGX_OK; }
static int launch_time_avg_finish(mgx_engine*) { return MGX_OK; }
static int clear_time_avg(mgx_engine*, const int32_t*, const uint32_t*, int, const uint8_t*) { return MGX_OK; }
static int move_time_avg(mgx_engine*, const int32_t*, int, int) { return MGX_OK; }
static int launch_policy_stats(mgx_engine*) { return MGX_OK; }
static int launch_map_stats(mgx_engine*) { return MGX_OK; }
static int launch_pool_draw(mgx_engine*, const MgxList&) { return MGX_OK; }
static int launch_replay(mgx_engine*) { return MGX_OK; }
static int mark_replay(mgx_engine*, const int32_t*, int, uint32_t) { return MGX_OK; }
static int launch_mapgen_envs(mgx_engine*, const MgxList&, const uint32_t*) { return MGX_OK; }
#else
static int launch_mapgen_envs(mgx_engine* e, const MgxList& l, const uint32_t* dseeds_packed);   // (beside mgx_set_map_generator)
// d.shadow: bring the float stat cells of the listed envs (or all) up to date with the integer counters (mgx_episode.h)
static int flush_shadow(mgx_engine* e, const int32_t* list, const uint32_t* list_n, unsigned grid) {
  if (!e->d.shadow) return MGX_OK;
  hipLaunchKernelGGL(mgx_shadow_flush_kernel, dim3(grid), dim3(256), 0, e->stream, dev_copy(e), list, list_n);
  HIP_TRY(hipGetLastError());
  return MGX_OK;
}
// A reducer's f64 totals -> its snapshot buffer, the totals cleared by the reducer's column rule (csrc/mgx_totals.h).
template <class Kind>
static int launch_totals_snapshot(mgx_engine* e, MgxSnapshot& s, const Kind kind) {
  hipLaunchKernelGGL(mgx_totals_snapshot_kernel<Kind>, dim3(1), dim3(256), 0, e->stream, kind, (double*)s.d_totals, (double*)s.d_snap, (int)(s.bytes / 8));
  HIP_TRY(hipGetLastError());
  return MGX_OK;
}
// Episode-end statistics of the envs in the done list (csrc/mgx_episode.h): records, then batch totals (+ log).
static int launch_episode_stats(mgx_engine* e) {
  const MgxDev& d = e->d;
  MgxList dl;
  dl.n_host = -1;
  {
    int frc = flush_shadow(e, (const int32_t*)e->d_done_list, (const uint32_t*)e->d_done_n, (list_grid(e, dl, 128, 2048) * (unsigned)d.A + 255) / 256);
    if (frc) return frc;
  }
  hipLaunchKernelGGL(mgx_episode_record_kernel, dim3((list_grid(e, dl, 128, 2048) + 3) / 4), dim3(256), 0, e->stream, dev_copy(e), e->ep,
                     (const int32_t*)e->d_done_list, (const uint32_t*)e->d_done_n, e->ep_red.rec, e->ep_red.log.d_log, (const uint32_t*)e->ep_red.log.d_state,
                     e->ep_red.log.cap, (const uint32_t*)e->d_early, (const uint32_t*)e->d_episodes, (const int32_t*)(e->n_pool > 0 ? e->d_map_index : nullptr),
                     (const uint32_t*)e->dseeds);
  HIP_TRY(hipGetLastError());
  const int nchunks_max = (d.E + MGX_EP_CHUNK - 1) / MGX_EP_CHUNK;
  hipLaunchKernelGGL(mgx_episode_accum_kernel, dim3((unsigned)std::min(nchunks_max, 16)), dim3(256), 0, e->stream, e->ep,
                     (const uint32_t*)e->d_done_n, (const uint32_t*)e->ep_red.rec, e->ep_red.partial, e->ep_red.totals(), e->ep_red.ticket,
                     e->ep_red.log.d_state, e->ep_red.log.cap, e->ep_red.log.d_log ? 1 : 0);
  HIP_TRY(hipGetLastError());
  return MGX_OK;
}
// Time-averaged game stats (csrc/mgx_time_avg.h).  Every step: sums += the step's game stats, one lane per (env, column) slot,
// at most 2 048 workgroups walking the slots grid-stride.
static int launch_time_avg_accum(mgx_engine* e) {
  const long long slots = (long long)e->d.E * e->ta.L.NGP;
  const unsigned grid = (unsigned)std::max<long long>(1, std::min<long long>((slots + 255) / 256, 2048));
  hipLaunchKernelGGL(mgx_time_avg_accum_kernel, dim3(grid), dim3(256), 0, e->stream, dev_copy(e), e->ta);
  HIP_TRY(hipGetLastError());
  return MGX_OK;
}
// The envs of the done list: averages -> records (+ log), then batch totals in the fixed chunk order.
static int launch_time_avg_finish(mgx_engine* e) {
  MgxList dl;
  dl.n_host = -1;
  hipLaunchKernelGGL(mgx_time_avg_finish_kernel, dim3((list_grid(e, dl, 128, 2048) + 3) / 4), dim3(256), 0, e->stream, dev_copy(e), e->ta,
                     (const int32_t*)e->d_done_list, (const uint32_t*)e->d_done_n, e->ta_red.rec, e->ta_red.log.d_log, (const uint32_t*)e->ta_red.log.d_state,
                     e->ta_red.log.cap, (const uint32_t*)e->d_episodes);
  HIP_TRY(hipGetLastError());
  const int nchunks_max = (e->d.E + MGX_EP_CHUNK - 1) / MGX_EP_CHUNK;
  hipLaunchKernelGGL(mgx_time_avg_total_kernel, dim3((unsigned)std::min(nchunks_max, 16)), dim3(256), 0, e->stream, e->ta.L,
                     (const uint32_t*)e->d_done_n, (const uint32_t*)e->ta_red.rec, e->ta_red.partial, e->ta_red.totals(), e->ta_red.ticket,
                     e->ta_red.log.d_state, e->ta_red.log.cap, e->ta_red.log.d_log ? 1 : 0);
  HIP_TRY(hipGetLastError());
  return MGX_OK;
}
// on_episode_start: the accumulators of a device list of envs (n on the device, or n_host >= 0), or of a device mask, -> 0.
static int clear_time_avg(mgx_engine* e, const int32_t* list, const uint32_t* list_n, int n_host, const uint8_t* dmask) {
  if (!e->ta_on) return MGX_OK;
  MgxList l;
  l.list = list; l.n = list_n; l.n_host = n_host;
  hipLaunchKernelGGL(mgx_time_avg_clear_kernel, dim3(list ? list_grid(e, l, 128, 1024) : (unsigned)std::min(e->d.E, 4096)), dim3(64), 0, e->stream,
                     e->ta, list, list_n, n_host, dmask, e->d.E);
  HIP_TRY(hipGetLastError());
  return MGX_OK;
}
// d_ta_block for the packed accumulators of n envs.
static int reserve_time_avg_block(mgx_engine* e, int n) {
  const size_t bytes = mgx_ta_block_bytes(e->ta.L, (size_t)n);
  if (bytes > e->ta_block_bytes) {
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (e->d_ta_block) (void)hipFree(e->d_ta_block);
    e->d_ta_block = nullptr;
    e->ta_block_bytes = 0;
    HIP_TRY(hipMalloc((void**)&e->d_ta_block, bytes));
    e->ta_block_bytes = bytes;
  }
  return MGX_OK;
}
// The packed accumulators of n listed envs (device list) <-> d_ta_block (dir 0: get).
static int move_time_avg(mgx_engine* e, const int32_t* dlist, int n, int dir) {
  { int rc = reserve_time_avg_block(e, n); if (rc) return rc; }
  const long long lanes = (long long)n * std::max(1, e->ta.L.NG);
  hipLaunchKernelGGL(mgx_time_avg_move_kernel, dim3((unsigned)std::min<long long>((lanes + 255) / 256, 1024)), dim3(256), 0, e->stream, e->ta,
                     dlist, n, e->d_ta_block, dir);
  HIP_TRY(hipGetLastError());
  return MGX_OK;
}
// Per-policy episode statistics (csrc/mgx_policy_stats.h) of the envs of the done list: records (+ log), then batch totals in
// the fixed chunk order.  Behind launch_episode_stats, which has flushed the integer counters into the stat cells.
static int launch_policy_stats(mgx_engine* e) {
  MgxList dl;
  dl.n_host = -1;
  const int P = e->ps.L.P;
  auto kernel = P <= 2 ? mgx_policy_record_kernel<2> : P <= 4 ? mgx_policy_record_kernel<4> : P <= 8 ? mgx_policy_record_kernel<8>
                                                                                                    : mgx_policy_record_kernel<MGX_PS_MAX_POLICIES>;
  hipLaunchKernelGGL(kernel, dim3((list_grid(e, dl, 128, 2048) + 3) / 4), dim3(256), 0, e->stream, dev_copy(e), e->ps,
                     (const int32_t*)e->d_done_list, (const uint32_t*)e->d_done_n, e->ps_red.rec, e->ps_red.log.d_log, (const uint32_t*)e->ps_red.log.d_state,
                     e->ps_red.log.cap, (const uint32_t*)e->d_early, (const uint32_t*)e->d_episodes);
  HIP_TRY(hipGetLastError());
  const int nchunks_max = (e->d.E + MGX_EP_CHUNK - 1) / MGX_EP_CHUNK;
  const unsigned groups = (unsigned)((P * e->ps.L.NS + P + 255) / 256);   // work items: the (policy, column) sums, then the policy headers
  hipLaunchKernelGGL(mgx_policy_total_kernel, dim3((unsigned)std::min(nchunks_max, 16), groups), dim3(256), 0, e->stream, e->ps.L,
                     (const uint32_t*)e->d_done_n, (const uint32_t*)e->ps_red.rec, e->ps_red.partial, e->ps_red.totals(), e->ps_red.ticket,
                     e->ps_red.log.d_state, e->ps_red.log.cap, e->ps_red.log.d_log ? 1 : 0);
  HIP_TRY(hipGetLastError());
  return MGX_OK;
}
// Per-map episode statistics (csrc/mgx_pool_sample.h): the step's episode records -> the table, one thread per record.  Behind
// launch_episode_stats, which wrote the records.
static int launch_map_stats(mgx_engine* e) {
  MgxList dl;
  dl.n_host = -1;
  hipLaunchKernelGGL(mgx_map_stats_kernel, dim3((list_grid(e, dl, 128, 2048) + 255) / 256), dim3(256), 0, e->stream, (const uint32_t*)e->d_done_n,
                     (const uint32_t*)e->ep_red.rec, e->ep.rec_words, e->d.A, e->n_pool, (unsigned long long*)e->ms_snap.d_totals);
  HIP_TRY(hipGetLastError());
  return MGX_OK;
}
// The per-map table -> its snapshot buffer, the table cleared.
static int launch_map_stats_snapshot(mgx_engine* e) {
  MgxSnapshot& s = e->ms_snap;
  hipLaunchKernelGGL(mgx_map_stats_snapshot_kernel, dim3(1), dim3(256), 0, e->stream, (unsigned long long*)s.d_totals, (unsigned long long*)s.d_snap,
                     (int)(s.bytes / 8));
  HIP_TRY(hipGetLastError());
  return MGX_OK;
}
// Weighted pool sampling (csrc/mgx_pool_sample.h): the listed envs' next pool map, behind the bump of mgx_clear_rows_kernel
// (whose rotation-rule index it overwrites).
static int launch_pool_draw(mgx_engine* e, const MgxList& l) {
  if (!l.list) return fail(MGX_ERR_BAD_ARG, "pool sampling: the restart has no env list");
  const MgxPoolSample s{e->d_smp_edges, e->n_pool, e->smp_seed, e->smp_offset};
  hipLaunchKernelGGL(mgx_pool_draw_kernel, dim3((list_grid(e, l, 128, 2048) + 255) / 256), dim3(256), 0, e->stream, s, l.list,
                     l.n_host >= 0 ? (const uint32_t*)nullptr : l.n, l.n_host >= 0 ? l.n_host : 0, (const uint32_t*)e->d_episodes,
                     (const uint32_t*)nullptr, e->d_map_index);
  HIP_TRY(hipGetLastError());
  return MGX_OK;
}
// The step's changes of the watched envs -> their logs (csrc/mgx_replay.h); nothing without a watch list.
static int launch_replay(mgx_engine* e) {
  if (!e->rpl_n) return MGX_OK;
  hipLaunchKernelGGL(mgx_replay_kernel, dim3((unsigned)e->rpl_n), dim3(MGX_RPL_THREADS), 0, e->stream, dev_copy(e), e->rpl);
  HIP_TRY(hipGetLastError());
  return MGX_OK;
}
// The episodes of the envs in a DEVICE list are cut from outside a step: END marker with `flags`, keyframe next.
static int mark_replay(mgx_engine* e, const int32_t* dlist, int n, uint32_t flags) {
  if (!e->rpl_n || n <= 0) return MGX_OK;
  hipLaunchKernelGGL(mgx_replay_mark_kernel, dim3((unsigned)e->rpl_n), dim3(MGX_RPL_THREADS), 0, e->stream, dev_copy(e), e->rpl, dlist, n, flags);
  HIP_TRY(hipGetLastError());
  return MGX_OK;
}
// The chosen stat columns of every env and agent -> the caller's tensors (csrc/mgx_step_stats.h); nothing without columns.
// One lane per (row, column) pair, at most 2 048 workgroups walking the pairs grid-stride.
static int launch_step_stats(mgx_engine* e) {
  if (!e->ss_on) return MGX_OK;
  { int frc = consume_out_fence(e); if (frc) return frc; }   // (the step's observation pass has consumed it: a writer of outputs all the same)
  const long long pairs = (long long)e->d.E * e->d.A * e->ss.KA + (long long)e->d.E * e->ss.KG;
  const unsigned grid = (unsigned)std::max<long long>(1, std::min<long long>((pairs + 255) / 256, 2048));
  hipLaunchKernelGGL(mgx_step_stats_kernel, dim3(grid), dim3(256), 0, e->stream, dev_copy(e), e->ss);
  HIP_TRY(hipGetLastError());
  return MGX_OK;
}
// Every env's objects -> the caller's token rows (csrc/mgx_global_state.h): one wavefront per env, four envs per workgroup;
// `dmask` (device, u8 [E]) restricts the pass to the marked envs.  Nothing while the feature is off.
static int launch_global_state(mgx_engine* e, const uint8_t* dmask) {
  if (!e->gs_on) return MGX_OK;
  { int frc = consume_out_fence(e); if (frc) return frc; }   // (the rows are outputs like the bound buffers)
  const unsigned per = 256 / MGX_WAVE;
  hipLaunchKernelGGL(mgx_global_state_kernel, dim3(((unsigned)e->d.E + per - 1) / per), dim3(256), 0, e->stream, dev_copy(e), e->gs, dmask);
  HIP_TRY(hipGetLastError());
  return MGX_OK;
}
#endif  // MGX_CPU_EMU
static int flush_shadow_all(mgx_engine* e) {
  return flush_shadow(e, nullptr, nullptr, (unsigned)std::min<long long>(((long long)e->d.E * e->d.A + 255) / 256, 4096));
}

extern "C" {

const char* mgx_last_error(void) { return g_err.c_str(); }

// construction / episode restart: one wavefront per env on the GPU, the lane-per-env statement in the CPU sanitizer build
// (dc, maps, map_index, seeds, mask, list): `list` is an MgxList; the sanitizer build only knows masks
#ifdef MGX_CPU_EMU
#define MGX_LAUNCH_INIT(stream, dc, maps, mi, sd, mask, l) hipLaunchKernelGGL(mgx_init_kernel, dim3((d.E + MGX_WAVE - 1) / MGX_WAVE), dim3(MGX_WAVE), 0, stream, dc, maps, mi, sd, mask)
#else
#define MGX_LAUNCH_INIT(stream, dc, maps, mi, sd, mask, l)                                                                          \
  do {                                                                                                                              \
    const bool listed_ = (l).list != nullptr && (l).n_host < 0;   /* a list of unknown length: seeded inside the kernel */             \
    if (!listed_) hipLaunchKernelGGL(mgx_seed_mt_kernel, dim3((unsigned)((d.E + 255) / 256)), dim3(256), 0, stream, dc, sd, mask);    \
    /* a few listed envs: 256 threads each (latency of ONE construction); whole batches: one wavefront per env, so that as  \
       many serial registration passes as possible are in flight (rung 4, 65 536 envs: 58 ms against 265 ms) */              \
    hipLaunchKernelGGL(mgx_init_wave_kernel, dim3((l).list ? list_grid(e, (l), 128, 2048) : (unsigned)d.E),                          \
                       dim3((unsigned)(listed_ ? std::min(MGX_INIT_THREADS, std::max(MGX_WAVE, (d.H * d.W + MGX_WAVE - 1) / MGX_WAVE * MGX_WAVE)) : MGX_WAVE)), 0, \
                       stream, dc, maps, mi, listed_ ? (sd) : (const uint32_t*)nullptr, (l).list ? (const uint8_t*)nullptr : (mask),  \
                       (l).list, (l).n);                                                                                             \
  } while (0)
#endif
static std::mutex g_live_mu;
static std::vector<mgx_engine*> g_live;  // engines between mgx_create and mgx_destroy

static int hip_rc(hipError_t he, const char* what) {
  return he == hipSuccess ? MGX_OK : fail(MGX_ERR_HIP, std::string(what) + ": " + hipGetErrorString(he));
}
// MGX_VERBOSE: the paths mgx_create chose
static void report_plan(const mgx_engine* e, size_t program_words) {
  const MgxDev& d = e->d;
  if (e->aoe_kernel)
    fprintf(stderr, "[mgx] aoe kernel: %d agent stats staged per lane, %d B of LDS per workgroup\n", d.aoe_nstat, mgx_aoe_lds_bytes(d.aoe_nstat));
  fprintf(stderr, "[mgx] E=%d A=%d S=%d program=%zu B world: X=%d prog_in_lds=%d lds=%zu B\n", d.E, d.A, d.S, program_words * 4, d.X,
          (int)e->prog_in_lds, e->lds_world);
  if (d.X) fprintf(stderr, "[mgx] action-phase handlers on the %s VM\n", d.flat_top ? "register" : "LDS");
  fprintf(stderr, "[mgx] handler code: %s\n", d.gen_prog ? "generated for this program at build()" : "interpreter");
  if (!d.X && !d.act_par) fprintf(stderr, "[mgx] lean world kernel: %s\n", e->world_variant ? "the instance compiled for this shape" : "generic (shape read at run time)");
  fprintf(stderr, "[mgx] lean dispatch: move targets %s\n", !d.move_fast ? "read by every move" : d.mf_exact ?
          "resolved in the staging pass, trivial actions run ahead (exact dirty bitmap)" : "resolved in the staging pass, trivial actions run ahead (hashed dirty mask)");
  fprintf(stderr, "[mgx] lean dispatch: %s\n", d.duo ? "two agents of an env at a time (disjoint footprints)" : "one agent at a time");
  fprintf(stderr, "[mgx] action dispatch: one lane per %s\n", d.act_par ? "agent (conflict-ordered rounds)" : "env");
  if (d.X) fprintf(stderr, "[mgx] extended world kernel: %zu bytes of private memory per lane\n", mgx_world_x_private_bytes());
}

int mgx_create(const int32_t* program, size_t program_words, const uint16_t* class_maps, const uint32_t* seeds,
               int32_t num_envs, int32_t device, mgx_engine** out) {
  if (!program || !class_maps || !seeds || !out || num_envs <= 0) return fail(MGX_ERR_BAD_ARG, "mgx_create: null/empty argument");
  // ---- plan (mgx_plan.h): every refusal of the program or the maps happens here, before any HIP call ----
  const MgxSwitches sw = mgx_read_switches();
  MgxPlan plan;
  std::string why;
  int rc = mgx_plan(program, program_words, class_maps, num_envs, sw, plan, why);
  if (rc != MGX_OK) return fail(rc, why);
  HIP_TRY(hipSetDevice(device));
  mgx_engine* e = new mgx_engine();
  static_cast<MgxPlan&>(*e) = std::move(plan);
  e->sw = sw;
  e->device = device;
  e->prog.assign(program, program + program_words);
  if (sw.verbose) report_plan(e, program_words);
  MgxDev& d = e->d;
  const int32_t* P = program;
  const size_t E = d.E, HW = (size_t)d.H * d.W, S = d.S, A = d.A, rows = E * A;
#define A_(call) if (rc == MGX_OK) rc = (call)
#define H_(call, what) if (rc == MGX_OK) rc = hip_rc((call), what)
  H_(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking), "hipStreamCreate");

  // ---- allocate: the env state arrays (mgx_env_state.h: ONE list serves allocation, the restart table rows_state and the
  // records of mgx_save_envs), the derived per-env arrays, the plan's tables, caller-visible buffers ----
  int32_t* dprog = nullptr;
  A_(e->alloc(&dprog, program_words));
  e->es = mgx_env_state_layout_of(d, P, program_words);
  for (const MgxSegDef& s : e->es.segs) {
    if (s.kind == MGX_SEG_ROW) {
      A_(e->alloc_env_bytes(mgx_seg_ptr(d, s), s.bytes, s.fill));
    } else if (s.kind == MGX_SEG_WORD || s.kind == MGX_SEG_MT) {
      A_(e->alloc_bytes(mgx_seg_ptr(d, s), (size_t)s.bytes * E, s.fill));
    }
  }
  A_(e->alloc(&e->own_obs, rows * d.T * 3, 0xFF));
  // not an env state array: a restart keeps the rows and so their counts; whatever may break "0xFF behind the count" resets
  // them to 0xFFFF (invalidate_obs)
  if (sw.obs_tail) A_(e->alloc(&d.obs_used, rows, 0xFF));
  if (d.move_fast && sw.move_fast_count) A_(e->alloc(&d.mf_count, E * 2));
  A_(e->alloc(&e->own_term, rows));
  A_(e->alloc(&e->own_trunc, rows));
  A_(e->alloc(&e->own_rew, rows));
  A_(e->alloc(&e->own_act, rows));
  A_(e->alloc(&e->own_vact, rows));
  if (d.X) {   // derived per-env arrays: rebuilt from the state before they are read (DESIGN.md "Env state")
    if (d.NF && e->aoe_kernel) A_(e->alloc(&d.fx_pack, E * (size_t)d.NF));
    if (d.NM && e->aoe_kernel) A_(e->alloc(&d.mb_pack, E * (size_t)d.NM));
    if (d.NT > 0 && d.NTS > 0) A_(e->alloc(&d.terr_owner, E * (size_t)d.NT * HW, 0xFF));
    A_(e->alloc(&d.qws, E * d.QB * S));
    A_(e->alloc(&d.qvis, E * (d.QD + 1) * d.SW));
  }
  int16_t* dids = nullptr;
  uint8_t* dmap = nullptr;
  if (e->aoe_kernel) { A_(e->alloc(&dids, std::max<size_t>(1, e->aoe_stat_ids.size()))); A_(e->alloc(&dmap, 256)); }
  uint32_t* dinfo = nullptr;
  uint16_t* dtoks = nullptr;
  A_(e->alloc(&dinfo, e->cls_tokinfo.size()));
  A_(e->alloc(&dtoks, e->cls_tok.size()));
  if (e->obsval) A_(e->alloc(&d.obsval, E * A * (size_t)d.n_obs_values));
  A_(e->alloc(&e->d_dev, 1));
  A_(e->alloc(&e->d_hot, 1));
  A_(e->alloc(&e->dmaps, E * HW));
  A_(e->alloc(&e->dseeds, E));
  A_(e->alloc(&e->dmask, E));
  d.P = dprog;
  d.aoe_stat_ids = dids; d.aoe_stat_map = dmap;
  d.cls_tokinfo = dinfo; d.cls_tok = dtoks;
  d.obs = e->own_obs; d.terminals = e->own_term; d.truncations = e->own_trunc; d.rewards = e->own_rew;
  d.actions = e->own_act; d.vibe_actions = e->own_vact;

  // ---- raise the kernels' dynamic LDS limits (past 64 KB they need the opt-in attribute) ----
  if (rc == MGX_OK) {  // constant-memory slot of the lean world kernel: engines take them round-robin
    static std::mutex mu;
    static int next_slot = 0;
    std::lock_guard<std::mutex> lock(mu);
    e->slot = next_slot;
    if (!d.X) next_slot = (next_slot + 1) % MGX_FAST_SLOTS;
  }
  if (rc == MGX_OK && e->aoe_kernel && !mgx_aoe_set_lds(d.aoe_nstat, e->aoe_prog_lds ? e->prog_lds_words : 0))
    rc = fail(MGX_ERR_HIP, "mgx_create: cannot raise the area-effect kernel's dynamic LDS limit");
  if (rc == MGX_OK && !(d.X ? mgx_world_x_set_lds(e->lds_world) : g_world_fast[e->slot].set_lds(e->lds_world)))
    rc = fail(MGX_ERR_HIP, "mgx_create: cannot raise the world kernel's dynamic LDS limit");
  if (rc == MGX_OK && d.act_par && !(d.X ? mgx_act_x_set_lds(e->lds_act) : mgx_act_fast_set_lds_s0(e->lds_act)))
    rc = fail(MGX_ERR_HIP, "mgx_create: cannot raise the action kernel's dynamic LDS limit");
  A_(raise_obs_lds(e));

  // ---- upload: the program, the plan's tables, maps and seeds ----
  H_(hipMemcpyAsync(dprog, program, program_words * 4, hipMemcpyHostToDevice, e->stream), "mgx_create upload");
  if (e->aoe_kernel) {
    if (!e->aoe_stat_ids.empty())
      H_(hipMemcpyAsync(dids, e->aoe_stat_ids.data(), e->aoe_stat_ids.size() * 2, hipMemcpyHostToDevice, e->stream), "aoe stat table upload");
    H_(hipMemcpyAsync(dmap, e->aoe_stat_map.data(), 256, hipMemcpyHostToDevice, e->stream), "aoe stat table upload");
  }
  H_(hipMemcpyAsync(dinfo, e->cls_tokinfo.data(), e->cls_tokinfo.size() * 4, hipMemcpyHostToDevice, e->stream), "class token upload");
  H_(hipMemcpyAsync(dtoks, e->cls_tok.data(), e->cls_tok.size() * 2, hipMemcpyHostToDevice, e->stream), "class token upload");
  H_(hipMemcpyAsync(e->dmaps, class_maps, E * HW * 2, hipMemcpyHostToDevice, e->stream), "mgx_create upload");
  H_(hipMemcpyAsync(e->dseeds, seeds, E * 4, hipMemcpyHostToDevice, e->stream), "mgx_create upload");

  // ---- construct: the init kernel, then ctor -> _make_buffers -> set_buffers -> _init_buffers (mettagrid_c.cpp:190, 271-292) ----
  if (rc == MGX_OK) {
    MGX_LAUNCH_INIT(e->stream, dev_copy(e), (const uint16_t*)e->dmaps, (const int32_t*)nullptr, (const uint32_t*)e->dseeds,
                    (const uint8_t*)nullptr, MgxList());
    rc = hip_rc(hipGetLastError(), "mgx_init_kernel");
  }
  H_(hipStreamSynchronize(e->stream), "mgx_init_kernel");
#undef A_
#undef H_
  if (rc == MGX_OK) {
    MGX_TRACE_POINT(e, "init kernel");
    for (int i = 0; i <= MGX_T_COUNT; i++) (void)hipEventCreate(&e->ev[i]);
    (void)hipEventCreateWithFlags(&e->world_done, hipEventDisableTiming);
    rc = init_buffers(e);
  }
  if (rc != MGX_OK) { mgx_destroy(e); return rc; }
  { std::lock_guard<std::mutex> g(g_live_mu); g_live.push_back(e); }
  *out = e;
  return MGX_OK;
}

void mgx_destroy(mgx_engine* e) {
  if (!e) return;
  {  // engines chained behind this one (mgx_chain_world) lose the dependency
    std::lock_guard<std::mutex> g(g_live_mu);
    g_live.erase(std::remove(g_live.begin(), g_live.end(), e), g_live.end());
    for (mgx_engine* o : g_live) if (o->world_after == e) o->world_after = nullptr;
  }
  (void)hipSetDevice(e->device);
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  for (void* p : e->allocs) (void)hipFree(p);
  if (e->d_pool) (void)hipFree(e->d_pool);
  if (e->d_gen_recipe) (void)hipFree(e->d_gen_recipe);
  if (e->d_stage) (void)hipFree(e->d_stage);
  if (e->d_objs) (void)hipFree(e->d_objs);
  if (e->d_es_buf) (void)hipFree(e->d_es_buf);
  if (e->es_ev) (void)hipEventDestroy(e->es_ev);
  if (e->d_rnd_atlas) (void)hipFree(e->d_rnd_atlas);
  if (e->d_rnd_envs) (void)hipFree(e->d_rnd_envs);
  if (e->d_rnd_cells) (void)hipFree(e->d_rnd_cells);
  if (e->rnd_ev) (void)hipEventDestroy(e->rnd_ev);
  if (e->h_flags) (void)hipHostFree(e->h_flags);
  if (e->h_act_err) (void)hipHostFree(e->h_act_err);
  if (e->jit_world.mod) (void)hipModuleUnload(e->jit_world.mod);
  if (e->jit_obs.mod) (void)hipModuleUnload(e->jit_obs.mod);
  if (e->jit_actx.mod) (void)hipModuleUnload(e->jit_actx.mod);
  free_episode_stats(e);
  free_pool_sampling(e);
  free_replay(e);
  free_step_stats(e);
  free_global_state(e);
  for (int i = 0; i <= MGX_T_COUNT; i++) if (e->ev[i]) (void)hipEventDestroy(e->ev[i]);
  if (e->world_done) (void)hipEventDestroy(e->world_done);
  if (e->stream) (void)hipStreamDestroy(e->stream);
  delete e;
}

int mgx_set_buffers(mgx_engine* e, uint8_t* observations, uint8_t* terminals, uint8_t* truncations, float* rewards,
                    int32_t* actions, int32_t* vibe_actions, int64_t n_rows, int64_t n_tokens, int32_t mem_kind) {
  if (!e) return fail(MGX_ERR_BAD_ARG, "mgx_set_buffers: null engine");
  HIP_TRY(hipSetDevice(e->device));
  MgxDev& d = e->d;
  bool all_null = !observations && !terminals && !truncations && !rewards && !actions && !vibe_actions;
  if (!all_null) {
    if (!observations || !terminals || !truncations || !rewards || !actions || !vibe_actions)
      return fail(MGX_ERR_BAD_ARG, "mgx_set_buffers: all six buffers are required");
    if (n_rows != (int64_t)d.E * d.A)  // validate_buffers (mettagrid_c.cpp:1104-1150)
      return fail(MGX_ERR_BAD_ARG, "observations has shape [" + std::to_string(n_rows) + ", " + std::to_string(n_tokens) +
                                       ", 3] but expected [" + std::to_string((int64_t)d.E * d.A) + ", [something], 3]");
    if (n_tokens != d.T) return fail(MGX_ERR_BAD_ARG, "observations token dimension does not match num_observation_tokens");
  }
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (all_null || mem_kind == MGX_MEM_HOST) {
    d.obs = e->own_obs; d.terminals = e->own_term; d.truncations = e->own_trunc; d.rewards = e->own_rew;
    d.actions = e->own_act; d.vibe_actions = e->own_vact;
  }
  if (all_null) {
    e->mem_kind = MGX_MEM_DEVICE;
    e->external = false;
  } else if (mem_kind == MGX_MEM_HOST) {
    e->mem_kind = MGX_MEM_HOST;
    e->external = true;
    e->h_obs = observations; e->h_term = terminals; e->h_trunc = truncations; e->h_rew = rewards;
    e->h_act = actions; e->h_vact = vibe_actions;
  } else if (mem_kind == MGX_MEM_DEVICE) {
    e->mem_kind = MGX_MEM_DEVICE;
    e->external = true;
    d.obs = observations; d.terminals = terminals; d.truncations = truncations; d.rewards = rewards;
    d.actions = actions; d.vibe_actions = vibe_actions;
  } else {
    return fail(MGX_ERR_BAD_ARG, "mgx_set_buffers: unknown mem_kind");
  }
  return init_buffers(e);
}

// Table of the arrays a restart clears, on the device (rebuilt when the bound caller buffers change).
static int upload_rows(mgx_engine* e) {
  const MgxDev& d = e->d;
  std::vector<MgxRow> rows;
  for (const auto& r : e->rows_state) rows.push_back({(uint8_t*)r.base, (unsigned long long)r.row_bytes, r.fill, 0});
  // caller-visible rows of the restarted envs: terminals / truncations / rewards cleared (_init_buffers :294-319)
  rows.push_back({(uint8_t*)d.terminals, (unsigned long long)d.A, 0, 0});
  rows.push_back({(uint8_t*)d.truncations, (unsigned long long)d.A, 0, 0});
  rows.push_back({(uint8_t*)d.rewards, (unsigned long long)d.A * 4, 0, 0});
  if (rows.size() == e->rows_host.size() && memcmp(rows.data(), e->rows_host.data(), rows.size() * sizeof(MgxRow)) == 0) return MGX_OK;
  if (!e->d_rows) { int rc = e->alloc(&e->d_rows, rows.size()); if (rc) return rc; }
  HIP_TRY(hipMemcpyAsync(e->d_rows, rows.data(), rows.size() * sizeof(MgxRow), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));  // `rows` is a local
  e->rows_host = rows;
  e->n_rows = (int)rows.size();
  return MGX_OK;
}
static int stage(mgx_engine* e, size_t bytes) {
  if (bytes <= e->stage_bytes) return MGX_OK;
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (e->d_stage) (void)hipFree(e->d_stage);
  e->d_stage = nullptr;
  e->stage_bytes = 0;
  HIP_TRY(hipMalloc(&e->d_stage, bytes));
  e->stage_bytes = bytes;
  return MGX_OK;
}
// Restart the envs of a DEVICE mask: clear their state rows, rebuild them (construction kernel), initial observations.
// from_pool: maps come from the pool through d_map_index; bump: auto-reset bookkeeping (episode counter, next pool map).
// generate: the listed envs' maps are generated into dmaps first (mgx_mapgen.h; gen_seeds: one seed per list entry, or the
// slot rule base + episodes).
// l: the same envs as an ascending device list (the kernels then walk the list with a small grid instead of testing E mask bytes).
static int restart_masked(mgx_engine* e, const uint8_t* dmask, bool from_pool, bool bump, const MgxList& l = MgxList(),
                          bool generate = false, const uint32_t* gen_seeds = nullptr) {
  const MgxDev& d = e->d;
  int rc = consume_out_fence(e);   // the cleared rows include terminals / truncations / rewards
  if (rc) return rc;
  rc = upload_rows(e);
  if (rc) return rc;
#ifdef MGX_CPU_EMU
  MgxList ll;   // the sanitizer build runs the mask forms
#else
  MgxList ll = l;
#endif
  ll.passes = 2;   // new MettaGrid + set_buffers = two initial observation passes in the reference (token statistics)
  hipLaunchKernelGGL(mgx_clear_rows_kernel, dim3(ll.list ? list_grid(e, ll, 128, 1024) : (unsigned)d.E), dim3(256), 0, e->stream, (const MgxRow*)e->d_rows,
                     e->n_rows, dmask, d.E, bump ? e->d_episodes : (uint32_t*)nullptr, bump ? e->d_map_index : (int32_t*)nullptr, e->n_pool,
                     e->pool_stride, ll.list, ll.n);
  HIP_TRY(hipGetLastError());
  if (e->ta_on) { rc = clear_time_avg(e, ll.list, ll.n, ll.n_host, dmask); if (rc) return rc; }   // on_episode_start (time_averaged_stats.py:26-28)
  if (bump && from_pool && e->smp_on) { rc = launch_pool_draw(e, ll); if (rc) return rc; }   // (replaces the index the bump has just written)
  if (generate) {   // behind the bump: the map of seed base[env] + episodes[env] (or the caller's seeds) into dmaps[env]
    rc = launch_mapgen_envs(e, ll, gen_seeds);
    if (rc) return rc;
  }
  MGX_LAUNCH_INIT(e->stream, dev_copy(e),
                     (const uint16_t*)(from_pool ? e->d_pool : e->dmaps), (const int32_t*)(from_pool ? e->d_map_index : nullptr),
                     (const uint32_t*)e->dseeds, dmask, ll);
  HIP_TRY(hipGetLastError());
  return launch_obs(e, false, dmask, ll);
}
// Class ids of maps handed over by the caller: 0 = empty, else class index + 1.
static int validate_maps(const mgx_engine* e, const uint16_t* maps, size_t n_maps, const uint8_t* mask, const char* who) {
  const size_t hw = (size_t)e->d.H * e->d.W;
  const int nc = e->prog[MGX_H_NUM_CLASSES];
  for (size_t m = 0; m < n_maps; m++) {
    if (mask && !mask[m]) continue;
    for (size_t i = 0; i < hw; i++)
      if (maps[m * hw + i] > nc)
        return fail(MGX_ERR_BAD_ARG, std::string(who) + ": class map holds id " + std::to_string(maps[m * hw + i]) +
                                         " but the program has " + std::to_string(nc) + " classes");
  }
  return MGX_OK;
}
// A larger LDS token pool for the observation kernel (new maps, or a loaded state from an engine that saw denser maps).
static int grow_pool(mgx_engine* e, int need) {
  if (need <= e->pool_tokens) return MGX_OK;
  const bool jit = e->obs_variant == 9 && e->jit_obs.mod;
  e->pool_tokens = need;
  if (!e->size_obs(e->sw)) return fail(MGX_ERR_PROGRAM, MGX_OBS_LDS_REFUSAL);
  if (jit && e->lds_obs <= 64 * 1024) e->obs_variant = 9;   // (the code object's shape does not depend on the pool size)
  return raise_obs_lds(e);
}
// AoE / territory source counts of a set of maps against the capacities sized at mgx_create, and the observation kernel's
// token pool against their object lists.
static int fit_maps(mgx_engine* e, const uint16_t* maps, size_t first, size_t count, const uint8_t* mask, const char* who) {
  const MgxDev& d = e->d;
  const int32_t* P = e->prog.data();
  const size_t hw = (size_t)d.H * d.W;
  if (d.X && (d.NF || d.NM || d.NTS || mgx_sec_cnt(P, MGX_SEC_AOES) > 0 || d.NT > 0)) {
    const std::vector<MgxSources> cls = mgx_class_sources(P);
    for (size_t m = first; m < first + count; m++) {
      if (mask && !mask[m]) continue;
      const MgxSources s = mgx_map_sum(cls, maps + m * hw, hw);
      if (s.f > d.NF || s.m > d.NM || s.t > d.NTS)
        return fail(MGX_ERR_PROGRAM, std::string(who) + ": a map holds more AoE / territory sources (" + std::to_string(s.f) + " fixed, " +
                                         std::to_string(s.m) + " mobile, " + std::to_string(s.t) + " territory) than any map given to "
                                         "mgx_create (capacity " + std::to_string(d.NF) + " / " + std::to_string(d.NM) + " / " +
                                         std::to_string(d.NTS) + "): create the engine with a map that has the maximum");
    }
  }
  if (e->pool_from_maps)  // new maps may hold more non-static objects than any map seen so far
    return grow_pool(e, mgx_pool_tokens(e->pool_prefix, e->list_tokens_bound(maps, first, count, mask)));
  return MGX_OK;
}

// One per-env uint32 column of a host-driven restart: the masked envs' values of `src` (host [E], or none) travel in the
// staging block and are scattered into the device array `dst` [E] (none: only read from the block, as generator seeds are).
struct MgxResetCol { const uint32_t* src; uint32_t* dst; };
// The host-driven restart behind mgx_reset_envs*: the masked envs as ONE upload [indices | column 0 | column 1 | maps | n]
// (absent sections take no room, every section starts on a 16-byte boundary), scattered on the device; then the replay
// marker (it carries the step of the episode that ends, so it stays in front of the clear), restart_masked, and the
// restarted rows to host buffers.  gen_col: the column restart_masked's generator reads its seeds from (generate only).
static int reset_from_host(mgx_engine* e, const uint8_t* env_mask, MgxResetCol col0, MgxResetCol col1, const uint16_t* class_maps,
                           bool from_pool, bool generate = false, int gen_col = -1) {
  const MgxDev& d = e->d;
  const size_t E = d.E, HW = (size_t)d.H * d.W;
  std::vector<int32_t> idx;
  for (size_t i = 0; i < E; i++) if (env_mask[i]) idx.push_back((int32_t)i);
  if (idx.empty()) return MGX_OK;
  const size_t n = idx.size();
  const MgxResetCol cols[2] = {col0, col1};
  size_t off_col[2], end = n * 4;
  auto section = [&end](size_t bytes) { const size_t off = (end + 15) & ~(size_t)15; end = off + bytes; return off; };
  for (int c = 0; c < 2; c++) off_col[c] = section(cols[c].src ? n * 4 : 0);
  const size_t off_maps = section(class_maps ? n * HW * 2 : 0);
  const size_t off_n = section(16);   // the list length, for the list-walking kernels
  std::vector<uint8_t> host(end);
  memcpy(host.data(), idx.data(), n * 4);
  { const uint32_t n32 = (uint32_t)n; memcpy(host.data() + off_n, &n32, 4); }
  for (size_t k = 0; k < n; k++) {
    for (int c = 0; c < 2; c++) if (cols[c].src) memcpy(host.data() + off_col[c] + k * 4, cols[c].src + idx[k], 4);
    if (class_maps) memcpy(host.data() + off_maps + k * HW * 2, class_maps + (size_t)idx[k] * HW, HW * 2);
  }
  int rc = stage(e, host.size());
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(e->dmask, env_mask, E, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(e->d_stage, host.data(), host.size(), hipMemcpyHostToDevice, e->stream));
  const uint8_t* st = (const uint8_t*)e->d_stage;
  MgxList l;
  l.list = (const int32_t*)st; l.n = (const uint32_t*)(st + off_n); l.n_host = (int)n;
  for (int c = 0; c < 2; c++)
    if (cols[c].src && cols[c].dst)
      hipLaunchKernelGGL(mgx_scatter_words_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e->stream, cols[c].dst,
                         (const uint32_t*)(st + off_col[c]), l.list, (int)n);
  if (class_maps) hipLaunchKernelGGL(mgx_scatter_maps_kernel, dim3(4, (unsigned)n), dim3(256), 0, e->stream, e->dmaps,
                                     (const uint16_t*)(st + off_maps), l.list, (int)n, (int)HW);
  HIP_TRY(hipGetLastError());
  rc = mark_replay(e, l.list, (int)n, MGX_RPL_E_ABORTED);
  if (rc) return rc;
  rc = restart_masked(e, e->dmask, from_pool, false, l, generate,
                      gen_col >= 0 && cols[gen_col].src ? (const uint32_t*)(st + off_col[gen_col]) : nullptr);
  if (rc) return rc;
  rc = copy_out_envs(e, idx.data(), n);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));  // `host` is a local
  return MGX_OK;
}

int mgx_reset_envs(mgx_engine* e, const uint8_t* env_mask, const uint16_t* class_maps, const uint32_t* seeds) {
  if (!e || !env_mask) return fail(MGX_ERR_BAD_ARG, "mgx_reset_envs: null argument");
  HIP_TRY(hipSetDevice(e->device));
  if (class_maps) {
    int rc = validate_maps(e, class_maps, (size_t)e->d.E, env_mask, "mgx_reset_envs");
    if (!rc) rc = fit_maps(e, class_maps, 0, (size_t)e->d.E, env_mask, "mgx_reset_envs");
    if (rc) return rc;
  }
  return reset_from_host(e, env_mask, {seeds, e->dseeds}, {nullptr, nullptr}, class_maps, false);
}

int mgx_set_map_pool(mgx_engine* e, const uint16_t* class_maps, int32_t n_maps) {
  if (!e || !class_maps || n_maps <= 0) return fail(MGX_ERR_BAD_ARG, "mgx_set_map_pool: null/empty argument");
  if ((e->smp_on || e->ms_on) && n_maps != e->n_pool)   // (thresholds and table rows are per pool map; the same size keeps them)
    return fail(MGX_ERR_BAD_ARG, "mgx_set_map_pool: " + std::to_string(n_maps) + " maps, but pool sampling / map statistics are on for " +
                                     std::to_string(e->n_pool) + ": switch them off first (mgx_set_pool_sampling, mgx_set_map_stats)");
  HIP_TRY(hipSetDevice(e->device));
  const MgxDev& d = e->d;
  const size_t HW = (size_t)d.H * d.W;
  int rc = validate_maps(e, class_maps, (size_t)n_maps, nullptr, "mgx_set_map_pool");
  if (!rc) rc = fit_maps(e, class_maps, 0, (size_t)n_maps, nullptr, "mgx_set_map_pool");
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (e->d_pool) (void)hipFree(e->d_pool);
  e->d_pool = nullptr;
  HIP_TRY(hipMalloc((void**)&e->d_pool, (size_t)n_maps * HW * 2));
  HIP_TRY(hipMemcpyAsync(e->d_pool, class_maps, (size_t)n_maps * HW * 2, hipMemcpyHostToDevice, e->stream));
  if (!e->d_map_index) {
    rc = e->alloc(&e->d_map_index, (size_t)d.E);
    if (!rc) rc = e->alloc(&e->d_episodes, (size_t)d.E);
    if (rc) return rc;
  }
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->n_pool = n_maps;
  return MGX_OK;
}

int mgx_reset_envs_from_pool(mgx_engine* e, const uint8_t* env_mask, const int32_t* pool_index, const uint32_t* seeds) {
  if (!e || !env_mask || !pool_index) return fail(MGX_ERR_BAD_ARG, "mgx_reset_envs_from_pool: null argument");
  if (e->n_pool <= 0) return fail(MGX_ERR_BAD_ARG, "mgx_reset_envs_from_pool: no map pool (mgx_set_map_pool)");
  HIP_TRY(hipSetDevice(e->device));
  for (int i = 0; i < e->d.E; i++)
    if (env_mask[i] && (pool_index[i] < 0 || pool_index[i] >= e->n_pool))
      return fail(MGX_ERR_BAD_ARG, "mgx_reset_envs_from_pool: pool index out of range");
  return reset_from_host(e, env_mask, {(const uint32_t*)pool_index, (uint32_t*)e->d_map_index}, {seeds, e->dseeds}, nullptr, true);
}

int mgx_set_auto_reset(mgx_engine* e, int32_t enabled, int32_t pool_stride, const uint32_t* early_end_steps) {
  if (!e) return fail(MGX_ERR_BAD_ARG, "mgx_set_auto_reset: null engine");
  HIP_TRY(hipSetDevice(e->device));
  if (!enabled) { e->auto_reset = false; return MGX_OK; }
  if (e->n_pool <= 0 && !e->gen.kind) return fail(MGX_ERR_BAD_ARG, "mgx_set_auto_reset: no map pool (mgx_set_map_pool)");
  const MgxDev& d = e->d;
  int rc = MGX_OK;
  if (!e->d_next_mask) {
    rc = e->alloc(&e->d_next_mask, ((size_t)d.E + 3) & ~(size_t)3);
    if (!rc) rc = e->alloc(&e->d_counters, 2);
    if (!rc && !e->d_done_list) rc = e->alloc(&e->d_done_list, (size_t)d.E);
    if (!rc && !e->d_done_n) rc = e->alloc(&e->d_done_n, 4);
    if (rc) return rc;
    HIP_TRY(hipHostMalloc((void**)&e->h_flags, 8, hipHostMallocMapped));
    e->h_flags[0] = 0xFFFFFFFFu; e->h_flags[1] = 0;
    HIP_TRY(hipHostGetDevicePointer((void**)&e->h_flags_dev, e->h_flags, 0));
  }
  if (early_end_steps) {
    if (!e->d_early) { rc = e->alloc(&e->d_early, (size_t)d.E); if (rc) return rc; }
    HIP_TRY(hipMemcpyAsync(e->d_early, early_end_steps, (size_t)d.E * 4, hipMemcpyHostToDevice, e->stream));
  } else if (e->d_early) {
    HIP_TRY(hipMemsetAsync(e->d_early, 0, (size_t)d.E * 4, e->stream));
  }
  HIP_TRY(hipMemsetAsync(e->d_next_mask, 0, (size_t)d.E, e->stream));
  HIP_TRY(hipMemsetAsync(e->d_done_n, 0, 4, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->pool_stride = pool_stride > 0 ? pool_stride : 1;
  e->auto_reset = true;
  e->h_flags[0] = e->step_seq; e->h_flags[1] = 0;  // nothing is done before the first step
  return MGX_OK;
}

int mgx_get_episodes(mgx_engine* e, uint32_t* episodes, int32_t* map_index) {
  if (!e || (!episodes && !map_index)) return fail(MGX_ERR_BAD_ARG, "mgx_get_episodes: null argument");
  if (!e->d_episodes) return fail(MGX_ERR_BAD_ARG, "mgx_get_episodes: no map pool (mgx_set_map_pool)");
  HIP_TRY(hipSetDevice(e->device));
  if (episodes) HIP_TRY(hipMemcpyAsync(episodes, e->d_episodes, (size_t)e->d.E * 4, hipMemcpyDeviceToHost, e->stream));
  if (map_index) HIP_TRY(hipMemcpyAsync(map_index, e->d_map_index, (size_t)e->d.E * 4, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return MGX_OK;
}

#ifndef MGX_CPU_EMU
// ---- device map generator (csrc/mgx_mapgen.h) ------------------------------------------------------------------------------
static void free_map_generator(mgx_engine* e) {
  if (e->d_gen_recipe) (void)hipFree(e->d_gen_recipe);
  e->d_gen_recipe = nullptr;
  e->gen = MgxMapRecipe{};
  e->gen_lds = 0;
}
static int raise_mapgen_lds(mgx_engine* e, size_t bytes) {
  static MgxLdsLimit limit;
  return raise_lds(limit, {(const void*)mgx_mapgen_kernel, (const void*)mgx_mapscene_kernel, (const void*)mgx_maze_kernel}, e, bytes);
}
// The kernel of the recipe that is set: map k of `grid`-strided n (or *n_dev) maps (mgx_mapgen_run's arguments).
static int launch_mapgen(mgx_engine* e, unsigned grid, const uint32_t* seeds, const uint32_t* base, const uint32_t* episodes,
                         const int32_t* env_list, const uint32_t* n_dev, int n, uint16_t* out, uint32_t* cur_seed) {
#define MGX_LAUNCH_MAPGEN(kernel, recipe) \
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(MGX_WAVE), e->gen_lds, e->stream, recipe, seeds, base, episodes, env_list, n_dev, n, out, cur_seed)
  switch (e->gen.kind) {
    case MGX_GEN_RANDOM: MGX_LAUNCH_MAPGEN(mgx_mapgen_kernel, e->gen.random); break;
    case MGX_GEN_SCENE: MGX_LAUNCH_MAPGEN(mgx_mapscene_kernel, e->gen.scene); break;
    case MGX_GEN_MAZE: MGX_LAUNCH_MAPGEN(mgx_maze_kernel, e->gen.maze); break;
    default: return fail(MGX_ERR_BAD_ARG, "map generator: not set (mgx_set_map_generator)");
  }
#undef MGX_LAUNCH_MAPGEN
  HIP_TRY(hipGetLastError());
  return MGX_OK;
}
// The listed envs' maps into dmaps (restart_masked): seeds one per list entry, or base[env] + episodes[env].
static int launch_mapgen_envs(mgx_engine* e, const MgxList& l, const uint32_t* dseeds_packed) {
  if (!e->gen.kind || !l.list) return fail(MGX_ERR_BAD_ARG, "map generator: not set (mgx_set_map_generator)");
  return launch_mapgen(e, list_grid(e, l, 128, 2048), dseeds_packed, (const uint32_t*)e->d_gen_base, (const uint32_t*)e->d_episodes, l.list,
                       l.n_host >= 0 ? (const uint32_t*)nullptr : l.n, l.n_host >= 0 ? l.n_host : 0, e->dmaps, e->d_gen_seed);
}

// The setters' common end, with the plan `p` of a planner entry (csrc/mgx_mapgen_plan.h).  What needs the engine happens
// here: the capacity checks on the ONE representative map, the kernels' LDS limit, the per-slot seed arrays and the upload of
// the recipe blob with the base seeds.  The old recipe is freed only when nothing can fail any more; the new one is on (its
// three pointers into the uploaded blob) only when everything has landed.
static int accept_map_recipe(mgx_engine* e, const char* who, const MgxMapPlan& p, const uint32_t* map_seed_base) {
  const MgxDev& d = e->d;
  int rc = validate_maps(e, p.one.data(), 1, nullptr, who);   // (kept as defence behind the planner's own check: fit_maps indexes by these ids)
  if (!rc) rc = fit_maps(e, p.one.data(), 0, 1, nullptr, who);
  if (!rc) rc = raise_mapgen_lds(e, p.lds);
  if (rc) return rc;
  // accepted: replace the recipe
  void* blob = nullptr;
  HIP_TRY(hipMalloc(&blob, p.blob.size()));
  if (!e->d_gen_base) {
    rc = e->alloc(&e->d_gen_base, (size_t)d.E);
    if (!rc) rc = e->alloc(&e->d_gen_seed, (size_t)d.E);
    if (!rc && !e->d_map_index) {   // the episode counters of auto-reset (shared with the pool)
      rc = e->alloc(&e->d_map_index, (size_t)d.E);
      if (!rc) rc = e->alloc(&e->d_episodes, (size_t)d.E);
    }
    if (rc) { (void)hipFree(blob); return rc; }
  }
  HIP_TRY(hipStreamSynchronize(e->stream));
  free_map_generator(e);
  e->d_gen_recipe = blob;
  HIP_TRY(hipMemcpyAsync(blob, p.blob.data(), p.blob.size(), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(e->d_gen_base, map_seed_base, (size_t)d.E * 4, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(e->d_gen_seed, map_seed_base, (size_t)d.E * 4, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));   // the plan is the caller's local
  e->gen_lds = p.lds;
  e->gen = p.recipe;
  e->gen.point_into(blob, p.off_rename, p.off_off);
  return MGX_OK;
}
static MgxMapWorld map_world(const mgx_engine* e) { return {e->d.H, e->d.W, e->prog[MGX_H_NUM_CLASSES], getenv("MGX_MAPGEN_LDS_BYTES")}; }

int mgx_set_map_generator(mgx_engine* e, const uint16_t* inner, int32_t n_inner, int32_t border_width, int32_t border_code,
                          const uint16_t* rename, const int32_t* rename_off, int32_t n_teams, const uint32_t* map_seed_base) {
  if (!e) return fail(MGX_ERR_BAD_ARG, "mgx_set_map_generator: null engine");
  HIP_TRY(hipSetDevice(e->device));
  if (!inner) {   // off: the recipe goes, the base seeds stay allocated with the engine
    if (e->gen.kind && e->auto_reset && e->n_pool <= 0)   // (finished envs would be rebuilt from their stale dmaps)
      return fail(MGX_ERR_BAD_ARG, "mgx_set_map_generator: the generator is the map source of auto-reset; switch that off first (mgx_set_auto_reset)");
    HIP_TRY(hipStreamSynchronize(e->stream));
    free_map_generator(e);
    return MGX_OK;
  }
  MgxMapPlan p;
  std::string why;
  const int rc = mgx_plan_map_random(map_world(e), inner, n_inner, border_width, border_code, rename, rename_off, n_teams, map_seed_base, p, why);
  if (rc) return fail(rc, why);
  return accept_map_recipe(e, "mgx_set_map_generator", p, map_seed_base);
}

int mgx_set_map_scene_generator(mgx_engine* e, int32_t room_height, int32_t room_width, int32_t n_inst, int32_t rows, int32_t cols,
                                int32_t border_width, int32_t instance_border_width, int32_t border_code, int32_t instance_border_code,
                                int32_t first_on_root, const uint16_t* symbols, int32_t n_sym, const uint16_t* rename,
                                const int32_t* rename_off, int32_t n_teams, const uint32_t* map_seed_base) {
  if (!e) return fail(MGX_ERR_BAD_ARG, "mgx_set_map_scene_generator: null engine");
  HIP_TRY(hipSetDevice(e->device));
  MgxMapPlan p;
  std::string why;
  const int rc = mgx_plan_map_rooms(map_world(e), nullptr, room_height, room_width, n_inst, rows, cols, border_width, instance_border_width,
                                    border_code, instance_border_code, first_on_root, symbols, n_sym, rename, rename_off, n_teams, map_seed_base, p, why);
  if (rc) return fail(rc, why);
  return accept_map_recipe(e, "mgx_set_map_scene_generator", p, map_seed_base);
}

int mgx_set_map_maze_generator(mgx_engine* e, int32_t room_height, int32_t room_width, int32_t n_inst, int32_t rows, int32_t cols,
                               int32_t border_width, int32_t instance_border_width, int32_t border_code, int32_t instance_border_code,
                               int32_t algorithm, int32_t room_size, int32_t wall_size, int32_t wall_code, int32_t first_on_root,
                               int32_t key_offset, const uint16_t* symbols, int32_t n_sym, const uint16_t* rename,
                               const int32_t* rename_off, int32_t n_teams, const uint32_t* map_seed_base) {
  if (!e) return fail(MGX_ERR_BAD_ARG, "mgx_set_map_maze_generator: null engine");
  HIP_TRY(hipSetDevice(e->device));
  const MgxMazeArgs mz = {algorithm, room_size, wall_size, wall_code, key_offset};
  MgxMapPlan p;
  std::string why;
  const int rc = mgx_plan_map_rooms(map_world(e), &mz, room_height, room_width, n_inst, rows, cols, border_width, instance_border_width,
                                    border_code, instance_border_code, first_on_root, symbols, n_sym, rename, rename_off, n_teams, map_seed_base, p, why);
  if (rc) return fail(rc, why);
  return accept_map_recipe(e, "mgx_set_map_maze_generator", p, map_seed_base);
}

int mgx_generate_maps(mgx_engine* e, const uint32_t* map_seeds, int32_t n, uint16_t* out, int32_t out_is_device) {
  if (!e || !map_seeds || !out || n <= 0) return fail(MGX_ERR_BAD_ARG, "mgx_generate_maps: null/empty argument");
  if (!e->gen.kind) return fail(MGX_ERR_BAD_ARG, "mgx_generate_maps: no map generator (mgx_set_map_generator)");
  HIP_TRY(hipSetDevice(e->device));
  const size_t HW = (size_t)e->d.H * e->d.W, seed_bytes = ((size_t)n * 4 + 15) & ~(size_t)15;
  int rc = stage(e, seed_bytes + (out_is_device ? 0 : (size_t)n * HW * 2));
  if (rc) return rc;
  uint8_t* st = (uint8_t*)e->d_stage;
  uint16_t* dout = out_is_device ? out : (uint16_t*)(st + seed_bytes);
  HIP_TRY(hipMemcpyAsync(st, map_seeds, (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
  rc = launch_mapgen(e, (unsigned)n, (const uint32_t*)st, nullptr, nullptr, nullptr, nullptr, (int)n, dout, nullptr);
  if (rc) return rc;
  if (!out_is_device) HIP_TRY(hipMemcpyAsync(out, dout, (size_t)n * HW * 2, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));   // the caller's seeds were read; host output has landed
  return MGX_OK;
}

int mgx_reset_envs_generated(mgx_engine* e, const uint8_t* env_mask, const uint32_t* map_seeds, const uint32_t* seeds) {
  if (!e || !env_mask) return fail(MGX_ERR_BAD_ARG, "mgx_reset_envs_generated: null argument");
  if (!e->gen.kind) return fail(MGX_ERR_BAD_ARG, "mgx_reset_envs_generated: no map generator (mgx_set_map_generator)");
  HIP_TRY(hipSetDevice(e->device));
  return reset_from_host(e, env_mask, {map_seeds, nullptr}, {seeds, e->dseeds}, nullptr, false, true, 0);
}

int mgx_get_map_seeds(mgx_engine* e, uint32_t* out) {
  if (!e || !out) return fail(MGX_ERR_BAD_ARG, "mgx_get_map_seeds: null argument");
  if (!e->d_gen_seed) return fail(MGX_ERR_BAD_ARG, "mgx_get_map_seeds: no map generator (mgx_set_map_generator)");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipMemcpyAsync(out, e->d_gen_seed, (size_t)e->d.E * 4, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return MGX_OK;
}
#endif  // MGX_CPU_EMU

int mgx_attach_code(mgx_engine* e, int32_t kind, const char* path) {
  if (!e || !path) return fail(MGX_ERR_BAD_ARG, "mgx_attach_code: null argument");
#ifdef MGX_CPU_EMU
  return fail(MGX_ERR_BAD_ARG, "mgx_attach_code: not part of the sanitizer build");
#else
  HIP_TRY(hipSetDevice(e->device));
  const MgxDev& d = e->d;
  if (kind != MGX_CODE_WORLD && kind != MGX_CODE_OBS && kind != MGX_CODE_ACT_X) return fail(MGX_ERR_BAD_ARG, "mgx_attach_code: unknown kind");
  if ((d.X != 0) != (kind == MGX_CODE_ACT_X))
    return fail(MGX_ERR_PROGRAM, "mgx_attach_code: world / observation code objects are for lean programs, the dispatch one for extended programs");
  mgx_engine::Jit& j = kind == MGX_CODE_WORLD ? e->jit_world : kind == MGX_CODE_OBS ? e->jit_obs : e->jit_actx;
  if (j.mod) return fail(MGX_ERR_BAD_ARG, "mgx_attach_code: a code object of this kind is attached already");
  hipModule_t mod = nullptr;
  hipError_t he = hipModuleLoad(&mod, path);
  if (he != hipSuccess) return fail(MGX_ERR_HIP, std::string("mgx_attach_code: hipModuleLoad(") + path + "): " + hipGetErrorString(he));
  auto refuse = [&](const std::string& why) { (void)hipModuleUnload(mod); return fail(MGX_ERR_PROGRAM, "mgx_attach_code: " + why); };
  auto read_sym = [&](const char* name, void* dst, size_t bytes) -> bool {
    hipDeviceptr_t p = nullptr;
    size_t n = 0;
    if (hipModuleGetGlobal(&p, &n, mod, name) != hipSuccess || n < bytes) return false;
    return hipMemcpy(dst, p, bytes, hipMemcpyDeviceToHost) == hipSuccess;
  };
  // The 8-word mgx_jit_info block of a world / dispatch code object: empty when it fits this library, this engine's
  // program and 64 KiB of LDS, else why not.
  unsigned long long info[8] = {};
  auto info_refusal = [&](unsigned long long magic, const char* what, size_t lds, bool name_fps) -> std::string {
    if (!read_sym("mgx_jit_info", info, sizeof info) || info[0] != magic) return std::string("not a ") + what + " code object";
    if (info[1] != sizeof(MgxDev) || info[6] != (unsigned long long)MGX_VERSION) return "built against other headers than this libmgx";
    if (info[4] != e->handler_fp) {
      char buf[96] = "";
      if (name_fps) snprintf(buf, sizeof buf, " (code object %016llx, engine %016llx)", info[4], e->handler_fp);
      return std::string("generated for another program (handler tables differ)") + buf;
    }
    if (lds > 64 * 1024) return "the kernel needs more than 64 KiB of LDS";
    return "";
  };
  if (kind == MGX_CODE_ACT_X) {
    if (!d.act_par) return refuse("the engine does not run the lane-per-agent dispatch for this program");
    const std::string why = info_refusal(0x4D47584A49544131ull, "dispatch", e->lds_act, false);
    if (!why.empty()) return refuse(why);
    if ((int)info[2] != mgx_act_x_epg()) return refuse("built for another workgroup shape");
    if (hipModuleGetFunction(&j.f0, mod, "mgx_jit_act_x") != hipSuccess) return refuse("no mgx_jit_act_x kernel");
    j.epg = (int)info[2];
    j.mod = mod;
    e->d.gen_prog = (int)info[5];
  } else if (kind == MGX_CODE_WORLD) {
    if (d.act_par) return refuse("the engine runs the lane-per-agent dispatch (MGX_ACT_LEAN), not the kernel this code object replaces");
    const std::string why = info_refusal(0x4D47584A49545731ull, "world", e->lds_world, true);
    if (!why.empty()) return refuse(why);
    hipDeviceptr_t sym = nullptr;
    size_t n = 0;
    if (hipModuleGetGlobal(&sym, &n, mod, "g_mgx_dev") != hipSuccess || n != sizeof(MgxDev)) return refuse("no g_mgx_dev symbol of the right size");
    if (hipModuleGetFunction(&j.f0, mod, e->prog_in_lds ? "mgx_jit_world_pl" : "mgx_jit_world_pg") != hipSuccess)
      return refuse(std::string("no ") + (e->prog_in_lds ? "mgx_jit_world_pl" : "mgx_jit_world_pg") + " kernel");
    {   // a code object compiled for one shape (MGX_JIT_WORLD_SHAPE): every field equal, with the handler id it will run under
      int ks[1 + MGX_WORLD_SHAPE_NFIELDS] = {}, mine[MGX_WORLD_SHAPE_NFIELDS];
      if (!read_sym("mgx_jit_world_shape", ks, sizeof ks)) return refuse("no mgx_jit_world_shape symbol");
      MgxDev t = d;
      t.gen_prog = (int)info[5];
      mgx_world_shape_of(t, mine);
      if (ks[0] != 0 && (ks[0] != MGX_WORLD_SHAPE_NFIELDS || memcmp(ks + 1, mine, sizeof mine) != 0)) return refuse("compiled for another world shape");
    }
    j.dev_sym = sym; j.epg = (int)info[2]; j.threads = (int)info[3];
    j.mod = mod;
    e->d.gen_prog = (int)info[5];
  } else {
    long long info[24] = {};
    if (!read_sym("mgx_jit_obs_info", info, sizeof info) || info[0] != 0x4D47584A49544F31ll) return refuse("not an observation code object");
    if (info[1] != (long long)sizeof(MgxDev) || info[4] != MGX_VERSION) return refuse("built against other headers than this libmgx");
    if (!e->obs_blk_lds || e->box_dtype != MGX_BOX_OFF) return refuse("the engine does not run the lean token-row kernel with the program block in LDS");
    const long long* K = info + 5;   // H, W, A, S, T, NOFF, BASE, NOV, NT, NRW, FLAGS, MAX_STEPS, BLKW, MASK_FEAT, REWARDS_EARLY
    const int rmode = e->rmode;
    const bool same = d.H == K[0] && d.W == K[1] && d.A == K[2] && d.S == K[3] && d.T == K[4] && d.NOFF == K[5] && d.base == K[6] &&
                      d.n_obs_values == K[7] && d.NT == K[8] && d.NRW == K[9] && d.flags == K[10] && (K[11] < 0 || d.max_steps == K[11]) &&
                      e->obs_blk_words == K[12] && d.aoe_mask_feat == K[13] && rmode == K[14];
    if (!same) return refuse("compiled for another observation shape");
    if (e->lds_obs > 64 * 1024) return refuse("the kernel needs more than 64 KiB of LDS");
    if (hipModuleGetFunction(&j.f0, mod, "mgx_jit_obs_r") != hipSuccess || hipModuleGetFunction(&j.f1, mod, "mgx_jit_obs_n") != hipSuccess)
      return refuse("kernels missing");
    j.threads = (int)info[2];
    j.mod = mod;
    e->obs_variant = 9;
  }
  return MGX_OK;
#endif
}

int mgx_set_episode_stats(mgx_engine* e, int32_t enabled, int32_t log_capacity, int32_t log_per_agent) {
  if (!e) return fail(MGX_ERR_BAD_ARG, "mgx_set_episode_stats: null engine");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  free_episode_stats(e);
  if (!enabled) return MGX_OK;
#ifdef MGX_CPU_EMU
  return fail(MGX_ERR_BAD_ARG, "mgx_set_episode_stats: not part of the sanitizer build");
#else
  static_assert(MGX_EPT_HEADER == MGX_EP_TOT_HDR, "totals header");
  if (log_capacity < 0) return fail(MGX_ERR_BAD_ARG, "mgx_set_episode_stats: negative log capacity");
  const MgxDev& d = e->d;
  e->ep = mgx_ep_layout(d.NG, d.NS, d.A, d.NSP, log_per_agent ? 1 : 0);
  { int rc = e->ep_red.create(e->stream, (size_t)d.E, e->ep.rec_words, e->ep_tw(), log_capacity, e->ep.log_words); if (rc) return rc; }
  if (!e->d_done_list) { int rc = e->alloc(&e->d_done_list, (size_t)d.E); if (rc) return rc; }
  if (!e->d_done_n) { int rc = e->alloc(&e->d_done_n, 4); if (rc) return rc; }
  // totals start as a cleared snapshot would leave them
  { int rc = launch_totals_snapshot(e, e->ep_red.snap, MgxEpKind{}); if (rc) return rc; }
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->ep_stats = true;
  return MGX_OK;
#endif
}

int mgx_episode_stats_layout(mgx_engine* e, int32_t* out) {
  if (!e || !out) return fail(MGX_ERR_BAD_ARG, "mgx_episode_stats_layout: null argument");
  if (!e->ep_stats) return fail(MGX_ERR_BAD_ARG, "mgx_episode_stats_layout: episode statistics are off (mgx_set_episode_stats)");
  const MgxEpLayout& L = e->ep;
  const int32_t v[MGX_EPL_COUNT] = {L.NG, L.NS, L.A, e->ep_tw(), L.rec_words, L.log_words, L.off_game, L.off_gbits, L.off_agent, L.off_abits,
                                    L.off_rew, L.off_pa, L.off_pabits, L.off_invk, L.off_invn, L.per_agent, e->ep_red.log.cap};
  memcpy(out, v, sizeof(v));
  return MGX_OK;
}

int mgx_record_episodes(mgx_engine* e, const uint8_t* env_mask) {
  if (!e || !env_mask) return fail(MGX_ERR_BAD_ARG, "mgx_record_episodes: null argument");
  if (!e->ep_stats) return fail(MGX_ERR_BAD_ARG, "mgx_record_episodes: episode statistics are off (mgx_set_episode_stats)");
  if (e->auto_reset) return fail(MGX_ERR_BAD_ARG, "mgx_record_episodes: the engine is in auto-reset mode and records finished envs itself");
  HIP_TRY(hipSetDevice(e->device));
  std::vector<int32_t> idx;
  for (int i = 0; i < e->d.E; i++) if (env_mask[i]) idx.push_back(i);
  if (idx.empty()) return MGX_OK;
  const uint32_t n = (uint32_t)idx.size();
  HIP_TRY(hipMemcpyAsync(e->d_done_list, idx.data(), (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(e->d_done_n, &n, 4, hipMemcpyHostToDevice, e->stream));
  int rc = launch_episode_stats(e);
  if (!rc && e->ms_on) rc = launch_map_stats(e);
  if (!rc && e->ps_on) rc = launch_policy_stats(e);
  if (!rc && e->ta_on) rc = launch_time_avg_finish(e);
  if (!rc) rc = mark_replay(e, e->d_done_list, (int)n, 0);
  if (rc) return rc;
  HIP_TRY(hipMemsetAsync(e->d_done_n, 0, 4, e->stream));   // the list belongs to this call only
  HIP_TRY(hipStreamSynchronize(e->stream));  // `idx` and `n` are locals
  return MGX_OK;
}

int mgx_request_episode_stats(mgx_engine* e) {
  if (!e) return fail(MGX_ERR_BAD_ARG, "mgx_request_episode_stats: null engine");
  if (!e->ep_stats) return fail(MGX_ERR_BAD_ARG, "mgx_request_episode_stats: episode statistics are off (mgx_set_episode_stats)");
#ifdef MGX_CPU_EMU
  return MGX_OK;
#else
  return e->ep_red.snap.request(e->device, e->stream, [e] { return launch_totals_snapshot(e, e->ep_red.snap, MgxEpKind{}); });
#endif
}

int mgx_fetch_episode_stats(mgx_engine* e, int32_t wait, double* totals, int32_t* ready) {
  if (!e || !totals || !ready) return fail(MGX_ERR_BAD_ARG, "mgx_fetch_episode_stats: null argument");
  *ready = 0;
  if (!e->ep_stats) return fail(MGX_ERR_BAD_ARG, "mgx_fetch_episode_stats: episode statistics are off (mgx_set_episode_stats)");
  return e->ep_red.snap.fetch(e->device, wait, totals, ready);
}

int mgx_drain_episode_log(mgx_engine* e, uint32_t* records, int32_t max_records, int32_t* n_records, int32_t* n_dropped) {
  if (!e || !records || !n_records) return fail(MGX_ERR_BAD_ARG, "mgx_drain_episode_log: null argument");
  if (!e->ep_stats || !e->ep_red.log.d_log) return fail(MGX_ERR_BAD_ARG, "mgx_drain_episode_log: no episode log (mgx_set_episode_stats)");
  if (max_records < e->ep_red.log.cap) return fail(MGX_ERR_BAD_ARG, "mgx_drain_episode_log: the buffer must hold the whole log (log_capacity records)");
  return e->ep_red.log.drain(e->device, e->stream, records, n_records, n_dropped);
}

// ---- time-averaged game stats (csrc/mgx_time_avg.h) -----------------------------------------------------------------------
static void ta_layout_words(const MgxTaLayout& L, int log_cap, int32_t* out) {
  const int32_t v[MGX_TAL_COUNT] = {L.NG, L.NGW, L.rec_words, L.rec_words, MGX_TA_HDR, L.off_avg, L.off_seen, L.tot_words, MGX_TA_TOT_HDR, log_cap};
  memcpy(out, v, sizeof(v));
}
int mgx_time_average_layout_of(int32_t num_game_stats, int32_t log_capacity, int32_t* out) {
  if (!out || num_game_stats < 0 || log_capacity < 0) return fail(MGX_ERR_BAD_ARG, "mgx_time_average_layout_of: null / negative argument");
  ta_layout_words(mgx_ta_layout(num_game_stats), log_capacity, out);
  return MGX_OK;
}
int mgx_time_average_layout(mgx_engine* e, int32_t* out) {
  if (!e || !out) return fail(MGX_ERR_BAD_ARG, "mgx_time_average_layout: null argument");
  if (!e->ta_on) return fail(MGX_ERR_BAD_ARG, "mgx_time_average_layout: time averages are off (mgx_set_time_averages)");
  ta_layout_words(e->ta.L, e->ta_red.log.cap, out);
  return MGX_OK;
}

int mgx_set_time_averages(mgx_engine* e, int32_t enabled, int32_t log_capacity) {
  if (!e) return fail(MGX_ERR_BAD_ARG, "mgx_set_time_averages: null engine");
  if (enabled && !e->ep_stats)
    return fail(MGX_ERR_BAD_ARG, "mgx_set_time_averages: episode statistics are off (mgx_set_episode_stats): the averages are finished on their done list");
  if (enabled && log_capacity < 0) return fail(MGX_ERR_BAD_ARG, "mgx_set_time_averages: negative log capacity");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  free_time_averages(e);
  if (!enabled) return MGX_OK;
#ifdef MGX_CPU_EMU
  return fail(MGX_ERR_BAD_ARG, "mgx_set_time_averages: not part of the sanitizer build");
#else
  static_assert(MGX_TAT_HEADER == MGX_TA_TOT_HDR, "totals header");
  const MgxDev& d = e->d;
  e->ta.L = mgx_ta_layout(d.NG);
  const MgxTaLayout& L = e->ta.L;
  const size_t E = (size_t)d.E;
  const size_t sum_bytes = std::max<size_t>(8, E * L.NG * 8), seen_bytes = std::max<size_t>(4, E * L.NGW * 4);
  HIP_TRY(hipMalloc((void**)&e->ta.sum, sum_bytes));
  HIP_TRY(hipMalloc((void**)&e->ta.seen, seen_bytes));
  HIP_TRY(hipMalloc((void**)&e->ta.steps, E * 4));
  { int rc = e->ta_red.create(e->stream, E, L.rec_words, L.tot_words, log_capacity, L.rec_words); if (rc) return rc; }
  // an episode's accumulators are zero when it starts; an env inside an episode now finishes it as a partial one
  HIP_TRY(hipMemsetAsync(e->ta.sum, 0, sum_bytes, e->stream));
  HIP_TRY(hipMemsetAsync(e->ta.seen, 0, seen_bytes, e->stream));
  HIP_TRY(hipMemsetAsync(e->ta.steps, 0, E * 4, e->stream));
  // totals start as a cleared snapshot would leave them
  { int rc = launch_totals_snapshot(e, e->ta_red.snap, MgxTaKind{}); if (rc) return rc; }
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->ta_on = true;
  return MGX_OK;
#endif
}

int mgx_request_time_averages(mgx_engine* e) {
  if (!e) return fail(MGX_ERR_BAD_ARG, "mgx_request_time_averages: null engine");
  if (!e->ta_on) return fail(MGX_ERR_BAD_ARG, "mgx_request_time_averages: time averages are off (mgx_set_time_averages)");
#ifdef MGX_CPU_EMU
  return MGX_OK;
#else
  return e->ta_red.snap.request(e->device, e->stream, [e] { return launch_totals_snapshot(e, e->ta_red.snap, MgxTaKind{}); });
#endif
}

int mgx_fetch_time_averages(mgx_engine* e, int32_t wait, double* totals, int32_t* ready) {
  if (!e || !totals || !ready) return fail(MGX_ERR_BAD_ARG, "mgx_fetch_time_averages: null argument");
  *ready = 0;
  if (!e->ta_on) return fail(MGX_ERR_BAD_ARG, "mgx_fetch_time_averages: time averages are off (mgx_set_time_averages)");
  return e->ta_red.snap.fetch(e->device, wait, totals, ready);
}

int mgx_drain_time_average_log(mgx_engine* e, uint32_t* records, int32_t max_records, int32_t* n_records, int32_t* n_dropped) {
  if (!e || !records || !n_records) return fail(MGX_ERR_BAD_ARG, "mgx_drain_time_average_log: null argument");
  if (!e->ta_on || !e->ta_red.log.d_log) return fail(MGX_ERR_BAD_ARG, "mgx_drain_time_average_log: no log (mgx_set_time_averages)");
  if (max_records < e->ta_red.log.cap) return fail(MGX_ERR_BAD_ARG, "mgx_drain_time_average_log: the buffer must hold the whole log (log_capacity records)");
  return e->ta_red.log.drain(e->device, e->stream, records, n_records, n_dropped);
}

// ---- per-policy episode statistics (csrc/mgx_policy_stats.h) ----------------------------------------------------------------
static void ps_layout_words(const MgxPsLayout& L, int log_cap, int32_t* out) {
  const int32_t v[MGX_PSL_COUNT] = {L.NS, L.A, L.P, L.NSW, L.rec_words, L.rec_words, MGX_PS_HDR, L.off_rew, L.off_cnt, L.off_sum, L.off_bits,
                                    L.tot_words, MGX_PS_TOT_HDR, MGX_PS_TOT_POLICY, L.tot_off_sum, L.tot_off_cnt, log_cap};
  memcpy(out, v, sizeof(v));
}
static int ps_check_policies(int32_t P, const char* who) {
  static_assert(MGX_MAX_POLICIES == MGX_PS_MAX_POLICIES && MGX_PST_HEADER == MGX_PS_TOT_HDR && MGX_PST_POLICY_WORDS == MGX_PS_TOT_POLICY, "mgx.h");
  if (P < 1 || P > MGX_MAX_POLICIES)
    return fail(MGX_ERR_BAD_ARG, std::string(who) + ": " + std::to_string(P) + " policies, outside [1, " + std::to_string(MGX_MAX_POLICIES) + "]");
  return MGX_OK;
}
static int ps_check_rows(const uint8_t* rows, size_t n_rows, int A, int P, const char* who) {
  for (size_t k = 0; k < n_rows * (size_t)A; k++)
    if (rows[k] >= P)
      return fail(MGX_ERR_BAD_ARG, std::string(who) + ": row " + std::to_string(k / A) + ", agent " + std::to_string(k % A) + ": policy " +
                                       std::to_string(rows[k]) + " of " + std::to_string(P));
  return MGX_OK;
}
int mgx_policy_stats_layout_of(int32_t num_agent_stats, int32_t num_agents, int32_t num_policies, int32_t log_capacity, int32_t* out) {
  if (!out || num_agent_stats < 0 || num_agents < 1 || log_capacity < 0)
    return fail(MGX_ERR_BAD_ARG, "mgx_policy_stats_layout_of: null / negative argument");
  { int rc = ps_check_policies(num_policies, "mgx_policy_stats_layout_of"); if (rc) return rc; }
  ps_layout_words(mgx_ps_layout(num_agent_stats, num_agents, num_agent_stats, num_policies), log_capacity, out);
  return MGX_OK;
}
int mgx_policy_stats_layout(mgx_engine* e, int32_t* out) {
  if (!e || !out) return fail(MGX_ERR_BAD_ARG, "mgx_policy_stats_layout: null argument");
  if (!e->ps_on) return fail(MGX_ERR_BAD_ARG, "mgx_policy_stats_layout: policy statistics are off (mgx_set_policy_stats)");
  ps_layout_words(e->ps.L, e->ps_red.log.cap, out);
  return MGX_OK;
}

int mgx_set_policy_stats(mgx_engine* e, int32_t enabled, int32_t num_policies, const uint8_t* assignments, int32_t log_capacity) {
  if (!e) return fail(MGX_ERR_BAD_ARG, "mgx_set_policy_stats: null engine");
  if (enabled) {   // every refusal comes before anything is touched
    if (!e->ep_stats)
      return fail(MGX_ERR_BAD_ARG, "mgx_set_policy_stats: episode statistics are off (mgx_set_episode_stats): the records are written on their done list");
    if (!assignments) return fail(MGX_ERR_BAD_ARG, "mgx_set_policy_stats: null assignment table");
    if (log_capacity < 0) return fail(MGX_ERR_BAD_ARG, "mgx_set_policy_stats: negative log capacity");
    int rc = ps_check_policies(num_policies, "mgx_set_policy_stats");
    if (!rc) rc = ps_check_rows(assignments, (size_t)e->d.E, e->d.A, num_policies, "mgx_set_policy_stats");
    if (rc) return rc;
  }
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  free_policy_stats(e);
  if (!enabled) return MGX_OK;
#ifdef MGX_CPU_EMU
  return fail(MGX_ERR_BAD_ARG, "mgx_set_policy_stats: not part of the sanitizer build");
#else
  const MgxDev& d = e->d;
  e->ps.L = mgx_ps_layout(d.NS, d.A, d.NSP, num_policies);
  const MgxPsLayout& L = e->ps.L;
  const size_t E = (size_t)d.E, table = E * d.A;
  HIP_TRY(hipMalloc((void**)&e->ps.assign, table));
  HIP_TRY(hipMalloc((void**)&e->d_ps_rows, table));
  HIP_TRY(hipMalloc((void**)&e->d_ps_list, E * 4));
  { int rc = e->ps_red.create(e->stream, E, L.rec_words, L.tot_words, log_capacity, L.rec_words); if (rc) return rc; }
  HIP_TRY(hipMemcpyAsync(e->ps.assign, assignments, table, hipMemcpyHostToDevice, e->stream));
  // totals start as a cleared snapshot would leave them
  { int rc = launch_totals_snapshot(e, e->ps_red.snap, MgxPsKind{L.tot_off_sum}); if (rc) return rc; }
  HIP_TRY(hipStreamSynchronize(e->stream));   // (`assignments` is the caller's)
  e->ps_on = true;
  return MGX_OK;
#endif
}

int mgx_set_policy_assignments(mgx_engine* e, const int32_t* envs, int32_t n, const uint8_t* rows) {
  if (!e || !rows) return fail(MGX_ERR_BAD_ARG, "mgx_set_policy_assignments: null argument");
  if (!e->ps_on) return fail(MGX_ERR_BAD_ARG, "mgx_set_policy_assignments: policy statistics are off (mgx_set_policy_stats)");
  if (!envs || n <= 0) return fail(MGX_ERR_BAD_ARG, "mgx_set_policy_assignments: empty env list");
  std::vector<uint8_t> dup((size_t)e->d.E, 0);
  for (int32_t k = 0; k < n; k++) {
    if (envs[k] < 0 || envs[k] >= e->d.E)
      return fail(MGX_ERR_BAD_ARG, "mgx_set_policy_assignments: env index " + std::to_string(envs[k]) + " out of range [0, " + std::to_string(e->d.E) + ")");
    if (dup[envs[k]]++) return fail(MGX_ERR_BAD_ARG, "mgx_set_policy_assignments: env " + std::to_string(envs[k]) + " listed twice");
  }
  { int rc = ps_check_rows(rows, (size_t)n, e->d.A, e->ps.L.P, "mgx_set_policy_assignments"); if (rc) return rc; }
#ifndef MGX_CPU_EMU
  HIP_TRY(hipSetDevice(e->device));
  const long long cells = (long long)n * e->d.A;
  HIP_TRY(hipMemcpyAsync(e->d_ps_list, envs, (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(e->d_ps_rows, rows, (size_t)cells, hipMemcpyHostToDevice, e->stream));
  hipLaunchKernelGGL(mgx_policy_assign_kernel, dim3((unsigned)std::min<long long>((cells + 255) / 256, 1024)), dim3(256), 0, e->stream, e->ps.assign,
                     (const int32_t*)e->d_ps_list, (int)n, (const uint8_t*)e->d_ps_rows, e->d.A);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(e->stream));   // (`envs` and `rows` are the caller's, and the staging is reused by the next call)
#endif
  return MGX_OK;
}

int mgx_request_policy_stats(mgx_engine* e) {
  if (!e) return fail(MGX_ERR_BAD_ARG, "mgx_request_policy_stats: null engine");
  if (!e->ps_on) return fail(MGX_ERR_BAD_ARG, "mgx_request_policy_stats: policy statistics are off (mgx_set_policy_stats)");
#ifdef MGX_CPU_EMU
  return MGX_OK;
#else
  return e->ps_red.snap.request(e->device, e->stream,
                                [e] { return launch_totals_snapshot(e, e->ps_red.snap, MgxPsKind{e->ps.L.tot_off_sum}); });
#endif
}

int mgx_fetch_policy_stats(mgx_engine* e, int32_t wait, double* totals, int32_t* ready) {
  if (!e || !totals || !ready) return fail(MGX_ERR_BAD_ARG, "mgx_fetch_policy_stats: null argument");
  *ready = 0;
  if (!e->ps_on) return fail(MGX_ERR_BAD_ARG, "mgx_fetch_policy_stats: policy statistics are off (mgx_set_policy_stats)");
  return e->ps_red.snap.fetch(e->device, wait, totals, ready);
}

int mgx_drain_policy_log(mgx_engine* e, uint32_t* records, int32_t max_records, int32_t* n_records, int32_t* n_dropped) {
  if (!e || !records || !n_records) return fail(MGX_ERR_BAD_ARG, "mgx_drain_policy_log: null argument");
  if (!e->ps_on || !e->ps_red.log.d_log) return fail(MGX_ERR_BAD_ARG, "mgx_drain_policy_log: no log (mgx_set_policy_stats)");
  if (max_records < e->ps_red.log.cap) return fail(MGX_ERR_BAD_ARG, "mgx_drain_policy_log: the buffer must hold the whole log (log_capacity records)");
  return e->ps_red.log.drain(e->device, e->stream, records, n_records, n_dropped);
}

#ifndef MGX_CPU_EMU
// ---- weighted pool sampling and per-map episode statistics (csrc/mgx_pool_sample.h) ------------------------------------------
int mgx_pool_quantise(const double* weights, int32_t n, uint64_t* edges) {
  static_assert(sizeof(uint64_t) == sizeof(unsigned long long) && MGX_MS_COUNT == MGX_MS_COLS, "mgx.h");
  if (const char* why = mgx_pool_quantise_host(weights, n, (unsigned long long*)edges)) return fail(MGX_ERR_BAD_ARG, std::string("mgx_pool_quantise: ") + why);
  return MGX_OK;
}
int mgx_pool_draw_words(uint32_t sample_seed, const uint32_t* a, const uint32_t* k, int32_t n, uint32_t* out) {
  if (!a || !k || !out || n < 0) return fail(MGX_ERR_BAD_ARG, "mgx_pool_draw_words: null / negative argument");
  for (int32_t i = 0; i < n; i++) out[i] = mgx_pool_draw_word(sample_seed, a[i], k[i]);
  return MGX_OK;
}

// Thresholds of `weights` through the next pinned slot to the device, ordered on the engine's stream.  The host waits only when
// the slot's upload of MGX_SMP_RING calls ago has not landed yet.
static int upload_pool_edges(mgx_engine* e, const std::vector<unsigned long long>& edges) {
  const int slot = e->smp_slot;
  e->smp_slot = (slot + 1) % MGX_SMP_RING;
  HIP_TRY(hipEventSynchronize(e->smp_ev[slot]));   // (an event never recorded counts as complete)
  unsigned long long* h = e->h_smp_edges + (size_t)slot * e->n_pool;
  memcpy(h, edges.data(), edges.size() * 8);
  HIP_TRY(hipMemcpyAsync(e->d_smp_edges, h, edges.size() * 8, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipEventRecord(e->smp_ev[slot], e->stream));
  return MGX_OK;
}

int mgx_set_pool_sampling(mgx_engine* e, const double* weights, uint32_t sample_seed, uint32_t env_offset) {
  if (!e) return fail(MGX_ERR_BAD_ARG, "mgx_set_pool_sampling: null engine");
  std::vector<unsigned long long> edges;
  if (weights) {   // every refusal comes before anything is touched
    if (e->n_pool <= 0) return fail(MGX_ERR_BAD_ARG, "mgx_set_pool_sampling: no map pool (mgx_set_map_pool)");
    edges.resize((size_t)e->n_pool);
    if (const char* why = mgx_pool_quantise_host(weights, e->n_pool, edges.data()))
      return fail(MGX_ERR_BAD_ARG, std::string("mgx_set_pool_sampling: ") + why);
  }
  HIP_TRY(hipSetDevice(e->device));
  if (!weights) {
    if (e->smp_on) HIP_TRY(hipStreamSynchronize(e->stream));   // (restarts enqueued earlier still read the thresholds)
    free_pool_sampling(e);
    return MGX_OK;
  }
  if (!e->smp_on) {
    HIP_TRY(hipMalloc((void**)&e->d_smp_edges, edges.size() * 8));
    HIP_TRY(hipHostMalloc((void**)&e->h_smp_edges, (size_t)MGX_SMP_RING * edges.size() * 8, hipHostMallocDefault));
    for (hipEvent_t& ev : e->smp_ev) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  }
  int rc = upload_pool_edges(e, edges);
  if (rc) { free_pool_sampling(e); return rc; }
  e->smp_seed = sample_seed; e->smp_offset = env_offset;
  e->smp_on = true;
  return MGX_OK;
}

int mgx_set_pool_weights(mgx_engine* e, const double* weights) {
  if (!e || !weights) return fail(MGX_ERR_BAD_ARG, "mgx_set_pool_weights: null argument");
  if (!e->smp_on) return fail(MGX_ERR_BAD_ARG, "mgx_set_pool_weights: pool sampling is off (mgx_set_pool_sampling)");
  std::vector<unsigned long long> edges((size_t)e->n_pool);
  if (const char* why = mgx_pool_quantise_host(weights, e->n_pool, edges.data()))
    return fail(MGX_ERR_BAD_ARG, std::string("mgx_set_pool_weights: ") + why);
  HIP_TRY(hipSetDevice(e->device));
  return upload_pool_edges(e, edges);
}

int mgx_pool_draws(mgx_engine* e, const int32_t* envs, const uint32_t* episodes, int32_t n, int32_t* map_index_out) {
  if (!e || !envs || !episodes || !map_index_out) return fail(MGX_ERR_BAD_ARG, "mgx_pool_draws: null argument");
  if (!e->smp_on) return fail(MGX_ERR_BAD_ARG, "mgx_pool_draws: pool sampling is off (mgx_set_pool_sampling)");
  if (n <= 0) return n == 0 ? MGX_OK : fail(MGX_ERR_BAD_ARG, "mgx_pool_draws: negative count");
  for (int32_t k = 0; k < n; k++)
    if (envs[k] < 0 || envs[k] >= e->d.E)
      return fail(MGX_ERR_BAD_ARG, "mgx_pool_draws: env index " + std::to_string(envs[k]) + " out of range [0, " + std::to_string(e->d.E) + ")");
  HIP_TRY(hipSetDevice(e->device));
  const size_t col = ((size_t)n * 4 + 15) & ~(size_t)15;
  int rc = stage(e, 3 * col);
  if (rc) return rc;
  uint8_t* st = (uint8_t*)e->d_stage;
  HIP_TRY(hipMemcpyAsync(st, envs, (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(st + col, episodes, (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
  const MgxPoolSample s{e->d_smp_edges, e->n_pool, e->smp_seed, e->smp_offset};
  hipLaunchKernelGGL(mgx_pool_draw_kernel, dim3((unsigned)std::min(((size_t)n + 255) / 256, (size_t)2048)), dim3(256), 0, e->stream, s, (const int32_t*)st,
                     (const uint32_t*)nullptr, (int)n, (const uint32_t*)nullptr, (const uint32_t*)(st + col), (int32_t*)(st + 2 * col));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(map_index_out, st + 2 * col, (size_t)n * 4, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));   // (the arrays are the caller's)
  return MGX_OK;
}

int mgx_set_map_stats(mgx_engine* e, int32_t enabled) {
  if (!e) return fail(MGX_ERR_BAD_ARG, "mgx_set_map_stats: null engine");
  if (enabled) {   // every refusal comes before anything is touched
    if (!e->ep_stats)
      return fail(MGX_ERR_BAD_ARG, "mgx_set_map_stats: episode statistics are off (mgx_set_episode_stats): the table is built from their records");
    if (e->n_pool <= 0) return fail(MGX_ERR_BAD_ARG, "mgx_set_map_stats: no map pool (mgx_set_map_pool)");
  }
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  free_map_stats(e);
  if (!enabled) return MGX_OK;
  { int rc = e->ms_snap.create(((size_t)e->n_pool + 1) * MGX_MS_COLS * 8); if (rc) return rc; }
  // the table starts as a cleared snapshot would leave it
  { int rc = launch_map_stats_snapshot(e); if (rc) return rc; }
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->ms_on = true;
  return MGX_OK;
}

int mgx_request_map_stats(mgx_engine* e) {
  if (!e) return fail(MGX_ERR_BAD_ARG, "mgx_request_map_stats: null engine");
  if (!e->ms_on) return fail(MGX_ERR_BAD_ARG, "mgx_request_map_stats: map statistics are off (mgx_set_map_stats)");
  return e->ms_snap.request(e->device, e->stream, [e] { return launch_map_stats_snapshot(e); });
}

int mgx_fetch_map_stats(mgx_engine* e, int32_t wait, uint64_t* table, int32_t* ready) {
  if (!e || !table || !ready) return fail(MGX_ERR_BAD_ARG, "mgx_fetch_map_stats: null argument");
  *ready = 0;
  if (!e->ms_on) return fail(MGX_ERR_BAD_ARG, "mgx_fetch_map_stats: map statistics are off (mgx_set_map_stats)");
  return e->ms_snap.fetch(e->device, wait, table, ready);
}
#endif  // MGX_CPU_EMU

int mgx_set_replay(mgx_engine* e, const int32_t* envs, int32_t n_envs, int32_t words_per_env, const int32_t* static_type_ids,
                   int32_t n_static) {
  if (!e) return fail(MGX_ERR_BAD_ARG, "mgx_set_replay: null engine");
  HIP_TRY(hipSetDevice(e->device));
  if (n_envs == 0) {
    HIP_TRY(hipStreamSynchronize(e->stream));
    free_replay(e);
    return MGX_OK;
  }
#ifdef MGX_CPU_EMU
  (void)envs; (void)words_per_env; (void)static_type_ids; (void)n_static;
  return fail(MGX_ERR_BAD_ARG, "mgx_set_replay: not part of the sanitizer build");
#else
  // every refusal comes before anything is touched: a recorder that is running keeps running, its log undrained
  const MgxDev& d = e->d;
  if (n_envs < 0 || !envs || words_per_env <= 0 || n_static < 0 || (n_static > 0 && !static_type_ids))
    return fail(MGX_ERR_BAD_ARG, "mgx_set_replay: bad argument (env list, words_per_env > 0, static type ids)");
  if (e->mem_kind == MGX_MEM_HOST) return fail(MGX_ERR_BAD_ARG, "mgx_set_replay: the engine is bound to host buffers (MGX_MEM_HOST); replays need device buffers");
  std::vector<uint8_t> seen((size_t)d.E, 0);
  for (int32_t k = 0; k < n_envs; k++) {
    if (envs[k] < 0 || envs[k] >= d.E)
      return fail(MGX_ERR_BAD_ARG, "mgx_set_replay: env index " + std::to_string(envs[k]) + " out of range [0, " + std::to_string(d.E) + ")");
    if (seen[envs[k]]++) return fail(MGX_ERR_BAD_ARG, "mgx_set_replay: env " + std::to_string(envs[k]) + " listed twice");
  }
  HIP_TRY(hipStreamSynchronize(e->stream));
  free_replay(e);   // an accepted call replaces the recorder: what the old one had logged and not drained is gone
  const int nc = e->prog[MGX_H_NUM_CLASSES];
  std::vector<uint32_t> bits((size_t)(nc + 31) / 32 + 1, 0u);
  const int32_t* cls0 = e->prog.data() + mgx_sec_off(e->prog.data(), MGX_SEC_CLASSES);
  for (int c = 0; c < nc; c++)
    for (int32_t k = 0; k < n_static; k++)
      if (cls0[c * MGX_C_WORDS + MGX_C_TYPE_ID] == static_type_ids[k]) bits[c >> 5] |= 1u << (c & 31);
  const std::vector<uint32_t> st0((size_t)n_envs, (uint32_t)MGX_RPL_ENV_KEYFRAME_NEXT);
  const size_t n = (size_t)n_envs, shadow_words = n * MGX_RPL_SLOT_WORDS * (size_t)d.S;
  MgxRpl& r = e->rpl;
  hipError_t he = hipMalloc((void**)&r.envs, n * 4);
  if (he == hipSuccess) he = hipMalloc((void**)&r.log, n * (size_t)words_per_env * 4);
  if (he == hipSuccess) he = hipMalloc((void**)&r.cursor, n * 4);
  if (he == hipSuccess) he = hipMalloc((void**)&r.state, n * 4);
  if (he == hipSuccess) he = hipMalloc((void**)&r.shadow, shadow_words * 4);
  if (he == hipSuccess) he = hipMalloc((void**)&r.static_cls, bits.size() * 4);
  if (he == hipSuccess) he = hipMemcpyAsync((void*)r.envs, envs, n * 4, hipMemcpyHostToDevice, e->stream);
  if (he == hipSuccess) he = hipMemcpyAsync(r.state, st0.data(), n * 4, hipMemcpyHostToDevice, e->stream);
  if (he == hipSuccess) he = hipMemcpyAsync((void*)r.static_cls, bits.data(), bits.size() * 4, hipMemcpyHostToDevice, e->stream);
  if (he == hipSuccess) he = hipMemsetAsync(r.cursor, 0, n * 4, e->stream);
  if (he == hipSuccess) he = hipMemsetAsync(r.shadow, 0, shadow_words * 4, e->stream);
  if (he == hipSuccess) he = hipStreamSynchronize(e->stream);   // the uploads read locals
  if (he != hipSuccess) {
    free_replay(e);
    return fail(MGX_ERR_HIP, std::string("mgx_set_replay: ") + hipGetErrorString(he));
  }
  r.words_per_env = (uint32_t)words_per_env;
  e->rpl_n = n_envs;
  return MGX_OK;
#endif
}

int mgx_replay_layout(mgx_engine* e, int32_t* out) {
  if (!e || !out) return fail(MGX_ERR_BAD_ARG, "mgx_replay_layout: null argument");
  const long long max_step = (long long)MGX_RPL_STEP_WORDS + (long long)e->d.S * (1 + MGX_RPL_SLOT_WORDS) + MGX_RPL_END_WORDS;
  const int32_t v[MGX_RPL_L_COUNT] = {e->rpl_n, (int32_t)e->rpl.words_per_env, MGX_RPL_STEP_WORDS, MGX_RPL_END_WORDS, MGX_RPL_SLOT_WORDS,
                                      MGX_RPL_AMOUNT_WORDS, MGX_RPL_GROUPS, e->d.S, (int32_t)std::min<long long>(max_step, INT32_MAX)};
  memcpy(out, v, sizeof(v));
  return MGX_OK;
}

int mgx_drain_replay(mgx_engine* e, uint32_t* words_out, int32_t* n_words_out, uint32_t* flags_out) {
  if (!e || !words_out || !n_words_out) return fail(MGX_ERR_BAD_ARG, "mgx_drain_replay: null argument");
  if (!e->rpl_n) return fail(MGX_ERR_BAD_ARG, "mgx_drain_replay: no watch list (mgx_set_replay)");
  HIP_TRY(hipSetDevice(e->device));
  const size_t n = (size_t)e->rpl_n, cap = e->rpl.words_per_env;
  std::vector<uint32_t> cur(n), st(n);
  HIP_TRY(hipMemcpyAsync(cur.data(), e->rpl.cursor, n * 4, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipMemcpyAsync(st.data(), e->rpl.state, n * 4, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  for (size_t k = 0; k < n; k++) {
    const size_t used = std::min<size_t>(cur[k], cap);
    n_words_out[k] = (int32_t)used;
    if (flags_out) flags_out[k] = st[k];
    if (used) HIP_TRY(hipMemcpyAsync(words_out + k * cap, e->rpl.log + k * cap, used * 4, hipMemcpyDeviceToHost, e->stream));
    st[k] &= ~(uint32_t)MGX_RPL_ENV_OVERFLOW;
  }
  HIP_TRY(hipMemsetAsync(e->rpl.cursor, 0, n * 4, e->stream));
  HIP_TRY(hipMemcpyAsync(e->rpl.state, st.data(), n * 4, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));   // `st` is a local; the caller reads words_out
  return MGX_OK;
}

#ifndef MGX_CPU_EMU
// ---- per-step stat readout (csrc/mgx_step_stats.h) --------------------------------------------------------------------------
int mgx_set_step_stats(mgx_engine* e, const int32_t* game_cols, int32_t n_game, const int32_t* agent_cols, int32_t n_agent,
                       float* game_out, uint8_t* game_exists, float* agent_out, uint8_t* agent_exists) {
  if (!e) return fail(MGX_ERR_BAD_ARG, "mgx_set_step_stats: null engine");
  HIP_TRY(hipSetDevice(e->device));
  const MgxDev& d = e->d;
  if (n_game < 0 || n_agent < 0 || n_game > MGX_SS_MAX_COLUMNS || n_agent > MGX_SS_MAX_COLUMNS)
    return fail(MGX_ERR_BAD_ARG, "mgx_set_step_stats: at most " + std::to_string(MGX_SS_MAX_COLUMNS) + " game and " +
                                     std::to_string(MGX_SS_MAX_COLUMNS) + " agent columns (got " + std::to_string(n_game) + ", " +
                                     std::to_string(n_agent) + ")");
  if (n_game == 0 && n_agent == 0) {   // off: the step enqueues nothing for it any more
    HIP_TRY(hipStreamSynchronize(e->stream));   // (a kernel in flight still reads the column table)
    free_step_stats(e);
    return MGX_OK;
  }
  if (e->mem_kind == MGX_MEM_HOST)
    return fail(MGX_ERR_BAD_ARG, "mgx_set_step_stats: the engine is bound to host buffers (MGX_MEM_HOST); the readout needs device buffers");
  if ((n_game > 0 && (!game_cols || !game_out || !game_exists)) || (n_agent > 0 && (!agent_cols || !agent_out || !agent_exists)))
    return fail(MGX_ERR_BAD_ARG, "mgx_set_step_stats: null column list or output of a non-empty table");
  // resolve every column before anything is touched: a readout that is running keeps running when the call is refused
  uint32_t cols[2 * MGX_SS_MAX_COLUMNS];
  int32_t kinds[2 * MGX_SS_MAX_COLUMNS];
  for (int c = 0; c < n_game; c++) {
    const int id = game_cols[c];
    int kind;
    if (id == MGX_SS_ABSENT) kind = MGX_SSK_ABSENT;
    else if (id == MGX_SS_STEPS) kind = MGX_SSK_STEPS;
    else if (id >= 0 && id < d.NG) kind = MGX_SSK_STAT;
    else return fail(MGX_ERR_BAD_ARG, "mgx_set_step_stats: game column " + std::to_string(c) + ": id " + std::to_string(id) +
                                          " is neither a game stat id in [0, " + std::to_string(d.NG) + ") nor MGX_SS_ABSENT / MGX_SS_STEPS");
    kinds[c] = kind;
    cols[c] = MGX_SS_COL(kind, 0, kind == MGX_SSK_STAT ? id : 0);
  }
  // the stats this engine keeps as integers (d.shadow): ids in the order of mgx_shadow_flush_kernel's loop
  const int cnt_ids[8] = {d.wk[MGX_S_NOOP_SUCCESS], d.wk[MGX_S_NOOP_SUCCESS + 1], d.wk[MGX_S_MOVE_SUCCESS], d.wk[MGX_S_MOVE_SUCCESS + 1],
                          d.wk[MGX_S_VIBE_SUCCESS], d.wk[MGX_S_VIBE_SUCCESS + 1], d.wk[MGX_S_ACTION_FAILED], d.wk[MGX_S_MAX_STEPS_WITHOUT_MOTION]};
  for (int c = 0; c < n_agent; c++) {
    const int id = agent_cols[c];
    int kind, q = 0;
    if (id == MGX_SS_ABSENT) kind = MGX_SSK_ABSENT;
    else if (id == MGX_SS_REWARD_STEP) kind = MGX_SSK_REWARD_STEP;
    else if (id == MGX_SS_REWARD_EPISODE) kind = MGX_SSK_REWARD_EPISODE;
    else if (id >= 0 && id < d.NS) {
      kind = MGX_SSK_STAT;
      if (d.shadow & 1)
        for (int k = 0; k < 8; k++)
          if (cnt_ids[k] == id) { kind = MGX_SSK_COUNTER; q = k; }
      if (d.shadow & 2) {
        if (d.wk[MGX_S_CELL_UNIQUE] == id) kind = MGX_SSK_COV_UNIQUE;
        if (d.wk[MGX_S_CELL_MAXDIST] == id) kind = MGX_SSK_COV_MAXDIST;
      }
    } else
      return fail(MGX_ERR_BAD_ARG, "mgx_set_step_stats: agent column " + std::to_string(c) + ": id " + std::to_string(id) +
                                       " is neither an agent stat id in [0, " + std::to_string(d.NS) +
                                       ") nor MGX_SS_ABSENT / MGX_SS_REWARD_STEP / MGX_SS_REWARD_EPISODE");
    kinds[n_game + c] = kind;
    cols[n_game + c] = MGX_SS_COL(kind, q, id >= 0 ? id : 0);
  }
  if (d.NS > 0xFFFF || d.NG > 0xFFFF) return fail(MGX_ERR_BAD_ARG, "mgx_set_step_stats: stat ids do not fit a column word");
  uint32_t* dcols = nullptr;
  HIP_TRY(hipMalloc((void**)&dcols, sizeof(cols)));
  hipError_t he = hipMemcpyAsync(dcols, cols, (size_t)(n_game + n_agent) * 4, hipMemcpyHostToDevice, e->stream);
  if (he == hipSuccess) he = hipStreamSynchronize(e->stream);   // `cols` is a local; a kernel in flight still reads the old table
  if (he != hipSuccess) {
    (void)hipFree(dcols);
    return fail(MGX_ERR_HIP, std::string("mgx_set_step_stats: ") + hipGetErrorString(he));
  }
  free_step_stats(e);
  e->ss.KG = n_game; e->ss.KA = n_agent; e->ss.cols = dcols;
  e->ss.game_out = game_out; e->ss.game_exists = game_exists; e->ss.agent_out = agent_out; e->ss.agent_exists = agent_exists;
  memcpy(e->ss_kinds, kinds, (size_t)(n_game + n_agent) * sizeof(int32_t));
  e->ss_on = true;
  return MGX_OK;
}

int mgx_step_stats_columns(mgx_engine* e, int32_t* kinds_out) {
  if (!e || !kinds_out) return fail(MGX_ERR_BAD_ARG, "mgx_step_stats_columns: null argument");
  if (!e->ss_on) return fail(MGX_ERR_BAD_ARG, "mgx_step_stats_columns: no columns set (mgx_set_step_stats)");
  memcpy(kinds_out, e->ss_kinds, (size_t)(e->ss.KG + e->ss.KA) * sizeof(int32_t));
  return MGX_OK;
}

// ---- global state rows (csrc/mgx_global_state.h) ---------------------------------------------------------------------------
// Worst-case tokens of one env under a class filter: per object its class's tag bound, and for a non-static class the vibe,
// every digit of R resources and an agent's two tokens; at most min(S, H*W) objects, at most A of them agents.
static int global_state_bound(const mgx_engine* e, const uint8_t* include) {
  const MgxDev& d = e->d;
  const int nc = e->prog[MGX_H_NUM_CLASSES], digits = mgx_gs_amount_digits(d.base);
  long long agent_max = 0, other_max = 0;
  for (int c = 0; c < nc; c++) {
    if (include && !include[c]) continue;
    const uint32_t ci = e->cls_tokinfo[(size_t)c];
    const bool is_static = (ci >> 31) != 0, is_agent = (ci & 0x40000000u) != 0;
    long long n = (long long)((ci >> 24) & 0x3Fu);
    if (!is_static) n += e->prog[MGX_H_NUM_MATQ_TAGS] + 1 + (long long)d.R * digits + (is_agent ? 2 : 0);   // (+ the tags materialized queries may add)
    (is_agent ? agent_max : other_max) = std::max(is_agent ? agent_max : other_max, n);
  }
  const long long objs = std::min<long long>(d.S, (long long)d.H * d.W), agents = std::min<long long>(d.A, objs);
  const long long bound = agent_max > other_max ? agents * agent_max + (objs - agents) * other_max : objs * other_max;
  return (int)std::max<long long>(1, std::min<long long>(bound, 0x7FFFFFFF));
}

int mgx_global_state_bound(mgx_engine* e, const uint8_t* class_include, int32_t* max_tokens) {
  if (!e || !max_tokens) return fail(MGX_ERR_BAD_ARG, "mgx_global_state_bound: null argument");
  *max_tokens = global_state_bound(e, class_include);
  return MGX_OK;
}

int mgx_set_global_state(mgx_engine* e, uint32_t* tokens, int32_t max_tokens, uint32_t* counts, int32_t* agent_start,
                         const uint8_t* class_include) {
  if (!e) return fail(MGX_ERR_BAD_ARG, "mgx_set_global_state: null engine");
  HIP_TRY(hipSetDevice(e->device));
  const MgxDev& d = e->d;
  if (!tokens) {   // off: the step enqueues nothing for it any more
    HIP_TRY(hipStreamSynchronize(e->stream));   // (a kernel in flight still reads the filter and the row lengths)
    free_global_state(e);
    return MGX_OK;
  }
  if (e->mem_kind == MGX_MEM_HOST)
    return fail(MGX_ERR_BAD_ARG, "mgx_set_global_state: the engine is bound to host buffers (MGX_MEM_HOST); the rows need device buffers");
  if (max_tokens < 1) return fail(MGX_ERR_BAD_ARG, "mgx_set_global_state: the row length must be at least 1 (got " + std::to_string(max_tokens) + ")");
  if (!counts) return fail(MGX_ERR_BAD_ARG, "mgx_set_global_state: null counts");
  const size_t E = (size_t)d.E, nc = (size_t)e->prog[MGX_H_NUM_CLASSES];
  const size_t inc_off = E * 4, mask_off = (inc_off + nc + 15) & ~(size_t)15, bytes = mask_off + E;
  std::vector<uint8_t> inc(nc, 1);
  if (class_include) memcpy(inc.data(), class_include, nc);
  uint8_t* block = nullptr;
  HIP_TRY(hipMalloc((void**)&block, bytes));
  hipError_t he = hipMemsetAsync(block, 0, bytes, e->stream);   // previous row lengths 0: the rows are filled below
  if (he == hipSuccess) he = hipMemcpyAsync(block + inc_off, inc.data(), nc, hipMemcpyHostToDevice, e->stream);
  if (he == hipSuccess) he = hipMemsetAsync(tokens, 0xFF, E * (size_t)max_tokens * 4, e->stream);
  if (he == hipSuccess) he = hipStreamSynchronize(e->stream);   // `inc` is a local; a kernel in flight still reads the old block
  if (he != hipSuccess) {
    (void)hipFree(block);
    return fail(MGX_ERR_HIP, std::string("mgx_set_global_state: ") + hipGetErrorString(he));
  }
  free_global_state(e);
  e->gs.tokens = tokens; e->gs.counts = counts; e->gs.agent_start = agent_start; e->gs.TG = max_tokens;
  e->gs.n_classes = (int)nc; e->gs.n_cls_tok = (int)e->cls_tok.size();
  e->gs.used = (uint32_t*)block; e->gs.include = block + inc_off; e->d_gs_mask = block + mask_off;
  e->gs_on = true;
  return launch_global_state(e, nullptr);   // the current state
}

int mgx_write_global_state(mgx_engine* e, const uint8_t* env_mask) {
  if (!e) return fail(MGX_ERR_BAD_ARG, "mgx_write_global_state: null engine");
  if (!e->gs_on) return fail(MGX_ERR_BAD_ARG, "mgx_write_global_state: no rows set (mgx_set_global_state)");
  HIP_TRY(hipSetDevice(e->device));
  if (!env_mask) return launch_global_state(e, nullptr);
  HIP_TRY(hipStreamSynchronize(e->stream));   // (an earlier masked pass may still read the staged mask)
  HIP_TRY(hipMemcpyAsync(e->d_gs_mask, env_mask, (size_t)e->d.E, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));   // the caller's mask has been read
  return launch_global_state(e, e->d_gs_mask);
}
#endif  // MGX_CPU_EMU

int mgx_step(mgx_engine* e) {
  if (!e) return fail(MGX_ERR_BAD_ARG, "mgx_step: null engine");
  HIP_TRY(hipSetDevice(e->device));
  const MgxDev& d = e->d;
  const size_t rows = (size_t)d.E * d.A;
  e->terr_fresh = false;
  if (e->mem_kind == MGX_MEM_HOST) {
    HIP_TRY(hipMemcpyAsync(e->own_act, e->h_act, rows * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->own_vact, e->h_vact, rows * 4, hipMemcpyHostToDevice, e->stream));
  }
  if (e->auto_reset) {
    // Lazy auto-reset (mettagrid_puffer_env.py:299-302): envs found done at the end of the previous step are restarted
    // first, then stepped.  The previous step published its done count in host-visible memory; when the host has
    // already synchronised with it and nothing was done, the restart launches are skipped altogether.
    const bool known_none = e->h_flags[0] == e->step_seq && e->h_flags[1] == 0;
    if (!known_none) {
      MgxList l;
      l.list = e->d_done_list; l.n = e->d_done_n;
      // map source: the pool when there is one, else the generator (mgx_set_auto_reset refuses an engine with neither)
      const bool pool = e->n_pool > 0;
      int rrc = restart_masked(e, e->d_next_mask, pool, true, l, !pool && e->gen.kind);
      if (rrc) return rrc;
    }
  }
  // timing segments (profiling only): event k closes segment k - 1 of include/mgx.h MGX_T_*
#define MGX_MARK(k) do { if (e->profiling) HIP_TRY(hipEventRecord(e->ev[k], e->stream)); } while (0)
  MGX_MARK(0);
  {
    const int pw = e->prog_lds_words;
    if (e->world_after) HIP_TRY(hipStreamWaitEvent(e->stream, e->world_after->world_done, 0));
    MGX_TRACE_POINT(e, "before world");
    const bool x_events = d.n_schedule > 0 || (d.any_on_tick && !d.tick_in_aoe);   // what is left of the action launch behind mgx_act_kernel
    if (!d.X) {
      if (d.act_par) {
        mgx_launch_act_fast_s0(e->prog_in_lds, e->lds_act, e->stream, e->d, pw);   // (one constant-memory copy: an opt-in path)
      } else {
        if (e->jit_world.mod) { int jrc = launch_world_jit(e, pw); if (jrc) return jrc; }
        else g_world_fast[e->slot].launch(e->prog_in_lds, e->world_variant, e->lds_world, e->stream, e->d, pw);
      }
      MGX_MARK(1); MGX_MARK(2); MGX_MARK(3);
    } else if (e->aoe_kernel) {
      if (d.act_par) {
        int jrc = launch_act_x(e, pw);
        if (jrc) return jrc;
        if (x_events) launch_world_x(e, pw, MGX_PH_EVENTS);
      } else {
        launch_world_x(e, pw, MGX_PH_ACTIONS | MGX_PH_EVENTS);
      }
      MGX_TRACE_POINT(e, "world kernel (actions)");
      MGX_MARK(1);
      int trc = launch_terr(e);  // the per-agent territory effects read the ownership map
      if (trc) return trc;
      mgx_launch_aoe(e->stream, e->d, dev_copy(e), e->aoe_prog_lds ? dev_copy_hot(e) : nullptr, e->aoe_prog_lds ? e->prog_lds_words : 0);
      MGX_TRACE_POINT(e, "aoe kernel");
      MGX_MARK(2);
      if (!d.cov_in_aoe) launch_world_x(e, pw, MGX_PH_TAIL);
      else e->terr_fresh = true;   // target-local area effects move no source and change no tag: the ownership maps stay current
      MGX_MARK(3);
    } else {
      if (d.act_par) {
        int jrc = launch_act_x(e, pw);
        if (jrc) return jrc;
        launch_world_x(e, pw, MGX_PH_ALL & ~MGX_PH_ACTIONS);
      } else {
        launch_world_x(e, pw, MGX_PH_ALL);
      }
      MGX_MARK(1); MGX_MARK(2); MGX_MARK(3);
    }
    MGX_TRACE_POINT(e, "world kernel");
    if (e->world_chained) HIP_TRY(hipEventRecord(e->world_done, e->stream));
  }
  HIP_TRY(hipGetLastError());
  int rc = launch_obs(e, true);   // (+ ownership map refresh and query-backed obs values in front of it)
  if (rc) return rc;
  MGX_TRACE_POINT(e, "obs kernel");
  MGX_MARK(4);
  if (e->rewards_ext) { mgx_launch_values(e->stream, e->d, dev_copy(e), 1, nullptr); HIP_TRY(hipGetLastError()); }
  MGX_MARK(5);
#undef MGX_MARK
  if (e->profiling) e->timing_valid = true;
  if (e->ta_on) { int trc = launch_time_avg_accum(e); if (trc) return trc; }   // on_step, before the done envs are finished (simulator.py:180-190)
  if (e->auto_reset) {
    e->step_seq++;
#ifdef MGX_CPU_EMU
    const unsigned bt = 1;  // the sanitizer build runs work-items one after another: one env per workgroup
#else
    const unsigned bt = MGX_EPEND_THREADS;
#endif
    hipLaunchKernelGGL(mgx_episode_end_kernel, dim3((d.E + bt - 1) / bt), dim3(bt), 0, e->stream, dev_copy(e), (const uint32_t*)e->d_early,
                       (const uint32_t*)e->d_episodes, e->d_next_mask, e->d_counters, (volatile uint32_t*)e->h_flags_dev, e->step_seq,
                       e->d_counters + 1, e->d_done_list, e->d_done_n);
    HIP_TRY(hipGetLastError());
    if (e->ep_stats) { int erc = launch_episode_stats(e); if (erc) return erc; }
    if (e->ms_on) { int mrc = launch_map_stats(e); if (mrc) return mrc; }
    if (e->ps_on) { int prc = launch_policy_stats(e); if (prc) return prc; }
    if (e->ta_on) { int trc = launch_time_avg_finish(e); if (trc) return trc; }
  }
  if (e->rpl_n) { int prc = launch_replay(e); if (prc) return prc; }
  if (e->ss_on) { int src = launch_step_stats(e); if (src) return src; }   // (behind the episode statistics: a step that ends an episode reports its final values)
  if (e->gs_on) { int grc = launch_global_state(e, nullptr); if (grc) return grc; }   // (the restart is lazy: a finished env still shows its final state, as its observations do)
  if (e->mem_kind == MGX_MEM_HOST) {
    rc = copy_out(e, 0, (size_t)d.E);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
  }
  return MGX_OK;
}

int mgx_sync(mgx_engine* e) {
  if (!e) return fail(MGX_ERR_BAD_ARG, "mgx_sync: null engine");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return MGX_OK;
}

void* mgx_stream(mgx_engine* e) { return e ? (void*)e->stream : nullptr; }

int mgx_chain_world(mgx_engine* e, mgx_engine* after) {
  if (!e || e == after) return fail(MGX_ERR_BAD_ARG, "mgx_chain_world: needs two different engines");
  if (after && after->device != e->device) return fail(MGX_ERR_BAD_ARG, "mgx_chain_world: engines live on different devices");
  e->world_after = after;
  if (after) after->world_chained = true;
  return MGX_OK;
}

int mgx_wait_before_outputs(mgx_engine* e, void* hip_event) {
  if (!e) return fail(MGX_ERR_BAD_ARG, "mgx_wait_before_outputs: null engine");
  if (e->out_fence && hip_event && e->out_fence != (hipEvent_t)hip_event) {
    // a second consumer before the next writer: the first one's event is not dropped — the engine's stream waits for it now
    // (coarser than needed: the world update of the next step waits too)
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamWaitEvent(e->stream, e->out_fence, 0));
  }
  e->out_fence = (hipEvent_t)hip_event;
  return MGX_OK;
}

int mgx_get_buffers(mgx_engine* e, uint8_t** observations, uint8_t** terminals, uint8_t** truncations,
                    float** rewards, int32_t** actions, int32_t** vibe_actions, int32_t* mem_kind) {
  if (!e) return fail(MGX_ERR_BAD_ARG, "mgx_get_buffers: null engine");
  bool host = e->mem_kind == MGX_MEM_HOST;
  if (observations) *observations = host ? e->h_obs : e->d.obs;
  if (terminals) *terminals = host ? e->h_term : e->d.terminals;
  if (truncations) *truncations = host ? e->h_trunc : e->d.truncations;
  if (rewards) *rewards = host ? e->h_rew : e->d.rewards;
  if (actions) *actions = host ? e->h_act : (int32_t*)e->d.actions;
  if (vibe_actions) *vibe_actions = host ? e->h_vact : (int32_t*)e->d.vibe_actions;
  if (mem_kind) *mem_kind = e->mem_kind;
  return MGX_OK;
}

static int d2h(mgx_engine* e, void* dst, const void* src, size_t bytes) {
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return MGX_OK;
}

int mgx_get_episode_rewards(mgx_engine* e, float* out) {
  if (!e || !out) return fail(MGX_ERR_BAD_ARG, "mgx_get_episode_rewards: null argument");
  return d2h(e, out, e->d.episode_rewards, (size_t)e->d.E * e->d.A * 4);
}
int mgx_get_action_success(mgx_engine* e, uint8_t* out) {
  if (!e || !out) return fail(MGX_ERR_BAD_ARG, "mgx_get_action_success: null argument");
  return d2h(e, out, e->d.success, (size_t)e->d.E * e->d.A);
}
int mgx_get_executed_actions(mgx_engine* e, int32_t* out) {
  if (!e || !out) return fail(MGX_ERR_BAD_ARG, "mgx_get_executed_actions: null argument");
  return d2h(e, out, e->d.executed, (size_t)e->d.E * e->d.A * 4);
}
int mgx_invalidate_observations(mgx_engine* e) {
  if (!e) return fail(MGX_ERR_BAD_ARG, "mgx_invalidate_observations: null engine");
  HIP_TRY(hipSetDevice(e->device));
  return invalidate_obs(e);
}
int mgx_get_observation_counts(mgx_engine* e, uint16_t* out) {
  if (!e || !out) return fail(MGX_ERR_BAD_ARG, "mgx_get_observation_counts: null argument");
  const size_t rows = (size_t)e->d.E * e->d.A;
  if (!e->d.obs_used) {   // MGX_OBS_FULL_ROWS: nothing is kept
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (size_t i = 0; i < rows; i++) out[i] = 0xFFFF;
    return MGX_OK;
  }
  return d2h(e, out, e->d.obs_used, rows * 2);
}
int mgx_get_current_steps(mgx_engine* e, uint32_t* out) {
  if (!e || !out) return fail(MGX_ERR_BAD_ARG, "mgx_get_current_steps: null argument");
  return d2h(e, out, e->d.step, (size_t)e->d.E * 4);
}

int mgx_get_stats(mgx_engine* e, int32_t env, float* game_values, uint8_t* game_touched, float* agent_values,
                  uint8_t* agent_touched) {
  if (!e || env < 0 || env >= e->d.E) return fail(MGX_ERR_BAD_ARG, "mgx_get_stats: bad env");
  const MgxDev& d = e->d;
  std::vector<uint32_t> gt(d.NGW), at((size_t)d.A * d.NSW);
  int rc = flush_shadow_all(e);
  if (rc) return rc;
  rc = d2h(e, game_values, d.game_stats + (size_t)env * d.NG, (size_t)d.NG * 4);
  if (rc) return rc;
  rc = d2h(e, gt.data(), d.game_touched + (size_t)env * d.NGW, (size_t)d.NGW * 4);
  if (rc) return rc;
  {  // device rows have pitch NSP; the caller's array is [A][NS]
    std::vector<float> rows((size_t)d.A * d.NSP);
    rc = d2h(e, rows.data(), d.ag_stats + (size_t)env * d.A * d.NSP, rows.size() * 4);
    if (rc) return rc;
    for (int a = 0; a < d.A; a++) memcpy(agent_values + (size_t)a * d.NS, rows.data() + (size_t)a * d.NSP, (size_t)d.NS * 4);
  }
  rc = d2h(e, at.data(), d.ag_touched + (size_t)env * d.A * d.NSW, (size_t)d.A * d.NSW * 4);
  if (rc) return rc;
  for (int i = 0; i < d.NG; i++) game_touched[i] = ((gt[i >> 5] >> (i & 31)) & 1u) | (game_values[i] != 0.f);
  for (int a = 0; a < d.A; a++)
    for (int i = 0; i < d.NS; i++) agent_touched[(size_t)a * d.NS + i] =
          ((at[(size_t)a * d.NSW + (i >> 5)] >> (i & 31)) & 1u) | (agent_values[(size_t)a * d.NS + i] != 0.f);
  return MGX_OK;
}

int mgx_get_invalid_index_extra(mgx_engine* e, int32_t env, int32_t* k_out, float* n_out) {
  if (!e || !k_out || !n_out || env < 0 || env >= e->d.E) return fail(MGX_ERR_BAD_ARG, "mgx_get_invalid_index_extra: bad argument");
  const MgxDev& d = e->d;
  const size_t n = (size_t)d.A * MGX_INVALID_EXTRA;
  int rc = d2h(e, k_out, d.ag_invk + (size_t)env * n, n * 4);
  if (rc) return rc;
  return d2h(e, n_out, d.ag_invn + (size_t)env * n, n * 4);
}

int mgx_get_objects(mgx_engine* e, int32_t env, int32_t* out, int32_t* n_objects) {
  if (!e || !out || !n_objects || env < 0 || env >= e->d.E) return fail(MGX_ERR_BAD_ARG, "mgx_get_objects: bad argument");
  const MgxDev& d = e->d;
  const size_t S = d.S;
  std::vector<uint16_t> cls(S), rc(S), inv(S * MGX_INV_PITCH);
  std::vector<uint8_t> vibe(S), agent(S), oflags(S, 0);
  std::vector<unsigned long long> ord(S);
  std::vector<uint32_t> tags(d.obj_tags ? S * MGX_TAG_WORDS : 0);
  uint32_t n = 0;
  int r = d2h(e, &n, d.num_objs + env, 4);
  if (!r) r = d2h(e, cls.data(), d.obj_cls + env * S, S * 2);
  if (!r) r = d2h(e, rc.data(), d.obj_rc + env * S, S * 2);
  if (!r) r = d2h(e, vibe.data(), d.obj_vibe + env * S, S);
  if (!r) r = d2h(e, agent.data(), d.obj_agent + env * S, S);
  if (!r) r = d2h(e, inv.data(), d.obj_inv + env * S * MGX_INV_PITCH, S * MGX_INV_PITCH * 2);
  if (!r) r = d2h(e, ord.data(), d.obj_order + env * S, S * 8);
  if (!r && d.obj_flags) r = d2h(e, oflags.data(), d.obj_flags + env * S, S);
  if (!r && d.obj_tags) r = d2h(e, tags.data(), d.obj_tags + env * S * MGX_TAG_WORDS, S * MGX_TAG_WORDS * 4);
  if (r) return r;
  for (uint32_t s = 0; s < n; s++) {
    int32_t* w = out + (size_t)s * MGX_OBJ_RECORD_WORDS;
    w[0] = (int)s + 1; w[1] = cls[s]; w[2] = rc[s] >> 8; w[3] = rc[s] & 0xFF; w[4] = vibe[s];
    w[5] = cls[s] != MGX_DEAD_CLASS && !(oflags[s] & 1); w[6] = agent[s] == MGX_NO_AGENT ? -1 : agent[s];
    int cnt = 0;
    for (int k = 0; k < MGX_MAX_RESOURCES; k++) {
      int item = (int)((ord[s] >> (4 * k)) & 0xF);
      if (item == 0xF) { for (int q = k; q < MGX_MAX_RESOURCES; q++) w[8 + q] = -1; break; }
      w[8 + k] = item;
      cnt++;
    }
    w[7] = cnt;
    for (int k = 0; k < MGX_MAX_RESOURCES; k++) w[8 + MGX_MAX_RESOURCES + k] = k < d.R ? inv[s * MGX_INV_PITCH + k] : 0;
    for (int k = 0; k < MGX_TAG_WORDS; k++)
      w[8 + 2 * MGX_MAX_RESOURCES + k] = d.obj_tags ? (int32_t)tags[s * MGX_TAG_WORDS + k]
                                                    : (cls[s] != MGX_DEAD_CLASS ? e->prog[d.sec[MGX_SEC_CLASSES] + cls[s] * MGX_C_WORDS + MGX_C_TAGS + k] : 0);
  }
  *n_objects = (int32_t)n;
  return MGX_OK;
}

int mgx_get_objects_batch(mgx_engine* e, const int32_t* envs, int32_t n_envs, int32_t* out, int32_t* n_objects) {
  if (!e || !envs || !out || !n_objects || n_envs <= 0) return fail(MGX_ERR_BAD_ARG, "mgx_get_objects_batch: bad argument");
  const MgxDev& d = e->d;
  for (int i = 0; i < n_envs; i++)
    if (envs[i] < 0 || envs[i] >= d.E) return fail(MGX_ERR_BAD_ARG, "mgx_get_objects_batch: env index out of range");
  HIP_TRY(hipSetDevice(e->device));
  const size_t rec = (size_t)d.S * MGX_OBJ_RECORD_WORDS, n = (size_t)n_envs;
  if (n > e->objs_cap) {
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (e->d_objs) (void)hipFree(e->d_objs);
    e->d_objs = nullptr;
    e->objs_cap = 0;
    HIP_TRY(hipMalloc((void**)&e->d_objs, n * (2 + rec) * 4));
    e->objs_cap = n;
  }
  int32_t* d_envs = e->d_objs;
  int32_t* d_counts = e->d_objs + e->objs_cap;
  int32_t* d_recs = e->d_objs + 2 * e->objs_cap;
  HIP_TRY(hipMemcpyAsync(d_envs, envs, n * 4, hipMemcpyHostToDevice, e->stream));
  hipLaunchKernelGGL(mgx_objects_kernel, dim3((unsigned)n), dim3(256), 0, e->stream, dev_copy(e), (const int32_t*)d_envs, d_recs, d_counts);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(n_objects, d_counts, n * 4, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipMemcpyAsync(out, d_recs, n * rec * 4, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return MGX_OK;
}

int mgx_get_reward_state(mgx_engine* e, int32_t env, float* out) {
  if (!e || !out || env < 0 || env >= e->d.E) return fail(MGX_ERR_BAD_ARG, "mgx_get_reward_state: bad argument");
  const MgxDev& d = e->d;
  std::vector<float> prev((size_t)d.A * d.NRW);
  std::vector<uint16_t> ag_obj(d.A), cls(d.S);
  int r = d2h(e, prev.data(), d.ag_rprev + (size_t)env * d.A * d.NRW, prev.size() * 4);
  if (!r) r = d2h(e, ag_obj.data(), d.ag_obj + (size_t)env * d.A, (size_t)d.A * 2);
  if (!r) r = d2h(e, cls.data(), d.obj_cls + (size_t)env * d.S, (size_t)d.S * 2);
  if (r) return r;
  for (int a = 0; a < d.A; a++) {
    const uint16_t c = ag_obj[a] < d.S ? cls[ag_obj[a]] : (uint16_t)MGX_DEAD_CLASS;
    int n = c == MGX_DEAD_CLASS ? 0 : e->prog[d.sec[MGX_SEC_CLASSES] + c * MGX_C_WORDS + MGX_C_REWARD_COUNT];
    float t = 0.f;
    for (int k = 0; k < n; k++) t += prev[(size_t)a * d.NRW + k];
    out[a] = t;
  }
  return MGX_OK;
}

int mgx_set_inventory(mgx_engine* e, int32_t env, int32_t agent_id, const int32_t* items, const int32_t* amounts, int32_t n) {
  if (!e || env < 0 || env >= e->d.E || n < 0 || (n > 0 && (!items || !amounts)))
    return fail(MGX_ERR_BAD_ARG, "mgx_set_inventory: bad argument");
  if (agent_id < 0 || agent_id >= e->d.A) return MGX_OK;  // the reference ignores unknown agent ids (mettagrid_py.cpp:205)
  for (int i = 0; i < n; i++)
    if (items[i] < 0 || items[i] >= e->d.R || amounts[i] < 0 || amounts[i] > 65535)
      return fail(MGX_ERR_BAD_ARG, "mgx_set_inventory: resource id or amount out of range");
  HIP_TRY(hipSetDevice(e->device));
  int32_t* dbuf = nullptr;
  if (n > 0) {
    HIP_TRY(hipMalloc((void**)&dbuf, (size_t)n * 8));
    HIP_TRY(hipMemcpyAsync(dbuf, items, (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(dbuf + n, amounts, (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
  }
  hipLaunchKernelGGL(mgx_set_inventory_kernel, dim3(1), dim3(1), 0, e->stream, dev_copy(e), env, agent_id,
                     (const int32_t*)dbuf, (const int32_t*)(dbuf + n), n);
  hipError_t le = hipGetLastError();
  hipError_t se = hipStreamSynchronize(e->stream);
  if (dbuf) (void)hipFree(dbuf);
  if (le != hipSuccess || se != hipSuccess) return fail(MGX_ERR_HIP, "mgx_set_inventory: kernel failed");
  return MGX_OK;
}

int mgx_count_objects_with_tag(mgx_engine* e, int32_t env, int32_t tag_id, int32_t* out) {
  if (!e || !out || env < 0 || env >= e->d.E) return fail(MGX_ERR_BAD_ARG, "mgx_count_objects_with_tag: bad argument");
  *out = 0;
  if (tag_id < 0 || tag_id >= 256) return MGX_OK;
  const MgxDev& d = e->d;
  const size_t S = d.S;
  uint32_t n = 0;
  std::vector<uint16_t> cls(S);
  std::vector<uint8_t> oflags(S, 0);
  std::vector<uint32_t> tags(d.obj_tags ? S * MGX_TAG_WORDS : 0);
  int r = d2h(e, &n, d.num_objs + env, 4);
  if (!r) r = d2h(e, cls.data(), d.obj_cls + env * S, S * 2);
  if (!r && d.obj_flags) r = d2h(e, oflags.data(), d.obj_flags + env * S, S);
  if (!r && d.obj_tags) r = d2h(e, tags.data(), d.obj_tags + env * S * MGX_TAG_WORDS, S * MGX_TAG_WORDS * 4);
  if (r) return r;
  int count = 0;
  for (uint32_t s = 0; s < n; s++) {
    if (cls[s] == MGX_DEAD_CLASS || (oflags[s] & 1)) continue;  // removed objects are unregistered (tag_index.cpp:21-31)
    const uint32_t w = d.obj_tags ? tags[s * MGX_TAG_WORDS + (tag_id >> 5)]
                                  : (uint32_t)e->prog[d.sec[MGX_SEC_CLASSES] + cls[s] * MGX_C_WORDS + MGX_C_TAGS + (tag_id >> 5)];
    count += (w >> (tag_id & 31)) & 1u;
  }
  *out = count;
  return MGX_OK;
}

int mgx_state_digests(mgx_engine* e, uint64_t* out) {
  if (!e || !out) return fail(MGX_ERR_BAD_ARG, "mgx_state_digests: null argument");
  HIP_TRY(hipSetDevice(e->device));
  if (!e->d_digest) { int rc = e->alloc(&e->d_digest, (size_t)e->d.E); if (rc) return rc; }
  { int rc = flush_shadow_all(e); if (rc) return rc; }
  hipLaunchKernelGGL(mgx_digest_kernel, dim3((unsigned)e->d.E), dim3(MGX_WAVE), 0, e->stream, dev_copy(e), e->d_digest);
  HIP_TRY(hipGetLastError());
  return d2h(e, out, e->d_digest, (size_t)e->d.E * 8);
}

// ---- saved env state (mgx_env_state.h) ------------------------------------------------------------------------------------
static void es_info(const MgxEnvStateLayout& L, int pool_tokens, mgx_env_state_info_t* out) {
  out->record_bytes = L.record_bytes;
  out->format = L.format;
  out->version = MGX_ES_VERSION;
  out->pool_tokens = pool_tokens;
  out->n_segments = (int32_t)L.segs.size();
  out->reserved = 0;
}
int mgx_env_state_layout(const int32_t* program, size_t program_words, const uint16_t* class_maps, int32_t n_maps,
                         mgx_env_state_info_t* out) {
  if (!program || !class_maps || !out || n_maps <= 0) return fail(MGX_ERR_BAD_ARG, "mgx_env_state_layout: null/empty argument");
  MgxPlan plan;
  std::string why;
  const int rc = mgx_plan(program, program_words, class_maps, n_maps, mgx_read_switches(), plan, why);
  if (rc != MGX_OK) return fail(rc, why);
  es_info(mgx_env_state_layout_of(plan.d, program, program_words), plan.pool_tokens, out);
  return MGX_OK;
}
int mgx_env_state_info(mgx_engine* e, mgx_env_state_info_t* out) {
  if (!e || !out) return fail(MGX_ERR_BAD_ARG, "mgx_env_state_info: null argument");
  es_info(e->es, e->pool_tokens, out);
  return MGX_OK;
}
// The device segment table for the current pointers (the bound caller buffers and the lazily allocated auto-reset words
// change after mgx_create).
static int es_upload_segs(mgx_engine* e) {
  MgxDev& d = e->d;
  std::vector<MgxSeg> t;
  for (size_t i = 0; i < e->es.segs.size(); i++) {
    const MgxSegDef& s = e->es.segs[i];
    if (!s.bytes) continue;
    void* base = nullptr;
    if (s.kind != MGX_SEG_AUTO) base = *mgx_seg_ptr(d, s);
    else if (s.off == MGX_AUTO_NEXT_MASK) base = e->d_next_mask;
    else if (s.off == MGX_AUTO_EPISODES) base = e->d_episodes;
    else if (s.off == MGX_AUTO_MAP_INDEX) base = e->d_map_index;
    else base = e->d_early;
    t.push_back({(uint8_t*)base, (unsigned long long)s.bytes, (unsigned long long)e->es.offs[i], s.kind == MGX_SEG_MT ? 1 : 0, 0});
  }
  if (t.size() == e->es_segs_host.size() && memcmp(t.data(), e->es_segs_host.data(), t.size() * sizeof(MgxSeg)) == 0) return MGX_OK;
  if (!e->d_es_segs) { int rc = e->alloc(&e->d_es_segs, e->es.segs.size()); if (rc) return rc; }
  HIP_TRY(hipMemcpyAsync(e->d_es_segs, t.data(), t.size() * sizeof(MgxSeg), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));   // `t` is a local
  e->es_segs_host = t;
  return MGX_OK;
}
// Host-side checks shared by the three calls: a positive count, indices in range, no destination twice (dst_unique).
static int es_check_list(const mgx_engine* e, const int32_t* envs, int32_t n, bool dst_unique, const char* who) {
  if (!envs || n <= 0) return fail(MGX_ERR_BAD_ARG, std::string(who) + ": empty env list");
  if (e->box_dtype != MGX_BOX_OFF) return fail(MGX_ERR_BAD_ARG, std::string(who) + ": box output is on (mgx_set_box_output): states hold observation rows");
  std::vector<uint8_t> seen(dst_unique ? (size_t)e->d.E : 0, 0);
  for (int32_t k = 0; k < n; k++) {
    if (envs[k] < 0 || envs[k] >= e->d.E)
      return fail(MGX_ERR_BAD_ARG, std::string(who) + ": env index " + std::to_string(envs[k]) + " out of range [0, " + std::to_string(e->d.E) + ")");
    if (dst_unique && seen[envs[k]]++) return fail(MGX_ERR_BAD_ARG, std::string(who) + ": destination env " + std::to_string(envs[k]) + " listed twice");
  }
  return MGX_OK;
}
// Upload env lists through d_stage: [list 0 | list 1 | n], each list n int32 on a 16-byte boundary.  The host vector is
// reused only once the previous upload from it has completed (the calls return without waiting for the device).
static int es_stage_lists(mgx_engine* e, const int32_t* a, const int32_t* b, int32_t n, const int32_t** da, const int32_t** db,
                          const uint32_t** dn) {
  const size_t L = ((size_t)n * 4 + 15) & ~(size_t)15, total = 2 * L + 16;
  int rc = stage(e, total);
  if (rc) return rc;
  if (!e->es_ev) HIP_TRY(hipEventCreateWithFlags(&e->es_ev, hipEventDisableTiming));
  if (e->es_ev_pending) HIP_TRY(hipEventSynchronize(e->es_ev));
  e->es_lists.assign(total, 0);
  memcpy(e->es_lists.data(), a, (size_t)n * 4);
  if (b) memcpy(e->es_lists.data() + L, b, (size_t)n * 4);
  const uint32_t n32 = (uint32_t)n;
  memcpy(e->es_lists.data() + 2 * L, &n32, 4);
  HIP_TRY(hipMemcpyAsync(e->d_stage, e->es_lists.data(), total, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipEventRecord(e->es_ev, e->stream));
  e->es_ev_pending = true;
  const uint8_t* st = (const uint8_t*)e->d_stage;
  *da = (const int32_t*)st; *db = (const int32_t*)(st + L); *dn = (const uint32_t*)(st + 2 * L);
  return MGX_OK;
}
static void es_launch(mgx_engine* e, const int32_t* list, int32_t n, uint8_t* buf, int dir) {
  hipLaunchKernelGGL(mgx_env_state_kernel, dim3((unsigned)((n + MGX_ES_EPG - 1) / MGX_ES_EPG)), dim3(256), 0, e->stream,
                     (const MgxSeg*)e->d_es_segs, (int)e->es_segs_host.size(), list, (int)n, buf, (unsigned long long)e->es.record_bytes,
                     (unsigned long long)e->es.format, dir, e->d.E, (const uint32_t*)e->d.step, e->d.err, e->d.terr_dirty, e->d.obs_used, e->d.A);
}
// After envs were written: the auto-reset done list follows their restart-pending words; MGX_MEM_HOST: their caller rows
// go to the bound host buffers.
static int es_after_write(mgx_engine* e, const int32_t* envs, int32_t n) {
  const MgxDev& d = e->d;
  if (e->auto_reset && e->d_next_mask && e->d_done_list) {
    e->step_seq++;   // (mgx_step skips the restart launches only once this kernel has published the new count)
    hipLaunchKernelGGL(mgx_es_done_list_kernel, dim3(1), dim3(256), 0, e->stream, (const uint8_t*)e->d_next_mask, d.E, e->d_done_list,
                       e->d_done_n, (volatile uint32_t*)e->h_flags_dev, e->step_seq);
    HIP_TRY(hipGetLastError());
  }
  if (e->mem_kind == MGX_MEM_HOST) {
    int rc = copy_out_envs(e, envs, (size_t)n);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
  }
  return MGX_OK;
}
// The raw time-average accumulators of a host list of envs (csrc/mgx_time_avg.h), read (put = false) or written through the
// staged list and d_ta_block; both wait for the device.
static int ta_state(mgx_engine* e, const int32_t* envs, int32_t n, double* sums, uint32_t* steps, uint32_t* seen, bool put, const char* who) {
  if (!e || !sums || !steps || !seen) return fail(MGX_ERR_BAD_ARG, std::string(who) + ": null argument");
  if (!e->ta_on) return fail(MGX_ERR_BAD_ARG, std::string(who) + ": time averages are off (mgx_set_time_averages)");
  if (!envs || n <= 0) return fail(MGX_ERR_BAD_ARG, std::string(who) + ": empty env list");
  std::vector<uint8_t> dup(put ? (size_t)e->d.E : 0, 0);
  for (int32_t k = 0; k < n; k++) {
    if (envs[k] < 0 || envs[k] >= e->d.E)
      return fail(MGX_ERR_BAD_ARG, std::string(who) + ": env index " + std::to_string(envs[k]) + " out of range [0, " + std::to_string(e->d.E) + ")");
    if (put && dup[envs[k]]++) return fail(MGX_ERR_BAD_ARG, std::string(who) + ": env " + std::to_string(envs[k]) + " listed twice");
  }
#ifndef MGX_CPU_EMU
  HIP_TRY(hipSetDevice(e->device));
  const MgxTaLayout& L = e->ta.L;
  const size_t sb = (size_t)n * L.NG * 8, wb = (size_t)n * L.NGW * 4, tb = (size_t)n * 4;
  const int32_t *dl = nullptr, *unused = nullptr;
  const uint32_t* dn = nullptr;
  int rc = es_stage_lists(e, envs, nullptr, n, &dl, &unused, &dn);
  if (rc) return rc;
  if (put) {
    rc = reserve_time_avg_block(e, n);
    if (rc) return rc;
    if (sb) HIP_TRY(hipMemcpyAsync(e->d_ta_block, sums, sb, hipMemcpyHostToDevice, e->stream));
    if (wb) HIP_TRY(hipMemcpyAsync(e->d_ta_block + sb, seen, wb, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->d_ta_block + sb + wb, steps, tb, hipMemcpyHostToDevice, e->stream));
    rc = move_time_avg(e, dl, n, 1);
    if (rc) return rc;
  } else {
    rc = move_time_avg(e, dl, n, 0);
    if (rc) return rc;
    if (sb) HIP_TRY(hipMemcpyAsync(sums, e->d_ta_block, sb, hipMemcpyDeviceToHost, e->stream));
    if (wb) HIP_TRY(hipMemcpyAsync(seen, e->d_ta_block + sb, wb, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(steps, e->d_ta_block + sb + wb, tb, hipMemcpyDeviceToHost, e->stream));
  }
  HIP_TRY(hipStreamSynchronize(e->stream));
#endif
  return MGX_OK;
}
int mgx_get_time_average_state(mgx_engine* e, const int32_t* envs, int32_t n, double* sums, uint32_t* steps, uint32_t* seen) {
  return ta_state(e, envs, n, sums, steps, seen, false, "mgx_get_time_average_state");
}
int mgx_put_time_average_state(mgx_engine* e, const int32_t* envs, int32_t n, const double* sums, const uint32_t* steps, const uint32_t* seen) {
  return ta_state(e, envs, n, const_cast<double*>(sums), const_cast<uint32_t*>(steps), const_cast<uint32_t*>(seen), true, "mgx_put_time_average_state");
}
int mgx_save_envs(mgx_engine* e, const int32_t* envs, int32_t n, void* dst) {
  if (!e || !dst) return fail(MGX_ERR_BAD_ARG, "mgx_save_envs: null argument");
  int rc = es_check_list(e, envs, n, false, "mgx_save_envs");
  if (rc) return rc;
  HIP_TRY(hipSetDevice(e->device));
  rc = es_upload_segs(e);
  const int32_t *dl = nullptr, *unused = nullptr;
  const uint32_t* dn = nullptr;
  if (!rc) rc = es_stage_lists(e, envs, nullptr, n, &dl, &unused, &dn);
  if (!rc) rc = flush_shadow(e, dl, dn, (unsigned)(((long long)n * e->d.A + 255) / 256));   // the records' stat cells are current
  if (rc) return rc;
  es_launch(e, dl, n, (uint8_t*)dst, MGX_ES_SAVE);
  HIP_TRY(hipGetLastError());
  return MGX_OK;
}
int mgx_load_envs(mgx_engine* e, const int32_t* envs, int32_t n, const void* src, const mgx_env_state_info_t* saved) {
  if (!e || !src || !saved) return fail(MGX_ERR_BAD_ARG, "mgx_load_envs: null argument");
  if (saved->format != e->es.format || saved->record_bytes != e->es.record_bytes || saved->version != MGX_ES_VERSION) {
    char buf[160];
    snprintf(buf, sizeof buf, "mgx_load_envs: the state has format %016llx, this engine %016llx (other program, capacities or "
             "integer bookkeeping)", (unsigned long long)saved->format, (unsigned long long)e->es.format);
    return fail(MGX_ERR_BAD_ARG, buf);
  }
  int rc = es_check_list(e, envs, n, true, "mgx_load_envs");
  if (rc) return rc;
  HIP_TRY(hipSetDevice(e->device));
  rc = grow_pool(e, saved->pool_tokens);
  if (!rc) rc = es_upload_segs(e);
  if (!rc) rc = consume_out_fence(e);   // the caller rows are written
  const int32_t *dl = nullptr, *unused = nullptr;
  const uint32_t* dn = nullptr;
  if (!rc) rc = es_stage_lists(e, envs, nullptr, n, &dl, &unused, &dn);
  if (!rc) rc = mark_replay(e, dl, n, MGX_RPL_E_DISCONTINUITY);   // (before the write: the marker carries the step of the episode that ends here)
  if (rc) return rc;
  es_launch(e, dl, n, (uint8_t*)src, MGX_ES_LOAD);
  HIP_TRY(hipGetLastError());
  if (e->ta_on) { rc = clear_time_avg(e, dl, dn, n, nullptr); if (rc) return rc; }   // the record holds no accumulators: the episode is partial unless they are put back
  return es_after_write(e, envs, n);
}
int mgx_copy_envs(mgx_engine* e, const int32_t* src_envs, const int32_t* dst_envs, int32_t n) {
  if (!e) return fail(MGX_ERR_BAD_ARG, "mgx_copy_envs: null engine");
  int rc = es_check_list(e, src_envs, n, false, "mgx_copy_envs");
  if (!rc) rc = es_check_list(e, dst_envs, n, true, "mgx_copy_envs");
  if (rc) return rc;
  HIP_TRY(hipSetDevice(e->device));
  const size_t bytes = (size_t)n * (size_t)e->es.record_bytes;
  if (bytes > e->es_buf_bytes) {   // sources are saved here first: every source is read before any destination is written
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (e->d_es_buf) (void)hipFree(e->d_es_buf);
    e->d_es_buf = nullptr;
    e->es_buf_bytes = 0;
    HIP_TRY(hipMalloc((void**)&e->d_es_buf, bytes));
    e->es_buf_bytes = bytes;
  }
  rc = es_upload_segs(e);
  if (!rc) rc = consume_out_fence(e);
  const int32_t *ds = nullptr, *dd = nullptr;
  const uint32_t* dn = nullptr;
  if (!rc) rc = es_stage_lists(e, src_envs, dst_envs, n, &ds, &dd, &dn);
  if (!rc) rc = flush_shadow(e, ds, dn, (unsigned)(((long long)n * e->d.A + 255) / 256));
  if (rc) return rc;
  es_launch(e, ds, n, e->d_es_buf, MGX_ES_SAVE);
  rc = mark_replay(e, dd, n, MGX_RPL_E_DISCONTINUITY);
  if (rc) return rc;
  es_launch(e, dd, n, e->d_es_buf, MGX_ES_LOAD);
  HIP_TRY(hipGetLastError());
  if (e->ta_on) {   // a fork continues the source's average: every source is read before any destination is written
    rc = move_time_avg(e, ds, n, 0);
    if (!rc) rc = move_time_avg(e, dd, n, 1);
    if (rc) return rc;
  }
  return es_after_write(e, dst_envs, n);
}

// joint action id -> (primary, vibe) action indices (mettagrid_puffer_env.py:331-381), one thread per agent row
// ... and the range checks MettaGridPufferEnv.step makes on the host (:336-360: negative ids, ids >= num_primary * (num_vibe + 1)):
// a bad id sets a flag word in host-visible memory (bit 0 negative, bit 1 too large) — read by mgx_poll_action_errors without
// waiting for the device — and keeps the lowest offending (row, value) in device memory.
__global__ void __launch_bounds__(256) mgx_joint_actions_kernel(const int32_t* __restrict__ joint, int32_t* __restrict__ actions,
                                                                int32_t* __restrict__ vibe_actions, const int32_t* __restrict__ vibe_ids,
                                                                long long rows, int num_primary, int num_vibe,
                                                                unsigned long long* __restrict__ first_bad, uint32_t* __restrict__ host_err) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows) return;
  const int a = joint[i];
  const int max_valid = num_vibe > 0 ? num_primary + num_primary * num_vibe : num_primary;
  if (a < 0 || a >= max_valid) {
    const unsigned long long key = ((unsigned long long)i << 32) | (uint32_t)a;
    atomicMin(first_bad, key);   // the lowest bad row (fetched by the host once it has seen the flag)
    atomicOr(host_err, a < 0 ? 1u : 2u);
  }
  int core = a, vibe = 0;
  if (num_vibe > 0 && a >= num_primary) {
    const int off = a - num_primary;
    core = off / num_vibe;
    vibe = vibe_ids[off % num_vibe];
  }
  actions[i] = core;
  vibe_actions[i] = vibe;
}

int mgx_set_joint_actions(mgx_engine* e, const int32_t* joint, int32_t num_primary, const int32_t* vibe_ids, int32_t num_vibe) {
  if (!e || !joint || num_primary <= 0 || num_vibe < 0 || num_vibe > 256 || (num_vibe > 0 && !vibe_ids))
    return fail(MGX_ERR_BAD_ARG, "mgx_set_joint_actions: bad argument");
  if (e->mem_kind != MGX_MEM_DEVICE) return fail(MGX_ERR_BAD_ARG, "mgx_set_joint_actions: needs device buffers");
  HIP_TRY(hipSetDevice(e->device));
  const MgxDev& d = e->d;
  if (!e->d_vibe_ids) { int rc = e->alloc(&e->d_vibe_ids, 256); if (rc) return rc; }
  if (num_vibe > 0 && (e->n_vibe_ids != num_vibe || memcmp(e->vibe_ids_host, vibe_ids, (size_t)num_vibe * 4) != 0)) {
    memcpy(e->vibe_ids_host, vibe_ids, (size_t)num_vibe * 4);
    e->n_vibe_ids = num_vibe;
    HIP_TRY(hipMemcpyAsync(e->d_vibe_ids, e->vibe_ids_host, (size_t)num_vibe * 4, hipMemcpyHostToDevice, e->stream));
  }
  const long long rows = (long long)d.E * d.A;
  if (!e->h_act_err) {
    HIP_TRY(hipHostMalloc((void**)&e->h_act_err, 16, hipHostMallocMapped));
    memset(e->h_act_err, 0, 16);
    HIP_TRY(hipHostGetDevicePointer((void**)&e->h_act_err_dev, e->h_act_err, 0));
    int rc = e->alloc(&e->d_first_bad, 1, 0xFF);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(mgx_joint_actions_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, e->stream, joint, (int32_t*)d.actions, (int32_t*)d.vibe_actions,
                     (const int32_t*)e->d_vibe_ids, rows, num_primary, num_vibe, e->d_first_bad, e->h_act_err_dev);
  HIP_TRY(hipGetLastError());
  return MGX_OK;
}

int mgx_poll_action_errors(mgx_engine* e, int32_t wait, uint32_t* flags, int64_t* row, int32_t* value) {
  if (!e || !flags) return fail(MGX_ERR_BAD_ARG, "mgx_poll_action_errors: null argument");
  *flags = 0;
  if (!e->h_act_err) return MGX_OK;   // mgx_set_joint_actions has not run
  if (wait) { HIP_TRY(hipSetDevice(e->device)); HIP_TRY(hipStreamSynchronize(e->stream)); }
  const uint32_t f = ((volatile uint32_t*)e->h_act_err)[0];
  if (!f) return MGX_OK;
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));   // (an error is the slow path: report the lowest bad row of everything enqueued)
  *flags = ((volatile uint32_t*)e->h_act_err)[0];
  unsigned long long key = 0;
  HIP_TRY(hipMemcpy(&key, e->d_first_bad, 8, hipMemcpyDeviceToHost));
  if (row) *row = (int64_t)(key >> 32);
  if (value) *value = (int32_t)(uint32_t)key;
  memset(e->h_act_err, 0, 16);
  HIP_TRY(hipMemsetAsync(e->d_first_bad, 0xFF, 8, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return MGX_OK;
}

// e->d_scale = the caller's float[256] scale table, uploaded on the engine's stream when it differs from the last one
static int upload_scale(mgx_engine* e, const float* scale) {
  if (!e->d_scale) { int rc = e->alloc(&e->d_scale, 256); if (rc) return rc; }
  if (!e->scale_valid || memcmp(e->scale_host, scale, sizeof e->scale_host) != 0) {
    memcpy(e->scale_host, scale, sizeof e->scale_host);
    HIP_TRY(hipMemcpyAsync(e->d_scale, e->scale_host, sizeof e->scale_host, hipMemcpyHostToDevice, e->stream));
    e->scale_valid = true;
  }
  return MGX_OK;
}

int mgx_decode_obs(mgx_engine* e, const uint8_t* tokens, int64_t n_rows, float* box, int32_t num_features, const float* scale) {
  if (!e || !box || !scale || num_features < 1 || num_features > 256) return fail(MGX_ERR_BAD_ARG, "mgx_decode_obs: bad argument");
  HIP_TRY(hipSetDevice(e->device));
  const MgxDev& d = e->d;
  if (!tokens) { tokens = d.obs; n_rows = (int64_t)d.E * d.A; }
  if (n_rows <= 0) return fail(MGX_ERR_BAD_ARG, "mgx_decode_obs: no rows");
  if (int rc = upload_scale(e, scale)) return rc;
  const int rc = mgx_launch_decode(e->stream, tokens, box, e->d_scale, (long long)n_rows, d.T, num_features, e->prog[MGX_H_OBS_HEIGHT],
                                   e->prog[MGX_H_OBS_WIDTH]);
  if (rc == -1) return fail(MGX_ERR_PROGRAM, "mgx_decode_obs: the box of one agent does not fit the decode kernel's LDS");
  if (rc) return fail(MGX_ERR_HIP, "mgx_decode_obs: launch failed");
  return MGX_OK;
}

int mgx_token_bag(mgx_engine* e, const uint8_t* tokens, int64_t n_rows, void* bag, int32_t dtype, int32_t* counts, int32_t num_features,
                  const float* scale) {
  if (!e || !bag || !counts || !scale || num_features < 1 || num_features > 256 || (dtype != MGX_BOX_F32 && dtype != MGX_BOX_BF16))
    return fail(MGX_ERR_BAD_ARG, "mgx_token_bag: bad argument");
  const MgxDev& d = e->d;
  if (!tokens) {
    if (e->box_dtype != MGX_BOX_OFF) return fail(MGX_ERR_BAD_ARG, "mgx_token_bag: box output is on (mgx_set_box_output): no observation rows");
    tokens = d.obs; n_rows = (int64_t)d.E * d.A;
  }
  if (n_rows <= 0) return fail(MGX_ERR_BAD_ARG, "mgx_token_bag: no rows");
#ifdef MGX_CPU_EMU   // (wavefront-cooperative: ballot, LDS float adds)
  return fail(MGX_ERR_PROGRAM, "mgx_token_bag: the token-bag kernel is not part of the sanitizer build");
#else
  HIP_TRY(hipSetDevice(e->device));
  if (int rc = upload_scale(e, scale)) return rc;
  const int rc = mgx_launch_token_bag(e->stream, tokens, bag, dtype == MGX_BOX_BF16, counts, e->d_scale, (long long)n_rows, d.T, num_features);
  if (rc == -1) return fail(MGX_ERR_PROGRAM, "mgx_token_bag: one row's tokens and bins do not fit the kernel's LDS");
  if (rc) return fail(MGX_ERR_HIP, "mgx_token_bag: launch failed");
  return MGX_OK;
#endif
}

// ---- rendering (csrc/mgx_render.h, mgx_render.hip) ---------------------------------------------------------------------------
#ifndef MGX_CPU_EMU
// e->d_rnd_envs = the caller's env list (checked by the caller), uploaded on the engine's stream when it differs from the
// last one.
static int upload_render_envs(mgx_engine* e, const int32_t* envs, int32_t n) {
  if (e->rnd_envs_host.size() == (size_t)n && memcmp(e->rnd_envs_host.data(), envs, (size_t)n * 4) == 0) return MGX_OK;
  if (!e->rnd_ev) HIP_TRY(hipEventCreateWithFlags(&e->rnd_ev, hipEventDisableTiming));
  if (e->rnd_ev_pending) { HIP_TRY(hipEventSynchronize(e->rnd_ev)); e->rnd_ev_pending = false; }
  e->rnd_envs_host.clear();   // (whatever fails below, the next call uploads again)
  if ((size_t)n > e->rnd_envs_cap) {
    HIP_TRY(hipStreamSynchronize(e->stream));   // (a kernel in flight still reads the old list)
    if (e->d_rnd_envs) (void)hipFree(e->d_rnd_envs);
    e->d_rnd_envs = nullptr;
    e->rnd_envs_cap = 0;
    HIP_TRY(hipMalloc((void**)&e->d_rnd_envs, (size_t)n * 4));
    e->rnd_envs_cap = (size_t)n;
  }
  std::vector<int32_t> list(envs, envs + n);
  HIP_TRY(hipMemcpyAsync(e->d_rnd_envs, list.data(), (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
  e->rnd_envs_host.swap(list);   // (the upload reads this buffer: it stays as it is until rnd_ev has completed)
  HIP_TRY(hipEventRecord(e->rnd_ev, e->stream));
  e->rnd_ev_pending = true;
  return MGX_OK;
}
#endif

static int check_render_envs(const mgx_engine* e, const int32_t* envs, int32_t n, const char* who) {
  if (!envs || n < 1) return fail(MGX_ERR_BAD_ARG, std::string(who) + ": bad argument (env list, n >= 1)");
  for (int32_t k = 0; k < n; k++)
    if (envs[k] < 0 || envs[k] >= e->d.E)
      return fail(MGX_ERR_BAD_ARG, std::string(who) + ": env index " + std::to_string(envs[k]) + " out of range [0, " + std::to_string(e->d.E) + ")");
  return MGX_OK;
}

int mgx_render_cells(mgx_engine* e, const int32_t* envs, int32_t n, uint32_t* out) {
  if (!e || !out) return fail(MGX_ERR_BAD_ARG, "mgx_render_cells: null argument");
  if (int rc = check_render_envs(e, envs, n, "mgx_render_cells")) return rc;
#ifdef MGX_CPU_EMU
  return fail(MGX_ERR_PROGRAM, "mgx_render_cells: the render kernels are not part of the sanitizer build");
#else
  HIP_TRY(hipSetDevice(e->device));
  const MgxDev& d = e->d;
  const size_t words = (size_t)n * (size_t)d.H * (size_t)d.W;
  if (words > e->rnd_cells_cap) {
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (e->d_rnd_cells) (void)hipFree(e->d_rnd_cells);
    e->d_rnd_cells = nullptr;
    e->rnd_cells_cap = 0;
    HIP_TRY(hipMalloc((void**)&e->d_rnd_cells, words * 4));
    e->rnd_cells_cap = words;
  }
  if (int rc = upload_render_envs(e, envs, n)) return rc;
  const int rc = mgx_launch_render_cells(e->stream, dev_copy(e), e->d_rnd_envs, n, d.H, d.W, e->d_rnd_cells);
  if (rc == -1) return fail(MGX_ERR_BAD_ARG, "mgx_render_cells: too many envs for one launch");
  if (rc) return fail(MGX_ERR_HIP, "mgx_render_cells: launch failed");
  HIP_TRY(hipMemcpyAsync(out, e->d_rnd_cells, words * 4, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return MGX_OK;
#endif
}

int mgx_set_render_tiles(mgx_engine* e, const uint8_t* tiles, int32_t n_tiles, int32_t tile_px, const uint16_t* class_tile,
                         const uint16_t* agent_tile, const uint8_t* vibe_rgb, int32_t n_vibes) {
  if (!e) return fail(MGX_ERR_BAD_ARG, "mgx_set_render_tiles: null engine");
  HIP_TRY(hipSetDevice(e->device));
  if (!tiles) {   // off: the atlas is freed once the frames in flight are written
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (e->d_rnd_atlas) (void)hipFree(e->d_rnd_atlas);
    e->d_rnd_atlas = nullptr;
    e->rnd = MgxRenderAtlas{};
    return MGX_OK;
  }
  // every refusal comes before anything is touched: an atlas that is set stays in force
  const int nc = e->prog[MGX_H_NUM_CLASSES], A = e->d.A;
  if (n_tiles < 1 || n_tiles > 65536 || tile_px < 1 || tile_px > MGX_RENDER_MAX_TILE_PX || !class_tile || !agent_tile)
    return fail(MGX_ERR_BAD_ARG, "mgx_set_render_tiles: bad argument (1 <= n_tiles <= 65536, 1 <= tile_px <= 32, class and agent tables)");
  if (vibe_rgb && (n_vibes < 1 || n_vibes > 256)) return fail(MGX_ERR_BAD_ARG, "mgx_set_render_tiles: n_vibes must be in [1, 256]");
  for (int c = 0; c < nc; c++)
    if (class_tile[c] >= n_tiles) return fail(MGX_ERR_BAD_ARG, "mgx_set_render_tiles: class_tile[" + std::to_string(c) + "] is not a tile of the atlas");
  for (int a = 0; a < A; a++)
    if (agent_tile[a] >= n_tiles) return fail(MGX_ERR_BAD_ARG, "mgx_set_render_tiles: agent_tile[" + std::to_string(a) + "] is not a tile of the atlas");
#ifdef MGX_CPU_EMU
  return fail(MGX_ERR_PROGRAM, "mgx_set_render_tiles: the render kernels are not part of the sanitizer build");
#else
  // one block: tiles | class_tile | agent_tile | vibe_rgb (the u16 tables on an even offset)
  const size_t tile_bytes = (size_t)n_tiles * tile_px * tile_px * 3, off_cls = (tile_bytes + 15) & ~(size_t)15;
  const size_t off_ag = off_cls + (((size_t)nc * 2 + 15) & ~(size_t)15), off_vibe = off_ag + (((size_t)A * 2 + 15) & ~(size_t)15);
  std::vector<uint8_t> host(off_vibe + (vibe_rgb ? (size_t)n_vibes * 3 : 0) + 16, 0);
  memcpy(host.data(), tiles, tile_bytes);
  memcpy(host.data() + off_cls, class_tile, (size_t)nc * 2);
  memcpy(host.data() + off_ag, agent_tile, (size_t)A * 2);
  if (vibe_rgb) memcpy(host.data() + off_vibe, vibe_rgb, (size_t)n_vibes * 3);
  uint8_t* block = nullptr;
  HIP_TRY(hipMalloc((void**)&block, host.size()));
  hipError_t he = hipMemcpyAsync(block, host.data(), host.size(), hipMemcpyHostToDevice, e->stream);
  if (he == hipSuccess) he = hipStreamSynchronize(e->stream);   // `host` is a local; frames in flight read the old atlas
  if (he != hipSuccess) { (void)hipFree(block); return fail(MGX_ERR_HIP, std::string("mgx_set_render_tiles: ") + hipGetErrorString(he)); }
  if (e->d_rnd_atlas) (void)hipFree(e->d_rnd_atlas);
  e->d_rnd_atlas = block;
  e->rnd.tiles = block;
  e->rnd.class_tile = (const uint16_t*)(block + off_cls);
  e->rnd.agent_tile = (const uint16_t*)(block + off_ag);
  e->rnd.vibe_rgb = vibe_rgb ? block + off_vibe : nullptr;
  e->rnd.n_tiles = n_tiles; e->rnd.s = tile_px; e->rnd.n_vibes = vibe_rgb ? n_vibes : 0; e->rnd.n_classes = nc;
  return MGX_OK;
#endif
}

int mgx_render_rgb(mgx_engine* e, const int32_t* envs, int32_t n, uint8_t* frames) {
  if (!e || !frames) return fail(MGX_ERR_BAD_ARG, "mgx_render_rgb: null argument");
  if (int rc = check_render_envs(e, envs, n, "mgx_render_rgb")) return rc;
  if (!e->rnd.tiles) return fail(MGX_ERR_BAD_ARG, "mgx_render_rgb: no atlas (mgx_set_render_tiles)");
#ifdef MGX_CPU_EMU
  return fail(MGX_ERR_PROGRAM, "mgx_render_rgb: the render kernels are not part of the sanitizer build");
#else
  HIP_TRY(hipSetDevice(e->device));
  if (int rc = upload_render_envs(e, envs, n)) return rc;
  const int rc = mgx_launch_render_rgb(e->stream, dev_copy(e), e->rnd, e->d_rnd_envs, n, e->d.H, e->d.W, frames);
  if (rc == -1) return fail(MGX_ERR_BAD_ARG, "mgx_render_rgb: too many envs for one launch");
  if (rc) return fail(MGX_ERR_HIP, "mgx_render_rgb: launch failed");
  return MGX_OK;
#endif
}

int mgx_set_box_output(mgx_engine* e, void* box, int32_t dtype, int32_t num_features, const float* scale) {
  if (!e) return fail(MGX_ERR_BAD_ARG, "mgx_set_box_output: null engine");
  if (dtype == MGX_BOX_OFF || !box) { e->box_dtype = MGX_BOX_OFF; e->box_out = nullptr; return MGX_OK; }
  if ((dtype != MGX_BOX_F32 && dtype != MGX_BOX_BF16) || !scale || num_features < 1 || num_features > 256)
    return fail(MGX_ERR_BAD_ARG, "mgx_set_box_output: bad argument");
#ifdef MGX_CPU_EMU
  return fail(MGX_ERR_PROGRAM, "mgx_set_box_output: the observation kernel is not part of the sanitizer build");
#endif
  HIP_TRY(hipSetDevice(e->device));
  if (!e->d_scale) { int rc = e->alloc(&e->d_scale, 256); if (rc) return rc; }
  if (!e->scale_valid || memcmp(e->scale_host, scale, sizeof e->scale_host) != 0) {
    HIP_TRY(hipStreamSynchronize(e->stream));
    memcpy(e->scale_host, scale, sizeof e->scale_host);
    HIP_TRY(hipMemcpyAsync(e->d_scale, e->scale_host, sizeof e->scale_host, hipMemcpyHostToDevice, e->stream));
    e->scale_valid = true;
  }
  e->box_out = box; e->box_dtype = dtype; e->box_C = num_features;
  return MGX_OK;   // (from the next observation pass on; the box of the observations already made: mgx_decode_obs)
}

int mgx_poll_errors(mgx_engine* e, uint32_t* bits, int32_t* first_env) {
  if (!e || !bits) return fail(MGX_ERR_BAD_ARG, "mgx_poll_errors: null argument");
  std::vector<uint32_t> err(e->d.E);
  int r = d2h(e, err.data(), e->d.err, (size_t)e->d.E * 4);
  if (r) return r;
  uint32_t all = 0;
  int first = -1;
  for (int i = 0; i < e->d.E; i++) {
    if (err[i] && first < 0) first = i;
    all |= err[i];
  }
  *bits = all;
  if (first_env) *first_env = first;
  return MGX_OK;
}

int mgx_set_profiling(mgx_engine* e, int32_t enabled) {
  if (!e) return fail(MGX_ERR_BAD_ARG, "mgx_set_profiling: null engine");
  e->profiling = enabled != 0;
  e->timing_valid = false;
  return MGX_OK;
}
int mgx_get_step_timing(mgx_engine* e, float* ms_out) {
  if (!e || !ms_out) return fail(MGX_ERR_BAD_ARG, "mgx_get_step_timing: null argument");
  if (!e->profiling) return fail(MGX_ERR_BAD_ARG, "mgx_get_step_timing: profiling is off");
  if (!e->timing_valid) {  // no step since profiling was switched on: nothing recorded yet
    for (int k = 0; k < MGX_T_COUNT; k++) ms_out[k] = 0.f;
    return MGX_OK;
  }
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipEventSynchronize(e->ev[MGX_T_COUNT]));
  for (int k = 0; k < MGX_T_COUNT; k++) HIP_TRY(hipEventElapsedTime(&ms_out[k], e->ev[k], e->ev[k + 1]));
  return MGX_OK;
}

int32_t mgx_obs_variant(const mgx_engine* e) { return e ? e->obs_variant : 0; }
int32_t mgx_world_variant(const mgx_engine* e) { return !e || e->d.X || e->d.act_par ? 0 : e->jit_world.mod ? 9 : e->world_variant; }
int32_t mgx_world_shape_fields(const int32_t* program, size_t program_words, int32_t* out, int32_t capacity) {
  if (!program || !out || capacity < 0) return fail(MGX_ERR_BAD_ARG, "mgx_world_shape_fields: null argument");
  if (program_words < MGX_H_WORDS || program[MGX_H_HEIGHT] < 0 || program[MGX_H_WIDTH] < 0 || program[MGX_H_HEIGHT] > 255 || program[MGX_H_WIDTH] > 255)
    return fail(MGX_ERR_PROGRAM, "mgx_world_shape_fields: not an mgx program");
  const std::vector<uint16_t> empty_map((size_t)program[MGX_H_HEIGHT] * program[MGX_H_WIDTH] + 1, 0);   // nothing of the shape depends on the maps
  MgxPlan plan;
  std::string why;
  const int rc = mgx_plan(program, program_words, empty_map.data(), 1, mgx_read_switches(), plan, why);
  if (rc != MGX_OK) return fail(rc, why);
  int v[MGX_WORLD_SHAPE_NFIELDS];
  mgx_world_shape_of(plan.d, v);
  for (int i = 0; i < MGX_WORLD_SHAPE_NFIELDS && i < capacity; i++) out[i] = v[i];
  return MGX_WORLD_SHAPE_NFIELDS;
}
int32_t mgx_act_variant(const mgx_engine* e) { return e ? e->d.act_par : 0; }
int32_t mgx_handler_variant(const mgx_engine* e) { return e ? e->d.gen_prog : 0; }
int32_t mgx_world_prog_in_lds(const mgx_engine* e) { return e && e->prog_in_lds ? 1 : 0; }
int32_t mgx_is_extended(const mgx_engine* e) { return e && e->d.X ? 1 : 0; }
int32_t mgx_dispatch_pairs(const mgx_engine* e) { return e && e->d.duo ? 1 : 0; }
int32_t mgx_integer_bookkeeping(const mgx_engine* e) { return e ? e->d.shadow : 0; }
int32_t mgx_move_fast(const mgx_engine* e) { return e ? e->d.move_fast : 0; }
int mgx_move_fast_counts(mgx_engine* e, uint64_t* out) {
  if (!e || !out) return fail(MGX_ERR_BAD_ARG, "mgx_move_fast_counts: null argument");
  out[0] = out[1] = 0;
  if (!e->d.mf_count) return MGX_OK;
  std::vector<uint32_t> h((size_t)e->d.E * 2);
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipMemcpyAsync(h.data(), e->d.mf_count, h.size() * 4, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  for (size_t i = 0; i < h.size(); i += 2) { out[0] += h[i]; out[1] += h[i + 1]; }
  return MGX_OK;
}
int32_t mgx_create_paths(const mgx_engine* e) {
  if (!e) return 0;
  const MgxDev& d = e->d;
  int32_t p = 0;
  auto set = [&](int bit, bool on) { if (on) p |= bit; };
  set(MGX_PATH_X, d.X != 0);
  set(MGX_PATH_PROG_LDS, e->prog_in_lds);
  set(MGX_PATH_AOE_LOCAL, e->aoe_kernel);
  set(MGX_PATH_TICK_IN_AOE, d.tick_in_aoe != 0);
  set(MGX_PATH_COV_IN_AOE, d.cov_in_aoe != 0);
  set(MGX_PATH_AOE_PROG_LDS, e->aoe_prog_lds);
  set(MGX_PATH_X_AOE_LDS, d.x_aoe_lds != 0);
  set(MGX_PATH_FLAT_TOP, d.flat_top != 0);
  set(MGX_PATH_TICK_SPLIT, d.tick_split != 0);
  set(MGX_PATH_ACT_PAR, d.act_par != 0);
  set(MGX_PATH_DUO, d.duo != 0);
  set(MGX_PATH_ACT_MAP, d.act_map != 0);
  set(MGX_PATH_SHADOW, d.shadow != 0);
  set(MGX_PATH_REWARDS_EARLY, e->rmode == 1);
  set(MGX_PATH_REWARDS_MID, e->rmode == 2);
  set(MGX_PATH_REWARDS_EXT, e->rewards_ext);
  set(MGX_PATH_OBS_512, e->obs_threads == 512);
  set(MGX_PATH_WORLD_LDS_64K, e->lds_world > 64 * 1024);
  set(MGX_PATH_GEN, d.gen_prog != 0);
  return p;
}
int32_t mgx_num_envs(const mgx_engine* e) { return e ? e->d.E : 0; }
int32_t mgx_num_agents(const mgx_engine* e) { return e ? e->d.A : 0; }
int32_t mgx_num_tokens(const mgx_engine* e) { return e ? e->d.T : 0; }
int64_t mgx_state_bytes(const mgx_engine* e) { return e ? e->state_bytes : 0; }

}  // extern "C"

#ifdef MGX_WORLD_TIMING  // instrumented developer build only (scripts/world_timing.py); not part of the ABI
extern "C" void mgx_debug_obs_cycles(unsigned long long* out, int reset) { (void)mgx_read_cycles(&mgx_dbg_cycles, out, reset); }
#endif
