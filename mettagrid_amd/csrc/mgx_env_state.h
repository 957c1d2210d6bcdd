// mgx_env_state.h — what one env's state is, and the kernel that saves, loads and copies it (mgx_save_envs / mgx_load_envs /
// mgx_copy_envs, include/mgx.h).  Included by mgx_engine.hip.
//
// ONE list, mgx_env_segments(), names every per-env array of MgxDev that an episode owns, with its bytes per env and the
// value a fresh allocation holds.  mgx_create allocates the env-major state arrays by walking it (so the restart table
// rows_state is this list too), and the record layout of a saved env is laid out from it.  The host half makes no HIP call:
// mgx_env_state_layout() runs it on the planner's result alone.  What is deliberately NOT in the list (derived or transient
// arrays, slot-owned arrays) is tabled in DESIGN.md "Env state".
//
// A record (one env): the header of include/mgx_program.h (MGX_ES_*), then every segment of the list at a 16-byte aligned
// offset.
// The format word (mgx_env_state_layout_of) hashes the program words, the list of (kind, bytes) of every segment — which
// carries every create-time capacity — and d.shadow, the one create path that changes what a state array holds.
#ifndef MGX_ENV_STATE_H_
#define MGX_ENV_STATE_H_

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "mgx.h"
#include "mgx_device.h"

#define MGX_ES_EPG 16              // envs per workgroup of mgx_env_state_kernel

// kinds of segment
enum {
  MGX_SEG_ROW = 0,     // env-major state array that an episode restart refills (mgx_engine::rows_state)
  MGX_SEG_WORD = 1,    // env-major array a restart does not touch: step, err, mt_idx
  MGX_SEG_MT = 2,      // the env-minor Mersenne-Twister state [624][E]: one word per env every E words
  MGX_SEG_CALLER = 3,  // caller-visible row of the env in the bound buffers: observations, rewards, terminals, truncations
  MGX_SEG_AUTO = 4,    // auto-reset word of the engine (allocated lazily; zero in a record when the engine has none)
};
// the auto-reset words, in record order (MgxSegDef::off of an MGX_SEG_AUTO segment)
enum { MGX_AUTO_NEXT_MASK = 0, MGX_AUTO_EPISODES, MGX_AUTO_MAP_INDEX, MGX_AUTO_EARLY };

struct MgxSegDef {
  size_t off;        // offsetof(MgxDev, <pointer>) — or MGX_AUTO_* of an MGX_SEG_AUTO segment
  uint32_t bytes;    // per env
  uint8_t fill;      // byte a fresh allocation and a restart write (MGX_SEG_ROW)
  uint8_t kind;
};

// Every per-env array that an episode owns, in record order.  `d` is the planner's MgxDev (capacities and paths set, no
// pointers); P the program.
inline std::vector<MgxSegDef> mgx_env_segments(const MgxDev& d, const int32_t* P) {
  std::vector<MgxSegDef> s;
  const uint32_t HW = (uint32_t)(d.H * d.W), S = (uint32_t)d.S, A = (uint32_t)d.A;
  auto row = [&](size_t off, uint32_t bytes, int fill = 0) { s.push_back({off, bytes, (uint8_t)fill, (uint8_t)MGX_SEG_ROW}); };
#define MGX_SEG(f, bytes, ...) row(offsetof(MgxDev, f), (uint32_t)(bytes), ##__VA_ARGS__)
  MGX_SEG(grid, HW * 2);
  MGX_SEG(obj_cls, S * 2, 0xFF);
  MGX_SEG(obj_rc, S * 2);
  MGX_SEG(obj_vibe, S);
  MGX_SEG(obj_agent, S, 0xFF);
  MGX_SEG(obj_visited, S * 4);
  MGX_SEG(obj_inv, S * MGX_INV_PITCH * 2);
  MGX_SEG(obj_order, S * 8, 0xFF);
  MGX_SEG(num_objs, 4);
  MGX_SEG(ag_obj, A * 2);
  MGX_SEG(ag_prev, A * 2);
  MGX_SEG(ag_spawn, A * 2);
  MGX_SEG(ag_rc, A * 2);
  MGX_SEG(ag_rwinfo, A * 4);
  MGX_SEG(ag_cls, A * 2);
  MGX_SEG(ag_stepprev, A * 2);
  MGX_SEG(ag_covrc, A * 2, 0xFF);
  MGX_SEG(ag_invk, A * MGX_INVALID_EXTRA * 4);
  MGX_SEG(ag_invn, A * MGX_INVALID_EXTRA * 4);
  MGX_SEG(ag_swm, A * 4);
  MGX_SEG(ag_cnt, A * 8 * 4);
  MGX_SEG(ag_maxdist, A * 4);
  MGX_SEG(ag_unique, A * 4);
  MGX_SEG(ag_seen, A * d.SEENW * 4);
  MGX_SEG(ag_rprev, A * d.NRW * 4);
  MGX_SEG(ag_stats, A * d.NSP * 4);
  MGX_SEG(ag_touched, A * d.NSW * 4);
  MGX_SEG(game_stats, d.NG * 4);
  MGX_SEG(game_touched, d.NGW * 4);
  MGX_SEG(executed, A * 4);
  MGX_SEG(success, A);
  MGX_SEG(episode_rewards, A * 4);
  if (d.X) {
    if (P[MGX_H_DYNAMIC_TAGS]) MGX_SEG(obj_tags, S * MGX_TAG_WORDS * 4);
    if (d.NL) { MGX_SEG(tl_items, d.NL * S * 2); MGX_SEG(tl_count, d.NL * 2); }
    if (d.NF) { MGX_SEG(fx_obj, d.NF * 2); MGX_SEG(fx_aoe, d.NF * 2); MGX_SEG(fx_rc, d.NF * 2); MGX_SEG(fx_inside, A * d.FW * 4); MGX_SEG(fx_count, 2); }
    if (d.NM) { MGX_SEG(mb_obj, d.NM * 2); MGX_SEG(mb_aoe, d.NM * 2); MGX_SEG(mb_inside, A * d.MW * 4); MGX_SEG(mb_count, 2); }
    if (d.NTS) { MGX_SEG(ts_obj, d.NTS * 2); MGX_SEG(ts_ctrl, d.NTS * 2); MGX_SEG(ts_rc, d.NTS * 2); MGX_SEG(ts_count, 2); }
    MGX_SEG(terr_prev, A * (d.NT > 0 ? d.NT : 1) * 2);
    if (d.NT > 0 && d.NTS > 0) MGX_SEG(terr_dirty, 1, 1);   // (terr_owner, its cache, is derived: a load sets this byte)
    MGX_SEG(next_event, 4);
    MGX_SEG(obj_flags, S);
    if (P[MGX_H_SPAWNS]) { MGX_SEG(def_aoe, S * 2); MGX_SEG(def_count, 2); }
  }
#undef MGX_SEG
  s.push_back({offsetof(MgxDev, step), 4, 0, (uint8_t)MGX_SEG_WORD});
  s.push_back({offsetof(MgxDev, err), 4, 0, (uint8_t)MGX_SEG_WORD});
  s.push_back({offsetof(MgxDev, mt_idx), 4, 0, (uint8_t)MGX_SEG_WORD});
  s.push_back({offsetof(MgxDev, mt), 624 * 4, 0, (uint8_t)MGX_SEG_MT});
  s.push_back({offsetof(MgxDev, obs), A * (uint32_t)d.T * 3, 0xFF, (uint8_t)MGX_SEG_CALLER});
  s.push_back({offsetof(MgxDev, rewards), A * 4, 0, (uint8_t)MGX_SEG_CALLER});
  s.push_back({offsetof(MgxDev, terminals), A, 0, (uint8_t)MGX_SEG_CALLER});
  s.push_back({offsetof(MgxDev, truncations), A, 0, (uint8_t)MGX_SEG_CALLER});
  s.push_back({MGX_AUTO_NEXT_MASK, 1, 0, (uint8_t)MGX_SEG_AUTO});
  s.push_back({MGX_AUTO_EPISODES, 4, 0, (uint8_t)MGX_SEG_AUTO});
  s.push_back({MGX_AUTO_MAP_INDEX, 4, 0, (uint8_t)MGX_SEG_AUTO});
  s.push_back({MGX_AUTO_EARLY, 4, 0, (uint8_t)MGX_SEG_AUTO});
  return s;
}
// where a segment's pointer lives in an MgxDev (not for MGX_SEG_AUTO)
inline void** mgx_seg_ptr(MgxDev& d, const MgxSegDef& s) { return (void**)((char*)&d + s.off); }

// The layout of a record: offset of every segment (0 for an empty one) and the record size.
struct MgxEnvStateLayout {
  std::vector<MgxSegDef> segs;
  std::vector<uint64_t> offs;
  int64_t record_bytes = 0;
  uint64_t format = 0;
};
inline uint64_t mgx_es_fnv(uint64_t h, uint32_t w) { return (h ^ (uint64_t)w) * 1099511628211ull; }
inline MgxEnvStateLayout mgx_env_state_layout_of(const MgxDev& d, const int32_t* P, size_t program_words) {
  MgxEnvStateLayout L;
  L.segs = mgx_env_segments(d, P);
  uint64_t off = MGX_ES_HEADER_BYTES;
  uint64_t h = 14695981039346656037ull;
  h = mgx_es_fnv(h, MGX_ES_VERSION);
  for (size_t i = 0; i < program_words; i++) h = mgx_es_fnv(h, (uint32_t)P[i]);
  for (const MgxSegDef& s : L.segs) {
    L.offs.push_back(s.bytes ? off : 0);
    off += (s.bytes + (MGX_ES_ALIGN - 1)) & ~(uint64_t)(MGX_ES_ALIGN - 1);
    h = mgx_es_fnv(h, s.kind);
    h = mgx_es_fnv(h, s.bytes);
  }
  h = mgx_es_fnv(h, (uint32_t)d.shadow);   // the integer bookkeeping in ag_cnt, flushed into the stat cells (mgx_episode.h)
  L.record_bytes = (int64_t)off;
  L.format = h;
  return L;
}

// ---- device side ------------------------------------------------------------------------------------------------------------
// One entry of the device segment table: env-major (row at base + env * bytes) or env-minor (word k at base[k * E + env]).
struct MgxSeg {
  uint8_t* base;                // nullptr: the engine has no such array (auto-reset words): zeros are saved, nothing is loaded
  unsigned long long bytes;     // per env
  unsigned long long rec_off;   // offset in the record
  int minor;                    // 1: env-minor words (stride E)
  int pad;
};
enum { MGX_ES_SAVE = 0, MGX_ES_LOAD = 1 };

// `n` bytes from `src` to `dst`: 16-byte moves when both ends and the size allow them, else dwords, else bytes; the lanes
// of one wavefront share the work (lane, nl: index and count of the sharing lanes).
__device__ __forceinline__ void mgx_es_move(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, size_t n, int lane, int nl) {
  const uintptr_t a = (uintptr_t)dst | (uintptr_t)src | (uintptr_t)n;
  if ((a & 15) == 0) {
    uint4* d16 = (uint4*)dst;
    const uint4* s16 = (const uint4*)src;
    const size_t n16 = n / 16;
    size_t i = (size_t)lane;
    for (; i + 3 * (size_t)nl < n16; i += 4 * (size_t)nl) {   // four independent loads in flight per lane
      const uint4 v0 = s16[i], v1 = s16[i + nl], v2 = s16[i + 2 * nl], v3 = s16[i + 3 * nl];
      d16[i] = v0; d16[i + nl] = v1; d16[i + 2 * nl] = v2; d16[i + 3 * nl] = v3;
    }
    for (; i < n16; i += (size_t)nl) d16[i] = s16[i];
  } else if ((a & 3) == 0) {
    for (size_t i = (size_t)lane; i < n / 4; i += (size_t)nl) ((uint32_t*)dst)[i] = ((const uint32_t*)src)[i];
  } else {
    for (size_t i = (size_t)lane; i < n; i += (size_t)nl) dst[i] = src[i];
  }
}
__device__ __forceinline__ bool mgx_es_header_ok(const uint8_t* rec, unsigned long long format) {
  const uint32_t* h = (const uint32_t*)rec;
  return h[0] == (uint32_t)MGX_ES_MAGIC && h[1] == MGX_ES_VERSION && (((unsigned long long)h[3] << 32) | h[2]) == format;
}

// Save (records <- envs) or load (envs <- records) the envs of a device list: record k belongs to env list[k].  A workgroup
// of 256 work-items takes MGX_ES_EPG consecutive list entries: each wavefront the env-major segments of every fourth of
// them (the lanes share each row), then all work-items the env-minor segment (consecutive envs of the list in consecutive
// lanes: with an ascending list each access of a wavefront is 4 runs of 64 bytes).
// Load checks each record's header first: a record of another layout leaves its env untouched and sets MGX_ENV_BAD_STATE.
// A loaded env's territory ownership map is marked for a rebuild (terr_dirty), and the token counts of its observation rows
// (obs_used, MgxDev::obs_used: not part of a record) become unknown: the rows now hold another env's tokens.
__global__ void __launch_bounds__(256) mgx_env_state_kernel(const MgxSeg* __restrict__ segs, int n_segs, const int32_t* __restrict__ list,
                                                            int n, uint8_t* __restrict__ buf, unsigned long long record_bytes,
                                                            unsigned long long format, int dir, int E, const uint32_t* __restrict__ step,
                                                            uint32_t* __restrict__ err, uint8_t* __restrict__ terr_dirty, uint16_t* __restrict__ obs_used,
                                                            int A) {
  const int k0 = (int)blockIdx.x * MGX_ES_EPG;
  const int wave = (int)threadIdx.x / MGX_WAVE, lane = (int)threadIdx.x & (MGX_WAVE - 1), NWV = (int)blockDim.x / MGX_WAVE;
  for (int q = wave; q < MGX_ES_EPG && k0 + q < n; q += NWV) {
    const int k = k0 + q, env = list[k];
    uint8_t* rec = buf + (size_t)k * record_bytes;
    if (dir == MGX_ES_LOAD && !mgx_es_header_ok(rec, format)) {
      if (lane == 0) err[env] |= MGX_ENV_BAD_STATE;
      continue;
    }
    if (dir == MGX_ES_SAVE && lane == 0) {
      uint32_t* h = (uint32_t*)rec;
      h[0] = (uint32_t)MGX_ES_MAGIC; h[1] = MGX_ES_VERSION; h[2] = (uint32_t)format; h[3] = (uint32_t)(format >> 32);
      h[4] = step[env]; h[5] = (uint32_t)env; h[6] = (uint32_t)record_bytes; h[7] = 0;
    }
    for (int s = 0; s < n_segs; s++) {
      const MgxSeg g = segs[s];
      if (g.minor) continue;
      uint8_t* r = rec + g.rec_off;
      if (!g.base) {   // an auto-reset word the engine does not have: zeros in the record, nothing to load
        if (dir == MGX_ES_SAVE) for (size_t i = (size_t)lane; i < g.bytes; i += MGX_WAVE) r[i] = 0;
        continue;
      }
      uint8_t* row = g.base + (size_t)env * g.bytes;
      if (dir == MGX_ES_SAVE) mgx_es_move(r, row, g.bytes, lane, MGX_WAVE);
      else mgx_es_move(row, r, g.bytes, lane, MGX_WAVE);
    }
    if (dir == MGX_ES_LOAD && terr_dirty && lane == 0) terr_dirty[env] = 1;   // (after this lane's own copy of the byte)
    if (dir == MGX_ES_LOAD && obs_used)
      for (int a = lane; a < A; a += MGX_WAVE) obs_used[(size_t)env * A + a] = 0xFFFF;
  }
  // env-minor segments: work-item t moves words t / EPG, t / EPG + 256 / EPG, ... of env list[k0 + t % EPG]
  const int q = (int)threadIdx.x % MGX_ES_EPG, k = k0 + q;
  if (k >= n) return;
  const int env = list[k];
  uint8_t* rec = buf + (size_t)k * record_bytes;
  if (dir == MGX_ES_LOAD && !mgx_es_header_ok(rec, format)) return;
  for (int s = 0; s < n_segs; s++) {
    const MgxSeg g = segs[s];
    if (!g.minor) continue;
    uint32_t* r = (uint32_t*)(rec + g.rec_off);
    uint32_t* base = (uint32_t*)g.base;
    for (int w = (int)threadIdx.x / MGX_ES_EPG; w < (int)(g.bytes / 4); w += (int)blockDim.x / MGX_ES_EPG) {
      if (dir == MGX_ES_SAVE) r[w] = base[(size_t)w * E + env];
      else base[(size_t)w * E + env] = r[w];
    }
  }
}

// Auto-reset engines after a load / copy: the envs whose restart is pending (next_mask) listed in ascending order, their count
// in done_n and in the host-visible flags with the sequence number `seq` (what mgx_episode_end_kernel leaves behind a step).
// One workgroup: work-item t counts a contiguous chunk, a scan over the workgroup places it.
__global__ void __launch_bounds__(256) mgx_es_done_list_kernel(const uint8_t* __restrict__ next_mask, int E, int32_t* __restrict__ done_list,
                                                               uint32_t* __restrict__ done_n, volatile uint32_t* host_flags, uint32_t seq) {
#ifdef MGX_CPU_EMU
  // (the sanitizer build runs work-items one after another: one of them lists, serially)
  if (threadIdx.x != 0) return;
  uint32_t m = 0;
  for (int i = 0; i < E; i++) if (next_mask[i]) done_list[m++] = i;
  *done_n = m;
  host_flags[1] = m;
  host_flags[0] = seq;
  return;
#endif
  __shared__ uint32_t cnt[256];
  const int t = (int)threadIdx.x, per = (E + 255) / 256, first = t * per;
  uint32_t c = 0;
  for (int i = first; i < first + per && i < E; i++) c += next_mask[i] ? 1u : 0u;
  cnt[t] = c;
  __syncthreads();
  if (t == 0) {   // (256 entries, once per load)
    uint32_t run = 0;
    for (int i = 0; i < 256; i++) { const uint32_t v = cnt[i]; cnt[i] = run; run += v; }
    *done_n = run;
    host_flags[1] = run;
    __threadfence_system();
    host_flags[0] = seq;
  }
  __syncthreads();
  uint32_t o = cnt[t];
  for (int i = first; i < first + per && i < E; i++) if (next_mask[i]) done_list[o++] = i;
}

#endif  // MGX_ENV_STATE_H_
