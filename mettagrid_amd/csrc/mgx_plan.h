// mgx_plan.h — the host-only half of mgx_create: validates a program and chooses every code path, capacity and LDS layout
// of an engine from the program, the class maps, the env count and the create-time switches.  No HIP call is made here,
// so a program is refused before a stream exists or memory is allocated.  Included by mgx_engine.hip.
#ifndef MGX_PLAN_H_
#define MGX_PLAN_H_

#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

#include "mgx.h"
#include "mgx_device.h"
#include "mgx_obs.h"
#include "mgx_world.h"
#include "mgx_host.h"   // the kernel units' sizes and host analyses, mgx_pow2_at_least
#include "mgx_aoe_local.h"
#include "mgx_presets_gen.h"
#include "mgx_handlers_fp.h"

// The environment switches that choose create-time paths (tests/test_gpu_paths.py), read once by mgx_create and kept for
// the engine's lifetime: a later reset that grows the token pool sizes the observation kernel with the same ones.
struct MgxSwitches {   // (mgx_read_switches: which switch sets or clears each)
  bool verbose, prog_lds, aoe_local, tick_in_aoe, aoe_prog_lds, flat_top, tick_split, rewards_mid, obs_512, obs_preset, act_lean,
      act_par, act_map, act_replay, duo, coop_passes, move_fast, move_fast_count, mf_serial_book, shadow, gen, obs_tail, world_preset;
};
inline MgxSwitches mgx_read_switches() {
  auto on = [](const char* name) { return getenv(name) != nullptr; };
  const char* prog_lds = getenv("MGX_PROG_LDS");
  MgxSwitches s;
  s.verbose = on("MGX_VERBOSE");                    // report the chosen paths on stderr
  s.prog_lds = !prog_lds || atoi(prog_lds) != 0;    // 0: the world kernels read the program from HBM
  s.aoe_local = !on("MGX_AOE_SERIAL");              // area effects in the world kernel, one lane per env
  s.tick_in_aoe = !on("MGX_TICK_SERIAL");           // on_tick handlers and coverage stay out of the area-effect kernel
  s.aoe_prog_lds = !on("MGX_AOE_PROG_HBM");         // the area-effect kernel reads the program from HBM
  s.flat_top = !on("MGX_NO_FLAT_TOP");              // action-phase handlers on the LDS VM
  s.tick_split = !on("MGX_NO_TICK_SPLIT");
  s.rewards_mid = !on("MGX_REWARDS_LATE");          // extended games evaluate rewards at the observation kernel's end
  s.obs_512 = !on("MGX_OBS_256");
  s.obs_preset = !on("MGX_OBS_GENERIC");            // no preset instance of the observation kernel
  s.act_lean = on("MGX_ACT_LEAN");                  // lean games may take the lane-per-agent dispatch too
  s.act_par = !on("MGX_ACT_SERIAL");                // action dispatch one lane per env
  s.act_map = !on("MGX_ACT_NO_MAP");                // conflicts by an all-pairs walk
  s.act_replay = on("MGX_ACT_SHUFFLE_REPLAY");      // the shuffle always takes its serial replay path (tests)
  s.duo = !on("MGX_NO_DUO");
  s.coop_passes = !on("MGX_WORLD_PASSES_PER_ENV");  // the lean kernel's batched per-agent passes one lane per env
  s.move_fast = !on("MGX_NO_MOVE_FAST");            // the lean kernel resolves no move target up front: every action takes the trip loop
  s.move_fast_count = on("MGX_MOVE_FAST_COUNT");    // ... and counts run-ahead actions and stale entries per env (tests)
  s.mf_serial_book = on("MGX_MF_SERIAL_BOOK");      // ... with the run-ahead's first form: one agent at a time, bookkeeping inside (the A/B switch)
  s.shadow = !on("MGX_NO_SHADOW");                  // no integer bookkeeping
  s.gen = !on("MGX_NO_GEN");                        // handlers on the interpreter
  s.obs_tail = !on("MGX_OBS_FULL_ROWS");            // every observation pass rewrites whole rows (no MgxDev::obs_used)
  s.world_preset = !on("MGX_WORLD_GENERIC");        // no preset instance of the lean world kernel (the A/B switch on one binary)
#ifdef MGX_CPU_EMU
  // the sanitizer build runs work-items one by one: no LDS program copies (they need a workgroup barrier), no flush kernel
  // for the integer bookkeeping, no wavefront-cooperative (ballot / readlane) lane-per-agent dispatch
  s.prog_lds = s.aoe_prog_lds = s.shadow = s.act_par = false;
  s.move_fast = false;   // (like coop_passes it needs the helper lanes of the GPU build)
#endif
  return s;
}

// Does any instruction of the game-value code [start, start + count) satisfy `pred`?
template <class F>
inline bool mgx_gv_any(const int32_t* P, int start, int count, F&& pred) {
  const int32_t* code = P + mgx_sec_off(P, MGX_SEC_GV_CODE);
  for (int i = start; i < start + count; i++)
    if (pred(code + i * MGX_GV_WORDS)) return true;
  return false;
}
// ... of game value record `rec` (MGX_SEC_OBS_VALUES; none: false, past the section: true)
template <class F>
inline bool mgx_value_any(const int32_t* P, int rec, F&& pred) {
  if (rec < 0) return false;
  if (rec >= mgx_sec_cnt(P, MGX_SEC_OBS_VALUES)) return true;
  const int32_t* V = P + mgx_sec_off(P, MGX_SEC_OBS_VALUES) + rec * MGX_OV_WORDS;
  return mgx_gv_any(P, V[MGX_OV_GV_START], V[MGX_OV_GV_COUNT], pred);
}
// ... of any reward expression
template <class F>
inline bool mgx_rewards_any(const int32_t* P, F&& pred) {
  const int32_t* rw = P + mgx_sec_off(P, MGX_SEC_REWARDS);
  for (int k = 0; k < mgx_sec_cnt(P, MGX_SEC_REWARDS); k++)
    if (mgx_gv_any(P, rw[k * MGX_RW_WORDS + MGX_RW_GV_START], rw[k * MGX_RW_WORDS + MGX_RW_GV_COUNT], pred)) return true;
  return false;
}
inline bool mgx_gv_query(const int32_t* g) { return g[MGX_GV_OP] == MGX_GOP_QUERY_INVENTORY || g[MGX_GV_OP] == MGX_GOP_QUERY_COUNT; }
inline bool mgx_gv_agent_stat(const int32_t* g) { return g[MGX_GV_OP] == MGX_GOP_STAT && g[MGX_GV_A0] != 1; }

// The handlers reachable from `roots` (children of non-leaf handlers, filter DAGs of leaves): mut_ok is asked about every
// mutation of a reached leaf, atom_ok about every atom of its filter; the walk stops at the first refusal.
struct MgxReach {
  bool ok = true;
  std::vector<const int32_t*> muts;   // mutation records of the reached leaves, in walk order
  bool uses_target() const {           // UseTarget applies the target's on_use / the actor's on_after_use
    for (const int32_t* m : muts) if (m[MGX_MU_OP] == MGX_MOP_USE_TARGET) return true;
    return false;
  }
  std::vector<int> game_sets() const {  // game-scope stats a StatsMutation SETs, in the order first reached
    std::vector<int> ids;
    for (const int32_t* m : muts)
      if (m[MGX_MU_OP] == MGX_MOP_STATS && m[MGX_MU_A0] == 0 && std::find(ids.begin(), ids.end(), m[MGX_MU_A2]) == ids.end())
        ids.push_back(m[MGX_MU_A2]);
    return ids;
  }
};
template <class M, class F>
inline MgxReach mgx_reach(const int32_t* P, const std::vector<int>& roots, M&& mut_ok, F&& atom_ok) {
  const int n_hd = mgx_sec_cnt(P, MGX_SEC_HANDLERS), n_atoms = mgx_sec_cnt(P, MGX_SEC_ATOMS);
  MgxReach r;
  std::vector<char> hseen(n_hd, 0);
  std::vector<int> stack;
  auto push = [&](int h) { if (h >= 0 && h < n_hd && !hseen[h]) { hseen[h] = 1; stack.push_back(h); } };
  for (int h : roots) push(h);
  while (!stack.empty() && r.ok) {
    const int32_t* hd = P + mgx_sec_off(P, MGX_SEC_HANDLERS) + stack.back() * MGX_HD_WORDS;
    stack.pop_back();
    if (hd[MGX_HD_KIND] != MGX_HK_LEAF) {
      const int32_t* kids = P + mgx_sec_off(P, MGX_SEC_CHILDREN) + hd[MGX_HD_CHILD_START];
      for (int i = 0; i < hd[MGX_HD_CHILD_COUNT]; i++) push(kids[i]);
      continue;
    }
    for (int i = 0; i < hd[MGX_HD_MUT_COUNT] && r.ok; i++) {
      r.muts.push_back(P + mgx_sec_off(P, MGX_SEC_MUTS) + (hd[MGX_HD_MUT_START] + i) * MGX_MU_WORDS);
      r.ok = mut_ok(r.muts.back());
    }
    std::vector<int> pcs{hd[MGX_HD_FILTER_PC]};
    std::vector<char> aseen(n_atoms, 0);
    while (!pcs.empty() && r.ok) {
      const int pc = pcs.back();
      pcs.pop_back();
      if (pc < 0 || pc >= n_atoms || aseen[pc]) continue;
      aseen[pc] = 1;
      const int32_t* a = P + mgx_sec_off(P, MGX_SEC_ATOMS) + pc * MGX_AT_WORDS;
      r.ok = atom_ok(a);
      pcs.push_back(a[MGX_AT_ON_TRUE]);
      pcs.push_back(a[MGX_AT_ON_FALSE]);
    }
  }
  return r;
}

// Sum of a per-class value over the objects of one class map (0: empty cell, else class + 1).
template <class T>
inline T mgx_map_sum(const std::vector<T>& per_class, const uint16_t* map, size_t hw) {
  T s{};
  for (size_t i = 0; i < hw; i++)
    if (map[i] > 0 && map[i] <= per_class.size()) s += per_class[map[i] - 1];
  return s;
}
// Area-effect and territory sources of each class.
struct MgxSources {   // fixed AoE, mobile AoE, territory
  int f = 0, m = 0, t = 0;
  MgxSources& operator+=(const MgxSources& o) { f += o.f; m += o.m; t += o.t; return *this; }
};
inline std::vector<MgxSources> mgx_class_sources(const int32_t* P) {
  std::vector<MgxSources> s(P[MGX_H_NUM_CLASSES]);
  for (size_t c = 0; c < s.size(); c++) {
    const int32_t* C = P + mgx_sec_off(P, MGX_SEC_CLASSES) + c * MGX_C_WORDS;
    for (int i = 0; i < C[MGX_C_AOE_COUNT]; i++)
      (P[mgx_sec_off(P, MGX_SEC_AOES) + (C[MGX_C_AOE_START] + i) * MGX_AO_WORDS + MGX_AO_STATIC] ? s[c].f : s[c].m)++;
    s[c].t = C[MGX_C_TERR_COUNT];
  }
  return s;
}

// Entries of the observation kernel's LDS token pool: the class-tag prefix + the per-step lists, capped and rounded to 8.
inline int mgx_pool_tokens(int prefix, long long list_tokens) { return (prefix + (int)std::min<long long>(list_tokens, 16384) + 7) & ~7; }

struct MgxPlan {
  MgxDev d{};                  // every scalar field and path decision; the pointers are the engine's
  int num_tags = 0;            // MGX_H_NUM_TAGS
  unsigned long long handler_fp = 0;  // FNV-1a of the handler tables (gen_handlers.py fingerprint())
  // lane-per-agent area-effect kernel (mgx_aoe_kernel): runs when area effects only touch their target and the game has sources
  bool aoe_kernel = false;
  bool aoe_prog_lds = false;   // ... with the hot program range (prog_lds_words) copied into its LDS
  std::vector<int16_t> aoe_stat_ids;   // the agent stats it stages per lane (MgxDev::aoe_stat_ids)
  std::vector<uint8_t> aoe_stat_map;   // stat id -> local index, 0xFF = not staged (MgxDev::aoe_stat_map)
  // world kernels
  size_t lds_world = 0, lds_act = 0;
  bool prog_in_lds = false;
  int prog_lds_words = 0;      // program words the world kernels copy into LDS, rounded up to 4
  int hot_lo = 0, hot_hi = 0;  // [hot_lo, hot_hi): program words of the extended kernels' copy (the hot range)
  // observation kernel
  int obs_blk_start = 0, obs_blk_words = 0;  // program block the observation kernel interprets
  bool obs_blk_lds = false;
  std::vector<uint32_t> cls_tokinfo;   // per-class static tag tokens (MgxDev::cls_tokinfo / cls_tok)
  std::vector<uint16_t> cls_tok;
  int pool_prefix = 0;         // entries of the per-class static tag table at the head of the pool
  int pool_tokens = 0;         // capacity of the LDS token pool (entries), including the class-tag prefix
  std::vector<int> class_list_tokens;  // worst-case per-step token list length per class (0: static class)
  bool pool_from_maps = false;         // pool sized from the class maps (no run-time object creation / tag changes)
  int obs_threads = MGX_OBS_THREADS, obs_ew = MGX_OBS_THREADS / MGX_WAVE;
  size_t lds_obs = 0;
  int obs_variant = 0;   // 0: generic observation kernel; 3 / 5: the instances for the shape of BASELINE.json configs[2]; 9: mgx_attach_code
  int world_variant = 0; // 0: generic lean world kernel; 3: the instance compiled for the shape of BASELINE.json configs[2] (MgxWorldShapeR3)
  // where reward expressions are evaluated: 1 beside the token-cache phase (no stat operands, lean), 2 during the extended
  // kernel's encode phase (nothing it writes is read), 0 at the kernel's end
  int rmode = 0;
  bool rewards_ext = false;    // reward expressions have query operands: evaluated by mgx_values_kernel after the obs kernel
  bool obsval = false;         // observation values have query operands: MgxDev::obsval, written by mgx_values_kernel

  // max over the selected envs of the summed worst-case list lengths of the objects on their class maps
  long long list_tokens_bound(const uint16_t* class_maps, size_t first, size_t count, const uint8_t* mask) const {
    const size_t hw = (size_t)d.H * d.W;
    long long best = 0;
    for (size_t env = first; env < first + count; env++)
      if (!mask || mask[env]) best = std::max<long long>(best, mgx_map_sum(class_list_tokens, class_maps + env * hw, hw));
    return best;
  }
  // dynamic LDS of the observation kernel for the current pool with `ew` encode wavefronts
  size_t obs_lds_bytes(int ew) const {
    const int xmode = mgx_obs_xmode(d.X != 0, d.X && d.aoe_mask_feat != 0 && d.NT > 0, d.S, num_tags);
    return (size_t)mgx_obs_lds_layout(d.H * d.W, d.NOFF, d.S, d.A, d.T, pool_tokens, xmode, d.n_obs_values, obs_blk_lds ? obs_blk_words : 0,
                                      mgx_obs_gt(d.n_obs_values, d.base, d.flags), rmode == 1, ew).total;
  }
  // The observation kernel's shape for the current pool: threads, encode wavefronts, dynamic LDS and the preset instance
  // (0 / 3 / 5).  false: the staging does not fit a CU.
  bool size_obs(const MgxSwitches& sw) {
    // extended games with many agents per env: 512 threads, of which EW wavefronts encode (4 staging rows each).  Fewer
    // encode wavefronts = fewer rows in LDS: the largest EW of 4, 3, 2 that lets three workgroups share a CU's 160 KB is
    // taken (rung 4, T = 200: EW 4, 52.8 KB, 4.3 ms; all eight wavefronts encoding: 66.6 KB, two workgroups, 5.2 ms;
    // T = 256: EW 3, 52.6 KB, 4.8 ms against 6.1 ms for EW 4 at two workgroups; 1 024 threads 8.6 ms; 256 threads 7.25 ms;
    // the lean kernel with 512 threads 1.14 instead of 0.67 ms)
    obs_threads = (d.X && d.A >= 48 && sw.obs_512) ? 512 : MGX_OBS_THREADS;
    obs_ew = obs_threads / MGX_WAVE;
    if (obs_threads == 512) {
      obs_ew = 4;
      for (int ew : {4, 3, 2})
        if (obs_lds_bytes(ew) <= 53760) { obs_ew = ew; break; }
    }
    lds_obs = obs_lds_bytes(obs_ew);
    obs_variant = 0;
    if (sw.obs_preset && !d.X && obs_blk_lds) {
      if (mgx_obs_shape_matches<MgxObsShapeR3>(d, obs_blk_words, rmode)) obs_variant = 3;
      else if (mgx_obs_shape_matches<MgxObsShapeR3AnyLength>(d, obs_blk_words, rmode)) obs_variant = 5;   // same shape, max_steps set
      // (an instance for the shape of configs[3], MgxObsShapeR4, was measured too: 5.07 ms against the generic kernel's 5.01 —
      // the extended kernel's time is barrier and LDS latency, not scalar arithmetic; it is not built)
    }
    return lds_obs <= 160 * 1024;
  }
};
#define MGX_OBS_LDS_REFUSAL "map/object count too large for the LDS staging of the observation kernel"

// Validate `P` (`words` words) and the class maps of `E` envs, and plan the engine.  MGX_OK, or the refusal's code with
// its message in `why`.
inline int mgx_plan(const int32_t* P, size_t words, const uint16_t* class_maps, int E, const MgxSwitches& sw, MgxPlan& p,
                    std::string& why) {
  auto refuse = [&](int code, const std::string& msg) { why = msg; return code; };
  if (words < MGX_H_WORDS || P[MGX_H_MAGIC] != MGX_MAGIC || P[MGX_H_VERSION] != MGX_VERSION || (size_t)P[MGX_H_TOTAL_WORDS] != words)
    return refuse(MGX_ERR_PROGRAM, "mgx_create: not a version-" + std::to_string(MGX_VERSION) + " mgx program");
  if (P[MGX_H_NUM_RESOURCES] > MGX_MAX_RESOURCES || P[MGX_H_NUM_AGENTS] > MGX_MAX_AGENTS || P[MGX_H_HEIGHT] > 255 ||
      P[MGX_H_WIDTH] > 255 || P[MGX_H_NUM_AGENTS] < 1 || P[MGX_H_TOKEN_BASE] < 2 || P[MGX_H_TOKEN_BASE] > 256 ||
      P[MGX_H_NUM_TOKENS] < 1 || P[MGX_H_OBS_HEIGHT] > 15 || P[MGX_H_OBS_WIDTH] > 15)
    return refuse(MGX_ERR_PROGRAM, "mgx_create: program exceeds engine limits (resources<=13, agents<255, map<=255x255)");
  // the handler VM's context slots hold object slot ids as (id + 2) & 0xFFFF (mgx_world.h ctx_store): ids up to 65533
  if (P[MGX_H_MAX_OBJECTS] < 1 || P[MGX_H_MAX_OBJECTS] > MGX_MAX_OBJECT_SLOTS)
    return refuse(MGX_ERR_PROGRAM, "mgx_create: max_objects must be 1.." + std::to_string(MGX_MAX_OBJECT_SLOTS));
  // Nesting the device evaluates in fixed storage: queries (eval_query<3>), the game-value stack (MgxValueStack) and the
  // levels of a handler tree (VM frames; lean programs run on the register VM, which has fewer: checked once d.X is known).
  if (P[MGX_H_QUERY_DEPTH] > MGX_MAX_QUERY_DEPTH)
    return refuse(MGX_ERR_PROGRAM, "mgx_create: queries nest deeper than " + std::to_string(MGX_MAX_QUERY_DEPTH) + " levels");
  const int n_code = mgx_sec_cnt(P, MGX_SEC_GV_CODE);
  {
    auto stack_ok = [&](int start, int count) {
      if (start < 0 || count < 0 || start + count > n_code) return false;
      int depth = 0;
      return !mgx_gv_any(P, start, count, [&](const int32_t* g) {
        const int op = g[MGX_GV_OP];
        depth += (op == MGX_GOP_ADD_TERM || op == MGX_GOP_RATIO || op == MGX_GOP_MAX2 || op == MGX_GOP_MIN2) ? -1 : 1;
        return depth > MGX_VALUE_STACK;
      });
    };
    bool ok = true;
    for (int k = 0; k < mgx_sec_cnt(P, MGX_SEC_OBS_VALUES) && ok; k++) {
      const int32_t* V = P + mgx_sec_off(P, MGX_SEC_OBS_VALUES) + k * MGX_OV_WORDS;
      ok = stack_ok(V[MGX_OV_GV_START], V[MGX_OV_GV_COUNT]);
    }
    for (int k = 0; k < mgx_sec_cnt(P, MGX_SEC_REWARDS) && ok; k++) {
      const int32_t* R = P + mgx_sec_off(P, MGX_SEC_REWARDS) + k * MGX_RW_WORDS;
      ok = stack_ok(R[MGX_RW_GV_START], R[MGX_RW_GV_COUNT]);
    }
    if (!ok)
      return refuse(MGX_ERR_PROGRAM, "mgx_create: a game value expression needs more than " + std::to_string(MGX_VALUE_STACK) + " stack entries");
  }
  int hnest = 0;   // VM frames the deepest handler tree needs (children are laid out before their parent)
  {
    const int n_hd = mgx_sec_cnt(P, MGX_SEC_HANDLERS);
    std::vector<int> lv(n_hd, 1);
    for (int h = 0; h < n_hd; h++) {
      const int32_t* hd = P + mgx_sec_off(P, MGX_SEC_HANDLERS) + h * MGX_HD_WORDS;
      if (hd[MGX_HD_KIND] != MGX_HK_LEAF)
        for (int i = 0; i < hd[MGX_HD_CHILD_COUNT]; i++) {
          const int k = P[mgx_sec_off(P, MGX_SEC_CHILDREN) + hd[MGX_HD_CHILD_START] + i];
          lv[h] = std::max(lv[h], k >= 0 && k < h ? lv[k] + 1 : MGX_MAX_HANDLER_NESTING + 1);
        }
      hnest = std::max(hnest, lv[h]);
    }
    // an on_use / on_after_use tree runs on frames above the move handler whose UseTarget reached it
    auto level = [&](int h) { return h >= 0 && h < n_hd ? lv[h] : 0; };
    int mv = 0, use = 0;
    for (int k = 0; k < P[MGX_H_NUM_MOVE_HANDLERS]; k++)
      mv = std::max(mv, level(P[mgx_sec_off(P, MGX_SEC_MOVE_HANDLERS) + k * MGX_MH_WORDS + MGX_MH_HANDLER]));
    for (int c = 0; c < P[MGX_H_NUM_CLASSES]; c++) {
      const int32_t* C = P + mgx_sec_off(P, MGX_SEC_CLASSES) + c * MGX_C_WORDS;
      use = std::max(use, std::max(level(C[MGX_C_ON_USE]), level(C[MGX_C_ON_AFTER_USE])));
    }
    if (use > 0) hnest = std::max(hnest, mv + use);
    if (hnest > MGX_MAX_HANDLER_NESTING)
      return refuse(MGX_ERR_PROGRAM, "mgx_create: handlers nest deeper than " + std::to_string(MGX_MAX_HANDLER_NESTING) + " levels");
  }
  const int nc = P[MGX_H_NUM_CLASSES];
  const size_t hw = (size_t)P[MGX_H_HEIGHT] * P[MGX_H_WIDTH];
  for (size_t i = 0; i < (size_t)E * hw; i++)
    if (class_maps[i] > nc)
      return refuse(MGX_ERR_BAD_ARG, "mgx_create: class map holds id " + std::to_string(class_maps[i]) + " but the program has " +
                                         std::to_string(nc) + " classes");

  // ---- the scalar table ----
  MgxDev& d = p.d;
  d.E = E; d.H = P[MGX_H_HEIGHT]; d.W = P[MGX_H_WIDTH]; d.A = P[MGX_H_NUM_AGENTS]; d.S = P[MGX_H_MAX_OBJECTS];
  d.R = P[MGX_H_NUM_RESOURCES] > 0 ? P[MGX_H_NUM_RESOURCES] : 1;
  d.T = P[MGX_H_NUM_TOKENS];
  d.NS = P[MGX_H_NUM_AGENT_STATS]; d.NG = P[MGX_H_NUM_GAME_STATS];
  d.NSW = (d.NS + 31) / 32; d.NGW = (d.NG + 31) / 32;
  d.NSP = d.NSW * 32;
  d.SEENW = (d.H * d.W + 31) / 32;
  d.NOFF = P[MGX_H_NUM_OBS_OFFSETS];
  d.base = P[MGX_H_TOKEN_BASE];
  d.max_steps = P[MGX_H_MAX_STEPS]; d.truncates = P[MGX_H_EPISODE_TRUNCATES]; d.max_priority = P[MGX_H_MAX_PRIORITY];
  d.nact = P[MGX_H_NUM_ACTIONS]; d.flags = P[MGX_H_GLOBAL_FLAGS]; d.hp_res = P[MGX_H_HP_RESOURCE];
  if (d.nact > 32000) return refuse(MGX_ERR_PROGRAM, "mgx_create: more than 32000 actions");
  d.n_obs_values = P[MGX_H_NUM_OBS_VALUES]; d.n_move_handlers = P[MGX_H_NUM_MOVE_HANDLERS];
  for (int i = 0; i < 14; i++) d.feat[i] = P[MGX_H_FEAT_BASE + i];
  d.feat[14] = P[MGX_H_OBS_HEIGHT] >> 1;
  d.feat[15] = P[MGX_H_OBS_WIDTH] >> 1;
  for (int i = 0; i < 32; i++) d.wk[i] = P[MGX_H_STAT_BASE + i];
  for (int s = 0; s < MGX_SEC_COUNT; s++) d.sec[s] = mgx_sec_off(P, s);
  d.NRW = 1;
  for (int c = 0; c < nc; c++) {
    const int32_t* C = P + d.sec[MGX_SEC_CLASSES] + c * MGX_C_WORDS;
    d.NRW = std::max(d.NRW, (int)C[MGX_C_REWARD_COUNT]);
    if (C[MGX_C_ON_TICK] >= 0) d.any_on_tick = 1;
  }

  // ---- extended (rung 4) features: capacities come from a host scan of the class maps ----
  d.n_events = P[MGX_H_NUM_EVENTS]; d.n_schedule = P[MGX_H_NUM_SCHEDULE]; d.n_matq = P[MGX_H_NUM_MATQ];
  d.NT = P[MGX_H_NUM_TERRITORIES]; d.game_on_tick = P[MGX_H_GAME_ON_TICK]; d.NL = P[MGX_H_NUM_INDEXED_TAGS];
  d.aoe_mask_feat = P[MGX_H_FEAT_BASE + MGX_F_AOE_MASK];
  p.num_tags = P[MGX_H_NUM_TAGS];
  d.QD = std::max(1, (int)P[MGX_H_QUERY_DEPTH]) + 1;
  d.QB = 3 + 2 * (d.QD + 1);
  d.AW = (d.A + 31) / 32;
  d.SW = (d.S + 31) / 32;
  {
    const std::vector<MgxSources> cls = mgx_class_sources(P);
    MgxSources cap, per;   // max over the maps, max over the classes
    for (const MgxSources& s : cls) { per.f = std::max(per.f, s.f); per.m = std::max(per.m, s.m); }
    const bool any_aoe = per.f > 0 || per.m > 0;
    if (any_aoe || d.NT > 0)
      for (int env = 0; env < E; env++) {
        const MgxSources s = mgx_map_sum(cls, class_maps + (size_t)env * hw, hw);
        cap.f = std::max(cap.f, s.f); cap.m = std::max(cap.m, s.m); cap.t = std::max(cap.t, s.t);
      }
    if (P[MGX_H_SPAWNS]) {  // spawned objects may bring AoEs: leave room for one set per object slot
      cap.f += per.f ? std::min<int>(d.S * per.f, 4096) : 0;
      cap.m += per.m ? std::min<int>(d.S * per.m, 4096) : 0;
    }
    d.NF = cap.f; d.NM = cap.m; d.NTS = cap.t;
    // A territory type without a source on any create map: the observation kernel's aoe_mask staging, the area-effect
    // kernel and cell_owner read the ownership map and the source count of every env unconditionally, so both exist
    // (room for one source, none registered) — with NTS = 0 they were null pointers and the first observation pass faulted.
    if (d.NT > 0 && d.NTS == 0) d.NTS = 1;
    d.FW = std::max(1, (d.NF + 31) / 32); d.MW = std::max(1, (d.NM + 31) / 32);
    d.X = (any_aoe || d.NT > 0 || d.n_schedule > 0 || d.n_matq > 0 || d.game_on_tick >= 0 || P[MGX_H_DYNAMIC_TAGS] ||
           mgx_sec_cnt(P, MGX_SEC_QUERIES) > 0) ? 1 : 0;
  }
  p.aoe_kernel = d.X && (d.NF > 0 || d.NM > 0 || d.NT > 0) && sw.aoe_local && mgx_aoe_is_target_local(P);
  d.x_aoe_lds = (d.X && !p.aoe_kernel) ? 1 : 0;   // otherwise the extended world kernel runs the AoE phase itself
  if (!d.X && hnest > MGX_MAX_HANDLER_NESTING_REG)   // lean programs run every handler on the register VM
    return refuse(MGX_ERR_PROGRAM, "mgx_create: handlers of a lean program nest deeper than " +
                                       std::to_string(MGX_MAX_HANDLER_NESTING_REG) + " levels (the register VM's frames)");
  // The world kernel stages per agent and env 17 B (lean, 64 envs per workgroup) or 15 B (extended, 32 envs), plus per env
  // 144 B of VM words and, when the AoE phase runs in the world kernel, 176 B of scratch (extended) — at most 160 KB: the
  // agents an env may have depend on the program.  The program copy below is added only when it fits.  Past 64 KB the
  // kernels need the opt-in attribute.
  p.lds_world = d.X ? mgx_world_x_lds_bytes(d.A, d.x_aoe_lds != 0) : mgx_world_fast_lds_bytes(d.A);
  if (p.lds_world > 160 * 1024)
    return refuse(MGX_ERR_PROGRAM, "mgx_create: " + std::to_string(d.A) + " agents per env are too many for the " +
                                       (d.X ? "extended" : "lean") + " world kernel's LDS staging (" + std::to_string(p.lds_world) +
                                       " B > 160 KB per workgroup)");
  d.tick_in_aoe = (p.aoe_kernel && d.any_on_tick && sw.tick_in_aoe && mgx_aoe_on_tick_local(P)) ? 1 : 0;
  d.cov_in_aoe = (p.aoe_kernel && d.game_on_tick < 0 && sw.tick_in_aoe) ? 1 : 0;
  // The world kernels copy the program — everything in front of the schedule, the last and only section that grows with
  // the episode length — into LDS when it leaves room for 4 (lean) / 3 (extended) workgroups per CU (160 KB LDS).
  // (Rung 4, measured: the copy at 2 workgroups per CU is slower than the program in HBM at 3: 9.8 against 8.4 ms.)
  p.prog_lds_words = (int)((d.sec[MGX_SEC_SCHEDULE] + 3) & ~3);
  if (d.X) {  // extended kernel: only the sections the handler VM walks (LIMITS .. TERR_CONTROLS); the class table — one
              // record per agent — and the tag-list index are read from HBM / L2 (mgx_world.h MGX_HOT_PROG)
    p.hot_lo = d.sec[MGX_SEC_LIMITS] & ~3;
    p.hot_hi = d.sec[MGX_SEC_TAG_LISTS];
    p.prog_lds_words = ((p.hot_hi - p.hot_lo) + 3) & ~3;
  }
  p.prog_in_lds = sw.prog_lds && (size_t)p.prog_lds_words * 4 + p.lds_world <= (size_t)(d.X ? 53 : 40) * 1024;
  if (p.prog_in_lds) p.lds_world += (size_t)p.prog_lds_words * 4;

  if (p.aoe_kernel) {
    // the agent stats the lane-per-agent area-effect kernel keeps in LDS (mgx_aoe_local.h)
    mgx_aoe_collect_stats(P, d.tick_in_aoe != 0, d.cov_in_aoe != 0, p.aoe_stat_ids);
    p.aoe_stat_map.assign(256, 0xFF);
    for (size_t k = 0; k < p.aoe_stat_ids.size(); k++) p.aoe_stat_map[(size_t)p.aoe_stat_ids[k]] = (uint8_t)k;
    d.aoe_nstat = (int)p.aoe_stat_ids.size();
    // hot program range in the kernel's LDS when it leaves room for three workgroups per CU
    p.aoe_prog_lds = sw.aoe_prog_lds && (size_t)mgx_aoe_lds_bytes(d.aoe_nstat) + (size_t)p.prog_lds_words * 4 <= 52 * 1024;
  }
  // ---- observation kernel ----
  // Per-class static tag tokens (ascending tag id, core/grid_object.cpp:181-186) at the head of the LDS token pool, then
  // room for the per-step lists (objects of non-static classes).  Worst case per class from the program: tags + vibe +
  // R * digits + 2.  Without run-time object creation and without tag mutations the class maps bound it exactly (sum over
  // the env's objects, max over envs); otherwise one worst-case list per slot.
  int digits = 1;
  for (unsigned v = 65535u / (unsigned)d.base; v > 0; v /= (unsigned)d.base) digits++;
  int max_per_obj = 1;
  p.cls_tokinfo.assign(nc, 0);
  p.class_list_tokens.assign(nc, 0);
  for (int c = 0; c < nc; c++) {
    const int32_t* C = P + d.sec[MGX_SEC_CLASSES] + c * MGX_C_WORDS;
    const uint32_t start = (uint32_t)p.cls_tok.size();
    int nt = 0;
    for (int t = 0; t < 256; t++)
      if (((uint32_t)C[MGX_C_TAGS + (t >> 5)] >> (t & 31)) & 1u) { p.cls_tok.push_back((uint16_t)(d.feat[MGX_F_TAG] | (t << 8))); nt++; }
    if (nt > 63 || start > 0xFFFF) return refuse(MGX_ERR_PROGRAM, "mgx_create: more than 63 tags on one class");
    p.cls_tokinfo[c] = start | ((uint32_t)(C[MGX_C_GROUP] & 0xFF) << 16) | ((uint32_t)nt << 24) |
                       (C[MGX_C_KIND] == MGX_KIND_AGENT ? 0x40000000u : 0u) | (C[MGX_C_STATIC] ? 0x80000000u : 0u);
    const int n = nt + (C[MGX_C_STATIC] ? 0 : 1 + P[MGX_H_NUM_RESOURCES] * digits + (C[MGX_C_KIND] == MGX_KIND_AGENT ? 2 : 0) +
                                              P[MGX_H_NUM_MATQ_TAGS]);  // + the tags materialized queries may add
    max_per_obj = std::max(max_per_obj, n);
    p.class_list_tokens[c] = C[MGX_C_STATIC] ? 0 : n;
  }
  if (p.cls_tok.empty()) p.cls_tok.push_back(0);
  p.pool_prefix = (int)p.cls_tok.size();
  p.pool_from_maps = !P[MGX_H_SPAWNS] && !P[MGX_H_TAG_MUTATIONS];
  p.pool_tokens = mgx_pool_tokens(p.pool_prefix, p.pool_from_maps ? p.list_tokens_bound(class_maps, 0, (size_t)E, nullptr)
                                                                   : (long long)d.S * max_per_obj);
  {  // sections INV_FEATURES..OBS_VALUES are contiguous (sections are laid out in id order); small block -> LDS copy
    const int b0 = d.sec[MGX_SEC_INV_FEATURES], b1 = d.sec[MGX_SEC_WORDLIST];
    const bool ordered = b0 <= d.sec[MGX_SEC_GV_CODE] && d.sec[MGX_SEC_GV_CODE] <= d.sec[MGX_SEC_REWARDS] &&
                         d.sec[MGX_SEC_REWARDS] <= d.sec[MGX_SEC_OBS_VALUES] && d.sec[MGX_SEC_OBS_VALUES] <= b1;
    p.obs_blk_start = b0;
    p.obs_blk_words = b1 - b0;
    p.obs_blk_lds = !d.X && ordered && (b0 & 3) == 0 && (p.obs_blk_words & 3) == 0 && p.obs_blk_words * 4 <= 8 * 1024;
  }

  // ---- per-action bookkeeping ----
  {
    const int n_mut = mgx_sec_cnt(P, MGX_SEC_MUTS);
    auto any_mut = [&](auto&& pred) {
      for (int i = 0; i < n_mut; i++)
        if (pred(P + d.sec[MGX_SEC_MUTS] + i * MGX_MU_WORDS)) return true;
      return false;
    };
    // a mutation that writes an agent stat `stat` admits: SetStat, or a game-value mutation whose target is a StatValue
    auto writes = [&](const int32_t* m, auto&& stat) {
      if (m[MGX_MU_OP] == MGX_MOP_STATS) return m[MGX_MU_A0] != 0 && stat(m[MGX_MU_A2]);
      if (m[MGX_MU_OP] != MGX_MOP_GAME_VALUE || m[MGX_MU_A1] < 0) return false;
      const int32_t* V = P + d.sec[MGX_SEC_OBS_VALUES] + m[MGX_MU_A1] * MGX_OV_WORDS;
      const int32_t* c0 = P + d.sec[MGX_SEC_GV_CODE] + V[MGX_OV_GV_START] * MGX_GV_WORDS;
      return V[MGX_OV_GV_COUNT] > 0 && mgx_gv_agent_stat(c0) && stat(c0[MGX_GV_A1]);
    };
    // the counters the deferred pass writes: the per-kind success / failed counters, action.failed and
    // max_steps_without_motion (a game that counts zone entries in an agent stat and adds to it from a territory handler
    // does not care when `action.move.success` is brought up to date)
    auto booked = [&](int id) {
      for (int k : {MGX_S_NOOP_SUCCESS, MGX_S_MOVE_SUCCESS, MGX_S_VIBE_SUCCESS})
        if (id == d.wk[k] || id == d.wk[k + 1]) return true;
      return id == d.wk[MGX_S_ACTION_FAILED] || id == d.wk[MGX_S_MAX_STEPS_WITHOUT_MOTION];
    };
    auto covers = [&](int id) { return id == d.wk[MGX_S_CELL_UNIQUE] || id == d.wk[MGX_S_CELL_MAXDIST]; };
    // Per-action bookkeeping stats can be applied at the end of the tick unless a game value evaluated mid-tick reads one
    // of them (reward expressions run in the observation kernel, after the flush) ...
    std::vector<char> in_reward(n_code, 0);
    const int32_t* rw = P + d.sec[MGX_SEC_REWARDS];
    for (int k = 0; k < mgx_sec_cnt(P, MGX_SEC_REWARDS); k++)
      for (int i = 0; i < rw[k * MGX_RW_WORDS + MGX_RW_GV_COUNT]; i++) {
        const int at = rw[k * MGX_RW_WORDS + MGX_RW_GV_START] + i;
        if (at >= 0 && at < n_code) in_reward[at] = 1;
      }
    const int32_t* code = P + d.sec[MGX_SEC_GV_CODE];
    const bool reads_mid = mgx_gv_any(P, 0, n_code, [&](const int32_t* g) {
      return !in_reward[(g - code) / MGX_GV_WORDS] && mgx_gv_agent_stat(g) && booked(g[MGX_GV_A1]); });
    // ... or a handler WRITES one of them mid-tick (SetStat / a game-value mutation on a StatValue): set-then-deferred-add
    // would end on a different value than the reference's add-then-set
    d.defer_book = (reads_mid || any_mut([&](const int32_t* m) { return writes(m, booked); })) ? 0 : 1;  // (flushed at the end of the launch that runs the action phase)
    // ... and can be kept as integers beside the stat rows (mgx_world.h tail_shadow) when nothing on the device reads the
    // cells between two flushes: no game value at all — rewards and observation values included — reads one of them or a
    // coverage stat, and no mutation writes a coverage stat.  The dispatch narrows this further below.
    const bool counters = d.defer_book && sw.shadow &&
                          !mgx_gv_any(P, 0, n_code, [&](const int32_t* g) { return mgx_gv_agent_stat(g) && booked(g[MGX_GV_A1]); });
    const bool coverage = !mgx_gv_any(P, 0, n_code, [&](const int32_t* g) { return mgx_gv_agent_stat(g) && covers(g[MGX_GV_A1]); }) &&
                          !any_mut([&](const int32_t* m) { return writes(m, covers); });
    d.shadow = !counters ? 0 : coverage ? 3 : 1;
  }

  // ---- handlers ----
  std::vector<int> act_roots, tick_roots;   // where the action phase starts (move handlers, on_use, on_after_use); on_tick
  const int32_t* mh = P + d.sec[MGX_SEC_MOVE_HANDLERS];
  bool range1 = true;   // every move handler looks one cell ahead
  bool moving_terr = false;   // an agent class is a territory source (it re-registers when it moves)
  for (int k = 0; k < d.n_move_handlers; k++) {
    act_roots.push_back(mh[k * MGX_MH_WORDS + MGX_MH_HANDLER]);
    if (mh[k * MGX_MH_WORDS + MGX_MH_MAX_RANGE] != 1) range1 = false;
  }
  for (int c = 0; c < nc; c++) {
    const int32_t* C = P + d.sec[MGX_SEC_CLASSES] + c * MGX_C_WORDS;
    act_roots.push_back(C[MGX_C_ON_USE]);
    act_roots.push_back(C[MGX_C_ON_AFTER_USE]);
    tick_roots.push_back(C[MGX_C_ON_TICK]);
    if (C[MGX_C_KIND] == MGX_KIND_AGENT && C[MGX_C_TERR_COUNT] > 0) moving_terr = true;
  }
  if (d.X) {  // can the action phase's top-level handlers run on the register VM (four frames)?  (mgx_world.h apply_top)
    std::vector<int> roots = act_roots;
    roots.insert(roots.end(), tick_roots.begin(), tick_roots.end());
    roots.push_back(d.game_on_tick);
    d.flat_top = sw.flat_top && hnest <= MGX_MAX_HANDLER_NESTING_REG &&
                 mgx_reach(P, roots,
                           [](const int32_t* m) {
                             switch (m[MGX_MU_OP]) {
                               case MGX_MOP_RESOURCE_DELTA: case MGX_MOP_RESOURCE_TRANSFER: case MGX_MOP_CLEAR_INVENTORY: case MGX_MOP_ATTACK:
                               case MGX_MOP_STATS: case MGX_MOP_CHANGE_VIBE: case MGX_MOP_RELOCATE: case MGX_MOP_SWAP: case MGX_MOP_USE_TARGET:
                               case MGX_MOP_GAME_VALUE: return true;
                               default: return false;   // tag mutations (lifecycle handlers), query recomputation, push / spawn / query inventory
                             }
                           },
                           [&](const int32_t* a) {   // filters: no atom that evaluates a query (check_filters<0>)
                             if (a[MGX_AT_OP] == MGX_FOP_QUERY_RESOURCE || (a[MGX_AT_OP] == MGX_FOP_MAX_DISTANCE && a[MGX_AT_A2] >= 0)) return false;
                             return a[MGX_AT_OP] != MGX_FOP_GAME_VALUE || (!mgx_value_any(P, a[MGX_AT_A1], mgx_gv_query) && !mgx_value_any(P, a[MGX_AT_A2], mgx_gv_query));
                           }).ok;
  }
  {  // Do the handler tables equal a preset the build generated straight-line handler code for (mgx_handlers_gen.h)?
    unsigned long long h = 0xCBF29CE484222325ull;   // FNV-1a over 32-bit words: mettagrid_amd/gen_handlers.py fingerprint()
    auto mix = [&](int32_t v) { h = (h ^ (unsigned long long)(uint32_t)v) * 0x100000001B3ull; };
    const int secs[5] = {MGX_SEC_HANDLERS, MGX_SEC_CHILDREN, MGX_SEC_ATOMS, MGX_SEC_MUTS, MGX_SEC_MOVE_HANDLERS};
    const int words[5] = {MGX_HD_WORDS, 1, MGX_AT_WORDS, MGX_MU_WORDS, MGX_MH_WORDS};
    for (int k = 0; k < 5; k++) {
      const int n = mgx_sec_cnt(P, secs[k]);
      mix(n);
      for (int i = 0; i < n * words[k]; i++) mix(P[d.sec[secs[k]] + i]);
    }
    mix(nc);
    for (int c = 0; c < nc; c++) {
      const int32_t* C = P + d.sec[MGX_SEC_CLASSES] + c * MGX_C_WORDS;
      mix(C[MGX_C_ON_USE]); mix(C[MGX_C_ON_AFTER_USE]); mix(C[MGX_C_ON_TICK]);
    }
    mix(P[MGX_H_GAME_ON_TICK]);
    p.handler_fp = h;
    d.gen_prog = !sw.gen ? 0 : (!d.X && h == MGX_GEN_R3_FP) ? 3 : (d.X && h == MGX_GEN_R4_FP) ? 4 : 0;
  }
  {  // Can the action dispatch run with one lane per AGENT (mgx_act.h)?  Every handler an action reaches must stay with
     // its actor and target, look at no game-wide state, and the order of game-stat SETs must be recoverable.
    auto pure = [&](int rec) {   // reads inventories, agent-scope stats and constants only
      return !mgx_value_any(P, rec, [](const int32_t* g) { return mgx_gv_query(g) || (g[MGX_GV_OP] == MGX_GOP_STAT && g[MGX_GV_A0] == 1); });
    };
    auto local = [&](const std::vector<int>& roots, bool may_move) {
      return mgx_reach(P, roots,
                       [&](const int32_t* m) {
                         switch (m[MGX_MU_OP]) {
                           case MGX_MOP_RESOURCE_DELTA: case MGX_MOP_CLEAR_INVENTORY: case MGX_MOP_ATTACK: case MGX_MOP_CHANGE_VIBE:
                           case MGX_MOP_USE_TARGET: return true;
                           case MGX_MOP_RESOURCE_TRANSFER: return !(d.X && m[MGX_MU_A4]);   // may remove the emptied object
                           case MGX_MOP_RELOCATE: case MGX_MOP_SWAP: return may_move;
                           case MGX_MOP_STATS: return pure(m[MGX_MU_A3]);
                           case MGX_MOP_GAME_VALUE: return pure(m[MGX_MU_A1]) && pure(m[MGX_MU_A2]);   // (a game-scope target is impure too)
                           default: return false;
                         }
                       },
                       [&](const int32_t* a) {
                         switch (a[MGX_AT_OP]) {
                           case MGX_FOP_VIBE: case MGX_FOP_RESOURCE: case MGX_FOP_SHARED_TAG: case MGX_FOP_TAG: case MGX_FOP_TARGET_LOC_EMPTY:
                           case MGX_FOP_TARGET_IS_USABLE: case MGX_FOP_PERIODIC: case MGX_FOP_TRUE: return true;
                           case MGX_FOP_GAME_VALUE: return pure(a[MGX_AT_A1]) && pure(a[MGX_AT_A2]);
                           case MGX_FOP_MAX_DISTANCE: return a[MGX_AT_A2] < 0;
                           default: return false;
                         }
                       });
    };
    const MgxReach act = local(act_roots, true), tick = local(tick_roots, false);
    const std::vector<int> act_sets = act.game_sets(), tick_sets = tick.game_sets();
    // Measured (MI355X, 65 536 envs): 64 agents per env 4.92 -> 2.0 ms; 16 agents per env 0.445 -> 0.52 ms — four envs share
    // a wavefront there and a round costs what 2.4 serial steps cost, so lean games stay lane per env unless asked.
    bool par = sw.act_par && d.A <= 64 && range1 && act.ok &&
               (d.X ? d.flat_top && p.prog_in_lds && !moving_terr   // tag mutations, query recomputation / filters: lane-per-env
                                                                    // VM; mgx_act_x.hip is built for the hot range in LDS only
                    : 16 * mgx_pow2_at_least(d.A) <= 256 && sw.act_lean);   // mgx_act_fast.hip: 16 envs per workgroup of at most 256 lanes
    std::vector<int> gset = act_sets;
    if (!d.X) {   // the lean kernel is the whole world update: its on_tick handlers must be lane-local as well
      if (d.any_on_tick && (!tick.ok || tick.uses_target())) par = false;   // (an on_tick handler that uses itself: lane per env)
      for (int id : tick_sets)
        if (std::find(gset.begin(), gset.end(), id) == gset.end()) gset.push_back(id);
    }
    if (gset.size() > 4) par = false;
    // Two agents of an env side by side in the lean lane-per-env kernel (MgxDev::duo, mgx_world.h): the same conditions as the
    // lane-per-agent dispatch — every handler an action reaches stays with actor and target, move handlers look one cell
    // ahead, at most four game-scope stats are SET — without that kernel's shape limits.
    const bool duo = !d.X && sw.duo && d.A >= 2 && range1 && act.ok && act_sets.size() <= 4 && !par;
    // on_tick handlers that stay with their agent (no game-scope stat, no UseTarget, nothing that moves): the helper lanes
    // of the lean kernel may run them for half of the agents (MgxDev::tick_split)
    d.tick_split = (d.any_on_tick && !d.X && tick.ok && !tick.uses_target() && tick_sets.empty() && sw.tick_split) ? 1 : 0;
    d.act_par = par ? 1 : 0;
    d.act_tick = (par && !d.X) ? 1 : 0;
    d.duo = duo ? 1 : 0;
    d.coop_passes = (!d.X && sw.coop_passes) ? 1 : 0;
    d.act_replay = sw.act_replay ? 1 : 0;
    {  // MgxDev::move_fast: the move-handler table has the shape of the reference's default move — [0] relocate when the cell
       // ahead is empty, optionally [1] use the target when it is not, both one cell ahead — so the outcome of a move follows
       // from the grid entry ahead and its class's on_use alone (a class without on_use fails UseTarget with no side effect:
       // run_handler, the generated h1_L0).  Needs the paired dispatch's analysis (writes stay inside footprints) and the
       // deferred bookkeeping (a consumed action leaves a result byte, no stat update).
      const int n_hd = mgx_sec_cnt(P, MGX_SEC_HANDLERS), n_atoms = mgx_sec_cnt(P, MGX_SEC_ATOMS);
      auto leaf = [&](int h, int fop, int mop) {   // one filter atom `fop`, one mutation `mop`
        if (h < 0 || h >= n_hd) return false;
        const int32_t* hd = P + d.sec[MGX_SEC_HANDLERS] + h * MGX_HD_WORDS;
        const int pc = hd[MGX_HD_FILTER_PC];
        if (hd[MGX_HD_KIND] != MGX_HK_LEAF || hd[MGX_HD_MUT_COUNT] != 1 || pc < 0 || pc >= n_atoms) return false;
        const int32_t* a = P + d.sec[MGX_SEC_ATOMS] + pc * MGX_AT_WORDS;
        if (a[MGX_AT_OP] != fop || a[MGX_AT_ON_TRUE] != MGX_PC_PASS || a[MGX_AT_ON_FALSE] != MGX_PC_FAIL) return false;
        return (P + d.sec[MGX_SEC_MUTS] + hd[MGX_HD_MUT_START] * MGX_MU_WORDS)[MGX_MU_OP] == mop;
      };
      const int nm = d.n_move_handlers;
      bool mf = sw.move_fast && duo && d.defer_book && range1 && (nm == 1 || nm == 2) && mh[MGX_MH_ACCEPTS_EMPTY] != 0 &&
                leaf(mh[MGX_MH_HANDLER], MGX_FOP_TARGET_LOC_EMPTY, MGX_MOP_RELOCATE) &&
                (nm == 1 || leaf(mh[MGX_MH_WORDS + MGX_MH_HANDLER], MGX_FOP_TARGET_IS_USABLE, MGX_MOP_USE_TARGET));
      if (mf) {
        // LDS behind everything else of the kernel (the program copy included): an exact bitmap of the map up to 1 024 cells,
        // a 128-bit hashed mask above that or where only the bitmap would cost the kernel its fourth workgroup per CU (40 KB).
        // The fast path never moves a kernel across the 64 KB opt-in or past the CU's 160 KB: it stays off there.
        const size_t hw = (size_t)d.H * d.W, pre = ((size_t)d.A * MGX_WORLD_EPG + 15) & ~(size_t)15;
        const size_t cap = p.lds_world <= 64 * 1024 ? 64 * 1024 : 160 * 1024;
        int words = hw <= 1024 ? (int)((hw + 31) / 32) : 4;
        bool exact = hw <= 1024;
        if (exact && words > 4 && p.lds_world + pre + (size_t)4 * 4 * MGX_WORLD_EPG <= 40 * 1024 &&
            p.lds_world + pre + (size_t)4 * words * MGX_WORLD_EPG > 40 * 1024) { words = 4; exact = false; }
        if (p.lds_world + pre + (size_t)4 * words * MGX_WORLD_EPG > cap) mf = false;
        else {
          d.mf_lds_off = (int)p.lds_world;
          d.mf_dirty_words = words;
          d.mf_exact = exact ? 1 : 0;
          p.lds_world += pre + (size_t)4 * words * MGX_WORLD_EPG;
        }
      }
      d.move_fast = mf ? (nm == 1 ? 3 : 1) | (sw.mf_serial_book ? 4 : 0) : 0;
    }
    {  // MgxDev::act_kinds / act_args_lo / act_args_hi: the action table as three words, for shapes compiled into a kernel
      const int32_t* ac = P + d.sec[MGX_SEC_ACTIONS];
      bool fits = d.nact <= 16;
      uint32_t kinds = 0, lo = 0, hi = 0;
      for (int a = 0; fits && a < d.nact; a++) {
        const int kind = ac[a * MGX_AC_WORDS + MGX_AC_KIND], arg = ac[a * MGX_AC_WORDS + MGX_AC_ARG];
        if (kind < 0 || kind > 2 || arg < 0 || arg > 15) { fits = false; break; }
        kinds |= (uint32_t)kind << (2 * a);
        (a < 8 ? lo : hi) |= (uint32_t)arg << (4 * (a & 7));
      }
      d.act_kinds = fits ? (int)kinds : -1;
      d.act_args_lo = fits ? (int)lo : -1;
      d.act_args_hi = fits ? (int)hi : -1;
    }
    // game-stat SETs are applied in agent order through per-env cells (the paired dispatch too)
    const std::vector<int>& sets = par ? gset : duo ? act_sets : std::vector<int>();
    d.act_ngset = (int)sets.size();
    for (int k = 0; k < 4; k++) d.act_gset_ids[k] = k < (int)sets.size() ? sets[k] : -1;
    // integer bookkeeping: counters and coverage stats in the lean lane-per-env kernel (all or nothing: one fused pass),
    // counters only in the lane-per-agent dispatch kernels (bookkeeping_flush_one), none in the extended lane-per-env kernel
    if (d.act_par) d.shadow &= 1;
    else if (d.X || d.shadow != 3) d.shadow = 0;
    if (d.act_par) {  // footprint table + (maps up to 64 x 64) the cell map of the conflict lookup, per workgroup
      const int epg = d.X ? mgx_act_x_epg() : mgx_act_fast_epg();
      d.act_map = (d.H * d.W <= 4096 && sw.act_map) ? 1 : 0;
      d.act_lds_extra = ((4 * mgx_pow2_at_least(d.A) * epg + 15) & ~15) + (d.act_map ? epg * ((d.H * d.W + 15) & ~15) : 0);
      p.lds_act = (d.X ? mgx_act_x_lds_bytes(d.A, d.x_aoe_lds != 0, d.act_lds_extra) : mgx_act_fast_lds_bytes(d.A, d.act_lds_extra)) +
                  (p.prog_in_lds ? (size_t)p.prog_lds_words * 4 : 0);
    }
  }

  // ---- rewards and observation values ----
  // reward code made only of inventory / constant arithmetic reads nothing the observation kernel writes: evaluated early
  const bool rewards_pure = !d.X && !mgx_rewards_any(P, [](const int32_t* g) { return g[MGX_GV_OP] == MGX_GOP_STAT || mgx_gv_query(g); });
  // Extended games: the reward expressions may still be evaluated before the kernel's end — by a wavefront that has no
  // share of the encode — when no operand is something this kernel writes (the cell.visited agent stat, the token game
  // stats) and none is a query (those go through mgx_values_kernel).
  const bool rewards_safe = d.X && !mgx_rewards_any(P, [&](const int32_t* g) {
    const int id = g[MGX_GV_A1];
    if (mgx_gv_query(g)) return true;
    if (g[MGX_GV_OP] != MGX_GOP_STAT) return false;
    return g[MGX_GV_A0] != 1 ? id == d.wk[MGX_S_CELL_VISITED]
                             : id == d.wk[MGX_S_GAME_TOKENS_WRITTEN] || id == d.wk[MGX_S_GAME_TOKENS_FREE] || id == d.wk[MGX_S_GAME_TOKENS_DROPPED];
  });
  p.rmode = rewards_pure ? 1 : (rewards_safe && sw.rewards_mid) ? 2 : 0;
  p.rewards_ext = mgx_rewards_any(P, mgx_gv_query);
  for (int i = 0; i < d.n_obs_values; i++)
    if (mgx_value_any(P, i, mgx_gv_query)) p.obsval = true;
  if (!p.size_obs(sw)) return refuse(MGX_ERR_PROGRAM, MGX_OBS_LDS_REFUSAL);
  // The lean world kernel's preset instance (mgx_world_fast.hip): every field of its shape equal — gen_prog among them, so a program
  // on the interpreter (MGX_NO_GEN, other handler tables) never takes it — and the program copy in LDS, the one form it is built in.
  p.world_variant = 0;
  if (sw.world_preset && !d.X && !d.act_par && p.prog_in_lds && d.gen_prog == 3 && mgx_world_shape_matches<MgxWorldShapeR3>(d)) p.world_variant = 3;
  return MGX_OK;
}

#endif  // MGX_PLAN_H_
