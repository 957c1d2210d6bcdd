// mgx_agent_rules.h — the small per-agent rules of the world kernels, each stated ONCE: the orientation table, the cell
// footprint of the paired dispatch, the three bytes the passes hand each other (result, resolved, outcome), handle_action's
// bookkeeping (actions/action_handler.hpp:78-105) in its LDS-side, integer-record and stat-row forms, and track_coverage.
// Functions of values in registers: no MgxDev, no LDS pointers, no loads or stores — the callers (mgx_world.h, mgx_act.h,
// mgx_aoe_local.h) keep their loads, stores and batching.  Checked exhaustively on the host by
// tests/cpu_emu/agent_rules_check.cpp; the oracle keeps its own independent statement of these rules.
#ifndef MGX_AGENT_RULES_H_
#define MGX_AGENT_RULES_H_

#include <stdint.h>

#include "mgx_program.h"  // MGX_AK_*

#define MGX_RULE __host__ __device__ __forceinline__

// ---- orientation -> (dx, dy) (orientation.hpp:28-48): 0 north, 1 south, 2 west, 3 east, 4 NW, 5 NE, 6 SW, 7 SE ----
// Defined for 0..7 (every value a valid program's move argument takes); anything else is "no step" (0, 0).
MGX_RULE int mgx_orient_dx(int orient) {
  return (orient == 2 || orient == 4 || orient == 6) ? -1 : (orient == 3 || orient == 5 || orient == 7) ? 1 : 0;
}
MGX_RULE int mgx_orient_dy(int orient) {
  return (orient == 0 || orient == 4 || orient == 5) ? -1 : (orient == 1 || orient == 6 || orient == 7) ? 1 : 0;
}
// The same table as packed constants (dx + 1, dy + 1, two bits each): branch-free, for the pipelined run-ahead loop, which needs
// the deltas in front of its dirty-word addresses.  Defined for 0..7 ONLY (a larger value gives -1, -1).
MGX_RULE int mgx_orient_dx_packed(int orient) { return (int)((0x8885u >> (orient * 2)) & 3u) - 1; }
MGX_RULE int mgx_orient_dy_packed(int orient) { return (int)((0xa058u >> (orient * 2)) & 3u) - 1; }

// ---- cells and footprints.  A cell is (r << 8) | c. ----
// The cell one step ahead of `own` on an H x W map, -1 when it is off the map.
MGX_RULE int mgx_cell_ahead(uint32_t own, int orient, int H, int W) {
  const int r = (int)(own >> 8) + mgx_orient_dy(orient), c = (int)(own & 0xFF) + mgx_orient_dx(orient);
  return (r >= 0 && c >= 0 && r < H && c < W) ? ((r << 8) | c) : -1;
}
// Footprint of an action in the paired / lane-per-agent dispatch: own cell << 16 | the cell ahead of a move (target < 0: own cell)
MGX_RULE uint32_t mgx_footprint(uint32_t own, int target) { return (own << 16) | (target < 0 ? own : (uint32_t)target); }
MGX_RULE uint32_t mgx_fp_own(uint32_t F) { return F >> 16; }
MGX_RULE uint32_t mgx_fp_target(uint32_t F) { return F & 0xFFFFu; }
// b may run beside a (a first in the order): b does not stand on a's target, acts on neither a's cell nor a's target
MGX_RULE bool mgx_fp_disjoint(uint32_t Fa, uint32_t Fb) {
  return mgx_fp_own(Fb) != mgx_fp_target(Fa) && mgx_fp_target(Fb) != mgx_fp_own(Fa) && mgx_fp_target(Fb) != mgx_fp_target(Fa);
}

// ---- result byte: what a handle_action call leaves in place of the consumed action id (MgxALds::act); 0 = no call ----
enum { MGX_RB_CALLED = 1, MGX_RB_KIND_SHIFT = 1, MGX_RB_KIND_MASK = 3, MGX_RB_OK = 8, MGX_RB_MOVED = 16 };
MGX_RULE int16_t mgx_result_byte(int kind, bool ok, bool moved) {
  return (int16_t)(MGX_RB_CALLED | (kind << MGX_RB_KIND_SHIFT) | (ok ? MGX_RB_OK : 0) | (moved ? MGX_RB_MOVED : 0));
}
MGX_RULE bool mgx_rb_called(uint32_t r) { return (r & MGX_RB_CALLED) != 0; }
MGX_RULE int mgx_rb_kind(uint32_t r) { return (int)((r >> MGX_RB_KIND_SHIFT) & MGX_RB_KIND_MASK); }
MGX_RULE bool mgx_rb_ok(uint32_t r) { return (r & MGX_RB_OK) != 0; }
MGX_RULE bool mgx_rb_moved(uint32_t r) { return (r & MGX_RB_MOVED) != 0; }
MGX_RULE bool mgx_rb_failed(uint32_t r) { return (r & (MGX_RB_CALLED | MGX_RB_OK)) == MGX_RB_CALLED; }   // a call that failed
// The stat a call adds 1 to, picked from the six result counters (ids, or indices of ids); -1 without a call.
MGX_RULE int mgx_rb_stat(uint32_t r, int noop_ok, int noop_no, int move_ok, int move_no, int vibe_ok, int vibe_no) {
  const int kind = mgx_rb_kind(r);
  const bool ok = mgx_rb_ok(r);
  const int id = kind == MGX_AK_NOOP ? (ok ? noop_ok : noop_no) : kind == MGX_AK_MOVE ? (ok ? move_ok : move_no) : (ok ? vibe_ok : vibe_no);
  return mgx_rb_called(r) ? id : -1;
}

// ---- run-ahead (MgxDev::move_fast): the resolved byte of the staging pass and the outcome byte the pipelined loop writes over
// it.  Same kind bits in both; kind MGX_PRE_GENERAL = the general path (invalid index), cell MGX_PRE_DONE = an outcome byte ----
enum { MGX_PRE_EMPTY = 0, MGX_PRE_NO_USE = 1, MGX_PRE_ON_USE = 2, MGX_PRE_DONE = 3, MGX_PRE_CELL_MASK = 3,   // the cell ahead
       MGX_PRE_KIND_SHIFT = 2, MGX_PRE_KIND_MASK = 3, MGX_PRE_GENERAL = 3,
       MGX_PRE_ORIENT_SHIFT = 4, MGX_PRE_ORIENT_MASK = 7, MGX_PRE_OFF_MAP = 0x80,                              // resolved byte
       MGX_OUT_OK = 16, MGX_OUT_MOVED = 32 };                                                                  // outcome byte
// kind: MGX_AK_* or MGX_PRE_GENERAL; orient / off_map: of a move, else 0 / false; mgx_pre_with_cell adds the cell field
MGX_RULE uint32_t mgx_resolved_byte(int kind, int orient, bool off_map) {
  return (uint32_t)(kind << MGX_PRE_KIND_SHIFT) | ((uint32_t)orient & MGX_PRE_ORIENT_MASK) << MGX_PRE_ORIENT_SHIFT | (off_map ? MGX_PRE_OFF_MAP : 0u);
}
MGX_RULE uint32_t mgx_pre_with_cell(uint32_t w, bool occupied, bool on_use) {
  return w | (!occupied ? MGX_PRE_EMPTY : !on_use ? MGX_PRE_NO_USE : MGX_PRE_ON_USE);
}
MGX_RULE uint32_t mgx_pre_cell(uint32_t w) { return w & MGX_PRE_CELL_MASK; }
MGX_RULE int mgx_pre_kind(uint32_t w) { return (int)((w >> MGX_PRE_KIND_SHIFT) & MGX_PRE_KIND_MASK); }
MGX_RULE int mgx_pre_orient(uint32_t w) { return (int)((w >> MGX_PRE_ORIENT_SHIFT) & MGX_PRE_ORIENT_MASK); }
MGX_RULE bool mgx_pre_off_map(uint32_t w) { return (w & MGX_PRE_OFF_MAP) != 0; }
MGX_RULE uint32_t mgx_outcome_byte(int kind, bool ok, bool moved) {
  return MGX_PRE_DONE | (uint32_t)(kind << MGX_PRE_KIND_SHIFT) | (ok ? MGX_OUT_OK : 0u) | (moved ? MGX_OUT_MOVED : 0u);
}
MGX_RULE bool mgx_is_outcome(uint32_t o) { return (o & MGX_PRE_CELL_MASK) == MGX_PRE_DONE; }
MGX_RULE bool mgx_out_ok(uint32_t o) { return (o & MGX_OUT_OK) != 0; }
MGX_RULE bool mgx_out_moved(uint32_t o) { return (o & MGX_OUT_MOVED) != 0; }

// ---- handle_action's bookkeeping (action_handler.hpp:78-105) ----
MGX_RULE uint32_t mgx_swm_step(uint32_t swm, bool moved) { return moved ? 0u : swm + 1u; }   // steps_without_motion after a call
// The LDS-side half at the agent's turn (the pipelined run-ahead takes `moved` and leaves the counter to mf_book: mgx_swm_step)
struct MgxBookStep { bool moved; uint32_t prev, swm; };
MGX_RULE MgxBookStep mgx_book_step(uint32_t rc, uint32_t prev, uint32_t swm) {
  const bool moved = rc != prev;
  return MgxBookStep{moved, moved ? rc : prev, mgx_swm_step(swm, moved)};
}

// The deferred half: ONE call replayed from its result byte; a tick is its primary-stream byte, then its vibe-stream byte.  Into
// the integer record ag_cnt, two 16-byte halves (V4: x y z w): lo = noop ok | noop failed | move ok | move failed, hi = vibe ok |
// vibe failed | action.failed | max steps without motion — each a function of the byte (and swm) alone: the flat pass splits them.
template <class V4>
MGX_RULE V4 mgx_replay_cnt_lo(V4 a, uint32_t r) {
  if (!mgx_rb_called(r)) return a;
  const int kind = mgx_rb_kind(r);
  const uint32_t ok = mgx_rb_ok(r) ? 1u : 0u, no = ok ^ 1u;
  if (kind == MGX_AK_NOOP) { a.x += ok; a.y += no; }
  else if (kind == MGX_AK_MOVE) { a.z += ok; a.w += no; }
  return a;
}
MGX_RULE uint32_t mgx_replay_swm(uint32_t swm, uint32_t r) { return mgx_rb_called(r) ? mgx_swm_step(swm, mgx_rb_moved(r)) : swm; }
template <class V4>
MGX_RULE V4 mgx_replay_cnt_hi(V4 b, uint32_t r, uint32_t& swm) {
  if (!mgx_rb_called(r)) return b;
  swm = mgx_swm_step(swm, mgx_rb_moved(r));
  if (!mgx_rb_moved(r)) b.w = b.w > swm ? b.w : swm;
  const int kind = mgx_rb_kind(r);
  const uint32_t ok = mgx_rb_ok(r) ? 1u : 0u, no = ok ^ 1u;
  if (kind != MGX_AK_NOOP && kind != MGX_AK_MOVE) { b.x += ok; b.y += no; }
  b.z += no;
  return b;
}
// Into the stat row: the counter, the running max and whether a call raised it (the +1 cells: mgx_rb_stat / mgx_rb_failed)
MGX_RULE void mgx_replay_max(uint32_t r, uint32_t& swm, float& mx, bool& set_max) {
  if (!mgx_rb_called(r)) return;
  swm = mgx_swm_step(swm, mgx_rb_moved(r));
  if (!mgx_rb_moved(r) && (float)swm > mx) { mx = (float)swm; set_max = true; }
}

// ---- Agent::track_coverage (objects/agent.cpp:49-57) on loaded values; `seen`: word mgx_cov_bit >> 5 of the visited bitmap ----
MGX_RULE int mgx_cov_bit(uint32_t rc, int W) { return (int)(rc >> 8) * W + (int)(rc & 0xFF); }
struct MgxCoverage { uint32_t seen, unique, maxdist; bool fresh; };   // fresh: the cell was new (seen and unique changed)
MGX_RULE MgxCoverage mgx_coverage(uint32_t rc, uint32_t spawn, int W, uint32_t seen, uint32_t unique, uint32_t maxdist) {
  const int r = (int)(rc >> 8), c = (int)(rc & 0xFF);
  const uint32_t m = 1u << (mgx_cov_bit(rc, W) & 31);
  const bool fresh = !(seen & m);
  const int dr = (int)(spawn >> 8) - r, dc = c - (int)(spawn & 0xFF);
  const uint32_t dist = (uint32_t)((dr < 0 ? -dr : dr) + (dc < 0 ? -dc : dc));
  return MgxCoverage{seen | m, fresh ? unique + 1u : unique, maxdist > dist ? maxdist : dist, fresh};
}

#endif  // MGX_AGENT_RULES_H_
