// TEST INFRASTRUCTURE ONLY — a stand-alone program for mettagrid_amd/csrc/mgx_agent_rules.h (the per-agent rules of the world
// kernels) on the emulated HIP runtime of this directory, built with AddressSanitizer + UndefinedBehaviorSanitizer and run by
// tests/test_agent_rules_host.py:
//   clang++ -std=c++17 -fsanitize=address,undefined -DMGX_CPU_EMU -I tests/cpu_emu -I include -I mettagrid_amd/csrc
//           tests/cpu_emu/agent_rules_check.cpp
// The domains are tiny, so every check is exhaustive.  Exit status 0 and "agent rules ok" when every rule below holds.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <set>

#include "mgx_device.h"
#include "mgx_world.h"   // mgx_move_target (includes mgx_agent_rules.h)

thread_local dim3 threadIdx, blockIdx, blockDim, gridDim;

static int g_failed = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) { if (g_failed < 20) fprintf(stderr, "line %d: %s\n", __LINE__, #cond); g_failed++; } \
  } while (0)

// ---- the three bytes: every field round-trips, and the layouts are the ones the kernels' comments promise ----
static void check_bytes() {
  CHECK(mgx_result_byte(MGX_AK_MOVE, true, false) == (1 | (1 << 1) | (1 << 3)));   // 1 | kind << 1 | ok << 3 | moved << 4
  CHECK(mgx_result_byte(MGX_AK_VIBE, false, true) == (1 | (2 << 1) | (1 << 4)));
  CHECK(mgx_outcome_byte(MGX_AK_MOVE, true, true) == (3u | (1u << 2) | (1u << 4) | (1u << 5)));   // 3 | kind << 2 | ok << 4 | moved << 5
  CHECK(mgx_pre_with_cell(mgx_resolved_byte(MGX_AK_MOVE, 5, true), true, true) == (2u | (1u << 2) | (5u << 4) | 0x80u));
  CHECK(!mgx_rb_called(0) && mgx_rb_stat(0, 10, 11, 12, 13, 14, 15) == -1 && !mgx_rb_failed(0));   // no call: an empty byte
  for (int kind = 0; kind < 3; kind++)
    for (int ok = 0; ok < 2; ok++)
      for (int moved = 0; moved < 2; moved++) {
        const uint32_t r = (uint32_t)(uint16_t)mgx_result_byte(kind, ok, moved);
        CHECK(r < 256 && mgx_rb_called(r) && mgx_rb_kind(r) == kind && mgx_rb_ok(r) == (ok != 0) && mgx_rb_moved(r) == (moved != 0));
        CHECK(mgx_rb_failed(r) == (ok == 0));
        CHECK(mgx_rb_stat(r, 10, 11, 12, 13, 14, 15) == 10 + 2 * kind + (ok ? 0 : 1));
        const uint32_t o = mgx_outcome_byte(kind, ok, moved);
        CHECK(o < 256 && mgx_is_outcome(o) && mgx_pre_kind(o) == kind && mgx_out_ok(o) == (ok != 0) && mgx_out_moved(o) == (moved != 0));
        CHECK((uint32_t)(uint16_t)mgx_result_byte(mgx_pre_kind(o), mgx_out_ok(o), mgx_out_moved(o)) == r);   // mf_book
      }
  for (int kind = 0; kind < 4; kind++)   // 3: MGX_PRE_GENERAL
    for (int orient = 0; orient < 8; orient++)
      for (int off = 0; off < 2; off++)
        for (int cell = 0; cell < 3; cell++) {
          const uint32_t w = mgx_pre_with_cell(mgx_resolved_byte(kind, orient, off), cell != 0, cell == 2);
          CHECK(w < 256 && !mgx_is_outcome(w) && mgx_pre_kind(w) == kind && mgx_pre_orient(w) == orient && mgx_pre_off_map(w) == (off != 0));
          CHECK(mgx_pre_cell(w) == (uint32_t)cell);
        }
  CHECK(MGX_PRE_EMPTY == 0 && MGX_PRE_NO_USE == 1 && MGX_PRE_ON_USE == 2 && MGX_PRE_GENERAL == 3);
}

// ---- orientation and footprint ----
// a plain restatement of the eight orientations: north, south, west, east, then the four diagonals NW NE SW SE; rows grow southwards
static const int kDr[8] = {-1, 1, 0, 0, -1, -1, 1, 1};
static const int kDc[8] = {0, 0, -1, 1, -1, 1, -1, 1};

static void check_orientation() {
  for (int o = 0; o < 8; o++) {
    CHECK(mgx_orient_dx(o) == kDc[o] && mgx_orient_dy(o) == kDr[o]);
    CHECK(mgx_orient_dx_packed(o) == mgx_orient_dx(o) && mgx_orient_dy_packed(o) == mgx_orient_dy(o));
  }
  CHECK(mgx_orient_dx(8) == 0 && mgx_orient_dy(8) == 0 && mgx_orient_dx(-1) == 0 && mgx_orient_dy(-1) == 0);
}

static void check_footprint(int H, int W) {
  using namespace MGX_TU_NS;
  // action 0: noop, 1..8: move in orientation 0..7, 9: change_vibe
  int32_t acts[10 * MGX_AC_WORDS] = {};
  acts[0 * MGX_AC_WORDS + MGX_AC_KIND] = MGX_AK_NOOP;
  for (int o = 0; o < 8; o++) { acts[(1 + o) * MGX_AC_WORDS + MGX_AC_KIND] = MGX_AK_MOVE; acts[(1 + o) * MGX_AC_WORDS + MGX_AC_ARG] = o; }
  acts[9 * MGX_AC_WORDS + MGX_AC_KIND] = MGX_AK_VIBE;
  acts[9 * MGX_AC_WORDS + MGX_AC_ARG] = 3;
  MgxDev d = {};
  d.H = H; d.W = W; d.nact = 10;
  for (int r = 0; r < H; r++)
    for (int c = 0; c < W; c++) {
      const uint32_t own = (uint32_t)((r << 8) | c);
      for (int a = -1; a <= 10; a++) {
        const int t = mgx_move_target<MgxWorldShapeDyn>(d, (const int32_t*)acts, a, own);
        int want = -1;   // restated: the cell one step ahead of a move, when it is on the map
        if (a >= 1 && a <= 8) {
          const int rr = r + kDr[a - 1], cc = c + kDc[a - 1];
          if (rr >= 0 && cc >= 0 && rr < H && cc < W) want = (rr << 8) | cc;
          CHECK(mgx_cell_ahead(own, a - 1, H, W) == want);
        }
        CHECK(t == want);
        const uint32_t F = mgx_footprint(own, t);
        CHECK(mgx_fp_own(F) == own && mgx_fp_target(F) == (t < 0 ? own : (uint32_t)t));
        CHECK(F == ((own << 16) | (want < 0 ? own : (uint32_t)want)));
      }
    }
  // two agents may run side by side exactly when no cell of one's footprint is acted on or left by the other
  const uint32_t A = mgx_footprint(0x0101, 0x0102), B = mgx_footprint(0x0103, 0x0102), C = mgx_footprint(0x0102, -1),
                 D = mgx_footprint(0x0001, 0x0101), E = mgx_footprint(0x0201, 0x0202);
  CHECK(!mgx_fp_disjoint(A, B));   // same target
  CHECK(!mgx_fp_disjoint(A, C));   // b stands on a's target
  CHECK(!mgx_fp_disjoint(A, D));   // b acts on a's cell
  CHECK(mgx_fp_disjoint(A, E) && mgx_fp_disjoint(E, A));
}

// ---- handle_action's bookkeeping: the deferred replays against a plain restatement of the rule ----
struct PlainAgent {   // what the rule touches, as the reference keeps it: a counter and eight stat cells
  uint32_t swm = 0;
  float stat[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // noop ok / failed, move ok / failed, vibe ok / failed, action.failed, max steps without motion
  bool max_set = false;
};
// one call of kind `kind` that succeeded or not, by an agent that did or did not change its cell since its last call
static void plain_call(PlainAgent& g, int kind, bool ok, bool moved) {
  if (!moved) {
    g.swm += 1;
    if ((float)g.swm > g.stat[7]) { g.stat[7] = (float)g.swm; g.max_set = true; }
  } else {
    g.swm = 0;
  }
  if (ok) g.stat[2 * kind] += 1.f;
  else { g.stat[2 * kind + 1] += 1.f; g.stat[6] += 1.f; }
}

static void check_replay() {
  uint32_t calls[13];   // every result byte, and "no call"
  int n = 0;
  calls[n++] = 0;
  for (int kind = 0; kind < 3; kind++)
    for (int ok = 0; ok < 2; ok++)
      for (int moved = 0; moved < 2; moved++) calls[n++] = (uint32_t)(uint16_t)mgx_result_byte(kind, ok, moved);
  const uint32_t swm_starts[4] = {0, 1, 5, 41}, max_starts[4] = {0, 1, 6, 100};
  for (int i0 = 0; i0 < 13; i0++)
    for (int i1 = 0; i1 < 13; i1++)
      for (uint32_t swm0 : swm_starts)
        for (uint32_t max0 : max_starts) {
          const uint32_t r0 = calls[i0], r1 = calls[i1];
          const uint4 a0 = make_uint4(3, 4, 5, 6), b0 = make_uint4(7, 8, 9, max0);
          // the rule, restated
          PlainAgent g;
          g.swm = swm0;
          const float start[8] = {3, 4, 5, 6, 7, 8, 9, (float)max0};
          for (int k = 0; k < 8; k++) g.stat[k] = start[k];
          for (uint32_t r : {r0, r1})
            if (r & 1u) plain_call(g, (int)((r >> 1) & 3u), (r & 8u) != 0, (r & 16u) != 0);
          // whole-record integer form (tail_shadow, bookkeeping_flush_one)
          uint32_t swm = swm0;
          const uint4 a = mgx_replay_cnt_lo(mgx_replay_cnt_lo(a0, r0), r1);
          const uint4 b = mgx_replay_cnt_hi(mgx_replay_cnt_hi(b0, r0, swm), r1, swm);
          const uint32_t got[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
          for (int k = 0; k < 8; k++) CHECK((float)got[k] == g.stat[k]);
          CHECK(swm == g.swm);
          // by halves, as tail_shadow_flat walks them: element u of the run is half u & 1 of a record, replayed by a lane of
          // its own from the bytes and the OLD counter; the counter itself is written by the pass behind
          uint4 half[2] = {a0, b0};
          for (int u = 0; u < 2; u++) {
            uint32_t s = swm0;
            half[u] = (u & 1) != 0 ? mgx_replay_cnt_hi(mgx_replay_cnt_hi(half[u], r0, s), r1, s)
                                   : mgx_replay_cnt_lo(mgx_replay_cnt_lo(half[u], r0), r1);
          }
          const uint32_t got_h[8] = {half[0].x, half[0].y, half[0].z, half[0].w, half[1].x, half[1].y, half[1].z, half[1].w};
          for (int k = 0; k < 8; k++) CHECK((float)got_h[k] == g.stat[k]);
          CHECK(mgx_replay_swm(mgx_replay_swm(swm0, r0), r1) == g.swm);
          // stat-row form (bookkeeping_flush, bookkeeping_flush_one): +1.f on the cell of each call, action.failed once
          // per failed call, the max cell set when a call raised it
          float row[8];
          for (int k = 0; k < 8; k++) row[k] = start[k];
          uint32_t swm_f = swm0;
          float mx = row[7];
          bool set_max = false;
          mgx_replay_max(r0, swm_f, mx, set_max);
          mgx_replay_max(r1, swm_f, mx, set_max);
          if (set_max) row[7] = mx;
          for (uint32_t r : {r0, r1}) {
            const int id = mgx_rb_stat(r, 0, 1, 2, 3, 4, 5);
            if (id >= 0) row[id] += 1.f;
            if (mgx_rb_failed(r)) row[6] += 1.f;
          }
          for (int k = 0; k < 8; k++) CHECK(row[k] == g.stat[k]);
          CHECK(swm_f == g.swm && set_max == g.max_set && (set_max || mx == (float)max0));
        }
}

// the LDS-side half at the agent's turn, then the replay of the byte it leaves: together one call of the rule
static void check_book_step() {
  for (uint32_t rc : {0x0101u, 0x0102u})
    for (uint32_t prev : {0x0101u, 0x0102u})
      for (uint32_t swm : {0u, 7u}) {
        const MgxBookStep s = mgx_book_step(rc, prev, swm);
        CHECK(s.moved == (rc != prev) && s.prev == rc && s.swm == (rc != prev ? 0u : swm + 1u));
        CHECK(mgx_swm_step(swm, s.moved) == s.swm);
        const uint32_t r = (uint32_t)(uint16_t)mgx_result_byte(MGX_AK_MOVE, true, s.moved);
        CHECK(mgx_replay_swm(swm, r) == s.swm);   // the HBM counter replayed from the byte ends where the LDS copy did
      }
}

// ---- Agent::track_coverage ----
static void check_coverage() {
  const int W = 40;   // bits of a row straddle a word
  std::set<uint32_t> visited;
  uint32_t seen[64] = {}, unique = 0, maxdist = 0;
  const uint32_t spawn = (5u << 8) | 7u;
  // a walk with a revisited cell (5,8 twice), new cells, and a new maximum distance in either direction
  const uint32_t walk[][2] = {{5, 7}, {5, 8}, {5, 7}, {5, 8}, {4, 8}, {0, 39}, {1, 0}, {20, 7}, {5, 7}};
  uint32_t want_max = 0;
  for (const auto& p : walk) {
    const uint32_t rc = (p[0] << 8) | p[1];
    const bool fresh = visited.insert(rc).second;
    const uint32_t dist = (uint32_t)(abs((int)p[0] - 5) + abs((int)p[1] - 7));
    if (dist > want_max) want_max = dist;
    const int bit = mgx_cov_bit(rc, W);
    CHECK(bit == (int)(p[0] * W + p[1]) && (bit >> 5) < 64);
    const uint32_t before = seen[bit >> 5];
    const MgxCoverage cv = mgx_coverage(rc, spawn, W, before, unique, maxdist);
    CHECK(cv.fresh == fresh);
    CHECK(cv.seen == (before | (1u << (bit & 31))) && (fresh || cv.seen == before));
    CHECK(cv.unique == (uint32_t)visited.size() && cv.maxdist == want_max);
    seen[bit >> 5] = cv.seen; unique = cv.unique; maxdist = cv.maxdist;
  }
  CHECK(unique == 6 && maxdist == 37);
}

int main() {
  check_bytes();
  check_orientation();
  check_footprint(3, 3);
  check_footprint(1, 5);
  check_replay();
  check_book_step();
  check_coverage();
  if (g_failed) { fprintf(stderr, "%d checks failed\n", g_failed); return 1; }
  printf("agent rules ok\n");
  return 0;
}
