// mgx_mapgen_plan.h — the host-only half of the mgx_set_map_*generator calls (include/mgx.h): checks a map
// recipe against the program's map shape and class count and decides everything the engine needs to accept it — the
// representative map its capacity checks run on, the generator kernel's LDS bytes, the recipe blob and the kernel's argument.
// No HIP call is made here, so the whole of it runs in a stand-alone program (tests/cpu_emu/mapgen_plan_check.cpp).
// Included by mgx_engine.hip.
#ifndef MGX_MAPGEN_PLAN_H_
#define MGX_MAPGEN_PLAN_H_

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "mgx.h"
#include "mgx_mapgen.h"

// What the planner knows of the engine: the program's map and class count, and the MGX_MAPGEN_LDS_BYTES variable (or null).
struct MgxMapWorld { int H, W, n_classes; const char* lds_bytes; };

// The recipe an engine holds: the kind and, of that kind, the generator kernel's argument.
enum { MGX_GEN_OFF = 0, MGX_GEN_RANDOM, MGX_GEN_SCENE, MGX_GEN_MAZE };
struct MgxMapRecipe {
  int kind = MGX_GEN_OFF;   // (off: mgx_step and the restarts enqueue nothing for the generator)
  MgxMapGen random{};       // only the one that `kind` names is filled
  MgxMapScene scene{};
  MgxMapMaze maze{};
  // The three device pointers of the kind's argument, into an uploaded blob of the layout below.
  void point_into(const void* blob, size_t off_rename, size_t off_off) {
    auto point = [&](const uint16_t*& cells, const uint16_t*& rename, const int32_t*& rename_off) {
      cells = (const uint16_t*)blob;
      rename = (const uint16_t*)((const uint8_t*)blob + off_rename);
      rename_off = (const int32_t*)((const uint8_t*)blob + off_off);
    };
    switch (kind) {
      case MGX_GEN_RANDOM: point(random.inner, random.rename, random.rename_off); break;
      case MGX_GEN_SCENE: point(scene.symbols, scene.rename, scene.rename_off); break;
      case MGX_GEN_MAZE: point(maze.symbols, maze.rename, maze.rename_off); break;
    }
  }
};

// What a planner entry decides about a recipe it accepts.
struct MgxMapPlan {
  MgxMapRecipe recipe;         // filled, its pointers still null
  // ONE generated map stands for all of them in the engine's capacity checks (AoE / territory source counts, the bound of
  // the observation token pool): every map of a recipe holds the same multiset of cells, and the renaming hands out the
  // same classes in another order.  Each entry says why its representative is such a map.
  std::vector<uint16_t> one;
  size_t lds = 0;              // dynamic LDS of the kind's kernel ...
  std::string lds_what;        // ... and what needs it, for the refusal
  std::vector<uint8_t> blob;   // cells | rename | rename_off, 16-byte aligned parts
  size_t off_rename = 0, off_off = 0;
};

inline int mgx_map_refusal(int code, const char* who, const std::string& msg, std::string& why) {
  why = std::string(who) + ": " + msg;
  return code;
}
template <class It>
inline int mgx_check_class_ids(const char* who, It first, It last, int nc, std::string& why) {
  for (; first != last; ++first)
    if ((int)*first < 0 || (int)*first > nc)
      return mgx_map_refusal(MGX_ERR_BAD_ARG, who, "class map holds id " + std::to_string((int)*first) + " but the program has " +
                                                        std::to_string(nc) + " classes", why);
  return MGX_OK;
}
// rename / rename_off of any recipe kind: shape, ascending offsets, class ids.
inline int mgx_check_rename_tables(const char* who, int nc, const uint16_t* rename, const int32_t* rename_off, int32_t n_teams, std::string& why) {
  auto refuse = [&](const std::string& msg) { return mgx_map_refusal(MGX_ERR_BAD_ARG, who, msg, why); };
  if (n_teams < 0 || n_teams > MGX_MAPGEN_MAX_TEAMS || (n_teams > 0 && (!rename || !rename_off)) || (n_teams > 0 && rename_off[0] != 0))
    return refuse("bad rename tables");
  for (int t = 0; t < n_teams; t++)
    if (rename_off[t + 1] < rename_off[t]) return refuse("rename offsets must ascend");
  return mgx_check_class_ids(who, rename, rename + (n_teams > 0 ? rename_off[n_teams] : 0), nc, why);
}
// The room grid of MapGen.prepare_grid (mapgen.py:305-315), in 64 bits: rows x cols for n_inst rooms, adding up to the program's map.
inline int mgx_check_room_grid(const MgxMapWorld& w, const char* who, int rh, int rw, int n_inst, int rows, int cols, int b, int ibw,
                               std::string& why) {
  int want_rows = 1;
  while ((long long)want_rows * want_rows < n_inst) want_rows++;
  const int want_cols = (n_inst + want_rows - 1) / want_rows;
  const long long wantH = (long long)rows * rh + (long long)(rows - 1) * ibw + 2LL * b, wantW = (long long)cols * rw + (long long)(cols - 1) * ibw + 2LL * b;
  if (rows != want_rows || cols != want_cols || wantH != w.H || wantW != w.W)
    return mgx_map_refusal(MGX_ERR_BAD_ARG, who,
                           std::to_string(n_inst) + " instances are a grid of " + std::to_string(want_rows) + " x " + std::to_string(want_cols) +
                               " rooms, and rooms, instance borders and the outer border must add up to the program's " + std::to_string(w.H) +
                               " x " + std::to_string(w.W) + " map (they give " + std::to_string(wantH) + " x " + std::to_string(wantW) + ")", why);
  return MGX_OK;
}
// The team cells of `cells` renamed in order: the k-th cell of team t becomes rename[rename_off[t] + k].  what: who names a team.
inline int mgx_rename_one_map(const char* who, const char* what, std::vector<uint16_t>& cells, const uint16_t* rename, const int32_t* rename_off,
                              int32_t n_teams, std::string& why) {
  auto refuse = [&](const std::string& msg) { return mgx_map_refusal(MGX_ERR_BAD_ARG, who, msg, why); };
  std::vector<int> seen((size_t)std::max(n_teams, 1), 0);
  for (uint16_t& v : cells) {
    if (v < MGX_MAPGEN_TEAM0) continue;
    const int t = v - MGX_MAPGEN_TEAM0;
    if (t >= n_teams) return refuse(std::string(what) + " names team " + std::to_string(t) + " of " + std::to_string(n_teams));
    const int k = seen[t]++;
    if (k >= rename_off[t + 1] - rename_off[t]) return refuse("more cells of team " + std::to_string(t) + " than entries in its rename table");
    v = rename[rename_off[t] + k];
  }
  return MGX_OK;
}
// The recipe blob: cells | rename | rename_off, 16-byte aligned parts.
inline void mgx_pack_map_recipe(MgxMapPlan& p, const uint16_t* cells, size_t n_cells, const uint16_t* rename, const int32_t* rename_off, int32_t n_teams) {
  const int n_rename = n_teams > 0 ? rename_off[n_teams] : 0;
  p.off_rename = (n_cells * 2 + 15) & ~(size_t)15;
  p.off_off = (p.off_rename + (size_t)n_rename * 2 + 15) & ~(size_t)15;
  p.blob.assign(p.off_off + ((size_t)n_teams + 1) * 4, 0);
  if (n_cells) memcpy(p.blob.data(), cells, n_cells * 2);
  if (n_rename) memcpy(p.blob.data() + p.off_rename, rename, (size_t)n_rename * 2);
  if (n_teams) memcpy(p.blob.data() + p.off_off, rename_off, ((size_t)n_teams + 1) * 4);
}
// The end of every entry, with p.one, p.lds and p.lds_what set: the representative's class ids, the LDS limit, the blob.
inline int mgx_finish_map_plan(const MgxMapWorld& w, const char* who, MgxMapPlan& p, const uint16_t* cells, size_t n_cells, const uint16_t* rename,
                               const int32_t* rename_off, int32_t n_teams, std::string& why) {
  const int rc = mgx_check_class_ids(who, p.one.begin(), p.one.end(), w.n_classes, why);
  if (rc) return rc;
  size_t lds_max = MGX_MAPGEN_LDS_MAX;
  // Test hook: a map of at most 255 x 255 cells needs 127 KB, so no program reaches the real limit; the tests of this refusal
  // lower it with MGX_MAPGEN_LDS_BYTES (a decimal byte count, only ever lowering).  Anything else in the variable is an error.
  if (const char* s = w.lds_bytes) {
    char* end = nullptr;
    const unsigned long long v = strtoull(s, &end, 10);
    if (end == s || *end || *s < '0' || *s > '9')
      return mgx_map_refusal(MGX_ERR_BAD_ARG, who, std::string("MGX_MAPGEN_LDS_BYTES = '") + s + "' is not a decimal byte count", why);
    lds_max = std::min<size_t>(lds_max, (size_t)v);
  }
  if (p.lds > lds_max)
    return mgx_map_refusal(MGX_ERR_PROGRAM, who, p.lds_what + " needs " + std::to_string(p.lds) + " B of LDS, the generator's workgroup has " +
                                                     std::to_string(lds_max), why);
  mgx_pack_map_recipe(p, cells, n_cells, rename, rename_off, n_teams);
  return MGX_OK;
}

// ---- the random builder (mgx_set_map_generator; inner != null) ----
// Its representative: a shuffle keeps the multiset of cells, so the unshuffled recipe is such a map.
inline int mgx_plan_map_random(const MgxMapWorld& w, const uint16_t* inner, int32_t n_inner, int32_t border_width, int32_t border_code,
                               const uint16_t* rename, const int32_t* rename_off, int32_t n_teams, const uint32_t* map_seed_base, MgxMapPlan& p,
                               std::string& why) {
  const char* who = "mgx_set_map_generator";
  p = MgxMapPlan{};
  const int ih = w.H - 2 * border_width, iw = w.W - 2 * border_width;
  if (!map_seed_base || border_width < 0 || ih <= 0 || iw <= 0 || n_inner != ih * iw)
    return mgx_map_refusal(MGX_ERR_BAD_ARG, who,
                           "the inner array must hold (H - 2 * border_width) * (W - 2 * border_width) = " +
                               std::to_string(ih > 0 && iw > 0 ? ih * iw : 0) + " cells of the program's " + std::to_string(w.H) + " x " +
                               std::to_string(w.W) + " map, and base seeds must be given", why);
  int rc = mgx_check_rename_tables(who, w.n_classes, rename, rename_off, n_teams, why);
  if (!rc) rc = mgx_check_class_ids(who, &border_code, &border_code + 1, w.n_classes, why);
  if (rc) return rc;
  std::vector<uint16_t> cells(inner, inner + n_inner);
  rc = mgx_rename_one_map(who, "an inner cell", cells, rename, rename_off, n_teams, why);
  if (rc) return rc;
  p.one.assign((size_t)w.H * w.W, (uint16_t)border_code);
  for (int i = 0; i < n_inner; i++) p.one[(size_t)(i / iw + border_width) * w.W + (i % iw + border_width)] = cells[(size_t)i];
  p.lds = ((size_t)n_inner * 2 + 15) & ~(size_t)15;
  p.lds_what = "the inner area of " + std::to_string(n_inner) + " cells";
  p.recipe.kind = MGX_GEN_RANDOM;
  MgxMapGen& g = p.recipe.random;
  g.n_inner = n_inner; g.ih = ih; g.iw = iw; g.border = border_width; g.H = w.H; g.W = w.W; g.n_teams = n_teams;
  g.border_code = (uint32_t)border_code;
  return mgx_finish_map_plan(w, who, p, inner, (size_t)n_inner, rename, rename_off, n_teams, why);
}

// ---- MapGen with a Random or a Maze instance scene (mgx_set_map_scene_generator, mgx_set_map_maze_generator) ----
// MazeGrid (mapgen/scenes/maze.py): the clamped sizes, the maze cells of a room and the walls between neighbouring cells
// (a wall as wide as the room's longer side or wider leaves one maze cell whatever its width: clamped, so that sums stay small).
struct MgxMazeGeometry { int rs, ws, mcols, mrows, cells, n_walls; };
inline MgxMazeGeometry mgx_maze_geometry(int rh, int rw, int room_size, int wall_size) {
  MgxMazeGeometry m;
  m.rs = std::max(1, std::min(room_size, std::min(rw, rh)));
  m.ws = std::min(std::max(1, wall_size), std::max(rw, rh));
  m.mcols = (rw + m.ws) / (m.rs + m.ws);
  m.mrows = (rh + m.ws) / (m.rs + m.ws);
  m.cells = m.mcols * m.mrows;
  m.n_walls = m.mcols * (m.mrows - 1) + (m.mcols - 1) * m.mrows;
  return m;
}
// A maze of the recipe that needs no draw, rh x rw: the comb (every wall between vertical neighbours open, between horizontal
// neighbours in the top row only).  Every maze of a recipe is a spanning tree of the same maze cells, so all hold as many wall
// and empty cells as this one.
inline std::vector<uint16_t> mgx_maze_comb(int rh, int rw, const MgxMazeGeometry& m, int algorithm, int wall_code) {
  const int p = m.rs + m.ws;
  std::vector<uint16_t> room((size_t)rh * rw);
  for (int i = 0; i < rh * rw; i++) {
    const int x = i % rw, y = i / rw;
    const bool strip = (x % p >= m.rs && x / p < m.mcols - 1) || (y % p >= m.rs && y / p < m.mrows - 1);
    const bool cell = x % p < m.rs && x / p < m.mcols && y % p < m.rs && y / p < m.mrows;
    const bool open_down = x % p < m.rs && x / p < m.mcols && y % p >= m.rs && y / p < m.mrows - 1;
    const bool open_right = y < m.rs && x % p >= m.rs && x / p < m.mcols - 1;
    const bool wall = algorithm == MGX_MAZE_KRUSKAL ? (strip && !open_down && !open_right) : !(cell || open_down || open_right);
    room[(size_t)i] = wall ? (uint16_t)wall_code : (uint16_t)0;
  }
  return room;
}
struct MgxMazeArgs { int32_t algorithm, room_size, wall_size, wall_code, key_offset; };
// Both kinds in one entry; mz: the maze's own arguments (null: the scene recipe, whose rooms start empty).  The
// representative: every symbol is always placed, so symbol q of an instance on the q-th empty cell of its room (a comb maze's
// room for the maze recipe) is a map of the recipe's multiset.
inline int mgx_plan_map_rooms(const MgxMapWorld& w, const MgxMazeArgs* mz, int32_t rh, int32_t rw, int32_t n_inst, int32_t rows,
                              int32_t cols, int32_t b, int32_t ibw, int32_t border_code, int32_t instance_border_code, int32_t first_on_root,
                              const uint16_t* symbols, int32_t n_sym, const uint16_t* rename, const int32_t* rename_off, int32_t n_teams,
                              const uint32_t* map_seed_base, MgxMapPlan& p, std::string& why) {
  const char* who = mz ? "mgx_set_map_maze_generator" : "mgx_set_map_scene_generator";
  auto refuse = [&](const std::string& msg) { return mgx_map_refusal(MGX_ERR_BAD_ARG, who, msg, why); };
  p = MgxMapPlan{};
  if (!map_seed_base || rh <= 0 || rw <= 0 || rh > w.H || rw > w.W || b < 0 || ibw < 0 || ibw > 0xFFFF || n_inst < 1 || rows < 1 || cols < 1 || n_sym < 0 ||
      (n_sym > 0 && !symbols) || (mz && mz->key_offset != 0 && mz->key_offset != 1))
    return refuse(std::string("null / negative argument, ") + (mz ? "a key offset other than 0 or 1, " : "") + "or base seeds not given");
  if (mz && mz->algorithm != MGX_MAZE_KRUSKAL && mz->algorithm != MGX_MAZE_DFS)
    return refuse("algorithm " + std::to_string(mz->algorithm) + " is neither kruskal (0) nor dfs (1)");
  int rc = mgx_check_room_grid(w, who, rh, rw, n_inst, rows, cols, b, ibw, why);
  if (rc) return rc;
  const int area = rh * rw, HW = w.H * w.W;
  const MgxMazeGeometry m = mz ? mgx_maze_geometry(rh, rw, mz->room_size, mz->wall_size) : MgxMazeGeometry{};
  if (mz && (m.mcols < 1 || m.mrows < 1 || m.n_walls > 0xFFFF))
    return refuse("a room of " + std::to_string(rh) + " x " + std::to_string(rw) + " holds " + std::to_string(m.mrows) + " x " +
                  std::to_string(m.mcols) + " maze cells");
  if (!mz && n_sym > area) return refuse(std::to_string(n_sym) + " symbols do not fit the " + std::to_string(area) + " cells of a room");
  rc = mgx_check_rename_tables(who, w.n_classes, rename, rename_off, n_teams, why);
  if (rc) return rc;
  const std::initializer_list<int32_t> codes = {border_code, instance_border_code, mz ? mz->wall_code : 0};
  rc = mgx_check_class_ids(who, codes.begin(), codes.end(), w.n_classes, why);
  if (rc) return rc;
  if (mz && mz->wall_code == 0) return refuse("the wall code is 0 (empty)");
  std::vector<uint16_t> room;   // maze: the comb's cells and, in row-major order, its empty ones (a scene's room is all empty)
  std::vector<int> empties;
  if (mz) {
    room = mgx_maze_comb(rh, rw, m, mz->algorithm, mz->wall_code);
    for (int i = 0; i < area; i++)
      if (!room[(size_t)i]) empties.push_back(i);
    if (n_sym > (int)empties.size())
      return refuse(std::to_string(n_sym) + " symbols do not fit the " + std::to_string(empties.size()) + " empty cells of a room's maze");
  }
  auto shape = [&](auto& g) {   // the fields MgxMapScene and MgxMapMaze have in common
    g.H = w.H; g.W = w.W; g.border = b; g.ibw = ibw; g.rh = rh; g.rw = rw; g.n_inst = n_inst; g.rows = rows; g.cols = cols;
    g.border_code = (uint32_t)border_code; g.iborder_code = (uint32_t)instance_border_code;
    g.n_sym = n_sym; g.n_teams = n_teams; g.first_on_root = first_on_root ? 1 : 0;
  };
  MgxMapScene s{};   // the scene kernel's argument; its frame is the frame of either kind's representative
  shape(s);
  p.one.resize((size_t)HW);
  for (int i = 0; i < HW; i++) p.one[(size_t)i] = (uint16_t)s.cell(i / w.W, i % w.W);
  for (int k = 0; k < n_inst; k++) {
    uint16_t* at = p.one.data() + (size_t)s.origin(k).y * w.W + s.origin(k).x;
    for (size_t i = 0; i < room.size(); i++) at[(i / rw) * w.W + i % rw] = room[i];
    for (int q = 0; q < n_sym; q++) {
      const int c = mz ? empties[(size_t)q] : q;
      at[(size_t)(c / rw) * w.W + c % rw] = symbols[(size_t)k * n_sym + q];
    }
  }
  rc = mgx_rename_one_map(who, "a symbol", p.one, rename, rename_off, n_teams, why);   // row-major over the whole map
  if (rc) return rc;
  p.lds_what = "the map of " + std::to_string(HW) + " cells with a room of " + std::to_string(area);
  p.recipe.kind = mz ? MGX_GEN_MAZE : MGX_GEN_SCENE;
  if (mz) {
    MgxMapMaze& z = p.recipe.maze;
    shape(z);
    z.key_offset = mz->key_offset; z.algorithm = mz->algorithm; z.rs = m.rs; z.ws = m.ws; z.mcols = m.mcols; z.mrows = m.mrows;
    z.n_walls = m.n_walls; z.n_work = std::max(m.n_walls, m.cells); z.wall_code = (uint32_t)mz->wall_code;
    p.lds = MGX_MAZE_LDS_BYTES(HW, z.n_work, m.cells, area, n_sym);
    p.lds_what += ", " + std::to_string(m.cells) + " maze cells, " + std::to_string(m.n_walls) + " walls";
  } else {
    p.recipe.scene = s;
    p.lds = MGX_MAPSCENE_LDS_BYTES(HW, area, n_sym);
  }
  p.lds_what += " and " + std::to_string(n_sym) + " symbols";
  return mgx_finish_map_plan(w, who, p, symbols, (size_t)n_inst * n_sym, rename, rename_off, n_teams, why);
}

#endif  // MGX_MAPGEN_PLAN_H_
