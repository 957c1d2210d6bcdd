// TEST INFRASTRUCTURE ONLY — a stand-alone program for mettagrid_amd/csrc/mgx_mapgen_plan.h (the host-only half of the
// mgx_set_map_*generator calls), built with AddressSanitizer + UndefinedBehaviorSanitizer and run by
// tests/test_mapgen_plan_host.py:
//   clang++ -std=c++17 -fsanitize=address,undefined -DMGX_CPU_EMU -I tests/cpu_emu -I include -I mettagrid_amd/csrc
//           tests/cpu_emu/mapgen_plan_check.cpp
//   mapgen_plan_check RECIPES [LDS_BYTES]
// RECIPES: whitespace-separated decimal integers, one recipe per record; an ARRAY is its length followed by its values.
// LDS_BYTES: what the planner is given as the MGX_MAPGEN_LDS_BYTES variable (absent: unset).
//   record  = kind H W n_classes body n_teams ARRAY(rename) ARRAY(rename_off)       (H, W, n_classes: the program's)
//   kind 1  (mgx_set_map_generator)        body = border_width border_code n_inner ARRAY(inner)
//   kind 2  (mgx_set_map_scene_generator)  body = rooms first_on_root n_sym ARRAY(symbols)
//   kind 3  (mgx_set_map_maze_generator)   body = rooms algorithm room_size wall_size wall_code first_on_root key_offset n_sym ARRAY(symbols)
//   rooms   = room_height room_width n_inst rows cols border_width instance_border_width border_code instance_border_code
// An empty array is passed as a null pointer (as mettagrid_amd/engine.py does); base seeds are always given.
// Per record, on stdout: "refused CODE TEXT", or the four lines
//   ok kind K lds N off_rename A off_off B
//   what TEXT            (the phrase of the LDS refusal)
//   blob HEX             (the recipe blob's bytes)
//   one V V ...          (the representative map, H * W cells)
#include <hip/hip_runtime.h>

#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "mgx_mapgen_plan.h"

thread_local dim3 threadIdx, blockIdx, blockDim, gridDim;

static std::ifstream in;
static long long next() {
  long long v = 0;
  if (!(in >> v)) { fprintf(stderr, "recipes: a record ends early\n"); exit(2); }
  return v;
}
template <class T>
static std::vector<T> next_array() {
  std::vector<T> a((size_t)next());
  for (T& v : a) v = (T)next();
  return a;
}
template <class T>
static const T* ptr(const std::vector<T>& a) { return a.empty() ? nullptr : a.data(); }

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: mapgen_plan_check RECIPES [LDS_BYTES]\n"); return 2; }
  in.open(argv[1]);
  const uint32_t base = 0;
  long long kind;
  while (in >> kind) {
    MgxMapWorld w = {(int)next(), (int)next(), (int)next(), argc > 2 ? argv[2] : nullptr};
    int a[16] = {};
    const int n_args = kind == 1 ? 3 : kind == 2 ? 11 : 16;
    for (int i = 0; i < n_args; i++) a[i] = (int)next();
    const std::vector<uint16_t> cells = next_array<uint16_t>();
    const int n_teams = (int)next();
    const std::vector<uint16_t> rename = next_array<uint16_t>();
    const std::vector<int32_t> off = next_array<int32_t>();
    MgxMapPlan p;
    std::string why;
    int rc;
    if (kind == 1) {
      rc = mgx_plan_map_random(w, cells.data(), a[2], a[0], a[1], ptr(rename), ptr(off), n_teams, &base, p, why);
    } else if (kind == 2) {
      rc = mgx_plan_map_rooms(w, nullptr, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], ptr(cells), a[10], ptr(rename), ptr(off),
                              n_teams, &base, p, why);
    } else {
      const MgxMazeArgs mz = {a[9], a[10], a[11], a[12], a[14]};
      rc = mgx_plan_map_rooms(w, &mz, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[13], ptr(cells), a[15], ptr(rename), ptr(off),
                              n_teams, &base, p, why);
    }
    if (rc) { printf("refused %d %s\n", rc, why.c_str()); continue; }
    printf("ok kind %d lds %zu off_rename %zu off_off %zu\nwhat %s\nblob ", p.recipe.kind, p.lds, p.off_rename, p.off_off, p.lds_what.c_str());
    for (uint8_t b : p.blob) printf("%02x", b);
    printf("\none");
    for (uint16_t v : p.one) printf(" %d", v);
    printf("\n");
  }
  return 0;
}
