// mgx_global_state.h — the whole state of every env as one token row, written on the device behind every step.
//
// The observation kernel gives a policy what each AGENT sees (a window, per-observer tokens).  A centralised critic, a league's
// value baseline or a tool that looks at all envs at once needs the env itself: PettingZoo's state().  The reference has a stub
// there (python/src/mettagrid/envs/pettingzoo_env.py:178-190 returns zeros); mgx_get_objects* serve it through the host, per
// list of envs.  Here one kernel behind the step writes, per env, the tokens of every object ON THE GRID into caller-owned
// device memory:
//
//   tokens       u32 [E][TG]   row | col << 8 | feature << 16 | value << 24 (as bytes: r, c, f, v); 0xFFFFFFFF behind the last
//   counts       u32 [E]       the UNTRUNCATED number of tokens (> TG: the row overflowed; nothing is stored outside it)
//   agent_start  i32 [E][A]    index of the first token of agent i's object, -1: excluded by the class filter or at / behind TG
//
// Objects come in row-major order of their cells (the grid decides what is on the map: a removed object has no cell); the
// tokens of one object are exactly the (feature, value) list the observation encoder emits for it to any observer
// (mgx_obs.h phase 0c; core/grid_object.cpp:178-203, objects/agent.cpp:142-154, observation_encoder.hpp:198-225): tags in
// ascending id, vibe if not 0, inventory items in iteration order as base digit + :pK digits, agents' group and id.  The
// per-observer tokens (cell.visited staleness, territory aoe_mask, location-0xFE globals) are not state and are left out.
//
//   mgx_global_state_kernel   one WAVEFRONT per env, four envs per 256-thread workgroup, no barrier inside the walk.  The wavefront
//                             walks the env's grid in 64-cell chunks (one coalesced 128-byte load); a lane with an occupied,
//                             included cell loads its slot's fields in one round (issued one chunk ahead of their use),
//                             counts its tokens, and a DPP scan plus the carry of the earlier chunks gives its offset.  The chunk's tokens are staged in the wavefront's
//                             LDS window and streamed to HBM as coalesced dword stores.  The tail is not rewritten: the
//                             engine keeps each row's previous length and only the span new end .. old end is filled.
//
//                             The small tables every token list is looked up in (class info, class tag lists, inventory
//                             feature ids) are staged in LDS once per workgroup, in front of the only workgroup barrier.
//
// The kernel only READS engine state; one wavefront owns one row: no atomics, no scratch.
#ifndef MGX_GLOBAL_STATE_H_
#define MGX_GLOBAL_STATE_H_

#include "mgx_obs.h"   // mgx_wave_incl_scan, MgxBase, MGX_MAX_ITEMS

#define MGX_GS_WINDOW 512   // staged tokens per wavefront and pass (2 KiB; four wavefronts: 8 KiB of LDS per workgroup)
#define MGX_GS_LDS_CLASSES 512    // class tables of at most this many classes ...
#define MGX_GS_LDS_CLS_TOK 1024   // ... and class tag lists of at most this many tokens are staged in LDS (5.5 KiB)

struct MgxGlobalState {
  uint32_t* tokens;          // [E][TG]   caller-owned device memory
  uint32_t* counts;          // [E]
  int32_t* agent_start;      // [E][A] or nullptr
  uint32_t* used;            // [E] tokens the last pass left in the row (engine-owned): everything behind them is 0xFFFFFFFF
  const uint8_t* include;    // [classes] device copy of the class filter (0: objects of the class emit nothing)
  int TG;
  int n_classes, n_cls_tok;  // entries of MgxDev::cls_tokinfo / cls_tok (and of `include`)
};

// Digits of the largest inventory amount (u16) in `base`: the per-item bound of the host's row bound.
inline int mgx_gs_amount_digits(int base) {
  int digits = 1;
  for (unsigned v = 65535u / (unsigned)base; v > 0; v /= (unsigned)base) digits++;
  return digits;
}

#ifndef MGX_CPU_EMU
// One object slot's fields as the kernel loads them: one round of independent loads per chunk, issued one chunk AHEAD of
// their use (the loads of chunk i + 1 are in flight while chunk i's tokens are built and stored).
struct MgxGsObj {
  uint32_t cls, vibe, agent_id, oflags;
  unsigned long long ord;
  uint4 r0, r1;                  // the 32-byte inventory row
  uint4 t0, t1;                  // the eight tag words (programs with per-object tags)
};
// word w of eight held as two uint4 (w is a constant wherever this is called: it folds to one register)
__device__ __forceinline__ uint32_t mgx_gs_word(const uint4& a, const uint4& b, int w) {
  switch (w) {
    case 0: return a.x; case 1: return a.y; case 2: return a.z; case 3: return a.w;
    case 4: return b.x; case 5: return b.y; case 6: return b.z; default: return b.w;
  }
}
__device__ __forceinline__ void mgx_gs_load(const MgxDev& d, int env, uint32_t gv, MgxGsObj& o) {
  o.cls = MGX_DEAD_CLASS; o.vibe = 0; o.agent_id = MGX_NO_AGENT; o.oflags = 0; o.ord = ~0ull;
  o.r0 = make_uint4(0u, 0u, 0u, 0u); o.r1 = o.r0; o.t0 = o.r0; o.t1 = o.r0;
  if (gv != 0) {
    const size_t so = (size_t)env * d.S + (gv - 1);
    o.cls = d.obj_cls[so];
    o.vibe = d.obj_vibe[so];
    o.agent_id = d.obj_agent[so];
    o.ord = d.obj_order[so];
    static_assert(MGX_INV_PITCH == 16, "inventory rows are two 16-byte words");
    o.r0 = ((const uint4*)(d.obj_inv + so * MGX_INV_PITCH))[0];
    o.r1 = ((const uint4*)(d.obj_inv + so * MGX_INV_PITCH))[1];
    if (d.obj_flags) o.oflags = d.obj_flags[so];
    static_assert(MGX_TAG_WORDS == 8, "tag rows are two 16-byte words");
    if (d.obj_tags) { o.t0 = ((const uint4*)(d.obj_tags + so * MGX_TAG_WORDS))[0]; o.t1 = ((const uint4*)(d.obj_tags + so * MGX_TAG_WORDS))[1]; }
  }
}

// env_mask (device, u8 [E]) or nullptr = all envs.
__global__ void __launch_bounds__(256) mgx_global_state_kernel(const MgxDev* __restrict__ dp, const MgxGlobalState g,
                                                               const uint8_t* __restrict__ env_mask) {
  const MgxDev& d = *dp;
  __shared__ uint32_t s_stage[256 / MGX_WAVE][MGX_GS_WINDOW];
  // what every object's token list is looked up in — per-class info and filter, the class tag lists, the inventory feature
  // ids — once per workgroup in LDS: in HBM each of them is one more dependent round trip per object, the feature ids one
  // per DIGIT of a serial loop (tables over these sizes are read where they are)
  __shared__ uint32_t s_cinfo[MGX_GS_LDS_CLASSES];
  __shared__ uint8_t s_inc[MGX_GS_LDS_CLASSES];
  __shared__ uint16_t s_ctok[MGX_GS_LDS_CLS_TOK];
  __shared__ int32_t s_feat[16 * MGX_IF_WORDS];
  // each lane's inventory row, word w of thread t at [w][t] (conflict-free): an item's amount is picked by its DYNAMIC id, and
  // picking it out of eight registers makes the compiler park the row in scratch
  __shared__ uint32_t s_inv[MGX_INV_PITCH / 2][256];
  const int lane = (int)threadIdx.x & (MGX_WAVE - 1), wave = (int)threadIdx.x / MGX_WAVE;
  const int env = (int)blockIdx.x * (256 / MGX_WAVE) + wave;
  const bool tables_in_lds = g.n_classes <= MGX_GS_LDS_CLASSES && g.n_cls_tok <= MGX_GS_LDS_CLS_TOK;
  {
    const int32_t* feat_g = d.P + d.sec[MGX_SEC_INV_FEATURES];
    for (int i = (int)threadIdx.x; i < d.R * MGX_IF_WORDS && i < 16 * MGX_IF_WORDS; i += 256) s_feat[i] = feat_g[i];
    if (tables_in_lds) {
      for (int i = (int)threadIdx.x; i < g.n_classes; i += 256) { s_cinfo[i] = d.cls_tokinfo[i]; s_inc[i] = g.include[i]; }
      for (int i = (int)threadIdx.x; i < g.n_cls_tok; i += 256) s_ctok[i] = d.cls_tok[i];
    }
  }
  __syncthreads();                             // the only workgroup barrier; from here on a wavefront is on its own
  if (env >= d.E) return;                      // (wavefront-uniform: the partial last workgroup)
  if (env_mask && !env_mask[env]) return;
  const uint32_t* cinfo_t = tables_in_lds ? s_cinfo : d.cls_tokinfo;   // start(16) | group(8) | ntags(6) | is_agent(1) | is_static(1)
  const uint8_t* inc_t = tables_in_lds ? s_inc : g.include;
  const uint16_t* ctok_t = tables_in_lds ? s_ctok : d.cls_tok;
  uint32_t* stage = s_stage[wave];
  const int HW = d.H * d.W, W = d.W, TG = g.TG, S = d.S;
  const MgxBase B((uint32_t)d.base);
  const int f_vibe = d.feat[MGX_F_VIBE], f_group = d.feat[MGX_F_GROUP], f_agent = d.feat[MGX_F_AGENT_ID], f_tag = d.feat[MGX_F_TAG];
  const bool dyn_tags = d.obj_tags != nullptr;
  const uint16_t* grid = d.grid + (size_t)env * HW;
  uint32_t* row = g.tokens + (size_t)env * TG;
  const uint32_t prev = g.used[env];
  // a cell word: 0 = empty, else slot + 1 (a word past the env's slots — never in a sound env — counts as empty: nothing is
  // read outside the env's rows)
  auto cell_word = [&](int idx) -> uint32_t { const uint32_t v = idx < HW ? grid[idx] : 0u; return v > (uint32_t)S ? 0u : v; };
  uint32_t carry = 0;                          // tokens of the chunks in front of this one (untruncated)
  uint32_t gv = cell_word(lane), gv_next = cell_word(MGX_WAVE + lane);
  MgxGsObj o;
  mgx_gs_load(d, env, gv, o);
  for (int base = 0; base < HW; base += MGX_WAVE) {
    const int cellidx = base + lane;
    // ---- the pipeline: the fields of the NEXT chunk's objects and the cell words of the one behind it ----
    MgxGsObj o_next;
    mgx_gs_load(d, env, gv_next, o_next);
    const uint32_t gv_next2 = cell_word(base + 2 * MGX_WAVE + lane);
    // ---- this lane's object ----
    bool have = false, is_static = false, is_agent = false, dyn = false;
    uint32_t cinfo = 0, live_mask = 0;
    const uint32_t vibe = o.vibe, agent_id = o.agent_id;
    unsigned long long ord = o.ord;
    {
      uint32_t* mine = &s_inv[0][threadIdx.x];
      mine[0 * 256] = o.r0.x; mine[1 * 256] = o.r0.y; mine[2 * 256] = o.r0.z; mine[3 * 256] = o.r0.w;
      mine[4 * 256] = o.r1.x; mine[5 * 256] = o.r1.y; mine[6 * 256] = o.r1.z; mine[7 * 256] = o.r1.w;
    }
    int n = 0, ntags = 0;
    if (gv != 0 && o.cls != MGX_DEAD_CLASS && o.cls < (uint32_t)g.n_classes && inc_t[o.cls]) {
      have = true;
      cinfo = cinfo_t[o.cls];
      is_static = (cinfo >> 31) != 0;
      is_agent = (cinfo & 0x40000000u) != 0;
      dyn = dyn_tags && !is_static;
      if (o.oflags & 2u) ord = ~0ull;          // created at run time without an ObservationEncoder: no inventory tokens
      ntags = (int)((cinfo >> 24) & 0x3Fu);
      if (dyn) {
        ntags = 0;
#pragma unroll
        for (int w = 0; w < MGX_TAG_WORDS; w++) ntags += __popc(mgx_gs_word(o.t0, o.t1, w));
      }
      n = ntags;
    }
    auto amount_of = [&](int item) -> uint32_t {   // (the lane's own words: program order, no fence)
      const uint32_t w = s_inv[item >> 1][threadIdx.x];
      return (item & 1) ? (w >> 16) : (w & 0xFFFFu);
    };
    if (have && !is_static) {
      n += (vibe != 0 ? 1 : 0) + (is_agent ? 2 : 0);
      bool live = true;
#pragma unroll
      for (int k = 0; k < MGX_MAX_ITEMS; k++) {
        const int item = (int)((ord >> (4 * k)) & 0xF);
        live = live && item != 0xF;
        if (live) { live_mask |= 1u << k; n += B.digits(amount_of(item)); }
      }
    }
    // ---- ordered compaction: offset of the lane's first token in the chunk, the chunk's total ----
    const int incl = mgx_wave_incl_scan(n);
    const int total = __builtin_amdgcn_readlane(incl, MGX_WAVE - 1);
    const int off = incl - n;
    if (gv != 0 && g.agent_start && agent_id < (uint32_t)d.A) {   // an agent's object (of an excluded class: -1)
      const uint32_t first = carry + (uint32_t)off;
      g.agent_start[(size_t)env * d.A + agent_id] = have && first < (uint32_t)TG ? (int32_t)first : -1;
    }
    // ---- the chunk's tokens, MGX_GS_WINDOW at a time: staged in LDS by their owners, streamed out by the wavefront ----
    const uint32_t loc = (uint32_t)(cellidx / W) | ((uint32_t)(cellidx % W) << 8);
    for (int w0 = 0; w0 < total && carry + (uint32_t)w0 < (uint32_t)TG; w0 += MGX_GS_WINDOW) {
      if (n > 0 && off < w0 + MGX_GS_WINDOW && off + n > w0) {
        int pos = off - w0;                    // window index of the lane's next token
        auto put = [&](uint32_t f, uint32_t v) {
          if ((unsigned)pos < (unsigned)MGX_GS_WINDOW) stage[pos] = loc | ((f & 0xFFu) << 16) | ((v & 0xFFu) << 24);
          pos++;
        };
        if (dyn) {                             // ascending tag id (core/grid_object.cpp:181-186)
#pragma unroll
          for (int wd = 0; wd < MGX_TAG_WORDS; wd++) {
            uint32_t m = mgx_gs_word(o.t0, o.t1, wd);
            while (m) { const int b = __ffs(m) - 1; m &= m - 1; put((uint32_t)f_tag, (uint32_t)(wd * 32 + b)); }
          }
        } else {
          const uint16_t* src = ctok_t + (cinfo & 0xFFFFu);   // class tag list: feature | tag id << 8
          for (int k = 0; k < ntags; k++) { const uint32_t t = src[k]; put(t & 0xFFu, t >> 8); }
        }
        if (!is_static) {
          if (vibe != 0) put((uint32_t)f_vibe, vibe);
#pragma unroll
          for (int k = 0; k < MGX_MAX_ITEMS; k++) {   // observation_encoder.hpp:198-225: base digit, then :pK digits
            if (live_mask & (1u << k)) {
              const int item = (int)((ord >> (4 * k)) & 0xF);
              const int32_t* F = s_feat + item * MGX_IF_WORDS;
              uint32_t rem = amount_of(item);
              put((uint32_t)F[0], B.lo(rem));
              rem = B.hi(rem);
              for (int pdig = 1; rem > 0 && pdig < MGX_IF_WORDS; pdig++) { put((uint32_t)F[pdig], B.lo(rem)); rem = B.hi(rem); }
            }
          }
          if (is_agent) {
            put((uint32_t)f_group, (cinfo >> 16) & 0xFFu);
            put((uint32_t)f_agent, agent_id);
          }
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();         // the window is complete before any lane reads it back
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const int nwin = min(total - w0, MGX_GS_WINDOW);
      for (int i = lane; i < nwin; i += MGX_WAVE) {
        const uint32_t k = carry + (uint32_t)(w0 + i);
        if (k < (uint32_t)TG) row[k] = stage[i];
      }
      __builtin_amdgcn_wave_barrier();         // ... and read back by every lane before the next window overwrites it
    }
    carry += (uint32_t)total;
    gv = gv_next; gv_next = gv_next2; o = o_next;
  }
  // ---- the tail: 0xFF from this pass's end to the previous pass's end; everything behind that is 0xFF already ----
  const uint32_t now = min(carry, (uint32_t)TG);
  for (uint32_t k = now + (uint32_t)lane; k < prev && k < (uint32_t)TG; k += MGX_WAVE) row[k] = 0xFFFFFFFFu;
  if (lane == 0) { g.used[env] = now; g.counts[env] = carry; }
}
#endif  // !MGX_CPU_EMU

#endif  // MGX_GLOBAL_STATE_H_
