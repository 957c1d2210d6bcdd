// mgx_replay.h — per-step change log of a short list of WATCHED envs, written on the device (include/mgx.h mgx_set_replay).
//
// Reference: ReplayLogWriter (python/src/mettagrid/simulator/replay_log_writer.py) calls grid_objects() after every step and
// merges the dicts into per-object change series on the host.  Here the compare runs at the end of mgx_step, one workgroup of
// 256 per watched env, against a SHADOW of what was last logged, and only the changes are appended to the env's own region of
// a log in HBM; mettagrid_amd/replay.py turns drained words into the reference's replay dicts.
//
// Logged state of an object slot = MGX_RPL_SLOT_WORDS words in five groups (one bit of the event's field mask each):
//   CORE   [0] rc | class << 16 (MGX_DEAD_CLASS: unused slot)   [1] alive | vibe << 8 | agent index << 16 (0xFF: none)
//   INV    [2..3] the inventory order list (4-bit ids, 0xF ends)   [4..10] u16 amounts by resource id, absent keys as 0
//   TAGS   [11..18] tag bits
//   LIMITS [19..25] u16 effective limit by resource id (effective_limit of mgx_world.h), 0xFFFF = the class has none
//   AGENT  [26] executed action | success << 16   [27] f32 bits of this step's reward        (zero for non-agents)
// A slot at or behind the env's object count reads as an unused slot with every other word 0.
//
// Words of one step (all of it or nothing is written):
//   MGX_RPL_STEP | flags, current step, n event words
//   per slot with a change, ascending: slot | mask << 16, then the words of the groups in the mask, in group order
//   if the step left the env done: MGX_RPL_END | flags, current step
// A KEYFRAME step (the first logged step of an episode or of a freshly watched env) writes every live slot in full and sets
// the whole shadow — a slot that is not alive gets the words of an unused slot there, so that it is logged in full when
// it turns alive (the reader starts an episode from "every slot unused" too); behind the keyframe slots of a static class
// (the caller's static type ids) are skipped.  The words are a pure
// function of (shadow, state): mettagrid_amd/replay.py::encode_step restates them.
#ifndef MGX_REPLAY_H_
#define MGX_REPLAY_H_

#include "mgx_device.h"

#define MGX_RPL_THREADS 256
#define MGX_RPL_WAVES (MGX_RPL_THREADS / MGX_WAVE)

struct MgxRpl {
  const int32_t* envs;         // [n] the watched envs
  uint32_t* log;               // [n][words_per_env]
  uint32_t* cursor;            // [n] words used
  uint32_t* state;             // [n] MGX_RPL_ENV_* bits
  uint32_t* shadow;            // [n][MGX_RPL_SLOT_WORDS][S]: word k of all slots side by side
  const uint32_t* static_cls;  // bit c: class c has a static type id
  uint32_t words_per_env;
};

static_assert(MGX_MAX_OBJECT_SLOTS < 65536, "an event header is slot | field mask << 16");
static_assert(MGX_RPL_SLOT_WORDS == 28 && MGX_RPL_AMOUNT_WORDS * 2 >= MGX_MAX_RESOURCES, "replay slot layout");

#ifndef MGX_CPU_EMU
__device__ __forceinline__ int mgx_rpl_group_start(int g) { return g == 0 ? 0 : g == 1 ? 2 : g == 2 ? 11 : g == 3 ? 19 : 26; }
__device__ __forceinline__ int mgx_rpl_group_words(int g) { return g == 0 ? 2 : g == 1 ? 9 : g == 2 ? 8 : g == 3 ? 7 : 2; }
__device__ __forceinline__ uint32_t mgx_rpl_event_words(uint32_t mask) {
  return mask ? 1u + ((mask & 1) ? 2u : 0u) + ((mask & 2) ? 9u : 0u) + ((mask & 4) ? 8u : 0u) + ((mask & 8) ? 7u : 0u) + ((mask & 16) ? 2u : 0u) : 0u;
}

// The logged state of slot s (n: the env's object count) and whether it is alive / of a static class.
__device__ __forceinline__ void mgx_rpl_slot_state(const MgxDev& d, const MgxEnvX& e, const uint32_t* __restrict__ static_cls, int s, int n,
                                                   uint32_t (&w)[MGX_RPL_SLOT_WORDS], bool& alive, bool& is_static) {
#pragma unroll
  for (int k = 0; k < MGX_RPL_SLOT_WORDS; k++) w[k] = 0;
  alive = false; is_static = false;
  if (s >= n) { w[0] = (uint32_t)MGX_DEAD_CLASS << 16; return; }
  const size_t o = e.so(s);
  const uint32_t cls = d.obj_cls[o], ag = d.obj_agent[o];
  const uint8_t oflags = d.obj_flags ? d.obj_flags[o] : 0;
  const bool has_cls = cls != MGX_DEAD_CLASS;
  alive = has_cls && !(oflags & 1);
  is_static = has_cls && ((static_cls[cls >> 5] >> (cls & 31)) & 1u);
  w[0] = (uint32_t)d.obj_rc[o] | cls << 16;
  w[1] = (alive ? 1u : 0u) | (uint32_t)d.obj_vibe[o] << 8 | ag << 16;
  const unsigned long long ord = d.obj_order[o];
  w[2] = (uint32_t)ord; w[3] = (uint32_t)(ord >> 32);
  uint32_t present = 0;   // the keys of the inventory are the order list, whatever their amounts
  bool ended = false;
#pragma unroll
  for (int k = 0; k < MGX_MAX_RESOURCES; k++) {
    const uint32_t item = (uint32_t)((ord >> (4 * k)) & 0xF);
    ended = ended || item == 0xF;
    if (!ended) present |= 1u << item;
  }
  const MgxEnvX::InvRow row = e.inv_row(s);
#pragma unroll
  for (int q = 0; q < MGX_RPL_AMOUNT_WORDS; q++)
    w[4 + q] = (((present >> (2 * q)) & 1u) ? row.w[q] & 0xFFFFu : 0u) | (((present >> (2 * q + 1)) & 1u) ? row.w[q] & 0xFFFF0000u : 0u);
#pragma unroll
  for (int k = 0; k < MGX_TAG_WORDS; k++)
    w[11 + k] = d.obj_tags ? d.obj_tags[o * MGX_TAG_WORDS + k] : (has_cls ? (uint32_t)mgx_cls(d, (int)cls)[MGX_C_TAGS + k] : 0u);
#pragma unroll
  for (int r = 0; r < 2 * MGX_RPL_AMOUNT_WORDS; r++) {
    uint32_t lim = 0xFFFFu;
    if (r < MGX_MAX_RESOURCES && r < d.R && has_cls) {
      const int li = mgx_cls(d, (int)cls)[MGX_C_RES_LIMIT + r];
      if (li >= 0) lim = (uint32_t)e.effective_limit(row, d.P + d.sec[MGX_SEC_LIMITS] + li * MGX_L_WORDS);
    }
    w[19 + (r >> 1)] |= lim << (16 * (r & 1));
  }
  if (ag != MGX_NO_AGENT && has_cls) {
    const size_t a = e.ao((int)ag);
    w[26] = ((uint32_t)d.executed[a] & 0xFFFFu) | (d.success[a] ? 1u << 16 : 0u);
    w[27] = __float_as_uint(d.rewards[a]);
  }
}

// Field mask of slot s for this step; `sh` = the env's shadow, word k of slot s at sh[k * S + s].
__device__ __forceinline__ uint32_t mgx_rpl_slot_mask(const uint32_t (&w)[MGX_RPL_SLOT_WORDS], bool alive, bool is_static, bool key,
                                                      const uint32_t* __restrict__ sh, int S, int s) {
  if (key) return alive ? (MGX_RPL_M_CORE | MGX_RPL_M_INV | MGX_RPL_M_TAGS | MGX_RPL_M_LIMITS | (((w[1] >> 16) & 0xFF) != MGX_NO_AGENT ? MGX_RPL_M_AGENT : 0)) : 0u;
  if (is_static) return 0u;
  uint32_t mask = 0;
#pragma unroll
  for (int g = 0; g < MGX_RPL_GROUPS; g++) {
    bool diff = false;
#pragma unroll
    for (int k = 0; k < mgx_rpl_group_words(g); k++) diff = diff || sh[(size_t)(mgx_rpl_group_start(g) + k) * S + s] != w[mgx_rpl_group_start(g) + k];
    mask |= diff ? 1u << g : 0u;
  }
  return mask;
}

// One workgroup per watched env, at the end of mgx_step (rewards, executed, success, terminals / truncations are final).
__global__ void __launch_bounds__(MGX_RPL_THREADS) mgx_replay_kernel(const MgxDev* __restrict__ dp, const MgxRpl r) {
  const MgxDev& d = *dp;
  const int wi = (int)blockIdx.x, env = r.envs[wi], tid = (int)threadIdx.x, lane = tid & (MGX_WAVE - 1), wave = tid / MGX_WAVE;
  const int S = d.S;
  __shared__ uint32_t s_wsum[MGX_RPL_WAVES], s_cursor, s_not[2];
  const uint32_t st = r.state[wi], cur = r.cursor[wi], cap = r.words_per_env;
  // Simulation.is_done (simulator.py:145-146): every agent terminal, or every agent truncated
  if (tid < 2) s_not[tid] = 0;
  __syncthreads();
  for (int a = tid; a < d.A; a += MGX_RPL_THREADS) {
    if (!d.terminals[(size_t)env * d.A + a]) s_not[0] = 1;
    if (!d.truncations[(size_t)env * d.A + a]) s_not[1] = 1;
  }
  __syncthreads();
  const bool all_term = !s_not[0], all_trunc = !s_not[1], done = all_term || all_trunc;
  if (st & MGX_RPL_ENV_MUTED) {   // overflowed earlier in this episode: nothing until the next one starts
    if (done && tid == 0) r.state[wi] = (st & ~(uint32_t)MGX_RPL_ENV_MUTED) | MGX_RPL_ENV_KEYFRAME_NEXT;
    return;
  }
  const bool key = (st & MGX_RPL_ENV_KEYFRAME_NEXT) != 0;
  const int n = min((int)d.num_objs[env], S);
  const MgxEnvX e(d, d.P, env);
  uint32_t* sh = r.shadow + (size_t)wi * MGX_RPL_SLOT_WORDS * S;
  uint32_t* log = r.log + (size_t)wi * cap;
  // ---- pass 1: the words this step needs ----
  uint32_t cnt = 0;
  for (int s = tid; s < S; s += MGX_RPL_THREADS) {
    uint32_t w[MGX_RPL_SLOT_WORDS];
    bool alive, is_static;
    mgx_rpl_slot_state(d, e, r.static_cls, s, n, w, alive, is_static);
    cnt += mgx_rpl_event_words(mgx_rpl_slot_mask(w, alive, is_static, key, sh, S, s));
  }
  for (int o = MGX_WAVE / 2; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
  if (lane == 0) s_wsum[wave] = cnt;
  __syncthreads();
  uint32_t total = 0;
  for (int q = 0; q < MGX_RPL_WAVES; q++) total += s_wsum[q];
  __syncthreads();   // (s_wsum is reused by the scan below)
  const uint32_t need = MGX_RPL_STEP_WORDS + total + (done ? MGX_RPL_END_WORDS : 0u);
  if (need > cap || cur > cap - need) {   // does not fit: nothing of the step is written, the shadow stays
    if (tid == 0) r.state[wi] = MGX_RPL_ENV_OVERFLOW | (done ? MGX_RPL_ENV_KEYFRAME_NEXT : MGX_RPL_ENV_MUTED);
    return;
  }
  // ---- pass 2: events in ascending slot order; a chunk of 256 slots at a time, exclusive scan of their word counts ----
  if (tid == 0) s_cursor = cur + MGX_RPL_STEP_WORDS;
  for (int c0 = 0; c0 < S; c0 += MGX_RPL_THREADS) {
    const int s = c0 + tid;
    uint32_t w[MGX_RPL_SLOT_WORDS];
    bool alive = false, is_static = false;
    uint32_t mask = 0;
    if (s < S) {
      mgx_rpl_slot_state(d, e, r.static_cls, s, n, w, alive, is_static);
      mask = mgx_rpl_slot_mask(w, alive, is_static, key, sh, S, s);
    }
    const uint32_t c = mgx_rpl_event_words(mask);
    uint32_t incl = c;
    for (int o = 1; o < MGX_WAVE; o <<= 1) { const uint32_t v = __shfl_up(incl, o); if (lane >= o) incl += v; }
    if (lane == MGX_WAVE - 1) s_wsum[wave] = incl;
    __syncthreads();
    uint32_t off = s_cursor + incl - c, chunk = 0;
    for (int q = 0; q < MGX_RPL_WAVES; q++) { off += q < wave ? s_wsum[q] : 0u; chunk += s_wsum[q]; }
    if (s < S) {
      if (mask) {   // (off + c <= cur + 3 + total <= cap: inside the env's region)
        log[off++] = (uint32_t)s | mask << 16;
#pragma unroll
        for (int g = 0; g < MGX_RPL_GROUPS; g++)
          if ((mask >> g) & 1u) {
#pragma unroll
            for (int k = 0; k < mgx_rpl_group_words(g); k++) log[off++] = w[mgx_rpl_group_start(g) + k];
          }
      }
      const uint32_t upd = key ? (1u << MGX_RPL_GROUPS) - 1u : mask;   // a keyframe sets the whole shadow, dead and static slots too
      if (key && !alive) {   // ... a slot that is not alive as an unused one: whatever it holds is logged when it turns alive
#pragma unroll
        for (int k = 0; k < MGX_RPL_SLOT_WORDS; k++) w[k] = 0;
        w[0] = (uint32_t)MGX_DEAD_CLASS << 16;
      }
#pragma unroll
      for (int g = 0; g < MGX_RPL_GROUPS; g++)
        if ((upd >> g) & 1u) {
#pragma unroll
          for (int k = 0; k < mgx_rpl_group_words(g); k++) sh[(size_t)(mgx_rpl_group_start(g) + k) * S + s] = w[mgx_rpl_group_start(g) + k];
        }
    }
    __syncthreads();
    if (tid == 0) s_cursor += chunk;
  }
  if (tid == 0) {
    log[cur] = MGX_RPL_STEP | (key ? MGX_RPL_F_KEYFRAME : 0u);
    log[cur + 1] = d.step[env];
    log[cur + 2] = total;
    if (done) {
      log[cur + MGX_RPL_STEP_WORDS + total] = MGX_RPL_END | (all_term ? MGX_RPL_E_TERMINAL : 0u) | (all_trunc ? MGX_RPL_E_TRUNCATED : 0u);
      log[cur + MGX_RPL_STEP_WORDS + total + 1] = d.step[env];
    }
    r.cursor[wi] = cur + need;
    r.state[wi] = (st & MGX_RPL_ENV_OVERFLOW) | (done ? MGX_RPL_ENV_KEYFRAME_NEXT : 0u);
  }
}

// An episode of some envs is cut from outside a step (mgx_record_episodes, mgx_reset_envs*, mgx_load_envs / mgx_copy_envs):
// every watched env in `list` that is inside an episode gets an END marker with `flags` and starts over with a keyframe.
// One workgroup per watched env; its threads look for the env in the list.
__global__ void __launch_bounds__(MGX_RPL_THREADS) mgx_replay_mark_kernel(const MgxDev* __restrict__ dp, const MgxRpl r, const int32_t* __restrict__ list,
                                                                          int n_list, uint32_t flags) {
  const MgxDev& d = *dp;
  const int wi = (int)blockIdx.x, env = r.envs[wi], tid = (int)threadIdx.x;
  __shared__ uint32_t s_hit, s_not[2];
  if (tid == 0) s_hit = 0;
  if (tid < 2) s_not[tid] = 0;
  __syncthreads();
  for (int k = tid; k < n_list; k += MGX_RPL_THREADS) if (list[k] == env) s_hit = 1;
  for (int a = tid; a < d.A; a += MGX_RPL_THREADS) {
    if (!d.terminals[(size_t)env * d.A + a]) s_not[0] = 1;
    if (!d.truncations[(size_t)env * d.A + a]) s_not[1] = 1;
  }
  __syncthreads();
  if (tid != 0 || !s_hit) return;
  const uint32_t st = r.state[wi], cur = r.cursor[wi], cap = r.words_per_env;
  if (st & MGX_RPL_ENV_MUTED) { r.state[wi] = (st & ~(uint32_t)MGX_RPL_ENV_MUTED) | MGX_RPL_ENV_KEYFRAME_NEXT; return; }
  if (st & MGX_RPL_ENV_KEYFRAME_NEXT) return;   // its episode has ended already, or none has begun
  if (cap < MGX_RPL_END_WORDS || cur > cap - MGX_RPL_END_WORDS) { r.state[wi] = st | MGX_RPL_ENV_OVERFLOW | MGX_RPL_ENV_KEYFRAME_NEXT; return; }
  uint32_t* log = r.log + (size_t)wi * cap;
  log[cur] = MGX_RPL_END | flags | (!s_not[0] ? MGX_RPL_E_TERMINAL : 0u) | (!s_not[1] ? MGX_RPL_E_TRUNCATED : 0u);
  log[cur + 1] = d.step[env];
  r.cursor[wi] = cur + MGX_RPL_END_WORDS;
  r.state[wi] = st | MGX_RPL_ENV_KEYFRAME_NEXT;
}
#endif  // !MGX_CPU_EMU

#endif  // MGX_REPLAY_H_
