"""Replays of watched envs: the host side of the device recorder (include/mgx.h "Replays", csrc/mgx_replay.h).

* ``encode_step`` — the numpy restatement of what ``mgx_replay_kernel`` appends for one step: a pure function of the shadow
  (what was logged last) and a snapshot of the env (raw object records, per-agent rewards / executed action / success).
* ``ReplayAssembler`` — consumes drained words, across any number of drains, and yields one finished episode at a time as
  the replay dict MettaScope reads (format version 4, the schema of the reference's
  python/src/mettagrid/simulator/replay_log_writer.py).
* ``write_replay`` — JSON, zlib for ``.z``, gzip for ``.gz``.

Not recorded: ``animation_id`` is always 0; policy infos, talk and monologue fields are caller data and
hold their constant defaults.
"""
from __future__ import annotations

import gzip
import json
import zlib

import numpy as np

from .fmt import K

SLOT_WORDS, AMOUNT_WORDS, GROUPS = K.RPL_SLOT_WORDS, K.RPL_AMOUNT_WORDS, K.RPL_GROUPS
GROUP_START = (0, 2, 11, 19, 26)
GROUP_WORDS = (2, 9, 8, 7, 2)
ALL_OBJECT_GROUPS = K.RPL_M_CORE | K.RPL_M_INV | K.RPL_M_TAGS | K.RPL_M_LIMITS
DEAD_CLASS, NO_AGENT, MAXR = 0xFFFF, 0xFF, K.MAX_RESOURCES
MARK = 0xFFFF0000


def event_words(mask: int) -> int:
    return 1 + sum(GROUP_WORDS[g] for g in range(GROUPS) if (mask >> g) & 1) if mask else 0


class _Tables:
    """What the encoding needs from the compiled program: per class its type id, group, tags and limit records."""

    def __init__(self, prog) -> None:
        w = np.asarray(prog.words, dtype=np.int64)
        self.R = int(w[K.H_NUM_RESOURCES])
        self.S = int(w[K.H_MAX_OBJECTS])
        nc = int(w[K.H_NUM_CLASSES])
        coff = int(w[K.H_SECTION_BASE + 2 * K.SEC_CLASSES])
        loff = int(w[K.H_SECTION_BASE + 2 * K.SEC_LIMITS])
        moff = int(w[K.H_SECTION_BASE + 2 * K.SEC_MODS])
        self.cls = [w[coff + c * K.C_WORDS: coff + (c + 1) * K.C_WORDS] for c in range(nc)]
        self.limits = {}
        for C in self.cls:
            for r in range(self.R):
                li = int(C[K.C_RES_LIMIT + r])
                if li >= 0 and li not in self.limits:
                    L = w[loff + li * K.L_WORDS: loff + (li + 1) * K.L_WORDS]
                    m0, mc = int(L[K.L_MOD_START]), int(L[K.L_MOD_COUNT])
                    mods = [(int(w[moff + (m0 + i) * K.MOD_WORDS + K.MOD_ITEM]), int(w[moff + (m0 + i) * K.MOD_WORDS + K.MOD_BONUS]))
                            for i in range(mc)]
                    self.limits[li] = (int(L[K.L_MIN]), int(L[K.L_MAX]), mods)

    def effective_limit(self, li: int, amounts) -> int:
        """effective_limit of csrc/mgx_world.h (objects/inventory.hpp:26-40) over the raw amounts of the object."""
        lo, hi, mods = self.limits[li]
        s = sum(int(amounts[item]) * bonus for item, bonus in mods)
        return min(max(min(hi, max(lo, s)), 0), 65535)


def _tables(prog) -> _Tables:
    t = getattr(prog, "_replay_tables", None)
    if t is None:
        t = _Tables(prog)
        try:
            prog._replay_tables = t
        except Exception:
            pass
    return t


class Shadow:
    """Recorder state of one watched env: the last logged words of every slot and the keyframe / muted flags."""

    def __init__(self, prog, static_types=("wall",)) -> None:
        self.prog = prog
        self.t = _tables(prog)
        self.words = np.zeros((self.t.S, SLOT_WORDS), np.uint32)
        self.keyframe_next, self.muted, self.overflow = True, False, False
        tids = {i for i, n in enumerate(prog.type_names) if n in set(static_types)}
        self.static_cls = {c for c, C in enumerate(self.t.cls) if int(C[K.C_TYPE_ID]) in tids}


def slot_words(t: _Tables, rec, rewards, executed, success) -> np.ndarray:
    """The MGX_RPL_SLOT_WORDS logged words of one slot from its raw object record (None: a slot behind the object count)."""
    w = np.zeros(SLOT_WORDS, np.uint64)
    if rec is None:
        w[0] = DEAD_CLASS << 16
        return w.astype(np.uint32)
    cls, r, c, vibe, alive, agent = (int(rec[i]) for i in (1, 2, 3, 4, 5, 6))
    has_cls = cls != DEAD_CLASS
    ag = NO_AGENT if agent < 0 else agent
    w[0] = ((r << 8) | c) | (cls << 16)
    w[1] = (1 if alive else 0) | (vibe << 8) | (ag << 16)
    order = []
    for k in range(MAXR):
        item = int(rec[8 + k])
        if item < 0:
            break
        order.append(item)
    nib = order + [0xF] * (16 - len(order))
    o64 = sum(v << (4 * k) for k, v in enumerate(nib))
    w[2], w[3] = o64 & 0xFFFFFFFF, o64 >> 32
    amounts = [int(rec[8 + MAXR + k]) & 0xFFFF for k in range(MAXR)] + [0] * (2 * AMOUNT_WORDS - MAXR)
    for k in range(2 * AMOUNT_WORDS):
        if k in order:
            w[4 + (k >> 1)] |= amounts[k] << (16 * (k & 1))
    for k in range(K.TAG_WORDS):
        w[11 + k] = int(rec[8 + 2 * MAXR + k]) & 0xFFFFFFFF
    for k in range(2 * AMOUNT_WORDS):
        lim = 0xFFFF
        if k < t.R and has_cls:
            li = int(t.cls[cls][K.C_RES_LIMIT + k])
            if li >= 0:
                lim = t.effective_limit(li, amounts)
        w[19 + (k >> 1)] |= lim << (16 * (k & 1))
    if ag != NO_AGENT and has_cls:
        w[26] = (int(executed[ag]) & 0xFFFF) | ((1 << 16) if success[ag] else 0)
        w[27] = int(np.asarray(rewards[ag], dtype=np.float32).view(np.uint32))
    return w.astype(np.uint32)


def encode_step(shadow: Shadow, snapshot: dict, room: int | None = None) -> np.ndarray:
    """The words ``mgx_replay_kernel`` writes for one step of one env, and the shadow brought up to date.

    ``snapshot``: ``objects`` raw records [n, 42] (mgx_get_objects), ``rewards`` f32 [A], ``executed`` i32 [A], ``success``
    bool [A], ``step`` (current step after the step), ``terminals`` / ``truncations`` bool [A].  ``room``: words left in the
    env's log region (None: unbounded); a step that does not fit returns no words and mutes the shadow as the kernel does."""
    t = shadow.t
    all_term = bool(np.all(snapshot["terminals"]))
    all_trunc = bool(np.all(snapshot["truncations"]))
    done = all_term or all_trunc
    if shadow.muted:
        if done:
            shadow.muted, shadow.keyframe_next = False, True
        return np.zeros(0, np.uint32)
    key = shadow.keyframe_next
    objs = snapshot["objects"]
    n = min(len(objs), t.S)
    body, updates = [], []
    unused = slot_words(t, None, None, None, None)
    for s in range(t.S):
        rec = objs[s] if s < n else None
        if not key and rec is not None and int(rec[1]) in shadow.static_cls:
            continue   # (a static class: not looked at behind the keyframe)
        w = unused if rec is None else slot_words(t, rec, snapshot["rewards"], snapshot["executed"], snapshot["success"])
        cls = int(w[0]) >> 16
        if key:
            alive = int(w[1]) & 1
            mask = (ALL_OBJECT_GROUPS | (K.RPL_M_AGENT if ((int(w[1]) >> 16) & 0xFF) != NO_AGENT else 0)) if alive else 0
            upd = (1 << GROUPS) - 1
        elif cls != DEAD_CLASS and cls in shadow.static_cls:
            mask = upd = 0
        else:
            mask = 0
            for g in range(GROUPS):
                a, b = GROUP_START[g], GROUP_START[g] + GROUP_WORDS[g]
                if not np.array_equal(shadow.words[s, a:b], w[a:b]):
                    mask |= 1 << g
            upd = mask
        if mask:
            body.append(np.uint32(s | (mask << 16)))
            for g in range(GROUPS):
                if (mask >> g) & 1:
                    body.extend(w[GROUP_START[g]:GROUP_START[g] + GROUP_WORDS[g]])
        if key and not mask:
            w = unused   # a slot that is not alive enters the keyframe's shadow as an unused one: logged in full when it turns alive
        if upd:
            updates.append((s, upd, w))
    need = K.RPL_STEP_WORDS + len(body) + (K.RPL_END_WORDS if done else 0)
    if room is not None and need > room:
        shadow.overflow = True
        shadow.keyframe_next, shadow.muted = (True, False) if done else (False, True)
        return np.zeros(0, np.uint32)
    for s, upd, w in updates:
        for g in range(GROUPS):
            if (upd >> g) & 1:
                a, b = GROUP_START[g], GROUP_START[g] + GROUP_WORDS[g]
                shadow.words[s, a:b] = w[a:b]
    step = int(snapshot["step"])
    out = [K.RPL_STEP | (K.RPL_F_KEYFRAME if key else 0), step, len(body)] + [int(x) for x in body]
    if done:
        out += [K.RPL_END | (K.RPL_E_TERMINAL if all_term else 0) | (K.RPL_E_TRUNCATED if all_trunc else 0), step]
    shadow.keyframe_next = done
    return np.asarray(out, dtype=np.uint32)


def encode_end(shadow: Shadow, step: int, flags: int) -> np.ndarray:
    """The END marker of an episode cut from outside a step (``mgx_replay_mark_kernel``)."""
    if shadow.muted:
        shadow.muted, shadow.keyframe_next = False, True
        return np.zeros(0, np.uint32)
    if shadow.keyframe_next:
        return np.zeros(0, np.uint32)
    shadow.keyframe_next = True
    return np.asarray([K.RPL_END | flags, step], dtype=np.uint32)


def parse_words(words) -> list:
    """Drained words -> [("step", flags, step, [(slot, mask, {group: words})]) | ("end", flags, step)]."""
    w = np.asarray(words, dtype=np.uint32)
    out, i = [], 0
    while i < len(w):
        tag, flags = int(w[i]) & MARK, int(w[i]) & 0xFFFF
        if tag == K.RPL_END:
            out.append(("end", flags, int(w[i + 1])))
            i += K.RPL_END_WORDS
        elif tag == K.RPL_STEP:
            step, nw = int(w[i + 1]), int(w[i + 2])
            i += K.RPL_STEP_WORDS
            end, events = i + nw, []
            while i < end:
                slot, mask = int(w[i]) & 0xFFFF, int(w[i]) >> 16
                i += 1
                groups = {}
                for g in range(GROUPS):
                    if (mask >> g) & 1:
                        groups[g] = w[i:i + GROUP_WORDS[g]]
                        i += GROUP_WORDS[g]
                events.append((slot, mask, groups))
            if i != end:
                raise ValueError("replay log: a step's events run past its word count")
            out.append(("step", flags, step, events))
        else:
            raise ValueError(f"replay log: unknown marker word {int(w[i]):#010x} at {i}")
    return out


def _default_for(value):
    if isinstance(value, list):
        return []
    if isinstance(value, bool):   # (the reference tests int first, and bool is an int: False == 0 either way)
        return 0
    if isinstance(value, int):
        return 0
    if isinstance(value, float):
        return 0.0
    if isinstance(value, str):
        return ""
    raise ValueError(f"no default for {type(value)}")


class _Episode:
    """The reference's EpisodeReplay merge rules over per-step object dicts."""

    def __init__(self, static_types) -> None:
        self.objects, self.index, self.step = [], {}, 0
        self.static_types = set(static_types)

    def log_step(self, updates: dict) -> None:
        """``updates``: {object id: update dict} of the objects present this step (static ones only at step 0)."""
        seen = set()
        for oid, upd in updates.items():
            idx = self.index.get(oid)
            if idx is None:
                idx = self.index[oid] = len(self.objects)
                self.objects.append({} if self.step == 0 else {"alive": [[0, False]]})
            seen.add(idx)
            obj = self.objects[idx]
            for key, value in upd.items():
                if key not in obj:
                    obj[key] = [[0, value]] if self.step == 0 else [[0, _default_for(value)], [self.step, value]]
                elif obj[key][-1][1] != value:
                    obj[key].append([self.step, value])
            for key in obj:
                if key not in upd:
                    last = obj[key][-1][1]
                    if last != _default_for(last):
                        obj[key].append([self.step, _default_for(last)])
        if self.step > 0:
            for idx in self.index.values():
                if idx in seen:
                    continue
                obj = self.objects[idx]
                tn = obj.get("type_name")
                if tn and tn[-1][1] in self.static_types:
                    continue
                if obj.get("alive") and obj["alive"][-1][1] is not False:
                    obj["alive"].append([self.step, False])
        self.step += 1

    def finish(self) -> list:
        out = []
        for obj in self.objects:
            out.append({k: (v[0][1] if len(v) == 1 else v) for k, v in obj.items()})
        return out


class ReplayAssembler:
    """Drained words of ONE watched env -> finished episodes as version-4 replay dicts.

    ``feed(words)`` may be called with the words of any number of drains, cut anywhere between steps; it returns the
    episodes that ended within them.  ``capacity_groups``: {group name: [resource names]} of the first agent's inventory
    limits (the reference's ``capacity_names``); without it the first agent's explicit limits are named by their resources.
    ``mg_config`` / ``policy_env_interface``: taken from a caller that has a reference config, else left out."""

    def __init__(self, prog, static_types=("wall",), capacity_groups: dict | None = None, mg_config=None,
                 policy_env_interface=None, seed: int | None = None) -> None:
        self.prog, self.t = prog, _tables(prog)
        self.static_types = tuple(static_types)
        if capacity_groups is None:
            capacity_groups = {"+".join(lim.resources): list(lim.resources) for lim in prog.spec.agents[0].inventory.limits} if prog.spec.agents else {}
        self.capacity_names = sorted(capacity_groups)
        self.res_to_cap = {}
        for cid, name in enumerate(self.capacity_names):
            for rn in capacity_groups[name]:
                if rn in prog.resource_names:
                    self.res_to_cap[prog.resource_names.index(rn)] = cid
        self.mg_config, self.policy_env_interface, self.seed = mg_config, policy_env_interface, seed
        self.state = np.zeros((self.t.S, SLOT_WORDS), np.uint32)   # the logged state, rebuilt from the events
        self.state[:, 0] = DEAD_CLASS << 16
        self.known = np.zeros(self.t.S, bool)
        self.ep = None
        self.total = None
        self.pending = np.zeros(0, np.uint32)
        self.last_end_flags = 0

    # ---- one object's update dict from its logged words (format_grid_object of the reference) ----
    def _update(self, slot: int, w) -> dict:
        cls = int(w[0]) >> 16
        C = self.t.cls[cls]
        rc = int(w[0]) & 0xFFFF
        order = []
        o64 = int(w[2]) | (int(w[3]) << 32)
        for k in range(MAXR):
            item = (o64 >> (4 * k)) & 0xF
            if item == 0xF:
                break
            order.append(item)
        amount = lambda base, k: (int(w[base + (k >> 1)]) >> (16 * (k & 1))) & 0xFFFF   # noqa: E731
        caps = {}
        for r in range(self.t.R):
            if int(C[K.C_RES_LIMIT + r]) >= 0:
                cid = self.res_to_cap.get(r)
                if cid is not None and cid not in caps:
                    caps[cid] = amount(19, r)
        upd = {"id": slot + 1, "alive": True, "type_name": self.prog.type_names[int(C[K.C_TYPE_ID])],
               "location": [rc & 0xFF, rc >> 8], "orientation": 0,
               "inventory": [[k, amount(4, k)] for k in sorted(order)], "inventory_max": 0,
               "inventory_capacities": [[c, v] for c, v in sorted(caps.items())], "color": 0,
               "tag_ids": [t for t in range(256) if (int(w[11 + (t >> 5)]) >> (t & 31)) & 1]}
        ag = (int(w[1]) >> 16) & 0xFF
        if ag != NO_AGENT:
            reward = float(np.asarray(w[27], dtype=np.uint32).view(np.float32))
            self.step_rewards[ag] = reward
            vibe = (int(w[1]) >> 8) & 0xFF
            upd.update({"is_agent": True, "agent_id": ag, "vision_size": 13, "action_id": int(w[26]) & 0xFFFF, "action_param": 0,
                        "action_success": bool((int(w[26]) >> 16) & 1), "animation_id": 0, "current_reward": reward,
                        "total_reward": None, "group_id": int(C[K.C_GROUP]), "vibe_id": vibe, "vibe": vibe,
                        "monologue_append": "", "monologue_reset": False})
        return upd

    def _is_static(self, w) -> bool:
        cls = int(w[0]) >> 16
        return cls != DEAD_CLASS and self.prog.type_names[int(self.t.cls[cls][K.C_TYPE_ID])] in self.static_types

    def _step(self, flags: int, events) -> None:
        key = bool(flags & K.RPL_F_KEYFRAME)
        if key:
            self.ep = _Episode(self.static_types)
            self.total = np.zeros(self.prog.num_agents, np.float64)
            self.state[:] = 0
            self.state[:, 0] = DEAD_CLASS << 16
            self.known[:] = False
        if self.ep is None:
            return   # words of an episode whose start was not logged
        for slot, mask, groups in events:
            for g, ws in groups.items():
                self.state[slot, GROUP_START[g]:GROUP_START[g] + GROUP_WORDS[g]] = ws
            self.known[slot] = True
        self.step_rewards = np.zeros(self.prog.num_agents, np.float64)
        updates = {}
        for slot in np.nonzero(self.known)[0]:
            w = self.state[slot]
            if not (int(w[1]) & 1):
                continue   # not alive: absent from grid_objects()
            if self.ep.step > 0 and self._is_static(w):
                continue
            updates[int(slot) + 1] = self._update(int(slot), w)
        self.total += self.step_rewards   # f64 sum of the f32 step rewards, as the reference accumulates them
        for upd in updates.values():
            if "agent_id" in upd:
                upd["total_reward"] = float(self.total[upd["agent_id"]])
        self.ep.log_step(updates)

    def _finish(self, flags: int, steps: int) -> dict:
        p, w = self.prog, self.prog.words
        out = {"version": 4, "action_names": list(p.action_names), "animation_names": ["none", "bump"],
               "item_names": list(p.resource_names), "type_names": list(p.type_names), "capacity_names": list(self.capacity_names),
               "tags": {n: i for i, n in enumerate(p.tag_names)}, "map_size": [int(w[K.H_WIDTH]), int(w[K.H_HEIGHT])],
               "num_agents": int(p.num_agents), "max_steps": self.ep.step}
        if self.mg_config is not None:
            out["mg_config"] = self.mg_config
        if self.policy_env_interface is not None:
            out["policy_env_interface"] = self.policy_env_interface
        out["objects"] = self.ep.finish()
        att = {"map_w": int(w[K.H_WIDTH]), "map_h": int(w[K.H_HEIGHT]), "steps": int(steps), "max_steps": int(w[K.H_MAX_STEPS])}
        if self.seed is not None:
            att["seed"] = int(self.seed)
        out["infos"] = {"attributes": att, "episode_rewards": self.total.tolist(), "end_flags": int(flags)}
        self.ep, self.total = None, None
        return out

    def feed(self, words) -> list:
        """Consume drained words; returns the replay dicts of the episodes that ended in them."""
        done = []
        for item in parse_words(words):
            if item[0] == "step":
                self._step(item[1], item[3])
            elif self.ep is not None:
                done.append(self._finish(item[1], item[2]))
        return done

    def partial(self):
        """The episode under way as a replay dict (None when there is none); the assembler keeps going."""
        if self.ep is None:
            return None
        import copy
        ep, total = copy.deepcopy(self.ep), self.total.copy()
        out = self._finish(0, self.ep.step)
        self.ep, self.total = ep, total
        return out


def write_replay(replay: dict, path: str) -> None:
    """``replay`` as JSON: zlib for ``.z``, gzip for ``.gz`` (the reference's choice by extension), plain otherwise."""
    data = json.dumps(replay).encode("utf-8")
    if path.endswith(".gz"):
        data = gzip.compress(data)
    elif path.endswith(".z"):
        data = zlib.compress(data)
    with open(path, "wb") as f:
        f.write(data)


def read_replay(path: str) -> dict:
    data = open(path, "rb").read()
    if path.endswith(".gz"):
        data = gzip.decompress(data)
    elif path.endswith(".z"):
        data = zlib.decompress(data)
    return json.loads(data.decode("utf-8"))
