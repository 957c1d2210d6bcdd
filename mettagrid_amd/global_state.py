"""Global state rows: the numpy restatement of the contract of include/mgx.h ``mgx_set_global_state`` (kernel:
csrc/mgx_global_state.h) and the helpers that read such rows.  Nothing here needs a GPU.

A row holds the tokens of every object on an env's grid, one uint32 per token: ``row | col << 8 | feature << 16 |
value << 24`` (as bytes ``(r, c, f, v)``), ``0xFFFFFFFF`` behind the last one.  Objects come in row-major order of their
cells; the tokens of one object are what the observation encoder emits for it to any observer (core/grid_object.cpp:178-203,
objects/agent.cpp:142-154, observation_encoder.hpp:198-225): tags in ascending id, ``vibe`` if not 0, the inventory items in
iteration order (base digit, then the ``:pK`` digits in ``token_value_base``), and for agents ``agent:group`` and ``agent_id``.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from .fmt import K

EMPTY = 0xFFFFFFFF
_MAXR = 13          # MGX_MAX_RESOURCES: the raw object record's order / amount columns (include/mgx.h mgx_get_objects)
_GLOBAL_LOC, _PAD_LOC = 0xFE, 0xFF

ExpectedRow = namedtuple("ExpectedRow", "tokens count agent_start")


def _classes(prog):
    """The program's class records, and per class what ``object_tokens`` needs of it (built once per program)."""
    cached = prog.__dict__.get("_gs_classes")
    if cached is None:
        w = prog.words
        off = int(w[K.H_SECTION_BASE + 2 * K.SEC_CLASSES])
        n = int(w[K.H_NUM_CLASSES])
        cached = prog.__dict__["_gs_classes"] = [w[off + c * K.C_WORDS: off + (c + 1) * K.C_WORDS] for c in range(n)]
    return cached


def _tag_tokens(f_tag: int, words) -> list:
    return [(f_tag, 32 * i + b) for i, x in enumerate(words) if int(x) for b in range(32) if (int(x) >> b) & 1]


def class_include(prog, exclude=()) -> np.ndarray:
    """The class filter u8 [classes] that leaves out ``exclude``: class ids, map cell names (aliases included; a team's cell
    name covers its per-agent classes) or type names such as ``"wall"``.  ValueError for a name the program does not know."""
    classes = _classes(prog)
    inc = np.ones(len(classes), np.uint8)
    for x in exclude:
        if isinstance(x, (int, np.integer)):
            if not 0 <= int(x) < len(classes):
                raise ValueError(f"global state filter: class id {x} out of range [0, {len(classes)})")
            ids = [int(x)]
        else:
            name = str(x)
            ids = [c for c, C in enumerate(classes) if prog.type_names[int(C[K.C_TYPE_ID])] == name or prog.class_cells[c] == name]
            if name in prog.cell_to_class:
                ids.append(int(prog.cell_to_class[name]))
            ids += [int(c) for c in prog.agent_rename.get(name, [])]
            if not ids:
                raise ValueError(f"global state filter: the program has no class, cell or type named {name!r}")
        inc[ids] = 0
    return inc


def _digits(v: int, base: int) -> list:
    out = [v % base]
    v //= base
    while v > 0:
        out.append(v % base)
        v //= base
    return out


def object_tokens(prog, rec, spawned: bool = False) -> list:
    """The (feature, value) list of one raw object record, as the observation encoder emits it.  ``spawned``: the object was
    created at run time (no ObservationEncoder, grid_object.cpp:194): its inventory is not observable."""
    w = prog.words
    C = _classes(prog)[int(rec[1])]
    feat = lambda f: int(w[K.H_FEAT_BASE + f])  # noqa: E731
    if C[K.C_STATIC]:   # the class's own tags, whatever the record says: nothing about such an object changes
        static = prog.__dict__.setdefault("_gs_static", {})
        if int(rec[1]) not in static:
            static[int(rec[1])] = [(f & 0xFF, v & 0xFF) for f, v in _tag_tokens(feat(K.F_TAG), C[K.C_TAGS: K.C_TAGS + K.TAG_WORDS])]
        return static[int(rec[1])]
    out = _tag_tokens(feat(K.F_TAG), rec[8 + 2 * _MAXR: 8 + 2 * _MAXR + K.TAG_WORDS])
    if int(rec[4]) != 0:
        out.append((feat(K.F_VIBE), int(rec[4])))
    if not spawned:
        base = int(w[K.H_TOKEN_BASE])
        ioff = int(w[K.H_SECTION_BASE + 2 * K.SEC_INV_FEATURES])
        for k in range(int(rec[7])):
            item = int(rec[8 + k])
            for p, dig in enumerate(_digits(int(rec[8 + _MAXR + item]), base)):
                out.append((int(w[ioff + item * K.IF_WORDS + p]), dig))
    if int(rec[6]) >= 0:
        out += [(feat(K.F_GROUP), int(C[K.C_GROUP]) & 0xFF), (feat(K.F_AGENT_ID), int(rec[6]))]
    return [(f & 0xFF, v & 0xFF) for f, v in out]


def expected_rows(prog, raw_objects, class_include=None, n_initial=None, max_tokens=None) -> ExpectedRow:
    """The row of ONE env from its raw object records (``BatchedMettaGrid.raw_objects`` or the oracle's): ``tokens`` uint32
    (all of them, or exactly ``max_tokens`` dwords — truncated / padded with 0xFFFFFFFF — when that is given), ``count`` the
    untruncated number and ``agent_start`` int32 [A] (-1: filtered out, or at / behind ``max_tokens``).
    ``class_include``: u8 [classes], 0 = leave the class out.  ``n_initial``: objects the map created (its non-empty cells);
    records with a higher id were created at run time and show no inventory.  The raw record does not say so itself: leave it
    None only for programs that create no objects."""
    A = prog.num_agents
    on_grid = sorted((rec for rec in raw_objects if int(rec[5])), key=lambda rec: (int(rec[2]), int(rec[3])))
    toks, start = [], np.full(A, -1, np.int32)
    for rec in on_grid:
        if class_include is not None and not class_include[int(rec[1])]:
            continue
        if int(rec[6]) >= 0:
            start[int(rec[6])] = len(toks)
        r, c = int(rec[2]), int(rec[3])
        spawned = n_initial is not None and int(rec[0]) > int(n_initial)
        toks += [r | (c << 8) | (f << 16) | (v << 24) for f, v in object_tokens(prog, rec, spawned)]
    tokens, count = np.asarray(toks, dtype=np.uint32), len(toks)
    if max_tokens is not None:
        row = np.full(int(max_tokens), EMPTY, np.uint32)
        row[: min(count, int(max_tokens))] = tokens[: int(max_tokens)]
        start[start >= int(max_tokens)] = -1
        tokens = row
    return ExpectedRow(tokens, count, start)


def split_row(row) -> list:
    """A row (uint32 [TG], or u8 [TG][4]) -> ``[(r, c, [(f, v), ...]), ...]`` in row order; stops at the first 0xFFFFFFFF."""
    a = np.ascontiguousarray(row)
    if a.dtype == np.uint8:
        a = a.reshape(-1, 4).view(np.uint32).reshape(-1)
    out = []
    for t in a.astype(np.uint32).tolist():
        if t == EMPTY:
            break
        r, c, f, v = t & 0xFF, (t >> 8) & 0xFF, (t >> 16) & 0xFF, t >> 24
        if out and out[-1][0] == r and out[-1][1] == c:
            out[-1][2].append((f, v))
        else:
            out.append((r, c, [(f, v)]))
    return out


def from_observation(obs_row, agent_r: int, agent_c: int, prog) -> list:
    """One agent's reference observation row u8 [T][3] -> the object token groups it shows, with absolute coordinates:
    ``[(r, c, [(f, v), ...]), ...]`` in the row's order.  Dropped: padding (location 0xFF), the global tokens (location
    0xFE) and the per-observer territory token (feature ``aoe_mask``).  A row without padding may have lost tokens to the
    budget, so its last group is dropped too (it may be cut short)."""
    w = prog.words
    oh, ow = int(w[K.H_OBS_HEIGHT]), int(w[K.H_OBS_WIDTH])
    f_mask = int(w[K.H_FEAT_BASE + K.F_AOE_MASK])
    obs = np.asarray(obs_row, dtype=np.uint8).reshape(-1, 3)
    groups, order = {}, []
    for loc, f, v in obs.tolist():
        if loc in (_PAD_LOC, _GLOBAL_LOC):
            continue
        key = (agent_r + (loc >> 4) - oh // 2, agent_c + (loc & 0xF) - ow // 2)
        if key not in groups:
            groups[key] = []
            order.append(key)
        if f != f_mask or f_mask <= 0:
            groups[key].append((f, v))
    if len(obs) and obs[-1, 0] != _PAD_LOC and order:
        last = (agent_r + (int(obs[-1, 0]) >> 4) - oh // 2, agent_c + (int(obs[-1, 0]) & 0xF) - ow // 2)
        if int(obs[-1, 0]) != _GLOBAL_LOC and last in groups:
            order.remove(last)
    return [(r, c, groups[(r, c)]) for r, c in order if groups[(r, c)]]
