"""Looking at envs: the host side of include/mgx.h ``mgx_render_cells`` / ``mgx_render_rgb`` (kernels: csrc/mgx_render.h;
DESIGN.md §7k).  Nothing here needs a GPU.

A frame is made of one uint32 per map cell: ``0`` for an empty cell, else ``(class + 1) | agent_id << 16 | vibe << 24`` of the
object there (``agent_id`` 0xFF: not an agent; ``class``: the engine's class index, ``class_id`` of ``grid_objects()``).

``ansi`` restates the text frame of the reference's ``MettaGridPufferEnv.render()`` (envs/mettagrid_puffer_env.py:505-524:
``MapBuffer.render_full_map`` of renderer/miniscope/buffer.py:124-153,198-215,266-267 with ``get_symbol_for_object`` of
renderer/miniscope/symbol.py:26-46) on such words; ``rgb_host`` restates the frame rule of ``mgx_render_rgb`` in numpy;
``default_tiles`` draws an atlas for it.
"""
from __future__ import annotations

import numpy as np

from .fmt import K

NO_AGENT = 0xFF

# the reference's numbered squares of agents 0..9 and its default symbol table (renderer/miniscope/symbol.py:2-23), written out;
# tests/test_render_host.py compares them with the values recorded in tests/golden/render_frames.json
AGENT_SQUARES = ["\U0001F7E6", "\U0001F7E7", "\U0001F7E9", "\U0001F7E8", "\U0001F7EA", "\U0001F7E5", "\U0001F7EB", "⬛",
                 "\U0001F7E6", "\U0001F7E7"]
DEFAULT_SYMBOLS = {
    "wall": "⬜",
    "empty": "· ",
    "block": "\U0001F4E6",
    "agent": "\U0001F916",
    "agent.agent": "\U0001F916",
    "agent.team_1": "\U0001F535",
    "agent.team_2": "\U0001F534",
    "agent.team_3": "\U0001F7E2",
    "agent.team_4": "\U0001F7E1",
    "agent.prey": "\U0001F430",
    "agent.predator": "\U0001F981",
    "cursor": "\U0001F3AF",
    "aoe": "· ",
    "?": "❓",
}
# colours of the ten agent tiles of ``default_tiles``, in the order of AGENT_SQUARES: blue, orange, green, yellow, purple, red,
# brown, black, blue, orange
_AGENT_RGB = [(0, 116, 217), (255, 133, 27), (46, 204, 64), (255, 220, 0), (177, 13, 201), (255, 65, 54), (133, 88, 57),
              (17, 17, 17), (0, 116, 217), (255, 133, 27)]
_BACKGROUND = (32, 32, 36)


def _classes(prog) -> list:
    w = prog.words
    off = int(w[K.H_SECTION_BASE + 2 * K.SEC_CLASSES])
    return [w[off + c * K.C_WORDS: off + (c + 1) * K.C_WORDS] for c in range(int(w[K.H_NUM_CLASSES]))]


def class_type_names(prog) -> list:
    """``type_name`` of every class, by class index: the table ``signature.objects_from_raw`` resolves a record's class with."""
    return [prog.type_names[int(C[K.C_TYPE_ID])] for C in _classes(prog)]


def cells_from_objects(prog, objects: dict, H: int, W: int) -> np.ndarray:
    """The cell words uint32 [H, W] of a ``grid_objects()`` dict — what ``BatchedMettaGrid.render_cells`` returns for that env.
    The class is the object's ``class_id`` (``BatchedMettaGrid.grid_objects`` gives it); a dict without it, such as the
    reference's, gets the first class of the object's ``type_name`` (and ``group_id``, for agents): equal for the text frame,
    which only looks at the type name.  An object outside the map or of an unknown type is a ValueError."""
    classes = _classes(prog)
    names = class_type_names(prog)
    out = np.zeros((H, W), np.uint32)
    for obj in objects.values():
        r, c = int(obj["r"]), int(obj["c"])
        if not (0 <= r < H and 0 <= c < W):
            raise ValueError(f"cells_from_objects: object at ({r}, {c}) outside the {H}x{W} map")
        agent = int(obj["agent_id"]) if obj.get("agent_id") is not None else NO_AGENT
        cls = obj.get("class_id")
        if cls is None:
            fit = [k for k, n in enumerate(names) if n == obj["type_name"]
                   and (agent == NO_AGENT or "group_id" not in obj or int(classes[k][K.C_GROUP]) == int(obj["group_id"]))]
            if not fit:
                raise ValueError(f"cells_from_objects: the program has no class of type {obj['type_name']!r}")
            cls = fit[0]
        out[r, c] = (int(cls) + 1) | (agent & 0xFF) << 16 | (int(obj.get("vibe", 0)) & 0xFF) << 24
    return out


def ansi(cells, type_names_by_class, symbols=None) -> str:
    """The reference's text frame of one env's cell words [H, W].  ``symbols`` overrides entries of ``DEFAULT_SYMBOLS`` (the
    reference's ``game.render.symbols``, which never reaches the engine's config).  The frame is cropped to the bounding box
    of the objects whose type is ``"wall"`` (of all objects when there is none; 1x1 at (0, 0) on an empty map): MapBuffer
    recomputes its bounds on the first call whatever size it was given, and objects outside the box are not drawn.  An agent
    with an id below ten is its numbered square; otherwise the symbol of the full type name, of its part before the first
    ``.``, or of ``"?"``."""
    cells = np.asarray(cells, dtype=np.uint32)
    if cells.ndim != 2:
        raise ValueError("ansi: cells of ONE env, [H, W]")
    table = dict(DEFAULT_SYMBOLS)
    table.update(symbols or {})
    rr, cc = np.nonzero(cells)
    objs = [(int(r), int(c), type_names_by_class[(int(cells[r, c]) & 0xFFFF) - 1], (int(cells[r, c]) >> 16) & 0xFF) for r, c in zip(rr, cc)]
    box = [(r, c) for r, c, name, _ in objs if name == "wall"] or [(r, c) for r, c, _, _ in objs]
    if box:
        r0, c0 = min(r for r, _ in box), min(c for _, c in box)
        h, w = max(r for r, _ in box) - r0 + 1, max(c for _, c in box) - c0 + 1
    else:
        r0, c0, h, w = 0, 0, 1, 1
    grid = [[table.get("empty", "⬜")] * w for _ in range(h)]
    for r, c, name, agent in objs:
        if not (0 <= r - r0 < h and 0 <= c - c0 < w):
            continue
        if name.startswith("agent") and agent != NO_AGENT and agent < 10:
            sym = AGENT_SQUARES[agent]
        elif name in table:
            sym = table[name]
        else:
            sym = table.get(name.split(".")[0], table.get("?", "❓"))
        grid[r - r0][c - c0] = sym
    return "\n".join("".join(row) for row in grid)


def rgb_host(cells, tiles, class_tile, agent_tile, vibe_rgb=None) -> np.ndarray:
    """The frames ``mgx_render_rgb`` writes for these cell words ([H, W] or [n, H, W]): uint8 [..., H * s, W * s, 3].  A cell shows
    tile 0 when empty, ``agent_tile[agent]`` for an agent, else ``class_tile[class]``; with ``vibe_rgb`` [n_vibes, 3] and
    s >= 3, a cell whose vibe is in 1 .. n_vibes - 1 gets that colour on the q x q pixels of its top right corner, q = s // 3."""
    cells = np.asarray(cells, dtype=np.uint32)
    tiles = np.asarray(tiles, dtype=np.uint8)
    class_tile, agent_tile = np.asarray(class_tile, dtype=np.int64), np.asarray(agent_tile, dtype=np.int64)
    s = tiles.shape[1]
    if cells.ndim not in (2, 3) or tiles.ndim != 4 or tiles.shape[1:] != (s, s, 3):
        raise ValueError("rgb_host: cells [H, W] or [n, H, W], tiles [n_tiles, s, s, 3]")
    cls = (cells & 0xFFFF).astype(np.int64) - 1
    agent = ((cells >> 16) & 0xFF).astype(np.int64)
    vibe = (cells >> 24).astype(np.int64)
    is_agent = (agent != NO_AGENT) & (agent < len(agent_tile))
    t = np.where(cells == 0, 0, np.where(is_agent, agent_tile[np.minimum(agent, len(agent_tile) - 1)],
                                         class_tile[np.clip(cls, 0, len(class_tile) - 1)]))
    H, W = cells.shape[-2:]
    pix = np.moveaxis(tiles[t], -4, -3).copy()        # [..., H, W, s, s, 3] -> [..., H, s, W, s, 3]
    q = s // 3
    if vibe_rgb is not None and q > 0:
        vibe_rgb = np.asarray(vibe_rgb, dtype=np.uint8).reshape(-1, 3)
        marked = (vibe > 0) & (vibe < len(vibe_rgb))
        colour = vibe_rgb[np.minimum(vibe, len(vibe_rgb) - 1)]                                   # [..., H, W, 3]
        corner = pix[..., :q, :, s - q:, :]                                                     # [..., H, q, W, q, 3]
        pix[..., :q, :, s - q:, :] = np.where(marked[..., :, None, :, None, None], colour[..., :, None, :, None, :], corner)
    return pix.reshape(cells.shape[:-2] + (H * s, W * s, 3))


def _type_rgb(i: int) -> tuple:
    # 97, 57 and 151 are coprime with 192: the red channel alone tells the first 192 types apart
    return (64 + (i * 97 + 31) % 192, 64 + (i * 57 + 101) % 192, 64 + (i * 151 + 7) % 192)


def default_tiles(prog, scale: int = 8):
    """A deterministic atlas for ``prog``: ``(tiles u8 [n_tiles, s, s, 3], class_tile u16 [classes], agent_tile u16 [A],
    vibe_rgb u8 [n_vibes, 3])`` with s = ``scale`` in 1..32.  Tile 0 is the background; every type has one tile in a colour of
    its own — wall-kind types filled edge to edge, other objects with a one-pixel margin; agents are diamonds in ten colours
    that follow the reference's numbered squares and cycle from agent 10 on; every vibe has a marker colour."""
    s = int(scale)
    if not 1 <= s <= 32:
        raise ValueError("default_tiles: scale must be in [1, 32]")
    classes = _classes(prog)
    n_types = len(prog.type_names)
    tiles = np.empty((1 + n_types + 10, s, s, 3), np.uint8)
    tiles[:] = np.asarray(_BACKGROUND, np.uint8)
    wall_types = {int(C[K.C_TYPE_ID]) for C in classes if int(C[K.C_KIND]) == K.KIND_WALL}
    m = 1 if s >= 3 else 0
    for i in range(n_types):
        rgb = (168, 168, 168) if prog.type_names[i] == "wall" else _type_rgb(i)
        if i in wall_types:
            tiles[1 + i] = rgb
        else:
            tiles[1 + i, m:s - m, m:s - m] = rgb
    y, x = np.mgrid[0:s, 0:s]
    diamond = (np.abs(2 * y + 1 - s) + np.abs(2 * x + 1 - s) <= s) if s >= 3 else np.ones((s, s), bool)
    for k, rgb in enumerate(_AGENT_RGB):
        tiles[1 + n_types + k][diamond] = rgb
    class_tile = np.asarray([1 + int(C[K.C_TYPE_ID]) for C in classes], np.uint16)
    agent_tile = np.asarray([1 + n_types + a % 10 for a in range(prog.num_agents)], np.uint16)
    n_vibes = max(1, len(prog.vibe_names))
    vibe_rgb = np.asarray([(255 - (v * 83) % 160, 96 + (v * 131) % 160, 255 - (v * 47 + 60) % 200) for v in range(n_vibes)], np.uint8)
    return tiles, class_tile, agent_tile, vibe_rgb
