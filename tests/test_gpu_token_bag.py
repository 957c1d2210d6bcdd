"""GPU: the token-bag kernel (mgx_token_bag, csrc/mgx_token_bag.hip) against the numpy restatement
mettagrid_amd/token_bag.py::bag_host, TokenBagEmbedding on the device, the wrapper's ``token_bag`` option and the refusals.

Tolerances (u = 2**-24, nothing tuned on the kernel): every term of a bin is the same float32 quotient on both sides and
non-negative, so a float32 sum of at most T of them in ANY order is within (T - 1) u (1 + O(u)) of the exact sum, relative:
2 T u is asked.  bfloat16 adds one rounding to 8 bits: 2**-8.  Bins without a token are exactly 0, bins with one token hold
that term bit for bit."""
import numpy as np
import pytest

from mettagrid_amd import presets
from mettagrid_amd import token_bag as tb
from mettagrid_amd.compiler import compile_spec
from mettagrid_amd.engine import BatchedMettaGrid
from mettagrid_amd.mapgen import random_class_maps

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
R3_OBJECTS, R3_AGENTS = {"wall": 40, "extractor": 8, "chest": 4}, {"red": 8, "blue": 8}
RPW = tb.ROWS_PER_WORKGROUP
_engines = {}


def engine_for(T: int, E: int = 1) -> BatchedMettaGrid:
    """One small rung-3 engine per token budget, shared by the tests of this module (the kernel takes T from the engine)."""
    if (T, E) not in _engines:
        prog = compile_spec(presets.rung3_spec(obs_tokens=T), 32, 32, max_objects=192)
        cms = random_class_maps(prog, 32, 32, R3_OBJECTS, R3_AGENTS, range(E))
        _engines[(T, E)] = BatchedMettaGrid(prog, cms, np.arange(E, dtype=np.uint32), buffers="device", specialize=False)
    return _engines[(T, E)]


def tokens_per_bin(tok: np.ndarray, C: int) -> np.ndarray:
    coord, fid = tok[..., 0].astype(np.int64), tok[..., 1].astype(np.int64)
    valid = (coord != 0xFF) & (fid < C)
    n = np.zeros((tok.shape[0], 32 + C), np.int64)
    r = np.broadcast_to(np.arange(tok.shape[0])[:, None], coord.shape)
    for col in (coord & 15, 16 + (coord >> 4), 32 + fid):
        np.add.at(n, (r[valid], col[valid]), 1)
    return n


def check_bag(got_bag, got_counts, tok: np.ndarray, scale: np.ndarray, C: int, what: str, rel: float = 0.0) -> None:
    """counts exact; every entry within (rel + 2 T u) x the float64 sum; empty bins 0; with rel = 0 (float32) single-token
    bins bit-equal to their term."""
    T = tok.shape[1]
    want, want_counts = tb.bag_host(tok, scale, C)
    got = got_bag.float().cpu().numpy().astype(np.float64)
    assert got.shape == want.shape, what
    assert np.array_equal(got_counts.cpu().numpy(), want_counts), what
    err = np.abs(got - want)
    worst = (err / np.where(want > 0, want, 1.0)).max()
    print(f"{what}: max relative error {worst / U:.2f} u (allowed {(rel + 2 * T * U) / U:.0f} u)")
    assert (err <= (rel + 2 * T * U) * want).all(), (what, np.argwhere(err > (rel + 2 * T * U) * want)[:5])
    n = tokens_per_bin(tok, C)
    assert not got[n == 0].any(), what
    if rel == 0.0:
        assert np.array_equal(got[n == 1], want[n == 1]), what


def step_random(eng, gen) -> None:
    import torch
    n = len(eng.prog.action_names)
    eng.actions.copy_(torch.randint(0, n, tuple(eng.actions.shape), dtype=torch.int32, device="cuda", generator=gen))
    eng.vibe_actions.copy_(torch.randint(0, n, tuple(eng.actions.shape), dtype=torch.int32, device="cuda", generator=gen))
    torch.cuda.synchronize()
    eng.step()
    eng.sync()


def foreign_rows(rows: int, T: int, C: int, seed: int) -> np.ndarray:
    """Row 0: every token on one coord and one feature with value 255; row 1: all padding; row 2: also tokens of features
    >= C (where C < 256) and padding in the middle; the rest: random fill, a cell's tokens following each other, 0xFE among
    the coords."""
    rng = np.random.default_rng(seed)
    tok = np.full((rows, T, 3), 0xFF, np.uint8)
    fmax = min(256, C + 3)
    for r in range(rows):
        if r == 0:
            tok[r] = (0x5A, C - 1, 255)
            continue
        if r == 1:
            continue
        n = T if r == 2 else int(rng.integers(0, T + 1))
        t = 0
        while t < n:
            k = min(n - t, int(rng.integers(1, 9)))
            tok[r, t:t + k, 0] = rng.choice([0xFE, 0xFF, int(rng.integers(0, 0xFE))], p=[.1, .05, .85])
            tok[r, t:t + k, 1] = rng.integers(0, fmax if rng.random() < .2 else C, k)
            tok[r, t:t + k, 2] = rng.integers(0, 256, k)
            t += k
        if r == 2:
            tok[r, ::2, 1] = fmax - 1        # every other token: a feature >= C (where C < 256)
            tok[r, T // 2, 0] = 0xFF         # padding in the middle of the row
    return tok


@pytest.fixture(scope="module")
def tail_buffer():
    """A 12 MiB allocation of its own (the caching allocator serves a request of that size with one device allocation of
    exactly that size): token rows placed at its end end where the allocation ends."""
    import torch
    torch.cuda.empty_cache()   # (no cached block to carve the request from)
    return torch.empty(12 << 20, dtype=torch.uint8, device="cuda")


def test_engine_rows():
    import torch
    eng = engine_for(200, 6)
    gen = torch.Generator(device="cuda").manual_seed(2)
    for _ in range(5):
        step_random(eng, gen)
    bag, counts = eng.token_bag()
    eng.sync()
    C = len(eng.prog.feature_norms)
    assert bag.dtype == torch.float32 and tuple(bag.shape) == (6 * eng.A, 32 + C) and counts.dtype == torch.int32
    obs = eng.obs.cpu().numpy()
    assert (obs[..., 0] != 0xFF).any()
    check_bag(bag, counts, obs, eng.feature_scale(), C, "engine rows")
    # caller-owned outputs are filled in place, whatever they held
    out, cnt = torch.full_like(bag, 7.0), torch.full_like(counts, -3)
    got = eng.token_bag(out, cnt)
    eng.sync()
    assert got[0] is out and got[1] is cnt and torch.equal(out, bag) and torch.equal(cnt, counts)


@pytest.mark.parametrize("T", [1, 63, 64, 65, 200])
def test_foreign_rows(T, tail_buffer):
    import torch
    eng = engine_for(T)
    scale = eng.feature_scale()
    for C in (1, 17, 256):
        tok = foreign_rows(257, T, C, seed=1000 * T + C)
        for rows in sorted({1, RPW - 1, RPW, RPW + 1, 257}):
            # the rows sit at the END of the allocation: a read past the last row leaves it
            dev = tail_buffer[tail_buffer.numel() - rows * T * 3:].view(rows, T, 3)
            dev.copy_(torch.from_numpy(tok[:rows]))
            torch.cuda.synchronize()
            bag, counts = eng.token_bag(tokens=dev, num_features=C)
            eng.sync()
            check_bag(bag, counts, tok[:rows], scale, C, f"T={T} C={C} rows={rows}")
            if rows >= 3:
                s = np.float32(255) / (scale[C - 1] + np.float32(1e-6))
                assert counts[0].item() == T and counts[1].item() == 0 and not bag[1].any().item()
                assert abs(bag[0, 0xA].item() - T * float(s)) <= 2 * T * U * T * float(s)
                assert C == 256 or (tok[2, :, 1] >= C).any()


@pytest.mark.parametrize("C", [1, 2, 17, 256])
def test_bfloat16(C):
    """Row strides of 33 and 49 (2-byte stores), 34 (dword stores) and 288 (16-byte stores) bfloat16 elements."""
    import torch
    T = 200
    eng = engine_for(T)
    tok = foreign_rows(RPW + 2, T, C, seed=77 + C)
    dev = torch.from_numpy(tok).cuda()
    out = torch.full((tok.shape[0], 32 + C), 3.0, dtype=torch.bfloat16, device="cuda")
    bag, counts = eng.token_bag(out=out, tokens=dev, num_features=C)
    eng.sync()
    assert bag is out
    check_bag(bag, counts, tok, eng.feature_scale(), C, f"bfloat16 C={C}", rel=2.0 ** -8)
    # ... and it is the float32 bag rounded to nearest even
    f32, _ = eng.token_bag(tokens=dev, num_features=C)
    eng.sync()
    assert torch.equal(f32.to(torch.bfloat16), bag)


def test_embedding_on_the_device():
    import torch
    eng = engine_for(200, 6)
    gen = torch.Generator(device="cuda").manual_seed(9)
    for _ in range(3):
        step_random(eng, gen)
    T, C = eng.T, len(eng.prog.feature_norms)
    bag, counts = eng.token_bag()
    eng.sync()
    rows = bag.shape[0]
    torch.manual_seed(4)
    m = tb.TokenBagEmbedding.from_engine(eng).cuda()
    assert np.array_equal(m._feature_scale.cpu().numpy(), eng.feature_scale())
    out = m(bag, counts)
    assert out.dtype == torch.float32 and tuple(out.shape) == (rows, 192)
    px, py, ft = (w.detach().cpu().numpy().astype(np.float64) for w in (m.pos_x_embed.weight, m.pos_y_embed.weight, m.feature_embed.weight))
    hbag, hcounts = tb.bag_host(eng.obs.cpu().numpy(), eng.feature_scale(), C)
    want = tb.summary_host(hbag, hcounts, px, py, ft)
    table = np.abs(np.concatenate([px[:16], py[:16], ft[:C]]))
    bound = (np.abs(hbag) @ table) / np.sqrt(np.maximum(hcounts, 1))[:, None]
    err = np.abs(out.detach().cpu().numpy().astype(np.float64) - want)
    print(f"summary: max |delta| / bound = {(err / np.where(bound > 0, bound, 1.0)).max() / U:.2f} u (allowed {T + 40 + C})")
    assert (err <= (T + 40 + C) * U * bound).all()
    # backward: torch's own GEMM backward reaches the three tables; float64 restatement from the same bag
    G = torch.randn(out.shape, generator=torch.Generator().manual_seed(6)).cuda()
    out.backward(G)
    bag_n = bag.cpu().numpy().astype(np.float64) / np.sqrt(np.maximum(counts.cpu().numpy(), 1))[:, None]
    g64 = G.cpu().numpy().astype(np.float64)
    want_grad = bag_n.T @ g64
    tol = 2 * rows * U * (np.abs(bag_n).T @ np.abs(g64))
    got_grad = np.concatenate([m.pos_x_embed.weight.grad[:16].cpu().numpy(), m.pos_y_embed.weight.grad[:16].cpu().numpy(),
                               m.feature_embed.weight.grad[:C].cpu().numpy()]).astype(np.float64)
    gerr = np.abs(got_grad - want_grad)
    print(f"gradients: max |delta| / (|bag_n|^T |G|) = {(gerr / np.where(tol > 0, tol / (2 * rows * U), 1.0)).max() / U:.2f} u (allowed {2 * rows})")
    assert (gerr <= tol).all()
    assert not m.pos_x_embed.weight.grad[16:].any().item() and not m.feature_embed.weight.grad[C:].any().item()


def test_wrapper_rows_follow_the_observations():
    import torch
    from mettagrid_amd.envs import MettaGridBatchedEnv
    E, M = 4, 3
    spec = presets.rung3_spec()
    spec.max_steps = 3
    spec.episode_truncates = True
    prog = compile_spec(spec, 32, 32, max_objects=192)
    pool = random_class_maps(prog, 32, 32, R3_OBJECTS, R3_AGENTS, range(M))
    C = len(prog.feature_norms)
    with pytest.raises(ValueError):
        MettaGridBatchedEnv(prog, E, map_pool=pool, buffers="host", token_bag=True)
    with pytest.raises(ValueError):
        MettaGridBatchedEnv(prog, E, map_pool=pool, token_bag="float16")
    plain = MettaGridBatchedEnv(prog, E, map_pool=pool, seed=3, specialize=False, episode_stats=False)
    assert plain.token_bag is None
    env = MettaGridBatchedEnv(prog, E, map_pool=pool, seed=3, specialize=False, episode_stats=False, token_bag=True)
    env16 = MettaGridBatchedEnv(prog, E, map_pool=pool, seed=3, specialize=False, episode_stats=False, token_bag="bfloat16")
    obs, _ = env.reset()
    plain.reset(); env16.reset()
    scale = env.engine.feature_scale()
    bag, counts = env.token_bag
    assert bag.dtype == torch.float32 and tuple(bag.shape) == (E * prog.num_agents, 32 + C) and env16.token_bag[0].dtype == torch.bfloat16
    check_bag(bag, counts, obs.cpu().numpy(), scale, C, "wrapper reset")   # (the caller's stream: ordered by the wrapper)
    g = torch.Generator(device="cuda").manual_seed(1)
    ends = 0
    for t in range(4):
        a = torch.randint(0, env.transport_action_n, (env.num_agents,), dtype=torch.int32, device="cuda", generator=g)
        obs, _, _, trunc, _ = env.step(a)
        pobs = plain.step(a)[0]
        o16 = env16.step(a)[0]
        assert env.token_bag[0] is bag and env.token_bag[1] is counts     # updated in place
        assert torch.equal(obs, pobs) and torch.equal(obs, o16)           # the option changes nothing else
        check_bag(bag, counts, obs.cpu().numpy(), scale, C, f"wrapper step {t + 1}")
        assert torch.equal(env16.token_bag[0], bag.to(torch.bfloat16)) and torch.equal(env16.token_bag[1], counts)
        ends += int(bool(trunc.all()))
    assert ends >= 1   # an episode ended and restarted on the device within the checked steps
    st = env.save_state([0])
    env.step(torch.zeros(env.num_agents, dtype=torch.int32, device="cuda"))
    env.load_state(st, [2])
    check_bag(bag, counts, env.engine.obs.cpu().numpy(), scale, C, "wrapper load_state")
    for e in (plain, env, env16):
        e.close()


def test_refusals():
    import torch
    eng = engine_for(200, 6)
    L, h = eng.L, eng.h
    C = len(eng.prog.feature_norms)
    rows = 6 * eng.A
    bag, counts = eng.token_bag()
    eng.sync()
    keep_bag, keep_counts = bag.clone(), counts.clone()
    # ---- Python level: ValueError before the library is called ----
    tok = torch.full((5, eng.T, 3), 0xFF, dtype=torch.uint8, device="cuda")
    bad_calls = [
        dict(out=torch.zeros((rows, 32 + C), dtype=torch.float16, device="cuda")),
        dict(out=torch.zeros((rows, 32 + C), dtype=torch.float64, device="cuda")),
        dict(out=torch.zeros((rows, 31 + C), device="cuda")),
        dict(out=torch.zeros((rows + 1, 32 + C), device="cuda")),
        dict(out=torch.zeros((32 + C, rows), device="cuda").t()),
        dict(out=torch.zeros((rows, 32 + C))),
        dict(counts=torch.zeros(rows, dtype=torch.int64, device="cuda")),
        dict(counts=torch.zeros(rows + 1, dtype=torch.int32, device="cuda")),
        dict(counts=torch.zeros(2 * rows, dtype=torch.int32, device="cuda")[::2]),
        dict(tokens=tok.to(torch.int8)),
        dict(tokens=tok[:, :-1]),
        dict(tokens=tok[:, :, :2]),
        dict(tokens=tok[:0]),
        dict(tokens=torch.full((5, 3, eng.T), 0xFF, dtype=torch.uint8, device="cuda").transpose(1, 2)),
        dict(tokens=tok.cpu()),
        dict(num_features=0),
        dict(num_features=257),
        dict(tokens=tok, out=torch.zeros((rows, 32 + C), device="cuda")),   # rows of the token tensor, not E*A
    ]
    for kw in bad_calls:
        with pytest.raises(ValueError):
            eng.token_bag(**kw)
    # ---- C level: MGX_ERR_BAD_ARG (-1) before anything is enqueued ----
    scale = eng.feature_scale()
    b, c, s, t = bag.data_ptr(), counts.data_ptr(), scale.ctypes.data, tok.data_ptr()
    assert L.mgx_token_bag(h, None, 0, b, 1, c, C, s) == 0     # (a valid call through the same path)
    for args in [(None, None, 0, b, 1, c, C, s), (h, None, 0, None, 1, c, C, s), (h, None, 0, b, 1, None, C, s), (h, None, 0, b, 1, c, C, None),
                 (h, None, 0, b, 1, c, 0, s), (h, None, 0, b, 1, c, 257, s), (h, None, 0, b, 1, c, -1, s),
                 (h, None, 0, b, 0, c, C, s), (h, None, 0, b, 3, c, C, s),
                 (h, t, 0, b, 1, c, C, s), (h, t, -1, b, 1, c, C, s)]:
        assert L.mgx_token_bag(*args) == -1, args
    eng.sync()
    assert torch.equal(bag, keep_bag) and torch.equal(counts, keep_counts)   # nothing was enqueued
    box = torch.zeros((rows, C, int(eng.prog.words[13]), int(eng.prog.words[14])), device="cuda")
    eng.set_box_output(box)
    assert L.mgx_token_bag(h, None, 0, b, 1, c, C, s) == -1    # no observation rows while box output is on
    with pytest.raises(ValueError):
        eng.token_bag(bag, counts)
    assert L.mgx_token_bag(h, t, 5, b, 1, c, C, s) == 0        # foreign rows are still served (the first 5 rows of bag)
    eng.set_box_output(None)
    eng.sync()
    assert torch.equal(bag[5:], keep_bag[5:]) and torch.equal(counts[5:], keep_counts[5:])
    assert not bag[:5].any().item() and not counts[:5].any().item()        # the all-padding foreign rows
    assert L.mgx_token_bag(h, None, 0, b, 1, c, C, s) == 0
    eng.sync()
    assert torch.equal(bag, keep_bag) and torch.equal(counts, keep_counts)


def teardown_module(module):
    for eng in _engines.values():
        eng.close()
    _engines.clear()
