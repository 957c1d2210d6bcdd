"""GPU: the dense-policy front end (csrc/mgx_byte_linear.hip, mettagrid_amd/byte_linear.py).

Exact cases (scale = 1, integer weights and gradients): every product and every partial sum is an integer below 2**24, so any
float32 summation order gives the same bits and a wrong lane map, tail or chunk shows as a wrong VALUE.

Real-valued cases against the float64 host functions on the kernel's own operands.  The tolerance is derived, not tuned
(u = 2**-24): a product of an 8-bit by an 8-bit significand is exact in float32; what remains is a float32 sum of
terms * K such products in an unspecified order, one scaling and one bias add, first-order bound
(terms * K + 2) u S with S = |s| sum_k |x w_hi| + |s| sum_k |x w_lo| + |b|; asked is twice that (the project's usual
margin; the MFMA's internal rounding is not documented to be per-add round-to-nearest).  The weight gradient:
K replaced by N, the sums over rows.  bfloat16 output adds 2**-8 |y|."""
import numpy as np
import pytest
import torch

from mettagrid_amd import byte_linear as bl
from mettagrid_amd.engine import load_lib

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
NS, KS, HS = (1, 15, 16, 17, 257), (1, 31, 32, 33, 600, 603), (16, 128, 144)


@pytest.fixture(scope="module")
def tail_buffer():
    """A 12 MiB allocation of its own (the caching allocator serves a request of that size with one device allocation of
    exactly that size): rows placed at its end end where the allocation ends."""
    torch.cuda.empty_cache()
    return torch.empty(12 << 20, dtype=torch.uint8, device="cuda")


def at_tail(tail, x: np.ndarray) -> torch.Tensor:
    """x [N, K] as a device tensor whose last byte is the last byte of the allocation (its first byte where that falls)."""
    n, k = x.shape
    dev = tail[tail.numel() - n * k:].view(n, k)
    dev.copy_(torch.from_numpy(x))
    return dev


def rows(n: int, k: int, seed: int) -> np.ndarray:
    """Row 0 all zero, row 1 all 0xFF, row 2 one non-zero byte, the rest random bytes with a 0xFF tail of random length."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, (n, k), dtype=np.uint8)
    for r in range(n):
        x[r, int(rng.integers(0, k + 1)):] = 0xFF
    x[0] = 0
    if n > 1:
        x[1] = 0xFF
    if n > 2:
        x[2] = 0
        x[2, (7 * k) // 11] = 201
    return x


def bf16(a: np.ndarray) -> torch.Tensor:
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16)
    assert np.array_equal(t.float().numpy(), a)     # the test's weights are bfloat16 values
    return t.cuda()


@pytest.mark.parametrize("K", KS)
def test_forward_exact(K, tail_buffer):
    rng = np.random.default_rng(K)
    for H in HS:
        w_hi = rng.integers(-8, 9, (H, K)).astype(np.float32)
        w_lo = rng.integers(-8, 9, (H, K)).astype(np.float32)
        b = rng.integers(-1000, 1001, H).astype(np.float32)
        idx = rng.integers(0, K, H)
        idx[0], idx[-1] = K - 1, 0
        sel = np.zeros((H, K), np.float32)
        sel[np.arange(H), idx] = 1.0
        d_hi, d_lo, d_sel, d_b = bf16(w_hi), bf16(w_lo), bf16(sel), torch.from_numpy(b).cuda()
        for N in NS:
            x = rows(N, K, seed=1000 * K + N)
            dev = at_tail(tail_buffer, x)
            x64 = x.astype(np.int64)
            what = f"N={N} K={K} H={H}"
            # selector weights: y[n][h] == x[n][idx[h]]
            y = bl.byte_linear(dev, d_sel, scale=1.0)
            assert y.dtype == torch.float32 and np.array_equal(y.cpu().numpy(), x[:, idx].astype(np.float32)), what
            # integer weights, two terms, bias: |sum| <= 603 * 255 * 16 + 1000 < 2**24
            want = x64 @ (w_hi.astype(np.int64) + w_lo.astype(np.int64)).T + b.astype(np.int64)
            assert np.abs(want).max() < 2 ** 24
            y2 = bl.byte_linear(dev, d_hi, d_lo, d_b, scale=1.0)
            assert np.array_equal(y2.cpu().numpy().astype(np.int64), want), what
            # one term; all-zero rows give the bias, all-0xFF rows 255 * the row sums of W
            y1 = bl.byte_linear(dev, d_hi, None, d_b, scale=1.0).cpu().numpy()
            assert np.array_equal(y1.astype(np.int64), x64 @ w_hi.astype(np.int64).T + b.astype(np.int64)), what
            assert np.array_equal(y1[0], b), what
            if N > 2:
                assert np.array_equal(y1[1], 255 * w_hi.sum(1) + b) and np.array_equal(y1[2], 201 * w_hi[:, (7 * K) // 11] + b), what


def test_forward_layouts(tail_buffer):
    """An odd start address, a row stride larger than K (4-aligned and not), strided outputs on the 16-byte store path and
    off it, bfloat16 output: all bit-equal to the plain call."""
    rng = np.random.default_rng(5)
    for K, H, N in ((600, 128, 257), (603, 144, 17), (33, 16, 130)):
        x = rows(N, K, seed=K)
        w = rng.integers(-8, 9, (H, K)).astype(np.float32)
        b = torch.from_numpy(rng.integers(-1000, 1001, H).astype(np.float32)).cuda()
        d_w = bf16(w)
        want = torch.from_numpy((x.astype(np.int64) @ w.astype(np.int64).T).astype(np.float32)).cuda() + b
        plain = bl.byte_linear(torch.from_numpy(x).cuda(), d_w, None, b, scale=1.0)
        assert torch.equal(plain, want)
        for start, stride in ((1, K), (3, K + 1), (0, K + 4), (2, K + 8), (0, 2 * K + 1)):
            dev = torch.as_strided(tail_buffer, (N, K), (stride, 1), 4096 + start)
            assert dev.data_ptr() % 4 == start
            dev.copy_(torch.from_numpy(x))
            assert torch.equal(bl.byte_linear(dev, d_w, None, b, scale=1.0), want), (K, start, stride)
        for stride in (K + 4, K + 5):   # strided rows whose last byte is the last byte of the allocation
            dev = torch.as_strided(tail_buffer, (N, K), (stride, 1), tail_buffer.numel() - ((N - 1) * stride + K))
            dev.copy_(torch.from_numpy(x))
            assert torch.equal(bl.byte_linear(dev, d_w, None, b, scale=1.0), want), (K, stride)
        dev = torch.from_numpy(x).cuda()
        for pad, off, dtype in ((16, 0, torch.float32), (11, 5, torch.float32), (8, 0, torch.bfloat16), (3, 1, torch.bfloat16)):
            big = torch.full((N, H + pad), -7.0, dtype=dtype, device="cuda")
            out = big[:, off:off + H]
            got = bl.byte_linear(dev, d_w, None, b, scale=1.0, out=out)
            assert got is out and torch.equal(out, want.to(dtype)), (K, pad, off, dtype)   # (bfloat16: the float32 result, rounded)
            mask = torch.ones_like(big, dtype=torch.bool)
            mask[:, off:off + H] = False
            assert (big[mask] == -7.0).all()                                              # nothing outside the view was written
        assert torch.equal(bl.byte_linear(dev, d_w, None, b, scale=1.0, out_dtype=torch.bfloat16), want.to(torch.bfloat16))


def wgrad(dev, dy, scale, terms):
    """byte_linear_wgrad with a scratch of exactly mgx_byte_linear_scratch_bytes, filled with NaN bits beforehand."""
    L = load_lib()
    N, K, H = dev.shape[0], dev.shape[1], dy.shape[1]
    chunk = L.mgx_byte_linear_chunk_rows()
    need = L.mgx_byte_linear_scratch_bytes(N, K, H)
    assert need == -(-N // chunk) * H * K * 4
    scratch = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
    return bl.byte_linear_wgrad(dev, dy, scale, terms, scratch=scratch)


@pytest.mark.parametrize("K", KS)
def test_wgrad_exact(K, tail_buffer):
    rng = np.random.default_rng(100 + K)
    for H in HS:
        for N in NS:
            x = rows(N, K, seed=2000 * K + N)
            dev = at_tail(tail_buffer, x)
            x64 = x.astype(np.float64)
            what = f"N={N} K={K} H={H}"
            # integer dy in [-8, 8]: |sum| <= 4096 * 8 * 255 < 2**24, exact in any order, for every dtype and term count
            dy = rng.integers(-8, 9, (N, H)).astype(np.float32)
            want = (dy.astype(np.float64).T @ x64).astype(np.float32)
            d32 = torch.from_numpy(dy).cuda()
            for d, terms in ((d32, 1), (d32, 2), (d32.to(torch.bfloat16), 1), (d32.to(torch.bfloat16), 2)):
                got = wgrad(dev, d, 1.0, terms)
                assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), want), (what, d.dtype, terms)
            # one-hot dy: dW[h] is the sum of the rows that chose h
            pick = rng.integers(0, H, N)
            pick[0] = H - 1
            hot = np.zeros((N, H), np.float32)
            hot[np.arange(N), pick] = 1.0
            want = np.zeros((H, K), np.float64)
            np.add.at(want, pick, x64)
            assert np.array_equal(wgrad(dev, torch.from_numpy(hot).cuda(), 1.0, 2).cpu().numpy(), want.astype(np.float32)), what


def test_wgrad_chunks_and_repeats(tail_buffer):
    chunk = bl.chunk_rows()
    assert chunk == load_lib().mgx_byte_linear_chunk_rows() and chunk >= 64
    rng = np.random.default_rng(9)
    for K, H, ns in ((67, 32, (chunk - 1, chunk, chunk + 1, 2 * chunk + 3)), (600, 128, (2 * chunk + 3,))):
        for N in ns:
            x = rows(N, K, seed=N + K)
            dev = at_tail(tail_buffer, x)
            # dy in {-1, 0, 1}: |sum| <= (2 chunk + 3) * 255 < 2**24 for the library's chunk, exact across the chunk boundaries
            assert N * 255 < 2 ** 24
            dy = rng.integers(-1, 2, (N, H)).astype(np.float32)
            want = (dy.astype(np.float64).T @ x.astype(np.float64)).astype(np.float32)
            assert np.array_equal(wgrad(dev, torch.from_numpy(dy).cuda(), 1.0, 2).cpu().numpy(), want), (N, K, H)
            # real values: the same bits from call to call
            g = torch.randn((N, H), generator=torch.Generator().manual_seed(N)).cuda()
            a, b = wgrad(dev, g, 1.0 / 255.0, 2), wgrad(dev, g, 1.0 / 255.0, 2)
            assert torch.equal(a, b), (N, K, H)


@pytest.mark.parametrize("N,K,H", [(257, 600, 128), (130, 603, 144), (17, 33, 16)])
def test_real_values(N, K, H, tail_buffer):
    scale = 1.0 / 255.0
    s = float(np.float32(scale))
    g = torch.Generator().manual_seed(N + K)
    w = torch.randn(H, K, generator=g) * 0.1
    b = torch.randn(H, generator=g)
    dy = torch.randn(N, H, generator=g)
    x = rows(N, K, seed=N * K)
    dev = at_tail(tail_buffer, x)
    ax = x.astype(np.float64)
    hi, lo = bl.split_bf16(w)
    for terms in (1, 2):
        lo_t = lo if terms == 2 else None
        want = bl.byte_linear_host(x, hi, lo_t, b, scale)
        S = s * (ax @ hi.double().abs().numpy().T) + (s * (ax @ lo.double().abs().numpy().T) if terms == 2 else 0.0) + b.double().abs().numpy()
        bound = 2 * (terms * K + 2) * U * S
        y = bl.byte_linear(dev, hi.cuda(), None if lo_t is None else lo.cuda(), b.cuda(), scale)
        err = np.abs(y.cpu().numpy().astype(np.float64) - want)
        print(f"forward N={N} K={K} H={H} terms={terms}: max err / (u S) = {(err / (U * S)).max():.3f} (allowed {2 * (terms * K + 2)})")
        assert (err <= bound).all()
        y16 = bl.byte_linear(dev, hi.cuda(), None if lo_t is None else lo.cuda(), b.cuda(), scale, out_dtype=torch.bfloat16)
        assert torch.equal(y16, y.to(torch.bfloat16))
        assert (np.abs(y16.float().cpu().numpy().astype(np.float64) - want) <= bound + 2.0 ** -8 * np.abs(want)).all()
        # weight gradient: float32 dy (split for two terms), and bfloat16 dy
        for d in (dy, dy.to(torch.bfloat16)):
            dterms = terms if d.dtype == torch.float32 else 1
            want_g = bl.byte_linear_wgrad_host(x, d, scale, dterms)
            d32 = d.float().numpy()
            dhi = bl._bf16_round_np(d32)
            Sg = s * (np.abs(dhi).astype(np.float64).T @ ax)
            if dterms == 2:
                Sg = Sg + s * (np.abs(bl._bf16_round_np(d32 - dhi)).astype(np.float64).T @ ax)
            got = wgrad(dev, d.cuda(), scale, terms)
            gerr = np.abs(got.cpu().numpy().astype(np.float64) - want_g)
            ratio = (gerr / np.where(Sg > 0, U * Sg, 1.0)).max()
            print(f"wgrad N={N} K={K} H={H} terms={terms} dy={d.dtype}: max err / (u S) = {ratio:.3f} (allowed {2 * (dterms * N + 2)})")
            assert (gerr <= 2 * (dterms * N + 2) * U * Sg).all()


@pytest.fixture(scope="module")
def engine_rows():
    """u8 [E * A, T, 3] on the device: the observation rows of a 64-env rung-3 engine after a few random steps."""
    from mettagrid_amd import presets
    from mettagrid_amd.compiler import compile_spec
    from mettagrid_amd.engine import BatchedMettaGrid
    from mettagrid_amd.mapgen import random_class_maps
    E = 64
    prog = compile_spec(presets.rung3_spec(), 32, 32, max_objects=192)
    cms = random_class_maps(prog, 32, 32, {"wall": 40, "extractor": 8, "chest": 4}, {"red": 8, "blue": 8}, range(E))
    eng = BatchedMettaGrid(prog, cms, np.arange(E, dtype=np.uint32), buffers="device", specialize=False)
    gen = torch.Generator(device="cuda").manual_seed(3)
    n = len(prog.action_names)
    for _ in range(4):
        eng.actions.copy_(torch.randint(0, n, tuple(eng.actions.shape), dtype=torch.int32, device="cuda", generator=gen))
        eng.vibe_actions.copy_(torch.randint(0, n, tuple(eng.actions.shape), dtype=torch.int32, device="cuda", generator=gen))
        torch.cuda.synchronize()
        eng.step()
        eng.sync()
    obs = eng.obs.clone()
    eng.close()
    return obs


@pytest.mark.parametrize("precision", ["bf16", "bf16x2"])
def test_layer_on_engine_rows(precision, engine_rows):
    """ByteRowLinear on the device against its CPU path (float64 on the same operands, rounded once), on the engine's own
    rows."""
    E, obs = 64, engine_rows
    N, T = obs.shape[0], obs.shape[1]
    K, H, terms = 3 * T, 128, bl.PRECISIONS[precision]
    assert (obs[..., 0] != 0xFF).any().item()
    torch.manual_seed(11)
    cpu = bl.ByteRowLinear(K, H, precision=precision)
    dev = bl.ByteRowLinear.from_linear(cpu, precision=precision).cuda()
    G = torch.randn(N, H, generator=torch.Generator().manual_seed(12))
    obs_cpu = obs.cpu()
    y_cpu = cpu(obs_cpu)
    y_cpu.backward(G)
    y_dev = dev(obs.view(E, N // E, T, 3))                  # leading dimensions are flattened
    assert tuple(y_dev.shape) == (E, N // E, H) and y_dev.dtype == torch.float32
    y_dev.backward(G.cuda().view(E, N // E, H))
    s = float(np.float32(1.0 / 255.0))
    ax = obs_cpu.reshape(N, K).numpy().astype(np.float64)
    hi, lo = bl.split_bf16(cpu.weight)
    S = s * (ax @ hi.double().abs().numpy().T) + (s * (ax @ lo.double().abs().numpy().T) if terms == 2 else 0.0) + cpu.bias.detach().double().abs().numpy()
    err = np.abs(y_dev.detach().reshape(N, H).cpu().numpy().astype(np.float64) - y_cpu.detach().numpy().astype(np.float64))
    assert (err <= 2 * (terms * K + 2) * U * S + U * np.abs(y_cpu.detach().numpy())).all()      # (+ the CPU path's one rounding)
    d32 = G.numpy()
    dhi = bl._bf16_round_np(d32)
    Sg = s * (np.abs(dhi).astype(np.float64).T @ ax)
    if terms == 2:
        Sg = Sg + s * (np.abs(bl._bf16_round_np(d32 - dhi)).astype(np.float64).T @ ax)
    gerr = np.abs(dev.weight.grad.cpu().numpy().astype(np.float64) - cpu.weight.grad.numpy().astype(np.float64))
    assert (gerr <= 2 * (terms * N + 2) * U * Sg + U * np.abs(cpu.weight.grad.numpy())).all()
    berr = np.abs(dev.bias.grad.cpu().numpy().astype(np.float64) - cpu.bias.grad.numpy().astype(np.float64))
    assert (berr <= 2 * N * U * np.abs(d32).astype(np.float64).sum(0)).all()                      # dy.sum(0) in float32 on both sides


def test_refusals_and_no_rows():
    L = load_lib()
    N, K, H = 5, 40, 32
    x = torch.zeros((N, K), dtype=torch.uint8, device="cuda")
    w = torch.zeros((H, K), dtype=torch.bfloat16, device="cuda")
    w24 = torch.zeros((24, K), dtype=torch.bfloat16, device="cuda")
    b = torch.zeros(H, device="cuda")
    y = torch.full((N, H), 3.0, device="cuda")
    dy = torch.zeros((N, H), device="cuda")
    dw = torch.full((H, K), 3.0, device="cuda")
    scratch = torch.zeros(L.mgx_byte_linear_scratch_bytes(N, K, H), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    X, W, B, Y, DY, DW, SC = (t.data_ptr() for t in (x, w, b, y, dy, dw, scratch))
    # ---- C level: MGX_ERR_BAD_ARG (-1) before anything is enqueued ----
    ok = (X, N, K, K, W, None, 1, B, 1.0, Y, 1, H, H, st)
    bad = [
        (X, N, K, K, W, None, 1, B, 1.0, Y, 1, 24, 24, st),      # H = 24
        (X, N, 0, K, W, None, 1, B, 1.0, Y, 1, H, H, st),        # K = 0
        (X, N, 65536, 65536, W, None, 1, B, 1.0, Y, 1, H, H, st),
        (X, N, K, K, W, None, 1, B, 1.0, Y, 1, 4112, 4112, st),  # H past the limit
        (None, N, K, K, W, None, 1, B, 1.0, Y, 1, H, H, st),     # null pointers
        (X, N, K, K, None, None, 1, B, 1.0, Y, 1, H, H, st),
        (X, N, K, K, W, None, 2, B, 1.0, Y, 1, H, H, st),        # two terms without w_lo
        (X, N, K, K, W, None, 1, B, 1.0, None, 1, H, H, st),
        (X, N, K, K, W, None, 3, B, 1.0, Y, 1, H, H, st),
        (X, N, K, K, W, None, 1, B, 1.0, Y, 0, H, H, st),
        (X, N, K, K - 1, W, None, 1, B, 1.0, Y, 1, H, H, st),    # a row stride below K
        (X, N, K, K, W, None, 1, B, 1.0, Y, 1, H - 1, H, st),
        (X, -1, K, K, W, None, 1, B, 1.0, Y, 1, H, H, st),
    ]
    for args in bad:
        assert L.mgx_byte_linear_forward(*args) == -1, args
    gok = (X, N, K, K, DY, 1, H, 2, 1.0, DW, SC, st)
    gbad = [(X, N, K, K, DY, 1, 24, 2, 1.0, DW, SC, st), (X, N, 0, K, DY, 1, H, 2, 1.0, DW, SC, st), (None, N, K, K, DY, 1, H, 2, 1.0, DW, SC, st),
            (X, N, K, K, None, 1, H, 2, 1.0, DW, SC, st), (X, N, K, K, DY, 1, H, 2, 1.0, None, SC, st), (X, N, K, K, DY, 1, H, 2, 1.0, DW, None, st),
            (X, N, K, K, DY, 3, H, 2, 1.0, DW, SC, st), (X, N, K, K, DY, 1, H, 0, 1.0, DW, SC, st)]
    for args in gbad:
        assert L.mgx_byte_linear_wgrad(*args) == -1, args
    # N = 0: accepted, nothing enqueued
    assert L.mgx_byte_linear_forward(None, 0, K, K, W, None, 1, B, 1.0, None, 1, H, H, st) == 0
    assert L.mgx_byte_linear_wgrad(None, 0, K, K, None, 1, H, 2, 1.0, DW, SC, st) == 0
    assert L.mgx_byte_linear_scratch_bytes(0, K, H) == 0
    torch.cuda.synchronize()
    assert (y == 3.0).all().item() and (dw == 3.0).all().item()
    # ... and the valid calls through the same path do write
    assert L.mgx_byte_linear_forward(*ok) == 0 and L.mgx_byte_linear_wgrad(*gok) == 0
    torch.cuda.synchronize()
    assert not y.any().item() and not dw.any().item()
    # ---- Python level: ValueError before the library is called ----
    calls = [lambda: bl.byte_linear(x, w24), lambda: bl.byte_linear(x[:, :0], w[:, :0]), lambda: bl.byte_linear(x.float(), w),
             lambda: bl.byte_linear(x, w.float()), lambda: bl.byte_linear(x, w[:, :-1]), lambda: bl.byte_linear(x, w, w24),
             lambda: bl.byte_linear(x, w, None, b.double()), lambda: bl.byte_linear(x, w, None, b[:-1]), lambda: bl.byte_linear(x.cpu(), w),
             lambda: bl.byte_linear(x, w, out=torch.zeros((N, H), dtype=torch.float16, device="cuda")),
             lambda: bl.byte_linear(x, w, out=torch.zeros((H, N), device="cuda").t()), lambda: bl.byte_linear(x, w, out=y[:-1]),
             lambda: bl.byte_linear(x, w, out_dtype=torch.float16), lambda: bl.byte_linear(x.t(), w[:, :N]),
             lambda: bl.byte_linear_wgrad(x, dy.double()), lambda: bl.byte_linear_wgrad(x, dy[:-1]), lambda: bl.byte_linear_wgrad(x, dy[:, :24].contiguous()),
             lambda: bl.byte_linear_wgrad(x, dy, terms=3), lambda: bl.byte_linear_wgrad(x, dy, scratch=scratch[:-1])]
    for f in calls:
        with pytest.raises(ValueError):
            f()
    # no rows through Python: an empty output, a zero gradient, a layer that still works
    assert tuple(bl.byte_linear(x[:0], w).shape) == (0, H)
    g0 = bl.byte_linear_wgrad(x[:0], dy[:0], terms=2)
    assert tuple(g0.shape) == (H, K) and not g0.any().item()
    m = bl.ByteRowLinear(K, H).cuda()
    out = m(x[:0])
    out.sum().backward()
    assert tuple(out.shape) == (0, H) and not m.weight.grad.any().item()
