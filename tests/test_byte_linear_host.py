"""Host: the dense-policy front end (mettagrid_amd/byte_linear.py) against the reference's form, restated:
python/src/mettagrid/policy/stateless.py:29,42 (and lstm.py:31-37,73-84) flatten a row, ``observations.view(B, -1).float() /
255.0``, and feed it to ``Linear(3T, 128)``.  Here that form runs in float64 on the float32 weights:
``F.linear(x.reshape(N, -1).double() * scale, W.double(), b.double())``.

Bounds (nothing tuned): the two-term weights differ from W by ``r = W - hi - lo`` exactly (float64 differences of float32
values), so the operator differs from the reference form by at most ``scale * sum_k |x| |r|`` plus the float64 rounding of two
600-term sums (``4 K 2**-53`` of ``scale * sum |x| |W|``); the CPU path of the layer adds one rounding to float32 (``2**-24 |y|``).
A float32 ``dy`` used as hi + lo is off by at most ``2**-16 |dy|`` per element."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mettagrid_amd import byte_linear as bl

U = 2.0 ** -24
N, T, H = 37, 50, 48
K = 3 * T


def rows(n=N, t=T, seed=0) -> np.ndarray:
    """Observation-like rows: a used prefix of random bytes, 0xFF padding behind it; row 0 empty, row 1 full."""
    rng = np.random.default_rng(seed)
    x = np.full((n, t, 3), 0xFF, np.uint8)
    for r in range(n):
        used = 0 if r == 0 else t if r == 1 else int(rng.integers(0, t + 1))
        x[r, :used] = rng.integers(0, 256, (used, 3))
    return x


def reference_form(x: np.ndarray, w: torch.Tensor, b, scale: float) -> torch.Tensor:
    """stateless.py:29,42 in float64 with the float32 weights."""
    xs = torch.from_numpy(x).reshape(x.shape[0], -1).double() * float(np.float32(scale))
    return F.linear(xs, w.double(), None if b is None else b.double())


def test_split_bf16():
    g = torch.Generator().manual_seed(1)
    w = torch.cat([torch.randn(4000, generator=g) * 0.1, torch.randn(96, generator=g) * 1e4, torch.tensor([0.0, 1.0, -1.0, 255.0, 2.0 ** -20])])
    hi, lo = bl.split_bf16(w)
    assert hi.dtype == torch.bfloat16 and lo.dtype == torch.bfloat16 and hi.shape == w.shape
    w64 = w.double()
    res = (w64 - hi.double() - lo.double()).abs()
    print(f"split_bf16: max |w - hi - lo| / |w| = 2**{np.log2((res / w64.abs().clamp_min(1e-300)).max().item()):.1f}")
    assert (res <= 2.0 ** -16 * w64.abs()).all()
    assert torch.equal(hi, w.to(torch.bfloat16))
    # numpy in, float32 arrays of bfloat16-representable values out, the same values
    nhi, nlo = bl.split_bf16(w.numpy())
    assert nhi.dtype == np.float32 and nlo.dtype == np.float32
    for a, t in ((nhi, hi), (nlo, lo)):
        assert not (a.view(np.uint32) & 0xFFFF).any()                 # bfloat16-representable
        assert np.array_equal(a, t.float().numpy())


def test_host_form_against_the_reference_form():
    x = rows()
    g = torch.Generator().manual_seed(2)
    w = torch.randn(H, K, generator=g) * 0.1
    b = torch.randn(H, generator=g)
    scale = 1.0 / 255.0
    hi, lo = bl.split_bf16(w)
    got = bl.byte_linear_host(x, hi, lo, b, scale)
    want = reference_form(x, w, b, scale).numpy()
    ax = x.reshape(N, -1).astype(np.float64)
    r = (w.double() - hi.double() - lo.double()).abs().numpy()
    s = float(np.float32(scale))
    bound = s * (ax @ r.T) + 4 * K * 2.0 ** -53 * (s * (ax @ w.double().abs().numpy().T) + b.double().abs().numpy())
    err = np.abs(got - want)
    print(f"two terms against the reference form: max err / bound = {(err / np.where(bound > 0, bound, 1.0)).max():.3f}")
    assert (err <= bound).all()
    # one term: the same bound with r = w - hi
    got1 = bl.byte_linear_host(x, hi, None, b, scale)
    r1 = (w.double() - hi.double()).abs().numpy()
    assert (np.abs(got1 - want) <= s * (ax @ r1.T) + 4 * K * 2.0 ** -53 * (s * (ax @ w.double().abs().numpy().T) + b.double().abs().numpy())).all()
    assert (np.abs(got1 - want) > bound).any()                         # (and one term is visibly coarser than two)


def test_wgrad_host_form():
    x = rows(seed=3)
    g = torch.Generator().manual_seed(4)
    dy = torch.randn(N, H, generator=g)
    scale = 1.0 / 255.0
    s = float(np.float32(scale))
    ax = x.reshape(N, -1).astype(np.float64)
    want = s * (dy.double().numpy().T @ ax)
    for terms, rel in ((2, 2.0 ** -16), (1, 2.0 ** -8)):
        got = bl.byte_linear_wgrad_host(x, dy, scale, terms)
        bound = (rel + 4 * N * 2.0 ** -53) * s * (dy.double().abs().numpy().T @ ax)
        assert got.shape == (H, K) and (np.abs(got - want) <= bound).all(), terms
    # a bfloat16 dy is used as it is, whatever the terms
    d16 = dy.to(torch.bfloat16)
    assert np.array_equal(bl.byte_linear_wgrad_host(x, d16, scale, 2), s * (d16.double().numpy().T @ ax))


@pytest.mark.parametrize("precision", ["bf16", "bf16x2"])
def test_layer_on_cpu_tensors(precision):
    x = rows(seed=5)
    torch.manual_seed(6)
    m = bl.ByteRowLinear(K, H, precision=precision)
    assert [n for n, _ in m.named_parameters()] == ["weight", "bias"]
    assert tuple(m.weight.shape) == (H, K) and tuple(m.bias.shape) == (H,) and m.weight.dtype == torch.float32
    obs = torch.from_numpy(x)
    y = m(obs)
    assert y.dtype == torch.float32 and tuple(y.shape) == (N, H) and y.requires_grad
    terms = bl.PRECISIONS[precision]
    rel = 2.0 ** -16 if terms == 2 else 2.0 ** -8
    s = float(np.float32(1.0 / 255.0))
    ax = x.reshape(N, -1).astype(np.float64)
    w64, b64 = m.weight.detach().double(), m.bias.detach().double()
    want = reference_form(x, m.weight.detach(), m.bias.detach(), 1.0 / 255.0)
    mag = s * (ax @ w64.abs().numpy().T) + b64.abs().numpy()
    err = np.abs(y.detach().double().numpy() - want.numpy())
    assert (err <= (rel + 4 * K * 2.0 ** -53) * mag + U * np.abs(want.numpy())).all()
    # gradients against autograd through the reference form in float64
    G = torch.randn(N, H, generator=torch.Generator().manual_seed(7))
    y.backward(G)
    wref, bref = w64.clone().requires_grad_(), b64.clone().requires_grad_()
    F.linear(torch.from_numpy(x).reshape(N, -1).double() * s, wref, bref).backward(G.double())
    gmag = s * (G.double().abs().numpy().T @ ax)
    gerr = np.abs(m.weight.grad.double().numpy() - wref.grad.numpy())
    assert m.weight.grad.dtype == torch.float32
    assert (gerr <= (rel + 4 * N * 2.0 ** -53) * gmag + U * np.abs(wref.grad.numpy())).all()
    berr = np.abs(m.bias.grad.double().numpy() - bref.grad.numpy())
    assert (berr <= 2 * N * U * G.double().abs().sum(0).numpy()).all()   # dy.sum(0) in float32
    assert obs.grad is None


def test_layer_takes_linear_weights_and_batches():
    torch.manual_seed(8)
    lin = torch.nn.Linear(K, H)
    m = bl.ByteRowLinear.from_linear(lin, precision="bf16x2")
    assert torch.equal(m.weight, lin.weight) and torch.equal(m.bias, lin.bias) and m.weight is not lin.weight
    m2 = bl.ByteRowLinear(K, H)
    m2.load_state_dict(lin.state_dict())                  # nn.Linear's names and shapes
    assert torch.equal(m2.weight, lin.weight) and torch.equal(m2.bias, lin.bias)
    assert set(m2.state_dict()) == set(lin.state_dict())
    nb = bl.ByteRowLinear.from_linear(torch.nn.Linear(K, H, bias=False))
    assert nb.bias is None and set(nb.state_dict()) == {"weight"}
    # [segments, bptt, T, 3] and [segments, bptt, K] give [segments, bptt, H], equal to the flat call
    x = torch.from_numpy(rows(n=12, seed=9))
    flat = m(x)
    assert torch.equal(m(x.reshape(3, 4, T, 3)), flat.reshape(3, 4, H))
    assert torch.equal(m(x.reshape(3, 4, K)), flat.reshape(3, 4, H))
    assert tuple(m(x[:0]).shape) == (0, H)
    # the init is nn.Linear's: the same draws from the same seed
    torch.manual_seed(10)
    a = torch.nn.Linear(K, H)
    torch.manual_seed(10)
    b = bl.ByteRowLinear(K, H)
    assert torch.equal(a.weight, b.weight) and torch.equal(a.bias, b.bias)
    # bfloat16 output: the float32 result rounded
    m16 = bl.ByteRowLinear.from_linear(lin, precision="bf16x2", out_dtype=torch.bfloat16)
    assert torch.equal(m16(x), flat.to(torch.bfloat16))


def test_value_errors():
    for kw in (dict(in_features=0, out_features=16), dict(in_features=65536, out_features=16), dict(in_features=K, out_features=24),
               dict(in_features=K, out_features=0), dict(in_features=K, out_features=bl.MAX_H + 16),
               dict(in_features=K, out_features=H, precision="fp8"), dict(in_features=K, out_features=H, out_dtype=torch.float16)):
        with pytest.raises(ValueError):
            bl.ByteRowLinear(**kw)
    with pytest.raises(ValueError, match="65535"):
        bl.ByteRowLinear(70000, 16)
    with pytest.raises(ValueError, match="multiple of 16"):
        bl.ByteRowLinear(K, 24)
    m = bl.ByteRowLinear(K, H)
    x = torch.from_numpy(rows(n=4))
    for bad in (x.float(), x.to(torch.int8), x[:, :-1], x.reshape(4, K)[:, :-1], x.reshape(-1)):
        with pytest.raises(ValueError):
            m(bad)
    with pytest.raises(ValueError):
        bl.byte_linear_host(np.zeros((4, K), np.float32), np.zeros((H, K), np.float32))
    # the raw ops refuse host tensors: there is no CPU kernel behind them
    hi, lo = bl.split_bf16(m.weight)
    with pytest.raises(ValueError):
        bl.byte_linear(x.reshape(4, K), hi, lo)
    with pytest.raises(ValueError):
        bl.byte_linear_wgrad(x.reshape(4, K), torch.zeros(4, H))
