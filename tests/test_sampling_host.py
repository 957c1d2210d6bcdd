"""Host side of the policy output path (mettagrid_amd/sampling.py), no GPU: the Philox known answers, the
float64 host functions against torch.distributions.Categorical and torch autograd, the independence of a row's draw from how
rows are split, the refusals of the three C entry points (made before anything is enqueued: they return on a host without a
device), and ActionSampler's state."""
import ctypes

import numpy as np
import pytest
import torch

from mettagrid_amd import sampling as sa
from mettagrid_amd.engine import load_lib

KNOWN = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


def test_philox_known_answers():
    for ctr, key, want in KNOWN:
        got = sa.philox4x32(np.array(ctr, np.uint32), np.array(key, np.uint32))
        assert got.dtype == np.uint32 and tuple(int(x) for x in got) == want
    # batched, and the kernel's counter / key layout: (row lo, row hi, step lo, step hi) under (seed lo, seed hi)
    ctrs = np.array([k[0] for k in KNOWN], np.uint32)
    keys = np.array([k[1] for k in KNOWN], np.uint32)
    assert np.array_equal(sa.philox4x32(ctrs, keys), np.array([k[2] for k in KNOWN], np.uint32))
    c, k, _ = KNOWN[2]
    c = (c[0], c[1] & 0x7FFFFFFF, c[2], c[3])         # (rows are int64)
    w = sa.philox4x32(np.array(c, np.uint32), np.array(k, np.uint32))
    u = sa.uniforms(seed=k[0] | k[1] << 32, step=c[2] | c[3] << 32, rows=[c[0] | c[1] << 32])
    assert u[0] == (int(w[0]) >> 8) * 2.0 ** -24 and 0.0 <= u[0] < 1.0


def masked_logits(n: int, a: int, seed: int) -> np.ndarray:
    """3 * normal float32, 10 % masked; row 0 all equal, row 1 one finite entry, row 2 a lead of 1e4."""
    rng = np.random.default_rng(seed)
    x = (3.0 * rng.standard_normal((n, a))).astype(np.float32)
    x[rng.random((n, a)) < 0.1] = -np.inf
    x[np.arange(n), rng.integers(0, a, n)] = rng.standard_normal(n).astype(np.float32)   # every row keeps a finite entry
    x[0] = 0.25
    if n > 1:
        x[1] = -np.inf
        x[1, (5 * a) // 7] = -2.0
    if n > 2 and a > 1:
        x[2] = rng.standard_normal(a).astype(np.float32)
        x[2, a // 3] += 1e4
    return x


@pytest.mark.parametrize("A", (1, 2, 5, 21, 130))
def test_host_functions_against_categorical(A):
    N = 37
    x = masked_logits(N, A, seed=A)
    act, lp, ent = sa.sample_host(x, seed=5, step=2)
    xt = torch.from_numpy(x).double().requires_grad_(True)
    dist = torch.distributions.Categorical(logits=xt)
    at = torch.from_numpy(act.astype(np.int64))
    want_lp, want_ent = dist.log_prob(at), dist.entropy()
    assert np.abs(lp - want_lp.detach().numpy()).max() <= 1e-12
    assert np.abs(ent - want_ent.detach().numpy()).max() <= 1e-12
    assert np.isfinite(lp).all()                      # a masked action was never drawn
    lp2, ent2, lse = sa.logprob_entropy_host(x, act)
    assert np.array_equal(lp2, lp) and np.array_equal(ent2, ent)
    assert np.abs(lse - torch.logsumexp(xt.detach(), 1).numpy()).max() <= 1e-12
    rng = np.random.default_rng(A)
    d_lp, d_ent = rng.standard_normal(N), rng.standard_normal(N)
    # Categorical.entropy() multiplies probabilities by logits clamped to the most negative float64: its autograd gives NaN
    # in rows with a masked entry.  Those rows take the same entropy written with the masked terms selected away (equal to
    # Categorical's in value); rows without a masked entry are also compared against Categorical's own graph.
    logp = xt - torch.logsumexp(xt, 1, keepdim=True)
    keep = torch.isfinite(xt.detach())
    safe = torch.where(keep, logp, torch.zeros_like(logp))
    guarded = -(torch.where(keep, safe.exp(), torch.zeros_like(logp)) * safe).sum(1)
    assert (guarded - want_ent).abs().max() <= 1e-12
    (want_lp * torch.from_numpy(d_lp) + guarded * torch.from_numpy(d_ent)).sum().backward(retain_graph=True)
    g = sa.logprob_entropy_grad_host(x, act, d_lp, d_ent)
    assert np.abs(g - xt.grad.numpy()).max() <= 1e-12
    full = keep.all(1).numpy()
    xt.grad = None
    (want_lp * torch.from_numpy(d_lp) + want_ent * torch.from_numpy(d_ent)).sum().backward()
    assert full.sum() >= (3 if A <= 5 else 0) and np.abs(g[full] - xt.grad.numpy()[full]).max(initial=0.0) <= 1e-12
    assert (g[np.isneginf(x)] == 0.0).all() and not np.signbit(g[np.isneginf(x)]).any()
    assert np.array_equal(sa.logprob_entropy_grad_host(x, act, d_lp, None), sa.logprob_entropy_grad_host(x, act, d_lp, np.zeros(N)))


def test_temperature_and_bf16_operands():
    x = masked_logits(19, 7, seed=3)
    act, lp, ent = sa.sample_host(x, 1, 1, inv_temperature=0.5)
    dist = torch.distributions.Categorical(logits=torch.from_numpy(x).double() * 0.5)
    assert np.abs(lp - dist.log_prob(torch.from_numpy(act.astype(np.int64))).numpy()).max() <= 1e-12
    assert np.abs(ent - dist.entropy().numpy()).max() <= 1e-12
    xb = torch.from_numpy(x).to(torch.bfloat16)       # taken at its exact values
    a1 = sa.sample_host(xb, 1, 1)
    a2 = sa.sample_host(xb.float().numpy(), 1, 1)
    assert all(np.array_equal(p, q) for p, q in zip(a1, a2))


def test_autograd_function_on_cpu_matches_categorical():
    x = masked_logits(23, 9, seed=11)
    act = torch.from_numpy(sa.sample_host(x, 0, 0)[0].astype(np.int64))
    for t in (1.0, 0.5, 2.0):
        a = torch.from_numpy(x).double().requires_grad_(True)
        b = torch.from_numpy(x).double().requires_grad_(True)
        lp, ent = sa.action_logprob_entropy(a, act, inv_temperature=t)
        dist = torch.distributions.Categorical(logits=b * t)
        w = torch.linspace(-1.0, 2.0, 23, dtype=torch.float64)
        (lp * w - 0.3 * ent).sum().backward()
        (dist.log_prob(act) * w - 0.3 * dist.entropy()).sum().backward()
        assert (lp - dist.log_prob(act)).abs().max() <= 1e-12 and (ent - dist.entropy()).abs().max() <= 1e-12
        assert (a.grad - b.grad).abs().max() <= 1e-12
    f = torch.from_numpy(x).requires_grad_(True)      # float32 in, float32 out, gradient in the logits' dtype
    lp, ent = sa.action_logprob_entropy(f.view(23, 1, 9), act.view(23, 1))
    lp.sum().backward()
    assert lp.dtype == torch.float32 and lp.shape == (23, 1) and f.grad.dtype == torch.float32 and f.grad.shape == (23, 9)


def test_draws_do_not_depend_on_the_split_and_change_with_seed_and_step():
    N, A = 300, 21
    x = masked_logits(N, A, seed=1)
    full = sa.sample_host(x, seed=9, step=4)
    rng = np.random.default_rng(0)
    perm = rng.permutation(N)
    for idx in (perm[:113], perm[113:]):
        part = sa.sample_host(x[idx], seed=9, step=4, rows=idx)
        assert all(np.array_equal(p, f[idx]) for p, f in zip(part, full))
    base = full[0]
    other_seed = sa.sample_host(x, seed=10, step=4)[0]
    other_step = sa.sample_host(x, seed=9, step=5)[0]
    high_step = sa.sample_host(x, seed=9, step=4 + (1 << 32))[0]
    assert (base != other_seed).mean() > 0.3 and (base != other_step).mean() > 0.3 and (base != high_step).mean() > 0.3
    assert np.array_equal(base, sa.sample_host(x, seed=9, step=4)[0])


def test_greedy_takes_the_lowest_index_among_ties():
    x = np.full((4, 6), -1.0, np.float32)
    x[0, [2, 4]] = 3.0
    x[1, :] = 0.5
    x[2, [0, 5]] = [-np.inf, 7.0]
    x[3, [1, 3, 5]] = 2.0
    act, lp, ent = sa.sample_host(x, 0, 0, greedy=True)
    assert act.tolist() == [2, 0, 5, 1]
    assert np.allclose(lp[1], -np.log(6.0), atol=1e-12) and np.allclose(ent[1], np.log(6.0), atol=1e-12)
    assert np.array_equal(act, sa.sample_host(x, 77, 12345, greedy=True)[0])       # no random number


def test_histogram_of_one_row():
    n = 65536
    l = np.array([0.3, -np.inf, 1.7, -0.9, 0.0], np.float32)
    act = sa.sample_host(np.broadcast_to(l, (n, 5)), seed=2, step=0)[0]
    p = np.exp(l.astype(np.float64))
    p /= p.sum()
    counts = np.bincount(act, minlength=5)
    sigma = np.sqrt(n * p * (1 - p))
    assert counts[1] == 0
    assert (np.abs(counts - n * p) <= 5 * sigma).all(), (counts, n * p)


def test_bad_rows_on_the_host():
    x = np.zeros((5, 4), np.float32)
    x[1] = -np.inf
    x[2, 1] = np.nan
    x[3, 3] = np.inf
    act, lp, ent = sa.sample_host(x, 0, 0)
    assert act[[1, 2, 3]].tolist() == [0, 0, 0] and np.isnan(lp[[1, 2, 3]]).all() and np.isnan(ent[[1, 2, 3]]).all()
    assert np.isfinite(lp[[0, 4]]).all()
    lp, ent, lse = sa.logprob_entropy_host(x, np.array([0, 0, 0, 0, 4]))
    assert np.isnan(lp[1:]).all() and np.isnan(lse[1:]).all() and np.isfinite(lp[0])


def _sample_args(**kw):
    a = dict(logits=0x10000, dtype=1, n=8, A=5, stride=5, rows=None, t=1.0, mode=0, seed=1, step=2, actions=0x20000, logprob=0x30000,
             entropy=0x40000, bad=0x50000, stream=None)
    a.update(kw)
    return [a[k] for k in ("logits", "dtype", "n", "A", "stride", "rows", "t", "mode", "seed", "step", "actions", "logprob", "entropy", "bad",
                           "stream")]


def _logprob_args(**kw):
    a = dict(logits=0x10000, dtype=1, n=8, A=5, stride=8, actions=0x20000, t=1.0, logprob=0x30000, entropy=0x40000, lse=0x50000, bad=None,
             stream=None)
    a.update(kw)
    return [a[k] for k in ("logits", "dtype", "n", "A", "stride", "actions", "t", "logprob", "entropy", "lse", "bad", "stream")]


def _backward_args(**kw):
    a = dict(logits=0x10000, dtype=1, n=8, A=5, stride=5, actions=0x20000, t=1.0, lse=0x30000, d_lp=0x40000, d_ent=None, d_logits=0x50000,
             d_dtype=2, d_stride=5, stream=None)
    a.update(kw)
    return [a[k] for k in ("logits", "dtype", "n", "A", "stride", "actions", "t", "lse", "d_lp", "d_ent", "d_logits", "d_dtype", "d_stride",
                           "stream")]


COMMON_REFUSALS = (dict(logits=None), dict(logits=0x10002), dict(dtype=0), dict(dtype=3), dict(A=0), dict(A=4097), dict(n=-1), dict(n=(1 << 25) + 1),
                   dict(stride=4), dict(t=0.0), dict(t=-1.0), dict(t=float("inf")), dict(t=float("nan")), dict(actions=None),
                   dict(actions=0x20002))


def test_refusals_through_the_c_abi():
    """Every refusal returns MGX_ERR_BAD_ARG (-1) here, where no device exists: the check comes before any enqueue.  (The
    pointers are never dereferenced on the host.)"""
    L = load_lib()
    for kw in COMMON_REFUSALS + (dict(mode=2), dict(mode=-1), dict(rows=0x60004), dict(logprob=0x30001), dict(entropy=0x40002),
                                 dict(bad=0x50001), dict(dtype=2, logits=0x10001)):
        assert L.mgx_sample_actions(*_sample_args(**kw)) == -1, kw
    for kw in COMMON_REFUSALS + (dict(logprob=None), dict(logprob=0x30002), dict(entropy=0x40001), dict(lse=0x50002), dict(bad=0x50003),
                                 dict(dtype=2, logits=0x10001)):
        assert L.mgx_action_logprob(*_logprob_args(**kw)) == -1, kw
    for kw in COMMON_REFUSALS + (dict(lse=None), dict(lse=0x30001), dict(d_lp=0x40002), dict(d_ent=0x40001), dict(d_logits=None),
                                 dict(d_logits=0x50001), dict(d_dtype=0), dict(d_dtype=3), dict(d_stride=4),
                                 dict(d_dtype=1, d_logits=0x50002)):
        assert L.mgx_action_logprob_backward(*_backward_args(**kw)) == -1, kw
    # N = 0 with sound arguments enqueues nothing and succeeds
    assert L.mgx_sample_actions(*_sample_args(n=0)) == 0
    assert L.mgx_action_logprob(*_logprob_args(n=0)) == 0
    assert L.mgx_action_logprob_backward(*_backward_args(n=0)) == 0
    assert ctypes.sizeof(ctypes.c_void_p) == 8


def test_python_ops_refuse_what_the_kernels_refuse():
    x = torch.zeros((4, 5))
    a = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError):
        sa.sample_actions(x, a, 0, 0)                  # not a device tensor
    with pytest.raises(ValueError):
        sa.action_logprob(x, a)
    with pytest.raises(ValueError):
        sa.action_logprob_backward(x, a, torch.zeros(4))
    with pytest.raises(ValueError):
        sa.action_logprob_entropy(x, torch.zeros(4, dtype=torch.int64), inv_temperature=0.0)
    with pytest.raises(ValueError):
        sa.sample_host(np.zeros((2, 3), np.float32), 0, 0, inv_temperature=-1.0)
    with pytest.raises(ValueError):
        sa.ActionSampler(4, 4097, device="cpu")


def test_action_sampler_state_round_trip():
    N, A = 40, 6
    x = torch.from_numpy(masked_logits(N, A, seed=8))
    s = sa.ActionSampler(N, A, seed=123, device="cpu")
    assert s.actions.dtype == torch.int32 and s.actions.shape == (N,) and s.state_dict() == {"seed": 123, "step": 0}
    with pytest.raises(ValueError):
        s.sample(x, advance=False)                    # no step begun yet
    first = [t.clone() for t in s.sample(x)]
    want = sa.sample_host(x, 123, 0)
    assert np.array_equal(first[0].numpy(), want[0]) and np.allclose(first[1].numpy(), want[1], rtol=1e-6)
    state = s.state_dict()
    assert state == {"seed": 123, "step": 1}
    second = [t.clone() for t in s.sample(x)]
    assert not torch.equal(first[0], second[0])
    # two policies of one step: the halves drawn with advance=False equal the single call
    t2 = sa.ActionSampler(N, A, seed=0, device="cpu")
    t2.load_state_dict(state)
    rows_a, rows_b = torch.arange(0, N, 2), torch.arange(1, N, 2)
    t2.sample(x[rows_a], rows=rows_a)
    got = [t.clone() for t in t2.sample(x[rows_b], rows=rows_b, advance=False)]
    assert t2.state_dict() == s.state_dict() == {"seed": 123, "step": 2}
    assert all(torch.equal(g, w) for g, w in zip(got, second))
    t2.check()
    with pytest.raises(ValueError):
        t2.sample(x[rows_a], rows=rows_a + N)         # outside the joint tensor
    bad = x.clone()
    bad[3] = float("nan")
    t2.sample(bad)
    with pytest.raises(RuntimeError):
        t2.check()
    t2.check()                                        # the counter was cleared
