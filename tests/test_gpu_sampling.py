"""GPU: the policy output side (csrc/mgx_sample.hip, mettagrid_amd/sampling.py) against the float64 host
functions on the kernels' own operands (z = fl32(t * l), bfloat16 logits at their exact values).

Bounds, with u = 2**-24 and per row D = the largest finite |z_a - m| (derived, not tuned; each is the first-order bound of a
sequential float32 sum of A non-negative terms plus exp / log within 4 ulp and the closing operations, doubled: the project's
usual margin):
  sampled action   equal to sample_host's, or the neighbouring positive-probability action with the float64 normalised CDF
                   boundary between the two within delta = 2 u (A + 16) of the row's u; at most 2 % of a case's rows may
                   use that allowance; a masked action is never returned
  logprob, lse     |d| <= 2 u (A + 16 + 4 (max|z| + D))
  entropy          |d| <= 2 u (A + 16) (1 + ln A + D)
  backward         |d| <= 2 u t (A + 16 + D) (|d_logprob| + |d_entropy| (1 + D + 2 ln A)), bfloat16 output + 2**-8 |g|;
                   masked entries exactly 0.0
Greedy actions are compared exactly: the host forms z in float32 as the kernels do, so equal float32 maxima are ties on both
sides and both take the lowest index."""
import numpy as np
import pytest
import torch

from mettagrid_amd import presets
from mettagrid_amd import sampling as sa
from mettagrid_amd.compiler import compile_spec
from mettagrid_amd.envs import MettaGridBatchedEnv

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
NS, AS = (1, 63, 64, 65, 4099), (1, 2, 5, 21, 64, 65, 130)
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
SEED, STEP = 0x123456789ABCDEF, (7 << 32) | 5


@pytest.fixture(scope="module")
def tail_buffer():
    """A 12 MiB allocation of its own (the caching allocator serves a request of that size with one device allocation of
    exactly that size): logits placed at its end end where the allocation ends."""
    torch.cuda.empty_cache()
    return torch.empty(12 << 20, dtype=torch.uint8, device="cuda")


def make_logits(n: int, a: int, seed: int, dtype) -> np.ndarray:
    """float32 [n, a] holding values of `dtype`: 3 * normal, 10 % masked; row 0 all equal, row 1 one finite entry, row 2 a
    lead of 1e4 over the rest."""
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
    return torch.from_numpy(x).to(dtype).float().numpy()


def sparse_logits(n: int, a: int, seed: int, dtype) -> np.ndarray:
    """Only the entries at {0, 63, 64, 2047, a - 97, a - 1} (those inside the row) are finite."""
    rng = np.random.default_rng(seed)
    x = np.full((n, a), -np.inf, np.float32)
    for p in (0, 63, 64, 2047, a - 97, a - 1):
        if 0 <= p < a:
            x[:, p] = (3.0 * rng.standard_normal(n)).astype(np.float32)
    return torch.from_numpy(x).to(dtype).float().numpy()


def on_device(x: np.ndarray, dtype, stride: int = 0) -> torch.Tensor:
    """x as a device tensor of `dtype`, rows `stride` elements apart (0: back to back); the gaps hold NaN."""
    n, a = x.shape
    if not stride or stride == a:
        return torch.from_numpy(x).to(dtype).cuda()
    big = torch.full((n, stride), float("nan"), dtype=dtype, device="cuda")
    big[:, :a] = torch.from_numpy(x).to(dtype).cuda()
    return big[:, :a]


def row_terms(x: np.ndarray, t: float):
    """float64 per row: z, pt, S, D, max|z|."""
    z = sa._z64(x, t)
    fin = np.isfinite(z)
    m = np.where(fin, z, -np.inf).max(1)
    pt = np.where(fin, np.exp(np.where(fin, z - m[:, None], 0.0)), 0.0)
    D = np.where(fin, np.abs(z - m[:, None]), 0.0).max(1)
    zmax = np.where(fin, np.abs(z), 0.0).max(1)
    return z, pt, pt.sum(1), D, zmax


def check_sampled(x, t, got, rows, seed, step, what):
    """The sampled-action rule of the module docstring; returns the number of rows that used the allowance."""
    n, a = x.shape
    want = sa.sample_host(x, seed, step, rows, t)[0]
    z, pt, S, _, _ = row_terms(x, t)
    assert got.min() >= 0 and got.max() < a, what
    assert (pt[np.arange(n), got] > 0).all(), f"{what}: a masked action was returned"
    diff = np.nonzero(got != want)[0]
    if diff.size:
        u = sa.uniforms(seed, step, np.arange(n) if rows is None else rows)
        c = np.cumsum(pt, axis=1) / S[:, None]
        delta = 2 * U * (a + 16)
        for i in diff:
            lo, hi = sorted((int(got[i]), int(want[i])))
            assert not (pt[i, lo + 1:hi] > 0).any(), f"{what}: row {i} got {got[i]}, want {want[i]}: not neighbours"
            assert abs(c[i, lo] - u[i]) <= delta, f"{what}: row {i} got {got[i]}, want {want[i]}: boundary {c[i, lo]} u {u[i]}"
        assert diff.size <= 0.02 * n, f"{what}: {diff.size} of {n} rows used the allowance"
    return int(diff.size)


def check_logprob_entropy(x, t, act, lp, ent, lse, what):
    n, a = x.shape
    want_lp, want_ent, want_lse = sa.logprob_entropy_host(x, act, t)
    _, _, _, D, zmax = row_terms(x, t)
    tol_lp = 2 * U * (a + 16 + 4 * (zmax + D))
    tol_ent = 2 * U * (a + 16) * (1 + np.log(a) + D)
    d_lp, d_ent = np.abs(lp.astype(np.float64) - want_lp), np.abs(ent.astype(np.float64) - want_ent)
    print(f"{what}: max |d logprob| / tol {np.max(d_lp / tol_lp):.3f}, max |d entropy| / tol {np.max(d_ent / tol_ent):.3f}")
    assert (d_lp <= tol_lp).all(), f"{what}: logprob off by {d_lp.max()} (row {int(np.argmax(d_lp / tol_lp))})"
    assert (d_ent <= tol_ent).all(), f"{what}: entropy off by {d_ent.max()} (row {int(np.argmax(d_ent / tol_ent))})"
    if lse is not None:
        d_lse = np.abs(lse.astype(np.float64) - want_lse)
        assert (d_lse <= tol_lp).all(), f"{what}: lse off by {d_lse.max()}"


def run_case(x: np.ndarray, dtype, stride: int, t: float, what: str, dev=None):
    """Sampler, greedy, log-probability and backward of one logits array, every output against the host functions."""
    n, a = x.shape
    dev = on_device(x, dtype, stride) if dev is None else dev
    act = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    lp, ent = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    sa.sample_actions(dev, act, SEED, STEP, None, t, False, lp, ent, bad)
    got = act.cpu().numpy()
    used = check_sampled(x, t, got, None, SEED, STEP, what)
    check_logprob_entropy(x, t, got, lp.cpu().numpy(), ent.cpu().numpy(), None, what + " sampled")
    # greedy: exact
    g_act = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    sa.sample_actions(dev, g_act, SEED, STEP, None, t, True, lp, ent, bad)
    want_g = sa.sample_host(x, SEED, STEP, None, t, greedy=True)[0]
    assert np.array_equal(g_act.cpu().numpy(), want_g), what + " greedy"
    check_logprob_entropy(x, t, want_g, lp.cpu().numpy(), ent.cpu().numpy(), None, what + " greedy")
    # log-probability of the sampled actions, then the gradient
    lp2, ent2, lse = sa.action_logprob(dev, act, t, bad_rows=bad)
    check_logprob_entropy(x, t, got, lp2.cpu().numpy(), ent2.cpu().numpy(), lse.cpu().numpy(), what + " logprob")
    assert int(bad.item()) == 0, what
    rng = np.random.default_rng(n * 131 + a)
    d_lp = rng.standard_normal(n).astype(np.float32)
    d_ent = rng.standard_normal(n).astype(np.float32)
    _, _, _, D, _ = row_terms(x, t)
    masked = np.isneginf(x)
    for out_dtype in (torch.float32, torch.bfloat16):
        for with_ent in (True, False):
            g = sa.action_logprob_backward(dev, act, lse, torch.from_numpy(d_lp).cuda(), torch.from_numpy(d_ent).cuda() if with_ent else None,
                                           t, out_dtype=out_dtype)
            assert g.dtype == out_dtype and tuple(g.shape) == (n, a)
            gh = g.float().cpu().numpy()
            want = sa.logprob_entropy_grad_host(x, got, d_lp, d_ent if with_ent else None, t)
            tol = 2 * U * t * (a + 16 + D) * (np.abs(d_lp) + (np.abs(d_ent) if with_ent else 0.0) * (1 + D + 2 * np.log(a)))
            tol = np.broadcast_to(tol[:, None], want.shape) + (2.0 ** -8 * np.abs(want) if out_dtype == torch.bfloat16 else 0.0)
            d = np.abs(gh - want)
            assert (d <= tol).all(), f"{what} backward {out_dtype} entropy={with_ent}: off by {d.max()} at {np.unravel_index(np.argmax(d - tol), d.shape)}"
            assert (gh[masked] == 0.0).all(), f"{what} backward: a masked entry is not 0"
    return used


@pytest.mark.parametrize("A", AS)
@pytest.mark.parametrize("kind", list(DTYPES))
def test_shapes_against_the_host_functions(A, kind):
    dtype = DTYPES[kind]
    used = total = 0
    for N in NS:
        x = make_logits(N, A, seed=1000 * A + N, dtype=dtype)
        for stride in (0, A + 3):
            used += run_case(x, dtype, stride, 1.0, f"{kind} N={N} A={A} stride={stride or A}")
            total += N
    print(f"{kind} A={A}: {used} of {total} rows used the neighbour allowance")


@pytest.mark.parametrize("A", (1024, 4096))
def test_long_rows_with_six_finite_entries(A):
    for kind, dtype in DTYPES.items():
        x = sparse_logits(65, A, seed=A, dtype=dtype)
        run_case(x, dtype, 0, 1.0, f"{kind} sparse A={A}")


@pytest.mark.parametrize("t", (0.5, 2.0))
def test_inverse_temperature(t):
    for A, stride in ((21, 0), (21, 24), (130, 0)):
        x = make_logits(257, A, seed=int(10 * t) + A, dtype=torch.float32)
        run_case(x, torch.float32, stride, t, f"t={t} A={A} stride={stride or A}")
    x = make_logits(257, 21, seed=5, dtype=torch.bfloat16)
    run_case(x, torch.bfloat16, 0, t, f"t={t} bf16 A=21")


def test_logits_at_the_end_of_their_allocation(tail_buffer):
    """The last logit is the last element of the allocation, for both kernel forms and a span that does not end on a
    16-byte vector."""
    for kind, dtype in DTYPES.items():
        for N, A in ((4099, 21), (65, 5), (63, 64), (257, 65)):
            x = make_logits(N, A, seed=N + A, dtype=dtype)
            size = N * A * (4 if dtype == torch.float32 else 2)
            dev = tail_buffer[tail_buffer.numel() - size:].view(dtype).view(N, A)
            dev.copy_(torch.from_numpy(x).to(dtype))
            run_case(x, dtype, 0, 1.0, f"tail {kind} N={N} A={A}", dev=dev)


def test_unaligned_base_takes_the_scalar_loads():
    """A base address that is 4-aligned but not 16-aligned: the lane-per-row kernels fall back to element loads / stores."""
    for kind, dtype in DTYPES.items():
        N, A = 300, 21
        x = make_logits(N, A, seed=77, dtype=dtype)
        flat = torch.empty(N * A + 8, dtype=dtype, device="cuda")
        dev = flat[1 if dtype == torch.float32 else 2:][:N * A].view(N, A)
        assert dev.data_ptr() % 16 == 4
        dev.copy_(torch.from_numpy(x).to(dtype))
        run_case(x, dtype, 0, 1.0, f"unaligned {kind}", dev=dev)


def test_repeatable_and_step_dependent_and_routed():
    for N, A in ((4099, 21), (1000, 130)):
        x = make_logits(N, A, seed=3, dtype=torch.float32)
        dev = on_device(x, torch.float32)

        def draw(step, rows=None, logits=dev, into=None):
            act = torch.full((N,), -1, dtype=torch.int32, device="cuda") if into is None else into[0]
            lp = torch.full((N,), 9.0, device="cuda") if into is None else into[1]
            ent = torch.full((N,), 9.0, device="cuda") if into is None else into[2]
            sa.sample_actions(logits, act, SEED, step, rows, 1.0, False, lp, ent)
            return act, lp, ent

        one, two = draw(STEP), draw(STEP)
        assert all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(one, two))     # identical bits
        other = draw(STEP + 1)
        assert (one[0] != other[0]).float().mean() > 0.3
        # rows routed to two policies, written into one joint tensor: bit for bit the single call
        perm = torch.from_numpy(np.random.default_rng(1).permutation(N)).cuda()
        rows_a, rows_b = perm[:N // 3].sort().values, perm[N // 3:].sort().values
        joint = draw(STEP, rows_a, dev[rows_a].contiguous())
        joint = draw(STEP, rows_b, dev[rows_b].contiguous(), into=joint)
        assert all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(one, joint))
        check_sampled(x[rows_a.cpu().numpy()], 1.0, joint[0][rows_a].cpu().numpy(), rows_a.cpu().numpy(), SEED, STEP, f"routed A={A}")


def test_histogram_of_one_row_on_the_device():
    n = 65536
    l = np.array([0.3, -np.inf, 1.7, -0.9, 0.0], np.float32)
    act = torch.empty(n, dtype=torch.int32, device="cuda")
    sa.sample_actions(torch.from_numpy(np.broadcast_to(l, (n, 5)).copy()).cuda(), act, 2, 0)
    p = np.exp(l.astype(np.float64))
    p /= p.sum()
    counts = np.bincount(act.cpu().numpy(), minlength=5)
    assert counts[1] == 0 and (np.abs(counts - n * p) <= 5 * np.sqrt(n * p * (1 - p))).all(), (counts, n * p)


@pytest.mark.parametrize("A", (21, 130))
def test_bad_rows_are_counted(A):
    N = 300
    x = make_logits(N, A, seed=9, dtype=torch.float32)
    x[5] = -np.inf
    x[64, A // 2] = np.nan
    x[129, A - 1] = np.inf
    x[299] = np.nan
    bad_idx = [5, 64, 129, 299]
    dev = on_device(x, torch.float32)
    act = torch.full((N,), -1, dtype=torch.int32, device="cuda")
    lp, ent = torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    for greedy in (False, True):
        bad.zero_()
        sa.sample_actions(dev, act, 1, 1, None, 1.0, greedy, lp, ent, bad)
        assert int(bad.item()) == 4
        assert act[bad_idx].tolist() == [0, 0, 0, 0] and torch.isnan(lp[bad_idx]).all() and torch.isnan(ent[bad_idx]).all()
        good = np.setdiff1d(np.arange(N), bad_idx)
        assert torch.isfinite(lp[good]).all() and torch.isfinite(ent[good]).all()
    # an action outside [0, A) is counted too
    acts = torch.zeros(N, dtype=torch.int32, device="cuda")
    acts[7], acts[200] = A, -1
    bad.zero_()
    lp2, ent2, lse = sa.action_logprob(dev, acts, bad_rows=bad)
    assert int(bad.item()) == 6
    for i in bad_idx + [7, 200]:
        assert torch.isnan(lp2[i]) and torch.isnan(ent2[i]) and torch.isnan(lse[i])
    assert torch.isfinite(lse[np.setdiff1d(np.arange(N), bad_idx + [7, 200])]).all()
    # the sampler object raises
    s = sa.ActionSampler(N, A, seed=1)
    s.sample(dev)
    with pytest.raises(RuntimeError, match="4 rows"):
        s.check()
    s.check()


def test_autograd_function_on_the_device():
    N, A = 513, 21
    x = make_logits(N, A, seed=4, dtype=torch.float32)
    act = torch.from_numpy(sa.sample_host(x, 0, 0)[0].astype(np.int64)).cuda()
    for dtype in (torch.float32, torch.bfloat16):
        xv = torch.from_numpy(x).to(dtype)
        a = xv.cuda().requires_grad_(True)
        lp, ent = sa.action_logprob_entropy(a.view(27, 19, A), act.view(27, 19), inv_temperature=0.5)
        assert lp.shape == (27, 19) and lp.dtype == torch.float32
        w = torch.linspace(-1.0, 2.0, N, device="cuda").view(27, 19)
        (lp * w - 0.3 * ent).sum().backward()
        assert a.grad.dtype == dtype and a.grad.shape == (N, A)
        b = xv.double().requires_grad_(True)
        lp_c, ent_c = sa.action_logprob_entropy(b, act.cpu(), inv_temperature=0.5)
        (lp_c * w.cpu().view(-1).double() - 0.3 * ent_c).sum().backward()
        _, _, _, D, zmax = row_terms(xv.float().numpy(), 0.5)
        assert ((lp.detach().view(-1).cpu().double() - lp_c.detach()).abs().numpy() <= 2 * U * (A + 16 + 4 * (zmax + D))).all()
        tol = 2 * U * 0.5 * (A + 16 + D) * (np.abs(w.cpu().view(-1).numpy()) + 0.3 * (1 + D + 2 * np.log(A)))
        want = b.grad.numpy()
        tol = tol[:, None] + (2.0 ** -8 * np.abs(want) if dtype == torch.bfloat16 else 0.0)
        assert (np.abs(a.grad.float().cpu().numpy() - want) <= tol).all()


def test_sampler_drives_the_env_like_the_host_actions():
    prog = compile_spec(presets.rung1_spec(), 16, 16)
    pool = np.stack([prog.class_map(presets.rung1_map())])
    E = 6
    env = MettaGridBatchedEnv(prog, E, map_pool=pool, seed=5)
    twin = MettaGridBatchedEnv(prog, E, map_pool=pool, seed=5)
    try:
        env.reset()
        twin.reset()
        s = env.action_sampler(seed=3)
        n = E * prog.num_agents
        assert s.actions.shape == env.engine.actions.shape and s.actions.dtype == torch.int32 and s.n_actions == env.transport_action_n
        rng = np.random.default_rng(2)
        for k in range(8):
            logits = (3.0 * rng.standard_normal((n, env.transport_action_n))).astype(np.float32)
            obs, rew, *_ = env.step(s.sample(torch.from_numpy(logits).cuda())[0])
            want = sa.sample_host(logits, 3, k)[0]
            obs_t, rew_t, *_ = twin.step(torch.from_numpy(want).cuda())
            assert np.array_equal(s.actions.cpu().numpy(), want), k      # (A = 5: a boundary within delta of u is a 1e-5 event)
            assert torch.equal(obs, obs_t) and torch.equal(rew, rew_t), k
        env.check_actions()
        s.check()
        assert s.state_dict() == {"seed": 3, "step": 8}
    finally:
        env.close()
        twin.close()
