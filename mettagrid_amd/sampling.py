"""Policy output side: sampled actions, their log-probabilities and the entropy straight from the logits.

Every reference policy ends in ``Categorical(logits=logits).sample()`` or pufferlib's ``sample_logits(logits)``
(python/src/mettagrid/policy/lstm.py:232, stateless.py:98, token_encoder.py:149, puffer_default.py:107, pufferlib.py:73), and a
trainer re-evaluates ``log_prob(actions)`` and ``entropy()`` of the same logits with a gradient.  The kernels
(csrc/mgx_sample.hip) read the logits once per call; the draws come from a counter-based generator, so a rollout can be
replayed and does not change when the rows are routed to several policies.

    z_a = fl32(t * l_a)    m = max z    pt_a = exp(z_a - m)    S = sum pt_a    logp_a = z_a - m - log S
    H = log S - (sum_{pt_a > 0} pt_a (z_a - m)) / S            lse = m + log S
    u = (x0 >> 8) * 2**-24,  x0 = Philox4x32-10(counter = (r lo, r hi, step lo, step hi), key = (seed lo, seed hi))[0]
    sampled action = the smallest a with c_a > u * c_{A-1}, c the running sum of pt in index order (the last a with
    pt_a > 0 if rounding leaves none); greedy = the lowest index among the maxima of z
    d_logits[a] = t * (d_logprob * ([a = act] - p_a) - d_entropy * p_a * (logp_a + H)),  exactly 0 where l_a = -inf

A row with no finite entry, or with a NaN or ``+inf``, is bad: action 0, NaN ``logprob`` / ``entropy``, counted in ``bad_rows``.
``philox4x32`` / ``uniforms`` / ``sample_host`` / ``logprob_entropy_host`` / ``logprob_entropy_grad_host`` restate all of it in
numpy float64 on the kernels' operands (bfloat16 logits at their exact values, ``z`` rounded to float32 as the kernels form
it); ``sample_actions`` / ``action_logprob`` / ``action_logprob_backward`` are the raw ops on torch's current stream;
``action_logprob_entropy`` is the differentiable form and ``ActionSampler`` the rollout-side object that owns the joint action
tensor ``MettaGridBatchedEnv.step`` takes.  Importable without a GPU; CPU tensors take a float64 path of the same definition."""
from __future__ import annotations

import numpy as np

MAX_ACTIONS = 4096      # include/mgx.h mgx_sample_actions: 1 <= n_actions <= 4096
MAX_ROWS = 1 << 25      # 0 <= n_rows <= 2**25
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK32 = (1 << 64) - 1


def philox4x32(counter, key) -> np.ndarray:
    """Philox4x32-10 (Salmon et al., SC'11): ``counter`` uint32 [..., 4] and ``key`` uint32 [..., 2] (broadcast against each
    other) -> uint32 [..., 4]."""
    c = np.asarray(counter, dtype=np.uint32)
    k = np.asarray(key, dtype=np.uint32)
    if c.shape[-1] != 4 or k.shape[-1] != 2:
        raise ValueError("philox4x32: counter [..., 4], key [..., 2]")
    lead = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c = np.broadcast_to(c, lead + (4,)).astype(np.uint64)
    k = np.broadcast_to(k, lead + (2,)).astype(np.uint64)
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    lo32, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2          # 32 x 32 -> 64 bits, exact in uint64
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & lo32, (p0 >> s32) ^ c3 ^ k1, p0 & lo32
        k0, k1 = (k0 + np.uint64(_W0)) & lo32, (k1 + np.uint64(_W1)) & lo32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def uniforms(seed: int, step: int, rows) -> np.ndarray:
    """float64 [n]: the kernel's ``u`` in [0, 1) of the output rows ``rows`` (global row indices) at ``(seed, step)``."""
    r = np.asarray(rows, dtype=np.int64).reshape(-1).astype(np.uint64)
    seed, step = int(seed) & _MASK32, int(step) & _MASK32
    ctr = np.empty((r.size, 4), np.uint32)
    ctr[:, 0] = (r & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    ctr[:, 1] = (r >> np.uint64(32)).astype(np.uint32)
    ctr[:, 2] = step & 0xFFFFFFFF
    ctr[:, 3] = step >> 32
    x0 = philox4x32(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint32))[:, 0]
    return (x0 >> np.uint32(8)).astype(np.float64) * 2.0 ** -24


def _z64(logits, inv_temperature: float) -> np.ndarray:
    """float64 [N, A]: ``fl32(t * l)`` of float32 / bfloat16 logits (torch or numpy), the kernels' ``z``."""
    try:
        import torch
        if isinstance(logits, torch.Tensor):
            logits = logits.detach().cpu().to(torch.float32).numpy()
    except ImportError:
        pass
    l32 = np.asarray(logits, dtype=np.float32)
    if l32.ndim != 2 or l32.shape[1] < 1:
        raise ValueError("logits: [N, A] with A >= 1")
    t = np.float32(inv_temperature)
    if not (t > 0 and np.isfinite(t)):
        raise ValueError("inv_temperature must be positive and finite")
    with np.errstate(invalid="ignore", over="ignore"):
        return (l32 * t).astype(np.float32).astype(np.float64)


def _row_stats(z: np.ndarray):
    """(bad [N], m [N], pt [N, A], S [N], H [N]) in float64; bad rows hold NaN."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        bad = ~np.isfinite(z).any(1) | np.isnan(z).any(1) | (z == np.inf).any(1)
        zz = np.where(bad[:, None], 0.0, z)
        m = zz.max(1)
        d = zz - m[:, None]
        pt = np.exp(d)
        S = pt.sum(1)
        T = np.where(pt > 0, pt * np.where(pt > 0, d, 0.0), 0.0).sum(1)
        H = np.log(S) - T / S
    nan = np.where(bad, np.nan, 0.0)
    return bad, m + nan, pt, S + nan, H + nan


def sample_host(logits, seed: int, step: int, rows=None, inv_temperature: float = 1.0, greedy: bool = False):
    """``(actions int32 [N], logprob float64 [N], entropy float64 [N])`` of ``logits`` [N, A], entry ``i`` drawn with the
    counter of global row ``rows[i]`` (None: ``i``) — what ``mgx_sample_actions`` writes at ``rows[i]``."""
    z = _z64(logits, inv_temperature)
    N, A = z.shape
    r = np.arange(N, dtype=np.int64) if rows is None else np.asarray(_to_numpy(rows), dtype=np.int64).reshape(-1)
    if r.size != N:
        raise ValueError(f"rows: {r.size} indices for {N} rows of logits")
    bad, m, pt, S, H = _row_stats(z)
    if greedy:
        act = np.where(bad, 0, np.argmax(np.where(bad[:, None], 0.0, z), axis=1))   # (argmax: the first of equal maxima)
    else:
        c = np.cumsum(pt, axis=1)
        thr = uniforms(seed, step, r) * c[:, -1]
        over = c > thr[:, None]
        first = np.argmax(over, axis=1)
        last_pos = A - 1 - np.argmax(pt[:, ::-1] > 0, axis=1)
        act = np.where(bad, 0, np.where(over.any(1), first, last_pos))
    act = act.astype(np.int32)
    with np.errstate(invalid="ignore", divide="ignore"):
        lp = z[np.arange(N), act] - (m + np.log(S))
    return act, np.where(bad, np.nan, lp), H


def logprob_entropy_host(logits, actions, inv_temperature: float = 1.0):
    """``(logprob, entropy, lse)`` float64 [N] of ``actions`` [N] under ``logits`` [N, A]; NaN for a bad row or an action
    outside [0, A)."""
    z = _z64(logits, inv_temperature)
    N, A = z.shape
    act = np.asarray(_to_numpy(actions), dtype=np.int64).reshape(-1)
    if act.size != N:
        raise ValueError(f"actions: {act.size} entries for {N} rows of logits")
    bad, m, _, S, H = _row_stats(z)
    out = (act < 0) | (act >= A)
    bad = bad | out
    with np.errstate(invalid="ignore", divide="ignore"):
        lse = m + np.log(S)
        lp = z[np.arange(N), np.where(out, 0, act)] - lse
    nan = np.where(bad, np.nan, 0.0)
    return lp + nan, H + nan, lse + nan


def logprob_entropy_grad_host(logits, actions, d_logprob=None, d_entropy=None, inv_temperature: float = 1.0) -> np.ndarray:
    """float64 [N, A]: the gradient of ``sum(d_logprob * logprob + d_entropy * entropy)`` with respect to the logits
    (None = zeros); exactly 0 at masked entries."""
    z = _z64(logits, inv_temperature)
    N, A = z.shape
    act = np.asarray(_to_numpy(actions), dtype=np.int64).reshape(-1)
    lp_a, H, lse = logprob_entropy_host(logits, actions, inv_temperature)
    dlp = np.zeros(N) if d_logprob is None else np.asarray(_to_numpy(d_logprob), dtype=np.float64).reshape(-1)
    dH = np.zeros(N) if d_entropy is None else np.asarray(_to_numpy(d_entropy), dtype=np.float64).reshape(-1)
    t = float(np.float32(inv_temperature))
    masked = z == -np.inf
    with np.errstate(invalid="ignore", over="ignore"):
        logp = np.where(masked, 0.0, z - lse[:, None])
        p = np.where(masked, 0.0, np.exp(logp))
        onehot = (np.arange(A)[None, :] == act[:, None]).astype(np.float64)
        g = t * (dlp[:, None] * (onehot - p) - dH[:, None] * p * (logp + H[:, None]))
    return np.where(masked, 0.0, g)


def _to_numpy(a):
    try:
        import torch
        if isinstance(a, torch.Tensor):
            return a.detach().cpu().numpy()
    except ImportError:
        pass
    return a


def _lib():
    from .engine import load_lib
    return load_lib()


def _check_t(t) -> float:
    t = float(t)
    if not (t > 0.0 and np.isfinite(np.float32(t))):
        raise ValueError(f"inv_temperature = {t}: must be positive and finite")
    return t


def _check_logits(logits, what: str):
    import torch
    if (not isinstance(logits, torch.Tensor) or logits.dtype not in (torch.float32, torch.bfloat16) or logits.dim() != 2
            or not logits.is_cuda):
        raise ValueError(f"{what}: logits must be a float32 or bfloat16 [N, A] device tensor")
    N, A = int(logits.shape[0]), int(logits.shape[1])
    if not 1 <= A <= MAX_ACTIONS:
        raise ValueError(f"{what}: A = {A} actions, must be in [1, {MAX_ACTIONS}]")
    if N > MAX_ROWS:
        raise ValueError(f"{what}: N = {N} rows, at most {MAX_ROWS} per call")
    if (A > 1 and logits.stride(1) != 1) or (N > 1 and logits.stride(0) < A):
        raise ValueError(f"{what}: logits need unit stride along the actions and a row stride >= A")
    return N, A, (int(logits.stride(0)) if N > 1 else A)


def _check_vec(t, name: str, what: str, dtype, n: int, device, optional: bool = False):
    import torch
    if t is None and optional:
        return None
    if (not isinstance(t, torch.Tensor) or t.dtype != dtype or t.dim() != 1 or t.device != device or not t.is_contiguous()
            or (n is not None and t.numel() != n)):
        raise ValueError(f"{what}: {name} must be a contiguous {dtype} [{'n' if n is None else n}] tensor on the logits' device")
    return t


def _ptr(t):
    return None if t is None else t.data_ptr()


def _code(dtype) -> int:
    import torch
    return 1 if dtype == torch.float32 else 2


def sample_actions(logits, actions, seed: int, step: int, rows=None, inv_temperature: float = 1.0, greedy: bool = False,
                   logprob=None, entropy=None, bad_rows=None):
    """``mgx_sample_actions`` on torch's current stream.  ``logits`` float32 / bfloat16 [N, A] (unit stride along A, row stride
    >= A); ``actions`` int32 [R], ``logprob`` / ``entropy`` float32 [R] or None, ``bad_rows`` int32 [1] or None: the joint
    outputs, entry ``rows[i]`` (``rows`` int64 [N] on the device, None: ``i``, then R >= N) written for logits row ``i``.  The
    caller keeps ``rows`` inside [0, R): the kernel does not check.  ValueError for whatever the kernel refuses."""
    import torch
    N, A, stride = _check_logits(logits, "sample_actions")
    t = _check_t(inv_temperature)
    dev = logits.device
    _check_vec(actions, "actions", "sample_actions", torch.int32, None, dev)
    R = int(actions.numel())
    _check_vec(logprob, "logprob", "sample_actions", torch.float32, R, dev, True)
    _check_vec(entropy, "entropy", "sample_actions", torch.float32, R, dev, True)
    _check_vec(bad_rows, "bad_rows", "sample_actions", torch.int32, 1, dev, True)
    if rows is None:
        if R < N:
            raise ValueError(f"sample_actions: {N} rows of logits, room for {R} actions")
    else:
        _check_vec(rows, "rows", "sample_actions", torch.int64, N, dev)
    if N == 0:
        return actions
    with torch.cuda.device(dev):
        rc = _lib().mgx_sample_actions(logits.data_ptr(), _code(logits.dtype), N, A, stride, _ptr(rows), t, 1 if greedy else 0,
                                       int(seed) & _MASK32, int(step) & _MASK32, actions.data_ptr(), _ptr(logprob), _ptr(entropy),
                                       _ptr(bad_rows), torch.cuda.current_stream().cuda_stream)
    if rc == -1:
        raise ValueError("mgx_sample_actions refused its arguments")
    if rc:
        raise RuntimeError(f"mgx_sample_actions failed ({rc})")
    return actions


def action_logprob(logits, actions, inv_temperature: float = 1.0, entropy: bool = True, lse: bool = True, bad_rows=None):
    """``mgx_action_logprob`` on torch's current stream: ``(logprob, entropy, lse)`` float32 [N] (None where not asked for) of
    ``actions`` int32 [N] under ``logits`` [N, A]."""
    import torch
    N, A, stride = _check_logits(logits, "action_logprob")
    t = _check_t(inv_temperature)
    dev = logits.device
    _check_vec(actions, "actions", "action_logprob", torch.int32, N, dev)
    _check_vec(bad_rows, "bad_rows", "action_logprob", torch.int32, 1, dev, True)
    lp = torch.empty(N, dtype=torch.float32, device=dev)
    ent = torch.empty(N, dtype=torch.float32, device=dev) if entropy else None
    ls = torch.empty(N, dtype=torch.float32, device=dev) if lse else None
    if N == 0:
        return lp, ent, ls
    with torch.cuda.device(dev):
        rc = _lib().mgx_action_logprob(logits.data_ptr(), _code(logits.dtype), N, A, stride, actions.data_ptr(), t, lp.data_ptr(), _ptr(ent),
                                       _ptr(ls), _ptr(bad_rows), torch.cuda.current_stream().cuda_stream)
    if rc == -1:
        raise ValueError("mgx_action_logprob refused its arguments")
    if rc:
        raise RuntimeError(f"mgx_action_logprob failed ({rc})")
    return lp, ent, ls


def action_logprob_backward(logits, actions, lse, d_logprob=None, d_entropy=None, inv_temperature: float = 1.0, out=None, out_dtype=None):
    """``mgx_action_logprob_backward`` on torch's current stream: ``d_logits`` [N, A] in ``out_dtype`` (default: the logits'),
    or written into ``out`` (unit stride along A, row stride >= A).  ``d_logprob`` / ``d_entropy`` float32 [N] or None = zeros."""
    import torch
    N, A, stride = _check_logits(logits, "action_logprob_backward")
    t = _check_t(inv_temperature)
    dev = logits.device
    _check_vec(actions, "actions", "action_logprob_backward", torch.int32, N, dev)
    _check_vec(lse, "lse", "action_logprob_backward", torch.float32, N, dev)
    _check_vec(d_logprob, "d_logprob", "action_logprob_backward", torch.float32, N, dev, True)
    _check_vec(d_entropy, "d_entropy", "action_logprob_backward", torch.float32, N, dev, True)
    if out is None:
        out_dtype = logits.dtype if out_dtype is None else out_dtype
        if out_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("action_logprob_backward: out_dtype must be torch.float32 or torch.bfloat16")
        out = torch.empty((N, A), dtype=out_dtype, device=dev)
    elif (not isinstance(out, torch.Tensor) or out.dtype not in (torch.float32, torch.bfloat16) or tuple(out.shape) != (N, A)
          or out.device != dev or (A > 1 and out.stride(1) != 1) or (N > 1 and out.stride(0) < A)):
        raise ValueError("action_logprob_backward: out must be a float32 or bfloat16 [N, A] tensor on the logits' device with unit stride along A")
    if N == 0:
        return out
    with torch.cuda.device(dev):
        rc = _lib().mgx_action_logprob_backward(logits.data_ptr(), _code(logits.dtype), N, A, stride, actions.data_ptr(), t, lse.data_ptr(),
                                                _ptr(d_logprob), _ptr(d_entropy), out.data_ptr(), _code(out.dtype),
                                                int(out.stride(0)) if N > 1 else A, torch.cuda.current_stream().cuda_stream)
    if rc == -1:
        raise ValueError("mgx_action_logprob_backward refused its arguments")
    if rc:
        raise RuntimeError(f"mgx_action_logprob_backward failed ({rc})")
    return out


def _z_torch(logits, t: float):
    import torch
    return (logits.detach().to(torch.float32) * torch.tensor(t, dtype=torch.float32)).to(torch.float64)


def _function():
    import torch

    class ActionLogProb(torch.autograd.Function):
        """``(logits [N, A], actions [N], inv_temperature) -> (logprob [N], entropy [N])`` with a gradient for ``logits`` only,
        in the logits' dtype.  Device tensors: the two kernels, with the logits, the actions and ``lse`` [N] kept for backward
        (nothing of size [N, A] beyond the input itself).  CPU tensors: the same definition in torch float64."""

        @staticmethod
        def forward(ctx, logits, actions, inv_temperature):
            t = _check_t(inv_temperature)
            ctx.t = t
            if logits.is_cuda:
                act = actions.to(torch.int32).contiguous()
                lp, ent, lse = action_logprob(logits, act, t)
                ctx.save_for_backward(logits, act, lse)
                return lp, ent
            if logits.dim() != 2 or not 1 <= logits.shape[1] <= MAX_ACTIONS:
                raise ValueError(f"action_logprob_entropy: logits must be [N, A] with 1 <= A <= {MAX_ACTIONS}")
            out_dtype = torch.float64 if logits.dtype == torch.float64 else torch.float32
            z = (logits.detach() * t) if logits.dtype == torch.float64 else _z_torch(logits, t)
            A = z.shape[1]
            act = actions.to(torch.int64)
            bad = ~torch.isfinite(z).any(1) | torch.isnan(z).any(1) | (z == float("inf")).any(1) | (act < 0) | (act >= A)
            zz = torch.where(bad[:, None], torch.zeros_like(z), z)
            m = zz.max(1).values
            d = zz - m[:, None]
            pt = d.exp()
            S = pt.sum(1)
            T = torch.where(pt > 0, pt * torch.where(pt > 0, d, torch.zeros_like(d)), torch.zeros_like(d)).sum(1)
            nan = torch.where(bad, torch.full_like(S, float("nan")), torch.zeros_like(S))
            lse = m + S.log() + nan
            H = S.log() - T / S + nan
            lp = zz.gather(1, act.clamp(0, A - 1)[:, None])[:, 0] - lse
            ctx.save_for_backward(logits, act, lse)
            ctx.H = H
            return lp.to(out_dtype), H.to(out_dtype)

        @staticmethod
        def backward(ctx, d_lp, d_ent):
            logits, act, lse = ctx.saved_tensors
            if not ctx.needs_input_grad[0]:
                return None, None, None
            t = ctx.t
            if logits.is_cuda:
                g = action_logprob_backward(logits, act, lse, None if d_lp is None else d_lp.to(torch.float32).contiguous(),
                                            None if d_ent is None else d_ent.to(torch.float32).contiguous(), t)
                return g, None, None
            z = (logits.detach() * t) if logits.dtype == torch.float64 else _z_torch(logits, t)
            masked = z == float("-inf")
            zero = torch.zeros_like(z)
            logp = torch.where(masked, zero, z - lse[:, None])
            p = torch.where(masked, zero, logp.exp())
            onehot = (torch.arange(z.shape[1])[None, :] == act[:, None]).to(z.dtype)
            dlp = torch.zeros_like(lse) if d_lp is None else d_lp.to(z.dtype)
            dH = torch.zeros_like(lse) if d_ent is None else d_ent.to(z.dtype)
            tt = t if logits.dtype == torch.float64 else float(np.float32(t))
            g = tt * (dlp[:, None] * (onehot - p) - dH[:, None] * p * (logp + ctx.H[:, None]))
            return torch.where(masked, zero, g).to(logits.dtype), None, None

    return ActionLogProb


_FN = None


def _fn():
    global _FN
    if _FN is None:
        _FN = _function()
    return _FN


def __getattr__(name):   # ActionLogProb is built on first use: torch is imported then, not with the module
    if name == "ActionLogProb":
        return _fn()
    raise AttributeError(name)


def action_logprob_entropy(logits, actions, inv_temperature: float = 1.0):
    """``(logprob, entropy)`` of ``actions`` [...] under ``logits`` [..., A], differentiable with respect to the logits
    (``ActionLogProb``): what ``Categorical(logits=logits * inv_temperature)`` gives for ``log_prob(actions)`` and
    ``entropy()``, in one read of the logits forward and one backward."""
    A = logits.shape[-1]
    lead = logits.shape[:-1]
    if tuple(actions.shape) != tuple(lead):
        raise ValueError(f"action_logprob_entropy: actions have shape {tuple(actions.shape)}, logits {tuple(logits.shape)}")
    l2 = logits.reshape(-1, A)
    if l2.is_cuda and l2.shape[0] > 1 and A > 1 and l2.stride(1) != 1:
        l2 = l2.contiguous()
    lp, ent = _fn().apply(l2, actions.reshape(-1), float(inv_temperature))
    return lp.reshape(lead), ent.reshape(lead)


class ActionSampler:
    """The rollout side: owns the joint ``actions`` int32 [n_rows] (what ``MettaGridBatchedEnv.step`` takes on its one-kernel
    path), ``logprob`` / ``entropy`` float32 [n_rows], the ``bad_rows`` counter and a host-side ``step`` counter.

    ``sample(logits, rows=None, greedy=False, advance=True)`` fills the tensors in place — all rows, or the rows ``rows`` (int64
    device tensor, e.g. ``env.policy_rows(p)``) from ``logits [len(rows), A]`` — with the draws of step ``step`` and returns
    ``(actions, logprob, entropy)``.  ``advance=True`` (the first policy of an env step) begins a new step; the second and later
    policies of the same step pass ``advance=False`` and draw from the same step's counters, so the joint result does not depend
    on how the rows are split.  ``check()`` reads ``bad_rows`` (a device synchronisation) and raises.  ``state_dict()`` carries
    ``(seed, step)``: a restored sampler continues the same stream of draws.  On the CPU the tensors are filled by
    ``sample_host``."""

    def __init__(self, n_rows: int, n_actions: int, seed: int = 0, device="cuda") -> None:
        import torch
        n_rows, n_actions = int(n_rows), int(n_actions)
        if n_rows < 1 or n_rows > MAX_ROWS or not 1 <= n_actions <= MAX_ACTIONS:
            raise ValueError(f"ActionSampler: n_rows in [1, {MAX_ROWS}] and n_actions in [1, {MAX_ACTIONS}], got {n_rows}, {n_actions}")
        self.n_rows, self.n_actions = n_rows, n_actions
        self.seed = int(seed) & _MASK32
        self.step = 0            # env steps begun so far; the draws of the current step use the counter step - 1
        self.actions = torch.zeros(n_rows, dtype=torch.int32, device=torch.device(device))
        self.device = self.actions.device    # ("cuda" -> the current device's ordinal)
        self.logprob = torch.zeros(n_rows, dtype=torch.float32, device=self.device)
        self.entropy = torch.zeros(n_rows, dtype=torch.float32, device=self.device)
        self.bad_rows = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._rows_ok = None     # (data_ptr, version, numel) of the last rows tensor whose range was checked

    def _check_rows(self, rows, n: int):
        import torch
        if not isinstance(rows, torch.Tensor) or rows.dtype != torch.int64 or rows.dim() != 1 or rows.numel() != n or rows.device != self.device:
            raise ValueError(f"ActionSampler.sample: rows must be an int64 [{n}] tensor on {self.device}, one index per row of logits")
        rows = rows.contiguous()
        key = (rows.data_ptr(), rows._version, rows.numel())
        if key != self._rows_ok and n:    # the kernel trusts the indices: read their range once per list
            lo, hi = int(rows.min()), int(rows.max())
            if lo < 0 or hi >= self.n_rows:
                raise ValueError(f"ActionSampler.sample: rows outside [0, {self.n_rows}): min {lo}, max {hi}")
            self._rows_ok = key
        return rows

    def sample(self, logits, rows=None, greedy: bool = False, advance: bool = True, inv_temperature: float = 1.0):
        import torch
        if not isinstance(logits, torch.Tensor) or logits.dim() != 2 or logits.shape[1] != self.n_actions or logits.device != self.device:
            raise ValueError(f"ActionSampler.sample: logits must be [n, {self.n_actions}] on {self.device}")
        n = int(logits.shape[0])
        if rows is None:
            if n != self.n_rows:
                raise ValueError(f"ActionSampler.sample: {n} rows of logits for {self.n_rows} rows (pass rows=...)")
        else:
            rows = self._check_rows(rows, n)
        if not advance and self.step == 0:
            raise ValueError("ActionSampler.sample: advance=False before the first step")
        if advance:
            self.step += 1
        s = self.step - 1
        if self.device.type == "cuda":
            sample_actions(logits, self.actions, self.seed, s, rows, inv_temperature, greedy, self.logprob, self.entropy, self.bad_rows)
        else:
            idx = np.arange(n) if rows is None else rows.numpy()
            act, lp, ent = sample_host(logits, self.seed, s, idx, inv_temperature, greedy)
            sel = slice(None) if rows is None else rows
            self.actions[sel] = torch.from_numpy(act)
            self.logprob[sel] = torch.from_numpy(lp).to(torch.float32)
            self.entropy[sel] = torch.from_numpy(ent).to(torch.float32)
            self.bad_rows += int(np.isnan(lp).sum())
        return self.actions, self.logprob, self.entropy

    def check(self) -> None:
        """Raise if a sampled row was bad (no finite logit, a NaN or ``+inf``) since the last check; synchronises."""
        n = int(self.bad_rows.item())
        if n:
            self.bad_rows.zero_()
            raise RuntimeError(f"ActionSampler: {n} rows of logits had no finite entry, a NaN or +inf (action 0 was played)")

    def state_dict(self) -> dict:
        return {"seed": int(self.seed), "step": int(self.step)}

    def load_state_dict(self, state: dict) -> None:
        seed, step = int(state["seed"]), int(state["step"])
        if step < 0:
            raise ValueError("ActionSampler.load_state_dict: step < 0")
        self.seed, self.step = seed & _MASK32, step
