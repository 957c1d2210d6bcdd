"""Dense-policy front end: the first ``Linear`` of the reference's trainable baselines, read straight from
the u8 observation rows.

The reference nets flatten a row and scale it (python/src/mettagrid/policy/stateless.py:29,42 and lstm.py:31-37,73-84:
``observations.view(B, -1).float() / 255.0``; puffer_default.py:57,65: ``.float() * (1.0 / 255.0)``) and feed the result to
``Linear(3T, hidden)``.  Every u8 value is exact in bfloat16, so the kernels (csrc/mgx_byte_linear.hip) take the row itself
as a matrix-core operand: no float copy of the observations is made and the input is never rounded.

    y[n][h]  = fl( fl( s * sum_k x[n][k] * W[h][k] ) + b[h] )      x u8 [N, K], W [H, K] (torch's Linear layout), s the scale
    dW[h][k] = s * sum_n dy[n][h] * x[n][k]                         (no gradient for x: it is data)

``W`` reaches the kernels as bfloat16: one term (``precision="bf16"``: ``w_hi = bf16(W)``) or two (``"bf16x2"``:
``w_hi + w_lo``, ``|W - w_hi - w_lo| <= 2**-16 |W|``, a near drop-in for a float32 layer).  The weight gradient treats ``dy`` the
same way.  ``split_bf16`` / ``byte_linear_host`` / ``byte_linear_wgrad_host`` restate both in numpy float64 on exactly the
kernels' operands; ``byte_linear`` / ``byte_linear_wgrad`` are the raw ops on torch's current stream; ``ByteRowLinear`` is the
layer, with ``nn.Linear``'s parameter names, shapes and init.  Importable without a GPU; CPU tensors take a torch path of
the same definition."""
from __future__ import annotations

import math

import numpy as np

MAX_K = 65535        # include/mgx.h mgx_byte_linear_forward: 1 <= K <= 65535
MAX_H = 4096         # H a multiple of 16, 16 <= H <= 4096
PRECISIONS = {"bf16": 1, "bf16x2": 2}


def _bf16_round_np(a: np.ndarray) -> np.ndarray:
    """float32 array -> float32 array of the nearest bfloat16 values (ties to even)."""
    bits = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    out = ((bits + np.uint32(0x7FFF) + ((bits >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)).view(np.float32)
    return np.where(np.isfinite(a), out, a).astype(np.float32)


def split_bf16(w):
    """``(hi, lo)`` with ``hi = bf16(w)`` and ``lo = bf16(w - hi)`` (round to nearest even; ``w - hi`` is exact in float32):
    ``|w - hi - lo| <= 2**-16 |w|``.  A torch tensor gives two bfloat16 tensors, anything else two float32 numpy arrays
    holding bfloat16-representable values."""
    try:
        import torch
        if isinstance(w, torch.Tensor):
            w32 = w.detach().to(torch.float32)
            hi = w32.to(torch.bfloat16)
            return hi, (w32 - hi.to(torch.float32)).to(torch.bfloat16)
    except ImportError:
        pass
    w32 = np.asarray(w, dtype=np.float32)
    hi = _bf16_round_np(w32)
    return hi, _bf16_round_np(w32 - hi)


def _as_f64(a) -> np.ndarray:
    try:
        import torch
        if isinstance(a, torch.Tensor):
            return a.detach().cpu().to(torch.float64).numpy()
    except ImportError:
        pass
    return np.asarray(a, dtype=np.float64)


def _rows_2d(x) -> np.ndarray:
    x = np.asarray(x)
    if x.dtype != np.uint8 or x.ndim < 2:
        raise ValueError("x: u8 [N, K] (or [N, T, 3])")
    return x.reshape(x.shape[0], -1)


def byte_linear_host(x, w_hi, w_lo=None, bias=None, scale=1.0 / 255.0) -> np.ndarray:
    """float64 [N, H]: ``float32(scale) * (x @ (w_hi + w_lo).T) + bias`` on the kernel's operands, every step in float64."""
    x2 = _rows_2d(x).astype(np.float64)
    w = _as_f64(w_hi) + (0.0 if w_lo is None else _as_f64(w_lo))
    y = float(np.float32(scale)) * (x2 @ w.T)
    return y if bias is None else y + _as_f64(bias)[None, :]


def dy_terms_host(dy, terms: int) -> np.ndarray:
    """float64: ``dy`` as the weight-gradient kernel uses it: bfloat16 hi + lo for two terms and float32 ``dy``, else
    ``bf16(dy)`` (a bfloat16 ``dy`` is its own value)."""
    d32 = _as_f64(dy).astype(np.float32)
    hi = _bf16_round_np(d32)
    if int(terms) == 2:
        return hi.astype(np.float64) + _bf16_round_np(d32 - hi).astype(np.float64)
    return hi.astype(np.float64)


def byte_linear_wgrad_host(x, dy, scale=1.0 / 255.0, terms: int = 1) -> np.ndarray:
    """float64 [H, K]: ``float32(scale) * dy_terms.T @ x``."""
    x2 = _rows_2d(x).astype(np.float64)
    return float(np.float32(scale)) * (dy_terms_host(dy, terms).T @ x2)


def _check_shape(K: int, H: int) -> None:
    if not 1 <= K <= MAX_K:
        raise ValueError(f"byte_linear: K = {K} input bytes per row, must be in [1, {MAX_K}]")
    if H % 16 or not 16 <= H <= MAX_H:
        raise ValueError(f"byte_linear: H = {H} output features, must be a multiple of 16 in [16, {MAX_H}]")


def _lib():
    from .engine import load_lib
    return load_lib()


def chunk_rows() -> int:
    """Rows per partial tile of the weight-gradient kernel (mgx_byte_linear_chunk_rows)."""
    return int(_lib().mgx_byte_linear_chunk_rows())


def _check_x(x, what: str):
    import torch
    if not isinstance(x, torch.Tensor) or x.dtype != torch.uint8 or x.dim() != 2 or not x.is_cuda:
        raise ValueError(f"{what}: x must be a u8 [N, K] device tensor")
    if (x.shape[1] > 1 and x.stride(1) != 1) or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        raise ValueError(f"{what}: x needs unit stride along K and a row stride >= K")


def byte_linear(x, w_hi, w_lo=None, bias=None, scale: float = 1.0 / 255.0, out=None, out_dtype=None):
    """The forward kernel on torch's current stream: ``x`` u8 [N, K] (unit stride along K, any row stride >= K, any
    alignment), ``w_hi`` / ``w_lo`` bfloat16 [H, K] contiguous, ``bias`` float32 [H] or None; returns ``out`` [N, H], float32
    (default) or bfloat16 (= the float32 result rounded to nearest even), which may be a caller's view with unit stride along
    H and any row stride >= H.  ValueError for anything the kernel does not take."""
    import torch
    _check_x(x, "byte_linear")
    N, K = int(x.shape[0]), int(x.shape[1])
    for name, w in (("w_hi", w_hi), ("w_lo", w_lo)):
        if w is None and name == "w_lo":
            continue
        if not isinstance(w, torch.Tensor) or w.dtype != torch.bfloat16 or w.dim() != 2 or w.device != x.device or not w.is_contiguous():
            raise ValueError(f"byte_linear: {name} must be a contiguous bfloat16 [H, K] tensor on x's device")
        if tuple(w.shape) != tuple(w_hi.shape) or w.shape[1] != K:
            raise ValueError(f"byte_linear: {name} has shape {tuple(w.shape)}, x has K = {K}")
    H = int(w_hi.shape[0])
    _check_shape(K, H)
    if bias is not None and (not isinstance(bias, torch.Tensor) or bias.dtype != torch.float32 or tuple(bias.shape) != (H,)
                             or bias.device != x.device or not bias.is_contiguous()):
        raise ValueError("byte_linear: bias must be a contiguous float32 [H] tensor on x's device")
    if out is None:
        out_dtype = torch.float32 if out_dtype is None else out_dtype
        if out_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("byte_linear: out_dtype must be torch.float32 or torch.bfloat16")
        out = torch.empty((N, H), dtype=out_dtype, device=x.device)
    else:
        if (not isinstance(out, torch.Tensor) or out.dtype not in (torch.float32, torch.bfloat16) or tuple(out.shape) != (N, H)
                or out.device != x.device or out.stride(1) != 1 or (N > 1 and out.stride(0) < H)):
            raise ValueError("byte_linear: out must be a float32 or bfloat16 [N, H] tensor on x's device with unit stride along H")
        if out_dtype is not None and out_dtype != out.dtype:
            raise ValueError("byte_linear: out_dtype differs from out.dtype")
    if N == 0:
        return out
    L = _lib()
    with torch.cuda.device(x.device):
        stream = torch.cuda.current_stream().cuda_stream
        rc = L.mgx_byte_linear_forward(x.data_ptr(), N, K, x.stride(0) if N > 1 else K, w_hi.data_ptr(), None if w_lo is None else w_lo.data_ptr(),
                                       1 if w_lo is None else 2, None if bias is None else bias.data_ptr(), float(scale), out.data_ptr(),
                                       1 if out.dtype == torch.float32 else 2, out.stride(0) if N > 1 else H, H, stream)
    if rc:
        raise RuntimeError(f"mgx_byte_linear_forward failed ({rc})")
    return out


def byte_linear_wgrad(x, dy, scale: float = 1.0 / 255.0, terms: int = 1, scratch=None):
    """The weight-gradient kernels on torch's current stream: ``x`` as for ``byte_linear``, ``dy`` float32 or bfloat16 [N, H]
    contiguous; returns float32 [H, K].  ``scratch``: a device tensor of at least
    ``mgx_byte_linear_scratch_bytes(N, K, H)`` bytes to reuse (allocated otherwise).  Bit-identical from call to call."""
    import torch
    _check_x(x, "byte_linear_wgrad")
    N, K = int(x.shape[0]), int(x.shape[1])
    if (not isinstance(dy, torch.Tensor) or dy.dtype not in (torch.float32, torch.bfloat16) or dy.dim() != 2 or dy.shape[0] != N
            or dy.device != x.device or not dy.is_contiguous()):
        raise ValueError("byte_linear_wgrad: dy must be a contiguous float32 or bfloat16 [N, H] tensor on x's device")
    H = int(dy.shape[1])
    _check_shape(K, H)
    if terms not in (1, 2):
        raise ValueError("byte_linear_wgrad: terms must be 1 or 2")
    if N == 0:
        return torch.zeros((H, K), dtype=torch.float32, device=x.device)
    L = _lib()
    need = int(L.mgx_byte_linear_scratch_bytes(N, K, H))
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=x.device)
    elif (not isinstance(scratch, torch.Tensor) or scratch.device != x.device or not scratch.is_contiguous()
          or scratch.numel() * scratch.element_size() < need):
        raise ValueError(f"byte_linear_wgrad: scratch must be a contiguous device tensor of at least {need} bytes")
    dw = torch.empty((H, K), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        stream = torch.cuda.current_stream().cuda_stream
        rc = L.mgx_byte_linear_wgrad(x.data_ptr(), N, K, x.stride(0) if N > 1 else K, dy.data_ptr(), 1 if dy.dtype == torch.float32 else 2, H,
                                     int(terms), float(scale), dw.data_ptr(), scratch.data_ptr(), stream)
    if rc:
        raise RuntimeError(f"mgx_byte_linear_wgrad failed ({rc})")
    return dw


def _bf16_terms(t, terms: int):
    """float64 tensor of ``t`` as the kernels use it (hi, or hi + lo)."""
    import torch
    hi, lo = split_bf16(t)
    v = hi.to(torch.float64)
    return v + lo.to(torch.float64) if terms == 2 else v


def _function():
    import torch

    class _ByteLinearFn(torch.autograd.Function):
        """x u8 [N, K], weight [H, K], bias [H] or None -> [N, H].  Device tensors: the two kernels, weights cast and split per
        call.  CPU tensors: the same definition in float64, rounded once to the output dtype."""

        @staticmethod
        def forward(ctx, x, weight, bias, scale, terms, out_dtype):
            ctx.save_for_backward(x)
            ctx.scale, ctx.terms, ctx.w_dtype, ctx.has_bias = scale, terms, weight.dtype, bias is not None
            ctx.b_dtype = None if bias is None else bias.dtype
            if x.is_cuda:
                hi, lo = split_bf16(weight)
                b = None if bias is None else bias.detach().to(torch.float32).contiguous()
                return byte_linear(x, hi.contiguous(), lo.contiguous() if terms == 2 else None, b, scale, out_dtype=out_dtype)
            s = float(np.float32(scale))
            y = s * (x.to(torch.float64) @ _bf16_terms(weight, terms).t())
            if bias is not None:
                y = y + bias.detach().to(torch.float64)
            return y.to(out_dtype)

        @staticmethod
        def backward(ctx, dy):
            (x,) = ctx.saved_tensors
            gw = gb = None
            if ctx.needs_input_grad[1]:
                if x.is_cuda:
                    d = dy if dy.dtype == torch.bfloat16 else dy.to(torch.float32)
                    gw = byte_linear_wgrad(x, d.contiguous(), ctx.scale, ctx.terms).to(ctx.w_dtype)
                else:
                    d = _bf16_terms(dy, ctx.terms if dy.dtype != torch.bfloat16 else 1)
                    gw = (float(np.float32(ctx.scale)) * (d.t() @ x.to(torch.float64))).to(ctx.w_dtype)
            if ctx.has_bias and ctx.needs_input_grad[2]:
                gb = dy.to(torch.float32).sum(0).to(ctx.b_dtype)
            return None, gw, gb, None, None, None

    return _ByteLinearFn


_FN = None


def _module_base():
    import torch
    return torch.nn.Module


class ByteRowLinear(_module_base()):
    """``Linear(in_features, out_features)`` over u8 observation rows: ``forward(obs)`` takes u8 ``[..., T, 3]`` (3 T =
    in_features) or ``[..., K]`` and returns ``[..., out_features]``; leading dimensions are flattened for the kernels, so a
    ``[segments, bptt, T, 3]`` batch works.  ``weight [H, K]`` and ``bias [H]`` are float32 parameters with ``nn.Linear``'s
    names, shapes and init: the reference nets' ``_net.0.*`` / ``encoder.*`` entries load unchanged.  ``precision``: "bf16"
    (the weights rounded to bfloat16) or "bf16x2" (hi + lo, within 2**-16 of the float32 weights).  No gradient reaches
    ``obs``.  The activation and everything behind it stay the user's."""

    def __init__(self, in_features: int, out_features: int, bias: bool = True, scale: float = 1.0 / 255.0, precision: str = "bf16",
                 out_dtype=None) -> None:
        import torch
        super().__init__()
        in_features, out_features = int(in_features), int(out_features)
        _check_shape(in_features, out_features)
        if precision not in PRECISIONS:
            raise ValueError(f'ByteRowLinear: precision must be "bf16" or "bf16x2", not {precision!r}')
        out_dtype = torch.float32 if out_dtype is None else out_dtype
        if out_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("ByteRowLinear: out_dtype must be torch.float32 or torch.bfloat16")
        self.in_features, self.out_features = in_features, out_features
        self.scale, self.precision, self.out_dtype = float(scale), precision, out_dtype
        self.weight = torch.nn.Parameter(torch.empty((out_features, in_features), dtype=torch.float32))
        if bias:
            self.bias = torch.nn.Parameter(torch.empty(out_features, dtype=torch.float32))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self) -> None:   # nn.Linear.reset_parameters
        import torch
        torch.nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if self.bias is not None:
            bound = 1.0 / math.sqrt(self.in_features)
            torch.nn.init.uniform_(self.bias, -bound, bound)

    @classmethod
    def from_linear(cls, linear, scale: float = 1.0 / 255.0, precision: str = "bf16", out_dtype=None) -> "ByteRowLinear":
        """A layer with ``linear``'s weights (an ``nn.Linear``), on its device."""
        import torch
        m = cls(linear.in_features, linear.out_features, linear.bias is not None, scale, precision, out_dtype)
        m = m.to(linear.weight.device)
        with torch.no_grad():
            m.weight.copy_(linear.weight)
            if linear.bias is not None:
                m.bias.copy_(linear.bias)
        return m

    def extra_repr(self) -> str:
        return (f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, "
                f"scale={self.scale:g}, precision={self.precision}")

    def forward(self, obs):
        import torch
        global _FN
        K = self.in_features
        if not isinstance(obs, torch.Tensor) or obs.dtype != torch.uint8:
            raise ValueError("ByteRowLinear: obs must be a uint8 tensor (the observation rows)")
        if obs.dim() >= 2 and obs.shape[-1] == 3 and obs.shape[-2] * 3 == K:
            lead = obs.shape[:-2]
        elif obs.dim() >= 1 and obs.shape[-1] == K:
            lead = obs.shape[:-1]
        else:
            raise ValueError(f"ByteRowLinear: obs has shape {tuple(obs.shape)}, expected [..., {K}]" +
                             (f" or [..., {K // 3}, 3]" if K % 3 == 0 else ""))
        if obs.device != self.weight.device:
            raise ValueError(f"ByteRowLinear: obs is on {obs.device}, the weights on {self.weight.device}")
        x = obs.reshape(-1, K)
        if x.is_cuda and x.shape[0] > 1 and x.stride(1) != 1:
            x = x.contiguous()
        if _FN is None:
            _FN = _function()
        y = _FN.apply(x, self.weight, self.bias, self.scale, PRECISIONS[self.precision], self.out_dtype)
        return y.reshape(*lead, self.out_features)
