"""Cost of the dense-policy front end (mgx_byte_linear_forward / _wgrad) at the rung-3 headline shape (65 536
envs x 16 agents = 1 048 576 rows, K = 600 bytes per row, H = 128), in one process, on the engine's own observation rows after
20 random steps.  The variants alternate round by round (interleave what you compare, report the spread); every round times
`reps` back-to-back passes of each variant between two events on the stream; per variant the median over the rounds is
reported with min / max and the coefficient of variation:
  torch_f32        the reference's form in torch: F.linear(x.view(N, -1).float() * (1 / 255), W, b)   (the yardstick)
  torch_autocast   the same under torch.autocast(bfloat16)
  bl_t1_f32 / bl_t1_bf16 / bl_t2_f32 / bl_t2_bf16     byte_linear, one / two weight terms, float32 / bfloat16 output
  *_bwd            forward + backward to the weight and the bias: the two torch forms, ByteRowLinear "bf16" and "bf16x2"
  wgrad_t1 / wgrad_t2   the weight-gradient kernels alone (float32 dy)
For the forward kernel also the bytes one pass must move — N K + N H sizeof(out) + the weights — and that over the kernel's
time as a fraction of 8 TB/s.  Prints one JSON line.
Usage (GPU box): python scripts/byte_linear_timing.py [envs] [rounds] [reps] [hidden]"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mettagrid_amd import byte_linear as bl  # noqa: E402
from mettagrid_amd import presets  # noqa: E402
from mettagrid_amd.compiler import compile_spec  # noqa: E402
from mettagrid_amd.engine import BatchedMettaGrid  # noqa: E402
from mettagrid_amd.mapgen import random_class_maps  # noqa: E402

E = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
H = int(sys.argv[4]) if len(sys.argv) > 4 else 128
WARMUP_STEPS = 20


def main() -> None:
    prog = compile_spec(presets.rung3_spec(), 32, 32, max_objects=192)
    maps = random_class_maps(prog, 32, 32, {"wall": 40, "extractor": 8, "chest": 4}, {"red": 8, "blue": 8}, range(16))
    eng = BatchedMettaGrid(prog, maps[np.arange(E) % 16], np.arange(E, dtype=np.uint32), buffers="device", specialize=False)
    rows = E * prog.num_agents
    dev = eng.obs.device
    gen = torch.Generator(device=dev).manual_seed(1)
    nact = len(prog.action_names)
    for _ in range(WARMUP_STEPS):
        eng.actions.copy_(torch.randint(0, nact, (rows,), generator=gen, device=dev, dtype=torch.int32))
        eng.vibe_actions.copy_(torch.randint(0, nact, (rows,), generator=gen, device=dev, dtype=torch.int32))
        eng.wait_for_caller()
        eng.step()
    eng.sync()
    obs = eng.obs.clone()          # u8 [rows, T, 3]: the engine's own rows, from here on on torch's stream
    eng.close()
    torch.cuda.synchronize()
    K = obs.shape[1] * 3
    x = obs.view(rows, K)
    used = float((obs[..., 0] != 0xFF).sum(1).double().mean())

    torch.manual_seed(0)
    lin = torch.nn.Linear(K, H).to(dev)
    m1 = bl.ByteRowLinear.from_linear(lin, precision="bf16")
    m2 = bl.ByteRowLinear.from_linear(lin, precision="bf16x2")
    hi, lo = bl.split_bf16(lin.weight)
    bias = lin.bias.detach()
    grad_out = torch.randn((rows, H), device=dev)
    out32 = torch.empty((rows, H), dtype=torch.float32, device=dev)
    out16 = torch.empty((rows, H), dtype=torch.bfloat16, device=dev)
    scratch = torch.empty(bl._lib().mgx_byte_linear_scratch_bytes(rows, K, H), dtype=torch.uint8, device=dev)

    def torch_form(autocast: bool, backward: bool) -> None:
        with torch.set_grad_enabled(backward), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            y = F.linear(x.view(rows, -1).float() * (1.0 / 255.0), lin.weight, lin.bias)
        if backward:
            lin.zero_grad(set_to_none=True)
            y.backward(grad_out.to(y.dtype))

    def layer(m, backward: bool) -> None:
        with torch.set_grad_enabled(backward):
            y = m(obs)
        if backward:
            m.zero_grad(set_to_none=True)
            y.backward(grad_out)

    variants = {
        "torch_f32": lambda: torch_form(False, False),
        "torch_autocast": lambda: torch_form(True, False),
        "bl_t1_f32": lambda: bl.byte_linear(x, hi, None, bias, out=out32),
        "bl_t1_bf16": lambda: bl.byte_linear(x, hi, None, bias, out=out16),
        "bl_t2_f32": lambda: bl.byte_linear(x, hi, lo, bias, out=out32),
        "bl_t2_bf16": lambda: bl.byte_linear(x, hi, lo, bias, out=out16),
        "torch_f32_bwd": lambda: torch_form(False, True),
        "torch_autocast_bwd": lambda: torch_form(True, True),
        "bl_t1_bwd": lambda: layer(m1, True),
        "bl_t2_bwd": lambda: layer(m2, True),
        "wgrad_t1": lambda: bl.byte_linear_wgrad(x, grad_out, terms=1, scratch=scratch),
        "wgrad_t2": lambda: bl.byte_linear_wgrad(x, grad_out, terms=2, scratch=scratch),
    }

    def timed(f, n: int) -> float:
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(n):
            f()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) / n

    for f in variants.values():   # warm every shape the timed window uses
        f()
    torch.cuda.synchronize()
    # what the kernels computed, against the yardstick form (a sanity line, not a test)
    with torch.no_grad():
        ref = F.linear(x.float() * (1.0 / 255.0), lin.weight, lin.bias)
        d2 = float((bl.byte_linear(x, hi, lo, bias) - ref).abs().max())
        d1 = float((bl.byte_linear(x, hi, None, bias) - ref).abs().max())
        ref_abs = float(ref.abs().max())
        del ref
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for name, f in variants.items():
            ms[name].append(timed(f, reps))
    torch.cuda.synchronize()
    out = {"envs": E, "rows": rows, "K": K, "H": H, "rounds": rounds, "reps": reps, "mean_tokens_per_row": round(used, 1),
           "chunk_rows": bl.chunk_rows(), "max_abs_y": round(ref_abs, 4), "max_abs_diff_t1": d1, "max_abs_diff_t2": d2,
           "lib": os.path.basename(bl._lib()._name)}
    wbytes = H * K * 2
    must = {"bl_t1_f32": rows * K + rows * H * 4 + wbytes, "bl_t1_bf16": rows * K + rows * H * 2 + wbytes,
            "bl_t2_f32": rows * K + rows * H * 4 + 2 * wbytes, "bl_t2_bf16": rows * K + rows * H * 2 + 2 * wbytes}
    for name in variants:
        a = np.asarray(ms[name])
        out[name] = {"ms_median": round(float(np.median(a)), 4), "ms_min": round(float(a.min()), 4), "ms_max": round(float(a.max()), 4),
                     "cv_pct": round(float(a.std() / a.mean() * 100), 2)}
        if name in must:
            out[name]["bytes_per_pass"] = must[name]
            out[name]["fraction_of_8TBps"] = round(must[name] / (float(np.median(a)) * 1e-3) / 8e12, 4)
    print(json.dumps(out), flush=True)


main()
