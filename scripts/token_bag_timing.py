"""Cost of the token-bag features (mgx_token_bag) at the rung-3 headline shape (65 536 envs x 16 agents, 200
tokens per row), in one process, on the observations after a warm-up of random steps.  The variants alternate round by round
(interleave what you compare, report the spread); every round times `reps` back-to-back passes of each variant between two
events on the engine's stream; per variant the median over the rounds is reported with min / max and the coefficient of
variation:
  decode      mgx_decode_obs on the same rows (the yardstick kernel: it writes 26x the token bytes)
  bag_f32     mgx_token_bag, float32 bag          bag_bf16    ... bfloat16 bag
  bag_gemm    bag_f32 + TokenBagEmbedding.forward (one GEMM and the normalisation)
  bag_gemm_bwd  ... + backward to the three tables (torch's GEMM backward)
  gather_fwd / gather_fwd_bwd   the reference's form in torch (token_encoder.py:88-114: three embedding gathers per token,
              multiply, mask, sum), in chunks of `chunk` rows so that its [rows, T, hidden] float32 intermediates fit, over
              the first `gather_rows` rows only; `ms_all_rows` scales that time to all rows (the form is row-parallel)
For the bag kernel also the bytes one pass must move — 3 T + 4 (32 + C) + 4 per row (2 (32 + C) for bfloat16) — and that
over the kernel's time as a fraction of 8 TB/s.  Prints one JSON line.
Usage (GPU box): python scripts/token_bag_timing.py [envs] [rounds] [reps] [gather_rows] [chunk]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mettagrid_amd import presets  # noqa: E402
from mettagrid_amd.compiler import compile_spec  # noqa: E402
from mettagrid_amd.engine import BatchedMettaGrid  # noqa: E402
from mettagrid_amd.mapgen import random_class_maps  # noqa: E402
from mettagrid_amd.token_bag import TokenBagEmbedding  # noqa: E402

E = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
gather_rows = int(sys.argv[4]) if len(sys.argv) > 4 else 131072
chunk = int(sys.argv[5]) if len(sys.argv) > 5 else 16384
WARMUP_STEPS = 20


def gather_form(m: TokenBagEmbedding, tokens: torch.Tensor) -> torch.Tensor:
    """TokenPolicyNet._encode_tokens up to the input of token_mlp, on the module's tables."""
    coord = tokens[..., 0].long()
    fid = tokens[..., 1].long()
    valid = coord != 0xFF
    emb = m.pos_x_embed(coord & 15) + m.pos_y_embed((coord >> 4) & 15) + m.feature_embed(fid)
    emb = emb * (tokens[..., 2].float() / (m._feature_scale[fid] + 1e-6)).unsqueeze(-1)
    emb = emb * valid.unsqueeze(-1).to(emb.dtype)
    return emb.sum(dim=-2) / torch.sqrt(valid.sum(dim=-1, keepdim=True).clamp_min(1).float())


def main() -> None:
    prog = compile_spec(presets.rung3_spec(), 32, 32, max_objects=192)
    maps = random_class_maps(prog, 32, 32, {"wall": 40, "extractor": 8, "chest": 4}, {"red": 8, "blue": 8}, range(16))
    eng = BatchedMettaGrid(prog, maps[np.arange(E) % 16], np.arange(E, dtype=np.uint32), buffers="device", specialize=False)
    A, T, C = prog.num_agents, eng.T, len(prog.feature_norms)
    rows = E * A
    dev = eng.obs.device
    stream = eng._ext_stream()
    gen = torch.Generator(device=dev).manual_seed(1)
    nact = len(prog.action_names)
    for _ in range(WARMUP_STEPS):
        eng.actions.copy_(torch.randint(0, nact, (rows,), generator=gen, device=dev, dtype=torch.int32))
        eng.vibe_actions.copy_(torch.randint(0, nact, (rows,), generator=gen, device=dev, dtype=torch.int32))
        eng.wait_for_caller()
        eng.step()
    eng.sync()
    torch.cuda.synchronize()
    Hh, Ww = int(prog.words[13]), int(prog.words[14])   # MGX_H_OBS_HEIGHT / WIDTH
    box = torch.empty((rows, C, Hh, Ww), dtype=torch.float32, device=dev)
    bag32 = torch.empty((rows, 32 + C), dtype=torch.float32, device=dev)
    bag16 = torch.empty((rows, 32 + C), dtype=torch.bfloat16, device=dev)
    counts = torch.empty((rows,), dtype=torch.int32, device=dev)
    torch.manual_seed(0)
    m = TokenBagEmbedding.from_engine(eng).to(dev)
    g_rows = min(gather_rows, rows)
    grad_out = torch.randn((rows, m.hidden_size), device=dev)
    torch.cuda.synchronize()

    def bag_gemm(backward: bool) -> None:
        eng.token_bag(bag32, counts)
        with torch.cuda.stream(stream), torch.set_grad_enabled(backward):
            out = m(bag32, counts)
            if backward:
                m.zero_grad(set_to_none=True)
                out.backward(grad_out)

    def gather(backward: bool) -> None:
        with torch.cuda.stream(stream), torch.set_grad_enabled(backward):
            if backward:
                m.zero_grad(set_to_none=True)
            for r0 in range(0, g_rows, chunk):
                out = gather_form(m, eng.obs[r0:min(r0 + chunk, g_rows)])
                if backward:
                    out.backward(grad_out[r0:r0 + out.shape[0]])

    variants = {
        "decode": (lambda: eng.decode_obs(out=box), reps),
        "bag_f32": (lambda: eng.token_bag(bag32, counts), reps),
        "bag_bf16": (lambda: eng.token_bag(bag16, counts), reps),
        "bag_gemm": (lambda: bag_gemm(False), reps),
        "bag_gemm_bwd": (lambda: bag_gemm(True), reps),
        "gather_fwd": (lambda: gather(False), 1),
        "gather_fwd_bwd": (lambda: gather(True), 1),
    }

    def timed(f, n: int) -> float:
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        for _ in range(n):
            f()
        t1.record(stream)
        t1.synchronize()
        return t0.elapsed_time(t1) / n

    for f, _ in variants.values():   # warm every shape the timed window uses
        f()
    eng.sync()
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for name, (f, n) in variants.items():
            ms[name].append(timed(f, n))
    eng.sync()
    mean_tokens = float(counts.double().mean())
    out = {"envs": E, "rows": rows, "T": T, "C": C, "rounds": rounds, "reps": reps, "mean_tokens_per_row": round(mean_tokens, 1),
           "gather_rows": g_rows, "chunk": chunk, "lib": os.path.basename(eng.L._name)}
    row_bytes = {"bag_f32": 3 * T + 4 * (32 + C) + 4, "bag_bf16": 3 * T + 2 * (32 + C) + 4, "decode": 3 * T + 4 * C * Hh * Ww}
    for name in variants:
        a = np.asarray(ms[name])
        out[name] = {"ms_median": round(float(np.median(a)), 4), "ms_min": round(float(a.min()), 4), "ms_max": round(float(a.max()), 4),
                     "cv_pct": round(float(a.std() / a.mean() * 100), 2)}
        if name in row_bytes:
            out[name]["bytes_per_pass"] = rows * row_bytes[name]
            out[name]["fraction_of_8TBps"] = round(rows * row_bytes[name] / (float(np.median(a)) * 1e-3) / 8e12, 4)
        if name.startswith("gather"):
            out[name]["ms_all_rows"] = round(float(np.median(a)) * rows / g_rows, 2)
    eng.close()
    print(json.dumps(out), flush=True)


main()
