"""Cost of the policy output side (mgx_sample_actions / mgx_action_logprob / _backward) at the rung-3 headline
batch (65 536 envs x 16 agents = 1 048 576 rows), for A = the rung-3 preset's transport_action_n and A = 64, float32 and
bfloat16 logits, in one process.  The variants alternate round by round (interleave what you compare, report the spread);
every round times `reps` back-to-back passes of each variant between two events on the stream; per variant the median over
the rounds is reported with min / max and the coefficient of variation:
  torch_sample     the reference's form in torch: log_softmax, exp, multinomial, gather, entropy = -(p * logp).sum(-1)
  mgx_sample       sample_actions (actions + logprob + entropy in one kernel)
  mgx_greedy       the same kernel, greedy
  torch_fwd_bwd    Categorical(logits).log_prob(a) / .entropy() and backward of (w * logprob - c * entropy).sum()
  mgx_fwd_bwd      action_logprob_entropy forward + backward of the same loss
  mgx_logprob / mgx_backward   the two kernels alone
For the kernels also the bytes one pass must move and that over the kernel's time as a fraction of 8 TB/s:
  sample N A e + 12 N, logprob N A e + 16 N, backward 2 N A e + 16 N   (e = bytes per logit).
Prints one JSON line.
Usage (GPU box): python scripts/action_sampling_timing.py [rows] [rounds] [reps]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mettagrid_amd import presets  # noqa: E402
from mettagrid_amd import sampling as sa  # noqa: E402
from mettagrid_amd.compiler import compile_spec  # noqa: E402
from mettagrid_amd.envs import split_action_names  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 65536 * 16
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5


def preset_actions() -> int:
    prog = compile_spec(presets.rung3_spec(), 32, 32, max_objects=192)
    names, vibes = split_action_names(prog.action_names)   # MettaGridBatchedEnv.transport_action_n
    return len(names) * (len(vibes) + 1) if vibes else len(names)


def timed(f, n: int) -> float:
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(n):
        f()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / n


def shape(A: int, dtype) -> dict:
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(A)
    logits = (3.0 * torch.randn((N, A), generator=gen, device=dev)).to(dtype)
    leaf = logits.clone().requires_grad_(True)
    w = torch.randn(N, generator=gen, device=dev)
    act = torch.empty(N, dtype=torch.int32, device=dev)
    lp, ent = torch.empty(N, device=dev), torch.empty(N, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    grad = torch.empty((N, A), dtype=dtype, device=dev)
    sa.sample_actions(logits, act, 1, 0, None, 1.0, False, lp, ent, bad)
    act64 = act.to(torch.int64)
    _, _, lse = sa.action_logprob(logits, act)
    state = {"step": 0}

    def torch_sample() -> None:
        with torch.no_grad():
            logp = torch.log_softmax(logits.float(), dim=-1)
            p = logp.exp()
            a = torch.multinomial(p, 1)
            logp.gather(1, a)
            -(p * logp).sum(-1)

    def mgx_sample(greedy: bool) -> None:
        state["step"] += 1
        sa.sample_actions(logits, act, 1, state["step"], None, 1.0, greedy, lp, ent, bad)

    def torch_fwd_bwd() -> None:
        leaf.grad = None
        d = torch.distributions.Categorical(logits=leaf.float())
        (w * d.log_prob(act64) - 0.01 * d.entropy()).sum().backward()

    def mgx_fwd_bwd() -> None:
        leaf.grad = None
        l, e = sa.action_logprob_entropy(leaf, act)
        (w * l - 0.01 * e).sum().backward()

    variants = {
        "torch_sample": torch_sample,
        "mgx_sample": lambda: mgx_sample(False),
        "mgx_greedy": lambda: mgx_sample(True),
        "torch_fwd_bwd": torch_fwd_bwd,
        "mgx_fwd_bwd": mgx_fwd_bwd,
        "mgx_logprob": lambda: sa.action_logprob(logits, act),
        "mgx_backward": lambda: sa.action_logprob_backward(logits, act, lse, w, lp, 1.0, out=grad),
    }
    for f in variants.values():   # warm every shape the timed window uses
        f()
    torch.cuda.synchronize()
    # what the kernels computed, against the torch form (a sanity line, not a test)
    with torch.no_grad():
        d = torch.distributions.Categorical(logits=logits.float())
        l, e, _ = sa.action_logprob(logits, act)
        d_lp, d_ent = float((l - d.log_prob(act.to(torch.int64))).abs().max()), float((e - d.entropy()).abs().max())   # (act: the last draw)
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for name, f in variants.items():
            ms[name].append(timed(f, reps))
    torch.cuda.synchronize()
    e = logits.element_size()
    must = {"mgx_sample": N * A * e + 12 * N, "mgx_greedy": N * A * e + 12 * N, "mgx_logprob": N * A * e + 16 * N,
            "mgx_backward": 2 * N * A * e + 16 * N}
    out = {"A": A, "dtype": str(dtype).replace("torch.", ""), "max_abs_diff_logprob": d_lp, "max_abs_diff_entropy": d_ent,
           "bad_rows": int(bad.item())}
    for name in variants:
        a = np.asarray(ms[name])
        out[name] = {"ms_median": round(float(np.median(a)), 4), "ms_min": round(float(a.min()), 4), "ms_max": round(float(a.max()), 4),
                     "cv_pct": round(float(a.std() / a.mean() * 100), 2)}
        if name in must:
            out[name]["bytes_per_pass"] = must[name]
            out[name]["fraction_of_8TBps"] = round(must[name] / (float(np.median(a)) * 1e-3) / 8e12, 4)
    out["sample_speedup"] = round(out["torch_sample"]["ms_median"] / out["mgx_sample"]["ms_median"], 2)
    out["fwd_bwd_speedup"] = round(out["torch_fwd_bwd"]["ms_median"] / out["mgx_fwd_bwd"]["ms_median"], 2)
    return out


def main() -> None:
    A3 = preset_actions()
    out = {"rows": N, "rounds": rounds, "reps": reps, "preset_actions": A3, "lib": os.path.basename(sa._lib()._name), "shapes": []}
    for A in (A3, 64):
        for dtype in (torch.float32, torch.bfloat16):
            out["shapes"].append(shape(A, dtype))
            torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)


main()
