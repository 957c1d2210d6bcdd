"""BUILD-CONTAINER ONLY — golden output of the reference's own token baseline front end.

    python tests/golden/make_token_policy_fixture.py

Builds the REFERENCE's ``TokenPolicyNet`` (python/src/mettagrid/policy/token_encoder.py:33-73) for a dozen features of mixed
normalisations, runs its ``_encode_tokens`` (:88-114) over seeded token rows and captures what reaches ``token_mlp``: the
per-row summary that ``mettagrid_amd/token_bag.py`` restates as bag @ table.  ``pufferlib`` is not installed here; the net
only wraps its Linear layers in ``pufferlib.pytorch.layer_init``, none of which lies before the captured tensor, so this
script's own stand-in (orthogonal weights, constant bias) takes its place in ``sys.modules``.
Rows: 0 all padding, 1 full (every token valid), 2 only 0xFE tokens, 3.. random fill (tokens grouped by cell as the engine
emits them, a random number of them, 0xFF behind).
Output: tests/golden/ref_token_policy_summary.npz — tokens u8 [rows, T, 3], feature_norms f32 [C], px / py f32 [16, hidden],
feat f32 [C, hidden], summary f32 [rows, hidden] (data only).
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_reference_fixtures as mrf  # noqa: E402

NORMS = [0.5, 1.0, 1.0, 10.0, 255.0, 255.0, 100.0, 0.25, 10.0, 1.0, 255.0, 30.0]
ROWS, T, SEED = 37, 200, 20240607


def layer_init_stand_in():
    import torch

    def layer_init(layer, std=np.sqrt(2), bias_const=0.0):
        torch.nn.init.orthogonal_(layer.weight, std)
        torch.nn.init.constant_(layer.bias, bias_const)
        return layer

    import importlib.machinery
    pufferlib, pytorch = types.ModuleType("pufferlib"), types.ModuleType("pufferlib.pytorch")
    for m in (pufferlib, pytorch):   # (the reference asks importlib.util.find_spec whether pufferlib is there)
        m.__spec__ = importlib.machinery.ModuleSpec(m.__name__, None)
    pytorch.layer_init = layer_init
    pufferlib.pytorch = pytorch
    sys.modules["pufferlib"], sys.modules["pufferlib.pytorch"] = pufferlib, pytorch


def token_rows(rng: np.random.Generator) -> np.ndarray:
    C = len(NORMS)
    tok = np.full((ROWS, T, 3), 0xFF, np.uint8)
    for r in range(1, ROWS):
        n = T if r in (1, 2) else int(rng.integers(1, T + 1))
        t = 0
        while t < n:   # a cell's tokens follow each other
            k = min(n - t, int(rng.integers(1, 9)))
            tok[r, t:t + k, 0] = 0xFE if r == 2 else int(rng.integers(0, 11)) << 4 | int(rng.integers(0, 11))
            tok[r, t:t + k, 1] = rng.integers(0, C, k)
            tok[r, t:t + k, 2] = rng.integers(0, 256, k)
            t += k
    return tok


def main() -> None:
    import torch
    layer_init_stand_in()
    mrf.import_reference(shim=True)
    from mettagrid.policy.token_encoder import TokenPolicyNet
    torch.manual_seed(SEED)
    features = [types.SimpleNamespace(id=i, normalization=z) for i, z in enumerate(NORMS)]
    actions = types.SimpleNamespace(actions=lambda: ["noop", "move_north", "move_south", "move_west", "move_east"])
    net = TokenPolicyNet(features, actions).eval()
    captured = []
    net.token_mlp.register_forward_pre_hook(lambda module, args: captured.append(args[0].detach().clone()))
    tok = token_rows(np.random.default_rng(SEED))
    with torch.no_grad():
        net._encode_tokens(torch.from_numpy(tok))
    (summary,) = captured
    assert summary.dtype == torch.float32 and tuple(summary.shape) == (ROWS, net.hidden_size)
    C = len(NORMS)
    p = os.path.join(HERE, "ref_token_policy_summary.npz")
    np.savez_compressed(p, tokens=tok, feature_norms=np.asarray(NORMS, np.float32), px=net.pos_x_embed.weight[:16].detach().numpy(),
                        py=net.pos_y_embed.weight[:16].detach().numpy(), feat=net.feature_embed.weight[:C].detach().numpy(),
                        summary=summary.numpy())
    print(p, os.path.getsize(p), "bytes;", ROWS, "rows")


if __name__ == "__main__":
    main()
