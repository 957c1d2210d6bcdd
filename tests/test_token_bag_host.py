"""Host: the token-bag restatement of the reference's token baseline front end (mettagrid_amd/token_bag.py)
against the reference's own summary (tests/golden/ref_token_policy_summary.npz, captured at the input of TokenPolicyNet's
token_mlp by tests/golden/make_token_policy_fixture.py), and TokenBagEmbedding against the plain gather-multiply-sum form."""
import os

import numpy as np
import pytest

from mettagrid_amd import token_bag as tb

HERE = os.path.dirname(os.path.abspath(__file__))
U = 2.0 ** -24   # unit roundoff of float32


@pytest.fixture(scope="module")
def fix():
    z = np.load(os.path.join(HERE, "golden", "ref_token_policy_summary.npz"))
    scale = np.ones(256, np.float32)
    scale[:len(z["feature_norms"])] = np.maximum(z["feature_norms"], np.float32(1.0))
    return {k: z[k] for k in z.files} | {"scale": scale, "C": len(z["feature_norms"])}


def test_bag_form_equals_the_reference_summary(fix):
    """|summary_host(bag_host(rows)) - reference| <= (T + 8) u (|bag| @ |E|) / sqrt(max(count, 1)), componentwise: the
    reference's own float32 rounding (three roundings per token, a T-term sum, the normalisation).  Measured on this fixture: 3.0 u."""
    tok, C = fix["tokens"], fix["C"]
    T = tok.shape[1]
    bag, counts = tb.bag_host(tok, fix["scale"], C)
    got = tb.summary_host(bag, counts, fix["px"], fix["py"], fix["feat"])
    table = np.concatenate([fix["px"], fix["py"], fix["feat"]]).astype(np.float64)
    bound = (np.abs(bag) @ np.abs(table)) / np.sqrt(np.maximum(counts, 1))[:, None]
    err = np.abs(got - fix["summary"].astype(np.float64))
    ratio = (err / np.where(bound > 0, bound, 1.0)).max() / U
    print(f"max |delta| / bound = {ratio:.2f} u (allowed {T + 8})")
    assert (err <= (T + 8) * U * bound).all()
    # row 0 is all padding: exactly zero, count 0
    assert counts[0] == 0 and not bag[0].any() and not got[0].any() and not fix["summary"][0].any()
    # row 1 is full
    assert counts[1] == T
    # row 2 holds only 0xFE tokens: x = 14, y = 15, nothing else among the position columns
    assert (tok[2, :, 0] == 0xFE).all() and counts[2] == T
    assert bag[2, 14] > 0 and bag[2, 16 + 15] == bag[2, 14] and np.count_nonzero(bag[2, :32]) == 2
    only_fe = (bag[2, 14] * (fix["px"][14].astype(np.float64) + fix["py"][15]) + bag[2, 32:] @ fix["feat"].astype(np.float64)) / np.sqrt(T)
    assert np.allclose(got[2], only_fe, rtol=1e-12, atol=0)


def test_bag_host_skips_foreign_features_and_padding():
    tok = np.array([[[0x21, 0, 10], [0x21, 3, 7], [0xFF, 0, 9], [0xFE, 1, 255], [0x00, 2, 0]]], np.uint8)
    scale = np.ones(256, np.float32)
    scale[1] = 10.0
    bag, counts = tb.bag_host(tok, scale, 3)
    assert counts.tolist() == [3]           # feature 3 >= C and the padding token are not counted
    s0 = np.float64(np.float32(10) / (np.float32(1) + np.float32(1e-6)))
    s1 = np.float64(np.float32(255) / (np.float32(10) + np.float32(1e-6)))
    want = np.zeros(35)
    want[1] = want[16 + 2] = want[32 + 0] = s0
    want[14] = want[16 + 15] = want[32 + 1] = s1
    assert np.array_equal(bag[0], want)


def _gather_form(tok, scale, C, px, py, feat):
    """The reference's computation written out in torch (float64): gather three rows per token, multiply, mask, sum."""
    import torch
    t = torch.from_numpy(tok.astype(np.int64))
    coord, fid = t[..., 0], t[..., 1]
    valid = (coord != 0xFF) & (fid < C)
    fc = fid.clamp(max=C - 1)
    emb = px[coord & 15] + py[(coord >> 4) & 15] + feat[fc]
    s = torch.from_numpy((tok[..., 2].astype(np.float32) / (scale[np.minimum(tok[..., 1], 255)] + np.float32(1e-6))).astype(np.float64))
    emb = emb * (s * valid).unsqueeze(-1)
    return emb.sum(dim=-2) / torch.sqrt(valid.sum(dim=-1, keepdim=True).clamp_min(1).double())


def test_embedding_module_matches_the_gather_form_and_its_gradients(fix):
    import torch
    tok, C, scale = fix["tokens"], fix["C"], fix["scale"]
    torch.manual_seed(5)
    m = tb.TokenBagEmbedding(hidden=24, feature_scale=scale).double()
    bag, counts = tb.bag_host(tok, scale, C)
    out = m(torch.from_numpy(bag), torch.from_numpy(counts))
    want = tb.summary_host(bag, counts, m.pos_x_embed.weight.detach().numpy(), m.pos_y_embed.weight.detach().numpy(),
                           m.feature_embed.weight.detach().numpy())
    assert np.allclose(out.detach().numpy(), want, rtol=1e-12, atol=0)
    g = torch.from_numpy(np.random.default_rng(1).standard_normal(out.shape))
    out.backward(g)
    px, py, ft = (w.detach().clone().requires_grad_(True) for w in (m.pos_x_embed.weight, m.pos_y_embed.weight, m.feature_embed.weight))
    ref = _gather_form(tok, scale, C, px, py, ft)
    assert torch.allclose(out.detach(), ref.detach(), rtol=1e-10, atol=0)
    ref.backward(g)
    for name, mine, theirs in (("pos_x", m.pos_x_embed.weight.grad, px.grad), ("pos_y", m.pos_y_embed.weight.grad, py.grad),
                               ("feature", m.feature_embed.weight.grad, ft.grad)):
        assert theirs.abs().max().item() > 0, name
        assert torch.allclose(mine, theirs, rtol=1e-10, atol=0), name
    assert not m.pos_x_embed.weight.grad[16:].any() and not m.pos_y_embed.weight.grad[16:].any()
    assert not m.feature_embed.weight.grad[C:].any()


def test_reference_state_dict_entries_load():
    """The four entries of a reference TokenPolicyNet state_dict that belong to the front end: same names, same shapes."""
    import torch
    g = torch.Generator().manual_seed(3)
    ref_entries = {"_feature_scale": torch.rand(256, generator=g) + 1, "pos_x_embed.weight": torch.randn(256, 192, generator=g),
                   "pos_y_embed.weight": torch.randn(256, 192, generator=g), "feature_embed.weight": torch.randn(256, 192, generator=g)}
    m = tb.TokenBagEmbedding()
    assert set(m.state_dict()) == set(ref_entries)
    m.load_state_dict(ref_entries, strict=True)
    for k, v in ref_entries.items():
        assert torch.equal(m.state_dict()[k], v)
    full = dict(ref_entries, **{"token_mlp.0.weight": torch.zeros(192, 192)})   # a whole reference dict: the rest is the user's
    missing, unexpected = m.load_state_dict(full, strict=False)
    assert not missing and unexpected == ["token_mlp.0.weight"]
