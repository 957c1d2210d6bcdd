"""Token-bag features: the front end of the reference's token baseline
(python/src/mettagrid/policy/token_encoder.py:88-114, ``TokenPolicyNet._encode_tokens``) as one pass over the token rows
plus one GEMM.

The reference sums ``s_t * (Px[x_t] + Py[y_t] + F[f_t])`` over a row's valid tokens (``coord != 0xFF``), with
``s_t = value_t / (scale[f_t] + 1e-6)``, and divides by ``sqrt(max(count, 1))``.  That is linear in the row's *bag*: the sums
of ``s_t`` per x nibble (16 columns), per y nibble (16) and per feature (C), so

    summary = (bag @ concat(Px[:16], Py[:16], F[:C])) / sqrt(max(count, 1))

``BatchedMettaGrid.token_bag`` computes ``(bag, counts)`` on the device (csrc/mgx_token_bag.hip); ``bag_host`` /
``summary_host`` restate both steps in numpy; ``TokenBagEmbedding`` carries the three tables under the reference net's
names and computes the summary with autograd reaching them through the GEMM: no [rows, T, hidden] intermediate, no
scatter-add in the backward pass.  Coord 0xFE (global tokens) is x = 14, y = 15 here, as in the reference net."""
from __future__ import annotations

import numpy as np

ROWS_PER_WORKGROUP = 4   # csrc/mgx_token_bag.hip MGX_BAG_WAVES: one wavefront per row (the tests' row counts sit around it)


def bag_host(tokens, scale, num_features: int):
    """``(bag float64 [rows, 32 + C], counts int32 [rows])`` of token rows u8 [rows, T, 3]: every term is the reference's
    float32 quotient ``float32(value) / (scale[feature] + float32(1e-6))``, the terms are summed in float64.  A token counts
    when ``coord != 0xFF`` and ``feature < C``."""
    tok = np.asarray(tokens, dtype=np.uint8)
    if tok.ndim != 3 or tok.shape[2] != 3:
        raise ValueError("tokens: u8 [rows, T, 3]")
    C = int(num_features)
    if not 1 <= C <= 256:
        raise ValueError("num_features must be in [1, 256]")
    scale = np.asarray(scale, dtype=np.float32)
    rows = tok.shape[0]
    coord, fid = tok[..., 0].astype(np.int64), tok[..., 1].astype(np.int64)
    valid = (coord != 0xFF) & (fid < C)
    denom = scale[np.minimum(fid, len(scale) - 1)] + np.float32(1e-6)     # float32 + float32, rounded once
    s = (tok[..., 2].astype(np.float32) / denom).astype(np.float64) * valid
    bag = np.zeros((rows, 32 + C), np.float64)
    r = np.broadcast_to(np.arange(rows)[:, None], coord.shape)
    np.add.at(bag, (r[valid], (coord & 15)[valid]), s[valid])
    np.add.at(bag, (r[valid], 16 + (coord >> 4)[valid]), s[valid])
    np.add.at(bag, (r[valid], 32 + fid[valid]), s[valid])
    return bag, valid.sum(axis=1).astype(np.int32)


def summary_host(bag, counts, Px, Py, F):
    """float64 [rows, hidden]: ``(bag @ concat(Px[:16], Py[:16], F[:C])) / sqrt(max(counts, 1))``."""
    bag = np.asarray(bag, dtype=np.float64)
    C = bag.shape[1] - 32
    table = np.concatenate([np.asarray(Px, np.float64)[:16], np.asarray(Py, np.float64)[:16], np.asarray(F, np.float64)[:C]])
    return (bag @ table) / np.sqrt(np.maximum(np.asarray(counts, np.float64), 1.0))[:, None]


def _module_base():
    import torch
    return torch.nn.Module


class TokenBagEmbedding(_module_base()):
    """The learned half of ``TokenPolicyNet._encode_tokens`` over bags: ``pos_x_embed``, ``pos_y_embed``, ``feature_embed``
    (``nn.Embedding(256, hidden)``) and the buffer ``_feature_scale`` — the reference net's names and shapes, so those four
    entries of its ``state_dict`` load unchanged.  ``forward(bag, counts)`` returns the input of the reference's ``token_mlp``;
    the MLP and the heads behind it stay the user's."""

    def __init__(self, hidden: int = 192, feature_scale=None) -> None:
        import torch
        super().__init__()
        self.hidden_size = int(hidden)
        scale = torch.ones(256, dtype=torch.float32)
        if feature_scale is not None:
            scale = torch.as_tensor(np.asarray(feature_scale, dtype=np.float32)).clone()
            if tuple(scale.shape) != (256,):
                raise ValueError("feature_scale: float32 [256]")
        self.register_buffer("_feature_scale", scale)
        self.pos_x_embed = torch.nn.Embedding(256, self.hidden_size)
        self.pos_y_embed = torch.nn.Embedding(256, self.hidden_size)
        self.feature_embed = torch.nn.Embedding(256, self.hidden_size)

    @classmethod
    def from_engine(cls, engine, hidden: int = 192) -> "TokenBagEmbedding":
        """Tables for ``engine.token_bag()``'s bags: the scale buffer is ``engine.feature_scale()``."""
        return cls(hidden, engine.feature_scale())

    def table(self, num_features: int):
        """[32 + C, hidden]: the rows of the three tables a bag's columns multiply."""
        import torch
        return torch.cat([self.pos_x_embed.weight[:16], self.pos_y_embed.weight[:16], self.feature_embed.weight[:num_features]])

    def forward(self, bag, counts):
        import torch
        C = bag.shape[-1] - 32
        if not 1 <= C <= 256:
            raise ValueError("bag: [rows, 32 + C] with C in [1, 256]")
        table = self.table(C)
        norm = torch.rsqrt(torch.clamp(counts, min=1).to(table.dtype))
        return (bag.to(table.dtype) @ table) * norm.unsqueeze(-1)
