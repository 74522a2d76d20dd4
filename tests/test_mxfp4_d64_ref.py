"""The learned sink logit's merge (csrc/mxfp4_attn.h mx_merge_row SINK), restated in torch float32 and held to
float64 softmax attention with a sink, and the rotary table widths of head_dim 64.  CPU only."""
import math

import pytest
import torch


def sink_merge(M, L, acc, sink):
    """M, L [R], acc [R, D] fp32: the rows' merged states, M an integer or -inf -> (O, lse) after the sink joins."""
    z = sink * torch.tensor(math.log2(math.e), dtype=torch.float32)
    Mp = torch.maximum(M, torch.ceil(z))
    w = torch.where(torch.isinf(M), torch.zeros_like(M), torch.exp2(M - Mp))
    Lp = w * L + torch.exp2(z - Mp)
    return (w[:, None] * acc) / Lp[:, None], Mp + torch.log2(Lp)


@pytest.mark.parametrize("sink", [-30.0, 0.0, 5.0, 40.0])
def test_sink_merge_is_softmax_with_a_sink(sink):
    g = torch.Generator().manual_seed(1)
    s = torch.randn((64, 200), generator=g, dtype=torch.float64) * 4      # scores, log2 units
    s[0] = float("-inf")                                                   # a row that sees no key
    v = torch.randn((200, 16), generator=g, dtype=torch.float64)
    M = torch.ceil(s.amax(-1))
    p = torch.where(torch.isinf(s), torch.zeros_like(s), torch.exp2(s - M[:, None]))
    O, lse = sink_merge(M.float(), p.sum(-1).float(), (p @ v).float(), torch.full((64,), sink))
    z = sink * math.log2(math.e)
    den = torch.exp2(s).sum(-1) + 2.0 ** z
    assert torch.allclose(O.double(), (torch.exp2(s) @ v) / den[:, None], rtol=1e-5, atol=1e-6)
    assert torch.allclose(lse.double(), torch.log2(den), rtol=0, atol=1e-4)
    assert (O[0] == 0).all() and abs(lse[0].item() - z) <= 1e-5


def test_rope_tables_are_64_or_128_wide():
    from quantizedattention_amd._lib import QAttnError
    from quantizedattention_amd.attention_mxfp4 import Rope, rope_table
    assert rope_table(5, head_dim=64).shape == (5, 64) and rope_table(5).shape == (5, 128)
    assert torch.equal(rope_table(5, head_dim=64)[:, 0], torch.arange(5, dtype=torch.float64).cos().float())
    for bad in (lambda: rope_table(5, head_dim=96), lambda: Rope(torch.zeros((4, 96)))):
        with pytest.raises(QAttnError):
            bad()
