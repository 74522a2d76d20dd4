"""The capped restatement (tests/mxfp4_softcap_ref.py) against plain float64 capped attention on the dequantised
operands (CPU)."""
import torch

import mxfp4_ragged_ref as RR
import mxfp4_softcap_ref as CR
import mxfp4_split_ref as SR


def _figures(got, want):
    return ((got[0].double() - want[0]).norm() / want[0].norm()).item(), (got[1] - want[1]).abs().max().item()


def test_capped_restatement_follows_float64_capped_attention():
    """The bar is the uncapped oracle's own error against float64 uncapped attention on the same inputs, times 1.5
    (a capped, flatter row spreads P over more FP4 blocks); the inputs bite when float64 UNCAPPED attention misses
    the capped reference by 5 bars or more.  Both errors are the FP4 rounding of P, which cancels in O / l on a row
    that one key dominates, so the comparison needs inputs that reach the cap without making the uncapped rows
    one-hot: q and k with a common component (randn + 3 at head_dim 128: scale * s = 102 +- 4, EVERY logit past
    the cap of 50, the rows of the uncapped oracle as spread as on plain inputs), 4 / 2 heads, 33 causal queries
    over 200 keys.  Measured, (relL2 of O, max |dlse|):

        uncapped oracle against float64 uncapped   (9.24e-2, 0.325)   -> bars (1.39e-1, 0.487)
        capped restatement against float64 capped  (9.67e-2, 0.053)
        float64 uncapped against float64 capped    (5.76, 92.2)

    (Zero-mean inputs that reach the cap, 32 q, make every uncapped row one-hot and its O error vanish, 1.8e-2,
    while the capped rows keep 6.3e-2: there the FP4 regimes differ and the ratio says nothing about the cap.)"""
    g = torch.Generator().manual_seed(11)
    q = (torch.randn((1, 4, 33, 128), generator=g) + 3).half()
    k, v = (torch.randn((1, 2, 200, 128), generator=g) + 3).half(), torch.randn((1, 2, 200, 128), generator=g).half()
    O, lse = SR.merge(*RR.sequence_partials(q, k, v, True, 128, 2))
    plain, capped = CR.dense_reference(q, k, v, "causal"), CR.dense_reference(q, k, v, "causal", 50.0)
    bars = [1.5 * x for x in _figures((O.view(q.shape), lse), plain)]
    got = _figures(CR.mxfp4_fwd_softcap(q, k, v, "causal", 128, 50.0), capped)
    bite = _figures(plain, capped)
    print(f"bars {bars}, capped restatement {got}, float64 uncapped against capped {bite}")
    assert bite[0] >= 5 * bars[0] and bite[1] >= 5 * bars[1]
    assert got[0] <= bars[0] and got[1] <= bars[1]
