"""The windowed restatement (tests/mxfp4_window_ref.py) on the CPU: with a window that covers the whole
sequence it IS the ragged causal restatement (torch.equal on O and lse, whatever the sink count), and
against float64 softmax attention with the same mask on the dequantised operands it keeps the bar
tests/test_mxfp4_oracle.py and tests/test_mxfp4_causal_ref.py hold the definition to (cosine >= 0.95).
tests/test_gpu_mxfp4_window.py pins the kernel to this restatement.
"""
import pytest
import torch

import mxfp4_masked_ref as MR
import mxfp4_ragged_ref as RR
import mxfp4_window_ref as WR


def _sequence(Hq, Hkv, Sq, L, seed=2):
    q, ks, vs = RR.inputs(1, Hq, Hkv, Sq, (L,), seed=seed)
    return q, ks[0], vs[0]


@pytest.mark.parametrize("S", [0, 4, 100])
@pytest.mark.parametrize("Sq,L,kps", [(1, 200, 64), (33, 130, 128), (70, 70, 64), (3, 256, 4096)])
def test_window_of_everything_is_the_ragged_causal_restatement(Sq, L, kps, S):
    q, k, v = _sequence(4, 2, Sq, L)
    RO, Rl, (Rm, Rll) = RR.mxfp4_fwd_ragged(q, [k], [v], True, kps)
    for W in (L, L + 1, 1 << 40):
        O, lse, (m, l) = WR.mxfp4_fwd_window(q, k, v, W, S, kps)
        assert torch.equal(O, RO) and torch.equal(lse, Rl), (W, S)
        assert torch.equal(m, Rm) and torch.equal(l, Rll), (W, S)


def test_split_structure():
    # (L, Sq, W, S, kps) -> tile ranges
    assert WR.split_tiles(32768, 1, 4096, 4, 1024) == [(0, 1)] + [(t, min(512, t + 16)) for t in range(448, 512, 16)]
    assert WR.split_tiles(200, 1, 72, 0, 64) == [(2, 3), (3, 4)]                     # S = 0: no sink split
    assert WR.split_tiles(321, 1, 129, 64, 64) == [(0, 1), (3, 4), (4, 5), (5, 6)]
    assert WR.split_tiles(256, 33, 100, 70, 128) == [(0, 2), (2, 4)]                 # the runs touch
    assert WR.split_tiles(256, 1, 37, 64, 128) == [(0, 1), (3, 4)]


def test_s0_gap_has_no_sink_split():
    """S = 0 and a window far from the start: wt0 > nst = 0, a gap with no sink tile, so the plan has no
    sink split (rec[6] = 0) and its splits start at rec[5] = wt0."""
    from quantizedattention_amd.kv_cache_mxfp4 import _window_tiles, plan_varlen
    assert _window_tiles(200, 1, 72, 0) == (2, 0, 4)
    kps, rec, work, rows = plan_varlen([200], [0], [1], 4, 2, 64, True, 72, 0)
    assert rec == [[0, 0, 1, 2, 0, 2, 0, 0]] and sorted(w[2] for w in work) == [0, 1] and rows == 2 * 2 * 2


@pytest.mark.parametrize("W,S", [(1, 0), (1, 4), (5, 0), (64, 0), (100, 4), (100, 70), (37, 64)])
def test_definition_accuracy(W, S):
    for Sq, L in ((3, 130), (33, 256)):
        q, k, v = _sequence(4, 2, Sq, L)
        O, lse, _ = WR.mxfp4_fwd_window(q, k, v, W, S, 64)
        RO, Rl = WR.dense_reference(q, k, v, W, S)
        cos = MR.cosine(O, RO)
        print(f"MXFP4-WINDOW-DEF W={W} S={S} Sq={Sq} L={L} cos {cos:.4f} "
              f"lse err {(lse.double() - Rl).abs().max().item():.4f}")
        assert torch.isfinite(lse).all() and torch.isfinite(O.float()).all()
        assert cos >= 0.95, cos
