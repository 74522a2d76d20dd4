"""The CPU side of the forward-mode block instrument (tests/jvp_blocks.py; on the GPU
tests/test_gpu_jvp_blocks.py).

  * The bars are pinned to the restatement: on every case of a family ``restate`` sits within a third
    of the family's bars of ``truth`` (tO and O block by block, lse in absolute terms), and the worst
    case reaches at least 0.8 of that third, so a constant cannot drift away from what it was measured on.
  * Every ladder and climb case moves the running max on some (wave block, key tile after the first)
    pair: a case that stops doing so stops testing the rescale, and fails here.
  * Five faults planted one at a time in the restatement are each rejected by the per-block bar on the
    climb and on every ladder case; the first of them (H's lo residual dropped in the fp32 mode, a
    500-fold loss of accuracy) passes the operand bound of test_gpu_edge.test_jvp_running_max_moves.
"""
import functools

import pytest
import torch

import jvp_blocks as JB

from oracle import restate as R

FAMILIES = ("ladder", "lit", "climb")


def _cases(mode, family):
    """(name, primals, tangents, lit (shape, which, block) or None) of every case of a family."""
    if family == "ladder":
        for shape in JB.shapes(mode):
            xs = JB.ladder_inputs(shape)
            for t in JB.TERMS:
                yield f"{JB.shape_id(shape)}-{t}", xs[:3], JB.term(xs[3:], t), None
    elif family == "climb":
        xs = JB.climb_inputs()
        for t in JB.TERMS:
            yield f"climb-{t}", xs[:3], JB.term(xs[3:], t), None
    else:
        for shape in JB.shapes(mode, JB.LIT_SHAPES):
            prim = JB.lit_primals(shape)
            for which, blk in JB.lit_cases(shape):
                yield f"{JB.shape_id(shape)}-{which}{blk}", prim, JB.lit(shape, which, blk), (shape, which, blk)


@functools.lru_cache(maxsize=None)
def _full(mode, family):
    """[(name, inputs, truth)] of the all-terms cases (ladder, climb), computed once for the faults."""
    out = []
    for name, prim, tans, _ in _cases(mode, family):
        if name.endswith("-all"):
            xs = list(prim) + list(tans)
            out.append((name, xs, JB.truth(*xs, mode)))
    return out


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("mode", JB.MODES)
def test_restatement_within_a_third_of_the_bars(mode, family):
    bars = JB.BARS[(mode, family)]
    worst = [0.0, 0.0, 0.0]
    n = 0
    for name, prim, tans, lit in _cases(mode, family):
        got = JB.restate(*prim, *tans, mode)
        ref = JB.truth(*prim, *tans, mode)
        if lit is not None:
            JB.assert_lit_zeros(*lit, got[1], "restate")
            JB.assert_lit_zeros(*lit, ref[1], "truth")
        fig = JB.figures(got, ref)
        for i, what in enumerate(("tO block", "O block", "lse")):
            assert fig[i] <= bars[i] / 3, (mode, name, what, fig[i], bars[i] / 3)
        worst = [max(a, b) for a, b in zip(worst, fig[:3])]
        n += 1
    print(f"jvp-{mode}-{family}: {n} cases, worst tO block {worst[0]:.3e}, O block {worst[1]:.3e}, "
          f"lse {worst[2]:.3e}")
    assert n == {"ladder": 4 * len(JB.shapes(mode)), "climb": 4,
                 "lit": sum(len(JB.lit_cases(s)) for s in JB.shapes(mode, JB.LIT_SHAPES))}[family]
    for w, b in zip(worst, bars):
        assert w >= 0.8 * b / 3, (mode, family, w, b / 3)


@pytest.mark.parametrize("mode", JB.MODES)
def test_every_ladder_and_climb_case_moves_the_max(mode):
    for family in ("ladder", "climb"):
        for name, xs, _ in _full(mode, family):
            stats = {}
            JB.restate(*xs, mode, stats=stats)
            print(f"jvp-{mode} {name}: {stats['moved']} of {stats['pairs']} pairs move the running max")
            assert stats["pairs"] > 0 and stats["moved"] >= 1, (mode, name, stats)
    # the randn inputs of tests/test_gpu_jvp.py never move it after the first tile: the gap
    g = torch.Generator().manual_seed(7)
    xs = [torch.randn((2, 2, 256, 128), generator=g) for _ in range(6)]
    stats = {}
    JB.restate(*xs, mode, stats=stats)
    assert stats == {"pairs": 224, "moved": 0}


FAULTS = [("h_lo", "fp32")] + [(f, m) for f in ("tk_prev", "tv_cols", "racc_unscaled", "racc_neighbour")
                               for m in JB.MODES]


@pytest.mark.parametrize("fault,mode", FAULTS)
def test_planted_fault_fails_the_block_bar(fault, mode):
    for family in ("ladder", "climb"):
        bar = JB.BARS[(mode, family)][0]
        for name, xs, ref in _full(mode, family):
            healthy = JB.figures(JB.restate(*xs, mode), ref)[0]
            faulty = JB.figures(JB.restate(*xs, mode, fault=fault), ref)[0]
            print(f"jvp-{mode} {name} {fault}: worst tO block {faulty:.3e} (healthy {healthy:.3e}, bar {bar:.3e})")
            assert healthy <= bar / 3 and faulty > bar, (mode, name, fault, healthy, faulty, bar)


def test_dropped_h_lo_passes_the_operand_bound():
    """test_gpu_edge.test_jvp_running_max_moves, fp32 mode, on its own inputs, reference and bar:
    the restatement without H's lo residual is 0.34 from torch.func.jvp where max|tO| is 51, and the
    bar is 0.71."""
    q, k, v, tq, tk, tv = xs = JB.climb_inputs()
    _, tOt = R.jvp_truth(*xs)
    sm = q.shape[-1] ** -0.5
    s_max = (q.abs() @ k.abs().transpose(-1, -2)).max().item() * sm
    ts_max = ((tq @ k.transpose(-1, -2) + q @ tk.transpose(-1, -2)) * sm).abs().max().item()
    old_bar = 2.0 ** -16 * s_max * (tv.abs().max().item() + ts_max * v.abs().max().item())
    e_ok = (JB.restate(*xs, "fp32")[1] - tOt).abs().max().item()
    e_bad = (JB.restate(*xs, "fp32", fault="h_lo")[1] - tOt).abs().max().item()
    print(f"max-abs tO error: healthy {e_ok:.3g}, H lo dropped {e_bad:.3g}, operand bound {old_bar:.3g}")
    assert e_ok <= old_bar and e_bad <= old_bar
    assert e_bad > 100 * e_ok


def test_climb_inputs_are_the_edge_tests():
    import test_gpu_edge as E
    for a, b in zip(JB.climb_inputs()[:3], E._ramp_inputs((1, 2, 256, 128), 46, kscale=16.0)):
        assert torch.equal(a, b)
    B, Hq, Hkv, Sq, Sk, D = JB.CLIMB_SHAPE
    assert JB.climb_inputs()[0].shape == (B, Hq, Sq, D) and JB.climb_inputs()[4].shape == (B, Hkv, Sk, D)


def test_lit_tangents():
    shape = JB.LIT_SHAPES[0]
    for which, blk in JB.lit_cases(shape):
        tans = JB.lit(shape, which, blk)
        b, h, rows = JB.lit_block(shape, which, blk)
        for name, t in zip(JB.TERMS, tans):
            if name == which:
                assert (t[b, h, rows] != 0).all()
                assert int((t != 0).sum()) == 32 * shape[5]
            else:
                assert (t == 0).all()
    assert JB.lit_block(shape, "tq", 1)[:2] == (1, 5) and JB.lit_block(shape, "tv", 1)[:2] == (1, 2)
    z = JB.lit_zero_mask(shape, "tk", 0)
    assert int((~z).sum()) == 2 * shape[3] and not z[1, 4:].any()


def test_images_are_hi_plus_lo():
    x = torch.randn(4096, generator=torch.Generator().manual_seed(3))
    assert torch.equal(JB.images(x, "bf16"), x.bfloat16().double())
    hi = x.bfloat16().float()
    assert torch.equal(JB.images(x, "fp32"), hi.double() + (x - hi).bfloat16().double())
    assert ((JB.images(x, "fp32") - x.double()).abs() <= 2.0 ** -17 * x.abs().double()).all()
