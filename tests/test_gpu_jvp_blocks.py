"""The forward-mode kernel's tangent, term by term and 32-row block by block (tests/jvp_blocks.py;
what the instrument sees is shown on the CPU in tests/test_jvp_blocks.py).

Every test runs in both modes through ``attention_jvp._jvp``.  tO and O are compared block by block
(grad_blocks.block_rel: no block left out, no floor under a denominator) and lse in absolute terms with
``torch.func.jvp`` in float64 on the same rounded inputs, under the bars of jvp_blocks.BARS: three
times the worst figure of the CPU restatement of the kernel over the family's cases.  The ladder and
the climb launch the three terms (tq, 0, 0), (0, tk, 0), (0, 0, tv) and their sum, so a wrong term
is named; the lit tangents hold every row, head and batch entry without a tangent to exactly zero
and go through the key blocks one launch at a time.  Every maximum is printed as
``RELL2-BLOCK jvp-<mode>-<term> <output> <value>`` (``-climb-`` / ``-lit-`` for the other families);
DESIGN.md §4 has the measured ones.
"""
import pytest
import torch

import jvp_blocks as JB

pytestmark = pytest.mark.gpu


def _run(mode, prim, tans):
    """One launch on the GPU -> (O, tO, lse) on the CPU."""
    from quantizedattention_amd.attention_jvp import _jvp
    dev = lambda t: JB.to_mode(t, mode).cuda()  # noqa: E731
    O, tO, lse = _jvp(*(dev(t) for t in prim), None if tans is None else tuple(dev(t) for t in tans))
    torch.cuda.synchronize()
    return O.cpu(), None if tO is None else tO.cpu(), lse.cpu()


def _terms(mode, xs, path, family):
    worst = [0.0, 0.0, 0.0]
    for t in JB.TERMS:
        tans = JB.term(xs[3:], t)
        got = _run(mode, xs[:3], tans)
        fig = JB.check(f"{path}-{t}", got, JB.truth(*xs[:3], *tans, mode), JB.BARS[(mode, family)])
        worst = [max(a, b) for a, b in zip(worst, fig)]
    return worst


def _ids(case):
    return f"{case[0]}-{JB.shape_id(case[1])}"


# (the 96-key shape runs in the fp32 mode only: the bf16 kernel stages 64 keys at a time)
LADDER_CASES = [(m, s) for m in JB.MODES for s in JB.shapes(m)]
LIT_CASES = [(m, s) for m in JB.MODES for s in JB.shapes(m, JB.LIT_SHAPES)]


@pytest.mark.parametrize("case", LADDER_CASES, ids=_ids)
def test_jvp_ladder_terms(lib, case):
    mode, shape = case
    _terms(mode, JB.ladder_inputs(shape), f"jvp-{mode}", "ladder")


@pytest.mark.parametrize("mode", JB.MODES)
def test_jvp_climb_terms(lib, mode):
    _terms(mode, JB.climb_inputs(), f"jvp-{mode}-climb", "climb")


@pytest.mark.parametrize("case", LIT_CASES, ids=_ids)
def test_jvp_lit_tangents(lib, case):
    """tq lit on one middle query block: tO exactly zero on every other row, head and batch entry.
    tk, then tv, lit on each 32-key block of the last key/value head in turn: tO exactly zero for every
    query head of the other key/value heads and batch entries, every query block of the lit group
    within the bar."""
    mode, shape = case
    prim = JB.lit_primals(shape)
    for which, blk in JB.lit_cases(shape):
        tans = JB.lit(shape, which, blk)
        got = _run(mode, prim, tans)
        JB.assert_lit_zeros(shape, which, blk, got[1], f"jvp-{mode}")
        JB.check(f"jvp-{mode}-lit-{which}{blk}", got, JB.truth(*prim, *tans, mode), JB.BARS[(mode, "lit")])


def _identity_inputs():
    yield "grouped", JB.ladder_inputs(JB.SHAPES[1])      # (2,6,3,96,320,64)
    yield "climb", JB.climb_inputs()
    yield "d128", JB.ladder_inputs(JB.SHAPES[2])         # (1,4,2,192,320,128)


@pytest.mark.parametrize("mode", JB.MODES)
def test_jvp_identities(lib, mode):
    """Read off the instruction sequence, no tolerance.  Zero tangents: tS = 0, so H, racc and both
    MFMA chains into AB are exact zeros.  (0, 0, tv): H = 0 again, AB = P tV runs the MFMAs of
    O = P V in the same order with tV for V and the H V chain adds exact zeros, and AB takes the
    same ``rs`` as O, so tO is the primal kernel's O on (q, k, tv).  Doubling the tangents doubles
    tS, H (before and after its rounding), racc and AB exactly."""
    for name, xs in _identity_inputs():
        prim, tans = xs[:3], xs[3:]
        zeros = [torch.zeros_like(t) for t in tans]
        O0, tO0, lse0 = _run(mode, prim, zeros)
        Op, _, lsep = _run(mode, prim, None)
        assert (tO0 == 0).all(), (mode, name)
        assert torch.equal(O0, Op) and torch.equal(lse0, lsep), (mode, name)
        tOv = _run(mode, prim, JB.term(tans, "tv"))[1]
        Ov = _run(mode, [prim[0], prim[1], tans[2]], None)[0]
        assert torch.equal(tOv, Ov), (mode, name, (tOv - Ov).abs().max().item())
        O1, tO1, lse1 = _run(mode, prim, tans)
        O2, tO2, lse2 = _run(mode, prim, [2 * t for t in tans])
        assert torch.isfinite(tO1).all() and (tO1 != 0).any()
        assert torch.equal(tO2, 2 * tO1), (mode, name, (tO2 - 2 * tO1).abs().max().item())
        assert torch.equal(O2, O1) and torch.equal(lse2, lse1) and torch.equal(O1, Op), (mode, name)
