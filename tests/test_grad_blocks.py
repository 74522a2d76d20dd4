"""What the block-wise gradient comparison (tests/grad_blocks.py) sees and a whole-tensor relL2 does
not (CPU, oracle only; the GPU side is tests/test_gpu_grad_blocks.py).

Three faults of the kind a backward kernel makes on an edge tile are planted, one at a time, into the
oracle's own int8 gradients of a ladder case:

  * 8 rows of one 32-row block scaled by 1.5 (the store-data hazard of DESIGN.md §4 moved 8 rows);
  * one block scaled as if it had been given its neighbour's block scale;
  * one (query tile, key tile) contribution missing from dk (the contribution itself is the oracle's
    result for a dO that is lit on that query tile only).

``block_rel`` must pass its bar on exactly the blocks the fault touches and read exactly 0 on every
other.  The same faults planted into a one-head 1024 x 1024 oracle run, on the 32-row block whose
gradient is the smallest of its head (where a ladder puts a fault a norm over the whole tensor cannot
see), stay under the whole-tensor bar: that is the gap.  Last, the exact zero pattern of a lit tile
holds in both restatements, causal and not.
"""
import pytest
import torch

import grad_blocks as GB
from conftest import INT8_BWD_REL, INT8_BWD_REL_FUZZ

from oracle import restate as R

BLOCK_BAR = 3 * INT8_BWD_REL


def test_block_bar_is_the_fuzz_bar():
    assert BLOCK_BAR == pytest.approx(INT8_BWD_REL_FUZZ)


def _int8_oracle(shape, seed):
    """Ladder inputs through the int8 restatement: (forward tuple, dO fp16, multipliers, grads)."""
    (q, k, v, dO), mult = GB.ladder_inputs(shape, "int8", seed)
    causal = shape[6]
    f = R.int8_fwd(q.half(), k.half(), v.half(), causal=causal)
    assert torch.isfinite(f[0].float()).all()
    dO = dO.half()
    return f, dO, mult, _int8_bwd(shape, f, dO)


def _int8_bwd(shape, f, dO):
    return R.int8_bwd(dO, f[2], f[5], f[3], None, f[6], f[4], f[7], f[0], f[1], causal=shape[6],
                      kv_heads=shape[2])


def _only(rel, where, bar):
    """The blocks past the bar are exactly ``where``; every other block reads exactly zero."""
    hit = {tuple(int(i) for i in idx) for idx in (rel > bar).nonzero()}
    assert hit == {where}, (hit, where)
    rest = rel.clone()
    rest[where] = 0
    assert (rest == 0).all()


def _scale_rows(x, b, h, rows, f):
    y = x.clone()
    y[b, h, rows] = (y[b, h, rows].float() * f).to(x.dtype)
    return y


@pytest.fixture(scope="module")
def small():
    return _int8_oracle(GB.SHAPES[1], seed=101)    # (2,6,3,160,288,64) causal


@pytest.fixture(scope="module")
def large():
    shape = (1, 1, 1, 1024, 1024, 64, False)
    f, dO, mult, grads = _int8_oracle(shape, seed=102)
    # the interior block of dq with the smallest norm: dq of a block scales with its dO multiplier
    norms = grads[0].float().reshape(32, -1).norm(dim=-1)
    t = 1 + int(norms[1:-1].argmin())
    lit = torch.zeros_like(dO)
    lit[0, 0, 32 * t:32 * t + 32] = dO[0, 0, 32 * t:32 * t + 32]
    return shape, dO, mult, grads, t, _int8_bwd(shape, f, lit)


def test_eight_rows_of_one_block(small, large):
    _, _, _, (dq, _, _) = small
    where = (1, 3, 2)
    bad = _scale_rows(dq, 1, 3, slice(64 + 8, 64 + 16), 1.5)
    rel = GB.block_rel(bad, dq)
    assert rel[where] > 0.2          # 0.5 * sqrt(8 / 32) of a block with even rows
    _only(rel, where, BLOCK_BAR)
    _, _, _, (dq, _, _), t, _ = large
    bad = _scale_rows(dq, 0, 0, slice(32 * t + 8, 32 * t + 16), 1.5)
    assert GB.block_rel(bad, dq)[0, 0, t] > BLOCK_BAR
    whole = GB.whole_rel(bad, dq)
    print(f"whole-tensor relL2 of 8 rows x 1.5 at 1024 x 1024: {whole:.5f}")
    assert whole < INT8_BWD_REL, whole


def test_neighbours_multiplier(small, large):
    """dq of a block is linear in that block's dO, so a dO block dequantised with the next block's
    scale shows as dq times the ratio of the two ladder multipliers (2x or more either way)."""
    _, _, mult, (dq, _, _) = small
    where = (1, 3, 2)
    m = mult[3][1, 3, ::32, 0]
    bad = _scale_rows(dq, 1, 3, slice(64, 96), float(m[3] / m[2]))
    rel = GB.block_rel(bad, dq)
    assert rel[where] >= 0.49
    _only(rel, where, BLOCK_BAR)
    _, _, mult, (dq, _, _), t, _ = large
    m = mult[3][0, 0, ::32, 0]
    bad = _scale_rows(dq, 0, 0, slice(32 * t, 32 * t + 32), float(m[t + 1] / m[t]))
    assert GB.block_rel(bad, dq)[0, 0, t] >= 0.49
    whole = GB.whole_rel(bad, dq)
    print(f"whole-tensor relL2 of a block with its neighbour's multiplier at 1024 x 1024: {whole:.5f}")
    assert whole < INT8_BWD_REL, whole


def test_one_pair_missing_from_dk(small, large):
    shape = GB.SHAPES[1]
    f, dO, _, (_, dk, _) = small
    b, h, t = GB.lit_tile(shape)
    pair = _int8_bwd(shape, f, GB.lit_dO(shape, 0, like=dO).half())[1]
    kvh, kt = h // (shape[1] // shape[2]), 1        # a key tile the causal query tile t = 2 sees whole
    rows = slice(32 * kt, 32 * kt + 32)
    bad = dk.clone()
    bad[b, kvh, rows] = (dk[b, kvh, rows].float() - pair[b, kvh, rows].float()).half()
    rel = GB.block_rel(bad, dk)
    _only(rel, (b, kvh, kt), BLOCK_BAR)
    shape, dO, _, (_, dk, _), t, (_, pair, _) = large
    rows = slice(512, 544)
    bad = dk.clone()
    bad[0, 0, rows] = (dk[0, 0, rows].float() - pair[0, 0, rows].float()).half()
    assert (bad != dk).any()
    whole = GB.whole_rel(bad, dk)
    print(f"whole-tensor relL2 of one missing pair at 1024 x 1024: {whole:.5f} "
          f"(its block: {GB.block_rel(bad, dk)[0, 0, 16].item():.5f})")
    assert whole < INT8_BWD_REL, whole


def test_block_rel_zero_blocks():
    """A block the oracle has exactly zero is not divided: -0 passes, anything else is inf."""
    ref = torch.zeros((1, 1, 64, 4))
    ref[0, 0, 32:] = 1.0
    a = ref.clone()
    a[0, 0, 3, 1] = -0.0
    assert (GB.block_rel(a, ref) == 0).all()
    a[0, 0, 3, 1] = 1e-30
    rel = GB.block_rel(a, ref)
    assert torch.isinf(rel[0, 0, 0]) and rel[0, 0, 1] == 0


def test_ladder_steps():
    g = torch.Generator().manual_seed(0)
    for choices in (GB.QK_INT8, GB.V_DO):
        m = GB.ladder(2, 3, 320, choices, g)[..., ::32, 0]
        step = torch.maximum(m[..., 1:] / m[..., :-1], m[..., :-1] / m[..., 1:])
        assert (step >= 2).all() and set(m.flatten().tolist()) == set(choices)


@pytest.mark.parametrize("shape", GB.SHAPES, ids=GB.shape_id)
def test_lit_tile_zero_pattern_int8(shape):
    q, k, v = (t.half() for t in GB.randn_inputs(shape, 111))
    f = R.int8_fwd(q, k, v, causal=shape[6])
    dq, dk, dv = _int8_bwd(shape, f, GB.lit_dO(shape, 112).half())
    GB.assert_lit_zeros(shape, dq, dk, dv, "R.int8_bwd")


@pytest.mark.parametrize("shape", GB.SHAPES, ids=GB.shape_id)
def test_lit_tile_zero_pattern_bf16(shape):
    """(The causal bf16 restatement with its denormal results read as zero: its masked P is
    exp2(-128 - lse), an fp32 denormal that a GPU's exp2 returns as 0; grad_blocks.flush_denormals.)"""
    q, k, v = GB.randn_inputs(shape, 113)
    q, k, v = q.half(), k.half(), v.bfloat16()
    causal = shape[6]
    O, lse = R.bf16_fwd(q, k, v, causal, kt=16)
    assert torch.isfinite(O).all()
    dO = GB.lit_dO(shape, 114)
    dq, dk, dv = GB.flush_denormals(*R.bf16_bwd(q, k, v, O, lse, causal, dO))
    GB.assert_lit_zeros(shape, dq, dk, dv, "R.bf16_bwd")
    if causal:   # what it flushed past the lit tile were denormals only
        _, zk = GB.lit_zero_masks(shape)
        for x in R.bf16_bwd(q, k, v, O, lse, causal, dO)[1:]:
            assert x[zk].abs().max().item() < 2.0 ** -126
