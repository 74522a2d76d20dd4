"""The tree-masked restatement (tests/mxfp4_tree_ref.py) on the CPU: a chain tree IS the ragged causal
restatement (torch.equal on O, lse, m and l); rows whose mask row is the causal row keep the causal
restatement's bits whatever their neighbours see; against float64 softmax attention with the same mask on
the dequantised operands it keeps the bar of tests/test_mxfp4_window_ref.py (cosine >= 0.95); and the trees
the GPU tests use move lse far enough for a wrong mask to be seen.  The words are those the product makes
(kv_cache_mxfp4.tree_ancestor_masks), which the restatement's own ``ancestors`` must equal.
tests/test_gpu_mxfp4_tree.py pins the kernel to this restatement.
"""
import pytest
import torch

import mxfp4_masked_ref as MR
import mxfp4_ragged_ref as RR
import mxfp4_tree_ref as TR
from quantizedattention_amd.kv_cache_mxfp4 import tree_ancestor_masks

SHAPES = [(1, 64, 64), (3, 130, 128), (33, 256, 64), (64, 70, 64), (64, 64, 64)]     # (n, L, kps)
SENSITIVE = [(64, 70), (33, 40), (64, 200)]                                           # (n, L)


def test_the_product_makes_the_restatements_words():
    for nd in (1, 2, 5, 33, 64):
        for parents in [TR.chain(nd)] + [f(nd) for f in TR.TREES.values()]:
            assert tree_ancestor_masks(parents) == TR.ancestors(parents)


def _sequence(Hq, Hkv, Sq, L, seed=2):
    q, ks, vs = RR.inputs(1, Hq, Hkv, Sq, (L,), seed=seed)
    return q, ks[0], vs[0]


@pytest.mark.parametrize("n,L,kps", SHAPES)
def test_chain_is_the_ragged_causal_restatement(n, L, kps):
    q, k, v = _sequence(4, 2, n, L)
    RO, Rl, (Rm, Rll) = RR.mxfp4_fwd_ragged(q, [k], [v], True, kps)
    for nd in sorted({0, 1, n // 2, n}):
        O, lse, (m, l) = TR.mxfp4_fwd_tree(q, k, v, nd, tree_ancestor_masks(TR.chain(nd)), kps)
        assert torch.equal(O, RO) and torch.equal(lse, Rl), nd
        assert torch.equal(m, Rm) and torch.equal(l, Rll), nd


@pytest.mark.parametrize("n,L,kps", SHAPES[2:])
def test_causal_rows_stay_causal(n, L, kps):
    """Two branches: a chain from node 0 and a second branch off the chain's second-to-last node.  The
    chain's rows (and the rows before the tree) have the causal row as their mask row."""
    q, k, v = _sequence(4, 2, n, L)
    RO, Rl, _ = RR.mxfp4_fwd_ragged(q, [k], [v], True, kps)
    nd = n - 1
    first = (nd + 1) // 2
    parents = TR.chain(first) + [max(first - 2, 0)] + list(range(first, nd - 1))
    masks = tree_ancestor_masks(parents)
    O, lse, _ = TR.mxfp4_fwd_tree(q, k, v, nd, masks, kps)
    vis, causal = TR.visible(n, L, nd, masks), RR.visible(n, L, RR.ceil64(L), True)
    same = (vis == causal).all(1)
    assert same[:n - nd + first].all() and not same[n - nd + first:].any()
    assert torch.equal(O[:, :, same], RO[:, :, same]) and torch.equal(lse[:, same], Rl[:, same])
    assert not torch.equal(lse[:, ~same], Rl[:, ~same])


@pytest.mark.parametrize("tree", sorted(TR.TREES))
def test_definition_accuracy(tree):
    for n, L, kps in SHAPES + [(5, 5, 64)]:
        nd = n
        masks = tree_ancestor_masks(TR.TREES[tree](nd))
        q, k, v = _sequence(4, 2, n, L)
        O, lse, _ = TR.mxfp4_fwd_tree(q, k, v, nd, masks, kps)
        RO, Rl = TR.dense_reference(q, k, v, nd, masks)
        cos = MR.cosine(O, RO)
        print(f"MXFP4-TREE-DEF {tree} n={n} L={L} cos {cos:.4f} "
              f"lse err {(lse.double() - Rl).abs().max().item():.4f}")
        assert torch.isfinite(lse).all() and torch.isfinite(O.float()).all()
        assert cos >= 0.95, cos


@pytest.mark.parametrize("n,L", SENSITIVE)
@pytest.mark.parametrize("tree", sorted(TR.TREES))
def test_sensitivity(tree, n, L):
    """The restatement alone sees a wrong mask on the shapes the GPU test uses: a non-chain tree moves lse by
    more than 0.5 against the causal restatement, and clearing the last node's parent bit moves it by at
    least 1e-2, a hundred times the GPU bar on lse."""
    parents = TR.TREES[tree](n)
    masks = tree_ancestor_masks(parents)
    q, k, v = _sequence(4, 2, n, L)
    _, lse, _ = TR.mxfp4_fwd_tree(q, k, v, n, masks, 64)
    _, Rl, _ = RR.mxfp4_fwd_ragged(q, [k], [v], True, 64)
    d_causal = (lse - Rl).abs().max().item()
    assert parents[-1] >= 0
    wrong = masks[:-1] + [masks[-1] & ~(1 << parents[-1])]
    _, lse2, _ = TR.mxfp4_fwd_tree(q, k, v, n, wrong, 64)
    d_bit = (lse2 - lse).abs().max().item()
    print(f"MXFP4-TREE-SENS {tree} n={n} L={L}: against causal {d_causal:.3f}, parent bit cleared {d_bit:.3e}")
    assert d_causal > 0.5 and d_bit >= 1e-2, (d_causal, d_bit)
