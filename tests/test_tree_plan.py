"""The host side of speculative decoding on the paged MX-FP4 cache, pure Python: the ancestor words and
paths of a draft tree (kv_cache_mxfp4.tree_ancestor_masks, tree_path) with their refusals, plan_varlen with
tree lengths (the causal plan except seq_rec[j][7]) and PageAllocator.shrink (reference counts, the free
list, holes below the cut, all or nothing).
"""
import pytest

from quantizedattention_amd import _lib
from quantizedattention_amd.kv_cache_mxfp4 import (PageAllocator, _tree_args, plan_varlen, tree_ancestor_masks,
                                                   tree_path)


# ------------------------------------------------------------------ trees
def test_ancestor_masks_by_hand():
    assert tree_ancestor_masks([]) == []
    assert tree_ancestor_masks([-1]) == [1]
    assert tree_ancestor_masks([-1, 0, 1, 2]) == [0b1, 0b11, 0b111, 0b1111]                   # a chain
    assert tree_ancestor_masks([-1, 0, 0, 0]) == [0b1, 0b11, 0b101, 0b1001]                   # a star
    #        0
    #      1   2        5 (a second root)
    #     3 4           6
    assert tree_ancestor_masks([-1, 0, 0, 1, 1, -1, 5]) == [0b1, 0b11, 0b101, 0b1011, 0b10011, 0b100000,
                                                            0b1100000]
    chain = tree_ancestor_masks(list(range(-1, 63)))
    assert len(chain) == 64 and chain[63] == (1 << 64) - 1 and chain[31] == (1 << 32) - 1
    for t, w in enumerate(tree_ancestor_masks([-1, 0, 0, 2, 1, 3, 3, 0])):       # a subset of bits <= t with bit t
        assert w >> t == 1


def test_tree_path_by_hand():
    parents = [-1, 0, 0, 1, 1, -1, 5]
    assert tree_path(parents, 0) == [0] and tree_path(parents, 4) == [0, 1, 4]
    assert tree_path(parents, 2) == [0, 2] and tree_path(parents, 6) == [5, 6]
    assert tree_path(list(range(-1, 63)), 63) == list(range(64))
    for leaf in range(7):       # the path is the set bits of the leaf's word
        w = tree_ancestor_masks(parents)[leaf]
        assert tree_path(parents, leaf) == [b for b in range(7) if w >> b & 1]


@pytest.mark.parametrize("parents", [[0], [-1, 1], [-1, 0, 3, 0], [-2], [-1, 0, -5], list(range(-1, 64))])
def test_tree_refusals(parents):
    with pytest.raises(_lib.QAttnError, match="tree"):
        tree_ancestor_masks(parents)
    with pytest.raises(_lib.QAttnError, match="tree"):
        tree_path(parents, 0)


def test_tree_path_refuses_a_node_it_does_not_have():
    for leaf in (-1, 3):
        with pytest.raises(_lib.QAttnError, match="tree"):
            tree_path([-1, 0, 0], leaf)


def test_tree_args():
    """What the packed call makes of ``tree``: the lengths and one word per packed token as two int32 halves,
    zero outside a tree; None when no sequence has a tree; every refusal names "tree"."""
    assert _tree_args([None, None], [3, 1], True, None, False) is None
    assert _tree_args([None, []], [3, 1], True, None, False) is None
    nds, words = _tree_args([[-1, 0], None, [-1]], [3, 2, 1], True, None, False)
    words = words.tolist()
    assert nds == [2, 0, 1] and words == [0, 0, 1, 0, 3, 0] + [0] * 4 + [1, 0]
    nds, words = _tree_args([list(range(-1, 63))], [64], True, None, False)
    words = words.tolist()
    assert nds == [64] and words[2 * 31:2 * 31 + 2] == [-1, 0] and words[-2:] == [-1, -1]
    assert words[2 * 32:2 * 32 + 2] == [-1, 1]
    for bad in (lambda: _tree_args([None], [3], False, None, False),
                lambda: _tree_args([None], [3], True, 64, False),
                lambda: _tree_args([None], [3], True, None, True),
                lambda: _tree_args([None], [3, 1], True, None, False),
                lambda: _tree_args([[-1, 0, 1, 2]], [3], True, None, False),
                lambda: _tree_args([list(range(-1, 64))], [70], True, None, False),
                lambda: _tree_args([[-1, 1]], [3], True, None, False)):
        with pytest.raises(_lib.QAttnError, match="tree"):
            bad()


# ------------------------------------------------------------------ the plan
@pytest.mark.parametrize("kps", [64, 128, 1024])
def test_plan_with_trees_is_the_causal_plan_except_rec7(kps):
    lengths, ids, q_lens, Hq, Hkv = [64, 0, 70, 0, 130, 256], [4, 0, 5, 2], [3, 1, 64, 70], 4, 2
    want = plan_varlen(lengths, ids, q_lens, Hq, Hkv, kps, True)
    for nds in ([0, 0, 0, 0], [3, 1, 64, 64], [2, 0, 20, 1]):
        got = plan_varlen(lengths, ids, q_lens, Hq, Hkv, kps, True, tree_lens=nds)
        assert got[0] == want[0] and got[2:] == want[2:]
        assert [r[7] for r in got[1]] == nds and [r[7] for r in want[1]] == [0] * 4
        assert [r[:7] for r in got[1]] == [r[:7] for r in want[1]]


def test_plan_tree_refusals():
    lengths, ids, q_lens = [64, 0, 70, 0, 130, 256], [4, 0, 5, 2], [3, 1, 64, 70]
    for kw in (dict(causal=True, tree_lens=[4, 0, 0, 0]), dict(causal=True, tree_lens=[0, 0, 0, 65]),
               dict(causal=True, tree_lens=[0, -1, 0, 0]), dict(causal=True, tree_lens=[0, 0, 0]),
               dict(causal=False, tree_lens=[0, 0, 0, 0]),
               dict(causal=True, window=64, tree_lens=[0, 0, 0, 0])):
        with pytest.raises(_lib.QAttnError, match="tree"):
            plan_varlen(lengths, ids, q_lens, 4, 2, 64, **kw)


# ------------------------------------------------------------------ PageAllocator.shrink
def _state(a):
    return (list(a._free), list(a.refcount), [list(p) for p in a.pages], list(a.nholes), [list(r) for r in a.table])


def test_shrink_gives_back_what_reserve_took():
    a = PageAllocator(16, 64, 3, 8)
    a.reserve([(0, 130), (1, 64)])
    before = _state(a)
    a.reserve([(0, 400)])                                      # 3 -> 7 pages
    assert len(a.pages[0]) == 7 and a.free_pages == 16 - 8
    assert a.shrink(0, 3) == 4
    got = _state(a)
    assert got[:4] == before[:4]                               # the free list in its old order too
    assert got[4][0][:3] == before[4][0][:3]                   # the table below the cut
    a.reserve([(2, 256)])                                      # what a pool that never grew would hand out
    b = PageAllocator(16, 64, 3, 8)
    b.reserve([(0, 130), (1, 64)])
    b.reserve([(2, 256)])
    assert a.pages == b.pages and a._free == b._free
    assert a.shrink(0, 3) == 0 and a.shrink(1, 0) == 1 and a.pages[1] == [] and a.refcount[b.pages[1][0]] == 0


def test_shrink_and_shared_pages():
    a = PageAllocator(8, 64, 3, 6)
    a.reserve([(0, 256)])
    a.share(0, 1, 3, 1)                                        # three shared pages and one of its own
    shared, own = a.pages[1][:3], a.pages[1][3]
    assert a.shrink(1, 1) == 1                                 # its own page is free, two shared lose a reference
    assert a.refcount[own] == 0 and a._free[-1] == own
    assert [a.refcount[p] for p in shared] == [2, 1, 1] and a.pages[1] == shared[:1]
    assert a.pages[0][:3] == shared and a.shrink(0, 0) == 3    # page 0 is still sequence 1's
    assert a.refcount[shared[0]] == 1 and a.free_pages == 7


def test_shrink_keeps_the_holes_below_the_cut():
    a = PageAllocator(16, 64, 2, 10)
    a.reserve([(0, 640)])
    a.drop(0, 1, 4)
    a.drop(0, 6, 8)
    assert a.nholes[0] == 5 and a.free_pages == 6 + 5
    assert a.shrink(0, 7) == 2                                 # pages 8, 9 return; hole 7 is no longer counted
    assert a.holes(0) == [1, 2, 3, 6] and a.nholes[0] == 4 and len(a.pages[0]) == 7 and a.free_pages == 13
    assert a.shrink(0, 2) == 2 and a.holes(0) == [1] and a.nholes[0] == 1
    a.reserve([(0, 192)])                                      # grows on as before, behind the hole
    assert len(a.pages[0]) == 3 and a.pages[0][1] is None and a.pages[0][2] is not None


def test_shrink_is_all_or_nothing():
    a = PageAllocator(8, 64, 2, 4)
    a.reserve([(0, 130)])
    before = _state(a)
    for b, pages in ((0, 4), (0, -1), (2, 0), (-1, 0)):
        with pytest.raises(_lib.QAttnError):
            a.shrink(b, pages)
        assert _state(a) == before
