"""Tree-masked verify attention over the paged MX-FP4 cache on the GPU:
attention_mxfp4_varlen_paged(tree=) (qattn_mxfp4_attn_fwd_varlen_paged_tree + qattn_mxfp4_varlen_combine) and
torch.ops.qattn.mxfp4_varlen_paged_tree.

torch.equal wherever an exact instrument exists: a chain tree is the causal call; a row whose mask row is the
causal row keeps the causal call's bits whatever its neighbours see; order, company and the page size change
no bit; a word with its self bit cleared or bits above the diagonal gives the bits of the cleaned word.  The
general trees are held to the CPU restatement tests/mxfp4_tree_ref.py within the bars of
tests/test_gpu_mxfp4_ragged.py (O max-abs <= 2e-2, lse <= 1e-4, relL2 <= 2e-3), on shapes where
tests/test_mxfp4_tree_ref.py shows that the mask moves lse by a hundred times that bar.  Pools are handed out
in mxfp4_varlen_helpers.scatter order and two slots stay empty.
"""
import functools

import pytest
import torch

import mxfp4_tree_ref as TR
import mxfp4_varlen_helpers as H

pytestmark = pytest.mark.gpu

HEADS = [(4, 2), (4, 4)]
POOLS = [(64, 32), (256, 48)]     # (page tokens, pages)
LENGTHS = H.LENGTHS[1]            # (64, 130, 256, 70)
Q_LENS = (1, 3, 33, 64)
SENS_LENGTHS, SENS_Q, SENS_ND = (70, 40, 200), (64, 33, 64), (64, 33, 64)


def _call(q, cache, ids, q_lens, kps, tree):
    from quantizedattention_amd.kv_cache_mxfp4 import attention_mxfp4_varlen_paged
    O, lse = attention_mxfp4_varlen_paged(q, cache, ids, q_lens, causal=True, keys_per_split=kps, tree=tree)
    assert O.shape == q.shape and O.dtype == torch.float16 and lse.shape == q.shape[:2]
    assert lse.dtype == torch.float32
    assert torch.isfinite(O.float()).all() and torch.isfinite(lse).all()
    return O, lse


@functools.lru_cache(maxsize=None)
def _pool(Hkv, lengths, P, pages):
    """Shared; do not modify."""
    if len(lengths) == len(H.SLOTS):
        return H.pool(Hkv, lengths, P, pages)
    return H.fill_pool(Hkv, lengths, P, pages, slots=H.SLOTS[:len(lengths)])


def _causal_rows(lengths, q_lens, trees):
    """bool [T]: the packed tokens whose mask row is the causal row."""
    rows = []
    for L, n, p in zip(lengths, q_lens, trees):
        nd = 0 if p is None else len(p)
        vis = TR.visible(n, L, nd, TR.ancestors(p or []))
        rows.append((vis == TR.RR.visible(n, L, vis.shape[1], True)).all(1))
    return torch.cat(rows)


def _two_branch(nd):
    """A chain of ``first`` nodes from node 0, then a second branch off the chain's second-to-last node."""
    first = (nd + 1) // 2
    return TR.chain(first) + [first - 2] + list(range(first, nd - 1)), first


# ------------------------------------------------------------------ 1. a chain is the causal call
@pytest.mark.parametrize("kps", [64, 128, None])
@pytest.mark.parametrize("P,pages", POOLS)
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_chain_is_causal(lib, Hq, Hkv, P, pages, kps):
    cache, q = H.pool(Hkv, LENGTHS, P, pages), H.packed_q(Hq, Q_LENS)
    RO, Rl = _call(q, cache, H.SLOTS, Q_LENS, kps, None)
    for trees in ([TR.chain(n) for n in Q_LENS], [TR.chain(1), None, TR.chain(20), TR.chain(63)]):
        O, lse = _call(q, cache, H.SLOTS, Q_LENS, kps, trees)
        assert torch.equal(O, RO) and torch.equal(lse, Rl)


# ------------------------------------------------------------------ 2, 3. causal rows keep the causal bits
@pytest.mark.parametrize("kps", [64, 128])
@pytest.mark.parametrize("P,pages", POOLS)
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_causal_rows_stay_causal(lib, Hq, Hkv, P, pages, kps):
    """None beside trees, a tree-less sequence of 70 query tokens, a tree on the last 20 of 33 tokens, and a
    two-branch tree whose first branch is a chain."""
    cache = H.pool(Hkv, LENGTHS, P, pages)
    two, first = _two_branch(64)
    for q_lens, trees in ((H.Q_LENS, [None, TR.star(3), TR.heap(20), None]),
                          (H.Q_LENS, [TR.star(1), None, TR.rand_tree(33), None]),
                          (Q_LENS, [None, None, _two_branch(33)[0], two])):
        q = H.packed_q(Hq, q_lens)
        RO, Rl = _call(q, cache, H.SLOTS, q_lens, kps, None)
        O, lse = _call(q, cache, H.SLOTS, q_lens, kps, trees)
        same = _causal_rows(LENGTHS, q_lens, trees).cuda()
        assert same.any() and not same.all()
        assert torch.equal(O[same], RO[same]) and torch.equal(lse[same], Rl[same])
        assert not torch.equal(lse[~same], Rl[~same])           # and the other rows moved
    assert same[-64:-64 + first].all() and not same[-64 + first:].any()     # the first branch, the second


# ------------------------------------------------------------------ 4. general trees: the restatement
@functools.lru_cache(maxsize=None)
def _restated(Hq, Hkv, lengths, q_lens, j, tree, nd, kps):
    k, v = H.tokens(Hkv, lengths)[j]
    q = H.per_sequence(H.packed_q(Hq, q_lens), q_lens, j)
    masks = TR.ancestors(TR.TREES[tree](nd)) if nd else []
    O, lse, _ = TR.mxfp4_fwd_tree(q.cpu(), k[None].cpu(), v[None].cpu(), nd, masks, kps)
    return O, lse


@pytest.mark.parametrize("kps", [64, 128])
@pytest.mark.parametrize("tree", sorted(TR.TREES))
@pytest.mark.parametrize("lengths,q_lens,nds", [(LENGTHS, Q_LENS, Q_LENS), (SENS_LENGTHS, SENS_Q, SENS_ND),
                                                (LENGTHS, H.Q_LENS, (0, 2, 20, 64))])
def test_trees_against_the_restatement(lib, lengths, q_lens, nds, tree, kps):
    Hq, Hkv = 4, 2
    ids = H.SLOTS[:len(lengths)]
    trees = [TR.TREES[tree](nd) if nd else None for nd in nds]
    cache, q = _pool(Hkv, lengths, 64, 32), H.packed_q(Hq, q_lens)
    O, lse = _call(q, cache, ids, q_lens, kps, trees)
    for P, pages in POOLS[1:]:      # the page size changes no bit
        O2, lse2 = _call(q, _pool(Hkv, lengths, P, pages), ids, q_lens, kps, trees)
        assert torch.equal(O, O2) and torch.equal(lse, lse2)
    for j in range(len(ids)):
        RO, Rl = _restated(Hq, Hkv, lengths, q_lens, j, tree, nds[j], kps)
        Oj, lj = H.per_sequence(O, q_lens, j).cpu(), H.per_sequence(lse, q_lens, j)[0].cpu()
        err = (Oj.float() - RO.float()).abs().max().item()
        lerr = (lj - Rl).abs().max().item()
        rel = ((Oj.float() - RO.float()).norm() / RO.float().norm()).item()
        print(f"MXFP4-TREE {tree} L={lengths[j]} n={q_lens[j]} nd={nds[j]} kps={kps}: O {err:.3e} lse {lerr:.3e} "
              f"relL2 {rel:.3e}")
        assert err <= 2e-2 and lerr <= 1e-4 and rel <= 2e-3, (j, err, lerr, rel)


# ------------------------------------------------------------------ 5. order and company
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_reversed_and_alone(lib, Hq, Hkv):
    cache, q = H.pool(Hkv, LENGTHS, 64, 32), H.packed_q(Hq, Q_LENS)
    trees = [TR.star(1), None, TR.heap(20), TR.rand_tree(64)]
    O, lse = _call(q, cache, H.SLOTS, Q_LENS, 64, trees)
    n = len(H.SLOTS)
    qs = [H.per_sequence(q, Q_LENS, j)[0].transpose(0, 1) for j in range(n)]        # [n_j, Hq, D]
    rev = list(range(n))[::-1]
    rq, rlens = torch.cat([qs[j] for j in rev]), [Q_LENS[j] for j in rev]
    RO, Rl = _call(rq, cache, [H.SLOTS[j] for j in rev], rlens, 64, [trees[j] for j in rev])
    for pos, j in enumerate(rev):
        want = (H.per_sequence(O, Q_LENS, j), H.per_sequence(lse, Q_LENS, j)[0])
        H.assert_sequence_equals(RO, Rl, rlens, pos, want)
        AO, Al = _call(qs[j].contiguous(), cache, [H.SLOTS[j]], [Q_LENS[j]], 64, [trees[j]])
        H.assert_sequence_equals(AO, Al, [Q_LENS[j]], 0, want)


# ------------------------------------------------------------------ 6. the C entry on flat buffers
def test_nothing_is_written_past_the_buffers(lib):
    """The tree entry and the merge on flat buffers with 128 sentinel rows behind opart, ml, O and lse: every
    partial row is written, nothing past the end; the refused argument sets return 1 and write nothing; words
    with the self bit cleared and bits set above the diagonal give the bits of the cleaned words."""
    from quantizedattention_amd import _lib
    from quantizedattention_amd.attention_mxfp4 import _qk_scale, mxfp4_quantize_rows
    from quantizedattention_amd.kv_cache_mxfp4 import plan_varlen, tree_ancestor_masks
    SENT, D, pad = -12288.0, 128, 128
    Hq, Hkv = 4, 2
    cache, q = H.pool(Hkv, LENGTHS, 64, 32), H.packed_q(Hq, Q_LENS)
    T = q.shape[0]
    trees = [TR.star(1), TR.heap(2), TR.rand_tree(33), TR.forest(64)]
    nds = [len(p) for p in trees]
    kps, rec, work, rows = plan_varlen(cache.lengths, H.SLOTS, Q_LENS, Hq, Hkv, 64, True, tree_lens=nds)
    assert [r[7] for r in rec] == nds
    clean, dirty = [], []
    for n, p in zip(Q_LENS, trees):
        anc = tree_ancestor_masks(p)
        clean += [0] * (n - len(p)) + anc
        # the self bit cleared, every bit above the diagonal set; the words outside a tree are never read
        dirty += [5] * (n - len(p)) + [w & ~(1 << t) | (-1 << t + 1) & (1 << 64) - 1 for t, w in enumerate(anc)]
    assert clean != dirty
    signed = lambda ws: torch.tensor([w - (1 << 64) if w >> 63 else w for w in ws], dtype=torch.int64).cuda()  # noqa: E731
    rec_d, work_d = (torch.tensor(t, dtype=torch.int32).cuda() for t in (rec, work))
    q4, qs = mxfp4_quantize_rows(q)
    st = _lib.stream_of(q)
    lib_ = _lib.load()
    results = []
    for words in (clean, dirty):
        masks = signed(words)
        opart = torch.full(((rows + pad) * D,), SENT, dtype=torch.float32, device="cuda")
        ml = torch.full(((rows + pad) * 2,), SENT, dtype=torch.float32, device="cuda")
        out = torch.full(((T * Hq + pad) * D,), SENT, dtype=torch.float16, device="cuda")
        lse = torch.full((T * Hq + pad,), SENT, dtype=torch.float32, device="cuda")
        args = (_lib.ptr(q4), _lib.ptr(qs), *(_lib.ptr(t) for t in cache.kv), _lib.ptr(opart), _lib.ptr(ml),
                _lib.ptr(cache.lens), _lib.ptr(cache.block_table), _lib.ptr(rec_d), _lib.ptr(work_d), len(rec),
                len(work), T, rows, H.MAX_SEQS, Hkv, Hq // Hkv, cache.num_pages, 64,
                cache.alloc.max_pages_per_seq)
        for causal, m in ((0, _lib.ptr(masks)), (1, _lib.ptr(masks)), (2, None)):     # refused: status 1
            assert lib_.qattn_mxfp4_attn_fwd_varlen_paged_tree(*args, causal, kps, D, _qk_scale(D), m, st) == 1
        torch.cuda.synchronize()
        assert (opart == SENT).all() and (ml == SENT).all()
        _lib.call("qattn_mxfp4_attn_fwd_varlen_paged_tree", *args, 2, kps, D, _qk_scale(D), _lib.ptr(masks), st)
        torch.cuda.synchronize()
        for t in (opart[rows * D:], ml[rows * 2:], out, lse):
            assert t.numel() >= 128 and (t == SENT).all()
        assert not (opart[:rows * D] == SENT).any() and not (ml[:rows * 2] == SENT).any()
        _lib.call("qattn_mxfp4_varlen_combine", _lib.ptr(opart), _lib.ptr(ml), _lib.ptr(out), _lib.ptr(lse),
                  _lib.ptr(rec_d), len(rec), T, Hq, Hkv, rows, D, st)
        torch.cuda.synchronize()
        for t in (opart[rows * D:], ml[rows * 2:], out[T * Hq * D:], lse[T * Hq:]):
            assert t.numel() >= 128 and (t == SENT).all()
        results.append((out[:T * Hq * D].view(T, Hq, D), lse[:T * Hq].view(T, Hq), opart[:rows * D],
                        ml[:rows * 2]))
    O, l2 = _call(q, cache, H.SLOTS, Q_LENS, 64, trees)
    for out, lse, _, _ in results:
        assert torch.equal(out, O) and torch.equal(lse, l2)
    assert torch.equal(results[0][2], results[1][2]) and torch.equal(results[0][3], results[1][3])


# ------------------------------------------------------------------ 7. the operator, the Python refusals
def test_operator_equals_the_python_call(lib):
    import quantizedattention_amd.ops as ops
    from quantizedattention_amd.kv_cache_mxfp4 import plan_varlen, tree_ancestor_masks
    Hq, Hkv = 4, 2
    cache, q = H.pool(Hkv, LENGTHS, 64, 32), H.packed_q(Hq, Q_LENS)
    trees = [None, TR.star(3), TR.heap(20), TR.rand_tree(64)]
    nds = [len(p or []) for p in trees]
    words = [w for n, p in zip(Q_LENS, trees) for w in [0] * (n - len(p or [])) + tree_ancestor_masks(p or [])]
    masks = torch.tensor([w - (1 << 64) if w >> 63 else w for w in words], dtype=torch.int64).cuda()
    for split in (128, None):
        O, lse = _call(q, cache, H.SLOTS, Q_LENS, split, trees)
        O1, l1 = ops.mxfp4_varlen_paged(q, cache, H.SLOTS, Q_LENS, causal=True, keys_per_split=split, tree=trees)
        assert torch.equal(O, O1) and torch.equal(lse, l1)
        kps, rec, work, rows = plan_varlen(cache.lengths, H.SLOTS, Q_LENS, Hq, Hkv, split, True, tree_lens=nds)
        args = (q, *cache.kv, cache.lens, cache.block_table, torch.tensor(rec, dtype=torch.int32).cuda(),
                torch.tensor(work, dtype=torch.int32).cuda(), masks, rows, 1, kps)
        O2, l2 = torch.ops.qattn.mxfp4_varlen_paged_tree(*args)
        assert O2.dtype == torch.float16 and l2.dtype == torch.float32
        assert torch.equal(O, O2) and torch.equal(lse, l2)
    RO, Rl = _call(q, cache, H.SLOTS, Q_LENS, None, None)           # every entry None: the plain causal call
    O3, l3 = ops.mxfp4_varlen_paged(q, cache, H.SLOTS, Q_LENS, causal=True, tree=[None] * 4)
    assert torch.equal(O3, RO) and torch.equal(l3, Rl)
    op = torch.ops.qattn.mxfp4_varlen_paged_tree
    torch.library.opcheck(op, args, test_utils="test_faketensor")
    for bad in ((*args[:11], 0, args[12]), (*args[:9], masks[:-1], *args[10:]), (*args[:9], masks.int(), *args[10:]),
                (*args[:12], 96), (q[:, :3], *args[1:])):
        with pytest.raises(RuntimeError):
            op(*bad)


def test_python_refusals_leave_the_pool_untouched(lib):
    import quantizedattention_amd.ops as ops
    from quantizedattention_amd import _lib
    from quantizedattention_amd.kv_cache_mxfp4 import attention_mxfp4_varlen_paged
    Hq, Hkv = 4, 2
    cache, q = H.fill_pool(Hkv, LENGTHS, 64, 32), H.packed_q(Hq, H.Q_LENS)
    a = cache.alloc
    dev = [t.clone() for t in (*cache.kv, cache.vtail, cache.lens, cache.block_table)]
    host = (list(cache.lengths), list(a._free), list(a.refcount), [list(p) for p in a.pages],
            [list(r) for r in a.table])

    def unchanged():
        torch.cuda.synchronize()
        assert host == (list(cache.lengths), list(a._free), list(a.refcount), [list(p) for p in a.pages],
                        [list(r) for r in a.table])
        for x, y in zip(dev, (*cache.kv, cache.vtail, cache.lens, cache.block_table)):
            assert torch.equal(x, y)

    trees = [None, TR.star(3), TR.heap(20), TR.chain(64)]
    for fn in (attention_mxfp4_varlen_paged, ops.mxfp4_varlen_paged):
        for kw in (dict(causal=True, window=64, tree=trees), dict(causal=True, share_prefix=True, tree=trees),
                   dict(causal=False, tree=trees), dict(causal=False, tree=[None] * 4),
                   dict(causal=True, tree=[None, TR.star(4), None, None]),           # nd > n
                   dict(causal=True, tree=[None, None, None, TR.chain(65)]),         # nd > 64
                   dict(causal=True, tree=trees[:3]), dict(causal=True, tree=[None, [-1, 1], None, None])):
            with pytest.raises(_lib.QAttnError, match="tree"):
                fn(q, cache, H.SLOTS, H.Q_LENS, **kw)
            unchanged()
