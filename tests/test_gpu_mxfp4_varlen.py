"""The packed (varlen) step over the paged MX-FP4 cache on the GPU: attention_mxfp4_varlen_paged
(qattn_mxfp4_attn_fwd_varlen_paged + qattn_mxfp4_varlen_combine), PagedKVFP4.append_packed
(qattn_mxfp4_paged_append_packed) and torch.ops.qattn.mxfp4_varlen_paged.

One criterion throughout, torch.equal: for every listed sequence the packed outputs equal
attention_mxfp4_decode on a batch-1 PreallocatedKVFP4 fed the same tokens, with Sq = q_lens[j], the same
causal flag and the same keys per split (mxfp4_varlen_helpers.reference); that entry is held to its CPU
restatement in tests/test_gpu_mxfp4_ragged.py.  With keys_per_split None the reference is given the
one value the plan chose for the call (the preallocated entry would otherwise plan per batch).  Pools
are handed out in a scattered order and two of the six slots stay empty.
"""
import pytest
import torch

import mxfp4_varlen_helpers as H

pytestmark = pytest.mark.gpu

HEADS = [(4, 2), (4, 4)]
POOLS = [(64, 32), (256, 48)]     # (page tokens, pages)


def _varlen(q, cache, ids, q_lens, causal, kps):
    from quantizedattention_amd.kv_cache_mxfp4 import attention_mxfp4_varlen_paged
    O, lse = attention_mxfp4_varlen_paged(q, cache, ids, q_lens, causal=causal, keys_per_split=kps)
    assert O.shape == q.shape and O.dtype == torch.float16 and lse.shape == q.shape[:2]
    assert torch.isfinite(O.float()).all() and torch.isfinite(lse).all()
    return O, lse


def _plan_kps(cache, ids, q_lens, Hq, kps):
    from quantizedattention_amd.kv_cache_mxfp4 import plan_varlen
    return plan_varlen(cache.lengths, ids, q_lens, Hq, cache.k4.shape[1], kps)[0]


# ------------------------------------------------------------------ 1. every sequence = its run alone
@pytest.mark.parametrize("kps", [64, 128, None])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("lengths", H.LENGTHS)
@pytest.mark.parametrize("P,pages", POOLS)
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_every_sequence_equals_its_run_alone(lib, Hq, Hkv, P, pages, lengths, causal, kps):
    """ns_j differ within one call (64 keys per split: 1, 1, 2 and 4 splits), a 140-row virtual head
    crosses a row block and a wave crosses a head boundary, a 2-row one leaves a wave nearly empty."""
    cache, q = H.pool(Hkv, lengths, P, pages), H.packed_q(Hq)
    O, lse = _varlen(q, cache, H.SLOTS, H.Q_LENS, causal, kps)
    ref_kps = _plan_kps(cache, H.SLOTS, H.Q_LENS, Hq, kps)
    if kps is not None:
        assert ref_kps == kps
    for j in range(len(H.SLOTS)):
        H.assert_sequence_equals(O, lse, H.Q_LENS, j, H.reference(Hq, Hkv, lengths, j, causal, ref_kps))


# ------------------------------------------------------------------ 2. order and company do not matter
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_reversed_and_alone(lib, Hq, Hkv, causal):
    lengths = H.LENGTHS[1]
    cache, q = H.pool(Hkv, lengths, 64, 32), H.packed_q(Hq)
    n = len(H.SLOTS)
    qs = [H.per_sequence(q, H.Q_LENS, j)[0].transpose(0, 1) for j in range(n)]        # [n_j, Hq, D]
    rev = list(range(n))[::-1]
    rq, rlens = torch.cat([qs[j] for j in rev]), [H.Q_LENS[j] for j in rev]
    RO, Rl = _varlen(rq, cache, [H.SLOTS[j] for j in rev], rlens, causal, 64)
    for pos, j in enumerate(rev):
        want = H.reference(Hq, Hkv, lengths, j, causal, 64)
        H.assert_sequence_equals(RO, Rl, rlens, pos, want)
        AO, Al = _varlen(qs[j].contiguous(), cache, [H.SLOTS[j]], [H.Q_LENS[j]], causal, 64)
        H.assert_sequence_equals(AO, Al, [H.Q_LENS[j]], 0, want)


# ------------------------------------------------------------------ 3. unlisted slots are never read
@pytest.mark.parametrize("P,pages", POOLS)
def test_unlisted_slots_may_hold_anything(lib, P, pages):
    """Garbage in the device lengths and table rows of the slots that are not listed (the kernels clamp
    pages into the pool, so a read of them would show as a wrong answer, not a fault), and a listed
    subset that leaves a FILLED slot out: nothing moves by a bit."""
    Hq, Hkv, lengths = 4, 2, H.LENGTHS[0]
    cache, q = H.fill_pool(Hkv, lengths, P, pages), H.packed_q(Hq)
    O, lse = _varlen(q, cache, H.SLOTS, H.Q_LENS, True, 64)
    for b, junk in ((1, -1), (3, 1 << 30)):
        assert cache.lengths[b] == 0
        cache.lens[b] = junk
        cache.block_table[b] = -junk
    O2, lse2 = _varlen(q, cache, H.SLOTS, H.Q_LENS, True, 64)
    assert torch.equal(O, O2) and torch.equal(lse, lse2)
    # slot SLOTS[1] filled but not listed, its device row garbage as well
    cache.lens[H.SLOTS[1]] = 1 << 30
    cache.block_table[H.SLOTS[1]] = -1
    keep = [0, 2, 3]
    sub_q = torch.cat([H.per_sequence(q, H.Q_LENS, j)[0].transpose(0, 1) for j in keep])
    sub_lens = [H.Q_LENS[j] for j in keep]
    SO, Sl = _varlen(sub_q, cache, [H.SLOTS[j] for j in keep], sub_lens, True, 64)
    for pos, j in enumerate(keep):
        H.assert_sequence_equals(SO, Sl, sub_lens, pos, H.reference(Hq, Hkv, lengths, j, True, 64))


# ------------------------------------------------------------------ 4. a uniform batch = the paged decode
@pytest.mark.parametrize("kps", [64, 128])
@pytest.mark.parametrize("causal", [False, True])
def test_uniform_batch_equals_the_paged_decode(lib, causal, kps):
    """Every slot listed, one Sq: attention_mxfp4_decode_paged after the layout change.  That entry also
    runs the splits past a sequence's end (the empty state), which weigh exactly 0 in its merge."""
    import mxfp4_ragged_ref as RR
    from quantizedattention_amd.kv_cache_mxfp4 import PagedKVFP4, attention_mxfp4_decode_paged
    B, Hq, Hkv, Sq, lens = 3, 4, 2, 33, (97, 250, 64)
    q, ks, vs = RR.inputs(B, Hq, Hkv, Sq, lens)
    q = q.cuda()
    cache = PagedKVFP4.allocate(32, 64, B, Hkv, 4, "cuda", free_order=H.scatter(32))
    k = torch.zeros((B, Hkv, max(lens), 128), dtype=torch.float16)
    v = torch.zeros_like(k)
    for b, L in enumerate(lens):
        k[b, :, :L], v[b, :, :L] = ks[b][0], vs[b][0]
    cache.append(k.cuda(), v.cuda(), counts=list(lens))
    PO, Pl = attention_mxfp4_decode_paged(q, cache, causal=causal, keys_per_split=kps)
    packed = q.permute(0, 2, 1, 3).reshape(B * Sq, Hq, 128)
    O, lse = _varlen(packed, cache, list(range(B)), [Sq] * B, causal, kps)
    assert torch.equal(O.view(B, Sq, Hq, 128).permute(0, 2, 1, 3), PO)
    assert torch.equal(lse.view(B, Sq, Hq).permute(0, 2, 1).reshape(B * Hq, Sq), Pl)


@pytest.mark.parametrize("causal", [False, True])
def test_long_uniform_batch_equals_the_paged_decode(lib, causal):
    """2 x 32 / 8 heads, 32 new tokens, 2048 cached, the plan's split (1024 keys, 4 pages of 256).  At
    outputs this small the merge's last step shows: the existing merge rounds two of every eight columns
    once and six twice, which differs from a uniform choice by an f16 ulp in about one row of 300 here
    (measured: 3 of 1024 rows at one sequence of this shape), and in none of the short cases above."""
    from quantizedattention_amd.kv_cache_mxfp4 import PagedKVFP4, attention_mxfp4_decode_paged
    B, Hq, Hkv, Sq, Sk, P = 2, 32, 8, 32, 2048, 256
    g = torch.Generator(device="cuda").manual_seed(43)
    rand = lambda *s: torch.randn(s, device="cuda", generator=g).half()  # noqa: E731
    cache = PagedKVFP4.allocate(B * Sk // P, P, B, Hkv, Sk // P, "cuda", free_order=H.scatter(B * Sk // P))
    cache.append_packed(rand(B * Sk, Hkv, 128), rand(B * Sk, Hkv, 128), [1, 0], [Sk, Sk])
    q = rand(B, Hq, Sq, 128)
    PO, Pl = attention_mxfp4_decode_paged(q, cache, causal=causal)
    packed = q.permute(0, 2, 1, 3).reshape(B * Sq, Hq, 128)
    O, lse = _varlen(packed, cache, [0, 1], [Sq] * B, causal, None)
    assert _plan_kps(cache, [0, 1], [Sq] * B, Hq, None) == 1024
    assert torch.equal(O.view(B, Sq, Hq, 128).permute(0, 2, 1, 3), PO)
    assert torch.equal(lse.view(B, Sq, Hq).permute(0, 2, 1).reshape(B * Hq, Sq), Pl)


# ------------------------------------------------------------------ 5. a fork and its source in one call
def test_fork_and_source_in_one_call(lib):
    """150 tokens at P = 64 forked (two shared full pages, a copied partial page), then both grow apart
    by one packed append; one call attends both, a slot between them empty."""
    from quantizedattention_amd.kv_cache_mxfp4 import PagedKVFP4, PreallocatedKVFP4, attention_mxfp4_decode
    g = torch.Generator().manual_seed(17)
    rand = lambda *s: torch.randn(s, generator=g).half().cuda()  # noqa: E731
    pk, pv = rand(150, 2, 128), rand(150, 2, 128)
    nk, nv = rand(75, 2, 128), rand(75, 2, 128)
    cache = PagedKVFP4.allocate(32, 64, 4, 2, 4, "cuda", free_order=H.scatter(32))
    cache.append_packed(pk, pv, [0], [150])
    cache.fork(0, 2)
    p0, p2 = cache.alloc.pages[0], cache.alloc.pages[2]
    assert p0[:2] == p2[:2] and p0[2] != p2[2] and cache.lengths == [150, 0, 150, 0]
    cache.append_packed(nk, nv, [2, 0], [70, 5])
    assert cache.lengths == [155, 0, 220, 0]
    refs = {}
    for b, lo, n in ((2, 0, 70), (0, 70, 5)):
        k = torch.cat([pk, nk[lo:lo + n]]).transpose(0, 1)[None]
        v = torch.cat([pv, nv[lo:lo + n]]).transpose(0, 1)[None]
        refs[b] = PreallocatedKVFP4.allocate(1, 2, 256, "cuda").append(k, v)
    q_lens = [5, 70]                           # each sequence's new tokens, causal after its own append
    q = rand(75, 4, 128)
    for causal in (False, True):
        O, lse = _varlen(q, cache, [0, 2], q_lens, causal, 64)
        for j, b in enumerate((0, 2)):
            want = attention_mxfp4_decode(H.per_sequence(q, q_lens, j), refs[b], causal=causal, keys_per_split=64)
            H.assert_sequence_equals(O, lse, q_lens, j, want)


# ------------------------------------------------------------------ 6. append_packed keeps the invariant
@pytest.mark.parametrize("P", [64, 128])
@pytest.mark.parametrize("smoothed", [False, True])
def test_append_packed_invariant(lib, smoothed, P):
    """test_gpu_mxfp4_paged.test_append_invariant's schedule, packed: counts (1, 62, 1, 1, 70, 64, 57) on
    one sequence and smaller ones on two others, each left out of some steps (and slot 1 of all); after
    every step the gather through the device table equals a PreallocatedKVFP4 fed the same tokens."""
    from quantizedattention_amd.kv_cache_mxfp4 import PagedKVFP4, PreallocatedKVFP4
    g = torch.Generator().manual_seed(11)
    B, Hkv = 4, 2
    k = torch.randn((B, Hkv, 256, 128), generator=g).half().cuda()
    v = torch.randn((B, Hkv, 256, 128), generator=g).half().cuda()
    k_mean = torch.randn((B, Hkv, 1, 128), generator=g).half().cuda() if smoothed else None
    ref = PreallocatedKVFP4.allocate(B, Hkv, 256, "cuda", k_mean)
    cache = PagedKVFP4.allocate(32, P, B, Hkv, 256 // P, "cuda", k_mean, free_order=H.scatter(32))
    schedule = {2: (1, 62, 1, 1, 70, 64, 57), 0: (1, 0, 1, 1, 33, 64, 7), 3: (0, 5, 0, 64, 0, 3, 9)}
    order = ([2, 0, 3], [3, 2, 0], [0, 2, 3])

    def step(counts, ids):
        """The same tokens into both caches: packed here, padded (counts, 0 = left out) there."""
        n = max(counts.values())
        kn = torch.full((B, Hkv, n, 128), 999.0, dtype=torch.float16, device="cuda")
        vn = torch.full((B, Hkv, n, 128), -999.0, dtype=torch.float16, device="cuda")
        pk, pv = [], []
        for b in ids:
            L, c = cache.lengths[b], counts[b]
            kn[b, :, :c], vn[b, :, :c] = k[b, :, L:L + c], v[b, :, L:L + c]
            pk.append(k[b, :, L:L + c].transpose(0, 1))
            pv.append(v[b, :, L:L + c].transpose(0, 1))
        ref.append(kn, vn, counts=[counts.get(b, 0) for b in range(B)])
        assert cache.append_packed(torch.cat(pk), torch.cat(pv), ids, [counts[b] for b in ids]) is cache
        H.assert_same_bytes(cache, ref)

    for i in range(7):
        counts = {b: c[i] for b, c in schedule.items() if c[i]}
        step(counts, [b for b in order[i % 3] if b in counts])
    assert cache.lengths == [107, 0, 256, 81] and cache.free_pages == 32 - sum(-(-L // P) for L in cache.lengths)
    H.assert_scattered(cache)
    # a freed sequence starts again elsewhere: its old first page is not its new first page
    old = list(cache.alloc.pages[2])
    cache.free([2])
    ref.reset([2])
    step({2: 70, 3: 47}, [3, 2])                       # slot 3 to 128 exactly, slot 2 from 0 into two tiles
    assert cache.lengths == [107, 0, 70, 128] and cache.alloc.pages[2][0] != old[0]
    assert set(cache.alloc.pages[2]) <= set(old)


# ------------------------------------------------------------------ 7. refused appends change nothing
def test_refused_append_packed_changes_nothing(lib):
    from quantizedattention_amd import _lib
    from quantizedattention_amd.kv_cache_mxfp4 import PagedKVFP4
    g = torch.Generator().manual_seed(29)
    rand = lambda *s: torch.randn(s, generator=g).half().cuda()  # noqa: E731
    cache = PagedKVFP4.allocate(3, 64, 3, 2, 2, "cuda", free_order=[2, 0, 1])
    cache.append_packed(rand(70, 2, 128), rand(70, 2, 128), [1], [70])           # two of three pages
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

    k, v = rand(131, 2, 128), rand(131, 2, 128)
    with pytest.raises(_lib.QAttnError, match="max_pages_per_seq"):
        cache.append_packed(k, v, [0, 2], [129, 2])      # three pages in a table row of two
    unchanged()
    with pytest.raises(_lib.QAttnError, match="out of pages"):
        cache.append_packed(k, v, [2, 1], [127, 4])      # slot 2 needs two pages, one is free
    unchanged()
    with pytest.raises(_lib.QAttnError, match="distinct"):
        cache.append_packed(k, v, [1, 1], [65, 66])
    with pytest.raises(_lib.QAttnError, match="sum\\(counts\\)"):
        cache.append_packed(k, v, [0, 2], [64, 64])
    unchanged()
    cache.append_packed(k[:64], v[:64], [2], [64])        # the last page
    assert cache.free_pages == 0 and cache.lengths == [0, 70, 64]


# ------------------------------------------------------------------ 8. the operator
def test_operator_equals_the_python_call(lib):
    import quantizedattention_amd.ops as ops
    from quantizedattention_amd.kv_cache_mxfp4 import plan_varlen
    Hq, Hkv, lengths = 4, 2, H.LENGTHS[1]
    cache, q = H.pool(Hkv, lengths, 64, 32), H.packed_q(Hq)
    for causal, split in ((True, 128), (False, None)):
        O, lse = _varlen(q, cache, H.SLOTS, H.Q_LENS, causal, split)
        O1, l1 = ops.mxfp4_varlen_paged(q, cache, H.SLOTS, H.Q_LENS, causal=causal, keys_per_split=split)
        assert torch.equal(O, O1) and torch.equal(lse, l1)
        kps, rec, work, rows = plan_varlen(cache.lengths, H.SLOTS, H.Q_LENS, Hq, Hkv, split, causal)
        args = (q, *cache.kv, cache.lens, cache.block_table, torch.tensor(rec, dtype=torch.int32).cuda(),
                torch.tensor(work, dtype=torch.int32).cuda(), rows, int(causal), kps)
        O2, l2 = torch.ops.qattn.mxfp4_varlen_paged(*args)
        assert O2.dtype == torch.float16 and l2.dtype == torch.float32
        assert torch.equal(O, O2) and torch.equal(lse, l2)
        # the work list in another order: the same bits
        shuffled = torch.tensor(work[::-1], dtype=torch.int32).cuda()
        O3, l3 = torch.ops.qattn.mxfp4_varlen_paged(*args[:8], shuffled, *args[9:])
        assert torch.equal(O, O3) and torch.equal(lse, l3)
    torch.library.opcheck(torch.ops.qattn.mxfp4_varlen_paged, args, test_utils="test_faketensor")
    op = torch.ops.qattn.mxfp4_varlen_paged
    with pytest.raises(RuntimeError):
        op(*args[:-1], 96)
    with pytest.raises(RuntimeError):
        op(q[:, :3], *args[1:])
    with pytest.raises(RuntimeError):
        op(*args[:7], args[7][:, :4].contiguous(), *args[8:])


# ------------------------------------------------------------------ 9. views
def test_views_give_the_same_bits(lib):
    """q, k and v as offset and transposed views (a misaligned storage offset, the decode layout
    transposed back) against their contiguous copies."""
    from quantizedattention_amd.kv_cache_mxfp4 import PagedKVFP4
    Hq, Hkv, lengths = 4, 2, H.LENGTHS[0]
    cache, q = H.pool(Hkv, lengths, 64, 32), H.packed_q(Hq)
    O, lse = _varlen(q, cache, H.SLOTS, H.Q_LENS, True, 64)
    flat = torch.zeros(q.numel() + 3, dtype=torch.float16, device="cuda")
    flat[3:] = q.reshape(-1)
    for view in (flat[3:].view(q.shape), q.transpose(0, 1).contiguous().transpose(0, 1)):
        assert not view.is_contiguous() or view.data_ptr() % 16
        O2, lse2 = _varlen(view, cache, H.SLOTS, H.Q_LENS, True, 64)
        assert torch.equal(O, O2) and torch.equal(lse, lse2)
    g = torch.Generator().manual_seed(41)
    k, v = (torch.randn((Hkv, 71, 128), generator=g).half().cuda() for _ in range(2))
    pools = []
    for kk, vv in ((k.transpose(0, 1), v.transpose(0, 1)),
                   (k.transpose(0, 1).contiguous(), v.transpose(0, 1).contiguous())):
        c = PagedKVFP4.allocate(8, 64, 2, Hkv, 2, "cuda", free_order=H.scatter(8))
        pools.append(c.append_packed(kk, vv, [1], [71]))
    for a, b in zip(H.gather(pools[0], 1), H.gather(pools[1], 1)):
        assert torch.equal(a, b)
    assert torch.equal(pools[0].vtail[1, :, :7], pools[1].vtail[1, :, :7])


# ------------------------------------------------------------------ 10. the C entries on flat buffers
def test_nothing_is_written_past_the_buffers(lib):
    """The three entries on flat buffers with 128 sentinel rows behind opart, ml, O and lse: every
    partial row is written, no split is an empty state (only splits < ns_j run), nothing past the end."""
    from quantizedattention_amd import _lib
    from quantizedattention_amd.attention_mxfp4 import _qk_scale, mxfp4_quantize_rows
    from quantizedattention_amd.kv_cache_mxfp4 import plan_varlen
    SENT, D, pad = -12288.0, 128, 128
    Hq, Hkv, lengths = 4, 2, H.LENGTHS[1]
    cache, q = H.pool(Hkv, lengths, 64, 32), H.packed_q(Hq)
    T = q.shape[0]
    kps, rec, work, rows = plan_varlen(cache.lengths, H.SLOTS, H.Q_LENS, Hq, Hkv, 64)
    assert rows == sum(ns * Hkv * 2 * n for ns, n in zip((1, 3, 4, 2), H.Q_LENS))
    rec_d, work_d = (torch.tensor(t, dtype=torch.int32).cuda() for t in (rec, work))
    q4, qs = mxfp4_quantize_rows(q)
    opart = torch.full(((rows + pad) * D,), SENT, dtype=torch.float32, device="cuda")
    ml = torch.full(((rows + pad) * 2,), SENT, dtype=torch.float32, device="cuda")
    out = torch.full(((T * Hq + pad) * D,), SENT, dtype=torch.float16, device="cuda")
    lse = torch.full((T * Hq + pad,), SENT, dtype=torch.float32, device="cuda")
    st = _lib.stream_of(q)
    _lib.call("qattn_mxfp4_attn_fwd_varlen_paged", _lib.ptr(q4), _lib.ptr(qs), *(_lib.ptr(t) for t in cache.kv),
              _lib.ptr(opart), _lib.ptr(ml), _lib.ptr(cache.lens), _lib.ptr(cache.block_table), _lib.ptr(rec_d),
              _lib.ptr(work_d), len(rec), len(work), T, rows, H.MAX_SEQS, Hkv, Hq // Hkv, cache.num_pages, 64,
              cache.alloc.max_pages_per_seq, 0, kps, D, _qk_scale(D), st)
    torch.cuda.synchronize()
    for t in (opart[rows * D:], ml[rows * 2:], out, lse):
        assert t.numel() >= 128 and (t == SENT).all()
    m = ml[:rows * 2].view(rows, 2)
    assert not (opart[:rows * D] == SENT).any() and not (m == SENT).any()
    assert torch.isfinite(m).all() and (m[:, 1] > 0).all()
    _lib.call("qattn_mxfp4_varlen_combine", _lib.ptr(opart), _lib.ptr(ml), _lib.ptr(out), _lib.ptr(lse),
              _lib.ptr(rec_d), len(rec), T, Hq, Hkv, rows, D, st)
    torch.cuda.synchronize()
    for t in (opart[rows * D:], ml[rows * 2:], out[T * Hq * D:], lse[T * Hq:]):
        assert t.numel() >= 128 and (t == SENT).all()
    O, l2 = _varlen(q, cache, H.SLOTS, H.Q_LENS, False, 64)
    assert torch.equal(out[:T * Hq * D].view(T, Hq, D), O) and torch.equal(lse[:T * Hq].view(T, Hq), l2)
