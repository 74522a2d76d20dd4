"""The paged MX-FP4 cache on the GPU: PagedKVFP4 (qattn_mxfp4_paged_append),
attention_mxfp4_decode_paged (qattn_mxfp4_attn_fwd_split_paged) and torch.ops.qattn.mxfp4_decode_paged.

One reference throughout: PreallocatedKVFP4 + attention_mxfp4_decode fed the same tokens, compared
with torch.equal (the paged kernels run the preallocated ones' arithmetic on the same bytes; only
where the bytes lie differs).  The preallocated path itself is held to its restatement in
tests/test_gpu_mxfp4_ragged.py.  Page pools are handed out in a scattered order (``_scatter``) so that no
sequence's pages are adjacent or ascending: an identity table would hide a kernel that ignores it.
"""
import functools

import pytest
import torch

import mxfp4_ragged_ref as RR

pytestmark = pytest.mark.gpu

SENTINEL = -12288.0   # exact in fp16
EXTRA = (3, 4, 2, 3, (37, 128, 200))
SHAPES = [c[:5] for c in RR.CASES] + [EXTRA]


def _scatter(n):
    """A free order whose first n // 3 pages descend in steps of 3."""
    return [p for r in range(3) for p in range(n - 1 - r, -1, -3)]


def _assert_scattered(cache):
    for pages in cache.alloc.pages:
        assert all(b < a - 1 for a, b in zip(pages, pages[1:])), pages


def _batch(ks, vs):
    """The sequences ks / vs (per sequence [1, Hkv, L_b, 128]) as one append with counts; the tokens a
    sequence does not take are garbage."""
    B, Hkv, lens = len(ks), ks[0].shape[1], [k.shape[2] for k in ks]
    n = max(lens)
    k = torch.full((B, Hkv, n, 128), 777.0, dtype=torch.float16)
    v = torch.full((B, Hkv, n, 128), -555.0, dtype=torch.float16)
    for b, L in enumerate(lens):
        k[b, :, :L], v[b, :, :L] = ks[b][0], vs[b][0]
    return k.cuda(), v.cuda(), lens


def _fill(ks, vs, cap, k_mean=None):
    from quantizedattention_amd.kv_cache_mxfp4 import PreallocatedKVFP4
    k, v, lens = _batch(ks, vs)
    cache = PreallocatedKVFP4.allocate(len(ks), ks[0].shape[1], cap, "cuda", k_mean)
    cache.append(k, v, counts=lens)
    assert cache.lengths == lens
    return cache


def _fill_paged(ks, vs, P, num_pages=32, mpp=None, k_mean=None):
    from quantizedattention_amd.kv_cache_mxfp4 import PagedKVFP4
    k, v, lens = _batch(ks, vs)
    mpp = -(-256 // P) if mpp is None else mpp
    cache = PagedKVFP4.allocate(num_pages, P, len(ks), ks[0].shape[1], mpp, "cuda", k_mean,
                                free_order=_scatter(num_pages))
    cache.append(k, v, counts=lens)
    assert cache.lengths == lens
    _assert_scattered(cache)
    return cache


def _gather(cache, b):
    """Sequence b's rows and tiles through the DEVICE table: (k4 [Hkv, L, 64], ks [Hkv, L, 4], vt [Hkv,
    ceil(L/64), 128, 32], vs [Hkv, ceil(L/64), 128, 2])."""
    L, P, H = cache.lengths[b], cache.page_tokens, cache.k4.shape[1]
    ids = cache.block_table[b, :-(-L // P)].long()
    k4, ks, vt, vs = (t[ids].transpose(0, 1).reshape(H, -1, *t.shape[3:]) for t in cache.kv)
    nt = -(-L // 64)
    return k4[:, :L], ks[:, :L], vt[:, :nt], vs[:, :nt]


def _assert_same_bytes(paged, ref):
    """The invariant: through its table, every sequence holds the preallocated cache's bytes."""
    H = ref.k4.shape[1]
    assert paged.lengths == ref.lengths and paged.lens.cpu().tolist() == paged.lengths
    table = paged.block_table.cpu().tolist()
    for b, L in enumerate(paged.lengths):
        pages = paged.alloc.pages[b]
        assert len(pages) == -(-L // paged.page_tokens) and table[b][:len(pages)] == pages, b
        if L == 0:
            continue
        nt = -(-L // 64)
        k4, ks, vt, vs = _gather(paged, b)
        assert torch.equal(k4, ref.k4[b, :, :L]) and torch.equal(ks, ref.ks[b, :, :L]), (b, L)
        assert torch.equal(vt, ref.vt[b * H:b * H + H, :nt]), (b, L)
        assert torch.equal(vs, ref.vs[b * H:b * H + H, :nt]), (b, L)


def _assert_decodes_equal(q, paged, ref, causal, kps):
    from quantizedattention_amd.kv_cache_mxfp4 import attention_mxfp4_decode, attention_mxfp4_decode_paged
    O, lse = attention_mxfp4_decode_paged(q, paged, causal=causal, keys_per_split=kps)
    RO, Rl = attention_mxfp4_decode(q, ref, causal=causal, keys_per_split=kps)
    assert O.shape == RO.shape and lse.shape == Rl.shape and lse.dtype == torch.float32
    assert torch.equal(O, RO) and torch.equal(lse, Rl)
    assert torch.isfinite(O.float()).all() and torch.isfinite(lse).all()
    return O, lse


# ------------------------------------------------------------------ 1. the append invariant
@pytest.mark.parametrize("P", [64, 128])
@pytest.mark.parametrize("smoothed", [False, True])
def test_append_invariant(lib, smoothed, P):
    """test_gpu_mxfp4_ragged.test_append_invariant's schedule into both caches: after every append the
    gather through the table equals the preallocated cache's rows and tiles."""
    from quantizedattention_amd.kv_cache_mxfp4 import PagedKVFP4, PreallocatedKVFP4
    g = torch.Generator().manual_seed(11)
    k = torch.randn((2, 2, 256, 128), generator=g).half()
    v = torch.randn((2, 2, 256, 128), generator=g).half()
    k_mean = torch.randn((2, 2, 1, 128), generator=g).half().cuda() if smoothed else None
    ref = PreallocatedKVFP4.allocate(2, 2, 256, "cuda", k_mean)
    cache = PagedKVFP4.allocate(32, P, 2, 2, 256 // P, "cuda", k_mean, free_order=_scatter(32))
    assert cache.lengths == [0, 0] and cache.free_pages == 32 and cache.shape == (2, 2, 256, 128)
    for n, c1 in zip((1, 62, 1, 1, 70, 64, 57), (1, 0, 1, 1, 33, 64, 7)):
        kn = torch.full((2, 2, n, 128), 999.0, dtype=torch.float16)   # what is not taken is garbage
        vn = torch.full((2, 2, n, 128), -999.0, dtype=torch.float16)
        for b, c in enumerate((n, c1)):
            L = cache.lengths[b]
            kn[b, :, :c], vn[b, :, :c] = k[b, :, L:L + c], v[b, :, L:L + c]
        ref.append(kn.cuda(), vn.cuda(), counts=[n, c1])
        assert cache.append(kn.cuda(), vn.cuda(), counts=[n, c1]) is cache
        _assert_same_bytes(cache, ref)
    assert cache.lengths == [256, 107]
    assert [cache.capacity_tokens(b) for b in (0, 1)] == [256, 128]
    assert cache.free_pages == 32 - 256 // P - 128 // P
    _assert_scattered(cache)
    # without counts every sequence takes all n; a freed sequence starts again on other pages
    cache.free([0])
    ref.reset([0])
    assert cache.lengths == [0, 107] and cache.lens.cpu().tolist() == [0, 107]
    kn = torch.stack([k[0, :, :5], k[1, :, 107:112]]).cuda()
    vn = torch.stack([v[0, :, :5], v[1, :, 107:112]]).cuda()
    cache.append(kn, vn)
    ref.append(kn, vn)
    assert cache.lengths == [5, 112]
    _assert_same_bytes(cache, ref)
    cache.append(k[:, :, 128:187].cuda(), v[:, :, 128:187].cuda(), counts=[59, 16])   # to 64 and 128 exactly
    ref.append(k[:, :, 128:187].cuda(), v[:, :, 128:187].cuda(), counts=[59, 16])
    snap, want = cache.snapshot(1), ref.snapshot(1)
    for a, b in zip((*snap.kv, snap.k_mean), (*want.kv, want.k_mean)):
        assert (a is None and b is None) or torch.equal(a, b)


# ------------------------------------------------------------------ 2. decode = the preallocated decode
@functools.lru_cache(maxsize=None)
def _shape_inputs(shape):
    """(q on the device, ks, vs, the preallocated reference cache) of one of SHAPES; do not modify."""
    B, Hq, Hkv, Sq, lens = shape
    q, ks, vs = RR.inputs(B, Hq, Hkv, Sq, lens)
    return q.cuda(), ks, vs, _fill(ks, vs, 256)


@functools.lru_cache(maxsize=None)
def _shape_paged(shape, P):
    """The paged cache of one of SHAPES; do not modify."""
    _, ks, vs, _ = _shape_inputs(shape)
    return _fill_paged(ks, vs, P)


@pytest.mark.parametrize("kps", [64, 128, None])
@pytest.mark.parametrize("P", [64, 128])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_decode_equals_preallocated(lib, shape, causal, P, kps):
    """A split inside a page (P 128, 64 keys per split), a split over several pages (P 64, 128 keys per
    split) and the plan, on scattered tables."""
    q, _, _, ref = _shape_inputs(shape)
    _assert_decodes_equal(q, _shape_paged(shape, P), ref, causal, kps)


# ------------------------------------------------------------------ 3. nothing unowned matters
@pytest.mark.parametrize("P", [64, 128])
@pytest.mark.parametrize("shape", [SHAPES[1], EXTRA])
def test_nothing_unowned_matters(lib, shape, P):
    """0xFF (scale byte 255 is NaN) in every free page, in every owned page past the length and in the
    unused vtail slots, and every table entry past a sequence's pages pointing at a poisoned page: O and
    lse do not move by a bit, and neither does what the next append writes."""
    from quantizedattention_amd.kv_cache_mxfp4 import attention_mxfp4_decode_paged
    B, Hq, Hkv, Sq, lens = shape
    q, ks, vs, _ = _shape_inputs(shape)
    cache = _fill_paged(ks, vs, P)
    ref = _fill(ks, vs, 256)
    O, lse = attention_mxfp4_decode_paged(q, cache, causal=True, keys_per_split=64)
    free = sorted(set(range(cache.num_pages)) - {p for pages in cache.alloc.pages for p in pages})
    assert len(free) == cache.free_pages > 0
    for t in cache.kv:
        t[torch.tensor(free, device="cuda")] = 0xFF
    for b, L in enumerate(lens):
        pages = cache.alloc.pages[b]
        last, r, nt = pages[-1], L - (len(pages) - 1) * P, -(-L // 64) - (len(pages) - 1) * (P // 64)
        cache.k4[last, :, r:] = 0xFF
        cache.ks[last, :, r:] = 0xFF
        cache.vt[last, :, nt:] = 0xFF
        cache.vs[last, :, nt:] = 0xFF
        cache.vtail[b, :, L % 64:] = float("nan")
        cache.block_table[b, len(pages):] = free[b % len(free)]     # an existing, poisoned page
        cache.alloc.table[b][len(pages):] = [free[b % len(free)]] * (cache.alloc.max_pages_per_seq - len(pages))
    O2, lse2 = attention_mxfp4_decode_paged(q, cache, causal=True, keys_per_split=64)
    assert torch.equal(O, O2) and torch.equal(lse, lse2)
    assert torch.isfinite(O2.float()).all() and torch.isfinite(lse2).all()
    g = torch.Generator().manual_seed(3)
    kn, vn = (torch.randn((B, Hkv, 3, 128), generator=g).half().cuda() for _ in range(2))
    cache.append(kn, vn)
    ref.append(kn, vn)
    _assert_same_bytes(cache, ref)
    _assert_decodes_equal(q, cache, ref, False, 64)


# ------------------------------------------------------------------ 4. fork
def test_fork_shares_the_full_pages(lib):
    """A prompt of 150 tokens at P = 64 forked to two slots that then grow apart."""
    from quantizedattention_amd.kv_cache_mxfp4 import PagedKVFP4, PreallocatedKVFP4
    g = torch.Generator().manual_seed(17)
    rand = lambda *s: torch.randn(s, generator=g).half().cuda()  # noqa: E731
    prompt_k, prompt_v = rand(1, 2, 150, 128).expand(3, -1, -1, -1), rand(1, 2, 150, 128).expand(3, -1, -1, -1)
    new_k, new_v, q = rand(3, 2, 70, 128), rand(3, 2, 70, 128), rand(3, 4, 2, 128)
    k_mean = rand(1, 2, 1, 128).expand(3, -1, -1, -1)      # one prompt, one mean
    cache = PagedKVFP4.allocate(32, 64, 3, 2, 4, "cuda", k_mean, free_order=_scatter(32))
    cache.append(prompt_k, prompt_v, counts=[150, 0, 0])
    src = [t.clone() for t in _gather(cache, 0)]
    cache.fork(0, 1)
    cache.fork(0, 2)
    assert cache.lengths == [150, 150, 150] and cache.free_pages == 32 - 3 - 2
    p0, p1, p2 = cache.alloc.pages
    assert p1[:2] == p0[:2] == p2[:2] and len({p0[2], p1[2], p2[2]}) == 3
    cache.append(new_k, new_v, counts=[0, 5, 70])
    assert set(p1) & set(p2) == set(p0[:2]) and len(set(p1) & set(p2)) == 2
    assert [cache.alloc.refcount[p] for p in p0] == [3, 3, 1]
    ref = PreallocatedKVFP4.allocate(3, 2, 256, "cuda", k_mean)
    ref.append(prompt_k, prompt_v)
    ref.append(new_k, new_v, counts=[0, 5, 70])
    _assert_same_bytes(cache, ref)
    for causal in (False, True):
        _assert_decodes_equal(q, cache, ref, causal, 64)
    assert cache.lengths[0] == 150
    for a, b in zip(src, _gather(cache, 0)):
        assert torch.equal(a, b)
    cache.free([0, 1, 2])
    assert cache.free_pages == cache.num_pages == 32 and cache.lengths == [0, 0, 0]
    assert cache.lens.cpu().tolist() == [0, 0, 0]


# ------------------------------------------------------------------ 5. reuse
def test_freed_pages_are_reused(lib):
    from quantizedattention_amd.kv_cache_mxfp4 import PagedKVFP4, PreallocatedKVFP4
    g = torch.Generator().manual_seed(19)
    rand = lambda *s: torch.randn(s, generator=g).half().cuda()  # noqa: E731
    k, v, q = rand(2, 2, 150, 128), rand(2, 2, 150, 128), rand(2, 4, 1, 128)
    cache = PagedKVFP4.allocate(5, 64, 2, 2, 4, "cuda", free_order=[4, 2, 0, 3, 1])
    ref = PreallocatedKVFP4.allocate(2, 2, 256, "cuda")
    for c in (cache, ref):
        c.append(k[:, :, :100], v[:, :, :100], counts=[100, 60])
    held = set(cache.alloc.pages[0])
    assert len(held) == 2 and cache.free_pages == 2
    cache.free([0])
    ref.reset([0])
    for c in (cache, ref):
        c.append(k, v, counts=[0, 150])              # 210 tokens: four pages, two of them sequence 0's
    assert held <= set(cache.alloc.pages[1]) and cache.free_pages == 1
    for c in (cache, ref):
        c.append(k[:, :, 100:130], v[:, :, 100:130], counts=[30, 0])
    assert cache.free_pages == 0 and cache.lengths == [30, 210]
    _assert_same_bytes(cache, ref)
    _assert_decodes_equal(q, cache, ref, False, 64)
    _assert_decodes_equal(q, cache, ref, True, None)


# ------------------------------------------------------------------ 6. a decode loop
def test_decode_loop(lib):
    """70 tokens in one append, then 60 steps of one appended token and one causal query, crossing a
    page at 128; every step beside the preallocated loop."""
    from quantizedattention_amd.kv_cache_mxfp4 import (PagedKVFP4, PreallocatedKVFP4, attention_mxfp4_decode,
                                                       attention_mxfp4_decode_paged)
    g = torch.Generator().manual_seed(7)
    kd = torch.randn((1, 1, 130, 128), generator=g).half().cuda()
    vd = torch.randn((1, 1, 130, 128), generator=g).half().cuda()
    qd = torch.randn((130, 1, 4, 1, 128), generator=g).half().cuda()
    ref = PreallocatedKVFP4.allocate(1, 1, 192, "cuda")
    cache = PagedKVFP4.allocate(8, 64, 1, 1, 3, "cuda", free_order=_scatter(8))
    outs = []
    for c in (cache, ref):
        c.append(kd[:, :, :70], vd[:, :, :70])
    for t in range(70, 130):
        for c in (cache, ref):
            c.append(kd[:, :, t:t + 1], vd[:, :, t:t + 1])
        outs.append((attention_mxfp4_decode_paged(qd[t], cache, causal=True),
                     attention_mxfp4_decode(qd[t], ref, causal=True)))
    torch.cuda.synchronize()
    assert cache.lengths == [130] and cache.lens.cpu().tolist() == [130]
    assert len(cache.alloc.pages[0]) == 3
    for step, ((O, lse), (RO, Rl)) in enumerate(outs):
        assert torch.equal(O, RO) and torch.equal(lse, Rl), 71 + step
        assert torch.isfinite(O.float()).all() and torch.isfinite(lse).all(), 71 + step


# ------------------------------------------------------------------ 7. the C entry on flat buffers
def test_empty_splits_and_row_tails(lib):
    """lens (64, 256), 64 keys per split, rows = 5 (G = 5, one query position), 128 sentinel rows behind
    opart and ml: empty splits write (-inf, 0, 0) and nothing is written past the end."""
    from quantizedattention_amd import _lib
    from quantizedattention_amd.attention_mxfp4 import _qk_scale, mxfp4_quantize_rows
    from quantizedattention_amd.kv_cache_mxfp4 import attention_mxfp4_decode
    q, ks, vs = RR.inputs(2, 5, 1, 1, (64, 256))
    cache, ref = _fill_paged(ks, vs, 64), _fill(ks, vs, 256)
    q = q.cuda()
    R, ns, D, pad = 10, 4, 128, 128
    q4, qs = mxfp4_quantize_rows(q)
    opart = torch.full(((ns * R + pad) * D,), SENTINEL, dtype=torch.float32, device="cuda")
    ml = torch.full(((ns * R + pad) * 2,), SENTINEL, dtype=torch.float32, device="cuda")
    out = torch.full(((R + pad) * D,), SENTINEL, dtype=torch.float16, device="cuda")
    lse = torch.full((R + pad,), SENTINEL, dtype=torch.float32, device="cuda")
    st = _lib.stream_of(q)
    _lib.call("qattn_mxfp4_attn_fwd_split_paged", _lib.ptr(q4), _lib.ptr(qs), *(_lib.ptr(t) for t in cache.kv),
              _lib.ptr(opart), _lib.ptr(ml), _lib.ptr(cache.lens), _lib.ptr(cache.block_table), 2, 1, 5, 1,
              cache.num_pages, 64, cache.alloc.max_pages_per_seq, 256, 0, 64, D, _qk_scale(D), st)
    torch.cuda.synchronize()
    for t in (opart[ns * R * D:], ml[ns * R * 2:], out, lse):
        assert t.numel() >= 128 and (t == SENTINEL).all()
    _lib.call("qattn_mxfp4_split_combine", _lib.ptr(opart), _lib.ptr(ml), _lib.ptr(out), _lib.ptr(lse),
              R, ns, D, st)
    torch.cuda.synchronize()
    for t in (opart[ns * R * D:], ml[ns * R * 2:], out[R * D:], lse[R:]):
        assert t.numel() >= 128 and (t == SENTINEL).all()
    op, m = opart[:ns * R * D].view(ns, R, D).cpu(), ml[:ns * R * 2].view(ns, R, 2).cpu()
    assert not (op == SENTINEL).any() and not (m == SENTINEL).any()      # every partial row written
    empty = torch.isinf(m[..., 0]) & (m[..., 0] < 0)
    want = torch.zeros((4, 10), dtype=torch.bool)
    want[1:, :5] = True                     # splits 1-3 of sequence 0 (64 keys: one tile)
    assert torch.equal(empty, want)
    assert (m[..., 1][empty] == 0).all() and (op[empty] == 0).all()
    assert (m[..., 1][~empty] > 0).all()
    O, l2 = attention_mxfp4_decode(q, ref, keys_per_split=64)
    assert torch.equal(out[:R * D].view(R, D), O.reshape(R, D)) and torch.equal(lse[:R], l2.reshape(-1))
    assert torch.isfinite(O.float()).all() and torch.isfinite(l2).all()


# ------------------------------------------------------------------ 8. the operator
def test_operator_equals_the_python_call(lib):
    import quantizedattention_amd.ops as ops
    from quantizedattention_amd.kv_cache_mxfp4 import attention_mxfp4_decode_paged
    shape = SHAPES[1]
    q, _, _, _ = _shape_inputs(shape)
    cache = _shape_paged(shape, 64)
    for split in (128, None):
        O, lse = attention_mxfp4_decode_paged(q, cache, causal=True, keys_per_split=split)
        O1, l1 = ops.mxfp4_decode_paged(q, cache, causal=True, keys_per_split=split)
        assert torch.equal(O, O1) and torch.equal(lse, l1)
        O2, l2 = torch.ops.qattn.mxfp4_decode_paged(q, *cache.kv, cache.lens, cache.block_table, 256, 1,
                                                    0 if split is None else split)
        assert torch.equal(O, O2) and torch.equal(lse, l2)


# ------------------------------------------------------------------ 9. operands past 4 GiB
def test_pool_past_4gib(lib):
    """k4 and vt of 2^15 + 8 pages x 2 heads x 1024 tokens are 4 GiB + 1 MiB each; one sequence of two
    pages lies on the highest page ids, past byte 2^32 of both."""
    from quantizedattention_amd.kv_cache_mxfp4 import PagedKVFP4, PreallocatedKVFP4
    if torch.cuda.mem_get_info()[0] < 24 << 30:
        pytest.skip("needs 24 GiB of free device memory")
    N, P = (1 << 15) + 8, 1024
    order = [N - 1, N - 3] + [p for p in range(N) if p not in (N - 1, N - 3)]
    cache = PagedKVFP4.allocate(N, P, 1, 2, 2, "cuda", free_order=order)
    assert cache.k4.numel() > 1 << 32 and cache.vt.numel() > 1 << 32
    g = torch.Generator().manual_seed(23)
    rand = lambda *s: torch.randn(s, generator=g).half().cuda()  # noqa: E731
    k, v, q = rand(1, 2, 1324, 128), rand(1, 2, 1324, 128), rand(1, 4, 2, 128)
    ref = PreallocatedKVFP4.allocate(1, 2, 2048, "cuda")
    for c in (cache, ref):
        c.append(k[:, :, :1000], v[:, :, :1000])
        c.append(k[:, :, 1000:], v[:, :, 1000:])
    assert cache.alloc.pages[0] == [N - 1, N - 3]
    assert (N - 3) * 2 * P * 64 > 1 << 32          # the lower of the two pages starts past 4 GiB
    _assert_same_bytes(cache, ref)
    _assert_decodes_equal(q, cache, ref, False, None)
    _assert_decodes_equal(q, cache, ref, True, 128)
    del cache
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ 10. errors
def _device_state(cache):
    return [t.clone() for t in (*cache.kv, cache.vtail, cache.lens, cache.block_table)]


def _host_state(cache):
    a = cache.alloc
    return (list(cache.lengths), list(a._free), list(a.refcount), [list(p) for p in a.pages],
            [list(r) for r in a.table])


def test_errors_leave_the_state_unchanged(lib):
    from quantizedattention_amd import _lib
    from quantizedattention_amd.kv_cache_mxfp4 import PagedKVFP4, attention_mxfp4_decode_paged
    g = torch.Generator().manual_seed(29)
    rand = lambda *s: torch.randn(s, generator=g).half().cuda()  # noqa: E731
    for p in (0, 32, 96, 2048):
        with pytest.raises(_lib.QAttnError, match="page_tokens"):
            PagedKVFP4.allocate(8, p, 2, 2, 4, "cuda")
    cache = PagedKVFP4.allocate(3, 64, 2, 2, 2, "cuda", free_order=[2, 0, 1])
    cache.append(rand(2, 2, 70, 128), rand(2, 2, 70, 128), counts=[70, 0])     # two of three pages
    dev, host = _device_state(cache), _host_state(cache)

    def unchanged():
        torch.cuda.synchronize()
        assert _host_state(cache) == host
        for a, b in zip(dev, _device_state(cache)):
            assert torch.equal(a, b)

    k3, v3 = rand(2, 2, 129, 128), rand(2, 2, 129, 128)
    with pytest.raises(_lib.QAttnError, match="max_pages_per_seq"):
        cache.append(k3, v3, counts=[0, 129])            # three pages in a table row of two
    unchanged()
    with pytest.raises(_lib.QAttnError, match="out of pages"):
        cache.append(k3, v3, counts=[58, 128])           # sequence 1 needs two pages, one is free
    unchanged()
    q = rand(2, 4, 3, 128)
    with pytest.raises(_lib.QAttnError, match="at least one cached token"):
        attention_mxfp4_decode_paged(q, cache)           # sequence 1 is empty
    unchanged()
    cache.fork(0, 1)
    dev, host = _device_state(cache), _host_state(cache)
    assert cache.lengths == [70, 70] and cache.free_pages == 0
    with pytest.raises(_lib.QAttnError, match="not empty"):
        cache.fork(0, 1)
    unchanged()
    with pytest.raises(_lib.QAttnError, match="causal"):
        attention_mxfp4_decode_paged(rand(2, 4, 71, 128), cache, causal=True)
    with pytest.raises(_lib.QAttnError, match="keys_per_split"):
        attention_mxfp4_decode_paged(q, cache, keys_per_split=96)
    with pytest.raises(_lib.QAttnError, match="PagedKVFP4"):
        attention_mxfp4_decode_paged(q, object())
    unchanged()
    attention_mxfp4_decode_paged(q, cache, causal=True)
