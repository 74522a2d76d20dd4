"""Sliding-window attention with sinks over the paged MX-FP4 cache on the GPU:
attention_mxfp4_varlen_paged(window=, sinks=) (qattn_mxfp4_attn_fwd_varlen_paged_window +
qattn_mxfp4_varlen_combine), PagedKVFP4.trim and torch.ops.qattn.mxfp4_varlen_paged_window.

torch.equal wherever an exact instrument exists: a window of everything is the causal call; a decode
window that starts on a tile is attention_mxfp4_decode on a cache that holds only the window's (and the
sinks') tokens; order, company and trimmed pages change no bit.  The general masks are held to the CPU
restatement tests/mxfp4_window_ref.py within the bars of tests/test_gpu_mxfp4_ragged.py (O max-abs <=
2e-2, lse <= 1e-4, relL2 <= 2e-3).  Pools are handed out in mxfp4_varlen_helpers.scatter order and two
slots stay empty.
"""
import functools

import pytest
import torch

import mxfp4_varlen_helpers as H

pytestmark = pytest.mark.gpu

HEADS = [(4, 2), (4, 4)]
POOLS = [(64, 32), (256, 48)]     # (page tokens, pages)
ALIGNED_POOLS = [(64, 48), (256, 48)]     # two sequences of 321 tokens: 12 pages of the scattered run
MASKS = [(1, 0), (1, 4), (5, 0), (64, 0), (100, 4), (100, 70), (37, 64)]


def _window(q, cache, ids, q_lens, kps, W, S):
    from quantizedattention_amd.kv_cache_mxfp4 import attention_mxfp4_varlen_paged
    O, lse = attention_mxfp4_varlen_paged(q, cache, ids, q_lens, causal=True, keys_per_split=kps, window=W, sinks=S)
    assert O.shape == q.shape and O.dtype == torch.float16 and lse.shape == q.shape[:2]
    assert lse.dtype == torch.float32
    assert torch.isfinite(O.float()).all() and torch.isfinite(lse).all()
    return O, lse


def _fill(Hkv, lengths, P, pages, mpp, slots=H.SLOTS):
    """mxfp4_varlen_helpers.fill_pool with a table row of ``mpp`` pages (it stops at 320 tokens)."""
    from quantizedattention_amd.kv_cache_mxfp4 import PagedKVFP4
    kv, n = H.tokens(Hkv, lengths), max(lengths)
    k = torch.full((H.MAX_SEQS, Hkv, n, H.D), 777.0, dtype=torch.float16, device="cuda")
    v = torch.full((H.MAX_SEQS, Hkv, n, H.D), -555.0, dtype=torch.float16, device="cuda")
    counts = [0] * H.MAX_SEQS
    for (kj, vj), b, L in zip(kv, slots, lengths):
        k[b, :, :L], v[b, :, :L], counts[b] = kj, vj, L
    cache = PagedKVFP4.allocate(pages, P, H.MAX_SEQS, Hkv, mpp, "cuda", free_order=H.scatter(pages))
    cache.append(k, v, counts=counts)
    H.assert_scattered(cache)
    return cache


@functools.lru_cache(maxsize=None)
def _pool(Hkv, lengths, P, pages, mpp):
    """Shared; do not modify."""
    return _fill(Hkv, lengths, P, pages, mpp)


# ------------------------------------------------------------------ 1. a window of everything is causal
@pytest.mark.parametrize("kps", [64, 128, None])
@pytest.mark.parametrize("S", [0, 4])
@pytest.mark.parametrize("lengths", H.LENGTHS)
@pytest.mark.parametrize("P,pages", POOLS)
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_window_of_everything_is_causal(lib, Hq, Hkv, P, pages, lengths, S, kps):
    from quantizedattention_amd.kv_cache_mxfp4 import attention_mxfp4_varlen_paged
    cache, q = H.pool(Hkv, lengths, P, pages), H.packed_q(Hq)
    RO, Rl = attention_mxfp4_varlen_paged(q, cache, H.SLOTS, H.Q_LENS, causal=True, keys_per_split=kps)
    for W in (max(lengths), 1 << 40):
        O, lse = _window(q, cache, H.SLOTS, H.Q_LENS, kps, W, S)
        assert torch.equal(O, RO) and torch.equal(lse, Rl), W


# ------------------------------------------------------------------ 2, 3. aligned decode windows
def _truncated(Hq, Hkv, L, j, keep, kps):
    """attention_mxfp4_decode, Sq = 1, of sequence j of tokens(Hkv, (L, L)) on a batch-1 preallocated
    cache fed only the token ranges ``keep``."""
    from quantizedattention_amd.kv_cache_mxfp4 import PreallocatedKVFP4, attention_mxfp4_decode
    k, v = H.tokens(Hkv, (L, L))[j]
    ref = PreallocatedKVFP4.allocate(1, Hkv, 320, "cuda")
    for a, b in keep:
        ref.append(k[None, :, a:b].contiguous(), v[None, :, a:b].contiguous())
    q = H.packed_q(Hq, (1, 1))[j][None, :, None]                     # [1, Hq, 1, D]
    return attention_mxfp4_decode(q, ref, causal=True, keys_per_split=kps)


@pytest.mark.parametrize("kps", [64, 128])
@pytest.mark.parametrize("L,W", [(200, 72), (256, 64), (130, 66), (321, 129)])
@pytest.mark.parametrize("P,pages", ALIGNED_POOLS)
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_aligned_decode_window_is_the_truncated_cache(lib, Hq, Hkv, P, pages, L, W, kps):
    assert (L - W) % 64 == 0
    cache, q = _pool(Hkv, (L, L), P, pages, -(-384 // P)), H.packed_q(Hq, (1, 1))
    O, lse = _window(q, cache, H.SLOTS[:2], (1, 1), kps, W, 0)
    for j in range(2):
        H.assert_sequence_equals(O, lse, (1, 1), j, _truncated(Hq, Hkv, L, j, [(L - W, L)], kps))


@pytest.mark.parametrize("L,W", [(321, 129), (256, 64)])
@pytest.mark.parametrize("P,pages", ALIGNED_POOLS)
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_aligned_sinks(lib, Hq, Hkv, P, pages, L, W):
    """S = 64, 64 keys per split: the sink tile is split 0 here and in the reference cache, which holds
    tokens [0, 64) followed by [L - W, L)."""
    cache, q = _pool(Hkv, (L, L), P, pages, -(-384 // P)), H.packed_q(Hq, (1, 1))
    O, lse = _window(q, cache, H.SLOTS[:2], (1, 1), 64, W, 64)
    for j in range(2):
        H.assert_sequence_equals(O, lse, (1, 1), j, _truncated(Hq, Hkv, L, j, [(0, 64), (L - W, L)], 64))


# ------------------------------------------------------------------ 4. general masks: the restatement
@functools.lru_cache(maxsize=None)
def _restated(Hq, Hkv, j, W, S, kps):
    import mxfp4_window_ref as WR
    k, v = H.tokens(Hkv, H.LENGTHS[1])[j]
    q = H.per_sequence(H.packed_q(Hq), H.Q_LENS, j)
    O, lse, _ = WR.mxfp4_fwd_window(q.cpu(), k[None].cpu(), v[None].cpu(), W, S, kps)
    return O, lse


@pytest.mark.parametrize("kps", [64, 128])
@pytest.mark.parametrize("W,S", MASKS)
def test_general_masks_against_the_restatement(lib, W, S, kps):
    Hq, Hkv, lengths = 4, 2, H.LENGTHS[1]
    cache, q = H.pool(Hkv, lengths, 64, 32), H.packed_q(Hq)
    O, lse = _window(q, cache, H.SLOTS, H.Q_LENS, kps, W, S)
    for P, pages in POOLS[1:]:      # the page size changes no bit
        O2, lse2 = _window(q, H.pool(Hkv, lengths, P, pages), H.SLOTS, H.Q_LENS, kps, W, S)
        assert torch.equal(O, O2) and torch.equal(lse, lse2)
    for j in range(len(H.SLOTS)):
        RO, Rl = _restated(Hq, Hkv, j, W, S, kps)
        Oj, lj = H.per_sequence(O, H.Q_LENS, j).cpu(), H.per_sequence(lse, H.Q_LENS, j)[0].cpu()
        err = (Oj.float() - RO.float()).abs().max().item()
        lerr = (lj - Rl).abs().max().item()
        rel = ((Oj.float() - RO.float()).norm() / RO.float().norm()).item()
        print(f"MXFP4-WINDOW W={W} S={S} kps={kps} seq {j}: O {err:.3e} lse {lerr:.3e} relL2 {rel:.3e}")
        assert err <= 2e-2 and lerr <= 1e-4 and rel <= 2e-3, (j, err, lerr, rel)


# ------------------------------------------------------------------ 5. order and company
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_reversed_and_alone(lib, Hq, Hkv):
    W, S, lengths = 100, 4, H.LENGTHS[1]
    cache, q = H.pool(Hkv, lengths, 64, 32), H.packed_q(Hq)
    O, lse = _window(q, cache, H.SLOTS, H.Q_LENS, 64, W, S)
    n = len(H.SLOTS)
    qs = [H.per_sequence(q, H.Q_LENS, j)[0].transpose(0, 1) for j in range(n)]        # [n_j, Hq, D]
    rev = list(range(n))[::-1]
    rq, rlens = torch.cat([qs[j] for j in rev]), [H.Q_LENS[j] for j in rev]
    RO, Rl = _window(rq, cache, [H.SLOTS[j] for j in rev], rlens, 64, W, S)
    for pos, j in enumerate(rev):
        want = (H.per_sequence(O, H.Q_LENS, j), H.per_sequence(lse, H.Q_LENS, j)[0])
        H.assert_sequence_equals(RO, Rl, rlens, pos, want)
        AO, Al = _window(qs[j].contiguous(), cache, [H.SLOTS[j]], [H.Q_LENS[j]], 64, W, S)
        H.assert_sequence_equals(AO, Al, [H.Q_LENS[j]], 0, want)


# ------------------------------------------------------------------ 6. trim
def test_trim_changes_nothing_and_frees_what_it_says(lib):
    from quantizedattention_amd import _lib
    from quantizedattention_amd.kv_cache_mxfp4 import (attention_mxfp4_decode_paged,
                                                       attention_mxfp4_varlen_paged)
    Hq, Hkv, W, S, lengths = 4, 2, 130, 4, (700, 70)
    A, B, C = H.SLOTS[0], H.SLOTS[1], 1
    cache, twin = (_fill(Hkv, lengths, 64, 40, 12, H.SLOTS[:2]) for _ in range(2))
    g = torch.Generator().manual_seed(43)
    rand = lambda *s: torch.randn(s, generator=g).half().cuda()  # noqa: E731
    q = rand(4, Hq, 128)
    O, lse = _window(q, cache, [A, B], [1, 3], 64, W, S)
    free = cache.free_pages
    want = [p for p in range(11) if p * 64 >= S and (p + 1) * 64 <= 700 - W + 1]
    assert want == list(range(1, 8))
    assert cache.trim([A, B], W, S) == len(want) and cache.free_pages == free + len(want)
    assert cache.alloc.holes(A) == want and cache.alloc.holes(B) == []
    # the freed pages are overwritten by another sequence, the trimmed table entries made invalid
    dropped = set(twin.alloc.pages[A][1:8])
    k3, v3 = rand(300, Hkv, 128), rand(300, Hkv, 128)
    for c in (cache, twin):
        c.append_packed(k3, v3, [C], [300])
    assert set(cache.alloc.pages[C]) <= dropped
    cache.block_table[A, 1:8] = -1
    O2, lse2 = _window(q, cache, [A, B], [1, 3], 64, W, S)
    assert torch.equal(O, O2) and torch.equal(lse, lse2)
    # one more token, decoded under the window: the untrimmed twin's bits
    k1, v1, q1 = rand(1, Hkv, 128), rand(1, Hkv, 128), rand(1, Hq, 128)
    outs = []
    for c in (cache, twin):
        c.append_packed(k1, v1, [A], [1])
        outs.append(_window(q1, c, [A], [1], 64, W, S))
    assert cache.lengths[A] == 701 and cache.capacity_tokens(A) == 11 * 64
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    # whatever would read a hole raises before any launch and changes nothing
    a = cache.alloc
    cache.block_table[A, 1:8] = -1      # (the append re-uploaded the host table)
    dev = [t.clone() for t in (*cache.kv, cache.vtail, cache.lens, cache.block_table)]
    host = (list(cache.lengths), list(a._free), list(a.refcount), [list(p) for p in a.pages],
            [list(r) for r in a.table])

    def unchanged():
        torch.cuda.synchronize()
        assert host == (list(cache.lengths), list(a._free), list(a.refcount), [list(p) for p in a.pages],
                        [list(r) for r in a.table])
        for x, y in zip(dev, (*cache.kv, cache.vtail, cache.lens, cache.block_table)):
            assert torch.equal(x, y)

    for call in (lambda: attention_mxfp4_varlen_paged(q1, cache, [A], [1], causal=True),
                 lambda: attention_mxfp4_varlen_paged(q1, cache, [A], [1]),
                 lambda: _window(q1, cache, [A], [1], 64, W + 64, S),
                 lambda: _window(q1, cache, [A], [1], 64, W, 65),
                 lambda: _window(q, cache, [A, B], [1, 3], 64, 1 << 40, 0),
                 lambda: cache.gather(A), lambda: cache.snapshot(A), lambda: cache.fork(A, 3)):
        with pytest.raises(_lib.QAttnError, match="trimmed"):
            call()
        unchanged()
    for b in range(H.MAX_SEQS):          # the padded decode needs every slot filled
        if cache.lengths[b] == 0:
            cache.append_packed(k1, v1, [b], [1])
    host = (list(cache.lengths), list(a._free), list(a.refcount), [list(p) for p in a.pages],
            [list(r) for r in a.table])
    cache.block_table[A, 1:8] = -1
    dev = [t.clone() for t in (*cache.kv, cache.vtail, cache.lens, cache.block_table)]
    with pytest.raises(_lib.QAttnError, match="trimmed"):
        attention_mxfp4_decode_paged(rand(H.MAX_SEQS, Hq, 1, 128), cache)
    unchanged()
    _window(q1, cache, [A], [1], 64, W, S)      # the window the holes allow still runs
    free = cache.free_pages
    cache.free([A])                              # the four pages it still held
    assert cache.free_pages == free + 4 and cache.lengths[A] == 0 and a.pages[A] == []


# ------------------------------------------------------------------ 7. the C entry on flat buffers
def test_nothing_is_written_past_the_buffers(lib):
    """The windowed entry and the merge on flat buffers with 128 sentinel rows behind opart, ml, O and lse:
    every partial row is written, nothing past the end; a partial row is the empty state exactly where its
    query sees no key of the split's tiles, and the merged row never is.  (With S >= 1 every query sees key
    0, so a row of a sink split is never empty; the empty rows lie in the splits wholly above a row's
    diagonal or wholly below its window, as in the causal call.)"""
    import mxfp4_window_ref as WR
    from quantizedattention_amd import _lib
    from quantizedattention_amd.attention_mxfp4 import _qk_scale, mxfp4_quantize_rows
    from quantizedattention_amd.kv_cache_mxfp4 import plan_varlen
    SENT, D, pad, W, S = -12288.0, 128, 128, 100, 4
    Hq, Hkv, lengths = 4, 2, H.LENGTHS[1]
    cache, q = H.pool(Hkv, lengths, 64, 32), H.packed_q(Hq)
    T = q.shape[0]
    kps, rec, work, rows = plan_varlen(cache.lengths, H.SLOTS, H.Q_LENS, Hq, Hkv, 64, True, W, S)
    # (64, 1): one tile; (130, 3): tiles 0..2, the runs touch; (256, 33): lo = 124, tiles 1..3 after the sink
    # tile: a gap of none, they touch; (70, 70): two tiles
    assert [r[3] for r in rec] == [1, 3, 4, 2] and [r[5:7] for r in rec] == [[0, 0]] * 4
    rec_d, work_d = (torch.tensor(t, dtype=torch.int32).cuda() for t in (rec, work))
    q4, qs = mxfp4_quantize_rows(q)
    opart = torch.full(((rows + pad) * D,), SENT, dtype=torch.float32, device="cuda")
    ml = torch.full(((rows + pad) * 2,), SENT, dtype=torch.float32, device="cuda")
    out = torch.full(((T * Hq + pad) * D,), SENT, dtype=torch.float16, device="cuda")
    lse = torch.full((T * Hq + pad,), SENT, dtype=torch.float32, device="cuda")
    st = _lib.stream_of(q)
    args = (_lib.ptr(q4), _lib.ptr(qs), *(_lib.ptr(t) for t in cache.kv), _lib.ptr(opart), _lib.ptr(ml),
            _lib.ptr(cache.lens), _lib.ptr(cache.block_table), _lib.ptr(rec_d), _lib.ptr(work_d), len(rec),
            len(work), T, rows, H.MAX_SEQS, Hkv, Hq // Hkv, cache.num_pages, 64, cache.alloc.max_pages_per_seq)
    lib_ = _lib.load()
    for causal, w, s in ((0, W, S), (1, W, S), (2, 0, S), (2, W, -1)):     # refused: status 1, no launch
        assert lib_.qattn_mxfp4_attn_fwd_varlen_paged_window(*args, causal, kps, D, _qk_scale(D), w, s, st) == 1
    torch.cuda.synchronize()
    assert (opart == SENT).all() and (ml == SENT).all()
    _lib.call("qattn_mxfp4_attn_fwd_varlen_paged_window", *args, 2, kps, D, _qk_scale(D), W, S, st)
    torch.cuda.synchronize()
    for t in (opart[rows * D:], ml[rows * 2:], out, lse):
        assert t.numel() >= 128 and (t == SENT).all()
    m = ml[:rows * 2].view(rows, 2)
    assert not (opart[:rows * D] == SENT).any() and not (m == SENT).any()
    empty = m[:, 0] == float("-inf")
    # where the mask says so and nowhere else: row r of split s of sequence j (rows [split][kv head][g * n + i])
    want, G = torch.zeros(rows, dtype=torch.bool), Hq // Hkv
    for r_, L, n in zip(rec, lengths, H.Q_LENS):
        vis = WR.visible(n, L, -(-L // 64) * 64, W, S)
        for s_, (lo, hi) in enumerate(WR.split_tiles(L, n, W, S, kps)):
            none = ~vis[:, 64 * lo:64 * hi].any(1)                    # per query i
            want[r_[4] + s_ * Hkv * G * n:r_[4] + (s_ + 1) * Hkv * G * n] = none.repeat(Hkv * G)
    assert want.any() and torch.equal(empty.cpu(), want)
    assert (m[empty, 1] == 0).all() and (opart[:rows * D].view(rows, D)[empty] == 0).all()
    assert torch.isfinite(m[~empty]).all() and (m[~empty, 1] > 0).all()
    _lib.call("qattn_mxfp4_varlen_combine", _lib.ptr(opart), _lib.ptr(ml), _lib.ptr(out), _lib.ptr(lse),
              _lib.ptr(rec_d), len(rec), T, Hq, Hkv, rows, D, st)
    torch.cuda.synchronize()
    for t in (opart[rows * D:], ml[rows * 2:], out[T * Hq * D:], lse[T * Hq:]):
        assert t.numel() >= 128 and (t == SENT).all()
    O, l2 = _window(q, cache, H.SLOTS, H.Q_LENS, 64, W, S)             # finite: every merged l > 0
    assert torch.equal(out[:T * Hq * D].view(T, Hq, D), O) and torch.equal(lse[:T * Hq].view(T, Hq), l2)


# ------------------------------------------------------------------ 8. the operator
def test_operator_equals_the_python_call(lib):
    import quantizedattention_amd.ops as ops
    from quantizedattention_amd.kv_cache_mxfp4 import plan_varlen
    Hq, Hkv, lengths = 4, 2, H.LENGTHS[1]
    cache, q = H.pool(Hkv, lengths, 64, 32), H.packed_q(Hq)
    for W, S, split in ((100, 4, 128), (37, 64, None)):
        O, lse = _window(q, cache, H.SLOTS, H.Q_LENS, split, W, S)
        O1, l1 = ops.mxfp4_varlen_paged(q, cache, H.SLOTS, H.Q_LENS, causal=True, keys_per_split=split,
                                        window=W, sinks=S)
        assert torch.equal(O, O1) and torch.equal(lse, l1)
        kps, rec, work, rows = plan_varlen(cache.lengths, H.SLOTS, H.Q_LENS, Hq, Hkv, split, True, W, S)
        args = (q, *cache.kv, cache.lens, cache.block_table, torch.tensor(rec, dtype=torch.int32).cuda(),
                torch.tensor(work, dtype=torch.int32).cuda(), rows, 1, kps, W, S)
        O2, l2 = torch.ops.qattn.mxfp4_varlen_paged_window(*args)
        assert O2.dtype == torch.float16 and l2.dtype == torch.float32
        assert torch.equal(O, O2) and torch.equal(lse, l2)
    op = torch.ops.qattn.mxfp4_varlen_paged_window
    torch.library.opcheck(op, args, test_utils="test_faketensor")
    for bad in ((*args[:-2], 0, S), (*args[:-2], W, -1), (*args[:10], 0, *args[11:]), (*args[:11], 96, W, S),
                (q[:, :3], *args[1:])):
        with pytest.raises(RuntimeError):
            op(*bad)
