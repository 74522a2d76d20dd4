"""Checkpoint, rollback and accept on the paged MX-FP4 cache on the GPU (PagedKVFP4.checkpoint / rollback /
accept, qattn_mxfp4_paged_rollback, PageAllocator.shrink).

The instrument is exact: a twin pool that only ever appends what survives.  After ``rollback`` the pool holds,
byte for byte, what the twin holds -- rows [0, L0) of k4 / ks, tiles [0, ceil(L0 / 64)) of vt / vs (the tile at
L0 // 64 quantised again from the saved rows, the drafts' scales gone), vtail rows [0, L0 % 64), lens, the
free-page count -- and after ``accept`` again, so that attention over both pools gives the same bits.  Every
refusal leaves host and device state unchanged.
"""
import dataclasses

import pytest
import torch

import mxfp4_varlen_helpers as H

pytestmark = pytest.mark.gpu

HQ, HKV = 4, 2
A, B, FREE, OTHER = 2, 0, 1, 3      # the rolled-back slot, its neighbour, a slot that stays free, a taker of pages
LB = 70
#        L0  drafts  kept
CASES = [(60, 10, 3),     # crosses a tile and, at P = 64, a page
         (64, 8, 8),      # L0 on a tile boundary
         (130, 5, 0),     # nothing kept
         (1, 64, 2),      # the shortest prefix, the longest draft
         (200, 64, 5),    # crosses a tile and, at P = 256, a page
         (0, 7, 1),       # an empty sequence
         (63, 1, 0)]      # a single draft, nothing kept


def _rand(g, *shape):
    return torch.randn(shape, generator=g).half().cuda()


def _pool(P, pages=24, tokens=768):
    from quantizedattention_amd.kv_cache_mxfp4 import PagedKVFP4
    return PagedKVFP4.allocate(pages, P, 4, HKV, -(-tokens // P), "cuda", free_order=H.scatter(pages))


def _same(cache, twin, slots=(A, B, OTHER)):
    """The invariant, slot by slot against the twin, through each pool's own device table."""
    assert cache.lengths == twin.lengths and cache.lens.cpu().tolist() == cache.lengths
    assert twin.lens.cpu().tolist() == twin.lengths
    assert cache.free_pages == twin.free_pages
    for b in slots:
        L = cache.lengths[b]
        assert len(cache.alloc.pages[b]) == len(twin.alloc.pages[b]) == -(-L // cache.page_tokens), b
        if L == 0:
            continue
        for x, y in zip(H.gather(cache, b), H.gather(twin, b)):
            assert torch.equal(x, y), (b, L)
        assert torch.equal(cache.vtail[b, :, :L % 64], twin.vtail[b, :, :L % 64]), (b, L)


def _attend(cache, twin, q, ids, q_lens, **kw):
    from quantizedattention_amd.kv_cache_mxfp4 import attention_mxfp4_varlen_paged
    O, lse = attention_mxfp4_varlen_paged(q, cache, ids, q_lens, causal=True, keys_per_split=64, **kw)
    TO, Tl = attention_mxfp4_varlen_paged(q, twin, ids, q_lens, causal=True, keys_per_split=64, **kw)
    assert torch.isfinite(lse).all() and torch.equal(O, TO) and torch.equal(lse, Tl)


@pytest.mark.parametrize("L0,drafts,kept", CASES)
@pytest.mark.parametrize("P", [64, 256])
def test_rollback_and_accept_against_the_twin(lib, P, L0, drafts, kept):
    g = torch.Generator().manual_seed(1000 * L0 + drafts)
    cache, twin = _pool(P), _pool(P)
    ids, cnt = ([A, B], [L0, LB]) if L0 else ([B], [LB])
    k0, v0 = _rand(g, sum(cnt), HKV, 128), _rand(g, sum(cnt), HKV, 128)
    for c in (cache, twin):
        c.append_packed(k0, v0, ids, cnt)
    ckpt = cache.checkpoint([B, A])
    free0, pages0 = cache.free_pages, list(cache.alloc.pages[A])
    # the draft step: `drafts` tokens for A; B decodes a real token in both pools and is not rolled back
    kd, vd = _rand(g, drafts, HKV, 128), _rand(g, drafts, HKV, 128)
    kb, vb = _rand(g, 1, HKV, 128), _rand(g, 1, HKV, 128)
    cache.append_packed(kd, vd, [A], [drafts])
    for c in (cache, twin):
        c.append_packed(kb, vb, [B], [1])
    taken = [p for p in cache.alloc.pages[A] if p not in pages0]
    assert len(taken) == -(-(L0 + drafts) // P) - -(-L0 // P) and cache.lengths[A] == L0 + drafts
    assert cache.rollback(ckpt, [A]) is cache
    assert cache.lengths[A] == L0 and cache.alloc.pages[A] == pages0 and cache.free_pages == free0
    _same(cache, twin)
    # the released pages are handed out to another sequence and overwritten
    n = max(len(taken), 1) * P
    ko, vo = _rand(g, n, HKV, 128), _rand(g, n, HKV, 128)
    for c in (cache, twin):
        c.append_packed(ko, vo, [OTHER], [n])
    assert set(taken) <= set(cache.alloc.pages[OTHER]) and cache.lengths[FREE] == 0
    _same(cache, twin)
    # a second draft round through the same checkpoint, accepted
    kd, vd = _rand(g, drafts, HKV, 128), _rand(g, drafts, HKV, 128)
    cache.append_packed(kd, vd, [A], [drafts])
    keep = sorted(torch.randperm(drafts, generator=g)[:kept].tolist())
    assert cache.accept(ckpt, kd, vd, [A], [drafts], [keep]) is cache
    if kept:
        idx = torch.tensor(keep).cuda()
        twin.append_packed(kd[idx], vd[idx], [A], [kept])
    assert cache.lengths[A] == L0 + kept
    _same(cache, twin)
    if L0 + kept:
        nA = min(3, L0 + kept)
        _attend(cache, twin, _rand(g, nA + 2, HQ, 128), [A, B], [nA, 2])
    # one more decode token
    k1, v1 = _rand(g, 2, HKV, 128), _rand(g, 2, HKV, 128)
    for c in (cache, twin):
        c.append_packed(k1, v1, [B, A], [1, 1])
    _same(cache, twin)
    _attend(cache, twin, _rand(g, 2, HQ, 128), [A, B], [1, 1])


def test_accept_of_several_sequences(lib):
    """Two sequences drafted in one step, one keeps a path and one keeps nothing; a third is left alone."""
    from quantizedattention_amd.kv_cache_mxfp4 import tree_path
    g = torch.Generator().manual_seed(7)
    cache, twin = _pool(64), _pool(64)
    k0, v0 = _rand(g, 60 + LB + 130, HKV, 128), _rand(g, 60 + LB + 130, HKV, 128)
    for c in (cache, twin):
        c.append_packed(k0, v0, [A, B, OTHER], [60, LB, 130])
    ckpt = cache.checkpoint([A, B, OTHER])
    parents = [-1, 0, 0, 1, 1, 2, 2, 3, 5, 8]
    kd, vd = _rand(g, 10 + 6, HKV, 128), _rand(g, 10 + 6, HKV, 128)
    cache.append_packed(kd, vd, [OTHER, A], [10, 6])
    path = tree_path(parents, 9)
    assert path == [0, 2, 5, 8, 9]
    cache.accept(ckpt, kd, vd, [OTHER, A], [10, 6], [path, []])
    twin.append_packed(kd[torch.tensor(path).cuda()], vd[torch.tensor(path).cuda()], [OTHER], [5])
    assert cache.lengths[A] == 60 and cache.lengths[OTHER] == 135
    _same(cache, twin)
    _attend(cache, twin, _rand(g, 6, HQ, 128), [OTHER, A, B], [3, 2, 1])
    for bad in ([path], [path, [6]], [[0, 0], []], [path, [-1]]):
        with pytest.raises(RuntimeError, match="accepted"):
            cache.accept(ckpt, kd, vd, [OTHER, A], [10, 6], bad)
    _same(cache, twin)


def test_refusals_change_nothing(lib):
    from quantizedattention_amd import _lib
    g = torch.Generator().manual_seed(11)
    cache = _pool(64)
    k0, v0 = _rand(g, 70 + LB, HKV, 128), _rand(g, 70 + LB, HKV, 128)
    cache.append_packed(k0, v0, [A, B], [70, LB])
    a = cache.alloc

    def state():
        torch.cuda.synchronize()
        return ((list(cache.lengths), list(cache.epoch), list(a._free), list(a.refcount), [list(p) for p in a.pages],
                 list(a.nholes), [list(r) for r in a.table]),
                [t.clone() for t in (*cache.kv, cache.vtail, cache.lens, cache.block_table)])

    def refused(reason, ckpt, seq_ids=None):
        host, dev = state()
        saved, stamp = ckpt.saved.clone(), list(ckpt.epochs)
        with pytest.raises(_lib.QAttnError, match=reason):
            cache.rollback(ckpt, seq_ids)
        host2, dev2 = state()
        assert host == host2 and all(torch.equal(x, y) for x, y in zip(dev, dev2))
        assert torch.equal(saved, ckpt.saved) and stamp == ckpt.epochs

    # "shorter": a checkpoint that claims more tokens than the sequence holds (no call of the pool's own
    # makes one: whatever shortens a sequence also makes its checkpoints stale)
    ckpt = cache.checkpoint([A, B])
    refused("shorter", dataclasses.replace(ckpt, lengths=[71, LB]))
    # "shared": a fork after the checkpoint shares the page that holds position L0 = 70
    kd, vd = _rand(g, 58, HKV, 128), _rand(g, 58, HKV, 128)
    cache.append_packed(kd, vd, [A], [58])
    cache.fork(A, OTHER)
    assert a.refcount[a.pages[A][1]] == 2
    refused("shared", ckpt)
    refused("shared", ckpt, [A])
    cache.rollback(ckpt, [B])                   # B is not shared; and the checkpoint still serves A afterwards
    cache.free([OTHER])
    cache.rollback(ckpt, [A])
    assert cache.lengths[A] == 70
    # "stale": rolled back through another checkpoint, trimmed, freed
    older = cache.checkpoint([A])
    cache.append_packed(kd, vd, [A], [58])
    newer = cache.checkpoint([A])
    cache.rollback(older)
    refused("stale", newer)
    cache.rollback(older)                       # stamped again: it serves the next round
    ckpt = cache.checkpoint([A, B])
    cache.trim([A], 16)
    refused("stale", ckpt, [A])
    refused("stale", ckpt)
    cache.rollback(ckpt, [B])
    ckpt = cache.checkpoint([B])
    cache.free([B])
    refused("stale", ckpt)
    cache.append_packed(k0[:LB], v0[:LB], [B], [LB])
    refused("stale", ckpt)
    # a checkpoint of another pool, a sequence the checkpoint does not hold
    refused("checkpoint", _pool(64).checkpoint([B]))
    refused("checkpoint", cache.checkpoint([B]), [A])


def test_rollback_below_trim_holes(lib):
    """A sequence with trim holes below L0 rolls back, and its windowed call still equals the untrimmed twin's."""
    from quantizedattention_amd.kv_cache_mxfp4 import attention_mxfp4_varlen_paged
    g = torch.Generator().manual_seed(13)
    W, S, L0 = 130, 4, 700
    cache, twin = _pool(64, 40), _pool(64, 40)
    k0, v0 = _rand(g, L0 + LB, HKV, 128), _rand(g, L0 + LB, HKV, 128)
    for c in (cache, twin):
        c.append_packed(k0, v0, [A, B], [L0, LB])
    assert cache.trim([A], W, S) == 7
    holes = cache.alloc.holes(A)
    ckpt = cache.checkpoint([A])
    kd, vd = _rand(g, 60, HKV, 128), _rand(g, 60, HKV, 128)
    cache.append_packed(kd, vd, [A], [60])      # 700 -> 760: into the next tile and the next page
    free = cache.free_pages
    cache.rollback(ckpt)
    assert cache.lengths[A] == L0 and cache.alloc.holes(A) == holes and cache.alloc.nholes[A] == 7
    assert cache.free_pages == free + 1 and len(cache.alloc.pages[A]) == 11
    q = _rand(g, 3, HQ, 128)
    _attend(cache, twin, q, [A, B], [1, 2], window=W, sinks=S)
    cache.append_packed(kd, vd, [A], [60])
    cache.accept(ckpt, kd, vd, [A], [60], [[0, 3, 59]])
    idx = torch.tensor([0, 3, 59]).cuda()
    twin.append_packed(kd[idx], vd[idx], [A], [3])
    _attend(cache, twin, q, [A, B], [2, 1], window=W, sinks=S)
    with pytest.raises(RuntimeError, match="trimmed"):
        attention_mxfp4_varlen_paged(q, cache, [A, B], [2, 1], causal=True)
