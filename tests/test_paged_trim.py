"""Releasing pages behind a window: PageAllocator.drop and the pages PagedKVFP4.trim picks.  Host only:
no device, no kernel (the pool's tensors are never touched by either).
"""
import pytest

from quantizedattention_amd import _lib
from quantizedattention_amd.kv_cache_mxfp4 import PageAllocator, PagedKVFP4


def _state(a):
    assert a.nholes == [p.count(None) for p in a.pages]
    return (list(a._free), list(a.refcount), [list(p) for p in a.pages], [list(r) for r in a.table])


def test_drop_makes_holes_and_frees_in_order():
    a = PageAllocator(10, 64, 3, 8, free_order=[7, 3, 9, 1, 0, 2, 4, 5, 6, 8])
    a.reserve([(0, 5 * 64), (1, 64)])
    assert a.pages[0] == [7, 3, 9, 1, 0] and a.pages[1] == [2] and a.free_pages == 4
    assert a.drop(0, 1, 3) == 2
    assert a.pages[0] == [7, None, None, 1, 0] and len(a.pages[0]) == 5
    assert a.refcount[3] == 0 and a.refcount[9] == 0 and a.free_pages == 6
    assert a.nholes == [2, 0, 0]
    assert a.holes(0) == [1, 2] and a.holes(0, 2) == [2] and a.holes(0, 3, 5) == [] and a.holes(1) == []
    # dropped pages are the next handed out (the last dropped first), before the untouched free pages
    a.reserve([(1, 3 * 64)])
    assert a.pages[1] == [2, 9, 3]
    # dropping a hole again changes nothing
    before = _state(a)
    assert a.drop(0, 1, 3) == 0 and _state(a) == before
    assert a.drop(0, 2, 2) == 0 and _state(a) == before


def test_reserve_and_release_with_holes():
    a = PageAllocator(8, 64, 2, 8)
    a.reserve([(0, 4 * 64)])
    a.drop(0, 0, 2)
    assert a.pages_for(4 * 64 + 1) == 5
    assert a.reserve([(0, 4 * 64 + 1)]) == [0]            # the logical page count goes on from 4
    assert len(a.pages[0]) == 5 and a.pages[0][:2] == [None, None] and a.table[0][4] == a.pages[0][4]
    assert a.reserve([(0, 5 * 64)]) == []                 # capacity counts the holes
    free = a.free_pages
    a.release(0)                                          # three real pages come back, the holes are skipped
    assert a.pages[0] == [] and a.free_pages == free + 3 == 8 and a.refcount == [0] * 8 and a.nholes == [0, 0]
    assert sorted(a._free) == list(range(8))


def test_shared_pages_lose_one_reference():
    a = PageAllocator(8, 64, 3, 4)
    a.reserve([(0, 3 * 64)])
    a.share(0, 1, 3)
    assert [a.refcount[p] for p in a.pages[0]] == [2, 2, 2] and a.free_pages == 5
    assert a.drop(0, 0, 2) == 0                           # still held by the fork: nothing returns
    assert a.pages[0] == [None, None, 2] and a.pages[1] == [0, 1, 2]
    assert [a.refcount[p] for p in a.pages[1]] == [1, 1, 2] and a.free_pages == 5
    assert a.drop(1, 0, 1) == 1 and a.refcount[0] == 0 and a.free_pages == 6
    with pytest.raises(_lib.QAttnError, match="trimmed"):
        a.share(1, 2, 2)                                  # a hole cannot be shared
    a.share(0, 2, 0)                                      # no page asked for: fine
    a.release(0)
    a.release(1)
    a.release(2)
    assert a.free_pages == 8 and a.refcount == [0] * 8


def test_refused_drop_changes_nothing():
    a = PageAllocator(6, 64, 2, 4)
    a.reserve([(0, 3 * 64)])
    before = _state(a)
    for args in ((0, 2, 4), (0, -1, 2), (0, 2, 1), (2, 0, 1), (1, 0, 1)):
        with pytest.raises(_lib.QAttnError):
            a.drop(*args)
        assert _state(a) == before


def _pool(P, L, pages=40):
    """A PagedKVFP4 without tensors (trim touches none) holding one sequence of L tokens in slot 1."""
    alloc = PageAllocator(pages, P, 3, pages)
    cache = PagedKVFP4(None, None, None, None, None, None, None, alloc)
    alloc.reserve([(1, L)])
    cache.lengths[1] = L
    return cache


def _dropped(P, L, W, S):
    cache = _pool(P, L)
    free = cache.free_pages
    n = cache.trim([1], W, S)
    holes = cache.alloc.holes(1)
    assert n == len(holes) == cache.free_pages - free
    # the definition: the pages none of whose keys a query at a position >= L can see
    want = [p for p in range(-(-L // P)) if p * P >= S and (p + 1) * P <= L - W + 1]
    assert holes == want, (P, L, W, S)
    # every key a query at position L (the next token) or later sees lies in a page that is left
    for k in list(range(min(S, L))) + list(range(max(0, L - W + 1), L)):
        assert k // P not in holes
    return holes


@pytest.mark.parametrize("P", [64, 256])
def test_trim_edges(P):
    # L - W + 1 exactly on a page boundary: the page below it goes; one below the boundary: it stays
    assert _dropped(P, 5 * P + 9, 10, 0) == [0, 1, 2, 3, 4]           # L - W + 1 = 5 P
    assert _dropped(P, 5 * P + 8, 10, 0) == [0, 1, 2, 3]              # 5 P - 1
    assert _dropped(P, 5 * P, 1, 0) == [0, 1, 2, 3, 4]                # W = 1: every full page
    assert _dropped(P, 5 * P - 1, 1, 0) == [0, 1, 2, 3]               # the partial last page never
    # sinks: page 0 is kept by one sink key, page 1 by the key after P
    assert _dropped(P, 6 * P, P, 0) == [0, 1, 2, 3, 4]
    assert _dropped(P, 6 * P, P, 1) == [1, 2, 3, 4]
    assert _dropped(P, 6 * P, P, P) == [1, 2, 3, 4]
    assert _dropped(P, 6 * P, P, P + 1) == [2, 3, 4]
    assert _dropped(P, 6 * P, P, 7 * P) == []
    # a window that covers the sequence drops nothing
    for W in (6 * P, 6 * P + 1, 1 << 40):
        assert _dropped(P, 6 * P, W, 0) == []
    assert _dropped(P, 1, 1, 0) == [] and _dropped(P, P, 2, 0) == []


def test_trim_twice_and_append_after():
    cache = _pool(64, 700)
    assert cache.trim([1], 130, 4) == 7                   # pages 1 .. 7; 700 - 130 + 1 = 571 = 8 * 64 + 59
    assert cache.alloc.holes(1) == list(range(1, 8))
    assert cache.trim([1], 130, 4) == 0 and cache.trim([1], 500, 4) == 0
    assert cache.capacity_tokens(1) == 11 * 64
    cache.alloc.reserve([(1, 705)])
    cache.lengths[1] = 769                                # as an append of 69 tokens would leave it
    assert cache.alloc.reserve([(1, 769)]) == [1] and len(cache.alloc.pages[1]) == 13
    assert cache.trim([1], 130, 4) == 2 and cache.alloc.holes(1) == list(range(1, 10))
    with pytest.raises(_lib.QAttnError, match="window"):
        cache.trim([1], 0)
    with pytest.raises(_lib.QAttnError, match="window"):
        cache.trim([1], None)
    with pytest.raises(_lib.QAttnError, match="no sequence"):
        cache.trim([5], 4)


def test_decode_paged_refuses_a_trimmed_pool(monkeypatch):
    import torch
    z = lambda *s, dt=torch.uint8: torch.zeros(s, dtype=dt)  # noqa: E731
    alloc = PageAllocator(8, 64, 2, 4)
    cache = PagedKVFP4(z(8, 2, 64, 64), z(8, 2, 64, 4), z(8, 2, 1, 128, 32), z(8, 2, 1, 128, 2),
                       z(2, 2, 64, 128, dt=torch.float16), z(2, dt=torch.int32), z(2, 4, dt=torch.int32), alloc)
    alloc.reserve([(0, 10), (1, 200)])
    cache.lengths = [10, 200]
    assert cache.trim([1], 64, 0) == 2
    from quantizedattention_amd.kv_cache_mxfp4 import attention_mxfp4_decode_paged

    def trap(*a, **k):
        raise AssertionError("a tensor was made before the error was raised")
    monkeypatch.setattr(torch, "tensor", trap)
    monkeypatch.setattr(torch, "empty", trap)
    with pytest.raises(_lib.QAttnError, match="trimmed"):
        attention_mxfp4_decode_paged(z(2, 4, 1, 128, dt=torch.float16), cache, keys_per_split=64)
