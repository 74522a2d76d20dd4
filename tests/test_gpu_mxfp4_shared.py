"""Shared-prefix attention over the paged MX-FP4 cache: attention_mxfp4_varlen_paged(share_prefix=True).

The specification is one equality: the shared call returns, bit for bit, what the same call without
``share_prefix`` returns at the same explicit ``keys_per_split`` -- O and lse, grouped and ungrouped
sequences alike.  Every comparison below is torch.equal against that call on the same pool and stream.
Before the calls of a group case the plan is asked whether the group path is taken at all, and the
shared call's fresh buffers (torch.empty) are filled with NaN, so a partial row that no workgroup wrote
cannot pass by holding what an earlier call left in the same memory.

Shapes are the smallest at which each mechanism can go wrong (Hkv = 2, G = 2 unless said): see the cases.
"""
import contextlib
import functools

import pytest
import torch

from mxfp4_varlen_helpers import scatter

pytestmark = pytest.mark.gpu
D = 128


@functools.lru_cache(maxsize=None)
def pool(P, Hkv, ops, max_seqs=8, num_pages=40, mpp=6, smooth=False, scattered=False, seed=5):
    """A pool after ``ops``: ("app", slot, n) appends n random tokens, ("fork", src, dst) forks.  Shared
    between tests: do not modify."""
    from quantizedattention_amd.kv_cache_mxfp4 import PagedKVFP4
    g = torch.Generator().manual_seed(seed)
    k_mean = (0.5 * torch.randn((max_seqs, Hkv, 1, D), generator=g)).half() if smooth else None
    cache = PagedKVFP4.allocate(num_pages, P, max_seqs, Hkv, mpp, "cuda", k_mean=k_mean,
                                free_order=scatter(num_pages) if scattered else None)
    for op in ops:
        if op[0] == "fork":
            cache.fork(op[1], op[2])
        else:
            k = torch.randn((op[2], Hkv, D), generator=g).half().cuda()
            v = torch.randn((op[2], Hkv, D), generator=g).half().cuda()
            cache.append_packed(k, v, [op[1]], [op[2]])
    return cache


@contextlib.contextmanager
def poisoned_empty():
    """torch.empty gives NaN (floating) or 0xff (integer) instead of whatever the allocator holds."""
    real = torch.empty

    def empty(*a, **k):
        t = real(*a, **k)
        return t.fill_(float("nan")) if t.is_floating_point() else t.fill_(255)
    torch.empty = empty
    try:
        yield
    finally:
        torch.empty = real


def plan_of(cache, ids, q_lens, Hq, causal, kps):
    from quantizedattention_amd.kv_cache_mxfp4 import plan_varlen_shared
    return plan_varlen_shared(cache.lengths, ids, q_lens, Hq, cache.shape[1], cache.prefix_groups(ids), kps,
                              causal, page_tokens=cache.page_tokens)


def check(cache, ids, q_lens, Hq, causal, kps, shared_splits, seed=41):
    """The shared call against the plain one; ``shared_splits``: ns_g of every group the plan must hold
    (an empty list: no group, the plain call is made)."""
    from quantizedattention_amd.kv_cache_mxfp4 import attention_mxfp4_varlen_paged
    plan = plan_of(cache, ids, q_lens, Hq, causal, kps)
    assert [g[2] for g in plan[4]] == list(shared_splits)
    assert sum(w[3] for w in plan[2]) == sum(ns * -(-R // 128) for _, _, ns, R in plan[4])
    q = torch.randn((sum(q_lens), Hq, D), generator=torch.Generator().manual_seed(seed)).half().cuda()
    O, lse = attention_mxfp4_varlen_paged(q, cache, ids, q_lens, causal=causal, keys_per_split=kps)
    with poisoned_empty():
        SO, Slse = attention_mxfp4_varlen_paged(q, cache, ids, q_lens, causal=causal, keys_per_split=kps,
                                                share_prefix=True)
    assert not torch.isnan(O.float()).any() and not torch.isnan(lse).any()
    assert torch.equal(SO, O)
    assert torch.equal(Slse, lse)
    return q, O, lse


# prompt of 192 keys (3 pages of 64) in slot 0, forked into slots 1..3, which append 1, 70 and 1 own tokens
FORKS3 = (("app", 0, 192), ("fork", 0, 1), ("fork", 0, 2), ("fork", 0, 3), ("app", 1, 1), ("app", 2, 70),
          ("app", 3, 1))
# the same, the forks appending 5, 71 and 3
CHUNKS3 = FORKS3[:4] + (("app", 1, 5), ("app", 2, 71), ("app", 3, 3))


@pytest.mark.parametrize("kps,ns", [(64, 3), (128, 1)])
def test_decode_forks(kps, ns):
    """1: three forks decode one token each; at kps 128 the split [128, 256) stays per sequence."""
    check(pool(64, 2, FORKS3), [1, 2, 3], [1, 1, 1], 4, True, kps, [ns])


@pytest.mark.parametrize("causal", [True, False])
def test_wave_crosses_member_boundaries(causal):
    """2: q_lens 5, 1, 3 after appending that many: 18 stacked rows in one wave, three values of sq."""
    check(pool(64, 2, CHUNKS3), [1, 2, 3], [5, 1, 3], 4, causal, 64, [3])


def test_diagonal_inside_the_common_pages():
    """2b: 5 queries over 193 keys see only 189 of them all: the third common page stays per sequence."""
    check(pool(64, 2, FORKS3), [1, 2, 3], [5, 1, 3], 4, True, 64, [2])
    check(pool(64, 2, FORKS3), [1, 2, 3], [5, 1, 3], 4, False, 64, [3])


def test_second_row_block():
    """3: 33 forks, G = 4, one token each: 132 stacked rows, a second row block of 4 rows, three idle waves."""
    ops = (("app", 0, 128),) + tuple(("fork", 0, b) for b in range(1, 34)) + tuple(
        ("app", b, 1) for b in range(1, 34))
    cache = pool(64, 2, ops, max_seqs=34, num_pages=40, mpp=3)
    plan = plan_of(cache, list(range(1, 34)), [1] * 33, 8, True, 64)
    assert plan[4] == [[0, 33, 2, 132]] and [w for w in plan[2] if w[3] == 1 and w[1] == 1]
    check(cache, list(range(1, 34)), [1] * 33, 8, True, 64, [2])


def test_two_groups_a_loner_and_an_empty_slot():
    """4: groups of different prompts and different ns_g, an unrelated sequence, slot 3 empty and unlisted,
    seq_ids not ascending."""
    ops = (("app", 0, 192), ("fork", 0, 1), ("fork", 0, 2), ("app", 4, 64), ("fork", 4, 5), ("app", 6, 100),
           ("app", 0, 2), ("app", 1, 4), ("app", 2, 66), ("app", 4, 1), ("app", 5, 130))
    cache = pool(64, 2, ops)
    assert cache.lengths[3] == 0
    ids, q_lens = [5, 2, 6, 0, 4, 1], [1, 2, 3, 1, 1, 4]
    assert cache.prefix_groups(ids) == [([0, 4], 1), ([1, 3, 5], 3)]
    for causal in (True, False):
        check(cache, ids, q_lens, 4, causal, 64, [1, 3])
    check(cache, ids, q_lens, 4, True, 128, [1])          # the 64-key group dissolves


def test_fork_of_a_fork_and_a_copied_page():
    """5: a fork of a fork (2 common pages of 3) and a source forked at L % P != 0, whose copied page is
    read per sequence."""
    ops = (("app", 0, 128), ("fork", 0, 1), ("app", 1, 64), ("fork", 1, 2), ("app", 0, 70), ("app", 1, 10),
           ("fork", 1, 3), ("app", 2, 1), ("app", 3, 1))
    cache = pool(64, 2, ops)
    assert cache.prefix_groups([0, 1, 2, 3]) == [([0, 1, 2, 3], 2)]
    assert cache.prefix_groups([1, 2, 3]) == [([0, 1, 2], 3)]
    assert cache.alloc.pages[1][3] != cache.alloc.pages[3][3]       # the copied partial page
    check(cache, [0, 1, 2, 3], [1, 1, 1, 1], 4, True, 64, [2])
    check(cache, [3, 1, 2], [1, 2, 1], 4, True, 64, [3])


@pytest.mark.parametrize("kps,ns", [(64, 16), (512, 2)])
def test_large_pages(kps, ns):
    """6: P = 256: several splits per page at kps 64; at kps 512 a group run crosses a page."""
    ops = (("app", 0, 1024), ("fork", 0, 1), ("fork", 0, 2), ("fork", 0, 3), ("app", 1, 1), ("app", 2, 300),
           ("app", 3, 7))
    check(pool(256, 2, ops, num_pages=12, mpp=6), [1, 2, 3], [1, 2, 1], 4, True, kps, [ns])


def test_smoothed_cache():
    """7: k_mean given: the forks carry the prompt's mean."""
    check(pool(64, 2, CHUNKS3, smooth=True), [1, 2, 3], [5, 1, 3], 4, True, 64, [3])


def test_scattered_pages():
    """8: a scattered free order: physical pages do not ascend."""
    cache = pool(64, 2, CHUNKS3, scattered=True)
    pages = cache.alloc.pages[1]
    assert any(b < a for a, b in zip(pages, pages[1:]))
    check(cache, [3, 1, 2], [3, 5, 1], 4, True, 64, [3])


def test_no_groups_is_the_plain_call():
    """9: unrelated sequences: share_prefix=True makes the plain call."""
    cache = pool(64, 2, (("app", 0, 100), ("app", 2, 200), ("app", 5, 64)))
    assert cache.prefix_groups([5, 0, 2]) == []
    check(cache, [5, 0, 2], [1, 3, 2], 4, True, 64, [])
    # forks, but no whole split inside the common pages
    check(pool(64, 2, FORKS3), [1, 2, 3], [1, 1, 1], 4, True, 256, [])


def test_window_raises():
    """10: share_prefix with a window is refused before any launch."""
    from quantizedattention_amd import _lib, ops
    from quantizedattention_amd.kv_cache_mxfp4 import attention_mxfp4_varlen_paged
    cache = pool(64, 2, FORKS3)
    q = torch.zeros((3, 4, D), dtype=torch.float16, device="cuda")
    for fn in (attention_mxfp4_varlen_paged, ops.mxfp4_varlen_paged):
        with pytest.raises(_lib.QAttnError, match="share_prefix with a window"):
            fn(q, cache, [1, 2, 3], [1, 1, 1], causal=True, window=64, share_prefix=True)


def test_operator_path():
    """11: ops.mxfp4_varlen_paged(share_prefix=True) equals the function."""
    from quantizedattention_amd import ops
    cache = pool(64, 2, CHUNKS3)
    for causal in (True, False):
        q, O, lse = check(cache, [1, 2, 3], [5, 1, 3], 4, causal, 64, [3])
        junk = [torch.full((n, D), float("nan"), device="cuda") for n in (72, 72, 36, 36)]   # freed below
        del junk
        PO, Plse = ops.mxfp4_varlen_paged(q, cache, [1, 2, 3], [5, 1, 3], causal=causal, keys_per_split=64,
                                          share_prefix=True)
        assert torch.equal(PO, O) and torch.equal(Plse, lse)
    # without groups the operator makes the plain call too
    q = torch.randn((2, 4, D), generator=torch.Generator().manual_seed(3)).half().cuda()
    lone = pool(64, 2, (("app", 0, 100), ("app", 2, 200), ("app", 5, 64)))
    a = ops.mxfp4_varlen_paged(q, lone, [0, 5], [1, 1], keys_per_split=64, share_prefix=True)
    b = ops.mxfp4_varlen_paged(q, lone, [0, 5], [1, 1], keys_per_split=64)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_default_keys_per_split():
    """12: keys_per_split=None: the shared call equals the plain call at the kps the shared plan chose."""
    from quantizedattention_amd.kv_cache_mxfp4 import attention_mxfp4_varlen_paged
    ops = (("app", 0, 1536), ("fork", 0, 1), ("fork", 0, 2), ("app", 1, 1), ("app", 2, 40))
    cache = pool(256, 2, ops, num_pages=12, mpp=7)
    ids, q_lens = [2, 1], [2, 1]
    plan = plan_of(cache, ids, q_lens, 4, True, None)
    kps = plan[0]
    assert plan[4] and kps <= 1536
    q = torch.randn((3, 4, D), generator=torch.Generator().manual_seed(43)).half().cuda()
    O, lse = attention_mxfp4_varlen_paged(q, cache, ids, q_lens, causal=True, keys_per_split=kps)
    with poisoned_empty():
        SO, Slse = attention_mxfp4_varlen_paged(q, cache, ids, q_lens, causal=True, share_prefix=True)
    assert torch.equal(SO, O) and torch.equal(Slse, lse)
