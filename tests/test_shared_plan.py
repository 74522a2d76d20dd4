"""The host side of shared-prefix attention: PageAllocator.prefix_groups and kv_cache_mxfp4.plan_varlen_shared.
Pure Python, no device.

prefix_groups is held on allocators driven by ``share``, ``reserve`` and ``drop``.  The plan is interpreted
in Python on seeded random pools and calls (240 cases: group sizes 2..40, q_lens 1..9, P in {64, 256}, kps
in {64, 128, 256, None}, causal and not): every (sequence, virtual row, split < ns_j) is produced by
exactly one work record (a record stands for every key/value head), group records touch only tiles inside
the common pages and, causal, below every member's first diagonal, and ``seq_rec`` / ``part_rows`` are
plan_varlen's at the same kps.
"""
import random
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "quantizedattention_amd" / "libqattn.so"
needs_lib = pytest.mark.skipif(not LIB.exists(), reason="libqattn.so not built (run __graft_entry__.build())")


def _alloc(num_pages=64, P=64, max_seqs=8, mpp=8, **kw):
    from quantizedattention_amd.kv_cache_mxfp4 import PageAllocator
    return PageAllocator(num_pages, P, max_seqs, mpp, **kw)


def _fork(alloc, lengths, src, dst):
    """PagedKVFP4.fork on the host mirrors alone: the full pages shared, a partial last page fresh."""
    L, P = lengths[src], alloc.page_tokens
    alloc.share(src, dst, L // P, 1 if L % P else 0)
    lengths[dst] = L


# ------------------------------------------------------------------------------ prefix_groups
def test_groups_of_forks():
    a, lengths = _alloc(), [0] * 8
    a.reserve([(0, 192)])
    lengths[0] = 192
    _fork(a, lengths, 0, 1)
    _fork(a, lengths, 0, 2)
    assert a.prefix_groups([0, 1, 2]) == [([0, 1, 2], 3)]
    # members are indices into seq_ids, ascending, whatever the order of the slots
    assert a.prefix_groups([2, 5, 0]) == [([0, 2], 3)]
    # unlisted slots are ignored; one listed member is no group
    assert a.prefix_groups([1, 4]) == [] and a.prefix_groups([1]) == []
    # the members grow on their own: the common pages stay
    a.reserve([(1, 193), (2, 400)])
    assert a.prefix_groups([0, 1, 2]) == [([0, 1, 2], 3)]


def test_fork_of_a_fork_takes_the_minimum():
    a, lengths = _alloc(), [0] * 8
    a.reserve([(0, 128)])
    lengths[0] = 128
    _fork(a, lengths, 0, 1)
    a.reserve([(1, 192)])          # sequence 1 fills a third page of its own
    lengths[1] = 192
    _fork(a, lengths, 1, 2)        # shares three pages with 1, two of them with 0
    a.reserve([(0, 192)])          # a third page of sequence 0, not the one 1 and 2 hold
    assert a.prefix_groups([0, 1, 2]) == [([0, 1, 2], 2)]
    assert a.prefix_groups([1, 2]) == [([0, 1], 3)]
    # one level of sharing: the sub-group {1, 2} gets only the group's two pages when 0 is listed


def test_a_partial_last_page_is_not_shared():
    a, lengths = _alloc(), [0] * 8
    a.reserve([(0, 100)])
    lengths[0] = 100
    _fork(a, lengths, 0, 1)        # page 0 shared, the partial page 1 copied into a fresh page
    assert a.pages[0][0] == a.pages[1][0] and a.pages[0][1] != a.pages[1][1]
    assert a.prefix_groups([0, 1]) == [([0, 1], 1)]
    b, lengths = _alloc(), [0] * 8
    b.reserve([(0, 40)])
    lengths[0] = 40
    _fork(b, lengths, 0, 1)        # nothing but a partial page: no common page, no group
    assert b.prefix_groups([0, 1]) == []


def test_a_trimmed_member_is_excluded():
    a, lengths = _alloc(), [0] * 8
    a.reserve([(0, 256)])
    lengths[0] = 256
    for dst in (1, 2):
        _fork(a, lengths, 0, dst)
    a.drop(1, 1, 3)
    assert a.prefix_groups([0, 1, 2]) == [([0, 2], 4)]
    a.drop(2, 2, 3)
    assert a.prefix_groups([0, 1, 2]) == []
    a.release(1)                   # empty again: no holes, no pages, still never grouped
    assert a.prefix_groups([0, 1, 2]) == []


def test_two_independent_groups():
    a, lengths = _alloc(max_seqs=8), [0] * 8
    a.reserve([(0, 128), (3, 320), (6, 64)])
    lengths[0], lengths[3], lengths[6] = 128, 320, 64
    _fork(a, lengths, 0, 1)
    _fork(a, lengths, 3, 4)
    _fork(a, lengths, 3, 5)
    assert a.prefix_groups([5, 1, 6, 0, 3, 4]) == [([0, 4, 5], 5), ([1, 3], 2)]
    from quantizedattention_amd import _lib
    with pytest.raises(_lib.QAttnError, match="no sequence"):
        a.prefix_groups([0, 8])


def test_cache_prefix_groups_is_the_allocators():
    from quantizedattention_amd.kv_cache_mxfp4 import PagedKVFP4
    a, lengths = _alloc(), [0] * 8
    a.reserve([(2, 64)])
    lengths[2] = 64
    _fork(a, lengths, 2, 7)
    cache = PagedKVFP4(None, None, None, None, None, None, None, a)
    assert cache.prefix_groups([7, 2]) == [([0, 1], 1)]


# ------------------------------------------------------------------------------ the plan, interpreted
def _ceil64(n):
    return -(-n // 64) * 64


def _random_call(rng, P):
    """A pool of prompts, forks and loners -> (allocator, lengths, seq_ids, q_lens)."""
    max_seqs, mpp = 64, 12
    a = _alloc(num_pages=1024, P=P, max_seqs=max_seqs, mpp=mpp)
    lengths, free = [0] * max_seqs, list(range(max_seqs))
    rng.shuffle(free)
    listed = []
    for _ in range(rng.randint(1, 2)):                      # groups of 2..40 forks of one prompt
        size = min(rng.randint(2, 40), len(free) - 4)
        if size < 2:
            break
        src = free.pop()
        L0 = rng.choice((P, 2 * P, 3 * P, rng.randint(1, 4 * P), 3 * P + 1, 192))
        a.reserve([(src, L0)])
        lengths[src] = L0
        group = [src]
        for _ in range(size - 1):
            dst = free.pop()
            _fork(a, lengths, rng.choice(group) if rng.random() < 0.2 else src, dst)
            group.append(dst)
        for b in group:                                      # own tokens, the prompt's slot too
            lengths[b] += rng.choice((0, 1, 1, 5, 70, rng.randint(0, 3 * P)))
            a.reserve([(b, lengths[b])])
        listed += group if rng.random() < 0.8 else group[1:]
    for _ in range(rng.randint(0, 4)):                      # unrelated sequences
        b = free.pop()
        lengths[b] = rng.randint(1, 6 * P)
        a.reserve([(b, lengths[b])])
        listed.append(b)
    rng.shuffle(listed)
    return a, lengths, listed, [rng.randint(1, 9) for _ in listed]


def _interpret(a, lengths, ids, q_lens, Hq, Hkv, kps_in, causal):
    from quantizedattention_amd.kv_cache_mxfp4 import plan_varlen, plan_varlen_shared
    P, G = a.page_tokens, Hq // Hkv
    if causal:   # a listed sequence holds at least its own queries
        q_lens = [min(n, lengths[b]) for n, b in zip(q_lens, ids)]
    groups = a.prefix_groups(ids)
    kps, seq_rec, work, part_rows, grp_rec, members = plan_varlen_shared(
        lengths, ids, q_lens, Hq, Hkv, groups, kps_in, causal, page_tokens=P)
    assert kps >= 64 and kps % 64 == 0
    if kps_in is not None:
        assert kps == min(kps_in, _ceil64(max(lengths[b] for b in ids)))
    plain = plan_varlen(lengths, ids, q_lens, Hq, Hkv, kps, causal)
    assert (plain[0], plain[1], plain[3]) == (kps, seq_rec, part_rows)
    # the tables against the groups they came from
    common = {tuple(m): c for m, c in groups}
    vis = [lengths[b] - n + 1 if causal else lengths[b] for b, n in zip(ids, q_lens)]
    seen, shared_of = set(), {}
    for first, count, ns_g, R in grp_rec:
        mem = members[first:first + count]
        js = [j for j, _ in mem]
        shared_of.update((j, ns_g) for j in js)
        assert tuple(js) in common and count >= 2 and not seen & set(js)
        seen |= set(js)
        assert ns_g == min(common[tuple(js)] * P, min(vis[j] for j in js)) // kps and ns_g >= 1
        rows = 0
        for j, start in mem:
            assert start == rows
            rows += G * q_lens[j]
        assert R == rows
        # what a group workgroup touches: tiles inside the common pages, every key visible to every row
        assert ns_g * kps <= common[tuple(js)] * P
        assert all(ns_g * kps <= vis[j] for j in js)
        pages = -(-ns_g * kps // P)
        assert all(a.pages[ids[j]][:pages] == a.pages[ids[js[0]]][:pages] for j in js)
    for m, c in groups:   # a group that is not in the tables had nothing to share
        if not set(m) & seen:
            assert min(c * P, min(vis[j] for j in m)) < kps
    # coverage: every (sequence, virtual row, split) exactly once; a record stands for every kv head
    got = {}
    tiles = []
    for w in work:
        assert len(w) == 4 and w[3] in (0, 1)
        if w[3] == 0:
            j, rb, s = w[:3]
            rows = range(rb * 128, min(rb * 128 + 128, G * q_lens[j]))
            assert len(rows) and s >= shared_of.get(j, 0)   # the shared splits are the group's alone
            cells = [(j, r, s) for r in rows]
            tiles.append(min(-(-lengths[ids[j]] // 64), (s + 1) * (kps // 64)) - s * (kps // 64))
        else:
            first, count, ns_g, R = grp_rec[w[0]]
            rb, s = w[1:3]
            assert s < ns_g and rb * 128 < R
            cells = []
            for r in range(rb * 128, min(rb * 128 + 128, R)):
                j, start = [x for x in members[first:first + count] if x[1] <= r][-1]
                assert r - start < G * q_lens[j]
                cells.append((j, r - start, s))
            tiles.append(kps // 64)
        for c in cells:
            got[c] = got.get(c, 0) + 1
    want = {(j, r, s) for j, rec in enumerate(seq_rec) for r in range(G * q_lens[j]) for s in range(rec[3])}
    assert set(got) == want and set(got.values()) == {1}
    assert all(t >= 1 for t in tiles) and tiles == sorted(tiles, reverse=True)
    return kps, grp_rec


def _cases():
    rng = random.Random(11)
    for i in range(240):
        P = (64, 256)[i % 2]
        yield (i, P, (64, 128, 256, None)[(i // 2) % 4], bool((i // 8) % 2), rng.getrandbits(32))


@needs_lib
def test_plan_covers_every_row_and_split_once():
    grouped = defaulted = 0
    for i, P, kps_in, causal, seed in _cases():
        rng = random.Random(seed)
        a, lengths, ids, q_lens = _random_call(rng, P)
        Hkv = rng.choice((1, 2))
        kps, grp_rec = _interpret(a, lengths, ids, q_lens, Hkv * rng.choice((1, 2, 4)), Hkv, kps_in, causal)
        grouped += bool(grp_rec)
        defaulted += kps_in is None and bool(grp_rec)
    assert grouped >= 120 and defaulted >= 20   # the cases do exercise the group path


def test_rounding_keeps_the_cut_split_per_sequence():
    """192 common keys at kps 128: one shared split; [128, 256) stays with every sequence."""
    from quantizedattention_amd.kv_cache_mxfp4 import plan_varlen_shared
    a, lengths = _alloc(), [0] * 8
    a.reserve([(0, 192)])
    lengths[0] = 192
    _fork(a, lengths, 0, 1)
    _fork(a, lengths, 0, 2)
    for b, n in ((0, 1), (1, 70), (2, 1)):
        lengths[b] += n
        a.reserve([(b, lengths[b])])
    ids, q_lens = [0, 1, 2], [1, 1, 1]
    kps, seq_rec, work, part_rows, grp_rec, members = plan_varlen_shared(
        lengths, ids, q_lens, 4, 2, a.prefix_groups(ids), 128, True, page_tokens=64)
    assert grp_rec == [[0, 3, 1, 6]] and members == [[0, 0], [1, 2], [2, 4]]
    assert [w for w in work if w[3] == 1] == [[0, 0, 0, 1]]
    assert sorted(w[:3] for w in work if w[3] == 0) == [[0, 0, 1], [1, 0, 1], [1, 0, 2], [2, 0, 1]]
    # kps 64: all three common pages are shared; kps 256: nothing is, and the tables are empty
    assert plan_varlen_shared(lengths, ids, q_lens, 4, 2, a.prefix_groups(ids), 64, True,
                              page_tokens=64)[4] == [[0, 3, 3, 6]]
    assert plan_varlen_shared(lengths, ids, q_lens, 4, 2, a.prefix_groups(ids), 256, True,
                              page_tokens=64)[4:] == ([], [])
    # causal with a chunk: 70 queries after 262 keys see only 193 of them all; 5 queries cut a 64-key split
    assert plan_varlen_shared(lengths, ids, [1, 70, 1], 4, 2, a.prefix_groups(ids), 64, True,
                              page_tokens=64)[4] == [[0, 3, 3, 144]]
    lengths[1] = 195
    assert plan_varlen_shared(lengths, ids, [1, 5, 1], 4, 2, a.prefix_groups(ids), 64, True,
                              page_tokens=64)[4] == [[0, 3, 2, 14]]
    assert plan_varlen_shared(lengths, ids, [1, 5, 1], 4, 2, a.prefix_groups(ids), 64, False,
                              page_tokens=64)[4] == [[0, 3, 3, 14]]


@needs_lib
def test_default_kps_lets_every_group_share():
    from quantizedattention_amd import _lib
    from quantizedattention_amd.kv_cache_mxfp4 import plan_varlen_shared
    lib = _lib.load()
    # 64 forks of a 32768-key prompt with 256 own keys each, 32 / 8 heads, P = 256: two group row blocks
    lengths = [33024] * 64
    groups = [(list(range(64)), 128)]
    kps, _, work, _, grp_rec, _ = plan_varlen_shared(lengths, range(64), [1] * 64, 32, 8, groups, None, True,
                                                     page_tokens=256)
    assert kps == lib.qattn_split_keys(8 * 2, 1, 33024, 64) and kps <= 32768
    assert grp_rec == [[0, 64, 32768 // kps, 256]]
    # a group that can share 192 keys lowers a larger rule to 192; one that can share none is left out
    lengths = [8192 + 192, 8192 + 192, 5000, 40, 40]
    groups = [([0, 1], 3), ([3, 4], 1)]
    kps, _, _, _, grp_rec, members = plan_varlen_shared(lengths, range(5), [1] * 5, 4, 2, groups, None,
                                                        page_tokens=64)
    assert lib.qattn_split_keys(2 * 4, 1, 8384, 64) > 192 and kps == 192
    assert grp_rec == [[0, 2, 1, 4]] and members == [[0, 0], [1, 2]]


def test_errors():
    from quantizedattention_amd import _lib
    from quantizedattention_amd.kv_cache_mxfp4 import plan_varlen_shared
    lengths = [200, 200, 200, 0, 64]
    ok = [([0, 1], 2)]
    plan = lambda ids, q, Hq, Hkv, groups, kps=64, causal=False, P=64: plan_varlen_shared(  # noqa: E731
        lengths, ids, q, Hq, Hkv, groups, kps, causal, page_tokens=P)
    plan([0, 1, 2], [1, 1, 1], 4, 2, ok)
    bad = [
        # plan_varlen's own
        (([3, 1], [1, 1], 4, 2, ok), "at least one cached token"),
        (([0, 1], [201, 1], 4, 2, ok, 64, True), "causal"),
        (([0, 0], [1, 1], 4, 2, ok), "distinct"),
        (([0, 5], [1, 1], 4, 2, ok), "distinct"),
        (([], [], 4, 2, []), "nseq >= 1"),
        (([0, 1], [1], 4, 2, ok), "nseq >= 1"),
        (([0, 1], [1, 0], 4, 2, ok), ">= 1"),
        (([0, 1], [1, 1], 3, 2, ok), "heads"),
        (([0, 1], [1, 1], 4, 2, ok, 96), "keys_per_split"),
        (([0, 1], [1, 1], 4, 2, ok, 0), "keys_per_split"),
        # the groups
        (([0, 1, 2], [1, 1, 1], 4, 2, [([0, 3], 2)]), "ascending indices"),
        (([0, 1, 2], [1, 1, 1], 4, 2, [([-1, 1], 2)]), "ascending indices"),
        (([0, 1, 2], [1, 1, 1], 4, 2, [([1, 0], 2)]), "ascending indices"),
        (([0, 1, 2], [1, 1, 1], 4, 2, [([1, 1], 2)]), "ascending indices"),
        (([0, 1, 2], [1, 1, 1], 4, 2, [([0, 1], 2), ([1, 2], 1)]), "two prefix groups"),
        (([0, 1, 2], [1, 1, 1], 4, 2, [([0], 2)]), "at least two members"),
        (([0, 1, 2], [1, 1, 1], 4, 2, [([0, 1], 0)]), "at least two members"),
        (([0, 1], [1, 1], 4, 2, ok, 64, False, 96), "page_tokens"),
    ]
    for args, match in bad:
        with pytest.raises(_lib.QAttnError, match=match):
            plan(*args)
    with pytest.raises(_lib.QAttnError, match="2\\^31"):
        plan_varlen_shared([1 << 25, 1 << 25], [0, 1], [1 << 13, 1], 1, 1, [([0, 1], 1)], 64, page_tokens=64)


def test_share_prefix_with_a_window_raises_before_any_tensor(monkeypatch):
    import torch

    from quantizedattention_amd import _lib
    from quantizedattention_amd.kv_cache_mxfp4 import PagedKVFP4, attention_mxfp4_varlen_paged
    z = lambda *s, dt=torch.uint8: torch.zeros(s, dtype=dt)  # noqa: E731
    a = _alloc(4, 64, 4, 2)
    cache = PagedKVFP4(z(4, 2, 64, 64), z(4, 2, 64, 4), z(4, 2, 1, 128, 32), z(4, 2, 1, 128, 2),
                       z(4, 2, 64, 128, dt=torch.float16), z(4, dt=torch.int32), z(4, 2, dt=torch.int32), a)
    a.reserve([(0, 64)])
    cache.lengths[0] = 64
    _fork(a, cache.lengths, 0, 2)
    q = z(2, 4, 128, dt=torch.float16)

    def trap(*args, **kw):
        raise AssertionError("a tensor was made before the error was raised")
    monkeypatch.setattr(torch, "tensor", trap)
    monkeypatch.setattr(torch, "empty", trap)
    with pytest.raises(_lib.QAttnError, match="share_prefix with a window"):
        attention_mxfp4_varlen_paged(q, cache, [0, 2], [1, 1], causal=True, window=16, share_prefix=True)
    # without the window the shared plan is made and the call stops at the device check; without groups too
    with pytest.raises(_lib.QAttnError, match="no CPU fallback"):
        attention_mxfp4_varlen_paged(q, cache, [0, 2], [1, 1], causal=True, keys_per_split=64, share_prefix=True)
    with pytest.raises(_lib.QAttnError, match="no CPU fallback"):
        attention_mxfp4_varlen_paged(q[:1], cache, [0], [1], keys_per_split=64, share_prefix=True)
