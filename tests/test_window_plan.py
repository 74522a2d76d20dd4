"""The host plan of the windowed packed step, kv_cache_mxfp4.plan_varlen(window=, sinks=): pure Python.

On the batches of tests/test_varlen_plan.py (hand-written and seeded random) under several (window,
sinks): every (row block, split < ns_j) is listed once, the partial rows are dense, ns_j and the tiles of
every split are those of the tile-range rule (the sink split, then the window splits from wt0),
``window=None`` returns today's tuple, a 4096-key window at 32768 cached keys runs 1 + 65 tiles and not
512, and every contract error raises before a tensor is made.
"""
import pytest

from test_varlen_plan import BATCHES, needs_lib

WINDOWS = [(1, 0), (1, 4), (64, 0), (100, 4), (100, 70), (37, 64), (4096, 4), (1 << 40, 0), (300, 129)]


def _ranges(L, n, W, S, kps):
    """The rule of the tile range, restated: [(first tile, last tile)] per split and (wt0', nst')."""
    nt, T = -(-L // 64), kps // 64
    wt0, nst = max(0, L - n - W + 1) // 64, -(-min(S, L) // 64)
    if wt0 <= nst:
        return [(t, min(nt, t + T)) for t in range(0, nt, T)], (0, 0)
    return [(0, nst)] * (nst > 0) + [(t, min(nt, t + T)) for t in range(wt0, nt, T)], (wt0, nst)


def _check(batch, kps_in, W, S):
    from quantizedattention_amd.kv_cache_mxfp4 import plan_varlen
    lengths, ids, q_lens, Hq, Hkv = batch
    q_lens = [min(n, lengths[b]) for b, n in zip(ids, q_lens)]      # causal: n_j <= L_j
    kps, seq_rec, work, part_rows = plan_varlen(lengths, ids, q_lens, Hq, Hkv, kps_in, True, W, S)
    G = Hq // Hkv
    assert kps % 64 == 0 and kps >= 64
    first, blocks, expect, tiles_of = 0, [], set(), {}
    run = []
    for j, (rec, b, n) in enumerate(zip(seq_rec, ids, q_lens)):
        ranges, (wt0, nst) = _ranges(lengths[b], n, W, S, kps)
        run.append(sum(hi - lo for lo, hi in ranges))
        ns = len(ranges)
        assert len(rec) == 8 and rec[7] == 0
        assert rec[:4] == [b, first, n, ns] and rec[5:7] == [wt0, nst], (j, rec, ranges)
        blocks.append((rec[4], rec[4] + ns * Hkv * G * n))
        for s, (lo, hi) in enumerate(ranges):
            assert hi > lo
            for rb in range(-(-G * n // 128)):
                expect.add((j, rb, s))
                tiles_of[(j, rb, s)] = hi - lo
        first += n
    if kps_in is not None:
        assert kps == min(kps_in, 64 * max(run))
    blocks.sort()
    assert blocks[0][0] == 0 and blocks[-1][1] == part_rows
    assert all(a[1] == b[0] for a, b in zip(blocks, blocks[1:]))
    assert all(len(w) == 4 and w[3] == 0 for w in work)
    got = [tuple(w[:3]) for w in work]
    assert len(got) == len(set(got)) and set(got) == expect
    tiles = [tiles_of[g] for g in got]
    assert tiles == sorted(tiles, reverse=True)
    return kps, seq_rec, work, part_rows, run


@pytest.mark.parametrize("kps", [64, 1024])
def test_window_plan_given_split(kps):
    for batch in BATCHES[:120]:
        for W, S in WINDOWS:
            _check(batch, kps, W, S)


@needs_lib
def test_window_plan_none_is_the_library_rule_at_the_tiles_run():
    from quantizedattention_amd import _lib
    lib = _lib.load()
    for batch in BATCHES[:120]:
        lengths, ids, q_lens, Hq, Hkv = batch
        for W, S in ((100, 4), (4096, 4), (1 << 40, 0)):
            kps, _, _, _, run = _check(batch, None, W, S)
            nwg = Hkv * sum(-(-(Hq // Hkv) * min(n, lengths[b]) // 128) for b, n in zip(ids, q_lens))
            sk_max = 64 * max(run)
            assert kps == min(lib.qattn_split_keys(nwg, 1, sk_max, 64), sk_max)


def test_window_none_is_todays_plan():
    from quantizedattention_amd.kv_cache_mxfp4 import plan_varlen
    for lengths, ids, q_lens, Hq, Hkv in BATCHES[:60]:
        for causal in (False, True):
            n = [min(a, lengths[b]) for b, a in zip(ids, q_lens)]
            want = plan_varlen(lengths, ids, n, Hq, Hkv, 1024, causal)
            assert plan_varlen(lengths, ids, n, Hq, Hkv, 1024, causal, None, 0) == want
            assert plan_varlen(lengths, ids, n, Hq, Hkv, 1024, causal, window=None) == want
            assert all(r[5:] == [0, 0, 0] for r in want[1])
        # a window that covers everything plans the causal call's splits
        kps, rec, work, rows = plan_varlen(lengths, ids, n, Hq, Hkv, 1024, True, 1 << 30, 4)
        assert (kps, rec, work, rows) == plan_varlen(lengths, ids, n, Hq, Hkv, 1024, True)


def test_a_decode_window_runs_its_own_tiles():
    """W = 4096, S = 4, n = 1 at 32768 cached keys: one sink tile and the window's tiles, not 512.  The new
    token appended to 32768 cached keys sits at p = 32768 (L = 32769): its window [28673, 32768] starts
    inside tile 448 and ends in tile 512, 65 tiles.  At L = 32768 exactly (p = 32767) the window [28672,
    32767] is tile-aligned: 64 tiles."""
    for L, first, window_tiles in ((32769, 448, 65), (32768, 448, 64), (32767, 447, 65)):
        for kps_in in (64, 1024, 4096):
            kps, rec, work, rows, run = _check(([L] * 3, [0, 1, 2], [1, 1, 1], 32, 8), kps_in, 4096, 4)
            assert run == [1 + window_tiles] * 3 and rec[0][5:7] == [first, 1]
            assert rec[0][3] == 1 + -(-window_tiles * 64 // kps)
            per_seq = [sum(1 for w in work if w[0] == j) for j in range(3)]
            assert per_seq == [rec[0][3]] * 3
    ranges, _ = _ranges(32769, 1, 4096, 4, 1024)
    assert ranges[0] == (0, 1) and ranges[1][0] == 448 and sum(b - a for a, b in ranges) == 1 + 65


def test_window_errors():
    from quantizedattention_amd import _lib
    from quantizedattention_amd.kv_cache_mxfp4 import plan_varlen
    lengths = [10, 0, 200, 64]
    for kw, match in [({"window": 0}, "window"), ({"window": -3}, "window"), ({"window": 8, "sinks": -1}, "sinks"),
                      ({"sinks": 4}, "sinks without a window"), ({"window": 2.5}, "window"),
                      ({"window": 8, "causal": False}, "implies causal")]:
        with pytest.raises(_lib.QAttnError, match=match):
            plan_varlen(lengths, [0, 2], [1, 3], 4, 2, 64, **{"causal": True, **kw})
    with pytest.raises(_lib.QAttnError, match="causal"):       # 11 queries over 10 cached tokens
        plan_varlen(lengths, [0, 2], [11, 3], 4, 2, 64, True, 8, 0)
    plan_varlen(lengths, [0, 2], [1, 3], 4, 2, 64, True, 8, 0)


def test_entry_window_errors_raise_before_any_tensor(monkeypatch):
    """attention_mxfp4_varlen_paged(window=) on CPU tensors: every contract error, a trimmed page this call
    would read included, raises before a tensor is made or moved (torch.tensor / torch.empty are trapped),
    and changes nothing on the host."""
    import torch

    from quantizedattention_amd import _lib
    from quantizedattention_amd.kv_cache_mxfp4 import PageAllocator, PagedKVFP4, attention_mxfp4_varlen_paged
    z = lambda *s, dt=torch.uint8: torch.zeros(s, dtype=dt)  # noqa: E731
    alloc = PageAllocator(12, 64, 4, 8)
    cache = PagedKVFP4(z(12, 2, 64, 64), z(12, 2, 64, 4), z(12, 2, 1, 128, 32), z(12, 2, 1, 128, 2),
                       z(4, 2, 64, 128, dt=torch.float16), z(4, dt=torch.int32), z(4, 8, dt=torch.int32), alloc)
    alloc.reserve([(0, 10), (2, 500)])
    cache.lengths = [10, 0, 500, 0]
    assert cache.trim([0, 2], 130, 4) == 4 and alloc.pages[2][1:5] == [None] * 4      # 500 - 130 + 1 = 371
    host = (list(cache.lengths), list(alloc._free), [list(p) for p in alloc.pages], list(alloc.refcount))
    q = z(5, 4, 128, dt=torch.float16)

    def trap(*a, **k):
        raise AssertionError("a tensor was made before the error was raised")
    monkeypatch.setattr(torch, "tensor", trap)
    monkeypatch.setattr(torch, "empty", trap)
    for kw, match in [({"window": 0}, "window"), ({"window": 130, "sinks": -1}, "sinks"),
                      ({"sinks": 4}, "sinks without a window"), ({"window": 130, "causal": False}, "implies causal"),
                      ({}, "trimmed"),                                   # no window: every page
                      ({"window": 131, "sinks": 4}, "no CPU fallback"),  # the window only grows with L
                      ({"window": 200, "sinks": 4}, "trimmed"),          # a larger window
                      ({"window": 130, "sinks": 65}, "trimmed"),         # more sinks: page 1
                      ({"window": 130, "sinks": 64}, "no CPU fallback"),  # 64 sinks still lie in page 0
                      ({"window": 130, "sinks": 4}, "no CPU fallback")]:
        with pytest.raises(_lib.QAttnError, match=match):
            attention_mxfp4_varlen_paged(q, cache, [0, 2], [2, 3], **{"causal": True, "keys_per_split": 64, **kw})
    with pytest.raises(_lib.QAttnError, match="trimmed"):
        attention_mxfp4_varlen_paged(z(61, 4, 128, dt=torch.float16), cache, [0, 2], [1, 60], causal=True,
                                     window=130, sinks=4)                # 60 queries reach back 59 keys more
    for call in (lambda: cache.gather(2), lambda: cache.snapshot(2), lambda: cache.fork(2, 1)):
        with pytest.raises(_lib.QAttnError, match="trimmed"):
            call()
    assert host == (list(cache.lengths), list(alloc._free), [list(p) for p in alloc.pages], list(alloc.refcount))
