"""The host side of the device-planned decode step (kv_cache_mxfp4.DecodeStep): plan_decode_step, the pure-
Python statement of the tables qattn_mxfp4_decode_step_plan writes, against plan_varlen; the bound
decode_step_splits; the padding records; and what DecodeStep.prepare refuses.  No device, no kernel.
"""
import pytest
import torch

from quantizedattention_amd import _lib
from quantizedattention_amd.kv_cache_mxfp4 import (DecodeStep, PageAllocator, PagedKVFP4, decode_step_splits,
                                                   plan_decode_step, plan_varlen)

KPS = (64, 128, 256)
WINDOWS = (None, (70, 3), (64, 0), (1, 130))
HKV, G = 2, 2


def _win(w):
    return {} if w is None else {"window": w[0], "sinks": w[1]}


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("kps", KPS)
def test_plan_is_plan_varlens_at_one_query(kps, window):
    """ns, wt0, nst of every L in [0, 400] equal plan_varlen's for one sequence of L + 1 keys and one query;
    the host call clamps kps to the sequence's longest run, which moves no split boundary."""
    splits = decode_step_splits(401, kps, **_win(window))
    for L in range(401):
        tab, tiles, pos, rec, work = plan_decode_step([L], [0], kps, splits, HKV, G, **_win(window))
        hk, hrec, hwork, rows = plan_varlen([L + 1], [0], [1], HKV * G, HKV, kps, causal=True, **_win(window))
        assert rec == [[0, 0, 1, hrec[0][3], 0, hrec[0][5], hrec[0][6], 0]], (L, rec, hrec)
        assert hk <= kps and rows == hrec[0][3] * HKV * G and len(hwork) == hrec[0][3]
        if hk < kps:   # clamped: one run shorter than kps, so one split (two with a sink run) either way
            assert hrec[0][3] == 1 + (hrec[0][6] > 0)
        assert tab == [[0, 1, 0, 0]] and tiles == [[0, L // 64]] and pos == [L]
        order = list(range(splits))
        if window is not None and window[1] and splits > 1:   # the sink run, the short one, last
            order = order[1:] + [0]
        assert work == [[0, 0, s, 0] for s in order]


@pytest.mark.parametrize("window", WINDOWS + ((4096, 4),))
@pytest.mark.parametrize("kps", KPS + (1024,))
def test_splits_bound_every_length_and_are_reached(kps, window):
    for max_keys in (1, 63, 64, 65, 200, 401, 1000, 6000):
        splits = decode_step_splits(max_keys, kps, **_win(window))
        # (128 splits: above 6000 / 64, so no count is held to the grid's)
        ns = [plan_decode_step([L], [0], kps, 128, 1, 1, **_win(window))[3][0][3] for L in range(max_keys)]
        assert max(ns) == splits < 128, (max_keys, kps, window)
    if window is not None:   # no growth with max_keys: at most 1 + the splits of the W-key run, which reaches
        W = window[0]        # into a partial tile at either end (W + 127 keys of tiles at the most)
        assert decode_step_splits(1 << 25, kps, *window) == decode_step_splits(W + 64 * 8, kps, *window)
        assert decode_step_splits(1 << 25, kps, *window) <= 1 + -(-(W + 128) // kps)
    else:
        assert decode_step_splits(32768, kps) == 32768 // kps
    for bad in ((0, 64), (10, 96), (10, 0)):
        with pytest.raises(_lib.QAttnError, match="keys_per_split"):
            decode_step_splits(*bad)
    with pytest.raises(_lib.QAttnError, match="sinks"):
        decode_step_splits(100, 64, None, 3)


def test_padding_entries():
    """Slots outside [0, max_seqs) and lengths outside [0, capacity) give the padding records; the listed
    entries beside them keep their rows of the partials."""
    lengths = [130, 0, 63, 256]
    slots = [2, -1, 4, 0, -7, 3, 1]
    tab, tiles, pos, rec, work = plan_decode_step(lengths, slots, 64, 5, HKV, G, capacity=256)
    base = [i * 5 * HKV * G for i in range(len(slots))]
    for i in (1, 2, 4, 5):   # -1, max_seqs, -7, and slot 3 at the capacity
        assert tab[i] == [-1, 0, i, 0] and tiles[i] == [-1, 0] and pos[i] == 0
        assert rec[i] == [-1, i, 1, 0, base[i], 0, 0, 0]
    assert tab[0] == [2, 1, 0, 0] and tiles[0] == [0, 0] and pos[0] == 63 and rec[0] == [2, 0, 1, 1, 0, 0, 0, 0]
    assert tab[3] == [0, 1, 3, 0] and tiles[3] == [3, 2] and pos[3] == 130
    assert rec[3] == [0, 3, 1, 3, base[3], 0, 0, 0]
    assert tab[6] == [1, 1, 6, 0] and tiles[6] == [6, 0] and pos[6] == 0 and rec[6][3] == 1   # an empty slot appends
    assert sorted(map(tuple, work)) == [(i, 0, s, 0) for i in range(7) for s in range(5)]
    assert plan_decode_step(lengths, [3], 64, 5, HKV, G)[3][0][3] == 5   # no capacity given: 257 keys, 5 splits
    assert plan_decode_step(lengths, [3], 64, 3, HKV, G)[3][0][3] == 3   # ns is held to the grid's splits


def _host_step(N, max_keys, window=None, sinks=0, kps=64):
    """A DecodeStep without its device tensors (its constructor takes a GPU): what prepare uses."""
    step = DecodeStep.__new__(DecodeStep)
    step.N, step.max_keys, step.q_heads, step.kv_heads, step.kps = N, max_keys, HKV * G, HKV, kps
    step.window, step.sinks, step.splits = window, sinks, decode_step_splits(max_keys, kps, window, sinks)
    step.slots, step.listed = torch.full((N,), -1, dtype=torch.int32), []
    return step


def _host_pool(pages=12, mpp=8):
    z = lambda *s, dt=torch.uint8: torch.zeros(s, dtype=dt)  # noqa: E731
    alloc = PageAllocator(pages, 64, 4, mpp)
    cache = PagedKVFP4(z(pages, HKV, 64, 64), z(pages, HKV, 64, 4), z(pages, HKV, 1, 128, 32),
                       z(pages, HKV, 1, 128, 2), z(4, HKV, 64, 128, dt=torch.float16), z(4, dt=torch.int32),
                       z(4, mpp, dt=torch.int32), alloc)
    return cache, alloc


def _host_state(cache):
    a = cache.alloc
    return (list(cache.lengths), list(a._free), [list(p) for p in a.pages], list(a.refcount),
            cache.block_table.clone())


def _same(a, b):
    return a[:4] == b[:4] and torch.equal(a[4], b[4])


def test_prepare_refuses_with_the_pool_unchanged():
    cache, alloc = _host_pool()
    alloc.reserve([(0, 10), (2, 500), (3, 64)])
    cache.lengths = [10, 0, 500, 64]
    step = _host_step(3, 500)
    before = _host_state(cache)
    for ids, match in [([0, 0], "distinct"), ([0, 4], "distinct"), ([-1], "distinct"), ([0, 1, 2, 3], "at most 3"),
                       ([0, 1], "at least one cached token"), ([2, 0], "would pass 500 keys")]:
        with pytest.raises(_lib.QAttnError, match=match):
            step.prepare(cache, ids)
        assert _same(before, _host_state(cache)) and step.listed == [] and step.slots.tolist() == [-1] * 3, ids
    # the pool's own capacity (8 pages of 64) under a step that would allow more
    cache.lengths[2] = 512
    alloc.reserve([(2, 512)])
    before = _host_state(cache)
    with pytest.raises(_lib.QAttnError, match="would pass 512 keys"):
        _host_step(3, 4096).prepare(cache, [2])
    assert _same(before, _host_state(cache))
    # out of pages: all or nothing, the lengths included (slot 3 needs a page and none is free)
    alloc.reserve([(1, 64)])
    assert alloc.free_pages == 1
    cache.lengths[1] = 64
    before = _host_state(cache)
    with pytest.raises(_lib.QAttnError, match="out of pages"):
        _host_step(3, 4096).prepare(cache, [0, 1, 3])
    assert _same(before, _host_state(cache))
    # a trimmed page the step's window would read; the window it was trimmed for passes
    cache.lengths[2] = 500
    assert cache.trim([2], 130, 4) == 4
    before = _host_state(cache)
    for kw in ({}, {"window": 200, "sinks": 4}, {"window": 130, "sinks": 70}):
        with pytest.raises(_lib.QAttnError, match="trimmed"):
            _host_step(3, 4096, **kw).prepare(cache, [2, 0])
        assert _same(before, _host_state(cache)), kw
    with pytest.raises(_lib.QAttnError, match="PagedKVFP4"):
        step.prepare(object(), [0])


def test_prepare_reserves_uploads_and_bumps(monkeypatch):
    """What prepare does when it accepts: the page of position L, the table, slots padded with -1, lengths + 1;
    and it neither plans nor lists tiles on the host."""
    from quantizedattention_amd import kv_cache_mxfp4 as K
    cache, alloc = _host_pool()
    alloc.reserve([(0, 10), (2, 500), (3, 64)])
    cache.lengths = [10, 0, 500, 64]
    cache.block_table.copy_(torch.tensor(alloc.table, dtype=torch.int32))
    cache.trim([2], 130, 4)

    def trap(*a, **k):
        raise AssertionError("prepare planned on the host")
    monkeypatch.setattr(K, "plan_varlen", trap)
    monkeypatch.setattr(K, "plan_decode_step", trap)
    step = _host_step(3, 4096, window=130, sinks=4)
    free = alloc.free_pages
    assert step.prepare(cache, [3, 2]) is step
    assert cache.lengths == [10, 0, 501, 65] and step.listed == [3, 2] and step.slots.tolist() == [3, 2, -1]
    assert alloc.free_pages == free - 1 and len(alloc.pages[3]) == 2        # 64 -> 65 opens a page at P = 64
    assert cache.block_table.tolist()[3][:2] == alloc.pages[3]
    table = cache.block_table.clone()
    step.prepare(cache, torch.tensor([0]))
    assert cache.lengths == [11, 0, 501, 65] and step.slots.tolist() == [0, -1, -1]
    assert torch.equal(table, cache.block_table) and alloc.free_pages == free - 1


def test_exports_and_fake_kernels():
    from quantizedattention_amd import kv_cache_mxfp4 as K, ops
    assert {"DecodeStep", "decode_step_splits", "plan_decode_step"} <= set(K.__all__)
    assert {"mxfp4_decode_step_plan", "mxfp4_decode_step"} <= set(ops.__all__)
    assert {"qattn_mxfp4_decode_step_plan", "qattn_mxfp4_attn_fwd_decode_step",
            "qattn_mxfp4_decode_step_combine"} <= set(_lib.SIGNATURES)
    with pytest.raises(_lib.QAttnError, match="no CPU fallback"):
        DecodeStep(4, 512, 4, 2, "cpu")
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        i32 = lambda *s: torch.empty(s, dtype=torch.int32, device="cuda")  # noqa: E731
        u8 = lambda *s: torch.empty(s, dtype=torch.uint8, device="cuda")  # noqa: E731
        tab, tiles, pos, rec = torch.ops.qattn.mxfp4_decode_step_plan(i32(6), i32(6), 320, 2, 2, 64, 5, 0, 0)
        assert (tab.shape, tiles.shape, pos.shape, rec.shape) == ((6, 4), (6, 2), (6,), (6, 8))
        assert rec.dtype == torch.int32 and rec.device.type == "cuda"
        q = torch.empty((6, 4, 128), dtype=torch.float16, device="cuda")
        O, lse = torch.ops.qattn.mxfp4_decode_step(q, u8(8, 2, 64, 64), u8(8, 2, 64, 4), u8(8, 2, 1, 128, 32),
                                                   u8(8, 2, 1, 128, 2), i32(6), i32(6, 5), rec, i32(30, 4), 5, 64,
                                                   0, 0)
        assert O.shape == (6, 4, 128) and O.dtype == torch.float16 and lse.shape == (6, 4)
        assert lse.dtype == torch.float32
