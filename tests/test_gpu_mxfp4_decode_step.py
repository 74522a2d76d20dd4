"""The device-planned decode step (kv_cache_mxfp4.DecodeStep) on the GPU.  One criterion throughout, torch.equal:
every listed entry gets, bit for bit, what the host-planned pair gives on a twin pool fed the same tokens --
``append_packed(k, v, ids, [1] * n)`` followed by ``attention_mxfp4_varlen_paged(q, twin, ids, [1] * n,
causal=True, keys_per_split=step.kps[, window, sinks][, rope])`` -- and the pool holds the twin's bytes.
Shapes are tests/mxfp4_varlen_helpers.py's: 6 slots, four of them in use, N = 6 entries, so at least two are
padding.
"""
import pytest
import torch

import mxfp4_varlen_helpers as H

pytestmark = pytest.mark.gpu

N = H.MAX_SEQS
HEADS = ((4, 2), (4, 4))
POOLS = ((64, 32), (256, 48))
LENGTHS = ((1, 63, 64, 200), (127, 130, 255, 70))


def _K():
    from quantizedattention_amd import kv_cache_mxfp4 as K
    return K


def _rows(Hq, Hkv, seed):
    """(k, v [N, Hkv, 128], q [N, Hq, 128]) of one step; the rows of padding entries hold values too."""
    g = torch.Generator().manual_seed(seed)
    r = lambda h: torch.randn((N, h, H.D), generator=g).half().cuda()  # noqa: E731
    return r(Hkv), r(Hkv), r(Hq)


def _twins(Hkv, lengths, P, pages):
    return H.fill_pool(Hkv, lengths, P, pages), H.fill_pool(Hkv, lengths, P, pages)


def _same_pool(cache, twin):
    """lens, and per slot the gathered rows and tiles and the live vtail rows."""
    assert cache.lengths == twin.lengths and cache.alloc.pages == twin.alloc.pages
    assert cache.lens.cpu().tolist() == cache.lengths and torch.equal(cache.lens, twin.lens)
    for b, L in enumerate(cache.lengths):
        if L == 0:
            continue
        for x, y in zip(H.gather(cache, b), H.gather(twin, b)):
            assert torch.equal(x, y), (b, L)
        assert torch.equal(cache.vtail[b, :, :L % 64], twin.vtail[b, :, :L % 64]), (b, L)


def _host_step(twin, ids, k, v, q, kps, window=None, sinks=0, rope=None):
    K = _K()
    n = len(ids)
    twin.append_packed(k[:n], v[:n], ids, [1] * n, rope=rope)
    return K.attention_mxfp4_varlen_paged(q[:n], twin, ids, [1] * n, causal=True, keys_per_split=kps,
                                          window=window, sinks=sinks, rope=rope)


def _check_step(O, lse, want, n):
    RO, Rl = want
    assert O.shape[0] == N and lse.dtype == torch.float32
    assert torch.equal(O[:n], RO) and torch.equal(lse[:n], Rl)
    assert not O[n:].any() and bool((lse[n:] == float("-inf")).all())


# ------------------------------------------------------------------------------ 1. the plan kernel
@pytest.mark.parametrize("window", (None, (70, 3)))
@pytest.mark.parametrize("kps", (64, 128))
@pytest.mark.parametrize("lengths", LENGTHS)
def test_plan_kernel_writes_the_host_statement(lengths, kps, window):
    from quantizedattention_amd import _lib
    K = _K()
    Hq, Hkv = HEADS[0]
    cache = H.pool(Hkv, lengths, 64, 32)   # shared: only its lens is read here
    W, S = window or (None, 0)
    step = K.DecodeStep(N, 320, Hq, Hkv, "cuda", keys_per_split=kps, window=W, sinks=S)
    assert step.splits == K.decode_step_splits(320, kps, W, S) and step.kps == kps
    slots = [4, 0, 5, 2, -1, H.MAX_SEQS]
    step.slots.copy_(torch.tensor(slots, dtype=torch.int32))
    a = cache.alloc
    cap = a.max_pages_per_seq * a.page_tokens
    _lib.call("qattn_mxfp4_decode_step_plan", _lib.ptr(step.slots), _lib.ptr(cache.lens), _lib.ptr(step.seq_tab),
              _lib.ptr(step.tiles), _lib.ptr(step.seq_rec), _lib.ptr(step.pos), N, a.max_seqs, cap, Hkv, Hq // Hkv,
              kps, step.splits, W or 0, S, _lib.stream_of(step.slots))
    tab, tiles, pos, rec, work = K.plan_decode_step(cache.lengths, slots, kps, step.splits, Hkv, Hq // Hkv, W, S,
                                                    capacity=cap)
    assert step.seq_tab.cpu().tolist() == tab and step.tiles.cpu().tolist() == tiles
    assert step.pos.cpu().tolist() == pos and step.seq_rec.cpu().tolist() == rec
    assert step.work.cpu().tolist() == work
    assert [r[3] for r in rec[4:]] == [0, 0] and max(r[3] for r in rec) >= 1


# ------------------------------------------------------------------------------ 2. three steps against a twin
@pytest.mark.parametrize("P,pages", POOLS)
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_three_steps_equal_the_host_planned_pair(Hq, Hkv, P, pages):
    """(1, 63, 64, 200): 63 -> 64 fills a tile, 64 -> 65 opens one (and, at P = 64, a page), 200 has four splits
    at 64 keys per split."""
    K = _K()
    cache, twin = _twins(Hkv, LENGTHS[0], P, pages)
    step = K.DecodeStep(N, 320, Hq, Hkv, "cuda", keys_per_split=64)
    ids = list(H.SLOTS)
    for t in range(3):
        k, v, q = _rows(Hq, Hkv, 100 + t)
        want = _host_step(twin, ids, k, v, q, step.kps)
        step.prepare(cache, ids)
        step.append(cache, k, v)
        O, lse = step.attend(cache, q)
        _check_step(O, lse, want, len(ids))
        _same_pool(cache, twin)
    assert cache.lengths[2] == 203 and step.seq_rec[3, 3].item() == 4 and step.splits == 5


def test_default_keys_per_split_and_a_second_pool():
    """kps None is the library's rule at the step's own grid; one step object serves two pools in turn."""
    from quantizedattention_amd import _lib
    K = _K()
    Hq, Hkv = HEADS[0]
    step = K.DecodeStep(N, 320, Hq, Hkv, "cuda")
    assert step.kps == _lib.load().qattn_split_keys(Hkv * N, 1, 320, 64)
    assert step.splits == K.decode_step_splits(320, step.kps)
    pools = [_twins(Hkv, lengths, 64, 32) for lengths in LENGTHS]
    k, v, q = _rows(Hq, Hkv, 7)
    ids = [5, 4, 2]
    for cache, twin in pools:
        want = _host_step(twin, ids, k, v, q, step.kps)
        step.prepare(cache, ids)
        O, lse = step.append(cache, k, v).attend(cache, q)
        _check_step(O, lse, want, len(ids))
        _same_pool(cache, twin)


# ------------------------------------------------------------------------------ 3. window
@pytest.mark.parametrize("window,sinks", ((70, 3), (64, 0)))
@pytest.mark.parametrize("P,pages,lengths", ((64, 48, (60, 150, 300, 316)), (256, 48, (60, 197, 255, 330))))
def test_window_steps_equal_the_host_planned_pair(P, pages, lengths, window, sinks):
    """Under window 70 the sequences of 198 keys or more have a gap between the sink tile and the window's
    first tile (a sink split and window splits), the shorter ones do not; 197 -> 198 crosses over."""
    K = _K()
    Hq, Hkv = HEADS[0]
    cache, twin = _twins(Hkv, lengths, P, pages)
    step = K.DecodeStep(N, -(-320 // P) * P, Hq, Hkv, "cuda", keys_per_split=64, window=window, sinks=sinks)
    assert step.splits == K.decode_step_splits(step.max_keys, 64, window, sinks) <= 4
    ids = list(H.SLOTS)
    gaps = set()
    for t in range(3):
        k, v, q = _rows(Hq, Hkv, 200 + t)
        want = _host_step(twin, ids, k, v, q, step.kps, window, sinks)
        step.prepare(cache, ids)
        O, lse = step.append(cache, k, v).attend(cache, q)
        _check_step(O, lse, want, len(ids))
        _same_pool(cache, twin)
        gaps |= {r[5] > 0 for r in step.seq_rec.cpu().tolist()[:4]}
    assert gaps == {True, False}


# ------------------------------------------------------------------------------ 4. rope
def test_rope_step_equals_the_host_planned_rope_pair():
    K = _K()
    Hq, Hkv = HEADS[0]
    rope = K.Rope(K.rope_table(512, 10000., "cuda"))
    cache, twin = _twins(Hkv, LENGTHS[1], 64, 32)
    step = K.DecodeStep(N, 320, Hq, Hkv, "cuda", keys_per_split=128)
    ids = [2, 4, 0]
    for t in range(2):
        k, v, q = _rows(Hq, Hkv, 300 + t)
        want = _host_step(twin, ids, k, v, q, step.kps, rope=rope)
        step.prepare(cache, ids)
        O, lse = step.append(cache, k, v, rope=rope).attend(cache, q, rope=rope)
        _check_step(O, lse, want, len(ids))
        _same_pool(cache, twin)
    assert step.pos.cpu().tolist() == [cache.lengths[b] - 1 for b in ids] + [0] * 3


# ------------------------------------------------------------------------------ 5. graph
def test_captured_step_replays_over_moving_lengths():
    """append + attend captured once (a linear chain on one stream, static k, v, q), then four replays, each
    after prepare and copies into the static inputs: sequences leave and join, slot 0 goes 62 -> .. -> 67
    across a page boundary (P = 64), and every replay equals the twin's eager host-planned step."""
    K = _K()
    Hq, Hkv = HEADS[0]
    cache, twin = _twins(Hkv, (1, 62, 130, 200), 64, 32)
    step = K.DecodeStep(N, 320, Hq, Hkv, "cuda", keys_per_split=64)
    sk, sv, sq = _rows(Hq, Hkv, 1)
    ids = [4, 0, 5]
    want = _host_step(twin, ids, sk, sv, sq, step.kps)          # the eager warm-up step
    step.prepare(cache, ids)
    O, lse = step.append(cache, sk, sv).attend(cache, sq)
    _check_step(O, lse, want, len(ids))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                               # captured, not run: nothing moves here
        gO, glse = step.append(cache, sk, sv).attend(cache, sq)
    _same_pool(cache, twin)
    pages0 = len(cache.alloc.pages[0])
    for t, ids in enumerate(([4, 0, 5], [0, 2, 4, 5], [2, 0], [5, 0, 2, 4])):
        k, v, q = _rows(Hq, Hkv, 400 + t)
        want = _host_step(twin, ids, k, v, q, step.kps)
        step.prepare(cache, ids)
        sk.copy_(k), sv.copy_(v), sq.copy_(q)
        graph.replay()
        _check_step(gO, glse, want, len(ids))
        _same_pool(cache, twin)
    assert cache.lengths[0] == 67 and len(cache.alloc.pages[0]) == pages0 + 1


# ------------------------------------------------------------------------------ 6. bad slots
def test_bad_slots_move_nothing():
    K = _K()
    Hq, Hkv = HEADS[0]
    cache, twin = _twins(Hkv, LENGTHS[0], 64, 32)
    step = K.DecodeStep(N, 320, Hq, Hkv, "cuda", keys_per_split=64)
    k, v, q = _rows(Hq, Hkv, 5)
    held = [t.clone() for t in (*cache.kv, cache.vtail, cache.lens, cache.block_table)]
    step.slots.copy_(torch.tensor([-1, H.MAX_SEQS, -7, 1 << 30, -(1 << 31), -1], dtype=torch.int32))
    O, lse = step.append(cache, k, v).attend(cache, q)
    assert not O.any() and bool((lse == float("-inf")).all())
    for a, b in zip(held, (*cache.kv, cache.vtail, cache.lens, cache.block_table)):
        assert torch.equal(a, b)
    # bad values beside two listed sequences: those two are the twin's, the rest is padding
    step.prepare(cache, [4, 0])
    step.slots.copy_(torch.tensor([4, -1, H.MAX_SEQS, 0, -7, -1], dtype=torch.int32))
    O, lse = step.append(cache, k, v).attend(cache, q)
    RO, Rl = _host_step(twin, [4, 0], k[[0, 3]], v[[0, 3]], q[[0, 3]], step.kps)
    assert torch.equal(O[[0, 3]], RO) and torch.equal(lse[[0, 3]], Rl)
    assert not O[[1, 2, 4, 5]].any() and bool((lse[[1, 2, 4, 5]] == float("-inf")).all())
    _same_pool(cache, twin)


# ------------------------------------------------------------------------------ 7. operators
@pytest.mark.parametrize("window,sinks", ((None, 0), (70, 3)))
def test_operators_equal_the_python_entries(window, sinks):
    from quantizedattention_amd import ops
    K = _K()
    Hq, Hkv = HEADS[0]
    cache = H.fill_pool(Hkv, LENGTHS[1], 64, 32)
    step = K.DecodeStep(N, 320, Hq, Hkv, "cuda", keys_per_split=64, window=window, sinks=sinks)
    k, v, q = _rows(Hq, Hkv, 9)
    step.prepare(cache, [0, 5, 2, 4])
    tabs = ops.mxfp4_decode_step_plan(step, cache)            # before the append: the lengths it reads
    step.append(cache, k, v)
    for mine, op in zip((step.seq_tab, step.tiles, step.pos, step.seq_rec), tabs):
        assert mine.dtype == op.dtype and torch.equal(mine, op)
    O2, lse2 = ops.mxfp4_decode_step(q, step, cache, seq_rec=tabs[3])
    O, lse = step.attend(cache, q)
    assert O2.data_ptr() != O.data_ptr() and torch.equal(O, O2) and torch.equal(lse, lse2)
    assert bool((lse[4:] == float("-inf")).all()) and bool(torch.isfinite(lse[:4]).all())
