"""The device-planned verify step (kv_cache_mxfp4.VerifyStep) on the GPU.  One criterion throughout, torch.equal:
every listed entry gets, bit for bit, what the host-planned pair gives on a twin pool fed the same tokens --
``append_packed(k, v, ids, [K] * n[, rope=rope, tree=trees])`` followed by ``attention_mxfp4_varlen_paged(q, twin,
ids, [K] * n, causal=True, keys_per_split=step.kps, tree=trees[, rope=rope])`` -- and the pool holds the twin's
bytes.  Shapes are tests/mxfp4_varlen_helpers.py's: 6 slots, four of them in use, N = 6 entries, so at least two
are padding.
"""
import random

import pytest
import torch

import mxfp4_varlen_helpers as H

pytestmark = pytest.mark.gpu

N = H.MAX_SEQS
POOLS = ((64, 32), (256, 48))
LENGTHS = ((1, 63, 64, 200), (127, 130, 255, 70))


def _K():
    from quantizedattention_amd import kv_cache_mxfp4 as K
    return K


def chain(n):
    return list(range(-1, n - 1))


def wide(n):
    return [-1] + [0] * (n - 1)


def heap(n):
    return [-1] + [(t - 1) // 2 for t in range(1, n)]


def forest(n):
    """two roots, every other node under the node two before it"""
    return [-1, -1][:n] + list(range(n - 2))


SHAPES = (chain, wide, heap, forest)


def _rows(Hq, Hkv, K, seed):
    """(k, v [N * K, Hkv, 128], q [N * K, Hq, 128]) of one step; the rows of padding entries hold values too."""
    g = torch.Generator().manual_seed(seed)
    r = lambda h: torch.randn((N * K, h, H.D), generator=g).half().cuda()  # noqa: E731
    return r(Hkv), r(Hkv), r(Hq)


def _twins(Hkv, lengths, P, pages):
    return H.fill_pool(Hkv, lengths, P, pages), H.fill_pool(Hkv, lengths, P, pages)


def _same_pool(cache, twin):
    """lens, and per slot the gathered rows and tiles and the live vtail rows."""
    assert cache.lengths == twin.lengths and cache.alloc.pages == twin.alloc.pages
    assert cache.free_pages == twin.free_pages
    assert cache.lens.cpu().tolist() == cache.lengths and torch.equal(cache.lens, twin.lens)
    for b, L in enumerate(cache.lengths):
        if L == 0:
            continue
        for x, y in zip(H.gather(cache, b), H.gather(twin, b)):
            assert torch.equal(x, y), (b, L)
        assert torch.equal(cache.vtail[b, :, :L % 64], twin.vtail[b, :, :L % 64]), (b, L)


def _snapshot(cache):
    """What the invariant specifies of a pool: lengths, pages, and per slot the gathered rows and tiles and the
    live vtail rows, cloned."""
    rows = {b: [x.clone() for x in H.gather(cache, b)] + [cache.vtail[b, :, :L % 64].clone()]
            for b, L in enumerate(cache.lengths) if L}
    return list(cache.lengths), [list(p) for p in cache.alloc.pages], cache.free_pages, cache.lens.clone(), rows


def _assert_snapshot(cache, snap):
    lengths, pages, free, lens, rows = snap
    assert cache.lengths == lengths and cache.alloc.pages == pages and cache.free_pages == free
    assert torch.equal(cache.lens, lens)
    for b, held in rows.items():
        now = list(H.gather(cache, b)) + [cache.vtail[b, :, :lengths[b] % 64]]
        for x, y in zip(held, now):
            assert torch.equal(x, y), b


def _host_step(twin, ids, k, v, q, K, kps, trees, rope=None):
    Km = _K()
    n = len(ids)
    if rope is None:
        twin.append_packed(k[:n * K], v[:n * K], ids, [K] * n)
    else:
        twin.append_packed(k[:n * K], v[:n * K], ids, [K] * n, rope=rope, tree=trees)
    return Km.attention_mxfp4_varlen_paged(q[:n * K], twin, ids, [K] * n, causal=True, keys_per_split=kps,
                                           tree=trees, rope=rope)


def _check_step(O, lse, want, n, K):
    RO, Rl = want
    assert O.shape[0] == N * K and lse.dtype == torch.float32 and O.dtype == torch.float16
    assert torch.equal(O[:n * K], RO) and torch.equal(lse[:n * K], Rl)
    assert not O[n * K:].any() and bool((lse[n * K:] == float("-inf")).all())


# ------------------------------------------------------------------------------ 1. the plan kernel
@pytest.mark.parametrize("K", (1, 5, 64))
@pytest.mark.parametrize("kps", (64, 128))
@pytest.mark.parametrize("lengths", LENGTHS)
def test_plan_kernel_writes_the_host_statement(lengths, kps, K):
    from quantizedattention_amd import _lib
    Km = _K()
    Hq, Hkv = 4, 2
    cache = H.pool(Hkv, lengths, 64, 32)   # shared: only its lens is read here
    step = Km.VerifyStep(N, 320, Hq, Hkv, "cuda", K, keys_per_split=kps)
    assert step.splits == Km.verify_step_splits(320, kps) and step.kps == kps
    slots = [4, 0, 5, 2, -1, H.MAX_SEQS]
    # words as a caller might leave them: bits above the node set, the node's own bit missing in some
    clean = [w for i in range(N) for w in Km.tree_ancestor_masks(SHAPES[i % 4](K))]
    words = [((w | (0xff << (t % K + 1))) & ~((t % 3 == 0) << (t % K))) & ((1 << 64) - 1) for t, w in enumerate(clean)]
    step.slots.copy_(torch.tensor(slots, dtype=torch.int32))
    step.tree.copy_(torch.tensor([w - (1 << 64) if w >> 63 else w for w in words], dtype=torch.int64))
    a = cache.alloc
    cap = a.max_pages_per_seq * a.page_tokens
    _lib.call("qattn_mxfp4_verify_step_plan", _lib.ptr(step.slots), _lib.ptr(cache.lens), _lib.ptr(step.tree),
              _lib.ptr(step.seq_tab), _lib.ptr(step.tiles), _lib.ptr(step.seq_rec), _lib.ptr(step.pos), N, K,
              a.max_seqs, cap, Hkv, Hq // Hkv, kps, step.splits, _lib.stream_of(step.slots))
    tab, tiles, pos, rec, work = Km.plan_verify_step(cache.lengths, slots, K, words, kps, step.splits, Hkv,
                                                     Hq // Hkv, capacity=cap)
    assert (tab, tiles, pos, rec, work) == Km.plan_verify_step(cache.lengths, slots, K, clean, kps, step.splits,
                                                               Hkv, Hq // Hkv, capacity=cap)
    assert step.seq_tab.cpu().tolist() == tab and step.tiles.cpu().tolist() == tiles
    assert step.pos.cpu().tolist() == pos and step.seq_rec.cpu().tolist() == rec
    assert step.work.cpu().tolist() == work
    assert [r[3] for r in rec[4:]] == [0, 0] and min(r[3] for r in rec[:4]) >= 1


# ------------------------------------------------------------------------------ 2. three steps against a twin
CASES = {
    # K = 5 at 63 -> 68 crosses a tile and, at P = 64, a page; 64 keys per split: a split boundary inside the
    # tree keys, and short sequences with fewer splits than the grid holds
    "k5": (4, 2, 5, 64, (1, 63, 64, 200)),
    # G * K = 160 rows: a second, partly filled row block and waves that straddle a head boundary; 63 + 40
    # puts a tree's nodes in two key tiles
    "k40": (8, 2, 40, 64, (1, 63, 64, 200)),
    # the widest tree, at L = 1 and L = 64
    "k64": (4, 2, 64, 128, (1, 64, 100, 70)),
}


@pytest.mark.parametrize("P,pages", POOLS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_three_steps_equal_the_host_planned_pair(case, P, pages):
    Km = _K()
    Hq, Hkv, K, kps, lengths = CASES[case]
    cache, twin = _twins(Hkv, lengths, P, pages)
    step = Km.VerifyStep(N, 320, Hq, Hkv, "cuda", K, parents=heap(K), keys_per_split=kps)
    ids = list(H.SLOTS)
    for t in range(3):
        k, v, q = _rows(Hq, Hkv, K, 100 + t)
        shapes = [SHAPES[(j + t) % 4](K) for j in range(len(ids))]     # differ between entries and steps
        given = list(shapes)
        if t == 0:   # None is the step's default topology
            given[0] = given[2] = None
            shapes[0] = shapes[2] = heap(K)
        want = _host_step(twin, ids, k, v, q, K, step.kps, shapes)
        step.prepare(cache, ids, trees=given)
        step.append(cache, k, v)
        O, lse = step.attend(cache, q)
        _check_step(O, lse, want, len(ids), K)
        _same_pool(cache, twin)
    rec = step.seq_rec.cpu().tolist()
    assert [r[3] for r in rec[4:]] == [0, 0]
    assert len({r[3] for r in rec[:4]}) > 1 and max(r[3] for r in rec[:4]) <= step.splits
    assert step.nrb == (2 if case == "k40" else 1)


@pytest.mark.parametrize("P,pages", POOLS)
def test_one_draft_token_equals_the_decode_step(P, pages):
    """K = 1, parents [-1]: the host pair's bits and DecodeStep's on a third pool."""
    Km = _K()
    Hq, Hkv, lengths = 4, 2, LENGTHS[0]
    cache, twin = _twins(Hkv, lengths, P, pages)
    third = H.fill_pool(Hkv, lengths, P, pages)
    step = Km.VerifyStep(N, 320, Hq, Hkv, "cuda", 1, parents=[-1], keys_per_split=64)
    dec = Km.DecodeStep(N, 320, Hq, Hkv, "cuda", keys_per_split=64)
    ids = list(H.SLOTS)
    for t in range(3):
        k, v, q = _rows(Hq, Hkv, 1, 150 + t)
        want = _host_step(twin, ids, k, v, q, 1, step.kps, [[-1]] * 4)
        step.prepare(cache, ids)
        O, lse = step.append(cache, k, v).attend(cache, q)
        _check_step(O, lse, want, len(ids), 1)
        dec.prepare(third, ids)
        DO, Dl = dec.append(third, k, v).attend(third, q)
        assert torch.equal(O, DO) and torch.equal(lse, Dl)
        _same_pool(cache, twin)
        _same_pool(cache, third)


def test_default_keys_per_split():
    from quantizedattention_amd import _lib
    Km = _K()
    step = Km.VerifyStep(N, 320, 8, 2, "cuda", 40)
    assert step.nrb == 2 and step.kps == _lib.load().qattn_split_keys(2 * N * 2, 1, 320, 64)
    assert step.splits == Km.verify_step_splits(320, step.kps)
    assert step.tree.shape == (N * 40,) and step.tree.dtype == torch.int64 and step.tiles.shape == (2 * N, 2)
    assert step.O.shape == (N * 40, 8, 128) and step.lse.shape == (N * 40, 8)


# ------------------------------------------------------------------------------ 3. rope
@pytest.mark.parametrize("interleaved", (False, True))
def test_rope_step_equals_the_host_planned_rope_pair(interleaved):
    Km = _K()
    Hq, Hkv, K = 4, 2, 5
    rope = Km.Rope(Km.rope_table(512, 10000., "cuda"), interleaved=interleaved)
    cache, twin = _twins(Hkv, LENGTHS[1], 64, 32)
    step = Km.VerifyStep(N, 320, Hq, Hkv, "cuda", K, keys_per_split=128)
    ids = [2, 4, 0]
    for t in range(2):
        k, v, q = _rows(Hq, Hkv, K, 300 + t)
        shapes = [SHAPES[(j + t + 1) % 4](K) for j in range(len(ids))]
        want = _host_step(twin, ids, k, v, q, K, step.kps, shapes, rope=rope)
        step.prepare(cache, ids, trees=shapes)
        O, lse = step.append(cache, k, v, rope=rope).attend(cache, q, rope=rope)
        _check_step(O, lse, want, len(ids), K)
        _same_pool(cache, twin)
        before = [L - K for L in cache.lengths]
        assert step.pos.cpu().tolist() == Km.rope_positions(before, ids, [K] * 3, shapes) + [0] * (3 * K)


# ------------------------------------------------------------------------------ 4. graph
def test_captured_step_replays_over_rounds_of_speculation():
    """append + attend captured once (static k, v, q), then four rounds, each checkpoint -> prepare -> fill the
    static inputs -> replay -> accept of a random root-to-node path (three rounds) or rollback (one), driven
    identically on the twin.  Trees change between rounds; between rounds a sequence is freed, one joins in the
    freed slot and one is a fork of another."""
    Km = _K()
    Hq, Hkv, K = 4, 2, 5
    cache, twin = _twins(Hkv, (1, 62, 130, 200), 64, 40)
    step = Km.VerifyStep(N, 320, Hq, Hkv, "cuda", K, keys_per_split=64)
    sk, sv, sq = _rows(Hq, Hkv, K, 1)
    ids = [4, 0, 5]
    ckpts = [c.checkpoint(ids) for c in (cache, twin)]          # the eager warm-up round, rolled back
    want = _host_step(twin, ids, sk, sv, sq, K, step.kps, [chain(K)] * 3)
    step.prepare(cache, ids)
    O, lse = step.append(cache, sk, sv).attend(cache, sq)
    _check_step(O, lse, want, len(ids), K)
    for c, ck in zip((cache, twin), ckpts):
        c.rollback(ck)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                               # captured, not run: nothing moves here
        gO, glse = step.append(cache, sk, sv).attend(cache, sq)
    _same_pool(cache, twin)
    rng = random.Random(5)
    rounds = (([4, 0, 5], "accept"), ([0, 2, 4, 5], "rollback"), ([2, 0, 1], "accept"), ([5, 0, 3, 1], "accept"))
    for t, (ids, end) in enumerate(rounds):
        if t == 2:      # slot 4 leaves, a new sequence joins in a freed slot (1), slot 3 becomes a fork of 0
            g = torch.Generator().manual_seed(77)
            nk, nv = (torch.randn((1, Hkv, 9, H.D), generator=g).half().cuda() for _ in range(2))
            for c in (cache, twin):
                c.free([4])
                c.append_packed(nk[0].transpose(0, 1).contiguous(), nv[0].transpose(0, 1).contiguous(), [1], [9])
                c.fork(0, 3)
        n = len(ids)
        k, v, q = _rows(Hq, Hkv, K, 400 + t)
        shapes = [SHAPES[(j + t) % 4](K) for j in range(n)]
        snap = _snapshot(cache)
        ckpts = [c.checkpoint(ids) for c in (cache, twin)]
        want = _host_step(twin, ids, k, v, q, K, step.kps, shapes)
        step.prepare(cache, ids, trees=shapes)
        sk.copy_(k), sv.copy_(v), sq.copy_(q)
        graph.replay()
        _check_step(gO, glse, want, n, K)
        _same_pool(cache, twin)
        if end == "rollback":
            for c, ck in zip((cache, twin), ckpts):
                c.rollback(ck)
            _assert_snapshot(cache, snap)       # the pool's bytes before the checkpoint
        else:
            paths = [Km.tree_path(p, rng.randrange(K)) for p in shapes]
            for c, ck in zip((cache, twin), ckpts):
                c.accept(ck, k[:n * K], v[:n * K], ids, [K] * n, paths)
        _same_pool(cache, twin)
    assert cache.lengths[3] > 0 and cache.lengths[4] == 0


def test_rollback_restores_the_bytes_before_the_checkpoint():
    """checkpoint -> prepare -> step -> rollback: every byte the invariant specifies is what it was."""
    Km = _K()
    Hq, Hkv, K = 4, 2, 33
    cache, ref = _twins(Hkv, LENGTHS[0], 64, 32)
    step = Km.VerifyStep(N, 320, Hq, Hkv, "cuda", K, parents=heap(K), keys_per_split=64)
    ids = list(H.SLOTS)
    k, v, q = _rows(Hq, Hkv, K, 9)
    free = cache.free_pages
    ck = cache.checkpoint(ids)
    step.prepare(cache, ids)
    step.append(cache, k, v).attend(cache, q)
    assert cache.lengths[0] == 63 + K and cache.free_pages < free
    cache.rollback(ck)
    assert cache.free_pages == free
    _same_pool(cache, ref)


# ------------------------------------------------------------------------------ 5. refusals
def test_every_refusal_names_its_reason_and_changes_nothing():
    from quantizedattention_amd import _lib
    Km = _K()
    Hq, Hkv, K = 4, 2, 5
    cache = H.fill_pool(Hkv, (1, 63, 316, 200), 64, 32)
    step = Km.VerifyStep(N, 320, Hq, Hkv, "cuda", K)
    step.prepare(cache, [4])
    del cache.alloc._free[:]                                # the pool is full from here on
    state = lambda: (list(cache.lengths), [list(p) for p in cache.alloc.pages], cache.free_pages,  # noqa: E731
                     step.slots.cpu().tolist(), step.tree.cpu().tolist(), list(step.listed))
    held = state()
    assert held[3] == [4, -1, -1, -1, -1, -1] and held[0][4] == 6

    def refused(match, ids, trees=None, st=step, pool=cache):
        with pytest.raises(_lib.QAttnError, match=match):
            st.prepare(pool, ids, trees)
        assert state() == held, match

    refused("distinct", [4, 4])
    refused("distinct", [4, 6])
    refused("distinct", [-1])
    refused("at most 6", [0, 1, 2, 3, 4, 5, 0])
    refused("at least one cached token", [4, 1])
    refused("would pass 320 keys", [4, 5])                   # 316 + 5 passes the table row and max_keys
    small = Km.VerifyStep(N, 66, Hq, Hkv, "cuda", K)
    refused("would pass 66 keys", [0], st=small)             # 63 + 5 passes the step's max_keys
    refused("out of pages", [4, 0])                          # 63 -> 68 needs a page
    refused("5 draft", [4, 0], [None, chain(4)])
    refused("5 draft", [4, 0], [chain(6), None])
    refused("one entry", [4, 0], [None])
    refused("parent outside", [4, 0], [None, [-1, 0, 2, 1, 0]])
    refused("parent outside", [4, 0], [None, [-1, 0, 1, 3, 0]])
    other = H.fill_pool(4, (1, 63, 64, 200), 64, 32)
    with pytest.raises(_lib.QAttnError, match="2 key/value heads"):
        step.prepare(other, [4])
    assert state() == held
    big = H.fill_pool(Hkv, (1, 63, 64, 300), 64, 32)
    assert big.trim([2], 70, 3) > 0
    lengths, pages = list(big.lengths), [list(p) for p in big.alloc.pages]
    with pytest.raises(_lib.QAttnError, match="trimmed"):
        step.prepare(big, [4, 2])
    assert big.lengths == lengths and [list(p) for p in big.alloc.pages] == pages
    assert state() == held
    with pytest.raises(_lib.QAttnError, match=r"\[1, 64\]"):
        Km.VerifyStep(N, 320, Hq, Hkv, "cuda", 65)
    with pytest.raises(_lib.QAttnError, match="5 draft"):
        Km.VerifyStep(N, 320, Hq, Hkv, "cuda", 5, parents=chain(4))
    with pytest.raises(_lib.QAttnError, match="at most 64"):
        Km.VerifyStep(N, 320, Hq, Hkv, "cuda", 64, parents=chain(65))
    with pytest.raises(_lib.QAttnError, match="multiple of 64"):
        Km.VerifyStep(N, 320, Hq, Hkv, "cuda", 5, keys_per_split=96)
    k, v, q = _rows(Hq, Hkv, K, 3)
    with pytest.raises(_lib.QAttnError, match="k, v must be"):
        step.append(cache, k[:-1], v[:-1])
    with pytest.raises(_lib.QAttnError, match="q must be"):
        step.attend(cache, q[:, :2])
    rope = Km.Rope(Km.rope_table(4, 10000., "cuda"))
    with pytest.raises(_lib.QAttnError, match="positions reach"):
        step.append(cache, k, v, rope=rope)
    assert state() == held


def test_c_entries_refuse_bad_sizes():
    from quantizedattention_amd import _lib
    lib = _lib.load()
    Km = _K()
    step = Km.VerifyStep(N, 320, 4, 2, "cuda", 5, keys_per_split=64)
    cache = H.pool(2, LENGTHS[0], 64, 32)
    p = _lib.ptr
    plan = lambda n=N, K=5, B=6, cap=320, hkv=2, g=2, kps=64, splits=5: lib.qattn_mxfp4_verify_step_plan(  # noqa: E731
        p(step.slots), p(cache.lens), p(step.tree), p(step.seq_tab), p(step.tiles), p(step.seq_rec), p(step.pos),
        n, K, B, cap, hkv, g, kps, splits, None)
    assert plan(n=0) == 0
    for bad in (dict(K=0), dict(K=65), dict(n=-1), dict(B=0), dict(cap=100), dict(cap=0), dict(hkv=0), dict(g=0),
                dict(kps=96), dict(kps=0), dict(splits=0), dict(splits=65536), dict(n=1 << 40)):
        assert plan(**bad) == 1, bad
    comb = lambda n=N, K=5, splits=5, hq=4, hkv=2, D=128: lib.qattn_mxfp4_verify_step_combine(  # noqa: E731
        p(step.opart), p(step.ml), p(step.O), p(step.lse), p(step.seq_rec), n, K, splits, hq, hkv, D, None)
    assert comb(n=0) == 0
    for bad in (dict(K=0), dict(K=65), dict(splits=0), dict(hq=3), dict(hkv=0), dict(D=64), dict(n=1 << 40)):
        assert comb(**bad) == 1, bad
