"""Rotary positions fused into the packed MX-FP4 cache path on the GPU: mxfp4_quantize_rows_rope
(qattn_mxfp4_quant_rows_rope), PagedKVFP4.append_packed / accept with rope=
(qattn_mxfp4_paged_append_packed_rope), attention_mxfp4_varlen_paged with rope= and the two operators.

One criterion throughout, torch.equal: a call with ``rope=`` gives the bytes of the same call without it on
rows rotated on the CPU by tests/mxfp4_rope_ref.py rope_ref, the contract written with separate fp32 tensor
operations.  No tolerance anywhere.  tests/test_mxfp4_rope_ref.py shows, on these very tensors, that a
kernel which fuses its multiply-adds, pairs the other way or is a position off would change the bytes
compared here.  No test feeds a position outside the table to a kernel.
"""
import pytest
import torch

import mxfp4_rope_ref as R
import mxfp4_varlen_helpers as H

pytestmark = pytest.mark.gpu

PAIRINGS = [False, True]
KPS = 64      # keys per split: both sequences of the attention tests then have two splits or more


def _rope(interleaved):
    from quantizedattention_amd.kv_cache_mxfp4 import Rope
    return Rope(R.table().cuda(), interleaved)


def _ref(x, pos, interleaved):
    return R.rope_ref(x, R.table(), pos, interleaved).cuda()


def _pool(k_mean=True, pages=16):
    from quantizedattention_amd.kv_cache_mxfp4 import PagedKVFP4
    return PagedKVFP4.allocate(pages, 64, R.SLOTS, R.HKV, 4, "cuda", k_mean=R.k_mean() if k_mean else None,
                               free_order=H.scatter(pages))


def _same_bytes(a, b):
    """Two pools that saw the same calls: every tensor and every host mirror, whole."""
    for name in ("k4", "ks", "vt", "vs", "vtail", "lens", "block_table"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert a.lengths == b.lengths == a.lens.cpu().tolist()
    assert a.alloc.pages == b.alloc.pages and a.alloc.table == b.alloc.table and a.free_pages == b.free_pages


# ------------------------------------------------------------------ 1. the quantiser
@pytest.mark.parametrize("interleaved", PAIRINGS)
def test_quantiser_equals_the_quantiser_of_rotated_rows(lib, interleaved):
    """67 tokens x 3 heads: 804 blocks, a partial fourth workgroup, an odd heads-per-token stride; positions
    0, max_pos - 1, repeats, a descending run; block magnitudes 2^5 and 2^14 apart, so the scale bytes
    depend on the rotated partner.  Host list, host tensor and device positions, an offset non-contiguous
    view of x, and a stream of its own."""
    from quantizedattention_amd.attention_mxfp4 import mxfp4_quantize_rows, mxfp4_quantize_rows_rope
    rope = _rope(interleaved)
    x, pos = R.quant_inputs()
    want4, wants = mxfp4_quantize_rows(_ref(x, pos, interleaved))
    assert len(set(wants.cpu().flatten().tolist())) >= 8       # many block scales
    xd = x.cuda()
    for p in (pos, torch.tensor(pos), torch.tensor(pos, dtype=torch.int32).cuda()):
        q4, qs = mxfp4_quantize_rows_rope(xd, rope, p)
        assert q4.shape == (R.QUANT_T * R.QUANT_H, 64) and qs.shape == (R.QUANT_T * R.QUANT_H, 4)
        assert torch.equal(q4, want4) and torch.equal(qs, wants)
    big = torch.zeros((R.QUANT_T + 1, R.QUANT_H, 256), dtype=torch.float16, device="cuda")
    view = big[1:, :, 64:192]
    view.copy_(xd)
    assert not view.is_contiguous()
    q4, qs = mxfp4_quantize_rows_rope(view, rope, pos)
    assert torch.equal(q4, want4) and torch.equal(qs, wants)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        q4, qs = mxfp4_quantize_rows_rope(xd, rope, pos)
    side.synchronize()
    assert torch.equal(q4, want4) and torch.equal(qs, wants)


# ------------------------------------------------------------------ 2. the append
def _positions(mode, step):
    if mode == "default":
        return None, R.STEP_POS[step]
    if mode == "device":
        return torch.tensor(R.STEP_POS[step], dtype=torch.int32).cuda(), R.STEP_POS[step]
    shifted = [p + R.SHIFT for p in R.STEP_POS[step]]
    return shifted, shifted


@pytest.mark.parametrize("mode", ["default", "device", "shifted"])
@pytest.mark.parametrize("interleaved", PAIRINGS)
def test_append_equals_the_append_of_rotated_keys(lib, interleaved, mode):
    """Two pools of one allocate (k_mean set, pages of 64, Hkv 2, three slots, slot 1 never listed): A
    appends k with rope=, B the keys rotated on the CPU.  Two steps, 0 -> 60 and 0 -> 5, then 60 -> 69 (over
    a page and a V tile) and 5 -> 6; after each, every tensor and mirror of the pools is equal byte for
    byte.  With the default positions, the same as a device tensor, and a shifted explicit list."""
    rope = _rope(interleaved)
    A, B = _pool(), _pool()
    for step, counts in enumerate(R.STEPS):
        k, v = R.append_inputs(step)
        given, used = _positions(mode, step)
        A.append_packed(k.cuda(), v.cuda(), R.IDS, counts, rope=rope, positions=given)
        B.append_packed(_ref(k, used, interleaved), v.cuda(), R.IDS, counts)
        _same_bytes(A, B)
        assert A.lengths[1] == 0 and not A.vtail[1].any() and not A.alloc.pages[1]
    assert A.lengths == [6, 0, 69]


# ------------------------------------------------------------------ 3. attention, every mode
_POOLS = {}


def _grown_pool(interleaved):
    """Pool B of the append test (keys rotated on the CPU), grown to 76 and 209 keys."""
    if interleaved not in _POOLS:
        cache = _pool()
        steps = [(R.append_inputs(s), R.STEP_POS[s], R.STEPS[s]) for s in range(2)]
        steps.append((R.grow_inputs(), R.GROW_POS, R.GROW))
        for (k, v), pos, counts in steps:
            cache.append_packed(_ref(k, pos, interleaved), v.cuda(), R.IDS, counts)
        assert tuple(cache.lengths) == R.LENGTHS
        _POOLS[interleaved] = cache
    return _POOLS[interleaved]


MODES = {
    "noncausal": dict(causal=False),
    "causal": dict(causal=True),
    "window": dict(causal=True, window=64, sinks=2),
    "shared": dict(causal=True, share_prefix=True),
    "tree": dict(causal=True, tree=[R.TREE, None]),
}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("interleaved", PAIRINGS)
def test_attention_equals_attention_of_rotated_queries(lib, interleaved, mode):
    """attention_mxfp4_varlen_paged(q, ..., rope=) against the same call on rope_ref(q, positions), O and
    lse, Hq 4 over Hkv 2 at 64 keys per split (4 and 2 splits; the window leaves a gap behind one sink
    tile; the fork shares three pages).  The default positions are the hand-written ones of the helper;
    for tree= they also equal the explicit rope_positions(..., tree=)."""
    from quantizedattention_amd.kv_cache_mxfp4 import (attention_mxfp4_varlen_paged, plan_varlen,
                                                       rope_positions)
    rope, cache, kw = _rope(interleaved), _grown_pool(interleaved), MODES[mode]
    ids, q_lens, pos = R.IDS, R.Q_LENS, R.Q_POS_TREE if mode == "tree" else R.Q_POS
    if mode == "shared":
        if not cache.lengths[1]:
            cache.fork(2, 1)
        ids, q_lens, pos = R.FORK_IDS, R.FORK_Q_LENS, R.FORK_Q_POS
        assert cache.prefix_groups(ids) == [([0, 2], 3)]
    _, seq_rec, _, _ = plan_varlen(cache.lengths, ids, q_lens, R.HQ, R.HKV, KPS, kw["causal"],
                                   kw.get("window"), kw.get("sinks", 0))
    assert all(rec[3] >= 2 for rec in seq_rec)
    q = R.attention_q(sum(q_lens))
    O, lse = attention_mxfp4_varlen_paged(q.cuda(), cache, ids, q_lens, keys_per_split=KPS, rope=rope, **kw)
    WO, Wl = attention_mxfp4_varlen_paged(_ref(q, pos, interleaved), cache, ids, q_lens, keys_per_split=KPS, **kw)
    assert torch.isfinite(Wl).all() and torch.equal(O, WO) and torch.equal(lse, Wl)
    if mode == "tree":
        before = [L - n for L, n in zip(cache.lengths, (q_lens[1], 0, q_lens[0]))]
        explicit = rope_positions(before, ids, q_lens, tree=kw["tree"])
        assert explicit == pos
        EO, El = attention_mxfp4_varlen_paged(q.cuda(), cache, ids, q_lens, keys_per_split=KPS, rope=rope,
                                              positions=torch.tensor(explicit, dtype=torch.int32).cuda(), **kw)
        assert torch.equal(EO, WO) and torch.equal(El, Wl)


# ------------------------------------------------------------------ 4. draft, verify, accept
def _invariant_equal(a, b, slot=0):
    """The pool's invariant against a twin: rows [0, L) of k4 / ks, tiles [0, ceil(L / 64)) of vt / vs through
    each pool's own table, the live vtail rows, lens and the mirrors (K rows past L are unspecified: the
    pool that drafted keeps the rejected drafts there)."""
    L = a.lengths[slot]
    assert a.lengths == b.lengths == a.lens.cpu().tolist() == b.lens.cpu().tolist()
    assert a.free_pages == b.free_pages and len(a.alloc.pages[slot]) == len(b.alloc.pages[slot])
    for x, y in zip(H.gather(a, slot), H.gather(b, slot)):
        assert torch.equal(x, y)
    assert torch.equal(a.vtail[slot, :, :L % 64], b.vtail[slot, :, :L % 64])


@pytest.mark.parametrize("interleaved", PAIRINGS)
def test_draft_and_accept_equal_a_pool_that_appended_the_path(lib, interleaved):
    """L0 = 61, a draft of six nodes appended with rope= and tree= (61 -> 67, over a tile edge), then accept
    of the path 0 1 3 4 with rope=, given the UNROTATED draft keys: the pool equals a fresh one that appended
    the prefill and then only the path's rows, rotated on the CPU to 61 .. 64 (V tile 0 quantised again and
    tile 1 begun).  The draft step itself is held to keys rotated by depth."""
    from quantizedattention_amd.kv_cache_mxfp4 import tree_path
    rope = _rope(interleaved)
    pk, pv = R.prefill_inputs()
    dk, dv = R.draft_inputs()
    pool, twin, fresh = (_pool(k_mean=False, pages=6) for _ in range(3))
    for c in (pool, twin, fresh):
        c.append_packed(_ref(pk, list(range(R.L0)), interleaved), pv.cuda(), [0], [R.L0])
    ckpt = pool.checkpoint([0])
    pool.append_packed(dk.cuda(), dv.cuda(), [0], [len(R.DRAFT)], rope=rope, tree=[R.DRAFT])
    twin.append_packed(_ref(dk, R.DRAFT_POS, interleaved), dv.cuda(), [0], [len(R.DRAFT)])
    _invariant_equal(pool, twin)
    path = tree_path(R.DRAFT, R.LEAF)
    pool.accept(ckpt, dk.cuda(), dv.cuda(), [0], [len(R.DRAFT)], [path], rope=rope)
    fresh.append_packed(_ref(dk[path], R.PATH_POS, interleaved), dv[path].cuda(), [0], [len(path)])
    assert pool.lengths[0] == R.L0 + 4 == 65
    _invariant_equal(pool, fresh)


# ------------------------------------------------------------------ 5. the operators
@pytest.mark.parametrize("interleaved", PAIRINGS)
def test_operators_equal_the_python_entries(lib, interleaved):
    from quantizedattention_amd import ops
    from quantizedattention_amd.attention_mxfp4 import mxfp4_quantize_rows_rope
    from quantizedattention_amd.kv_cache_mxfp4 import attention_mxfp4_varlen_paged
    rope = _rope(interleaved)
    x, pos = R.quant_inputs()
    want = mxfp4_quantize_rows_rope(x.cuda(), rope, pos)
    got = ops.mxfp4_quant_rows_rope(x.cuda(), rope, pos)
    raw = torch.ops.qattn.mxfp4_quant_rows_rope(x.cuda(), rope.table, torch.tensor(pos, dtype=torch.int32).cuda(),
                                                interleaved)
    for g in (got, raw):
        assert torch.equal(g[0], want[0]) and torch.equal(g[1], want[1])
    cache, q = _grown_pool(interleaved), R.attention_q().cuda()
    for causal in (False, True):
        WO, Wl = attention_mxfp4_varlen_paged(q, cache, R.IDS, R.Q_LENS, causal=causal, keys_per_split=KPS,
                                              rope=rope)
        O, lse = ops.mxfp4_varlen_paged(q, cache, R.IDS, R.Q_LENS, causal=causal, keys_per_split=KPS, rope=rope)
        assert torch.equal(O, WO) and torch.equal(lse, Wl)
    with pytest.raises(RuntimeError, match="window, share_prefix or tree"):
        ops.mxfp4_varlen_paged(q, cache, R.IDS, R.Q_LENS, causal=True, window=64, rope=rope)


def test_fake_kernels_give_shapes_and_dtypes(lib):
    import quantizedattention_amd.ops  # noqa: F401
    m = lambda *s, dt=torch.uint8: torch.empty(s, dtype=dt, device="meta")  # noqa: E731
    q4, qs = torch.ops.qattn.mxfp4_quant_rows_rope(m(9, 3, 128, dt=torch.float16), m(50, 128, dt=torch.float32),
                                                   m(9, dt=torch.int32), True)
    assert q4.shape == (27, 64) and qs.shape == (27, 4) and q4.dtype == qs.dtype == torch.uint8
    i32 = lambda *s: m(*s, dt=torch.int32)  # noqa: E731
    O, lse = torch.ops.qattn.mxfp4_varlen_paged_rope(
        m(9, 4, 128, dt=torch.float16), m(16, 2, 64, 64), m(16, 2, 64, 4), m(16, 2, 1, 128, 32), m(16, 2, 1, 128, 2),
        i32(3), i32(3, 4), i32(2, 8), i32(5, 4), 40, 1, 64, m(50, 128, dt=torch.float32), i32(9), False)
    assert O.shape == (9, 4, 128) and O.dtype == torch.float16 and O.device.type == "meta"
    assert lse.shape == (9, 4) and lse.dtype == torch.float32


# ------------------------------------------------------------------ 6. no rope, no change
def test_without_rope_nothing_changes(lib):
    """append_packed and the varlen call with rope=None spelled out give the bits of the positional calls (a
    guard for the shared bodies; the existing suites are what holds those calls)."""
    from quantizedattention_amd.kv_cache_mxfp4 import attention_mxfp4_varlen_paged
    A, B = _pool(), _pool()
    for step, counts in enumerate(R.STEPS):
        k, v = (t.cuda() for t in R.append_inputs(step))
        A.append_packed(k, v, R.IDS, counts)
        B.append_packed(k, v, R.IDS, counts, rope=None, positions=None, tree=None)
        _same_bytes(A, B)
    q = R.attention_q(2).cuda()
    O, lse = attention_mxfp4_varlen_paged(q, A, [2], [2], True, KPS)
    PO, Pl = attention_mxfp4_varlen_paged(q, B, [2], [2], True, KPS, None, 0, False, None, rope=None, positions=None)
    assert torch.equal(O, PO) and torch.equal(lse, Pl)
    rope = _rope(False)
    for kw in (dict(positions=[0] * 6), dict(tree=[None, None])):
        with pytest.raises(RuntimeError, match="without rope"):
            A.append_packed(*(t.cuda() for t in R.append_inputs(0)), R.IDS, R.STEPS[0], **kw)
    with pytest.raises(RuntimeError, match="outside the table"):
        A.append_packed(*(t.cuda() for t in R.append_inputs(1)), R.IDS, R.STEPS[1], rope=rope,
                        positions=[R.MAX_POS] * 10)
    _same_bytes(A, B)      # the refusals came before any page was reserved
