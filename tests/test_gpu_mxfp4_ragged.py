"""The preallocated MX-FP4 cache on the GPU: PreallocatedKVFP4 (qattn_mxfp4_cache_append),
attention_mxfp4_decode (qattn_mxfp4_attn_fwd_split_len) and torch.ops.qattn.mxfp4_decode.

References: the cache's own invariant (quantize_kv_fp4 of the zero-padded prefix, bit for bit), the
existing key-split kernel (bit for bit, on full tiles and through the identity shown on the CPU in
tests/test_mxfp4_ragged_ref.py) and the restatement tests/mxfp4_ragged_ref.py at the project's MX-FP4
bars of tests/test_gpu_mxfp4_cache.py: O max-abs <= 2e-2, lse <= 1e-4, relL2 <= 2e-3 on the cases with
at least 64 query rows.  Measured values are printed as "MXFP4-RAGGED ...".
"""
import pytest
import torch

import mxfp4_masked_ref as MR
import mxfp4_ragged_ref as RR

pytestmark = pytest.mark.gpu

SENTINEL = -12288.0   # exact in fp16


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-30)).item()


def _fill(ks, vs, cap, k_mean=None):
    """A cache holding the sequences ks / vs (per sequence [1, Hkv, L_b, 128]) after ONE append with
    counts; the tokens a sequence does not take are garbage."""
    from quantizedattention_amd.kv_cache_mxfp4 import PreallocatedKVFP4
    B, Hkv, lens = len(ks), ks[0].shape[1], [k.shape[2] for k in ks]
    n = max(lens)
    k = torch.full((B, Hkv, n, 128), 777.0, dtype=torch.float16)
    v = torch.full((B, Hkv, n, 128), -555.0, dtype=torch.float16)
    for b, L in enumerate(lens):
        k[b, :, :L], v[b, :, :L] = ks[b][0], vs[b][0]
    cache = PreallocatedKVFP4.allocate(B, Hkv, cap, "cuda", k_mean)
    cache.append(k.cuda(), v.cuda(), counts=lens)
    assert cache.lengths == lens
    return cache


def _check_bars(tag, O, lse, RO, Rl, nrows):
    O, lse = O.cpu(), lse.cpu()
    assert torch.isfinite(O.float()).all() and torch.isfinite(lse).all()
    err = (O.float() - RO.float()).abs().max().item()
    rel, lerr = _rel(O, RO), (lse - Rl).abs().max().item()
    print(f"MXFP4-RAGGED {tag} maxabs {err:.3e} relL2 {rel:.3e} lse {lerr:.3e} "
          f"O bit-equal {torch.equal(O, RO)}")
    assert err <= 2e-2, err
    assert lerr <= 1e-4, lerr
    if nrows >= 64:
        assert rel <= 2e-3, rel


# ------------------------------------------------------------------ 1. the append invariant
def _assert_invariant(cache, k, v, k_mean):
    from quantizedattention_amd.kv_cache_mxfp4 import quantize_kv_fp4
    B, H, cap, D = cache.shape
    assert cache.lens.cpu().tolist() == cache.lengths
    for b, L in enumerate(cache.lengths):
        if L == 0:
            continue
        nt = -(-L // 64)
        want = quantize_kv_fp4(RR.pad64(k[b:b + 1, :, :L]).cuda(), RR.pad64(v[b:b + 1, :, :L]).cuda(),
                               smooth=False, k_mean=None if k_mean is None else k_mean[b:b + 1])
        assert torch.equal(cache.k4[b, :, :L], want.k4[0, :, :L]), (b, L)
        assert torch.equal(cache.ks[b, :, :L], want.ks[0, :, :L]), (b, L)
        assert torch.equal(cache.vt[b * H:b * H + H, :nt], want.vt), (b, L)
        assert torch.equal(cache.vs[b * H:b * H + H, :nt], want.vs), (b, L)


@pytest.mark.parametrize("smoothed", [False, True])
def test_append_invariant(lib, smoothed):
    """Sequence 0 reaches a tile boundary exactly (1 + 62 + 1), starts on one, crosses 128 and 192
    inside a call and fills to the capacity; sequence 1 takes other counts, 0 among them."""
    from quantizedattention_amd import _lib
    from quantizedattention_amd.kv_cache_mxfp4 import PreallocatedKVFP4
    g = torch.Generator().manual_seed(11)
    k = torch.randn((2, 2, 256, 128), generator=g).half()
    v = torch.randn((2, 2, 256, 128), generator=g).half()
    k_mean = torch.randn((2, 2, 1, 128), generator=g).half().cuda() if smoothed else None
    cache = PreallocatedKVFP4.allocate(2, 2, 256, "cuda", k_mean)
    assert cache.lengths == [0, 0] and cache.capacity == 256 and cache.shape == (2, 2, 256, 128)
    for n, c1 in zip((1, 62, 1, 1, 70, 64, 57), (1, 0, 1, 1, 33, 64, 7)):
        kn = torch.full((2, 2, n, 128), 999.0, dtype=torch.float16)   # what is not taken is garbage
        vn = torch.full((2, 2, n, 128), -999.0, dtype=torch.float16)
        for b, c in enumerate((n, c1)):
            L = cache.lengths[b]
            kn[b, :, :c], vn[b, :, :c] = k[b, :, L:L + c], v[b, :, L:L + c]
        assert cache.append(kn.cuda(), vn.cuda(), counts=[n, c1]) is cache
        _assert_invariant(cache, k, v, k_mean)
    assert cache.lengths == [256, 107]
    before = [t.clone() for t in (*cache.kv, cache.vtail, cache.lens)]
    one = torch.ones((2, 2, 1, 128), dtype=torch.float16, device="cuda")
    with pytest.raises(_lib.QAttnError, match="capacity"):
        cache.append(one, one)                      # sequence 0 is full
    torch.cuda.synchronize()
    assert cache.lengths == [256, 107]
    for a, b in zip(before, (*cache.kv, cache.vtail, cache.lens)):
        assert torch.equal(a, b)
    # without counts every sequence takes all n; reset empties a sequence
    cache.reset([0])
    assert cache.lengths == [0, 107] and cache.lens.cpu().tolist() == [0, 107]
    kn = torch.stack([k[0, :, :5], k[1, :, 107:112]]).cuda()
    vn = torch.stack([v[0, :, :5], v[1, :, 107:112]]).cuda()
    cache.append(kn, vn)
    assert cache.lengths == [5, 112]
    _assert_invariant(cache, k, v, k_mean)


# ------------------------------------------------------------------ 2. full tiles = the cached forward
@pytest.mark.parametrize("shape", [(2, 4, 2, 1, 256), (1, 4, 1, 33, 192)])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("plan", [False, True])
def test_full_tiles_equal_the_cached_forward(lib, shape, causal, plan):
    from quantizedattention_amd.kv_cache_mxfp4 import (_split_plan_fp4, attention_mxfp4_cached,
                                                       attention_mxfp4_decode)
    B, Hq, Hkv, Sq, L = shape
    q, k, v = MR.randn_qkv(shape)
    cache = _fill([k[b:b + 1] for b in range(B)], [v[b:b + 1] for b in range(B)], 384)
    q = q.cuda()
    # the plan is taken for the batch; the snapshots (batch 1) are given the same split
    kps = _split_plan_fp4(B * Hkv, (Hq // Hkv) * Sq, L) if plan else 64
    O, lse = attention_mxfp4_decode(q, cache, causal=causal, keys_per_split=None if plan else 64)
    assert O.shape == (B, Hq, Sq, 128) and lse.shape == (B * Hq, Sq) and lse.dtype == torch.float32
    for b in range(B):
        O1, l1 = attention_mxfp4_cached(q[b:b + 1], cache.snapshot(b), causal=causal, keys_per_split=kps)
        assert torch.equal(O[b:b + 1], O1) and torch.equal(lse[b * Hq:b * Hq + Hq], l1), b


# ------------------------------------------------------------------ 3. ragged = the existing kernel
@pytest.mark.parametrize("Sq,lens,causal", [(1, (100, 64, 1, 191), False), (5, (100, 64, 5, 191), True)])
def test_ragged_equals_the_existing_kernel(lib, Sq, lens, causal):
    """The identity of tests/test_mxfp4_ragged_ref.py: sequence b is the first Sq rows of the existing
    bottom-right kernel on the zero-padded keys with Sq + ceil64(L) - L query rows."""
    from quantizedattention_amd.kv_cache_mxfp4 import (attention_mxfp4_cached, attention_mxfp4_decode,
                                                       quantize_kv_fp4)
    q, ks, vs = RR.inputs(4, 4, 1, Sq, lens)
    cache = _fill(ks, vs, 256)
    O, lse = attention_mxfp4_decode(q.cuda(), cache, causal=causal, keys_per_split=64)
    for b in range(4):
        q2, kp, vp = RR.identity_problem(q[b:b + 1], ks[b], vs[b], causal)
        O2, l2 = attention_mxfp4_cached(q2.cuda(), quantize_kv_fp4(kp.cuda(), vp.cuda(), smooth=False),
                                        causal=True, keys_per_split=64)
        assert torch.equal(O[b], O2[0, :, :Sq]), b
        assert torch.equal(lse[4 * b:4 * b + 4], l2[:, :Sq]), b


# ------------------------------------------------------------------ 4. against the restatement
@pytest.mark.parametrize("case,smoothed", [(c, False) for c in RR.CASES] + [(RR.CASES[1], True)])
def test_ragged_vs_restatement(lib, case, smoothed):
    from quantizedattention_amd.kv_cache_mxfp4 import attention_mxfp4_decode
    B, Hq, Hkv, Sq, lens, causal, kps = case
    q, ks, vs, RO, Rl = RR.case_reference(case, smoothed)
    k_mean = torch.cat([RR.k_mean_of(k) for k in ks]).cuda() if smoothed else None
    cache = _fill(ks, vs, 256, k_mean)
    O, lse = attention_mxfp4_decode(q.cuda(), cache, causal=bool(causal), keys_per_split=kps)
    torch.cuda.synchronize()
    _check_bars(f"{case} smoothed={smoothed}", O, lse, RO, Rl, B * Hq * Sq)


# ------------------------------------------------------------------ 5. bytes past the length
@pytest.mark.parametrize("case", RR.CASES[:2])
def test_bytes_past_the_length_never_matter(lib, case):
    """K rows and scales at or past L and V tiles at or past ceil(L / 64), up to the capacity, filled
    with 0xFF (scale byte 255 is NaN): O and lse do not move by a bit and are finite."""
    from quantizedattention_amd.kv_cache_mxfp4 import attention_mxfp4_decode
    B, Hq, Hkv, Sq, lens, causal, kps = case
    q, ks, vs = RR.inputs(B, Hq, Hkv, Sq, lens)
    cache = _fill(ks, vs, 256)
    q = q.cuda()
    O, lse = attention_mxfp4_decode(q, cache, causal=bool(causal), keys_per_split=kps)
    for b, L in enumerate(lens):
        nt = -(-L // 64)
        cache.k4[b, :, L:] = 0xFF
        cache.ks[b, :, L:] = 0xFF
        cache.vt[b * Hkv:b * Hkv + Hkv, nt:] = 0xFF
        cache.vs[b * Hkv:b * Hkv + Hkv, nt:] = 0xFF
    O2, lse2 = attention_mxfp4_decode(q, cache, causal=bool(causal), keys_per_split=kps)
    assert torch.equal(O, O2) and torch.equal(lse, lse2)
    assert torch.isfinite(O2.float()).all() and torch.isfinite(lse2).all()


# ------------------------------------------------------------------ 6. empty splits and row tails
def test_empty_splits_and_row_tails(lib):
    """The C entry on flat buffers: lens (64, 256), 64 keys per split, rows = 5 (G = 5, one query
    position), 128 sentinel rows behind every output."""
    from quantizedattention_amd import _lib
    from quantizedattention_amd.attention_mxfp4 import _qk_scale, mxfp4_quantize_rows
    from quantizedattention_amd.kv_cache_mxfp4 import attention_mxfp4_decode
    q, ks, vs = RR.inputs(2, 5, 1, 1, (64, 256))
    cache = _fill(ks, vs, 256)
    q = q.cuda()
    R, ns, D, pad = 10, 4, 128, 128
    q4, qs = mxfp4_quantize_rows(q)
    opart = torch.full(((ns * R + pad) * D,), SENTINEL, dtype=torch.float32, device="cuda")
    ml = torch.full(((ns * R + pad) * 2,), SENTINEL, dtype=torch.float32, device="cuda")
    out = torch.full(((R + pad) * D,), SENTINEL, dtype=torch.float16, device="cuda")
    lse = torch.full((R + pad,), SENTINEL, dtype=torch.float32, device="cuda")
    st = _lib.stream_of(q)
    _lib.call("qattn_mxfp4_attn_fwd_split_len", _lib.ptr(q4), _lib.ptr(qs), *(_lib.ptr(t) for t in cache.kv),
              _lib.ptr(opart), _lib.ptr(ml), _lib.ptr(cache.lens), 2, 1, 5, 1, 256, 256, 0, 64, D,
              _qk_scale(D), st)
    torch.cuda.synchronize()
    for t in (opart[ns * R * D:], ml[ns * R * 2:], out, lse):
        assert t.numel() >= 128 and (t == SENTINEL).all()
    _lib.call("qattn_mxfp4_split_combine", _lib.ptr(opart), _lib.ptr(ml), _lib.ptr(out), _lib.ptr(lse),
              R, ns, D, st)
    torch.cuda.synchronize()
    for t in (opart[ns * R * D:], ml[ns * R * 2:], out[R * D:], lse[R:]):
        assert t.numel() >= 128 and (t == SENTINEL).all()
    op, m = opart[:ns * R * D].view(ns, R, D).cpu(), ml[:ns * R * 2].view(ns, R, 2).cpu()
    assert not (op == SENTINEL).any() and not (m == SENTINEL).any()      # every partial row written
    empty = torch.isinf(m[..., 0]) & (m[..., 0] < 0)
    want = torch.zeros((4, 10), dtype=torch.bool)
    want[1:, :5] = True                     # splits 1-3 of sequence 0 (64 keys: one tile)
    assert torch.equal(empty, want)
    assert (m[..., 1][empty] == 0).all() and (op[empty] == 0).all()
    assert (m[..., 1][~empty] > 0).all()
    fin = m[..., 0][~empty]
    assert torch.equal(fin, fin.round())
    O, l2 = attention_mxfp4_decode(q, cache, keys_per_split=64)
    assert torch.equal(out[:R * D].view(R, D), O.reshape(R, D)) and torch.equal(lse[:R], l2.reshape(-1))
    assert torch.isfinite(O.float()).all() and torch.isfinite(l2).all()


# ------------------------------------------------------------------ 7. each sequence = its run alone
@pytest.mark.parametrize("causal", [False, True])
def test_each_sequence_equals_its_run_alone(lib, causal):
    from quantizedattention_amd.kv_cache_mxfp4 import attention_mxfp4_decode
    q, ks, vs = RR.inputs(3, 4, 2, 3, (37, 128, 200), seed=5)
    q = q.cuda()
    O, lse = attention_mxfp4_decode(q, _fill(ks, vs, 256), causal=causal, keys_per_split=64)
    for b in range(3):
        O1, l1 = attention_mxfp4_decode(q[b:b + 1], _fill(ks[b:b + 1], vs[b:b + 1], 256), causal=causal,
                                        keys_per_split=64)
        assert torch.equal(O[b:b + 1], O1) and torch.equal(lse[4 * b:4 * b + 4], l1), b


# ------------------------------------------------------------------ 8. a decode loop
def test_decode_loop(lib):
    """70 tokens in one append, then 60 steps of one appended token and one causal query."""
    from quantizedattention_amd.kv_cache_mxfp4 import (PreallocatedKVFP4, attention_mxfp4_cached,
                                                       attention_mxfp4_decode, quantize_kv_fp4)
    g = torch.Generator().manual_seed(7)
    k = torch.randn((1, 1, 130, 128), generator=g).half()
    v = torch.randn((1, 1, 130, 128), generator=g).half()
    qs = torch.randn((130, 1, 4, 1, 128), generator=g).half()
    kd, vd, qd = k.cuda(), v.cuda(), qs.cuda()
    cache = PreallocatedKVFP4.allocate(1, 1, 192, "cuda")
    cache.append(kd[:, :, :70], vd[:, :, :70])
    outs = {}
    for t in range(70, 130):
        cache.append(kd[:, :, t:t + 1], vd[:, :, t:t + 1])
        outs[t + 1] = attention_mxfp4_decode(qd[t], cache, causal=True)
    torch.cuda.synchronize()
    assert cache.lengths == [130] and cache.lens.cpu().tolist() == [130]
    for L, (O, lse) in outs.items():
        assert torch.isfinite(O.float()).all() and torch.isfinite(lse).all(), L
    O1, l1 = attention_mxfp4_cached(qd[127], quantize_kv_fp4(kd[:, :, :128], vd[:, :, :128], smooth=False),
                                    causal=True)
    assert torch.equal(outs[128][0], O1) and torch.equal(outs[128][1], l1)
    for L in (71, 127, 129):
        RO, Rl, _ = RR.mxfp4_fwd_ragged(qs[L - 1], [k[:, :, :L]], [v[:, :, :L]], True)
        _check_bars(f"decode loop L={L}", *outs[L], RO, Rl, 4)


# ------------------------------------------------------------------ 9. the operator
def test_operator_equals_the_python_call(lib):
    import quantizedattention_amd.ops as ops
    from quantizedattention_amd.kv_cache_mxfp4 import attention_mxfp4_decode
    B, Hq, Hkv, Sq, lens, causal, kps = case = RR.CASES[1]
    q, ks, vs, _, _ = RR.case_reference(case)
    cache = _fill(ks, vs, 256)
    q = q.cuda()
    for split in (kps, None):
        O, lse = attention_mxfp4_decode(q, cache, causal=bool(causal), keys_per_split=split)
        O1, l1 = ops.mxfp4_decode(q, cache, causal=bool(causal), keys_per_split=split)
        assert torch.equal(O, O1) and torch.equal(lse, l1)
        O2, l2 = torch.ops.qattn.mxfp4_decode(q, *cache.kv, cache.lens, 256, 1, 0 if split is None else split)
        assert torch.equal(O, O2) and torch.equal(lse, l2)
