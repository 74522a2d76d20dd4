"""MX-FP4 key/value cache on the GPU: QuantizedKVFP4, attention_mxfp4_cached and the C entries
qattn_mxfp4_attn_fwd_split / qattn_mxfp4_split_combine.

The reference is the ONE-PASS restatement tests/mxfp4_masked_ref.py (tests/test_mxfp4_cache_ref.py
shows on the CPU that the split definition equals it).  Bars are the project's MX-FP4 bars of
tests/test_gpu_mxfp4.py: operands bit-exact, O max-abs <= 2e-2, lse <= 1e-4 on every case, and
relL2 <= 2e-3 on the cases with at least 64 query rows (one flipped fp4 code in a 4-row case can
exceed a relative bar that was set on hundreds of rows).  Measured values are printed as
"MXFP4-CACHE ...".
"""
import pytest
import torch

import mxfp4_masked_ref as MR
import mxfp4_split_ref as SR
from oracle import mxfp4 as M

pytestmark = pytest.mark.gpu

HUGE = 60000.0
SENTINEL = -12288.0   # exact in fp16


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-30)).item()


def _cache(k, v, smooth=False):
    from quantizedattention_amd.kv_cache_mxfp4 import quantize_kv_fp4
    return quantize_kv_fp4(k.cuda(), v.cuda(), smooth=smooth)


# ------------------------------------------------------------------ 4. one split = the one-pass kernel
@pytest.mark.parametrize("shape,causal", [((1, 4, 2, 32, 256), 0), ((2, 4, 1, 64, 192), 2)])
def test_one_split_is_the_one_pass_kernel(lib, shape, causal):
    from quantizedattention_amd.attention_mxfp4 import mxfp4_attn_fwd, mxfp4_attn_fwd_kv
    from quantizedattention_amd.kv_cache_mxfp4 import attention_mxfp4_cached
    q, k, v = (t.cuda() for t in MR.randn_qkv(shape))
    Sk = shape[4]
    kv = _cache(k, v)
    O, lse = attention_mxfp4_cached(q, kv, causal=bool(causal), keys_per_split=Sk)
    O1, lse1 = mxfp4_attn_fwd_kv(q, kv.kv, causal=causal)
    torch.cuda.synchronize()
    assert O.shape == O1.shape and lse.shape == lse1.shape and lse.dtype == torch.float32
    assert torch.equal(O, O1) and torch.equal(lse, lse1)
    kvs = _cache(k, v, smooth=True)
    assert kvs.k_mean is not None and kvs.k_mean.shape == (shape[0], shape[2], 1, 128)
    Os, _ = attention_mxfp4_cached(q, kvs, causal=bool(causal), keys_per_split=Sk)
    Or, _, ops = mxfp4_attn_fwd(q, k, v, smooth_k=True, causal=causal)
    assert torch.equal(Os, Or)
    for a, b in zip(kvs.kv, ops[2:]):
        assert torch.equal(a.reshape(b.shape), b)


# ------------------------------------------------------------------ 5. split vs the restatement
@pytest.mark.parametrize("case,qmul", [(c, 1) for c in SR.CASES] + [(SR.CASES[5], 3)])
def test_split_vs_restatement(lib, case, qmul):
    from quantizedattention_amd.attention_mxfp4 import mxfp4_quantize_rows
    from quantizedattention_amd.kv_cache_mxfp4 import attention_mxfp4_cached
    B, H, Hkv, Sq, Sk, causal, kps = case
    q, k, v, RO, Rl, rops = SR.case_reference(case, qmul)
    kv = _cache(k, v)
    q4, qs = mxfp4_quantize_rows(q.cuda())
    for a, b in zip((q4, qs) + kv.kv, rops):
        assert torch.equal(a.cpu().reshape(b.shape), b)
    O, lse = attention_mxfp4_cached(q.cuda(), kv, causal=bool(causal), keys_per_split=kps)
    torch.cuda.synchronize()
    assert O.shape == (B, H, Sq, 128) and lse.shape == (B * H, Sq)
    O, lse = O.cpu(), lse.cpu()
    assert torch.isfinite(O.float()).all() and torch.isfinite(lse).all()
    err = (O.float() - RO.float()).abs().max().item()
    rel, lerr = _rel(O, RO), (lse - Rl).abs().max().item()
    print(f"MXFP4-CACHE {case} qx{qmul} maxabs {err:.3e} relL2 {rel:.3e} lse {lerr:.3e} "
          f"O bit-equal {torch.equal(O, RO)}")
    assert err <= 2e-2, err
    assert lerr <= 1e-4, lerr
    if B * H * Sq >= 64:
        assert rel <= 2e-3, rel


# ------------------------------------------------------------------ the C entries, called directly
def _c_split(q, kv, G, sq_head, causal, kps, pad_rows=0, fill=float("nan")):
    """qattn_mxfp4_attn_fwd_split + qattn_mxfp4_split_combine on flat buffers with ``pad_rows`` extra
    rows of ``fill`` behind each -> (opart [ns, R, D], ml [ns, R, 2], out [R, D], lse [R], tails)."""
    from quantizedattention_amd import _lib
    from quantizedattention_amd.attention_mxfp4 import _qk_scale, mxfp4_quantize_rows
    B, Hkv, Sk, D = kv.shape
    bhv, rows = B * Hkv, G * sq_head
    R, ns = bhv * rows, -(-Sk // kps)
    q4, qs = mxfp4_quantize_rows(q)
    dev = q.device
    opart = torch.full(((ns * R + pad_rows) * D,), fill, dtype=torch.float32, device=dev)
    ml = torch.full(((ns * R + pad_rows) * 2,), fill, dtype=torch.float32, device=dev)
    out = torch.full(((R + pad_rows) * D,), fill, dtype=torch.float16, device=dev)
    lse = torch.full((R + pad_rows,), fill, dtype=torch.float32, device=dev)
    st = _lib.stream_of(q)
    _lib.call("qattn_mxfp4_attn_fwd_split", _lib.ptr(q4), _lib.ptr(qs), *(_lib.ptr(t) for t in kv.kv),
              _lib.ptr(opart), _lib.ptr(ml), bhv, rows, sq_head, Sk, causal, kps, D, _qk_scale(D), st)
    torch.cuda.synchronize()
    after_split = (opart[ns * R * D:].clone(), ml[ns * R * 2:].clone(), out.clone(), lse.clone())
    _lib.call("qattn_mxfp4_split_combine", _lib.ptr(opart), _lib.ptr(ml), _lib.ptr(out), _lib.ptr(lse),
              R, ns, D, st)
    torch.cuda.synchronize()
    tails = (opart[ns * R * D:], ml[ns * R * 2:], out[R * D:], lse[R:])
    return (opart[:ns * R * D].view(ns, R, D), ml[:ns * R * 2].view(ns, R, 2), out[:R * D].view(R, D),
            lse[:R], tails, after_split)


# ------------------------------------------------------------------ 6. empty partials
def test_empty_partials(lib):
    case = SR.CASES[5]
    assert case == (1, 2, 1, 96, 256, 2, 64)
    q, k, v, RO, Rl, _ = SR.case_reference(case, 1)
    kv = _cache(k, v)
    opart, ml, out, lse, _, _ = _c_split(q.cuda(), kv, 2, 96, 2, 64)
    opart, ml, out, lse = opart.cpu(), ml.cpu(), out.cpu(), lse.cpu()
    assert not torch.isnan(opart).any() and not torch.isnan(ml).any()      # every partial row written
    empty = torch.isinf(ml[..., 0]) & (ml[..., 0] < 0)
    want = torch.zeros((4, 192), dtype=torch.bool)
    want[3, 0:32] = True        # head 0, query positions 0..31: keys <= 191, nothing of split 3
    want[3, 96:128] = True      # head 1
    assert int(empty.sum()) == 64 and torch.equal(empty, want)
    assert (ml[..., 1][empty] == 0).all() and (opart[empty] == 0).all()
    assert (ml[..., 1][~empty] > 0).all()
    fin = ml[..., 0][~empty]
    assert torch.equal(fin, fin.round())
    assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all()
    RO = RO.reshape(192, 128)
    assert (out.float() - RO.float()).abs().max().item() <= 2e-2
    assert _rel(out, RO) <= 2e-3
    assert (lse - Rl.reshape(-1)).abs().max().item() <= 1e-4


# ------------------------------------------------------------------ the merge, bit for bit
def _merge(opart, ml, rec, T, Hq, Hkv):
    """qattn_mxfp4_varlen_combine (``rec``: its seq_rec rows) or, rec None, qattn_mxfp4_split_combine of
    the padded partials, on the GPU -> (out fp16 [T * Hq, D], lse fp32 [T * Hq]) on the CPU."""
    from quantizedattention_amd import _lib
    D = opart.shape[-1]
    op_d, ml_d = opart.cuda().contiguous(), ml.cuda().contiguous()
    out = torch.full((T * Hq, D), SENTINEL, dtype=torch.float16, device="cuda")
    lse = torch.full((T * Hq,), SENTINEL, dtype=torch.float32, device="cuda")
    st = _lib.stream_of(op_d)
    if rec is None:
        _lib.call("qattn_mxfp4_split_combine", _lib.ptr(op_d), _lib.ptr(ml_d), _lib.ptr(out), _lib.ptr(lse),
                  T * Hq, opart.shape[0], D, st)
    else:
        rec_d = torch.tensor(rec, dtype=torch.int32).cuda()
        _lib.call("qattn_mxfp4_varlen_combine", _lib.ptr(op_d), _lib.ptr(ml_d), _lib.ptr(out), _lib.ptr(lse),
                  _lib.ptr(rec_d), len(rec), T, Hq, Hkv, ml_d.numel() // 2, D, st)
    torch.cuda.synchronize()
    return out.cpu(), lse.cpu()


def test_merge_bit_for_bit(lib):
    """Both merge kernels give the bits of the CPU restatement SR.merge_bits -- the rounding of every
    column included: SR.merge_case has elements in both kinds of column where rounding once and rounding
    twice differ (tests/test_mxfp4_cache_ref.py).  lse: the two kernels agree bit for bit and are within
    test_split_vs_restatement's 1e-4 of M + log2(L).  With one key/value head, one query head and one
    sequence the packed entry's compact layout is the padded one."""
    opart, ml, RO, differs, Rl = SR.merge_case()
    ns, R, D = opart.shape
    O1, l1 = _merge(opart, ml, None, R, 1, 1)
    O2, l2 = _merge(opart, ml, [[0, 0, R, ns, 0, 0, 0, 0]], R, 1, 1)
    for name, O, lse in (("padded", O1, l1), ("packed", O2, l2)):
        ne = O.view(torch.int16) != RO.view(torch.int16)
        print(f"MXFP4-CACHE merge {name}: {int(ne.sum())} of {ne.numel()} elements differ from merge_bits "
              f"({int((ne & differs).sum())} of them among the {int(differs.sum())} the two roundings tell "
              f"apart), lse {(lse - Rl).abs().max().item():.3e}")
    assert torch.equal(O1, RO)
    assert torch.equal(O2, RO)
    assert torch.equal(l1, l2)
    assert (l1 - Rl).abs().max().item() <= 1e-4 and (l2 - Rl).abs().max().item() <= 1e-4

    # the compact layout proper: 4 query heads over 2 key/value heads, two sequences of 37 and 50 tokens
    # with 2 and 3 splits; sequence j's partial rows are [split][kv head][g * n_j + i] from its first one
    Hq, Hkv, G = 4, 2, 2
    seqs, rec, first, base = [], [], 0, 0
    for j, (n, nsp) in enumerate(((37, 2), (50, 3))):
        po, pm = SR.merge_partials(10 + j, nsp, n * Hq)   # in output order: row = token * Hq + head
        tok, head = torch.arange(n * Hq) // Hq, torch.arange(n * Hq) % Hq
        rows = (base + torch.arange(nsp)[:, None] * (Hkv * G * n) + (head // G * (G * n) + head % G * n + tok)[None])
        seqs.append((po, pm, rows, first * Hq, n * Hq))
        rec.append([j, first, n, nsp, base, 0, 0, 0])
        first, base = first + n, base + nsp * Hkv * G * n
    opart, ml = torch.zeros((base, D)), torch.zeros((base, 2))
    for po, pm, rows, _, _ in seqs:
        opart[rows.reshape(-1)], ml[rows.reshape(-1)] = po.reshape(-1, D), pm.reshape(-1, 2)
    O, lse = _merge(opart, ml, rec, first, Hq, Hkv)
    for po, pm, _, r0, nr in seqs:
        RO, _, Rl = SR.merge_bits(po, pm)
        assert torch.equal(O[r0:r0 + nr], RO)
        assert (lse[r0:r0 + nr] - Rl).abs().max().item() <= 1e-4


# ------------------------------------------------------------------ 7. row tails write nothing else
@pytest.mark.parametrize("G,sq_head,causal", [(5, 1, 0), (1, 33, 0), (1, 33, 2), (2, 65, 2), (1, 130, 0)])
def test_row_tails_write_nothing_else(lib, G, sq_head, causal):
    """rows = 5, 33 and 130 per key/value head (two heads): 128 sentinel rows behind bhv * rows in
    out / lse and behind the last split in opart / ml stay untouched by split and by combine, and
    the rows in front are the Python entry's."""
    from quantizedattention_amd.kv_cache_mxfp4 import attention_mxfp4_cached
    q, k, v = MR.randn_qkv((1, 2 * G, 2, sq_head, 192))
    kv = _cache(k, v)
    opart, ml, out, lse, tails, after_split = _c_split(q.cuda(), kv, G, sq_head, causal, 64, 128, SENTINEL)
    for t in after_split + tails:
        assert t.numel() >= 128 and (t == SENTINEL).all()
    assert not (opart == SENTINEL).any() and not (ml == SENTINEL).any()
    O, l2 = attention_mxfp4_cached(q.cuda(), kv, causal=bool(causal), keys_per_split=64)
    assert torch.equal(out, O.reshape(out.shape)) and torch.equal(lse, l2.reshape(-1))
    assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all()


# ------------------------------------------------------------------ 8. masked keys are inert
def test_masked_keys_are_inert(lib):
    """Causal (1, 4, 1, 8, 256), 64 keys per split: row i (position 248 + i) cannot see the keys past
    248 + i.  Row by row, those keys are poisoned -- K rows to +-60000 in fp16 (K's blocks lie inside
    a key row, so the visible keys' operands do not move), V to the largest fp4 code +-6 x scale in
    the quantised operand (V's blocks run along the keys of a tile: poisoning the fp16 values would
    change the scale of the visible keys' block) -- and the row's O and lse stay bit-identical."""
    from quantizedattention_amd.kv_cache_mxfp4 import QuantizedKVFP4, attention_mxfp4_cached
    q, k, v = MR.randn_qkv((1, 4, 1, 8, 256))
    kv = _cache(k, v)
    O, lse = attention_mxfp4_cached(q.cuda(), kv, causal=True, keys_per_split=64)
    order = M.vt_key_order()                    # [2, 32]: key of nibble j of half h
    for i in range(7):
        k2 = k.clone()
        hidden = torch.arange(248 + i + 1, 256)
        k2[:, :, hidden] = HUGE * (1 - 2 * (hidden % 2))[None, None, :, None].half()
        kv2 = _cache(k2, v)
        vt = kv2.vt.cpu().clone()
        for key in hidden.tolist():
            h, j = (order == key - 192).nonzero()[0].tolist()
            byte = vt[0, 3, :, 16 * h + j // 2]
            code = 0x7 if key % 2 else 0xF
            vt[0, 3, :, 16 * h + j // 2] = (byte & (0xF0 if j % 2 == 0 else 0x0F)) | (code << (4 * (j % 2)))
        assert not torch.equal(vt, kv.vt.cpu()) and not torch.equal(kv2.k4, kv.k4)
        vis = torch.arange(0, 248 + i + 1)
        assert torch.equal(kv2.k4[:, :, vis], kv.k4[:, :, vis])
        kv2 = QuantizedKVFP4(kv2.k4, kv2.ks, vt.cuda(), kv2.vs)
        O2, lse2 = attention_mxfp4_cached(q.cuda(), kv2, causal=True, keys_per_split=64)
        assert torch.equal(O2[:, :, i], O[:, :, i]) and torch.equal(lse2[:, i], lse[:, i]), i
        assert torch.isfinite(O2[:, :, :i + 1].float()).all() and torch.isfinite(lse2[:, :i + 1]).all()


# ------------------------------------------------------------------ 9. append
def test_append(lib):
    from quantizedattention_amd import _lib
    from quantizedattention_amd.kv_cache_mxfp4 import QuantizedKVFP4, attention_mxfp4_cached
    q, k, v = (t.cuda() for t in MR.randn_qkv((2, 4, 2, 3, 256)))
    whole = _cache(k, v)
    grown = _cache(k[:, :, :128], v[:, :, :128])
    grown = grown.append(k[:, :, 128:192], v[:, :, 128:192]).append(k[:, :, 192:], v[:, :, 192:])
    assert grown.shape == whole.shape == (2, 2, 256, 128)
    for name in ("k4", "ks", "vt", "vs"):
        assert torch.equal(getattr(grown, name), getattr(whole, name)), name
    back = QuantizedKVFP4.from_bytes(grown.to_bytes().cpu(), device="cuda")   # through the wire format
    for causal in (False, True):
        O1, l1 = attention_mxfp4_cached(q, whole, causal=causal, keys_per_split=128)
        O2, l2 = attention_mxfp4_cached(q, back, causal=causal, keys_per_split=128)
        assert torch.equal(O1, O2) and torch.equal(l1, l2)
    with pytest.raises(_lib.QAttnError):
        whole.append(k[:, :, :32], v[:, :, :32])
    # a smoothed cache keeps its k_mean for the appended keys
    sm = _cache(k[:, :, :128], v[:, :, :128], smooth=True)
    sm2 = sm.append(k[:, :, 128:], v[:, :, 128:])
    assert sm2.k_mean is sm.k_mean and torch.equal(sm2.k4[:, :, :128], sm.k4)
    from quantizedattention_amd.attention_mxfp4 import mxfp4_quantize_rows
    k4b, _ = mxfp4_quantize_rows(k[:, :, 128:].contiguous(), sm.k_mean)
    assert torch.equal(sm2.k4[:, :, 128:].reshape(k4b.shape), k4b)


# ------------------------------------------------------------------ 10. rejections
def test_rejections(lib):
    from quantizedattention_amd import _lib
    from quantizedattention_amd.attention_mxfp4 import _qk_scale, mxfp4_quantize_rows
    from quantizedattention_amd.kv_cache_mxfp4 import attention_mxfp4_cached, quantize_kv_fp4
    q, k, v = (t.cuda() for t in MR.randn_qkv((1, 4, 2, 8, 128)))
    kv = _cache(k, v)
    with pytest.raises(_lib.QAttnError):
        attention_mxfp4_cached(q, kv, keys_per_split=96)
    with pytest.raises(_lib.QAttnError):
        attention_mxfp4_cached(torch.zeros((1, 4, 192, 128), dtype=torch.float16, device="cuda"), kv,
                               causal=True)                                   # Sq > Sk
    with pytest.raises(_lib.QAttnError):
        attention_mxfp4_cached(q[:, :3], kv)                                  # Hq % Hkv
    with pytest.raises(_lib.QAttnError):
        attention_mxfp4_cached(q[..., :64], kv)                               # head_dim 64
    with pytest.raises(_lib.QAttnError):
        quantize_kv_fp4(k[..., :64], v[..., :64])
    with pytest.raises(_lib.QAttnError, match="no CPU fallback"):
        attention_mxfp4_cached(q.cpu(), kv)
    with pytest.raises(_lib.QAttnError, match="no CPU fallback"):
        quantize_kv_fp4(k.cpu(), v.cpu())
    # the C entries: bhv = 2, G = 2, sq_head = 8 -> rows = 16
    q4, qs = mxfp4_quantize_rows(q)
    opart = torch.empty((2, 32, 128), dtype=torch.float32, device="cuda")
    ml = torch.empty((2, 32, 2), dtype=torch.float32, device="cuda")
    out = torch.empty((32, 128), dtype=torch.float16, device="cuda")
    lse = torch.empty((32,), dtype=torch.float32, device="cuda")
    fn = lib.qattn_mxfp4_attn_fwd_split

    def status(bhv=2, rows=16, sq_head=8, sk=128, causal=0, kps=64, hd=128):
        return fn(_lib.ptr(q4), _lib.ptr(qs), *(_lib.ptr(t) for t in kv.kv), _lib.ptr(opart), _lib.ptr(ml),
                  bhv, rows, sq_head, sk, causal, kps, hd, _qk_scale(128), _lib.stream_of(q))
    assert status(kps=96) == 1 and status(kps=32) == 1 and status(kps=0) == 1
    assert status(causal=1) == 1 and status(causal=3) == 1 and status(causal=-1) == 1
    assert status(rows=16, sq_head=16, sk=0, causal=2) == 1          # sk < sq_head (and sk == 0)
    assert status(bhv=1, rows=256, sq_head=256, sk=128, causal=2) == 1   # Sq > Sk
    assert status(rows=4, sq_head=4, sk=0) == 1                      # no keys
    assert status(rows=16, sq_head=5) == 1 and status(sq_head=0) == 1   # rows % sq_head, sq_head < 1
    assert status(sk=96) == 1 and status(hd=64) == 1
    assert status(bhv=0) == 0 and status(rows=0) == 0                # nothing to do: no launch
    assert status() == 0 and status(causal=2) == 0
    cf = lib.qattn_mxfp4_split_combine
    cargs = lambda n, ns, hd: (_lib.ptr(opart), _lib.ptr(ml), _lib.ptr(out), _lib.ptr(lse), n, ns, hd,  # noqa: E731
                               _lib.stream_of(q))
    assert cf(*cargs(32, 2, 64)) == 1 and cf(*cargs(32, 0, 128)) == 1
    assert cf(*cargs(0, 2, 128)) == 0 and cf(*cargs(32, 2, 128)) == 0
    torch.cuda.synchronize()
