"""The MX-FP4 forwards (mxfp4_attn_fwd, mxfp4_attn_fwd_kv, attention_mxfp4_cached) on inputs whose
integer running max keeps moving, on full grids and on long key runs, against the restatements
tests/mxfp4_masked_ref.py / tests/mxfp4_split_ref.py through tests/mxfp4_cases.py.

N(0, 1) inputs raise m in a row's first visible tile and never again, so on them the rescale branch
of mx_tile (csrc/mxfp4_attn.hip) multiplies by 2^0 or not at all.  The families ramp, spikes and fall
of mxfp4_cases make rows raise late, at tiles of their own (partially raising waves), inside causal
diagonal tiles and inside key splits, and give the splits of a row very different m_s.
tests/test_mxfp4_cases_ref.py shows on the CPU that they do, for every case used here.

Bars (mxfp4_cases.compare): quantised operands bit-exact; on the rows the classifier does not call
fragile O max-abs <= 2e-2, relL2 <= 2e-3 (from 64 rows on), lse <= 1e-4 * max(1, max|lse|); on every
row O, lse finite and O inside the hull of the visible dequantised V; at most 2 % fragile rows.
Measured values are printed as "MXFP4-FUZZ ..." and tabulated in DESIGN.md section 4.  The placement
tests are bit-identity: no tolerance.
"""
import pytest
import torch

import mxfp4_cases as C
import mxfp4_masked_ref as MR
import mxfp4_split_ref as SR

pytestmark = pytest.mark.gpu


def _ids(cases):
    return [f"{c[1]}-{'x'.join(map(str, c[0]))}-c{c[3]}" for c in cases]


def _ops_equal(ops, rops):
    for a, b in zip(ops, rops):
        assert torch.equal(a.cpu().reshape(b.shape), b)


def _cache(k, v, smooth=False):
    from quantizedattention_amd.kv_cache_mxfp4 import quantize_kv_fp4
    return quantize_kv_fp4(k.cuda(), v.cuda(), smooth=smooth)


def _gpu_kmean(k):
    """The fp16 token mean the smoothing forward subtracts (qattn_kmean), back on the CPU."""
    from quantizedattention_amd import _lib
    B, Hkv, Sk, D = k.shape
    kc = k.cuda().contiguous()
    km = torch.empty((B, Hkv, 1, D), dtype=torch.float16, device="cuda")
    _lib.call("qattn_kmean", _lib.ptr(kc), _lib.ptr(km), B * Hkv, Sk, D, _lib.stream_of(kc))
    torch.cuda.synchronize()
    return km.cpu()


def _smoothed(k, km):
    return (k.float() - km.float()).half()


def _cached_vs_reference(q, kv, ref, causal, kps, name):
    from quantizedattention_amd.attention_mxfp4 import mxfp4_quantize_rows
    from quantizedattention_amd.kv_cache_mxfp4 import attention_mxfp4_cached
    _ops_equal(mxfp4_quantize_rows(q.cuda()) + kv.kv, ref["ops"])
    O, lse = attention_mxfp4_cached(q.cuda(), kv, causal=bool(causal), keys_per_split=kps)
    torch.cuda.synchronize()
    assert O.shape == q.shape and lse.shape == (q.shape[0] * q.shape[1], q.shape[2])
    C.compare(O, lse, ref["O"], ref["lse"], ref["fragile"], ref["vminmax"], name)
    return O, lse


def _split_m(q, kv, G, sq_head, causal, kps):
    """m_s [nsplit, bhv * rows] of qattn_mxfp4_attn_fwd_split, read through the C entry as
    tests/test_gpu_mxfp4_cache.py::_c_split does."""
    from quantizedattention_amd import _lib
    from quantizedattention_amd.attention_mxfp4 import _qk_scale, mxfp4_quantize_rows
    B, Hkv, Sk, D = kv.shape
    bhv, rows = B * Hkv, G * sq_head
    R, ns = bhv * rows, -(-Sk // kps)
    qc = q.cuda()
    q4, qs = mxfp4_quantize_rows(qc)
    opart = torch.empty((ns, R, D), dtype=torch.float32, device="cuda")
    ml = torch.empty((ns, R, 2), dtype=torch.float32, device="cuda")
    _lib.call("qattn_mxfp4_attn_fwd_split", _lib.ptr(q4), _lib.ptr(qs), *(_lib.ptr(t) for t in kv.kv),
              _lib.ptr(opart), _lib.ptr(ml), bhv, rows, sq_head, Sk, 2 if causal else 0, kps, D, _qk_scale(D),
              _lib.stream_of(qc))
    torch.cuda.synchronize()
    return ml[..., 0].cpu()


def _assert_m_of_the_splits(q, k, v, kv, shape, causal, kps, spread=True):
    """The kernel's m_s are the split restatement's, exactly: S is exact on the matrix core and m an
    integer, so the raise test ``mx > m + 8`` decides the same on both sides (a kernel that raised at
    another slack would still return the same O and lse, by design, but other m_s).  With ``spread``
    some row's finite m_s differ by more than 8 between splits: the merge weighs far from 1."""
    B, H, Hkv, Sq, Sk = shape
    m = _split_m(q, kv, H // Hkv, Sq, causal, kps)
    mr = SR.split_partials(q, k, v, causal, kps)[0]
    assert torch.equal(m.double(), mr.reshape(m.shape))
    if not spread:
        return
    fin = torch.isfinite(m)
    d = m.masked_fill(~fin, float("-inf")).amax(0) - m.masked_fill(~fin, float("inf")).amin(0)
    assert d.max().item() > 8, d.max().item()


# ------------------------------------------------------------------------------ a. structured parity
@pytest.mark.parametrize("case", C.ONEPASS_STRUCT, ids=_ids(C.ONEPASS_STRUCT))
def test_structured_one_pass(lib, case):
    from quantizedattention_amd.attention_mxfp4 import mxfp4_attn_fwd, mxfp4_attn_fwd_kv
    shape, kind, seed, causal = case
    q, k, v = C.case_inputs(*case)
    ref = C.case_reference(*case)
    O, lse, ops = mxfp4_attn_fwd(q.cuda(), k.cuda(), v.cuda(), smooth_k=False, causal=causal)
    torch.cuda.synchronize()
    _ops_equal(ops, ref["ops"])
    assert O.shape == q.shape and lse.shape == (shape[0] * shape[1], shape[3])
    C.compare(O, lse, ref["O"], ref["lse"], ref["fragile"], ref["vminmax"], f"one-pass {case}")
    O2, lse2 = mxfp4_attn_fwd_kv(q.cuda(), ops[2:], causal=causal)
    assert torch.equal(O2, O) and torch.equal(lse2, lse)


@pytest.mark.parametrize("case,kpss", C.CACHED_STRUCT, ids=_ids([c for c, _ in C.CACHED_STRUCT]))
def test_structured_cached(lib, case, kpss):
    from quantizedattention_amd.kv_cache_mxfp4 import attention_mxfp4_cached
    shape, kind, seed, causal = case
    q, k, v = C.case_inputs(*case)
    ref = C.case_reference(*case)
    kv = _cache(k, v)
    for kps in kpss:
        O, lse = _cached_vs_reference(q, kv, ref, causal, kps, f"cached {case} kps={kps}")
        if kps < shape[4]:
            _assert_m_of_the_splits(q, k, v, kv, shape, causal, kps, spread=kind == "ramp")
        if shape[3] == 1:     # one query at the end of the cache sees every key: the mask changes no bit
            Oc, lc = attention_mxfp4_cached(q.cuda(), kv, causal=not causal, keys_per_split=kps)
            assert torch.equal(Oc, O) and torch.equal(lc, lse)


# ------------------------------------------------------------------------------ b. seeded fuzz
@pytest.mark.parametrize("i", range(C.N_FUZZ))
def test_fuzz(lib, i):
    from quantizedattention_amd.attention_mxfp4 import mxfp4_attn_fwd
    f = C.fuzz_case(i)
    shape, causal, smooth = f["shape"], f["causal"], f["smooth"]
    q, k, v = C.case_inputs(shape, f["kind"], f["seed"], causal)
    name = f"fuzz{i} {shape} {f['kind']} causal={causal} smooth={smooth}" + (f" kps={f['kps']}" if f["cached"] else "")
    if f["cached"]:
        kv = _cache(k, v, smooth=smooth)
        assert (kv.k_mean is not None) == smooth
        ref = C.reference(q, _smoothed(k, kv.k_mean.cpu()) if smooth else k, v, causal)
        _cached_vs_reference(q, kv, ref, causal, f["kps"], name)
    else:
        ref = C.reference(q, _smoothed(k, _gpu_kmean(k)) if smooth else k, v, causal)
        O, lse, ops = mxfp4_attn_fwd(q.cuda(), k.cuda(), v.cuda(), smooth_k=smooth, causal=causal)
        torch.cuda.synchronize()
        _ops_equal(ops, ref["ops"])
        C.compare(O, lse, ref["O"], ref["lse"], ref["fragile"], ref["vminmax"], name)


# ------------------------------------------------------------------------------ c. placement is invisible
@pytest.mark.parametrize("case", C.PLACEMENT_ONEPASS, ids=_ids(C.PLACEMENT_ONEPASS))
def test_one_pass_head_alone_is_bit_identical(lib, case):
    """BH = 16 takes the (nbh & 7) == 0 branch of xcd_remap / xcd_remap_lpt with nq = 3 (the last
    workgroup of a head has two idle waves), BH = 9 the other branch with 27 workgroups.  A row's
    result does not depend on the workgroup that runs it: every head equals the run of that head alone."""
    from quantizedattention_amd.attention_mxfp4 import mxfp4_attn_fwd
    (B, H, Hkv, Sq, Sk), kind, seed, causal = case
    G = H // Hkv
    q, k, v = (t.cuda() for t in C.case_inputs(*case))
    O, lse, _ = mxfp4_attn_fwd(q, k, v, smooth_k=False, causal=causal)
    lse = lse.view(B, H, Sq)
    assert torch.isfinite(O.float()).all() and torch.isfinite(lse).all()
    for b in range(B):
        for h in range(H):
            kh = h // G
            O1, l1, _ = mxfp4_attn_fwd(q[b:b + 1, h:h + 1], k[b:b + 1, kh:kh + 1], v[b:b + 1, kh:kh + 1],
                                       smooth_k=False, causal=causal)
            assert torch.equal(O1[0, 0], O[b, h]) and torch.equal(l1[0], lse[b, h]), (b, h)


@pytest.mark.parametrize("case", C.PLACEMENT_CACHED, ids=_ids(C.PLACEMENT_CACHED))
def test_cached_head_alone_is_bit_identical(lib, case):
    """bhv = 8 takes the (nbh & 7) == 0 branch of xcd_remap in the key-split kernel; rows = G * Sq = 200
    are two row blocks, the second with a partial wave.  Each key/value head's group equals the run on
    that head alone, and each query head the run with G = 1 (other wave neighbours, other diagonal
    flags) on that head alone."""
    from quantizedattention_amd.kv_cache_mxfp4 import attention_mxfp4_cached
    (B, H, Hkv, Sq, Sk), kind, seed, causal = case
    G = H // Hkv
    q, k, v = (t.cuda() for t in C.case_inputs(*case))
    O, lse = attention_mxfp4_cached(q, _cache(k, v), causal=bool(causal), keys_per_split=128)
    lse = lse.view(B, H, Sq)
    assert torch.isfinite(O.float()).all() and torch.isfinite(lse).all()
    for b in range(B):
        for kh in range(Hkv):
            kv1 = _cache(k[b:b + 1, kh:kh + 1], v[b:b + 1, kh:kh + 1])
            hs = slice(kh * G, kh * G + G)
            Og, lg = attention_mxfp4_cached(q[b:b + 1, hs], kv1, causal=bool(causal), keys_per_split=128)
            assert torch.equal(Og[0], O[b, hs]) and torch.equal(lg, lse[b, hs]), (b, kh)
            for h in range(kh * G, kh * G + G):
                O1, l1 = attention_mxfp4_cached(q[b:b + 1, h:h + 1], kv1, causal=bool(causal),
                                                keys_per_split=128)
                assert torch.equal(O1[0, 0], O[b, h]) and torch.equal(l1[0], lse[b, h]), (b, h)


# ------------------------------------------------------------------------------ d. long key runs
@pytest.mark.parametrize("case", C.LONG_ONEPASS, ids=_ids(C.LONG_ONEPASS))
def test_long_one_pass(lib, case):
    """128 key tiles: the 4-slot ring wraps 32 times while m keeps climbing."""
    from quantizedattention_amd.attention_mxfp4 import mxfp4_attn_fwd
    shape, kind, seed, causal = case
    q, k, v = C.case_inputs(*case)
    ref = C.case_reference(*case)
    O, lse, ops = mxfp4_attn_fwd(q.cuda(), k.cuda(), v.cuda(), smooth_k=False, causal=causal)
    torch.cuda.synchronize()
    _ops_equal(ops, ref["ops"])
    C.compare(O, lse, ref["O"], ref["lse"], ref["fragile"], ref["vminmax"], f"long one-pass {case}")


@pytest.mark.parametrize("case,kpss", C.LONG_CACHED, ids=_ids([c for c, _ in C.LONG_CACHED]))
def test_long_cached(lib, case, kpss):
    """8192 keys in 128 splits of one tile, in 8 of 16 tiles, and as _split_plan_fp4 cuts them."""
    from quantizedattention_amd.kv_cache_mxfp4 import _split_plan_fp4
    shape, kind, seed, causal = case
    B, H, Hkv, Sq, Sk = shape
    q, k, v = C.case_inputs(*case)
    ref = C.case_reference(*case)
    kv = _cache(k, v)
    plan = _split_plan_fp4(B * Hkv, (H // Hkv) * Sq, Sk)
    assert 64 <= plan < Sk and None in kpss          # the plan does split this shape
    for kps in kpss:
        _cached_vs_reference(q, kv, ref, causal, kps, f"long cached {case} kps={kps}")
        _assert_m_of_the_splits(q, k, v, kv, shape, causal, plan if kps is None else kps)


# ------------------------------------------------------------------------------ e. tail merge by lse
@pytest.mark.parametrize("smooth", [False, True])
def test_tail_merge_by_lse(lib, smooth):
    """kv_cache_mxfp4's advice to callers: 256 tokens in the cache, a tail of 17 in fp16, attended
    exactly and merged by the two base-2 lse.  The same merge runs on the restatement's (O, lse), and
    the kernel's merged result meets the compare bars against it.  With a smoothed cache the lse is
    that of the scores q . (k - k_mean), so the tail keys take the same k_mean off first; merged that
    way the result stays as close to exact attention over all 273 keys as the restatement's does."""
    from quantizedattention_amd.attention_mxfp4 import mxfp4_quantize_rows
    from quantizedattention_amd.kv_cache_mxfp4 import attention_mxfp4_cached
    (B, H, Hkv, Sq, _), kind, seed, causal = C.TAIL_CASE
    q, k, v = C.case_inputs(*C.TAIL_CASE)
    n0, n1 = C.TAIL_CACHE, C.TAIL_CACHE + C.TAIL_LEN
    kc, vc, kt, vt = k[:, :, :n0], v[:, :, :n0], k[:, :, n0:n1].float(), v[:, :, n0:n1]
    kv = _cache(kc, vc, smooth=smooth)
    if smooth:
        km = kv.k_mean.cpu()
        kc, kt = _smoothed(kc, km), kt - km.float()
    ref = C.reference(q, kc, vc, 0)
    _ops_equal(mxfp4_quantize_rows(q.cuda()) + kv.kv, ref["ops"])
    O, lse = attention_mxfp4_cached(q.cuda(), kv, causal=False)
    torch.cuda.synchronize()
    C.compare(O, lse, ref["O"], ref["lse"], ref["fragile"], ref["vminmax"], f"tail: cache alone smooth={smooth}")
    Ot, lt = C.exact_tail(q, kt, vt)
    shape2 = (B * H, Sq)
    Om, lm = C.merge_lse2(O.cpu().view(B, H, Sq, 128), lse.cpu().view(B, H, Sq), Ot, lt.view(B, H, Sq))
    ROm, Rlm = C.merge_lse2(ref["O"], ref["lse"].view(B, H, Sq), Ot, lt.view(B, H, Sq))
    G = H // Hkv
    tlo = vt.double().amin(2, keepdim=True).repeat_interleave(G, 1).reshape(B * H, 1, 128)
    thi = vt.double().amax(2, keepdim=True).repeat_interleave(G, 1).reshape(B * H, 1, 128)
    lo, hi = ref["vminmax"]
    C.compare(Om, lm.reshape(shape2), ROm, Rlm.reshape(shape2), ref["fragile"],
              (torch.minimum(lo, tlo), torch.maximum(hi, thi)), f"tail: merged smooth={smooth}")
    # the tail weighs in: without it the result is another one
    assert (Om - O.cpu().float()).abs().max().item() > 0.1
    exact = MR.exact_masked_attention(q, k[:, :, :n1], v[:, :, :n1], 0)
    cos, rcos = MR.cosine(Om, exact), MR.cosine(ROm, exact)
    print(f"MXFP4-FUZZ tail smooth={smooth}: merged vs exact attention over {n1} keys: cosine {cos:.4f} "
          f"(restatement {rcos:.4f})")
    assert cos >= rcos - 1e-3, (cos, rcos)
    # the project's end-to-end bar; on the CPU the restatement merges to 0.966 (plain) and 0.981
    # (smoothed), and to 0.860 when the smoothed cache meets tail keys that kept their mean
    assert rcos >= 0.95, rcos
