"""The int8 and bf16 forwards against the oracle key tile by key tile, on key runs long enough to
switch on the bias fold, the scale tables' shift, the ring's remainder, ragged key splits, the split
fixup, the merge and the causal V-suffix sums (tests/fwd_blocks.py; what the instrument sees and
today's whole-tensor bars do not is shown on the CPU in tests/test_fwd_blocks.py).

V is zero outside one 32-key block per key/value head (a different tile in each, one head dark), q
and k carry a ladder, and O is compared per 32-row query block with ``grad_blocks.block_rel`` -- no
block left out, no floor; a block the oracle has exactly zero (the dark head, the rows of an int8
causal case above the lit tile, a key split without the lit tile) must be exactly zero.  Bars:
``fwd_blocks.INT8_BLOCK_REL`` and ``fwd_blocks.BF16_BLOCK_REL``, both taken from CPU figures; lse under
the elementwise bars of tests/test_gpu_int8.py and tests/test_gpu_bf16.py.  Every maximum is printed
as ``RELL2-BLOCK fwd-<entry>-<case> <value>``; DESIGN.md §4 has the measured ones.

The bf16 reference does not exclude a causal row's masked keys: they keep the weight of the fill
score (bf16_fwd.hip:7), so there every tile reaches every row and no row is zero -- which is what
lets a lit tile past the diagonal hold the V-suffix sums.
"""
import os

import pytest
import torch

import fwd_blocks as FB

from oracle import restate as R

pytestmark = pytest.mark.gpu

FIX_M32 = 0x7fc0e5a5      # int8_attn_fwd.hip: the mark of a split wave handed to the fixup launch


def _check_int8(entry, name, O, lse, ref=None):
    """O [B, Hq, Sq, D] block by block and lse elementwise against the oracle's tuple ``ref``."""
    ref = FB.int8_oracle(name)[3] if ref is None else ref
    O, lse = O.detach().cpu(), lse.detach().cpu()
    assert torch.isfinite(O.float()).all() and torch.isfinite(lse.float()).all(), (entry, name)
    w, where = FB.worst_block(O, ref[0])
    ok, lerr = FB.lse_within_bar(lse.reshape(-1), ref[1])
    print(f"RELL2-BLOCK fwd-{entry}-{name} {w:.5f}")
    print(f"ABS fwd-{entry}-{name} lse {lerr:.2e}")
    FB.assert_dark_zero(name, O, entry)
    assert w <= FB.INT8_BLOCK_REL, (entry, name, "block (b, h, s/32)", where, w)
    assert ok, (entry, name, "lse", lerr)


def _cache(k, v):
    from quantizedattention_amd.kv_cache import quantize_kv
    return quantize_kv(k.cuda(), v.cuda(), smooth=False)


def _cache_is_the_oracles(kv, ref):
    """k_i8, v_i8, sk, sv bit-exact with the oracle's (ref[3] is k_i8 transposed)."""
    D = kv.shape[3]
    assert torch.equal(kv.k_i8.reshape(-1, D).cpu(), ref[3].t()) and torch.equal(kv.v_i8.reshape(-1, D).cpu(), ref[4])
    assert torch.equal(kv.sk.cpu(), ref[6]) and torch.equal(kv.sv.cpu(), ref[7])


# ----------------------------------------------------------------------------------- one pass
@pytest.mark.parametrize("name", ["a", "b", "c", "a1", "b1", "c1"])
def test_int8_q_fused_forward(lib, name):
    """``helion_atten_int8_hl_dot_fwd``: q quantised in the kernel, the fixup inline; non-causal and
    causal from the first key."""
    from quantizedattention_amd.attention_int8 import helion_atten_int8_hl_dot_fwd
    q, k, v, ref = FB.int8_oracle(name)
    out = helion_atten_int8_hl_dot_fwd(q.cuda(), k.cuda(), v.cuda(), causal=bool(FB.CASES[name][1]))
    torch.cuda.synchronize()
    for i in (2, 3, 4, 5, 6, 7):
        assert torch.equal(out[i].cpu(), ref[i]), f"quantisation output {i} differs"
    _check_int8("int8-qf", name, out[0], out[1])


@pytest.mark.parametrize("name,causal", [("a2", True), ("b2", True), ("b", False), ("a", False)])
def test_int8_cached_one_pass(lib, name, causal):
    """``attention_int8_cached``: causal against a cache (qattn_int8_attn_fwd_ex, the last query at the
    last key, the fixup a launch of its own) at D = 128 and 64; non-causal at D = 64, and at D = 128 in
    the decoding layout with one split (a key/value head's query heads as one run of rows)."""
    from quantizedattention_amd.kv_cache import _split_plan, attention_int8_cached
    q, k, v, ref = FB.int8_oracle(name)
    B, Hq, Hkv, Sq, Sk, D = FB.CASES[name][0]
    if not causal and D == 128:
        assert _split_plan(B * Hkv, (Hq // Hkv) * Sq, Sk) >= Sk
    kv = _cache(k, v)
    _cache_is_the_oracles(kv, ref)
    O, lse = attention_int8_cached(q.cuda(), kv, causal=causal)
    torch.cuda.synchronize()
    _check_int8("int8-cached", name, O, lse)


# --------------------------------------------------------------------------------- key splits
def _quantise_q(q):
    from quantizedattention_amd import _lib
    B, H, S, D = q.shape
    N = B * H * S
    qi = torch.empty((N, D), dtype=torch.int8, device=q.device)
    sq = torch.empty((N // 32,), dtype=torch.float16, device=q.device)
    _lib.call("qattn_int8_quant", _lib.ptr(q), _lib.ptr(qi), _lib.ptr(sq), None, None, N, S, D, _lib.stream_of(q))
    return qi, sq


@pytest.mark.parametrize("name", ["s1", "s2"])
def test_int8_key_splits_each_alone_and_merged(lib, name):
    """``qattn_int8_attn_fwd_split`` + ``qattn_int8_split_combine`` with explicit keys per split, the
    query heads of a key/value head as one run of G * Sq rows (192 and 64: idle waves).  Every split
    on its own against the oracle on that key slice -- opart[s] block by block, m_s + log2 l_s under
    the lse bar -- then the merged output against the oracle on all keys.  QATTN_FWD_SKIP_FIXUP (the
    library's diagnostic switch, tests/test_gpu_fixup.py) shows first that the fixup launch has waves
    to redo.  s1: four splits of 256 keys and one of 96; s2: two of 1056 keys (the bias fold inside a
    split) and one of 32."""
    from quantizedattention_amd import _lib
    q, k, v, ref = FB.int8_oracle(name)
    B, Hq, Hkv, Sq, Sk, D = FB.CASES[name][0]
    ks = FB.KEYS_PER_SPLIT[name]
    slices = FB.split_slices(Sk, ks)
    nsplit, bhv, rows = len(slices), B * Hkv, (Hq // Hkv) * Sq
    qc = q.cuda()
    qi, sq = _quantise_q(qc)
    kv = _cache(k, v)
    _cache_is_the_oracles(kv, ref)
    assert torch.equal(qi.cpu(), ref[2]) and torch.equal(sq.cpu(), ref[5])
    st = _lib.stream_of(qc)

    def split(skip_fixup):
        opart = torch.full((nsplit, bhv * rows, D), float("nan"), dtype=torch.float16, device="cuda")
        ml = torch.full((nsplit, bhv * rows, 2), float("nan"), dtype=torch.float32, device="cuda")
        os.environ["QATTN_FWD_SKIP_FIXUP"] = "1" if skip_fixup else "0"
        try:
            _lib.call("qattn_int8_attn_fwd_split", _lib.ptr(qi), _lib.ptr(sq), _lib.ptr(kv.k_i8), _lib.ptr(kv.sk),
                      _lib.ptr(kv.vt()), _lib.ptr(kv.sv), _lib.ptr(opart), _lib.ptr(ml), bhv, rows, Sk, 1, ks, D,
                      _lib.qk_scale(D), st)
            torch.cuda.synchronize()
        finally:
            os.environ.pop("QATTN_FWD_SKIP_FIXUP", None)
        return opart, ml

    # the split fixup is part of what is held: the ladder's peaked rows mark waves, its flat ones do not
    marked = int((split(True)[1][..., 0].contiguous().view(torch.int32) == FIX_M32).sum())
    print(f"{name}: {marked // 32} of {nsplit * bhv * rows // 32} split waves marked for the fixup")
    assert 0 < marked < nsplit * bhv * rows and marked % 32 == 0
    opart, ml = split(False)
    O = torch.empty((B, Hq, Sq, D), dtype=torch.float16, device="cuda")
    lse = torch.empty((B * Hq * Sq,), dtype=torch.float16, device="cuda")
    _lib.call("qattn_int8_split_combine", _lib.ptr(opart), _lib.ptr(ml), _lib.ptr(O), _lib.ptr(lse),
              bhv * rows, nsplit, D, st)
    torch.cuda.synchronize()
    assert torch.isfinite(opart.float()).all() and torch.isfinite(ml).all()
    worst = 0.0
    for s, sl in enumerate(slices):
        r = R.int8_fwd(q, k[:, :, sl], v[:, :, sl])
        w, where = FB.worst_block(opart[s].cpu().view(B, Hq, Sq, D), r[0])
        ok, lerr = FB.lse_within_bar(ml[s, :, 0].cpu() + torch.log2(ml[s, :, 1].cpu()), r[1])
        print(f"RELL2-BLOCK fwd-int8-split{s}-{name} {w:.5f}")
        assert w <= FB.INT8_BLOCK_REL, (name, "split", s, "block (b, h, s/32)", where, w)
        assert ok, (name, "split", s, "m + log2 l", lerr)
        worst = max(worst, w)
    print(f"RELL2-BLOCK fwd-int8-splits-{name} {worst:.5f}")
    _check_int8("int8-merged", name, O, lse)


def test_int8_cached_splits_by_plan(lib):
    """``attention_int8_cached`` non-causal at the smallest cache its plan splits (2048 keys, two
    splits of 1024): lit tiles at both ends of both splits."""
    from quantizedattention_amd.kv_cache import _split_plan, attention_int8_cached
    q, k, v, ref = FB.int8_oracle("p")
    B, Hq, Hkv, Sq, Sk, D = FB.CASES["p"][0]
    assert _split_plan(B * Hkv, (Hq // Hkv) * Sq, Sk) == FB.KEYS_PER_SPLIT["p"] < Sk      # the split path runs
    assert _split_plan(B * Hkv, (Hq // Hkv) * Sq, Sk - 32) >= Sk - 32                     # and no shorter cache does
    kv = _cache(k, v)
    _cache_is_the_oracles(kv, ref)
    O, lse = attention_int8_cached(q.cuda(), kv, causal=False)
    torch.cuda.synchronize()
    _check_int8("int8-cached-split", "p", O, lse)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("nsplit", [1, 2, 5, 33])
def test_split_combine_is_the_merge(lib, nsplit, D):
    """``qattn_int8_split_combine`` on synthetic split states against ``fwd_blocks.split_merge_ref``:
    O within one fp16 ulp, lse within two.  The fp32 sum of nsplit terms and one reciprocal stay far
    below half an fp16 ulp, so one ulp covers the final rounding; the second on lse is for v_log_f32
    and the inner f16(log2 L).  Two places where that reasoning needs its premise spelled out, both
    met by these inputs (m_s over +-30, l_s in [1, 1000], randn Ô_s: 128000 entries a case):

      * the fp32 sum rounds at the size of its terms, not of its result: where terms of size 1 cancel
        to a result in fp16's subnormal range (spacing 2^-24) that is no longer "far below".  So O is
        allowed one fp16 ulp plus (nsplit + 2) 2^-23 sum_s |w_s Ô_s| / L, the bound on the fp32 sum,
        exp2 and reciprocal; on a result of the terms' size that adds less than 1 % of an ulp;
      * the inner f16(log2 L) rounds at the size of log2 L (up to 15), not of lse = M + log2 L, which
        can cancel to near 0.  So the second ulp of lse is an fp16 ulp of the larger of |lse| and
        |log2 L| (the same two ulp wherever |lse| >= |log2 L|), plus the fp32 sum's 2^-22 (|M| + |log2 L|).

    37 and 1000 rows are no multiple of a 256-thread block's rows."""
    from quantizedattention_amd import _lib
    for rows in (37, 1000):
        opart, ml = FB.merge_inputs(nsplit, rows, D, seed=600 + nsplit + D + rows)
        Or, lr = FB.split_merge_ref(opart, ml)
        terms, log2L, M = FB.merge_rounding(opart, ml)
        oc, mc = opart.cuda(), ml.cuda()
        O = torch.full((rows, D), float("nan"), dtype=torch.float16, device="cuda")
        lse = torch.full((rows,), float("nan"), dtype=torch.float16, device="cuda")
        _lib.call("qattn_int8_split_combine", _lib.ptr(oc), _lib.ptr(mc), _lib.ptr(O), _lib.ptr(lse), rows,
                  nsplit, D, _lib.stream_of(oc))
        torch.cuda.synchronize()
        eo, el = (O.cpu().double() - Or).abs(), (lse.cpu().double() - lr).abs()
        bo = FB.fp16_ulp(Or) + (nsplit + 2) * 2.0 ** -23 * terms
        bl = FB.fp16_ulp(lr) + torch.maximum(FB.fp16_ulp(lr), FB.fp16_ulp(log2L)) + 2.0 ** -22 * (M.abs() + log2L.abs())
        print(f"ULP fwd-int8-combine-{nsplit}x{rows}x{D} O {(eo / FB.fp16_ulp(Or)).max().item():.3f} "
              f"lse {(el / FB.fp16_ulp(lr)).max().item():.3f}; of the bounds: O {(eo / bo).max().item():.3f} "
              f"lse {(el / bl).max().item():.3f}")
        assert (eo <= bo).all(), (nsplit, rows, D, (eo / bo).max().item())
        assert (el <= bl).all(), (nsplit, rows, D, (el / bl).max().item())
        if nsplit > 2:   # some weights vanish against the row's largest (below fp32's 2^-24 of it)
            assert (torch.exp2(ml[..., 0] - ml[..., 0].amax(0)) < 2.0 ** -24).any()


# ------------------------------------------------------------------------------ a smoothed cache
def test_int8_smoothed_cache(lib):
    """``quantize_kv(smooth=True)`` on the first 544 keys, the other 576 appended against the stored
    mean: the lit instrument against the oracle on the keys minus that mean (softmax does not see the
    shift; the quantised keys do)."""
    from quantizedattention_amd.kv_cache import attention_int8_cached, quantize_kv
    q, k, v = FB.case_inputs("sm")
    n = FB.SMOOTH_HEAD
    kv = quantize_kv(k[:, :, :n].cuda(), v[:, :, :n].cuda(), smooth=True)
    kv = kv.append(k[:, :, n:].cuda(), v[:, :, n:].cuda())
    assert kv.k_mean is not None and kv.shape[2] == k.shape[2]
    km = kv.k_mean.cpu()
    assert (km.float() - R._f(k[:, :, :n]).mean(dim=-2, keepdim=True)).abs().max().item() <= 2e-3
    ref = R.int8_fwd(q, FB.smooth_shift(k, km), v)
    _cache_is_the_oracles(kv, ref)
    O, lse = attention_int8_cached(q.cuda(), kv, causal=False)
    torch.cuda.synchronize()
    _check_int8("int8-cached-smooth", "sm", O, lse, ref)


# ----------------------------------------------------------------------------------------- bf16
def _check_bf16(entry, name, O, lse):
    Or, lr = FB.bf16_oracle(name)[3:]
    O, lse = O.detach().cpu().view_as(Or), lse.detach().cpu().view_as(lr)
    assert torch.isfinite(O).all() and torch.isfinite(lse).all(), (entry, name)
    w, where = FB.worst_block(O, Or)
    lerr = (lse - lr).abs().max().item()
    print(f"RELL2-BLOCK fwd-{entry}-{name} {w:.5f}")
    print(f"ABS fwd-{entry}-{name} lse {lerr:.2e}")
    FB.assert_dark_zero(name, O, entry)
    assert w <= FB.BF16_BLOCK_REL, (entry, name, "block (b, h, s/32)", where, w)
    assert lerr <= FB.BF16_LSE_ABS, (entry, name, lerr)


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_bf16_tile_loop(lib, name):
    from quantizedattention_amd.attention_bf16 import helion_atten_bf16_fwd_training
    q, k, v = FB.bf16_oracle(name)[:3]
    O, lse = helion_atten_bf16_fwd_training(q.cuda(), k.cuda(), v.cuda(), False)
    torch.cuda.synchronize()
    _check_bf16("bf16", name, O, lse)


@pytest.mark.parametrize("name", ["a1f", "b1f", "c1f"])
def test_bf16_causal_both_paths(lib, name):
    """Causal: the masked tile loop (qattn_bf16_fwd_ex) and the V-suffix path (qattn_bf16_fwd_ws_ex with
    its workspace).  The lit diagonal tile of a middle query block is half tile loop, half suffix for
    its own wave and all suffix for the waves above; tiles 31 to 34 are suffix for every wave."""
    from quantizedattention_amd import _lib
    q, k, v = (t.cuda() for t in FB.bf16_oracle(name)[:3])
    B, Hq, Hkv, Sq, Sk, D = FB.CASES[name][0]
    for entry, fn in (("bf16-causal-loop", "qattn_bf16_fwd_ex"), ("bf16-causal-suffix", "qattn_bf16_fwd_ws_ex")):
        O = torch.full((B, Hq, Sq, D), float("nan"), device="cuda")
        lse = torch.full((B * Hq, Sq), float("nan"), device="cuda")
        args = (_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(O), _lib.ptr(lse), B * Hq, Sq, Sk, Hq // Hkv, 1, D,
                _lib.qk_scale(D))
        if fn.endswith("ws_ex"):
            ws = torch.full((lib.qattn_bf16_fwd_ws_bytes(B * Hkv, Sk, D) // 4,), float("nan"), device="cuda")
            args += (_lib.ptr(ws),)
        _lib.call(fn, *args, _lib.stream_of(q))
        torch.cuda.synchronize()
        _check_bf16(entry, name, O, lse)
