"""Addressing past 2^31 elements, 2^32 bytes and 4 GiB of workspace: where the 64-bit head and row
offsets of every kernel are actually exercised.

A head or row offset computed in ``int``, or a byte offset in ``unsigned``, wraps at these sizes and
reads another head's rows: a silent wrong answer that no smaller test can see.  The instrument is the
head-alone one of tests/test_gpu_head_alone.py: the full launch on a big tensor, then one key/value
head with its query heads alone, on copies, compared with ``torch.equal`` on the bit patterns (no
tolerance).  Not every head runs alone: key/value head 0, the boundary head (``boundary_heads`` of
tests/head_alone.py computes it from the shape: the head that holds element 2^31 - 1, so it straddles
2^31 or ends exactly there) and the last head, which lies wholly past 2^31.  The last head's run alone
is also held to the CPU oracle at the bar of the path's own parity test (imported, not restated), so a
launch that were wrong in both runs alike would still show.  No big tensor is copied to the host.
tests/test_head_alone_helper.py shows on the CPU that the instrument names a truncated offset.

Shapes (B = 1, D = 128), the smallest at which a 32-bit index can wrap while the work stays small:

  *query side* (Hq, Hkv, Sq, Sk) = (35000, 17500, 480, 128): q, O, dO, dq and the int8 / bf16 images of
      q hold 35000 * 480 * 128 = 2.15e9 > 2^31 elements (> 2^32 bytes in fp16), 16 800 000 > 2^24 rows.
      G = 2: key/value head 17476 (query heads 34952, 34953) straddles row 2^24, head 17499 lies past
      it.  Sq = 3 * 128 + 96 leaves a ragged last workgroup and, with G > 1, takes the non-causal int8
      forward's "virtual head" branch (2 * 480 rows per key/value head).  The keys are tiny: ~1 TFLOP.
      35000 heads are a multiple of 8, 17500 are not: both branches of the workgroup remaps.  Many short
      heads rather than few long ones: the count that crosses 2^31 is what matters, and the last head's
      run alone is 960 rows, the scale at which the parity bars it is held to were set (they bound a
      maximum over at most 2048 rows; DESIGN.md section 4 has the measured growth of that maximum with
      the row count, on a head alone, where no big address is involved).  Streamed query tiles per
      key/value head stay far below the int8 record kernel's limit (tests/test_plan.py).
  *key side* (4104, 4104, 64, 4096): k, v, dk, dv and their images pass 2^31 elements; head 4096 starts
      exactly at element 2^31, so the boundary head is 4095, and the last, 4103, lies past it.
  *2^32 elements* (int8 forward only) (70000, 35000, 480, 128): q_i8 and the scale tables have 1-byte
      and 2-byte elements, so their byte offsets wrap only at 2^32 elements: rows * D = 4.30e9.
      Key/value head 34952 straddles element 2^32 (and 17476 still straddles 2^31).
  *workspace* Sq = Sk = 8192, G = 1: the int8 dS records take 64 MiB + 256 KiB per head, the bf16
      records 128 MiB; 65 resp. 33 heads are the fewest whose records pass 4 GiB by a whole head.
  *cache bytes* PreallocatedKVFP4 with B = 66, Hkv = 8, capacity 131072: k4 and vt take 4.43e9 > 2^32
      bytes each; sequence 64 starts exactly at byte 2^32 and sequence 65 lies past it.

The JVP's fp32 (X3) kernel runs on the query side only: its key-side offset ``kv0`` is the same
expression as the bf16 mode's (csrc/jvp_fwd.hip), and a key-side X3 case would need about 70 GB.

Every test computes the device memory it needs from its shapes and skips, with both figures in the
reason, only when ``torch.cuda.mem_get_info`` shows less free; on an idle MI355X none skips.  Tensors
are freed as the tests go and the module ends with ``torch.cuda.empty_cache()``.  Each test prints
``BIGINDEX <test> <seconds> s peak <GiB> GiB``.  Forwards run before backwards, small footprints first.
"""
import time

import pytest
import torch

from conftest import INT8_BWD_REL
from head_alone import _Diff, _gen, _randn, boundary_heads
from test_gpu_bf16 import BWD_REL as BF16_BWD_REL
from test_gpu_bf16 import FWD_BAR as BF16_FWD_BAR
from test_gpu_head_alone import FWD_NAMES, FWD_SIDE, _int8_bwd_args, _int8_fwd, _int8_fwd_parts
from test_gpu_int8 import O_BAR as INT8_O_BAR
from test_gpu_int8 import lse_within_bar
from test_gpu_jvp import BF16_BAR as JVP_BF16_BAR
from test_gpu_jvp import FP32_BAR as JVP_FP32_BAR
from test_gpu_mxfp4 import LSE_BAR as MX_LSE_BAR
from test_gpu_mxfp4 import O_BAR as MX_O_BAR
from test_gpu_mxfp4 import O_REL as MX_O_REL

pytestmark = pytest.mark.gpu

D = 128
GiB = 2 ** 30
# (Hq, Hkv, Sq, Sk)
SIDES = {"q-side": (35000, 17500, 480, 128), "k-side": (4104, 4104, 64, 4096)}
CAUSAL = pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
SIDE = pytest.mark.parametrize("side", list(SIDES))


@pytest.fixture(scope="module", autouse=True)
def _release_the_cache():
    yield
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def _time_and_peak(request):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    print(f"\nBIGINDEX {request.node.name} {time.perf_counter() - t0:.2f} s peak "
          f"{torch.cuda.max_memory_allocated() / GiB:.2f} GiB")
    torch.cuda.empty_cache()


def _need(nbytes):
    """Skip when the device has less free than the test's tensors take (plus a tenth for the
    generator's slices and the heads run alone)."""
    need = int(nbytes * 1.1) + GiB
    free, _total = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip(f"needs {need / GiB:.1f} GiB of device memory, {free / GiB:.1f} GiB are free")


def _big_randn(shape, g, dtype, scale=1.0):
    """``_randn`` of a [1, H, S, D] tensor in slices of at most 2^28 elements (the fp32 draw of a
    whole one would double the footprint)."""
    out = torch.empty(shape, dtype=dtype, device="cuda")
    step = max(1, (1 << 28) // out[0, 0].numel())
    for h in range(0, shape[1], step):
        n = min(step, shape[1] - h)
        out[:, h:h + n] = _randn((1, n) + tuple(shape[2:]), g, dtype, scale)
    return out


def _heads_alone(side, threshold=2 ** 31, shape=None):
    """(Hq, Hkv, Sq, Sk, G, the key/value heads to run alone), the heads from the big tensor's shape."""
    Hq, Hkv, Sq, Sk = shape or SIDES[side]
    G = Hq // Hkv
    assert Hq == G * Hkv and Sq % 32 == 0 and Sk % 64 == 0
    per_head = G * Sq * D if side == "q-side" else Sk * D    # elements of one key/value head's share
    heads = boundary_heads(Hkv, per_head, threshold)
    if side == "q-side":     # the boundary head straddles the threshold, the ragged last workgroup stays
        assert heads[1] * per_head < threshold < (heads[1] + 1) * per_head
        assert Sq % 128 != 0 and G > 1
    else:                    # a head starts exactly at the threshold: the boundary head ends there
        assert (heads[1] + 1) * per_head == threshold
    return Hq, Hkv, Sq, Sk, G, heads


def _elems(side, what, shape=None):
    Hq, Hkv, Sq, Sk = shape or SIDES[side]
    return Hq * Sq * D if what == "q" else Hkv * Sk * D


def _cpu(*xs):
    return [None if x is None else x.cpu() for x in xs]


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


def test_shapes_cross_what_they_claim():
    """The thresholds of the module docstring, from the shapes."""
    assert _heads_alone("q-side")[5] == (0, 17476, 17499) and _heads_alone("k-side")[5] == (0, 4095, 4103)
    assert _elems("q-side", "q") > 2 ** 31 and _elems("q-side", "q") // D > 2 ** 24
    assert _elems("k-side", "k") > 2 ** 31 and 4096 * 4096 * D == 2 ** 31
    assert _heads_alone("q-side", 2 ** 32, X32)[5] == (0, 34952, 34999) and X32[0] * X32[2] * D > 2 ** 32
    assert WS_INT8_HEADS * WS_INT8_HEAD_BYTES >= 2 ** 32 + WS_INT8_HEAD_BYTES > (WS_INT8_HEADS - 1) * WS_INT8_HEAD_BYTES
    assert WS_BF16_HEADS * WS_BF16_HEAD_BYTES >= 2 ** 32 + WS_BF16_HEAD_BYTES > (WS_BF16_HEADS - 1) * WS_BF16_HEAD_BYTES
    B, Hkv, cap = CACHE
    assert B * Hkv * cap * 64 > 2 ** 32 and 64 * Hkv * cap * 64 == 2 ** 32 and B - 1 > 64


X32 = (70000, 35000, 480, 128)
WS_S = 8192
WS_INT8_HEAD_BYTES, WS_BF16_HEAD_BYTES = (WS_S // 32) ** 2 * (1024 + 4), (WS_S // 32) ** 2 * 2048
WS_INT8_HEADS, WS_BF16_HEADS = 65, 33
CACHE = (66, 8, 131072)


# ------------------------------------------------------------------------- split into bf16 images
def test_split_bf16_past_2_31():
    """``qattn_split_bf16`` at n = 2^31 + 4096 fp32 elements (x 8 GiB; hi, lo 4 GiB each: their byte
    offsets pass 2^32 too) against ``x.bfloat16()`` and ``(x - hi).bfloat16()`` computed by torch on
    the GPU, slice by slice over the whole range."""
    from quantizedattention_amd import _lib
    n = 2 ** 31 + 4096
    _need(n * (4 + 2 + 2))
    g = _gen("split-bf16")
    x = torch.empty((n,), dtype=torch.float32, device="cuda")
    step = 1 << 27
    for i in range(0, n, step):
        x[i:i + step] = _randn((min(step, n - i),), g, torch.float32, 3.0)
    hi, lo = torch.empty((n,), dtype=torch.bfloat16, device="cuda"), torch.empty((n,), dtype=torch.bfloat16, device="cuda")
    _lib.call("qattn_split_bf16", _lib.ptr(x), _lib.ptr(hi), _lib.ptr(lo), n, _lib.stream_of(x))
    bad = []
    for i in range(0, n, step):
        xs = x[i:i + step]
        h = xs.bfloat16()
        if not torch.equal(hi[i:i + step], h):
            bad.append(("hi", i))
        if not torch.equal(lo[i:i + step], (xs - h.float()).bfloat16()):
            bad.append(("lo", i))
    assert not bad, bad


# ------------------------------------------------------------------------------------ MX-FP4
@pytest.mark.parametrize("side,causal", [("q-side", 0), ("q-side", 1), ("k-side", 0), ("k-side", 1), ("k-side", 2)])
def test_mxfp4_forward_and_quantisers(lib, side, causal):
    """``mxfp4_attn_fwd``: O, lse and the six operands, so ``mxfp4_quantize_rows`` runs on q (query
    side) and on k (key side) and ``mxfp4_quantize_v`` on v (key side) with inputs past 2^31 elements;
    q4 / k4 hold half a byte and qs / ks 1/32 byte per element, vt / vs likewise.  causal 2
    (bottom-right) needs Sk >= Sq: key side only.  Last head: oracle/mxfp4.py, which has no mask, so only
    the cases that are not causal reach it; the causal ones rest on the bit comparison alone."""
    from oracle import mxfp4 as M
    from quantizedattention_amd.attention_mxfp4 import mxfp4_attn_fwd
    Hq, Hkv, Sq, Sk, G, heads = _heads_alone(side)
    nq, nk = _elems(side, "q"), _elems(side, "k")
    _need(nq * (2 + 2 + 0.6) + nk * (2 + 2 + 1.2) + Hq * Sq * 4)
    g = _gen("big-mxfp4", side, causal)
    q = _big_randn((1, Hq, Sq, D), g, torch.float16)
    k = _big_randn((1, Hkv, Sk, D), g, torch.float16)
    v = _big_randn((1, Hkv, Sk, D), g, torch.float16)
    O, lse, ops = mxfp4_attn_fwd(q, k, v, smooth_k=False, causal=causal)
    full = [O.view(1, Hq, -1), lse.view(1, Hq, -1), ops[0].view(1, Hq, -1), ops[1].view(1, Hq, -1)] + \
           [t.view(1, Hkv, -1) for t in ops[2:]]
    names = ("O", "lse", "q4", "qs", "k4", "ks", "vt", "vs")
    diff = _Diff()
    for kh in heads:
        hs = slice(kh * G, kh * G + G)
        qa, ka, va = q[:, hs].clone(), k[:, kh:kh + 1].clone(), v[:, kh:kh + 1].clone()
        O1, l1, ops1 = mxfp4_attn_fwd(qa, ka, va, smooth_k=False, causal=causal)
        for i, (name, a) in enumerate(zip(names, (O1, l1) + tuple(ops1))):
            f = full[i][0, hs] if i < 4 else full[i][0, kh]
            assert i >= 2 or torch.isfinite(f).all()
            diff.eq(name, (0, kh), a, f)
        if kh == heads[-1] and causal == 0:
            RO, Rl, rops = M.mxfp4_fwd(*_cpu(qa, ka, va))
            for a, b in zip(ops1, rops):
                assert torch.equal(a.cpu().reshape(b.shape), b)
            assert (O1.float().cpu() - RO.float()).abs().max().item() <= MX_O_BAR
            assert _rel(O1.cpu(), RO) <= MX_O_REL
            assert (l1.cpu() - Rl).abs().max().item() <= MX_LSE_BAR
    diff.done()


def test_mxfp4_cached_one_token_key_side(lib):
    """``attention_mxfp4_cached`` with one query token per head on the key side's cache
    (``quantize_kv_fp4`` of k, v past 2^31 elements; the decoding layout with its merge), causal and
    not: each boundary head against a cache of that head alone, at the full launch's keys per split
    (a head alone would plan more, shorter splits, and the merge sums them in another order).  No
    oracle here: oracle/mxfp4.py restates the one-pass forward on unsmoothed keys, not the decoding
    layout on a smoothed cache, whose parity tests/test_gpu_mxfp4_cache.py holds at small sizes; the
    quantisers and the forward on these same big tensors reach the oracle in the test above."""
    from quantizedattention_amd.kv_cache_mxfp4 import (QuantizedKVFP4, _split_plan_fp4, attention_mxfp4_cached,
                                                       quantize_kv_fp4)
    Hq, Hkv, Sq, Sk, G, heads = _heads_alone("k-side")
    nk = _elems("k-side", "k")
    _need(nk * (2 + 2 + 1.2))
    g = _gen("big-mxfp4-cached")
    k = _big_randn((1, Hkv, Sk, D), g, torch.float16)
    v = _big_randn((1, Hkv, Sk, D), g, torch.float16)
    q = _randn((1, Hq, 1, D), g, torch.float16)
    kv = quantize_kv_fp4(k, v)
    del k, v
    kps = _split_plan_fp4(Hkv, 1, Sk)
    diff = _Diff()
    for causal in (False, True):
        O, lse = attention_mxfp4_cached(q, kv, causal=causal, keys_per_split=kps)
        assert torch.isfinite(O).all() and torch.isfinite(lse).all()
        for kh in heads:
            one = QuantizedKVFP4(kv.k4[:, kh:kh + 1].clone(), kv.ks[:, kh:kh + 1].clone(), kv.vt[kh:kh + 1].clone(),
                                 kv.vs[kh:kh + 1].clone(), kv.k_mean[:, kh:kh + 1].clone())
            O1, l1 = attention_mxfp4_cached(q[:, kh:kh + 1].clone(), one, causal=causal, keys_per_split=kps)
            diff.eq(f"O.causal{int(causal)}", (0, kh), O1, O[0, kh])
            diff.eq(f"lse.causal{int(causal)}", (0, kh), l1, lse[kh])
    diff.done()


def test_preallocated_cache_past_2_32_bytes(lib):
    """``PreallocatedKVFP4`` with B = 66, Hkv = 8, capacity 131072 (k4 and vt 4.43e9 bytes each) holding
    a few hundred ragged tokens per sequence: two appends (the second with per-sequence counts) and
    ``attention_mxfp4_decode`` must equal, bit for bit, the same sequences in a cache of capacity 512:
    the appended rows and tiles, vtail, lens, O and lse.  Compared: sequence 0, 63 (the last below byte
    2^32), 64 (which starts at it) and 65 (past it), and O / lse of every sequence."""
    from quantizedattention_amd.kv_cache_mxfp4 import PreallocatedKVFP4, attention_mxfp4_decode
    B, Hkv, cap = CACHE
    _need(2 * B * Hkv * cap * 64 * 1.07)
    g = _gen("big-cache")
    n1, n2 = 200, 150
    k1, v1 = (_randn((B, Hkv, n1, D), g, torch.float16) for _ in range(2))
    k2, v2 = (_randn((B, Hkv, n2, D), g, torch.float16) for _ in range(2))
    counts = [(37 * b + 11) % (n2 + 1) for b in range(B)]
    q = _randn((B, 2 * Hkv, 2, D), g, torch.float16)
    k_mean = _randn((B, Hkv, 1, D), g, torch.float16, 0.1)
    caches = []
    for c in (cap, 512):
        cache = PreallocatedKVFP4.allocate(B, Hkv, c, "cuda", k_mean)
        cache.append(k1, v1).append(k2, v2, counts)
        caches.append((cache, attention_mxfp4_decode(q, cache), attention_mxfp4_decode(q, cache, causal=True)))
    (big, *big_out), (small, *small_out) = caches
    assert big.lengths == small.lengths == [n1 + c for c in counts] and len(set(counts)) > 32
    assert big.k4.numel() > 2 ** 32 and big.vt.numel() > 2 ** 32
    diff = _Diff()
    for b in (0, 63, 64, 65):
        assert (b * Hkv * cap * 64 >= 2 ** 32) == (b >= 64)
        hs = slice(b * Hkv, b * Hkv + Hkv)
        diff.eq("k4", (b,), big.k4[b, :, :512], small.k4[b])
        diff.eq("ks", (b,), big.ks[b, :, :512], small.ks[b])
        diff.eq("vt", (b,), big.vt[hs, :8], small.vt[hs])
        diff.eq("vs", (b,), big.vs[hs, :8], small.vs[hs])
        diff.eq("vtail", (b,), big.vtail[hs], small.vtail[hs])
        # nothing was written past the tiles the tokens reach
        assert not big.k4[b, :, 512:].any() and not big.vt[hs, 8:].any()
    diff.eq("lens", (), big.lens, small.lens)
    for name, a, s in zip(("O", "lse", "O.causal", "lse.causal"), big_out[0] + big_out[1], small_out[0] + small_out[1]):
        assert torch.isfinite(a).all()
        diff.eq(name, (), a, s)
    diff.done()


# -------------------------------------------------------------------------------- int8 forward
def _int8_forward_case(key, side, causal, shape=None, threshold=2 ** 31, extra_heads=()):
    from oracle import restate as R
    Hq, Hkv, Sq, Sk, G, heads = _heads_alone(side, threshold, shape)
    heads = tuple(sorted(set(heads + tuple(extra_heads))))
    g = _gen(*key)
    q = _big_randn((1, Hq, Sq, D), g, torch.float16)
    k = _big_randn((1, Hkv, Sk, D), g, torch.float16)
    v = _big_randn((1, Hkv, Sk, D), g, torch.float16)
    diff = _Diff()
    for smooth in (True, False):
        full = _int8_fwd(q, k, v, causal, smooth)
        parts = _int8_fwd_parts(full, 1, Hq, Hkv)
        for kh in heads:
            hs = slice(kh * G, kh * G + G)
            qa, ka, va = q[:, hs].clone(), k[:, kh:kh + 1].clone(), v[:, kh:kh + 1].clone()
            alone = _int8_fwd(qa, ka, va, causal, smooth)
            for name, sd, a, f in zip(FWD_NAMES, FWD_SIDE, _int8_fwd_parts(alone, 1, G, 1), parts):
                if f is not None:
                    f = f[0, hs] if sd == "q" else f[0, kh]
                    assert not f.is_floating_point() or torch.isfinite(f).all()
                    diff.eq(f"{name}.smooth{int(smooth)}", (0, kh), a, f)
            if kh == heads[-1] and not smooth:
                ref = R.int8_fwd(*_cpu(qa, ka, va), causal=causal)
                for i in (2, 3, 4, 5, 6, 7):
                    assert torch.equal(alone[i].cpu(), ref[i]), FWD_NAMES[i]
                assert (alone[0].float().cpu() - ref[0].float()).abs().max().item() <= INT8_O_BAR
                ok, lerr = lse_within_bar(alone[1].cpu(), ref[1])
                assert ok, lerr
        del full, parts
    diff.done()


@SIDE
@CAUSAL
def test_int8_forward(lib, side, causal):
    """``_int8_forward(smooth=True, images=True)`` and ``helion_atten_int8_hl_dot_fwd`` with every
    quantiser they call (q in the attention kernel, k with its mean, v with its operand image, the
    bf16 images): all eleven outputs.  Last head, plain forward: oracle/restate.py ``int8_fwd``."""
    nq, nk = _elems(side, "q"), _elems(side, "k")
    _need(nq * (2 + 2 + 1 + 2) + nk * (2 + 2 + 1 + 1 + 1 + 2))
    _int8_forward_case(("big-int8-fwd", side, causal), side, causal)


@CAUSAL
def test_int8_forward_past_2_32_elements(lib, causal):
    """The int8 forward, smoothed and plain, with its quantisers on the doubled query side, rows * D =
    4.30e9 > 2^32: the 1-byte q_i8 and the 2-byte sq / lse tables wrap only here.  Heads 0, 17476
    (straddles 2^31), 34952 (straddles 2^32) and 34999 alone; the last head's plain run against
    ``R.int8_fwd``.  About 30 GiB."""
    nq = X32[0] * X32[2] * D
    _need(nq * (2 + 2 + 1 + 2))
    at_2_31 = _heads_alone("q-side", 2 ** 31, X32)[5][1]
    assert at_2_31 == _heads_alone("q-side")[5][1]
    _int8_forward_case(("big-int8-fwd-2^32", causal), "q-side", causal, X32, 2 ** 32, extra_heads=(at_2_31,))


# -------------------------------------------------------------------------------- bf16 forward
def _bf16_inputs(key, Hq, Hkv, Sq, Sk):
    g = _gen(*key)
    q = _big_randn((1, Hq, Sq, D), g, torch.float16, 0.75)
    k = _big_randn((1, Hkv, Sk, D), g, torch.float16, 0.75)
    v = _big_randn((1, Hkv, Sk, D), g, torch.bfloat16)
    return q, k, v, g


@SIDE
@CAUSAL
def test_bf16_forward(lib, side, causal):
    """``helion_atten_bf16_fwd_training``; causal takes the V-suffix workspace, one table per
    key/value head (4104 tables of 129 rows on the key side, 17500 of 5 on the query side).  Last head: ``R.bf16_fwd`` at kt = 16."""
    from oracle import restate as R
    from quantizedattention_amd.attention_bf16 import helion_atten_bf16_fwd_training as fwd
    Hq, Hkv, Sq, Sk, G, heads = _heads_alone(side)
    _need(_elems(side, "q") * (2 + 4) + _elems(side, "k") * (2 + 2) + Hkv * (Sk // 32 + 1) * D * 4)
    q, k, v, _ = _bf16_inputs(("big-bf16-fwd", side, causal), Hq, Hkv, Sq, Sk)
    O, lse = fwd(q, k, v, causal)
    lse = lse.view(1, Hq, Sq)
    diff = _Diff()
    for kh in heads:
        hs = slice(kh * G, kh * G + G)
        qa, ka, va = q[:, hs].clone(), k[:, kh:kh + 1].clone(), v[:, kh:kh + 1].clone()
        O1, l1 = fwd(qa, ka, va, causal)
        assert torch.isfinite(O[0, hs]).all() and torch.isfinite(lse[0, hs]).all()
        diff.eq("O", (0, kh), O1, O[0, hs])
        diff.eq("lse", (0, kh), l1, lse[0, hs])
        if kh == heads[-1]:
            O_ref, l_ref = R.bf16_fwd(*_cpu(qa, ka, va), causal, kt=16)
            e_O = (O1.cpu() - O_ref).abs().view(-1, D).max(-1).values
            e_l = (l1.cpu().view(-1) - l_ref.view(-1)).abs()
            print(f"ORACLE bf16-fwd {side} causal={causal}: rows {e_O.numel()}, max|O err| {e_O.max().item():.5f} "
                  f"(rows over the bar {int((e_O > BF16_FWD_BAR).sum())}), max|lse err| {e_l.max().item():.5f} "
                  f"(rows over the bar {int((e_l > BF16_FWD_BAR).sum())})")
            assert e_O.max().item() <= BF16_FWD_BAR
            assert e_l.max().item() <= BF16_FWD_BAR
    diff.done()


# ------------------------------------------------------------------------------------- JVP
def _jvp_truth(q, k, v, tq, tk, tv, G):
    """torch.func.jvp of the fp32 baseline on the CPU (key/value heads repeated for the group) and lse
    in base 2."""
    from oracle import restate as R
    q, k, v, tq, tk, tv = (t.float() for t in _cpu(q, k, v, tq, tk, tv))
    k, v, tk, tv = (t.repeat_interleave(G, dim=1) for t in (k, v, tk, tv))
    O, tO = R.jvp_truth(q, k, v, tq, tk, tv)
    s = q @ k.transpose(-1, -2) / D ** 0.5
    return O, tO, torch.logsumexp(s, -1) * 1.4426950408889634


@pytest.mark.parametrize("case", ["q-side-bf16", "k-side-bf16", "q-side-primal-bf16", "k-side-primal-bf16", "q-side-fp32"])
def test_jvp(lib, case):
    """``_jvp``: the tangent kernel and the primal-only kernel in bf16 mode on both sides, and the fp32
    (X3) tangent kernel, with ``qattn_split_bf16`` of every operand, on the query side (module
    docstring).  Last head: torch.func.jvp of the fp32 baseline."""
    from quantizedattention_amd.attention_jvp import _jvp
    side = case[:6]
    fp32, tangent = case.endswith("fp32"), "primal" not in case
    dt = torch.float32 if fp32 else torch.bfloat16
    Hq, Hkv, Sq, Sk, G, heads = _heads_alone(side)
    nq, nk, es = _elems(side, "q"), _elems(side, "k"), 4 if fp32 else 2
    nt = 2 if tangent else 1
    _need(nt * (nq * (es + 4 + (4 if fp32 else 0)) + 2 * nk * (es + (4 if fp32 else 0))))
    g = _gen("big-jvp", case)
    q = _big_randn((1, Hq, Sq, D), g, dt)
    k, v = (_big_randn((1, Hkv, Sk, D), g, dt) for _ in range(2))
    tq = _big_randn((1, Hq, Sq, D), g, dt) if tangent else None
    tk, tv = (_big_randn((1, Hkv, Sk, D), g, dt) for _ in range(2)) if tangent else (None, None)
    O, tO, lse = _jvp(q, k, v, (tq, tk, tv) if tangent else None)
    lse = lse.view(1, Hq, Sq)
    diff = _Diff()
    for kh in heads:
        hs = slice(kh * G, kh * G + G)
        cq = lambda x: x[:, hs].clone()            # noqa: E731
        ck = lambda x: x[:, kh:kh + 1].clone()     # noqa: E731
        qa, ka, va = cq(q), ck(k), ck(v)
        tans = (cq(tq), ck(tk), ck(tv)) if tangent else None
        O1, tO1, l1 = _jvp(qa, ka, va, tans)
        assert torch.isfinite(O[0, hs]).all() and torch.isfinite(lse[0, hs]).all()
        diff.eq("O", (0, kh), O1, O[0, hs])
        diff.eq("lse", (0, kh), l1, lse[0, hs])
        if tangent:
            assert torch.isfinite(tO[0, hs]).all()
            diff.eq("tO", (0, kh), tO1, tO[0, hs])
        if kh == heads[-1]:
            zeros = tuple(torch.zeros_like(t) for t in (qa, ka, va))
            Ot, tOt, lt = _jvp_truth(qa, ka, va, *(tans or zeros), G)
            bar = JVP_FP32_BAR if fp32 else JVP_BF16_BAR
            print(f"ORACLE jvp {case}: max|O err| {(O1.cpu() - Ot).abs().max().item():.3g}, max|lse err| "
                  f"{(l1.cpu().view(lt.shape) - lt).abs().max().item():.3g}" +
                  (f", max|tO err| {(tO1.cpu() - tOt).abs().max().item():.3g} at max|tO| {tOt.abs().max().item():.3g}"
                   if tangent else ""))
            assert (O1.cpu() - Ot).abs().max().item() <= bar
            assert (l1.cpu().view(lt.shape) - lt).abs().max().item() <= bar * (max(1.0, lt.abs().max().item()) if fp32 else 1.0)
            if tangent:
                tmax = tOt.abs().max().item()
                assert (tO1.cpu() - tOt).abs().max().item() <= bar * max(1.0, tmax if fp32 else tmax / 10)
    diff.done()


# ------------------------------------------------------------------------------- int8 backward
BWD_FULL = (("recompute", dict(use_ws=False)), ("ws-onepass", dict(use_ws=True, ws_chunk=0)),
            ("ws-chunk96", dict(use_ws=True, ws_chunk=96)))
BWD_ALONE = {"recompute": dict(use_ws=False), "ws": dict(use_ws=True, ws_chunk=0)}


def _spy_on_calls(monkeypatch):
    """Every ``_lib.call`` from here on, as (entry name, arguments): a record backward falls back to
    recomputation without a word when its workspace cannot be allocated or its plan says so, and a
    test of the records must not pass on that."""
    from quantizedattention_amd import _lib
    seen, real = [], _lib.call

    def call(name, *args):
        seen.append((name, args))
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", call)
    return seen


def _took_records(seen, entry, other, ws_index):
    """The launches since ``seen`` was cleared went to the record entry, with a workspace, and never
    to the recomputing one."""
    names = [n for n, _ in seen]
    assert entry in names and other not in names, names
    for n, args in seen:
        if n == entry:
            assert args[ws_index] is not None and args[ws_index].value, "no workspace reached the record entry"


def _int8_backward_case(monkeypatch, key, Hq, Hkv, Sq, Sk, causal, heads, variants, oracle=True):
    from oracle import restate as R
    from quantizedattention_amd.attention_int8 import _int8_backward, _int8_forward
    seen = _spy_on_calls(monkeypatch)
    G = Hq // Hkv
    g = _gen(*key)
    q = _big_randn((1, Hq, Sq, D), g, torch.float16)
    k = _big_randn((1, Hkv, Sk, D), g, torch.float16)
    v = _big_randn((1, Hkv, Sk, D), g, torch.float16)
    dO = _big_randn((1, Hq, Sq, D), g, torch.float16)
    fwd = _int8_forward(q, k, v, smooth=True, images=True, causal=causal)
    del q, k, v
    O, lse, qi, kiT, vi, sq, sk, sv, _, qb, kb = fwd
    parts = _int8_fwd_parts(fwd, 1, Hq, Hkv)
    alone = {}
    for kh in heads:
        hs = slice(kh * G, kh * G + G)
        args = _int8_bwd_args(parts, dO, 1, Hq, Hkv, 0, kh, hs)
        alone[kh] = {key_: _int8_backward(*args, causal=causal, kv_heads=1, **kw) for key_, kw in BWD_ALONE.items()}
        if oracle and kh == heads[-1]:
            a = _cpu(*args)
            ref = R.int8_bwd(a[0], a[1], a[2], a[3], None, a[4], a[5], a[6], a[7], a[8], causal=causal, kv_heads=1)
            for name, x, r in zip(("dq", "dk", "dv"), alone[kh]["recompute"], ref):
                rel = _rel(x.cpu(), r)
                print(f"RELL2 int8-bwd-vs-oracle {name} {rel:.5f}")
                assert rel <= INT8_BWD_REL, (name, rel)
    diff = _Diff()
    for kh in heads:      # alone, the records give what recomputing gives
        for gname, x, r in zip(("dq", "dk", "dv"), alone[kh]["ws"], alone[kh]["recompute"]):
            diff.eq(f"alone.ws==recompute.{gname}", (0, kh), x, r)
    assert variants[0][0] == "recompute"
    whole = None          # the recomputing launch's gradients, whole: every head of the record launches
    for name, kw in variants:
        del seen[:]
        dq, dk, dv = _int8_backward(dO, qi, sq, kiT, sk, vi, sv, O, lse, qb, kb, causal=causal, kv_heads=Hkv, **kw)
        if name == "recompute":
            assert [n for n, _ in seen if "attn_bwd" in n] == ["qattn_int8_attn_bwd_ex"]
        else:
            _took_records(seen, "qattn_int8_attn_bwd_wsc", "qattn_int8_attn_bwd_ex", 15)
            chunks = [args[16] for n, args in seen if n == "qattn_int8_attn_bwd_wsc"]
            assert chunks == [Hkv if kw["ws_chunk"] == 0 else kw["ws_chunk"]]
        for kh in heads:
            hs = slice(kh * G, kh * G + G)
            a = alone[kh]["recompute" if name == "recompute" else "ws"]
            for gname, x, f in (("dq", a[0], dq[0, hs]), ("dk", a[1], dk[0, kh]), ("dv", a[2], dv[0, kh])):
                assert torch.isfinite(f).all() and f.abs().max().item() > 0
                diff.eq(f"{name}.{gname}", (0, kh), x, f)
        if whole is None:
            whole = (dq, dk, dv)
        else:
            for gname, x, r in zip(("dq", "dk", "dv"), (dq, dk, dv), whole):
                diff.eq(f"{name}==recompute.{gname}", ("every head",), x, r)
        del dq, dk, dv
    diff.done()


@SIDE
@CAUSAL
def test_int8_backward(lib, monkeypatch, side, causal):
    """``_int8_backward`` on the full launch's own forward outputs: dq, dk, dv of the recomputing
    backward, of the record backward in one pass and in chunks of 96 key/value heads (a short last
    chunk on both sides).  The three heads against their runs alone; the whole dq, dk, dv of both record
    launches against the recomputing launch's, so every head is looked at; and the record launches must
    have reached ``qattn_int8_attn_bwd_wsc`` with a workspace.  Last head, recomputing:
    oracle/restate.py ``int8_bwd``."""
    Hq, Hkv, Sq, Sk, G, heads = _heads_alone(side)
    nq, nk = _elems(side, "q"), _elems(side, "k")
    records = Hq * (Sq // 32) * (Sk // 32) * (1024 + 4)
    _need(nq * (2 + 2 + 1 + 2 + 2 + 1 + 2 + 2 + 2) + nk * (2 + 2 + 1 + 1 + 1 + 2 + 2 + 2 + 4) + records)
    _int8_backward_case(monkeypatch, ("big-int8-bwd", side, causal), Hq, Hkv, Sq, Sk, causal, heads, BWD_FULL)


# ------------------------------------------------------------------------------- bf16 backward
BF16_ENTRIES = ("ws", "qattn_bf16_bwd_ex", "qattn_bf16_bwd_split_ex")


def _bf16_backward_case(monkeypatch, key, Hq, Hkv, Sq, Sk, causal, heads, entries, oracle=True):
    from oracle import restate as R
    from quantizedattention_amd import attention_bf16 as A
    seen = _spy_on_calls(monkeypatch)
    G = Hq // Hkv
    q, k, v, g = _bf16_inputs(key, Hq, Hkv, Sq, Sk)
    dO = _big_randn((1, Hq, Sq, D), g, torch.float32)
    O, lse = A.helion_atten_bf16_fwd_training(q, k, v, causal)
    alone = {}
    for kh in heads:
        hs = slice(kh * G, kh * G + G)
        args = (q[:, hs].clone(), k[:, kh:kh + 1].clone(), v[:, kh:kh + 1].clone(), O[:, hs].clone(),
                lse.view(1, Hq, Sq)[0, hs].clone(), causal, dO[:, hs].clone())
        alone[kh] = {}
        for entry in entries:
            monkeypatch.setattr(A, "_BWD_ENTRY", entry)
            alone[kh][entry] = A.helion_flash_atten_2_algo_4_bwd(*args)
        if oracle and kh == heads[-1]:
            a = _cpu(*args[:5]) + [causal] + _cpu(args[6])
            for name, x, r in zip(("dq", "dk", "dv"), alone[kh][entries[0]], R.bf16_bwd(*a)):
                assert _rel(x.cpu(), r) <= BF16_BWD_REL, (name, _rel(x.cpu(), r))
    diff = _Diff()
    assert entries[0] == "ws" and entries[1] == "qattn_bf16_bwd_ex"
    for kh in heads:      # alone, every entry gives what the recomputing one gives
        for entry in entries:
            if entry != entries[1]:
                for gname, x, r in zip(("dq", "dk", "dv"), alone[kh][entry], alone[kh][entries[1]]):
                    diff.eq(f"alone.{entry}==recompute.{gname}", (0, kh), x, r)
    whole = {}            # every entry's gradients, whole: every head of the launches against each other
    for entry in entries:
        monkeypatch.setattr(A, "_BWD_ENTRY", entry)
        del seen[:]
        dq, dk, dv = A.helion_flash_atten_2_algo_4_bwd(q, k, v, O, lse, causal, dO)
        if entry == "ws":
            _took_records(seen, "qattn_bf16_bwd_ws_ex", "qattn_bf16_bwd_ex", -2)
        else:
            assert [n for n, _ in seen if "bf16_bwd" in n and "prep" not in n] == [entry]
        for kh in heads:
            hs = slice(kh * G, kh * G + G)
            a = alone[kh][entry]
            for gname, x, f in (("dq", a[0], dq[0, hs]), ("dk", a[1], dk[0, kh]), ("dv", a[2], dv[0, kh])):
                assert torch.isfinite(f).all() and f.abs().max().item() > 0
                diff.eq(f"{entry}.{gname}", (0, kh), x, f)
        whole[entry] = (dq, dk, dv)
        if entry != "ws":
            for gname, x, r in zip(("dq", "dk", "dv"), whole[entry], whole["ws"]):
                diff.eq(f"{entry}==ws.{gname}", ("every head",), x, r)
            del whole[entry]
        del dq, dk, dv
    diff.done()


@SIDE
@CAUSAL
def test_bf16_backward(lib, monkeypatch, side, causal):
    """``helion_flash_atten_2_algo_4_bwd`` through its three entries: the dS records (4.3 GB of them on
    the query side, past 2^32 bytes themselves), the fused
    dK+dV with a recomputing dQ, and the split dV / dK kernels.  The three heads against their runs
    alone; the whole dq, dk, dv of the recomputing and the split launch against the record launch's, so
    every head is looked at; and the record launch must have reached ``qattn_bf16_bwd_ws_ex`` with a
    workspace.  Last head: ``R.bf16_bwd``."""
    Hq, Hkv, Sq, Sk, G, heads = _heads_alone(side)
    nq, nk = _elems(side, "q"), _elems(side, "k")
    records = Hq * (Sq // 32) * (Sk // 32) * 2048
    _need(nq * (2 + 4 + 4 + 2 + 2 + 4 + 4) + nk * (2 + 2 + 2 + 4 + 4 + 8) + records)
    _bf16_backward_case(monkeypatch, ("big-bf16-bwd", side, causal), Hq, Hkv, Sq, Sk, causal, heads, BF16_ENTRIES)


# ----------------------------------------------------------------- record workspaces past 4 GiB
@CAUSAL
def test_int8_records_past_4_gib(lib, monkeypatch, causal):
    """65 heads at Sq = Sk = 8192: the int8 dS records pass 4 GiB by one whole head region.  The whole
    dq, dk, dv of one pass (``ws_chunk=0``) and of chunks of 16 heads (a last chunk of one) against the
    recomputing backward's, all 65 heads; heads 0, 63 (its records end just below 4 GiB) and 64 (wholly
    past it) against the head alone, records and recomputing.  The record launches must have reached
    ``qattn_int8_attn_bwd_wsc`` with a workspace: a fallback to recomputation fails the test."""
    from quantizedattention_amd import _lib
    H, S = WS_INT8_HEADS, WS_S
    assert _lib.int8_bwd_plan(H, 1, S, S, causal, 0, _lib.UNBOUNDED)[0] == H * WS_INT8_HEAD_BYTES
    n = H * S * D
    _need(n * (2 + 2 + 1 + 2 + 2 + 1 + 2 + 2 + 2 * (2 + 2 + 1 + 1 + 1 + 2 + 2)) + H * WS_INT8_HEAD_BYTES)
    heads = (0, (2 ** 32 - 1) // WS_INT8_HEAD_BYTES, H - 1)
    assert heads == (0, 63, 64) and heads[2] * (S // 32) ** 2 * 1024 >= 2 ** 32
    variants = (("recompute", dict(use_ws=False)), ("ws-onepass", dict(use_ws=True, ws_chunk=0)),
                ("ws-chunk16", dict(use_ws=True, ws_chunk=16)))
    _int8_backward_case(monkeypatch, ("big-int8-ws", causal), H, H, S, S, causal, heads, variants, oracle=False)


@CAUSAL
def test_bf16_records_past_4_gib(lib, monkeypatch, causal):
    """33 heads at Sq = Sk = 8192: the bf16 dS records (128 MiB per head) pass 4 GiB by one whole head
    region.  The whole dq, dk, dv of the record entry against the recomputing one's, all 33 heads; heads
    0, 31 and 32 against the head alone.  The record launch must have reached ``qattn_bf16_bwd_ws_ex``
    with a workspace: a fallback to recomputation fails the test."""
    from quantizedattention_amd import _lib
    H, S = WS_BF16_HEADS, WS_S
    assert _lib.load().qattn_bf16_bwd_ws_bytes(H, S, S) == H * WS_BF16_HEAD_BYTES
    n = H * S * D
    _need(n * (2 + 4 + 4 + 2 + 2 + 4 + 2 + 2 + 2 + 4 + 4) + H * WS_BF16_HEAD_BYTES)
    heads = (0, (2 ** 32 - 1) // WS_BF16_HEAD_BYTES, H - 1)
    assert heads == (0, 31, 32)
    _bf16_backward_case(monkeypatch, ("big-bf16-ws", causal), H, H, S, S, causal, heads,
                        ("ws", "qattn_bf16_bwd_ex"), oracle=False)
