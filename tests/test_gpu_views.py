"""Every public entry gives the same bits whatever view its inputs arrive as.

The wrappers normalise inputs with ``_lib.kernel_input`` (dtype, contiguous, 16-byte aligned address;
``qattn_ops.cpp`` has the same helper) and hand ``data_ptr()`` to kernels that read 16-byte vectors
and LDS-DMA dwordx4 from it.  Each entry runs with all of its tensor inputs in four forms:

  clone        a fresh contiguous tensor (the reference);
  offset       ``big[1:]`` of a buffer with one more leading entry: contiguous, a non-zero storage
               offset, 16-byte aligned, the neighbours on both sides filled with large finite garbage
               (a kernel that read before or past its tensor would show it);
  transposed   a ``[B, S, H, D]`` tensor seen as ``[B, H, S, D]`` (4-D tensors; the others as clones);
  misaligned   ``flat[1:1 + n].view(shape)``: contiguous, one element past an aligned address, which
               the helper must copy (``_lib.ptr`` refuses such an address outright).

and every output must equal the clone form's, bit for bit.  For the caches the offset form also
applies to the cache's own ``k_mean``, ``lens`` / ``block_table`` and operand buffers.

Shapes (B, Hq, Hkv, Sq, Sk): one grouped and ragged (2, 4, 2, 96, 160), one ungrouped with an odd head
count and Sq > Sk (1, 3, 3, 160, 96); Sq is no multiple of a 128- or 256-row workgroup.  The paths that
stream 64-key stages (JVP bf16 mode, MX-FP4) take Sk rounded up to 192 / 128.
"""
import pytest
import torch

from head_alone import _Diff, _gen, _randn

pytestmark = pytest.mark.gpu

FORMS = ("offset", "transposed", "misaligned")
SHAPES = [(2, 4, 2, 96, 160), (1, 3, 3, 160, 96)]
SHAPE_IDS = ["grouped-96x160", "odd-heads-160x96"]


def _garbage(n, dtype):
    """Large finite values of alternating sign; for int32 (lengths, counts, page tables) small wrong
    values, which a kernel that read them would still index in range with."""
    if dtype == torch.int32:
        return torch.ones((n,), dtype=dtype, device="cuda")
    big = {torch.float16: 6.0e4, torch.bfloat16: 3.0e38, torch.float32: 3.0e38, torch.int8: 127,
           torch.uint8: 255, torch.int64: 1}[dtype]
    t = torch.full((n,), big, dtype=dtype, device="cuda")
    if dtype != torch.uint8:
        t[1::2] = -big
    return t


def _embedded(x, lead):
    """``x`` as a contiguous view ``lead`` elements into a flat buffer of garbage."""
    flat = _garbage(lead + x.numel() + 64, x.dtype)
    y = flat[lead:lead + x.numel()].view(x.shape)
    y.copy_(x)
    return y


def _form(x, form):
    """``x`` (a tensor, or anything else, which passes through) in one of the four forms."""
    if not isinstance(x, torch.Tensor) or x.numel() == 0:
        return x
    if x.dim() == 2 and not x.is_contiguous():        # k_i8T: the [D, N] view of a row-major [N, D]
        return _form(x.t(), form).t()
    if form == "clone":
        return x.clone()
    if form == "transposed":
        if x.dim() != 4:
            return x.clone()
        y = x.transpose(1, 2).contiguous().transpose(1, 2)
        assert y.shape == x.shape and (y.is_contiguous() == (x.shape[1] == 1 or x.shape[2] == 1))
        return y
    if form == "offset":
        lead = x[0].numel() if x.dim() == 4 and x[0].numel() * x.element_size() % 16 == 0 else 64
        y = _embedded(x, lead)
        assert y.is_contiguous() and y.storage_offset() > 0 and y.data_ptr() % 16 == 0
        return y
    assert form == "misaligned"
    y = _embedded(x, 1)
    assert y.is_contiguous() and y.data_ptr() % 16 == x.element_size() % 16 != 0
    return y


def _forms(args, form):
    return [_form(a, form) for a in args]


def _same(diff, name, form, got, want):
    """Every tensor of ``got`` (a tensor or a tuple) equals its partner in ``want`` bit for bit."""
    got = (got,) if isinstance(got, torch.Tensor) else got
    want = (want,) if isinstance(want, torch.Tensor) else want
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        if isinstance(b, torch.Tensor):
            assert a.shape == b.shape and a.dtype == b.dtype
            diff.eq(f"{name}[{i}]", (form,), a, b)
        else:
            assert a == b


def _every_form(diff, name, fn, args):
    """``fn(*args)`` in the clone form, then in every other form against it; returns the former."""
    want = fn(*_forms(args, "clone"))
    for form in FORMS:
        _same(diff, name, form, fn(*_forms(args, form)), want)
    return want


def _qkv(key, shape, D, dtypes, sk_mult=32, scale=1.0):
    B, Hq, Hkv, Sq, Sk = shape
    Sk = -(-Sk // sk_mult) * sk_mult
    g = _gen(*key)
    shapes = ((B, Hq, Sq, D), (B, Hkv, Sk, D), (B, Hkv, Sk, D))
    return [_randn(s, g, dt, scale) for s, dt in zip(shapes, dtypes)], g


def test_forms_are_what_they_say(lib):
    """The four forms hold equal values, the garbage really surrounds the views, and a misaligned
    address never reaches a kernel: ``kernel_input`` copies it, ``ptr`` refuses it."""
    from quantizedattention_amd import _lib
    x = _randn((2, 3, 32, 64), _gen("forms"), torch.float16)
    for form in ("clone",) + FORMS:
        y = _form(x, form)
        assert torch.equal(y, x) and y.data_ptr() != x.data_ptr()
        z = _lib.kernel_input(y)
        assert z.is_contiguous() and z.data_ptr() % 16 == 0 and torch.equal(z, x)
        assert (z.data_ptr() == y.data_ptr()) == (form in ("clone", "offset"))
    y = _form(x, "offset")
    before = torch.as_strided(y, (8,), (1,), y.storage_offset() - 8)
    after = torch.as_strided(y, (8,), (1,), y.storage_offset() + y.numel())
    assert float(before.abs().min()) == 6.0e4 and float(after.abs().min()) == 6.0e4
    with pytest.raises(_lib.QAttnError, match="not a multiple of 16"):
        _lib.ptr(_form(x, "misaligned"))
    assert _lib.ptr(None) is None and _lib.kernel_input(None) is None
    assert _lib.kernel_input(x, torch.bfloat16).dtype == torch.bfloat16


# ------------------------------------------------------------------------------------ int8
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("D", [64, 128])
def test_int8(lib, D, causal, shape):
    """``_int8_forward`` (smoothed, with images), ``helion_atten_int8_hl_dot_fwd`` / ``_bwd``,
    ``_int8_backward`` from records and by recomputation, and ``sage_attention_3_int8`` through
    autograd."""
    from quantizedattention_amd import attention_int8 as A
    (q, k, v), g = _qkv(("views-int8", D, causal, shape), shape, D, [torch.float16] * 3)
    dO = _randn(q.shape, g, torch.float16)
    Hkv = shape[2]
    diff = _Diff()
    tensors = lambda out: tuple(t for t in out if isinstance(t, torch.Tensor))   # noqa: E731
    O, lse, qi, kiT, vi, sq, sk, sv, kmean, qbf, kbf = _every_form(
        diff, "fwd-smooth", lambda *a: tensors(A._int8_forward(*a, smooth=True, images=True, causal=causal)), (q, k, v))
    _every_form(diff, "fwd-plain", lambda *a: tensors(A.helion_atten_int8_hl_dot_fwd(*a, causal=causal)), (q, k, v))
    _every_form(diff, "bwd", lambda *a: A.helion_atten_int8_hl_dot_bwd(*a, 32, 32, causal=causal, kv_heads=Hkv),
                (dO, qi, sq, kiT, kmean, sk, vi, sv, O, lse))
    for use_ws in (True, False):
        _every_form(diff, f"bwd-ws{int(use_ws)}",
                    lambda *a: A._int8_backward(*a, causal=causal, kv_heads=Hkv, use_ws=use_ws),
                    (dO, qi, sq, kiT, sk, vi, sv, O, lse, qbf, kbf))

    def autograd(q_, k_, v_, dO_):
        leaves = [t.requires_grad_(True) for t in (q_, k_, v_)]
        out = A.sage_attention_3_int8(*leaves, causal)
        out.backward(dO_)
        return (out.detach(),) + tuple(t.grad for t in leaves)
    _every_form(diff, "autograd", autograd, (q, k, v, dO))
    diff.done()


# ------------------------------------------------------------------------------------ bf16
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("D", [64, 128])
def test_bf16(lib, D, causal, shape):
    """``helion_atten_bf16_fwd_training``, ``helion_flash_atten_2_algo_4_bwd`` and
    ``flash_atten_2_bf16`` through autograd."""
    from quantizedattention_amd import attention_bf16 as A
    (q, k, v), g = _qkv(("views-bf16", D, causal, shape), shape, D,
                        [torch.float16, torch.float16, torch.bfloat16], scale=0.75)
    dO = _randn(q.shape, g, torch.float32)
    diff = _Diff()
    O, lse = _every_form(diff, "fwd", lambda *a: A.helion_atten_bf16_fwd_training(*a, causal), (q, k, v))
    _every_form(diff, "bwd", lambda q_, k_, v_, O_, l_, dO_: A.helion_flash_atten_2_algo_4_bwd(q_, k_, v_, O_, l_, causal, dO_),
                (q, k, v, O, lse, dO))

    def autograd(q_, k_, v_, dO_):
        leaves = [t.requires_grad_(True) for t in (q_, k_, v_)]
        out = A.flash_atten_2_bf16(*leaves, causal)
        out.backward(dO_)
        return (out.detach(),) + tuple(t.grad for t in leaves)
    _every_form(diff, "autograd", autograd, (q, k, v, dO))
    diff.done()


# ------------------------------------------------------------------------------------- JVP
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("D", [64, 128])
def test_jvp(lib, D, mode, shape):
    """``helion_attention_jvp_forward_fp32`` in both modes and the primal-only kernel behind
    ``attention_jvp``."""
    from quantizedattention_amd import attention_jvp as A
    dt = torch.bfloat16 if mode == "bf16" else torch.float32
    (q, k, v), g = _qkv(("views-jvp", D, mode, shape), shape, D, [dt] * 3, sk_mult=64 if mode == "bf16" else 32)
    tq, tk, tv = (_randn(t.shape, g, dt) for t in (q, k, v))
    diff = _Diff()
    _every_form(diff, "tangent", A.helion_attention_jvp_forward_fp32, (q, k, v, tq, tk, tv))
    _every_form(diff, "primal", A.attention_jvp, (q, k, v))
    diff.done()


# ----------------------------------------------------------------------------------- MX-FP4
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("causal", [0, 1], ids=["full", "causal"])
def test_mxfp4_forward_and_quantised_cache(lib, causal, shape):
    """``mxfp4_attn_fwd`` (O, lse and the six operands), ``quantize_kv_fp4`` with its own and with a
    given ``k_mean``, and ``attention_mxfp4_cached`` with one query token per head."""
    from quantizedattention_amd.attention_mxfp4 import mxfp4_attn_fwd
    from quantizedattention_amd.kv_cache_mxfp4 import attention_mxfp4_cached, quantize_kv_fp4
    (q, k, v), g = _qkv(("views-mxfp4", causal, shape), shape, 128, [torch.float16] * 3, sk_mult=64)
    if causal and q.shape[2] > k.shape[2]:
        causal = 1      # (top-left; bottom-right needs Sk >= Sq)
    k_mean = _randn((k.shape[0], k.shape[1], 1, 128), g, torch.float16, 0.1)
    diff = _Diff()

    def fwd(q_, k_, v_):
        O, lse, ops = mxfp4_attn_fwd(q_, k_, v_, causal=causal)
        return (O, lse) + tuple(ops)
    _every_form(diff, "fwd", fwd, (q, k, v))
    flat = lambda kv: kv.kv + ((kv.k_mean,) if kv.k_mean is not None else ())   # noqa: E731
    _every_form(diff, "quantize_kv", lambda k_, v_: flat(quantize_kv_fp4(k_, v_)), (k, v))
    _every_form(diff, "quantize_kv-mean", lambda k_, v_, m_: flat(quantize_kv_fp4(k_, v_, k_mean=m_)), (k, v, k_mean))
    kv = quantize_kv_fp4(k, v)
    q1 = q[:, :, :1]
    _every_form(diff, "cached", lambda q_: attention_mxfp4_cached(q_, kv, causal=bool(causal)), (q1.contiguous(),))
    diff.done()


def _cache_state(cache, extra=()):
    return tuple(t.clone() for t in (cache.k4, cache.ks, cache.vt, cache.vs, cache.vtail, cache.lens) + tuple(extra))


def _offset_buffers(cache, names):
    """The cache's own buffers as offset views (same values, garbage around them)."""
    for name in names:
        setattr(cache, name, _form(getattr(cache, name), "offset"))
    return cache


@pytest.mark.parametrize("smoothed", [False, True], ids=["plain", "smoothed"])
def test_preallocated_cache(lib, smoothed):
    """``PreallocatedKVFP4``: two ragged appends (the second with per-sequence counts given as a
    tensor) and ``attention_mxfp4_decode``, causal and not: the cache's bytes, lengths, O and lse."""
    from quantizedattention_amd.kv_cache_mxfp4 import PreallocatedKVFP4, attention_mxfp4_decode
    B, Hq, Hkv, cap = 3, 4, 2, 256
    g = _gen("views-prealloc", smoothed)
    k1, v1, k2, v2 = (_randn((B, Hkv, n, 128), g, torch.float16) for n in (70, 70, 45, 45))
    q = _randn((B, Hq, 3, 128), g, torch.float16)
    k_mean = _randn((B, Hkv, 1, 128), g, torch.float16, 0.1) if smoothed else None
    counts = torch.tensor([45, 0, 17], dtype=torch.int32, device="cuda")
    BUFFERS = ("k4", "ks", "vt", "vs", "vtail", "lens") + (("k_mean",) if smoothed else ())

    def run(k1_, v1_, k2_, v2_, q_, counts_, mean_, offset_cache=False):
        cache = PreallocatedKVFP4.allocate(B, Hkv, cap, "cuda", mean_)
        if offset_cache:
            _offset_buffers(cache, BUFFERS)
        cache.append(k1_, v1_).append(k2_, v2_, counts_)
        assert cache.lengths == [115, 70, 87]
        outs = ()
        for causal in (False, True):
            outs += attention_mxfp4_decode(q_, cache, causal=causal)
        return _cache_state(cache) + outs

    args = (k1, v1, k2, v2, q, counts, k_mean)
    diff = _Diff()
    want = _every_form(diff, "cache", run, args)
    _same(diff, "cache", "offset-buffers", run(*_forms(args, "offset"), offset_cache=True), want)
    diff.done()


def test_paged_cache(lib):
    """``PagedKVFP4``: the same appends into a page pool with a shuffled free list, and
    ``attention_mxfp4_decode_paged``; it must also equal the preallocated cache's O and lse."""
    from quantizedattention_amd.kv_cache_mxfp4 import (PagedKVFP4, PreallocatedKVFP4, attention_mxfp4_decode,
                                                       attention_mxfp4_decode_paged)
    B, Hq, Hkv = 3, 4, 2
    g = _gen("views-paged")
    k1, v1, k2, v2 = (_randn((B, Hkv, n, 128), g, torch.float16) for n in (70, 70, 45, 45))
    q = _randn((B, Hq, 3, 128), g, torch.float16)
    k_mean = _randn((B, Hkv, 1, 128), g, torch.float16, 0.1)
    counts = torch.tensor([45, 0, 17], dtype=torch.int32, device="cuda")
    order = [5, 2, 7, 0, 3, 6, 1, 4]

    def run(k1_, v1_, k2_, v2_, q_, counts_, mean_, offset_cache=False):
        cache = PagedKVFP4.allocate(8, 64, B, Hkv, 3, "cuda", mean_, free_order=order)
        if offset_cache:
            _offset_buffers(cache, ("k4", "ks", "vt", "vs", "vtail", "lens", "block_table", "k_mean"))
        cache.append(k1_, v1_).append(k2_, v2_, counts_)
        assert cache.lengths == [115, 70, 87]
        outs = ()
        for causal in (False, True):
            outs += attention_mxfp4_decode_paged(q_, cache, causal=causal)
        return _cache_state(cache, (cache.block_table,)) + outs

    args = (k1, v1, k2, v2, q, counts, k_mean)
    diff = _Diff()
    want = _every_form(diff, "paged", run, args)
    _same(diff, "paged", "offset-buffers", run(*_forms(args, "offset"), offset_cache=True), want)
    flat = PreallocatedKVFP4.allocate(B, Hkv, 192, "cuda", k_mean)
    flat.append(k1, v1).append(k2, v2, counts)
    ref = attention_mxfp4_decode(q, flat, causal=False) + attention_mxfp4_decode(q, flat, causal=True)
    _same(diff, "paged-vs-preallocated", "clone", want[-4:], ref)
    diff.done()


def test_misaligned_cache_buffer_is_refused(lib):
    """The caches pass their own buffers to the kernels as they are, so one at a misaligned address is
    refused by ``_lib.ptr`` (and by the operators) before a launch."""
    from quantizedattention_amd import _lib, ops
    from quantizedattention_amd.kv_cache_mxfp4 import PreallocatedKVFP4, attention_mxfp4_decode
    g = _gen("views-refused")
    k, v = (_randn((2, 2, 64, 128), g, torch.float16) for _ in range(2))
    q = _randn((2, 4, 1, 128), g, torch.float16)
    cache = PreallocatedKVFP4.allocate(2, 2, 128, "cuda").append(k, v)
    want = attention_mxfp4_decode(q, cache)
    cache.lens = _form(cache.lens, "misaligned")
    with pytest.raises(_lib.QAttnError, match="not a multiple of 16"):
        attention_mxfp4_decode(q, cache)
    with pytest.raises(_lib.QAttnError, match="not a multiple of 16"):
        cache.append(k[:, :, :1], v[:, :, :1])
    assert cache.lengths == [64, 64]
    with pytest.raises(RuntimeError, match="not a multiple of 16"):
        ops.mxfp4_decode(q, cache)
    cache.lens = _form(cache.lens, "offset")
    got = attention_mxfp4_decode(q, cache)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# -------------------------------------------------------------------------------- operators
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_operators(lib, shape):
    """Every ``torch.ops.qattn`` operator that takes tensors a caller made (D = 128, causal)."""
    from quantizedattention_amd import ops
    from quantizedattention_amd.kv_cache_mxfp4 import PagedKVFP4, PreallocatedKVFP4, quantize_kv_fp4
    B, Hq, Hkv, Sq, Sk = shape
    (q, k, v), g = _qkv(("views-ops", shape), shape, 128, [torch.float16] * 3, sk_mult=64)
    dO = _randn(q.shape, g, torch.float16)
    diff = _Diff()
    _every_form(diff, "int8_quant", lambda x: ops.int8_quant(x, 32), (q,))
    O, lse, qi, ki, vi, sq, sk, sv = _every_form(diff, "int8_fwd", lambda *a: ops.int8_fwd(*a, True, True), (q, k, v))
    _every_form(diff, "int8_bwd", lambda *a: ops.int8_bwd(*a, True, Hkv), (dO, qi, sq, ki, sk, vi, sv, O, lse))
    vb = v.bfloat16()
    Ob, lb = _every_form(diff, "bf16_fwd", lambda *a: ops.bf16_fwd(*a, True), (q * 0.75, k * 0.75, vb))
    _every_form(diff, "bf16_bwd", lambda q_, k_, v_, O_, l_, d_: ops.bf16_bwd(q_, k_, v_, O_, l_, True, d_),
                (q * 0.75, k * 0.75, vb, Ob, lb, dO.float()))
    for dt in (torch.bfloat16, torch.float32):
        x = [t.to(dt) for t in (q, k, v, dO, k.flip(2), v.flip(2))]
        _every_form(diff, f"jvp_fwd-{dt}", ops.jvp_fwd, x)
    mode = 2 if Sq <= k.shape[2] else 1
    _every_form(diff, "mxfp4_fwd", ops.mxfp4_fwd, (q, k, v))
    _every_form(diff, "mxfp4_fwd_ex", lambda *a: ops.mxfp4_fwd_ex(*a, mode), (q, k, v))
    q1 = q[:, :, :1].contiguous()
    kv = quantize_kv_fp4(k, v)
    _every_form(diff, "mxfp4_cached", lambda q_: ops.mxfp4_cached(q_, kv, True), (q1,))
    pre = PreallocatedKVFP4.allocate(B, Hkv, 256, "cuda").append(k[:, :, :77], v[:, :, :77])
    _every_form(diff, "mxfp4_decode", lambda q_: ops.mxfp4_decode(q_, pre, True), (q1,))
    paged = PagedKVFP4.allocate(2 * B, 64, B, Hkv, 2, "cuda").append(k[:, :, :77], v[:, :, :77])
    _every_form(diff, "mxfp4_decode_paged", lambda q_: ops.mxfp4_decode_paged(q_, paged, True), (q1,))
    diff.done()
