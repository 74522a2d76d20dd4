"""Edge cases on the GPU: empty batches, all-zero blocks (zero scales), constant inputs and large
magnitudes, through the drop-ins, the C++ operators and the decoding path."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


def _exact_attention(q, k, v, causal=False):
    """fp32 softmax attention on the CPU (no quantisation), the yardstick for both int8 paths."""
    q, k, v = (t.float() for t in (q, k, v))
    s = q @ k.transpose(-1, -2) / q.shape[-1] ** 0.5
    if causal:
        s = s.masked_fill(torch.ones(s.shape[-2:], dtype=torch.bool).triu(1), float("-inf"))
    return torch.softmax(s, dim=-1) @ v


def _exact_lse2(q, k, causal=False):
    """log2 of the softmax denominator of exact attention (the reference's lse is in log2 units),
    flattened like the drop-in's lse."""
    q, k = q.float(), k.float()
    s = q @ k.transpose(-1, -2) / q.shape[-1] ** 0.5 * 1.4426950408889634
    if causal:
        s = s.masked_fill(torch.ones(s.shape[-2:], dtype=torch.bool).triu(1), float("-inf"))
    return (torch.logsumexp(s * 0.6931471805599453, dim=-1) * 1.4426950408889634).reshape(-1)


def test_empty_batch(lib):
    import quantizedattention_amd.ops  # noqa: F401
    from quantizedattention_amd.attention_bf16 import flash_atten_2_bf16
    from quantizedattention_amd.attention_int8 import sage_attention_3_int8
    from quantizedattention_amd.attention_jvp import helion_attention_jvp_forward_fp32
    q = torch.zeros((0, 2, 64, 128), dtype=torch.float16, device="cuda", requires_grad=True)
    O = sage_attention_3_int8(q, q, q)
    assert O.shape == q.shape
    O.sum().backward()
    assert q.grad.shape == q.shape
    Ob = flash_atten_2_bf16(q.detach(), q.detach(), q.detach().bfloat16(), False)
    assert Ob.shape == q.shape
    x = torch.zeros((0, 2, 64, 128), dtype=torch.bfloat16, device="cuda")
    O, tO, lse = helion_attention_jvp_forward_fp32(x, x, x, x, x, x)
    assert O.shape == x.shape and tO.shape == x.shape and lse.numel() == 0
    outs = torch.ops.qattn.int8_fwd(q.detach(), q.detach(), q.detach(), True, False)
    assert outs[0].shape == q.shape and outs[2].numel() == 0
    torch.cuda.synchronize()


def _z(shape, dt=torch.float16):
    return torch.zeros(shape, dtype=dt, device="cuda")


# (q shape, k / v shape): no batch entry, no query head, no query token -- each with keys to attend to
# wherever a key/value head exists
EMPTY_ROWS = {"B=0": ((0, 4, 64, 128), (0, 2, 64, 128)), "Hq=0": ((1, 0, 64, 128), (1, 2, 64, 128)),
              "Sq=0": ((1, 4, 0, 128), (1, 2, 64, 128))}


@pytest.mark.parametrize("which", list(EMPTY_ROWS))
def test_empty_query_rows(lib, which):
    """B = 0, Hq = 0 and Sq = 0: every path returns empty outputs of the right shapes (and zero dk, dv
    of k's shape where it has a backward) without launching an attention kernel."""
    from quantizedattention_amd import ops
    from quantizedattention_amd.attention_bf16 import flash_atten_2_bf16, helion_atten_bf16_fwd_training
    from quantizedattention_amd.attention_int8 import helion_atten_int8_hl_dot_fwd, sage_attention_3_int8
    from quantizedattention_amd.attention_jvp import attention_jvp, helion_attention_jvp_forward_fp32
    from quantizedattention_amd.attention_mxfp4 import mxfp4_attn_fwd, sage_attention_3_fp4
    qs, ks = EMPTY_ROWS[which]
    rows = qs[0] * qs[1] * qs[2]
    assert rows == 0
    # int8, through autograd and the reference-shaped forward
    q, k, v = _z(qs).requires_grad_(True), _z(ks).requires_grad_(True), _z(ks).requires_grad_(True)
    for causal in (False, True):
        O = sage_attention_3_int8(q, k, v, causal)
        assert O.shape == qs and O.dtype == torch.float16
        O.sum().backward()
        assert q.grad.shape == qs and k.grad.shape == ks and v.grad.shape == ks
        assert not k.grad.any() and not v.grad.any()
    out = helion_atten_int8_hl_dot_fwd(q.detach(), k.detach(), v.detach())
    assert out[0].shape == qs and out[1].numel() == 0 and out[2].shape == (0, 128) and out[5].numel() == 0
    assert out[3].shape == (128, ks[0] * ks[1] * ks[2])
    # bf16, forward and autograd
    qb, kb, vb = _z(qs).requires_grad_(True), _z(ks).requires_grad_(True), _z(ks, torch.bfloat16).requires_grad_(True)
    for causal in (False, True):
        O, lse = helion_atten_bf16_fwd_training(qb.detach(), kb.detach(), vb.detach(), causal)
        assert O.shape == qs and O.dtype == torch.float32 and lse.shape == (qs[0] * qs[1], qs[2])
        O = flash_atten_2_bf16(qb, kb, vb, causal)
        O.sum().backward()
        assert qb.grad.shape == qs and kb.grad.shape == ks and vb.grad.shape == ks
        assert not kb.grad.any() and not vb.grad.any()
    # JVP, both modes, and the autograd Function's plain forward
    for dt in (torch.bfloat16, torch.float32):
        x, y = _z(qs, dt), _z(ks, dt)
        O, tO, lse = helion_attention_jvp_forward_fp32(x, y, y, x, y, y)
        assert O.shape == qs and tO.shape == qs and lse.shape == (qs[0] * qs[1], qs[2])
        assert attention_jvp(x, y, y).shape == qs
        O, tO, lse = ops.jvp_fwd(x, y, y, x, y, y)
        assert O.shape == qs and tO.shape == qs and lse.shape == (qs[0] * qs[1], qs[2])
    # MX-FP4
    for causal in (0, 1, 2):
        O, lse, _ = mxfp4_attn_fwd(q.detach(), k.detach(), v.detach(), causal=causal)
        assert O.shape == qs and lse.shape == (qs[0] * qs[1], qs[2])
        assert ops.mxfp4_fwd_ex(q.detach(), k.detach(), v.detach(), causal).shape == qs
    assert sage_attention_3_fp4(q.detach(), k.detach(), v.detach()).shape == qs
    assert ops.mxfp4_fwd(q.detach(), k.detach(), v.detach()).shape == qs
    # the other operators
    for smooth in (False, True):
        outs = ops.int8_fwd(q.detach(), k.detach(), v.detach(), smooth, False)
        assert outs[0].shape == qs and outs[2].numel() == 0 and outs[3].shape == (ks[0] * ks[1] * ks[2], 128)
        dq, dk, dv = ops.int8_bwd(_z(qs), outs[2], outs[5], outs[3], outs[6], outs[4], outs[7], outs[0],
                                  outs[1], False, ks[1])
        # (the operator reads Sk off k_i8 [B*Hkv*Sk, D], which an empty batch does not tell)
        ks_op = ks if ks[0] else (0, ks[1], 0, 128)
        assert dq.shape == qs and dk.shape == ks_op and dv.shape == ks_op and not dk.any() and not dv.any()
    O, lse = ops.bf16_fwd(qb.detach(), kb.detach(), vb.detach(), True)
    assert O.shape == qs and lse.shape == (qs[0] * qs[1], qs[2])
    dq, dk, dv = ops.bf16_bwd(qb.detach(), kb.detach(), vb.detach(), O, lse, True, _z(qs, torch.float32))
    assert dq.shape == qs and dk.shape == ks and dv.shape == ks and not dk.any() and not dv.any()
    torch.cuda.synchronize()


def _raises_without_allocating(exc, fn, *args, **kw):
    """``fn`` raises ``exc`` and the allocator's peak does not move: the refusal comes first."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    with pytest.raises(exc, match="empty key sequence"):
        fn(*args, **kw)
    assert torch.cuda.max_memory_allocated() == before


def test_empty_keys_refused(lib):
    """Sk = 0 with rows > 0: every public entry raises QAttnError and every ``torch.ops.qattn``
    operator RuntimeError, before anything is allocated.  (Every query keeps a key: an empty softmax
    has no value, and the JVP kernels would stage key tiles from an empty tensor.)"""
    from quantizedattention_amd import _lib, ops
    from quantizedattention_amd import attention_bf16 as A16
    from quantizedattention_amd import attention_int8 as A8
    from quantizedattention_amd import attention_jvp as AJ
    from quantizedattention_amd import attention_mxfp4 as A4
    E = _lib.QAttnError
    qs, ks = (1, 4, 64, 128), (1, 2, 0, 128)
    q, k, dO = _z(qs), _z(ks), _z(qs)
    vb = _z(ks, torch.bfloat16)
    for causal in (False, True):
        _raises_without_allocating(E, A8.sage_attention_3_int8, q, k, k, causal)
        _raises_without_allocating(E, A8.helion_atten_int8_hl_dot_fwd, q, k, k, causal=causal)
        _raises_without_allocating(E, A16.flash_atten_2_bf16, q, k, vb, causal)
        _raises_without_allocating(E, A16.helion_atten_bf16_fwd_training, q, k, vb, causal)
        _raises_without_allocating(E, A16.helion_flash_atten_2_algo_4_bwd, q, k, vb, _z(qs, torch.float32),
                                   _z((4, 64), torch.float32), causal, _z(qs, torch.float32))
        _raises_without_allocating(E, A4.mxfp4_attn_fwd, q, k, k, causal=causal)
        _raises_without_allocating(E, A4.sage_attention_3_fp4, q, k, k, causal=causal)
    # the int8 backward, on forward outputs of an empty key sequence's shapes
    qi, sq, lse = _z((256, 128), torch.int8), _z((8,)), _z((256,))
    kiT, vi, s0 = _z((128, 0), torch.int8), _z((0, 128), torch.int8), _z((0,))
    _raises_without_allocating(E, A8.helion_atten_int8_hl_dot_bwd, dO, qi, sq, kiT, None, s0, vi, s0, q, lse,
                               32, 32, kv_heads=2)
    _raises_without_allocating(E, A8._int8_backward, dO, qi, sq, kiT, s0, vi, s0, q, lse, kv_heads=2, use_ws=True)
    _raises_without_allocating(E, A8._int8_backward, dO, qi, sq, kiT, s0, vi, s0, q, lse, kv_heads=2, use_ws=False)
    for dt in (torch.bfloat16, torch.float32):
        x, y = _z(qs, dt), _z(ks, dt)
        _raises_without_allocating(E, AJ.helion_attention_jvp_forward_fp32, x, y, y, x, y, y)
        _raises_without_allocating(E, AJ.attention_jvp, x, y, y)
        _raises_without_allocating(E, AJ._jvp, x, y, y, None)
        _raises_without_allocating(RuntimeError, ops.jvp_fwd, x, y, y, x, y, y)
    R = RuntimeError
    _raises_without_allocating(R, ops.int8_fwd, q, k, k, True, False)
    _raises_without_allocating(R, ops.int8_fwd, q, k, k, False, True)
    _raises_without_allocating(R, ops.int8_bwd, dO, qi, sq, kiT.t(), s0, vi, s0, q, lse, False, 2)
    _raises_without_allocating(R, ops.bf16_fwd, q, k, vb, True)
    _raises_without_allocating(R, ops.bf16_bwd, q, k, vb, _z(qs, torch.float32), _z((4, 64), torch.float32), False,
                               _z(qs, torch.float32))
    _raises_without_allocating(R, ops.mxfp4_fwd, q, k, k)
    _raises_without_allocating(R, ops.mxfp4_fwd_ex, q, k, k, 1)
    torch.cuda.synchronize()


# C entries that take (bh, sq, sk): (pointer arguments before the sizes, the scalars after the sizes,
# pointer arguments after them, the stream excluded); D = 128, group 1, not causal
_QKS, _SMS = 0.1275174, 0.0883883
EMPTY_KEY_ENTRIES = {
    "qattn_int8_attn_fwd_ex": (8, (1, 0, 128, _QKS), 0),
    "qattn_int8_attn_fwd_qf": (10, (1, 0, 128, _QKS), 0),
    "qattn_int8_attn_bwd_ex": (15, (1, 0, 128, _QKS, _SMS), 0),
    "qattn_int8_attn_bwd_ws": (16, (1, 0, 128, _QKS, _SMS), 0),
    "qattn_bf16_fwd": (5, (128, 0, _QKS), 0),
    "qattn_bf16_fwd_ex": (5, (1, 0, 128, _QKS), 0),
    "qattn_bf16_fwd_ws_ex": (5, (1, 1, 128, _QKS), 1),
    "qattn_bf16_bwd": (10, (128, 0, _QKS, _SMS), 0),
    "qattn_bf16_bwd_ex": (10, (1, 0, 128, _QKS, _SMS), 0),
    "qattn_bf16_bwd_ws_ex": (10, (1, 1, 128, _QKS, _SMS), 1),
    "qattn_bf16_bwd_split_ex": (10, (1, 0, 128, _QKS, _SMS), 0),
    "qattn_jvp_fwd": (9, (128, 0, _QKS, _SMS), 0),
    "qattn_jvp_fwd_ex": (9, (1, 128, _QKS, _SMS), 0),
    "qattn_jvp_fwd_x3": (15, (128, _QKS, _SMS), 0),
    "qattn_jvp_fwd_x3_ex": (15, (1, 128, _QKS, _SMS), 0),
    "qattn_jvp_primal_ex": (5, (1, 128, _QKS, _SMS), 0),
    "qattn_jvp_primal_x3_ex": (8, (1, 128, _QKS, _SMS), 0),
    "qattn_mxfp4_attn_fwd_ex": (8, (1, 0, 128, _QKS), 0),
}


def test_empty_keys_status(lib):
    """The C entries called directly: status 1 for sk = 0 with rows > 0, status 0 (nothing to do) for
    bh = 0 or sq = 0, each decided before a pointer is read.  Every pointer names one 1 MiB buffer,
    several times the largest operand of these sizes (4 heads of 64 rows: 128 KiB of fp32 O; the 64 key
    rows a JVP stage reads: 16 KiB), so an entry that stopped refusing would show as a wrong status and
    a changed fill, not as an access out of range."""
    from quantizedattention_amd import _lib
    buf = torch.full((1 << 20,), 0x5A, dtype=torch.uint8, device="cuda")
    st = _lib.stream_of(buf)

    def status(name, bh, sq, sk):
        nptr, tail, nafter = EMPTY_KEY_ENTRIES[name]
        assert len(_lib.SIGNATURES[name]) == nptr + 3 + len(tail) + nafter + 1, name
        return getattr(lib, name)(*([_lib.ptr(buf)] * nptr), bh, sq, sk, *tail, *([_lib.ptr(buf)] * nafter), st)

    for name in EMPTY_KEY_ENTRIES:
        assert status(name, 4, 64, 0) == 1, name
        assert status(name, 0, 64, 0) == 0 and status(name, 4, 0, 0) == 0, name
        assert status(name, 0, 64, 64) == 0 and status(name, 4, 0, 64) == 0, name
    # the head-chunked record backward takes the chunk size before the sizes
    wsc = lambda bh, sq, sk: lib.qattn_int8_attn_bwd_wsc(*([_lib.ptr(buf)] * 16), 1, bh, sq, sk, 1, 0, 128,  # noqa: E731
                                                         _QKS, _SMS, st)
    assert wsc(4, 64, 0) == 1
    assert wsc(0, 64, 0) == 0 and wsc(4, 0, 0) == 0 and wsc(0, 64, 64) == 0 and wsc(4, 0, 64) == 0
    torch.cuda.synchronize()
    assert bool((buf == 0x5A).all())


def test_record_limits_status(lib):
    """The int8 record entries refuse the shapes whose per-tile LDS tables do not fit (the plan's
    limits, tests/test_plan.py::test_int8_plan_lds_tables) with status 1 before they launch.  Every
    pointer names one 64 MiB buffer, more than the largest operand of these shapes (8 heads of 8160
    rows: 16 MiB of bf16 images; 89632 keys: 22 MiB), so a lost refusal is a wrong status and a changed
    fill."""
    from quantizedattention_amd import _lib
    buf = torch.full((64 << 20,), 0x5A, dtype=torch.uint8, device="cuda")
    st, p = _lib.stream_of(buf), _lib.ptr(buf)
    for causal in (0, 1):
        tail = (causal, 128, _QKS, _SMS, st)
        assert lib.qattn_int8_attn_bwd_ws(*([p] * 16), 8, 8160, 128, 8, *tail) == 1       # 2040 query tiles
        assert lib.qattn_int8_attn_bwd_wsc(*([p] * 16), 1, 8, 8160, 128, 8, *tail) == 1
        assert lib.qattn_int8_attn_bwd_ws(*([p] * 16), 1, 32, 2801 * 32, 1, *tail) == 1   # 2801 key tiles
        assert lib.qattn_int8_attn_bwd_wsc(*([p] * 16), 1, 1, 32, 2801 * 32, 1, *tail) == 1
    torch.cuda.synchronize()
    assert bool((buf == 0x5A).all())


def test_zero_and_constant_inputs(lib):
    """All-zero q (every quantisation scale 0, indices 0): uniform softmax, O = the mean of v over the
    keys (within the int8 bar), lse = log2(Sk); a constant v gives O = v."""
    from quantizedattention_amd.attention_int8 import helion_atten_int8_hl_dot_fwd
    g = torch.Generator(device="cuda").manual_seed(41)
    S, D = 256, 128
    q = torch.zeros((1, 2, S, D), dtype=torch.float16, device="cuda")
    k = torch.randn((1, 2, S, D), device="cuda", generator=g).half()
    v = torch.randn((1, 2, S, D), device="cuda", generator=g).half()
    O, lse, qi, _, _, sq, *_ = helion_atten_int8_hl_dot_fwd(q, k, v)
    assert int(qi.abs().max()) == 0 and float(sq.abs().max()) == 0.0
    ref = v.float().mean(dim=2, keepdim=True).expand_as(v)
    assert (O.float() - ref).abs().max().item() <= 1e-2
    assert (lse.float() - 8.0).abs().max().item() <= 1e-2          # log2(256)
    # a constant v: exact attention gives 0.75; the reference's P_i8 truncation (trunc(127 e) with l
    # from the unquantised e) biases O low on peaked rows (q = k), so the bar is the oracle's
    from oracle import restate as R
    vc = torch.full_like(v, 0.75)
    O2 = helion_atten_int8_hl_dot_fwd(k, k, vc)[0].float().cpu()
    O2_ref = R.int8_fwd(k.cpu(), k.cpu(), vc.cpu())[0].float()
    assert (O2 - O2_ref).abs().max().item() <= 1e-2
    assert (O2 - 0.75).abs().max().item() <= (O2_ref - 0.75).abs().max().item() + 1e-2
    assert (O2 <= 0.75 + 1e-3).all()   # truncation only ever lowers P_i8


def test_large_magnitudes(lib):
    """fp16 inputs near the top of the fp16 range quantise without overflow (s = amax/127 stays
    finite) and the forward stays finite and within the int8 bar of the oracle."""
    from oracle import restate as R
    from quantizedattention_amd.attention_int8 import helion_atten_int8_hl_dot_fwd
    g = torch.Generator().manual_seed(42)
    q = (torch.randn((1, 1, 128, 128), generator=g) * 2000).clamp(-60000, 60000).half()
    k = (torch.randn((1, 1, 128, 128), generator=g) * 0.01).half()
    v = (torch.randn((1, 1, 128, 128), generator=g) * 3000).clamp(-60000, 60000).half()
    out = helion_atten_int8_hl_dot_fwd(q.cuda(), k.cuda(), v.cuda())
    ref = R.int8_fwd(q, k, v)
    for i in (2, 3, 4, 5, 6, 7):
        assert torch.equal(out[i].cpu(), ref[i]), i
    O = out[0].float().cpu()
    assert torch.isfinite(O).all()
    # relative bar: the 1e-2 absolute bar scaled by the magnitude of v
    assert (O - ref[0].float()).abs().max().item() <= 1e-2 * float(v.float().abs().max())


def test_decode_single_block_cache(lib):
    """A cache of exactly one 32-token block and 32 queries per head through the decoding path."""
    from quantizedattention_amd.attention_int8 import helion_atten_int8_hl_dot_fwd
    from quantizedattention_amd.kv_cache import attention_int8_cached, quantize_kv
    g = torch.Generator(device="cuda").manual_seed(43)
    q = torch.randn((2, 8, 32, 128), device="cuda", generator=g).half()
    k, v = (torch.randn((2, 2, 32, 128), device="cuda", generator=g).half() for _ in range(2))
    O, lse = attention_int8_cached(q, quantize_kv(k, v, smooth=False))
    ref = helion_atten_int8_hl_dot_fwd(q, k, v)
    assert torch.equal(O, ref[0]) and torch.equal(lse, ref[1])


@pytest.mark.parametrize("D,causal", [(128, False), (64, False), (128, True), (64, True)])
def test_running_max_moves_vs_oracle(lib, D, causal):
    """Keys whose scale grows along the sequence (and q = k, a peaked diagonal): the row max climbs
    by far more than the deferred-max threshold (8 in log2 units) from tile to tile, so the rare
    rescale branch runs on most tiles, including while the previous tile's P.V is in flight."""
    from oracle import restate as R
    from quantizedattention_amd import attention_int8 as A
    g = torch.Generator().manual_seed(44)
    S = 256
    ramp = (1.0 + torch.arange(S, dtype=torch.float32) / 24.0).view(1, 1, S, 1)
    k = (torch.randn((1, 2, S, D), generator=g) * ramp).half()
    for q in (k.clone(), (torch.randn((1, 2, S, D), generator=g) * 2.0).half()):
        v = torch.randn((1, 2, S, D), generator=g).half()
        out = A.helion_atten_int8_hl_dot_fwd(q.cuda(), k.cuda(), v.cuda(), causal=causal)
        ref = R.int8_fwd(q, k, v, causal=causal)
        for i in (2, 3, 4, 5, 6, 7):
            assert torch.equal(out[i].cpu(), ref[i]), i
        exact = _exact_attention(q, k, v, causal)
        d_ref = (out[0].float().cpu() - ref[0].float()).abs().max().item()
        e_ours = (out[0].float().cpu() - exact).abs().max().item()
        e_ref = (ref[0].float() - exact).abs().max().item()
        print(f"D={D} causal={causal}: |O-O_ref| {d_ref:.4f}  |O-exact| {e_ours:.4f}  "
              f"|O_ref-exact| {e_ref:.4f}")
        lse_x = _exact_lse2(q, k, causal)
        dl_ref = (out[1].float().cpu() - ref[1].float()).abs().max().item()
        el_ours = (out[1].float().cpu().reshape(-1) - lse_x).abs().max().item()
        el_ref = (ref[1].float().reshape(-1) - lse_x).abs().max().item()
        print(f"   lse: |l-l_ref| {dl_ref:.4f}  |l-exact| {el_ours:.4f}  |l_ref-exact| {el_ref:.4f}")
        # lse = f16(m + f16(log2 l)) (int8:252): within 2 fp16 steps of the oracle's, and never
        # further from exact than the oracle's
        ulp = 2.0 ** (math.floor(math.log2(max(1.0, ref[1].float().abs().max().item()))) - 10)
        lerr = (out[1].float().cpu() - ref[1].float()).abs()
        assert (lerr <= 2 * 2.0 ** -10 * ref[1].float().abs() + 1e-3).all(), dl_ref
        assert el_ours <= el_ref + 2 * ulp
        # Peaked rows (a handful of keys carry the row sum): a single P_i8 step weighs ~1/127 of the
        # row.  The tiles that can weigh that much take the reference's literal P chain (the vote of
        # csrc/int8_attn_fwd.hip), so O stays within the north star's 1e-2 of the
        # oracle here too (round 4, without the vote: 1.3e-2 .. 1.8e-2).
        assert d_ref <= 1e-2
        assert e_ours <= e_ref + 1e-2


def _ramp_inputs(shape, seed, kscale=24.0):
    """q random, k scaled by a ramp along the keys (the row max climbs tile after tile), v random."""
    B, H, S, D = shape
    g = torch.Generator().manual_seed(seed)
    ramp = (1.0 + torch.arange(S, dtype=torch.float32) / kscale).view(1, 1, S, 1)
    q = torch.randn(shape, generator=g)
    k = torch.randn(shape, generator=g) * ramp
    v = torch.randn(shape, generator=g)
    return q, k, v


def test_bf16_running_max_moves_vs_oracle(lib):
    """The bf16 forward (exact running-max rule, rescale on every move, the reference's beta rule)
    on a climbing row max, causal.  The beta rule compares raw scores with the scaled max
    (bf16:248) and doubles m when two raw scores pass it; on these inputs it fires on most late
    tiles, and whether it fires hinges on single bf16 steps of S (ties M2 == thr on the bf16 grid),
    which the fp32 accumulation order of the S product can move -- the oracle's CPU matmul and the
    MFMA sum in different orders, as the reference's own GPU kernel would.  A flipped decision
    changes m by 2x from then on (and can push every P of the row below the fp32 denormal range,
    which v_exp_f32 flushes: l = 0).  Bar: >= 95 % of the rows within 5e-3 of the oracle (measured:
    501 of 512); non-causal, the doublings overflow m and the oracle itself turns NaN."""
    from oracle import restate as R
    from quantizedattention_amd.attention_bf16 import helion_atten_bf16_fwd_training
    q, k, v = _ramp_inputs((1, 2, 256, 128), 45, kscale=96.0)
    q, k, v = q.half(), k.half(), v.bfloat16()
    O_ref, lse_ref = R.bf16_fwd(q, k, v, True, kt=16)
    assert torch.isfinite(O_ref).all()
    O, lse = helion_atten_bf16_fwd_training(q.cuda(), k.cuda(), v.cuda(), True)
    D = O.shape[-1]
    e_O = (O.cpu().view(-1, D) - O_ref.view(-1, D)).abs().max(-1).values
    e_l = (lse.cpu().view(-1) - lse_ref.view(-1)).abs()
    ok = (e_O <= 5e-3) & (e_l <= 5e-3)    # (NaN compares False)
    print(f"rows {ok.numel()}, matching the oracle {int(ok.sum())}")
    assert int(ok.sum()) >= 0.95 * ok.numel()


@pytest.mark.parametrize("fp32", [True, False])
def test_jvp_running_max_moves(lib, fp32):
    """The JVP forward's deferred running max (moves only past 8 log2 units) on a climbing row max,
    vs torch.func.jvp of the fp32 baseline.  Bars from the operand precision (these logits reach
    |S| ~ 45, far past the random inputs of tests/test_gpu_jvp.py): the fp32 mode's products carry
    the 2^-16 relative residual of the hi/lo split, so O and tO move by up to 2^-16 max|S| max|v|
    (resp. max|tv| + max|tS| max|v|); the bf16 mode rounds P and H = P tS to bf16 (2^-9), which
    moves tO by up to 2^-9 max|tS| max|v| (measured 0.33 at max|tO| = 51)."""
    from oracle import restate as R
    from quantizedattention_amd.attention_jvp import helion_attention_jvp_forward_fp32
    q, k, v = _ramp_inputs((1, 2, 256, 128), 46, kscale=16.0)
    g = torch.Generator().manual_seed(47)
    tq, tk, tv = (torch.randn(q.shape, generator=g) for _ in range(3))
    if not fp32:
        q, k, v, tq, tk, tv = (t.bfloat16().float() for t in (q, k, v, tq, tk, tv))
    dt = torch.float32 if fp32 else torch.bfloat16
    O, tO, lse = helion_attention_jvp_forward_fp32(*(t.cuda().to(dt) for t in (q, k, v, tq, tk, tv)))
    Ot, tOt = R.jvp_truth(q, k, v, tq, tk, tv)
    sm = q.shape[-1] ** -0.5
    s_max = (q.abs() @ k.abs().transpose(-1, -2)).max().item() * sm
    ts_max = ((tq @ k.transpose(-1, -2) + q @ tk.transpose(-1, -2)) * sm).abs().max().item()
    vm, tvm = v.abs().max().item(), tv.abs().max().item()
    e_O = (O.cpu() - Ot).abs().max().item()
    e_tO = (tO.cpu() - tOt).abs().max().item()
    print(f"fp32={fp32}: |O err| {e_O:.3g}  |tO err| {e_tO:.3g}  max|S| {s_max:.1f}  max|tS| {ts_max:.1f}")
    if fp32:
        assert e_O <= 2.0 ** -16 * s_max * vm
        assert e_tO <= 2.0 ** -16 * s_max * (tvm + ts_max * vm)
    else:
        assert e_O <= 1e-2
        assert e_tO <= 2.0 ** -9 * ts_max * vm


def test_mxfp4_running_max_moves_vs_oracle(lib):
    """The MX-FP4 forward's integer running max (raised past MSLACK) on a climbing row max."""
    from oracle import mxfp4 as M
    from quantizedattention_amd.attention_mxfp4 import mxfp4_attn_fwd
    q, k, v = (t.half() for t in _ramp_inputs((1, 2, 128, 128), 48, kscale=12.0))
    O, lse, ops = mxfp4_attn_fwd(q.cuda(), k.cuda(), v.cuda(), smooth_k=False)
    RO, Rl, rops = M.mxfp4_fwd(q, k, v)
    for a, b in zip(ops, rops):
        assert torch.equal(a.cpu().reshape(b.shape), b)
    assert (O.float().cpu() - RO.float()).abs().max().item() <= 2e-2
    assert (lse.cpu() - Rl).abs().max().item() <= 1e-4 * max(1.0, Rl.abs().max().item())


def test_workspace_refusal_is_remembered(lib, monkeypatch):
    """A backward workspace the allocator refuses is not requested again (each refusal flushes the
    caching allocator) until the device has room for it; smaller ones still are."""
    from quantizedattention_amd import _lib
    dev = torch.device("cuda", torch.cuda.current_device())
    _lib._WS_REFUSED.pop(dev.index, None)
    huge = 1 << 46                     # 64 TiB: refused by any allocator
    assert _lib.try_workspace(huge, dev) is None
    assert _lib._WS_REFUSED[dev.index] == huge
    calls = []
    orig = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, **kw: calls.append(a) or orig(*a, **kw))
    assert _lib.try_workspace(huge, dev) is None and not calls      # not asked again
    ws = _lib.try_workspace(1 << 20, dev)                            # a smaller one is
    assert ws is not None and ws.numel() == 1 << 20 and len(calls) == 1
    _lib._WS_REFUSED.pop(dev.index, None)
