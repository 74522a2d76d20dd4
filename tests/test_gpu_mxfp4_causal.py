"""Causal MX-FP4 forward on the GPU (qattn_mxfp4_attn_fwd_ex, mxfp4_attn_fwd(causal=),
mxfp4_attn_fwd_kv, qattn::mxfp4_fwd_ex) against the masked restatement tests/mxfp4_masked_ref.py.

Bars of the kernel against the restatement are those of tests/test_gpu_mxfp4.py (operands
bit-exact, O max-abs <= 2e-2 and relL2 <= 2e-3, lse <= 1e-4), on every row: measured on an
MI355X, O equals the restatement's in every element and lse is within 9.6e-7, the rows that see
fewer than 64 keys included (printed as "MXFP4-CAUSAL ...").  The bit-identity tests (chunk
identity, huge masked keys, causal = 0) hold whatever the tolerance: they are what catches a wrong
per-wave tile bound or a masked key that leaks into a row max or a P block.
"""
import math

import pytest
import torch

import mxfp4_masked_ref as MR
from oracle import mxfp4 as M

pytestmark = pytest.mark.gpu

HUGE = 60000.0


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-30)).item()


def _fwd(q, k, v, causal, smooth_k=False):
    from quantizedattention_amd.attention_mxfp4 import mxfp4_attn_fwd
    O, lse, ops = mxfp4_attn_fwd(q.cuda(), k.cuda(), v.cuda(), smooth_k=smooth_k, causal=causal)
    torch.cuda.synchronize()
    return O, lse, ops


@pytest.mark.parametrize("case", MR.CASES)
def test_kernel_vs_masked_restatement(lib, case):
    B, H, Hkv, Sq, Sk, causal = case
    q, k, v, RO, Rl, rops = MR.case_reference(case)
    O, lse, ops = _fwd(q, k, v, causal)
    for a, b in zip(ops, rops):
        assert torch.equal(a.cpu().reshape(b.shape), b)
    assert O.shape == (B, H, Sq, 128) and lse.shape == (B * H, Sq)
    O, lse = O.float().cpu(), lse.cpu()
    assert torch.isfinite(O).all() and torch.isfinite(lse).all()
    d = (O - RO.float()).abs()
    err, rel, lerr = d.max().item(), _rel(O, RO), (lse - Rl).abs().max().item()
    # the same figures over the rows that see fewer than 64 keys (none of the bidirectional
    # kernel's rows do), for the record
    few = (torch.arange(Sq) + MR.key_offset(causal, Sq, Sk) + 1).clamp(max=Sk) < 64
    ferr = d[:, :, few].max().item() if few.any() else 0.0
    flerr = (lse - Rl)[:, few].abs().max().item() if few.any() else 0.0
    print(f"MXFP4-CAUSAL {tuple(case[:5])} causal={causal} maxabs {err:.3e} relL2 {rel:.3e} lse {lerr:.3e}"
          f" | rows<64keys: {int(few.sum())} maxabs {ferr:.3e} lse {flerr:.3e}")
    assert err <= 2e-2, err
    assert rel <= 2e-3, rel
    assert lerr <= 1e-4, lerr


def test_ex_causal0_is_the_plain_entry(lib):
    from quantizedattention_amd import _lib
    from quantizedattention_amd.attention_mxfp4 import _qk_scale, mxfp4_attn_fwd
    q, k, v = (t.cuda() for t in MR.randn_qkv((2, 4, 2, 96, 256)))
    O, lse, ops = mxfp4_attn_fwd(q, k, v)
    outs = []
    for name, extra in (("qattn_mxfp4_attn_fwd", ()), ("qattn_mxfp4_attn_fwd_ex", (0,))):
        o, l = torch.full_like(O, float("nan")), torch.full_like(lse, float("nan"))
        _lib.call(name, *(_lib.ptr(t) for t in ops), _lib.ptr(o), _lib.ptr(l), 8, 96, 256, 2, *extra, 128,
                  _qk_scale(128), _lib.stream_of(q))
        outs.append((o, l))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(outs[0][0], O) and torch.equal(outs[0][1], lse)
    O0, lse0, _ = mxfp4_attn_fwd(q, k, v, causal=False)
    assert torch.equal(O0, O) and torch.equal(lse0, lse)


def test_chunk_identity(lib):
    """A query chunk against the quantised K/V of the whole prefill (causal = 2) reproduces the
    prefill's rows bit for bit: tile skipping and the per-wave bounds change nothing."""
    from quantizedattention_amd.attention_mxfp4 import mxfp4_attn_fwd_kv
    q, k, v = (t.cuda() for t in MR.randn_qkv((1, 2, 2, 256, 256)))
    O1, l1, ops = _fwd(q, k, v, 1)
    kv = ops[2:]
    O2, l2 = mxfp4_attn_fwd_kv(q[:, :, 160:], kv, causal=2)
    assert torch.equal(O2, O1[:, :, 160:]) and torch.equal(l2, l1[:, 160:])
    O3, l3 = mxfp4_attn_fwd_kv(q, kv, causal=1)
    assert torch.equal(O3, O1) and torch.equal(l3, l1)


def test_kv_entry_with_smoothed_cache_and_gqa(lib):
    """mxfp4_attn_fwd_kv reads Hkv and Sk from vt; a smoothed cache is queried as it is."""
    from quantizedattention_amd.attention_mxfp4 import mxfp4_attn_fwd_kv
    q, k, v = (t.cuda() for t in MR.randn_qkv((2, 4, 2, 96, 256)))
    O1, l1, ops = _fwd(q, k, v, 2, smooth_k=True)
    O2, l2 = mxfp4_attn_fwd_kv(q, ops[2:], causal=2)
    assert torch.equal(O2, O1) and torch.equal(l2, l1)


def test_later_tiles_are_ignored(lib):
    q, k, v = MR.randn_qkv((1, 2, 2, 128, 256))
    O, lse, _ = _fwd(q, k, v, 1)
    k2, v2 = k.clone(), v.clone()
    k2[:, :, 128:] = HUGE
    v2[:, :, 128:] = HUGE
    O2, lse2, _ = _fwd(q, k2, v2, 1)
    assert torch.equal(O2, O) and torch.equal(lse2, lse)
    assert torch.isfinite(O2.float()).all() and torch.isfinite(lse2).all()


def test_masked_keys_in_the_own_tile_are_ignored(lib):
    q, k, v = MR.randn_qkv((1, 2, 2, 128, 128))
    O, lse, _ = _fwd(q, k, v, 1)
    k2 = k.clone()
    k2[:, :, 32:64] = HUGE
    O2, lse2, _ = _fwd(q, k2, v, 1)
    assert torch.equal(O2[:, :, :32], O[:, :, :32]) and torch.equal(lse2[:, :32], lse[:, :32])
    assert torch.isfinite(O2.float()).all() and torch.isfinite(lse2).all()


def _units(n):
    """32 values, each 0, 1, 2, 3, 4, 6 or 8, that sum to n (8 <= n <= 256) and hold an 8: one MX
    block whose scale makes 1 the half-step of its e2m1 grid, so every value is a code."""
    assert 8 <= n <= 256
    vals = [8] * (n // 8)
    r = n % 8
    vals += {0: [], 5: [4, 1], 7: [6, 1]}.get(r, [r])
    assert len(vals) <= 32 and sum(vals) == n
    return torch.tensor(vals + [0] * (32 - len(vals)), dtype=torch.float32)


def test_smallest_problem_row0_sees_one_key(lib):
    """causal = 1, Sq = 32, Sk = 64.  Row 0 sees key 0 alone, so O[0] is the dequantised V row 0.
    lse[0] = m + log2(l) with l the *quantised* P (the definition: l adds what the matrix core
    adds), so it equals S00 * qks only where P = exp2(S00 * qks - m) is an fp4 value.  Row 0 of q
    is therefore built from fp4-exact values whose product with a key row of ones is
    S00 = K / 4096 with K = ceil(4096 / qks): S00 * qks exceeds 1 by less than 4e-5, so m = 2 and
    P = 0.5 + a little, which is code 4 at scale 2^-3 = 0.5, and lse[0] = 1.  (Just below 1 it
    would be m = 1, P = 1 - a little, which saturates to 6 * 2^-3.)  The other rows are random."""
    qks = M.qk_scale(128)
    K = math.ceil(4096 / qks)
    q, k, v = MR.randn_qkv((1, 1, 1, 32, 64), seed=7)
    q[0, 0, 0] = 0.0
    q[0, 0, 0, :32] = (_units(K % 128) * 2.0 ** -12).half()
    q[0, 0, 0, 32:64] = (_units(K // 128) * 2.0 ** -5).half()
    k[0, 0, 0] = 1.0
    O, lse, ops = _fwd(q, k, v, 1)
    q4, qs, k4, ks, vt, vs = (t.cpu() for t in ops)
    s00 = (M.deq_rows(q4, qs)[0] * M.deq_rows(k4.reshape(64, 64), ks.reshape(64, 4))[0]).sum().item()
    assert s00 == K / 4096 and 0.0 < s00 * qks - 1.0 <= 4e-5, (s00, K)      # the construction
    v0 = M.deq_vt(vt, vs)[0, 0].float()
    assert (O[0, 0, 0].float().cpu() - v0).abs().max().item() <= 1e-3
    assert abs(lse[0, 0].item() - s00 * qks) <= 1e-4, (lse[0, 0].item(), s00 * qks)
    RO, Rl, _ = MR.mxfp4_fwd_masked(q, k, v, 1)
    assert (O.float().cpu() - RO.float()).abs().max().item() <= 2e-2
    assert (lse.cpu() - Rl).abs().max().item() <= 1e-4


@pytest.mark.parametrize("Sq,Sk,causal", [(512, 512, True), (256, 512, 2)])
def test_sage_attention_3_fp4_causal_accuracy(lib, Sq, Sk, causal):
    """End to end with k smoothing, vs exact masked fp32 attention."""
    from quantizedattention_amd.attention_mxfp4 import sage_attention_3_fp4
    q, k, v = MR.accuracy_inputs(Sq, Sk)
    O = sage_attention_3_fp4(q.cuda(), k.cuda(), v.cuda(), causal=causal)
    cos = MR.cosine(O.cpu(), MR.exact_masked_attention(q, k, v, int(causal)))
    print(f"MXFP4-CAUSAL e2e ({Sq},{Sk}) causal={int(causal)} cos {cos:.4f}")
    assert cos >= 0.95, cos


def test_operator_matches_dropin_and_compiles(lib):
    import quantizedattention_amd.ops as ops
    from quantizedattention_amd.attention_mxfp4 import sage_attention_3_fp4
    q, k, v = (t.cuda() for t in MR.randn_qkv((2, 4, 2, 96, 256)))
    for c in (0, 1, 2):
        O = torch.ops.qattn.mxfp4_fwd_ex(q, k, v, c)
        assert torch.equal(O, sage_attention_3_fp4(q, k, v, causal=c)), c
        assert torch.equal(O, ops.mxfp4_fwd_ex(q, k, v, c)), c
    assert torch.equal(torch.ops.qattn.mxfp4_fwd_ex(q, k, v, 0), torch.ops.qattn.mxfp4_fwd(q, k, v))

    def f(q, k, v):
        return torch.ops.qattn.mxfp4_fwd_ex(q, k, v, 2).float() * 2.0

    cf = torch.compile(f, backend="eager", fullgraph=True)
    assert torch.equal(cf(q, k, v), f(q, k, v))


def test_refusals(lib):
    from quantizedattention_amd import _lib
    from quantizedattention_amd.attention_mxfp4 import (_qk_scale, mxfp4_attn_fwd, mxfp4_attn_fwd_kv,
                                                        sage_attention_3_fp4)
    q = torch.zeros((1, 2, 128, 128), dtype=torch.float16, device="cuda")
    kk = q[:, :, :64]
    with pytest.raises(_lib.QAttnError):
        mxfp4_attn_fwd(q, kk, kk, causal=2)                          # Sq > Sk, bottom-right
    with pytest.raises(_lib.QAttnError):
        mxfp4_attn_fwd(q, q, q, causal=3)
    with pytest.raises(_lib.QAttnError):
        sage_attention_3_fp4(q, q[:, :, :48], q[:, :, :48], causal=True)   # Sk % 64
    with pytest.raises(_lib.QAttnError):
        mxfp4_attn_fwd(q[..., :64], q[..., :64], q[..., :64], causal=1)   # head_dim 64
    O, lse, ops = mxfp4_attn_fwd(q, kk, kk, causal=1)               # top-left allows Sq > Sk
    with pytest.raises(_lib.QAttnError):
        mxfp4_attn_fwd_kv(q, ops[2:], causal=2)
    with pytest.raises(_lib.QAttnError):
        mxfp4_attn_fwd_kv(q, ops[2:], causal=3)
    fn = lib.qattn_mxfp4_attn_fwd_ex
    args = lambda sq, sk, c: ([_lib.ptr(t) for t in ops] + [_lib.ptr(O), _lib.ptr(lse), 2, sq, sk, 1, c,  # noqa: E731
                                                          128, _qk_scale(128), _lib.stream_of(q)])
    assert fn(*args(128, 64, 2)) == 1
    assert fn(*args(128, 64, 3)) == 1
    assert fn(*args(128, 64, -1)) == 1
    assert fn(*args(128, 64, 1)) == 0
    torch.cuda.synchronize()
