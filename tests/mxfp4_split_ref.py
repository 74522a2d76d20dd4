"""CPU restatement of the key-split MX-FP4 forward (csrc/mxfp4_attn.hip, "key-split forward").

TEST INFRASTRUCTURE ONLY.  Built from the pieces of ``oracle/mxfp4.py`` like
``mxfp4_masked_ref.mxfp4_fwd_masked``, whose tile loop it runs once per split, from m = -inf, over
the keys [s * kps, min(Sk, s * kps + kps)); a row that sees no key of a split keeps m = -inf, l = 0,
O = 0 (its P is selected to 0: exp2(S - (-inf)) is inf).  The merge is float64:

    M = max_s m_s;  w_s = 2^(m_s - M) (0 for m_s = -inf);  L = sum_s w_s l_s
    O = f16((sum_s w_s O_s) / L);  lse = f32(M + log2 L)

Every m_s is an integer, so the weights are exact and the split result equals the one-pass one up to
the order of the float64 additions.
"""
from __future__ import annotations

import functools

import torch

import mxfp4_masked_ref as MR
from oracle import mxfp4 as M

# (B, Hq, Hkv, Sq, Sk, causal, keys per split): rows 4 / 4 / 66 / 130 / 32 / 192 / 5 per key/value head
CASES = [(1, 4, 1, 1, 256, 0, 64), (2, 8, 2, 1, 320, 0, 128), (1, 2, 1, 33, 256, 0, 64),
         (1, 4, 2, 65, 192, 0, 64), (1, 4, 1, 8, 256, 2, 64), (1, 2, 1, 96, 256, 2, 64),
         (1, 2, 2, 5, 128, 2, 64)]


def inputs(case, qmul=1):
    B, H, Hkv, Sq, Sk, causal, kps = case
    q, k, v = MR.randn_qkv((B, H, Hkv, Sq, Sk), seed=2)
    if qmul != 1:
        q = (q.float() * qmul).half()
    return q, k, v


def split_partials(q, k, v, causal, kps, mslack=8.0):
    """-> (m [ns, BH, Sq], l [ns, BH, Sq], O [ns, BH, Sq, D], all float64; operands)."""
    B, H, Sq, D = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
    G = H // Hkv
    BH = B * H
    qks = M.qk_scale(D)
    q4, qs = M.quant_rows(q.reshape(BH * Sq, D))
    k4, ks = M.quant_rows(k.reshape(B * Hkv * Sk, D))
    vt, vs = M.quant_vt(v.reshape(B * Hkv, Sk, D))
    kvh = torch.arange(BH) // G
    dq = M.deq_rows(q4, qs).reshape(BH, Sq, D)
    dk = M.deq_rows(k4, ks).reshape(B * Hkv, Sk, D)[kvh]
    dv = M.deq_vt(vt, vs)[kvh]
    vis_all = MR.visible_mask(int(causal), Sq, Sk)
    order = M.vt_key_order()
    ms, ls, Os = [], [], []
    for k_lo in range(0, Sk, kps):
        m = torch.full((BH, Sq, 1), float("-inf"), dtype=torch.float64)
        l = torch.zeros((BH, Sq, 1), dtype=torch.float64)
        O = torch.zeros((BH, Sq, D), dtype=torch.float64)
        for k0 in range(k_lo, min(Sk, k_lo + kps), 64):
            vis = vis_all[None, :, k0:k0 + 64]
            acc = (dq @ dk[:, k0:k0 + 64].transpose(1, 2)).to(torch.float32)
            mx = (acc * qks).masked_fill(~vis, float("-inf")).amax(-1, keepdim=True).double()
            raise_ = mx > m + mslack
            nm = torch.where(raise_, torch.ceil(mx), m)
            r = torch.where(torch.isinf(m), torch.zeros_like(m), torch.pow(2.0, m - nm))
            O, l, m = O * r, l * r, nm
            P = torch.exp2((acc.double() * qks - m).to(torch.float32))
            P = torch.where(vis & ~torch.isinf(m), P, torch.zeros_like(P))   # empty rows: P = 0
            codes, b = M.quant_block32(P[..., order])
            Pd = torch.zeros((BH, Sq, 64), dtype=torch.float64)
            Pd[..., order] = M.decode(codes) * M.scale_value(b)[..., None]
            l = l + Pd.sum(-1, keepdim=True)
            O = O + Pd @ dv[:, k0:k0 + 64]
        ms.append(m.squeeze(-1))
        ls.append(l.squeeze(-1))
        Os.append(O)
    return torch.stack(ms), torch.stack(ls), torch.stack(Os), (q4, qs, k4, ks, vt, vs)


def merge(m, l, O):
    """float64 merge of the partials -> (O fp16 [BH, Sq, D], lse fp32 [BH, Sq])."""
    Mx = m.amax(0)
    w = torch.where(torch.isinf(m), torch.zeros_like(m), torch.pow(2.0, m - Mx))
    L = (w * l).sum(0)
    Om = (w[..., None] * O).sum(0) / L[..., None]
    return Om.to(torch.float16), (Mx + torch.log2(L)).to(torch.float32)


def merge_bits(opart, ml):
    """The kernels' merge (csrc/mxfp4_attn.hip mx_merge_row) restated bit for bit on the CPU: fp32
    ``opart`` [ns, R, D] and ``ml`` [ns, R, 2] = {m_s, l_s} -> (O fp16 [R, D], differs bool [R, D], lse fp32
    [R]).  In fp32: M = max_s m_s; w_s = 2^(m_s - M), 0 for m_s = -inf; L = w_s * l_s + L and acc = w_s *
    O_s + acc over the splits in order, a multiply and then an add -- w_s is a power of two, so the product
    is exact and this is the kernel's fmaf (as long as no product is subnormal); inv = 1 / L, correctly
    rounded.  Then the conversion as the kernel defines it: a column c with c % 8 in (0, 7) is the exact
    product acc * inv (float64 holds it) rounded to fp16 ONCE, by numpy -- torch's float64 -> float16 goes
    through float32 on the CPU -- and every other column is the fp32 product, rounded, then converted.
    ``differs`` marks the elements where the two forms disagree, whichever the column takes; ``lse`` is
    M + log2(L) in float64, for a tolerance."""
    import numpy as np
    opart, ml = opart.detach().float().cpu(), ml.detach().float().cpu()
    ns, R, D = opart.shape
    m, l = ml[..., 0], ml[..., 1]
    Mx = m.amax(0)
    gone = torch.isinf(m)
    e = torch.where(gone, torch.zeros_like(m), m - Mx).to(torch.int32)
    w = torch.where(gone, torch.zeros_like(m), torch.ldexp(torch.ones_like(m), e))
    L = torch.zeros(R, dtype=torch.float32)
    acc = torch.zeros((R, D), dtype=torch.float32)
    for s in range(ns):
        L = w[s] * l[s] + L
        acc = w[s][:, None] * opart[s] + acc
    inv = 1.0 / L
    twice = (acc * inv[:, None]).to(torch.float16)
    once = torch.from_numpy((acc.double().numpy() * inv.double().numpy()[:, None]).astype(np.float16))
    col = torch.arange(D) % 8
    out = torch.where(((col == 0) | (col == 7))[None, :], once, twice)
    differs = once.view(torch.int16) != twice.view(torch.int16)
    return out, differs, (Mx.double() + torch.log2(L.double())).to(torch.float32)


def merge_partials(seed, nsplit, R, D=128):
    """Random partials of R rows -> (opart fp32 [nsplit, R, D], ml fp32 [nsplit, R, 2]): O_s = 40 randn, m_s
    integers in [-3, 3] with every seventh row of split 0 at -inf (every row keeps a finite m), l_s in
    [1, 61)."""
    g = torch.Generator().manual_seed(seed)
    opart = 40 * torch.randn((nsplit, R, D), generator=g)
    m = torch.randint(-3, 4, (nsplit, R), generator=g).float()
    m[0, ::7] = float("-inf")
    l = 1 + 60 * torch.rand((nsplit, R), generator=g)
    return opart, torch.stack([m, l], -1).contiguous()


@functools.lru_cache(maxsize=None)
def merge_case(seed=0, nsplit=3, R=2048):
    """``merge_partials`` on which the two conversions of :func:`merge_bits` differ in both kinds of
    column (tests/test_mxfp4_cache_ref.py), with their merge, computed once per session; do not modify ->
    (opart, ml, O, differs, lse)."""
    opart, ml = merge_partials(seed, nsplit, R)
    return (opart, ml) + merge_bits(opart, ml)


def mxfp4_fwd_split(q, k, v, causal, kps):
    """-> (O fp16 [B,H,Sq,D], lse fp32 [B*H,Sq], operands, (m, l) of the partials)."""
    m, l, O, ops = split_partials(q, k, v, causal, kps)
    Oh, lse = merge(m, l, O)
    return Oh.view(q.shape), lse, ops, (m, l)


@functools.lru_cache(maxsize=None)
def case_reference(case, qmul=1):
    """(q, k, v, O, lse, operands) of the ONE-PASS restatement for one of CASES, computed once per
    session; do not modify.  (tests/test_mxfp4_cache_ref.py shows the split restatement equals it.)"""
    q, k, v = inputs(case, qmul)
    return (q, k, v) + MR.mxfp4_fwd_masked(q, k, v, case[5])
