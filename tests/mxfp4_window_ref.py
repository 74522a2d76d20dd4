"""CPU restatement of the windowed packed step (csrc/mxfp4_attn.hip, mxfp4_attn_split_kernel with
WINDOW; kv_cache_mxfp4.attention_mxfp4_varlen_paged(window=, sinks=)).

TEST INFRASTRUCTURE ONLY.  Built from the pieces of ``oracle/mxfp4.py`` as
``mxfp4_ragged_ref.sequence_partials`` is, whose tile body it runs.  One sequence of L keys and Sq queries,
the sequence's last Sq positions: query i sits at p = L - Sq + i and sees key k iff

    k <= p  and  (k > p - W  or  k < S)

The splits are those of the kernel.  With nt = ceil(L / 64), T = kps / 64, wt0 = max(0, L - Sq - W + 1) //
64 and nst = ceil(min(S, L) / 64):

    wt0 <= nst   split s runs the tiles [s T, min(nt, s T + T)), ns = ceil(nt / T)
    wt0 >  nst   split 0 runs the sink tiles [0, nst); split s >= 1 the tiles [wt0 + (s-1) T, min(nt, wt0 +
                 s T)); ns = 1 + ceil((nt - wt0) / T).  Without sinks (nst = 0) there is no sink split:
                 split s runs [wt0 + s T, ..) and ns = ceil((nt - wt0) / T)

each from m = -inf; a row that sees no key of a split keeps (-inf, 0, 0).  The merge is
``mxfp4_split_ref.merge`` (float64).
"""
from __future__ import annotations

import torch

import mxfp4_ragged_ref as RR
import mxfp4_split_ref as SR
from oracle import mxfp4 as M


def visible(Sq: int, L: int, Skp: int, W: int, S: int) -> torch.Tensor:
    """bool [Sq, Skp]"""
    assert Sq <= L and W >= 1 and S >= 0
    k = torch.arange(Skp)[None, :]
    p = torch.arange(Sq)[:, None] + (L - Sq)
    return (k <= p) & ((k > p - W) | (k < S))


def split_tiles(L: int, Sq: int, W: int, S: int, kps: int) -> list:
    """The tile range [first, last) of every split of the sequence."""
    nt, T = -(-L // 64), kps // 64
    wt0, nst = max(0, L - Sq - W + 1) // 64, -(-min(S, L) // 64)
    if wt0 <= nst:
        return [(t, min(nt, t + T)) for t in range(0, nt, T)]
    return [(0, nst)] * (nst > 0) + [(t, min(nt, t + T)) for t in range(wt0, nt, T)]


def sequence_partials(q, k, v, W, S, kps, nsplit=None, mslack=8.0):
    """One sequence: q fp16 [1, H, Sq, D], k, v fp16 [1, Hkv, L, D] (any L >= Sq) -> (m [ns, H, Sq], l
    [ns, H, Sq], O [ns, H, Sq, D], float64).  ``nsplit`` > ns appends empty splits (-inf, 0, 0)."""
    _, H, Sq, D = q.shape
    Hkv, L = k.shape[1], k.shape[2]
    k, v = RR.pad64(k), RR.pad64(v)
    Skp = k.shape[2]
    qks = M.qk_scale(D)
    q4, qs = M.quant_rows(q.reshape(H * Sq, D))
    k4, ks = M.quant_rows(k.reshape(Hkv * Skp, D))
    vt, vs = M.quant_vt(v.reshape(Hkv, Skp, D))
    kvh = torch.arange(H) // (H // Hkv)
    dq = M.deq_rows(q4, qs).reshape(H, Sq, D)
    dk = M.deq_rows(k4, ks).reshape(Hkv, Skp, D)[kvh]
    dv = M.deq_vt(vt, vs)[kvh]
    vis_all = visible(Sq, L, Skp, W, S)
    order = M.vt_key_order()
    ranges = split_tiles(L, Sq, W, S, kps)
    ranges += [(0, 0)] * ((nsplit or 0) - len(ranges))
    ms, ls, Os = [], [], []
    for t_lo, t_hi in ranges:
        m = torch.full((H, Sq, 1), float("-inf"), dtype=torch.float64)
        l = torch.zeros((H, Sq, 1), dtype=torch.float64)
        O = torch.zeros((H, Sq, D), dtype=torch.float64)
        for k0 in range(64 * t_lo, 64 * t_hi, 64):
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
            Pd = torch.zeros((H, Sq, 64), dtype=torch.float64)
            Pd[..., order] = M.decode(codes) * M.scale_value(b)[..., None]
            l = l + Pd.sum(-1, keepdim=True)
            O = O + Pd @ dv[:, k0:k0 + 64]
        ms.append(m.squeeze(-1))
        ls.append(l.squeeze(-1))
        Os.append(O)
    return torch.stack(ms), torch.stack(ls), torch.stack(Os)


def mxfp4_fwd_window(q, k, v, W, S, kps, nsplit=None):
    """One sequence -> (O fp16 [1, H, Sq, D], lse fp32 [H, Sq], (m, l) of the partials)."""
    kps = min(int(kps), RR.ceil64(k.shape[2]))
    m, l, O = sequence_partials(q, k, v, W, S, kps, nsplit)
    Oh, lse = SR.merge(m, l, O)
    return Oh.view(q.shape), lse, (m, l)


def dense_reference(q, k, v, W, S):
    """float64 softmax attention with the window mask on the DEQUANTISED operands of one sequence ->
    (O [1, H, Sq, D], lse base 2 [H, Sq])."""
    _, H, Sq, D = q.shape
    Hkv, L = k.shape[1], k.shape[2]
    kp, vp = RR.pad64(k), RR.pad64(v)
    Skp = kp.shape[2]
    q4, qs = M.quant_rows(q.reshape(H * Sq, D))
    k4, ks = M.quant_rows(kp.reshape(Hkv * Skp, D))
    vt, vs = M.quant_vt(vp.reshape(Hkv, Skp, D))
    kvh = torch.arange(H) // (H // Hkv)
    dq = M.deq_rows(q4, qs).reshape(H, Sq, D).double()
    dk = M.deq_rows(k4, ks).reshape(Hkv, Skp, D)[kvh].double()
    dv = M.deq_vt(vt, vs)[kvh].double()
    s = (dq @ dk.transpose(1, 2)) * M.qk_scale(D)
    s = s.masked_fill(~visible(Sq, L, Skp, W, S)[None], float("-inf"))
    mx = s.amax(-1, keepdim=True)
    p = torch.exp2(s - mx)
    lsum = p.sum(-1, keepdim=True)
    return ((p / lsum) @ dv)[None], (mx + torch.log2(lsum)).squeeze(-1)
