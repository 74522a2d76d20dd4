"""CPU restatement of logit soft-capping in the packed step (csrc/mxfp4_attn.h mx_tile SOFTCAP).  TEST
INFRASTRUCTURE ONLY: the capped counterpart of ``oracle.mxfp4.mxfp4_fwd``'s tile loop, from that module's quantisers
and the masks, tile ranges and merge of ``mxfp4_ragged_ref``, ``mxfp4_window_ref`` and ``mxfp4_split_ref``.  With acc
the fp32 S of a tile, c1 = f32(2 qks / cap) and C = f32(cap log2(e)) (the C entry's constants), the logit of a visible
key in log2 units is C t, t = tanh(acc c1 / (2 log2(e))) = tanh(scale s / cap) taken in float64 and rounded to fp32
once; the row max is over the fp32 products C t of the visible keys and P = exp2(f32(C t - m)).
"""
from __future__ import annotations

import math

import torch

import mxfp4_ragged_ref as RR
import mxfp4_split_ref as SR
import mxfp4_window_ref as WR
from oracle import mxfp4 as M

LOG2E = 1.4426950408889634


def _f32(x: float) -> float:
    return float(torch.tensor(x, dtype=torch.float32))


def _sequence(q, k, v, mode):
    """q fp16 [1, H, Sq, D], k, v fp16 [1, Hkv, L, D]; mode "full", "causal" or (W, S) -> the dequantised
    operands dq [H, Sq, D], dk, dv [H, Skp, D] (float64) and the mask bool [Sq, Skp]."""
    _, H, Sq, D = q.shape
    Hkv, L = k.shape[1], k.shape[2]
    k, v = RR.pad64(k), RR.pad64(v)
    Skp = k.shape[2]
    kvh = torch.arange(H) // (H // Hkv)
    dq = M.deq_rows(*M.quant_rows(q.reshape(H * Sq, D))).reshape(H, Sq, D)
    dk = M.deq_rows(*M.quant_rows(k.reshape(Hkv * Skp, D))).reshape(Hkv, Skp, D)[kvh]
    dv = M.deq_vt(*M.quant_vt(v.reshape(Hkv, Skp, D)))[kvh]
    vis = WR.visible(Sq, L, Skp, *mode) if isinstance(mode, tuple) else RR.visible(Sq, L, Skp, mode == "causal")
    return dq, dk, dv, vis


def mxfp4_fwd_softcap(q, k, v, mode, kps, softcap, scale=None, mslack=8.0):
    """One sequence under the kernel's tile loop -> (O fp16 [1, H, Sq, D], lse fp32 [H, Sq] base 2)."""
    _, H, Sq, D = q.shape
    L = k.shape[2]
    dq, dk, dv, vis_all = _sequence(q, k, v, mode)
    qks = M.qk_scale(D) if scale is None else _f32(scale * M.LOG2E_LITERAL)
    c1, C = _f32(2.0 * qks / _f32(softcap)), _f32(_f32(softcap) * LOG2E)
    kps = min(int(kps), RR.ceil64(L))
    nt, T = RR.ceil64(L) // 64, kps // 64
    ranges = (WR.split_tiles(L, Sq, *mode, kps) if isinstance(mode, tuple)
              else [(t, min(nt, t + T)) for t in range(0, nt, T)])
    order = M.vt_key_order()
    ms, ls, Os = [], [], []
    for t_lo, t_hi in ranges:
        m = torch.full((H, Sq, 1), float("-inf"), dtype=torch.float64)
        l = torch.zeros((H, Sq, 1), dtype=torch.float64)
        O = torch.zeros((H, Sq, D), dtype=torch.float64)
        for k0 in range(64 * t_lo, 64 * t_hi, 64):
            vis = vis_all[None, :, k0:k0 + 64]
            acc = (dq @ dk[:, k0:k0 + 64].transpose(1, 2)).to(torch.float32)
            t = torch.tanh(acc.double() * (c1 / (2 * LOG2E))).to(torch.float32)
            mx = (t * C).masked_fill(~vis, float("-inf")).amax(-1, keepdim=True).double()
            nm = torch.where(mx > m + mslack, torch.ceil(mx), m)
            r = torch.where(torch.isinf(m), torch.zeros_like(m), torch.pow(2.0, m - nm))
            O, l, m = O * r, l * r, nm
            P = torch.exp2((t.double() * C - m).to(torch.float32))
            P = torch.where(vis & ~torch.isinf(m), P, torch.zeros_like(P))   # masked keys and empty rows: P = 0
            codes, b = M.quant_block32(P[..., order])
            Pd = torch.zeros((H, Sq, 64), dtype=torch.float64)
            Pd[..., order] = M.decode(codes) * M.scale_value(b)[..., None]
            l = l + Pd.sum(-1, keepdim=True)
            O = O + Pd @ dv[:, k0:k0 + 64]
        ms.append(m.squeeze(-1))
        ls.append(l.squeeze(-1))
        Os.append(O)
    Oh, lse = SR.merge(torch.stack(ms), torch.stack(ls), torch.stack(Os))
    return Oh.view(q.shape), lse


def dense_reference(q, k, v, mode, softcap=None, scale=None):
    """Plain float64 attention on the DEQUANTISED operands of one sequence, logits softcap * tanh(scale * s /
    softcap) (``softcap`` None: scale * s) -> (O [1, H, Sq, D], lse base 2 [H, Sq])."""
    dq, dk, dv, vis = _sequence(q, k, v, mode)
    z = (dq @ dk.transpose(1, 2)) * (1.0 / math.sqrt(q.shape[3]) if scale is None else scale)
    if softcap is not None:
        z = softcap * torch.tanh(z / softcap)
    z = (z * LOG2E).masked_fill(~vis[None], float("-inf"))
    mx = z.amax(-1, keepdim=True)
    p = torch.exp2(z - mx)
    lsum = p.sum(-1, keepdim=True)
    return ((p / lsum) @ dv)[None], (mx + torch.log2(lsum)).squeeze(-1)
