"""CPU restatement of the tree-masked packed step (csrc/mxfp4_attn.hip, mxfp4_attn_split_kernel with TREE;
kv_cache_mxfp4.attention_mxfp4_varlen_paged(tree=)).

TEST INFRASTRUCTURE ONLY.  ``mxfp4_window_ref.sequence_partials`` with another mask: one sequence of L keys
and n queries, the sequence's last n positions, whose last nd <= min(n, 64) queries are the nodes of a draft
tree appended at keys base = L - nd ...  With t = i - (n - nd), query i sees key k iff

    t <  0:  k <= L - n + i                                           (plain causal)
    t >= 0:  k < base  or  (k = base + b  and  bit b of masks[t] set)

``masks[t]`` holds node t's ancestors and t itself (``kv_cache_mxfp4.tree_ancestor_masks``); it is used as
given, so a test can hand in a wrong word.  The splits are the causal call's: split s runs the tiles [s T,
min(nt, s T + T)), T = kps / 64, each from m = -inf.  The merge is ``mxfp4_split_ref.merge`` (float64).
"""
from __future__ import annotations

import random

import torch

import mxfp4_ragged_ref as RR
import mxfp4_split_ref as SR
from oracle import mxfp4 as M


def ancestors(parents) -> list:
    """``tree_ancestor_masks`` restated: parents[t] in [-1, t)."""
    anc = []
    for t, p in enumerate(parents):
        assert -1 <= p < t
        anc.append((anc[p] if p >= 0 else 0) | 1 << t)
    return anc


def chain(nd):
    return list(range(-1, nd - 1))


def star(nd):
    """A root and nd - 1 leaves."""
    return [-1] + [0] * (nd - 1)


def heap(nd):
    return [(t - 1) // 2 if t else -1 for t in range(nd)]


def forest(nd, every=5):
    """Chains of ``every`` nodes: a root every ``every`` nodes."""
    return [-1 if t % every == 0 else t - 1 for t in range(nd)]


def rand_tree(nd, seed=5):
    rng = random.Random(seed)
    return [-1] + [rng.randrange(t) for t in range(1, nd)]


TREES = {"star": star, "heap": heap, "random": rand_tree, "forest": forest}


def visible(n: int, L: int, nd: int, masks, Skp=None) -> torch.Tensor:
    """bool [n, Skp]"""
    assert 0 <= nd <= min(n, 64) and n <= L and len(masks) == nd
    Skp = RR.ceil64(L) if Skp is None else Skp
    vis = RR.visible(n, L, Skp, True).clone()
    base = L - nd
    for t, w in enumerate(masks):
        row = torch.zeros(Skp, dtype=torch.bool)
        row[:base] = True
        for b in range(64):
            if w >> b & 1 and base + b < Skp:
                row[base + b] = True
        vis[n - nd + t] = row
    return vis


def sequence_partials(q, k, v, nd, masks, kps, mslack=8.0):
    """One sequence: q fp16 [1, H, n, D], k, v fp16 [1, Hkv, L, D] (L >= n) -> (m [ns, H, n], l [ns, H, n],
    O [ns, H, n, D], float64)."""
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
    vis_all = visible(Sq, L, nd, masks, Skp)
    order = M.vt_key_order()
    ms, ls, Os = [], [], []
    for s0 in range(0, Skp, kps):
        m = torch.full((H, Sq, 1), float("-inf"), dtype=torch.float64)
        l = torch.zeros((H, Sq, 1), dtype=torch.float64)
        O = torch.zeros((H, Sq, D), dtype=torch.float64)
        for k0 in range(s0, min(Skp, s0 + kps), 64):
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


def mxfp4_fwd_tree(q, k, v, nd, masks, kps):
    """One sequence -> (O fp16 [1, H, n, D], lse fp32 [H, n], (m, l) of the partials)."""
    kps = min(int(kps), RR.ceil64(k.shape[2]))
    m, l, O = sequence_partials(q, k, v, nd, masks, kps)
    Oh, lse = SR.merge(m, l, O)
    return Oh.view(q.shape), lse, (m, l)


def dense_reference(q, k, v, nd, masks):
    """float64 softmax attention with the tree mask on the DEQUANTISED operands of one sequence -> (O [1, H,
    n, D], lse base 2 [H, n])."""
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
    s = s.masked_fill(~visible(Sq, L, nd, masks, Skp)[None], float("-inf"))
    mx = s.amax(-1, keepdim=True)
    p = torch.exp2(s - mx)
    lsum = p.sum(-1, keepdim=True)
    return ((p / lsum) @ dv)[None], (mx + torch.log2(lsum)).squeeze(-1)
