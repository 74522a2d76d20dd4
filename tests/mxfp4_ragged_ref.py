"""CPU restatement of the length-aware key-split MX-FP4 forward (csrc/mxfp4_attn.hip,
mxfp4_attn_split_kernel with LEN; kv_cache_mxfp4.attention_mxfp4_decode).

TEST INFRASTRUCTURE ONLY.  Built from the pieces of ``oracle/mxfp4.py`` like
``mxfp4_masked_ref.mxfp4_fwd_masked`` and ``mxfp4_split_ref.split_partials``, whose tile loop it runs.
Sequence b of a batch has its own L_b keys.  Per sequence, k and v are zero-padded to Sk' = ceil64(L)
keys and quantised as the cache is; query position i of Sq sees key j iff

    j <= L - 1              (not causal)
    j <= i + L - Sq         (causal: the queries are the sequence's last Sq positions, Sq <= L)

Split s of nsplit = ceil(sk_max / kps), sk_max = ceil64(max_b L_b), runs the tiles of the keys
[s * kps, min(Sk', s * kps + kps)) from m = -inf; when that range is empty its state is (-inf, 0, 0).
The merge is ``mxfp4_split_ref.merge`` (float64).
"""
from __future__ import annotations

import functools

import torch

import mxfp4_split_ref as SR
from oracle import mxfp4 as M


def ceil64(n: int) -> int:
    return -(-n // 64) * 64


def pad64(x: torch.Tensor) -> torch.Tensor:
    """[.., L, D] -> [.., ceil64(L), D], zero-padded."""
    L = x.shape[-2]
    out = torch.zeros((*x.shape[:-2], ceil64(L), x.shape[-1]), dtype=x.dtype)
    out[..., :L, :] = x
    return out


def visible(Sq: int, L: int, Skp: int, causal: bool) -> torch.Tensor:
    """bool [Sq, Skp]"""
    j = torch.arange(Skp)[None, :]
    if causal:
        assert Sq <= L
        return j <= torch.arange(Sq)[:, None] + (L - Sq)
    return (j <= L - 1).expand(Sq, Skp)


def sequence_partials(q, k, v, causal, kps, nsplit, mslack=8.0):
    """One sequence: q fp16 [1, H, Sq, D], k, v fp16 [1, Hkv, L, D] (any L >= 1) ->
    (m [nsplit, H, Sq], l [nsplit, H, Sq], O [nsplit, H, Sq, D], float64)."""
    _, H, Sq, D = q.shape
    Hkv, L = k.shape[1], k.shape[2]
    k, v = pad64(k), pad64(v)
    Skp = k.shape[2]
    qks = M.qk_scale(D)
    q4, qs = M.quant_rows(q.reshape(H * Sq, D))
    k4, ks = M.quant_rows(k.reshape(Hkv * Skp, D))
    vt, vs = M.quant_vt(v.reshape(Hkv, Skp, D))
    kvh = torch.arange(H) // (H // Hkv)
    dq = M.deq_rows(q4, qs).reshape(H, Sq, D)
    dk = M.deq_rows(k4, ks).reshape(Hkv, Skp, D)[kvh]
    dv = M.deq_vt(vt, vs)[kvh]
    vis_all = visible(Sq, L, Skp, causal)
    order = M.vt_key_order()
    ms, ls, Os = [], [], []
    for s in range(nsplit):
        m = torch.full((H, Sq, 1), float("-inf"), dtype=torch.float64)
        l = torch.zeros((H, Sq, 1), dtype=torch.float64)
        O = torch.zeros((H, Sq, D), dtype=torch.float64)
        for k0 in range(s * kps, min(Skp, s * kps + kps), 64):
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


def mxfp4_fwd_ragged(q, ks, vs, causal, kps=None):
    """q fp16 [B, H, Sq, D]; ks, vs: per sequence fp16 [1, Hkv, L_b, D] -> (O fp16 [B, H, Sq, D], lse
    fp32 [B*H, Sq], (m, l) of the partials [nsplit, B*H, Sq]).  kps None: one split."""
    B, H, Sq, D = q.shape
    sk_max = ceil64(max(k.shape[2] for k in ks))
    kps = sk_max if kps is None else min(int(kps), sk_max)
    nsplit = -(-sk_max // kps)
    parts = [sequence_partials(q[b:b + 1], ks[b], vs[b], causal, kps, nsplit) for b in range(B)]
    m, l, O = (torch.cat([p[i] for p in parts], 1) for i in range(3))
    Oh, lse = SR.merge(m, l, O)
    return Oh.view(B, H, Sq, D), lse, (m, l)


def identity_problem(q_b, k_b, v_b, causal):
    """The problem of the EXISTING bottom-right definition whose first Sq rows are sequence b's ragged
    result: the keys zero-padded to Sk' = ceil64(L) and Sq' = Sq + Sk' - L query rows (the extra rows
    are zeros), causal 2.  Non-causal is stated for Sq = 1 only (row 0 of Sq' = Sk' - L + 1)."""
    Sq, L = q_b.shape[2], k_b.shape[2]
    assert causal or Sq == 1
    kp, vp = pad64(k_b), pad64(v_b)
    q2 = torch.zeros((1, q_b.shape[1], Sq + kp.shape[2] - L, 128), dtype=torch.float16)
    q2[:, :, :Sq] = q_b
    return q2, kp, vp


def inputs(B, Hq, Hkv, Sq, lens, seed=2, kshift=0.0):
    """fp16 q [B, Hq, Sq, 128] and per sequence k, v [1, Hkv, L_b, 128]."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn((B, Hq, Sq, 128), generator=g).half()
    ks = [(torch.randn((1, Hkv, L, 128), generator=g) + kshift).half() for L in lens]
    vs = [torch.randn((1, Hkv, L, 128), generator=g).half() for L in lens]
    return q, ks, vs


# (B, Hq, Hkv, Sq, lens, causal, keys per split): the kernel-vs-restatement cases
# (tests/test_gpu_mxfp4_ragged.py)
CASES = [(3, 4, 2, 1, (37, 128, 200), 0, 64), (2, 2, 1, 33, (97, 250), 2, 128),
         (2, 8, 2, 4, (64, 65), 2, 64)]


@functools.lru_cache(maxsize=None)
def case_reference(case, k_mean_shift=False):
    """(q, ks, vs, O, lse) of one of CASES, computed once per session; do not modify.  With
    ``k_mean_shift`` the keys are drawn around +2 and the reference runs on f16(k - k_mean), k_mean the
    fp16 token mean of each sequence's first min(L, 64) keys: what a smoothed cache holds."""
    B, Hq, Hkv, Sq, lens, causal, kps = case
    q, ks, vs = inputs(B, Hq, Hkv, Sq, lens, kshift=2.0 if k_mean_shift else 0.0)
    kq = ks
    if k_mean_shift:
        kq = [(k.float() - k_mean_of(k).float()).half() for k in ks]
    O, lse, _ = mxfp4_fwd_ragged(q, kq, vs, bool(causal), kps)
    return q, ks, vs, O, lse


def k_mean_of(k):
    """fp16 [1, Hkv, 1, D]: the token mean of the first min(L, 64) keys."""
    return k[:, :, :min(k.shape[2], 64)].float().mean(2, keepdim=True).half()
