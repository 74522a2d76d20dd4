"""CPU restatement of the *masked* MX-FP4 forward (csrc/mxfp4_attn.hip header, "Causal").

TEST INFRASTRUCTURE ONLY.  ``oracle/mxfp4.py::mxfp4_fwd`` restates the bidirectional kernel; this
is that function, built from the same oracle pieces, with the two changes the mask makes:

    (acc * qks).masked_fill(~visible, -inf)    before the row max
    P = where(visible, P, 0)                   before quant_block32

``visible[i, j] = j <= i + qoff`` with qoff = 0 (causal 1, top-left) or Sk - Sq (causal 2,
bottom-right; Sk >= Sq).  A row that sees nothing of a tile has mx = -inf there, which raises
nothing, and an all-zero P block quantises to scale byte 0 and zero codes.  Key 0 is visible to
every row, so m is finite after tile 0.  With causal = 0 every step is the oracle's.
"""
from __future__ import annotations

import functools
import math

import torch

from oracle import mxfp4 as M


def key_offset(causal: int, Sq: int, Sk: int) -> int:
    assert causal in (1, 2) and (causal == 1 or Sk >= Sq)
    return 0 if causal == 1 else Sk - Sq


def visible_mask(causal: int, Sq: int, Sk: int) -> torch.Tensor:
    """bool [Sq, Sk]"""
    if not causal:
        return torch.ones((Sq, Sk), dtype=torch.bool)
    return torch.arange(Sk)[None, :] <= torch.arange(Sq)[:, None] + key_offset(causal, Sq, Sk)


def mxfp4_fwd_masked(q, k, v, causal=0, mslack=8.0):
    """As M.mxfp4_fwd: -> (O fp16 [B,H,Sq,D], lse fp32 [B*H,Sq], (q4, qs, k4, ks, vt, vs))."""
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
    vis_all = visible_mask(int(causal), Sq, Sk)
    m = torch.full((BH, Sq, 1), float("-inf"), dtype=torch.float64)
    l = torch.zeros((BH, Sq, 1), dtype=torch.float64)
    O = torch.zeros((BH, Sq, D), dtype=torch.float64)
    order = M.vt_key_order()
    for t in range(Sk // 64):
        k0 = 64 * t
        vis = vis_all[None, :, k0:k0 + 64]
        acc = (dq @ dk[:, k0:k0 + 64].transpose(1, 2)).to(torch.float32)
        mx = (acc * qks).masked_fill(~vis, float("-inf")).amax(-1, keepdim=True).double()
        raise_ = mx > m + mslack
        nm = torch.where(raise_, torch.ceil(mx), m)
        r = torch.where(torch.isinf(m), torch.zeros_like(m), torch.pow(2.0, m - nm))
        O, l, m = O * r, l * r, nm
        P = torch.exp2((acc.double() * qks - m).to(torch.float32))
        P = torch.where(vis, P, torch.zeros_like(P))
        codes, b = M.quant_block32(P[..., order])
        Pd = torch.zeros((BH, Sq, 64), dtype=torch.float64)
        Pd[..., order] = M.decode(codes) * M.scale_value(b)[..., None]
        l = l + Pd.sum(-1, keepdim=True)
        O = O + Pd @ dv[:, k0:k0 + 64]
    lse = (m + torch.log2(l)).squeeze(-1).to(torch.float32)
    Oh = (O / l).to(torch.float16)
    return Oh.view(B, H, Sq, D), lse, (q4, qs, k4, ks, vt, vs)


def exact_masked_attention(q, k, v, causal=0):
    """softmax(mask(q k^T / sqrt(D))) v in fp32 with masked scores at -inf; GQA by head h -> h // G."""
    B, H, Sq, D = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
    kk = k.float().repeat_interleave(H // Hkv, 1)
    vv = v.float().repeat_interleave(H // Hkv, 1)
    s = q.float() @ kk.transpose(2, 3) / math.sqrt(D)
    s = s.masked_fill(~visible_mask(int(causal), Sq, Sk), float("-inf"))
    return torch.softmax(s, -1) @ vv


def cosine(a, b):
    return torch.nn.functional.cosine_similarity(a.float().flatten(), b.float().flatten(), 0).item()


def randn_qkv(shape, seed=2):
    """(B, Hq, Hkv, Sq, Sk) -> fp16 q, k, v at D = 128, drawn as tests/test_gpu_mxfp4.py draws them."""
    B, H, Hkv, Sq, Sk = shape
    g = torch.Generator().manual_seed(seed)
    q = torch.randn((B, H, Sq, 128), generator=g).half()
    k = torch.randn((B, Hkv, Sk, 128), generator=g).half()
    v = torch.randn((B, Hkv, Sk, 128), generator=g).half()
    return q, k, v


# (B, Hq, Hkv, Sq, Sk, causal): the kernel-vs-restatement cases (tests/test_gpu_mxfp4_causal.py)
CASES = [(1, 2, 2, 128, 128, 1), (1, 2, 1, 160, 320, 2), (2, 4, 2, 96, 256, 2), (1, 1, 1, 256, 512, 1),
         (1, 2, 2, 384, 384, 1), (1, 1, 1, 256, 128, 1)]


@functools.lru_cache(maxsize=None)
def case_reference(case):
    """(q, k, v, O, lse, operands) of one of CASES, computed once per session; do not modify."""
    *shape, causal = case
    q, k, v = randn_qkv(tuple(shape))
    return (q, k, v) + mxfp4_fwd_masked(q, k, v, causal)


def accuracy_inputs(Sq, Sk):
    """The inputs of test_gpu_mxfp4.py's accuracy test (seed 4, keys + 2.0) at (2, 4, 2, Sq, Sk)."""
    g = torch.Generator().manual_seed(4)
    q = torch.randn((2, 4, Sq, 128), generator=g).half()
    k = (torch.randn((2, 2, Sk, 128), generator=g) + 2.0).half()
    v = torch.randn((2, 2, Sk, 128), generator=g).half()
    return q, k, v


def smooth_fp16(k):
    """k - its fp16 token mean per (batch, head), in fp16: what the smoothing quantiser sees."""
    km = k.float().mean(2, keepdim=True).half()
    return (k.float() - km.float()).half()
