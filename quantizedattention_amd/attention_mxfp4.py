"""MX-FP4 inference attention forward on gfx950 block-scaled MFMA.

The reference lists SageAttention3's FP4 attention (README.md:49-55) as its goal but ships only the
int8 variant; this module is the FP4 forward built on the CDNA4 ``v_mfma_scale_f32_32x32x64_f8f6f4``
instruction (4x the bf16 MFMA rate).  There is no reference interface to mirror, so the names
follow the int8 module: ``sage_attention_3_fp4(q, k, v, causal=False)`` is the drop-in style entry,
``mxfp4_attn_fwd`` also returns the quantised operands, and ``mxfp4_attn_fwd_kv(q, kv, causal)``
takes the key/value operands back: a later query chunk runs against an already quantised K/V
(chunked prefill, ``causal=2``) and only q is quantised again.

Numerics (csrc/mxfp4_attn.hip header): Q and K are MX-FP4 along head_dim (32-element blocks,
e8m0 scales); V along keys; P is re-quantised to MX-FP4 per query row and 32 keys inside the
kernel; the softmax state is fp32 and the row sum l adds the quantised P (on the matrix core).
The running max is kept as an integer raised lazily, so every rescale is a power of two and the
fp4 codes of P do not depend on the tile order of the max updates.  K is smoothed by its token mean first
(SageAttention), which leaves softmax unchanged and shrinks the K block ranges.  ``causal`` is
``False``/``0``, ``True``/``1`` (top-left: row i sees keys j <= i) or ``2`` (bottom-right: j <= i +
Sk - Sq, Sk >= Sq); a masked key takes no part in the row max and its P is exactly 0 before the
fp4 quantisation, and key tiles past a row block's diagonal are never read.  Forward only: the
outputs carry no autograd graph.
"""
from __future__ import annotations

import torch

from . import _lib

__all__ = ["mxfp4_quantize_rows", "mxfp4_quantize_v", "mxfp4_attn_fwd", "mxfp4_attn_fwd_kv",
           "sage_attention_3_fp4"]


_qk_scale = _lib.qk_scale


def mxfp4_quantize_rows(x: torch.Tensor, mean: torch.Tensor | None = None):
    """x [..., S, D] (fp16) -> (packed uint8 [rows, D/2], scales uint8 [rows, D/32]).

    ``mean`` [..., 1, D] (fp16, one row per leading index): quantise f16(x - mean) instead.
    """
    _lib.require_gpu(x)
    D = x.shape[-1]
    if D not in (64, 128):
        raise _lib.QAttnError("qattn mxfp4: head_dim must be 64 or 128")
    x = _lib.kernel_input(x, torch.float16)
    rows = x.numel() // D
    seq = x.shape[-2] if x.dim() >= 2 else rows
    if mean is not None:
        mean = _lib.kernel_input(mean, torch.float16)
        if mean.numel() * seq != x.numel():
            raise _lib.QAttnError("qattn mxfp4: mean must hold one row per sequence")
    q4 = torch.empty((rows, D // 2), dtype=torch.uint8, device=x.device)
    sc = torch.empty((rows, D // 32), dtype=torch.uint8, device=x.device)
    _lib.call("qattn_mxfp4_quant_rows", _lib.ptr(x), _lib.ptr(mean) if mean is not None else None,
              _lib.ptr(q4), _lib.ptr(sc), rows, seq, D, _lib.stream_of(x))
    return q4, sc


def mxfp4_quantize_v(v: torch.Tensor):
    """v [B, H, S, D] (fp16) -> (vt uint8 [B*H, S/64, D, 32], vs uint8 [B*H, S/64, D, 2])."""
    _lib.require_gpu(v)
    B, H, S, D = v.shape
    if S % 64:
        raise _lib.QAttnError("qattn mxfp4: key tokens must be a multiple of 64")
    if D not in (64, 128):
        raise _lib.QAttnError("qattn mxfp4: head_dim must be 64 or 128")
    v = _lib.kernel_input(v, torch.float16)
    vt = torch.empty((B * H, S // 64, D, 32), dtype=torch.uint8, device=v.device)
    vs = torch.empty((B * H, S // 64, D, 2), dtype=torch.uint8, device=v.device)
    _lib.call("qattn_mxfp4_quant_vt", _lib.ptr(v), _lib.ptr(vt), _lib.ptr(vs), B * H, S, D,
              _lib.stream_of(v))
    return vt, vs


def _check(q, k, v):
    if q.dim() != 4 or k.shape != v.shape or q.shape[0] != k.shape[0] or q.shape[-1] != k.shape[-1]:
        raise _lib.QAttnError("qattn mxfp4: q [B,H,Sq,D], k = v [B,Hkv,Sk,D] expected")
    if q.shape[1] % k.shape[1]:
        raise _lib.QAttnError("qattn mxfp4: query heads must be a multiple of key/value heads")
    if q.shape[-1] != 128:
        raise _lib.QAttnError("qattn mxfp4: head_dim must be 128")
    if q.shape[2] % 32 or k.shape[2] % 64:
        raise _lib.QAttnError("qattn mxfp4: q tokens must be a multiple of 32, k tokens of 64")


def _causal_mode(causal, Sq: int, Sk: int) -> int:
    mode = int(causal)
    if mode not in (0, 1, 2):
        raise _lib.QAttnError("qattn mxfp4: causal must be False/0, True/1 (top-left) or 2 (bottom-right)")
    if mode == 2 and Sq > Sk:
        raise _lib.QAttnError("qattn mxfp4: causal=2 (bottom-right) needs Sk >= Sq")
    return mode


def _attn(q4, qs, k4, ks, vt, vs, B, H, Hkv, Sq, Sk, D, mode, like):
    out = torch.empty((B, H, Sq, D), dtype=torch.float16, device=like.device)
    lse = torch.empty((B * H, Sq), dtype=torch.float32, device=like.device)
    if B * H * Sq:   # (without query rows there is nothing to launch: empty outputs)
        _lib.call("qattn_mxfp4_attn_fwd_ex", _lib.ptr(q4), _lib.ptr(qs), _lib.ptr(k4), _lib.ptr(ks),
                  _lib.ptr(vt), _lib.ptr(vs), _lib.ptr(out), _lib.ptr(lse), B * H, Sq, Sk, H // Hkv, mode, D,
                  _qk_scale(D), _lib.stream_of(like))
    return out, lse


@torch.no_grad()
def mxfp4_attn_fwd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, smooth_k: bool = True,
                   causal=False):
    """-> (O fp16 [B,H,Sq,D], lse fp32 [B*H, Sq] base 2, (q4, qs, k4, ks, vt, vs)).

    ``smooth_k`` quantises k - k_mean with k_mean the fp16 token mean per (batch, head)
    (qattn_kmean, as the int8 path); softmax is invariant to it.  ``causal``: module docstring.
    The last four operands are the ``kv`` of ``mxfp4_attn_fwd_kv``.
    """
    _check(q, k, v)
    _lib.require_gpu(q, k, v)
    B, H, Sq, D = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
    mode = _causal_mode(causal, Sq, Sk)
    _lib.refuse_empty_keys("qattn mxfp4", B * H * Sq, Sk)
    k = _lib.kernel_input(k, torch.float16)
    k_mean = None
    if smooth_k:   # f16 token mean per (batch, head), subtracted inside the quantiser
        k_mean = torch.empty((B, Hkv, 1, D), dtype=torch.float16, device=q.device)
        _lib.call("qattn_kmean", _lib.ptr(k), _lib.ptr(k_mean), B * Hkv, Sk, D, _lib.stream_of(k))
    q4, qs = mxfp4_quantize_rows(q)
    k4, ks = mxfp4_quantize_rows(k, k_mean)
    vt, vs = mxfp4_quantize_v(v)
    out, lse = _attn(q4, qs, k4, ks, vt, vs, B, H, Hkv, Sq, Sk, D, mode, q)
    return out, lse, (q4, qs, k4, ks, vt, vs)


@torch.no_grad()
def mxfp4_attn_fwd_kv(q: torch.Tensor, kv, causal=False):
    """q [B,H,Sq,D] against already quantised keys/values -> (O fp16 [B,H,Sq,D], lse fp32 [B*H, Sq]).

    ``kv = (k4, ks, vt, vs)`` as ``mxfp4_attn_fwd`` returns them (its operands ``[2:]``): the
    key/value head count and Sk are read from ``vt`` [B*Hkv, Sk/64, D, 32] and q's batch.  Only q
    is quantised.  ``causal=2`` places the Sq query rows at the end of the Sk keys, which is a
    chunk of a prefill against its cache.  A cache quantised with ``smooth_k`` is queried as it
    is: the shift k_mean adds the same q . k_mean to every score of a row, which softmax ignores
    (lse is then that of the smoothed scores, as ``mxfp4_attn_fwd`` itself returns it).
    """
    k4, ks, vt, vs = kv
    _lib.require_gpu(q, k4, ks, vt, vs)
    if q.dim() != 4 or vt.dim() != 4 or vs.dim() != 4:
        raise _lib.QAttnError("qattn mxfp4: q [B,H,Sq,D], vt [B*Hkv,Sk/64,D,32], vs [B*Hkv,Sk/64,D,2] expected")
    B, H, Sq, D = q.shape
    if D != 128 or vt.shape[2] != D or vt.shape[3] != 32 or tuple(vs.shape) != (*vt.shape[:3], 2):
        raise _lib.QAttnError("qattn mxfp4: head_dim must be 128 in q and in the quantised values")
    if B == 0 or vt.shape[0] % B:
        raise _lib.QAttnError("qattn mxfp4: the quantised values do not hold q's batch")
    Hkv, Sk = vt.shape[0] // B, vt.shape[1] * 64
    if Hkv == 0 or H % Hkv:
        raise _lib.QAttnError("qattn mxfp4: query heads must be a multiple of key/value heads")
    if Sq % 32:
        raise _lib.QAttnError("qattn mxfp4: q tokens must be a multiple of 32, k tokens of 64")
    rows = B * Hkv * Sk
    if k4.numel() != rows * (D // 2) or ks.numel() != rows * (D // 32):
        raise _lib.QAttnError("qattn mxfp4: k4 / ks do not match the key count of vt")
    if any(t.dtype != torch.uint8 or not t.is_contiguous() for t in (k4, ks, vt, vs)):
        raise _lib.QAttnError("qattn mxfp4: the quantised operands must be contiguous uint8")
    mode = _causal_mode(causal, Sq, Sk)
    _lib.refuse_empty_keys("qattn mxfp4", B * H * Sq, Sk)
    q4, qs = mxfp4_quantize_rows(q)
    return _attn(q4, qs, k4, ks, vt, vs, B, H, Hkv, Sq, Sk, D, mode, q)


def sage_attention_3_fp4(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, causal=False) -> torch.Tensor:
    """softmax(mask(q k^T / sqrt(D))) v with MX-FP4 operands (inference; fp16 output)."""
    return mxfp4_attn_fwd(q, k, v, causal=causal)[0]
