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

from dataclasses import dataclass

import torch

from . import _lib

__all__ = ["mxfp4_quantize_rows", "mxfp4_quantize_v", "mxfp4_attn_fwd", "mxfp4_attn_fwd_kv",
           "sage_attention_3_fp4", "Rope", "rope_table", "mxfp4_quantize_rows_rope"]


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


ROPE_DIM = 128   # the head_dim of every rotary entry


@dataclass(frozen=True)
class Rope:
    """A rotary table for the ``rope=`` arguments of the packed MX-FP4 cache path.

    ``table`` fp32 [max_pos, 128], contiguous, on the GPU: row p holds cos theta(p, i) in column i and
    sin theta(p, i) in column 64 + i for pair i in [0, 64) (the ``cos_sin_cache`` convention, so a table
    scaled by YaRN, llama3 or NTK is passed as it is; :func:`rope_table` makes the plain one).
    ``interleaved=False`` (NeoX, rotate half) pairs elements (i, i + 64) of a head's row, ``True`` (GPT-J)
    elements (2i, 2i + 1).  The rotation itself is defined bit for bit (include/qattn.h): per pair (a, b),
    ``f16(f32(a c) - f32(b s))`` and ``f16(f32(b c) + f32(a s))``, what ``(a.float() * c - b.float() *
    s).half()`` gives in torch."""

    table: torch.Tensor
    interleaved: bool = False

    def __post_init__(self):
        t = self.table
        if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 2
                or t.shape[1] != ROPE_DIM or t.shape[0] < 1 or not t.is_contiguous()):
            raise _lib.QAttnError("qattn mxfp4 rope: the table must be a contiguous fp32 tensor [max_pos >= 1, 128] "
                                  "(cos in columns [0, 64), sin in [64, 128))")
        _lib.require_gpu(t)
        if not isinstance(self.interleaved, bool):
            raise _lib.QAttnError(f"qattn mxfp4 rope: interleaved must be a bool, got {self.interleaved!r}")

    @property
    def max_pos(self) -> int:
        return self.table.shape[0]


def rope_table(max_pos: int, base: float = 10000.0, device=None) -> torch.Tensor:
    """The plain rotary table fp32 [max_pos, 128] of :class:`Rope`: the angles ``p * base ** (-2 i / 128)``
    are computed in float64 on the host, their cos (columns [0, 64)) and sin (columns [64, 128)) rounded
    once to fp32, then moved to ``device`` (None: left on the host)."""
    if int(max_pos) < 1 or not base > 0:
        raise _lib.QAttnError(f"qattn mxfp4 rope: max_pos >= 1 and base > 0 expected, got {max_pos}, {base}")
    i = torch.arange(ROPE_DIM // 2, dtype=torch.float64)
    inv_freq = torch.pow(torch.tensor(float(base), dtype=torch.float64), -2.0 * i / ROPE_DIM)
    ang = torch.arange(int(max_pos), dtype=torch.float64)[:, None] * inv_freq[None, :]
    table = torch.cat([ang.cos(), ang.sin()], 1).to(torch.float32).contiguous()
    return table if device is None else table.to(device)


def _host_positions(positions, tokens: int, max_pos: int) -> torch.Tensor:
    """Host ``positions`` (a list or a host tensor) of a rotary call as a host int32 tensor of ``tokens``
    values in [0, max_pos); raises :class:`QAttnError` otherwise.  No device."""
    pos = torch.as_tensor(positions, dtype=torch.int64).reshape(-1)
    if pos.numel() != tokens:
        raise _lib.QAttnError(f"qattn mxfp4 rope: {pos.numel()} positions for {tokens} packed tokens")
    if tokens and (int(pos.min()) < 0 or int(pos.max()) >= max_pos):
        bad = pos[(pos < 0) | (pos >= max_pos)][:8].tolist()
        raise _lib.QAttnError(f"qattn mxfp4 rope: positions {bad} outside the table's [0, {max_pos})")
    return pos.to(torch.int32)


def _device_positions(positions, tokens: int) -> bool:
    """Whether ``positions`` is a device tensor, which is then held to int32 [tokens], contiguous; it is
    used as given and never read back (the kernels clamp it to the table)."""
    if not (isinstance(positions, torch.Tensor) and positions.is_cuda):
        return False
    if positions.dtype != torch.int32 or tuple(positions.shape) != (tokens,) or not positions.is_contiguous():
        raise _lib.QAttnError(f"qattn mxfp4 rope: device positions must be a contiguous int32 tensor [{tokens}]")
    return True


def mxfp4_quantize_rows_rope(x: torch.Tensor, rope: Rope, positions):
    """Packed x [T, H, 128] (fp16, token-major), each row rotated by its token's position first (:class:`Rope`)
    -> (packed uint8 [T*H, 64], scales uint8 [T*H, 4]), bit for bit ``mxfp4_quantize_rows`` of the rotated
    fp16 rows.  ``positions``: T ints in [0, rope.max_pos) as a list or a host tensor (checked, uploaded
    without a synchronisation), or a device int32 tensor [T], used as given."""
    if not isinstance(rope, Rope):
        raise _lib.QAttnError("qattn mxfp4 rope: rope must be a Rope")
    if x.dim() != 3 or x.shape[2] != ROPE_DIM:
        raise _lib.QAttnError("qattn mxfp4 rope: packed rows must be x [T, H, 128]")
    T, H, D = x.shape
    if T * H >= 1 << 31:
        raise _lib.QAttnError("qattn mxfp4 rope: fewer than 2^31 packed rows expected")
    if not _device_positions(positions, T):
        positions = _host_positions(positions, T, rope.max_pos)
    _lib.require_gpu(x, rope.table)
    x = _lib.kernel_input(x, torch.float16)
    pos = _lib.kernel_input(positions.to(x.device, non_blocking=True))
    q4 = torch.empty((T * H, D // 2), dtype=torch.uint8, device=x.device)
    sc = torch.empty((T * H, D // 32), dtype=torch.uint8, device=x.device)
    _lib.call("qattn_mxfp4_quant_rows_rope", _lib.ptr(x), _lib.ptr(q4), _lib.ptr(sc), _lib.ptr(rope.table),
              _lib.ptr(pos), T, H, rope.max_pos, int(rope.interleaved), D, _lib.stream_of(x))
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
