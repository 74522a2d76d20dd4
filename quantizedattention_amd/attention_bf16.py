"""Drop-in for ``attention_bf16`` of selau642/QuantizedAttention, backed by gfx950 HIP kernels.

Public names (same signatures, outputs and assertion messages):
  FlashAttention_2_BF16_autograd_function   attention_bf16.py:16-85
  flash_atten_2_bf16                        attention_bf16.py:87-105
  helion_atten_bf16_fwd_training            attention_bf16.py:107-296
  helion_flash_atten_2_algo_4_bwd           attention_bf16.py:299-448
  baseline_pytorch_attention                attention_bf16.py:450-478

Forward: bf16 FlashAttention with the reference's "multiple-max" beta rule emulated at its pinned
k-tile of 16 (bf16:736).  Extension: k, v may have fewer heads than q (grouped-query
attention, query head h reads key/value head h // (Hq / Hkv)); dk, dv then sum over each group.  Backward: FA2 algorithm 4 with the build-contract fixes of SURVEY F3
(dS = P*(dP-D), sm_scale, deterministic dQ).
"""
from __future__ import annotations

from typing import Tuple

import torch
from torch.autograd import Function

from . import _lib
from ._baseline import baseline_pytorch_attention  # noqa: F401

__all__ = [
    "FlashAttention_2_BF16_autograd_function", "flash_atten_2_bf16",
    "helion_atten_bf16_fwd_training", "helion_flash_atten_2_algo_4_bwd",
    "baseline_pytorch_attention",
]

KT = 16  # k-tile of the beta rule (reference tuned config, bf16:736)


def _check(q, k, v):
    batch, head, q_tokens, q_head_dim = q.shape
    k_batch, k_head, k_tokens, k_head_dim = k.shape
    v_batch, v_head, v_tokens, v_head_dim = v.shape
    assert k_tokens == v_tokens, "input k_tokens must match v_tokens"  # bf16:154
    assert q_head_dim == k.size(-1) == v.size(-1), \
        "all head dimensions must match for q, k, v tensors"  # bf16:155
    if not (q.shape[0] == k.shape[0] and k.shape[:2] == v.shape[:2] and head % k.shape[1] == 0):
        raise _lib.QAttnError("qattn bf16: batch must match and q heads must be a multiple of k/v heads")
    if q_tokens % 32 or k_tokens % 32:
        raise _lib.QAttnError("qattn bf16: token counts must be multiples of 32")
    if q_head_dim not in (64, 128):
        raise _lib.QAttnError("qattn bf16: head_dim must be 64 or 128")


def helion_atten_bf16_fwd_training(
    q_fp16_input: torch.Tensor,
    k_fp16_input: torch.Tensor,
    v_bf16_input: torch.Tensor,
    causal: bool,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """bf16:111-296 -> (O fp32 [B,H,S,D], lse fp32 [B*H, S], base-2 units)."""
    _check(q_fp16_input, k_fp16_input, v_bf16_input)
    _lib.require_gpu(q_fp16_input, k_fp16_input, v_bf16_input)
    _lib.refuse_empty_keys("qattn bf16", q_fp16_input.numel() // q_fp16_input.shape[3],
                           k_fp16_input.shape[2])
    q = _lib.kernel_input(q_fp16_input, torch.float16)
    k = _lib.kernel_input(k_fp16_input, torch.float16)
    v = _lib.kernel_input(v_bf16_input, torch.bfloat16)
    B, H, S, D = q.shape
    Sk = k.shape[2]
    O = torch.empty((B, H, S, D), dtype=torch.float32, device=q.device)
    lse = torch.empty((B * H, S), dtype=torch.float32, device=q.device)
    qks = _lib.qk_scale(D)
    # grouped-query attention (SURVEY §8f N2 extension): query head h reads k/v head h // (H / Hkv);
    # causal: the per-head V suffix sums stand in for the fully masked key tiles (include/qattn.h);
    # without room for them the kernel runs the whole masked tile loop (same results)
    ws = None
    if causal and B * H * S > 0:
        ws = _lib.try_workspace(_lib.load().qattn_bf16_fwd_ws_bytes(B * k.shape[1], Sk, D), q.device)
    if B * H * S:   # (without query rows there is nothing to launch: empty outputs)
        _lib.call("qattn_bf16_fwd_ws_ex", _lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(O), _lib.ptr(lse),
                  B * H, S, Sk, H // k.shape[1], int(bool(causal)), D, qks, _lib.ptr(ws), _lib.stream_of(q))
    return O, lse


def helion_flash_atten_2_algo_4_bwd(
    q_input: torch.Tensor,
    k_input: torch.Tensor,
    v_input: torch.Tensor,
    O_input: torch.Tensor,
    lse_input: torch.Tensor,
    causal: bool,
    dO_input: torch.Tensor,
):
    """bf16:309-448 (corrected) -> fp32 (dq, dk, dv)."""
    _check(q_input, k_input, v_input)
    _lib.require_gpu(q_input, k_input, v_input, O_input, lse_input, dO_input)
    _lib.refuse_empty_keys("qattn bf16 backward", q_input.numel() // q_input.shape[3], k_input.shape[2])
    q = _lib.kernel_input(q_input, torch.float16)
    k = _lib.kernel_input(k_input, torch.float16)
    v = _lib.kernel_input(v_input, torch.bfloat16)
    O = _lib.kernel_input(O_input, torch.float32)
    dO = _lib.kernel_input(dO_input, torch.float32)
    lse = _lib.kernel_input(lse_input, torch.float32)
    B, H, S, D = q.shape
    Sk = k.shape[2]
    dev = q.device
    if B * H * S == 0:   # no query rows: dq is empty, dk and dv are zero
        z = dict(dtype=torch.float32, device=dev)
        return torch.zeros(q.shape, **z), torch.zeros(k.shape, **z), torch.zeros(k.shape, **z)
    st = _lib.stream_of(q)
    dO_bf = torch.empty((B, H, S, D), dtype=torch.bfloat16, device=dev)
    LD = torch.empty((B * H, S, 2), dtype=torch.float32, device=dev)
    _lib.call("qattn_bf16_bwd_prep", _lib.ptr(dO), _lib.ptr(O), _lib.ptr(lse), _lib.ptr(dO_bf),
              _lib.ptr(LD), B * H, S, D, st)
    q_bf = torch.empty(q.shape, dtype=torch.bfloat16, device=dev)
    k_bf = torch.empty(k.shape, dtype=torch.bfloat16, device=dev)
    _lib.call("qattn_f16_to_bf16", _lib.ptr(q), _lib.ptr(q_bf), q.numel(), st)
    _lib.call("qattn_f16_to_bf16", _lib.ptr(k), _lib.ptr(k_bf), k.numel(), st)
    dq = torch.empty((B, H, S, D), dtype=torch.float32, device=dev)
    Hkv = k.shape[1]
    dk = torch.empty((B, Hkv, Sk, D), dtype=torch.float32, device=dev)
    dv = torch.empty((B, Hkv, Sk, D), dtype=torch.float32, device=dev)
    args = (_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(dO_bf), _lib.ptr(LD), _lib.ptr(q_bf),
            _lib.ptr(k_bf), _lib.ptr(dq), _lib.ptr(dk), _lib.ptr(dv),
            B * H, S, Sk, H // Hkv, int(bool(causal)), D, _lib.qk_scale(D), _lib.sm_scale(D))
    force = {"auto": -1, "ws": 1}.get(_BWD_ENTRY)   # (None: an entry by name, no records)
    ws = None
    if force is not None:
        ws_bytes = _lib.load().qattn_bf16_bwd_plan(B * H, S, Sk, int(bool(causal)), force,
                                                   -1 if WS_MAX_BYTES is None else max(0, WS_MAX_BYTES))
        if ws_bytes > 0:
            # (None when there is no room for the dS records: recompute dS in the dQ pass, same
            # results)
            ws = _lib.try_workspace(ws_bytes, dev)
    if ws is not None:
        _lib.call("qattn_bf16_bwd_ws_ex", *args, _lib.ptr(ws), st)
    else:
        _lib.call("qattn_bf16_bwd_ex" if force is not None else _BWD_ENTRY, *args, st)
    return dq, dk, dv


# "auto" (default): the library's plan (qattn_bf16_bwd_plan: records when causal; QATTN_BF16_BWD_WS=1
# / 0 forces them on / off).  "qattn_bf16_bwd_ex": fused dK+dV, dQ recomputing S and dP; "ws": the
# fused kernel also stores bf16 dS records (2 B per score, up to QATTN_BWD_WS_MAX bytes) and dQ reads
# them -- non-causal at config 3 the record traffic costs what the dQ pass saves, causal it is 7 %
# faster; "qattn_bf16_bwd_split_ex": separate dV and dK kernels.  All give
# bit-identical gradients.
_BWD_ENTRY = "auto"
# None: the library's shared cap (qattn_bwd_ws_cap), as the int8 backward and the C++ operators
WS_MAX_BYTES = None


class FlashAttention_2_BF16_autograd_function(Function):
    """bf16:16-85: forward in bf16 (returns O fp32, lse fp32), backward in fp32-accumulated MFMA."""

    @staticmethod
    def forward(q_fp16, k_fp16, v_bf16, causal):
        return helion_atten_bf16_fwd_training(q_fp16, k_fp16, v_bf16, causal)

    @staticmethod
    def setup_context(ctx, inputs, output):
        q_fp16, k_fp16, v_bf16, causal = inputs
        O_fp32, lse_fp32 = output
        ctx.mark_non_differentiable(lse_fp32)  # bf16:55
        ctx.save_for_backward(q_fp16, k_fp16, v_bf16, O_fp32, lse_fp32)  # bf16:56
        ctx.args = causal

    @staticmethod
    def backward(ctx, dO, _lse):
        # plain tensors under torch.func transforms (_lib.plain); a no-op otherwise
        q_fp16, k_fp16, v_bf16, O_fp32, lse_fp32 = (_lib.plain(t) for t in ctx.saved_tensors)
        causal = ctx.args
        with torch._C._DisableFuncTorch():
            dO = torch.zeros_like(O_fp32) if dO is None else _lib.plain(dO)
            dq, dk, dv = helion_flash_atten_2_algo_4_bwd(q_fp16, k_fp16, v_bf16, O_fp32, lse_fp32,
                                                         causal, dO)
        return dq, dk, dv, None  # bf16:85


def flash_atten_2_bf16(q_fp16, k_fp16, v_bf16, causal):
    """bf16:87-105: returns O fp32."""
    o_fp32, _lse_fp32 = FlashAttention_2_BF16_autograd_function.apply(q_fp16, k_fp16, v_bf16, causal)
    return o_fp32
