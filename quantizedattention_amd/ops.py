"""The ``qattn::`` dispatcher operators ("C++ op layer").

The operators are defined and implemented in C++ (``csrc/torch/qattn_ops.cpp`` ->
``libqattn_torch.so``: ``TORCH_LIBRARY(qattn)`` schemas, CUDA-key kernels that allocate the outputs,
enter a HIP device guard and enqueue the C-ABI kernels of ``include/qattn.h`` on torch's current
stream).  This module loads that library and adds what belongs to the Python side of an operator:
its fake (meta) implementation, for graph capture (``torch.compile``, ``torch.export``, FX), and
the autograd rules of ``int8_fwd`` and ``bf16_fwd`` (their backward operators).

    torch.ops.qattn.int8_quant(x, block) -> (idx, scale)
    torch.ops.qattn.int8_fwd(q, k, v, smooth, causal) -> (O, lse, q_i8, k_i8, v_i8, sq, sk, sv)
    torch.ops.qattn.int8_bwd(dO, q_i8, sq, k_i8, sk, v_i8, sv, O, lse, causal, kv_heads)
        -> (dq, dk, dv)
    torch.ops.qattn.bf16_fwd(q, k, v, causal) -> (O, lse)
    torch.ops.qattn.bf16_bwd(q, k, v, O, lse, causal, dO) -> (dq, dk, dv)
    torch.ops.qattn.jvp_fwd(q, k, v, tq, tk, tv) -> (O, tO, lse)
    torch.ops.qattn.mxfp4_fwd(q, k, v) -> O
    torch.ops.qattn.mxfp4_fwd_ex(q, k, v, causal) -> O      (causal 0 / 1 top-left / 2 bottom-right)
    torch.ops.qattn.mxfp4_cached(q, k4, ks, vt, vs, causal, keys_per_split) -> (O, lse)
    torch.ops.qattn.mxfp4_decode(q, k4, ks, vt, vs, lens, sk_max, causal, keys_per_split) -> (O, lse)
    torch.ops.qattn.mxfp4_decode_paged(q, k4, ks, vt, vs, lens, block_table, sk_max, causal,
                                       keys_per_split) -> (O, lse)
    torch.ops.qattn.mxfp4_varlen_paged(q, k4, ks, vt, vs, lens, block_table, seq_rec, work, part_rows,
                                       causal, keys_per_split) -> (O, lse)
    torch.ops.qattn.mxfp4_varlen_paged_window(q, k4, ks, vt, vs, lens, block_table, seq_rec, work,
                                              part_rows, causal, keys_per_split, window, sinks) -> (O, lse)
    torch.ops.qattn.mxfp4_varlen_paged_shared(q, k4, ks, vt, vs, lens, block_table, seq_rec, work, grp_rec,
                                              members, part_rows, causal, keys_per_split) -> (O, lse)
    torch.ops.qattn.mxfp4_varlen_paged_tree(q, k4, ks, vt, vs, lens, block_table, seq_rec, work, tree_masks,
                                            part_rows, causal, keys_per_split) -> (O, lse)
    torch.ops.qattn.mxfp4_quant_rows_rope(x, cos_sin, pos, interleaved) -> (q4, qs)
    torch.ops.qattn.mxfp4_varlen_paged_rope(q, k4, ks, vt, vs, lens, block_table, seq_rec, work, part_rows,
                                            causal, keys_per_split, cos_sin, pos, interleaved) -> (O, lse)
    torch.ops.qattn.mxfp4_decode_step_plan(slots, lens, capacity, kv_heads, group, keys_per_split, splits,
                                           window, sinks) -> (seq_tab, tiles, pos, seq_rec)
    torch.ops.qattn.mxfp4_decode_step(q, k4, ks, vt, vs, lens, block_table, seq_rec, work, splits,
                                      keys_per_split, window, sinks) -> (O, lse)
    torch.ops.qattn.mxfp4_verify_step_plan(slots, lens, tree, draft_tokens, capacity, kv_heads, group,
                                           keys_per_split, splits) -> (seq_tab, tiles, pos, seq_rec)
    torch.ops.qattn.mxfp4_verify_step(q, k4, ks, vt, vs, lens, block_table, seq_rec, work, tree, draft_tokens,
                                      splits, keys_per_split) -> (O, lse)

Shapes follow the drop-in functions (attention_int8.py:259-262 for the int8 outputs) except that
k_i8 is returned row-major [B*Hkv*Sk, D] (the drop-in's k_i8T is its transposed view: an operator
output may not be a view).  There is no CPU kernel, as for the drop-in functions: a CPU tensor
raises NotImplementedError from the dispatcher.  The Python wrappers below only forward to
``torch.ops.qattn`` (the names existing callers import).
"""
from __future__ import annotations

import itertools

import torch

from . import _lib

__all__ = ["int8_quant", "int8_fwd", "int8_bwd", "bf16_fwd", "bf16_bwd", "jvp_fwd", "mxfp4_fwd",
           "mxfp4_fwd_ex", "mxfp4_cached", "mxfp4_decode", "mxfp4_decode_paged", "mxfp4_varlen_paged",
           "mxfp4_quant_rows_rope", "mxfp4_decode_step_plan", "mxfp4_decode_step",
           "mxfp4_verify_step_plan", "mxfp4_verify_step"]

_lib.load_ops()
_ops = torch.ops.qattn


# ---------------------------------------------------------------------------- fake kernels
@torch.library.register_fake("qattn::int8_quant")
def _(x, block):
    return (x.new_empty(x.shape, dtype=torch.int8),
            x.new_empty((*x.shape[:-2], x.shape[-2] // 32), dtype=torch.float16))


@torch.library.register_fake("qattn::int8_fwd")
def _(q, k, v, smooth, causal):
    B, H, S, D = q.shape
    Nq, Nkv = B * H * S, k.shape[0] * k.shape[1] * k.shape[2]
    e = lambda *s, dt: q.new_empty(s, dtype=dt)  # noqa: E731
    return (e(B, H, S, D, dt=torch.float16), e(Nq, dt=torch.float16), e(Nq, D, dt=torch.int8),
            e(Nkv, D, dt=torch.int8), e(Nkv, D, dt=torch.int8), e(Nq // 32, dt=torch.float16),
            e(Nkv // 32, dt=torch.float16), e(Nkv // 32, dt=torch.float16))


@torch.library.register_fake("qattn::int8_bwd")
def _(dO, q_i8, sq, k_i8, sk, v_i8, sv, O, lse, causal, kv_heads):
    B, H, S, D = O.shape
    Sk = k_i8.shape[0] // (B * kv_heads)
    return (O.new_empty((B, H, S, D), dtype=torch.float16),
            O.new_empty((B, kv_heads, Sk, D), dtype=torch.float16),
            O.new_empty((B, kv_heads, Sk, D), dtype=torch.float16))


@torch.library.register_fake("qattn::bf16_fwd")
def _(q, k, v, causal):
    B, H, S, D = q.shape
    return (q.new_empty((B, H, S, D), dtype=torch.float32),
            q.new_empty((B * H, S), dtype=torch.float32))


@torch.library.register_fake("qattn::bf16_bwd")
def _(q, k, v, O, lse, causal, dO):
    return (q.new_empty(q.shape, dtype=torch.float32), k.new_empty(k.shape, dtype=torch.float32),
            v.new_empty(v.shape, dtype=torch.float32))


@torch.library.register_fake("qattn::jvp_fwd")
def _(q, k, v, tq, tk, tv):
    B, H, S, D = q.shape
    return (q.new_empty((B, H, S, D), dtype=torch.float32),
            q.new_empty((B, H, S, D), dtype=torch.float32),
            q.new_empty((B * H, S), dtype=torch.float32))


@torch.library.register_fake("qattn::mxfp4_fwd")
def _(q, k, v):
    return q.new_empty(q.shape, dtype=torch.float16)


@torch.library.register_fake("qattn::mxfp4_fwd_ex")
def _(q, k, v, causal):
    return q.new_empty(q.shape, dtype=torch.float16)


@torch.library.register_fake("qattn::mxfp4_cached")
def _(q, k4, ks, vt, vs, causal, keys_per_split):
    B, H, S, D = q.shape
    return (q.new_empty((B, H, S, D), dtype=torch.float16),
            q.new_empty((B * H, S), dtype=torch.float32))


@torch.library.register_fake("qattn::mxfp4_decode")
def _(q, k4, ks, vt, vs, lens, sk_max, causal, keys_per_split):
    B, H, S, D = q.shape
    return (q.new_empty((B, H, S, D), dtype=torch.float16),
            q.new_empty((B * H, S), dtype=torch.float32))


@torch.library.register_fake("qattn::mxfp4_decode_paged")
def _(q, k4, ks, vt, vs, lens, block_table, sk_max, causal, keys_per_split):
    B, H, S, D = q.shape
    return (q.new_empty((B, H, S, D), dtype=torch.float16),
            q.new_empty((B * H, S), dtype=torch.float32))


@torch.library.register_fake("qattn::mxfp4_varlen_paged")
def _(q, k4, ks, vt, vs, lens, block_table, seq_rec, work, part_rows, causal, keys_per_split):
    T, H, D = q.shape
    return (q.new_empty((T, H, D), dtype=torch.float16), q.new_empty((T, H), dtype=torch.float32))


@torch.library.register_fake("qattn::mxfp4_varlen_paged_window")
def _(q, k4, ks, vt, vs, lens, block_table, seq_rec, work, part_rows, causal, keys_per_split, window, sinks):
    T, H, D = q.shape
    return (q.new_empty((T, H, D), dtype=torch.float16), q.new_empty((T, H), dtype=torch.float32))


@torch.library.register_fake("qattn::mxfp4_varlen_paged_shared")
def _(q, k4, ks, vt, vs, lens, block_table, seq_rec, work, grp_rec, members, part_rows, causal, keys_per_split):
    T, H, D = q.shape
    return (q.new_empty((T, H, D), dtype=torch.float16), q.new_empty((T, H), dtype=torch.float32))


@torch.library.register_fake("qattn::mxfp4_varlen_paged_tree")
def _(q, k4, ks, vt, vs, lens, block_table, seq_rec, work, tree_masks, part_rows, causal, keys_per_split):
    T, H, D = q.shape
    return (q.new_empty((T, H, D), dtype=torch.float16), q.new_empty((T, H), dtype=torch.float32))


@torch.library.register_fake("qattn::mxfp4_quant_rows_rope")
def _(x, cos_sin, pos, interleaved):
    T, H, D = x.shape
    return (x.new_empty((T * H, D // 2), dtype=torch.uint8), x.new_empty((T * H, D // 32), dtype=torch.uint8))


@torch.library.register_fake("qattn::mxfp4_varlen_paged_rope")
def _(q, k4, ks, vt, vs, lens, block_table, seq_rec, work, part_rows, causal, keys_per_split, cos_sin, pos,
      interleaved):
    T, H, D = q.shape
    return (q.new_empty((T, H, D), dtype=torch.float16), q.new_empty((T, H), dtype=torch.float32))


@torch.library.register_fake("qattn::mxfp4_decode_step_plan")
def _(slots, lens, capacity, kv_heads, group, keys_per_split, splits, window, sinks):
    n = slots.shape[0]
    e = lambda *s: slots.new_empty(s, dtype=torch.int32)  # noqa: E731
    return e(n, 4), e(n, 2), e(n), e(n, 8)


@torch.library.register_fake("qattn::mxfp4_decode_step")
def _(q, k4, ks, vt, vs, lens, block_table, seq_rec, work, splits, keys_per_split, window, sinks):
    T, H, D = q.shape
    return (q.new_empty((T, H, D), dtype=torch.float16), q.new_empty((T, H), dtype=torch.float32))


@torch.library.register_fake("qattn::mxfp4_verify_step_plan")
def _(slots, lens, tree, draft_tokens, capacity, kv_heads, group, keys_per_split, splits):
    n = slots.shape[0]
    e = lambda *s: slots.new_empty(s, dtype=torch.int32)  # noqa: E731
    return e(n, 4), e(2 * n, 2), e(n * draft_tokens), e(n, 8)


@torch.library.register_fake("qattn::mxfp4_verify_step")
def _(q, k4, ks, vt, vs, lens, block_table, seq_rec, work, tree, draft_tokens, splits, keys_per_split):
    T, H, D = q.shape
    return (q.new_empty((T, H, D), dtype=torch.float16), q.new_empty((T, H), dtype=torch.float32))


# ---------------------------------------------------------------------------- autograd rules
def _int8_setup(ctx, inputs, output):
    q, k, v, smooth, causal = inputs[:5]
    ctx.n_inputs = len(inputs)
    O, lse, q_i8, k_i8, v_i8, sq, sk, sv = output
    ctx.save_for_backward(O, lse, q_i8, k_i8, v_i8, sq, sk, sv)
    ctx.causal, ctx.kv_heads = causal, k.shape[1]
    ctx.dtypes = (q.dtype, k.dtype, v.dtype)
    ctx.kv_shape = k.shape


def _int8_backward_rule(ctx, dO, *_unused):
    # gradient of O only (the quantised outputs are not differentiable, int8:52-56); k smoothing
    # adds no gradient (softmax-invariant), so the same backward serves smooth and plain forwards
    O, lse, q_i8, k_i8, v_i8, sq, sk, sv = ctx.saved_tensors
    rest = (None,) * (ctx.n_inputs - 3)   # smooth, causal
    if dO is None:
        return (None, None, None) + rest
    qd, kd, vd = ctx.dtypes
    if O.numel() == 0 or k_i8.numel() == 0:   # nothing attends (an empty batch): zero gradients
        z = dict(device=O.device)
        return (torch.zeros(O.shape, dtype=qd, **z), torch.zeros(ctx.kv_shape, dtype=kd, **z),
                torch.zeros(ctx.kv_shape, dtype=vd, **z)) + rest
    dq, dk, dv = _ops.int8_bwd(dO.to(torch.float16), q_i8, sq, k_i8, sk, v_i8, sv, O, lse, ctx.causal,
                               ctx.kv_heads)
    return (dq.to(qd), dk.to(kd), dv.to(vd)) + rest


torch.library.register_autograd("qattn::int8_fwd", _int8_backward_rule, setup_context=_int8_setup)


def _bf16_setup(ctx, inputs, output):
    q, k, v, causal = inputs
    O, lse = output
    ctx.save_for_backward(q, k, v, O, lse)
    ctx.causal = causal


def _bf16_backward_rule(ctx, dO, _dlse):
    q, k, v, O, lse = ctx.saved_tensors
    if dO is None:
        return None, None, None, None
    dq, dk, dv = _ops.bf16_bwd(q, k, v, O, lse, ctx.causal, dO)
    return dq.to(q.dtype), dk.to(k.dtype), dv.to(v.dtype), None


torch.library.register_autograd("qattn::bf16_fwd", _bf16_backward_rule, setup_context=_bf16_setup)


# ---------------------------------------------------------------------------- Python names
def int8_quant(x, block):
    """Per-32-token block quantiser (attention_int8.py:178-186): x fp16 [..., S, D] ->
    (idx int8 [..., S, D], scale fp16 [..., S/32]); s = f16(amax/127), idx = trunc(f16(x/s))."""
    return _ops.int8_quant(x, block)


def int8_fwd(q, k, v, smooth, causal):
    """SageAttention-3 int8 forward (attention_int8.py:97-262, per (batch, head)); the same kernels
    as ``sage_attention_3_int8``."""
    return _ops.int8_fwd(q, k, v, smooth, causal)


def int8_bwd(dO, q_i8, sq, k_i8, sk, v_i8, sv, O, lse, causal, kv_heads):
    """Corrected int8 backward (attention_int8.py:264-432); k_i8 row-major."""
    return _ops.int8_bwd(dO, q_i8, sq, k_i8, sk, v_i8, sv, O, lse, causal, kv_heads)


def bf16_fwd(q, k, v, causal):
    """FA2 forward with the corrected beta rule (attention_bf16.py:107-296): (O fp32, lse fp32)."""
    return _ops.bf16_fwd(q, k, v, causal)


def bf16_bwd(q, k, v, O, lse, causal, dO):
    """FA2 algorithm-4 backward, corrected (attention_bf16.py:299-448): fp32 grads."""
    return _ops.bf16_bwd(q, k, v, O, lse, causal, dO)


def jvp_fwd(q, k, v, tq, tk, tv):
    """Attention with its forward-mode tangent (attention_jvp.py:24-195): (O, tO, lse) fp32."""
    return _ops.jvp_fwd(q, k, v, tq, tk, tv)


def mxfp4_fwd(q, k, v):
    """MX-FP4 inference forward, k smoothed: O fp16."""
    return _ops.mxfp4_fwd(q, k, v)


def mxfp4_fwd_ex(q, k, v, causal):
    """``mxfp4_fwd`` with a causal mask: 0 none, 1 top-left, 2 bottom-right (Sk >= Sq); the same
    kernels as ``sage_attention_3_fp4(q, k, v, causal=causal)``."""
    return _ops.mxfp4_fwd_ex(q, k, v, int(causal))


def mxfp4_cached(q, kv, causal=False, keys_per_split=None):
    """``kv_cache_mxfp4.attention_mxfp4_cached`` as one operator: q [B, Hq, Sq, 128] (any Sq >= 1)
    against a ``QuantizedKVFP4`` -> (O fp16, lse fp32 [B*Hq, Sq]); ``keys_per_split`` None: the plan."""
    return _ops.mxfp4_cached(q, kv.k4, kv.ks, kv.vt, kv.vs, int(bool(causal)),
                             0 if keys_per_split is None else int(keys_per_split))


def mxfp4_decode(q, cache, causal=False, keys_per_split=None):
    """``kv_cache_mxfp4.attention_mxfp4_decode`` as one operator: q [B, Hq, Sq, 128] against a
    ``PreallocatedKVFP4``, sequence b over its own length -> (O fp16, lse fp32 [B*Hq, Sq]).  The
    lengths are checked here, on the cache's host mirror (the operator reads only ``lens`` on the
    device); ``keys_per_split`` None: the plan."""
    from .kv_cache_mxfp4 import _decode_plan
    _, _, sk_max, _, _ = _decode_plan(q, cache, causal, keys_per_split)
    return _ops.mxfp4_decode(q, cache.k4, cache.ks, cache.vt, cache.vs, cache.lens, sk_max,
                             int(bool(causal)), 0 if keys_per_split is None else int(keys_per_split))


def mxfp4_decode_paged(q, cache, causal=False, keys_per_split=None):
    """``kv_cache_mxfp4.attention_mxfp4_decode_paged`` as one operator: q [max_seqs, Hq, Sq, 128]
    against a ``PagedKVFP4``, sequence b over its own length and pages -> (O fp16, lse fp32
    [max_seqs*Hq, Sq]).  The lengths are checked here, on the cache's host mirror (the operator reads
    only ``lens`` and ``block_table`` on the device); ``keys_per_split`` None: the plan."""
    from .kv_cache_mxfp4 import PagedKVFP4, _decode_plan
    _, _, sk_max, _, _ = _decode_plan(q, cache, causal, keys_per_split, PagedKVFP4)
    return _ops.mxfp4_decode_paged(q, cache.k4, cache.ks, cache.vt, cache.vs, cache.lens, cache.block_table,
                                   sk_max, int(bool(causal)), 0 if keys_per_split is None else int(keys_per_split))


def mxfp4_quant_rows_rope(x, rope, positions):
    """``attention_mxfp4.mxfp4_quantize_rows_rope`` as one operator: packed x [T, H, 128] rotated by its
    tokens' positions through ``rope`` (a ``Rope``), then quantised -> (q4 u8 [T*H, 64], qs u8 [T*H, 4]).
    Host ``positions`` are checked against the table and uploaded here; a device int32 tensor is passed on."""
    from .attention_mxfp4 import Rope, _device_positions, _host_positions
    if not isinstance(rope, Rope):
        raise _lib.QAttnError("qattn mxfp4 rope: rope must be a Rope")
    if x.dim() != 3:
        raise _lib.QAttnError("qattn mxfp4 rope: packed rows must be x [T, H, 128]")
    if not _device_positions(positions, x.shape[0]):
        positions = _host_positions(positions, x.shape[0], rope.max_pos).to(x.device, non_blocking=True)
    return _ops.mxfp4_quant_rows_rope(x, rope.table, positions, rope.interleaved)


def mxfp4_varlen_paged(q, cache, seq_ids, q_lens, causal=False, keys_per_split=None, window=None, sinks=0,
                       share_prefix=False, tree=None, rope=None, positions=None):
    """``kv_cache_mxfp4.attention_mxfp4_varlen_paged`` as one operator: packed q [T, Hq, 128] against
    a ``PagedKVFP4``, the ``q_lens[j]`` tokens of slot ``seq_ids[j]`` over that sequence's own length
    and pages -> (O fp16 [T, Hq, 128], lse fp32 [T, Hq]).  The plan (``plan_varlen``) is made and checked
    here, on the cache's host mirror, and its two tables are uploaded without a synchronisation; the
    operator reads only ``lens``, ``block_table`` and the tables on the device.  ``window`` (with
    ``sinks``) routes to ``torch.ops.qattn.mxfp4_varlen_paged_window``: a sliding window with sinks, as the
    Python call's.  ``share_prefix=True`` (without a window) routes to
    ``torch.ops.qattn.mxfp4_varlen_paged_shared`` with the tables of ``plan_varlen_shared`` when the listed
    sequences hold leading pages in common (``PagedKVFP4.prefix_groups``), and to the plain operator when
    they do not: the same bits either way.  ``tree`` (causal only, without a window or ``share_prefix``; one
    entry per sequence, None or a ``parents`` list) routes to ``torch.ops.qattn.mxfp4_varlen_paged_tree``, the
    tree-masked verify step of the Python call, and to the plain operator when every entry is None.  ``rope``
    (with ``positions``, as the Python call's; without a window, ``share_prefix`` or ``tree``: those
    combinations are the Python call's alone) routes to ``torch.ops.qattn.mxfp4_varlen_paged_rope``."""
    from .kv_cache_mxfp4 import (PagedKVFP4, _check_trimmed, _packed_lists, _query_positions, _shared_plan,
                                 _tree_args, _window_args, plan_varlen)
    if not isinstance(cache, PagedKVFP4):
        raise _lib.QAttnError("qattn mxfp4 kv cache: cache must be a PagedKVFP4")
    if q.dim() != 3:
        raise _lib.QAttnError("qattn mxfp4 paged cache: packed queries must be q [T, Hq, 128]")
    ids, sq = _packed_lists(cache.alloc.max_seqs, seq_ids, q_lens, "q_lens")
    if sum(sq) != q.shape[0]:
        raise _lib.QAttnError(f"qattn mxfp4 paged cache: q holds {q.shape[0]} tokens, q_lens sum to {sum(sq)}")
    if (rope is not None or positions is not None) and (window is not None or share_prefix or tree is not None):
        raise _lib.QAttnError("qattn mxfp4 rope: the rope operator takes no window, share_prefix or tree; "
                              "kv_cache_mxfp4.attention_mxfp4_varlen_paged serves those with rope=")
    trees = None if tree is None else _tree_args(tree, sq, causal, window, share_prefix)
    if trees is not None:
        kps, seq_rec, work, part_rows = plan_varlen(cache.lengths, ids, sq, q.shape[1], cache.k4.shape[1],
                                                    keys_per_split, causal, None, 0, trees[0])
        _check_trimmed(cache, ids, sq, None, 0)
        _lib.require_gpu(q, cache.k4)
        # one upload: the two tables, then the ancestor words
        flat = torch.tensor(list(itertools.chain.from_iterable(seq_rec + work)), dtype=torch.int32)
        flat = torch.cat([flat, trees[1]]).to(q.device, non_blocking=True)
        a, b = 8 * len(seq_rec), 8 * len(seq_rec) + 4 * len(work)
        return _ops.mxfp4_varlen_paged_tree(q, cache.k4, cache.ks, cache.vt, cache.vs, cache.lens,
                                            cache.block_table, flat[:a].view(-1, 8), flat[a:b].view(-1, 4),
                                            flat[b:].view(torch.int64), part_rows, 1, kps)
    shared = _shared_plan(cache, ids, sq, q.shape[1], keys_per_split, causal, window) if share_prefix else None
    if shared is not None:
        kps, seq_rec, work, part_rows, grp_rec, members = shared
        _check_trimmed(cache, ids, sq, None, 0)
        _lib.require_gpu(q, cache.k4)
        # one upload of the four tables, cut into views
        flat = torch.tensor(list(itertools.chain.from_iterable(seq_rec + work + grp_rec + members)),
                            dtype=torch.int32).to(q.device, non_blocking=True)
        cut = itertools.accumulate((0, 8 * len(seq_rec), 4 * len(work), 4 * len(grp_rec), 2 * len(members)))
        cut = list(cut)
        rec_d, work_d, grp_d, mem_d = (flat[a:b].view(-1, w) for a, b, w in zip(cut, cut[1:], (8, 4, 4, 2)))
        return _ops.mxfp4_varlen_paged_shared(q, cache.k4, cache.ks, cache.vt, cache.vs, cache.lens,
                                              cache.block_table, rec_d, work_d, grp_d, mem_d, part_rows,
                                              int(bool(causal)), kps)
    kps, seq_rec, work, part_rows = plan_varlen(cache.lengths, ids, sq, q.shape[1], cache.k4.shape[1],
                                                keys_per_split, causal, window, sinks)
    W, S = _window_args(window, sinks)
    _check_trimmed(cache, ids, sq, W, S)
    pos = _query_positions(cache, ids, sq, None, rope, positions)
    _lib.require_gpu(q, cache.k4)
    rec_d = torch.tensor(seq_rec, dtype=torch.int32).to(q.device, non_blocking=True)
    work_d = torch.tensor(work, dtype=torch.int32).to(q.device, non_blocking=True)
    if rope is not None:
        return _ops.mxfp4_varlen_paged_rope(q, cache.k4, cache.ks, cache.vt, cache.vs, cache.lens,
                                            cache.block_table, rec_d, work_d, part_rows, int(bool(causal)), kps,
                                            rope.table, pos.to(q.device, non_blocking=True), rope.interleaved)
    if W is not None:
        return _ops.mxfp4_varlen_paged_window(q, cache.k4, cache.ks, cache.vt, cache.vs, cache.lens,
                                              cache.block_table, rec_d, work_d, part_rows, int(bool(causal)),
                                              kps, min(W, 1 << 26), min(S, 1 << 26))
    return _ops.mxfp4_varlen_paged(q, cache.k4, cache.ks, cache.vt, cache.vs, cache.lens, cache.block_table,
                                   rec_d, work_d, part_rows, int(bool(causal)), kps)


def mxfp4_decode_step_plan(step, cache):
    """The tables of ``kv_cache_mxfp4.DecodeStep.append`` as one operator: from ``step.slots`` (what
    ``step.prepare`` uploaded) and ``cache.lens``, the lengths BEFORE the step's append -> new device tensors
    (seq_tab [N, 4], tiles [N, 2], pos [N], seq_rec [N, 8]), what ``qattn_mxfp4_decode_step_plan`` writes into
    the step's own tables."""
    a = cache.alloc
    return _ops.mxfp4_decode_step_plan(step.slots, cache.lens, a.max_pages_per_seq * a.page_tokens, step.kv_heads,
                                       step.q_heads // step.kv_heads, step.kps, step.splits, step.window or 0,
                                       step.sinks)


def mxfp4_decode_step(q, step, cache, seq_rec=None):
    """``kv_cache_mxfp4.DecodeStep.attend`` (without ``rope``) as one operator that allocates its outputs: q [N,
    Hq, 128] against ``cache`` after the step's append, over ``seq_rec`` (default: the step's own, which its
    ``append`` wrote) and the step's ``work`` -> (O, lse), the Python call's bits."""
    return _ops.mxfp4_decode_step(q, cache.k4, cache.ks, cache.vt, cache.vs, cache.lens, cache.block_table,
                                  step.seq_rec if seq_rec is None else seq_rec, step.work, step.splits, step.kps,
                                  step.window or 0, step.sinks)


def mxfp4_verify_step_plan(step, cache):
    """The tables of ``kv_cache_mxfp4.VerifyStep.append`` as one operator: from ``step.slots`` and ``step.tree``
    (what ``step.prepare`` uploaded) and ``cache.lens``, the lengths BEFORE the step's append -> new device tensors
    (seq_tab [N, 4], tiles [2 N, 2], pos [N * K], seq_rec [N, 8]), what ``qattn_mxfp4_verify_step_plan`` writes
    into the step's own tables."""
    a = cache.alloc
    return _ops.mxfp4_verify_step_plan(step.slots, cache.lens, step.tree, step.K,
                                       a.max_pages_per_seq * a.page_tokens, step.kv_heads,
                                       step.q_heads // step.kv_heads, step.kps, step.splits)


def mxfp4_verify_step(q, step, cache, seq_rec=None):
    """``kv_cache_mxfp4.VerifyStep.attend`` (without ``rope``) as one operator that allocates its outputs: q [N *
    K, Hq, 128] against ``cache`` after the step's append, over ``seq_rec`` (default: the step's own, which its
    ``append`` wrote), the step's ``work`` and ``tree`` -> (O, lse), the Python call's bits."""
    return _ops.mxfp4_verify_step(q, cache.k4, cache.ks, cache.vt, cache.vs, cache.lens, cache.block_table,
                                  step.seq_rec if seq_rec is None else seq_rec, step.work, step.tree, step.K,
                                  step.splits, step.kps)
