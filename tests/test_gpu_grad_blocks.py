"""Gradients of the int8 and bf16 backwards against the oracle, 32-row block by 32-row block
(tests/grad_blocks.py; what the instrument sees is shown on the CPU in tests/test_grad_blocks.py).

Inputs: the ladder (every block of q, k, v and dO with a multiplier of its own, neighbours a factor of
two apart, so a neighbouring block's sq / sk / sv / sdO, lse or D row puts a block off by 50 % or more)
and the lit tile (dO zero outside one 32-row query tile of one query head: exact zeros everywhere that
tile cannot reach, and every key block of dk / dv on the lit head is one (query tile, key tile) pair).
Shapes (grad_blocks.SHAPES): 288 / 320 keys are a full 256-key dK+dV workgroup and a 32- / 64-key one,
whose second, staggered half of the 8 waves idles; 5, 6 and 9 query tiles wrap the 4-slot rings;
grouped and odd head counts; D = 64 and 128; two causal cases with 6 key/value heads.

Bars: every block within 3 * INT8_BWD_REL (= INT8_BWD_REL_FUZZ) for int8 and 3e-2 for bf16, no block
left out and no floor under a denominator; a block the oracle has exactly zero must be exactly zero.
The whole-tensor bars of tests/test_gpu_int8.py and tests/test_gpu_bf16.py are asserted beside them.
Every maximum is printed as ``RELL2-BLOCK <path> <grad> <value>``; DESIGN.md §4 has the measured ones.
"""
import pytest
import torch

import grad_blocks as GB
from conftest import INT8_BWD_REL

from oracle import restate as R

pytestmark = pytest.mark.gpu

INT8_BLOCK_REL = 3 * INT8_BWD_REL

# the record backward with one key/value head per workspace chunk, and the recomputing backward
INT8_PATHS = (("records", dict(use_ws=True, ws_chunk=1)), ("recompute", dict(use_ws=False)))
BF16_ENTRIES = ("ws", "qattn_bf16_bwd_ex")


def _int8(shape, q, k, v, dO, tag):
    """Forward on the GPU, the oracle's backward on the forward's own outputs, both GPU backwards."""
    from quantizedattention_amd.attention_int8 import _int8_backward, helion_atten_int8_hl_dot_fwd
    causal, Hkv = shape[6], shape[2]
    q, k, v, dO = q.half(), k.half(), v.half(), dO.half()
    assert torch.isfinite(R.int8_fwd(q, k, v, causal=causal)[0].float()).all()
    O, lse, qi, kiT, vi, sq, sk, sv, _, _ = helion_atten_int8_hl_dot_fwd(q.cuda(), k.cuda(), v.cuda(),
                                                                        causal=causal)
    ref = R.int8_bwd(dO, qi.cpu(), sq.cpu(), kiT.cpu(), None, sk.cpu(), vi.cpu(), sv.cpu(), O.cpu(),
                     lse.cpu(), causal=causal, kv_heads=Hkv)
    out = []
    for name, kw in INT8_PATHS:
        grads = _int8_backward(dO.cuda(), qi, sq, kiT, sk, vi, sv, O, lse, causal=causal, kv_heads=Hkv, **kw)
        torch.cuda.synchronize()
        GB.check(f"int8-{tag}-{name}", grads, ref, INT8_BLOCK_REL, INT8_BWD_REL)
        out.append(grads)
    return ref, out


def _bf16(shape, q, k, v, dO, tag, monkeypatch):
    from quantizedattention_amd import attention_bf16 as A
    causal = shape[6]
    q, k, v = q.half(), k.half(), v.bfloat16()
    assert torch.isfinite(R.bf16_fwd(q, k, v, causal, kt=16)[0]).all()
    O, lse = A.helion_atten_bf16_fwd_training(q.cuda(), k.cuda(), v.cuda(), causal)
    ref = GB.flush_denormals(*R.bf16_bwd(q, k, v, O.cpu(), lse.cpu(), causal, dO))
    out = []
    for entry in BF16_ENTRIES:
        monkeypatch.setattr(A, "_BWD_ENTRY", entry)
        grads = A.helion_flash_atten_2_algo_4_bwd(q.cuda(), k.cuda(), v.cuda(), O, lse, causal, dO.cuda())
        torch.cuda.synchronize()
        GB.check(f"bf16-{tag}-{entry}", grads, ref, GB.BF16_BLOCK_REL, GB.BF16_BWD_REL)
        out.append(grads)
    return ref, out


@pytest.mark.parametrize("shape", GB.SHAPES, ids=GB.shape_id)
def test_int8_ladder_blocks(lib, shape):
    (q, k, v, dO), _ = GB.ladder_inputs(shape, "int8", seed=201)
    _int8(shape, q, k, v, dO, "ladder")


@pytest.mark.parametrize("shape", GB.SHAPES, ids=GB.shape_id)
def test_int8_lit_tile(lib, shape):
    """dO lit on one query tile: dq outside its rows, dk / dv of every other key/value head and batch
    entry and (causal) of every key tile past it are exactly zero, in the oracle and on the GPU, and
    the single pairs that make up dk / dv of the lit head each sit within the per-block bar."""
    q, k, v = GB.randn_inputs(shape, 202)
    ref, outs = _int8(shape, q, k, v, GB.lit_dO(shape, 203), "lit")
    GB.assert_lit_zeros(shape, *ref, "R.int8_bwd")
    for (name, _), grads in zip(INT8_PATHS, outs):
        GB.assert_lit_zeros(shape, *grads, name)


@pytest.mark.parametrize("shape", GB.SHAPES, ids=GB.shape_id)
def test_bf16_ladder_blocks(lib, monkeypatch, shape):
    (q, k, v, dO), _ = GB.ladder_inputs(shape, "bf16", seed=204)
    _bf16(shape, q, k, v, dO, "ladder", monkeypatch)


@pytest.mark.parametrize("shape", GB.SHAPES, ids=GB.shape_id)
def test_bf16_lit_tile(lib, monkeypatch, shape):
    """As test_int8_lit_tile.  (The restatement's causal fill leaves fp32 denormals where the GPU has
    zeros; they are read as zeros, grad_blocks.flush_denormals.)"""
    q, k, v = GB.randn_inputs(shape, 205)
    ref, outs = _bf16(shape, q, k, v, GB.lit_dO(shape, 206), "lit", monkeypatch)
    GB.assert_lit_zeros(shape, *ref, "R.bf16_bwd")
    for entry, grads in zip(BF16_ENTRIES, outs):
        GB.assert_lit_zeros(shape, *grads, entry)
