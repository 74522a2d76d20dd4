"""The masked MX-FP4 definition (tests/mxfp4_masked_ref.py) on the CPU: it is the oracle's
bidirectional definition when nothing is masked, its two alignments agree, masked keys cannot
reach the result however large they are, and it stays within the project's end-to-end accuracy
bar (cosine >= 0.95) of exact masked fp32 attention.  tests/test_gpu_mxfp4_causal.py pins the
kernel to this definition.
"""
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import mxfp4_masked_ref as MR
from oracle import mxfp4 as M

HUGE = 60000.0


def test_causal0_is_the_oracle():
    q, k, v = MR.randn_qkv((2, 4, 2, 96, 256))
    O, lse, ops = MR.mxfp4_fwd_masked(q, k, v, 0)
    RO, Rl, rops = M.mxfp4_fwd(q, k, v)
    assert torch.equal(O, RO) and torch.equal(lse, Rl)
    for a, b in zip(ops, rops):
        assert torch.equal(a, b)


def test_chunk_identity():
    """causal = 2 on the last 96 query rows is those rows of the square causal = 1 call."""
    q, k, v = MR.randn_qkv((1, 2, 2, 256, 256))
    O1, l1, _ = MR.mxfp4_fwd_masked(q, k, v, 1)
    O2, l2, _ = MR.mxfp4_fwd_masked(q[:, :, 160:], k, v, 2)
    assert torch.equal(O2, O1[:, :, 160:])
    assert torch.equal(l2, l1[:, 160:])


def test_later_tiles_are_ignored():
    q, k, v = MR.randn_qkv((1, 2, 2, 128, 256))
    O, lse, _ = MR.mxfp4_fwd_masked(q, k, v, 1)
    k2, v2 = k.clone(), v.clone()
    k2[:, :, 128:] = HUGE
    v2[:, :, 128:] = HUGE
    O2, lse2, _ = MR.mxfp4_fwd_masked(q, k2, v2, 1)
    assert torch.equal(O2, O) and torch.equal(lse2, lse)


def test_masked_keys_in_the_own_tile_are_ignored():
    q, k, v = MR.randn_qkv((1, 2, 2, 128, 128))
    O, lse, _ = MR.mxfp4_fwd_masked(q, k, v, 1)
    k2 = k.clone()
    k2[:, :, 32:64] = HUGE
    O2, lse2, _ = MR.mxfp4_fwd_masked(q, k2, v, 1)
    assert torch.equal(O2[:, :, :32], O[:, :, :32]) and torch.equal(lse2[:, :32], lse[:, :32])
    assert torch.isfinite(O2.float()).all() and torch.isfinite(lse2).all()


@pytest.mark.parametrize("case", MR.CASES)
def test_definition_accuracy_randn(case):
    q, k, v, O, lse, _ = MR.case_reference(case)
    cos = MR.cosine(O, MR.exact_masked_attention(q, k, v, case[-1]))
    print(f"MXFP4-CAUSAL-DEF {case} cos {cos:.4f}")
    assert cos >= 0.95, cos


@pytest.mark.parametrize("Sq,Sk,causal", [(512, 512, 1), (256, 512, 2)])
def test_definition_accuracy_smoothed(Sq, Sk, causal):
    """The existing accuracy test's inputs (a large shared key offset, smoothed) made causal."""
    q, k, v = MR.accuracy_inputs(Sq, Sk)
    O, _, _ = MR.mxfp4_fwd_masked(q, MR.smooth_fp16(k), v, causal)
    cos = MR.cosine(O, MR.exact_masked_attention(q, k, v, causal))
    print(f"MXFP4-CAUSAL-DEF smoothed ({Sq},{Sk}) causal={causal} cos {cos:.4f}")
    assert cos >= 0.95, cos


def test_op_registered_and_fake_shape():
    import quantizedattention_amd.ops as ops
    assert hasattr(torch.ops.qattn, "mxfp4_fwd_ex") and "mxfp4_fwd_ex" in ops.__all__
    op = torch.ops.qattn.mxfp4_fwd_ex.default
    assert torch._C._dispatch_has_kernel_for_dispatch_key(op.name(), "CUDA")
    assert not torch._C._dispatch_has_kernel_for_dispatch_key(op.name(), "CPU")
    with FakeTensorMode():
        q = torch.empty((2, 8, 256, 128), dtype=torch.float16, device="cuda")
        k = torch.empty((2, 2, 512, 128), dtype=torch.float16, device="cuda")
        for c in (0, 1, 2):
            O = torch.ops.qattn.mxfp4_fwd_ex(q, k, k, c)
            assert O.shape == q.shape and O.dtype == torch.float16
