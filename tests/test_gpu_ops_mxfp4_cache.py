"""qattn::mxfp4_cached (csrc/torch/qattn_ops.cpp): the operator equals
kv_cache_mxfp4.attention_mxfp4_cached bit for bit, split and unsplit, its fake kernel gives the right
shapes and dtypes, and it is one graph node under torch.compile(fullgraph=True)."""
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import mxfp4_masked_ref as MR

pytestmark = pytest.mark.gpu


def _setup(shape):
    from quantizedattention_amd.kv_cache_mxfp4 import quantize_kv_fp4
    q, k, v = (t.cuda() for t in MR.randn_qkv(shape))
    return q, quantize_kv_fp4(k, v)


@pytest.mark.parametrize("shape", [(1, 4, 2, 1, 256), (2, 4, 1, 33, 192), (1, 8, 2, 1, 2048)])
def test_operator_equals_the_python_call(lib, shape):
    import quantizedattention_amd.ops as ops
    from quantizedattention_amd.kv_cache_mxfp4 import _split_plan_fp4, attention_mxfp4_cached
    q, kv = _setup(shape)
    Sk = shape[4]
    for causal in (False, True):
        for kps in (None, 64, Sk):                      # the plan, split, one split
            O, lse = attention_mxfp4_cached(q, kv, causal=causal, keys_per_split=kps)
            O2, lse2 = torch.ops.qattn.mxfp4_cached(q, *kv.kv, int(causal), 0 if kps is None else kps)
            assert O2.dtype == torch.float16 and lse2.dtype == torch.float32
            assert torch.equal(O, O2) and torch.equal(lse, lse2), (causal, kps)
            O3, lse3 = ops.mxfp4_cached(q, kv, causal, kps)
            assert torch.equal(O, O3) and torch.equal(lse, lse3)
    if Sk == 2048:   # here the plan itself splits
        assert _split_plan_fp4(shape[0] * shape[2], (shape[1] // shape[2]) * shape[3], Sk) == 1024


def test_fake_kernel_and_one_graph_node(lib):
    import quantizedattention_amd.ops  # noqa: F401
    q, kv = _setup((2, 4, 2, 5, 128))
    with FakeTensorMode() as mode:
        fq = torch.empty((2, 8, 3, 128), dtype=torch.float16, device="cuda")
        u8 = lambda *s: torch.empty(s, dtype=torch.uint8, device="cuda")  # noqa: E731
        O, lse = torch.ops.qattn.mxfp4_cached(fq, u8(2, 2, 256, 64), u8(2, 2, 256, 4), u8(4, 4, 128, 32),
                                              u8(4, 4, 128, 2), 1, 0)
        assert O.shape == (2, 8, 3, 128) and O.dtype == torch.float16 and O.device.type == "cuda"
        assert lse.shape == (16, 3) and lse.dtype == torch.float32
    assert mode is not None

    def f(q, k4, ks, vt, vs):
        O, lse = torch.ops.qattn.mxfp4_cached(q, k4, ks, vt, vs, 1, 64)
        return O.float() * 2.0 + lse.view(2, 4, 5, 1)

    graphs = []

    def backend(gm, example_inputs):
        graphs.append(gm)
        return gm.forward

    cf = torch.compile(f, backend=backend, fullgraph=True)
    assert torch.equal(cf(q, *kv.kv), f(q, *kv.kv))
    assert len(graphs) == 1
    calls = [n for n in graphs[0].graph.nodes if n.op == "call_function" and "mxfp4_cached" in str(n.target)]
    assert len(calls) == 1


def test_operator_refusals(lib):
    q, kv = _setup((1, 4, 2, 8, 128))
    op = torch.ops.qattn.mxfp4_cached
    with pytest.raises(RuntimeError):
        op(q, *kv.kv, 0, 96)
    with pytest.raises(RuntimeError):
        op(q, *kv.kv, 2, 0)
    with pytest.raises(RuntimeError):
        op(q[:, :3], *kv.kv, 0, 0)
    with pytest.raises(RuntimeError):
        op(torch.zeros((1, 4, 192, 128), dtype=torch.float16, device="cuda"), *kv.kv, 1, 0)
    with pytest.raises(RuntimeError):
        op(q[..., :64], *kv.kv, 0, 0)
    with pytest.raises((RuntimeError, NotImplementedError)):
        op(q.cpu(), *(t.cpu() for t in kv.kv), 0, 0)
