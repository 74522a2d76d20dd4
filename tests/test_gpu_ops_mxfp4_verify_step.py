"""qattn::mxfp4_verify_step_plan and qattn::mxfp4_verify_step (csrc/torch/qattn_ops.cpp): the operators equal
kv_cache_mxfp4.VerifyStep's own launches bit for bit (GPU), and their fake kernels give the right shapes and
dtypes (no GPU needed)."""
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import mxfp4_varlen_helpers as H

N = H.MAX_SEQS


def heap(n):
    return [-1] + [(t - 1) // 2 for t in range(1, n)]


@pytest.mark.gpu
@pytest.mark.parametrize("Hq,Hkv,K", ((4, 2, 5), (8, 2, 40)))
def test_operators_equal_the_python_entries(Hq, Hkv, K):
    from quantizedattention_amd import kv_cache_mxfp4 as Km, ops
    cache = H.fill_pool(Hkv, (127, 130, 255, 70), 64, 32)
    step = Km.VerifyStep(N, 320, Hq, Hkv, "cuda", K, parents=heap(K), keys_per_split=64)
    g = torch.Generator().manual_seed(9)
    k, v, q = (torch.randn((N * K, h, H.D), generator=g).half().cuda() for h in (Hkv, Hkv, Hq))
    step.prepare(cache, [0, 5, 2, 4], trees=[None, list(range(-1, K - 1)), None, [-1] + [0] * (K - 1)])
    tabs = ops.mxfp4_verify_step_plan(step, cache)            # before the append: the lengths it reads
    step.append(cache, k, v)
    for mine, op in zip((step.seq_tab, step.tiles, step.pos, step.seq_rec), tabs):
        assert mine.dtype == op.dtype and mine.shape == op.shape and torch.equal(mine, op)
    O2, lse2 = ops.mxfp4_verify_step(q, step, cache, seq_rec=tabs[3])
    O, lse = step.attend(cache, q)
    assert O2.data_ptr() != O.data_ptr() and torch.equal(O, O2) and torch.equal(lse, lse2)
    assert bool((lse[4 * K:] == float("-inf")).all()) and bool(torch.isfinite(lse[:4 * K]).all())
    with pytest.raises(RuntimeError, match="tree must be"):
        torch.ops.qattn.mxfp4_verify_step_plan(step.slots, cache.lens, step.tree[:-1], K, 320, Hkv, Hq // Hkv, 64,
                                               step.splits)
    with pytest.raises(RuntimeError, match="work must be"):
        torch.ops.qattn.mxfp4_verify_step(q, cache.k4, cache.ks, cache.vt, cache.vs, cache.lens, cache.block_table,
                                          step.seq_rec, step.work[:-1], step.tree, K, step.splits, 64)


def test_exports_and_fake_kernels():
    from quantizedattention_amd import _lib, kv_cache_mxfp4 as Km, ops
    assert {"VerifyStep", "verify_step_splits", "plan_verify_step"} <= set(Km.__all__)
    assert {"mxfp4_verify_step_plan", "mxfp4_verify_step"} <= set(ops.__all__)
    assert {"qattn_mxfp4_verify_step_plan", "qattn_mxfp4_attn_fwd_verify_step",
            "qattn_mxfp4_verify_step_combine"} <= set(_lib.SIGNATURES)
    with pytest.raises(_lib.QAttnError, match="no CPU fallback"):
        Km.VerifyStep(4, 512, 4, 2, "cpu", 5)
    with FakeTensorMode():
        i32 = lambda *s: torch.empty(s, dtype=torch.int32, device="cuda")  # noqa: E731
        u8 = lambda *s: torch.empty(s, dtype=torch.uint8, device="cuda")  # noqa: E731
        tree = torch.empty((6 * 40,), dtype=torch.int64, device="cuda")
        tab, tiles, pos, rec = torch.ops.qattn.mxfp4_verify_step_plan(i32(6), i32(6), tree, 40, 320, 2, 4, 64, 5)
        assert (tab.shape, tiles.shape, pos.shape, rec.shape) == ((6, 4), (12, 2), (240,), (6, 8))
        assert all(t.dtype == torch.int32 and t.device.type == "cuda" for t in (tab, tiles, pos, rec))
        q = torch.empty((240, 8, 128), dtype=torch.float16, device="cuda")
        O, lse = torch.ops.qattn.mxfp4_verify_step(q, u8(8, 2, 64, 64), u8(8, 2, 64, 4), u8(8, 2, 1, 128, 32),
                                                   u8(8, 2, 1, 128, 2), i32(6), i32(6, 5), rec, i32(60, 4), tree,
                                                   40, 5, 64)
        assert O.shape == (240, 8, 128) and O.dtype == torch.float16 and lse.shape == (240, 8)
        assert lse.dtype == torch.float32
