"""CPU tests of the preallocated MX-FP4 cache's host side and of its restatement
(tests/mxfp4_ragged_ref.py): the ragged definition reduces to the existing ones, the identity the GPU
test relies on holds in it bit for bit, the new C entries and the Python layer refuse bad arguments
before any launch, and the operator's fake kernel gives the right shapes.
"""
import ctypes

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import mxfp4_masked_ref as MR
import mxfp4_ragged_ref as RR
import mxfp4_split_ref as SR


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("causal", [0, 2])
def test_equal_full_lengths_are_the_masked_forward(causal):
    """Every length the same multiple of 64, one split: mxfp4_fwd_masked bit for bit."""
    q, k, v = MR.randn_qkv((2, 4, 2, 5, 128))
    O, lse, _ = RR.mxfp4_fwd_ragged(q, [k[b:b + 1] for b in range(2)], [v[b:b + 1] for b in range(2)],
                                    bool(causal))
    RO, Rl, _ = MR.mxfp4_fwd_masked(q, k, v, causal)
    assert torch.equal(O, RO) and torch.equal(lse, Rl)


@pytest.mark.parametrize("Sq,lens,causal", [(1, (100, 64, 1, 191), False), (5, (100, 64, 5, 191), True)])
def test_ragged_is_the_first_rows_of_the_bottom_right_problem(Sq, lens, causal):
    q, ks, vs = RR.inputs(4, 4, 1, Sq, lens)
    O, lse, _ = RR.mxfp4_fwd_ragged(q, ks, vs, causal, 64)
    for b in range(4):
        q2, kp, vp = RR.identity_problem(q[b:b + 1], ks[b], vs[b], causal)
        O2, l2, _, _ = SR.mxfp4_fwd_split(q2, kp, vp, 2, 64)
        assert torch.equal(O[b], O2[0, :, :Sq]), b
        assert torch.equal(lse.view(4, 4, Sq)[b], l2.view(4, -1)[:, :Sq]), b


def test_empty_splits_in_the_restatement():
    q, ks, vs = RR.inputs(2, 2, 1, 1, (64, 256))
    _, _, (m, l) = RR.mxfp4_fwd_ragged(q, ks, vs, False, 64)
    assert m.shape == (4, 4, 1)
    assert torch.isinf(m[1:, :2]).all() and (l[1:, :2] == 0).all()
    assert torch.isfinite(m[:, 2:]).all() and torch.isfinite(m[0]).all()


# ------------------------------------------------------------------ the C entries refuse bad arguments
X = ctypes.c_void_p(256)   # a non-null pointer nothing dereferences: every case returns before a launch


def test_fwd_split_len_rejects(lib):
    fn = lib.qattn_mxfp4_attn_fwd_split_len

    def status(lens=X, bhv=4, hps=2, rows=8, sq_head=4, cap=256, sk_max=128, causal=0, kps=64, hd=128):
        return fn(X, X, X, X, X, X, X, X, lens, bhv, hps, rows, sq_head, cap, sk_max, causal, kps, hd,
                  0.1275, None)
    assert status(hd=64) == 1
    assert status(cap=200) == 1 and status(sk_max=100) == 1          # not multiples of 64
    assert status(cap=128, sk_max=192) == 1                          # sk_max > cap
    assert status(sk_max=0) == 1                                     # sk_max < 64
    assert status(cap=(1 << 25) + 64) == 1
    assert status(kps=0) == 1 and status(kps=32) == 1 and status(kps=96) == 1
    assert status(sq_head=0) == 1 and status(rows=8, sq_head=3) == 1
    assert status(hps=0) == 1 and status(bhv=4, hps=3) == 1
    assert status(causal=1) == 1 and status(causal=3) == 1 and status(causal=-1) == 1
    assert status(lens=None) == 1
    assert status(bhv=0) == 0 and status(rows=0) == 0                # nothing to do: no launch


def test_cache_append_rejects(lib):
    fn = lib.qattn_mxfp4_cache_append

    def status(ptrs=(X,) * 10, batch=2, heads=2, n=1, cap=256, hd=128):
        return fn(*ptrs, batch, heads, n, cap, hd, None)
    assert status(hd=64) == 1 and status(n=0) == 1 and status(n=-1) == 1 and status(cap=100) == 1
    for i in (0, 1, 3, 4, 5, 6, 7, 8):   # k, v, k4, kscale, vt, vscale, vtail, lens (k_mean, counts may be null)
        ptrs = [X] * 10
        ptrs[i] = None
        assert status(ptrs=tuple(ptrs)) == 1, i
    assert status(batch=0) == 0                                      # nothing to do: no launch


# ------------------------------------------------------------------ the Python layer
def _host_cache(lengths, cap=128, heads=2):
    """A PreallocatedKVFP4 of CPU tensors: enough for the checks that come before any launch."""
    from quantizedattention_amd.kv_cache_mxfp4 import PreallocatedKVFP4
    B = len(lengths)
    z = lambda *s: torch.zeros(s, dtype=torch.uint8)  # noqa: E731
    return PreallocatedKVFP4(z(B, heads, cap, 64), z(B, heads, cap, 4), z(B * heads, cap // 64, 128, 32),
                             z(B * heads, cap // 64, 128, 2), torch.zeros((B * heads, 64, 128), dtype=torch.float16),
                             torch.tensor(lengths, dtype=torch.int32), lengths)


def test_python_argument_errors(lib):
    from quantizedattention_amd import _lib
    from quantizedattention_amd import kv_cache_mxfp4 as KC
    E = _lib.QAttnError
    assert {"PreallocatedKVFP4", "attention_mxfp4_decode"} <= set(KC.__all__)
    with pytest.raises(E):
        KC.PreallocatedKVFP4.allocate(1, 1, 100, "cuda")               # capacity % 64
    with pytest.raises(E, match="no CPU fallback"):
        KC.PreallocatedKVFP4.allocate(1, 1, 128, "cpu")
    c = _host_cache([100, 64])
    h = lambda *s: torch.zeros(s, dtype=torch.float16)  # noqa: E731
    with pytest.raises(E, match="capacity"):
        c.append(h(2, 2, 29, 128), h(2, 2, 29, 128))                     # 100 + 29 > 128
    with pytest.raises(E, match="capacity"):
        c.append(h(2, 2, 65, 128), h(2, 2, 65, 128), counts=[1, 65])
    with pytest.raises(E, match="counts"):
        c.append(h(2, 2, 4, 128), h(2, 2, 4, 128), counts=[5, 0])
    with pytest.raises(E, match="counts"):
        c.append(h(2, 2, 4, 128), h(2, 2, 4, 128), counts=[-1, 0])
    with pytest.raises(E, match="counts"):
        c.append(h(2, 2, 4, 128), h(2, 2, 4, 128), counts=[1])
    for bad in (h(2, 2, 0, 128), h(2, 1, 4, 128), h(1, 2, 4, 128), h(2, 2, 4, 64), h(2, 4, 128)):
        with pytest.raises(E):
            c.append(bad, bad)
    with pytest.raises(E):
        c.append(h(2, 2, 4, 128), h(2, 2, 5, 128))
    with pytest.raises(E, match="no CPU fallback"):
        c.append(h(2, 2, 4, 128), h(2, 2, 4, 128))                       # valid, but not on the GPU
    assert c.lengths == [100, 64]                                        # no refused call moved a length
    with pytest.raises(E):
        c.snapshot(0)                                                    # 100 is no multiple of 64
    with pytest.raises(E):
        c.snapshot(2)
    with pytest.raises(E):
        c.reset([2])
    # decode
    q = h(2, 4, 1, 128)
    with pytest.raises(E, match="no CPU fallback"):
        KC.attention_mxfp4_decode(q, c)
    with pytest.raises(E, match="at least one"):
        KC.attention_mxfp4_decode(q, _host_cache([0, 64]))
    with pytest.raises(E, match="causal"):
        KC.attention_mxfp4_decode(h(2, 4, 65, 128), c, causal=True)    # Sq > min(lengths)
    with pytest.raises(E):
        KC.attention_mxfp4_decode(q, c, keys_per_split=96)
    with pytest.raises(E):
        KC.attention_mxfp4_decode(h(2, 3, 1, 128), c)                    # Hq % Hkv
    with pytest.raises(E):
        KC.attention_mxfp4_decode(h(1, 4, 1, 128), c)                    # batch
    with pytest.raises(E):
        KC.attention_mxfp4_decode(h(2, 4, 1, 64), c)                     # head_dim
    with pytest.raises(E):
        KC.attention_mxfp4_decode(h(2, 4, 0, 128), c)                    # Sq = 0
    with pytest.raises(E):
        KC.attention_mxfp4_decode(q, KC.QuantizedKVFP4(c.k4, c.ks, c.vt, c.vs))
    c.reset([0])
    assert c.lengths == [0, 64] and c.lens.tolist() == [0, 64]
    bhv, rows, sk_max, kps, ns = KC._decode_plan(h(2, 8, 3, 128), _host_cache([100, 64]), True, None)
    assert (bhv, rows, sk_max, kps, ns) == (4, 12, 128, 128, 1)
    assert KC._decode_plan(q, _host_cache([65, 1], cap=256), False, 64)[2:] == (128, 64, 2)


def test_op_registered_and_fake_shape():
    import quantizedattention_amd.ops as ops
    assert hasattr(torch.ops.qattn, "mxfp4_decode") and "mxfp4_decode" in ops.__all__
    op = torch.ops.qattn.mxfp4_decode.default
    assert torch._C._dispatch_has_kernel_for_dispatch_key(op.name(), "CUDA")
    assert not torch._C._dispatch_has_kernel_for_dispatch_key(op.name(), "CPU")
    with FakeTensorMode():
        e = lambda *s, dt=torch.uint8: torch.empty(s, dtype=dt, device="cuda")  # noqa: E731
        q = e(3, 8, 5, 128, dt=torch.float16)
        for causal in (0, 1):
            O, lse = torch.ops.qattn.mxfp4_decode(q, e(3, 2, 256, 64), e(3, 2, 256, 4), e(6, 4, 128, 32),
                                                  e(6, 4, 128, 2), e(3, dt=torch.int32), 192, causal, 0)
            assert O.shape == (3, 8, 5, 128) and O.dtype == torch.float16
            assert lse.shape == (24, 5) and lse.dtype == torch.float32
