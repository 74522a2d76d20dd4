"""CPU tests of the MX-FP4 key/value cache: the split definition restated (tests/mxfp4_split_ref.py)
equals the one-pass restatement, the wire format round-trips and the two cache classes refuse each
other's buffers, and the split plan keeps its stated rules.  No kernel runs here.
"""
import pytest
import torch

import mxfp4_masked_ref as MR
import mxfp4_split_ref as SR
from quantizedattention_amd import _lib
from quantizedattention_amd.kv_cache import MAGIC as MAGIC_INT8
from quantizedattention_amd.kv_cache import QuantizedKV
from quantizedattention_amd.kv_cache_mxfp4 import (MAGIC, MIN_SPLIT_KEYS, QuantizedKVFP4,
                                                   _split_plan_fp4)


@pytest.mark.parametrize("qmul", [1, 3])
@pytest.mark.parametrize("case", SR.CASES)
def test_split_restatement_is_the_one_pass_restatement(case, qmul):
    """Splitting over the keys and merging changes nothing: every m_s is an integer, so the merge's
    weights are exact powers of two.  q x 3 raises m mid-stream."""
    B, H, Hkv, Sq, Sk, causal, kps = case
    q, k, v = SR.inputs(case, qmul)
    O1, l1, ops1 = MR.mxfp4_fwd_masked(q, k, v, causal)
    O2, l2, ops2, (m, l) = SR.mxfp4_fwd_split(q, k, v, causal, kps)
    for a, b in zip(ops1, ops2):
        assert torch.equal(a, b)
    assert m.shape == (-(-Sk // kps), B * H, Sq)
    fin = m[~torch.isinf(m)]
    assert torch.equal(fin, fin.round())                   # integer running maxima
    assert torch.isfinite(O2.float()).all() and torch.isfinite(l2).all()
    assert torch.equal(O2, O1)
    assert (l2 - l1).abs().max().item() <= 1e-6
    empty = torch.isinf(m) & (m < 0)
    assert torch.equal(empty, l == 0)
    if case == (1, 2, 1, 96, 256, 2, 64):
        # rows 0..31 of both heads see keys <= 160 + 31: nothing of split 3 (keys 192..255)
        assert int(empty.sum()) == 64 and bool(empty[3, :, :32].all())
    elif not causal:
        assert not empty.any()


def test_merge_case_tells_the_two_roundings_apart():
    """The partials tests/test_gpu_mxfp4_cache.py merges on the GPU discriminate: the product rounded to
    fp16 once and the one rounded twice differ in at least 4 elements of the columns that take the first
    form (c % 8 in (0, 7)) and in at least 4 of the others, so a kernel that used one form everywhere, or
    swapped them, would not reproduce ``merge_bits``."""
    opart, ml, O, differs, lse = SR.merge_case()
    assert opart.shape == (3, 2048, 128) and ml.shape == (3, 2048, 2)
    m = ml[..., 0]
    assert bool(torch.isinf(m[0, ::7]).all()) and bool(torch.isfinite(m).any(0).all())
    assert torch.equal(m[torch.isfinite(m)], m[torch.isfinite(m)].round())
    assert bool(torch.isfinite(O.float()).all()) and bool(torch.isfinite(lse).all())
    col = torch.arange(128) % 8
    edge = (col == 0) | (col == 7)
    print(f"differing elements: {int(differs[:, edge].sum())} in columns 0/7, {int(differs[:, ~edge].sum())} "
          f"in the others, of {differs.numel()}")
    assert int(differs[:, edge].sum()) >= 4 and int(differs[:, ~edge].sum()) >= 4
    # a second evaluation gives the same bits
    assert torch.equal(SR.merge_bits(opart, ml)[0], O)


# ------------------------------------------------------------------------------ wire format
def _random_cache(B=2, H=3, S=128, D=128, smoothed=True, seed=0):
    g = torch.Generator().manual_seed(seed)
    u8 = lambda *s: torch.randint(0, 256, s, generator=g, dtype=torch.uint8)  # noqa: E731
    km = torch.randn(B, H, 1, D, generator=g).half() if smoothed else None
    return QuantizedKVFP4(u8(B, H, S, D // 2), u8(B, H, S, D // 32), u8(B * H, S // 64, D, 32),
                          u8(B * H, S // 64, D, 2), km)


@pytest.mark.parametrize("smoothed", [False, True])
def test_wire_format_round_trip(smoothed):
    kv = _random_cache(smoothed=smoothed)
    assert kv.shape == (2, 3, 128, 128) and len(kv.kv) == 4 and kv.kv[2] is kv.vt
    buf = kv.to_bytes()
    assert buf.dtype == torch.uint8 and bytes(buf[:8].tolist()) == MAGIC and MAGIC != MAGIC_INT8
    back = QuantizedKVFP4.from_bytes(buf)
    for name in ("k4", "ks", "vt", "vs"):
        a, b = getattr(back, name), getattr(kv, name)
        assert a.dtype == torch.uint8 and a.shape == b.shape and torch.equal(a, b), name
    assert (back.k_mean is None) == (not smoothed)
    if smoothed:
        assert torch.equal(back.k_mean, kv.k_mean)
    import json
    hlen = int.from_bytes(bytes(buf[8:12].tolist()), "little")
    header = json.loads(bytes(buf[12:12 + hlen].tolist()).decode())
    assert header["format"] == "mxfp4" and header["block"] == 64 and header["tokens"] == 128
    assert all(o % 256 == 0 for o, *_ in header["sections"].values())


def test_wire_format_rejects_garbage_and_the_other_cache():
    with pytest.raises(_lib.QAttnError, match="magic"):
        QuantizedKVFP4.from_bytes(torch.zeros(64, dtype=torch.uint8))
    g = torch.Generator().manual_seed(1)
    i8 = lambda *s: torch.randint(-127, 128, s, generator=g, dtype=torch.int8)  # noqa: E731
    int8_kv = QuantizedKV(i8(1, 2, 64, 64), i8(1, 2, 64, 64), torch.rand(4, generator=g).half(),
                          torch.rand(4, generator=g).half())
    with pytest.raises(_lib.QAttnError):
        QuantizedKVFP4.from_bytes(int8_kv.to_bytes())          # a QATTNKV1 buffer
    with pytest.raises(_lib.QAttnError):
        QuantizedKV.from_bytes(_random_cache().to_bytes())     # the MX-FP4 magic


# ------------------------------------------------------------------------------ split plan
def test_split_plan():
    assert MIN_SPLIT_KEYS % 64 == 0
    for bhv in (1, 2, 8, 32, 64, 128, 256, 512):
        for rows in (1, 4, 5, 32, 33, 128, 130, 512, 4096):
            for sk in (64, 192, 1024, 1088, 8192, 32768, 131072 + 64):
                kps = _split_plan_fp4(bhv, rows, sk)
                assert kps % 64 == 0 and 64 <= kps <= sk, (bhv, rows, sk, kps)
                nsplit = -(-sk // kps)
                if bhv * -(-rows // 128) >= 512:        # the row blocks alone fill the chip
                    assert kps == sk
                if nsplit > 1:                          # never a split shorter than the minimum
                    assert kps >= MIN_SPLIT_KEYS and sk - (nsplit - 1) * kps >= 64
    assert _split_plan_fp4(64, 128, 8192) == 1024            # 64 workgroups x 8 splits = 512
    assert _split_plan_fp4(256, 2048, 4096) == 4096


def test_host_side_refusals():
    """Argument checks that answer before any GPU is touched."""
    from quantizedattention_amd.kv_cache_mxfp4 import attention_mxfp4_cached, quantize_kv_fp4
    kv = _random_cache(B=1, H=2, S=128, smoothed=False)
    q = torch.zeros((1, 4, 1, 128), dtype=torch.float16)
    with pytest.raises(_lib.QAttnError, match="no CPU fallback"):
        attention_mxfp4_cached(q, kv)
    with pytest.raises(_lib.QAttnError, match="no CPU fallback"):
        quantize_kv_fp4(torch.zeros((1, 2, 64, 128), dtype=torch.float16),
                        torch.zeros((1, 2, 64, 128), dtype=torch.float16))
    with pytest.raises(_lib.QAttnError):
        quantize_kv_fp4(torch.zeros((1, 2, 64, 64), dtype=torch.float16),
                        torch.zeros((1, 2, 64, 64), dtype=torch.float16))      # head_dim 64
    with pytest.raises(_lib.QAttnError):
        kv.append(torch.zeros((1, 2, 32, 128), dtype=torch.float16),
                  torch.zeros((1, 2, 32, 128), dtype=torch.float16))          # 32 tokens
