"""CPU tests of the launch plans of libqattn.so (csrc/plan.hip: host code only, no device).

A plan -- keys per split, key/value heads per workspace chunk, records or recomputation -- never
changes a result bit, so the parity tests cannot see a wrong one.  These tests hold the library's
functions to the rules restated here and to pinned values, and the Python wrappers to the library.
"""
import ctypes
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "quantizedattention_amd" / "libqattn.so"
pytestmark = pytest.mark.skipif(not LIB.exists(),
                                reason="libqattn.so not built (run __graft_entry__.build())")

ENV = ("QATTN_BWD_WS_CHUNK", "QATTN_BWD_WS_MAX", "QATTN_BF16_BWD_WS")


@pytest.fixture
def lib(monkeypatch):
    from quantizedattention_amd import _lib
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    return _lib.load()


def int8_plan(lib, bkv, group, sq, sk, causal, req, cap=-1):
    chunk = ctypes.c_long(-7)
    nbytes = lib.qattn_int8_bwd_plan(bkv, group, sq, sk, causal, req, cap, ctypes.byref(chunk))
    return nbytes, chunk.value


# ------------------------------------------------------------------------------------ key splits
def split_rule(bhv, rows, sk, tile):
    """kv_cache._split_plan / kv_cache_mxfp4._split_plan_fp4 before the library held the rule."""
    wgs = bhv * -(-rows // 128)
    nsplit = max(1, min(sk // 1024, -(-512 // wgs)))
    return -(-(sk // tile) // nsplit) * tile


@pytest.mark.parametrize("tile", [32, 64])
def test_split_keys_is_the_rule(lib, tile):
    for bhv in (1, 2, 8, 64, 256):
        for rows in (1, 32, 128, 129, 2048):
            for n in (1, 2, 15, 16, 17, 64, 128, 512, 1024):
                sk = tile * n
                assert lib.qattn_split_keys(bhv, rows, sk, tile) == split_rule(bhv, rows, sk, tile), \
                    (bhv, rows, sk, tile)


def test_split_keys_pinned(lib):
    assert lib.qattn_split_keys(64, 128, 8192, 32) == 1024
    assert lib.qattn_split_keys(64, 128, 8192, 64) == 1024
    assert lib.qattn_split_keys(2, 128, 4096, 32) == 1024
    assert lib.qattn_split_keys(8, 128, 32768, 64) == 1024
    assert lib.qattn_split_keys(0, 32, 4096, 64) == 4096       # an empty batch: no division by zero
    assert lib.qattn_split_keys(8, 0, 4096, 32) == 4096
    assert lib.qattn_split_keys(64, 128, 8192, 48) == -1       # not a tile of either kernel
    assert lib.qattn_split_keys(64, 128, 8192 + 32, 64) == -1  # sk not a multiple of the tile
    assert lib.qattn_split_keys(64, 128, 100, 32) == -1


def test_split_wrappers_return_the_library_plan(lib):
    from quantizedattention_amd.kv_cache import _split_plan
    from quantizedattention_amd.kv_cache_mxfp4 import _split_plan_fp4
    for bhv, rows, sk in ((64, 128, 8192), (2, 128, 4096), (256, 2048, 4096), (8, 1, 32768), (0, 32, 4096)):
        assert _split_plan(bhv, rows, sk) == lib.qattn_split_keys(bhv, rows, sk, 32)
        assert _split_plan_fp4(bhv, rows, sk) == lib.qattn_split_keys(bhv, rows, sk, 64)


# ---------------------------------------------------------------------------- int8 record backward
REC = 1024 + 4   # bytes per 32x32 tile: the dS_i8 record and its fp32 scale


def test_int8_plan_pinned(lib):
    assert int8_plan(lib, 128, 1, 4096, 4096, 0, -1) == (538968064, 32)      # config 3: 4 chunks
    assert int8_plan(lib, 128, 1, 4096, 4096, 1, -1) == (2155872256, 128)    # causal: one pass
    assert int8_plan(lib, 4, 1, 256, 256, 0, -1) == (263168, 4)
    assert int8_plan(lib, 8, 2, 512, 512, 0, 3) == (1579008, 3)
    assert int8_plan(lib, 8, 2, 512, 512, 0, 0) == (8 * 2 * 16 * 16 * REC, 8)
    assert int8_plan(lib, 8, 2, 512, 512, 0, 1000) == (8 * 2 * 16 * 16 * REC, 8)
    assert int8_plan(lib, 64, 4, 8192, 8192, 0, -1) == (16 * 4 * 256 * 256 * REC, 16)


def test_int8_plan_cap(lib):
    nbytes = 3 * 2 * 16 * 16 * REC
    assert int8_plan(lib, 8, 2, 512, 512, 0, 3, nbytes) == (nbytes, 3)
    assert int8_plan(lib, 8, 2, 512, 512, 0, 3, nbytes - 1) == (0, 3)
    assert int8_plan(lib, 8, 2, 512, 512, 0, 3, 0) == (0, 3)
    assert int8_plan(lib, 8, 2, 512, 512, 0, 3, 2 ** 63 - 1) == (nbytes, 3)


@pytest.mark.parametrize("causal", [0, 1])
def test_int8_plan_region_and_shapes(lib, causal):
    """One key/value head's records are addressed with 32-bit offsets: group * (S/32)^2 KiB < 2 GiB."""
    big = 2 ** 62
    assert int8_plan(lib, 1, 8, 32768, 32768, causal, -1, big)[0] == 0       # an 8 GiB region
    assert int8_plan(lib, 1, 1, 46336, 46336, causal, -1)[0] == 2155411712   # 1448^2 KiB < 2 GiB
    assert int8_plan(lib, 1, 1, 65536, 65536, causal, -1, big)[0] == 0       # 4 GiB
    assert int8_plan(lib, 4, 1, 100, 256, causal, -1)[0] == -1
    assert int8_plan(lib, 4, 1, 256, 100, causal, -1)[0] == -1
    assert int8_plan(lib, 4, 0, 256, 256, causal, -1)[0] == -1


@pytest.mark.parametrize("causal", [0, 1])
def test_int8_plan_lds_tables(lib, causal):
    """The record kernels keep per-tile tables in LDS (dK+dV: 36 B per streamed query tile of the
    key/value head, dQ: 32 B per key tile), so past QATTN_WS_MAX_QUERY_TILES = 1790 tiles of G * Sq / 32
    or QATTN_WS_MAX_KEY_TILES = 2800 of Sk / 32 the plan recomputes (the launch would be refused: G = 8
    query heads of 8160 rows are 2040 tiles); tests/test_gpu_edge.py::test_record_limits_status holds
    the record entries, which return 1 for the same shapes, on buffers of the operands' size."""
    big = 2 ** 62
    assert int8_plan(lib, 260, 8, 8160, 128, causal, 0, big)[0] == 0            # 2040 query tiles
    assert int8_plan(lib, 520, 4, 8160, 128, causal, 0, big)[0] == 520 * 4 * 255 * 4 * REC
    assert int8_plan(lib, 2, 1, 1790 * 32, 128, causal, 0, big)[0] == 2 * 1790 * 4 * REC
    assert int8_plan(lib, 2, 2, 1790 * 16 + 32, 128, causal, 0, big)[0] == 0    # 1792 with the group
    assert int8_plan(lib, 2, 1, 32, 2800 * 32, causal, 0, big)[0] == 2 * 2800 * REC
    assert int8_plan(lib, 2, 1, 32, 2801 * 32, causal, 0, big)[0] == 0


def test_int8_plan_environment(lib, monkeypatch):
    monkeypatch.setenv("QATTN_BWD_WS_CHUNK", "3")
    assert int8_plan(lib, 8, 2, 512, 512, 0, -1) == (1579008, 3)
    assert int8_plan(lib, 8, 2, 512, 512, 0, 5) == (5 * 2 * 16 * 16 * REC, 5)   # the argument wins
    monkeypatch.setenv("QATTN_BWD_WS_CHUNK", "-1")                               # negative: auto
    assert int8_plan(lib, 128, 1, 4096, 4096, 0, -1) == (538968064, 32)
    assert int8_plan(lib, 128, 1, 4096, 4096, 1, -1) == (2155872256, 128)
    monkeypatch.setenv("QATTN_BWD_WS_CHUNK", "0")                                # all heads
    assert int8_plan(lib, 128, 1, 4096, 4096, 0, -1) == (2155872256, 128)
    monkeypatch.delenv("QATTN_BWD_WS_CHUNK")
    monkeypatch.setenv("QATTN_BWD_WS_MAX", "0")
    assert int8_plan(lib, 128, 1, 4096, 4096, 0, -1) == (0, 32)
    assert int8_plan(lib, 128, 1, 4096, 4096, 0, -1, 2 ** 40) == (538968064, 32)   # the argument wins


def test_ws_chunk_returns_the_library_plan(lib, monkeypatch):
    from quantizedattention_amd.attention_int8 import _ws_chunk
    for chunk, req in ((None, -1), (0, 0), (3, 3), (1000, 1000)):
        for causal in (False, True):
            for bkv, sk in ((128, 4096), (4, 256), (8, 512), (64, 8192)):
                assert _ws_chunk(chunk, causal, bkv, sk) == int8_plan(lib, bkv, 1, 32, sk, int(causal), req)[1]
    assert _ws_chunk(None, False, 128, 4096) == 32 and _ws_chunk(None, True, 128, 4096) == 128
    monkeypatch.setenv("QATTN_BWD_WS_CHUNK", "3")      # read at the call, not at import
    assert _ws_chunk(None, False, 128, 4096) == 3 and _ws_chunk(7, False, 128, 4096) == 7


# ------------------------------------------------------------------------------------ bf16 backward
def test_bf16_plan(lib, monkeypatch):
    bh, sq, sk = 6, 96, 160
    nbytes = bh * (sq // 32) * (sk // 32) * 2048
    assert lib.qattn_bf16_bwd_plan(bh, sq, sk, 1, -1, -1) == nbytes      # causal: records
    assert lib.qattn_bf16_bwd_plan(bh, sq, sk, 0, -1, -1) == 0           # else recompute
    assert lib.qattn_bf16_bwd_plan(bh, sq, sk, 0, 1, -1) == nbytes       # forced on / off
    assert lib.qattn_bf16_bwd_plan(bh, sq, sk, 1, 0, -1) == 0
    assert lib.qattn_bf16_bwd_plan(bh, sq, sk, 1, -1, 0) == 0            # the cap
    assert lib.qattn_bf16_bwd_plan(bh, sq, sk, 1, -1, nbytes) == nbytes
    assert lib.qattn_bf16_bwd_plan(bh, sq, sk, 1, -1, nbytes - 1) == 0
    assert lib.qattn_bf16_bwd_plan(bh, 100, sk, 1, -1, -1) == -1
    monkeypatch.setenv("QATTN_BF16_BWD_WS", "0")
    assert lib.qattn_bf16_bwd_plan(bh, sq, sk, 1, -1, -1) == 0
    assert lib.qattn_bf16_bwd_plan(bh, sq, sk, 1, 1, -1) == nbytes       # the argument wins
    monkeypatch.setenv("QATTN_BF16_BWD_WS", "1")
    assert lib.qattn_bf16_bwd_plan(bh, sq, sk, 0, -1, -1) == nbytes
    monkeypatch.setenv("QATTN_BWD_WS_MAX", "0")
    assert lib.qattn_bf16_bwd_plan(bh, sq, sk, 0, -1, -1) == 0


# ------------------------------------------------------------------------------------------- scales
@pytest.mark.parametrize("D", [64, 128])
def test_scales(D):
    import math

    from quantizedattention_amd import _lib, attention_int8, attention_mxfp4
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))  # noqa: E731
    assert _lib.qk_scale(D) == f32(1.0 / math.sqrt(D) * 1.44269504)
    assert _lib.sm_scale(D) == f32(1.0 / math.sqrt(D))
    assert attention_int8._qk_scale(D) == 1.0 / math.sqrt(D) * 1.44269504      # the double
    assert attention_mxfp4._qk_scale(D) == _lib.qk_scale(D)
