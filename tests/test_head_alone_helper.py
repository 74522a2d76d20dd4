"""The head-alone instrument can fail: on the CPU, with the stand-in "kernel" of tests/head_alone.py in
place of a HIP kernel, a row offset truncated to fewer bits than the tensor needs is named by ``_Diff``
for exactly the heads a big-index test (tests/test_gpu_big_index.py) runs alone past the threshold.
No kernel runs and nothing is planted in the library: the threshold is 2^15 elements here instead of
2^31, the comparison logic is the same."""
import pytest
import torch

from head_alone import _Diff, _gen, _randn, boundary_heads, standin_head_scale

# 23 heads x 24 rows x 64: 35328 elements > 2^15; row 512 = 2^15 / 64 lies inside head 21 (rows 504 ..
# 527), so head 21 straddles the threshold and head 22 lies wholly past it
H, R, D, BITS = 23, 24, 64, 15


def _compare(offset_bits):
    x = _randn((H, R, D), _gen("standin", device="cpu"), torch.float16)
    full = standin_head_scale(x, offset_bits)
    heads = boundary_heads(H, R * D, 1 << BITS)
    diff = _Diff()
    for h in heads:
        alone = standin_head_scale(x[h:h + 1].clone())   # a head alone starts at offset 0
        diff.eq("out", (0, h), alone, full[h])
    return heads, diff


def test_boundary_heads_come_from_the_shape():
    assert boundary_heads(H, R * D, 1 << BITS) == (0, 21, 22)
    # a head that starts exactly at the threshold: the boundary head is the one that ends there
    assert boundary_heads(40, 1 << 10, 1 << 15) == (0, 31, 39)
    # the shapes of tests/test_gpu_big_index.py, in rows of 128 elements
    assert boundary_heads(17500, 2 * 480 * 128) == (0, 17476, 17499)
    assert boundary_heads(4104, 4096 * 128) == (0, 4095, 4103)
    with pytest.raises(AssertionError):
        boundary_heads(22, R * D, 1 << BITS)       # nothing wholly past the threshold
    with pytest.raises(AssertionError):
        boundary_heads(8, R * D, 1 << BITS)        # the tensor does not reach it


def test_full_width_offsets_pass():
    heads, diff = _compare(64)
    assert diff.n == len(heads) == 3
    diff.done()


def test_truncated_offset_is_named():
    """Offsets kept in 15 bits: head 0 is intact, the straddling head differs in the rows past the
    threshold, the last head in all of them, and ``done`` raises naming both."""
    heads, diff = _compare(BITS)
    assert heads == (0, 21, 22)
    named = {(name, h): n for name, _b, h, n in diff.bad}
    assert set(named) == {("out", 21), ("out", 22)}
    assert 0 < named[("out", 21)] <= (R - (512 - 21 * R)) * D and named[("out", 22)] > R * D // 2
    with pytest.raises(AssertionError, match="22"):
        diff.done()
