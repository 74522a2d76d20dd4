"""The head-alone instrument, shared by tests/test_gpu_head_alone.py (every head of a full grid),
tests/test_gpu_big_index.py (the heads around element 2^31) and tests/test_gpu_views.py: inputs drawn
on the GPU from a generator seeded by the test's own parameters, bit patterns compared with
``torch.equal``, and a collector that names every (output, batch entry, key/value head) that differs.

``boundary_heads`` picks the heads a big-index test runs alone, and ``standin_head_scale`` is a tiny
stand-in "kernel" whose row offsets can be truncated to a given width: tests/test_head_alone_helper.py
holds the instrument to it on the CPU (a truncated offset must be named, head by head).  Nothing here
needs a GPU at import.
"""
import zlib

import torch


def _gen(*key, device="cuda"):
    """A generator seeded from the test's own parameters: no two tests draw the same inputs."""
    return torch.Generator(device=device).manual_seed(zlib.crc32(repr(key).encode()))


def _randn(shape, g, dtype, scale=1.0):
    return (torch.randn(shape, device=g.device, generator=g) * scale).to(dtype)


def _bits(t):
    t = t.contiguous()
    if t.dtype in (torch.float16, torch.bfloat16):
        return t.view(torch.int16)
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _groups(B, Hq, Hkv):
    """(batch entry, key/value head, slice of its query heads)."""
    G = Hq // Hkv
    return [(b, kh, slice(kh * G, kh * G + G)) for b in range(B) for kh in range(Hkv)]


def _heads(x, B, H):
    """[B, H, the rest flattened]: a view of a contiguous head-major tensor of any rank."""
    return x.reshape(B, H, -1)


def _cut(x, B, H, b, hs):
    """A copy of the heads ``hs`` of batch entry ``b`` of a head-major tensor, flattened per head."""
    return _heads(x, B, H)[b:b + 1, hs].clone()


class _Diff:
    """Collects the outputs that differ, to name every (output, batch entry, key/value head)."""

    def __init__(self):
        self.bad, self.n = [], 0

    def eq(self, name, where, alone, full_part):
        self.n += 1
        a, f = _bits(alone).reshape(-1), _bits(full_part).reshape(-1)
        if a.shape != f.shape or not torch.equal(a, f):
            self.bad.append((name,) + tuple(where) + (int((a != f).sum()) if a.shape == f.shape else "shape",))

    def done(self):
        assert self.n > 0
        assert not self.bad, (len(self.bad), "of", self.n, "differ; first:", self.bad[:8])


def boundary_heads(heads, head_elems, threshold=2 ** 31):
    """The heads of a head-major tensor of ``heads`` x ``head_elems`` elements that a big-index test
    runs alone: head 0, the boundary head (the one that holds element ``threshold - 1``: it straddles
    ``threshold``, or ends exactly there when a head starts at it) and the last head, which must lie
    wholly past ``threshold``."""
    assert heads * head_elems > threshold, "the tensor does not pass the threshold"
    boundary, last = (threshold - 1) // head_elems, heads - 1
    assert 0 < boundary < last
    assert boundary * head_elems < threshold <= (boundary + 1) * head_elems
    assert last * head_elems >= threshold, "the last head must lie wholly past the threshold"
    return 0, boundary, last


def standin_head_scale(x, offset_bits=64):
    """A stand-in "kernel" on a head-major [H, R, D] tensor: out[h, r] = 2 * x at row offset
    (h * R + r) * D, the offset kept in ``offset_bits`` bits as an unsigned index would be.  With 64
    bits it is 2 * x; with fewer, the rows past element 2^offset_bits read another head's rows."""
    H, R, D = x.shape
    flat = x.reshape(-1)
    off = torch.arange(H * R, dtype=torch.int64) * D
    if offset_bits < 63:
        off = off % (1 << offset_bits)
    idx = off[:, None] + torch.arange(D, dtype=torch.int64)[None, :]
    return (2 * flat[idx]).reshape(H, R, D)
