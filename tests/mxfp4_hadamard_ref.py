"""The Hadamard-rotated quantisers of the paged MX-FP4 cache (PagedKVFP4.allocate(hadamard=True)) restated in torch
on the CPU, after include/qattn.h "Hadamard-rotated pools": the f16 row (after rope and f16(x - k_mean)) converted
exactly to fp32, log2(D) stages of (a + b, a - b) butterflies, one rounded fp32 operation each, then
oracle/mxfp4.py's block quantiser on the fp32 values.  TEST INFRASTRUCTURE ONLY.
"""
import torch

from oracle import mxfp4 as M


def hadamard(x: torch.Tensor) -> torch.Tensor:
    """x fp32 [..., D], D a power of two -> H x, the staged transform."""
    assert x.dtype == torch.float32
    D, s = x.shape[-1], 1
    while s < D:
        y = x.reshape(*x.shape[:-1], D // (2 * s), 2, s)      # [.., pair group, a | b, s]: b is a's i + 2^stage
        a, b = y[..., 0, :], y[..., 1, :]
        x = torch.stack([a + b, a - b], -2).reshape(x.shape)
        s *= 2
    return x


def rope(x: torch.Tensor, tab: torch.Tensor, pos, interleaved: bool) -> torch.Tensor:
    """The rotary contract at any width: x f16 [T, H, D], tab f32 [max_pos, D] -> f16 [T, H, D]."""
    h = x.shape[-1] // 2
    rows = tab[torch.as_tensor(pos, dtype=torch.long)]
    c, s = rows[:, None, :h], rows[:, None, h:]
    a, b = (x[..., 0::2], x[..., 1::2]) if interleaved else (x[..., :h], x[..., h:])
    a, b = a.float(), b.float()
    first, second = (a * c - b * s).half(), (b * c + a * s).half()
    return torch.stack([first, second], -1).flatten(-2) if interleaved else torch.cat([first, second], -1)


def rotated(x: torch.Tensor, mean=None) -> torch.Tensor:
    """x f16 [..., D] (after rope) -> fp32 H f16(x - mean): what the rotated quantiser scales and packs."""
    assert x.dtype == torch.float16
    if mean is not None:
        x = (x.float() - mean.float()).half()
    return hadamard(x.float())


quant_rows_had = lambda x, mean=None: M.quant_rows(rotated(x, mean))   # noqa: E731  f16 [rows, D] -> (codes, scales)


def outlier_inputs(D: int, L: int = 449, Hq: int = 8, channels: int = 4, gain: float = 32.0, seed: int = 17):
    """q f16 [1, Hq, D], k, v f16 [L, 1, D] with ``channels`` of the D channels of q and k scaled by ``gain``, the
    whole scaled so that the logits keep unit variance."""
    g = torch.Generator().manual_seed(seed)
    amp = torch.full((D,), 1.0)
    amp[torch.randperm(D, generator=g)[:channels]] = gain
    sd = (D / (D - channels + channels * gain ** 2)) ** 0.25    # q . k / sqrt(D) of unit variance
    q = (torch.randn((1, Hq, D), generator=g) * amp * sd).half()
    k = (torch.randn((L, 1, D), generator=g) * amp * sd).half()
    v = torch.randn((L, 1, D), generator=g).half()
    return q, k, v


def exact_attention(q, k, v):
    """float64 softmax(q k^T / sqrt(D)) v on the fp16 inputs: q [n, Hq, D], k, v [L, 1, D] -> [n, Hq, D]."""
    q, k, v = q.double(), k[:, 0].double(), v[:, 0].double()
    return torch.softmax(q @ k.T / q.shape[-1] ** 0.5, -1) @ v
