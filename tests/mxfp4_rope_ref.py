"""The rotary contract of the packed MX-FP4 cache path, restated in torch on the CPU, and the inputs the
CPU and GPU rope tests share.

Contract (include/qattn.h): a table fp32 [max_pos, 128] holds cos theta(p, i) in column i and sin theta(p, i)
in column 64 + i; NeoX pairs elements (i, i + 64) of a row, interleaved pairs (2i, 2i + 1); a pair (a, b)
of fp16 inputs at position p becomes

    first  = f16( f32(a * c) - f32(b * s) )
    second = f16( f32(b * c) + f32(a * s) )

with every product and the sum a separate, rounded fp32 operation.  :func:`rope_ref` is that, written with
separate fp32 tensor operations (torch does not fuse them on the CPU).  :func:`rope_ref_contracted` is the
planted fault: each output as one fused multiply-add would give it.
"""
import torch

D = 128
MAX_POS = 331     # not a multiple of anything the kernels use


def table(max_pos: int = MAX_POS) -> torch.Tensor:
    from quantizedattention_amd.attention_mxfp4 import rope_table
    return rope_table(max_pos)


def _pairs(x: torch.Tensor, interleaved: bool):
    """(first elements, second elements) of every pair, each [..., 64], pair i at index i."""
    return (x[..., 0::2], x[..., 1::2]) if interleaved else (x[..., :D // 2], x[..., D // 2:])


def _unpair(first: torch.Tensor, second: torch.Tensor, interleaved: bool) -> torch.Tensor:
    if interleaved:
        return torch.stack([first, second], -1).reshape(*first.shape[:-1], D)
    return torch.cat([first, second], -1)


def _cos_sin(tab: torch.Tensor, pos, like: torch.Tensor):
    """cos, sin fp32 [T, 1, 64] of the positions (one per token of ``like`` [T, H, 128])."""
    pos = torch.as_tensor(pos, dtype=torch.long)
    assert tab.dtype == torch.float32 and tab.shape[1] == D and pos.shape == (like.shape[0],)
    assert int(pos.min()) >= 0 and int(pos.max()) < tab.shape[0]
    rows = tab[pos]
    return rows[:, None, :D // 2], rows[:, None, D // 2:]


def rope_ref(x: torch.Tensor, tab: torch.Tensor, pos, interleaved: bool) -> torch.Tensor:
    """x fp16 [T, H, 128] on the CPU rotated by pos[token] -> fp16 [T, H, 128]; the contract above."""
    assert x.dtype == torch.float16 and x.dim() == 3 and x.shape[2] == D and not x.is_cuda
    c, s = _cos_sin(tab, pos, x)
    a, b = (t.float() for t in _pairs(x, interleaved))
    ac, bs, bc, as_ = a * c, b * s, b * c, a * s          # four rounded fp32 products
    return _unpair((ac - bs).half(), (bc + as_).half(), interleaved)


def rope_ref_contracted(x: torch.Tensor, tab: torch.Tensor, pos, interleaved: bool) -> torch.Tensor:
    """The planted fault: first = f16(fma(a, c, -f32(b s))), second = f16(fma(b, c, f32(a s))).  The fused
    product is emulated in float64, where the product of two fp32 values is exact, and rounded once."""
    c, s = _cos_sin(tab, pos, x)
    a, b = (t.float() for t in _pairs(x, interleaved))
    bs, as_ = (b * s).double(), (a * s).double()
    first = (a.double() * c.double() - bs).float().half()
    second = (b.double() * c.double() + as_).float().half()
    return _unpair(first, second, interleaved)


def rope_exact(x: torch.Tensor, tab: torch.Tensor, pos, interleaved: bool):
    """The rotation by the table's own cos and sin as a float64 complex product, no rounding that matters
    -> (rotated float64 [T, H, 128], |a c| + |b s| resp. |b c| + |a s| per element, float64)."""
    c, s = (t.double() for t in _cos_sin(tab, pos, x))
    a, b = (t.double() for t in _pairs(x, interleaved))
    z = torch.complex(a, b) * torch.complex(c, s)
    mag = _unpair((a * c).abs() + (b * s).abs(), (b * c).abs() + (a * s).abs(), interleaved)
    return _unpair(z.real, z.imag, interleaved), mag


# ------------------------------------------------------------------ the inputs the GPU tests use
# Every tensor below is rotated by both the CPU and the GPU tests, at the positions written out here by hand
# (tests/test_mxfp4_rope_ref.py holds rope_positions to them).  A fused multiply-add moves an fp32 result by
# an ulp, which survives the rounding to fp16 about once in 2^13 elements and the MX-FP4 quantiser far more
# rarely still, so random data alone would not let a bit-for-bit comparison see a contracting kernel.  Each
# tensor therefore carries two planted pairs, one per pairing (WITNESS: token, head, pair index, the fp16
# bit patterns of a and b), found by a seeded search on the CPU: rope_ref and rope_ref_contracted differ on
# them in fp16 and in the quantised bytes (after the pool's k_mean where the test's pool has one).
def rand16(seed: int, *shape) -> torch.Tensor:
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).half()


def pair_elements(i: int, interleaved: bool):
    return (2 * i, 2 * i + 1) if interleaved else (i, i + D // 2)


def _planted(name: str, x: torch.Tensor) -> torch.Tensor:
    x = x.clone()
    for interleaved in (False, True):
        t, h, i, a, b = WITNESS[(name, interleaved)]
        ea, eb = pair_elements(i, interleaved)
        x[t, h, ea] = torch.tensor(a, dtype=torch.int16).view(torch.float16)
        x[t, h, eb] = torch.tensor(b, dtype=torch.int16).view(torch.float16)
    return x


# 1. the quantiser: 67 tokens x 3 heads (a partial last workgroup, an odd heads-per-token stride)
QUANT_T, QUANT_H = 67, 3
BLOCK_SCALES = (1.0, 1.0 / 32, 32.0, 512.0)   # per 32-element block of a row: partners differ by 2^5 and 2^14


def _quant_positions():
    pos = [0, MAX_POS - 1, 5, 5, 5, MAX_POS - 1] + list(range(60, 30, -1))
    g = torch.Generator().manual_seed(12)
    return pos + torch.randint(0, MAX_POS, (QUANT_T - len(pos),), generator=g).tolist()


def _quant_raw():
    x = torch.randn((QUANT_T, QUANT_H, D), generator=torch.Generator().manual_seed(11))
    return (x * torch.tensor(BLOCK_SCALES).repeat_interleave(32)).half()


def quant_inputs():
    """-> (x fp16 [67, 3, 128], positions): the blocks of a row differ in magnitude by 2^5 and more, so a
    rotated block's e8m0 byte depends on its partner block's values; the positions hold 0, MAX_POS - 1,
    repeats and a descending run."""
    return _planted("quantiser", _quant_raw()), _quant_positions()


# 2. the append: Hkv 2, three slots (slot 1 never listed), two steps: 0 -> 60 and 0 -> 5, then 60 -> 69
# (crosses a page of 64 and a V tile) and 5 -> 6
HKV, SLOTS, IDS = 2, 3, (2, 0)
STEPS = ((60, 5), (9, 1))
STEP_POS = (list(range(60)) + list(range(5)), list(range(60, 69)) + [5])
SHIFT = 17    # the explicit-position case: every default position + SHIFT


def _append_raw(step: int):
    return rand16(21 + step, sum(STEPS[step]), HKV, D)


def append_inputs(step: int):
    """-> (k, v) fp16 [sum(counts), 2, 128] of step 0 or 1."""
    return _planted(f"append {step}", _append_raw(step)), rand16(31 + step, sum(STEPS[step]), HKV, D)


def k_mean():
    return (0.25 * torch.randn((SLOTS, HKV, 1, D), generator=torch.Generator().manual_seed(41))).half()


# 3. attention: the pool of 2 grown to (slot 2, slot 0) = (209, 76) keys, so that at 64 keys per split both
# sequences have two splits or more, window 64 + 2 sinks leaves a gap in slot 2 (first window tile 2 > 1 sink
# tile) and a fork of slot 2 into slot 1 shares three full pages of 64
GROW = (140, 70)
GROW_POS = list(range(69, 209)) + list(range(6, 76))
LENGTHS = (76, 0, 209)       # per slot, after the growth
HQ, Q_LENS = 4, (7, 3)
Q_POS = list(range(202, 209)) + [73, 74, 75]
TREE = [-1, 0, 0, 1, 1]      # a branching 5-node tree: depths 0 1 1 2 2, behind 2 plain queries of slot 2
Q_POS_TREE = [202, 203, 204, 205, 205, 206, 206] + [73, 74, 75]
FORK_IDS, FORK_Q_LENS = (2, 0, 1), (7, 3, 2)      # slot 1 = fork of slot 2
FORK_Q_POS = Q_POS + [207, 208]


def grow_inputs():
    T = sum(GROW)
    return rand16(51, T, HKV, D), rand16(52, T, HKV, D)


def _q_raw():
    return rand16(53, sum(FORK_Q_LENS), HQ, D)


def attention_q(n: int = sum(Q_LENS)):
    """The first n packed query tokens (the fork case takes all 12)."""
    return _planted("attention", _q_raw())[:n].contiguous()


# 4. draft, verify, accept: L0 = 61, six draft nodes, the kept path 0 -> 1 -> 3 -> 4 of four nodes ends at 65
L0, DRAFT, LEAF = 61, [-1, 0, 0, 1, 3, 2], 4
DRAFT_POS = [61, 62, 62, 63, 64, 63]      # by depth
PATH, PATH_POS = [0, 1, 3, 4], [61, 62, 63, 64]


def prefill_inputs():
    return rand16(61, L0, HKV, D), rand16(62, L0, HKV, D)


def _draft_raw():
    return rand16(63, len(DRAFT), HKV, D)


def draft_inputs():
    return _planted("draft", _draft_raw()), rand16(64, len(DRAFT), HKV, D)


def quantised(rot: torch.Tensor, mean=None):
    """(codes, scale bytes) of rotated rows fp16 [..., 128] as the cache's row quantiser gives them on the
    CPU (oracle/mxfp4.py), after f16(x - mean) when the pool smooths its keys."""
    from oracle import mxfp4 as OM
    if mean is not None:
        rot = (rot.float() - mean.float()).half()
    return OM.quant_rows(rot.reshape(-1, D))


def witness_sites():
    """(name, unplanted tensor, positions, token, first head, k_mean rows [Hkv, 128] of the token's slot or
    None) of every planted pair; the interleaved witness goes to the next head."""
    km = k_mean()[IDS[0], :, 0]
    yield "quantiser", _quant_raw(), _quant_positions(), 40, 0, None
    yield "append 0", _append_raw(0), STEP_POS[0], 7, 0, km      # tokens of slot IDS[0]
    yield "append 1", _append_raw(1), STEP_POS[1], 3, 0, km
    yield "attention", _q_raw(), FORK_Q_POS, 1, 1, None      # a plain query of slot 2, at 203 in every mode
    yield "draft", _draft_raw(), DRAFT_POS, 1, 0, None        # node 1 of the kept path; that pool is unsmoothed


WITNESS = {
    ("quantiser", False): (40, 0, 3, 15812, 19209),
    ("quantiser", True): (40, 1, 18, -22455, 11398),
    ("append 0", False): (7, 0, 25, 14980, -17506),
    ("append 0", True): (7, 1, 15, 14692, 14993),
    ("append 1", False): (3, 0, 24, -17932, 15525),
    ("append 1", True): (3, 1, 35, 12153, 14810),
    ("attention", False): (1, 1, 42, -18213, -20793),
    ("attention", True): (1, 2, 25, 15802, -17354),
    ("draft", False): (1, 0, 50, -18179, 10896),
    ("draft", True): (1, 1, 19, 14675, -17335),
}
