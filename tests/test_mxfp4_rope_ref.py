"""CPU tests of the rotary layer of the packed MX-FP4 cache path: the table, the contract's restatement
(tests/mxfp4_rope_ref.py), the default positions, the host refusals, and -- on the very tensors
tests/test_gpu_mxfp4_rope.py compares bit for bit -- that the faults those comparisons are meant to catch
(a fused multiply-add, the other pairing, a position off by one) do change fp16 elements.
"""
import math

import pytest
import torch

import mxfp4_rope_ref as R


def _err():
    from quantizedattention_amd._lib import QAttnError
    return QAttnError


# ------------------------------------------------------------------ the table
def test_rope_table_is_the_rounded_float64_table():
    """fp32 [max_pos, 128], cos in columns [0, 64), sin in [64, 128), each float32(f(float64 angle)) with
    angle = p * base ** (-2 i / 128) in float64."""
    from quantizedattention_amd.attention_mxfp4 import rope_table
    for max_pos, base in ((R.MAX_POS, 10000.0), (7, 500000.0)):
        t = rope_table(max_pos, base)
        assert t.dtype == torch.float32 and tuple(t.shape) == (max_pos, 128) and t.is_contiguous()
        p = torch.arange(max_pos, dtype=torch.float64)[:, None]
        inv = torch.pow(torch.tensor(base, dtype=torch.float64), -2.0 * torch.arange(64, dtype=torch.float64) / 128)
        assert torch.equal(t[:, :64], (p * inv).cos().float()) and torch.equal(t[:, 64:], (p * inv).sin().float())
        for pp, i in ((0, 0), (1, 0), (max_pos - 1, 63), (max_pos // 2, 17)):   # the formula itself, by libm
            ang = pp * base ** (-2.0 * i / 128)
            assert abs(float(t[pp, i]) - math.cos(ang)) <= 2.0 ** -23
            assert abs(float(t[pp, 64 + i]) - math.sin(ang)) <= 2.0 ** -23
    assert torch.equal(R.table(), rope_table(R.MAX_POS))          # deterministic
    for bad in ((0, 10000.0), (4, 0.0)):
        with pytest.raises(_err(), match="rope"):
            rope_table(*bad)


def test_rope_holder_refuses_on_the_host():
    from quantizedattention_amd.attention_mxfp4 import Rope
    t = R.table(8)
    for bad in (t.double(), t[:, :64], t.t(), t.view(-1)):
        with pytest.raises(_err(), match="contiguous fp32"):
            Rope(bad)
    with pytest.raises(_err(), match="no CPU fallback"):
        Rope(t)


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("interleaved", [False, True])
def test_position_zero_is_the_identity(interleaved):
    x, _ = R.quant_inputs()
    out = R.rope_ref(x, R.table(), [0] * x.shape[0], interleaved)
    assert torch.equal(out.view(torch.int16), x.view(torch.int16))


@pytest.mark.parametrize("interleaved", [False, True])
def test_rope_ref_within_its_four_roundings(interleaved):
    """Against the float64 complex rotation (a + ib)(c + is) by the table's own c and s, r = a c - b s (and
    b c + a s).  rope_ref rounds four times.  With u = 2^-24: the two products carry relative errors e1,
    e2 <= u and the sum e3 <= u, so the fp32 value y = (a c (1 + e1) - b s (1 + e2))(1 + e3) has
    |y - r| <= E32 = (2 u + u^2)(|a c| + |b s|).  The last rounding adds half an fp16 ulp of y: at most
    2^-11 |y| for a normal result and 2^-25 for a subnormal one, and |y| <= |r| + E32.  Hence
    |out - r| <= E32 + max(2^-11 (|r| + E32), 2^-25).  No result here overflows fp16."""
    x, pos = R.quant_inputs()
    out = R.rope_ref(x, R.table(), pos, interleaved).double()
    r, mag = R.rope_exact(x, R.table(), pos, interleaved)
    u = 2.0 ** -24
    e32 = (2 * u + u * u) * mag
    bound = e32 + torch.maximum(2.0 ** -11 * (r.abs() + e32), torch.full_like(r, 2.0 ** -25))
    assert torch.isfinite(out).all() and r.abs().max() < 60000
    excess = ((out - r).abs() - bound).max().item()
    assert excess <= 0, excess
    # and the bound is no formality: the error reaches a good part of it somewhere
    assert ((out - r).abs() / bound).max().item() > 0.5


# ------------------------------------------------------------------ default positions
def test_rope_positions_plain_and_consecutive_steps():
    from quantizedattention_amd.kv_cache_mxfp4 import rope_positions
    lengths = [6, 0, 60, 0]
    assert rope_positions(lengths, [2, 0], [3, 2]) == [60, 61, 62, 6, 7]
    assert rope_positions(lengths, [0], [1]) == [6]
    assert rope_positions(torch.tensor(lengths), torch.tensor([3]), torch.tensor([2])) == [0, 1]
    # the next step continues where the first ended
    after = [8, 0, 63, 0]
    assert rope_positions(after, [2, 0], [2, 1]) == [63, 64, 8]


def test_rope_positions_trees():
    from quantizedattention_amd.kv_cache_mxfp4 import rope_positions, tree_path
    # a chain is the plain step
    assert rope_positions([10], [0], [4], tree=[[-1, 0, 1, 2]]) == rope_positions([10], [0], [4]) == [10, 11, 12, 13]
    # a branching tree: siblings share a depth
    assert rope_positions([10], [0], [5], tree=[[-1, 0, 0, 1, 1]]) == [10, 11, 11, 12, 12]
    # queries in front of a tree, a sequence without one beside it, a forest (two roots)
    assert rope_positions([3, 100], [1, 0], [7, 2], tree=[R.TREE, None]) == [100, 101, 102, 103, 103, 104, 104, 3, 4]
    assert rope_positions([0], [0], [4], tree=[[-1, -1, 0, 1]]) == [0, 0, 1, 1]
    # every node of a path lands where an accept puts it: L0 + its index in the path
    parents = [-1, 0, 0, 1, 3, 2]
    pos = rope_positions([61], [0], [6], tree=[parents])
    path = tree_path(parents, 4)
    assert path == [0, 1, 3, 4] and [pos[t] for t in path] == [61, 62, 63, 64]


def test_rope_positions_refusals():
    from quantizedattention_amd.kv_cache_mxfp4 import rope_positions
    E = _err()
    for ids, cnt in (([], []), ([0, 0], [1, 1]), ([0], [1, 2]), ([4], [1]), ([-1], [1]), ([0], [0])):
        with pytest.raises(E, match="paged cache"):
            rope_positions([5, 5, 5, 5], ids, cnt)
    with pytest.raises(E, match="one entry"):
        rope_positions([5, 5], [0, 1], [2, 2], tree=[[-1]])
    with pytest.raises(E, match="tree of 3 nodes"):
        rope_positions([5], [0], [2], tree=[[-1, 0, 1]])
    with pytest.raises(E, match="topological"):
        rope_positions([5], [0], [3], tree=[[-1, 2, 0]])
    with pytest.raises(E, match="at most 64"):
        rope_positions([5], [0], [80], tree=[[-1] * 65])


def test_host_positions_are_held_to_the_table():
    """What append_packed, the varlen call and mxfp4_quantize_rows_rope do to a list or a host tensor of
    positions, before they touch a page or a device."""
    from quantizedattention_amd.attention_mxfp4 import _device_positions, _host_positions
    from quantizedattention_amd.kv_cache_mxfp4 import _rope_args
    E = _err()
    got = _host_positions([0, 7, 330], 3, R.MAX_POS)
    assert got.dtype == torch.int32 and not got.is_cuda and got.tolist() == [0, 7, 330]
    assert _host_positions(torch.tensor([4, 4]), 2, 5).tolist() == [4, 4]
    for bad in ([0, R.MAX_POS], [-1, 3], torch.tensor([0, 1 << 20])):
        with pytest.raises(E, match="outside the table"):
            _host_positions(bad, 2, R.MAX_POS)
    with pytest.raises(E, match="3 positions for 2"):
        _host_positions([1, 2, 3], 2, R.MAX_POS)
    assert not _device_positions([1, 2], 2) and not _device_positions(torch.tensor([1, 2]), 2)
    # positions or tree without rope
    default = lambda: ([5], [0], [2], None)  # noqa: E731
    assert _rope_args(None, None, None, 2, default) is None
    for pos, tree in (([0, 1], None), (None, [None])):
        with pytest.raises(E, match="without rope"):
            _rope_args(None, pos, tree, 2, default)
    with pytest.raises(E, match="must be a Rope"):
        _rope_args(R.table(), None, None, 2, default)


def test_default_positions_know_their_range():
    """The default positions are checked against the table by their lowest and highest value, which the
    builder reports; long runs come as ranges, short ones and tree nodes as lists, in packed order."""
    from quantizedattention_amd.kv_cache_mxfp4 import ARANGE_TOKENS, _default_positions
    n = ARANGE_TOKENS + 1
    cases = [([5, 0, 900], [2, 0], [n, 3], None), ([5, 0, 900], [0, 2, 1], [2, n + 7, n], [[-1, 0], None, None]),
             ([0], [0], [n + 5], [[-1, 0, 0, 1, 3]]), ([7, 7], [1, 0], [1, 1], None)]
    for lengths, ids, counts, tree in cases:
        pos, lo, hi = _default_positions(lengths, ids, counts, tree)
        want, first = [], 0
        for j, (b, c) in enumerate(zip(ids, counts)):      # the definition, token by token
            par = [] if tree is None or tree[j] is None else tree[j]
            depth = []
            for p in par:
                depth.append(depth[p] + 1 if p >= 0 else 0)
            want += [lengths[b] + i for i in range(c - len(par))] + [lengths[b] + c - len(par) + d for d in depth]
        assert pos.dtype == torch.int32 and pos.tolist() == want
        assert hi == max(want) and lo == min(lengths[b] for b in ids) <= min(want)


# ------------------------------------------------------------------ the GPU inputs can see the faults
def test_helper_positions_are_the_default_positions():
    """The positions tests/mxfp4_rope_ref.py writes out by hand for the GPU tests are what rope_positions
    gives at the lengths those tests reach."""
    from quantizedattention_amd.kv_cache_mxfp4 import rope_positions, tree_path
    lens = [0] * R.SLOTS
    for counts, want in zip(R.STEPS + (R.GROW,), R.STEP_POS + (R.GROW_POS,)):
        assert rope_positions(lens, R.IDS, counts) == want
        for b, c in zip(R.IDS, counts):
            lens[b] += c
    assert tuple(lens) == R.LENGTHS
    before = list(R.LENGTHS)
    for b, n in zip(R.IDS, R.Q_LENS):
        before[b] -= n
    assert rope_positions(before, R.IDS, R.Q_LENS) == R.Q_POS
    assert rope_positions(before, R.IDS, R.Q_LENS, tree=[R.TREE, None]) == R.Q_POS_TREE
    forked = [R.LENGTHS[0], R.LENGTHS[2], R.LENGTHS[2]]
    assert rope_positions([L - n for L, n in zip(forked, (3, 2, 7))], R.FORK_IDS, R.FORK_Q_LENS) == R.FORK_Q_POS
    assert rope_positions([R.L0], [0], [len(R.DRAFT)], tree=[R.DRAFT]) == R.DRAFT_POS
    assert tree_path(R.DRAFT, R.LEAF) == R.PATH
    assert [R.DRAFT_POS[t] for t in R.PATH] == R.PATH_POS == rope_positions([R.L0], [0], [len(R.PATH)])


def _gpu_cases():
    """(name, x, positions, k_mean row per token or None) of every rotation tests/test_gpu_mxfp4_rope.py
    compares, on the tensors it uses."""
    x, pos = R.quant_inputs()
    yield "quantiser", x, pos, None
    km = R.k_mean()[:, :, 0]                                       # [slot, Hkv, 128]
    for step, counts in enumerate(R.STEPS):
        slot = torch.tensor([b for b, c in zip(R.IDS, counts) for _ in range(c)])
        yield f"append {step}", R.append_inputs(step)[0], R.STEP_POS[step], km[slot]
    yield "attention", R.attention_q(), R.Q_POS, None
    yield "attention tree", R.attention_q(), R.Q_POS_TREE, None
    yield "attention fork", R.attention_q(sum(R.FORK_Q_LENS)), R.FORK_Q_POS, None
    yield "draft", R.draft_inputs()[0], R.DRAFT_POS, None
    yield "accepted path", R.draft_inputs()[0][R.PATH], R.PATH_POS, None


def _differ(a, b):
    return int((a.view(torch.int16) != b.view(torch.int16)).sum())


def _bytes_differ(a, b, mean):
    (c0, s0), (c1, s1) = R.quantised(a, mean), R.quantised(b, mean)
    return int((c0 != c1).sum()) + int((s0 != s1).sum())


@pytest.mark.parametrize("interleaved", [False, True])
def test_gpu_inputs_see_contraction_pairing_and_position_faults(interleaved):
    """A kernel that fuses its multiply-adds, pairs the elements the other way or is a position off changes
    fp16 elements of every rotated tensor the GPU tests compare -- and the MX-FP4 bytes those tests actually
    read, which is what the planted pairs of the helper are for."""
    tab = R.table()
    seen = 0
    for name, x, pos, mean in _gpu_cases():
        seen += 1
        good = R.rope_ref(x, tab, pos, interleaved)
        fused = R.rope_ref_contracted(x, tab, pos, interleaved)
        assert _differ(good, fused) >= 1 and _bytes_differ(good, fused, mean) >= 1, name
        other = R.rope_ref(x, tab, pos, not interleaved)
        assert _differ(good, other) >= x.numel() // 8 and _bytes_differ(good, other, mean) >= 1, name
        off = R.rope_ref(x, tab, [p + 1 if p + 1 < R.MAX_POS else p - 1 for p in pos], interleaved)
        assert _differ(good, off) >= x.numel() // 8 and _bytes_differ(good, off, mean) >= 1, name
    assert seen == 8


def test_tree_positions_differ_from_step_indices():
    """Placing the draft nodes by their index in the step, the documented trap, changes bytes too."""
    k = R.draft_inputs()[0]
    by_index = [R.L0 + i for i in range(len(R.DRAFT))]
    assert by_index != R.DRAFT_POS
    a, b = R.rope_ref(k, R.table(), R.DRAFT_POS, False), R.rope_ref(k, R.table(), by_index, False)
    assert _differ(a, b) > 0 and _bytes_differ(a, b, None) > 0
