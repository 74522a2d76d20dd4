"""Block-wise gradient parity: the helper of tests/test_grad_blocks.py (CPU) and
tests/test_gpu_grad_blocks.py (GPU).

A whole-tensor relL2 on i.i.d. randn inputs hides a mistake confined to a few 32-row blocks: every
block carries nearly the same norm and the same quantisation scale, so the wrong block's scale on an
edge tile, or one dropped (query tile, key tile) pair, moves the norm of the whole tensor by less than
the distance between kernel and oracle.  Three pieces close that:

  * ``block_rel``: the relL2 of every 32-row block on its own, no block left out, no floor;
  * ``ladder_inputs``: randn times a per-(batch, head, 32-row block) multiplier, drawn separately for
    q, k, v and dO, neighbouring blocks a factor of two or more apart, so that a neighbour's scale,
    lse or D row puts a block off by at least 50 %;
  * ``lit_dO``: dO zero outside one 32-row query tile of one query head.  dP and D = rowsum(dO * O)
    are then zero off that tile, so dq is exactly zero outside its rows, dk and dv exactly zero for
    every other key/value head and batch entry (and, causal, for every key tile past it), and each
    32-key block of dk / dv on the lit head is the contribution of one (query tile, key tile) pair.
"""
import torch

BLOCK = 32

# multipliers of the ladder (int8: q, k keep the scores inside the f16 exponent range of the
# reference's softmax; bf16: larger logits send the reference's beta rule to NaN, tests/test_gpu_fuzz.py)
QK_INT8 = (0.5, 1.0, 2.0)
QK_BF16 = (0.4, 0.7, 1.0)
V_DO = (0.25, 0.5, 1.0, 2.0, 4.0)

# Per-block bars: three times the whole-tensor bars of the same comparison (3 * conftest.INT8_BWD_REL
# = conftest.INT8_BWD_REL_FUZZ for int8; 3 * the 1e-2 of tests/test_gpu_bf16.py for bf16).  On the CPU a
# restatement of the int8 kernel's first documented departure (fp32 S and P) sits at most 0.0119 from
# the oracle on any block of the four shapes below, and the bf16 oracle at most 0.0195 per block from
# fp32 autograd: block by block costs about 2x the whole-tensor figure, 3x leaves the usual margin.
BF16_BWD_REL = 1e-2
BF16_BLOCK_REL = 3 * BF16_BWD_REL

# (B, Hq, Hkv, Sq, Sk, D, causal): Sk = 288 / 320 is one full 256-key dK+dV workgroup plus a partial
# one, five or six (nine) query tiles wrap the 4-slot rings, every case has two or more query heads per
# key/value head or an odd head count, B * Hq is no multiple of 8, and the causal cases have 6
# key/value heads in all (a partial group of four for the grouped causal grid order).
SHAPES = [(1, 2, 2, 160, 288, 64, False), (2, 6, 3, 160, 288, 64, True),
          (1, 4, 2, 192, 320, 128, False), (1, 6, 6, 288, 288, 128, True)]


def shape_id(s):
    return "x".join(str(int(x)) for x in s[:6]) + ("-causal" if s[6] else "")


def block_rel(a, ref):
    """[B, H, S, D] -> [B, H, S / 32]: ||a_b - r_b|| / ||r_b|| of every 32-row block b.  A block the
    oracle has exactly zero is not divided: it reads 0 where ``a`` is exactly zero there too (-0
    counts), and inf otherwise.  No other block is excluded and no denominator has a floor."""
    B, H, S, D = ref.shape
    assert a.shape == ref.shape and S % BLOCK == 0
    a = a.detach().double().cpu().reshape(B, H, S // BLOCK, BLOCK * D)
    r = ref.detach().double().cpu().reshape(B, H, S // BLOCK, BLOCK * D)
    num, den = (a - r).norm(dim=-1), r.norm(dim=-1)
    zero = (r == 0).all(-1)
    exact = (a == 0).all(-1)
    rel = num / torch.where(zero, torch.ones_like(den), den)
    return torch.where(zero, torch.where(exact, torch.zeros_like(rel), torch.full_like(rel, float("inf"))),
                       rel)


def whole_rel(a, ref):
    return ((a.double().cpu() - ref.double().cpu()).norm() / ref.double().cpu().norm()).item()


def ladder(B, H, S, choices, gen):
    """[B, H, S, 1] multipliers, constant over each 32-row block, drawn from ``choices``; two
    neighbouring blocks never get the same one."""
    n = S // BLOCK
    idx = torch.empty((B, H, n), dtype=torch.long)
    idx[..., 0] = torch.randint(len(choices), (B, H), generator=gen)
    for i in range(1, n):   # any of the other len - 1 choices
        idx[..., i] = (idx[..., i - 1] + 1 + torch.randint(len(choices) - 1, (B, H), generator=gen)) % len(choices)
    return torch.tensor(choices)[idx].repeat_interleave(BLOCK, dim=-1).unsqueeze(-1)


def free_ladder(B, H, S, choices, gen):
    """As ``ladder`` with every block drawn on its own (neighbours may coincide)."""
    idx = torch.randint(len(choices), (B, H, S // BLOCK), generator=gen)
    return torch.tensor(choices)[idx].repeat_interleave(BLOCK, dim=-1).unsqueeze(-1)


def ladder_inputs(shape, path, seed):
    """fp32 (q, k, v, dO) of the ladder and their four multiplier tensors.  ``path`` "int8": q, k in
    {0.5, 1, 2}; "bf16": q, k in {0.4, 0.7, 1.0}, every block drawn on its own.  v, dO in
    {0.25 .. 4} on both.  The caller casts to the path's dtypes."""
    B, Hq, Hkv, Sq, Sk, D = shape[:6]
    g = torch.Generator().manual_seed(seed)
    dims = ((B, Hq, Sq), (B, Hkv, Sk), (B, Hkv, Sk), (B, Hq, Sq))
    if path == "int8":
        mult = [ladder(*dims[0], QK_INT8, g), ladder(*dims[1], QK_INT8, g)]
    else:
        mult = [free_ladder(*dims[0], QK_BF16, g), free_ladder(*dims[1], QK_BF16, g)]
    mult += [ladder(*dims[2], V_DO, g), ladder(*dims[3], V_DO, g)]
    xs = [torch.randn(d + (D,), generator=g) * m for d, m in zip(dims, mult)]
    return xs, mult


def randn_inputs(shape, seed):
    B, Hq, Hkv, Sq, Sk, D = shape[:6]
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g) for s in ((B, Hq, Sq, D), (B, Hkv, Sk, D), (B, Hkv, Sk, D))]


def lit_tile(shape):
    """(batch entry, query head, query tile) of the lit tile: the last batch entry, the last query head
    (so the last key/value group), a tile that is neither the first nor the last."""
    B, Hq, Hkv, Sq = shape[:4]
    return B - 1, Hq - 1, (Sq // BLOCK) // 2


def lit_dO(shape, seed, like=None):
    """dO that is zero except for the lit tile (randn there, or the rows of ``like``)."""
    B, Hq, Hkv, Sq, Sk, D = shape[:6]
    b, h, t = lit_tile(shape)
    dO = torch.zeros((B, Hq, Sq, D))
    rows = slice(BLOCK * t, BLOCK * t + BLOCK)
    dO[b, h, rows] = (torch.randn((BLOCK, D), generator=torch.Generator().manual_seed(seed))
                      if like is None else like[b, h, rows].float())
    return dO


def lit_zero_masks(shape):
    """Boolean masks of the entries the lit tile must leave exactly zero: (dq [B,Hq,Sq], dkv [B,Hkv,Sk])."""
    B, Hq, Hkv, Sq, Sk, D, causal = shape
    b, h, t = lit_tile(shape)
    zq = torch.ones((B, Hq, Sq), dtype=torch.bool)
    zq[b, h, BLOCK * t:BLOCK * t + BLOCK] = False
    zk = torch.ones((B, Hkv, Sk), dtype=torch.bool)
    zk[b, h // (Hq // Hkv), :min(Sk, BLOCK * t + BLOCK) if causal else Sk] = False
    return zq, zk


def assert_lit_zeros(shape, dq, dk, dv, who):
    zq, zk = lit_zero_masks(shape)
    for name, x, z in (("dq", dq, zq), ("dk", dk, zk), ("dv", dv, zk)):
        bad = (x.detach().cpu()[z] != 0)
        assert not bad.any(), (who, name, int(bad.sum()), "entries off the lit tile are not zero")
        assert (x.detach().cpu()[~z] != 0).any(), (who, name, "the lit part is empty")


def flush_denormals(*xs):
    """The bf16 reference fills masked scores with -128 (bf16:379-389), so a masked P is
    exp2(-128 - lse), about 1e-40: an fp32 denormal, which a GPU's exp2 returns as 0 and the CPU's
    does not.  A key tile no lit query sees then holds dk, dv of about 1e-40 in the CPU restatement
    and exactly 0 on the GPU.  This reads the restatement's denormal results as the zeros they are
    there (nothing else changes: the next larger value is 1.2e-38)."""
    tiny = torch.finfo(torch.float32).tiny
    return tuple(torch.where(x.abs() < tiny, torch.zeros_like(x), x) for x in xs)


def check(path, grads, refs, block_bar, whole_bar):
    """Print and assert the per-block and whole-tensor distances of (dq, dk, dv) from the oracle's."""
    worst = {}
    for name, a, r in zip(("dq", "dk", "dv"), grads, refs):
        assert torch.isfinite(a).all(), (path, name)
        br = block_rel(a, r)
        worst[name] = (br.max().item(), whole_rel(a, r), tuple(int(i) for i in (br == br.max()).nonzero()[0]))
        print(f"RELL2-BLOCK {path} {name} {worst[name][0]:.5f}")
        print(f"RELL2 {path} {name} {worst[name][1]:.5f}")
    for name, (blk, whole, where) in worst.items():
        assert blk <= block_bar, (path, name, "block (b, h, s/32)", where, blk)
        assert whole <= whole_bar, (path, name, whole)
    return worst
