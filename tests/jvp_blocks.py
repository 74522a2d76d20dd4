"""Block-wise parity of the forward-mode kernel (csrc/jvp_fwd.hip): the helper of
tests/test_jvp_blocks.py (CPU) and tests/test_gpu_jvp_blocks.py (GPU).

The whole-tensor max-abs bars of tests/test_gpu_jvp.py are tight only on randn inputs, where the
running max never moves after the first key tile; where it moves (tests/test_gpu_edge.py,
tests/test_gpu_fuzz.py) the bar is a worst-case operand bound that a 500-fold loss of accuracy still
passes.  Here tO is held 32-row block by 32-row block (grad_blocks.block_rel) against
``torch.func.jvp`` in float64, under bars that come from a CPU restatement of the kernel's own
arithmetic (``restate``): three times the restatement's worst block, per mode and input family.

Families: the *ladder* (randn times a multiplier per (batch, head, 32-row block), drawn separately for
each of the six operands; q, k in {0.5, 1, 2} spread the logits enough to move the running max after
the first tile), *lit* tangents (zero outside one 32-row block of one head of the last batch entry:
exact zeros wherever that block cannot reach, and one launch per key block shows a misplaced
half-stage or ring slot at the block where it happens) and the *climb* (keys scaled by a ramp, the
inputs of test_gpu_edge.test_jvp_running_max_moves: logits to |S| ~ 45, the max moves on most tiles).
"""
import math

import torch

import grad_blocks as GB

from oracle import restate as R

BLOCK = GB.BLOCK
JVP_THR = 8.0          # jvp_fwd.hip:30
MODES = ("bf16", "fp32")
TERMS = ("tq", "tk", "tv", "all")
QK = (0.5, 1.0, 2.0)

# (B, Hq, Hkv, Sq, Sk, D).  Sq = 160 / 96 / 288 / 64 leaves one to three of a workgroup's four waves
# idle; 192 / 320 / 128 keys are 3, 5 and 2 sixty-four-key stages of the bf16 mode (the two-slot ring
# wrapped an odd and an even number of times; 6, 10 and 4 stages of the fp32 mode); Sk = 96 is an odd
# count of 32-key stages, which only the fp32 mode admits; grouped and odd head counts.
SHAPES = [(1, 2, 2, 160, 192, 64), (2, 6, 3, 96, 320, 64), (1, 4, 2, 192, 320, 128),
          (1, 3, 3, 288, 128, 128)]
FP32_ONLY = (1, 2, 1, 64, 96, 64)
LIT_SHAPES = [(2, 6, 3, 96, 192, 64), (1, 4, 2, 160, 320, 128)]
CLIMB_SHAPE = (1, 2, 2, 256, 256, 128)
LADDER_SEED, LIT_SEED = 301, 302

# Bars: 3 x the worst figure of ``restate`` against ``truth`` over every case of the family (every
# shape of the mode, every term of TERMS; lit: every launch of lit_cases), the 3 x of grad_blocks.py:
# room for the summation order inside an MFMA and for v_exp_f32 / v_log_f32.  tO and O: relL2 of the worst 32-row
# block; lse: max-abs (log2 units).  The measured figure stands beside each constant, which is that
# figure rounded up by 3 to 7 % (a CPU's exp2 may differ in the last place);
# tests/test_jvp_blocks.py holds the restatement between 0.8 of a third of each and that third.
BARS = {
    # (mode, family): (tO block, O block, lse abs)
    ("bf16", "ladder"): (3 * 7.6e-3, 3 * 2.0e-3, 3 * 2.3e-6),    # measured 7.40e-3, 1.91e-3, 2.24e-6
    ("bf16", "lit"): (3 * 2.8e-3, 3 * 1.9e-3, 3 * 9.0e-7),       # 2.66e-3, 1.82e-3, 8.41e-7
    ("bf16", "climb"): (3 * 1.75e-2, 3 * 3.5e-4, 3 * 1.3e-5),    # 1.695e-2 (the tk term), 3.36e-4, 1.21e-5
    ("fp32", "ladder"): (3 * 1.4e-5, 3 * 3.6e-6, 3 * 6.0e-6),    # 1.34e-5, 3.45e-6, 5.79e-6
    ("fp32", "lit"): (3 * 4.7e-6, 3 * 3.0e-6, 3 * 9.2e-7),       # 4.48e-6, 2.85e-6, 8.82e-7
    ("fp32", "climb"): (3 * 2.4e-5, 3 * 1.1e-6, 3 * 2.5e-5),     # 2.31e-5 (the tk term), 1.04e-6, 2.37e-5
}


def shape_id(s):
    return "x".join(str(int(x)) for x in s)


def shapes(mode, base=None):
    return list(SHAPES if base is None else base) + ([FP32_ONLY] if mode == "fp32" else [])


def split(x, mode):
    """The float64 images of an operand as the kernel multiplies it: [bf16(x)], or in the fp32 mode
    [hi, lo] = [bf16(x), bf16(x - bf16(x))] (split_bf16_kernel, jvp_fwd.hip:274-284)."""
    x = x.float()
    hi = x.bfloat16().float()
    if mode == "bf16":
        return [hi.double()]
    return [hi.double(), (x - hi).bfloat16().double()]


def images(x, mode):
    """The operand's value to the kernel: the sum of its images (exact in float64)."""
    return sum(split(x, mode))


def mfma(acc, prods):
    """acc (fp32 [..., M, N]) += sum over ``prods`` of rows . cols^T, as the kernel's MFMA chains
    accumulate it: 16 of the contracted index per v_mfma_f32_32x32x16_bf16, within such a step the
    products of ``prods`` in turn and of each product the image pairs in the order of ``mm``
    (jvp_fwd.hip:128-136: A hi . B hi, A hi . B lo, A lo . B hi, A lo . B lo, where A is the operand that
    indexes the columns here), and the fp32 accumulator rounded once per instruction (its 16 products
    summed exactly)."""
    K = prods[0][0][0].shape[-1]
    for c in range(0, K, 16):
        ch = slice(c, c + 16)
        for rows, cols in prods:
            for a in cols:
                for b in rows:
                    acc = (acc.double() + b[..., ch] @ a[..., ch].transpose(-1, -2)).float()
    return acc


def to_mode(x, mode):
    """The tensor handed to attention_jvp._jvp: bf16 selects the bf16 kernel, fp32 the split one."""
    return x.bfloat16() if mode == "bf16" else x.float()


def restate(q, k, v, tq, tk, tv, mode, fault=None, stats=None):
    """jvp_fwd_kernel (csrc/jvp_fwd.hip) as written, on the CPU -> (O, tO, lse [B*Hq, Sq]).

      * operands: bf16, or hi + lo (:20-22, :99-104; ``images``); query head h reads key/value head
        h // G (:111);
      * S^T = K q^T and tS^T = K tq^T + tK q^T (:146-163), accumulated in fp32 over the D / 16 MFMA
        steps and, in the fp32 mode, the four image pairs of each (``mfma``).  (With exact sums rounded once
        to fp32 the fp32 mode's lse is 6.1e-6 from the truth on the climb and the kernel's 2.7e-5:
        |S| reaches 512 there before the scale, one fp32 step of S is 8e-6 of lse, and the kernel
        rounds the accumulator after each of its 32 MFMAs; restated so, 2.4e-5.);
      * 32-key tiles: the ``u`` loop of a 64-key stage in the bf16 mode, a stage in the fp32 mode
        (:42, :145);
      * cand = max(m, rowmax * qks) (:164-175); when any of a wave's 32 rows has cand > m + 8, all 32
        take m = cand and rs = exp2(m - cand) on l, racc, O and AB (:176-187);
      * P = exp2(S * qks - m), H = P * (tS * sm); l and racc summed in fp32 from the unrounded P and H
        (:188-201); a P below the normal range is zero (raw v_exp_f32, common.h:112).  hipcc contracts
        S * qks - m to one v_fma_f32 (a single rounding: at |S qks| ~ 64 the product's own rounding
        would cost 4e-6 of P), and the same default contraction applies to AB - racc * O;
      * P and H rounded to bf16, or to hi + lo, for O += P V and AB += P tV + H V, 16 keys per MFMA
        step, the two chains of AB interleaved step by step (:203-246);
      * lse = m + log2(l), O = O / l, tO = (AB - racc * O) / l (:255-265).

    ``fault`` (tests/test_jvp_blocks.py only) plants one mistake: "h_lo" drops H's lo residual in the
    fp32 mode, "tk_prev" reads the last 32-key block's tK from the block before it, "tv_cols" takes
    the last 32 columns of tV from V on the last key block, "racc_unscaled" leaves racc out of the
    rescale, "racc_neighbour" finishes every query block with the previous block's racc.
    ``stats``: a dict that receives the count of (wave block, key tile after the first) pairs and of
    those that moved the running max."""
    assert mode in MODES and fault in (None, "h_lo", "tk_prev", "tv_cols", "racc_unscaled", "racc_neighbour")
    B, Hq, Sq, D = q.shape
    Hkv, Sk = k.shape[1:3]
    G = Hq // Hkv
    f32 = torch.float32
    qks, sm = torch.tensor(R.qk_scale(D), dtype=f32), torch.tensor(R.sm_scale(D), dtype=f32)
    qi, tqi = split(q, mode), split(tq, mode)
    ki, vi, tki, tvi = ([y.repeat_interleave(G, dim=1) for y in split(x, mode)] for x in (k, v, tk, tv))
    cut = lambda imgs, ks: [y[:, :, ks] for y in imgs]  # noqa: E731
    T = lambda imgs: [y.transpose(-1, -2) for y in imgs]  # noqa: E731
    m = torch.full((B, Hq, Sq), float("-inf"), dtype=f32)
    l, racc = torch.zeros((B, Hq, Sq), dtype=f32), torch.zeros((B, Hq, Sq), dtype=f32)
    O, AB = torch.zeros((B, Hq, Sq, D), dtype=f32), torch.zeros((B, Hq, Sq, D), dtype=f32)
    tiny = torch.finfo(f32).tiny
    pairs = moved = 0
    for k0 in range(0, Sk, BLOCK):
        last = k0 + BLOCK == Sk
        ks = slice(k0, k0 + BLOCK)
        kt, vt, tkt, tvt = cut(ki, ks), cut(vi, ks), cut(tki, ks), cut(tvi, ks)
        if fault == "tk_prev" and last:
            tkt = cut(tki, slice(k0 - BLOCK, k0))
        if fault == "tv_cols" and last:
            tvt = [torch.cat([t[..., :D - 32], y[..., D - 32:]], -1) for t, y in zip(tvt, vt)]
        zero = torch.zeros((B, Hq, Sq, BLOCK), dtype=f32)
        S = mfma(zero, [(qi, kt)])
        tS = mfma(zero, [(tqi, kt), (qi, tkt)])
        cand = torch.maximum(m, S.amax(-1) * qks)
        move = (cand > m + JVP_THR).reshape(B, Hq, Sq // BLOCK, BLOCK).any(-1)
        if k0:
            pairs, moved = pairs + move.numel(), moved + int(move.sum())
        move = move.repeat_interleave(BLOCK, dim=-1)
        rs = torch.where(move, torch.exp2(m - cand), torch.ones_like(m))
        m = torch.where(move, cand, m)
        l = l * rs
        if fault != "racc_unscaled":
            racc = racc * rs
        O, AB = O * rs[..., None], AB * rs[..., None]
        P = torch.exp2((S.double() * qks.double() - m[..., None].double()).float())   # one v_fma_f32
        P = torch.where(P < tiny, torch.zeros_like(P), P)
        H = P * (tS * sm)
        l = l + P.sum(-1)
        racc = racc + H.sum(-1)
        Pi, Hi = split(P, mode), split(H, "bf16" if fault == "h_lo" else mode)
        O = mfma(O, [(Pi, T(vt))])
        AB = mfma(AB, [(Pi, T(tvt)), (Hi, T(vt))])
    if stats is not None:
        stats.update(pairs=pairs, moved=moved)
    lse = m + torch.log2(l)
    Of = O / l[..., None]
    if fault == "racc_neighbour":
        racc = racc.roll(BLOCK, dims=-1)
    tO = (AB.double() - racc[..., None].double() * Of.double()).float() / l[..., None]   # contracted
    return Of, tO, lse.reshape(B * Hq, Sq)


def truth(q, k, v, tq, tk, tv, mode):
    """torch.func.jvp of softmax attention in float64 on the same rounded inputs (``images``), keys
    and values expanded over the group -> (O, tO, lse in log2 units [B*Hq, Sq])."""
    B, Hq, Sq, D = q.shape
    G = Hq // k.shape[1]
    qd, tqd = images(q, mode), images(tq, mode)
    kd, vd, tkd, tvd = (images(x, mode).repeat_interleave(G, dim=1) for x in (k, v, tk, tv))
    s = 1.0 / math.sqrt(D)
    f = lambda a, b, c: torch.softmax(a @ b.transpose(-1, -2) * s, -1) @ c  # noqa: E731
    O, tO = torch.func.jvp(f, (qd, kd, vd), (tqd, tkd, tvd))
    lse = torch.logsumexp(qd @ kd.transpose(-1, -2) * s, -1) / math.log(2.0)
    return O, tO, lse.reshape(B * Hq, Sq)


def dims(shape):
    B, Hq, Hkv, Sq, Sk, D = shape
    return (B, Hq, Sq, D), (B, Hkv, Sk, D)


def ladder_inputs(shape, seed=LADDER_SEED):
    """fp32 [q, k, v, tq, tk, tv]: q and k randn times grad_blocks.free_ladder over (0.5, 1, 2); v, tq,
    tk and tv each randn times a grad_blocks.ladder of its own over V_DO."""
    qs, ks = dims(shape)
    g = torch.Generator().manual_seed(seed)
    order = (qs, ks, ks, qs, ks, ks)
    mult = [GB.free_ladder(*qs[:3], QK, g), GB.free_ladder(*ks[:3], QK, g)]
    mult += [GB.ladder(*s[:3], GB.V_DO, g) for s in order[2:]]
    return [torch.randn(s, generator=g) * mu for s, mu in zip(order, mult)]


def ramp_inputs(shape, seed, kscale):
    """test_gpu_edge._ramp_inputs (tests/test_jvp_blocks.py holds the two equal)."""
    B, H, S, D = shape
    g = torch.Generator().manual_seed(seed)
    ramp = (1.0 + torch.arange(S, dtype=torch.float32) / kscale).view(1, 1, S, 1)
    q = torch.randn(shape, generator=g)
    k = torch.randn(shape, generator=g) * ramp
    v = torch.randn(shape, generator=g)
    return q, k, v


def climb_inputs():
    """The inputs of test_gpu_edge.test_jvp_running_max_moves: a key ramp of 1 .. 17, randn tangents."""
    q, k, v = ramp_inputs((1, 2, 256, 128), 46, kscale=16.0)
    g = torch.Generator().manual_seed(47)
    return [q, k, v] + [torch.randn(q.shape, generator=g) for _ in range(3)]


def term(tans, which):
    """(tq, tk, tv) with every tangent but ``which`` zero ("all": as they are)."""
    return [t if which in ("all", n) else torch.zeros_like(t) for n, t in zip(TERMS, tans)]


def lit_block(shape, which, block):
    """(batch entry, head, rows) of the lit block: the last batch entry; the last query head for tq,
    the last key/value head for tk and tv."""
    B, Hq, Hkv = shape[:3]
    return B - 1, (Hq if which == "tq" else Hkv) - 1, slice(BLOCK * block, BLOCK * block + BLOCK)


def lit(shape, which, block, seed=LIT_SEED):
    """(tq, tk, tv), all zero except one 32-row block of ``which`` (randn there)."""
    qs, ks = dims(shape)
    tans = [torch.zeros(qs), torch.zeros(ks), torch.zeros(ks)]
    b, h, rows = lit_block(shape, which, block)
    g = torch.Generator().manual_seed(seed + 1 + TERMS.index(which))
    tans[TERMS.index(which)][b, h, rows] = torch.randn((BLOCK, qs[3]), generator=g)
    return tans


def lit_primals(shape, seed=LIT_SEED):
    return GB.randn_inputs(shape, seed)


def lit_cases(shape):
    """Every lit launch of a shape: tq on one middle query block, then tk and tv on each 32-key block
    in turn."""
    Sq, Sk = shape[3], shape[4]
    return [("tq", (Sq // BLOCK) // 2)] + [(w, j) for w in ("tk", "tv") for j in range(Sk // BLOCK)]


def lit_zero_mask(shape, which, block):
    """[B, Hq, Sq] bool: the rows of tO that the lit block cannot reach (they must be exactly zero)."""
    B, Hq, Hkv, Sq = shape[:4]
    z = torch.ones((B, Hq, Sq), dtype=torch.bool)
    b, h, rows = lit_block(shape, which, block)
    if which == "tq":
        z[b, h, rows] = False
    else:
        G = Hq // Hkv
        z[b, h * G:(h + 1) * G] = False
    return z


def assert_lit_zeros(shape, which, block, tO, who):
    z = lit_zero_mask(shape, which, block)
    x = tO.detach().cpu()
    bad = x[z] != 0          # -0 counts as zero
    assert not bad.any(), (who, which, block, int(bad.sum()), "entries the lit block cannot reach are not zero")
    assert (x[~z] != 0).any(), (who, which, block, "the lit part is empty")


def figures(got, ref):
    """(worst tO block, worst O block, lse max-abs, tO whole relL2, where the worst tO block is)."""
    O, tO, lse = got
    Or, tOr, lser = ref
    for x in (O, tO, lse):
        assert torch.isfinite(x).all()
    bt, bo = GB.block_rel(tO, tOr), GB.block_rel(O, Or)
    where = tuple(int(i) for i in (bt == bt.max()).nonzero()[0])
    return (bt.max().item(), bo.max().item(), (lse.double().cpu() - lser).abs().max().item(),
            GB.whole_rel(tO, tOr), where)


def check(path, got, ref, bars):
    """Print and assert tO and O block by block, lse in absolute terms, against ``ref`` (truth)."""
    t, o, ls, whole, where = figures(got, ref)
    print(f"RELL2-BLOCK {path} tO {t:.3e}")
    print(f"RELL2-BLOCK {path} O {o:.3e}")
    print(f"RELL2 {path} tO {whole:.3e}")
    print(f"ABS {path} lse {ls:.3e}")
    assert t <= bars[0], (path, "tO block (b, h, s/32)", where, t, bars[0])
    assert whole <= bars[0], (path, "tO", whole)     # a norm over the tensor is no larger than its worst block's
    assert o <= bars[1], (path, "O block", o, bars[1])
    assert ls <= bars[2], (path, "lse", ls, bars[2])
    return t, o, ls
