"""Structured inputs for the MX-FP4 forwards, a classifier of the rows that sit on a rounding
boundary, and the comparison of a kernel result with the restatements.

TEST INFRASTRUCTURE ONLY, imported by plain name like ``mxfp4_masked_ref``.

Why: N(0, 1) inputs set the integer running max m in a row's first visible tile and never raise it
again, so the rescale branch of ``mx_tile`` (csrc/mxfp4_attn.hip), a raise inside a causal diagonal
tile or inside a key split, a tile in which only some rows of a wave raise, and a merge of splits
with very different m_s all stay unrun.  The families below make m move.

Input families -- ``family(shape, kind, seed, causal=0)``, shape = (B, Hq, Hkv, Sq, Sk), D = 128, fp16.
v ~ N(0, 1) in every family, so the absolute O bar keeps its meaning.  q, k, v are first drawn as
``mxfp4_masked_ref.randn_qkv`` draws them, then:

    randn    nothing more.
    ramp     k += u * linspace(0, RAMP_A, n_visible) along the keys (u a unit vector; the keys past
             n_visible, which no query sees, keep RAMP_A) and q += u * gain[row], gain ~ U(0, 8) per
             query row: the row max climbs at a rate of its own, so neighbouring rows raise m in
             different tiles and a wave raises partially.  n_visible = min(Sq, Sk) for causal = 1
             (top-left: no query sees more), else Sk.
    spikes   about n_visible / 96 random keys per key/value head times 6, query rows times 2^U(-1, 2).
    fall     the ramp reversed: tile 0 sets m and later tiles sink far below it (their P blocks take
             ever smaller scale bytes): such tiles must add next to nothing and no NaN.

Row classifier -- ``fragile_rows(q, k, causal, delta)``, from the restatement alone.  The kernel
takes exp2 from v_exp_f32 (1 ulp) where the restatement takes torch.exp2, so a P that sits on an
e2m1 rounding boundary of its block may take the neighbouring code on the GPU, and in a peaked row
one flipped code of a dominant P moves O by far more than the 2e-2 bar.  A row is fragile if in any
tile, for a visible element, y = P / block scale has 0 < |y - b| <= delta * b for a rounding boundary
b in {0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5}, or if a block's max argument a = fma(amx, qks, -m) has
0 < |a - round(a)| <= 2 * delta (the scale byte itself could flip).  Exact ties (S = 0: the argument
is an integer, P an exact power of two, exp2 exact on both sides) are not fragile.  delta = 2^-16 is
128 x the 1-ulp error of v_exp_f32 and about 4 x one ulp of an fp32 score of magnitude 100.  The key
split runs the same tiles from another m: its fp32 argument differs from the one-pass one by half an
ulp of a value below 64 (2^-19), well inside delta, so the one-pass walk classifies for both kernels.

Comparison -- ``compare``: on the non-fragile rows the project's MX-FP4 bars (O max-abs <= 2e-2,
relL2 <= 2e-3 from 64 rows on, |lse - ref| <= 1e-4 * max(1, max|ref|)); on every row O and lse
finite and O[d] inside [min, max] of the dequantised V column d over the row's visible keys, widened
by one fp16 ulp (O is a convex combination of those values); at most 2 % of the rows fragile.
"""
from __future__ import annotations

import functools

import torch

import mxfp4_masked_ref as MR
from oracle import mxfp4 as M

KINDS = ("randn", "ramp", "spikes", "fall")
RAMP_A = 40.0
DELTA = 2.0 ** -16
BOUNDARIES = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)
MAX_FRAGILE_SHARE = 0.02
O_MAXABS, O_RELL2, LSE_REL, RELL2_MIN_ROWS = 2e-2, 2e-3, 1e-4, 64


def n_visible(Sq, Sk, causal):
    return min(Sq, Sk) if int(causal) == 1 else Sk


def family(shape, kind, seed, causal=0):
    """(B, Hq, Hkv, Sq, Sk), one of KINDS, seed -> fp16 q [B,Hq,Sq,128], k, v [B,Hkv,Sk,128]."""
    assert kind in KINDS, kind
    B, H, Hkv, Sq, Sk = shape
    q, k, v = MR.randn_qkv(shape, seed=seed)
    if kind == "randn":
        return q, k, v
    g = torch.Generator().manual_seed(seed + 7919)
    q, k = q.float(), k.float()
    nv = n_visible(Sq, Sk, causal)
    if kind in ("ramp", "fall"):
        u = torch.randn(128, generator=g)
        u = u / u.norm()
        r = torch.linspace(0.0, RAMP_A, nv)
        r = torch.cat([r, r[-1:].expand(Sk - nv)])
        if kind == "fall":
            r = RAMP_A - r
        k = k + u * r[:, None]
        q = q + u * (8.0 * torch.rand((B, H, Sq, 1), generator=g))
    else:
        n = max(1, round(nv / 96))
        for b in range(B):
            for h in range(Hkv):
                k[b, h, torch.randperm(nv, generator=g)[:n]] *= 6.0
        q = q * torch.exp2(3.0 * torch.rand((B, H, Sq, 1), generator=g) - 1.0)
    return q.half(), k.half(), v


def walk(q, k, causal=0, delta=DELTA):
    """The one-pass restatement's tile loop over q and k alone (mxfp4_masked_ref.mxfp4_fwd_masked
    without V) -> dict: ``fragile`` bool [BH, Sq]; ``raised`` bool [tiles, BH, Sq], the restatement's
    own ``mx > m + 8`` per tile; ``late`` bool [tiles, BH, Sq], the raises of a row whose m was
    already finite (after its first visible tile)."""
    B, H, Sq, D = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
    BH = B * H
    qks = M.qk_scale(D)
    dq = M.deq_rows(*M.quant_rows(q.reshape(BH * Sq, D))).reshape(BH, Sq, D)
    dk = M.deq_rows(*M.quant_rows(k.reshape(B * Hkv * Sk, D))).reshape(B * Hkv, Sk, D)
    dk = dk[torch.arange(BH) // (H // Hkv)]
    vis_all = MR.visible_mask(int(causal), Sq, Sk)
    order = M.vt_key_order()
    m = torch.full((BH, Sq, 1), float("-inf"), dtype=torch.float64)
    fragile = torch.zeros((BH, Sq), dtype=torch.bool)
    raised, late = [], []
    for k0 in range(0, Sk, 64):
        vis = vis_all[None, :, k0:k0 + 64]
        acc = (dq @ dk[:, k0:k0 + 64].transpose(1, 2)).to(torch.float32)
        mx = (acc * qks).masked_fill(~vis, float("-inf")).amax(-1, keepdim=True).double()
        raise_ = mx > m + 8.0
        raised.append(raise_.squeeze(-1))
        late.append((raise_ & torch.isfinite(m)).squeeze(-1))
        m = torch.where(raise_, torch.ceil(mx), m)
        arg = (acc.double() * qks - m).to(torch.float32)
        P = torch.where(vis, torch.exp2(arg), torch.zeros_like(arg))[..., order]      # [BH, Sq, 2, 32]
        visb = vis.expand(1, Sq, 64)[..., order]
        y = P.double() / M.scale_value(M.e8m0(P.amax(-1)))[..., None]
        near = torch.zeros(y.shape, dtype=torch.bool)
        for b in BOUNDARIES:
            d = (y - b).abs()
            near = near | ((d > 0) & (d <= delta * b))
        near = near & visb
        amax_arg = arg.masked_fill(~vis, float("-inf"))[..., order].amax(-1).double()   # [BH, Sq, 2]
        fr = (amax_arg - amax_arg.round()).abs()
        byte = torch.isfinite(amax_arg) & (fr > 0) & (fr <= 2 * delta)
        fragile |= near.any(-1).any(-1) | byte.any(-1)
    return {"fragile": fragile, "raised": torch.stack(raised), "late": torch.stack(late)}


def fragile_rows(q, k, causal=0, delta=DELTA):
    """bool [BH, Sq]: the rows in which a P code or a P scale byte sits within delta of a rounding
    boundary (module docstring).  From the restatement alone."""
    return walk(q, k, causal, delta)["fragile"]


def raise_stats(w, rows_per_wave_group):
    """From walk(): (share of rows that raise late, number of (32-row wave x tile) pairs in which some
    but not all rows raise).  ``rows_per_wave_group``: the rows a kernel cuts into waves of 32 -- Sq for
    the one-pass kernel (one head), G * Sq for the key-split kernel (the virtual head)."""
    late, raised = w["late"], w["raised"]
    share = late.any(0).float().mean().item()
    nt = raised.shape[0]
    r = raised.reshape(nt, -1, rows_per_wave_group)
    pad = -rows_per_wave_group % 32
    real = torch.ones_like(r)
    if pad:
        r = torch.cat([r, torch.zeros(r.shape[:2] + (pad,), dtype=torch.bool)], -1)
        real = torch.cat([real, torch.zeros(real.shape[:2] + (pad,), dtype=torch.bool)], -1)
    n = r.reshape(nt, r.shape[1], -1, 32).sum(-1)
    nreal = real.reshape(nt, r.shape[1], -1, 32).sum(-1)
    return share, int(((n > 0) & (n < nreal)).sum())


def v_visible_minmax(vt, vs, BH, Sq, causal):
    """(lo, hi) float64 [BH, Sq, D]: min and max of the dequantised V column over the keys each query
    row sees (vt, vs: the restatement's quantised V operands)."""
    dv = M.deq_vt(vt, vs)
    BHkv, Sk, D = dv.shape
    kvh = torch.arange(BH) // (BH // BHkv)
    if not int(causal):
        lo, hi = dv.amin(1, keepdim=True).expand(-1, Sq, -1), dv.amax(1, keepdim=True).expand(-1, Sq, -1)
    else:
        last = (torch.arange(Sq) + MR.key_offset(int(causal), Sq, Sk)).clamp(max=Sk - 1)
        lo, hi = dv.cummin(1).values[:, last], dv.cummax(1).values[:, last]
    return lo[kvh], hi[kvh]


def fp16_ulp(x):
    """One fp16 step at the magnitude of x (float64), 2^-24 below the normal range."""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -14)))
    return torch.exp2(e - 10)


@functools.lru_cache(maxsize=None)
def case_inputs(shape, kind, seed, causal):
    """family(...) computed once per session; do not modify."""
    return family(shape, kind, seed, causal)


def reference(q, k, v, causal):
    """The one-pass restatement and what compare() needs -> dict(O, lse, ops, fragile, vminmax, walk)."""
    RO, Rl, rops = MR.mxfp4_fwd_masked(q, k, v, int(causal))
    w = walk(q, k, int(causal))
    BH, Sq = q.shape[0] * q.shape[1], q.shape[2]
    return {"O": RO, "lse": Rl, "ops": rops, "fragile": w["fragile"], "walk": w,
            "vminmax": v_visible_minmax(rops[4], rops[5], BH, Sq, causal)}


@functools.lru_cache(maxsize=None)
def case_reference(shape, kind, seed, causal):
    """reference() of case_inputs(), computed once per session; do not modify."""
    return reference(*case_inputs(shape, kind, seed, causal), causal)


def compare(O, lse, RO, Rl, fragile, V_deq_visible_minmax, name=""):
    """Kernel (O [B,H,Sq,D], lse [BH,Sq]) against the restatement (RO, Rl); module docstring.  Prints
    ``MXFP4-FUZZ <name> maxabs .. relL2 .. lse .. fragile n/N bit-equal ..`` and returns the figures."""
    BH, Sq = fragile.shape
    D = RO.shape[-1]
    O = O.detach().cpu().reshape(BH, Sq, D)
    lse = lse.detach().cpu().reshape(BH, Sq).float()
    RO, Rl = RO.reshape(BH, Sq, D), Rl.reshape(BH, Sq).float()
    ok = ~fragile
    nfr, N = int(fragile.sum()), BH * Sq
    Of, ROf = O.float()[ok], RO.float()[ok]
    err = (Of - ROf).abs().max().item() if ok.any() else 0.0
    rel = ((Of - ROf).norm() / ROf.norm().clamp_min(1e-30)).item() if ok.any() else 0.0
    lerr = (lse[ok] - Rl[ok]).abs().max().item() if ok.any() else 0.0
    lbar = LSE_REL * max(1.0, Rl.abs().max().item())
    biteq = torch.equal(O, RO)
    print(f"MXFP4-FUZZ {name} maxabs {err:.3e} relL2 {rel:.3e} lse {lerr:.3e} (bar {lbar:.1e}) "
          f"fragile {nfr}/{N} bit-equal {biteq}")
    assert torch.isfinite(O.float()).all() and torch.isfinite(lse).all(), name
    lo, hi = V_deq_visible_minmax
    Od = O.double()
    below, above = (lo - fp16_ulp(lo)) - Od, Od - (hi + fp16_ulp(hi))
    assert below.max().item() <= 0 and above.max().item() <= 0, (name, below.max().item(), above.max().item())
    assert nfr <= MAX_FRAGILE_SHARE * N, (name, nfr, N)
    assert err <= O_MAXABS, (name, err)
    if int(ok.sum()) >= RELL2_MIN_ROWS:
        assert rel <= O_RELL2, (name, rel)
    assert lerr <= lbar, (name, lerr, lbar)
    return {"maxabs": err, "relL2": rel, "lse": lerr, "fragile": nfr, "rows": N, "bit_equal": biteq}


def merge_lse2(O1, l1, O2, l2):
    """Merge two attention results over disjoint key sets by their base-2 lse, in fp32:
    O [.., rows, D] and lse [.., rows] -> (O fp32, lse fp32)."""
    O1, O2, l1, l2 = O1.float(), O2.float(), l1.float(), l2.float()
    mx = torch.maximum(l1, l2)
    w1, w2 = torch.exp2(l1 - mx), torch.exp2(l2 - mx)
    return (w1[..., None] * O1 + w2[..., None] * O2) / (w1 + w2)[..., None], mx + torch.log2(w1 + w2)


def exact_tail(q, k_tail, v_tail):
    """Exact fp32 attention of q [B,Hq,Sq,D] over a short fp16 tail [B,Hkv,n,D], every key visible ->
    (O fp32 [B,Hq,Sq,D], lse fp32 [B*Hq, Sq] base 2 of the scores q.k / sqrt(D))."""
    B, H, Sq, D = q.shape
    G = H // k_tail.shape[1]
    kk, vv = k_tail.float().repeat_interleave(G, 1), v_tail.float().repeat_interleave(G, 1)
    s = (q.float() @ kk.transpose(2, 3)) * M.qk_scale(D)
    mx = s.amax(-1, keepdim=True)
    p = torch.exp2(s - mx)
    l = p.sum(-1, keepdim=True)
    return (p @ vv) / l, (mx + torch.log2(l)).reshape(B * H, Sq)


# ------------------------------------------------------------------------------ the cases
# every entry: (shape (B, Hq, Hkv, Sq, Sk), kind, seed, causal).  The seeds are chosen so that the CPU
# conditions of tests/test_mxfp4_cases_ref.py hold in every case: top-left causal spikes at (1,2,2,384,384)
# reach 25 % late raises in few draws (rows in front of the first spike cannot raise; 0.05 to 0.27 over
# seeds 1..79)
SEEDS = {"ramp": 11, "spikes": 78, "fall": 11}
SEED = SEEDS["ramp"]
STRUCT_KINDS = ("ramp", "spikes", "fall")
ONEPASS_STRUCT = [(s, kind, SEEDS[kind], c) for kind in STRUCT_KINDS
                  for s, c in (((1, 4, 2, 160, 640), 0), ((1, 4, 2, 160, 640), 2), ((1, 2, 2, 384, 384), 1))]
# cached: (shape, kind, seed, causal 0 / 2) and the keys per split it runs with
CACHED_STRUCT = [((s, kind, SEEDS[kind], c), kpss) for kind in STRUCT_KINDS
                 for s, c, kpss in (((1, 4, 2, 33, 640), 0, (64, 192, 640)), ((1, 4, 2, 33, 640), 2, (64, 192, 640)),
                                    ((2, 8, 2, 1, 640), 0, (128,)))]
PLACEMENT_ONEPASS = [((B, H, Hkv, 320, 384), "ramp", SEED, c) for B, H, Hkv in ((2, 8, 2), (1, 9, 3))
                     for c in (0, 1, 2)]
PLACEMENT_CACHED = [((2, 8, 4, 100, 384), "ramp", SEED, c) for c in (0, 2)]
LONG_ONEPASS = [((1, 2, 1, 32, 8192), "ramp", SEED, c) for c in (0, 2)]
LONG_CACHED = [(((1, 8, 1, 1, 8192), "ramp", SEED, 0), (64, 1024, None))]
# tail merge: 256 cached tokens + 17 tail tokens, cut from one 320-key draw so the ramp runs on through
# the tail
TAIL_CASE = ((1, 4, 2, 8, 320), "ramp", SEED, 0)
TAIL_CACHE, TAIL_LEN = 256, 17

N_FUZZ = 16
FUZZ_BUDGET = 1 << 21     # B * Hq * Sq * Sk: about a second of CPU restatement
# 5000 + i + 100 j with the smallest j for which the CPU conditions of tests/test_mxfp4_cases_ref.py hold
# (fragile share, and for ramp / spikes the share of late raises); the seed draws shape and data
FUZZ_SEEDS = [5000, 5701, 5002, 5403, 5004, 5005, 5006, 5007, 5008, 5009, 5010, 5511, 5012, 5013, 5014, 5015]


def fuzz_case(i):
    """Seeded case i -> dict(shape, kind, seed, causal, smooth, cached, kps).  Cases 0..7 run the
    one-pass entry (Sq = 32 * {1..9}), 8..15 the cache (Sq in [1, 200], keys per split from {64, 128,
    192, Sk, None}).  The family rotates so that each occurs in both halves, smoothed (odd i) and not;
    ramp and spikes take Sk >= 256 (with fewer than four key tiles there is hardly a later tile to raise in)."""
    g = torch.Generator().manual_seed(FUZZ_SEEDS[i])
    pick = lambda xs: xs[int(torch.randint(len(xs), (1,), generator=g))]  # noqa: E731
    cached = i >= N_FUZZ // 2
    kind = KINDS[(i + i // 4) % 4]
    Sk = 64 * pick(list(range(4 if kind in ("ramp", "spikes") else 1, 25)))
    Sq = int(torch.randint(1, 201, (1,), generator=g)) if cached else 32 * pick(list(range(1, 10)))
    B, Hkv, G = 1, 1, 1
    for _ in range(16):
        b, hkv, grp = pick([1, 2, 3]), pick([1, 2, 3, 4, 8]), pick([1, 2, 4, 5])
        if b * hkv * grp * Sq * Sk <= FUZZ_BUDGET:
            B, Hkv, G = b, hkv, grp
            break
    if cached:
        causal = pick([0, 2] if Sq <= Sk else [0])
        kps = pick([64, 128, 192, Sk, None])
    else:
        causal = pick([0, 1, 2] if Sq <= Sk else [0, 1])
        kps = None
    smooth = bool(i % 2)
    return {"shape": (B, Hkv * G, Hkv, Sq, Sk), "kind": kind, "seed": FUZZ_SEEDS[i] + 1000, "causal": causal,
            "smooth": smooth, "cached": cached, "kps": kps}
