"""Key tile by key tile parity of the int8 and bf16 forwards on long key runs: the helper of
tests/test_fwd_blocks.py (CPU) and tests/test_gpu_fwd_blocks.py (GPU).

O is an average over the keys, so one 32-key tile's share of a row falls like 32 / Sk while a
whole-tensor bar on max|O - O_oracle| stays where it is: at 4096 keys a tile that is dropped, or
dequantised with twice its scale, moves O by about the 1e-2 of tests/test_gpu_int8.py, at 8192 keys by
less (tests/test_fwd_blocks.py has the figures).  The machinery that only long runs switch on -- the
fold of the KMAG bias every 32 tiles, the per-tile scale tables in LDS with their one-tile shift, the
four-slot ring in groups of four with a remainder, key splits with a ragged last split, the split
fixup, the merge weights, the bf16 forward's causal V-suffix sums -- is then held by nothing.

The instrument is a *lit value block*: V is zero outside one 32-key block of a key/value head, so
every O row of that head is the contribution of that one key tile alone, sum_k P_k v_k / l, while the
softmax weights and lse are what they would be for any V.  A wrong sp, sv, sk, key order, ring slot,
split boundary or merge weight for that tile shows at its full relative size whatever the length of
the key run.  q and k carry a ladder (grad_blocks.ladder: every 32-row block a multiplier of its own,
neighbours a factor of two or more apart), so a neighbouring tile's sk is a gross error in the tile's
P.  One launch lights a different tile in every key/value head but one, which stays dark: its O must
be exactly zero (a zero V block quantises to sv = 0 and indices 0, so its dequantisation factor
sp * sv is 0, the KMAG bias it carries is KMAG * 0, and the merge sums zeros; the bf16 forward adds
P . 0 and p * 0).  O is compared per 32-row query block with ``grad_blocks.block_rel``: no block left
out, no floor, a block the oracle has exactly zero must be exactly zero.

Bars.  int8: 3 x the worst block of ``restate_int8_fast`` -- the forward's fast chain restated on the
CPU -- against ``R.int8_fwd`` over every case the GPU test runs, every split on its own included;
bf16: 3 x the worst block of ``R.bf16_fwd(kt=16)`` against float64 softmax attention on the same
rounded inputs.  Neither comes from a GPU result.  lse keeps the elementwise bars of
tests/test_gpu_int8.py and tests/test_gpu_bf16.py.
"""
import math

import numpy as np
import torch

import grad_blocks as GB

from oracle import restate as R

BLOCK = GB.BLOCK
KMAG = 12582912.0          # common.h: 1.5 * 2^23, the bias of the int32 accumulators read as fp32
FWD_THR = 8.0              # int8_fwd_plan.h QA_FWD_THR
REBIAS = 32                # int8_attn_fwd.hip QA_FWD_REBIAS
F16_TINY = 2.0 ** -14      # the smallest normal fp16

# ---------------------------------------------------------------------------------------- bars
# int8: 3 x the worst 32-row block of restate_int8_fast against R.int8_fwd (the oracle) over INT8_RUNS
# (whole runs and every key split on its own), the 3 x of grad_blocks.py and jvp_blocks.py: room for
# the last bit of v_exp_f16 and for the waves redone with the reference's literal chain.  The constant
# is the measured figure rounded up by 3 to 7 %; tests/test_fwd_blocks.py holds the restatement
# between 0.8 of a third of it and that third.  Cap: no int8 bar above 0.10.
INT8_BLOCK_REL = 3 * 7.9e-3          # measured 7.68e-3 (case b2; splits alone 7.11e-3), against the oracle; cap 0.10
INT8_CAP = 0.10
# bf16: 3 x the worst 32-row block of R.bf16_fwd(kt=16) against float64 softmax attention on the same
# rounded inputs over BF16_RUNS.  Cap: grad_blocks.BF16_BLOCK_REL (3e-2).  With the multipliers
# GB.QK_BF16 = (0.4, 0.7, 1.0) the oracle alone sits at 0.050 (3 x = 0.15, past the cap): it rounds the
# scores and S qks - m to bf16, one step of which is 1.4 % of a P at |S qks - m| = 8, and a single
# tile has no other tiles to average that over.  So the lit bf16 inputs take the milder ladder
# QK_BF16_LIT below (logits a sixth as large), where the oracle measures 6.9e-3.
# Causal: a key at or above the query keeps the weight of the fill score, and the reference rounds
# fill - m (between -16 and -32) to bf16, whose step there is 2^-3: up to 4.4 % of that weight, the
# same for every masked key of a row.  Float64 attention cannot be held to that, so the figure is
# taken over the blocks that attend the lit tile (``attending_blocks``: the tile's own query block
# and those below it); the blocks that reach it through the fill alone sit 0.054 from float64
# attention and are held to the oracle on the GPU under the same bar.
QK_BF16_LIT = (0.1, 0.2, 0.4)
BF16_BLOCK_REL = 3 * 7.2e-3          # measured 6.87e-3 (case a), against float64 attention; cap 3e-2
BF16_CAP = GB.BF16_BLOCK_REL
BF16_LSE_ABS = 5e-3                  # tests/test_gpu_bf16.py


def lse_within_bar(lse, ref):
    """tests/test_gpu_int8.py: lse within 2 fp16 ulp of |lse_oracle| (+1e-3 abs), elementwise."""
    lerr = (lse.float().cpu() - ref.float().cpu()).abs()
    return bool((lerr <= 2 * 2.0 ** -10 * ref.float().cpu().abs() + 1e-3).all()), lerr.max().item()


# --------------------------------------------------------------------------------------- cases
# name: ((B, Hq, Hkv, Sq, Sk, D), causal, lit tiles in key/value-head order (None: the dark head), seed).
# causal 0: none; 1: the first query at the first key (the drop-in forwards); 2: the last query at the
# last key (a cache: offset Sk - Sq).
#
# Sk = 1120 keys are 35 tiles: the bias fold after tile 31, the four-slot ring wrapped eight times and
# three tiles left over after the groups of four.  Sq = 288 / 96 / 160 leave three, one and three of a
# workgroup's four waves idle in the last workgroup; B * Hkv = 6 with two or four query heads per
# key/value head or an odd head count.  Five heads are lit and one is dark, so the tiles 0, 3, 4 (the
# first group of four and the first of the next), 31, 32 (either side of the fold) and 34 (the last of
# the remainder) are spread over the three shapes, each at least twice.  Causal: the diagonal tile of
# a middle query block and the tile before it, and (causal 2) the tiles of the last query blocks.
_A = (1, 12, 6, 288, 1120, 128)
_B = (2, 12, 3, 96, 1120, 64)
_C = (2, 3, 3, 160, 1120, 128)
CASES = {
    "a": (_A, 0, (0, 4, 31, 32, 34, None), 401),
    "b": (_B, 0, (3, 31, None, 32, 34, 0), 402),
    "c": (_C, 0, (None, 34, 32, 4, 3, 31), 403),
    # top-left causal: only the tiles up to Sq / 32 are seen; block 4 of 9 (diagonal 4, before it 3),
    # block 1 of 3, block 2 of 5
    "a1": (_A, 1, (0, None, 3, 4, 5, 8), 404),
    "b1": (_B, 1, (1, 0, 2, None, 1, 2), 405),
    "c1": (_C, 1, (2, 1, 0, 4, 3, None), 406),
    # bottom-right causal: query block b ends at tile (Sk - Sq) / 32 + b; Sq = 288: block 4 has the
    # diagonal tile 30; Sq = 96: blocks 0..2 have 32, 33, 34
    "a2": (_A, 2, (0, 29, None, 30, 32, 34), 407),
    "b2": (_B, 2, (3, 31, 32, 33, None, 34), 408),
    # the key-split pair called directly: 256 keys per split are four full splits and one of 96 keys
    # (the first tile of split 1, the last of split 2, one of the ragged split, the last of split 3);
    # 1056 keys per split of 2144 fold the bias inside a split and leave a last split of one tile
    "s1": ((1, 12, 6, 96, 1120, 128), 0, (8, 23, 33, None, 0, 31), 409),
    "s2": ((2, 6, 3, 32, 2144, 128), 0, (31, 32, None, 33, 65, 66), 410),
    # the smallest cache that kv_cache._split_plan splits (two splits of 1024 keys)
    "p": ((2, 6, 3, 96, 2048, 128), 0, (0, 31, 32, None, 63, 40), 411),
    # a smoothed cache: 544 keys quantised with their mean, 576 appended against it
    "sm": ((1, 6, 3, 96, 1120, 128), 0, (16, None, 34), 412),
    # bf16 causal: masked keys keep the weight of the fill value (bf16_fwd.hip), so every tile reaches
    # every row: the diagonal tile of a middle block (half in the tile loop, half in the V suffix),
    # the tile before it, and tiles only the suffix sums hold
    "a1f": (_A, 1, (3, 4, 5, None, 31, 34), 413),
    "b1f": (_B, 1, (0, 1, 2, 32, 34, None), 414),
    "c1f": (_C, 1, (None, 1, 2, 4, 33, 3), 415),
}
KEYS_PER_SPLIT = {"s1": 256, "s2": 1056, "p": 1024}
SMOOTH_HEAD = 544          # keys of case "sm" the cache is created from

# every int8 run of tests/test_gpu_fwd_blocks.py (the split cases also split by split)
INT8_RUNS = ("a", "b", "c", "a1", "b1", "c1", "a2", "b2", "s1", "s2", "p", "sm")
BF16_RUNS = ("a", "b", "c", "a1f", "b1f", "c1f")

# log2 of the power of two each lit block is scaled by (lit_inputs): found once so that at least 99 %
# of the lit heads' O entries are normal fp16 numbers in the oracle and none overflows;
# tests/test_fwd_blocks.py asserts the share.  (bf16 returns fp32: no scale.)
V_EXP = {"a": (9, 9, 10, 10, 4), "b": (3, 4, 3, 9, 2), "c": (6, 9, 9, 10, 3), "a1": (4, 4, -1, 7, 1),
         "b1": (0, -3, 0, 7, 0), "c1": (-2, 0, 0, 1, 2), "a2": (9, 10, 3, 10, 12), "b2": (10, 8, 7, 7, 5),
         "s1": (10, 7, 5, 3, 4), "s2": (4, 2, 11, 3, 2), "p": (8, 11, 11, 8, 5), "sm": (7, 9)}


def lit_list(name):
    """[(batch entry, key/value head, key tile)] of a case, and its dark (batch entry, head)."""
    (B, Hq, Hkv, Sq, Sk, D), _, tiles, _ = CASES[name]
    assert len(tiles) == B * Hkv and tiles.count(None) == 1
    lit = [(i // Hkv, i % Hkv, t) for i, t in enumerate(tiles) if t is not None]
    dark = tiles.index(None)
    return lit, (dark // Hkv, dark % Hkv)


def causal_offset(name):
    (B, Hq, Hkv, Sq, Sk, D), causal = CASES[name][:2]
    return Sk - Sq if causal == 2 else 0


def lit_inputs(shape, lit, seed, path, v_exp=None):
    """fp32 (q, k, v): q and k randn times a ``grad_blocks.ladder`` per 32-row block (GB.QK_INT8 for
    ``path`` "int8", QK_BF16_LIT for "bf16"); v zero except for one randn 32-key block per
    (batch entry, key/value head, key tile) of ``lit``, times 2 ** v_exp[i].  The caller casts."""
    B, Hq, Hkv, Sq, Sk, D = shape
    assert len({(b, h) for b, h, _ in lit}) == len(lit), "at most one lit tile per key/value head"
    g = torch.Generator().manual_seed(seed)
    choices = GB.QK_INT8 if path == "int8" else QK_BF16_LIT
    q = torch.randn((B, Hq, Sq, D), generator=g) * GB.ladder(B, Hq, Sq, choices, g)
    k = torch.randn((B, Hkv, Sk, D), generator=g) * GB.ladder(B, Hkv, Sk, choices, g)
    v = torch.zeros((B, Hkv, Sk, D))
    for i, (b, h, t) in enumerate(lit):
        blk = torch.randn((BLOCK, D), generator=g)
        v[b, h, BLOCK * t:BLOCK * t + BLOCK] = blk * 2.0 ** (0 if v_exp is None else v_exp[i])
    return q, k, v


def case_inputs(name, path="int8"):
    """(q, k, v) of a case in the path's dtypes."""
    shape, _, _, seed = CASES[name]
    lit, _ = lit_list(name)
    q, k, v = lit_inputs(shape, lit, seed, path, V_EXP.get(name) if path == "int8" else None)
    return q.half(), k.half(), (v.half() if path == "int8" else v.bfloat16())


def smooth_shift(k, k_mean=None):
    """Keys minus the mean a smoothed cache stores (R.k_smooth on the first SMOOTH_HEAD keys when
    ``k_mean`` is not given), rounded to fp16 as the quantiser reads them."""
    if k_mean is None:
        k_mean = R._h(R._f(k[:, :, :SMOOTH_HEAD]).mean(dim=-2, keepdim=True))
    return R._h(R._f(k) - R._f(k_mean))


_ORACLE = {}


def int8_oracle(name):
    """(q, k, v, R.int8_fwd's tuple) of a case, computed once per process and shared (nobody writes to
    it); case "sm" on the keys minus the CPU's mean of the first SMOOTH_HEAD."""
    if name not in _ORACLE:
        q, k, v = case_inputs(name)
        if name == "sm":
            k = smooth_shift(k)
        ref = R.int8_fwd(q, k, v, causal=bool(CASES[name][1]), causal_offset=causal_offset(name))
        _ORACLE[name] = (q, k, v, ref)
    return _ORACLE[name]


def bf16_oracle(name):
    """(q, k, v, O, lse) of R.bf16_fwd(kt=16) on a case, computed once per process."""
    key = ("bf16", name)
    if key not in _ORACLE:
        q, k, v = case_inputs(name, "bf16")
        _ORACLE[key] = (q, k, v) + tuple(R.bf16_fwd(q, k, v, bool(CASES[name][1]), kt=16))
    return _ORACLE[key]


def lit_rows(name, O):
    """The rows [n, Sq, D] of O [B, Hq, Sq, D] that belong to lit key/value heads."""
    (B, Hq, Hkv, Sq, Sk, D) = CASES[name][0]
    G = Hq // Hkv
    lit, _ = lit_list(name)
    return torch.cat([O[b, h * G:(h + 1) * G] for b, h, _ in lit])


def normal_share(name, O):
    """Share of the lit heads' O entries that are normal fp16 numbers (a causal case: of the entries
    the oracle does not have exactly zero, which the mask puts above the lit tile)."""
    return normal_share_of(lit_rows(name, O))


def normal_share_of(O):
    x = O.float().abs()
    x = x[x != 0]
    return (x >= F16_TINY).float().mean().item()


def assert_dark_zero(name, O, who):
    (B, Hq, Hkv, Sq, Sk, D) = CASES[name][0]
    G = Hq // Hkv
    _, (b, h) = lit_list(name)
    x = O.detach().cpu()[b, h * G:(h + 1) * G]
    assert (x == 0).all(), (who, name, "the dark head is not exactly zero", int((x != 0).sum()))
    assert all((lit_rows(name, O.detach().cpu()) != 0).any(-1).any(-1)), (who, name, "a lit head is empty")


def worst_block(a, ref):
    """(worst per-block relL2, (b, h, s / 32) of it)."""
    rel = GB.block_rel(a, ref)
    return rel.max().item(), tuple(int(i) for i in (rel == rel.max()).nonzero()[0])


# ---------------------------------------------------------------------- the int8 forward's fast chain
def _exp2_f16(d):
    """exp2 of fp16 arguments, correctly rounded to fp16 (float64 exp2 rounded once: numpy converts
    float64 to float16 directly, torch goes through float32)."""
    return torch.from_numpy(np.exp2(d.double().numpy()).astype(np.float16))


def _exp2_f32(x):
    return torch.exp2(x.double()).float()


def _clear_last_bit(c):
    """common.h kmag_scale: the last significand bit cleared, so that KMAG * c is exact."""
    return (c.contiguous().view(torch.int32) & ~1).view(torch.float32)


# the keys of a 32-key tile that lane half h sums, in the order of the packed f16 tree of sm2:
# register r of half h holds key (r & 3) + 8 (r >> 2) + 4 h; pair j is registers 2j, 2j + 1
_LO = torch.tensor([(2 * j & 3) + 8 * (2 * j >> 2) for j in range(8)])


def _half_sum(e, h):
    """sm2's row sum of lane half ``h``: packed f16 adds as ((e0+e1)+(e2+e3))+((e4+e5)+(e6+e7)), then
    the two halves of the pair in fp32 (pk_hsum)."""
    out = []
    for idx in (_LO + 4 * h, _LO + 4 * h + 1):
        x = e[..., idx]
        s = ((x[..., 0] + x[..., 1]) + (x[..., 2] + x[..., 3])) + ((x[..., 4] + x[..., 5]) + (x[..., 6] + x[..., 7]))
        out.append(s.float())
    return out[0] + out[1]


def restate_int8_fast(q, k, v, causal=False, causal_offset=0, state=False):
    """The int8 forward's fast chain (csrc/int8_attn_fwd.hip) on the CPU ->
    (O fp16 [B,H,S,D], lse fp16 [B*H*S]); ``state``: (Ô = fp16(O / l), m fp32, l fp32) as a key split
    writes them.  The quantised operands are the oracle's (bit-exact on the GPU too).  Per 32-row wave
    and 32-key tile:

      * S = f16(f32(X c)), c = sq * (sk * qks) with its last bit cleared (kmag_scale), one fma on the
        biased accumulator (:480-485); rm = the row max; d = f16(S - rm) (:494), -inf on a masked key;
      * the deferred running max: when some row of the wave has rm > f16(m + 8), every row takes
        m = max(m, rm) and l, O, the bias sum and the pending P.V factor are scaled by
        exp2(f16(m_old - m)) (:503-516);
      * er = exp2(f16(rm - m)), the tile's factor cpv = er * (sv / 127) (:517-518);
      * e = exp2_f16(d) correctly rounded where the GPU has v_exp_f16; l += er * sum e, the sum in
        packed f16 per lane half (:573-576); P_i8 = trunc(127 e) (p_index8);
      * O += (KMAG + X) * cpv in one fma per element after the next tile's SM1 (:626-627), and the
        bias KMAG * sum cpv folded out every 32 tiles (:435-446) and in the epilogue's fma (:721);
      * lse = f16(m + f16(log2 l)), O = f16(fma(O, 1 / l, -KMAG obias / l)).

    Left out: the deferred votes and the literal chain of the waves they mark (closer to the oracle).
    """
    B, H, S, D = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
    G, BH, nw = H // Hkv, B * H, S // BLOCK
    f32 = torch.float32
    qks = torch.tensor(R.qk_scale(D), dtype=f32)
    qi, sq = R.quant_blocks(q.reshape(BH, S, D))
    ki, sk = R.quant_blocks(k.reshape(B * Hkv, Sk, D))
    vi, sv = R.quant_blocks(v.reshape(B * Hkv, Sk, D))
    kvh = torch.arange(BH) // G
    ki, sk, vi, sv = ki[kvh].double(), sk[kvh], vi[kvh].double(), sv[kvh]
    qd = qi.double()
    cq = sq.float().repeat_interleave(BLOCK, dim=1)                     # [BH, S]
    ck = sk.float() * qks                                               # [BH, tiles]
    svq = sv.float() * torch.tensor(1.0 / 127.0, dtype=f32)
    ninf = float("-inf")
    m = torch.full((BH, S), ninf, dtype=torch.float16)
    m_thr = m.clone()
    l = torch.zeros((BH, S, 2), dtype=f32)
    O = torch.zeros((BH, S, D), dtype=f32)
    obias = torch.zeros((BH, S), dtype=f32)
    rows = torch.arange(S)

    def sm1(t):
        nonlocal m, m_thr, l, O, obias, pend
        ks = slice(BLOCK * t, BLOCK * t + BLOCK)
        X = qd @ ki[:, ks].transpose(1, 2)
        c = _clear_last_bit(cq * ck[:, t, None])
        S16 = (X * c[..., None].double()).float().half()
        if causal:
            keep = (torch.arange(ks.start, ks.stop)[None, :] <= rows[:, None] + causal_offset)[None]
            # (a row that keeps no key of the tile: the max of INT_MIN patterns reads -0.0, rm = f16(-KMAG c))
            none = (-KMAG * c.double()).float().half()
            rm = torch.where(keep, S16, torch.full_like(S16, ninf)).amax(-1)
            rm = torch.where(torch.isinf(rm), none, rm)
        else:
            rm = S16.amax(-1)
        d = S16 - rm[..., None]
        if causal:
            d = torch.where(keep, d, torch.full_like(d, ninf))
        move = (rm > m_thr).reshape(BH, nw, BLOCK).any(-1).repeat_interleave(BLOCK, dim=1)
        nm = torch.where(move, torch.maximum(m, rm), m)
        r = torch.where(move, _exp2_f32((m - nm).float()), torch.ones((), dtype=f32))
        r = torch.where(torch.isnan(r), torch.ones((), dtype=f32), r)   # (-inf) - (-inf) cannot happen: rm is finite
        m = nm
        m_thr = torch.where(move, m + torch.tensor(FWD_THR, dtype=torch.float16), m_thr)
        l, O, obias = l * r[..., None], O * r[..., None], obias * r
        if pend is not None:
            pend = pend * r
        er = _exp2_f32((rm - m).float())
        return d, er, er * svq[:, t, None]

    pend = None
    d, er, cpv = sm1(0)
    nt = Sk // BLOCK
    for t in range(nt):
        e = _exp2_f16(d)
        for h in (0, 1):
            l[..., h] = (_half_sum(e, h).double() * er.double() + l[..., h].double()).float()
        Pi = torch.trunc(e.double() * 127.0)
        X = Pi @ vi[:, BLOCK * t:BLOCK * t + BLOCK]
        pend = cpv
        if t + 1 < nt:
            d, er, cpv = sm1(t + 1)
        O = ((KMAG + X) * pend[..., None].double() + O.double()).float()
        obias = obias + pend
        if (t + 1) % REBIAS == 0:
            O = (O.double() - KMAG * obias[..., None].double()).float()
            obias = torch.zeros_like(obias)
    lt = l[..., 0] + l[..., 1]
    inv = 1.0 / lt
    add = (-KMAG * obias).float() * inv
    Oh = (O.double() * inv[..., None].double() + add[..., None].double()).float().half()
    if state:
        return Oh.view(B, H, S, D), m.float().view(B, H, S), lt.view(B, H, S)
    lse = (m.float() + torch.log2(lt.double()).float().half().float()).half()
    return Oh.view(B, H, S, D), lse.reshape(-1)


# ------------------------------------------------------------- the oracle with hooks (a fake forward)
def hooked_int8_fwd(q, k, v, causal=False, causal_offset=0, fault=None, state=False):
    """``R.int8_fwd`` with one planted mistake (tests/test_fwd_blocks.py; without one it returns the
    oracle's bits) -> (O fp16 [B,H,S,D], lse fp16 [B*H*S]); ``state``: (Ô fp16, m, l) of the key run as
    a split would hand them to the merge.  ``fault`` is (name, tile, ...):

      ("sv_next", t)        tile t dequantised with tile t + 1's sv
      ("sv_double", t)      tile t's sv doubled
      ("sk_shift", t0)      the sk table shifted by one tile from tile t0 on
      ("drop", t)           tile t's P.V left out
      ("perm", t)           the 32 keys of tile t reversed in the P.V operand
      ("offset", w, n)      the causal offset n keys off for the 32-row query block w
      ("wave_scale", t, w, f)  tile t's product scaled by f for the 32-row query block w only
    """
    B, H, S, D = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
    G, BH = H // Hkv, B * H
    name = fault[0] if fault else None
    qks = R.qk_scale(D)
    _f, _h, _exp2 = R._f, R._h, R._exp2
    qi, sq = R.quant_blocks(q.reshape(BH, S, D))
    ki_kv, sk_kv = R.quant_blocks(k.reshape(B * Hkv, Sk, D))
    vi_kv, sv_kv = R.quant_blocks(v.reshape(B * Hkv, Sk, D))
    kvh = torch.arange(BH) // G
    ki, sk, vi, sv = ki_kv[kvh], sk_kv[kvh], vi_kv[kvh], sv_kv[kvh]
    nt = Sk // BLOCK
    O = torch.zeros((BH, S, D), dtype=torch.float32)
    l = torch.ones((BH, S, 1), dtype=torch.float32)
    m = torch.full((BH, S, 1), float("-inf"), dtype=torch.float16)
    qd = qi.double()
    sqf = _f(sq).repeat_interleave(BLOCK, dim=1)[..., None]
    off = torch.full((S,), causal_offset)
    if name == "offset":
        off[BLOCK * fault[1]:BLOCK * fault[1] + BLOCK] += fault[2]
    for t in range(nt):
        k0, k1 = t * BLOCK, (t + 1) * BLOCK
        tk = min(t + 1, nt - 1) if name == "sk_shift" and t >= fault[1] else t
        acc = _f(qd @ ki[:, k0:k1].double().transpose(1, 2))
        S16 = _h(((acc * sqf) * _f(sk[:, tk])[:, None, None]) * qks)
        if causal:
            keep = torch.arange(k0, k1)[None, :] <= torch.arange(S)[:, None] + off[:, None]
            S16 = torch.where(keep[None], S16, torch.full_like(S16, float("-inf")))
        rm = S16.amax(-1, keepdim=True)
        nm = torch.maximum(m, rm)
        P = _exp2(_h(_f(S16) - _f(nm)))
        lt = P.sum(-1, keepdim=True)
        r = _exp2(_h(_f(m) - _f(nm)))
        m = nm
        l = l * r + lt
        O = O * r
        sp = _exp2(_h(_f(rm) - _f(m))) / 127
        Pi = torch.where(sp > 0, torch.trunc(P / torch.where(sp > 0, sp, 1.0)), 0.0)
        vt = vi[:, k0:k1].double()
        if name == "perm" and t == fault[1]:
            vt = vt.flip(1)
        pv = _f(Pi.double() @ vt)
        tv = min(t + 1, nt - 1) if name == "sv_next" and t == fault[1] else t
        add = (pv * sp) * _f(sv[:, tv])[:, None, None]
        if name == "sv_double" and t == fault[1]:
            add = add * 2
        if name == "drop" and t == fault[1]:
            add = add * 0
        if name == "wave_scale" and t == fault[1]:
            w = fault[2]
            add[:, BLOCK * w:BLOCK * w + BLOCK] *= fault[3]
        O = O + add
    Oh = _h(O / l).view(B, H, S, D)
    if state:
        return Oh, _f(m).view(B, H, S), l.view(B, H, S)
    lse = _h(_f(m.squeeze(-1)) + _f(_h(torch.log2(l).squeeze(-1))))
    return Oh, lse.reshape(-1)


# --------------------------------------------------------------------------- key splits and their merge
def split_slices(Sk, keys_per_split):
    return [slice(k0, min(k0 + keys_per_split, Sk)) for k0 in range(0, Sk, keys_per_split)]


def split_merge_ref(opart, ml, fault=None):
    """The merge of the key splits in float64.  opart [nsplit, rows, D] (the splits' normalised
    outputs Ô_s), ml [nsplit, rows, 2] = {m_s, l_s} -> (O [rows, D], lse [rows]):
    M = max_s m_s, w_s = 2^(m_s - M) l_s, O = sum_s w_s Ô_s / sum_s w_s, lse = M + log2 sum_s w_s.
    ``fault`` (tests/test_fwd_blocks.py): "no_l" weighs by 2^(m_s - M) alone; "m_split0" takes the
    weights against split 0's m and keeps the normaliser and lse against M (taken consistently, the
    reference point of the weights cancels: that merge is the same merge)."""
    o, m, l = opart.double(), ml[..., 0].double(), ml[..., 1].double()
    M = m.amax(0)
    w = torch.exp2(m - M) * (1.0 if fault == "no_l" else l)
    L = w.sum(0)
    wo = torch.exp2(m - m[0]) * l if fault == "m_split0" else w
    return (wo[..., None] * o).sum(0) / L[..., None], M + torch.log2(L)


def merge_rounding(opart, ml):
    """What the merge kernel's fp32 arithmetic can lose, in float64: (sum_s |w_s Ô_s| / sum_s w_s
    [rows, D], the size of the terms the fp32 sum of O rounds at; log2 sum_s w_s [rows], the size the
    inner f16(log2 L) of lse rounds at; M [rows])."""
    o, m, l = opart.double(), ml[..., 0].double(), ml[..., 1].double()
    M = m.amax(0)
    w = torch.exp2(m - M) * l
    L = w.sum(0)
    return (w[..., None] * o.abs()).sum(0) / L[..., None], torch.log2(L), M


def fp16_ulp(x):
    """The spacing of fp16 numbers at |x| (float64 tensor), the subnormal spacing below 2^-14."""
    e = torch.floor(torch.log2(x.abs().clamp_min(F16_TINY)))
    return torch.exp2(e - 10)


def merge_inputs(nsplit, rows, D, seed):
    """Synthetic split states: Ô_s randn fp16, m_s spread over +-30 (some weights underflow to 0
    against the row's largest), l_s in [1, 1000]."""
    g = torch.Generator().manual_seed(seed)
    opart = torch.randn((nsplit, rows, D), generator=g).half()
    m = (torch.rand((nsplit, rows), generator=g) * 60 - 30).float()
    l = torch.exp2(torch.rand((nsplit, rows), generator=g) * math.log2(1000.0)).float()
    return opart, torch.stack([m, l], -1).contiguous()


# ----------------------------------------------------------------------------------------- bf16
def bf16_truth(q, k, v, causal):
    """float64 softmax attention on the same rounded inputs, with the reference's causal rule (keys at
    or above the query keep the fill score -126 before the scale, bf16_fwd.hip:7) ->
    (O [B,H,S,D], lse in log2 units [B*H, S])."""
    B, H, S, D = q.shape
    G = H // k.shape[1]
    qd = q.double()
    kd, vd = (x.double().repeat_interleave(G, dim=1) for x in (k, v))
    s = qd @ kd.transpose(-1, -2)
    if causal:
        keep = (torch.arange(S)[:, None] - torch.arange(k.shape[2])[None, :]) > 0
        s = torch.where(keep, s, torch.full_like(s, -126.0))
    s = s * float(torch.tensor(R.qk_scale(D), dtype=torch.float32))
    lse = torch.logsumexp(s * math.log(2.0), -1) / math.log(2.0)
    return torch.exp2(s - lse[..., None]) @ vd, lse.reshape(B * H, S)


def attending_blocks(name):
    """[B, Hq, Sq / 32] bool: the query blocks of a top-left causal case that keep a key of their
    head's lit tile (its own block and those below); every block of a non-causal case."""
    (B, Hq, Hkv, Sq, Sk, D), causal = CASES[name][:2]
    G = Hq // Hkv
    seen = torch.full((B, Hq, Sq // BLOCK), not causal)
    if causal:
        for b, h, t in lit_list(name)[0]:
            seen[b, h * G:(h + 1) * G, t:] = True
    return seen
