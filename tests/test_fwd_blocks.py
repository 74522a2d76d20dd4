"""What the lit value block (tests/fwd_blocks.py) sees in the int8 and bf16 forwards and today's
whole-tensor bars do not (CPU, oracle only; the GPU side is tests/test_gpu_fwd_blocks.py).

First the conditions the GPU test rests on, for every case it runs: at least 99 % of the lit heads'
O entries are normal fp16 numbers in the oracle, the dark head is exactly zero, the CPU restatement
of the forward's fast chain sits inside the band its bar was taken from, and the bars respect their
caps.

Then the table of planted faults (``FAULTS``).  Each is planted into a fake forward -- the oracle with
hooks, ``fwd_blocks.hooked_int8_fwd``, and the float64 merge ``fwd_blocks.split_merge_ref`` -- twice:

  * on randn inputs of 64 query rows and one head at 512, 4096 and 8192 keys (the benchmark's and the
    decode benchmark's lengths), read with today's bars: max|O - O_oracle| <= 1e-2, lse within 2 fp16
    ulp + 1e-3, and for the split faults |O_split - O_one_pass| <= 2e-3 at 1120 and 8288 keys;
  * on lit inputs at 1120 and 8192 keys, read with the instrument: a block past
    ``fwd_blocks.INT8_BLOCK_REL``, or lse past its bar.

Every fault must be caught by the blocks at both lengths.  ``FAULTS`` records which ones today's bars
let through; the figures measured here are max|dO| of the randn runs over the three tiles each fault
was planted on (today's bar is 1e-2), and the worst block of the lit runs (the bar is 0.0237):

  fault                        512 keys        4096 keys       8192 keys       lit block, 1120 / 8192 keys
  sv of the next tile          0.9-2.6e-2      0.06-1.7e-3     0.5-1.3e-3      1.00 / 1.00
  sk shifted from tile 32 on   (no tile 32)    5.3e-2          2.9e-2          0.94 / 0.72
  one tile's P.V dropped       1.4-1.6e-1      1.1-3.1e-2      5.5-6.4e-3      1.00 / 1.00
  one tile's sv doubled        1.4-1.6e-1      1.1-3.1e-2      5.5-6.4e-3      1.00 / 1.00
  a tile's 32 keys permuted    1.5-2.2e-1      1.2-4.2e-2      0.7-1.1e-2      0.68 / 1.23
  causal offset 32 keys off    8.8e-2          1.4e-2          3.6e-3          1.19 / 1.04
  25 % on one tile, one wave   2.4-3.7e-2      1.8-2.8e-3      1.1-1.5e-3      0.25 / 0.25

  (|O_split - O_one_pass|, bar 2e-3)           1120 keys / 256  8288 keys / 1024
  ragged split run over keys_per_split keys    1.1e-1           2.3e-2          0.12 / 0.23
  merge weights without l_s                    2.4e-1           1.1e-1          1.13 / 1.83
  merge weights against split 0's m            1.1              2.7e-1          141 / 36

So today's bars let through: a tile dequantised with its neighbour's sv at every length past 512
keys (randn tiles have nearly equal scales: only a ladder or a lit block tells one tile's scale from
the next); a 25 % error on one tile for one wave from 4096 keys on; a dropped or doubled tile and a
causal offset one tile off at 8192 keys, the decode benchmark's length (at the benchmark's 4096 keys
the tile faults fail by a tenth of the bar on two of three tiles, 1.1e-2 against 1e-2, and the
offset at 1.4e-2); a permuted tile
on two of three tiles at 8192 keys.  The shifted sk table and the three split faults are gross on
randn inputs too -- where a test has the shape for them: tests/test_gpu_fixup.py splits 1024 keys
into four equal splits, so no ragged split runs under its 2e-3.
"""
import pytest
import torch

import fwd_blocks as FB
import grad_blocks as GB

from oracle import restate as R

O_BAR = 1e-2          # tests/test_gpu_int8.py
SPLIT_BAR = 2e-3      # tests/test_gpu_fixup.py, kv_cache.attention_int8_cached


# ------------------------------------------------------------------------------ the conditions
def test_bars_respect_their_caps():
    assert FB.INT8_BLOCK_REL <= FB.INT8_CAP == 0.10
    assert FB.BF16_BLOCK_REL <= FB.BF16_CAP == GB.BF16_BLOCK_REL == pytest.approx(3e-2)


def test_cases_are_well_formed():
    tiles = set()
    for name, (shape, causal, lit, _) in FB.CASES.items():
        B, Hq, Hkv, Sq, Sk, D = shape
        assert B * Hkv == len(lit) and Hq % Hkv == 0 and Sq % 32 == 0 and Sk % 32 == 0
        assert all(t is None or 0 <= t < Sk // 32 for t in lit)
        FB.lit_list(name)
        if name in ("a", "b", "c"):
            assert B * Hkv == 6
            tiles |= {t for t in lit if t is not None}
    assert tiles == {0, 3, 4, 31, 32, 34}
    assert set(FB.INT8_RUNS) | set(FB.BF16_RUNS) == set(FB.CASES)


def test_lit_inputs_shape_of_v():
    shape, _, _, seed = FB.CASES["b"]
    lit, (db, dh) = FB.lit_list("b")
    q, k, v = FB.lit_inputs(shape, lit, seed, "int8", FB.V_EXP["b"])
    nz = (v != 0).any(-1)
    want = torch.zeros_like(nz)
    for b, h, t in lit:
        want[b, h, 32 * t:32 * t + 32] = True
    assert torch.equal(nz, want) and not nz[db, dh].any()
    for x in (q, k):   # the ladder: neighbouring 32-row blocks a factor of two or more apart
        n = x.reshape(*x.shape[:2], -1, 32 * x.shape[3]).norm(dim=-1)
        step = torch.maximum(n[..., 1:] / n[..., :-1], n[..., :-1] / n[..., 1:])
        assert step.min() > 1.5


@pytest.fixture(scope="module")
def int8_figures():
    """Per int8 run of the GPU test: the restatement's worst block against the oracle (whole run, then
    every split on its own)."""
    out = {}
    for name in FB.INT8_RUNS:
        q, k, v, ref = FB.int8_oracle(name)
        causal, off = bool(FB.CASES[name][1]), FB.causal_offset(name)
        O, lse = FB.restate_int8_fast(q, k, v, causal, off)
        fig = [FB.worst_block(O, ref[0])[0]]
        ok = [FB.lse_within_bar(lse, ref[1])[0]]
        FB.assert_dark_zero(name, O, "restate_int8_fast")
        if name in FB.KEYS_PER_SPLIT:
            for sl in FB.split_slices(k.shape[2], FB.KEYS_PER_SPLIT[name]):
                r = R.int8_fwd(q, k[:, :, sl], v[:, :, sl])
                o, m, l = FB.restate_int8_fast(q, k[:, :, sl], v[:, :, sl], state=True)
                fig.append(FB.worst_block(o, r[0])[0])
                ok.append(FB.lse_within_bar((m + torch.log2(l)).reshape(-1), r[1])[0])
        out[name] = (max(fig), all(ok))
        print(f"RELL2-BLOCK fwd-restate-int8-{name} {max(fig):.5f}")
    return out


@pytest.mark.parametrize("name", FB.INT8_RUNS)
def test_int8_input_conditions(name, int8_figures):
    """A condition on the inputs, not a measurement: the lit heads' O is made of normal fp16 numbers
    (a subnormal O would be compared at a few bits), and the dark head is exactly zero."""
    ref = FB.int8_oracle(name)[3]
    assert torch.isfinite(ref[0].float()).all()
    assert FB.normal_share(name, ref[0]) >= 0.99, (name, FB.normal_share(name, ref[0]))
    FB.assert_dark_zero(name, ref[0], "R.int8_fwd")
    fig, lse_ok = int8_figures[name]
    assert fig <= FB.INT8_BLOCK_REL / 3, (name, fig)
    assert lse_ok, name


def test_int8_restatement_band(int8_figures):
    worst = max(f for f, _ in int8_figures.values())
    assert 0.8 * FB.INT8_BLOCK_REL / 3 <= worst <= FB.INT8_BLOCK_REL / 3, worst


def test_int8_causal_rows_above_the_lit_tile_are_zero():
    """Queries above the lit tile read exactly zero there (int8 excludes masked keys: P = 0)."""
    for name in ("a1", "a2"):
        (B, Hq, Hkv, Sq, Sk, D) = FB.CASES[name][0]
        O = FB.int8_oracle(name)[3][0]
        G, off = Hq // Hkv, FB.causal_offset(name)
        for b, h, t in FB.lit_list(name)[0]:
            above = max(0, min(Sq, 32 * t - off))       # rows whose last kept key lies before the tile
            assert (O[b, h * G:(h + 1) * G, :above] == 0).all()
            assert (O[b, h * G:(h + 1) * G, above:] != 0).any(-1).all()


def test_bf16_conditions_and_band():
    """R.bf16_fwd(kt=16) against float64 attention on the blocks that attend the lit tile; the dark
    head exactly zero."""
    worst = 0.0
    for name in FB.BF16_RUNS:
        q, k, v, O, lse = FB.bf16_oracle(name)
        assert torch.isfinite(O).all() and torch.isfinite(lse).all()
        FB.assert_dark_zero(name, O, "R.bf16_fwd")
        To, _ = FB.bf16_truth(q, k, v, bool(FB.CASES[name][1]))
        rel = GB.block_rel(O, To)[FB.attending_blocks(name)].max().item()
        print(f"RELL2-BLOCK fwd-oracle-bf16-{name} {rel:.5f}")
        assert rel <= FB.BF16_BLOCK_REL / 3, (name, rel)
        worst = max(worst, rel)
    assert worst >= 0.8 * FB.BF16_BLOCK_REL / 3, worst


def test_hooks_leave_the_oracle_alone():
    q, k, v, ref = FB.int8_oracle("b2")
    O, lse = FB.hooked_int8_fwd(q, k, v, True, FB.causal_offset("b2"))
    assert torch.equal(O, ref[0]) and torch.equal(lse, ref[1])


def test_split_merge_ref_is_the_one_pass_forward():
    """The oracle's own state of each key slice, merged in float64, is the oracle's one-pass result
    within the block bar (the oracle's P_i8 of a tile depends on the running max it is rounded
    against, which a split starts afresh); weights taken against any common reference give the same merge."""
    q, k, v, ref = FB.int8_oracle("s1")
    rows, D = ref[0].numel() // 128, 128
    parts = [FB.hooked_int8_fwd(q, k[:, :, sl], v[:, :, sl], state=True)
             for sl in FB.split_slices(k.shape[2], FB.KEYS_PER_SPLIT["s1"])]
    opart = torch.stack([p[0].reshape(rows, D) for p in parts])
    ml = torch.stack([torch.stack([p[1].reshape(rows), p[2].reshape(rows)], -1) for p in parts])
    O, lse = FB.split_merge_ref(opart, ml)
    assert FB.worst_block(O.view_as(ref[0]), ref[0])[0] <= FB.INT8_BLOCK_REL
    assert FB.lse_within_bar(lse, ref[1])[0]
    shifted = ml.clone()
    shifted[..., 0] += 3.0
    O2, lse2 = FB.split_merge_ref(opart, shifted)
    assert torch.allclose(O2, O, rtol=1e-12, atol=0) and torch.allclose(lse2, lse + 3.0, rtol=1e-12)


def test_fp16_ulp():
    x = torch.tensor([1.0, 1.5, 2.0, 0.75, 2.0 ** -14, 2.0 ** -20, 0.0, -3.0], dtype=torch.float64)
    want = torch.tensor([2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -11, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 2.0 ** -9],
                        dtype=torch.float64)
    assert torch.equal(FB.fp16_ulp(x), want)


# ------------------------------------------------------------------------ the planted faults
OLD_LENGTHS = (512, 4096, 8192)
LIT_LENGTHS = (1120, 8192)
SPLIT_LENGTHS = ((1120, 256), (8288, 1024))      # (keys, keys per split): a ragged last split of 96 keys

# name: (whether today's bars notice it at each of OLD_LENGTHS, on every tile it is planted on; for the
# split faults at each of SPLIT_LENGTHS).  None: some tiles only, or within half the bar of it
# (printed, not asserted).
FAULTS = {
    "sv_next": (None, False, False),       # 512 keys: two of three tiles
    "sk_shift": (None, True, True),        # 512 keys have no tile 32
    "drop": (True, None, False),           # 4096 keys: 1.1e-2 against 1e-2 on two of three tiles
    "sv_double": (True, None, False),
    "perm": (True, True, None),            # 8192 keys: one of three tiles
    "offset": (True, None, False),         # 4096 keys: 1.4e-2
    "wave_scale": (True, False, False),
    "ragged": (True, True),
    "no_l": (True, True),
    "m_split0": (True, True),
}


def _randn(shape, seed):
    B, Hq, Hkv, Sq, Sk, D = shape
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((B, Hq, Sq, D), generator=g).half(), torch.randn((B, Hkv, Sk, D), generator=g).half(),
            torch.randn((B, Hkv, Sk, D), generator=g).half())


def _lit(shape, tile, seed):
    """One lit tile in the first key/value head (the others dark)."""
    q, k, v = FB.lit_inputs(shape, [(0, 0, tile)], seed, "int8", (8,))
    return q.half(), k.half(), v.half()


OLD_TILES = {512: (3, 7, 12), 4096: (31, 64, 126), 8192: (31, 128, 254)}


def _tile_fault(name, Sk, t):
    """(the fault, causal, offset) for tile ``t`` of a key run of Sk keys."""
    if name == "sk_shift":
        return ("sk_shift", 32), False, 0
    if name == "offset":                # a cache: query block 0 ends at tile (Sk - 64) / 32
        return ("offset", 0, 32), True, Sk - 64
    if name == "wave_scale":
        return ("wave_scale", t, 1, 1.25), False, 0
    return (name, t), False, 0


def _tiles(name, Sk, lit):
    """The tiles a fault is planted on (lit: the tile that is lit)."""
    if name == "sk_shift":              # the shifted part of the table; 512 keys have none
        return (33,) if Sk > 34 * 32 else ()
    if name == "offset":                # the diagonal tile of query block 0
        return ((Sk - 64) // 32,)
    return (32,) if lit else OLD_TILES[Sk]


def _noticed_today(O, lse, Oc, lsec):
    d = (O.float() - Oc.float()).abs().max().item()
    return d > O_BAR or not FB.lse_within_bar(lse, lsec)[0], d


def _caught_by_blocks(O, lse, Oc, lsec):
    w = FB.worst_block(O, Oc)[0]
    return w > FB.INT8_BLOCK_REL or not FB.lse_within_bar(lse, lsec)[0], w


@pytest.mark.parametrize("name", ["sv_next", "sk_shift", "drop", "sv_double", "perm", "offset", "wave_scale"])
def test_single_tile_faults(name):
    for i, Sk in enumerate(OLD_LENGTHS):
        q, k, v = _randn((1, 1, 1, 64, Sk, 128), 500 + i)
        seen = []
        for t in _tiles(name, Sk, lit=False):
            fault, causal, off = _tile_fault(name, Sk, t)
            clean = FB.hooked_int8_fwd(q, k, v, causal, off)
            noticed, d = _noticed_today(*FB.hooked_int8_fwd(q, k, v, causal, off, fault), *clean)
            seen.append(noticed)
            print(f"FAULT {name} randn {Sk} keys tile {t}: max|dO| {d:.2e} (max|O| "
                  f"{clean[0].float().abs().max():.3f}) {'noticed by' if noticed else 'passes'} today's bars")
        if FAULTS[name][i] is not None:
            assert seen and all(x == FAULTS[name][i] for x in seen), (name, Sk, seen)
    for i, Sk in enumerate(LIT_LENGTHS):
        for t in _tiles(name, Sk, lit=True):
            fault, causal, off = _tile_fault(name, Sk, t)
            q, k, v = _lit((1, 2, 2, 64, Sk, 128), t, 510 + i)
            clean = FB.hooked_int8_fwd(q, k, v, causal, off)
            assert FB.normal_share_of(clean[0][:, :1]) >= 0.99
            caught, w = _caught_by_blocks(*FB.hooked_int8_fwd(q, k, v, causal, off, fault), *clean)
            print(f"FAULT {name} lit {Sk} keys tile {t}: worst block {w:.3f}")
            assert caught and w > 0.2, (name, Sk, w)     # at its full relative size, whatever the length


def _split_run(q, k, v, ks, ragged=False, merge=None):
    """The key-split forward as the oracle's own state per key slice and the float64 merge, rounded
    as the merge kernel stores it.  ``ragged``: the last split of every key/value head runs over ks
    keys, into the rows that follow it in memory (the next head's, zeros after the last)."""
    B, Hkv, Sk, D = k.shape
    rows = q.numel() // D
    flat = [torch.cat([x.reshape(B * Hkv * Sk, D), torch.zeros((ks, D), dtype=x.dtype)]) for x in (k, v)]
    parts = []
    for sl in FB.split_slices(Sk, ks):
        kk, vv = k[:, :, sl], v[:, :, sl]
        if ragged and sl.stop - sl.start < ks:
            idx = (torch.arange(B * Hkv) * Sk)[:, None] + sl.start + torch.arange(ks)[None, :]
            kk, vv = (f[idx].view(B, Hkv, ks, D) for f in flat)
        parts.append(FB.hooked_int8_fwd(q, kk, vv, state=True))
    opart = torch.stack([p[0].reshape(rows, D) for p in parts])
    ml = torch.stack([torch.stack([p[1].reshape(rows), p[2].reshape(rows)], -1) for p in parts])
    O, lse = FB.split_merge_ref(opart, ml, merge)
    return O.float().half().view(q.shape), lse.float().half()


@pytest.mark.parametrize("name", ["ragged", "no_l", "m_split0"])
def test_split_and_merge_faults(name):
    kw = dict(ragged=True) if name == "ragged" else dict(merge=name)
    for i, (Sk, ks) in enumerate(SPLIT_LENGTHS):
        q, k, v = _randn((1, 2, 2, 64, Sk, 128), 520 + i)
        one = FB.hooked_int8_fwd(q, k, v)
        O, lse = _split_run(q, k, v, ks, **kw)
        d = (O.float() - one[0].float()).abs().max().item()
        noticed = d > SPLIT_BAR
        print(f"FAULT {name} randn {Sk} keys in splits of {ks}: |O_split - O_one| {d:.2e} "
              f"{'noticed' if noticed else 'passes'} today's 2e-3 (clean: "
              f"{(_split_run(q, k, v, ks)[0].float() - one[0].float()).abs().max():.1e})")
        if FAULTS[name][i] is not None:
            assert noticed == FAULTS[name][i], (name, Sk, d)
        # lit: a tile of the ragged split in head 0, head 1 dark
        q, k, v = _lit((1, 2, 2, 64, Sk, 128), Sk // 32 - 2, 530 + i)
        one = FB.hooked_int8_fwd(q, k, v)
        assert FB.worst_block(_split_run(q, k, v, ks)[0], one[0])[0] <= FB.INT8_BLOCK_REL
        caught, w = _caught_by_blocks(*_split_run(q, k, v, ks, **kw), *one)
        print(f"FAULT {name} lit {Sk} keys: worst block {w:.3f}")
        assert caught, (name, Sk, w)
