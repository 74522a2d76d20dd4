"""CPU tests of tests/mxfp4_cases.py, the inputs and the comparison of tests/test_gpu_mxfp4_fuzz.py.
No kernel runs here: everything below is a statement about the restatements
(tests/mxfp4_masked_ref.py, tests/mxfp4_split_ref.py) on the inputs the GPU tests use --

  * ramp and spikes raise the integer running max after a row's first visible tile in >= 25 % of the
    rows, and in at least one (32-row wave x tile) pair only some rows raise, counted with the
    restatement's own ``mx > m + 8``: the GPU tests do run the rescale branch, partially too;
  * at most 2 % of a case's rows are fragile (sit within delta = 2^-16 of a rounding boundary);
  * the split restatement equals the one-pass restatement at the bars of tests/test_mxfp4_cache_ref.py
    (O bit-equal, lse <= 1e-6), on every family, at the splits the GPU tests use;
  * how far the MX-FP4 definition is from exact attention on such peaked inputs (pinned below: a
    number of the definition, not of the kernel).

A smoothed fuzz case is smoothed here with the CPU's fp16 token mean; the GPU test takes the GPU's.
"""
import pytest
import torch

import mxfp4_cases as C
import mxfp4_masked_ref as MR
import mxfp4_split_ref as SR
from quantizedattention_amd.kv_cache_mxfp4 import _split_plan_fp4


def _fuzz_entries():
    out = []
    for i in range(C.N_FUZZ):
        f = C.fuzz_case(i)
        out.append((f"fuzz{i}", (f["shape"], f["kind"], f["seed"], f["causal"]), f["smooth"], f["cached"],
                    (f["kps"],) if f["cached"] else ()))
    return out


# (id, (shape, kind, seed, causal), smoothed, cached, keys per split the GPU tests run)
ENTRIES = ([("struct", c, False, False, ()) for c in C.ONEPASS_STRUCT]
           + [("struct-cached", c, False, True, kpss) for c, kpss in C.CACHED_STRUCT]
           + [("placement", c, False, False, ()) for c in C.PLACEMENT_ONEPASS]
           + [("placement-cached", c, False, True, (128,)) for c in C.PLACEMENT_CACHED]
           + [("long", c, False, False, ()) for c in C.LONG_ONEPASS]
           + [("long-cached", c, False, True, kpss) for c, kpss in C.LONG_CACHED]
           + [("tail", C.TAIL_CASE, False, True, ())]
           + _fuzz_entries())
IDS = [f"{e[0]}-{e[1][1]}-{'x'.join(map(str, e[1][0]))}-c{e[1][3]}" for e in ENTRIES]


def _inputs(case, smooth):
    q, k, v = C.case_inputs(*case)
    return (q, MR.smooth_fp16(k), v) if smooth else (q, k, v)


def test_families():
    shape = (2, 4, 2, 96, 256)
    r = MR.randn_qkv(shape, seed=5)
    for kind in C.KINDS:
        q, k, v = C.family(shape, kind, 5)
        assert q.shape == (2, 4, 96, 128) and k.shape == v.shape == (2, 2, 256, 128)
        assert q.dtype == k.dtype == v.dtype == torch.float16
        assert torch.isfinite(q.float()).all() and torch.isfinite(k.float()).all()
        assert torch.equal(v, r[2])                                # v ~ N(0, 1) in every family
        assert torch.equal(q, r[0]) == (kind == "randn") and torch.equal(k, r[1]) == (kind == "randn")
    # the ramp spans the keys the queries see: top-left with Sq < Sk stops climbing at key Sq
    _, k1, _ = C.family((1, 1, 1, 64, 256), "ramp", 5, causal=1)
    _, k0, _ = C.family((1, 1, 1, 64, 256), "ramp", 5, causal=0)
    _, kr, _ = C.family((1, 1, 1, 64, 256), "randn", 5)
    d1, d0 = (k1.float() - kr.float()).norm(dim=-1)[0, 0], (k0.float() - kr.float()).norm(dim=-1)[0, 0]
    assert abs(d1[63].item() - C.RAMP_A) < 0.1 and abs(d1[255].item() - C.RAMP_A) < 0.1
    assert abs(d0[255].item() - C.RAMP_A) < 0.1 and d0[63].item() < C.RAMP_A / 3
    _, kf, _ = C.family((1, 1, 1, 64, 256), "fall", 5)
    df = (kf.float() - kr.float()).norm(dim=-1)[0, 0]
    assert abs(df[0].item() - C.RAMP_A) < 0.1 and df[255].item() < 0.05


def test_classifier_scales_with_delta_and_spares_exact_ties():
    q, k, _ = C.family((1, 2, 2, 64, 256), "randn", 3)
    assert not C.fragile_rows(q, k, 0, 0.0).any()                  # 0 < |y - b| <= 0 never holds
    f16, f10, f4 = (C.fragile_rows(q, k, 0, 2.0 ** -e) for e in (16, 10, 4))
    assert (f16 <= f10).all() and (f10 <= f4).all() and f4.all() and int(f10.sum()) > int(f16.sum())
    # k = 0: S = 0 everywhere, every argument the integer -m and every P an exact power of two, which
    # sits ON the boundaries of nothing: no row is fragile however large delta is
    assert not C.fragile_rows(q, torch.zeros_like(k), 0, 2.0 ** -4).any()
    assert torch.equal(C.fragile_rows(q, k, 2), C.walk(q, k, 2)["fragile"])


def test_compare_bites():
    case = C.ONEPASS_STRUCT[0]
    q, k, v = C.case_inputs(*case)
    ref = C.case_reference(*case)
    RO, Rl, fr, mm = ref["O"], ref["lse"], ref["fragile"], ref["vminmax"]
    st = C.compare(RO.clone(), Rl.clone(), RO, Rl, fr, mm, "self")
    assert st["maxabs"] == 0 and st["bit_equal"] and st["rows"] == fr.numel()
    row = int((~fr.reshape(-1)).nonzero()[0])
    bad = RO.clone().reshape(-1, 128)
    bad[row, 5] += 0.03                                            # past the O bar on a sound row
    with pytest.raises(AssertionError):
        C.compare(bad.view(RO.shape), Rl, RO, Rl, fr, mm, "O off")
    bl = Rl.clone().reshape(-1)
    bl[row] += 2e-4 * max(1.0, Rl.abs().max().item())
    with pytest.raises(AssertionError):
        C.compare(RO, bl.view(Rl.shape), RO, Rl, fr, mm, "lse off")
    nan = RO.clone()
    nan[0, 0, 0, 0] = float("nan")
    with pytest.raises(AssertionError):
        C.compare(nan, Rl, RO, Rl, fr, mm, "nan")
    # on a fragile row only finiteness and the hull of the visible V hold: a value outside it fails
    allfr = torch.ones_like(fr)
    hull = RO.clone().reshape(-1, 128)
    hull[row, 7] = (mm[1].reshape(-1, 128)[row, 7] + 0.01).half()
    with pytest.raises(AssertionError):
        C.compare(hull.view(RO.shape), Rl, RO, Rl, allfr, mm, "outside the hull")
    with pytest.raises(AssertionError):                            # and every row fragile is > 2 %
        C.compare(RO, Rl, RO, Rl, allfr, mm, "all fragile")


@pytest.mark.parametrize("entry", ENTRIES, ids=IDS)
def test_cases_raise_and_stay_classifiable(entry):
    name, case, smooth, cached, _ = entry
    shape, kind, seed, causal = case
    q, k, _ = _inputs(case, smooth)
    if name == "tail":
        k = k[:, :, :C.TAIL_CACHE]
    w = C.walk(q, k, causal)
    G = shape[1] // shape[2]
    share, partial = C.raise_stats(w, (G if cached else 1) * shape[3])
    nfr, N = int(w["fragile"].sum()), w["fragile"].numel()
    print(f"MXFP4-CASES {name} {case} smooth={smooth}: late-raising rows {share:.2f}, partial wave x tile "
          f"pairs {partial}, fragile {nfr}/{N}")
    assert nfr <= C.MAX_FRAGILE_SHARE * N, (nfr, N)
    if kind in ("ramp", "spikes"):
        assert share >= 0.25, share
        assert partial >= 1, partial
    if kind == "fall":       # m stays where the first tiles put it: nothing raises past the ramp's top
        assert share <= 0.05, share


@pytest.mark.parametrize("entry", [e for e in ENTRIES if e[4]], ids=[i for e, i in zip(ENTRIES, IDS) if e[4]])
def test_split_restatement_is_the_one_pass_restatement(entry):
    name, case, smooth, _, kpss = entry
    shape, kind, seed, causal = case
    B, H, Hkv, Sq, Sk = shape
    q, k, v = _inputs(case, smooth)
    O1, l1, ops1 = MR.mxfp4_fwd_masked(q, k, v, causal)
    for kps in kpss:
        kps = min(Sk, _split_plan_fp4(B * Hkv, (H // Hkv) * Sq, Sk) if kps is None else kps)
        O2, l2, ops2, (m, l) = SR.mxfp4_fwd_split(q, k, v, causal, kps)
        for a, b in zip(ops1, ops2):
            assert torch.equal(a, b)
        assert m.shape == (-(-Sk // kps), B * H, Sq)
        fin = m[~torch.isinf(m)]
        assert torch.equal(fin, fin.round())
        assert torch.isfinite(O2.float()).all() and torch.isfinite(l2).all()
        assert torch.equal(O2, O1), (kps, (O2.float() - O1.float()).abs().max().item())
        assert (l2 - l1).abs().max().item() <= 1e-6, kps
        assert torch.equal(torch.isinf(m) & (m < 0), l == 0)
        if kind == "ramp" and m.shape[0] > 1:    # the merge runs far from weight 1
            assert ((m.amax(0) - m.amin(0)) > 8).any()


# Restatement vs exact masked fp32 attention on the structured cases, measured on the CPU:
# (cosine, relL2) per (kind, shape, causal).  A peaked row hands its weight to a few keys, whose P
# and V are fp4: the definition is further from exact attention here than on N(0, 1) inputs (cosine
# 0.969 to 0.977 there).  Pinned with a 10 % margin: cosine >= 0.9 x, relL2 <= 1.1 x.
S640, S384, S33, S1 = (1, 4, 2, 160, 640), (1, 2, 2, 384, 384), (1, 4, 2, 33, 640), (2, 8, 2, 1, 640)
DEFINITION_VS_EXACT = {
    ("ramp", S640, 0): (0.8587, 0.5633), ("ramp", S640, 2): (0.8892, 0.4791), ("ramp", S384, 1): (0.9492, 0.3175),
    ("spikes", S640, 0): (0.9319, 0.3644), ("spikes", S640, 2): (0.9337, 0.3592),
    ("spikes", S384, 1): (0.9599, 0.2815),
    ("fall", S640, 0): (0.8823, 0.5467), ("fall", S640, 2): (0.8824, 0.5462), ("fall", S384, 1): (0.9028, 0.4620),
    ("ramp", S33, 0): (0.8810, 0.5461), ("ramp", S33, 2): (0.8816, 0.5227), ("ramp", S1, 0): (0.8813, 0.5067),
    ("spikes", S33, 0): (0.9386, 0.3492), ("spikes", S33, 2): (0.9386, 0.3492), ("spikes", S1, 0): (0.9424, 0.3392),
    ("fall", S33, 0): (0.8777, 0.5340), ("fall", S33, 2): (0.8777, 0.5339), ("fall", S1, 0): (0.8888, 0.4787),
}


@pytest.mark.parametrize("case", C.ONEPASS_STRUCT + [c for c, _ in C.CACHED_STRUCT])
def test_definition_vs_exact_attention_on_peaked_inputs(case):
    """Measured (DEFINITION_VS_EXACT): cosine 0.859 to 0.949 on ramp, 0.932 to 0.960 on spikes, 0.878
    to 0.903 on fall; relL2 0.32 to 0.56, 0.28 to 0.36 and 0.46 to 0.55.  The kernel is held to the
    restatement (tests/test_gpu_mxfp4_fuzz.py), the restatement to these figures."""
    shape, kind, seed, causal = case
    q, k, v = C.case_inputs(*case)
    RO = C.case_reference(*case)["O"]
    ex = MR.exact_masked_attention(q, k, v, causal)
    cos = MR.cosine(RO, ex)
    rel = ((RO.float() - ex).norm() / ex.norm()).item()
    print(f"MXFP4-CASES definition vs exact {case}: cosine {cos:.4f} relL2 {rel:.4f}")
    pc, pr = DEFINITION_VS_EXACT[(kind, shape, causal)]
    assert cos >= 0.9 * pc, (cos, pc)
    assert rel <= 1.1 * pr, (rel, pr)
