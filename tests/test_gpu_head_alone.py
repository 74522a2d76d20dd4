"""Grid independence, bit for bit: the part of a multi-head launch that belongs to one key/value head
and its G query heads equals the launch of that part alone (B = 1, Hkv = 1, Hq = G, same Sq, Sk, D
and causal flag).

Every entry here is deterministic (no atomics, one writer per output tile, a fixed streaming order)
and heads are independent, so which workgroup runs a tile, on which XCD, in which order, beside which
other heads and in which workspace chunk may not change a bit of it.  The schedulers under test are
``xcd_remap``, ``xcd_remap_lpt`` and ``xcd_remap_lpt_grouped`` (csrc/common.h; both of their branches,
heads a multiple of 8 or not), the causal dK+dV groups of ``QA_DKV_HG`` = 4 heads per XCD, the
head-chunked dS workspace (``qattn_int8_attn_bwd_wsc``), the grouped-query "virtual head" of the
non-causal int8 forward and the bf16 forward's per-head V-suffix workspace.  (The largest tensor here
holds 3.4e7 elements, so a head offset computed in 32 bits would pass: tests/test_gpu_big_index.py is
where the 64-bit offsets are exercised, with this instrument on tensors past 2^31 elements.)  The other
exact comparisons of the suite hold two entries to each other that run
the same dK+dV kernel on the same grid; this one gives every head of the grid a second opinion.

No tolerance appears in this module: ``torch.equal`` on the bit patterns.  The full launch runs
first, on inputs seeded per test and generated on the GPU, and every slice input is a copy, so a slice
run cannot see its neighbours' rows and a tile the full launch never wrote cannot hold a stale value.
None of this runs the CPU oracle.

Shapes.  *Ragged full grid*: (B, Hq, Hkv) = (3, 42, 21), so B*Hq = 126 and B*Hkv = 63 are no
multiples of 8 (nor B*Hkv of 4) and G = 2; Sq = Sk = 2080 = 16 * 128 + 32 = 8 * 256 + 32 leaves a last
workgroup of one active wave for every workgroup size in play, and the non-causal cases also run
Sq = 1056 = 8 * 128 + 32 against Sk = 2080.  The JVP uses Sk = 2112 (its bf16 mode streams 64-key
stages).  Workgroups per launch, from the launch code in csrc/*.hip, at Sq = 2080 (Sq = 1056):

  int8 forward, 128 query rows: causal 126 * 17 = 2142; non-causal the G = 2 heads of a key/value
      head run as one virtual head of G * Sq rows, 63 * 33 = 2079 (63 * 17 = 1071)
  int8 fused dK+dV, 256 keys: 63 * 9 = 567 in one pass, 9 / 45 per chunk of 1 / 5 key/value heads
  int8 dQ from records, 256 query rows: 126 * 9 = 1134 (126 * 5 = 630); recomputing dQ, 128 rows:
      126 * 17 = 2142 (126 * 9 = 1134)
  bf16 forward, 128 query rows: 2142 (1134); its V-suffix passes 63 * 65 = 4095 and 63
  bf16 fused dK+dV and split dV / dK, 128 keys: 63 * 17 = 1071 each; dQ and dQ from records, 256
      query rows (recomputing at D = 64: 128): 1134 (630), at D = 64 2142 (1134)
  JVP, 128 query rows: 2142

all above twice the 256 CUs.  (With (3, 14, 7), a third of the heads, the fused dK+dV kernels would
launch 189 and 357.)  *The headline*: (4, 32, 4096, 128), G = 1, the benchmark's configuration with the
default workspace plan (4 chunks of 32 heads non-causal, one pass causal; 128 heads take the
multiple-of-8 branches and the grouped causal order): all 128 heads against their own single-head run.
"""
import pytest
import torch

from head_alone import _Diff, _cut, _gen, _groups, _heads, _randn  # noqa: F401

pytestmark = pytest.mark.gpu

B_, HQ, HKV = 3, 42, 21
S_LONG, S_SHORT, SK_JVP = 2080, 1056, 2112
# (causal, Sq, Sk)
SEQ = [(True, S_LONG, S_LONG), (False, S_LONG, S_LONG), (False, S_SHORT, S_LONG)]
SEQ_IDS = ["causal-2080", "full-2080", "full-1056x2080"]


def _finite(*xs):
    for x in xs:
        if x is not None and x.is_floating_point():
            assert torch.isfinite(x).all()


# ------------------------------------------------------------------------------------ int8
FWD_NAMES = ("O", "lse", "q_i8", "k_i8", "v_i8", "sq", "sk", "sv", "k_mean", "q_bf", "k_bf")
FWD_SIDE = ("q", "q", "q", "kv", "kv", "q", "kv", "kv", "kv", "q", "kv")


def _int8_fwd_parts(out, B, Hq, Hkv):
    """The forward's outputs as [B, H, flat] views (k_i8T back in its row-major [N, D] form)."""
    out = list(out)
    out[3] = out[3].t()
    return [None if x is None else _heads(x, B, Hq if side == "q" else Hkv)
            for x, side in zip(out, FWD_SIDE)]


def _int8_fwd(q, k, v, causal, smooth):
    from quantizedattention_amd.attention_int8 import _int8_forward, helion_atten_int8_hl_dot_fwd
    if smooth:
        return _int8_forward(q, k, v, smooth=True, images=True, causal=causal)
    return tuple(helion_atten_int8_hl_dot_fwd(q, k, v, causal=causal)[:8]) + (None, None, None)


def _check_int8_fwd(q, k, v, causal, smooth, diff):
    B, Hq, Hkv = q.shape[0], q.shape[1], k.shape[1]
    full = _int8_fwd(q, k, v, causal, smooth)
    _finite(full[0], full[1], full[5], full[6], full[7], full[8])
    parts = _int8_fwd_parts(full, B, Hq, Hkv)
    for b, kh, hs in _groups(B, Hq, Hkv):
        alone = _int8_fwd(q[b:b + 1, hs].clone(), k[b:b + 1, kh:kh + 1].clone(), v[b:b + 1, kh:kh + 1].clone(),
                          causal, smooth)
        for name, side, a, f in zip(FWD_NAMES, FWD_SIDE, _int8_fwd_parts(alone, 1, hs.stop - hs.start, 1), parts):
            if f is not None:
                diff.eq(name, (b, kh), a, f[b, hs] if side == "q" else f[b, kh])
    return full


def _int8_bwd_args(parts, dO, B, Hq, Hkv, b, kh, hs):
    """Copies of one key/value head's share of the forward's outputs, in _int8_backward's order and
    shapes: (dO, q_i8, sq, k_i8T, sk, v_i8, sv, O, lse, q_bf, k_bf)."""
    O, lse, qi, ki, vi, sq, sk, sv, _, qb, kb = parts
    G, Sq, D = hs.stop - hs.start, dO.shape[2], dO.shape[3]
    c = lambda x, h: x[b:b + 1, h].clone()   # noqa: E731
    kh1 = slice(kh, kh + 1)
    return (c(_heads(dO, B, Hq), hs).view(1, G, Sq, D), c(qi, hs).view(-1, D), c(sq, hs).view(-1),
            c(ki, kh1).view(-1, D).t(), c(sk, kh1).view(-1), c(vi, kh1).view(-1, D), c(sv, kh1).view(-1),
            c(O, hs).view(1, G, Sq, D), c(lse, hs).view(-1), c(qb, hs).view(-1, D), c(kb, kh1).view(-1, D))


# the recomputing backward, and the record backward in one pass, in chunks of one key/value head and
# in chunks of 5 (63 = 12 * 5 + 3: a short last chunk).  Alone, a head is its own chunk either way.
BWD_FULL = (("recompute", dict(use_ws=False)), ("ws-onepass", dict(use_ws=True, ws_chunk=0)),
            ("ws-chunk1", dict(use_ws=True, ws_chunk=1)), ("ws-chunk5", dict(use_ws=True, ws_chunk=5)))
BWD_ALONE = {"recompute": dict(use_ws=False), "ws": dict(use_ws=True, ws_chunk=0)}


def _check_int8_bwd(full_fwd, dO, Hkv, causal, variants, alone_kw, diff):
    from quantizedattention_amd.attention_int8 import _int8_backward
    B, Hq = dO.shape[0], dO.shape[1]
    O, lse, qi, kiT, vi, sq, sk, sv, _, qb, kb = full_fwd
    full = {name: _int8_backward(dO, qi, sq, kiT, sk, vi, sv, O, lse, qb, kb, causal=causal, kv_heads=Hkv, **kw)
            for name, kw in variants}
    for grads in full.values():
        _finite(*grads)
        assert all(g.abs().max().item() > 0 for g in grads)
    parts = _int8_fwd_parts(full_fwd, B, Hq, Hkv)
    for b, kh, hs in _groups(B, Hq, Hkv):
        args = _int8_bwd_args(parts, dO, B, Hq, Hkv, b, kh, hs)
        alone = {key: _int8_backward(*args, causal=causal, kv_heads=1, **kw) for key, kw in alone_kw.items()}
        for name, _ in variants:
            a = alone["recompute" if name == "recompute" else "ws"]
            f = full[name]
            diff.eq(f"{name}.dq", (b, kh), a[0], f[0][b, hs])
            diff.eq(f"{name}.dk", (b, kh), a[1], f[1][b, kh])
            diff.eq(f"{name}.dv", (b, kh), a[2], f[2][b, kh])


def _int8_inputs(key, B, Hq, Hkv, Sq, Sk, D):
    g = _gen(*key)
    q = _randn((B, Hq, Sq, D), g, torch.float16)
    k = _randn((B, Hkv, Sk, D), g, torch.float16)
    v = _randn((B, Hkv, Sk, D), g, torch.float16)
    dO = _randn((B, Hq, Sq, D), g, torch.float16)
    return q, k, v, dO


@pytest.mark.parametrize("seq", SEQ, ids=SEQ_IDS)
@pytest.mark.parametrize("D", [64, 128])
def test_int8_forward_full_grid(lib, D, seq):
    """``_int8_forward(smooth=True, images=True)`` and ``helion_atten_int8_hl_dot_fwd``: O, lse, the
    three quantised operands with their scales, k_mean and the backward's bf16 images."""
    causal, Sq, Sk = seq
    q, k, v, _ = _int8_inputs(("int8-fwd", D, seq), B_, HQ, HKV, Sq, Sk, D)
    diff = _Diff()
    _check_int8_fwd(q, k, v, causal, True, diff)
    _check_int8_fwd(q, k, v, causal, False, diff)
    diff.done()


@pytest.mark.parametrize("seq", SEQ, ids=SEQ_IDS)
@pytest.mark.parametrize("D", [64, 128])
def test_int8_backward_full_grid(lib, D, seq):
    """``_int8_backward`` on the full launch's own forward outputs: dq, dk, dv of the recomputing
    backward and of the record backward in one pass, in chunks of 1 and of 5 key/value heads."""
    from quantizedattention_amd.attention_int8 import _int8_forward
    causal, Sq, Sk = seq
    q, k, v, dO = _int8_inputs(("int8-bwd", D, seq), B_, HQ, HKV, Sq, Sk, D)
    fwd = _int8_forward(q, k, v, smooth=True, images=True, causal=causal)
    diff = _Diff()
    _check_int8_bwd(fwd, dO, HKV, causal, BWD_FULL, BWD_ALONE, diff)
    diff.done()


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_int8_headline_every_head(lib, causal):
    """(4, 32, 4096, 128), the benchmark's configuration: forward and backward with the default
    workspace plan, each of the 128 heads against the run of that head alone."""
    from quantizedattention_amd import _lib
    B, H, S, D = 4, 32, 4096, 128
    assert _lib.int8_bwd_plan(B * H, 1, S, S, causal)[1] == (B * H if causal else 32)
    q, k, v, dO = _int8_inputs(("int8-headline", causal), B, H, H, S, S, D)
    diff = _Diff()
    fwd = _check_int8_fwd(q, k, v, causal, True, diff)
    default = dict(use_ws=None, ws_chunk=None)
    _check_int8_bwd(fwd, dO, H, causal, (("default", default),), {"ws": default}, diff)
    assert diff.n == 128 * (11 + 3)
    diff.done()


# ------------------------------------------------------------------------------------ bf16
def _bf16_inputs(key, Sq, Sk, D):
    # (q, k at 0.75: the reference's beta rule, which the forward follows, overflows on large logits)
    g = _gen(*key)
    q = _randn((B_, HQ, Sq, D), g, torch.float16, 0.75)
    k = _randn((B_, HKV, Sk, D), g, torch.float16, 0.75)
    v = _randn((B_, HKV, Sk, D), g, torch.bfloat16)
    dO = _randn((B_, HQ, Sq, D), g, torch.float32)
    return q, k, v, dO


@pytest.mark.parametrize("seq", SEQ, ids=SEQ_IDS)
@pytest.mark.parametrize("D", [64, 128])
def test_bf16_forward_full_grid(lib, D, seq):
    """``helion_atten_bf16_fwd_training``; causal is the V-suffix workspace path, one suffix table per
    key/value head."""
    from quantizedattention_amd.attention_bf16 import helion_atten_bf16_fwd_training as fwd
    causal, Sq, Sk = seq
    q, k, v, _ = _bf16_inputs(("bf16-fwd", D, seq), Sq, Sk, D)
    O, lse = fwd(q, k, v, causal)
    _finite(O, lse)
    lse = lse.view(B_, HQ, Sq)
    diff = _Diff()
    for b, kh, hs in _groups(B_, HQ, HKV):
        O1, l1 = fwd(q[b:b + 1, hs].clone(), k[b:b + 1, kh:kh + 1].clone(), v[b:b + 1, kh:kh + 1].clone(), causal)
        diff.eq("O", (b, kh), O1, O[b, hs])
        diff.eq("lse", (b, kh), l1, lse[b, hs])
    diff.done()


BF16_ENTRIES = ("ws", "qattn_bf16_bwd_ex", "qattn_bf16_bwd_split_ex")


@pytest.mark.parametrize("seq", SEQ, ids=SEQ_IDS)
@pytest.mark.parametrize("D", [64, 128])
def test_bf16_backward_full_grid(lib, monkeypatch, D, seq):
    """``helion_flash_atten_2_algo_4_bwd`` through its three entries: dS records, the fused dK+dV
    with a recomputing dQ, and the split dV / dK kernels."""
    from quantizedattention_amd import attention_bf16 as A
    causal, Sq, Sk = seq
    q, k, v, dO = _bf16_inputs(("bf16-bwd", D, seq), Sq, Sk, D)
    O, lse = A.helion_atten_bf16_fwd_training(q, k, v, causal)
    full = {}
    for entry in BF16_ENTRIES:
        monkeypatch.setattr(A, "_BWD_ENTRY", entry)
        full[entry] = A.helion_flash_atten_2_algo_4_bwd(q, k, v, O, lse, causal, dO)
        _finite(*full[entry])
    diff = _Diff()
    for b, kh, hs in _groups(B_, HQ, HKV):
        args = (q[b:b + 1, hs].clone(), k[b:b + 1, kh:kh + 1].clone(), v[b:b + 1, kh:kh + 1].clone(),
                O[b:b + 1, hs].clone(), lse.view(B_, HQ, Sq)[b, hs].clone(), causal, dO[b:b + 1, hs].clone())
        for entry in BF16_ENTRIES:
            monkeypatch.setattr(A, "_BWD_ENTRY", entry)
            dq, dk, dv = A.helion_flash_atten_2_algo_4_bwd(*args)
            f = full[entry]
            diff.eq(f"{entry}.dq", (b, kh), dq, f[0][b, hs])
            diff.eq(f"{entry}.dk", (b, kh), dk, f[1][b, kh])
            diff.eq(f"{entry}.dv", (b, kh), dv, f[2][b, kh])
    diff.done()


# ------------------------------------------------------------------------------------- JVP
@pytest.mark.parametrize("mode", ["bf16", "fp32", "primal-bf16", "primal-fp32"])
@pytest.mark.parametrize("D", [64, 128])
def test_jvp_full_grid(lib, D, mode):
    """``_jvp`` with bf16 inputs, with fp32 inputs (the x3 kernel) and primal-only: O, tO and lse."""
    from quantizedattention_amd.attention_jvp import _jvp
    dt = torch.bfloat16 if mode.endswith("bf16") else torch.float32
    g = _gen("jvp", D, mode)
    qs, ks = (B_, HQ, S_LONG, D), (B_, HKV, SK_JVP, D)
    q, k, v, tq, tk, tv = (_randn(s, g, dt) for s in (qs, ks, ks, qs, ks, ks))
    tangent = not mode.startswith("primal")
    O, tO, lse = _jvp(q, k, v, (tq, tk, tv) if tangent else None)
    _finite(O, tO, lse)
    lse = lse.view(B_, HQ, S_LONG)
    diff = _Diff()
    for b, kh, hs in _groups(B_, HQ, HKV):
        cq = lambda x: x[b:b + 1, hs].clone()            # noqa: E731
        ck = lambda x: x[b:b + 1, kh:kh + 1].clone()     # noqa: E731
        O1, tO1, l1 = _jvp(cq(q), ck(k), ck(v), (cq(tq), ck(tk), ck(tv)) if tangent else None)
        diff.eq("O", (b, kh), O1, O[b, hs])
        diff.eq("lse", (b, kh), l1, lse[b, hs])
        if tangent:
            diff.eq("tO", (b, kh), tO1, tO[b, hs])
    diff.done()
