"""The paged MX-FP4 cache at head_dim 64 (csrc/mxfp4_attn_d64.hip) and the learned sink logit of the packed
step, on the GPU.

Attention is held to the CPU oracle at D = 64 (oracle/mxfp4.py through tests/mxfp4_ragged_ref.py and
tests/mxfp4_window_ref.py, per sequence, same mask and split merge) within the bars of tests/test_gpu_mxfp4.py:
max|O - O_ref| <= 2e-2, relL2 <= 2e-3, |lse - lse_ref| <= 1e-4.  Page size, company and the ring's pairing
change no bit.  The sink logit is held to the call without it: lse' = log2(2^lse + 2^z) to 1e-4 and O' = O *
2^(lse - lse') within 2^-10 |O| + 2^-24 (one f16 rounding on either side).  The entry takes no sequence
without a visible key (every listed sequence holds a key, and a causal or windowed query sees itself), so the
row that sees no key is covered by tests/test_mxfp4_d64_ref.py alone.
"""
import functools
import math

import pytest
import torch

import mxfp4_ragged_ref as RR
import mxfp4_split_ref as SR
import mxfp4_window_ref as WR
from oracle import mxfp4 as M

pytestmark = pytest.mark.gpu

G = 8


def _pool(Hkv, lens, P=64, D=64, seed=5):
    """A pool holding one sequence per length, appended in one packed call -> (cache, [(k, v) [L, Hkv, D]])."""
    from quantizedattention_amd.kv_cache_mxfp4 import PagedKVFP4
    g = torch.Generator().manual_seed(seed)
    kv = [(torch.randn((L, Hkv, D), generator=g).half(), torch.randn((L, Hkv, D), generator=g).half()) for L in lens]
    mpp = -(-max(lens) // P) + 1
    cache = PagedKVFP4.allocate(len(lens) * mpp, P, len(lens), Hkv, mpp, "cuda", head_dim=D)
    cache.append_packed(torch.cat([k for k, _ in kv]).cuda(), torch.cat([v for _, v in kv]).cuda(),
                        list(range(len(lens))), list(lens))
    return cache, kv


def _q(Hq, T, D=64, seed=9):
    return torch.randn((T, Hq, D), generator=torch.Generator().manual_seed(seed)).half()


def _attend(q, cache, q_lens, mode, kps, ids=None, **kw):
    from quantizedattention_amd.kv_cache_mxfp4 import attention_mxfp4_varlen_paged
    W, S = {"window": (128, 0), "gap": (100, 4)}.get(mode, (None, 0))
    O, lse = attention_mxfp4_varlen_paged(q.cuda(), cache, list(range(len(q_lens))) if ids is None else ids,
                                          list(q_lens), causal=mode != "full", keys_per_split=kps, window=W,
                                          sinks=S, **kw)
    return O.cpu(), lse.cpu()


def _oracle(q_j, k, v, mode, kps):
    """One sequence: q_j [n, Hq, D], k, v [L, Hkv, D] -> (O [n, Hq, D] fp16, lse [n, Hq]) of the CPU oracle."""
    q4, k4, v4 = (x.transpose(0, 1)[None] for x in (q_j, k, v))
    if mode in ("window", "gap"):
        O, lse, _ = WR.mxfp4_fwd_window(q4, k4, v4, *((128, 0) if mode == "window" else (100, 4)), kps)
    else:
        kps = min(kps, RR.ceil64(k.shape[0]))
        m, l, Op = RR.sequence_partials(q4, k4, v4, mode == "causal", kps, -(-RR.ceil64(k.shape[0]) // kps))
        O, lse = SR.merge(m, l, Op)
    return O.view(q4.shape)[0].transpose(0, 1), lse.view(q4.shape[1], -1).transpose(0, 1)


# (mode, Hkv, lengths, q_len, keys_per_split): every length of {1, 63, 64, 65, 127, 128, 129, 200, 449}, a lone
# last tile in a pair slot, splits of an odd tile count (192), 33 * 8 = 264 rows across a head boundary
CASES = [("full", 1, (1, 63, 449), 1, 128), ("full", 2, (65, 127, 200), 33, 192),
         ("causal", 2, (1, 65, 129), 1, 128), ("causal", 1, (64, 128, 449), 33, 192),
         ("causal", 1, (127, 200, 449), 33, 128), ("window", 2, (129, 200, 449), 33, 128),
         ("window", 1, (63, 128, 449), 1, 192), ("gap", 1, (449, 200), 33, 128), ("gap", 2, (449, 65), 1, 192)]


@pytest.mark.parametrize("mode,Hkv,lens,n,kps", CASES)
def test_attention_matches_the_oracle(mode, Hkv, lens, n, kps):
    cache, kv = _pool(Hkv, lens)
    q = _q(G * Hkv, n * len(lens))
    O, lse = _attend(q, cache, [n] * len(lens), mode, kps)
    for j, (k, v) in enumerate(kv):
        Or, lr = _oracle(q[j * n:(j + 1) * n], k, v, mode, kps)
        Oj, lj = O[j * n:(j + 1) * n].double(), lse[j * n:(j + 1) * n]
        err, rel = (Oj - Or.double()).abs().max().item(), ((Oj - Or.double()).norm() / Or.double().norm()).item()
        dl = (lj - lr).abs().max().item()
        print(f"{mode} L={lens[j]} n={n} kps={kps}: max|dO| {err:.3e} relL2 {rel:.3e} |dlse| {dl:.3e}")
        assert err <= 2e-2 and rel <= 2e-3 and dl <= 1e-4, (mode, lens[j], err, rel, dl)
    if mode == "full" and n == 1:   # the end-to-end bar: float64 attention on the fp16 inputs
        k, v = (x.transpose(0, 1).double() for x in kv[2])
        qj = q[2:3].transpose(0, 1).double()
        ref = torch.softmax(qj @ k[torch.arange(G * Hkv) // G].transpose(1, 2) / 8.0, -1) @ v[torch.arange(G * Hkv) // G]
        cos = torch.nn.functional.cosine_similarity(O[2].double().flatten(), ref.flatten(), dim=0).item()
        print(f"cosine against float64 attention: {cos:.4f}")
        assert cos >= 0.95


RAGGED, RAGGED_Q = (449, 129, 65), (33, 1, 3)


@functools.lru_cache(maxsize=None)
def _ragged(P, kps):
    cache, _ = _pool(2, RAGGED, P)
    q = _q(16, sum(RAGGED_Q))
    return cache, q, _attend(q, cache, RAGGED_Q, "causal", kps)


@pytest.mark.parametrize("kps", [128, 192])
def test_page_size_and_company_change_no_bit(kps):
    (cache, q, (O, lse)), (_, _, (O256, lse256)) = _ragged(64, kps), _ragged(256, kps)
    assert torch.equal(O, O256) and torch.equal(lse, lse256)
    first = 0
    for j, n in enumerate(RAGGED_Q):
        Oj, lj = _attend(q[first:first + n], cache, [n], "causal", kps, ids=[j])
        assert torch.equal(Oj, O[first:first + n]) and torch.equal(lj, lse[first:first + n]), j
        first += n


@pytest.mark.parametrize("window", [None, 100])
def test_operator_gives_the_python_calls_bits(window):
    from quantizedattention_amd import ops
    cache, q, _ = _ragged(64, 128)
    ids, kw = [0, 1, 2], dict(causal=True, keys_per_split=128, window=window, sinks=4 if window else 0)
    from quantizedattention_amd.kv_cache_mxfp4 import attention_mxfp4_varlen_paged
    want = attention_mxfp4_varlen_paged(q.cuda(), cache, ids, list(RAGGED_Q), **kw)
    got = ops.mxfp4_varlen_paged(q.cuda(), cache, ids, list(RAGGED_Q), **kw)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def _rotate(x, tab, pos, interleaved):
    """The bit definition of the rotation at half-width 32: x f16 [T, H, 64], tab f32 [max_pos, 64]."""
    c, s = tab[pos][:, None, :32], tab[pos][:, None, 32:]
    a, b = (x[..., 0::2], x[..., 1::2]) if interleaved else (x[..., :32], x[..., 32:])
    a, b = a.float(), b.float()
    first, second = (a * c - b * s).half(), (b * c + a * s).half()
    return torch.stack([first, second], -1).flatten(-2) if interleaved else torch.cat([first, second], -1)


@pytest.mark.parametrize("rope", [None, False, True])
def test_append_matches_the_oracle_quantisers(rope):
    """70, 1 and 57 tokens cross a tile and a page; ``rope``: the pairing (None: no rotation)."""
    from quantizedattention_amd.kv_cache_mxfp4 import PagedKVFP4, Rope, rope_table
    g = torch.Generator().manual_seed(3)
    k, v = torch.randn((128, 2, 64), generator=g).half(), torch.randn((128, 2, 64), generator=g).half()
    tab = rope_table(160, head_dim=64)
    cache = PagedKVFP4.allocate(4, 64, 2, 2, 3, "cuda", head_dim=64)
    assert cache.shape == (2, 2, 192, 64)
    first = 0
    for n in (70, 1, 57):
        cache.append_packed(k[first:first + n].cuda(), v[first:first + n].cuda(), [1], [n],
                            rope=None if rope is None else Rope(tab.cuda(), rope))
        first += n
    if rope is not None:
        k = _rotate(k, tab, torch.arange(128), rope)
    snap = cache.snapshot(1)
    k4, ks = M.quant_rows(k.transpose(0, 1).reshape(256, 64))
    vt, vs = M.quant_vt(v.transpose(0, 1).contiguous())
    for got, want in ((snap.k4, k4), (snap.ks, ks), (snap.vt, vt), (snap.vs, vs)):
        assert torch.equal(got.cpu().reshape(want.shape), want)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("mode", ["full", "causal", "gap"])
def test_sink_logit_joins_the_denominator(D, mode):
    cache, _ = _pool(1, (449, 200), D=D)
    q = _q(G, 6, D)
    O, lse = _attend(q, cache, (3, 3), mode, 128)
    O0, lse0 = _attend(q, cache, (3, 3), mode, 128, sink_logit=None)
    assert torch.equal(O, O0) and torch.equal(lse, lse0)
    # far below, level with, above the scores, and above every score
    sink = torch.tensor([-30.0, 0.0, 5.0, 40.0] * 2)
    Os, ls = _attend(q, cache, (3, 3), mode, 128, sink_logit=sink.cuda())
    z = (sink.double() * math.log2(math.e))[None, :]
    want = torch.log2(torch.exp2(lse.double()) + torch.exp2(z))
    assert (ls.double() - want).abs().max().item() <= 1e-4
    Ow = O.double() * torch.exp2(lse.double() - want)[..., None]
    assert ((Os.double() - Ow).abs() <= 2.0 ** -10 * Ow.abs() + 2.0 ** -24).all()


def _refusals():
    from quantizedattention_amd import kv_cache_mxfp4 as KC
    h = lambda *s: torch.zeros(s, dtype=torch.float16, device="cuda")  # noqa: E731
    att = lambda c, **kw: KC.attention_mxfp4_varlen_paged(h(2, 8, 64), c, [0, 1], [1, 1], causal=True, **kw)  # noqa: E731
    return {"share_prefix": lambda c: att(c, share_prefix=True), "tree": lambda c: att(c, tree=[[-1], None]),
            "checkpoint": lambda c: c.checkpoint([0]), "rollback": lambda c: c.rollback(None),
            "accept": lambda c: c.accept(None, h(1, 1, 64), h(1, 1, 64), [0], [1], [[0]]),
            "DecodeStep": lambda c: KC.DecodeStep(2, 256, 8, 1, "cuda").prepare(c, [0, 1]),
            "VerifyStep": lambda c: KC.VerifyStep(2, 256, 8, 1, "cuda", 2).prepare(c, [0, 1]),
            "append": lambda c: c.append(h(2, 1, 1, 64), h(2, 1, 1, 64)),
            "decode_paged": lambda c: KC.attention_mxfp4_decode_paged(h(2, 8, 1, 64), c),
            "rope width": lambda c: c.append_packed(h(1, 1, 64), h(1, 1, 64), [0], [1],
                                                    rope=KC.Rope(KC.rope_table(8, device="cuda")))}


@pytest.mark.parametrize("what", ["share_prefix", "tree", "checkpoint", "rollback", "accept", "DecodeStep",
                                  "VerifyStep", "append", "decode_paged", "rope width"])
def test_unsupported_calls_raise_and_change_nothing(what):
    from quantizedattention_amd._lib import QAttnError
    cache, _ = _pool(1, (70, 5))
    before = (cache.free_pages, list(cache.lengths))
    with pytest.raises(QAttnError if what == "rope width" else ValueError, match="head_dim"):
        _refusals()[what](cache)
    assert (cache.free_pages, list(cache.lengths)) == before
