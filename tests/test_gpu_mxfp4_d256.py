"""The paged MX-FP4 cache at head_dim 256 (csrc/mxfp4_attn_d256.hip), on the GPU.

Attention is held to the CPU oracle at D = 256 (as tests/test_gpu_mxfp4_d64.py holds it at 64, per sequence, same
mask and split merge) within the bars of both other widths: max|O - O_ref| <= 2e-2, relL2 <= 2e-3, |lse - lse_ref|
<= 1e-4.  Page size and company change no bit, the operator gives the Python call's bits, the appends are the
oracle's quantisers bit for bit, the sink logit keeps its relation, and what a D = 256 pool does not serve raises.
"""
import functools
import math

import pytest
import torch

import test_gpu_mxfp4_d64 as D64   # its helpers take the head dim: pools, queries, the call, the oracle per sequence
from oracle import mxfp4 as M
from test_gpu_mxfp4_d64 import _attend, _oracle

pytestmark = pytest.mark.gpu

D = 256


_pool, _q = functools.partial(D64._pool, D=D), functools.partial(D64._q, D=D)


# (mode, Hkv, G, lengths, q_len, keys_per_split): every length of {1, 63, 64, 65, 127, 128, 129, 200, 449}, splits of
# an odd tile count (192), 65 * 2 = 130 rows (a second row block, a wave across a head boundary), one group of 8
CASES = [("full", 1, 2, (1, 63, 449), 1, 128), ("full", 2, 2, (65, 127, 200), 33, 192),
         ("causal", 2, 2, (1, 65, 129), 1, 128), ("causal", 1, 2, (64, 128, 449), 33, 192),
         ("causal", 1, 2, (127, 200, 449), 65, 128), ("causal", 1, 8, (129, 449), 33, 192),
         ("window", 2, 2, (129, 200, 449), 33, 128), ("window", 1, 2, (63, 128, 449), 1, 192),
         ("gap", 1, 2, (449, 200), 33, 128), ("gap", 2, 2, (449, 65), 1, 192)]


@pytest.mark.parametrize("mode,Hkv,G,lens,n,kps", CASES)
def test_attention_matches_the_oracle(mode, Hkv, G, lens, n, kps):
    cache, kv = _pool(Hkv, lens)
    q = _q(G * Hkv, n * len(lens))
    O, lse = _attend(q, cache, [n] * len(lens), mode, kps)
    for j, (k, v) in enumerate(kv):
        Or, lr = _oracle(q[j * n:(j + 1) * n], k, v, mode, kps)
        Oj, lj = O[j * n:(j + 1) * n].double(), lse[j * n:(j + 1) * n]
        err, rel = (Oj - Or.double()).abs().max().item(), ((Oj - Or.double()).norm() / Or.double().norm()).item()
        dl = (lj - lr).abs().max().item()
        print(f"{mode} L={lens[j]} n={n} G={G} kps={kps}: max|dO| {err:.3e} relL2 {rel:.3e} |dlse| {dl:.3e}")
        assert err <= 2e-2 and rel <= 2e-3 and dl <= 1e-4, (mode, lens[j], err, rel, dl)
    if mode == "full" and n == 1:   # the end-to-end bar: float64 attention on the fp16 inputs
        # The oracle alone gives cosine 0.9697 on these inputs (0.9730 on those of the D = 64 test, whose bar is
        # 0.95): the same margin of 0.023 below the oracle's own figure.
        k, v = (x.transpose(0, 1).double() for x in kv[2])
        qj = q[2:3].transpose(0, 1).double()
        heads = torch.arange(G * Hkv) // G
        ref = torch.softmax(qj @ k[heads].transpose(1, 2) / math.sqrt(D), -1) @ v[heads]
        cos = torch.nn.functional.cosine_similarity(O[2].double().flatten(), ref.flatten(), dim=0).item()
        print(f"cosine against float64 attention: {cos:.4f}")
        assert cos >= 0.946


RAGGED, RAGGED_Q = (449, 129, 65), (33, 1, 3)


@functools.lru_cache(maxsize=None)
def _ragged(P, kps):
    cache, _ = _pool(2, RAGGED, P)
    q = _q(4, sum(RAGGED_Q))
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
    from quantizedattention_amd.kv_cache_mxfp4 import attention_mxfp4_varlen_paged
    cache, q, _ = _ragged(64, 128)
    ids, kw = [0, 1, 2], dict(causal=True, keys_per_split=128, window=window, sinks=4 if window else 0)
    want = attention_mxfp4_varlen_paged(q.cuda(), cache, ids, list(RAGGED_Q), **kw)
    got = ops.mxfp4_varlen_paged(q.cuda(), cache, ids, list(RAGGED_Q), **kw)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def _rotate(x, tab, pos, interleaved):
    """The bit definition of the rotation at half-width 128: x f16 [T, H, 256], tab f32 [max_pos, 256]."""
    c, s = tab[pos][:, None, :128], tab[pos][:, None, 128:]
    a, b = (x[..., 0::2], x[..., 1::2]) if interleaved else (x[..., :128], x[..., 128:])
    a, b = a.float(), b.float()
    first, second = (a * c - b * s).half(), (b * c + a * s).half()
    return torch.stack([first, second], -1).flatten(-2) if interleaved else torch.cat([first, second], -1)


@pytest.mark.parametrize("rope", [None, False, True])
def test_append_matches_the_oracle_quantisers(rope):
    """70, 1 and 57 tokens cross a tile and a page; ``rope``: the pairing (None: no rotation)."""
    from quantizedattention_amd.kv_cache_mxfp4 import PagedKVFP4, Rope, rope_table
    g = torch.Generator().manual_seed(3)
    k, v = torch.randn((128, 2, D), generator=g).half(), torch.randn((128, 2, D), generator=g).half()
    tab = rope_table(160, head_dim=D)
    cache = PagedKVFP4.allocate(4, 64, 2, 2, 3, "cuda", head_dim=D)
    assert cache.shape == (2, 2, 192, D)
    first = 0
    for n in (70, 1, 57):
        cache.append_packed(k[first:first + n].cuda(), v[first:first + n].cuda(), [1], [n],
                            rope=None if rope is None else Rope(tab.cuda(), rope))
        first += n
    if rope is not None:
        k = _rotate(k, tab, torch.arange(128), rope)
    snap = cache.snapshot(1)
    k4, ks = M.quant_rows(k.transpose(0, 1).reshape(256, D))
    vt, vs = M.quant_vt(v.transpose(0, 1).contiguous())
    for got, want in ((snap.k4, k4), (snap.ks, ks), (snap.vt, vt), (snap.vs, vs)):
        assert torch.equal(got.cpu().reshape(want.shape), want)


@pytest.mark.parametrize("mode", ["full", "causal", "gap"])
def test_sink_logit_joins_the_denominator(mode):
    D64.test_sink_logit_joins_the_denominator(D, mode)   # the relation of that test, at this width


def _refusals():
    from quantizedattention_amd import kv_cache_mxfp4 as KC
    h = lambda *s: torch.zeros(s, dtype=torch.float16, device="cuda")  # noqa: E731
    att = lambda c, **kw: KC.attention_mxfp4_varlen_paged(h(2, 2, D), c, [0, 1], [1, 1], causal=True, **kw)  # noqa: E731
    return {"share_prefix": lambda c: att(c, share_prefix=True), "tree": lambda c: att(c, tree=[[-1], None]),
            "checkpoint": lambda c: c.checkpoint([0]), "accept": lambda c: c.accept(None, h(1, 1, D), h(1, 1, D), [0], [1], [[0]]),
            "DecodeStep": lambda c: KC.DecodeStep(2, 256, 2, 1, "cuda").prepare(c, [0, 1]),
            "VerifyStep": lambda c: KC.VerifyStep(2, 256, 2, 1, "cuda", 2).prepare(c, [0, 1]),
            "append": lambda c: c.append(h(2, 1, 1, D), h(2, 1, 1, D)),
            "decode_paged": lambda c: KC.attention_mxfp4_decode_paged(h(2, 2, 1, D), c),
            "rope width": lambda c: c.append_packed(h(1, 1, D), h(1, 1, D), [0], [1],
                                                    rope=KC.Rope(KC.rope_table(8, device="cuda")))}


@pytest.mark.parametrize("what", ["share_prefix", "tree", "checkpoint", "accept", "DecodeStep", "VerifyStep",
                                  "append", "decode_paged", "rope width"])
def test_unsupported_calls_raise_and_change_nothing(what):
    cache, _ = _pool(1, (70, 5))
    before = (cache.free_pages, list(cache.lengths))
    with pytest.raises(ValueError, match="head_dim"):
        _refusals()[what](cache)
    assert (cache.free_pages, list(cache.lengths)) == before
