"""Logit soft-capping and the softmax scale on the paged MX-FP4 cache (mx_tile SOFTCAP), on the GPU, per sequence
against tests/mxfp4_softcap_ref.py: the O bars of tests/test_gpu_mxfp4_d64.py and |dlse| <= 1e-4 + softcap * log2(e)
* 2^-22 (two 1-ulp hardware transcendentals and the subtraction inside the kernel's tanh).  Settings: softcap 50 on
32 q (a good share of |scale * s| pass 50) and softcap 4 on plain inputs (a masked key leaked at -4 would weigh)."""
import math

import pytest
import torch

import mxfp4_softcap_ref as CR
from test_gpu_mxfp4_d64 import G, _attend, _pool, _q

pytestmark = pytest.mark.gpu
MODES = {"window": (128, 0), "gap": (100, 4)}


def _check(q, kv, n, mode, kps, got, cap, scale=None):
    """Every sequence of the call (n queries each) against the restatement."""
    assert bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[1]).all())
    for j, (k, v) in enumerate(kv):
        q4, k4, v4 = (x.transpose(0, 1)[None] for x in (q[j * n:(j + 1) * n], k, v))
        Or, lr = CR.mxfp4_fwd_softcap(q4, k4, v4, MODES.get(mode, mode), kps, cap, scale)
        dO = got[0][j * n:(j + 1) * n].double() - Or[0].transpose(0, 1).double()
        err, rel = dO.abs().max().item(), (dO.norm() / Or.double().norm()).item()
        dl = (got[1][j * n:(j + 1) * n] - lr.transpose(0, 1)).abs().max().item()
        print(f"{mode} D={q.shape[2]} L={k.shape[0]} n={n} kps={kps} cap={cap}: {err:.3e} {rel:.3e} {dl:.3e}")
        assert err <= 2e-2 and rel <= 2e-3 and dl <= 1e-4 + cap * CR.LOG2E * 2.0 ** -22, (j, err, rel, dl)


# (D, mode, Hkv, lengths, q_len, keys_per_split, softcap, power of two on q)
CASES = [(64, "full", 1, (1, 63, 449), 1, 128, 50.0, 32), (64, "causal", 2, (65, 129), 33, 192, 4.0, 1),
         (64, "gap", 1, (449, 200), 33, 128, 50.0, 32), (64, "window", 1, (63, 449), 1, 192, 4.0, 1),
         (128, "full", 2, (65, 200), 33, 192, 4.0, 1), (128, "causal", 1, (64, 449), 33, 128, 50.0, 32),
         (128, "causal", 2, (1, 129), 1, 128, 4.0, 1), (128, "window", 1, (129, 449), 33, 128, 50.0, 32),
         (128, "gap", 2, (449, 65), 1, 192, 4.0, 1), (256, "full", 1, (63, 449), 1, 128, 4.0, 1),
         (256, "causal", 1, (64, 200), 33, 192, 50.0, 32), (256, "gap", 1, (449,), 33, 128, 50.0, 32),
         (256, "window", 1, (200,), 1, 192, 4.0, 1)]


@pytest.mark.parametrize("D,mode,Hkv,lens,n,kps,cap,qmul", CASES)
def test_capped_attention_matches_the_restatement(D, mode, Hkv, lens, n, kps, cap, qmul):
    cache, kv = _pool(Hkv, lens, D=D)
    q = _q(G * Hkv, n * len(lens), D) * qmul
    _check(q, kv, n, mode, kps, _attend(q, cache, [n] * len(lens), mode, kps, softcap=cap), cap)


def test_saturated_logits_stay_finite():
    """A scale at which every nonzero |scale * s / cap| passes 20, so 2^(s c1) is inf or 0 and the logit +-C up to
    rounding.  (A few scores in a thousand are exactly 0 on the FP4 grid; their logit is 0 at any scale.)"""
    cache, kv = _pool(1, (200, 65), D=128)
    q, smin = _q(G, 6, 128), math.inf
    for j, (k, v) in enumerate(kv):
        dq, dk, _, _ = CR._sequence(*(x.transpose(0, 1)[None] for x in (q[3 * j:3 * j + 3], k, v)), "causal")
        s = (dq @ dk[:, :k.shape[0]].transpose(1, 2)).abs()
        smin = min(smin, s[s > 0].min().item())
    scale = 2.0 ** math.ceil(math.log2(20 * 50.0 / smin))
    _check(q, kv, 3, "causal", 128, _attend(q, cache, (3, 3), "causal", 128, softcap=50.0, scale=scale), 50.0, scale)


@pytest.mark.parametrize("D,mode,kw", [(64, "causal", {}), (256, "gap", {}), (128, "full", {}),
                                       (128, "causal", dict(tree=[[-1, 0, 0], None])),
                                       (128, "causal", dict(share_prefix=True))])
def test_scale_alone_is_the_scaled_query(D, mode, kw):
    """scale = 2^3 / sqrt(D) equals the default scale on 8 q bit for bit (the MX scale bytes of q move by 3)."""
    cache, _ = _pool(1, (449, 200), D=D)
    q = _q(G, 6, D)
    got = _attend(q, cache, (3, 3), mode, 128, scale=8.0 / math.sqrt(D), **kw)
    want = _attend(q * 8, cache, (3, 3), mode, 128, **kw)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.parametrize("D,kps,window", [(64, 192, None), (128, 128, 100), (256, 128, None)])
def test_page_size_company_and_operator_change_no_bit(D, kps, window):
    from quantizedattention_amd import ops
    lens, q_lens = (449, 129, 65), (33, 1, 3)
    q = _q(16, sum(q_lens), D) * 32
    kw = dict(causal=True, keys_per_split=kps, window=window, sinks=4 if window else 0, softcap=50.0)
    (cache, _), (cache256, _) = _pool(2, lens, 64, D), _pool(2, lens, 256, D)
    O, lse = (x.cpu() for x in ops.mxfp4_varlen_paged(q.cuda(), cache256, [0, 1, 2], list(q_lens), **kw))
    first = 0
    for j, n in enumerate(q_lens):   # the Python call, 64-token pages, the sequence alone
        Oj, lj = _attend(q[first:first + n], cache, [n], "gap" if window else "causal", kps, ids=[j], softcap=50.0)
        assert torch.equal(Oj, O[first:first + n]) and torch.equal(lj, lse[first:first + n]), j
        first += n


@pytest.mark.parametrize("D,window,sinks", [(64, None, 0), (256, 100, 4)])
def test_decode_step_equals_the_host_planned_capped_pair(D, window, sinks):
    """Eager, then two replays of one captured graph while the lengths grow (63 -> 66 crosses a tile): every step
    is append_packed + the capped packed call at keys_per_split = step.kps, bit for bit; so is the operator."""
    from quantizedattention_amd import kv_cache_mxfp4 as K, ops
    lens, ids = (63, 200, 129), [0, 1, 2]
    (cache, _), (twin, _) = _pool(1, lens, D=D), _pool(1, lens, D=D)
    step = K.DecodeStep(3, 320, G, 1, "cuda", keys_per_split=128, window=window, sinks=sinks, head_dim=D,
                        softcap=50.0)
    assert step.kps == 128 and step.splits == K.decode_step_splits(320, 128, window, sinks)

    def rows(seed):
        g = torch.Generator().manual_seed(seed)
        return [(torch.randn((3, h, D), generator=g) * m).half().cuda() for h, m in ((1, 1), (1, 1), (G, 32))]

    def host(k, v, q):
        twin.append_packed(k, v, ids, [1, 1, 1])
        return K.attention_mxfp4_varlen_paged(q, twin, ids, [1, 1, 1], causal=True, keys_per_split=step.kps,
                                              window=window, sinks=sinks, softcap=50.0)

    sk, sv, sq = rows(1)
    want = host(sk, sv, sq)
    step.prepare(cache, ids)
    for got in (step.append(cache, sk, sv).attend(cache, sq), ops.mxfp4_decode_step(sq, step, cache)):
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gO, glse = step.append(cache, sk, sv).attend(cache, sq)
    for t in (2, 3):
        k, v, q = rows(t)
        want = host(k, v, q)
        step.prepare(cache, ids)
        sk.copy_(k), sv.copy_(v), sq.copy_(q)
        graph.replay()
        assert torch.equal(gO, want[0]) and torch.equal(glse, want[1]), t
    assert cache.lengths == twin.lengths == [66, 203, 132]


def test_sink_logit_joins_the_capped_denominator():
    cache, _ = _pool(1, (449, 200), D=128)
    q = _q(G, 6, 128) * 32
    O, lse = _attend(q, cache, (3, 3), "gap", 128, softcap=50.0)
    sink = torch.tensor([-60.0, 0.0, 45.0, 80.0] * 2)   # below -cap, inside, near the cap, above every capped logit
    Os, ls = _attend(q, cache, (3, 3), "gap", 128, softcap=50.0, sink_logit=sink.cuda())
    want = torch.log2(torch.exp2(lse.double()) + torch.exp2((sink.double() * math.log2(math.e))[None, :]))
    assert (ls.double() - want).abs().max().item() <= 1e-4
    Ow = O.double() * torch.exp2(lse.double() - want)[..., None]
    assert ((Os.double() - Ow).abs() <= 2.0 ** -10 * Ow.abs() + 2.0 ** -24).all()


@pytest.mark.parametrize("name,kw", [("softcap", dict(softcap=50.0, tree=[[-1], None])),
                                     ("softcap", dict(softcap=50.0, share_prefix=True)),
                                     ("softcap", dict(softcap=0.0)), ("softcap", dict(softcap=float("inf"))),
                                     ("scale", dict(scale=-1.0)), ("scale", dict(scale=float("nan")))])
def test_refusals_name_the_argument_and_change_nothing(name, kw):
    from quantizedattention_amd import kv_cache_mxfp4 as K
    from quantizedattention_amd._lib import QAttnError
    cache, _ = _pool(1, (70, 5), D=128)
    before = (cache.free_pages, list(cache.lengths))
    q = torch.zeros((2, G, 128), dtype=torch.float16, device="cuda")
    with pytest.raises(QAttnError, match=name):
        K.attention_mxfp4_varlen_paged(q, cache, [0, 1], [1, 1], causal=True, **kw)
    if len(kw) == 1:
        with pytest.raises(QAttnError, match=name):
            K.DecodeStep(2, 256, G, 1, "cuda", head_dim=128, **kw)
    assert (cache.free_pages, list(cache.lengths)) == before
