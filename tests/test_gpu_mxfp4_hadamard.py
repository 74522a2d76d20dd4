"""Hadamard-rotated pools (PagedKVFP4.allocate(hadamard=True)) on the GPU.  The oracle (tests/mxfp4_ragged_ref.py) has
its qks built in, so qks / D reaches it as the exact power of two 1 / D folded into the rotated queries: the same
codes, block scales D times smaller, and every fp32 rounding of scores and logits is invariant under that factor.
"""
import pytest
import torch

import mxfp4_hadamard_ref as HR
import mxfp4_ragged_ref as RR
import mxfp4_split_ref as SR
from quantizedattention_amd import kv_cache_mxfp4 as K
from quantizedattention_amd._lib import QAttnError

pytestmark = pytest.mark.gpu
DIMS = [64, 128, 256]


def _rand(seed, *shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).half()


def _rope(D, interleaved, max_pos=160):
    tab = K.rope_table(max_pos, head_dim=D)
    return tab, None if interleaved is None else K.Rope(tab.cuda(), interleaved)


@pytest.mark.parametrize("smooth", [False, True])
@pytest.mark.parametrize("interleaved", [None, False, True])
@pytest.mark.parametrize("D", DIMS)
def test_append_matches_the_restated_quantiser(D, interleaved, smooth):
    """70, 1 and 57 tokens to slot 1 cross a tile and a page of 64; V is the plain pool's, byte for byte."""
    k, v = _rand(3, 128, 2, D), _rand(4, 128, 2, D)
    mean = (0.25 * _rand(5, 2, 2, 1, D).float()).half() if smooth else None
    tab, rope = _rope(D, interleaved)
    pools = [K.PagedKVFP4.allocate(4, 64, 2, 2, 3, "cuda", k_mean=mean, head_dim=D, hadamard=h) for h in (True, False)]
    for cache in pools:
        first = 0
        for n in (70, 1, 57):
            cache.append_packed(k[first:first + n].cuda(), v[first:first + n].cuda(), [1], [n], rope=rope)
            first += n
    if rope is not None:
        k = HR.rope(k, tab, torch.arange(128), interleaved)
    want4, wants = HR.quant_rows_had(k.transpose(0, 1).reshape(256, D),
                                     None if mean is None else mean[1].expand(2, 128, D).reshape(256, D))
    (k4, ks, vt, vs), plain = pools[0].gather(1), pools[1].gather(1)
    assert torch.equal(k4.cpu().reshape(want4.shape), want4) and torch.equal(ks.cpu().reshape(wants.shape), wants)
    assert torch.equal(vt, plain[2]) and torch.equal(vs, plain[3]) and not torch.equal(k4, plain[0])


@pytest.mark.parametrize("interleaved", [None, False, True])
@pytest.mark.parametrize("T,H", [(3, 1), (5, 3)])   # 3 rows: a partly filled wave of 6, 12 or 24 lanes
@pytest.mark.parametrize("D", DIMS)
def test_query_operator_matches_the_restated_quantiser(D, T, H, interleaved):
    from quantizedattention_amd import ops
    x, pos = _rand(7, T, H, D), [159, 0, 77, 3, 3][:T]
    tab, rope = _rope(D, interleaved)
    q4, qs = ops.mxfp4_quant_rows_had(x.cuda(), rope, None if rope is None else pos)
    want4, wants = HR.quant_rows_had((x if rope is None else HR.rope(x, tab, pos, interleaved)).reshape(T * H, D))
    assert torch.equal(q4.cpu(), want4) and torch.equal(qs.cpu(), wants)


def _oracle(q, k, v, causal, kps):
    """One sequence on rotated operands: q f16 [n, Hq, D], k, v f16 [L, Hkv, D] -> (O [n, Hq, D], lse [n, Hq])."""
    D, L = q.shape[-1], k.shape[0]
    q4, k4, v4 = (x.transpose(0, 1)[None] for x in (HR.rotated(q) / D, HR.rotated(k), v))
    m, l, Op = RR.sequence_partials(q4, k4, v4, causal, min(kps, RR.ceil64(L)), -(-RR.ceil64(L) // kps))
    O, lse = SR.merge(m, l, Op)
    return O.view(q4.shape)[0].transpose(0, 1), lse.view(q4.shape[1], -1).transpose(0, 1)


def _pool(D, kv, hadamard=True, P=64):
    lens = [k.shape[0] for k, _ in kv]
    mpp = -(-max(lens) // P) + 1
    cache = K.PagedKVFP4.allocate(len(kv) * mpp, P, len(kv), kv[0][0].shape[1], mpp, "cuda", head_dim=D,
                                  hadamard=hadamard)
    return cache.append_packed(torch.cat([k for k, _ in kv]).cuda(), torch.cat([v for _, v in kv]).cuda(),
                               list(range(len(kv))), lens)


@pytest.mark.parametrize("D", DIMS)
def test_scores_are_preserved(D):
    """One ragged causal call; the bars of tests/test_gpu_mxfp4.py: max|dO| 2e-2, relL2 2e-3, |dlse| 1e-4."""
    lens, q_lens, kps = (65, 129, 449), (33, 1, 3), 128
    kv = [(_rand(20 + j, L, 1, D), _rand(30 + j, L, 1, D)) for j, L in enumerate(lens)]
    q = _rand(9, sum(q_lens), 8, D)
    O, lse = K.attention_mxfp4_varlen_paged(q.cuda(), _pool(D, kv), [0, 1, 2], list(q_lens), causal=True,
                                            keys_per_split=kps)
    first = 0
    for (k, v), n in zip(kv, q_lens):
        Or, lr = _oracle(q[first:first + n], k, v, True, kps)
        d, dl = O[first:first + n].cpu().double() - Or.double(), (lse[first:first + n].cpu() - lr).abs().max().item()
        err, rel = d.abs().max().item(), (d.norm() / Or.double().norm()).item()
        assert err <= 2e-2 and rel <= 2e-3 and dl <= 1e-4, (k.shape[0], err, rel, dl)
        first += n


ORACLE_COS = {64: (0.6075, 0.9523), 128: (0.5421, 0.9685), 256: (0.4526, 0.8971)}


@pytest.mark.parametrize("D", DIMS)
def test_rotation_helps_on_outlier_channels(D):
    """4 of D channels of q and k are 32 times the rest (HR.outlier_inputs, seed 17), one non-causal query over 449
    keys.  Cosine against float64 attention on the fp16 inputs, from the CPU oracle (plain, rotated): 0.6075, 0.9523
    at D = 64; 0.5421, 0.9685 at 128; 0.4526, 0.8971 at 256.  The rotated pool must pass the midpoint and the plain
    pool's own figure."""
    q, k, v = HR.outlier_inputs(D)
    ref = HR.exact_attention(q, k, v)
    cos = {}
    for had in (False, True):
        O, _ = K.attention_mxfp4_varlen_paged(q.cuda(), _pool(D, [(k, v)], had), [0], [1], keys_per_split=128)
        cos[had] = torch.nn.functional.cosine_similarity(O.cpu().double().flatten(), ref.flatten(), dim=0).item()
    assert cos[True] >= sum(ORACLE_COS[D]) / 2 and cos[True] > cos[False]


@pytest.mark.parametrize("D", DIMS)
def test_decode_step_equals_the_host_planned_pair(D):
    """Eager, then one replay of the captured step, with rope: the step asks the pool, the pair on a twin pool."""
    N, Hq, Hkv, ids = 4, 8, 2, [2, 0, 3]
    kv = [(_rand(40 + j, L, Hkv, D), _rand(50 + j, L, Hkv, D)) for j, L in enumerate((63, 5, 64, 200))]
    cache, twin = _pool(D, kv), _pool(D, kv)
    rope = K.Rope(K.rope_table(208, 10000., "cuda", head_dim=D))
    step = K.DecodeStep(N, 320, Hq, Hkv, "cuda", keys_per_split=128, head_dim=D)
    static = [torch.zeros((N, h, D), dtype=torch.float16, device="cuda") for h in (Hkv, Hkv, Hq)]
    run = lambda: step.append(cache, static[0], static[1], rope=rope).attend(cache, static[2], rope=rope)  # noqa: E731
    graph = None
    for t in range(2):
        [dst.copy_(_rand(60 + 3 * t + i, *dst.shape)) for i, dst in enumerate(static)]
        step.prepare(cache, ids)
        if t == 0:
            O, lse = run()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):   # captured, not run
                run()
        else:
            graph.replay()
        n = len(ids)
        twin.append_packed(static[0][:n], static[1][:n], ids, [1] * n, rope=rope)
        RO, Rl = K.attention_mxfp4_varlen_paged(static[2][:n], twin, ids, [1] * n, causal=True,
                                                keys_per_split=step.kps, rope=rope)
        assert torch.equal(O[:n], RO) and torch.equal(lse[:n], Rl)
        pools = ((*c.kv, c.vtail, c.lens) for c in (cache, twin))
        assert all(torch.equal(x, y) for x, y in zip(*pools))


@pytest.mark.parametrize("D", DIMS)
def test_operators_give_the_python_calls_bits(D):
    """ops.mxfp4_varlen_paged (plain, window + cap, rope), ops.mxfp4_decode_step and, at 128, the verify step."""
    from quantizedattention_amd import ops
    same = lambda a, b: torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])  # noqa: E731
    cache = _pool(D, [(_rand(70 + j, L, 2, D), _rand(80 + j, L, 2, D)) for j, L in enumerate((65, 200))])
    q, rope = _rand(8, 4, 8, D).cuda(), K.Rope(K.rope_table(208, 10000., "cuda", head_dim=D))
    for kw in ({}, dict(window=100, sinks=4, softcap=30.0), dict(rope=rope)):
        args = (q, cache, [0, 1], [3, 1])
        kw = dict(causal=True, keys_per_split=128, **kw)
        assert same(ops.mxfp4_varlen_paged(*args, **kw), K.attention_mxfp4_varlen_paged(*args, **kw)), kw
    k, v = _rand(90, 4, 2, D).cuda(), _rand(91, 4, 2, D).cuda()
    step = K.DecodeStep(2, 320, 8, 2, "cuda", keys_per_split=128, head_dim=D)
    want = step.prepare(cache, [1, 0]).append(cache, k[:2], v[:2]).attend(cache, q[:2])
    assert same(ops.mxfp4_decode_step(q[:2], step, cache), want)
    if D == 128:   # two chained draft tokens per sequence: the step, its operator and the host-planned tree call
        step = K.VerifyStep(2, 320, 8, 2, "cuda", 2, keys_per_split=128)
        want = step.prepare(cache, [1, 0]).append(cache, k, v).attend(cache, q)
        assert same(ops.mxfp4_verify_step(q, step, cache), want)
        assert same(K.attention_mxfp4_varlen_paged(q, cache, [1, 0], [2, 2], causal=True, keys_per_split=128,
                                                   tree=[[-1, 0]] * 2), want)


@pytest.mark.parametrize("what", ["append", "decode_paged", "decode_paged operator", "snapshot"])
@pytest.mark.parametrize("D", DIMS)
def test_refusals_name_hadamard_and_change_nothing(D, what):
    from quantizedattention_amd import ops
    cache = _pool(D, [(_rand(1, 64, 1, D), _rand(2, 64, 1, D))] * 2)
    h = lambda *s: torch.zeros(s, dtype=torch.float16, device="cuda")  # noqa: E731
    call = {"append": lambda: cache.append(h(2, 1, 1, D), h(2, 1, 1, D)),
            "decode_paged": lambda: K.attention_mxfp4_decode_paged(h(2, 8, 1, D), cache),
            "decode_paged operator": lambda: ops.mxfp4_decode_paged(h(2, 8, 1, D), cache),
            "snapshot": lambda: cache.snapshot(0)}[what]
    before = (cache.free_pages, list(cache.lengths), cache.lens.tolist())
    with pytest.raises(QAttnError, match="hadamard"):
        call()
    assert (cache.free_pages, list(cache.lengths), cache.lens.tolist()) == before
