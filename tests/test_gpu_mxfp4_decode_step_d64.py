"""DecodeStep(head_dim=64) and attend(sink_logit=) on the GPU, by torch.equal: every listed entry gets what the host-
planned pair (``append_packed``, ``attention_mxfp4_varlen_paged`` at the step's keys per split) gives on a twin pool
fed the same tokens, the pools hold the same bytes, padding rows (two of N = 6 entries) are O = 0, lse = -inf."""
import math

import pytest
import torch

import mxfp4_varlen_helpers as H
import mxfp4_window_ref as WR
from quantizedattention_amd import kv_cache_mxfp4 as K
from quantizedattention_amd._lib import QAttnError

pytestmark = pytest.mark.gpu

N, SLOTS = H.MAX_SEQS, list(H.SLOTS)
LENGTHS = (1, 63, 64, 200)   # 63 -> 64 fills a tile, 64 -> 65 opens a tile (and a page at P = 64)
WINDOW = (70, 3)             # 200 keys leave a gap behind the sink tile, the shorter sequences none
# natural-log units, from below to above the rows' maxima: both branches of M' = max(M, ceil z) occur
_sink = lambda Hq: torch.linspace(-4.0, 6.0, Hq).cuda()  # noqa: E731


def _fill(Hkv, lengths, P, pages, D=64):
    # a scattered pool, sequence j in SLOTS[j] (one packed append) -> (cache, [(k, v) [L, Hkv, D]] on the host)
    g = torch.Generator().manual_seed(31)
    kv = [tuple(torch.randn((L, Hkv, D), generator=g).half() for _ in "kv") for L in lengths]
    cache = K.PagedKVFP4.allocate(pages, P, N, Hkv, -(-320 // P), "cuda", free_order=H.scatter(pages), head_dim=D)
    cache.append_packed(*(torch.cat([x[i] for x in kv]).cuda() for i in (0, 1)), SLOTS, list(lengths))
    return cache, kv


def _rows(Hq, Hkv, seed, D=64):
    g = torch.Generator().manual_seed(seed)   # k, v [N, Hkv, D], q [N, Hq, D]: padding rows hold values too
    return tuple(torch.randn((N, h, D), generator=g).half().cuda() for h in (Hkv, Hkv, Hq))


def _check_step(cache, twin, ids, kvq, got, kps, W=None, S=0, rope=None, sink=None):
    n, (k, v, q), (O, lse) = len(ids), kvq, got   # the step's (O, lse) against the pair on ``twin``, then the pools
    twin.append_packed(k[:n], v[:n], ids, [1] * n, rope=rope)
    RO, Rl = K.attention_mxfp4_varlen_paged(q[:n], twin, ids, [1] * n, causal=True, keys_per_split=kps, window=W,
                                            sinks=S, rope=rope, sink_logit=sink)
    assert O.shape == (N, *q.shape[1:]) and torch.equal(O[:n], RO) and torch.equal(lse[:n], Rl)
    assert not O[n:].any() and bool((lse[n:] == float("-inf")).all())
    assert cache.lengths == twin.lengths == cache.lens.tolist() and cache.alloc.pages == twin.alloc.pages
    for x, y in zip((*cache.kv, cache.vtail, cache.block_table), (*twin.kv, twin.vtail, twin.block_table)):
        assert torch.equal(x, y)


# 192 keys are three tiles: a pair slot ends on a lone tile, the next split starts on an odd tile (two pages at P = 64)
CASES = [(64, *pool, *heads, kps, mode) for pool in ((64, 32), (256, 48)) for heads in ((8, 1), (8, 2))
         for kps in (64, 192) for mode in ("plain", "window", "rope", "sink")]
CASES.append((128, 64, 32, 8, 2, 64, "sink"))   # at head_dim 128 the sink logit is what is new


@pytest.mark.parametrize("D,P,pages,Hq,Hkv,kps,mode", CASES)
def test_three_steps_equal_the_host_planned_pair(D, P, pages, Hq, Hkv, kps, mode):
    from quantizedattention_amd import ops
    (cache, _), (twin, _) = _fill(Hkv, LENGTHS, P, pages, D), _fill(Hkv, LENGTHS, P, pages, D)
    W, S = WINDOW if mode == "window" else (None, 0)
    step = K.DecodeStep(N, 320, Hq, Hkv, "cuda", keys_per_split=kps, window=W, sinks=S, head_dim=D)
    # the table's last row is the last position the three steps reach
    rope = K.Rope(K.rope_table(max(LENGTHS) + 3, 10000., "cuda", head_dim=D)) if mode == "rope" else None
    sink = _sink(Hq) if mode == "sink" else None
    for t in range(3):
        kvq = _rows(Hq, Hkv, 100 + t, D)
        step.prepare(cache, SLOTS).append(cache, kvq[0], kvq[1], rope=rope)
        got = step.attend(cache, kvq[2], rope=rope, sink_logit=sink)
        _check_step(cache, twin, SLOTS, kvq, got, step.kps, W, S, rope, sink)
    if rope is None:   # the operator allocates its outputs and gives the Python call's bits, with and without a sink
        O2, lse2 = ops.mxfp4_decode_step(kvq[2], step, cache, sink_logit=sink)
        assert O2.data_ptr() != got[0].data_ptr() and torch.equal(O2, got[0]) and torch.equal(lse2, got[1])


def test_captured_step_replays_with_window_and_sink():
    Hq, Hkv, lengths, (W, S) = 8, 2, (1, 62, 130, 200), WINDOW
    (cache, _), (twin, _) = _fill(Hkv, lengths, 64, 32), _fill(Hkv, lengths, 64, 32)
    step = K.DecodeStep(N, 320, Hq, Hkv, "cuda", keys_per_split=64, window=W, sinks=S, head_dim=64)
    static, sink = _rows(Hq, Hkv, 1), _sink(Hq)
    run = lambda: step.append(cache, static[0], static[1]).attend(cache, static[2], sink_logit=sink)  # noqa: E731
    step.prepare(cache, SLOTS)
    _check_step(cache, twin, SLOTS, static, run(), step.kps, W, S, None, sink)   # the eager warm-up step
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):   # captured, not run
        got = run()
    for t, ids in enumerate(([4, 0, 5, 2], [0, 1, 2, 4], [1, 0])):
        for c in (cache, twin) if t == 1 else ():   # slot 5 leaves, slot 1 joins with five tokens
            c.free([5])
            c.append_packed(static[0][:5], static[1][:5], [1], [5])
        kvq = _rows(Hq, Hkv, 400 + t)
        step.prepare(cache, ids)
        [dst.copy_(src) for dst, src in zip(static, kvq)]   # into the tensors the graph reads
        graph.replay()
        _check_step(cache, twin, ids, kvq, got, step.kps, W, S, None, sink)
    assert (cache.lengths[0], cache.lengths[5], cache.lengths[1]) == (66, 0, 7)


@pytest.mark.parametrize("window", (None, WINDOW))
def test_step_matches_the_oracle_and_the_sink_formula(window):
    # the bars and the sink formula of tests/test_gpu_mxfp4_d64.py; without a window the oracle's is unbounded
    Hq, Hkv, kps, lengths, (W, S) = 8, 2, 128, (63, 129, 64, 200), window or (1 << 25, 0)
    cache, kv = _fill(Hkv, lengths, 64, 32)
    step = K.DecodeStep(N, 320, Hq, Hkv, "cuda", keys_per_split=kps, window=window and W, sinks=S, head_dim=64)
    k, v, q = _rows(Hq, Hkv, 11)
    step.prepare(cache, SLOTS).append(cache, k, v)
    O, lse = (x.cpu().clone() for x in step.attend(cache, q))
    for j, (kj, vj) in enumerate(kv):   # per sequence: q [1, Hq, 1, D], k, v [1, Hkv, L + 1, D]
        k4, v4 = (torch.cat([a, b[j:j + 1].cpu()]).transpose(0, 1)[None] for a, b in ((kj, k), (vj, v)))
        Or, lr, _ = WR.mxfp4_fwd_window(q[j:j + 1].cpu().transpose(0, 1)[None], k4, v4, W, S, kps)
        d, Or = O[j].double() - Or.reshape(Hq, 64).double(), Or.double()
        err, rel, dl = d.abs().max().item(), (d.norm() / Or.norm()).item(), (lse[j] - lr.reshape(Hq)).abs().max().item()
        assert err <= 2e-2 and rel <= 2e-3 and dl <= 1e-4, (lengths[j], err, rel, dl)
    Os, ls = (x.cpu() for x in step.attend(cache, q, sink_logit=_sink(Hq)))
    wl = torch.log2(torch.exp2(lse[:4].double()) + torch.exp2(_sink(Hq).cpu().double() * math.log2(math.e))[None, :])
    assert (ls[:4].double() - wl).abs().max().item() <= 1e-4
    Ow = O[:4].double() * torch.exp2(lse[:4].double() - wl)[..., None]
    assert ((Os[:4].double() - Ow).abs() <= 2.0 ** -10 * Ow.abs() + 2.0 ** -24).all()
    assert not Os[4:].any() and bool((ls[4:] == float("-inf")).all())


h = lambda *s: torch.zeros(s, dtype=torch.float16, device="cuda")  # noqa: E731
sunk = lambda t: lambda s, c: s.attend(c, h(N, 8, 64), sink_logit=t())  # noqa: E731


@pytest.mark.parametrize("pool_dim,step_dim,error,call", [   # the pool's head_dim, the step's, the error, the call
    (128, 64, K.HeadDimError, lambda s, c: s.prepare(c, SLOTS)),
    (64, 128, K.HeadDimError, lambda s, c: s.prepare(c, SLOTS)), (64, 96, K.HeadDimError, None),
    (64, 64, QAttnError, lambda s, c: s.attend(c, h(N, 8, 128))),
    (64, 64, QAttnError, lambda s, c: s.append(c, h(N, 2, 128), h(N, 2, 128))),
    (64, 64, QAttnError, sunk(lambda: torch.zeros(4, device="cuda"))),   # a sink logit of wrong shape, dtype, device
    (64, 64, QAttnError, sunk(lambda: h(8))), (64, 64, QAttnError, sunk(lambda: torch.zeros(8)))])
def test_refusals_change_nothing(pool_dim, step_dim, error, call):
    cache, _ = _fill(2, LENGTHS, 64, 32, pool_dim)
    before = (cache.free_pages, list(cache.lengths), cache.lens.clone())
    with pytest.raises(error):
        call(K.DecodeStep(N, 320, 8, 2, "cuda", keys_per_split=64, head_dim=step_dim), cache)
    assert (cache.free_pages, list(cache.lengths)) == before[:2] and torch.equal(cache.lens, before[2])
