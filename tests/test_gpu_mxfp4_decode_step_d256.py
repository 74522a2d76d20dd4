"""DecodeStep(head_dim=256) on the GPU, by torch.equal: every listed entry gets what the host-planned pair
(``append_packed``, ``attention_mxfp4_varlen_paged`` at the step's keys per split) gives on a twin pool fed the same
tokens, the pools hold the same bytes, padding rows (two of N = 6 entries) are O = 0, lse = -inf; eager and replayed
from one captured graph while the lengths grow; one step against the CPU oracle."""
import functools

import pytest
import torch

import mxfp4_window_ref as WR
import test_gpu_mxfp4_decode_step_d64 as S64   # its helpers take the head dim: the scattered pool, the rows, the check
from quantizedattention_amd import kv_cache_mxfp4 as K
from test_gpu_mxfp4_decode_step_d64 import LENGTHS, N, SLOTS, WINDOW, _check_step, _sink

pytestmark = pytest.mark.gpu

D = 256


_fill, _rows = functools.partial(S64._fill, D=D), functools.partial(S64._rows, D=D)


# Gemma's group of 2 at one and two key/value heads; 192 keys are three tiles, so a split starts on an odd tile
CASES = [(*pool, *heads, kps, mode) for pool in ((64, 32), (256, 48)) for heads in ((2, 1), (4, 2))
         for kps in (64, 192) for mode in ("plain", "window", "rope", "sink")]


@pytest.mark.parametrize("P,pages,Hq,Hkv,kps,mode", CASES)
def test_three_steps_equal_the_host_planned_pair(P, pages, Hq, Hkv, kps, mode):
    from quantizedattention_amd import ops
    (cache, _), (twin, _) = _fill(Hkv, LENGTHS, P, pages), _fill(Hkv, LENGTHS, P, pages)
    W, S = WINDOW if mode == "window" else (None, 0)
    step = K.DecodeStep(N, 320, Hq, Hkv, "cuda", keys_per_split=kps, window=W, sinks=S, head_dim=D)
    rope = K.Rope(K.rope_table(max(LENGTHS) + 3, 10000., "cuda", head_dim=D)) if mode == "rope" else None
    sink = _sink(Hq) if mode == "sink" else None
    for t in range(3):
        kvq = _rows(Hq, Hkv, 100 + t)
        step.prepare(cache, SLOTS).append(cache, kvq[0], kvq[1], rope=rope)
        got = step.attend(cache, kvq[2], rope=rope, sink_logit=sink)
        _check_step(cache, twin, SLOTS, kvq, got, step.kps, W, S, rope, sink)
    if rope is None:   # the operator allocates its outputs and gives the Python call's bits
        O2, lse2 = ops.mxfp4_decode_step(kvq[2], step, cache, sink_logit=sink)
        assert O2.data_ptr() != got[0].data_ptr() and torch.equal(O2, got[0]) and torch.equal(lse2, got[1])


def test_captured_step_replays_with_window_and_sink():
    Hq, Hkv, lengths, (W, S) = 4, 2, (1, 62, 130, 200), WINDOW
    (cache, _), (twin, _) = _fill(Hkv, lengths, 64, 32), _fill(Hkv, lengths, 64, 32)
    step = K.DecodeStep(N, 320, Hq, Hkv, "cuda", keys_per_split=64, window=W, sinks=S, head_dim=D)
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
def test_step_matches_the_oracle(window):
    # the bars of tests/test_gpu_mxfp4_d256.py; without a window the oracle's is unbounded
    Hq, Hkv, kps, lengths, (W, S) = 4, 2, 128, (63, 129, 64, 200), window or (1 << 25, 0)
    cache, kv = _fill(Hkv, lengths, 64, 32)
    step = K.DecodeStep(N, 320, Hq, Hkv, "cuda", keys_per_split=kps, window=window and W, sinks=S, head_dim=D)
    k, v, q = _rows(Hq, Hkv, 11)
    step.prepare(cache, SLOTS).append(cache, k, v)
    O, lse = (x.cpu().clone() for x in step.attend(cache, q))
    for j, (kj, vj) in enumerate(kv):   # per sequence: q [1, Hq, 1, D], k, v [1, Hkv, L + 1, D]
        k4, v4 = (torch.cat([a, b[j:j + 1].cpu()]).transpose(0, 1)[None] for a, b in ((kj, k), (vj, v)))
        Or, lr, _ = WR.mxfp4_fwd_window(q[j:j + 1].cpu().transpose(0, 1)[None], k4, v4, W, S, kps)
        d, Or = O[j].double() - Or.reshape(Hq, D).double(), Or.double()
        err, rel, dl = d.abs().max().item(), (d.norm() / Or.norm()).item(), (lse[j] - lr.reshape(Hq)).abs().max().item()
        print(f"L={lengths[j] + 1} window={window}: max|dO| {err:.3e} relL2 {rel:.3e} |dlse| {dl:.3e}")
        assert err <= 2e-2 and rel <= 2e-3 and dl <= 1e-4, (lengths[j], err, rel, dl)
