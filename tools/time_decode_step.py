"""One layer's decode step over the paged MX-FP4 cache -- one new token for each of N sequences, append +
attention -- as the host-planned pair, as kv_cache_mxfp4.DecodeStep called eagerly and as DecodeStep.prepare
followed by the replay of a captured graph (dev tool).  The method of tools/time_decode_varlen.py: one process;
the candidates alternate over PASSES passes of ITERS event-timed whole steps; the figure is the median of a
candidate's steps, the spread the range of its per-pass medians.  Every step, whatever the candidate, ends with
the same roll-back of the lengths (a device copy of ``lens`` and the host mirror), so that every step appends
at the same place; the pages the new token needs are reserved by the first step.  Before anything is timed the
three candidates' outputs are compared bit for bit.

    python tools/time_decode_step.py

(a) 8 sequences x 32 / 8 heads at 8192 cached keys, causal: case (a) of DESIGN.md section 5.
(d) 64 sequences at 32768 cached keys under window 4096 with 4 sinks: the windowed decode of section 5.

After each case the attention kernels alone: REPS back-to-back launches of the host plan's entry on its tables
and of the fixed grid's entry on the step's, on one pool at the lengths after the append, divided by REPS.

Results: DESIGN.md section 5.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from time_decode_ragged import alternate, report  # noqa: E402
from time_decode_varlen import HKV, HQ, P, D, REPS, pool_of, window_kernel  # noqa: E402

from quantizedattention_amd import _lib  # noqa: E402
from quantizedattention_amd.attention_mxfp4 import _qk_scale, mxfp4_quantize_rows  # noqa: E402
from quantizedattention_amd.kv_cache_mxfp4 import DecodeStep, attention_mxfp4_varlen_paged  # noqa: E402


def step_kernel(step, cache, q):
    """REPS launches of the fixed grid's attention kernel alone, on the tables the step's last append wrote."""
    q4, qs = mxfp4_quantize_rows(q)
    a = cache.alloc
    args = (_lib.ptr(q4), _lib.ptr(qs), *(_lib.ptr(x) for x in cache.kv), _lib.ptr(step.opart), _lib.ptr(step.ml),
            _lib.ptr(cache.lens), _lib.ptr(cache.block_table), _lib.ptr(step.seq_rec), _lib.ptr(step.work), step.N,
            step.splits, a.max_seqs, HKV, HQ // HKV, a.num_pages, a.page_tokens, a.max_pages_per_seq, step.kps, D,
            _qk_scale(D), step.window or 0, step.sinks, _lib.stream_of(q))
    ns = step.seq_rec[:, 3].cpu().tolist()
    print(f"  fixed grid: {step.N} entries x {step.splits} splits x {HKV} heads = {step.N * step.splits * HKV} "
          f"workgroups, {sum(ns) * HKV} of them with work; {step.kps} keys per split", flush=True)

    def kernel(keep=(q4, qs)):
        for _ in range(REPS):
            _lib.call("qattn_mxfp4_attn_fwd_decode_step", *args)
    return kernel


def case(name, B, L, W, S, rand, passes, iters):
    cache = pool_of([L] * B, rand, extra=1)
    ids, ones = list(range(B)), [1] * B
    k, v, q = rand(B, HKV, D), rand(B, HKV, D), rand(B, HQ, D)
    step = DecodeStep(B, cache.alloc.max_pages_per_seq * P, HQ, HKV, "cuda", window=W, sinks=S)
    saved, lengths = cache.lens.clone(), list(cache.lengths)
    win = {} if W is None else {"window": W, "sinks": S}

    def rollback():
        cache.lengths = list(lengths)
        cache.lens.copy_(saved)

    def host(kps=None):
        cache.append_packed(k, v, ids, ones)
        out = attention_mxfp4_varlen_paged(q, cache, ids, ones, causal=True, keys_per_split=kps, **win)
        rollback()
        return out

    def eager():
        step.prepare(cache, ids)
        out = step.append(cache, k, v).attend(cache, q)
        rollback()
        return out

    RO, Rl = host(step.kps)
    O, lse = eager()
    assert torch.equal(O, RO) and torch.equal(lse, Rl)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gO, glse = step.append(cache, k, v).attend(cache, q)

    def replay():
        step.prepare(cache, ids)
        graph.replay()
        rollback()

    gO.zero_()
    replay()
    assert torch.equal(gO, RO) and torch.equal(glse, Rl)
    print(f"{name}: {B} x {HQ}/{HKV} heads at {L} cached, P {P}, window {W} sinks {S}; the step's {step.kps} keys per "
          f"split, {step.splits} splits; the three steps bit-equal", flush=True)
    report(alternate({"host-planned pair": host,
                      f"host-planned pair, {step.kps} keys": lambda: host(step.kps),
                      "DecodeStep eager": eager,
                      "prepare + graph replay": replay}, passes, iters))
    # the kernels alone, at the lengths after the append
    step.prepare(cache, ids)
    step.append(cache, k, v)
    report(alternate({f"host plan's kernel x{REPS}": window_kernel(q, cache, ids, ones, W, S),
                      f"fixed grid's kernel x{REPS}": step_kernel(step, cache, q)}, passes, iters))
    rollback()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    assert args.passes >= 3
    print(f"device {torch.cuda.get_device_name(0)}; {args.passes} alternating passes x {args.iters} steps, "
          "whole step (append + attention + roll-back of the lengths)", flush=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    rand = lambda *s: torch.randn(s, device="cuda", generator=g).half()  # noqa: E731
    case("(a)", 8, 8192, None, 0, rand, args.passes, args.iters)
    torch.cuda.empty_cache()
    case("(d)", 64, 32768, 4096, 4, rand, args.passes, args.iters)


if __name__ == "__main__":
    main()
