"""One layer's verify step of speculative decoding over the paged MX-FP4 cache -- K draft tokens for each of N
sequences, append + tree-masked attention -- as the host-planned pair (``append_packed`` +
``attention_mxfp4_varlen_paged(tree=)``), as kv_cache_mxfp4.VerifyStep called eagerly and as VerifyStep.prepare
followed by the replay of a captured graph (dev tool).  The method of tools/time_decode_step.py: one process; the
candidates alternate over PASSES passes of ITERS event-timed whole steps; the figure is the median of a
candidate's steps, the spread the range of its per-pass medians.  Every step, whatever the candidate, ends with the
same roll-back of the lengths (a device copy of ``lens`` and the host mirror), so that every step appends at the
same place; the pages the draft tokens need are reserved by the first step.  Before anything is timed the three
candidates' outputs are compared bit for bit.

    python tools/time_verify_step.py

(a) 8 sequences x 32 / 8 heads at 8192 cached keys, a chain of K = 8.
(b) 64 sequences at 8192 cached keys, a heap tree of 16 nodes (node t under (t - 1) // 2).

Results: DESIGN.md section 5.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from time_decode_ragged import alternate, report  # noqa: E402
from time_decode_varlen import HKV, HQ, P, D, pool_of  # noqa: E402

from quantizedattention_amd.kv_cache_mxfp4 import VerifyStep, attention_mxfp4_varlen_paged  # noqa: E402


def case(name, B, L, parents, rand, passes, iters):
    K = len(parents)
    cache = pool_of([L] * B, rand, extra=K)
    ids, cnt, trees = list(range(B)), [K] * B, [parents] * B
    k, v, q = rand(B * K, HKV, D), rand(B * K, HKV, D), rand(B * K, HQ, D)
    step = VerifyStep(B, cache.alloc.max_pages_per_seq * P, HQ, HKV, "cuda", K, parents=parents)
    saved, lengths = cache.lens.clone(), list(cache.lengths)

    def rollback():
        cache.lengths = list(lengths)
        cache.lens.copy_(saved)

    def host(kps=None):
        cache.append_packed(k, v, ids, cnt)
        out = attention_mxfp4_varlen_paged(q, cache, ids, cnt, causal=True, keys_per_split=kps, tree=trees)
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
    print(f"{name}: {B} x {HQ}/{HKV} heads at {L} cached, P {P}, {K} draft tokens per sequence; the step's "
          f"{step.kps} keys per split, {step.splits} splits, {step.nrb} row blocks: "
          f"{B * step.nrb * step.splits * HKV} workgroups; the three steps bit-equal", flush=True)
    report(alternate({"host-planned pair": host,
                      f"host-planned pair, {step.kps} keys": lambda: host(step.kps),
                      "VerifyStep eager": eager,
                      "prepare + graph replay": replay}, passes, iters))


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
    case("(a) chain of 8", 8, 8192, list(range(-1, 7)), rand, args.passes, args.iters)
    torch.cuda.empty_cache()
    case("(b) tree of 16", 64, 8192, [-1] + [(t - 1) // 2 for t in range(1, 16)], rand, args.passes, args.iters)


if __name__ == "__main__":
    main()
