"""The paged MX-FP4 cache (kv_cache_mxfp4.PagedKVFP4, attention_mxfp4_decode_paged) against the
preallocated one (PreallocatedKVFP4, attention_mxfp4_decode) at the decode shapes of
``_split_plan_fp4``'s docstring, the same lengths in both (dev tool).  One process; per measurement the
candidates alternate over PASSES passes of ITERS event-timed calls each; the figure is the median of a
candidate's calls, the spread the range of its per-pass medians.

    python tools/time_decode_paged.py

Per shape and page size P in (64, 256), with the pages handed out in ascending order ("identity":
sequence after sequence, page after page) and in a seeded random order ("shuffled"):
1. the whole Python call (q quantisation, allocations, split kernel, merge), which is host-bound at
   these shapes;
2. the split kernel alone: REPS back-to-back launches of the C entry on buffers made once, divided by
   REPS (the kernel's time while it is longer than a launch call).
The outputs are compared bit for bit before anything is timed.  Results: DESIGN.md section 5.
"""
import argparse
import os
import random
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from time_decode_ragged import alternate, report  # noqa: E402

from quantizedattention_amd import _lib  # noqa: E402
from quantizedattention_amd.attention_mxfp4 import _qk_scale, mxfp4_quantize_rows  # noqa: E402
from quantizedattention_amd.kv_cache_mxfp4 import (PagedKVFP4, PreallocatedKVFP4, _decode_plan,  # noqa: E402
                                                   attention_mxfp4_decode, attention_mxfp4_decode_paged)

SHAPES = [(8, 32, 8, 32, 8192), (8, 32, 32, 32, 8192), (1, 32, 8, 32, 32768), (4, 32, 32, 128, 8192),
          (8, 32, 8, 1, 8192)]
PAGES = (64, 256)
D = 128
REPS = 20


def split_launches(q, cache, paged):
    """REPS back-to-back launches of the split entry of ``cache`` on buffers made once."""
    bhv, rows, sk_max, kps, nsplit = _decode_plan(q, cache, False, None, PagedKVFP4 if paged else None)
    B, Hkv, cap, _ = cache.shape
    q4, qs = mxfp4_quantize_rows(q)
    opart = torch.empty((nsplit, bhv * rows, D), dtype=torch.float32, device="cuda")
    ml = torch.empty((nsplit, bhv * rows, 2), dtype=torch.float32, device="cuda")
    head = (_lib.ptr(q4), _lib.ptr(qs), *(_lib.ptr(t) for t in cache.kv), _lib.ptr(opart), _lib.ptr(ml),
            _lib.ptr(cache.lens))
    tail = (sk_max, 0, kps, D, _qk_scale(D), _lib.stream_of(q))
    if paged:
        name = "qattn_mxfp4_attn_fwd_split_paged"
        args = (*head, _lib.ptr(cache.block_table), bhv, Hkv, rows, q.shape[2], cache.num_pages,
                cache.page_tokens, cache.alloc.max_pages_per_seq, *tail)
    else:
        name = "qattn_mxfp4_attn_fwd_split_len"
        args = (*head, bhv, Hkv, rows, q.shape[2], cap, *tail)

    def f(keep=(q4, qs, opart, ml)):
        for _ in range(REPS):
            _lib.call(name, *args)
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--shapes", type=int, nargs="*", default=list(range(len(SHAPES))),
                    help="indices into SHAPES")
    args = ap.parse_args()
    assert args.passes >= 3
    print(f"device {torch.cuda.get_device_name(0)}; {args.passes} alternating passes x {args.iters} calls; "
          f"kernel alone = {REPS} back-to-back launches / {REPS}")
    g = torch.Generator(device="cuda").manual_seed(0)
    rand = lambda *s: torch.randn(s, device="cuda", generator=g).half()  # noqa: E731
    for B, Hq, Hkv, Sq, Sk in (SHAPES[i] for i in args.shapes):
        k, v, q = rand(B, Hkv, Sk, D), rand(B, Hkv, Sk, D), rand(B, Hq, Sq, D)
        pre = PreallocatedKVFP4.allocate(B, Hkv, Sk, "cuda").append(k, v)
        RO, Rl = attention_mxfp4_decode(q, pre)
        for P in PAGES:
            n = B * Sk // P
            caches = {}
            for kind, order in (("identity", None), ("shuffled", random.Random(P).sample(range(n), n))):
                c = PagedKVFP4.allocate(n, P, B, Hkv, Sk // P, "cuda", free_order=order).append(k, v)
                O, lse = attention_mxfp4_decode_paged(q, c)
                assert torch.equal(O, RO) and torch.equal(lse, Rl), (P, kind)
                caches[kind] = c
            print(f" (B,Hq,Hkv,Sq,Sk)=({B},{Hq},{Hkv},{Sq},{Sk}) P={P}: bit-equal to the preallocated decode",
                  flush=True)
            cands = {"preallocated": lambda: attention_mxfp4_decode(q, pre)}
            for kind, c in caches.items():
                cands[f"paged {kind}"] = lambda c=c: attention_mxfp4_decode_paged(q, c)
            print("  whole call")
            report(alternate(cands, args.passes, args.iters))
            cands = {"preallocated": split_launches(q, pre, False)}
            for kind, c in caches.items():
                cands[f"paged {kind}"] = split_launches(q, c, True)
            res = {n_: (med / REPS, [p / REPS for p in pm])
                   for n_, (med, pm) in alternate(cands, args.passes, args.iters).items()}
            print("  the split kernel alone")
            report(res)
            base = res["preallocated"]
            for kind in caches:
                r = res[f"paged {kind}"]
                print(f"  kernel paged {kind} / preallocated {r[0] / base[0]:.3f} "
                      f"(preallocated pass medians within {(max(base[1]) - min(base[1])) / base[0]:.1%})",
                      flush=True)
            del caches, cands, res
            torch.cuda.empty_cache()
        del k, v, q, pre
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
