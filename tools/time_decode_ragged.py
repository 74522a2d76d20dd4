"""The preallocated MX-FP4 cache (kv_cache_mxfp4.PreallocatedKVFP4, attention_mxfp4_decode) against
the immutable one (QuantizedKVFP4, attention_mxfp4_cached) at decode shapes (dev tool).  One process;
per measurement the candidates alternate over PASSES passes of ITERS event-timed calls each (whole
Python call: q quantisation, allocations, kernels); the figure is the median of a candidate's calls,
the spread the range of its per-pass medians.

    python tools/time_decode_ragged.py

1. equal full lengths: the length-aware forward runs the same tiles as the cached one;
2. mixed lengths: a batch of 8 with lengths 64 .. 8192 beside all-8192 (what the early exit buys);
3. append: one token into a preallocated cache of 8 x 8 heads holding 8192 tokens, beside
   QuantizedKVFP4.append of 64 tokens to a cache of that size (torch.cat: a copy of the whole cache).

Measured on one MI355X (2026-10-20, median us of 3 x 30 alternating calls, range of the pass medians;
two runs agree within 1 us):
  equal full lengths, decode against cached, outputs bit-identical: (8,32,8,1,8192) 46.3 (46.1..47.6)
  against 47.4 (46.8..47.7); (8,32,8,32,8192) 45.8 (44.9..47.3) against 46.8 (46.4..47.8);
  (1,32,8,1,32768) 45.1 (44.7..45.4) against 46.4 (45.8..46.6).  The calls are host-bound (the split
  kernel takes 20.8 us), so the 2-3 % in favour of decode are host work, not the kernel.
  mixed lengths (0.38 of the keys) against all-8192: whole call 45.7 (45.3..45.9) against 45.0
  (44.7..45.2), host-bound; the split kernel alone 16.5 (16.5..16.6) against 20.8 (20.8..20.9): the
  grid is resident at once, so the launch lasts as long as a split of the longest sequence.
  append: one token into the preallocated cache 23.0 (22.0..23.7); QuantizedKVFP4.append of 64 tokens
  at 8192 cached 110.0 (108.6..110.9).
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quantizedattention_amd import _lib  # noqa: E402
from quantizedattention_amd.attention_mxfp4 import _qk_scale, mxfp4_quantize_rows  # noqa: E402
from quantizedattention_amd.kv_cache_mxfp4 import (PreallocatedKVFP4, _decode_plan,  # noqa: E402
                                                   attention_mxfp4_cached, attention_mxfp4_decode,
                                                   quantize_kv_fp4)

SHAPES = [(8, 32, 8, 1, 8192), (8, 32, 8, 32, 8192), (1, 32, 8, 1, 32768)]
MIXED = (64, 512, 1024, 2048, 3072, 4096, 6144, 8192)
D = 128


def timed(f, iters):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        f()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1e3 for a, b in ev]   # us


def alternate(cands, passes, iters):
    """{name: f} -> {name: (median us over all calls, [per-pass medians])}"""
    for f in cands.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    calls = {n: [] for n in cands}
    meds = {n: [] for n in cands}
    for _ in range(passes):
        for n, f in cands.items():
            t = timed(f, iters)
            calls[n] += t
            meds[n].append(statistics.median(t))
    return {n: (statistics.median(calls[n]), meds[n]) for n in cands}


def report(res):
    for n, (med, pm) in res.items():
        print(f"  {n:28s} {med:8.1f} us  pass medians {min(pm):.1f}..{max(pm):.1f} "
              f"(spread {(max(pm) - min(pm)) / med:.1%})", flush=True)


def filled(k, v, cap, lens=None):
    B, Hkv = k.shape[:2]
    cache = PreallocatedKVFP4.allocate(B, Hkv, cap, "cuda")
    return cache.append(k, v, counts=lens)


def split_launches(q, cache, reps):
    """reps back-to-back launches of qattn_mxfp4_attn_fwd_split_len on buffers made once: between two
    events they take reps x the kernel's time while the kernel is longer than a launch call, and the
    host's time per launch otherwise (then the figure is an upper bound of the kernel's)."""
    bhv, rows, sk_max, kps, nsplit = _decode_plan(q, cache, False, None)
    B, Hkv, cap, _ = cache.shape
    q4, qs = mxfp4_quantize_rows(q)
    opart = torch.empty((nsplit, bhv * rows, D), dtype=torch.float32, device="cuda")
    ml = torch.empty((nsplit, bhv * rows, 2), dtype=torch.float32, device="cuda")
    args = (_lib.ptr(q4), _lib.ptr(qs), *(_lib.ptr(t) for t in cache.kv), _lib.ptr(opart), _lib.ptr(ml),
            _lib.ptr(cache.lens), bhv, Hkv, rows, q.shape[2], cap, sk_max, 0, kps, D, _qk_scale(D),
            _lib.stream_of(q))

    def f(keep=(q4, qs, opart, ml)):
        for _ in range(reps):
            _lib.call("qattn_mxfp4_attn_fwd_split_len", *args)
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--iters", type=int, default=30)
    args = ap.parse_args()
    assert args.passes >= 3
    print(f"device {torch.cuda.get_device_name(0)}; {args.passes} alternating passes x {args.iters} calls")
    g = torch.Generator(device="cuda").manual_seed(0)
    rand = lambda *s: torch.randn(s, device="cuda", generator=g).half()  # noqa: E731

    print("1. equal full lengths: decode (length-aware) against cached")
    for B, Hq, Hkv, Sq, Sk in SHAPES:
        k, v, q = rand(B, Hkv, Sk, D), rand(B, Hkv, Sk, D), rand(B, Hq, Sq, D)
        kv4 = quantize_kv_fp4(k, v, smooth=False)
        cache = filled(k, v, Sk)
        del k, v
        O, lse = attention_mxfp4_decode(q, cache)
        O1, l1 = attention_mxfp4_cached(q, kv4)
        print(f" (B,Hq,Hkv,Sq,Sk)=({B},{Hq},{Hkv},{Sq},{Sk}) bit-equal {torch.equal(O, O1) and torch.equal(lse, l1)}")
        res = alternate({"cached": lambda: attention_mxfp4_cached(q, kv4),
                         "decode": lambda: attention_mxfp4_decode(q, cache)}, args.passes, args.iters)
        report(res)
        c, d = res["cached"], res["decode"]
        where = "inside" if min(c[1]) <= d[0] <= max(c[1]) else "outside"
        print(f"  decode / cached {d[0] / c[0]:.3f}; decode {where} the cached candidate's pass medians",
              flush=True)
        del kv4, cache, q
        torch.cuda.empty_cache()

    print(f"2. mixed lengths {MIXED} beside all-8192, (B,Hq,Hkv,Sq)=(8,32,8,1)")
    k, v, q = rand(8, 8, 8192, D), rand(8, 8, 8192, D), rand(8, 32, 1, D)
    full, mixed = filled(k, v, 8192), filled(k, v, 8192, list(MIXED))
    report(alternate({"decode all 8192": lambda: attention_mxfp4_decode(q, full),
                      "decode mixed": lambda: attention_mxfp4_decode(q, mixed)}, args.passes, args.iters))
    print(f"  keys: mixed / full = {sum(MIXED) / (8 * 8192):.3f}")
    reps = 20
    res = alternate({"full": split_launches(q, full, reps), "mixed": split_launches(q, mixed, reps)},
                    args.passes, args.iters)
    print(f"  the split kernel alone, {reps} back-to-back launches / {reps}:")
    report({n: (med / reps, [p / reps for p in pm]) for n, (med, pm) in res.items()})
    del full, mixed
    torch.cuda.empty_cache()

    print("3. append at 8 x 8 heads with 8192 cached")
    total = 3 + args.passes * args.iters
    cache = filled(k, v, 8192 + -(-total // 64) * 64)
    kv4 = quantize_kv_fp4(k, v, smooth=False)
    k1, v1, k64, v64 = rand(8, 8, 1, D), rand(8, 8, 1, D), rand(8, 8, 64, D), rand(8, 8, 64, D)
    report(alternate({"preallocated append 1": lambda: cache.append(k1, v1),
                      "QuantizedKVFP4.append 64": lambda: kv4.append(k64, v64)}, args.passes, args.iters))
    print(f"  lengths after the run {cache.lengths[0]} (device {cache.lens.cpu().tolist()[0]})")


if __name__ == "__main__":
    main()
