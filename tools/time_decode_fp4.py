"""MX-FP4 KV-cache attention at decode shapes against the one-pass MX-FP4 forward and the int8 cache
(dev tool).  One process; per shape the candidates alternate over PASSES passes of ITERS event-timed
calls each (whole Python call: q quantisation, allocations, kernels); the figure is the median of a
candidate's calls, the spread the range of its per-pass medians.

    python tools/time_decode_fp4.py            # the plan against one pass and int8
    python tools/time_decode_fp4.py --kps      # plus a sweep of keys_per_split (for _split_plan_fp4)

TB/s = cache bytes / time, against the 8 TB/s HBM peak; the caches up to 256 MB may sit in the
Infinity Cache between calls, for every candidate alike.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quantizedattention_amd.attention_mxfp4 import mxfp4_attn_fwd_kv  # noqa: E402
from quantizedattention_amd.kv_cache import attention_int8_cached, quantize_kv  # noqa: E402
from quantizedattention_amd.kv_cache_mxfp4 import (_split_plan_fp4, attention_mxfp4_cached,  # noqa: E402
                                                   quantize_kv_fp4)

SHAPES = [(8, 32, 8, 1, 8192), (8, 32, 8, 32, 8192), (8, 32, 32, 32, 8192), (1, 32, 8, 1, 32768),
          (1, 32, 8, 32, 32768), (4, 32, 32, 128, 8192)]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kps", action="store_true", help="sweep keys_per_split per shape")
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--shapes", type=int, nargs="*", help="indices into SHAPES (default: all)")
    args = ap.parse_args()
    assert args.passes >= 3
    print(f"device {torch.cuda.get_device_name(0)}; {args.passes} alternating passes x {args.iters} calls")
    for idx, (B, Hq, Hkv, Sq, Sk) in enumerate(SHAPES):
        if args.shapes and idx not in args.shapes:
            continue
        g = torch.Generator(device="cuda").manual_seed(0)
        k, v = (torch.randn((B, Hkv, Sk, D), device="cuda", generator=g).half() for _ in range(2))
        q = torch.randn((B, Hq, Sq, D), device="cuda", generator=g).half()
        kv4 = quantize_kv_fp4(k, v)
        bytes4 = sum(t.numel() for t in kv4.kv)
        plan = _split_plan_fp4(B * Hkv, (Hq // Hkv) * Sq, Sk)
        cands = {"fp4 split": lambda: attention_mxfp4_cached(q, kv4)}
        nbytes = {"fp4 split": bytes4}
        if Sq % 32 == 0:
            kv8 = quantize_kv(k, v)
            cands["fp4 one pass"] = lambda: mxfp4_attn_fwd_kv(q, kv4.kv)
            cands["int8 cached"] = lambda: attention_int8_cached(q, kv8)
            nbytes["fp4 one pass"] = bytes4
            nbytes["int8 cached"] = 2 * B * Hkv * Sk * D + 2 * 2 * B * Hkv * Sk // 32
        del k, v
        if args.kps:
            for kps in (256, 512, 1024, 2048, 4096, 8192, Sk):
                if kps <= Sk and kps != plan and f"fp4 kps={kps}" not in cands:
                    cands[f"fp4 kps={kps}"] = (lambda kps=kps: attention_mxfp4_cached(q, kv4, keys_per_split=kps))
                    nbytes[f"fp4 kps={kps}"] = bytes4
        res = alternate(cands, args.passes, args.iters)
        print(f"(B,Hq,Hkv,Sq,Sk)=({B},{Hq},{Hkv},{Sq},{Sk}) plan: {plan} keys per split, "
              f"{-(-Sk // plan)} split(s)")
        for n, (med, pm) in res.items():
            nb = nbytes[n]
            print(f"  {n:14s} {med:8.1f} us  pass medians {min(pm):.1f}..{max(pm):.1f} "
                  f"(spread {(max(pm) - min(pm)) / med:.1%})  cache {nb / 1e6:6.1f} MB  "
                  f"{nb / med / 1e6:5.2f} TB/s ({nb / med / 1e6 / 8:.1%} of 8 TB/s)", flush=True)
        if "fp4 one pass" in res:
            s, o, i8 = res["fp4 split"][0], res["fp4 one pass"][0], res["int8 cached"][0]
            print(f"  split / one pass {s / o:.3f}; split / int8 {s / i8:.3f} (byte ratio "
                  f"{bytes4 / nbytes['int8 cached']:.2f})", flush=True)
        del kv4, q, cands
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
