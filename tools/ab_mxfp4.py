"""Time the MX-FP4 forward kernel and its quantisers (dev tool).

    python tools/ab_mxfp4.py [B,H,S,D] [--causal {0,1,2}] [--sq N]

Without --causal the plain entry qattn_mxfp4_attn_fwd is timed; with it, qattn_mxfp4_attn_fwd_ex
with that mask (0 none, 1 top-left, 2 bottom-right).  --sq sets the query tokens (default S, the
key tokens): a chunk against a cache is --causal 2 --sq 128.
"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quantizedattention_amd import _lib  # noqa: E402
from quantizedattention_amd.attention_mxfp4 import (mxfp4_attn_fwd, mxfp4_quantize_rows,  # noqa: E402
                                                    mxfp4_quantize_v)

ap = argparse.ArgumentParser()
ap.add_argument("shape", nargs="?", default="4,32,4096,128")
ap.add_argument("--causal", type=int, choices=(0, 1, 2), default=None)
ap.add_argument("--sq", type=int, default=None)
a = ap.parse_args()
B, H, S, D = (int(x) for x in a.shape.split(","))
Sq = a.sq if a.sq is not None else S
mode = a.causal or 0
g = torch.Generator(device="cuda").manual_seed(0)
q = torch.randn((B, H, Sq, D), device="cuda", generator=g).half()
k = torch.randn((B, H, S, D), device="cuda", generator=g).half()
v = torch.randn((B, H, S, D), device="cuda", generator=g).half()
fwd = (lambda: mxfp4_attn_fwd(q, k, v)) if a.causal is None else (lambda: mxfp4_attn_fwd(q, k, v, causal=mode))
O, lse, (q4, qs, k4, ks, vt, vs) = fwd()
qks = float(torch.tensor(1.0 / math.sqrt(D) * 1.44269504, dtype=torch.float32))
st = _lib.stream_of(q)


def kernel():
    if a.causal is None:
        _lib.call("qattn_mxfp4_attn_fwd", _lib.ptr(q4), _lib.ptr(qs), _lib.ptr(k4), _lib.ptr(ks), _lib.ptr(vt),
                  _lib.ptr(vs), _lib.ptr(O), _lib.ptr(lse), B * H, Sq, S, 1, D, qks, st)
    else:
        _lib.call("qattn_mxfp4_attn_fwd_ex", _lib.ptr(q4), _lib.ptr(qs), _lib.ptr(k4), _lib.ptr(ks),
                  _lib.ptr(vt), _lib.ptr(vs), _lib.ptr(O), _lib.ptr(lse), B * H, Sq, S, 1, mode, D, qks, st)


def timed(f, n=20):
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


tk = timed(kernel)
tq = timed(lambda: (mxfp4_quantize_rows(q), mxfp4_quantize_rows(k), mxfp4_quantize_v(v)))
te = timed(fwd)
# visible (query, key) pairs: all, or those on and below the diagonal of the chosen alignment
qoff = {0: None, 1: 0, 2: S - Sq}[mode]
pairs = Sq * S if qoff is None else sum(min(S, i + qoff + 1) for i in range(Sq))
flop = 4 * B * H * pairs * D
entry = "fwd" if a.causal is None else f"fwd_ex causal={mode}"
print(f"{os.environ.get('QATTN_LIB', 'default')}: mxfp4 {entry} Sq={Sq} Sk={S} kernel {tk * 1e3:.1f} us = "
      f"{flop / tk / 1e9:.0f} TFLOP/s "
      f"({flop / tk / 1e9 / 10066 * 100:.1f}% of the 10.07 PF dense fp4 peak); "
      f"quantisers {tq * 1e3:.1f} us; end-to-end {te * 1e3:.1f} us", flush=True)
