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

--head-dim 64: the same two shapes with gpt-oss-style heads, 64 query / 8 key-value heads of head_dim 64
(DecodeStep(head_dim=64), the pair ring of csrc/mxfp4_attn_d64.hip over the fixed grid).  Beside the three
candidates: the replay of a graph captured with one tile per ring slot (QATTN_MX64_TPS=1 while it is captured),
and the workaround the step replaces, the replay of a head_dim 128 step on a head_dim 128 pool with q, k, v
zero-padded to 128.  The kernels alone at this head dim: tools/time_decode_varlen.py --head-dim 64.
--head-dim 256: the same two shapes with Gemma-style heads, 16 query / 8 key-value heads of head_dim 256
(DecodeStep(head_dim=256), the ring of csrc/mxfp4_attn_d256.hip over the fixed grid): the three candidates; there is
no padded workaround at this width.  The kernel alone: tools/time_decode_varlen.py --head-dim 256.
--sink: every candidate takes a learned sink logit per query head (``sink_logit``).

Results: DESIGN.md section 5.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from time_decode_ragged import alternate, report  # noqa: E402
from time_decode_varlen import HKV, HQ, P, D, REPS, pool64, pool_of, window_kernel  # noqa: E402

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


def runners(cache, k, v, q, W, S, sink):
    """The candidates of one pool (either head_dim; q [B, Hq, D]) -> (step, host, eager, capture): the host-
    planned pair, the eager step, and ``capture() -> (replay, (O, lse))`` after an eager step has warmed up.
    Every candidate ends with the roll-back of the lengths."""
    B, hq, Dh = q.shape
    ids, ones = list(range(B)), [1] * B
    step = DecodeStep(B, cache.alloc.max_pages_per_seq * P, hq, HKV, "cuda", window=W, sinks=S, head_dim=Dh)
    saved, lengths = cache.lens.clone(), list(cache.lengths)
    win = {} if W is None else {"window": W, "sinks": S}

    def rollback():
        cache.lengths = list(lengths)
        cache.lens.copy_(saved)

    def host(kps=None):
        cache.append_packed(k, v, ids, ones)
        out = attention_mxfp4_varlen_paged(q, cache, ids, ones, causal=True, keys_per_split=kps, sink_logit=sink,
                                           **win)
        rollback()
        return out

    def eager():
        step.prepare(cache, ids)
        out = step.append(cache, k, v).attend(cache, q, sink_logit=sink)
        rollback()
        return out

    def capture():
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = step.append(cache, k, v).attend(cache, q, sink_logit=sink)

        def replay(keep=graph):
            step.prepare(cache, ids)
            keep.replay()
            rollback()
        return replay, out
    return step, host, eager, capture


def case(name, B, L, W, S, rand, passes, iters, Dh=D, use_sink=False):
    hq = {D: HQ, 64: 64, 256: 16}[Dh]
    k, v, q = rand(B, HKV, Dh), rand(B, HKV, Dh), rand(B, hq, Dh)
    sink = rand(hq).float() if use_sink else None
    if Dh == D:
        cache = pool_of([L] * B, rand, extra=1)
    else:
        os.environ["QATTN_MX64_TPS"] = "2"
        kk, vv = rand(L, HKV, Dh), rand(L, HKV, Dh)
        cache = pool64([L] * B, kk, vv, Dh, extra=1)
    step, host, eager, capture = runners(cache, k, v, q, W, S, sink)
    RO, Rl = host(step.kps)
    O, lse = eager()
    assert torch.equal(O, RO) and torch.equal(lse, Rl)
    replay, (gO, glse) = capture()
    gO.zero_()
    replay()
    assert torch.equal(gO, RO) and torch.equal(glse, Rl)
    print(f"{name}: {B} x {hq}/{HKV} heads of head_dim {Dh} at {L} cached, P {P}, window {W} sinks {S}, sink_logit "
          f"{use_sink}; the step's {step.kps} keys per split, {step.splits} splits; the three steps bit-equal",
          flush=True)
    cands = {"host-planned pair": host,
             f"host-planned pair, {step.kps} keys": lambda: host(step.kps),
             "DecodeStep eager": eager,
             "prepare + graph replay": replay}
    if Dh == 64:
        os.environ["QATTN_MX64_TPS"] = "1"   # read at every launch: the captured graph keeps the one-tile kernel
        eager()                              # the one-tile kernel's first launch stays outside the capture
        replay1, (O1, lse1) = capture()
        os.environ["QATTN_MX64_TPS"] = "2"
        O1.zero_()
        replay1()
        assert torch.equal(O1, RO) and torch.equal(lse1, Rl)
        pad = lambda x: torch.nn.functional.pad(x, (0, 64))  # noqa: E731
        wide = pool64([L] * B, kk, vv, 128, extra=1)
        # qk_scale(128) on the padded rows = qk_scale(64)
        _, _, eager128, capture128 = runners(wide, pad(k), pad(v), (pad(q) * 2.0 ** 0.5).half(), W, S, sink)
        O128, _ = eager128()
        print(f"  max |O_64 - O_padded| {(RO.float() - O128[..., :64].float()).abs().max():.3e}", flush=True)
        cands["prepare + graph replay, one tile per slot"] = replay1
        cands["prepare + graph replay, head_dim 128 step on zero-padded inputs"] = capture128()[0]
    report(alternate(cands, passes, iters))
    if Dh != D:
        return
    # the kernels alone, at the lengths after the append
    ids, ones = list(range(B)), [1] * B
    step.prepare(cache, ids)
    step.append(cache, k, v)
    report(alternate({f"host plan's kernel x{REPS}": window_kernel(q, cache, ids, ones, W, S),
                      f"fixed grid's kernel x{REPS}": step_kernel(step, cache, q)}, passes, iters))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--head-dim", type=int, default=128, choices=(64, 128, 256),
                    help="64: 64 / 8 heads of head_dim 64; 256: 16 / 8 heads of head_dim 256")
    ap.add_argument("--sink", action="store_true", help="with a learned sink logit per query head")
    args = ap.parse_args()
    assert args.passes >= 3
    print(f"device {torch.cuda.get_device_name(0)}; {args.passes} alternating passes x {args.iters} steps, "
          "whole step (append + attention + roll-back of the lengths)", flush=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    rand = lambda *s: torch.randn(s, device="cuda", generator=g).half()  # noqa: E731
    case("(a)", 8, 8192, None, 0, rand, args.passes, args.iters, args.head_dim, args.sink)
    torch.cuda.empty_cache()
    case("(d)", 64, 32768, 4096, 4, rand, args.passes, args.iters, args.head_dim, args.sink)


if __name__ == "__main__":
    main()
