"""The packed (varlen) step over the paged MX-FP4 cache (kv_cache_mxfp4.attention_mxfp4_varlen_paged,
PagedKVFP4.append_packed) against the padded entries on the same tokens (dev tool).  One process; per
measurement the candidates alternate over PASSES passes of ITERS event-timed whole Python calls (plan,
uploads, q quantisation, allocations, kernels); the figure is the median of a candidate's calls, the
spread the range of its per-pass medians.  In (a) the two outputs are compared bit for bit before
anything is timed (the pools of (b) hold different random tokens).

    python tools/time_decode_varlen.py

(a) uniform: 8 sequences x 32 / 8 heads, 32 new tokens each, 8192 cached, causal: the packed call against
    attention_mxfp4_decode_paged on the same pool -- what the tables and the row mapping cost.
(b) mixed: one causal chunk beside single-token decodes with lengths spread over 512 .. 8192 (MIXED:
    a 2048-token chunk beside 63 decodes, a 512-token chunk beside 15): the packed call at the plan's
    keys per split, at half and at double of it (and at 1024, the rule's floor), against the same work
    as two padded calls on pools of their own (the chunk alone, the decodes alone).
(c) append: append_packed of the mixed batch's new tokens against the padded append, which takes k, v
    [max_seqs, Hkv, longest, D].  Both are followed by the same roll-back of the lengths (a device copy),
    so that every call appends at the same place.

(d) with --window W [--sinks S] (default off; then only (d) runs): a 64-sequence decode batch at 32768 cached
    keys under the window -- the windowed call, the causal call on the same pool, and the causal call on a
    pool whose sequences hold W + 64 tokens (the window's amount of work without the window) -- then the
    three kernels alone, the windowed kernel alone with no sinks and the windowed kernel on the short pool
    with a window of everything (the causal kernel's tiles through the windowed instantiation), and
    free_pages before and after PagedKVFP4.trim of the batch.

After (a) and (b) the packed call is taken apart: the host plan alone (plan_varlen, a host clock), the
two table uploads alone (event-timed) and the attention kernel alone (REPS back-to-back launches of the
C entry on buffers and tables made once, divided by REPS), beside the paged kernel alone in (a).

Results: DESIGN.md section 5.
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from time_decode_ragged import alternate, report  # noqa: E402

from quantizedattention_amd import _lib  # noqa: E402
from quantizedattention_amd.attention_mxfp4 import _qk_scale, mxfp4_quantize_rows  # noqa: E402
from quantizedattention_amd.kv_cache_mxfp4 import (PagedKVFP4, _decode_plan, attention_mxfp4_decode_paged,  # noqa: E402
                                                   attention_mxfp4_varlen_paged, plan_varlen)

D, HQ, HKV, P = 128, 32, 8, 256
MIXED = [(2048, 63), (512, 15)]      # (chunk tokens at 8192 cached, single-token decodes)
REPS = 20


def packed_parts(q, cache, ids, q_lens, kps=None):
    """The packed call taken apart -> {name: f} for ``alternate`` (kernel: REPS launches) after printing
    the host plan's time."""
    t = []
    for _ in range(50):
        t0 = time.perf_counter()
        plan = plan_varlen(cache.lengths, ids, q_lens, HQ, HKV, kps, True)
        t.append((time.perf_counter() - t0) * 1e6)
    kps, rec, work, rows = plan
    print(f"  host plan alone (plan_varlen, {len(work)} work records): median {statistics.median(t):.1f} us",
          flush=True)
    rec_d, work_d = (torch.tensor(x, dtype=torch.int32).cuda() for x in (rec, work))
    q4, qs = mxfp4_quantize_rows(q)
    opart = torch.empty((rows, D), dtype=torch.float32, device="cuda")
    ml = torch.empty((rows, 2), dtype=torch.float32, device="cuda")
    args = (_lib.ptr(q4), _lib.ptr(qs), *(_lib.ptr(x) for x in cache.kv), _lib.ptr(opart), _lib.ptr(ml),
            _lib.ptr(cache.lens), _lib.ptr(cache.block_table), _lib.ptr(rec_d), _lib.ptr(work_d), len(rec),
            len(work), q.shape[0], rows, cache.alloc.max_seqs, HKV, HQ // HKV, cache.num_pages, P,
            cache.alloc.max_pages_per_seq, 2, kps, D, _qk_scale(D), _lib.stream_of(q))

    def kernel(keep=(q4, qs, opart, ml, rec_d, work_d)):
        for _ in range(REPS):
            _lib.call("qattn_mxfp4_attn_fwd_varlen_paged", *args)

    def uploads():
        torch.tensor(rec, dtype=torch.int32).to("cuda", non_blocking=True)
        torch.tensor(work, dtype=torch.int32).to("cuda", non_blocking=True)
    return {f"packed kernel x{REPS}": kernel, "the two uploads": uploads}


def paged_kernel(q, cache):
    bhv, rows, sk_max, kps, nsplit = _decode_plan(q, cache, True, None, PagedKVFP4)
    q4, qs = mxfp4_quantize_rows(q)
    opart = torch.empty((nsplit, bhv * rows, D), dtype=torch.float32, device="cuda")
    ml = torch.empty((nsplit, bhv * rows, 2), dtype=torch.float32, device="cuda")
    args = (_lib.ptr(q4), _lib.ptr(qs), *(_lib.ptr(x) for x in cache.kv), _lib.ptr(opart), _lib.ptr(ml),
            _lib.ptr(cache.lens), _lib.ptr(cache.block_table), bhv, HKV, rows, q.shape[2], cache.num_pages, P,
            cache.alloc.max_pages_per_seq, sk_max, 2, kps, D, _qk_scale(D), _lib.stream_of(q))

    def kernel(keep=(q4, qs, opart, ml)):
        for _ in range(REPS):
            _lib.call("qattn_mxfp4_attn_fwd_split_paged", *args)
    return kernel


def pool_of(lengths, rand, extra=0):
    """A pool holding len(lengths) sequences of those lengths (random tokens), page after page, with
    room for ``extra`` more tokens per sequence."""
    B, n = len(lengths), max(lengths)
    pages = sum(-(-(L + extra) // P) for L in lengths)
    cache = PagedKVFP4.allocate(pages, P, B, HKV, -(-(n + extra) // P), "cuda")
    step = 2048                       # padded appends of at most 2048 tokens at a time
    for t0 in range(0, n, step):
        c = [min(max(L - t0, 0), step) for L in lengths]
        cache.append(rand(B, HKV, max(c), D), rand(B, HKV, max(c), D), counts=c)
    assert cache.lengths == list(lengths)
    return cache


def uniform(rand, passes, iters):
    B, Sq, Sk = 8, 32, 8192
    cache = pool_of([Sk] * B, rand)
    q = rand(B, HQ, Sq, D)
    packed = q.permute(0, 2, 1, 3).reshape(B * Sq, HQ, D).contiguous()
    ids, lens = list(range(B)), [Sq] * B
    kps = plan_varlen(cache.lengths, ids, lens, HQ, HKV)[0]
    PO, Pl = attention_mxfp4_decode_paged(q, cache, causal=True)
    O, lse = attention_mxfp4_varlen_paged(packed, cache, ids, lens, causal=True)
    assert torch.equal(O.view(B, Sq, HQ, D).permute(0, 2, 1, 3), PO)
    assert torch.equal(lse.view(B, Sq, HQ).permute(0, 2, 1).reshape(B * HQ, Sq), Pl)
    print(f"(a) uniform {B} x {HQ}/{HKV} heads, Sq {Sq}, {Sk} cached, causal, P {P}: bit-equal; plan {kps} keys",
          flush=True)
    report(alternate({"paged decode": lambda: attention_mxfp4_decode_paged(q, cache, causal=True),
                      "packed": lambda: attention_mxfp4_varlen_paged(packed, cache, ids, lens, causal=True)},
                     passes, iters))
    parts = packed_parts(packed, cache, ids, lens)
    parts[f"paged kernel x{REPS}"] = paged_kernel(q, cache)
    report(alternate(parts, passes, iters))


def mixed(chunk, ndec, rand, passes, iters):
    lengths = [8192] + [512 + (8192 - 512) * i // max(ndec - 1, 1) for i in range(ndec)]
    B = len(lengths)
    cache = pool_of(lengths, rand)
    q_lens, ids = [chunk] + [1] * ndec, list(range(B))
    q = rand(sum(q_lens), HQ, D)
    # the same work as two padded calls on pools of their own
    pool_c, pool_d = pool_of(lengths[:1], rand), pool_of(lengths[1:], rand)
    q_c = q[:chunk].transpose(0, 1)[None].contiguous()
    q_d = q[chunk:, :, None].contiguous()
    kps = plan_varlen(cache.lengths, ids, q_lens, HQ, HKV)[0]
    print(f"(b) mixed: one {chunk}-token causal chunk at 8192 cached + {ndec} decodes over 512..8192; "
          f"plan {kps} keys per split", flush=True)

    def two_padded():
        attention_mxfp4_decode_paged(q_c, pool_c, causal=True)
        attention_mxfp4_decode_paged(q_d, pool_d, causal=True)

    cands = {"two padded calls": two_padded}
    half, double = max(64, (kps // 2 + 63) // 64 * 64), min(2 * kps, 8192)
    for name, s in (("packed, plan", None), (f"packed, half ({half})", half),
                    (f"packed, double ({double})", double), ("packed, 1024", 1024)):
        cands[name] = lambda s=s: attention_mxfp4_varlen_paged(q, cache, ids, q_lens, causal=True,
                                                               keys_per_split=s)
    report(alternate(cands, passes, iters))
    for s in (None, half):
        print(f"  keys per split {kps if s is None else s}:")
        report(alternate(packed_parts(q, cache, ids, q_lens, s), passes, iters))
    return cache, lengths, q_lens


def append(lengths, counts, rand, passes, iters):
    B, n = len(lengths), max(counts)
    room = pool_of(lengths, rand, extra=n)            # pages for the append reserved on the first call
    pk, pv = rand(sum(counts), HKV, D), rand(sum(counts), HKV, D)
    dk, dv = rand(B, HKV, n, D), rand(B, HKV, n, D)
    saved = room.lens.clone()
    ids = list(range(B))

    def rollback():
        room.lengths = list(lengths)
        room.lens.copy_(saved)

    def packed():
        room.append_packed(pk, pv, ids, counts)
        rollback()

    def padded():
        room.append(dk, dv, counts=counts)
        rollback()

    print(f"(c) append of {sum(counts)} packed tokens ({B} sequences, longest {n}) against the padded "
          f"[{B}, {HKV}, {n}, {D}]", flush=True)
    report(alternate({"padded append": padded, "append_packed": packed}, passes, iters))


def window_kernel(q, cache, ids, q_lens, W, S):
    """REPS launches of the attention kernel alone: the windowed entry, or with W None the causal one."""
    kps, rec, work, rows = plan_varlen(cache.lengths, ids, q_lens, HQ, HKV, None, True, W, S if W else 0)
    rec_d, work_d = (torch.tensor(x, dtype=torch.int32).cuda() for x in (rec, work))
    q4, qs = mxfp4_quantize_rows(q)
    opart = torch.empty((rows, D), dtype=torch.float32, device="cuda")
    ml = torch.empty((rows, 2), dtype=torch.float32, device="cuda")
    args = (_lib.ptr(q4), _lib.ptr(qs), *(_lib.ptr(x) for x in cache.kv), _lib.ptr(opart), _lib.ptr(ml),
            _lib.ptr(cache.lens), _lib.ptr(cache.block_table), _lib.ptr(rec_d), _lib.ptr(work_d), len(rec),
            len(work), q.shape[0], rows, cache.alloc.max_seqs, HKV, HQ // HKV, cache.num_pages, P,
            cache.alloc.max_pages_per_seq, 2, kps, D, _qk_scale(D))
    name = "qattn_mxfp4_attn_fwd_varlen_paged" + ("_window" if W else "")
    tail = ((W, S) if W else ()) + (_lib.stream_of(q),)
    print(f"  kernel alone, window {W} sinks {S}: {kps} keys per split, {len(work)} work records", flush=True)

    def kernel(keep=(q4, qs, opart, ml, rec_d, work_d)):
        for _ in range(REPS):
            _lib.call(name, *args, *tail)
    return kernel


def windowed(W, S, rand, passes, iters):
    B, L = 64, 32768
    cache, short = pool_of([L] * B, rand), pool_of([W + 64] * B, rand)
    q, ids, lens = rand(B, HQ, D), list(range(B)), [1] * B
    print(f"(d) window {W}, sinks {S}: {B} decodes x {HQ}/{HKV} heads at {L} cached, P {P}", flush=True)
    report(alternate({
        "windowed": lambda: attention_mxfp4_varlen_paged(q, cache, ids, lens, causal=True, window=W, sinks=S),
        "causal, same pool": lambda: attention_mxfp4_varlen_paged(q, cache, ids, lens, causal=True),
        f"causal, {W + 64} cached": lambda: attention_mxfp4_varlen_paged(q, short, ids, lens, causal=True),
    }, passes, iters))
    report(alternate({f"windowed kernel x{REPS}": window_kernel(q, cache, ids, lens, W, S),
                      f"windowed kernel, no sinks x{REPS}": window_kernel(q, cache, ids, lens, W, 0),
                      f"causal kernel x{REPS}": window_kernel(q, cache, ids, lens, None, 0),
                      f"causal kernel, {W + 64} cached x{REPS}": window_kernel(q, short, ids, lens, None, 0),
                      # the same tiles as the line above through the windowed instantiation: what its code costs
                      f"windowed kernel, {W + 64} cached x{REPS}": window_kernel(q, short, ids, lens, W + 64, 0)},
                     passes, iters))
    before = cache.free_pages
    freed = cache.trim(ids, W, S)
    print(f"  trim: free_pages {before} -> {cache.free_pages} of {cache.num_pages} ({freed} returned)", flush=True)
    O1, _ = attention_mxfp4_varlen_paged(q, cache, ids, lens, causal=True, window=W, sinks=S)
    assert torch.isfinite(O1.float()).all()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--window", type=int, default=None, help="run only (d), with this window")
    ap.add_argument("--sinks", type=int, default=0)
    args = ap.parse_args()
    assert args.passes >= 3
    print(f"device {torch.cuda.get_device_name(0)}; {args.passes} alternating passes x {args.iters} calls, "
          "whole Python call", flush=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    rand = lambda *s: torch.randn(s, device="cuda", generator=g).half()  # noqa: E731
    if args.window is not None:
        windowed(args.window, args.sinks, rand, args.passes, args.iters)
        return
    uniform(rand, args.passes, args.iters)
    torch.cuda.empty_cache()
    for i, (chunk, ndec) in enumerate(MIXED):
        cache, lengths, q_lens = mixed(chunk, ndec, rand, args.passes, args.iters)
        if i == 0:
            append(lengths, q_lens, rand, args.passes, args.iters)
        del cache
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
