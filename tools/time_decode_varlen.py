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

(e) with --head-dim 64 (then only (e) runs): gpt-oss-style heads, 64 query / 8 key-value heads of head_dim 64, at
    three shapes -- 8 decodes at 8192 cached, 64 decodes at 32768 cached under window 128, a 512-token chunk
    beside 15 decodes.  Per shape, kernel alone (REPS launches): the D = 64 kernel with two tiles per ring slot,
    with one (QATTN_MX64_TPS), and today's workaround, the same q, k, v zero-padded to 128 on a D = 128 pool;
    then the whole call with and without ``sink_logit``.

(f) with --head-dim 256 (then only (f) runs): Gemma-style heads, 16 query / 8 key-value heads of head_dim 256, at
    the two decode shapes of (e) with a window of 4096.  Per shape, the kernel alone (REPS launches) with the bytes
    it must read (the visited 64-key tiles at 272 B per key and key/value head) and the fraction of the HBM peak
    (8 TB/s) that makes, then the whole call.

(g) with --softcap C (then only (g) runs): the attention kernel alone (REPS launches) with the logit cap C
    (qattn_mxfp4_attn_fwd_varlen_paged_softcap) beside the uncapped kernel of the same build, alternating, at the two
    decode shapes of (f) and at one 512-token prefill chunk over 8192 cached keys at head_dim 128, 32 / 8 heads.

(h) with --hadamard (then only (h) runs): the two quantisers of a Hadamard-rotated pool beside the plain ones of
    the same build, alternating, at the three shapes of (g): the Q quantiser alone (REPS launches) and the packed
    append's C entry (V, K and length launches; REPS times the entry followed by a copy that puts the lengths back,
    the same copy for both candidates), on pools that differ only in ``hadamard``.

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


def pool64(lengths, k, v, Dp, extra=0, hadamard=False):
    """A pool of head_dim ``Dp`` holding the first ``lengths[j]`` rows of k, v [n, 8, D <= Dp] per sequence, zero-
    padded to ``Dp``, with room for ``extra`` more tokens per sequence."""
    B, n = len(lengths), max(lengths)
    cache = PagedKVFP4.allocate(sum(-(-(L + extra) // P) for L in lengths), P, B, 8, -(-(n + extra) // P), "cuda",
                                head_dim=Dp, hadamard=hadamard)
    pad = lambda x: torch.nn.functional.pad(x, (0, Dp - k.shape[2]))  # noqa: E731
    for t0 in range(0, n, 4096):
        c = [min(max(L - t0, 0), 4096) for L in lengths]
        ids = [j for j in range(B) if c[j]]
        cache.append_packed(torch.cat([pad(k[t0:t0 + c[j]]) for j in ids]), torch.cat([pad(v[t0:t0 + c[j]]) for j in ids]),
                            ids, [c[j] for j in ids])
    return cache


def kernel64(q, cache, q_lens, W, tps, softcap=None):
    """REPS launches of the packed attention kernel alone on ``cache`` (any head_dim); tps: tiles per slot; softcap:
    the capped entry."""
    Dp, ids = cache.shape[3], list(range(len(q_lens)))
    kps, rec, work, rows = plan_varlen(cache.lengths, ids, q_lens, q.shape[1], 8, None, True, W, 0)
    rec_d, work_d = (torch.tensor(x, dtype=torch.int32).cuda() for x in (rec, work))
    q4, qs = mxfp4_quantize_rows(q)
    opart = torch.empty((rows, Dp), dtype=torch.float32, device="cuda")
    ml = torch.empty((rows, 2), dtype=torch.float32, device="cuda")
    args = (_lib.ptr(q4), _lib.ptr(qs), *(_lib.ptr(x) for x in cache.kv), _lib.ptr(opart), _lib.ptr(ml),
            _lib.ptr(cache.lens), _lib.ptr(cache.block_table), _lib.ptr(rec_d), _lib.ptr(work_d), len(rec),
            len(work), q.shape[0], rows, cache.alloc.max_seqs, 8, q.shape[1] // 8, cache.num_pages, P,
            cache.alloc.max_pages_per_seq, 2, kps, Dp, _qk_scale(Dp))
    name = "qattn_mxfp4_attn_fwd_varlen_paged" + ("_softcap" if softcap else "_window" if W else "")
    tail = ((W or 0, 0, softcap) if softcap else (W, 0) if W else ()) + (_lib.stream_of(q),)

    def kernel(keep=(q4, qs, opart, ml, rec_d, work_d)):
        os.environ["QATTN_MX64_TPS"] = str(tps)
        for _ in range(REPS):
            _lib.call(name, *args, *tail)
    return kernel


def d64(rand, passes, iters):
    os.environ["QATTN_MX64_TPS"] = "2"
    shapes = [("8 decodes at 8192 cached", [8192] * 8, [1] * 8, None),
              ("64 decodes at 32768 cached, window 128", [32768] * 64, [1] * 64, 128),
              ("a 512-token chunk + 15 decodes over 512..8192", [8192] + [512 + 7680 * i // 14 for i in range(15)],
               [512] + [1] * 15, None)]
    k, v = rand(32768, 8, 64), rand(32768, 8, 64)
    for name, lengths, q_lens, W in shapes:
        c64, c128 = pool64(lengths, k, v, 64), pool64(lengths, k, v, 128)
        q = rand(sum(q_lens), 64, 64)
        q128 = torch.nn.functional.pad(q, (0, 64)) * (2.0 ** 0.5)   # qk_scale(128) on the padded rows = qk_scale(64)
        ids = list(range(len(lengths)))
        O, _ = attention_mxfp4_varlen_paged(q, c64, ids, q_lens, causal=True, window=W)
        O128, _ = attention_mxfp4_varlen_paged(q128.half(), c128, ids, q_lens, causal=True, window=W)
        print(f"(e) {name}: 64/8 heads, P {P}; max |O_64 - O_padded| {(O.float() - O128[..., :64].float()).abs().max():.3e}",
              flush=True)
        report(alternate({f"D 64, two tiles per slot x{REPS}": kernel64(q, c64, q_lens, W, 2),
                          f"D 64, one tile per slot x{REPS}": kernel64(q, c64, q_lens, W, 1),
                          f"padded to 128 x{REPS}": kernel64(q128.half(), c128, q_lens, W, 2)}, passes, iters))
        os.environ["QATTN_MX64_TPS"] = "2"
        sink = rand(64).float()
        report(alternate({
            "whole call, D 64": lambda: attention_mxfp4_varlen_paged(q, c64, ids, q_lens, causal=True, window=W),
            "whole call, D 64, sink_logit": lambda: attention_mxfp4_varlen_paged(q, c64, ids, q_lens, causal=True,
                                                                                 window=W, sink_logit=sink),
            "whole call, padded to 128": lambda: attention_mxfp4_varlen_paged(q128.half(), c128, ids, q_lens,
                                                                              causal=True, window=W)},
            passes, iters))
        del c64, c128
        torch.cuda.empty_cache()


HBM_PEAK = 8.0e12   # bytes / s


def d256(rand, passes, iters):
    shapes = [("8 decodes at 8192 cached", [8192] * 8, None),
              ("64 decodes at 32768 cached, window 4096", [32768] * 64, 4096)]
    k, v = rand(32768, 8, 256), rand(32768, 8, 256)
    for name, lengths, W in shapes:
        cache, q_lens, ids = pool64(lengths, k, v, 256), [1] * len(lengths), list(range(len(lengths)))
        q = rand(len(lengths), 16, 256)
        # the 64-key tiles a decode query's workgroups visit: all of them, or from the window's first tile on
        tiles = sum(-(-L // 64) - (max(0, L - W) // 64 if W else 0) for L in lengths)
        nbytes = tiles * 64 * 8 * 272
        print(f"(f) {name}: 16/8 heads of head_dim 256, P {P}; {nbytes / 1e6:.1f} MB to read", flush=True)
        res = alternate({f"D 256 kernel x{REPS}": kernel64(q, cache, q_lens, W, 2)}, passes, iters)
        report(res)
        med, pm = next(iter(res.values()))
        print(f"  kernel {med / REPS:.1f} us: {nbytes / (med / REPS * 1e-6) / 1e12:.2f} TB/s, "
              f"{nbytes / (med / REPS * 1e-6) / HBM_PEAK:.1%} of the HBM peak", flush=True)
        report(alternate({"whole call, D 256": lambda: attention_mxfp4_varlen_paged(q, cache, ids, q_lens, causal=True,
                                                                                   window=W)}, passes, iters))
        del cache
        torch.cuda.empty_cache()


def softcapped(cap, rand, passes, iters):
    shapes = [("8 decodes at 8192 cached", 256, 16, [8192] * 8, [1] * 8, None),
              ("64 decodes at 32768 cached, window 4096", 256, 16, [32768] * 64, [1] * 64, 4096),
              ("a 512-token chunk at 8192 cached", 128, 32, [8192], [512], None)]
    for name, Dp, hq, lengths, q_lens, W in shapes:
        cache = pool64(lengths, rand(max(lengths), 8, Dp), rand(max(lengths), 8, Dp), Dp)
        q = rand(sum(q_lens), hq, Dp)
        print(f"(g) {name}: {hq}/8 heads of head_dim {Dp}, P {P}", flush=True)
        report(alternate({f"uncapped kernel x{REPS}": kernel64(q, cache, q_lens, W, 2),
                          f"softcap {cap:g} kernel x{REPS}": kernel64(q, cache, q_lens, W, 2, cap)}, passes, iters))
        del cache
        torch.cuda.empty_cache()


def append_entry(cache, k, v, counts):
    """REPS times the packed append's C entry on ``cache`` (the plain or the rotated one, by the pool), each followed
    by the copy that puts the lengths back.  The first, untimed append here reserves the pages."""
    B, Dp = len(counts), cache.shape[3]
    lengths, saved = list(cache.lengths), cache.lens.clone()
    cache.append_packed(k, v, list(range(B)), counts)
    cache.lengths = list(lengths)
    cache.lens.copy_(saved)
    tab, tiles, first = [], [], 0
    for j, (L, c) in enumerate(zip(lengths, counts)):
        tab += [j, c, first, 0]
        tiles += [x for g in range(L // 64, (L + c - 1) // 64 + 1) for x in (j, g)]
        first += c
    dev = torch.tensor(tab + tiles, dtype=torch.int32).cuda()
    a = cache.alloc
    args = (_lib.ptr(k), _lib.ptr(v), None, *(_lib.ptr(x) for x in cache.kv), _lib.ptr(cache.vtail),
            _lib.ptr(cache.lens), _lib.ptr(cache.block_table), _lib.ptr(dev), _lib.ptr(dev[len(tab):]), B,
            len(tiles) // 2, k.shape[0], a.max_seqs, 8, a.num_pages, P, a.max_pages_per_seq, Dp)
    tail = (None, None, 0, 0) if cache.hadamard else ()
    entry = "qattn_mxfp4_paged_append_packed" + ("_had" if cache.hadamard else "")

    def run(keep=(dev, saved)):
        for _ in range(REPS):
            _lib.call(entry, *args, *tail, _lib.stream_of(k))
            cache.lens.copy_(saved)
    return run


def hadamard(rand, passes, iters):
    shapes = [("8 decodes at 8192 cached", 256, 16, [8192] * 8, [1] * 8),
              ("64 decodes at 32768 cached", 256, 16, [32768] * 64, [1] * 64),
              ("a 512-token chunk at 8192 cached", 128, 32, [8192], [512])]
    for name, Dp, hq, lengths, q_lens in shapes:
        T = sum(q_lens)
        q, k, v = rand(T, hq, Dp), rand(T, 8, Dp), rand(T, 8, Dp)
        q4 = torch.empty((T * hq, Dp // 2), dtype=torch.uint8, device="cuda")
        qs = torch.empty((T * hq, Dp // 32), dtype=torch.uint8, device="cuda")
        st = _lib.stream_of(q)

        def quant(had, keep=(q, q4, qs)):
            for _ in range(REPS):
                if had:
                    _lib.call("qattn_mxfp4_quant_rows_had", _lib.ptr(q), _lib.ptr(q4), _lib.ptr(qs), None, None, T,
                              hq, 0, 0, Dp, st)
                else:
                    _lib.call("qattn_mxfp4_quant_rows", _lib.ptr(q), None, _lib.ptr(q4), _lib.ptr(qs), T * hq, hq,
                              Dp, st)

        print(f"(h) {name}: {hq}/8 heads of head_dim {Dp}, P {P}", flush=True)
        report(alternate({f"plain Q quantiser x{REPS}": lambda: quant(False),
                          f"rotated Q quantiser x{REPS}": lambda: quant(True)}, passes, iters))
        fill = rand(max(lengths), 8, Dp)
        pools = [pool64(lengths, fill, fill, Dp, max(q_lens), h) for h in (False, True)]
        report(alternate({f"plain append entry x{REPS}": append_entry(pools[0], k, v, q_lens),
                          f"rotated append entry x{REPS}": append_entry(pools[1], k, v, q_lens)}, passes, iters))
        del pools
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--window", type=int, default=None, help="run only (d), with this window")
    ap.add_argument("--sinks", type=int, default=0)
    ap.add_argument("--head-dim", type=int, default=128, choices=(64, 128, 256),
                    help="64: run only (e); 256: run only (f)")
    ap.add_argument("--softcap", type=float, default=None, help="run only (g), with this logit cap")
    ap.add_argument("--hadamard", action="store_true", help="run only (h): the rotated quantisers beside the plain")
    args = ap.parse_args()
    assert args.passes >= 3
    print(f"device {torch.cuda.get_device_name(0)}; {args.passes} alternating passes x {args.iters} calls, "
          "whole Python call", flush=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    rand = lambda *s: torch.randn(s, device="cuda", generator=g).half()  # noqa: E731
    if args.hadamard:
        hadamard(rand, args.passes, args.iters)
        return
    if args.softcap is not None:
        softcapped(args.softcap, rand, args.passes, args.iters)
        return
    if args.head_dim == 64:
        d64(rand, args.passes, args.iters)
        return
    if args.head_dim == 256:
        d256(rand, args.passes, args.iters)
        return
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
