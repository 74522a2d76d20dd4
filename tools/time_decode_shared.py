"""Shared-prefix attention (kv_cache_mxfp4.attention_mxfp4_varlen_paged(share_prefix=True)) against the
plain packed call on the same pool (dev tool).  The method of tools/time_decode_varlen.py: one process;
per measurement the candidates alternate over PASSES passes of ITERS event-timed whole Python calls
(prefix_groups, plan, uploads, q quantisation, allocations, kernels); the figure is the median of a
candidate's calls, the spread the range of its per-pass medians.  Then the attention kernels alone (REPS
back-to-back launches of the C entry on buffers and tables made once, divided by REPS).  Before anything
is timed the two outputs are compared bit for bit at every keys_per_split that is timed.

    python tools/time_decode_shared.py [--shape 0..3]

Shapes (32 / 8 heads, P = 256, one new token per sequence, causal):
  0  64 forks of a 32768-key prompt, 256 own keys each (key/value bytes by the layout: 43 x fewer)
  1  8 forks of the same prompt
  2  64 forks of a 2048-key prompt, 256 own keys each (sharing may not pay)
  3  one group of 16 forks of an 8192-key prompt beside 16 unrelated decodes over 512 .. 8192 keys
For each: the plain call at its own rule's keys per split (the baseline, unchanged code), the shared call
at plan_varlen_shared's rule, at half of it and at 1024, and the plain call at those three values.
Sharing counts as a win on a shape only when it beats the plain call by more than the spread of the pass
medians.  Results: DESIGN.md section 5.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from time_decode_ragged import alternate, report  # noqa: E402

from quantizedattention_amd import _lib  # noqa: E402
from quantizedattention_amd.attention_mxfp4 import _qk_scale, mxfp4_quantize_rows  # noqa: E402
from quantizedattention_amd.kv_cache_mxfp4 import (PagedKVFP4, attention_mxfp4_varlen_paged, plan_varlen,  # noqa: E402
                                                   plan_varlen_shared)

D, HQ, HKV, P = 128, 32, 8, 256
REPS = 20
# (forks, prompt keys, own keys, unrelated decodes)
SHAPES = [(64, 32768, 256, 0), (8, 32768, 256, 0), (64, 2048, 256, 0), (16, 8192, 256, 16)]


def build(forks, prompt, own, loners, rand):
    """Slot 0 holds the prompt, slots 1 .. forks - 1 are its forks, every one of them then appends ``own``
    tokens; ``loners`` unrelated sequences follow."""
    lone = [512 + (8192 - 512) * i // max(loners - 1, 1) for i in range(loners)]
    B = forks + loners
    pages = prompt // P + forks * -(-own // P) + sum(-(-L // P) for L in lone)
    cache = PagedKVFP4.allocate(pages, P, B, HKV, -(-(max([prompt + own] + lone)) // P), "cuda")
    for t0 in range(0, prompt, 2048):
        n = min(2048, prompt - t0)
        cache.append_packed(rand(n, HKV, D), rand(n, HKV, D), [0], [n])
    for b in range(1, forks):
        cache.fork(0, b)
    ids = list(range(forks))
    cache.append_packed(rand(forks * own, HKV, D), rand(forks * own, HKV, D), ids, [own] * forks)
    for b, L in zip(range(forks, B), lone):
        for t0 in range(0, L, 2048):
            n = min(2048, L - t0)
            cache.append_packed(rand(n, HKV, D), rand(n, HKV, D), [b], [n])
    assert cache.free_pages == 0
    return cache


def kernel_alone(q, cache, ids, q_lens, kps, shared):
    """REPS launches of the attention kernel alone at ``kps``: the shared entry or the plain one."""
    if shared:
        kps, rec, work, rows, grp, mem = plan_varlen_shared(cache.lengths, ids, q_lens, HQ, HKV,
                                                           cache.prefix_groups(ids), kps, True, page_tokens=P)
    else:
        kps, rec, work, rows = plan_varlen(cache.lengths, ids, q_lens, HQ, HKV, kps, True)
        grp, mem = [], []
    dev = [torch.tensor(x, dtype=torch.int32).cuda() for x in (rec, work, grp or [[0] * 4], mem or [[0] * 2])]
    q4, qs = mxfp4_quantize_rows(q)
    opart = torch.empty((rows, D), dtype=torch.float32, device="cuda")
    ml = torch.empty((rows, 2), dtype=torch.float32, device="cuda")
    args = (_lib.ptr(q4), _lib.ptr(qs), *(_lib.ptr(x) for x in cache.kv), _lib.ptr(opart), _lib.ptr(ml),
            _lib.ptr(cache.lens), _lib.ptr(cache.block_table), _lib.ptr(dev[0]), _lib.ptr(dev[1]), len(rec),
            len(work), q.shape[0], rows, cache.alloc.max_seqs, HKV, HQ // HKV, cache.num_pages, P,
            cache.alloc.max_pages_per_seq, 2, kps, D, _qk_scale(D))
    if grp:
        name, tail = "qattn_mxfp4_attn_fwd_varlen_paged_shared", (_lib.ptr(dev[2]), _lib.ptr(dev[3]), len(grp),
                                                                  len(mem), _lib.stream_of(q))
    else:
        name, tail = "qattn_mxfp4_attn_fwd_varlen_paged", (_lib.stream_of(q),)
    print(f"    {'shared' if shared else 'plain'} kernel at {kps}: {len(work)} work records, "
          f"{sum(w[3] for w in work)} of them group records", flush=True)

    def kernel(keep=(q4, qs, opart, ml, dev)):
        for _ in range(REPS):
            _lib.call(name, *args, *tail)
    return kernel


def shape(i, rand, passes, iters):
    forks, prompt, own, loners = SHAPES[i]
    cache = build(forks, prompt, own, loners, rand)
    B = forks + loners
    ids, q_lens = list(range(B)), [1] * B
    q = rand(B, HQ, D)
    groups = cache.prefix_groups(ids)
    rule = plan_varlen_shared(cache.lengths, ids, q_lens, HQ, HKV, groups, None, True, page_tokens=P)[0]
    plain_rule = plan_varlen(cache.lengths, ids, q_lens, HQ, HKV, None, True)[0]
    sweep = [rule, max(64, rule // 2 // 64 * 64), 1024]
    print(f"shape {i}: {forks} forks of a {prompt}-key prompt + {own} own keys, {loners} unrelated decodes; "
          f"groups {[(len(m), c) for m, c in groups]}; shared rule {rule} keys per split, plain rule "
          f"{plain_rule}", flush=True)
    run = lambda kps, share: attention_mxfp4_varlen_paged(q, cache, ids, q_lens, causal=True,  # noqa: E731
                                                          keys_per_split=kps, share_prefix=share)
    for kps in sweep:
        (O, lse), (SO, Slse) = run(kps, False), run(kps, True)
        assert torch.equal(O, SO) and torch.equal(lse, Slse), kps
    print("  bit-equal to the plain call at", sweep, flush=True)
    cands = {f"plain, own rule ({plain_rule})": lambda: run(None, False)}
    for kps in dict.fromkeys(sweep):
        cands[f"shared, {kps}"] = lambda kps=kps: run(kps, True)
        cands[f"plain, {kps}"] = lambda kps=kps: run(kps, False)
    print("  whole call:")
    report(alternate(cands, passes, iters))
    print(f"  kernels alone (x{REPS}):")
    cands = {f"plain kernel, own rule x{REPS}": kernel_alone(q, cache, ids, q_lens, None, False)}
    for kps in dict.fromkeys(sweep):
        cands[f"shared kernel, {kps} x{REPS}"] = kernel_alone(q, cache, ids, q_lens, kps, True)
        cands[f"plain kernel, {kps} x{REPS}"] = kernel_alone(q, cache, ids, q_lens, kps, False)
    report(alternate(cands, passes, iters))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--shape", type=int, default=None, help="one of the shapes 0..3 (default: all)")
    args = ap.parse_args()
    assert args.passes >= 3
    print(f"device {torch.cuda.get_device_name(0)}; {args.passes} alternating passes x {args.iters} calls",
          flush=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    rand = lambda *s: torch.randn(s, device="cuda", generator=g).half()  # noqa: E731
    for i in range(len(SHAPES)) if args.shape is None else [args.shape]:
        shape(i, rand, args.passes, args.iters)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
