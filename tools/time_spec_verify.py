"""Speculative decoding on the paged MX-FP4 cache: the tree-masked verify call
(kv_cache_mxfp4.attention_mxfp4_varlen_paged(tree=)) against the causal packed call on the same pool, and
PagedKVFP4.checkpoint / rollback / accept against append_packed of the same tokens alone (dev tool).  One
process; per measurement the candidates alternate over PASSES passes of ITERS event-timed whole Python calls;
the figure is the median of a candidate's calls, the spread the range of its per-pass medians.

    python tools/time_spec_verify.py [--nodes 16 64]

Per tree size nd (heap trees, parent = (t - 1) // 2): 64 sequences x 32 / 8 heads, P = 256, 8192 cached keys
and the nd draft tokens appended behind them.
(a) verify: the tree call and the causal call (n_j = nd queries per sequence either way; the causal kernel is
    the parent commit's, instruction for instruction), compared first -- the rows of the tree's leftmost chain
    are the causal rows, bit for bit -- then timed as whole calls and as kernels alone (REPS back-to-back
    launches of the C entries on buffers and tables made once, divided by REPS).
(b) rollback: on a pool at 8192 keys with room for the drafts, append_packed of the nd x 64 draft tokens
    followed by a copy of the saved lengths (what a caller without rollback would fake), against
    checkpoint alone, rollback alone (of a pool that stands at the checkpoint), append_packed + rollback and
    append_packed + accept of a depth-4 path + rollback.  The differences are what the extra launch, the
    tails copy and the gather cost.

Results: DESIGN.md section 5.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from time_decode_ragged import alternate, report  # noqa: E402
from time_decode_varlen import pool_of  # noqa: E402

from quantizedattention_amd import _lib  # noqa: E402
from quantizedattention_amd.attention_mxfp4 import _qk_scale, mxfp4_quantize_rows  # noqa: E402
from quantizedattention_amd.kv_cache_mxfp4 import (attention_mxfp4_varlen_paged, plan_varlen,  # noqa: E402
                                                   tree_ancestor_masks, tree_path)

D, HQ, HKV, P = 128, 32, 8, 256
B, CACHED = 64, 8192
REPS = 20


def heap(nd):
    return [(t - 1) // 2 if t else -1 for t in range(nd)]


def kernel_alone(q, cache, ids, q_lens, parents):
    """REPS launches of the attention kernel alone: the tree entry, or with parents None the causal one."""
    nds = None if parents is None else [len(parents)] * len(ids)
    kps, rec, work, rows = plan_varlen(cache.lengths, ids, q_lens, HQ, HKV, None, True, tree_lens=nds)
    rec_d, work_d = (torch.tensor(x, dtype=torch.int32).cuda() for x in (rec, work))
    q4, qs = mxfp4_quantize_rows(q)
    opart = torch.empty((rows, D), dtype=torch.float32, device="cuda")
    ml = torch.empty((rows, 2), dtype=torch.float32, device="cuda")
    args = (_lib.ptr(q4), _lib.ptr(qs), *(_lib.ptr(x) for x in cache.kv), _lib.ptr(opart), _lib.ptr(ml),
            _lib.ptr(cache.lens), _lib.ptr(cache.block_table), _lib.ptr(rec_d), _lib.ptr(work_d), len(rec),
            len(work), q.shape[0], rows, cache.alloc.max_seqs, HKV, HQ // HKV, cache.num_pages, P,
            cache.alloc.max_pages_per_seq, 2, kps, D, _qk_scale(D))
    masks = None
    if parents is not None:
        words = tree_ancestor_masks(parents) * len(ids)      # n_j = nd: every packed token is a node
        masks = torch.tensor([w - (1 << 64) if w >> 63 else w for w in words], dtype=torch.int64).cuda()
    name = "qattn_mxfp4_attn_fwd_varlen_paged" + ("" if parents is None else "_tree")
    tail = (() if parents is None else (_lib.ptr(masks),)) + (_lib.stream_of(q),)
    print(f"  kernel alone, {'causal' if parents is None else 'tree'}: {kps} keys per split, {len(work)} work "
          "records", flush=True)

    def kernel(keep=(q4, qs, opart, ml, rec_d, work_d, masks)):
        for _ in range(REPS):
            _lib.call(name, *args, *tail)
    return kernel


def verify(nd, rand, passes, iters):
    cache = pool_of([CACHED + nd] * B, rand)
    ids, q_lens, parents = list(range(B)), [nd] * B, heap(nd)
    q = rand(B * nd, HQ, D)
    trees = [parents] * B
    O, lse = attention_mxfp4_varlen_paged(q, cache, ids, q_lens, causal=True, tree=trees)
    CO, Cl = attention_mxfp4_varlen_paged(q, cache, ids, q_lens, causal=True)
    chain = torch.arange(min(nd, 2)).cuda()                  # nodes 0 and 1 of a heap see what a causal row sees
    rows = (torch.arange(B).cuda()[:, None] * nd + chain[None]).reshape(-1)
    assert torch.isfinite(lse).all() and torch.equal(O[rows], CO[rows]) and torch.equal(lse[rows], Cl[rows])
    assert not torch.equal(lse, Cl)
    print(f"(a) verify, heap trees of {nd}: {B} sequences x {HQ}/{HKV} heads, {CACHED} cached + {nd} drafts, P {P}; "
          "the causal rows of the tree call are the causal call's", flush=True)
    report(alternate({
        "tree": lambda: attention_mxfp4_varlen_paged(q, cache, ids, q_lens, causal=True, tree=trees),
        "causal": lambda: attention_mxfp4_varlen_paged(q, cache, ids, q_lens, causal=True)}, passes, iters))
    report(alternate({f"tree kernel x{REPS}": kernel_alone(q, cache, ids, q_lens, parents),
                      f"causal kernel x{REPS}": kernel_alone(q, cache, ids, q_lens, None)}, passes, iters))


def rollback(nd, rand, passes, iters):
    # two pools: the faked roll-back keeps the drafts' pages (reserved by its first call, as in
    # time_decode_varlen), the real one gives them back and takes them again every time
    room, fake = pool_of([CACHED] * B, rand, extra=2 * nd), pool_of([CACHED] * B, rand, extra=2 * nd)
    ids, counts = list(range(B)), [nd] * B
    k, v = rand(B * nd, HKV, D), rand(B * nd, HKV, D)
    path = tree_path(heap(nd), min(nd - 1, 14))     # depth 4 (3 for the smallest trees)
    accepted = [path] * B
    saved = fake.lens.clone()
    ckpt = room.checkpoint(ids)

    def faked():
        fake.append_packed(k, v, ids, counts)
        fake.lengths = [CACHED] * B
        fake.lens.copy_(saved)

    def both():
        room.append_packed(k, v, ids, counts)
        room.rollback(ckpt)

    def accept():
        room.append_packed(k, v, ids, counts)
        room.accept(ckpt, k, v, ids, counts, accepted)
        room.rollback(ckpt)

    print(f"(b) rollback, {nd} drafts x {B} sequences at {CACHED} cached; accept keeps {len(path)} tokens each",
          flush=True)
    report(alternate({"append_packed, lens copied": faked, "checkpoint alone": lambda: room.checkpoint(ids),
                      "rollback alone": lambda: room.rollback(ckpt), "append_packed + rollback": both,
                      "append + accept + rollback": accept}, passes, iters))
    assert room.lengths == [CACHED] * B and room.lens.tolist() == room.lengths


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--nodes", type=int, nargs="+", default=[16, 64])
    args = ap.parse_args()
    assert args.passes >= 3 and all(1 <= nd <= 64 for nd in args.nodes)
    print(f"device {torch.cuda.get_device_name(0)}; {args.passes} alternating passes x {args.iters} calls",
          flush=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    rand = lambda *s: torch.randn(s, device="cuda", generator=g).half()  # noqa: E731
    for nd in args.nodes:
        verify(nd, rand, args.passes, args.iters)
        torch.cuda.empty_cache()
        rollback(nd, rand, args.passes, args.iters)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
