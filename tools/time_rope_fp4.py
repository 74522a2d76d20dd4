"""One layer's packed step over the paged MX-FP4 cache with rotary positions, two ways (dev tool): the
rotation as separate torch operations on q and k followed by append_packed and
attention_mxfp4_varlen_paged (what a caller did before rope=), against the same two calls with rope=.
One process; per shape the candidates alternate over PASSES passes of ITERS event-timed steps each (whole
Python calls: the rotation or the position upload, the plans, allocations, kernels); the figure is the
median of a candidate's steps, the spread the range of its per-pass medians.  After every step the pool
is rolled back outside the timed window, so every step sees the same lengths.

    python tools/time_rope_fp4.py                 # the three shapes, NeoX pairing
    python tools/time_rope_fp4.py --interleaved

Candidates: "unfused" (positions already on the device, as a model holds them), "fused" (default positions
from the pool's host mirror, uploaded with the records) and "fused dev" (the same device positions as the
unfused one).  Before timing, the three are held to one another bit for bit on O and lse.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quantizedattention_amd.kv_cache_mxfp4 import (PagedKVFP4, Rope, attention_mxfp4_varlen_paged,  # noqa: E402
                                                   rope_positions, rope_table)

# (sequences, Hq, Hkv, cached tokens, new tokens per sequence)
SHAPES = [(8, 32, 8, 8192, 1), (8, 32, 8, 8192, 32), (1, 32, 8, 0, 2048)]
D, P = 128, 256


def rotate(x, table, pos, interleaved):
    """rope_ref's operations (tests/mxfp4_rope_ref.py) on the device: x fp16 [T, H, 128] -> fp16."""
    rows = table.index_select(0, pos)
    c, s = rows[:, None, :D // 2], rows[:, None, D // 2:]
    if interleaved:
        a, b = x[..., 0::2].float(), x[..., 1::2].float()
        return torch.stack([(a * c - b * s).half(), (b * c + a * s).half()], -1).reshape(x.shape)
    a, b = x[..., :D // 2].float(), x[..., D // 2:].float()
    return torch.cat([(a * c - b * s).half(), (b * c + a * s).half()], -1)


def timed(step, undo, iters):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        step()
        b.record()
        undo()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1e3 for a, b in ev]   # us


def alternate(cands, undo, passes, iters):
    """{name: step} -> {name: (median us over all steps, [per-pass medians])}"""
    for f in cands.values():
        for _ in range(3):
            f()
            undo()
    torch.cuda.synchronize()
    calls = {n: [] for n in cands}
    meds = {n: [] for n in cands}
    for _ in range(passes):
        for n, f in cands.items():
            t = timed(f, undo, iters)
            calls[n] += t
            meds[n].append(statistics.median(t))
    return {n: (statistics.median(calls[n]), meds[n]) for n in cands}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--interleaved", action="store_true", help="GPT-J pairing (default: NeoX)")
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--shapes", type=int, nargs="*", help="indices into SHAPES (default: all)")
    args = ap.parse_args()
    assert args.passes >= 3
    assert torch.cuda.is_available(), "this tool times the GPU; there is nothing to measure without one"
    il = args.interleaved
    print(f"device {torch.cuda.get_device_name(0)}; {args.passes} alternating passes x {args.iters} steps; "
          f"{'interleaved' if il else 'NeoX'} pairing")
    for idx, (B, Hq, Hkv, L, n) in enumerate(SHAPES):
        if args.shapes and idx not in args.shapes:
            continue
        g = torch.Generator(device="cuda").manual_seed(0)
        rand = lambda *s: torch.randn(s, device="cuda", generator=g).half()  # noqa: E731
        mpp = -(-(L + n) // P)
        cache = PagedKVFP4.allocate(B * mpp, P, B, Hkv, mpp, "cuda")
        ids, counts = list(range(B)), [n] * B
        rope = Rope(rope_table(L + n, device="cuda"), il)
        if L:
            cache.append_packed(rand(B * L, Hkv, D), rand(B * L, Hkv, D), ids, [L] * B, rope=rope)
        q, k, v = rand(B * n, Hq, D), rand(B * n, Hkv, D), rand(B * n, Hkv, D)
        pos_d = torch.tensor(rope_positions(cache.lengths, ids, counts), dtype=torch.int32).cuda()
        pos_l = pos_d.long()
        ckpt = cache.checkpoint(ids)
        out = {}

        def unfused():
            cache.append_packed(rotate(k, rope.table, pos_l, il), v, ids, counts)
            out["unfused"] = attention_mxfp4_varlen_paged(rotate(q, rope.table, pos_l, il), cache, ids, counts,
                                                          causal=True)

        def fused():
            cache.append_packed(k, v, ids, counts, rope=rope)
            out["fused"] = attention_mxfp4_varlen_paged(q, cache, ids, counts, causal=True, rope=rope)

        def fused_dev():
            cache.append_packed(k, v, ids, counts, rope=rope, positions=pos_d)
            out["fused dev"] = attention_mxfp4_varlen_paged(q, cache, ids, counts, causal=True, rope=rope,
                                                            positions=pos_d)

        cands = {"unfused": unfused, "fused": fused, "fused dev": fused_dev}
        undo = lambda: cache.rollback(ckpt)  # noqa: E731
        for f in cands.values():
            f()
            undo()
        torch.cuda.synchronize()
        same = all(torch.equal(out["unfused"][i], out[c][i]) for c in ("fused", "fused dev") for i in (0, 1))
        assert same, "the fused step does not give the unfused step's bits"
        res = alternate(cands, undo, args.passes, args.iters)
        print(f"(seqs,Hq,Hkv,cached,new)=({B},{Hq},{Hkv},{L},{n}) O and lse bit-identical across the candidates")
        for name, (med, pm) in res.items():
            print(f"  {name:10s} {med:8.1f} us  pass medians {min(pm):.1f}..{max(pm):.1f} "
                  f"(spread {(max(pm) - min(pm)) / med:.1%})", flush=True)
        u = res["unfused"][0]
        print(f"  fused / unfused {res['fused'][0] / u:.3f}; fused dev / unfused {res['fused dev'][0] / u:.3f}",
              flush=True)
        del cache, q, k, v, cands, ckpt
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
