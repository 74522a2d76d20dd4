"""sha256 of what the MX-FP4 cache paths compute, one line per tensor, for a bit-for-bit comparison of two
builds of the whole tree (dev tool): run it in each tree and diff the two outputs.

    python tools/mxfp4_cache_hashes.py > hashes.txt

Per case: O and lse of the five attention paths (attention_mxfp4_cached, _decode, _decode_paged at two
page sizes, _varlen_paged and _varlen_paged with a window) and k4 / ks / vt / vs / vtail / lens after the
padded, the paged and the packed appends.  The cases cover causal and not, ragged lengths, forced and
planned splits and one long batch, (B, Hq, Hkv, Sq, Sk) = (8, 32, 8, 32, 8192): about 10^6 output
elements, enough of them where a product rounded to f16 once and one rounded twice differ.  The caches are
zero-filled before the appends, so every byte of them is determined.

Then the packed path at head_dim 64, 128 and 256 (`packed`): small sequences at page_tokens = 64 and keys_per_split
128 and 192, so that runs of an odd tile count, runs that start on an odd tile and a page crossing inside a pair
slot occur; the packed append plain and with both rope pairings; the packed step non-causal, causal, with a
window and a gap behind the sinks, with a soft cap, merged with and without a sink logit; and the decode step
(plain, windowed, capped, with rope) with a padding entry and sequences that need fewer splits than its grid.
"""
import hashlib
import os
import random
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quantizedattention_amd.kv_cache_mxfp4 import (DecodeStep, PagedKVFP4, PreallocatedKVFP4, Rope,  # noqa: E402
                                                   attention_mxfp4_cached, attention_mxfp4_decode,
                                                   attention_mxfp4_decode_paged,
                                                   attention_mxfp4_varlen_paged, quantize_kv_fp4, rope_table)

D = 128
# name, B, Hq, Hkv, Sq, tokens per sequence after each of the append steps, keys per split
CASES = [
    ("small", 3, 4, 2, 5, [(64, 64, 64), (70, 131, 200)], 64),
    ("even", 2, 8, 4, 40, [(128, 128), (320, 320)], 128),
    ("ragged", 4, 8, 2, 17, [(1, 64, 65, 100), (33, 600, 129, 1000), (40, 601, 130, 1001)], 256),
    ("plan", 2, 32, 8, 1, [(2048, 2048), (2113, 3000)], None),
    ("long", 8, 32, 8, 32, [(8192,) * 8], None),
]


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def show(name: str, **tensors) -> None:
    for k, t in tensors.items():
        print(f"{name} {k} {sha(t)}", flush=True)


def state(name: str, c) -> None:
    show(name, k4=c.k4, ks=c.ks, vt=c.vt, vs=c.vs, vtail=c.vtail, lens=c.lens)


def packed(D: int) -> None:
    """The packed path of one head_dim: two packed appends (the second grows every sequence from the middle of a
    tile), the packed step, the decode step."""
    g = torch.Generator().manual_seed(D)
    rand = lambda *s: torch.randn(s, generator=g).half().cuda()  # noqa: E731
    Hq, Hkv, P, ids = 8, 2, 64, [3, 0, 2, 1]
    steps = [(65, 30, 200, 129), (200, 65, 449, 330)]   # tokens of slots 3, 0, 2, 1 after each append
    sq = [5, 1, 33, 17]
    sink = torch.linspace(-2.0, 3.0, Hq).cuda()
    ropes = {"none": None, "neox": Rope(rope_table(512, 10000., "cuda", head_dim=D)),
             "il": Rope(rope_table(512, 10000., "cuda", head_dim=D), interleaved=True)}
    for rname, rope in ropes.items():
        pool = PagedKVFP4.allocate(32, P, 4, Hkv, 8, "cuda", head_dim=D,
                                   free_order=random.Random(D).sample(range(32), 32))
        done = [0] * 4
        for step in steps:
            cnt = [L - L0 for L, L0 in zip(step, done)]
            pool.append_packed(rand(sum(cnt), Hkv, D), rand(sum(cnt), Hkv, D), ids, cnt, rope=rope)
            done = list(step)
        name = f"packed D={D} rope={rname}"
        state(f"{name} append", pool)
        qp = rand(sum(sq), Hq, D)
        for kps in (128, 192):
            for causal in (False, True):
                O, lse = attention_mxfp4_varlen_paged(qp, pool, ids, sq, causal, kps, rope=rope)
                show(f"{name} varlen kps={kps} causal={int(causal)}", O=O, lse=lse)
            if rope is not None:
                continue
            O, lse = attention_mxfp4_varlen_paged(qp, pool, ids, sq, True, kps, sink_logit=sink)
            show(f"{name} varlen kps={kps} sink", O=O, lse=lse)
            for W, S in ((100, 0), (130, 70)):   # the second: a gap behind two sink tiles in the long sequences
                O, lse = attention_mxfp4_varlen_paged(qp, pool, ids, sq, True, kps, window=W, sinks=S)
                show(f"{name} window kps={kps} W={W} S={S}", O=O, lse=lse)
            O, lse = attention_mxfp4_varlen_paged(qp, pool, ids, sq, True, kps, window=130, sinks=70,
                                                  sink_logit=sink, softcap=30.0)
            show(f"{name} window softcap sink kps={kps}", O=O, lse=lse)
            for causal in (False, True):
                O, lse = attention_mxfp4_varlen_paged(qp, pool, ids, sq, causal, kps, softcap=30.0)
                show(f"{name} softcap kps={kps} causal={int(causal)}", O=O, lse=lse)
        # the decode step: 4 entries for 3 listed slots (the last is padding), a grid sized for 512 keys
        for kps in (128, 192):
            for mode, kw in (("plain", {}), ("window", dict(window=130, sinks=70)), ("softcap", dict(softcap=30.0)),
                             ("window softcap", dict(window=130, sinks=70, softcap=30.0))):
                if rope is not None and mode != "plain":
                    continue
                dec = DecodeStep(4, 512, Hq, Hkv, "cuda", keys_per_split=kps, head_dim=D, **kw)
                for t in range(2):
                    dec.prepare(pool, [2, 0, 1]).append(pool, rand(4, Hkv, D), rand(4, Hkv, D), rope=rope)
                    q = rand(4, Hq, D)
                    for sname, z in (("", None), (" sink", sink)):
                        O, lse = dec.attend(pool, q, rope=rope, sink_logit=z)
                        show(f"{name} decode step {mode}{sname} kps={kps} t={t}", O=O, lse=lse)
        state(f"{name} after the decode steps", pool)
        del pool


def main():
    g = torch.Generator().manual_seed(0)
    rand = lambda *s: torch.randn(s, generator=g).half().cuda()  # noqa: E731
    for name, B, Hq, Hkv, Sq, steps, kps in CASES:
        Sk = max(steps[-1])
        cap = -(-Sk // 1024) * 1024
        k, v, q = rand(B, Hkv, Sk, D), rand(B, Hkv, Sk, D), rand(B, Hq, Sq, D)
        mean = rand(B, Hkv, 1, D) if name == "ragged" else None
        # the counts of every append step, and the padded new tokens of it
        news, done = [], [0] * B
        for lens in steps:
            cnt = [L - L0 for L, L0 in zip(lens, done)]
            n = max(cnt)
            kn, vn = (torch.zeros(B, Hkv, n, D, dtype=torch.float16, device="cuda") for _ in range(2))
            for b, (L0, c) in enumerate(zip(done, cnt)):
                kn[b, :, :c], vn[b, :, :c] = k[b, :, L0:L0 + c], v[b, :, L0:L0 + c]
            news.append((kn, vn, cnt))
            done = list(lens)
        lens = steps[-1]

        if all(L == Sk for L in lens) and Sk % 64 == 0:
            kv = quantize_kv_fp4(k, v, smooth=False)
            for causal in (False, True):
                O, lse = attention_mxfp4_cached(q, kv, causal, kps)
                show(f"{name} cached causal={int(causal)}", O=O, lse=lse)
            del kv

        pre = PreallocatedKVFP4.allocate(B, Hkv, cap, "cuda", k_mean=mean)
        for kn, vn, cnt in news:
            pre.append(kn, vn, counts=cnt)
        state(f"{name} padded append", pre)
        for causal in (False, True):
            O, lse = attention_mxfp4_decode(q, pre, causal, kps)
            show(f"{name} decode causal={int(causal)}", O=O, lse=lse)
        del pre

        for P in (64, 256):
            mpp, npool = cap // P, B * (cap // P)
            order = random.Random(P).sample(range(npool), npool)
            pool = PagedKVFP4.allocate(npool, P, B, Hkv, mpp, "cuda", k_mean=mean, free_order=order)
            for kn, vn, cnt in news:
                pool.append(kn, vn, counts=cnt)
            state(f"{name} paged append P={P}", pool)
            for causal in (False, True):
                O, lse = attention_mxfp4_decode_paged(q, pool, causal, kps)
                show(f"{name} paged P={P} causal={int(causal)}", O=O, lse=lse)
            del pool

            # the packed step: the same tokens appended token-major, the listed slots in reverse order
            pool = PagedKVFP4.allocate(npool, P, B, Hkv, mpp, "cuda", k_mean=mean, free_order=order)
            ids, done = list(range(B))[::-1], [0] * B
            for step in steps:
                cnt = [step[b] - done[b] for b in ids]
                live = [(b, c) for b, c in zip(ids, cnt) if c]
                kp = torch.cat([k[b, :, done[b]:done[b] + c].transpose(0, 1) for b, c in live]).contiguous()
                vp = torch.cat([v[b, :, done[b]:done[b] + c].transpose(0, 1) for b, c in live]).contiguous()
                pool.append_packed(kp, vp, [b for b, _ in live], [c for _, c in live])
                done = list(step)
            state(f"{name} packed append P={P}", pool)
            # ragged query counts: sequence b brings min(Sq + b, L_b) queries
            sq = [min(Sq + b, lens[b]) for b in ids]
            qp = torch.cat([rand(n, Hq, D) for n in sq])
            for causal in (False, True):
                O, lse = attention_mxfp4_varlen_paged(qp, pool, ids, sq, causal, kps)
                show(f"{name} varlen P={P} causal={int(causal)}", O=O, lse=lse)
            for W, S in ((100, 0), (1500, 70)):
                O, lse = attention_mxfp4_varlen_paged(qp, pool, ids, sq, True, kps, window=W, sinks=S)
                show(f"{name} window P={P} W={W} S={S}", O=O, lse=lse)
            del pool
        del k, v, q
        torch.cuda.empty_cache()
    for head_dim in (64, 128, 256):
        packed(head_dim)


if __name__ == "__main__":
    main()
