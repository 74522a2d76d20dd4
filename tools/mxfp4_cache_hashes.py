"""sha256 of what the MX-FP4 cache paths compute, one line per tensor, for a bit-for-bit comparison of two
builds of the whole tree (dev tool): run it in each tree and diff the two outputs.

    python tools/mxfp4_cache_hashes.py > hashes.txt

Per case: O and lse of the five attention paths (attention_mxfp4_cached, _decode, _decode_paged at two
page sizes, _varlen_paged and _varlen_paged with a window) and k4 / ks / vt / vs / vtail / lens after the
padded, the paged and the packed appends.  The cases cover causal and not, ragged lengths, forced and
planned splits and one long batch, (B, Hq, Hkv, Sq, Sk) = (8, 32, 8, 32, 8192): about 10^6 output
elements, enough of them where a product rounded to f16 once and one rounded twice differ.  The caches are
zero-filled before the appends, so every byte of them is determined.
"""
import hashlib
import os
import random
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quantizedattention_amd.kv_cache_mxfp4 import (PagedKVFP4, PreallocatedKVFP4,  # noqa: E402
                                                   attention_mxfp4_cached, attention_mxfp4_decode,
                                                   attention_mxfp4_decode_paged,
                                                   attention_mxfp4_varlen_paged, quantize_kv_fp4)

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


if __name__ == "__main__":
    main()
