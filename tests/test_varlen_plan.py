"""The host plan of the packed (varlen) step, kv_cache_mxfp4.plan_varlen: pure Python, no device.

Held on hand-written batches and on seeded random ones (nseq 1..12, q_lens 1..300, lengths 1..5000, G
in {1, 2, 4, 8}, keys per split None / 64 / 1024): the work list holds every (sequence, row block,
split < ns_j) once and nothing else, the partial blocks tile [0, part_rows) without a gap, ns_j is
ceil(ceil64(L_j) / kps), the planned kps is the library's rule at the call's real workgroup count,
every error of the contract raises, and the order of ``seq_ids`` changes nothing but the bases.
"""
import random
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "quantizedattention_amd" / "libqattn.so"
needs_lib = pytest.mark.skipif(not LIB.exists(), reason="libqattn.so not built (run __graft_entry__.build())")

# (lengths per slot, seq_ids, q_lens, Hq, Hkv)
HAND = [
    ([7], [0], [1], 4, 4),
    ([0, 1, 0, 63, 65, 200], [1, 3, 4, 5], [1, 3, 33, 70], 4, 2),
    ([64, 130, 256, 70, 0, 0], [3, 0, 2, 1], [70, 1, 33, 3], 4, 4),
    ([8192] + [512 + 120 * i for i in range(63)], list(range(64)), [2048] + [1] * 63, 32, 8),
    ([5000, 1, 4999], [2, 0], [300, 129], 8, 1),
    ([1024, 1025, 1023], [0, 1, 2], [128, 129, 127], 2, 2),
]


def _random_batches(count, seed):
    rng = random.Random(seed)
    for _ in range(count):
        slots = rng.randint(1, 16)
        nseq = rng.randint(1, min(12, slots))
        lengths = [rng.choice((0, rng.randint(1, 5000))) for _ in range(slots)]
        ids = rng.sample(range(slots), nseq)
        for b in ids:
            lengths[b] = rng.choice((1, 63, 64, 65, rng.randint(1, 5000)))
        Hkv = rng.choice((1, 2, 4))
        yield lengths, ids, [rng.randint(1, 300) for _ in ids], Hkv * rng.choice((1, 2, 4, 8)), Hkv


BATCHES = HAND + list(_random_batches(300, 5))


def _ceil64(n):
    return -(-n // 64) * 64


def _check(batch, kps_in):
    from quantizedattention_amd.kv_cache_mxfp4 import plan_varlen
    lengths, ids, q_lens, Hq, Hkv = batch
    kps, seq_rec, work, part_rows = plan_varlen(lengths, ids, q_lens, Hq, Hkv, kps_in)
    G = Hq // Hkv
    assert kps % 64 == 0 and kps >= 64
    if kps_in is not None:
        assert kps == min(kps_in, _ceil64(max(lengths[b] for b in ids)))
    assert len(seq_rec) == len(ids)
    first, blocks, expect = 0, [], set()
    for j, (rec, b, n) in enumerate(zip(seq_rec, ids, q_lens)):
        assert len(rec) == 8 and rec[5:] == [0, 0, 0]
        ns = -(-_ceil64(lengths[b]) // kps)
        assert rec[:4] == [b, first, n, ns], (j, rec)
        blocks.append((rec[4], rec[4] + ns * Hkv * G * n))
        expect |= {(j, rb, s) for rb in range(-(-G * n // 128)) for s in range(ns)}
        first += n
    # the partial blocks: disjoint and dense in [0, part_rows)
    blocks.sort()
    assert blocks[0][0] == 0 and blocks[-1][1] == part_rows
    assert all(a[1] == b[0] for a, b in zip(blocks, blocks[1:]))
    # the work list: every (j, row block, split) once, nothing else, longest first
    assert all(len(w) == 4 and w[3] == 0 for w in work)
    got = [tuple(w[:3]) for w in work]
    assert len(got) == len(set(got)) and set(got) == expect
    tiles = [min(-(-lengths[ids[j]] // 64), (s + 1) * (kps // 64)) - s * (kps // 64) for j, _, s in got]
    assert all(t >= 1 for t in tiles) and tiles == sorted(tiles, reverse=True)
    return kps, seq_rec, work, part_rows


@pytest.mark.parametrize("kps", [64, 1024])
def test_plan_given_split(kps):
    for batch in BATCHES:
        _check(batch, kps)


@needs_lib
def test_plan_none_is_the_library_rule():
    from quantizedattention_amd import _lib
    lib = _lib.load()
    for batch in BATCHES:
        lengths, ids, q_lens, Hq, Hkv = batch
        kps, _, _, _ = _check(batch, None)
        W = Hkv * sum(-(-(Hq // Hkv) * n // 128) for n in q_lens)
        sk_max = _ceil64(max(lengths[b] for b in ids))
        assert kps == min(lib.qattn_split_keys(W, 1, sk_max, 64), sk_max)
        assert lib.qattn_split_keys(W, 1, sk_max, 64) <= sk_max
    # the mixed batch (one 2048-token chunk beside 63 decodes): 8 * (64 + 63) = 1016 workgroups are more
    # than the rule's 512, so it does not split; a lone decode over 8192 keys splits at the 1024-key floor
    assert _check(HAND[3], None)[0] == 8192
    assert _check(([8192], [0], [1], 32, 8), None)[0] == 1024


def test_partials_are_compact():
    """One long sequence beside a large chunk: each pays for its own splits only."""
    lengths, ids, q_lens, Hq, Hkv = [65536, 64], [0, 1], [1, 2048], 32, 8
    _, seq_rec, work, part_rows = _check((lengths, ids, q_lens, Hq, Hkv), 1024)
    assert [r[3] for r in seq_rec] == [64, 1]
    assert part_rows == 64 * 32 * 1 + 1 * 32 * 2048            # not 64 * 32 * 2049
    assert len(work) == 64 + 2048 * 4 // 128


def test_shuffled_order_gives_the_same_records():
    from quantizedattention_amd.kv_cache_mxfp4 import plan_varlen
    rng = random.Random(9)
    for lengths, ids, q_lens, Hq, Hkv in BATCHES[:60]:
        kps, rec, work, rows = plan_varlen(lengths, ids, q_lens, Hq, Hkv, 1024)
        perm = list(range(len(ids)))
        rng.shuffle(perm)
        kps2, rec2, work2, rows2 = plan_varlen(lengths, [ids[p] for p in perm], [q_lens[p] for p in perm],
                                               Hq, Hkv, 1024)
        assert (kps2, rows2, len(work2)) == (kps, rows, len(work))
        by_slot = {r[0]: (r[2], r[3]) for r in rec}
        assert {r[0]: (r[2], r[3]) for r in rec2} == by_slot       # all but the two bases
        per_seq = lambda recs, ws: sorted((recs[w[0]][0], w[1], w[2]) for w in ws)  # noqa: E731
        assert per_seq(rec, work) == per_seq(rec2, work2)


def test_errors():
    from quantizedattention_amd import _lib
    from quantizedattention_amd.kv_cache_mxfp4 import plan_varlen
    lengths = [10, 0, 200, 64]
    bad = [
        (([2, 1], [1, 1], 4, 2, 64), "at least one cached token"),       # a listed slot of length 0
        (([0, 2], [11, 3], 4, 2, 64, True), "causal"),                   # q_lens > L, causal
        (([0, 0], [1, 1], 4, 2, 64), "distinct"),
        (([0, 4], [1, 1], 4, 2, 64), "distinct"),                        # out of range
        (([-1], [1], 4, 2, 64), "distinct"),
        (([], [], 4, 2, 64), "nseq >= 1"),
        (([0, 2], [1], 4, 2, 64), "nseq >= 1"),
        (([0], [0], 4, 2, 64), ">= 1"),
        (([0], [1], 3, 2, 64), "heads"),
        (([0], [1], 4, 2, 96), "keys_per_split"),
        (([0], [1], 4, 2, 0), "keys_per_split"),
        (([0], [1], 4, 2, 32), "keys_per_split"),
    ]
    for args, match in bad:
        with pytest.raises(_lib.QAttnError, match=match):
            plan_varlen(lengths, *args)
    # not causal: q_lens may pass the length; an unlisted empty slot is nobody's business
    plan_varlen(lengths, [0, 2], [11, 3], 4, 2, 64)
    # 2^31 packed rows / partial rows are refused, not wrapped
    with pytest.raises(_lib.QAttnError, match="2\\^31"):
        plan_varlen([64], [0], [1 << 24], 128, 1, 64)
    with pytest.raises(_lib.QAttnError, match="2\\^31"):
        plan_varlen([1 << 25], [0], [1 << 13], 1, 1, 64)      # 2^19 splits x 2^13 rows


def test_entry_errors_raise_before_any_tensor(monkeypatch):
    """attention_mxfp4_varlen_paged and append_packed on CPU tensors: every contract error raises
    before a tensor is made or moved (torch.tensor / torch.empty are trapped)."""
    import torch

    from quantizedattention_amd import _lib
    from quantizedattention_amd.kv_cache_mxfp4 import PageAllocator, PagedKVFP4, attention_mxfp4_varlen_paged
    z = lambda *s, dt=torch.uint8: torch.zeros(s, dtype=dt)  # noqa: E731
    alloc = PageAllocator(4, 64, 4, 2)
    cache = PagedKVFP4(z(4, 2, 64, 64), z(4, 2, 64, 4), z(4, 2, 1, 128, 32), z(4, 2, 1, 128, 2),
                       z(4, 2, 64, 128, dt=torch.float16), z(4, dt=torch.int32), z(4, 2, dt=torch.int32), alloc)
    alloc.reserve([(0, 10), (2, 100)])
    cache.lengths = [10, 0, 100, 0]
    host = (list(cache.lengths), list(alloc._free), [list(p) for p in alloc.pages])
    q = z(5, 4, 128, dt=torch.float16)

    def trap(*a, **k):
        raise AssertionError("a tensor was made before the error was raised")
    monkeypatch.setattr(torch, "tensor", trap)
    monkeypatch.setattr(torch, "empty", trap)
    for ids, lens_, kw, match in [([0, 1], [2, 3], {}, "at least one cached token"),
                                  ([2, 0], [1, 4], {"causal": True, "keys_per_split": 64}, "no CPU fallback"),
                                  ([0, 0], [2, 3], {}, "distinct"), ([0, 7], [2, 3], {}, "distinct"),
                                  ([0, 2], [2, 2], {}, "q_lens sum"),
                                  ([0, 2], [2, 3], {"keys_per_split": 96}, "keys_per_split")]:
        with pytest.raises(_lib.QAttnError, match=match):
            attention_mxfp4_varlen_paged(q, cache, ids, lens_, **kw)
    with pytest.raises(_lib.QAttnError, match="heads"):
        attention_mxfp4_varlen_paged(z(5, 3, 128, dt=torch.float16), cache, [0, 2], [2, 3])
    with pytest.raises(_lib.QAttnError, match="causal"):           # 11 queries over 10 cached tokens
        attention_mxfp4_varlen_paged(z(12, 4, 128, dt=torch.float16), cache, [0, 2], [11, 1], causal=True)
    with pytest.raises(_lib.QAttnError, match="no CPU fallback"):
        attention_mxfp4_varlen_paged(q, cache, [0, 2], [2, 3], keys_per_split=64)
    k = z(5, 2, 128, dt=torch.float16)
    for ids, cnt, match in [([0, 0], [2, 3], "distinct"), ([0, 4], [2, 3], "distinct"), ([0, 2], [5, 0], ">= 1"),
                            ([0, 2], [2, 2], "sum\\(counts\\)"), ([0], [5], "no CPU fallback")]:
        with pytest.raises(_lib.QAttnError, match=match):
            cache.append_packed(k, k, ids, cnt)
    assert host == (list(cache.lengths), list(alloc._free), [list(p) for p in alloc.pages])
