"""Helpers of tests/test_gpu_mxfp4_varlen.py: the small helpers of tests/test_gpu_mxfp4_paged.py
restated (scattered page pools, the gather through the device table) and the per-sequence reference of
the packed step -- ``attention_mxfp4_decode`` on a batch-1 ``PreallocatedKVFP4`` fed the same tokens.

TEST INFRASTRUCTURE ONLY.  What the lru caches return is shared between tests: do not modify it.
"""
import functools

import torch

D = 128
MAX_SEQS = 6
SLOTS = (4, 0, 5, 2)        # the slots of sequences 0..3; slots 1 and 3 stay empty
LENGTHS = ((1, 63, 65, 200), (64, 130, 256, 70))
Q_LENS = (1, 3, 33, 70)     # G * 70 = 140 rows cross a 128-row block, G * 1 = 2 rows: a nearly empty wave


def scatter(n):
    """A free order whose first n // 3 pages descend in steps of 3."""
    return [p for r in range(3) for p in range(n - 1 - r, -1, -3)]


def assert_scattered(cache):
    for pages in cache.alloc.pages:
        assert all(b < a - 1 for a, b in zip(pages, pages[1:])), pages


def gather(cache, b):
    """Sequence b's rows and tiles through the DEVICE table: (k4 [Hkv, L, 64], ks [Hkv, L, 4], vt [Hkv,
    ceil(L/64), 128, 32], vs [Hkv, ceil(L/64), 128, 2])."""
    L, P, H = cache.lengths[b], cache.page_tokens, cache.k4.shape[1]
    ids = cache.block_table[b, :-(-L // P)].long()
    k4, ks, vt, vs = (t[ids].transpose(0, 1).reshape(H, -1, *t.shape[3:]) for t in cache.kv)
    nt = -(-L // 64)
    return k4[:, :L], ks[:, :L], vt[:, :nt], vs[:, :nt]


def assert_same_bytes(paged, ref):
    """The invariant, slot by slot against a PreallocatedKVFP4 with one sequence per slot: lengths,
    table, rows [0, L) of k4 / ks, tiles [0, ceil(L / 64)) of vt / vs and the live vtail rows."""
    H = ref.k4.shape[1]
    assert paged.lengths == ref.lengths and paged.lens.cpu().tolist() == paged.lengths
    assert ref.lens.cpu().tolist() == ref.lengths
    table = paged.block_table.cpu().tolist()
    for b, L in enumerate(paged.lengths):
        pages = paged.alloc.pages[b]
        assert len(pages) == -(-L // paged.page_tokens) and table[b][:len(pages)] == pages, b
        if L == 0:
            continue
        nt = -(-L // 64)
        k4, ks, vt, vs = gather(paged, b)
        assert torch.equal(k4, ref.k4[b, :, :L]) and torch.equal(ks, ref.ks[b, :, :L]), (b, L)
        assert torch.equal(vt, ref.vt[b * H:b * H + H, :nt]), (b, L)
        assert torch.equal(vs, ref.vs[b * H:b * H + H, :nt]), (b, L)
        assert torch.equal(paged.vtail[b, :, :L % 64], ref.vtail[b * H:b * H + H, :L % 64]), (b, L)


@functools.lru_cache(maxsize=None)
def tokens(Hkv, lengths, seed=31):
    """Per sequence fp16 (k, v) [Hkv, L, 128] on the device."""
    g = torch.Generator().manual_seed(seed)
    return tuple((torch.randn((Hkv, L, D), generator=g).half().cuda(),
                  torch.randn((Hkv, L, D), generator=g).half().cuda()) for L in lengths)


@functools.lru_cache(maxsize=None)
def packed_q(Hq, q_lens=Q_LENS, seed=37):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((sum(q_lens), Hq, D), generator=g).half().cuda()


def fill_pool(Hkv, lengths, P, num_pages, slots=SLOTS, max_seqs=MAX_SEQS):
    """A fresh pool with sequence j of ``tokens(Hkv, lengths)`` in slot slots[j], written by the PADDED
    append (so the attention tests do not lean on append_packed); the other slots are empty."""
    from quantizedattention_amd.kv_cache_mxfp4 import PagedKVFP4
    kv = tokens(Hkv, lengths)
    n = max(lengths)
    k = torch.full((max_seqs, Hkv, n, D), 777.0, dtype=torch.float16, device="cuda")
    v = torch.full((max_seqs, Hkv, n, D), -555.0, dtype=torch.float16, device="cuda")
    counts = [0] * max_seqs
    for (kj, vj), b, L in zip(kv, slots, lengths):
        k[b, :, :L], v[b, :, :L], counts[b] = kj, vj, L
    cache = PagedKVFP4.allocate(num_pages, P, max_seqs, Hkv, -(-320 // P), "cuda", free_order=scatter(num_pages))
    cache.append(k, v, counts=counts)
    assert [cache.lengths[b] for b in slots] == list(lengths) and sum(cache.lengths) == sum(lengths)
    assert_scattered(cache)
    return cache


@functools.lru_cache(maxsize=None)
def pool(Hkv, lengths, P, num_pages):
    """The shared pool of one configuration; do not modify."""
    return fill_pool(Hkv, lengths, P, num_pages)


@functools.lru_cache(maxsize=None)
def alone(Hkv, lengths, j):
    """Sequence j of ``tokens(Hkv, lengths)`` in a batch-1 preallocated cache; do not modify."""
    from quantizedattention_amd.kv_cache_mxfp4 import PreallocatedKVFP4
    k, v = tokens(Hkv, lengths)[j]
    return PreallocatedKVFP4.allocate(1, Hkv, 320, "cuda").append(k[None], v[None])


def per_sequence(q, q_lens, j):
    """Sequence j's packed tokens [n_j, Hq, ..] as the decode layout [1, Hq, n_j, ..] (a view)."""
    first = sum(q_lens[:j])
    return q[first:first + q_lens[j]].transpose(0, 1)[None]


@functools.lru_cache(maxsize=None)
def reference(Hq, Hkv, lengths, j, causal, kps, q_lens=Q_LENS):
    """(O [1, Hq, n_j, 128], lse [Hq, n_j]) of sequence j alone: attention_mxfp4_decode, Sq = q_lens[j]."""
    from quantizedattention_amd.kv_cache_mxfp4 import attention_mxfp4_decode
    q = per_sequence(packed_q(Hq, q_lens), q_lens, j)
    return attention_mxfp4_decode(q, alone(Hkv, lengths, j), causal=causal, keys_per_split=kps)


def assert_sequence_equals(O, lse, q_lens, j, want):
    """Packed outputs of sequence j against (O [1, Hq, n_j, 128], lse [Hq, n_j]) by torch.equal alone."""
    RO, Rl = want
    Oj, lj = per_sequence(O, q_lens, j), per_sequence(lse, q_lens, j)[0]
    assert Oj.shape == RO.shape and lj.shape == Rl.shape and lse.dtype == torch.float32
    assert torch.equal(Oj, RO), j
    assert torch.equal(lj, Rl), j
