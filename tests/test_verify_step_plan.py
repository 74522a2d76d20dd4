"""The plan of the device-planned verify step (kv_cache_mxfp4.plan_verify_step, the pure-Python statement of
qattn_mxfp4_verify_step_plan) against the host plan it replaces: plan_varlen's records with every query a tree
node, rope_positions' depths and append_packed's tile list.  No device.
"""
import random

import pytest

from quantizedattention_amd import _lib
from quantizedattention_amd import kv_cache_mxfp4 as K

LENGTHS = list(range(1, 401))
KS = (1, 5, 33, 64)
KPS = (64, 128, 320)
HQ, HKV = 8, 2


def chain(n):
    return list(range(-1, n - 1))


def wide(n):
    """every node a child of the root"""
    return [-1] + [0] * (n - 1)


def heap(n):
    """deep and wide: node t hangs under (t - 1) // 2"""
    return [-1] + [(t - 1) // 2 for t in range(1, n)]


TREES = (chain, wide, heap)


def words_of(trees):
    return [w for p in trees for w in K.tree_ancestor_masks(p)]


def append_tiles(lengths_before, ids, k):
    """the tile list PagedKVFP4.append_packed builds for counts [k] * n"""
    return [[j, g] for j, b in enumerate(ids)
            for g in range(lengths_before[b] // 64, (lengths_before[b] + k - 1) // 64 + 1)]


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("kps", KPS)
@pytest.mark.parametrize("k", KS)
def test_plan_equals_the_host_plan(k, kps, tree):
    """Every L in [1, 400], one sequence per slot in a shuffled order, so that first tokens and partial bases
    are not the slot's."""
    ids = list(range(len(LENGTHS)))
    random.Random(k * 1000 + kps).shuffle(ids)
    trees = [tree(k)] * len(ids)
    splits = K.verify_step_splits(max(LENGTHS) + k, kps)
    tab, tiles, pos, rec, work = K.plan_verify_step(LENGTHS, ids, k, words_of(trees), kps, splits, HKV, HQ // HKV)
    after = [L + k for L in LENGTHS]
    kps_h, want, _, _ = K.plan_varlen(after, ids, [k] * len(ids), HQ, HKV, kps, causal=True,
                                      tree_lens=[k] * len(ids))
    assert kps_h == kps
    for f in (0, 2, 3, 5, 6, 7):
        assert [r[f] for r in rec] == [r[f] for r in want], f
    assert [r[1] for r in rec] == [i * k for i in range(len(ids))] == [r[1] for r in want]
    assert [r[4] for r in rec] == [i * splits * HQ * k for i in range(len(ids))]
    assert pos == K.rope_positions(LENGTHS, ids, [k] * len(ids), trees)
    assert [t for t in tiles if t != [-1, 0]] == append_tiles(LENGTHS, ids, k)
    assert len(tiles) == 2 * len(ids) and all(tiles[2 * i][0] == i for i in range(len(ids)))
    assert tab == [[b, k, i * k, 0] for i, b in enumerate(ids)]
    assert max(r[3] for r in rec) == splits


@pytest.mark.parametrize("k", KS)
def test_a_sequence_alone_equals_the_host_plan_at_its_clamped_split(k):
    """One sequence per call: plan_varlen clamps kps to the call's keys, which leaves one split either way."""
    for L in (1, 63, 64, 65, 127, 200, 255, 256, 399):
        for kps in KPS:
            for tree in TREES:
                w = words_of([tree(k)])
                rec = K.plan_verify_step([0, L], [1], k, w, kps, 8, HKV, HQ // HKV)[3]
                want = K.plan_varlen([0, L + k], [1], [k], HQ, HKV, kps, causal=True, tree_lens=[k])[1]
                assert rec[0][:4] == want[0][:4] and rec[0][5:] == want[0][5:], (L, kps)


def test_words_are_cleaned_as_the_kernel_cleans_them():
    """Bits above t and a missing own bit do not change the plan."""
    k = 5
    clean = words_of([heap(k)])
    dirty = [(w & ~(1 << t)) | (0xffff << (t + 1)) for t, w in enumerate(clean)]
    signed = [w - (1 << 64) if w >> 63 else w for w in dirty]
    a = K.plan_verify_step([70], [0], k, clean, 64, 3, HKV, 4)
    assert a == K.plan_verify_step([70], [0], k, dirty, 64, 3, HKV, 4)
    assert a == K.plan_verify_step([70], [0], k, signed, 64, 3, HKV, 4)
    assert a[2] == [70, 71, 71, 72, 72]
    top = K.plan_verify_step([70], [0], 64, [(1 << 64) - 1] * 64, 64, 3, HKV, 4)[2]
    assert top == list(range(70, 134))


@pytest.mark.parametrize("kps", KPS)
def test_splits_hold_every_length(kps):
    for max_keys in (1, 64, 65, 320, 321, 400):
        splits = K.verify_step_splits(max_keys, kps)
        assert splits == -(-(-(-max_keys // 64) * 64) // kps)
        for k in KS:
            Ls = [L for L in range(1, max_keys + 1) if L + k <= max_keys]
            if not Ls:
                continue
            rec = K.plan_verify_step(Ls, range(len(Ls)), k, [0] * (k * len(Ls)), kps, 64, HKV, 1)[3]
            assert max(r[3] for r in rec) <= splits
            if max(Ls) + k == max_keys:
                assert max(r[3] for r in rec) == splits
    with pytest.raises(_lib.QAttnError):
        K.verify_step_splits(0, 64)
    with pytest.raises(_lib.QAttnError):
        K.verify_step_splits(64, 96)


def test_padding_is_laid_out_as_specified():
    k, kps, splits, G = 5, 64, 6, 2
    lengths = [1, 0, 316, 315, 200, 0]
    slots = [4, -1, 2, 6, 3, 1]           # -1 and 6 out of range; 316 + 5 > 320; 315 + 5 = 320 is live
    w = words_of([heap(k)] * len(slots))
    tab, tiles, pos, rec, work = K.plan_verify_step(lengths, slots, k, w, kps, splits, HKV, G, capacity=320)
    base = [i * splits * HKV * G * k for i in range(6)]
    pad = lambda i: ([-1, 0, i * k, 0], [[-1, 0], [-1, 0]], [0] * k, [-1, i * k, k, 0, base[i], 0, 0, k])  # noqa: E731
    for i in (1, 2, 3):
        assert (tab[i], tiles[2 * i:2 * i + 2], pos[i * k:i * k + k], rec[i]) == pad(i), i
    assert tab[0] == [4, k, 0, 0] and tiles[0:2] == [[0, 3], [-1, 0]] and rec[0] == [4, 0, k, 4, 0, 0, 0, k]
    assert pos[0:k] == [200, 201, 201, 202, 202]
    assert tab[4] == [3, k, 20, 0] and tiles[8:10] == [[4, 4], [-1, 0]] and rec[4][3] == 5
    # a length of 0 is live to the plan (the host's prepare refuses it): one tile, one split
    assert tab[5] == [1, k, 25, 0] and tiles[10:12] == [[5, 0], [-1, 0]] and rec[5][3] == 1
    # 62 + 5 crosses a tile: both tile records are the entry's
    assert K.plan_verify_step([62], [0], k, w[:k], kps, splits, HKV, G)[1] == [[0, 0], [0, 1]]
    # without a capacity only the slot range pads
    rec2 = K.plan_verify_step(lengths, slots, k, w, kps, splits, HKV, G)[3]
    assert [r[0] for r in rec2] == [4, -1, 2, -1, 3, 1]


@pytest.mark.parametrize("k,group,nrb", ((1, 2, 1), (40, 4, 2), (64, 4, 2), (64, 2, 1), (33, 8, 3)))
def test_work_covers_the_grid_once(k, group, nrb):
    n, splits = 6, 5
    work = K.plan_verify_step([10] * n, range(n), k, [0] * (n * k), 64, splits, HKV, group)[4]
    assert len(work) == n * nrb * splits and all(w[3] == 0 for w in work)
    assert sorted(tuple(w[:3]) for w in work) == [(i, rb, s) for i in range(n) for rb in range(nrb)
                                                 for s in range(splits)]


def test_refusals():
    for bad in (dict(K=0), dict(K=65), dict(kps=96), dict(splits=0), dict(words=[0] * 4)):
        a = dict(K=5, words=[0] * 5, kps=64, splits=2)
        a.update(bad)
        with pytest.raises(_lib.QAttnError):
            K.plan_verify_step([10], [0], a["K"], a["words"], a["kps"], a["splits"], HKV, 2)
