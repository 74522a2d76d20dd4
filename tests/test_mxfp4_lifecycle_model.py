"""The lifecycle fuzz of tests/mxfp4_lifecycle.py, proven on the CPU before it judges the GPU.

1. The schedules cover what they must: over SCHEDULES, the fixed ``(seed, P)`` list that
   tests/test_gpu_mxfp4_lifecycle.py replays, every situation of COVERAGE occurs at least twice.  The count is
   the model's, never the code's under test.
2. The instrument sees faults: :class:`FakePool` is a CPU stand-in with the methods of ``PagedKVFP4`` the
   harness calls -- the real ``PageAllocator``, fp16 rows per physical page, a ``vtail``, epochs, the oracle's
   quantisers behind ``kv`` and the float64 restatements as its attention.  The clean fake passes every schedule;
   each planted fault (a one-line variant) fails the harness on the schedule and the check FAULTS names.
3. The decode step: the old schedules are, by digest, what they were before the generator learnt the ``step``
   operation; over STEP_SCHEDULES every situation of STEP_COVERAGE occurs at least twice and the old operations
   still happen around the steps; ``FakeBackend.step`` (``prepare``'s checks in its order, one row through
   ``_write``, the float64 restatement; no graph) passes every step schedule and five planted faults on it fail.
"""
import collections
import hashlib

import pytest
import torch

import mxfp4_lifecycle as LC
import mxfp4_rope_ref as R
from mxfp4_lifecycle import D, HKV, ceil_div
from oracle import mxfp4 as M
from quantizedattention_amd._lib import QAttnError
from quantizedattention_amd.kv_cache_mxfp4 import PageAllocator

SCHEDULES = LC.SCHEDULES

# every situation must occur at least twice over SCHEDULES
COVERAGE = (
    "fork at L % P != 0 (a copied page)", "fork at L % P == 0", "fork of a fork",
    "fork source freed while its fork lives", "freed source's unshared pages handed to another slot",
    "freed slot used again as a fork target", "freed slot used again as an append target",
    "rollback, L0 % 64 != 0, drafts crossed a tile boundary", "rollback, drafts crossed a page boundary",
    "rollback, L0 % 64 == 0", "rollback, L0 == 0", "two draft rounds through one checkpoint",
    "accept keeping nothing", "accept keeping a proper path in non-ascending order", "accept keeping every draft",
    "rollback with shared pages below L0 (forked before the checkpoint)",
    "refused rollback_shared", "fork after the checkpoint, L0 % P == 0: rollback allowed",
    "trim whose dropped pages a fork still holds", "windowed call on a slot trimmed under a fork",
    "plain call on the fork of a trimmed slot", "trim before the checkpoint, then rollback", "refused stale_trim",
    "shared call, a member has appended or rolled back since", "shared call with an unrelated slot",
    "shared call beside a trimmed former member", "tree call over sequences that share pages",
    "refused out_of_pages_append", "refused out_of_pages_packed", "refused out_of_pages_fork", "refused max_pages",
    "refused fork_nonempty", "refused fork_trimmed", "refused gather_trimmed", "refused plain_trimmed",
    "refused window_too_large", "refused stale_free", "refused stale_rollback", "refused tree_window",
    "refused shared_window", "out of pages after a sequence that would have found its own",
    "attend causal", "attend noncausal", "attend window", "attend shared", "attend tree", "attend decode")


# every situation must occur at least twice over STEP_SCHEDULES
STEP_COVERAGE = (
    "step eager", "step replayed", "step with padding entries", "step listing every slot",
    "replay whose listed slots or their order differ from the configuration's previous step",
    "step at L % 64 == 63 (fills a tile)", "step at L % 64 == 0 (opens a tile)", "step at L % P == 0 (opens a page)",
    "step on a fork while its source lives", "step on a source while its fork lives",
    "step on a slot freed and filled again since the configuration's previous step",
    "windowed step on a slot with holes (a gap)", "windowed step without a gap",
    "step between a checkpoint and its rollback", "step after a rollback", "step after an accept", "rope step",
    "refused step_slots", "refused step_empty", "refused step_full", "refused step_plain_trimmed",
    "refused step_window_trimmed", "refused step_out_of_pages")

# sha256(repr(schedule))[:16] of every entry of SCHEDULES, recorded before the generator learnt the step
# operation: with ``steps`` off it draws what it drew then
DIGESTS = {
    (5, 64, False): "a3f8778adada5fb7", (29, 64, True): "005bb15be9b49719", (89, 64, False): "c91f4dd3461a94b3",
    (94, 64, False): "9d0fbc3421478c8d", (126, 64, False): "c2f84ae876f665f1", (141, 64, False): "f59c38305d467eff",
    (9, 256, False): "43a425529775e0ee", (33, 256, True): "0d26b49690f72961", (37, 256, False): "8a5e65a6f4dc4db9",
    (76, 256, False): "4d1542d679446d9b", (78, 256, False): "1c3959ef1b430b64", (115, 256, False): "a14a1b1bfa9f6d9c"}


def _ops(seed, P, smoothed):
    if (seed, P, smoothed) in LC.STEP_SCHEDULES:
        return LC.step_spec(seed, P, smoothed), LC.step_schedule(seed, P, smoothed)
    return LC.spec(seed, P, smoothed=smoothed), LC.schedule(seed, P, smoothed=smoothed)


def test_the_old_schedules_are_what_they_were():
    assert set(DIGESTS) == set(SCHEDULES) and len(SCHEDULES) == 12 and not set(SCHEDULES) & set(LC.STEP_SCHEDULES)
    for (seed, P, smoothed), digest in DIGESTS.items():
        ops = LC.schedule(seed, P, smoothed=smoothed)
        assert hashlib.sha256(repr(ops).encode()).hexdigest()[:16] == digest, (seed, P)
        assert not any(op["op"] == "step" for op in ops)


def test_step_schedules_cover_the_situations():
    total = collections.Counter()
    per_size = collections.Counter()
    for seed, P, smoothed in LC.STEP_SCHEDULES:
        sp, ops = _ops(seed, P, smoothed)
        assert sp.steps and len(ops) == LC.STEP_N_OPS and ops == LC.step_schedule(seed, P, smoothed)     # seeded
        per_size[P, smoothed] += 1
        cfgs = LC.step_cfgs(sp)
        assert cfgs[0][1] is None and cfgs[1][1:] in LC.TRIMS[P] and cfgs[0][0] != cfgs[1][0]
        assert {c[0] for c in cfgs} <= set(LC.KPS)
        for op in ops:
            if op["op"] == "step":
                assert (op["kps"], op["window"], op["sinks"]) == cfgs[op["cfg"]] and op["how"] in ("eager", "graph")
        total += LC.coverage(sp, ops)
        # the old operations still happen around the steps
        done = collections.Counter(op["op"] for op in ops if not op["refuse"])
        assert all(done[o] for o in ("fork", "free", "trim", "rollback", "step")), (seed, P, done)
        assert any(op["op"] == "attend" and not op["refuse"] and (op["share"] or op["trees"] is not None)
                   for op in ops), (seed, P)
    for P in (64, 256):
        assert per_size[P, False] + per_size[P, True] >= 3 and per_size[P, True] >= 1
    for what in STEP_COVERAGE:
        print(f"MXFP4-LIFE-COVERAGE {total[what]:3d}  {what}")
    assert not [w for w in STEP_COVERAGE if total[w] < 2], {w: total[w] for w in STEP_COVERAGE if total[w] < 2}


def test_the_rope_rows_of_the_steps_are_the_exact_rotation():
    """The rows the model stores for a rope step (mxfp4_rope_ref.rope_ref, the bit-for-bit contract) against the
    float64 rotation ``rope_exact``: the two differ by the roundings of the contract alone -- two fp32 products
    and their fp32 sum, 1.5 * 2^-24 of |a c| + |b s|, then half an fp16 ulp of the result."""
    seed, P, smoothed = LC.STEP_SCHEDULES[0]
    sp, n = LC.step_spec(seed, P, smoothed), 0
    for op in LC.step_schedule(seed, P, smoothed):
        if op["op"] == "step" and op["rope"] and not op["refuse"]:
            k = LC.step_rows(op["seed"], sp.slots)[0]
            pos = [(37 * i + op["seed"]) % LC.MAX_TOKENS[P] for i in range(sp.slots)]
            exact, mag = R.rope_exact(k, LC.rope_of(sp)[0], pos, LC.rope_of(sp)[1])
            got = LC.rotated(sp, k, pos).double()
            ulp = 2.0 ** (torch.floor(torch.log2(exact.abs().clamp_min(2.0 ** -14))) - 10)
            assert bool(((got - exact).abs() <= 0.5 * ulp + 1.5 * 2.0 ** -24 * mag + 2.0 ** -25).all())
            n += 1
    assert n >= 2


def test_schedules_cover_the_situations():
    total = collections.Counter()
    for seed, P, smoothed in SCHEDULES:
        sp, ops = _ops(seed, P, smoothed)
        assert len(ops) == LC.N_OPS and ops == LC.schedule(seed, P, smoothed=smoothed)     # seeded
        assert sp.slots in (5, 6) and (14 <= sp.pages <= 24 if P == 64 else 6 <= sp.pages <= 8)
        total += LC.coverage(sp, ops)
    for what in COVERAGE:
        print(f"MXFP4-LIFE-COVERAGE {total[what]:3d}  {what}")
    assert not [w for w in COVERAGE if total[w] < 2], {w: total[w] for w in COVERAGE if total[w] < 2}
    # (every refusal but that of an accept whose pages a later fork holds, which has a schedule of its own)
    assert set(LC.WORD) - {"out_of_pages_accept"} <= {w[len("refused "):] for w in COVERAGE + STEP_COVERAGE
                                                     if w.startswith("refused ")}


# ------------------------------------------------------------------------------------------------ the fake pool
class _Ckpt:
    def __init__(self, seq_ids, lengths, pages, epochs, saved):
        self.seq_ids, self.lengths, self.pages, self.epochs, self.saved = seq_ids, lengths, pages, epochs, saved


class FakePool:
    """``PagedKVFP4`` without a device: the real allocator, fp16 rows per physical page (``kf``, and ``vf``, the
    rows each V tile was last quantised from), ``vtail``, epochs, and ``kv``, the four operands through the
    oracle's quantisers (quantised when read, from the rows written since).  ``fault`` plants one wrong line."""

    def __init__(self, num_pages, P, slots, Hkv, max_pages, k_mean=None, free_order=None, fault=None):
        self.alloc = PageAllocator(num_pages, P, slots, max_pages, free_order)
        self.P, self.fault = P, fault
        self.kf = torch.zeros((num_pages, Hkv, P, D), dtype=torch.float16)
        self.vf = torch.zeros((num_pages, Hkv, P, D), dtype=torch.float16)
        z = lambda *shape: torch.zeros(shape, dtype=torch.uint8)  # noqa: E731
        self._kv = (z(num_pages, Hkv, P, D // 2), z(num_pages, Hkv, P, D // 32), z(num_pages, Hkv, P // 64, D, 32),
                    z(num_pages, Hkv, P // 64, D, 2))
        self._krows, self._vtiles = [], set()
        self.vtail = torch.zeros((slots, Hkv, 64, D), dtype=torch.float16)
        self.lens = torch.zeros(slots, dtype=torch.int32)
        self.block_table = torch.zeros((slots, max_pages), dtype=torch.int32)
        self.lengths, self.epoch, self.k_mean = [0] * slots, [0] * slots, k_mean

    page_tokens = property(lambda self: self.P)
    num_pages = property(lambda self: self.alloc.num_pages)
    free_pages = property(lambda self: self.alloc.free_pages)

    @property
    def kv(self):
        k4, ks, vt, vs = self._kv
        for x, r0, r1 in self._krows:
            q4, qs = M.quant_rows(self.kf[x, :, r0:r1].reshape(-1, D))
            k4[x, :, r0:r1], ks[x, :, r0:r1] = q4.view(HKV, r1 - r0, D // 2), qs.view(HKV, r1 - r0, D // 32)
        for x, t in self._vtiles:
            qt, qs = M.quant_vt(self.vf[x, :, 64 * t:64 * t + 64])
            vt[x, :, t], vs[x, :, t] = qt[:, 0], qs[:, 0]
        self._krows, self._vtiles = [], set()
        return self._kv

    def _upload(self, table=True):
        if table:
            self.block_table = torch.tensor(self.alloc.table, dtype=torch.int32)
        self.lens = torch.tensor(self.lengths, dtype=torch.int32)

    def _write(self, b, k, v):
        """The append of k, v [c, Hkv, 128] to slot b, whose pages are reserved."""
        P, L, c = self.P, self.lengths[b], k.shape[0]
        if self.k_mean is not None:
            k = (k.float() - self.k_mean[b][:, 0].float()).half()
        pages = self.alloc.pages[b]
        if L % 64:      # the last partial tile is quantised again from its rows in vtail
            x, r = pages[L // P], L % P - L % 64
            self.vf[x, :, r:r + L % 64] = self.vtail[b, :, :L % 64]
        for p in range(L // P, (L + c - 1) // P + 1):
            r0, r1 = max(L, p * P), min(L + c, (p + 1) * P)
            x = pages[p]
            self.kf[x, :, r0 - p * P:r1 - p * P] = k[r0 - L:r1 - L].transpose(0, 1)
            self.vf[x, :, r0 - p * P:r1 - p * P] = v[r0 - L:r1 - L].transpose(0, 1)
            self._krows.append((x, r0 - p * P, r1 - p * P))
        L += c
        if L % 64:      # rows at or past L of the last tile are zero
            x, r = pages[(L - 1) // P], L % P
            self.vf[x, :, r:r - r % 64 + 64] = 0
            self.vtail[b, :, :L % 64] = self.vf[x, :, r - L % 64:r]
        self._vtiles |= {(pages[t * 64 // P], t % (P // 64)) for t in range(self.lengths[b] // 64, (L - 1) // 64 + 1)}
        self.lengths[b] = L

    def append(self, k, v, counts=None):
        grown = self.alloc.reserve([(b, self.lengths[b] + c) for b, c in enumerate(counts) if c])
        for b, c in enumerate(counts):
            if c:
                self._write(b, k[b, :, :c].transpose(0, 1), v[b, :, :c].transpose(0, 1))
        self._upload(bool(grown))
        return self

    def append_packed(self, k, v, seq_ids, counts):
        if self.fault == "append_packed reserves sequence by sequence":
            grown = [self.alloc.reserve([(b, self.lengths[b] + c)]) for b, c in zip(seq_ids, counts)]
        else:
            grown = self.alloc.reserve([(b, self.lengths[b] + c) for b, c in zip(seq_ids, counts)])
        first = 0
        for b, c in zip(seq_ids, counts):
            self._write(b, k[first:first + c], v[first:first + c])
            first += c
        self._upload(bool(grown))
        return self

    def free(self, seqs):
        for b in seqs:
            if self.fault == "free returns a page a fork still holds":
                self.alloc._free += [x for x in self.alloc.pages[b] if x is not None and self.alloc.refcount[x] > 1]
            self.lengths[b] = 0
            self.alloc.release(b)
            self.epoch[b] += 0 if self.fault == "free does not bump the epoch" else 1
        self._upload(False)

    def _whole(self, b, what):
        if self.alloc.nholes[b]:
            raise QAttnError(f"fake pool: {what} would read trimmed pages of sequence {b}")

    def trim(self, seq_ids, window, sinks=0):
        freed = 0
        for b in seq_ids:
            first, last = ceil_div(sinks, self.P), (self.lengths[b] - window + 1) // self.P
            if self.fault == "trim drops the page that holds position L - window" and last > first:
                last += 1
            if last > first:
                freed += self.alloc.drop(b, first, last)
            self.epoch[b] += 1
        return freed

    def checkpoint(self, seq_ids):
        ids, a = list(seq_ids), self.alloc
        return _Ckpt(ids, [self.lengths[b] for b in ids], [len(a.pages[b]) for b in ids],
                     [self.epoch[b] for b in ids], self.vtail[ids].clone())

    def _rollback_check(self, ck, seq_ids):
        ids = ck.seq_ids if seq_ids is None else list(seq_ids)
        rows = [ck.seq_ids.index(b) for b in ids]
        for r in rows:
            b, L0 = ck.seq_ids[r], ck.lengths[r]
            if self.epoch[b] != ck.epochs[r]:
                raise QAttnError(f"fake pool: stale checkpoint of sequence {b}")
            page = self.alloc.pages[b][L0 // self.P] if L0 % self.P else None
            if page is not None and self.alloc.refcount[page] > 1:
                raise QAttnError(f"fake pool: the page that holds position {L0} of sequence {b} is shared")
        return rows

    def _rollback(self, ck, rows):
        P = self.P
        for r in rows:
            b, L0 = ck.seq_ids[r], ck.lengths[r]
            if self.fault != "rollback does not restore vtail":
                self.vtail[b] = ck.saved[r]
            if L0 % 64 and self.fault != "rollback leaves tile L0 // 64 as the drafts quantised it":
                x, r0 = self.alloc.pages[b][L0 // P], L0 % P - L0 % 64
                self.vf[x, :, r0:r0 + 64] = 0
                self.vf[x, :, r0:r0 + L0 % 64] = ck.saved[r][:, :L0 % 64]
                self._vtiles.add((x, r0 // 64))
            keep = ck.pages[r]
            if self.fault == "rollback keeps one page past ceil(L0 / P)":
                keep = min(keep + 1, len(self.alloc.pages[b]))
            self.alloc.shrink(b, keep)
            self.lengths[b] = L0
            self.epoch[b] += 1
            ck.epochs[r] = self.epoch[b]
        self._upload(False)

    def rollback(self, ck, seq_ids=None):
        self._rollback(ck, self._rollback_check(ck, seq_ids))
        return self

    def accept(self, ck, k, v, seq_ids, counts, accepted):
        rows, a, past, need = self._rollback_check(ck, seq_ids), self.alloc, collections.Counter(), 0
        if self.fault == "accept rolls back before it looks for pages":
            self._rollback(ck, rows)
        for r, b, acc in zip(rows, seq_ids, accepted):
            past.update(x for x in a.pages[b][ck.pages[r]:] if x is not None)
            need += max(0, ceil_div(ck.lengths[r] + len(acc), self.P) - ck.pages[r])
        if need > a.free_pages + sum(1 for x, n in past.items() if a.refcount[x] == n):
            raise QAttnError("fake pool: out of pages for the accepted tokens")
        self._rollback(ck, rows)
        first = 0
        kept = []
        for b, c, acc in zip(seq_ids, counts, accepted):
            if self.fault == "accept appends the kept rows in index order":
                acc = sorted(acc)
            kept += [(b, [first + i for i in acc])] if acc else []
            first += c
        if kept:
            idx = torch.tensor([i for _, a in kept for i in a])
            self.append_packed(k[idx], v[idx], [b for b, _ in kept], [len(a) for _, a in kept])
        return self

    def fork(self, src, dst):
        self._whole(src, "fork")
        if self.lengths[dst]:
            raise QAttnError(f"fake pool: fork into sequence {dst}, which is not empty")
        L, P = self.lengths[src], self.P
        if self.fault == "fork shares the partial page":
            self.alloc.share(src, dst, ceil_div(L, P), 0)
        else:
            fresh = self.alloc.share(src, dst, L // P, 1 if L % P else 0)
            if fresh:
                old = self.alloc.pages[src][L // P]
                self.kv     # (the copy takes the bytes as they are)
                for t in (self.kf, self.vf, *self._kv):
                    t[fresh[0]] = t[old]
        if self.fault != "fork does not copy vtail":
            self.vtail[dst] = self.vtail[src]
        if self.k_mean is not None:
            self.k_mean[dst] = self.k_mean[src]
        self.lengths[dst] = L
        self._upload()

    def gather(self, b):
        self._whole(b, "gather")
        pages = torch.tensor(self.alloc.pages[b], dtype=torch.long)
        return tuple(t[pages].transpose(0, 1).reshape(HKV, -1, *t.shape[3:]) for t in self.kv)

    def rows(self, b):
        """fp16 (k, v) [Hkv, L, 128] of slot b through the host page list; the rows of holes are zero."""
        L = self.lengths[b]
        k, v = (torch.zeros((HKV, ceil_div(L, self.P) * self.P, D), dtype=torch.float16) for _ in range(2))
        for i, x in enumerate(self.alloc.pages[b][:ceil_div(L, self.P)]):
            if x is not None:
                k[:, i * self.P:(i + 1) * self.P], v[:, i * self.P:(i + 1) * self.P] = self.kf[x], self.vf[x]
        return k[:, :L].contiguous(), v[:, :L].contiguous()


class FakeBackend:
    device, ops_varlen, ops_step = "cpu", None, None

    def __init__(self, fault=None):
        self.fault = fault

    @staticmethod
    def step_kps(cfg):
        return cfg[0]

    def step(self, pool, cfg, ids, k, v, q, rope, how):
        """``DecodeStep`` without a device and without a graph ("graph" and "eager" are one): ``prepare``'s checks
        in ``prepare``'s order against the real allocator, then one row per listed slot through ``_write`` and
        the float64 restatement of one causal query per slot."""
        (kps, W, S), a, P, N, n, fault = cfg, pool.alloc, pool.P, k.shape[0], len(ids), self.fault
        if n > N or len(set(ids)) != n or any(not 0 <= b < a.max_seqs for b in ids):
            raise QAttnError(f"fake step: seq_ids must be at most {N} distinct slots")
        Ls = [pool.lengths[b] for b in ids]
        if any(L < 1 for L in Ls):
            raise QAttnError("fake step: every listed sequence needs at least one cached token")
        if any(L + 1 > LC.MAX_TOKENS[P] for L in Ls):
            raise QAttnError(f"fake step: a sequence would pass {LC.MAX_TOKENS[P]} keys")
        for b in ids:
            pool.lengths[b] += 1
        try:
            for b in ids:
                holes = set(a.holes(b))
                if holes and (W is None or LC.window_pages(pool.lengths[b], 1, W, S, P) & holes):
                    raise QAttnError(f"fake step: the step would read trimmed pages of sequence {b}")
            grown = a.reserve([(b, pool.lengths[b]) for b in ids])
        except QAttnError:
            for b in ids:
                pool.lengths[b] -= 0 if fault == "a refused prepare keeps the lengths it added" else 1
            raise
        for b in ids:       # (_write adds it again)
            pool.lengths[b] -= 1
        tab, il = rope if rope is not None else (None, False)
        at = [L + 1 for L in Ls] if fault == "the new key is rotated to L + 1" else Ls
        kr = R.rope_ref(k[:n], tab, at, il) if rope is not None else k
        for j, b in enumerate(ids):
            pool._write(b, kr[j:j + 1], v[j:j + 1])
        if fault == "a padding entry's row is appended to the slot its index names":
            for i in range(n, N):
                if i not in ids and pool.lengths[i] % 64:     # (room in its tile, so in its page)
                    pool._write(i, k[i:i + 1], v[i:i + 1])
        pool._upload(bool(grown))
        qr = R.rope_ref(q[:n], tab, Ls, il) if rope is not None else q
        O, lse = torch.zeros((N, LC.HQ, D), dtype=torch.float16), torch.full((N, LC.HQ), float("-inf"))
        for j, b in enumerate(ids):
            kb, vb = pool.rows(b)
            if fault == "the step attends over L keys, not L + 1":
                kb, vb = kb[:, :Ls[j]], vb[:, :Ls[j]]
            O[j], lse[j] = (t[0] for t in LC.restated(
                "fake", qr[j:j + 1], kb, vb, True, kps, W, 0 if fault == "a windowed step ignores its sinks" else S))
        return O, lse

    def allocate(self, *args):
        return FakePool(*args, fault=self.fault)

    def sync(self):
        pass

    @staticmethod
    def varlen(q, pool, ids, q_lens, causal=False, keys_per_split=None, window=None, sinks=0, share_prefix=False,
               tree=None):
        if tree is not None and (window is not None or share_prefix or not causal):
            raise QAttnError("fake pool: tree cannot be combined with a window")
        if share_prefix and window is not None:
            raise QAttnError("fake pool: share_prefix with a window is not supported")
        for b, n in zip(ids, q_lens):
            holes = set(pool.alloc.holes(b))
            if holes and (window is None or LC.window_pages(pool.lengths[b], n, window, sinks, pool.P) & holes):
                raise QAttnError(f"fake pool: the call would read trimmed pages of sequence {b}")
        O, lse, first = [], [], 0
        for j, (b, n) in enumerate(zip(ids, q_lens)):
            k, v = pool.rows(b)
            o, l = LC.restated("fake", q[first:first + n], k, v, causal, keys_per_split, window, sinks,
                               None if tree is None else tree[j])
            O.append(o), lse.append(l)
            first += n
        return torch.cat(O), torch.cat(lse)

    @staticmethod
    def decode(q, pool, causal, keys_per_split):
        B, Hq, n, _ = q.shape
        for b in range(B):
            pool._whole(b, "decode")
        out = [LC.restated("fake", q[b].transpose(0, 1), *pool.rows(b), causal, keys_per_split) for b in range(B)]
        return (torch.stack([o.transpose(0, 1) for o, _ in out]),
                torch.stack([l.transpose(0, 1) for _, l in out]).reshape(B * Hq, n))


# ------------------------------------------------------------------------------------------------ the instrument
def _run(seed, P, smoothed, fault=None):
    sp, ops = _ops(seed, P, smoothed)
    return LC.Harness(FakeBackend(fault), sp, log=lambda *_: None).run(ops)


ACCEPT = "append64-checkpoint-draft64-fork-append70-accept_all_refused-tree-accept_nothing"


def test_the_named_regressions_on_the_clean_fake():
    """The accept whose pages a later fork holds is refused, and afterwards the drafts are still there."""
    sp, ops = LC.regressions()[ACCEPT]
    assert [op["refuse"] for op in ops] == [None] * 5 + ["out_of_pages_accept"] + [None] * 3
    h = LC.Harness(FakeBackend(), sp, log=lambda *_: None).run(ops)
    assert h.m.lengths == [64, 128, 70, 0, 0] and h.m.free == 0
    with pytest.raises(LC.CheckFailed) as e:
        LC.Harness(FakeBackend("accept rolls back before it looks for pages"), sp, log=lambda *_: None).run(ops)
    assert e.value.check == "a refusal changes nothing", str(e.value)


@pytest.mark.parametrize("seed,P,smoothed", SCHEDULES + LC.STEP_SCHEDULES)
def test_the_clean_fake_passes(seed, P, smoothed):
    h = _run(seed, P, smoothed)
    assert h.m.cov == LC.coverage(*_ops(seed, P, smoothed))
    assert all(w == [0.0, 0.0, 0.0] for w in h.worst.values()) and h.worst
    assert ("step" in h.worst) == ((seed, P, smoothed) in LC.STEP_SCHEDULES)


# fault -> ((seed, P, smoothed) of a schedule of SCHEDULES that catches it, the check that fails)
FAULTS = {
    "fork shares the partial page": ((78, 256, False), "free pages"),
    "fork does not copy vtail": ((37, 256, False), "vtail"),
    "rollback leaves tile L0 // 64 as the drafts quantised it": ((141, 64, False), "V scales"),
    "rollback does not restore vtail": ((141, 64, False), "vtail"),
    "free returns a page a fork still holds": ((141, 64, False), "free pages"),
    "rollback keeps one page past ceil(L0 / P)": ((141, 64, False), "free pages"),
    "trim drops the page that holds position L - window": ((89, 64, False), "free pages"),
    "accept appends the kept rows in index order": ((94, 64, False), "K bytes"),
    "free does not bump the epoch": ((78, 256, False), "refusal"),            # the stale rollback is not refused
    # "a refusal changes nothing" itself: the first sequences keep the pages they took before the pool ran out
    "append_packed reserves sequence by sequence": ((78, 256, False), "a refusal changes nothing"),
    # the fake step (FakeBackend.step), on schedules of STEP_SCHEDULES
    "a refused prepare keeps the lengths it added": ((26, 256, False), "a refusal changes nothing"),
    "the new key is rotated to L + 1": ((7, 64, True), "K bytes"),
    "the step attends over L keys, not L + 1": ((108, 256, False), "attention equals the twin pool's"),
    "a windowed step ignores its sinks": ((43, 256, True), "attention equals the twin pool's"),
    "a padding entry's row is appended to the slot its index names": ((72, 64, False), "lengths"),
}
STEP_FAULTS = tuple(f for f in FAULTS if "step" in f or "prepare" in f or "new key" in f or "padding" in f)


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_a_planted_fault_is_caught(fault):
    where, check = FAULTS[fault]
    assert where in (LC.STEP_SCHEDULES if fault in STEP_FAULTS else SCHEDULES) and len(STEP_FAULTS) == 5
    with pytest.raises(LC.CheckFailed) as e:
        _run(*where, fault=fault)
    assert e.value.check == check, str(e.value)
