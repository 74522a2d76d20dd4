"""A seeded, model-based lifecycle fuzz of the paged MX-FP4 cache (kv_cache_mxfp4.PagedKVFP4): the model,
the schedule generator and the checker that tests/test_mxfp4_lifecycle_model.py (CPU, on a fake pool) and
tests/test_gpu_mxfp4_lifecycle.py (on the real pool) share.

TEST INFRASTRUCTURE ONLY.

The model (:class:`Model`) is plain Python with CPU tensors and never looks at the code under test.  Per slot it
holds the fp16 K and V rows the sequence holds ([Hkv, L, 128]; K as the pool quantises it, the slot's mean
subtracted), per logical page an identity token or None for a trimmed hole, the ``(window, sinks)`` of its last
trim and the draft that is outstanding on it; per checkpoint the slots, their L0, page count and model epoch.
Identities are integers the model hands out: ``fork`` copies those of the L // P full pages and makes a new one
for a copied partial page, the pool's expected free count is ``num_pages - #distinct identities`` and two
logical pages must be one physical page iff their identities are equal.  Physical page numbers are never
predicted (the pools hand pages out in the scattered order of ``mxfp4_varlen_helpers.scatter``).

``schedule(seed, P, n_ops)`` draws operations with ``random.Random(seed)`` from the model's state alone, illegal
ones included (the model predicts the refusal and the word its message must name), so one schedule replays on
any pool.  :class:`Harness` replays it: ``check`` after every operation (host and table state, then the bytes
against ``oracle.mxfp4``), "a refusal changes nothing" after every refusal, and ``attended`` for every attend
operation and for the slots an operation touched: bit for bit against a fresh twin pool built from the model's
rows by one padded append, and against the float64 restatements at the bars of
``test_trees_against_the_restatement``.  A failure raises :class:`CheckFailed`, which names the check.

With ``Spec.steps`` on (``STEP_SCHEDULES``) the generator also draws decode steps (``DecodeStep``): a ``step``
operation lists slots, one of the schedule's two configurations (``step_cfgs``: plain, and windowed at a
``(W, S)`` of TRIMS), "eager" or "graph", ``rope`` or not.  In the model it is ``append_packed(ids, [1] * n)``
(a rope step stores the key rotated to the length before the step) and one causal query per slot; the
refusals are ``prepare``'s, in its order.  ``Harness.stepped`` sends the listed rows through ``attended`` as mode
"step" and holds the padding rows to O = 0, lse = -inf.
"""
from __future__ import annotations

import collections
import random

import torch

import mxfp4_ragged_ref as RR
import mxfp4_rope_ref as ROPE
import mxfp4_tree_ref as TR
import mxfp4_varlen_helpers as VH
import mxfp4_window_ref as WR
from oracle import mxfp4 as M

D, HQ, HKV = 128, 4, 2
MAX_TOKENS = {64: 384, 256: 768}        # max_pages_per_seq * P
N_OPS = 40
STEP_N_OPS = 48                         # of a schedule with steps
BARS = (2e-2, 1e-4, 2e-3)               # max|dO|, max|dlse|, relL2: test_trees_against_the_restatement's
KPS = (64, 128, None)
TRIMS = {64: ((16, 0), (16, 4), (70, 64), (130, 4), (40, 70)), 256: ((16, 0), (70, 4), (130, 0), (16, 256))}

ROPE_MAX = 800                          # rows of the rotary table of the rope steps (> MAX_TOKENS + 1)

# ``steps``: the schedule also draws decode steps (kv_cache_mxfp4.DecodeStep); off, _Gen draws what it always drew
Spec = collections.namedtuple("Spec", "seed P slots pages smoothed n_ops steps", defaults=(False,))

# (seed, P, smoothed): the schedules both test files replay; one per page size runs a smoothed pool
SCHEDULES = ((5, 64, False), (29, 64, True), (89, 64, False), (94, 64, False), (126, 64, False),
             (141, 64, False), (9, 256, False), (33, 256, True), (37, 256, False), (76, 256, False),
             (78, 256, False), (115, 256, False))

# (seed, P, smoothed) with ``steps`` on: the schedules that hold the decode step, eager and graph-replayed
# (tests/test_mxfp4_lifecycle_model.py::STEP_COVERAGE)
STEP_SCHEDULES = ((7, 64, True), (9, 64, False), (72, 64, False), (103, 64, False), (26, 256, False),
                  (43, 256, True), (99, 256, False), (108, 256, False))

# what a refusal of each kind must name
WORD = {"out_of_pages_append": "out of pages", "out_of_pages_packed": "out of pages",
        "out_of_pages_fork": "out of pages", "out_of_pages_accept": "out of pages",
        "max_pages": "max_pages_per_seq", "fork_nonempty": "not empty",
        "fork_trimmed": "trimmed", "gather_trimmed": "trimmed", "plain_trimmed": "trimmed",
        "window_too_large": "trimmed", "stale_free": "stale", "stale_trim": "stale", "stale_rollback": "stale",
        "rollback_shared": "shared", "tree_window": "tree", "shared_window": "share_prefix",
        # DecodeStep.prepare, in the order of its checks
        "step_slots": "distinct", "step_empty": "at least one cached token", "step_full": "would pass",
        "step_plain_trimmed": "trimmed", "step_window_trimmed": "trimmed", "step_out_of_pages": "out of pages"}


def spec(seed: int, P: int, n_ops: int = N_OPS, smoothed: bool = False, steps: bool = False) -> Spec:
    """The pool of schedule ``(seed, P)``: 5 or 6 slots and a pool small enough to run out by itself."""
    pages = 14 + (5 * seed) % 11 if P == 64 else 6 + seed % 3
    return Spec(seed, P, 5 + seed % 2, pages, smoothed, n_ops, steps)


def step_spec(seed: int, P: int, smoothed: bool = False) -> Spec:
    """The pool of the step schedule ``(seed, P)``."""
    return spec(seed, P, STEP_N_OPS, smoothed, steps=True)


def step_cfgs(sp: Spec) -> tuple:
    """The two step configurations ``(kps, window, sinks)`` of a schedule: plain at one ``kps``, windowed at a
    ``(W, S)`` of TRIMS[P] at another."""
    rng = random.Random(7919 * sp.seed + sp.P)
    k0, k1 = rng.sample(KPS, 2)
    return (k0, None, 0), (k1, *rng.choice(TRIMS[sp.P]))


def step_rows(seed: int, n: int):
    """The fp16 (k, v [n, Hkv, 128], q [n, Hq, 128]) of a step of n entries; the rows of padding entries hold
    values too."""
    g = torch.Generator().manual_seed(seed + 29)
    r = lambda h: torch.randn((n, h, D), generator=g).half()  # noqa: E731
    return r(HKV), r(HKV), r(HQ)


_ROPE = []


def rope_of(sp: Spec) -> tuple:
    """(table fp32 [ROPE_MAX, 128] on the CPU, interleaved) of the rope steps of a schedule; odd seeds pair
    elements (2i, 2i + 1)."""
    if not _ROPE:
        _ROPE.append(ROPE.table(ROPE_MAX))
    return _ROPE[0], bool(sp.seed % 2)


def rotated(sp: Spec, x, pos):
    """x fp16 [n, H, 128] rotated to ``pos`` as include/qattn.h defines it bit for bit (mxfp4_rope_ref.rope_ref),
    so that the rows are what the pool must quantise."""
    tab, interleaved = rope_of(sp)
    return ROPE.rope_ref(x, tab, list(pos), interleaved)


def rows(seed: int, n: int):
    """The fp16 (k, v) [n, Hkv, 128] an operation appends."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn((n, HKV, D), generator=g).half(), torch.randn((n, HKV, D), generator=g).half()


def queries(seed: int, n: int):
    return torch.randn((n, HQ, D), generator=torch.Generator().manual_seed(seed + 7)).half()


def means(seed: int, slots: int):
    return torch.randn((slots, HKV, 1, D), generator=torch.Generator().manual_seed(seed + 13)).half()


def ceil_div(a: int, b: int) -> int:
    return -(-a // b)


def window_pages(L: int, n: int, W: int, S: int, P: int) -> set:
    """The pages a windowed call of n queries reads of a sequence of L keys (module docstring of
    kv_cache_mxfp4: the sink run and the window run, or every tile when the two touch)."""
    nt, first, sink = ceil_div(L, 64), max(0, L - n - W + 1) // 64, ceil_div(min(S, L), 64)
    tiles = set(range(nt)) if first <= sink else set(range(sink)) | set(range(first, nt))
    return {t // (P // 64) for t in tiles}


class CheckFailed(AssertionError):
    def __init__(self, check: str, detail=""):
        super().__init__(f"{check}: {detail}")
        self.check = check


def need(cond, check: str, detail="") -> None:
    if not cond:
        raise CheckFailed(check, detail() if callable(detail) else detail)


# ------------------------------------------------------------------------------------------------ model
class Seq:
    def __init__(self, was_freed=False):
        self.L, self.k, self.v, self.ids = 0, None, None, []
        self.trim = None            # (window, sinks) of the last trim
        self.version = 0            # bumped whenever the rows change
        self.draft = None           # the outstanding draft: {"ckpt", "parents", "n"}
        self.is_fork = self.has_forks = self.mutated = False
        self.was_freed = was_freed
        self.trim_shared = self.holds_trimmed = False
        self.family = None
        self.exp = None             # the expected bytes (Model.expected)
        self.parent = None          # the Seq this one was forked from
        self.after = None           # "rollback" / "accept" until the next step

    @property
    def holes(self) -> set:
        return {i for i, x in enumerate(self.ids) if x is None}


class Model:
    def __init__(self, sp: Spec, data: bool = True):
        self.sp, self.P, self.pages, self.nslots, self.data = sp, sp.P, sp.pages, sp.slots, data
        self.maxp = MAX_TOKENS[sp.P] // sp.P
        self.mean = means(sp.seed, sp.slots) if sp.smoothed else None
        self.seqs = [Seq() for _ in range(sp.slots)]
        self.epoch, self.why = [0] * sp.slots, [None] * sp.slots
        self.ckpts, self.next_id, self.families, self.tick = [], 0, 0, 0
        self.cov = collections.Counter()
        self.pending_reuse = None   # the slot whose shared-source free released unshared pages
        self.frees = [0] * sp.slots  # how often each slot was freed
        self.stepped = {}           # per step configuration, its last step: {"ids", "frees"}

    def _bump(self, s) -> None:
        self.tick += 1
        s.version = self.tick

    # ---------------------------------------------------------------------------- queries
    @property
    def lengths(self) -> list:
        return [s.L for s in self.seqs]

    def held(self) -> collections.Counter:
        return collections.Counter(i for s in self.seqs for i in set(s.ids) if i is not None)

    @property
    def free(self) -> int:
        return self.pages - len(self.held())

    def shares(self, b: int, upto=None) -> bool:
        held = self.held()
        return any(i is not None and held[i] > 1 for i in self.seqs[b].ids[:upto])

    def _grow_refusal(self, reqs, kind: str):
        needs = {b: max(0, ceil_div(self.seqs[b].L + c, self.P) - len(self.seqs[b].ids)) for b, c in reqs if c}
        if any(len(self.seqs[b].ids) + n > self.maxp for b, n in needs.items()):
            return "max_pages"
        return kind if sum(needs.values()) > self.free else None

    def _rollback_refusal(self, c: int, slots):
        ck = self.ckpts[c]
        held = self.held()
        for b in ck["slots"] if slots is None else slots:
            if self.epoch[b] != ck["epochs"][b]:
                return "stale_" + self.why[b]
            L0, s = ck["L0"][b], self.seqs[b]
            if L0 % self.P and held[s.ids[L0 // self.P]] > 1:
                return "rollback_shared"
        return None

    def accept_fits(self, c: int, accepted) -> bool:
        """Whether the append of an accept finds its pages after the rollback: a page past the cut comes back
        only when the listed sequences are all its holders (a fork made after the drafts keeps it)."""
        ck, d = self.ckpts[c], self.ckpts[c]["draft"]
        held, needs, past = self.held(), 0, collections.Counter()
        for b, acc in zip(d["ids"], accepted):
            keep = ceil_div(ck["L0"][b], self.P)
            past.update(self.seqs[b].ids[keep:])
            needs += max(0, ceil_div(ck["L0"][b] + len(acc), self.P) - keep)
        return needs <= self.free + sum(1 for i, n in past.items() if held[i] == n)

    def refusal(self, op):
        """The kind of refusal (a key of WORD) the pool owes this operation, or None."""
        o = op["op"]
        if o == "append_packed":
            return self._grow_refusal(zip(op["ids"], op["counts"]), "out_of_pages_packed")
        if o == "step":
            return self._step_refusal(op)
        if o == "draft":
            return self._grow_refusal(zip(op["ids"], [len(t) for t in op["trees"]]), "out_of_pages_packed")
        if o == "append":
            return self._grow_refusal(enumerate(op["counts"]), "out_of_pages_append")
        if o == "fork":
            s, d = self.seqs[op["src"]], self.seqs[op["dst"]]
            if s.holes:
                return "fork_trimmed"
            if d.L:
                return "fork_nonempty"
            return "out_of_pages_fork" if s.L % self.P and self.free < 1 else None
        if o == "gather":
            return "gather_trimmed" if self.seqs[op["slot"]].holes else None
        if o == "rollback":
            return self._rollback_refusal(op["ckpt"], op["slots"])
        if o == "accept":
            kind = self._rollback_refusal(op["ckpt"], self.ckpts[op["ckpt"]]["draft"]["ids"])
            return kind or (None if self.accept_fits(op["ckpt"], op["accepted"]) else "out_of_pages_accept")
        if o == "attend":
            if op["trees"] is not None and op["window"] is not None:
                return "tree_window"
            if op["share"] and op["window"] is not None:
                return "shared_window"
            if op["mode"] == "decode":
                return "plain_trimmed" if any(s.holes for s in self.seqs) else None
            for b, n in zip(op["ids"], op["q_lens"]):
                s = self.seqs[b]
                if op["window"] is None:
                    if s.holes:
                        return "plain_trimmed"
                elif window_pages(s.L, n, op["window"], op["sinks"], self.P) & s.holes:
                    return "window_too_large"
        return None

    def _step_refusal(self, op):
        """DecodeStep.prepare's checks, in its order."""
        ids, W, S = op["ids"], op["window"], op["sinks"]
        if len(ids) > self.nslots or len(set(ids)) != len(ids) or any(not 0 <= b < self.nslots for b in ids):
            return "step_slots"
        seqs = [self.seqs[b] for b in ids]
        if any(not s.L for s in seqs):
            return "step_empty"
        if any(s.L + 1 > MAX_TOKENS[self.P] for s in seqs):
            return "step_full"
        for s in seqs:      # the lengths the step attends at
            if W is None:
                if s.holes:
                    return "step_plain_trimmed"
            elif window_pages(s.L + 1, 1, W, S, self.P) & s.holes:
                return "step_window_trimmed"
        return self._grow_refusal([(b, 1) for b in ids], "step_out_of_pages")

    def note_refusal(self, kind: str, op=None) -> None:
        self.cov["refused " + kind] += 1
        if kind in ("out_of_pages_packed", "out_of_pages_append") and op is not None and op["op"] != "draft":
            reqs = zip(op["ids"], op["counts"]) if "ids" in op else enumerate(op["counts"])
            needs = [ceil_div(self.seqs[b].L + c, self.P) - len(self.seqs[b].ids) for b, c in reqs if c]
            if 0 < needs[0] <= self.free:   # a reservation made sequence by sequence would have begun
                self.cov["out of pages after a sequence that would have found its own"] += 1

    # ---------------------------------------------------------------------------- transitions
    def _new_ids(self, b: int, count: int) -> list:
        if count and self.pending_reuse is not None and self.pending_reuse != b:
            self.cov["freed source's unshared pages handed to another slot"] += 1
            self.pending_reuse = None
        out = list(range(self.next_id, self.next_id + count))
        self.next_id += count
        return out

    def _grow(self, b: int, c: int, k=None, v=None) -> None:
        """Append c tokens, raw fp16 ``k, v`` [c, Hkv, 128], to slot b."""
        s = self.seqs[b]
        if s.L == 0:
            if s.was_freed:
                self.cov["freed slot used again as an append target"] += 1
                s.was_freed = False
            if s.family is None:
                s.family, self.families = self.families, self.families + 1
        s.ids += self._new_ids(b, ceil_div(s.L + c, self.P) - len(s.ids))
        if self.data:
            if self.mean is not None:
                k = (k.float() - self.mean[b][:, 0].float()).half()
            k, v = k.transpose(0, 1), v.transpose(0, 1)
            s.k = k.clone() if s.k is None else torch.cat([s.k, k], 1)
            s.v = v.clone() if s.v is None else torch.cat([s.v, v], 1)
        s.L += c
        self._bump(s)
        s.mutated = True

    def _cut(self, b: int, L0: int) -> None:
        s = self.seqs[b]
        s.ids = s.ids[:ceil_div(L0, self.P)]
        if self.data and s.k is not None:
            s.k, s.v = s.k[:, :L0], s.v[:, :L0]
        if s.exp is not None:
            s.exp["L"] = min(s.exp["L"], L0)
        s.L = L0
        self._bump(s)

    def _rollback(self, c: int, b: int) -> None:
        ck, s, P = self.ckpts[c], self.seqs[b], self.P
        L0, L = ck["L0"][b], s.L
        if L > L0:
            if L0 % 64 and (L - 1) // 64 > L0 // 64:
                self.cov["rollback, L0 % 64 != 0, drafts crossed a tile boundary"] += 1
            if L0 % P and ceil_div(L, P) > ceil_div(L0, P):
                self.cov["rollback, drafts crossed a page boundary"] += 1
            if L0 and L0 % 64 == 0:
                self.cov["rollback, L0 % 64 == 0"] += 1
            if L0 == 0:
                self.cov["rollback, L0 == 0"] += 1
            if self.shares(b, ceil_div(L0, P)):
                self.cov["rollback with shared pages below L0 (forked before the checkpoint)"] += 1
            if b in ck["forked_after"] and L0 % P == 0:
                self.cov["fork after the checkpoint, L0 % P == 0: rollback allowed"] += 1
            if s.holes:
                self.cov["trim before the checkpoint, then rollback"] += 1
            if b in ck["stepped"]:
                self.cov["step between a checkpoint and its rollback"] += 1
        self._cut(b, L0)
        ck["stepped"].discard(b)
        s.draft, s.mutated = None, True
        self.epoch[b] += 1
        self.why[b] = "rollback"
        ck["epochs"][b] = self.epoch[b]

    def apply(self, op) -> list:
        """Make the (legal) operation happen in the model -> the slots whose state it touched."""
        o, P = op["op"], self.P
        if o in ("append_packed", "append"):
            pairs = list(zip(op["ids"], op["counts"])) if o == "append_packed" else \
                [(b, c) for b, c in enumerate(op["counts"]) if c]
            k, v = rows(op["seed"], sum(op["counts"])) if self.data else (None, None)
            first = sum(op["counts"][:pairs[0][0]]) if o == "append" else 0
            for b, c in pairs:      # (a padded append carries the packed rows of its seed, slot by slot)
                self._grow(b, c, *((k[first:first + c], v[first:first + c]) if self.data else ()))
                first += c
            return [b for b, _ in pairs]
        if o == "fork":
            s, d, L = self.seqs[op["src"]], self.seqs[op["dst"]], self.seqs[op["src"]].L
            self.cov["fork at L % P != 0 (a copied page)" if L % P else "fork at L % P == 0"] += 1
            if s.is_fork:
                self.cov["fork of a fork"] += 1
            if d.was_freed:
                self.cov["freed slot used again as a fork target"] += 1
            d.__init__()
            d.ids = s.ids[:L // P] + self._new_ids(op["dst"], 1 if L % P else 0)
            d.k, d.v, d.L = s.k, s.v, L
            self._bump(d)
            d.is_fork, d.family, s.has_forks, s.mutated = True, s.family, True, False
            d.parent = s
            if self.mean is not None:
                self.mean[op["dst"]] = self.mean[op["src"]]
            for ck in self.ckpts:
                if op["src"] in ck["slots"] and ck["epochs"][op["src"]] == self.epoch[op["src"]]:
                    ck["forked_after"].add(op["src"])
            return [op["src"], op["dst"]]
        if o == "free":
            for b in op["slots"]:
                s, held = self.seqs[b], self.held()
                if s.has_forks and any(held[i] > 1 for i in s.ids if i is not None):
                    self.cov["fork source freed while its fork lives"] += 1
                    if any(held[i] == 1 for i in s.ids if i is not None):
                        self.pending_reuse = b
                self.seqs[b] = Seq(was_freed=s.L > 0 or s.was_freed)
                self.frees[b] += 1
                self._bump(self.seqs[b])
                self.epoch[b] += 1
                self.why[b] = "free"
            return list(op["slots"])
        if o == "trim":
            W, S = op["window"], op["sinks"]
            for b in op["slots"]:
                s = self.seqs[b]
                first, last = ceil_div(S, P), (s.L - W + 1) // P
                gone = [s.ids[p] for p in range(first, last) if s.ids[p] is not None]
                for p in range(first, last):
                    s.ids[p] = None
                held = self.held()
                if any(held[i] for i in gone):      # a fork still holds them: fewer freed than holes
                    self.cov["trim whose dropped pages a fork still holds"] += 1
                    s.trim_shared = True
                    for t in self.seqs:
                        t.holds_trimmed |= any(i in t.ids for i in gone)
                s.trim = (W, S)
                self.epoch[b] += 1
                self.why[b] = "trim"
            return list(op["slots"])
        if o == "checkpoint":
            self.ckpts.append({"slots": list(op["slots"]), "L0": {b: self.seqs[b].L for b in op["slots"]},
                               "npages": {b: len(self.seqs[b].ids) for b in op["slots"]},
                               "epochs": {b: self.epoch[b] for b in op["slots"]},
                               "rounds": collections.Counter(), "forked_after": set(), "draft": None,
                               "stepped": set()})
            return []
        if o == "draft":
            ck = self.ckpts[op["ckpt"]]
            counts = [len(t) for t in op["trees"]]
            k, v = rows(op["seed"], sum(counts)) if self.data else (None, None)
            first = 0
            for b, t in zip(op["ids"], op["trees"]):
                self._grow(b, len(t), *((k[first:first + len(t)], v[first:first + len(t)]) if self.data else ()))
                first += len(t)
                self.seqs[b].draft = {"ckpt": op["ckpt"], "parents": list(t), "n": len(t)}
                ck["rounds"][b] += 1
                if ck["rounds"][b] == 2:
                    self.cov["two draft rounds through one checkpoint"] += 1
            ck["draft"] = {"ids": list(op["ids"]), "counts": counts, "seed": op["seed"]}
            return list(op["ids"])
        if o == "rollback":
            slots = self.ckpts[op["ckpt"]]["slots"] if op["slots"] is None else op["slots"]
            for b in slots:
                self._rollback(op["ckpt"], b)
                self.seqs[b].after = "rollback"
            return list(slots)
        if o == "accept":
            d = self.ckpts[op["ckpt"]]["draft"]
            k, v = rows(d["seed"], sum(d["counts"])) if self.data else (None, None)
            first = 0
            for b, c, acc in zip(d["ids"], d["counts"], op["accepted"]):
                self._rollback(op["ckpt"], b)
                what = "nothing" if not acc else "every draft" if len(acc) == c else \
                    "a proper path in non-ascending order" if acc != sorted(acc) else "a proper path"
                self.cov["accept keeping " + what] += 1
                if acc:
                    idx = torch.tensor([first + i for i in acc])
                    self._grow(b, len(acc), *((k[idx], v[idx]) if self.data else ()))
                first += c
                self.seqs[b].after = "accept"
            return list(d["ids"])
        if o == "step":
            return self._step(op)
        if o == "attend":
            self._cover_attend(op)
        return []

    def _step(self, op) -> list:
        """One decode step: ``append_packed(ids, [1] * n)`` of the first n rows of the step's k, v (with ``rope``
        the key of slot b rotated to L_b, its length before the step); the attend that follows changes nothing."""
        ids, cfg, P, cov = op["ids"], op["cfg"], self.P, self.cov
        prev, n = self.stepped.get(cfg), len(ids)
        replayed = op["how"] == "graph" and prev is not None    # the first step of a configuration warms up
        cov["step replayed" if replayed else "step eager"] += 1
        cov["step with padding entries" if n < self.nslots else "step listing every slot"] += 1
        if replayed and prev["ids"] != ids:
            cov["replay whose listed slots or their order differ from the configuration's previous step"] += 1
        if op["rope"]:
            cov["rope step"] += 1
        live = lambda a, b: any(t is a for t in self.seqs) and set(a.ids) & set(b.ids) - {None}  # noqa: E731
        for b in ids:
            s, L = self.seqs[b], self.seqs[b].L
            cov["step at L % 64 == 63 (fills a tile)"] += L % 64 == 63
            cov["step at L % 64 == 0 (opens a tile)"] += L % 64 == 0
            cov["step at L % P == 0 (opens a page)"] += L % P == 0
            cov["step on a fork while its source lives"] += bool(s.parent is not None and live(s.parent, s))
            cov["step on a source while its fork lives"] += any(t.parent is s and live(t, s) for t in self.seqs)
            cov["step on a slot freed and filled again since the configuration's previous step"] += \
                prev is not None and self.frees[b] > prev["frees"][b]
            if op["window"] is not None:    # window_pages: the sink run and the window run, apart or touching
                gap = (L + 1 - op["window"]) // 64 > ceil_div(min(op["sinks"], L + 1), 64)
                cov["windowed step on a slot with holes (a gap)"] += bool(gap and s.holes)
                cov["windowed step without a gap"] += not gap
            if s.after:
                cov["step after " + ("a rollback" if s.after == "rollback" else "an accept")] += 1
                s.after = None
            for ck in self.ckpts:
                if b in ck["slots"] and ck["epochs"][b] == self.epoch[b]:
                    ck["stepped"].add(b)
        if self.data:
            k, v, _ = step_rows(op["seed"], self.nslots)
            k = rotated(self.sp, k[:n], [self.seqs[b].L for b in ids]) if op["rope"] else k
        for j, b in enumerate(ids):
            self._grow(b, 1, *((k[j:j + 1], v[j:j + 1]) if self.data else ()))
        self.stepped[cfg] = {"ids": list(ids), "frees": list(self.frees)}
        return list(ids)

    def _cover_attend(self, op) -> None:
        mode = op["mode"]
        self.cov["attend " + mode] += 1
        seqs = [self.seqs[b] for b in op["ids"]]
        if op["window"] is not None:
            if any(s.trim_shared and s.holes for s in seqs):
                self.cov["windowed call on a slot trimmed under a fork"] += 1
        elif any(s.holds_trimmed for s in seqs):
            self.cov["plain call on the fork of a trimmed slot"] += 1
        if op["share"]:
            groups = collections.defaultdict(list)
            for b in op["ids"]:
                groups[self.seqs[b].ids[0]].append(b)
            grouped = [g for g in groups.values() if len(g) > 1]
            members = {b for g in grouped for b in g}
            if any(self.seqs[b].mutated for b in members):
                self.cov["shared call, a member has appended or rolled back since"] += 1
            if grouped and len(members) < len(op["ids"]):
                self.cov["shared call with an unrelated slot"] += 1
            fams = {self.seqs[b].family for b in members}
            if any(s.holes and s.family in fams for s in self.seqs):
                self.cov["shared call beside a trimmed former member"] += 1
        if op["trees"] is not None and any(t is not None and self.shares(b) for b, t in zip(op["ids"], op["trees"])):
            self.cov["tree call over sequences that share pages"] += 1

    # ---------------------------------------------------------------------------- expected bytes
    def expected(self, b: int):
        """(k4 [Hkv, L, 64], ks [Hkv, L, 4], vt [Hkv, ceil(L/64), 128, 32], vs [.., 2]) of slot b from the
        oracle's quantisers, V zero-padded to a multiple of 64; kept per slot and extended from the rows
        that were there already, so a check quantises only what is new."""
        s = self.seqs[b]
        e = s.exp
        if e is not None and e["version"] == s.version:
            return e["out"]
        if e is None:
            e = {"L": 0, "k4": torch.zeros((HKV, 0, D // 2), dtype=torch.uint8),
                 "ks": torch.zeros((HKV, 0, D // 32), dtype=torch.uint8),
                 "vt": torch.zeros((HKV, 0, D, 32), dtype=torch.uint8),
                 "vs": torch.zeros((HKV, 0, D, 2), dtype=torch.uint8)}
        L0, L = e["L"], s.L
        k4, ks = M.quant_rows(s.k[:, L0:L].reshape(HKV * (L - L0), D))
        e["k4"] = torch.cat([e["k4"][:, :L0], k4.view(HKV, L - L0, D // 2)], 1)
        e["ks"] = torch.cat([e["ks"][:, :L0], ks.view(HKV, L - L0, D // 32)], 1)
        t0 = L0 // 64
        vt, vs = M.quant_vt(RR.pad64(s.v[:, 64 * t0:L]))
        e["vt"], e["vs"] = torch.cat([e["vt"][:, :t0], vt], 1), torch.cat([e["vs"][:, :t0], vs], 1)
        e.update(L=L, version=s.version, out=(e["k4"], e["ks"], e["vt"], e["vs"]))
        s.exp = e
        return e["out"]


def padded_rows(op, slots: int):
    """k, v [slots, Hkv, n, 128] of a padded append: the packed rows of its seed, sequence by sequence, in a
    filler no sequence may take."""
    n = max(op["counts"])
    pk, pv = rows(op["seed"], sum(op["counts"]))
    k = torch.full((slots, HKV, n, D), 777.0, dtype=torch.float16)
    v = torch.full((slots, HKV, n, D), -555.0, dtype=torch.float16)
    first = 0
    for b, c in enumerate(op["counts"]):
        k[b, :, :c], v[b, :, :c] = pk[first:first + c].transpose(0, 1), pv[first:first + c].transpose(0, 1)
        first += c
    return k, v


# ------------------------------------------------------------------------------------------------ generator
def _tree(rng: random.Random, nd: int) -> list:
    shape = rng.choice(("chain", "star", "random", "random", "heap", "forest"))
    if shape == "chain":
        return TR.chain(nd)
    if shape == "star":
        return TR.star(nd)
    if shape == "heap":
        return TR.heap(nd)
    if shape == "forest":
        return TR.forest(nd, rng.randint(2, 6))
    return [-1] + [rng.randrange(t) for t in range(1, nd)]


def _path(parents, leaf: int) -> list:
    path = []
    while leaf >= 0:
        path.append(leaf)
        leaf = parents[leaf]
    return path[::-1]


class _Gen:
    """Draws operations from the model's state alone.  The weights below were set until the situations of
    tests/test_mxfp4_lifecycle_model.py::COVERAGE occur over SCHEDULES."""

    WEIGHTS = (("append_packed", 5), ("grow", 3), ("append", 2), ("fork", 5), ("free", 3), ("trim", 4),
               ("checkpoint", 4), ("draft", 6), ("rollback", 4), ("accept", 4), ("attend", 8), ("illegal", 4))

    def __init__(self, sp: Spec):
        self.sp, self.rng, self.m = sp, random.Random(1000 * sp.seed + sp.P), Model(sp, data=False)
        self.n, self.refused = 0, 0
        # with steps on: the step move (set until STEP_COVERAGE occurs over STEP_SCHEDULES) and its configurations
        self.weights = self.WEIGHTS + ((("step", 12),) if sp.steps else ())
        self.cfgs = step_cfgs(sp) if sp.steps else ()

    # -- helpers
    def live(self, whole=False):
        return [b for b, s in enumerate(self.m.seqs) if s.L and not (whole and s.holes)]

    def count(self, L: int) -> int:
        r, P = self.rng.random(), self.sp.P
        if r < .12:
            return 1
        if r < .22:
            return self.rng.randint(2, 8)
        if r < .4 and P - L % P <= 70:
            return P - L % P
        if r < .55:
            return 64 - L % 64
        return self.rng.randint(30 if P == 256 else 9, 70)

    def seed(self) -> int:
        return 100003 * self.sp.seed + 101 * self.n + self.sp.P

    def room(self, b: int, c: int) -> int:
        return max(0, min(c, MAX_TOKENS[self.sp.P] - self.m.seqs[b].L))

    # -- moves: each returns an operation or None when the state offers none
    def append_packed(self):
        rng, m = self.rng, self.m
        cand = [b for b in range(m.nslots) if not m.seqs[b].draft]
        if not cand:
            return None
        ids = rng.sample(cand, min(len(cand), rng.choice((1, 1, 2, 3))))
        longest = max(cand, key=lambda b: m.seqs[b].L)
        if rng.random() < .4 and longest not in ids:
            ids[0] = longest
        pairs = [(b, self.room(b, self.count(m.seqs[b].L))) for b in ids]
        pairs = [(b, c) for b, c in pairs if c]
        if not pairs:
            return None
        return {"op": "append_packed", "ids": [b for b, _ in pairs], "counts": [c for _, c in pairs],
                "seed": self.seed()}

    def grow(self):
        """The longest sequence grows: long sequences are what trims, full pages and max_pages_per_seq need."""
        m = self.m
        cand = [b for b in self.live() if not m.seqs[b].draft and m.seqs[b].L < MAX_TOKENS[self.sp.P]]
        if not cand:
            return None
        b = max(cand, key=lambda x: m.seqs[x].L)
        c = self.room(b, self.rng.randint(50, 70))
        return {"op": "append_packed", "ids": [b], "counts": [c], "seed": self.seed()}

    def append(self):
        rng, m = self.rng, self.m
        counts = [self.room(b, self.count(s.L)) if not s.draft and rng.random() < .5 else 0
                  for b, s in enumerate(m.seqs)]
        return {"op": "append", "counts": counts, "seed": self.seed()} if any(counts) else None

    def fork(self):
        rng, m = self.rng, self.m
        src, dst = self.live(whole=True), [b for b, s in enumerate(m.seqs) if not s.L]
        if not src or not dst:
            return None
        # the sources that matter most: a drafted slot whose drafts filled the page that holds L0, a
        # checkpointed slot, a fork
        hot = [b for b in src if m.seqs[b].draft or m.seqs[b].is_fork
               or any(b in ck["slots"] and ck["epochs"][b] == m.epoch[b] for ck in m.ckpts)]
        P = self.sp.P
        # a draft that filled the page holding L0: after this fork the rollback must be refused ("shared")
        trap = [b for b in src if m.seqs[b].draft and m.ckpts[m.seqs[b].draft["ckpt"]]["L0"][b] % P
                and m.seqs[b].L // P > m.ckpts[m.seqs[b].draft["ckpt"]]["L0"][b] // P]
        full = [b for b in src if m.seqs[b].L >= P]
        even = [b for b in src if m.seqs[b].L % P == 0]
        b = rng.choice(trap) if trap and rng.random() < .7 else rng.choice(even) if even and rng.random() < .6 \
            else rng.choice(hot) if hot and rng.random() < .5 else rng.choice(full) if full and rng.random() < .8 \
            else rng.choice(src)
        return {"op": "fork", "src": b, "dst": rng.choice(dst)}

    def free(self):
        rng, m = self.rng, self.m
        live = self.live()
        if len(live) < 2 and m.free > 2:
            return None
        sources = [b for b in live if m.seqs[b].has_forks and m.shares(b)]
        if sources and rng.random() < .6:
            return {"op": "free", "slots": [rng.choice(sources)]}
        return {"op": "free", "slots": rng.sample(live, min(len(live), rng.choice((1, 1, 2))))}

    def trim(self):
        rng, m, P = self.rng, self.m, self.sp.P
        opts = [(b, W, S) for b in self.live() for W, S in TRIMS[P]
                if (m.seqs[b].L - W + 1) // P > ceil_div(S, P) and m.seqs[b].trim in (None, (W, S))]
        if not opts:
            return None
        if self.sp.steps and rng.random() < .7:   # the trim the windowed steps can follow
            opts = [o for o in opts if o[1:] == self.cfgs[1][1:]] or opts
        shared = [o for o in opts if m.shares(o[0])]
        b, W, S = rng.choice(shared if shared and rng.random() < .7 else opts)
        return {"op": "trim", "slots": [b], "window": W, "sinks": S}

    def checkpoint(self):
        rng, m = self.rng, self.m
        cand = [b for b in range(m.nslots) if not m.seqs[b].draft]
        if not self.live() or not cand:
            return None
        forks = [b for b in cand if m.seqs[b].L and m.shares(b)]
        slots = rng.sample(cand, min(len(cand), rng.choice((1, 2, 2, 3))))
        if forks and rng.random() < .7 and forks[0] not in slots:
            slots[0] = rng.choice(forks)
        return {"op": "checkpoint", "slots": list(dict.fromkeys(slots))}

    def _fresh(self, c: int) -> list:
        ck, m = self.m.ckpts[c], self.m
        return [b for b in ck["slots"] if ck["epochs"][b] == m.epoch[b] and not m.seqs[b].draft]

    def draft(self):
        rng, m = self.rng, self.m
        cks = [c for c in range(len(m.ckpts)) if self._fresh(c)]
        if not cks:
            return None
        c = rng.choice(cks[-3:])
        ids = [b for b in self._fresh(c) if rng.random() < .8] or self._fresh(c)[:1]
        trees = []
        for b in ids:
            L = m.seqs[b].L
            r = rng.random()
            nd = 64 if r < .12 else 64 - L % 64 + rng.randint(1, 6) if r < .4 else rng.randint(1, 24)
            nd = self.room(b, min(nd, 64))
            trees.append(_tree(rng, nd) if nd else None)
        ids, trees = [b for b, t in zip(ids, trees) if t], [t for t in trees if t]
        return {"op": "draft", "ckpt": c, "ids": ids, "trees": trees, "seed": self.seed()} if ids else None

    def rollback(self):
        rng, m = self.rng, self.m
        cand = [(c, b) for c, ck in enumerate(m.ckpts) for b in ck["slots"]
                if ck["epochs"][b] == m.epoch[b] and m.seqs[b].L >= ck["L0"][b]]
        drafted = [(c, b) for c, b in cand if m.seqs[b].draft and m.seqs[b].draft["ckpt"] == c]
        stepped = [(c, b) for c, b in cand if b in m.ckpts[c]["stepped"] and not m.seqs[b].draft] \
            if self.sp.steps else []
        if stepped and rng.random() < .6:     # a rollback that takes decode steps back
            c, b = rng.choice(stepped)
            return {"op": "rollback", "ckpt": c, "slots": [b]}
        if not cand or not drafted and rng.random() < .75:
            return None
        c, b = rng.choice(drafted if drafted and rng.random() < .85 else cand)
        if rng.random() < .3:
            return {"op": "rollback", "ckpt": c, "slots": None}
        more = [x for y, x in drafted if y == c and x != b and rng.random() < .5]
        return {"op": "rollback", "ckpt": c, "slots": [b] + more}

    def accept(self):
        rng, m = self.rng, self.m
        cks = [c for c, ck in enumerate(m.ckpts) if ck["draft"] is not None
               and all(m.seqs[b].draft and m.seqs[b].draft["ckpt"] == c for b in ck["draft"]["ids"])]
        if not cks:
            return None
        c = rng.choice(cks)
        accepted = []
        for b in m.ckpts[c]["draft"]["ids"]:
            par = m.seqs[b].draft["parents"]
            r = rng.random()
            if r < .2:
                acc = []
            elif r < .4:
                acc = list(range(len(par)))
            else:
                acc = _path(par, rng.randrange(len(par)))
                if rng.random() < .5:
                    acc = acc[::-1] if rng.random() < .5 else rng.sample(acc, len(acc))
            accepted.append(acc)
        return {"op": "accept", "ckpt": c, "accepted": accepted}

    def _q_len(self, L: int) -> int:
        r = self.rng.random()
        return 1 if r < .4 else min(L, self.rng.randint(2, 5)) if r < .8 else min(L, self.rng.randint(6, 70))

    def attend(self, mode=None):
        rng, m = self.rng, self.m
        live, whole = self.live(), self.live(whole=True)
        if not live:
            return None
        op = {"op": "attend", "mode": None, "ids": None, "q_lens": None, "kps": rng.choice(KPS), "causal": True,
              "window": None, "sinks": 0, "share": False, "trees": None, "seed": self.seed()}
        by_page = collections.defaultdict(list)
        for b in whole:
            by_page[m.seqs[b].ids[0]].append(b)
        groups = [g for g in by_page.values() if len(g) > 1]
        drafted = [b for b in whole if m.seqs[b].draft]
        modes = ["window", "window"]
        modes += ["causal", "causal", "noncausal"] if whole else []
        modes += ["shared"] * 4 if groups else []
        # a group whose former member was trimmed: the trimmed one must have fallen out of it
        orphaned = [g for g in groups if any(s.holes and s.family == m.seqs[g[0]].family for s in m.seqs)]
        modes += ["shared"] * 8 if orphaned else []
        modes += ["tree"] * 4 if drafted else []
        modes += ["decode"] * 3 if len(whole) == m.nslots else []
        mode = op["mode"] = mode or rng.choice(modes)
        if mode not in modes:
            return None
        if mode == "decode":
            op["causal"] = rng.random() < .5
            n = rng.randint(1, 3)
            op["ids"], op["q_lens"] = list(range(m.nslots)), [min(n, *m.lengths) if op["causal"] else n] * m.nslots
            return op
        if mode == "window":
            trimmed = [b for b in live if m.seqs[b].holes]
            ids = rng.sample(live, min(len(live), rng.randint(1, 3)))
            if trimmed:
                t = rng.choice(trimmed)
                ids = [t] + [b for b in ids if not m.seqs[b].holes]
                W, S = m.seqs[t].trim
                W, S = (W, S) if rng.random() < .7 else (rng.randint(1, W), rng.randint(0, S))
            else:
                W, S = rng.choice((1, 16, 70, 130, 1000)), rng.choice((0, 4, 64, 70))
            op.update(ids=ids, window=W, sinks=S)
            # queries at positions the trim left visible: the tokens appended since, or the last one
            op["q_lens"] = [min(self._q_len(m.seqs[b].L), 3) if m.seqs[b].holes else self._q_len(m.seqs[b].L)
                            for b in ids]
            return op
        if mode == "shared":
            g = rng.choice(orphaned or groups)
            ids = list(g)
            others = [b for b in whole if b not in g]
            if others and rng.random() < .7:
                ids.append(rng.choice(others))
            rng.shuffle(ids)
            op.update(ids=ids, share=True, causal=rng.random() < .8, kps=rng.choice((64, 128)))
        elif mode == "tree":
            ids = [b for b in drafted if rng.random() < .8] or drafted[:1]
            ids += [b for b in whole if b not in drafted and rng.random() < .3]
            rng.shuffle(ids)
            op.update(ids=ids, trees=[m.seqs[b].draft["parents"] if m.seqs[b].draft else None for b in ids])
            op["q_lens"] = [min(m.seqs[b].L, m.seqs[b].draft["n"] + rng.choice((0, 0, 1, 3))) if m.seqs[b].draft
                            else self._q_len(m.seqs[b].L) for b in ids]
            return op
        else:
            op.update(ids=rng.sample(whole, min(len(whole), rng.randint(1, 4))), causal=mode == "causal")
        op["q_lens"] = [self._q_len(m.seqs[b].L) for b in op["ids"]]
        return op

    def _steppable(self, cfg: int) -> list:
        """The slots a step of configuration ``cfg`` may list: not empty, not full, no outstanding draft (as for
        ``append_packed``) and no hole the step would read."""
        m, P, (_, W, S) = self.m, self.sp.P, self.cfgs[cfg]
        return [b for b, s in enumerate(m.seqs) if s.L and not s.draft and s.L < MAX_TOKENS[P]
                and not (s.holes if W is None else window_pages(s.L + 1, 1, W, S, P) & s.holes)]

    def _step_op(self, cfg: int, ids) -> dict:
        kps, W, S = self.cfgs[cfg]
        return {"op": "step", "ids": list(ids), "cfg": cfg, "kps": kps, "window": W, "sinks": S,
                "how": self.rng.choice(("eager", "graph", "graph")), "rope": self.rng.random() < .4,
                "seed": self.seed()}

    def step(self):
        rng, m = self.rng, self.m
        cfg = rng.randrange(2)
        cand = self._steppable(cfg)
        if not cand:
            return None
        ids = rng.sample(cand, len(cand) if rng.random() < .35 else rng.randint(1, len(cand)))
        holed = [b for b in cand if m.seqs[b].holes]
        if holed and rng.random() < .7 and not set(holed) & set(ids):
            ids[0] = rng.choice(holed)
        return self._step_op(cfg, ids)

    def _illegal_steps(self, cheap: bool = True) -> list:
        """Steps DecodeStep.prepare must refuse, of the kinds the state offers."""
        rng, m, P = self.rng, self.m, self.sp.P
        cfg = rng.randrange(2)
        good = self._steppable(cfg)
        base = rng.sample(good, min(len(good), 2))
        offers = []
        if cheap and rng.random() < .3:     # the refusals every state offers
            empty = [b for b, s in enumerate(m.seqs) if not s.L]
            offers += [self._step_op(cfg, base + [b]) for b in empty[:1]]
            if base:
                offers.append(self._step_op(cfg, base + [rng.choice((base[0], m.nslots, -1))]))
        for b, s in enumerate(m.seqs):
            if s.L == MAX_TOKENS[P]:
                offers += [self._step_op(cfg, base + [b])] * 3
            if s.holes and not s.draft and s.L < MAX_TOKENS[P]:
                offers += [self._step_op(c, [x for x in base if x in self._steppable(c)] + [b]) for c in (0, 1)]
        opening = [b for b in good if m.seqs[b].L % P == 0]
        if len(opening) > m.free:
            offers += [self._step_op(cfg, rng.sample(opening, len(opening)))] * 3
        return offers

    def illegal(self):
        """An operation the pool must refuse, of a kind the state offers (the rarest kinds first)."""
        rng, m = self.rng, self.m
        live, holed = self.live(), [b for b in self.live() if m.seqs[b].holes]
        offers = []
        stale = [(c, b) for c, ck in enumerate(m.ckpts) for b in ck["slots"] if ck["epochs"][b] != m.epoch[b]]
        for c, b in stale[-3:]:
            offers.append({"op": "rollback", "ckpt": c, "slots": [b] if rng.random() < .6 else None})
        for c, ck in enumerate(m.ckpts):
            if m._rollback_refusal(c, None) == "rollback_shared":
                offers += [{"op": "rollback", "ckpt": c, "slots": None}] * 3
        for b in holed:
            empty = [d for d, s in enumerate(m.seqs) if not s.L]
            if empty:
                offers.append({"op": "fork", "src": b, "dst": rng.choice(empty)})
            offers.append({"op": "gather", "slot": b})
            W, S = m.seqs[b].trim
            for kind in ("plain", "wide"):
                a = self.attend("window")
                a["ids"], a["q_lens"] = [b], [1]
                if kind == "plain":
                    a.update(mode=rng.choice(("causal", "noncausal")), window=None, sinks=0)
                    a["causal"] = a["mode"] == "causal"
                else:
                    a.update(window=W + rng.choice((64, 200, 1000)), sinks=S)
                offers.append(a)
        whole = self.live(whole=True)
        cheap = rng.random() < .3     # the refusals every state offers
        if len(live) > 1 and whole and cheap:
            src = rng.choice(whole)
            offers.append({"op": "fork", "src": src, "dst": rng.choice([b for b in live if b != src])})
        top = max(range(m.nslots), key=lambda b: m.seqs[b].L)
        if not m.seqs[top].draft and m.seqs[top].L + 70 > MAX_TOKENS[self.sp.P]:
            c = MAX_TOKENS[self.sp.P] - m.seqs[top].L + rng.randint(1, 5)
            offers += [{"op": "append_packed", "ids": [top], "counts": [c], "seed": self.seed()}] * 3
        empty = [d for d, s in enumerate(m.seqs) if not s.L]
        if not m.free and empty:
            offers += [{"op": "fork", "src": b, "dst": rng.choice(empty)} for b in whole if m.seqs[b].L % self.sp.P] * 3
        if m.free <= 3:   # one sequence more than the pool can serve: the first ones would find their pages
            cand = [b for b in range(m.nslots) if not m.seqs[b].draft and m.seqs[b].L + 70 <= MAX_TOKENS[self.sp.P]
                    and ceil_div(m.seqs[b].L + 70, self.sp.P) > len(m.seqs[b].ids)]
            if len(cand) > m.free:
                ids = rng.sample(cand, m.free + 1)
                offers += [{"op": "append_packed", "ids": ids, "counts": [70] * len(ids), "seed": self.seed()}] * 3
                counts = [70 if b in ids else 0 for b in range(m.nslots)]
                offers += [{"op": "append", "counts": counts, "seed": self.seed()}] * 2
        if live and cheap:
            a = self.attend("causal" if whole else "window")
            if a["mode"] == "causal":
                if rng.random() < .5:
                    a.update(mode="shared+window", share=True, window=64, kps=64)
                else:
                    a.update(mode="tree+window", window=64, trees=[[-1]] * len(a["ids"]))
                offers.append(a)
        if self.sp.steps:
            offers += self._illegal_steps()
        offers = [o for o in offers if m.refusal(o)]
        if not offers:
            return None
        rare = [o for o in offers if m.cov["refused " + m.refusal(o)] == 0]
        return rng.choice(rare or offers)

    def draw(self):
        rng, m = self.rng, self.m
        if not self.live():
            ids = rng.sample(range(m.nslots), 3)
            return {"op": "append_packed", "ids": ids, "counts": [rng.randint(40, 70) for _ in ids],
                    "seed": self.seed()}
        names, weights = zip(*self.weights)
        if self.sp.steps and rng.random() < .4 and self.refused <= .25 * (self.n + 4):
            # a step refusal of a kind this schedule has not had yet, whenever the state offers one
            new = [o for o in self._illegal_steps(cheap=False) if m.refusal(o) and not m.cov["refused " + m.refusal(o)]]
            if new:
                return rng.choice(new)
            fill = [b for b in self._steppable(0) if m.seqs[b].L % self.sp.P]
            if not m.free and fill and not m.cov["refused step_out_of_pages"]:
                # the pool is empty: fill a page to its end, so that a step on that slot needs a page
                b = rng.choice(fill)
                return {"op": "append_packed", "ids": [b], "counts": [self.sp.P - m.seqs[b].L % self.sp.P],
                        "seed": self.seed()}
        for _ in range(200):
            name = rng.choices(names, weights)[0]
            if name == "free" and m.free > 3 and rng.random() < .5 and not any(
                    s.has_forks and s.L and m.shares(b) for b, s in enumerate(m.seqs)):
                continue
            op = getattr(self, name)()
            if op is None:
                continue
            kind = m.refusal(op)
            if kind and (name != "illegal" and rng.random() < .5 or self.refused > .25 * (self.n + 4)):
                continue
            return op
        raise RuntimeError("the generator found no operation")

    def run(self) -> list:
        out = []
        for self.n in range(self.sp.n_ops):
            op = self.draw()
            kind = self.m.refusal(op)
            op["refuse"] = kind
            if kind:
                self.refused += 1
                self.m.note_refusal(kind, op)
            else:
                self.m.apply(op)
            out.append(op)
        return out


def schedule(seed: int, P: int, n_ops: int = N_OPS, smoothed: bool = False, steps: bool = False) -> list:
    """The operations of schedule ``(seed, P)``; each carries the refusal the model predicts ("refuse")."""
    return _Gen(spec(seed, P, n_ops, smoothed, steps)).run()


def step_schedule(seed: int, P: int, smoothed: bool = False) -> list:
    """The operations of the step schedule ``(seed, P)``: STEP_N_OPS of them, decode steps among them."""
    return _Gen(step_spec(seed, P, smoothed)).run()


def scripted(sp: Spec, ops) -> list:
    """A hand-written schedule: every operation gets a seed and the refusal the model predicts."""
    m = Model(sp, data=False)
    for i, op in enumerate(ops):
        if op["op"] == "attend":
            op = ops[i] = {"kps": 64, "causal": True, "window": None, "sinks": 0, "share": False, "trees": None, **op}
        if op["op"] == "step":
            op = ops[i] = {"cfg": 0, "kps": 64, "window": None, "sinks": 0, "how": "eager", "rope": False, **op}
        op.setdefault("seed", 900001 + 101 * i)
        op["refuse"] = m.refusal(op)
        m.note_refusal(op["refuse"], op) if op["refuse"] else m.apply(op)
    return ops


def regressions() -> dict:
    """The shortest schedules that failed on the pool, named by their operations -> {name: (Spec, ops)}."""
    out = {}
    # accept rolled back and only then found the pool empty: a fork made after the drafts held the drafts' page,
    # so the rollback returned nothing, the append of the kept tokens raised and the drafts were gone
    out["append64-checkpoint-draft64-fork-append70-accept_all_refused-tree-accept_nothing"] = (
        Spec(0, 64, 5, 4, False, 9), scripted(Spec(0, 64, 5, 4, False, 9), [
            {"op": "append_packed", "ids": [0], "counts": [64]},
            {"op": "checkpoint", "slots": [0]},
            {"op": "draft", "ckpt": 0, "ids": [0], "trees": [TR.chain(64)]},
            {"op": "fork", "src": 0, "dst": 1},
            {"op": "append_packed", "ids": [2], "counts": [70]},
            {"op": "accept", "ckpt": 0, "accepted": [list(range(64))]},
            {"op": "attend", "mode": "tree", "ids": [0, 1], "q_lens": [64, 2], "trees": [TR.chain(64), None]},
            {"op": "accept", "ckpt": 0, "accepted": [[]]},
            {"op": "attend", "mode": "causal", "ids": [2, 0, 1], "q_lens": [3, 1, 5]}]))
    return out


def coverage(sp: Spec, ops) -> collections.Counter:
    """The situations the model counts while it replays ``ops`` (no data, no pool)."""
    m = Model(sp, data=False)
    for op in ops:
        kind = m.refusal(op)
        assert kind == op["refuse"], (name_of(op), kind)
        m.note_refusal(kind, op) if kind else m.apply(op)
    return m.cov


def name_of(op) -> str:
    o = op["op"]
    if o == "attend":
        return f"attend:{op['mode']}{op['ids']}x{op['q_lens']}"
    extra = op.get("ids", op.get("slots", op.get("slot", "")))
    if o == "fork":
        extra = f"{op['src']}->{op['dst']}"
    if o == "append":
        extra = op["counts"]
    if "counts" in op and o == "append_packed":
        extra = f"{op['ids']}+{op['counts']}"
    if o == "draft":
        extra = f"{op['ids']}+{[len(t) for t in op['trees']]}"
    if o == "accept":
        extra = f"ckpt{op['ckpt']}{[len(a) for a in op['accepted']]}"
    if o == "rollback":
        extra = f"ckpt{op['ckpt']}{op['slots']}"
    if o == "step":
        extra = f"{op['ids']}cfg{op['cfg']}:{op['how']}" + ("+rope" if op["rope"] else "")
    return f"{o}{extra}" + (f"!{op['refuse']}" if op.get("refuse") else "")


# ------------------------------------------------------------------------------------------------ restatements
_REF = {}


def restated(mode: str, q, k, v, causal: bool, kps, window=None, sinks=0, parents=None):
    """One sequence of a packed call on the CPU in float64: q [n, Hq, 128], k, v [Hkv, L, 128] -> (O fp16 [n, Hq,
    128], lse fp32 [n, Hq]).  ``mxfp4_ragged_ref`` / ``mxfp4_window_ref`` / ``mxfp4_tree_ref`` with
    ``mxfp4_split_ref.merge``; kept by content, so the same call on two pools is restated once."""
    key = (causal, kps, window, sinks, None if parents is None else tuple(parents),
           q.numpy().tobytes(), hash(k.numpy().tobytes()), hash(v.numpy().tobytes()), k.shape[1])
    if key not in _REF:
        if len(_REF) > 64:
            _REF.clear()
        q1, k1, v1 = q.transpose(0, 1)[None], k[None], v[None]
        big = RR.ceil64(k.shape[1]) if kps is None else kps
        if window is not None:
            O, lse, _ = WR.mxfp4_fwd_window(q1, k1, v1, window, sinks, big)
        elif parents is not None:
            O, lse, _ = TR.mxfp4_fwd_tree(q1, k1, v1, len(parents), TR.ancestors(parents), big)
        else:
            O, lse, _ = RR.mxfp4_fwd_ragged(q1, [k1], [v1], causal, big)
        _REF[key] = (O[0].transpose(0, 1).contiguous(), lse.view(HQ, -1).transpose(0, 1).contiguous())
    return _REF[key]


# ------------------------------------------------------------------------------------------------ harness
class Harness:
    """Replays a schedule on a pool of ``backend`` and holds it to the model after every operation.

    ``backend`` has ``device``, ``allocate(num_pages, P, slots, Hkv, max_pages, k_mean, free_order)``,
    ``varlen(q, pool, ids, q_lens, **kw)``, ``decode(q, pool, causal, keys_per_split)``, ``sync()`` and
    ``ops_varlen`` (the operator form of ``varlen``, or None); for a schedule with steps also ``step(pool, cfg,
    ids, k, v, q, rope, how) -> (O [N, Hq, 128], lse [N, Hq])`` -- one decode step of configuration ``cfg`` =
    ``(kps, window, sinks)`` over the slots ``ids``, ``rope`` None or ``rope_of(sp)``, ``how`` "eager" or "graph"
    --, ``step_kps(cfg)``, the keys per split that configuration runs at, and ``ops_step`` (below, or None)."""

    def __init__(self, backend, sp: Spec, log=print):
        self.be, self.sp, self.m, self.log = backend, sp, Model(sp), log
        km = None if self.m.mean is None else self.m.mean.clone()
        self.pool = backend.allocate(sp.pages, sp.P, sp.slots, HKV, self.m.maxp, km, VH.scatter(sp.pages))
        self.ckpts, self.restated, self.worst, self.n, self._twin = [], set(), {}, 0, (None, None)

    def dev(self, t):
        return t.to(self.be.device)

    # ---------------------------------------------------------------------------- execution
    def execute(self, op):
        o, pool = op["op"], self.pool
        if o == "append_packed":
            k, v = rows(op["seed"], sum(op["counts"]))
            pool.append_packed(self.dev(k), self.dev(v), op["ids"], op["counts"])
        elif o == "append":
            k, v = padded_rows(op, self.sp.slots)
            pool.append(self.dev(k), self.dev(v), counts=op["counts"])
        elif o == "fork":
            pool.fork(op["src"], op["dst"])
        elif o == "gather":
            pool.gather(op["slot"])
        elif o == "free":
            pool.free(op["slots"])
        elif o == "trim":
            pool.trim(op["slots"], op["window"], op["sinks"])
        elif o == "checkpoint":
            self.ckpts.append(pool.checkpoint(op["slots"]))
        elif o == "draft":
            counts = [len(t) for t in op["trees"]]
            k, v = rows(op["seed"], sum(counts))
            pool.append_packed(self.dev(k), self.dev(v), op["ids"], counts)
        elif o == "rollback":
            pool.rollback(self.ckpts[op["ckpt"]], op["slots"])
        elif o == "accept":
            d = self.m.ckpts[op["ckpt"]]["draft"]
            k, v = rows(d["seed"], sum(d["counts"]))
            pool.accept(self.ckpts[op["ckpt"]], self.dev(k), self.dev(v), d["ids"], d["counts"], op["accepted"])
        elif o == "attend":
            return self.call(pool, op)
        elif o == "step":
            k, v, q = (self.dev(t) for t in step_rows(op["seed"], self.sp.slots))
            O, lse = self.be.step(pool, (op["kps"], op["window"], op["sinks"]), op["ids"], k, v, q,
                                  rope_of(self.sp) if op["rope"] else None, op["how"])
            return O.cpu(), lse.cpu()

    @staticmethod
    def q_of(op):
        """The packed queries of an attend operation: those of its seed, or the ones it carries (a step's)."""
        return op["q"] if "q" in op else queries(op["seed"], sum(op["q_lens"]))

    def call(self, pool, op, share=None, fn=None):
        """The attention call of ``op`` on ``pool`` -> (O, lse) on the CPU, packed [T, Hq, ..]."""
        q = self.dev(self.q_of(op))
        if op["mode"] == "decode":
            n = op["q_lens"][0]
            O, lse = self.be.decode(q.view(self.sp.slots, n, HQ, D).transpose(1, 2).contiguous(), pool, op["causal"],
                                    op["kps"])
            return (O.transpose(1, 2).reshape(-1, HQ, D).cpu(),
                    lse.view(self.sp.slots, HQ, n).transpose(1, 2).reshape(-1, HQ).cpu())
        kw = dict(causal=op["causal"], keys_per_split=op["kps"])
        if op["window"] is not None:
            kw.update(window=op["window"], sinks=op["sinks"])
        if op["share"] if share is None else share:
            kw["share_prefix"] = True
        if op["trees"] is not None:
            kw["tree"] = op["trees"]
        O, lse = (fn or self.be.varlen)(q, pool, op["ids"], op["q_lens"], **kw)
        return O.cpu(), lse.cpu()

    def snapshot(self):
        self.be.sync()
        p, a = self.pool, self.pool.alloc
        host = (list(p.lengths), list(p.epoch), list(a._free), list(a.refcount), [list(x) for x in a.pages],
                list(a.nholes), [list(r) for r in a.table], [list(c.epochs) for c in self.ckpts])
        dev = [t.clone() for t in (*p.kv, p.vtail, p.lens, p.block_table)]
        dev += [c.saved.clone() for c in self.ckpts] + ([] if p.k_mean is None else [p.k_mean.clone()])
        return host, dev

    def step(self, op):
        kind = self.m.refusal(op)
        need(kind == op["refuse"], "schedule", f"op {self.n} {name_of(op)}: the model now says {kind}")
        before = self.snapshot() if kind else None
        refused = out = None
        try:
            out = self.execute(op)
        except RuntimeError as e:
            if type(e).__name__ != "QAttnError":    # anything else is no refusal: a launch or the device failed
                raise
            refused = str(e)
        what = f"seed={self.sp.seed} P={self.sp.P} op={self.n} {name_of(op)}"
        if kind:
            self.m.note_refusal(kind, op)
            need(refused is not None, "refusal", f"{what}: not refused")
            need(WORD[kind] in refused, "refusal", f"{what}: the message does not name {WORD[kind]!r}: {refused}")
            host, dev = self.snapshot()
            need(host == before[0] and all(torch.equal(x, y) for x, y in zip(dev, before[1])),
                 "a refusal changes nothing", what)
            touched = []
        else:
            need(refused is None, "refusal", f"{what}: refused: {refused}")
            touched = self.m.apply(op)
        self.check(what)
        if op["op"] == "attend" and not kind:
            self.attended(op, out, what)
        if op["op"] == "step" and not kind:
            self.stepped(op, out, what)
            touched = []    # (the step attended on exactly the slots it touched)
        for b in touched:
            if self.m.seqs[b].L:
                self.attended(self.touch(b), None, what)
        self.n += 1

    def stepped(self, op, out, what=""):
        """The (O, lse) [N, ..] of a step: the listed entries are an attend operation of mode "step" (one causal
        query per slot at the step's keys per split and window; for a rope step the queries rotated to the
        lengths before the step, and no ``rope=``), the padding entries O = 0 and lse = -inf."""
        (O, lse), ids, n = out, op["ids"], len(op["ids"])
        need(not bool(O[n:].any()) and bool((lse[n:] == float("-inf")).all()), "padding rows",
             lambda: f"{what}: O {O[n:].abs().max():.3e}, lse {lse[n:].tolist()}")
        q = step_rows(op["seed"], self.sp.slots)[2][:n]
        if op["rope"]:
            q = rotated(self.sp, q, [self.m.seqs[b].L - 1 for b in ids])
        cfg = (op["kps"], op["window"], op["sinks"])
        att = {"op": "attend", "mode": "step", "ids": ids, "q_lens": [1] * n, "kps": self.be.step_kps(cfg),
               "causal": True, "window": op["window"], "sinks": op["sinks"], "share": False, "trees": None,
               "seed": op["seed"], "q": q}
        self.attended(att, (O[:n].contiguous(), lse[:n].contiguous()), f"{what} {name_of(op)}")

    def touch(self, b: int):
        """A small causal call on slot b (under its window when it is trimmed), or None where the holes allow
        no call of one query."""
        s = self.m.seqs[b]
        op = {"op": "attend", "mode": "touched", "ids": [b], "q_lens": [min(2, s.L)], "kps": 64, "causal": True,
              "window": None, "sinks": 0, "share": False, "trees": None, "seed": 7919 * self.n + b}
        if s.holes:
            op.update(window=s.trim[0], sinks=s.trim[1], q_lens=[1])
        return None if self.m.refusal(op) else op

    # ---------------------------------------------------------------------------- check
    def check(self, what=""):
        """Host and table state, then the bytes (module docstring)."""
        self.be.sync()
        m, p, a, P = self.m, self.pool, self.pool.alloc, self.sp.P
        lens, table = p.lens.cpu().tolist(), p.block_table.cpu().tolist()
        need(list(p.lengths) == m.lengths, "lengths", lambda: f"{what}: {p.lengths} != {m.lengths}")
        need(lens == m.lengths, "lens on the device", lambda: f"{what}: {lens} != {m.lengths}")
        need(p.free_pages == m.free, "free pages", lambda: f"{what}: {p.free_pages} free, the model has {m.free}")
        phys, ident, holders = {}, {}, collections.Counter()
        for b, s in enumerate(m.seqs):
            pages = a.pages[b]
            need(len(pages) == len(s.ids), "page count", lambda: f"{what}: slot {b} {pages} for {s.ids}")
            need({i for i, x in enumerate(pages) if x is None} == s.holes and a.nholes[b] == len(s.holes),
                 "holes", lambda: f"{what}: slot {b} {pages} ({a.nholes[b]} counted) for {s.ids}")
            for i, (x, y) in enumerate(zip(pages, s.ids)):
                if y is None:
                    continue
                holders[x] += 1
                need(phys.setdefault(y, x) == x and ident.setdefault(x, y) == y, "page identity",
                     lambda: f"{what}: slot {b} page {i} is physical {x} with identity {y}; {phys}")
                need(i >= ceil_div(s.L, P) or table[b][i] == x, "device table",
                     lambda: f"{what}: slot {b} page {i}: {table[b][i]} on the device, {x} on the host")
        need(all(a.refcount[x] == holders[x] for x in range(a.num_pages)), "reference counts",
             lambda: f"{what}: {a.refcount} for holders {dict(holders)}")
        need(sorted(list(a._free) + list(holders)) == list(range(a.num_pages)), "free list",
             lambda: f"{what}: free {a._free}, held {sorted(holders)}")
        k4, ks, vt, vs = (t.cpu() for t in p.kv)
        vtail, tpp = p.vtail.cpu(), P // 64
        for b, s in enumerate(m.seqs):
            if not s.L:
                continue
            e4, es, et, ev = m.expected(b)
            nt = ceil_div(s.L, 64)
            for i in range(ceil_div(s.L, P)):
                if s.ids[i] is None:
                    continue
                x, r0, r1, t0, t1 = table[b][i], i * P, min(s.L, (i + 1) * P), i * tpp, min(nt, (i + 1) * tpp)
                where = f"{what}: slot {b} page {i} (physical {x})"
                need(torch.equal(k4[x, :, :r1 - r0], e4[:, r0:r1]) and torch.equal(ks[x, :, :r1 - r0], es[:, r0:r1]),
                     "K bytes", where)
                need(torch.equal(vs[x, :, :t1 - t0], ev[:, t0:t1]), "V scales", where)
                need(torch.equal(vt[x, :, :t1 - t0], et[:, t0:t1]), "V bytes", where)
            need(torch.equal(vtail[b, :, :s.L % 64], s.v[:, s.L - s.L % 64:]), "vtail", f"{what}: slot {b}")

    # ---------------------------------------------------------------------------- attended
    def twin(self):
        """A fresh pool with ascending pages, no forks and no holes that holds the model's rows, written by
        one padded append."""
        key = tuple(s.version for s in self.m.seqs)
        if self._twin[0] != key:
            sp, m = self.sp, self.m
            t = self.be.allocate(sp.slots * m.maxp, sp.P, sp.slots, HKV, m.maxp, None, None)
            n = max(m.lengths)
            k = torch.full((sp.slots, HKV, n, D), 777.0, dtype=torch.float16)
            v = torch.full((sp.slots, HKV, n, D), -555.0, dtype=torch.float16)
            for b, s in enumerate(m.seqs):
                if s.L:
                    k[b, :, :s.L], v[b, :, :s.L] = s.k, s.v
            t.append(self.dev(k), self.dev(v), counts=m.lengths)
            self._twin = (key, t)
        return self._twin[1]

    def attended(self, op, out, what=""):
        if op is None:
            return
        O, lse = self.call(self.pool, op) if out is None else out
        mode = op["mode"]
        need(bool(torch.isfinite(lse).all()) and bool(torch.isfinite(O).all()), "attention is finite",
             f"{what} {mode}")
        TO, Tl = self.call(self.twin(), op, share=False)
        need(torch.equal(O, TO) and torch.equal(lse, Tl), "attention equals the twin pool's",
             lambda: f"{what} {name_of(op)}: O differs by {(O.float() - TO.float()).abs().max():.3e}, lse by "
                     f"{(lse - Tl).abs().max():.3e}")
        if mode == "touched" or mode in self.restated:
            return
        self.restated.add(mode)
        first, worst = 0, [0.0, 0.0, 0.0]
        for j, (b, n) in enumerate(zip(op["ids"], op["q_lens"])):
            s = self.m.seqs[b]
            q = self.q_of(op)[first:first + n]
            par = None if op["trees"] is None else op["trees"][j]
            RO, Rl = restated(mode, q, s.k, s.v, op["causal"], op["kps"], op["window"], op["sinks"], par)
            Oj, lj = O[first:first + n].float(), lse[first:first + n]
            fig = ((Oj - RO.float()).abs().max().item(), (lj - Rl).abs().max().item(),
                   ((Oj - RO.float()).norm() / RO.float().norm()).item())
            worst = [max(x, y) for x, y in zip(worst, fig)]
            first += n
        self.worst[mode] = worst
        self.log(f"MXFP4-LIFE {mode} seed={self.sp.seed} P={self.sp.P} op={self.n} O {worst[0]:.3e} lse "
                 f"{worst[1]:.3e} relL2 {worst[2]:.3e}")
        need(worst[0] <= BARS[0] and worst[1] <= BARS[1] and worst[2] <= BARS[2], "attention against the restatement",
             f"{what} {name_of(op)}: {worst}")

    # ---------------------------------------------------------------------------- the ops layer
    def operators(self):
        """One call of each operator form the final state allows must equal the Python call bit for bit."""
        if self.be.ops_varlen is None:
            return []
        g, done = _Gen(self.sp), []
        g.m, g.n = self.m, self.sp.n_ops
        g.rng = random.Random(self.sp.seed)
        for mode in ("causal", "window", "shared", "tree"):
            for _ in range(20):
                op = g.attend(mode)
                if op and op["mode"] == mode and not self.m.refusal(op):
                    O, lse = self.call(self.pool, op)
                    XO, Xl = self.call(self.pool, op, fn=self.be.ops_varlen)
                    need(torch.equal(O, XO) and torch.equal(lse, Xl), "the operator equals the Python call",
                         f"seed={self.sp.seed} P={self.sp.P} {name_of(op)}")
                    done.append(mode)
                    break
        for cfg in range(2 if self.sp.steps and self.be.ops_step else 0):
            ids = g._steppable(cfg)
            if not ids or self.m.refusal(g._step_op(cfg, ids)):     # (the pool may be out of pages)
                continue
            op = {**g._step_op(cfg, ids), "how": "eager", "rope": False}
            k, v, q = (self.dev(t) for t in step_rows(op["seed"], self.sp.slots))
            pairs = self.be.ops_step(self.pool, (op["kps"], op["window"], op["sinks"]), ids, k, v, q)
            need(all(x.dtype == y.dtype and torch.equal(x, y) for x, y in pairs),
                 "the operator equals the Python call", f"seed={self.sp.seed} P={self.sp.P} {name_of(op)}")
            self.m.apply(op)
            self.check(f"seed={self.sp.seed} P={self.sp.P} operators {name_of(op)}")
            done.append(f"step cfg{cfg}")
        return done

    def run(self, ops):
        for op in ops:
            self.step(op)
        return self
