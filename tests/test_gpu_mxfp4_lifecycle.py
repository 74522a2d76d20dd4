"""The seeded lifecycle fuzz of tests/mxfp4_lifecycle.py on the real paged MX-FP4 cache (PagedKVFP4: append,
append_packed, fork, free, trim, checkpoint / rollback / accept; attention_mxfp4_varlen_paged with window, sinks,
share_prefix and tree; attention_mxfp4_decode_paged), all on one long-lived pool whose pages are scattered.

Each test replays one schedule of ``mxfp4_lifecycle.SCHEDULES`` -- the list whose coverage
tests/test_mxfp4_lifecycle_model.py asserts -- with the model's ``check`` after every operation and ``attended``
for every attend operation and every touched slot.  Every illegal operation of a schedule is one the Python layer
refuses before any launch.  At the end of a schedule one call of each operator form the final state allows
(``ops.mxfp4_varlen_paged``: torch.ops.qattn.mxfp4_varlen_paged, _window, _shared, _tree) must equal the Python
call bit for bit.

The schedules of ``mxfp4_lifecycle.STEP_SCHEDULES`` also draw decode steps (``DecodeStep``: ``prepare``, ``append``,
``attend``), eager and graph-replayed, plain and windowed, with and without ``rope=``, between all of the above on
the same pool: ``Backend.step`` owns one ``DecodeStep`` per configuration and one captured graph per
(configuration, rope), captured once and replayed for every later "graph" step of the schedule, whatever was
forked, freed, trimmed or rolled back in between.  For those schedules ``ops.mxfp4_decode_step_plan`` and
``ops.mxfp4_decode_step`` join the operator forms.
"""
import time

import pytest
import torch

import mxfp4_lifecycle as LC

pytestmark = pytest.mark.gpu


def _pool_tensors(pool):
    return (*pool.kv, pool.vtail, pool.lens, pool.block_table)


class Backend:
    device = "cuda"

    def __init__(self):
        self.steps, self.static, self.graphs, self.ropes, self.warm = {}, {}, {}, {}, set()

    def _step(self, pool, cfg):
        """The DecodeStep of configuration ``cfg`` = (kps, window, sinks) and its static k, v, q."""
        if cfg not in self.steps:
            from quantizedattention_amd.kv_cache_mxfp4 import DecodeStep
            kps, W, S = cfg
            N = pool.alloc.max_seqs
            self.steps[cfg] = DecodeStep(N, LC.MAX_TOKENS[pool.page_tokens], LC.HQ, LC.HKV, "cuda",
                                         keys_per_split=kps, window=W, sinks=S)
            self.static[cfg] = tuple(torch.zeros((N, h, LC.D), dtype=torch.float16, device="cuda")
                                     for h in (LC.HKV, LC.HKV, LC.HQ))
        return self.steps[cfg]

    def step_kps(self, cfg):
        return self.steps[cfg].kps

    def _rope(self, rope):
        from quantizedattention_amd.kv_cache_mxfp4 import Rope
        if rope is not None and rope[1] not in self.ropes:
            self.ropes[rope[1]] = Rope(rope[0].cuda(), interleaved=rope[1])
        return None if rope is None else self.ropes[rope[1]]

    def step(self, pool, cfg, ids, k, v, q, rope, how):
        """One decode step.  The first step of a configuration runs eagerly (the warm-up), and so does every
        "eager" one; the first "graph" step after the warm-up captures ``append`` + ``attend`` on the static k, v,
        q -- one linear chain, and a capture launches nothing, so the pool must be as it was -- and every "graph"
        step is ``prepare``, three copies into the static inputs and a replay."""
        step, rope = self._step(pool, cfg), self._rope(rope)
        step.prepare(pool, ids)     # (a refused step warms nothing up)
        if cfg not in self.warm or how == "eager":
            self.warm.add(cfg)
            return step.append(pool, k, v, rope=rope).attend(pool, q, rope=rope)
        key = (cfg, rope is not None)
        sk, sv, sq = self.static[cfg]
        if key not in self.graphs:
            before = [t.clone() for t in _pool_tensors(pool)]
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = step.append(pool, sk, sv, rope=rope).attend(pool, sq, rope=rope)
            assert all(torch.equal(x, y) for x, y in zip(before, _pool_tensors(pool))), "the capture moved the pool"
            self.graphs[key] = (graph, out)
        graph, out = self.graphs[key]
        sk.copy_(k), sv.copy_(v), sq.copy_(q)
        graph.replay()
        return out

    def ops_step(self, pool, cfg, ids, k, v, q):
        """One eager step through the operators beside the Python entries -> the pairs that must be equal: the
        plan's four tables, O and lse."""
        import quantizedattention_amd.ops as ops
        step = self._step(pool, cfg)
        step.prepare(pool, ids)
        tabs = ops.mxfp4_decode_step_plan(step, pool)       # before the append: the lengths it reads
        step.append(pool, k, v)
        pairs = [(mine.clone(), op) for mine, op in zip((step.seq_tab, step.tiles, step.pos, step.seq_rec), tabs)]
        XO, Xl = ops.mxfp4_decode_step(q, step, pool, seq_rec=tabs[3])
        O, lse = step.attend(pool, q)
        return pairs + [(O, XO), (lse, Xl)]

    @staticmethod
    def allocate(num_pages, P, slots, Hkv, max_pages, k_mean, free_order):
        from quantizedattention_amd.kv_cache_mxfp4 import PagedKVFP4
        return PagedKVFP4.allocate(num_pages, P, slots, Hkv, max_pages, "cuda", k_mean, free_order)

    @staticmethod
    def varlen(q, pool, ids, q_lens, **kw):
        from quantizedattention_amd.kv_cache_mxfp4 import attention_mxfp4_varlen_paged
        return attention_mxfp4_varlen_paged(q, pool, ids, q_lens, **kw)

    @staticmethod
    def ops_varlen(q, pool, ids, q_lens, **kw):
        import quantizedattention_amd.ops as ops
        return ops.mxfp4_varlen_paged(q, pool, ids, q_lens, **kw)

    @staticmethod
    def decode(q, pool, causal, keys_per_split):
        from quantizedattention_amd.kv_cache_mxfp4 import attention_mxfp4_decode_paged
        return attention_mxfp4_decode_paged(q, pool, causal=causal, keys_per_split=keys_per_split)

    @staticmethod
    def sync():
        torch.cuda.synchronize()


def _replay(seed, P, smoothed, operators=True):
    t0 = time.perf_counter()
    if (seed, P, smoothed) in LC.STEP_SCHEDULES:
        sp, ops = LC.step_spec(seed, P, smoothed), LC.step_schedule(seed, P, smoothed)
    else:
        sp, ops = LC.spec(seed, P, smoothed=smoothed), LC.schedule(seed, P, smoothed=smoothed)
    be = Backend()
    h = LC.Harness(be, sp).run(ops)
    assert h.n == sp.n_ops and h.worst and ("step" in h.worst) == sp.steps
    if sp.steps:    # every "graph" step after a configuration's warm-up was a replay of one of these
        print(f"MXFP4-LIFE graphs seed={seed} P={P}: {sorted(map(str, be.graphs))}")
        assert be.graphs and len(be.graphs) <= 4
    if operators:
        print(f"MXFP4-LIFE operators seed={seed} P={P}: {h.operators()}")
    print(f"MXFP4-LIFE time seed={seed} P={P}: {time.perf_counter() - t0:.2f} s")
    return h


@pytest.mark.parametrize("seed,P,smoothed", LC.SCHEDULES + LC.STEP_SCHEDULES)
def test_lifecycle_schedule(lib, seed, P, smoothed):
    _replay(seed, P, smoothed)


@pytest.mark.parametrize("name", sorted(LC.regressions()))
def test_lifecycle_regression(lib, name):
    """The schedules the fuzz once failed on, named by their operations (mxfp4_lifecycle.regressions)."""
    sp, ops = LC.regressions()[name]
    h = LC.Harness(Backend(), sp).run(ops)
    assert h.n == len(ops)
    print(f"MXFP4-LIFE operators {name}: {h.operators()}")


def test_lifecycle_off_the_default_stream(lib):
    """Two schedules, and one with decode steps, on a stream of their own: append, fork, free, rollback and the
    packed call are stream-ordered and read nothing back, and so are ``prepare``'s uploads, the copies into a
    graph's static inputs and its replay, so only the checker synchronises."""
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for seed, P, smoothed in (LC.SCHEDULES[0], LC.SCHEDULES[-1], LC.STEP_SCHEDULES[2]):
            _replay(seed, P, smoothed, operators=False)
    torch.cuda.synchronize()
