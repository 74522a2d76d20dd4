"""The seeded lifecycle fuzz of tests/mxfp4_lifecycle.py on the real paged MX-FP4 cache (PagedKVFP4: append,
append_packed, fork, free, trim, checkpoint / rollback / accept; attention_mxfp4_varlen_paged with window, sinks,
share_prefix and tree; attention_mxfp4_decode_paged), all on one long-lived pool whose pages are scattered.

Each test replays one schedule of ``mxfp4_lifecycle.SCHEDULES`` -- the list whose coverage
tests/test_mxfp4_lifecycle_model.py asserts -- with the model's ``check`` after every operation and ``attended``
for every attend operation and every touched slot.  Every illegal operation of a schedule is one the Python layer
refuses before any launch.  At the end of a schedule one call of each operator form the final state allows
(``ops.mxfp4_varlen_paged``: torch.ops.qattn.mxfp4_varlen_paged, _window, _shared, _tree) must equal the Python
call bit for bit.
"""
import time

import pytest
import torch

import mxfp4_lifecycle as LC

pytestmark = pytest.mark.gpu


class Backend:
    device = "cuda"

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
    sp = LC.spec(seed, P, smoothed=smoothed)
    h = LC.Harness(Backend, sp).run(LC.schedule(seed, P, smoothed=smoothed))
    assert h.n == sp.n_ops and h.worst
    if operators:
        print(f"MXFP4-LIFE operators seed={seed} P={P}: {h.operators()}")
    print(f"MXFP4-LIFE time seed={seed} P={P}: {time.perf_counter() - t0:.2f} s")
    return h


@pytest.mark.parametrize("seed,P,smoothed", LC.SCHEDULES)
def test_lifecycle_schedule(lib, seed, P, smoothed):
    _replay(seed, P, smoothed)


@pytest.mark.parametrize("name", sorted(LC.regressions()))
def test_lifecycle_regression(lib, name):
    """The schedules the fuzz once failed on, named by their operations (mxfp4_lifecycle.regressions)."""
    sp, ops = LC.regressions()[name]
    h = LC.Harness(Backend, sp).run(ops)
    assert h.n == len(ops)
    print(f"MXFP4-LIFE operators {name}: {h.operators()}")


def test_lifecycle_off_the_default_stream(lib):
    """Two schedules on a stream of their own: append, fork, free, rollback and the packed call are
    stream-ordered and read nothing back, so only the checker synchronises."""
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for seed, P, smoothed in (LC.SCHEDULES[0], LC.SCHEDULES[-1]):
            _replay(seed, P, smoothed, operators=False)
    torch.cuda.synchronize()
