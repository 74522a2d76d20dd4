"""bench.py's output contract (one JSON line on rank 0) on a small shape, run as the driver runs it:
a child process on the GPU.  The numbers themselves are measured elsewhere (profiles/)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEADLINE = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
            "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config")
FULL_ONLY = ("bf16", "int8_fwd", "kernel_ms", "mxfp4_fwd", "configs", "without_gather", "roofline",
             "cpu_baseline")


def _bench(*args):
    r = subprocess.run([sys.executable, "bench.py", "--steps", "2", "--warmup", "1", "--shape",
                        "1,4,1024,128", *args], cwd=ROOT, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    for key in HEADLINE:
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["value"] > 0
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and "workload" in d["config"]
    assert "(1,4,1024,128)" in d["config"]["workload"]
    assert d["unit"] == "TFLOP/s" and d["dtype"] == "int8" and d["ms_per_step"] > 0
    # value is the credited work of one step over ms_per_step
    assert abs(d["value"] - 14.0 * 4 * 1024 * 1024 * 128 / (d["ms_per_step"] * 1e-3) / 1e12) \
        <= 1e-9 * d["value"]
    return d


def test_bench_json_contract():
    d = _bench("--full", "--cpu-seconds", "1")
    for key in FULL_ONLY:
        assert key in d, key
    rf = d["roofline"]
    assert rf["bound"] in ("hbm", "mfma") and rf["unit"] in ("GB/s", "TFLOP/s")
    assert 0 < rf["frac"] < 1 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-9
    cb = d["cpu_baseline"]
    assert cb["value"] > 0 and cb["kind"] in ("port", "reference") and cb["cores"] >= 1
    assert cb["logical_cpus"] >= cb["cores"] and "cpu_model" in cb
    assert d["bf16"]["value"] > 0 and d["kernel_ms"]["int8_attn_fwd_kernel"] > 0


def test_bench_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    """A plain run reports the headline alone, and --dump-outputs writes what its last timed step
    computed: float32 arrays that equal, bit for bit, the same step run here on the same seeded
    inputs (so the inputs are the same from process to process)."""
    import bench
    from quantizedattention_amd.attention_int8 import _int8_backward, _int8_forward
    out = tmp_path / "dump"
    d = _bench("--dump-outputs", str(out))
    for key in FULL_ONLY:
        assert key not in d, key
    shape = (1, 4, 1024, 128)
    (q, k, v, dO), _ = bench.make_inputs(3, "1,4,1024,128", 1, 0, torch.device("cuda", 0))
    O, lse, qi, kiT, vi, sq, sk, sv, km, qb, kb = _int8_forward(q, k, v, smooth=True, images=True)
    dq, dk, dv = _int8_backward(dO, qi, sq, kiT, sk, vi, sv, O, lse, qb, kb)
    want = {"O": O, "lse": lse, "dq": dq, "dk": dk, "dv": dv}
    assert sorted(os.listdir(out)) == sorted(n + ".npy" for n in want)
    for name, t in want.items():
        got = np.load(out / f"{name}.npy")
        assert got.dtype == np.float32 and got.shape == tuple(t.shape), name
        assert np.array_equal(got, t.float().cpu().numpy()), name
    assert want["O"].shape == shape and np.isfinite(np.load(out / "dq.npy")).all()
