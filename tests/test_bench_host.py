"""Host logic of bench.py (no GPU): the --gpus N launcher, the config-4 sharding of the global
problem, the CPU-baseline core accounting and the traffic source hash."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_gpus_n_without_torchrun_spawns_ranks(monkeypatch):
    seen = {}

    def fake_call(cmd):
        seen["cmd"] = cmd
        return 7
    monkeypatch.setattr(bench.subprocess, "call", fake_call)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "5"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 7
    cmd = seen["cmd"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node=4" in cmd
    assert "--master-addr=127.0.0.1" in cmd and cmd[-4:] == ["--gpus", "4", "--steps", "5"]


def test_world_size_mismatch_fails_fast(monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "8"])
    with pytest.raises(SystemExit, match="WORLD_SIZE=2"):
        bench.main()


@pytest.mark.parametrize("world", [1, 2, 4, 8])
def test_config4_shards_cover_the_global_problem(world):
    """Rank r's heads are rows [r*256/N, (r+1)*256/N) of the global (8*32) heads: together exactly
    the global problem, each rank's slice contiguous."""
    from quantizedattention_amd.sharded import shard_for
    covered = []
    for r in range(world):
        sh = bench.shard_for(8, 32, world, r)
        assert sh == shard_for(8, 32, world, r) and sh.n == 256 // world
        covered += list(range(sh.bh0, sh.bh1))
    assert covered == list(range(256))


def test_cpu_info_and_threads():
    info = bench.cpu_info()
    assert info["logical_cpus"] == os.cpu_count() and info["affinity_cpus"] >= 1
    assert info["physical_cores"] is None or 1 <= info["physical_cores"] <= info["logical_cpus"]


def test_source_hash_tracks_the_kernel_sources():
    h = bench.source_hash()
    assert len(h) == 64 and h == bench.source_hash()


def test_chunk_heads_match_the_step():
    """bench.py times the record backward as the step launches it: chunks of >= 512 dK+dV
    workgroups (attention_int8._ws_chunk), 32 heads at config 3 -> 4 launches per step."""
    assert bench.ws_chunk_heads(128, 4096) == 32
    assert bench.ws_chunk_heads(4, 256) == 4        # small problems: one launch over all heads


def test_plain_run_is_the_default_and_steps_are_checked(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "0"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 0
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()


def test_timed_runs_warmup_then_exactly_steps_calls(monkeypatch):
    monkeypatch.setattr(bench.torch.cuda, "synchronize", lambda: None)
    calls = []
    t = bench.timed(lambda: calls.append("step"), 5, 2, 1, last=lambda: calls.append("last"))
    assert calls == ["step"] * 6 + ["last"] and t >= 0
    calls.clear()
    bench.timed(lambda: calls.append("step"), 1, 0, 1)
    assert calls == ["step"]


def test_dump_samples_large_outputs_at_fixed_indices(tmp_path):
    """An output above bench.DUMP_MAX_ELEMS elements is stored as a fixed seeded sample: the same
    sorted flat indices on every call, the values at them in float32; five such arrays (O, lse, dq,
    dk, dv) stay under 64 MB."""
    import numpy as np
    n = bench.DUMP_MAX_ELEMS + 12345
    x = torch.arange(n, dtype=torch.float32).view(-1, 5)
    bench.dump_outputs(str(tmp_path / "a"), {"x": x.half().float(), "small": x[:7].double()})
    bench.dump_outputs(str(tmp_path / "b"), {"x": x})
    a, b = np.load(tmp_path / "a" / "x.npy"), np.load(tmp_path / "b" / "x.npy")
    assert b.dtype == np.float32 and b.shape == (bench.DUMP_MAX_ELEMS,)
    # drawn with replacement from barely more indices than the sample holds: ~1 - 1/e of them distinct
    assert (np.diff(b) >= 0).all() and 0 <= b[0] and b[-1] < n and len(np.unique(b)) > 0.6 * len(b)
    assert np.array_equal(a, x.half().float().view(-1).numpy()[b.astype(np.int64)])   # same indices
    small = np.load(tmp_path / "a" / "small.npy")
    assert small.dtype == np.float32 and np.array_equal(small, x[:7].numpy())
    assert 5 * 4 * bench.DUMP_MAX_ELEMS <= 64e6


def test_profile_tools_tell_grids_apart(tmp_path):
    """tools/profile_summary.key_of separates the chunk-sized and one-pass launches of the same
    kernel by their grids, and tools/trace_summary.py groups a kernel trace per (kernel, grid)."""
    import csv
    import subprocess
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from profile_summary import key_of, workgroups
    name = "void qattn::int8_bwd_kernel<128, 3, false, true>(signed char const*)"
    assert key_of(name, 512) == "int8_bwd_dkdv_kernel<dK+dV, dS out>"
    assert key_of(name, 2048) == "int8_bwd_dkdv_kernel<dK+dV, dS out, one pass>"
    fwd = "void qattn::int8_attn_fwd_kernel<128, false, false, true, false, true>(signed char const*)"
    assert key_of(fwd, 4096) == "int8_attn_fwd_kernel"
    fwd = "void qattn::int8_attn_fwd_kernel<128, false, false, false, false, false>(signed char const*)"
    assert key_of(fwd, 4096) == "int8_attn_fwd_kernel<q_i8 in>"
    assert workgroups({"Grid_Size_X": "262144", "Workgroup_Size_X": "512"}) == 512
    d = tmp_path / "trace"
    d.mkdir()
    cols = ["Kernel_Name", "Start_Timestamp", "End_Timestamp", "Grid_Size_X", "Workgroup_Size_X",
            "LDS_Block_Size"]
    rows = [(name, 0, 500, 262144, 512, 1024), (name, 1000, 1510, 262144, 512, 1024),
            (name, 2000, 4000, 1048576, 512, 1024)]
    with open(d / "run_kernel_trace.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(cols)
        w.writerows(rows)
    out = tmp_path / "shapes.csv"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "trace_summary.py"), str(d), str(out)],
                   check=True, capture_output=True)
    got = {r["bench_key"]: r for r in csv.DictReader(open(out))}
    assert got["int8_bwd_dkdv_kernel<dK+dV, dS out>"]["Calls"] == "2"
    assert got["int8_bwd_dkdv_kernel<dK+dV, dS out>"]["AverageNs"] == "505"
    assert got["int8_bwd_dkdv_kernel<dK+dV, dS out, one pass>"]["AverageNs"] == "2000"
