"""A plain bench.py run: --steps sets the number of timed steps (batches), the line carries the
headline figures only, and --dump-outputs writes the last timed step's per-packet results, which
must be the oracle's for that step's batch.  --full brings the readouts and the roofline back."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, V, NB, WARMUP, STEPS = 65536, 4096, 8, 5, 11   # 8 batches per launch: 11 steps = launches of 8 + 3


def _bench(extra):
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--config", "classifier", "--packets", str(N), "--vcpus", str(V),
           "--batches", str(NB), "--steps", str(STEPS), "--warmup", str(WARMUP)] + extra
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_times_the_steps_asked_for_and_dumps_the_last_step(gpu, tmp_path):
    import bench
    import oracle
    from mimic_amd import workloads as W

    d = _bench(["--dump-outputs", str(tmp_path)])
    assert d["steps"] == STEPS and d["warmup"] == WARMUP and d["n_gpus"] == 1
    assert d["config"]["batches_per_launch"] == 8 and d["launches"] == 2
    assert d["unit"] == "Mpkts/s" and d["higher_is_better"] is True and d["dtype"] == "u64"
    assert d["value"] > 0 and d["ms_per_step"] > 0
    # value and ms_per_step describe the same steps of N packets (ms_per_step is rounded to 1e-4 ms)
    assert abs(d["ms_per_step"] - N / (d["value"] * 1e6) * 1e3) <= 1e-4
    for k in ("roofline", "cpu_baseline", "host_resident", "insns_per_s", "counters_sum", "status_ok_frac"):
        assert k not in d, k
    assert sorted(os.listdir(tmp_path)) == ["r0.npy", "status.npy"]
    r0, st = np.load(tmp_path / "r0.npy"), np.load(tmp_path / "status.npy")
    assert r0.dtype == np.float64 and st.dtype == np.float32 and r0.shape == st.shape == (N,)
    b = (WARMUP + STEPS - 1) % NB   # the batch of the last timed step
    wl = bench.Workload("classifier", N, W.SEED + 1000 * b, 0, 1, b)
    p = W.prog_classifier()
    vm = oracle.OracleVM(64)
    mid = vm.map_create("verdicts", 6, 4, 8, 4)
    pid = vm.prog_load(p.name, p.raw, [(s, mid) for s, _ in p.relocs])
    o = vm.run_xdp_batch(pid, wl.buf, wl.off, wl.lens, W.schedule_cpu(N, 64, "interleaved"), write_back=False)
    vm.close()
    assert np.array_equal(r0, np.asarray(o["r0"]).astype(np.float64))
    assert np.array_equal(st, np.asarray(o["status"]).astype(np.float32))
    assert set(np.unique(r0).tolist()) == {1.0, 2.0}


def test_full_run_keeps_the_readouts(gpu):
    d = _bench(["--full", "--no-cpu-baseline"])
    assert d["steps"] == STEPS and d["launches"] == 2
    assert d["status_ok_frac"] == 1.0 and sum(d["counters_sum"]) == N * (WARMUP + STEPS)
    assert d["mean_insns_per_packet"] > 20 and d["roofline"]["avg_launch_ms"] > 0
    assert d["host_resident"]["ok_frac"] == 1.0 and "kernel_src_hash" in d["config"]
