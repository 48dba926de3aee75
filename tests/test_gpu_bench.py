"""bench.py on the GPU: --steps sets the timed steps, and --dump-outputs writes the rows the last timed step emitted - the same
rows a separate engine computes on the same seeded workload."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE = 0.02


def test_bench_dump_outputs_equal_a_separate_run(tmp_path):
    import bench
    from frisk_amd import Engine, synth
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "shard", "--shard-scale", str(SCALE),
                          "--steps", "3", "--warmup", "1", "--cpu-windows", "0", "--no-upload", "--no-extra",
                          "--dump-outputs", str(tmp_path)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    line = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    got = {name: np.load(str(tmp_path / (name + ".npy"))) for name in ("candidate",) + bench.DUMP_COLUMNS}
    # the bench's workload, rebuilt: one rank, shard 0 of the C5 shape at SCALE, the same seed and step
    lens = [max(1, int(x * SCALE)) for x in synth.c5_shard_lens(8, 0)]
    with Engine(bench.KMIN, bench.KMAX) as e:
        e.synth(lens, seed=0xC5, island_frac=0.02, n_frac=0.07, lower_frac=0.0, repeats_per_kb=0.0)
        e.profile_reset(); e.profile_add(); e.profile_finalize()
        res = e.scan(bench.W, bench.INC)
    kept = np.nonzero(res.kept)[0]
    assert line["dump_outputs"]["candidate_windows"] == len(res)
    assert line["dump_outputs"]["rows_written"] == len(kept) == line["config"]["rows_per_gpu_rank0"] > 0
    assert len(kept) <= bench.DUMP_ROWS and np.array_equal(got["candidate"], kept)
    for name in bench.DUMP_COLUMNS:
        assert got[name].dtype == np.float64 and np.all(np.isfinite(got[name])), name
        assert np.array_equal(got[name], getattr(res, name)[kept].astype(np.float64)), name
