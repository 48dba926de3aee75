"""bench.py's launch contract on the CPU: `python bench.py --gpus N` without a launcher must start N ranks itself
(torch.distributed.run on 127.0.0.1) before touching the GPU, and rank 0 must print ONE JSON line."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True,
                          timeout=300)


def test_gpus_n_without_launcher_spawns_n_ranks():
    out = _run(["--gpus", "2", "--dry-run"])
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    doc = json.loads(lines[0])
    assert doc == {"dry_run": True, "world": 2, "ranks_seen": 2}


def test_single_gpu_default_needs_no_launcher():
    out = _run(["--dry-run"])
    assert out.returncode == 0, out.stderr[-2000:]
    assert json.loads(out.stdout.strip().splitlines()[-1]) == {"dry_run": True, "world": 1, "ranks_seen": 1}


def test_mismatched_world_size_fails_loudly():
    out = _run(["--gpus", "4", "--dry-run"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert out.returncode != 0 and "WORLD_SIZE=2" in (out.stderr + out.stdout)


def test_failing_rank_propagates_a_nonzero_exit():
    out = _run(["--gpus", "2", "--dry-run", "--steps", "not-a-number"])
    assert out.returncode != 0


def test_steps_below_one_is_refused():
    out = _run(["--dry-run", "--steps", "0"])
    assert out.returncode != 0 and "--steps" in out.stderr


def _fake_scan(n, seed):
    import numpy as np
    from frisk_amd.engine import ScanResult
    rng = np.random.default_rng(seed)
    status = rng.integers(0, 4, n).astype(np.uint32)
    kld, gc = rng.random(n), rng.random(n)
    kld[(status & 1) == 0] = gc[(status & 1) == 0] = np.nan        # as the kernels leave the windows the reference drops
    return ScanResult(seq_index=rng.integers(0, 424, n).astype(np.int32), start=np.arange(n, dtype=np.int64) * 1000 + 2 ** 40,
                      stop=np.arange(n, dtype=np.int64) * 1000 + 2 ** 40 + 5000, status=status, kld=kld, gc=gc)


def _load_dump(path):
    import numpy as np
    got = {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path))}
    assert set(got) == {"candidate", "seq_index", "start", "stop", "status", "kld", "gc"}
    assert all(a.dtype == np.float64 and np.all(np.isfinite(a)) for a in got.values())
    return got


def test_dump_outputs_is_bounded_seeded_and_exact(tmp_path):
    """--dump-outputs: the emitted rows only, as finite float64 arrays, 64 MB at most in all, the same sample of a large scan
    every time, values bit-equal to the rows they were taken from."""
    import numpy as np
    import bench
    res = _fake_scan(2 * bench.DUMP_ROWS + 54321, 1)
    assert res.kept.sum() > bench.DUMP_ROWS
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    assert bench.dump_outputs(a, res)["rows_written"] == bench.DUMP_ROWS
    bench.dump_outputs(b, res)
    assert sum(os.path.getsize(os.path.join(a, f)) for f in os.listdir(a)) <= 64 * 10 ** 6
    got, again = _load_dump(a), _load_dump(b)
    for name in got:
        assert np.array_equal(got[name], again[name], equal_nan=True), name
    idx = got["candidate"].astype(np.int64)
    assert len(idx) == bench.DUMP_ROWS and np.all(np.diff(idx) > 0) and idx[-1] < len(res) and np.all(res.kept[idx])
    for name in bench.DUMP_COLUMNS:
        assert np.array_equal(got[name], getattr(res, name)[idx].astype(np.float64), equal_nan=True), name
    assert np.array_equal(got["start"].astype(np.int64), res.start[idx])


def test_dump_outputs_writes_every_emitted_row_of_a_small_scan(tmp_path):
    import numpy as np
    import bench
    res = _fake_scan(1000, 2)
    bench.dump_outputs(str(tmp_path), res)
    got = _load_dump(str(tmp_path))
    kept = np.nonzero(res.kept)[0]
    assert np.array_equal(got["candidate"], kept)
    assert np.array_equal(got["kld"], res.kld[kept]) and np.array_equal(got["gc"], res.gc[kept])
