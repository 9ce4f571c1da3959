"""bench.py as a launcher: `--gpus N` must either run N ranks or fail loudly -- never print a
1-GPU number labelled N.  Rehearsed on CPU: the stub render path uses the same process-group setup, FrameGather,
barriers and JSON plumbing as the GPU path, over gloo."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(args, env=None, timeout=300):
    e = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    e.update(env or {})
    return subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, env=e, timeout=timeout)


def test_plain_start_launches_its_own_ranks():
    r = _run(["--gpus", "2", "--stub-render", "--size", "72", "--row-block", "8", "--steps", "2", "--warmup", "1"])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1                       # rank 0 only
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["rccl_world"] == 2 and d["frame_ok"] is True


def test_three_ranks_ragged_partition():
    r = _run(["--gpus", "3", "--stub-render", "--size", "50", "--row-block", "16", "--steps", "1", "--warmup", "0"])
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert d["n_gpus"] == 3 and d["frame_ok"] is True


def test_world_size_mismatch_is_an_error():
    r = _run(["--gpus", "4", "--stub-render", "--size", "32"], env={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE=1" in r.stderr and not r.stdout.strip()


def test_more_gpus_than_the_node_has_fails_loudly():
    import torch
    have = torch.cuda.device_count()
    r = _run(["--gpus", str(max(have, 1) + 1), "--steps", "1", "--warmup", "0", "--no-cpu-baseline"])
    assert r.returncode != 0 and f"has {have} GPU" in r.stderr
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]       # no JSON line: nothing to misread


def test_a_failing_rank_fails_the_launch():
    # rank 1 cannot initialise (bad backend name): the launcher must return non-zero, not hang on rank 0's barrier
    r = _run(["--gpus", "2", "--stub-render", "--size", "32", "--backend", "no_such_backend"], timeout=120)
    assert r.returncode != 0


def test_dump_outputs_writes_the_gathered_frame(tmp_path):
    # the stub path hands --dump-outputs the frame rank 0 assembled: float32 .npy files, the whole frame when it is small
    import numpy as np
    r = _run(["--gpus", "2", "--stub-render", "--size", "72", "--row-block", "8", "--steps", "2", "--warmup", "1",
              "--dump-outputs", str(tmp_path)])
    assert r.returncode == 0, r.stderr[-2000:]
    rgba, idx = np.load(tmp_path / "rgba.npy"), np.load(tmp_path / "pixel_index.npy")
    assert rgba.dtype == np.float32 and idx.dtype == np.float64 and rgba.shape == (72 * 72, 4)
    assert np.array_equal(idx, np.arange(72 * 72))
    y, x = np.divmod(np.arange(72 * 72), 72)
    expect = (y[:, None] * 131 + x[:, None] * 7 + np.arange(4)[None, :] * 3) % 251
    assert np.array_equal(rgba, expect.astype(np.float32))


def test_dump_outputs_needs_a_timed_step():
    r = _run(["--stub-render", "--size", "32", "--steps", "0", "--dump-outputs", "unused"])
    assert r.returncode != 0 and "--steps >= 1" in r.stderr


def test_dump_sample_is_seeded_and_bounded():
    import bench
    import numpy as np
    a, b = bench.dump_sample_index(4096 * 4096), bench.dump_sample_index(4096 * 4096)
    assert np.array_equal(a, b) and a.size == bench.DUMP_PIXELS and np.all(np.diff(a) > 0) and a.max() < 4096 * 4096
    assert np.array_equal(bench.dump_sample_index(1000), np.arange(1000))


def test_dumped_final_alpha_is_finite_with_an_escaped_mask(tmp_path):
    # the library's final_alpha is NaN where a ray did not escape: the dump writes 0 there plus escaped = 0, and refuses
    # any array that is not finite
    import numpy as np
    import pytest
    import torch
    import bench
    fa, esc = bench.split_final_alpha(torch.tensor([0.5, float("nan"), 1.25, float("nan")]))
    assert fa.tolist() == [0.5, 0.0, 1.25, 0.0] and esc.tolist() == [1.0, 0.0, 1.0, 0.0]
    assert fa.dtype == esc.dtype == torch.float32
    with pytest.raises(ValueError):
        bench.write_outputs(str(tmp_path), {"final_alpha": np.array([0.5, np.nan], dtype=np.float32)})
    with pytest.raises(ValueError):
        bench.write_outputs(str(tmp_path), {"winding": np.array([1, 2], dtype=np.int16)})
