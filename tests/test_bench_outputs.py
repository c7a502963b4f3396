"""bench.py --dump-outputs / --full: a plain run times its steps and writes what the last one
returned (float arrays within the size budget, identical from run to run); the CPU baseline and
the kernel pass with its rooflines run only with --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "2", "--warmup", "2", "--batch", "3", "--n-az", "300"]
NAMES = {"mask_pose", "bg_mask", "plane_count", "plane_xyzi", "plane_normal", "plane_normal_valid",
         "pose_rel", "pose_abs"}


def test_sample_is_fixed_and_ascending():
    import bench
    assert np.array_equal(bench._sample(10, 20, 1), np.arange(10))
    s = bench._sample(100000, 500, 1)
    assert s.shape == (500,) and s.min() >= 0 and s.max() < 100000 and np.all(np.diff(s) >= 0)
    assert np.array_equal(s, bench._sample(100000, 500, 1))
    assert not np.array_equal(s, bench._sample(100000, 500, 2))


def test_dump_outputs_keeps_dtype_and_budget(tmp_path):
    import bench
    ok = {"a": np.zeros((4, 7)), "b": np.ones(5, dtype=np.float32)}
    bench.dump_outputs(str(tmp_path / "d"), ok)
    assert sorted(os.listdir(tmp_path / "d")) == ["a.npy", "b.npy"]
    assert np.load(tmp_path / "d" / "b.npy").dtype == np.float32
    with pytest.raises(RuntimeError):
        bench.dump_outputs(str(tmp_path / "e"), {"i": np.zeros(3, dtype=np.int32)})
    with pytest.raises(RuntimeError):
        bench.dump_outputs(str(tmp_path / "f"), {"big": np.zeros(bench.DUMP_MAX_BYTES // 8 + 1)})
    assert not (tmp_path / "e").exists() and not (tmp_path / "f").exists()


def test_full_is_off_by_default():
    import bench
    assert bench.parse([]).full is False and bench.parse([]).dump_outputs is None
    assert bench.parse(["--full"]).full is True


def test_long_runs_walk_the_resident_frames_back_and_forth():
    import bench
    assert [bench.reflect(k, 4) for k in range(14)] == [0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1]
    assert [bench.reflect(k, 106) for k in range(106)] == list(range(106))
    for m in (3, 4, 130):       # every step pairs two neighbouring frames
        assert all(abs(bench.reflect(k + 1, m) - bench.reflect(k, m)) == 1 for k in range(5 * m))
    a = bench.parse([])
    a.batch = 256
    # the no-flag shape: 737 MB per frame; 100 steps + 5 warmup + frame 0 fit, 5000 steps do not
    assert bench.resident_frames(a, 106) == 106
    m = bench.resident_frames(a, 5006)
    assert 106 <= m and m * 256 * 120000 * 24 <= 96e9
    f = bench.Frames(list("abcd"))
    assert len(f) == 4 and "".join(f[k] for k in range(8)) == "abcdcbab"
    # pairs (a b) (b c) (c d) | (d c) (c b) (b a) | (a b): the walk turns at steps 4 and 7
    assert [k for k in range(9) if f.turns(k)] == [4, 7]


def test_invert_poses_is_the_rigid_inverse():
    import torch
    import bench
    g = torch.Generator().manual_seed(3)
    q = torch.randn(5, 4, generator=g, dtype=torch.float64)
    pose = torch.cat([q / q.norm(dim=1, keepdim=True), torch.randn(5, 3, generator=g, dtype=torch.float64)], 1)

    def apply(p, x):            # R(q) x + t, q = (x, y, z, w)
        u, w = p[:, :3], p[:, 3:4]
        c = torch.cross(u, x, dim=1)
        return x + 2.0 * (w * c + torch.cross(u, c, dim=1)) + p[:, 4:]

    x = torch.randn(5, 3, generator=g, dtype=torch.float64)
    inv = pose.clone()
    bench.invert_poses(inv)
    assert torch.allclose(apply(inv, apply(pose, x)), x, atol=1e-12)
    assert torch.allclose(apply(pose, apply(inv, x)), x, atol=1e-12)


def _bench(*extra):
    r = subprocess.run([sys.executable, "bench.py", *SMALL, *extra], cwd=REPO, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_its_last_step(dev, tmp_path):
    runs = []
    for name in ("a", "b"):
        line = _bench("--dump-outputs", str(tmp_path / name))
        assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["unit"] == "frames/s"
        assert line["value"] == pytest.approx(3 * 1e3 / line["ms_per_step"])
        assert line["full"] is False and line["cpu_baseline"] is None
        assert line["kernels"] == {} and line["roofline"] is None
        d = {f[:-4]: np.load(tmp_path / name / f) for f in os.listdir(tmp_path / name)}
        assert set(d) == NAMES
        assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in d.values())
        runs.append(d)
    a, b = runs
    assert all(np.array_equal(a[k], b[k]) for k in NAMES)
    # the arrays are the step's results, not buffers left as allocated
    count = a["plane_count"]
    assert a["mask_pose"].shape == (3, 25) and (a["mask_pose"][:, 16] == 0).all()
    assert count.shape == (3,) and (count > 100).all()
    live = np.abs(a["plane_xyzi"][:, :, :3]).sum(axis=2) > 0
    assert np.array_equal(live.sum(axis=1), np.minimum(count, live.shape[1]))
    nn = np.linalg.norm(a["plane_normal"], axis=2)
    assert np.array_equal(nn > 0, a["plane_normal_valid"] > 0) and a["plane_normal_valid"].sum() > 100
    assert set(np.unique(a["bg_mask"])) <= {0.0, 1.0} and 0.5 < a["bg_mask"].mean() < 1.0
    assert np.allclose(np.linalg.norm(a["pose_abs"][:, :4], axis=1), 1.0, atol=1e-9)
    assert np.abs(a["pose_rel"][:, 4:]).max() > 1e-3


@pytest.mark.gpu
def test_more_steps_than_resident_frames(dev, tmp_path):
    """9 steps over 3 resident frames: the run completes, reports its steps, and every pair it
    registered was a pair of neighbouring frames.  Full 120k-point scans (8.6 MB per frame of 3
    sequences): the 19k-point scans of the other cases do not constrain the registration along the
    street, forwards or backwards."""
    line = _bench("--steps", "7", "--n-az", "1875", "--resident-gb", "0.03", "--dump-outputs", str(tmp_path / "d"))
    assert line["steps"] == 7 and line["ms_per_step"] > 0
    assert line["config"]["frame_window"]["resident_frames"] == 3
    assert line["config"]["frame_window"]["frames_per_sequence"] == 10
    pose = np.load(tmp_path / "d" / "pose_abs.npy")
    assert np.isfinite(pose).all() and np.allclose(np.linalg.norm(pose[:, :4], axis=1), 1.0, atol=1e-9)
    # 2 + 7 steps walk frames 0 1 2 1 0 1 2 1 0 (ssf.synth EGO_SPEED = 1 m per frame): the
    # accumulated pose ends nearer to frame 0's than to any other frame's (half the spacing), and
    # the last pair (frame 1 -> frame 0) moved one frame backwards, nearer to -1 m than to 0 or -2
    rel = np.load(tmp_path / "d" / "pose_rel.npy")
    assert np.linalg.norm(pose[:, 4:], axis=1).max() < 0.5
    assert np.abs(rel[:, 4] + 1.0).max() < 0.5 and np.abs(rel[:, 5:]).max() < 0.5
    assert (np.load(tmp_path / "d" / "mask_pose.npy")[:, 16] == 0).all()


@pytest.mark.gpu
def test_full_run_adds_the_kernel_pass(dev):
    # two pass steps: the first has no previous frame to register against (no k_solve launch)
    line = _bench("--full", "--no-cpu-baseline", "--kernel-pass", "2")
    assert line["full"] is True and line["steps"] == 2 and line["ms_per_step"] > 0
    assert "k_mask_pose" in line["kernels"] and "k_solve" in line["kernels"]
    assert line["roofline"]["kernel"] == "k_mask_pose" and line["mask_passes_per_frame"] > 0
