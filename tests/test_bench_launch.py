"""bench.py's launcher and its configs[1] input, on the CPU.

- `python bench.py --gpus N` (no torch.distributed launcher) must start N ranks
  itself and report them; under a launcher WORLD_SIZE must equal --gpus
  (VERDICT r3 item 2).  `--check-launch` runs the launch and the candidate
  sharding (k -> rank k % world, batch.cpp:183-187) over gloo without GPU work.
- The steady synthetic sequence the headline uses holds 10k +- 10 % FAST
  keypoints on every candidate at bench.py's one threshold (configs[1]: 1080p,
  10k kpts/frame; the reference uses one featureExtractingThreshold for the
  whole batch, batch.cpp:245-253).  Checked with the oracle's FAST on a sample.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "slam-indoor-code_amd"))


def _run(args, env_extra=None):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, cwd=ROOT,
                          capture_output=True, text=True, timeout=180)


def _line(out):
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out
    return json.loads(lines[0])


def test_bench_gpus2_launches_two_ranks():
    r = _run(["--gpus", "2", "--check-launch"])
    assert r.returncode == 0, r.stderr[-2000:]
    d = _line(r.stdout)
    assert d["n_gpus"] == 2 and d["world_size"] == 2
    assert [x["rank"] for x in d["ranks"]] == [0, 1]
    assert [x["candidates"] for x in d["ranks"]] == [105, 105]


def test_bench_gpus3_ragged_shards():
    r = _run(["--gpus", "3", "--batch", "22", "--check-launch"])
    assert r.returncode == 0, r.stderr[-2000:]
    d = _line(r.stdout)
    assert d["n_gpus"] == 3
    assert [x["candidates"] for x in d["ranks"]] == [8, 7, 7]


def test_bench_world_mismatch_fails():
    r = _run(["--gpus", "1", "--check-launch"], {"WORLD_SIZE": "2", "RANK": "0"})
    assert r.returncode != 0
    assert "WORLD_SIZE=2" in r.stderr


def test_bench_single_rank_default():
    r = _run(["--check-launch"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert _line(r.stdout)["n_gpus"] == 1


def test_steady_sequence_holds_10k_keypoints():
    import slamhip
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_ffi as O
    spec = {}
    exec(compile("\n".join(l for l in open(os.path.join(ROOT, "bench.py")).read().splitlines()
                           if l.startswith(("THRESHOLD =", "SYNTH_PATH ="))), "bench", "exec"), spec)
    assert spec["SYNTH_PATH"] == slamhip.SYNTH_STEADY
    counts = []
    for k in (0, 1, 37, 70, 105, 140, 175, 209, 210):       # the query frame 0 and candidates 1..210
        f = slamhip.synth_frames(1920, 1080, k, 1, seed=1234, path=slamhip.SYNTH_STEADY)[0]
        counts.append(len(O.fast(f, spec["THRESHOLD"], True)))
    assert 9000 <= min(counts) and max(counts) <= 11000, counts
    assert abs(np.mean(counts) - 10000) <= 500, counts


def test_synth_paths_differ_and_drift_is_default():
    import slamhip
    a = slamhip.synth_frames(160, 120, 5, 1, seed=3)
    b = slamhip.synth_frames(160, 120, 5, 1, seed=3, path=slamhip.SYNTH_DRIFT)
    c = slamhip.synth_frames(160, 120, 5, 1, seed=3, path=slamhip.SYNTH_STEADY)
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    with pytest.raises(Exception):
        slamhip.synth_frames(160, 120, 5, 1, seed=3, path=7)


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_bench_plain_run_is_the_default(monkeypatch):
    """`--full` and `--dump-outputs` are off unless asked for; --steps counts timed steps (at least one)"""
    bench = _bench_module()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "0"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 0)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()


def test_bench_dump_outputs_layout(tmp_path):
    """--dump-outputs: one float .npy per result, records as one column per field"""
    from slamhip._lib import DMATCH_DTYPE, KEYPOINT_DTYPE
    bench = _bench_module()
    kps = np.zeros(3, KEYPOINT_DTYPE)
    kps["x"], kps["y"], kps["octave"] = [1.5, 2.5, 3.5], [4, 5, 6], [7, 8, 9]
    mts = np.zeros(2, DMATCH_DTYPE)
    mts["queryIdx"], mts["trainIdx"], mts["distance"] = [0, 2], [1, 0], [0.25, 0.5]
    desc = np.arange(3 * 128, dtype=np.float32).reshape(3, 128)
    d = str(tmp_path / "out")
    bench.dump_outputs(d, np.array([10, 11, 12, 13]), np.array([1, 2, 0, 3]), 1, (kps, mts), desc)
    got = {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}
    assert sorted(got) == ["good", "keypoint_counts", "match_counts", "winner_descriptors", "winner_keypoints",
                           "winner_matches"]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert got["keypoint_counts"].tolist() == [10, 11, 12, 13] and got["match_counts"].tolist() == [1, 2, 0, 3]
    assert got["good"].tolist() == [1]
    assert got["winner_keypoints"].shape == (3, 7) and got["winner_keypoints"][:, 0].tolist() == [1.5, 2.5, 3.5]
    assert got["winner_keypoints"][:, 5].tolist() == [7, 8, 9]
    assert got["winner_matches"].shape == (2, 4) and got["winner_matches"][:, 3].tolist() == [0.25, 0.5]
    assert np.array_equal(got["winner_descriptors"], desc)
    # no winner (good = -1): empty arrays, no descriptors file
    d2 = str(tmp_path / "none")
    bench.dump_outputs(d2, np.array([10]), np.array([0]), -1, None, None)
    assert sorted(os.listdir(d2)) == ["good.npy", "keypoint_counts.npy", "match_counts.npy", "winner_keypoints.npy",
                                      "winner_matches.npy"]
    assert np.load(os.path.join(d2, "winner_matches.npy")).size == 0


@pytest.mark.gpu
def test_bench_plain_run_line_and_outputs(tmp_path):
    """a plain run (small batch): the headline fields, nothing of `--full`, and the
    last timed step's results under --dump-outputs, consistent with each other"""
    out = str(tmp_path / "dump")
    r = _run(["--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "6", "--dump-outputs", out])
    assert r.returncode == 0, r.stderr[-2000:]
    d = _line(r.stdout)
    assert d["unit"] == "frames/s" and d["higher_is_better"] is True and d["metric"] and d["dtype"]
    assert d["steps"] == 2 and d["warmup"] == 1 and d["full"] is False
    assert d["ms_per_step"] > 0 and abs(d["value"] * d["ms_per_step"] * 1e-3 - 6) <= 1e-6 * 6
    for k in ("with_ba", "cpu_baseline", "rooflines", "kernels_sequential", "value_incl_h2d", "value_h2d_loop", "orb",
              "sift_4k", "ba_window", "sift_detector", "triangulation", "pipeline", "pipeline_b210"):
        assert d[k] is None, k
    assert d["kernels"]["sift_desc"]["launches"] == 2        # the timed steps and nothing else
    a = {f[:-4]: np.load(os.path.join(out, f)) for f in os.listdir(out)}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert a["keypoint_counts"].shape == (6,) and a["match_counts"].shape == (6,)
    assert d["config"]["min_kps"] == a["keypoint_counts"].min() and d["config"]["max_kps"] == a["keypoint_counts"].max()
    g = int(a["good"][0])
    assert 0 <= g < 6 and a["match_counts"][g] >= 500      # first fit found a candidate with the required matches
    assert len(a["winner_matches"]) == a["match_counts"][g]
    assert a["winner_keypoints"].shape == (d["config"]["prev_kps"], 7)
    assert a["winner_descriptors"].shape == (d["config"]["prev_kps"], 128)
    assert a["winner_matches"][:, 1].max() < len(a["winner_keypoints"])
