"""bench.py's own output: the result line (compact, headline fields kept) and --dump-outputs (the arrays of the last timed step)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_result_line_keeps_the_headline_and_summarises_the_side_legs():
    import bench
    with open(os.path.join(ROOT, "profiles", "r06", "bench_n1.json")) as f:  # a full record of round 6 (34.7 kB as one line)
        record = json.loads(f.read().strip().splitlines()[-1])
    line = bench.result_line(record)
    assert len(json.dumps(line)) < 16384
    for k, v in record.items():
        if k not in bench.SIDE_LEGS:
            assert line[k] == v, k
    for k in ("value", "unit", "n_gpus", "steps", "warmup", "ms_per_step"):
        assert line[k] == record[k]
    assert line["closed_loop"]["value"] == record["closed_loop"]["value"]
    assert line["closed_loop"]["parity_vs_oracle_chain"] == record["closed_loop"]["parity_vs_oracle_chain"]
    assert line["other_configs"]["euroc"]["ms_per_step"] == record["other_configs"]["euroc"]["ms_per_step"]
    assert line["a13_alt"]["readings"]["shipped"]["value"] == record["a13_alt"]["readings"]["shipped"]["value"]


def test_steps_below_one_are_refused():
    run = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 2 and "--steps" in run.stderr


def test_help_prints_and_names_full():
    run = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "--full" in run.stdout, run.stderr[-2000:]


def _parse(monkeypatch, *argv):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py"] + list(argv))
    return bench.parse()


def test_a_plain_run_does_nothing_besides_its_headline(monkeypatch):
    """without --full nothing follows the timed steps, on any rank; the flags that narrow --full do not switch anything on"""
    import bench
    for argv in ([], ["--gpus", "1", "--steps", "10", "--warmup", "2"], ["--no-cpu-baseline"], ["--timing-steps", "8", "--cpu-frames", "64"]):
        args = _parse(monkeypatch, *argv)
        assert args.full is False
        for rank, world in ((0, 1), (0, 2), (1, 2)):
            assert not any(bench.extras(args, rank, world).values()), (argv, rank, world)


def test_full_runs_everything_and_its_flags_narrow_it(monkeypatch):
    import bench
    everything = {"kernel_times", "steady_state", "cpu_baseline", "other_configs"}
    on = lambda *argv, rank=0, world=1: {k for k, v in bench.extras(_parse(monkeypatch, "--full", *argv), rank, world).items() if v}  # noqa: E731
    assert on() == on("--gpus", "1", "--steps", "10", "--warmup", "2") == everything
    assert on("--no-steady-state") == everything - {"steady_state"}
    assert on("--no-cpu-baseline") == on("--cpu-frames", "0") == everything - {"cpu_baseline"}
    assert on("--no-other-configs") == everything - {"other_configs"}
    # the legs take the whole device and the host's cores: rank 0 of a 1-GPU run; the per-kernel pass runs on every rank
    assert on(rank=0, world=2) == on(rank=1, world=2) == {"kernel_times"}


@pytest.mark.gpu
def test_a_plain_run_prints_the_headline_alone(tmp_path):
    """bench.py end to end without --full at a small shape: the line holds the contract's fields and what the timed steps produced,
    none of the objects that take runs of their own; --dump-outputs still writes the last timed step"""
    import bench
    run = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "512",
                          "--keypoints", "1000", "--moving", "1000", "--max-fixed", "512", "--unique", "13", "--dump-outputs", str(tmp_path / "out")],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = [l for l in run.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert set(line) == {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
                         "data", "config", "dump_outputs"}
    assert not set(line) & set(bench.SIDE_LEGS)
    assert line["unit"] == "frames/s" and line["higher_is_better"] is True and line["n_gpus"] == 1 and line["steps"] == 2 and line["warmup"] == 1
    assert line["value"] > 0 and abs(line["value"] - 512 / (line["ms_per_step"] * 1e-3)) <= 1e-6 * line["value"]
    assert line["config"]["frames_per_step_per_gpu"] == 512 and line["dump_outputs"]["bytes"] > 0
    assert np.load(tmp_path / "out" / "pose.npy").shape == (512, 4, 4)


@pytest.mark.gpu
def test_dump_outputs_holds_what_the_last_step_computed(tmp_path):
    import torch
    import bench
    from srrg2_proslam_amd import configs, synthetic as syn
    w = bench.FrameWorkload(configs.get("kitti"), 0, 512, 1000, 1000, 512, 13, syn.seed_for(1, 0))
    stream = torch.cuda.Stream(device=w.dev)
    with torch.cuda.stream(stream):
        w.ctx.use_torch_stream()
        w.step()
        w.step()
        total = w.dump_outputs(str(tmp_path / "a"))
        X, n_corr = w.aframes.X.cpu().numpy(), w.aframes.n_corr.cpu().numpy()
        res = [w.aframes.result_of(b) for b in range(w.B)]
        w.step()
        w.dump_outputs(str(tmp_path / "b"))
        sample = np.load(tmp_path / "a" / "sample_frames.npy").astype(np.int64)
        corr = [w.aframes.corr_of(int(b)) for b in sample]
        matches = [w.sframes.matches_of(int(b)) for b in sample]
    w.close()
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    size = 0
    for name in names:
        a, b = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert a.dtype in (np.float32, np.float64), name
        assert np.array_equal(a, b, equal_nan=True), name  # same inputs, same step: the same outputs
        size += a.nbytes
    assert size == total <= bench.DUMP_BUDGET_BYTES
    d = {n[:-4]: np.load(tmp_path / "a" / n) for n in names}
    assert np.array_equal(d["pose"].reshape(w.B, 16), X)
    assert np.array_equal(d["n_correspondences"], n_corr.astype(np.float64))
    assert np.array_equal(d["align_iterations_executed"], [r.iterations_executed for r in res])
    assert np.array_equal(d["align_status"], [r.status for r in res])
    assert len(sample) == 256 and np.all(np.diff(sample) > 0)
    for k, (c, m) in enumerate(zip(corr, matches)):
        got = d["sample_correspondences"][k]
        assert np.array_equal(got[: len(c), 0], c["fixed_idx"]) and np.array_equal(got[: len(c), 1], c["moving_idx"])
        assert np.array_equal(got[: len(c), 2], c["response"]) and not got[len(c):].any()
        got = d["sample_stereo_matches"][k]
        assert np.array_equal(got[: len(m), 0], m["fixed_idx"]) and np.array_equal(got[: len(m), 2], m["response"])
        assert not got[len(m):].any()
