"""bench.py --dump-outputs / --full contract, rehearsed on CPU: the
result line keeps its fields, --steps sets the number of timed steps,
the dump holds float32/float64 arrays of at most 64 MB, and two runs
with the same arguments see the same inputs and write the same arrays."""

import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _start(dump_dir, extra=()):
    env = dict(os.environ)
    env["CUDA_VISIBLE_DEVICES"] = ""
    env["HIP_VISIBLE_DEVICES"] = ""
    # the two runs share the machine; a few threads each keeps them quick
    env["OMP_NUM_THREADS"] = "2"
    cmd = [sys.executable, os.path.join(REPO, "bench.py"),
           "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--dump-outputs", dump_dir] + list(extra)
    return subprocess.Popen(cmd, cwd=REPO, env=env, text=True,
                            stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def _finish(proc):
    stdout, stderr = proc.communicate(timeout=300)
    assert proc.returncode == 0, stdout[-1500:] + stderr[-1500:]
    line = [ln for ln in stdout.splitlines() if ln.startswith("{")][-1]
    return json.loads(line)


def test_dump_outputs_repeatable_and_bounded(tmp_path):
    dirs = [str(tmp_path / "a"), str(tmp_path / "b")]
    procs = [_start(dirs[0]), _start(dirs[1], ["--full"])]
    recs = [_finish(p) for p in procs]
    for rec in recs:
        assert rec["metric"] == "images/sec" and rec["unit"] == "images/s"
        assert rec["higher_is_better"] is True and rec["dtype"] == "bf16"
        assert rec["steps"] == 2 and rec["warmup"] == 1
        assert rec["value"] > 0 and rec["ms_per_step"] > 0
        # value and ms_per_step describe the same timed window
        batch = rec["config"]["global_batch"]
        assert abs(rec["value"] * rec["ms_per_step"] / 1000.0 / batch - 1) \
            < 1e-2

    names = sorted(os.listdir(dirs[0]))
    assert names == sorted(os.listdir(dirs[1]))
    assert set(names) == {"loss.npy", "params.npy"}
    total = 0
    for name in names:
        a = np.load(os.path.join(dirs[0], name))
        b = np.load(os.path.join(dirs[1], name))
        assert a.dtype in (np.float32, np.float64)
        assert a.size > 0 and np.isfinite(a).all()
        total += a.nbytes
        np.testing.assert_array_equal(a, b)
    assert total <= 64 * 1024 * 1024


def _import_bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "sparkdl_bench", os.path.join(REPO, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_steps_sets_number_of_timed_steps(monkeypatch, capsys, tmp_path):
    """--steps N --warmup W calls the step W + N times, plus once more
    for the dumped step, and ms_per_step is the timed window over N."""
    import argparse
    import time
    import torch
    bench = _import_bench()
    calls = []

    def fake_builder(args, device, use_cuda):
        def step():
            calls.append(time.perf_counter())
            time.sleep(0.01)
            return torch.tensor(1.0)
        helper = argparse.Namespace(
            snapshot=lambda: calls.append("snapshot"),
            restore=lambda: calls.append("restore"),
            outputs=lambda: {"out": np.ones(3, dtype=np.float64)})
        return step, 8, {"model": "fake"}, helper

    monkeypatch.setattr(bench, "build_resnet_step", fake_builder)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for var in ("WORLD_SIZE", "RANK"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setattr(sys, "argv", [
        "bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2",
        "--dump-outputs", str(tmp_path / "d")])
    bench.main()
    assert calls[0] == "snapshot" and calls[-2] == "restore"
    assert len([c for c in calls if isinstance(c, float)]) == 2 + 5 + 1
    rec = json.loads([ln for ln in capsys.readouterr().out.splitlines()
                      if ln.startswith("{")][-1])
    assert rec["steps"] == 5
    # five sleeps of 10 ms: well above one step, well below eight
    assert 10.0 <= rec["ms_per_step"] < 16.0
    assert sorted(os.listdir(tmp_path / "d")) == ["loss.npy", "out.npy"]
    assert np.load(tmp_path / "d" / "out.npy").dtype == np.float64

    # a plain run takes no snapshot and no extra step
    del calls[:]
    monkeypatch.setattr(sys, "argv", [
        "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    bench.main()
    assert len(calls) == 4 and all(isinstance(c, float) for c in calls)


def test_miopen_tuning_is_loaded_from_a_scratch_copy(monkeypatch):
    import hashlib
    import shutil
    import torch
    bench = _import_bench()
    db = os.path.join(REPO, "miopen_gfx950")

    def digest():
        return {f: hashlib.sha256(open(os.path.join(db, f), "rb").read())
                .hexdigest() for f in sorted(os.listdir(db))}

    before = digest()
    assert before, "committed MIOpen tuning files are missing"
    monkeypatch.delenv("MIOPEN_USER_DB_PATH", raising=False)
    # the MIOpen build the committed files were captured with
    monkeypatch.setattr(torch.backends.cudnn, "version", lambda: 3005000)
    tmp = bench._load_miopen_tuning(512)
    try:
        assert tmp and os.path.realpath(tmp) != os.path.realpath(db)
        assert os.environ["MIOPEN_USER_DB_PATH"] == tmp
        assert sorted(os.listdir(tmp)) == sorted(before)
        with open(os.path.join(tmp, sorted(before)[0]), "a") as f:
            f.write("scribble\n")   # MIOpen may rewrite its copy
        assert digest() == before
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
        os.environ.pop("MIOPEN_USER_DB_PATH", None)

    # another MIOpen build: nothing is loaded
    monkeypatch.delenv("MIOPEN_USER_DB_PATH", raising=False)
    monkeypatch.setattr(torch.backends.cudnn, "version", lambda: 9009009)
    assert bench._load_miopen_tuning(512) is None
    assert "MIOPEN_USER_DB_PATH" not in os.environ

    # an explicit MIOPEN_USER_DB_PATH wins
    monkeypatch.setenv("MIOPEN_USER_DB_PATH", "/nonexistent")
    monkeypatch.setattr(torch.backends.cudnn, "version", lambda: 3005000)
    assert bench._load_miopen_tuning(512) is None
    assert os.environ["MIOPEN_USER_DB_PATH"] == "/nonexistent"
