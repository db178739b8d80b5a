"""GPU: bench.py's plain run -- the headline only (no CPU baseline, no extras, no detail file), `--steps` timed steps,
and `--dump-outputs` writing the last timed step's top-k, identical from run to run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, timeout=600):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True,
                          text=True, timeout=timeout)
    assert proc.returncode == 0, "\n".join((proc.stdout + proc.stderr).splitlines()[-20:])
    lines = [x for x in proc.stdout.splitlines() if x.strip()]
    assert len(lines) == 1, proc.stdout[-2000:]   # ONE JSON line on stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_times_the_headline_and_dumps_the_last_steps_topk(tmp_path):
    rows, steps, k = 3_000_000, 4, 100
    args = ["--gpus", "1", "--steps", str(steps), "--warmup", "2", "--rows", str(rows), "--k", str(k)]
    a = _bench(args + ["--dump-outputs", str(tmp_path / "a")])
    b = _bench(args + ["--dump-outputs", str(tmp_path / "b")])
    for d in (a, b):
        assert d["steps"] == steps and d["warmup"] == 2 and d["higher_is_better"] is True and d["dtype"] == "f32"
        assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(rows / (d["ms_per_step"] * 1e-3), rel=1e-4)
        assert d["roofline"]["launches"] == steps                  # the scans of the timed steps, no more
        assert d["cpu_baseline"] is None and d["extras"] == {} and d["detail"] is None
    imgs, scores = np.load(tmp_path / "a" / "topk_images.npy"), np.load(tmp_path / "a" / "topk_scores.npy")
    assert imgs.dtype == np.float64 and scores.dtype == np.float32 and imgs.shape == scores.shape == (k,)
    assert np.array_equal(imgs, np.round(imgs)) and len(np.unique(imgs)) == k and (imgs >= 0).all()
    assert (np.diff(scores) <= 0).all()                            # ranked, best first
    assert a["top1"] == {"image": int(imgs[0]), "score": float(scores[0])}
    for name in ("topk_images.npy", "topk_scores.npy"):            # same arguments -> same inputs -> same outputs
        assert (tmp_path / "a" / name).read_bytes() == (tmp_path / "b" / name).read_bytes(), name
