"""bench.py's plain run on the GPU: the headline alone, --steps timed steps, and
--dump-outputs writing what the last timed step computed (checked against the
oracle), identically from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

H, W, F = 72, 104, 3
ARGS = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--settle-max-s", "0", "--frames", str(F),
        "--height", str(H), "--width", str(W)]


def _bench(*extra):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *ARGS, *extra],
                       env=env, capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_is_the_headline_and_dumps_the_last_step(tmp_path):
    from bench import synth_frame
    from oracle import oracle as O
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    line = _bench("--dump-outputs", d1)
    assert line["full"] is False and line["steps"] == 3 and line["warmup"] == 1
    assert line["metric"] == "Mpixels/s encode (DCT+deadzone) at 4K" and line["unit"] == "Mpixels/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["ms_per_step"] > 0 and line["value"] > 0
    # value and ms_per_step are the same measurement (F frames per step), up to
    # the line's rounding: ms_per_step to 4 decimals, value to 1
    tol = 0.5e-4 / line["ms_per_step"] + 0.05 / line["value"] + 1e-6
    assert abs(F * H * W / (line["ms_per_step"] * 1e-3) / 1e6 / line["value"] - 1) <= 1.01 * tol / (1 - tol)
    for key in ("cpu_baseline", "parity", "c4_e2e_with_gather", "c4_tiff_e2e_with_gather", "c5_e2e_with_gather",
                "c3_dwt", "c2_encode_decode_fn"):
        assert key not in line, key
    assert os.listdir(d1) == ["dct_dz_indices.npy"]
    got = np.load(os.path.join(d1, "dct_dz_indices.npy"))
    assert got.dtype == np.float32 and got.shape == (F, H * W * 3) and line["dumped_outputs"]["shape"] == [F, H * W * 3]
    for f in range(F):
        want = O.encode_frame(synth_frame(H, W, seed=f), 32)
        assert np.array_equal(got[f], want.reshape(-1).astype(np.float32)), f"frame {f}"
    _bench("--dump-outputs", d2)
    assert np.array_equal(np.load(os.path.join(d2, "dct_dz_indices.npy")), got)
