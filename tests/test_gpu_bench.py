"""bench.py's plain run and --dump-outputs (needs the GPU): the line carries the headline only, and the dumped frame is the one the
timed path drew -- the oracle's within RGBA_TOL, the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import DEFAULT_CAMERA, ROOT

RGBA_TOL = 1   # LSB per channel, as tests/test_gpu_parity.py


def run_bench(out, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args, "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1]), np.load(os.path.join(out, "rgba.npy"))


@pytest.mark.gpu
def test_plain_run_dumps_the_last_timed_frame(tmp_path, oracle, luts):
    W, G = 640, 256
    args = ("--steps", "5", "--warmup", "2", "--size", str(W), "--grid", str(G))
    d, a = run_bench(tmp_path / "a", *args)
    _, b = run_bench(tmp_path / "b", *args)
    assert d["steps"] == 5 and d["ms_per_step"] > 0 and d["value"] > 0 and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["cpu_baseline"] is None and d["other_camera"] is None and d["roofline_fragment"] is None and "api_latency_ms" not in d
    assert a.dtype == np.float32 and a.shape == (W, W, 4)
    assert np.array_equal(a, b), "the same arguments gave two different frames"
    h = np.random.default_rng(20250816).random((G, G), dtype=np.float32) * np.float32(0.5) - np.float32(0.25)   # bench.py's C4 heights
    u = oracle.look_at_uniforms(1, W, W, *DEFAULT_CAMERA)
    ref, _ = oracle.render_terrain(u, W, W, G, h, luts["viridis"], want_vis=False, nthreads=8)
    assert np.abs(a - ref.astype(np.float32)).max() <= RGBA_TOL


@pytest.mark.gpu
def test_c4_dump_is_a_fixed_sample(tmp_path):
    d, a = run_bench(tmp_path, "--steps", "3", "--warmup", "1")
    assert d["steps"] == 3 and (d["config"]["width"], d["config"]["grid"]) == (4096, 4096)
    assert a.dtype == np.float32 and a.shape == (3 << 20, 4) and a.nbytes <= 64 << 20
    assert a.min() >= 0 and a.max() <= 255 and len(np.unique(a, axis=0)) > 100
