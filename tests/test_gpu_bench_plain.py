"""bench.py's plain run: the headline figure only (--steps timed frames, `ms_per_step`), and --dump-outputs writes the
last timed frame's planes identically from run to run. What --full adds is covered by test_gpu_bench_bands.py."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_is_lean_and_dumps_repeat():
    """Two plain runs side by side at 320 x 256 (3 timed frames, 4 frames in flight): the line carries the headline
    fields and none of the --full measurements; each dump holds the four planes whole (81920 pixels x RGBA float32,
    far below the sampling threshold), finite, and bit-identical between the runs."""
    with tempfile.TemporaryDirectory() as d:
        procs = []
        for tag in "ab":
            cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                   "--width", "320", "--height", "256", "--dump-outputs", os.path.join(d, tag)]
            procs.append(subprocess.Popen(cmd, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
        lines = []
        for p in procs:
            out, err = p.communicate(timeout=300)
            assert p.returncode == 0, err[-4000:]
            assert len(out.strip().splitlines()) == 1, out  # one JSON line on stdout
            lines.append(json.loads(out))
        for line in lines:
            assert line["steps"] == 3 and line["full"] is False and line["n_gpus"] == 1
            assert line["unit"] == "frames/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
            assert line["ms_per_step"] > 0 and abs(line["value"] * line["ms_per_step"] / 1e3 - 1.0) < 1e-2
            assert not {"roofline", "cpu_baseline", "path_tracer", "passes_ms", "fps_serial", "fps_1080p", "surface_view",
                        "moving", "dynamic_bvh", "config0", "latency"} & set(line)
        names = sorted(os.listdir(os.path.join(d, "a")))
        assert names == ["albedo.npy", "atrous.npy", "color.npy", "modulate.npy"] == sorted(os.listdir(os.path.join(d, "b")))
        total = 0
        for n in names:
            a, b = np.load(os.path.join(d, "a", n)), np.load(os.path.join(d, "b", n))
            total += a.nbytes
            assert a.dtype == np.float32 and a.shape == (320 * 256, 4) == b.shape
            assert np.isfinite(a).all() and np.array_equal(a.view(np.uint32), b.view(np.uint32)), n
        assert np.load(os.path.join(d, "a", "modulate.npy"))[:, :3].max() > 0  # a rendered frame, not an empty plane
        assert total <= 64 << 20
