"""python -m ptsvgf.render_cli --spp N: the flag reaches the path tracer. The CLI's main() runs in this process on
the session's library (its own init / shutdown are left to the `gpu` fixture) and on the session's small Cornell
scene instead of a scene built per call."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _pfm(path):
    data = open(path, "rb").read()
    head, size, scale, body = data.split(b"\n", 3)
    w, h = (int(v) for v in size.split())
    assert head == b"PF" and float(scale) < 0
    return np.frombuffer(body, "<f4").reshape(h, w, 3)


def test_spp_flag_changes_the_image(gpu, scene_cornell, tmp_path, monkeypatch):
    from ptsvgf import gl, render_cli
    from ptsvgf import scene as scene_mod

    monkeypatch.setattr(scene_mod, "build_scene", lambda name: scene_cornell)

    monkeypatch.setattr(gl, "init", lambda device=0: None)
    monkeypatch.setattr(gl, "shutdown", lambda: None)
    out = {}
    for n in (1, 2):
        png, pfm = str(tmp_path / f"spp{n}.png"), str(tmp_path / f"spp{n}.pfm")
        args = ["--width", "64", "--height", "48", "--frames", "2", "--scene", "cornell_teapot", "--view",
                "path_tracing_pic_1spp", "--png", png, "--pfm", pfm]
        assert render_cli.main(args + (["--spp", str(n)] if n > 1 else [])) == 0
        assert os.path.getsize(png) > 0
        out[n] = (open(png, "rb").read(), _pfm(pfm))
    assert out[1][1].shape == out[2][1].shape == (48, 64, 3)
    assert np.isfinite(out[2][1]).all() and out[2][1].any()
    assert not np.array_equal(out[1][1], out[2][1])
    assert out[1][0] != out[2][0]  # the written image differs too
    with pytest.raises(ValueError):
        render_cli.main(["--width", "64", "--height", "48", "--frames", "1", "--scene", "cornell_teapot", "--spp", "9"])
