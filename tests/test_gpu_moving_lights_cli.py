"""render_cli --light-orbit DEG: light 0 turns about the scene's vertical axis each frame (Renderer.set_lights).
main() runs in this process on the session's library, as in test_render_cli_spp.py."""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_light_orbit_flag(gpu, scene_small, tmp_path, monkeypatch):
    from ptsvgf import gl, render_cli
    from ptsvgf import scene as scene_mod

    # (set_lights keeps scene.lights in step: each run gets a scene object of its own)
    monkeypatch.setattr(scene_mod, "build_scene",
                        lambda name: dataclasses.replace(scene_small, lights=scene_small.lights.copy()))
    monkeypatch.setattr(gl, "init", lambda device=0: None)
    monkeypatch.setattr(gl, "shutdown", lambda: None)
    base = ["--width", "160", "--height", "96", "--frames", "4", "--view", "path_tracing_pic_1spp"]
    out = {}
    for name, extra in (("plain", []), ("zero", ["--light-orbit", "0"]), ("orbit", ["--light-orbit", "5"])):
        png = tmp_path / f"{name}.png"
        assert render_cli.main(base + ["--png", str(png)] + extra) == 0
        out[name] = png.read_bytes()
        assert out[name][:8] == b"\x89PNG\r\n\x1a\n" and len(out[name]) > 1000
    assert out["zero"] == out["plain"]
    assert out["orbit"] != out["plain"]  # the light moved 20 degrees: its shadows did too


def test_light_orbit_turns_about_the_vertical_axis(scene_small):
    from ptsvgf.render_cli import _light_orbit_setup

    at = _light_orbit_setup(scene_small)
    rec0 = scene_small.lights[0]
    assert np.array_equal(at(0.0), rec0)
    assert np.allclose(at(360.0), rec0, atol=1e-5)
    a = at(90.0)
    assert a[1] == rec0[1] and np.array_equal(a[3:], rec0[3:])  # height and colour stay
    half = at(180.0)
    axis = (half[[0, 2]] + rec0[[0, 2]]) / 2  # the axis lies midway between a point and its half turn
    for deg in (5.0, 90.0, 270.0):
        p = at(deg)
        assert np.isclose(np.hypot(*(p[[0, 2]] - axis)), np.hypot(*(rec0[[0, 2]] - axis)), atol=1e-5)
