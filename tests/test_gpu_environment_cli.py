"""render_cli --sky-turn DEG: the environment map's columns are rolled from the original before each frame
(Renderer.set_environment). main() runs in this process on the session's library, as in test_gpu_moving_lights_cli.py;
its last frame equals a Renderer driven by the same rolls."""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, FRAMES, DEG = 160, 96, 4, 25.0
VIEW = "path_tracing_pic_1spp"


def test_sky_turn_flag(gpu, scene_small, tmp_path, monkeypatch):
    from ptsvgf import gl, render_cli
    from ptsvgf import scene as scene_mod
    from ptsvgf.camera import parameter_config
    from ptsvgf.renderer import Renderer

    # (set_environment keeps scene.hdr in step: each run gets a scene object of its own)
    own = lambda: dataclasses.replace(scene_small, hdr=scene_small.hdr.copy(), cache=scene_small.cache.copy())
    monkeypatch.setattr(scene_mod, "build_scene", lambda name: own())
    monkeypatch.setattr(gl, "init", lambda device=0: None)
    monkeypatch.setattr(gl, "shutdown", lambda: None)
    base = ["--width", str(W), "--height", str(H), "--frames", str(FRAMES), "--view", VIEW]
    out = {}
    for name, extra in (("plain", []), ("zero", ["--sky-turn", "0"]), ("turn", ["--sky-turn", str(DEG)])):
        png = tmp_path / f"{name}.png"
        assert render_cli.main(base + ["--png", str(png)] + extra) == 0
        out[name] = png.read_bytes()
        assert out[name][:8] == b"\x89PNG\r\n\x1a\n" and len(out[name]) > 1000
    assert out["zero"] == out["plain"]
    assert out["turn"] != out["plain"]
    # the same rolls through the Renderer
    r = Renderer(own(), W, H, parameter_config(), mode="fast", run_taa=True, run_output=True)
    r.set_view(VIEW)
    sky0 = scene_small.hdr
    shifts = [render_cli.sky_shift(f, DEG, sky0.shape[1]) for f in range(FRAMES)]
    assert shifts[0] == 0 and len(set(shifts)) == FRAMES
    for s in shifts:
        r.set_environment(np.roll(sky0, s, axis=1))
        r.frame()
    gl.sync()
    png = tmp_path / "renderer.png"
    render_cli.write_png(str(png), gl.readback(r.planes()["output"]))
    r.close()
    assert png.read_bytes() == out["turn"]
