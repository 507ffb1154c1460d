"""render_cli --hue-cycle DEG [--hue-object K]: object K's baseColor hue turns each frame (Renderer.set_materials).
main() runs in this process on the session's library, as in test_gpu_moving_lights_cli.py."""
import dataclasses

import numpy as np
import pytest


@pytest.mark.gpu
def test_hue_cycle_flag(gpu, scene_small, tmp_path, monkeypatch):
    from ptsvgf import gl, render_cli
    from ptsvgf import scene as scene_mod

    # (set_materials keeps scene.tri_enc in step: each run gets a scene object of its own)
    monkeypatch.setattr(scene_mod, "build_scene",
                        lambda name: dataclasses.replace(scene_small, tri_enc=scene_small.tri_enc.copy()))
    monkeypatch.setattr(gl, "init", lambda device=0: None)
    monkeypatch.setattr(gl, "shutdown", lambda: None)
    base = ["--width", "160", "--height", "96", "--frames", "4", "--view", "path_tracing_pic_1spp"]
    before = scene_small.tri_enc.copy()
    out = {}
    for name, extra in (("plain", []), ("zero", ["--hue-cycle", "0"]), ("cycle", ["--hue-cycle", "40"]),
                        ("table", ["--hue-cycle", "40", "--hue-object", "0"])):
        png = tmp_path / f"{name}.png"
        assert render_cli.main(base + ["--png", str(png)] + extra) == 0
        out[name] = png.read_bytes()
        assert out[name][:8] == b"\x89PNG\r\n\x1a\n" and len(out[name]) > 1000
    assert out["zero"] == out["plain"]
    assert out["cycle"] != out["plain"]  # the clock's brass has turned 160 degrees
    assert out["table"] != out["plain"] and out["table"] != out["cycle"]
    assert np.array_equal(before, scene_small.tri_enc)  # the session's fixture stays as it is
    with pytest.raises(SystemExit):
        render_cli.main(base + ["--png", str(tmp_path / "none.png"), "--hue-cycle", "40", "--hue-object", "9"])


def test_hue_turn_keeps_the_rest_of_the_material():
    from ptsvgf.materials import hue_turned
    from ptsvgf.scene import material

    m = material(baseColor=(0.8, 0.2, 0.2), emissive=(1.0, 2.0, 3.0), roughness=0.35, metallic=0.6)
    assert np.allclose(hue_turned(m, 0.0), m, atol=1e-6) and np.allclose(hue_turned(m, 360.0), m, atol=1e-6)
    t = hue_turned(m, 120.0)
    assert np.allclose(t[3:6], (0.2, 0.8, 0.2), atol=1e-6)  # red a third of the way round is green
    keep = np.r_[0:3, 6:18]
    assert np.array_equal(t[keep], m[keep]) and t.dtype == np.float32
