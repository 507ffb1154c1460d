"""Measurements of DESIGN.md "Moving point lights" on the bench scene: what a moved light costs per frame.

    python tools/moving_lights_bench.py fps   [--pkg DIR] [--variants static,walk1,update,newbuf] [--reps 3]
    python tools/moving_lights_bench.py build [--pkg DIR] [--one-light]

fps    frames per second and the longest frame at 3840 x 2160 with 4 frames in flight and a standing camera, the
       variants alternating in one process, --reps times:
         static  the lights never change (all four binned);
         walk1   light 1 moved once and left "moved, bins pending" (light_settle never reached): the gain of one
                 light's bins per frame is static against this;
         update  Renderer.set_lights moves light 1 every frame;
         newbuf  the route before pt_lights_update: a new lights texture buffer per frame, the old one destroyed.
build  one first frame (the bins' full build at R = 128) and, with --one-light, a move of light 1 with
       light_settle = 0 and one more frame (that light's rebuild); prints the frames' wall times. Run it under
       `rocprofv3 --kernel-trace --stats -- python tools/moving_lights_bench.py build ...` for the pb_* kernels' times.

--pkg DIR runs another checkout's package (its path-tracing-svgf_amd directory), e.g. the parent commit's, for
same-box comparisons; variants that need set_lights are refused there.
One JSON line per result on stdout.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _moved(lights, step):
    """Light 1 on a small circle about its first position (clear of the bench scene's geometry)."""
    rec = np.array(lights[1:2], np.float32, copy=True)
    a = 0.1 * step
    rec[0, 0] += np.float32(0.15 * np.cos(a) - 0.15)
    rec[0, 2] += np.float32(0.15 * np.sin(a))
    return rec


def _renderer(scene, W, H, K, **kw):
    from ptsvgf.camera import parameter_config
    from ptsvgf.renderer import Renderer

    return Renderer(scene, W, H, parameter_config(), mode="fast", aspect_corrected=True, run_taa=False,
                    run_output=False, frames_in_flight=K, host_pace=True, **kw)


def run_fps(gl, scene, variant, W, H, K, steps, warmup, has_update):
    import dataclasses

    sc = dataclasses.replace(scene, lights=scene.lights.copy())
    kw = {}
    if variant in ("walk1", "update"):
        if not has_update:
            raise SystemExit(f"variant {variant} needs Renderer.set_lights")
        kw["light_settle"] = 1 << 30
    r = _renderer(sc, W, H, K, **kw)
    base = scene.lights.copy()
    spans = []
    for f in range(warmup + steps):
        if f == warmup:
            gl.sync()
            t0 = time.perf_counter()
        t = time.perf_counter()
        if variant == "update" or (variant == "walk1" and f == 1):
            r.set_lights(_moved(base, f + 1), first=1)
        elif variant == "newbuf":
            lights = base.copy()
            lights[1:2] = _moved(base, f + 1)
            old = r.pointLightBuffer
            r.pointLightBuffer = gl.texture_buffer(lights)
            r._owned.append(r.pointLightBuffer)
            r._owned.remove(old)
        r.frame()
        if variant == "newbuf":
            gl.destroy_texture(old)
        if f >= warmup:
            spans.append(time.perf_counter() - t)
    r.flush()
    gl.sync()
    dt = time.perf_counter() - t0
    r.close()
    return {"variant": variant, "fps": round(steps / dt, 2), "longest_frame_ms": round(1e3 * max(spans), 3),
            "median_frame_ms": round(1e3 * float(np.median(spans)), 3), "steps": steps, "K": K, "size": [W, H]}


def run_build(gl, scene, one_light, has_update):
    import dataclasses

    sc = dataclasses.replace(scene, lights=scene.lights.copy())
    kw = {"light_settle": 0} if has_update else {}
    r = _renderer(sc, 160, 96, 4, **kw)
    out = {}

    def frame(tag):
        gl.sync()
        t = time.perf_counter()
        r.frame()
        r.flush()
        gl.sync()
        out[tag] = round(1e3 * (time.perf_counter() - t), 3)

    frame("first_frame_ms")
    frame("second_frame_ms")
    if one_light:
        if not has_update:
            raise SystemExit("--one-light needs Renderer.set_lights")
        r.set_lights(_moved(scene.lights, 5), first=1)
        frame("rebuild_frame_ms")
        frame("frame_after_ms")
    info = gl.point_bins_info(r.trianglesTextureBuffer, r.nodesTextureBuffer)
    out["R"] = info["R"]
    out["entries"] = [q["entries"] for q in info["per_light"]]
    out["large"] = [q.get("large") for q in info["per_light"]]
    r.close()
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("mode", choices=("fps", "build"))
    ap.add_argument("--pkg", default=os.path.join(REPO, "path-tracing-svgf_amd"))
    ap.add_argument("--variants", default="static,walk1,update,newbuf")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--frames-in-flight", type=int, default=4)
    ap.add_argument("--one-light", action="store_true")
    a = ap.parse_args(argv)
    sys.path.insert(0, a.pkg)
    from ptsvgf import gl
    from ptsvgf.renderer import Renderer
    from ptsvgf.scene import build_scene

    has_update = hasattr(Renderer, "set_lights")
    scene = build_scene("table_clock_plant")
    gl.init(0)
    try:
        if a.mode == "build":
            print(json.dumps({"mode": "build", "pkg": a.pkg, **run_build(gl, scene, a.one_light, has_update)}), flush=True)
        else:
            for rep in range(a.reps):
                for v in a.variants.split(","):
                    res = run_fps(gl, scene, v, a.width, a.height, a.frames_in_flight, a.steps, a.warmup, has_update)
                    print(json.dumps({"mode": "fps", "pkg": a.pkg, "rep": rep, **res}), flush=True)
    finally:
        gl.shutdown()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
