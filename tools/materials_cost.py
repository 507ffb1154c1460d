"""Measurements of DESIGN.md "Material edits" on the bench scene: what a material edit costs.

    python tools/materials_cost.py fps    [--pkg DIR] [--variants none,update,rebuffer] [--reps 3]
    python tools/materials_cost.py update [--calls 200]

fps     ms per frame at 3840 x 2160 with 4 frames in flight and a standing camera, the variants alternating in one
        process, --reps times:
          none      no edits;
          update    Renderer.set_materials recolours object 1 (the clock) every frame;
          rebuffer  the route before pt_materials_update: a new triangle texture buffer with the edited rows per
                    frame, bound in place of the old one, which is destroyed.
update  the update alone on a small standing renderer: the host time of a call and, with nothing else queued, the
        time from issuing --calls updates to the device having run them, per call. Run it under
        `rocprofv3 --kernel-trace --stats -- python tools/materials_cost.py update` for the materials_* kernels' times.

--pkg DIR runs another checkout's package (its path-tracing-svgf_amd directory), e.g. the parent commit's, for
same-box comparisons; `update` and the update variant are refused there.
One JSON line per result on stdout.
"""
from __future__ import annotations

import argparse
import dataclasses
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = 1


def _material(step):
    from ptsvgf.scene import material

    a = 0.1 * step
    return material(baseColor=(0.5 + 0.4 * np.cos(a), 0.5 + 0.4 * np.sin(a), 0.35), metallic=0.6, specular=0.0,
                    roughness=0.35, clearcoat=0.0, clearcoatGloss=0.0)


def _edited(tri, m):
    out = np.array(tri, np.float32, copy=True)
    out[out[:, 42] == np.float32(OBJ), 18:36] = m
    return out


def _renderer(scene, W, H, K):
    from ptsvgf.camera import parameter_config
    from ptsvgf.renderer import Renderer

    return Renderer(scene, W, H, parameter_config(), mode="fast", aspect_corrected=True, run_taa=False,
                    run_output=False, frames_in_flight=K, host_pace=True)


def run_fps(gl, scene, variant, W, H, K, steps, warmup):
    sc = dataclasses.replace(scene, tri_enc=scene.tri_enc.copy())
    r = _renderer(sc, W, H, K)
    if variant == "update" and not hasattr(r, "set_materials"):
        raise SystemExit("variant update needs Renderer.set_materials")
    spans = []
    for f in range(warmup + steps):
        if f == warmup:
            gl.sync()
            t0 = time.perf_counter()
        t = time.perf_counter()
        old = None
        if variant == "update":
            r.set_materials({OBJ: _material(f + 1)})
        elif variant == "rebuffer":
            old = r.trianglesTextureBuffer
            r.trianglesTextureBuffer = gl.texture_buffer(_edited(scene.tri_enc, _material(f + 1)))
            r._owned.append(r.trianglesTextureBuffer)
            r._owned.remove(old)
        r.frame()
        if old is not None:
            gl.destroy_texture(old)
        if f >= warmup:
            spans.append(time.perf_counter() - t)
    r.flush()
    gl.sync()
    dt = time.perf_counter() - t0
    r.close()
    return {"variant": variant, "ms_per_frame": round(1e3 * dt / steps, 4), "fps": round(steps / dt, 2),
            "longest_frame_ms": round(1e3 * max(spans), 3), "median_issue_ms": round(1e3 * float(np.median(spans)), 3),
            "steps": steps, "K": K, "size": [W, H]}


def run_update(gl, scene, calls):
    sc = dataclasses.replace(scene, tri_enc=scene.tri_enc.copy())
    r = _renderer(sc, 160, 96, 4)
    for _ in range(4):
        r.frame()
    r.flush()
    gl.sync()
    mats = [_material(i)[None] for i in range(calls + 8)]
    tt = r.trianglesTextureBuffer
    for i in range(8):  # the first updates allocate
        gl.materials_update(tt, OBJ, mats[i])
    gl.sync()
    host = []
    t0 = time.perf_counter()
    for i in range(calls):
        t = time.perf_counter()
        gl.materials_update(tt, OBJ, mats[8 + i])
        host.append(time.perf_counter() - t)
    gl.sync()
    dt = time.perf_counter() - t0
    state = gl.materials_state(tt, r.nodesTextureBuffer)
    r.close()
    return {"triangles": int(scene.tri_enc.shape[0]), "calls": calls,
            "host_us_per_call_median": round(1e6 * float(np.median(host)), 2),
            "issue_to_done_us_per_call": round(1e6 * dt / calls, 2), **state}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("mode", choices=("fps", "update"))
    ap.add_argument("--pkg", default=os.path.join(REPO, "path-tracing-svgf_amd"))
    ap.add_argument("--variants", default="none,update,rebuffer")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rebuffer-steps", type=int, default=24, help="steps of the rebuffer variant (each rebuilds all)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--frames-in-flight", type=int, default=4)
    ap.add_argument("--calls", type=int, default=200)
    a = ap.parse_args(argv)
    sys.path.insert(0, a.pkg)
    from ptsvgf import gl
    from ptsvgf.scene import build_scene

    scene = build_scene("table_clock_plant")
    gl.init(0)
    try:
        if a.mode == "update":
            if not hasattr(gl, "materials_update"):
                raise SystemExit("update needs pt_materials_update")
            print(json.dumps({"mode": "update", **run_update(gl, scene, a.calls)}), flush=True)
        else:
            for rep in range(a.reps):
                for v in a.variants.split(","):
                    slow = v == "rebuffer"
                    res = run_fps(gl, scene, v, a.width, a.height, a.frames_in_flight,
                                  a.rebuffer_steps if slow else a.steps, 4 if slow else a.warmup)
                    print(json.dumps({"mode": "fps", "pkg": a.pkg, "rep": rep, **res}), flush=True)
    finally:
        gl.shutdown()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
