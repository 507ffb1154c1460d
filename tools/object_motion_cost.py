#!/usr/bin/env python3
"""Cost of the G-buffer's object-motion path (DESIGN.md "Dynamic scenes"): the G-buffer pass time at 4K on the bench
scene with object_motion 1 (the frame right after a rebuild_bvh(prev_raster=...)) and 0 (the frame after it: the same
geometry through the kernels without the motion path), alternating in one process, with the plant alone moved and
with every triangle moved. pt_set_profiling / Renderer.pass_times; one JSON line per pair and a summary.

    python tools/object_motion_cost.py [--reps 8] [--width 3840 --height 2160] [--gbuffer-mode 1]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "path-tracing-svgf_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--gbuffer-mode", type=int, default=1)
    a = ap.parse_args()
    from ptsvgf import gl
    from ptsvgf.renderer import Renderer
    from ptsvgf.scene import build_scene

    scene = build_scene("table_clock_plant")
    gl.init(0)
    r = Renderer(scene, a.width, a.height, mode="fast")
    for p in r.init_pass:
        p.set_uniform_int("gbuffer_mode", a.gbuffer_mode)
    n_plant = int(np.sum(scene.tri_enc[:, 42] == 2.0))
    cur = scene.raster.reshape(-1, 3, 6)
    cases = {}
    prev = cur.copy()
    prev[len(cur) - n_plant:, :, 1] -= np.float32(0.05)  # the plant (the last object emitted) was lower
    cases["plant"] = prev.reshape(-1)
    prev = cur.copy()
    prev[:, :, :3] -= np.array([0.02, 0.03, -0.01], np.float32)
    cases["all"] = prev.reshape(-1)
    for _ in range(3):
        r.frame()
    out = {}
    for name, prev in cases.items():
        ms = {0: [], 1: []}
        for rep in range(a.reps):
            r.rebuild_bvh(raster=scene.raster, prev_raster=prev)
            for om in (1, 0):  # the frame after the rebuild draws with 1, the next with 0
                r.profile(True)
                r.frame()
                r.planes()
                t = r.pass_times()["gbuffer"]
                r.profile(False)
                ms[om].append(t)
            print(json.dumps(dict(moved=name, rep=rep, gbuffer_ms_om1=ms[1][-1], gbuffer_ms_om0=ms[0][-1])), flush=True)
        out[name] = {f"om{k}": dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))
                     for k, v in ms.items()}
    print(json.dumps(dict(summary=out, width=a.width, height=a.height, gbuffer_mode=a.gbuffer_mode,
                          triangles=int(len(cur)), plant_triangles=n_plant)))
    r.close()
    gl.shutdown()


if __name__ == "__main__":
    main()
