#!/usr/bin/env python3
"""Cost of posing objects by matrix on the device against a refit from host arrays (DESIGN.md "Posed objects") on
the bench scene at 4K, K = 4, at rebuild_bvh's defaults, the two paths alternating in one process; one JSON line per
repetition and a summary with the median and the min-max range of each figure:

  device    pt_pose_apply's out_ms (both pose kernels, both refits, both derivations) against pt_bvh_refit's (the
            path tracer's refit and derivation alone)
  wall      "all trees + frame" with the plant moved a little further each step: pose_objects({2: M_step}) + frame +
            synchronise against refit_bvh(tri, raster=..., prev_raster=True) + the same, the host arrays of the
            latter prepared outside the timed region

A refit_bvh call releases the pose (mixing the two needs a rebuild_bvh in between), so every timed call starts from
an untimed rebuild_bvh (the posed path also from one untimed pose_objects call, which creates the pose) and a frame;
the order of the two timed paths alternates with the repetition.

    python tools/pose_cost.py [--reps 8] [--width 3840 --height 2160] [--k 4]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stat(v):
    return dict(median=round(float(np.median(v)), 4), min=round(float(np.min(v)), 4), max=round(float(np.max(v)), 4),
                n=len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--k", type=int, default=4)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(REPO, "path-tracing-svgf_amd"))
    import torch

    from ptsvgf import gl
    from ptsvgf.camera import parameter_config
    from ptsvgf.renderer import Renderer
    from ptsvgf.scene import build_scene, transform

    scene = build_scene("table_clock_plant")
    gl.init(0)
    r = Renderer(scene, a.width, a.height, parameter_config(), mode="fast", aspect_corrected=True, run_taa=False,
                 run_output=False, frames_in_flight=a.k)
    sel = scene.tri_enc[:, 42] == 2.0  # the plant, the last object emitted into the raster list
    n_plant = int(sel.sum())

    def lifted(dy):
        tri = scene.tri_enc.copy()
        tri[sel, 1:9:3] += np.float32(dy)
        v = scene.raster.reshape(-1, 3, 6).copy()
        v[len(v) - n_plant:, :, 1] += np.float32(dy)
        return tri, v.reshape(-1)

    def matrix(step):  # lifted and turned a little further each step
        return transform(rot=(0.0, 0.05 * step, 0.0), trans=(0.0, 0.002 * step, 0.0))

    def sync():
        torch.cuda.synchronize()

    def fresh(with_pose):
        r.rebuild_bvh(raster=scene.raster)
        if with_pose:
            r.pose_objects({2: matrix(0)})  # creates the pose: one upload of the rest lists, not timed
        r.frame()
        sync()

    out = dict(width=a.width, height=a.height, k=a.k, triangles=int(scene.ntris), plant_triangles=n_plant)
    fresh(False)
    for _ in range(a.warmup):
        r.frame()
    sync()

    dev = {"pose": [], "refit": []}
    wall = {"pose": [], "refit": []}
    step = 0
    for rep in range(a.reps + 1):  # the first pair warms both paths up and is dropped
        for name in (("pose", "refit") if rep % 2 == 0 else ("refit", "pose")):
            step += 1
            if name == "pose":
                fresh(True)
                m = {2: matrix(step)}
            else:
                fresh(False)
                tri, raster = lifted(0.002 * step)
            sync()
            t0 = time.perf_counter()
            if name == "pose":
                ms = r.pose_objects(m)
            else:
                ms = r.refit_bvh(tri, raster=raster, prev_raster=True)
            r.frame()
            sync()
            w = (time.perf_counter() - t0) * 1e3
            if rep:
                dev[name].append(ms)
                wall[name].append(w)
        if rep:
            print(json.dumps(dict(rep=rep - 1, device_ms={k: round(v[-1], 4) for k, v in dev.items()},
                                  wall_ms={k: round(v[-1], 3) for k, v in wall.items()})), flush=True)
    out["device_ms"] = {k: _stat(v) for k, v in dev.items()}
    out["all_trees_plus_frame_ms"] = {k: _stat(v) for k, v in wall.items()}

    # a frame alone, issued serially, for scale
    alone = []
    for _ in range(a.reps):
        sync()
        t0 = time.perf_counter()
        r.frame()
        sync()
        alone.append((time.perf_counter() - t0) * 1e3)
    out["frame_alone_ms"] = _stat(alone)
    print(json.dumps(dict(summary=out)))
    r.close()
    gl.shutdown()


if __name__ == "__main__":
    main()
