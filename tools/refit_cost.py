#!/usr/bin/env python3
"""Cost of a BVH refit against a rebuild (DESIGN.md "Dynamic scenes", Refit) on the bench scene at 4K, K = 4, at
rebuild_bvh's defaults, the variants alternating in one process; one JSON line per repetition and a summary with the
median and the min-max range of each figure:

  device    pt_bvh_refit's out_ms against pt_bvh_build's (both with the walk trees' derivation)
  wall      "all trees + frame" with the plant lifted a little further each step: refit_bvh(tri, raster=...,
            prev_raster=True) + frame + synchronise against rebuild_bvh(tri, raster=..., prev_raster=True) + the same
  decay     frames/s over a tree refitted after the plant has moved by 1 %, 5 % and 20 % of the scene's extent, against
            a fresh rebuild at the same positions

    python tools/refit_cost.py [--reps 8] [--steps 60 --warmup 10] [--width 3840 --height 2160] [--k 4]
    python tools/refit_cost.py --rebuild-only --pkg OTHER_TREE/path-tracing-svgf_amd    # the rebuild path of another
                                                                                        # checkout (no refit there)
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
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--rebuild-only", action="store_true")
    ap.add_argument("--pkg", default=os.path.join(REPO, "path-tracing-svgf_amd"))
    a = ap.parse_args()
    sys.path.insert(0, a.pkg)
    import torch

    from ptsvgf import gl
    from ptsvgf.camera import parameter_config
    from ptsvgf.renderer import Renderer
    from ptsvgf.scene import build_scene

    scene = build_scene("table_clock_plant")
    gl.init(0)
    r = Renderer(scene, a.width, a.height, parameter_config(), mode="fast", aspect_corrected=True, run_taa=False,
                 run_output=False, frames_in_flight=a.k)
    sel = scene.tri_enc[:, 42] == 2.0  # the plant, the last object emitted into the raster list
    n_plant = int(sel.sum())
    pos = scene.tri_enc[:, :9].reshape(-1, 3)
    extent = float(np.max(pos.max(0) - pos.min(0)))

    def lifted(dy):
        tri = scene.tri_enc.copy()
        tri[sel, 1:9:3] += np.float32(dy)
        v = scene.raster.reshape(-1, 3, 6).copy()
        v[len(v) - n_plant:, :, 1] += np.float32(dy)
        return tri, v.reshape(-1)

    def sync():
        torch.cuda.synchronize()

    out = dict(width=a.width, height=a.height, k=a.k, triangles=int(scene.ntris), plant_triangles=n_plant,
               extent=round(extent, 4), rebuild_only=a.rebuild_only)
    r.rebuild_bvh(raster=scene.raster)
    for _ in range(a.warmup):
        r.frame()
    sync()

    # 1. device time
    dev = {"rebuild": [], "refit": []}
    for rep in range(a.reps):
        tri, _ = lifted(0.001 * (rep + 1))
        dev["rebuild"].append(r.rebuild_bvh(tri_enc=tri)[1])
        if not a.rebuild_only:
            dev["refit"].append(r.refit_bvh(tri))
        print(json.dumps(dict(part="device", rep=rep, **{k: round(v[-1], 4) for k, v in dev.items() if v})), flush=True)
    out["device_ms"] = {k: _stat(v) for k, v in dev.items() if v}

    # 2. wall time per moved frame: all trees + frame
    wall = {"rebuild": [], "refit": []}
    step = 0
    for rep in range(a.reps + 1):  # the first pair warms both paths up and is dropped
        for name in ("rebuild", "refit"):
            if name == "refit" and a.rebuild_only:
                continue
            step += 1
            tri, raster = lifted(0.002 * step)
            sync()
            t0 = time.perf_counter()
            if name == "rebuild":
                r.rebuild_bvh(tri_enc=tri, raster=raster, prev_raster=True)
            else:
                r.refit_bvh(tri, raster=raster, prev_raster=True)
            r.frame()
            sync()
            ms = (time.perf_counter() - t0) * 1e3
            if rep:
                wall[name].append(ms)
        if rep:
            print(json.dumps(dict(part="wall", rep=rep - 1, **{k: round(v[-1], 3) for k, v in wall.items() if v})),
                  flush=True)
    out["all_trees_plus_frame_ms"] = {k: _stat(v) for k, v in wall.items() if v}

    # 3. tree decay: frames/s over a refitted against a rebuilt tree at the same positions
    def fps():
        for _ in range(a.warmup):
            r.frame()
        sync()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            r.frame()
        sync()
        return a.steps / (time.perf_counter() - t0)

    if not a.rebuild_only:
        decay = {}
        for frac in (0.01, 0.05, 0.20):
            tri, raster = lifted(frac * extent)
            f = {"refit": [], "rebuild": []}
            for rep in range(2):
                r.rebuild_bvh(raster=scene.raster)  # the tree of the positions before the move
                r.refit_bvh(tri, raster=raster)
                f["refit"].append(fps())
                r.rebuild_bvh(tri_enc=tri, raster=raster)
                f["rebuild"].append(fps())
                print(json.dumps(dict(part="decay", moved=frac, rep=rep, refit_fps=round(f["refit"][-1], 2),
                                      rebuild_fps=round(f["rebuild"][-1], 2))), flush=True)
            decay[str(frac)] = {k: _stat(v) for k, v in f.items()}
        out["decay_fps"] = decay
    print(json.dumps(dict(summary=out)))
    r.close()
    gl.shutdown()


if __name__ == "__main__":
    main()
