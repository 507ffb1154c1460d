"""Measurements of DESIGN.md "Environment edits" on the bench scene: what a new environment map costs.

    python tools/environment_cost.py fps    [--variants none,host,device,upload] [--reps 3]
    python tools/environment_cost.py update [--calls 40]

fps     ms per frame at 3840 x 2160 with 4 frames in flight and a standing camera, the variants alternating in one
        process, --reps times:
          none    no edits;
          host    Renderer.set_environment every frame with the 2048 x 1024 map rolled, a numpy array;
          device  the same with the rolled map a device tensor;
          upload  the route before pt_environment_update: hdr_cache on the host, Renderer.flush(), the device idle,
                  two pt_texture2d_upload calls.
update  the update alone on a small standing renderer with the bench map: the host time of a call (host and device
        source) and, with nothing else queued, the time from issuing an update to the device having run it. Run
        it under `rocprofv3 --kernel-trace --stats -- python tools/environment_cost.py update` for the env_* kernels'
        times (env_total_kernel is the sequential sum).

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
sys.path.insert(0, os.path.join(REPO, "path-tracing-svgf_amd"))


def _renderer(scene, W, H, K):
    from ptsvgf.camera import parameter_config
    from ptsvgf.renderer import Renderer

    sc = dataclasses.replace(scene, hdr=scene.hdr.copy(), cache=scene.cache.copy())
    return Renderer(sc, W, H, parameter_config(), mode="fast", aspect_corrected=True, run_taa=False,
                    run_output=False, frames_in_flight=K, host_pace=True)


def run_fps(gl, scene, variant, W, H, K, steps, warmup):
    from ptsvgf.scene import hdr_cache

    r = _renderer(scene, W, H, K)
    m0 = scene.hdr
    dev = None
    if variant == "device":
        import torch

        dev = torch.from_numpy(np.ascontiguousarray(m0)).cuda()
    spans = []
    for f in range(warmup + steps):
        if f == warmup:
            r.flush()
            gl.sync()
            t0 = time.perf_counter()
        t = time.perf_counter()
        if variant == "host":
            r.set_environment(np.roll(m0, 7 * (f + 1), axis=1))
        elif variant == "device":
            import torch

            r.set_environment(torch.roll(dev, 7 * (f + 1), dims=1))
        elif variant == "upload":
            m = np.ascontiguousarray(np.roll(m0, 7 * (f + 1), axis=1))
            c = hdr_cache(m)
            r.flush()
            gl.sync()
            gl.upload_rgb32f(r.hdrMap, m)
            gl.upload_rgb32f(r.hdrCache, c)
        r.frame()
        if f >= warmup:
            spans.append(time.perf_counter() - t)
    r.flush()
    gl.sync()
    dt = time.perf_counter() - t0
    r.close()
    return {"variant": variant, "ms_per_frame": round(1e3 * dt / steps, 4), "fps": round(steps / dt, 2),
            "longest_frame_ms": round(1e3 * max(spans), 3), "median_issue_ms": round(1e3 * float(np.median(spans)), 3),
            "steps": steps, "K": K, "size": [W, H], "map": [int(m0.shape[1]), int(m0.shape[0])]}


def run_update(gl, scene, calls):
    import torch

    r = _renderer(scene, 160, 96, 4)
    for _ in range(4):
        r.frame()
    r.flush()
    gl.sync()
    m0 = scene.hdr
    maps = [np.ascontiguousarray(np.roll(m0, 11 * (i + 1), axis=1)) for i in range(8)]
    out = {}
    for source in ("host", "device"):
        src = maps if source == "host" else [torch.from_numpy(m).cuda() for m in maps]
        for i in range(6):  # the first updates allocate
            gl.environment_update(r.hdrMap, r.hdrCache, src[i % 8])
        torch.cuda.synchronize()  # (every stream: the builds run on a stream of their own)
        host, done = [], []
        for i in range(calls):
            t = time.perf_counter()
            gl.environment_update(r.hdrMap, r.hdrCache, src[i % 8])
            host.append(time.perf_counter() - t)
            torch.cuda.synchronize()
            done.append(time.perf_counter() - t)
        out[source] = {"host_ms_per_call_median": round(1e3 * float(np.median(host)), 3),
                       "issue_to_done_ms_median": round(1e3 * float(np.median(done)), 3)}
    state = gl.environment_state(r.hdrMap)
    r.close()
    return {"map": [int(m0.shape[1]), int(m0.shape[0])], "calls": calls, **out, **state}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("mode", choices=("fps", "update"))
    ap.add_argument("--variants", default="none,host,device,upload")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--upload-steps", type=int, default=8, help="steps of the upload variant (each waits for the host)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--frames-in-flight", type=int, default=4)
    ap.add_argument("--calls", type=int, default=40)
    a = ap.parse_args(argv)
    from ptsvgf import gl
    from ptsvgf.scene import build_scene

    scene = build_scene("table_clock_plant")
    gl.init(0)
    try:
        if a.mode == "update":
            print(json.dumps({"mode": "update", **run_update(gl, scene, a.calls)}), flush=True)
        else:
            for rep in range(a.reps):
                for v in a.variants.split(","):
                    slow = v == "upload"
                    res = run_fps(gl, scene, v, a.width, a.height, a.frames_in_flight,
                                  a.upload_steps if slow else a.steps, 2 if slow else a.warmup)
                    print(json.dumps({"mode": "fps", "rep": rep, **res}), flush=True)
    finally:
        gl.shutdown()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
