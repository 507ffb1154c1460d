#!/usr/bin/env python3
"""Cost of N samples per pixel per frame (DESIGN.md "Samples per pixel") on the bench scene at 4K, K = 4, for
spp in {1, 2, 4, 8}: one JSON line per run and a summary with the median and the min-max range of each figure.

  native     Renderer(frames_in_flight=4, spp=N) on this tree's library: frames/s of the whole pipeline (G-buffer, path
             tracer, SVGF chain) over --steps frames, and the path tracer's ms per frame from the library's draw
             events with one draw at a time (Renderer.profile).
  yardstick  the same pixels without the feature: N path-tracing passes with the counters F * N + s in one
             pt_pass_draw_batch (N primary stages, N sets of output planes) and a mean on the device (torch, in
             sample order, N elementwise launches), timed with events around both, one frame at a time. It runs
             against the library in --parent-lib (the parent commit's build), which knows nothing of spp.

Each run is a fresh child process (a process loads one library); the two kinds alternate, --reps times each.

    python tools/spp_cost.py --parent-lib path-tracing-svgf_amd/lib_prev [--reps 2] [--out profiles/spp/spp_cost.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "path-tracing-svgf_amd"))
SPPS = (1, 2, 4, 8)


def _stat(v):
    import numpy as np

    return dict(median=round(float(np.median(v)), 4), min=round(float(np.min(v)), 4), max=round(float(np.max(v)), 4),
                n=len(v))


def _setup():
    from ptsvgf import gl
    from ptsvgf.scene import build_scene

    scene = build_scene("table_clock_plant")
    gl.init(0)
    return gl, scene


def child_native(a):
    import torch

    from ptsvgf.camera import parameter_config
    from ptsvgf.renderer import Renderer

    gl, scene = _setup()
    out = {}
    for n in a.spps:
        r = Renderer(scene, a.width, a.height, parameter_config(), mode="fast", aspect_corrected=True, run_taa=False,
                     run_output=False, frames_in_flight=a.k, spp=n)
        for _ in range(a.warmup):
            r.frame()
        r.flush()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            r.frame()
        r.flush()
        torch.cuda.synchronize()
        fps = a.steps / (time.perf_counter() - t0)
        r.profile(True)
        for _ in range(a.profile_frames):
            r.frame()
        r.flush()
        torch.cuda.synchronize()
        pt_ms = r.pass_times()["pathtrace"] / a.profile_frames
        r.profile(False)
        r.close()
        out[str(n)] = dict(fps=round(fps, 2), frame_ms=round(1e3 / fps, 4), pathtrace_ms=round(pt_ms, 4))
    gl.shutdown()
    print(json.dumps(dict(kind="native", spp=out)), flush=True)


def child_yardstick(a):
    import torch

    from ptsvgf.camera import parameter_config
    from ptsvgf.renderer import Renderer

    gl, scene = _setup()
    out = {}
    for n in a.spps:
        tensors = {}

        def factory(w, h):
            t = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
            handle = gl.wrap_device_texture(t.data_ptr(), w, h)
            tensors[handle] = t
            return handle

        k = max(a.k, n)
        r = Renderer(scene, a.width, a.height, parameter_config(), mode="fast", aspect_corrected=True, run_taa=False,
                     run_output=False, frames_in_flight=k, tex_factory=factory)
        for _ in range(max(a.warmup, k)):  # every slot's pass bound
            r.frame()
        r.flush()
        torch.cuda.synchronize()
        stream = torch.cuda.current_stream()
        r._stream_to(stream)
        passes = [p for p, _ in r.pt_slots[:n]]
        cols = [tensors[outs[0]] for _, outs in r.pt_slots[:n]]
        mean = torch.empty_like(cols[0])
        passes[0].set_uniform_int("trace_batch", n)
        ms = []
        for f in range(a.profile_frames + 2):
            for s, p in enumerate(passes):
                p.set_uniform_uint("frameCounter", f * n + s)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            gl.draw_batch(passes)
            if n > 1:
                torch.add(cols[0], cols[1], out=mean)
                for c in cols[2:]:
                    mean.add_(c)
                mean.div_(float(n))
            e1.record(stream)
            torch.cuda.synchronize()
            if f >= 2:
                ms.append(e0.elapsed_time(e1))
        r.close()
        out[str(n)] = dict(pathtrace_ms=round(sum(ms) / len(ms), 4))
    gl.shutdown()
    lib = "parent commit" if os.environ.get("PTSVGF_LIB_DIR") else "this tree"
    print(json.dumps(dict(kind="yardstick", lib=lib, spp=out)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=("native", "yardstick"))
    ap.add_argument("--parent-lib", default=None, help="directory of the parent commit's libraries (the yardstick's)")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--steps", type=int, default=120)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--profile-frames", type=int, default=12)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--spps", type=int, nargs="+", default=list(SPPS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return (child_native if a.child == "native" else child_yardstick)(a)
    runs = []
    common = [sys.executable, os.path.abspath(__file__), "--steps", str(a.steps), "--warmup", str(a.warmup),
              "--profile-frames", str(a.profile_frames), "--width", str(a.width), "--height", str(a.height), "--k",
              str(a.k), "--spps"] + [str(n) for n in a.spps]
    for rep in range(a.reps):
        for kind in (("native", "yardstick") if rep % 2 == 0 else ("yardstick", "native")):
            env = dict(os.environ)
            if kind == "yardstick" and a.parent_lib:
                env["PTSVGF_LIB_DIR"] = os.path.abspath(a.parent_lib)
            p = subprocess.run(common + ["--child", kind], env=env, capture_output=True, text=True, timeout=900)
            if p.returncode != 0:  # stop: nothing more is started on the device after a failed run
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit(f"{kind} run ended with status {p.returncode}")
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
            print(line, flush=True)
            runs.append(json.loads(line))
    summary = dict(width=a.width, height=a.height, k=a.k, steps=a.steps, reps=a.reps)
    for kind in ("native", "yardstick"):
        mine = [r["spp"] for r in runs if r["kind"] == kind]
        summary[kind] = {n: {key: _stat([m[n][key] for m in mine]) for key in mine[0][n]} for n in mine[0]}
    print(json.dumps(dict(summary=summary)))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(runs=runs, summary=summary), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
