#!/usr/bin/env python3
"""Cost and effect of SVGF from sample moments (DESIGN.md "SVGF from sample moments") on the bench scene at 4K.
Every run is a fresh child process; this tree and the parent commit's tree (a checkout with its libraries built,
--parent-tree) alternate, --reps times each.

  bench     `bench.py --gpus 1` of each tree: the headline frames/s (the unchanged path).
  plain     Renderer(frames_in_flight=4, spp=4) of each tree, no switch: frames/s over --steps frames.
  cost      this tree, N = 4, K = 4, the switch off and on: frames/s.
  quality   this tree, one frame at a time, a still camera, N in --spps, the switch off and on, with and without
            adaptive = 1: the RMSE on surface pixels of the chain's output (modulate) against a converged image
            (`accumulate` over --converge frames of the same view at one sample, as tools/adaptive_cost.py builds it)
            at frames 1, 2, 4, 8, 32 and 150 of a fresh history.
  trace     a few frames, one at a time, N = 4, the switch off then on, for a kernel trace of its own:
            rocprofv3 --kernel-trace --stats -- python tools/sample_moments_cost.py --child trace

    python tools/sample_moments_cost.py --parent-tree DIR [--reps 2] [--out profiles/sample_moments/cost.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AT = (1, 2, 4, 8, 32, 150)


def _setup(a):
    tree = os.path.abspath(a.tree) if a.tree else REPO
    sys.path.insert(0, os.path.join(tree, "path-tracing-svgf_amd"))
    from ptsvgf import gl
    from ptsvgf.scene import build_scene

    scene = build_scene("table_clock_plant")
    gl.init(0)
    return gl, scene


def _renderer(scene, a, k, cfg=None, **kw):
    from ptsvgf.camera import parameter_config
    from ptsvgf.renderer import Renderer

    return Renderer(scene, a.width, a.height, cfg or parameter_config(), mode="fast", aspect_corrected=True,
                    run_taa=False, run_output=False, frames_in_flight=k, **kw)


def _fps(r, a):
    import torch

    def frames(n):
        for _ in range(n):
            r.frame()
        r.flush()
        torch.cuda.synchronize()

    frames(a.warmup)
    t0 = time.perf_counter()
    frames(a.steps)
    return round(a.steps / (time.perf_counter() - t0), 2)


def child_plain(a):
    gl, scene = _setup(a)
    r = _renderer(scene, a, a.k, spp=4)
    fps = _fps(r, a)
    r.close()
    gl.shutdown()
    print(json.dumps(dict(kind="plain", tree="parent" if a.tree else "this", fps=fps)), flush=True)


def child_cost(a):
    gl, scene = _setup(a)
    out = {}
    for on in (False, True, False, True):
        r = _renderer(scene, a, a.k, spp=4, sample_moments=on)
        out.setdefault("on" if on else "off", []).append(_fps(r, a))
        r.close()
    gl.shutdown()
    print(json.dumps(dict(kind="cost", fps=out)), flush=True)


def child_quality(a):
    import torch

    gl, scene = _setup(a)
    from ptsvgf.camera import parameter_config

    def plane(r, key):
        return torch.from_numpy(gl.readback(r.planes()[key])).cuda()

    cfg = parameter_config()
    cfg.accumulate_color = True
    r = _renderer(scene, a, 1, cfg)
    for _ in range(a.converge):
        r.frame()
    conv = plane(r, "color")[..., :3]
    surf = plane(r, "normal_depth")[..., 3] != 1.0
    r.close()
    rows = []
    for n in a.spps:
        for tau in (None, 1.0):
            for on in (False, True):
                r = _renderer(scene, a, 1, spp=n, adaptive=tau, sample_moments=on)
                row = dict(spp=n, adaptive=tau, sample_moments=on, rmse={})
                for f in range(1, max(AT) + 1):
                    r.frame()
                    if f in AT:
                        d = (plane(r, "modulate")[..., :3] - conv)[surf]
                        row["rmse"][str(f)] = round(float(torch.sqrt((d * d).mean())), 5)
                r.close()
                rows.append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
    gl.shutdown()
    print(json.dumps(dict(kind="quality", converge=a.converge, rows=rows)), flush=True)


def child_trace(a):
    import torch

    gl, scene = _setup(a)
    for on in (False, True):
        r = _renderer(scene, a, 1, spp=4, sample_moments=on)
        for _ in range(a.profile_frames):
            r.frame()
        r.flush()
        torch.cuda.synchronize()
        r.close()
    gl.shutdown()
    print(json.dumps(dict(kind="trace")), flush=True)


def _stat(v):
    import numpy as np

    return dict(median=round(float(np.median(v)), 4), min=round(float(np.min(v)), 4), max=round(float(np.max(v)), 4),
                n=len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=("plain", "cost", "quality", "trace"))
    ap.add_argument("--tree", default=None, help="(child) the tree whose package and libraries to load")
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its libraries built")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--steps", type=int, default=120)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--profile-frames", type=int, default=12)
    ap.add_argument("--converge", type=int, default=1024)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--spps", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--skip", nargs="*", default=[], choices=("bench", "plain", "cost", "quality"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return dict(plain=child_plain, cost=child_cost, quality=child_quality, trace=child_trace)[a.child](a)
    common = ["--steps", str(a.steps), "--warmup", str(a.warmup), "--profile-frames", str(a.profile_frames), "--width",
              str(a.width), "--height", str(a.height), "--k", str(a.k), "--converge", str(a.converge), "--spps"] + \
             [str(n) for n in a.spps]
    trees = [("this", REPO)] + ([("parent", os.path.abspath(a.parent_tree))] if a.parent_tree else [])
    runs = []
    me = os.path.abspath(__file__)

    def run(cmd, tag, timeout=900):
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
        if p.returncode != 0:  # stop: nothing more is started on the device after a failed run
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit(f"{tag} ended with status {p.returncode}")
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
        print(tag, line, flush=True)
        return json.loads(line)

    for rep in range(a.reps):
        for name, tree in (trees if rep % 2 == 0 else trees[::-1]):
            if "bench" not in a.skip:
                b = run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "100", "--warmup", "10",
                         "--no-cpu-baseline", "--no-1080p", "--no-extras"], f"bench {name}")
                runs.append(dict(kind="bench", tree=name, fps=b["value"]))
            if "plain" not in a.skip:
                cmd = [sys.executable, me, "--child", "plain"] + common
                runs.append(run(cmd + (["--tree", tree] if name == "parent" else []), f"plain {name}"))
        if "cost" not in a.skip:
            runs.append(run([sys.executable, me, "--child", "cost"] + common, "cost"))
    if "quality" not in a.skip:
        runs.append(run([sys.executable, me, "--child", "quality"] + common, "quality", timeout=1100))
    summary = {}
    for name, _ in trees:
        for kind in ("bench", "plain"):
            v = [r["fps"] for r in runs if r["kind"] == kind and r.get("tree") == name]
            if v:
                summary.setdefault(name, {})[kind + "_fps"] = _stat(v)
    cost = [r["fps"] for r in runs if r["kind"] == "cost"]
    if cost:
        summary["cost_fps"] = {k: _stat([x for c in cost for x in c[k]]) for k in ("off", "on")}
    print(json.dumps(dict(summary=summary)))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(runs=runs, summary=summary), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
