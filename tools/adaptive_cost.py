#!/usr/bin/env python3
"""Cost and quality of adaptive sample counts (DESIGN.md "Adaptive sample counts") on the bench scene at 4K, K = 4.
Every run is a fresh child process; this tree and the parent commit's tree (a checkout with its libraries built,
--parent-tree) alternate, --reps times each.

  bench     `bench.py --gpus 1` of each tree: the headline frames/s (nothing bound: the unchanged path).
  plain     Renderer(frames_in_flight=4, spp=N) of each tree for N = 1 and 4, no `adaptive`: frames/s over --steps
            frames and the path tracer's ms per draw (one draw at a time).
  feature   this tree, N = 4 and 8, uniform counts and three tolerances, a still camera and one orbiting 1 degree per
            frame: frames/s, the path tracer's draw, the mean count over all pixels and over surface pixels, the share
            of surface pixels that took N for lack of an estimate (miss), bounce + shadow rays of one frame, and, for
            the still camera, the RMSE on surface pixels of the path tracer's colour and of the chain's output
            (modulate) against a converged image: `accumulate` over --converge frames of the same view at one sample.
  trace     a few frames of each launch mix, one frame at a time, for a kernel trace of its own:
            rocprofv3 --kernel-trace --stats -- python tools/adaptive_cost.py --child trace

    python tools/adaptive_cost.py --parent-tree DIR [--reps 2] [--out profiles/adaptive/adaptive_cost.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAUS = (0.5, 1.0, 2.0)


def _tree(a):
    tree = os.path.abspath(a.tree) if a.tree else REPO
    sys.path.insert(0, os.path.join(tree, "path-tracing-svgf_amd"))
    return tree


def _setup():
    from ptsvgf import gl
    from ptsvgf.scene import build_scene

    scene = build_scene("table_clock_plant")
    gl.init(0)
    return gl, scene


def _renderer(scene, a, k=None, **kw):
    from ptsvgf.camera import parameter_config
    from ptsvgf.renderer import Renderer

    return Renderer(scene, a.width, a.height, parameter_config(), mode="fast", aspect_corrected=True, run_taa=False,
                    run_output=False, frames_in_flight=a.k if k is None else k, **kw)


def _timed(r, a, orbit=0.0):
    """frames/s over a.steps frames, then the path tracer's ms per draw with one draw at a time."""
    import torch

    def frames(n):
        for _ in range(n):
            if orbit:
                r.camera.orbit(orbit, 0.0)
            r.frame()
        r.flush()
        torch.cuda.synchronize()

    frames(a.warmup)
    t0 = time.perf_counter()
    frames(a.steps)
    fps = a.steps / (time.perf_counter() - t0)
    r.profile(True)
    frames(a.profile_frames)
    pt_ms = r.pass_times()["pathtrace"] / a.profile_frames
    r.profile(False)
    return dict(fps=round(fps, 2), frame_ms=round(1e3 / fps, 4), pathtrace_ms=round(pt_ms, 4))


def child_plain(a):
    gl, scene = _setup()
    out = {}
    for n in (1, 4):
        r = _renderer(scene, a, spp=n)
        out[str(n)] = _timed(r, a)
        r.close()
    gl.shutdown()
    print(json.dumps(dict(kind="plain", tree="parent" if a.tree else "this", spp=out)), flush=True)


def _miss_share(stats, motion, nd, lag, W, H):
    """Share of the surface pixels whose count is N for lack of an estimate: the position `lag` frames ago is off the
    frame or non-finite, or a texel of the 3 x 3 block there holds none (v < 0, NaN). Torch restatement of the derive
    rule's steps 2 and 3 for this one figure."""
    import torch
    import torch.nn.functional as F

    ys, xs = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32),
                            torch.arange(W, device="cuda", dtype=torch.float32), indexing="ij")
    fx = (xs + 0.5) - (lag * motion[..., 0]) * float(W)
    fy = (ys + 0.5) - (lag * motion[..., 1]) * float(H)
    inside = torch.isfinite(fx) & torch.isfinite(fy) & (fx >= 0) & (fx < W) & (fy >= 0) & (fy < H)
    none = ((stats[..., 1] < 0) | torch.isnan(stats[..., 0]) | torch.isnan(stats[..., 1])).float()
    block = F.max_pool2d(none[None, None], 3, 1, 1)[0, 0] > 0
    qx = torch.where(inside, fx.floor(), torch.zeros_like(fx)).long()
    qy = torch.where(inside, fy.floor(), torch.zeros_like(fy)).long()
    miss = ~inside | block[qy, qx]
    surf = nd[..., 3] != 1.0
    return float((miss & surf).sum() / surf.sum().clamp(min=1))


def _planes(gl, r, keys):
    import torch

    pl = r.planes()
    return {k: torch.from_numpy(gl.readback(pl[k])).cuda() for k in keys}


def _one_frame(gl, r, a, orbit):
    """One more frame after the timed ones: its counts, miss share and ray counters, and its planes."""
    import torch

    n, out = r.spp, {}
    if orbit:
        r.camera.orbit(orbit, 0.0)
    if r.adaptive is not None:
        r.flush()
        torch.cuda.synchronize()
        ad = r._ad[r.frame_index % len(r.pt_slots)]
        prev, lag = ad["stats"].clone(), float(r.frame_index - ad["last"])
    st = r.trace_stats()
    out["rays"] = st["bounce_rays"] + st["shadow_rays"]
    pl = _planes(gl, r, ("color", "modulate", "normal_depth", "velocity"))
    surf = pl["normal_depth"][..., 3] != 1.0
    if r.adaptive is not None:
        c = torch.from_numpy(r.sample_counts()).cuda().clamp(1, n).float()
        out["mean_count"] = round(float(c.mean()), 4)
        out["mean_count_surface"] = round(float(c[surf].mean()), 4)
        out["miss_share"] = round(_miss_share(prev, pl["velocity"], pl["normal_depth"], lag, r.W, r.H), 5)
    else:
        out["mean_count"] = out["mean_count_surface"] = float(n)
    return out, pl, surf


def child_feature(a):
    import torch

    gl, scene = _setup()
    # the converged image of the still view: accumulate at one sample per pixel, one frame at a time
    from ptsvgf.camera import parameter_config
    from ptsvgf.renderer import Renderer

    cfg = parameter_config()
    cfg.accumulate_color = True
    r = Renderer(scene, a.width, a.height, cfg, mode="fast", aspect_corrected=True, run_taa=False, run_output=False)
    for _ in range(a.converge):
        r.frame()
    conv = _planes(gl, r, ("color",))["color"][..., :3]
    r.close()
    rows = []
    for orbit in (0.0, 1.0):
        for n in a.spps:
            for tau in (None,) + tuple(a.taus):
                r = _renderer(scene, a, spp=n, adaptive=tau)
                row = dict(camera="still" if not orbit else "orbit 1 deg/frame", spp=n, tau=tau)
                row.update(_timed(r, a, orbit))
                more, pl, surf = _one_frame(gl, r, a, orbit)
                row.update(more)
                if not orbit:
                    for key in ("color", "modulate"):
                        d = (pl[key][..., :3] - conv)[surf]
                        row["rmse_" + key] = round(float(torch.sqrt((d * d).mean())), 5)
                r.close()
                rows.append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
    gl.shutdown()
    print(json.dumps(dict(kind="feature", converge=a.converge, rows=rows)), flush=True)


def child_trace(a):
    """Launch mixes for a kernel trace, one frame at a time at N = 4: plain, counts + statistics (adaptive), and the
    adaptive renderer's counts with the statistics plane unbound."""
    import torch

    gl, scene = _setup()
    for mix in ("plain", "adaptive", "counts only"):
        r = _renderer(scene, a, k=1, spp=4, adaptive=None if mix == "plain" else a.taus[1])
        for f in range(a.profile_frames):
            if mix == "counts only" and f == 2:  # two frames of statistics, then their counts without new ones
                torch.cuda.synchronize()
                for p, _ in r.pt_slots:
                    p.set_sample_stats(0)
                r.adaptive = None  # (no further derive: the count plane stays)
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
    ap.add_argument("--child", choices=("plain", "feature", "trace"))
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
    ap.add_argument("--spps", type=int, nargs="+", default=[4, 8])
    ap.add_argument("--taus", type=float, nargs="+", default=list(TAUS))
    ap.add_argument("--skip", nargs="*", default=[], choices=("bench", "plain", "feature"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        _tree(a)
        return dict(plain=child_plain, feature=child_feature, trace=child_trace)[a.child](a)
    common = ["--steps", str(a.steps), "--warmup", str(a.warmup), "--profile-frames", str(a.profile_frames), "--width",
              str(a.width), "--height", str(a.height), "--k", str(a.k), "--converge", str(a.converge), "--spps"] + \
             [str(n) for n in a.spps] + ["--taus"] + [str(t) for t in a.taus]
    trees = [("this", REPO)] + ([("parent", os.path.abspath(a.parent_tree))] if a.parent_tree else [])
    runs = []

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
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "plain"] + common
                runs.append(run(cmd + (["--tree", tree] if name == "parent" else []), f"plain {name}"))
        if "feature" not in a.skip:
            runs.append(run([sys.executable, os.path.abspath(__file__), "--child", "feature"] + common, "feature",
                            timeout=1100))
    summary = {}
    for name, _ in trees:
        bench = [r["fps"] for r in runs if r["kind"] == "bench" and r["tree"] == name]
        plain = [r["spp"] for r in runs if r["kind"] == "plain" and r["tree"] == name]
        summary[name] = dict(bench_fps=_stat(bench) if bench else None,
                             plain={n: {k: _stat([m[n][k] for m in plain]) for k in plain[0][n]} for n in plain[0]}
                             if plain else None)
    feats = [r["rows"] for r in runs if r["kind"] == "feature"]
    if feats:
        summary["feature"] = []
        for i, row in enumerate(feats[0]):
            s = dict(camera=row["camera"], spp=row["spp"], tau=row["tau"])
            for k, v in row.items():
                if k not in s:
                    s[k] = _stat([f[i][k] for f in feats])
            summary["feature"].append(s)
    print(json.dumps(dict(summary=summary)))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(runs=runs, summary=summary), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
