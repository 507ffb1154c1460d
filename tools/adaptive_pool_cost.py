#!/usr/bin/env python3
"""Cost and quality of pooled adaptive sample counts (DESIGN.md "Pooled sample statistics") on the bench scene at 4K,
K = 4, beside the un-pooled rule and uniform counts. Modelled on tools/adaptive_cost.py, whose helpers it uses; every
run is a fresh child process.

  unchanged  `bench.py --gpus 1` and Renderer(spp=4, adaptive=1.0) of this tree and of the parent commit's tree (a
             checkout with its libraries built, --parent-tree), alternating, --reps times each.
  feature    this tree, a still camera and one orbiting 1 degree per frame: uniform N (2, 3 and --spps), the un-pooled
             rule per tolerance, and the pooled rule per tolerance, rule and w_max: frames/s, the path tracer's draw,
             the mean count over all pixels and over surface pixels, bounce + shadow rays of one frame, the share of
             surface pixels at N for lack of an estimate (miss) and, for the still camera, the RMSE on surface pixels
             of the path tracer's colour and of the chain's output (modulate) against a converged image.
  trace      a few frames of the un-pooled and the pooled renderer, one frame at a time, for a kernel trace of its own:
             rocprofv3 --kernel-trace --stats -- python tools/adaptive_pool_cost.py --child trace

    python tools/adaptive_pool_cost.py --parent-tree DIR [--reps 2] [--out profiles/adaptive_pool/cost.json]
"""
import argparse
import json
import os
import subprocess
import sys

from adaptive_cost import TAUS, _one_frame, _planes, _renderer, _setup, _stat, _timed, _tree

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RULES = ("relative", "absolute")


def child_unchanged(a):
    gl, scene = _setup()
    r = _renderer(scene, a, spp=4, adaptive=1.0)
    out = _timed(r, a)
    r.close()
    gl.shutdown()
    print(json.dumps(dict(kind="unchanged", tree="parent" if a.tree else "this", adaptive=out)), flush=True)


def _one_frame_pool(gl, r, a, orbit):
    """adaptive_cost._one_frame for a pooled renderer: the miss share is read off the frame's own pool plane (a
    surface pixel misses when a surface texel of its 3 x 3 block holds a weight below 2)."""
    import torch
    import torch.nn.functional as F

    n, out = r.spp, {}
    if orbit:
        r.camera.orbit(orbit, 0.0)
    st = r.trace_stats()
    out["rays"] = st["bounce_rays"] + st["shadow_rays"]
    pl = _planes(gl, r, ("color", "modulate", "normal_depth"))
    surf = pl["normal_depth"][..., 3] != 1.0
    c = torch.from_numpy(r.sample_counts()).cuda().clamp(1, n).float()
    w = torch.from_numpy(r.sample_pool()).cuda()[..., 2]
    none = (surf & (w < 2)).float()
    miss = (F.max_pool2d(none[None, None], 3, 1, 1)[0, 0] > 0) & surf
    out["mean_count"] = round(float(c.mean()), 4)
    out["mean_count_surface"] = round(float(c[surf].mean()), 4)
    out["miss_share"] = round(float(miss.sum() / surf.sum().clamp(min=1)), 5)
    return out, pl, surf


def _configs(a):
    for n in (2, 3):
        yield dict(spp=n, tau=None)
    for n in a.spps:
        yield dict(spp=n, tau=None)
        for tau in a.taus:
            yield dict(spp=n, tau=tau)
        for rule in RULES:
            for wmax in a.wmaxs:
                for tau in a.taus:
                    yield dict(spp=n, tau=tau, rule=rule, w_max=wmax)


def child_feature(a):
    import torch

    from ptsvgf.camera import parameter_config
    from ptsvgf.renderer import Renderer

    gl, scene = _setup()
    cfg = parameter_config()
    cfg.accumulate_color = True  # the converged image of the still view: one sample per pixel, one frame at a time
    r = Renderer(scene, a.width, a.height, cfg, mode="fast", aspect_corrected=True, run_taa=False, run_output=False)
    for _ in range(a.converge):
        r.frame()
    conv = _planes(gl, r, ("color",))["color"][..., :3]
    r.close()
    rows = []
    for orbit in (0.0, 1.0):
        for c in _configs(a):
            kw = dict(adaptive_pool=c["w_max"], adaptive_rule=c["rule"]) if "rule" in c else {}
            r = _renderer(scene, a, spp=c["spp"], adaptive=c["tau"], **kw)
            row = dict(camera="still" if not orbit else "orbit 1 deg/frame", **c)
            row.update(_timed(r, a, orbit))
            more, pl, surf = (_one_frame_pool if kw else _one_frame)(gl, r, a, orbit)
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
    import torch

    gl, scene = _setup()
    for kw in (dict(), dict(adaptive_pool=a.wmaxs[0])):
        r = _renderer(scene, a, k=1, spp=4, adaptive=1.0, **kw)
        for _ in range(a.profile_frames):
            r.frame()
        r.flush()
        torch.cuda.synchronize()
        r.close()
    gl.shutdown()
    print(json.dumps(dict(kind="trace")), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=("unchanged", "feature", "trace"))
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
    ap.add_argument("--wmaxs", type=float, nargs="+", default=[8.0, 32.0])
    ap.add_argument("--skip", nargs="*", default=[], choices=("unchanged", "feature"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        _tree(a)
        return dict(unchanged=child_unchanged, feature=child_feature, trace=child_trace)[a.child](a)
    common = ["--steps", str(a.steps), "--warmup", str(a.warmup), "--profile-frames", str(a.profile_frames), "--width",
              str(a.width), "--height", str(a.height), "--k", str(a.k), "--converge", str(a.converge), "--spps"] + \
             [str(n) for n in a.spps] + ["--taus"] + [str(t) for t in a.taus] + ["--wmaxs"] + [str(w) for w in a.wmaxs]
    trees = [("this", REPO)] + ([("parent", os.path.abspath(a.parent_tree))] if a.parent_tree else [])
    runs = []

    def run(cmd, tag, timeout=900):
        # (the child's stderr passes through: the feature child reports every row there as it goes)
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=timeout)
        if p.returncode != 0:  # stop: nothing more is started on the device after a failed run
            sys.stderr.write(p.stdout[-2000:])
            raise SystemExit(f"{tag} ended with status {p.returncode}")
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
        print(tag, line if len(line) < 400 else line[:400] + " ...", flush=True)
        return json.loads(line)

    me = os.path.abspath(__file__)
    if "unchanged" not in a.skip:
        for rep in range(a.reps):
            for name, tree in (trees if rep % 2 == 0 else trees[::-1]):
                b = run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "100", "--warmup", "10",
                         "--no-cpu-baseline", "--no-1080p", "--no-extras"], f"bench {name}")
                runs.append(dict(kind="bench", tree=name, fps=b["value"]))
                # (the parent's tree has no such tool: this file runs with the parent's package and libraries)
                cmd = [sys.executable, me, "--child", "unchanged"] + common
                runs.append(run(cmd + (["--tree", tree] if name == "parent" else []), f"adaptive {name}"))
    if "feature" not in a.skip:
        runs.append(run([sys.executable, me, "--child", "feature"] + common, "feature", timeout=1150))
    summary = {}
    for name, _ in trees:
        bench = [r["fps"] for r in runs if r["kind"] == "bench" and r["tree"] == name]
        ad = [r["adaptive"] for r in runs if r["kind"] == "unchanged" and r["tree"] == name]
        if bench:
            summary[name] = dict(bench_fps=_stat(bench), adaptive={k: _stat([m[k] for m in ad]) for k in ad[0]})
    feats = [r["rows"] for r in runs if r["kind"] == "feature"]
    if feats:
        summary["feature"] = feats[0]
    print(json.dumps(dict(summary=summary)))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(runs=runs, summary=summary), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
