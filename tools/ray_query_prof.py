#!/usr/bin/env python3
"""Ray-query throughput on the bench scene (DESIGN.md "Ray queries"): the two kernel variants, one ray per lane
against lane refill, on (a) the primary rays of the 4K bench view and (b) 2^22 incoherent rays whose origins are (a)'s
hit points and whose directions are seeded uniform, each as a closest-hit and as an occlusion query.

Per workload and query: warm-up runs of both variants, then `--reps` repetitions alternating the variants, each timed
with HIP events around as many back-to-back queries as last at least `--min-seconds`. The two variants' results on the
timed inputs are compared for equality. Prints a table (Mrays/s, mean and spread = max - min over the repetitions) and
one JSON line; --out also writes them to a file.

    python tools/ray_query_prof.py --out profiles/ray_queries/ray_query_prof.log
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "path-tracing-svgf_amd"))

VARIANTS = ((0, "lane"), (1, "refill"))


def main(argv=None) -> int:
    import numpy as np
    import torch

    from ptsvgf import gl
    from ptsvgf._lib import check, pt
    from ptsvgf.camera import Camera, rigid_inverse
    from ptsvgf.scene import build_scene

    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--incoherent", type=int, default=1 << 22)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--scene", default="table_clock_plant")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)

    scene = build_scene(a.scene)
    gl.init(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    try:
        check(pt().pt_set_stream(torch.cuda.current_stream().cuda_stream))
        tt, nt = gl.texture_buffer(scene.tri_enc), gl.texture_buffer(scene.node_enc)
        W, H = a.width, a.height
        cam = Camera(W, H)
        cam.update()
        n_a = W * H
        # every pixel, written on the device
        rays_a = torch.empty((n_a, 8), dtype=torch.float32, device="cuda")
        eye = np.ascontiguousarray(cam.cam_position, np.float32)
        rot = np.ascontiguousarray(rigid_inverse(cam.cam_view_mat), np.float32).reshape(16)
        check(pt().pt_rays_primary(eye.ctypes.data_as(C.POINTER(C.c_float)), rot.ctypes.data_as(C.POINTER(C.c_float)),
                                   W, H, 1 if W != H else 0, None, n_a, C.c_void_p(rays_a.data_ptr())))
        hits_a = gl.rays_closest(tt, nt, rays_a)
        torch.cuda.synchronize()
        on = hits_a.view(torch.int32)[:, 1] >= 0
        P = hits_a[on][:, 4:7]
        say(f"scene {a.scene}: {scene.ntris} triangles; (a) {n_a} primary rays of the {W}x{H} bench view, "
            f"{int(on.sum())} hit")
        n_b = a.incoherent
        g = torch.Generator(device="cuda").manual_seed(20240607)
        d = torch.randn((n_b, 3), generator=g, device="cuda", dtype=torch.float32)
        d = d / d.norm(dim=1, keepdim=True)
        rays_b = torch.zeros((n_b, 8), dtype=torch.float32, device="cuda")
        rays_b[:, 0:3] = P[torch.arange(n_b, device="cuda") % P.shape[0]]
        rays_b[:, 4:7] = d
        rays_b[:, 7] = float("inf")
        torch.cuda.synchronize()
        say(f"(b) {n_b} incoherent rays: origins (a)'s hit points, seeded uniform directions")

        results = []
        for wname, rays in (("a primary", rays_a), ("b incoherent", rays_b)):
            n = rays.shape[0]
            for qname in ("closest", "occluded"):
                out = {v: (torch.empty((n, 8), dtype=torch.float32, device="cuda") if qname == "closest"
                           else torch.empty((n,), dtype=torch.uint8, device="cuda")) for v, _ in VARIANTS}
                fn = pt().pt_rays_closest if qname == "closest" else pt().pt_rays_occluded

                def run(v, count):
                    gl.rays_variant(v)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(count):
                        check(fn(tt, nt, C.c_void_p(rays.data_ptr()), n, C.c_void_p(out[v].data_ptr())))
                    e1.record()
                    e1.synchronize()
                    return e0.elapsed_time(e1) / 1e3

                def bits_equal():  # (as integers: tri = -1 read as a float is a NaN)
                    a0, a1 = (out[v].view(torch.int32) if qname == "closest" else out[v] for v, _ in VARIANTS)
                    return bool(torch.equal(a0, a1))

                once = {}
                for v, _ in VARIANTS:
                    for _ in range(a.warmup):
                        once[v] = run(v, 1)
                same = bits_equal()
                rate = {v: [] for v, _ in VARIANTS}
                for _ in range(a.reps):
                    for v, _ in VARIANTS:  # alternating
                        count = max(1, int(np.ceil(a.min_seconds / max(once[v], 1e-6))))
                        s = run(v, count)
                        rate[v].append(n * count / s / 1e6)
                same = same and bits_equal()
                row = {"workload": wname, "query": qname, "rays": n, "equal": same}
                for v, name in VARIANTS:
                    row[name] = {"mrays_s": [round(x, 1) for x in rate[v]], "mean": round(float(np.mean(rate[v])), 1),
                                 "spread": round(float(max(rate[v]) - min(rate[v])), 1)}
                results.append(row)
                say(f"{wname:13s} {qname:9s} lane {row['lane']['mean']:8.1f} Mrays/s (spread {row['lane']['spread']:.1f}, "
                    f"{row['lane']['mrays_s']})  refill {row['refill']['mean']:8.1f} (spread {row['refill']['spread']:.1f}, "
                    f"{row['refill']['mrays_s']})  results equal: {same}")
        gl.rays_variant(-1)
        say(json.dumps({"ray_query_prof": results}))
        ok = all(r["equal"] for r in results)
    finally:
        gl.shutdown()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    raise SystemExit(main())
