"""Headless render to image files: the reference's window loop (main.cpp:436-602) for N frames with the
debug-view switch of its GUI (main.cpp:398-415, gui_config.h:7-45) as a flag, the output pass's display image
written as PNG and, optionally, the selected plane's raw floats as PFM.

    python -m ptsvgf.render_cli --width 800 --height 800 --frames 8 --view final_pic --png out.png

--sway DEG bends the bench scene's plant on the device each frame (Renderer.set_skin / skin_objects).
--light-orbit DEG turns point light 0 about the scene's vertical axis each frame (Renderer.set_lights).
--hue-cycle DEG [--hue-object K] turns the hue of object K's baseColor each frame (Renderer.set_materials).
--sky-turn DEG turns the environment map about the vertical axis by DEG per frame (Renderer.set_environment).
--pick X,Y (repeatable) prints, after the last frame, one JSON line {"pick": {...}} with what lies under pixel (X, Y)
of the last frame's view (Y from the bottom row; Renderer.pick), or {"pick": null}.
"""
from __future__ import annotations

import argparse
import json
import struct
import zlib

import numpy as np


def write_png(path: str, rgb01: np.ndarray) -> None:
    """8-bit RGB PNG of an (H, W, 3) image in [0, 1], GL row 0 (bottom) written last (images are top-down)."""
    img = np.clip(np.round(np.nan_to_num(rgb01[::-1, :, :3]) * 255.0), 0, 255).astype(np.uint8)
    h, w, _ = img.shape
    raw = b"".join(b"\x00" + img[y].tobytes() for y in range(h))

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def write_pfm(path: str, rgb: np.ndarray) -> None:
    """Portable float map (little endian), rows bottom-up as PFM stores them = GL row order."""
    h, w, _ = rgb.shape
    with open(path, "wb") as f:
        f.write(f"PF\n{w} {h}\n-1.0\n".encode())
        f.write(np.ascontiguousarray(rgb[..., :3], "<f4").tobytes())


SWAY_BONES = 8
SWAY_PERIOD = 48  # frames per swing


def _sway_setup(r, scene, obj: int = 2):
    """--sway: the scene rebuilt on the device with its raster list, the corners of object `obj` (the bench scene's
    plant) skinned to a chain of SWAY_BONES bones up its vertical extent. Returns bend_deg -> the chain's matrices."""
    from . import skin

    tp, rp = skin.corner_positions(scene.tri_enc), skin.corner_positions_raster(scene.raster)
    tmask = np.repeat(scene.tri_enc[:, 42] == float(obj), 3)
    rmask = np.repeat(np.asarray(scene.raster_obj) == obj, 3)
    if not tmask.any():
        raise SystemExit(f"--sway: the scene has no object {obj}")
    lo, hi = tp[tmask].min(axis=0), tp[tmask].max(axis=0)
    base = np.array([(lo[0] + hi[0]) / 2, lo[1], (lo[2] + hi[2]) / 2])
    tip = np.array([base[0], hi[1], base[2]])
    r.rebuild_bvh(raster=scene.raster)
    tb, tw = skin.chain_weights(tp, base, tip, SWAY_BONES, tmask)
    rb, rw = skin.chain_weights(rp, base, tip, SWAY_BONES, rmask)
    r.set_skin(tb, tw, rb, rw)
    return lambda deg: skin.chain_bones(base, tip, SWAY_BONES, deg, (0.0, 0.0, 1.0))


def sky_shift(f: int, deg: float, width: int) -> int:
    """--sky-turn: the columns the original map is rolled by before frame f."""
    return int(round(f * deg / 360.0 * width))


def _light_orbit_setup(scene, light: int = 0):
    """--light-orbit: frame count -> the light's record turned by that many steps about the vertical (y) axis through
    the middle of the scene's bounds. Each position is turned from the first one, so the steps do not accumulate
    rounding."""
    from . import skin

    if scene.lights.shape[0] <= light:
        raise SystemExit(f"--light-orbit: the scene has no light {light}")
    tp = skin.corner_positions(scene.tri_enc)
    tp = tp[np.all(np.isfinite(tp), axis=1)]
    cx, cz = ((tp[:, 0].min() + tp[:, 0].max()) / 2, (tp[:, 2].min() + tp[:, 2].max()) / 2) if len(tp) else (0.0, 0.0)
    rec0 = np.array(scene.lights[light], np.float64)

    def at(deg: float) -> np.ndarray:
        c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
        x, z = rec0[0] - cx, rec0[2] - cz
        rec = rec0.copy()
        rec[0], rec[2] = cx + c * x + s * z, cz - s * x + c * z
        return rec.astype(np.float32)

    return at


def main(argv=None) -> int:
    from . import gl
    from .camera import parameter_config
    from .renderer import Renderer
    from .scene import build_scene, load_hdr

    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--scene", default="table_clock_plant")
    ap.add_argument("--hdr", default=None, help="Radiance .hdr environment (default: the synthetic room.hdr)")
    ap.add_argument("--view", default="final_pic", choices=Renderer.VIEWS)
    ap.add_argument("--orbit", type=float, default=0.0, help="degrees per frame (moving camera)")
    ap.add_argument("--mode", default="fast", choices=("fast", "reference"))
    ap.add_argument("--png", default="render.png")
    ap.add_argument("--pfm", default=None, help="also write the selected plane's floats")
    ap.add_argument("--spp", type=int, default=1, help="path-tracing samples per pixel per frame (1 .. 8)")
    ap.add_argument("--adaptive", type=float, default=None, metavar="TAU",
                    help="adaptive sample counts: relative tolerance of a pixel's mean luminance (needs --spp >= 2)")
    ap.add_argument("--adaptive-pool", type=float, default=None, metavar="W",
                    help="pool the sample statistics over frames, the pooled weight held to W >= 2 (needs --adaptive)")
    ap.add_argument("--adaptive-rule", default="relative", choices=("relative", "absolute"),
                    help="TAU bounds the error relative to the mean luminance, or absolutely (needs --adaptive-pool)")
    ap.add_argument("--sample-moments", action="store_true",
                    help="SVGF's variance from the samples' own moments (needs --spp >= 2)")
    ap.add_argument("--sway", type=float, default=None, metavar="DEG",
                    help="bend the plant (object 2) by an 8-bone chain, the angle a sine over the frames of this amplitude")
    ap.add_argument("--light-orbit", type=float, default=0.0, metavar="DEG",
                    help="turn point light 0 about the scene's vertical axis by DEG per frame (moving light)")
    ap.add_argument("--hue-cycle", type=float, default=0.0, metavar="DEG",
                    help="turn the hue of one object's baseColor by DEG per frame (material edits in place)")
    ap.add_argument("--sky-turn", type=float, default=0.0, metavar="DEG",
                    help="turn the environment map by DEG per frame: its columns rolled from the original (environment edits)")
    ap.add_argument("--hue-object", type=int, default=1, metavar="K", help="the object --hue-cycle recolours")
    ap.add_argument("--pick", action="append", default=[], metavar="X,Y",
                    help="after the last frame print {\"pick\": ...} for the pixel (Y from the bottom row); repeatable")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    picks = []
    for s in a.pick:
        try:
            x, y = (int(v) for v in s.split(","))
        except ValueError:
            ap.error(f"--pick {s!r}: expected X,Y")
        if not (0 <= x < a.width and 0 <= y < a.height):
            ap.error(f"--pick {s!r}: outside {a.width} x {a.height}")
        picks.append((x, y))

    scene = build_scene(a.scene)
    if a.hdr:
        from .scene import hdr_cache
        scene.hdr = load_hdr(a.hdr)
        scene.cache = hdr_cache(scene.hdr)
    gl.init(a.device)
    try:
        r = Renderer(scene, a.width, a.height, parameter_config(), mode=a.mode, run_taa=True, run_output=True,
                     spp=a.spp, adaptive=a.adaptive, adaptive_pool=a.adaptive_pool, adaptive_rule=a.adaptive_rule,
                     sample_moments=a.sample_moments)
        r.set_view(a.view)
        sway = _sway_setup(r, scene) if a.sway is not None else None
        light_at = _light_orbit_setup(scene) if a.light_orbit else None
        hue0 = None
        if a.hue_cycle:
            from .materials import hue_turned, object_material

            try:
                hue0 = object_material(scene.tri_enc, a.hue_object)  # each hue is turned from the first material
            except ValueError as e:
                raise SystemExit(f"--hue-cycle: {e}")
        sky0 = np.array(scene.hdr, np.float32, copy=True) if a.sky_turn else None  # each turn rolls the original
        for f in range(a.frames):
            if sky0 is not None:
                r.set_environment(np.roll(sky0, sky_shift(f, a.sky_turn, sky0.shape[1]), axis=1))
            if hue0 is not None:
                r.set_materials({a.hue_object: hue_turned(hue0, a.hue_cycle * (f + 1))})
            if light_at is not None:
                r.set_lights(light_at(a.light_orbit * (f + 1)), first=0)
            if a.orbit:
                r.camera.orbit(a.orbit, 0.0)
            if sway is not None:
                r.skin_objects(sway(a.sway * float(np.sin(2.0 * np.pi * (f + 1) / SWAY_PERIOD))))
            r.frame()
        gl.sync()
        write_png(a.png, gl.readback(r.planes()["output"]))
        if a.pfm:
            write_pfm(a.pfm, gl.readback(r._view_plane(r.frame_index - 1)))
        for x, y in picks:
            print(json.dumps({"pick": r.pick(x, y)}))
        r.close()
    finally:
        gl.shutdown()
    print(f"wrote {a.png}" + (f" and {a.pfm}" if a.pfm else ""))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
