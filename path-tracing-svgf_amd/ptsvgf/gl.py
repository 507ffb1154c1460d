"""Python mirror of the reference's GPU plumbing API (layer L2), over the C ABI.

Same names, argument meaning and call order as the reference's C++ classes, so
a port of ``main.cpp`` reads line for line:

==========================================  ===================================
reference (file:line)                       here
==========================================  ===================================
``getShaderProgram`` Utils/shader.h:21-67   :func:`getShaderProgram`
``getTextureRGB32F`` Utils/help_func.h:22   :func:`getTextureRGB32F`
``glTexBuffer(RGB32F)`` main.cpp:136-168    :func:`texture_buffer`
``glTexImage2D(RGB32F)`` main.cpp:173-180   :func:`upload_rgb32f`
``RenderPass`` Utils/render_pass.h:82-182   :class:`RenderPass`
``Rasterize_RenderPass`` render_pass.h:5-80 :class:`Rasterize_RenderPass`
==========================================  ===================================

Errors: where the reference ``exit(-1)``s (missing shader, shader.h:8-12) or
prints (incomplete FBO, render_pass.h:58-59) this raises :class:`PtError`.
Unknown uniform names are ignored, as GL ignores location -1.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import (PT_RGB32F, PT_RGBA32F, PT_TEXTURE_2D, PT_TEXTURE_2D_ARRAY, PT_TEXTURE_BUFFER, check, fptr,
                   pt)

GL_TEXTURE_2D = PT_TEXTURE_2D
GL_TEXTURE_BUFFER = PT_TEXTURE_BUFFER
GL_TEXTURE_2D_ARRAY = PT_TEXTURE_2D_ARRAY
GL_RGB32F = PT_RGB32F
GL_RGBA32F = PT_RGBA32F

SCR_WIDTH = 800   # Utils/camera.h:5-6
SCR_HEIGHT = 800


def init(device: int = 0) -> None:
    check(pt().pt_init(device))


def shutdown() -> None:
    check(pt().pt_shutdown())


def sync() -> None:
    check(pt().pt_sync())


def set_band(frame_w: int, frame_h: int, y0: int, y1: int, row0: int, rows: int) -> None:
    check(pt().pt_set_band(frame_w, frame_h, y0, y1, row0, rows))


def set_profiling(on: bool) -> None:
    check(pt().pt_set_profiling(1 if on else 0))


def getShaderProgram(fshader: str, vshader: str) -> int:
    h = C.c_uint32()
    check(pt().pt_program_create(fshader.encode(), vshader.encode(), C.byref(h)))
    return h.value


def getTextureRGB32F(width: int, height: int) -> int:
    h = C.c_uint32()
    check(pt().pt_texture2d_create(width, height, C.byref(h)))
    return h.value


def wrap_device_texture(ptr: int, width: int, height: int) -> int:
    h = C.c_uint32()
    check(pt().pt_texture2d_wrap(C.c_void_p(ptr), width, height, C.byref(h)))
    return h.value


def upload_rgb32f(tex: int, data: np.ndarray) -> None:
    """glTexImage2D(GL_TEXTURE_2D, 0, GL_RGB32F|GL_RGBA32F, w, h, ...) of a full image (h, w, 3|4)."""
    a = np.ascontiguousarray(data, dtype=np.float32)
    h, w, ch = a.shape
    check(pt().pt_texture2d_upload(tex, w, h, PT_RGB32F if ch == 3 else PT_RGBA32F, fptr(a)))


def texture_buffer(data: np.ndarray) -> int:
    """glGenBuffers + glBufferData + glTexBuffer(GL_TEXTURE_BUFFER, GL_RGB32F, ...)."""
    a = np.ascontiguousarray(data, dtype=np.float32)
    h = C.c_uint32()
    check(pt().pt_texbuffer_create(a.ctypes.data_as(C.c_void_p), a.nbytes, PT_RGB32F, C.byref(h)))
    return h.value


def lights_update(tex: int, first: int, lights) -> None:
    """pt_lights_update: replaces lights first .. of the lights texture buffer `tex` by `lights` ((n, 6) float32:
    position, colour). Draws already enqueued keep the values they were enqueued with; nothing waits for the device."""
    a = np.ascontiguousarray(lights, dtype=np.float32).reshape(-1, 6)
    check(pt().pt_lights_update(tex, int(first), a.shape[0], fptr(a)))


def materials_update(tri_tex: int, first_obj: int, materials, pose: int = 0) -> None:
    """pt_materials_update: objects first_obj .. of the triangle buffer `tri_tex` take `materials` ((n, 18) float32 in
    ptsvgf_scene.h's order; tests/materials_ref.py is the definition). `pose`: the pt_pose_create handle made from that
    buffer, whose rest list is patched too. Draws already enqueued keep their materials; nothing waits for the device."""
    a = np.ascontiguousarray(materials, dtype=np.float32).reshape(-1, 18)
    check(pt().pt_materials_update(tri_tex, int(pose), int(first_obj), a.shape[0], fptr(a)))


def environment_update(hdr_tex: int, cache_tex: int, rgb) -> None:
    """pt_environment_update: a new map of the same size for the hdrMap / hdrCache pair, its importance cache built on
    the device (tests/environment_ref.py is the definition). `rgb` is (h, w, 3) float32: a numpy array, or a contiguous
    CUDA torch tensor, consumed in stream order on the library's current stream. Draws already enqueued keep the
    environment they were enqueued with; nothing waits for the device."""
    if _is_tensor(rgb):
        if not rgb.is_cuda or str(rgb.dtype) != "torch.float32" or not rgb.is_contiguous() or rgb.dim() != 3:
            raise ValueError("environment_update: a contiguous float32 CUDA tensor of shape (h, w, 3)")
        h, w, ch = rgb.shape
        ptr, dev = C.c_void_p(rgb.data_ptr()), 1
    else:
        a = np.ascontiguousarray(rgb, dtype=np.float32)
        if a.ndim != 3:
            raise ValueError("environment_update: an array of shape (h, w, 3)")
        h, w, ch = a.shape
        ptr, dev = a.ctypes.data_as(C.c_void_p), 0
    if ch != 3:
        raise ValueError("environment_update: 3 floats per texel")
    check(pt().pt_environment_update(hdr_tex, cache_tex, ptr, int(w), int(h), dev))


def environment_state(hdr_tex: int) -> dict:
    """pt_debug_environment_state (include/ptsvgf_debug_environment.h): {"version", "device_versions",
    "staging_slots"}."""
    ver, n, m = C.c_uint64(), C.c_int(), C.c_int()
    check(pt().pt_debug_environment_state(hdr_tex, C.byref(ver), C.byref(n), C.byref(m)))
    return {"version": ver.value, "device_versions": n.value, "staging_slots": m.value}


# A hit record of pt_rays_closest (32 bytes; the last float, always 0, has no field)
HIT_DTYPE = np.dtype({"names": ["t", "tri", "obj", "inside", "P"], "formats": ["<f4", "<i4", "<i4", "<i4", ("<f4", (3,))],
                      "offsets": [0, 4, 8, 12, 16], "itemsize": 32})


def _is_tensor(a) -> bool:
    return type(a).__module__.split(".")[0] == "torch"


def _device_rays(rays):
    """(device tensor (n, 8) float32, came from the host) of a ray list given as a numpy array or a torch tensor."""
    import torch

    if _is_tensor(rays):
        if not rays.is_cuda or rays.dtype != torch.float32 or rays.dim() != 2 or rays.shape[1] != 8 \
                or not rays.is_contiguous():
            raise ValueError("rays: a contiguous float32 (n, 8) device tensor")
        return rays, False
    a = np.ascontiguousarray(rays, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] != 8:
        raise ValueError(f"rays: float32 (n, 8), got {a.shape}")
    t = torch.from_numpy(a).cuda()
    torch.cuda.current_stream().synchronize()  # the upload, before the library's stream reads it
    return t, True


def rays_closest(tri_tex: int, node_tex: int, rays):
    """pt_rays_closest: the closest hit of every ray (8 floats: origin, -, direction as given, tmax) over the scene in
    (tri_tex, node_tex), as the reference's hitBVH returns it (tests/ray_query_ref.py). A numpy (n, 8) array is
    uploaded, the call synchronises, and a structured array (HIT_DTYPE: t, tri, obj, inside, P) comes back. A torch
    device tensor is read where it lies on the library's current stream and a float32 (n, 8) device tensor of the raw
    records comes back without synchronising (floats 1-3 hold the int32 bits of tri, obj, inside)."""
    import torch

    t, host = _device_rays(rays)
    n = t.shape[0]
    out = torch.empty((n, 8), dtype=torch.float32, device=t.device)
    check(pt().pt_rays_closest(tri_tex, node_tex, C.c_void_p(t.data_ptr() if n else None), n,
                               C.c_void_p(out.data_ptr() if n else None)))
    if not host:
        return out
    if n:
        sync()
    return out.cpu().numpy().view(HIT_DTYPE).reshape(n)


def rays_occluded(tri_tex: int, node_tex: int, rays):
    """pt_rays_occluded: per ray, whether its closest hit exists and lies at t < tmax (float 7; +inf: any hit). numpy
    in, bool array out (synchronises); torch device tensor in, uint8 device tensor out (no synchronisation)."""
    import torch

    t, host = _device_rays(rays)
    n = t.shape[0]
    out = torch.empty((n,), dtype=torch.uint8, device=t.device)
    check(pt().pt_rays_occluded(tri_tex, node_tex, C.c_void_p(t.data_ptr() if n else None), n,
                                C.c_void_p(out.data_ptr() if n else None)))
    if not host:
        return out
    if n:
        sync()
    return out.cpu().numpy().astype(bool)


def rays_primary(eye, cameraRotate, width: int, height: int, aspect_corrected: bool, xy=None):
    """pt_rays_primary: the path-tracing pass's primary rays as ray records. xy None: every pixel, row-major, row 0 at
    the bottom; a numpy (n, 2) int array of (x, y): those pixels (one outside the frame raises PtError PT_ERR_ARG),
    numpy (n, 8) float32 back after a synchronisation; a torch int32 (n, 2) device tensor: read where it lies on the
    library's current stream (a pixel outside the frame yields the direction 0, a ray that misses), a device tensor
    back without synchronising."""
    import torch

    from ._lib import PtError

    e = np.ascontiguousarray(eye, dtype=np.float32).reshape(3)
    m = np.ascontiguousarray(cameraRotate, dtype=np.float32).reshape(16)
    host = not _is_tensor(xy)
    if xy is None:
        n, dxy = int(width) * int(height), None
    elif host:
        a = np.ascontiguousarray(xy, dtype=np.int32).reshape(-1, 2)
        if a.size and (a.min() < 0 or (a[:, 0] >= width).any() or (a[:, 1] >= height).any()):
            raise PtError(-6, "rays_primary: a pixel outside the frame")
        n, dxy = a.shape[0], torch.from_numpy(a).cuda()
        torch.cuda.current_stream().synchronize()
    else:
        if not xy.is_cuda or xy.dtype != torch.int32 or xy.dim() != 2 or xy.shape[1] != 2 or not xy.is_contiguous():
            raise ValueError("xy: a contiguous int32 (n, 2) device tensor")
        n, dxy = xy.shape[0], xy
    out = torch.empty((n, 8), dtype=torch.float32, device="cuda")
    check(pt().pt_rays_primary(fptr(e), fptr(m), int(width), int(height), 1 if aspect_corrected else 0,
                               C.c_void_p(dxy.data_ptr() if dxy is not None and n else None), n,
                               C.c_void_p(out.data_ptr() if n else None)))
    if not host:
        return out
    if n:
        sync()
    return out.cpu().numpy()


def rays_variant(variant: int) -> None:
    """pt_debug_rays_variant (include/ptsvgf_debug_rays.h): 0 one ray per lane, 1 lane refill, -1 the default."""
    check(pt().pt_debug_rays_variant(int(variant)))


def rays_state() -> dict:
    """pt_debug_rays_state: {"stack_kind" (0 small, 1 full, 2 deep), "variant"} of the last query that launched,
    {"scratch_allocs", "scratch_bytes"} of the deep trees' spill scratch."""
    k, v, a, b = C.c_int(), C.c_int(), C.c_uint64(), C.c_size_t()
    check(pt().pt_debug_rays_state(C.byref(k), C.byref(v), C.byref(a), C.byref(b)))
    return {"stack_kind": k.value, "variant": v.value, "scratch_allocs": a.value, "scratch_bytes": b.value}


def materials_state(tri_tex: int, node_tex: int) -> dict:
    """pt_debug_materials_state (include/ptsvgf_debug_materials.h) of the scene decoded from the two buffers:
    {"shade_version", "device_versions", "staging_slots"}."""
    ver, n, m = C.c_uint64(), C.c_int(), C.c_int()
    check(pt().pt_debug_materials_state(tri_tex, node_tex, C.byref(ver), C.byref(n), C.byref(m)))
    return {"shade_version": ver.value, "device_versions": n.value, "staging_slots": m.value}


def lights_state(tex: int, nl: int = 4) -> dict:
    """pt_debug_lights_state (include/ptsvgf_debug_lights.h): {"version", "pos_stamps" (per light: the version at which
    its position last changed, 0 never), "device_versions" (device buffers the texture owns)}."""
    ver, n = C.c_uint64(), C.c_int()
    st = (C.c_uint64 * max(nl, 1))()
    check(pt().pt_debug_lights_state(tex, C.byref(ver), st, int(nl), C.byref(n)))
    return {"version": ver.value, "pos_stamps": [int(v) for v in st][:nl], "device_versions": n.value}


def lights_moved_mask(pos_stamps, since: int) -> int:
    """pt_debug_lights_moved_mask: bit l for every light whose position stamp is newer than `since`. Host only."""
    a, pa = _key_ptr(pos_stamps)
    m = C.c_uint32()
    check(pt().pt_debug_lights_moved_mask(pa, int(a.size), int(since), C.byref(m)))
    return m.value


def lights_settle(stamps, settle: int) -> list:
    """pt_debug_lights_settle: what consecutive draws do with one light's bins (built at stamp 0) as they meet
    `stamps`: 0 keep, 1 mark moved, 2 still marked, 3 rebuild. Host only."""
    a, pa = _key_ptr(stamps)
    out = (C.c_int * max(int(a.size), 1))()
    check(pt().pt_debug_lights_settle(pa, int(a.size), int(settle), out))
    return [int(v) for v in out][:a.size]


def lights_key_mode(last, last_valid: bool, now, stage_reused: bool, enabled: bool) -> tuple:
    """pt_debug_lights_key_mode: (mode 0 off / 1 reset / 2 use, forgets) of a draw with verdict-cache key `now` after
    the draw that left `last`, with the moved-lights rule. Host only."""
    last, pl = _key_ptr(last)
    now, pn = _key_ptr(now)
    mode, forget = C.c_int(), C.c_int()
    check(pt().pt_debug_lights_key_mode(pl, 1 if last_valid else 0, pn, int(min(last.size, now.size)),
                                        1 if stage_reused else 0, 1 if enabled else 0, C.byref(mode), C.byref(forget)))
    return mode.value, bool(forget.value)


def lights_key_field(which: int) -> int:
    """pt_debug_lights_key_field: the key word of 0 the lights handle, 1 their device pointer, 2 their version, 3
    point_bins, 4 the bins' device pointer."""
    return check(pt().pt_debug_lights_key_field(int(which)))


def point_bins_read(tri_tex: int, node_tex: int, light: int):
    """pt_debug_point_bins_read: (hdr (6 R R + 1, 2) int32, ent (entries, 2) uint32) of one light's lists as they lie
    on the device; (hdr, None) for a light without usable lists."""
    R = point_bins_info(tri_tex, node_tex)["R"]
    n1 = 6 * R * R + 1
    hdr = np.zeros((n1, 2), np.int32)
    n = C.c_int()
    check(pt().pt_debug_point_bins_read(tri_tex, node_tex, int(light), hdr.ctypes.data_as(C.POINTER(C.c_int32)),
                                        hdr.size, None, 0, C.byref(n)))
    if n.value < 0:
        return hdr, None
    ent = np.zeros((n.value, 2), np.uint32)
    check(pt().pt_debug_point_bins_read(tri_tex, node_tex, int(light), None, 0,
                                        ent.ctypes.data_as(C.POINTER(C.c_uint32)), ent.size, C.byref(n)))
    return hdr, ent


def buffer_readback(tex: int) -> np.ndarray:
    """Device contents of a texture buffer as flat float32 (3 floats per RGB32F texel)."""
    w, _, _ = texture_info(tex)
    out = np.empty(w * 3, np.float32)
    check(pt().pt_texture_readback(tex, fptr(out), out.nbytes))
    return out


def bvh_build(tri_in: int, tri_out: int, node_out: int, leaf_n: int = 8, ploc_radius: int = 0):
    """pt_bvh_build: GPU LBVH over the device triangles of tri_in (Triangle_encoded texels) into tri_out (leaf
    order) and node_out (BVHNode_encoded, dummy node 0, root 1) — the reference's buffer formats (main.cpp:88-151);
    ploc_radius > 0 rebuilds the tree above the LBVH leaves by PLOC. Returns (node count, device build ms)."""
    n, ms = C.c_int(), C.c_float()
    check(pt().pt_bvh_build(tri_in, leaf_n, ploc_radius, tri_out, node_out, C.byref(n), C.byref(ms)))
    return n.value, ms.value


def bvh_refit(tri_in: int, tri_out: int, node_out: int) -> float:
    """pt_bvh_refit: the triangles of tri_in (those of the bvh_build that wrote tri_out / node_out, in its input order,
    at new positions) permuted into tri_out, and node_out's boxes recomputed over the unchanged topology; the walk
    trees are derived again. Returns the device ms, that derivation included."""
    ms = C.c_float()
    check(pt().pt_bvh_refit(tri_in, tri_out, node_out, C.byref(ms)))
    return ms.value


def lbvh_order(node_tex: int) -> np.ndarray:
    """pt_debug_lbvh_order (include/ptsvgf_debug_refit.h): the leaf order of the bvh_build that wrote node_tex, order[p] =
    the index in its tri_in of the triangle at position p of its tri_out."""
    n = C.c_size_t()
    check(pt().pt_debug_lbvh_order(node_tex, None, 0, C.byref(n)))
    out = np.zeros(n.value, np.int32)
    if n.value:
        check(pt().pt_debug_lbvh_order(node_tex, out.ctypes.data_as(C.POINTER(C.c_int)), n.value, C.byref(n)))
    return out


def pose_create(tri_rest: int, raster_rest=None, raster_obj=None) -> int:
    """pt_pose_create: a pose over the device triangles of the texbuffer tri_rest (the rows a bvh_build received, in
    its input order; it may be destroyed afterwards) and, optionally, the rest raster vertex list with one object
    index per raster triangle. Returns the pose handle."""
    h = C.c_uint32()
    if raster_rest is None:
        check(pt().pt_pose_create(tri_rest, None, 0, None, C.byref(h)))
        return h.value
    v = np.ascontiguousarray(raster_rest, np.float32).reshape(-1)
    o = np.ascontiguousarray(raster_obj, np.int32).reshape(-1)
    if o.size * 18 != v.size:
        raise ValueError(f"pose_create: {o.size} raster objects for {v.size / 18:g} raster triangles")
    check(pt().pt_pose_create(tri_rest, fptr(v), v.size, o.ctypes.data_as(C.POINTER(C.c_int)), C.byref(h)))
    return h.value


def pose_apply(pose: int, mats, tri_out: int, node_out: int, raster_pass: int = 0, motion: bool = True) -> float:
    """pt_pose_apply: the rest lists of `pose` placed by mats ((n_obj, 16), glm column-major, absolute), tri_out /
    node_out refitted as bvh_refit would with the posed triangles, the rasterize pass (handle, 0: none) refitted with
    the posed raster list and, with motion, given displacement records from the previous pose. Returns device ms."""
    m = np.ascontiguousarray(mats, np.float32).reshape(-1, 16)
    ms = C.c_float()
    check(pt().pt_pose_apply(pose, fptr(m), m.shape[0], tri_out, node_out, raster_pass, 1 if motion else 0,
                             C.byref(ms)))
    return ms.value


def pose_set_skin(pose: int, tri_bones, tri_weights, raster_bones=None, raster_weights=None) -> None:
    """pt_pose_set_skin: four bone indices (uint16) and four weights (float32) per corner, 12 entries per record of
    the pose's triangle list and, for a pose with a raster list, 12 per raster triangle. A second call replaces the
    skin."""
    def pair(bones, weights, what):
        if bones is None and weights is None:
            return None, None, None, None
        if bones is None or weights is None:
            raise ValueError(f"pose_set_skin: {what} bones and weights go together")
        b = np.asarray(bones)
        if b.size and (b.min() < 0 or b.max() > 0xFFFF):
            raise ValueError(f"pose_set_skin: {what} bone index outside uint16")
        b = np.ascontiguousarray(b, np.uint16).reshape(-1)
        w = np.ascontiguousarray(weights, np.float32).reshape(-1)
        if b.size != w.size or b.size % 12:
            raise ValueError(f"pose_set_skin: {b.size} {what} bones for {w.size} weights (12 per triangle each)")
        return b, w, b.ctypes.data_as(C.POINTER(C.c_uint16)), fptr(w)

    tb, tw, tbp, twp = pair(tri_bones, tri_weights, "triangle")
    rb, rw, rbp, rwp = pair(raster_bones, raster_weights, "raster")
    n = C.c_size_t()
    check(pt().pt_debug_pose_raster(pose, 0, None, 0, C.byref(n)))  # also: the pose exists
    if rb is not None and rb.size * 18 != n.value * 12:
        raise ValueError(f"pose_set_skin: {rb.size // 12} raster triangles of influences for {n.value // 18}")
    check(pt().pt_pose_set_skin(pose, tbp, twp, rbp, rwp))


def pose_apply_skin(pose: int, bones, tri_out: int, node_out: int, raster_pass: int = 0, motion: bool = True) -> float:
    """pt_pose_apply_skin: pose_apply with the pose's skin blended from bones ((n_bones, 16), glm column-major,
    absolute) in place of one matrix per object. Returns device ms."""
    m = np.ascontiguousarray(bones, np.float32).reshape(-1, 16)
    ms = C.c_float()
    check(pt().pt_pose_apply_skin(pose, fptr(m), m.shape[0], tri_out, node_out, raster_pass, 1 if motion else 0,
                                  C.byref(ms)))
    return ms.value


def pose_destroy(pose: int) -> None:
    check(pt().pt_pose_destroy(pose))


def pose_raster(pose: int, which: int = 0) -> np.ndarray:
    """pt_debug_pose_raster (include/ptsvgf_debug_pose.h): the pose's current (which = 0) or previous (1) posed
    raster vertex list as flat float32."""
    n = C.c_size_t()
    check(pt().pt_debug_pose_raster(pose, which, None, 0, C.byref(n)))
    out = np.zeros(n.value, np.float32)
    if n.value:
        check(pt().pt_debug_pose_raster(pose, which, fptr(out), out.size, C.byref(n)))
    return out


LBVH_INFO_KEYS = ("root_ref", "need", "nleaves", "root4", "need4", "wide_nodes", "nan", "stage_us")


def lbvh_trees(tex: int, source: int = 0) -> dict:
    """pt_debug_lbvh_trees (include/ptsvgf_debug.h): the walk trees of a node buffer bvh_build wrote — source 0 the
    buffers the device stage derived, 1 the host functions that define them run on the host mirror of the texels.
    Returns {"binary": (k, 16), "leaves": (k, 8), "wide": (k, 28) float32 arrays, "info": the 8 ints} plus the ints
    by name (LBVH_INFO_KEYS)."""
    out = {}
    info = (C.c_int * 8)()
    for which, (name, width) in enumerate((("binary", 16), ("leaves", 8), ("wide", 28))):
        nbytes = C.c_size_t()
        check(pt().pt_debug_lbvh_trees(tex, source, which, None, 0, C.byref(nbytes), info))
        a = np.zeros(nbytes.value // 4, np.float32)
        if a.size:
            check(pt().pt_debug_lbvh_trees(tex, source, which, a.ctypes.data_as(C.c_void_p), a.nbytes,
                                           C.byref(nbytes), info))
        out[name] = a.reshape(-1, width)
    out["info"] = [int(v) for v in info]
    out.update(zip(LBVH_INFO_KEYS, out["info"]))
    return out


def point_bins_info(tri_tex: int, node_tex: int) -> dict:
    """pt_point_bins_info: the point-light triangle bins the last path-tracing draw of the scene (tri_tex, node_tex)
    built: cells per face edge R, lights, entry capacity per light, bytes per entry, allocated bytes, and per light
    {"off": no usable bins (2: the light moved, its bins are pending), "entries", "list_bytes" (entries x
    entry_bytes), "catch_all", "pos", "magnitude", "large": (triangle, face) boxes its last build binned a wave each}."""
    info = (C.c_int * 32)()
    dims = (C.c_int * 4)()
    nbytes = C.c_size_t()
    check(pt().pt_point_bins_info(tri_tex, node_tex, info, dims, C.byref(nbytes)))
    raw = np.array(list(info), np.int32).reshape(4, 8)
    lights = [{"off": int(r[0]), "entries": int(r[1]), "list_bytes": int(r[1]) * dims[3], "catch_all": int(r[6]),
               "pos": r[2:5].view(np.float32).tolist(), "magnitude": float(r[5:6].view(np.float32)[0]),
               "large": int(r[7])}
              for r in raw[:dims[1]]]
    return {"R": dims[0], "lights": dims[1], "cap": dims[2], "entry_bytes": dims[3], "bytes": nbytes.value,
            "per_light": lights}


def point_bins_overlap(px, py, fw: float, R: int, box) -> tuple:
    """pt_debug_point_bins_overlap: which cells of box = (cx0, cy0, cx1, cy1) of an R x R face list a triangle whose
    projected polygon has the cell coordinates (px, py), widened by fw: (kept[cy - cy0, cx - cx0] bool array,
    degenerate). Runs on the host."""
    px = np.ascontiguousarray(px, np.float32)
    py = np.ascontiguousarray(py, np.float32)
    cx0, cy0, cx1, cy1 = (int(v) for v in box)
    kept = np.zeros((cy1 - cy0 + 1, cx1 - cx0 + 1), np.uint8)
    deg = C.c_int()
    fp = C.POINTER(C.c_float)
    check(pt().pt_debug_point_bins_overlap(px.ctypes.data_as(fp), py.ctypes.data_as(fp), len(px), float(fw), int(R),
                                           cx0, cy0, cx1, cy1, kept.ctypes.data_as(C.POINTER(C.c_uint8)), kept.size,
                                           C.byref(deg)))
    return kept.astype(bool), bool(deg.value)


def static_key_words(kind: int) -> int:
    """pt_debug_static_key_words: 64-bit words of a static-view key (kind 0: the primary stage's, 1: the G-buffer
    draw's; csrc/static_key.h)."""
    return check(pt().pt_debug_static_key_words(int(kind)))


def _key_ptr(a):
    a = np.ascontiguousarray(a, np.uint64)
    return a, a.ctypes.data_as(C.POINTER(C.c_uint64))


def static_key_diff(kind: int, a, b) -> int:
    """pt_debug_static_key_diff: the first word in which two keys differ, -1 when they are equal. Runs on the host."""
    a, pa = _key_ptr(a)
    b, pb = _key_ptr(b)
    field = C.c_int()
    check(pt().pt_debug_static_key_diff(int(kind), pa, pb, int(min(a.size, b.size)), C.byref(field)))
    return field.value


def static_key_hit(kind: int, last, last_valid: bool, now, enabled: bool) -> bool:
    """pt_debug_static_key_hit: may a draw with key `now` reuse the work of the draw that left `last`?"""
    last, pl = _key_ptr(last)
    now, pn = _key_ptr(now)
    hit = C.c_int()
    check(pt().pt_debug_static_key_hit(int(kind), pl, 1 if last_valid else 0, pn, int(min(last.size, now.size)),
                                       1 if enabled else 0, C.byref(hit)))
    return bool(hit.value)


def point_cache_word(op: int, word: int, arg: int = 0) -> int:
    """pt_debug_point_cache_word: the verdict word's bit operations (csrc/point_cache.h) on the host. op 0: look-up of
    light `arg` (-1 not known, 0 lit, 1 occluded); 1: the pending light (-1 none); 2: mark light `arg` pending;
    3: resolve the pending light with verdict `arg`; 5: forget the lights of the bit mask `arg` (4 is no op)."""
    out = C.c_uint32()
    check(pt().pt_debug_point_cache_word(int(op), int(word), int(arg), C.byref(out)))
    return C.c_int32(out.value).value if op in (0, 1) else out.value


def point_cache_key_words() -> int:
    """pt_debug_point_cache_key_words: 64-bit words of the verdict cache's key (csrc/static_key.h LightsKey)."""
    return check(pt().pt_debug_point_cache_key_words())


def point_cache_key_diff(a, b) -> int:
    """pt_debug_point_cache_key_diff: the first word in which two keys differ, -1 when they are equal."""
    a, pa = _key_ptr(a)
    b, pb = _key_ptr(b)
    field = C.c_int()
    check(pt().pt_debug_point_cache_key_diff(pa, pb, int(min(a.size, b.size)), C.byref(field)))
    return field.value


def point_cache_key_mode(last, last_valid: bool, now, stage_reused: bool, enabled: bool) -> int:
    """pt_debug_point_cache_key_mode: the mode (0 off, 1 reset, 2 use) of a draw with key `now` after the draw that
    left `last`."""
    last, pl = _key_ptr(last)
    now, pn = _key_ptr(now)
    mode = C.c_int()
    check(pt().pt_debug_point_cache_key_mode(pl, 1 if last_valid else 0, pn, int(min(last.size, now.size)),
                                             1 if stage_reused else 0, 1 if enabled else 0, C.byref(mode)))
    return mode.value


class PtTileSeg(C.Structure):
    _fields_ = [("y_begin", C.c_int), ("y_end", C.c_int), ("offset", C.c_int), ("packed", C.c_void_p)]


def tiles_count(frame_w: int, stride: int, offset: int, y0: int, y1: int, tile_y0: int = 0) -> int:
    """Pixels per texture of the tile subset k * stride + offset in rows [y0, y1) (pt_tiles_count)."""
    n = C.c_int64()
    check(pt().pt_tiles_count(frame_w, tile_y0, stride, offset, y0, y1, C.byref(n)))
    return n.value


def tiles_copy(textures, stride: int, segs, unpack: bool, tile_y0: int = 0) -> None:
    """pt_tiles_copy: segs = [(y0, y1, offset, packed device pointer)]; one launch on the library stream."""
    tex = (C.c_uint32 * len(textures))(*textures)
    arr = (PtTileSeg * max(1, len(segs)))(*[PtTileSeg(a, b, o, C.c_void_p(p)) for a, b, o, p in segs])
    check(pt().pt_tiles_copy(tex, len(textures), tile_y0, stride, C.cast(arr, C.c_void_p), len(segs), int(bool(unpack))))


def texture_array(layers: np.ndarray) -> int:
    """main.cpp:184-205: glTexStorage3D(GL_TEXTURE_2D_ARRAY, 1, GL_RGBA8, w, h, n) + one glTexSubImage3D per layer
    (help_func.h:4-20). `layers` is (n, h, w, 3|4) uint8, rows already in GL order (stbi flipped on load)."""
    a = np.ascontiguousarray(layers, dtype=np.uint8)
    n, hh, ww, ch = a.shape
    h = C.c_uint32()
    check(pt().pt_texarray_create(ww, hh, n, C.byref(h)))
    for i in range(n):
        check(pt().pt_texarray_upload_layer(h.value, i, ww, hh, ch, a[i].ctypes.data_as(C.POINTER(C.c_uint8))))
    return h.value


def texture_info(tex: int):
    w, h, r0 = C.c_int(), C.c_int(), C.c_int()
    check(pt().pt_texture_info(tex, C.byref(w), C.byref(h), C.byref(r0)))
    return w.value, h.value, r0.value


def draw_batch(passes) -> None:
    """pt_pass_draw_batch: the frames of up to 8 path-tracing passes in one run, their traversals batched."""
    hs = (C.c_uint32 * len(passes))(*[p._handle() for p in passes])
    check(pt().pt_pass_draw_batch(hs, len(passes)))


def sample_counts_derive(stats_ptr: int, motion_tex: int, nd_tex: int, lag: float, tolerance: float, nmax: int,
                         out_ptr: int) -> None:
    """pt_sample_counts_derive: the next draw's per-pixel sample counts (W * H uint8 at out_ptr) from a draw's
    statistics plane (W * H float32 pairs at stats_ptr), followed along this frame's motion vectors, on the
    library's current stream."""
    check(pt().pt_sample_counts_derive(C.c_void_p(stats_ptr or None), motion_tex, nd_tex, float(np.float32(lag)),
                                       float(np.float32(tolerance)), int(nmax), C.c_void_p(out_ptr or None)))


def sample_counts_pool(stats_ptr: int, counts_prev_ptr: int, nmax_prev: int, pool_in_ptr: int, motion_tex: int,
                       nd_tex: int, lag: float, wmax: float, zeta: float, rule: int, tolerance: float, nmax: int,
                       pool_out_ptr: int, out_ptr: int) -> None:
    """pt_sample_counts_pool: the next draw's per-pixel sample counts (W * H uint8 at out_ptr) and the pool plane
    (W * H float4 (m, v, w, z) at pool_out_ptr) from the previous draw's statistics, the counts it read and the pool
    plane of its step (each pointer may be 0), followed along this frame's motion vectors, on the library's current
    stream. rule: 0 relative, 1 absolute."""
    f = lambda v: float(np.float32(v))  # noqa: E731
    check(pt().pt_sample_counts_pool(C.c_void_p(stats_ptr or None), C.c_void_p(counts_prev_ptr or None),
                                     int(nmax_prev), C.c_void_p(pool_in_ptr or None), motion_tex, nd_tex, f(lag),
                                     f(wmax), f(zeta), int(rule), f(tolerance), int(nmax),
                                     C.c_void_p(pool_out_ptr or None), C.c_void_p(out_ptr or None)))


def readback(tex: int) -> np.ndarray:
    """Stored rows of an RGBA32F texture as (rows, W, 4) float32."""
    w, rows, _ = texture_info(tex)
    out = np.empty((rows, w, 4), np.float32)
    check(pt().pt_texture_readback(tex, fptr(out), out.nbytes))
    return out


def readback_aux(tex: int):
    """pt_texture_readback_aux: the compact one-float side plane of a texture's stored rows as
    (rows, W) float32, or None when the texture holds none that matches its texels."""
    w, rows, _ = texture_info(tex)
    n = C.c_size_t()
    check(pt().pt_texture_readback_aux(tex, None, 0, C.byref(n)))
    if not n.value:
        return None
    out = np.empty((rows, w), np.float32)
    check(pt().pt_texture_readback_aux(tex, fptr(out), out.nbytes, C.byref(n)))
    return out


def upload_rgba(tex: int, data: np.ndarray) -> None:
    a = np.ascontiguousarray(data, dtype=np.float32)
    check(pt().pt_texture_upload_rgba(tex, fptr(a), a.nbytes))


def device_ptr(tex: int) -> int:
    p = C.c_void_p()
    check(pt().pt_texture_device_ptr(tex, C.byref(p)))
    return p.value or 0


def background_stamp(tex: int):
    """pt_debug_bg_stamp: (content id, scope) of a texture's background stamp (DESIGN.md "Static view, part 3")."""
    i, sc = C.c_uint64(), C.c_uint64()
    check(pt().pt_debug_bg_stamp(tex, C.byref(i), C.byref(sc)))
    return i.value, sc.value


def destroy_texture(tex: int) -> None:
    check(pt().pt_texture_destroy(tex))


class RenderPass:
    """Utils/render_pass.h:82-182 — a full-screen pass drawing into MRT attachments."""

    def __init__(self, program: int = 0, width: int = SCR_WIDTH, height: int = SCR_HEIGHT):
        self.program = program
        self.colorAttachments: list[int] = []
        self.width = width
        self.height = height
        self.texture_slot = 0
        self._h = None

    def _handle(self) -> int:
        if self._h is None:
            h = C.c_uint32()
            check(pt().pt_pass_create(self.program, self.width, self.height, C.byref(h)))
            self._h = h.value
        return self._h

    def bindData(self, finalPass: bool = False) -> None:
        h = self._handle()
        for t in self.colorAttachments:
            check(pt().pt_pass_add_color_attachment(h, t))
        check(pt().pt_pass_bind(h, 1 if finalPass else 0))

    def draw(self, texPassArray=()) -> None:
        h = self._handle()
        for i, t in enumerate(texPassArray):
            check(pt().pt_pass_set_texture(h, GL_TEXTURE_2D, t, f"texPass{i}".encode()))
        check(pt().pt_pass_draw(h))

    def reset_texture_slot(self) -> None:
        self.texture_slot = 0
        check(pt().pt_pass_reset_texture_slot(self._handle()))

    def set_texture_uniform(self, target: int, texture: int, uniform_name: str) -> None:
        check(pt().pt_pass_set_texture(self._handle(), target, texture, uniform_name.encode()))
        self.texture_slot += 1

    def set_uniform_mat4(self, name: str, value) -> None:
        m = np.ascontiguousarray(value, dtype=np.float32).reshape(16)
        check(pt().pt_pass_set_uniform_mat4(self._handle(), name.encode(), fptr(m)))

    def set_uniform_float(self, name: str, value: float) -> None:
        check(pt().pt_pass_set_uniform_float(self._handle(), name.encode(), float(np.float32(value))))

    def set_uniform_int(self, name: str, value: int) -> None:
        check(pt().pt_pass_set_uniform_int(self._handle(), name.encode(), int(value)))

    def set_uniform_uint(self, name: str, value: int) -> None:
        check(pt().pt_pass_set_uniform_uint(self._handle(), name.encode(), int(value) & 0xFFFFFFFF))

    def set_uniform_bool(self, name: str, value: bool) -> None:
        check(pt().pt_pass_set_uniform_bool(self._handle(), name.encode(), 1 if value else 0))

    def set_uniform_vec3(self, name: str, value) -> None:
        v = np.ascontiguousarray(value, dtype=np.float32).reshape(3)
        check(pt().pt_pass_set_uniform_vec3(self._handle(), name.encode(), fptr(v)))

    # MI355X extensions
    def set_rows(self, y0: int, y1: int) -> None:
        check(pt().pt_pass_set_rows(self._handle(), y0, y1))

    def set_row_cost(self, device_ptr: int) -> None:
        """Accumulate per-row BVH visits into a device uint32 array (path tracer; 0 disables)."""
        check(pt().pt_pass_set_row_cost(self._handle(), C.c_void_p(device_ptr or None)))

    def set_trace_stats(self, device_ptr: int, count: int = 14) -> None:
        """Path-tracing pass: add traversal counters (`count` x uint64, pt_pass_set_trace_stats_n; the library writes
        pt_trace_stats_count() = 14, and none past `count`) on every draw (0 disables)."""
        check(pt().pt_pass_set_trace_stats_n(self._handle(), C.c_void_p(device_ptr or None), count))

    def set_spp(self, n: int) -> None:
        """Path-tracing pass: samples per pixel of every draw (int uniform spp, 1 .. 8; the draw refuses others)."""
        self.set_uniform_int("spp", n)

    def set_sample_counts(self, device_ptr: int) -> None:
        """Path-tracing pass, spp = N > 1: per-pixel sample counts (W * H uint8 on the device, global rows; a pixel
        takes min(max(c, 1), N) samples; 0 unbinds)."""
        check(pt().pt_pass_set_sample_counts(self._handle(), C.c_void_p(device_ptr or None)))

    def set_sample_stats(self, device_ptr: int) -> None:
        """Path-tracing pass, spp > 1: the resolve writes (mean, variance) of each pixel's sample luminances into
        W * H float32 pairs on the device (0 unbinds)."""
        check(pt().pt_pass_set_sample_stats(self._handle(), C.c_void_p(device_ptr or None)))

    def set_sample_moments(self, device_ptr: int) -> None:
        """Path-tracing pass, spp > 1: the resolve writes (mu, nu, r, n) of each pixel's demodulated sample
        luminances into W * H float32 quadruples on the device (0 unbinds): device_ptr() of the RGBA32F
        texture the reproject and variance passes bind as "gSampleMoments"."""
        check(pt().pt_pass_set_sample_moments(self._handle(), C.c_void_p(device_ptr or None)))

    def set_motion_bound(self, device_ptr: int) -> None:
        """G-buffer pass: store the largest |motion.y| of every draw into a device uint32 (float bits; 0 disables)."""
        check(pt().pt_pass_set_motion_bound(self._handle(), C.c_void_p(device_ptr or None)))

    def stage_counts(self):
        """pt_debug_stage_counts (DESIGN.md "Static view"): (runs, reuses) of this pass's draws. A path-tracing pass:
        the draws that ran the primary stage / that read the cached primary hit; a rasterize pass: the G-buffer draws
        that launched / that were elided (int uniform reuse_static)."""
        runs, reuses = C.c_uint64(), C.c_uint64()
        check(pt().pt_debug_stage_counts(self._handle(), C.byref(runs), C.byref(reuses)))
        return runs.value, reuses.value

    def background_counts(self):
        """pt_debug_bg_counts (DESIGN.md "Static view, part 3"): (mode, reason, skipped, total) of this SVGF pass's last
        draw: mode 0 off / 1 armed / 2 skip, the reason of a bypass (include/ptsvgf_debug_background.h), the tiles the
        draw skipped and those it has. Synchronises the device when the draw skipped."""
        mode, reason, skipped, total = C.c_int(), C.c_int(), C.c_uint64(), C.c_uint64()
        check(pt().pt_debug_bg_counts(self._handle(), C.byref(mode), C.byref(reason), C.byref(skipped), C.byref(total)))
        return mode.value, reason.value, skipped.value, total.value

    def first_hit_last(self):
        """pt_debug_firsthit_last (DESIGN.md "Static view, part 4"): (mode, reason, kept) of this path-tracing pass:
        its last draw's mode 0 off / 1 full / 2 keep and reason (include/ptsvgf_debug_firsthit.h), its kept draws."""
        mode, reason, kept = C.c_int(), C.c_int(), C.c_uint64()
        check(pt().pt_debug_firsthit_last(self._handle(), C.byref(mode), C.byref(reason), C.byref(kept)))
        return mode.value, reason.value, kept.value

    def first_hit_busy(self):
        """pt_debug_firsthit_busy: (busy, tiles) of this path-tracing pass's busy-tile list, busy -1 when none stands.
        Synchronises the device."""
        busy, tiles = C.c_int(), C.c_int()
        check(pt().pt_debug_firsthit_busy(self._handle(), C.byref(busy), C.byref(tiles)))
        return busy.value, tiles.value

    def poke_primary_hit(self, x: int, y: int, tri: int, t: float) -> None:
        """pt_debug_bg_poke_hit0: make pixel (x, y) of this path-tracing pass's primary plane a hit of triangle tri."""
        check(pt().pt_debug_bg_poke_hit0(self._handle(), x, y, tri, t))

    def point_cache_counts(self):
        """pt_debug_point_cache_counts (DESIGN.md "Static view, part 2"): (served, queued), the bounce-0 point-light
        verdicts of this path-tracing pass's last draw that came from the cache / that were queued as rays.
        Synchronises the device."""
        served, queued = C.c_uint64(), C.c_uint64()
        check(pt().pt_debug_point_cache_counts(self._handle(), C.byref(served), C.byref(queued)))
        return served.value, queued.value

    def point_cache_mode(self):
        """pt_debug_point_cache_mode: (mode of the last draw: 0 off, 1 reset, 2 use; plane valid)."""
        mode, valid = C.c_int(), C.c_int()
        check(pt().pt_debug_point_cache_mode(self._handle(), C.byref(mode), C.byref(valid)))
        return mode.value, bool(valid.value)

    def point_cache_forgotten(self) -> int:
        """pt_debug_point_cache_forgotten: the lights (bit i: light i) the verdict cache forgot at the top of the
        pass's last draw; 0: none."""
        m = C.c_uint32()
        check(pt().pt_debug_point_cache_forgotten(self._handle(), C.byref(m)))
        return m.value

    def point_cache_read(self, n: int):
        """pt_debug_point_cache_read: the verdict plane, one uint16 per pixel of the rows last drawn (n of them)."""
        a = np.empty(int(n), np.uint16)
        check(pt().pt_debug_point_cache_read(self._handle(), a.ctypes.data_as(C.POINTER(C.c_uint16)), a.size))
        return a

    def point_cache_write(self, words) -> None:
        """pt_debug_point_cache_write: replaces the verdict plane (tests of the cache's effect)."""
        a = np.ascontiguousarray(words, np.uint16)
        check(pt().pt_debug_point_cache_write(self._handle(), a.ctypes.data_as(C.POINTER(C.c_uint16)), a.size))

    def destroy(self) -> None:
        if self._h is not None:
            check(pt().pt_pass_destroy(self._h))
            self._h = None

    def last_ms(self) -> float:
        v = C.c_float()
        check(pt().pt_pass_last_ms(self._handle(), C.byref(v)))
        return v.value


class Rasterize_RenderPass(RenderPass):
    """Utils/render_pass.h:5-80 — the G-buffer pass over the model's vertex list."""

    def bindData(self, vertices) -> None:  # type: ignore[override]
        h = self._handle()
        for t in self.colorAttachments:
            check(pt().pt_pass_add_color_attachment(h, t))
        v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1)
        check(pt().pt_raster_pass_bind(h, fptr(v), v.size))

    def rebind_vertices(self, vertices) -> None:
        """A new vertex list for the bound pass (moved geometry): pt_raster_pass_bind again, attachments kept."""
        v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1)
        check(pt().pt_raster_pass_bind(self._handle(), fptr(v), v.size))

    def rebind_vertices_device(self, device_ptr: int, n_floats: int, ploc_radius: int = 16) -> None:
        """pt_raster_pass_bind_device: the vertex list already in device memory, its tree built on the GPU."""
        check(pt().pt_raster_pass_bind_device(self._handle(), C.c_void_p(device_ptr), n_floats, ploc_radius))

    def refit_vertices_device(self, device_ptr: int, n_floats: int) -> None:
        """pt_raster_pass_refit_device: the same triangles in the same order at new positions (a device vertex list)
        for a pass rebind_vertices_device bound: records decoded again, the tree's boxes recomputed, topology kept."""
        check(pt().pt_raster_pass_refit_device(self._handle(), C.c_void_p(device_ptr), n_floats))

    def adopt(self, y0: int, y1: int) -> None:
        """pt_raster_pass_adopt: the attachments' rows [y0, y1) were written elsewhere (another rank's draw of the same
        frame); derive the a-trous side data a draw makes, on the current library stream."""
        check(pt().pt_raster_pass_adopt(self._handle(), y0, y1))

    def set_prev_vertices(self, prev_ptr, cur_ptr, n_floats: int) -> None:
        """pt_raster_pass_set_prev_vertices: the device vertex list the bound triangles had one frame ago (and the
        one bound now), for object motion vectors; prev_ptr None (or 0) drops the records."""
        check(pt().pt_raster_pass_set_prev_vertices(self._handle(), C.c_void_p(prev_ptr or None),
                                                    C.c_void_p(cur_ptr or None), n_floats))

    def bind_shared(self, src: "Rasterize_RenderPass") -> None:
        """bindData for a pass that draws src's triangles: the attachments, then share_vertices."""
        h = self._handle()
        for t in self.colorAttachments:
            check(pt().pt_pass_add_color_attachment(h, t))
        self.share_vertices(src)

    def share_vertices(self, src: "Rasterize_RenderPass") -> None:
        """pt_raster_pass_share: draw src's triangles and tree (src bound on its own)."""
        check(pt().pt_raster_pass_share(self._handle(), src._handle()))
