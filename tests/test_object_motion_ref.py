"""The float64 restatement of object motion vectors (tests/object_motion_ref.py) on closed forms, without a GPU, and
the new C-ABI entry's declaration, export and binding. tests/test_gpu_object_motion.py holds the G-buffer kernels to
the restatement."""
import ctypes as C
import os
import re

import numpy as np

import object_motion_ref as R
from ptsvgf.camera import Camera, mat_mul


def _camera(rot=0.0):
    cam = Camera(96, 64)
    cam.orbit(rot, 0.0)
    cam.update()
    return mat_mul(cam.cam_proj_mat, cam.cam_view_mat)


TRI = np.array([[0.1, -0.2, 0.3], [0.7, -0.1, 0.2], [0.2, 0.5, 0.1]])


def _point(u, v):
    return TRI[0] * (1 - u - v) + TRI[1] * u + TRI[2] * v


def _clip(m, P):
    m = np.asarray(m, np.float64).reshape(4, 4).T
    return m @ np.r_[P, 1.0]


def test_projection_and_linear_depth_are_the_shader_forms():
    M = _camera()
    P = _point(0.3, 0.4)
    c = _clip(M, P)
    assert np.allclose(R.proj(M, P), c[:2] / c[3] * 0.5 + 0.5, rtol=0, atol=1e-15)
    # gl_FragCoord.z / gl_FragCoord.w = window z * clip w
    assert np.isclose(R.lin_z(M, P), (c[2] / c[3] * 0.5 + 0.5) / (1.0 / c[3]), rtol=1e-15, atol=0)


def test_zero_displacement_is_the_camera_only_velocity():
    M, PV = _camera(3.0), _camera(0.0)
    P = np.stack([_point(0.2, 0.3), _point(0.6, 0.1)])
    got = R.motion(P, TRI, TRI, M, PV)
    assert np.array_equal(got[:, :2], R.proj(M, P) - R.proj(PV, P))
    assert np.all(np.abs(got[:, :2]) > 1e-4)  # the camera did move
    assert np.array_equal(got[:, 2], np.zeros(2))


def test_uniform_translation():
    M, PV = _camera(3.0), _camera(0.0)
    d_prev = np.array([-0.02, -0.03, 0.01])  # where the triangle was, relative to now
    P = np.stack([_point(0.2, 0.3), _point(0.0, 0.0), _point(0.25, 0.75)])
    got = R.motion(P, TRI, TRI + d_prev, M, PV)
    for k in range(len(P)):
        prevP = P[k] + d_prev
        c, pc, pc0 = _clip(M, P[k]), _clip(PV, prevP), _clip(PV, P[k])
        want_xy = (c[:2] / c[3] * 0.5 + 0.5) - (pc[:2] / pc[3] * 0.5 + 0.5)
        want_z = (pc[2] / pc[3] * 0.5 + 0.5) * pc[3] - (pc0[2] / pc0[3] * 0.5 + 0.5) * pc0[3]
        assert np.allclose(got[k, :2], want_xy, rtol=0, atol=1e-14)
        assert np.isclose(got[k, 2], want_z, rtol=0, atol=1e-13)
    assert np.allclose(got, R.motion_from_displacement(P, d_prev, M, PV), rtol=0, atol=1e-14)
    # a static camera sees the depth term as the plain change of linear depth
    got = R.motion(P, TRI, TRI + d_prev, PV, PV)
    assert np.allclose(got[:, 2], R.lin_z(PV, P + d_prev) - R.lin_z(PV, P), rtol=0, atol=1e-14)


def test_one_moved_vertex_blends_with_the_barycentrics():
    M = PV = _camera()
    prev = TRI.copy()
    prev[1] += [0.05, -0.02, 0.04]  # vertex 2 was elsewhere: its weight is u
    for u, v in [(0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (0.25, 0.5), (0.5, 0.5)]:
        P = _point(u, v)
        assert np.allclose(R.barycentrics(P, TRI), (u, v), rtol=0, atol=1e-14)
        D = R.displacement(P, TRI, prev)
        assert np.allclose(D, u * np.array([0.05, -0.02, 0.04]), rtol=0, atol=1e-15)
        got = R.motion(P, TRI, prev, M, PV)
        assert np.allclose(got[:2], R.proj(M, P) - R.proj(PV, P + D), rtol=0, atol=1e-15)
    # the other two vertices hold still: no motion at all there (static camera)
    assert np.array_equal(R.motion(_point(0.0, 0.0), TRI, prev, M, PV), np.zeros(3))
    assert np.array_equal(R.motion(_point(0.0, 1.0), TRI, prev, M, PV), np.zeros(3))
    # vectorised over pixels with one triangle each
    Ps = np.stack([_point(0.25, 0.5), _point(0.5, 0.25)])
    both = R.motion(Ps, np.stack([TRI, TRI]), np.stack([prev, TRI]), M, PV)
    assert np.array_equal(both[0], R.motion(Ps[0], TRI, prev, M, PV))
    assert np.array_equal(both[1], np.zeros(3))


def test_entry_point_is_declared_exported_and_bound():
    from ptsvgf import _lib

    name = "pt_raster_pass_set_prev_vertices"
    txt = open(os.path.join(_lib.INCLUDE_DIR, "ptsvgf.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(\s*uint32_t\s+\w+,\s*const\s+void\s*\*\s*\w+,\s*const\s+void\s*\*\s*\w+,"
                     r"\s*size_t\s+\w+\s*\)\s*;" % name, txt)
    lib = C.CDLL(os.path.join(_lib.LIB_DIR, "libptsvgf.so"))
    assert hasattr(lib, name)
    sig = {n: (r, a) for n, r, a in _lib._PT_SIGS}[name]
    assert sig == (C.c_int, [C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t])
    assert name in _lib.exported_symbols()[0]
    from ptsvgf import gl
    from ptsvgf.renderer import Renderer
    import inspect

    assert callable(gl.Rasterize_RenderPass.set_prev_vertices)
    assert "prev_raster" in inspect.signature(Renderer.rebuild_bvh).parameters
    host = open(os.path.join(_lib.PKG_ROOT, "host", "render_pass.h")).read()
    assert name in host and "set_prev_vertices" in host
