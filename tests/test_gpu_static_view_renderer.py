"""The whole renderer over a camera that rests, moves and rests again, with frames in flight (DESIGN.md "Static view"):
K = 3 path-tracing slots on their own streams and K + 1 G-buffer sets, host_pace both ways. The planes bench.py compares
(its PARITY_PLANES) must equal, bit for bit and frame by frame, those of a renderer with both switches off
(primary_cache = 0, reuse_static = 0), and pt_debug_stage_counts must show work exactly where the keys say: a slot's
primary stage runs when the view or the geometry differ from that slot's last stage, a set's G-buffer draw launches
when view, pre_viewproj, geometry or the pending object motion differ from that set's last draw. 160 x 96."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, K = 160, 96, 3
PARITY_PLANES = ("color", "albedo", "reproj_illum", "variance", "history_illum", "atrous", "modulate")  # bench.py's

# 5 static frames, 2 orbit steps, 5 static, one pose_objects, 4 static
STEPS = [None] * 5 + ["orbit", "orbit"] + [None] * 5 + ["pose"] + [None] * 3


def _expected():
    """Per frame (primary stage runs, G-buffer draw launches) from the keys: the view, the view before it
    (pre_viewproj), the geometry and whether motion records are pending, against what the frame's slot / set saw at
    its last stage / draw."""
    view = geom = 0
    pre = 0
    motion_left = 0
    slot, gset = {}, {}
    out = []
    for f, st in enumerate(STEPS):
        if st == "orbit":
            view += 1
        if st == "pose":
            geom += 1
            motion_left = 1  # the first frame after the pose draws with the records, every later one without
        kp = (view, geom)
        kg = (view, pre, geom, motion_left > 0)
        out.append((slot.get(f % K) != kp, gset.get(f % (K + 1)) != kg))
        slot[f % K], gset[f % (K + 1)] = kp, kg
        pre = view
        motion_left = max(0, motion_left - 1)
    return out


def _run(gl, scene, reuse, host_pace):
    from ptsvgf.renderer import Renderer
    from ptsvgf.scene import transform

    r = Renderer(scene, W, H, mode="fast", aspect_corrected=True, run_taa=False, run_output=False, frames_in_flight=K,
                 host_pace=host_pace)
    if not reuse:
        for p in r.init_pass:
            p.set_uniform_int("reuse_static", 0)
        for p, _ in r.pt_slots:
            p.set_uniform_int("primary_cache", 0)
    r.rebuild_bvh(raster=scene.raster, leaf_n=8, ploc_radius=16)

    def counts():
        a = [p.stage_counts() for p, _ in r.pt_slots]
        b = [p.stage_counts() for p in r.init_pass]
        return tuple(sum(x[i] for x in c) for c in (a, b) for i in (0, 1))

    frames, work = [], []
    for st in STEPS:
        if st == "orbit":
            r.camera.orbit(2.0, 1.0)
        elif st == "pose":
            r.pose_objects({2: transform(rot=(0, 5, 0), trans=(0, 0.05, 0))})
        c0 = counts()
        r.frame()
        pl = r.planes()
        frames.append({k: gl.readback(pl[k]) for k in PARITY_PLANES})
        c1 = counts()
        work.append(tuple(b - a for a, b in zip(c0, c1)))  # (stage runs, stage reuses, draws, elided draws)
    r.close()
    return frames, work


@pytest.mark.parametrize("host_pace", [False, True])
def test_rest_move_rest_pose(gpu, scene_small, host_pace):
    on, w_on = _run(gpu, scene_small, True, host_pace)
    off, w_off = _run(gpu, scene_small, False, host_pace)
    want = _expected()
    print("stage runs / draws with reuse on:", [(a, c) for a, _, c, _ in w_on])
    assert w_on == [(int(p), 1 - int(p), int(g), 1 - int(g)) for p, g in want], w_on
    assert w_off == [(1, 0, 1, 0)] * len(STEPS)
    # reuse in every static run, none on the frames that changed
    for lo, hi in ((0, 5), (7, 12)):
        assert any(not p for p, _ in want[lo:hi]) and any(not g for _, g in want[lo:hi])
    for f, st in enumerate(STEPS):
        if st:
            assert want[f] == (True, True), f
    for f, (a, b) in enumerate(zip(on, off)):
        for k in PARITY_PLANES:
            bad = np.argwhere(np.any(a[k].view(np.uint32) != b[k].view(np.uint32), axis=-1))
            assert len(bad) == 0, (f, k, len(bad), bad[:5].tolist())
