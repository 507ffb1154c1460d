"""Headless ``main.cpp``: the reference's startup (main.cpp:65-338) and frame
loop (main.cpp:436-602) driven through the drop-in C ABI.

Two drivers over the same kernels:

* :class:`Renderer` (``mode="reference"``) issues the reference's exact call
  sequence — every pass, every ping-pong ``bilt`` copy, the iteration-1 history
  copy and the 5-target ``save_frame_data`` copy (main.cpp:499-553). This is
  what a C++ ``main.cpp`` linked against libptsvgf.so does.
* ``mode="fast"`` keeps the identical math but replaces the copies with
  double-buffered targets (pointer swaps, SURVEY.md §2 "build replaces with
  pointer swaps"): same outputs bit for bit (tests/test_gpu_frame.py), fewer
  HBM bytes per frame. This is the benchmarked path.

TAA and the output tonemap run in both modes (main.cpp:537-590).
"""
from __future__ import annotations

import os
import time

import numpy as np

from . import gl
from .camera import Camera, mat_mul, parameter_config, rigid_inverse
from .gl import GL_TEXTURE_2D, GL_TEXTURE_2D_ARRAY, GL_TEXTURE_BUFFER, RenderPass, Rasterize_RenderPass, getShaderProgram, getTextureRGB32F
from .scene import Scene

SHADERS = "./shaders/"
VISIT_BUDGET = 256  # node + triangle visits before a ray goes to the wave-cooperative walk (_ensure_slots)


def _prog(frag: str, vert: str = "vert.vert") -> int:
    return getShaderProgram(SHADERS + frag, SHADERS + vert)


class PassGroup:
    """Several passes of one program driven as one: a call applies to each (returns the first result)."""

    def __init__(self, passes):
        self.passes = list(passes)

    def __getattr__(self, name):
        fns = [getattr(p, name) for p in self.passes]

        def call(*a, **k):
            return [f(*a, **k) for f in fns][0]

        return call


def _set_stream(stream) -> None:
    from ._lib import check, pt

    check(pt().pt_set_stream(stream.cuda_stream))


_FREE_STREAMS: dict = {}  # (device, priority) -> streams a closed renderer gave back


def acquire_stream(priority: int = 0):
    """A stream no live renderer holds. torch.cuda.Stream() hands out its fixed per-priority pool (32 streams)
    round-robin, so after 32 of them two live objects share one queue: a renderer's streams, or a renderer's and a
    process group's communication stream (taken from the same pool). Recycling what closed renderers held keeps
    the allocations far below the pool's size over a run of many renderers (bench calibration, several views)."""
    import torch

    key = (torch.cuda.current_device(), priority)
    pool = _FREE_STREAMS.setdefault(key, [])
    if pool:
        return pool.pop()
    stream = torch.cuda.Stream(priority=priority)
    stream._ptsvgf_key = key  # the bucket it returns to (the priority torch reports may be clamped)
    return stream


def release_stream(stream) -> None:
    """Give a stream back to the pool; the library first drops what it holds for it (pt_stream_release: the
    trace_fork side stream, merged-environment reader events), so the next holder starts afresh."""
    from ._lib import check, pt

    key = getattr(stream, "_ptsvgf_key", None)
    if key is None:
        return  # not from the pool
    handle = getattr(stream, "cuda_stream", None)
    if handle is not None:
        rc = pt().pt_stream_release(handle)
        if rc != -9:  # PT_ERR_STATE: the library was never initialised, so it holds nothing for the stream
            check(rc)
    _FREE_STREAMS.setdefault(key, []).append(stream)


def reserved_cus(ncu: int, reserve: int, xcds: int = 8) -> list:
    """`reserve` CU indices spread evenly over the XCDs whether the CU mask numbers CUs XCD by XCD (XCD = i // (ncu /
    xcds)) or round-robin (XCD = i % xcds): the j-th reserved CU sits in block j % xcds at residue j % xcds."""
    per = ncu // xcds
    out = []
    for j in range(reserve):
        b, k = j % xcds, j // xcds
        out.append(b * per + (b + xcds * k) % per)
    return sorted(set(out))


def masked_stream(exclude: list):
    """A stream whose kernels never run on the CUs in `exclude` (pt_stream_create_cu_masked), as a torch external
    stream; returns (stream, raw handle) — destroy the handle with pt_stream_destroy after the last use."""
    import ctypes as C

    import torch

    from ._lib import check, pt

    n = C.c_int()
    check(pt().pt_device_cus(C.byref(n)))
    words = (n.value + 31) // 32
    mask = (C.c_uint32 * words)(*([0xFFFFFFFF] * words))
    for i in range(n.value, words * 32):
        mask[i // 32] &= ~(1 << (i % 32)) & 0xFFFFFFFF
    for i in exclude:
        mask[i // 32] &= ~(1 << (i % 32)) & 0xFFFFFFFF
    h = C.c_void_p()
    check(pt().pt_stream_create_cu_masked(words, mask, C.byref(h)))
    return torch.cuda.ExternalStream(h.value), h.value


def priority_stream(priority: int):
    """A stream at HIP queue priority `priority` (pt_stream_create_priority: lower = higher; torch's pool stops at
    0 and -1, this reaches HIP's low priority too), as a torch external stream; returns (stream, raw handle) — destroy
    the handle with pt_stream_destroy after the last use."""
    import ctypes as C

    import torch

    from ._lib import check, pt

    h = C.c_void_p()
    check(pt().pt_stream_create_priority(int(priority), C.byref(h)))
    return torch.cuda.ExternalStream(h.value), h.value


class Renderer:
    # True (set before a frame is drawn): the fast driver's G-buffer draws also write the primary rasterisers' bound of
    # every pixel as one float (vec3 uniform bound_eye; kernels_pt.hip gb_finish), which the frame's path tracer then
    # reads instead of the two hint planes (its int uniform bound_plane = 0 keeps the two-plane read). Same bits; off
    # by default: it measured inside the noise (DESIGN.md "Paths end in place")
    bound_plane = False

    def __init__(self, scene: Scene, width: int, height: int, config: parameter_config | None = None,
                 mode: str = "fast", aspect_corrected: bool | None = None, band=None, prune: bool = True,
                 atrous_exact: bool = False, run_taa: bool = True, run_output: bool = True, tex_factory=None,
                 halo=None, gbuffer_rows=None, frames_in_flight: int = 1, after_gbuffer=None, back_lag: int = 0,
                 trace_batch: int = 1, front_streams: int | None = None, pt_source=None, pt_flush=None,
                 stage_rows=None, early_history=None, draw_gbuffer: bool = True, fuse_modulate: bool = True,
                 host_pace: bool = False, spp: int = 1, adaptive=None, adaptive_pool=None,
                 adaptive_rule: str = "relative", adaptive_zeta: float = 0.1, sample_moments: bool = False,
                 static_background: bool = True, light_settle: int | None = None):
        """band = (y0, y1, row0, rows) for screen-band sharding; tex_factory(w, h) -> handle allocates the
        frame-sized planes (ptsvgf.dist wraps torch tensors); halo(stage, {plane name: handle}) is called before
        the SVGF passes that read rows beyond the band (dist.HALO_SCHEDULE names the planes); after_gbuffer(set,
        torch stream) right after a G-buffer draw is issued; gbuffer_rows = (y0, y1) rows the G-buffer computes
        (default: the band).

        frames_in_flight = K > 1 (fast driver): the G-buffer + path tracer of frame f (the front end, which
        depends on nothing but the camera) run on stream f % K while the SVGF chain (sequential: each frame
        reads the previous frame's history) runs on one back-end stream. Frame f's front end waits only for
        the SVGF of frame f-K, whose buffers it reuses. The front end's launches end in long tails (a few
        rays through dense geometry); with K frames in flight another frame's work fills them. Same
        kernels, same inputs, same bits as K = 1 (tests/test_gpu_parity.py); throughput rises, latency
        from camera to finished frame is up to K frames.

        back_lag = D (0 <= D < K, frames in flight only): frame() issues the front end of frame f and the SVGF
        back end of frame f - D, so a host wait before a back-end pass (the band renderer's motion bound, read
        from the G-buffer before the reprojection exchange is sized) finds a G-buffer issued D frames earlier
        instead of stalling the issue of the next front end. planes() and time_atrous() first issue the back
        ends still pending (flush); results are those of D = 0.

        trace_batch = B (2..8, at most K, frames in flight only): the path tracer of B consecutive frames runs as
        one batched draw (pt_pass_draw_batch) issued with the last of them — its list-driven traversal launches
        trace all B frames' rays at once, so a thin band's launches carry B times the rays. The back lag is raised
        to at least B - 1 (a frame's back end needs its batch). Same bits.

        front_streams = S (frames in flight only, default K): the front ends of frame f run on stream f % S (the K
        frame slots are unchanged). pt_source(f, slot, stream) (fast driver, frames in flight): instead of drawing
        the path tracer, fill frame f's colour / emission / albedo planes of `slot` from elsewhere
        (dist.FrameShardRenderer: some rank traced the whole frame) once the slot is free; it is called right after the
        G-buffer of f is issued on `stream` and returns a holder dict whose "ev" (a torch event, set by the time the
        back end of f is issued) the back end waits for; pt_flush() is called by flush() before the pending back
        ends are issued.

        host_pace (frames in flight only): before issuing frame f's front end the host waits for the back end of
        frame f - K, which that front end waits for on the GPU anyway. Without it the host queues frames as fast as it
        can issue them and each frame's camera reaches the GPU long before its G-buffer runs (camera-to-modulate ≈ 8
        frames at K = 4); with it at most K frames are queued.

        spp = N (1 .. 8, either driver; also the settable property `spp`): every path-tracing draw takes N samples
        per pixel over one primary hit, sample s with the counter frameCounter * N + s, and writes their mean (in
        sample order) to the colour plane the SVGF chain reads; emission / albedo are unchanged (DESIGN.md "Samples
        per pixel"). The samples fill the traversal launches as a batch's frames do, so frames are not batched
        (trace_batch) while N > 1.

        adaptive = tau (a tolerance > 0; default None; needs spp >= 2; either driver): per-pixel sample counts
        (DESIGN.md "Adaptive sample counts"). Every path-tracing slot owns a statistics plane its draws' resolve
        writes and a count plane its draws read. Before a slot's draw, on the front end's stream right after the
        G-buffer, the count plane is derived on the device from the statistics of the slot's own previous draw, looked
        up along this frame's motion vectors scaled by the frames since that draw; a slot that has not drawn takes N
        samples everywhere. sample_counts() / sample_stats() read the planes back.

        adaptive_pool = W (a pooled weight cap >= 2; default None, which leaves the path above as it is; needs
        adaptive), adaptive_rule = "relative" | "absolute" ("absolute" needs adaptive_pool), adaptive_zeta (relative
        depth tolerance of the history, > 0): the counts come from luminance statistics pooled over the slot's draws
        (DESIGN.md "Pooled sample statistics", pt_sample_counts_pool). Every slot owns two pool planes and two count
        planes, swapped every draw; the step runs at every frame of the slot, the first included (which writes the
        depths and gives N on surfaces, 1 on the background). sample_pool() reads the current pool plane back.

        sample_moments (default False; needs spp >= 2; either driver, any K; composes with adaptive, adaptive_pool and
        accumulate_color): SVGF's variance from the samples' own moments (DESIGN.md "SVGF from sample moments").
        Every path-tracing slot owns one RGBA32F texture its draws' resolve fills with (mu, nu, r, n) per pixel
        (pt_pass_set_sample_moments); the reproject and variance passes of that frame's back end bind it as
        gSampleMoments. The mode is fixed for the renderer's life: its history holds per-sample moments from the
        first frame on. sample_moments() reads the last frame's plane back.

        static_background (default True; one-GPU fast driver only, under the conditions of the G-buffer's
        reuse_static and without bands, stage rows, sample moments or accumulation): the reproject, variance and
        a-trous passes get the int uniform static_background = 1, so on a standing view their draws skip the tiles
        that are all background and already hold what the draw would store (DESIGN.md "Static view, part 3"). Same
        bits in every plane. The G-buffer sets then share one copy of the triangles from construction on, as they do
        after rebuild_bvh. PTSVGF_STATIC_BACKGROUND=0 in the environment forces it off, here (the renderer is then
        constructed as with static_background=False) and in the library."""
        if mode not in ("fast", "reference"):
            raise ValueError(mode)
        self._pool = self._check_adaptive_pool(adaptive, adaptive_pool, adaptive_rule, adaptive_zeta)
        self._sm_on = self._check_sample_moments(sample_moments, self._check_spp(spp), band, pt_source)
        if self._sm_on and int(trace_batch) > 1:
            raise ValueError("sample_moments needs the slot's own draws: no trace batching")
        self.mode = mode
        self.W, self.H = int(width), int(height)
        self.cfg = config or parameter_config()
        self.camera = Camera(self.W, self.H)
        self.aspect_corrected = (self.W != self.H) if aspect_corrected is None else bool(aspect_corrected)
        self.prune = prune
        self.atrous_exact = atrous_exact
        self.run_taa = run_taa
        self.run_output = run_output
        self.scene = scene
        self._after_gbuffer = after_gbuffer
        self._lib_stream = None  # torch stream the library draws on (None: torch's current stream)
        if band is not None:
            y0, y1, row0, rows = band
            gl.set_band(self.W, self.H, y0, y1, row0, rows)
        self.band = band
        self._halo_cb = halo
        W, H = self.W, self.H
        self._owned: list[int] = []   # every texture this renderer created (close() destroys them)
        make = tex_factory or getTextureRGB32F

        def tex(w, h):
            t = make(w, h)
            self._owned.append(t)
            return t

        self._tex = tex

        # scene buffers (main.cpp:136-181)
        self.trianglesTextureBuffer = gl.texture_buffer(scene.tri_enc)
        self.nodesTextureBuffer = gl.texture_buffer(scene.node_enc)
        self.pointLightBuffer = gl.texture_buffer(scene.lights)
        hh, hw, _ = scene.hdr.shape
        self.hdrMap = getTextureRGB32F(hw, hh)
        gl.upload_rgb32f(self.hdrMap, scene.hdr)
        self.hdrCache = getTextureRGB32F(hw, hh)
        gl.upload_rgb32f(self.hdrCache, scene.cache)
        self._owned += [self.trianglesTextureBuffer, self.nodesTextureBuffer, self.pointLightBuffer, self.hdrMap,
                        self.hdrCache]
        self.materials_array = None                            # main.cpp:184-205
        if getattr(scene, "textures", None) is not None:
            self.materials_array = gl.texture_array(scene.textures)
            self._owned.append(self.materials_array)
        self.hdrResolution = hw

        self.K = int(frames_in_flight)
        if self.K < 1 or (self.K > 1 and mode != "fast"):
            raise ValueError("frames_in_flight must be >= 1, and > 1 only with the fast driver")
        self.B = int(trace_batch)
        self._spp = self._check_spp(spp)
        self.adaptive = self._check_adaptive(adaptive, self._spp)
        self._ad: list = []  # per path-tracing slot: stats / counts (device tensors), last (frame of its last draw)
        self._sm: list = []  # per path-tracing slot: the texture its resolve writes (sample_moments)
        if self.adaptive is not None and pt_source is not None:
            raise ValueError("adaptive needs the renderer's own path-tracing draws (no pt_source)")
        if not 1 <= self.B <= min(self.K, 8) or (self.B > 1 and mode != "fast"):
            raise ValueError(f"trace_batch must be in [1, min(frames_in_flight, 8)] (fast driver), got {trace_batch}")
        self.lag = max(int(back_lag), self.B - 1)
        self.host_pace = bool(host_pace) and self.K > 1
        self.pace_wait_s = 0.0  # host time spent in host_pace's waits (diagnostics)
        if not 0 <= self.lag < self.K:
            raise ValueError(f"back_lag must be in [0, frames_in_flight) = [0, {self.K}), got {back_lag}")
        self._nfs = self.K if front_streams is None else int(front_streams)
        if not 1 <= self._nfs <= self.K:
            raise ValueError(f"front_streams must be in [1, frames_in_flight], got {front_streams}")
        if pt_source is not None and (mode != "fast" or self.K < 2 or self.B > 1):
            raise ValueError("pt_source needs the fast driver with frames in flight and no trace batching")
        self._pt_source = pt_source
        self._pt_flush = pt_flush
        self._stage_rows = stage_rows
        self._draw_gbuffer = bool(draw_gbuffer)
        if not draw_gbuffer and pt_source is None:
            raise ValueError("draw_gbuffer=False needs a pt_source that provides the G-buffer planes")
        self._early_history = early_history
        # fast driver: the last a-trous iteration also writes the modulated colour (svgf_modulate.frag) from its
        # epilogue, saving the modulate pass's launch and its re-read of the a-trous output and normal/depth
        # (same arithmetic, same bits: tests/test_gpu_parity.py::test_fused_modulate_equals_modulate_pass)
        self.fuse_modulate = bool(fuse_modulate) and mode == "fast"
        self._ready = None  # pt_source's event for the front end being issued
        self._batch: list = []  # path-tracing passes of the open batch: (pass, G-buffer-done event, stream, holder)
        self._pending: list = []  # front ends whose back end is not issued yet (back_lag)
        # a serial renderer draws on torch's stream of its construction, whatever stream another renderer in the
        # process left the library on (the library's stream is process-global, pt_set_stream)
        self._serial_stream = None
        if self.K == 1:
            import torch

            self._serial_stream = torch.cuda.current_stream()
        self.back_set = 0         # G-buffer set of the back end being issued (halo / after_gbuffer users)
        # G-buffer sets: the reference has one; fast mode alternates two (this frame / previous frame);
        # with K frames in flight, frame f writes set f % (K+1) once SVGF(f-K) has read it (as "previous")
        nbuf = (self.K + 1 if self.K > 1 else 2) if mode == "fast" else 1
        # G-buffer (main.cpp:208-226); fast mode double-buffers it (prev normal/depth = other parity)
        self.init_pass = []
        self.gbuf = []
        # object motion (rebuild_bvh(prev_raster=...)): records bound on init_pass[0]; the next frame draws with them
        self.object_motion = True
        self._pose = None       # pose_objects: the pt_pose handle, and the rest pose the last rebuild_bvh received
        self._pose_rest = None
        self._skin = None       # set_skin: the influences of skin_objects, kept with the rest pose
        self._skin_set = False  # whether the pose holds them
        self._motion_records = self._motion_pending = False
        self._last_raster =np.ascontiguousarray(scene.raster, np.float32).reshape(-1)
        raster_prog = _prog("rasterize_frag.frag", "rasterize_vert.vert")
        # static_background: the SVGF passes of this renderer write planes nothing else writes (reuse_static's
        # condition below), and every draw of a frame covers the whole frame with one sample's colour and its own
        # history. PTSVGF_STATIC_BACKGROUND=0 turns it off here as in the library, so that such a process is
        # constructed as with static_background=False.
        self._static_bg = (bool(static_background) and os.environ.get("PTSVGF_STATIC_BACKGROUND", "1") != "0"
                           and self._draw_gbuffer and after_gbuffer is None and pt_source is None and halo is None
                           and tex_factory is None and mode == "fast" and band is None and stage_rows is None
                           and early_history is None and not self._sm_on and not self.cfg.accumulate_color)
        for b in range(nbuf):
            g = dict(world=tex(W, H), normal_depth=tex(W, H), velocity=tex(W, H), fwidth=tex(W, H))
            p = Rasterize_RenderPass(raster_prog, W, H)
            p.colorAttachments += [g["world"], g["normal_depth"], g["velocity"], g["fwidth"]]
            p.set_uniform_int("screen_width", W)
            p.set_uniform_int("screen_height", H)
            if gbuffer_rows is not None:
                p.set_rows(*gbuffer_rows)
            # reuse_static (DESIGN.md "Static view"): this renderer alone writes its G-buffer sets: it draws them
            # itself into planes the library allocated, and no hook (after_gbuffer, pt_source, halo) hands them to
            # code that could write them. A static view then draws each set once and leaves it.
            own_planes = (self._draw_gbuffer and after_gbuffer is None and pt_source is None and halo is None
                          and tex_factory is None)
            p.set_uniform_int("reuse_static", 1 if own_planes else 0)
            self._own_planes = own_planes and band is None  # (the path-tracing passes' reuse_static, _ensure_slots)
            # one copy of the triangles for every set: the sets of one view then have one G-buffer content, which
            # is what lets a quiet-tile set serve the frames of all of them
            if b > 0 and self._static_bg:
                p.bind_shared(self.init_pass[0])
            else:
                p.bindData(scene.raster)
            self.init_pass.append(p)
            self.gbuf.append(g)

        # path tracer (main.cpp:229-248)
        # (one pass + output set per frame in flight: each owns its wavefront state)
        # accumulate mode (path_tracing.frag:1116-1119) reads the previous frame's colour: the fast driver keeps
        # at least two slots so lastFrame is the other slot's colour output (the reference copies it,
        # save_frame_data.frag), and with frames in flight each front end then waits for the previous one
        self.accumulate = bool(self.cfg.accumulate_color)
        nslots = max(self.K, 2) if (self.accumulate and mode == "fast") else self.K
        self.pt_slots = []
        # set_lights: the path-tracing draws a moved light stands before its triangle bins are rebuilt (uniform
        # point_bins_settle); None: the library's default
        if light_settle is not None and int(light_settle) < 0:
            raise ValueError(f"light_settle must be >= 0, got {light_settle}")
        self._light_settle = None if light_settle is None else int(light_settle)
        self._pt_prune = prune
        self._ensure_slots(nslots)
        self._use_slot(0)
        self._streams = None
        if self.K > 1:
            import torch  # streams and events are torch plumbing (the kernels are the library's)

            self._streams = [acquire_stream() for _ in range(self._nfs)]
            # the SVGF back end is a chain of short launches (and, on bands, exchanges) beside the front ends' long
            # traversal launches: on a high-priority queue its kernels take CUs as soon as waves retire instead of
            # queueing behind resident traversal waves (PTSVGF_BACK_PRIORITY=0: normal priority, A/B)
            hi = os.environ.get("PTSVGF_BACK_PRIORITY", "1") != "0"
            self._back = acquire_stream(-1 if hi else 0)
            self._slot_free = [None] * self.K  # event: SVGF of the frame that last used the slot is done
            self._fe_prev = None

        # SVGF targets
        if mode == "reference":
            self._build_reference_passes()
        else:
            self._build_fast_passes()
        # output / tonemap (main.cpp:336-338); a readable target instead of the default framebuffer
        self.output_tex = tex(W, H)
        self.output_pass = RenderPass(_prog("output_pass.frag"), W, H)
        self.output_pass.colorAttachments.append(self.output_tex)
        self.output_pass.bindData(True)
        self.pre_viewproj = mat_mul(self.camera.cam_proj_mat, self.camera.cam_view_mat)  # main.h:48
        self.frame_index = 0
        self._profile = False
        self._times: dict = {}
        self.back_events = None  # [start, end] HIP events per back end when set to a list (frames in flight only)
        # (camera, modulate done) HIP events per frame when set to a list (frames in flight only): latency_ms()
        self.latency_events = None
        self._clock = None  # the stream camera-time events are recorded on (idle)
        if self.K > 1:
            # the planes were zero-filled on the stream current at their creation (the library's memset, a tex_factory's
            # torch.zeros) and frames draw on the renderer's own streams, which do not wait for that one: a first frame
            # could read (or be overwritten by) a late fill. Memory a closed renderer freed still holds its old values,
            # so this showed as a history differing from the one-GPU frame after band calibration.
            import torch

            torch.cuda.synchronize()

    # ------------------------------------------------------------ passes ---
    def _svgf_pass(self, frag: str, atts) -> RenderPass:
        p = RenderPass(_prog(frag), self.W, self.H)
        p.colorAttachments += list(atts)
        p.bindData(False)
        return p

    def _build_reference_passes(self):
        W, H, tex = self.W, self.H, self._tex
        self.tmp_atrous_result = tex(W, H)
        self.bilt_pass = self._svgf_pass("bilt.frag", [self.tmp_atrous_result])
        self.next_frame_color_input = tex(W, H)
        self.save_next_frame_pass = self._svgf_pass("bilt.frag", [self.next_frame_color_input])
        self.taa_output = tex(W, H)
        self.pass_taa = self._svgf_pass("taa.frag", [self.taa_output])
        self.pass_taa.set_uniform_int("screen_width", W)
        self.pass_taa.set_uniform_int("screen_height", H)
        self.curIllumination, self.curMomentHistory = tex(W, H), tex(W, H)
        self.reproject_pass = self._svgf_pass("svgf_reproject.frag", [self.curIllumination, self.curMomentHistory])
        self.variance_compute_illumination = tex(W, H)
        self.variance_compute_pass = self._svgf_pass("svgf_variance.frag", [self.variance_compute_illumination])
        self.atrous_output = tex(W, H)
        self.atrous_pass = self._svgf_pass("svgf_Atrous.frag", [self.atrous_output])
        self.modulate_color = tex(W, H)
        self.svgf_modulate_pass = self._svgf_pass("svgf_modulate.frag", [self.modulate_color])
        self.lastIllumination, self.last_normal_depth = tex(W, H), tex(W, H)
        self.last_Moments_HistoryLength, self.last_acc_color, self.last_taa_color = tex(W, H), tex(W, H), tex(W, H)
        self.next_frame_input = self._svgf_pass("save_frame_data.frag", [
            self.lastIllumination, self.last_normal_depth, self.last_Moments_HistoryLength, self.last_acc_color,
            self.last_taa_color])
        for p in (self.reproject_pass, self.variance_compute_pass, self.atrous_pass):
            p.set_uniform_float("inv_screen_width", 1.0 / W)
            p.set_uniform_float("inv_screen_height", 1.0 / H)

    def _build_fast_passes(self):
        W, H, tex = self.W, self.H, self._tex
        self.illum = tex(W, H)                                  # reproject out 0
        self.moments = [tex(W, H), tex(W, H)]                   # reproject out 1 (history, by parity)
        self.hist_illum = [tex(W, H), tex(W, H)]                # a-trous iteration 1 output (history)
        self.var_out = tex(W, H)
        self.ping, self.pong = tex(W, H), tex(W, H)
        self.modulate_color = tex(W, H)
        self.taa = [tex(W, H), tex(W, H)]
        self.reproject = [self._svgf_pass("svgf_reproject.frag", [self.illum, self.moments[b]]) for b in (0, 1)]
        self.variance_compute_pass = self._svgf_pass("svgf_variance.frag", [self.var_out])
        self.atrous_to = {"ping": self._svgf_pass("svgf_Atrous.frag", [self.ping]),
                          "pong": self._svgf_pass("svgf_Atrous.frag", [self.pong]),
                          "hist0": self._svgf_pass("svgf_Atrous.frag", [self.hist_illum[0]]),
                          "hist1": self._svgf_pass("svgf_Atrous.frag", [self.hist_illum[1]])}
        self.svgf_modulate_pass = self._svgf_pass("svgf_modulate.frag", [self.modulate_color])
        # the last iteration with the modulate fused (colour attachment 1, "fuse_modulate"), per destination
        self.atrous_mod_to = {k: self._svgf_pass("svgf_Atrous.frag", [self._atrous_tex(k), self.modulate_color])
                              for k in self.atrous_to}
        for p in self.atrous_mod_to.values():
            p.set_uniform_int("fuse_modulate", 1)
        self.pass_taa = [self._svgf_pass("taa.frag", [self.taa[b]]) for b in (0, 1)]
        for p in self.pass_taa:
            p.set_uniform_int("screen_width", W)
            p.set_uniform_int("screen_height", H)
        for p in self.reproject + [self.variance_compute_pass, *self.atrous_to.values(), *self.atrous_mod_to.values()]:
            p.set_uniform_float("inv_screen_width", 1.0 / W)
            p.set_uniform_float("inv_screen_height", 1.0 / H)
            p.set_uniform_int("static_background", 1 if self._static_bg else 0)

    # ------------------------------------------------------------- frame ---
    def _ensure_slots(self, n: int) -> None:
        """Path-tracing passes + colour/emission/albedo outputs, one per frame slot (main.cpp:229-248)."""
        W, H, scene = self.W, self.H, self.scene
        while len(self.pt_slots) < n:
            p = RenderPass(_prog("path_tracing.frag"), W, H)
            outs = (self._tex(W, H), self._tex(W, H), self._tex(W, H))  # color, emission, albedo
            p.colorAttachments += list(outs)
            p.bindData(False)
            p.set_uniform_int("nTriangles", scene.ntris)
            p.set_uniform_int("nNodes", scene.node_enc.shape[0])
            p.set_uniform_int("width", W)
            p.set_uniform_int("height", H)
            p.set_uniform_int("pointLightSize", scene.lights.shape[0])
            p.set_uniform_int("aspect_corrected", int(self.aspect_corrected))
            p.set_uniform_int("prune", int(self._pt_prune))
            # lane-refill traversal waves: +8 % frames/s with frames in flight, -6 % serial (kernels_wf_trace.hip)
            # share of each bounce / shadow list traced by lane-refill waves (frames in flight only); with up to 12
            # chunk rounds per wave 75 / 85 / 90 / 95 % measured 183.1 / 184.3 / 183.7 / 183.9 fps at 4K and 57.2 / 58.7 /
            # 59.5 / 60.6 fps on the surface view, 1080p and 8 bands within noise (tools/refill_pct_sweep.sh)
            # (round 4, 8 waves per SIMD, 26 resident waves per CU: 100 % gave 4K 220.9 / 221.2 against 221.4 / 220.3 for
            # 90 and the surface view 74.4 / 74.2 against 71.3 / 72.1, profiles/r04/refill_pct_ab.log)
            # (round 5: also one frame at a time, now that the visit budgets below cut the refill waves' tails)
            p.set_uniform_int("trace_refill", 100)
            # one frame at a time: the bounce-0 shadow walk on a side stream beside the bounce-1 closest-hit walk
            # (their launch tails overlap): 4K serial 131.3 -> 145.4 fps, surface view 48.3 -> 49.3; with frames in
            # flight the other frames already fill those tails (215.7 / 215.6 fps at K = 4, profiles/r04/fork/)
            p.set_uniform_int("trace_fork", 1 if self.K == 1 else 0)
            # point-light shadow rays by the lights' triangle bins: +3.4 % at 4K with K = 4; one frame at a
            # time the bins' launch and the HDR walk run one after the other and measured 2.6 % slower
            # (profiles/point_bins/ab_first.log): off then. With frames in flight the library's default holds.
            if self.K == 1:
                p.set_uniform_int("point_bins", 0)
            if self._light_settle is not None:
                p.set_uniform_int("point_bins_settle", self._light_settle)
            # a ray still walking past VISIT_BUDGET node + triangle visits is finished by the wave-cooperative walk
            # (same bits): the launches no longer end on a few long walks. Round 5, same box (profiles/r05/serial/):
            # one frame at a time with lane refill 145.2 -> 160.8 fps at 4K (budgets 128 / 512: 151.3 / 151.8; refill
            # without budgets 146.6; without the fork 133.6); K = 4 219.8 / 220.7 -> 223.9 (512 / 1024: 222.1 / 220.0)
            p.set_uniform_int("shadow_budget", VISIT_BUDGET)
            p.set_uniform_int("closest_budget", VISIT_BUDGET)
            p.set_uniform_int("trace_batch", self.B)
            # reuse_static (DESIGN.md "Static view, part 4"): nothing but this slot's own draws writes its three outputs
            # under the conditions of the G-buffer's; a standing view's bounce-0 shade then keeps what they hold
            p.set_uniform_int("reuse_static", 1 if self._own_planes else 0)
            p.set_spp(self._spp)
            if self.adaptive is not None:
                import torch

                ad = dict(stats=torch.zeros((H, W, 2), dtype=torch.float32, device="cuda"),
                          counts=torch.full((H, W), 255, dtype=torch.uint8, device="cuda"), last=None)
                if self._pool is not None:  # the planes of the previous step beside those of this one
                    ad.update(counts_prev=torch.full((H, W), 255, dtype=torch.uint8, device="cuda"),
                              pool=torch.zeros((H, W, 4), dtype=torch.float32, device="cuda"),
                              pool_prev=torch.zeros((H, W, 4), dtype=torch.float32, device="cuda"), n_prev=None)
                torch.cuda.current_stream().synchronize()  # the slot's draws run on the renderer's own streams
                p.set_sample_stats(ad["stats"].data_ptr())
                p.set_sample_counts(ad["counts"].data_ptr())
                self._ad.append(ad)
            if self._sm_on:  # (library-allocated: the resolve addresses it by its device pointer in global rows)
                import torch

                sm = getTextureRGB32F(W, H)
                torch.cuda.synchronize()  # its zero fill, before a draw on one of the renderer's own streams
                self._owned.append(sm)
                p.set_sample_moments(gl.device_ptr(sm))
                self._sm.append(sm)
            self.pt_slots.append((p, outs))
        self.pass_path_tracing = PassGroup([p for p, _ in self.pt_slots])  # settings apply to every slot

    VIEWS = ("path_tracing_pic_1spp", "svgf_reprojected_pic", "svgf_variance_pic", "svgf_atrous_pic",
             "svgf_modulate_pic", "taa_pic", "final_pic", "accumulate_color")  # gui_config.h:7-17

    def set_view(self, view: str) -> None:
        """The debug-view switch (main.cpp:398-415 radio buttons + gui_config.h:37-45): selects the plane the
        output pass shows (main.cpp:558-586); accumulate_color turns accumulation on, every other view off, and
        any change restarts the frame counter."""
        if view not in self.VIEWS:
            raise ValueError(f"unknown view {view!r}; one of {self.VIEWS}")
        self.view = view
        self.cfg.accumulate_color = view == "accumulate_color"
        self.accumulate = self.cfg.accumulate_color
        if self.accumulate and self.mode == "fast":
            self._ensure_slots(max(self.K, 2))
        self.camera.frameCounter = 0

    def _view_plane(self, f: int) -> int:
        v = getattr(self, "view", "final_pic")
        pl = self._planes_of(f)
        return {"path_tracing_pic_1spp": pl["color"], "accumulate_color": pl["color"],
                "svgf_reprojected_pic": pl["reproj_illum"], "svgf_variance_pic": pl["variance"],
                "svgf_atrous_pic": pl["atrous"], "svgf_modulate_pic": pl["modulate"],
                "taa_pic": pl["final"], "final_pic": pl["final"]}[v]

    def _use_slot(self, s: int) -> None:
        """Path-tracing pass and outputs of frame slot s (frame f uses slot f % K)."""
        self._slot = s
        self.pt_pass, (self.curColor, self.Emission, self.Albedo) = self.pt_slots[s]

    def _gbuffer_and_pt(self, b: int):
        self._gbuffer(b)
        if self._pt_source is not None:
            self._ready = self._pt_source(self.frame_index, self._slot, self._lib_stream)
            return
        if self.adaptive is not None:
            self._derive_counts(self.gbuf[b])
        self._path_trace(self.gbuf[b] if self.mode == "fast" else None)

    def _gbuffer(self, b: int):
        cam = self.camera
        view, proj = cam.cam_view_mat, cam.cam_proj_mat
        ip = self.init_pass[b]
        ip.set_uniform_mat4("view", view)                      # main.cpp:436-443
        ip.set_uniform_mat4("projection", proj)
        ip.set_uniform_mat4("pre_viewproj", self.pre_viewproj)
        ip.set_uniform_uint("frameCounter", cam.frameCounter)
        if self.mode == "fast" and self.bound_plane:
            ip.set_uniform_vec3("bound_eye", cam.cam_position)
        if self._motion_records:  # only the first frame after a rebuild_bvh(prev_raster=...) sees the objects move
            ip.set_uniform_int("object_motion", 1 if self._motion_pending and self.object_motion else 0)
            self._motion_pending = False
        if not self._draw_gbuffer:  # its planes come with the path tracer's (pt_source)
            return
        self._draw(ip, "gbuffer")
        if self._after_gbuffer is not None:
            import torch

            self._after_gbuffer(b, self._lib_stream or torch.cuda.current_stream())

    def _path_trace(self, hint=None):
        """hint: this frame's G-buffer set (drawn before on the same stream); its world position and normal/depth
        planes bound the primary rays' walk (a result-preserving hint with no GL counterpart, kernels_wf_primary.hip
        wf_primary). The reference driver binds none, as main.cpp."""
        cam, cfg = self.camera, self.cfg
        view = cam.cam_view_mat
        self.cameraRotate = rigid_inverse(view)                # main.cpp:445
        pt = self.pt_pass                                      # main.cpp:447-470
        pt.set_uniform_vec3("eye", cam.cam_position)
        pt.set_uniform_mat4("cameraRotate", self.cameraRotate)
        pt.set_uniform_uint("frameCounter", cam.frameCounter)
        pt.set_uniform_int("hdrResolution", self.hdrResolution)
        pt.set_uniform_bool("use_normal_map", cfg.use_normal_texture)
        pt.set_uniform_bool("accumulate", cfg.accumulate_color)
        pt.set_uniform_float("clamp_threshold", cfg.clamp_threshold)
        pt.set_uniform_int("max_tracing_depth", cfg.max_tracing_depth)
        pt.reset_texture_slot()
        pt.set_texture_uniform(GL_TEXTURE_BUFFER, self.trianglesTextureBuffer, "triangles")
        pt.set_texture_uniform(GL_TEXTURE_BUFFER, self.nodesTextureBuffer, "nodes")
        if cfg.accumulate_color:
            last_acc = (self.last_acc_color if self.mode == "reference"
                        else self.pt_slots[(self.frame_index - 1) % len(self.pt_slots)][1][0])
            pt.set_texture_uniform(GL_TEXTURE_2D, last_acc, "lastFrame")
        if self.materials_array is not None:
            pt.set_texture_uniform(GL_TEXTURE_2D_ARRAY, self.materials_array, "material_array")
        pt.set_texture_uniform(GL_TEXTURE_2D, self.hdrMap, "hdrMap")
        pt.set_texture_uniform(GL_TEXTURE_2D, self.hdrCache, "hdrCache")
        pt.set_texture_uniform(GL_TEXTURE_BUFFER, self.pointLightBuffer, "pointLights")
        if hint is not None:
            pt.set_texture_uniform(GL_TEXTURE_2D, hint["world"], "gWorldPos")
            pt.set_texture_uniform(GL_TEXTURE_2D, hint["normal_depth"], "gNormalAndLinearZ")
        if self._batching():
            return  # drawn with its batch (_front_fast)
        self._draw(pt, "pathtrace")

    def _derive_counts(self, g: dict) -> None:
        """The current slot's count plane from its own previous statistics (library stream, after the G-buffer `g`).
        That draw's resolve is ordered before this launch by what already orders the slot's reuse (_slot_free; one
        stream when K = 1)."""
        ad = self._ad[self._slot]
        if self._pool is not None:
            return self._pool_counts(ad, g)
        if ad["last"] is not None:
            gl.sample_counts_derive(ad["stats"].data_ptr(), g["velocity"], g["normal_depth"],
                                    float(self.frame_index - ad["last"]), self.adaptive, self._spp,
                                    ad["counts"].data_ptr())
        ad["last"] = self.frame_index

    def _pool_counts(self, ad: dict, g: dict) -> None:
        """_derive_counts with adaptive_pool: swap the slot's planes, then one pt_sample_counts_pool from the previous
        step's planes into this one's; the pass reads the new count plane. At the slot's first frame nothing is
        bound: the step writes the depths and N on surfaces."""
        first = ad["last"] is None
        ad["counts"], ad["counts_prev"] = ad["counts_prev"], ad["counts"]
        ad["pool"], ad["pool_prev"] = ad["pool_prev"], ad["pool"]
        po = self._pool
        gl.sample_counts_pool(0 if first else ad["stats"].data_ptr(), 0 if first else ad["counts_prev"].data_ptr(),
                              self._spp if first else ad["n_prev"], 0 if first else ad["pool_prev"].data_ptr(),
                              g["velocity"], g["normal_depth"], 1.0 if first else float(self.frame_index - ad["last"]),
                              po["wmax"], po["zeta"], po["rule"], self.adaptive, self._spp, ad["pool"].data_ptr(),
                              ad["counts"].data_ptr())
        self.pt_slots[self._slot][0].set_sample_counts(ad["counts"].data_ptr())
        ad["last"], ad["n_prev"] = self.frame_index, self._spp

    def sample_counts(self) -> np.ndarray:
        """The count plane the last frame's path-tracing draw read, (H, W) uint8: 255 (= N) before the slot's first
        draw, else pt_sample_counts_derive's values 1 .. N (with adaptive_pool: pt_sample_counts_pool's 1 .. N at every
        frame). adaptive only."""
        return self._ad_read("counts")

    def sample_stats(self) -> np.ndarray:
        """The (mean, variance) plane the last frame's path-tracing draw wrote, (H, W, 2) float32. adaptive only."""
        return self._ad_read("stats")

    def sample_pool(self) -> np.ndarray:
        """The pool plane (m, v, w, z) the last frame's step wrote, (H, W, 4) float32. adaptive_pool only."""
        if self._pool is None:
            raise ValueError("the renderer was built without adaptive_pool")
        return self._ad_read("pool")

    def _ad_read(self, key: str) -> np.ndarray:
        if self.adaptive is None:
            raise ValueError("the renderer was built without adaptive")
        if self.frame_index < 1:
            raise ValueError("no frame drawn yet")
        import torch

        self.flush()
        torch.cuda.synchronize()
        return self._ad[(self.frame_index - 1) % len(self.pt_slots)][key].cpu().numpy()

    def sample_moments(self) -> np.ndarray:
        """The plane (mu, nu, r, n) the last frame's path-tracing draw wrote, (H, W, 4) float32. sample_moments only."""
        if not self._sm_on:
            raise ValueError("the renderer was built without sample_moments")
        if self.frame_index < 1:
            raise ValueError("no frame drawn yet")
        import torch

        self.flush()
        torch.cuda.synchronize()
        return gl.readback(self._sm[(self.frame_index - 1) % len(self.pt_slots)])

    @staticmethod
    def _check_sample_moments(on, spp, band=None, pt_source=None) -> bool:
        if not on:
            return False
        if spp < 2:
            raise ValueError("sample_moments needs spp >= 2: the plane is ignored at one sample per pixel")
        if band is not None:
            raise ValueError("sample_moments holds whole frames: no band")
        if pt_source is not None:
            raise ValueError("sample_moments needs the renderer's own path-tracing draws (no pt_source)")
        return True

    @staticmethod
    def _check_adaptive(tau, spp):
        if tau is None:
            return None
        if not float(tau) > 0.0:
            raise ValueError(f"adaptive must be a tolerance > 0 (or None), got {tau!r}")
        if spp < 2:
            raise ValueError("adaptive needs spp >= 2: one sample gives no variance estimate")
        return float(tau)

    @staticmethod
    def _check_adaptive_pool(adaptive, wmax, rule, zeta):
        """None without adaptive_pool, else the step's settings; ValueError for what the arguments refuse."""
        if rule not in ("relative", "absolute"):
            raise ValueError(f"adaptive_rule must be 'relative' or 'absolute', got {rule!r}")
        if wmax is None:
            if rule == "absolute":
                raise ValueError("adaptive_rule='absolute' needs adaptive_pool")
            return None
        if adaptive is None:
            raise ValueError("adaptive_pool needs adaptive (the tolerance)")
        if not float(wmax) >= 2.0:
            raise ValueError(f"adaptive_pool must be a weight cap >= 2 (or None), got {wmax!r}")
        if not float(zeta) > 0.0:
            raise ValueError(f"adaptive_zeta must be > 0, got {zeta!r}")
        return dict(wmax=float(wmax), rule=int(rule == "absolute"), zeta=float(zeta))

    def _batching(self) -> bool:
        return self.B > 1 and self.mode == "fast" and not self.cfg.accumulate_color and self._spp == 1

    @staticmethod
    def _check_spp(n) -> int:
        if int(n) != n or not 1 <= int(n) <= 8:
            raise ValueError(f"spp must be an integer in [1, 8], got {n!r}")
        return int(n)

    @property
    def spp(self) -> int:
        """Samples per pixel of every path-tracing draw (the int uniform spp of every slot's pass)."""
        return self._spp

    @spp.setter
    def spp(self, n) -> None:
        n = self._check_spp(n)
        self._check_adaptive(self.adaptive, n)
        self._check_sample_moments(self._sm_on, n)
        if n == self._spp:
            return
        self._issue_batch()  # frames of an open batch were set up at the old count
        self._spp = n
        for p, _ in self.pt_slots:
            p.set_spp(n)

    def set_lights(self, lights, first: int = 0) -> None:
        """Moving point lights (pt_lights_update): lights first .. first + n - 1 become `lights` ((n, 6): position,
        colour) from the next frame() on. The frames in flight are not flushed and keep the lights they were issued
        with; only an open path-tracing batch (trace_batch > 1), whose draws are still to be issued, is issued first.
        A light whose position changed walks the tree until it has stood for light_settle frames; then its triangle
        bins are rebuilt. Same bits as a renderer built on these lights."""
        a = np.ascontiguousarray(lights, dtype=np.float32).reshape(-1, 6)
        first = int(first)
        if first < 0 or first + a.shape[0] > self.scene.lights.shape[0]:
            raise ValueError(f"set_lights: lights {first} .. {first + a.shape[0] - 1} of {self.scene.lights.shape[0]}")
        self._issue_batch()
        gl.lights_update(self.pointLightBuffer, first, a)
        new = np.array(self.scene.lights, dtype=np.float32, copy=True)
        new[first:first + a.shape[0]] = a
        self.scene.lights = new

    def set_materials(self, materials: dict) -> None:
        """Material edits (pt_materials_update): `materials` is {obj_index: 18 floats in ptsvgf_scene.h's order}; the
        triangles of those objects take them from the next frame() on. The frames in flight are not flushed and keep
        the materials they were issued with; only an open path-tracing batch is issued first. Nothing that reads
        geometry alone is rebuilt or forgotten (trees, point-light bins, the static view's primary hit and verdicts);
        on a standing view each slot's next frame writes its emission and albedo planes in full once. The renderer's
        pose (pose_objects / skin_objects) and the rest pose rebuild_bvh received follow, and so does scene.tri_enc.
        Contiguous object ranges go in one call each. Same bits as a renderer built on these materials."""
        from .materials import apply_materials

        table = {}
        for o, m in materials.items():
            m = np.ascontiguousarray(m, dtype=np.float32).reshape(-1)
            if int(o) != o or int(o) < 0 or m.size != 18:
                raise ValueError(f"set_materials: object {o!r} needs an index >= 0 and 18 floats")
            table[int(o)] = m
        if not table:
            return
        self._issue_batch()
        objs = sorted(table)
        runs, start = [], 0
        for i in range(1, len(objs) + 1):
            if i == len(objs) or objs[i] != objs[i - 1] + 1 or i - start == 4096:
                runs.append(objs[start:i])
                start = i
        pose = self._pose or 0
        for run in runs:
            block = np.stack([table[o] for o in run])
            gl.materials_update(self.trianglesTextureBuffer, run[0], block, pose)
            self.scene.tri_enc = apply_materials(self.scene.tri_enc, run[0], block)
            if self._pose_rest is not None:  # a pose created later starts from these rows
                self._pose_rest = (apply_materials(self._pose_rest[0], run[0], block),) + tuple(self._pose_rest[1:])

    def set_environment(self, hdr) -> None:
        """Environment edits (pt_environment_update): `hdr`, an (h, w, 3) float32 numpy array or CUDA torch tensor of
        the map's size, is the environment from the next frame() on; its importance cache is built on the device.
        The frames in flight are not flushed and keep the environment they were issued with; only an open
        path-tracing batch is issued first. A tensor is consumed in the order of torch's current stream: what that
        stream has queued produced it, and it may be overwritten there right after the call. Trees, point-light bins
        and the static view's primary hit and verdicts stay; on a standing view each slot redraws what depends on the
        miss colour once. For a host array scene.hdr follows; scene.cache is dropped (nothing reads it after
        construction). Same bits as a renderer built on (hdr, hdr_cache(hdr))."""
        tensor = type(hdr).__module__.split(".")[0] == "torch"
        if not tensor:
            hdr = np.ascontiguousarray(hdr, dtype=np.float32)
        if tuple(hdr.shape) != (self.scene.hdr.shape[0], self.hdrResolution, 3):
            raise ValueError(f"set_environment: a map of shape {tuple(self.scene.hdr.shape)}, not {tuple(hdr.shape)}")
        self._issue_batch()
        if tensor:
            import torch

            _set_stream(torch.cuda.current_stream())
            try:
                gl.environment_update(self.hdrMap, self.hdrCache, hdr)
            finally:
                if self._lib_stream is not None:  # the draws' stream, as the last frame left it
                    _set_stream(self._lib_stream)
        else:
            gl.environment_update(self.hdrMap, self.hdrCache, hdr)
            self.scene.hdr = np.array(hdr, dtype=np.float32, copy=True)
        self.scene.cache = None

    # ------------------------------------------------------- ray queries ---
    def cast_rays(self, rays):
        """Closest hits of the caller's rays (gl.rays_closest) over the buffers the renderer draws now: after
        rebuild_bvh / refit_bvh / pose_objects / skin_objects the built pair, so `tri` indexes its leaf order.
        rays: (n, 8) float32 (origin, -, direction, tmax), numpy or a torch device tensor."""
        return gl.rays_closest(self.trianglesTextureBuffer, self.nodesTextureBuffer, rays)

    def occluded(self, rays):
        """Per ray, whether anything lies before its tmax (gl.rays_occluded); a bool array for numpy rays."""
        return gl.rays_occluded(self.trianglesTextureBuffer, self.nodesTextureBuffer, rays)

    def pick(self, x: int, y: int):
        """What lies under pixel (x, y) (y from the bottom row, as the textures count) for the renderer's current eye,
        cameraRotate and aspect_corrected: {"obj", "tri", "t", "point", "inside"}, or None on a miss. Issued on the
        library's own stream and waited for there alone: the frames in flight are not flushed and draw nothing anew."""
        from ._lib import check, pt

        cam = self.camera
        if not (0 <= int(x) < self.W and 0 <= int(y) < self.H):
            raise ValueError(f"pick: pixel ({x}, {y}) outside {self.W} x {self.H}")
        check(pt().pt_use_own_stream())
        try:
            rays = gl.rays_primary(cam.cam_position, rigid_inverse(cam.cam_view_mat), self.W, self.H,
                                   self.aspect_corrected, np.array([[int(x), int(y)]], np.int32))
            h = self.cast_rays(rays)[0]
        finally:
            if self._lib_stream is not None:  # the draws' stream, as the last frame left it
                _set_stream(self._lib_stream)
        if h["tri"] < 0:
            return None
        return {"obj": int(h["obj"]), "tri": int(h["tri"]), "t": float(h["t"]),
                "point": [float(v) for v in h["P"]], "inside": bool(h["inside"])}

    def _issue_batch(self) -> None:
        """Draw the open batch's path tracers on the stream of its last frame, after all its G-buffers."""
        if not self._batch:
            return
        import torch

        stream = self._batch[-1][2]
        for _, ev, _, _ in self._batch:
            stream.wait_event(ev)
        self._stream_to(stream)
        passes = [p for p, _, _, _ in self._batch]
        gl.draw_batch(passes)
        if self._profile:
            self._times.setdefault("pathtrace", []).append(passes[0].last_ms())
        done = torch.cuda.Event()
        done.record(stream)
        for _, _, _, holder in self._batch:
            holder["ev"] = done
        self._batch = []

    def _frame_reference(self):
        cfg = self.cfg
        g = self.gbuf[0]
        self._gbuffer_and_pt(0)
        rp = self.reproject_pass                               # main.cpp:474-486
        rp.reset_texture_slot()
        rp.set_uniform_float("depth_threshold", cfg.reproj_depth_threshold)
        rp.set_uniform_float("normal_threshold", cfg.reproj_normal_threshold)
        rp.set_texture_uniform(GL_TEXTURE_2D, g["velocity"], "gMotion")
        rp.set_texture_uniform(GL_TEXTURE_2D, self.curColor, "gColor")
        rp.set_texture_uniform(GL_TEXTURE_2D, self.Albedo, "gAlbedo")
        rp.set_texture_uniform(GL_TEXTURE_2D, self.Emission, "gEmission")
        rp.set_texture_uniform(GL_TEXTURE_2D, self.lastIllumination, "gPrevIllum")
        rp.set_texture_uniform(GL_TEXTURE_2D, self.last_Moments_HistoryLength, "gPrevMoments_HistoryLength")
        rp.set_texture_uniform(GL_TEXTURE_2D, g["normal_depth"], "gNormalAndLinearZ")
        rp.set_texture_uniform(GL_TEXTURE_2D, self.last_normal_depth, "gPrevNormalAndLinearZ")
        rp.set_texture_uniform(GL_TEXTURE_2D, g["fwidth"], "gNormalDepthFwidth")
        if self._sm_on:
            rp.set_texture_uniform(GL_TEXTURE_2D, self._sm[self._slot], "gSampleMoments")
        self._draw(rp, "reproject")
        vp = self.variance_compute_pass                        # main.cpp:488-495
        vp.reset_texture_slot()
        vp.set_uniform_float("gPhiColor", cfg.sigma_l)
        vp.set_uniform_float("gPhiNormal", cfg.sigma_n)
        vp.set_texture_uniform(GL_TEXTURE_2D, self.curIllumination, "gIllumination")
        vp.set_texture_uniform(GL_TEXTURE_2D, self.curMomentHistory, "gMoments_HistoryLength")
        vp.set_texture_uniform(GL_TEXTURE_2D, g["normal_depth"], "gNormalAndLinearZ")
        vp.set_texture_uniform(GL_TEXTURE_2D, g["fwidth"], "gNormalDepthFwidth")
        if self._sm_on:
            vp.set_texture_uniform(GL_TEXTURE_2D, self._sm[self._slot], "gSampleMoments")
        self._draw(vp, "variance")
        ap = self.atrous_pass                                  # main.cpp:499-526
        for i in range(cfg.num_atrous_iterations):
            ap.reset_texture_slot()
            ap.set_uniform_float("gPhiColor", cfg.sigma_l)
            ap.set_uniform_float("gPhiNormal", cfg.sigma_n)
            ap.set_uniform_int("gStepSize", 1 << i)
            ap.set_uniform_int("exact", int(self.atrous_exact))
            ap.set_texture_uniform(GL_TEXTURE_2D, g["normal_depth"], "gNormalAndLinearZ")
            ap.set_texture_uniform(GL_TEXTURE_2D, g["fwidth"], "gNormalDepthFwidth")
            src = self.variance_compute_illumination if i == 0 else self.tmp_atrous_result
            ap.set_texture_uniform(GL_TEXTURE_2D, src, "gIllumination")
            self._draw(ap, "atrous")
            self.bilt_pass.reset_texture_slot()
            self.bilt_pass.set_texture_uniform(GL_TEXTURE_2D, self.atrous_output, "in_texture")
            self._draw(self.bilt_pass, "copy")
            if i == 1:
                self.save_next_frame_pass.reset_texture_slot()
                self.save_next_frame_pass.set_texture_uniform(GL_TEXTURE_2D, self.atrous_output, "in_texture")
                self._draw(self.save_next_frame_pass, "copy")
        mp = self.svgf_modulate_pass                           # main.cpp:530-535
        mp.reset_texture_slot()
        mp.set_texture_uniform(GL_TEXTURE_2D, self.Albedo, "gAlbedo")
        mp.set_texture_uniform(GL_TEXTURE_2D, self.Emission, "gEmission")
        mp.set_texture_uniform(GL_TEXTURE_2D, self.atrous_output, "gIllumination")
        mp.set_texture_uniform(GL_TEXTURE_2D, g["normal_depth"], "gNormalAndLinearZ")
        self._rows(mp, "modulate")
        self._draw(mp, "modulate")
        if self.run_taa:                                       # main.cpp:537-544
            tp = self.pass_taa
            tp.reset_texture_slot()
            tp.set_texture_uniform(GL_TEXTURE_2D, self.modulate_color, "currentColor")
            tp.set_texture_uniform(GL_TEXTURE_2D, self.last_taa_color, "previousColor")
            tp.set_texture_uniform(GL_TEXTURE_2D, g["velocity"], "velocityTexture")
            tp.set_texture_uniform(GL_TEXTURE_2D, g["normal_depth"], "normal_depth")
            tp.set_uniform_uint("frameCounter", self.camera.frameCounter)
            self._draw(tp, "taa")
        nf = self.next_frame_input                             # main.cpp:546-553
        nf.reset_texture_slot()
        nf.set_texture_uniform(GL_TEXTURE_2D, self.next_frame_color_input, "texPass0")
        nf.set_texture_uniform(GL_TEXTURE_2D, g["normal_depth"], "texPass1")
        nf.set_texture_uniform(GL_TEXTURE_2D, self.curMomentHistory, "texPass2")
        nf.set_texture_uniform(GL_TEXTURE_2D, self.curColor, "accColor")
        nf.set_texture_uniform(GL_TEXTURE_2D, self.taa_output, "taaOutput")
        self._draw(nf, "copy")
        self.final = self.taa_output if self.run_taa else self.modulate_color

    def _front_fast(self) -> dict:
        """G-buffer + path tracer of frame f (the front end); returns what its back end needs."""
        f = self.frame_index
        ng = len(self.gbuf)
        s = f % len(self.pt_slots)
        self._use_slot(s)
        done = None
        t_cam = None
        if self.latency_events is not None and self.K > 1:
            # camera time: an event on a stream nothing else uses completes as soon as it is issued, so its timestamp is
            # the moment this frame's camera went to the GPU (a busy front-end stream would record it later)
            import torch

            if self._clock is None:
                self._clock = acquire_stream()
            t_cam = torch.cuda.Event(enable_timing=True)
            t_cam.record(self._clock)
        if self.K > 1:                                         # front end on stream s, after SVGF(f - K)
            import torch

            fe = self._streams[f % self._nfs]
            if self._slot_free[f % self.K] is not None:
                fe.wait_event(self._slot_free[f % self.K])
            if self.accumulate and self._fe_prev is not None:  # lastFrame = the previous front end's colour
                fe.wait_event(self._fe_prev)
            self._ready = None
            self._stream_to(fe)
            self._gbuffer_and_pt(f % ng)
            done = torch.cuda.Event()
            done.record(fe)
            self._fe_prev = done
            if self._batching():  # the path tracer waits for its batch; the back end for the batch's draw
                holder = {}
                self._batch.append((self.pt_pass, done, fe, holder))
                done = holder
                if len(self._batch) == self.B:
                    self._issue_batch()
        else:
            self._gbuffer_and_pt(f % ng)
        return dict(f=f, slot=s, done=done, ready=self._ready, frame_counter=self.camera.frameCounter, t_cam=t_cam)

    def _back_fast(self, ctx: dict):
        """The SVGF chain of the frame whose front end made ctx (back-end stream, sequential over frames)."""
        cfg = self.cfg
        f = ctx["f"]
        b = f & 1                                              # history parity (back end, sequential)
        pb = 1 - b
        ng = len(self.gbuf)
        g, gp = self.gbuf[f % ng], self.gbuf[(f - 1) % ng]
        _, (color, emission, albedo) = self.pt_slots[ctx["slot"]]
        self.back_set = f % ng
        if self.K > 1:
            done = ctx["done"]
            if isinstance(done, dict):  # batched path tracer: its batch must have been drawn
                if "ev" not in done:
                    self._issue_batch()
                done = done["ev"]
            self._back.wait_event(done)
            if ctx.get("ready") is not None:  # pt_source: the colour / emission / albedo planes have arrived
                if "ev" not in ctx["ready"]:
                    raise RuntimeError(f"pt_source has not delivered frame {f} by its back end (back_lag too small)")
                self._back.wait_event(ctx["ready"]["ev"])
            self._stream_to(self._back)
            if self.back_events is not None:  # diagnostics: when each frame's SVGF chain starts and ends on its stream
                import torch

                e0 = torch.cuda.Event(enable_timing=True)
                e0.record(self._back)
                self.back_events.append([e0, None])
        self._halo("reproject", {"prev_illum": self.hist_illum[pb], "prev_moments": self.moments[pb],
                                 "prev_nd": gp["normal_depth"]})
        rp = self.reproject[b]
        rp.reset_texture_slot()
        rp.set_uniform_float("depth_threshold", cfg.reproj_depth_threshold)
        rp.set_uniform_float("normal_threshold", cfg.reproj_normal_threshold)
        rp.set_texture_uniform(GL_TEXTURE_2D, g["velocity"], "gMotion")
        rp.set_texture_uniform(GL_TEXTURE_2D, color, "gColor")
        rp.set_texture_uniform(GL_TEXTURE_2D, albedo, "gAlbedo")
        rp.set_texture_uniform(GL_TEXTURE_2D, emission, "gEmission")
        rp.set_texture_uniform(GL_TEXTURE_2D, self.hist_illum[pb], "gPrevIllum")
        rp.set_texture_uniform(GL_TEXTURE_2D, self.moments[pb], "gPrevMoments_HistoryLength")
        rp.set_texture_uniform(GL_TEXTURE_2D, g["normal_depth"], "gNormalAndLinearZ")
        rp.set_texture_uniform(GL_TEXTURE_2D, gp["normal_depth"], "gPrevNormalAndLinearZ")
        rp.set_texture_uniform(GL_TEXTURE_2D, g["fwidth"], "gNormalDepthFwidth")
        if self._sm_on:
            rp.set_texture_uniform(GL_TEXTURE_2D, self._sm[ctx["slot"]], "gSampleMoments")
        self._rows(rp, "reproject")
        self._draw(rp, "reproject")
        self._halo("variance", {"illum": self.illum, "moments": self.moments[b], "nd": g["normal_depth"]})
        vp = self.variance_compute_pass
        vp.reset_texture_slot()
        vp.set_uniform_float("gPhiColor", cfg.sigma_l)
        vp.set_uniform_float("gPhiNormal", cfg.sigma_n)
        vp.set_texture_uniform(GL_TEXTURE_2D, self.illum, "gIllumination")
        vp.set_texture_uniform(GL_TEXTURE_2D, self.moments[b], "gMoments_HistoryLength")
        vp.set_texture_uniform(GL_TEXTURE_2D, g["normal_depth"], "gNormalAndLinearZ")
        vp.set_texture_uniform(GL_TEXTURE_2D, g["fwidth"], "gNormalDepthFwidth")
        if self._sm_on:
            vp.set_texture_uniform(GL_TEXTURE_2D, self._sm[ctx["slot"]], "gSampleMoments")
        self._rows(vp, "variance")
        self._draw(vp, "variance")
        # a-trous chain without copies: i0 var->ping, i1 ping->hist[b] (next frame's history),
        # then alternate through ping/pong
        src = self.var_out
        hist_key = "hist0" if b == 0 else "hist1"
        dests = []
        n = cfg.num_atrous_iterations
        for i in range(n):
            if i == 1:
                dests.append(hist_key)
            else:
                prev_tex = None if not dests else self._atrous_tex(dests[-1])
                dests.append("pong" if prev_tex == self.ping else "ping")
        self._atrous_last = (g, [(dests[i], 1 << i) for i in range(n)], src)
        fused = self.fuse_modulate and n > 0
        for i in range(n):
            self._halo(f"atrous{i}", {"atrous_in": src})
            last = fused and i == n - 1
            ap = (self.atrous_mod_to if last else self.atrous_to)[dests[i]]
            ap.reset_texture_slot()
            if last:
                ap.set_texture_uniform(GL_TEXTURE_2D, albedo, "gAlbedo")
                ap.set_texture_uniform(GL_TEXTURE_2D, emission, "gEmission")
            ap.set_uniform_float("gPhiColor", cfg.sigma_l)
            ap.set_uniform_float("gPhiNormal", cfg.sigma_n)
            ap.set_uniform_int("gStepSize", 1 << i)
            ap.set_uniform_int("exact", int(self.atrous_exact))
            ap.set_texture_uniform(GL_TEXTURE_2D, g["normal_depth"], "gNormalAndLinearZ")
            ap.set_texture_uniform(GL_TEXTURE_2D, g["fwidth"], "gNormalDepthFwidth")
            ap.set_texture_uniform(GL_TEXTURE_2D, src, "gIllumination")
            self._rows(ap, "atrous")
            self._draw(ap, "atrous_modulate" if last else "atrous")
            src = self._atrous_tex(dests[i])
            if i == 1 and self._early_history is not None:  # the next frame's history is written
                nxt = self._pending[0] if self._pending and self._pending[0]["f"] == f + 1 else None
                with self._on_back():
                    self._early_history({"prev_illum": self.hist_illum[b], "prev_moments": self.moments[b],
                                         "prev_nd": g["normal_depth"]}, None if nxt is None else (f + 1) % ng)
        self.atrous_final = src
        if not fused:
            mp = self.svgf_modulate_pass
            mp.reset_texture_slot()
            mp.set_texture_uniform(GL_TEXTURE_2D, albedo, "gAlbedo")
            mp.set_texture_uniform(GL_TEXTURE_2D, emission, "gEmission")
            mp.set_texture_uniform(GL_TEXTURE_2D, src, "gIllumination")
            mp.set_texture_uniform(GL_TEXTURE_2D, g["normal_depth"], "gNormalAndLinearZ")
            self._rows(mp, "modulate")
            self._draw(mp, "modulate")
        if self.run_taa:
            self._halo("taa", {"modulate": self.modulate_color, "velocity": g["velocity"], "prev_taa": self.taa[pb]})
            tp = self.pass_taa[b]
            tp.reset_texture_slot()
            tp.set_texture_uniform(GL_TEXTURE_2D, self.modulate_color, "currentColor")
            tp.set_texture_uniform(GL_TEXTURE_2D, self.taa[pb], "previousColor")
            tp.set_texture_uniform(GL_TEXTURE_2D, g["velocity"], "velocityTexture")
            tp.set_texture_uniform(GL_TEXTURE_2D, g["normal_depth"], "normal_depth")
            tp.set_uniform_uint("frameCounter", ctx["frame_counter"])
            self._rows(tp, "taa")
            self._draw(tp, "taa")
        self.final = self.taa[b] if self.run_taa else self.modulate_color

    def _rows(self, p: RenderPass, stage: str) -> None:
        if self._stage_rows is not None:
            rows = self._stage_rows(stage)
            if rows is not None:
                p.set_rows(*rows)

    def time_atrous(self, reps: int = 20) -> float:
        """Average duration (ms) of one a-trous launch: the last frame's iterations (same inputs, so the
        replay rewrites the same bits) issued `reps` times back to back between two HIP events on the
        library's stream, kernels alone on the GPU (everything in flight is drained first). Fast driver."""
        import torch

        self.flush()
        g, iters, src0 = self._atrous_last
        stream = self._back if self.K > 1 else self._serial_stream
        torch.cuda.synchronize()
        self._stream_to(stream)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def once():
            src = src0
            for key, step in iters:
                ap = self.atrous_to[key]
                ap.set_uniform_int("gStepSize", step)
                ap.set_texture_uniform(GL_TEXTURE_2D, src, "gIllumination")
                ap.draw()
                src = self._atrous_tex(key)

        once()  # warm
        e0.record(stream)
        for _ in range(reps):
            once()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / (reps * len(iters))

    STAT_KEYS = ("primary_rays", "primary_visits", "bounce_rays", "bounce_visits", "shadow_rays", "shadow_visits",
                 "tie_rewalks", "primary_retries", "spills", "primary_slots", "bounce_slots",
                 "shadow_slots", "shadow_point_rays", "shadow_occluded")  # pt_pass_set_trace_stats order (pt_device.h kStat*)
    # the counters after those (pt_trace_stats_total): point-light rays decided by the lights' triangle bins / walked
    STAT_KEYS_POINT_BINS = ("shadow_point_binned", "shadow_point_fallback")

    def trace_stats(self) -> dict:
        """Render one frame with the path tracer's traversal counters on (pt_pass_set_trace_stats): rays traced and
        node + triangle visits per traversal kind. Synchronises; diagnostics, not for timed frames."""
        import torch

        keys = self.STAT_KEYS + self.STAT_KEYS_POINT_BINS
        buf = torch.zeros(len(keys), dtype=torch.int64, device="cuda")
        self.flush()  # frames already issued are not counted
        torch.cuda.synchronize()
        for p, _ in self.pt_slots:
            p.set_trace_stats(buf.data_ptr(), buf.numel())
        try:
            self.frame()
            self._issue_batch()  # this frame alone
            torch.cuda.synchronize()
        finally:
            for p, _ in self.pt_slots:
                p.set_trace_stats(0)
        return dict(zip(keys, (int(v) for v in buf.cpu().tolist())))

    def latency_ms(self) -> float | None:
        """Mean camera-to-modulate latency (ms) of the frames recorded since latency_events was set to a list: from
        the moment a frame's camera went to the GPU to the end of its SVGF chain (flushes and synchronises)."""
        import torch

        self.flush()
        torch.cuda.synchronize()
        ev = self.latency_events or []
        return sum(a.elapsed_time(b) for a, b in ev) / len(ev) if ev else None

    def _stream_to(self, stream) -> None:
        """Issue the following draws on this torch stream."""
        _set_stream(stream)
        self._lib_stream = stream

    def _on_back(self):
        """Context: torch's current stream = the back end's (exchanges issue on the current stream)."""
        import contextlib

        if self.K > 1:
            import torch

            return torch.cuda.stream(self._back)
        return contextlib.nullcontext()

    def _halo(self, stage: str, handles: dict) -> None:
        if self._halo_cb is None:
            return
        stages = getattr(self._halo_cb, "stages", None)  # the stages the callback acts on (None: all)
        if stages is not None and stage not in stages:
            return  # (a stream context per stage costs host time on every frame)
        with self._on_back():
            self._halo_cb(stage, handles)

    def _draw(self, p: RenderPass, name: str) -> None:
        p.draw()
        if self._profile:
            self._times.setdefault(name, []).append(p.last_ms())

    def profile(self, on: bool) -> None:
        """Time every draw with HIP events (synchronises after each draw: diagnostics only)."""
        gl.set_profiling(on)
        self._profile = on
        self._times = {}

    def pass_times(self) -> dict:
        """Per-pass ms of the profiled frames (sum per frame) + the a-trous per-launch average."""
        out = {k: float(np.sum(v)) for k, v in self._times.items()}
        if self._times.get("atrous"):
            out["atrous_avg_ms"] = float(np.mean(self._times["atrous"]))
        out["frame_sum_ms"] = float(sum(np.sum(v) for k, v in self._times.items()))
        return out

    def _atrous_tex(self, key: str) -> int:
        return {"ping": self.ping, "pong": self.pong, "hist0": self.hist_illum[0], "hist1": self.hist_illum[1]}[key]

    def frame(self) -> None:
        """One iteration of main.cpp's while-loop body (436-602), headless (with back_lag D: this frame's front
        end and frame f - D's back end)."""
        if self.host_pace and self._slot_free[self.frame_index % self.K] is not None:
            t0 = time.perf_counter()
            self._slot_free[self.frame_index % self.K].synchronize()  # before the camera is read (host_pace)
            self.pace_wait_s += time.perf_counter() - t0
        self.camera.update()
        if self._serial_stream is not None:
            self._stream_to(self._serial_stream)
        if self.mode == "reference":
            self._frame_reference()
            self._finish(None)
        else:
            self._pending.append(self._front_fast())
            while len(self._pending) > self.lag:
                self._finish(self._pending.pop(0))
        # main.cpp:599-600: pre_viewproj = projection * inverse(cameraRotate) = projection * view
        self.pre_viewproj = mat_mul(self.camera.cam_proj_mat, self.camera.cam_view_mat)
        self.camera.frameCounter += 1
        self.frame_index += 1

    def flush(self) -> None:
        """Issue the open path-tracing batch and the back ends still pending (back_lag)."""
        self._issue_batch()
        if self._pt_flush is not None:
            self._pt_flush()
        while self._pending:
            self._finish(self._pending.pop(0))

    def _finish(self, ctx) -> None:
        """Back end (fast driver) + output pass of one frame; then its frame slot is free for frame f + K."""
        f = self.frame_index if ctx is None else ctx["f"]
        if ctx is not None:
            self._back_fast(ctx)
        if self.run_output:                                    # main.cpp:556-590 (final view)
            op = self.output_pass
            op.reset_texture_slot()
            op.set_uniform_bool("accumulate", self.cfg.accumulate_color)
            op.set_texture_uniform(GL_TEXTURE_2D, self._view_plane(f), "texPass0")
            self._draw(op, "output")
        if self.K > 1:  # the slot's buffers are free again once this frame's back end has run
            import torch

            ev = torch.cuda.Event()
            ev.record(self._back)
            if self.back_events is not None and ctx is not None:
                e1 = torch.cuda.Event(enable_timing=True)
                e1.record(self._back)
                self.back_events[-1][1] = e1
            if self.latency_events is not None and ctx is not None and ctx.get("t_cam") is not None:
                e1 = torch.cuda.Event(enable_timing=True)
                e1.record(self._back)
                self.latency_events.append((ctx["t_cam"], e1))
            self._slot_free[f % self.K] = ev

    # --------------------------------------------------------- accessors ---
    def rebuild_bvh(self, tri_enc=None, raster=None, leaf_n: int = 3, ploc_radius: int = 32, prev_raster=None,
                    raster_obj=None):
        """Dynamic scenes: rebuild the path tracer's BVH on the GPU (pt_bvh_build) into the scene
        buffers the passes are bound to. `tri_enc` (Triangle_encoded rows, any order; default: the scene's
        triangles) carries moved vertices; `raster` (the pre-BVH vertex list, obj_loader.h:143-160) moves the
        G-buffer's triangles with them; ploc_radius > 0 rebuilds the tree above the LBVH leaves by PLOC (0: the plain
        LBVH). Defaults: the fastest 4K walk measured (tools/dyn_sweep.py: leaves of <= 3, radius 32: 160 fps, against
        146 for 8 / 16 and 126 for the plain LBVH; all over the binary walk). The build also derives the walk trees on
        the device, among them the 4-wide tree the path tracer then walks (set_lbvh_wide; DESIGN.md "Dynamic scenes").
        `prev_raster` (with `raster`: the vertex list the same triangles had one frame ago, or True for the list of
        the previous rebuild_bvh call) gives the next frame object motion vectors (pt_raster_pass_set_prev_vertices):
        the first frame issued after the rebuild draws its G-buffer with object_motion = 1, so SVGF and TAA fetch a
        moved object's history from where it was; later frames draw with 0 (the geometry is stationary again, the
        planes those of a plain bind). `self.object_motion = False` keeps every frame at 0.
        What this call receives is also the rest pose of pose_objects: `tri_enc`, `raster` and `raster_obj` (one
        object index per raster triangle; default: the scene's raster_obj); a pose of an earlier call is released.
        Frames already issued finish first. Returns (nodes, device ms, that derivation included)."""
        if self._streams is not None:
            import torch

            self.flush()
            torch.cuda.synchronize()
        self._drop_pose()  # the order changes
        rest = np.asarray(self.scene.tri_enc if tri_enc is None else tri_enc, np.float32)
        src = gl.texture_buffer(rest)
        try:
            nodes, ms = gl.bvh_build(src, self.trianglesTextureBuffer, self.nodesTextureBuffer, leaf_n, ploc_radius)
        finally:
            gl.destroy_texture(src)
        self._pose_rest = (rest, None if raster is None else np.ascontiguousarray(raster, np.float32).reshape(-1),
                           self.scene.raster_obj if raster_obj is None else raster_obj)
        for p, _ in self.pt_slots:
            p.set_uniform_int("nNodes", nodes)
        if raster is not None:
            # the G-buffer passes: trees built on the GPU from one device copy; a plain LBVH, since the tile-binned
            # rasteriser walks it only when a tile list overflows
            import torch

            cur = np.ascontiguousarray(raster, np.float32).reshape(-1)
            if prev_raster is True:
                prev_raster = self._last_raster
            self._last_raster = cur
            v = torch.from_numpy(cur).cuda()
            torch.cuda.synchronize()
            self.init_pass[0].rebind_vertices_device(v.data_ptr(), v.numel(), 0)  # drops displacement records
            self._motion_records = self._motion_pending = False
            if prev_raster is not None:
                pv = torch.from_numpy(np.ascontiguousarray(prev_raster, np.float32).reshape(-1)).cuda()
                torch.cuda.synchronize()
                self.init_pass[0].set_prev_vertices(pv.data_ptr(), v.data_ptr(), v.numel())
                self._motion_records = self._motion_pending = True
            for p in self.init_pass[1:]:  # the other G-buffer sets draw the same triangles: one tree
                p.share_vertices(self.init_pass[0])
        return nodes, ms

    def refit_bvh(self, tri_enc, raster=None, prev_raster=None) -> float:
        """Dynamic scenes, geometry that moved but kept its triangles and their order (deformation, rigid motion):
        refit the tree rebuild_bvh built instead of building another (pt_bvh_refit). `tri_enc` holds the scene's
        Triangle_encoded rows in the order of that rebuild_bvh call's rows, at the new positions; the topology stays
        and every box is recomputed, so nNodes does not change. `raster` (the vertex list at the new positions, same
        triangles, same order) refits the G-buffer pass rebuild_bvh(raster=...) bound on the device
        (pt_raster_pass_refit_device); `prev_raster` arms object motion vectors for exactly the next frame, as in
        rebuild_bvh (True: the list of the previous rebuild_bvh / refit_bvh call). A refitted tree keeps the
        topology chosen for the old positions: rebuild once the geometry has moved far (DESIGN.md "Refit").
        Frames already issued finish first. Returns the device ms of the path tracer's refit, the walk trees'
        derivation included. Raises PtError (PT_ERR_STATE) when the scene buffers are not rebuild_bvh's."""
        from ._lib import PtError

        if self._streams is not None:
            import torch

            self.flush()
            torch.cuda.synchronize()
        self._drop_pose()  # its current list would no longer be the pass's: pose_objects needs a rebuild_bvh first
        src = gl.texture_buffer(np.asarray(tri_enc, np.float32))
        try:
            ms = gl.bvh_refit(src, self.trianglesTextureBuffer, self.nodesTextureBuffer)
        except PtError as e:
            if e.code == -9:  # PT_ERR_STATE
                raise PtError(e.code, "refit_bvh: the scene buffers were not built by rebuild_bvh (call it once "
                                      "before the first refit, and again after a change of topology)") from e
            raise
        finally:
            gl.destroy_texture(src)
        if raster is not None:
            import torch

            cur = np.ascontiguousarray(raster, np.float32).reshape(-1)
            if prev_raster is True:
                prev_raster = self._last_raster
            self._last_raster = cur
            v = torch.from_numpy(cur).cuda()
            torch.cuda.synchronize()
            self.init_pass[0].refit_vertices_device(v.data_ptr(), v.numel())  # drops displacement records
            self._motion_records = self._motion_pending = False
            if prev_raster is not None:
                pv = torch.from_numpy(np.ascontiguousarray(prev_raster, np.float32).reshape(-1)).cuda()
                torch.cuda.synchronize()
                self.init_pass[0].set_prev_vertices(pv.data_ptr(), v.data_ptr(), v.numel())
                self._motion_records = self._motion_pending = True
        return ms

    _NOT_REBUILT = ("the scene buffers were not built by rebuild_bvh (call it once before the first refit, and again "
                    "after a change of topology)")

    def _drop_pose(self) -> None:
        """Release the pose and forget its rest pose (rebuild_bvh sets a new one)."""
        if getattr(self, "_pose", None):
            gl.pose_destroy(self._pose)
        self._pose = None
        self._pose_rest = None
        self._skin = None
        self._skin_set = False

    def _ensure_pose(self) -> None:
        """The pose over the rest lists of the last rebuild_bvh, created at the first call that needs it."""
        if self._pose is None:
            rest, raster, raster_obj = self._pose_rest
            if raster is not None and raster_obj is None:
                # only pose_objects reads the objects, and it refuses a raster list without them: none is named
                raster_obj = np.full(raster.size // 18, -1, np.int32)
            src = gl.texture_buffer(rest)
            try:
                self._pose = gl.pose_create(src, raster, raster_obj)
            finally:
                gl.destroy_texture(src)

    def pose_objects(self, mats, motion: bool = True) -> float:
        """Dynamic scenes, rigid (or any affine) motion of whole objects: place every object by one matrix, on the
        device (pt_pose_apply). `mats` is {obj_index: 4x4 or 16 floats} or an (n_obj, 16) array, the floats glm
        column-major as scene.transform returns them; objects not named keep the identity. Matrices are absolute:
        each call poses the rest pose, which is what the last rebuild_bvh call received (its tri_enc, its raster, its
        raster_obj), so posing with identities restores it bit for bit. Positions are transformed by glm's
        mat4 * vec4, normals by the normalised cofactor matrix (tests/pose_ref.py; DESIGN.md "Posed objects").
        The path tracer's tree is refitted as refit_bvh would with the posed rows; if rebuild_bvh was given a `raster`,
        the G-buffer pass is refitted with the posed vertex list, and with `motion` (and self.object_motion) the next
        frame gets object motion vectors from the previous pose to this one, as refit_bvh(prev_raster=True) arms them.
        No vertex data crosses the bus and the call synchronises once. The first call after a rebuild_bvh creates the
        pose (one upload of the rest lists); rebuild_bvh, refit_bvh and close() release it. Mixing with refit_bvh
        needs a rebuild_bvh in between: after a refit_bvh this raises until rebuild_bvh has run again.
        Like a refitted tree, a posed one keeps the topology chosen for the rest pose; there is no rebuild policy
        for poses far from it (compare `frame alone` against a fresh rebuild_bvh, DESIGN.md "Refit").
        Frames already issued finish first. Returns the device ms of the pose: both pose kernels, both refits and
        the walk trees' derivation. Raises PtError (PT_ERR_STATE) when rebuild_bvh has not run."""
        from ._lib import PtError

        if getattr(self, "_pose_rest", None) is None:
            raise PtError(-9, "refit_bvh: " + self._NOT_REBUILT)
        rest, raster, raster_obj = self._pose_rest
        if isinstance(mats, dict):
            n_obj = max([int(k) for k in mats] + [0]) + 1
            if raster_obj is not None and len(raster_obj):
                n_obj = max(n_obj, int(np.max(raster_obj)) + 1)
            table = np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (n_obj, 1))
            for k, m in mats.items():
                if int(k) < 0:
                    raise ValueError("pose_objects: negative object index")
                table[int(k)] = np.asarray(m, np.float32).reshape(16)
        else:
            table = np.ascontiguousarray(mats, np.float32).reshape(-1, 16)
        if self._streams is not None:
            import torch

            self.flush()
            torch.cuda.synchronize()
        if raster is not None and raster_obj is None:
            raise ValueError("pose_objects: no raster_obj (Scene.raster_obj or rebuild_bvh(raster_obj=...))")
        self._ensure_pose()
        raster_pass = 0 if raster is None else self.init_pass[0]._handle()
        arm = bool(motion) and raster is not None
        try:
            ms = gl.pose_apply(self._pose, table, self.trianglesTextureBuffer, self.nodesTextureBuffer, raster_pass, arm)
        except PtError as e:
            if e.code == -9:  # PT_ERR_STATE
                raise PtError(e.code, "refit_bvh: " + self._NOT_REBUILT) from e
            raise
        if raster is not None:
            self._motion_records = self._motion_pending = arm
        return ms

    def set_skin(self, tri_bones, tri_weights, raster_bones=None, raster_weights=None) -> None:
        """The skin of skin_objects: four bone indices (uint16) and four weights (float32) per corner, as arrays of
        12 entries per row of the rest `tri_enc` the last rebuild_bvh received (3 corners x 4) and, if that call got a
        `raster`, 12 per raster triangle (required then, refused otherwise). Weights are not normalised; unused slots
        carry weight 0 and any valid index; a corner whose weights are all 0 stays where the rest pose has it
        (ptsvgf.skin.chain_weights makes such arrays for a bending chain). Valid after a rebuild_bvh; kept with the
        rest pose and dropped wherever it is dropped (rebuild_bvh, refit_bvh, close); a second call replaces it.
        Raises PtError (PT_ERR_STATE) when rebuild_bvh has not run."""
        from ._lib import PtError

        if getattr(self, "_pose_rest", None) is None:
            raise PtError(-9, "refit_bvh: " + self._NOT_REBUILT)
        rest, raster, _ = self._pose_rest

        def pair(bones, weights, ntris, what):
            b = np.asarray(bones)
            if b.size and (b.min() < 0 or b.max() > 0xFFFF):
                raise ValueError(f"set_skin: {what} bone index outside uint16")
            b = np.ascontiguousarray(b, np.uint16).reshape(-1)
            w = np.ascontiguousarray(weights, np.float32).reshape(-1)
            if b.size != ntris * 12 or w.size != ntris * 12:
                raise ValueError(f"set_skin: {b.size} bones and {w.size} weights for {ntris} {what} triangles "
                                 "(12 each per triangle)")
            return b, w

        if (raster is None) != (raster_bones is None) or (raster is None) != (raster_weights is None):
            raise ValueError("set_skin: raster_bones and raster_weights are required exactly when rebuild_bvh got a "
                             "raster list")
        skin = pair(tri_bones, tri_weights, rest.size // 45, "scene")
        if raster is not None:
            skin += pair(raster_bones, raster_weights, raster.size // 18, "raster")
        self._skin = skin
        self._skin_set = False

    def skin_objects(self, bones, motion: bool = True) -> float:
        """Dynamic scenes, geometry that deforms but keeps its topology: linear blend skinning on the device
        (pt_pose_apply_skin). `bones` is an (n_bones, 16) array (or n_bones 4x4s) of glm column-major matrices as
        scene.transform returns them, n_bones above every index set_skin received. Every corner is placed by the
        blend of its four bones, M = ((w0 B0 + w1 B1) + w2 B2) + w3 B3 over the 12 affine floats; positions go through
        M, normals through its normalised cofactor matrix (tests/skin_ref.py; DESIGN.md "Skinned objects"). Matrices
        are absolute: each call skins the rest pose of the last rebuild_bvh. Everything after the vertices is
        pose_objects': the refits, the G-buffer pass, the object motion vectors of the next frame (`motion`), one
        synchronisation, no vertex data over the bus; the two calls may alternate. The first call after a
        rebuild_bvh creates the pose and uploads the skin once. Frames already issued finish first. Returns the
        device ms: both skin kernels, both refits and the walk trees' derivation. Raises PtError (PT_ERR_STATE) when
        rebuild_bvh or set_skin has not run."""
        from ._lib import PtError

        if getattr(self, "_pose_rest", None) is None:
            raise PtError(-9, "refit_bvh: " + self._NOT_REBUILT)
        if self._skin is None:
            raise PtError(-9, "skin_objects: no skin (call set_skin after rebuild_bvh)")
        raster = self._pose_rest[1]
        table = np.ascontiguousarray(bones, np.float32).reshape(-1, 16)
        if self._streams is not None:
            import torch

            self.flush()
            torch.cuda.synchronize()
        self._ensure_pose()
        if not self._skin_set:
            gl.pose_set_skin(self._pose, *self._skin)
            self._skin_set = True
        raster_pass = 0 if raster is None else self.init_pass[0]._handle()
        arm = bool(motion) and raster is not None
        try:
            ms = gl.pose_apply_skin(self._pose, table, self.trianglesTextureBuffer, self.nodesTextureBuffer,
                                    raster_pass, arm)
        except PtError as e:
            if e.code == -9:  # PT_ERR_STATE
                raise PtError(e.code, "refit_bvh: " + self._NOT_REBUILT) from e
            raise
        if raster is not None:
            self._motion_records = self._motion_pending = arm
        return ms

    def set_lbvh_wide(self, on: bool) -> None:
        """Pass uniform lbvh_wide on every path-tracing slot: whether a scene rebuild_bvh built is walked through
        the 4-wide tree derived with it (the default) or through its binary tree alone. Same image either way."""
        for p, _ in self.pt_slots:
            p.set_uniform_int("lbvh_wide", 1 if on else 0)

    def close(self) -> None:
        """Release every pass and texture this renderer created (the GL objects main.cpp never frees)."""
        if self._streams is not None:
            import torch

            torch.cuda.synchronize()  # frames may still be in flight on the renderer's streams
            for st in self._streams + [self._back] + ([self._clock] if self._clock is not None else []):
                release_stream(st)
            self._streams = []
            self._back = None
            self._clock = None
        for v in list(vars(self).values()):
            if isinstance(v, PassGroup):
                continue  # its passes are the pt_slots' (destroyed below)
            for q in (v if isinstance(v, list) else list(v.values()) if isinstance(v, dict) else [v]):
                if isinstance(q, tuple):
                    q = q[0]  # pt_slots entries: (pass, outputs)
                if isinstance(q, RenderPass):
                    q.destroy()
        self._drop_pose()
        for t in self._owned:
            gl.destroy_texture(t)
        self._owned = []

    def planes(self) -> dict:
        """Handles of the last frame's per-pass outputs (for readback / tests); issues pending back ends first."""
        self.flush()
        return self._planes_of(self.frame_index - 1)

    def _planes_of(self, f: int) -> dict:
        if self.mode == "reference":
            g = self.gbuf[0]
            return dict(world=g["world"], normal_depth=g["normal_depth"], velocity=g["velocity"], fwidth=g["fwidth"],
                        color=self.curColor, emission=self.Emission, albedo=self.Albedo,
                        reproj_illum=self.curIllumination, reproj_moments=self.curMomentHistory,
                        variance=self.variance_compute_illumination, atrous=self.atrous_output,
                        history_illum=self.lastIllumination, modulate=self.modulate_color, final=self.final,
                        output=self.output_tex)
        b = f & 1
        g = self.gbuf[f % len(self.gbuf)]
        _, (color, emission, albedo) = self.pt_slots[f % len(self.pt_slots)]
        return dict(world=g["world"], normal_depth=g["normal_depth"], velocity=g["velocity"], fwidth=g["fwidth"],
                    color=color, emission=emission, albedo=albedo, reproj_illum=self.illum,
                    reproj_moments=self.moments[b], variance=self.var_out, atrous=self.atrous_final,
                    history_illum=self.hist_illum[b], modulate=self.modulate_color, final=self.final,
                    output=self.output_tex)
