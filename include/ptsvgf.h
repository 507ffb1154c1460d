/* ptsvgf.h — the drop-in boundary: a C ABI into HIP that replaces the
 * reference's OpenGL plumbing API (layer L2) for the path-tracing + SVGF hot
 * path. A main.cpp-shaped host issues the SAME call sequence it issues against
 * the reference classes; each entry point names the reference interface it
 * replaces (file:line under the reference tree):
 *
 *   getShaderProgram(frag, vert)            Utils/shader.h:21-67    -> pt_program_create
 *   getTextureRGB32F(w, h)                  Utils/help_func.h:22-32 -> pt_texture2d_create
 *   glTexImage2D(... RGB32F ...)            main.cpp:173-180        -> pt_texture2d_upload
 *   glTexBuffer(GL_TEXTURE_BUFFER, RGB32F)  main.cpp:136-168        -> pt_texbuffer_create
 *   glTexStorage3D / glTexSubImage3D        main.cpp:184-205,
 *                                           Utils/help_func.h:4-20  -> pt_texarray_create / _upload_layer
 *   RenderPass{program,colorAttachments,width,height}
 *                                           Utils/render_pass.h:82-90 -> pt_pass_create / _add_color_attachment
 *   RenderPass::bindData(finalPass)         render_pass.h:92-119    -> pt_pass_bind
 *   RenderPass::draw()                      render_pass.h:120-140   -> pt_pass_draw
 *   RenderPass::reset_texture_slot()        render_pass.h:141-143   -> pt_pass_reset_texture_slot
 *   RenderPass::set_texture_uniform(t,tex,n) render_pass.h:144-150  -> pt_pass_set_texture
 *   RenderPass::set_uniform_{mat4,float,int,uint,bool,vec3}
 *                                           render_pass.h:152-180   -> pt_pass_set_uniform_*
 *   Rasterize_RenderPass::bindData(verts)   render_pass.h:19-62     -> pt_raster_pass_bind
 *   Rasterize_RenderPass::draw()            render_pass.h:64-79     -> pt_pass_draw
 *   glUniform*(glGetUniformLocation(...))   main.cpp:223-226,243-247,436-441 -> pt_pass_set_uniform_* (same)
 *   buildBVHwithSAH + node/triangle encode  Utils/BVH.h:42-173, main.cpp:88-151 -> pt_bvh_build (GPU, dynamic
 *                                           scenes: a different tree in the same buffer formats; pt_bvh_refit
 *                                           keeps that tree and moves its boxes)
 *
 * Conventions:
 *  - handles are opaque uint32 owned by the library (0 is never a valid handle);
 *  - every function returns int status: PT_OK (0) or a negative PT_ERR_*;
 *    pt_last_error() gives the message. Where the reference calls exit(-1)
 *    (missing shader file, shader.h:8-12) this returns PT_ERR_FILE instead;
 *  - an unknown uniform name is silently ignored (GL location -1 semantics);
 *  - textures are RGBA32F, row-major, row 0 = GL window row 0 (bottom);
 *  - mat4 arguments are 16 floats column-major (glm::value_ptr order);
 *  - texture targets / formats keep their GL enum values so call sites port 1:1;
 *  - draws are asynchronous on the library stream (GL orders passes the same
 *    way); pt_sync() / pt_texture_readback() synchronise.
 *
 * MI355X extensions (no GL counterpart): pt_init (device + rank), pt_set_stream
 * (run on the caller's HIP stream, e.g. torch's), pt_texture2d_wrap (adopt
 * external device memory), pt_set_band (screen-band sharding across GPUs:
 * textures hold rows [row0, row0+rows) of the global frame).
 */
#ifndef PTSVGF_H
#define PTSVGF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PT_OK 0
#define PT_ERR_INVALID_HANDLE (-1)
#define PT_ERR_UNKNOWN_PROGRAM (-2)
#define PT_ERR_FILE (-3)
#define PT_ERR_MISSING_TEXTURE (-4)
#define PT_ERR_HIP (-5)
#define PT_ERR_ARG (-6)
#define PT_ERR_FORMAT (-7)
#define PT_ERR_NO_DEVICE (-8)
#define PT_ERR_STATE (-9)

/* GL enum values (texture targets and formats) */
#define PT_TEXTURE_2D 0x0DE1
#define PT_TEXTURE_BUFFER 0x8C2A
#define PT_TEXTURE_2D_ARRAY 0x8C1A
#define PT_RGB32F 0x8815
#define PT_RGBA32F 0x8814
#define PT_RGB 0x1907
#define PT_RGBA 0x1908

/* ---- library / device ---------------------------------------------------- */
int pt_init(int device);                    /* select HIP device, create stream */
int pt_shutdown(void);                      /* free every handle and the stream */
int pt_set_stream(void* hip_stream);        /* run on this stream; NULL = HIP default (null) stream */
int pt_use_own_stream(void);                /* back to the library's own stream (the pt_init default) */
/* The caller draws no more on this stream (it may be destroyed, or its handle
 * reused): the library drops its per-stream state (the trace_fork side stream,
 * the merged environment's reader event) once that state's work is done, and
 * falls back to its own stream if this one is current. No GL counterpart. */
int pt_stream_release(void* hip_stream);
/* A new stream whose kernels run only on the CUs whose bits are set in
 * mask[0..words) (hipExtStreamCreateWithCUMask; bit i of word w = CU 32 w + i),
 * e.g. to keep a set of CUs free of long traversal launches for a latency-bound
 * chain on another stream. Destroy with pt_stream_destroy. No GL counterpart. */
int pt_stream_create_cu_masked(uint32_t words, const uint32_t* mask, void** out);
/* A new non-blocking stream at queue priority `priority` (hipStreamCreateWithPriority;
 * numerically lower = higher, clamped into pt_stream_priority_range), e.g. to
 * put long traversal launches below a latency-bound chain. A trace_fork side
 * stream takes its draw stream's priority. Destroy with pt_stream_destroy. */
int pt_stream_create_priority(int priority, void** out);
int pt_stream_priority_range(int* least, int* greatest);
int pt_stream_destroy(void* hip_stream);   /* release (above), wait for its work, destroy */
/* Host-only check of the trees the library derives from a reference tree
 * (node_enc / tri_enc as pts_scene_encode writes them), built with 4-wide
 * collapse mode `collapse` (0..3, PTSVGF_WIDE_COLLAPSE) and `treelet` passes of
 * treelet restructuring (PTSVGF_TREELET). Needs no device and no pt_init.
 * out[0..PT_TREE_CHECK_COUNT): 1/0 every reference-leaf triangle is held by
 * exactly one leaf of the binary any-hit tree / the any-hit 4-wide tree / the
 * closest-hit 4-wide tree (and no other triangle); 1/0 every child box lies
 * inside its parent's box and every leaf box holds its triangles (boxes under a
 * reference leaf's own box excepted: its fine boxes only cull); SAH cost / root
 * area before and after the treelet passes; summed 4-wide node area / root area
 * of the any-hit and closest-hit trees; 4-wide nodes (both trees); binary depth;
 * 4-wide stack need; 1 when the closest-hit tree is a separate one.
 * No GL counterpart: the reference walks its own tree only. */
#define PT_TREE_CHECK_COUNT 12
int pt_tree_check(const float* node_enc, int nnodes, const float* tri_enc, int ntris, int collapse, int treelet,
                  double* out, int nout);
int pt_device_cus(int* n);                 /* compute units of the library's device */
int pt_sync(void);                          /* wait for all queued draws */
const char* pt_last_error(void);
int pt_version(void);

/* Band sharding: this rank renders global rows [y_begin, y_end) of a
 * frame_w x frame_h frame; every 2-D texture of exactly that size created
 * afterwards stores global rows [row0, row0 + rows) (band + ghost rows).
 * Default (never called): one band covering the frame. */
int pt_set_band(int frame_w, int frame_h, int y_begin, int y_end, int row0, int rows);
/* Record HIP events around every draw so pt_pass_last_ms can report it. */
int pt_set_profiling(int on);

/* ---- programs (getShaderProgram) ------------------------------------------- */
/* The fragment shader's basename selects the HIP kernel: path_tracing.frag,
 * svgf_reproject.frag, svgf_variance.frag, svgf_Atrous.frag, svgf_modulate.frag,
 * bilt.frag, save_frame_data.frag, output_pass.frag, taa.frag (full-screen,
 * vert.vert) and rasterize_frag.frag (rasterize_vert.vert). The shader files are
 * not read (the kernels are compiled in); an unknown basename or a mismatched
 * vertex stage returns PT_ERR_UNKNOWN_PROGRAM where the reference exit(-1)s. */
int pt_program_create(const char* frag_path, const char* vert_path, uint32_t* out_program);

/* ---- textures -------------------------------------------------------------- */
int pt_texture2d_create(int width, int height, uint32_t* out_tex);                 /* RGBA32F, zeroed */
int pt_texture2d_upload(uint32_t tex, int width, int height, uint32_t fmt,         /* PT_RGB32F | PT_RGBA32F */
                        const float* host_data);
int pt_texture2d_wrap(void* device_ptr, int width, int height, uint32_t* out_tex); /* RGBA32F, not owned;
    the library does not see writes to wrapped memory: a wrapped hdrMap / hdrCache whose contents change must be
    wrapped again (a new handle) for the path tracer's merged environment to be rebuilt */
int pt_texbuffer_create(const void* host_data, size_t bytes, uint32_t fmt, uint32_t* out_tex); /* RGB32F */
/* Moving point lights (DESIGN.md "Moving point lights"): replaces lights first .. first + count - 1 of the lights
 * texture buffer a path-tracing pass binds as pointLights. A light is 6 floats, position then colour, as in
 * main.cpp's light list. Draws already enqueued, on any stream, still read the values they were enqueued with; draws
 * issued after the call read the new ones. The call does not wait for the device. What was cached per light follows
 * the lights whose position changed bitwise: the triangle bins of such a light are set aside (its shadow rays walk
 * the tree) and rebuilt once it has stood for `point_bins_settle` path-tracing draws (int uniform of the
 * path-tracing pass, >= 0, default 8; 0: at the first draw after the move), and the static view's verdict cache
 * forgets that light alone. A colour-only change invalidates nothing. Same bits as a fresh buffer with these lights.
 * PT_ERR_INVALID_HANDLE: not a texture buffer; PT_ERR_ARG: null data, or a range outside the buffer. */
int pt_lights_update(uint32_t lights_tex, int first, int count, const float* pos_rgb6);
/* Material edits (DESIGN.md "Material edits"): the Triangle_encoded records of objects first_obj .. first_obj +
 * count - 1 in the triangle buffer tri_tex take new materials; material18 holds `count` materials of
 * PTS_MATERIAL_FLOATS (18) floats in ptsvgf_scene.h's order, object first_obj + k takes the k-th. A record belongs
 * to object o when its objIndex (float 42) compares == (float)o; records of no named object keep their bits. Draws
 * issued after the call render, bit for bit, what a library given a triangle buffer with floats 18 .. 35 of those
 * records replaced would render; draws already enqueued, on any stream, read the materials they were enqueued with.
 * The call does not wait for the device and, after the first few, does not allocate. The buffer's version does not
 * advance: walk trees, point-light bins, the primary-hit and verdict caches and a pt_bvh_build pair stay valid; on a
 * standing view each pass's next draw writes its emission and albedo planes in full once. A buffer no draw has
 * decoded yet is no error. pose (0: none): a pt_pose_create handle made from this buffer, whose rest list is patched
 * too; without it the next pt_pose_apply / pt_pose_apply_skin copies the old materials back. pt_bvh_refit copies
 * whatever its tri_in holds: a caller that keeps a rest buffer of its own edits that one as well.
 * PT_ERR_ARG: null material18, count outside [1, 4096], first_obj < 0 or first_obj + count > 2^24, a pose of another
 * triangle count, a buffer that is not whole 45-float records; PT_ERR_INVALID_HANDLE: tri_tex is not a texture
 * buffer, or the pose is unknown. Every check runs before anything is launched or changed. */
int pt_materials_update(uint32_t tri_tex, uint32_t pose, int first_obj, int count, const float* material18);
/* Environment edits (DESIGN.md "Environment edits"): a new map of the same size for the 2-D textures a path-tracing
 * pass binds as hdrMap and hdrCache, with its importance cache built on the device. rgb holds width * height texels
 * of 3 floats in file scanline order, the layout pt_texture2d_upload(.., PT_RGB32F, ..) takes: a host pointer when
 * on_device is 0, else a device pointer (4-byte aligned). Afterwards hdr_tex holds (R, G, B, 1) and cache_tex
 * (x, y, pdf, 1) per texel, bit for bit what pt_texture2d_upload(hdr_tex, rgb) and pt_texture2d_upload(cache_tex,
 * pts_hdr_cache(rgb)) leave, except that a NaN pdf may be another NaN. Draws already enqueued, on any stream, read the
 * environment they were enqueued with (the merged plane of hdr_merge included); draws issued afterwards read the new
 * one. The call does not wait for the device and, after the first few, does not allocate. Host data is consumed
 * before the call returns. Device data is consumed in stream order on the library's current stream: work queued there
 * before the call has produced it, work queued there afterwards may overwrite it. Both textures' versions advance and
 * nothing else does: walk trees, point-light bins, the primary-hit and verdict caches and the G-buffer draw's key stay
 * valid; on a standing view each pass redraws what depends on the miss colour once. pt_texture_readback sees the
 * current version; pt_texture_device_ptr returns its plane, another pointer after every update, whose texels are
 * complete once the device is idle (the builds run on a stream of their own; pt_texture_readback waits for every
 * stream) — the library's draws wait for them themselves. A later
 * pt_texture2d_upload keeps its contract (no draw in flight); pt_texture_destroy of either texture and pt_shutdown
 * free the versions. PT_ERR_ARG: null rgb, hdr_tex == cache_tex, width or height outside [1, 8192], a size other
 * than both textures' (a new size goes through pt_texture2d_upload); PT_ERR_INVALID_HANDLE: not a 2-D texture;
 * PT_ERR_STATE: a wrapped texture, or one that stores a band of its rows. Every check runs before anything is
 * launched or changed. */
int pt_environment_update(uint32_t hdr_tex, uint32_t cache_tex, const void* rgb, int width, int height, int on_device);
/* GPU BVH builder for dynamic scenes. The reference builds once on the host
 * (buildBVHwithSAH, Utils/BVH.h:42-173, main.cpp:88-96) and encodes triangles and nodes (main.cpp:101-151);
 * this builds a Karras LBVH on the device from the DEVICE contents of tri_in (Triangle_encoded texels, e.g.
 * after moving vertices through pt_texture_device_ptr) and writes, in those same formats, the triangles in leaf
 * order into tri_out and BVHNode_encoded nodes (dummy node 0, root node 1, leaves of <= leaf_n triangles) into
 * node_out. ploc_radius > 0 (e.g. 16) rebuilds the tree above the LBVH leaves by PLOC clustering with that search
 * radius (a surface-area-driven top, cheaper to walk); 0 keeps the plain LBVH. tri_out / node_out are existing
 * texbuffers (any size, e.g. created empty), distinct from tri_in and each other; their device and host copies are
 * replaced, so passes bound to them draw the new scene next time. leaf_n in [1, 15], ploc_radius in [0, 256].
 * The walk trees of the new nodes (the packed binary tree, the leaf list and a 4-wide tree) are derived on the device
 * right after the build and kept with node_out, so the first draw over the new buffers packs nothing on the host; a
 * path-tracing pass walks the 4-wide tree unless its int uniform lbvh_wide is 0 (same image either way).
 * out_nodes: node count (dummy included); out_ms: device time of the build, that derivation included (NULL: skipped).
 * Synchronous (waits for the build on the library stream). */
int pt_bvh_build(uint32_t tri_in, int leaf_n, int ploc_radius, uint32_t tri_out, uint32_t node_out, int* out_nodes,
                 float* out_ms);
/* Refit for geometry that moved but kept its triangles and their order (deformation, rigid motion): the topology
 * of a built tree stays, only its boxes are recomputed. tri_out / node_out are the pair one pt_bvh_build call wrote,
 * not written since (refits excepted); tri_in holds as many Triangle_encoded records as that build's tri_in, in its
 * order (vertices and any other field may differ). After the call tri_out = tri_in permuted by the build's leaf
 * order; every node's childs and leafInfo texels are unchanged bit for bit; a leaf's AA / BB are its triangles'
 * min(p1, min(p2, p3)) / max(p1, max(p2, p3)) folded in leaf order from the first (lo = min(lo, lo_t)), an interior
 * node's min / max (left, right) of its children's, glm's min / max throughout (tests/lbvh_refit_ref.py restates
 * it); the dummy node 0 is untouched. Both buffers are written where they lie (no staging copy); their host mirrors
 * are brought up to date when next read. The walk trees are derived again as in pt_bvh_build (a new set replaces the
 * old) and both textures' versions advance, so the next draw decodes the triangles and reads the new trees. The
 * caller has no draw in flight that reads these buffers. Synchronous on the library stream.
 * out_ms: device time, the derivation included (NULL: skipped).
 * PT_ERR_ARG: a handle used twice, a non-texbuffer, tri_in not whole records or another triangle count than the
 * build's. PT_ERR_STATE: tri_out / node_out are not a pair of one pt_bvh_build, or one of them was written by
 * another build or upload since. On either the buffers and their trees are unchanged. */
int pt_bvh_refit(uint32_t tri_in, uint32_t tri_out, uint32_t node_out, float* out_ms);
int pt_texarray_create(int width, int height, int layers, uint32_t* out_tex);     /* RGBA8 2-D array */
int pt_texarray_upload_layer(uint32_t tex, int layer, int width, int height, int channels,
                             const uint8_t* host_data);
int pt_texture_readback(uint32_t tex, float* host_out, size_t bytes);             /* syncs the device */
/* The compact one-float side plane of a 2-D texture's stored rows (width x rows floats): a depth-fwidth attachment's
 * fwidth.y with the background flag in its sign bit; a world-position attachment's primary-ray bound, written by a
 * rasterize draw with the vec3 uniform bound_eye set (+inf: none). *bytes receives its size, 0 when the texture holds
 * none that matches its texels; it is copied to host_out when host_out is not NULL (cap: its room). Syncs the device. */
int pt_texture_readback_aux(uint32_t tex, float* host_out, size_t cap, size_t* bytes);
int pt_texture_upload_rgba(uint32_t tex, const float* host_rgba, size_t bytes);   /* raw RGBA32F rows */
int pt_texture_device_ptr(uint32_t tex, void** out_ptr);
int pt_texture_info(uint32_t tex, int* width, int* height, int* row0);
int pt_texture_destroy(uint32_t tex);

/* ---- ray queries (no GL counterpart) ----------------------------------------- */
/* Closest hit, occlusion and picking for the caller's own rays over the scene in (tri_tex, node_tex): the scene the
 * path-tracing draws of these buffers walk, decoded by the first query or draw and current after pt_bvh_build,
 * pt_bvh_refit, pt_pose_apply and pt_pose_apply_skin (DESIGN.md "Ray queries"; tests/ray_query_ref.py restates the
 * definition).
 * A ray is 8 floats on the device, 16-byte aligned: floats 0-2 the origin S, float 3 ignored, floats 4-6 the
 * direction d, used as given and never normalised (as hitBVH uses ray.direction), float 7 tmax, which only
 * pt_rays_occluded reads. A hit is 32 bytes: {float t; int32 tri; int32 obj; int32 inside; float P[3]; float zero;}.
 *
 * pt_rays_closest: hit i is what hitBVH (path_tracing.frag:372-424) returns for ray i, bit for bit: the least t and,
 * when several triangles attain it, the one the reference's depth-first order meets first. t: hitTriangle's distance;
 * tri: the record's index in tri_tex as the buffer lies now (for a pt_bvh_build pair: in tri_out, leaf order); obj:
 * (int)objIndex of that record (float 42), -1 when that float is not finite or lies outside +-2^24; inside:
 * hitTriangle's isInside; P = S + d * t in float32, one rounding per operation. A miss: t = 114514 (the reference's
 * INF), tri = obj = -1, inside = 0, P = 0. The last float is 0.
 * pt_rays_occluded: byte i is 1 iff ray i's closest hit exists and its t < tmax (in units of t, not of length; a
 * tmax of +inf asks for any hit), else 0.
 * pt_rays_primary: the ray records of the pixels (x, y) given as n int32 pairs in device_xy (8-byte aligned), or with
 * device_xy NULL and n = width * height of every pixel, row-major, row 0 at the bottom: S = eye3, d the path-tracing
 * pass's primary direction for cameraRotate16 (column-major) and aspect_corrected, bit for bit, tmax = +inf, float 3
 * = 0. A pixel outside the frame yields d = 0, a ray that misses everything.
 *
 * All three are asynchronous on the library's current stream, like draws. n == 0 returns PT_OK and launches nothing.
 * Every check runs before anything is launched: PT_ERR_INVALID_HANDLE: tri_tex or node_tex is not a texture buffer;
 * PT_ERR_ARG: a null pointer with n > 0, n < 0 or n > 2^28, a record pointer that is not 16-byte aligned, width or
 * height < 1, a NULL device_xy with n != width * height; and the scene errors a draw reports for these buffers
 * (PT_ERR_FORMAT for a tree deeper than the reference's stack[256]). A query over a tree deeper than the LDS stack
 * grows a scratch buffer before its launch and keeps it until pt_shutdown. A query touches no pass: primary-hit and
 * verdict caches, static-view keys and tile orders stay as they are. A pt_materials_update issued after a query does
 * not disturb it. As for draws, the caller has no query in flight on buffers it hands to pt_bvh_build, pt_bvh_refit,
 * pt_pose_apply or pt_pose_apply_skin. The walks prune with the draws' margins, which are sized for directions of
 * about unit length. */
int pt_rays_closest(uint32_t tri_tex, uint32_t node_tex, const void* device_rays, int64_t n, void* device_hits);
int pt_rays_occluded(uint32_t tri_tex, uint32_t node_tex, const void* device_rays, int64_t n, void* device_u8);
int pt_rays_primary(const float* eye3, const float* cameraRotate16, int width, int height, int aspect_corrected,
                    const int32_t* device_xy, int64_t n, void* device_rays_out);

/* ---- passes (RenderPass / Rasterize_RenderPass) ---------------------------- */
int pt_pass_create(uint32_t program, int width, int height, uint32_t* out_pass);
int pt_pass_add_color_attachment(uint32_t pass, uint32_t tex);
int pt_pass_bind(uint32_t pass, int final_pass);
int pt_raster_pass_bind(uint32_t pass, const float* vertices, size_t n_floats);   /* pos3+nrm3 per vertex */
/* Dynamic scenes: pt_raster_pass_bind from a DEVICE vertex list (same layout), its G-buffer tree built by the GPU
 * builder (LBVH, PLOC top with ploc_radius > 0) and its records decoded on the device; the G-buffer does not depend
 * on the tree (closest t, ties to the lower original index), so the planes equal the host bind's bit for bit. */
int pt_raster_pass_bind_device(uint32_t pass, const void* device_vertices, size_t n_floats, int ploc_radius);
/* Refit of a pass pt_raster_pass_bind_device bound (not sharing), for a DEVICE vertex list of the same triangles in
 * the same order at new positions: the records are decoded again in the bind's leaf order (a record's original index
 * is unchanged), the bind's tree keeps its topology and gets new boxes, and the packed tree is derived from it again.
 * Displacement records are dropped, as a bind drops them (pt_raster_pass_set_prev_vertices sets new ones; its order
 * argument still holds). Passes sharing this pass see the new records. Complete when it returns; no draw of the pass
 * may be in flight. PT_ERR_ARG: another triangle count, a sharing pass, a non-raster pass. PT_ERR_STATE: the pass was
 * bound on the host, or its device bind took the host fallback (a tree too deep for the walk's stack): bind again.
 * On either the pass draws as before. */
int pt_raster_pass_refit_device(uint32_t pass, const void* device_vertices, size_t n_floats);
/* Dynamic scenes, no GL counterpart: the vertex list this (bound, not sharing) rasterize pass's triangles had one
 * frame ago. Both lists are DEVICE pointers in pt_raster_pass_bind's layout with the bound triangle count and order.
 * device_prev = NULL drops the records. While records are bound and the pass's int uniform object_motion is not 0
 * (the default is 1), a surface pixel on a triangle that moved gets motion.xy measured to where its surface point was
 * one frame ago, and motion.z = that point's change of linear depth under pre_viewproj, which svgf_reproject adds to
 * this frame's depth before its history depth test; every other pixel is written as without records. The records
 * are complete when the call returns; a bind drops them; passes sharing this pass's triangles read them too.
 * PT_ERR_ARG for a wrong size, a sharing pass, an unbound pass or a non-raster pass. */
int pt_raster_pass_set_prev_vertices(uint32_t pass, const void* device_prev, const void* device_cur, size_t n_floats);

/* ---- posed objects (dynamic scenes, no GL counterpart) ---------------------- */
/* Rigid (or any affine) motion of whole objects without vertex data crossing the bus: a pose keeps the rest-pose
 * triangles and raster vertices on the device and places them by one matrix per object (tests/pose_ref.py restates
 * it: positions by glm's mat4 * vec4, normals by the normalised cofactor matrix; a record whose objIndex names no
 * object, and every record of an object whose matrix is the identity, keeps its bits).
 * pt_pose_create copies the device contents of the texbuffer tri_rest (whole Triangle_encoded records in the order of
 * the tri_in pt_bvh_build received; the caller may destroy it afterwards), uploads the rest raster list (pos3 + nrm3
 * per vertex, n_floats a multiple of 18) with one object index per raster triangle (pts_scene_raster_objects), and
 * allocates the posed triangle list and two posed raster lists, the current one starting as a copy of the rest list.
 * raster_rest may be NULL with n_floats 0: the pose then serves the path tracer only. Released by pt_pose_destroy
 * and by pt_shutdown. */
int pt_pose_create(uint32_t tri_rest, const float* raster_rest, size_t n_floats, const int* raster_obj,
                   uint32_t* out_pose);
/* Poses the rest lists by mats16 (n_obj in [1, 4096] glm column-major mat4s, object k's at mats16 + 16 k; absolute:
 * every call poses the rest pose) and refits tri_out / node_out exactly as pt_bvh_refit would with the posed list as
 * tri_in (its version, host-mirror and walk-tree rules hold). With raster_pass != 0 the pass is refitted as
 * pt_raster_pass_refit_device would with the newly posed raster list; motion != 0 then binds displacement records
 * from the pose's current list to the new one, as pt_raster_pass_set_prev_vertices(pass, current, new, n) would,
 * motion == 0 leaves the pass without records; the new list becomes the current one. Synchronous on the library
 * stream, one synchronisation in all; the caller has no draw in flight that reads the buffers or the pass.
 * out_ms: device time from the first pose kernel to the end of the tree derivations (NULL: skipped).
 * All checks run before the first launch: on an error the pose, the buffers, their trees and the pass are unchanged.
 * PT_ERR_INVALID_HANDLE: an unknown pose. PT_ERR_ARG: null mats16, n_obj out of range, a handle used twice, a
 * non-texbuffer, raster_pass given for a pose without a raster list, a sharing or non-raster pass, a triangle count
 * that differs from the pose's. PT_ERR_STATE: whatever pt_bvh_refit or pt_raster_pass_refit_device report so. */
int pt_pose_apply(uint32_t pose, const float* mats16, int n_obj, uint32_t tri_out, uint32_t node_out,
                  uint32_t raster_pass, int motion, float* out_ms);
/* Skinned objects: linear blend skinning of the pose's rest lists on the device (tests/skin_ref.py restates it).
 * Every corner (a vertex of a Triangle_encoded record, or of a raster triangle) has four bone indices and four
 * weights; the 12 affine floats of a bone (floats 3, 7, 11, 15 of its mat4 are not read) are blended as
 * M[j] = ((w0 B0[j] + w1 B1[j]) + w2 B2[j]) + w3 B3[j], positions go through M as in a pose and normals through the
 * normalised cofactor matrix of M. Weights are not normalised; unused slots carry weight 0 and any valid index. A
 * corner whose four weights all compare == 0 keeps the bits of its position and normal (a NaN weight is not == 0: that
 * corner is skinned, to NaN). All four terms are always evaluated: a non-finite float in a bone named with weight 0
 * yields NaN. A singular blend gives NaN normals and finite positions.
 * pt_pose_set_skin copies the influences to the device: tri_bones / tri_weights hold 12 entries per record of the
 * pose (3 corners x 4, in the order of its tri_rest), raster_bones / raster_weights 12 per raster triangle; the raster
 * arrays are required exactly when the pose has a raster list (PT_ERR_ARG otherwise, and for null tri arrays). A
 * second call replaces the skin; pt_pose_destroy releases it.
 * pt_pose_apply_skin is pt_pose_apply with bones16 (n_bones in [1, 4096] glm column-major mat4s, absolute: every call
 * skins the rest lists) in place of the object matrices: the same refits, displacement records from whichever list
 * is current, one synchronisation, out_ms from the first skin kernel to the end of the tree derivations. The two
 * calls may alternate on one pose. All checks run before the first launch: on an error the pose, the buffers, their
 * trees and the pass are unchanged. PT_ERR_STATE: the pose has no skin. PT_ERR_ARG: null bones16, n_bones out of range
 * or <= the largest index of the skin. Otherwise whatever pt_pose_apply reports, for the same causes. */
int pt_pose_set_skin(uint32_t pose, const uint16_t* tri_bones, const float* tri_weights,
                     const uint16_t* raster_bones, const float* raster_weights);
int pt_pose_apply_skin(uint32_t pose, const float* bones16, int n_bones, uint32_t tri_out, uint32_t node_out,
                       uint32_t raster_pass, int motion, float* out_ms);
int pt_pose_destroy(uint32_t pose);
/* A rasterize pass drawing another (bound) rasterize pass's triangles and tree: the reference has one G-buffer pass;
 * a driver with several G-buffer targets (frames in flight) binds one and shares it. Rebinding `pass` ends the share;
 * destroying `src_pass` first makes `pass`'s draws fail with PT_ERR_STATE. */
int pt_raster_pass_share(uint32_t pass, uint32_t src_pass);
/* The G-buffer planes of a rasterize pass's attachments were written elsewhere for rows [y_begin, y_end) (multi-GPU:
 * another rank drew these rows of the same frame and sent them; the G-buffer is per pixel, so they equal a draw's):
 * derive what a draw makes beside its planes (the a-trous's compact depth-fwidth plane and per-tile surface flags,
 * "atrous_rows_begin" / "_end" as for a draw) on the current stream. No reference counterpart. */
int pt_raster_pass_adopt(uint32_t pass, int y_begin, int y_end);
/* Tile shard (multi-GPU, no GL counterpart): a path-tracing pass with "tile_stride" = S and "tile_offset" = o draws the
 * 16 x 16 tiles t = k * S + o of its rows, numbered row-major from its first row (tile_y0) with frame_w / 16 tiles per
 * row. pt_tiles_copy moves the pixels of such subsets between textures (RGBA32F, the same width, a multiple of 16) and
 * packed device buffers, one segment per (rows, subset, buffer): unpack = 0 writes the segment's packed block from the
 * textures, 1 writes the textures from it. A block holds, for each texture in order, each row of [y_begin, y_end) in
 * order, each row's subset tiles in x order: pt_tiles_count(...) pixels per texture (16 B each). Asynchronous on the
 * library stream; segment rows must lie in every texture's stored rows. */
typedef struct {
  int y_begin, y_end, offset;
  void* packed;
} PtTileSeg;
int pt_tiles_count(int frame_w, int tile_y0, int stride, int offset, int y_begin, int y_end, int64_t* out_pixels);
int pt_tiles_copy(const uint32_t* tex, int ntex, int tile_y0, int stride, const PtTileSeg* segs, int nseg, int unpack);
int pt_pass_reset_texture_slot(uint32_t pass);
int pt_pass_set_texture(uint32_t pass, uint32_t target, uint32_t tex, const char* name);
int pt_pass_set_uniform_mat4(uint32_t pass, const char* name, const float* m16);
int pt_pass_set_uniform_float(uint32_t pass, const char* name, float v);
int pt_pass_set_uniform_int(uint32_t pass, const char* name, int v);
int pt_pass_set_uniform_uint(uint32_t pass, const char* name, uint32_t v);
int pt_pass_set_uniform_bool(uint32_t pass, const char* name, int v);
int pt_pass_set_uniform_vec3(uint32_t pass, const char* name, const float* v3);
/* Rows this pass computes (global coords); default = the band. The G-buffer
 * pass uses it to compute ghost rows locally for multi-GPU halos. */
int pt_pass_set_rows(uint32_t pass, int y_begin, int y_end);
/* Load-balancing probe (path-tracing pass, wavefront kernel): while set, every
 * draw ADDS the BVH node + triangle visits of each pixel's rays into
 * device_counts[row - y_begin] (uint32 per computed row; caller zeroes it).
 * NULL disables. No reference counterpart (multi-GPU band planning). */
int pt_pass_set_row_cost(uint32_t pass, void* device_counts);
/* Per-pixel sample counts (path-tracing pass, wavefront kernel, spp = N > 1):
 * while set, a draw reads device_u8[y * width + x] (one uint8 per frame pixel,
 * global rows; the caller fills it before the draw on the drawing stream) and
 * takes n = min(max(c, 1), N) samples at that pixel: sample s exists iff
 * s < n, keeps the counter F * N + s, and the colour is the mean of the first
 * n samples in sample order. A sample that does not exist traces no ray.
 * Ignored at spp = 1. NULL unbinds. A draw with the plane bound under an
 * active pt_set_band partition fails with PT_ERR_STATE before it launches
 * anything. No reference counterpart. */
int pt_pass_set_sample_counts(uint32_t pass, void* device_u8);
/* Per-pixel sample statistics (path-tracing pass, wavefront kernel, spp > 1):
 * while set, the resolve of a draw stores for every pixel it resolves the pair
 * device_f32x2[y * width + x] = (m, v): mean and unbiased variance of the
 * luminances (svgf_reproject.frag's) of the pixel's n samples, (l_0, -1) when
 * n < 2. Pixels outside the drawn rows or tile subset keep their contents.
 * Ignored at spp = 1. NULL unbinds. PT_ERR_STATE under an active pt_set_band
 * partition, as above. No reference counterpart. */
int pt_pass_set_sample_stats(uint32_t pass, void* device_f32x2);
/* Per-pixel sample moments for SVGF (path-tracing pass, wavefront kernel,
 * spp = N > 1): while set, the resolve of a draw stores for every pixel it
 * resolves device_f32x4[y * width + x] = (mu, nu, r, float(n)), n the
 * pixel's sample count. With e, a the draw's own emission and albedo texels,
 * illum_s = (c_s.rgb - e.rgb) / max(a.rgb, 0.001) per channel (0 if a channel
 * is NaN) and l_s its luminance (0.2125, 0.7154, 0.0721): mu = (l_0 + l_1 +
 * ...) / float(n), nu = (l_0 l_0 + l_1 l_1 + ...) / float(n), in sample
 * order; r = 1 / float(n), times 1 / float(frameCounter + 1) when the draw
 * accumulates. float32, one rounding per operation. Pixels outside the drawn
 * rows or tile subset keep their contents. Ignored at spp = 1. NULL unbinds.
 * PT_ERR_STATE under an active pt_set_band partition, as above.
 *
 * The plane is meant to be an RGBA32F texture of the frame's size (its
 * pointer from pt_texture_device_ptr), bound by pt_pass_set_texture as the
 * optional sampler "gSampleMoments" of the svgf_reproject.frag and
 * svgf_variance.frag passes that denoise this draw's colour (PT_ERR_ARG for
 * a texture of another size). With sm its texel, on surface pixels:
 *   reproject  m0 = (1 - alpha) prev.x + alpha sm.x, m1 likewise with .y,
 *              variance = max(0, m1 - m0 m0) * sm.z; the rest as without it;
 *   variance   the spatial estimate runs iff h * sm.w < 4 (h: the history
 *              length; the shader's rule is h < 4), its sums as without it,
 *              variance = (m1 - m0 m0) * (4 / (h * sm.w)) * sm.z.
 * With sm = (lum, lum^2, 1, 1) both passes write the bits they write without
 * the sampler. A history written without the sampler holds per-frame moments,
 * one written with it per-sample moments: mixing the two modes over one
 * history's life is the caller's affair. No reference counterpart. */
int pt_pass_set_sample_moments(uint32_t pass, void* device_f32x4);
/* The next draw's sample counts from a draw's statistics, on the library's
 * current stream: for every pixel of the frame out_u8 = 1 where nd_tex.w == 1
 * (background); else the statistics are looked up at the texel holding
 * (pixel centre) - lag * motion_tex.xy * (width, height) and the count is the
 * largest, over the 3 x 3 texels around it inside the frame, of nmax where
 * v < 0 or m or v is NaN, else ceil(v / (tolerance * max(m, 1e-4))^2) held to
 * 2 .. nmax; nmax where that position is non-finite or outside the frame.
 * stats: width * height float pairs (pt_pass_set_sample_stats); motion_tex,
 * nd_tex: this frame's gMotion and gNormalAndLinearZ textures; lag: frames
 * since the statistics' draw; out_u8: width * height bytes. PT_ERR_ARG for a
 * tolerance that is not > 0, nmax outside 2 .. 8, null planes or textures of
 * different sizes; PT_ERR_STATE for textures created under an active
 * pt_set_band partition. Nothing is launched on an error. */
int pt_sample_counts_derive(const void* stats, uint32_t motion_tex, uint32_t nd_tex, float lag, float tolerance,
                            int nmax, void* out_u8);
/* The next draw's sample counts from statistics pooled over a slot's draws, on
 * the library's current stream (DESIGN.md "Pooled sample statistics"). A pool
 * plane holds width * height float4 (m, v, w, z): mean and unbiased variance
 * of the pooled luminances, the pooled sample weight (0: empty) and nd_tex.z
 * of the pixel when the texel was written. For every pixel p of the frame a
 * texel T(p) is formed: (0, 0, 0, z) on the background (nd_tex.w == 1) or
 * where the position (pixel centre) - lag * motion_tex.xy * (width, height)
 * is non-finite or outside the frame; else, with q the texel holding that
 * position, the history a = pool_in[q] is rejected (T empty) unless
 * |a.z - z| <= zeta * max(|z|, 1e-4), and is valid when a.w >= 1 and a.m, a.v
 * are finite; the new samples are n_s = min(max(counts_prev[q], 1), nmax_prev)
 * (nmax_prev without a plane) with (m_s, v_s) = stats[q], valid when m_s is
 * finite and n_s < 2 or v_s is finite and >= 0 (v_s counts as 0 at n_s < 2).
 * T is the valid one of the two, or their pairwise combination (Chan) with
 * the weight a.w + n_s held to wmax, or empty. T asks for nmax samples where
 * w < 2, else for ceil(v / d^2) held to 1 .. nmax with d = tolerance *
 * max(m, 1e-4) (rule 0, relative) or d = tolerance (rule 1, absolute).
 * pool_out[p] = T(p); out_u8[p] = 1 on the background, else the largest ask
 * over the surface texels of the 3 x 3 block around p inside the frame.
 * stats (width * height float pairs, pt_pass_set_sample_stats), counts_prev
 * (width * height bytes: the plane the statistics' draw read, nmax_prev its
 * spp) and pool_in (the plane the previous call wrote) are in that draw's
 * pixel coordinates; each may be NULL. lag: frames since that draw.
 * PT_ERR_ARG for a null pool_out or out_u8, pool_out == pool_in, out_u8 ==
 * counts_prev, a tolerance or zeta that is not > 0, wmax that is not >= 2, a
 * rule other than 0 or 1, nmax or nmax_prev outside 2 .. 8, or textures of
 * different sizes; PT_ERR_STATE for textures created under an active
 * pt_set_band partition. Nothing is launched on an error. */
int pt_sample_counts_pool(const void* stats, const void* counts_prev, int nmax_prev, const void* pool_in,
                          uint32_t motion_tex, uint32_t nd_tex, float lag, float wmax, float zeta, int rule,
                          float tolerance, int nmax, void* pool_out, void* out_u8);
/* Motion bound (G-buffer pass): while set, every draw first zeroes *device_u32 and
 * then stores there the largest |motion.y| (UV units, the bits of a non-negative
 * float; +inf for a non-finite motion) over the surface pixels it computes. The
 * multi-GPU band renderer sizes its reprojection / TAA history exchange from it
 * (svgf_reproject.frag:45-156 reads the history at uv - motion). NULL disables.
 * No reference counterpart (the single-GPU reference reads the whole frame). */
int pt_pass_set_motion_bound(uint32_t pass, void* device_u32);
/* Traversal counters (path-tracing pass, wavefront kernel): while set, every
 * draw ADDS to device_u64[0..13] (caller zeroes): primary rays, primary node +
 * triangle visits, bounce rays, bounce visits, shadow rays, shadow visits,
 * exact-tie re-walks on the reference tree, primary rays retried unbounded after
 * the G-buffer bound, rays whose stack spilled past the LDS stack (reference
 * trees deeper than 32 levels), the lane slots of primary / bounce / shadow
 * waves (64 x the wave's largest visit count), and, counted from the shadow
 * verdicts, the shadow rays toward point lights and the occluded shadow rays.
 * device_u64 holds `count` counters: counters past count are not written
 * (pt_trace_stats_count() = how many this library has; count above it is
 * capped, count <= 0 with a buffer is PT_ERR_ARG).
 * Wave-aggregated atomics; NULL disables (the default).
 * A draw with the int uniform "spp" = N > 1 (below) traces the primary rays
 * once: the primary counters (rays, visits, slots, retries) count one sample,
 * the bounce and shadow counters the rays of all N samples. */
int pt_pass_set_trace_stats_n(uint32_t pass, void* device_u64, int count);
/* The first form of the call: a buffer of PT_TRACE_STATS_V1 (12) counters,
 * the first 12 above; the two shadow-split counters are not written. */
#define PT_TRACE_STATS_V1 12
int pt_pass_set_trace_stats(uint32_t pass, void* device_u64);
/* 14: the counters of the form above, kept for callers that sized their buffers
 * by this call before the two point-light counters below were added. New
 * callers size their buffer by pt_trace_stats_total(). */
int pt_trace_stats_count(void);
/* Every traversal counter this library writes (16): the 14 above, then the
 * point-light shadow rays decided by the lights' triangle bins (pass uniform
 * point_bins) and those handed to the tree walk instead. A buffer of this many
 * counters, passed with its count to pt_pass_set_trace_stats_n, receives all. */
int pt_trace_stats_total(void);
/* The point-light triangle bins (pass uniform point_bins) of the scene decoded
 * from (tri_tex, node_tex), as the last path-tracing draw of that scene built
 * them; PT_ERR_STATE when it has none. Synchronises the device.
 * info8x4[8 * l ..] for light l < lights: [0] != 0 the light has no usable bins
 * (its rays walk; 2: it moved, pt_lights_update, and its lists are pending), [1] entries, [2..4] float bits of the light position the
 * bins were built around, [5] float bits of the coordinate magnitude the build
 * assumed, [6] entries of its catch-all list, [7] the (triangle, face) boxes
 * of more than 64 cells its last build binned a wave each.
 * dims4: cells per cube-face edge, lights, entries a light has room for, bytes
 * per entry (a light's lists hold [1] * that many bytes).
 * *bytes: the allocation. Any output may be NULL. */
int pt_point_bins_info(uint32_t tri_tex, uint32_t node_tex, int* info8x4, int* dims4, size_t* bytes);
/* A draw may reuse the work of the pass's last draw when nothing it depends on
 * has changed (a view that stands still; DESIGN.md "Static view"). Results are
 * bit for bit those of doing the work again.
 *  - path-tracing pass, int uniform primary_cache (default 1): the primary stage is
 *    skipped while eye, cameraRotate, the rows, the tile subset, the geometry and
 *    the stage's settings are those of the stage the pass last ran. Its state is
 *    the pass's own; 0 runs the stage in every draw. Bypassed while trace
 *    statistics or row costs are bound, by pt_kernel = 1 and by pt_pass_draw_batch.
 *  - rasterize pass, int uniform reuse_static (default 0): the caller's statement
 *    that nothing outside the library writes this pass's attachments between its
 *    draws (no write through pt_texture_device_ptr or into wrapped memory). Then a
 *    draw whose uniforms, triangles and attachments are as the pass's last draw
 *    left them launches nothing and returns PT_OK. The library tracks its own
 *    writes (draws of any pass, uploads, pt_tiles_copy, adopt) and every call that
 *    changes the triangles; a pass with a motion bound always draws.
 *    PTSVGF_STATIC_REUSE=0 in the environment forces 0.
 *  - path-tracing pass, int uniform reuse_static (default 0): the same statement
 *    about its three attachments. Then a one-sample, whole-frame draw that reuses
 *    the primary stage, and finds on its attachments the records of an earlier
 *    draw with the same view, scene, environment and settings, leaves its miss
 *    pixels and the emission and albedo planes as they are (DESIGN.md "Static
 *    view, part 4"; include/ptsvgf_debug_firsthit.h). The environment variable
 *    forces this 0 as well. */
int pt_pass_draw(uint32_t pass);
/* Draw `count` (1..8) path-tracing passes — the frames of a batch, each with its
 * own uniforms, samplers and attachments, one scene, size and band — as one
 * wavefront run whose list-driven traversal launches trace every frame's rays at
 * once (no GL counterpart: the reference draws one frame at a time). Results are
 * those of drawing each pass alone. passes[0] owns the shared wavefront state,
 * sized for max(count, its "trace_batch" uniform) frames; the batch is timed as
 * its draw. Accumulation (lastFrame) is refused; tile subsets are batched when every pass traces the same one
 * ("tile_stride" / "tile_offset").
 *
 * Samples per pixel: the int uniform "spp" = N of a path-tracing pass (default 1,
 * 1 .. 8) makes pt_pass_draw take N samples per pixel. Sample s is the
 * reference's main() with frameCounter replaced by F * N + s (uint32, wrapping;
 * F the pass's "frameCounter") and accumulation off; the colour attachment
 * receives (c_0 + c_1 + ... + c_{N-1}) / float(N) summed in that order in
 * float32, alpha 1, then (uniform "accumulate") mixed with lastFrame at
 * 1 / float(F + 1u); emission and albedo are those of one sample (the primary
 * ray does not depend on it, so the primary hit is traced once). N = 1 is the
 * plain draw, launch for launch. The samples run as the frames of a batch do
 * (one traversal launch per bounce takes every sample's rays); the pass's
 * wavefront state is sized for max(N, "trace_batch") frames plus N colour
 * planes of its band. PT_ERR_ARG, before anything is launched and with every
 * plane untouched: N outside 1 .. 8, N > 1 with "pt_kernel" != 0, and a pass
 * with N > 1 inside pt_pass_draw_batch. */
int pt_pass_draw_batch(const uint32_t* passes, int count);
/* Time the last draw of this pass (ms, HIP events on the library stream; syncs). */
int pt_pass_last_ms(uint32_t pass, float* ms);
int pt_pass_destroy(uint32_t pass);

#ifdef __cplusplus
}
#endif
#endif
