// capi_materials.hip — materials edited in place (DESIGN.md "Material edits"): pt_materials_update and the
// diagnostics of include/ptsvgf_debug_materials.h. The definition is tests/materials_ref.py's; the kernels are
// kernels_materials.hip's. The versions of a scene's tri_shade records are a Versions (capi_state.h), written on the
// one stream all updates share; the first-hit key takes the scene's shade version where the draws are issued
// (capi_static.hip).
#include "../../include/ptsvgf_debug_materials.h"
#include "capi_state.h"
#include "materials_host.h"

using namespace ptapi;

namespace ptapi {

namespace {

// One update's table: pinned host staging, its device copy and the event after the update's last kernel. A slot is
// taken again once that event has completed, so a few serve every update.
struct MatSlot {
  float* host = nullptr;
  float* dev = nullptr;
  hipEvent_t done = nullptr;
};
constexpr int kMaterialsMaxObjects = 4096;  // as for poses
constexpr size_t kMatSlotBytes = (size_t)kMaterialsMaxObjects * ptk::kMaterialFloats * sizeof(float);

struct MaterialState {
  hipStream_t upload = nullptr;  // the updates' stream (non-blocking, created by the first update)
  hipEvent_t last = nullptr;     // recorded after every update's last kernel (materials_order)
  std::vector<MatSlot> slots;
} g_mat;

int take_slot(MatSlot** out) {
  for (MatSlot& s : g_mat.slots)
    if (hipEventQuery(s.done) == hipSuccess) {
      *out = &s;
      return PT_OK;
    }
  MatSlot s;
  HIPCHK(hipHostMalloc((void**)&s.host, kMatSlotBytes, hipHostMallocDefault));
  if (hipMalloc((void**)&s.dev, kMatSlotBytes) != hipSuccess ||
      hipEventCreateWithFlags(&s.done, hipEventDisableTiming) != hipSuccess) {
    if (s.dev) (void)hipFree(s.dev);
    (void)hipHostFree(s.host);
    return err(PT_ERR_HIP, "pt_materials_update: out of memory for the material table");
  }
  g_mat.slots.push_back(s);
  *out = &g_mat.slots.back();
  return PT_OK;
}

}  // namespace

void free_shade(SceneGPU& sg) {
  if (sg.shade.edited() || !sg.shade.sb.spare.empty()) (void)hipDeviceSynchronize();  // readers may run on any stream
  sg.shade.free();
}

int materials_order(hipStream_t s) {
  if (g_mat.last) HIPCHK(hipStreamWaitEvent(s, g_mat.last, 0));
  return PT_OK;
}

void free_materials() {
  for (MatSlot& s : g_mat.slots) {
    (void)hipHostFree(s.host);
    (void)hipFree(s.dev);
    (void)hipEventDestroy(s.done);
  }
  if (g_mat.last) (void)hipEventDestroy(g_mat.last);
  if (g_mat.upload) (void)hipStreamDestroy(g_mat.upload);
  g_mat = MaterialState{};
}

}  // namespace ptapi

extern "C" {

int pt_materials_update(uint32_t tri_tex, uint32_t pose, int first_obj, int count, const float* material18) {
  if (!material18) return err(PT_ERR_ARG, "pt_materials_update: null material18");
  if (count < 1 || count > kMaterialsMaxObjects)
    return err(PT_ERR_ARG, "pt_materials_update: count must be in [1, 4096]");
  if (first_obj < 0 || first_obj > (1 << 24) - count)
    return err(PT_ERR_ARG, "pt_materials_update: objects must lie in [0, 2^24) (float-encoded indices)");
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  Texture* t = tex_of(tri_tex);
  if (!t || t->target != PT_TEXTURE_BUFFER)
    return err(PT_ERR_INVALID_HANDLE, "pt_materials_update: tri_tex is not a texture buffer");
  if (t->bytes % (45 * sizeof(float)))
    return err(PT_ERR_ARG, "pt_materials_update: tri_tex must hold whole Triangle_encoded records (45 floats)");
  const size_t nt = t->bytes / (45 * sizeof(float));
  if (nt > (1u << 24)) return err(PT_ERR_ARG, "pt_materials_update: more than 2^24 triangles");
  Pose* ps = nullptr;
  if (pose) {
    auto it = g.poses.find(pose);
    if (it == g.poses.end()) return err(PT_ERR_INVALID_HANDLE, "pt_materials_update: unknown pose");
    ps = it->second.get();
    if ((size_t)ps->ntris != nt)
      return err(PT_ERR_ARG, "pt_materials_update: the pose holds another triangle count than tri_tex");
  }
  if (nt == 0) return PT_OK;
  const int n = (int)nt;

  if (!g_mat.upload) HIPCHK(hipStreamCreateWithFlags(&g_mat.upload, hipStreamNonBlocking));
  if (!g_mat.last) HIPCHK(hipEventCreateWithFlags(&g_mat.last, hipEventDisableTiming));
  hipStream_t up = g_mat.upload;
  MatSlot* slot = nullptr;
  TRY(take_slot(&slot));
  const size_t tbytes = (size_t)count * ptk::kMaterialFloats * sizeof(float);
  memcpy(slot->host, material18, tbytes);
  HIPCHK(hipMemcpyAsync(slot->dev, slot->host, tbytes, hipMemcpyHostToDevice, up));

  // A device decode of these texels that a draw queued (get_scene_lbvh) runs first: the texels are patched in place
  // below, and that draw reads the materials it was enqueued with. (Builds, refits and poses have synchronised.)
  for (auto& kv : g.scenes)
    if (kv.first.first == tri_tex && kv.second.shade.sb.built) HIPCHK(kv.second.shade.sb.wait_built(up));

  // the decoded records of every scene that holds this buffer's current contents: a version nothing in flight reads
  for (auto& kv : g.scenes) {
    SceneGPU& sg = kv.second;
    SharedBuf& sb = sg.shade.sb;
    if (kv.first.first != tri_tex || !sg.geom || !sb.buf || sg.tri_ver != t->version || sg.ntris != n) continue;
    // the version written last stays valid to read once retired: only a later update is handed it, and that one's
    // kernel runs after this one on the same stream
    const float4* old = (const float4*)sb.buf;
    const bool decoded = !sg.shade.edited();  // it is the decode's buffer
    if (const hipError_t e = sg.shade.next(sb.buf, (size_t)n * 9 * sizeof(float4))) {
      // the current version was retired and none found: the scene's next draw decodes it again (get_scene frees the
      // versions first), from texels and a mirror this call has not touched
      if (!sb.buf) sg.tri_ver = 0;
      return hip_err(e, "pt_materials_update: a new version of the shading records");
    }
    if (decoded && sb.built) {  // the decode's event (waited for above) does not describe the new version
      (void)hipEventDestroy(sb.built);
      sb.built = nullptr;
    }
    const int rc = ptk::materials_shade_launch(old, (float4*)sb.buf, n, slot->dev, first_obj, count, up);
    if (rc) return hip_err((hipError_t)rc, "pt_materials_update: shading records");
    HIPCHK(sb.mark_built(up));
    sg.shade_ver++;
  }

  // the texels and the pose's rest list where they lie: read only by library work that orders itself after this
  // (materials_order; refresh_host synchronises the device). No queued draw reads either.
  if (t->dev) {
    const int rc = ptk::materials_records_launch((float*)t->dev, n, slot->dev, first_obj, count, up);
    if (rc) return hip_err((hipError_t)rc, "pt_materials_update: texels");
  }
  if (ps && ps->tri_rest) {
    const int rc = ptk::materials_records_launch(ps->tri_rest, n, slot->dev, first_obj, count, up);
    if (rc) return hip_err((hipError_t)rc, "pt_materials_update: rest list");
  }
  if (!t->host_stale && t->host.size() == t->bytes)  // (a stale mirror is read back from the patched texels)
    patch_records_host((float*)t->host.data(), nt, material18, first_obj, count);
  HIPCHK(hipEventRecord(slot->done, up));
  HIPCHK(hipEventRecord(g_mat.last, up));
  return PT_OK;
}

// ------------------------------------------------------------ diagnostics (ptsvgf_debug_materials.h) ---
int pt_debug_materials_state(uint32_t tri_tex, uint32_t node_tex, uint64_t* shade_version, int* device_versions,
                             int* staging_slots) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  auto it = g.scenes.find({tri_tex, node_tex});
  if (it == g.scenes.end() || !it->second.shade.sb.buf)
    return err(PT_ERR_STATE, "pt_debug_materials_state: no scene decoded from these buffers");
  const SceneGPU& sg = it->second;
  if (shade_version) *shade_version = sg.shade_ver;
  if (device_versions) *device_versions = sg.shade.count();
  if (staging_slots) *staging_slots = (int)g_mat.slots.size();
  return PT_OK;
}

}  // extern "C"
