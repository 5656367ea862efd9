// engine_geometry.cpp -- C ABI of geometry changes on a resident context (4-D scans, cbctmc/mc/simulation.py:527-710) and of the
// voxel-file writers.
#include "engine_internal.hpp"
#include "resample.hpp"

using namespace mcgpu;

namespace {

// ---- one install path: mcgpu_set_geometry_arrays and the two image routes
VoxelGrid grid_of(const int n[3], const float spacing_cm[3]) {  // the dimensions; the voxel arrays are the caller's to fill or to leave empty
  VoxelGrid v;
  for (int k = 0; k < 3; ++k) {
    v.n[k] = n[k];
    v.voxel_size[k] = spacing_cm[k];
    v.size_bbox[k] = v.n[k] * v.voxel_size[k];
    v.inv_voxel_size[k] = 1.0f / v.voxel_size[k];
  }
  for (int k = 0; k < kMaxMaterials; ++k) v.density_max[k] = -999.0f;
  return v;
}

void check_voxel(int material, float density) {  // load_voxels' two refusals
  require(material >= 1 && material <= kMaxMaterials, -2, "!!ERROR load_voxels!! Voxel material number out of range!!");
  require(density >= 1.0e-9f, -2, "!!ERROR load_voxels!! Voxel density can not be 0 or negative");
}

// The context's geometry := `grid`, whose voxels are its own arrays or, with a `source`, classes on the device (the arrays stay empty:
// sync_host_voxels fills them on demand).  Everything that can fail is built beside the live model and swapped in at the end: when this
// throws, the context is what it was.  The Woodcock majorant and the set of loaded materials depend on the volume
// (MC-GPU_v1.3.cu:2220-2233,2294-2296), so the material tables are rebuilt.  Returns the superseded device model, which frees its memory --
// its correspondence model and its warp base too -- when the caller lets go of it.  NB: the dose tallies belong to a geometry and restart
// from zero with the new one.
DeviceModel install_geometry(mcgpu_ctx& C, VoxelGrid&& grid, const DeviceVolumeSource* source) {
  HostModel& H = C.host;
  MaterialTables mat;
  load_material_files(H.cfg.file_materials, grid, mat);
  int roi[6];
  clip_dose_roi(H.cfg.dose_roi_input, grid.n, roi);  // from the input's ROI, whatever geometries came between; Error -2 when nothing of it is left
  if (C.has_device) {  // the last calls that can fail without a rollback
    HIP_TRY(hipSetDevice(C.dev.device_id));
    HIP_TRY(hipDeviceSynchronize());
  }
  const auto swap_host = [&] {  // its own inverse
    std::swap(H.voxels, grid);
    std::swap(H.mat, mat);
    for (int k = 0; k < 6; ++k) std::swap(H.cfg.dose_roi[k], roi[k]);
  };
  swap_host();
  DeviceModel model;
  if (C.has_device) {
    try {
      model = upload_model(H, C.dev.device_id, source);
      for (int k = 0; k < 5; ++k) model.sched[k] = C.dev.sched[k];  // the tuned FAST schedule survives a geometry change
      model.sched_set = C.dev.sched_set;
      apply_schedule(model);
    } catch (...) {
      swap_host();
      throw;
    }
    std::swap(C.dev, model);
  }
  C.host_voxels_stale = source != nullptr;
  C.table_cache.clear();
  return model;
}

}  // namespace

// ---- on-device warps of the resident geometry (geometry_device.hip)
void WarpBase::make(DeviceModel& D) {
  if (vol) return;
  unsigned char* base = D.put(std::vector<unsigned char>(D.vol_bytes, 0));
  HIP_TRY(hipMemcpy(base, D.vol, D.vol_bytes, hipMemcpyDeviceToDevice));
  sub_first = D.put(std::vector<unsigned short>((size_t)D.sub_n[0] * D.sub_n[1] * D.sub_n[2], 0));
  brick_first = D.put(std::vector<unsigned short>((size_t)D.brick_count, 0));
  code_of = D.put(std::vector<unsigned char>(D.code_of, D.code_of + 256));
  rebuild_out = D.put(std::vector<unsigned int>(32, 0u));
  ev[0] = D.mem.event(hipEventDefault);
  ev[1] = D.mem.event(hipEventDefault);
  vol = base;  // last: a base that was not made whole is made again
}

void WarpBase::copy_field(DeviceModel& D, const float* displacement, size_t nvox) {
  if (!dvf) dvf = D.put(std::vector<float>(3 * nvox, 0.f));  // the field buffer exists only on this route
  const Stopwatch copy;
  HIP_TRY(hipMemcpy(dvf, displacement, 3 * nvox * 4, hipMemcpyHostToDevice));
  field_copy_ms = (float)copy.ms();
  field_bytes = 3 * nvox * 4;
}

namespace {

int compact_material(const DeviceModel& D, int entry) {  // of a palette entry: palette_host holds {density, bits(compact material)} pairs
  int mc;
  memcpy(&mc, &D.palette_host[2 * entry + 1], 4);
  return mc;
}

int palette_index(const DeviceModel& D, int material, float density) {  // of a (material, density) as a voxel file would carry it; -1: none
  const float dq = density_as_in_a_voxel_file(density);
  for (int e = 0; e < D.palette_size; ++e)
    if (compact_material(D, e) == D.compact_of[material - 1] && D.palette_host[2 * e] == dq) return e;
  return -1;
}

GeometryRebuild rebuild_arguments(const HostModel& H, const DeviceModel& D, int default_index) {  // all but the field's source
  GeometryRebuild g;
  g.nx = H.voxels.n[0]; g.ny = H.voxels.n[1]; g.nz = H.voxels.n[2];
  g.brick_shift = D.brick_shift;
  for (int k = 0; k < 3; ++k) { g.bn[k] = D.brick_n[k]; g.sn[k] = D.sub_n[k]; g.rn[k] = D.rec_n[k]; }
  g.base_idx = D.warp.vol; g.dvf = D.warp.dvf; g.default_index = (unsigned char)default_index;
  g.idx = (unsigned char*)D.vol;
  g.sub_first = D.warp.sub_first; g.brick_first = D.warp.brick_first;
  g.sub = D.sub; g.bricks = D.bricks; g.code_of = D.warp.code_of; g.background = D.background;
  g.rec = D.tile_rec;
  g.out = D.warp.rebuild_out;
  return g;
}

// largest density per material among the palette entries that occur (bit e of `occurs`) -> Woodcock majorant, the only table that depends on it
void densest_per_material(const DeviceModel& D, const unsigned int* occurs, float density_max[kMaxMaterials]) {
  for (int m = 0; m < kMaxMaterials; ++m) density_max[m] = -999.0f;
  for (int e = 0; e < D.palette_size; ++e)
    if (occurs[e >> 5] & (1u << (e & 31)))
      for (int m = 0; m < kMaxMaterials; ++m)
        if (D.compact_of[m] == compact_material(D, e)) density_max[m] = std::max(density_max[m], D.palette_host[2 * e]);
}

// What the rebuild kernels left (out: 16 words of occurring palette entries, then the mixed sub-bricks) becomes the context's geometry
void adopt_rebuilt_geometry(mcgpu_ctx& C, const unsigned int out[17]) {
  HostModel& H = C.host;
  DeviceModel& D = C.dev;
  densest_per_material(D, out, H.voxels.density_max);
  rebuild_woodcock(H.mat, H.voxels.density_max);
  refresh_woodcock(H, D);
  D.sub_mixed = (int)out[16];
  // The object region (box and, where it pays, elliptic cylinder) and the first-level codes follow from the bricks' classification
  // exactly as at upload (brick_codes): 64 KB of `brick_first` come down, 16 KB of codes go up.
  std::vector<unsigned short> bf((size_t)D.brick_count);
  HIP_TRY(hipMemcpy(bf.data(), D.warp.brick_first, bf.size() * 2, hipMemcpyDeviceToHost));
  const std::vector<unsigned char> bricks = brick_codes(H, D, bf, true);
  HIP_TRY(hipMemcpy(D.bricks, bricks.data(), bricks.size(), hipMemcpyHostToDevice));
  refresh_cold_geometry(D);
  C.host_voxels_stale = true;
  C.table_cache.clear();
}

// What mcgpu_warp_geometry and mcgpu_warp_geometry_signal share -- everything but where the field comes from: `displacement` (host
// floats, copied to the device) or, when it is null, the resident correspondence model at `signal` (nothing is copied).
void warp_resident_geometry(mcgpu_ctx* ctx, const char* who, const float* displacement, const double* signal, int frame, int default_material,
                            float default_density) {
  const std::string pre = std::string("!!ERROR!! ") + who + ": ";
  DeviceModel& D = ctx->dev;
  WarpBase& W = D.warp;
  require(D.vol_kind == kVolU8, -5, (pre + "needs a palette volume (<= 256 distinct (material, density) pairs); use mcgpu_set_geometry_arrays").c_str());
  require(default_material >= 1 && default_material <= kMaxMaterials && D.compact_of[default_material - 1] >= 0, -5,
          (pre + "the default material has no data file in this simulation").c_str());
  const int default_index = palette_index(D, default_material, default_density);
  require(default_index >= 0, -5, (pre + "the default (material, density) is not in the palette; use mcgpu_set_geometry_arrays").c_str());
  HIP_TRY(hipSetDevice(D.device_id));
  HIP_TRY(hipDeviceSynchronize());
  W.make(D);
  W.field_bytes = 0;
  W.field_copy_ms = 0.f;
  if (displacement) W.copy_field(D, displacement, ctx->host.voxels.count());
  GeometryRebuild g = rebuild_arguments(ctx->host, D, default_index);
  if (!displacement) g.model = D.corr.args(signal);
  HIP_TRY(launch_geometry_rebuild(g, frame, !D.knobs.no_exterior, nullptr, W.ev[0], W.ev[1]));
  unsigned int out[17];
  HIP_TRY(hipMemcpy(out, W.rebuild_out, sizeof out, hipMemcpyDeviceToHost));  // waits for the kernels
  HIP_TRY(hipEventElapsedTime(&W.kernel_ms, W.ev[0], W.ev[1]));
  adopt_rebuilt_geometry(*ctx, out);
}

// The rule of mcgpu_correspondence_set and _fit: the previous model goes first, and when `build` throws none is resident afterwards
template <class Build>
void replace_correspondence(DeviceModel& D, Build&& build) {
  D.corr.drop(D.mem);
  try {
    build();
  } catch (...) {
    D.corr.drop(D.mem);
    throw;
  }
}

// ---- CT image + segmentations -> geometry (image_map.hip)
unsigned char* device_room(CallDevice& dev, size_t bytes) { return dev.alloc<unsigned char>(std::max<size_t>(bytes, 16)); }

struct DeviceImage {  // the inputs of a mapping on the device, buffers of a CallDevice
  ImageMapArgs args{};
  double ms_upload = 0.0;
  size_t bytes = 0;
};
// Copies of the host arrays (`copy`) or buffers a kernel fills later, one for the image and one for every segmentation whose pointer is
// not null (the resampled inputs of mcgpu_set_geometry_image_resampled)
DeviceImage place_image(CallDevice& dev, size_t nvox, const void* image, int image_dtype, const uint8_t* const* segmentations, const float* thresholds,
                        bool copy) {
  DeviceImage in;
  const Stopwatch upload;
  const auto buffer = [&](const void* host, size_t n) {
    unsigned char* d = device_room(dev, n);
    if (copy) HIP_TRY(hipMemcpy(d, host, n, hipMemcpyHostToDevice));
    in.bytes += n;
    return d;
  };
  in.args.image_is_f32 = image_dtype == MCGPU_IMAGE_FLOAT32 ? 1 : 0;
  in.args.image = buffer(image, nvox * (in.args.image_is_f32 ? 4 : 2));
  for (int k = 0; k < kImageSegmentations; ++k) in.args.seg[k] = segmentations[k] ? buffer(segmentations[k], nvox) : nullptr;
  for (int k = 0; k < 3; ++k) in.args.threshold[k] = thresholds[k];
  unsigned int words[kImageStatWords];
  image_map_stats_init(words);
  in.args.stats = dev.upload(words, kImageStatWords);
  in.ms_upload = copy ? upload.ms() : 0.0;
  return in;
}

mcgpu_image_map_report filled_image_report(const unsigned int* words, double ms_kernel, double ms_upload, size_t kernel_bytes) {
  mcgpu_image_map_report r;
  memset(&r, 0, sizeof r);
  for (int c = 0; c < kImageClasses; ++c) {
    r.count[c] = words[c];
    r.first[c] = words[kImageClasses + c] == 0xFFFFFFFFu ? -1LL : (long long)words[kImageClasses + c];
  }
  r.unmapped = words[2 * kImageClasses];
  r.ms_kernel = ms_kernel; r.ms_upload = ms_upload;
  r.kernel_bytes = kernel_bytes;
  return r;
}

void check_image_arguments(const char* who, const mcgpu_ctx* ctx, const int* n, const void* image, int image_dtype, const uint8_t* const* segmentations,
                           const mcgpu_image_class* table, const float* thresholds, const mcgpu_image_map_report* report) {
  const std::string pre = std::string("!!ERROR!! ") + who + ": ";
  require(ctx && ctx->has_device && n && image && segmentations && table && thresholds && n[0] > 0 && n[1] > 0 && n[2] > 0 &&
              (image_dtype == MCGPU_IMAGE_INT16 || image_dtype == MCGPU_IMAGE_FLOAT32),
          -1, (pre + "bad argument (the context needs a device)").c_str());
  require((unsigned long long)n[0] * n[1] * n[2] < (1ULL << 31), -2, "!!ERROR!! voxel grid too large for the 32-bit voxel index of the kernel");
  check_report(who, "report", "mcgpu_image_map_report", report);
}

// What mcgpu_set_geometry_arrays derives from the voxel arrays, from the statistics of the classes (`words`): the classes as the
// source of a device model, and the densest occurrence of every material into `density_max`
DeviceVolumeSource classes_as_source(const unsigned char* classes, size_t bytes, const mcgpu_image_class* table, const unsigned int* words,
                                     float density_max[kMaxMaterials]) {
  DeviceVolumeSource src;
  src.classes_tiled = classes;
  src.bytes = bytes;
  for (int c = 0; c < kImageClasses; ++c) {
    src.material[c] = table[c].material;
    src.density[c] = density_as_in_a_voxel_file(table[c].density);  // once per class instead of once per voxel
    src.first[c] = words[kImageClasses + c];
    if (src.first[c] == 0xFFFFFFFFu) continue;
    check_voxel(src.material[c], src.density[c]);
    density_max[src.material[c] - 1] = std::max(density_max[src.material[c] - 1], src.density[c]);
  }
  return src;
}

// What mcgpu_set_geometry_image and mcgpu_set_geometry_image_resampled share: the inputs are on the device (`in`, buffers of `dev`), of
// the engine's grid `n`; map them beside the live model and install the result.  Nothing of the context has changed when it throws.
void install_mapped_image(mcgpu_ctx* ctx, const char* who, const int n[3], const float spacing_cm[3], CallDevice& dev, const DeviceImage& in,
                          const mcgpu_image_class* table, int frame, mcgpu_image_map_report* report) {
  const size_t tiled_bytes = (size_t)((n[0] + 3) >> 2) * ((n[1] + 3) >> 2) * ((n[2] + 3) >> 2) * 64;
  unsigned char* classes = device_room(dev, tiled_bytes);
  double ms_kernel = 0.0;
  {
    Stage stage(dev, ms_kernel);
    HIP_TRY(launch_image_map_tiled(in.args, frame, n[0], n[1], n[2], classes, ctx->dev.num_cus, nullptr));
    stage.done();
  }
  unsigned int words[kImageStatWords];
  HIP_TRY(hipMemcpy(words, in.args.stats, sizeof words, hipMemcpyDeviceToHost));
  const Stopwatch install;
  mcgpu_image_map_report rep = filled_image_report(words, ms_kernel, in.ms_upload, in.bytes + tiled_bytes);
  write_report(report, rep);  // the counts reach the caller whether or not the volume is refused
  if (rep.unmapped != 0) {
    char msg[200];
    snprintf(msg, sizeof msg, "!!ERROR!! %s: %u voxels are unmapped (no line of the mapping touches them: a body segmentation is missing)", who,
             words[2 * kImageClasses]);
    throw Error(-2, msg);
  }
  VoxelGrid v = grid_of(n, spacing_cm);
  const DeviceVolumeSource src = classes_as_source(classes, tiled_bytes, table, words, v.density_max);
  const DeviceModel superseded = install_geometry(*ctx, std::move(v), &src);  // freed when this returns: after the context is ready
  rep.ms_install = install.ms();
  write_report(report, rep);
}

}  // namespace

extern "C" {

int mcgpu_map_image(mcgpu_ctx* ctx, const int n[3], const void* image, int image_dtype, const uint8_t* const segmentations[8],
                    const mcgpu_image_class table[12], const float thresholds[3], uint8_t* material_out, float* density_out,
                    mcgpu_image_map_report* report) {
  ABI_BEGIN
  check_image_arguments("mcgpu_map_image", ctx, n, image, image_dtype, segmentations, table, thresholds, report);
  require(material_out && density_out, -1, "!!ERROR!! mcgpu_map_image: null output");
  unsigned char material[kImageClasses];
  float density[kImageClasses];
  for (int c = 0; c < kImageClasses; ++c) {
    require(table[c].material >= 0 && table[c].material <= 255, -1, "!!ERROR!! mcgpu_map_image: material number of a class out of range");
    material[c] = (unsigned char)table[c].material;
    density[c] = table[c].density;
  }
  DeviceModel& D = ctx->dev;
  HIP_TRY(hipSetDevice(D.device_id));
  const size_t nvox = (size_t)n[0] * n[1] * n[2];
  CallDevice dev;
  dev.events();
  const DeviceImage in = place_image(dev, nvox, image, image_dtype, segmentations, thresholds, true);
  unsigned char* m_out = device_room(dev, nvox);
  float* d_out = (float*)device_room(dev, nvox * 4);
  double ms_kernel = 0.0;
  {
    Stage stage(dev, ms_kernel);
    HIP_TRY(launch_image_map_plain(in.args, n[0], n[1], n[2], material, density, m_out, d_out, D.num_cus, nullptr));
    stage.done();
  }
  unsigned int words[kImageStatWords];
  HIP_TRY(hipMemcpy(words, in.args.stats, sizeof words, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(material_out, m_out, nvox, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(density_out, d_out, nvox * 4, hipMemcpyDeviceToHost));
  write_report(report, filled_image_report(words, ms_kernel, in.ms_upload, in.bytes + nvox * 5));
  return 0;
  ABI_END
}

int mcgpu_set_geometry_image(mcgpu_ctx* ctx, const int n[3], const float spacing_cm[3], const void* image, int image_dtype,
                             const uint8_t* const segmentations[8], const mcgpu_image_class table[12], const float thresholds[3], int frame,
                             mcgpu_image_map_report* report) {
  ABI_BEGIN
  check_image_arguments("mcgpu_set_geometry_image", ctx, n, image, image_dtype, segmentations, table, thresholds, report);
  require(spacing_cm && (frame == 0 || frame == 1), -1, "!!ERROR!! mcgpu_set_geometry_image: bad argument");
  HIP_TRY(hipSetDevice(ctx->dev.device_id));
  HIP_TRY(hipDeviceSynchronize());
  CallDevice dev;  // the mapping's inputs and the class volume: they live through the install
  dev.events();
  const DeviceImage in = place_image(dev, (size_t)n[0] * n[1] * n[2], image, image_dtype, segmentations, thresholds, true);
  install_mapped_image(ctx, "mcgpu_set_geometry_image", n, spacing_cm, dev, in, table, frame, report);
  return 0;
  ABI_END
}

int mcgpu_set_geometry_image_resampled(mcgpu_ctx* ctx, const int n_in[3], const double spacing_in_mm[3], const double spacing_out_mm[3],
                                       const void* image, int image_dtype, const uint8_t* const segmentations[8],
                                       const mcgpu_image_class table[12], const float thresholds[3], int frame, double image_default,
                                       mcgpu_image_map_report* image_report, mcgpu_resample_report* resample_report) {
  ABI_BEGIN
  const char* who = "mcgpu_set_geometry_image_resampled";
  check_image_arguments(who, ctx, n_in, image, image_dtype, segmentations, table, thresholds, image_report);
  require(spacing_in_mm && spacing_out_mm && (frame == 0 || frame == 1), -1, "!!ERROR!! mcgpu_set_geometry_image_resampled: bad argument");
  check_report(who, "resample_report", "mcgpu_resample_report", resample_report);
  const ResamplePlan plan = make_resample_plan(who, n_in, spacing_in_mm, spacing_out_mm);
  // the engine's grid and voxel size from the arrays' axes: frame 0 [nz][ny][nx], frame 1 [gx][gy][gz] = [ny][nx][nz]
  const int ax[3] = {frame == 0 ? 2 : 1, frame == 0 ? 1 : 0, frame == 0 ? 0 : 2};
  int n[3];
  float spacing_cm[3];
  for (int k = 0; k < 3; ++k) {
    n[k] = plan.n_out[ax[k]];
    spacing_cm[k] = (float)(spacing_out_mm[ax[k]] / 10.0);
  }
  HIP_TRY(hipSetDevice(ctx->dev.device_id));
  HIP_TRY(hipDeviceSynchronize());
  const size_t nvox_in = plan.voxels_in(), nvox_out = plan.voxels_out(), image_size = resample_element_size(image_dtype);
  CallDevice dev;  // the mapping's inputs, filled by the resampler, and the class volume: they live through the install
  dev.events();
  const DeviceImage in = place_image(dev, nvox_out, image, image_dtype, segmentations, thresholds, false);
  {
    mcgpu_resample_report rep;
    memset(&rep, 0, sizeof rep);
    const Stopwatch upload;
    CallDevice native;  // the arrays at their own spacing and the plan: gone before the mapping starts
    native.events();
    const ResampleArgs args = upload_resample_plan(native, plan);
    const void* d_image = native.upload((const unsigned char*)image, nvox_in * image_size);
    const unsigned char* d_seg[kImageSegmentations];
    for (int k = 0; k < kImageSegmentations; ++k) d_seg[k] = segmentations[k] ? native.upload(segmentations[k], nvox_in) : nullptr;
    rep.ms_upload = upload.ms();
    Stage stage(native, rep.ms_kernel);
    HIP_TRY(launch_resample(args, image_dtype, kResampleLinear, image_default, d_image, const_cast<void*>(in.args.image), nullptr));
    rep.kernel_bytes += (nvox_in + nvox_out) * image_size;
    for (int k = 0; k < kImageSegmentations; ++k) {
      if (!d_seg[k]) continue;
      HIP_TRY(launch_resample(args, MCGPU_IMAGE_UINT8, kResampleNearest, 0.0, d_seg[k], const_cast<unsigned char*>(in.args.seg[k]), nullptr));
      rep.kernel_bytes += nvox_in + nvox_out;
    }
    stage.done();
    write_report(resample_report, rep);
  }
  install_mapped_image(ctx, who, n, spacing_cm, dev, in, table, frame, image_report);
  return 0;
  ABI_END
}

// ---- 4-D support: one resident context, many (geometry, projection angle) jobs (cbctmc/mc/simulation.py:527-710)
int mcgpu_set_projection_angles(mcgpu_ctx* ctx, int n, const float* angles_deg) {
  ABI_BEGIN
  require(ctx && angles_deg && n >= 2 && n <= kMaxProjections, -1, "!!ERROR!! mcgpu_set_projection_angles: need 2..1024 angles");
  HostModel& H = ctx->host;
  require(H.cfg.num_projections >= 2, -2,
          "!!ERROR!! mcgpu_set_projection_angles: the input file must define a CT trajectory (more than one projection)");
  H.cfg.enable_specific_angles = 1;
  H.cfg.specific_angles.assign(angles_deg, angles_deg + n);
  H.cfg.num_projections = n;
  H.source.resize(1);    // pose 0 is the input file's (MC-GPU_v1.3.cu:3313); the others follow the angles
  H.detector.resize(1);
  build_ct_trajectory(H);
  if (ctx->has_device) {
    DeviceModel& D = ctx->dev;
    HIP_TRY(hipSetDevice(D.device_id));
    HIP_TRY(hipDeviceSynchronize());
    SourcePose* old_src = D.src_all;
    DetectorPose* old_det = D.det_all;
    D.src_all = D.put(H.source);
    D.det_all = D.put(H.detector);
    D.mem.free(old_src);
    D.mem.free(old_det);
  }
  return 0;
  ABI_END
}

int mcgpu_set_geometry_arrays(mcgpu_ctx* ctx, const int n[3], const float spacing_cm[3], const uint8_t* material, const float* density) {
  ABI_BEGIN
  require(ctx && n && spacing_cm && material && density && n[0] > 0 && n[1] > 0 && n[2] > 0, -1, "!!ERROR!! mcgpu_set_geometry_arrays: bad argument");
  VoxelGrid v = grid_of(n, spacing_cm);
  const size_t nvox = v.count();
  v.material.assign(material, material + nvox);
  v.density.resize(nvox);
  VoxelFileDensities as_in_a_file;
  for (size_t i = 0; i < nvox; ++i) {
    const float d = as_in_a_file(density[i]);
    check_voxel(material[i], d);
    v.density[i] = d;
    if (d > v.density_max[material[i] - 1]) v.density_max[material[i] - 1] = d;
  }
  install_geometry(*ctx, std::move(v), nullptr);
  return 0;
  ABI_END
}

int mcgpu_warp_geometry(mcgpu_ctx* ctx, const float* displacement, int frame, int default_material, float default_density) {
  ABI_BEGIN
  require(ctx && ctx->has_device && displacement && (frame == 0 || frame == 1), -1, "!!ERROR!! mcgpu_warp_geometry: bad argument (the context needs a device)");
  warp_resident_geometry(ctx, "mcgpu_warp_geometry", displacement, nullptr, frame, default_material, default_density);
  return 0;
  ABI_END
}

// ---- the correspondence model resident on the device (cbctmc/registration/correspondence.py:149-226; kernels: correspondence.hip)
int mcgpu_correspondence_clear(mcgpu_ctx* ctx) {
  ABI_BEGIN
  require(ctx && ctx->has_device, -1, "!!ERROR!! mcgpu_correspondence_clear: bad argument (the context needs a device)");
  HIP_TRY(hipSetDevice(ctx->dev.device_id));
  HIP_TRY(hipDeviceSynchronize());
  ctx->dev.corr.drop(ctx->dev.mem);
  return 0;
  ABI_END
}

int mcgpu_correspondence_set(mcgpu_ctx* ctx, const void* mean, int mean_is_f64, const double* coefficients, const double* mean_signal, int K, int frame) {
  ABI_BEGIN
  require(ctx && ctx->has_device && mean && coefficients && mean_signal && K >= 1 && (frame == 0 || frame == 1), -1,
          "!!ERROR!! mcgpu_correspondence_set: bad argument (the context needs a device)");
  DeviceModel& D = ctx->dev;
  HIP_TRY(hipSetDevice(D.device_id));
  HIP_TRY(hipDeviceSynchronize());
  replace_correspondence(D, [&] {
    require(K <= kFieldModelMaxK, -5, "!!ERROR!! mcgpu_correspondence_set: more than 4 signal dimensions: predict on the host and use mcgpu_warp_geometry");
    const size_t n = 3 * ctx->host.voxels.count();
    D.corr.alloc(D.mem, n, K, mean_is_f64 != 0, frame, mean_signal);
    HIP_TRY(hipMemcpy(D.corr.mean, mean, n * (mean_is_f64 ? 8 : 4), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(D.corr.coef, coefficients, n * K * 8, hipMemcpyHostToDevice));
  });
  return 0;
  ABI_END
}

int mcgpu_correspondence_fit(mcgpu_ctx* ctx, const float* const* fields, int T, const double* pinv, const double* mean_signal, int K, int frame,
                             float* mean_out, double* coefficients_out) {
  ABI_BEGIN
  require(ctx && ctx->has_device && fields && pinv && mean_signal && T >= 1 && K >= 1 && (frame == 0 || frame == 1), -1,
          "!!ERROR!! mcgpu_correspondence_fit: bad argument (the context needs a device)");
  for (int t = 0; t < T; ++t) require(fields[t] != nullptr, -1, "!!ERROR!! mcgpu_correspondence_fit: null field");
  DeviceModel& D = ctx->dev;
  HIP_TRY(hipSetDevice(D.device_id));
  HIP_TRY(hipDeviceSynchronize());
  replace_correspondence(D, [&] {
    require(K <= kFieldModelMaxK && T <= kFitMaxTimesteps, -5,
            "!!ERROR!! mcgpu_correspondence_fit: more than 4 signal dimensions or more than 64 time steps: fit on the host");
    const size_t n = 3 * ctx->host.voxels.count();
    D.corr.alloc(D.mem, n, K, false, frame, mean_signal);
    {  // the T fields pass through the device in slabs of elements, [T][slab], so that the inputs take a bounded amount of memory
      const size_t slab = std::min<size_t>(n, (size_t)std::max(1, knob_int("MCGPU_CORRESPONDENCE_SLAB", 1 << 22)));
      CallDevice dev;
      float* stage = dev.alloc<float>((size_t)T * slab * 4);
      for (size_t e0 = 0; e0 < n; e0 += slab) {
        const size_t m = std::min(slab, n - e0);
        for (int t = 0; t < T; ++t) HIP_TRY(hipMemcpy(stage + (size_t)t * m, fields[t] + e0, m * 4, hipMemcpyHostToDevice));
        HIP_TRY(launch_fit_model(stage, m, T, pinv, K, (float*)D.corr.mean + e0, D.corr.coef + e0 * K, nullptr));
        HIP_TRY(hipDeviceSynchronize());  // the next slab overwrites the stage
      }
    }
    if (mean_out) HIP_TRY(hipMemcpy(mean_out, D.corr.mean, n * 4, hipMemcpyDeviceToHost));
    if (coefficients_out) HIP_TRY(hipMemcpy(coefficients_out, D.corr.coef, n * K * 8, hipMemcpyDeviceToHost));
  });
  return 0;
  ABI_END
}

int mcgpu_correspondence_predict(mcgpu_ctx* ctx, const double* signal, int K, float* field_out) {
  ABI_BEGIN
  require(ctx && ctx->has_device && signal && field_out && K >= 1, -1, "!!ERROR!! mcgpu_correspondence_predict: bad argument (the context needs a device)");
  DeviceModel& D = ctx->dev;
  require(D.corr.resident(), -5, "!!ERROR!! mcgpu_correspondence_predict: no correspondence model is resident (mcgpu_correspondence_set)");
  require(K == D.corr.k, -1, "!!ERROR!! mcgpu_correspondence_predict: the signal does not have the model's number of dimensions");
  HIP_TRY(hipSetDevice(D.device_id));
  const size_t n = 3 * ctx->host.voxels.count();
  CallDevice dev;
  float* out = dev.alloc<float>(n * 4);
  HIP_TRY(launch_predict_field(D.corr.args(signal), n, out, nullptr));
  HIP_TRY(hipMemcpy(field_out, out, n * 4, hipMemcpyDeviceToHost));  // waits for the kernel
  return 0;
  ABI_END
}

int mcgpu_warp_geometry_signal(mcgpu_ctx* ctx, const double* signal, int K, int default_material, float default_density) {
  ABI_BEGIN
  require(ctx && ctx->has_device && signal && K >= 1, -1, "!!ERROR!! mcgpu_warp_geometry_signal: bad argument (the context needs a device)");
  DeviceModel& D = ctx->dev;
  require(D.corr.resident(), -5, "!!ERROR!! mcgpu_warp_geometry_signal: no correspondence model is resident (mcgpu_correspondence_set)");
  require(K == D.corr.k, -1, "!!ERROR!! mcgpu_warp_geometry_signal: the signal does not have the model's number of dimensions");
  warp_resident_geometry(ctx, "mcgpu_warp_geometry_signal", nullptr, signal, D.corr.frame, default_material, default_density);
  return 0;
  ABI_END
}

int mcgpu_warp_volume(mcgpu_ctx* ctx, const int n[3], const uint8_t* material, const float* density, const float* displacement,
                      int default_material, float default_density, uint8_t* material_out, float* density_out) {
  ABI_BEGIN
  require(ctx && ctx->has_device && n && material && density && displacement && material_out && density_out, -1,
          "!!ERROR!! mcgpu_warp_volume: bad argument (the context needs a device)");
  HIP_TRY(hipSetDevice(ctx->dev.device_id));
  const size_t nvox = (size_t)n[0] * n[1] * n[2];
  CallDevice dev;
  unsigned char *m_in = dev.alloc<unsigned char>(nvox), *m_out = dev.alloc<unsigned char>(nvox);
  float *d_in = dev.alloc<float>(nvox * 4), *d_out = dev.alloc<float>(nvox * 4), *u = dev.alloc<float>(nvox * 12);
  HIP_TRY(hipMemcpy(m_in, material, nvox, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_in, density, nvox * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(u, displacement, nvox * 12, hipMemcpyHostToDevice));
  HIP_TRY(launch_warp(n[0], n[1], n[2], m_in, d_in, u, (unsigned char)default_material, default_density, m_out, d_out, nullptr));
  HIP_TRY(hipMemcpy(material_out, m_out, nvox, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(density_out, d_out, nvox * 4, hipMemcpyDeviceToHost));
  return 0;
  ABI_END
}

int mcgpu_write_voxel_file(const char* path, const int n[3], const float spacing_cm[3], const uint8_t* material, const float* density,
                           int gzip) {
  ABI_BEGIN
  require(path && n && spacing_cm && material && density, -1, "!!ERROR!! mcgpu_write_voxel_file: null argument");
  write_voxel_file(path, n, spacing_cm, material, density, gzip != 0);
  return 0;
  ABI_END
}

int mcgpu_write_voxel_binary(const char* path, const int n[3], const float spacing_cm[3], const uint8_t* material, const float* density) {
  ABI_BEGIN
  require(path && n && spacing_cm && material && density, -1, "!!ERROR!! mcgpu_write_voxel_binary: null argument");
  write_voxel_binary(path, n, spacing_cm, material, density);
  return 0;
  ABI_END
}

}  // extern "C"
