// engine_geometry.cpp -- C ABI of geometry changes on a resident context (4-D scans, cbctmc/mc/simulation.py:527-710) and of the
// voxel-file writers.
#include "engine_internal.hpp"
#include "resample.hpp"

#include <cstddef>

using namespace mcgpu;

namespace {

void drop_correspondence(DeviceModel& D) {
  if (D.corr_mean) D.mem.free(D.corr_mean);
  if (D.corr_coef) D.mem.free(D.corr_coef);
  D.corr_mean = nullptr;
  D.corr_coef = nullptr;
  D.corr_k = 0;
}

void alloc_correspondence(DeviceModel& D, size_t n, int K, bool mean_is_f64, int frame, const double* mean_signal) {
  D.corr_mean = D.mem.device_bytes(n * (mean_is_f64 ? 8 : 4));
  D.corr_coef = (double*)D.mem.device_bytes(n * K * 8);
  D.corr_k = K;
  D.corr_mean_is_f64 = mean_is_f64 ? 1 : 0;
  D.corr_frame = frame;
  for (int k = 0; k < K; ++k) D.corr_mean_signal[k] = mean_signal[k];
}

// the resident model as the field source of one respiratory state: d = signal - mean_signal, in double on the host
FieldModelArgs correspondence_args(const DeviceModel& D, const double* signal) {
  FieldModelArgs m;
  m.mean = D.corr_mean; m.coef = D.corr_coef; m.k = D.corr_k; m.mean_is_f64 = D.corr_mean_is_f64;
  for (int k = 0; k < D.corr_k; ++k) m.d[k] = signal[k] - D.corr_mean_signal[k];
  return m;
}

// What mcgpu_warp_geometry and mcgpu_warp_geometry_signal share -- everything but where the field comes from: `displacement` (host
// floats, copied to the device) or, when it is null, the resident correspondence model at `signal` (nothing is copied).
void warp_resident_geometry(mcgpu_ctx* ctx, const char* who, const float* displacement, const double* signal, int frame, int default_material,
                            float default_density) {
  const std::string pre = std::string("!!ERROR!! ") + who + ": ";
  HostModel& H = ctx->host;
  DeviceModel& D = ctx->dev;
  require(D.vol_kind == kVolU8, -5, (pre + "needs a palette volume (<= 256 distinct (material, density) pairs); use mcgpu_set_geometry_arrays").c_str());
  require(default_material >= 1 && default_material <= kMaxMaterials && D.compact_of[default_material - 1] >= 0, -5,
          (pre + "the default material has no data file in this simulation").c_str());
  int default_index = -1;
  {
    char t[64];
    snprintf(t, sizeof t, "%.6f", (double)default_density);  // densities as a voxel file would carry them
    const float dq = strtof(t, nullptr);
    for (int e = 0; e < D.palette_size && default_index < 0; ++e) {
      int mc;
      memcpy(&mc, &D.palette_host[2 * e + 1], 4);
      if (mc == D.compact_of[default_material - 1] && D.palette_host[2 * e] == dq) default_index = e;
    }
  }
  require(default_index >= 0, -5, (pre + "the default (material, density) is not in the palette; use mcgpu_set_geometry_arrays").c_str());
  HIP_TRY(hipSetDevice(D.device_id));
  HIP_TRY(hipDeviceSynchronize());
  const size_t nvox = H.voxels.count();
  const size_t nsub = (size_t)D.sub_n[0] * D.sub_n[1] * D.sub_n[2];
  if (!D.vol_base) {  // first call: what is resident now is the base geometry of every later warp
    D.vol_base = D.put(std::vector<unsigned char>(D.vol_bytes, 0));
    HIP_TRY(hipMemcpy(D.vol_base, D.vol, D.vol_bytes, hipMemcpyDeviceToDevice));
    D.sub_first = D.put(std::vector<unsigned short>(nsub, 0));
    D.brick_first = D.put(std::vector<unsigned short>((size_t)D.brick_count, 0));
    D.code_of_dev = D.put(std::vector<unsigned char>(D.code_of, D.code_of + 256));
    D.rebuild_out = D.put(std::vector<unsigned int>(32, 0u));
  }
  GeometryRebuild g;
  D.warp_field_bytes = 0;
  D.warp_field_copy_ms = 0.f;
  if (displacement) {  // the field buffer exists only on this route
    if (!D.dvf) D.dvf = D.put(std::vector<float>(3 * nvox, 0.f));
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipMemcpy(D.dvf, displacement, 3 * nvox * 4, hipMemcpyHostToDevice));
    D.warp_field_copy_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    D.warp_field_bytes = 3 * nvox * 4;
  } else {
    g.model = correspondence_args(D, signal);
  }
  g.nx = H.voxels.n[0]; g.ny = H.voxels.n[1]; g.nz = H.voxels.n[2];
  g.brick_shift = D.brick_shift;
  for (int k = 0; k < 3; ++k) { g.bn[k] = D.brick_n[k]; g.sn[k] = D.sub_n[k]; }
  g.base_idx = D.vol_base; g.dvf = D.dvf; g.default_index = (unsigned char)default_index;
  g.idx = (unsigned char*)D.vol;
  g.sub_first = D.sub_first; g.brick_first = D.brick_first;
  g.sub = D.sub; g.bricks = D.bricks; g.code_of = D.code_of_dev; g.background = D.background;
  g.rec = D.tile_rec;
  for (int k = 0; k < 3; ++k) g.rn[k] = D.rec_n[k];
  g.out = D.rebuild_out;
  const bool allow_exterior = !D.knobs.no_exterior;
  if (!D.warp_ev[0]) { D.warp_ev[0] = D.mem.event(hipEventDefault); D.warp_ev[1] = D.mem.event(hipEventDefault); }
  HIP_TRY(launch_geometry_rebuild(g, frame, allow_exterior, nullptr, D.warp_ev[0], D.warp_ev[1]));
  unsigned int out[17];
  HIP_TRY(hipMemcpy(out, D.rebuild_out, sizeof out, hipMemcpyDeviceToHost));  // waits for the kernels
  HIP_TRY(hipEventElapsedTime(&D.warp_kernel_ms, D.warp_ev[0], D.warp_ev[1]));
  // largest density per material among the palette entries that occur -> Woodcock majorant (the only table that depends on it)
  for (int m = 0; m < kMaxMaterials; ++m) H.voxels.density_max[m] = -999.0f;
  for (int e = 0; e < D.palette_size; ++e)
    if (out[e >> 5] & (1u << (e & 31))) {
      int mc;
      memcpy(&mc, &D.palette_host[2 * e + 1], 4);
      for (int m = 0; m < kMaxMaterials; ++m)
        if (D.compact_of[m] == mc) H.voxels.density_max[m] = std::max(H.voxels.density_max[m], D.palette_host[2 * e]);
    }
  rebuild_woodcock(H.mat, H.voxels.density_max);
  refresh_woodcock(H, D);
  D.sub_mixed = (int)out[16];
  // The object region (box and, where it pays, elliptic cylinder) and the first-level codes follow from the bricks' classification
  // exactly as at upload (brick_codes): 64 KB of `brick_first` come down, 16 KB of codes go up.
  std::vector<unsigned short> bf((size_t)D.brick_count);
  HIP_TRY(hipMemcpy(bf.data(), D.brick_first, bf.size() * 2, hipMemcpyDeviceToHost));
  const std::vector<unsigned char> bricks = brick_codes(H, D, bf, true);
  HIP_TRY(hipMemcpy(D.bricks, bricks.data(), bricks.size(), hipMemcpyHostToDevice));
  refresh_cold_geometry(D);
  ctx->host_voxels_stale = true;
  ctx->table_cache.clear();
}

// ---- CT image + segmentations -> geometry (image_map.hip)
// The inputs of a mapping on the device, freed when the holder goes.
struct MappedInputs {
  std::vector<void*> buffers;
  ImageMapArgs args{};
  double ms_upload = 0.0;
  size_t bytes = 0;
  ~MappedInputs() { release(); }
  void release() {
    for (void* p : buffers) (void)hipFree(p);
    buffers.clear();
  }
  void* device_copy(const void* host, size_t n) {
    void* d = nullptr;
    HIP_TRY(hipMalloc(&d, std::max<size_t>(n, 16)));
    buffers.push_back(d);
    if (host) HIP_TRY(hipMemcpy(d, host, n, hipMemcpyHostToDevice));
    return d;
  }
  // The mapping's inputs as buffers of this holder: copies of the host arrays (`copy`), or buffers a kernel fills later, one for the
  // image and one for every segmentation whose pointer is not null (the resampled inputs of mcgpu_set_geometry_image_resampled).
  void place(size_t nvox, const void* image, int image_dtype, const uint8_t* const* segmentations, const float* thresholds, bool copy) {
    const auto t0 = std::chrono::steady_clock::now();
    args.image_is_f32 = image_dtype == MCGPU_IMAGE_FLOAT32 ? 1 : 0;
    args.image = device_copy(copy ? image : nullptr, nvox * (args.image_is_f32 ? 4 : 2));
    bytes = nvox * (args.image_is_f32 ? 4 : 2);
    for (int k = 0; k < kImageSegmentations; ++k) {
      args.seg[k] = segmentations[k] ? (const unsigned char*)device_copy(copy ? segmentations[k] : nullptr, nvox) : nullptr;
      if (segmentations[k]) bytes += nvox;
    }
    for (int k = 0; k < 3; ++k) args.threshold[k] = thresholds[k];
    unsigned int words[kImageStatWords];
    image_map_stats_init(words);
    args.stats = (unsigned int*)device_copy(words, sizeof words);
    ms_upload = copy ? std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() : 0.0;
  }
  void upload(size_t nvox, const void* image, int image_dtype, const uint8_t* const* segmentations, const float* thresholds) {
    place(nvox, image, image_dtype, segmentations, thresholds, true);
  }
};

void fill_image_report(mcgpu_image_map_report* report, const unsigned int* words, double ms_kernel, double ms_upload, double ms_install, size_t kernel_bytes) {
  if (!report) return;
  mcgpu_image_map_report r;
  memset(&r, 0, sizeof r);
  r.struct_size = (unsigned int)sizeof r;
  for (int c = 0; c < kImageClasses; ++c) {
    r.count[c] = words[c];
    r.first[c] = words[kImageClasses + c] == 0xFFFFFFFFu ? -1LL : (long long)words[kImageClasses + c];
  }
  r.unmapped = words[2 * kImageClasses];
  r.ms_kernel = ms_kernel; r.ms_upload = ms_upload; r.ms_install = ms_install;
  r.kernel_bytes = kernel_bytes;
  const unsigned int want = report->struct_size;  // as the caller was compiled
  memcpy(report, &r, std::min<size_t>(want, sizeof r));
  report->struct_size = want;
}

void check_image_arguments(const char* who, const mcgpu_ctx* ctx, const int* n, const void* image, int image_dtype, const uint8_t* const* segmentations,
                           const mcgpu_image_class* table, const float* thresholds, const mcgpu_image_map_report* report) {
  const std::string pre = std::string("!!ERROR!! ") + who + ": ";
  require(ctx && ctx->has_device && n && image && segmentations && table && thresholds && n[0] > 0 && n[1] > 0 && n[2] > 0 &&
              (image_dtype == MCGPU_IMAGE_INT16 || image_dtype == MCGPU_IMAGE_FLOAT32),
          -1, (pre + "bad argument (the context needs a device)").c_str());
  require((unsigned long long)n[0] * n[1] * n[2] < (1ULL << 31), -2, "!!ERROR!! voxel grid too large for the 32-bit voxel index of the kernel");
  require(!report || report->struct_size >= 8, -1, (pre + "set report->struct_size = sizeof(mcgpu_image_map_report)").c_str());
}

float density_as_in_a_voxel_file(float density) {  // "%.6f", cbctmc/mc/voxel_data.pyx:25
  char t[64];
  snprintf(t, sizeof t, "%.6f", (double)density);
  return strtof(t, nullptr);
}

// What mcgpu_set_geometry_image and mcgpu_set_geometry_image_resampled share: the inputs are on the device (`in`), of the engine's grid
// `n`; map them, derive the model and swap it in.  Nothing of the context has changed when it throws.
void install_mapped_image(mcgpu_ctx* ctx, const char* who, const int n[3], const float spacing_cm[3], MappedInputs& in, const mcgpu_image_class* table,
                          int frame, mcgpu_image_map_report* report) {
  HostModel& H = ctx->host;
  const int device_id = ctx->dev.device_id, num_cus = ctx->dev.num_cus;
  VoxelGrid v;  // its voxel arrays stay empty: the voxels exist on the device only (sync_host_voxels fills them on demand)
  for (int k = 0; k < 3; ++k) {
    v.n[k] = n[k];
    v.voxel_size[k] = spacing_cm[k];
    v.size_bbox[k] = v.n[k] * v.voxel_size[k];
    v.inv_voxel_size[k] = 1.0f / v.voxel_size[k];
  }
  const size_t tiled_bytes = (size_t)((n[0] + 3) >> 2) * ((n[1] + 3) >> 2) * ((n[2] + 3) >> 2) * 64;
  // 1. the mapping, beside the live model
  unsigned char* classes = (unsigned char*)in.device_copy(nullptr, tiled_bytes);
  float ms = 0.f;
  unsigned int words[kImageStatWords];
  {
    Event ev[2];
    HIP_TRY(hipEventCreate(ev[0].make(device_id)));
    HIP_TRY(hipEventCreate(ev[1].make(device_id)));
    HIP_TRY(hipEventRecord(ev[0], nullptr));
    HIP_TRY(launch_image_map_tiled(in.args, frame, n[0], n[1], n[2], classes, num_cus, nullptr));
    HIP_TRY(hipEventRecord(ev[1], nullptr));
    HIP_TRY(hipMemcpy(words, in.args.stats, sizeof words, hipMemcpyDeviceToHost));  // waits for the kernel
    HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
  }
  const auto t_install = std::chrono::steady_clock::now();
  fill_image_report(report, words, ms, in.ms_upload, 0.0, in.bytes + tiled_bytes);
  if (words[2 * kImageClasses] != 0u) {
    char msg[200];
    snprintf(msg, sizeof msg, "!!ERROR!! %s: %u voxels are unmapped (no line of the mapping touches them: a body segmentation is missing)", who,
             words[2 * kImageClasses]);
    throw Error(-2, msg);
  }
  // 2. what mcgpu_set_geometry_arrays derives from the voxel arrays, from the statistics of the classes
  DeviceVolumeSource src;
  src.classes_tiled = classes;
  src.bytes = tiled_bytes;
  for (int k = 0; k < kMaxMaterials; ++k) v.density_max[k] = -999.0f;
  for (int c = 0; c < kImageClasses; ++c) {
    src.material[c] = table[c].material;
    src.density[c] = density_as_in_a_voxel_file(table[c].density);  // once per class instead of once per voxel
    src.first[c] = words[kImageClasses + c];
    if (src.first[c] == 0xFFFFFFFFu) continue;
    require(src.material[c] >= 1 && src.material[c] <= kMaxMaterials, -2, "!!ERROR load_voxels!! Voxel material number out of range!!");
    require(src.density[c] >= 1.0e-9f, -2, "!!ERROR load_voxels!! Voxel density can not be 0 or negative");
    v.density_max[src.material[c] - 1] = std::max(v.density_max[src.material[c] - 1], src.density[c]);
  }
  MaterialTables mat;
  load_material_files(H.cfg.file_materials, v, mat);
  int roi[6], roi_old[6];
  for (int k = 0; k < 6; ++k) roi_old[k] = H.cfg.dose_roi[k];
  clip_dose_roi(H.cfg.dose_roi_input, v.n, roi);  // from the input's ROI, whatever geometries came between; Error -2 when nothing of it is left
  std::swap(H.voxels, v);
  std::swap(H.mat, mat);
  for (int k = 0; k < 6; ++k) H.cfg.dose_roi[k] = roi[k];
  DeviceModel fresh;
  try {
    fresh = upload_model(H, device_id, &src);
    for (int k = 0; k < 5; ++k) fresh.sched[k] = ctx->dev.sched[k];  // the tuned FAST schedule survives a geometry change
    fresh.sched_set = ctx->dev.sched_set;
    apply_schedule(fresh);
  } catch (...) {
    std::swap(H.voxels, v);
    std::swap(H.mat, mat);
    for (int k = 0; k < 6; ++k) H.cfg.dose_roi[k] = roi_old[k];
    throw;
  }
  ctx->dev = std::move(fresh);  // with the superseded model go its correspondence model and its warp base
  ctx->host_voxels_stale = true;
  ctx->table_cache.clear();
  if (report && report->struct_size >= offsetof(mcgpu_image_map_report, ms_install) + sizeof(double))
    report->ms_install = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_install).count();
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
  MappedInputs in;
  in.upload(nvox, image, image_dtype, segmentations, thresholds);
  unsigned char* m_out = (unsigned char*)in.device_copy(nullptr, nvox);
  float* d_out = (float*)in.device_copy(nullptr, nvox * 4);
  Event ev[2];
  HIP_TRY(hipEventCreate(ev[0].make(D.device_id)));
  HIP_TRY(hipEventCreate(ev[1].make(D.device_id)));
  float ms = 0.f;
  unsigned int words[kImageStatWords];
  HIP_TRY(hipEventRecord(ev[0], nullptr));
  HIP_TRY(launch_image_map_plain(in.args, n[0], n[1], n[2], material, density, m_out, d_out, D.num_cus, nullptr));
  HIP_TRY(hipEventRecord(ev[1], nullptr));
  HIP_TRY(hipMemcpy(words, in.args.stats, sizeof words, hipMemcpyDeviceToHost));  // waits for the kernel
  HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
  HIP_TRY(hipMemcpy(material_out, m_out, nvox, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(density_out, d_out, nvox * 4, hipMemcpyDeviceToHost));
  fill_image_report(report, words, ms, in.ms_upload, 0.0, in.bytes + nvox * 5);
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
  MappedInputs in;
  in.upload((size_t)n[0] * n[1] * n[2], image, image_dtype, segmentations, thresholds);
  install_mapped_image(ctx, "mcgpu_set_geometry_image", n, spacing_cm, in, table, frame, report);
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
  require(!resample_report || resample_report->struct_size >= 8, -1,
          "!!ERROR!! mcgpu_set_geometry_image_resampled: set resample_report->struct_size = sizeof(mcgpu_resample_report)");
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
  MappedInputs in;
  in.place(nvox_out, image, image_dtype, segmentations, thresholds, false);
  double ms_kernel = 0.0;
  size_t kernel_bytes = 0;
  const auto t0 = std::chrono::steady_clock::now();
  {
    CallDevice native;  // the arrays at their own spacing and the plan: gone before the mapping starts
    native.events();
    const ResampleArgs args = upload_resample_plan(native, plan);
    const void* d_image = native.upload((const unsigned char*)image, nvox_in * image_size);
    const unsigned char* d_seg[kImageSegmentations];
    for (int k = 0; k < kImageSegmentations; ++k) d_seg[k] = segmentations[k] ? native.upload(segmentations[k], nvox_in) : nullptr;
    const double ms_upload = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    Stage stage(native, ms_kernel);
    HIP_TRY(launch_resample(args, image_dtype, kResampleLinear, image_default, d_image, const_cast<void*>(in.args.image), nullptr));
    kernel_bytes += (nvox_in + nvox_out) * image_size;
    for (int k = 0; k < kImageSegmentations; ++k) {
      if (!d_seg[k]) continue;
      HIP_TRY(launch_resample(args, MCGPU_IMAGE_UINT8, kResampleNearest, 0.0, d_seg[k], const_cast<unsigned char*>(in.args.seg[k]), nullptr));
      kernel_bytes += nvox_in + nvox_out;
    }
    stage.done();
    fill_resample_report(resample_report, ms_kernel, ms_upload, 0.0, kernel_bytes);
  }
  install_mapped_image(ctx, who, n, spacing_cm, in, table, frame, image_report);
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
  HostModel& H = ctx->host;
  VoxelGrid v;
  for (int k = 0; k < 3; ++k) {
    v.n[k] = n[k];
    v.voxel_size[k] = spacing_cm[k];
    v.size_bbox[k] = v.n[k] * v.voxel_size[k];
    v.inv_voxel_size[k] = 1.0f / v.voxel_size[k];
  }
  const size_t nvox = v.count();
  v.material.assign(material, material + nvox);
  v.density.resize(nvox);
  for (int k = 0; k < kMaxMaterials; ++k) v.density_max[k] = -999.0f;
  // densities as the voxel file would carry them ("%.6f", cbctmc/mc/voxel_data.pyx:25), so that handing arrays over
  // in-process gives the tables -- and therefore the tallies -- of the file-based flow
  std::unordered_map<uint32_t, float> q;
  for (size_t i = 0; i < nvox; ++i) {
    uint32_t b;
    memcpy(&b, &density[i], 4);
    auto it = q.find(b);
    float d;
    if (it != q.end()) d = it->second;
    else {
      char t[64];
      snprintf(t, sizeof t, "%.6f", (double)density[i]);
      d = strtof(t, nullptr);
      q.emplace(b, d);
    }
    const int mat = material[i];
    require(mat >= 1 && mat <= kMaxMaterials, -2, "!!ERROR load_voxels!! Voxel material number out of range!!");
    require(d >= 1.0e-9f, -2, "!!ERROR load_voxels!! Voxel density can not be 0 or negative");
    v.density[i] = d;
    if (d > v.density_max[mat - 1]) v.density_max[mat - 1] = d;
  }
  // Everything that can fail is built beside the live model and swapped in at the end: after an error return the context
  // is what it was before the call.  The Woodcock majorant and the set of loaded materials depend on the volume
  // (MC-GPU_v1.3.cu:2220-2233,2294-2296), so the material tables are rebuilt.
  MaterialTables mat;
  load_material_files(H.cfg.file_materials, v, mat);
  int roi[6];
  clip_dose_roi(H.cfg.dose_roi_input, v.n, roi);  // from the input's ROI, whatever geometries came between; Error -2 when nothing of it is left
  std::swap(H.voxels, v);
  std::swap(H.mat, mat);
  int roi_old[6];
  for (int k = 0; k < 6; ++k) { roi_old[k] = H.cfg.dose_roi[k]; H.cfg.dose_roi[k] = roi[k]; }
  if (ctx->has_device) {
    HIP_TRY(hipSetDevice(ctx->dev.device_id));
    HIP_TRY(hipDeviceSynchronize());
    DeviceModel fresh;
    try {
      fresh = upload_model(H, ctx->dev.device_id);
      for (int k = 0; k < 5; ++k) fresh.sched[k] = ctx->dev.sched[k];  // the tuned FAST schedule survives a geometry change
      fresh.sched_set = ctx->dev.sched_set;
      apply_schedule(fresh);
    } catch (...) {
      std::swap(H.voxels, v);
      std::swap(H.mat, mat);
      for (int k = 0; k < 6; ++k) H.cfg.dose_roi[k] = roi_old[k];
      throw;
    }
    ctx->dev = std::move(fresh);  // `fresh` now holds the superseded model and frees it.  NB: the dose tallies belong to a geometry and restart from zero with the new one
  }
  ctx->host_voxels_stale = false;
  ctx->table_cache.clear();
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
  drop_correspondence(ctx->dev);
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
  drop_correspondence(D);  // whatever follows, the previous model is gone: after a failure none is resident
  require(K <= kFieldModelMaxK, -5, "!!ERROR!! mcgpu_correspondence_set: more than 4 signal dimensions: predict on the host and use mcgpu_warp_geometry");
  const size_t n = 3 * ctx->host.voxels.count();
  try {
    alloc_correspondence(D, n, K, mean_is_f64 != 0, frame, mean_signal);
    HIP_TRY(hipMemcpy(D.corr_mean, mean, n * (mean_is_f64 ? 8 : 4), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(D.corr_coef, coefficients, n * K * 8, hipMemcpyHostToDevice));
  } catch (...) {
    drop_correspondence(D);
    throw;
  }
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
  drop_correspondence(D);
  require(K <= kFieldModelMaxK && T <= kFitMaxTimesteps, -5,
          "!!ERROR!! mcgpu_correspondence_fit: more than 4 signal dimensions or more than 64 time steps: fit on the host");
  const size_t n = 3 * ctx->host.voxels.count();
  // the T fields pass through the device in slabs of elements, [T][slab], so that the inputs take a bounded amount of memory
  const size_t slab = std::min<size_t>(n, (size_t)std::max(1, knob_int("MCGPU_CORRESPONDENCE_SLAB", 1 << 22)));
  float* stage = nullptr;
  try {
    alloc_correspondence(D, n, K, false, frame, mean_signal);
    stage = (float*)D.mem.device_bytes((size_t)T * slab * 4);
    for (size_t e0 = 0; e0 < n; e0 += slab) {
      const size_t m = std::min(slab, n - e0);
      for (int t = 0; t < T; ++t) HIP_TRY(hipMemcpy(stage + (size_t)t * m, fields[t] + e0, m * 4, hipMemcpyHostToDevice));
      HIP_TRY(launch_fit_model(stage, m, T, pinv, K, (float*)D.corr_mean + e0, D.corr_coef + e0 * K, nullptr));
      HIP_TRY(hipDeviceSynchronize());  // the next slab overwrites the stage
    }
    D.mem.free(stage);
    stage = nullptr;
    if (mean_out) HIP_TRY(hipMemcpy(mean_out, D.corr_mean, n * 4, hipMemcpyDeviceToHost));
    if (coefficients_out) HIP_TRY(hipMemcpy(coefficients_out, D.corr_coef, n * K * 8, hipMemcpyDeviceToHost));
  } catch (...) {
    if (stage) D.mem.free(stage);
    drop_correspondence(D);
    throw;
  }
  return 0;
  ABI_END
}

int mcgpu_correspondence_predict(mcgpu_ctx* ctx, const double* signal, int K, float* field_out) {
  ABI_BEGIN
  require(ctx && ctx->has_device && signal && field_out && K >= 1, -1, "!!ERROR!! mcgpu_correspondence_predict: bad argument (the context needs a device)");
  DeviceModel& D = ctx->dev;
  require(D.corr_coef != nullptr, -5, "!!ERROR!! mcgpu_correspondence_predict: no correspondence model is resident (mcgpu_correspondence_set)");
  require(K == D.corr_k, -1, "!!ERROR!! mcgpu_correspondence_predict: the signal does not have the model's number of dimensions");
  HIP_TRY(hipSetDevice(D.device_id));
  const size_t n = 3 * ctx->host.voxels.count();
  float* out = (float*)D.mem.device_bytes(n * 4);
  try {
    HIP_TRY(launch_predict_field(correspondence_args(D, signal), n, out, nullptr));
    HIP_TRY(hipMemcpy(field_out, out, n * 4, hipMemcpyDeviceToHost));  // waits for the kernel
  } catch (...) {
    D.mem.free(out);
    throw;
  }
  D.mem.free(out);
  return 0;
  ABI_END
}

int mcgpu_warp_geometry_signal(mcgpu_ctx* ctx, const double* signal, int K, int default_material, float default_density) {
  ABI_BEGIN
  require(ctx && ctx->has_device && signal && K >= 1, -1, "!!ERROR!! mcgpu_warp_geometry_signal: bad argument (the context needs a device)");
  DeviceModel& D = ctx->dev;
  require(D.corr_coef != nullptr, -5, "!!ERROR!! mcgpu_warp_geometry_signal: no correspondence model is resident (mcgpu_correspondence_set)");
  require(K == D.corr_k, -1, "!!ERROR!! mcgpu_warp_geometry_signal: the signal does not have the model's number of dimensions");
  warp_resident_geometry(ctx, "mcgpu_warp_geometry_signal", nullptr, signal, D.corr_frame, default_material, default_density);
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
