#pragma once
// engine_internal.hpp -- what the translation units of the engine library share: the device model and the context (the error
// plumbing and the per-call owners are hip_host.hpp's).
// (engine.cpp: the C ABI of a context -- creation, configuration, files, dose, finalize, stacks; engine_launch.cpp: the tracking launch,
// its arguments and the staged tally's host state; model_device.cpp: the device model's memory and its upload in stages (upload_model);
// engine_geometry.cpp: geometry changes of a resident context; engine_kat.cpp: known-answer and micro-benchmark hooks.)
//
// Replaces init_CUDA_device (docker/mcgpu/MC-GPU_v1.3.cu:2454-2724) and the per-projection driver of
// main() (:667-1056).  Compiled with hipcc; every HIP call lives here or in the kernel TUs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <unordered_map>

#include "../../include/mcgpu_amd.h"
#include "knobs.hpp"
#include "hip_host.hpp"
#include "device_model.hpp"
#include "ascii_device.hpp"
#include "geometry_device.hpp"
#include "image_map.hpp"

namespace mcgpu {

hipError_t launch_track_compat(const TrackArgs& args, int blocks, hipStream_t stream);
// the FAST kernels: device_model.hpp: fast_kernels<kDouble, kW2, kStats>()
hipError_t launch_kat_fast64(int n, const unsigned int* u, const double* a, const double* b, const double* c, const float* dir, double* out, hipStream_t stream);
// kat_scatter.inc, once per arithmetic (track_fast.hip / track_fast64.hip)
hipError_t launch_kat_scatter_fast(const TrackArgs& args, int kind, int n, unsigned int seed, unsigned int stream_key, const float* in4,
                                   const unsigned long long* in_u64, const int* mc, float* out4, unsigned int* out_u4, hipStream_t stream);
hipError_t launch_kat_scatter_fast64(const TrackArgs& args, int kind, int n, unsigned int seed, unsigned int stream_key, const float* in4,
                                     const unsigned long long* in_u64, const int* mc, float* out4, unsigned int* out_u4, hipStream_t stream);
// kat_history.inc, once per arithmetic (track_fast.hip / track_fast64.hip)
hipError_t launch_kat_history_fast(const TrackArgs& args, int kind, int n, const float* in8, const unsigned long long* in_u64, float* out8,
                                   unsigned int* out_u8, hipStream_t stream);
hipError_t launch_kat_history_fast64(const TrackArgs& args, int kind, int n, const float* in8, const unsigned long long* in_u64, float* out8,
                                     unsigned int* out_u8, hipStream_t stream);
// kat_flight.inc, once per arithmetic (track_fast.hip / track_fast64.hip)
hipError_t launch_kat_flight_fast(const TrackArgs& args, int kind, int n, int max_steps, const float* in8, const unsigned long long* in_u64,
                                  unsigned int* out, hipStream_t stream);
hipError_t launch_kat_flight_fast64(const TrackArgs& args, int kind, int n, int max_steps, const float* in8, const unsigned long long* in_u64,
                                    unsigned int* out, hipStream_t stream);
hipError_t prepare_tally_fold(const StageArgs& S);  // tally_fold.hip
hipError_t launch_tally_fold(const StageArgs& S, unsigned int workgroups, unsigned long long* image, hipStream_t stream);
hipError_t launch_tally_fold_squares(const StageArgs& S, unsigned int workgroups, unsigned long long* w2, hipStream_t stream);
hipError_t microbench_valu_issue(int num_cus, double out3[3], hipStream_t stream);
hipError_t microbench_atomic_rate(double* out, hipStream_t stream);
hipError_t microbench_copy_rate(int num_cus, double* out, hipStream_t stream);
hipError_t launch_kat_rng(int mode, int seed, int batch, int hpt, int n, float* out_dev, hipStream_t stream);
hipError_t launch_kat_streams_fast(int generator, unsigned int seed, unsigned int stream_key, unsigned long long first_id,
                                   const unsigned long long* ids_dev, int n_ids, int n_draws, unsigned int* out_dev, hipStream_t stream);
hipError_t launch_kat_math(int n, const double* x, double* l, double* e, double* s, double* c, hipStream_t stream);
hipError_t launch_kat_expf(int n, const float* x, float* e, hipStream_t stream);
hipError_t launch_kat_f32(int op, int n, const float* a, const float* b, float* out, hipStream_t stream);
hipError_t launch_warp(int nx, int ny, int nz, const unsigned char* mat, const float* dens, const float* dvf, unsigned char default_mat,
                       float default_dens, unsigned char* out_mat, float* out_dens, hipStream_t stream);
hipError_t launch_finalize(unsigned long long* image, int nx, int nz, int crop_nx, double norm, float* planes, int clear, hipStream_t stream);
hipError_t launch_finalize_variance(const unsigned long long* image, unsigned long long* w2, int nx, int nz, int crop_nx, unsigned long long histories,
                                    double c, float* planes, int clear, hipStream_t stream);

// What a device model allocated -- device buffers, pinned host buffers, streams, events -- released on its device (the one current at
// the first allocation) when the owner goes.  Move-only: a move assignment hands the previous contents to the source, which frees them.
class DeviceOwner {
 public:
  DeviceOwner() = default;
  DeviceOwner(const DeviceOwner&) = delete;
  DeviceOwner& operator=(const DeviceOwner&) = delete;
  DeviceOwner(DeviceOwner&& o) noexcept { swap(o); }
  DeviceOwner& operator=(DeviceOwner&& o) noexcept { swap(o); return *this; }
  ~DeviceOwner();
  void* device_bytes(size_t bytes);
  void* pinned_bytes(size_t bytes, unsigned int flags);
  hipStream_t stream(unsigned int flags);
  hipEvent_t event(unsigned int flags);
  void free(void* device_buffer);  // one device buffer before the owner goes

 private:
  void claim();
  void swap(DeviceOwner& o) noexcept;
  int device_ = -1;
  std::vector<void*> buffers_, pinned_;
  std::vector<hipStream_t> streams_;
  std::vector<hipEvent_t> events_;
};

// Host state of the staged detector tally (tally_stage.hpp) and the code that reads and writes it (engine_launch.cpp).  The cursor table's
// place in the LDS image is fixed at upload (-1: it does not fit, this model runs the direct atomics); the buffers belong to the device
// model's owner `mem`, are allocated at the first staged launch and only grow.
struct DeviceModel;
struct TallyStage {
  int cursor = -1;
  unsigned int bins = 0;
  unsigned long long* region = nullptr;
  size_t region_bytes = 0;
  unsigned int* counts = nullptr;
  size_t counts_bytes = 0;
  unsigned long long* fallback = nullptr;
  bool alloc_failed = false, fold_ready = false;
  TallyStagePlan plan{};  // of the last staged (sub-)launch

  bool wanted(const DeviceModel& D, bool has_w2) const;  // whether a launch of this model stages its hits
  void prepare(DeviceModel& D, unsigned long long detector_words, TrackArgs& A, int blocks, hipStream_t stream);
  unsigned long long fallback_hits(const DeviceModel& D) const;  // both wait for the device
  unsigned long long staged_hits(const DeviceModel& D) const;
};

// On-device geometry changes (mcgpu_warp_geometry, mcgpu_warp_geometry_signal): the base geometry that every warp starts from, the
// scratch of the rebuild and what the last warp measured.  The device memory and the events belong to the device model's owner `mem`.
#pragma GCC visibility push(hidden)  // used inside the library only: nothing of the two joins its dynamic symbols
struct WarpBase {
  unsigned char* vol = nullptr;  // the base geometry's palette index volume; null: nothing has been warped yet
  unsigned short *sub_first = nullptr, *brick_first = nullptr;  // scratch of the rebuild
  unsigned char* code_of = nullptr;  // the code assignment of the base geometry
  unsigned int* rebuild_out = nullptr;
  float* dvf = nullptr;            // the field of mcgpu_warp_geometry (allocated on its first call; the model route has none)
  hipEvent_t ev[2] = {nullptr, nullptr};  // around the warp kernel of the last geometry warp
  float kernel_ms = 0.f;      // its time (config key "warp_kernel_ms")
  float field_copy_ms = 0.f;  // host time of the field's copy to the device in the last geometry warp (0: no field was copied)
  size_t field_bytes = 0;     // field bytes the last geometry warp copied from the host (0: evaluated from the resident model)

  void make(DeviceModel& D);  // at the first warp: what is resident now is the base geometry of every later one
  void copy_field(DeviceModel& D, const float* displacement, size_t nvox);  // the host's field into `dvf`, timed
};

// The correspondence model resident on the device (mcgpu_correspondence_set / _fit; geometry_device.hpp: FieldModelArgs): mean [3N]
// float or double, coefficients double[3N][k], in the layout of `frame`
struct ResidentCorrespondence {
  void* mean = nullptr;
  double* coef = nullptr;
  int k = 0, mean_is_f64 = 0, frame = 0;
  double mean_signal[4] = {0, 0, 0, 0};

  bool resident() const { return coef != nullptr; }
  void alloc(DeviceOwner& mem, size_t n, int K, bool f64_mean, int in_frame, const double* signal_mean) {
    mean = mem.device_bytes(n * (f64_mean ? 8 : 4));
    coef = (double*)mem.device_bytes(n * K * 8);
    k = K;
    mean_is_f64 = f64_mean ? 1 : 0;
    frame = in_frame;
    for (int j = 0; j < K; ++j) mean_signal[j] = signal_mean[j];
  }
  void drop(DeviceOwner& mem) {
    if (mean) mem.free(mean);
    if (coef) mem.free(coef);
    mean = nullptr;
    coef = nullptr;
    k = 0;
  }
  // the model as the field source of one respiratory state: d = signal - mean_signal, in double on the host
  FieldModelArgs args(const double* signal) const {
    FieldModelArgs m;
    m.mean = mean; m.coef = coef; m.k = k; m.mean_is_f64 = mean_is_f64;
    for (int j = 0; j < k; ++j) m.d[j] = signal[j] - mean_signal[j];
    return m;
  }
};
#pragma GCC visibility pop

struct DeviceModel {
  int device_id = -1;
  void* vol = nullptr;
  size_t vol_bytes = 0;
  int vol_kind = kVolU8, palette_size = 0;
  float* palette = nullptr;
  unsigned char* bricks = nullptr;
  // on-device formatter of the ASCII projection files (mcgpu_format_projection): a few slots, so that the host writes
  // the text of earlier projections while the next is formatted
  struct AsciiSlot {
    char* text_dev = nullptr;
    char* text_host = nullptr;            // pinned
    unsigned long long* rows_dev = nullptr;   // row_len[nz] row_off[nz+1] row_arg[nz] | row_sum[nz] row_max[nz] | flags
    unsigned long long* rows_host = nullptr;  // pinned copy of the same block
    hipStream_t copy_stream = nullptr;        // the slot's download (copy engine)
    hipEvent_t ready = nullptr;               // recorded behind the formatter and the download of the row block
  } ascii[MCGPU_ASCII_SLOTS];
  unsigned long long ascii_capacity = 0;
  WarpBase warp;               // on-device geometry changes, above
  ResidentCorrespondence corr;  // the correspondence model resident on the device, above
  std::vector<float> palette_host;  // {density, bits(compact material)} pairs
  unsigned char code_of[256];
  int background = 0;
  unsigned char* sub = nullptr;   // second-level codes: 4 bits per sub-brick of 4^3 voxels, dense over the volume (u8 volumes)
  int sub_n[3] = {1, 1, 1}, sub_mixed = 0;
  TileRecord* tile_rec = nullptr;  // second level as 16-byte records of the tiles (MCGPU_TILE_RECORDS; device_model.hpp), or null
  int rec_n[3] = {1, 1, 1};        // cubes of 2x2x2 tiles per axis
  long long tiles_in_mixed_bricks = 0;  // tiles a flight step can ask the second level / the volume for (hot set of the voxel gathers)
  int brick_shift = 0, brick_n[3] = {1, 1, 1}, brick_count = 0, brick_bytes = 0, bricks_mixed = 0;
  int brick_palette[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  int has_exterior = 0, bricks_exterior = 0;
  float objbox_lo[3] = {0, 0, 0}, objbox_hi[3] = {0, 0, 0};
  float ell_c[2] = {0, 0}, ell_inv[2] = {0, 0};  // elliptic cylinder around the object (TrackCold::ell_*); inv 0: none
  LdsLayout lds;
  TrackCold* cold = nullptr;      // device copy of the rarely used table pointers
  TrackCold cold_host;            // its host image (re-uploaded when a tuning knob changes)
  unsigned long long* dose_voxels = nullptr;     // ulonglong2 per ROI voxel (null: tally off)
  unsigned long long* dose_materials = nullptr;  // ulonglong2 x 25 (null: tally off)
  size_t dose_roi_voxels = 0;
  int dose_flags = 0;
  SourcePose* src_all = nullptr;  // [num_projections]
  DetectorPose* det_all = nullptr;
  int resident_fast = 0;  // workgroups per CU (occupancy query), 0 = not asked yet
  bool resident_covers_w2 = false;  // ... and the w2 instantiations have been asked too (at the first launch with a w2)
  unsigned long long* stats = nullptr;  // kNumStats scheduler counters of the diagnostic build
  unsigned long long* work_counter = nullptr;  // history-id dispenser of the FAST kernel
  TallyStage stage;  // staged detector tally: its host state, above
  unsigned long long* scratch_image = nullptr;  // device tally of mcgpu_run_projection (allocated on first use)
  unsigned long long* scratch_w2 = nullptr;     // ... and the squared weights of mcgpu_run_projection_w2
  float *woodcock = nullptr, *mfp = nullptr, *mfp_tot = nullptr;
  float* wood_coarse = nullptr;  // FAST: majorant per coarse energy bin (LdsLayout::wood), rebuilt with the Woodcock table
  int sig_shift = -1;            // cross-section brackets of the FAST flight step (model_device.cpp: sigma_brackets), -1: none
  int sched[5] = {40, 12, 44, 12, 40};  // FAST batching thresholds {compton, rayleigh, new, flyable_low, swap_batch} (mcgpu_set_fast_schedule; re-tuned in round 5: profiles/r05p_*)
  bool sched_set = false;              // mcgpu_set_fast_schedule has been called (else the scheduler's own defaults apply)
  // Tuning knobs of the environment.  Read when the device model is built and again only by
  // mcgpu_reload_env_knobs: the launch path itself never looks at the environment and never synchronises.
  struct Knobs {
    int exterior_mode = 3;                           // MCGPU_EXTERIOR_MODE: bit 0 hop during flight, bit 1 hop at the source
    bool compat_stats = false;                       // MCGPU_COMPAT_STATS: hand the diagnostic COMPAT build its counter buffer
    int compat_thresh[4] = {-1, -1, -1, -1};         // MCGPU_COMPAT_THRESH_{COMPTON,RAYLEIGH,NEW,TAKE}; -1: chosen from the materials (make_args)
    int blocks_per_cu = 0;                           // MCGPU_BLOCKS_PER_CU (0: ask the occupancy API)
    int grid_spare_percent = 0;                      // MCGPU_GRID_SPARE_PERCENT
    int sched_override[5] = {-1, -1, -1, -1, -1};    // MCGPU_THRESH_{COMPTON,RAYLEIGH,NEW}, MCGPU_FLYABLE_LOW, MCGPU_SWAP_BATCH (-1: sched[])
    int slot_trade = 3, hold_q = 6;                  // MCGPU_SLOT_TRADE, MCGPU_HOLD_Q
    bool no_exterior = false;                        // MCGPU_NO_EXTERIOR (also read by the geometry builders)
    int segment_loop = -1;                           // MCGPU_SEGMENT_LOOP: -1 chosen from the model (make_args), 0 / 1 forced
    int tally_stage = -1;                            // MCGPU_TALLY_STAGE: detector hits staged and folded (tally_stage.hpp): 1 on, 0 direct atomics, -1 by the exterior share (engine_launch.cpp: TallyStage::wanted)
    int stage_cap = 0;                               // MCGPU_TALLY_STAGE_CAP (test hook): records per (workgroup, bin), 0: from the plan
    unsigned long long stage_max_histories = 1ULL << 27;  // MCGPU_TALLY_STAGE_MAX_HISTORIES: sub-launch limit of a staged launch
    int fast_sched = 0;                              // MCGPU_FAST_SCHED: 0 per-wave pools, 1 workgroup-level pool (fixes the LDS layout: read at upload)
  } knobs;
  int nmat = 0;
  int compact_of[kMaxMaterials];
  hipEvent_t ev_start = nullptr, ev_stop = nullptr;
  bool timed = false;
  int num_cus = 256;
  DeviceOwner mem;  // everything above that points to device or pinned memory, streams and events; freed with the model

  template <typename T>
  T* put(const std::vector<T>& host) {
    void* d = mem.device_bytes(std::max<size_t>(host.size() * sizeof(T), 16));
    if (!host.empty()) HIP_TRY(hipMemcpy(d, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
    return (T*)d;
  }
};

}  // namespace mcgpu

struct mcgpu_ctx {
  mcgpu::HostModel host;
  mcgpu::DeviceModel dev;
  bool has_device = false;
  bool host_voxels_stale = false;  // the device holds a geometry warped or mapped there (mcgpu_warp_geometry, mcgpu_set_geometry_image): H.voxels is downloaded on demand
  std::map<std::string, std::vector<unsigned char>> table_cache;
};

namespace mcgpu {
// model_device.cpp
std::vector<float> coarse_woodcock(const HostModel& H);  // LdsLayout::wood from the host's Woodcock table
// Shared by the upload of a geometry and the device-side geometry change (mcgpu_warp_geometry):
constexpr unsigned short kMixedBrick = 0x100;  // brick_first entry of a brick that holds more than one palette entry (as geometry_device.hip writes it)
std::vector<unsigned char> brick_codes(const HostModel& H, DeviceModel& D, const std::vector<unsigned short>& brick_first,
                                       bool have_background);  // object region, exterior bricks, packed first-level codes
void refresh_woodcock(const HostModel& H, DeviceModel& D);      // the Woodcock table and its coarse LDS copy, from H
void refresh_cold_geometry(DeviceModel& D);                     // object region and brick palette into TrackCold, uploaded if changed
void read_env_knobs(DeviceModel& D);
void apply_schedule(DeviceModel& D);
// A u8 volume that is already on the device as classes (image_map.hip), for upload_model to build the model around instead of H.voxels' arrays
struct DeviceVolumeSource {
  const unsigned char* classes_tiled = nullptr;  // class per voxel, 4x4x4-tiled, padding as tiled_volume writes it
  size_t bytes = 0;
  int material[kImageClasses];                   // material number and density (as a voxel file would carry it) of every class
  float density[kImageClasses];
  unsigned int first[kImageClasses];             // smallest [z][y][x] index of the class, 0xFFFFFFFF: it does not occur
};
DeviceModel upload_model(const HostModel& H, int device_id, const DeviceVolumeSource* mapped = nullptr);
TrackArgs make_args(const mcgpu_ctx& C, int p);  // engine_launch.cpp
void sync_host_voxels(mcgpu_ctx& C);
const void* host_table(mcgpu_ctx& C, const std::string& name, size_t& bytes);
}  // namespace mcgpu

