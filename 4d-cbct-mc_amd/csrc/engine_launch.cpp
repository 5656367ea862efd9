// engine_launch.cpp -- the tracking launch of an engine context: its arguments, the host state of the staged detector tally, the grid
// size, the COMPAT and FAST launches, the scheduler's knobs and counters.  Replaces the per-projection driver of main() (docker/mcgpu/MC-GPU_v1.3.cu:667-1056).
#include "engine_internal.hpp"

using namespace mcgpu;

namespace mcgpu {

TrackArgs make_args(const mcgpu_ctx& C, int p) {
  const HostModel& H = C.host;
  const DeviceModel& D = C.dev;
  TrackArgs A;
  memset(&A, 0, sizeof A);
  A.vol = D.vol; A.palette = D.palette; A.vol_kind = D.vol_kind; A.palette_size = D.palette_size;
  A.brick_shift = D.brick_shift; A.brick_nx = D.brick_n[0]; A.brick_nxy = D.brick_n[0] * D.brick_n[1];
  A.brick_bytes = D.vol_kind == kVolU8 ? D.brick_bytes : 0;
  A.sub = D.vol_kind == kVolU8 ? D.sub : nullptr; A.sub_nx = D.sub_n[0]; A.sub_nxy = D.sub_n[0] * D.sub_n[1];
  A.sub_kind = A.sub ? 1 : 0;
  A.rec_nx = D.rec_n[0]; A.rec_nxy = D.rec_n[0] * D.rec_n[1];
  if (D.vol_kind == kVolU8 && D.tile_rec) { A.sub = reinterpret_cast<const unsigned char*>(D.tile_rec); A.sub_kind = 2; }  // the records win over the code table
  A.lds = D.lds;
  A.nx = H.voxels.n[0]; A.ny = H.voxels.n[1]; A.nz = H.voxels.n[2]; A.nxy = A.nx * A.ny;
  for (int k = 0; k < 3; ++k) {
    A.inv_vs[k] = H.voxels.inv_voxel_size[k];
    A.bbox[k] = H.voxels.size_bbox[k];
    // upper clamp of the FAST kernel: bbox - EPS_SOURCE (MC-GPU_v1.3.h:87), lowered until it indexes the last voxel
    float hi = A.bbox[k] - 0.000015f;
    while ((int)(hi * A.inv_vs[k]) > H.voxels.n[k] - 1) hi = std::nextafter(hi, 0.0f);
    A.bbox_hi[k] = hi;
  }
  require((long long)A.nx * A.ny < (1LL << 24) && (long long)H.voxels.count() < (1LL << 31), -2,
          "!!ERROR!! voxel grid too large for the 32-bit voxel index of the kernel");
  A.e0 = H.mat.e0; A.ide = H.mat.ide; A.num_values = H.mat.num_values; A.nmat = D.nmat;
  A.woodcock = D.woodcock; A.mfp = D.mfp; A.mfp_tot = D.mfp_tot; A.sig_shift = D.sig_shift;
  A.cold = D.cold;
  A.nbins = H.spectrum.num_bins;
  A.src = D.src_all + p; A.det = D.det_all + p;
  A.stream_key = (unsigned)p;
  A.dose_flags = D.dose_flags;

  A.sched_kind = D.knobs.fast_sched;
  A.has_exterior = (D.vol_kind == kVolU8 && D.has_exterior) ? D.knobs.exterior_mode : 0;  // bit 0: hop during flight, bit 1: hop at the source
  // batching thresholds of the COMPAT kernel (lanes of a wave64 holding such a history in their registers or their parking slot)
  // The Compton batch of the COMPAT kernel walks every electron shell of the material several times in the reference's own
  // arithmetic: with tissue tables (29-40 shells) it is 60-73 % of the kernel and wants FULL batches -- threshold 40 of 64 lanes
  // instead of 20: thorax +39 %, CIRS +32 % (tools/compat_sweep.py) -- while the 4-12 shells of the Catphan's plastics prefer
  // photons back in flight early (40: -21 %).  Chosen from the mean shell count of the materials in use; tallies do not depend on it.
  // Second sweep: the tally/source batch is cheap and should not hold lanes back (24 -> 12..16 lanes), which in turn lets the
  // Compton batch wait for 48: thorax 1.9e8 -> 2.95e8, CIRS 4.6e8 -> 6.5e8, Catphan 1.58e9 -> 1.66e9 histories/s.
  // Round 3, with resumable Compton trials and two batches per lane (track_kernel.inc), the same thresholds are still the best of
  // the sweep (profiles/r03u_compat_sweep.txt): thorax 4.1e8, CIRS 9.2e8, Catphan 1.8e9; exchanging the two histories of a lane
  // pays from 1-8 takers on (thresh_take), 16+ loses.
  // Later in round 3 the Compton batch lost two thirds of its cost (S0 bounds, in-place Klein-Nishina rejections) and the wave takes
  // four flight steps between two looks at its state: 48 / 8 / 16 on tissue and 32 / 4 / 24 on plastics sit on flat optima
  // (profiles/r03y_compat_sweep.txt).
  int shells = 0, used = 0;
  for (int m = 0; m < kMaxMaterials; ++m)
    if (D.compact_of[m] >= 0) { shells += std::min(H.mat.noscco[m], kMaxShells); ++used; }
  const bool many_shells = used > 0 && shells >= 20 * used;
  A.segment_loop = D.knobs.segment_loop >= 0 ? D.knobs.segment_loop : ((A.sub_kind == 2 || many_shells) ? 1 : 0);  // track_pool.inc: kSegmentLoop
  A.thresh_compton = D.knobs.compat_thresh[0] >= 0 ? D.knobs.compat_thresh[0] : (many_shells ? 48 : 32);
  A.thresh_rayleigh = D.knobs.compat_thresh[1] >= 0 ? D.knobs.compat_thresh[1] : (many_shells ? 8 : 4);
  A.thresh_new = D.knobs.compat_thresh[2] >= 0 ? D.knobs.compat_thresh[2] : (many_shells ? 16 : 24);
  A.thresh_take = D.knobs.compat_thresh[3] >= 0 ? D.knobs.compat_thresh[3] : 2;
  // One source of truth: the FAST kernel reads mfp / e0 / ide / bbox / lds from TrackCold, written once in upload_model
  // (they would otherwise sit in scalar registers for the whole persistent loop); the COMPAT kernel reads the copies above.
  if (D.cold) {
    const TrackCold& ch = D.cold_host;
    require(ch.mfp == A.mfp && ch.e0 == A.e0 && ch.ide == A.ide && memcmp(ch.bbox, A.bbox, sizeof A.bbox) == 0 && memcmp(&ch.lds, &A.lds, sizeof A.lds) == 0, -9,
            "!!ERROR!! internal: TrackCold and the launch arguments disagree on mfp / e0 / ide / bbox / lds (upload_model and make_args have drifted apart)");
  }
  return A;
}

// Whether a launch of this model stages its detector hits (MCGPU_TALLY_STAGE: 1 / 0 force it, default -1 = the rules below).
// Without w2, staging pays where the scattered tally atomics bind the launch, i.e. where most histories are detected: a small object in a large
// volume of background, which the engine knows as the share of EXTERIOR bricks (the source's photons that miss the object region
// reach the detector unattenuated).  Measured (profiles/tally_stage_ab.md): the Catphan in its 512^3 of air gains 2.9-3.1 %, the body-sized
// CIRS and thorax phantoms lose 1.7-6 % to the fold and the longer tally service -- they sit below the threshold and keep the atomics.
// With w2 the launch stages wherever the model has a plan, against that default rule: its direct route is two atomics per hit,
// the fold's second pass over the records is cheaper (profiles/tally_variance_ab.md).  MCGPU_TALLY_STAGE=0 still forces the atomics.
bool TallyStage::wanted(const DeviceModel& D, bool has_w2) const {
  if (cursor < 0 || D.knobs.tally_stage == 0) return false;
  if (has_w2 || D.knobs.tally_stage > 0) return true;
  return D.brick_count > 0 && 100LL * D.bricks_exterior >= (long long)kStageExteriorPercent * D.brick_count;
}

// Buffers and launch arguments of one staged (sub-)launch of `blocks` workgroups and A.count histories.  The buffers belong to the
// device model, are allocated at the first staged launch and only grow (launches of one context share them, as they share the id
// dispensers: one launch at a time).  An allocation that fails leaves this and every later launch on the direct atomics.
void TallyStage::prepare(DeviceModel& D, unsigned long long detector_words, TrackArgs& A, int blocks, hipStream_t stream) {
  if (alloc_failed || blocks <= 0) return;
  const TallyStagePlan P = tally_stage_plan(detector_words, A.count, (unsigned int)blocks, bins, (unsigned int)D.knobs.stage_cap);
  if (P.n_bins == 0u || P.n_bins != bins) return;
  const size_t counts_needed = (size_t)blocks * P.n_bins * 4;
  try {
    if (!fallback) fallback = D.put(std::vector<unsigned long long>(2, 0ULL));
    if (counts_needed > counts_bytes) {
      if (counts) { D.mem.free(counts); counts = nullptr; counts_bytes = 0; }
      counts = (unsigned int*)D.mem.device_bytes(counts_needed);
      counts_bytes = counts_needed;
    }
    if (P.bytes > region_bytes) {
      if (region) { D.mem.free(region); region = nullptr; region_bytes = 0; }
      region = (unsigned long long*)D.mem.device_bytes((size_t)P.bytes);
      region_bytes = (size_t)P.bytes;
    }
  } catch (const Error&) {
    (void)hipGetLastError();
    alloc_failed = true;
    return;
  }
  StageArgs S{};
  S.region = region; S.counts = counts; S.fallback = fallback;
  S.pixels = P.pixels; S.n_bins = P.n_bins; S.magic = P.magic; S.bin_pixels = P.bin_pixels; S.cap = P.cap;
  S.cursor = cursor;
  if (!fold_ready) {
    HIP_TRY(prepare_tally_fold(S));
    fold_ready = true;
  }
  // `counts` is not cleared: every launched workgroup overwrites all its entries behind its final barrier (stage_counts_publish),
  // and the fold reads the entries of the launched workgroups only
  plan = P;
  A.stage = S;
}

// `bytes` of the model's device memory once the device is idle
static void read_back(const DeviceModel& D, void* host, const void* device, size_t bytes) {
  HIP_TRY(hipSetDevice(D.device_id));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(host, device, bytes, hipMemcpyDeviceToHost));
}

// hits that took the direct atomic since the context was created
unsigned long long TallyStage::fallback_hits(const DeviceModel& D) const {
  unsigned long long n = 0;
  if (fallback) read_back(D, &n, fallback, 8);
  return n;
}

// test support (downloads the counts table): records the last staged (sub-)launch stored (its hits = these + its share of the fallback hits)
unsigned long long TallyStage::staged_hits(const DeviceModel& D) const {
  unsigned long long n = 0;
  const size_t words = (size_t)plan.workgroups * plan.n_bins;
  if (counts && words != 0) {
    std::vector<unsigned int> c(words);
    read_back(D, c.data(), counts, words * 4);
    for (unsigned int v : c) n += v;
  }
  return n;
}

namespace {

void launch_compat(mcgpu_ctx& C, TrackArgs& A, hipStream_t stream) {
  DeviceModel& D = C.dev;
  require(A.hpt > 0, -2, "!!ERROR!! mcgpu_launch_projection: histories per thread must be positive in COMPAT mode");
  require(A.seed > 0 && A.seed < 2147483399, -2, "!!ERROR!! mcgpu_launch_projection: RANECU seed out of range");
  const unsigned long long blocks = (A.count + kTrackBlockThreads - 1) / kTrackBlockThreads;
  require(blocks <= 0x7fffffffULL, -2, "!!ERROR!! mcgpu_launch_projection: too many batches");
  if (D.knobs.compat_stats) {  // diagnostic build only (-DMC_COMPAT_STATS): the kernel's wave-level counters
    if (!D.stats) D.stats = D.put(std::vector<unsigned long long>(kNumStats + 3 * kWaveTrace, 0ULL));
    A.stats = D.stats;
  }
  HIP_TRY(launch_track_compat(A, (int)blocks, stream));
}

// The persistent grid of a FAST launch: exactly the resident workgroups (an over-subscribed grid would run a second, thin round), one
// size for all instantiations of the context -- asked of the f32 and f64 kernels at the first launch, of their w2 instantiations at the
// first launch with a w2, never of the diagnostic kernel.  No environment read and no synchronisation here: the scheduler's parameters
// were uploaded by apply_schedule.
unsigned long long resident_workgroups(DeviceModel& D, const TrackArgs& A, bool has_w2) {
  const auto fewest = [&A](const FastKernels& f32, const FastKernels& f64) { return std::min(f32.occupancy(A), f64.occupancy(A)); };
  if (D.resident_fast <= 0) {
    D.resident_fast = D.knobs.blocks_per_cu > 0 ? D.knobs.blocks_per_cu : fewest(fast_kernels<0, 0, 0>(), fast_kernels<1, 0, 0>());
    if (D.resident_fast <= 0) D.resident_fast = 1;
    D.resident_covers_w2 = false;
  }
  if (has_w2 && !D.resident_covers_w2) {
    if (D.knobs.blocks_per_cu <= 0) D.resident_fast = std::max(1, std::min(D.resident_fast, fewest(fast_kernels<0, 1, 0>(), fast_kernels<1, 1, 0>())));
    D.resident_covers_w2 = true;
  }
  unsigned long long resident = (unsigned long long)D.num_cus * (unsigned long long)D.resident_fast;
  resident += resident * (unsigned long long)D.knobs.grid_spare_percent / 100ULL;  // spare workgroups: see the kernel's prologue
  return resident;
}

const FastKernels& kernels_of(int mode, bool has_w2) {
  if (mode == MCGPU_MODE_FAST_STATS) return fast_kernels<0, 1, 1>();  // one diagnostic kernel, with and without a w2
  if (mode == MCGPU_MODE_FAST_F64) return has_w2 ? fast_kernels<1, 1, 0>() : fast_kernels<1, 0, 0>();
  return has_w2 ? fast_kernels<0, 1, 0>() : fast_kernels<0, 0, 0>();
}

// Staged detector tally (tally_stage.hpp): the launch is cut into sub-launches of at most the knob's limit -- history ids are
// explicit (first + id), so a cut cannot move a result -- and each is followed by its fold, in this stream and inside the events.
void launch_fast(mcgpu_ctx& C, TrackArgs& A, int mode, hipStream_t stream) {
  DeviceModel& D = C.dev;
  const bool has_w2 = A.w2 != nullptr;
  const FastKernels& K = kernels_of(mode, has_w2);
  const unsigned long long resident = resident_workgroups(D, A, has_w2);
  A.work_counter = D.work_counter;
  const unsigned long long first = A.first, count = A.count;
  // the kernels draw their tickets from the low dword of a counter (id_tickets.hpp): 2^40 histories are 2^26 tickets per counter
  require(count <= (1ULL << 40), -2, "!!ERROR!! mcgpu_launch_projection: more than 2^40 histories in one FAST launch");
  const bool staged = D.stage.wanted(D, has_w2);
  const unsigned long long limit = staged ? D.knobs.stage_max_histories : count;
  const unsigned long long n_sub = staged ? stage_sub_launches(count, limit) : 1ULL;
  for (unsigned long long k = 0; k < n_sub; ++k) {
    stage_sub_launch(first, count, limit, k, A.first, A.count);
    const int blocks = (int)std::min((A.count + kPoolBlockThreads - 1) / kPoolBlockThreads, resident);
    HIP_TRY(hipMemsetAsync(D.work_counter, 0, (size_t)kNumCounters * kCounterStride * 8, stream));  // the ticket counters and their exhaustion mask
    A.stage = StageArgs{};
    if (staged) D.stage.prepare(D, 4ULL * (unsigned long long)C.host.detector[0].total_pixels, A, blocks, stream);  // leaves A.stage.region null where the buffers cannot be had
    if (mode == MCGPU_MODE_FAST_STATS) {
      if (!D.stats) D.stats = D.put(std::vector<unsigned long long>(kNumStats + 3 * kWaveTrace, 0ULL));
      A.stats = D.stats;
    }
    HIP_TRY(K.launch(A, blocks, stream));
    if (A.stage.region != nullptr) {
      HIP_TRY(launch_tally_fold(A.stage, (unsigned int)blocks, A.image, stream));
      if (has_w2) HIP_TRY(launch_tally_fold_squares(A.stage, (unsigned int)blocks, A.w2, stream));
    }
  }
}

}  // namespace
}  // namespace mcgpu

extern "C" {

// The plan of the staged tally for a detector of `detector_words` tally words, a launch of `histories` and `workgroups` workgroups
// (`bins` = 0: the engine's own choice): out6 = {bins, words per bin, bin pixels, capacity, bytes, sub-launches at `limit`}.  Pure host
// arithmetic: works without a context and on one created with device = -1.
int mcgpu_tally_stage_plan(const mcgpu_ctx* ctx, unsigned long long detector_words, unsigned long long histories, int workgroups, int bins,
                           unsigned long long limit, unsigned long long* out6) {
  ABI_BEGIN
  (void)ctx;
  require(out6 && workgroups > 0 && bins >= 0 && limit > 0, -1, "!!ERROR!! mcgpu_tally_stage_plan: bad argument");
  const TallyStagePlan P = tally_stage_plan(detector_words, std::min(histories, limit), (unsigned int)workgroups, (unsigned int)bins, 0u);
  out6[0] = P.n_bins; out6[1] = P.words_per_bin; out6[2] = P.bin_pixels; out6[3] = P.cap; out6[4] = P.bytes;
  out6[5] = stage_sub_launches(histories, limit);
  return 0;
  ABI_END
}

// Tally words first .. first + n - 1 of that plan -> bin and bin-relative word (the mapping the kernels use, tally_stage.hpp)
int mcgpu_tally_stage_map(unsigned long long detector_words, int bins, unsigned long long first, unsigned long long n, unsigned int* bin_out,
                          unsigned int* rel_out) {
  ABI_BEGIN
  require(bin_out && rel_out && bins >= 0 && first + n <= detector_words, -1, "!!ERROR!! mcgpu_tally_stage_map: bad argument");
  const TallyStagePlan P = tally_stage_plan(detector_words, 1, 1, (unsigned int)bins, 0u);
  require(P.n_bins != 0u, -2, "!!ERROR!! mcgpu_tally_stage_map: no staging plan for this detector");
  for (unsigned long long i = 0; i < n; ++i) {
    stage_map((unsigned int)(first + i), P.pixels, P.n_bins, P.magic, P.bin_pixels, bin_out[i], rel_out[i]);
    require(stage_unmap(bin_out[i], rel_out[i], P.pixels, P.n_bins, P.bin_pixels) == (unsigned int)(first + i), -9,
            "!!ERROR!! internal: stage_map and stage_unmap disagree");
  }
  return 0;
  ABI_END
}

// Sub-launch k of a staged launch: its range of histories
int mcgpu_tally_stage_sub_launch(unsigned long long first, unsigned long long count, unsigned long long limit, unsigned long long k,
                                 unsigned long long* sub_first, unsigned long long* sub_count) {
  ABI_BEGIN
  require(sub_first && sub_count && limit > 0, -1, "!!ERROR!! mcgpu_tally_stage_sub_launch: bad argument");
  stage_sub_launch(first, count, limit, k, *sub_first, *sub_count);
  return 0;
  ABI_END
}

// Tickets first_ticket .. first_ticket + n - 1 of id dispenser `counter` in a FAST launch of `count` histories (id_tickets.hpp, the
// functions the kernels use): ids lo_out[i] .. hi_out[i] - 1 of the launch, lo == hi for a ticket past the dispenser's last.
// *n_tickets (may be null): the dispenser's non-empty tickets.
int mcgpu_id_tickets(unsigned long long count, int counter, unsigned long long first_ticket, unsigned long long n, unsigned long long* lo_out,
                     unsigned long long* hi_out, unsigned long long* n_tickets) {
  ABI_BEGIN
  require(counter >= 0 && counter < kNumCounters && (n == 0 || (lo_out && hi_out)), -1, "!!ERROR!! mcgpu_id_tickets: bad argument");
  unsigned long long base, size;
  id_counter_part(count, (unsigned int)counter, base, size);
  for (unsigned long long i = 0; i < n; ++i) {
    id_ticket_range(size, first_ticket + i, lo_out[i], hi_out[i]);
    lo_out[i] += base;
    hi_out[i] += base;
  }
  if (n_tickets) *n_tickets = id_ticket_count(size);
  return 0;
  ABI_END
}

// The dispenser a wave asks after `counter` given the exhaustion mask `mask` (id_tickets.hpp), or the number of dispensers when none is left
int mcgpu_id_next_counter(unsigned long long mask, int counter) {
  if (counter < 0 || counter >= kNumCounters) return -1;
  return (int)id_next_counter(mask, (unsigned int)counter);
}

int mcgpu_launch_projection(mcgpu_ctx* ctx, int p, int mode, int seed, unsigned long long first, unsigned long long count, int hpt,
                            void* image_dev, void* hip_stream) {
  return mcgpu_launch_projection_w2(ctx, p, mode, seed, first, count, hpt, image_dev, nullptr, hip_stream);
}

// The launch, with the tally of squared weights `w2_dev` beside the image (tally_stage.hpp; null: none).
int mcgpu_launch_projection_w2(mcgpu_ctx* ctx, int p, int mode, int seed, unsigned long long first, unsigned long long count, int hpt,
                               void* image_dev, void* w2_dev, void* hip_stream) {
  ABI_BEGIN
  require(ctx && ctx->has_device, -1, "!!ERROR!! mcgpu_launch_projection: the context has no device (created with device_id < 0)");
  require(p >= 0 && p < ctx->host.cfg.num_projections, -1, "!!ERROR!! mcgpu_launch_projection: projection index out of range");
  require(image_dev != nullptr, -1, "!!ERROR!! mcgpu_launch_projection: null image buffer");
  require(mode == MCGPU_MODE_FAST || mode == MCGPU_MODE_COMPAT || mode == MCGPU_MODE_FAST_STATS || mode == MCGPU_MODE_FAST_F64, -1, "!!ERROR!! mcgpu_launch_projection: unknown mode");
  DeviceModel& D = ctx->dev;
  HIP_TRY(hipSetDevice(D.device_id));
  hipStream_t stream = (hipStream_t)hip_stream;
  TrackArgs A = make_args(*ctx, p);
  A.image = (unsigned long long*)image_dev;
  A.w2 = (unsigned long long*)w2_dev;
  A.seed = seed; A.hpt = hpt; A.first = first; A.count = count;
  HIP_TRY(hipEventRecord(D.ev_start, stream));
  if (count > 0) {
    if (mode == MCGPU_MODE_COMPAT) launch_compat(*ctx, A, stream);
    else launch_fast(*ctx, A, mode, stream);
  }
  HIP_TRY(hipEventRecord(D.ev_stop, stream));
  D.timed = true;
  return 0;
  ABI_END
}

int mcgpu_set_fast_schedule(mcgpu_ctx* ctx, int thresh_compton, int thresh_rayleigh, int thresh_new, int flyable_low, int swap_batch) {
  ABI_BEGIN
  require(ctx && ctx->has_device, -1, "!!ERROR!! mcgpu_set_fast_schedule: no device context");
  require(thresh_compton >= 1 && thresh_rayleigh >= 1 && thresh_new >= 1 && flyable_low >= 1 && swap_batch >= 1 && thresh_compton <= 64 &&
              thresh_rayleigh <= 64 && thresh_new <= 64 && flyable_low <= 64 && swap_batch <= 64,
          -2, "!!ERROR!! mcgpu_set_fast_schedule: thresholds are lane counts in 1..64");
  const int v[5] = {thresh_compton, thresh_rayleigh, thresh_new, flyable_low, swap_batch};
  for (int k = 0; k < 5; ++k) ctx->dev.sched[k] = v[k];
  ctx->dev.sched_set = true;
  apply_schedule(ctx->dev);
  return 0;
  ABI_END
}

int mcgpu_reload_env_knobs(mcgpu_ctx* ctx) {
  ABI_BEGIN
  require(ctx && ctx->has_device, -1, "!!ERROR!! mcgpu_reload_env_knobs: no device context");
  const int sched_kind = ctx->dev.knobs.fast_sched;  // fixed when the model was uploaded (it shapes the LDS image)
  read_env_knobs(ctx->dev);
  ctx->dev.knobs.fast_sched = sched_kind;
  ctx->dev.resident_fast = 0;  // MCGPU_BLOCKS_PER_CU may have changed: asked again at the next launch
  apply_schedule(ctx->dev);
  return 0;
  ABI_END
}

int mcgpu_scheduler_stats_ex(mcgpu_ctx* ctx, unsigned long long* out, int capacity, int reset) {
  ABI_BEGIN
  require(ctx && ctx->has_device && out && capacity > 0, -1, "!!ERROR!! mcgpu_scheduler_stats: bad argument");
  HIP_TRY(hipSetDevice(ctx->dev.device_id));
  const int n = std::min(capacity, kNumStats + 3 * kWaveTrace);  // counters, then the wave trace (device_model.hpp)
  for (int k = 0; k < capacity; ++k) out[k] = 0;
  if (!ctx->dev.stats) return 0;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, ctx->dev.stats, (size_t)n * 8, hipMemcpyDeviceToHost));
  if (reset) HIP_TRY(hipMemset(ctx->dev.stats, 0, (size_t)(kNumStats + 3 * kWaveTrace) * 8));
  return 0;
  ABI_END
}

int mcgpu_scheduler_stats(mcgpu_ctx* ctx, unsigned long long* out8, int reset) { return mcgpu_scheduler_stats_ex(ctx, out8, 8, reset); }

int mcgpu_last_kernel_ms(mcgpu_ctx* ctx, float* ms) {
  ABI_BEGIN
  require(ctx && ctx->has_device && ms, -1, "!!ERROR!! mcgpu_last_kernel_ms: bad argument");
  require(ctx->dev.timed, -1, "!!ERROR!! mcgpu_last_kernel_ms: nothing launched yet");
  HIP_TRY(hipEventSynchronize(ctx->dev.ev_stop));
  HIP_TRY(hipEventElapsedTime(ms, ctx->dev.ev_start, ctx->dev.ev_stop));
  return 0;
  ABI_END
}

int mcgpu_run_projection(mcgpu_ctx* ctx, int p, int mode, int seed, unsigned long long first, unsigned long long count, int hpt,
                         uint64_t* image_host, double* kernel_seconds, unsigned long long* histories_done) {
  return mcgpu_run_projection_w2(ctx, p, mode, seed, first, count, hpt, image_host, nullptr, kernel_seconds, histories_done);
}

int mcgpu_run_projection_w2(mcgpu_ctx* ctx, int p, int mode, int seed, unsigned long long first, unsigned long long count, int hpt,
                            uint64_t* image_host, uint64_t* w2_host, double* kernel_seconds, unsigned long long* histories_done) {
  ABI_BEGIN
  require(ctx && ctx->has_device && image_host, -1, "!!ERROR!! mcgpu_run_projection: bad argument");
  HIP_TRY(hipSetDevice(ctx->dev.device_id));
  const size_t bytes = (size_t)32 * ctx->host.detector[0].total_pixels;
  if (!ctx->dev.scratch_image) ctx->dev.scratch_image = (unsigned long long*)ctx->dev.put(std::vector<unsigned char>(bytes, 0));  // kept for the next call
  if (w2_host && !ctx->dev.scratch_w2) ctx->dev.scratch_w2 = (unsigned long long*)ctx->dev.put(std::vector<unsigned char>(bytes, 0));
  void* img = ctx->dev.scratch_image;
  void* w2 = w2_host ? ctx->dev.scratch_w2 : nullptr;
  HIP_TRY(hipMemset(img, 0, bytes));
  if (w2) HIP_TRY(hipMemset(w2, 0, bytes));
  int rc = mcgpu_launch_projection_w2(ctx, p, mode, seed, first, count, hpt, img, w2, nullptr);
  if (rc == 0) {
    float ms = 0.f;
    rc = mcgpu_last_kernel_ms(ctx, &ms);
    if (kernel_seconds) *kernel_seconds = ms * 1e-3;
    HIP_TRY(hipMemcpy(image_host, img, bytes, hipMemcpyDeviceToHost));
    if (w2) HIP_TRY(hipMemcpy(w2_host, w2, bytes, hipMemcpyDeviceToHost));
    if (histories_done) *histories_done = (mode == MCGPU_MODE_COMPAT) ? count * (unsigned long long)hpt : count;
  }
  return rc;
  ABI_END
}

}  // extern "C"
