// scan.cpp -- mcgpu_run_scan / mcgpu_run_scan_multi: the projection loop of main() (docker/mcgpu/MC-GPU_v1.3.cu:667-1056)
// as a device/host pipeline, written on top of the engine's own C ABI.
//
// Reference flow per projection, all on one host thread per rank: kernel -> D2H of the 45 MB tally -> MPI_Reduce to rank 0
// (:1019) -> ~0.9 s of fprintf -> re-zero.  Here every device has ONE tracking stream and everything it does is ordered on it;
// the sum of the per-device tallies is the tally exchange of exchange.cpp (the same code bench.py's ranks run, here between
// contexts of one process):
//   every device : begin(i) -> track kernel for its shard of projection i -> submit(i): devices that do not own projection i
//                  push their tally to the owner with a copy engine while projection i + 1 is tracked
//   owner of i-1 : collect(i - 1) behind its kernel i: one fused add of the landed tallies -> [ASCII text formatted on the
//                  device, only when the files are wanted] -> finalize kernel (float32 planes) -> copy of the planes (9 MB)
//                  to one of two pinned buffers -> event
//   writer thread : waits on the event, appends the planes to the three MetaImage stacks, hands the ASCII text to its worker.
// The owner rotates over the devices (projection i belongs to device i mod N; MCGPU_EXCHANGE_POLICY=0: always the first
// device, the reference's root): the only work that is exposed on a tracking stream -- the fused add, finalize -- is spread
// evenly, and so are the xGMI links.  The one-projection lag means no owner ever waits for a push (it had a whole kernel's
// time to land), and nothing ever runs BESIDE a tracking launch: a kernel that is still resident while the persistent tracking
// grid is dispatched fragments the CUs' register files for that whole launch (144 of 256 CUs then hold one workgroup instead
// of two: 9.2 -> 12.5 ms, tools/placement_probe.py).  With one device the lag is zero.
// History sharding keeps per-history RNG streams and integer tallies, so the result is identical for any number of
// devices (tests run several "devices" on one).
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <strings.h>
#include <thread>
#include <vector>

#include "../../include/mcgpu_amd.h"
#include "hip_host.hpp"
#include "knobs.hpp"
using mcgpu::knob_set;
using mcgpu::knob_str;

namespace {

using mcgpu::DeviceBuffer;
using mcgpu::Error;
using mcgpu::Event;
using mcgpu::PinnedBuffer;
using mcgpu::Stream;

constexpr int kAsciiSlots = MCGPU_ASCII_SLOTS;
constexpr int kExchangeUnavailable = -7;  // the devices of a multi-device scan cannot reach each other (set-up phase only)
constexpr int kRcclUnavailable = -8;      // the RCCL route cannot be set up on these devices (set-up phase only)

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

#define ABI_OK(expr)                                             \
  do {                                                           \
    const int _rc = (expr);                                      \
    if (_rc != 0) throw Error(_rc, std::string(mcgpu_last_error())); \
  } while (0)

// ---- what both sharding paths derive from the contexts' configuration and the options, validated once
struct ScanPlan {
  std::vector<mcgpu_ctx*> ctxs;  // ctxs[0]: configuration, file names, calibration
  std::vector<int> devs;         // device of every context
  int mode = MCGPU_MODE_FAST, first = 0, range = 0, phase = 0;
  long long nproj_all = 1, hist_in = 0, seed = 0, tpb = 128, hpt = 150, nx = 0, nz = 0, fast_scheduler = 0;
  double d_angle = -1.0, angle0 = 0.0, roi0 = 0.0, roi1 = 0.0;
  bool by_time = false;  // the input's history count is a time budget in seconds per projection
  // offsets within the range of the projections this scan simulates, and their ordinal among ALL simulated projections of the
  // trajectory (a projection-sharded scan takes every stride-th of them: the COMPAT seed still moves on once per simulated
  // projection, whoever simulates it)
  std::vector<int> sim, ord;
  int cx = 0;                   // columns of the stacks (half-fan crop)
  size_t words = 0, plane = 0;  // uint64 words of one tally, floats of one cropped plane
  // write_variance: the squared weights (mcgpu_launch_projection_w2) live directly behind the image in the same allocation -- one
  // buffer of 2 x words that is zeroed, and would be exchanged, as one -- and the three variance planes directly behind the three planes
  bool variance = false;
  size_t tally_words() const { return variance ? 2 * words : words; }
  size_t planes() const { return variance ? 6 : 3; }
  double sx = 0.0, sy = 0.0;    // MetaImage spacing
  std::string folder;

  int count() const { return (int)sim.size(); }
  // projections outside the input's angular region of interest are not simulated (MC-GPU_v1.3.cu:670-677; like the
  // reference, the test uses initial_angle + p * D_angle even when specific angles are given)
  bool outside_roi(int p) const {
    const double a = angle0 + p * d_angle;
    return a < roi0 || a > roi1;
  }
};

// Checks in this order: the mode, the devices, then the range and the stride / phase.
ScanPlan plan_scan(mcgpu_ctx* const* ctxs, int n_ctx, const mcgpu_scan_options* opt) {
  if (opt->mode != MCGPU_MODE_FAST && opt->mode != MCGPU_MODE_COMPAT && opt->mode != MCGPU_MODE_FAST_F64)
    throw Error(-1, "!!ERROR!! mcgpu_run_scan: unknown mode " + std::to_string(opt->mode) +
                        " (MCGPU_MODE_FAST, MCGPU_MODE_COMPAT or MCGPU_MODE_FAST_F64)");
  ScanPlan s;
  s.mode = opt->mode;
  s.ctxs.assign(ctxs, ctxs + n_ctx);
  for (mcgpu_ctx* c : s.ctxs) {
    long long dev = -1;
    ABI_OK(mcgpu_config_i64(c, "device_id", &dev));
    if (dev < 0) throw Error(-1, "!!ERROR!! mcgpu_run_scan: a context has no device");
    s.devs.push_back((int)dev);
  }
  mcgpu_ctx* const ctx = ctxs[0];
  double px_x = 0, px_z = 0;
  const std::pair<const char*, long long*> i64[] = {{"num_projections", &s.nproj_all}, {"total_histories", &s.hist_in}, {"seed", &s.seed},
      {"threads_per_block", &s.tpb}, {"histories_per_thread", &s.hpt}, {"num_pixels_x", &s.nx}, {"num_pixels_z", &s.nz}, {"fast_scheduler", &s.fast_scheduler}};
  const std::pair<const char*, double*> f64[] = {{"pixel_size_x_mm", &px_x}, {"pixel_size_z_mm", &px_z}, {"D_angle", &s.d_angle},
      {"initial_angle", &s.angle0}, {"angularROI_0", &s.roi0}, {"angularROI_1", &s.roi1}};
  for (const auto& c : i64) ABI_OK(mcgpu_config_i64(ctx, c.first, c.second));
  for (const auto& c : f64) ABI_OK(mcgpu_config_f64(ctx, c.first, c.second));
  s.first = opt->first_projection > 0 ? opt->first_projection : 0;
  s.range = (opt->num_projections > 0) ? opt->num_projections : (int)s.nproj_all - s.first;
  if (s.first + s.range > s.nproj_all || s.range <= 0) throw Error(-1, "!!ERROR!! mcgpu_run_scan: projection range outside the trajectory");
  const int stride = opt->projection_stride > 1 ? opt->projection_stride : 1;
  s.phase = stride > 1 ? opt->projection_phase : 0;
  if (s.phase < 0 || s.phase >= stride) throw Error(-1, "!!ERROR!! mcgpu_run_scan: projection_phase outside [0, projection_stride)");
  if (opt->shared_stacks && !opt->slice_of_projection) throw Error(-1, "!!ERROR!! mcgpu_run_scan: shared_stacks needs slice_of_projection");
  int before = 0;  // simulated projections of the trajectory before the range
  for (int p = 0; p < s.first; ++p) before += !s.outside_roi(p);
  for (int k = 0, n_sim = 0; k < s.range; ++k)
    if (!s.outside_roi(s.first + k)) {
      if (n_sim % stride == s.phase) { s.sim.push_back(k); s.ord.push_back(before + n_sim); }
      ++n_sim;
    }
  s.by_time = !opt->histories_per_projection && s.hist_in < 95000;
  s.cx = (opt->crop_nx > 0 && opt->crop_nx < s.nx) ? opt->crop_nx : (int)s.nx;
  s.words = (size_t)4 * s.nx * s.nz;
  s.plane = (size_t)s.cx * s.nz;
  s.variance = opt->write_variance != 0;
  s.sx = opt->pixel_spacing_x > 0 ? opt->pixel_spacing_x : px_x;
  s.sy = opt->pixel_spacing_y > 0 ? opt->pixel_spacing_y : px_z;
  if (opt->output_folder) s.folder = opt->output_folder;
  else {
    char name[1024];
    ABI_OK(mcgpu_projection_file_name(ctx, 0, name, sizeof name));
    s.folder = name;
    const size_t slash = s.folder.find_last_of('/');
    s.folder = slash == std::string::npos ? "." : s.folder.substr(0, slash);
  }
  return s;
}

// Launch shape of H histories per projection: COMPAT rounds to the reference's grid and launches blocks * tpb units.
struct Shape { int blocks, hpt; unsigned long long total, units; };
Shape launch_shape(const ScanPlan& plan, unsigned long long H) {
  Shape s{1, (int)plan.hpt, H, H};
  if (plan.mode == MCGPU_MODE_COMPAT) {
    ABI_OK(mcgpu_launch_shape(H, (int)plan.tpb, (int)plan.hpt, &s.blocks, &s.hpt, &s.total));
    s.units = (unsigned long long)s.blocks * (unsigned long long)plan.tpb;
  }
  return s;
}

// An input history count below 95000 is a time budget in seconds per projection (MC-GPU_v1.3.cu:650-655, :689-809: the reference
// runs a speed test and converts).  Two throw-away launches on the first device measure its rate.  n_share devices share every
// projection's histories (their rates add up); `per_device`: every device simulates whole projections alone.
unsigned long long budget_histories(const ScanPlan& plan, hipStream_t stream, int n_share, bool per_device, bool progress) {
  const unsigned long long probe = 4000000ULL;
  const unsigned long long probe_units = plan.mode == MCGPU_MODE_COMPAT ? (probe + (unsigned long long)plan.hpt - 1) / (unsigned long long)plan.hpt : probe;
  DeviceBuffer tally;
  float ms = 0.f;
  HIP_TRY(hipSetDevice(plan.devs[0]));
  HIP_TRY(hipMalloc(tally.make(plan.devs[0]), plan.words * 8));
  HIP_TRY(hipMemsetAsync(tally, 0, plan.words * 8, stream));
  for (int rep = 0; rep < 2; ++rep) {  // the first launch pays one-off costs
    ABI_OK(mcgpu_launch_projection(plan.ctxs[0], plan.first, plan.mode, (int)plan.seed, 0, probe_units, (int)plan.hpt, tally, stream));
    ABI_OK(mcgpu_last_kernel_ms(plan.ctxs[0], &ms));
  }
  ABI_OK(mcgpu_dose_clear(plan.ctxs[0]));
  HIP_TRY(hipStreamSynchronize(stream));
  const double rate = (double)probe / (ms > 0.f ? ms * 1e-3 : 1e-3) * n_share;
  const unsigned long long H = std::max(100000ULL, (unsigned long long)(rate * (double)plan.hist_in));
  if (progress) {
    printf("       Time-limited run: %lld s per projection at %.3e x-rays/s%s -> %llu histories per projection\n", plan.hist_in, rate,
           per_device ? " per device" : "", per_device ? H : launch_shape(plan, H).total);
    fflush(stdout);
  }
  return H;
}

// FAST batching thresholds: a few presets timed with throw-away launches on the first simulated projection (the best one
// differs between geometries by 5-7 %; the tallies do not depend on the choice), then set on every context.  Skipped for short
// scans and when the environment pins the knobs; the presets are per-wave pool thresholds, the workgroup-level pool
// (fast_scheduler) keeps its own defaults.
void choose_fast_preset(const ScanPlan& plan, unsigned long long total, hipStream_t stream, bool progress) {
  if (plan.mode == MCGPU_MODE_COMPAT || plan.fast_scheduler != 0 || total < 20000000ULL || knob_set("MCGPU_THRESH_COMPTON") ||
      knob_set("MCGPU_THRESH_NEW") || knob_set("MCGPU_SWAP_BATCH") || knob_set("MCGPU_NO_AUTOTUNE"))
    return;
  static const int presets[3][5] = {{40, 12, 44, 12, 40}, {32, 8, 36, 12, 40}, {36, 16, 44, 12, 44}};  // profiles/r05o_*, r05p_*
  const unsigned long long probe = 6000000ULL;
  mcgpu_ctx* const ctx = plan.ctxs[0];
  const int p = plan.first + (plan.count() > 0 ? plan.sim[0] : 0);
  DeviceBuffer tally;
  HIP_TRY(hipSetDevice(plan.devs[0]));
  HIP_TRY(hipMalloc(tally.make(plan.devs[0]), plan.words * 8));
  HIP_TRY(hipMemsetAsync(tally, 0, plan.words * 8, stream));
  int best = 0;
  float best_ms = 1e30f;
  for (int c = 0; c < 3; ++c) {
    ABI_OK(mcgpu_set_fast_schedule(ctx, presets[c][0], presets[c][1], presets[c][2], presets[c][3], presets[c][4]));
    float ms = 0.f, fastest = 1e30f;
    for (int rep = 0; rep < 3; ++rep) {  // the first launch of a preset pays the parameter upload
      ABI_OK(mcgpu_launch_projection(ctx, p, plan.mode, (int)plan.seed, 0, probe, (int)plan.hpt, tally, stream));
      ABI_OK(mcgpu_last_kernel_ms(ctx, &ms));
      if (rep > 0 && ms < fastest) fastest = ms;
    }
    if (fastest < best_ms) { best_ms = fastest; best = c; }
  }
  for (mcgpu_ctx* c : plan.ctxs) ABI_OK(mcgpu_set_fast_schedule(c, presets[best][0], presets[best][1], presets[best][2], presets[best][3], presets[best][4]));
  HIP_TRY(hipSetDevice(plan.devs[0]));
  ABI_OK(mcgpu_dose_clear(ctx));
  if (progress) {
    printf("       FAST batching preset %d of 3 (thresholds %d/%d/%d, %d, %d)\n", best + 1, presets[best][0], presets[best][1], presets[best][2],
           presets[best][3], presets[best][4]);
    fflush(stdout);
  }
  HIP_TRY(hipStreamSynchronize(stream));
}

// f(0), f(1), f(2) side by side (page-cache work on three different files): 0, or the code of the first that failed with its
// message as this thread's last error.
template <class F>
int side_by_side(const F& f) {
  int rc[3] = {0, 0, 0};
  std::string err[3];
  auto one = [&](int k) { if ((rc[k] = f(k)) != 0) err[k] = mcgpu_last_error(); };  // the last error is per thread
  std::thread side[2] = {std::thread(one, 1), std::thread(one, 2)};
  one(0);
  for (auto& t : side) t.join();
  for (int k = 0; k < 3; ++k)
    if (rc[k] != 0) return mcgpu::set_error(rc[k], err[k]);
  return 0;
}

// The scan's own MetaImage stacks {total, unscattered, scattered}: stacks that are not finished are closed when this goes.
struct OutputStacks {
  mcgpu_stack* stack[3] = {nullptr, nullptr, nullptr};
  mcgpu_stack* variance[3] = {nullptr, nullptr, nullptr};  // write_variance: the per-pixel variance of each stack
  ~OutputStacks() {
    for (mcgpu_stack* st : stack)
      if (st) (void)mcgpu_stack_finish(st, 0, nullptr);  // error path: close the files
    for (mcgpu_stack* st : variance)
      if (st) (void)mcgpu_stack_finish(st, 0, nullptr);
  }
  bool open() const { return stack[0] != nullptr; }
  void create(const ScanPlan& plan) {
    static const char* kNames[3] = {"projections_total.mha", "projections_unscattered.mha", "projections_scattered.mha"};
    for (int k = 0; k < 3; ++k) ABI_OK(mcgpu_stack_create((plan.folder + "/" + kNames[k]).c_str(), plan.cx, (int)plan.nz, plan.count(), plan.sx, plan.sy, &stack[k]));
    static const char* kVariance[3] = {"projections_total_variance.mha", "projections_unscattered_variance.mha", "projections_scattered_variance.mha"};
    for (int k = 0; k < 3 && plan.variance; ++k)
      ABI_OK(mcgpu_stack_create((plan.folder + "/" + kVariance[k]).c_str(), plan.cx, (int)plan.nz, plan.count(), plan.sx, plan.sy, &variance[k]));
  }
  // a projection's three planes, side by side (each append scans its plane for zeros and copies it into the page cache)
  int append(const float* planes, size_t plane) {
    if (const int rc = side_by_side([&](int k) { return mcgpu_stack_append(stack[k], planes + (size_t)k * plane); })) return rc;
    if (!variance[0]) return 0;
    return side_by_side([&](int k) { return mcgpu_stack_append(variance[k], planes + (size_t)(3 + k) * plane); });
  }
  // zero replacement and close side by side, then the air normalisation of the total stack
  void finish(const ScanPlan& plan, const mcgpu_scan_options* opt, float repl[3]) {
    mcgpu_stack* st[3] = {stack[0], stack[1], stack[2]};
    stack[0] = stack[1] = stack[2] = nullptr;
    if (const int rc = side_by_side([&](int k) { return mcgpu_stack_finish(st[k], 1, &repl[k]); })) throw Error(rc, mcgpu_last_error());
    if (variance[0]) {  // a variance of zero is a value: no replacement
      mcgpu_stack* sv[3] = {variance[0], variance[1], variance[2]};
      variance[0] = variance[1] = variance[2] = nullptr;
      if (const int rc = side_by_side([&](int k) { return mcgpu_stack_finish(sv[k], 0, nullptr); })) throw Error(rc, mcgpu_last_error());
    }
    if (opt->air_stack)
      ABI_OK(mcgpu_normalize_stack((plan.folder + "/projections_total.mha").c_str(), opt->air_stack, opt->air_sigma_y, opt->air_sigma_x,
                                   (plan.folder + "/projections_total_normalized.mha").c_str(), plan.sx, plan.sy));
  }
};

// The host end of the pipeline.  The writer thread takes the projections in order as they are published: it waits for their
// download, writes the planes to the stacks and the ASCII file (host formatter) or hands the file to the worker of its formatter
// slot.  One worker per slot, so that several files are written side by side (writes to ONE file do not scale with threads --
// they serialise on its inode lock -- writes to different files do).
struct Output {
  struct Projection {                 // what the writer needs of one projection, final when it is published
    int p = 0, offset = 0;            // index in the trajectory; offset within the scan's range
    int dev = -1;                     // the owner device, whose event `downloaded` says the planes (and image) are on the host
    hipEvent_t downloaded = nullptr;
    const float* planes = nullptr;
    const uint64_t* image = nullptr;  // the tally (host ASCII formatter only)
    mcgpu_ctx* formatter = nullptr;   // the context whose formatter slot holds the device-formatted text
    double seconds = 0.0;             // kernel time
  };
  const mcgpu_scan_options* const opt;
  mcgpu_ctx* const ctx;
  const size_t plane;
  OutputStacks* const stacks;
  const bool ascii_on_host = knob_set("MCGPU_ASCII_HOST");  // A/B: the threaded host formatter of report.cpp
  const int n_ascii = [] {  // formatter slots in use = files written side by side
    const char* w = knob_str("MCGPU_ASCII_WRITERS");
    return w ? std::min(std::max(atoi(w), 1), kAsciiSlots) : kAsciiSlots;
  }();
  unsigned long long total = 0;
  std::thread writer, ascii_worker[kAsciiSlots];
  std::mutex mu;  // guards everything below
  std::condition_variable cv;
  std::vector<Projection> queue;
  int queued = 0, written = 0;  // projections handed to / finished by the writer
  bool aborted = false, ascii_quit = false;
  std::string error;
  double busy_s = 0.0;
  bool ascii_busy[kAsciiSlots] = {};
  Projection ascii[kAsciiSlots];

  ~Output() { abort(); }
  void start(int count, unsigned long long total_histories) {
    total = total_histories;
    queue.assign((size_t)count, Projection{});
    if (opt->write_ascii && !ascii_on_host)
      for (int a = 0; a < n_ascii; ++a) ascii_worker[a] = std::thread(&Output::write_ascii, this, a);
    writer = std::thread(&Output::write_all, this);
  }
  // Pinned buffer j & 1 is free once projection j - 2 has been written.  Formatter slot j % n_ascii was last used by projection
  // j - n_ascii: that one must have been HANDED to its worker (the writer sets the slot busy when it has written the
  // projection's stacks, together with `written`) and the worker must be done.  With one slot the previous projection itself is
  // the slot's last user, so `written >= j - 1` is not enough (it would let projection j be formatted over the text of j - 1
  // before j - 1 was even handed over).
  void wait_for_buffers(int j) {
    const int handed = j - std::min(1, n_ascii - 1);
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return (written >= handed && !ascii_busy[j % n_ascii]) || aborted; });
    if (aborted) throw Error(-3, error);
  }
  void publish(int j, const Projection& pr) {
    std::lock_guard<std::mutex> lk(mu);
    queue[(size_t)j] = pr;
    queued = j + 1;
    cv.notify_all();
  }
  // normal end: the writer is done, then every worker finishes the file it holds; the first failure is thrown
  void join() {
    writer.join();
    stop(ascii_quit);
    std::lock_guard<std::mutex> lk(mu);
    if (aborted) throw Error(-3, error);
  }
  void abort() { stop(aborted); }  // error path: the threads stop where they are
  void stop(bool& flag) {
    { std::lock_guard<std::mutex> lk(mu); flag = true; cv.notify_all(); }
    if (writer.joinable()) writer.join();
    for (auto& w : ascii_worker)
      if (w.joinable()) w.join();
  }
  void write_all() {
    for (int i = 0; i < (int)queue.size(); ++i) {
      Projection pr;
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return queued > i || aborted; });
        if (aborted) return;
        pr = queue[(size_t)i];
      }
      if (hipSetDevice(pr.dev) != hipSuccess || hipEventSynchronize(pr.downloaded) != hipSuccess) {
        std::lock_guard<std::mutex> lk(mu);
        error = "!!HIP ERROR!! waiting for projection results";
        aborted = true;
        cv.notify_all();
        return;
      }
      const double tw0 = now_s();
      int wrc = 0;
      if (opt->shared_stacks)
        for (int k = 0; k < 3 && wrc == 0; ++k)
          wrc = mcgpu_stack_write_slice(opt->shared_stacks[k], opt->slice_of_projection[pr.offset], pr.planes + (size_t)k * plane);
      else if (opt->write_stacks)
        wrc = stacks->append(pr.planes, plane);
      if (wrc == 0 && opt->write_ascii && ascii_on_host) wrc = mcgpu_write_projection(ctx, pr.p, pr.image, total, pr.seconds, nullptr);
      std::lock_guard<std::mutex> lk(mu);
      if (wrc == 0 && opt->write_ascii && !ascii_on_host) {  // the slot is free: the projection loop waited for that before it formatted into it
        ascii[i % n_ascii] = pr;
        ascii_busy[i % n_ascii] = true;
      }
      busy_s += now_s() - tw0;
      if (wrc != 0) { error = mcgpu_last_error(); aborted = true; }
      written = i + 1;
      cv.notify_all();
      if (wrc != 0) return;
    }
  }
  void write_ascii(int a) {
    for (;;) {
      Projection pr;
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return ascii_busy[a] || ascii_quit || aborted; });
        if (!ascii_busy[a]) return;
        pr = ascii[a];
      }
      const double tw0 = now_s();
      const int wrc = mcgpu_write_formatted_projection(pr.formatter, pr.p, a, total, pr.seconds, nullptr);
      std::lock_guard<std::mutex> lk(mu);
      busy_s += now_s() - tw0;
      if (wrc != 0) { error = mcgpu_last_error(); aborted = true; }
      ascii_busy[a] = false;
      cv.notify_all();
      if (wrc != 0) return;
    }
  }
};

// One scan over n devices that share every projection's histories (n = 1: the plain single-device pipeline).  `use_rccl`: the
// per-device tallies of a projection are summed by one ncclReduce to the projection's owner (reduce_rccl.cpp) instead of through
// the tally exchange.
struct HistoryScan {
  struct Lane {  // per device
    mcgpu_ctx* ctx = nullptr;
    int dev = -1;
    Stream stream;                        // the tracking stream
    mcgpu_exchange* x = nullptr;          // this device's end of the tally exchange (owns the tally buffers)
    DeviceBuffer planes_dev[2];           // float32 planes of the projections this device owns
    Stream copy;                          // their download: a copy engine, beside the next tracking kernel
    Event finalized[2];                   // planes_dev[b] has been written (tracking stream)
    Event done[2];                        // planes of pinned buffer b are on the host (system-scope release; copy stream)
    bool done_valid[2] = {false, false};
    unsigned long long lo = 0, hi = 0;    // shard of the units of every projection
    // RCCL route (reduce_rccl.cpp): the collective runs on a stream of its own, beside the next projection's kernel
    Stream reduce;
    void* tally[2] = {nullptr, nullptr};  // this device's tally of the projection with that parity
    Event tracked[2];                     // the tracking kernel of that projection has run (tracking stream)
    Event reduced[2];                     // the collective over that tally has run here (reduce stream)
    bool reduced_valid[2] = {false, false};
  };
  const mcgpu_scan_options* const opt;
  const ScanPlan plan;
  const int n;
  const bool use_rccl;
  int policy = MCGPU_EXCHANGE_LOCAL | MCGPU_EXCHANGE_ROTATE;
  Shape shape{};
  std::vector<unsigned char> mailboxes;  // host region of the exchange (contexts of one process: plain memory)
  std::vector<Lane> lanes;
  mcgpu_rccl* rccl = nullptr;
  PinnedBuffer planes_host[2], image_host[2];
  std::vector<float> kms;  // kernel time per projection (final before the projection is published)
  OutputStacks stacks;
  Output out{opt, plan.ctxs[0], plan.plane, &stacks};

  HistoryScan(mcgpu_ctx* const* ctxs, int n_ctx, const mcgpu_scan_options* o, bool rccl_route)
      : opt(o), plan(plan_scan(ctxs, n_ctx, o)), n(n_ctx), use_rccl(rccl_route), lanes((size_t)n_ctx) {
    if (const char* v = knob_str("MCGPU_EXCHANGE_POLICY")) policy = MCGPU_EXCHANGE_LOCAL | (atoi(v) ? MCGPU_EXCHANGE_ROTATE : 0);
    for (int g = 0; g < n; ++g) { lanes[g].ctx = ctxs[g]; lanes[g].dev = plan.devs[g]; }
  }

  // Teardown, error path and normal end alike, in the one order that is safe:
  //   1. stop the writer and ASCII threads, before anything they read is freed;
  //   2. drain every stream of every device;
  //   3. destroy the RCCL communicator;
  //   4. free the buffers and events;
  //   5. destroy the exchange ends -- only now that EVERY device has drained: peers push into their memory;
  //   6. destroy the tracking streams.
  ~HistoryScan() {
    out.abort();
    for (Lane& l : lanes) {
      if (!l.stream) continue;
      (void)hipSetDevice(l.dev);
      for (hipStream_t s : {(hipStream_t)l.stream, (hipStream_t)l.copy, (hipStream_t)l.reduce})
        if (s) (void)hipStreamSynchronize(s);
    }
    if (rccl) mcgpu_rccl_destroy(rccl);
    for (int b = 0; b < 2; ++b) {
      planes_host[b].reset();
      image_host[b].reset();
      for (Lane& l : lanes) { l.planes_dev[b].reset(); l.done[b].reset(); l.finalized[b].reset(); l.tracked[b].reset(); l.reduced[b].reset(); }
    }
    for (Lane& l : lanes) { l.copy.reset(); l.reduce.reset(); }
    for (Lane& l : lanes)
      if (l.x) mcgpu_exchange_destroy(l.x);
    for (Lane& l : lanes) l.stream.reset();
  }

  // Tracking streams and exchange ends; then the route of the sum, tried before anything is simulated or written.
  void connect() {
    const size_t shared_bytes = mcgpu_exchange_shared_bytes(n);
    mailboxes.assign(shared_bytes * (size_t)(use_rccl ? n : 1), 0);
    for (int g = 0; g < n; ++g) {
      Lane& l = lanes[g];
      HIP_TRY(hipSetDevice(l.dev));
      HIP_TRY(hipStreamCreate(l.stream.make(l.dev)));
      if (!use_rccl) {
        ABI_OK(mcgpu_exchange_create(l.dev, g, n, plan.tally_words(), policy, mailboxes.data(), &l.x));
        continue;
      }
      // every device keeps its double-buffered tally in an exchange end of its own (a world of one: begin / submit / collect stay local)
      ABI_OK(mcgpu_exchange_create(l.dev, 0, 1, plan.tally_words(), MCGPU_EXCHANGE_LOCAL, mailboxes.data() + (size_t)g * shared_bytes, &l.x));
      HIP_TRY(hipStreamCreateWithFlags(l.reduce.make(l.dev), hipStreamNonBlocking));
      for (int b = 0; b < 2; ++b) {
        HIP_TRY(hipEventCreateWithFlags(l.tracked[b].make(l.dev), hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(l.reduced[b].make(l.dev), hipEventDisableTiming));
      }
    }
    if (use_rccl) {
      if (mcgpu_rccl_create(plan.devs.data(), n, &rccl) != 0) throw Error(kRcclUnavailable, mcgpu_last_error());
      return;
    }
    try {
      // peer access between every pair of devices, and one small copy-engine transfer into every peer's landing buffer: a node
      // on which either fails is reported with kExchangeUnavailable BEFORE anything has been simulated or written, and
      // mcgpu_run_scan_multi then shards the scan by projection instead (same output bytes, nothing crosses between devices)
      if (n > 1 && knob_set("MCGPU_EXCHANGE_FAIL_PROBE")) throw Error(-1, "!!ERROR!! tally exchange: probe failure requested (MCGPU_EXCHANGE_FAIL_PROBE)");  // test hook
      for (int g = 0; g < n; ++g)
        for (int h = 0; h < n; ++h)
          if (g != h) ABI_OK(mcgpu_exchange_connect_local(lanes[g].x, lanes[h].x));
      for (Lane& l : lanes) ABI_OK(mcgpu_exchange_probe(l.x));
    } catch (const Error& e) {
      throw Error(kExchangeUnavailable, e.what());
    }
  }

  // Download resources of every device that can own a projection, the pinned buffers, and the scan's own stacks.
  void allocate() {
    for (int g = 0; g < n; ++g) {
      if (g > 0 && !(policy & MCGPU_EXCHANGE_ROTATE)) break;
      Lane& l = lanes[g];
      HIP_TRY(hipSetDevice(l.dev));
      HIP_TRY(hipStreamCreateWithFlags(l.copy.make(l.dev), hipStreamNonBlocking));
      for (int b = 0; b < 2; ++b) {
        HIP_TRY(hipEventCreateWithFlags(l.finalized[b].make(l.dev), hipEventDisableTiming));
        HIP_TRY(hipMalloc(l.planes_dev[b].make(l.dev), plan.planes() * plan.plane * 4));
        // the writer thread reads non-coherent pinned memory after waiting on this event: that needs a SYSTEM-scope release,
        // which a default event does not promise (device scope only)
        HIP_TRY(hipEventCreateWithFlags(l.done[b].make(l.dev), hipEventDisableTiming | hipEventReleaseToSystem));
      }
    }
    // non-coherent (CPU-cacheable) pinned memory: the writer thread reads every byte (ordering: see the event above); portable:
    // it is filled from whichever device owns the projection
    const unsigned int pinned_flags = (knob_set("MCGPU_PINNED_COHERENT") ? hipHostMallocDefault : hipHostMallocNonCoherent) | hipHostMallocPortable;
    const int dev0 = lanes[0].dev;
    HIP_TRY(hipSetDevice(dev0));
    for (int b = 0; b < 2; ++b) {
      HIP_TRY(hipHostMalloc(planes_host[b].make(dev0), plan.planes() * plan.plane * 4, pinned_flags));
      if (opt->write_ascii && out.ascii_on_host) HIP_TRY(hipHostMalloc(image_host[b].make(dev0), plan.words * 8, pinned_flags));
    }
    if (opt->write_stacks && !opt->shared_stacks && plan.count() > 0) stacks.create(plan);
  }

  int owner_of(int j) const {  // the device that holds the summed tally of projection j, finalizes and downloads it
    return use_rccl ? ((policy & MCGPU_EXCHANGE_ROTATE) ? j % n : 0) : mcgpu_exchange_owner(lanes[0].x, j);
  }

  // Every device tracks its shard of projection i into a zeroed tally buffer; the devices that do not own the projection then
  // push theirs to the owner (copy engine, beside the next projection's kernel).
  void track(int i, int seed) {
    const int b = i & 1, p = plan.first + plan.sim[i];
    for (Lane& l : lanes) {
      HIP_TRY(hipSetDevice(l.dev));
      void* tally = nullptr;
      if (use_rccl && l.reduced_valid[b]) HIP_TRY(hipStreamWaitEvent(l.stream, l.reduced[b], 0));  // begin() zeroes the buffer the collective of i - 2 read
      ABI_OK(mcgpu_exchange_begin(l.x, i, l.stream, &tally));
      void* const w2 = plan.variance ? (void*)((unsigned long long*)tally + plan.words) : nullptr;
      ABI_OK(mcgpu_launch_projection_w2(l.ctx, p, plan.mode, seed, l.lo, l.hi - l.lo, shape.hpt, tally, w2, l.stream));
      ABI_OK(mcgpu_exchange_submit(l.x, i, l.stream));
      if (use_rccl) {
        l.tally[b] = tally;
        HIP_TRY(hipEventRecord(l.tracked[b], l.stream));
      }
    }
  }

  // Sum + finalize of projection j on its owner's tracking stream, then the download of its planes.
  void reduce_and_download(int j) {
    const int b = j & 1, o = owner_of(j);
    out.wait_for_buffers(j);
    if (use_rccl) {
      // one ncclReduce(uint64, sum, root = owner) over the devices' tallies of projection j (the reference's MPI_Reduce,
      // MC-GPU_v1.3.cu:1019), on the reduce streams: behind kernel j of each device, beside its kernel j + 1
      std::vector<void*> bufs((size_t)n), streams((size_t)n);
      for (int g = 0; g < n; ++g) {
        HIP_TRY(hipSetDevice(lanes[g].dev));
        HIP_TRY(hipStreamWaitEvent(lanes[g].reduce, lanes[g].tracked[b], 0));
        bufs[(size_t)g] = lanes[g].tally[b];
        streams[(size_t)g] = (void*)(hipStream_t)lanes[g].reduce;
      }
      ABI_OK(mcgpu_rccl_reduce_u64(rccl, bufs.data(), plan.tally_words(), o, streams.data()));
      for (Lane& l : lanes) {
        HIP_TRY(hipSetDevice(l.dev));
        HIP_TRY(hipEventRecord(l.reduced[b], l.reduce));
        l.reduced_valid[b] = true;
      }
      HIP_TRY(hipSetDevice(lanes[o].dev));
      HIP_TRY(hipStreamWaitEvent(lanes[o].stream, lanes[o].reduced[b], 0));  // the owner's tracking stream goes on with the summed tally
      for (int g = 0; g < n; ++g)
        if (g != o) { void* unused = nullptr; ABI_OK(mcgpu_exchange_collect(lanes[g].x, j, lanes[g].stream, &unused)); }  // bookkeeping of the local ends
    }
    Lane& l = lanes[o];
    HIP_TRY(hipSetDevice(l.dev));
    hipStream_t const so = l.stream;
    void* tally = nullptr;
    ABI_OK(mcgpu_exchange_collect(l.x, j, so, &tally));  // exchange: the landed tallies of the other devices, added in one pass
    if (!tally) throw Error(-1, "!!ERROR!! mcgpu_run_scan: the owner of a projection got no tally");
    // the reference's ASCII file: its 63 MB of text are formatted on the device (ascii_device.hip) while the tally is there; the
    // writer thread downloads and writes them while the next projection is tracked
    if (opt->write_ascii) {
      if (out.ascii_on_host) HIP_TRY(hipMemcpyAsync(image_host[b], tally, plan.words * 8, hipMemcpyDeviceToHost, so));
      else ABI_OK(mcgpu_format_projection(l.ctx, tally, shape.total, j % out.n_ascii, so));
    }
    // planes_dev[b] was last downloaded two projections ago (by this device, if it owned that one)
    if (l.done_valid[b]) HIP_TRY(hipStreamWaitEvent(so, l.done[b], 0));
    ABI_OK(mcgpu_finalize_projection(l.ctx, tally, shape.total, plan.cx, l.planes_dev[b], 0, so));  // begin() zeroes the buffer for its next user
    if (plan.variance)
      ABI_OK(mcgpu_finalize_variance(l.ctx, tally, (unsigned long long*)tally + plan.words, shape.total, plan.cx, (float*)(void*)l.planes_dev[b] + 3 * plan.plane, 0, so));
    // the 9 MB of planes go to the host on a copy engine, beside the next tracking kernel (on the tracking stream the copy held
    // the next launch back by 0.17 ms per projection)
    HIP_TRY(hipEventRecord(l.finalized[b], so));
    HIP_TRY(hipStreamWaitEvent(l.copy, l.finalized[b], 0));
    HIP_TRY(hipMemcpyAsync(planes_host[b], l.planes_dev[b], plan.planes() * plan.plane * 4, hipMemcpyDeviceToHost, l.copy));
    HIP_TRY(hipEventRecord(l.done[b], l.copy));
    l.done_valid[b] = true;
  }

  void publish(int j) {  // kms[j] is final: the writer may take projection j
    const Lane& l = lanes[owner_of(j)];
    out.publish(j, {plan.first + plan.sim[j], plan.sim[j], l.dev, l.done[j & 1], static_cast<const float*>((void*)planes_host[j & 1]),
                    static_cast<const uint64_t*>((void*)image_host[j & 1]), l.ctx, (double)kms[j] * 1e-3});
  }

  void print_skipped(int from, int to) const {  // offsets [from, to) of the range
    for (int k = from; k < to && opt->progress && plan.phase == 0; ++k)
      if (plan.outside_roi(plan.first + k))
        printf("         << Skipping projection #%d of %d >> Angle %f degrees: outside angular region of interest.\n", plan.first + k + 1, (int)plan.nproj_all,
               (plan.angle0 + (plan.first + k) * plan.d_angle) * (180.0 / 3.14159265358979323846));
  }

  void run(mcgpu_scan_report* report) {
    connect();
    HIP_TRY(hipSetDevice(lanes[0].dev));
    unsigned long long H = opt->histories_per_projection ? opt->histories_per_projection : (unsigned long long)plan.hist_in;
    if (plan.by_time) H = budget_histories(plan, lanes[0].stream, n, false, opt->progress);  // calibrated on device 0
    shape = launch_shape(plan, H);
    choose_fast_preset(plan, shape.total, lanes[0].stream, opt->progress);
    for (int g = 0; g < n; ++g) { lanes[g].lo = shape.units * g / n; lanes[g].hi = shape.units * (g + 1) / n; }
    allocate();
    const int count = plan.count();
    kms.assign((size_t)count, 0.f);
    out.start(count, shape.total);

    // the pipeline of the file header: kernel i on every device, then the sum + finalize + download of the previous projection
    // on its owner (one device: of this projection), then the kernel time -- waiting for it also paces the host
    const bool single = n == 1;
    const double t0 = now_s();
    double kernel_s = 0.0, t_last_kernel = t0;
    int seed = (int)plan.seed, seed_ord = 0;  // seed_ord: simulated projections the seed has moved on past
    for (int i = 0; i < count; ++i) {
      const int p = plan.first + plan.sim[i];
      print_skipped(i ? plan.sim[i - 1] + 1 : 0, plan.sim[i]);
      if (plan.nproj_all != 1 && opt->progress) {
        printf("\n\n\n   << Simulating Projection %d of %d >>\n\n\n", p + 1, (int)plan.nproj_all);  // cbctmc/mc/simulation.py:200-219 parses this
        fflush(stdout);
      }
      if (plan.mode == MCGPU_MODE_COMPAT)  // the seed moves on per SIMULATED projection (MC-GPU_v1.3.cu:869)
        for (; seed_ord < plan.ord[i]; ++seed_ord) seed = mcgpu_advance_seed(1, shape.total, seed);
      track(i, seed);
      if (single) reduce_and_download(i);
      else if (i >= 1) { reduce_and_download(i - 1); publish(i - 1); }
      float ms = 0.f;  // the slowest device's launch
      for (const Lane& l : lanes) {
        float m = 0.f;
        ABI_OK(mcgpu_last_kernel_ms(l.ctx, &m));
        ms = m > ms ? m : ms;
      }
      kms[i] = ms;
      kernel_s += ms * 1e-3;
      t_last_kernel = now_s();
      if (single) publish(i);
    }
    print_skipped(count ? plan.sim[count - 1] + 1 : 0, plan.range);
    if (!single && count > 0) { reduce_and_download(count - 1); publish(count - 1); }
    out.join();
    float repl[3] = {0.f, 0.f, 0.f};
    if (stacks.open()) stacks.finish(plan, opt, repl);
    if (report) {
      report->projections = count;
      report->histories_per_projection = shape.total;
      report->seconds_total = now_s() - t0;
      report->seconds_kernels = kernel_s;
      report->seconds_after_last_kernel = now_s() - t_last_kernel;
      report->seconds_writer = out.busy_s;
      report->kernel_ms_min = count > 0 ? *std::min_element(kms.begin(), kms.end()) : 0.0;
      report->kernel_ms_max = count > 0 ? *std::max_element(kms.begin(), kms.end()) : 0.0;
      for (int k = 0; k < 3; ++k) report->zero_replacement[k] = repl[k];
    }
  }
};

int run_scan_sharing_histories(mcgpu_ctx* const* ctxs, int n_ctx, const mcgpu_scan_options* opt, mcgpu_scan_report* report, bool use_rccl = false) {
  ABI_BEGIN  // the code chooses the caller's next route: nothing is thrown past here (this also runs on threads of its own)
  HistoryScan(ctxs, n_ctx, opt, use_rccl).run(report);
  return 0;
  ABI_END
}

// Projection sharding (SURVEY.md 8e's fallback mode; the reference has no counterpart -- its ranks always share a projection,
// MC-GPU_v1.3.cu:913-1019): context g runs the single-device pipeline over the simulated projections number g, g + n, ... on a
// thread of its own, with all of their histories.  Nothing crosses between the devices: no exchange, no peer access, no
// collective.  The MetaImage stacks are shared and filled by slice index; ASCII files are per projection anyway.  Every output
// byte equals a one-device scan's (per-history streams / per-projection seeds do not depend on who simulates a projection).
int run_scan_sharing_projections(mcgpu_ctx* const* ctxs, int n_ctx, const mcgpu_scan_options* opt, mcgpu_scan_report* report) {
  ABI_BEGIN
    const ScanPlan plan = plan_scan(ctxs, n_ctx, opt);
    if (opt->projection_stride > 1) throw Error(-1, "!!ERROR!! mcgpu_run_scan_multi: MCGPU_SHARD_PROJECTIONS sets the projection stride itself");
    const int count = plan.count();
    // slice of every offset of the range: its ordinal among the simulated projections (the order a one-device scan appends in)
    std::vector<int> slice_of((size_t)plan.range, -1);
    for (int i = 0; i < count; ++i) slice_of[(size_t)plan.sim[i]] = i;
    OutputStacks stacks;
    if (opt->write_stacks && !opt->shared_stacks && count > 0) stacks.create(plan);
    std::vector<mcgpu_scan_options> o((size_t)n_ctx, *opt);
    // a time-limited run: ONE calibration, on device 0, for all the shards -- each device calibrating by itself would simulate
    // its own history count and the files would depend on who wrote them
    if (plan.by_time && count > 0) {
      const unsigned long long H = budget_histories(plan, nullptr, 1, true, opt->progress);  // a device simulates a projection alone
      for (auto& og : o) og.histories_per_projection = H;
    }
    std::vector<mcgpu_scan_report> r((size_t)n_ctx);
    std::vector<int> rcs((size_t)n_ctx, 0);
    std::vector<std::string> errs((size_t)n_ctx);
    std::vector<std::thread> th;
    const double t0 = now_s();
    for (int g = 0; g < n_ctx; ++g) {
      o[(size_t)g].shard = MCGPU_SHARD_HISTORIES;  // a single-context scan
      o[(size_t)g].projection_stride = n_ctx;
      o[(size_t)g].projection_phase = g;
      o[(size_t)g].air_stack = nullptr;  // normalisation runs once, below, over the finished stack
      if (stacks.open()) {
        o[(size_t)g].shared_stacks = stacks.stack;
        o[(size_t)g].slice_of_projection = slice_of.data();
      }
      th.emplace_back([&, g] {
        rcs[(size_t)g] = run_scan_sharing_histories(&ctxs[g], 1, &o[(size_t)g], &r[(size_t)g]);
        if (rcs[(size_t)g] != 0) errs[(size_t)g] = mcgpu_last_error();  // the last error is per thread
      });
    }
    for (auto& t : th) t.join();
    for (int g = 0; g < n_ctx; ++g)
      if (rcs[(size_t)g] != 0) throw Error(rcs[(size_t)g], errs[(size_t)g]);
    float repl[3] = {0.f, 0.f, 0.f};
    if (stacks.open()) stacks.finish(plan, opt, repl);
    if (report) {
      memset(report, 0, sizeof *report);
      report->histories_per_projection = r[0].histories_per_projection;
      report->seconds_total = now_s() - t0;
      report->kernel_ms_min = 1e30;
      for (int g = 0; g < n_ctx; ++g) {
        if (r[(size_t)g].projections > 0) {
          report->kernel_ms_min = std::min(report->kernel_ms_min, r[(size_t)g].kernel_ms_min);
          report->kernel_ms_max = std::max(report->kernel_ms_max, r[(size_t)g].kernel_ms_max);
        }
        report->projections += r[(size_t)g].projections;
        report->seconds_kernels = std::max(report->seconds_kernels, r[(size_t)g].seconds_kernels);  // the devices run side by side
        report->seconds_after_last_kernel = std::max(report->seconds_after_last_kernel, r[(size_t)g].seconds_after_last_kernel);
        report->seconds_writer += r[(size_t)g].seconds_writer;
      }
      if (report->projections == 0) report->kernel_ms_min = 0.0;
      for (int k = 0; k < 3; ++k) report->zero_replacement[k] = repl[k];
    }
    return 0;
  ABI_END
}

int refuse(const char* message) { return mcgpu::set_error(-1, message); }

}  // namespace

// Both entry points; `multi`: through mcgpu_run_scan_multi
static int run_scan_entry(mcgpu_ctx* const* ctxs, int n_ctx, const mcgpu_scan_options* caller_opt, mcgpu_scan_report* report, bool multi) {
  ABI_BEGIN
  if (!ctxs || n_ctx < 1 || !caller_opt || !ctxs[0]) return refuse("!!ERROR!! mcgpu_run_scan: null argument");
  mcgpu_scan_options local;
  mcgpu::read_options("mcgpu_run_scan", "mcgpu_scan_options", caller_opt, local);
  const mcgpu_scan_options* opt = &local;
  // the variance stacks: an output of the one-device scan's own stacks (4-D and multi-device variance are not built yet); an unknown
  // mode is still reported first, by plan_scan
  if (opt->write_variance && (opt->mode == MCGPU_MODE_FAST || opt->mode == MCGPU_MODE_COMPAT || opt->mode == MCGPU_MODE_FAST_F64)) {
    if (multi) return refuse("!!ERROR!! mcgpu_run_scan_multi: write_variance is an option of mcgpu_run_scan (one device)");
    if (!opt->write_stacks) return refuse("!!ERROR!! mcgpu_run_scan: write_variance needs write_stacks (the variance stacks are written beside the stacks)");
    if (opt->shared_stacks) return refuse("!!ERROR!! mcgpu_run_scan: write_variance cannot be combined with shared_stacks");
  }
  for (int g = 0; g < n_ctx; ++g)
    if (!ctxs[g]) return refuse("!!ERROR!! mcgpu_run_scan: null context");
  if (n_ctx > 1 && opt->shard == MCGPU_SHARD_PROJECTIONS) return run_scan_sharing_projections(ctxs, n_ctx, opt, report);
  // Routes of the per-projection tally sum between the devices (each is tried in its set-up phase, before anything is simulated or
  // written; every route gives the same output bytes):
  //   AUTO            the tally exchange (exchange.cpp: copy-engine pushes to the owner, one fused add); where the devices cannot reach
  //                   each other: projection sharding -- no traffic between the devices at all (SURVEY.md 8e's fallback mode)
  //   --reduce rccl   one ncclReduce per projection (reduce_rccl.cpp: north_star's collective, the reference's MPI_Reduce); where RCCL
  //                   cannot be set up: projection sharding
  // Round 6: AUTO no longer tries RCCL between the two.  The RCCL route has only ever run over a communicator of one
  // rank (no node); on a node without peer access it would stage 45 MB x (n - 1) per projection through host memory, where
  // projection sharding needs no traffic and writes the same bytes.  It is taken when asked for, and only then.
  const char* env_reduce = knob_str("MCGPU_REDUCE");
  // (asked for explicitly, the RCCL route also runs over ONE device -- a communicator of one rank: everything but the transport
  // between devices is then exercised on a one-GPU box, tests/test_gpu_dropin.py)
  const bool want_rccl = opt->reduce == MCGPU_REDUCE_RCCL || (opt->reduce == MCGPU_REDUCE_AUTO && env_reduce && !strcasecmp(env_reduce, "rccl"));
  auto say = [&](const char* what) {
    if (!opt->progress) return;
    // the reason, without the word the reference's log scanner takes for a failed run (cbctmc/mc/simulation.py:204)
    std::string why = mcgpu_last_error();
    for (size_t at = 0; at + 5 <= why.size(); ++at)
      if (strncasecmp(why.c_str() + at, "error", 5) == 0) why.replace(at, 5, "fault");
    for (size_t at; (at = why.find("!!")) != std::string::npos;) why.erase(at, 2);
    printf("       %s (%s)\n", what, why.c_str());
    fflush(stdout);
  };
  if (!want_rccl) {
    const int rc = run_scan_sharing_histories(ctxs, n_ctx, opt, report, false);
    if (rc != kExchangeUnavailable) return rc;
    // no peer access / no copy-engine path between these devices: the reference's split (histories of one projection on several
    // devices) needs a way to sum the tallies; whole projections per device need none and give the same files
    say("Tally exchange between the devices is not available: every device simulates whole projections instead (--reduce rccl asks for one RCCL reduction per projection)");
    return run_scan_sharing_projections(ctxs, n_ctx, opt, report);
  }
  const int rc = run_scan_sharing_histories(ctxs, n_ctx, opt, report, true);
  if (rc == 0 && opt->progress) { printf("       Detector tallies summed with one RCCL reduction (uint64, sum) per projection\n"); fflush(stdout); }
  if (rc != kRcclUnavailable) return rc;
  if (n_ctx == 1) {
    say("The RCCL reduction is not available: the device's own tally is the sum");
    return run_scan_sharing_histories(ctxs, n_ctx, opt, report, false);
  }
  say("The RCCL reduction that was asked for is not available: every device simulates whole projections instead");
  return run_scan_sharing_projections(ctxs, n_ctx, opt, report);
  ABI_END
}

extern "C" int mcgpu_run_scan_multi(mcgpu_ctx* const* ctxs, int n_ctx, const mcgpu_scan_options* options, mcgpu_scan_report* report) {
  return run_scan_entry(ctxs, n_ctx, options, report, true);
}

extern "C" int mcgpu_run_scan(mcgpu_ctx* ctx, const mcgpu_scan_options* opt, mcgpu_scan_report* report) {
  return run_scan_entry(&ctx, 1, opt, report, false);
}
