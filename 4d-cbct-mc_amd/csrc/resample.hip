// resample.hip -- a 3-D image to another voxel spacing, on the device (row f12): SimpleITK's Resample as the reference's
// resample_image_spacing calls it (cbctmc/utils.py:76-102), by the rule resample.hpp states.
//
// The rule is separable per axis, so the host evaluates it once per output index of every axis, in double (make_resample_plan: size,
// base / next tap, fraction, nearest index, inside flag; a few KB) and the kernels only gather and blend:
//   resample_nearest_kernel<T>   out = in[nearest0][nearest1][nearest2], or the default outside
//   resample_linear_kernel<T>    the eight taps blended in float64 in the rule's order (last axis, middle, first), cast by resample_cast
// T = uint8, int16, float32; output type = input type.  One thread takes a run of 8 consecutive outputs of one row of the fastest axis:
// the taps of a run lie in at most four input rows, read through the caches (an upsampled axis reads each element several times), and the
// run is stored as one 8-byte (uint8), one 16-byte (int16) or two 16-byte (float32) words where it is whole and aligned, element by
// element at ragged row ends and in rows that do not start on the vector's alignment.  Indexing is 32-bit: both volumes hold fewer than
// 2^31 voxels (checked by make_resample_plan before any device call).  No LDS.  Measured (profiles/resample_ab.md): 0.3 - 0.5 TB/s on a
// 512 x 512 x 160 CT, bound by the loads per output (plan entries and scalar taps) and not by the bytes; 3 ms for a CT and eight
// segmentations, 2 % of the call that installs them.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "engine_internal.hpp"
#include "resample.hpp"

namespace mcgpu {
namespace {

constexpr int kRun = 8;  // outputs per thread, along the fastest axis

template <typename T>
__device__ __forceinline__ void store_run(T* __restrict__ out, const T (&r)[kRun], int count) {
  constexpr int kBytes = kRun * (int)sizeof(T), kVec = kBytes < 16 ? kBytes : 16;
  if (count == kRun && (reinterpret_cast<uintptr_t>(out) & (uintptr_t)(kVec - 1)) == 0) {
    if constexpr (kBytes == 8) {
      uint2 w;
      __builtin_memcpy(&w, r, 8);
      *reinterpret_cast<uint2*>(out) = w;
    } else {
      uint4 w[kBytes / 16];
      __builtin_memcpy(w, r, kBytes);
#pragma unroll
      for (int q = 0; q < kBytes / 16; ++q) reinterpret_cast<uint4*>(out)[q] = w[q];
    }
  } else {
#pragma unroll
    for (int k = 0; k < kRun; ++k)
      if (k < count) out[k] = r[k];
  }
}

struct RunPosition {
  unsigned int row;  // i0 * n_out[1] + i1
  int e0, e1, i2, count;
  bool valid, row_inside;
};

__device__ __forceinline__ RunPosition run_position(const ResampleArgs& a, unsigned int runs_per_row, unsigned int n_runs) {
  RunPosition p{};
  const unsigned int t = blockIdx.x * 256u + threadIdx.x;
  p.valid = t < n_runs;
  if (!p.valid) return p;
  p.row = t / runs_per_row;
  p.i2 = (int)(t - p.row * runs_per_row) * kRun;
  const unsigned int i0 = p.row / (unsigned int)a.n_out[1];
  p.e0 = a.off[0] + (int)i0;
  p.e1 = a.off[1] + (int)(p.row - i0 * (unsigned int)a.n_out[1]);
  p.count = min(kRun, a.n_out[2] - p.i2);
  p.row_inside = a.inside[p.e0] != 0 && a.inside[p.e1] != 0;
  return p;
}

// plan entry of output k of the run; the outputs past a ragged row end read the row's last entry and are not stored
__device__ __forceinline__ int run_entry(const ResampleArgs& a, const RunPosition& p, int k) { return a.off[2] + min(p.i2 + k, a.n_out[2] - 1); }

__device__ __forceinline__ double lerp(double a, double b, double d) { return a + (b - a) * d; }

template <typename T>
__global__ __launch_bounds__(256) void resample_nearest_kernel(ResampleArgs a, const T* __restrict__ in, T* __restrict__ out, T default_value,
                                                               unsigned int runs_per_row, unsigned int n_runs) {
  const RunPosition p = run_position(a, runs_per_row, n_runs);
  if (!p.valid) return;
  T r[kRun];
  const T* __restrict__ src = in + ((unsigned int)a.nearest[p.e0] * (unsigned int)a.n_in[1] + (unsigned int)a.nearest[p.e1]) * (unsigned int)a.n_in[2];
#pragma unroll
  for (int k = 0; k < kRun; ++k) {
    const int e2 = run_entry(a, p, k);
    r[k] = p.row_inside && a.inside[e2] ? src[a.nearest[e2]] : default_value;
  }
  store_run(out + (p.row * (unsigned int)a.n_out[2] + (unsigned int)p.i2), r, p.count);
}

template <typename T>
__global__ __launch_bounds__(256) void resample_linear_kernel(ResampleArgs a, const T* __restrict__ in, T* __restrict__ out, T default_value,
                                                              unsigned int runs_per_row, unsigned int n_runs) {
  const RunPosition p = run_position(a, runs_per_row, n_runs);
  if (!p.valid) return;
  T r[kRun];
  const unsigned int n1 = (unsigned int)a.n_in[1], n2 = (unsigned int)a.n_in[2];
  const unsigned int b0 = (unsigned int)a.base[p.e0], t0 = (unsigned int)a.next[p.e0], b1 = (unsigned int)a.base[p.e1], t1 = (unsigned int)a.next[p.e1];
  const T* __restrict__ r00 = in + (b0 * n1 + b1) * n2;  // the four input rows of the run: [axis 0 tap][axis 1 tap]
  const T* __restrict__ r01 = in + (b0 * n1 + t1) * n2;
  const T* __restrict__ r10 = in + (t0 * n1 + b1) * n2;
  const T* __restrict__ r11 = in + (t0 * n1 + t1) * n2;
  const double d0 = a.frac[p.e0], d1 = a.frac[p.e1];
#pragma unroll
  for (int k = 0; k < kRun; ++k) {
    const int e2 = run_entry(a, p, k);
    const int b2 = a.base[e2], t2 = a.next[e2];
    const double d2 = a.frac[e2];
    const double x00 = lerp((double)r00[b2], (double)r00[t2], d2), x01 = lerp((double)r01[b2], (double)r01[t2], d2);
    const double x10 = lerp((double)r10[b2], (double)r10[t2], d2), x11 = lerp((double)r11[b2], (double)r11[t2], d2);
    const double v = lerp(lerp(x00, x01, d1), lerp(x10, x11, d1), d0);
    r[k] = p.row_inside && a.inside[e2] ? resample_cast<T>(v) : default_value;
  }
  store_run(out + (p.row * (unsigned int)a.n_out[2] + (unsigned int)p.i2), r, p.count);
}

template <typename T>
hipError_t launch_typed(const ResampleArgs& a, int interpolator, double default_value, const void* in, void* out, hipStream_t stream) {
  const unsigned int runs_per_row = ((unsigned int)a.n_out[2] + kRun - 1) / kRun;
  const unsigned long long n_runs = (unsigned long long)a.n_out[0] * a.n_out[1] * runs_per_row;
  if (n_runs >= (1ULL << 31)) return hipErrorInvalidValue;
  const dim3 grid((unsigned int)((n_runs + 255) / 256)), block(256);
  const T dflt = resample_cast<T>(default_value);
  if (interpolator == kResampleNearest)
    hipLaunchKernelGGL(resample_nearest_kernel<T>, grid, block, 0, stream, a, (const T*)in, (T*)out, dflt, runs_per_row, (unsigned int)n_runs);
  else
    hipLaunchKernelGGL(resample_linear_kernel<T>, grid, block, 0, stream, a, (const T*)in, (T*)out, dflt, runs_per_row, (unsigned int)n_runs);
  return hipGetLastError();
}

// the options as this library knows them, refused unless they name an element type and an interpolator
mcgpu_resample_options checked_options(const char* fn, const mcgpu_resample_options* caller) {
  mcgpu_resample_options o;
  read_options(fn, "mcgpu_resample_options", caller, o);
  const std::string pre = std::string("!!ERROR!! ") + fn + ": ";
  require(o.dtype == MCGPU_IMAGE_INT16 || o.dtype == MCGPU_IMAGE_FLOAT32 || o.dtype == MCGPU_IMAGE_UINT8, -1,
          (pre + "dtype is MCGPU_IMAGE_UINT8, MCGPU_IMAGE_INT16 or MCGPU_IMAGE_FLOAT32").c_str());
  require(o.interpolator == kResampleNearest || o.interpolator == kResampleLinear, -1, (pre + "interpolator is 0 (nearest) or 1 (linear)").c_str());
  return o;
}

}  // namespace

ResamplePlan make_resample_plan(const char* who, const int n_in[3], const double spacing_in[3], const double spacing_out[3]) {
  const std::string pre = std::string("!!ERROR!! ") + who + ": ";
  ResamplePlan p;
  for (int k = 0; k < 3; ++k) {
    require(n_in[k] > 0, -1, (pre + "every axis needs at least one voxel").c_str());
    require(std::isfinite(spacing_in[k]) && spacing_in[k] > 0.0 && std::isfinite(spacing_out[k]) && spacing_out[k] > 0.0, -1,
            (pre + "spacings are finite and positive").c_str());
    const double m = std::nearbyint(n_in[k] * (spacing_in[k] / spacing_out[k]));
    require(m >= 1.0, -1, (pre + "an axis of the resampled volume rounds to 0 voxels").c_str());
    require(m <= 2147483647.0, -2, "!!ERROR!! voxel grid too large for the 32-bit voxel index of the kernel");
    p.n_in[k] = n_in[k];
    p.n_out[k] = (int)m;
  }
  for (const int* n : {p.n_in, p.n_out})
    require((unsigned long long)n[0] * n[1] < (1ULL << 31) && (unsigned long long)n[0] * n[1] * n[2] < (1ULL << 31), -2,
            "!!ERROR!! voxel grid too large for the 32-bit voxel index of the kernel");
  int total = 0;
  for (int k = 0; k < 3; ++k) { p.off[k] = total; total += p.n_out[k]; }
  p.base.resize(total); p.next.resize(total); p.nearest.resize(total); p.frac.resize(total); p.inside.resize(total);
  for (int k = 0; k < 3; ++k) {
    const int N = p.n_in[k];
    const double os = spacing_in[k], ns = spacing_out[k], last = (double)(N - 1);
    for (int i = 0; i < p.n_out[k]; ++i) {
      const double c = ((double)i * ns) / os;
      const double b = std::min(std::max(std::floor(c), 0.0), last);
      const int e = p.off[k] + i;
      p.inside[e] = (c >= -0.5 && c < (double)N - 0.5) ? 1 : 0;
      p.base[e] = (int)b;
      p.next[e] = std::min((int)b + 1, N - 1);
      p.frac[e] = std::max(c - b, 0.0);
      p.nearest[e] = (int)std::min(std::max(std::floor(c + 0.5), 0.0), last);
    }
  }
  return p;
}

ResampleArgs upload_resample_plan(CallDevice& dev, const ResamplePlan& plan) {
  ResampleArgs a;
  for (int k = 0; k < 3; ++k) { a.n_in[k] = plan.n_in[k]; a.n_out[k] = plan.n_out[k]; a.off[k] = plan.off[k]; }
  a.base = dev.upload(plan.base);
  a.next = dev.upload(plan.next);
  a.nearest = dev.upload(plan.nearest);
  a.frac = dev.upload(plan.frac);
  a.inside = dev.upload(plan.inside);
  return a;
}

hipError_t launch_resample(const ResampleArgs& a, int dtype, int interpolator, double default_value, const void* in, void* out, hipStream_t stream) {
  if (interpolator != kResampleNearest && interpolator != kResampleLinear) return hipErrorInvalidValue;
  if (dtype == MCGPU_IMAGE_UINT8) return launch_typed<unsigned char>(a, interpolator, default_value, in, out, stream);
  if (dtype == MCGPU_IMAGE_INT16) return launch_typed<short>(a, interpolator, default_value, in, out, stream);
  if (dtype == MCGPU_IMAGE_FLOAT32) return launch_typed<float>(a, interpolator, default_value, in, out, stream);
  return hipErrorInvalidValue;
}

}  // namespace mcgpu

using namespace mcgpu;

extern "C" {

int mcgpu_resample_plan(const mcgpu_resample_options* options, int n_out[3], int* base, int* next, double* frac, int* nearest, unsigned char* inside) {
  ABI_BEGIN
  require(options && n_out, -1, "!!ERROR!! mcgpu_resample_plan: null argument");
  const mcgpu_resample_options o = checked_options("mcgpu_resample_plan", options);
  const ResamplePlan p = make_resample_plan("mcgpu_resample_plan", o.n_in, o.spacing_in, o.spacing_out);
  for (int k = 0; k < 3; ++k) n_out[k] = p.n_out[k];
  if (base) memcpy(base, p.base.data(), p.base.size() * sizeof(int));
  if (next) memcpy(next, p.next.data(), p.next.size() * sizeof(int));
  if (frac) memcpy(frac, p.frac.data(), p.frac.size() * sizeof(double));
  if (nearest) memcpy(nearest, p.nearest.data(), p.nearest.size() * sizeof(int));
  if (inside) memcpy(inside, p.inside.data(), p.inside.size());
  return 0;
  ABI_END
}

int mcgpu_resample_volume(mcgpu_ctx* ctx, const mcgpu_resample_options* options, const void* in, void* out, mcgpu_resample_report* report) {
  ABI_BEGIN
  require(ctx && ctx->has_device && options && in && out, -1, "!!ERROR!! mcgpu_resample_volume: bad argument (the context needs a device)");
  check_report("mcgpu_resample_volume", "report", "mcgpu_resample_report", report);
  const mcgpu_resample_options o = checked_options("mcgpu_resample_volume", options);
  const ResamplePlan plan = make_resample_plan("mcgpu_resample_volume", o.n_in, o.spacing_in, o.spacing_out);
  const size_t size = resample_element_size(o.dtype), bytes_in = plan.voxels_in() * size, bytes_out = plan.voxels_out() * size;
  HIP_TRY(hipSetDevice(ctx->dev.device_id));
  CallDevice dev;
  dev.events();
  mcgpu_resample_report rep;
  memset(&rep, 0, sizeof rep);
  rep.kernel_bytes = bytes_in + bytes_out;
  const Stopwatch upload;
  const ResampleArgs args = upload_resample_plan(dev, plan);
  const unsigned char* d_in = dev.upload((const unsigned char*)in, bytes_in);
  unsigned char* d_out = dev.alloc<unsigned char>(bytes_out);
  rep.ms_upload = upload.ms();
  {
    Stage stage(dev, rep.ms_kernel);
    HIP_TRY(launch_resample(args, o.dtype, o.interpolator, o.default_value, d_in, d_out, nullptr));
    stage.done();
  }
  const Stopwatch download;
  HIP_TRY(hipMemcpy(out, d_out, bytes_out, hipMemcpyDeviceToHost));
  rep.ms_download = download.ms();
  write_report(report, rep);
  return 0;
  ABI_END
}

}  // extern "C"
