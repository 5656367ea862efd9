// field_inverse.hip -- the inverse of a displacement field by fixed-point iteration (row f22), and the residual that says how far two
// fields are from being each other's inverse.  It gives CorrespondenceModel.inverted / build_pair the opposite motion model without a
// second registration sweep (registration.hip, row f14).  What is pinned is the rule below, its float64 restatement
// (tests/field_inverse_ref.py) and these kernels held to that restatement.
//
// THE RULE.  u: float32 [3][n0][n1][n2] in voxels, component i along axis i, axis 2 the fastest in memory (the layout of mcgpu_register's
// result); v_0: the same shape, or none for zeros; iterations K >= 0; relaxation w, 0 < w <= 1 (rounded to float32).
// Result: v with u(x + v(x)) + v(x) ~ 0.  If moving(x + u(x)) ~ fixed(x), then fixed(y + v(y)) ~ moving(y).
//   Sampler.  S_i(v)(x) = u_i at c = x + v(x) (float32 sum): registration.hip's sampler (trilinear_sample.inc).  c is clamped to
//     [0, n_j - 1], base index floor(c), the upper tap's index clamped, fraction c - floor(c); blend a + (b - a) t along axis 2, then 1,
//     then 0, every operation rounded to float32.  The three components share indices and fractions.
//   Residual.  r_i(x) = v_i(x) + S_i(v)(x), float32.
//   Step.      v_i <- v_i - w r_i: a float32 product, then a float32 difference.  Jacobi: every tap reads the old v, the new one goes to
//     a second buffer.  No early stop: the result is a function of (u, v_0, K, w) alone, two calls give the same bytes.
//   Report.    residual_max = max |r_i(x)| over components and voxels; residual_rms = sqrt(sum double(r_i)^2 / (3 N)); both before the
//     first step and after the last one.  The sum is taken in double on a fixed grid by a fixed tree per block, and the blocks' partial
//     sums are added on the host in block order (as registration.hip's msd_kernel): no float atomics.
//   No operation is contracted (this file is built with -ffp-contract=off).
//   The iteration is v <- (1 - w) v - w u(x + v).  In one dimension it contracts where -1 < du/dx < (2 - w) / w: w = 1 needs slopes of u
//   below 1, w = 0.5 takes slopes up to 3.  A field that folds (du/dx <= -1, not invertible) leaves a residual that does not fall: the
//   caller reads residual_max_after.
//
// THE KERNELS.  "Row" is a run along axis 2.
//   invert_step    : one thread per voxel, lanes consecutive along a row: three coalesced reads of v, one set of indices and fractions
//                    for 3 x 8 taps of u (a gather: neighbouring lanes read neighbouring taps where v is smooth, and u is read through
//                    the caches), three coalesced writes.  24 B of v traffic per voxel and step, plus what of u misses the caches
//   field_residual : the same evaluation on the fixed reduce grid; stores r where asked; one double partial sum and one float partial
//                    maximum per block
// The residual is not fused into the step: it runs twice per call (before, after), a fused step would carry the reduction K times.  No
// A/B of a fusion has been run (profiles/field_inverse.md).
// Device memory: u and two v buffers, 9 N floats (mcgpu_field_residual: u, v and r where asked).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <utility>

#include "../../include/mcgpu_amd.h"
#include "hip_host.hpp"

namespace {

using mcgpu::blocks_of;
using mcgpu::refuse;

#include "fixed_sum.inc"

constexpr int kReduceBlocks = 256;    // the fixed grid of field_residual_kernel
constexpr int kIterationChunk = 128;  // steps between two waits of the host

#include "trilinear_sample.inc"

// r(x) = v(x) + u(x + v(x)) of voxel i = (i0, i1, i2); v(x) comes back too
__device__ __forceinline__ void residual_at(const float* __restrict__ u, const float* __restrict__ v, const Shape s, size_t i, int i0, int i1, int i2, float (&vx)[3],
                                            float (&r)[3]) {
  const size_t n = s.voxels();
  vx[0] = v[i];
  vx[1] = v[n + i];
  vx[2] = v[2 * n + i];
  int a0, b0, a1, b1, a2, b2;
  float t0, t1, t2;
  split((float)i0 + vx[0], s.n0, a0, b0, t0);
  split((float)i1 + vx[1], s.n1, a1, b1, t1);
  split((float)i2 + vx[2], s.n2, a2, b2, t2);
#pragma unroll
  for (int c = 0; c < 3; ++c) r[c] = vx[c] + blend8(u + (size_t)c * n, s, a0, b0, t0, a1, b1, t1, a2, b2, t2);
}

__global__ __launch_bounds__(256) void invert_step_kernel(const float* __restrict__ u, const float* __restrict__ v, float* __restrict__ v_out, const Shape s, float w) {
  int i0, i1, i2;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (!voxel_of(i, s, i0, i1, i2)) return;
  const size_t n = s.voxels();
  float vx[3], r[3];
  residual_at(u, v, s, i, i0, i1, i2, vx, r);
#pragma unroll
  for (int c = 0; c < 3; ++c) v_out[(size_t)c * n + i] = vx[c] - w * r[c];
}

// partial_sum[block] = sum of double(r_i)^2, partial_max[block] = max |r_i|; every thread takes the voxels block x 256 + thread + m x grid
// x 256 in rising m (components 0, 1, 2 of a voxel in that order), a block combines its 256 (sum, maximum) pairs by the fixed tree
// (fixed_sum.inc).  r is also stored where r_out is given
__global__ __launch_bounds__(256) void field_residual_kernel(const float* __restrict__ u, const float* __restrict__ v, const Shape s, float* __restrict__ r_out,
                                                             double* __restrict__ partial_sum, float* __restrict__ partial_max) {
  double sum = 0.0;
  float top = 0.f;
  const size_t n = s.voxels();
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    int i0, i1, i2;
    voxel_of(i, s, i0, i1, i2);
    float vx[3], r[3];
    residual_at(u, v, s, i, i0, i1, i2, vx, r);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (r_out) r_out[(size_t)c * n + i] = r[c];
      sum += (double)r[c] * (double)r[c];
      top = fmaxf(top, fabsf(r[c]));
    }
  }
  const SumMax total = block_tree(SumMax{sum, top});
  if (threadIdx.x == 0) {
    partial_sum[blockIdx.x] = total.sum;
    partial_max[blockIdx.x] = total.top;
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------------

mcgpu_invert_options checked_options(const char* fn, const mcgpu_invert_options* caller) {
  mcgpu_invert_options o;
  mcgpu::read_options(fn, "mcgpu_invert_options", caller, o);
  if (o.nx < 1 || o.ny < 1 || o.nz < 1) refuse(fn, "every axis needs at least one voxel (" + std::to_string(o.nx) + " x " + std::to_string(o.ny) + " x " + std::to_string(o.nz) + ")");
  if ((unsigned long long)o.nx * o.ny * o.nz >= (1ULL << 31)) refuse(fn, "the field has 2^31 voxels or more");
  if (o.iterations < 0) refuse(fn, "iterations " + std::to_string(o.iterations) + " is negative");
  if (!std::isfinite(o.relaxation) || !(o.relaxation > 0.0) || o.relaxation > 1.0) refuse(fn, "relaxation " + std::to_string(o.relaxation) + " is outside (0, 1]");
  if (o.device < 0) refuse(fn, "device " + std::to_string(o.device) + " is negative");
  return o;
}

// the partial sums and maxima of the reduce grid on the device, and their combination on the host
struct Reducer {
  double* d_sum = nullptr;
  float* d_max = nullptr;
  void alloc(mcgpu::CallDevice& dev) {
    d_sum = dev.alloc<double>(kReduceBlocks * sizeof(double));
    d_max = dev.alloc<float>(kReduceBlocks * sizeof(float));
  }
  // max |r| and sqrt(sum r^2 / (3 N)) of v against u; r goes to d_r where that is given
  void run(const float* u, const float* v, const Shape& s, float* d_r, double& residual_max, double& residual_rms) const {
    hipLaunchKernelGGL(field_residual_kernel, dim3(kReduceBlocks), dim3(256), 0, nullptr, u, v, s, d_r, d_sum, d_max);
    HIP_TRY(hipGetLastError());
    double sum;
    fold_blocks(d_sum, kReduceBlocks, 1, &sum);
    float maxima[kReduceBlocks];
    HIP_TRY(hipMemcpy(maxima, d_max, sizeof maxima, hipMemcpyDeviceToHost));
    float top = 0.f;
    for (int b = 0; b < kReduceBlocks; ++b) top = std::max(top, maxima[b]);
    residual_max = (double)top;
    residual_rms = std::sqrt(sum / (3.0 * (double)s.voxels()));
  }
};

}  // namespace

extern "C" int mcgpu_invert_field(const mcgpu_invert_options* caller_o, const float* field, float* inverse_out, mcgpu_invert_report* report) {
  static const char* const fn = "mcgpu_invert_field";
  ABI_BEGIN
  const mcgpu::Stopwatch call;
  const mcgpu_invert_options o = checked_options(fn, caller_o);
  mcgpu::check_report(fn, "report", "mcgpu_invert_report", report);
  if (!field || !inverse_out) refuse(fn, "null pointer: field and inverse_out are required");
  const Shape s{o.nx, o.ny, o.nz};
  const size_t n = s.voxels();
  const float w = (float)o.relaxation;
  mcgpu_invert_report rep;
  memset(&rep, 0, sizeof rep);
  rep.iterations = o.iterations;

  HIP_TRY(hipSetDevice(o.device));
  mcgpu::CallDevice dev;
  dev.events();
  const float* d_u;
  float *v, *v2;
  {
    const mcgpu::Stopwatch upload;
    d_u = dev.upload(field, 3 * n);
    if (o.initial) {
      v = dev.upload(o.initial, 3 * n);
    } else {
      v = dev.alloc_zeroed<float>(3 * n * 4);
    }
    rep.ms_upload += upload.ms();
  }
  v2 = dev.alloc<float>(3 * n * 4);
  Reducer reducer;
  reducer.alloc(dev);
  {
    mcgpu::Stage st(dev, rep.ms_reduce);
    reducer.run(d_u, v, s, nullptr, rep.residual_max_before, rep.residual_rms_before);
    st.done();
  }
  // the host waits once per kIterationChunk steps
  for (int first = 0; first < o.iterations; first += kIterationChunk) {
    const int count = std::min(kIterationChunk, o.iterations - first);
    mcgpu::Stage st(dev, rep.ms_step);
    for (int it = 0; it < count; ++it) {
      hipLaunchKernelGGL(invert_step_kernel, dim3(blocks_of(n)), dim3(256), 0, nullptr, d_u, v, v2, s, w);
      std::swap(v, v2);
    }
    st.done();
  }
  {
    mcgpu::Stage st(dev, rep.ms_reduce);
    reducer.run(d_u, v, s, nullptr, rep.residual_max_after, rep.residual_rms_after);
    st.done();
  }
  {
    const mcgpu::Stopwatch download;
    HIP_TRY(hipMemcpy(inverse_out, v, 3 * n * 4, hipMemcpyDeviceToHost));
    rep.ms_upload += download.ms();
  }
  rep.peak_device_bytes = (unsigned long long)dev.peak;
  rep.ms_total = call.ms();
  mcgpu::write_report(report, rep);
  return 0;
  ABI_END
}

extern "C" int mcgpu_field_residual(const mcgpu_invert_options* caller_o, const float* u, const float* v, float* residual_out, mcgpu_invert_report* report) {
  static const char* const fn = "mcgpu_field_residual";
  ABI_BEGIN
  const mcgpu::Stopwatch call;
  const mcgpu_invert_options o = checked_options(fn, caller_o);
  mcgpu::check_report(fn, "report", "mcgpu_invert_report", report);
  if (!u || !v) refuse(fn, "null pointer: u and v are required");
  const Shape s{o.nx, o.ny, o.nz};
  const size_t n = s.voxels();
  mcgpu_invert_report rep;
  memset(&rep, 0, sizeof rep);

  HIP_TRY(hipSetDevice(o.device));
  mcgpu::CallDevice dev;
  dev.events();
  const float *d_u, *d_v;
  {
    const mcgpu::Stopwatch upload;
    d_u = dev.upload(u, 3 * n);
    d_v = dev.upload(v, 3 * n);
    rep.ms_upload += upload.ms();
  }
  float* d_r = residual_out ? dev.alloc<float>(3 * n * 4) : nullptr;
  Reducer reducer;
  reducer.alloc(dev);
  {
    mcgpu::Stage st(dev, rep.ms_reduce);
    reducer.run(d_u, d_v, s, d_r, rep.residual_max_before, rep.residual_rms_before);
    st.done();
  }
  if (residual_out) {
    const mcgpu::Stopwatch download;
    HIP_TRY(hipMemcpy(residual_out, d_r, 3 * n * 4, hipMemcpyDeviceToHost));
    rep.ms_upload += download.ms();
  }
  rep.peak_device_bytes = (unsigned long long)dev.peak;
  rep.ms_total = call.ms();
  mcgpu::write_report(report, rep);
  return 0;
  ABI_END
}
