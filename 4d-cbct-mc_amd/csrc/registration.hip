// registration.hip -- demons registration of two volumes (row f14): what the reference's CorrespondenceModel.build_default obtains from
// vroc's variational registration (cbctmc/registration/correspondence.py:315-345; vroc is a third-party dependency that is not vendored
// in the reference tree, so parity with it is unpinned).  What is pinned is the rule below, its float64 restatement
// (tests/registration_ref.py) and these kernels held to that restatement.
//
// THE RULE.  fixed, moving: float32 [n0][n1][n2] (array axes x, y, z of an MCGeometry; z is the fastest in memory); fixed_mask: uint8 of
// that shape or none; iterations, tau, sigma = (s0, s1, s2) in voxels, n_levels.  Result: u [3][n0][n1][n2] in voxels on the fixed grid,
// component i along axis i, with moving(x + u(x)) ~ fixed(x).
//   Levels l = n_levels - 1 .. 0, level shape s_i = ceil(n_i / 2^l).  Level 0 takes the images and the mask as they are.  On the others an
//   image is resized trilinearly at the positions p_i = linspace(0, n_i - 1, s_i) (float64: k (n_i - 1) / (s_i - 1), the last one n_i - 1, 0
//   where s_i = 1), base index floor(p), fraction p - floor(p) rounded to float32, the upper tap's index clamped to n_i - 1; the mask is
//   resized by nearest neighbour, index floor(p + 0.5) clamped.  The field is 0 on the coarsest level and is carried to the next one by the
//   same trilinear resize per component, component i then multiplied by float32((s_new_i - 1) / (s_old_i - 1)), or 1 where s_old_i = 1.
//   Trilinear blend, everywhere: a + (b - a) t along axis 2, then axis 1, then axis 0, every operation rounded to float32.
//   One iteration on a level:
//     1. w = moving at c = x + u (float32 sum), c clamped to [0, s_i - 1], base floor(c), fraction c - floor(c), upper tap clamped
//     2. d = w - fixed
//     3. g_i = 0.5 (fixed[x + e_i] - fixed[x - e_i]), indices clamped;  den = ((g_0^2 + g_1^2) + g_2^2) + d^2
//     4. v_i = (-d g_i) / den where den > 1e-9, else 0; 0 where the mask is 0 (IEEE division)
//     5. u_i += tau v_i
//     6. every component of u is smoothed by a Gaussian along axis 0, then 1, then 2: radius r_i = int(4 s_i + 0.5), weights
//        exp(-k^2 / (2 s_i^2)) divided by their sum (float64, summed from k = -r upwards) and rounded to float32, index clamp at the border,
//        out = sum over k = -r .. r, in that order and starting from 0, of weight_k in[x + k e_i], float32 products and sums.  s_i = 0 skips
//        the pass.
//   No early stop.  No operation is contracted (this file is built with -ffp-contract=off), so the smoothing is the restatement's float32
//   run bit for bit and the rest differs from it only where the restatement's float32 run itself rounds differently (fractions).
//   Per level, the report holds the mean over the voxels of double(float32 d)^2 before the first and after the last iteration.
//
// THE KERNELS.  The fastest axis in memory is axis 2; "row" below is a run along it.
//   resize_linear / resize_nearest : one thread per output voxel; the per-axis tables (base, fraction, nearest) come from the host.
//                                    resample.hip's sampler is not reused: its plan derives the output size from two spacings
//                                    (nearbyint(n si / so)) and blends in float64, neither of which is this rule
//   force_step  : one thread per voxel along the rows: three coalesced field reads, eight taps of moving, seven of fixed, the mask byte;
//                 writes the updated field to a second buffer; g is recomputed, never stored.  28 B of HBM traffic per voxel + the mask
//   smooth_row<R> : axis 2.  A wave takes kRowTile = 64 outputs of a row; the segment and its halo (clamped indices) go through LDS
//   smooth_line<R> : axes 0 and 1.  The volume is [outer][n_axis][inner]; a thread owns one (outer, inner) position (consecutive lanes,
//                 consecutive addresses) and kSegment outputs along the axis, and slides along it with the 2 R + 1 window in registers: one new load
//                 per output.  Every tap clamps, so an axis shorter than the radius is handled by the same code
//   msd         : a fixed grid, a fixed tree per block, double; the blocks' partial sums are added on the host in block order (as
//                 wpc_fit.hip reduces its normal equations): no float atomics
// 24 B per voxel and pass, 100 B per voxel and iteration: 2.16 ms an iteration at 500 x 500 x 300 (force 0.55, passes 0.37, 0.40, 0.80).
// No pass is fused with another or with the force step: no A/B of a fusion has been run (profiles/registration_ab.md).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/mcgpu_amd.h"
#include "hip_host.hpp"

namespace {

using mcgpu::blocks_of;
using mcgpu::refuse;

#include "fixed_sum.inc"

constexpr int kMaxRadius = 16;
constexpr int kRowTile = 64, kRowsPerBlock = 4, kRowGroups = 4;  // smooth_row: 256 threads, a wave per row, 16 rows per block
constexpr int kSegment = 32;                      // smooth_line: outputs per thread along the axis
constexpr int kReduceBlocks = 256;                // the fixed grid of msd_kernel
constexpr int kIterationChunk = 128;              // iterations between two waits of the host

#include "trilinear_sample.inc"  // Shape, lerp, split, blend8, sample, voxel_of: shared with field_inverse.hip

// moving at x + u
__device__ __forceinline__ float warped(const float* __restrict__ moving, const float* __restrict__ u, const Shape s, size_t i, int i0, int i1, int i2) {
  const size_t n = s.voxels();
  return sample(moving, s, (float)i0 + u[i], (float)i1 + u[n + i], (float)i2 + u[2 * n + i]);
}

// the per-axis tables of a resize, axis k at off[k] .. off[k] + out.n_k
struct ResizeTables {
  const int* base;
  const float* frac;
  const int* nearest;
  int off[3];
};

__global__ __launch_bounds__(256) void resize_linear_kernel(const float* __restrict__ in, float* __restrict__ out, const Shape si, const Shape so, const ResizeTables T,
                                                            float scale) {
  int i0, i1, i2;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (!voxel_of(i, so, i0, i1, i2)) return;
  const int e0 = T.off[0] + i0, e1 = T.off[1] + i1, e2 = T.off[2] + i2;
  const int a0 = T.base[e0], a1 = T.base[e1], a2 = T.base[e2];
  out[i] = blend8(in, si, a0, min(a0 + 1, si.n0 - 1), T.frac[e0], a1, min(a1 + 1, si.n1 - 1), T.frac[e1], a2, min(a2 + 1, si.n2 - 1), T.frac[e2]) * scale;
}

__global__ __launch_bounds__(256) void resize_nearest_kernel(const unsigned char* __restrict__ in, unsigned char* __restrict__ out, const Shape si, const Shape so,
                                                             const ResizeTables T) {
  int i0, i1, i2;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (!voxel_of(i, so, i0, i1, i2)) return;
  out[i] = in[((size_t)T.nearest[T.off[0] + i0] * si.n1 + T.nearest[T.off[1] + i1]) * si.n2 + T.nearest[T.off[2] + i2]];
}

__global__ __launch_bounds__(256) void warp_linear_kernel(const float* __restrict__ moving, const float* __restrict__ u, float* __restrict__ out, const Shape s) {
  int i0, i1, i2;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (!voxel_of(i, s, i0, i1, i2)) return;
  out[i] = warped(moving, u, s, i, i0, i1, i2);
}

// steps 1 to 5
__global__ __launch_bounds__(256) void force_step_kernel(const float* __restrict__ fixed, const float* __restrict__ moving, const unsigned char* __restrict__ mask,
                                                         const float* __restrict__ u, float* __restrict__ u_out, const Shape s, float tau) {
  int i0, i1, i2;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (!voxel_of(i, s, i0, i1, i2)) return;
  const size_t n = s.voxels(), plane = (size_t)s.n1 * s.n2;
  const float u0 = u[i], u1 = u[n + i], u2 = u[2 * n + i];
  const float d = sample(moving, s, (float)i0 + u0, (float)i1 + u1, (float)i2 + u2) - fixed[i];
  const float* __restrict__ row = fixed + i - i2;
  const float g0 = 0.5f * (fixed[i + (i0 + 1 < s.n0 ? plane : 0)] - fixed[i - (i0 > 0 ? plane : 0)]);
  const float g1 = 0.5f * (fixed[i + (i1 + 1 < s.n1 ? (size_t)s.n2 : 0)] - fixed[i - (i1 > 0 ? (size_t)s.n2 : 0)]);
  const float g2 = 0.5f * (row[min(i2 + 1, s.n2 - 1)] - row[max(i2 - 1, 0)]);
  const float den = ((g0 * g0 + g1 * g1) + g2 * g2) + d * d;
  float v0 = 0.f, v1 = 0.f, v2 = 0.f;
  if (den > 1e-9f && (!mask || mask[i])) {
    v0 = (-d * g0) / den;
    v1 = (-d * g1) / den;
    v2 = (-d * g2) / den;
  }
  u_out[i] = u0 + tau * v0;
  u_out[n + i] = u1 + tau * v1;
  u_out[2 * n + i] = u2 + tau * v2;
}

// axis 2 of [rows][n2]: out[row][j] = sum_k w[k + R] in[row][clamp(j + k)].  blockIdx.y: the tile of the row; a block takes kRowGroups
// times kRowsPerBlock consecutive rows of blockIdx.x, one wave per row and turn: the 64 outputs of a wave and their halo go through its own
// LDS row.  The radius is a template argument as in smooth_line_kernel: the weights sit in scalar registers and the sum is unrolled.
// Measured at 500 x 500 x 300, sigma 1.25 (profiles/registration_ab.md): 0.80 ms a pass against 1.02 ms for blocks of 128 x 2 rows; the
// same pass with the radius as a run-time loop bound, every tap waiting for its weight's load, was slower again
template <int R>
__global__ __launch_bounds__(kRowTile* kRowsPerBlock) void smooth_row_kernel(const float* __restrict__ in, float* __restrict__ out, const float* __restrict__ w, size_t rows,
                                                                            int n2) {
  __shared__ float lds[kRowsPerBlock][kRowTile + 2 * R + 1];
  const int t = threadIdx.x, ry = threadIdx.y;
  const int j0 = blockIdx.y * kRowTile;
  float wk[2 * R + 1];
#pragma unroll
  for (int k = 0; k <= 2 * R; ++k) wk[k] = w[k];
  for (int g = 0; g < kRowGroups; ++g) {
    const size_t row = ((size_t)blockIdx.x * kRowGroups + g) * kRowsPerBlock + ry;  // uniform over each wave
    if (row < rows) {
      const float* __restrict__ src = in + row * n2;
      lds[ry][t] = src[min(max(j0 - R + t, 0), n2 - 1)];
      if (t < 2 * R) lds[ry][kRowTile + t] = src[min(max(j0 - R + kRowTile + t, 0), n2 - 1)];
    }
    __syncthreads();
    if (row < rows && j0 + t < n2) {
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k <= 2 * R; ++k) acc = acc + wk[k] * lds[ry][t + k];
      out[row * n2 + j0 + t] = acc;
    }
    __syncthreads();
  }
}

// an axis of [outer][n_axis][inner]: blockIdx.x x 256 + thread = outer x inner + inner position (a short `inner`, as the rows of the
// axis 1 pass are, still fills the waves), blockIdx.y = segment of the axis
template <int R>
__global__ __launch_bounds__(256) void smooth_line_kernel(const float* __restrict__ in, float* __restrict__ out, const float* __restrict__ w, int n_axis, size_t inner,
                                                          size_t lines) {
  const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= lines) return;
  const size_t o = id / inner, j = id - o * inner;
  const size_t base = o * n_axis * inner + j;
  const float* __restrict__ src = in + base;
  float* __restrict__ dst = out + base;
  const int a0 = blockIdx.y * kSegment, a1 = min(a0 + kSegment, n_axis), last = n_axis - 1;
  float wk[2 * R + 1], win[2 * R + 1];
#pragma unroll
  for (int k = 0; k <= 2 * R; ++k) {
    wk[k] = w[k];
    win[k] = src[(size_t)min(max(a0 - R + k, 0), last) * inner];
  }
  for (int a = a0; a < a1; ++a) {
    const float next = src[(size_t)min(a + 1 + R, last) * inner];  // the tap that enters the window for a + 1
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k <= 2 * R; ++k) acc = acc + wk[k] * win[k];
    dst[(size_t)a * inner] = acc;
#pragma unroll
    for (int k = 0; k < 2 * R; ++k) win[k] = win[k + 1];
    win[2 * R] = next;
  }
}

// partial[block] = sum of double(d)^2, d = float32(moving(x + u) - fixed); every thread takes the voxels block x 256 + thread + m x grid x 256
// in rising m, a block adds its 256 sums by the fixed tree (fixed_sum.inc).  d is also stored where diff is given
__global__ __launch_bounds__(256) void msd_kernel(const float* __restrict__ fixed, const float* __restrict__ moving, const float* __restrict__ u, const Shape s,
                                                  float* __restrict__ diff, double* __restrict__ partial) {
  double sum = 0.0;
  const size_t n = s.voxels();
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    int i0, i1, i2;
    voxel_of(i, s, i0, i1, i2);
    const float d = warped(moving, u, s, i, i0, i1, i2) - fixed[i];
    if (diff) diff[i] = d;
    sum += (double)d * (double)d;
  }
  const double total = block_tree(sum);
  if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

// ---- host -------------------------------------------------------------------------------------------------------------------

Shape level_shape(const Shape& s, int level) {
  auto up = [level](int n) { return (int)(((long long)n + (1LL << level) - 1) >> level); };
  return {up(s.n0), up(s.n1), up(s.n2)};
}

int radius_of(double sigma) { return (int)(4.0 * sigma + 0.5); }

// the rule's float32 weights of one axis
std::vector<float> gaussian_weights(double sigma) {
  const int r = radius_of(sigma);
  std::vector<double> e(2 * r + 1);
  double sum = 0.0;
  for (int k = -r; k <= r; ++k) {
    e[k + r] = std::exp(-(double)(k * k) / (2.0 * sigma * sigma));
    sum += e[k + r];
  }
  std::vector<float> w(2 * r + 1);
  for (int k = 0; k <= 2 * r; ++k) w[k] = (float)(e[k] / sum);
  return w;
}

// the tables of a resize from `in` to `out` on the device
ResizeTables upload_tables(mcgpu::CallDevice& dev, const Shape& in, const Shape& out) {
  const int n_in[3] = {in.n0, in.n1, in.n2}, n_out[3] = {out.n0, out.n1, out.n2};
  std::vector<int> base, nearest;
  std::vector<float> frac;
  ResizeTables T{};
  for (int k = 0; k < 3; ++k) {
    T.off[k] = (int)base.size();
    const int n = n_in[k], s = n_out[k];
    const double step = s > 1 ? (double)(n - 1) / (double)(s - 1) : 0.0;
    for (int i = 0; i < s; ++i) {
      const double p = s == 1 ? 0.0 : (i == s - 1 ? (double)(n - 1) : (double)i * step);
      const double b = std::min(std::floor(p), (double)(n - 1));
      base.push_back((int)b);
      frac.push_back((float)(p - b));
      nearest.push_back((int)std::min(std::floor(p + 0.5), (double)(n - 1)));
    }
  }
  T.base = dev.upload(base);
  T.frac = dev.upload(frac);
  T.nearest = dev.upload(nearest);
  return T;
}
void release_tables(mcgpu::CallDevice& dev, const ResizeTables& T) {
  dev.release((void*)T.base);
  dev.release((void*)T.frac);
  dev.release((void*)T.nearest);
}

template <int R>
void launch_line(dim3 grid, const float* in, float* out, const float* w, int n_axis, size_t inner, size_t lines) {
  hipLaunchKernelGGL(smooth_line_kernel<R>, grid, dim3(256), 0, nullptr, in, out, w, n_axis, inner, lines);
}
template <int R>
void launch_row(dim3 grid, const float* in, float* out, const float* w, size_t rows, int n2) {
  hipLaunchKernelGGL(smooth_row_kernel<R>, grid, dim3(kRowTile, kRowsPerBlock), 0, nullptr, in, out, w, rows, n2);
}
// the launches that depend on the compile-time radius
#define FOR_RADIUS(r, call, args)                                                                                                    \
  switch (r) {                                                                                                                       \
    case 0: call<0> args; break;   case 1: call<1> args; break;   case 2: call<2> args; break;   case 3: call<3> args; break;        \
    case 4: call<4> args; break;   case 5: call<5> args; break;   case 6: call<6> args; break;   case 7: call<7> args; break;        \
    case 8: call<8> args; break;   case 9: call<9> args; break;   case 10: call<10> args; break; case 11: call<11> args; break;      \
    case 12: call<12> args; break; case 13: call<13> args; break; case 14: call<14> args; break; case 15: call<15> args; break;      \
    case 16: call<16> args; break;                                                                                                   \
    default: refuse(fn, "no smoothing kernel for radius " + std::to_string(r));                                                      \
  }

// the Gaussian of the three components of a field, axis by axis; device weights, radii and which axes run
struct Smoother {
  const float* w[3] = {nullptr, nullptr, nullptr};
  int r[3] = {0, 0, 0};
  bool on[3] = {false, false, false};
  void upload(mcgpu::CallDevice& dev, const double sigma[3]) {
    for (int k = 0; k < 3; ++k) {
      on[k] = sigma[k] > 0.0;
      if (!on[k]) continue;
      r[k] = radius_of(sigma[k]);
      w[k] = dev.upload(gaussian_weights(sigma[k]));
    }
  }
  // one axis of [outer][n_axis][inner] by the sliding window
  void line(const char* fn, int k, const float* in, float* out, size_t outer, int n_axis, size_t inner) const {
    const dim3 grid(blocks_of(outer * inner), (unsigned int)((n_axis + kSegment - 1) / kSegment));
    if (grid.y > 65535u) refuse(fn, "an axis is too long for the smoothing kernels' grid");
    FOR_RADIUS(r[k], launch_line, (grid, in, out, w[k], n_axis, inner, outer * inner));
  }
  // smooths `cur` (3 components of shape s) using `other` as the second buffer; returns the buffer that holds the result
  float* run(const char* fn, const Shape& s, float* cur, float* other) const {
    if (on[0]) {
      line(fn, 0, cur, other, 3, s.n0, (size_t)s.n1 * s.n2);
      std::swap(cur, other);
    }
    if (on[1]) {
      line(fn, 1, cur, other, (size_t)3 * s.n0, s.n1, (size_t)s.n2);
      std::swap(cur, other);
    }
    if (on[2]) {
      const size_t rows = (size_t)3 * s.n0 * s.n1;
      const size_t per_block = (size_t)kRowsPerBlock * kRowGroups;
      const dim3 grid((unsigned int)((rows + per_block - 1) / per_block), (unsigned int)((s.n2 + kRowTile - 1) / kRowTile));
      if (grid.y > 65535u) refuse(fn, "an axis is too long for the smoothing kernels' grid");
      FOR_RADIUS(r[2], launch_row, (grid, cur, other, w[2], rows, s.n2));
      std::swap(cur, other);
    }
    return cur;
  }
};

// the events that time the iterations of one chunk
struct IterationTimer {
  std::vector<hipEvent_t> ev;
  IterationTimer() = default;
  IterationTimer(const IterationTimer&) = delete;
  ~IterationTimer() {
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
  }
  void reserve(int n) {
    ev.reserve(n);
    while ((int)ev.size() < n) {
      hipEvent_t e = nullptr;
      HIP_TRY(hipEventCreate(&e));
      ev.push_back(e);
    }
  }
  double elapsed(int a, int b) const {
    float t = 0.f;
    HIP_TRY(hipEventElapsedTime(&t, ev[a], ev[b]));
    return t;
  }
};

mcgpu_register_options checked_options(const char* fn, const mcgpu_register_options* caller, bool whole) {
  mcgpu_register_options o;
  mcgpu::read_options(fn, "mcgpu_register_options", caller, o);
  if (o.nx < 1 || o.ny < 1 || o.nz < 1) refuse(fn, "every axis needs at least one voxel (" + std::to_string(o.nx) + " x " + std::to_string(o.ny) + " x " + std::to_string(o.nz) + ")");
  if ((unsigned long long)o.nx * o.ny * o.nz >= (1ULL << 31)) refuse(fn, "the volume has 2^31 voxels or more");
  for (int k = 0; k < 3; ++k)
    if (!(o.sigma[k] >= 0.0) || o.sigma[k] > 4.0 || radius_of(o.sigma[k]) > kMaxRadius)
      refuse(fn, "sigma[" + std::to_string(k) + "] = " + std::to_string(o.sigma[k]) + " is outside [0, 4]");
  if (!std::isfinite(o.tau)) refuse(fn, "tau is not finite");
  if (whole) {
    if (o.iterations < 0) refuse(fn, "iterations " + std::to_string(o.iterations) + " is negative");
    if (o.n_levels < 1 || o.n_levels > MCGPU_REGISTER_MAX_LEVELS)
      refuse(fn, "n_levels " + std::to_string(o.n_levels) + " is outside 1.." + std::to_string((int)MCGPU_REGISTER_MAX_LEVELS));
  }
  return o;
}

// the mean of double(d)^2 over the level; d goes to diff_host where that is given
double mean_squared_difference(const float* fixed, const float* moving, const float* u, const Shape& s, float* d_diff, float* diff_host,
                               double* d_partial) {
  hipLaunchKernelGGL(msd_kernel, dim3(kReduceBlocks), dim3(256), 0, nullptr, fixed, moving, u, s, diff_host ? d_diff : nullptr, d_partial);
  HIP_TRY(hipGetLastError());
  double sum;
  fold_blocks(d_partial, kReduceBlocks, 1, &sum);
  if (diff_host) HIP_TRY(hipMemcpy(diff_host, d_diff, s.voxels() * 4, hipMemcpyDeviceToHost));
  return sum / (double)s.voxels();
}

}  // namespace

extern "C" int mcgpu_register(const mcgpu_register_options* caller_o, const float* fixed, const float* moving, const unsigned char* fixed_mask, float* field_out,
                              mcgpu_register_report* report) {
  static const char* const fn = "mcgpu_register";
  ABI_BEGIN
  const mcgpu::Stopwatch call;
  const mcgpu_register_options o = checked_options(fn, caller_o, true);
  mcgpu::check_report(fn, "report", "mcgpu_register_report", report);
  if (!fixed || !moving || !field_out) refuse(fn, "null pointer: fixed, moving and field_out are required");
  const Shape full{o.nx, o.ny, o.nz};
  const size_t n_full = full.voxels();
  const float tau = (float)o.tau;
  mcgpu_register_report rep;
  memset(&rep, 0, sizeof rep);
  rep.n_levels = o.n_levels;

  HIP_TRY(hipSetDevice(o.device));
  mcgpu::CallDevice dev;
  dev.events();
  Smoother smoother;
  smoother.upload(dev, o.sigma);
  IterationTimer timer;
  const float *d_fixed, *d_moving;
  const unsigned char* d_mask = nullptr;
  {
    const mcgpu::Stopwatch upload;
    d_fixed = dev.upload(fixed, n_full);
    d_moving = dev.upload(moving, n_full);
    if (fixed_mask) d_mask = dev.upload(fixed_mask, n_full);
    rep.ms_upload += upload.ms();
  }
  double* d_partial = dev.alloc<double>(kReduceBlocks * sizeof(double));
  float* d_diff = o.differences ? dev.alloc<float>(n_full * 4) : nullptr;
  float* diff_host = o.differences;

  float* u_prev = nullptr;  // the field of the level before, of shape `prev`
  Shape prev{0, 0, 0};
  for (int level = o.n_levels - 1; level >= 0; --level) {
    const Shape s = level_shape(full, level);
    const size_t n = s.voxels();
    const float *f = d_fixed, *m = d_moving;
    const unsigned char* mask = d_mask;
    float *f_level = nullptr, *m_level = nullptr;
    unsigned char* mask_level = nullptr;
    float* u = dev.alloc<float>(3 * n * 4);
    float* u2 = dev.alloc<float>(3 * n * 4);
    {
      mcgpu::Stage st(dev, rep.ms_resize);
      if (level > 0) {
        const ResizeTables T = upload_tables(dev, full, s);
        f_level = dev.alloc<float>(n * 4);
        m_level = dev.alloc<float>(n * 4);
        hipLaunchKernelGGL(resize_linear_kernel, dim3(blocks_of(n)), dim3(256), 0, nullptr, d_fixed, f_level, full, s, T, 1.f);
        hipLaunchKernelGGL(resize_linear_kernel, dim3(blocks_of(n)), dim3(256), 0, nullptr, d_moving, m_level, full, s, T, 1.f);
        if (d_mask) {
          mask_level = dev.alloc<unsigned char>(n);
          hipLaunchKernelGGL(resize_nearest_kernel, dim3(blocks_of(n)), dim3(256), 0, nullptr, d_mask, mask_level, full, s, T);
        }
        f = f_level; m = m_level; mask = mask_level;
        st.done();
        release_tables(dev, T);
      } else {
        st.done();
      }
    }
    if (!u_prev) {
      HIP_TRY(hipMemset(u, 0, 3 * n * 4));
    } else {
      mcgpu::Stage st(dev, rep.ms_resize);
      const ResizeTables T = upload_tables(dev, prev, s);
      const int so[3] = {prev.n0, prev.n1, prev.n2}, sn[3] = {s.n0, s.n1, s.n2};
      for (int c = 0; c < 3; ++c) {
        const float scale = so[c] == 1 ? 1.f : (float)((double)(sn[c] - 1) / (double)(so[c] - 1));
        hipLaunchKernelGGL(resize_linear_kernel, dim3(blocks_of(n)), dim3(256), 0, nullptr, u_prev + (size_t)c * prev.voxels(), u + (size_t)c * n, prev, s, T, scale);
      }
      st.done();
      release_tables(dev, T);
      dev.release(u_prev);
    }
    {
      mcgpu::Stage st(dev, rep.ms_reduce);
      rep.msd_before[level] = mean_squared_difference(f, m, u, s, d_diff, diff_host, d_partial);
      if (diff_host) diff_host += n;
      st.done();
    }
    // the host waits once per kIterationChunk iterations: events between the launches split the time into force and smoothing
    for (int first = 0; first < o.iterations; first += kIterationChunk) {
      const int count = std::min(kIterationChunk, o.iterations - first);
      timer.reserve(2 * count + 1);
      HIP_TRY(hipEventRecord(timer.ev[0], nullptr));
      for (int it = 0; it < count; ++it) {
        hipLaunchKernelGGL(force_step_kernel, dim3(blocks_of(n)), dim3(256), 0, nullptr, f, m, mask, u, u2, s, tau);
        HIP_TRY(hipEventRecord(timer.ev[2 * it + 1], nullptr));
        std::swap(u, u2);
        if (smoother.run(fn, s, u, u2) != u) std::swap(u, u2);
        HIP_TRY(hipEventRecord(timer.ev[2 * it + 2], nullptr));
      }
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipEventSynchronize(timer.ev[2 * count]));
      for (int it = 0; it < count; ++it) {
        rep.ms_force += timer.elapsed(2 * it, 2 * it + 1);
        rep.ms_smooth += timer.elapsed(2 * it + 1, 2 * it + 2);
      }
    }
    {
      mcgpu::Stage st(dev, rep.ms_reduce);
      rep.msd_after[level] = mean_squared_difference(f, m, u, s, d_diff, diff_host, d_partial);
      if (diff_host) diff_host += n;
      st.done();
    }
    dev.release(u2);
    if (f_level) dev.release(f_level);
    if (m_level) dev.release(m_level);
    if (mask_level) dev.release(mask_level);
    u_prev = u;
    prev = s;
  }
  {
    const mcgpu::Stopwatch download;
    HIP_TRY(hipMemcpy(field_out, u_prev, 3 * n_full * 4, hipMemcpyDeviceToHost));
    rep.ms_upload += download.ms();
  }
  rep.peak_device_bytes = (unsigned long long)dev.peak;
  rep.ms_total = call.ms();
  mcgpu::write_report(report, rep);
  return 0;
  ABI_END
}

extern "C" int mcgpu_register_stage(const mcgpu_register_options* caller_o, int stage, const float* fixed, const float* moving, const float* field,
                                    const unsigned char* fixed_mask, void* out, mcgpu_register_report* report) {
  static const char* const fn = "mcgpu_register_stage";
  ABI_BEGIN
  const mcgpu::Stopwatch call;
  const mcgpu_register_options o = checked_options(fn, caller_o, false);
  mcgpu::check_report(fn, "report", "mcgpu_register_report", report);
  if (!out) refuse(fn, "null pointer: out");
  if (stage < MCGPU_REGISTER_STAGE_RESIZE_LINEAR || stage > MCGPU_REGISTER_STAGE_SMOOTH) refuse(fn, "stage " + std::to_string(stage) + " is outside 0..4");
  const Shape s{o.nx, o.ny, o.nz};
  const size_t n = s.voxels();
  const bool resize = stage == MCGPU_REGISTER_STAGE_RESIZE_LINEAR || stage == MCGPU_REGISTER_STAGE_RESIZE_NEAREST;
  Shape so{o.out_nx, o.out_ny, o.out_nz};
  if (resize) {
    if (so.n0 < 1 || so.n1 < 1 || so.n2 < 1) refuse(fn, "every axis of the resized volume needs at least one voxel");
    if ((unsigned long long)so.n0 * so.n1 * so.n2 >= (1ULL << 31)) refuse(fn, "the resized volume has 2^31 voxels or more");
  }
  auto need = [&](const void* p, const char* name) {
    if (!p) refuse(fn, std::string("null pointer: ") + name);
  };
  mcgpu_register_report rep;
  memset(&rep, 0, sizeof rep);
  HIP_TRY(hipSetDevice(o.device));
  mcgpu::CallDevice dev;
  dev.events();
  switch (stage) {
    case MCGPU_REGISTER_STAGE_RESIZE_LINEAR: {
      need(moving, "moving");
      const float* d_in = dev.upload(moving, n);
      float* d_out = dev.alloc<float>(so.voxels() * 4);
      const ResizeTables T = upload_tables(dev, s, so);
      mcgpu::Stage st(dev, rep.ms_resize);
      hipLaunchKernelGGL(resize_linear_kernel, dim3(blocks_of(so.voxels())), dim3(256), 0, nullptr, d_in, d_out, s, so, T, 1.f);
      st.done();
      HIP_TRY(hipMemcpy(out, d_out, so.voxels() * 4, hipMemcpyDeviceToHost));
      break;
    }
    case MCGPU_REGISTER_STAGE_RESIZE_NEAREST: {
      need(fixed_mask, "fixed_mask");
      const unsigned char* d_in = dev.upload(fixed_mask, n);
      unsigned char* d_out = dev.alloc<unsigned char>(so.voxels());
      const ResizeTables T = upload_tables(dev, s, so);
      mcgpu::Stage st(dev, rep.ms_resize);
      hipLaunchKernelGGL(resize_nearest_kernel, dim3(blocks_of(so.voxels())), dim3(256), 0, nullptr, d_in, d_out, s, so, T);
      st.done();
      HIP_TRY(hipMemcpy(out, d_out, so.voxels(), hipMemcpyDeviceToHost));
      break;
    }
    case MCGPU_REGISTER_STAGE_WARP_LINEAR: {
      need(moving, "moving");
      need(field, "field");
      const float* d_m = dev.upload(moving, n);
      const float* d_u = dev.upload(field, 3 * n);
      float* d_out = dev.alloc<float>(n * 4);
      mcgpu::Stage st(dev, rep.ms_force);
      hipLaunchKernelGGL(warp_linear_kernel, dim3(blocks_of(n)), dim3(256), 0, nullptr, d_m, d_u, d_out, s);
      st.done();
      HIP_TRY(hipMemcpy(out, d_out, n * 4, hipMemcpyDeviceToHost));
      break;
    }
    case MCGPU_REGISTER_STAGE_FORCE_STEP: {
      need(fixed, "fixed");
      need(moving, "moving");
      need(field, "field");
      const float* d_f = dev.upload(fixed, n);
      const float* d_m = dev.upload(moving, n);
      const float* d_u = dev.upload(field, 3 * n);
      const unsigned char* d_mask = fixed_mask ? dev.upload(fixed_mask, n) : nullptr;
      float* d_out = dev.alloc<float>(3 * n * 4);
      mcgpu::Stage st(dev, rep.ms_force);
      hipLaunchKernelGGL(force_step_kernel, dim3(blocks_of(n)), dim3(256), 0, nullptr, d_f, d_m, d_mask, d_u, d_out, s, (float)o.tau);
      st.done();
      HIP_TRY(hipMemcpy(out, d_out, 3 * n * 4, hipMemcpyDeviceToHost));
      break;
    }
    case MCGPU_REGISTER_STAGE_SMOOTH: {
      need(field, "field");
      Smoother smoother;
      smoother.upload(dev, o.sigma);
      float* d_u = dev.upload(field, 3 * n);
      float* d_other = dev.alloc<float>(3 * n * 4);
      mcgpu::Stage st(dev, rep.ms_smooth);
      const float* result = smoother.run(fn, s, d_u, d_other);
      st.done();
      HIP_TRY(hipMemcpy(out, result, 3 * n * 4, hipMemcpyDeviceToHost));
      break;
    }
  }
  rep.peak_device_bytes = (unsigned long long)dev.peak;
  rep.ms_total = call.ms();
  mcgpu::write_report(report, rep);
  return 0;
  ABI_END
}
