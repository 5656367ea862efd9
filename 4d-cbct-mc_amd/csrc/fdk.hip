// fdk.hip -- circular cone-beam FDK reconstruction for MI355X (what `rtkfdk --hardware cuda` does for
// the reference, cbctmc/reconstruction/reconstruction.py:22-69, reconstructors.py).  RTK itself is an un-vendored
// third-party dependency of the reference; the algorithm and RTK's geometry conventions are restated in oracle/fdk_oracle.py
// (parity unpinned against RTK, pinned by analytic phantoms) and implemented here and in fdk_common.inc (the row kernels) as:
//   weight      : water pre-correction polynomial, cosine weight, displaced-detector (half-fan) weight (backproject_column.inc),
//                 zero padding of the short side to a detector symmetric about the central ray                 (streaming)
//   ramp        : rows zero-extended to L (7500 at the reference's size), batched hipFFT R2C -> multiply by the real spectrum of
//                 the (Hann-apodised) ramp -> C2R (HBM streaming); ramp_rows = the direct LDS convolution kept for A/B
//                 (MCGPU_FDK_DIRECT_RAMP)
//   extend_rows : --pad (RTK TruncationCorrection): every row continued on both sides by next = ceil(pad x width) columns with
//                 the feathered point reflection 2 p(border) - p(mirror), so that a truncated edge does not ring     (streaming)
//   smooth_cols : --hannY low-pass along v (3 taps for 1.0)                                                     (streaming)
//   backproject : voxel-driven, bilinear; a thread owns one (x, z) column of the volume, precomputes everything that does
//                 not depend on y for a batch of 8 projections in registers, then walks y (backproject_column.inc): 4 loads + 10 flops per update;
//                 the filtered projections of a batch (5.7 MB each, padded) stay L2 / Infinity-Cache resident.  One voxel step
//                 is 3.9 detector pixels, so the 4 loads of a wave touch ~32 cache lines for 64 updates: the vector L1
//                 (64 B/clk/CU) bounds the kernel at ~1 update/clk/CU; measured 0.78                              (L1/L2 gather)
//   backproject_motion : the same sample taken where a linear motion model puts the voxel at the projection's breathing state
//                 (row f15, mcgpu_fdk_reconstruct_motion; the model is motion_model.inc's, P' stands above backproject_motion_kernel)         (L1/L2 gather)
#include <hipfft/hipfft.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <complex>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/mcgpu_amd.h"
#include "hip_host.hpp"
#include "knobs.hpp"

namespace {

#include "fdk_common.inc"
#include "motion_model.inc"

// in: [n][nv][nu] raw line integrals; out: [n][nv][nu_p] weighted rows, padded with pad_l zero columns on the left (and zeros on the
// right) so that an off-centre detector becomes symmetric about the central ray (RTK: DisplacedDetectorImageFilter)
__global__ void weight_kernel(const float* __restrict__ in, float* __restrict__ out, int nu, int nv, int n, int nu_p /* row stride of out */, int pad_l, float du, float dv,
                              float u0, float v0, float sdd, const ProjParam* __restrict__ pp, const float* __restrict__ w_dis /*[n][nu]*/,
                              const float* __restrict__ wpc, int n_wpc) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = (size_t)n * nv * nu_p;
  if (i >= total) return;
  const int ip = (int)(i % nu_p), iv = (int)((i / nu_p) % nv), k = (int)(i / ((size_t)nu_p * nv));
  const int iu = ip - pad_l;
  float v = 0.f;
  if (iu >= 0 && iu < nu) {
    v = in[((size_t)k * nv + iv) * nu + iu];
    if (n_wpc > 0) v = wpc_polynomial(wpc, n_wpc, v);
    v *= detector_weight(sdd, u0 + du * iu + pp[k].off_x, v0 + dv * iv + pp[k].off_y, w_dis[(size_t)k * nu + iu]);
  }
  out[i] = v;
}

__global__ __launch_bounds__(256, 4) void backproject_kernel(float* __restrict__ vol, const float* __restrict__ q /*[nb][nv][nu]*/, const BackArgs A) {
  const int ix = blockIdx.x * blockDim.x + threadIdx.x, iz = blockIdx.y;
  if (ix >= A.nx) return;
  const float X = A.x0 + A.sx * ix, Z = A.z0 + A.sz * iz;
  Column col[kBatch];
#pragma unroll
  for (int k = 0; k < kBatch; ++k) col[k] = column_setup<true>(A, k, X, Z);
  const size_t plane = (size_t)A.stride * A.nv;
  float* out = vol + ((size_t)iz * A.ny) * A.nx + ix;
  for (int iy = 0; iy < A.ny; ++iy) {
    const float Y = A.y0 + A.sy * iy;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < kBatch; ++k) {
      const Column& c = col[k];
      int iv;
      float av;
      if (c.iu >= 0 && detector_rows(fmaf(c.av_a, Y, c.av_b), A.nv, iv, av))
        acc = fmaf(c.wg, detector_sample(q + (size_t)k * plane + (size_t)iv * A.stride + A.u_first + c.iu, A.stride, c.au, av), acc);
    }
    out[(size_t)iy * A.nx] += acc;
  }
}

// ---- motion-compensated back-projection ------------------------------------------------------------------
// The model, its layout and the displacement d of a voxel for a projection's delta are motion_model.inc's.  What is this kernel's own:
// the model says where the material of a reference-phase voxel IS at the projection's state (the inverse of a pull-back field; nothing
// here inverts a model), so for the voxel at P = (X, Y, Z) projection i gives what plain FDK gives at P' = P + d:  xr = X'c - Z's,
// zr = X's + Z'c, U = sid - zr, mag = sdd / U, fu = (mag xr - off_x - u0_p) / du, fv = (mag Y' - off_y - v0) / dv, weight
// gap_i (sid / U)^2, and the bilinear sample of the filtered, padded row buffer through detector_rows / detector_sample.  A sample
// counts only when U > 0, columns iu, iu + 1 lie inside the padded detector and rows iv, iv + 1 inside the detector.
//
// With motion every voxel has its own (fu, fv): the column trick of backproject_kernel is gone.  One thread per voxel, x fastest
// (model loads and the volume's read-modify-write coalesce; neighbouring lanes hit neighbouring detector columns); the thread loads
// its model once per launch and loops over the projections of the batch, whose poses and deltas are wave-uniform kernel arguments
// (scalar loads).  A voxel has one owner and the projections are summed in order: no atomics, two calls give the same bytes.
//
// projections per launch of the motion kernel.  The per-projection state is scalar, so the batch only sets how often the model
// (3 (K + 1) floats per voxel) is re-read and the volume re-written.  Measured at the reference's size with K = 2 on one MI355X, all
// in one process (profiles/fdk_motion.md; 30 VGPRs, no scratch, 8 waves per SIMD; 28 - 38 VGPRs over K = 1..4): 8 projections
// 206.3 ms, 16 191.2 ms, 32 (one launch per resident chunk) 184.2 ms, against 105.1 ms of backproject_kernel; as committed 185.2 ms,
// 1.76 x.
constexpr int kMotionBatch = 32;

struct MotionArgs {  // a sibling of BackArgs: the three column kernels' layout is untouched
  int nx, ny, nz, nu, nv, nb;
  int u_first, stride;
  float x0, y0, z0, sx, sy, sz;
  float sid, sdd, inv_du, inv_dv, u0, v0;
  ProjParam pp[kMotionBatch];
  float delta[kMotionBatch][kMotionMaxK];  // [p][k], k < K
};

template <int K>
__global__ __launch_bounds__(256) void backproject_motion_kernel(float* __restrict__ vol, const float* __restrict__ q /*[nb][nv][stride]*/,
                                                                 const float* __restrict__ mean, const float* __restrict__ coef, const MotionArgs A) {
  const size_t nvox = (size_t)A.nx * A.ny * A.nz;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nvox) return;
  int ix, iy, iz;
  voxel_index(i, A.nx, A.ny, ix, iy, iz);
  const float X = A.x0 + A.sx * ix, Y = A.y0 + A.sy * iy, Z = A.z0 + A.sz * iz;
  MotionVoxel<K> model;
  model.load(mean, coef, nvox, i);
  const size_t plane = (size_t)A.stride * A.nv;
  float acc = 0.f;
  for (int p = 0; p < A.nb; ++p) {
    const ProjParam& pp = A.pp[p];
    float dx, dy, dz;
    model.displacement(A.delta[p], dx, dy, dz);
    const float Xp = X + dx, Yp = Y + dy, Zp = Z + dz;
    const float xr = fmaf(Xp, pp.c, -(Zp * pp.s)), zr = fmaf(Xp, pp.s, Zp * pp.c);
    const float U = A.sid - zr;
    const float inv_U = 1.0f / U;  // the one reciprocal of an update, correctly rounded
    const float mag = A.sdd * inv_U, r = A.sid * inv_U;
    int iu, iv;
    float au, av;
    const bool in_u = detector_rows((fmaf(mag, xr, -pp.off_x) - A.u0) * A.inv_du, A.nu, iu, au);  // the same rule along u: iu, iu + 1 inside
    const bool in_v = detector_rows((fmaf(mag, Yp, -pp.off_y) - A.v0) * A.inv_dv, A.nv, iv, av);
    if (U > 0.f && in_u && in_v)
      acc = fmaf(pp.gap * r * r, detector_sample(q + (size_t)p * plane + (size_t)iv * A.stride + A.u_first + iu, A.stride, au, av), acc);
  }
  vol[i] += acc;
}

// one reconstruction on the device: the plan's tables and a chunk of projections resident, the volume accumulated there
struct FdkProblem {
  const mcgpu_fdk_options& o;
  const FdkPlan& P;
  mcgpu::CallDevice dev;
  RowFilters rows;
  mcgpu_fdk_report rep = {0.0, 0.0};
  float *d_raw = nullptr, *d_in = nullptr, *d_tmp = nullptr, *d_vol = nullptr, *d_wdis = nullptr, *d_wpc = nullptr;
  ProjParam* d_pp = nullptr;
  const float* filtered = nullptr;  // what filter() left for backproject(): d_tmp, or d_in after the hannY pass
  // the motion model of mcgpu_fdk_reconstruct_motion, resident for the call
  int motion_K = 0;
  DeviceMotionModel model;
  std::vector<std::array<float, kMotionMaxK>> delta32;  // [n]
  double ms_upload_model = 0.0;

  FdkProblem(const mcgpu_fdk_options& opt, const FdkPlan& plan, const char* fn = "mcgpu_fdk_reconstruct") : o(opt), P(plan), rows(plan, fn) {}

  void upload() {
    d_raw = dev.alloc<float>((size_t)P.chunk * P.plane * 4);
    d_in = dev.alloc<float>((size_t)P.chunk * P.plane_p * 4);
    d_tmp = dev.alloc<float>((size_t)P.chunk * P.plane_p * 4);
    d_vol = dev.alloc_zeroed<float>(P.nvox * 4);
    rows.upload(dev, P.chunk);
    d_wdis = dev.upload(P.wdis);
    d_pp = dev.upload(P.pp);
    if (!P.wpc.empty()) d_wpc = dev.upload(P.wpc);
    dev.events();
  }

  // projections [first, first + m) onto the device, weighted, extended, ramp-filtered and smoothed along v
  void filter(const float* projections, int first, int m) {
    const size_t elems = (size_t)m * P.plane_p;
    HIP_TRY(hipMemcpy(d_raw, projections + (size_t)first * P.plane, (size_t)m * P.plane * 4, hipMemcpyHostToDevice));
    rows.prepare(m);
    mcgpu::Stage st(dev, rep.ms_filter);
    const unsigned gb = (unsigned)((elems + 255) / 256);
    hipLaunchKernelGGL(weight_kernel, dim3(gb), dim3(256), 0, nullptr, d_raw, d_in, P.nu, P.nv, m, P.stride, P.next + P.pad_l, (float)o.du, (float)o.dv, (float)o.u0,
                       (float)o.v0, (float)o.sdd, d_pp + first, d_wdis + (size_t)first * P.nu, d_wpc, (int)P.wpc.size());
    filtered = rows.run(m, d_in, d_tmp);
    st.done();
  }

  void backproject(int first, int m) {
    mcgpu::Stage st(dev, rep.ms_backproject);
    for (int b = 0; b < m; b += kBatch) {
      const BackArgs A = back_args(o, P, first + b, std::min(kBatch, m - b));
      hipLaunchKernelGGL(backproject_kernel, dim3((unsigned)((o.nx + 255) / 256), (unsigned)o.nz), dim3(256), 0, nullptr, d_vol,
                         filtered + (size_t)b * P.plane_p, A);
    }
    st.done();
  }

  // backproject(first, m) with moving voxels
  void backproject_motion(int first, int m) {
    mcgpu::Stage st(dev, rep.ms_backproject);
    const unsigned blocks = (unsigned)((P.nvox + 255) / 256);
    for (int b = 0; b < m; b += kMotionBatch) {
      MotionArgs A;
      memset(&A, 0, sizeof A);
      A.nx = o.nx; A.ny = o.ny; A.nz = o.nz; A.nu = P.nu_p; A.nv = P.nv; A.nb = std::min(kMotionBatch, m - b);
      A.u_first = P.next; A.stride = P.stride;
      A.x0 = (float)P.ox0; A.y0 = (float)P.oy0; A.z0 = (float)P.oz0; A.sx = (float)o.sx; A.sy = (float)o.sy; A.sz = (float)o.sz;
      A.sid = (float)o.sid; A.sdd = (float)o.sdd; A.inv_du = (float)(1.0 / o.du); A.inv_dv = (float)(1.0 / o.dv);
      A.u0 = (float)P.u0_p; A.v0 = (float)o.v0;
      std::copy_n(&P.pp[first + b], A.nb, A.pp);
      memcpy(A.delta, &delta32[first + b], A.nb * sizeof delta32[0]);
      const float* q = filtered + (size_t)b * P.plane_p;
      dispatch_motion_k(motion_K, [&](auto k) {
        hipLaunchKernelGGL(backproject_motion_kernel<decltype(k)::value>, dim3(blocks), dim3(256), 0, nullptr, d_vol, q, model.mean, model.coef, A);
      });
    }
    st.done();
  }

  // the whole reconstruction: tables (and the model) up, every resident chunk filtered and back-projected, the volume down
  void run(const float* projections, float* volume, const mcgpu_fdk_motion* motion) {
    upload();
    if (motion) {  // the model onto the device once, as float32; delta rounded once to float32
      mcgpu::Stopwatch sw;
      motion_K = motion->n_signal_dims;
      model = upload_motion_model(dev, motion->mean, motion->coefficients, motion_K, P.nvox);
      delta32 = round_deltas(motion->delta, P.n, motion_K);
      ms_upload_model = sw.ms();
    }
    for (int first = 0; first < P.n; first += P.chunk) {
      const int m = std::min(P.chunk, P.n - first);
      filter(projections, first, m);
      if (motion) backproject_motion(first, m);
      else backproject(first, m);
    }
    HIP_TRY(hipMemcpy(volume, d_vol, P.nvox * 4, hipMemcpyDeviceToHost));
  }
};

}  // namespace

extern "C" int mcgpu_fdk_reconstruct(const mcgpu_fdk_options* caller_o, const float* projections, float* volume, mcgpu_fdk_report* report) {
  ABI_BEGIN
  mcgpu_fdk_options local;
  mcgpu::read_options("mcgpu_fdk_reconstruct", "mcgpu_fdk_options", caller_o, local);
  if (!projections || !volume || !fdk_options_ok(local)) throw mcgpu::Error(-1, "!!ERROR!! mcgpu_fdk_reconstruct: bad argument");
  HIP_TRY(hipSetDevice(local.device));
  const FdkPlan plan = plan_fdk(local);
  FdkProblem P(local, plan);
  P.run(projections, volume, nullptr);
  if (report) *report = P.rep;
  return 0;
  ABI_END
}

extern "C" int mcgpu_fdk_reconstruct_motion(const mcgpu_fdk_options* caller_o, const mcgpu_fdk_motion* caller_m, const float* projections, float* volume,
                                            mcgpu_fdk_motion_report* report) {
  ABI_BEGIN
  const char* fn = "mcgpu_fdk_reconstruct_motion";
  const std::string bad_argument = std::string("!!ERROR!! ") + fn + ": bad argument";
  mcgpu_fdk_options local;
  mcgpu::read_options(fn, "mcgpu_fdk_options", caller_o, local);
  mcgpu_fdk_motion motion;
  mcgpu::read_options(fn, "mcgpu_fdk_motion", caller_m, motion);
  if (!projections || !volume || !fdk_options_ok(local)) throw mcgpu::Error(-1, bad_argument);
  check_motion_k(fn, motion.n_signal_dims);
  if (!motion.mean || !motion.coefficients || !motion.delta) throw mcgpu::Error(-1, bad_argument);
  check_delta(fn, motion.delta, (size_t)local.n_proj * motion.n_signal_dims);
  HIP_TRY(hipSetDevice(local.device));
  const FdkPlan plan = plan_fdk(local);
  FdkProblem P(local, plan, fn);
  P.run(projections, volume, &motion);
  if (report) *report = {P.rep.ms_filter, P.rep.ms_backproject, P.ms_upload_model, (unsigned long long)P.dev.peak};
  return 0;
  ABI_END
}
