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
#include <hipfft/hipfft.h>

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mcgpu_amd.h"
#include "hip_host.hpp"
#include "knobs.hpp"

namespace {

#include "fdk_common.inc"

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

  FdkProblem(const mcgpu_fdk_options& opt, const FdkPlan& plan) : o(opt), P(plan), rows(plan, "mcgpu_fdk_reconstruct") {}

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
  P.upload();
  for (int first = 0; first < plan.n; first += plan.chunk) {
    const int m = std::min(plan.chunk, plan.n - first);
    P.filter(projections, first, m);
    P.backproject(first, m);
  }
  HIP_TRY(hipMemcpy(volume, P.d_vol, plan.nvox * 4, hipMemcpyDeviceToHost));
  if (report) *report = P.rep;
  return 0;
  ABI_END
}
