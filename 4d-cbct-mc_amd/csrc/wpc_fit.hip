// wpc_fit.hip -- the normal equations of the empirical water pre-correction (Sourbelle et al. 2005; the reference: scripts/fit_wpc.py,
// which reconstructs the powers q^0 .. q^N of the normalised projections of a water cylinder with N + 1 rtkfdk runs, averages 50
// central slices of each and solves the weighted normal equations against a template of known attenuation).  DESIGN.md row f13 states
// the rule; tests/wpc_ref.py restates it in float64.  The N + 1 reconstructions share everything but the power, and the fit reads
// only a slab mean of each, so one pass does them all and no volume is ever formed:
//   power_weight   : reads each raw pixel once and writes the C = N + 1 weighted planes q^n x detector weight (backproject_column.inc),
//                    padded as fdk.hip's weight_kernel pads; q^n by wpc_polynomial's chain pw *= v                (streaming)
//   extension, ramp, hannY : fdk_common.inc's row kernels, on C planes per projection instead of one
//   interleave     : [projection][power][v][u] -> [projection][v][u][power] for the back-projector (layout 2)     (streaming)
//   slab_backproject<C> : backproject_column.inc's column with the y walk cut to the slab and C accumulators per thread: the bilinear
//                    weights of a sample are computed once and applied to every power; adds into fbar[c][z][x] once per launch
//                    (layout 1: two 8-byte loads per power and row; layout 2: the 2 C floats of a row are contiguous)  (L1/L2 gather)
//   normal_equations<C> : B and a in double from fbar, weight and template: a fixed grid, a fixed tree per block, the blocks'
//                    partial sums added on the host in block order
#include <hipfft/hipfft.h>

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/mcgpu_amd.h"
#include "hip_host.hpp"
#include "knobs.hpp"

namespace {

#include "fdk_common.inc"
#include "fixed_sum.inc"

constexpr int kMaxOrder = 7;
constexpr int kChunk = 32;          // projections resident at a time when they fit (a multiple of kBatch; halved down to kBatch when not)
constexpr int kReduceBlocks = 64;   // the fixed grid of normal_equations_kernel
// measured at the reference's size, order 5 (profiles/wpc_fit_ab.md): the interleaved back-projector takes 83.8 ms against 91.4 ms, but
// the pass that interleaves costs 30 ms of the filter stage: 644 ms a call against 622 ms
constexpr int kDefaultLayout = 1;

// in: [n][nv][nu] raw line integrals; out: [n][C][nv][stride]: plane c of projection k holds q^c x cosine weight x displaced-detector
// weight on the detector's columns and 0 on the padding, as weight_kernel with wpc = e_c leaves it
__global__ void power_weight_kernel(const float* __restrict__ in, float* __restrict__ out, int nu, int nv, int n, int stride, int pad_l, float du, float dv, float u0,
                                    float v0, float sdd, const ProjParam* __restrict__ pp, const float* __restrict__ w_dis /*[n][nu]*/, int C) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = (size_t)n * nv * stride;
  if (i >= total) return;
  const int ip = (int)(i % stride), iv = (int)((i / stride) % nv), k = (int)(i / ((size_t)stride * nv));
  const int iu = ip - pad_l;
  float v = 0.f, w = 0.f;
  if (iu >= 0 && iu < nu) {
    v = in[((size_t)k * nv + iv) * nu + iu];
    w = detector_weight(sdd, u0 + du * iu + pp[k].off_x, v0 + dv * iv + pp[k].off_y, w_dis[(size_t)k * nu + iu]);
  }
  const size_t plane = (size_t)nv * stride;
  float* o = out + (size_t)k * C * plane + (size_t)iv * stride + ip;
  float pw = 1.f;
  for (int c = 0; c < C; ++c) {
    o[(size_t)c * plane] = pw * w;
    pw *= v;
  }
}

// in: [n][C][nv][stride], of which columns [u_first, u_first + nu) are the detector's; out: [n][nv][nu][C]
__global__ void interleave_kernel(const float* __restrict__ in, float* __restrict__ out, int nu, int nv, int n, int stride, int u_first, int C) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = (size_t)n * nv * nu * C;
  if (i >= total) return;
  const int c = (int)(i % C), iu = (int)((i / C) % nu), iv = (int)((i / ((size_t)C * nu)) % nv), k = (int)(i / ((size_t)C * nu * nv));
  out[i] = in[(((size_t)k * C + c) * nv + iv) * stride + u_first + iu];
}

// fbar[c][iz][ix] += sum over the batch's projections and the slab's y of the weighted bilinear sample of power c.  A as for
// backproject_kernel; interleaved: q is [nb][nv][nu][C] and A.stride = nu * C, A.u_first = 0; else q is [nb][C][nv][stride]
// 4 waves per SIMD as backproject_kernel; the 8 powers of order 7 do not fit 128 registers and take 2
template <int C, bool kInterleaved>
__global__ __launch_bounds__(256, C <= 7 ? 4 : 2) void slab_backproject_kernel(float* __restrict__ fbar, const float* __restrict__ q, const BackArgs A, int y_first, int y_count) {
  const int ix = blockIdx.x * blockDim.x + threadIdx.x, iz = blockIdx.y;
  if (ix >= A.nx) return;
  const float X = A.x0 + A.sx * ix, Z = A.z0 + A.sz * iz;
  Column col[kBatch];
#pragma unroll
  for (int k = 0; k < kBatch; ++k) col[k] = column_setup<false>(A, k, X, Z);
  const size_t plane = (size_t)A.stride * A.nv;
  float acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 0.f;
  for (int iy = y_first; iy < y_first + y_count; ++iy) {
    const float Y = A.y0 + A.sy * iy;
#pragma unroll
    for (int k = 0; k < kBatch; ++k) {
      int iv;
      float av;
      if (col[k].iu >= 0 && detector_rows(fmaf(col[k].av_a, Y, col[k].av_b), A.nv, iv, av)) {
        const float au = col[k].au, w = col[k].wg;
        if (kInterleaved) {
          // pixels (iu, iu + 1) of a row are 2 C contiguous floats (4-byte aligned: global loads need no more)
          const float* r0 = q + (size_t)k * plane + (size_t)iv * A.stride + (size_t)col[k].iu * C;
          float lo[2 * C], hi[2 * C];
          __builtin_memcpy(lo, r0, 8 * C);
          __builtin_memcpy(hi, r0 + A.stride, 8 * C);
#pragma unroll
          for (int c = 0; c < C; ++c) acc[c] = fmaf(w, detector_lerp(au, av, lo[c], lo[C + c], hi[c], hi[C + c]), acc[c]);
        } else {
          const float* r0 = q + (size_t)k * C * plane + (size_t)iv * A.stride + A.u_first + col[k].iu;
#pragma unroll
          for (int c = 0; c < C; ++c) acc[c] = fmaf(w, detector_sample(r0 + (size_t)c * plane, A.stride, au, av), acc[c]);
        }
      }
    }
  }
  const size_t npix = (size_t)A.nz * A.nx;
  float* out = fbar + (size_t)iz * A.nx + ix;
#pragma unroll
  for (int c = 0; c < C; ++c) out[(size_t)c * npix] += acc[c];
}

// the slab sums become slab means (float32 division, the rule's)
__global__ void slab_mean_kernel(float* __restrict__ fbar, size_t total, float y_count) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < total) fbar[i] = fbar[i] / y_count;
}

// partial[block][t]: t runs over B[i][j], j >= i, row by row, then a[i].  Every thread takes the pixels block * 256 + thread + m * grid
// * 256 in rising m, a block adds its 256 sums of a term by the fixed tree, term after term (fixed_sum.inc): the same bytes on every call
template <int C>
__global__ __launch_bounds__(256) void normal_equations_kernel(const float* __restrict__ fbar /*[C][npix]*/, const float* __restrict__ weight, const float* __restrict__ tmpl,
                                                               size_t npix, double* __restrict__ partial) {
  constexpr int T = C * (C + 1) / 2 + C;
  double s[T];
#pragma unroll
  for (int t = 0; t < T; ++t) s[t] = 0.0;
  for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < npix; p += (size_t)gridDim.x * 256) {
    const double w = weight[p], tp = tmpl[p];
    double f[C];
#pragma unroll
    for (int c = 0; c < C; ++c) f[c] = fbar[(size_t)c * npix + p];
    int t = 0;
#pragma unroll
    for (int i = 0; i < C; ++i) {
      const double wf = w * f[i];
#pragma unroll
      for (int j = i; j < C; ++j) s[t++] += wf * f[j];
    }
#pragma unroll
    for (int i = 0; i < C; ++i) s[t++] += w * f[i] * tp;
  }
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const double total = block_tree(s[t]);
    if (threadIdx.x == 0) partial[(size_t)blockIdx.x * T + t] = total;
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
const char* const kFn = "mcgpu_wpc_fit";

[[noreturn]] void refuse(const std::string& what) { mcgpu::refuse(kFn, what); }

// the launches that depend on the compile-time number of powers
template <int C>
void launch_slab(bool interleaved, dim3 grid, float* fbar, const float* q, const BackArgs& A, int y_first, int y_count) {
  if (interleaved) hipLaunchKernelGGL((slab_backproject_kernel<C, true>), grid, dim3(256), 0, nullptr, fbar, q, A, y_first, y_count);
  else hipLaunchKernelGGL((slab_backproject_kernel<C, false>), grid, dim3(256), 0, nullptr, fbar, q, A, y_first, y_count);
}
template <int C>
void launch_reduce(const float* fbar, const float* weight, const float* tmpl, size_t npix, double* partial) {
  hipLaunchKernelGGL(normal_equations_kernel<C>, dim3(kReduceBlocks), dim3(256), 0, nullptr, fbar, weight, tmpl, npix, partial);
}
#define WPC_FOR_C(C, call, args)                              \
  switch (C) {                                                \
    case 2: call<2> args; break;                              \
    case 3: call<3> args; break;                              \
    case 4: call<4> args; break;                              \
    case 5: call<5> args; break;                              \
    case 6: call<6> args; break;                              \
    case 7: call<7> args; break;                              \
    case 8: call<8> args; break;                              \
    default: refuse("no kernel for " + std::to_string(C) + " powers"); \
  }

// device bytes of a call that keeps `chunk` projections resident.  hipFFT's work areas are not known before its plans exist: they
// are counted as one more spectrum buffer (what the 2^a 3^b 5^c lengths of plan_fdk took at the reference's size)
size_t footprint(const FdkPlan& P, const mcgpu_fdk_options& o, int C, bool interleaved, int chunk) {
  const size_t planes = (size_t)chunk * C, npix = (size_t)o.nz * o.nx;
  size_t b = (size_t)chunk * P.plane * 4 + 2 * planes * P.plane_p * 4;
  if (!P.direct) b += 2 * planes * P.nv * P.nk * sizeof(float2);
  if (interleaved) b += planes * P.nv * P.nu_p * 4;
  b += (size_t)C * npix * 4 + 2 * npix * 4 + (size_t)kReduceBlocks * (C * (C + 1) / 2 + C) * 8;
  b += (P.wext.size() + P.h.size() + P.ky.size() + P.wdis.size()) * 4 + P.pp.size() * sizeof(ProjParam);
  return b;
}

}  // namespace

extern "C" int mcgpu_wpc_fit(const mcgpu_wpc_fit_options* caller_o, const float* projections, const float* weight, const float* template_, double* B, double* a,
                             float* basis_mean, mcgpu_wpc_fit_report* report) {
  ABI_BEGIN
  const mcgpu::Stopwatch call;
  mcgpu_wpc_fit_options w;
  mcgpu::read_options(kFn, "mcgpu_wpc_fit_options", caller_o, w);
  for (const auto& arg : {std::make_pair((const void*)projections, "projections"), std::make_pair((const void*)weight, "weight"),
                          std::make_pair((const void*)template_, "template_"), std::make_pair((const void*)B, "B"), std::make_pair((const void*)a, "a")})
    if (!arg.first) refuse(std::string("null pointer: ") + arg.second);
  if (w.order < 1 || w.order > kMaxOrder) refuse("order " + std::to_string(w.order) + " is outside 1.." + std::to_string(kMaxOrder));
  mcgpu_fdk_options o;
  memset(&o, 0, sizeof o);
  o.struct_size = (unsigned int)sizeof o;
  o.n_proj = w.n_proj; o.nu = w.nu; o.nv = w.nv; o.du = w.du; o.dv = w.dv; o.u0 = w.u0; o.v0 = w.v0; o.sid = w.sid; o.sdd = w.sdd;
  o.gantry_deg = w.gantry_deg; o.proj_offset_x = w.proj_offset_x; o.proj_offset_y = w.proj_offset_y;
  o.nx = w.nx; o.ny = w.ny; o.nz = w.nz; o.sx = w.sx; o.sy = w.sy; o.sz = w.sz; o.ox = w.ox; o.oy = w.oy; o.oz = w.oz;
  o.hann = w.hann; o.hann_y = w.hann_y; o.pad = w.pad; o.device = w.device;
  if (!fdk_options_ok(o))
    refuse("bad FDK argument (n_proj " + std::to_string(o.n_proj) + ", nu " + std::to_string(o.nu) + ", nv " + std::to_string(o.nv) + ", volume " + std::to_string(o.nx) +
           " x " + std::to_string(o.ny) + " x " + std::to_string(o.nz) + ", du " + std::to_string(o.du) + ", dv " + std::to_string(o.dv) + ", sid " + std::to_string(o.sid) +
           ", sdd " + std::to_string(o.sdd) + ", gantry_deg " + (o.gantry_deg ? "given" : "NULL") + ")");
  if (w.y_count < 1) refuse("y_count " + std::to_string(w.y_count) + " is below 1");
  if (w.y_first < 0 || (long long)w.y_first + w.y_count > o.ny)
    refuse("the slab [" + std::to_string(w.y_first) + ", " + std::to_string((long long)w.y_first + w.y_count) + ") is outside [0, " + std::to_string(o.ny) + ")");
  if (w.channel_layout < 0 || w.channel_layout > 2) refuse("channel_layout " + std::to_string(w.channel_layout) + " is outside 0..2");
  const int C = w.order + 1;
  const bool interleaved = (w.channel_layout ? w.channel_layout : kDefaultLayout) == 2;

  const FdkPlan P = plan_fdk(o);
  HIP_TRY(hipSetDevice(o.device));
  size_t free_bytes = 0, total_bytes = 0;
  HIP_TRY(hipMemGetInfo(&free_bytes, &total_bytes));
  int chunk = std::min(P.n, kChunk);
  while (chunk > kBatch && footprint(P, o, C, interleaved, chunk) > free_bytes) chunk = std::max(kBatch, chunk / 2);
  const size_t needed = footprint(P, o, C, interleaved, chunk);
  if (needed > free_bytes) refuse("the call needs " + std::to_string(needed) + " bytes of device memory, the device has " + std::to_string(free_bytes) + " free");

  mcgpu_wpc_fit_report rep = {0.0, 0.0, 0.0, 0.0, 0.0, 0ull};
  mcgpu::CallDevice dev;
  RowFilters rows(P, kFn);
  const size_t npix = (size_t)o.nz * o.nx, planes = (size_t)chunk * C;
  constexpr int kMaxTerms = (kMaxOrder + 1) * (kMaxOrder + 2) / 2 + kMaxOrder + 1;
  const int T = C * (C + 1) / 2 + C;
  float* d_raw = dev.alloc<float>((size_t)chunk * P.plane * 4);
  float* d_in = dev.alloc<float>(planes * P.plane_p * 4);
  float* d_tmp = dev.alloc<float>(planes * P.plane_p * 4);
  float* d_il = interleaved ? dev.alloc<float>(planes * P.nv * P.nu_p * 4) : nullptr;
  float* d_fbar = dev.alloc_zeroed<float>((size_t)C * npix * 4);
  rows.upload(dev, (int)planes);
  const float* d_wdis = dev.upload(P.wdis);
  const ProjParam* d_pp = dev.upload(P.pp);
  const float* d_weight = dev.upload(weight, npix);
  const float* d_tmpl = dev.upload(template_, npix);
  double* d_partial = dev.alloc<double>((size_t)kReduceBlocks * T * 8);
  dev.events();

  size_t fft_work = 0;
  for (int first = 0; first < P.n; first += chunk) {
    const int m = std::min(chunk, P.n - first);
    {
      const mcgpu::Stopwatch upload;
      HIP_TRY(hipMemcpy(d_raw, projections + (size_t)first * P.plane, (size_t)m * P.plane * 4, hipMemcpyHostToDevice));
      rep.ms_upload += upload.ms();
    }
    rows.prepare(m * C);
    fft_work = std::max(fft_work, rows.fft.work_bytes());
    const float* filtered = nullptr;
    {
      mcgpu::Stage st(dev, rep.ms_filter);
      const size_t elems = (size_t)m * P.plane_p;
      hipLaunchKernelGGL(power_weight_kernel, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, nullptr, d_raw, d_in, P.nu, P.nv, m, P.stride, P.next + P.pad_l, (float)o.du,
                         (float)o.dv, (float)o.u0, (float)o.v0, (float)o.sdd, d_pp + first, d_wdis + (size_t)first * P.nu, C);
      filtered = rows.run(m * C, d_in, d_tmp);
      if (interleaved) {
        const size_t n_il = (size_t)m * C * P.nv * P.nu_p;
        hipLaunchKernelGGL(interleave_kernel, dim3((unsigned)((n_il + 255) / 256)), dim3(256), 0, nullptr, filtered, d_il, P.nu_p, P.nv, m, P.stride, P.next, C);
        filtered = d_il;
      }
      st.done();
    }
    {
      mcgpu::Stage st(dev, rep.ms_backproject);
      const size_t per_projection = interleaved ? (size_t)P.nv * P.nu_p * C : (size_t)C * P.plane_p;
      for (int b = 0; b < m; b += kBatch) {
        BackArgs A = back_args(o, P, first + b, std::min(kBatch, m - b));
        if (interleaved) { A.stride = P.nu_p * C; A.u_first = 0; }
        const dim3 grid((unsigned)((o.nx + 255) / 256), (unsigned)o.nz);
        WPC_FOR_C(C, launch_slab, (interleaved, grid, d_fbar, filtered + (size_t)b * per_projection, A, w.y_first, w.y_count));
      }
      st.done();
    }
  }
  {
    mcgpu::Stage st(dev, rep.ms_reduce);
    hipLaunchKernelGGL(slab_mean_kernel, dim3((unsigned)(((size_t)C * npix + 255) / 256)), dim3(256), 0, nullptr, d_fbar, (size_t)C * npix, (float)w.y_count);
    WPC_FOR_C(C, launch_reduce, (d_fbar, d_weight, d_tmpl, npix, d_partial));
    st.done();
  }
  double sum[kMaxTerms];
  fold_blocks(d_partial, kReduceBlocks, T, sum);
  int t = 0;
  for (int i = 0; i < C; ++i)
    for (int j = i; j < C; ++j) B[i * C + j] = B[j * C + i] = sum[t++];
  for (int i = 0; i < C; ++i) a[i] = sum[t++];
  if (basis_mean) HIP_TRY(hipMemcpy(basis_mean, d_fbar, (size_t)C * npix * 4, hipMemcpyDeviceToHost));
  rep.peak_device_bytes = (unsigned long long)(dev.peak + fft_work);
  rep.ms_total = call.ms();
  if (report) *report = rep;
  return 0;
  ABI_END
}
