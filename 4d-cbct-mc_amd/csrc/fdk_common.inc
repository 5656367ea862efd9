// fdk_common.inc -- what fdk.hip and wpc_fit.hip share of the FDK chain: the plan a reconstruction derives from its options on the
// host, the hipFFT plan pair, the row kernels between the weighting and the back-projection (extension, ramp, spectrum, hannY), and,
// through backproject_column.inc, the back-projector's column and the rules of the weighting pass.
// Included inside each file's unnamed namespace, after hip_host.hpp, knobs.hpp and <hipfft/hipfft.h>.

#include "backproject_column.inc"  // kBatch, ProjParam, BackArgs and the back-projector's column

// rtkfdk --pad (rtk::FFTProjectionsConvolutionImageFilter::PadInputImageRegion with TruncationCorrection > 0; restated in
// oracle/fdk_oracle.py: truncation_extension).  A row occupies columns [next, next + n) of its buffer row; the columns at
// distance d = 1..next beyond either border get w[d] * (2 p(border) - p(border -/+ d)).  One thread per (row, d).
__global__ void extend_rows_kernel(float* __restrict__ rows, int stride, int n, int next, size_t n_rows, const float* __restrict__ w /*[next + 1]*/) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_rows * (size_t)next) return;
  const int d = (int)(i % next) + 1;
  float* row = rows + (i / next) * (size_t)stride + next;
  row[-d] = w[d] * (2.0f * row[0] - row[d]);
  row[n - 1 + d] = w[d] * (2.0f * row[n - 1] - row[n - 1 - d]);
}

// out[row][i] = scale * sum_j in[row][j] * h[i - j + nu - 1];  one block per row, 256 threads, 4 consecutive outputs per thread
__global__ __launch_bounds__(256) void ramp_rows_kernel(const float* __restrict__ in, float* __restrict__ out, const float* __restrict__ h, int nu, float scale,
                                                        int j0, int j1 /* columns outside [j0, j1) are zero (padding) */) {
  extern __shared__ float lds[];
  float* row = lds;             // [nu]
  float* hk = lds + nu;         // [2 nu - 1 + 3] (padded with zeros so that the window may run past the ends)
  const size_t base = (size_t)blockIdx.x * nu;
  for (int i = threadIdx.x; i < nu; i += blockDim.x) row[i] = in[base + i];
  for (int i = threadIdx.x; i < 2 * nu + 2; i += blockDim.x) hk[i] = (i < 2 * nu - 1) ? h[i] : 0.f;
  __syncthreads();
  for (int i0 = 4 * threadIdx.x; i0 < nu; i0 += 4 * blockDim.x) {
    // window w_m = h[i0 + m - j + nu - 1], m = 0..3; stepping j -> j + 1 shifts it down by one
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int idx = i0 + nu - 1 - j0;  // index of w_0 for j = j0
    float w0 = hk[idx], w1 = hk[idx + 1], w2 = hk[idx + 2], w3 = hk[idx + 3];
    for (int j = j0; j < j1; ++j) {
      const float r = row[j];
      a0 = fmaf(r, w0, a0); a1 = fmaf(r, w1, a1); a2 = fmaf(r, w2, a2); a3 = fmaf(r, w3, a3);
      w3 = w2; w2 = w1; w1 = w0;
      --idx;
      w0 = (idx >= 0) ? hk[idx] : 0.f;
    }
    if (i0 + 0 < nu) out[base + i0 + 0] = a0 * scale;
    if (i0 + 1 < nu) out[base + i0 + 1] = a1 * scale;
    if (i0 + 2 < nu) out[base + i0 + 2] = a2 * scale;
    if (i0 + 3 < nu) out[base + i0 + 3] = a3 * scale;
  }
}

// in/out rows have `stride` floats, of which the first `nu` are used
__global__ void smooth_cols_kernel(const float* __restrict__ in, float* __restrict__ out, int nu, int stride, int nv, int n, const float* __restrict__ ky, int nk) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = (size_t)n * nv * nu;
  if (i >= total) return;
  const int iu = (int)(i % nu), iv = (int)((i / nu) % nv), k = (int)(i / ((size_t)nu * nv));
  const size_t plane = (size_t)k * nv * stride;
  const int hk = nk / 2;
  float acc = 0.f;
  for (int j = 0; j < nk; ++j) {
    int r = iv + j - hk;
    r = r < 0 ? 0 : (r > nv - 1 ? nv - 1 : r);  // edge replicated
    acc += ky[j] * in[plane + (size_t)r * stride + iu];
  }
  out[plane + (size_t)iv * stride + iu] = acc;
}

// spectrum[row][k] *= H[k] (real: the ramp kernel is even), k = 0 .. L/2
__global__ void spectrum_kernel(float2* __restrict__ spec, const float* __restrict__ H, int nk, size_t total) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const float h = H[i % nk];
  float2 v = spec[i];
  v.x *= h; v.y *= h;
  spec[i] = v;
}

// ---- host helpers ------------------------------------------------------------------------------------------------
void fft(std::vector<std::complex<double>>& a, bool inverse) {  // radix 2, in place
  const size_t n = a.size();
  for (size_t i = 1, j = 0; i < n; ++i) {
    size_t bit = n >> 1;
    for (; j & bit; bit >>= 1) j ^= bit;
    j ^= bit;
    if (i < j) std::swap(a[i], a[j]);
  }
  for (size_t len = 2; len <= n; len <<= 1) {
    const double ang = 2.0 * M_PI / (double)len * (inverse ? 1.0 : -1.0);
    const std::complex<double> wl(std::cos(ang), std::sin(ang));
    for (size_t i = 0; i < n; i += len) {
      std::complex<double> w(1.0, 0.0);
      for (size_t k = 0; k < len / 2; ++k) {
        const std::complex<double> u = a[i + k], v = a[i + k + len / 2] * w;
        a[i + k] = u + v;
        a[i + k + len / 2] = u - v;
        w *= wl;
      }
    }
  }
  if (inverse)
    for (auto& x : a) x /= (double)n;
}

// oracle/fdk_oracle.py: ramp_kernel
std::vector<double> ramp_kernel(int n_half, double hann) {
  std::vector<double> h(2 * n_half + 1, 0.0);
  for (int n = -n_half; n <= n_half; ++n) {
    if (n == 0) h[n + n_half] = 0.25;
    else if (n % 2 != 0) h[n + n_half] = -1.0 / (M_PI * M_PI * (double)n * (double)n);
  }
  if (hann > 0.0) {
    size_t m = 1;
    while (m < (size_t)8 * (2 * n_half + 1)) m *= 2;
    std::vector<std::complex<double>> buf(m, 0.0);
    for (int i = 0; i <= n_half; ++i) buf[i] = h[n_half + i];
    for (int i = 1; i <= n_half; ++i) buf[m - i] = h[n_half - i];
    fft(buf, false);
    const double fc = 0.5 * hann;
    for (size_t i = 0; i < m; ++i) {
      const double f = (i < m / 2) ? (double)i / (double)m : (double)i / (double)m - 1.0;
      const double win = (std::fabs(f) < fc) ? 0.5 * (1.0 + std::cos(M_PI * f / fc)) : 0.0;
      buf[i] *= win;
    }
    fft(buf, true);
    for (int i = 0; i <= n_half; ++i) h[n_half + i] = buf[i].real();
    for (int i = 1; i <= n_half; ++i) h[n_half - i] = buf[m - i].real();
  }
  return h;
}

std::vector<double> hann_y_kernel(double hann_y) {
  if (hann_y <= 0.0) return {1.0};
  if (hann_y == 1.0) return {0.25, 0.5, 0.25};
  const size_t m = 4096;
  const int n_half = 8;
  std::vector<std::complex<double>> buf(m);
  const double fc = 0.5 * hann_y;
  for (size_t i = 0; i < m; ++i) {
    const double f = (i < m / 2) ? (double)i / (double)m : (double)i / (double)m - 1.0;
    buf[i] = (std::fabs(f) < fc) ? 0.5 * (1.0 + std::cos(M_PI * f / fc)) : 0.0;
  }
  fft(buf, true);
  std::vector<double> k(2 * n_half + 1);
  for (int i = 0; i <= n_half; ++i) k[n_half + i] = buf[i].real();
  for (int i = 1; i <= n_half; ++i) k[n_half - i] = buf[m - i].real();
  double sum = 0.0;
  for (double v : k) sum += v;
  for (double& v : k) v /= sum;  // truncated support: keep the DC gain at exactly 1
  return k;
}

// oracle/fdk_oracle.py: displaced_weights (Wang 2002) for the columns of one projection
void displaced_weights(int nu, double du, double u0, double off_x, double sdd, float* w) {
  const double lo = u0 + off_x, hi = u0 + du * (nu - 1) + off_x;
  if (lo >= 0.0 || hi <= 0.0) { for (int i = 0; i < nu; ++i) w[i] = 1.f; return; }
  const double theta = std::min(-lo, hi);
  if (std::fabs((-lo) - hi) < 1e-9 * std::max(-lo, hi)) { for (int i = 0; i < nu; ++i) w[i] = 0.5f; return; }
  const double sign = (hi > -lo) ? 1.0 : -1.0;
  for (int i = 0; i < nu; ++i) {
    const double s = sign * (u0 + du * i + off_x);
    double v = (s > theta) ? 1.0 : 0.0;
    if (std::fabs(s) <= theta) v = 0.5 * (std::sin(M_PI * std::atan(s / sdd) / (2.0 * std::atan(theta / sdd))) + 1.0);
    w[i] = (float)v;
  }
}

// ---- what a reconstruction derives from its options on the host, before any device call ---------------------------------------
struct FdkPlan {
  int n, nu, nv;
  size_t plane, nvox;
  std::vector<ProjParam> pp;  // with the angular gaps
  std::vector<float> ky, wdis, wext, wpc;
  std::vector<float> h;       // direct: the ramp kernel's taps; else its spectrum H[nk] with scale / L folded in
  double ox0, oy0, oz0, u0_p, scale;
  int pad_l, pad_r, nu_p, next, nu_e, max_lag, L, stride, nk, chunk;
  bool direct;
  size_t plane_p, lds_ramp;
};

FdkPlan plan_fdk(const mcgpu_fdk_options& opt) {
  const mcgpu_fdk_options* o = &opt;
  FdkPlan P;
  const int n = P.n = o->n_proj, nu = P.nu = o->nu, nv = P.nv = o->nv;
  P.plane = (size_t)nu * nv;
  P.nvox = (size_t)o->nx * o->ny * o->nz;
  const std::vector<double> kyd = hann_y_kernel(o->hann_y);
  P.ky = std::vector<float>(kyd.begin(), kyd.end());
  std::vector<ProjParam>& pp = P.pp = std::vector<ProjParam>(n);
  P.wdis = std::vector<float>((size_t)n * nu);
  for (int k = 0; k < n; ++k) {
    const mcgpu::ProjectionPose q = mcgpu::projection_pose(*o, k);
    pp[k] = {(float)q.c, (float)q.s, (float)q.off_x, (float)q.off_y, 0.f};
    displaced_weights(nu, o->du, o->u0, q.off_x, o->sdd, &P.wdis[(size_t)k * nu]);
  }
  {
    // Angular weight of a projection = half the distance to its two neighbours on the circle (what rtkfdk takes from
    // the geometry file: ThreeDCircularProjectionGeometry::GetAngularGaps); 2 pi / n only for a uniform full arc.
    // Projections at the same angle share their gap.
    std::vector<std::pair<double, int>> by_angle(n);
    for (int k = 0; k < n; ++k) {
      double a = std::fmod(o->gantry_deg[k], 360.0);
      if (a < 0) a += 360.0;
      by_angle[k] = {a, k};
    }
    std::sort(by_angle.begin(), by_angle.end());
    std::vector<double> uniq;
    std::vector<int> count;
    for (int k = 0; k < n; ++k) {
      if (uniq.empty() || by_angle[k].first - uniq.back() > 1e-9) { uniq.push_back(by_angle[k].first); count.push_back(1); }
      else ++count.back();
    }
    const int m = (int)uniq.size();
    int u = -1;
    double last = -1.0;
    for (int k = 0; k < n; ++k) {
      if (u < 0 || by_angle[k].first - last > 1e-9) { ++u; last = uniq[u]; }
      double gap = 360.0;
      if (m > 1) {
        const double prev = uniq[(u + m - 1) % m], next = uniq[(u + 1) % m];
        double d = next - prev;
        if (d <= 0) d += 360.0;
        gap = 0.5 * d;
        if (m == 2) gap = 180.0;
      }
      pp[by_angle[k].second].gap = (float)(gap * M_PI / 180.0 / count[u]);
    }
  }
  P.ox0 = mcgpu::centred_origin(o->nx, o->sx, o->ox);
  P.oy0 = mcgpu::centred_origin(o->ny, o->sy, o->oy);
  P.oz0 = mcgpu::centred_origin(o->nz, o->sz, o->oz);
  // symmetric padding of an off-centre detector (oracle/fdk_oracle.py: symmetric_padding), from the double offsets as the Wang
  // weights take them: the float offsets of pp[] can move the ceiling by one column where -2 off / du is an integer (the reference's
  // -159.856 mm at 0.388 mm pixels)
  int pad_l = 0, pad_r = 0;
  {
    double off_min = 1e300, off_max = -1e300;
    for (int k = 0; k < n; ++k) {
      const double ox = mcgpu::offset_x(*o, k);
      off_min = std::min(off_min, ox);
      off_max = std::max(off_max, ox);
    }
    const double last = o->u0 + (nu - 1) * o->du;
    const double lo = o->u0 + off_min, hi = last + off_max;
    if (lo < 0.0 && hi > 0.0) {
      const double extent = std::max(std::max(-(o->u0 + off_min), -(o->u0 + off_max)), std::max(last + off_min, last + off_max));
      pad_l = std::max(0, (int)std::ceil((extent + (o->u0 + off_min)) / o->du - 1e-9));
      pad_r = std::max(0, (int)std::ceil((extent - (last + off_max)) / o->du - 1e-9));
    }
  }
  P.pad_l = pad_l; P.pad_r = pad_r;
  const int nu_p = P.nu_p = nu + pad_l + pad_r;
  P.u0_p = o->u0 - pad_l * o->du;
  // rtkfdk --pad: the ramp sees rows of nu_e = nu_p + 2 next columns (extend_rows_kernel); the back-projector only the nu_p
  // detector columns in their middle
  const int next = P.next = (o->pad > 0.0) ? std::min((int)std::ceil(o->pad * nu_p), nu_p - 1) : 0;
  const int nu_e = P.nu_e = nu_p + 2 * next;
  // Ramp filter: FFT (hipFFT, rows zero-extended to L >= 2 nu_p - 1: no wrap-around inside the nu_p columns that are used) or,
  // with MCGPU_FDK_DIRECT_RAMP, the direct LDS convolution (same result up to float rounding; tests compare both to the oracle)
  const bool direct = P.direct = mcgpu::knob_set("MCGPU_FDK_DIRECT_RAMP");
  // The ramp is a linear convolution evaluated as a circular one of length L.  Only the nu_p detector columns in the middle of
  // a row are ever read, and for those the lag between an output and any of the nu_e data columns is at most M = nu_p + next - 1:
  // with the kernel cut to |lag| <= M, L >= 2 M + 1 keeps every lag distinct (and L >= nu_e holds the row).  L = the smallest
  // even 2^a 3^b 5^c at or above that -- 7500 for the reference's half-fan rows with pad = 1 (nu_e = 5545, M = 3696), where
  // L >= 2 nu_e - 1 rounded up to a power of two would be 16384.
  const int max_lag = P.max_lag = nu_p + next - 1;
  int L = std::max(2 * max_lag + 1, nu_e);
  for (;; ++L) {
    if (L & 1) continue;
    int m = L;
    for (int f : {2, 3, 5})
      while (m % f == 0) m /= f;
    if (m == 1) break;
  }
  P.L = L;
  P.stride = direct ? nu_e : L;        // floats per detector row in the filtered buffers
  const int nk = P.nk = L / 2 + 1;
  P.plane_p = (size_t)P.stride * nv;
  P.chunk = std::min(n, direct ? 64 : 32);  // projections resident on the device at a time (multiple of kBatch)
  const std::vector<double> hd = ramp_kernel(nu_e - 1, o->hann);
  if (next > 0) {
    P.wext = std::vector<float>((size_t)next + 1, 0.f);
    for (int d = 1; d <= next; ++d) P.wext[(size_t)d] = next > 1 ? (float)std::pow(std::sin((double)(next - d) * M_PI / (2.0 * next - 2.0)), 0.75) : 0.f;
  }
  const double scale = P.scale = (o->sdd / o->sid) / o->du;
  if (direct) {
    P.h = std::vector<float>(hd.begin(), hd.end());
  } else {
    // spectrum of the kernel laid out circularly (lag n at index n mod L); real because the kernel is even;
    // the scale of the filter and hipFFT's missing 1/L are folded in
    // L is not a power of two: the (real, even) kernel's spectrum by its cosine sum, H[k] = h[0] + 2 sum_lag h[lag] cos(2 pi k lag / L),
    // with one table of cosines (30 M multiply-adds in double: tens of milliseconds, once per reconstruction)
    std::vector<double> cosine((size_t)L);
    for (int t = 0; t < L; ++t) cosine[(size_t)t] = std::cos(2.0 * M_PI * (double)t / (double)L);
    P.h = std::vector<float>((size_t)nk);
    const double* h0 = hd.data() + (nu_e - 1);  // h0[lag], lag = -(nu_e - 1) .. nu_e - 1
    for (int k = 0; k < nk; ++k) {
      double acc = h0[0];
      size_t t = 0;  // (k * lag) mod L
      for (int lag = 1; lag <= max_lag; ++lag) {
        t += (size_t)k;
        if (t >= (size_t)L) t -= (size_t)L;
        acc += 2.0 * h0[lag] * cosine[t];
      }
      P.h[(size_t)k] = (float)(acc * scale / (double)L);
    }
  }
  for (int j = 0; j < o->n_wpc; ++j) P.wpc.push_back((float)o->wpc[j]);
  P.lds_ramp = ((size_t)nu_e + 2 * nu_e + 2) * 4;
  return P;
}

struct FftPlans {  // the batched R2C / C2R pair of one chunk size (hipfftDestroy returns hipfftResult: no mcgpu::Owned)
  hipfftHandle fwd = 0, inv = 0;
  int rows = 0;
  std::string fn = "mcgpu_fdk_reconstruct";  // the entry point named in the errors
  FftPlans() = default;
  FftPlans(const FftPlans&) = delete;
  ~FftPlans() { reset(); }
  void reset() {
    if (fwd) hipfftDestroy(fwd);
    if (inv) hipfftDestroy(inv);
    fwd = inv = 0;
    rows = 0;
  }
  size_t work_bytes() const {  // of both plans' work areas, which hipFFT allocates with the plans
    size_t a = 0, b = 0;
    if (fwd) (void)hipfftGetSize(fwd, &a);
    if (inv) (void)hipfftGetSize(inv, &b);
    return a + b;
  }
  void make(int L, int nk, int n_rows) {
    if (rows == n_rows) return;
    reset();
    int len[1] = {L};
    if (hipfftPlanMany(&fwd, 1, len, nullptr, 1, L, nullptr, 1, nk, HIPFFT_R2C, n_rows) != HIPFFT_SUCCESS ||
        hipfftPlanMany(&inv, 1, len, nullptr, 1, nk, nullptr, 1, L, HIPFFT_C2R, n_rows) != HIPFFT_SUCCESS)
      throw mcgpu::Error(-1, "!!ERROR!! " + fn + ": hipfftPlanMany failed");
    rows = n_rows;
  }
};


// The row filters between the weighting and the back-projection, on `planes` detector planes [nv][stride] at a time (a plane is one
// projection for mcgpu_fdk_reconstruct, one power of one projection for mcgpu_wpc_fit): the plan's tables on the device, and the
// launches of the --pad extension, the ramp (hipFFT, or the direct LDS convolution under MCGPU_FDK_DIRECT_RAMP) and the hannY pass
struct RowFilters {
  const FdkPlan& P;
  FftPlans fft;
  float *d_wext = nullptr, *d_h = nullptr, *d_ky = nullptr;
  float2* d_spec = nullptr;

  RowFilters(const FdkPlan& plan, const char* fn) : P(plan) { fft.fn = fn; }

  void upload(mcgpu::CallDevice& dev, int max_planes) {
    if (P.next > 0) d_wext = dev.upload(P.wext);
    d_h = dev.upload(P.h);
    if (!P.direct) d_spec = dev.alloc<float2>((size_t)max_planes * P.nv * P.nk * sizeof(float2));
    d_ky = dev.upload(P.ky);
    if (P.direct && P.lds_ramp > 64 * 1024)
      HIP_TRY(hipFuncSetAttribute((const void*)ramp_rows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)P.lds_ramp));
  }
  // outside a Stage: one batched plan per number of planes (at most two in a call: the full chunks and the last one)
  void prepare(int planes) {
    if (!P.direct) fft.make(P.L, P.nk, planes * P.nv);
  }
  // d_in holds the weighted planes; returns the buffer that holds the filtered ones: d_tmp, or d_in after the hannY pass
  const float* run(int planes, float* d_in, float* d_tmp) {
    const int nv = P.nv, next = P.next, nu_e = P.nu_e, stride = P.stride, nk = P.nk;
    if (next > 0) {
      const size_t ne = (size_t)planes * nv * next;
      hipLaunchKernelGGL(extend_rows_kernel, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, nullptr, d_in, stride, P.nu_p, next, (size_t)planes * nv, d_wext);
    }
    if (P.direct) {
      hipLaunchKernelGGL(ramp_rows_kernel, dim3((unsigned)(planes * nv)), dim3(256), P.lds_ramp, nullptr, d_in, d_tmp, d_h, nu_e, (float)P.scale, next > 0 ? 0 : P.pad_l,
                         next > 0 ? nu_e : P.pad_l + P.nu);
    } else {
      if (hipfftExecR2C(fft.fwd, d_in, (hipfftComplex*)d_spec) != HIPFFT_SUCCESS) throw mcgpu::Error(-1, "!!ERROR!! " + fft.fn + ": hipfftExecR2C failed");
      const size_t ns = (size_t)planes * nv * nk;
      hipLaunchKernelGGL(spectrum_kernel, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, nullptr, d_spec, d_h, nk, ns);
      if (hipfftExecC2R(fft.inv, (hipfftComplex*)d_spec, d_tmp) != HIPFFT_SUCCESS) throw mcgpu::Error(-1, "!!ERROR!! " + fft.fn + ": hipfftExecC2R failed");
    }
    if (P.ky.size() <= 1) return d_tmp;
    const size_t na = (size_t)planes * nv * nu_e;
    hipLaunchKernelGGL(smooth_cols_kernel, dim3((unsigned)((na + 255) / 256)), dim3(256), 0, nullptr, d_tmp, d_in, nu_e, stride, nv, planes, d_ky, (int)P.ky.size());
    return d_in;
  }
};

// what mcgpu_fdk_reconstruct refuses of its options (mcgpu_wpc_fit refuses the same)
inline bool fdk_options_ok(const mcgpu_fdk_options& o) {
  return o.n_proj >= 1 && o.nu >= 2 && o.nv >= 2 && o.nx >= 1 && o.ny >= 1 && o.nz >= 1 && o.gantry_deg && o.du > 0 && o.dv > 0 && o.sid > 0 && o.sdd > 0;
}

// the back-projection arguments of projections [first, first + nb) (nb <= kBatch)
inline BackArgs back_args(const mcgpu_fdk_options& o, const FdkPlan& P, int first, int nb) {
  BackArgs A;
  A.nx = o.nx; A.ny = o.ny; A.nz = o.nz; A.nu = P.nu_p; A.u_first = P.next; A.stride = P.stride; A.nv = P.nv; A.nb = nb;
  A.x0 = (float)P.ox0; A.y0 = (float)P.oy0; A.z0 = (float)P.oz0; A.sx = (float)o.sx; A.sy = (float)o.sy; A.sz = (float)o.sz;
  A.sid = (float)o.sid; A.sdd = (float)o.sdd; A.inv_du = (float)(1.0 / o.du); A.inv_dv = (float)(1.0 / o.dv);
  A.u0 = (float)P.u0_p; A.v0 = (float)o.v0;
  for (int k = 0; k < kBatch; ++k) A.pp[k] = (k < nb) ? P.pp[first + k] : ProjParam{1.f, 0.f, 0.f, 0.f, 0.f};
  return A;
}
