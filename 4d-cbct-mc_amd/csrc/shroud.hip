// shroud.hip -- the breathing signal from the projections alone: the Amsterdam shroud (Zijp, Sonke, van Herk 2004: "Extraction of the
// respiratory signal from sequential thorax cone-beam X-ray images") and the 1-D registration of its consecutive columns: what RTK does
// with rtkamsterdamshroud followed by rtkextractshroudsignal.  RTK is absent here and parity with it is unpinned; what is pinned is the
// rule below, its float64 restatement (tests/shroud_ref.py) and the kernels held to that restatement.  DESIGN.md row f21.
//
// Input.  P[n][v][u], float32, [n_proj][nv][nu]: the normalised projections (line integrals) as fdk and rooster4d take them.  A region
// of interest selects the columns u_first .. u_first + u_count - 1 and the rows v_first .. v_first + v_count - 1 (a count of 0: from the
// first one to the image's edge; the default is everything).  m = v_count.
//
// Stage A, the shroud A[n][r] (float32, [n_proj][m]); row r belongs to detector row v = v_first + r.
//   t(u)    = fl32(P[n][min(v + 1, nv - 1)][u] - P[n][max(v - 1, 0)][u])       one float32 subtraction; the neighbour rows are clamped
//                                                                              to the image, not to the region of interest
//   D[n][r] = 0.5 * sum over the region's columns of (double) t(u)             float64; the order is fixed: two calls give the same bytes
//   A[n][r] = fl32(D[n][r] - (1 / w) * sum_{k = -h .. h} D[clamp(n + k, 0, n_proj - 1)][r])   the unsharp mask along the projection
//             axis, odd width w (default 17), h = (w - 1) / 2, in float64 with k ascending; w = 0: A = fl32(D); an even w is refused
// Stage B, the costs, float64 from the float32 A: for i = 1 .. n_proj - 1 and integer s in [-S, S] (S = max_shift, default 16 rows)
//   c_i(s)  = mean over r with 0 <= r < m and 0 <= r + s < m of (A[i][r + s] - A[i - 1][r])^2;   2 S < m is required
// Stage C, the signal, on the host in double: k* = argmin_s c_i(s), the lowest s on an exact tie; where k* is interior and
//   den = c(k* - 1) - 2 c(k*) + c(k* + 1) > 0:  shift_i = k* + 0.5 (c(k* - 1) - c(k* + 1)) / den,  else shift_i = k*;
//   x_0 = 0, x_i = x_{i - 1} + shift_i, in rows: positive means that the anatomy moves toward larger v.
// The amplitude is not calibrated (the registration sees the whole column, not the diaphragm alone): the signal serves for the phase.
// The default S = 16 rests on an estimate (about 5 rows a projection for a fast diaphragm on the half-fan geometry), not on a scan.
//
// The kernels:
//   row_sums   : the hot path, bound by HBM: a workgroup of 256 threads walks kBand rows of one projection over a span of 1024 columns.
//                A thread owns 4 columns (one 16-byte load a row where nu is a multiple of 4; the at most 3 + 3 columns before and after
//                the aligned body go to threads 0 .. 5 of span 0 as one more scalar; else 4 scalar loads, a wave reading 64 neighbours)
//                and keeps rows v - 1, v and v + 1 IN REGISTERS: a row is loaded once and serves the two outputs it belongs to.  Only the
//                2 rows around a band are read again by its neighbours (2 / kBand of the stack, which the caches may or may not hold).
//                Measured at 894 x 768 x 1024: 0.483 ms, 5.8 TB/s over the stack's bytes counted once (profiles/shroud.md).
//                The differences of 4 rows are summed per thread in float64 and reduced across the wave together (a butterfly that halves
//                the values a lane keeps while it still has more than one: 7 exchanges for 4 rows); the 4 waves' sums meet in LDS after
//                the walk, added in wave order.  No atomics: a row wider than 1024 columns has one partial sum per span,
//   combine    : D = 0.5 x the spans' partial sums, added in span order,
//   unsharp    : A from D, one thread per element,
//   cost       : one wave per (pair, shift): lanes take r = lo + lane, + 64, ..; xor butterfly; divided by the count.
// The projections arrive as a host array and go up kChunk at a time (halved while the device lacks the memory), as in wpc_fit.hip.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mcgpu_amd.h"
#include "hip_host.hpp"

namespace {

using mcgpu::blocks_of;  // kThreads is its 256
using mcgpu::refuse;

constexpr int kThreads = 256;
constexpr int kSpan = kThreads * 4;  // the columns of a row that one workgroup takes
constexpr int kBand = 32;            // the rows that one workgroup walks (a multiple of 4)
constexpr int kChunk = 32;           // projections resident at a time (shroud.py: UPLOAD_BATCH)
constexpr int kMaxGridZ = 16384;     // projections of one row_sums launch

// the region of interest and how its columns are split among spans and threads
struct RowArgs {
  int nu, nv;
  int u_first, u_end;  // columns [u_first, u_end)
  int v_first, m;
  int body, n4;        // vector path: the first column of the 16-byte aligned body and its length in float4
  int n_head, tail;    // vector path: columns before the body, and the first column after it (the tail is [tail, u_end))
  int n_total;         // projections of the whole call: what separates the spans in `partial`
};

struct RowRegs {
  float x[5];
};

// the 5 values that this thread holds of one row (what it does not own stays 0 and adds 0)
template <bool kVec>
__device__ __forceinline__ RowRegs load_row(const float* __restrict__ row, const RowArgs& A, int first, int extra) {
  RowRegs r = {{0.f, 0.f, 0.f, 0.f, 0.f}};
  if (kVec) {
    if (first >= 0) {
      const float4 q = *reinterpret_cast<const float4*>(row + first);
      r.x[0] = q.x; r.x[1] = q.y; r.x[2] = q.z; r.x[3] = q.w;
    }
    if (extra >= 0) r.x[4] = row[extra];
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (first + kThreads * k < A.u_end) r.x[k] = row[first + kThreads * k];
  }
  return r;
}

__device__ __forceinline__ double difference_sum(const RowRegs& next, const RowRegs& prev) {
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < 5; ++k) s += (double)(next.x[k] - prev.x[k]);
  return s;
}

// partial[span][n][r] = sum over the span's columns of (double) t(u).  grid: (spans, bands, projections of the launch); P is the launch's
// first projection, which is projection `n_first` of the call
template <bool kVec>
__global__ __launch_bounds__(kThreads) void row_sums_kernel(const float* __restrict__ P, double* __restrict__ partial, const RowArgs A, int n_first) {
  __shared__ double wave_sum[kThreads / 64][kBand];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int span = blockIdx.x, r0 = blockIdx.y * kBand;
  const int rows = min(kBand, A.m - r0);
  const float* img = P + (size_t)blockIdx.z * A.nv * A.nu;
  int first, extra = -1;
  if (kVec) {
    const int j = span * kThreads + t;
    first = j < A.n4 ? A.body + 4 * j : -1;
    if (span == 0) {
      if (t < A.n_head) extra = A.u_first + t;
      else if (A.tail + (t - A.n_head) < A.u_end) extra = A.tail + (t - A.n_head);
    }
  } else {
    first = A.u_first + span * kSpan + t;
  }
  const int v0 = A.v_first + r0, last = A.nv - 1;
  RowRegs a = load_row<kVec>(img + (size_t)max(v0 - 1, 0) * A.nu, A, first, extra);
  RowRegs b = load_row<kVec>(img + (size_t)v0 * A.nu, A, first, extra);
  for (int g = 0; g < rows; g += 4) {
    // rows past the band's end are computed from clamped rows and not kept
    double s[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const RowRegs c = load_row<kVec>(img + (size_t)min(v0 + g + q + 1, last) * A.nu, A, first, extra);
      s[q] = difference_sum(c, a);
      a = b;
      b = c;
    }
    // 4 values a lane -> 1: lanes 32 .. 63 keep rows 2 and 3, then lanes with bit 4 set keep the odd row
    const bool up32 = lane & 32, up16 = lane & 16;
    const double k0 = (up32 ? s[2] : s[0]) + __shfl_xor(up32 ? s[0] : s[2], 32);
    const double k1 = (up32 ? s[3] : s[1]) + __shfl_xor(up32 ? s[1] : s[3], 32);
    double z = (up16 ? k1 : k0) + __shfl_xor(up16 ? k0 : k1, 16);
    z += __shfl_xor(z, 8);
    z += __shfl_xor(z, 4);
    z += __shfl_xor(z, 2);
    z += __shfl_xor(z, 1);
    if ((lane & 15) == 0) wave_sum[wave][g + (lane >> 4)] = z;  // lane 0: row g, 16: g + 1, 32: g + 2, 48: g + 3
  }
  __syncthreads();
  if (t < rows) {
    const double sum = ((wave_sum[0][t] + wave_sum[1][t]) + wave_sum[2][t]) + wave_sum[3][t];
    partial[((size_t)span * A.n_total + n_first + blockIdx.z) * A.m + r0 + t] = sum;
  }
}

__global__ void combine_kernel(const double* __restrict__ partial, double* __restrict__ D, size_t count, int spans) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  double s = 0.0;
  for (int k = 0; k < spans; ++k) s += partial[(size_t)k * count + i];
  D[i] = 0.5 * s;
}

__global__ void unsharp_kernel(const double* __restrict__ D, float* __restrict__ A, int n, int m, int w) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)n * m) return;
  const int p = (int)(i / m), r = (int)(i % m);
  double d = D[i];
  if (w > 0) {
    const int h = (w - 1) / 2;
    double s = 0.0;
    for (int k = -h; k <= h; ++k) s += D[(size_t)min(max(p + k, 0), n - 1) * m + r];
    d = d - (1.0 / (double)w) * s;
  }
  A[i] = (float)d;
}

// costs[i - 1][s + S] for the pairs i = 1 .. n - 1: one wave each
__global__ __launch_bounds__(kThreads) void cost_kernel(const float* __restrict__ A, double* __restrict__ costs, int n, int m, int S) {
  const int lane = threadIdx.x & 63;
  const size_t w = (size_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  const int shifts = 2 * S + 1;
  if (w >= (size_t)(n - 1) * shifts) return;  // the whole wave
  const int i = (int)(w / shifts) + 1, s = (int)(w % shifts) - S;
  const int lo = max(0, -s), hi = min(m, m - s);
  const float* cur = A + (size_t)i * m + s;
  const float* before = A + (size_t)(i - 1) * m;
  double sum = 0.0;
  for (int r = lo + lane; r < hi; r += 64) {
    const double d = (double)cur[r] - (double)before[r];
    sum += d * d;
  }
  for (int x = 32; x > 0; x >>= 1) sum += __shfl_xor(sum, x);
  if (lane == 0) costs[w] = sum / (double)(hi - lo);
}

// ---- host -------------------------------------------------------------------------------------------------------------------

// the options of a call that reads projections, with the counts of 0 resolved; everything is refused here, before the first HIP call
mcgpu_shroud_options checked_projection_options(const char* fn, const mcgpu_shroud_options* caller) {
  mcgpu_shroud_options o;
  mcgpu::read_options(fn, "mcgpu_shroud_options", caller, o);
  if (o.n_proj < 1 || o.nu < 1 || o.nv < 1)
    refuse(fn, "bad size (n_proj " + std::to_string(o.n_proj) + ", nu " + std::to_string(o.nu) + ", nv " + std::to_string(o.nv) + ")");
  if (o.u_first < 0 || o.u_count < 0 || o.u_first >= o.nu || (long long)o.u_first + o.u_count > o.nu)
    refuse(fn, "the columns u_first " + std::to_string(o.u_first) + ", u_count " + std::to_string(o.u_count) + " are outside [0, " + std::to_string(o.nu) + ")");
  if (o.v_first < 0 || o.v_count < 0 || o.v_first >= o.nv || (long long)o.v_first + o.v_count > o.nv)
    refuse(fn, "the rows v_first " + std::to_string(o.v_first) + ", v_count " + std::to_string(o.v_count) + " are outside [0, " + std::to_string(o.nv) + ")");
  if (o.u_count == 0) o.u_count = o.nu - o.u_first;
  if (o.v_count == 0) o.v_count = o.nv - o.v_first;
  if (o.unsharp < 0 || (o.unsharp > 0 && o.unsharp % 2 == 0)) refuse(fn, "unsharp " + std::to_string(o.unsharp) + ": an odd width, or 0 for no mask");
  if (o.device < 0) refuse(fn, "device " + std::to_string(o.device) + " is negative");
  return o;
}

void check_shift(const char* fn, int max_shift, int m) {
  if (max_shift < 0 || 2LL * max_shift >= m)
    refuse(fn, "max_shift " + std::to_string(max_shift) + ": 0 <= 2 max_shift < " + std::to_string(m) + " rows is required");
}

RowArgs row_args(const mcgpu_shroud_options& o, bool vec) {
  RowArgs A;
  memset(&A, 0, sizeof A);
  A.nu = o.nu; A.nv = o.nv; A.u_first = o.u_first; A.u_end = o.u_first + o.u_count; A.v_first = o.v_first; A.m = o.v_count; A.n_total = o.n_proj;
  if (vec) {
    A.body = std::min((o.u_first + 3) / 4 * 4, A.u_end);
    A.n4 = (A.u_end - A.body) / 4;
    A.n_head = A.body - A.u_first;
    A.tail = A.body + 4 * A.n4;
  }
  return A;
}

// 16-byte loads need every row of every projection to begin on a 16-byte boundary
bool vector_rows(const mcgpu_shroud_options& o, const float* d_projections) { return o.nu % 4 == 0 && ((size_t)d_projections & 15) == 0; }

int spans_of(const mcgpu_shroud_options& o, bool vec) {
  const RowArgs A = row_args(o, vec);
  return std::max(1, vec ? (A.n4 + kThreads - 1) / kThreads : (o.u_count + kSpan - 1) / kSpan);
}

// stage A up to the partial sums, for `count` projections that lie at d_projections and are the call's n_first ..
void launch_row_sums(const mcgpu_shroud_options& o, bool vec, const float* d_projections, int n_first, int count, double* d_partial) {
  const RowArgs A = row_args(o, vec);
  const unsigned spans = (unsigned)spans_of(o, vec), bands = (unsigned)((A.m + kBand - 1) / kBand);
  for (int first = 0; first < count; first += kMaxGridZ) {
    const dim3 grid(spans, bands, (unsigned)std::min(kMaxGridZ, count - first));
    const float* p = d_projections + (size_t)first * o.nv * o.nu;
    if (vec) hipLaunchKernelGGL(row_sums_kernel<true>, grid, dim3(kThreads), 0, nullptr, p, d_partial, A, n_first + first);
    else hipLaunchKernelGGL(row_sums_kernel<false>, grid, dim3(kThreads), 0, nullptr, p, d_partial, A, n_first + first);
  }
}

// stages B and C from the shroud on the device: costs (optional) and the signal to the host
void costs_and_signal(mcgpu::CallDevice& dev, const float* d_shroud, int n, int m, int S, double* costs_out, double* signal, double& ms_cost) {
  const int shifts = 2 * S + 1;
  std::vector<double> costs((size_t)(n - 1) * shifts);
  if (n > 1) {
    double* d_costs = dev.alloc<double>(costs.size() * 8);
    mcgpu::Stage st(dev, ms_cost);
    hipLaunchKernelGGL(cost_kernel, dim3((unsigned)((costs.size() + kThreads / 64 - 1) / (kThreads / 64))), dim3(kThreads), 0, nullptr, d_shroud, d_costs, n, m, S);
    st.done();
    HIP_TRY(hipMemcpy(costs.data(), d_costs, costs.size() * 8, hipMemcpyDeviceToHost));
  }
  signal[0] = 0.0;
  for (int i = 1; i < n; ++i) {
    const double* c = costs.data() + (size_t)(i - 1) * shifts;
    int k = 0;
    for (int j = 1; j < shifts; ++j)
      if (c[j] < c[k]) k = j;
    double shift = (double)(k - S);
    if (k > 0 && k < shifts - 1) {
      const double den = c[k - 1] - 2.0 * c[k] + c[k + 1];
      if (den > 0.0) shift = (double)(k - S) + 0.5 * (c[k - 1] - c[k + 1]) / den;
    }
    signal[i] = signal[i - 1] + shift;
  }
  if (costs_out && !costs.empty()) memcpy(costs_out, costs.data(), costs.size() * 8);
}

// what a call that keeps `chunk` projections resident holds on the device
size_t footprint(const mcgpu_shroud_options& o, int chunk, int spans) {
  const size_t nm = (size_t)o.n_proj * o.v_count;
  return (size_t)chunk * o.nv * o.nu * 4 + (size_t)spans * nm * 8 + nm * 8 + nm * 4 + (size_t)std::max(o.n_proj - 1, 0) * (2 * o.max_shift + 1) * 8;
}

}  // namespace

extern "C" int mcgpu_shroud_extract(const mcgpu_shroud_options* caller_o, const float* projections, float* shroud, double* costs, double* signal,
                                    mcgpu_shroud_report* report) {
  static const char* const fn = "mcgpu_shroud_extract";
  ABI_BEGIN
  const mcgpu::Stopwatch call;
  const mcgpu_shroud_options o = checked_projection_options(fn, caller_o);
  check_shift(fn, o.max_shift, o.v_count);
  mcgpu::check_report(fn, "report", "mcgpu_shroud_report", report);
  if (!projections || !signal) refuse(fn, "null pointer: projections and signal are required");
  const int n = o.n_proj, m = o.v_count;
  const size_t plane = (size_t)o.nv * o.nu, nm = (size_t)n * m;
  mcgpu_shroud_report rep;
  memset(&rep, 0, sizeof rep);

  HIP_TRY(hipSetDevice(o.device));
  const int most_spans = (o.u_count + kSpan - 1) / kSpan;
  size_t free_bytes = 0, total_bytes = 0;
  HIP_TRY(hipMemGetInfo(&free_bytes, &total_bytes));
  int chunk = std::min(n, kChunk);
  while (chunk > 1 && footprint(o, chunk, most_spans) > free_bytes) chunk /= 2;
  if (footprint(o, chunk, most_spans) > free_bytes)
    refuse(fn, "the call needs " + std::to_string(footprint(o, chunk, most_spans)) + " bytes of device memory, the device has " + std::to_string(free_bytes) + " free");
  mcgpu::CallDevice dev;
  dev.events();
  float* d_raw = dev.alloc<float>((size_t)chunk * plane * 4);
  const bool vec = vector_rows(o, d_raw);
  const int spans = spans_of(o, vec);
  double* d_partial = dev.alloc<double>((size_t)spans * nm * 8);
  double* d_rows = dev.alloc<double>(nm * 8);
  float* d_shroud = dev.alloc<float>(nm * 4);
  for (int first = 0; first < n; first += chunk) {
    const int count = std::min(chunk, n - first);
    {
      const mcgpu::Stopwatch upload;
      HIP_TRY(hipMemcpy(d_raw, projections + (size_t)first * plane, (size_t)count * plane * 4, hipMemcpyHostToDevice));
      rep.ms_upload += upload.ms();
    }
    mcgpu::Stage st(dev, rep.ms_shroud);
    launch_row_sums(o, vec, d_raw, first, count, d_partial);
    st.done();  // the next upload overwrites what the kernel reads
  }
  {
    mcgpu::Stage st(dev, rep.ms_shroud);
    hipLaunchKernelGGL(combine_kernel, dim3(blocks_of(nm)), dim3(kThreads), 0, nullptr, d_partial, d_rows, nm, spans);
    hipLaunchKernelGGL(unsharp_kernel, dim3(blocks_of(nm)), dim3(kThreads), 0, nullptr, d_rows, d_shroud, n, m, o.unsharp);
    st.done();
  }
  if (shroud) HIP_TRY(hipMemcpy(shroud, d_shroud, nm * 4, hipMemcpyDeviceToHost));
  costs_and_signal(dev, d_shroud, n, m, o.max_shift, costs, signal, rep.ms_cost);
  rep.peak_device_bytes = (unsigned long long)dev.peak;
  rep.ms_total = call.ms();
  mcgpu::write_report(report, rep);
  return 0;
  ABI_END
}

extern "C" int mcgpu_shroud_signal(const mcgpu_shroud_options* caller_o, const float* shroud, double* costs, double* signal, mcgpu_shroud_report* report) {
  static const char* const fn = "mcgpu_shroud_signal";
  ABI_BEGIN
  const mcgpu::Stopwatch call;
  mcgpu_shroud_options o;
  mcgpu::read_options(fn, "mcgpu_shroud_options", caller_o, o);
  if (o.n_proj < 1 || o.v_count < 1) refuse(fn, "bad size (n_proj " + std::to_string(o.n_proj) + ", v_count " + std::to_string(o.v_count) + ")");
  check_shift(fn, o.max_shift, o.v_count);
  if (o.device < 0) refuse(fn, "device " + std::to_string(o.device) + " is negative");
  mcgpu::check_report(fn, "report", "mcgpu_shroud_report", report);
  if (!shroud || !signal) refuse(fn, "null pointer: shroud and signal are required");
  mcgpu_shroud_report rep;
  memset(&rep, 0, sizeof rep);
  HIP_TRY(hipSetDevice(o.device));
  mcgpu::CallDevice dev;
  dev.events();
  const float* d_shroud;
  {
    const mcgpu::Stopwatch upload;
    d_shroud = dev.upload(shroud, (size_t)o.n_proj * o.v_count);
    rep.ms_upload += upload.ms();
  }
  costs_and_signal(dev, d_shroud, o.n_proj, o.v_count, o.max_shift, costs, signal, rep.ms_cost);
  rep.peak_device_bytes = (unsigned long long)dev.peak;
  rep.ms_total = call.ms();
  mcgpu::write_report(report, rep);
  return 0;
  ABI_END
}

extern "C" int mcgpu_shroud_rows_device(const mcgpu_shroud_options* caller_o, const float* projections_device, double* rows_device, mcgpu_shroud_report* report) {
  static const char* const fn = "mcgpu_shroud_rows_device";
  ABI_BEGIN
  const mcgpu::Stopwatch call;
  const mcgpu_shroud_options o = checked_projection_options(fn, caller_o);
  mcgpu::check_report(fn, "report", "mcgpu_shroud_report", report);
  if (!projections_device || !rows_device) refuse(fn, "null pointer: projections_device and rows_device are required");
  mcgpu_shroud_report rep;
  memset(&rep, 0, sizeof rep);
  HIP_TRY(hipSetDevice(o.device));
  const bool vec = vector_rows(o, projections_device);
  const int spans = spans_of(o, vec);
  const size_t nm = (size_t)o.n_proj * o.v_count;
  mcgpu::CallDevice dev;
  dev.events();
  double* d_partial = dev.alloc<double>((size_t)spans * nm * 8);
  HIP_TRY(hipDeviceSynchronize());  // what the caller's streams still write to the stack
  {
    mcgpu::Stage st(dev, rep.ms_shroud);
    launch_row_sums(o, vec, projections_device, 0, o.n_proj, d_partial);
    hipLaunchKernelGGL(combine_kernel, dim3(blocks_of(nm)), dim3(kThreads), 0, nullptr, d_partial, rows_device, nm, spans);
    st.done();
  }
  rep.peak_device_bytes = (unsigned long long)dev.peak;
  rep.ms_total = call.ms();
  mcgpu::write_report(report, rep);
  return 0;
  ABI_END
}
