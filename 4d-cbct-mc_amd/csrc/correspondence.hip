// correspondence.hip -- the reference's CorrespondenceModel (cbctmc/registration/correspondence.py:149-226) resident on the device:
// displacement field(signal) = mean + coefficients (signal - mean_signal), 3N elements, K signal dimensions.
//
// The reference predicts the field in numpy (float64, 3N x K matrix-vector product) per respiratory state and hands it to the warp
// as an array; this engine then copied it to the device (12 N bytes per state).  The field is a function of K numbers and of arrays
// that never change, so the arrays stay here and the field is evaluated where it is consumed:
//   warp_index_kernel<FRAME, FieldFromModel<K, M>>   fused predict + warp of the palette index volume (the kernel and the field
//                                                   source are field_source.hpp's: one definition for both sources)
//   predict_field_kernel                            the same field source written out as float32 [3][N] (tests, host fallback)
//   fit_model_kernel                                mean and coefficients of a slab of elements from T fields and the T x K pseudo-inverse
//
// Access shape of the fused kernel (it is bound by its reads: 3 (sizeof(M) + 8 K) bytes per voxel against 1 byte written).
// A wave owns one 4x4x4 tile, lane = x | y << 2 | z << 4.  Frame 0 (field as [3][nz][ny][nx]): the four lanes of an x-run read
// consecutive elements and the four waves of a workgroup own four tiles that are neighbours in x -- runs of 16 elements (K = 2:
// 256 B of coefficients, 64 B of a float mean) in memory order already.  Frame 1 (the reference's [3][gx][gy][gz]): consecutive
// elements are neighbours in z, so a wave reads 16 runs of 4 elements per component -- 64 B of coefficients, half a 128-byte
// line, and the tile that uses the other half lies snx * sny tiles further on in memory order.  Chosen: in frame 1 the four waves
// of a workgroup take four tiles that are neighbours in z (FieldFromModel::kZRuns); the workgroup then reads runs of 16 elements
// like frame 0, every 128-byte line of the coefficients is asked for by two waves of ONE workgroup, and the writes stay whole
// 64-byte tiles.  Staging the runs through LDS was not tried: the lines are already consumed whole within a workgroup.
// Measured on an MI355X (profiles/correspondence_ab.md, tools/correspondence_bench.py; K = 2, float mean, frame 1): z runs 0.25 ms
// for the CIRS phantom (305 x 300 x 152, 862 MB: 3.4 TB/s) and 1.08 ms for 512 x 512 x 256 (4.2 GB: 3.85 TB/s, 61 % of what a copy
// reaches); tiles in memory order 0.40 ms and 2.00 ms.  The kernel that reads a stored field (12 bytes per voxel) takes 0.20 ms and
// 0.89 ms: the gather and the warp's arithmetic, not the field's bytes, are most of the fused kernel's time as well.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "device_model.hpp"
#include "field_source.hpp"
#include "geometry_device.hpp"

namespace mcgpu {
namespace {

template <int K, typename M>
FieldFromModel<K, M> field_of(const FieldModelArgs& m, size_t nvox) {
  FieldFromModel<K, M> f;
  f.mean = (const M*)m.mean; f.coef = m.coef; f.nvox = nvox;
  for (int k = 0; k < K; ++k) f.d[k] = m.d[k];
  return f;
}

template <class Field>
__global__ __launch_bounds__(256) void predict_field_kernel(Field field, size_t n, float* __restrict__ out) {
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) out[e] = field.value(e);
}

struct FitPinv { double p[kFitMaxTimesteps * kFieldModelMaxK]; };  // [T][K], read with wave-uniform indices (scalar loads of the kernel arguments)

// One thread per element v of the slab; the order of the operations is the definition (CorrespondenceModel.fit):
//   mean[v] = float((sum_t double(u_t[v])) / T), t ascending;  coef[v][k] = sum_t (double(u_t[v]) - double(mean[v])) P[t][k], t ascending
template <int K>
__global__ __launch_bounds__(256) void fit_model_kernel(const float* __restrict__ fields, size_t slab, int T, FitPinv P, float* __restrict__ mean, double* __restrict__ coef) {
  const size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= slab) return;
  double sum = 0.0;
  for (int t = 0; t < T; ++t) sum = sum + (double)fields[(size_t)t * slab + v];
  const float m = (float)(sum / (double)T);
  double acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0.0;
  for (int t = 0; t < T; ++t) {  // the slab's second read comes from the caches
    const double c = (double)fields[(size_t)t * slab + v] - (double)m;
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = acc[k] + c * P.p[t * K + k];
  }
  mean[v] = m;
#pragma unroll
  for (int k = 0; k < K; ++k) coef[v * K + k] = acc[k];
}

// calls f(FieldFromModel<K, M>) for the model's K and mean type
template <class F>
hipError_t with_field(const FieldModelArgs& m, size_t nvox, F&& f) {
  if (!m.mean || !m.coef || m.k < 1 || m.k > kFieldModelMaxK) return hipErrorInvalidValue;
  switch (m.k * 2 + (m.mean_is_f64 ? 1 : 0)) {
    case 2: f(field_of<1, float>(m, nvox)); break;
    case 3: f(field_of<1, double>(m, nvox)); break;
    case 4: f(field_of<2, float>(m, nvox)); break;
    case 5: f(field_of<2, double>(m, nvox)); break;
    case 6: f(field_of<3, float>(m, nvox)); break;
    case 7: f(field_of<3, double>(m, nvox)); break;
    case 8: f(field_of<4, float>(m, nvox)); break;
    default: f(field_of<4, double>(m, nvox)); break;
  }
  return hipGetLastError();
}

}  // namespace

hipError_t launch_warp_index_model(const GeometryRebuild& g, int warp_frame, hipStream_t stream) {
  if (warp_frame != 0 && warp_frame != 1) return hipErrorInvalidValue;
  const size_t columns = (size_t)g.sn[0] * g.sn[1];
  const unsigned blocks = warp_index_blocks(warp_frame == 0 ? columns * g.sn[2] * 64 : columns * (size_t)((g.sn[2] + 3) / 4) * 4 * 64);
  if (!blocks) return hipErrorInvalidValue;
  return with_field(g.model, (size_t)g.nx * g.ny * g.nz, [&](auto field) {
    using Field = decltype(field);
    if (warp_frame == 0)
      hipLaunchKernelGGL((warp_index_kernel<0, Field>), dim3(blocks), dim3(256), 0, stream, g.nx, g.ny, g.nz, g.sn[0], g.sn[1], g.sn[2], g.base_idx, field,
                         g.default_index, g.idx);
    else
      hipLaunchKernelGGL((warp_index_kernel<1, Field>), dim3(blocks), dim3(256), 0, stream, g.nx, g.ny, g.nz, g.sn[0], g.sn[1], g.sn[2], g.base_idx, field,
                         g.default_index, g.idx);
  });
}

hipError_t launch_predict_field(const FieldModelArgs& m, size_t n_elements, float* out, hipStream_t stream) {
  if (!out || n_elements == 0 || n_elements % 3 != 0) return hipErrorInvalidValue;
  const unsigned blocks = (unsigned)std::min<size_t>((n_elements + 255) / 256, 256u * 64u);
  return with_field(m, n_elements / 3, [&](auto field) {
    hipLaunchKernelGGL((predict_field_kernel<decltype(field)>), dim3(blocks), dim3(256), 0, stream, field, n_elements, out);
  });
}

hipError_t launch_fit_model(const float* fields, size_t slab, int T, const double* pinv, int K, float* mean, double* coef, hipStream_t stream) {
  if (!fields || !pinv || !mean || !coef || slab == 0 || T < 1 || T > kFitMaxTimesteps || K < 1 || K > kFieldModelMaxK) return hipErrorInvalidValue;
  FitPinv P;
  for (int i = 0; i < kFitMaxTimesteps * kFieldModelMaxK; ++i) P.p[i] = i < T * K ? pinv[i] : 0.0;
  const dim3 grid((unsigned)((slab + 255) / 256)), block(256);
  switch (K) {
    case 1: hipLaunchKernelGGL(fit_model_kernel<1>, grid, block, 0, stream, fields, slab, T, P, mean, coef); break;
    case 2: hipLaunchKernelGGL(fit_model_kernel<2>, grid, block, 0, stream, fields, slab, T, P, mean, coef); break;
    case 3: hipLaunchKernelGGL(fit_model_kernel<3>, grid, block, 0, stream, fields, slab, T, P, mean, coef); break;
    default: hipLaunchKernelGGL(fit_model_kernel<4>, grid, block, 0, stream, fields, slab, T, P, mean, coef); break;
  }
  return hipGetLastError();
}

}  // namespace mcgpu
