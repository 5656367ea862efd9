// resample.hpp -- interface of the image resampler (resample.hip), used by engine_geometry.cpp, and THE RESAMPLING RULE (the one
// statement of it in the C sources; DESIGN.md row f12 repeats it for readers of the documents).
//
// The rule describes sitk.Resample(image, new_size, sitk.Transform(), interpolator, origin, new_spacing, direction, default, pixelID) as
// the reference's resample_image_spacing calls it (cbctmc/utils.py:76-102; linear with default -1000 for the CT, nearest neighbour with
// default 0 for every segmentation file, cbctmc/mc/geometry.py:252-261).  Origin and direction do not change, so only sizes and spacings
// matter and the rule works per axis, on a 3-D array [n0][n1][n2] (the last axis runs fastest) with one spacing per array axis.  N = input
// size, os / ns = old / new spacing of the axis, all arithmetic in IEEE double exactly as parenthesised here:
//   size        M = (int)nearbyint(N * (os / ns)), default rounding mode (half to even, Python's round); M < 1 on any axis is refused
//   index       the continuous input index of output index i is  c = (i * ns) / os
//   inside      -0.5 <= c < N - 0.5, the upper bound strict; an output voxel with any axis outside gets the default value
//   nearest     input index floor(c + 0.5) (ITK's RoundHalfIntegerUp); the plan clamps it into [0, N - 1], which changes it outside only
//   linear      b = clamp(floor(c), 0, N - 1), b1 = min(b + 1, N - 1), d = max(c - b, 0)   (the edge value within half a voxel of the border)
//               the eight taps are blended with lerps a + (b - a) * d in double, never contracted into a fused multiply-add: along the
//               LAST array axis first, then the middle one, then the first (itk::LinearInterpolateImageFunction::EvaluateOptimized on an
//               image whose x is the array's last axis)
//   cast        double -> float32 rounds to nearest; double -> int16 / uint8 clamps to the type's range and then TRUNCATES toward zero
//               (ITK's static_cast behind its bounds check; it does not round), a NaN becoming 0; the default value takes the same cast.
//               resample_cast below is the only place that casts.
// Output type = input type.  Nearest-neighbour results are input elements as they are.
// With ns == os, c == i wherever i * ns is exact (always for the dyadic and small-integer spacings of CT files): the identity is then
// reproduced bit for bit.
//
// PARITY AGAINST SimpleITK ITSELF IS UNPINNED (as FDK's and ROOSTER's against RTK): neither SimpleITK nor ITK was at hand.
//   - ITK walks a row by interpolating the continuous index between the row's two ends, so its index can differ from c above in the last
//     ulp.  That can only show at exact ties: c + 0.5 integral, c = N - 0.5, or an integer-typed result that is exactly an integer.
//   - The truncating cast is ITK's source as remembered; it has not been checked against a build of ITK.
//   - The lerp order follows the ARRAY's axes.  The package resamples the [x][y][z] arrays of the MCGeometry frame, so a CT is blended
//     along z, then y, then x, where ITK on the file blends x, y, z: the same class of difference (last ulp, visible at exact ties only).
//     Context.resample_volume on a [z][y][x] array blends in ITK's order.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/mcgpu_amd.h"
#include "hip_host.hpp"

namespace mcgpu {

constexpr int kResampleNearest = 0, kResampleLinear = 1;

template <typename T>
__host__ __device__ inline T resample_cast(double v);
template <>
__host__ __device__ inline float resample_cast<float>(double v) { return (float)v; }
template <>
__host__ __device__ inline short resample_cast<short>(double v) {
  return v != v ? (short)0 : (short)(int)(v < -32768.0 ? -32768.0 : v > 32767.0 ? 32767.0 : v);
}
template <>
__host__ __device__ inline unsigned char resample_cast<unsigned char>(double v) {
  return v != v ? (unsigned char)0 : (unsigned char)(int)(v < 0.0 ? 0.0 : v > 255.0 ? 255.0 : v);
}

// The rule per output index, the three axes one after the other: entry off[k] + i belongs to output index i of axis k
struct ResamplePlan {
  int n_in[3], n_out[3], off[3];
  std::vector<int> base, next, nearest;  // always valid input indices of their axis
  std::vector<double> frac;
  std::vector<unsigned char> inside;
  size_t voxels_in() const { return (size_t)n_in[0] * n_in[1] * n_in[2]; }
  size_t voxels_out() const { return (size_t)n_out[0] * n_out[1] * n_out[2]; }
};
// Checks sizes and spacings (Error -1: non-positive size, non-finite or non-positive spacing, an axis that rounds to 0; Error -2: more than
// 2^31 - 1 voxels on either side) and builds the plan on the host.  `who` names the caller in the messages.
ResamplePlan make_resample_plan(const char* who, const int n_in[3], const double spacing_in[3], const double spacing_out[3]);
inline size_t resample_element_size(int dtype) { return dtype == MCGPU_IMAGE_FLOAT32 ? 4 : dtype == MCGPU_IMAGE_INT16 ? 2 : 1; }

struct ResampleArgs {  // the plan on the device
  int n_in[3], n_out[3], off[3];
  const int *base, *next, *nearest;
  const double* frac;
  const unsigned char* inside;
};
ResampleArgs upload_resample_plan(CallDevice& dev, const ResamplePlan& plan);
// `in` [n_in] -> `out` [n_out], device memory of element type `dtype` (MCGPU_IMAGE_*), on `stream`
hipError_t launch_resample(const ResampleArgs& a, int dtype, int interpolator, double default_value, const void* in, void* out, hipStream_t stream);

}  // namespace mcgpu
