// motion_model.inc -- the linear motion model on the reconstruction grid, stated once for fdk.hip's backproject_motion_kernel (DESIGN.md
// row f15) and rooster4d.hip's warp4_kernel (row f16); a sibling of backproject_column.inc.  Needs hip_host.hpp.
//
// The model.  The grid is the FDK grid [nz][ny][nx] in RTK's IEC frame, nvox = nx ny nz voxels, x fastest.  A model on it is
//   mean         [3][nz][ny][nx]     float32, mm, components along IEC X, Y, Z
//   coefficients [K][3][nz][ny][nx]  float32, mm per signal unit, 1 <= K <= kMotionMaxK
// and a state (of a projection, of a frame) enters as delta[k] = signal[k] - mean_signal[k], given in double and rounded once to
// float32.  The displacement of the voxel at P for that state is, per component, float32 with explicit fmaf, k ascending:
//     d = mean(P);  for k in 0..K-1: d = fmaf(coefficients[k](P), delta[k], d)
// What the displacement means (where the material of P is, or where to pull from) and what is sampled at P + d is the user's own.
//
// On the device a thread owns one voxel: MotionVoxel<K> loads its 3 (K + 1) model values once and gives the displacement for any
// number of states.  K is a template parameter: the thread loads exactly the model it has and the chain is straight-line code (a
// uniform bound over zero-filled slots measured the same time and bytes, profiles/fdk_motion.md: not kept).  The deltas of a launch
// are kernel arguments, [state][kMotionMaxK] with the slots k >= K zero; the pointer handed to displacement() must be wave-uniform,
// so that they are read through scalar loads.  Included inside the including file's anonymous namespace, so it includes nothing
// itself: it also needs <array>, <limits>, <string>, <type_traits> and <vector>.
#pragma once

constexpr int kMotionMaxK = 4;

// voxel i of the grid, x fastest -> its index along every axis
__device__ __forceinline__ void voxel_index(size_t i, int nx, int ny, int& ix, int& iy, int& iz) {
  ix = (int)(i % nx), iy = (int)((i / nx) % ny), iz = (int)(i / ((size_t)nx * ny));
}

template <int K>
struct MotionVoxel {
  float mx, my, mz;
  float cx[K], cy[K], cz[K];

  __device__ __forceinline__ void load(const float* __restrict__ mean, const float* __restrict__ coef, size_t nvox, size_t i) {
    mx = mean[i]; my = mean[nvox + i]; mz = mean[2 * nvox + i];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      cx[k] = coef[((size_t)3 * k + 0) * nvox + i];
      cy[k] = coef[((size_t)3 * k + 1) * nvox + i];
      cz[k] = coef[((size_t)3 * k + 2) * nvox + i];
    }
  }

  __device__ __forceinline__ void displacement(const float* delta /*[K], wave-uniform*/, float& dx, float& dy, float& dz) const {
    dx = mx; dy = my; dz = mz;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float d = delta[k];
      dx = fmaf(cx[k], d, dx);
      dy = fmaf(cy[k], d, dy);
      dz = fmaf(cz[k], d, dz);
    }
  }
};

// ---- host ------------------------------------------------------------------------------------------------------------------
// f(std::integral_constant<int, K>{}) for the K of a checked model: the one place that turns K into a template argument
template <class F>
void dispatch_motion_k(int K, F&& f) {
  switch (K) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    default: f(std::integral_constant<int, kMotionMaxK>{}); break;
  }
}

// The refusals that need no device.  Whether an array is given is the caller's own check and message.
inline void check_motion_k(const char* fn, int K) {
  if (K < 1 || K > kMotionMaxK) throw mcgpu::Error(-1, std::string("!!ERROR!! ") + fn + ": n_signal_dims must lie in 1..4");
}
inline void check_delta(const char* fn, const double* delta, size_t count) {
  for (size_t j = 0; j < count; ++j)  // NaN, infinite, or infinite once it is float32
    if (!(std::fabs(delta[j]) <= (double)std::numeric_limits<float>::max())) throw mcgpu::Error(-1, std::string("!!ERROR!! ") + fn + ": delta is not finite");
}

// delta [n][K] in double -> [n][kMotionMaxK] rounded once to float32, the slots k >= K zero: the rows of a kernel's delta argument
inline std::vector<std::array<float, kMotionMaxK>> round_deltas(const double* delta, int n, int K) {
  std::vector<std::array<float, kMotionMaxK>> out(n, std::array<float, kMotionMaxK>{});
  for (int j = 0; j < n; ++j)
    for (int k = 0; k < K; ++k) out[j][k] = (float)delta[(size_t)j * K + k];
  return out;
}

// a model resident on the device for one call, as float32
struct DeviceMotionModel { const float *mean = nullptr, *coef = nullptr; };
inline DeviceMotionModel upload_motion_model(mcgpu::CallDevice& dev, const float* mean, const float* coef, int K, size_t nvox) {
  return {dev.upload(mean, 3 * nvox), dev.upload(coef, (size_t)K * 3 * nvox)};
}
