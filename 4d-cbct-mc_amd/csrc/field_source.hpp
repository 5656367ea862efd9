// field_source.hpp -- where the warp of the palette index volume takes its displacement field from, and the warp kernel itself
// (one definition for geometry_device.hip, which reads a field from memory, and correspondence.hip, which evaluates the resident
// correspondence model in place).
//
// A field source gives the three displacement components of one voxel of the field's own layout ([3][N], component-major):
//   FieldInMemory          u_c = dvf[c N + f]                                   12 bytes read per voxel
//   FieldFromModel<K, M>   u_c = float(double(mean[e]) + (coef[e][0] d[0] + coef[e][1] d[1] + ...)),  e = c N + f,
//                          products summed left to right in double, no fused multiply-add (the TUs are built with
//                          -ffp-contract=off): the arithmetic CorrespondenceModel.predict_field32 states in numpy, bit for bit.
//                          3 (sizeof(M) + 8 K) bytes read per voxel; `coef` is double[3N][K], the layout the reference's
//                          CorrespondenceModel keeps (cbctmc/registration/correspondence.py:202), so a loaded model is uploaded as it is.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "device_model.hpp"

namespace mcgpu {

// identity + displacement -> normalised -> grid_sample(align_corners=True) un-normalisation -> nearbyint, in float32 like
// torch (see warp.hip; known answers tests/golden/warp_kat.npz)
__device__ __forceinline__ float nearest_sample(float loc, int n) {
  const float t = 2.0f * (__fdiv_rn(loc, (float)(n - 1)) - 0.5f);
  return rintf(((t + 1.0f) / 2.0f) * (float)(n - 1));
}

struct FieldInMemory {
  static constexpr bool kZRuns = false;
  const float* __restrict__ dvf;
  size_t nvox;
  __device__ __forceinline__ void load(size_t f, float& ux, float& uy, float& uz) const {
    ux = dvf[f]; uy = dvf[nvox + f]; uz = dvf[2 * nvox + f];
  }
};

template <int K, typename MeanT>
struct FieldFromModel {
  static_assert(K >= 1 && K <= 4, "1 <= K <= 4");
  static constexpr bool kZRuns = true;  // frame 1: four z-adjacent tiles per workgroup (warp_index_kernel)
  const MeanT* __restrict__ mean;
  const double* __restrict__ coef;
  size_t nvox;
  double d[K];  // signal - mean_signal
  __device__ __forceinline__ float value(size_t e) const {
    double c[K];
    if constexpr (K == 2) {  // the reference's case (signal and its derivative): one 16-byte load per component
      const double2 v = *reinterpret_cast<const double2*>(coef + 2 * e);
      c[0] = v.x; c[1] = v.y;
    } else if constexpr (K == 4) {
      const double2 v = *reinterpret_cast<const double2*>(coef + 4 * e), w = *reinterpret_cast<const double2*>(coef + 4 * e + 2);
      c[0] = v.x; c[1] = v.y; c[2] = w.x; c[3] = w.y;
    } else {
#pragma unroll
      for (int k = 0; k < K; ++k) c[k] = coef[(size_t)K * e + k];
    }
    double acc = c[0] * d[0];
#pragma unroll
    for (int k = 1; k < K; ++k) acc = acc + c[k] * d[k];
    return (float)((double)mean[e] + acc);
  }
  __device__ __forceinline__ void load(size_t f, float& ux, float& uy, float& uz) const {
    ux = value(f); uy = value(nvox + f); uz = value(2 * nvox + f);
  }
};

// FRAME 0: the field is given in the engine's frame, [3][nz][ny][nx], components (x, y, z).
// FRAME 1: the field is given in the frame of the reference's MCGeometry arrays, [3][gx][gy][gz] with the engine volume =
//          rot90(k=3) of them in the x/y plane (create_mcgpu_geometry, cbctmc/mc/geometry.py:589-599): engine voxel
//          (x, y, z) is geometry voxel (gx, gy, gz) = (ny - 1 - y, x, z).  The warp is evaluated in the geometry's frame,
//          where the reference evaluates it (ties and border samples do not survive a mirrored axis), and only the
//          result is addressed in the engine's layout.
// Source and destination are TILED index volumes (device_model.hpp: tiled_voxel).  One thread per voxel of the padded
// grid: a wave writes one whole 64-byte tile (the padding voxels of edge tiles get the default).  The waves take the tiles in
// memory order, except for a source with kZRuns in frame 1: there the four waves of a workgroup take four tiles that are
// neighbours in z, so that the workgroup reads runs of 16 consecutive field elements (correspondence.hip says why).
template <int FRAME, class Field>
__global__ __launch_bounds__(256) void warp_index_kernel(int nx, int ny, int nz, int snx, int sny, int snz, const unsigned char* __restrict__ base,
                                                         Field field, unsigned char default_index, unsigned char* __restrict__ out) {
  constexpr bool kZRuns = FRAME == 1 && Field::kZRuns;
  const unsigned int snxy = (unsigned int)(snx * sny);
  const size_t nwave = kZRuns ? (size_t)snxy * (size_t)((snz + 3) / 4) * 4 : (size_t)snxy * snz;  // < 2^32 (warp_index_blocks)
  const size_t nslot = nwave * 64;
  for (size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x; s < nslot; s += (size_t)gridDim.x * blockDim.x) {
    const unsigned int w = (unsigned int)(s >> 6);  // the wave's number; 32-bit tile arithmetic (64-bit divisions are the kernel's cost otherwise)
    unsigned int column, tz;                        // the wave's tile: column of the x/y plane, z
    if (kZRuns) {  // wave (w & 3) of the workgroup
      column = (w >> 2) % snxy; tz = ((w >> 2) / snxy) * 4 + (w & 3);
      if (tz >= (unsigned int)snz) continue;
    } else {
      column = w % snxy; tz = w / snxy;
    }
    const unsigned int tx = column % (unsigned int)snx, ty = column / (unsigned int)snx;
    const size_t c = ((size_t)(column + tz * snxy) << 6) | (s & 63);
    const int x = (int)(tx << 2) | (int)(c & 3), y = (int)(ty << 2) | (int)((c >> 2) & 3), z = (int)(tz << 2) | (int)((c >> 4) & 3);
    unsigned char v = default_index;
    if (x < nx && y < ny && z < nz) {
      float ux, uy, uz;
      if (FRAME == 0) {
        field.load((size_t)x + (size_t)y * nx + (size_t)z * nx * ny, ux, uy, uz);
        const float sx = nearest_sample((float)x + ux, nx), sy = nearest_sample((float)y + uy, ny), sz = nearest_sample((float)z + uz, nz);
        if (sx >= 0.f && sx <= (float)(nx - 1) && sy >= 0.f && sy <= (float)(ny - 1) && sz >= 0.f && sz <= (float)(nz - 1))
          v = base[tiled_voxel((unsigned int)(int)sx, (unsigned int)(int)sy, (unsigned int)(int)sz, (unsigned int)snx, snxy)];
      } else {
        const int g0 = ny, g1 = nx, g2 = nz;  // extents of the geometry arrays
        const int gx = ny - 1 - y, gy = x, gz = z;
        field.load(((size_t)gx * g1 + gy) * g2 + gz, ux, uy, uz);
        const float sx = nearest_sample((float)gx + ux, g0), sy = nearest_sample((float)gy + uy, g1), sz = nearest_sample((float)gz + uz, g2);
        if (sx >= 0.f && sx <= (float)(g0 - 1) && sy >= 0.f && sy <= (float)(g1 - 1) && sz >= 0.f && sz <= (float)(g2 - 1))
          v = base[tiled_voxel((unsigned int)(int)sy, (unsigned int)(ny - 1 - (int)sx), (unsigned int)(int)sz, (unsigned int)snx, snxy)];
      }
    }
    out[c] = v;
  }
}

// blocks of 256 threads for `nslot` slots of the kernel above (grid-stride beyond 16384 blocks); 0: more than 2^32 tiles, which the
// kernel's 32-bit tile arithmetic does not address (a volume of 256 GB)
inline unsigned warp_index_blocks(size_t nslot) {
  if ((nslot >> 6) >> 32) return 0;
  return (unsigned)((nslot + 255) / 256 < 256u * 64u ? (nslot + 255) / 256 : 256u * 64u);
}

}  // namespace mcgpu
