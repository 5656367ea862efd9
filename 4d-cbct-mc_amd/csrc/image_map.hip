// image_map.hip -- a CT image and its tissue segmentations -> the class of every voxel, on the device (row f8).
//
// The reference maps on the host: nine boolean-mask passes over the volume and a scipy binary_erosion (cbctmc/mc/geometry.py:35-234,
// driven by MaterialMapperPipeline.execute, :237-309), after which the engine's host route quantises, palettises, tiles and classifies
// the (material, density) arrays once more.  The mapping (image_map.hpp states the rule) is a function of one image value, eight
// segmentation bits and the bone bit of the six face neighbours, so it is ONE streaming pass here:
//   map_tiled_kernel   reads image + segmentations once, in the inputs' own memory order, and writes the class of every voxel into the
//                      4x4x4-tiled u8 volume of the engine's frame.  A workgroup takes a block of whole tiles: it classifies the block's
//                      voxels with its lanes running along the inputs' fastest axis (x in frame 0, gz = z in frame 1: 64 consecutive
//                      elements per wave and load), parks the classes in LDS at their tiled positions, and after a barrier writes the
//                      tiles out with 16-byte vector stores, consecutive tiles side by side.  That LDS stage is the whole index
//                      permutation of frame 1 (engine voxel (x, y, z) = input voxel (ny - 1 - y, x, z)): neither side of it is strided.
//                      Blocks: frame 0 64 x 4 x 4 voxels (16 tiles along x, 1 KB), frame 1 16 x 4 x 64 (4 x 16 tiles, 4 KB).
//   map_plain_kernel   the mapping alone in the inputs' layout, (material, density) per voxel (mcgpu_map_image).
//   remap_kernel       class -> palette index, 16 bytes per lane (the palette's order is known only after the statistics).
// Bone halo: the six neighbours of the bone mask are loaded from memory, by the few voxels that need them (in the bone mask, at or above
// the bone_050 threshold); they lie in cache lines the workgroup or its neighbours stream anyway.
// Statistics (per class: count, smallest [z][y][x] index; unmapped voxels): a wave counts each class it holds with one ballot and one LDS
// atomic of the class's first lane; the minimum goes through LDS atomics that are issued only when they would lower it; a workgroup
// (persistent, grid-stride over blocks) flushes once, with vector atomics on 25 words.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "image_map.hpp"

namespace mcgpu {
namespace {

// Class of the voxel at element `lin` = (i2 n1 + i1) n0 + i0 of inputs laid out [n2][n1][n0].
template <typename T>
__device__ __forceinline__ unsigned char classify_voxel(const ImageMapArgs& a, unsigned int lin, int i0, int i1, int i2, int n0, int n1, int n2) {
  const float v = (float)reinterpret_cast<const T*>(a.image)[lin];
  unsigned char c = kImageUnmapped;
  bool body = false;
  if (a.seg[kSegBody]) {
    body = a.seg[kSegBody][lin] > 0;
    c = body ? (unsigned char)kClassSoftTissue : (unsigned char)kClassAir;
  }
  if (a.seg[kSegBone] && a.seg[kSegBone][lin] > 0) {
    const unsigned char* __restrict__ b = a.seg[kSegBone];
    if (v < a.threshold[0]) c = kClassRedMarrow;
    if (a.threshold[0] <= v && v < a.threshold[1]) c = kClassBone020;
    if (v >= a.threshold[1]) {
      bool inner = i0 > 0 && i0 < n0 - 1 && i1 > 0 && i1 < n1 - 1 && i2 > 0 && i2 < n2 - 1;  // a neighbour outside the volume is background
      if (inner) {
        const unsigned int s1 = (unsigned int)n0, s2 = (unsigned int)n0 * (unsigned int)n1;
        inner = b[lin - 1] > 0 && b[lin + 1] > 0 && b[lin - s1] > 0 && b[lin + s1] > 0 && b[lin - s2] > 0 && b[lin + s2] > 0;
      }
      c = inner ? (unsigned char)kClassBone050 : (unsigned char)kClassBone100;
    }
  }
  if (a.seg[kSegLung] && a.seg[kSegLung][lin] > 0) c = kClassLung;
  if (a.seg[kSegLiver] && a.seg[kSegLiver][lin] > 0) c = kClassLiver;
  if (a.seg[kSegStomach] && a.seg[kSegStomach][lin] > 0) c = kClassStomach;
  if (a.seg[kSegMuscle] && a.seg[kSegMuscle][lin] > 0) c = kClassMuscle;
  if (a.seg[kSegFat] && a.seg[kSegFat][lin] > 0) c = kClassAdipose;
  if (a.seg[kSegBody] && body && v < a.threshold[2]) c = kClassAir;
  if (a.seg[kSegVessels] && a.seg[kSegVessels][lin] > 0) c = kClassBlood;
  return c;
}

// s_cnt[13]: voxels per class, [12] unmapped; s_min[12]: smallest engine index per class.  Called by whole waves.
__device__ __forceinline__ void tally_classes(bool valid, unsigned char cls, unsigned int engine_lin, unsigned int* s_cnt, unsigned int* s_min) {
  const int lane = (int)(threadIdx.x & 63u);
  unsigned long long todo = __ballot(valid);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int c = __shfl((int)cls, leader);
    const unsigned long long same = __ballot(valid && (int)cls == c);
    if (lane == leader) atomicAdd(&s_cnt[c == kImageUnmapped ? kImageClasses : c], (unsigned int)__popcll(same));
    todo &= ~same;
  }
  if (valid && cls != kImageUnmapped && engine_lin < s_min[cls]) atomicMin(&s_min[cls], engine_lin);
}

__device__ __forceinline__ void stats_begin(unsigned int* s_cnt, unsigned int* s_min) {
  if (threadIdx.x <= (unsigned int)kImageClasses) s_cnt[threadIdx.x] = 0u;
  if (threadIdx.x < (unsigned int)kImageClasses) s_min[threadIdx.x] = 0xFFFFFFFFu;
  __syncthreads();
}

__device__ __forceinline__ void stats_flush(const ImageMapArgs& a, const unsigned int* s_cnt, const unsigned int* s_min) {
  __syncthreads();
  const unsigned int t = threadIdx.x;
  if (t <= (unsigned int)kImageClasses && s_cnt[t] != 0u) atomicAdd(&a.stats[t < (unsigned int)kImageClasses ? t : 2u * kImageClasses], s_cnt[t]);
  if (t < (unsigned int)kImageClasses && s_min[t] != 0xFFFFFFFFu) atomicMin(&a.stats[kImageClasses + t], s_min[t]);
}

template <int FRAME>
struct BlockShape {  // voxels of a workgroup's block, in the engine's frame
  static constexpr int kX = FRAME == 0 ? 64 : 16, kY = 4, kZ = FRAME == 0 ? 4 : 64;
  static constexpr int kTilesX = kX / 4, kTilesZ = kZ / 4, kTiles = kTilesX * kTilesZ, kVoxels = kX * kY * kZ;
};

template <int FRAME, typename T>
__global__ __launch_bounds__(256) void map_tiled_kernel(ImageMapArgs a, int nx, int ny, int nz, int snx, int sny, int snz, int nbx, int nby, int nbz,
                                                        unsigned char* __restrict__ out) {
  using B = BlockShape<FRAME>;
  __shared__ __attribute__((aligned(16))) unsigned char s_cls[B::kVoxels];
  __shared__ unsigned int s_cnt[kImageClasses + 1], s_min[kImageClasses];
  stats_begin(s_cnt, s_min);
  const unsigned int nblocks = (unsigned int)nbx * (unsigned int)nby * (unsigned int)nbz;
  for (unsigned int blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    const int bx = (int)(blk % (unsigned int)nbx), by = (int)((blk / (unsigned int)nbx) % (unsigned int)nby), bz = (int)(blk / ((unsigned int)nbx * (unsigned int)nby));
    for (int s = (int)threadIdx.x; s < B::kVoxels; s += 256) {
      int xl, yl, zl;
      if (FRAME == 0) { xl = s & 63; yl = (s >> 6) & 3; zl = s >> 8; }  // lanes along x
      else            { zl = s & 63; xl = (s >> 6) & 15; yl = s >> 10; }  // lanes along z = gz, the inputs' fastest axis
      const int x = bx * B::kX + xl, y = by * B::kY + yl, z = bz * B::kZ + zl;
      const bool valid = x < nx && y < ny && z < nz;
      unsigned char cls = 0;
      const unsigned int engine_lin = ((unsigned int)z * (unsigned int)ny + (unsigned int)y) * (unsigned int)nx + (unsigned int)x;
      if (valid) {
        if (FRAME == 0) {
          cls = classify_voxel<T>(a, engine_lin, x, y, z, nx, ny, nz);
        } else {
          const int gx = ny - 1 - y, gy = x, gz = z;  // inputs [gx][gy][gz], extents [ny][nx][nz]
          cls = classify_voxel<T>(a, ((unsigned int)gx * (unsigned int)nx + (unsigned int)gy) * (unsigned int)nz + (unsigned int)gz, gz, gy, gx, nz, nx, ny);
        }
      }
      s_cls[(((xl >> 2) + B::kTilesX * (zl >> 2)) << 6) | ((zl & 3) << 4) | ((yl & 3) << 2) | (xl & 3)] = cls;
      tally_classes(valid, cls, engine_lin, s_cnt, s_min);
    }
    __syncthreads();
    // the block's tiles, a quarter (one z layer, 16 bytes) per lane; tiles along x are neighbours in memory
    for (int q = (int)threadIdx.x; q < B::kTiles * 4; q += 256) {
      const int lt = q >> 2, dz = q & 3;
      const int tx = bx * B::kTilesX + lt % B::kTilesX, ty = by, tz = bz * B::kTilesZ + lt / B::kTilesX;
      if (tx >= snx || ty >= sny || tz >= snz) continue;
      uint4 w = *reinterpret_cast<const uint4*>(&s_cls[(lt << 6) | (dz << 4)]);
      const int x0 = tx << 2, y0 = ty << 2, z0 = tz << 2;
      if (x0 + 4 > nx || y0 + 4 > ny || z0 + 4 > nz) {  // an edge tile: its padding voxels repeat the tile's first voxel
        const unsigned int pad = s_cls[lt << 6];
        unsigned int word[4] = {w.x, w.y, w.z, w.w};
        for (int dy = 0; dy < 4; ++dy)
          for (int dx = 0; dx < 4; ++dx)
            if (x0 + dx >= nx || y0 + dy >= ny || z0 + dz >= nz) word[dy] = (word[dy] & ~(0xFFu << (8 * dx))) | (pad << (8 * dx));
        w = make_uint4(word[0], word[1], word[2], word[3]);
      }
      const size_t tile = (size_t)tx + (size_t)ty * (size_t)snx + (size_t)tz * (size_t)snx * (size_t)sny;
      *reinterpret_cast<uint4*>(out + (tile << 6) + ((size_t)dz << 4)) = w;
    }
    __syncthreads();  // the next block overwrites s_cls
  }
  stats_flush(a, s_cnt, s_min);
}

struct ClassTable {
  unsigned char material[16];
  float density[16];
};

template <typename T>
__global__ __launch_bounds__(256) void map_plain_kernel(ImageMapArgs a, int n0, int n1, int n2, ClassTable table, unsigned char* __restrict__ material_out,
                                                        float* __restrict__ density_out) {
  __shared__ unsigned int s_cnt[kImageClasses + 1], s_min[kImageClasses];
  __shared__ unsigned char s_mat[16];
  __shared__ float s_dens[16];
  if (threadIdx.x < 16) { s_mat[threadIdx.x] = table.material[threadIdx.x]; s_dens[threadIdx.x] = table.density[threadIdx.x]; }
  stats_begin(s_cnt, s_min);
  const unsigned int nvox = (unsigned int)n0 * (unsigned int)n1 * (unsigned int)n2;
  for (unsigned int base = blockIdx.x * 256u; base < nvox; base += gridDim.x * 256u) {  // whole waves stay in the loop (tally_classes)
    const unsigned int lin = base + threadIdx.x;
    const bool valid = lin < nvox;
    unsigned char cls = 0;
    if (valid) {
      const unsigned int row = lin / (unsigned int)n0;
      cls = classify_voxel<T>(a, lin, (int)(lin - row * (unsigned int)n0), (int)(row % (unsigned int)n1), (int)(row / (unsigned int)n1), n0, n1, n2);
      const int e = cls == kImageUnmapped ? kImageClasses : (int)cls;  // entry 12 of the table is (0, 0)
      material_out[lin] = s_mat[e];
      density_out[lin] = s_dens[e];
    }
    tally_classes(valid, cls, lin, s_cnt, s_min);
  }
  stats_flush(a, s_cnt, s_min);
}

struct Lut16 {
  unsigned char v[16];
};

__global__ __launch_bounds__(256) void remap_kernel(const uint4* __restrict__ in, uint4* __restrict__ out, size_t n16, Lut16 lut) {
  __shared__ unsigned char s_lut[16];
  if (threadIdx.x < 16) s_lut[threadIdx.x] = lut.v[threadIdx.x];
  __syncthreads();
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) {
    const uint4 w = in[i];
    const unsigned int word[4] = {w.x, w.y, w.z, w.w};
    unsigned int r[4];
    for (int k = 0; k < 4; ++k)
      r[k] = (unsigned int)s_lut[word[k] & 15u] | ((unsigned int)s_lut[(word[k] >> 8) & 15u] << 8) | ((unsigned int)s_lut[(word[k] >> 16) & 15u] << 16) |
             ((unsigned int)s_lut[(word[k] >> 24) & 15u] << 24);
    out[i] = make_uint4(r[0], r[1], r[2], r[3]);
  }
}

unsigned int persistent_grid(size_t work_items, int num_cus) {
  const size_t cap = (size_t)(num_cus > 0 ? num_cus : 256) * 8;
  return (unsigned int)(work_items < cap ? (work_items > 0 ? work_items : 1) : cap);
}

}  // namespace

hipError_t launch_image_map_tiled(const ImageMapArgs& a, int frame, int nx, int ny, int nz, unsigned char* classes_tiled, int num_cus, hipStream_t stream) {
  if (nx <= 0 || ny <= 0 || nz <= 0 || (frame != 0 && frame != 1) || (unsigned long long)nx * ny * nz >= (1ULL << 31)) return hipErrorInvalidValue;
  const int snx = (nx + 3) >> 2, sny = (ny + 3) >> 2, snz = (nz + 3) >> 2;
  const int kx = frame == 0 ? BlockShape<0>::kX : BlockShape<1>::kX, kz = frame == 0 ? BlockShape<0>::kZ : BlockShape<1>::kZ;
  const int nbx = (nx + kx - 1) / kx, nby = sny, nbz = (nz + kz - 1) / kz;
  const unsigned long long nblocks = (unsigned long long)nbx * nby * nbz;
  if (nblocks >= (1ULL << 32)) return hipErrorInvalidValue;
  const dim3 grid(persistent_grid((size_t)nblocks, num_cus)), block(256);
#define MCGPU_MAP_TILED(FRAME, T) hipLaunchKernelGGL((map_tiled_kernel<FRAME, T>), grid, block, 0, stream, a, nx, ny, nz, snx, sny, snz, nbx, nby, nbz, classes_tiled)
  if (frame == 0 && a.image_is_f32) MCGPU_MAP_TILED(0, float);
  else if (frame == 0) MCGPU_MAP_TILED(0, short);
  else if (a.image_is_f32) MCGPU_MAP_TILED(1, float);
  else MCGPU_MAP_TILED(1, short);
#undef MCGPU_MAP_TILED
  return hipGetLastError();
}

hipError_t launch_image_map_plain(const ImageMapArgs& a, int n0, int n1, int n2, const unsigned char material[kImageClasses], const float density[kImageClasses],
                                  unsigned char* material_out, float* density_out, int num_cus, hipStream_t stream) {
  if (n0 <= 0 || n1 <= 0 || n2 <= 0 || (unsigned long long)n0 * n1 * n2 >= (1ULL << 31)) return hipErrorInvalidValue;
  ClassTable t{};
  for (int c = 0; c < kImageClasses; ++c) { t.material[c] = material[c]; t.density[c] = density[c]; }
  const size_t nvox = (size_t)n0 * n1 * n2;
  const dim3 grid(persistent_grid((nvox + 255) / 256, num_cus)), block(256);
  if (a.image_is_f32) hipLaunchKernelGGL(map_plain_kernel<float>, grid, block, 0, stream, a, n0, n1, n2, t, material_out, density_out);
  else hipLaunchKernelGGL(map_plain_kernel<short>, grid, block, 0, stream, a, n0, n1, n2, t, material_out, density_out);
  return hipGetLastError();
}

hipError_t launch_image_remap(const unsigned char* in, unsigned char* out, size_t bytes, const unsigned char lut[16], hipStream_t stream) {
  if ((bytes & 15) != 0) return hipErrorInvalidValue;
  Lut16 l;
  for (int i = 0; i < 16; ++i) l.v[i] = lut[i];
  const size_t n16 = bytes >> 4;
  const size_t blocks = (n16 + 255) / 256;
  hipLaunchKernelGGL(remap_kernel, dim3((unsigned int)(blocks < 8192 ? (blocks ? blocks : 1) : 8192)), dim3(256), 0, stream, reinterpret_cast<const uint4*>(in),
                     reinterpret_cast<uint4*>(out), n16, l);
  return hipGetLastError();
}

}  // namespace mcgpu
