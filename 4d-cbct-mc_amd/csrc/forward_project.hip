// forward_project.hip -- ray-driven Joseph forward projection on a circular cone-beam geometry for MI355X (what the reference obtains
// from RTK's JosephForwardProjectionImageFilter, cbctmc/forward_projection.py: project_forward).  Geometry model as fdk.hip
// (rotation axis Y, source at Ry(gantry) (0, 0, sid), u = sdd x'/(sid - z') - proj_offset_x); the scheme as RTK documents it,
// restated in float64 by tests/joseph_ref.py (parity against RTK's own border handling is unpinned: RTK is absent here):
//   - one lane per detector pixel; a wave covers an 8x8 pixel tile, a workgroup 2x2 tiles, the grid one batch of projections
//     (per-projection constants in the kernarg block: wave-uniform scalar loads)
//   - per ray (float64, once): clip the segment source -> pixel to the volume box, which spans half a voxel beyond the outer voxel
//     centres; main axis = the largest component of the ray direction in index coordinates (ties: x before y before z)
//   - samples where the ray crosses the voxel-centre planes k = ns..fs of the main axis; each is a bilinear interpolation in the
//     other two axes with explicit float32 weights, taps outside the volume read 0; the first and last steps are weighted by the
//     fraction of a step the clipped segment covers, and the sum is scaled by the length in mm of one main-axis step
//   - tap positions and the sum over the planes in float64, the samples in float32, the result rounded once to float32 (RTK's
//     float pixel type): with both in float32 the 512^3 Catphan volume missed the restatement's tolerance fourfold (joseph_ray.inc)
// The traversal runs in the index frame of the IEC volume [nz][ny][nx]; only the voxel fetch differs between volume sources
// (template parameter): a float volume uploaded from the host, or the context's own representation (u8 tiled / u16 palette
// indices with the palette densities in LDS, raw {density, material} float2), read in the .vox frame.  All sources run the same
// arithmetic, so the same densities give bit-identical sums.  The per-ray body, the volume arguments and the pixel tile live in
// joseph_ray.inc, shared with rooster4d.hip.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "engine_internal.hpp"
#include "joseph_ray.inc"

namespace {

using namespace mcgpu;

constexpr int kBatch = 16;       // projections per launch (blockIdx.z)
constexpr int kChunk = 64;       // projections resident in the device output buffer (downloaded per chunk)
constexpr int kPalLds = 8192;    // palette densities staged in LDS up to this many entries (32 KB)

struct FpArgs : FpVolume {
  int nb;
  FpProj pp[kBatch];
};

// ---- voxel sources: density at IEC index (x, y, z), all inside the volume ------------------------------------------------
struct SrcFloat {
  static constexpr bool kPalette = false;
  static constexpr int kLdsN = 1;
  const float* v;
  int nx, nxy;
  __device__ float operator()(int x, int y, int z, const float*) const { return v[(size_t)z * nxy + (size_t)y * nx + x]; }
};

// The context's volume is stored in the .vox frame (geometry.py: mcgpu_arrays, rot90(k=3) of the MCGeometry arrays); with the IEC
// mapping of prepare_image_for_rtk (IEC X = MC x, Y = -MC z, Z = -MC y) an IEC voxel (x, y, z) is vox voxel
// (vnx - 1 - z, vny - 1 - x, vnz - 1 - y), where (vnx, vny, vnz) = (NZ, NX, NY).
struct VoxFrame {
  int vnx, vny, vnz;
  __device__ void map(int x, int y, int z, unsigned& vx, unsigned& vy, unsigned& vz) const {
    vx = (unsigned)(vnx - 1 - z); vy = (unsigned)(vny - 1 - x); vz = (unsigned)(vnz - 1 - y);
  }
};

struct SrcU8 {  // tiled palette indices (device_model.hpp: tiled_voxel), palette densities in LDS
  static constexpr bool kPalette = true;
  static constexpr int kLdsN = 256;
  const unsigned char* v;
  VoxFrame f;
  unsigned sub_nx, sub_nxy;
  __device__ float operator()(int x, int y, int z, const float* pal) const {
    unsigned vx, vy, vz;
    f.map(x, y, z, vx, vy, vz);
    return pal[v[tiled_voxel(vx, vy, vz, sub_nx, sub_nxy)]];
  }
};

template <bool kLds>
struct SrcU16 {  // x-fastest palette indices; densities in LDS when the palette fits, else read from the float2 palette
  static constexpr bool kPalette = kLds;
  static constexpr int kLdsN = kLds ? kPalLds : 1;
  const unsigned short* v;
  const float* pal2;
  VoxFrame f;
  __device__ float operator()(int x, int y, int z, const float* pal) const {
    unsigned vx, vy, vz;
    f.map(x, y, z, vx, vy, vz);
    const unsigned i = v[((size_t)vz * f.vny + vy) * f.vnx + vx];
    return kLds ? pal[i] : pal2[2 * (size_t)i];
  }
};

struct SrcRaw {  // {density, material} per voxel, x fastest
  static constexpr bool kPalette = false;
  static constexpr int kLdsN = 1;
  const float2* v;
  VoxFrame f;
  __device__ float operator()(int x, int y, int z, const float*) const {
    unsigned vx, vy, vz;
    f.map(x, y, z, vx, vy, vz);
    return v[((size_t)vz * f.vny + vy) * f.vnx + vx].x;
  }
};

template <class Src>
__global__ __launch_bounds__(256) void joseph_fp_kernel(float* __restrict__ out /*[nb][nv][nu]*/, const FpArgs A, const Src src,
                                                        const float* __restrict__ pal2, int pal_n) {
  __shared__ float pal[Src::kLdsN];
  if constexpr (Src::kPalette) {
    for (int i = threadIdx.x; i < pal_n; i += blockDim.x) pal[i] = pal2[2 * i];
    __syncthreads();
  }
  int iu, iv;
  if (!fp_pixel(A, iu, iv)) return;
  const float acc = joseph_ray(A, A.pp[blockIdx.z], iu, iv, src, pal);
  out[((size_t)blockIdx.z * A.nv + iv) * A.nu + iu] = acc;
}

void read_fp_options(const char* fn, const mcgpu_fp_options* caller, mcgpu_fp_options& o) {
  read_options(fn, "mcgpu_fp_options", caller, o);
  if (o.n_proj < 1 || o.nu < 1 || o.nv < 1 || !o.gantry_deg || !(o.du > 0) || !(o.dv > 0) || !(o.sid > 0) || !(o.sdd > 0))
    throw Error(-1, std::string("!!ERROR!! ") + fn + ": bad argument");
}

// all projections through one source; projections [n_proj][nv][nu] on the host
template <class Src>
void project_all(CallDevice& dev, const mcgpu_fp_options& o, const FpVolume& V, const Src& src, const float* pal2, int pal_n, float* projections, double& ms_kernel) {
  const size_t plane = (size_t)o.nu * o.nv;
  const int chunk = std::min(o.n_proj, kChunk);
  float* d_out = dev.alloc<float>((size_t)chunk * plane * 4);
  dev.events();
  FpArgs A{V};  // the per-projection block is filled per launch
  for (int first = 0; first < o.n_proj; first += chunk) {
    const int m = std::min(chunk, o.n_proj - first);
    Stage st(dev, ms_kernel);
    for (int b = 0; b < m; b += kBatch) {
      A.nb = std::min(kBatch, m - b);
      fp_poses(o, first + b, A.nb, A.pp);
      hipLaunchKernelGGL(joseph_fp_kernel<Src>, fp_grid(o.nu, o.nv, A.nb), dim3(256), 0, nullptr, d_out + (size_t)b * plane, A, src, pal2, pal_n);
    }
    st.done();
    HIP_TRY(hipMemcpy(projections + (size_t)first * plane, d_out, (size_t)m * plane * 4, hipMemcpyDeviceToHost));
  }
}

}  // namespace

extern "C" int mcgpu_forward_project(const mcgpu_fp_options* caller_o, const float* volume, float* projections, mcgpu_fp_report* report) {
  ABI_BEGIN
  mcgpu_fp_options o;
  read_fp_options("mcgpu_forward_project", caller_o, o);
  if (!volume || !projections || o.nx < 1 || o.ny < 1 || o.nz < 1 || !(o.sx > 0) || !(o.sy > 0) || !(o.sz > 0))
    throw Error(-1, "!!ERROR!! mcgpu_forward_project: bad volume argument");
  HIP_TRY(hipSetDevice(o.device));
  CallDevice dev;
  const size_t nvox = (size_t)o.nx * o.ny * o.nz;
  const Stopwatch clock;
  const float* d_vol = dev.upload(volume, nvox);
  const double ms_upload = clock.ms();
  const int n[3] = {o.nx, o.ny, o.nz};
  const double sp[3] = {o.sx, o.sy, o.sz};
  SrcFloat src{d_vol, o.nx, o.nx * o.ny};
  double ms_kernel = 0.0;
  project_all(dev, o, fp_volume(o, n, sp), src, nullptr, 0, projections, ms_kernel);
  if (report) { report->ms_kernel = ms_kernel; report->ms_upload = ms_upload; }
  return 0;
  ABI_END
}

extern "C" int mcgpu_forward_project_context(mcgpu_ctx* ctx, const mcgpu_fp_options* caller_o, float* projections, mcgpu_fp_report* report) {
  ABI_BEGIN
  mcgpu_fp_options o;
  read_fp_options("mcgpu_forward_project_context", caller_o, o);
  require(ctx && ctx->has_device && projections, -1, "!!ERROR!! mcgpu_forward_project_context: bad argument (the context needs a device)");
  const HostModel& H = ctx->host;
  const DeviceModel& D = ctx->dev;
  const int vn[3] = {H.voxels.n[0], H.voxels.n[1], H.voxels.n[2]};
  const int n[3] = {vn[1], vn[2], vn[0]};  // IEC (X, Y, Z) = (vox y, vox z, vox x), each reversed
  if ((o.nx || o.ny || o.nz) && (o.nx != n[0] || o.ny != n[1] || o.nz != n[2])) {
    throw Error(-1, "!!ERROR!! mcgpu_forward_project_context: volume size " + std::to_string(o.nx) + "x" + std::to_string(o.ny) + "x" +
                        std::to_string(o.nz) + " is not the context's IEC size " + std::to_string(n[0]) + "x" + std::to_string(n[1]) + "x" +
                        std::to_string(n[2]));
  }
  // spacing: the caller's (mm, IEC order) when given, else the context's voxel size (cm)
  const double sp[3] = {o.sx > 0 ? o.sx : 10.0 * H.voxels.voxel_size[1], o.sy > 0 ? o.sy : 10.0 * H.voxels.voxel_size[2],
                        o.sz > 0 ? o.sz : 10.0 * H.voxels.voxel_size[0]};
  HIP_TRY(hipSetDevice(D.device_id));
  CallDevice dev;
  const FpVolume A = fp_volume(o, n, sp);
  const VoxFrame f{vn[0], vn[1], vn[2]};
  double ms_kernel = 0.0;
  if (D.vol_kind == kVolU8) {
    SrcU8 src{(const unsigned char*)D.vol, f, (unsigned)((vn[0] + 3) >> 2), (unsigned)(((vn[0] + 3) >> 2) * ((vn[1] + 3) >> 2))};
    project_all(dev, o, A, src, D.palette, D.palette_size, projections, ms_kernel);
  } else if (D.vol_kind == kVolU16 && D.palette_size <= kPalLds) {
    SrcU16<true> src{(const unsigned short*)D.vol, D.palette, f};
    project_all(dev, o, A, src, D.palette, D.palette_size, projections, ms_kernel);
  } else if (D.vol_kind == kVolU16) {
    SrcU16<false> src{(const unsigned short*)D.vol, D.palette, f};
    project_all(dev, o, A, src, D.palette, D.palette_size, projections, ms_kernel);
  } else {
    SrcRaw src{(const float2*)D.vol, f};
    project_all(dev, o, A, src, nullptr, 0, projections, ms_kernel);
  }
  if (report) { report->ms_kernel = ms_kernel; report->ms_upload = 0.0; }
  return 0;
  ABI_END
}
