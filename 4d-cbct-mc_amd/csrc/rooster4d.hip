// rooster4d.hip -- 4-D ROOSTER reconstruction for MI355X (what the reference obtains from RTK's `rtkfourdrooster`,
// cbctmc/reconstruction/reconstruction.py: reconstruct_4d).  Geometry model as fdk.hip / forward_project.hip
// (rotation axis Y, source at Ry(gantry) (0, 0, sid), u = sdd x'/(sid - z') - proj_offset_x).  Restated in float64 by
// tests/rooster_ref.py.  Parity against rtkfourdrooster itself is unpinned: RTK is absent here.
//
// Unknowns: N frames x_f, f = 0..N-1, each on the FDK grid [nz][ny][nx] (IEC frame); projections p_k are line integrals after the
// optional water pre-correction (the polynomial sum_j c_j p^j of rtkfdk --wpc, backproject_column.inc: wpc_polynomial).
//   S   (phase -> interpolation weights, host: interpolation_weights): phi_k in [0, 1], t = phi_k N, l = floor(t) mod N,
//       h = (l + 1) mod N, w_h = t - floor(t), w_l = 1 - w_h.  S blends frames l and h for projection k, S^T distributes into them.
//   R   Joseph forward projection (joseph_ray.inc: float64 ray setup, tap positions and sums, float32 samples), reading the blend
//       w_l x_l + w_h x_h at every tap (SrcBlend).
//   B   voxel-driven bilinear back-projection with backproject_column.inc's detector sample (it counts only with both columns
//       and both rows inside the detector), without ramp filter or angular-gap weights, with the weight (sdd / U)^2 sx sy sz / (du dv),
//       U = sid - z_rot.  That weight makes B ~ R^T (the Joseph sum over the rays through a voxel, per unit of detector area at the
//       voxel's magnification), so the CG operator below is close to symmetric -- a deliberate departure from RTK's unweighted
//       CudaVoxelBased back-projector, whose operator S^T B R S is not symmetric and which CG only tolerates.
//   main iteration (niter times, from x = 0):
//     1. cgiter conjugate-gradient steps on A = S^T B R S, b = S^T B p, restarted from the current x (r = b - A x, direction = r)
//     2. positivity x = max(x, 0) (rtkfourdrooster without --nopositivity)
//     3. spatial TV denoising of every frame, 4. temporal TV denoising of every voxel's N-sample series (periodic)
//   TV denoising, min 1/2 |u - f|^2 + gamma TV(u), tviter iterations of the dual projected gradient (RTK's BPDQ family):
//     p = 0; repeat { u = f + div p; p <- Pi_gamma(p + tau grad u) }; u = f + div p.  grad = forward differences in index units,
//     Neumann in space (the last difference of an axis is 0), periodic in time; div = -grad^T exactly; Pi_gamma scales each
//     voxel's gradient vector to Euclidean norm <= gamma (3 spatial components together); tau = 1 / (4 d), d = 3 space, 1 time.
//   Dot products in float64, reduced in two fixed stages (a fixed grid of partial sums, then one block) without atomics: a run is
//   bit-reproducible.
// Kernels: fp4_kernel (R S, one lane per detector pixel as forward_project.hip), bp4_kernel (S^T B over a batch of projections
// that share their frame pair: two accumulators per voxel, frames l and h written once per batch), the CG vector kernels with
// float4 loads and the dot-product stages, positivity, tv_space_div / tv_space_grad (per frame: the spatial dual is 3 x one
// frame) and tv_time_kernel (a voxel's whole series and its dual in registers: one read and one write of the 4-D volume).
// Residency: the projection stack and the 4-D vectors x, b, r, d, A d stay on the device for the whole run.
//
// Motion-aware ROOSTER (mcgpu_rooster4d_reconstruct_motion; Mory, Janssens, Rit, PMB 2016; what RTK's
// `rtkfourdrooster --dvf --idvf` is for).  Two linear motion models live on the reconstruction grid; their layout and the
// displacement d of a voxel for a state's delta are motion_model.inc's.
//   to_reference   (forward model): the material of reference-phase voxel P is at P + F(P; s) at state s.
//   from_reference (pull-back model): frame_s(Q) = ref(Q + G(Q; s)).
// Frame f has a state s_f that enters as delta_to[f][k] = s_f[k] - mean_signal_to[k] and delta_from[f][k] likewise.  What is this
// file's own is where P + d goes, the sampling operator Sigma(model, delta) of a volume v at the voxel P = (ix, iy, iz):
//   position      per axis fx = fmaf(d_x, 1 / sx, (float)ix), clamped: fminf(fmaxf(fx, 0), nx - 1) -- the border is replicated and
//                 every index is in bounds for any float input, NaN and Inf included;
//   cell          i0 = (int)floorf(fx), t = fx - i0, i1 = min(i0 + 1, nx - 1);
//   value         trilinear with nested lerp(a, b, t) = fmaf(t, b - a, a) along x, then y, then z: a zero displacement returns
//                 the voxel bit for bit.
// (W x)_f = Sigma(to_reference, delta_to[f]) x_f carries every frame to the reference phase, (U c)_f = Sigma(from_reference,
// delta_from[f]) c_f carries it back.  Steps 1 - 3 are unchanged; step 4 becomes, with TVtime the temporal TV above,
//     y = W x;  c = TVtime(y) - y;  x = x + U c
// so only the regulariser's correction is resampled, never x itself: with gamma_time = 0 or tviter = 0 x is left untouched, and a
// displacement that is no whole number of voxels does not blur x.  A deliberate departure from RTK, which replaces x by
// U TVtime(W x) and so resamples the volume twice per main iteration.  Nothing here derives one model from the other, and a
// swapped pair is not detected.  Kernels: warp4_kernel (one thread per voxel, x fastest; it loads its model once
// and loops over the frames, whose deltas are wave-uniform kernel arguments; 8 gathers per frame; it stores W x twice, as y and as
// the input of TVtime, or adds U c to x) and subtract_kernel.  y and c are the CG vectors A d and r, free at step 4: no new 4-D
// allocation, peak memory grows by the two resident models, 2 x 3 (K + 1) frames.  Restated in float64 by tests/rooster_motion_ref.py.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/mcgpu_amd.h"
#include "hip_host.hpp"
#include "backproject_column.inc"
#include "joseph_ray.inc"

namespace {

#include "motion_model.inc"

using mcgpu::CallDevice;
using mcgpu::Stage;
using mcgpu::refuse;

#include "fixed_sum.inc"

constexpr int kFpBatch = 16;     // projections per forward launch (blockIdx.z)
constexpr int kBpBatch = kBatch; // projections per back-projection launch (backproject_column.inc's measured optimum)
constexpr int kMaxFrames = 32;   // frames of the temporal TV kernel's register arrays
constexpr int kRedBlocks = 1024; // blocks of the first reduction stage (fixed: the summation order does not depend on the device)
constexpr int kThreads = 256;

// ---- R S -----------------------------------------------------------------------------------------------------------------
struct Fp4Args : FpVolume {
  int nb;
  FpProj pp[kFpBatch];
  int fl[kFpBatch], fh[kFpBatch];  // frame pair of each projection
  float wl[kFpBatch], wh[kFpBatch];
};

struct SrcBlend {  // w_l x_l + w_h x_h at IEC index (x, y, z)
  const float* a;
  const float* b;
  float wa, wb;
  int nx, nxy;
  __device__ float operator()(int x, int y, int z, const float*) const {
    const size_t i = (size_t)z * nxy + (size_t)y * nx + x;
    return wa * a[i] + wb * b[i];
  }
};

__global__ __launch_bounds__(256) void fp4_kernel(float* __restrict__ out /*[nb][nv][nu]*/, const Fp4Args A, const float* __restrict__ x4, size_t frame) {
  int iu, iv;
  if (!fp_pixel(A, iu, iv)) return;
  const int k = blockIdx.z;
  const SrcBlend src{x4 + (size_t)A.fl[k] * frame, x4 + (size_t)A.fh[k] * frame, A.wl[k], A.wh[k], A.n[0], A.n[0] * A.n[1]};
  out[((size_t)k * A.nv + iv) * A.nu + iu] = joseph_ray(A, A.pp[k], iu, iv, src, nullptr);
}

// ---- S^T B -----------------------------------------------------------------------------------------------------------------
struct Bp4Args {
  int nx, ny, nz, nu, nv, nb;
  int fl, fh;                // the frame pair all projections of the batch share
  double x0, z0, sx, sz;     // column position (float64: computed once per column and projection)
  float y0, sy;
  double sid, sdd, inv_du, inv_dv, u0, v0;
  double K;                  // sx sy sz / (du dv)
  double c[kBpBatch], s[kBpBatch], off_x[kBpBatch];
  float av_b[kBpBatch];      // fv = mag / dv Y + av_b (wave-uniform: scalar registers)
  float wl[kBpBatch], wh[kBpBatch];
};

// a thread owns one (x, z) column and walks y (backproject_column.inc; the setup in double is this kernel's own); x4 += S^T B q for the batch
__global__ __launch_bounds__(256, 4) void bp4_kernel(float* __restrict__ x4, size_t frame, const float* __restrict__ q /*[nb][nv][nu]*/, const Bp4Args A) {
  const int ix = blockIdx.x * blockDim.x + threadIdx.x, iz = blockIdx.y;
  if (ix >= A.nx) return;
  const double X = A.x0 + A.sx * ix, Z = A.z0 + A.sz * iz;
  int iu[kBpBatch];
  float au[kBpBatch], g[kBpBatch], av_a[kBpBatch];
#pragma unroll
  for (int k = 0; k < kBpBatch; ++k) {
    iu[k] = -1; au[k] = 0.f; g[k] = 0.f; av_a[k] = 0.f;
    if (k < A.nb) {
      const double xr = X * A.c[k] - Z * A.s[k], zr = X * A.s[k] + Z * A.c[k];
      const double U = A.sid - zr;
      if (U > 0.0) {
        const double mag = A.sdd / U;
        const double fu = (mag * xr - A.off_x[k] - A.u0) * A.inv_du;
        const double fl = floor(fu);
        if (fl >= 0.0 && fl < A.nu - 1) {
          iu[k] = (int)fl;
          au[k] = (float)(fu - fl);
          g[k] = (float)(mag * mag * A.K);
          av_a[k] = (float)(mag * A.inv_dv);  // fv = av_a Y + av_b
        }
      }
    }
  }
  const size_t plane = (size_t)A.nu * A.nv;
  const size_t col = (size_t)iz * A.ny * A.nx + ix;
  float* out_l = x4 + (size_t)A.fl * frame + col;
  float* out_h = x4 + (size_t)A.fh * frame + col;
  for (int iy = 0; iy < A.ny; ++iy) {
    const float Y = A.y0 + A.sy * iy;
    float acc_l = 0.f, acc_h = 0.f;
#pragma unroll
    for (int k = 0; k < kBpBatch; ++k) {
      int iv;
      float av;
      if (iu[k] >= 0 && detector_rows(fmaf(av_a[k], Y, A.av_b[k]), A.nv, iv, av)) {
        const float gv = g[k] * detector_sample(q + (size_t)k * plane + (size_t)iv * A.nu + iu[k], A.nu, au[k], av);
        acc_l = fmaf(A.wl[k], gv, acc_l);
        acc_h = fmaf(A.wh[k], gv, acc_h);
      }
    }
    const size_t o = (size_t)iy * A.nx;
    out_l[o] += acc_l;
    out_h[o] += acc_h;  // frame l == h (N = 1): the same thread adds both, in order
  }
}

// ---- vectors: n4 float4 groups (every 4-D vector is allocated and zero-padded to a multiple of 4 floats) --------------------
__device__ inline double dot4(float4 a, float4 b) {
  return (double)a.x * b.x + (double)a.y * b.y + (double)a.z * b.z + (double)a.w * b.w;
}

// part[block] = sum of a . b over the block's grid-stride share
__global__ __launch_bounds__(256) void dot_partial_kernel(const float4* __restrict__ a, const float4* __restrict__ b, size_t n4, double* __restrict__ part) {
  double acc = 0.0;
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n4; i += (size_t)kRedBlocks * kThreads) acc += dot4(a[i], b[i]);
  const double s = block_tree(acc);  // fixed_sum.inc: thread 0 gets the total
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// out = sum of the kRedBlocks partials (second stage, one block)
__global__ __launch_bounds__(256) void sum_partials_kernel(const double* __restrict__ part, double* __restrict__ out) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < kRedBlocks; i += kThreads) acc += part[i];
  const double s = block_tree(acc);  // fixed_sum.inc: thread 0 gets the total
  if (threadIdx.x == 0) *out = s;
}

// r = b - Ad; d = r; partial r . r
__global__ __launch_bounds__(256) void cg_restart_kernel(const float4* __restrict__ b, const float4* __restrict__ Ax, float4* __restrict__ r, float4* __restrict__ d,
                                                         size_t n4, double* __restrict__ part) {
  double acc = 0.0;
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n4; i += (size_t)kRedBlocks * kThreads) {
    const float4 bb = b[i], aa = Ax[i];
    const float4 v = make_float4(bb.x - aa.x, bb.y - aa.y, bb.z - aa.z, bb.w - aa.w);
    r[i] = v;
    d[i] = v;
    acc += dot4(v, v);
  }
  const double s = block_tree(acc);  // fixed_sum.inc: thread 0 gets the total
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// x += alpha d; r -= alpha Ad; partial r . r
__global__ __launch_bounds__(256) void cg_update_kernel(float4* __restrict__ x, float4* __restrict__ r, const float4* __restrict__ d, const float4* __restrict__ Ad,
                                                        float alpha, size_t n4, double* __restrict__ part) {
  double acc = 0.0;
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n4; i += (size_t)kRedBlocks * kThreads) {
    float4 xv = x[i], rv = r[i];
    const float4 dv = d[i], av = Ad[i];
    xv.x = fmaf(alpha, dv.x, xv.x); xv.y = fmaf(alpha, dv.y, xv.y); xv.z = fmaf(alpha, dv.z, xv.z); xv.w = fmaf(alpha, dv.w, xv.w);
    rv.x = fmaf(-alpha, av.x, rv.x); rv.y = fmaf(-alpha, av.y, rv.y); rv.z = fmaf(-alpha, av.z, rv.z); rv.w = fmaf(-alpha, av.w, rv.w);
    x[i] = xv;
    r[i] = rv;
    acc += dot4(rv, rv);
  }
  const double s = block_tree(acc);  // fixed_sum.inc: thread 0 gets the total
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// d = r + beta d
__global__ __launch_bounds__(256) void cg_direction_kernel(const float4* __restrict__ r, float4* __restrict__ d, float beta, size_t n4) {
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n4; i += (size_t)kRedBlocks * kThreads) {
    const float4 rv = r[i];
    float4 dv = d[i];
    dv.x = fmaf(beta, dv.x, rv.x); dv.y = fmaf(beta, dv.y, rv.y); dv.z = fmaf(beta, dv.z, rv.z); dv.w = fmaf(beta, dv.w, rv.w);
    d[i] = dv;
  }
}

__global__ __launch_bounds__(256) void positivity_kernel(float4* __restrict__ x, size_t n4) {
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n4; i += (size_t)kRedBlocks * kThreads) {
    float4 v = x[i];
    v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
    x[i] = v;
  }
}

// rtkfdk --wpc on the resident projections: p <- sum_j c_j p^j
__global__ __launch_bounds__(256) void wpc_kernel(float* __restrict__ p, size_t n, const float* __restrict__ wpc, int n_wpc) {
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)kRedBlocks * kThreads) {
    p[i] = wpc_polynomial(wpc, n_wpc, p[i]);
  }
}

// ---- spatial TV of one frame ------------------------------------------------------------------------------------------------
// u = f + div p, div p (i) = p(i) [i < n - 1] - p(i - 1) [i >= 1] per axis (= -grad^T p).  u may be f (the final step, in place).
__global__ __launch_bounds__(256) void tv_space_div_kernel(const float* f, const float* __restrict__ px, const float* __restrict__ py, const float* __restrict__ pz,
                                                           float* u, int nx, int ny, int nz) {
  const size_t nxy = (size_t)nx * ny, nvox = nxy * nz;
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < nvox; i += (size_t)gridDim.x * kThreads) {
    const int x = (int)(i % nx), y = (int)((i / nx) % ny), z = (int)(i / nxy);
    float d = 0.f;
    if (x < nx - 1) d += px[i];
    if (x > 0) d -= px[i - 1];
    if (y < ny - 1) d += py[i];
    if (y > 0) d -= py[i - nx];
    if (z < nz - 1) d += pz[i];
    if (z > 0) d -= pz[i - nxy];
    u[i] = f[i] + d;
  }
}

// p <- Pi_gamma(p + tau grad u): the 3-vector scaled to norm <= gamma
__global__ __launch_bounds__(256) void tv_space_grad_kernel(const float* __restrict__ u, float* __restrict__ px, float* __restrict__ py, float* __restrict__ pz,
                                                            int nx, int ny, int nz, float tau, float gamma) {
  const size_t nxy = (size_t)nx * ny, nvox = nxy * nz;
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < nvox; i += (size_t)gridDim.x * kThreads) {
    const int x = (int)(i % nx), y = (int)((i / nx) % ny), z = (int)(i / nxy);
    const float c = u[i];
    const float gx = x < nx - 1 ? u[i + 1] - c : 0.f, gy = y < ny - 1 ? u[i + nx] - c : 0.f, gz = z < nz - 1 ? u[i + nxy] - c : 0.f;
    float qx = fmaf(tau, gx, px[i]), qy = fmaf(tau, gy, py[i]), qz = fmaf(tau, gz, pz[i]);
    const float nrm = sqrtf(qx * qx + qy * qy + qz * qz);
    if (nrm > gamma) {
      const float s = gamma / nrm;
      qx *= s; qy *= s; qz *= s;
    }
    px[i] = qx; py[i] = qy; pz[i] = qz;
  }
}

// ---- temporal TV: a voxel's N-sample series and its dual in registers (indices are compile-time: no scratch) --------------------
template <int NM>
__global__ __launch_bounds__(256) void tv_time_kernel(float* __restrict__ x4, size_t frame, int N, int iters, float tau, float gamma) {
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= frame) return;
  float f[NM], p[NM], u[NM];
#pragma unroll
  for (int t = 0; t < NM; ++t) { f[t] = t < N ? x4[(size_t)t * frame + i] : 0.f; p[t] = 0.f; }
  for (int it = 0; it <= iters; ++it) {
    float plast = 0.f;  // p(N - 1): the periodic predecessor of t = 0
#pragma unroll
    for (int t = 0; t < NM; ++t) if (t == N - 1) plast = p[t];
#pragma unroll
    for (int t = 0; t < NM; ++t) u[t] = f[t] + (p[t] - (t == 0 ? plast : p[t > 0 ? t - 1 : 0]));  // u = f + div p
    if (it == iters) break;
    const float u0 = u[0];
#pragma unroll
    for (int t = 0; t < NM; ++t) {
      if (t < N) {
        const float next = (t == N - 1) ? u0 : u[t + 1 < NM ? t + 1 : 0];
        const float q = fmaf(tau, next - u[t], p[t]);
        p[t] = fminf(fmaxf(q, -gamma), gamma);  // |q| <= gamma
      }
    }
  }
#pragma unroll
  for (int t = 0; t < NM; ++t) if (t < N) x4[(size_t)t * frame + i] = u[t];
}

// ---- motion-aware temporal step (the rule stands in this file's header) -------------------------------------
struct WarpArgs {
  int nx, ny, nz, N;
  float inv_sx, inv_sy, inv_sz;
  float delta[kMaxFrames][kMotionMaxK];  // [f][k], k < K: wave-uniform, read through scalar loads
};

// index position along one axis -> cell (i0, i1) and weight t.  The float clamp alone keeps every index in bounds for any input
// (fmaxf and fminf return the operand that is not NaN); the integer clamp states the same bound again where the addresses are formed.
__device__ inline void warp_cell(float d, float inv_s, int i, int n, int& i0, int& i1, float& t) {
  const float f = fminf(fmaxf(fmaf(d, inv_s, (float)i), 0.f), (float)(n - 1));
  const float fl = floorf(f);
  i0 = min(max((int)fl, 0), n - 1);
  t = f - fl;
  i1 = min(i0 + 1, n - 1);
}

__device__ inline float lerp(float a, float b, float t) { return fmaf(t, b - a, a); }

// dst_f(P) = [dst_f(P) +] Sigma(model, delta[f]) src_f (P) for every frame f; dst2 (optional, store mode) gets the same values.
// One thread per voxel, x fastest: the model loads and the stores coalesce, neighbouring lanes gather neighbouring voxels.  A voxel
// has one owner: no atomics.  src must not overlap dst or dst2.
template <int K, bool ACCUMULATE>
__global__ __launch_bounds__(256) void warp4_kernel(float* __restrict__ dst, float* __restrict__ dst2, const float* __restrict__ src, size_t frame,
                                                    const float* __restrict__ mean, const float* __restrict__ coef, const WarpArgs A) {
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= frame) return;
  int ix, iy, iz;
  voxel_index(i, A.nx, A.ny, ix, iy, iz);
  MotionVoxel<K> model;
  model.load(mean, coef, frame, i);
  const size_t nx = (size_t)A.nx, nxy = nx * A.ny;
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
  for (int f = 0; f < A.N; ++f) {
    float dx, dy, dz;
    model.displacement(A.delta[f], dx, dy, dz);
    int x0, x1, y0, y1, z0, z1;
    float tx, ty, tz;
    warp_cell(dx, A.inv_sx, ix, A.nx, x0, x1, tx);
    warp_cell(dy, A.inv_sy, iy, A.ny, y0, y1, ty);
    warp_cell(dz, A.inv_sz, iz, A.nz, z0, z1, tz);
    const float* s = src + (size_t)f * frame;
    const size_t r00 = z0 * nxy + y0 * nx, r01 = z0 * nxy + y1 * nx, r10 = z1 * nxy + y0 * nx, r11 = z1 * nxy + y1 * nx;
    const float a00 = lerp(s[r00 + x0], s[r00 + x1], tx), a01 = lerp(s[r01 + x0], s[r01 + x1], tx);
    const float a10 = lerp(s[r10 + x0], s[r10 + x1], tx), a11 = lerp(s[r11 + x0], s[r11 + x1], tx);
    const float v = lerp(lerp(a00, a01, ty), lerp(a10, a11, ty), tz);
    const size_t o = (size_t)f * frame + i;
    if (ACCUMULATE) {
      dst[o] += v;
    } else {
      dst[o] = v;
      if (dst2) dst2[o] = v;
    }
  }
}

// a -= b
__global__ __launch_bounds__(256) void subtract_kernel(float4* __restrict__ a, const float4* __restrict__ b, size_t n4) {
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n4; i += (size_t)kRedBlocks * kThreads) {
    float4 v = a[i];
    const float4 w = b[i];
    v.x -= w.x; v.y -= w.y; v.z -= w.z; v.w -= w.w;
    a[i] = v;
  }
}

// ---- host --------------------------------------------------------------------------------------------------------------------
// RTK's signal-to-weights rule for a periodic N-frame sequence: phase phi in [0, 1] lies between frames l = floor(phi N) mod N and
// h = l + 1 mod N with linear weights; phi = 1 is frame 0 again.  This is the rule as RTK documents it (rtkfourdrooster --signal,
// rtk::PhasesToInterpolationWeights); its exact match with RTK's code cannot be checked here (RTK is absent).
void interpolation_weights(double phase, int N, int& l, int& h, double& wl, double& wh) {
  const double t = phase * N, ft = std::floor(t);
  l = (int)(((long long)ft % N + N) % N);
  h = (l + 1) % N;
  wh = t - ft;
  wl = 1.0 - wh;
}


void read_options(const char* fn, const mcgpu_rooster4d_options* caller, mcgpu_rooster4d_options& o) {
  mcgpu::read_options(fn, "mcgpu_rooster4d_options", caller, o);
  if (o.n_proj < 1 || o.nu < 2 || o.nv < 2 || !o.gantry_deg || !(o.du > 0) || !(o.dv > 0) || !(o.sid > 0) || !(o.sdd > 0))
    refuse(fn, "bad geometry argument");
  if (o.nx < 1 || o.ny < 1 || o.nz < 1 || !(o.sx > 0) || !(o.sy > 0) || !(o.sz > 0)) refuse(fn, "bad volume argument");
  if (o.n_frames < 1 || o.n_frames > kMaxFrames) refuse(fn, "n_frames must be 1.." + std::to_string(kMaxFrames));
  if (!o.phase) refuse(fn, "phase is NULL");
  for (int k = 0; k < o.n_proj; ++k)
    if (!(o.phase[k] >= 0.0 && o.phase[k] <= 1.0)) refuse(fn, "phase[" + std::to_string(k) + "] is not in [0, 1]");
  if (o.niter < 0 || o.cgiter < 0 || o.tviter < 0) refuse(fn, "niter, cgiter and tviter must be >= 0");
  if (!(o.gamma_space >= 0.0) || !(o.gamma_time >= 0.0) || !std::isfinite(o.gamma_space) || !std::isfinite(o.gamma_time))
    refuse(fn, "gamma_space and gamma_time must be finite and >= 0");
  if (o.n_wpc < 0 || (o.n_wpc > 0 && !o.wpc)) refuse(fn, "bad wpc argument");
}

struct Problem {
  mcgpu_rooster4d_options o;
  int N;
  size_t frame, n4d, n4, plane;         // voxels per frame, 4-D floats, float4 groups (padded), pixels per projection
  std::vector<int> fl, fh;
  std::vector<double> wl, wh;
  Fp4Args fa;                           // per-launch fields filled in forward()
  std::vector<Bp4Args> bp;              // one per back-projection batch, with the first projection of each
  std::vector<int> bp_first;
  mcgpu_rooster4d_report rep;
  CallDevice dev;
  double* d_part = nullptr;
  double* d_sum = nullptr;
  // the two motion models of mcgpu_rooster4d_reconstruct_motion, resident for the call; motion_K == 0: plain ROOSTER, which launches
  // exactly what it launched without these members
  struct Warp {
    DeviceMotionModel model;
    WarpArgs args;  // grid, 1 / spacing and the frames' deltas (rounded once to float32)
  };
  int motion_K = 0;
  Warp to, from;  // W and U
  double ms_warp = 0.0, ms_upload_model = 0.0;

  explicit Problem(const mcgpu_rooster4d_options& opt) : o(opt), N(opt.n_frames) {
    memset(&rep, 0, sizeof rep);
    frame = (size_t)o.nx * o.ny * o.nz;
    n4d = frame * N;
    n4 = (n4d + 3) / 4;
    plane = (size_t)o.nu * o.nv;
    fl.resize(o.n_proj); fh.resize(o.n_proj); wl.resize(o.n_proj); wh.resize(o.n_proj);
    for (int k = 0; k < o.n_proj; ++k) interpolation_weights(o.phase[k], N, fl[k], fh[k], wl[k], wh[k]);
    const double sp[3] = {o.sx, o.sy, o.sz};
    const int n[3] = {o.nx, o.ny, o.nz};
    fa = Fp4Args{fp_volume(o, n, sp)};
    // back-projection batches: consecutive projections with the same frame pair, at most kBpBatch
    for (int k = 0; k < o.n_proj;) {
      Bp4Args A;
      memset(&A, 0, sizeof A);
      A.nx = o.nx; A.ny = o.ny; A.nz = o.nz; A.nu = o.nu; A.nv = o.nv;
      A.fl = fl[k]; A.fh = fh[k];
      A.x0 = fa.o[0]; A.z0 = fa.o[2]; A.sx = o.sx; A.sz = o.sz; A.y0 = (float)fa.o[1]; A.sy = (float)o.sy;
      A.sid = o.sid; A.sdd = o.sdd; A.inv_du = 1.0 / o.du; A.inv_dv = 1.0 / o.dv; A.u0 = o.u0; A.v0 = o.v0;
      A.K = o.sx * o.sy * o.sz / (o.du * o.dv);
      int m = 0;
      while (k + m < o.n_proj && m < kBpBatch && fl[k + m] == A.fl && fh[k + m] == A.fh) {
        const int p = k + m;
        const mcgpu::ProjectionPose q = mcgpu::projection_pose(o, p);
        A.c[m] = q.c; A.s[m] = q.s;
        A.off_x[m] = q.off_x;
        A.av_b[m] = (float)((-q.off_y - o.v0) / o.dv);
        A.wl[m] = (float)wl[p]; A.wh[m] = (float)wh[p];
        ++m;
      }
      A.nb = m;
      bp.push_back(A);
      bp_first.push_back(k);
      k += m;
    }
  }

  void init() {
    HIP_TRY(hipSetDevice(o.device));
    dev.events();
    d_part = dev.alloc_zeroed<double>(kRedBlocks * sizeof(double));
    d_sum = dev.alloc_zeroed<double>(sizeof(double));
  }
  float* alloc4d() { return dev.alloc_zeroed<float>(n4 * 16); }
  float* alloc_proj() { return dev.alloc_zeroed<float>((size_t)o.n_proj * plane * 4); }

  // proj = R S x4
  void forward(const float* x4, float* proj) {
    Stage st(dev, rep.ms_forward);
    Fp4Args A = fa;
    for (int b = 0; b < o.n_proj; b += kFpBatch) {
      A.nb = std::min(kFpBatch, o.n_proj - b);
      fp_poses(o, b, A.nb, A.pp);
      for (int k = 0; k < A.nb; ++k) {
        const int p = b + k;
        A.fl[k] = fl[p]; A.fh[k] = fh[p]; A.wl[k] = (float)wl[p]; A.wh[k] = (float)wh[p];
      }
      hipLaunchKernelGGL(fp4_kernel, fp_grid(o.nu, o.nv, A.nb), dim3(256), 0, nullptr, proj + (size_t)b * plane, A, x4, frame);
    }
    st.done();
  }

  // x4 = S^T B proj
  void back(const float* proj, float* x4) {
    Stage st(dev, rep.ms_back);
    HIP_TRY(hipMemsetAsync(x4, 0, n4 * 16, nullptr));
    for (size_t i = 0; i < bp.size(); ++i)
      hipLaunchKernelGGL(bp4_kernel, dim3((unsigned)((o.nx + 255) / 256), (unsigned)o.nz), dim3(256), 0, nullptr, x4, frame,
                         proj + (size_t)bp_first[i] * plane, bp[i]);
    st.done();
  }

  double reduce() {  // second stage of a dot product whose partials are in d_part
    hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(kThreads), 0, nullptr, d_part, d_sum);
    double s = 0.0;
    HIP_TRY(hipMemcpy(&s, d_sum, sizeof s, hipMemcpyDeviceToHost));
    return s;
  }

  double dot(const float* a, const float* b) {
    Stage st(dev, rep.ms_cg_vectors);
    hipLaunchKernelGGL(dot_partial_kernel, dim3(kRedBlocks), dim3(kThreads), 0, nullptr, (const float4*)a, (const float4*)b, n4, d_part);
    const double s = reduce();
    st.done();
    return s;
  }

  void tv_space(float* x4, float* work /*4 frames*/, int iters, float gamma) {
    Stage st(dev, rep.ms_tv_space);
    float *px = work, *py = work + frame, *pz = work + 2 * frame, *u = work + 3 * frame;
    const float tau = 1.f / 12.f;
    const unsigned g = (unsigned)std::min<size_t>((frame + kThreads - 1) / kThreads, 65536);
    for (int f = 0; f < N; ++f) {
      float* x = x4 + (size_t)f * frame;
      HIP_TRY(hipMemsetAsync(work, 0, 3 * frame * 4, nullptr));
      for (int it = 0; it < iters; ++it) {
        hipLaunchKernelGGL(tv_space_div_kernel, dim3(g), dim3(kThreads), 0, nullptr, x, px, py, pz, u, o.nx, o.ny, o.nz);
        hipLaunchKernelGGL(tv_space_grad_kernel, dim3(g), dim3(kThreads), 0, nullptr, u, px, py, pz, o.nx, o.ny, o.nz, tau, gamma);
      }
      hipLaunchKernelGGL(tv_space_div_kernel, dim3(g), dim3(kThreads), 0, nullptr, x, px, py, pz, x, o.nx, o.ny, o.nz);
    }
    st.done();
  }

  void tv_time(float* x4, int iters, float gamma) {
    Stage st(dev, rep.ms_tv_time);
    const dim3 g((unsigned)((frame + kThreads - 1) / kThreads));
    if (N <= 16) hipLaunchKernelGGL(tv_time_kernel<16>, g, dim3(kThreads), 0, nullptr, x4, frame, N, iters, 0.25f, gamma);
    else hipLaunchKernelGGL(tv_time_kernel<kMaxFrames>, g, dim3(kThreads), 0, nullptr, x4, frame, N, iters, 0.25f, gamma);
    st.done();
  }

  // both models onto the device once, as float32; the deltas rounded once to float32
  void upload_model(const mcgpu_rooster4d_motion& M) {
    const mcgpu::Stopwatch sw;
    motion_K = M.n_signal_dims;
    to.model = upload_motion_model(dev, M.to_reference_mean, M.to_reference_coefficients, motion_K, frame);
    from.model = upload_motion_model(dev, M.from_reference_mean, M.from_reference_coefficients, motion_K, frame);
    memset(&to.args, 0, sizeof to.args);
    to.args.nx = o.nx; to.args.ny = o.ny; to.args.nz = o.nz; to.args.N = N;
    to.args.inv_sx = (float)(1.0 / o.sx); to.args.inv_sy = (float)(1.0 / o.sy); to.args.inv_sz = (float)(1.0 / o.sz);
    from.args = to.args;
    memcpy(to.args.delta, round_deltas(M.delta_to, N, motion_K).data(), N * sizeof to.args.delta[0]);
    memcpy(from.args.delta, round_deltas(M.delta_from, N, motion_K).data(), N * sizeof from.args.delta[0]);
    ms_upload_model += sw.ms();
  }

  // dst = W src (to_reference) or U src (from reference); accumulate: dst += ...; dst2: a second copy of a stored result, or null
  void warp(bool to_reference, bool accumulate, float* dst, float* dst2, const float* src) {
    const Warp& w = to_reference ? to : from;
    const dim3 g((unsigned)((frame + kThreads - 1) / kThreads));
    dispatch_motion_k(motion_K, [&](auto k) {
      constexpr int K = decltype(k)::value;
      if (accumulate) hipLaunchKernelGGL((warp4_kernel<K, true>), g, dim3(kThreads), 0, nullptr, dst, dst2, src, frame, w.model.mean, w.model.coef, w.args);
      else hipLaunchKernelGGL((warp4_kernel<K, false>), g, dim3(kThreads), 0, nullptr, dst, dst2, src, frame, w.model.mean, w.model.coef, w.args);
    });
  }

  // step 4 along the model's trajectories: y = W x; c = TVtime(y) - y; x += U c.  y and c are two 4-D vectors the caller lends
  // (the CG vectors A d and r, both rewritten at the next restart).  gamma = 0 or no iterations: c = 0, x is left untouched.
  void tv_time_motion(float* x4, float* y, float* c, int iters, float gamma) {
    if (iters <= 0 || !(gamma > 0.f)) return;
    {
      Stage st(dev, ms_warp);
      warp(true, false, y, c, x4);
      st.done();
    }
    tv_time(c, iters, gamma);
    Stage st(dev, ms_warp);
    hipLaunchKernelGGL(subtract_kernel, dim3(kRedBlocks), dim3(kThreads), 0, nullptr, (float4*)c, (const float4*)y, n4);
    warp(false, true, x4, nullptr, c);
    st.done();
  }

  float* upload_projections(const float* projections, bool wpc) {
    const mcgpu::Stopwatch upload;
    float* d = alloc_proj();
    HIP_TRY(hipMemcpy(d, projections, (size_t)o.n_proj * plane * 4, hipMemcpyHostToDevice));
    if (wpc && o.n_wpc > 0) {
      std::vector<float> c(o.wpc, o.wpc + o.n_wpc);
      float* d_c = dev.alloc_zeroed<float>(c.size() * 4);
      HIP_TRY(hipMemcpy(d_c, c.data(), c.size() * 4, hipMemcpyHostToDevice));
      hipLaunchKernelGGL(wpc_kernel, dim3(kRedBlocks), dim3(kThreads), 0, nullptr, d, (size_t)o.n_proj * plane, d_c, o.n_wpc);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipDeviceSynchronize());
    }
    rep.ms_upload += upload.ms();
    return d;
  }

  float* upload_4d(const float* v) {
    const mcgpu::Stopwatch upload;
    float* d = alloc4d();
    HIP_TRY(hipMemcpy(d, v, n4d * 4, hipMemcpyHostToDevice));
    rep.ms_upload += upload.ms();
    return d;
  }

  void run(const float* projections, float* volume4d) {
    float* q = upload_projections(projections, true);     // measured projections; after b they hold R S d
    float* x = alloc4d();
    float* b = alloc4d();
    float* r = alloc4d();
    float* d = alloc4d();
    float* Ad = alloc4d();
    float* work = dev.alloc_zeroed<float>(4 * frame * 4);
    back(q, b);
    const unsigned g = kRedBlocks;
    bool x_zero = true;
    for (int it = 0; it < o.niter; ++it) {
      double* res = o.residuals ? o.residuals + (size_t)it * (o.cgiter + 1) : nullptr;
      if (x_zero) {
        HIP_TRY(hipMemsetAsync(Ad, 0, n4 * 16, nullptr));  // A 0 = 0
      } else {
        forward(x, q);
        back(q, Ad);
      }
      double rr;
      {
        Stage st(dev, rep.ms_cg_vectors);
        hipLaunchKernelGGL(cg_restart_kernel, dim3(g), dim3(kThreads), 0, nullptr, (const float4*)b, (const float4*)Ad, (float4*)r, (float4*)d, n4, d_part);
        rr = reduce();
        st.done();
      }
      if (res) res[0] = std::sqrt(rr);
      for (int j = 0; j < o.cgiter; ++j) {
        double alpha = 0.0, rr_new = rr;
        if (rr > 0.0) {
          forward(d, q);
          back(q, Ad);
          const double dAd = dot(d, Ad);
          if (dAd > 0.0) {
            alpha = rr / dAd;
            Stage st(dev, rep.ms_cg_vectors);
            hipLaunchKernelGGL(cg_update_kernel, dim3(g), dim3(kThreads), 0, nullptr, (float4*)x, (float4*)r, (const float4*)d, (const float4*)Ad, (float)alpha,
                               n4, d_part);
            rr_new = reduce();
            const double beta = rr > 0.0 ? rr_new / rr : 0.0;
            hipLaunchKernelGGL(cg_direction_kernel, dim3(g), dim3(kThreads), 0, nullptr, (const float4*)r, (float4*)d, (float)beta, n4);
            st.done();
            x_zero = false;
          }
        }
        rr = rr_new;
        if (res) res[j + 1] = std::sqrt(rr);
      }
      if (o.positivity) {
        Stage st(dev, rep.ms_cg_vectors);
        hipLaunchKernelGGL(positivity_kernel, dim3(g), dim3(kThreads), 0, nullptr, (float4*)x, n4);
        st.done();
      }
      if (o.tviter > 0) {
        tv_space(x, work, o.tviter, (float)o.gamma_space);
        if (motion_K) tv_time_motion(x, Ad, r, o.tviter, (float)o.gamma_time);
        else tv_time(x, o.tviter, (float)o.gamma_time);
      }
    }
    HIP_TRY(hipMemcpy(volume4d, x, n4d * 4, hipMemcpyDeviceToHost));
  }

  void stage(int which, const float* in, float* out) {
    if (which == MCGPU_ROOSTER4D_STAGE_FORWARD) {
      float* x = upload_4d(in);
      float* q = alloc_proj();
      forward(x, q);
      HIP_TRY(hipMemcpy(out, q, (size_t)o.n_proj * plane * 4, hipMemcpyDeviceToHost));
      return;
    }
    if (which == MCGPU_ROOSTER4D_STAGE_BACK) {
      float* q = upload_projections(in, false);
      float* x = alloc4d();
      back(q, x);
      HIP_TRY(hipMemcpy(out, x, n4d * 4, hipMemcpyDeviceToHost));
      return;
    }
    float* x = upload_4d(in);
    if (which == MCGPU_ROOSTER4D_STAGE_TV_SPACE) {
      float* work = dev.alloc_zeroed<float>(4 * frame * 4);
      tv_space(x, work, o.tviter, (float)o.gamma_space);
    } else {
      tv_time(x, o.tviter, (float)o.gamma_time);
    }
    HIP_TRY(hipMemcpy(out, x, n4d * 4, hipMemcpyDeviceToHost));
  }

  void motion_stage(int which, const float* in, float* out) {
    float* x = upload_4d(in);
    float* y = alloc4d();
    if (which == MCGPU_ROOSTER4D_MOTION_STAGE_TV_TIME_MOTION) {
      float* c = alloc4d();
      tv_time_motion(x, y, c, o.tviter, (float)o.gamma_time);
      HIP_TRY(hipMemcpy(out, x, n4d * 4, hipMemcpyDeviceToHost));
      return;
    }
    Stage st(dev, ms_warp);
    warp(which == MCGPU_ROOSTER4D_MOTION_STAGE_WARP, false, y, nullptr, x);
    st.done();
    HIP_TRY(hipMemcpy(out, y, n4d * 4, hipMemcpyDeviceToHost));
  }

  // the report of a call that took ms_total on the host, plain or with the two motion fields
  void write(double ms_total, mcgpu_rooster4d_report* out) {
    rep.peak_device_bytes = dev.peak;
    rep.ms_total = ms_total;
    *out = rep;
  }
  void write(double ms_total, mcgpu_rooster4d_motion_report* out) const {
    *out = {rep.ms_forward, rep.ms_back, rep.ms_cg_vectors, rep.ms_tv_space, rep.ms_tv_time, rep.ms_upload, ms_total,
            (unsigned long long)dev.peak, ms_warp, ms_upload_model};
  }
};

// the checks of a mcgpu_rooster4d_motion that need no device: refused with -1 before any HIP call
void read_motion(const char* fn, const mcgpu_rooster4d_motion* caller, int n_frames, mcgpu_rooster4d_motion& m) {
  mcgpu::read_options(fn, "mcgpu_rooster4d_motion", caller, m);
  check_motion_k(fn, m.n_signal_dims);
  if (!m.to_reference_mean || !m.to_reference_coefficients || !m.from_reference_mean || !m.from_reference_coefficients)
    refuse(fn, "a motion model array is NULL");
  if (!m.delta_to || !m.delta_from) refuse(fn, "delta_to or delta_from is NULL");
  check_delta(fn, m.delta_to, (size_t)n_frames * m.n_signal_dims);
  check_delta(fn, m.delta_from, (size_t)n_frames * m.n_signal_dims);
}

void check_stage(const char* fn, int stage, int first, int last, const float* in, const float* out) {
  if (stage < first || stage > last) refuse(fn, "unknown stage " + std::to_string(stage));
  if (!in || !out) refuse(fn, "in or out is NULL");
}

// What the four entry points share: the options (and, with_motion, the motion struct) read and checked, the entry point's own
// argument checks, then the host clock, Problem, init, the models, the body and the report.  Nothing before Problem touches HIP.
template <class Report, class Check, class Body>
int entry(const char* fn, const mcgpu_rooster4d_options* caller_o, bool with_motion, const mcgpu_rooster4d_motion* caller_m, Report* report, Check check, Body body) {
  ABI_BEGIN
  mcgpu_rooster4d_options o;
  read_options(fn, caller_o, o);
  mcgpu_rooster4d_motion m = {};
  if (with_motion) read_motion(fn, caller_m, o.n_frames, m);
  check();
  const mcgpu::Stopwatch call;
  Problem P(o);
  P.init();
  if (with_motion) P.upload_model(m);
  body(P);
  if (report) P.write(call.ms(), report);
  return 0;
  ABI_END
}

}  // namespace

extern "C" int mcgpu_rooster4d_reconstruct(const mcgpu_rooster4d_options* o, const float* projections, float* volume4d, mcgpu_rooster4d_report* report) {
  const char* fn = "mcgpu_rooster4d_reconstruct";
  return entry(fn, o, false, nullptr, report, [&] { if (!projections || !volume4d) refuse(fn, "projections or volume is NULL"); },
               [&](Problem& P) { P.run(projections, volume4d); });
}

extern "C" int mcgpu_rooster4d_stage(const mcgpu_rooster4d_options* o, int stage, const float* in, float* out, mcgpu_rooster4d_report* report) {
  const char* fn = "mcgpu_rooster4d_stage";
  return entry(fn, o, false, nullptr, report, [&] { check_stage(fn, stage, MCGPU_ROOSTER4D_STAGE_FORWARD, MCGPU_ROOSTER4D_STAGE_TV_TIME, in, out); },
               [&](Problem& P) { P.stage(stage, in, out); });
}

extern "C" int mcgpu_rooster4d_reconstruct_motion(const mcgpu_rooster4d_options* o, const mcgpu_rooster4d_motion* m, const float* projections, float* volume4d,
                                                  mcgpu_rooster4d_motion_report* report) {
  const char* fn = "mcgpu_rooster4d_reconstruct_motion";
  return entry(fn, o, true, m, report, [&] { if (!projections || !volume4d) refuse(fn, "projections or volume is NULL"); },
               [&](Problem& P) { P.run(projections, volume4d); });
}

extern "C" int mcgpu_rooster4d_motion_stage(const mcgpu_rooster4d_options* o, const mcgpu_rooster4d_motion* m, int stage, const float* in, float* out,
                                            mcgpu_rooster4d_motion_report* report) {
  const char* fn = "mcgpu_rooster4d_motion_stage";
  return entry(fn, o, true, m, report, [&] { check_stage(fn, stage, MCGPU_ROOSTER4D_MOTION_STAGE_WARP, MCGPU_ROOSTER4D_MOTION_STAGE_TV_TIME_MOTION, in, out); },
               [&](Problem& P) { P.motion_stage(stage, in, out); });
}
