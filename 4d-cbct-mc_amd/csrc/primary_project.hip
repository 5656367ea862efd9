// primary_project.hip -- the ray-traced primary: the expectation of the engine's `unscattered` plane, computed as a ray integral
// (source spectrum x Beer-Lambert attenuation along the straight line focal spot -> pixel) through the piecewise-constant voxels the
// context holds on the device, with the cross-section tables the flight step reads; and the small separable Gaussian that smooths
// the Monte Carlo scatter beside it (mcgpu_smooth_planes).  Restated in float64 by tests/primary_ref.py.  Its noise -- the moment planes of
// the compound Poisson tally and a seeded draw from them, stated after the rule -- is restated by tests/primary_noise_ref.py.
//
// THE RULE, for projection p of a context (resident geometry, pose, detector, spectrum) and pixel (px, pz) of the tally image [nz][nx]:
//  1 sub-points   The pixel is split into su x sv equal cells (1..8 each).  The centre of cell (i, j) has detector coordinates
//                 xd = px + (i + 1/2) / su, zd = pz + (j + 1/2) / sv and is the world point Q = O + xd U + zd V [cm]: the exact inverse of
//                 tally_pixel (track_common.inc) -- a photon flying from the focal spot through Q scores in word px + pz nx.  The host
//                 forms O, U, V in double from the pose: rotation_flag 0: the plane y = center.y, x / z from corner_min and the pixel
//                 pitch; rotation_flag 1: the plane through `center` normal to the source direction, coordinates r = rot_inv P, solved
//                 for r.y and taken back with the matrix inverse of rot_inv.
//  2 aperture     The ray direction d = (Q - S) / |Q - S| is taken back to the beam frame (inverse of rot_fan; identity for rotation_flag
//                 0) and is inside the beam iff it passes the acceptance of sample_source_direction: dz between cos_theta_low and
//                 cos_theta_low + D_cos_theta (the host stores a negative D_cos_theta), phi = atan2(dy, dx) in [phi_low, phi_low +
//                 D_phi] (modulo 2 pi), |dz / dy| <= max_height_at_y1cm.  A ray outside contributes 0.  Omega is the solid angle of
//                 that accepted set, the integral of dphi dz over it: computed once per call on the host in double by Gauss-Legendre
//                 on the pieces between the kinks of the integrand (1e-12 and better).  FAST's fmed3 clamp of dx / dy moves
//                 directions that the native sine / cosine put ~1e-6 outside the fan back onto its edge: it moves no measurable
//                 mass, and neither does the 1e-7 in the kernels' |dz / (dy + 1e-7)|.
//  3 thickness    The voxel grid (planes at k * voxel_size, k = 0..n, per axis) is traversed exactly by an incremental DDA from the
//                 entry to the exit of the bounding box (slab method; a ray parallel to an axis must lie within the box on that axis; a
//                 ray that misses has t = 0).  Start voxel: floor(position / voxel_size) at the entry, clamped.  Each step crosses the
//                 nearest next plane, x before y before z on ties, so a crossing shared by two or three planes yields zero-length
//                 segments and the sum is continuous there: no ray is ambiguous.  Consecutive voxels with the same (density, material)
//                 form a run; at its end t_m += rho * (float)(t_end - t_start) [g/cm^2] for the run's material m.  Material and density
//                 are read as flight_locate / flight_resolve read them: palette entry (u8 tiled, u16) or the raw float2.
//                 Parametric crossings are double, the run length is rounded once to float32, the accumulators t_m are float32.
//  4 spectrum     The source draws bin b with probability P_b (from the alias tables of sample_source_energy) and an energy uniform in
//                 [e_b, e_b+1]: Qn-point Gauss-Legendre per bin (1..4, default 2), nodes E_q, weights W_q = P_b g_j E_q (sum g_j = 1).
//                 K[q][m] = a_tot + E_q b_tot of material m in the table bin floor((E_q - e0) ide): the exact-table route of
//                 flight_resolve.  The host builds W and K in double.  S = sum_q W_q exp(-sum_m K[q][m] t_m): the exponent is summed in
//                 double, exp taken in float32 of its leading float with the remainder as a first-order factor, the sum over q in double.
//  5 pixel value  mean over the su sv sub-points of S cos(psi) / (r^2 Omega), r = |Q - S|, psi between the ray and the detector normal,
//                 rounded once to float32: eV / cm^2 per history, the unit of the `unscattered` plane finalize makes of a tally.
//                 Output layout as finalize's: [nz][crop_nx], z flipped, half-fan crop.
// Kernel shape: one lane per pixel (sub-points in sequence), a wave covers an 8x8 pixel tile, a workgroup 16x16, blockIdx.z the
// projection.  A lane's t_m live in LDS as [m][lane] (a dynamically indexed private array would land in scratch: joseph_ray.inc), the
// current run in registers.  W, K and the per-projection block are read at wave-uniform addresses (scalar loads).
//
// MOMENT PLANES (mcgpu_primary_moments).  The engine's detector is an ideal energy absorber, so the tally of a pixel is a compound
// Poisson sum: a Poisson number of photons, each adding its energy.  For k = 0, 1, 2 the plane M_k is steps 1 - 5 with the weights
// W_q^(k) = P_b g_j E_q^k in step 4: photons / cm^2, eV / cm^2 and eV^2 / cm^2 per history.  M_1 is the plane above; primary_kernel<VK, 3>
// forms the three sums from one traversal, one exponent and one expf per sub-point and node (primary_kernel<VK, 1> is the kernel of
// mcgpu_primary_project, instruction for instruction what it was before the moments existed).  Layout [projection][k][nz][crop_nx].
// With a = the pixel area [cm^2] and N histories, N a M_0 is the expected number of photons in a pixel and M_2 / (N a) the variance
// of the `unscattered` plane, up to the relative term a M_0 (about 1e-6) that the Poisson limit of the binomial count drops.
//
// THE NOISE RULE (mcgpu_primary_noisy, mcgpu_sample_compound_poisson), per pixel (x, y) = (column, row) of the plane as laid out above,
// in double from the float32 planes:
//  inputs   lambda = N a M_0, mu = M_1 / M_0, s2 = max(M_2 / M_0 - mu^2, 0).  A pixel whose M_0 is not > 0 gives exactly 0.
//  draws    philox_normal.inc: key = seed, counter (x, y, first_projection + p, k).  Draw k = 0 gives u (= u1 of word 0) and z0 (the
//           normal of words 0 and 1); draw k = 1 gives z1; draw k = 2 gives z2.
//  count    lambda < 64: inversion by sequential search, p = exp(-lambda), F = p, n = 0; while u > F and n < 1024: n += 1,
//           p *= lambda / n, F += p.  lambda >= 64: n = max(0, floor(lambda + sqrt(lambda) z0 + (z0^2 - 1) / 6 + 1/2)), the normal with
//           its first skewness correction (Cornish-Fisher).
//  value    max(0, n mu + sqrt(n s2) z1) / (N a), rounded once to float32; n = 0 gives exactly 0.
// The mean of the rule is M_1 and its variance M_2 / (N a); shadows get true zeros and integer-count statistics.  What it is not: the
// energy sum given n is a Gaussian of the right mean and variance, not the exact n-fold mixture of the transmitted spectrum, and
// u and z0 share their words (a pixel uses one of the two).
// mcgpu_sample_gaussian: max(0, mean + sqrt(max(variance, 0)) z2), rounded once to float32.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "engine_internal.hpp"

namespace {

using namespace mcgpu;

constexpr int kChunk = 64;  // projections resident in the device output buffer (downloaded per chunk)
constexpr int kLanes = 256;

struct PrimaryProj {  // one projection, host double
  double src[3], o[3], u[3], v[3], nrm[3];
  double beam[9];  // world -> beam frame
  double z_lo, z_hi, phi_lo, d_phi, height;
  double inv_omega;
};

struct PrimaryVol {
  const void* vol;
  const float2* pal;
  int pal_n, n[3];
  double vs[3];
  unsigned int sub_nx, sub_nxy;
  int nx, nz, crop_nx, su, sv, nq, nmat;
};

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

template <int VK>
__device__ __forceinline__ unsigned long long voxel_key(const PrimaryVol& A, int ix, int iy, int iz) {
  if (VK == kVolU8) return ((const unsigned char*)A.vol)[tiled_voxel((unsigned)ix, (unsigned)iy, (unsigned)iz, A.sub_nx, A.sub_nxy)];
  const size_t vi = ((size_t)iz * A.n[1] + iy) * A.n[0] + ix;
  if (VK == kVolU16) return ((const unsigned short*)A.vol)[vi];
  const float2 pd = ((const float2*)A.vol)[vi];
  return ((unsigned long long)__float_as_uint(pd.y) << 32) | __float_as_uint(pd.x);
}

// end of a run of voxels that share `key`: t_m += rho * len
template <int VK>
__device__ __forceinline__ void close_run(const PrimaryVol& A, unsigned long long key, float len, const float2* pal_lds, float* t_lane) {
  float2 pd;
  if (VK == kVolU8) pd = pal_lds[key];
  else if (VK == kVolU16) pd = A.pal[key < (unsigned long long)A.pal_n ? key : 0ULL];
  else pd = make_float2(__uint_as_float((unsigned int)key), __uint_as_float((unsigned int)(key >> 32)));
  const int m = clampi(__float_as_int(pd.y), A.nmat - 1);
  t_lane[m * kLanes] = fmaf(pd.x, len, t_lane[m * kLanes]);
}

// NM = 1: the plane M_1 from W [nq].  NM = 3: the planes M_0, M_1, M_2 from W = [W^(1) | W^(0) | W^(2)], nq each.
template <int VK, int NM>
__global__ __launch_bounds__(kLanes) void primary_kernel(float* __restrict__ out /*[nb][NM][nz][crop_nx]*/, const PrimaryVol A,
                                                         const PrimaryProj* __restrict__ proj, const double* __restrict__ W,
                                                         const double* __restrict__ K) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  float* const t_lds = reinterpret_cast<float*>(lds);                              // [nmat][kLanes]
  float2* const pal_lds = reinterpret_cast<float2*>(lds + (size_t)A.nmat * kLanes * 4);  // [256], u8 volumes
  if (VK == kVolU8) {
    for (int i = threadIdx.x; i < A.pal_n; i += kLanes) pal_lds[i] = A.pal[i];
    __syncthreads();
  }
  const int wave = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int px = blockIdx.x * 16 + (wave & 1) * 8 + (l & 7), pz = blockIdx.y * 16 + (wave >> 1) * 8 + (l >> 3);
  if (px >= A.crop_nx || pz >= A.nz) return;
  const PrimaryProj& P = proj[blockIdx.z];
  float* const t_lane = t_lds + threadIdx.x;
  const double bx = A.n[0] * A.vs[0], by = A.n[1] * A.vs[1], bz = A.n[2] * A.vs[2];
  const int max_steps = A.n[0] + A.n[1] + A.n[2] + 4;
  double sum = 0.0, sum0 = 0.0, sum2 = 0.0;
  for (int sj = 0; sj < A.sv; ++sj) {
    for (int si = 0; si < A.su; ++si) {
      const double xd = (double)px + ((double)si + 0.5) / (double)A.su, zd = (double)pz + ((double)sj + 0.5) / (double)A.sv;
      const double qx = P.o[0] + xd * P.u[0] + zd * P.v[0] - P.src[0];
      const double qy = P.o[1] + xd * P.u[1] + zd * P.v[1] - P.src[1];
      const double qz = P.o[2] + xd * P.u[2] + zd * P.v[2] - P.src[2];
      const double r2 = qx * qx + qy * qy + qz * qz, inv_r = 1.0 / sqrt(r2);
      const double dx = qx * inv_r, dy = qy * inv_r, dz = qz * inv_r;
      // aperture, in the beam frame
      const double ux = P.beam[0] * dx + P.beam[1] * dy + P.beam[2] * dz;
      const double uy = P.beam[3] * dx + P.beam[4] * dy + P.beam[5] * dz;
      const double uz = P.beam[6] * dx + P.beam[7] * dy + P.beam[8] * dz;
      double phi = atan2(uy, ux) - P.phi_lo;
      phi -= 6.283185307179586 * floor(phi / 6.283185307179586);
      if (!(uz >= P.z_lo && uz <= P.z_hi && phi <= P.d_phi && fabs(uz) <= P.height * fabs(uy))) continue;
      const double cospsi = fabs(dx * P.nrm[0] + dy * P.nrm[1] + dz * P.nrm[2]);
      for (int m = 0; m < A.nmat; ++m) t_lane[m * kLanes] = 0.0f;
      // slab method: [tmin, tmax] of the bounding box
      double tmin = 0.0, tmax = 1.0e300;
      bool hit = true;
      double ivx = 0.0, ivy = 0.0, ivz = 0.0;
      if (dx != 0.0) { ivx = 1.0 / dx; const double a = (0.0 - P.src[0]) * ivx, b = (bx - P.src[0]) * ivx; tmin = fmax(tmin, fmin(a, b)); tmax = fmin(tmax, fmax(a, b)); }
      else hit = hit && P.src[0] >= 0.0 && P.src[0] <= bx;
      if (dy != 0.0) { ivy = 1.0 / dy; const double a = (0.0 - P.src[1]) * ivy, b = (by - P.src[1]) * ivy; tmin = fmax(tmin, fmin(a, b)); tmax = fmin(tmax, fmax(a, b)); }
      else hit = hit && P.src[1] >= 0.0 && P.src[1] <= by;
      if (dz != 0.0) { ivz = 1.0 / dz; const double a = (0.0 - P.src[2]) * ivz, b = (bz - P.src[2]) * ivz; tmin = fmax(tmin, fmin(a, b)); tmax = fmin(tmax, fmax(a, b)); }
      else hit = hit && P.src[2] >= 0.0 && P.src[2] <= bz;
      if (hit && tmax > tmin) {
        int ix = clampi((int)floor((P.src[0] + tmin * dx) / A.vs[0]), A.n[0] - 1);
        int iy = clampi((int)floor((P.src[1] + tmin * dy) / A.vs[1]), A.n[1] - 1);
        int iz = clampi((int)floor((P.src[2] + tmin * dz) / A.vs[2]), A.n[2] - 1);
        const int sx = dx > 0.0 ? 1 : -1, sy = dy > 0.0 ? 1 : -1, sz = dz > 0.0 ? 1 : -1;
        const int fx = dx > 0.0 ? 1 : 0, fy = dy > 0.0 ? 1 : 0, fz = dz > 0.0 ? 1 : 0;
        double tnx = dx != 0.0 ? ((double)(ix + fx) * A.vs[0] - P.src[0]) * ivx : 1.0e300;
        double tny = dy != 0.0 ? ((double)(iy + fy) * A.vs[1] - P.src[1]) * ivy : 1.0e300;
        double tnz = dz != 0.0 ? ((double)(iz + fz) * A.vs[2] - P.src[2]) * ivz : 1.0e300;
        double tc = tmin, ts = tmin;
        unsigned long long run = 0ULL;
        bool have = false;
        for (int it = 0; it < max_steps; ++it) {
          const unsigned long long key = voxel_key<VK>(A, ix, iy, iz);
          if (!have || key != run) {
            if (have) close_run<VK>(A, run, (float)(tc - ts), pal_lds, t_lane);
            run = key; ts = tc; have = true;
          }
          double tn;
          bool inside;
          if (tnx <= tny && tnx <= tnz) { tn = tnx; ix += sx; inside = ix >= 0 && ix < A.n[0]; tnx = ((double)(ix + fx) * A.vs[0] - P.src[0]) * ivx; }
          else if (tny <= tnz) { tn = tny; iy += sy; inside = iy >= 0 && iy < A.n[1]; tny = ((double)(iy + fy) * A.vs[1] - P.src[1]) * ivy; }
          else { tn = tnz; iz += sz; inside = iz >= 0 && iz < A.n[2]; tnz = ((double)(iz + fz) * A.vs[2] - P.src[2]) * ivz; }
          tc = fmax(tc, fmin(tn, tmax));
          if (!inside || !(tn < tmax)) break;
        }
        if (have) close_run<VK>(A, run, (float)(tc - ts), pal_lds, t_lane);
      }
      // spectrum
      double s = 0.0, s0 = 0.0, s2 = 0.0;
      for (int q = 0; q < A.nq; ++q) {
        double x = 0.0;
        for (int m = 0; m < A.nmat; ++m) x = fma(K[q * A.nmat + m], (double)t_lane[m * kLanes], x);
        const float xh = (float)x, xl = (float)(x - (double)xh);
        if (NM == 1) {
          s = fma(W[q], (double)(expf(-xh) * (1.0f - xl)), s);
        } else {
          const double e = (double)(expf(-xh) * (1.0f - xl));
          s = fma(W[q], e, s);
          s0 = fma(W[A.nq + q], e, s0);
          s2 = fma(W[2 * A.nq + q], e, s2);
        }
      }
      sum += s * cospsi / r2;
      if (NM == 3) {
        sum0 += s0 * cospsi / r2;
        sum2 += s2 * cospsi / r2;
      }
    }
  }
  const double value = sum / (double)(A.su * A.sv) * P.inv_omega;
  if (NM == 1) {
    out[((size_t)blockIdx.z * A.nz + (size_t)(A.nz - 1 - pz)) * A.crop_nx + px] = (float)value;
  } else {
    const size_t plane = (size_t)A.nz * A.crop_nx, at = (size_t)blockIdx.z * 3 * plane + (size_t)(A.nz - 1 - pz) * A.crop_nx + px;
    out[at] = (float)(sum0 / (double)(A.su * A.sv) * P.inv_omega);
    out[at + plane] = (float)value;
    out[at + 2 * plane] = (float)(sum2 / (double)(A.su * A.sv) * P.inv_omega);
  }
}

// ---- the samplers ---------------------------------------------------------------------------------------------------------------
#include "philox_normal.inc"

// one draw of the rule: words of counter (x, y, projection, k)
__device__ __forceinline__ double draw_normal(int x, int y, unsigned projection, unsigned k, unsigned long long seed, double& u) {
  unsigned w0, w1;
  philox10((unsigned)x, (unsigned)y, projection, k, (unsigned)seed, (unsigned)(seed >> 32), w0, w1);
  return normal_of_words(w0, w1, u);
}

// THE NOISE RULE of the header.  m0, m1, m2: planes [ny][nx] of plane blockIdx.y, `stride` floats from one plane to the next; na = N a
__global__ __launch_bounds__(256) void compound_poisson_kernel(const float* __restrict__ m0, const float* __restrict__ m1, const float* __restrict__ m2,
                                                               size_t stride, float* __restrict__ out, int nx, unsigned int hw, double na,
                                                               unsigned long long seed, unsigned first_projection) {
  const unsigned int i = blockIdx.x * 256u + threadIdx.x;
  if (i >= hw) return;
  const size_t at = (size_t)blockIdx.y * stride + i;
  const double M0 = (double)m0[at], M1 = (double)m1[at], M2 = (double)m2[at];
  float value = 0.0f;
  if (M0 > 0.0) {
    const int x = (int)(i % (unsigned)nx), y = (int)(i / (unsigned)nx);
    const unsigned projection = first_projection + blockIdx.y;
    const double lambda = na * M0, mu = M1 / M0, s2 = fmax(M2 / M0 - mu * mu, 0.0);
    double u;
    const double z0 = draw_normal(x, y, projection, 0u, seed, u);
    double n = 0.0;
    if (lambda < 64.0) {
      double p = exp(-lambda), F = p;
      while (u > F && n < 1024.0) {
        n += 1.0;
        p *= lambda / n;
        F += p;
      }
    } else {
      n = fmax(0.0, floor(lambda + sqrt(lambda) * z0 + (z0 * z0 - 1.0) / 6.0 + 0.5));
    }
    if (n > 0.0) {
      double unused;
      const double z1 = draw_normal(x, y, projection, 1u, seed, unused);
      value = (float)(fmax(0.0, n * mu + sqrt(n * s2) * z1) / na);
    }
  }
  out[(size_t)blockIdx.y * hw + i] = value;
}

// max(0, mean + sqrt(max(variance, 0)) z2)
__global__ __launch_bounds__(256) void gaussian_sample_kernel(const float* __restrict__ mean, const float* __restrict__ variance, float* __restrict__ out,
                                                              int nx, unsigned int hw, unsigned long long seed, unsigned first_projection) {
  const unsigned int i = blockIdx.x * 256u + threadIdx.x;
  if (i >= hw) return;
  const size_t at = (size_t)blockIdx.y * hw + i;
  double unused;
  const double z2 = draw_normal((int)(i % (unsigned)nx), (int)(i / (unsigned)nx), first_projection + blockIdx.y, 2u, seed, unused);
  out[at] = (float)fmax(0.0, (double)mean[at] + sqrt(fmax((double)variance[at], 0.0)) * z2);
}

void launch_compound_poisson(const float* m0, const float* m1, const float* m2, size_t stride, float* out, int n_planes, int ny, int nx, double na,
                             unsigned long long seed, unsigned first_projection) {
  const unsigned int hw = (unsigned int)ny * (unsigned int)nx;
  hipLaunchKernelGGL(compound_poisson_kernel, dim3((hw + 255u) / 256u, (unsigned)n_planes), dim3(256), 0, nullptr, m0, m1, m2, stride, out, nx, hw, na, seed,
                     first_projection);
}

// ---- the separable Gaussian of mcgpu_smooth_planes: scipy.ndimage.gaussian_filter, truncate 4, mode reflect ----------------
__device__ __forceinline__ int reflect_index(int i, int n) {  // d c b a | a b c d | d c b a
  if (n == 1) return 0;
  const int period = 2 * n;
  i %= period;
  if (i < 0) i += period;
  return i < n ? i : period - 1 - i;
}
// one pass along the axis of stride `stride` and length n: double accumulation in scipy's symmetric order, float32 storage
__global__ __launch_bounds__(256) void gauss_pass_kernel(const float* __restrict__ in, float* __restrict__ out, int ny, int nx, int along_y,
                                                         const double* __restrict__ w, int radius) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= nx) return;
  const float* const plane = in + (size_t)blockIdx.z * ny * nx;
  const int n = along_y ? ny : nx, k = along_y ? y : x;
  const size_t base = along_y ? (size_t)x : (size_t)y * nx, stride = along_y ? (size_t)nx : 1;
  double tmp = (double)plane[base + (size_t)k * stride] * w[radius];
  for (int j = -radius; j < 0; ++j)
    tmp += ((double)plane[base + (size_t)reflect_index(k + j, n) * stride] + (double)plane[base + (size_t)reflect_index(k - j, n) * stride]) * w[j + radius];
  out[(size_t)blockIdx.z * ny * nx + (size_t)y * nx + x] = (float)tmp;
}

std::vector<double> gaussian_weights(double sigma, int& radius) {
  radius = (int)(4.0 * sigma + 0.5);
  std::vector<double> w(2 * radius + 1);
  double sum = 0.0;
  const double s2 = sigma * sigma;
  for (int i = -radius; i <= radius; ++i) { w[i + radius] = exp(-0.5 / s2 * (double)(i * i)); sum += w[i + radius]; }
  for (double& v : w) v /= sum;
  return w;
}

// ---- host: Gauss-Legendre, the solid angle, the spectrum tables, the poses ------------------------------------------------
// nodes on [-1, 1] and weights (sum 2) of the n-point rule, by Newton's iteration on the Legendre polynomial
void gauss_legendre(int n, std::vector<double>& x, std::vector<double>& w) {
  x.resize(n);
  w.resize(n);
  for (int i = 0; i < n; ++i) {
    double z = cos(kPi * (i + 0.75) / (n + 0.5)), pp = 1.0;
    for (int it = 0; it < 100; ++it) {
      double p1 = 1.0, p2 = 0.0;
      for (int j = 1; j <= n; ++j) { const double p3 = p2; p2 = p1; p1 = ((2.0 * j - 1.0) * z * p2 - (j - 1.0) * p3) / j; }
      pp = n * (z * p1 - p2) / (z * z - 1.0);
      const double dz = p1 / pp;
      z -= dz;
      if (fabs(dz) < 1e-16) break;
    }
    x[n - 1 - i] = z;
    w[n - 1 - i] = 2.0 / ((1.0 - z * z) * pp * pp);
  }
}

// Omega = int dphi [min(z_hi, g) - max(z_lo, -g)]+, g(phi) = h |sin phi| / sqrt(1 + h^2 sin^2 phi): |dz / dy| <= h with dy = sin(theta) sin(phi)
double solid_angle(const SourcePose& s) {
  const double z_a = s.cos_theta_low, z_b = z_a + (double)s.D_cos_theta, z_lo = std::min(z_a, z_b), z_hi = std::max(z_a, z_b), p0 = s.phi_low, p1 = p0 + (double)s.D_phi, h = s.max_height_at_y1cm;
  if (!(p1 > p0) || !(z_hi > z_lo) || !(h > 0.0)) return 0.0;
  std::vector<double> cuts{p0, p1};
  auto add = [&](double phi) {  // every image of phi modulo 2 pi inside (p0, p1)
    for (double k = floor((p0 - phi) / (2.0 * kPi)); phi + 2.0 * kPi * k < p1; k += 1.0)
      if (phi + 2.0 * kPi * k > p0) cuts.push_back(phi + 2.0 * kPi * k);
  };
  add(0.0);
  add(kPi);
  for (const double c : {z_hi, -z_lo}) {  // kinks: g(phi) = c
    if (!(c > 0.0 && c < 1.0)) continue;
    const double sn = c / (h * sqrt(1.0 - c * c));
    if (!(sn > 0.0 && sn < 1.0)) continue;
    const double a = asin(sn);
    add(a); add(kPi - a); add(kPi + a); add(2.0 * kPi - a);
  }
  std::sort(cuts.begin(), cuts.end());
  std::vector<double> gx, gw;
  gauss_legendre(24, gx, gw);
  double omega = 0.0;
  for (size_t i = 0; i + 1 < cuts.size(); ++i) {
    const double a = cuts[i], b = cuts[i + 1];
    if (!(b > a)) continue;
    for (int j = 0; j < 24; ++j) {
      const double phi = 0.5 * (a + b) + 0.5 * (b - a) * gx[j], sn = fabs(sin(phi));
      const double g = h * sn / sqrt(1.0 + h * h * sn * sn);
      omega += 0.5 * (b - a) * gw[j] * std::max(0.0, std::min(z_hi, g) - std::max(z_lo, -g));
    }
  }
  return omega;
}

void invert3(const double m[9], double inv[9]) {
  const double det = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
  require(fabs(det) > 1e-12, -1, "!!ERROR!! mcgpu_primary_project: a pose matrix of the context is singular");
  const double c[9] = {m[4] * m[8] - m[5] * m[7], m[2] * m[7] - m[1] * m[8], m[1] * m[5] - m[2] * m[4],
                       m[5] * m[6] - m[3] * m[8], m[0] * m[8] - m[2] * m[6], m[2] * m[3] - m[0] * m[5],
                       m[3] * m[7] - m[4] * m[6], m[1] * m[6] - m[0] * m[7], m[0] * m[4] - m[1] * m[3]};
  for (int i = 0; i < 9; ++i) inv[i] = c[i] / det;
}

PrimaryProj primary_pose(const SourcePose& s, const DetectorPose& d) {
  PrimaryProj P{};
  for (int k = 0; k < 3; ++k) P.src[k] = s.pos[k];
  const double pitch_x = 1.0 / (double)d.inv_pixel_size_X, pitch_z = 1.0 / (double)d.inv_pixel_size_Z;
  if (d.rotation_flag == 1) {
    double R[9], Ri[9], n[3], c[3];
    for (int i = 0; i < 9; ++i) R[i] = d.rot_inv[i];
    invert3(R, Ri);
    const double nn = sqrt((double)s.dir[0] * s.dir[0] + (double)s.dir[1] * s.dir[1] + (double)s.dir[2] * s.dir[2]);
    for (int k = 0; k < 3; ++k) P.nrm[k] = s.dir[k] / nn;
    for (int r = 0; r < 3; ++r) {
      n[r] = R[3 * r] * s.dir[0] + R[3 * r + 1] * s.dir[1] + R[3 * r + 2] * s.dir[2];
      c[r] = R[3 * r] * d.center[0] + R[3 * r + 1] * d.center[1] + R[3 * r + 2] * d.center[2];
    }
    require(fabs(n[1]) > 1e-6, -1, "!!ERROR!! mcgpu_primary_project: the detector pose of the context is degenerate");
    auto point = [&](double xd, double zd, double q[3]) {
      const double rx = (double)d.corner_min[0] + xd * pitch_x, rz = (double)d.corner_min[2] + zd * pitch_z;
      const double ry = c[1] + (n[0] * (c[0] - rx) + n[2] * (c[2] - rz)) / n[1];
      for (int k = 0; k < 3; ++k) q[k] = Ri[3 * k] * rx + Ri[3 * k + 1] * ry + Ri[3 * k + 2] * rz;
    };
    double qu[3], qv[3];
    point(0.0, 0.0, P.o);
    point(1.0, 0.0, qu);
    point(0.0, 1.0, qv);
    for (int k = 0; k < 3; ++k) { P.u[k] = qu[k] - P.o[k]; P.v[k] = qv[k] - P.o[k]; }
    double F[9];
    for (int i = 0; i < 9; ++i) F[i] = s.rot_fan[i];
    invert3(F, P.beam);
  } else {
    P.o[0] = d.corner_min[0]; P.o[1] = d.center[1]; P.o[2] = d.corner_min[2];
    P.u[0] = pitch_x; P.v[2] = pitch_z;
    P.nrm[1] = 1.0;
    P.beam[0] = P.beam[4] = P.beam[8] = 1.0;
  }
  P.z_lo = std::min((double)s.cos_theta_low, (double)s.cos_theta_low + (double)s.D_cos_theta);  // D_cos_theta is negative: the interval runs downwards
  P.z_hi = std::max((double)s.cos_theta_low, (double)s.cos_theta_low + (double)s.D_cos_theta);
  P.phi_lo = s.phi_low;
  P.d_phi = s.D_phi;
  P.height = s.max_height_at_y1cm;
  const double omega = solid_angle(s);
  require(omega > 0.0, -1, "!!ERROR!! mcgpu_primary_project: the source aperture of the context is empty");
  P.inv_omega = 1.0 / omega;
  return P;
}

// W[q] and K[q][compact material] of the context's spectrum and tables; moments == 3: W = [W^(1) | W^(0) | W^(2)], W^(k)_q = P_b g_j E_q^k
void spectrum_tables(const HostModel& H, const DeviceModel& D, int qn, int moments, std::vector<double>& W, std::vector<double>& K) {
  const Spectrum& sp = H.spectrum;
  const int nb = sp.num_bins;
  std::vector<double> prob(nb, 0.0);
  for (int i = 0; i < nb; ++i) {
    const double c = std::min(1.0, std::max(0.0, (double)sp.cutoff[i]));
    prob[i] += c / nb;
    const int a = sp.alias[i];
    if (a >= 0 && a < nb) prob[a] += (1.0 - c) / nb;
    else prob[i] += (1.0 - c) / nb;
  }
  std::vector<double> gx, gw;
  gauss_legendre(qn, gx, gw);
  int material_of[kMaxMaterials] = {};
  for (int m = 0; m < kMaxMaterials; ++m)
    if (D.compact_of[m] >= 0 && D.compact_of[m] < D.nmat) material_of[D.compact_of[m]] = m;
  W.clear();
  K.clear();
  std::vector<double> W0, W2;
  const double e0 = H.mat.e0, ide = H.mat.ide;
  for (int b = 0; b < nb; ++b) {
    if (!(prob[b] > 0.0)) continue;
    const double lo = sp.espc[b], hi = sp.espc[b + 1];
    for (int j = 0; j < qn; ++j) {
      const double E = 0.5 * (lo + hi) + 0.5 * (hi - lo) * gx[j];
      W.push_back(prob[b] * 0.5 * gw[j] * E);
      W0.push_back(prob[b] * 0.5 * gw[j]);
      W2.push_back(prob[b] * 0.5 * gw[j] * E * E);
      const int bin = std::min(std::max((int)floor((E - e0) * ide), 0), H.mat.num_values - 1);
      for (int mc = 0; mc < D.nmat; ++mc) {
        const size_t row = (size_t)bin * kMaxMaterials + material_of[mc];
        K.push_back((double)H.mat.a[row].x + E * (double)H.mat.b[row].x);
      }
    }
  }
  if (moments == 3) {
    W.insert(W.end(), W0.begin(), W0.end());
    W.insert(W.end(), W2.begin(), W2.end());
  }
}

template <int VK, int NM>
void launch_primary(float* d_out, const PrimaryVol& A, const PrimaryProj* d_proj, const double* d_W, const double* d_K, int nb) {
  const size_t lds = (size_t)A.nmat * kLanes * 4 + (VK == kVolU8 ? 256 * sizeof(float2) : 0);
  hipLaunchKernelGGL((primary_kernel<VK, NM>), dim3((A.crop_nx + 15) / 16, (A.nz + 15) / 16, nb), dim3(kLanes), lds, nullptr, d_out, A, d_proj, d_W, d_K);
}
template <int NM>
void launch_primary_of(int vol_kind, float* d_out, const PrimaryVol& A, const PrimaryProj* d_proj, const double* d_W, const double* d_K, int nb) {
  if (vol_kind == kVolU8) launch_primary<kVolU8, NM>(d_out, A, d_proj, d_W, d_K, nb);
  else if (vol_kind == kVolU16) launch_primary<kVolU16, NM>(d_out, A, d_proj, d_W, d_K, nb);
  else launch_primary<kVolRaw, NM>(d_out, A, d_proj, d_W, d_K, nb);
}


struct Noise {  // of mcgpu_primary_noisy: the moments stay on the device, the sampled plane comes back
  double histories;
  unsigned long long seed;
};

// The three entry points on a context: `moments` planes per projection (1: M_1, 3: M_0, M_1, M_2) to `planes`, or with `noise` the
// sampled plane alone.  Every refusal stands before the first HIP call.
void primary_run(const char* fn, mcgpu_ctx* ctx, const mcgpu_primary_options& o, int moments, const Noise* noise, float* planes,
                 mcgpu_primary_report* report) {
  check_report(fn, "report", "mcgpu_primary_report", report);
  if (!(ctx && ctx->has_device && planes)) refuse(fn, "bad argument (the context needs a device)");
  if (noise && !(std::isfinite(noise->histories) && noise->histories > 0.0)) refuse(fn, "histories must be finite and > 0");
  const HostModel& H = ctx->host;
  const DeviceModel& D = ctx->dev;
  const int np = (int)H.source.size();
  const int n_proj = o.n_projections > 0 ? o.n_projections : 1;
  if (o.first_projection < 0 || o.n_projections < 0 || o.first_projection + n_proj > np)
    refuse(fn, "projections " + std::to_string(o.first_projection) + " .. " + std::to_string(o.first_projection + n_proj - 1) +
                   " are not within the context's " + std::to_string(np));
  const int su = o.su ? o.su : 1, sv = o.sv ? o.sv : 1, qn = o.energy_points ? o.energy_points : 2;
  if (!(su >= 1 && su <= 8 && sv >= 1 && sv <= 8)) refuse(fn, "su and sv must be within 1 .. 8 (0: 1)");
  if (!(qn >= 1 && qn <= 4)) refuse(fn, "energy_points must be within 1 .. 4 (0: 2)");
  if (!(D.nmat >= 1 && D.nmat <= kMaxMaterials)) refuse(fn, "the context holds no material");
  const DetectorPose& d0 = H.detector[o.first_projection];
  const int nx = d0.nx, nz = d0.nz, crop = (o.crop_nx > 0 && o.crop_nx < nx) ? o.crop_nx : nx;
  const double na = noise ? noise->histories / ((double)d0.inv_pixel_size_X * (double)d0.inv_pixel_size_Z) : 0.0;  // N a
  if (noise && !(std::isfinite(na) && na > 0.0)) refuse(fn, "the pixel area of the context's detector is not positive");

  const Stopwatch clock;
  std::vector<double> W, K;
  spectrum_tables(H, D, qn, moments, W, K);
  std::vector<PrimaryProj> poses(n_proj);
  for (int k = 0; k < n_proj; ++k) poses[k] = primary_pose(H.source[o.first_projection + k], H.detector[o.first_projection + k]);
  double ms_tables = clock.ms();

  HIP_TRY(hipSetDevice(D.device_id));
  CallDevice dev;
  const Stopwatch up;
  const double* d_W = dev.upload(W);
  const double* d_K = dev.upload(K);
  const PrimaryProj* d_proj = dev.upload(poses);
  ms_tables += up.ms();
  PrimaryVol A{};
  A.vol = D.vol;
  A.pal = (const float2*)D.palette;
  A.pal_n = D.palette_size;
  for (int k = 0; k < 3; ++k) { A.n[k] = H.voxels.n[k]; A.vs[k] = H.voxels.voxel_size[k]; }
  A.sub_nx = (unsigned)((A.n[0] + 3) >> 2);
  A.sub_nxy = A.sub_nx * (unsigned)((A.n[1] + 3) >> 2);
  A.nx = nx; A.nz = nz; A.crop_nx = crop; A.su = su; A.sv = sv; A.nq = (int)W.size() / moments; A.nmat = D.nmat;
  if (!(D.vol_kind != kVolU8 || D.palette_size <= 256)) refuse(fn, "a u8 volume with more than 256 palette entries");
  const size_t plane = (size_t)crop * nz;
  const int chunk = std::min(n_proj, kChunk);
  float* d_out = dev.alloc_zeroed<float>((size_t)chunk * moments * plane * 4);
  float* d_noisy = noise ? dev.alloc_zeroed<float>((size_t)chunk * plane * 4) : nullptr;
  dev.events();
  double ms_kernel = 0.0, ms_sample = 0.0;
  for (int first = 0; first < n_proj; first += chunk) {
    const int m = std::min(chunk, n_proj - first);
    Stage st(dev, ms_kernel);
    if (moments == 3) launch_primary_of<3>(D.vol_kind, d_out, A, d_proj + first, d_W, d_K, m);
    else launch_primary_of<1>(D.vol_kind, d_out, A, d_proj + first, d_W, d_K, m);
    st.done();
    if (noise) {
      Stage sample(dev, ms_sample);
      launch_compound_poisson(d_out, d_out + plane, d_out + 2 * plane, 3 * plane, d_noisy, m, nz, crop, na, noise->seed, (unsigned)(o.first_projection + first));
      sample.done();
      HIP_TRY(hipMemcpy(planes + (size_t)first * plane, d_noisy, (size_t)m * plane * 4, hipMemcpyDeviceToHost));
    } else {
      HIP_TRY(hipMemcpy(planes + (size_t)first * moments * plane, d_out, (size_t)m * moments * plane * 4, hipMemcpyDeviceToHost));
    }
  }
  mcgpu_primary_report r{};
  r.ms_kernel = ms_kernel;
  r.ms_tables = ms_tables;
  r.solid_angle = 1.0 / poses[0].inv_omega;
  r.n_materials = D.nmat;
  r.n_energy_points = A.nq;
  r.ms_sample = ms_sample;
  write_report(report, r);
}

// what the two samplers on host planes refuse
void check_sampler(const char* fn, bool pointers, int n_planes, int ny, int nx, int first_projection) {
  if (!pointers) refuse(fn, "a plane pointer is NULL");
  if (!(n_planes >= 1 && n_planes <= 65535 && ny >= 1 && nx >= 1 && (unsigned long long)ny * (unsigned long long)nx <= 0x7fffffffull))
    refuse(fn, "n_planes must be within 1 .. 65535, ny and nx >= 1 and ny x nx below 2^31");
  if (first_projection < 0 || (long long)first_projection + n_planes > 0x7fffffffLL) refuse(fn, "first_projection must be >= 0");
}

}  // namespace

extern "C" int mcgpu_primary_project(mcgpu_ctx* ctx, const mcgpu_primary_options* caller_o, float* planes, mcgpu_primary_report* report) {
  ABI_BEGIN
  mcgpu_primary_options o;
  read_options("mcgpu_primary_project", "mcgpu_primary_options", caller_o, o);
  primary_run("mcgpu_primary_project", ctx, o, 1, nullptr, planes, report);
  return 0;
  ABI_END
}

extern "C" int mcgpu_primary_moments(mcgpu_ctx* ctx, const mcgpu_primary_options* caller_o, float* planes, mcgpu_primary_report* report) {
  ABI_BEGIN
  mcgpu_primary_options o;
  read_options("mcgpu_primary_moments", "mcgpu_primary_options", caller_o, o);
  primary_run("mcgpu_primary_moments", ctx, o, 3, nullptr, planes, report);
  return 0;
  ABI_END
}

extern "C" int mcgpu_primary_noisy(mcgpu_ctx* ctx, const mcgpu_primary_noisy_options* caller_o, float* planes, mcgpu_primary_report* report) {
  ABI_BEGIN
  mcgpu_primary_noisy_options n;
  read_options("mcgpu_primary_noisy", "mcgpu_primary_noisy_options", caller_o, n);
  mcgpu_primary_options o{};
  o.struct_size = (unsigned int)sizeof o;
  o.first_projection = n.first_projection; o.n_projections = n.n_projections; o.su = n.su; o.sv = n.sv;
  o.energy_points = n.energy_points; o.crop_nx = n.crop_nx;
  const Noise noise{n.histories, n.seed};
  primary_run("mcgpu_primary_noisy", ctx, o, 3, &noise, planes, report);
  return 0;
  ABI_END
}

extern "C" int mcgpu_sample_compound_poisson(int device, const float* m0, const float* m1, const float* m2, float* out, int n_planes, int ny, int nx,
                                             double histories, double pixel_area, unsigned long long seed, int first_projection) {
  ABI_BEGIN
  const char* fn = "mcgpu_sample_compound_poisson";
  check_sampler(fn, m0 && m1 && m2 && out, n_planes, ny, nx, first_projection);
  if (!(std::isfinite(histories) && histories > 0.0)) refuse(fn, "histories must be finite and > 0");
  const double na = histories * pixel_area;
  if (!(std::isfinite(pixel_area) && pixel_area > 0.0 && std::isfinite(na) && na > 0.0)) refuse(fn, "pixel_area must be finite and > 0");
  const size_t n = (size_t)n_planes * ny * nx;
  HIP_TRY(hipSetDevice(device));
  CallDevice dev;
  const float *d0 = dev.upload(m0, n), *d1 = dev.upload(m1, n), *d2 = dev.upload(m2, n);
  float* d_out = dev.alloc<float>(n * 4);
  launch_compound_poisson(d0, d1, d2, (size_t)ny * nx, d_out, n_planes, ny, nx, na, seed, (unsigned)first_projection);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, d_out, n * 4, hipMemcpyDeviceToHost));
  return 0;
  ABI_END
}

extern "C" int mcgpu_sample_gaussian(int device, const float* mean, const float* variance, float* out, int n_planes, int ny, int nx,
                                     unsigned long long seed, int first_projection) {
  ABI_BEGIN
  const char* fn = "mcgpu_sample_gaussian";
  check_sampler(fn, mean && variance && out, n_planes, ny, nx, first_projection);
  const size_t n = (size_t)n_planes * ny * nx;
  HIP_TRY(hipSetDevice(device));
  CallDevice dev;
  const float *d_mean = dev.upload(mean, n), *d_var = dev.upload(variance, n);
  float* d_out = dev.alloc<float>(n * 4);
  const unsigned int hw = (unsigned int)ny * (unsigned int)nx;
  hipLaunchKernelGGL(gaussian_sample_kernel, dim3((hw + 255u) / 256u, (unsigned)n_planes), dim3(256), 0, nullptr, d_mean, d_var, d_out, nx, hw, seed,
                     (unsigned)first_projection);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, d_out, n * 4, hipMemcpyDeviceToHost));
  return 0;
  ABI_END
}

extern "C" int mcgpu_smooth_planes(int device, const float* planes_in, float* planes_out, int n_planes, int ny, int nx, double sigma_y,
                                   double sigma_x, double* ms_kernel) {
  ABI_BEGIN
  require(planes_in && planes_out && n_planes >= 1 && n_planes <= 65535 && ny >= 1 && ny <= 65535 && nx >= 1, -1, "!!ERROR!! mcgpu_smooth_planes: bad argument");
  require(sigma_y >= 0.0 && sigma_x >= 0.0 && sigma_y <= 1.0e4 && sigma_x <= 1.0e4, -1, "!!ERROR!! mcgpu_smooth_planes: a sigma must be within 0 .. 1e4");
  const size_t n = (size_t)n_planes * ny * nx;
  double ms = 0.0;
  const bool along_y = sigma_y > 1e-15, along_x = sigma_x > 1e-15;
  if (!along_y && !along_x) {
    if (planes_out != planes_in) memmove(planes_out, planes_in, n * 4);
  } else {
    HIP_TRY(hipSetDevice(device));
    CallDevice dev;
    float* a = dev.upload(planes_in, n);
    float* b = dev.alloc<float>(n * 4);
    dev.events();
    const dim3 grid((unsigned)((nx + 255) / 256), (unsigned)ny, (unsigned)n_planes);
    Stage st(dev, ms);
    for (int pass = 0; pass < 2; ++pass) {
      if (!(pass == 0 ? along_y : along_x)) continue;
      int radius;
      const std::vector<double> w = gaussian_weights(pass == 0 ? sigma_y : sigma_x, radius);
      const double* d_w = dev.upload(w);
      hipLaunchKernelGGL(gauss_pass_kernel, grid, dim3(256), 0, nullptr, a, b, ny, nx, pass == 0 ? 1 : 0, d_w, radius);
      std::swap(a, b);
    }
    st.done();
    HIP_TRY(hipMemcpy(planes_out, a, n * 4, hipMemcpyDeviceToHost));
  }
  if (ms_kernel) *ms_kernel = ms;
  return 0;
  ABI_END
}
