// joseph_ray.inc -- the per-ray body of the Joseph forward projector, shared by forward_project.hip (3-D volumes) and rooster4d.hip
// (phase-blended 4-D frames).  Scheme and geometry: forward_project.hip's header.  The voxel fetch is a template parameter
// (src(x, y, z, pal) = density at IEC index (x, y, z), always inside the volume); everything else is the same arithmetic for every
// source, so the same densities give bit-identical sums.  With it what both kernels and both hosts said around the ray: the volume
// and detector part of the kernel arguments (FpVolume) and its fill from an options struct, the pixel a lane takes of its workgroup's
// tile, and the poses of one launch.  Included after hip_host.hpp.
#pragma once

using FpProj = mcgpu::ProjectionPose;  // c, s, off_x, off_y of one projection, in double

struct FpVolume {                  // what joseph_ray reads of its arguments; the kernels' argument structs derive from it
  int nu, nv;
  int n[3];                        // IEC volume size (x fastest)
  double u0, v0, du, dv, sid, sdd;
  double o[3], sp[3];              // origin (centre of voxel 0) and spacing, mm
};

// the FpVolume of a volume of n voxels of sp mm under the cone-beam fields of o (any options struct that has them)
template <class O>
FpVolume fp_volume(const O& o, const int n[3], const double sp[3]) {
  FpVolume A = {o.nu, o.nv, {n[0], n[1], n[2]}, o.u0, o.v0, o.du, o.dv, o.sid, o.sdd, {}, {sp[0], sp[1], sp[2]}};
  const double org[3] = {o.ox, o.oy, o.oz};
  for (int a = 0; a < 3; ++a) A.o[a] = mcgpu::centred_origin(n[a], sp[a], org[a]);
  return A;
}

// the poses of projections [first, first + nb) of o: the per-launch block of the kernel arguments
template <class O>
void fp_poses(const O& o, int first, int nb, FpProj* pp) {
  for (int k = 0; k < nb; ++k) pp[k] = mcgpu::projection_pose(o, first + k);
}

// One lane per detector pixel: a wave covers an 8 x 8 pixel tile, a workgroup of 256 lanes 2 x 2 tiles, blockIdx.z a projection of
// the batch.  fp_grid is the grid of nb projections, fp_pixel the lane's pixel; false beyond the detector's edge.
inline dim3 fp_grid(int nu, int nv, int nb) { return dim3((unsigned)((nu + 15) / 16), (unsigned)((nv + 15) / 16), (unsigned)nb); }
__device__ inline bool fp_pixel(const FpVolume& A, int& iu, int& iv) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  iu = blockIdx.x * 16 + (w & 1) * 8 + (l & 7);
  iv = blockIdx.y * 16 + (w >> 1) * 8 + (l >> 3);
  return iu < A.nu && iv < A.nv;
}

// element m of (v0, v1, v2) by selects: a per-lane index into a private array would put the array in scratch
template <class T>
__device__ inline T sel3(int m, T v0, T v1, T v2) { return m == 0 ? v0 : (m == 1 ? v1 : v2); }

// line integral of detector pixel (iu, iv) of the projection P
template <class Src>
__device__ inline float joseph_ray(const FpVolume& A, const FpProj& P, int iu, int iv, const Src& src, const float* pal) {
  // ray source -> pixel in world coordinates, then in index coordinates of the volume
  const double xr = A.u0 + A.du * iu + P.off_x, yr = A.v0 + A.dv * iv + P.off_y, zr = A.sid - A.sdd;
  const double S[3] = {P.s * A.sid, 0.0, P.c * A.sid};
  const double D[3] = {P.c * xr + P.s * zr - S[0], yr - S[1], -P.s * xr + P.c * zr - S[2]};
  double Si[3], Di[3];
  double t0 = 0.0, t1 = 1.0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    Si[a] = (S[a] - A.o[a]) / A.sp[a];
    Di[a] = D[a] / A.sp[a];
    const double lo = -0.5, hi = A.n[a] - 0.5;
    if (Di[a] != 0.0) {
      double ta = (lo - Si[a]) / Di[a], tb = (hi - Si[a]) / Di[a];
      if (ta > tb) { const double t = ta; ta = tb; tb = t; }
      t0 = fmax(t0, ta); t1 = fmin(t1, tb);
    } else if (Si[a] < lo || Si[a] > hi) {
      t1 = -1.0;
    }
  }
  float out = 0.f;
  if (t0 < t1) {
    int m = 0;
    if (fabs(Di[1]) > fabs(Di[0])) m = 1;
    if (fabs(Di[2]) > fabs(sel3(m, Di[0], Di[1], Di[2]))) m = 2;
    // (a1, a2) = the other two axes in increasing order
    const double Sm = sel3(m, Si[0], Si[1], Si[2]), Dm = sel3(m, Di[0], Di[1], Di[2]);
    const double S1 = (m == 0) ? Si[1] : Si[0], D1 = (m == 0) ? Di[1] : Di[0];
    const double S2 = (m == 2) ? Si[1] : Si[2], D2 = (m == 2) ? Di[1] : Di[2];
    const int nm = sel3(m, A.n[0], A.n[1], A.n[2]), na = (m == 0) ? A.n[1] : A.n[0], nb = (m == 2) ? A.n[1] : A.n[2];
    const double e0 = Sm + t0 * Dm, e1 = Sm + t1 * Dm;
    const double lo = fmin(e0, e1), hi = fmax(e0, e1);
    const int ns = max((int)floor(lo + 0.5), 0), fs = min((int)floor(hi + 0.5), nm - 1);
    if (ns <= fs) {
      const double r1 = D1 / Dm, r2 = D2 / Dm;
      const float w_first = (float)(ns == fs ? hi - lo : ns + 0.5 - lo), w_last = (float)(hi - fs + 0.5);
      const double A0 = S1 + (ns - Sm) * r1, B0 = S2 + (ns - Sm) * r2;
      // Tap positions and the running sum in float64, the bilinear sample itself in float32.  A float32 position near voxel 512
      // is off by up to 3e-5 voxel (its own rounding, and the rounded slope times up to 511 steps); along an edge of the
      // density that a ray follows for many steps these errors all have one sign.  A float32 sum of equal samples (a
      // homogeneous body) rounds the same way at every step of a binade.  On the Catphan604 volume of 512^3 voxels at the
      // reference's detector, against the float64 restatement (tests/test_forward_projection_configs.py): 4.1 x the tolerance
      // with both in float32 (measured), 1.3 x with the positions alone in float64 (emulated), 0.007 x as written here
      // (measured).  Cost on an MI355X: 2 % of the kernel time from a float volume, 7 % from the context's u8 volume.
      double acc = 0.0;
      for (int k = ns; k <= fs; ++k) {
        const double dk = (double)(k - ns);
        const double a = fma(dk, r1, A0), b = fma(dk, r2, B0);
        const double fa0 = floor(a), fb0 = floor(b);
        const int ia = (int)fa0, ib = (int)fb0;
        const float fa = (float)(a - fa0), fb = (float)(b - fb0);
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int qa = ia + (q & 1), qb = ib + (q >> 1);
          v[q] = 0.f;
          if ((unsigned)qa < (unsigned)na && (unsigned)qb < (unsigned)nb) {
            const int x = (m == 0) ? k : qa;
            const int y = (m == 1) ? k : (m == 0 ? qa : qb);
            const int z = (m == 2) ? k : qb;
            v[q] = src(x, y, z, pal);
          }
        }
        const float ga = 1.f - fa, gb = 1.f - fb;
        const float s = gb * (ga * v[0] + fa * v[1]) + fb * (ga * v[2] + fa * v[3]);
        const float wk = (k == ns) ? w_first : (k == fs ? w_last : 1.f);
        acc = fma((double)wk, (double)s, acc);
      }
      const double len = sqrt(D[0] * D[0] + D[1] * D[1] + D[2] * D[2]) / fabs(Dm);  // mm per main-axis step
      out = (float)(acc * len);
    }
  }
  return out;
}
