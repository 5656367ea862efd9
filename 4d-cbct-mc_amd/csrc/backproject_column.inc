// backproject_column.inc -- the voxel-driven bilinear back-projector's column, stated once for fdk.hip's backproject_kernel and
// wpc_fit.hip's slab_backproject_kernel (both through fdk_common.inc) and rooster4d.hip's bp4_kernel; the counterpart of joseph_ray.inc.
// A thread owns one (x, z) column of the volume, sets up what does not depend on y for a batch of projections (column_setup), then walks
// y and takes one detector sample per projection and step (detector_rows, detector_sample).  With them the two rules of the weighting
// pass: the water pre-correction polynomial and the detector weight.  Needs the HIP runtime header only.  All of it is explicit fmaf
// or single operations, except column_setup and wpc_polynomial, whose multiply-adds the including file's -ffp-contract setting decides.
// bp4_kernel shares the sample and keeps its own setup: that runs in double, refuses U <= 0 (FDK's kernels must not), takes av_b from
// the host, weighs by mag^2 K and reads its poses from three arrays -- more than a type parameter and one flag.
#pragma once

// projections per back-projection launch.  Measured at the reference's size (tools/archive/fdk_bench.py): 8 projections and 4 waves
// per SIMD (78 VGPRs) 101 ms; 16 / 4 waves (128 VGPRs + scratch) 133 ms; 8 / 8 waves (scratch) 132 ms; 32 / 2 waves 215 ms
constexpr int kBatch = 8;

struct ProjParam {  // per projection, wave-uniform in the kernels
  float c, s;       // cos / sin of the gantry angle
  float off_x, off_y;
  float gap;        // angular weight [rad]: half the distance to both neighbouring projections (RTK GetAngularGaps)
};

struct BackArgs {
  int nx, ny, nz, nu, nv, nb;  // nb = projections in this batch; nu = usable columns
  int u_first;                 // column of the buffer rows that holds detector column 0 (the --pad extension lies before it)
  int stride;                  // floats per detector row in q
  float x0, y0, z0, sx, sy, sz;
  float sid, sdd, inv_du, inv_dv, u0, v0;
  ProjParam pp[kBatch];
};

// ---- the y walk ------------------------------------------------------------------------------------------------------------
// the bilinear blend of detector pixels (iu, iu + 1) of rows iv (v00, v01) and iv + 1 (v10, v11)
__device__ inline float detector_lerp(float au, float av, float v00, float v01, float v10, float v11) {
  const float top = fmaf(au, v01 - v00, v00), bot = fmaf(au, v11 - v10, v10);
  return fmaf(av, bot - top, top);
}

// The detector sample of the y walk, in all three kernels: if (detector_rows(fv, nv, iv, av)) detector_sample(&row iv[iu], stride, au, av).
// rows iv = floor(fv), iv + 1 of a detector of nv rows: a sample counts only with both inside
__device__ inline bool detector_rows(float fv, int nv, int& iv, float& av) {
  const float fl = floorf(fv);
  iv = (int)fl;
  av = fv - fl;
  return iv >= 0 && iv < nv - 1;
}

// the blend at r0 = &row iv[iu]: (iu, iu + 1) of both rows with one 8-byte load each (4-byte aligned: global loads need no more).  The
// interleaved layout of the slab kernel loads for itself and shares detector_lerp
__device__ inline float detector_sample(const float* r0, int stride, float au, float av) {
  float2 lo, hi;
  __builtin_memcpy(&lo, r0, 8);
  __builtin_memcpy(&hi, r0 + stride, 8);
  return detector_lerp(au, av, lo.x, lo.y, hi.x, hi.y);
}

// ---- the column setup of FDK's geometry --------------------------------------------------------------------------------------
struct Column {     // what the walk of one projection needs of its (x, z) column
  int iu;           // -1: the column misses the detector (both columns inside, or none)
  float au, wg;     // column fraction; angular gap x (sid / U)^2
  float av_a, av_b; // fv = av_a * Y + av_b
};

// column (X, Z) under projection k of the batch.  An empty slot (k >= A.nb) holds the identity pose.  kSkipEmpty: leave it out with a
// scalar branch (backproject_kernel); else compute it too and refuse it in the range test (slab_backproject_kernel, where the branch
// costs registers)
template <bool kSkipEmpty>
__device__ inline Column column_setup(const BackArgs& A, int k, float X, float Z) {
  Column col = {-1, 0.f, 0.f, 0.f, 0.f};
  if (kSkipEmpty && k >= A.nb) return col;
  const float xr = X * A.pp[k].c - Z * A.pp[k].s, zr = X * A.pp[k].s + Z * A.pp[k].c;
  const float U = A.sid - zr, mag = A.sdd / U;
  const float fu = (mag * xr - A.pp[k].off_x - A.u0) * A.inv_du;
  const float fl = floorf(fu);
  const int i = (int)fl;
  if ((kSkipEmpty || k < A.nb) && i >= 0 && i < A.nu - 1) {
    col.iu = i;
    col.au = fu - fl;
    const float r = A.sid / U;
    col.wg = A.pp[k].gap * r * r;
    col.av_a = mag * A.inv_dv;
    col.av_b = (-A.pp[k].off_y - A.v0) * A.inv_dv;
  }
  return col;
}

// ---- the weighting pass ------------------------------------------------------------------------------------------------------
// rtkfdk --wpc: sum_j c_j p^j, in float32, in this order
__device__ inline float wpc_polynomial(const float* __restrict__ c, int n, float p) {
  float acc = 0.f, pw = 1.f;
  for (int j = 0; j < n; ++j) { acc += c[j] * pw; pw *= p; }
  return acc;
}

// cosine weight of the detector point (up, vp) [mm from the central ray] x the displaced-detector (half-fan) weight of its column
__device__ inline float detector_weight(float sdd, float up, float vp, float w_dis) { return sdd / sqrtf(sdd * sdd + up * up + vp * vp) * w_dis; }
