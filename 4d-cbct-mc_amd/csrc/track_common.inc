// track_common.inc -- device functions shared by the two photon-history kernels for CDNA4 (gfx950):
//   track_kernel.inc  COMPAT personality (one history per lane, RANECU batches; bit-exact against the CPU oracle)
//   track_pool.inc    FAST personality (two histories per lane: one in registers, one in a lane-private LDS slot)
// Included once per translation unit with MC_COMPAT defined to 1 (built with -ffp-contract=off) or 0.
//
// WHAT is computed follows the reference kernel track_particles and its helpers
// (docker/mcgpu/MC-GPU_kernel_v1.3.cu, "K.cu": source :626-686, move_to_bbox :714-805, locate_voxel
// :1033-1065, Woodcock loop :249-279, event selection :289-354, GCOa :1287-1515, GRAa :1181-1246,
// rotate_double :1103-1148, tally_image :482-604; SURVEY.md Appendix D).
//
//  * The voxel volume is a 1- or 2-byte palette index (device_model.hpp).  On top of it sits a brick grid
//    (bricks of 2^k voxels per side, 4 bits per brick, LDS-resident): a brick whose voxels all share one
//    palette entry answers the lookup from LDS; only bricks that straddle a material boundary go to the
//    volume in HBM/Infinity Cache.  Palette, Compton shells and the spectrum alias tables sit in LDS
//    (dynamic layout TrackArgs::lds, sized for the materials actually used); one 32-byte record per
//    (energy bin, material) replaces three table reads.
//  * COMPAT personality: RANECU leap-frog streams, the reference CPU-build arithmetic and the portable math
//    below -> integer tallies bit-identical to oracle/mcgpu_oracle.c (ORACLE_MATH_PORTABLE).
//    FAST personality: per-history counter-based streams (Philox4x32-7 -> multiply-with-carry), v_log/v_exp/v_sin,
//    the reference GPU-build integer conversions (floor / round-to-nearest).
//  * Tallies are 64-bit integer atomics: the image is independent of scheduling and of the rank split.

#include <hip/hip_runtime.h>

#include "device_model.hpp"

namespace mcgpu {
namespace {

constexpr int kBlock = kTrackBlockThreads;
constexpr float kEps = 0.000015f;  // EPS_SOURCE, MC-GPU_v1.3.h:87
// FAST: history ids are dealt from kNumCounters global counters, each owning a contiguous 1/kNumCounters of the launch, in
// tickets of at most kChunk ids (id_tickets.hpp; track_pool.inc: id dealing); counters sit kCounterStride words apart (different memory channels)
constexpr unsigned int kChunk = kIdChunk;
constexpr int kBrickMixed = 0xF;      // brick code: look in the volume
constexpr int kBrickExterior = 14;    // brick code: background outside the object box (palette slot 14)
constexpr int kPaletteBase = 16;      // LDS palette: entries 0..14 = brick codes, 16.. = palette indices

// ESCAPED (-> detector tally), ABSORBED (-> dose tally) and NEW all end in the source sampler: one contiguous range
enum Phase : int { PH_FLIGHT = 0, PH_COMPTON = 1, PH_RAYLEIGH = 2, PH_ESCAPED = 3, PH_ABSORBED = 4, PH_NEW = 5, PH_DONE = 6,
                   PH_REAL = 7,   // FAST: a real interaction whose kind has not been drawn yet (register history only)
                   PH_HOP = 8,    // FAST: in the homogeneous exterior, waiting to be moved analytically (per-wave pool: by the tally + source service)
                   // FAST: the polar angle of a Compton event has been accepted (tau in History::aux), the momentum trial of its
                   // first shell failed: shell and momentum are drawn again at that angle (K.cu:1374-1480)
                   PH_SHELL = 9,
                   // COMPAT: a Compton event whose normalisation S0 is known and whose polar angle is still being drawn
                   // (PH_COMPTON: S0 not computed yet; PH_SHELL: angle accepted, shell + momentum being drawn)
                   PH_CTRIAL = 10 };

// Dynamic LDS, laid out by the host (TrackArgs::lds, byte offsets).
extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
#define LDS_F(off) (reinterpret_cast<float*>(lds_raw + (off)))
#define LDS_I(off) (reinterpret_cast<int*>(lds_raw + (off)))
#define LDS_S(off) (reinterpret_cast<short*>(lds_raw + (off)))
#define LDS_F2(off) (reinterpret_cast<float2*>(lds_raw + (off)))
// Pointers read from TrackCold are generic to the compiler; they all point to global memory.
#define GLOBAL_AS __attribute__((address_space(1)))
template <typename T>
__device__ __forceinline__ const GLOBAL_AS T* as_global(const T* p) { return (const GLOBAL_AS T*)p; }
// The per-launch parameter blocks (TrackCold, SourcePose, DetectorPose) are written by the host before the launch and
// only read by the kernel, always at wave-uniform addresses: read through the constant address space they become scalar
// loads (s_load into SGPRs: scalar cache, no vector-memory round trip, not ordered behind the kernel's atomics).
#define CONST_AS __attribute__((address_space(4)))
#define COLD(A) ((const CONST_AS TrackCold*)(A).cold)
// A launch argument that only the tally + source service reads (pose pointers, tally, id range, seed, counters): loaded from the
// kernel-argument segment where it is used -- the kernel's one parameter is the TrackArgs, at offset 0 -- instead of sitting in scalar
// registers from the kernel's first instruction on (with TrackCold::lds / mfp / e0 / ide / bbox: 4-12 SGPR spills instead of 39-49)
#if MC_COMPAT
#define LARG(A, field) ((A).field)
#else
#define LARG(A, field) (((const CONST_AS TrackArgs*)__builtin_amdgcn_kernarg_segment_ptr())->field)
#endif
// ... and one that every kernel reads that way, COMPAT included: the pointer of the optional second tally (TrackArgs::w2) is wanted only
// where a photon scores; as a launch argument proper it would hold a pair of scalar registers for the whole kernel
#define KARG(field) (((const CONST_AS TrackArgs*)__builtin_amdgcn_kernarg_segment_ptr())->field)
#define SRC(A) ((const CONST_AS SourcePose*)LARG(A, src))
#define DET(A) ((const CONST_AS DetectorPose*)LARG(A, det))
// byte offset of a SERVICE-side table in the LDS image (TrackCold::lds)
// ... and a launch argument that only the services read (TrackCold::mfp, e0, ide, bbox)
// (the COMPAT kernel keeps the launch arguments: at 4 waves/SIMD it has 106 scalar registers, and the same treatment cost it 1.3 %,
// profiles/r05q_*)
#if MC_COMPAT
#define SLDS(A, field) ((A).lds.field)
#define SARG(A, field) ((A).field)
#else
#define SLDS(A, field) (COLD(A)->lds.field)
#define SARG(A, field) (COLD(A)->field)
#endif

// Row of (energy bin, compact material) in the cross-section tables mfp (32-byte records) and mfp_tot: MATERIAL-major.
// A photon's interactions happen in a handful of materials (soft tissue, muscle, adipose, lung ...) at any energy of the
// spectrum: with bin-major rows every 128-byte line held four materials of one bin, so the hot set was the whole table
// (24001 bins x 14 materials x 32 B = 10.7 MB against 4 MB of L2 per XCD); material-major, the tables of the materials that
// are rarely hit stay cold and the frequent ones are contiguous (384 KB of records each).
__device__ __forceinline__ unsigned int table_row(const TrackArgs& A, int index, int mc) {
  return __umul24((unsigned int)mc, (unsigned int)A.num_values) + (unsigned int)index;
}

#if MC_COMPAT
#include "compat_math.inc"  // pm_log / pm_exp / pm_sincos / gl_expf and their tables
#endif
// ================================================================================================
// Math personality
// ================================================================================================
#if MC_COMPAT
__device__ __forceinline__ float mc_logf(float x) { return (float)pm_log((double)x); }
__device__ __forceinline__ float mc_expf(float x) { return gl_expf<true>(x); }  // every argument in this path is finite and <= 0.5
__device__ __forceinline__ float mc_powf(float b, float y) { return (float)pm_exp((double)y * pm_log((double)b)); }
__device__ __forceinline__ float mc_sqrtf(float x) { return sqrtf(x); }
#else
// v_log_f32 (log2) without the denormal pre-scaling of __logf: every argument here is >= 2^-24 or a normal float
__device__ __forceinline__ float mc_logf(float x) { return __builtin_amdgcn_logf(x) * 0.69314718055994531f; }
__device__ __forceinline__ float mc_expf(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896341f); }
__device__ __forceinline__ float mc_powf(float b, float y) { return __builtin_amdgcn_exp2f(y * __builtin_amdgcn_logf(b)); }
__device__ __forceinline__ float mc_sqrtf(float x) { return __builtin_amdgcn_sqrtf(x); }  // v_sqrt_f32, 1 ulp
#endif

// float division: IEEE in COMPAT, v_rcp_f32-based (1 ulp reciprocal) in FAST
#if MC_COMPAT
#define MC_DIV(a, b) ((a) / (b))
#else
#define MC_DIV(a, b) ((a) * __builtin_amdgcn_rcpf(b))
#endif

// ================================================================================================
// Random numbers
// ================================================================================================
#if MC_COMPAT
// RANECU streams, one per batch: compat_math.inc
#else
// One independent stream per history: Philox4x32-7(key = seed, counter = history id, projection) seeds a lane generator.
// Lane generator: multiply-with-carry, base 2^32, lag 1 (Marsaglia; the multiplier 4294584393 is the MWC component of D. Jones'
// JKISS: a 2^32 - 1 and a 2^31 - 1 are both prime, period a 2^31 - 1 ~ 2^63).  x' = lo(a x + c), c' = hi(a x + c): ONE
// v_mad_u64_u32 per deviate.  Rounds 1-3 used xoshiro128+ (eight integer instructions per deviate, four words of state): about
// 16 deviates are drawn per history, a sixth of all the lane work of the kernel, and an integer instruction costs 1.5 fp32 ones on
// this part (profiles/r03v_imul_rate.txt) -- the change bought 6 % (Catphan), 9 % (CIRS), 3 % (thorax).  A history draws a few
// dozen deviates from a state seeded by Philox; only the 24 upper bits of x are used.  Against the bit-exact personality with
// 3.2e10 histories per mode the class energies and the block statistics are what they were with xoshiro
// (profiles/r03zz_fast_vs_compat_mwc.txt).
struct Rng { unsigned int x, c; };
#if defined(MC_RNG_PHILOX) && MC_RNG_PHILOX
// A/B yardstick, never the product (tools/rng_ab.py, tools/build_variant.sh): Philox4x32-10 evaluated PER DRAW -- a generator that
// passes BigCrush (Salmon et al., SC11) and has no state to correlate -- in place of the seeded multiply-with-carry.  The two state
// words hold the counter instead: x = draw number (16 bits) | projection (10 bits) << 16 | seed (6 bits) << 26, c = history id
// (32 bits: the experiment's launches stay below 2^32 histories, its seeds below 64).  The draw number wraps after 65536 draws: with
// 11 bits (the first version) one history in 1.6e10 -- a Compton event retrying shells at a nearly forward angle, acceptance ~1e-3 per
// trial -- found no accepted trial in its 2048-draw cycle and never ended.
__device__ __forceinline__ unsigned int rng_u32(Rng& r) {
  const unsigned int k = r.x & 65535u;
  unsigned int c0 = r.c, c1 = 0u, c2 = (r.x >> 16) & 1023u, c3 = k >> 2;
  unsigned int k0 = r.x >> 26, k1 = 0xCB435443u;
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const unsigned int hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned int hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  r.x = (r.x & ~65535u) | ((k + 1u) & 65535u);
  const unsigned int w = k & 3u;
  return w == 0u ? c0 : (w == 1u ? c1 : (w == 2u ? c2 : c3));
}
#else
__device__ __forceinline__ unsigned int rng_u32(Rng& r) {
  const unsigned long long t = 4294584393ULL * (unsigned long long)r.x + (unsigned long long)r.c;
  r.x = (unsigned int)t;
  r.c = (unsigned int)(t >> 32);
  return r.x;
}
#endif
// 24 upper bits -> k * 2^-24 + 2^-26, k = 0 .. 2^24 - 1: never 0, never 1 (the largest value rounds to 1 - 2^-24)
__device__ __forceinline__ float rng_f(Rng& r) { return fmaf((float)(rng_u32(r) >> 8), 5.9604644775390625e-08f, 1.4901161193847656e-08f); }
__device__ __forceinline__ double rng_d(Rng& r) { return ((double)rng_u32(r) + 0.5) * 2.3283064365386963e-10; }

// Philox4x32-7: the smallest member of the family that passes BigCrush (Salmon et al., "Parallel random numbers: as easy
// as 1, 2, 3", SC11, table 2); it only seeds the lane generator, one call per history
constexpr int kPhiloxRounds = 7;
__device__ void rng_init_history(Rng& r, unsigned long long hist, unsigned int seed, unsigned int stream_key) {
#if defined(MC_RNG_PHILOX) && MC_RNG_PHILOX
  r.x = ((stream_key & 1023u) << 16) | ((seed & 63u) << 26);
  r.c = (unsigned int)hist;
  return;
#endif
  unsigned int c0 = (unsigned int)hist, c1 = (unsigned int)(hist >> 32), c2 = stream_key, c3 = 0x4d43475u;
  unsigned int k0 = seed, k1 = 0xCB435443u;
  // the round keys are scalar additions: computed here every time (the compiler otherwise hoists all of them out of the
  // kernel's main loop, runs out of scalar registers and fetches them back with one v_readlane each)
  asm volatile("" : "+s"(k0));
  // both halves of a round's two products come from ONE v_mad_u64_u32 each (14 multiplies per history instead of 28: a
  // v_mul_hi_u32 + v_mul_lo_u32 pair costs 5.1 fp32 instructions' issue time on this part, the 64-bit multiply-add 3.5 --
  // profiles/r06b_mad64_rate.txt)
#pragma unroll
  for (int i = 0; i < kPhiloxRounds; ++i) {
    const unsigned long long p0 = (unsigned long long)c0 * 0xD2511F53ULL, p1 = (unsigned long long)c2 * 0xCD9E8D57ULL;
    const unsigned int hi0 = (unsigned int)(p0 >> 32), lo0 = (unsigned int)p0, hi1 = (unsigned int)(p1 >> 32), lo1 = (unsigned int)p1;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  r.x = c0 ^ c2;
  // umulhi(w, a - 1) <= a - 2 for every 32-bit w, so 1 <= c <= a - 1 ... and c = a - 1 is reached only by w = 2^32 - 1 with
  // umulhi = a - 2: the fixed points of the step, (0, 0) and (2^32 - 1, a - 1), need c = 0 or BOTH x = 2^32 - 1 and c = a - 1;
  // the second is excluded below (one compare, once per history; tests/test_fast_rng.py states the arithmetic)
  r.c = __umulhi(c1 ^ c3, 4294584392u) + 1u;
  if (r.x == 0xFFFFFFFFu && r.c == 4294584392u) r.c -= 1u;
}
#endif

// ================================================================================================
// Geometry helpers
// ================================================================================================
// distance to the entry plane of one axis (move_to_bbox, K.cu:719-777)
__device__ __forceinline__ float entry_dist(float p, float d, float size) {
  if (d > kEps) return (p > 0.0f) ? 0.0f : kEps + MC_DIV(-p, d);
  if (d < -kEps) return (p < size) ? 0.0f : kEps + MC_DIV(size - p, d);
  return -500000.0f;
}

struct Particle {
  float x, y, z, u, v, w, E;
};

// K.cu:1033-1065.  Returns the linear voxel index or -1 outside the (EPS-shrunk) bounding box.
__device__ __forceinline__ long locate_voxel(const TrackArgs& A, const Particle& P) {
  if ((P.y < kEps) || (P.y > (SARG(A, bbox)[1] - kEps)) || (P.x < kEps) || (P.x > (SARG(A, bbox)[0] - kEps)) || (P.z < kEps) ||
      (P.z > (SARG(A, bbox)[2] - kEps)))
    return -1;
  const int ix = (int)(P.x * A.inv_vs[0]);
  const int iy = (int)(P.y * A.inv_vs[1]);
  const int iz = (int)(P.z * A.inv_vs[2]);
  return (long)ix + (long)iy * A.nx + (long)iz * A.nxy;
}

// ================================================================================================
// rotate_double (K.cu:1103-1148)
// ================================================================================================
#if MC_COMPAT
__device__ void rotate_dir(Particle& P, double costh, double phi) {
  double DXY, NORM, cosphi, sinphi, SDT;
  DXY = (double)(P.u * P.u + P.v * P.v);  // float arithmetic then widened, as the reference expression evaluates
  pm_sincos(phi, sinphi, cosphi);
  NORM = DXY + (double)(P.w * P.w);
  if (fabs(NORM - 1.0) > 1.0e-14) {
    NORM = 1.0 / sqrt(NORM);
    P.u = (float)(NORM * (double)P.u);
    P.v = (float)(NORM * (double)P.v);
    P.w = (float)(NORM * (double)P.w);
    DXY = (double)(P.u * P.u + P.v * P.v);
  }
  if (DXY > 1.0e-28) {
    SDT = sqrt((1.0 - costh * costh) / DXY);
    const float xin = P.u;
    P.u = (float)((double)P.u * costh + SDT * ((double)(xin * P.w) * cosphi - (double)P.v * sinphi));
    P.v = (float)((double)P.v * costh + SDT * ((double)(P.v * P.w) * cosphi + (double)xin * sinphi));
    P.w = (float)((double)P.w * costh - DXY * SDT * cosphi);
  } else {
    SDT = sqrt(1.0 - costh * costh);
    P.v = (float)(SDT * sinphi);
    if (P.w > 0.0f) { P.u = (float)(SDT * cosphi); P.w = (float)costh; }
    else { P.u = (float)(-SDT * cosphi); P.w = (float)(-costh); }
  }
}
#else
// FAST comes in two arithmetics (MC_FAST_F64, one translation unit each: track_fast.hip / track_fast64.hip):
//   0  single precision throughout: the polar angle travels as omc = 1 - cos(theta), azimuth as a turn fraction (v_sin / v_cos);
//   1  the three sub-steps the reference computes in DOUBLE are in double here too -- rotate_double (K.cu:1103-1148), GRAa
//      (K.cu:1181-1246), GCOa's cdt1 / costh chain (K.cu:1329-1331, :1372, :1427-1435) -- with 32-bit deviates where the
//      reference calls ranecu_double.  Everything else (v_log / v_exp, the float chain of GCOa) is what the reference's GPU build
//      (-use_fast_math) computes in float as well.
#ifndef MC_FAST_F64
#define MC_FAST_F64 0
#endif
#ifndef MC_TALLY_W2
#define MC_TALLY_W2 0  // FAST: 1 in the instantiations that launches with a w2 run (tally_score)
#endif
#ifndef MC_STATS
#define MC_STATS 0  // FAST: 1 in the diagnostic build (track_stats.hip)
#endif
#if MC_FAST_F64
typedef double polar_t;  // cos(theta), as the reference carries it
// sin and cos of phi = 2 pi xi, xi = (u + 1/2) 2^-32 (rng_d), in double: the quarter turn nearest to xi is taken off in integer
// arithmetic (exact), the remainder |r| <= 1/8 turn goes through the Taylor polynomials of sin / cos on |x| <= pi/4 (to x^15 and x^16: truncation
// below 5e-17; the one rounding that matters is x = 2 pi r, as in the reference's 6.2831...*ranecu_double()).  The library's
// sincos() carries a Payne-Hanek reduction for arguments this call never sees and 30 vector registers this kernel does not have.
// A double constant assembled from two scalar words where it is used: v_fma_f64 takes no 64-bit literal, and constants left to the
// compiler are hoisted out of the persistent loop into vector registers the kernel does not have (35 spilled dwords, measured)
__device__ __forceinline__ double sconst(unsigned int lo, unsigned int hi) {
  asm volatile("" : "+s"(lo), "+s"(hi));
  return __hiloint2double((int)hi, (int)lo);
}
__device__ __forceinline__ void sincos_turn(unsigned int u, double& sinphi, double& cosphi) {
  const unsigned int k = (u + 0x20000000u) >> 30;              // nearest quarter turn, 0..4
  const int ri = (int)(u - (k << 30));                          // xi - k/4 in units of 2^-32 turn (wraps correctly for k = 4)
  const double x = ((double)ri + 0.5) * sconst(0x54442d18u, 0x3e1921fbu) /* 2 pi 2^-32 */;
  const double z = x * x;
  double sp = sconst(0xe733b81fu, 0xbd6ae7f3u) /* -7.64716373181981641e-13 */;  // -1/15!  (Taylor: x^17 / 17! < 5e-17 at pi/4)
  sp = fma(sp, z, sconst(0x13a86d09u, 0x3de61246u) /* 1.60590438368216133e-10 */);  // 1/13!
  sp = fma(sp, z, sconst(0x67f544e4u, 0xbe5ae645u) /* -2.50521083854417202e-08 */);  // -1/11!
  sp = fma(sp, z, sconst(0xa556c734u, 0x3ec71de3u) /* 2.75573192239858925e-06 */);  // 1/9!
  sp = fma(sp, z, sconst(0x1a01a01au, 0xbf2a01a0u) /* -1.98412698412698413e-04 */);  // -1/7!
  sp = fma(sp, z, sconst(0x11111111u, 0x3f811111u) /* 8.33333333333333322e-03 */);  // 1/5!
  sp = fma(sp, z, sconst(0x55555555u, 0xbfc55555u) /* -1.66666666666666657e-01 */);  // -1/3!
  const double s = fma(x * z, sp, x);
  double cp = sconst(0xe733b81fu, 0x3d2ae7f3u) /* 4.77947733238738525e-14 */;  // 1/16!  (x^18 / 18! < 3e-18 at pi/4)
  cp = fma(cp, z, sconst(0xa8c07c9du, 0xbda93974u) /* -1.14707455977297245e-11 */);  // -1/14!
  cp = fma(cp, z, sconst(0xeff8d898u, 0x3e21eed8u) /* 2.08767569878681002e-09 */);  // 1/12!
  cp = fma(cp, z, sconst(0xb7789f5cu, 0xbe927e4fu) /* -2.75573192239858883e-07 */);  // -1/10!
  cp = fma(cp, z, sconst(0x1a01a01au, 0x3efa01a0u) /* 2.48015873015873016e-05 */);  // 1/8!
  cp = fma(cp, z, sconst(0x16c16c17u, 0xbf56c16cu) /* -1.38888888888888894e-03 */);  // -1/6!
  cp = fma(cp, z, sconst(0x55555555u, 0x3fa55555u) /* 4.16666666666666644e-02 */);  // 1/4!
  cp = fma(cp, z, -0.5);
  const double c = fma(cp, z, 1.0);
  // quarter turns: (sin, cos)(x + k pi/2) = (s, c), (c, -s), (-s, -c), (-c, s)
  const bool odd = (k & 1u) != 0u;
  const double ss = odd ? c : s, cc = odd ? s : c;
  sinphi = (k & 2u) ? -ss : ss;
  cosphi = (((k + 1u) & 2u) != 0u) ? -cc : cc;
}
// Double-precision 1 / sqrt(x) and sqrt(a / b) from ONE v_rsq_f64 each (a 2^-26-ish estimate) and two Newton steps (relative error
// below 2^-51): the reference's CUDA build rounds its double division and square root correctly, these differ from that by at most
// two units in the last place of a DOUBLE -- 2e-16, in quantities whose next use rounds them to float (6e-8).  The correctly rounded
// sequences cost 25 instructions where these take 7 and 11 (profiles/r06j_*: the same class energies, a third of fast64's extra time).
__device__ __forceinline__ double rsqrt_d(double x) {
  double y = __builtin_amdgcn_rsq(x);
  y = y * fma(-0.5 * x * y, y, 1.5);
  y = y * fma(-0.5 * x * y, y, 1.5);
  return y;
}
__device__ __forceinline__ double sqrt_ratio_d(double a, double b) {  // sqrt(a / b) for a >= 0, b > 0: a / sqrt(a b)
  const double r = a * rsqrt_d(a * b);
  return a > 0.0 ? r : 0.0;
}
// K.cu:1103-1148 statement for statement (division and square roots as above)
__device__ __forceinline__ void rotate_dir(Particle& P, double costh, Rng& rng) {
  double DXY, NORM, cosphi, sinphi, SDT;
  DXY = (double)(P.u * P.u + P.v * P.v);  // a float expression in the reference, widened on assignment
  sincos_turn(rng_u32(rng), sinphi, cosphi);
  NORM = DXY + (double)(P.w * P.w);
  if (fabs(NORM - 1.0) > 1.0e-14) {
    NORM = rsqrt_d(NORM);
    P.u = (float)(NORM * (double)P.u);
    P.v = (float)(NORM * (double)P.v);
    P.w = (float)(NORM * (double)P.w);
    DXY = (double)(P.u * P.u + P.v * P.v);
  }
  if (DXY > 1.0e-28) {
    SDT = sqrt_ratio_d(fma(-costh, costh, 1.0), DXY);
    const float xin = P.u;
    P.u = (float)((double)P.u * costh + SDT * ((double)(xin * P.w) * cosphi - (double)P.v * sinphi));
    P.v = (float)((double)P.v * costh + SDT * ((double)(P.v * P.w) * cosphi + (double)xin * sinphi));
    P.w = (float)((double)P.w * costh - DXY * SDT * cosphi);
  } else {
    SDT = sqrt_ratio_d(fma(-costh, costh, 1.0), 1.0);
    P.v = (float)(SDT * sinphi);
    if (P.w > 0.0f) { P.u = (float)(SDT * cosphi); P.w = (float)costh; }
    else { P.u = (float)(-SDT * cosphi); P.w = (float)(-costh); }
  }
}
#else
typedef float polar_t;   // 1 - cos(theta)
// single precision; the polar angle arrives as omc = 1 - cos(theta), which keeps full relative precision for the
// forward-peaked angles (sin^2 = omc (2 - omc) exactly representable); azimuth from the turn fraction
// (v_sin_f32 / v_cos_f32 take revolutions)
__device__ __forceinline__ void rotate_dir(Particle& P, float omc, Rng& rng) {
  const float turn = rng_f(rng);
  const float sinphi = __builtin_amdgcn_sinf(turn), cosphi = __builtin_amdgcn_cosf(turn);
  const float costh = 1.0f - omc;
  float dxy = P.u * P.u + P.v * P.v;
  const float inv = __builtin_amdgcn_rsqf(dxy + P.w * P.w);
  P.u *= inv; P.v *= inv; P.w *= inv;
  dxy = P.u * P.u + P.v * P.v;
  const float st2 = fmaxf(omc * (2.0f - omc), 0.0f);
  // one square root serves both cases (the argument is selected, not the result: same bits, one transcendental fewer)
  // The reference's switch (K.cu:1127).  A float keeps the relative precision of u and v down to its smallest normal number, and
  // 1 / dxy <= 1e28 stays in range: the tilted formulas are as exact for a direction 1e-14 off the z axis as for any other.  With
  // the switch at 1e-12, where it first sat, a direction within 1e-6 of the axis was turned about the x axis instead of about its own
  // transverse axes -- the azimuth of the result off by the azimuth of (u, v), harmless to every tally (the azimuth is uniform) and
  // wrong against the rotation this function states (tests/test_scatter_gpu.py: test_rotate_f32_against_float64).
  const bool tilted = dxy > 1.0e-28f;
  const float sdt = __builtin_amdgcn_sqrtf(tilted ? st2 * __builtin_amdgcn_rcpf(dxy) : st2);
  if (tilted) {
    const float xin = P.u, yin = P.v;
    P.u = xin * costh + sdt * (xin * P.w * cosphi - yin * sinphi);
    P.v = yin * costh + sdt * (yin * P.w * cosphi + xin * sinphi);
    P.w = P.w * costh - dxy * sdt * cosphi;
  } else {
    P.v = sdt * sinphi;
    if (P.w > 0.0f) { P.u = sdt * cosphi; P.w = costh; }
    else { P.u = -sdt * cosphi; P.w = -costh; }
  }
}
#endif
#endif

// ================================================================================================
// GRAa (K.cu:1181-1246): Rayleigh polar angle (RITA inverse CDF of the squared form factor)
// ================================================================================================
#if !MC_COMPAT
// FAST: the same RITA inversion in single precision as ONE trial of the rejection loop (K.cu:1212-1270): true when the
// candidate is accepted, omc = 1 - cos(theta) (see rotate_dir).  A rejected lane stays in its phase and tries again in
// its wave's next Rayleigh batch (see compton_angle_trial for the reasoning); the random numbers consumed and the
// decisions taken per history are those of the loop.
#if MC_FAST_F64
// MC_FAST_F64: ONE trial of GRAa's loop in the reference's arithmetic (K.cu:1181-1246: double throughout, float table entries
// widened where the reference widens them), costh = cos(theta)
__device__ bool rayleigh_trial(const TrackArgs& A, float energy, int mc, float pmax_current, Rng& rng, double& costh) {
  const double xmax = ((double)energy) * 8.065535669099010e-5;
  const double xl = (double)as_global(COLD(A)->xco)[(mc + 1) * kRayleighPoints - 1];
  const double x2max = (xmax * xmax < xl) ? xmax * xmax : xl;
  if (xmax < 0.01) {
    do { costh = 1.0 - rng_d(rng) * 2.0; } while (rng_d(rng) > ((costh * costh + 1.0) * 0.5));
    return true;
  }
  const GLOBAL_AS float* pco = as_global(COLD(A)->pco) + mc * kRayleighPoints;
  const GLOBAL_AS float* xco = as_global(COLD(A)->xco) + mc * kRayleighPoints;
  const double ru = rng_d(rng) * (double)pmax_current;
  const int itn = (int)(ru * (kRayleighPoints - 1));
  int i = (int)as_global(COLD(A)->itl)[itn + mc * kRayleighPoints];
  int j = (int)as_global(COLD(A)->itu)[itn + mc * kRayleighPoints];
  while ((j - i) > 1) {
    const int k = (i + j) >> 1;
    if (ru > (double)pco[k - 1]) i = k; else j = k;
  }
  const int q = i - 1;
  const float p0 = pco[q], x0 = xco[q];
  const double rr = ru - (double)p0;
  double xx = (double)x0;
  if (rr > 1e-16) {
    const double d = (double)(pco[q + 1] - p0);
    const float a = as_global(COLD(A)->aco)[q + mc * kRayleighPoints], b = as_global(COLD(A)->bco)[q + mc * kRayleighPoints];
    xx = (double)x0 + (double)(a + 1.0f + b) * d * rr / (d * d + ((double)a * d + (double)b * rr) * rr) * (double)(xco[q + 1] - x0);
  }
  if (!(xx < x2max)) return false;
  costh = 1.0 - 2.0 * xx / x2max;
  return rng_d(rng) < ((costh * costh + 1.0) * 0.5);
}
#else
__device__ bool rayleigh_trial(const TrackArgs& A, float energy, int mc, float pmax_current, Rng& rng, float& omc) {
  const float xmax = energy * 8.065535669099010e-5f;
  const float xl = as_global(COLD(A)->xco)[(mc + 1) * kRayleighPoints - 1];
  const float x2max = fminf(xmax * xmax, xl);
  if (xmax < 0.01f) {
    float c;
    do { omc = rng_f(rng) * 2.0f; c = 1.0f - omc; } while (rng_f(rng) > ((c * c + 1.0f) * 0.5f));
    return true;
  }
  const GLOBAL_AS float* pco = as_global(COLD(A)->pco) + mc * kRayleighPoints;
  const GLOBAL_AS float* xco = as_global(COLD(A)->xco) + mc * kRayleighPoints;
  // The deviate of the table look-up is the whole 32-bit word, (w + 1/2) 2^-32 -- the value rng_d gives the double build -- carried as
  // two floats: hi = the 24 upper bits (exact), lo = the 8 lower ones and the half (exact).  GRAa inverts a distribution whose tail is
  // steep at the top of the tables: around ru = 0.9998 in water at 124.5 keV an interval of the table 1.1e-4 wide in ru spans 0.19 in
  // omc, so the 2^-24 grid of rng_f was a grid of 1e-4 .. 3.5e-4 in omc there, and rounding the product ru another 1e-4
  // (tests/test_scatter_gpu.py: test_rayleigh_replay, test_fast_and_fast64_take_the_same_decisions).  The search runs on the rounded
  // float ru as before; ru - p0 is then taken from the unrounded products -- one fused multiply-add and one multiply-add -- and where
  // that puts the point outside the interval the search chose (a table point within 2^-24 of ru) the interval moves with it.
  const unsigned int word = rng_u32(rng);
  const float hi = (float)(word >> 8) * 5.9604644775390625e-08f, lo = ((float)(word & 255u) + 0.5f) * 2.3283064365386963e-10f;
  const float ru = fmaf((float)(word >> 8), 5.9604644775390625e-08f, 1.4901161193847656e-08f) * pmax_current;  // rng_f's value
  const int itn = (int)(ru * (kRayleighPoints - 1));
  int i = (int)as_global(COLD(A)->itl)[itn + mc * kRayleighPoints];
  int j = (int)as_global(COLD(A)->itu)[itn + mc * kRayleighPoints];
  while ((j - i) > 1) {
    const int k = (i + j) >> 1;
    if (ru > pco[k - 1]) i = k; else j = k;
  }
  int q = i - 1;
  float p0 = pco[q], d = pco[q + 1] - p0;
  float rr = fmaf(hi, pmax_current, -p0) + lo * pmax_current;
  while (rr < 0.0f && q > 0) { --q; p0 = pco[q]; d = pco[q + 1] - p0; rr = fmaf(hi, pmax_current, -p0) + lo * pmax_current; }
  while (rr > d && q < kRayleighPoints - 2) { ++q; p0 = pco[q]; d = pco[q + 1] - p0; rr = fmaf(hi, pmax_current, -p0) + lo * pmax_current; }
  float xx = xco[q];
  if (rr > 1e-16f) {
    const float a = as_global(COLD(A)->aco)[q + mc * kRayleighPoints], b = as_global(COLD(A)->bco)[q + mc * kRayleighPoints];
    xx = xx + MC_DIV((a + 1.0f + b) * d * rr, d * d + (a * d + b * rr) * rr) * (xco[q + 1] - xx);
  }
  if (!(xx < x2max)) return false;
  omc = MC_DIV(2.0f * xx, x2max);
  const float c = 1.0f - omc;
  return rng_f(rng) < ((c * c + 1.0f) * 0.5f);
}
#endif
#endif
__device__ double sample_rayleigh(const TrackArgs& A, float energy, int mc, float pmax_current, Rng& rng) {
  double costh;
  const double xmax = ((double)energy) * 8.065535669099010e-5;
  const double xl = (double)as_global(COLD(A)->xco)[(mc + 1) * kRayleighPoints - 1];
  const double x2max = (xmax * xmax < xl) ? xmax * xmax : xl;
  if (xmax < 0.01) {
    do { costh = 1.0 - rng_d(rng) * 2.0; } while (rng_d(rng) > ((costh * costh + 1.0) * 0.5));
    return costh;
  }
  for (;;) {
    const double ru = rng_d(rng) * (double)pmax_current;
    const int itn = (int)(ru * (kRayleighPoints - 1));
    int i = (int)as_global(COLD(A)->itl)[itn + mc * kRayleighPoints];
    int j = (int)as_global(COLD(A)->itu)[itn + mc * kRayleighPoints];
    while ((j - i) > 1) {
      const int k = (i + j) >> 1;
      if (ru > (double)as_global(COLD(A)->pco)[k - 1 + mc * kRayleighPoints]) i = k; else j = k;
    }
    const int q = i - 1 + mc * kRayleighPoints;
    const double rr = ru - (double)as_global(COLD(A)->pco)[q];
    double xx;
    if (rr > 1e-16) {
      const double d = (double)(as_global(COLD(A)->pco)[q + 1] - as_global(COLD(A)->pco)[q]);
      const float a = as_global(COLD(A)->aco)[q], b = as_global(COLD(A)->bco)[q], x0 = as_global(COLD(A)->xco)[q];
      xx = (double)x0 + (double)(a + 1.0f + b) * d * rr / (d * d + ((double)a * d + (double)b * rr) * rr) * (double)(as_global(COLD(A)->xco)[q + 1] - x0);
    } else {
      xx = (double)as_global(COLD(A)->xco)[q];
    }
    if (xx < x2max) {
      costh = 1.0 - 2.0 * xx / x2max;
      if (rng_d(rng) < ((costh * costh + 1.0) * 0.5)) break;
    }
  }
  return costh;
}

// ================================================================================================
// GCOa (K.cu:1287-1515): Compton scattering, impulse approximation with analytical one-electron profiles.
// The reference keeps the per-shell profile integrals of the accepted trial in a 40-float local array
// (K.cu:1290); here they are recomputed on demand (same expression => same bits), which keeps the array
// out of the register file / scratch.
// ================================================================================================
__device__ __forceinline__ float shell_pz(float fj0, float aux, float u) {
#if MC_COMPAT
  return cm_divf(fj0 * (aux - u * 510998.918f), cm_sqrtf(aux + aux + u * u) * 510998.918f);  // == fj0 * (..) / (sqrtf(..) * mc2), compat_math.inc
#else
  return fj0 * (aux - u * 510998.918f) * __builtin_amdgcn_rsqf(aux + aux + u * u) * 1.956951306108245e-6f;
#endif
}
// profile integral n_i at cos-deflection cdt (K.cu:1361-1400); 0 for shells that cannot be ionised
// Compton shells in LDS, material after material: float4 {U_i, J_i, f_i, 0} at index `first shell of the material` + i
// ({U, J} come with one 8-byte read); LDS_I(nosc)[mc] = number of shells, LDS_I(nosc)[nmat + mc] = first shell
__device__ __forceinline__ float2 shell_uj(const TrackArgs& A, int base, int i) {
  return reinterpret_cast<const float2*>(lds_raw + SLDS(A, shells))[2 * (base + i)];
}
__device__ __forceinline__ float shell_f(const TrackArgs& A, int base, int i) { return LDS_F(SLDS(A, shells))[4 * (base + i) + 2]; }
__device__ __forceinline__ float shell_profile(const float2 r, float E, float cdtf) {
  float t = r.x;
  if (!(t < E)) return 0.0f;
  const float aux = E * (E - t) * cdtf;
  float pz;
  if ((aux > 1.0e-12f) || (t > 1.0e-12f)) pz = shell_pz(r.y, aux, t);
  else pz = 0.002f;
  t = pz * 1.4142135623731f;
  if (pz > 0.0f) t = 0.5f - (t + 0.70710678118654502f) * (t + 0.70710678118654502f);
  else t = 0.5f - (0.70710678118654502f - t) * (0.70710678118654502f - t);
  t = 0.5f * mc_expf(t);
  if (pz > 0.0f) t = 1.0f - t;
  return t;
}

#if MC_COMPAT
typedef double compton_angle_t;  // cos(theta)
#else
typedef float compton_angle_t;   // 1 - cos(theta) (see rotate_dir)
#endif
// diagnostic build: wave-level trips and lane-level trials of the two rejection loops (counters 16..19)
#if defined(MC_STATS) && MC_STATS
#define COMPTON_TRIP(slot)                                                                      \
  do {                                                                                          \
    const unsigned long long act_ = __ballot(1);                                                \
    if ((int)(threadIdx.x & 63) == __ffsll((long long)act_) - 1 && A.stats != nullptr) {        \
      atomicAdd(A.stats + (slot), 1ULL);                                                        \
      atomicAdd(A.stats + (slot) + 1, (unsigned long long)__popcll(act_));                      \
    }                                                                                           \
  } while (0)
#else
#define COMPTON_TRIP(slot)
#endif
#if MC_COMPAT
// COMPAT personality: GCOa (K.cu:1287-1515) in the reference's own arithmetic, cut at its two rejection loops into three
// resumable pieces:
//   compton_angle_trial  ONE trial of the polar-angle loop (K.cu:1316-1372: tau, S(theta), the test); the event's first trial
//                        also computes the normalisation S0 = sum_i f_i n_i(theta = pi) (K.cu:1300-1314) in the same pass
//   compton_shell_trial  ONE trial of the shell + electron-momentum loop (K.cu:1374-1480) and the photon's new energy
// A history draws exactly the random numbers of the reference's nested loops, in their order -- which lane-mates' trials run
// beside it makes no difference to its RANECU stream -- so the tallies are those of the monolithic function bit for bit.
// What changes is the schedule: in the nested form a wave stayed in the angle loop until its LAST lane had accepted and in the
// momentum loop likewise, every iteration a pass over 29-40 shells for a handful of lanes (PMC on the thorax workload: 23 % lane
// utilisation).  Now a rejected lane keeps its sub-state (s0, tau, S) and takes part in the wave's next Compton batch.
// cos-deflection of an accepted tau (K.cu:1329-1331); a pure function of (tau, E), so it is not carried between the trials
__device__ __forceinline__ double compton_cdt1(float tau, float E) {
  double cdt1 = (double)(1.f - tau) / (((double)tau) * ((double)E) * 1.956951306108245e-6);
  if (cdt1 > 2.0) cdt1 = 1.99999999;
  return cdt1;
}
// One trial of the polar angle: tau, s = S(E, theta) of that angle, the verdict of the rejection test.  `s0` is the event's S0 if an
// earlier trial had to compute it (compton_s0; it takes no random number, so when it is computed does not matter to the history's
// stream), or negative (unknown).
// `ck`: the partial sums of S after every kShellStride-th shell of this trial -- where compton_shell_trial may resume the
// cumulative selection instead of walking the shells again from the first one (same adds in the same order from the same partial
// sum: the same bits).
constexpr int kShellStride = 4;
constexpr int kShellMarks = (kMaxShells + kShellStride - 1) / kShellStride;
static_assert(kShellMarks <= 10, "compton_angle_trial spells out ck[0..9]: add cases to its switch before raising kMaxShells / lowering kShellStride");
// The test itself (K.cu:1367-1372: xi S0 > S T(tau) rejects) comes in two forms.  With the exact S0 (`need_s0`, or the value an
// earlier trial of the event computed) the verdict is the reference's.  Without it the kernel asks the rigorous bounds
// lo <= S0 <= hi of TrackCold::s0_bounds (engine.cpp): float multiplication by xi >= 0 is monotonic, so "xi lo > rhs" implies the
// reference's rejection and "not (xi hi > rhs)" its acceptance; a xi in between leaves the test open: the caller computes S0
// (compton_s0) and applies the reference's test to the same xi and rhs.
enum ComptonVerdict : int { kAngleRejected = 0, kAngleAccepted = 1, kAngleOpen = -1 };
__device__ int compton_angle_trial(const TrackArgs& A, float E, int mc, float s0, Rng& rng, float& tau, float& s,
                                   float (&ck)[kShellMarks], float& xi, float& rhs) {
  const int nosc = LDS_I(SLDS(A, nosc))[mc];
  const int sb = LDS_I(SLDS(A, nosc))[A.nmat + mc];
  const float ek = E * 1.956951306108245e-6f;
  const float ek2 = ek * 2.f + 1.f;
  const float ek3 = ek * ek;
  const float taumin = MC_DIV(1.f, ek2);
  const float a1 = mc_logf(ek2);
  int bin = (int)((E - COLD(A)->s0_emin) * COLD(A)->s0_inv_w);
  bin = min(max(bin, 0), kS0Bins - 1);
  const float2 b = *reinterpret_cast<const float2*>(COLD(A)->s0_bounds + 2 * (mc * kS0Bins + bin));  // lo <= S0 <= hi
  const float s0_low = (s0 >= 0.0f) ? s0 : b.x;
  float num, den;
  // Trials that need no pass over the shells: S(theta) <= S0 for every angle (each profile grows with the momentum transfer), so
  // rhs = S T(tau) is at most hi T(tau), and a xi with xi S0 above THAT is the reference's rejection whatever S(theta) is -- the
  // Klein-Nishina part of the rejection function, a third of all trials.  They repeat right here, drawing what the reference's
  // loop draws (two numbers for tau, then xi; the pass in between draws nothing), until a trial survives.
  for (;;) {
    if ((double)rng_f(rng) * ((double)a1 + 2. * (double)ek * (double)(ek + 1.f) * (double)taumin * (double)taumin) < (double)a1)
      tau = mc_powf(taumin, rng_f(rng));
    else
      tau = mc_sqrtf(1.f + rng_f(rng) * (taumin * taumin - 1.f));
    xi = rng_f(rng);
    num = 1.0f + tau * ((ek3 - ek2 - 1.0f) + tau * (ek2 + tau * ek3));
    den = ek3 * tau * (tau * tau + 1.0f);
    if (!(num > 0.0f && (xi * s0_low) > MC_DIV(b.y * num, den))) break;
  }
  const float cdtf = (float)compton_cdt1(tau, E);
  s = 0.0f;
  for (int i = 0; i < nosc; i++) {
    s += shell_f(A, sb, i) * shell_profile(shell_uj(A, sb, i), E, cdtf);
    if ((i & (kShellStride - 1)) == kShellStride - 1) {  // i is the same number in every lane still in the loop: a scalar branch
      switch (i / kShellStride) {
        case 0: ck[0] = s; break;
        case 1: ck[1] = s; break;
        case 2: ck[2] = s; break;
        case 3: ck[3] = s; break;
        case 4: ck[4] = s; break;
        case 5: ck[5] = s; break;
        case 6: ck[6] = s; break;
        case 7: ck[7] = s; break;
        case 8: ck[8] = s; break;
        default: ck[9] = s; break;
      }
    }
  }
  rhs = MC_DIV(s * num, den);
  if (s0 >= 0.0f) return !((xi * s0) > rhs) ? kAngleAccepted : kAngleRejected;  // S0 known: the reference's test
  if ((xi * b.x) > rhs) return kAngleRejected;
  if (!((xi * b.y) > rhs)) return kAngleAccepted;
  return kAngleOpen;
}
// S0 = S(E, theta = pi) as the reference computes it at the head of every event (K.cu:1300-1314), term by term
__device__ float compton_s0(const TrackArgs& A, float E, int mc) {
  const int nosc = LDS_I(SLDS(A, nosc))[mc];
  const int sb = LDS_I(SLDS(A, nosc))[A.nmat + mc];
  float s0 = 0.0f;
  for (int i = 0; i < nosc; i++) {
    const float2 r = shell_uj(A, sb, i);
    float t = r.x;
    if (t < E) {
      const float aux = E * (E - t) * 2.f;
      const float pz = shell_pz(r.y, aux, t);
      if (pz > 0.0f) t = (0.707106781186545f + pz * 1.4142135623731f) * (0.707106781186545f + pz * 1.4142135623731f);
      else t = (0.707106781186545f - pz * 1.4142135623731f) * (0.707106781186545f - pz * 1.4142135623731f);
      t = 0.5f * mc_expf(0.5f - t);
      if (pz > 0.0f) t = 1.0f - t;
      s0 += shell_f(A, sb, i) * t;
    }
  }
  return s0;
}
// true: shell and momentum accepted; `energy` becomes the scattered photon's, costh the cosine of the polar angle
// `ck`: the partial sums of S(theta) the angle trial of THIS angle left behind.
__device__ bool compton_shell_trial(const TrackArgs& A, float& energy, int mc, float tau, float s, Rng& rng, double& costh,
                                    const float (&ck)[kShellMarks]) {
  const float E = energy;
  const int nosc = LDS_I(SLDS(A, nosc))[mc];
  const int sb = LDS_I(SLDS(A, nosc))[A.nmat + mc];
  const double cdt1 = compton_cdt1(tau, E);
  const float cdtf = (float)cdt1;
  costh = 1.0 - cdt1;
  float t = s * rng_f(rng);
  float pac = 0.0f;
  int ishell = nosc - 1;
  float rn_sel = 0.0f;
  bool found = false;
  // K.cu:1383-1392 looks for the first shell whose cumulative sum exceeds t.  The sums never decrease (f >= 0, profile >= 0), so
  // the marks at or below t are a prefix: the walk starts behind the last of them, with its sum.
  int first = 0;
  bool prefix = true;
#pragma unroll
  for (int k = 0; k < kShellMarks; ++k) {
    prefix = prefix && (kShellStride * k + kShellStride - 1 < nosc) && !(ck[k] > t);
    if (prefix) { first = kShellStride * (k + 1); pac = ck[k]; }
  }
  for (int i = first; i < (nosc - 1); i++) {
    rn_sel = shell_profile(shell_uj(A, sb, i), E, cdtf);
    pac += shell_f(A, sb, i) * rn_sel;
    if (pac > t) { ishell = i; found = true; break; }
  }
  if (!found) rn_sel = shell_profile(shell_uj(A, sb, nosc - 1), E, cdtf);
  t = rng_f(rng) * rn_sel;
  const float fj = shell_uj(A, sb, ishell).y * 1.4142135623731f;
  float pzomc;
  if (t < 0.5f) pzomc = MC_DIV(0.70710678118654502f - mc_sqrtf(0.5f - mc_logf(t + t)), fj);
  else pzomc = MC_DIV(mc_sqrtf(0.5f - mc_logf(2.0f - 2.0f * t)) - 0.70710678118654502f, fj);
  if (pzomc < -1.0f) return false;
  t = (float)((double)tau * ((double)tau - costh * 2.0) + 1.0);
  float af;
  if (t > 1.0e-20f) af = mc_sqrtf(t) * (MC_DIV(tau * (tau - ((float)costh)), t) + 1.f);
  else af = 0.00200f;
  if (af > 0.0f) t = af * 0.2f + 1.f; else t = 1.f - af * 0.2f;
  float pzc = (pzomc < 0.2f) ? pzomc : 0.2f;
  pzc = (pzc > -0.2f) ? pzc : -0.2f;
  if (!(rng_f(rng) * t < (af * pzc + 1.f))) return false;
  t = pzomc * pzomc;
  const float b1 = 1.f - t * tau * tau;
  const float b2 = 1.f - t * tau * ((float)costh);
  float r = mc_sqrtf(fabsf(b2 * b2 - b1 * (1.0f - t)));
  if (pzomc < 0.0f) r *= -1.0f;
  t = MC_DIV(tau, b1) * (b2 + r);
  if (t > 1.0f) t = 1.0f;
  energy = E * t;
  return true;
}
#endif

#if !MC_COMPAT
// FAST personality: GCOa (K.cu:1287-1515) as single TRIALS with the shell drawn FIRST.
//
// The reference samples the polar angle by rejection against S(E, theta) = sum_i f_i n_i(E, theta) (one pass over the
// electron shells of the material per trial, K.cu:1316-1372), then the active shell from the cumulative f_i n_i (a second
// pass, K.cu:1374-1400) and the electron momentum; a rejected momentum goes back to the shell selection at the same angle
// (K.cu:1401-1480).  With tissue materials of 29-40 shells those passes are 70 % of the kernel.  The same joint law of
// (angle, shell) is sampled here without any pass:
//   * tau from the Klein-Nishina envelope exactly as the reference does (K.cu:1318-1327);
//   * a shell i with probability f_i / F (F = sum of all f: Walker alias table built by the host, one draw);
//   * accepted with probability T(tau) * n_i(E, tau), T <= 1 the reference's rejection function (K.cu:1367-1371) and
//     n_i <= 1 the profile integral of that ONE shell (0 for a shell that cannot be ionised).
// The accepted pair has density  envelope(tau) T(tau) f_i n_i(tau) / F: summed over i this is the reference's angular law
// envelope * T * S (its constant S0 = S(theta = pi) only scales the acceptance rate), and given tau the shell has
// probability f_i n_i / S -- the reference's cumulative selection.  A failed momentum trial parks the history as SHELL;
// its retry draws a shell with probability f_i / F and accepts it with probability n_i(tau): again f_i n_i / S.
// Both trials are O(1) in the number of shells, and a batch is one straight pass (no loops) for every lane:
//   lanes in COMPTON sample tau, lanes in SHELL bring theirs; all draw a shell, evaluate its profile, test, and the
//   accepted ones run the momentum trial (K.cu:1401-1480, unchanged).
// LDS shell table of this personality: float4 {U_i, J_i, alias cut-off, bits(alias shell)} (stage_tables).
struct ComptonTrial {
  float tau;   // E'/E of the free-electron kinematics
  float2 uj;   // {U, J} of the drawn shell
  float rn;    // n_i(E, tau) of the drawn shell
#if MC_FAST_F64
  double cdt1; // 1 - cos(theta) of the free-electron kinematics at tau, in double (K.cu:1329-1331)
#endif
};
#if MC_FAST_F64
// cos-deflection of a sampled tau (K.cu:1329-1331): the reference's expression in double; the quotient through a Newton-refined
// v_rcp_f64 and one residual correction (<= 1 ulp of double, see rsqrt_d)
__device__ __forceinline__ double compton_cdt1(float tau, float E) {
  const double num = (double)(1.f - tau), den = ((double)tau) * ((double)E) * sconst(0x5ba7c538u, 0x3ec06a85u) /* 1.956951306108245e-6 */;
  double y = __builtin_amdgcn_rcp(den);
  y = fma(fma(-den, y, 1.0), y, y);
  y = fma(fma(-den, y, 1.0), y, y);
  double cdt1 = num * y;
  cdt1 = fma(fma(-den, cdt1, num), y, cdt1);
  if (cdt1 > 2.0) cdt1 = sconst(0xfd50ce24u, 0x3fffffffu) /* 1.99999999 */;
  return cdt1;
}
#endif
// Draw tau (when `need_tau`) and a shell; true: the pair is accepted.
__device__ __forceinline__ bool compton_draw(const TrackArgs& A, float E, int mc, bool need_tau, Rng& rng, ComptonTrial& c) {
  const int nosc = LDS_I(SLDS(A, nosc))[mc];
  const int sb = LDS_I(SLDS(A, nosc))[A.nmat + mc];
  const float ek = E * 1.956951306108245e-6f;
  const float ek2 = ek * 2.f + 1.f;
  const float ek3 = ek * ek;
  float accept = 1.0f;  // T(tau); 1 for a retry at an angle that is already accepted
  if (need_tau) {
    const float taumin = MC_DIV(1.f, ek2);
    const float a1 = mc_logf(ek2);
    if (rng_f(rng) * (a1 + 2.f * ek * (ek + 1.f) * taumin * taumin) < a1) c.tau = mc_powf(taumin, rng_f(rng));
    else c.tau = mc_sqrtf(1.f + rng_f(rng) * (taumin * taumin - 1.f));
    const float tau = c.tau;
    accept = MC_DIV(1.0f + tau * ((ek3 - ek2 - 1.0f) + tau * (ek2 + tau * ek3)), ek3 * tau * (tau * tau + 1.0f));
  }
#if MC_FAST_F64
  c.cdt1 = compton_cdt1(c.tau, E);  // K.cu:1329-1331, in double; the profiles take it narrowed (K.cu:1340)
  const float cdtf = (float)c.cdt1;
#else
  const float cdtf = fminf(MC_DIV(1.f - c.tau, c.tau * ek), 1.99999988f);
#endif
  // alias draw from one 32-bit number: column = floor(u n / 2^32), position inside the column = the low word
  const unsigned int u = rng_u32(rng);
  const unsigned int col = __umulhi(u, (unsigned int)nosc);
  const float frac = (float)((u * (unsigned int)nosc) >> 8) * 5.9604644775390625e-08f;
  const float4 e = reinterpret_cast<const float4*>(lds_raw + SLDS(A, shells))[sb + (int)col];
  const int i = (frac < e.z) ? (int)col : __float_as_int(e.w);
  c.uj = shell_uj(A, sb, i);
  c.rn = shell_profile(c.uj, E, cdtf);
  return rng_f(rng) < accept * c.rn;
}
// Momentum trial of the drawn shell (K.cu:1401-1480).  true: accepted, `energy` is the scattered photon's energy and
// omc = 1 - cos(theta).
__device__ __forceinline__ bool compton_momentum_trial(float& energy, const ComptonTrial& c, Rng& rng, polar_t& angle) {
  const float E = energy, tau = c.tau;
#if MC_FAST_F64
  const double costh_d = 1.0 - c.cdt1;  // K.cu:1372
  const float costh = (float)costh_d;   // where the reference narrows it (K.cu:1435, :1468)
  angle = costh_d;
#else
  const float ek = E * 1.956951306108245e-6f;
  const float cdtf = fminf(MC_DIV(1.f - tau, tau * ek), 1.99999988f);
  const float costh = 1.0f - cdtf;
  angle = cdtf;
#endif
  float t = rng_f(rng) * c.rn;
  const float fj = c.uj.y * 1.4142135623731f;
  // K.cu:1418-1421: (0.7071 - sqrt(0.5 - ln 2t)) / fj below one half, (sqrt(0.5 - ln(2 - 2t)) - 0.7071) / fj above: ONE logarithm
  // and ONE square root of the selected argument (both sides used to be evaluated for every lane); same bits
  const bool lower = t < 0.5f;
  const float root = mc_sqrtf(0.5f - mc_logf(lower ? t + t : 2.0f - 2.0f * t));
  const float pzomc = MC_DIV(lower ? 0.70710678118654502f - root : root - 0.70710678118654502f, fj);
  if (pzomc < -1.0f) return false;
#if MC_FAST_F64
  t = (float)((double)tau * ((double)tau - costh_d * 2.0) + 1.0);  // K.cu:1427: costh is the double there
#else
  t = tau * (tau - costh * 2.f) + 1.f;
#endif
  float af;
  if (t > 1.0e-20f) af = mc_sqrtf(t) * (MC_DIV(tau * (tau - costh), t) + 1.f);
  else af = 0.00200f;
  if (af > 0.0f) t = af * 0.2f + 1.f; else t = 1.f - af * 0.2f;
  float pzc = (pzomc < 0.2f) ? pzomc : 0.2f;
  pzc = (pzc > -0.2f) ? pzc : -0.2f;
  if (!(rng_f(rng) * t < (af * pzc + 1.f))) return false;
  t = pzomc * pzomc;
  const float b1 = 1.f - t * tau * tau;
  const float b2 = 1.f - t * tau * costh;
  float r = mc_sqrtf(fabsf(b2 * b2 - b1 * (1.0f - t)));
  if (pzomc < 0.0f) r *= -1.0f;
  t = MC_DIV(tau, b1) * (b2 + r);
  if (t > 1.0f) t = 1.0f;
  energy = E * t;
  return true;
}
#endif

// ================================================================================================
// source (K.cu:626-686)
// ================================================================================================
__device__ __forceinline__ void sample_source_energy(const TrackArgs& A, Particle& P, Rng& rng);
__device__ __forceinline__ void sample_source_direction(const TrackArgs& A, Particle& P, Rng& rng);
__device__ __forceinline__ void move_to_bbox(const TrackArgs& A, Particle& P, bool& miss);
__device__ void sample_source(const TrackArgs& A, Particle& P, Rng& rng, bool& miss) {
  sample_source_energy(A, P, rng);
  sample_source_direction(A, P, rng);
  move_to_bbox(A, P, miss);
}
__device__ __forceinline__ void sample_source_energy(const TrackArgs& A, Particle& P, Rng& rng) {
  const float* const espc = LDS_F(SLDS(A, espc));
  const float RN = rng_f(rng) * A.nbins;
#if MC_COMPAT
  const int ip = (int)RN;
#else
  const int ip = __float2int_rd(RN);
#endif
  const float fr = RN - (float)ip;
  const int bin = (fr < LDS_F(SLDS(A, cutoff))[ip]) ? ip : (int)LDS_S(SLDS(A, alias))[ip];
  P.E = espc[bin] + rng_f(rng) * (espc[bin + 1] - espc[bin]);
}
// direction in the beam frame, rotated to the projection's pose; the photon starts at the focal spot
__device__ __forceinline__ void sample_source_direction(const TrackArgs& A, Particle& P, Rng& rng) {
  float dx, dy, dz;
  do {
    dz = SRC(A)->cos_theta_low + rng_f(rng) * SRC(A)->D_cos_theta;
    const float phi = SRC(A)->phi_low + rng_f(rng) * SRC(A)->D_phi;
    const float sth = mc_sqrtf(1.0f - dz * dz);
#if MC_COMPAT
    double sd, cd;
    pm_sincos((double)phi, sd, cd);
    const float sphi = (float)sd, cphi = (float)cd;
#else
    const float sphi = __sinf(phi), cphi = __cosf(phi);
#endif
    dy = sth * sphi;
    dx = sth * cphi;
  } while (fabsf(MC_DIV(dz, dy + 1.0e-7f)) > SRC(A)->max_height_at_y1cm);
#if !MC_COMPAT
  // keep dx / dy = cot(phi) inside the aperture the host computed in double (TrackCold::fan_ratio_*): the native sine / cosine
  // are good to ~1e-6, which at the half-fan beam edge -- a pixel boundary of the detector -- decides the column
  if (dy > 0.0f) dx = __builtin_amdgcn_fmed3f(dx, dy * COLD(A)->fan_ratio_lo, dy * COLD(A)->fan_ratio_hi);
#endif
  if (DET(A)->rotation_flag == 1) {
    const float tx = dx, ty = dy;
    dx = SRC(A)->rot_fan[0] * tx + SRC(A)->rot_fan[1] * ty + SRC(A)->rot_fan[2] * dz;
    dy = SRC(A)->rot_fan[3] * tx + SRC(A)->rot_fan[4] * ty + SRC(A)->rot_fan[5] * dz;
    dz = SRC(A)->rot_fan[6] * tx + SRC(A)->rot_fan[7] * ty + SRC(A)->rot_fan[8] * dz;
  }
  P.u = dx; P.v = dy; P.w = dz;
  P.x = SRC(A)->pos[0]; P.y = SRC(A)->pos[1]; P.z = SRC(A)->pos[2];
}
// move_to_bbox (K.cu:714-805)
__device__ __forceinline__ void move_to_bbox(const TrackArgs& A, Particle& P, bool& miss) {
  const float ey = entry_dist(P.y, P.v, SARG(A, bbox)[1]);
  const float ex = entry_dist(P.x, P.u, SARG(A, bbox)[0]);
  float ez = entry_dist(P.z, P.w, SARG(A, bbox)[2]);
  if ((ey > ex) && (ey > ez)) ez = ey;
  else if (ex > ez) ez = ex;
  P.x += ez * P.u; P.y += ez * P.v; P.z += ez * P.w;
  miss = false;
  if ((P.x < 0.0f) || (P.x > SARG(A, bbox)[0]) || (P.y < 0.0f) || (P.y > SARG(A, bbox)[1]) || (P.z < 0.0f) || (P.z > SARG(A, bbox)[2])) {
    P.x -= ez * P.u; P.y -= ez * P.v; P.z -= ez * P.w;
    miss = true;
  }
}

// ================================================================================================
// tally_image (K.cu:482-604)
// ================================================================================================
__device__ void tally_image(const TrackArgs& A, Particle P, int scatter_state) {
  float xd, zd;  // detector-frame coordinates relative to the lower corner, in pixels
  if (DET(A)->rotation_flag == 1) {
    const float cosang = P.u * SRC(A)->dir[0] + (P.v * SRC(A)->dir[1] + (P.w * SRC(A)->dir[2]));
    if (cosang < 0.025f) return;
    const float dist = MC_DIV((SRC(A)->dir[0] * (DET(A)->center[0] - P.x) + (SRC(A)->dir[1] * (DET(A)->center[1] - P.y) + (SRC(A)->dir[2] * (DET(A)->center[2] - P.z)))), cosang);
    P.x = P.x + dist * P.u;
    P.y = P.y + dist * P.v;
    P.z = P.z + dist * P.w;
    const float rx = DET(A)->rot_inv[0] * P.x + DET(A)->rot_inv[1] * P.y + DET(A)->rot_inv[2] * P.z;
    const float rz = DET(A)->rot_inv[6] * P.x + DET(A)->rot_inv[7] * P.y + DET(A)->rot_inv[8] * P.z;
    xd = (rx - DET(A)->corner_min[0]) * DET(A)->inv_pixel_size_X;
    zd = (rz - DET(A)->corner_min[2]) * DET(A)->inv_pixel_size_Z;
  } else {
    if (P.v < 0.0001f) return;
    const float dist = MC_DIV(DET(A)->center[1] - P.y, P.v);
    xd = (P.x + dist * P.u - DET(A)->corner_min[0]) * DET(A)->inv_pixel_size_X;
    zd = (P.z + dist * P.w - DET(A)->corner_min[2]) * DET(A)->inv_pixel_size_Z;
  }
#if MC_COMPAT
  // CPU-build index arithmetic in float (K.cu:556-563)
  const float px = (float)floor((double)xd);
  if ((px > -0.1f) && (px < ((float)DET(A)->nx - 0.1f))) {
    const float pz = (float)floor((double)zd);
    if ((pz > -0.1f) && (pz < ((float)DET(A)->nz - 0.1f))) {
      const int idx = (int)(((float)scatter_state) * (float)DET(A)->total_pixels + px + pz * (float)DET(A)->nx + 0.0001f);
      const unsigned long long w = (unsigned long long)(P.E * 100.0f + 0.5f);
      atomicAdd(A.image + idx, w);
      unsigned long long* const w2 = KARG(w2);
      if (w2 != nullptr) atomicAdd(w2 + idx, tally_w2_term(w));
    }
  }
#else
  const int px = __float2int_rd(xd);
  if ((px > -1) && (px < DET(A)->nx)) {
    const int pz = __float2int_rd(zd);
    if ((pz > -1) && (pz < DET(A)->nz)) {
      const size_t idx = (size_t)scatter_state * DET(A)->total_pixels + (size_t)px + (size_t)pz * DET(A)->nx;
      const unsigned long long w = (unsigned long long)__float2ull_rn(P.E * 100.0f);
      atomicAdd(A.image + idx, w);
      unsigned long long* const w2 = KARG(w2);
      if (w2 != nullptr) atomicAdd(w2 + idx, tally_w2_term(w));
    }
  }
#endif
}

#if !MC_COMPAT
// FAST: tally_image() in two halves.  tally_pixel() finds the word of the tally the photon scores in (-1: misses the
// detector); the caller issues the atomic add at the END of its service batch: a returnless atomic still occupies the
// in-order vector-memory counter, so every load waited for after it would also wait for the atomic's round trip.
__device__ __forceinline__ int tally_pixel(const TrackArgs& A, Particle P, int scatter_state) {
  // Straight-line code: every pose word is requested up front (one scalar-load round trip instead of one per nested
  // condition), the conditions of tally_image only select the result.  A photon that cannot reach the detector plane
  // (cosang < 0.025, K.cu:503) computes with a harmless divisor.
  float xd, zd;
  bool reaches;
  if (DET(A)->rotation_flag == 1) {
    const float cosang = P.u * SRC(A)->dir[0] + (P.v * SRC(A)->dir[1] + (P.w * SRC(A)->dir[2]));
    reaches = !(cosang < 0.025f);
    const float dist = MC_DIV((SRC(A)->dir[0] * (DET(A)->center[0] - P.x) + (SRC(A)->dir[1] * (DET(A)->center[1] - P.y) + (SRC(A)->dir[2] * (DET(A)->center[2] - P.z)))),
                              reaches ? cosang : 1.0f);
    P.x = P.x + dist * P.u;
    P.y = P.y + dist * P.v;
    P.z = P.z + dist * P.w;
    const float rx = DET(A)->rot_inv[0] * P.x + DET(A)->rot_inv[1] * P.y + DET(A)->rot_inv[2] * P.z;
    const float rz = DET(A)->rot_inv[6] * P.x + DET(A)->rot_inv[7] * P.y + DET(A)->rot_inv[8] * P.z;
    xd = (rx - DET(A)->corner_min[0]) * DET(A)->inv_pixel_size_X;
    zd = (rz - DET(A)->corner_min[2]) * DET(A)->inv_pixel_size_Z;
  } else {
    reaches = !(P.v < 0.0001f);
    const float dist = MC_DIV(DET(A)->center[1] - P.y, reaches ? P.v : 1.0f);
    xd = (P.x + dist * P.u - DET(A)->corner_min[0]) * DET(A)->inv_pixel_size_X;
    zd = (P.z + dist * P.w - DET(A)->corner_min[2]) * DET(A)->inv_pixel_size_Z;
  }
  const int px = __float2int_rd(xd), pz = __float2int_rd(zd);
  const int nx = DET(A)->nx, nz = DET(A)->nz, word = scatter_state * DET(A)->total_pixels + px + pz * nx;
  return (reaches && (px > -1) && (px < nx) && (pz > -1) && (pz < nz)) ? word : -1;
}
// FAST: score `value` in word `word` of the detector tally.  Staged (TrackArgs::stage, a wave-uniform launch argument): the hit takes
// the next slot of its bin in this workgroup's block -- an LDS returning add, which also settles lanes of one batch that hit the same
// bin -- and is written there with one plain 8-byte store; tally_fold.hip sums the blocks after the kernel.  A block that is full, or
// a launch without staging, takes the direct 64-bit add at the memory side: the image never depends on the capacity or the plan.
// In the instantiations with MC_TALLY_W2 (track_fast_w2.hip, track_fast64_w2.hip, the diagnostic build) that direct route also adds
// the hit's squared weight to TrackArgs::w2 (wave-uniform, null = off); a staged hit needs nothing here: the fold takes the square
// from the same record.  The production instantiations carry no trace of it: the test alone cost the CIRS workload, whose every hit
// takes the direct route, 0.2 % (profiles/tally_variance_ab.md).
__device__ __forceinline__ void tally_score(const TrackArgs& A, int word, unsigned int value) {
  unsigned long long* const region = LARG(A, stage.region);
  if (region != nullptr) {
    const unsigned int n_bins = LARG(A, stage.n_bins), cap = LARG(A, stage.cap);
    unsigned int bin, rel;
    stage_map((unsigned int)word, LARG(A, stage.pixels), n_bins, LARG(A, stage.magic), LARG(A, stage.bin_pixels), bin, rel);
    unsigned int* const cursor = reinterpret_cast<unsigned int*>(lds_raw + LARG(A, stage.cursor));
    const unsigned int slot = atomicAdd(cursor + bin, 1u);
    if (slot < cap) {
      ((GLOBAL_AS unsigned long long*)region)[(unsigned long long)(blockIdx.x * n_bins + bin) * cap + slot] = ((unsigned long long)rel << 32) | value;
      return;
    }
    atomicAdd(cursor + n_bins, 1u);  // hits of this workgroup that fell back
  }
  atomicAdd((unsigned long long*)as_global(LARG(A, image)) + (unsigned int)word, (unsigned long long)value);
#if MC_TALLY_W2
  unsigned long long* const w2 = KARG(w2);
  if (w2 != nullptr) atomicAdd((unsigned long long*)as_global(w2) + (unsigned int)word, tally_w2_term(value));
#endif
}
// every thread of the workgroup calls these once: before stage_tables() (whose barrier publishes the zeros) / after its history loop,
// behind the barrier of finish_workgroup()
__device__ __forceinline__ void stage_cursors_clear(const TrackArgs& A) {
  if (A.stage.region == nullptr) return;
  unsigned int* const cursor = reinterpret_cast<unsigned int*>(lds_raw + A.stage.cursor);
  for (unsigned int i = threadIdx.x; i <= A.stage.n_bins; i += blockDim.x) cursor[i] = 0u;
}
__device__ __forceinline__ void stage_counts_publish(const TrackArgs& A) {
  const unsigned int n_bins = LARG(A, stage.n_bins), cap = LARG(A, stage.cap);
  const unsigned int* const cursor = reinterpret_cast<const unsigned int*>(lds_raw + LARG(A, stage.cursor));
  unsigned int* const counts = LARG(A, stage.counts) + blockIdx.x * n_bins;
  for (unsigned int i = threadIdx.x; i < n_bins; i += blockDim.x) counts[i] = min(cursor[i], cap);
  if (threadIdx.x == 0 && cursor[n_bins] != 0u) atomicAdd(LARG(A, stage.fallback), (unsigned long long)cursor[n_bins]);
}
#endif

__device__ __forceinline__ int energy_index(const TrackArgs& A, float E) {
#if MC_COMPAT
  return (int)((E - SARG(A, e0)) * SARG(A, ide) + 0.00001f);
#else
  return __float2int_rd((E - SARG(A, e0)) * SARG(A, ide));
#endif
}

// ================================================================================================
// Dose tallies (tally_materials_dose K.cu:1547-1563, tally_voxel_energy_deposition K.cu:418-443) for an
// energy deposit `edep` [eV] at position P in compact material mc.  Material dose goes to per-workgroup LDS
// accumulators (25 counters hit by every lane would serialise in memory); flush_dose() adds them at kernel end.
// ================================================================================================
__device__ __forceinline__ unsigned long long dose_round(float v) {
#if MC_COMPAT
  return (unsigned long long)(v + 0.5f);  // CPU build (K.cu:438-439, :1558-1559)
#else
  return (unsigned long long)__float2ull_rn(v);  // GPU build (K.cu:435-436, :1555-1556)
#endif
}
__device__ void tally_dose(const TrackArgs& A, const Particle& P, float edep, int mc) {
  const unsigned long long e1 = dose_round(edep * 100.0f), e2 = dose_round(edep * edep);
  if (A.dose_flags & kDoseMaterials) {
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(lds_raw + SLDS(A, dose_mat)) + 2 * COLD(A)->material_of_compact[mc];
    atomicAdd(acc, e1);
    atomicAdd(acc + 1, e2);
  }
  if (A.dose_flags & kDoseVoxels) {
    const CONST_AS int* roi = COLD(A)->dose_roi;
    const int ix = (int)(P.x * A.inv_vs[0]), iy = (int)(P.y * A.inv_vs[1]), iz = (int)(P.z * A.inv_vs[2]);
    if (ix >= roi[0] && ix <= roi[1] && iy >= roi[2] && iy <= roi[3] && iz >= roi[4] && iz <= roi[5]) {
      const int dx = roi[1] - roi[0] + 1, dy = roi[3] - roi[2] + 1;
      const size_t v = (size_t)(ix - roi[0]) + (size_t)(iy - roi[2]) * dx + (size_t)(iz - roi[4]) * dx * dy;
      unsigned long long* out = (unsigned long long*)as_global(COLD(A)->dose_voxels) + 2 * v;
      atomicAdd(out, e1);
      atomicAdd(out + 1, e2);
    }
  }
}
// every thread of the workgroup calls this once after its history loop
__device__ __forceinline__ void flush_dose(const TrackArgs& A) {
  if (!(A.dose_flags & kDoseMaterials)) return;
  __syncthreads();
  if (threadIdx.x < 2 * kMaxMaterials) {
    const unsigned long long v = reinterpret_cast<unsigned long long*>(lds_raw + SLDS(A, dose_mat))[threadIdx.x];
    if (v != 0ULL) atomicAdd((unsigned long long*)as_global(COLD(A)->dose_materials) + threadIdx.x, v);
  }
}

// ================================================================================================
// Voxel lookup: (density, compact material) of voxel (ix, iy, iz)
// ================================================================================================
template <int VK>
__device__ __forceinline__ void lookup_voxel(const TrackArgs& A, int ix, int iy, int iz, float& dens, int& mc) {
  if (VK == kVolU8) {
    // 4-bit brick grid in LDS: code < 15 = homogeneous brick, answered from the first 16 palette slots
    const int b = (ix >> A.brick_shift) + (iy >> A.brick_shift) * A.brick_nx + (iz >> A.brick_shift) * A.brick_nxy;
    int e = ((int)(lds_raw + A.lds.brick)[b >> 1] >> ((b & 1) << 2)) & 0xF;
    if (e == kBrickMixed) e = kPaletteBase + (int)((const unsigned char*)A.vol)[tiled_voxel((unsigned int)ix, (unsigned int)iy, (unsigned int)iz, (unsigned int)A.sub_nx, (unsigned int)A.sub_nxy)];
    const float2 pd = LDS_F2(A.lds.pal)[e];
    dens = pd.x;
    mc = __float_as_int(pd.y);
  } else if (VK == kVolU16) {
    const int pi = (int)((const unsigned short*)A.vol)[(long)ix + (long)iy * A.nx + (long)iz * A.nxy];
    const float2 pd = ((const float2*)A.palette)[pi];
    dens = pd.x;
    mc = __float_as_int(pd.y);
  } else {
    const float2 pd = ((const float2*)A.vol)[(long)ix + (long)iy * A.nx + (long)iz * A.nxy];
    dens = pd.x;
    mc = __float_as_int(pd.y);
  }
}

// ================================================================================================
// Stage the small tables in LDS (layout TrackArgs::lds); ends with a workgroup barrier
// ================================================================================================
template <int VK>
__device__ __forceinline__ void stage_tables(const TrackArgs& A) {
  const int nmat = A.nmat;
  // cold->fco/uico/fj0 are [shell * nmat + material] (kMaxShells rows); cold->shell_first[material] = prefix sum of noscco
  for (int i = threadIdx.x; i < kMaxShells * nmat; i += (int)blockDim.x) {
    const int shell = i / nmat, m = i - shell * nmat;
    if (shell < as_global(COLD(A)->noscco)[m])
      reinterpret_cast<float4*>(lds_raw + SLDS(A, shells))[COLD(A)->shell_first[m] + shell] =
#if MC_COMPAT
          make_float4(as_global(COLD(A)->uico)[i], as_global(COLD(A)->fj0)[i], as_global(COLD(A)->fco)[i], 0.f);
#else
          // FAST: the shell is drawn from a Walker alias table of the f_i (compton_draw)
          make_float4(as_global(COLD(A)->uico)[i], as_global(COLD(A)->fj0)[i], as_global(COLD(A)->shell_cut)[i],
                      __int_as_float((int)as_global(COLD(A)->shell_alias)[i]));
#endif
  }
  for (int i = threadIdx.x; i < nmat; i += (int)blockDim.x) LDS_I(SLDS(A, nosc))[nmat + i] = COLD(A)->shell_first[i];
  for (int i = threadIdx.x; i < nmat; i += (int)blockDim.x) LDS_I(SLDS(A, nosc))[i] = as_global(COLD(A)->noscco)[i];
  // nbins + 1 entries each: espc[nbins] is the upper edge of the last bin (K.cu:640 reads espc[bin + 1]); the extra
  // cutoff/alias entry is only reachable by a RANECU draw of exactly 1.0f (DESIGN.md, deviation 4)
  const int ns = (A.nbins < kMaxSpectrumBins) ? A.nbins + 1 : kMaxSpectrumBins;
  for (int i = threadIdx.x; i < ns; i += (int)blockDim.x) {
    LDS_F(SLDS(A, espc))[i] = as_global(COLD(A)->espc)[i];
    LDS_F(SLDS(A, cutoff))[i] = as_global(COLD(A)->cutoff)[i];
    LDS_S(SLDS(A, alias))[i] = as_global(COLD(A)->alias)[i];
  }
  if (threadIdx.x == 0 && ns == A.nbins) LDS_F(SLDS(A, espc))[A.nbins] = as_global(COLD(A)->espc)[kMaxSpectrumBins - 1];
  if (VK == kVolU8) {
    for (int i = threadIdx.x; i < kPaletteBase + A.palette_size; i += (int)blockDim.x) {
      // slots 0..14: palette entry of brick code i; slots 16..: the palette itself
      const int src = (i < kPaletteBase) ? COLD(A)->brick_palette[i] : i - kPaletteBase;
      LDS_F2(A.lds.pal)[i] = ((const float2*)A.palette)[src];
    }
    for (int i = threadIdx.x; i < A.brick_bytes; i += (int)blockDim.x) (lds_raw + A.lds.brick)[i] = as_global(COLD(A)->bricks)[i];
  }
  if ((A.dose_flags & kDoseMaterials) && threadIdx.x < 2 * kMaxMaterials)
    reinterpret_cast<unsigned long long*>(lds_raw + SLDS(A, dose_mat))[threadIdx.x] = 0ULL;
#if !MC_COMPAT
  {  // Woodcock majorant per coarse energy bin (LdsLayout::wood)
    const int nw = (A.num_values + (1 << kWoodShift) - 1) >> kWoodShift;
    for (int i = threadIdx.x; i < nw; i += (int)blockDim.x) LDS_F(SLDS(A, wood))[i] = as_global(COLD(A)->wood_coarse)[i];
  }
  if (A.sig_shift >= 0) {  // cross-section brackets of the flight step (track_pool.inc)
    const int nc = (A.num_values + (1 << A.sig_shift) - 1) >> A.sig_shift;
    for (int i = threadIdx.x; i < nc * nmat; i += (int)blockDim.x)
      reinterpret_cast<unsigned short*>(lds_raw + A.lds.sig_mid)[i] = as_global(COLD(A)->sig_mid)[i];
    for (int i = threadIdx.x; i < nc; i += (int)blockDim.x) LDS_F(A.lds.sig_w)[i] = as_global(COLD(A)->sig_w)[i];
  }
#endif
  __syncthreads();
}

#if defined(MC_STATS) && MC_STATS
// diagnostic build only (track_stats.hip): scheduler statistics, one atomic per wave and counter at exit
#define STAT_ADD(slot, v) st[slot] += (unsigned long long)(v)
#else
#define STAT_ADD(slot, v)
#endif
