// track_pool.inc -- the FAST (production) photon-history kernel for CDNA4 (gfx950).  Included by track_fast.hip and,
// with MC_STATS, by track_stats.hip (#define MC_COMPAT 0, contraction allowed, native transcendental instructions).
//
// WHAT is computed: track_common.inc (reference K.cu:120-384 and helpers).  HOW it is scheduled:
//
//  * A lane owns TWO histories: one in registers (R) and one parked in a lane-private LDS slot (S, 12 dwords:
//    position, direction, energy, RNG state, majorant mean free path, packed {energy bin, material, scatter class}, tau).
//    Each has a phase {FLIGHT, COMPTON, SHELL, RAYLEIGH, HOP, ESCAPED, ABSORBED, NEW, DONE}; R alone can also be REAL.
//    The wave loops over Woodcock flight steps for the lanes whose R history is in FLIGHT.  A step needs only
//    the total cross section (8 bytes from a 1.9 MB, L2-resident table) and ends in FLIGHT (virtual interaction), REAL
//    (a real one, kind not drawn yet), HOP (virtual, in the homogeneous exterior) or ESCAPED.  Once `swap_batch` lanes
//    have parked, the wave stops at a scheduling point, where
//      - REAL histories draw the kind of their interaction from the full cross-section record (classify_real);
//      - a kind of work (Compton sampling / Rayleigh sampling / exterior crossing + detector and dose tally + source sampling) is
//        serviced when the lanes holding such a history in R or S reach its threshold: those lanes bring it into R, the batch runs
//        (round 6: HOP histories cross the exterior -- exterior_hop, one exact free-path sample -- in the tally + source service,
//        whose batches are full, instead of at every scheduling point at a handful of lanes: thorax +5 %, CIRS +2 %);
//      - every lane whose R history is parked and whose S history can fly exchanges the two.
//    So the heavy, rarely taken branches run on large batches instead of every lane waiting for the slowest history
//    of its wave (the reference structure, K.cu:237-375), and flight steps are not spent on empty space.
//  * A history's RNG stream depends only on its id and moves with it; tallies are integer atomics.  The image is
//    therefore independent of this schedule, of the thresholds and of the rank split (bit for bit).
//  * History ids are dealt dynamically, 256 at a time, from 64 global counters that each own a contiguous 1/64 of the
//    launch (id_tickets.hpp: a counter hands out tickets, ticket t is its t-th 256 ids).  A wave draws from its home counter
//    and, once that is exhausted, from the next one that no wave has reported exhausted in the counters' shared mask word:
//    all waves finish together, and the last moments of a launch are not spent on up to 63 empty tickets per wave -- 5e5
//    atomics over the headline grid, serialised per counter, which cost 3 % of the Catphan launch (profiles/launch_end_ab.md).
//    ONE counter was the first design -- and the bottleneck nobody saw: atomics on one address are serialised
//    at about 18 ns each, the 3.9e5 fetches of a 1e8-history launch took 7.2 ms, and no change to the kernel moved the
//    Catphan time any more (thresholds, slot trading, fewer source instructions: all +-0.5 %) until the chunk size was
//    varied.  With 64 addresses the same fetches cost nothing measurable: 7.25 -> 5.2 ms.
//  * Two schedulers run this: track_pool_kernel (the per-wave pool described above, the default) and track_wg_kernel (a pool per
//    workgroup, MCGPU_FAST_SCHED=1).  What they serve is defined ONCE, above both -- flight_iteration, serve_compton, serve_rayleigh,
//    score_finished, deal_history_ids, start_history, exchange_history -- and a kernel holds only what is its own: who holds which
//    history, when a batch runs, the settle step, and the counters about a batch as a whole.
#if MC_COMPAT
#error "track_pool.inc is the FAST kernel; the COMPAT kernel lives in track_kernel.inc"
#endif
#include <type_traits>

#include "track_common.inc"  // opens namespace mcgpu { namespace {

constexpr int kPoolBlock = kPoolBlockThreads;
static_assert(kStageWorkgroupSlack == 2u * (kPoolBlockThreads / 64) * kChunk, "tally_stage.hpp: the capacity's allowance is two id chunks per wave");
constexpr int kParked = kPoolParked;                 // parked histories per lane (LDS slots)
constexpr int kSlotStride = kParked * kPoolBlock;    // columns of the workgroup's slot array: word f of column t at slots[f * kSlotStride + t]

#if MC_STATS
// diagnostic build: wave-cycles (s_memtime) per section, counters 12..15 = Compton, Rayleigh, tally+source, flight steps
#define STAT_T0() const unsigned long long t_sec = __builtin_readcyclecounter()
#define STAT_T1(slot) st[slot] += __builtin_readcyclecounter() - t_sec
// the wave's counters: what STAT_ADD / STAT_T1 write as `st` (slots: include/mcgpu_amd.h, engine.py: scheduler_stats)
struct Stats {
  unsigned long long v[kNumStats] = {};
  __device__ __forceinline__ unsigned long long& operator[](int slot) { return v[slot]; }
};
#else
#define STAT_T0()
#define STAT_T1(slot)
struct Stats {};  // the product build counts nothing: the `st` the shared bodies take is empty
#endif

// the register-resident history of a lane
struct History {
  Particle P = {0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f};
  Rng rng = {1u, 1u};
  int index = 0;      // energy bin
  float mfpW = 0.f;   // Woodcock majorant mean free path at P.E
  float aux = 0.f;    // FLIGHT: total inverse mean free path of (P.E, mc_old), a register-only cache; SHELL: tau of the accepted angle
  int mc = 0;         // compact material of the last looked-up voxel (the interaction site when parked)
  int scatter = 0;    // 0 primary, 1 Compton, 2 Rayleigh, 3 multiple
};

// Exchange the register history with the one in an LDS slot: 12 words, word f of the slot at slot[f * kStride] (kStride: the
// columns of the slot array, so a wave-instruction touches 64 consecutive banks).  Bits 28..31 of the packed word are the caller's:
// `tag` goes into the slot, the slot's comes back.  The per-wave pool keeps its phases in registers and leaves them 0; the
// workgroup-level pool's slots belong to nobody, so the phase of the history travels there.
template <int kStride>
__device__ __forceinline__ unsigned int exchange_history(unsigned int* slot, History& h, unsigned int tag) {
  // ds_wrxchg_rtn_b32: the LDS write-exchange returns the old word, so the 12 words swap in place without temporaries
  auto xf = [&](int f, float& v) { v = __uint_as_float(atomicExch(slot + f * kStride, __float_as_uint(v))); };
  auto xu = [&](int f, unsigned int& v) { v = atomicExch(slot + f * kStride, v); };
  xf(0, h.P.x); xf(1, h.P.y); xf(2, h.P.z); xf(3, h.P.u); xf(4, h.P.v); xf(5, h.P.w); xf(6, h.P.E);
  xu(7, h.rng.x); xu(8, h.rng.c);
  xf(9, h.mfpW);
  unsigned int packed = (unsigned int)h.index | ((unsigned int)h.mc << 16) | ((unsigned int)h.scatter << 24) | (tag << 28);
  xu(10, packed);
  h.index = (int)(packed & 0xFFFFu);
  h.mc = (int)((packed >> 16) & 0xFFu);
  h.scatter = (int)((packed >> 24) & 0xFu);
  xf(11, h.aux);
  return packed >> 28;
}

// The region outside the object box is homogeneous background (device_model.hpp, brick code kBrickExterior): a photon
// there is moved in one exact step instead of being delta-tracked through it.  Free path s = -ln(xi) / (rho * sigma_tot)
// of the background material at the photon's energy; the target is the entry point of the object box (if the ray hits it)
// or the exit from the volume.  s < distance: a real interaction in the background at that point (kind drawn like any
// other); else the photon enters the object box (FLIGHT continues with Woodcock steps) or leaves (ESCAPED).  Woodcock
// tracking is exact for any majorant, so replacing it by the exact exponential law in a homogeneous region leaves every
// tally's distribution unchanged; on the Catphan workload it removes more than half of the 22.9 flight steps per history.
// total cross-section record of the background material at the history's energy bin (exterior_hop's only memory access;
// callers issue it early so that its latency overlaps other work)
__device__ __forceinline__ float2 exterior_record(const TrackArgs& A, int index) {
  const int mc_ext = __float_as_int(LDS_F2(A.lds.pal)[kBrickExterior].y);
  return ((const float2*)A.mfp_tot)[table_row(A, index, mc_ext)];
}
// Entry / exit parameters of the ray with the elliptic cylinder around the object (TrackCold::ell_*); a miss gives in > out.
__device__ __forceinline__ void cylinder_span(const TrackArgs& A, const Particle& P, float& t_in, float& t_out) {
  const float big = 3.0e30f;
  const float ia = COLD(A)->ell_inv[0], ib = COLD(A)->ell_inv[1];
  if (ia == 0.0f) { t_in = -big; t_out = big; return; }  // no cylinder for this geometry (a wave-uniform branch: scalar operands)
  const float dx = P.x - COLD(A)->ell_c[0], dy = P.y - COLD(A)->ell_c[1];
  const float qa = P.u * P.u * ia + P.v * P.v * ib, qb = dx * P.u * ia + dy * P.v * ib, qc = dx * dx * ia + dy * dy * ib - 1.0f;
  const float disc = qb * qb - qa * qc;
  const bool along = !(qa > 1.0e-12f);  // parallel to the axis: inside iff qc <= 0
  const float sq = __builtin_amdgcn_sqrtf(fmaxf(disc, 0.0f)), inv = __builtin_amdgcn_rcpf(along ? 1.0f : qa);
  t_in = along ? ((qc <= 0.0f) ? -big : big) : ((disc < 0.0f) ? big : (-qb - sq) * inv);
  t_out = along ? ((qc <= 0.0f) ? big : -big) : ((disc < 0.0f) ? -big : (-qb + sq) * inv);
}
__device__ __forceinline__ void exterior_hop(const TrackArgs& A, History& h, int& phase, const float2 t) {
  Particle& P = h.P;
  const float big = 3.0e30f;
  const float ix = (fabsf(P.u) > 1.0e-12f) ? __builtin_amdgcn_rcpf(P.u) : big, iy = (fabsf(P.v) > 1.0e-12f) ? __builtin_amdgcn_rcpf(P.v) : big,
              iz = (fabsf(P.w) > 1.0e-12f) ? __builtin_amdgcn_rcpf(P.w) : big;
  // slab test against the object box
  const float ax = (COLD(A)->objbox_lo[0] - P.x) * ix, bx = (COLD(A)->objbox_hi[0] - P.x) * ix;
  const float ay = (COLD(A)->objbox_lo[1] - P.y) * iy, by = (COLD(A)->objbox_hi[1] - P.y) * iy;
  const float az = (COLD(A)->objbox_lo[2] - P.z) * iz, bz = (COLD(A)->objbox_hi[2] - P.z) * iz;
  float c_in, c_out;
  cylinder_span(A, P, c_in, c_out);  // the object region is box AND cylinder
  const float t_in = fmaxf(fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fminf(az, bz)), c_in);
  const float t_out = fminf(fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz)), c_out);
  const bool hits = t_out >= fmaxf(t_in, 0.0f);
  // distance to the face through which the ray leaves the volume
  const float ex = ((P.u > 0.f ? SARG(A, bbox)[0] : 0.f) - P.x) * ix, ey = ((P.v > 0.f ? SARG(A, bbox)[1] : 0.f) - P.y) * iy,
              ez = ((P.w > 0.f ? SARG(A, bbox)[2] : 0.f) - P.z) * iz;
  const float t_exit = fminf(fminf(fabsf(ex), fabsf(ey)), fabsf(ez));
  const float target = hits ? fmaxf(t_in, 0.0f) : t_exit;
  const float2 pd = LDS_F2(A.lds.pal)[kBrickExterior];
  const int mc_ext = __float_as_int(pd.y);
  const float mu = pd.x * fmaf(P.E, t.y, t.x);  // attenuation coefficient of the background [1/cm]
  const float s = -0.69314718055994531f * __builtin_amdgcn_logf(rng_f(h.rng)) * __builtin_amdgcn_rcpf(mu);
  if (s < target) {
    P.x = fmaf(s, P.u, P.x); P.y = fmaf(s, P.v, P.y); P.z = fmaf(s, P.w, P.z);
    h.mc = mc_ext;
    phase = PH_REAL;
  } else if (hits) {
    const float m = target + 1.0e-4f;  // just inside the object box
    P.x = fmaf(m, P.u, P.x); P.y = fmaf(m, P.v, P.y); P.z = fmaf(m, P.w, P.z);
    phase = PH_FLIGHT;
  } else {
    phase = PH_ESCAPED;  // tally_image projects from any point of the ray
  }
}

// The reference's entry-face shell (K.cu:714-805, :249-262, :1036-1042).  move_to_bbox puts an entering photon EPS_SOURCE = 1.5e-5 cm past
// the entry face ALONG ITS RAY; locate_voxel calls everything within EPS_SOURCE of a face "outside"; float rounding at |position| ~ 100 cm
// (ulp 7.6e-6) moves the landing point by half that margin either way.  A first Woodcock step that ends before the photon is
// EPS_SOURCE deep -- a few 1e-5 of all photons, depending on projection angle and energy -- therefore ends the history at once: the
// photon is scored as an un-attenuated primary.  source_entry below crosses the exterior analytically and has no such shell; this
// function reproduces it by doing what the reference does ON THE ENTRY AXIS, in its arithmetic -- correctly rounded division,
// separately rounded multiply and add, the reference's own majorant a + E b of the energy bin (MC-GPU_kernel_v1.3.cu:228) -- for the
// few lanes whose shell deviate xi is close enough to 1 that the step -mfp ln(xi) could end inside the shell.  p, d, size:
// position and direction cosine of the photon on the axis through whose face it enters, and the volume's extent there.
// Returns true: the photon never gets in (the caller scores it from the focal spot: tally_image projects along the ray).
// (Not reproduced: the same shell along the EDGES of the entry face, 1e-6 of its area.)
__device__ __forceinline__ bool entry_face_shell(const TrackArgs& A, float p, float d, float size, float E, float xi, int index) {
  // a / b correctly rounded (Markstein): reciprocal refined by one Newton step, quotient corrected by its exact residual
  const float num = (d > 0.0f) ? -p : size - p;
  float y = __builtin_amdgcn_rcpf(d);
  y = fmaf(fmaf(-d, y, 1.0f), y, y);
  float q = num * y;
  q = fmaf(fmaf(-d, q, num), y, q);
  const float t = kEps + q;                           // entry_dist (track_common.inc)
  float c = p + t * d;                                // (no contraction in this translation unit)
  const float2 wk = ((const float2*)as_global(COLD(A)->woodcock))[index];  // (behind COLD: a pointer the hot path never needs costs it no scalar register)
  const float mfp = wk.x + E * wk.y;
  const float u = 1.0f - xi;                          // exact: xi = k 2^-24 + 2^-26
  const float step = mfp * fmaf(0.5f * u, u, u);      // -mfp ln(1 - u), u < 1e-3: the series to float accuracy
  c += step * d;
  return (d > 0.0f) ? (c < kEps) : (c > size - kEps);  // locate_voxel's test on that axis
}

// A new photon at the focal spot (outside the object box, normally outside the volume): move_to_bbox (K.cu:714-805) and
// the exterior hop in one.  Two slab tests share the reciprocals of the direction: against the volume (entry t_vol; a ray
// that misses the volume stays at the focal spot and is scored from there, K.cu:240-241,795-804) and against the object box
// (entry t_obj).  Only the stretch [t_vol, min(t_obj, volume exit)] holds matter (the background material); one exact free
// path against its length decides between an interaction in the background, entering the object box, and leaving.
__device__ __forceinline__ void source_entry(const TrackArgs& A, History& h, int& phase, const float2 t) {
  Particle& P = h.P;
  const float big = 3.0e30f;
  const float ix = (fabsf(P.u) > 1.0e-12f) ? __builtin_amdgcn_rcpf(P.u) : big, iy = (fabsf(P.v) > 1.0e-12f) ? __builtin_amdgcn_rcpf(P.v) : big,
              iz = (fabsf(P.w) > 1.0e-12f) ? __builtin_amdgcn_rcpf(P.w) : big;
  const float vax = -P.x * ix, vbx = (SARG(A, bbox)[0] - P.x) * ix, vay = -P.y * iy, vby = (SARG(A, bbox)[1] - P.y) * iy, vaz = -P.z * iz, vbz = (SARG(A, bbox)[2] - P.z) * iz;
  const float nx = fminf(vax, vbx), ny = fminf(vay, vby), nz = fminf(vaz, vbz);
  const float v_in = fmaxf(fmaxf(fmaxf(nx, ny), nz), 0.0f);
  const float v_out = fminf(fminf(fmaxf(vax, vbx), fmaxf(vay, vby)), fmaxf(vaz, vbz));
  const bool hits_vol = v_out >= v_in;
  // the entry-face shell of the reference: its own deviate.  The step -mfp ln(xi) can end within 6e-5 cm of the face (EPS_SOURCE plus
  // every rounding at 200 cm) only if (1 - xi) mfpW <= 6e-5 / |cos| -- mfpW, the coarse bin's majorant, is at most the reference's
  // mean free path, and 1 - xi at most -ln(xi).  Two levels, so that the common path pays three instructions: first against
  // |cos| >= 1/16 (a ray that enters a face at more than 86.4 degrees from its normal is not looked at: no beam of a CBCT fan
  // holds one), which one lane in 200 passes; those lanes then test their own entry axis (one in several thousand passes), and
  // only for them the reference's arithmetic runs.
  const float xi_shell = rng_f(h.rng);
  const float reach = (1.0f - xi_shell) * h.mfpW;
  if (__ballot(reach <= 16.0f * 6.0e-5f) != 0ULL) {
    const bool ax = (v_in == nx), ay = (v_in == ny);
    const float inv_entry = ax ? ix : (ay ? iy : iz);
    if (hits_vol && v_in > 0.0f && reach <= 6.0e-5f * fabsf(inv_entry) &&
        entry_face_shell(A, ax ? P.x : (ay ? P.y : P.z), ax ? P.u : (ay ? P.v : P.w), ax ? SARG(A, bbox)[0] : (ay ? SARG(A, bbox)[1] : SARG(A, bbox)[2]), P.E, xi_shell, h.index)) {
      phase = PH_ESCAPED;  // scored from the focal spot
      return;
    }
  }
  const float oax = (COLD(A)->objbox_lo[0] - P.x) * ix, obx = (COLD(A)->objbox_hi[0] - P.x) * ix;
  const float oay = (COLD(A)->objbox_lo[1] - P.y) * iy, oby = (COLD(A)->objbox_hi[1] - P.y) * iy;
  const float oaz = (COLD(A)->objbox_lo[2] - P.z) * iz, obz = (COLD(A)->objbox_hi[2] - P.z) * iz;
  float c_in, c_out;
  cylinder_span(A, P, c_in, c_out);  // the object region is box AND cylinder
  const float o_in = fmaxf(fmaxf(fmaxf(fmaxf(fminf(oax, obx), fminf(oay, oby)), fminf(oaz, obz)), c_in), 0.0f);
  const float o_out = fminf(fminf(fminf(fmaxf(oax, obx), fmaxf(oay, oby)), fmaxf(oaz, obz)), c_out);
  const bool hits_obj = o_out >= o_in;
  const float target = hits_obj ? o_in : v_out;
  const float2 pd = LDS_F2(A.lds.pal)[kBrickExterior];
  const float mu = pd.x * fmaf(P.E, t.y, t.x);  // attenuation coefficient of the background [1/cm]
  const float s = v_in - 0.69314718055994531f * __builtin_amdgcn_logf(rng_f(h.rng)) * __builtin_amdgcn_rcpf(mu);
  float m = 0.0f;  // a ray that leaves (or misses the volume) is scored from the focal spot: tally_image projects along the ray
  phase = PH_ESCAPED;
  if (hits_vol && s < target) { m = s; h.mc = __float_as_int(pd.y); phase = PH_REAL; }
  else if (hits_vol && hits_obj) { m = target + 1.0e-4f; phase = PH_FLIGHT; }  // just inside the object box
  P.x = fmaf(m, P.u, P.x); P.y = fmaf(m, P.v, P.y); P.z = fmaf(m, P.w, P.z);
}

// Draw the kind of a real interaction (K.cu:289-354) from the full 32-byte record: P(kind | real) = sigma_kind / sigma_total.
__device__ __forceinline__ const float4* real_record(const TrackArgs& A, const History& h) {
  return (const float4*)as_global(SARG(A, mfp)) + 2u * table_row(A, h.index, h.mc);
}
__device__ __forceinline__ void classify_real(const TrackArgs& A, History& h, int& phase, const float4 r0, const float4 r1) {
  const float E = h.P.E;
  const float s_tot = fmaf(E, r0.w, r0.x), s_co = fmaf(E, r1.x, r0.y), s_ra = fmaf(E, r1.y, r0.z);
  const float xi = rng_f(h.rng) * s_tot;
  phase = (xi < s_co) ? PH_COMPTON : ((xi < s_co + s_ra) ? PH_RAYLEIGH : PH_ABSORBED);
}

__device__ __forceinline__ bool wants_new(int ph) { return (unsigned int)(ph - PH_ESCAPED) < 3u; }  // ESCAPED, ABSORBED, NEW
// histories the tally + source service of the per-wave pool takes: the above plus the ones waiting in the homogeneous exterior (HOP)
__device__ __forceinline__ bool wants_service(int ph) { return wants_new(ph) || ph == PH_HOP; }
__device__ __forceinline__ bool in_compton(int ph) { return ph == PH_COMPTON || ph == PH_SHELL; }

// One Woodcock flight step of a history in FLIGHT (K.cu:249-279) per wave iteration.
//
// A step is a chain  random step -> position -> brick code (LDS) -> [mixed brick: voxel byte from memory] -> palette
// (LDS) -> virtual-or-real test [-> exact cross section from memory inside the bracket].  Measured and NOT adopted:
// computing the position after the next step speculatively (it depends on random numbers only if this step ends
// virtual) and requesting its voxel byte together with this one's -- two round trips in flight per lane, half as many
// wave iterations.  The iterations halved and took twice as long each: with 8 waves per SIMD a flight iteration is bound
// by instruction issue, not by the voxel round trip, and the dropped second steps (the first one ended the flight) made
// the thorax workload 7 % slower.
//
// flight_locate: position of the step from P, clamped to the bounding box (lanes that have just left the volume stay in
// bounds), brick code, and the request for the voxel byte of a mixed brick.  flight_resolve: material, density and the
// virtual-or-real test.
// Kernel variants of the FAST personality: the storage kinds of device_model.hpp plus "u8 with the second brick level"
// (a compile-time fact, so that the default -- second level off -- carries neither its test nor its pointer in the flight loop)
constexpr int kVolU8Sub = 3;
constexpr int kVolU8Rec = 4;  // u8 with the second level as 16-byte tile records (device_model.hpp: TileRecord)
__host__ __device__ constexpr bool is_u8(int vk) { return vk == kVolU8 || vk == kVolU8Sub || vk == kVolU8Rec; }

struct StepSite {
  float x, y, z;       // position after the step
  int e;               // LDS palette slot (brick code < 15), or kBrickMixed: `raw` holds the voxel's palette index
  unsigned int raw;    // voxel byte / 16-bit index (requested in flight_locate, first used in flight_resolve)
  float2 pd;           // raw-float2 volumes: the voxel itself
  bool out, exterior;
};
template <int VK>
__device__ __forceinline__ void flight_locate(const TrackArgs& A, const Particle& P, float px, float py, float pz, float step, const float hi_x,
                                              const float hi_y, const float hi_z, StepSite& s) {
  s.x = fmaf(step, P.u, px);
  s.y = fmaf(step, P.v, py);
  s.z = fmaf(step, P.w, pz);
  const float cx = __builtin_amdgcn_fmed3f(s.x, kEps, hi_x);
  const float cy = __builtin_amdgcn_fmed3f(s.y, kEps, hi_y);
  const float cz = __builtin_amdgcn_fmed3f(s.z, kEps, hi_z);
  s.out = (cx != s.x) | (cy != s.y) | (cz != s.z);  // locate_voxel (K.cu:1036-1042)
  s.exterior = false;
  s.raw = 0u;
  s.pd = make_float2(0.f, 0.f);
  const unsigned int ix = (unsigned int)(int)(cx * A.inv_vs[0]), iy = (unsigned int)(int)(cy * A.inv_vs[1]), iz = (unsigned int)(int)(cz * A.inv_vs[2]);
  if (is_u8(VK)) {
    // bricks are (2^k)^3 voxels: the brick coordinate is the voxel coordinate shifted
    const unsigned int bi = (ix >> A.brick_shift) + __umul24(iy >> A.brick_shift, (unsigned int)A.brick_nx) + __umul24(iz >> A.brick_shift, (unsigned int)A.brick_nxy);
    s.e = ((int)(lds_raw + A.lds.brick)[bi >> 1] >> ((bi & 1u) << 2)) & 0xF;
    s.exterior = (s.e == kBrickExterior);
    if (VK == kVolU8Rec && s.e == kBrickMixed) {
      // the tile's record instead of the voxel byte: 16 bytes, eight tiles (an 8^3 cube) per 128-byte line
      const unsigned int tx = ix >> 2, ty = iy >> 2, tz = iz >> 2;
      const unsigned int ri = ((((tx >> 1) + __umul24(ty >> 1, (unsigned int)A.rec_nx) + __umul24(tz >> 1, (unsigned int)A.rec_nxy))) << 3) | ((tz & 1u) << 2) |
                              ((ty & 1u) << 1) | (tx & 1u);
      const uint4 r = reinterpret_cast<const uint4*>(A.sub)[ri];
      const unsigned int bit = ((iz & 3u) << 4) | ((iy & 3u) << 2) | (ix & 3u);
      const unsigned int word = (bit & 32u) ? r.w : r.z;
      s.raw = ((word >> (bit & 31u)) & 1u) ? ((r.x >> 8) & 0xFFu) : (r.x & 0xFFu);
      if (r.y != 0u) {  // three or more palette entries in this tile (a junction; device_model.hpp: TileRecord)
        if (r.y >= kTileAskVolume) {  // no majority entry, or five and more: the byte itself
          const unsigned int si = tx + __umul24(ty, (unsigned int)A.sub_nx) + __umul24(tz, (unsigned int)A.sub_nxy);
          s.raw = (unsigned int)((const unsigned char*)A.vol)[(si << 6) | bit];
        } else if ((word >> (bit & 31u)) & 1u) {
          // not the majority entry: the rank of this voxel among the set bits of the mask selects its field of the code
          // (32-bit operations: the set bits of this voxel's word below it, plus the whole low word for a voxel of the high one)
          const unsigned int rank = (unsigned int)__popc(word & ((1u << (bit & 31u)) - 1u)) + ((bit & 32u) ? (unsigned int)__popc(r.z) : 0u);
          const unsigned int wide = r.y >> 30;  // 0: one bit per voxel (b, c), 1: two bits (b, c, d)
          const unsigned int sel = (r.y >> (rank << wide)) & (1u + 2u * wide);
          s.raw = (r.x >> (8u + 8u * sel)) & 0xFFu;
        }
      }
    } else if (s.e == kBrickMixed) {
      // sub-brick (4^3 voxels) of the step: index of its code in the second-level table AND of its 64-byte tile in the volume
      const unsigned int si = (ix >> 2) + __umul24(iy >> 2, (unsigned int)A.sub_nx) + __umul24(iz >> 2, (unsigned int)A.sub_nxy);
      // second level: the code of the sub-brick from the L2-resident table; the volume only for a mixed sub-brick
      // (measured and NOT adopted: both requests in flight together -- one round trip instead of two dependent ones, at the price of
      // voxel bytes fetched for homogeneous sub-bricks)
      if (VK == kVolU8Sub) s.e = ((int)A.sub[si >> 1] >> ((si & 1u) << 2)) & 0xF;
      if (s.e == kBrickMixed) s.raw = (unsigned int)((const unsigned char*)A.vol)[(si << 6) | ((iz & 3u) << 4) | ((iy & 3u) << 2) | (ix & 3u)];
    }
  } else {
    const unsigned int vi = ix + __umul24(iy, (unsigned int)A.nx) + __umul24(iz, (unsigned int)A.nxy);
    s.e = kBrickMixed;
    if (VK == kVolU16) s.raw = (unsigned int)((const unsigned short*)A.vol)[vi];
    else s.pd = ((const float2*)A.vol)[vi];
  }
}
// mc_old / h.aux cache the total cross section of the last material; st_mixed / st_sig report which memory path was
// taken (diagnostic build).  Returns the phase the step ends in: FLIGHT (virtual), HOP (virtual in the exterior), REAL,
// ESCAPED.
template <int VK>
__device__ __forceinline__ int flight_resolve(const TrackArgs& A, History& h, const StepSite& s, int& mc_old, const int nmat, bool& st_mixed,
                                              bool& st_sig) {
  float dens;
  if (is_u8(VK)) {
#if MC_STATS
    st_mixed = st_mixed || (s.e == kBrickMixed);
#endif
    const float2 pd = LDS_F2(A.lds.pal)[(s.e == kBrickMixed) ? kPaletteBase + (int)s.raw : s.e];
    dens = pd.x;
    h.mc = __float_as_int(pd.y);
  } else if (VK == kVolU16) {
    const float2 pd = ((const float2*)A.palette)[s.raw];
    dens = pd.x;
    h.mc = __float_as_int(pd.y);
  } else {
    dens = s.pd.x;
    h.mc = __float_as_int(s.pd.y);
  }
  // probability of a virtual interaction p0 = 1 - mfpW * dens * sigma_tot(E, material) (K.cu:268-274).  sigma_tot of
  // the material cached in h.aux is exact; for another material the LDS brackets [lo, hi] of the coarse energy bin
  // decide every random number outside [1 - m*hi, 1 - m*lo) (fma is monotonic, so the bounds hold for the rounded
  // values too); only the band in between requests the exact 8 bytes from the L2-resident table.  Same random
  // number, same decision as the exact test.  A real interaction is parked as REAL: its kind is drawn at the next
  // scheduling point from the full record, P(kind | real) = sigma_kind / sigma_total -- the same distribution as the
  // reference's cumulative test on one random number (K.cu:289-354).
  const float md = h.mfpW * dens;
  const float xi = rng_f(h.rng);
  // the step ends virtual iff xi < p_thr.  Same material as the cached cross section: p_thr = p0 exactly.  Another material: the
  // brackets settle the test without the table (p_thr = 2: virtual whatever xi is, p_thr = -1: real) or leave it open (p_thr
  // from the exact cross section, which becomes the cached one).  One float carries the verdict out of the branches instead of
  // two booleans (the compiler materialised those as 0 / 1 registers and merged them with selects: 9 instructions fewer).
  float p_thr = fmaf(-md, h.aux, 1.0f);
  if (h.mc != mc_old) {
    bool need_exact = true;
    if (A.sig_shift >= 0) {
      const int cb = h.index >> A.sig_shift;
      const float mid = (float)reinterpret_cast<const _Float16*>(lds_raw + A.lds.sig_mid)[__mul24(cb, nmat) + h.mc];
      const float w = LDS_F(A.lds.sig_w)[cb];
      const float p_lo = fmaf(-md, fmaf(mid, w, mid), 1.0f), p_hi = fmaf(-md, fmaf(-mid, w, mid), 1.0f);
      p_thr = (xi < p_lo) ? 2.0f : -1.0f;
      need_exact = !(xi < p_lo) && (xi < p_hi);
    }
    if (need_exact) {
#if MC_STATS
      st_sig = true;
#endif
      // total inverse mean free path per unit density at this energy (K.cu:268-269): 8 bytes from the L2-resident table
      const float2 t = ((const float2*)A.mfp_tot)[table_row(A, h.index, h.mc)];
      h.aux = fmaf(h.P.E, t.y, t.x);
      mc_old = h.mc;
      p_thr = fmaf(-md, h.aux, 1.0f);
    }
  }
  const bool is_virtual = xi < p_thr;
  // a virtual interaction in the exterior: from here on the photon is moved analytically (exterior_hop, batched)
  const int ph = is_virtual ? ((s.exterior && (A.has_exterior & 1)) ? PH_HOP : PH_FLIGHT) : PH_REAL;
  return s.out ? PH_ESCAPED : ph;
}
template <int VK>
__device__ __forceinline__ void flight_steps(const TrackArgs& A, History& h, int& phase, int& mc_old, const float negl2, const float hi_x,
                                             const float hi_y, const float hi_z, const int nmat, bool& st_mixed, bool& st_sig,
                                             unsigned long long& t_loaded) {
  Particle& P = h.P;
  StepSite a;
  flight_locate<VK>(A, P, P.x, P.y, P.z, negl2 * __builtin_amdgcn_logf(rng_f(h.rng)), hi_x, hi_y, hi_z, a);  // step = -mfpW * ln(xi)
#if MC_STATS
  if (VK != kVolRaw) asm volatile("" : "+v"(a.raw));
  t_loaded = __builtin_readcyclecounter();  // the voxel byte has arrived
#endif
  P.x = a.x; P.y = a.y; P.z = a.z;
  phase = flight_resolve<VK>(A, h, a, mc_old, nmat, st_mixed, st_sig);
}

// End of a FAST kernel: every wave of the workgroup arrives here exactly once -- both schedulers leave their loop by `break` only,
// waves that run out of work early (PH_DONE), the panic and the cycle-bound exits included -- and the conditions are launch arguments,
// the same for the whole grid.  Behind one barrier: the material dose accumulators (flush_dose) and the staging counts.
__device__ __forceinline__ void finish_workgroup(const TrackArgs& A) {
  const bool staged = LARG(A, stage.region) != nullptr, dose = (A.dose_flags & kDoseMaterials) != 0;
  if (!staged && !dose) return;
  __syncthreads();
  if (dose && threadIdx.x < 2 * kMaxMaterials) {
    const unsigned long long v = reinterpret_cast<unsigned long long*>(lds_raw + SLDS(A, dose_mat))[threadIdx.x];
    if (v != 0ULL) atomicAdd((unsigned long long*)as_global(COLD(A)->dose_materials) + threadIdx.x, v);
  }
  if (staged) stage_counts_publish(A);
}

// ================================================================================================
// What a scheduler serves: the bodies below are the physics of one batch, written once for both schedulers.  Each works on the
// register history of the calling lane; which lanes hold what, when a batch is worth running and what is counted about the batch
// as a whole is the calling scheduler's business.  `st`: the wave's counters (diagnostic build; empty otherwise).
// ================================================================================================

// One wave iteration of the flight loop: a Woodcock step (K.cu:249-279) for the lanes in FLIGHT.  Branch-free up to the two rare
// memory paths (mixed brick, new cross-section record): the position clamped to the bounding box indexes the lookups, so lanes that
// have just left the volume stay in bounds.  The caller takes the ballot of the lanes still in FLIGHT itself: taken in here, the
// compiler carries its predicate as a boolean through the divergent step -- four more instructions in a flight loop of 87 ... 142,
// the thorax workload 0.7 % slower (profiles/fast_services_refactor.md).
template <int VK>
__device__ __forceinline__ void flight_iteration(const TrackArgs& A, History& h, int& phase, int& mc_old, const float negl2, const float hi_x,
                                                 const float hi_y, const float hi_z, const int nmat, Stats& st) {
#if MC_STATS
  const unsigned long long t_fl = __builtin_readcyclecounter();
#endif
  bool st_mixed = false, st_sig = false;  // diagnostic build only (dead otherwise)
  unsigned long long t_loaded = 0;
  STAT_ADD(23, __popcll(__ballot(phase == PH_FLIGHT)));  // lanes that take this flight step
  if (phase == PH_FLIGHT) flight_steps<VK>(A, h, phase, mc_old, negl2, hi_x, hi_y, hi_z, nmat, st_mixed, st_sig, t_loaded);
#if MC_STATS
  {
    const unsigned long long t_end = __builtin_readcyclecounter();
    st[15] += t_end - t_fl;
    // wave-level split: up to the arrival of the voxel bytes (first active lane's stamp) / the rest of the iteration
    const unsigned long long act = __ballot(t_loaded != 0ULL);
    if (act != 0ULL) {
      const int l0 = __ffsll((long long)act) - 1;
      const unsigned long long tl = ((unsigned long long)__shfl((unsigned int)(t_loaded >> 32), l0) << 32) | (unsigned long long)__shfl((unsigned int)t_loaded, l0);
      st[28] += tl - t_fl;
      st[29] += t_end - tl;
    }
  }
#endif
  STAT_ADD(0, 1);
  STAT_ADD(1, __popcll(__ballot(phase == PH_FLIGHT)));
  STAT_ADD(24, __ballot(st_mixed) != 0ULL ? 1 : 0);
  STAT_ADD(25, __popcll(__ballot(st_mixed)));
  STAT_ADD(26, __ballot(st_sig) != 0ULL ? 1 : 0);
  STAT_ADD(27, __popcll(__ballot(st_sig)));
}

// Compton (K.cu:290-326): one straight pass for the lanes whose history is in COMPTON or SHELL (compton_draw: tau if not yet
// accepted, one shell, its profile, the test; then the momentum trial).  A lane whose trial fails keeps its phase (COMPTON: new
// angle; SHELL: new shell at the accepted angle) and takes part in a later batch.
__device__ __forceinline__ void serve_compton(const TrackArgs& A, History& h, int& phase, int& mc_old, float& negl2, Stats& st) {
  STAT_ADD(16, __popcll(__ballot(phase == PH_COMPTON)));
  STAT_ADD(17, __popcll(__ballot(phase == PH_SHELL)));
#if MC_STATS
  const bool st_was_compton = in_compton(phase);
#endif
  if (in_compton(phase)) {
    ComptonTrial c;
    c.tau = h.aux;
    if (compton_draw(A, h.P.E, h.mc, phase == PH_COMPTON, h.rng, c)) {
      const float e_in = h.P.E;
      polar_t omc;
      h.aux = c.tau;
      phase = PH_SHELL;
      if (compton_momentum_trial(h.P.E, c, h.rng, omc)) {
        rotate_dir(h.P, omc, h.rng);
        if (A.dose_flags != 0 && (e_in - h.P.E) > 0.001f) tally_dose(A, h.P, e_in - h.P.E, h.mc);  // K.cu:299,356-367
        h.index = energy_index(A, h.P.E);
        if (h.index > -1) {
          h.mfpW = LDS_F(SLDS(A, wood))[h.index >> kWoodShift];  // the coarse bin's majorant: no table fetch (LdsLayout::wood)
          negl2 = -0.69314718055994531f * h.mfpW;
          mc_old = -2;
          h.scatter = (h.scatter == 0) ? 1 : 3;
          phase = PH_FLIGHT;
        } else {
          h.index = 0;
          phase = PH_NEW;  // below the table cut-off: absorbed
        }
      }
    }
  }
#if MC_STATS
  STAT_ADD(18, __popcll(__ballot(st_was_compton && !in_compton(phase))));  // events completed in this batch
#endif
}

// Rayleigh (K.cu:329-347)
__device__ __forceinline__ void serve_rayleigh(const TrackArgs& A, History& h, int& phase) {
  if (phase == PH_RAYLEIGH) {
    const float pmaxn = as_global(SARG(A, mfp))[8u * table_row(A, h.index, h.mc) + 6u];  // pmax of bin index + 1 (K.cu:336)
    polar_t omc;
    if (rayleigh_trial(A, h.P.E, h.mc, pmaxn, h.rng, omc)) {
      rotate_dir(h.P, omc, h.rng);
      h.scatter = (h.scatter == 0) ? 2 : 3;
      phase = PH_FLIGHT;
    }
  }
}

// A finished history: an ESCAPED photon goes to the detector (tally_word: the word of the detector tally this lane scores in, -1 for
// none; the caller issues tally_score at the end of its batch), an ABSORBED one leaves its energy in its voxel (photoelectric
// absorption, K.cu:350-367).  Either way the lane wants a NEW history.
__device__ __forceinline__ void score_finished(const TrackArgs& A, const History& h, int& phase, int& tally_word, unsigned int& tally_value) {
  tally_word = -1;
  tally_value = 0;
  if (phase == PH_ESCAPED) {
    tally_word = tally_pixel(A, h.P, h.scatter);
    tally_value = __float2uint_rn(h.P.E * 100.0f);
    phase = PH_NEW;
  } else if (phase == PH_ABSORBED) {
    if (A.dose_flags != 0 && h.P.E > 0.001f) tally_dose(A, h.P, h.P.E, h.mc);
    phase = PH_NEW;
  }
}

// Deal history ids to the lanes that need one (phase NEW): wave-uniform bookkeeping executed by every lane (callers enter on a
// wave-uniform condition), ids ranked by ballot.  chunk_next / chunk_left: the first unassigned id of this wave's current ticket and
// how many follow it (at most kChunk: one register instead of the ticket's end); walk: the counter it draws from next (bits 0..7) and
// how many counters it has found exhausted (bits 8.., kWalkDone = all of them: no work is left) in one register.  Returns the lane's
// id, or ~0 for none.
constexpr unsigned int kWalkDone = (unsigned int)kNumCounters << 8;
__device__ __forceinline__ unsigned long long deal_history_ids(const TrackArgs& A, const int phase, unsigned long long& chunk_next, unsigned int& chunk_left,
                                                               unsigned int& walk) {
  unsigned long long my_id = ~0ULL;
  const unsigned long long need = __ballot(phase == PH_NEW);
  const unsigned int n_need = (unsigned int)__popcll(need);
  if (n_need != 0u) {
    const unsigned int rank = __builtin_amdgcn_mbcnt_hi((unsigned int)(need >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)need, 0u));
    const unsigned int avail = chunk_left;
    if (avail >= n_need) {
      my_id = chunk_next + rank;
      chunk_next += n_need;
      chunk_left -= n_need;
    } else {
      // the rest of the old ticket, then a new one (id_tickets.hpp): from this wave's counter or, once that one is exhausted, from
      // the next one that no wave has reported exhausted yet.  The last ticket of a counter may hold fewer ids than lanes ask: the
      // others stay NEW and ask again at the next service.
      if (rank < avail) my_id = chunk_next + rank;
      chunk_left = 0u;
      const int leader = __ffsll((long long)need) - 1;
      const bool leads = (int)(threadIdx.x & 63) == leader;
      while (walk < kWalkDone) {
        const unsigned int ctr = walk & 0xFFu;
        // a ticket: the counter's low dword, one 32-bit atomic (the host refuses a launch whose ticket numbers could pass 2^32); the
        // leader's value, wave-uniform from here on (scalar registers), read with a scalar lane index
        unsigned long long base, size, lo, hi;
        unsigned int tv = 0u;
        id_counter_part(LARG(A, count), ctr, base, size);
        if (leads) tv = atomicAdd(reinterpret_cast<unsigned int*>(LARG(A, work_counter) + ctr * (unsigned int)kCounterStride), 1u);
        id_ticket_range(size, (unsigned int)__builtin_amdgcn_readlane((int)tv, leader), lo, hi);
        if (lo >= hi) {
          // Exhausted: say so in the mask (only a wave that drew an empty ticket sets a bit, and no bit is cleared during a launch) and
          // go on with the first counter nobody has reported.  A bit not seen yet costs one more empty ticket, and the wave's own
          // empty tickets still end the walk at kNumCounters: nothing here waits for another wave.  The OR returns nothing -- a
          // returning one by every wave would be the serialised same-address traffic the mask removes -- and touches the bit's dword only.
          unsigned long long* const mask_word = LARG(A, work_counter) + kIdMaskWord;
          unsigned long long mv = 0;
          if (leads) mv = __hip_atomic_load(mask_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          unsigned long long mask = ((unsigned long long)(unsigned int)__builtin_amdgcn_readlane((int)(mv >> 32), leader) << 32) |
                                    (unsigned long long)(unsigned int)__builtin_amdgcn_readlane((int)mv, leader);
          if (leads && ((mask >> ctr) & 1ULL) == 0ULL) atomicOr(reinterpret_cast<unsigned int*>(mask_word) + (ctr >> 5), 1u << (ctr & 31u));
          mask |= 1ULL << ctr;
          const unsigned int next = id_next_counter(mask, ctr);  // kNumCounters: every counter is known to be exhausted
          walk = next < (unsigned int)kNumCounters ? ((walk & ~0xFFu) + 0x100u) | next : kWalkDone;
          continue;
        }
        // the ticket's first ids to the lanes the old one left out, the rest for later
        const unsigned int got = (unsigned int)(hi - lo), taken = min(n_need - avail, got);
        if (rank >= avail && rank - avail < got) my_id = base + lo + (rank - avail);
        chunk_next = base + lo + taken;
        chunk_left = got - taken;
        break;
      }
    }
  }
  return my_id;
}

// A lane in NEW starts history `my_id` (K.cu:206-247) -- or, given none, is DONE once every counter is exhausted (otherwise it stays
// NEW and asks again at the next service).
__device__ __forceinline__ void start_history(const TrackArgs& A, History& h, int& phase, int& mc_old, float& negl2, const unsigned long long my_id,
                                              const unsigned int walk) {
  if (phase == PH_NEW) {
    if (my_id != ~0ULL) {
      rng_init_history(h.rng, LARG(A, first) + my_id, (unsigned int)LARG(A, seed), LARG(A, stream_key));
      // energy first (K.cu:1033-1040): the two records that depend on it are requested before the direction is
      // sampled, so their latency is covered by that arithmetic
      sample_source_energy(A, h.P, h.rng);
      h.scatter = 0;
      h.index = energy_index(A, h.P.E);
      float2 t_ext = make_float2(0.f, 0.f);
      if (A.has_exterior & 2) t_ext = exterior_record(A, h.index);
      sample_source_direction(A, h.P, h.rng);
      h.mfpW = LDS_F(SLDS(A, wood))[h.index >> kWoodShift];
      negl2 = -0.69314718055994531f * h.mfpW;
      mc_old = -1;
      if (A.has_exterior & 2) {
        // the source sits outside the object box: straight to its entry point (or through / past the volume)
        source_entry(A, h, phase, t_ext);
        if (phase == PH_REAL) {  // REAL lives in registers only: settle it before any exchange
          const float4* rec = real_record(A, h);
          classify_real(A, h, phase, rec[0], rec[1]);
        }
      } else {
        bool miss;
        move_to_bbox(A, h.P, miss);
        phase = miss ? PH_ESCAPED : PH_FLIGHT;
      }
    } else if (walk >= kWalkDone) {
      phase = PH_DONE;  // every counter is exhausted
    }
  }
}

// kDouble: the arithmetic of this translation unit (MC_FAST_F64) as part of the kernel's NAME -- profilers tell track_fast.hip's
// track_pool_kernel<VK, seg, 0> from track_fast64.hip's <VK, seg, 1> (the body does not use it: the arithmetic is chosen by the macro)
template <int VK, bool kSegmentLoop, int kDouble = MC_FAST_F64>
__global__ __launch_bounds__(kPoolBlock, kPoolWavesPerSimd) void track_pool_kernel(const TrackArgs A) {
  [[maybe_unused]] Stats st;
#if MC_STATS
  const unsigned long long t_wave0 = __builtin_readcyclecounter();
  {  // where and when this wave runs: HW_ID (wave/simd/cu/sh/se fields), XCC_ID, constant-rate clock
    const unsigned int w = blockIdx.x * (kPoolBlock / 64) + (threadIdx.x >> 6);
    if ((threadIdx.x & 63) == 0 && A.stats != nullptr && w < (unsigned int)kWaveTrace) {
      const unsigned int hw = __builtin_amdgcn_s_getreg((4 /*HW_ID*/) | (0 << 6) | (31 << 11));
      const unsigned int xcc = __builtin_amdgcn_s_getreg((20 /*XCC_ID*/) | (0 << 6) | (31 << 11));
      A.stats[kNumStats + 3 * w + 0] = (unsigned long long)hw | ((unsigned long long)xcc << 32);
      A.stats[kNumStats + 3 * w + 1] = __builtin_amdgcn_s_memrealtime();
    }
  }
#endif
  stage_cursors_clear(A);
  stage_tables<is_u8(VK) ? (int)kVolU8 : VK>(A);
  // the slots this lane parks its other histories in: pointers, traded between the lanes of the wave (step 4 below).  Column t of
  // the workgroup's slot array: lane `threadIdx.x` starts with columns threadIdx.x + j * kPoolBlock, j < kParked.
  unsigned int* slot[kParked];
  int phS[kParked];  // phases of the parked histories
#pragma unroll
  for (int j = 0; j < kParked; ++j) {
    slot[j] = reinterpret_cast<unsigned int*>(lds_raw + A.lds.slots) + threadIdx.x + j * kPoolBlock;
    phS[j] = PH_NEW;  // NEW and DONE histories carry no state: the slots need not be initialised
  }

  History h;
  int phase = PH_NEW;
  // a parked history of this lane satisfies pred / how many of this lane's histories (register + parked) do
  auto parked = [&](auto pred) {
    bool any = false;
#pragma unroll
    for (int j = 0; j < kParked; ++j) any = any || pred(phS[j]);
    return any;
  };
  auto count = [&](auto pred) {
    int c = pred(phase) ? 1 : 0;
#pragma unroll
    for (int j = 0; j < kParked; ++j) c += pred(phS[j]) ? 1 : 0;
    return c;
  };
  // histories of the wave that satisfy pred (wave-uniform)
  auto wave_count = [&](auto pred) {
    int n = __popcll(__ballot(pred(phase)));
#pragma unroll
    for (int j = 0; j < kParked; ++j) n += __popcll(__ballot(pred(phS[j])));
    return n;
  };
  // h.aux = total inverse mean free path of (h.P.E, mc_old), valid while the R history stays in that material at that energy
  int mc_old = -1;
  float negl2 = 0.f;  // -ln(2) * h.mfpW: flight step = negl2 * log2(xi)
  const float hi_x = A.bbox_hi[0], hi_y = A.bbox_hi[1], hi_z = A.bbox_hi[2];
  unsigned long long chunk_next = 0;  // wave-uniform: unassigned ids of this wave's current ticket: the first ...
  unsigned int chunk_left = 0u;      // ... and how many
  // wave-uniform: the counter this wave draws from next, and how many counters it has found exhausted (all: no work left)
  // (the compiler cannot know that threadIdx.x >> 6 is wave-uniform: the counter, the chunk bounds and the branches on them live in vector
  // registers.  Telling it -- readfirstlane -- moves them to scalar registers the kernel does not have: 11 more spills, CIRS 3 % slower.)
  unsigned int walk = (blockIdx.x * (unsigned int)(kPoolBlock / 64) + (threadIdx.x >> 6)) % (unsigned int)kNumCounters;
  const int nmat = A.nmat;
  int hold = 0;  // wave-uniform: keep flying while more than `hold` lanes are in flight
  // the register history does not satisfy pred but a parked one does: exchange them (the first such slot)
  auto swap_in = [&](auto pred) {
    if (pred(phase)) return;
    int j = -1;
#pragma unroll
    for (int k = kParked - 1; k >= 0; --k) j = pred(phS[k]) ? k : j;
    if (j < 0) return;
    unsigned int* sp = slot[0];
    int ps = phS[0];
#pragma unroll
    for (int k = 1; k < kParked; ++k) if (j == k) { sp = slot[k]; ps = phS[k]; }
    exchange_history<kSlotStride>(sp, h, 0u);  // phases travel in registers
#pragma unroll
    for (int k = 0; k < kParked; ++k) if (j == k) phS[k] = phase;
    phase = ps;
    mc_old = -1;
    negl2 = -0.69314718055994531f * h.mfpW;
  };

  // Parked histories belong to the WAVE, not to a lane: a lane's slots are pointers.  Lanes that hold no history of the kind
  // `pred` (neither in registers nor parked) trade a slot with lanes that hold two or more, pairing the k-th of the one kind with
  // the k-th of the other -- six cross-lane permutes, no history is moved -- so that afterwards min(64, histories of that kind)
  // lanes hold one (with more than one parked history per lane: after kParked rounds at most; one round is run).  Within the wave
  // the slots stay a permutation of its 64 * kParked columns.
  auto trade_slots = [&](auto pred) {
    const int c = count(pred);
    const bool taker = c == 0;
    const bool donor = c >= 2;
    const unsigned long long m_t = __ballot(taker), m_d = __ballot(donor);
    const int n_pair = min(__popcll(m_t), __popcll(m_d));
    if (n_pair == 0) return;
    const int lane = (int)(threadIdx.x & 63u);
    auto rank_in = [](unsigned long long m) { return (int)__builtin_amdgcn_mbcnt_hi((unsigned int)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)m, 0u)); };
    const int r_t = rank_in(m_t), r_d = rank_in(m_d);
    const bool is_t = taker && r_t < n_pair, is_d = donor && r_d < n_pair;
    const unsigned long long s_t = __ballot(is_t), s_d = __ballot(is_d);
    // lane j < n_pair learns the lane number of the j-th taker / donor: a forward permute in which the selected lanes send
    // to their rank and everybody else to the remaining positions (a full permutation: no two senders collide)
    const int to_t = is_t ? r_t : n_pair + rank_in(~s_t), to_d = is_d ? r_d : n_pair + rank_in(~s_d);
    const int lane_of_t = __builtin_amdgcn_ds_permute(to_t << 2, lane), lane_of_d = __builtin_amdgcn_ds_permute(to_d << 2, lane);
    const int from = (is_t ? r_t : (is_d ? r_d : lane)) << 2;
    const int d_of_me = __builtin_amdgcn_ds_bpermute(from, lane_of_d), t_of_me = __builtin_amdgcn_ds_bpermute(from, lane_of_t);
    const int partner = is_t ? d_of_me : (is_d ? t_of_me : lane);
    // the slot this lane offers: a donor its first parked history of the kind, a taker its first slot (none of its slots is)
    int jo = 0;
#pragma unroll
    for (int k = kParked - 1; k >= 0; --k) jo = (donor && pred(phS[k])) ? k : jo;
    unsigned int* sp = slot[0];
    int ps = phS[0];
#pragma unroll
    for (int k = 1; k < kParked; ++k) if (jo == k) { sp = slot[k]; ps = phS[k]; }
    const unsigned int my_slot = (unsigned int)(reinterpret_cast<unsigned char*>(sp) - lds_raw);
    const unsigned int new_slot = (unsigned int)__builtin_amdgcn_ds_bpermute(partner << 2, (int)my_slot);
    ps = __builtin_amdgcn_ds_bpermute(partner << 2, ps);
    sp = reinterpret_cast<unsigned int*>(lds_raw + new_slot);
#pragma unroll
    for (int k = 0; k < kParked; ++k) if (jo == k) { slot[k] = sp; phS[k] = ps; }
    STAT_ADD(22, n_pair);
  };

  for (;;) {
    // kSegmentLoop (tissue volumes: many steps cross a material boundary and ask the cross-section brackets): the flight segment is
    // an inner loop of its own, so that what every step re-uses -- the bracket row of the history's energy bin, table bases -- is
    // computed once per segment and stays in registers (thorax +2.7 ... 4.5 %, CIRS +0.7 %).  Plastics (few boundary steps, segments
    // of three iterations) do not repay that set-up: there the step stays part of the main loop (Catphan -1 % otherwise).  The host
    // chooses (TrackArgs::segment_loop: tile records, or materials of 20 and more electron shells on average): profiles/r05d_*, r05i_*.
    unsigned long long fR;
    do {
      flight_iteration<VK>(A, h, phase, mc_old, negl2, hi_x, hi_y, hi_z, nmat, st);
      fR = __ballot(phase == PH_FLIGHT);
    } while (kSegmentLoop && __popcll(fR) > hold);
    if (!kSegmentLoop && __popcll(fR) > hold) continue;

    // ------------------------------------------------------------------ scheduling point
    // (0) the kind of the real interactions parked since
    //     the last scheduling point is drawn (one 32-byte record per lane, all lanes' loads in flight together).
    //     REAL lives in registers only and is settled here, before any exchange (HOP waits for the tally + source service).
#if MC_STATS
    const unsigned long long t_sp = __builtin_readcyclecounter();
#endif
    // the scheduler's parameters: one scalar load of six adjacent words, requested before the records below so that its
    // latency passes together with theirs
    const int t_compton = COLD(A)->thresh_compton, t_rayleigh = COLD(A)->thresh_rayleigh, t_new = COLD(A)->thresh_new;
    const int flyable_low = COLD(A)->flyable_low, swap_batch = COLD(A)->swap_batch;
    // Round 6: a history that ends a step in the homogeneous exterior (HOP) is no longer moved here, at whatever handful of lanes
    // each scheduling point finds (thorax: about 11 of 64), but in the tally + source service, whose batches are full -- most of
    // them leave the volume there and are scored in the same pass.  HOP is a parkable phase like the others.
    // (Measured and not kept: moving them here after all when a scheduling point finds a quorum of them -- 24 ... 48 lanes, the Catphan
    // in its 512^3 of air has 40 -- is within the run-to-run noise of never doing so on all three workloads: profiles/r06c_*.)
    if (phase == PH_REAL) {
      const float4* rec = real_record(A, h);
      classify_real(A, h, phase, rec[0], rec[1]);
    }
#if MC_STATS
    st[30] += __builtin_readcyclecounter() - t_sp;  // settle: HOP / REAL
#endif
    // histories of each kind in the wave's pool.  A batch serves one history per lane; slot trading brings min(64, histories) lanes
    // to hold one.
    const int trade = COLD(A)->trade_slots;
    const int n_fly = wave_count([](int p) { return p == PH_FLIGHT; });
    const int h_compton = wave_count([](int p) { return in_compton(p); });
    const int h_rayleigh = wave_count([](int p) { return p == PH_RAYLEIGH; });
    const int h_new = wave_count([](int p) { return wants_service(p); });
    if ((n_fly | h_compton | h_rayleigh | h_new) == 0) break;
    const bool drain = n_fly < flyable_low;
    // few lanes can fly: service the pending kinds, the well-populated ones only (a kind with a handful of lanes
    // waits for company unless it is all there is)
    // lanes a batch of each kind would serve: min(64, histories) once slots have been traded (step 4 and the services' own trades);
    // without trading (MCGPU_SLOT_TRADE bit 1 clear) only the lanes that hold such a history themselves
    auto lanes_with = [&](auto pred) { return __popcll(__ballot(pred(phase) || parked(pred))); };
    const bool trades = (trade & 2) != 0;
    const int n_compton = trades ? min(h_compton, 64) : lanes_with([](int p) { return in_compton(p); });
    const int n_rayleigh = lanes_with([](int p) { return p == PH_RAYLEIGH; });  // the Rayleigh service never trades
    const int n_new = trades ? min(h_new, 64) : lanes_with([](int p) { return wants_service(p); });
    const int n_most = max(n_compton, max(n_rayleigh, n_new));
    STAT_ADD(8, 1);
    STAT_ADD(11, drain ? 1 : 0);

    // (1) Compton: one pass for the lanes with an event in R or S (serve_compton)
    if (n_compton != 0 && ((drain && 2 * n_compton >= n_most) || n_compton >= t_compton)) {
      STAT_ADD(2, 1);
      STAT_ADD(3, n_compton);
      STAT_T0();
      if (trade & 2) trade_slots([](int p) { return in_compton(p); });
      swap_in([](int p) { return in_compton(p); });
      serve_compton(A, h, phase, mc_old, negl2, st);
      STAT_T1(12);
    }
    // (2) Rayleigh (K.cu:329-347)
    if (n_rayleigh != 0 && ((drain && 2 * n_rayleigh >= n_most) || n_rayleigh >= t_rayleigh)) {
      STAT_ADD(4, 1);
      STAT_ADD(5, n_rayleigh);
      STAT_T0();
      swap_in([](int p) { return p == PH_RAYLEIGH; });
      serve_rayleigh(A, h, phase);
      STAT_T1(13);
    }
    // (3) escaped photons -> detector; finished histories -> next history id
    if (n_new != 0 && ((drain && 2 * n_new >= n_most) || n_new >= t_new)) {
      STAT_ADD(6, 1);
      STAT_ADD(7, n_new);
      STAT_T0();
      if (trade & 2) trade_slots([](int p) { return wants_service(p); });
      swap_in([](int p) { return wants_service(p); });
      // histories waiting in the exterior cross it with one exact free-path sample: ESCAPED (scored below, in this pass), back in
      // FLIGHT at the object region's entry point, or a REAL interaction in the background material (its kind is drawn at once:
      // REAL lives in registers only)
      if (phase == PH_HOP) {
        exterior_hop(A, h, phase, exterior_record(A, h.index));
        if (phase == PH_REAL) {
          const float4* rec = real_record(A, h);
          classify_real(A, h, phase, rec[0], rec[1]);
        }
      }
      int tally_word;  // word of the detector tally this lane scores in (-1: none); the hit is scored at the end of the batch
      unsigned int tally_value;
      score_finished(A, h, phase, tally_word, tally_value);
      const unsigned long long my_id = deal_history_ids(A, phase, chunk_next, chunk_left, walk);
      start_history(A, h, phase, mc_old, negl2, my_id, walk);
      // One scattered 64-bit add per detected photon, executed at the memory side, was the wall of the Catphan launch: 7.5e7 of them
      // at 2.37e10/s = 3.18 ms of a 3.67 ms launch, whatever the kernel around them did (round-2 experiment, DESIGN.md 3.1: without
      // the add 17 % faster, a plain store in its place 15 %, a 32-bit add 4 %; issuing it later changes nothing).  The hit is now
      // STAGED (tally_score: an LDS add for its slot + one plain 8-byte store) and folded into the image after the kernel
      // (tally_fold.hip); the add remains for a full block and for launches without staging (profiles/tally_stage_ab.md).
      if (tally_word >= 0) tally_score(A, tally_word, tally_value);
      STAT_T1(14);
    }
    // (4) lanes that hold no flyable history get the spare one of a lane that holds two (trade_slots); measured before this
    //     step existed: after a scheduling point 25 of 64 lanes had nothing to fly while 14 held two flyable histories
    //     (Catphan workload)
    if (trade & 1) trade_slots([](int p) { return p == PH_FLIGHT; });
    //     lanes whose register history is parked take their slot history if that one can fly
    {
      const bool take = (phase != PH_FLIGHT) && parked([](int p) { return p == PH_FLIGHT; });
      const unsigned long long w_take = __ballot(take);
      if (w_take != 0ULL) {
        STAT_ADD(9, 1);
        STAT_ADD(10, __popcll(w_take));
        swap_in([](int p) { return p == PH_FLIGHT; });
      }
    }
    const int flying_now = __popcll(__ballot(phase == PH_FLIGHT));
#if MC_STATS
    STAT_ADD(19, wave_count([](int p) { return p == PH_FLIGHT; }));
    STAT_ADD(20, wave_count([](int p) { return wants_service(p); }));
    STAT_ADD(21, wave_count([](int p) { return in_compton(p); }));
#endif
    // the next scheduling point comes after `swap_batch` more lanes have parked, and no later than when all but
    // hold_q/16 of the lanes that fly now have (a segment that starts thin would otherwise run until its last lane parks)
    hold = max((flying_now > swap_batch) ? flying_now - swap_batch : 0, (flying_now * ((trade >> 8) & 15)) >> 4);
#if MC_STATS
    st[31] += __builtin_readcyclecounter() - t_sp;  // whole scheduling point (settle + services + exchanges)
#endif
  }
  finish_workgroup(A);
#if MC_STATS
  if ((threadIdx.x & 63) == 0 && A.stats != nullptr)
    for (int k = 0; k < kNumStats; ++k) atomicAdd(A.stats + k, st[k]);
  {
    const unsigned int w = blockIdx.x * (kPoolBlock / 64) + (threadIdx.x >> 6);
    if ((threadIdx.x & 63) == 0 && A.stats != nullptr && w < (unsigned int)kWaveTrace) {
      A.stats[kNumStats + 3 * w + 2] = __builtin_amdgcn_s_memrealtime();
      // shader cycles this wave lived (>> 8) in bits 36..63 of word 0: with the two constant-rate stamps -> the clock
      A.stats[kNumStats + 3 * w + 0] |= ((__builtin_readcyclecounter() - t_wave0) >> 8) << 36;
    }
  }
#endif
}

// ================================================================================================
// Workgroup-level pool (round 5): the same physics, scheduled per WORKGROUP instead of per wave.
//
// The per-wave pool above runs its batches with whatever its own 128 histories offer: Compton batches at 40-51 of 64 lanes,
// Rayleigh batches at 9, tally + source batches at 41-47, flight segments that start at about 58 (profiles/r04x_fast_section_stats.txt).
// Here a lane owns ONE history (registers); the 1024 LDS slots of the workgroup hold the parked ones and belong to nobody.  Per
// kind of work {flight, Compton, Rayleigh, tally + source} a ring of slot ids lists the slots whose history waits for it.  A wave
// cycles through
//   settle (HOP / REAL of the last flight segment)  ->  choose a task  ->  exchange  ->  run the task on the lanes that hold its kind
// where "exchange" pops as many slot ids of the task's kind as the wave has lanes holding something else, swaps register and slot
// history in place (ds_wrxchg, as before), and pushes each slot id to the ring of the kind that now sits in it.  A service runs
// when the wave's own histories of that kind plus the ring fill (nearly) 64 lanes -- decided atomically by the pop itself -- so
// batches are full whatever the mix of one wave is; flight segments start with 64 lanes.  Waves specialise by themselves: whoever
// finds a full batch of some kind runs it.  One RNG stream per history, integer tallies: the image is the per-wave kernel's bit for bit.
//
// Rings (multi-producer / multi-consumer, 1024 positions of u16, monotonic 32-bit head / tail per kind):
//   push  tail += n for all four kinds in ONE LDS atomic instruction (lane k serves kind k); then each lane writes its id.
//   pop   compare-and-swap on head against a snapshot of tail (tail only grows: a stale one is conservative); then each lane reads
//         its id and resets the entry to kRingEmpty.  A position may be claimed before its pusher has written it (tail moves at
//         the reservation): the popper waits for the entry to become non-empty -- its pusher is between two adjacent instructions.
//   A pusher writes without looking as long as the ring was less than half full when the wave last looked (at most 1024 ids
//   exist: the position it reserves was popped at least 512 - 64 x 15 ... in practice hundreds of pushes ago, long cleared);
//   above that -- only the tally + source ring at the start of a launch, which begins with every slot id in it -- it first waits
//   for its position to be empty, so a popper that has claimed a position and not yet cleared it is never overwritten.
// Every wait is bounded; a wave that gives up raises the workgroup's panic word and poisons image word 0 (a parity test cannot
// miss it), and the cycle count of a wave is bounded by the launch size: the grid drains whatever happens.
// ================================================================================================
constexpr int kQFly = 0, kQCompton = 1, kQRayleigh = 2, kQNew = 3, kKindNone = 4;
constexpr unsigned int kRingEntries = (unsigned int)kPoolBlock;
constexpr unsigned int kRingEmpty = 0xFFFFu;
constexpr int kCtlHead = 0, kCtlTail = 4, kCtlPanic = 8;
constexpr int kMaxSpin = 1 << 14;
static_assert(kPoolKinds == 4 && kPoolQueueBytes == 64 + 4 * kPoolBlock * 2, "LdsLayout::queues: control block + four rings of u16 slot ids");
// kind of work a history in phase `ph` waits for (settled phases only: REAL / HOP never reach an exchange): nibble ph of the constant
__device__ __forceinline__ int kind_of(int ph) { return (int)((0x1774333210ULL >> (ph << 2)) & 7ULL); }
static_assert(PH_FLIGHT == 0 && PH_COMPTON == 1 && PH_RAYLEIGH == 2 && PH_ESCAPED == 3 && PH_ABSORBED == 4 && PH_NEW == 5 && PH_DONE == 6 &&
                  PH_SHELL == 9, "kind_of: the nibble table is written for these phase numbers");

template <int VK>
__global__ __launch_bounds__(kPoolBlock, kPoolWavesPerSimd) void track_wg_kernel(const TrackArgs A) {
  [[maybe_unused]] Stats st;
  unsigned int* const ctl = reinterpret_cast<unsigned int*>(lds_raw + A.lds.queues);
  unsigned short* const rings = reinterpret_cast<unsigned short*>(lds_raw + A.lds.queues + 64);
  unsigned int* const slots = reinterpret_cast<unsigned int*>(lds_raw + A.lds.slots);
  {  // every slot holds a NEW history (no state), every slot id waits in the tally + source ring
    const unsigned int t = threadIdx.x;
#pragma unroll
    for (int f = 0; f < kSlotWords; ++f) slots[f * kPoolBlock + t] = (f == 10) ? ((unsigned int)PH_NEW << 28) : 0u;
    rings[kQFly * kRingEntries + t] = (unsigned short)kRingEmpty;
    rings[kQCompton * kRingEntries + t] = (unsigned short)kRingEmpty;
    rings[kQRayleigh * kRingEntries + t] = (unsigned short)kRingEmpty;
    rings[kQNew * kRingEntries + t] = (unsigned short)t;
    if (t < 16u) ctl[t] = (t == (unsigned int)(kCtlTail + kQNew)) ? kRingEntries : 0u;
  }
  stage_cursors_clear(A);
  stage_tables<is_u8(VK) ? (int)kVolU8 : VK>(A);  // ends with the workgroup barrier

  History h;
  int phase = PH_NEW;
  int mc_old = -1;
  float negl2 = 0.f;
  const float hi_x = A.bbox_hi[0], hi_y = A.bbox_hi[1], hi_z = A.bbox_hi[2];
  unsigned long long chunk_next = 0;
  unsigned int chunk_left = 0u;
  // (readfirstlane: threadIdx.x >> 6 is the same in every lane of a wave, which the compiler cannot know -- without it the counter, the chunk
  // bounds and every branch on them live in vector registers and run as divergent code)
  unsigned int walk = (unsigned int)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * (unsigned int)(kPoolBlock / 64) + (threadIdx.x >> 6)) % (unsigned int)kNumCounters));
  const int nmat = A.nmat;
  const int lane = (int)(threadIdx.x & 63u);
  auto rank_in = [](unsigned long long m) { return (int)__builtin_amdgcn_mbcnt_hi((unsigned int)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)m, 0u)); };
  auto uniform = [](unsigned int v) { return (unsigned int)__builtin_amdgcn_readfirstlane((int)v); };
  // cycles of one wave: about 0.1 per history of its share of the launch; 64 times that (and a floor for small launches) is never
  // reached by a healthy run and ends a sick one
  const unsigned long long share = LARG(A, count) / ((unsigned long long)gridDim.x * (unsigned long long)(kPoolBlock / 64)) + 1ULL;
  const unsigned int max_cycles = (unsigned int)min(share * 64ULL + 4096ULL, (unsigned long long)(1u << 26));
  int finished = 0;  // wave-uniform: the loop ended because no work is left (not by a bound, not by a panic)
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

  for (unsigned int cycle = 0; cycle < max_cycles; ++cycle) {
#if MC_STATS
    const unsigned long long t_sp = __builtin_readcyclecounter();
#endif
    // the rings' heads and tails: requested before the settling step's records so that the two latencies pass together
    const u32x4 hd = *reinterpret_cast<const volatile u32x4*>(ctl + kCtlHead);  // every lane reads the same bytes (a broadcast)
    const u32x4 tl = *reinterpret_cast<const volatile u32x4*>(ctl + kCtlTail);
    const unsigned int panic = *reinterpret_cast<const volatile unsigned int*>(ctl + kCtlPanic);
    // ------------------------------------------------------------------ (0) settle the last flight segment's HOP / REAL histories
    if (__ballot(phase == PH_HOP || phase == PH_REAL) != 0ULL) {
      float2 t_ext = make_float2(0.f, 0.f);
      float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0;
      const bool was_real = (phase == PH_REAL);
      if (phase == PH_HOP) t_ext = exterior_record(A, h.index);
      if (was_real) { const float4* rec = real_record(A, h); r0 = rec[0]; r1 = rec[1]; }
      if (phase == PH_HOP) exterior_hop(A, h, phase, t_ext);
      if (phase == PH_REAL) {
        if (!was_real) { const float4* rec = real_record(A, h); r0 = rec[0]; r1 = rec[1]; }  // interaction in the background (rare)
        classify_real(A, h, phase, r0, r1);
      }
    }
#if MC_STATS
    st[30] += __builtin_readcyclecounter() - t_sp;
#endif
    if (uniform(panic) != 0u) break;
    // ------------------------------------------------------------------ (1) choose the task
    const int t_compton = COLD(A)->thresh_compton, t_rayleigh = COLD(A)->thresh_rayleigh, t_new = COLD(A)->thresh_new;
    const int fly_low = COLD(A)->flyable_low, swap_batch = COLD(A)->swap_batch, hold_q = (COLD(A)->trade_slots >> 8) & 15;
    unsigned int head_fly = uniform(hd.x), head_compton = uniform(hd.y), head_rayleigh = uniform(hd.z), head_new = uniform(hd.w);
    const unsigned int tail_fly = uniform(tl.x), tail_compton = uniform(tl.y), tail_rayleigh = uniform(tl.z), tail_new = uniform(tl.w);
    const int q_fly = max((int)(tail_fly - head_fly), 0), q_compton = max((int)(tail_compton - head_compton), 0);
    const int q_rayleigh = max((int)(tail_rayleigh - head_rayleigh), 0), q_new = max((int)(tail_new - head_new), 0);
    // rings a pusher must not write into without looking (see above): half full now, i.e. short of kRingLoose by four whole pushes
    const int careful = (q_fly >= 512 ? 1 : 0) | (q_compton >= 512 ? 2 : 0) | (q_rayleigh >= 512 ? 4 : 0) | (q_new >= 512 ? 8 : 0);
    const int o_fly = __popcll(__ballot(phase == PH_FLIGHT)), o_compton = __popcll(__ballot(in_compton(phase)));
    const int o_rayleigh = __popcll(__ballot(phase == PH_RAYLEIGH)), o_new = __popcll(__ballot(wants_new(phase)));
    const int f_fly = min(o_fly + q_fly, 64), f_compton = min(o_compton + q_compton, 64);
    const int f_rayleigh = min(o_rayleigh + q_rayleigh, 64), f_new = min(o_new + q_new, 64);
    int task, need;  // need: lanes the batch must fill to be worth running (0: whatever there is)
    [[maybe_unused]] bool drain = false;
    if (f_compton >= t_compton) { task = kQCompton; need = t_compton; }
    else if (f_new >= t_new) { task = kQNew; need = t_new; }
    else if (f_rayleigh >= t_rayleigh) { task = kQRayleigh; need = t_rayleigh; }
    else if (f_fly >= fly_low) { task = kQFly; need = 0; }
    else {
      // nothing fills a batch (the launch's beginning and end): the fullest kind, partial
      const int best = max(max(f_fly, f_compton), max(f_rayleigh, f_new));
      if (best == 0) { finished = 1; break; }  // every history of this wave is DONE and no ring holds work
      task = (f_fly == best) ? kQFly : ((f_compton == best) ? kQCompton : ((f_new == best) ? kQNew : kQRayleigh));
      need = 0;
      drain = true;
    }
    STAT_ADD(8, 1);
    STAT_ADD(11, drain ? 1 : 0);
    STAT_ADD(19, q_fly);
    STAT_ADD(20, q_new);
    STAT_ADD(21, q_compton);
    // ------------------------------------------------------------------ (2) exchange: lanes that hold another kind take a slot of the task's kind
    {
      int my_kind = kind_of(phase);
      unsigned long long m_t = __ballot(my_kind != task);
      int got = 0;
      unsigned int h0 = 0u;
      // pop: compare-and-swap on the ring's head.  A service whose batch would stay below `need` (another wave was faster) is
      // given up for a flight segment -- flying needs no quorum -- in this same cycle.
      for (int attempt = 0; attempt < 2; ++attempt) {
        const int own = 64 - __popcll(m_t);
        unsigned int head = (task == kQFly) ? head_fly : ((task == kQCompton) ? head_compton : ((task == kQRayleigh) ? head_rayleigh : head_new));
        const unsigned int tail = (task == kQFly) ? tail_fly : ((task == kQCompton) ? tail_compton : ((task == kQRayleigh) ? tail_rayleigh : tail_new));
        bool enough = true;
        for (int tries = 0; tries < 16; ++tries) {
          const int n = min(max((int)(tail - head), 0), 64 - own);
          enough = own + n >= need;
          if (!enough || n == 0) break;
          unsigned int prev = 0u;
          if (lane == 0) prev = atomicCAS(ctl + kCtlHead + task, head, head + (unsigned int)n);
          prev = uniform(prev);
          if (prev == head) { got = n; h0 = head; break; }
          head = prev;  // another wave popped this ring in between
        }
        if (enough || task == kQFly) break;
        task = kQFly; need = 0;  // the quorum is gone
        m_t = __ballot(my_kind != task);
      }
      const int r_t = rank_in(m_t);
      const bool swaps = (my_kind != task) && r_t < got;
      // push, reservation: the lanes that will park their history, per kind; lane k < 4 adds kind k's count to its tail (one
      // LDS atomic instruction for all four rings), in flight together with the read of the popped ids
      unsigned int t_res = 0u;
      int rank_mine = 0;  // rank among the lanes that push to the same ring
      {
        const unsigned long long p_fly = __ballot(swaps && my_kind == kQFly), p_compton = __ballot(swaps && my_kind == kQCompton);
        const unsigned long long p_rayleigh = __ballot(swaps && my_kind == kQRayleigh), p_new = __ballot(swaps && my_kind == kQNew);
        const int n_mine = (lane == 0) ? __popcll(p_fly) : ((lane == 1) ? __popcll(p_compton) : ((lane == 2) ? __popcll(p_rayleigh) : __popcll(p_new)));
        if (lane < kPoolKinds && n_mine != 0) t_res = atomicAdd(ctl + kCtlTail + lane, (unsigned int)n_mine);
        rank_mine = rank_in((my_kind == kQFly) ? p_fly : ((my_kind == kQCompton) ? p_compton : ((my_kind == kQRayleigh) ? p_rayleigh : p_new)));
      }
      unsigned int id = kRingEmpty;
      if (swaps) {
        volatile unsigned short* const e_pop = rings + (unsigned int)task * kRingEntries + ((h0 + (unsigned int)r_t) & (kRingEntries - 1u));
        id = *e_pop;
        for (int spin = 0; id == kRingEmpty && spin < kMaxSpin; ++spin) {  // its pusher is between reserving and writing
          __builtin_amdgcn_s_sleep(1);
          id = *e_pop;
        }
        if (id == kRingEmpty) {
          *reinterpret_cast<volatile unsigned int*>(ctl + kCtlPanic) = 0x10000u | ((unsigned int)task << 12) | ((h0 + (unsigned int)r_t) & (kRingEntries - 1u));
          my_kind = kKindNone;  // nothing was parked
        } else {
          *e_pop = (unsigned short)kRingEmpty;
          phase = (int)exchange_history<kPoolBlock>(slots + id, h, (unsigned int)phase);  // the slot's phase travels in the packed word
          mc_old = -1;
          negl2 = -0.69314718055994531f * h.mfpW;
        }
      }
      STAT_ADD(9, 1);
      STAT_ADD(10, got);
      // push, the ids: position = the ring's reservation (held by lane `kind`) + rank among the lanes of the same kind
      const unsigned int t0 = (unsigned int)__builtin_amdgcn_ds_bpermute((my_kind & 3) << 2, (int)t_res);
      if (swaps && my_kind < kPoolKinds) {  // (a DONE history's slot leaves the circulation)
        const unsigned int pos = t0 + (unsigned int)rank_mine;
        volatile unsigned short* const e = rings + (unsigned int)my_kind * kRingEntries + (pos & (kRingEntries - 1u));
        if ((careful >> my_kind) & 1) {  // the ring may be nearly full: the position's last popper must have cleared it
          int spin = 0;
          while (*e != kRingEmpty && spin < kMaxSpin) { __builtin_amdgcn_s_sleep(1); ++spin; }
          if (spin >= kMaxSpin) *reinterpret_cast<volatile unsigned int*>(ctl + kCtlPanic) = 0x20000u | ((unsigned int)my_kind << 12) | (pos & (kRingEntries - 1u));
        }
        *e = (unsigned short)id;
      }
    }
#if MC_STATS
    st[31] += __builtin_readcyclecounter() - t_sp;
#endif
    // ------------------------------------------------------------------ (3) the task, on the lanes that hold its kind
    if (task == kQFly) {
      // Woodcock flight steps (K.cu:249-279) until all but `hold` of the lanes that fly now have parked
      const int flying_now = __popcll(__ballot(phase == PH_FLIGHT));
      const int hold = max((flying_now > swap_batch) ? flying_now - swap_batch : 0, (flying_now * hold_q) >> 4);
      unsigned long long fR;
      do {
        flight_iteration<VK>(A, h, phase, mc_old, negl2, hi_x, hi_y, hi_z, nmat, st);
        fR = __ballot(phase == PH_FLIGHT);
      } while (__popcll(fR) > hold);
    } else if (task == kQCompton) {
      STAT_ADD(2, 1);
      STAT_ADD(3, __popcll(__ballot(in_compton(phase))));
      STAT_T0();
      serve_compton(A, h, phase, mc_old, negl2, st);
      STAT_T1(12);
      STAT_T1(31);
    } else if (task == kQRayleigh) {
      STAT_ADD(4, 1);
      STAT_ADD(5, __popcll(__ballot(phase == PH_RAYLEIGH)));
      STAT_T0();
      serve_rayleigh(A, h, phase);
      STAT_T1(13);
      STAT_T1(31);
    } else {
      // escaped photons -> detector; finished histories -> next history id (K.cu:206-247, 350-375)
      STAT_ADD(6, 1);
      STAT_ADD(7, __popcll(__ballot(wants_new(phase))));
      STAT_T0();
      int tally_word;
      unsigned int tally_value;
      score_finished(A, h, phase, tally_word, tally_value);
      const unsigned long long my_id = deal_history_ids(A, phase, chunk_next, chunk_left, walk);
      start_history(A, h, phase, mc_old, negl2, my_id, walk);
      if (tally_word >= 0) tally_score(A, tally_word, tally_value);
      STAT_T1(14);
      STAT_T1(31);
    }
  }
  if (finished == 0 && lane == 0) {
    atomicAdd(A.image, 1ULL << 62);  // never silent: the tally is unusable and every check sees it
#ifdef MC_WG_DEBUG
    const unsigned int pn = *reinterpret_cast<const volatile unsigned int*>(ctl + kCtlPanic);
    atomicAdd(A.image + 1, pn ? 1ULL : (1ULL << 32));           // low: waves ended by panic, high: by the cycle bound
    for (int k = 0; k < 8; ++k) A.image[2 + k] = ((unsigned long long)blockIdx.x << 40) | ctl[k];   // heads and tails of the four rings
    A.image[14] = pn;
#endif
  }
  finish_workgroup(A);
#if MC_STATS
  if ((threadIdx.x & 63) == 0 && A.stats != nullptr)
    for (int k = 0; k < kNumStats; ++k) atomicAdd(A.stats + k, st[k]);
#endif
}


// LARG / SRC / DET (track_common.inc) read the kernel-argument segment as ONE TrackArgs at offset 0: every kernel of this file that
// reaches sample_source, tally_pixel or the id dispenser must take exactly that, by value, as its only parameter.
template <typename K> struct kernel_signature;
template <typename P> struct kernel_signature<void (*)(P)> { typedef P only_parameter; };
static_assert(std::is_same<kernel_signature<decltype(&track_pool_kernel<kVolU8, false>)>::only_parameter, TrackArgs>::value &&
                  std::is_same<kernel_signature<decltype(&track_wg_kernel<kVolU8>)>::only_parameter, TrackArgs>::value,
              "the FAST kernels' only parameter is a TrackArgs by value (LARG reads the kernel-argument segment at offset 0)");

}  // namespace

// host-side launchers of this personality: this translation unit's entry of the table of FAST kernels (device_model.hpp)
namespace {
typedef void (*TrackKernel)(const TrackArgs);
template <int VK>
TrackKernel pick(bool wg, bool seg) {
  return wg ? track_wg_kernel<VK> : (seg ? track_pool_kernel<VK, true> : track_pool_kernel<VK, false>);
}
TrackKernel pick_kernel(const TrackArgs& args) {
  const bool wg = args.sched_kind == 1, seg = args.segment_loop != 0;
  switch (args.vol_kind) {
    case kVolU8: return args.sub_kind == 2 ? pick<kVolU8Rec>(wg, seg) : (args.sub_kind == 1 ? pick<kVolU8Sub>(wg, seg) : pick<kVolU8>(wg, seg));
    case kVolU16: return pick<kVolU16>(wg, seg);
    default: return pick<kVolRaw>(wg, seg);
  }
}
// resident workgroups per CU for this kernel variant (persistent grids must not over-subscribe)
int occupancy(const TrackArgs& args) {
  int n = 0;
  const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, pick_kernel(args), kPoolBlock, (size_t)args.lds.total);
  return (e == hipSuccess && n > 0) ? n : 1;
}
hipError_t launch(const TrackArgs& args, int blocks, hipStream_t stream) {
  hipLaunchKernelGGL(pick_kernel(args), dim3((unsigned)blocks), dim3(kPoolBlock), (size_t)args.lds.total, stream, args);
  return hipGetLastError();
}
}  // namespace
template <>
const FastKernels& fast_kernels<MC_FAST_F64, MC_TALLY_W2, MC_STATS>() {
  static const FastKernels table = {launch, occupancy};
  return table;
}

}  // namespace mcgpu
