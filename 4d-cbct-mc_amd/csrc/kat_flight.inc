// kat_flight.inc -- known-answer hook of the middle of a FAST history, the Woodcock flight step (mcgpu_kat_flight; tests/test_flight_gpu.py).
// Included at the end of track_fast.hip and track_fast64.hip (from the tail of kat_history.inc): ONE kernel text, compiled in both
// arithmetics and in all five kernel variants {kVolU8, kVolU8Sub, kVolU8Rec, kVolU16, kVolRaw}, that calls the functions the two
// schedulers call -- flight_locate, flight_steps (flight_locate + flight_resolve), real_record and classify_real -- on one item per
// thread, from a stream the test can replay (oracle/fast_rng.py).  Every history takes 10 to 25 of these steps; a detector image shows
// a decode slip in a rare tile record, a bracket that misses its cross section in one bin or an index slip at a voxel face as a sliver
// of its noise.
//
//   kind kKatLookup  in8 = {x, y, z, ...}: flight_locate with step 0 from that point, then the palette read of flight_resolve through the
//                    same StepSite; no deviate is drawn.  out[8 i ..] = {bits(density), compact material, s.e, s.raw, out, exterior, variant, 0}
//   kind kKatFlight  in8 = {x, y, z, u, v, w, E, -}, in_u64 = history id: the history as start_history / swap_in leave it (energy bin, coarse
//                    majorant, negl2, mc_old = -1, aux = 0, the stream of the id), then flight_steps while the phase is FLIGHT, at most
//                    max_steps times; a history that ends REAL draws its kind (real_record + classify_real).
//                    out[(max_steps + 1) 8 i ..]: one row {bits(x), bits(y), bits(z), phase, h.mc, bits(h.aux), rng.x, rng.c} after EVERY step (the
//                    rows of steps not taken stay zero), then {final phase, steps taken, h.index, bits(h.mfpW), rng.x, rng.c, variant, mc_old}
//                    (mc_old, the material whose cross section h.aux caches, -1 for none: the cache rule decides nothing -- the brackets and the
//                    exact table agree by construction -- so a cache that is never filled shows in no other word)
// Launch: one thread per item, kKatBlock threads per workgroup, the LDS image of the production kernels (stage_tables), no dose tally,
// no staging region; nothing is tallied.  The step count is bounded by the argument: the hook cannot spin.
namespace mcgpu {
namespace {
constexpr int kKatLookup = 0, kKatFlight = 1;

// TrackArgs first and by value, as in the production kernels: LARG / KARG read the kernel-argument segment at offset 0
template <int VK>
__global__ __launch_bounds__(kKatBlock) void kat_flight_kernel(const TrackArgs A, int kind, int n, int max_steps, const float* in8,
                                                               const unsigned long long* in_u64, unsigned int* out) {
  stage_tables<is_u8(VK) ? (int)kVolU8 : VK>(A);  // as track_pool_kernel stages; ends with the workgroup's barrier: every thread takes part
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  const float hi_x = A.bbox_hi[0], hi_y = A.bbox_hi[1], hi_z = A.bbox_hi[2];
  const float* p = in8 + 8 * (size_t)i;
  History h;
  h.P.x = p[0]; h.P.y = p[1]; h.P.z = p[2];
  if (kind == kKatLookup) {
    h.P.u = h.P.v = h.P.w = 0.f;
    StepSite s;
    flight_locate<VK>(A, h.P, h.P.x, h.P.y, h.P.z, 0.f, hi_x, hi_y, hi_z, s);
    // the palette read of flight_resolve, through the same StepSite
    float2 pd;
    if (is_u8(VK)) pd = LDS_F2(A.lds.pal)[(s.e == kBrickMixed) ? kPaletteBase + (int)s.raw : s.e];
    else if (VK == kVolU16) pd = ((const float2*)A.palette)[s.raw];
    else pd = s.pd;
    unsigned int* q = out + 8 * (size_t)i;
    q[0] = __float_as_uint(pd.x); q[1] = __float_as_uint(pd.y); q[2] = (unsigned int)s.e; q[3] = s.raw;
    q[4] = s.out ? 1u : 0u; q[5] = s.exterior ? 1u : 0u; q[6] = (unsigned int)VK; q[7] = 0u;
    return;
  }
  h.P.u = p[3]; h.P.v = p[4]; h.P.w = p[5]; h.P.E = p[6];
  h.index = energy_index(A, h.P.E);
  h.mfpW = LDS_F(SLDS(A, wood))[h.index >> kWoodShift];
  const float negl2 = -0.69314718055994531f * h.mfpW;
  h.aux = 0.f;
  int mc_old = -1, phase = PH_FLIGHT, steps = 0;
  rng_init_history(h.rng, in_u64[i], (unsigned int)A.seed, A.stream_key);
  const int nmat = A.nmat;
  unsigned int* q = out + 8 * (size_t)i * (size_t)(max_steps + 1);
  while (phase == PH_FLIGHT && steps < max_steps) {
    bool st_mixed = false, st_sig = false;
    unsigned long long t_loaded = 0;
    flight_steps<VK>(A, h, phase, mc_old, negl2, hi_x, hi_y, hi_z, nmat, st_mixed, st_sig, t_loaded);
    q[0] = __float_as_uint(h.P.x); q[1] = __float_as_uint(h.P.y); q[2] = __float_as_uint(h.P.z); q[3] = (unsigned int)phase;
    q[4] = (unsigned int)h.mc; q[5] = __float_as_uint(h.aux); q[6] = h.rng.x; q[7] = h.rng.c;
    q += 8;
    ++steps;
  }
  if (phase == PH_REAL) {
    const float4* rec = real_record(A, h);
    classify_real(A, h, phase, rec[0], rec[1]);
  }
  q = out + 8 * ((size_t)i * (size_t)(max_steps + 1) + (size_t)max_steps);
  q[0] = (unsigned int)phase; q[1] = (unsigned int)steps; q[2] = (unsigned int)h.index; q[3] = __float_as_uint(h.mfpW);
  q[4] = h.rng.x; q[5] = h.rng.c; q[6] = (unsigned int)VK; q[7] = (unsigned int)mc_old;
}

typedef void (*KatFlightKernel)(const TrackArgs, int, int, int, const float*, const unsigned long long*, unsigned int*);
// pick_kernel's switch (track_pool.inc) on the storage kind and the second level
KatFlightKernel pick_kat_flight(const TrackArgs& args) {
  switch (args.vol_kind) {
    case kVolU8: return args.sub_kind == 2 ? kat_flight_kernel<kVolU8Rec> : (args.sub_kind == 1 ? kat_flight_kernel<kVolU8Sub> : kat_flight_kernel<kVolU8>);
    case kVolU16: return kat_flight_kernel<kVolU16>;
    default: return kat_flight_kernel<kVolRaw>;
  }
}
}  // namespace

#if MC_FAST_F64
#define MC_KAT_FLIGHT_NAME launch_kat_flight_fast64
#else
#define MC_KAT_FLIGHT_NAME launch_kat_flight_fast
#endif
// `args`: make_args() of the context and the projection with dose_flags = 0, first = 0, the seed, no staging region (engine_kat.cpp)
hipError_t MC_KAT_FLIGHT_NAME(const TrackArgs& args, int kind, int n, int max_steps, const float* in8, const unsigned long long* in_u64,
                              unsigned int* out, hipStream_t stream) {
  const dim3 grid((unsigned)((n + kKatBlock - 1) / kKatBlock)), block(kKatBlock);
  hipLaunchKernelGGL(pick_kat_flight(args), grid, block, (size_t)args.lds.total, stream, args, kind, n, max_steps, in8, in_u64, out);
  return hipGetLastError();
}
}  // namespace mcgpu
