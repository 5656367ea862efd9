// kat_history.inc -- known-answer hook of the two ends of a FAST history (mcgpu_kat_history; tests/test_source_gpu.py): the source with
// its entry into the volume, the detector tally, and the hop across the homogeneous exterior.  Included at the end of track_fast.hip and
// track_fast64.hip (from the tail of kat_scatter.inc): ONE kernel text, compiled in both arithmetics, that calls the functions the two schedulers
// call -- start_history (sample_source_energy, sample_source_direction, source_entry with cylinder_span and entry_face_shell, or
// move_to_bbox, classify_real), score_finished (tally_pixel) and exterior_record + exterior_hop -- on one item per thread, under the pose
// of a projection of the context, from a stream the test can replay (oracle/fast_rng.py).  A whole detector image shows none of this:
// a pixel-boundary slip, a tilted spectrum or a wrong branch of the cylinder test stays far below its noise.
//
//   kind kKatSource  in_u64 = history id: start_history with phase NEW and that id (TrackArgs::first = 0, seed, stream_key = projection)
//   kind kKatTally   in8 = {x, y, z, u, v, w, E, scatter state 0..3}: score_finished with phase ESCAPED
//   kind kKatHop     in8 = {x, y, z, u, v, w, E, -}, in_u64 = history id: exterior_record + exterior_hop, then classify_real when REAL
//   out8 = {E, u, v, w, x, y, z, mfpW}; out_u8 = {final phase, h.index, h.mc, h.scatter, generator state x, c, tally word, tally value}
// Launch: one thread per item, kKatBlock threads per workgroup, the LDS image of the production kernels (stage_tables), no dose tally,
// no staging region.  Nothing is tallied: score_finished hands the word and the value back, the caller's tally_score is not called.
namespace mcgpu {
namespace {
constexpr int kKatSource = 0, kKatTally = 1, kKatHop = 2;

// TrackArgs first and by value, as in the production kernels: LARG / KARG read the kernel-argument segment at offset 0
template <int VK>
__global__ __launch_bounds__(kKatBlock) void kat_history_kernel(const TrackArgs A, int kind, int n, const float* in8, const unsigned long long* in_u64,
                                                                float* out8, unsigned int* out_u8) {
  stage_tables<VK>(A);  // ends with the workgroup's barrier: every thread takes part, the ones past n included
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  History h;
  int phase = PH_NEW, mc_old = -1, tally_word = -1;
  unsigned int tally_value = 0u;
  float negl2 = 0.f;
  if (kind == kKatSource) {
    start_history(A, h, phase, mc_old, negl2, in_u64[i], 0u);
  } else {
    const float* p = in8 + 8 * (size_t)i;
    h.P.x = p[0]; h.P.y = p[1]; h.P.z = p[2]; h.P.u = p[3]; h.P.v = p[4]; h.P.w = p[5]; h.P.E = p[6];
    if (kind == kKatTally) {
      h.scatter = (int)p[7];
      phase = PH_ESCAPED;
      score_finished(A, h, phase, tally_word, tally_value);
    } else {
      h.index = energy_index(A, h.P.E);
      rng_init_history(h.rng, in_u64[i], (unsigned int)A.seed, A.stream_key);
      phase = PH_HOP;
      exterior_hop(A, h, phase, exterior_record(A, h.index));
      if (phase == PH_REAL) {
        const float4* rec = real_record(A, h);
        classify_real(A, h, phase, rec[0], rec[1]);
      }
    }
  }
  float* o = out8 + 8 * (size_t)i;
  o[0] = h.P.E; o[1] = h.P.u; o[2] = h.P.v; o[3] = h.P.w; o[4] = h.P.x; o[5] = h.P.y; o[6] = h.P.z; o[7] = h.mfpW;
  unsigned int* q = out_u8 + 8 * (size_t)i;
  q[0] = (unsigned int)phase; q[1] = (unsigned int)h.index; q[2] = (unsigned int)h.mc; q[3] = (unsigned int)h.scatter;
  q[4] = h.rng.x; q[5] = h.rng.c; q[6] = (unsigned int)tally_word; q[7] = tally_value;
}
}  // namespace

#if MC_FAST_F64
#define MC_KAT_HISTORY_NAME launch_kat_history_fast64
#else
#define MC_KAT_HISTORY_NAME launch_kat_history_fast
#endif
// `args`: make_args() of the context and the projection with dose_flags = 0, first = 0, the seed, no staging region (engine_kat.cpp)
hipError_t MC_KAT_HISTORY_NAME(const TrackArgs& args, int kind, int n, const float* in8, const unsigned long long* in_u64, float* out8,
                               unsigned int* out_u8, hipStream_t stream) {
  const dim3 grid((unsigned)((n + kKatBlock - 1) / kKatBlock)), block(kKatBlock);
  if (args.vol_kind == kVolU8)
    hipLaunchKernelGGL(kat_history_kernel<kVolU8>, grid, block, (size_t)args.lds.total, stream, args, kind, n, in8, in_u64, out8, out_u8);
  else  // the palette and the brick grid of the other storage kinds are not staged (stage_tables)
    hipLaunchKernelGGL(kat_history_kernel<kVolU16>, grid, block, (size_t)args.lds.total, stream, args, kind, n, in8, in_u64, out8, out_u8);
  return hipGetLastError();
}
}  // namespace mcgpu

// the sibling hook of the middle of a history, the Woodcock flight step (mcgpu_kat_flight), included from here for the reason this file
// hangs off kat_scatter.inc: both arithmetics get it, and the text of track_fast.hip stays what it was
#include "kat_flight.inc"
