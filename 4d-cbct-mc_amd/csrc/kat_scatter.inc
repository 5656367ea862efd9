// kat_scatter.inc -- known-answer hook of the FAST personality's scattering samplers (mcgpu_kat_scatter; tests/test_scatter_gpu.py).
// Included at the end of track_fast.hip and track_fast64.hip, behind track_pool.inc: ONE kernel text, compiled in both arithmetics,
// that runs the service bodies the two schedulers run -- serve_compton and serve_rayleigh, with compton_draw, compton_momentum_trial,
// rayleigh_trial and rotate_dir behind them -- on one event per thread, from a stream the test can replay (oracle/fast_rng.py).
// The detector images see these functions only as a small, smooth share of their counts, and an azimuth not at all.
//
//   kind kKatRotate    in4 = {u, v, w, polar argument}, in_u64 = one 32-bit deviate: the direction after rotate_dir (single
//                      precision only: the double one is covered by mcgpu_kat_fast64)
//   kind kKatRayleigh  in4 = {u, v, w, E}, in_u64 = history id, mc = compact material: serve_rayleigh until the phase leaves RAYLEIGH
//   kind kKatCompton   the same with serve_compton until the phase is neither COMPTON nor SHELL
//   out4 = {E', u', v', w'}; out_u4 = {service calls, final phase, generator state x, c}
// Launch: one thread per item, kKatBlock threads per workgroup, the LDS image of the production kernels (stage_tables), no dose tally.
namespace mcgpu {
namespace {
constexpr int kKatBlock = 256;
constexpr int kKatRotate = 0, kKatRayleigh = 1, kKatCompton = 2;
// an event whose trials never succeed would keep its workgroup forever: it ends here instead, and the phase it reports says so
constexpr unsigned int kKatMaxCalls = 1u << 20;

// TrackArgs first and by value, as in the production kernels: LARG / KARG read the kernel-argument segment at offset 0
template <int VK>
__global__ __launch_bounds__(kKatBlock) void kat_scatter_kernel(const TrackArgs A, int kind, int n, unsigned int seed, unsigned int stream_key,
                                                                const float* in4, const unsigned long long* in_u64, const int* mc,
                                                                float* out4, unsigned int* out_u4) {
  stage_tables<VK>(A);  // ends with the workgroup's barrier: every thread takes part, the ones past n included
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  History h;
  h.P.x = h.P.y = h.P.z = 0.f;
  h.P.u = in4[4 * i]; h.P.v = in4[4 * i + 1]; h.P.w = in4[4 * i + 2];
  int phase = PH_FLIGHT;
  unsigned int calls = 0u;
  if (kind == kKatRotate) {
#if !MC_FAST_F64
    // one multiply-with-carry step must produce the deviate: x' = lo(a x + c) with x = 0 gives x' = c
    h.rng.x = 0u; h.rng.c = (unsigned int)in_u64[i];
    rotate_dir(h.P, in4[4 * i + 3], h.rng);
#endif
  } else {
    h.P.E = in4[4 * i + 3];
    h.mc = mc[i];
    h.index = energy_index(A, h.P.E);
    rng_init_history(h.rng, in_u64[i], seed, stream_key);
    int mc_old = -1;
    float negl2 = 0.f;
    [[maybe_unused]] Stats st;
    if (kind == kKatCompton) {
      phase = PH_COMPTON;
      while (in_compton(phase) && calls < kKatMaxCalls) { serve_compton(A, h, phase, mc_old, negl2, st); ++calls; }
    } else {
      phase = PH_RAYLEIGH;
      while (phase == PH_RAYLEIGH && calls < kKatMaxCalls) { serve_rayleigh(A, h, phase); ++calls; }
    }
  }
  out4[4 * i] = h.P.E; out4[4 * i + 1] = h.P.u; out4[4 * i + 2] = h.P.v; out4[4 * i + 3] = h.P.w;
  out_u4[4 * i] = calls; out_u4[4 * i + 1] = (unsigned int)phase; out_u4[4 * i + 2] = h.rng.x; out_u4[4 * i + 3] = h.rng.c;
}
}  // namespace

#if MC_FAST_F64
#define MC_KAT_SCATTER_NAME launch_kat_scatter_fast64
#else
#define MC_KAT_SCATTER_NAME launch_kat_scatter_fast
#endif
// `args`: make_args() of the context with dose_flags = 0 (engine_kat.cpp)
hipError_t MC_KAT_SCATTER_NAME(const TrackArgs& args, int kind, int n, unsigned int seed, unsigned int stream_key, const float* in4,
                               const unsigned long long* in_u64, const int* mc, float* out4, unsigned int* out_u4, hipStream_t stream) {
  const dim3 grid((unsigned)((n + kKatBlock - 1) / kKatBlock)), block(kKatBlock);
  if (args.vol_kind == kVolU8)
    hipLaunchKernelGGL(kat_scatter_kernel<kVolU8>, grid, block, (size_t)args.lds.total, stream, args, kind, n, seed, stream_key, in4, in_u64, mc, out4, out_u4);
  else  // the palette and the brick grid of the other storage kinds are not staged (stage_tables)
    hipLaunchKernelGGL(kat_scatter_kernel<kVolU16>, grid, block, (size_t)args.lds.total, stream, args, kind, n, seed, stream_key, in4, in_u64, mc, out4, out_u4);
  return hipGetLastError();
}
}  // namespace mcgpu

// the sibling hook of the two ends of a history (mcgpu_kat_history), included from here so that both arithmetics get it wherever they
// get this one, and the text of track_fast.hip -- part of the kernel-build stamp of the committed counter summaries -- stays what it was
#include "kat_history.inc"
