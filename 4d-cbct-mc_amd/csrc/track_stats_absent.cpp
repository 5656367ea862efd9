// track_stats_absent.cpp -- the product library's entry for the diagnostic FAST kernel (device_model.hpp: FastKernels): it carries
// none (track_stats.hip is linked into libmcgpu_amd_stats.so only), so a MCGPU_MODE_FAST_STATS launch is refused.
#include "engine_internal.hpp"

namespace mcgpu {
static hipError_t refuse(const TrackArgs&, int, hipStream_t) {
  throw Error(-2, "!!ERROR!! mcgpu_launch_projection: MCGPU_MODE_FAST_STATS needs the diagnostic library (libmcgpu_amd_stats.so, MCGPU_AMD_LIB)");
}
template <>
const FastKernels& fast_kernels<0, 1, 1>() {
  static const FastKernels table = {refuse, [](const TrackArgs&) { return 1; }};
  return table;
}
}  // namespace mcgpu
