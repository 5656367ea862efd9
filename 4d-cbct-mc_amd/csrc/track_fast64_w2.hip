// track_fast64_w2.hip -- track_fast64.hip's kernels (MCGPU_MODE_FAST_F64) for launches that tally squared weights beside the image
// (mcgpu_launch_projection_w2): the second add of tally_score's direct route compiled in.
#define MC_COMPAT 0
#define MC_FAST_F64 1
#define MC_TALLY_W2 1
#include "track_pool.inc"
