// track_fast_w2.hip -- the FAST personality for launches that tally squared weights beside the image (mcgpu_launch_projection_w2):
// track_fast.hip's kernels with the second add of tally_score's direct route compiled in (tally_stage.hpp: the quantity).
#define MC_COMPAT 0
#define MC_TALLY_W2 1
#include "track_pool.inc"
