// k6_rate_planes.hip -- K6's plane-order instance (fri_hip_estimate_size_tiled420_dev: the tiles of a tiled 4:2:0 file, whose arrays hold the luma planes first),
// compiled from k6_rate.hip's kernels in a module of its own (see launch_rate_estimate_tiled420 there).
#define FRI_K6_PLANE_ORDER_INSTANCE 1
#include "k6_rate.hip"
