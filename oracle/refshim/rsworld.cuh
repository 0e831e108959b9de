// Stand-in for the simulator's "rsworld.cuh", which aggregation.cuh includes: the aggregation kernels need only the vector
// types and PerRayData.  No include guard, like ray_tracer.h itself: the harness includes each reference source inside a
// namespace of its own, and each gets its own PerRayData there.
#include "rts_refshim.h"
#include "ray_tracer.h"
