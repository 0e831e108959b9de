// Stand-in for <optixu/optixu_aabb_namespace.h>: the reference's device sources include it by this name; everything lives in rts_refshim.h.
#include "../rts_refshim.h"
