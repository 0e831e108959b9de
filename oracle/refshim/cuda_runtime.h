// Stand-in for <cuda_runtime.h>: the reference's device sources include it by this name; everything lives in rts_refshim.h.
#include "rts_refshim.h"
