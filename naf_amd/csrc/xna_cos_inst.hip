// One window of the cosine-head MFMA cell kernel (every channel-tile count that fits the LDS).
// Explicit instantiations only; xna_cos.hip declares them extern and dispatches.
#ifndef NAF_KS
#error "compile with -DNAF_KS=<window> (naf_amd/build.py: INSTANCES)"
#endif
#include "xna_cos_kernel.h"

NAF_XNA_COS_WINDOW(, NAF_KS)
