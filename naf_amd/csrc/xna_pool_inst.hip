// One window of the mask-pooling cell kernel (bf16 and byte masks) and its gather.
// Explicit instantiations only; xna_pool.hip declares them extern and dispatches.
#ifndef NAF_KS
#error "compile with -DNAF_KS=<window> (naf_amd/build.py: INSTANCES)"
#endif
#include "xna_pool_kernel.h"

NAF_XNA_POOL_WINDOW(, NAF_KS)
