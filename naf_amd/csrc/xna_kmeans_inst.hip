// One window of the k-means step's cell kernel (K <= 32 and K <= 64) with the pool kernel's gather.
// Explicit instantiations only; xna_kmeans.hip declares them extern and dispatches.
#ifndef NAF_KS
#error "compile with -DNAF_KS=<window> (naf_amd/build.py: INSTANCES)"
#endif
#include "xna_kmeans_kernel.h"

NAF_XNA_KMEANS_WINDOW(, NAF_KS)
