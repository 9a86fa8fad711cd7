// One window of the attention backward cell kernel: the plain backward and the one with a gradient of the scores.
// Explicit instantiations only; xna_bwd.hip declares them extern and dispatches.
#ifndef NAF_KS
#error "compile with -DNAF_KS=<window> (naf_amd/build.py: INSTANCES)"
#endif
#include "xna_bwd2_kernel.h"

template int xna_bwd2_launch_ks<NAF_KS, false>(const XnaBwdParams&, int, hipStream_t);
template int xna_bwd2_launch_ks<NAF_KS, true>(const XnaBwdScoresParams&, int, hipStream_t);
