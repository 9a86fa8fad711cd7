// One window (7 .. 15) of the persistent sliding-window kernel, bf16 / fp32 (NAF_HALF=0) or half (NAF_HALF=1) values.
// Explicit instantiations only; xna_mfma.hip declares them extern and dispatches.
#if !defined(NAF_KS) || !defined(NAF_HALF)
#error "compile with -DNAF_KS=<window> -DNAF_HALF=0|1 (naf_amd/build.py: INSTANCES)"
#endif
#include "xna_slide_kernel.h"

template int xna_slide_launch_ks<NAF_KS, NAF_HALF != 0>(const XnaSlideParams&, int, int, hipStream_t);
