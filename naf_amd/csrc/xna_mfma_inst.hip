// One window of the MFMA cell kernel, bf16 / fp32 (NAF_HALF=0) or half (NAF_HALF=1) values: one object per (window, value type), so the
// build compiles them in parallel.  Explicit instantiations only; xna_mfma.hip declares them extern and dispatches.
#if !defined(NAF_KS) || !defined(NAF_HALF)
#error "compile with -DNAF_KS=<window> -DNAF_HALF=0|1 (naf_amd/build.py: INSTANCES)"
#endif
#include "xna_mfma_kernel.h"

template int xna_mfma_launch_ks<NAF_KS, NAF_HALF != 0>(const XnaMfmaParams&, const XnaMfmaPlan&, int, hipStream_t);
