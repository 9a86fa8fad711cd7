// One window of the table-driven MFMA kernel, bf16 / fp32 (NAF_HALF=0) or half (NAF_HALF=1) values.
// Explicit instantiations only; xna_union.hip declares them extern and dispatches.
#if !defined(NAF_KS) || !defined(NAF_HALF)
#error "compile with -DNAF_KS=<window> -DNAF_HALF=0|1 (naf_amd/build.py: INSTANCES)"
#endif
#include "xna_union_kernel.h"

template int xna_union_launch_ks<NAF_KS, NAF_HALF != 0>(const XnaUnionParams&, int, int, size_t, hipStream_t);
