// One window of the table-driven MFMA kernel with the regression objective in its epilogue.
// Explicit instantiations only; xna_union_mse.hip declares them extern and dispatches.
#ifndef NAF_KS
#error "compile with -DNAF_KS=<window> (naf_amd/build.py: INSTANCES)"
#endif
#include "xna_union_mse_kernel.h"

template int xna_union_mse_launch_ks<NAF_KS>(const XnaUnionMseParams&, int, size_t, hipStream_t);
