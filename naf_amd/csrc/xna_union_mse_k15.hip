// Instantiations of the table-driven MFMA attention kernel with the regression objective for kernel_size = 15.
#include "xna_union_mse_kernel.h"

int naf_xna_union_mse_launch_k15(const XnaUnionMseParams& p, int wt, size_t lds, hipStream_t s) { return xna_union_mse_launch_ks<15>(p, wt, lds, s); }
