// Instantiations of the table-driven MFMA attention kernel for kernel_size = 15 with half values and output (NAF_F16).
#include "xna_union_kernel.h"

int naf_xna_union_launch_h_k15(const XnaUnionParams& p, int wt, int out_dtype, size_t lds, hipStream_t s) { return xna_union_launch_ks<15, true>(p, wt, out_dtype, lds, s); }
