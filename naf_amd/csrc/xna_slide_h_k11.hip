// Instantiations of the sliding-window attention kernel for kernel_size = 11 with half values and output (NAF_F16).
#include "xna_slide_kernel.h"

int naf_xna_slide_launch_h_k11(const XnaSlideParams& sp, int dvt, int out_dtype, hipStream_t s) { return xna_slide_launch_ks<11, true>(sp, dvt, out_dtype, s); }
