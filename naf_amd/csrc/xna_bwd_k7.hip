// Instantiations of the attention backward cell kernel for kernel_size = 7 (whole heads at every Dv: xna_bwd.hip).
#include "xna_bwd2_kernel.h"

int naf_xna_bwd_launch_k7(const XnaBwdParams& p, int Dv, hipStream_t s) { return xna_bwd2_launch_ks<7>(p, Dv, s); }
int naf_xna_bwd_scores_launch_k7(const XnaBwdScoresParams& p, int Dv, hipStream_t s) { return xna_bwd2_launch_ks<7, true>(p, Dv, s); }
