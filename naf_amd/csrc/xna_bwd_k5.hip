// Instantiations of the attention backward cell kernel for kernel_size = 5 (whole heads at every Dv: xna_bwd.hip).
#include "xna_bwd2_kernel.h"

int naf_xna_bwd_launch_k5(const XnaBwdParams& p, int Dv, hipStream_t s) { return xna_bwd2_launch_ks<5>(p, Dv, s); }
int naf_xna_bwd_scores_launch_k5(const XnaBwdScoresParams& p, int Dv, hipStream_t s) { return xna_bwd2_launch_ks<5, true>(p, Dv, s); }
