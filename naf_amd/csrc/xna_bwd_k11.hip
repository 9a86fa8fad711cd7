// Instantiations of the attention backward cell kernel for kernel_size = 11 (whole heads up to Dv = 128, two channel chunks above: xna_bwd.hip).
#include "xna_bwd2_kernel.h"

int naf_xna_bwd_launch_k11(const XnaBwdParams& p, int Dv, hipStream_t s) { return xna_bwd2_launch_ks<11>(p, Dv, s); }
int naf_xna_bwd_scores_launch_k11(const XnaBwdScoresParams& p, int Dv, hipStream_t s) { return xna_bwd2_launch_ks<11, true>(p, Dv, s); }
