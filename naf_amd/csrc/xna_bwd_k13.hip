// Instantiations of the attention backward cell kernel for kernel_size = 13 (channel chunks of at most 64: xna_bwd.hip).
#include "xna_bwd2_kernel.h"

int naf_xna_bwd_launch_k13(const XnaBwdParams& p, int Dv, hipStream_t s) { return xna_bwd2_launch_ks<13>(p, Dv, s); }
int naf_xna_bwd_scores_launch_k13(const XnaBwdScoresParams& p, int Dv, hipStream_t s) { return xna_bwd2_launch_ks<13, true>(p, Dv, s); }
