// Instantiations of the attention backward cell kernel for kernel_size = 15 (channel chunks of 32 or 64: xna_bwd.hip).
#include "xna_bwd2_kernel.h"

int naf_xna_bwd_launch_k15(const XnaBwdParams& p, int Dv, hipStream_t s) { return xna_bwd2_launch_ks<15>(p, Dv, s); }
int naf_xna_bwd_scores_launch_k15(const XnaBwdScoresParams& p, int Dv, hipStream_t s) { return xna_bwd2_launch_ks<15, true>(p, Dv, s); }
