// Head-summed MFMA cell kernel, 7x7 window (one translation unit per window: parallel compilation).
#include "xna_head_kernel.h"

int naf_xna_head_launch_k7(const XnaHeadParams& p, int out_dtype, hipStream_t s) {
    return xna_head_launch_ks<7>(p, out_dtype, s);
}

int naf_xna_head_ce_launch_k7(const XnaHeadParams& p, const XnaHeadCEExtra& x, hipStream_t s) {
    return xna_head_ce_launch_ks<7>(p, x, s);
}

int naf_xna_head_cm_launch_k7(const XnaHeadParams& p, const XnaHeadCMExtra& x, hipStream_t s) {
    return xna_head_cm_launch_ks<7>(p, x, s);
}
