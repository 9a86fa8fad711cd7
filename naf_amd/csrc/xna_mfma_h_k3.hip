// Instantiations of the MFMA cell kernel for kernel_size = 3 with half values and output (NAF_F16).
#include "xna_mfma_kernel.h"

int naf_xna_mfma_launch_h_k3(const XnaMfmaParams& p, const XnaMfmaPlan& pl, int out_dtype, hipStream_t s) {
    return xna_mfma_launch_ks<3, true>(p, pl, out_dtype, s);
}
