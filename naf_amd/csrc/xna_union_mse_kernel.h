// Instantiations of the table-driven MFMA attention kernel with the regression objective in its epilogue (xna_union_kernel.h, P = XnaUnionMseParams):
// the kernel of naf_xna_mse_fwd.  Same tiles, staging and softmax as xna_union_kernel; what is stored is the gradient of the mean
// squared error in bf16, and every wave leaves one fp32 partial sum of squared differences.
#pragma once
#include "xna_union_kernel.h"

// Waves per workgroup of the objective instantiations: the plain kernel's (xna_union_waves), except for the 15 x 15 window with 16
// slots per window row.  The epilogue adds the lane's sum, four target values and their address to the live set; at 12 waves (168
// registers) that one instantiation spills 13 registers to scratch, so it runs 8 waves (256 registers); all others fit without scratch
// (resource-usage remarks).
constexpr int xna_union_mse_waves_rt(int ks, int wt) { return wt == 16 ? (ks >= 15 ? 8 : 12) : (ks >= 13 ? 4 : 8); }
template <int KS, int WT>
constexpr int xna_union_mse_waves() {
    return xna_union_mse_waves_rt(KS, WT);
}

template <int KS, int WT>
static int xna_union_mse_launch_one(const XnaUnionMseParams& p, size_t lds, hipStream_t s) {
    constexpr int NW = xna_union_mse_waves<KS, WT>();
    auto kern = xna_union_kernel<KS, bf16_t, WT, NW, XnaUnionMseParams>;
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (attr != hipSuccess) {
        naf_set_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize): %s", hipGetErrorString(attr));
        return NAF_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(kern, dim3(p.nblocks), dim3(NW * 64), lds, s, p);
    return naf_check_launch("xna_union_kernel (objective)");
}

template <int KS>
int xna_union_mse_launch_ks(const XnaUnionMseParams& p, int wt, size_t lds, hipStream_t s) {
    if (wt == 16) return xna_union_mse_launch_one<KS, 16>(p, lds, s);
    return xna_union_mse_launch_one<KS, 32>(p, lds, s);
}
