// Cross-scale neighbourhood attention BACKWARD: mathematics, launch parameters and tile geometry of the MFMA cell kernel
// (xna_bwd2_kernel.h, gfx950 / CDNA4).
//
// Replaces what autograd runs through attentions.py:16-29 in the reference's training step (train.py:127-137,
// test/backward_speed.py:22-69): the backward of na2d_qk -> *scale -> softmax -> na2d_av plus the backward of the
// nearest-exact K/V upsampling (attentions.py:60-61), evaluated on the low-res grid like the forward
// (xna_mfma_kernel.h): every query of low-res cell (cy, cx) shares one clamped KS x KS window.
//
//   S = scale q.k^T   P = softmax_keys(S)   O = P v
//   dV[j] = sum_i P[i,j] dO[i]      dP[i,j] = dO[i].v[j]      delta[i] = sum_j P[i,j] dP[i,j]
//   dS[i,j] = scale P[i,j] (dP[i,j] - delta[i])      dQ[i] = sum_j dS[i,j] k[j]      dK[j] = sum_i dS[i,j] q[i]
//
// A cell's [KS*KS] x (64 + Dv) partial sums of dK / dV are added to the fp32 dK_lr / dV_lr accumulators with atomics (a low-res key
// sits in up to KS*KS windows).
#pragma once
#include <type_traits>

#include "naf_common.h"

struct XnaBwdParams {
    const bf16_t* q;
    const bf16_t* k;
    const bf16_t* v;
    const bf16_t* dout;
    bf16_t* dq;
    float* dk;   // [B, h, w, heads, 64] dense fp32 accumulator (pre-zeroed by the caller)
    float* dv;   // [B, h, w, heads, Dv]
    int32_t B, heads, Ho, Wo, h, w, dy, dx;
    uint32_t nblocks;
    int32_t seg_len, nseg;   // xna_bwd2_kernel.h: cells per run, runs per cell row (nblocks = runs there)
    float scale, scale_log2e;
    int64_t qs[4], ks[4], vs[4], gs[4], dqs[4];  // {b, head, y, x} element strides (gs: dout)
    // Channel chunks (xna_bwd.hip, windows whose K / V tiles + accumulators exceed the LDS / the register file at the full Dv): a launch
    // works on DV of the head's dv_pitch value channels (v, dout, dv point at its first one) -- the softmax does not depend on the
    // chunk and dQ, dK are sums over chunks, so every launch is a complete backward for its slice of V; launches after the first ADD
    // their dQ to what is there (dq_accum), dK accumulates through the atomics as it does across cells.
    int32_t dv_pitch, dq_accum;
#if defined(NAF_BWD_TIMING) || defined(NAF_BWD_TIMING2)
    unsigned long long* tim;   // tools/xna_bwd2_probe.hip: [workgroup][wave][8] s_memtime sums per phase
#endif
};

// 0.4.3 (naf_xna_bwd_scores): G, the gradient of the scaled scores L[i, j] = scale q_i . k_j that naf_xna_fwd returns as `logits`, enters as
// dS[i, j] += scale G[i, j] -- one fma onto the dS the kernel already makes, so a zero G gives the plain kernel's dS bit for bit.  The
// kernels that take it are separate instantiations (SG = true): the plain ones keep their code.  A chunked launch (xna_bwd.hip) runs the SG
// instantiation for its first channel chunk only, so G enters dQ / dK once.
struct XnaBwdScoresParams : XnaBwdParams {
    const float* dl;   // [B, heads, Ho, Wo, KS*KS] fp32, slot axis contiguous (slot = window row * KS + window column)
    int64_t dls[4];    // {b, head, y, x} element strides
};
template <bool SG>
using XnaBwdParamsT = std::conditional_t<SG, XnaBwdScoresParams, XnaBwdParams>;

template <int KS, int DV>
struct XnaBwdGeom {
    static constexpr int NSLOT = KS * KS;
    static constexpr int KPAD = ((NSLOT + 31) / 32) * 32;
    static constexpr int MT = KPAD / 16;      // 16-key tiles
    static constexpr int KST = KPAD / 32;     // 32-key steps (dQ contraction)
    static constexpr int KROW = 64 + 8;       // bf16 per K / Q row in LDS
    static constexpr int VROW = DV + 8;       // bf16 per V / dO row in LDS
    static constexpr int NVT = DV / 16;       // 16-channel tiles of dV
    static constexpr int NVW = (NVT + 3) / 4; // ... per wave
};
