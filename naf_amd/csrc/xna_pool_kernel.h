// Mask pooling: cross-scale neighbourhood attention summed under K masks, MFMA cell kernel + gather (gfx950 / CDNA4).
//
// A[b, g, k, j] = sum_px M[b, k, px] * P_g[px, j]       mass[b, k] = sum_px M[b, k, px]        (include/naf_hip.h: naf_xna_maskpool_args)
// pooled[b, k, c] = sum_j A[b, g(c), k, j] * V[b, c, j] is then a small contraction on the low-res grid (xna_pool.hip: naf_maskpool_apply);
// the [B, C, Ho, Wo] tensor never exists and V is not read here at all.
//
// The geometry is xna_head_kernel.h's (read its header comment first): one workgroup (8 waves) = one (batch, low-res cell), it LOOPS OVER
// THE HEADS, stages the head's K window in LDS, forms S^T = K . Q on v_mfma_f32_16x16x32_bf16 and takes the fp32 softmax, normalised
// BEFORE P is rounded to bf16 -- the same instructions in the same order as the head kernel, so the bf16 P is bit for bit that
// kernel's and sum_px M . head(pv) = sum_j A . pv holds up to fp32 accumulation (the adjoint test).  What is new:
//   * the contraction runs over the PIXELS of the cell, which the S tiles leave on the lane axis (lane col = pixel): a wave writes its
//     tile's P, transposed, into a workgroup-wide LDS array Pt[slot][pixel of the round] (bf16, rows padded by 16 bytes), and after a
//     barrier the waves split the OUTPUT tiles (16 slots x 16 masks) among themselves: a wave contracts its tile over all pixels of the
//     round, 32 per v_mfma_f32_16x16x32_bf16 -- A operand: 8 consecutive pixels of one slot row of Pt (one ds_read_b128), B operand: 8
//     consecutive pixels of one mask row straight from memory (one 16-byte load for bf16 masks, 8 bytes for byte masks).  No two
//     waves add into the same accumulator, so there is no cross-wave reduction and the order of every sum is fixed.
//   * a round is 16 row tiles (16 x 16 pixels: the whole cell at ratio 16); larger cells take several rounds and the lane that owns
//     an element adds the later rounds to what it stored (same lane, program order).
//   * hazards: the idle lanes of a partial row tile (14- and 15-pixel cells) repeat the row's last pixel in the S tiles -- their P is
//     finite and their MASK operand is zero; tiles past the cell have zero P AND zero mask; key slots >= NSLOT have P = 0 exactly (masked
//     logits) and are never stored; masks K .. Kpad-1 are zero operands.
//   * mass comes from the same mask fragments (head 0, slot tile 0): per-lane fp32 sums, naf_rows_sum over the four lane groups.
//   * each cell writes its [heads][NSLOT][Kpad] fp32 partial; xna_pool_gather_kernel sums, for each key j, the partials of the cells
//     whose clamped window holds j in ascending (cy, cx) order (the clamp is the cell kernels': y0 = min(max(cy - KS/2, 0), h - KS)).
//     No float atomics: the result is bit-reproducible from launch to launch.
//   * cells whose width is not a multiple of 8 pixels load the mask element by element (alignment); the arithmetic is the same.
#pragma once
#include "xna_mfma_kernel.h"

struct XnaPoolParams {
    const bf16_t* q;
    const bf16_t* k;
    const void* masks;   // [B, K, Ho, Wo] bf16 or bytes, x contiguous
    float* part;         // [B][h*w][heads][NSLOT][kpad]
    float* pmass;        // [B][h*w][kpad]
    const float* tab_y;  // rotate-on-load: RoPE tables [Ho][2][16] / [Wo][2][16], or nullptr
    const float* tab_x;
    int32_t B, heads, Ho, Wo, h, w, dy, dx;
    int32_t K, kpad;
    uint32_t nblocks;
    float scale_log2e;
    int64_t qs[4], ks[4], vs[4];  // {b, head, y, x} element strides (vs: unused, xna_fill_common's)
    int64_t ms[4];                // {b, k, y, x}
};

constexpr int XNA_POOL_NW = 8;          // waves per workgroup
constexpr int XNA_POOL_RPX = 256;       // pixels of a round: 16 row tiles
constexpr int XNA_POOL_PROW = XNA_POOL_RPX + 8;   // bf16 elements per Pt row (528 B: 16 lanes x 16 bytes land in 64 distinct banks)
constexpr int xna_pool_prows(int ks) { return (ks * ks + 15) / 16 * 16; }
constexpr size_t xna_pool_lds_for(int ks) { return (size_t)(ks * ks) * 72 * 2 + (size_t)xna_pool_prows(ks) * XNA_POOL_PROW * 2; }

template <int KS, bool U8>
__global__ __launch_bounds__(XNA_POOL_NW * 64) void xna_pool_kernel(const XnaPoolParams p) {
    constexpr int NW = XNA_POOL_NW, NT = NW * 64, TPW = 2;
    using G = XnaGeom<KS, 1>;
    constexpr int NSLOT = G::NSLOT, MT = G::MT, KROW = G::KROW;
    constexpr int PROWS = xna_pool_prows(KS), MTR = PROWS / 16, PROW = XNA_POOL_PROW;
    using MaskT = typename std::conditional<U8, uint8_t, bf16_t>::type;

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    bf16_t* Ks = reinterpret_cast<bf16_t*>(smem);
    bf16_t* Pt = Ks + NSLOT * KROW;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = lane & 15;
    const int grp = lane >> 4;

    uint32_t L = xna_block_order(blockIdx.x, p.nblocks, 16, 1u);
    const int cx = L % p.w;
    L /= p.w;
    const int cy = L % p.h;
    const int b = L / p.h;
    const int y0 = min(max(cy - KS / 2, 0), p.h - KS);   // the cell's clamped window
    const int x0 = min(max(cx - KS / 2, 0), p.w - KS);

    const int tpr = (p.dx + 15) >> 4;      // row tiles per cell row (host: xna_row_tiles_ok(dx))
    const int ntile = p.dy * tpr;          // <= 1024 (host)
    const uint32_t tmagic = (1u << 20) / (uint32_t)tpr + 1u;   // t / tpr for t, tpr <= 1024
    const bool rope = p.tab_y != nullptr;
    const bool vec = (p.dx & 7) == 0;      // mask fragments as one aligned vector load (host: pointer and strides)
    const bf16_t* q_cell = p.q + b * p.qs[0] + (int64_t)(cy * p.dy) * p.qs[2] + (int64_t)(cx * p.dx) * p.qs[3];
    const bf16_t* kb = p.k + b * p.ks[0];
    const MaskT* m_cell = reinterpret_cast<const MaskT*>(p.masks) + b * p.ms[0] + (int64_t)(cy * p.dy) * p.ms[2] + (int64_t)(cx * p.dx);
    const size_t cell = (size_t)b * (size_t)(p.h * p.w) + (size_t)(cy * p.w + cx);
    float* part_cell = p.part + cell * (size_t)p.heads * (size_t)(NSLOT * p.kpad);
    float* pmass_cell = p.pmass + cell * (size_t)p.kpad;
    const int KT = p.kpad >> 4;

    auto ka_of = [&](int mt) __attribute__((always_inline)) {
        const int row = (mt * 16 + 15 < NSLOT) ? mt * 16 + col : min(mt * 16 + col, NSLOT - 1);
        return Ks + row * KROW + grp * 8;
    };

    for (int t0 = 0; t0 < ntile; t0 += NW * TPW) {
        int tyv[TPW];
        bool livev[TPW];
        const bf16_t* qpv[TPW];
        f32x4_t cs[TPW][4] = {};
#pragma unroll
        for (int u = 0; u < TPW; ++u) {
            const int tt = t0 + u * NW + wave;
            livev[u] = tt < ntile;
            const int ttc = min(tt, ntile - 1);
            tyv[u] = (int)(((uint32_t)ttc * tmagic) >> 20);
            const int tx0 = (ttc - tyv[u] * tpr) * 16;
            const int xl = min(tx0 + col, p.dx - 1);   // lanes past a partial last tile re-read its last pixel
            qpv[u] = q_cell + (int64_t)tyv[u] * p.qs[2] + (int64_t)xl * p.qs[3] + grp * 8;
            if (rope) {
                const float* tr = ((grp >> 1) ? p.tab_x + (int64_t)(cx * p.dx + xl) * 32 : p.tab_y + (int64_t)(cy * p.dy + tyv[u]) * 32) + (grp & 1) * 8;
                cs[u][0] = *reinterpret_cast<const f32x4_t*>(tr);
                cs[u][1] = *reinterpret_cast<const f32x4_t*>(tr + 4);
                cs[u][2] = *reinterpret_cast<const f32x4_t*>(tr + 16);
                cs[u][3] = *reinterpret_cast<const f32x4_t*>(tr + 20);
            }
        }
        const int nlive = min(NW * TPW, ntile - t0);   // tiles of the round inside the cell
        const int nch = (nlive + 1) >> 1;              // 32-pixel chunks that hold one

        for (int head = 0; head < p.heads; ++head) {
            bf16x8_t qf[TPW][2];
#pragma unroll
            for (int u = 0; u < TPW; ++u) {
                const bf16_t* qp = qpv[u] + head * p.qs[1];
                qf[u][0] = *reinterpret_cast<const bf16x8_t*>(qp);
                qf[u][1] = *reinterpret_cast<const bf16x8_t*>(qp + 32);
            }
            __syncthreads();   // every wave is done with the previous head's K window and Pt
            {
                // ---- stage the K window (L2 -> registers -> LDS): all loads of a batch before its first LDS write
                const bf16_t* kh = kb + head * p.ks[1];
                constexpr int KTOT = NSLOT * 8;
                constexpr int KIT = (KTOT + NT - 1) / NT;
                u32x4_t val[KIT];
#pragma unroll
                for (int j = 0; j < KIT; ++j) {
                    const int i = min(j * NT + tid, KTOT - 1);
                    const int key = i >> 3, c = i & 7;
                    const int ry = key / KS, rx = key - ry * KS;
                    val[j] = *reinterpret_cast<const u32x4_t*>(kh + (int64_t)(y0 + ry) * p.ks[2] + (int64_t)(x0 + rx) * p.ks[3] + c * 8);
                }
#pragma unroll
                for (int j = 0; j < KIT; ++j) {
                    const int i = j * NT + tid;
                    if ((KTOT % NT == 0) || i < KTOT) *reinterpret_cast<u32x4_t*>(Ks + (i >> 3) * KROW + (i & 7) * 8) = val[j];
                }
            }
            __syncthreads();

#pragma unroll
            for (int u = 0; u < TPW; ++u) {
                bf16_t* pcol = Pt + (u * NW + wave) * 16 + col;   // this lane's pixel column of the round
                if (!livev[u]) {   // wave-uniform: a tile past the cell contributes zeros
#pragma unroll
                    for (int mt = 0; mt < MTR; ++mt)
#pragma unroll
                        for (int r = 0; r < 4; ++r) pcol[(mt * 16 + grp * 4 + r) * PROW] = (bf16_t)0.f;
                    continue;
                }
                if (rope) {
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        float o1, o2;
                        naf_rope_rotate((float)qf[u][0][i], (float)qf[u][1][i], cs[u][i >> 2][i & 3], cs[u][2 + (i >> 2)][i & 3], o1, o2);
                        qf[u][0][i] = (bf16_t)o1;
                        qf[u][1][i] = (bf16_t)o2;
                    }
                }
                // ---- S^T = K . Q^T: lane (col, grp) gets key slots mt*16 + grp*4 + r of query col ----
                f32x4_t s[MT];
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    s[mt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks) {
                        const bf16x8_t ka = *reinterpret_cast<const bf16x8_t*>(ka_of(mt) + ks * 32);
                        s[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ka, qf[u][ks], s[mt], 0, 0, 0);
                    }
                }
                // ---- softmax over the key slots, fp32; P is normalised before it is rounded to bf16 (the head kernel's code) ----
                float m = -INFINITY;
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        if (mt * 16 + 15 >= NSLOT) {   // tile contains pad slots: mask them
                            const bool valid = (mt * 16 + r + grp * 4) < NSLOT;
                            s[mt][r] = valid ? s[mt][r] : -INFINITY;
                        }
                        m = fmaxf(m, s[mt][r]);
                    }
                m = naf_rows_max(m);
                float sum = 0.f;
                const float mc = m * p.scale_log2e;
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float e = __builtin_amdgcn_exp2f(fmaf(s[mt][r], p.scale_log2e, -mc));
                        s[mt][r] = e;
                        sum += e;
                    }
                sum = naf_rows_sum(sum);
                const float inv = __builtin_amdgcn_rcpf(sum);   // sum >= 1
                // ---- P^T to LDS: slot rows, this lane's pixel column (slots >= NSLOT inside PROWS are exact zeros) ----
#pragma unroll
                for (int mt = 0; mt < MTR; ++mt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) pcol[(mt * 16 + grp * 4 + r) * PROW] = (bf16_t)(s[mt][r] * inv);
            }
            __syncthreads();

            // ---- A_cell[slot, k] = sum_px P[px, slot] * M[k, px]: output tile ot = kt * MTR + mt on wave ot % NW ----
            for (int ot = wave; ot < MTR * KT; ot += NW) {
                const int kt = ot / MTR, mt = ot - kt * MTR;
                const int km = kt * 16 + col;   // this lane's mask
                const MaskT* mk = m_cell + (int64_t)min(km, p.K - 1) * p.ms[1];
                f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
                float msum = 0.f;
                for (int c = 0; c < nch; ++c) {
                    const int tt = t0 + c * 2 + (grp >> 1);
                    const int ty = (int)(((uint32_t)min(tt, ntile - 1) * tmagic) >> 20);
                    const int tx = (min(tt, ntile - 1) - ty * tpr) * 16 + (grp & 1) * 8;   // first of this lane's 8 pixels in the cell row
                    const bool on = km < p.K && tt < ntile;
                    const MaskT* mp = mk + (int64_t)ty * p.ms[2] + tx;
                    bf16x8_t mf;
                    if (vec) {
                        const bool ld = on && tx < p.dx;   // dx % 8 == 0: all eight pixels or none
                        if constexpr (U8) {
                            uint64_t raw = 0;
                            if (ld) raw = *reinterpret_cast<const uint64_t*>(mp);
#pragma unroll
                            for (int j = 0; j < 8; ++j) mf[j] = (bf16_t)(float)((raw >> (8 * j)) & 0xffu);
                        } else {
                            u32x4_t raw = {0u, 0u, 0u, 0u};
                            if (ld) raw = *reinterpret_cast<const u32x4_t*>(mp);
                            mf = __builtin_bit_cast(bf16x8_t, raw);
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            float v = 0.f;
                            if (on && tx + j < p.dx) v = (float)mp[j];
                            mf[j] = (bf16_t)v;
                        }
                    }
                    const bf16x8_t pa = *reinterpret_cast<const bf16x8_t*>(Pt + (mt * 16 + col) * PROW + c * 32 + grp * 8);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa, mf, acc, 0, 0, 0);
                    if (head == 0 && mt == 0) {
#pragma unroll
                        for (int j = 0; j < 8; ++j) msum += (float)mf[j];
                    }
                }
                // lane (col, grp) holds slots mt*16 + grp*4 + r of mask kt*16 + col
                float* po = part_cell + (size_t)head * (size_t)(NSLOT * p.kpad) + km;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int slot = mt * 16 + grp * 4 + r;
                    if (slot < NSLOT) {
                        float* d = po + (size_t)slot * (size_t)p.kpad;
                        *d = t0 == 0 ? acc[r] : *d + acc[r];
                    }
                }
                if (head == 0 && mt == 0) {   // wave-uniform
                    msum = naf_rows_sum(msum);
                    if (grp == 0) pmass_cell[km] = t0 == 0 ? msum : pmass_cell[km] + msum;
                }
            }
        }
    }
}

// A[b, head, k, j] = sum over the cells whose clamped window holds key j of part[b][cell][head][slot of j][k], ascending (cy, cx).
template <int KS>
__global__ __launch_bounds__(256) void xna_pool_gather_kernel(const float* __restrict__ part, float* __restrict__ A, int B, int heads, int h, int w,
                                                              int K, int kpad) {
    constexpr int NSLOT = KS * KS;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t hw = (size_t)h * w;
    const size_t total = (size_t)B * heads * hw * kpad;
    if (idx >= total) return;
    const int k = (int)(idx % kpad);
    size_t r = idx / kpad;
    const int j = (int)(r % hw);
    r /= hw;
    const int head = (int)(r % heads);
    const int b = (int)(r / heads);
    if (k >= K) return;
    const int jy = j / w, jx = j - jy * w;
    float sum = 0.f;
    for (int cy = max(jy - KS + 1, 0); cy <= min(jy + KS - 1, h - 1); ++cy) {
        const int y0 = min(max(cy - KS / 2, 0), h - KS);
        if (jy < y0 || jy >= y0 + KS) continue;
        for (int cx = max(jx - KS + 1, 0); cx <= min(jx + KS - 1, w - 1); ++cx) {
            const int x0 = min(max(cx - KS / 2, 0), w - KS);
            if (jx < x0 || jx >= x0 + KS) continue;
            const int slot = (jy - y0) * KS + (jx - x0);
            sum += part[(((size_t)b * hw + (size_t)(cy * w + cx)) * heads + head) * (size_t)(NSLOT * kpad) + (size_t)slot * kpad + k];
        }
    }
    A[(((size_t)b * heads + head) * K + k) * hw + j] = sum;
}

// The window's entry point, one explicit instantiation per window in xna_pool_inst.hip: the cell kernel (bf16 or byte masks), then the gather.
template <int KS>
int xna_pool_launch_ks(const XnaPoolParams& p, bool u8, float* A, hipStream_t s) {
    constexpr size_t lds = xna_pool_lds_for(KS);
    static_assert(lds <= 160 * 1024, "LDS budget");
    auto kern = u8 ? xna_pool_kernel<KS, true> : xna_pool_kernel<KS, false>;
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) {
            naf_set_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize=%zu): %s", lds, hipGetErrorString(e));
            return NAF_ERR_LAUNCH;
        }
    }
    hipLaunchKernelGGL(kern, dim3(p.nblocks), dim3(XNA_POOL_NW * 64), lds, s, p);
    int rc = naf_check_launch("xna_pool_kernel");
    if (rc != NAF_OK) return rc;
    const size_t total = (size_t)p.B * p.heads * p.h * p.w * p.kpad;
    hipLaunchKernelGGL(xna_pool_gather_kernel<KS>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, p.part, A, p.B, p.heads, p.h, p.w, p.K, p.kpad);
    return naf_check_launch("xna_pool_gather_kernel");
}

// xna_pool_inst.hip (-DNAF_KS=<KS>) defines it, xna_pool.hip declares it (extern) and dispatches on the window.
#define NAF_XNA_POOL_WINDOW(LINKAGE, KS) LINKAGE template int xna_pool_launch_ks<KS>(const XnaPoolParams&, bool, float*, hipStream_t);
