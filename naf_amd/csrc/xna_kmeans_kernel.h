// K-means step on the upsampled features: assign and accumulate in one MFMA cell kernel (gfx950 / CDNA4).
//
// label(px) = argmax_k (bias[b, k] + sum_g sum_slot P_g[px, slot] * PV_g[cell(slot), k])                 (include/naf_hip.h: naf_xna_kmeans_args)
// A[b, g, k, j] = sum_px [label(px) = k] * P_g[px, j]       mass[b, k] = #{px: label(px) = k}
//
// Both halves exist: the assignment is xna_head_kernel.h's classification epilogue (a linear head with a bias and an argmax), the
// accumulation is xna_pool_kernel.h under one-hot masks.  The two kernels share their geometry -- one workgroup (8 waves) = one (batch,
// low-res cell), the same row tiles (tile t0 + u * 8 + wave of a round of 16), the same S^T = K . Q and softmax instructions -- so this
// kernel runs, per round of 256 pixels, first the one and then the other (read both headers first):
//   * phase A: the head kernel's head loop (stage the K and PV windows, S^T, fp32 softmax normalised before the bf16 rounding,
//     O^T += PV^T . P^T summed over the heads), + bias in fp32, and the classification epilogue's argmax: the lowest index among equal
//     maxima, channels >= K masked.  The pixel's grp == 0 lane writes the label as ONE BYTE to lab[tile of the round * 16 + col] in LDS
//     -- the column index Pt uses -- and, where a label map is asked for, to memory as that epilogue does.  0xFF is written for a tile
//     past the cell, for the idle lanes of a partial row tile (14- and 15-pixel cells repeat the row's last pixel) and for a label
//     outside [0, K): K <= 64, so 0xFF matches no cluster and such a pixel is counted nowhere.  (A pixel whose logits are all NaN
//     fails every comparison: its argmax is 0, here as in the head kernel, and it is counted in cluster 0 -- once.)
//   * phase B: the pool kernel's head loop (stage the K window, recompute S^T and the softmax from the same queries -- the cell's
//     queries were read a moment ago: L2 hits --, write Pt, barrier, split the output tiles among the waves).  The B operand of
//     v_mfma_f32_16x16x32_bf16 is built from the labels: one ds_read_b64 of eight labels, mf[j] = (lab[c*32 + grp*8 + j] == km) ? 1 : 0.
//     No mask is read from memory.  Chunk order, accumulator ownership, the per-cell partial layout [heads][NSLOT][Kpad], pmass, the
//     later-round adds and xna_pool_gather_kernel are the pool kernel's, so A and mass are bit for bit what that kernel returns for
//     the byte masks [label == k]; mass is an exact integer count.
//   * LDS: K window | PV window (phase A) aliased with Pt (phase B) | lab (256 bytes).  The barrier that opens every head iteration of
//     either phase separates the last reads of the one from the first writes of the other; lab is written after phase A's last
//     window reads and read only behind phase B's barriers, and rewritten two barriers after its last read.
//   * rotate-on-load: the round's RoPE table rows are fetched once and held through both phases (window 15: fetched at every rotation),
//     so both phases rotate identically.
//   * NCT in {2, 4}: K <= 64.  Two tiles per wave in both phases (xna_head_tpw(KS, NCT <= 4) == 2 == the pool kernel's).
// No float atomics: every output is bit-reproducible from launch to launch.
#pragma once
#include "xna_head_kernel.h"
#include "xna_pool_kernel.h"

struct XnaKmeansParams {
    const bf16_t* q;
    const bf16_t* k;
    const bf16_t* pv;
    const float* bias;   // [B][K] rows bias_stride_b apart, or nullptr
    uint8_t* labels;     // [B, Ho, Wo] or nullptr
    float* part;         // [B][h*w][heads][NSLOT][kpad]
    float* pmass;        // [B][h*w][kpad]
    const float* tab_y;  // rotate-on-load: RoPE tables [Ho][2][16] / [Wo][2][16], or nullptr
    const float* tab_x;
    int32_t B, heads, Ho, Wo, h, w, dy, dx;
    int32_t K, kpad;     // kpad: channels a pv row holds = masks of a partial row (K rounded up to 16)
    uint32_t nblocks;
    float scale_log2e;
    int64_t bias_stride_b;
    int64_t qs[4], ks[4], vs[4];  // {b, head, y, x} element strides (vs: pv)
    int64_t ls[3];                // {b, y, x} of labels
};

constexpr size_t xna_kmeans_lds_for(int ks, int nct) {
    const size_t vwin = (size_t)(ks * ks) * (nct * 16 + 16) * 2, pt = (size_t)xna_pool_prows(ks) * XNA_POOL_PROW * 2;
    return (size_t)(ks * ks) * 72 * 2 + (vwin > pt ? vwin : pt) + XNA_POOL_RPX;
}

template <int KS, int NCT>
__global__ __launch_bounds__(XNA_POOL_NW * 64) void xna_kmeans_kernel(const XnaKmeansParams p) {
    constexpr int NW = XNA_POOL_NW, NT = NW * 64, TPW = 2;
    static_assert(NCT == 2 || NCT == 4, "K <= 64");
    static_assert(XNA_HEAD_NW == NW && xna_head_tpw(KS, NCT) == TPW, "both phases walk the same row tiles");
    using G = XnaGeom<KS, 1>;
    constexpr int NSLOT = G::NSLOT, MT = G::MT, KST = G::KST, KROW = G::KROW;
    constexpr int DVT = NCT * 16, VROW = XnaVRow<DVT>::VROW, VCH = DVT / 8;
    constexpr int PROWS = xna_pool_prows(KS), MTR = PROWS / 16, PROW = XNA_POOL_PROW;
    constexpr size_t LAB_OFF = xna_kmeans_lds_for(KS, NCT) - XNA_POOL_RPX;
    static_assert(LAB_OFF % 16 == 0, "lab is read in 8-byte words");
    // window 15 has no registers to hold the round's RoPE table rows through the head loops (it spills): it fetches them again at every
    // rotation (L1 / L2 hits); the values, and so the rotation, are the same
    constexpr bool CSR = KS >= 15;

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    bf16_t* Ks = reinterpret_cast<bf16_t*>(smem);
    bf16_t* Vs = Ks + NSLOT * KROW;   // phase A
    bf16_t* Pt = Ks + NSLOT * KROW;   // phase B
    uint8_t* lab = smem + LAB_OFF;

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
    const bf16_t* q_cell = p.q + b * p.qs[0] + (int64_t)(cy * p.dy) * p.qs[2] + (int64_t)(cx * p.dx) * p.qs[3];
    const bf16_t* kb = p.k + b * p.ks[0];
    const bf16_t* vb = p.pv + b * p.vs[0];
    const size_t cell = (size_t)b * (size_t)(p.h * p.w) + (size_t)(cy * p.w + cx);
    float* part_cell = p.part + cell * (size_t)p.heads * (size_t)(NSLOT * p.kpad);
    float* pmass_cell = p.pmass + cell * (size_t)p.kpad;
    const int KT = p.kpad >> 4;

    // key slots >= NSLOT are not stored: their reads are clamped to the last real row, their logits masked, P = 0
    auto ka_of = [&](int mt) __attribute__((always_inline)) {
        const int row = (mt * 16 + 15 < NSLOT) ? mt * 16 + col : min(mt * 16 + col, NSLOT - 1);
        return Ks + row * KROW + grp * 8;
    };
    auto va_of = [&](int blk) __attribute__((always_inline)) {
        const int r = blk * 16 + grp * 4 + (col >> 2);
        const int row = (blk * 16 + 15 < NSLOT) ? r : min(r, NSLOT - 1);
        return Vs + row * VROW + (col & 3) * 4;
    };

    // the RoPE table rows of a tile: head dims [grp*8, +8) and their partners +32; dims < 16 turn with the row angle, dims >= 16 with the column angle
    auto load_cs = [&](int ty, int xl, f32x4_t (&c4)[4]) __attribute__((always_inline)) {
        const float* tr = ((grp >> 1) ? p.tab_x + (int64_t)(cx * p.dx + xl) * 32 : p.tab_y + (int64_t)(cy * p.dy + ty) * 32) + (grp & 1) * 8;
        c4[0] = *reinterpret_cast<const f32x4_t*>(tr);
        c4[1] = *reinterpret_cast<const f32x4_t*>(tr + 4);
        c4[2] = *reinterpret_cast<const f32x4_t*>(tr + 16);
        c4[3] = *reinterpret_cast<const f32x4_t*>(tr + 20);
    };

    for (int t0 = 0; t0 < ntile; t0 += NW * TPW) {
        // this wave's tiles of the round: t0 + u * NW + wave (wave-uniform), the same in both phases
        int tyv[TPW], tx0v[TPW];
        bool livev[TPW];
        const bf16_t* qpv[TPW];
        f32x4_t cs[TPW][4] = {};
#pragma unroll
        for (int u = 0; u < TPW; ++u) {
            const int tt = t0 + u * NW + wave;
            livev[u] = tt < ntile;
            const int ttc = min(tt, ntile - 1);
            tyv[u] = (int)(((uint32_t)ttc * tmagic) >> 20);
            tx0v[u] = (ttc - tyv[u] * tpr) * 16;
            const int xl = min(tx0v[u] + col, p.dx - 1);   // lanes past a partial last tile re-read its last pixel
            qpv[u] = q_cell + (int64_t)tyv[u] * p.qs[2] + (int64_t)xl * p.qs[3] + grp * 8;
            if (rope && !CSR) load_cs(tyv[u], xl, cs[u]);
        }
        const int nlive = min(NW * TPW, ntile - t0);   // tiles of the round inside the cell
        const int nch = (nlive + 1) >> 1;              // 32-pixel chunks that hold one

        // ================= phase A: labels (xna_head_kernel.h's head loop and the argmax of its classification epilogue) =================
        {
            f32x4_t acc[TPW][NCT];
#pragma unroll
            for (int u = 0; u < TPW; ++u)
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) acc[u][ct] = f32x4_t{0.f, 0.f, 0.f, 0.f};

            for (int head = 0; head < p.heads; ++head) {
                bf16x8_t qf[TPW][2];
#pragma unroll
                for (int u = 0; u < TPW; ++u) {
                    const bf16_t* qp = qpv[u] + head * p.qs[1];
                    qf[u][0] = *reinterpret_cast<const bf16x8_t*>(qp);
                    qf[u][1] = *reinterpret_cast<const bf16x8_t*>(qp + 32);
                }
                __syncthreads();   // every wave is done with the previous head's windows (and with the previous round's Pt)
                {
                    // ---- stage the K and PV windows (L2 -> registers -> LDS): all loads of a batch before its first LDS write
                    const bf16_t* kh = kb + head * p.ks[1];
                    const bf16_t* vh = vb + head * p.vs[1];
                    constexpr int KTOT = NSLOT * 8, VTOT = NSLOT * VCH;
                    constexpr int KIT = (KTOT + NT - 1) / NT, VIT = (VTOT + NT - 1) / NT;
                    constexpr int BATCH = 8;
                    const int vch_mem = p.kpad >> 3;   // 16-byte chunks a pv row holds in memory; the rest of the LDS row is zero
#pragma unroll
                    for (int j0 = 0; j0 < KIT + VIT; j0 += BATCH) {
                        u32x4_t val[BATCH];
#pragma unroll
                        for (int e = 0; e < BATCH; ++e) {
                            const int j = j0 + e;
                            if (j < KIT) {
                                const int i = min(j * NT + tid, KTOT - 1);
                                const int key = i >> 3, c = i & 7;
                                const int ry = key / KS, rx = key - ry * KS;
                                val[e] = *reinterpret_cast<const u32x4_t*>(kh + (int64_t)(y0 + ry) * p.ks[2] + (int64_t)(x0 + rx) * p.ks[3] + c * 8);
                            } else if (j < KIT + VIT) {
                                const int i = min((j - KIT) * NT + tid, VTOT - 1);
                                const int key = i / VCH, c = i - key * VCH;
                                const int ry = key / KS, rx = key - ry * KS;
                                const u32x4_t ld = *reinterpret_cast<const u32x4_t*>(vh + (int64_t)(y0 + ry) * p.vs[2] + (int64_t)(x0 + rx) * p.vs[3] + min(c, vch_mem - 1) * 8);
                                val[e] = c < vch_mem ? ld : u32x4_t{0u, 0u, 0u, 0u};
                            }
                        }
#pragma unroll
                        for (int e = 0; e < BATCH; ++e) {
                            const int j = j0 + e;
                            if (j < KIT) {
                                const int i = j * NT + tid;
                                if ((KTOT % NT == 0) || i < KTOT) *reinterpret_cast<u32x4_t*>(Ks + (i >> 3) * KROW + (i & 7) * 8) = val[e];
                            } else if (j < KIT + VIT) {
                                const int i = (j - KIT) * NT + tid;
                                const int key = i / VCH, c = i - key * VCH;
                                if ((VTOT % NT == 0) || i < VTOT) *reinterpret_cast<u32x4_t*>(Vs + key * VROW + c * 8) = val[e];
                            }
                        }
                    }
                }
                __syncthreads();

#pragma unroll
                for (int u = 0; u < TPW; ++u) {
                    if (!livev[u]) continue;   // wave-uniform
                    if (rope) {
                        if constexpr (CSR) load_cs(tyv[u], min(tx0v[u] + col, p.dx - 1), cs[u]);
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
                    // ---- softmax over the key slots, fp32; P is normalised before it is rounded to bf16 ----
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
                    // pack P to bf16 B-fragments: k index (g, j) <-> slot ks*32 + (j>>2)*16 + g*4 + (j&3)
                    bf16x8_t pf[KST];
#pragma unroll
                    for (int ks = 0; ks < KST; ++ks)
#pragma unroll
                        for (int j = 0; j < 8; ++j) pf[ks][j] = (bf16_t)(s[2 * ks + (j >> 2)][j & 3] * inv);
                    // ---- O^T += PV^T . P^T: lane (col, grp) owns channels ct*16 + grp*4 + r of query col ----
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct) {
#pragma unroll
                        for (int ks = 0; ks < KST; ++ks) {
                            const bf16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((NAF_LDS bf16x4_t*)(va_of(ks * 2) + ct * 16));
                            const bf16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((NAF_LDS bf16x4_t*)(va_of(ks * 2 + 1) + ct * 16));
                            bf16x8_t a;
                            a[0] = lo[0]; a[1] = lo[1]; a[2] = lo[2]; a[3] = lo[3];
                            a[4] = hi[0]; a[5] = hi[1]; a[6] = hi[2]; a[7] = hi[3];
                            acc[u][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, pf[ks], acc[u][ct], 0, 0, 0);
                        }
                    }
                }
            }

            // ---- z = acc + bias (fp32), label = lowest k with z[k] = max z: the classification epilogue's expressions ----
            // (the lane's coordinates are made opaque, as in that epilogue: what derives from them is invariant in the head loop and would
            // be hoisted above it and held in registers through it)
            int ecol = col, egrp = grp;
            asm volatile("" : "+v"(ecol), "+v"(egrp));
            const float* bias_b = p.bias != nullptr ? p.bias + b * p.bias_stride_b : nullptr;
#pragma unroll
            for (int u = 0; u < TPW; ++u) {
                uint8_t* lcol = lab + (u * NW + wave) * 16 + ecol;   // this lane's pixel column of the round
                if (!livev[u]) {   // wave-uniform: a tile past the cell counts nowhere
                    if (egrp == 0) *lcol = (uint8_t)0xFF;
                    continue;
                }
                const bool inpx = tx0v[u] + ecol < p.dx;
                float m = -INFINITY;
                int am = 0;
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int ch = ct * 16 + egrp * 4 + r;
                        if (ch < p.K) {
                            const float z = acc[u][ct][r] + (bias_b != nullptr ? bias_b[ch] : 0.f);
                            if (z > m) {   // a lane's channels ascend with (ct, r): the first of equal maxima stays
                                m = z;
                                am = ch;
                            }
                        }
                    }
                const float mall = naf_rows_max(m);
                // lowest index among the lanes that hold the maximum: indices <= 255 are exact in fp32
                const int label = (int)(-naf_rows_max(m == mall ? -(float)am : -INFINITY));
                if (egrp == 0) {
                    // the idle lanes of a partial tile repeat its last pixel: counted nowhere, stored nowhere
                    *lcol = (inpx && (unsigned)label < (unsigned)p.K) ? (uint8_t)label : (uint8_t)0xFF;
                    if (p.labels != nullptr && inpx) {
                        const int64_t gy = cy * p.dy + tyv[u];
                        const int64_t gx = cx * p.dx + tx0v[u] + ecol;
                        p.labels[b * p.ls[0] + gy * p.ls[1] + gx * p.ls[2]] = (uint8_t)label;
                    }
                }
            }
        }

        // ================= phase B: accumulate (xna_pool_kernel.h's head loop, the mask operand built from lab) =================
        for (int head = 0; head < p.heads; ++head) {
            bf16x8_t qf[TPW][2];
#pragma unroll
            for (int u = 0; u < TPW; ++u) {
                const bf16_t* qp = qpv[u] + head * p.qs[1];
                qf[u][0] = *reinterpret_cast<const bf16x8_t*>(qp);
                qf[u][1] = *reinterpret_cast<const bf16x8_t*>(qp + 32);
            }
            __syncthreads();   // every wave is done with the previous head's K window and Pt; head 0: with phase A's windows, and lab is written
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
                    if constexpr (CSR) load_cs(tyv[u], min(tx0v[u] + col, p.dx - 1), cs[u]);
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
                // ---- softmax over the key slots, fp32; P is normalised before it is rounded to bf16 (phase A's code) ----
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

            // ---- A_cell[slot, k] = sum_px P[px, slot] * [lab[px] == k]: output tile ot = kt * MTR + mt on wave ot % NW ----
            int ocol = col, ogrp = grp;   // opaque: the loop's addresses are not formed above the tiles and held through them
            asm volatile("" : "+v"(ocol), "+v"(ogrp));
            for (int ot = wave; ot < MTR * KT; ot += NW) {
                const int kt = ot / MTR, mt = ot - kt * MTR;
                const int km = kt * 16 + ocol;   // this lane's cluster (km >= K: no label equals it)
                f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
                float msum = 0.f;
                for (int c = 0; c < nch; ++c) {
                    const uint64_t raw = *reinterpret_cast<const uint64_t*>(lab + c * 32 + ogrp * 8);   // the labels of this lane's 8 pixels
                    bf16x8_t mf;
#pragma unroll
                    for (int j = 0; j < 8; ++j) mf[j] = (bf16_t)((int)((raw >> (8 * j)) & 0xffu) == km ? 1.f : 0.f);
                    const bf16x8_t pa = *reinterpret_cast<const bf16x8_t*>(Pt + (mt * 16 + ocol) * PROW + c * 32 + ogrp * 8);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa, mf, acc, 0, 0, 0);
                    if (head == 0 && mt == 0) {
#pragma unroll
                        for (int j = 0; j < 8; ++j) msum += (float)mf[j];
                    }
                }
                // lane (col, grp) holds slots mt*16 + grp*4 + r of cluster kt*16 + col
                float* po = part_cell + (size_t)head * (size_t)(NSLOT * p.kpad) + km;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int slot = mt * 16 + ogrp * 4 + r;
                    if (slot < NSLOT) {
                        float* d = po + (size_t)slot * (size_t)p.kpad;
                        *d = t0 == 0 ? acc[r] : *d + acc[r];
                    }
                }
                if (head == 0 && mt == 0) {   // wave-uniform
                    msum = naf_rows_sum(msum);
                    if (ogrp == 0) pmass_cell[km] = t0 == 0 ? msum : pmass_cell[km] + msum;
                }
            }
        }
    }
}

// The window's entry point, one explicit instantiation per window in xna_kmeans_inst.hip: the cell kernel, then the pool kernel's gather.
template <int KS, int NCT>
static int xna_kmeans_launch_one(const XnaKmeansParams& p, float* A, hipStream_t s) {
    constexpr size_t lds = xna_kmeans_lds_for(KS, NCT);
    static_assert(lds <= 160 * 1024, "LDS budget");
    auto kern = xna_kmeans_kernel<KS, NCT>;
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) {
            naf_set_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize=%zu): %s", lds, hipGetErrorString(e));
            return NAF_ERR_LAUNCH;
        }
    }
    hipLaunchKernelGGL(kern, dim3(p.nblocks), dim3(XNA_POOL_NW * 64), lds, s, p);
    int rc = naf_check_launch("xna_kmeans_kernel");
    if (rc != NAF_OK) return rc;
    const size_t total = (size_t)p.B * p.heads * p.h * p.w * p.kpad;
    hipLaunchKernelGGL(xna_pool_gather_kernel<KS>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, p.part, A, p.B, p.heads, p.h, p.w, p.K, p.kpad);
    return naf_check_launch("xna_pool_gather_kernel");
}

template <int KS>
int xna_kmeans_launch_ks(const XnaKmeansParams& p, float* A, hipStream_t s) {
    if (p.kpad <= 32) return xna_kmeans_launch_one<KS, 2>(p, A, s);
    if (p.kpad <= 64) return xna_kmeans_launch_one<KS, 4>(p, A, s);
    naf_set_error("xna_kmeans: no kernel for kernel_size=%d and %d clusters", KS, p.K);
    return NAF_ERR_UNSUPPORTED;
}

// xna_kmeans_inst.hip (-DNAF_KS=<KS>) defines it, xna_kmeans.hip declares it (extern) and dispatches on the window.
#define NAF_XNA_KMEANS_WINDOW(LINKAGE, KS) LINKAGE template int xna_kmeans_launch_ks<KS>(const XnaKmeansParams&, float*, hipStream_t);
