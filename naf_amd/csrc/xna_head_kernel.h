// Cross-scale neighbourhood attention with a linear head folded in, head-summed MFMA cell kernel (gfx950 / CDNA4).
//
// out[b, y, x, n] = bias[n] + sum_g sum_slot P_g[px, slot] * PV_g[cell(slot), n]       (include/naf_hip.h: naf_xna_head_args)
// PV_g = W[:, g*Dv:(g+1)*Dv] @ V_g is formed by the host on the low-res grid; the [B, C, Ho, Wo] tensor never exists.
//
// The per-head arithmetic is xna_mfma_kernel.h's (read its header comment first): S^T = K . Q on v_mfma_f32_16x16x32_bf16 with K rows
// from LDS and Q straight from memory, fp32 softmax over the key slots, O^T += PV^T . P^T with PV^T through ds_read_b64_tr_b16.  What the
// head sum changes:
//   * one workgroup (8 waves) = one (batch, low-res cell); it LOOPS OVER THE HEADS.  Per head it stages that head's K window
//     [slots][64 (+8)] and PV window [slots][NCT*16 (+16)] in LDS (pad channels up to NCT*16 are zero-filled, never stored) and every wave
//     runs the head on its TPW 16-query row tiles.  The O^T accumulators of a tile are NOT cleared between heads.
//   * so 1/sum of a head cannot be applied to the accumulators at the end.  P is normalised in fp32 BEFORE it is packed to bf16 -- the
//     choice the per-head kernel already makes (softmax, then attn . V, as the reference orders it): every head's contribution then
//     carries exactly the rounding of one naf_xna_fwd call, the head sum adds nothing but fp32 additions, and no second set of
//     accumulators (a per-head partial to scale and add) is needed.  sum >= 1 (the max slot contributes exp2(0)), so a peaked softmax
//     normalises as safely as a flat one.
//   * per head: the head's queries are requested, then barrier, window staging (one L2 round trip), barrier, tiles.  Requesting the NEXT
//     head's queries and windows into registers before the current head's tiles (software pipelining) was built and measured: 146
//     registers instead of 120 (one workgroup per CU instead of two), G1 / N = 21 0.224 -> 0.266 ms, N = 151 0.667 -> 0.644 ms; not kept
//     (profiles/head_fused.txt).  The kernel is bound by instruction issue per (tile, head), not by memory latency.
//   * a round covers NW * TPW tiles of the cell (16 x 16 pixels at the default 8 x 2: the whole cell); larger cells take several rounds
//     and re-stage the windows per round (L2 hits).
//   * all heads of a pixel are read by the same workgroup: with channels-last guidance a workgroup reads, head by head, every 128-byte run of
//     its pixels' 512-byte (heads x 64 x bf16) rows: whole rows in the end, from one CU.  Rotate-on-load as in the cell kernel: the tile's RoPE table rows are fetched once per round (they
//     do not depend on the head) and applied with naf_rope_rotate, the same arithmetic and rounding as naf_rope_pool_fwd's.
//   * the bias is added in the epilogue in fp32; a lane stores its 4 consecutive channels of its own pixel, channels >= N masked.
//
// Classification epilogue (template parameter CE, naf_xna_head_ce_fwd): the logits instantiations (CE = false) are the code they were.  With
// CE a pixel's N logits z sit, in fp32, in the four lanes col + 16 * grp of its tile, so the softmax over the CLASSES is the reduction the
// softmax over the key slots already uses (naf_rows_max / naf_rows_sum), channels >= N masked as key slots >= NSLOT are:
//     m = max z, lse = m + ln(sum exp(z - m)), label = lowest n with z[n] = m, loss = lse - z[t], g[n] = exp(z[n] - lse) - (n == t)
//   The target is one 8-byte load per lane of the pixel (the four lanes read the same word) and is ONLY COMPARED with channel indices,
//   never used in an address: t == ignore_index or t outside [0, N) makes the pixel ignored (loss 0, g = 0).  Loss (fp32) and label (uint8)
//   are stored by the pixel's grp = 0 lane; g is rounded once to bf16 and stored as 8-byte vectors by the lanes that own the channels,
//   zeros for channels N .. gc-1 -- also past the NCT*16 accumulator channels (Npad = 160 -> gc = 192), so the host never clears the buffer.
//   Every output is optional (NULL: a wave-uniform branch).  No atomics, no cross-workgroup reduction: the host sums the loss map.
//
// Confusion matrix (Extra = XnaHeadCMExtra, naf_xna_head_cm_fwd): further instantiations of the classification epilogue; the CE = false and
// the XnaHeadCEExtra ones keep their code (`if constexpr`).  A pixel that is inside the image, of a live tile and not ignored adds one to
// confusion[t][label] (int64, caller-owned, accumulated).  Never one atomic per pixel: label and t are known to all four lanes of a pixel,
// so tile u of the wave puts its key t * 256 + label into the lanes grp == u (-1 = counts nothing: repeated last pixel of a partial tile,
// dead tile, ignored pixel), and after the tiles ONE ballot loop runs over the wave: take the key of the first lane left, ballot the
// lanes that hold it, that lane owns the population count, clear them, repeat.  A tile lies inside one low-res cell, so on a real
// segmentation this is one or two rounds.  The FIRST pair of every wave goes to LDS (64 bytes of static LDS, these instantiations only)
// and, after a barrier, eight lanes of wave 0 merge the eight pairs: a cell inside one segment costs ONE atomic per round instead
// of eight on the same address -- with every pixel of G1 / N = 21 on one counter 0.463 -> 0.206 ms (profiles/head_confusion.txt).  Later pairs
// of a wave are added directly.  The adds are no-return 64-bit vector atomics; integer adds commute exactly, so the matrix does not
// depend on the order.  t * cm_stride + label is the ONE address formed from the target, after t AND label have been checked to lie
// in [0, N) (a pixel whose logits are NaN has no maximum and counts nothing).
//
// Regression epilogue (Extra = XnaHeadRegExtra, naf_xna_head_reg_fwd): a third epilogue, instantiated for N <= 32 only (NCT = 2); the
// logits, XnaHeadCEExtra and XnaHeadCMExtra instantiations keep their code (`if constexpr`).  With z = acc + bias as above and a dense
// fp32 target t [B, N, Ho, Wo] read at element strides, r[n] = z[n] - t[n]; a pixel is valid when there is no mask or its uint8 mask
// value is not 0.  Target and mask are only read as values: no address is formed from them.
//     loss[px] = sum_n l(r[n]) (0 where invalid),  l = |r| (L1), r*r (MSE), |r| < beta ? 0.5*r*r/beta : |r| - 0.5*beta (SMOOTH_L1)
//     g[px, n] = sign(r) (L1), (bf16)(2.f * r) (MSE), |r| < beta ? r/beta : sign(r) (SMOOTH_L1); zeros for n >= N and invalid pixels
//   A lane adds its channels in ascending order, the four lanes of the pixel add with naf_rows_sum; the grp = 0 lane stores the loss.  g is
//   rounded once to bf16 and stored as 8-byte vectors by the owning lanes, every one of the gc channels written, as the CE dlogits is.
//   Error statistics (N == 1, the evaluation of a depth probe): p = min(max(z, clamp_lo), clamp_hi), a pixel is counted when it is valid,
//   t > 0 and t, z are finite; d = ln p - ln t; ten sums over the counted pixels: n, |p-t|, (p-t)^2, |p-t|/t, (p-t)^2/t, d, d^2 and the
//   three counts max(p/t, t/p) < 1.25^k.  No float atomics.  Channel 0 of a pixel is in its grp = 0 lane: per round that lane adds its
//   (at most TPW = 2) pixels in fp32, the 16 lanes of the row add in a four-level DPP tree (naf_cols_sum), and lane 0 adds the wave's ten
//   fp32 sums to the wave's row of fp64 accumulators in LDS (640 bytes of static LDS, these instantiations only).  After the last round
//   the eight rows are added in wave order in fp64 and the workgroup writes ONE row of ten fp64 partials to the caller's workspace
//   [nblocks][10]; naf_xna_head_reg_fwd's finishing kernel adds the rows in block order.  So the longest fp32 addition chain between a
//   pixel's term and the fp64 sums is 2 + 4 = 6 additions (well inside the 64 the interface promises), counts are integers below 2^24
//   in fp32 and exact in fp64, and the result is bit-reproducible.  Every output is optional (NULL: a wave-uniform branch).
#pragma once
#include "xna_mfma_kernel.h"

struct XnaHeadParams {
    const bf16_t* q;
    const bf16_t* k;
    const bf16_t* pv;
    const float* bias;   // [N] or nullptr
    void* out;
    const float* tab_y;  // rotate-on-load: RoPE tables [Ho][2][16] / [Wo][2][16], or nullptr
    const float* tab_x;
    int32_t B, heads, Ho, Wo, h, w, dy, dx;
    int32_t N;           // stored channels
    int32_t npad;        // channels a pv row holds (N rounded up to 16)
    uint32_t nblocks;
    float scale_log2e;
    int64_t qs[4], ks[4], vs[4];  // {b, head, y, x} element strides
    int64_t os[3];                // {b, y, x}
};

// the classification epilogue's arguments (CE = true instantiations only; XnaHeadParams::out may be nullptr there).  The kernel reads
// them from the kernel-argument segment in the epilogue, not before (see there): held across the head loop they are 34 more scalar
// registers than there are, spilled into vector lanes.
struct XnaHeadCEExtra {
    const int64_t* target;   // [B, Ho, Wo] or nullptr
    float* loss;             // per-pixel lse - z[t], or nullptr
    uint8_t* labels;         // per-pixel argmax, or nullptr
    bf16_t* dlogits;         // [B, Ho, Wo, gc] softmax - onehot, or nullptr
    int64_t ignore_index;
    int64_t ts[3], ls[3], bs[3], gs[3];   // {b, y, x} element strides of target / loss / labels / dlogits
    int32_t gc;              // channels of a dlogits row the kernel writes (multiple of 8, >= npad)
};
// ... and with a confusion matrix: XnaHeadCEExtra first, so the epilogue reads both through the same pointer
struct XnaHeadCMExtra {
    XnaHeadCEExtra ce;
    unsigned long long* confusion;   // [N][cm_stride] counts, row = target, column = label; never nullptr (host)
    int64_t cm_stride;               // >= N (host)
};
template <typename... T> struct XnaHeadIsCM { static constexpr bool value = false; };
template <> struct XnaHeadIsCM<XnaHeadCMExtra> { static constexpr bool value = true; };
// the regression epilogue's arguments (see the header comment); read from the kernel-argument segment in the epilogue like XnaHeadCEExtra
constexpr int XNA_HEAD_REG_STATS = 10;   // NAF_HEAD_REG_STATS of include/naf_hip.h
struct XnaHeadRegExtra {
    const float* target;     // [B, N, Ho, Wo] or nullptr
    const uint8_t* valid;    // [B, Ho, Wo] or nullptr (every pixel valid)
    float* loss;             // per-pixel sum over the channels, or nullptr
    bf16_t* dlogits;         // [B, Ho, Wo, gc] gradient of that sum, or nullptr
    double* partial;         // [nblocks][XNA_HEAD_REG_STATS] error statistics of the workgroups (N == 1, host), or nullptr
    int64_t ts[4];           // {b, n, y, x} element strides of target
    int64_t ms[3], ls[3], gs[3];   // {b, y, x} element strides of valid / loss / dlogits
    int32_t gc;              // channels of a dlogits row the kernel writes (multiple of 8, >= npad)
    int32_t kind;            // naf_head_reg_kind
    float beta, clamp_lo, clamp_hi;
};
template <typename... T> struct XnaHeadIsReg { static constexpr bool value = false; };
template <> struct XnaHeadIsReg<XnaHeadRegExtra> { static constexpr bool value = true; };
static_assert(alignof(XnaHeadRegExtra) == alignof(XnaHeadCEExtra), "both epilogue structs follow XnaHeadParams at XNA_HEAD_CE_ARG_OFFSET");
// they are the kernel's SECOND argument: it follows XnaHeadParams in the kernel-argument segment at its natural alignment
constexpr size_t XNA_HEAD_CE_ARG_OFFSET = (sizeof(XnaHeadParams) + alignof(XnaHeadCEExtra) - 1) / alignof(XnaHeadCEExtra) * alignof(XnaHeadCEExtra);

constexpr int XNA_HEAD_NW = 8;   // waves per workgroup
// channel tiles (16 channels each) a workgroup accumulates: the smallest of these that holds Npad
constexpr int xna_head_nct(int npad) { return npad <= 32 ? 2 : npad <= 64 ? 4 : npad <= 160 ? 10 : 16; }
// 16-query tiles a wave carries through the head loop (accumulators: TPW * NCT * 4 registers)
constexpr int xna_head_tpw(int ks, int nct) { return (nct >= 10 && ks >= 11) ? 1 : 2; }
constexpr size_t xna_head_lds_for(int ks, int nct) { return (size_t)(ks * ks) * (72 + nct * 16 + 16) * 2; }

// sum over the 16 lanes of a row (col = lane & 15), every lane gets it: two quad permutes, then the mirrors of 8 and of 16 lanes (DPP);
// a fixed four-level tree.  All lanes of the wave must be active.
__device__ __forceinline__ float naf_cols_sum(float v) {
    int b = __float_as_int(v);
    v += __int_as_float(__builtin_amdgcn_update_dpp(b, b, 0xB1, 0xf, 0xf, false));    // quad_perm [1, 0, 3, 2]
    b = __float_as_int(v);
    v += __int_as_float(__builtin_amdgcn_update_dpp(b, b, 0x4E, 0xf, 0xf, false));    // quad_perm [2, 3, 0, 1]
    b = __float_as_int(v);
    v += __int_as_float(__builtin_amdgcn_update_dpp(b, b, 0x141, 0xf, 0xf, false));   // row_half_mirror
    b = __float_as_int(v);
    return v + __int_as_float(__builtin_amdgcn_update_dpp(b, b, 0x140, 0xf, 0xf, false));   // row_mirror
}

// CE = false: the logits kernel, one argument, the code it was before the classification epilogue existed (a parameter of another type, even
// one that is the same struct, moves its instruction schedule).  CE = true: Extra = XnaHeadCEExtra, read through the segment pointer.
template <int KS, int NCT, typename OutT, bool CE = false, typename... Extra>
__global__ __launch_bounds__(XNA_HEAD_NW * 64) void xna_head_kernel(const XnaHeadParams p, const Extra... extra) {
    static_assert(sizeof...(Extra) == (CE ? 1 : 0), "the classification epilogue takes XnaHeadCEExtra as its second argument");
    constexpr bool CM = XnaHeadIsCM<Extra...>::value;   // ... or XnaHeadCMExtra: it counts into a confusion matrix as well
    constexpr bool REG = XnaHeadIsReg<Extra...>::value; // ... or XnaHeadRegExtra: the regression epilogue in place of the classification one
    constexpr int NW = XNA_HEAD_NW, NT = NW * 64;
    constexpr int TPW = xna_head_tpw(KS, NCT);
    using G = XnaGeom<KS, 1>;
    constexpr int NSLOT = G::NSLOT, MT = G::MT, KST = G::KST, KROW = G::KROW;
    constexpr int DVT = NCT * 16, VROW = XnaVRow<DVT>::VROW, VCH = DVT / 8;

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    bf16_t* Ks = reinterpret_cast<bf16_t*>(smem);
    bf16_t* Vs = Ks + NSLOT * KROW;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = lane & 15;  // MFMA column (query within the tile) / A-row index (key or channel)
    const int grp = lane >> 4;  // MFMA k-group / result row group

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
    OutT* o_cell = reinterpret_cast<OutT*>(p.out) + b * p.os[0] + (int64_t)(cy * p.dy) * p.os[1] + (int64_t)(cx * p.dx) * p.os[2];
    const bf16_t* kb = p.k + b * p.ks[0];
    const bf16_t* vb = p.pv + b * p.vs[0];

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

    for (int t0 = 0; t0 < ntile; t0 += NW * TPW) {
        // this wave's tiles of the round: t0 + u * NW + wave (wave-uniform); a tile past the cell is computed on clamped
        // addresses and never stored
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
            if (rope) {
                // head dims [grp*8, +8) and their partners +32: dims < 16 turn with the row angle, dims >= 16 with the column angle
                const float* tr = ((grp >> 1) ? p.tab_x + (int64_t)(cx * p.dx + xl) * 32 : p.tab_y + (int64_t)(cy * p.dy + tyv[u]) * 32) + (grp & 1) * 8;
                cs[u][0] = *reinterpret_cast<const f32x4_t*>(tr);
                cs[u][1] = *reinterpret_cast<const f32x4_t*>(tr + 4);
                cs[u][2] = *reinterpret_cast<const f32x4_t*>(tr + 16);
                cs[u][3] = *reinterpret_cast<const f32x4_t*>(tr + 20);
            }
        }
        f32x4_t acc[TPW][NCT];
#pragma unroll
        for (int u = 0; u < TPW; ++u)
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) acc[u][ct] = f32x4_t{0.f, 0.f, 0.f, 0.f};

        for (int head = 0; head < p.heads; ++head) {
            // the head's queries are requested first: their latency hides under the window staging and the barrier
            bf16x8_t qf[TPW][2];
#pragma unroll
            for (int u = 0; u < TPW; ++u) {
                const bf16_t* qp = qpv[u] + head * p.qs[1];
                qf[u][0] = *reinterpret_cast<const bf16x8_t*>(qp);
                qf[u][1] = *reinterpret_cast<const bf16x8_t*>(qp + 32);
            }
            __syncthreads();   // every wave is done with the previous head's windows
            {
                // ---- stage the K and PV windows (L2 -> registers -> LDS): all loads of a batch before its first LDS write
                const bf16_t* kh = kb + head * p.ks[1];
                const bf16_t* vh = vb + head * p.vs[1];
                constexpr int KTOT = NSLOT * 8, VTOT = NSLOT * VCH;
                constexpr int KIT = (KTOT + NT - 1) / NT, VIT = (VTOT + NT - 1) / NT;
                constexpr int BATCH = 8;
                const int vch_mem = p.npad >> 3;   // 16-byte chunks a pv row holds in memory; the rest of the LDS row is zero
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
                // ---- softmax over the key slots, fp32; P is normalised before it is rounded to bf16 (see the header comment) ----
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
                    // wide heads: keep the scheduler from hoisting every channel tile's PV^T fragments above the first MFMA (it spills)
                    if constexpr (NCT * KST >= 40) __builtin_amdgcn_sched_barrier(0);
                }
            }
        }

        if constexpr (REG) {
            // ---- regression epilogue (see the header comment): residual, loss map, its gradient, error statistics ----
            static_assert(NCT == 2, "the regression epilogue is instantiated for N <= 32 only");
            // the epilogue's arguments and the lane's coordinates are made opaque for the reasons given in the classification epilogue below
            const char __attribute__((address_space(4)))* ka = (const char __attribute__((address_space(4)))*)__builtin_amdgcn_kernarg_segment_ptr();
            asm volatile("" : "+s"(ka));
            int ecol = col, egrp = grp, elane = lane;
            asm volatile("" : "+v"(ecol), "+v"(egrp), "+v"(elane));
            const XnaHeadRegExtra __attribute__((address_space(4)))* x = reinterpret_cast<const XnaHeadRegExtra __attribute__((address_space(4)))*>(ka + XNA_HEAD_CE_ARG_OFFSET);
            __shared__ double reg_acc[NW][XNA_HEAD_REG_STATS];   // each wave's sums over the rounds so far; only that wave touches its row
            const bool have_t = x->target != nullptr, stats = x->partial != nullptr;   // wave-uniform
            float es[XNA_HEAD_REG_STATS] = {};
#pragma unroll
            for (int u = 0; u < TPW; ++u) {
                if (!livev[u]) continue;   // wave-uniform: the four-lane reduction below runs on whole waves
                const bool inpx = tx0v[u] + ecol < p.dx;
                const int64_t gy = cy * p.dy + tyv[u];
                const int64_t gx = cx * p.dx + min(tx0v[u] + ecol, p.dx - 1);   // lanes past a partial last tile repeat its last pixel, store nothing
                bool ok = true;
                if (x->valid != nullptr) ok = x->valid[b * x->ms[0] + gy * x->ms[1] + gx * x->ms[2]] != 0;
                const float* tp = x->target + b * x->ts[0] + gy * x->ts[2] + gx * x->ts[3];
                float lsum = 0.f, tc0 = 0.f;
                bf16x4_t gv[NCT];
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int ch = ct * 16 + egrp * 4 + r;
                        float g = 0.f;
                        if (ch < p.N) {
                            // z = acc + bias: the expression of the logits epilogue, so a stored z is the logit naf_xna_head_fwd stores
                            const float z = acc[u][ct][r] + (p.bias != nullptr ? p.bias[ch] : 0.f);
                            acc[u][ct][r] = z;
                            if (have_t) {
                                const float t = tp[ch * x->ts[1]];
                                if (ct == 0 && r == 0) tc0 = t;
                                const float rr = z - t, a = fabsf(rr);
                                const float sg = rr > 0.f ? 1.f : (rr < 0.f ? -1.f : 0.f);
                                float term;
                                if (x->kind == NAF_HEAD_REG_L1) {
                                    term = a;
                                    g = sg;
                                } else if (x->kind == NAF_HEAD_REG_MSE) {
                                    term = rr * rr;
                                    g = 2.f * rr;
                                } else {
                                    const bool small = a < x->beta;
                                    term = small ? (0.5f * rr) * rr / x->beta : a - 0.5f * x->beta;
                                    g = small ? rr / x->beta : sg;
                                }
                                lsum += term;
                            }
                        }
                        gv[ct][r] = (bf16_t)(ok ? g : 0.f);
                    }
                lsum = naf_rows_sum(lsum);
                if (egrp == 0 && inpx && x->loss != nullptr) x->loss[b * x->ls[0] + gy * x->ls[1] + gx * x->ls[2]] = ok ? lsum : 0.f;
                if (p.out != nullptr && inpx) {
                    OutT* op = o_cell + (int64_t)tyv[u] * p.os[1] + (int64_t)(tx0v[u] + ecol) * p.os[2];
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int ch = ct * 16 + egrp * 4 + r;
                            if (ch < p.N) op[ch] = (OutT)acc[u][ct][r];
                        }
                }
                if (x->dlogits != nullptr && inpx) {
                    bf16_t* gp = x->dlogits + b * x->gs[0] + gy * x->gs[1] + gx * x->gs[2];
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct) {
                        const int c0 = ct * 16 + egrp * 4;
                        if (c0 >= x->gc) continue;   // gc is a multiple of 8: a lane's four channels are all inside or all outside
                        *reinterpret_cast<bf16x4_t*>(gp + c0) = gv[ct];
                    }
                    // channels past the accumulators (gc > 32): plain zero stores
                    for (int c0 = DVT + egrp * 4; c0 < x->gc; c0 += 16) *reinterpret_cast<bf16x4_t*>(gp + c0) = bf16x4_t{(bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f};
                }
                if (stats) {
                    // N == 1 (host): the pixel's one channel is in its grp = 0 lane.  What a lane that does not count computes is discarded.
                    const float z = acc[u][0][0];
                    const bool cnt = egrp == 0 && inpx && ok && tc0 > 0.f && tc0 < INFINITY && fabsf(z) < INFINITY;
                    const float pz = fminf(fmaxf(z, x->clamp_lo), x->clamp_hi);
                    const float e = pz - tc0, ae = fabsf(e), e2 = e * e;
                    const float d = logf(pz) - logf(tc0);
                    const float ratio = fmaxf(pz / tc0, tc0 / pz);
                    es[0] += cnt ? 1.f : 0.f;
                    es[1] += cnt ? ae : 0.f;
                    es[2] += cnt ? e2 : 0.f;
                    es[3] += cnt ? ae / tc0 : 0.f;
                    es[4] += cnt ? e2 / tc0 : 0.f;
                    es[5] += cnt ? d : 0.f;
                    es[6] += cnt ? d * d : 0.f;
                    es[7] += (cnt && ratio < 1.25f) ? 1.f : 0.f;
                    es[8] += (cnt && ratio < 1.5625f) ? 1.f : 0.f;
                    es[9] += (cnt && ratio < 1.953125f) ? 1.f : 0.f;
                }
            }
            if (stats) {
#pragma unroll
                for (int i = 0; i < XNA_HEAD_REG_STATS; ++i) {
                    const float v = naf_cols_sum(es[i]);   // lane 0: the sum over the grp = 0 lanes, which hold the pixels
                    if (elane == 0) reg_acc[wave][i] = (t0 == 0 ? 0.0 : reg_acc[wave][i]) + (double)v;   // the first round starts the sums
                }
                if (t0 + NW * TPW >= ntile) {   // the last round (uniform over the workgroup): the eight rows in wave order, one row out
                    __syncthreads();
                    if (wave == 0 && elane < XNA_HEAD_REG_STATS) {
                        double sum = 0.0;
#pragma unroll
                        for (int j = 0; j < NW; ++j) sum += reg_acc[j][elane];
                        x->partial[(int64_t)blockIdx.x * XNA_HEAD_REG_STATS + elane] = sum;
                    }
                }
            }
        } else if constexpr (CE) {
            // ---- classification epilogue (see the header comment): softmax over the classes, loss, label, softmax - onehot ----
            constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;
            // the epilogue's own arguments, fetched from the kernel-argument segment HERE: the empty asm makes the address opaque, so the
            // scalar loads cannot be hoisted above the head loop and held in registers across it
            const char __attribute__((address_space(4)))* ka = (const char __attribute__((address_space(4)))*)__builtin_amdgcn_kernarg_segment_ptr();
            asm volatile("" : "+s"(ka));
            // ... and the same for the lane's coordinates: what the epilogue derives from them (addresses, bias loads) is invariant in the
            // head loop and would be hoisted above it, 21 vector registers held through the loop (143 instead of 120 at 7 x 7, N <= 32)
            int ecol = col, egrp = grp;
            asm volatile("" : "+v"(ecol), "+v"(egrp));
            const XnaHeadCEExtra __attribute__((address_space(4)))* x = reinterpret_cast<const XnaHeadCEExtra __attribute__((address_space(4)))*>(ka + XNA_HEAD_CE_ARG_OFFSET);
            [[maybe_unused]] int cmkey = -1;   // CM: t * 256 + label of tile u's pixel in the lanes grp == u, -1 = counts nothing
            static_assert(!CM || TPW <= 4, "one lane group per tile of the wave");
#pragma unroll
            for (int u = 0; u < TPW; ++u) {
                if (!livev[u]) continue;   // wave-uniform: the four-lane reductions below run on whole waves
                const bool inpx = tx0v[u] + ecol < p.dx;
                const int64_t gy = cy * p.dy + tyv[u];
                const int64_t gx = cx * p.dx + min(tx0v[u] + ecol, p.dx - 1);   // lanes past a partial last tile repeat its last pixel, store nothing
                // z = acc + bias: the expression of the logits epilogue, so a stored z is the logit naf_xna_head_fwd stores
                float m = -INFINITY;
                int am = 0;
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int ch = ct * 16 + egrp * 4 + r;
                        if (ch < p.N) {
                            const float z = acc[u][ct][r] + (p.bias != nullptr ? p.bias[ch] : 0.f);
                            acc[u][ct][r] = z;
                            if (z > m) {   // a lane's channels ascend with (ct, r): the first of equal maxima stays
                                m = z;
                                am = ch;
                            }
                        }
                    }
                const float mall = naf_rows_max(m);
                // lowest index among the lanes that hold the maximum: indices <= 255 are exact in fp32
                const int label = (int)(-naf_rows_max(m == mall ? -(float)am : -INFINITY));
                int t = -1;   // the target as a channel index, -1 = ignored
                if (x->target != nullptr) {
                    const int64_t tv = x->target[b * x->ts[0] + gy * x->ts[1] + gx * x->ts[2]];
                    t = (tv != x->ignore_index && tv >= 0 && tv < (int64_t)p.N) ? (int)tv : -1;
                }
                float sum = 0.f, zt = 0.f;
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int ch = ct * 16 + egrp * 4 + r;
                        if (ch < p.N) {
                            sum += __builtin_amdgcn_exp2f((acc[u][ct][r] - mall) * LOG2E);
                            zt += ch == t ? acc[u][ct][r] : 0.f;   // one lane of the four holds z[t]
                        }
                    }
                sum = naf_rows_sum(sum);   // >= 1: the maximum contributes exp2(0)
                zt = naf_rows_sum(zt);
                if (egrp == 0 && inpx) {
                    if (x->loss != nullptr)
                        x->loss[b * x->ls[0] + gy * x->ls[1] + gx * x->ls[2]] = t >= 0 ? (mall + __builtin_amdgcn_logf(sum) * LN2) - zt : 0.f;
                    if (x->labels != nullptr) x->labels[b * x->bs[0] + gy * x->bs[1] + gx * x->bs[2]] = (uint8_t)label;
                }
                if constexpr (CM) {
                    // 0 <= t < N <= 256 (checked above); label < N unless the logits are NaN (no lane holds the maximum): such a pixel counts nothing
                    if (egrp == u && inpx && t >= 0 && (unsigned)label < (unsigned)p.N) cmkey = t * 256 + label;
                }
                if (p.out != nullptr && inpx) {
                    OutT* op = o_cell + (int64_t)tyv[u] * p.os[1] + (int64_t)(tx0v[u] + ecol) * p.os[2];
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int ch = ct * 16 + egrp * 4 + r;
                            if (ch < p.N) op[ch] = (OutT)acc[u][ct][r];
                        }
                }
                if (x->dlogits != nullptr && inpx) {
                    bf16_t* gp = x->dlogits + b * x->gs[0] + gy * x->gs[1] + gx * x->gs[2];
                    const float inv = __builtin_amdgcn_rcpf(sum);
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct) {
                        const int c0 = ct * 16 + egrp * 4;
                        if (c0 >= x->gc) continue;   // gc is a multiple of 8: a lane's four channels are all inside or all outside
                        bf16x4_t gv;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int ch = c0 + r;
                            const float e = __builtin_amdgcn_exp2f((acc[u][ct][r] - mall) * LOG2E) * inv - (ch == t ? 1.f : 0.f);
                            gv[r] = (bf16_t)((ch < p.N && t >= 0) ? e : 0.f);
                        }
                        *reinterpret_cast<bf16x4_t*>(gp + c0) = gv;
                    }
                    // channels past the accumulators (Npad = 160 -> gc = 192): plain zero stores
                    for (int c0 = DVT + egrp * 4; c0 < x->gc; c0 += 16) *reinterpret_cast<bf16x4_t*>(gp + c0) = bf16x4_t{(bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f};
                }
            }
            if constexpr (CM) {
                // ---- confusion[t][label] += 1 per counted pixel, aggregated over the wave and then over the workgroup (see the header comment) ----
                const XnaHeadCMExtra __attribute__((address_space(4)))* xc = reinterpret_cast<const XnaHeadCMExtra __attribute__((address_space(4)))*>(ka + XNA_HEAD_CE_ARG_OFFSET);
                int elane = lane;   // opaque like ecol / egrp: nothing of this block is computed above the head loop and held through it
                asm volatile("" : "+v"(elane));
                __shared__ int cm_key[NW], cm_cnt[NW];   // each wave's first (key, count) pair of the round; -1 = none
                auto count = [&](int key, int n) __attribute__((always_inline)) {
                    __hip_atomic_fetch_add(xc->confusion + (int64_t)(key >> 8) * xc->cm_stride + (key & 255), (unsigned long long)n, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
                };
                unsigned long long todo = __ballot(cmkey >= 0);
                bool first = true;
                if (todo == 0ull && elane == 0) cm_key[wave] = -1;
                while (todo != 0ull) {   // wave-uniform
                    const int lead = __builtin_ctzll(todo);
                    const int key = __builtin_amdgcn_readlane(cmkey, lead);
                    const unsigned long long same = __ballot(cmkey == key);
                    const int n = __builtin_popcountll(same);
                    if (elane == lead) {
                        if (first) {   // wave-uniform: to the workgroup's merge
                            cm_key[wave] = key;
                            cm_cnt[wave] = n;
                        } else {
                            count(key, n);
                        }
                    }
                    first = false;
                    todo &= ~same;
                }
                __syncthreads();   // the next round writes these slots only after two more barriers (head loop): wave 0 has read them by then
                if (wave == 0) {
                    // lane i < NW takes wave i's pair; the lowest lane of every distinct key adds the sum of that key's counts
                    const int kk = elane < NW ? cm_key[elane & (NW - 1)] : -1, cc = cm_cnt[elane & (NW - 1)];
                    int n = 0;
                    bool lowest = kk >= 0;
#pragma unroll
                    for (int j = 0; j < NW; ++j) {
                        const int kj = __builtin_amdgcn_readlane(kk, j), cj = __builtin_amdgcn_readlane(cc, j);
                        n += kj == kk ? cj : 0;
                        lowest = lowest && !(kj == kk && j < elane);
                    }
                    if (lowest) count(kk, n);
                }
            }
        } else {
            // ---- epilogue: + bias (fp32), store the N real channels of this lane's pixel ----
#pragma unroll
            for (int u = 0; u < TPW; ++u) {
                if (!livev[u] || tx0v[u] + col >= p.dx) continue;
                OutT* op = o_cell + (int64_t)tyv[u] * p.os[1] + (int64_t)(tx0v[u] + col) * p.os[2];
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int ch = ct * 16 + grp * 4 + r;
                        if (ch < p.N) op[ch] = (OutT)(acc[u][ct][r] + (p.bias != nullptr ? p.bias[ch] : 0.f));
                    }
                }
            }
        }
    }
}

// One launcher for the four variants: no Extra = logits, XnaHeadCEExtra = classification epilogue, XnaHeadCMExtra = ... with a
// confusion matrix, XnaHeadRegExtra = regression epilogue.  The optional outputs of an epilogue are run-time NULL checks inside the kernel.
template <int KS, int NCT, typename OutT, typename... Extra>
static int xna_head_launch_one(const XnaHeadParams& p, hipStream_t s, const char* what, const Extra&... extra) {
    constexpr size_t lds = xna_head_lds_for(KS, NCT);
    static_assert(lds <= 160 * 1024, "LDS budget");
    auto kern = xna_head_kernel<KS, NCT, OutT, sizeof...(Extra) != 0, Extra...>;
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) {
            naf_set_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize=%zu): %s", lds, hipGetErrorString(e));
            return NAF_ERR_LAUNCH;
        }
    }
    hipLaunchKernelGGL(kern, dim3(p.nblocks), dim3(XNA_HEAD_NW * 64), lds, s, p, extra...);
    return naf_check_launch(what);
}

// The window's entry point, one explicit instantiation per variant in xna_head_inst.hip.  `who` names the variant in the messages
// ("xna_head", "xna_head_ce", "xna_head_cm", "xna_head_reg"); the logits variant stores bf16 or float, the epilogues float only.
template <int KS, typename... Extra>
int xna_head_launch_ks(const XnaHeadParams& p, int out_dtype, hipStream_t s, const char* who, const char* what, const Extra&... extra) {
    const int nct = xna_head_nct(p.npad);
#define NAF_HEAD_CASE(C)                                                                                               \
    if (nct == C) {                                                                                                    \
        if constexpr (sizeof...(Extra) == 0)                                                                           \
            if (out_dtype == NAF_BF16) return xna_head_launch_one<KS, C, bf16_t>(p, s, what);                          \
        return xna_head_launch_one<KS, C, float>(p, s, what, extra...);                                                \
    }
    NAF_HEAD_CASE(2)
    if constexpr (!XnaHeadIsReg<Extra...>::value) {   // the regression epilogue serves N <= 32 only (the host refuses more)
        NAF_HEAD_CASE(4)
        NAF_HEAD_CASE(10)
        NAF_HEAD_CASE(16)
    }
#undef NAF_HEAD_CASE
    naf_set_error("%s: no kernel for kernel_size=%d channel tiles=%d", who, KS, nct);
    return NAF_ERR_UNSUPPORTED;
}

// xna_head_inst.hip (-DNAF_KS=<KS>) defines these four, xna_head.hip declares them (extern) and dispatches on the window.
#define NAF_XNA_HEAD_WINDOW(LINKAGE, KS)                                                                                                        \
    LINKAGE template int xna_head_launch_ks<KS>(const XnaHeadParams&, int, hipStream_t, const char*, const char*);                              \
    LINKAGE template int xna_head_launch_ks<KS>(const XnaHeadParams&, int, hipStream_t, const char*, const char*, const XnaHeadCEExtra&);       \
    LINKAGE template int xna_head_launch_ks<KS>(const XnaHeadParams&, int, hipStream_t, const char*, const char*, const XnaHeadCMExtra&);       \
    LINKAGE template int xna_head_launch_ks<KS>(const XnaHeadParams&, int, hipStream_t, const char*, const char*, const XnaHeadRegExtra&);
