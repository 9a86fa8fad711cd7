// Cross-scale neighbourhood attention with a COSINE head folded in, head-summed MFMA cell kernel (gfx950 / CDNA4).
//
// out[b, y, x, n] = logit_scale * (sum_g sum_slot P_g[px, slot] * PV_g[cell(slot), n]) / max(||f[px]||, 1e-12)   (include/naf_hip.h: naf_xna_cos_args)
// f[px] = the upsampled feature of the pixel, all heads' channels: f_g = sum_slot P_g[px, slot] * V_g[cell(slot), :].  PV_g = E^[:, g*Dv:(g+1)*Dv] @ V_g
// is formed by the host on the low-res grid from the NORMALISED rows E^ of the embedding matrix; f is never written.
//
// The numerator is xna_head_kernel.h's logits kernel (read its header comment first): one workgroup (8 waves) = one (batch, low-res
// cell), it loops over the heads, stages the head's K and PV windows in LDS, S^T = K . Q on v_mfma_f32_16x16x32_bf16, fp32 softmax over
// the key slots, P normalised in fp32 BEFORE it is packed to bf16, O^T += PV^T . P^T with the accumulators kept across the heads;
// rotate-on-load with naf_rope_rotate.  What the cosine adds is the DENOMINATOR:
//   * the head's VALUE window is staged in LDS as well, in channel chunks of XNA_COS_DVC = 64 ([slots][64 (+16)] bf16; a chunk past Dv is
//     zero-filled, its channel tiles are skipped).  Per chunk and 16-channel tile the wave forms F^T = V^T . P^T on the same MFMA with the
//     SAME packed P as the numerator, adds the squares of the four fp32 results of the lane into ONE fp32 sum per tile of the wave (fmaf,
//     fixed order) and drops them: P . V is never stored.  Chunks of a head and the heads themselves simply add.
//   * a head of more than 64 value channels takes several chunks: chunk 0 is staged with the K and PV windows, every further chunk
//     between two more barriers; the packed P of the wave's tiles is kept in registers across them.
//   * after the head loop the lane's partial sum holds the channels grp*4 + r of every tile; the four lanes col + 16 * grp of a pixel are
//     added with naf_rows_sum (the reduction the softmax over the key slots and the class softmax use; fixed order).
//   * epilogue: nrm = sqrt(sum), inv = 1 / max(nrm, 1e-12), out = logit_scale * (acc * inv), channels >= N masked; norms (optional, NULL:
//     a wave-uniform branch) receives nrm, fp32 and unclamped, from the pixel's grp = 0 lane.  A pixel whose window holds only zero
//     features has acc = 0 and sum = 0: out = 0 * 1e12 = 0, never NaN.  sqrt and the divide are the correctly rounded ones.
//   * no atomics, nothing crosses a workgroup: two launches give the same bits.
//   * the epilogue's own arguments (XnaCosEpilogue) are the kernel's second argument and are read from the kernel-argument segment in the
//     epilogue, behind an opaque address, as the classification epilogue of xna_head_kernel.h does: held across the head loop they cost
//     scalar registers the loop does not have.
// Which (window, channel tiles) instantiations exist and which of them the dispatcher serves is decided by the compiler's figures
// (profiles/cosine_head.txt): xna_cos_served below.
//
// Classification epilogue (template parameter Epi = XnaCosCEEpilogue, naf_xna_cos_ce_fwd): the cosine instantiations (Epi = XnaCosEpilogue)
// are the code they were (`if constexpr`).  With it a pixel's N scaled cosines z[n] = s * (acc[n] * inv) sit, in fp32, in the four lanes
// col + 16 * grp of its tile, where xna_head_kernel.h's classification epilogue finds its logits, and the arithmetic is that epilogue's:
//     m = max z, lse = m + ln(sum exp(z - m)), label = lowest n with z[n] = m, loss = lse - z[t],
//     g'[n] = (s * inv) * (exp(z[n] - lse) - (n == t))          rounded once to bf16: dL/d(acc[n]), the `dout` of naf_xna_bwd for all heads
//     ds    = sum_n (exp(z[n] - lse) - (n == t)) * (acc[n] * inv)   fp32, the lane's channels in ascending order, then naf_rows_sum
//   The norm does not depend on the embeddings, so g' is the whole gradient with respect to PV.  acc keeps the UNSCALED cosines and z is
//   formed from them where it is used; the block contracts nothing (fp contract off), so every use of z[n] has the bits the cosine
//   instantiation stores.  The target is only compared with channel indices; t == ignore_index or t outside [0, N): loss 0, g' = 0, ds = 0.
//   A pixel of norm 0 has every cosine 0 and loss ln N; its exact gradient is 0 (dE^ = sum_px g' f, f = 0): g' is stored as zeros, not as
//   1e12 * (softmax - onehot); ds = 0 follows from acc = 0.  g' is written as 8-byte vectors over all gc channels, zeros from N up, also
//   past the NCT*16 accumulator channels.  s is the struct's float, or one fp32 device value behind scale_ptr, read once per round of the
//   epilogue.  Every output is optional (NULL: a wave-uniform branch); vector stores only, no atomics, nothing crosses a workgroup.
//   Tiles per wave and which pairs exist: xna_cos_ce_tpw / xna_cos_ce_served (profiles/cosine_objective.txt).
//
// Peak epilogue (Epi = XnaCosPeakEpilogue, naf_xna_cos_peaks_fwd): the maximum of every channel over the PIXELS of the cell and where it
// is, so that the N-channel map need not exist.  z = logit_scale * (acc * inv) is the cosine epilogue's expression (nothing is
// contracted), so a peak has the bits naf_xna_cos_fwd stores; `out` stays optional and receives exactly those.  The pixel is on
// col = lane & 15, so the reduction runs across the 16 lanes of a row (naf_cols_max: DPP, no LDS), the direction naf_rows_max does not
// cover.  The comparator on (value, flat index y * Wo + x) is "greater value, or equal value and lower index": a total order, so the
// shape of the reduction cannot change the result.  Stages:
//   1. per live tile and channel: the row's maximum, then the lowest col that holds it (a ballot; a lower col is a lower index).  Lanes
//      past a partial last tile repeat the row's last pixel: they hold that pixel's value and can only tie with it, at a higher col.
//   2. lane col = r of a row owns channel ct*16 + grp*4 + r: it compare-updates the wave's own LDS array [wave][channel] of pairs (the
//      same lane reads and writes a slot: no race, no barrier).  The array lies past xna_cos_lds_for: K / PV / V are restaged every
//      round.  Tiles past the cell never get here; a wave without a live tile leaves (-inf, INT_MAX), which loses to everything.
//   3. after the last round: a barrier, thread n < N merges the eight waves' pairs and stores peak / where [b, cy, cx, n].
//   Vector stores only, no atomics, nothing crosses a workgroup.  Tiles per wave and which pairs exist: xna_cos_peak_tpw /
//   xna_cos_peak_served (profiles/cosine_peaks.txt).
#pragma once
#include "xna_head_kernel.h"

struct XnaCosParams {
    const bf16_t* q;
    const bf16_t* k;
    const bf16_t* pv;
    const bf16_t* v;
    float* out;
    const float* tab_y;  // rotate-on-load: RoPE tables [Ho][2][16] / [Wo][2][16], or nullptr
    const float* tab_x;
    int32_t B, heads, Ho, Wo, h, w, dy, dx;
    int32_t N;           // stored channels
    int32_t npad;        // channels a pv row holds (N rounded up to 16)
    int32_t dv;          // value channels of a head (a multiple of 16)
    uint32_t nblocks;
    float scale_log2e;
    int64_t qs[4], ks[4], vs[4], ws[4];  // {b, head, y, x} element strides of q, k, pv, v
    int64_t os[3];                       // {b, y, x}
};
// read in the epilogue only (see the header comment)
struct XnaCosEpilogue {
    float* norms;        // [B, Ho, Wo] by ns, or nullptr
    int64_t ns[3];       // {b, y, x}
    float logit_scale;
};
// ... and with the classification epilogue: XnaCosEpilogue first, so both are read through the same pointer (cos.out / norms stay optional)
struct XnaCosCEEpilogue {
    XnaCosEpilogue cos;
    const int64_t* target;     // [B, Ho, Wo] or nullptr
    float* loss;               // per-pixel lse - z[t], or nullptr
    uint8_t* labels;           // per-pixel argmax, or nullptr
    bf16_t* dlogits;           // [B, Ho, Wo, gc] g', or nullptr
    float* dscale;             // per-pixel ds, or nullptr
    const float* scale_ptr;    // one fp32 device value that replaces cos.logit_scale, or nullptr
    int64_t ignore_index;
    int64_t ts[3], ls[3], bs[3], gs[3], ds[3];   // {b, y, x} element strides of target / loss / labels / dlogits / dscale
    int32_t gc;                // channels of a dlogits row the kernel writes (multiple of 8, >= npad)
};
// ... and with the peak epilogue: XnaCosEpilogue first as well
struct XnaCosPeakEpilogue {
    XnaCosEpilogue cos;
    float* peak;               // [B, h, w, N] by ps: the cell's maximum
    int32_t* where;            // [B, h, w, N] by is: its flat index y * Wo + x
    int64_t ps[3], is[3];      // {b, cy, cx} element strides, channels contiguous
};
template <typename T> struct XnaCosIsCE { static constexpr bool value = false; };
template <> struct XnaCosIsCE<XnaCosCEEpilogue> { static constexpr bool value = true; };
template <typename T> struct XnaCosIsPeak { static constexpr bool value = false; };
template <> struct XnaCosIsPeak<XnaCosPeakEpilogue> { static constexpr bool value = true; };
constexpr size_t XNA_COS_ARG_OFFSET = (sizeof(XnaCosParams) + alignof(XnaCosEpilogue) - 1) / alignof(XnaCosEpilogue) * alignof(XnaCosEpilogue);

constexpr int XNA_COS_DVC = 64;   // value channels staged at a time
constexpr size_t xna_cos_lds_for(int ks, int nct) { return (size_t)(ks * ks) * (72 + nct * 16 + 16 + XNA_COS_DVC + 16) * 2; }
// 16-query tiles a wave carries through the head loop: the head kernel's two, and one where two tiles' accumulators, their packed P
// (kept across the value chunks) and the window's scores spill (the compiler's figures: profiles/cosine_head.txt)
constexpr int xna_cos_tpw(int ks, int nct) { return (xna_head_tpw(ks, nct) == 1 || ks >= 15 || (nct >= 10 && ks >= 9) || (nct >= 16 && ks >= 7)) ? 1 : 2; }
// instantiated: the windows fit the 160 KB of LDS (15 x 15 with 16 channel tiles does not)
constexpr bool xna_cos_fits(int ks, int nct) { return xna_cos_lds_for(ks, nct) <= 160 * 1024; }
// served: instantiated and free of scratch.  13 x 13 and 15 x 15 with 10 or 16 channel tiles (N > 64) spill even with one tile per wave
// (36 .. 260 bytes per lane): naf_xna_cos_select answers -NAF_ERR_UNSUPPORTED for them and the caller composes.
// (tools/cosine_head_time.py --resources compiles with -DNAF_XNA_COS_ALL to put the figures of the excluded ones on record.)
#ifdef NAF_XNA_COS_ALL
constexpr bool xna_cos_served(int ks, int nct) { return xna_cos_fits(ks, nct); }
#else
constexpr bool xna_cos_served(int ks, int nct) { return xna_cos_fits(ks, nct) && !(ks >= 13 && nct >= 10); }
#endif

// the classification epilogue's instantiations: tiles per wave and which exist, from the compiler's figures as above
// (profiles/cosine_objective.txt; tools/cosine_objective_time.py --resources).  Sixteen channel tiles with two tiles per wave spill in
// the epilogue at windows 3 and 5 (24 / 36 bytes per lane): one tile per wave there.  With that, every pair the cosine kernel serves is
// free of scratch with the epilogue too; windows 13 and 15 with 10 or 16 channel tiles spill in the head loop as the cosine kernel does.
constexpr int xna_cos_ce_tpw(int ks, int nct) { return nct >= 16 ? 1 : xna_cos_tpw(ks, nct); }
#ifdef NAF_XNA_COS_ALL
constexpr bool xna_cos_ce_served(int ks, int nct) { return xna_cos_fits(ks, nct); }
#else
constexpr bool xna_cos_ce_served(int ks, int nct) { return xna_cos_served(ks, nct); }
#endif

// the peak epilogue's instantiations, from the compiler's figures as above (profiles/cosine_peaks.txt; tools/cosine_peaks_time.py
// --resources).  Its per-wave pairs [8 waves][NCT * 16 channels] x 8 bytes follow the staged windows in LDS.
constexpr int xna_cos_peak_tpw(int ks, int nct) { return xna_cos_ce_tpw(ks, nct); }
constexpr size_t xna_cos_peak_lds(int nct) { return (size_t)XNA_HEAD_NW * nct * 16 * 8; }
#ifdef NAF_XNA_COS_ALL
constexpr bool xna_cos_peak_served(int ks, int nct) { return xna_cos_fits(ks, nct); }
#else
constexpr bool xna_cos_peak_served(int ks, int nct) { return xna_cos_served(ks, nct); }
#endif

// max over the 16 lanes of a row (col = lane & 15), every lane gets it: two quad permutes, then the mirrors of 8 and of 16 lanes (DPP)
__device__ __forceinline__ float naf_cols_max(float v) {
    int b = __float_as_int(v);
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(b, b, 0xB1, 0xf, 0xf, false)));    // quad_perm [1, 0, 3, 2]
    b = __float_as_int(v);
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(b, b, 0x4E, 0xf, 0xf, false)));    // quad_perm [2, 3, 0, 1]
    b = __float_as_int(v);
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(b, b, 0x141, 0xf, 0xf, false)));   // row_half_mirror
    b = __float_as_int(v);
    return fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(b, b, 0x140, 0xf, 0xf, false)));   // row_mirror
}

template <int KS, int NCT, typename Epi = XnaCosEpilogue>
__global__ __launch_bounds__(XNA_HEAD_NW * 64) void xna_cos_kernel(const XnaCosParams p, const Epi epi) {
    constexpr bool CE = XnaCosIsCE<Epi>::value, PK = XnaCosIsPeak<Epi>::value;
    constexpr int NW = XNA_HEAD_NW, NT = NW * 64;
    constexpr int TPW = CE ? xna_cos_ce_tpw(KS, NCT) : PK ? xna_cos_peak_tpw(KS, NCT) : xna_cos_tpw(KS, NCT);
    using G = XnaGeom<KS, 1>;
    constexpr int NSLOT = G::NSLOT, MT = G::MT, KST = G::KST, KROW = G::KROW;
    constexpr int DVT = NCT * 16, VROW = XnaVRow<DVT>::VROW, VCH = DVT / 8;
    constexpr int DVC = XNA_COS_DVC, WROW = XnaVRow<DVC>::VROW, WCH = DVC / 8;

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    bf16_t* Ks = reinterpret_cast<bf16_t*>(smem);
    bf16_t* Vs = Ks + NSLOT * KROW;     // the PV window
    bf16_t* Ws = Vs + NSLOT * VROW;     // a chunk of the value window

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
    const int nchunk = (p.dv + DVC - 1) / DVC;
    const bf16_t* q_cell = p.q + b * p.qs[0] + (int64_t)(cy * p.dy) * p.qs[2] + (int64_t)(cx * p.dx) * p.qs[3];
    float* o_cell = p.out + b * p.os[0] + (int64_t)(cy * p.dy) * p.os[1] + (int64_t)(cx * p.dx) * p.os[2];
    const bf16_t* kb = p.k + b * p.ks[0];
    const bf16_t* vb = p.pv + b * p.vs[0];
    const bf16_t* wb = p.v + b * p.ws[0];

    // key slots >= NSLOT are not stored: their reads are clamped to the last real row, their logits masked, P = 0
    auto ka_of = [&](int mt) __attribute__((always_inline)) {
        const int row = (mt * 16 + 15 < NSLOT) ? mt * 16 + col : min(mt * 16 + col, NSLOT - 1);
        return Ks + row * KROW + grp * 8;
    };
    auto va_row = [&](int blk) __attribute__((always_inline)) {
        const int r = blk * 16 + grp * 4 + (col >> 2);
        return (blk * 16 + 15 < NSLOT) ? r : min(r, NSLOT - 1);
    };
    // A-fragment (16 channels x 32 key slots) of a row-major [slots][ROW] window through the transposing LDS read
    auto a_frag = [&](const bf16_t* win, int ROW, int ks, int c0) __attribute__((always_inline)) {
        const bf16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((NAF_LDS bf16x4_t*)(win + va_row(ks * 2) * ROW + (col & 3) * 4 + c0));
        const bf16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((NAF_LDS bf16x4_t*)(win + va_row(ks * 2 + 1) * ROW + (col & 3) * 4 + c0));
        bf16x8_t a;
        a[0] = lo[0]; a[1] = lo[1]; a[2] = lo[2]; a[3] = lo[3];
        a[4] = hi[0]; a[5] = hi[1]; a[6] = hi[2]; a[7] = hi[3];
        return a;
    };

    // peak epilogue: the wave's running (value, flat index) per channel; lane (col < 4, grp) owns channels ct*16 + grp*4 + col
    u32x2_t* Pk = reinterpret_cast<u32x2_t*>(smem + xna_cos_lds_for(KS, NCT)) + wave * DVT;
    if constexpr (PK) {
        static_assert(xna_cos_lds_for(KS, NCT) % 8 == 0 && xna_cos_lds_for(KS, NCT) + xna_cos_peak_lds(NCT) <= 160 * 1024, "the peak pairs do not fit the LDS");
        if (col < 4) {
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) Pk[ct * 16 + grp * 4 + col] = u32x2_t{__float_as_uint(-INFINITY), 0x7fffffffu};
        }
    }

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
        float ssq[TPW];   // the lane's share of the pixel's squared norm: channels grp*4 + r of every 16-channel tile, all heads
#pragma unroll
        for (int u = 0; u < TPW; ++u) {
            ssq[u] = 0.f;
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) acc[u][ct] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        }

        for (int head = 0; head < p.heads; ++head) {
            // the head's queries are requested first: their latency hides under the window staging and the barrier
            bf16x8_t qf[TPW][2];
#pragma unroll
            for (int u = 0; u < TPW; ++u) {
                const bf16_t* qp = qpv[u] + head * p.qs[1];
                qf[u][0] = *reinterpret_cast<const bf16x8_t*>(qp);
                qf[u][1] = *reinterpret_cast<const bf16x8_t*>(qp + 32);
            }
            bf16x8_t pf[TPW][KST];   // P of the wave's tiles, packed once per head, used by the numerator and by every value chunk
            const bf16_t* wh = wb + head * p.ws[1];
            for (int chunk = 0; chunk < nchunk; ++chunk) {
                __syncthreads();   // every wave is done with the windows staged before
                if (chunk == 0) {
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
                const int c0 = chunk * DVC;
                const int wch_mem = min(p.dv - c0, DVC) >> 3;   // 16-byte chunks of this value chunk that exist (>= 2); the rest of the LDS row is zero
                {
                    // ---- stage value channels [c0, c0 + 64) of the window ----
                    constexpr int WTOT = NSLOT * WCH, WIT = (WTOT + NT - 1) / NT;
                    u32x4_t val[WIT];
#pragma unroll
                    for (int j = 0; j < WIT; ++j) {
                        const int i = min(j * NT + tid, WTOT - 1);
                        const int key = i / WCH, c = i - key * WCH;
                        const int ry = key / KS, rx = key - ry * KS;
                        const u32x4_t ld = *reinterpret_cast<const u32x4_t*>(wh + (int64_t)(y0 + ry) * p.ws[2] + (int64_t)(x0 + rx) * p.ws[3] + c0 + min(c, wch_mem - 1) * 8);
                        val[j] = c < wch_mem ? ld : u32x4_t{0u, 0u, 0u, 0u};
                    }
#pragma unroll
                    for (int j = 0; j < WIT; ++j) {
                        const int i = j * NT + tid;
                        const int key = i / WCH, c = i - key * WCH;
                        if ((WTOT % NT == 0) || i < WTOT) *reinterpret_cast<u32x4_t*>(Ws + key * WROW + c * 8) = val[j];
                    }
                }
                __syncthreads();

#pragma unroll
                for (int u = 0; u < TPW; ++u) {
                    if (!livev[u]) continue;   // wave-uniform
                    if (chunk == 0) {
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
#pragma unroll
                        for (int ks = 0; ks < KST; ++ks)
#pragma unroll
                            for (int j = 0; j < 8; ++j) pf[u][ks][j] = (bf16_t)(s[2 * ks + (j >> 2)][j & 3] * inv);
                        // ---- numerator: O^T += PV^T . P^T: lane (col, grp) owns channels ct*16 + grp*4 + r of query col ----
#pragma unroll
                        for (int ct = 0; ct < NCT; ++ct) {
#pragma unroll
                            for (int ks = 0; ks < KST; ++ks)
                                acc[u][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_frag(Vs, VROW, ks, ct * 16), pf[u][ks], acc[u][ct], 0, 0, 0);
                            // wide heads: keep the scheduler from hoisting every channel tile's PV^T fragments above the first MFMA (it spills)
                            if constexpr (NCT * KST >= 40) __builtin_amdgcn_sched_barrier(0);
                        }
                    }
                    // ---- denominator: F^T = V^T . P^T of this chunk's channel tiles, squared and dropped ----
#pragma unroll
                    for (int vt = 0; vt < DVC / 16; ++vt) {
                        if (vt * 2 >= wch_mem) continue;   // wave-uniform: the tile lies past Dv (dv is a multiple of 16)
                        f32x4_t f = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                        for (int ks = 0; ks < KST; ++ks) f = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_frag(Ws, WROW, ks, vt * 16), pf[u][ks], f, 0, 0, 0);
#pragma unroll
                        for (int r = 0; r < 4; ++r) ssq[u] = __builtin_fmaf(f[r], f[r], ssq[u]);
                    }
                }
            }
        }

        // ---- epilogue: the pixel's norm over all heads' channels, out = logit_scale * (acc / max(norm, 1e-12)) ----
        // its own arguments, fetched from the kernel-argument segment HERE: the empty asm makes the address opaque, so the scalar loads
        // cannot be hoisted above the head loop and held in registers across it; the same for the lane's coordinates
        const char __attribute__((address_space(4)))* ka = (const char __attribute__((address_space(4)))*)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(ka));
        int ecol = col, egrp = grp;
        asm volatile("" : "+v"(ecol), "+v"(egrp));
        const XnaCosEpilogue __attribute__((address_space(4)))* x = reinterpret_cast<const XnaCosEpilogue __attribute__((address_space(4)))*>(ka + XNA_COS_ARG_OFFSET);
        if constexpr (CE) {
            // ---- classification epilogue (see the header comment): softmax over the classes of the scaled cosines ----
#pragma clang fp contract(off)
            constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;
            const XnaCosCEEpilogue __attribute__((address_space(4)))* xc = reinterpret_cast<const XnaCosCEEpilogue __attribute__((address_space(4)))*>(ka + XNA_COS_ARG_OFFSET);
            const float* sp = xc->scale_ptr;
            const float ls = sp != nullptr ? *sp : x->logit_scale;
#pragma unroll
            for (int u = 0; u < TPW; ++u) {
                if (!livev[u]) continue;   // wave-uniform: the four-lane reductions below run on whole waves
                const float nrm = sqrtf(naf_rows_sum(ssq[u]));
                const float inv = 1.0f / fmaxf(nrm, 1e-12f);
                const bool inpx = tx0v[u] + ecol < p.dx;
                const int64_t gy = cy * p.dy + tyv[u];
                const int64_t gx = cx * p.dx + min(tx0v[u] + ecol, p.dx - 1);   // lanes past a partial last tile repeat its last pixel, store nothing
                // acc <- the unscaled cosine; z = ls * acc is the expression of the cosine epilogue, so a stored z is what naf_xna_cos_fwd stores
                float m = -INFINITY;
                int am = 0;
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int ch = ct * 16 + egrp * 4 + r;
                        if (ch < p.N) {
                            const float c = acc[u][ct][r] * inv;
                            acc[u][ct][r] = c;
                            const float z = ls * c;
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
                if (xc->target != nullptr) {
                    const int64_t tv = xc->target[b * xc->ts[0] + gy * xc->ts[1] + gx * xc->ts[2]];
                    t = (tv != xc->ignore_index && tv >= 0 && tv < (int64_t)p.N) ? (int)tv : -1;
                }
                // every pass forms z again from its own copy of the scale: sixteen channel tiles of z kept next to acc spill
                float ls2 = ls, ls3 = ls;
                asm volatile("" : "+v"(ls2), "+v"(ls3));
                float sum = 0.f, zt = 0.f;
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int ch = ct * 16 + egrp * 4 + r;
                        if (ch < p.N) {
                            const float z = ls2 * acc[u][ct][r];
                            sum += __builtin_amdgcn_exp2f((z - mall) * LOG2E);
                            zt += ch == t ? z : 0.f;   // one lane of the four holds z[t]
                        }
                    }
                sum = naf_rows_sum(sum);   // >= 1: the maximum contributes exp2(0)
                zt = naf_rows_sum(zt);
                if (egrp == 0 && inpx) {
                    if (xc->loss != nullptr)
                        xc->loss[b * xc->ls[0] + gy * xc->ls[1] + gx * xc->ls[2]] = t >= 0 ? (mall + __builtin_amdgcn_logf(sum) * LN2) - zt : 0.f;
                    if (xc->labels != nullptr) xc->labels[b * xc->bs[0] + gy * xc->bs[1] + gx * xc->bs[2]] = (uint8_t)label;
                    if (x->norms != nullptr) x->norms[b * x->ns[0] + gy * x->ns[1] + gx * x->ns[2]] = nrm;
                }
                if (p.out != nullptr && inpx) {
                    float* op = o_cell + (int64_t)tyv[u] * p.os[1] + (int64_t)(tx0v[u] + ecol) * p.os[2];
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int ch = ct * 16 + egrp * 4 + r;
                            if (ch < p.N) op[ch] = ls * acc[u][ct][r];
                        }
                }
                if (xc->dlogits != nullptr || xc->dscale != nullptr) {   // wave-uniform
                    bf16_t* gp = xc->dlogits != nullptr && inpx ? xc->dlogits + b * xc->gs[0] + gy * xc->gs[1] + gx * xc->gs[2] : nullptr;
                    const float rs = __builtin_amdgcn_rcpf(sum);
                    // the exponentials are formed again, not kept from the sum above (64 more registers at sixteen channel tiles: it spills)
                    float mg = mall;
                    asm volatile("" : "+v"(mg));
                    const bool counted = t >= 0;
                    const float gf = (counted && nrm > 0.f) ? ls * inv : 0.f;   // a zero feature: the exact gradient row is zero
                    float dsl = 0.f;
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct) {
                        const int c0 = ct * 16 + egrp * 4;
                        bf16x4_t gv;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int ch = c0 + r;
                            const float e = __builtin_amdgcn_exp2f((ls3 * acc[u][ct][r] - mg) * LOG2E) * rs - (ch == t ? 1.f : 0.f);
                            const bool on = ch < p.N && counted;
                            dsl += on ? e * acc[u][ct][r] : 0.f;
                            gv[r] = (bf16_t)((on && gf != 0.f) ? gf * e : 0.f);
                        }
                        // gc is a multiple of 8: a lane's four channels are all inside or all outside
                        if (gp != nullptr && c0 < xc->gc) *reinterpret_cast<bf16x4_t*>(gp + c0) = gv;
                    }
                    // channels past the accumulators (Npad = 160 -> gc = 192): plain zero stores
                    if (gp != nullptr)
                        for (int c0 = DVT + egrp * 4; c0 < xc->gc; c0 += 16) *reinterpret_cast<bf16x4_t*>(gp + c0) = bf16x4_t{(bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f};
                    dsl = naf_rows_sum(dsl);
                    if (xc->dscale != nullptr && egrp == 0 && inpx) xc->dscale[b * xc->ds[0] + gy * xc->ds[1] + gx * xc->ds[2]] = dsl;
                }
            }
        } else if constexpr (PK) {
            // ---- peak epilogue (see the header comment): the cell's maximum of every channel and its flat index ----
#pragma clang fp contract(off)
            const float ls = x->logit_scale;
#pragma unroll
            for (int u = 0; u < TPW; ++u) {
                if (!livev[u]) continue;   // wave-uniform: a tile past the cell takes no part; the lane reductions below run on whole waves
                const float nrm = sqrtf(naf_rows_sum(ssq[u]));
                const float inv = 1.0f / fmaxf(nrm, 1e-12f);
                const bool inpx = tx0v[u] + ecol < p.dx;   // lanes past a partial last tile hold the row's last pixel again, store nothing
                float* op = o_cell + (int64_t)tyv[u] * p.os[1] + (int64_t)min(tx0v[u] + ecol, p.dx - 1) * p.os[2];
                const bool st = p.out != nullptr && inpx;
                if (x->norms != nullptr && egrp == 0 && inpx)
                    x->norms[b * x->ns[0] + (int64_t)(cy * p.dy + tyv[u]) * x->ns[1] + (int64_t)(cx * p.dx + tx0v[u] + ecol) * x->ns[2]] = nrm;
                const int base = (cy * p.dy + tyv[u]) * p.Wo + cx * p.dx + tx0v[u];   // flat index of the tile's col 0 (host: Ho * Wo < 2^31)
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) {
                    if (ct * 16 >= p.N) continue;   // wave-uniform: channels that are never stored
                    float bv = 0.f;
                    int bi = 0;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float z = ls * (acc[u][ct][r] * inv);
                        if (st && ct * 16 + egrp * 4 + r < p.N) op[ct * 16 + egrp * 4 + r] = z;
                        const float m = naf_cols_max(z);
                        // the lowest col of the row that holds the maximum: a repeated last pixel ties only with itself, at a higher col
                        const uint32_t hit = (uint32_t)(__builtin_amdgcn_ballot_w64(z == m) >> (egrp * 16)) & 0xffffu;
                        if (ecol == r) {
                            bv = m;
                            bi = base + __builtin_ctz(hit | 0x10000u);
                        }
                    }
                    if (ecol < 4) {
                        u32x2_t* slot = Pk + ct * 16 + egrp * 4 + ecol;
                        const u32x2_t old = *slot;
                        const float ov = __uint_as_float(old[0]);
                        if (bv > ov || (bv == ov && bi < (int)old[1])) *slot = u32x2_t{__float_as_uint(bv), (uint32_t)bi};
                    }
                }
            }
        } else {
#pragma unroll
            for (int u = 0; u < TPW; ++u) {
                if (!livev[u]) continue;   // wave-uniform: the four-lane reduction below runs on whole waves
                const float nrm = sqrtf(naf_rows_sum(ssq[u]));
                const float inv = 1.0f / fmaxf(nrm, 1e-12f);
                if (tx0v[u] + ecol >= p.dx) continue;
                float* op = o_cell + (int64_t)tyv[u] * p.os[1] + (int64_t)(tx0v[u] + ecol) * p.os[2];
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int ch = ct * 16 + egrp * 4 + r;
                        if (ch < p.N) op[ch] = x->logit_scale * (acc[u][ct][r] * inv);
                    }
                }
                if (x->norms != nullptr && egrp == 0)
                    x->norms[b * x->ns[0] + (int64_t)(cy * p.dy + tyv[u]) * x->ns[1] + (int64_t)(cx * p.dx + tx0v[u] + ecol) * x->ns[2]] = nrm;
            }
        }
    }
    if constexpr (PK) {
        // ---- the eight waves' pairs of a channel, merged in wave order by the same comparator; one store per (cell, channel < N) ----
        __syncthreads();
        const char __attribute__((address_space(4)))* ka = (const char __attribute__((address_space(4)))*)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(ka));
        const XnaCosPeakEpilogue __attribute__((address_space(4)))* xp = reinterpret_cast<const XnaCosPeakEpilogue __attribute__((address_space(4)))*>(ka + XNA_COS_ARG_OFFSET);
        if (tid < DVT && tid < p.N) {
            const u32x2_t* all = reinterpret_cast<const u32x2_t*>(smem + xna_cos_lds_for(KS, NCT));
            float bv = __uint_as_float(all[tid][0]);
            int bi = (int)all[tid][1];
#pragma unroll
            for (int wv = 1; wv < NW; ++wv) {
                const u32x2_t o = all[wv * DVT + tid];
                const float ov = __uint_as_float(o[0]);
                if (ov > bv || (ov == bv && (int)o[1] < bi)) {
                    bv = ov;
                    bi = (int)o[1];
                }
            }
            xp->peak[b * xp->ps[0] + (int64_t)cy * xp->ps[1] + (int64_t)cx * xp->ps[2] + tid] = bv;
            xp->where[b * xp->is[0] + (int64_t)cy * xp->is[1] + (int64_t)cx * xp->is[2] + tid] = bi;
        }
    }
}

template <int KS, int NCT, typename Epi>
static int xna_cos_launch_one(const XnaCosParams& p, const Epi& epi, hipStream_t s) {
    constexpr bool CE = XnaCosIsCE<Epi>::value, PK = XnaCosIsPeak<Epi>::value;
    if constexpr (!(CE ? xna_cos_ce_served(KS, NCT) : PK ? xna_cos_peak_served(KS, NCT) : xna_cos_served(KS, NCT))) {
        naf_set_error("%s: no kernel for kernel_size=%d channel tiles=%d", CE ? "naf_xna_cos_ce_fwd" : PK ? "naf_xna_cos_peaks_fwd" : "naf_xna_cos_fwd", KS, NCT);
        return NAF_ERR_UNSUPPORTED;
    } else {
        constexpr size_t lds = xna_cos_lds_for(KS, NCT) + (PK ? xna_cos_peak_lds(NCT) : 0);
        auto kern = xna_cos_kernel<KS, NCT, Epi>;
        if (lds > 48 * 1024) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) {
                naf_set_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize=%zu): %s", lds, hipGetErrorString(e));
                return NAF_ERR_LAUNCH;
            }
        }
        hipLaunchKernelGGL(kern, dim3(p.nblocks), dim3(XNA_HEAD_NW * 64), lds, s, p, epi);
        return naf_check_launch(CE ? "xna_cos_kernel (classification epilogue)" : PK ? "xna_cos_kernel (peak epilogue)" : "xna_cos_kernel");
    }
}

// The window's entry point, one explicit instantiation per window in xna_cos_inst.hip.
template <int KS, typename Epi>
int xna_cos_launch_ks(const XnaCosParams& p, const Epi& epi, hipStream_t s) {
    const int nct = xna_head_nct(p.npad);
    if (nct == 2) return xna_cos_launch_one<KS, 2, Epi>(p, epi, s);
    if (nct == 4) return xna_cos_launch_one<KS, 4, Epi>(p, epi, s);
    if (nct == 10) return xna_cos_launch_one<KS, 10, Epi>(p, epi, s);
    if (nct == 16) return xna_cos_launch_one<KS, 16, Epi>(p, epi, s);
    naf_set_error("%s: no kernel for kernel_size=%d channel tiles=%d",
                  XnaCosIsCE<Epi>::value ? "naf_xna_cos_ce_fwd" : XnaCosIsPeak<Epi>::value ? "naf_xna_cos_peaks_fwd" : "naf_xna_cos_fwd", KS, nct);
    return NAF_ERR_UNSUPPORTED;
}

// xna_cos_inst.hip (-DNAF_KS=<KS>) defines the three, xna_cos.hip declares them (extern) and dispatches on the window.
#define NAF_XNA_COS_WINDOW(LINKAGE, KS)                                                                                    \
    LINKAGE template int xna_cos_launch_ks<KS>(const XnaCosParams&, const XnaCosEpilogue&, hipStream_t);                   \
    LINKAGE template int xna_cos_launch_ks<KS>(const XnaCosParams&, const XnaCosCEEpilogue&, hipStream_t);     \
    LINKAGE template int xna_cos_launch_ks<KS>(const XnaCosParams&, const XnaCosPeakEpilogue&, hipStream_t);
