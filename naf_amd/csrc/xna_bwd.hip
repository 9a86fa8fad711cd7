// Eligibility + dispatcher of the attention backward (mathematics: xna_bwd_params.h; the cell kernel: xna_bwd2_kernel.h).
#include "xna_bwd2_kernel.h"

// the instances: xna_bwd_inst.hip, one object per window (the plain backward and the one with a gradient of the scores)
#define NAF_X(K)                                                                             \
    extern template int xna_bwd2_launch_ks<K, false>(const XnaBwdParams&, int, hipStream_t); \
    extern template int xna_bwd2_launch_ks<K, true>(const XnaBwdScoresParams&, int, hipStream_t);
NAF_FOR_WINDOWS(NAF_X)
#undef NAF_X

// Value channels per launch.  A window whose K / V tiles, round buffers or accumulators do not fit at the full Dv is served in CHANNEL CHUNKS:
// the softmax depends on q and k only, dV splits by channel, and dQ / dK are sums over channels of V -- so the backward for a slice of V
// (and of dO) is a complete backward, and the slices' dQ / dK add up (XnaBwdParams::dq_accum; dK through the atomics).  The chunk is what the
// cell kernel takes at the window: 11 x 11 up to 128 channels (Dv 192 = 96 + 96, 256 = 128 + 128), 13 x 13 and 15 x 15 (BASELINE configs[2]'s
// largest window) up to 64 -- twelve / sixteen key tiles of S^T / dP^T leave its query waves no room for more, and at 15 x 15 the LDS is full
// (163.1 of 163.8 KB; profiles/r05_bwd_large_windows.txt).  0 = whole Dv.
static constexpr int bwd_chunk_limit(int ks) { return ks >= 13 ? 64 : ks >= 11 ? 128 : 0; }
static constexpr int bwd_next_chunk(int ks, int dv, int left) {
    const int lim = bwd_chunk_limit(ks);
    if (lim == 0 || dv <= lim) return left;
    const int n = (dv + lim - 1) / lim;                   // equal chunks where they are multiples of 32 (192 = 96 + 96: the 64-channel
    if (dv % n == 0 && (dv / n) % 32 == 0) return dv / n; // instantiation of the cell kernel at 11 x 11 carries 3 registers of scratch)
    return left < lim ? left : lim;
}

// Every chunk width the plan above emits, for every window and every Dv the backward takes, is a width the cell kernel is built for at that
// window (xna_bwd2_serves: registers and LDS) -- so eligibility below needs no LDS test and the launchers no fall-back.
template <int KS>
static constexpr bool bwd_chunk_served(int dvc) {
    return dvc == 32 ? xna_bwd2_serves<KS, 32>() : dvc == 64 ? xna_bwd2_serves<KS, 64>() : dvc == 96 ? xna_bwd2_serves<KS, 96>()
         : dvc == 128 ? xna_bwd2_serves<KS, 128>() : dvc == 192 ? xna_bwd2_serves<KS, 192>() : dvc == 256 ? xna_bwd2_serves<KS, 256>() : false;
}
template <int KS>
static constexpr bool bwd_plan_served() {
    for (const int dv : {32, 64, 96, 128, 192, 256})
        for (int c0 = 0; c0 < dv;) {
            const int dvc = bwd_next_chunk(KS, dv, dv - c0);
            if (dvc <= 0 || !bwd_chunk_served<KS>(dvc)) return false;
            c0 += dvc;
        }
    return true;
}
#define NAF_X(K) static_assert(bwd_plan_served<K>(), "the chunk plan emits a (window, channels per launch) combination xna_bwd2_kernel does not serve");
NAF_FOR_WINDOWS(NAF_X)
#undef NAF_X

// 1 when the cell kernel serves the request: the forward's MFMA conditions (square odd window 3..15, Dq = 64, integer
// ratio, h, w >= window) plus row tiles (Wo/w % 16 == 0; up to 9 x 9 also 14, 15, 28, 30 ...) and Dv in {32, 64, 96, 128, 192, 256}
// (all Dv up to k = 9 in one launch; wider heads at k = 11, 13 and 15 in channel chunks, above).
int naf_xna_bwd_eligible(const naf_xna_bwd_args* a) {
    if (!xna_cell_shape_ok(a)) return 0;
    // cell rows of whole 16-query tiles -- or (round 6) rows whose last tile is partial, where the forward takes them too (xna_row_tiles_ok: the
    // 14-pixel cells of patch-14 backbones, 15, 28, 30 ...): windows up to 9 x 9 (the reference's training windows), whole heads
    const int dx = a->Wo / a->w;
    if (dx % 16 != 0 && !(xna_row_tiles_ok(dx) && a->ky <= 9)) return 0;
    switch (a->Dv) {
        case 32: case 64: case 96: case 128: case 192: case 256: break;
        default: return 0;
    }
    if (!xna_qkv_layout_ok(a, a->v_lr, a->v_stride) || !naf_aligned(a->dout, 16) || !naf_aligned(a->dq, 16)) return 0;
    for (int i = 0; i < 4; ++i)
        if (a->dout_stride[i] % 8 || a->dq_stride[i] % 8) return 0;
    return 1;
}

// The launches naf_launch_xna_bwd issues for these arguments: chunk widths in launch order (include/naf_hip.h: naf_xna_bwd_chunk_plan)
int naf_xna_bwd_chunks(const naf_xna_bwd_args* a, int32_t* out, int cap) {
    if (!naf_xna_bwd_eligible(a)) return 0;
    int n = 0;
    for (int c0 = 0; c0 < a->Dv; ++n) {
        const int dvc = bwd_next_chunk(a->ky, a->Dv, a->Dv - c0);
        if (out != nullptr && n < cap) out[n] = dvc;
        c0 += dvc;
    }
    return n;
}

int naf_launch_xna_bwd(const naf_xna_bwd_args* a, float scale, hipStream_t s, const naf_xna_bwd_scores_args* sg) {
    if (!naf_xna_bwd_eligible(a)) {
        naf_set_error(
            "naf_xna_bwd: needs square odd kernel 3..15, Dq=64, integer ratio with row tiles (Wo/w %% 16 == 0, or 14 / 15 / 28 ... up to 9x9), h,w >= kernel, "
            "Dv in {32,64,96,128,192,256} and 16-byte aligned tensors (got k=%dx%d Dq=%d Dv=%d %dx%d -> %dx%d)",
            a->ky, a->kx, a->Dq, a->Dv, a->h, a->w, a->Ho, a->Wo);
        return NAF_ERR_UNSUPPORTED;
    }
    XnaBwdParams p;
    xna_fill_common(p, a, a->v_stride, scale);
    p.dq = static_cast<bf16_t*>(a->dq);
    p.dk = a->dk_lr;
    p.dy = a->Ho / a->h; p.dx = a->Wo / a->w;
    if (const int rc = xna_grid("naf_xna_bwd", (int64_t)a->B * a->h * a->w * a->heads, &p.nblocks)) return rc;
    p.seg_len = 1; p.nseg = a->w;
    p.scale = scale;
    for (int i = 0; i < 4; ++i) {
        p.gs[i] = a->dout_stride[i]; p.dqs[i] = a->dq_stride[i];
    }
    p.dv_pitch = a->Dv;
    p.dq_accum = 0;
    // a gradient of the scores (naf_xna_bwd_scores) enters dQ / dK once: in the first chunk, which runs the SG instantiation
    const bool scores = sg != nullptr && sg->dlogits != nullptr;
    XnaBwdScoresParams ps;
    // channel chunks (one launch where the whole Dv fits): v, dout and dv move to the chunk's first channel of every head
    for (int c0 = 0; c0 < a->Dv;) {
        const int dvc = bwd_next_chunk(a->ky, a->Dv, a->Dv - c0);
        p.v = static_cast<const bf16_t*>(a->v_lr) + c0;
        p.dout = static_cast<const bf16_t*>(a->dout) + c0;
        p.dv = a->dv_lr + c0;
        p.dq_accum = c0 > 0;
        int rc = NAF_ERR_UNSUPPORTED;
        if (scores && c0 == 0) {
            static_cast<XnaBwdParams&>(ps) = p;
            ps.dl = sg->dlogits;
            for (int i = 0; i < 4; ++i) ps.dls[i] = sg->dlogits_stride[i];
            switch (a->ky) {
#define NAF_X(K) case K: rc = xna_bwd2_launch_ks<K, true>(ps, dvc, s); break;
                NAF_FOR_WINDOWS(NAF_X)
#undef NAF_X
            }
        } else {
            switch (a->ky) {
#define NAF_X(K) case K: rc = xna_bwd2_launch_ks<K, false>(p, dvc, s); break;
                NAF_FOR_WINDOWS(NAF_X)
#undef NAF_X
            }
        }
        if (rc != NAF_OK) return rc;
        c0 += dvc;
    }
    return NAF_OK;
}
