// Eligibility test + dispatcher for the MFMA cell kernel (see xna_mfma_kernel.h).
#include <stdlib.h>

#include "xna_slide_kernel.h"

// the instances: xna_mfma_inst.hip / xna_slide_inst.hip, one object per (window, value type)
#define NAF_X(K)                                                                                                   \
    extern template int xna_mfma_launch_ks<K, false>(const XnaMfmaParams&, const XnaMfmaPlan&, int, hipStream_t);  \
    extern template int xna_mfma_launch_ks<K, true>(const XnaMfmaParams&, const XnaMfmaPlan&, int, hipStream_t);
NAF_FOR_WINDOWS(NAF_X)
#undef NAF_X
#define NAF_X(K)                                                                                  \
    extern template int xna_slide_launch_ks<K, false>(const XnaSlideParams&, int, int, hipStream_t); \
    extern template int xna_slide_launch_ks<K, true>(const XnaSlideParams&, int, int, hipStream_t);
NAF_FOR_SLIDE_WINDOWS(NAF_X)
#undef NAF_X

// Returns 1 when the MFMA cell kernel can serve the request (and the Dv tile / LDS bytes it would
// use), 0 otherwise.  Never sets the error string: ineligibility is not an error.
int naf_xna_mfma_eligible(const naf_xna_args* a, int* dvt_out, size_t* lds_out) {
    if (!xna_cell_shape_ok(a) || a->Dv % 16 != 0) return 0;
    if (!xna_qkv_layout_ok(a, a->v_lr, a->v_stride) || !naf_aligned(a->out, 16)) return 0;
    for (int i = 0; i < 4; ++i)
        if (a->o_stride[i] % 4) return 0;
    XnaMfmaPlan pl;
    if (!xna_mfma_plan(a->ky, a->Dv, a->out_dtype, &pl)) return 0;
    if (dvt_out) *dvt_out = pl.dvt;
    if (lds_out) *lds_out = pl.lds;
    return 1;
}

// Rotate-on-load (rope_tab_*) is implemented by the kernel's row-tile path: a 16-query tile is (up to) 16 consecutive
// pixels of one cell row (xna_row_tiles_ok(dx), <= 1024 tiles per cell).
int naf_xna_mfma_rope_ok(const naf_xna_args* a) {
    const int dy = a->Ho / a->h, dx = a->Wo / a->w;
    if (!xna_row_tiles_ok(dx) || (int64_t)dy * ((dx + 15) / 16) > 1024) return 0;
    return naf_xna_mfma_eligible(a, nullptr, nullptr);
}

int naf_launch_xna_mfma(const naf_xna_args* a, float scale, hipStream_t s) {
    int dvt = 0;
    size_t lds = 0;
    if (!naf_xna_mfma_eligible(a, &dvt, &lds)) {
        naf_set_error(
            "naf_xna_fwd: MFMA path needs square odd kernel 3..15, Dq=64, integer ratio, h,w >= kernel, Dv %% 16 == 0, "
            "16-byte aligned tensors (got k=%dx%d Dq=%d Dv=%d %dx%d -> %dx%d)",
            a->ky, a->kx, a->Dq, a->Dv, a->h, a->w, a->Ho, a->Wo);
        return NAF_ERR_UNSUPPORTED;
    }
    XnaMfmaParams p;
    xna_fill_common(p, a, a->v_stride, scale);
    p.v = static_cast<const bf16_t*>(a->v_lr);
    p.out = a->out;
    p.logits = a->logits;
    p.dy = a->Ho / a->h; p.dx = a->Wo / a->w;
    p.tab_y = a->rope_tab_y; p.tab_x = a->rope_tab_x;
    if (a->rope_tab_y != nullptr && !naf_xna_mfma_rope_ok(a)) {
        naf_set_error("naf_xna_fwd: rotate-on-load needs row tiles (Wo/w a multiple of 16, or 14, 15, 28 ...: got %dx%d -> %dx%d)", a->h, a->w, a->Ho, a->Wo);
        return NAF_ERR_UNSUPPORTED;
    }
    XnaMfmaPlan pl;
    xna_mfma_plan(a->ky, a->Dv, a->out_dtype, &pl);
    p.nchunk = a->Dv / pl.dvt;
    const int bh = (a->h + pl.cb - 1) / pl.cb, bw = (a->w + pl.cb - 1) / pl.cb;
    const int64_t nb = (int64_t)a->B * bh * bw * a->heads * p.nchunk;
    if (const int rc = xna_grid("naf_xna_fwd", nb, &p.nblocks)) return rc;
    // dispatch order in groups of 16 workgroups per XCD turn (xna_block_order; profiles/r02_hbm_ceiling.txt: all XCDs
    // sweep the same cell rows, +5..9 % over one band of cell rows per XCD); NAF_XNA_ORDER=0 restores the bands (A/B knob)
    static const int order = [] { const char* e = naf_knob("NAF_XNA_ORDER"); return e ? atoi(e) : 16; }();
    p.order = order;
    static const int rope_lds = [] { const char* e = naf_knob("NAF_XNA_ROPE_LDS"); return e ? atoi(e) : 1; }();   // A/B knob
    p.rope_lds = rope_lds;
    p.scale = scale;
    for (int i = 0; i < 4; ++i) p.os[i] = a->o_stride[i];
    // Whenever the plan has no staged stores (windows of 11x11 and up, fp32 output, windows + staging tiles that would
    // leave fewer than 3 workgroups per CU) and the geometry has row tiles: persistent sliding-window kernel
    // (xna_slide_kernel.h).  return_weights needs the window's row-major slot order and stays on the cell kernel.
    const bool half = a->out_dtype == NAF_F16;   // half values and output: the HALF instances
    static const bool no_slide = [] { const char* e = naf_knob("NAF_XNA_SLIDE"); return e && atoi(e) == 0; }();   // A/B knob
    if (a->ky >= 7 && !pl.staged && !no_slide && a->logits == nullptr && (p.dx % 16) == 0 && (int64_t)p.dy * p.dx / 16 <= 1024) {
        XnaSlideParams sp;
        sp.m = p;
        const int dvt_u = [&] {   // Dv tile of the unstaged plan: the largest divisor of Dv whose window fits the LDS
            static const int cand[] = {256, 192, 128, 96, 64, 48, 32, 16};
            static const int cap = [] { const char* e = naf_knob("NAF_XNA_SLIDE_DVT"); return e ? atoi(e) : 1 << 30; }();   // A/B knob
            for (int c : cand)
                if (c <= cap && a->Dv % c == 0 && xna_mfma_lds_for(a->ky, 1, c, false) <= 160 * 1024) return c;
            return 0;
        }();
        sp.m.nchunk = a->Dv / dvt_u;
        const int64_t rows = (int64_t)a->B * a->h * a->heads * sp.m.nchunk;
        int64_t nseg = (naf_cu_count() + rows - 1) / rows;             // enough workgroups for every CU ...
        const int64_t max_seg = (a->w + 3) / 4;                          // ... but segments of at least 4 cells
        if (nseg > max_seg) nseg = max_seg;
        if (nseg < 1) nseg = 1;
        sp.seg_len = (int32_t)((a->w + nseg - 1) / nseg);
        sp.nseg = (int32_t)((a->w + sp.seg_len - 1) / sp.seg_len);
        const int64_t nbs = rows * sp.nseg;
        if (const int rc = xna_grid("naf_xna_fwd", nbs, &sp.m.nblocks)) return rc;
        // (A tail hand-over -- finished workgroups claiming the last cells of other segments -- was built, bit-identical and 2-6 % slower at
        // G2-k11: profiles/r06_other_workloads.txt.  The split of a cell row into segments is static.)
        switch (a->ky) {
#define NAF_X(K) case K: return half ? xna_slide_launch_ks<K, true>(sp, dvt_u, a->out_dtype, s) : xna_slide_launch_ks<K, false>(sp, dvt_u, a->out_dtype, s);
            NAF_FOR_SLIDE_WINDOWS(NAF_X)
#undef NAF_X
        }
    }
    switch (a->ky) {
#define NAF_X(K) case K: return half ? xna_mfma_launch_ks<K, true>(p, pl, a->out_dtype, s) : xna_mfma_launch_ks<K, false>(p, pl, a->out_dtype, s);
        NAF_FOR_WINDOWS(NAF_X)
#undef NAF_X
    }
    naf_set_error("naf_xna_fwd: kernel size %d has no MFMA instantiation", a->ky);
    return NAF_ERR_UNSUPPORTED;
}
