// Eligibility test + dispatcher for the head-summed MFMA cell kernel (see xna_head_kernel.h).
#include "xna_head_kernel.h"

#define NAF_DECL(K) int naf_xna_head_launch_k##K(const XnaHeadParams& p, int out_dtype, hipStream_t s);
NAF_DECL(3) NAF_DECL(5) NAF_DECL(7) NAF_DECL(9) NAF_DECL(11) NAF_DECL(13) NAF_DECL(15)
#undef NAF_DECL
#define NAF_DECL(K) int naf_xna_head_ce_launch_k##K(const XnaHeadParams& p, const XnaHeadCEExtra& x, hipStream_t s);
NAF_DECL(3) NAF_DECL(5) NAF_DECL(7) NAF_DECL(9) NAF_DECL(11) NAF_DECL(13) NAF_DECL(15)
#undef NAF_DECL
#define NAF_DECL(K) int naf_xna_head_cm_launch_k##K(const XnaHeadParams& p, const XnaHeadCMExtra& x, hipStream_t s);
NAF_DECL(3) NAF_DECL(5) NAF_DECL(7) NAF_DECL(9) NAF_DECL(11) NAF_DECL(13) NAF_DECL(15)
#undef NAF_DECL

static bool head_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) % 16) == 0; }

// NAF_OK when the kernel serves the (validated) request; otherwise NAF_ERR_UNSUPPORTED with the reason in the error string.
int naf_xna_head_eligible(const naf_xna_head_args* a) {
    const int ks = a->ky;
    if (a->ky != a->kx || ks < 3 || ks > 15) {
        naf_set_error("naf_xna_head: the fused kernel needs a square window 3 .. 15 (got %dx%d)", a->ky, a->kx);
        return NAF_ERR_UNSUPPORTED;
    }
    if (a->Dq != 64) {
        naf_set_error("naf_xna_head: the fused kernel needs Dq = 64 (got %d)", a->Dq);
        return NAF_ERR_UNSUPPORTED;
    }
    if (a->h < ks || a->w < ks) {
        naf_set_error("naf_xna_head: the fused kernel needs h, w >= window (got %dx%d, window %d)", a->h, a->w, ks);
        return NAF_ERR_UNSUPPORTED;
    }
    if (a->Ho % a->h != 0 || a->Wo % a->w != 0) {
        naf_set_error("naf_xna_head: the fused kernel needs an integer ratio (got %dx%d -> %dx%d)", a->h, a->w, a->Ho, a->Wo);
        return NAF_ERR_UNSUPPORTED;
    }
    const int dy = a->Ho / a->h, dx = a->Wo / a->w;
    if (!xna_row_tiles_ok(dx) || (int64_t)dy * ((dx + 15) / 16) > 1024) {
        naf_set_error("naf_xna_head: the fused kernel needs row tiles (Wo/w a multiple of 16, or 14, 15, 28, 30 ...; at most 1024 tiles per cell; got %dx%d -> %dx%d)",
                      a->h, a->w, a->Ho, a->Wo);
        return NAF_ERR_UNSUPPORTED;
    }
    if (!head_aligned(a->q) || !head_aligned(a->k_lr) || !head_aligned(a->pv_lr)) {
        naf_set_error("naf_xna_head: the fused kernel needs 16-byte aligned q, k_lr, pv_lr");
        return NAF_ERR_UNSUPPORTED;
    }
    for (int i = 0; i < 4; ++i) {
        if (a->q_stride[i] % 8 || a->k_stride[i] % 8 || a->pv_stride[i] % 8) {
            naf_set_error("naf_xna_head: the fused kernel needs q / k_lr / pv_lr strides that are multiples of 8 elements");
            return NAF_ERR_UNSUPPORTED;
        }
    }
    return NAF_OK;
}

// What the classification epilogue asks beyond naf_xna_head_eligible (the request is validated: naf_api.hip).
int naf_xna_head_ce_eligible(const naf_xna_head_ce_args* c) {
    const int rc = naf_xna_head_eligible(&c->head);
    if (rc != NAF_OK) return rc;
    if (c->dlogits != nullptr) {
        if (!head_aligned(c->dlogits)) {
            naf_set_error("naf_xna_head_ce: the fused kernel needs a 16-byte aligned dlogits");
            return NAF_ERR_UNSUPPORTED;
        }
        for (int i = 0; i < 3; ++i) {
            if (c->dlogits_stride[i] % 8) {
                naf_set_error("naf_xna_head_ce: the fused kernel needs dlogits strides that are multiples of 8 elements");
                return NAF_ERR_UNSUPPORTED;
            }
        }
    }
    return NAF_OK;
}

static int head_fill_params(const naf_xna_head_args* a, float scale, const char* who, XnaHeadParams& p) {
    p.q = static_cast<const bf16_t*>(a->q);
    p.k = static_cast<const bf16_t*>(a->k_lr);
    p.pv = static_cast<const bf16_t*>(a->pv_lr);
    p.bias = a->bias;
    p.out = a->out;
    p.tab_y = a->rope_tab_y; p.tab_x = a->rope_tab_x;
    p.B = a->B; p.heads = a->heads; p.Ho = a->Ho; p.Wo = a->Wo; p.h = a->h; p.w = a->w;
    p.dy = a->Ho / a->h; p.dx = a->Wo / a->w;
    p.N = a->N;
    p.npad = (a->N + 15) & ~15;
    const int64_t nb = (int64_t)a->B * a->h * a->w;
    if (nb <= 0 || nb > 0x7fffffffLL) {
        naf_set_error("%s: grid of %lld workgroups out of range", who, (long long)nb);
        return NAF_ERR_INVALID;
    }
    p.nblocks = (uint32_t)nb;
    p.scale_log2e = scale * 1.4426950408889634f;
    for (int i = 0; i < 4; ++i) {
        p.qs[i] = a->q_stride[i]; p.ks[i] = a->k_stride[i]; p.vs[i] = a->pv_stride[i];
    }
    for (int i = 0; i < 3; ++i) p.os[i] = a->o_stride[i];
    return NAF_OK;
}

int naf_launch_xna_head(const naf_xna_head_args* a, float scale, hipStream_t s) {
    XnaHeadParams p;
    const int rc = head_fill_params(a, scale, "naf_xna_head_fwd", p);
    if (rc != NAF_OK) return rc;
    switch (a->ky) {
        case 3: return naf_xna_head_launch_k3(p, a->out_dtype, s);
        case 5: return naf_xna_head_launch_k5(p, a->out_dtype, s);
        case 7: return naf_xna_head_launch_k7(p, a->out_dtype, s);
        case 9: return naf_xna_head_launch_k9(p, a->out_dtype, s);
        case 11: return naf_xna_head_launch_k11(p, a->out_dtype, s);
        case 13: return naf_xna_head_launch_k13(p, a->out_dtype, s);
        case 15: return naf_xna_head_launch_k15(p, a->out_dtype, s);
    }
    naf_set_error("naf_xna_head_fwd: kernel size %d has no instantiation", a->ky);
    return NAF_ERR_UNSUPPORTED;
}

static void head_fill_ce(const naf_xna_head_ce_args* c, XnaHeadCEExtra& x) {
    x.target = c->target;
    x.loss = c->loss;
    x.labels = c->labels;
    x.dlogits = static_cast<bf16_t*>(c->dlogits);
    x.ignore_index = c->ignore_index;
    x.gc = c->dlogits != nullptr ? c->dlogits_channels : 0;
    for (int i = 0; i < 3; ++i) {
        x.ts[i] = c->t_stride[i]; x.ls[i] = c->loss_stride[i]; x.bs[i] = c->labels_stride[i]; x.gs[i] = c->dlogits_stride[i];
    }
}

int naf_launch_xna_head_ce(const naf_xna_head_ce_args* c, float scale, hipStream_t s) {
    XnaHeadParams p;
    const int rc = head_fill_params(&c->head, scale, "naf_xna_head_ce_fwd", p);
    if (rc != NAF_OK) return rc;
    XnaHeadCEExtra x;
    head_fill_ce(c, x);
    switch (c->head.ky) {
        case 3: return naf_xna_head_ce_launch_k3(p, x, s);
        case 5: return naf_xna_head_ce_launch_k5(p, x, s);
        case 7: return naf_xna_head_ce_launch_k7(p, x, s);
        case 9: return naf_xna_head_ce_launch_k9(p, x, s);
        case 11: return naf_xna_head_ce_launch_k11(p, x, s);
        case 13: return naf_xna_head_ce_launch_k13(p, x, s);
        case 15: return naf_xna_head_ce_launch_k15(p, x, s);
    }
    naf_set_error("naf_xna_head_ce_fwd: kernel size %d has no instantiation", c->head.ky);
    return NAF_ERR_UNSUPPORTED;
}

int naf_launch_xna_head_cm(const naf_xna_head_cm_args* m, float scale, hipStream_t s) {
    const naf_xna_head_ce_args* c = &m->ce;
    XnaHeadParams p;
    const int rc = head_fill_params(&c->head, scale, "naf_xna_head_cm_fwd", p);
    if (rc != NAF_OK) return rc;
    XnaHeadCMExtra x;
    head_fill_ce(c, x.ce);
    x.confusion = reinterpret_cast<unsigned long long*>(m->confusion);   // counts are non-negative: the 64-bit add is the same for both
    x.cm_stride = m->cm_stride;
    switch (c->head.ky) {
        case 3: return naf_xna_head_cm_launch_k3(p, x, s);
        case 5: return naf_xna_head_cm_launch_k5(p, x, s);
        case 7: return naf_xna_head_cm_launch_k7(p, x, s);
        case 9: return naf_xna_head_cm_launch_k9(p, x, s);
        case 11: return naf_xna_head_cm_launch_k11(p, x, s);
        case 13: return naf_xna_head_cm_launch_k13(p, x, s);
        case 15: return naf_xna_head_cm_launch_k15(p, x, s);
    }
    naf_set_error("naf_xna_head_cm_fwd: kernel size %d has no instantiation", c->head.ky);
    return NAF_ERR_UNSUPPORTED;
}
