// Eligibility test + dispatcher for the cosine-head MFMA cell kernel (see xna_cos_kernel.h).
#include "xna_cos_kernel.h"

// the instances: xna_cos_inst.hip, one object per window
#define NAF_X(K) NAF_XNA_COS_WINDOW(extern, K)
NAF_FOR_WINDOWS(NAF_X)
#undef NAF_X

// NAF_OK when the kernel serves the (validated) request; otherwise NAF_ERR_UNSUPPORTED with the reason in the error string.  The geometry
// and layout rules are the head family's (naf_common.h): what naf_xna_head_select grants, this kernel is asked to serve.
int naf_xna_cos_eligible(const naf_xna_cos_args* a) {
    const int rc = xna_headsum_shape_eligible("naf_xna_cos", a);
    if (rc != NAF_OK) return rc;
    if (a->Dv % 16 != 0) {
        naf_set_error("naf_xna_cos: the fused kernel needs Dv a multiple of 16 (got %d)", a->Dv);
        return NAF_ERR_UNSUPPORTED;
    }
    if (!xna_cos_served(a->ky, xna_head_nct((a->N + 15) & ~15))) {
        naf_set_error("naf_xna_cos: no fused kernel for window %d with N = %d (registers / LDS: the instantiation would spill)", a->ky, a->N);
        return NAF_ERR_UNSUPPORTED;
    }
    if (!xna_qkv_layout_ok(a, a->pv_lr, a->pv_stride) || !naf_aligned(a->v_lr, 16) ||
        a->v_stride[0] % 8 || a->v_stride[1] % 8 || a->v_stride[2] % 8 || a->v_stride[3] % 8) {
        if (!naf_aligned(a->q, 16) || !naf_aligned(a->k_lr, 16) || !naf_aligned(a->pv_lr, 16) || !naf_aligned(a->v_lr, 16))
            naf_set_error("naf_xna_cos: the fused kernel needs 16-byte aligned q, k_lr, pv_lr, v_lr");
        else naf_set_error("naf_xna_cos: the fused kernel needs q / k_lr / pv_lr / v_lr strides that are multiples of 8 elements");
        return NAF_ERR_UNSUPPORTED;
    }
    return NAF_OK;
}

// What the classification epilogue asks beyond naf_xna_cos_eligible (the request is validated: naf_api.hip).
int naf_xna_cos_ce_eligible(const naf_xna_cos_ce_args* c) {
    const int rc = naf_xna_cos_eligible(&c->cos);
    if (rc != NAF_OK) return rc;
    if (!xna_cos_ce_served(c->cos.ky, xna_head_nct((c->cos.N + 15) & ~15))) {
        naf_set_error("naf_xna_cos_ce: no fused kernel for window %d with N = %d (registers: the instantiation would spill)", c->cos.ky, c->cos.N);
        return NAF_ERR_UNSUPPORTED;
    }
    if (c->dlogits != nullptr) {
        if (!naf_aligned(c->dlogits, 16)) {
            naf_set_error("naf_xna_cos_ce: the fused kernel needs a 16-byte aligned dlogits");
            return NAF_ERR_UNSUPPORTED;
        }
        for (int i = 0; i < 3; ++i) {
            if (c->dlogits_stride[i] % 8) {
                naf_set_error("naf_xna_cos_ce: the fused kernel needs dlogits strides that are multiples of 8 elements");
                return NAF_ERR_UNSUPPORTED;
            }
        }
    }
    return NAF_OK;
}

// What the peak epilogue asks beyond naf_xna_cos_eligible (the request is validated: naf_api.hip).
int naf_xna_cos_peaks_eligible(const naf_xna_cos_peaks_args* c) {
    const int rc = naf_xna_cos_eligible(&c->cos);
    if (rc != NAF_OK) return rc;
    if (!xna_cos_peak_served(c->cos.ky, xna_head_nct((c->cos.N + 15) & ~15))) {
        naf_set_error("naf_xna_cos_peaks: no fused kernel for window %d with N = %d (registers: the instantiation would spill)", c->cos.ky, c->cos.N);
        return NAF_ERR_UNSUPPORTED;
    }
    return NAF_OK;
}

// `who` names the entry in the messages.
static int cos_fill(const naf_xna_cos_args* a, float scale, const char* who, XnaCosParams& p, XnaCosEpilogue& e) {
    const int rc = xna_headsum_fill(p, a, scale, who);
    if (rc != NAF_OK) return rc;
    p.v = static_cast<const bf16_t*>(a->v_lr);
    p.dv = a->Dv;
    for (int i = 0; i < 4; ++i) p.ws[i] = a->v_stride[i];
    e.norms = a->norms;
    for (int i = 0; i < 3; ++i) e.ns[i] = a->norms != nullptr ? a->norms_stride[i] : 0;
    e.logit_scale = a->logit_scale;
    return NAF_OK;
}

int naf_launch_xna_cos(const naf_xna_cos_args* a, float scale, hipStream_t s) {
    XnaCosParams p;
    XnaCosEpilogue e;
    const int rc = cos_fill(a, scale, "naf_xna_cos_fwd", p, e);
    if (rc != NAF_OK) return rc;
    switch (a->ky) {
#define NAF_X(K) case K: return xna_cos_launch_ks<K>(p, e, s);
        NAF_FOR_WINDOWS(NAF_X)
#undef NAF_X
    }
    naf_set_error("naf_xna_cos_fwd: kernel size %d has no instantiation", a->ky);
    return NAF_ERR_UNSUPPORTED;
}

int naf_launch_xna_cos_ce(const naf_xna_cos_ce_args* c, float scale, hipStream_t s) {
    XnaCosParams p;
    XnaCosCEEpilogue x;
    const int rc = cos_fill(&c->cos, scale, "naf_xna_cos_ce_fwd", p, x.cos);
    if (rc != NAF_OK) return rc;
    x.target = c->target;
    x.loss = c->loss;
    x.labels = c->labels;
    x.dlogits = static_cast<bf16_t*>(c->dlogits);
    x.dscale = c->dscale;
    x.scale_ptr = c->logit_scale_ptr;
    x.ignore_index = c->ignore_index;
    x.gc = c->dlogits != nullptr ? c->dlogits_channels : 0;
    for (int i = 0; i < 3; ++i) {
        x.ts[i] = c->t_stride[i]; x.ls[i] = c->loss_stride[i]; x.bs[i] = c->labels_stride[i]; x.gs[i] = c->dlogits_stride[i]; x.ds[i] = c->dscale_stride[i];
    }
    switch (c->cos.ky) {
#define NAF_X(K) case K: return xna_cos_launch_ks<K>(p, x, s);
        NAF_FOR_WINDOWS(NAF_X)
#undef NAF_X
    }
    naf_set_error("naf_xna_cos_ce_fwd: kernel size %d has no instantiation", c->cos.ky);
    return NAF_ERR_UNSUPPORTED;
}

int naf_launch_xna_cos_peaks(const naf_xna_cos_peaks_args* c, float scale, hipStream_t s) {
    XnaCosParams p;
    XnaCosPeakEpilogue x;
    const int rc = cos_fill(&c->cos, scale, "naf_xna_cos_peaks_fwd", p, x.cos);
    if (rc != NAF_OK) return rc;
    x.peak = c->peak;
    x.where = c->where;
    for (int i = 0; i < 3; ++i) {
        x.ps[i] = c->peak_stride[i]; x.is[i] = c->where_stride[i];
    }
    switch (c->cos.ky) {
#define NAF_X(K) case K: return xna_cos_launch_ks<K>(p, x, s);
        NAF_FOR_WINDOWS(NAF_X)
#undef NAF_X
    }
    naf_set_error("naf_xna_cos_peaks_fwd: kernel size %d has no instantiation", c->cos.ky);
    return NAF_ERR_UNSUPPORTED;
}
