// Eligibility test + dispatcher for the head-summed MFMA cell kernel (see xna_head_kernel.h).
#include <stdio.h>

#include "xna_head_kernel.h"

// the instances: xna_head_inst.hip, one object per window
#define NAF_X(K) NAF_XNA_HEAD_WINDOW(extern, K)
NAF_FOR_WINDOWS(NAF_X)
#undef NAF_X

// NAF_OK when the kernel serves the (validated) request; otherwise NAF_ERR_UNSUPPORTED with the reason in the error string.
int naf_xna_head_eligible(const naf_xna_head_args* a) {
    const int rc = xna_headsum_shape_eligible("naf_xna_head", a);
    if (rc != NAF_OK) return rc;
    if (!xna_qkv_layout_ok(a, a->pv_lr, a->pv_stride)) {   // which half of it
        if (!naf_aligned(a->q, 16) || !naf_aligned(a->k_lr, 16) || !naf_aligned(a->pv_lr, 16)) naf_set_error("naf_xna_head: the fused kernel needs 16-byte aligned q, k_lr, pv_lr");
        else naf_set_error("naf_xna_head: the fused kernel needs q / k_lr / pv_lr strides that are multiples of 8 elements");
        return NAF_ERR_UNSUPPORTED;
    }
    return NAF_OK;
}

// What the classification epilogue asks beyond naf_xna_head_eligible (the request is validated: naf_api.hip).
int naf_xna_head_ce_eligible(const naf_xna_head_ce_args* c) {
    const int rc = naf_xna_head_eligible(&c->head);
    if (rc != NAF_OK) return rc;
    if (c->dlogits != nullptr) {
        if (!naf_aligned(c->dlogits, 16)) {
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

// `tag` names the variant in the messages: the C entry point is naf_<tag>_fwd.
static int head_fill_params(const naf_xna_head_args* a, float scale, const char* tag, XnaHeadParams& p) {
    p.bias = a->bias;
    char who[32];
    snprintf(who, sizeof(who), "naf_%s_fwd", tag);
    return xna_headsum_fill(p, a, scale, who);
}

// Fills the parameters and dispatches on the window; `what` names the launch in a launch error, `x` is the variant's extra kernel argument.
template <typename... Extra>
static int head_launch(const naf_xna_head_args* a, float scale, hipStream_t s, const char* tag, const char* what, const Extra&... x) {
    XnaHeadParams p;
    const int rc = head_fill_params(a, scale, tag, p);
    if (rc != NAF_OK) return rc;
    switch (a->ky) {
#define NAF_X(K) case K: return xna_head_launch_ks<K>(p, a->out_dtype, s, tag, what, x...);
        NAF_FOR_WINDOWS(NAF_X)
#undef NAF_X
    }
    naf_set_error("naf_%s_fwd: kernel size %d has no instantiation", tag, a->ky);
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

int naf_launch_xna_head(const naf_xna_head_args* a, float scale, hipStream_t s) { return head_launch(a, scale, s, "xna_head", "xna_head_kernel"); }

int naf_launch_xna_head_ce(const naf_xna_head_ce_args* c, float scale, hipStream_t s) {
    XnaHeadCEExtra x;
    head_fill_ce(c, x);
    return head_launch(&c->head, scale, s, "xna_head_ce", "xna_head_kernel (classification epilogue)", x);
}

int naf_launch_xna_head_cm(const naf_xna_head_cm_args* m, float scale, hipStream_t s) {
    XnaHeadCMExtra x;
    head_fill_ce(&m->ce, x.ce);
    x.confusion = reinterpret_cast<unsigned long long*>(m->confusion);   // counts are non-negative: the 64-bit add is the same for both
    x.cm_stride = m->cm_stride;
    return head_launch(&m->ce.head, scale, s, "xna_head_cm", "xna_head_kernel (confusion matrix)", x);
}
