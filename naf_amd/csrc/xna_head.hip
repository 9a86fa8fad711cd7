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

// What the regression epilogue asks beyond naf_xna_head_eligible (the request is validated: naf_api.hip).
int naf_xna_head_reg_eligible(const naf_xna_head_reg_args* c) {
    if (c->head.N > 32) {
        naf_set_error("naf_xna_head_reg: the fused kernel serves N <= 32 outputs (got %d)", c->head.N);
        return NAF_ERR_UNSUPPORTED;
    }
    const int rc = naf_xna_head_eligible(&c->head);
    if (rc != NAF_OK) return rc;
    if (c->dlogits != nullptr) {
        const int gc = c->dlogits_channels;
        if (gc != 32 && gc != 64 && gc != 96 && gc != 128 && gc != 192 && gc != 256) {
            naf_set_error("naf_xna_head_reg: dlogits_channels %d is not a value width the attention backward serves (32, 64, 96, 128, 192, 256)", gc);
            return NAF_ERR_UNSUPPORTED;
        }
        if (!naf_aligned(c->dlogits, 16)) {
            naf_set_error("naf_xna_head_reg: the fused kernel needs a 16-byte aligned dlogits");
            return NAF_ERR_UNSUPPORTED;
        }
        for (int i = 0; i < 3; ++i) {
            if (c->dlogits_stride[i] % 8) {
                naf_set_error("naf_xna_head_reg: the fused kernel needs dlogits strides that are multiples of 8 elements");
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

// ---- the regression epilogue: one workgroup per (batch, cell) leaves a row of ten fp64 partial sums; the kernel below adds them ----
namespace {
constexpr int REG_FIN_T = 256;

// errors[i] += sum over the n rows of partial[row][i]: thread t adds rows t, t + 256, ... in that order, then a fixed tree over the 256
// threads, all in fp64 -- the same bits on every run
__global__ __launch_bounds__(REG_FIN_T) void xna_head_reg_finish_kernel(const double* __restrict__ partial, int64_t n, double* __restrict__ errors) {
    __shared__ double red[REG_FIN_T];
    double acc[XNA_HEAD_REG_STATS];
#pragma unroll
    for (int i = 0; i < XNA_HEAD_REG_STATS; ++i) acc[i] = 0.0;
    for (int64_t row = threadIdx.x; row < n; row += REG_FIN_T) {
#pragma unroll
        for (int i = 0; i < XNA_HEAD_REG_STATS; ++i) acc[i] += partial[row * XNA_HEAD_REG_STATS + i];
    }
#pragma unroll
    for (int i = 0; i < XNA_HEAD_REG_STATS; ++i) {
        red[threadIdx.x] = acc[i];
        __syncthreads();
        for (int s = REG_FIN_T / 2; s > 0; s >>= 1) {
            if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
            __syncthreads();
        }
        if (threadIdx.x == 0) errors[i] += red[0];
        __syncthreads();
    }
}
}  // namespace

// workgroups of the launch = rows of the statistics workspace (xna_headsum_fill's grid)
size_t naf_xna_head_reg_ws(const naf_xna_head_reg_args* c) {
    if (c->errors == nullptr) return 0;
    return (size_t)c->head.B * (size_t)c->head.h * (size_t)c->head.w * XNA_HEAD_REG_STATS * sizeof(double);
}

int naf_launch_xna_head_reg(const naf_xna_head_reg_args* c, float scale, hipStream_t s) {
    static_assert(XNA_HEAD_REG_STATS == NAF_HEAD_REG_STATS, "the kernel's row is the header's");
    XnaHeadRegExtra x;
    x.target = c->target;
    x.valid = c->valid;
    x.loss = c->loss;
    x.dlogits = static_cast<bf16_t*>(c->dlogits);
    x.partial = c->errors != nullptr ? static_cast<double*>(c->workspace) : nullptr;
    x.gc = c->dlogits != nullptr ? c->dlogits_channels : 0;
    x.kind = c->kind;
    x.beta = c->beta;
    x.clamp_lo = c->clamp_lo;
    x.clamp_hi = c->clamp_hi;
    for (int i = 0; i < 4; ++i) x.ts[i] = c->t_stride[i];
    for (int i = 0; i < 3; ++i) {
        x.ms[i] = c->valid_stride[i]; x.ls[i] = c->loss_stride[i]; x.gs[i] = c->dlogits_stride[i];
    }
    const int rc = head_launch(&c->head, scale, s, "xna_head_reg", "xna_head_kernel (regression epilogue)", x);
    if (rc != NAF_OK || c->errors == nullptr) return rc;
    const int64_t rows = (int64_t)c->head.B * c->head.h * c->head.w;
    hipLaunchKernelGGL(xna_head_reg_finish_kernel, dim3(1), dim3(REG_FIN_T), 0, s, static_cast<const double*>(c->workspace), rows, c->errors);
    return naf_check_launch("xna_head_reg_finish_kernel");
}
