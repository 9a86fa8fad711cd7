// naf_xna_mse_*: the table-driven MFMA attention forward with the training objective (mean squared error against a target) in its
// epilogue.  The attention launch (xna_union_mse_kernel.h) leaves one fp32 partial sum per wave in the caller's workspace; the
// one-workgroup kernel below adds them in fp64 in a fixed order.  The workgroup plan and the parameters are the plain kernel's (xna_union_fill).
#include <math.h>

#include "xna_union_mse_kernel.h"

// the instances: xna_union_mse_inst.hip, one object per window
#define NAF_X(K) extern template int xna_union_mse_launch_ks<K>(const XnaUnionMseParams&, int, size_t, hipStream_t);
NAF_FOR_WINDOWS(NAF_X)
#undef NAF_X

namespace {
constexpr int FIN_T = 256;

// loss = (sum of n partials) / N: thread t adds partials t, t + 256, ... in that order, then a fixed tree over the 256 threads
__global__ __launch_bounds__(FIN_T) void xna_mse_finish_kernel(const float* __restrict__ partial, int64_t n, double inv_n, float* __restrict__ loss) {
    __shared__ double red[FIN_T];
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += FIN_T) acc += (double)partial[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = FIN_T / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (float)(red[0] * inv_n);
}

struct MsePlan {
    UnionPlan pl;
    XnaUnionMseParams p;    // the plain kernel's part filled (xna_union_fill); the objective is naf_xna_mse_fwd's
    int nw;
};

// the request as the plain union kernel would see it (a stand-in for a NULL gradient buffer: nothing is dereferenced)
naf_xna_args plain_args(const naf_xna_mse_args* m) {
    naf_xna_args a = m->a;
    a.path = NAF_XNA_UNION;
    a.out_dtype = NAF_BF16;
    if (a.out == nullptr) {
        a.out = const_cast<void*>(a.q);
        a.o_stride[0] = (int64_t)a.Ho * a.Wo * a.heads * a.Dv;
        a.o_stride[1] = a.Dv;
        a.o_stride[2] = (int64_t)a.Wo * a.heads * a.Dv;
        a.o_stride[3] = (int64_t)a.heads * a.Dv;
    }
    return a;
}

// NAF_OK with *out filled, or the status naf_xna_mse_supported reports (negated there)
int mse_plan(const naf_xna_mse_args* m, MsePlan* out) {
    NAF_REQUIRE(m != nullptr, "naf_xna_mse: args is NULL");
    NAF_REQUIRE(m->a.q && m->a.k_lr && m->a.v_lr && m->target, "naf_xna_mse: NULL tensor pointer");
    NAF_REQUIRE(m->reserved == 0, "naf_xna_mse: reserved must be 0");
    NAF_REQUIRE(m->target_dtype == NAF_BF16 || m->target_dtype == NAF_F32, "naf_xna_mse: target_dtype %d", m->target_dtype);
    NAF_REQUIRE(naf_aligned(m->target, m->target_dtype == NAF_F32 ? 4 : 2), "naf_xna_mse: target is not aligned to its element size");
    NAF_REQUIRE(m->a.out == nullptr || m->a.out_dtype == NAF_BF16, "naf_xna_mse: the gradient buffer (a.out) must be NAF_BF16, got out_dtype %d", m->a.out_dtype);
    NAF_REQUIRE(m->a.logits == nullptr && m->a.rope_tab_y == nullptr && m->a.rope_tab_x == nullptr,
                "naf_xna_mse: logits and rotate-on-load (rope_tab_*) are not served by this entry");
    const naf_xna_args a = plain_args(m);   // strides of a stand-in buffer when there is no gradient to store
    const int sel = naf_xna_select(&a);     // argument validation and union eligibility, with naf_last_error set
    if (sel < 0) return -sel;
    if (sel != NAF_XNA_UNION || !(out->pl = plan_for(&a)).ok) {
        naf_set_error("naf_xna_mse: the table-driven MFMA kernel does not serve these arguments");
        return NAF_ERR_UNSUPPORTED;
    }
    out->nw = xna_union_mse_waves_rt(a.ky, out->pl.wt);
    const int rc = xna_union_fill(&a, out->pl, xna_scale(a.scale, a.Dq), "naf_xna_mse", out->p);
    out->p.out = m->a.out;
    return rc;
}
}  // namespace

extern "C" int naf_xna_mse_supported(const naf_xna_mse_args* m) {
    MsePlan pl;
    const int rc = mse_plan(m, &pl);
    return rc == NAF_OK ? 1 : -rc;
}

extern "C" size_t naf_xna_mse_workspace_bytes(const naf_xna_mse_args* m) {
    MsePlan pl;
    if (mse_plan(m, &pl) != NAF_OK) return 0;
    return (size_t)pl.p.nblocks * pl.nw * sizeof(float);
}

extern "C" int naf_xna_mse_fwd(const naf_xna_mse_args* m, naf_stream_t stream) {
    MsePlan pl;
    const int rc = mse_plan(m, &pl);
    if (rc != NAF_OK) return rc;
    const naf_xna_args* a = &m->a;
    NAF_REQUIRE(a->idx_y != nullptr && a->idx_x != nullptr, "naf_xna_mse_fwd: needs idx_y / idx_x from naf_axis_index_table");
    NAF_REQUIRE(m->loss != nullptr && naf_aligned(m->loss, 4), "naf_xna_mse_fwd: loss is NULL or misaligned");
    const size_t need = (size_t)pl.p.nblocks * pl.nw * sizeof(float);
    NAF_REQUIRE(m->workspace != nullptr && naf_aligned(m->workspace, 4) && m->workspace_bytes >= need,
                "naf_xna_mse_fwd: workspace of %zu bytes given, %zu needed (naf_xna_mse_workspace_bytes)", m->workspace ? m->workspace_bytes : (size_t)0, need);
    hipStream_t s = static_cast<hipStream_t>(stream);

    XnaUnionMseParams& p = pl.p;
    const double N = (double)a->B * a->heads * a->Dv * a->Ho * a->Wo;
    XnaUnionObjective& o = p.o;
    o.target = m->target;
    o.partial = static_cast<float*>(m->workspace);
    for (int i = 0; i < 4; ++i) o.ts[i] = m->target_stride[i];
    o.gscale = (float)(2.0 / N);
    o.tdtype = m->target_dtype;
    const int64_t* ts = m->target_stride;
    o.tvec = ts[1] == 1 && ts[0] % 4 == 0 && ts[2] % 4 == 0 && ts[3] % 4 == 0 && naf_aligned(m->target, m->target_dtype == NAF_F32 ? 16 : 8);
    o.grad = a->out != nullptr;

    int lrc;
    switch (a->ky) {
#define NAF_X(K) case K: lrc = xna_union_mse_launch_ks<K>(p, pl.pl.wt, pl.pl.lds, s); break;
        NAF_FOR_WINDOWS(NAF_X)
#undef NAF_X
        default:
            naf_set_error("naf_xna_mse_fwd: kernel size %d has no instantiation", a->ky);
            return NAF_ERR_UNSUPPORTED;
    }
    if (lrc != NAF_OK) return lrc;
    hipLaunchKernelGGL(xna_mse_finish_kernel, dim3(1), dim3(FIN_T), 0, s, static_cast<const float*>(m->workspace), (int64_t)p.nblocks * pl.nw, 1.0 / N, m->loss);
    return naf_check_launch("xna_mse_finish_kernel");
}
