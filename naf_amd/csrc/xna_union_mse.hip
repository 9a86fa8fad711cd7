// naf_xna_mse_*: the table-driven MFMA attention forward with the training objective (mean squared error against a target) in its
// epilogue.  The attention launch (xna_union_mse_kernel.h) leaves one fp32 partial sum per wave in the caller's workspace; the
// one-workgroup kernel below adds them in fp64 in a fixed order.  The workgroup plan is the plain kernel's (naf_xna_union_plan).
#include <math.h>

#include "xna_union_mse_kernel.h"

#define NAF_DECL(K) int naf_xna_union_mse_launch_k##K(const XnaUnionMseParams& p, int wt, size_t lds, hipStream_t s);
NAF_DECL(3) NAF_DECL(5) NAF_DECL(7) NAF_DECL(9) NAF_DECL(11) NAF_DECL(13) NAF_DECL(15)
#undef NAF_DECL

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
    int32_t pl[7];      // naf_xna_union_plan: {wt, ry, seg, hub, wub, dvt, lds}
    int nw;
    int64_t nblocks;
};

bool aligned_to(const void* p, size_t n) { return (reinterpret_cast<uintptr_t>(p) % n) == 0; }

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
    NAF_REQUIRE(aligned_to(m->target, m->target_dtype == NAF_F32 ? 4 : 2), "naf_xna_mse: target is not aligned to its element size");
    NAF_REQUIRE(m->a.out == nullptr || m->a.out_dtype == NAF_BF16, "naf_xna_mse: the gradient buffer (a.out) must be NAF_BF16, got out_dtype %d", m->a.out_dtype);
    NAF_REQUIRE(m->a.logits == nullptr && m->a.rope_tab_y == nullptr && m->a.rope_tab_x == nullptr,
                "naf_xna_mse: logits and rotate-on-load (rope_tab_*) are not served by this entry");
    const naf_xna_args a = plain_args(m);
    const int sel = naf_xna_select(&a);     // argument validation and union eligibility, with naf_last_error set
    if (sel < 0) return -sel;
    if (sel != NAF_XNA_UNION || !naf_xna_union_plan(&a, out->pl)) {
        naf_set_error("naf_xna_mse: the table-driven MFMA kernel does not serve these arguments");
        return NAF_ERR_UNSUPPORTED;
    }
    const int dvt = out->pl[5], ry = out->pl[1], seg = out->pl[2];
    out->nw = xna_union_mse_waves_rt(a.ky, out->pl[0]);
    out->nblocks = (int64_t)a.B * a.heads * (a.Dv / dvt) * ((a.Ho + ry - 1) / ry) * ((a.Wo + seg - 1) / seg);
    if (out->nblocks <= 0 || out->nblocks > 0x7fffffffLL) {
        naf_set_error("naf_xna_mse: grid of %lld workgroups out of range", (long long)out->nblocks);
        return NAF_ERR_INVALID;
    }
    return NAF_OK;
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
    return (size_t)pl.nblocks * pl.nw * sizeof(float);
}

extern "C" int naf_xna_mse_fwd(const naf_xna_mse_args* m, naf_stream_t stream) {
    MsePlan pl;
    const int rc = mse_plan(m, &pl);
    if (rc != NAF_OK) return rc;
    const naf_xna_args* a = &m->a;
    NAF_REQUIRE(a->idx_y != nullptr && a->idx_x != nullptr, "naf_xna_mse_fwd: needs idx_y / idx_x from naf_axis_index_table");
    NAF_REQUIRE(m->loss != nullptr && aligned_to(m->loss, 4), "naf_xna_mse_fwd: loss is NULL or misaligned");
    const size_t need = (size_t)pl.nblocks * pl.nw * sizeof(float);
    NAF_REQUIRE(m->workspace != nullptr && aligned_to(m->workspace, 4) && m->workspace_bytes >= need,
                "naf_xna_mse_fwd: workspace of %zu bytes given, %zu needed (naf_xna_mse_workspace_bytes)", m->workspace ? m->workspace_bytes : (size_t)0, need);
    hipStream_t s = static_cast<hipStream_t>(stream);

    const naf_xna_args pa = plain_args(m);      // strides of a stand-in buffer when there is no gradient to store
    XnaUnionMseParams p;
    p.q = static_cast<const bf16_t*>(a->q);
    p.k = static_cast<const bf16_t*>(a->k_lr);
    p.v = static_cast<const bf16_t*>(a->v_lr);
    p.out = a->out;
    p.idx_y = a->idx_y;
    p.idx_x = a->idx_x;
    p.B = a->B; p.heads = a->heads; p.Ho = a->Ho; p.Wo = a->Wo; p.h = a->h; p.w = a->w;
    p.dvt = pl.pl[5]; p.nchunk = a->Dv / pl.pl[5];
    p.ry = pl.pl[1]; p.seg = pl.pl[2];
    p.nyb = (a->Ho + p.ry - 1) / p.ry;
    p.nxb = (a->Wo + p.seg - 1) / p.seg;
    p.hub = pl.pl[3]; p.wub = pl.pl[4];
    p.nblocks = (uint32_t)pl.nblocks;
    p.scale_log2e = (a->scale > 0.f ? a->scale : 1.0f / sqrtf((float)a->Dq)) * 1.4426950408889634f;
    for (int i = 0; i < 4; ++i) {
        p.qs[i] = a->q_stride[i]; p.ks[i] = a->k_stride[i]; p.vs[i] = a->v_stride[i]; p.os[i] = pa.o_stride[i];
    }
    const double N = (double)a->B * a->heads * a->Dv * a->Ho * a->Wo;
    XnaUnionObjective& o = p.o;
    o.target = m->target;
    o.partial = static_cast<float*>(m->workspace);
    for (int i = 0; i < 4; ++i) o.ts[i] = m->target_stride[i];
    o.gscale = (float)(2.0 / N);
    o.tdtype = m->target_dtype;
    const int64_t* ts = m->target_stride;
    o.tvec = ts[1] == 1 && ts[0] % 4 == 0 && ts[2] % 4 == 0 && ts[3] % 4 == 0 && aligned_to(m->target, m->target_dtype == NAF_F32 ? 16 : 8);
    o.grad = a->out != nullptr;

    int lrc;
    const size_t lds = (size_t)pl.pl[6];
    switch (a->ky) {
        case 3: lrc = naf_xna_union_mse_launch_k3(p, pl.pl[0], lds, s); break;
        case 5: lrc = naf_xna_union_mse_launch_k5(p, pl.pl[0], lds, s); break;
        case 7: lrc = naf_xna_union_mse_launch_k7(p, pl.pl[0], lds, s); break;
        case 9: lrc = naf_xna_union_mse_launch_k9(p, pl.pl[0], lds, s); break;
        case 11: lrc = naf_xna_union_mse_launch_k11(p, pl.pl[0], lds, s); break;
        case 13: lrc = naf_xna_union_mse_launch_k13(p, pl.pl[0], lds, s); break;
        case 15: lrc = naf_xna_union_mse_launch_k15(p, pl.pl[0], lds, s); break;
        default:
            naf_set_error("naf_xna_mse_fwd: kernel size %d has no instantiation", a->ky);
            return NAF_ERR_UNSUPPORTED;
    }
    if (lrc != NAF_OK) return lrc;
    hipLaunchKernelGGL(xna_mse_finish_kernel, dim3(1), dim3(FIN_T), 0, s, static_cast<const float*>(m->workspace), (int64_t)pl.nblocks * pl.nw, 1.0 / N, m->loss);
    return naf_check_launch("xna_mse_finish_kernel");
}
