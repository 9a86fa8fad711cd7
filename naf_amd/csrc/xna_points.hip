// Cross-scale neighbourhood attention at N query pixels (include/naf_hip.h, naf_xna_points): the scores, the softmax weights and the
// upsampled feature vector of the points (b, y, x) a caller names, without the dense [B, heads, Ho, Wo, ...] tensors around them.  What the
// reference's attention viewer reads out of model(image, feats, size, return_weights=True) (notebooks/attention_maps.ipynb, cell 11: one
// pixel's k*k numbers per head out of a full score tensor), and what any sparse consumer (keypoints, correspondences) wants.
//
// The arithmetic and the launch shape are xna_generic_kernel's (xna_generic.hip): one wave per (point, head), four waves per workgroup; lanes
// split the Dq contraction in the same order, wave_sum per key, scores to LDS, wave softmax with the same exponential, lanes split Dv.  Same
// loops, same reductions: for a point's (b, head, y, x) the scores and the fp32 feature vector are the bits that kernel writes for the pixel.
//
// Two forms of the query operand:
//   * rotated bf16 queries (naf_rope_pool_fwd's q);
//   * the UN-rotated guidance with the RoPE tables: the wave rotates the one vector it reads with naf_rope_rotate and rounds it to bf16 -- the
//     arithmetic and rounding of naf_rope_pool_fwd, so both forms give the same bits -- and no [B, Ho, Wo, C] query tensor is ever written.
// Either way the wave's query sits in LDS as fp32 (a lane reads back only what it wrote), so the key loop is one code path.
//
// A coordinate is compared with the sizes before it is used in any address: a point outside [0, B) x [0, Ho) x [0, Wo) reads nothing and gets
// NaN in its rows.  Table entries are clamped to the low-res grid (a table is the caller's memory).  Plain C++ and vector stores only.
#include "naf_common.h"

namespace {

struct XnaPointsParams {
    const bf16_t* q;
    const bf16_t* k;
    const bf16_t* v;        // NULL: weights only
    const int32_t* points;  // [N][3] = (b, y, x)
    const int32_t* idx_y;
    const int32_t* idx_x;
    const float* tab_y;     // both NULL: q is rotated already
    const float* tab_x;
    float* logits;
    float* probs;
    float* out;
    int32_t B, heads, Ho, Wo, h, w, Dq, Dv, ky, kx;
    float scale;
    int64_t qs[4], ks[4], vs[4];
    int64_t nquery;         // N * heads
};

__device__ __forceinline__ float pt_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float pt_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// F16: the values are IEEE half (the output is fp32 either way)
template <bool F16>
__global__ __launch_bounds__(256) void xna_points_kernel(const XnaPointsParams p) {
    extern __shared__ __attribute__((aligned(16))) float lds_all[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int KK = p.ky * p.kx;
    float* lg = lds_all + wave * (KK + p.Dq);   // scores, then un-normalised weights
    float* qf = lg + KK;                        // this wave's query, fp32 of its bf16 values
    const int64_t qi = (int64_t)blockIdx.x * 4 + wave;
    if (qi >= p.nquery) return;  // whole wave exits together; no block-level sync below
    const int64_t n = qi / p.heads;
    const int head = (int)(qi - n * p.heads);
    const int32_t* pt = p.points + n * 3;
    const int b = pt[0], y = pt[1], x = pt[2];

    float* lo = p.logits ? p.logits + qi * KK : nullptr;
    float* po = p.probs ? p.probs + qi * KK : nullptr;
    float* oo = p.out ? p.out + qi * p.Dv : nullptr;
    // unsigned compare: negative coordinates are out of range as well; nothing below this block runs for such a point
    if ((uint32_t)b >= (uint32_t)p.B || (uint32_t)y >= (uint32_t)p.Ho || (uint32_t)x >= (uint32_t)p.Wo) {
        const float nan = __builtin_nanf("");
        if (lo) for (int key = lane; key < KK; key += 64) lo[key] = nan;
        if (po) for (int key = lane; key < KK; key += 64) po[key] = nan;
        if (oo) for (int c = lane; c < p.Dv; c += 64) oo[c] = nan;
        return;
    }

    const bf16_t* qp = p.q + b * p.qs[0] + head * p.qs[1] + (int64_t)y * p.qs[2] + (int64_t)x * p.qs[3];
    const bf16_t* kb = p.k + b * p.ks[0] + head * p.ks[1];
    const int32_t* iy = p.idx_y + (int64_t)y * p.ky;
    const int32_t* ix = p.idx_x + (int64_t)x * p.kx;

    if (p.tab_y != nullptr) {
        // RoPE (rope.py:15-34,139-153) inside the head: channel t < Dq/2 pairs with t + Dq/2; angle t < Dq/4 is the row's, else the column's
        const int half = p.Dq >> 1, quarter = p.Dq >> 2;
        const float* ty = p.tab_y + (int64_t)y * 2 * quarter;
        const float* tx = p.tab_x + (int64_t)x * 2 * quarter;
        for (int d = lane; d < p.Dq; d += 64) {
            const int t = d < half ? d : d - half;
            const float* tb = t < quarter ? ty + t : tx + (t - quarter);
            float o1, o2;
            naf_rope_rotate((float)qp[t], (float)qp[t + half], tb[0], tb[quarter], o1, o2);
            qf[d] = (float)(bf16_t)(d < half ? o1 : o2);
        }
    } else {
        for (int d = lane; d < p.Dq; d += 64) qf[d] = (float)qp[d];
    }

    // logits
    for (int key = 0; key < KK; ++key) {
        const int ty = key / p.kx, tx = key - ty * p.kx;
        const int cy = min(max(iy[ty], 0), p.h - 1), cx = min(max(ix[tx], 0), p.w - 1);
        const bf16_t* kp = kb + (int64_t)cy * p.ks[2] + (int64_t)cx * p.ks[3];
        float acc = 0.f;
        for (int d = lane; d < p.Dq; d += 64) acc = fmaf(qf[d], (float)kp[d], acc);
        acc = pt_wave_sum(acc) * p.scale;
        if (lane == 0) lg[key] = acc;
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): LDS writes of lane 0 visible to the wave
    if (lo) for (int key = lane; key < KK; key += 64) lo[key] = lg[key];
    // softmax
    float m = -INFINITY;
    for (int key = lane; key < KK; key += 64) m = fmaxf(m, lg[key]);
    m = pt_wave_max(m);
    float sum = 0.f;
    for (int key = lane; key < KK; key += 64) {
        const float e = __expf(lg[key] - m);
        lg[key] = e;
        sum += e;
    }
    sum = pt_wave_sum(sum);
    const float inv = 1.0f / sum;
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xc07f);
    if (po) for (int key = lane; key < KK; key += 64) po[key] = lg[key] * inv;
    if (!oo) return;
    // weighted sum of values
    const bf16_t* vb = p.v + b * p.vs[0] + head * p.vs[1];
    for (int c = lane; c < p.Dv; c += 64) {
        float acc = 0.f;
        for (int key = 0; key < KK; ++key) {
            const int ty = key / p.kx, tx = key - ty * p.kx;
            const int cy = min(max(iy[ty], 0), p.h - 1), cx = min(max(ix[tx], 0), p.w - 1);
            const bf16_t* vp = vb + (int64_t)cy * p.vs[2] + (int64_t)cx * p.vs[3];
            if constexpr (F16) acc = fmaf(lg[key], (float)reinterpret_cast<const f16_t*>(vp)[c], acc);
            else acc = fmaf(lg[key], (float)vp[c], acc);
        }
        oo[c] = acc * inv;
    }
}

}  // namespace

extern "C" int naf_xna_points(const naf_xna_points_args* a, naf_stream_t stream) {
    NAF_REQUIRE(a != nullptr, "naf_xna_points: args is NULL");
    NAF_REQUIRE(a->reserved == 0, "naf_xna_points: reserved fields must be 0");
    NAF_REQUIRE(a->N >= 0, "naf_xna_points: N = %d points", a->N);
    NAF_REQUIRE(a->B >= 1 && a->heads >= 1 && a->Ho >= 1 && a->Wo >= 1 && a->h >= 1 && a->w >= 1 && a->Dq >= 1 && a->ky >= 1 && a->kx >= 1,
                "naf_xna_points: every size must be at least 1 (got B=%d heads=%d Ho=%d Wo=%d h=%d w=%d Dq=%d ky=%d kx=%d)", a->B, a->heads,
                a->Ho, a->Wo, a->h, a->w, a->Dq, a->ky, a->kx);
    NAF_REQUIRE(a->logits || a->probs || a->out, "naf_xna_points: no output asked for (logits, probs and out are all NULL)");
    NAF_REQUIRE(!a->out || a->v_lr, "naf_xna_points: `out` needs the values v_lr (v_lr NULL produces weights only)");
    NAF_REQUIRE(!a->out || a->Dv >= 1, "naf_xna_points: Dv = %d value channels", a->Dv);
    NAF_REQUIRE(a->v_dtype == NAF_BF16 || a->v_dtype == NAF_F16, "naf_xna_points: v_dtype %d (the values are NAF_BF16 or NAF_F16)", a->v_dtype);
    NAF_REQUIRE((a->rope_tab_y == nullptr) == (a->rope_tab_x == nullptr), "naf_xna_points: rope_tab_y and rope_tab_x go together");
    NAF_REQUIRE(!a->rope_tab_y || a->Dq % 4 == 0, "naf_xna_points: RoPE needs a head dim that is a multiple of 4 (got Dq=%d)", a->Dq);
    for (int i = 0; i < 4; ++i)
        NAF_REQUIRE(a->q_stride[i] >= 0 && a->k_stride[i] >= 0 && (!a->v_lr || a->v_stride[i] >= 0), "naf_xna_points: strides are non-negative");
    const int64_t nquery = (int64_t)a->N * a->heads;
    const int64_t nb = (nquery + 3) / 4;
    NAF_REQUIRE(nb <= 0x7fffffffLL, "naf_xna_points: %lld (point, head) pairs out of range", (long long)nquery);
    const size_t lds = (size_t)4 * ((size_t)a->ky * a->kx + a->Dq) * sizeof(float);
    if (lds > 64 * 1024) {
        naf_set_error("naf_xna_points: kernel %dx%d with head dim %d too large for the point kernel's LDS", a->ky, a->kx, a->Dq);
        return NAF_ERR_UNSUPPORTED;
    }
    if (a->N == 0) return NAF_OK;   // nothing to launch; the pointers may be anything
    NAF_REQUIRE(a->q && a->k_lr && a->points && a->idx_y && a->idx_x, "naf_xna_points: NULL tensor pointer (q, k_lr, points, idx_y, idx_x)");
    NAF_REQUIRE(naf_aligned(a->q, 2) && naf_aligned(a->k_lr, 2) && naf_aligned(a->v_lr, 2) && naf_aligned(a->points, 4) && naf_aligned(a->idx_y, 4) &&
                    naf_aligned(a->idx_x, 4) && naf_aligned(a->rope_tab_y, 4) && naf_aligned(a->rope_tab_x, 4) && naf_aligned(a->logits, 4) &&
                    naf_aligned(a->probs, 4) && naf_aligned(a->out, 4),
                "naf_xna_points: a pointer is not aligned to its element size");
    XnaPointsParams p;
    p.q = static_cast<const bf16_t*>(a->q);
    p.k = static_cast<const bf16_t*>(a->k_lr);
    p.v = a->out ? static_cast<const bf16_t*>(a->v_lr) : nullptr;
    p.points = a->points;
    p.idx_y = a->idx_y; p.idx_x = a->idx_x;
    p.tab_y = a->rope_tab_y; p.tab_x = a->rope_tab_x;
    p.logits = a->logits; p.probs = a->probs; p.out = a->out;
    p.B = a->B; p.heads = a->heads; p.Ho = a->Ho; p.Wo = a->Wo; p.h = a->h; p.w = a->w; p.Dq = a->Dq; p.Dv = a->Dv; p.ky = a->ky; p.kx = a->kx;
    p.scale = xna_scale(a->scale, a->Dq);
    for (int i = 0; i < 4; ++i) {
        p.qs[i] = a->q_stride[i]; p.ks[i] = a->k_stride[i]; p.vs[i] = a->v_lr ? a->v_stride[i] : 0;
    }
    p.nquery = nquery;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (a->v_dtype == NAF_F16) hipLaunchKernelGGL(xna_points_kernel<true>, dim3((uint32_t)nb), dim3(256), lds, s, p);
    else hipLaunchKernelGGL(xna_points_kernel<false>, dim3((uint32_t)nb), dim3(256), lds, s, p);
    return naf_check_launch("xna_points_kernel");
}
