// Frame preparation (include/naf_hip.h, naf_image_prep): what the reference's callers do in torch before anything reaches naf(...) -- resize
// a decoded frame, normalise it with the backbone's and with the upsampler's statistics, resize the normalised image again
// (evaluation/eval_video_seg.py:577-597, train.py:115-126, utils/training.py:47, evaluation/eval_seg_probing.py:97-98) -- for up to
// NAF_IMAGE_PREP_MAX_VIEWS derived images of ONE source in ONE launch, without the intermediate images and from the uint8 frame as decoded.
//
// Decomposition:
//   * a view is: first resize -> normalise -> second resize -> store, every step optional.  All arithmetic is fp32, every operation rounded on
//     its own (__fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn, and the file is compiled with -ffp-contract=off, naf_amd/build.py)
//   * ONE form serves the three resize modes.  An axis is n taps with weights, n = 1 (none: weight 1), 2 (bilinear: l0, l1) or 4 (bicubic);
//     a value is the left-to-right sum over the rows of wy[j] * (the left-to-right sum over the columns of wx[i] * v[j][i]).  With two taps that
//     is ATen's h0 * (w0 * v00 + w1 * v01) + h1 * (w0 * v10 + w1 * v11) bit for bit, with four its cubic_interp1d over rows, then over the four
//     row results, and with one tap 1 * (1 * v) = v
//   * ip_first is THE normalised first-stage value of a view at (b, y, x), its three channels at once (they share the taps); the second
//     stage calls it once per tap -- 4 times (bilinear) or 16 times (bicubic) -- exactly as if that fp32 image had been written to memory.
//     At most 16 x 16 x 3 source reads per output pixel from an image of a few MB: they stay in the caches
//   * the source type and the first-stage mode are template arguments (a kernel per type, a body per mode, chosen per workgroup): as
//     run-time switches they put every load behind a branch of its own, one waiting for the other (0.057 ms against 0.024 ms on the DAVIS call)
//   * a flat block list over the views' output pixels: view v owns blocks [first_block, first_block + ceil(B * h2 * w2 / 256)), a thread owns
//     one output pixel and its three channels.  Consecutive threads are consecutive along x: the three bytes of an HWC uint8 pixel are adjacent,
//     the writes to each channel plane are consecutive
//   * pure gather: no workspace, no atomics, no LDS, no host synchronisation; two runs give the same bits
#include "naf_common.h"

namespace {

constexpr int IP_THREADS = 256;
constexpr int IP_MAX_VIEWS = NAF_IMAGE_PREP_MAX_VIEWS, IP_MAX_DIM = NAF_IMAGE_PREP_MAX_SIZE;

struct IpView {
    void* out;
    int64_t os[4];             // elements between images, channels, rows and columns of out
    float mean[3], std[3];
    float sy1, sx1, sy2, sx2;  // fl(float(n_in) / float(n_out)) of the two resizes
    int h1, w1, h2, w2;
    uint32_t first_block, pixels;   // pixels = B * h2 * w2 < 2^31
    int mode1, mode2, normalise, out_dtype;
};

struct IpParams {
    const void* src;
    int64_t ss[4];             // elements between images, channels, rows and columns of src
    int B, H, W;
    int src_dtype, hflip, n_views;
    IpView v[IP_MAX_VIEWS];
};

// One axis of a resize at destination index dst: the taps (clamped into the source) and their weights
struct IpAxis {
    int n;
    int i[4];
    float w[4];
};

// ATen's cubic convolution coefficients (UpSample.h, A = -0.75), every operation rounded: 1.25, 2.25, -3.75, -6 and -3 are exact
__device__ __forceinline__ float ip_c1(float x) {   // ((A + 2) x - (A + 3)) x x + 1
    return __fadd_rn(__fmul_rn(__fmul_rn(__fsub_rn(__fmul_rn(1.25f, x), 2.25f), x), x), 1.f);
}
__device__ __forceinline__ float ip_c2(float x) {   // ((A x - 5A) x + 8A) x - 4A
    return __fsub_rn(__fmul_rn(__fadd_rn(__fmul_rn(__fsub_rn(__fmul_rn(-0.75f, x), -3.75f), x), -6.f), x), -3.f);
}

__device__ __forceinline__ IpAxis ip_axis(int dst, float scale, int n_in, int mode) {
    IpAxis a;
    if (mode == NAF_PREP_NONE) {
        a.n = 1;
        a.i[0] = a.i[1] = a.i[2] = a.i[3] = min(dst, n_in - 1);
        a.w[0] = 1.f;
        a.w[1] = a.w[2] = a.w[3] = 0.f;
        return a;
    }
    // area_pixel_compute_source_index, align_corners = False
    const float real = __fsub_rn(__fmul_rn(scale, __fadd_rn((float)dst, 0.5f)), 0.5f);
    if (mode == NAF_PREP_BILINEAR) {
        const float src = fmaxf(real, 0.f);
        const int i0 = min((int)src, n_in - 1);   // (int)src <= n_in - 1 for every served size; the clamp keeps an address in bounds whatever src is
        a.n = 2;
        a.i[0] = i0;
        a.i[1] = a.i[2] = a.i[3] = min(i0 + 1, n_in - 1);
        a.w[1] = __fsub_rn(src, (float)i0);
        a.w[0] = __fsub_rn(1.f, a.w[1]);
        a.w[2] = a.w[3] = 0.f;
        return a;
    }
    const float fl = floorf(real);
    const float t = __fsub_rn(real, fl);
    const float u = __fsub_rn(1.f, t);
    const int i = (int)fl;
    a.n = 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) a.i[k] = min(max(i - 1 + k, 0), n_in - 1);
    a.w[0] = ip_c2(__fadd_rn(t, 1.f));
    a.w[1] = ip_c1(t);
    a.w[2] = ip_c1(u);
    a.w[3] = ip_c2(__fadd_rn(u, 1.f));   // ATen's 2 - t: (1 - t) + 1
    return a;
}

__device__ __forceinline__ int ip_tap(const IpAxis& a, int k) { return k == 0 ? a.i[0] : k == 1 ? a.i[1] : k == 2 ? a.i[2] : a.i[3]; }
__device__ __forceinline__ float ip_weight(const IpAxis& a, int k) { return k == 0 ? a.w[0] : k == 1 ? a.w[1] : k == 2 ? a.w[2] : a.w[3]; }

// The source value at element offset off: uint8 / 255 with a correctly rounded divide, fp32 as it is, bf16 widened
template <typename SrcT>
__device__ __forceinline__ float ip_load(const void* src, int64_t off) {
    if constexpr (std::is_same<SrcT, uint8_t>::value) return __fdiv_rn((float)static_cast<const uint8_t*>(src)[off], 255.f);
    else return (float)static_cast<const SrcT*>(src)[off];
}

// The normalised first-stage value of view v at (b, y, x), 0 <= y < h1, 0 <= x < w1: three channels.  The source type and the mode are
// template arguments: the N x N x 3 loads are independent instructions issued together, with no branch between them
template <typename SrcT, int M1>
__device__ __forceinline__ void ip_first(const IpParams& p, const IpView& v, int b, int y, int x, float out[3]) {
    constexpr int N = M1 == NAF_PREP_NONE ? 1 : M1 == NAF_PREP_BILINEAR ? 2 : 4;
    const IpAxis ay = ip_axis(y, v.sy1, p.H, M1), ax = ip_axis(x, v.sx1, p.W, M1);
    int64_t xo[N];
#pragma unroll
    for (int i = 0; i < N; ++i) xo[i] = (int64_t)(p.hflip ? p.W - 1 - ax.i[i] : ax.i[i]) * p.ss[3];
    const int64_t base = (int64_t)b * p.ss[0];
    float s[N][N][3];
#pragma unroll
    for (int j = 0; j < N; ++j)
#pragma unroll
        for (int i = 0; i < N; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) s[j][i][c] = ip_load<SrcT>(p.src, base + (int64_t)ay.i[j] * p.ss[2] + c * p.ss[1] + xo[i]);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            float r = __fmul_rn(ax.w[0], s[j][0][c]);
#pragma unroll
            for (int i = 1; i < N; ++i) r = __fadd_rn(r, __fmul_rn(ax.w[i], s[j][i][c]));
            const float t = __fmul_rn(ay.w[j], r);
            acc = j == 0 ? t : __fadd_rn(acc, t);
        }
        out[c] = v.normalise ? __fdiv_rn(__fsub_rn(acc, v.mean[c]), v.std[c]) : acc;
    }
}

// One output pixel of view v: the second resize over ip_first, and the store
template <typename SrcT, int M1>
__device__ __forceinline__ void ip_pixel(const IpParams& p, const IpView& v, uint32_t pix) {
    const uint32_t r = pix / (uint32_t)v.w2;
    const int x = (int)(pix - r * (uint32_t)v.w2), b = (int)(r / (uint32_t)v.h2), y = (int)(r - (uint32_t)b * (uint32_t)v.h2);
    const IpAxis ay = ip_axis(y, v.sy2, v.h1, v.mode2), ax = ip_axis(x, v.sx2, v.w1, v.mode2);
    float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll 1
    for (int j = 0; j < ay.n; ++j) {   // loops, not 16 copies of ip_first; the taps are picked with selects, so the axes stay in registers
        float row[3] = {0.f, 0.f, 0.f};
#pragma unroll 1
        for (int i = 0; i < ax.n; ++i) {
            float f[3];
            ip_first<SrcT, M1>(p, v, b, ip_tap(ay, j), ip_tap(ax, i), f);
            const float wx = ip_weight(ax, i);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float t = __fmul_rn(wx, f[c]);
                row[c] = i == 0 ? t : __fadd_rn(row[c], t);
            }
        }
        const float wy = ip_weight(ay, j);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float t = __fmul_rn(wy, row[c]);
            acc[c] = j == 0 ? t : __fadd_rn(acc[c], t);
        }
    }
    const int64_t o = (int64_t)b * v.os[0] + (int64_t)y * v.os[2] + (int64_t)x * v.os[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (v.out_dtype == NAF_F32) static_cast<float*>(v.out)[o + c * v.os[1]] = acc[c];
        else static_cast<bf16_t*>(v.out)[o + c * v.os[1]] = (bf16_t)acc[c];   // round to nearest even
    }
}

template <typename SrcT>
__global__ __launch_bounds__(IP_THREADS) void image_prep_kernel(const IpParams p) {
    int vi = 0;
#pragma unroll
    for (int k = 1; k < IP_MAX_VIEWS; ++k)
        if (k < p.n_views && blockIdx.x >= p.v[k].first_block) vi = k;   // block-uniform
    const IpView& v = p.v[vi];
    const uint32_t pix = (blockIdx.x - v.first_block) * IP_THREADS + threadIdx.x;
    if (pix >= v.pixels) return;
    if (v.mode1 == NAF_PREP_BILINEAR) ip_pixel<SrcT, NAF_PREP_BILINEAR>(p, v, pix);   // block-uniform
    else if (v.mode1 == NAF_PREP_BICUBIC) ip_pixel<SrcT, NAF_PREP_BICUBIC>(p, v, pix);
    else ip_pixel<SrcT, NAF_PREP_NONE>(p, v, pix);
}

inline bool ip_mode_ok(int m) { return m == NAF_PREP_NONE || m == NAF_PREP_BILINEAR || m == NAF_PREP_BICUBIC; }

}  // namespace

#define IP_SERVED(cond, ...)            \
    do {                                \
        if (!(cond)) {                  \
            naf_set_error(__VA_ARGS__); \
            return NAF_ERR_UNSUPPORTED; \
        }                               \
    } while (0)

extern "C" {

int naf_image_prep_select(const naf_image_prep_args* a) {
    NAF_REQUIRE(a != nullptr, "naf_image_prep: args is NULL");
    NAF_REQUIRE(a->reserved[0] == 0 && a->reserved[1] == 0, "naf_image_prep: reserved fields must be 0");
    NAF_REQUIRE(a->src_dtype == NAF_IMAGE_PREP_U8 || a->src_dtype == NAF_F32 || a->src_dtype == NAF_BF16,
                "naf_image_prep: src_dtype = %d; the source is NAF_IMAGE_PREP_U8, NAF_F32 or NAF_BF16", a->src_dtype);
    NAF_REQUIRE(a->hflip == 0 || a->hflip == 1, "naf_image_prep: hflip must be 0 or 1 (got %d)", a->hflip);
    NAF_REQUIRE(a->B >= 1 && a->H >= 1 && a->W >= 1, "naf_image_prep: B and every size must be at least 1 (got B=%d, source %d x %d)", a->B, a->H, a->W);
    NAF_REQUIRE(a->n_views >= 1, "naf_image_prep: n_views = %d: 1 <= views <= %d", a->n_views, IP_MAX_VIEWS);
    IP_SERVED(a->n_views <= IP_MAX_VIEWS, "naf_image_prep: n_views = %d views are not served: 1 <= views <= %d", a->n_views, IP_MAX_VIEWS);
    IP_SERVED(a->H <= IP_MAX_DIM && a->W <= IP_MAX_DIM, "naf_image_prep: a %d x %d source is not served: every size <= 16384", a->H, a->W);
    int64_t blocks = 0;
    for (int i = 0; i < a->n_views; ++i) {
        const naf_image_prep_view* v = &a->view[i];
        NAF_REQUIRE(v->reserved[0] == 0 && v->reserved[1] == 0, "naf_image_prep: view %d: reserved fields must be 0", i);
        NAF_REQUIRE(v->out_dtype == NAF_F32 || v->out_dtype == NAF_BF16, "naf_image_prep: view %d: out_dtype = %d; an output is NAF_F32 or NAF_BF16", i,
                    v->out_dtype);
        NAF_REQUIRE(ip_mode_ok(v->mode1) && ip_mode_ok(v->mode2), "naf_image_prep: view %d: modes (%d, %d); a mode is NAF_PREP_NONE, _BILINEAR or _BICUBIC",
                    i, v->mode1, v->mode2);
        NAF_REQUIRE(v->normalise == 0 || v->normalise == 1, "naf_image_prep: view %d: normalise must be 0 or 1 (got %d)", i, v->normalise);
        NAF_REQUIRE(v->h1 >= 1 && v->w1 >= 1 && v->h2 >= 1 && v->w2 >= 1,
                    "naf_image_prep: view %d: every size must be at least 1 (got %d x %d, then %d x %d)", i, v->h1, v->w1, v->h2, v->w2);
        IP_SERVED(v->h1 <= IP_MAX_DIM && v->w1 <= IP_MAX_DIM && v->h2 <= IP_MAX_DIM && v->w2 <= IP_MAX_DIM,
                  "naf_image_prep: view %d: %d x %d, then %d x %d is not served: every size <= 16384", i, v->h1, v->w1, v->h2, v->w2);
        NAF_REQUIRE(v->mode1 != NAF_PREP_NONE || (v->h1 == a->H && v->w1 == a->W),
                    "naf_image_prep: view %d: mode none requires equal sizes (first resize %d x %d -> %d x %d)", i, a->H, a->W, v->h1, v->w1);
        NAF_REQUIRE(v->mode2 != NAF_PREP_NONE || (v->h2 == v->h1 && v->w2 == v->w1),
                    "naf_image_prep: view %d: mode none requires equal sizes (second resize %d x %d -> %d x %d)", i, v->h1, v->w1, v->h2, v->w2);
        if (v->normalise)
            for (int c = 0; c < 3; ++c) {
                NAF_REQUIRE(v->mean[c] == v->mean[c] && v->std[c] == v->std[c], "naf_image_prep: view %d: mean / std of channel %d is NaN", i, c);
                NAF_REQUIRE(v->std[c] != 0.f, "naf_image_prep: view %d: std of channel %d is 0: std != 0", i, c);
            }
        const int64_t pixels = (int64_t)a->B * v->h2 * v->w2;
        IP_SERVED(pixels < (1LL << 31), "naf_image_prep: view %d: B * h * w = %lld output pixels are not served: below 2^31 per view", i, (long long)pixels);
        blocks += (pixels + IP_THREADS - 1) / IP_THREADS;
    }
    IP_SERVED(blocks <= 0x7fffffffLL, "naf_image_prep: a grid of %lld workgroups is not served: below 2^31", (long long)blocks);
    return NAF_OK;
}

int naf_image_prep(const naf_image_prep_args* a, naf_stream_t stream) {
    const int rc = naf_image_prep_select(a);
    if (rc != NAF_OK) return rc;
    NAF_REQUIRE(a->src != nullptr, "naf_image_prep: NULL source pointer");
    NAF_REQUIRE(naf_aligned(a->src, a->src_dtype == NAF_F32 ? 4 : a->src_dtype == NAF_BF16 ? 2 : 1),
                "naf_image_prep: the source must be aligned to its element (4 bytes for fp32, 2 for bf16)");
    IpParams p;
    p.src = a->src;
    for (int i = 0; i < 4; ++i) p.ss[i] = a->src_stride[i];
    p.B = a->B; p.H = a->H; p.W = a->W;
    p.src_dtype = a->src_dtype; p.hflip = a->hflip; p.n_views = a->n_views;
    uint32_t blocks = 0;
    for (int i = 0; i < IP_MAX_VIEWS; ++i) {
        const naf_image_prep_view* v = &a->view[i < a->n_views ? i : 0];   // unused slots repeat view 0: never selected (k < n_views)
        IpView& q = p.v[i];
        if (i < a->n_views) {
            NAF_REQUIRE(v->out != nullptr, "naf_image_prep: view %d: NULL output pointer", i);
            NAF_REQUIRE(naf_aligned(v->out, v->out_dtype == NAF_F32 ? 4 : 2),
                        "naf_image_prep: view %d: the output must be aligned to its element (4 bytes for fp32, 2 for bf16)", i);
        }
        q.out = v->out;
        for (int k = 0; k < 4; ++k) q.os[k] = v->out_stride[k];
        for (int c = 0; c < 3; ++c) {
            q.mean[c] = v->mean[c];
            q.std[c] = v->std[c];
        }
        q.sy1 = (float)a->H / (float)v->h1; q.sx1 = (float)a->W / (float)v->w1;
        q.sy2 = (float)v->h1 / (float)v->h2; q.sx2 = (float)v->w1 / (float)v->w2;
        q.h1 = v->h1; q.w1 = v->w1; q.h2 = v->h2; q.w2 = v->w2;
        q.mode1 = v->mode1; q.mode2 = v->mode2; q.normalise = v->normalise; q.out_dtype = v->out_dtype;
        q.pixels = (uint32_t)((int64_t)a->B * v->h2 * v->w2);
        q.first_block = blocks;
        if (i < a->n_views) blocks += (q.pixels + IP_THREADS - 1) / IP_THREADS;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (a->src_dtype == NAF_IMAGE_PREP_U8) hipLaunchKernelGGL(image_prep_kernel<uint8_t>, dim3(blocks), dim3(IP_THREADS), 0, s, p);
    else if (a->src_dtype == NAF_F32) hipLaunchKernelGGL(image_prep_kernel<float>, dim3(blocks), dim3(IP_THREADS), 0, s, p);
    else hipLaunchKernelGGL(image_prep_kernel<bf16_t>, dim3(blocks), dim3(IP_THREADS), 0, s, p);
    return naf_check_launch("image_prep_kernel");
}

}  // extern "C"
