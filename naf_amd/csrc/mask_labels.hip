// Soft masks to the label map of a video frame (include/naf_hip.h, naf_mask_labels): the reference's epilogue of one propagated frame
// (evaluation/eval_video_seg.py:444-457) -- bilinear upsample of the K soft masks to the mid grid, norm_mask per channel, argmax over the
// channels, PIL's nearest resize to the frame's size -- in two launches, without the [K, mid_h, mid_w] map and without a host synchronisation.
//
// Decomposition ("Masks to labels"):
//   * ml_value is THE upsampled value of (channel, mid pixel): ATen's align_corners = False arithmetic in fp32, every operation rounded on
//     its own (written with __fmul_rn / __fadd_rn / __fsub_rn, and the file is compiled with -ffp-contract=off, naf_amd/build.py).  Both
//     passes call it, so the value pass 2 normalises at the pixel that held a channel's maximum (minimum) IS that maximum (minimum): the
//     extreme pixels normalise to exactly 1 and 0
//   * pass 1, ml_minmax_kernel: workgroup (g, c) walks every G-th chunk of 256 mid pixels of channel c, a thread per pixel; minimum and
//     maximum go thread -> wave (shuffles) -> LDS -> ONE pair per workgroup in the caller's workspace [K][G][2].  Minimum and maximum do not
//     depend on the order they are taken in
//   * pass 2, ml_label_kernel: a workgroup owns 256 consecutive pixels of one output row.  Its prologue finishes the G pairs of every
//     channel (a wave per channel) and leaves, per channel, what norm_mask subtracts and divides by: (mn, mx - mn) where mx > 0, (0, 1)
//     where not -- u - 0 and u / 1 are u, so a channel without a positive value passes unchanged without a branch.  mx > 0 with mx == mn
//     divides 0 by 0: the channel is NaN, as in the reference.  Then a thread evaluates the K values at its output pixel's source mid pixel
//     (tab_y[oy], tab_x[ox]), normalises each (subtract, correctly rounded divide) and keeps the first maximum, a NaN beating everything
//     that is not one (torch.max on the CPU); one byte per thread, consecutive along x
#include "naf_common.h"

namespace {

constexpr int ML_THREADS = 256;
constexpr int ML_MAXK = NAF_MASK_LABELS_MAX_CHANNELS, ML_MAX_DIM = NAF_MASK_LABELS_MAX_SIZE;
constexpr int ML_PAIRS = 1024;   // most (channel, workgroup) pairs of pass 1: K * G <= ML_PAIRS
static_assert((size_t)ML_PAIRS * 2 * sizeof(float) == NAF_MASK_LABELS_WORKSPACE_BYTES, "the documented workspace holds every pair");
static_assert(ML_MAXK <= ML_PAIRS && ML_MAXK <= 255, "a workgroup per channel at least; labels are bytes");

struct MlParams {
    const float* seg;
    const int32_t* tab_y;
    const int32_t* tab_x;
    uint8_t* out;
    float* ws;
    int64_t sc, sy, sx;   // elements between channels, rows and columns of seg
    int64_t out_stride;
    int K, h, w, mh, mw, oh, ow;
    int G;                // workgroups per channel in pass 1
    float scale_y, scale_x;
};

// One axis of F.interpolate(mode = "bilinear", align_corners = False) at destination index dst: the two source indices and their weights
// (ATen area_pixel_compute_source_index / compute_indices_weights_linear, fp32)
struct MlAxis {
    int i0, i1;
    float l0, l1;
};

__device__ __forceinline__ MlAxis ml_axis(int dst, float scale, int in) {
    const float src = fmaxf(__fsub_rn(__fmul_rn(scale, __fadd_rn((float)dst, 0.5f)), 0.5f), 0.f);
    MlAxis a;
    a.i0 = min((int)src, in - 1);
    a.i1 = a.i0 + (a.i0 < in - 1 ? 1 : 0);
    a.l1 = __fsub_rn(src, (float)a.i0);
    a.l0 = __fsub_rn(1.f, a.l1);
    return a;
}

// h0 * (w0 * v00 + w1 * v01) + h1 * (w0 * v10 + w1 * v11), each operation rounded once; `ch` points at the channel's pixel (0, 0)
__device__ __forceinline__ float ml_value(const float* ch, int64_t sy, int64_t sx, const MlAxis& ay, const MlAxis& ax) {
    const float* r0 = ch + ay.i0 * sy;
    const float* r1 = ch + ay.i1 * sy;
    const float v00 = r0[ax.i0 * sx], v01 = r0[ax.i1 * sx], v10 = r1[ax.i0 * sx], v11 = r1[ax.i1 * sx];
    const float top = __fadd_rn(__fmul_rn(ax.l0, v00), __fmul_rn(ax.l1, v01));
    const float bot = __fadd_rn(__fmul_rn(ax.l0, v10), __fmul_rn(ax.l1, v11));
    return __fadd_rn(__fmul_rn(ay.l0, top), __fmul_rn(ay.l1, bot));
}

__device__ __forceinline__ void ml_wave_minmax(float& mn, float& mx) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, off, 64));
        mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    }
}

__global__ __launch_bounds__(ML_THREADS) void ml_minmax_kernel(const MlParams p) {
    __shared__ float red[2 * (ML_THREADS / 64)];
    const int tid = threadIdx.x, g = blockIdx.x, c = blockIdx.y;
    const float* ch = p.seg + c * p.sc;
    const uint32_t P = (uint32_t)p.mh * (uint32_t)p.mw, step = (uint32_t)p.G * ML_THREADS;   // P < 2^31, step <= 2^18
    float mn = __builtin_inff(), mx = -__builtin_inff();
    for (uint32_t i = (uint32_t)g * ML_THREADS + tid; i < P; i += step) {
        const uint32_t y = i / (uint32_t)p.mw, x = i - y * (uint32_t)p.mw;
        const float v = ml_value(ch, p.sy, p.sx, ml_axis((int)y, p.scale_y, p.h), ml_axis((int)x, p.scale_x, p.w));
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
    }
    ml_wave_minmax(mn, mx);
    if ((tid & 63) == 0) {
        red[2 * (tid >> 6)] = mn;
        red[2 * (tid >> 6) + 1] = mx;
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int wv = 1; wv < ML_THREADS / 64; ++wv) {
            mn = fminf(mn, red[2 * wv]);
            mx = fmaxf(mx, red[2 * wv + 1]);
        }
        float* d = p.ws + ((size_t)c * p.G + g) * 2;   // every workgroup holds at least one pixel (G <= chunks): never the +-inf it began with
        d[0] = mn;
        d[1] = mx;
    }
}

__global__ __launch_bounds__(ML_THREADS) void ml_label_kernel(const MlParams p) {
    __shared__ float sub[ML_MAXK], den[ML_MAXK];
    const int tid = threadIdx.x, lane = tid & 63;
    for (int c = tid >> 6; c < p.K; c += ML_THREADS / 64) {   // wave-uniform
        float mn = __builtin_inff(), mx = -__builtin_inff();
        const float* d = p.ws + (size_t)c * p.G * 2;
        for (int g = lane; g < p.G; g += 64) {
            mn = fminf(mn, d[2 * g]);
            mx = fmaxf(mx, d[2 * g + 1]);
        }
        ml_wave_minmax(mn, mx);
        if (lane == 0) {
            const bool pos = mx > 0.f;
            sub[c] = pos ? mn : 0.f;
            den[c] = pos ? __fsub_rn(mx, mn) : 1.f;
        }
    }
    __syncthreads();
    const int ox = blockIdx.x * ML_THREADS + tid, oy = blockIdx.y;
    if (ox >= p.ow) return;
    const int my = min(max(p.tab_y[oy], 0), p.mh - 1), mx_ = min(max(p.tab_x[ox], 0), p.mw - 1);   // a table is the caller's memory
    const MlAxis ay = ml_axis(my, p.scale_y, p.h), ax = ml_axis(mx_, p.scale_x, p.w);
    float best = 0.f;
    int label = 0;
    for (int c = 0; c < p.K; ++c) {
        const float u = ml_value(p.seg + c * p.sc, p.sy, p.sx, ay, ax);
        const float v = __fdiv_rn(__fsub_rn(u, sub[c]), den[c]);
        if (c == 0 || v > best || (v != v && best == best)) {
            best = v;
            label = c;
        }
    }
    p.out[(int64_t)oy * p.out_stride + ox] = (uint8_t)label;
}

// workgroups per channel in pass 1: one per 256 mid pixels, as many as K * G <= ML_PAIRS allows
inline int ml_groups(const naf_mask_labels_args* a) {
    const int64_t chunks = ((int64_t)a->mid_h * a->mid_w + ML_THREADS - 1) / ML_THREADS;
    const int64_t cap = ML_PAIRS / a->K;
    return (int)(chunks < cap ? chunks : cap);
}

}  // namespace

#define ML_SERVED(cond, ...)            \
    do {                                \
        if (!(cond)) {                  \
            naf_set_error(__VA_ARGS__); \
            return NAF_ERR_UNSUPPORTED; \
        }                               \
    } while (0)

extern "C" {

int naf_nearest_resize_table(int32_t* out, int32_t n_in, int32_t n_out) {
    NAF_REQUIRE(out != nullptr, "naf_nearest_resize_table: out is NULL");
    NAF_REQUIRE(n_in >= 1 && n_out >= 1, "naf_nearest_resize_table: sizes must be at least 1 (got n_in=%d n_out=%d)", n_in, n_out);
    // the accumulation IS the definition: xo after x additions is not (x + 0.5) * s rounded once
    const double s = (double)n_in / (double)n_out;
    volatile double xo = 0.5 * s;
    for (int x = 0; x < n_out; ++x) {
        const double v = xo;
        const int i = v >= (double)n_in ? n_in - 1 : (int)v;
        out[x] = i > n_in - 1 ? n_in - 1 : i;
        xo = v + s;
    }
    return NAF_OK;
}

int naf_mask_labels_select(const naf_mask_labels_args* a) {
    NAF_REQUIRE(a != nullptr, "naf_mask_labels: args is NULL");
    NAF_REQUIRE(a->K >= 1 && a->h >= 1 && a->w >= 1 && a->mid_h >= 1 && a->mid_w >= 1 && a->out_h >= 1 && a->out_w >= 1,
                "naf_mask_labels: K and every size must be at least 1 (got K=%d, %d x %d -> %d x %d -> %d x %d)", a->K, a->h, a->w, a->mid_h,
                a->mid_w, a->out_h, a->out_w);
    NAF_REQUIRE(a->reserved == 0, "naf_mask_labels: reserved fields must be 0");
    ML_SERVED(a->K <= ML_MAXK, "naf_mask_labels: K = %d channels are not served: 1 <= K <= 64", a->K);
    ML_SERVED(a->h <= ML_MAX_DIM && a->w <= ML_MAX_DIM, "naf_mask_labels: a %d x %d mask grid is not served: h, w <= 16384", a->h, a->w);
    ML_SERVED(a->mid_h <= ML_MAX_DIM && a->mid_w <= ML_MAX_DIM, "naf_mask_labels: a %d x %d mid grid is not served: mid_h, mid_w <= 16384", a->mid_h,
              a->mid_w);
    ML_SERVED(a->out_h <= ML_MAX_DIM && a->out_w <= ML_MAX_DIM, "naf_mask_labels: a %d x %d label map is not served: out_h, out_w <= 16384", a->out_h,
              a->out_w);
    return NAF_OK;
}

int naf_mask_labels(const naf_mask_labels_args* a, naf_stream_t stream) {
    const int rc = naf_mask_labels_select(a);
    if (rc != NAF_OK) return rc;
    NAF_REQUIRE(a->seg && a->tab_y && a->tab_x && a->out && a->workspace, "naf_mask_labels: NULL tensor pointer");
    NAF_REQUIRE(naf_aligned(a->seg, 4) && naf_aligned(a->tab_y, 4) && naf_aligned(a->tab_x, 4) && naf_aligned(a->workspace, 4),
                "naf_mask_labels: seg, tab_y, tab_x and workspace must be 4-byte aligned");
    NAF_REQUIRE(a->workspace_bytes >= NAF_MASK_LABELS_WORKSPACE_BYTES, "naf_mask_labels: workspace of %zu bytes, %d are needed", a->workspace_bytes,
                NAF_MASK_LABELS_WORKSPACE_BYTES);
    NAF_REQUIRE(a->out_stride >= a->out_w, "naf_mask_labels: out_stride = %lld bytes is shorter than a row of %d", (long long)a->out_stride, a->out_w);
    MlParams p;
    p.seg = a->seg; p.tab_y = a->tab_y; p.tab_x = a->tab_x; p.out = a->out; p.ws = a->workspace;
    p.sc = a->seg_stride[0]; p.sy = a->seg_stride[1]; p.sx = a->seg_stride[2];
    p.out_stride = a->out_stride;
    p.K = a->K; p.h = a->h; p.w = a->w; p.mh = a->mid_h; p.mw = a->mid_w; p.oh = a->out_h; p.ow = a->out_w;
    p.G = ml_groups(a);
    p.scale_y = (float)a->h / (float)a->mid_h;
    p.scale_x = (float)a->w / (float)a->mid_w;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(ml_minmax_kernel, dim3((unsigned)p.G, (unsigned)p.K), dim3(ML_THREADS), 0, s, p);
    int rl = naf_check_launch("ml_minmax_kernel");
    if (rl != NAF_OK) return rl;
    hipLaunchKernelGGL(ml_label_kernel, dim3((unsigned)((p.ow + ML_THREADS - 1) / ML_THREADS), (unsigned)p.oh), dim3(ML_THREADS), 0, s, p);
    return naf_check_launch("ml_label_kernel");
}

}  // extern "C"
