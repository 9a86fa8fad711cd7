// Denoising objective (include/naf_hip.h, naf_denoise_objective): the reference's DenoisingLoss with its backward (denoising.py:129-177) and
// its MetricsCalculator with the clamp in front of it (denoising.py:61-126, :302), one tile kernel plus a one-workgroup finishing kernel.
//
// Decomposition ("Denoising objective"):
//   * one workgroup (4 waves) owns one 32 x 32 tile of ONE (b, c) plane; planes are independent
//   * the tile of pred and target is staged in LDS as fp32 with a zero halo (zero padding is the reference's padding in both modes)
//   * loss: halo 2.  The SSIM terms S and the three adjoint maps a, b, c are formed on the tile plus ONE ring (34 x 34; zero outside the
//     image), a, b, c go to LDS, and a pixel's gradient is box(a) + 2 p box(b) + t box(c) over them: box is its own adjoint.  The nine
//     samples of a window sit in registers, so the (co)variances are taken in centred form, box((p - mu1)(t - mu2)): the same number as
//     box(p t) - mu1 mu2 without its cancellation against C2 = 9e-4.  Compiled with -ffp-contract=off (naf_amd/build.py): every fused
//     multiply-add here is written out, so that symmetric expressions of pred and target round symmetrically
//   * metrics: halo 5.  The 11 x 11 Gaussian window is separable: a horizontal pass writes the five row sums of 42 x 32 positions to LDS,
//     the vertical pass finishes them
//   * sums: a thread adds at most five terms, the workgroup's 256 threads add theirs in a binary tree (six shuffles, two LDS levels), the
//     partial goes to the caller's workspace; denoise_finish_kernel adds all partials in fp64 in a fixed order.  No atomics
#include "naf_common.h"

#include <math.h>

namespace {

constexpr int DN_T = 32;                          // tile edge
constexpr int DN_THREADS = 256;
constexpr int DN_LP = DN_T + 4, DN_LA = DN_T + 2; // loss: edge of the staged tile (halo 2) and of the a, b, c maps (halo 1)
constexpr int DN_WIN = 11, DN_MH = DN_WIN / 2;    // metrics window and halo
constexpr int DN_MP = DN_T + 2 * DN_MH;           // metrics: edge of the staged tile
constexpr float DN_C1 = 1e-4f, DN_C2 = 9e-4f;

struct DnParams {
    naf_denoise_args a;
    int tiles_x, tiles_y;
    float w1, w2, w3, inv_n;   // the gradient's fp32 constants
    float g[DN_WIN];           // the metrics window's fp32 vector
};

__device__ __forceinline__ float dn_load(const void* p, int dtype, int64_t off) {
    return dtype == NAF_F32 ? static_cast<const float*>(p)[off] : bf16_bits_to_float(static_cast<const uint16_t*>(p)[off]);
}

struct DnTile {
    int x0, y0;
    int64_t pbase, tbase, gbase;
};

__device__ __forceinline__ DnTile dn_tile(const DnParams& p) {
    const uint32_t bid = blockIdx.x, tx = bid % (uint32_t)p.tiles_x, r = bid / (uint32_t)p.tiles_x;
    const uint32_t ty = r % (uint32_t)p.tiles_y, plane = r / (uint32_t)p.tiles_y;
    const int64_t b = plane / (uint32_t)p.a.C, c = plane % (uint32_t)p.a.C;
    DnTile t;
    t.x0 = (int)tx * DN_T;
    t.y0 = (int)ty * DN_T;
    t.pbase = b * p.a.pred_stride[0] + c * p.a.pred_stride[1];
    t.tbase = b * p.a.target_stride[0] + c * p.a.target_stride[1];
    t.gbase = b * p.a.grad_stride[0] + c * p.a.grad_stride[1];
    return t;
}

// The workgroup's sum of each of v[0..2]: a binary tree over the 256 threads (8 additions on any path), written by thread 0 as one 16-byte
// line of the workspace.  `red` is 12 floats of LDS nothing else uses.
__device__ __forceinline__ void dn_block_partial(float (&v)[3], float* red, float* workspace) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v[k] += __shfl_xor(v[k], off, 64);
        if (lane == 0) red[wv * 3 + k] = v[k];
    }
    __syncthreads();
    if (tid == 0) {
        f32x4_t o;
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k] = (red[k] + red[3 + k]) + (red[6 + k] + red[9 + k]);
        o[3] = 0.f;
        reinterpret_cast<f32x4_t*>(workspace)[blockIdx.x] = o;
    }
}

__global__ __launch_bounds__(DN_THREADS) void denoise_loss_kernel(const DnParams p) {
    // staged pred | staged target | a | b | c | reduction scratch
    __shared__ float smem[2 * DN_LP * DN_LP + 3 * DN_LA * DN_LA + 12];
    float* sp = smem;
    float* st = sp + DN_LP * DN_LP;
    float* sa = st + DN_LP * DN_LP;
    float* sb = sa + DN_LA * DN_LA;
    float* sc = sb + DN_LA * DN_LA;
    float* red = sc + DN_LA * DN_LA;
    const int tid = threadIdx.x, H = p.a.H, W = p.a.W;
    const DnTile t = dn_tile(p);
    constexpr float inv9 = 1.f / 9.f;

    for (int i = tid; i < DN_LP * DN_LP; i += DN_THREADS) {
        const int iy = i / DN_LP, ix = i - iy * DN_LP, y = t.y0 - 2 + iy, x = t.x0 - 2 + ix;
        float vp = 0.f, vt = 0.f;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            vp = dn_load(p.a.pred, p.a.pred_dtype, t.pbase + y * p.a.pred_stride[2] + x * p.a.pred_stride[3]);
            vt = dn_load(p.a.target, p.a.target_dtype, t.tbase + y * p.a.target_stride[2] + x * p.a.target_stride[3]);
        }
        sp[i] = vp;
        st[i] = vt;
    }
    __syncthreads();

    // ---- S and the adjoint maps on the tile plus one ring; the tile's own positions add their terms ----
    float sums[3] = {0.f, 0.f, 0.f};   // |p - t|, (p - t)^2, S
    for (int i = tid; i < DN_LA * DN_LA; i += DN_THREADS) {
        const int iy = i / DN_LA, ix = i - iy * DN_LA, y = t.y0 - 1 + iy, x = t.x0 - 1 + ix;
        float av = 0.f, bv = 0.f, cv = 0.f;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            float pv[9], tv[9];
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    pv[dy * 3 + dx] = sp[(iy + dy) * DN_LP + ix + dx];
                    tv[dy * 3 + dx] = st[(iy + dy) * DN_LP + ix + dx];
                }
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                s1 += pv[k];
                s2 += tv[k];
            }
            const float mu1 = s1 * inv9, mu2 = s2 * inv9;
            float v11 = 0.f, v22 = 0.f, v12 = 0.f;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const float dp = pv[k] - mu1, dt = tv[k] - mu2;
                v11 = __builtin_fmaf(dp, dp, v11);
                v22 = __builtin_fmaf(dt, dt, v22);
                v12 = __builtin_fmaf(dp, dt, v12);
            }
            const float sg1 = v11 * inv9, sg2 = v22 * inv9, sg12 = v12 * inv9;
            const float n1 = 2.f * mu1 * mu2 + DN_C1, n2 = 2.f * sg12 + DN_C2;
            const float d1 = mu1 * mu1 + mu2 * mu2 + DN_C1, d2 = sg1 + sg2 + DN_C2;
            // S as a product of two quotients, b and c from ONE quotient u: where pred == target over the window, n1 == d1 and n2 == d2
            // bit for bit (this file is compiled without FMA contraction), so q1 = q2 = S = 1, a = 0 and 2 b + c = 0 exactly -- the
            // SSIM gradient of identical windows is exactly zero, as it is mathematically
            const float q1 = n1 / d1, q2 = n2 / d2, u = q1 / d2;
            const float S = q1 * q2;
            av = (2.f * mu2 * (n2 - n1) - 2.f * mu1 * S * (d2 - d1)) / (d1 * d2);
            bv = -(u * q2);
            cv = 2.f * u;
            if (iy >= 1 && iy <= DN_T && ix >= 1 && ix <= DN_T) {
                const float d = pv[4] - tv[4];
                sums[0] += fabsf(d);
                sums[1] = __builtin_fmaf(d, d, sums[1]);
                sums[2] += S;
            }
        }
        sa[i] = av;
        sb[i] = bv;
        sc[i] = cv;
    }
    __syncthreads();

    // ---- the gradient map ----
    if (p.a.grad != nullptr) {
#pragma unroll
        for (int k = 0; k < DN_T * DN_T / DN_THREADS; ++k) {
            const int py = (tid >> 5) + k * (DN_THREADS / DN_T), px = tid & 31, y = t.y0 + py, x = t.x0 + px;
            if (y >= H || x >= W) continue;
            float A = 0.f, B = 0.f, Cc = 0.f;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const int j = (py + dy) * DN_LA + px + dx;
                    A += sa[j];
                    B += sb[j];
                    Cc += sc[j];
                }
            const float pc = sp[(py + 2) * DN_LP + px + 2], tc = st[(py + 2) * DN_LP + px + 2], d = pc - tc;
            const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
            const float g = (p.w1 * sgn + 2.f * p.w2 * d - p.w3 * ((A + (2.f * pc * B + tc * Cc)) * inv9)) * p.inv_n;
            const int64_t off = t.gbase + y * p.a.grad_stride[2] + x * p.a.grad_stride[3];
            if (p.a.grad_dtype == NAF_F32)
                static_cast<float*>(p.a.grad)[off] = g;
            else
                static_cast<bf16_t*>(p.a.grad)[off] = (bf16_t)g;
        }
    }
    dn_block_partial(sums, red, static_cast<float*>(p.a.workspace));
}

__global__ __launch_bounds__(DN_THREADS) void denoise_metrics_kernel(const DnParams p) {
    // staged pred | staged target | five row sums [42][32] each | reduction scratch
    __shared__ float smem[2 * DN_MP * DN_MP + 5 * DN_MP * DN_T + 12];
    float* sp = smem;
    float* st = sp + DN_MP * DN_MP;
    float* hs = st + DN_MP * DN_MP;
    float* red = hs + 5 * DN_MP * DN_T;
    constexpr int HQ = DN_MP * DN_T;
    const int tid = threadIdx.x, H = p.a.H, W = p.a.W;
    const DnTile t = dn_tile(p);

    for (int i = tid; i < DN_MP * DN_MP; i += DN_THREADS) {
        const int iy = i / DN_MP, ix = i - iy * DN_MP, y = t.y0 - DN_MH + iy, x = t.x0 - DN_MH + ix;
        float vp = 0.f, vt = 0.f;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            vp = dn_load(p.a.pred, p.a.pred_dtype, t.pbase + y * p.a.pred_stride[2] + x * p.a.pred_stride[3]);
            vt = dn_load(p.a.target, p.a.target_dtype, t.tbase + y * p.a.target_stride[2] + x * p.a.target_stride[3]);
            if (p.a.clamp) vp = fminf(fmaxf(vp, 0.f), 1.f);
        }
        sp[i] = vp;
        st[i] = vt;
    }
    __syncthreads();

    for (int i = tid; i < HQ; i += DN_THREADS) {
        const int iy = i >> 5, ix = i & 31;
        float m1 = 0.f, m2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
#pragma unroll
        for (int k = 0; k < DN_WIN; ++k) {
            const float a = sp[iy * DN_MP + ix + k], b = st[iy * DN_MP + ix + k], g = p.g[k];
            m1 = __builtin_fmaf(g, a, m1);
            m2 = __builtin_fmaf(g, b, m2);
            e11 = __builtin_fmaf(g, a * a, e11);
            e22 = __builtin_fmaf(g, b * b, e22);
            e12 = __builtin_fmaf(g, a * b, e12);
        }
        hs[i] = m1;
        hs[HQ + i] = m2;
        hs[2 * HQ + i] = e11;
        hs[3 * HQ + i] = e22;
        hs[4 * HQ + i] = e12;
    }
    __syncthreads();

    float sums[3] = {0.f, 0.f, 0.f};   // unused, (p - t)^2, S
#pragma unroll
    for (int k4 = 0; k4 < DN_T * DN_T / DN_THREADS; ++k4) {
        const int py = (tid >> 5) + k4 * (DN_THREADS / DN_T), px = tid & 31, y = t.y0 + py, x = t.x0 + px;
        if (y >= H || x >= W) continue;
        float mu1 = 0.f, mu2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
#pragma unroll
        for (int k = 0; k < DN_WIN; ++k) {
            const int j = (py + k) * DN_T + px;
            const float g = p.g[k];
            mu1 = __builtin_fmaf(g, hs[j], mu1);
            mu2 = __builtin_fmaf(g, hs[HQ + j], mu2);
            e11 = __builtin_fmaf(g, hs[2 * HQ + j], e11);
            e22 = __builtin_fmaf(g, hs[3 * HQ + j], e22);
            e12 = __builtin_fmaf(g, hs[4 * HQ + j], e12);
        }
        const float m11 = mu1 * mu1, m22 = mu2 * mu2, m12 = mu1 * mu2;
        const float sg1 = e11 - m11, sg2 = e22 - m22, sg12 = e12 - m12;
        const float S = ((2.f * m12 + DN_C1) * (2.f * sg12 + DN_C2)) / ((m11 + m22 + DN_C1) * (sg1 + sg2 + DN_C2));
        const float d = sp[(py + DN_MH) * DN_MP + px + DN_MH] - st[(py + DN_MH) * DN_MP + px + DN_MH];
        sums[1] = __builtin_fmaf(d, d, sums[1]);
        sums[2] += S;
    }
    dn_block_partial(sums, red, static_cast<float*>(p.a.workspace));
}

// One workgroup: thread i adds partials i, i + 256, ... in fp64, then a binary tree in fp64; thread 0 finishes the scalars.
__global__ __launch_bounds__(DN_THREADS) void denoise_finish_kernel(const f32x4_t* __restrict__ partials, int64_t nblocks, float* __restrict__ out,
                                                                    int mode, double w1, double w2, double w3, double n) {
    __shared__ double sh[3][DN_THREADS];
    const int tid = threadIdx.x;
    double acc[3] = {0.0, 0.0, 0.0};
    for (int64_t i = tid; i < nblocks; i += DN_THREADS) {
        const f32x4_t v = partials[i];
        acc[0] += (double)v[0];
        acc[1] += (double)v[1];
        acc[2] += (double)v[2];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) sh[k][tid] = acc[k];
    __syncthreads();
    for (int s = DN_THREADS / 2; s >= 1; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int k = 0; k < 3; ++k) sh[k][tid] += sh[k][tid + s];
        }
        __syncthreads();
    }
    if (tid != 0) return;
    const double l1 = sh[0][0] / n, l2 = sh[1][0] / n, ss = sh[2][0] / n;
    float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (mode == NAF_DENOISE_LOSS) {
        const double t1 = w1 * l1, t2 = w2 * l2, t3 = w3 * (1.0 - ss);
        o[0] = (float)l1;
        o[1] = (float)l2;
        o[2] = (float)ss;
        o[3] = (float)t1;
        o[4] = (float)t2;
        o[5] = (float)t3;
        o[6] = (float)(t1 + t2 + t3);
    } else {
        o[0] = l2 > 0.0 ? (float)(-10.0 * log10(l2)) : __builtin_inff();
        o[1] = (float)ss;
        o[2] = (float)l2;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) out[k] = o[k];
}

int64_t dn_blocks(const naf_denoise_args* a) {
    const int64_t tx = ((int64_t)a->W + DN_T - 1) / DN_T, ty = ((int64_t)a->H + DN_T - 1) / DN_T;
    return tx * ty * (int64_t)a->B * (int64_t)a->C;
}

bool dn_dtype_ok(int32_t d) { return d == NAF_BF16 || d == NAF_F32; }

}  // namespace

static int denoise_validate(const naf_denoise_args* a) {
    NAF_REQUIRE(a != nullptr, "naf_denoise_objective: args is NULL");
    NAF_REQUIRE(a->pred != nullptr, "naf_denoise_objective: pred is NULL");
    NAF_REQUIRE(a->target != nullptr, "naf_denoise_objective: target is NULL");
    NAF_REQUIRE(a->out != nullptr, "naf_denoise_objective: out is NULL");
    NAF_REQUIRE(a->B >= 1 && a->C >= 1 && a->H >= 1 && a->W >= 1, "naf_denoise_objective: B, C, H and W must be at least 1 (got B=%d C=%d H=%d W=%d)",
                a->B, a->C, a->H, a->W);
    NAF_REQUIRE(a->mode == NAF_DENOISE_LOSS || a->mode == NAF_DENOISE_METRICS, "naf_denoise_objective: unknown mode %d (NAF_DENOISE_LOSS = 0, NAF_DENOISE_METRICS = 1)", a->mode);
    NAF_REQUIRE(dn_dtype_ok(a->pred_dtype), "naf_denoise_objective: unknown pred_dtype %d (NAF_BF16 = 0, NAF_F32 = 1)", a->pred_dtype);
    NAF_REQUIRE(dn_dtype_ok(a->target_dtype), "naf_denoise_objective: unknown target_dtype %d (NAF_BF16 = 0, NAF_F32 = 1)", a->target_dtype);
    NAF_REQUIRE(a->reserved == 0, "naf_denoise_objective: reserved must be 0");
    if (a->mode == NAF_DENOISE_LOSS) {
        NAF_REQUIRE(a->l1_weight >= 0.0 && a->l2_weight >= 0.0 && a->ssim_weight >= 0.0,
                    "naf_denoise_objective: l1_weight, l2_weight and ssim_weight must not be negative (got %g, %g, %g)", a->l1_weight, a->l2_weight, a->ssim_weight);
        NAF_REQUIRE(a->grad == nullptr || dn_dtype_ok(a->grad_dtype), "naf_denoise_objective: unknown grad_dtype %d (NAF_BF16 = 0, NAF_F32 = 1)", a->grad_dtype);
    } else {
        NAF_REQUIRE(a->grad == nullptr, "naf_denoise_objective: grad must be NULL in metrics mode (forward only)");
    }
    if (dn_blocks(a) >= ((int64_t)1 << 24)) {   // 256 threads each: a grid dimension stays below 2^32 threads
        naf_set_error("naf_denoise_objective: %lld tiles of 32 x 32 are not served: below 2^24", (long long)dn_blocks(a));
        return NAF_ERR_UNSUPPORTED;
    }
    NAF_REQUIRE(a->workspace != nullptr, "naf_denoise_objective: workspace is NULL");
    NAF_REQUIRE((reinterpret_cast<uintptr_t>(a->workspace) & 15) == 0, "naf_denoise_objective: workspace must be 16-byte aligned");
    NAF_REQUIRE(a->workspace_bytes >= (size_t)dn_blocks(a) * 16, "naf_denoise_objective: workspace_bytes = %zu, %zu needed (naf_denoise_workspace_bytes)",
                a->workspace_bytes, (size_t)dn_blocks(a) * 16);
    return NAF_OK;
}

extern "C" {

size_t naf_denoise_workspace_bytes(const naf_denoise_args* a) {
    if (a == nullptr || a->B < 1 || a->C < 1 || a->H < 1 || a->W < 1) return 0;
    return (size_t)dn_blocks(a) * 16;
}

int naf_denoise_objective(const naf_denoise_args* a, naf_stream_t stream) {
    const int rc = denoise_validate(a);
    if (rc != NAF_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DnParams p;
    p.a = *a;
    p.tiles_x = (a->W + DN_T - 1) / DN_T;
    p.tiles_y = (a->H + DN_T - 1) / DN_T;
    const double n = (double)a->B * (double)a->C * (double)a->H * (double)a->W;
    p.w1 = (float)a->l1_weight;
    p.w2 = (float)a->l2_weight;
    p.w3 = (float)a->ssim_weight;
    p.inv_n = (float)(1.0 / n);
    {   // the reference's create_window in fp32: exp(-(i - 5)^2 / (2 (11/6)^2)) divided by its sum.  The sum of the eleven fp32 values is taken
        // in fp64 and rounded once, which is what torch's fp32 sum of them returns
        const float denom = (float)(2.0 * (11.0 / 6.0) * (11.0 / 6.0));
        double sum = 0.0;
        for (int i = 0; i < DN_WIN; ++i) {
            const float d = (float)(i - DN_MH);
            p.g[i] = expf(-(d * d) / denom);
            sum += (double)p.g[i];
        }
        for (int i = 0; i < DN_WIN; ++i) p.g[i] /= (float)sum;
    }
    const int64_t nblocks = dn_blocks(a);
    if (a->mode == NAF_DENOISE_LOSS)
        hipLaunchKernelGGL(denoise_loss_kernel, dim3((unsigned)nblocks), dim3(DN_THREADS), 0, s, p);
    else
        hipLaunchKernelGGL(denoise_metrics_kernel, dim3((unsigned)nblocks), dim3(DN_THREADS), 0, s, p);
    const int lrc = naf_check_launch(a->mode == NAF_DENOISE_LOSS ? "denoise_loss_kernel" : "denoise_metrics_kernel");
    if (lrc != NAF_OK) return lrc;
    hipLaunchKernelGGL(denoise_finish_kernel, dim3(1), dim3(DN_THREADS), 0, s, static_cast<const f32x4_t*>(a->workspace), nblocks, a->out, (int)a->mode,
                       a->l1_weight, a->l2_weight, a->ssim_weight, n);
    return naf_check_launch("denoise_finish_kernel");
}

}  // extern "C"
