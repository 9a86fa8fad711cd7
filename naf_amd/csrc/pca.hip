// Feature PCA for display (include/naf_hip.h, naf_feature_moments / naf_pca_project / naf_pca_minmax): the device side of the reference's
// pca() (utils/visualization.py:135-190) -- the second moments of a feature map, its projection on a few components, their minima and maxima.
//
// Decomposition ("Feature PCA"):
//   * moments: a workgroup (4 waves) owns one 128 x 128 block (bi <= bj) of the upper triangle of x^T x for ONE slab of pixels.  Pixel tiles
//     of 32 rows go through LDS as they lie in memory ([pixel][channel], rows past the slab zero-filled, never read); because the channels
//     are the contiguous index, the operand "channel I + r at 8 consecutive pixels" is a transposed LDS read (ds_read_b64_tr_b16), and ONE
//     kind of fragment serves as the A and as the B operand of v_mfma_f32_16x16x32_bf16 -- both agree on the pixel order by construction.
//     Wave (wm, wn) owns the 64 x 64 quarter: 4 + 4 fragments per 16 MFMAs.  On a diagonal block the quarter below the diagonal is skipped,
//     and the waves on the diagonal also multiply their A fragments by a fragment of ones: the column sums, on the same pipe
//   * the fp32 partial block goes to the caller's workspace; feature_moments_finish_kernel adds a block's partials over the slabs in fp64 in
//     slab order and writes an element and its mirror image from the same register: exactly symmetric, no atomics, reproducible bits
//   * bf16 x bf16 is exact in fp32, so the only rounding is the fp32 accumulation over a slab: at most NAF_MOMENTS_CHAIN additions
//   * projection: 16 lanes share one pixel (16-byte chunks k, k + 16, ... of its row), fp32 fused multiply-adds in channel order per lane,
//     a four-step butterfly over the 16 lanes, the bias last.  The workgroup's minima and maxima go to the workspace, a one-workgroup launch
//     finishes them.  fminf / fmaxf are exact, so the order does not matter there
#include "naf_common.h"

#include <math.h>

namespace {

constexpr int FM_BLK = 128;                 // channels per block edge
constexpr int FM_PX = 32;                   // pixels per LDS tile = the k of one MFMA
constexpr int FM_PITCH = FM_BLK + 16;       // row pitch 288 B = 8 banks mod 64: the 4 rows x 32 B a 16-lane group reads per transposed read do not collide
constexpr int FM_THREADS = 256;
constexpr int FM_BLK_ELEMS = FM_BLK * FM_BLK;
constexpr int64_t FM_TARGET_WG = 512;       // workgroups the planner aims for (two per compute unit of an MI355X); a constant, so that the plan depends on P and C alone
constexpr int64_t FM_MIN_SLAB = 256;        // ... without cutting slabs shorter than this

struct FmPlan {
    int nb, T, nsplit;
    int64_t slab;
    size_t bytes;
};

FmPlan fm_plan(int64_t P, int C) {
    FmPlan pl;
    pl.nb = (C + FM_BLK - 1) / FM_BLK;
    pl.T = pl.nb * (pl.nb + 1) / 2;
    const size_t per_split = ((size_t)pl.T * FM_BLK_ELEMS + (size_t)pl.nb * FM_BLK) * sizeof(float);
    const int64_t need = (P + NAF_MOMENTS_CHAIN - 1) / NAF_MOMENTS_CHAIN;                    // the summation contract
    const int64_t want = (FM_TARGET_WG + pl.T - 1) / pl.T, by_px = (P + FM_MIN_SLAB - 1) / FM_MIN_SLAB;
    int64_t ns = want < by_px ? want : by_px;
    const int64_t by_cap = (int64_t)(NAF_MOMENTS_WORKSPACE_CAP / per_split);                 // >= 3 at C = 4096
    if (ns > by_cap) ns = by_cap;
    if (ns < need) ns = need;                                                                // the contract wins over the cap
    int64_t slab = (P + ns - 1) / ns;
    slab = (slab + FM_PX - 1) / FM_PX * FM_PX;
    pl.slab = slab;
    pl.nsplit = (int)((P + slab - 1) / slab);
    pl.bytes = per_split * (size_t)pl.nsplit;
    return pl;
}

struct FmParams {
    const bf16_t* x;
    float* ws;
    int64_t P, ld, slab;
    int32_t C, nb, T, nsplit;
};

// block t of the upper triangle, row by row: (0,0) (0,1) ... (0,nb-1) (1,1) ...
__device__ __forceinline__ void fm_block(int t, int nb, int& bi, int& bj) {
    bi = 0;
    while (t >= nb - bi) {
        t -= nb - bi;
        ++bi;
    }
    bj = bi + t;
}

__global__ __launch_bounds__(FM_THREADS) void feature_moments_kernel(const FmParams p) {
    // [2 buffers][I image | J image][32 px x FM_PITCH]
    __shared__ __attribute__((aligned(16))) bf16_t tile[2 * 2 * FM_PX * FM_PITCH];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    int bi, bj;
    fm_block((int)blockIdx.x, p.nb, bi, bj);
    const int split = blockIdx.y;
    const int I0 = bi * FM_BLK, J0 = bj * FM_BLK;
    const int ci = min(FM_BLK, p.C - I0), cj = min(FM_BLK, p.C - J0);      // multiples of 32
    const bool diag = bi == bj;
    const int64_t q0 = (int64_t)split * p.slab, q1 = q0 + p.slab < p.P ? q0 + p.slab : p.P;
    const int nit = (int)((q1 - q0 + FM_PX - 1) / FM_PX);

    f32x4_t acc[4][4], accs[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        accs[m] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[m][n] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    }
    // operand fragment out of a pixel-major tile: lane (r = lane & 15, kgrp = lane >> 4) gets T[8 kgrp + 0..7][col0 + r]
    const int g = lane >> 4, li = lane & 15;
    const int frag_off = (8 * g + (li >> 2)) * FM_PITCH + (li & 3) * 4;
    auto frag = [&](const bf16_t* img, int col0) __attribute__((always_inline)) {
        const bf16_t* a0 = img + frag_off + col0;
        const bf16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((NAF_LDS bf16x4_t*)a0);
        const bf16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((NAF_LDS bf16x4_t*)(a0 + 4 * FM_PITCH));
        return bf16x8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    };
    const bf16_t one = (bf16_t)1.0f;
    const bf16x8_t ones = {one, one, one, one, one, one, one, one};

    // staging: 32 px x (ci / 8) 16-byte chunks of the I image, and of the J image off the diagonal: at most 2 + 2 items per thread
    const int nchi = ci >> 3, nchj = cj >> 3;
    u32x4_t ireg[2], jreg[2];
    auto issue = [&](int s) __attribute__((always_inline)) {
        const int64_t qs = q0 + (int64_t)s * FM_PX;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int i = k * FM_THREADS + tid;
            ireg[k] = u32x4_t{0u, 0u, 0u, 0u};                  // past the slab: contributes nothing, and is not read
            jreg[k] = u32x4_t{0u, 0u, 0u, 0u};
            if (i < FM_PX * nchi) {
                const int px = i / nchi, ch = i - px * nchi;
                if (qs + px < q1) ireg[k] = *reinterpret_cast<const u32x4_t*>(p.x + (qs + px) * p.ld + I0 + ch * 8);
            }
            if (!diag && i < FM_PX * nchj) {
                const int px = i / nchj, ch = i - px * nchj;
                if (qs + px < q1) jreg[k] = *reinterpret_cast<const u32x4_t*>(p.x + (qs + px) * p.ld + J0 + ch * 8);
            }
        }
    };
    auto commit = [&](int buf) __attribute__((always_inline)) {
        bf16_t* Ib = tile + buf * 2 * FM_PX * FM_PITCH;
        bf16_t* Jb = Ib + FM_PX * FM_PITCH;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int i = k * FM_THREADS + tid;
            if (i < FM_PX * nchi) {
                const int px = i / nchi, ch = i - px * nchi;
                *reinterpret_cast<u32x4_t*>(Ib + px * FM_PITCH + ch * 8) = ireg[k];
            }
            if (!diag && i < FM_PX * nchj) {
                const int px = i / nchj, ch = i - px * nchj;
                *reinterpret_cast<u32x4_t*>(Jb + px * FM_PITCH + ch * 8) = jreg[k];
            }
        }
    };
    const bool work = !(diag && wm > wn);                       // wave-uniform: the quarter below the diagonal is the mirror image
    const bool sums = diag && wm == wn;
    if (nit > 0) {
        issue(0);
        commit(0);
        __syncthreads();
    }
    for (int s = 0; s < nit; ++s) {
        const int buf = s & 1;
        const bf16_t* Ib = tile + buf * 2 * FM_PX * FM_PITCH;
        const bf16_t* Jb = diag ? Ib : Ib + FM_PX * FM_PITCH;
        if (s + 1 < nit) issue(s + 1);
        if (work) {
            bf16x8_t fa[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int c0 = (wm * 4 + m) * 16;
                fa[m] = ones;
                if (c0 < ci) fa[m] = frag(Ib, c0);              // block-uniform
            }
            if (sums) {
#pragma unroll
                for (int m = 0; m < 4; ++m)
                    if ((wm * 4 + m) * 16 < ci) accs[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[m], ones, accs[m], 0, 0, 0);
            }
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const int c1 = (wn * 4 + n) * 16;
                if (c1 >= cj) continue;
                const bf16x8_t fb = frag(Jb, c1);
#pragma unroll
                for (int m = 0; m < 4; ++m)
                    if ((wm * 4 + m) * 16 < ci) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[m], fb, acc[m][n], 0, 0, 0);
            }
        }
        if (s + 1 < nit) commit(buf ^ 1);                       // the other buffer: its readers finished before the barrier of the step before
        __syncthreads();
    }
    if (!work) return;
    // D[i = 4 (lane >> 4) + r][j = lane & 15] of tile (m, n) -> the block's [128][128] partial
    float* blk = p.ws + ((size_t)split * p.T + blockIdx.x) * FM_BLK_ELEMS;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        if ((wm * 4 + m) * 16 >= ci) continue;
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            if ((wn * 4 + n) * 16 >= cj) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) blk[((wm * 4 + m) * 16 + 4 * g + r) * FM_BLK + (wn * 4 + n) * 16 + li] = acc[m][n][r];
        }
    }
    if (sums && li == 0) {
        float* sb = p.ws + (size_t)p.nsplit * p.T * FM_BLK_ELEMS + ((size_t)split * p.nb + bi) * FM_BLK;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            if ((wm * 4 + m) * 16 >= ci) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) sb[(wm * 4 + m) * 16 + 4 * g + r] = accs[m][r];
        }
    }
}

// Workgroups [0, 64 T): one element of one block each thread, the slabs added in fp64 in slab order, the element and its mirror image written
// from one register.  Workgroups [64 T, 64 T + nb): the channel sums.
__global__ __launch_bounds__(FM_THREADS) void feature_moments_finish_kernel(const float* __restrict__ ws, double* __restrict__ gram,
                                                                            double* __restrict__ sum, int C, int nb, int T, int nsplit) {
    const int tid = threadIdx.x;
    const int wg = blockIdx.x;
    if (wg < 64 * T) {
        const int t = wg >> 6, e = (wg & 63) * FM_THREADS + tid;
        int bi, bj;
        fm_block(t, nb, bi, bj);
        const int i = bi * FM_BLK + (e >> 7), j = bj * FM_BLK + (e & 127);
        if (i >= C || j >= C || i > j) return;
        double acc = 0.0;
        for (int s = 0; s < nsplit; ++s) acc += (double)ws[((size_t)s * T + t) * FM_BLK_ELEMS + e];
        gram[(size_t)i * C + j] = acc;
        gram[(size_t)j * C + i] = acc;
    } else {
        const int bi = wg - 64 * T, i = bi * FM_BLK + tid;
        if (tid >= FM_BLK || i >= C) return;
        const float* sb = ws + (size_t)nsplit * T * FM_BLK_ELEMS;
        double acc = 0.0;
        for (int s = 0; s < nsplit; ++s) acc += (double)sb[((size_t)s * nb + bi) * FM_BLK + tid];
        sum[i] = acc;
    }
}

// ---- projection and min-max ----
constexpr int PJ_THREADS = 256;
constexpr int PJ_GROUP = 16;                          // lanes per pixel
constexpr int PJ_PIX = PJ_THREADS / PJ_GROUP;         // pixels per workgroup and step
constexpr int PJ_MAX_N = 8;
constexpr int64_t PJ_MAX_WG = 1024;
constexpr size_t PJ_LINE = 2 * PJ_MAX_N * sizeof(float);   // one workgroup's minima and maxima

struct PjPlan {
    int64_t nwg, ppw;
};
PjPlan pj_plan(int64_t P) {
    PjPlan pl;
    int64_t nwg = (P + PJ_PIX - 1) / PJ_PIX;
    if (nwg > PJ_MAX_WG) nwg = PJ_MAX_WG;
    pl.ppw = ((P + nwg - 1) / nwg + PJ_PIX - 1) / PJ_PIX * PJ_PIX;
    pl.nwg = (P + pl.ppw - 1) / pl.ppw;
    return pl;
}

// The workgroup's minimum and maximum of each of mn[0..n), mx[0..n): thread r < n writes the pair to line `line` of the workspace.
__device__ __forceinline__ void pj_block_minmax(float (&mn)[PJ_MAX_N], float (&mx)[PJ_MAX_N], int n, float* ws, int64_t line) {
    __shared__ float red[PJ_THREADS / 64][2 * PJ_MAX_N];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
#pragma unroll
    for (int r = 0; r < PJ_MAX_N; ++r) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            mn[r] = fminf(mn[r], __shfl_xor(mn[r], off, 64));
            mx[r] = fmaxf(mx[r], __shfl_xor(mx[r], off, 64));
        }
        if (lane == 0) {
            red[wv][r] = mn[r];
            red[wv][PJ_MAX_N + r] = mx[r];
        }
    }
    __syncthreads();
    if (tid < n) {
        ws[line * (2 * PJ_MAX_N) + tid] = fminf(fminf(red[0][tid], red[1][tid]), fminf(red[2][tid], red[3][tid]));
        ws[line * (2 * PJ_MAX_N) + PJ_MAX_N + tid] =
            fmaxf(fmaxf(red[0][PJ_MAX_N + tid], red[1][PJ_MAX_N + tid]), fmaxf(red[2][PJ_MAX_N + tid], red[3][PJ_MAX_N + tid]));
    }
}

template <int N>
__global__ __launch_bounds__(PJ_THREADS) void pca_project_kernel(const bf16_t* __restrict__ x, const float* __restrict__ V, const float* __restrict__ b,
                                                                 float* __restrict__ y, float* __restrict__ ws, int64_t P, int64_t ld, int C,
                                                                 int64_t ppw) {
    const int tid = threadIdx.x, grp = tid >> 4, gl = tid & 15;
    const int64_t q0 = (int64_t)blockIdx.x * ppw, q1 = q0 + ppw < P ? q0 + ppw : P;
    const int nch = C >> 3;
    float mn[PJ_MAX_N], mx[PJ_MAX_N];
#pragma unroll
    for (int r = 0; r < PJ_MAX_N; ++r) {
        mn[r] = __builtin_inff();
        mx[r] = -__builtin_inff();
    }
    for (int64_t base = q0; base < q1; base += PJ_PIX) {      // workgroup-uniform trip count: the butterfly below needs every lane
        const int64_t q = base + grp;
        const bool valid = q < q1;
        float acc[N];
#pragma unroll
        for (int r = 0; r < N; ++r) acc[r] = 0.f;
        if (valid) {
            const bf16_t* row = x + q * ld;
            for (int ch = gl; ch < nch; ch += PJ_GROUP) {
                const bf16x8_t v = *reinterpret_cast<const bf16x8_t*>(row + ch * 8);
                const float* vc = V + (size_t)ch * 8 * N;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float xf = (float)v[e];
#pragma unroll
                    for (int r = 0; r < N; ++r) acc[r] = __builtin_fmaf(xf, vc[e * N + r], acc[r]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < N; ++r) {
#pragma unroll
            for (int off = 8; off >= 1; off >>= 1) acc[r] += __shfl_xor(acc[r], off, 64);
        }
        if (valid && gl == 0) {
#pragma unroll
            for (int r = 0; r < N; ++r) {
                const float o = acc[r] + b[r];
                y[q * N + r] = o;
                mn[r] = fminf(mn[r], o);
                mx[r] = fmaxf(mx[r], o);
            }
        }
    }
    pj_block_minmax(mn, mx, N, ws, blockIdx.x);
}

__global__ __launch_bounds__(PJ_THREADS) void pca_minmax_kernel(const float* __restrict__ y, float* __restrict__ ws, int64_t P, int64_t ld, int n,
                                                                int64_t ppw) {
    const int64_t q0 = (int64_t)blockIdx.x * ppw, q1 = q0 + ppw < P ? q0 + ppw : P;
    float mn[PJ_MAX_N], mx[PJ_MAX_N];
#pragma unroll
    for (int r = 0; r < PJ_MAX_N; ++r) {
        mn[r] = __builtin_inff();
        mx[r] = -__builtin_inff();
    }
    for (int64_t q = q0 + threadIdx.x; q < q1; q += PJ_THREADS) {
#pragma unroll
        for (int r = 0; r < PJ_MAX_N; ++r) {
            if (r < n) {
                const float o = y[q * ld + r];
                mn[r] = fminf(mn[r], o);
                mx[r] = fmaxf(mx[r], o);
            }
        }
    }
    pj_block_minmax(mn, mx, n, ws, blockIdx.x);
}

// One workgroup: the partial lines [0, nlines) of the workspace -> minmax[2][n]
__global__ __launch_bounds__(PJ_THREADS) void pca_minmax_finish_kernel(const float* __restrict__ ws, int64_t nlines, float* __restrict__ minmax, int n) {
    __shared__ float out[2 * PJ_MAX_N];
    float mn[PJ_MAX_N], mx[PJ_MAX_N];
#pragma unroll
    for (int r = 0; r < PJ_MAX_N; ++r) {
        mn[r] = __builtin_inff();
        mx[r] = -__builtin_inff();
    }
    for (int64_t i = threadIdx.x; i < nlines; i += PJ_THREADS) {
#pragma unroll
        for (int r = 0; r < PJ_MAX_N; ++r) {
            if (r < n) {
                mn[r] = fminf(mn[r], ws[i * (2 * PJ_MAX_N) + r]);
                mx[r] = fmaxf(mx[r], ws[i * (2 * PJ_MAX_N) + PJ_MAX_N + r]);
            }
        }
    }
    pj_block_minmax(mn, mx, n, out, 0);
    __syncthreads();
    if ((int)threadIdx.x < n) {
        minmax[threadIdx.x] = out[threadIdx.x];
        minmax[n + threadIdx.x] = out[PJ_MAX_N + threadIdx.x];
    }
}


// NAF_OK, NAF_ERR_INVALID or NAF_ERR_UNSUPPORTED from the scalar fields alone
int fm_check_scalars(const naf_feature_moments_args* a, const char* who) {
    NAF_REQUIRE(a != nullptr, "%s: args is NULL", who);
    NAF_REQUIRE(a->reserved == 0, "%s: reserved must be 0", who);
    NAF_REQUIRE(a->P >= 1 && a->C >= 1, "%s: P and C must be at least 1 (got P=%lld C=%d)", who, (long long)a->P, a->C);
    NAF_REQUIRE(a->ld >= a->C && a->ld % 8 == 0, "%s: ld = %lld: the row stride must be at least C = %d and a multiple of 8 elements", who,
                (long long)a->ld, a->C);
    if (a->C % 32 != 0 || a->C < 32 || a->C > NAF_PCA_MAX_C) {
        naf_set_error("%s: C = %d is not served: C %% 32 == 0 and 32 <= C <= %d", who, a->C, NAF_PCA_MAX_C);
        return NAF_ERR_UNSUPPORTED;
    }
    if (a->P > ((int64_t)1 << 31) - 1) {
        naf_set_error("%s: P = %lld is not served: below 2^31 pixels", who, (long long)a->P);
        return NAF_ERR_UNSUPPORTED;
    }
    return NAF_OK;
}

int pj_check_scalars(int64_t P, int64_t ld, int64_t ld_min, int n, int32_t r0, int32_t r1, const char* who) {
    NAF_REQUIRE(r0 == 0 && r1 == 0, "%s: reserved must be 0", who);
    NAF_REQUIRE(P >= 1 && n >= 1, "%s: P and n must be at least 1 (got P=%lld n=%d)", who, (long long)P, n);
    NAF_REQUIRE(ld >= ld_min, "%s: ld = %lld: the row stride must be at least %lld elements", who, (long long)ld, (long long)ld_min);
    if (n > NAF_PCA_MAX_COMPONENTS) {
        naf_set_error("%s: n = %d is not served: 1 <= n <= %d components", who, n, NAF_PCA_MAX_COMPONENTS);
        return NAF_ERR_UNSUPPORTED;
    }
    if (P > ((int64_t)1 << 31) - 1) {
        naf_set_error("%s: P = %lld is not served: below 2^31 pixels", who, (long long)P);
        return NAF_ERR_UNSUPPORTED;
    }
    return NAF_OK;
}

template <int N>
void pj_launch(const naf_pca_project_args* a, const PjPlan& pl, hipStream_t s) {
    hipLaunchKernelGGL(pca_project_kernel<N>, dim3((unsigned)pl.nwg), dim3(PJ_THREADS), 0, s, static_cast<const bf16_t*>(a->x), a->V, a->b, a->y,
                       static_cast<float*>(a->workspace), a->P, a->ld, (int)a->C, pl.ppw);
}

}  // namespace

extern "C" {

int naf_feature_moments_plan(const naf_feature_moments_args* a, int32_t* nsplit, int32_t* slab_pixels) {
    const int rc = fm_check_scalars(a, "naf_feature_moments_plan");
    if (rc != NAF_OK) return rc;
    NAF_REQUIRE(nsplit != nullptr && slab_pixels != nullptr, "naf_feature_moments_plan: nsplit or slab_pixels is NULL");
    const FmPlan pl = fm_plan(a->P, a->C);
    *nsplit = pl.nsplit;
    *slab_pixels = (int32_t)pl.slab;
    return NAF_OK;
}

size_t naf_feature_moments_workspace_bytes(const naf_feature_moments_args* a) {
    if (a == nullptr || a->P < 1 || a->P > ((int64_t)1 << 31) - 1 || a->C < 32 || a->C > NAF_PCA_MAX_C || a->C % 32 != 0) return 0;
    return fm_plan(a->P, a->C).bytes;
}

int naf_feature_moments(const naf_feature_moments_args* a, naf_stream_t stream) {
    const char* who = "naf_feature_moments";
    const int rc = fm_check_scalars(a, who);
    if (rc != NAF_OK) return rc;
    NAF_REQUIRE(a->x != nullptr, "%s: x is NULL", who);
    NAF_REQUIRE(a->gram != nullptr, "%s: gram is NULL", who);
    NAF_REQUIRE(a->sum != nullptr, "%s: sum is NULL", who);
    NAF_REQUIRE(a->workspace != nullptr, "%s: workspace is NULL", who);
    NAF_REQUIRE(naf_aligned(a->x, 16), "%s: x must be 16-byte aligned", who);
    NAF_REQUIRE(naf_aligned(a->gram, 8) && naf_aligned(a->sum, 8), "%s: gram and sum must be 8-byte aligned", who);
    NAF_REQUIRE(naf_aligned(a->workspace, 16), "%s: workspace must be 16-byte aligned", who);
    const FmPlan pl = fm_plan(a->P, a->C);
    NAF_REQUIRE(a->workspace_bytes >= pl.bytes, "%s: workspace_bytes = %zu, %zu needed (naf_feature_moments_workspace_bytes)", who, a->workspace_bytes,
                pl.bytes);
    hipStream_t s = static_cast<hipStream_t>(stream);
    FmParams p;
    p.x = static_cast<const bf16_t*>(a->x);
    p.ws = static_cast<float*>(a->workspace);
    p.P = a->P;
    p.ld = a->ld;
    p.slab = pl.slab;
    p.C = a->C;
    p.nb = pl.nb;
    p.T = pl.T;
    p.nsplit = pl.nsplit;
    hipLaunchKernelGGL(feature_moments_kernel, dim3((unsigned)pl.T, (unsigned)pl.nsplit), dim3(FM_THREADS), 0, s, p);
    const int lrc = naf_check_launch("feature_moments_kernel");
    if (lrc != NAF_OK) return lrc;
    hipLaunchKernelGGL(feature_moments_finish_kernel, dim3((unsigned)(64 * pl.T + pl.nb)), dim3(FM_THREADS), 0, s, p.ws, a->gram, a->sum, (int)a->C, pl.nb,
                       pl.T, pl.nsplit);
    return naf_check_launch("feature_moments_finish_kernel");
}

size_t naf_pca_project_workspace_bytes(const naf_pca_project_args* a) {
    if (a == nullptr || a->P < 1 || a->P > ((int64_t)1 << 31) - 1) return 0;
    return (size_t)pj_plan(a->P).nwg * PJ_LINE;
}

int naf_pca_project(const naf_pca_project_args* a, naf_stream_t stream) {
    const char* who = "naf_pca_project";
    NAF_REQUIRE(a != nullptr, "%s: args is NULL", who);
    NAF_REQUIRE(a->C >= 1, "%s: C must be at least 1 (got %d)", who, a->C);
    const int rc = pj_check_scalars(a->P, a->ld, a->C, a->n, a->reserved[0], a->reserved[1], who);
    if (rc != NAF_OK) return rc;
    NAF_REQUIRE(a->ld % 8 == 0, "%s: ld = %lld: the row stride must be a multiple of 8 elements", who, (long long)a->ld);
    if (a->C % 32 != 0 || a->C < 32 || a->C > NAF_PCA_MAX_C) {
        naf_set_error("%s: C = %d is not served: C %% 32 == 0 and 32 <= C <= %d", who, a->C, NAF_PCA_MAX_C);
        return NAF_ERR_UNSUPPORTED;
    }
    NAF_REQUIRE(a->x != nullptr, "%s: x is NULL", who);
    NAF_REQUIRE(a->V != nullptr, "%s: V is NULL", who);
    NAF_REQUIRE(a->b != nullptr, "%s: b is NULL", who);
    NAF_REQUIRE(a->y != nullptr, "%s: y is NULL", who);
    NAF_REQUIRE(a->minmax != nullptr, "%s: minmax is NULL", who);
    NAF_REQUIRE(a->workspace != nullptr, "%s: workspace is NULL", who);
    NAF_REQUIRE(naf_aligned(a->x, 16), "%s: x must be 16-byte aligned", who);
    NAF_REQUIRE(naf_aligned(a->V, 4) && naf_aligned(a->b, 4) && naf_aligned(a->y, 4) && naf_aligned(a->minmax, 4), "%s: V, b, y and minmax must be 4-byte aligned",
                who);
    NAF_REQUIRE(naf_aligned(a->workspace, 16), "%s: workspace must be 16-byte aligned", who);
    const PjPlan pl = pj_plan(a->P);
    NAF_REQUIRE(a->workspace_bytes >= (size_t)pl.nwg * PJ_LINE, "%s: workspace_bytes = %zu, %zu needed (naf_pca_project_workspace_bytes)", who,
                a->workspace_bytes, (size_t)pl.nwg * PJ_LINE);
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (a->n) {
        case 1: pj_launch<1>(a, pl, s); break;
        case 2: pj_launch<2>(a, pl, s); break;
        case 3: pj_launch<3>(a, pl, s); break;
        case 4: pj_launch<4>(a, pl, s); break;
        case 5: pj_launch<5>(a, pl, s); break;
        case 6: pj_launch<6>(a, pl, s); break;
        case 7: pj_launch<7>(a, pl, s); break;
        default: pj_launch<8>(a, pl, s); break;
    }
    const int lrc = naf_check_launch("pca_project_kernel");
    if (lrc != NAF_OK) return lrc;
    hipLaunchKernelGGL(pca_minmax_finish_kernel, dim3(1), dim3(PJ_THREADS), 0, s, static_cast<const float*>(a->workspace), pl.nwg, a->minmax, (int)a->n);
    return naf_check_launch("pca_minmax_finish_kernel");
}

int naf_pca_minmax(const naf_pca_minmax_args* a, naf_stream_t stream) {
    const char* who = "naf_pca_minmax";
    NAF_REQUIRE(a != nullptr, "%s: args is NULL", who);
    const int rc = pj_check_scalars(a->P, a->ld, a->n, a->n, a->reserved, 0, who);
    if (rc != NAF_OK) return rc;
    NAF_REQUIRE(a->y != nullptr, "%s: y is NULL", who);
    NAF_REQUIRE(a->minmax != nullptr, "%s: minmax is NULL", who);
    NAF_REQUIRE(a->workspace != nullptr, "%s: workspace is NULL", who);
    NAF_REQUIRE(naf_aligned(a->y, 4) && naf_aligned(a->minmax, 4), "%s: y and minmax must be 4-byte aligned", who);
    NAF_REQUIRE(naf_aligned(a->workspace, 16), "%s: workspace must be 16-byte aligned", who);
    const PjPlan pl = pj_plan(a->P);
    NAF_REQUIRE(a->workspace_bytes >= (size_t)pl.nwg * PJ_LINE, "%s: workspace_bytes = %zu, %zu needed (naf_pca_project_workspace_bytes of the same P)", who,
                a->workspace_bytes, (size_t)pl.nwg * PJ_LINE);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(pca_minmax_kernel, dim3((unsigned)pl.nwg), dim3(PJ_THREADS), 0, s, a->y, static_cast<float*>(a->workspace), a->P, a->ld, (int)a->n, pl.ppw);
    const int lrc = naf_check_launch("pca_minmax_kernel");
    if (lrc != NAF_OK) return lrc;
    hipLaunchKernelGGL(pca_minmax_finish_kernel, dim3(1), dim3(PJ_THREADS), 0, s, static_cast<const float*>(a->workspace), pl.nwg, a->minmax, (int)a->n);
    return naf_check_launch("pca_minmax_finish_kernel");
}

}  // extern "C"
