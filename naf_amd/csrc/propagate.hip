// Label propagation (include/naf_hip.h, naf_propagate_fwd): a windowed top-k affinity over a queue of context frames, with the affinity
// tensor never written.  Replaces label_propagation of the reference (evaluation/eval_video_seg.py:499-561) after feature extraction.
//
// Decomposition ("Label propagation"):
//   * one workgroup (4 waves) owns an 8 x 16 tile of target pixels for ALL context frames; wave v owns tile rows 2v and 2v+1, and keeps its
//     32 queries in registers as the MFMA B operand (C/32 fragments of 8 bf16 per 16-query row)
//   * the key rows of the tile's halo (16 + 2r columns, rounded up to 16-key blocks) stream through LDS, frame after frame, double-buffered
//     where two rows fit; a wave skips the rows outside its own queries' windows
//   * per key block one 16 x 16 tile of raw dot products (v_mfma_f32_16x16x32_bf16, keys as rows, queries as columns: a lane holds 4 keys of
//     ONE query), scaled by the two inverse norms and masked to the query's clipped window
//   * TWO passes over the keys in one launch.  Pass 1 keeps each query's topk largest scores (a sorted register list per lane, the four lanes
//     that share a query merge theirs at the end).  Pass 2 recomputes the scores -- the same instructions on the same data, so bit for bit the
//     same values -- and accumulates every candidate with s >= threshold: ties at the threshold are all kept, however many there are
//   * the label maps are gathered for kept candidates only; the sums live in LDS, one row per query, and the four lanes of a query add in a
//     fixed order (no atomics): the output is bit-reproducible
#include "naf_common.h"

namespace {

constexpr int PT_H = 8, PT_W = 16, PT_Q = PT_H * PT_W;   // the query tile
constexpr int PTK = 16;                                   // list slots (the served topk limit)
constexpr int PROP_LDS_MAX = 160 * 1024;

struct PropParams {
    naf_propagate_args a;
    int nkb;        // 16-key blocks per halo row
    int kstride;    // bytes between two keys of a row in LDS (2C + 16: consecutive keys start 4 banks apart)
    int nbuf;       // 2: the next row loads while this one is multiplied; 1 where two rows do not fit
    int tiles_x;
    float inv_t;
};

__device__ __forceinline__ void list_insert(float (&a)[PTK], float v) {
#pragma unroll
    for (int i = 0; i < PTK; ++i) {
        const float hi = fmaxf(a[i], v), lo = fminf(a[i], v);
        a[i] = hi;
        v = lo;
    }
}

template <int KSMAX>
__global__ __launch_bounds__(256) void propagate_kernel(const PropParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_pp[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int C = p.a.C, h = p.a.h, w = p.a.w, r = p.a.radius, K = p.a.K, topk = p.a.topk;
    const int nks = C >> 5, c8n = C >> 3, nkeys = p.nkb * 16;
    const int x0 = (int)(blockIdx.x % (uint32_t)p.tiles_x) * PT_W, y0 = (int)(blockIdx.x / (uint32_t)p.tiles_x) * PT_H;
    const int kx0 = x0 - r;

    // LDS: sums [128][K + 1] (slot K: the denominator) | inverse norms [nbuf][nkeys] | key rows [nbuf][nkeys][kstride bytes]
    float* acc = reinterpret_cast<float*>(smem_pp);
    float* invk = acc + ((PT_Q * (K + 1) + 3) & ~3);
    unsigned char* keys = reinterpret_cast<unsigned char*>(invk + p.nbuf * nkeys);
    const size_t bufbytes = (size_t)nkeys * p.kstride;
    for (int i = tid; i < PT_Q * (K + 1); i += 256) acc[i] = 0.f;

    // ---- the wave's 32 queries, stationary ----
    bf16x8_t qf[2][KSMAX];
    float invq[2];
    int qy[2];
    const int qx = x0 + l15;
    const bool qx_ok = qx < w;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        qy[u] = y0 + 2 * wv + u;
        const size_t pix = (size_t)min(qy[u], h - 1) * w + min(qx, w - 1);
        const bf16_t* qp = static_cast<const bf16_t*>(p.a.target) + pix * C + l4 * 8;
#pragma unroll
        for (int ks = 0; ks < KSMAX; ++ks)
            if (ks < nks) qf[u][ks] = *reinterpret_cast<const bf16x8_t*>(qp + ks * 32);
        invq[u] = p.a.target_inv[pix];
    }

    const int ylo = max(0, y0 - r), yhi = min(h - 1, y0 + PT_H - 1 + r), rows = yhi - ylo + 1, T = p.a.n * rows;

    auto load_row = [&](int it, int buf) {
        const int f = it / rows, y = ylo + it % rows;
        const bf16_t* src = static_cast<const bf16_t*>(p.a.context[f]) + (size_t)y * w * C;
        unsigned char* dst = keys + buf * bufbytes;
        for (int idx = tid; idx < nkeys * c8n; idx += 256) {
            const int j = idx / c8n, c8 = idx - j * c8n, x = kx0 + j;
            u32x4_t v = {0u, 0u, 0u, 0u};
            if (x >= 0 && x < w) v = *reinterpret_cast<const u32x4_t*>(src + (size_t)x * C + c8 * 8);
            *reinterpret_cast<u32x4_t*>(dst + (size_t)j * p.kstride + c8 * 16) = v;
        }
        if (tid < nkeys) {
            const int x = kx0 + tid;
            invk[buf * nkeys + tid] = (x >= 0 && x < w) ? p.a.context_inv[f][(size_t)y * w + x] : 0.f;
        }
    };

    // scores of key block kb of the row in `buf` against query row u: s[reg] belongs to key kb*16 + 4*l4 + reg and query l15
    auto scores = [&](int buf, int u, int kb) -> f32x4_t {
        f32x4_t s = {0.f, 0.f, 0.f, 0.f};
        const unsigned char* kp = keys + buf * bufbytes + (size_t)(kb * 16 + l15) * p.kstride + l4 * 16;
#pragma unroll
        for (int ks = 0; ks < KSMAX; ++ks)
            if (ks < nks) s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8_t*>(kp + ks * 64), qf[u][ks], s, 0, 0, 0);
        const float* ik = invk + buf * nkeys + kb * 16 + l4 * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] = (s[i] * invq[u]) * ik[i];
        return s;
    };
    auto row_in_window = [&](int u, int y) { return qy[u] < h && y >= qy[u] - r && y <= qy[u] + r; };        // wave-uniform
    auto block_in_image = [&](int kb) { return kx0 + kb * 16 + 15 >= 0 && kx0 + kb * 16 < w; };              // wave-uniform
    auto key_in_window = [&](int kb, int i) {
        const int x = kx0 + kb * 16 + l4 * 4 + i;
        return qx_ok && x >= 0 && x < w && x >= qx - r && x <= qx + r;
    };

    // ---- pass 1: each query's topk largest scores.  Slots [0, 16 - topk) hold +inf and never move; slot 15 is the running threshold ----
    float lst[2][PTK];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int i = 0; i < PTK; ++i) lst[u][i] = (i < PTK - topk) ? __builtin_inff() : -__builtin_inff();

    load_row(0, 0);
    __syncthreads();
    for (int it = 0; it < T; ++it) {
        const int buf = p.nbuf == 2 ? (it & 1) : 0;
        if (p.nbuf == 2 && it + 1 < T) load_row(it + 1, buf ^ 1);
        const int y = ylo + it % rows;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (!row_in_window(u, y)) continue;
            for (int kb = 0; kb < p.nkb; ++kb) {
                if (!block_in_image(kb)) continue;
                const f32x4_t s = scores(buf, u, kb);
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (key_in_window(kb, i) && s[i] > lst[u][PTK - 1]) list_insert(lst[u], s[i]);
            }
        }
        __syncthreads();
        if (p.nbuf == 1 && it + 1 < T) {
            load_row(it + 1, 0);
            __syncthreads();
        }
    }

    // the four lanes of a query (l, l^16, l^32, l^48) merge their lists: afterwards all four hold the query's topk largest
    float theta[2], smax[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        float own[PTK];
#pragma unroll
        for (int i = 0; i < PTK; ++i) own[i] = lst[u][i];
#pragma unroll
        for (int off = 16; off < 64; off += 16)
#pragma unroll
            for (int i = 0; i < PTK; ++i) {
                const float v = __shfl_xor(own[i], off, 64);
                if (i >= PTK - topk) list_insert(lst[u], v);
            }
        theta[u] = lst[u][PTK - 1];      // -inf with fewer than topk candidates: all of them are kept
        float m = -__builtin_inff();
#pragma unroll
        for (int i = 0; i < PTK; ++i)
            if (i == PTK - topk) m = lst[u][i];
        smax[u] = m;
    }

    // ---- pass 2: the same scores again; every candidate with s >= threshold adds w * segs to its query's sums ----
    load_row(0, 0);
    __syncthreads();
    for (int it = 0; it < T; ++it) {
        const int buf = p.nbuf == 2 ? (it & 1) : 0;
        if (p.nbuf == 2 && it + 1 < T) load_row(it + 1, buf ^ 1);
        const int f = it / rows, y = ylo + it % rows;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (!row_in_window(u, y)) continue;
            for (int kb = 0; kb < p.nkb; ++kb) {
                if (!block_in_image(kb)) continue;
                const f32x4_t s = scores(buf, u, kb);
                uint32_t kept = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (key_in_window(kb, i) && s[i] >= theta[u]) kept |= 1u << i;
                if (__any(kept != 0)) {
                    // rare (about topk of the (2r+1)^2 * n candidates).  The four lanes of a query take turns, lowest keys first.
                    float* ac = acc + ((2 * wv + u) * PT_W + l15) * (K + 1);
                    for (int turn = 0; turn < 4; ++turn) {
                        if (turn == l4 && kept != 0) {
                            for (int i = 0; i < 4; ++i) {
                                if (!((kept >> i) & 1u)) continue;
                                const float wgt = expf((s[i] - smax[u]) * p.inv_t);
                                const int x = kx0 + kb * 16 + l4 * 4 + i;
                                const float* sg = p.a.segs + (((size_t)f * h + y) * w + x) * K;
                                for (int k = 0; k < K; ++k) ac[k] += wgt * sg[k];
                                ac[K] += wgt;
                            }
                        }
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    }
                }
            }
        }
        __syncthreads();
        if (p.nbuf == 1 && it + 1 < T) {
            load_row(it + 1, 0);
            __syncthreads();
        }
    }

    // ---- out[k][p] = sum / denominator (>= 1: the largest score's weight is exp(0)) ----
    for (int idx = tid; idx < PT_Q * K; idx += 256) {
        const int k = idx / PT_Q, q = idx % PT_Q, oy = y0 + q / PT_W, ox = x0 + q % PT_W;
        if (oy < h && ox < w) p.a.out[((size_t)k * h + oy) * w + ox] = acc[q * (K + 1) + k] / acc[q * (K + 1) + K];
    }
}

// one 16-lane row of a wave per pixel: 16 bytes per lane and step, fp32 sum of squares
__global__ __launch_bounds__(256) void inv_norm_kernel(const bf16_t* __restrict__ x, float* __restrict__ inv, int64_t npix, int C) {
    const int64_t pix = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    const int l = threadIdx.x & 15;
    float ss = 0.f;
    if (pix < npix) {
        const bf16_t* px = x + pix * C;
        for (int c = l * 8; c < C; c += 128) {
            const bf16x8_t v = *reinterpret_cast<const bf16x8_t*>(px + c);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float f = (float)v[j];
                ss = __builtin_fmaf(f, f, ss);
            }
        }
    }
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) ss += __shfl_xor(ss, off, 16);
    if (pix < npix && l == 0) inv[pix] = 1.f / fmaxf(sqrtf(ss), 1e-12f);
}

size_t prop_lds(const naf_propagate_args* a, int nkb, int kstride, int nbuf) {
    const size_t accf = (size_t)((PT_Q * (a->K + 1) + 3) & ~3);
    return (accf + (size_t)nbuf * nkb * 16) * sizeof(float) + (size_t)nbuf * nkb * 16 * kstride;
}

template <int KSMAX>
int launch_ks(const PropParams& p, size_t lds, int grid, hipStream_t s) {
    auto kern = propagate_kernel<KSMAX>;
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, PROP_LDS_MAX);
    if (attr != hipSuccess) {
        naf_set_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize): %s", hipGetErrorString(attr));
        return NAF_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, s, p);
    return naf_check_launch("propagate_kernel");
}

}  // namespace

// The launch's choices from the scalar fields alone (host only): naf_propagate_plan reports them, naf_launch_propagate takes them from here.
struct PropPlan {
    int ksmax, nkb, kstride, nbuf;
    size_t lds;
};

static int prop_plan(const naf_propagate_args* a, PropPlan* pl) {
    pl->nkb = (PT_W + 2 * a->radius + 15) / 16;
    pl->kstride = 2 * a->C + 16;
    pl->nbuf = prop_lds(a, pl->nkb, pl->kstride, 2) <= (size_t)PROP_LDS_MAX ? 2 : 1;
    pl->lds = prop_lds(a, pl->nkb, pl->kstride, pl->nbuf);
    if (pl->lds > (size_t)PROP_LDS_MAX) {
        naf_set_error("naf_propagate_fwd: %zu bytes of LDS needed, %d available", pl->lds, PROP_LDS_MAX);
        return NAF_ERR_UNSUPPORTED;
    }
    const int nks = a->C / 32;
    pl->ksmax = nks <= 4 ? 4 : nks <= 8 ? 8 : nks <= 12 ? 12 : nks <= 16 ? 16 : nks <= 24 ? 24 : 32;
    return NAF_OK;
}

static int naf_launch_propagate(const naf_propagate_args* a, hipStream_t s) {
    PropPlan pl;
    const int rc = prop_plan(a, &pl);
    if (rc != NAF_OK) return rc;
    PropParams p;
    p.a = *a;
    p.nkb = pl.nkb;
    p.kstride = pl.kstride;
    p.nbuf = pl.nbuf;
    p.tiles_x = (a->w + PT_W - 1) / PT_W;
    p.inv_t = 1.f / a->temperature;
    const int64_t grid = (int64_t)p.tiles_x * ((a->h + PT_H - 1) / PT_H);
    switch (pl.ksmax) {
        case 4: return launch_ks<4>(p, pl.lds, (int)grid, s);
        case 8: return launch_ks<8>(p, pl.lds, (int)grid, s);
        case 12: return launch_ks<12>(p, pl.lds, (int)grid, s);
        case 16: return launch_ks<16>(p, pl.lds, (int)grid, s);
        case 24: return launch_ks<24>(p, pl.lds, (int)grid, s);
        default: return launch_ks<32>(p, pl.lds, (int)grid, s);
    }
}

static int naf_launch_inv_norm(const void* x, float* inv, int h, int w, int C, hipStream_t s) {
    const int64_t npix = (int64_t)h * w;
    hipLaunchKernelGGL(inv_norm_kernel, dim3((unsigned)((npix + 15) / 16)), dim3(256), 0, s, static_cast<const bf16_t*>(x), inv, npix, C);
    return naf_check_launch("inv_norm_kernel");
}

// ---- the C ABI ----
static int propagate_validate(const naf_propagate_args* a) {
    NAF_REQUIRE(a != nullptr, "naf_propagate: args is NULL");
    NAF_REQUIRE(a->n >= 1 && a->C >= 1 && a->h >= 1 && a->w >= 1 && a->K >= 1 && a->topk >= 1,
                "naf_propagate: n, C, h, w, K and topk must be at least 1 (got n=%d C=%d h=%d w=%d K=%d topk=%d)", a->n, a->C, a->h, a->w, a->K, a->topk);
    NAF_REQUIRE(a->radius >= 0, "naf_propagate: radius must not be negative (got %d)", a->radius);
    NAF_REQUIRE(a->temperature > 0.f, "naf_propagate: temperature must be > 0 (got %g)", (double)a->temperature);
    NAF_REQUIRE(a->reserved[0] == 0 && a->reserved[1] == 0, "naf_propagate: reserved fields must be 0");
    return NAF_OK;
}

#define PROP_SERVED(cond, ...)          \
    do {                                \
        if (!(cond)) {                  \
            naf_set_error(__VA_ARGS__); \
            return NAF_ERR_UNSUPPORTED; \
        }                               \
    } while (0)

extern "C" {

int naf_propagate_select(const naf_propagate_args* a) {
    const int rc = propagate_validate(a);
    if (rc != NAF_OK) return rc;
    PROP_SERVED(a->radius != 0, "naf_propagate: radius=0 is the dense case (no neighbourhood mask), which is not served: 1 <= radius <= 15");
    PROP_SERVED(a->radius <= 15, "naf_propagate: radius %d is not served: 1 <= radius <= 15", a->radius);
    PROP_SERVED(a->C % 32 == 0 && a->C >= 32 && a->C <= 1024, "naf_propagate: C = %d is not served: C %% 32 == 0 and 32 <= C <= 1024", a->C);
    PROP_SERVED(a->K <= 64, "naf_propagate: K = %d label channels are not served: 1 <= K <= 64", a->K);
    PROP_SERVED(a->topk <= 16, "naf_propagate: topk = %d is not served: 1 <= topk <= 16", a->topk);
    PROP_SERVED(a->n <= NAF_PROPAGATE_MAX_FRAMES, "naf_propagate: n = %d context frames are not served: 1 <= n <= 16", a->n);
    const int64_t per = (int64_t)a->h * a->w * (a->C > a->K ? a->C : a->K);
    PROP_SERVED(per < ((int64_t)1 << 31) && (int64_t)((a->w + PT_W - 1) / PT_W) * ((a->h + PT_H - 1) / PT_H) < ((int64_t)1 << 31),
                "naf_propagate: h * w * max(C, K) = %lld is not served: below 2^31 elements per frame", (long long)per);
    return NAF_OK;
}

int naf_propagate_plan(const naf_propagate_args* a, int32_t out[4]) {
    const int rc = naf_propagate_select(a);
    if (rc != NAF_OK) return rc;
    NAF_REQUIRE(out != nullptr, "naf_propagate_plan: out is NULL");
    PropPlan pl;
    const int prc = prop_plan(a, &pl);
    if (prc != NAF_OK) return prc;
    out[0] = pl.ksmax; out[1] = pl.nkb; out[2] = pl.nbuf; out[3] = (int32_t)pl.lds;
    return NAF_OK;
}

int naf_propagate_fwd(const naf_propagate_args* a, naf_stream_t stream) {
    const int rc = naf_propagate_select(a);
    if (rc != NAF_OK) return rc;
    NAF_REQUIRE(a->target && a->target_inv && a->segs && a->out, "naf_propagate_fwd: NULL tensor pointer");
    NAF_REQUIRE((reinterpret_cast<uintptr_t>(a->target) & 15) == 0, "naf_propagate_fwd: target must be 16-byte aligned");
    for (int f = 0; f < a->n; ++f) {
        NAF_REQUIRE(a->context[f] && a->context_inv[f], "naf_propagate_fwd: context frame %d is NULL", f);
        NAF_REQUIRE((reinterpret_cast<uintptr_t>(a->context[f]) & 15) == 0, "naf_propagate_fwd: context frame %d must be 16-byte aligned", f);
    }
    return naf_launch_propagate(a, static_cast<hipStream_t>(stream));
}

int naf_feature_inv_norm(const void* x, float* inv, int32_t h, int32_t w, int32_t C, naf_stream_t stream) {
    NAF_REQUIRE(x != nullptr && inv != nullptr, "naf_feature_inv_norm: NULL pointer");
    NAF_REQUIRE(h >= 1 && w >= 1 && C >= 8 && C % 8 == 0, "naf_feature_inv_norm: h, w >= 1 and C a positive multiple of 8 (got h=%d w=%d C=%d)", h, w, C);
    NAF_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0, "naf_feature_inv_norm: x must be 16-byte aligned");
    return naf_launch_inv_norm(x, inv, h, w, C, static_cast<hipStream_t>(stream));
}

}  // extern "C"
