// Eligibility test + dispatcher for the mask-pooling cell kernel (see xna_pool_kernel.h), the mass reduction and naf_maskpool_apply.
#include "xna_pool_kernel.h"

// the instances: xna_pool_inst.hip, one object per window
#define NAF_X(K) NAF_XNA_POOL_WINDOW(extern, K)
NAF_FOR_WINDOWS(NAF_X)
#undef NAF_X

// NAF_OK when the kernel serves the (validated) request; otherwise NAF_ERR_UNSUPPORTED with the reason in the error string.
int naf_xna_maskpool_eligible(const naf_xna_maskpool_args* a) {
    const int rc = xna_headsum_shape_eligible("naf_xna_maskpool", a);
    if (rc != NAF_OK) return rc;
    if (a->K > 64) {
        naf_set_error("naf_xna_maskpool: the fused kernel takes at most 64 masks per launch (got %d)", a->K);
        return NAF_ERR_UNSUPPORTED;
    }
    // cells that are no multiple of 8 pixels wide (14, 15, 30 ...) are read element by element: nothing is asked of the masks' alignment there
    const bool vec = ((a->Wo / a->w) & 7) == 0;
    if (!naf_aligned(a->q, 16) || !naf_aligned(a->k_lr, 16) || (vec && !naf_aligned(a->masks, 16))) {
        naf_set_error("naf_xna_maskpool: the fused kernel needs 16-byte aligned q, k_lr, masks");
        return NAF_ERR_UNSUPPORTED;
    }
    for (int i = 0; i < 4; ++i) {
        if (a->q_stride[i] % 8 || a->k_stride[i] % 8) {
            naf_set_error("naf_xna_maskpool: the fused kernel needs q / k_lr strides that are multiples of 8 elements");
            return NAF_ERR_UNSUPPORTED;
        }
    }
    if (a->m_stride[3] != 1 || (vec && (a->m_stride[0] % 8 || a->m_stride[1] % 8 || a->m_stride[2] % 8))) {
        naf_set_error("naf_xna_maskpool: the fused kernel needs x-contiguous masks whose b, k and y strides are multiples of 8 elements");
        return NAF_ERR_UNSUPPORTED;
    }
    return NAF_OK;
}

// (shared with the k-means step, xna_kmeans.hip, whose cell kernel writes the same partials)
size_t naf_xna_pool_ws(int B, int heads, int h, int w, int nslot, int K, size_t* mass_offset) {
    const size_t kpad = (size_t)((K + 15) & ~15), cells = (size_t)B * (size_t)h * (size_t)w;
    const size_t part = cells * (size_t)heads * (size_t)nslot * kpad * sizeof(float);
    if (mass_offset != nullptr) *mass_offset = part;
    return part + cells * kpad * sizeof(float);
}
size_t naf_xna_maskpool_ws(const naf_xna_maskpool_args* a, size_t* mass_offset) {
    return naf_xna_pool_ws(a->B, a->heads, a->h, a->w, a->ky * a->kx, a->K, mass_offset);
}

// mass[b, k] = sum over the cells of pmass[b][cell][k]: one workgroup per (b, k), thread t adds cells t, t + 256, ... in ascending
// order, then a tree over the 256 partial sums -- a fixed order, and exact for binary masks (integers below 2^24)
__global__ __launch_bounds__(256) void xna_pool_mass_kernel(const float* __restrict__ pmass, float* __restrict__ mass, int K, int kpad, int cells) {
    __shared__ float red[256];
    const int b = blockIdx.x / K, k = blockIdx.x - b * K;
    float s = 0.f;
    for (int c = threadIdx.x; c < cells; c += 256) s += pmass[((size_t)b * cells + c) * kpad + k];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int n = 128; n > 0; n >>= 1) {
        if ((int)threadIdx.x < n) red[threadIdx.x] += red[threadIdx.x + n];
        __syncthreads();
    }
    if (threadIdx.x == 0) mass[blockIdx.x] = red[0];
}

int naf_launch_xna_pool_mass(const float* pmass, float* mass, int B, int K, int kpad, int cells, hipStream_t s) {
    hipLaunchKernelGGL(xna_pool_mass_kernel, dim3((unsigned)(B * K)), dim3(256), 0, s, pmass, mass, K, kpad, cells);
    return naf_check_launch("xna_pool_mass_kernel");
}

int naf_launch_xna_maskpool(const naf_xna_maskpool_args* a, float scale, hipStream_t s) {
    XnaPoolParams p;
    xna_fill_common(p, a, a->k_stride, scale);
    size_t moff = 0;
    naf_xna_maskpool_ws(a, &moff);
    p.masks = a->masks;
    p.part = static_cast<float*>(a->workspace);
    p.pmass = reinterpret_cast<float*>(static_cast<char*>(a->workspace) + moff);
    p.tab_y = a->rope_tab_y; p.tab_x = a->rope_tab_x;
    p.dy = a->Ho / a->h; p.dx = a->Wo / a->w;
    p.K = a->K;
    p.kpad = (a->K + 15) & ~15;
    for (int i = 0; i < 4; ++i) p.ms[i] = a->m_stride[i];
    int rc = xna_grid("naf_xna_maskpool_fwd", (int64_t)a->B * a->h * a->w, &p.nblocks);
    if (rc != NAF_OK) return rc;
    const bool u8 = a->mask_dtype == NAF_MASK_U8;
    rc = NAF_ERR_UNSUPPORTED;
    switch (a->ky) {
#define NAF_X(K) case K: rc = xna_pool_launch_ks<K>(p, u8, a->A, s); break;
        NAF_FOR_WINDOWS(NAF_X)
#undef NAF_X
        default: naf_set_error("naf_xna_maskpool_fwd: kernel size %d has no instantiation", a->ky);
    }
    if (rc != NAF_OK) return rc;
    return naf_launch_xna_pool_mass(p.pmass, a->mass, a->B, a->K, p.kpad, a->h * a->w, s);
}

// pooled[b, k, c] = sum_j A[b, g(c), k, j] * v[b, c, j]: one wave per output, lane l takes j = l, l + 64, ... in ascending order
// (explicit fma), then the xor tree over the lanes -- a fixed order
__global__ __launch_bounds__(256) void maskpool_apply_kernel(const float* __restrict__ A, const bf16_t* __restrict__ v, const float* __restrict__ mass,
                                                             float* __restrict__ pooled, int heads, int K, int C, int hw, int64_t vsb, int64_t vsc,
                                                             int mean, size_t total) {
    const size_t o = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (o >= total) return;   // wave-uniform
    const int lane = threadIdx.x & 63;
    const int c = (int)(o % C);
    const size_t bk = o / C;
    const int k = (int)(bk % K), b = (int)(bk / K);
    const int g = c / (C / heads);
    const float* ap = A + (((size_t)b * heads + g) * K + k) * (size_t)hw;
    const bf16_t* vp = v + b * vsb + c * vsc;
    float s = 0.f;
    for (int j = lane; j < hw; j += 64) s = __builtin_fmaf(ap[j], (float)vp[j], s);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d, 64);
    if (lane == 0) {
        if (mean) {
            const float m = mass[bk];
            s = m != 0.f ? s / m : 0.f;
        }
        pooled[o] = s;
    }
}

int naf_launch_maskpool_apply(const float* A, const void* v, const float* mass, float* pooled, int B, int heads, int K, int C, int hw,
                              const int64_t* v_stride, int mean, hipStream_t s) {
    const size_t total = (size_t)B * K * C;
    hipLaunchKernelGGL(maskpool_apply_kernel, dim3((unsigned)((total + 3) / 4)), dim3(256), 0, s, A, static_cast<const bf16_t*>(v), mass, pooled, heads, K, C,
                       hw, v_stride[0], v_stride[1], mean, total);
    return naf_check_launch("maskpool_apply_kernel");
}
