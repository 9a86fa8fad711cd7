// Shared device/host helpers for libnaf_hip.so (gfx950 only).
#pragma once
#include <stdlib.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "naf_hip.h"

typedef __bf16 bf16_t;
typedef bf16_t bf16x8_t __attribute__((ext_vector_type(8)));
typedef bf16_t bf16x4_t __attribute__((ext_vector_type(4)));
typedef bf16_t bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));

typedef _Float16 f16_t;
typedef f16_t f16x8_t __attribute__((ext_vector_type(8)));

#define NAF_LDS __attribute__((address_space(3)))

// ---- the VALUE type of the attention forward kernels, chosen by their output type ----
// OutT = bf16_t / float: bf16 values, P rounded to bf16, v_mfma_f32_16x16x32_bf16 (what the kernels have always done).
// OutT = f16_t (NAF_F16): the values in memory and in the LDS are IEEE half, P is rounded to half, the PV product runs on
// v_mfma_f32_16x16x32_f16 (same lane maps, same rate) and the output is stored as half.  The kernels keep every 16-bit operand in
// bf16-typed registers -- loads, LDS transposes and lane exchanges move bits -- so only the three places below know the type.
// Half has 5 exponent bits: a softmax weight below 2^-14 would be a subnormal operand, and whether the matrix pipe honours those
// is not something the kernels rely on.  P is therefore multiplied by PSCALE = 2^8 before it is rounded (P <= 1 -> at most 256; the
// un-normalised weights of the row-streaming kernel are at most k*k * 2^8 < 65504) and the fp32 accumulator -- or the fp32
// normaliser -- is multiplied by 2^-8 before the store.  Both are exact, and a weight only vanishes below 2^-22.
template <typename OutT>
struct XnaVal {
    static constexpr bool F16 = std::is_same<OutT, f16_t>::value;
    static constexpr float PSCALE = F16 ? 256.f : 1.f;       // applied to P (through the normaliser) before the rounding
    static constexpr float UNSCALE = F16 ? 1.f / 256.f : 1.f;  // applied to the accumulator (or the normaliser) before the store
    // P -> the 16-bit B / A operand (the caller has applied PSCALE)
    __device__ static __forceinline__ bf16_t p(float x) {
        if constexpr (F16) return __builtin_bit_cast(bf16_t, (f16_t)x);
        else return (bf16_t)x;
    }
    // accumulator -> the 16-bit stored element (applies UNSCALE)
    __device__ static __forceinline__ bf16_t o(float x) {
        if constexpr (F16) return __builtin_bit_cast(bf16_t, (f16_t)(x * UNSCALE));
        else return (bf16_t)x;
    }
    __device__ static __forceinline__ f32x4_t mfma(bf16x8_t a, bf16x8_t b, f32x4_t c) {
        if constexpr (F16) return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
        else return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    }
};

// ---- error plumbing (naf_api.cpp owns the storage) ----
void naf_set_error(const char* fmt, ...);
int naf_check_launch(const char* what);
int naf_cu_count();   // compute units of the current device (cached per device)

#define NAF_REQUIRE(cond, ...)        \
    do {                              \
        if (!(cond)) {                \
            naf_set_error(__VA_ARGS__); \
            return NAF_ERR_INVALID;   \
        }                             \
    } while (0)

// ---- kernel launchers implemented in the .hip files ----
int naf_launch_xna_mfma(const naf_xna_args* a, float scale, hipStream_t s);      // xna_mfma.hip
int naf_xna_mfma_eligible(const naf_xna_args* a, int* dvt_out, size_t* lds_out);  // xna_mfma.hip
int naf_xna_mfma_rope_ok(const naf_xna_args* a);                                   // xna_mfma.hip
int naf_launch_xna_generic(const naf_xna_args* a, float scale, hipStream_t s);   // xna_generic.hip
int naf_launch_xna_union(const naf_xna_args* a, float scale, hipStream_t s);     // xna_union.hip
int naf_xna_union_eligible(const naf_xna_args* a);                               // xna_union.hip
int naf_launch_xna_rows(const naf_xna_args* a, float scale, hipStream_t s);      // xna_rows.hip
int naf_xna_rows_eligible(const naf_xna_args* a);                                // xna_rows.hip
int naf_launch_xna_head(const naf_xna_head_args* a, float scale, hipStream_t s);   // xna_head.hip
int naf_xna_head_eligible(const naf_xna_head_args* a);                          // xna_head.hip: NAF_OK, or NAF_ERR_UNSUPPORTED with the reason set
int naf_launch_xna_head_ce(const naf_xna_head_ce_args* a, float scale, hipStream_t s);   // xna_head.hip: the classification epilogue
int naf_launch_xna_head_cm(const naf_xna_head_cm_args* a, float scale, hipStream_t s);   // xna_head.hip: ... with a confusion matrix
int naf_xna_head_ce_eligible(const naf_xna_head_ce_args* a);                          // xna_head.hip: naf_xna_head_eligible plus the dlogits layout
int naf_launch_xna_head_reg(const naf_xna_head_reg_args* a, float scale, hipStream_t s);   // xna_head.hip: the regression epilogue and its finishing kernel
int naf_xna_head_reg_eligible(const naf_xna_head_reg_args* a);                          // xna_head.hip: naf_xna_head_eligible plus N <= 32 and the dlogits layout
size_t naf_xna_head_reg_ws(const naf_xna_head_reg_args* a);                             // xna_head.hip: bytes of the statistics workspace (0 without errors)
int naf_launch_xna_cos(const naf_xna_cos_args* a, float scale, hipStream_t s);     // xna_cos.hip: the cosine head
int naf_xna_cos_eligible(const naf_xna_cos_args* a);                              // xna_cos.hip: NAF_OK, or NAF_ERR_UNSUPPORTED with the reason set
int naf_launch_xna_cos_ce(const naf_xna_cos_ce_args* a, float scale, hipStream_t s);   // xna_cos.hip: ... with the classification epilogue
int naf_xna_cos_ce_eligible(const naf_xna_cos_ce_args* a);                            // xna_cos.hip: naf_xna_cos_eligible plus the dlogits layout
int naf_launch_xna_cos_peaks(const naf_xna_cos_peaks_args* a, float scale, hipStream_t s);   // xna_cos.hip: ... with the peak epilogue
int naf_xna_cos_peaks_eligible(const naf_xna_cos_peaks_args* a);                             // xna_cos.hip: naf_xna_cos_eligible plus the peak instantiation
int naf_launch_peaks_topk(const float* peak, const int32_t* where, float* values, int32_t* index, int B, int N, int n_cells, int k,
                          const int64_t* peak_stride, const int64_t* where_stride, hipStream_t s);   // peaks_topk.hip
int naf_launch_xna_maskpool(const naf_xna_maskpool_args* a, float scale, hipStream_t s);   // xna_pool.hip: mask pooling (cell kernel, gather, mass)
int naf_xna_maskpool_eligible(const naf_xna_maskpool_args* a);                          // xna_pool.hip: NAF_OK, or NAF_ERR_UNSUPPORTED with the reason set
size_t naf_xna_maskpool_ws(const naf_xna_maskpool_args* a, size_t* mass_offset);        // xna_pool.hip: workspace bytes, offset of the per-cell masses
int naf_launch_maskpool_apply(const float* A, const void* v, const float* mass, float* pooled, int B, int heads, int K, int C, int hw,
                              const int64_t* v_stride, int mean, hipStream_t s);        // xna_pool.hip
size_t naf_xna_pool_ws(int B, int heads, int h, int w, int nslot, int K, size_t* mass_offset);   // xna_pool.hip: the per-cell partials of both pooling families
int naf_launch_xna_pool_mass(const float* pmass, float* mass, int B, int K, int kpad, int cells, hipStream_t s);   // xna_pool.hip: mass[b, k] from the per-cell masses
int naf_launch_xna_kmeans(const naf_xna_kmeans_args* a, float scale, hipStream_t s);   // xna_kmeans.hip: k-means step (cell kernel, gather, mass)
int naf_xna_kmeans_eligible(const naf_xna_kmeans_args* a);                          // xna_kmeans.hip: NAF_OK, or NAF_ERR_UNSUPPORTED with the reason set
int naf_tile_span(int L_out, int L_in, int k);                                  // xna_rows.hip: low-res columns under 16 consecutive queries
// `sg` (0.4.3): the gradient of the scores (naf_xna_bwd_scores); nullptr = the plain backward, the same launches as before
int naf_launch_xna_bwd(const naf_xna_bwd_args* a, float scale, hipStream_t s, const naf_xna_bwd_scores_args* sg = nullptr);   // xna_bwd.hip
int naf_xna_bwd_eligible(const naf_xna_bwd_args* a);                             // xna_bwd.hip
int naf_xna_bwd_chunks(const naf_xna_bwd_args* a, int32_t* out, int cap);            // xna_bwd.hip
int naf_launch_xna_generic_bwd(const naf_xna_bwd_args* a, float scale, hipStream_t s, const naf_xna_bwd_scores_args* sg = nullptr);  // xna_generic.hip
int naf_launch_xna_rows_bwd(const naf_xna_bwd_args* a, float scale, hipStream_t s, const naf_xna_bwd_scores_args* sg = nullptr);     // xna_rows_bwd.hip
int naf_xna_rows_bwd_eligible(const naf_xna_bwd_args* a);                               // xna_rows_bwd.hip
size_t naf_xna_rows_bwd_workspace(const naf_xna_bwd_args* a);                           // xna_rows_bwd.hip
int naf_launch_rope_tables(float* ty, float* tx, const float* periods, int np, int Ho, int Wo, hipStream_t s);
int naf_launch_rope_pool(const naf_rope_pool_args* a, hipStream_t s);             // rope_pool.hip
int naf_launch_pack_values(void* vp, const void* v, int v_dtype, int B, int C, int h, int w,
                           const int64_t* vs, hipStream_t s);                    // pack.hip

int naf_launch_preshrink(float* out, const void* img, int dtype, int B, int H, int W, int Hs, int Ws, const int64_t* st, hipStream_t s);   // resize.hip
int naf_launch_pool_guidance(void* y, const void* x, int B, int H, int W, int Ho, int Wo, int C, hipStream_t s);   // pool.hip
int naf_launch_preshrink_bwd(void* dimg, const float* dout, int dtype, int B, int H, int W, int Hs, int Ws, const int64_t* st, hipStream_t s);   // resize.hip
int naf_launch_pool_guidance_bwd(void* dx, const void* dy, int B, int H, int W, int Ho, int Wo, int C, hipStream_t s);   // pool.hip

int naf_launch_stem_conv0(const naf_stem_conv0_args* a, hipStream_t s);            // stem_conv0.hip
int naf_launch_stem_conv(const naf_stem_conv_args* a, hipStream_t s, const naf_key_pool_args* kp = nullptr);   // stem_conv.hip
int naf_stem_conv_keys_ok(const naf_stem_conv_args* a, const naf_key_pool_args* kp);                            // stem_conv.hip
int naf_stem_conv3_plan(int B, int H, int W, bool keys, int64_t* nblocks);                                       // stem_conv.hip
int naf_launch_stem_conv1x1(const naf_stem_conv_args* a, hipStream_t s, const naf_key_pool_args* kp = nullptr);   // stem_conv1x1.hip (kp: also the branch's pooled keys)
int naf_stem_conv1x1_keys_ok(const naf_stem_conv_args* a, const naf_key_pool_args* kp);
int naf_launch_stem_conv0_generic(const naf_stem_conv0_args* a, hipStream_t s);    // stem_generic.hip (widths other than 128)
int naf_launch_stem_conv_generic(const naf_stem_conv_args* a, hipStream_t s);
int naf_launch_rope_pool_bwd(const naf_rope_pool_bwd_args* a, hipStream_t s);
int naf_launch_stem_wgrad(const naf_stem_wgrad_args* a, hipStream_t s);
int naf_launch_stem_wgrad_generic(const naf_stem_wgrad_args* a, hipStream_t s);   // stem_generic_bwd.hip: widths other than 128
int naf_launch_stem_conv0_wgrad(const naf_stem_conv0_wgrad_args* a, hipStream_t s);
int naf_launch_stem_conv0_dgrad(const naf_stem_conv0_dgrad_args* a, hipStream_t s);
int naf_launch_stem_act_fwd(const naf_stem_act_args* a, hipStream_t s);
int naf_launch_stem_act_bwd(const naf_stem_act_bwd_args* a, hipStream_t s);

int naf_launch_axis_table(int32_t* out_dev, int L_out, int L_in, int k, hipStream_t s);  // axis_table.hip

// ---- the per-axis neighbourhood rule, one definition for the host table and the device table ----
// NATTEN <= 0.17 get_window_start (published algorithm; NATTEN is not vendored by the reference).
__host__ __device__ inline int naf_window_start(int i, int L, int k, int dil) {
    const int r = k / 2;
    if (dil <= 1) return (i - r > 0 ? i - r : 0) + (i + r >= L ? (L - i - r - 1) : 0);
    const int ni = i - r * dil;
    if (ni < 0) return i % dil;
    if (i + r * dil >= L) {
        const int m = i % dil, a = (L / dil) * dil, b = L - a;
        return (m < b) ? (L - b + m - 2 * r * dil) : (a + m - k * dil);
    }
    return ni;
}
// F.interpolate(mode="nearest-exact") source index of position `pos` on the (virtual) upsampled grid, in ATen's
// device arithmetic (UpSample.cuh nearest_neighbor_exact_compute_source_index): all-fp32
// floorf((pos + 0.5f) * (float(in) / float(out))), clamped to in-1, every operation rounded on its own (no FMA
// contraction, correctly rounded division) so that host and device agree bit for bit.  At exact ties ATen's CPU
// build may differ by one; see DESIGN.md.
__host__ __device__ inline int naf_nearest_exact_src(int pos, int L_in, int L_out) {
#if defined(__HIP_DEVICE_COMPILE__)
    const float prod = __fmul_rn((float)pos + 0.5f, __fdiv_rn((float)L_in, (float)L_out));
#else
    const float scale = (float)L_in / (float)L_out;
    volatile float prod = ((float)pos + 0.5f) * scale;
#endif
    int src = (int)floorf(prod);
    return src > L_in - 1 ? L_in - 1 : src;
}

// ---- device helpers ----
__device__ __forceinline__ float bf16_bits_to_float(uint16_t b) { return __uint_as_float(((uint32_t)b) << 16); }

// RoPE pair rotation (rope.py:15-34): one definition for naf_rope_pool_fwd and for the rotate-on-load of
// naf_xna_fwd, so both round identically (explicit fma, the inner products are rounded on their own).
__device__ __forceinline__ void naf_rope_rotate(float a, float b, float c, float s, float& o1, float& o2) {
    o1 = __builtin_fmaf(a, c, -(b * s));
    o2 = __builtin_fmaf(b, c, a * s);
}

// Reductions over the four 16-lane rows of a wave (lanes l, l^16, l^32, l^48) on the VALU: v_permlane16_swap exchanges the
// odd rows of one register with the even rows of the other, v_permlane32_swap the upper half of one with the lower half of
// the other -- with both operands the same value, the two results hold "mine" and "my partner's".  (__shfl_xor goes through
// ds_bpermute: an LDS round trip of 100+ cycles on the softmax's critical path, four times per tile.)
__device__ __forceinline__ float naf_rows_max(float v) {
    const uint32_t b = __float_as_uint(v);
    const auto r16 = __builtin_amdgcn_permlane16_swap(b, b, false, false);
    const float m16 = fmaxf(__uint_as_float(r16[0]), __uint_as_float(r16[1]));
    const uint32_t c = __float_as_uint(m16);
    const auto r32 = __builtin_amdgcn_permlane32_swap(c, c, false, false);
    return fmaxf(__uint_as_float(r32[0]), __uint_as_float(r32[1]));
}
__device__ __forceinline__ float naf_rows_sum(float v) {
    const uint32_t b = __float_as_uint(v);
    const auto r16 = __builtin_amdgcn_permlane16_swap(b, b, false, false);
    const float s16 = __uint_as_float(r16[0]) + __uint_as_float(r16[1]);
    const uint32_t c = __float_as_uint(s16);
    const auto r32 = __builtin_amdgcn_permlane32_swap(c, c, false, false);
    return __uint_as_float(r32[0]) + __uint_as_float(r32[1]);
}

// GroupNorm sums travel as fp64 {sum, sum of squares} in NAF_STATS_SLOTS copies [slot][B][8][2] (include/naf_hip.h): a producer's
// workgroup adds into copy (workgroup index mod NAF_STATS_SLOTS), a consumer adds the copies up.  One copy of an image is one
// 128-byte line, and device-scope atomics to one line are served one after another (~4.6 ns each, tools/stem_rows_fixed_probe.hip:
// 256 workgroups x 16 atomics into ONE line held the end of every stem launch back by 17-20 us).
__device__ __forceinline__ double* naf_gn_slot(double* stats, int B, int b, uint32_t wg) {
    return stats + ((size_t)(wg % (uint32_t)NAF_STATS_SLOTS) * (size_t)B + (size_t)b) * 16;
}
__device__ __forceinline__ void naf_gn_sums(const double* stats, int B, int b, int g, double& s1, double& s2) {
    typedef double f64x2_t __attribute__((ext_vector_type(2)));
    f64x2_t acc = {0.0, 0.0};
#pragma unroll
    for (int sl = 0; sl < NAF_STATS_SLOTS; ++sl) acc += *reinterpret_cast<const f64x2_t*>(stats + ((size_t)sl * (size_t)B + (size_t)b) * 16 + g * 2);
    s1 = acc[0];
    s2 = acc[1];
}

// A/B tuning knobs (NAF_XNA_ORDER, NAF_XNA_STAGE, NAF_UNION_PLAN, ...) are measurement tools: they are honoured only when the
// process also sets NAF_HIP_KNOBS=1, so that a stray environment variable cannot change kernel selection in production.
inline const char* naf_knob(const char* name) {
    static const bool on = [] { const char* e = getenv("NAF_HIP_KNOBS"); return e != nullptr && atoi(e) != 0; }();
    return on ? getenv(name) : nullptr;
}

// ---- host helpers shared by the attention dispatchers ----
// The windows the cell, table-driven, head and backward kernels are instantiated for (one object per window: build.py INSTANCES),
// and the sliding kernel's.  A dispatcher declares its instances `extern template` and builds its switch from the same list.
#define NAF_FOR_WINDOWS(X) X(3) X(5) X(7) X(9) X(11) X(13) X(15)
#define NAF_FOR_SLIDE_WINDOWS(X) X(7) X(9) X(11) X(13) X(15)

inline bool naf_aligned(const void* p, size_t n) { return (reinterpret_cast<uintptr_t>(p) % n) == 0; }

// The softmax scale of a call: the caller's, or 1 / sqrt(Dq) when it leaves the field at 0.  The kernels take it times log2(e) (exp2).
inline float xna_scale(float scale, int Dq) { return scale > 0.f ? scale : 1.0f / sqrtf((float)Dq); }
constexpr float XNA_LOG2E = 1.4426950408889634f;

// The workgroup count of an attention launch: NAF_OK with *nblocks set, or NAF_ERR_INVALID with `who` (the entry's name) in the message.
inline int xna_grid(const char* who, int64_t nb, uint32_t* nblocks) {
    if (nb <= 0 || nb > 0x7fffffffLL) {
        naf_set_error("%s: grid of %lld workgroups out of range", who, (long long)nb);
        return NAF_ERR_INVALID;
    }
    *nblocks = (uint32_t)nb;
    return NAF_OK;
}

// What every cell kernel asks of the geometry (A: naf_xna_args, naf_xna_head_args or naf_xna_bwd_args): a square odd window 3 .. 15,
// Dq = 64, a grid no smaller than the window, an integer ratio.
template <typename A>
inline bool xna_cell_shape_ok(const A* a) {
    const int ks = a->ky;
    return a->ky == a->kx && ks >= 3 && ks <= 15 && (ks & 1) != 0 && a->Dq == 64 && a->h >= ks && a->w >= ks && a->Ho % a->h == 0 && a->Wo % a->w == 0;
}

// ... and of q / k / v (`v`: a->v_lr, or the head's a->pv_lr, with its strides): 16-byte pointers, strides in whole 16-byte chunks.
template <typename A>
inline bool xna_qkv_layout_ok(const A* a, const void* v, const int64_t* v_stride) {
    if (!naf_aligned(a->q, 16) || !naf_aligned(a->k_lr, 16) || !naf_aligned(v, 16)) return false;
    for (int i = 0; i < 4; ++i)
        if (a->q_stride[i] % 8 || a->k_stride[i] % 8 || v_stride[i] % 8) return false;
    return true;
}

// The fields every attention parameter struct shares (P: XnaMfmaParams, XnaUnionParams, XnaHeadParams, XnaBwdParams); the kernel's
// value pointer and the rest are the caller's.
template <typename P, typename A>
inline void xna_fill_common(P& p, const A* a, const int64_t* v_stride, float scale) {
    p.q = static_cast<const bf16_t*>(a->q);
    p.k = static_cast<const bf16_t*>(a->k_lr);
    p.B = a->B; p.heads = a->heads; p.Ho = a->Ho; p.Wo = a->Wo; p.h = a->h; p.w = a->w;
    p.scale_log2e = scale * XNA_LOG2E;
    for (int i = 0; i < 4; ++i) {
        p.qs[i] = a->q_stride[i]; p.ks[i] = a->k_stride[i]; p.vs[i] = v_stride[i];
    }
}

// Bijective XCD-aware remap: hardware places block b on XCD b % 8; give every XCD one contiguous
// range of logical ids so neighbouring cells (which share K/V windows) meet in the same L2.
__device__ __forceinline__ uint32_t naf_xcd_remap(uint32_t bid, uint32_t n) {
    const uint32_t q = n >> 3, r = n & 7u, xcd = bid & 7u, idx = bid >> 3;
    const uint32_t base = (xcd < r) ? xcd * (q + 1u) : r * (q + 1u) + (xcd - r) * q;
    return base + idx;
}

// Row tiles of the attention cell kernels: a 16-query tile is (up to) 16 consecutive pixels of one cell row.  Exact for Wo/w a multiple of 16;
// for other widths the last tile of a row is partial (masked lanes), taken while at most 1/7 of the row's lanes idle (14-pixel cells of
// patch-14 backbones, 15, 28, 30, 31 ...).  Forward: xna_mfma_kernel.h / xna_slide_kernel.h; backward: xna_bwd2_kernel.h (PT).
__host__ __device__ inline bool xna_row_tiles_ok(int dx) {
    const int pad = ((dx + 15) & ~15) - dx;
    return pad * 6 <= dx;
}

// ---- the two head-summed families (A: naf_xna_head_args or naf_xna_cos_args; `fam` prefixes the messages: "naf_xna_head", "naf_xna_cos") ----
// The geometry their cell kernel serves: NAF_OK, or NAF_ERR_UNSUPPORTED with the reason set.
template <typename A>
inline int xna_headsum_shape_eligible(const char* fam, const A* a) {
    if (!xna_cell_shape_ok(a)) {   // which of its conditions (an even window never gets here: the entries refuse it)
        const int ks = a->ky;
        if (a->ky != a->kx || ks < 3 || ks > 15) naf_set_error("%s: the fused kernel needs a square window 3 .. 15 (got %dx%d)", fam, a->ky, a->kx);
        else if (a->Dq != 64) naf_set_error("%s: the fused kernel needs Dq = 64 (got %d)", fam, a->Dq);
        else if (a->h < ks || a->w < ks) naf_set_error("%s: the fused kernel needs h, w >= window (got %dx%d, window %d)", fam, a->h, a->w, ks);
        else naf_set_error("%s: the fused kernel needs an integer ratio (got %dx%d -> %dx%d)", fam, a->h, a->w, a->Ho, a->Wo);
        return NAF_ERR_UNSUPPORTED;
    }
    const int dy = a->Ho / a->h, dx = a->Wo / a->w;
    if (!xna_row_tiles_ok(dx) || (int64_t)dy * ((dx + 15) / 16) > 1024) {
        naf_set_error("%s: the fused kernel needs row tiles (Wo/w a multiple of 16, or 14, 15, 28, 30 ...; at most 1024 tiles per cell; got %dx%d -> %dx%d)",
                      fam, a->h, a->w, a->Ho, a->Wo);
        return NAF_ERR_UNSUPPORTED;
    }
    return NAF_OK;
}

// What both families' parameter structs (P: XnaHeadParams, XnaCosParams) take from their arguments, and the grid; `who` names the entry.
template <typename P, typename A>
inline int xna_headsum_fill(P& p, const A* a, float scale, const char* who) {
    xna_fill_common(p, a, a->pv_stride, scale);
    p.pv = static_cast<const bf16_t*>(a->pv_lr);
    p.out = a->out;
    p.tab_y = a->rope_tab_y; p.tab_x = a->rope_tab_x;
    p.dy = a->Ho / a->h; p.dx = a->Wo / a->w;
    p.N = a->N;
    p.npad = (a->N + 15) & ~15;
    for (int i = 0; i < 3; ++i) p.os[i] = a->o_stride[i];
    return xna_grid(who, (int64_t)a->B * a->h * a->w, &p.nblocks);
}
