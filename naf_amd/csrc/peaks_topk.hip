// The k best cells of every (batch, channel) row of the cell peaks (include/naf_hip.h: naf_peaks_topk).
//
// Candidates are the n_cells pairs (peak, where) of a row, ordered by value descending, then by flat index ascending -- the comparator
// of the peak epilogue (xna_cos_kernel.h), a total order because every cell's index lies inside its own cell.  One wave per row makes k
// selection passes: pass j takes the best candidate that the (j - 1)-th result strictly beats, so nothing is marked, nothing is written
// but the results and there is no workspace.  A lane scans the cells lane, lane + 64, ... in ascending order, the 64 lanes are merged by
// a butterfly with the same comparator: the order of the merge cannot change the result.  Launch-scale work (k <= 64 passes over h * w
// pairs); it exists because the tie rule is stated on the flat index, which is not the order of the cells.
#include "naf_common.h"

constexpr int PEAKS_TOPK_WAVES = 4;   // rows per workgroup

__device__ __forceinline__ bool peaks_before(float av, int ai, float bv, int bi) { return av > bv || (av == bv && ai < bi); }

__global__ __launch_bounds__(PEAKS_TOPK_WAVES * 64) void peaks_topk_kernel(const float* __restrict__ peak, const int32_t* __restrict__ where,
                                                                         float* __restrict__ values, int32_t* __restrict__ index, int rows, int N,
                                                                         int n_cells, int k, int64_t ps_b, int64_t ps_c, int64_t is_b, int64_t is_c) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * PEAKS_TOPK_WAVES + (threadIdx.x >> 6);   // wave-uniform
    if (row >= rows) return;
    const int b = row / N, n = row - b * N;
    const float* pr = peak + b * ps_b + n;
    const int32_t* ir = where + b * is_b + n;
    float pv = INFINITY;   // the previous result: the first pass admits every finite candidate
    int pi = -1;
    for (int j = 0; j < k; ++j) {
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int c = lane; c < n_cells; c += 64) {
            const float v = pr[(int64_t)c * ps_c];
            const int i = ir[(int64_t)c * is_c];
            if (peaks_before(pv, pi, v, i) && peaks_before(v, i, bv, bi)) {
                bv = v;
                bi = i;
            }
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const float ov = __shfl_xor(bv, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            if (peaks_before(ov, oi, bv, bi)) {
                bv = ov;
                bi = oi;
            }
        }
        if (lane == 0) {
            values[(int64_t)row * k + j] = bv;
            index[(int64_t)row * k + j] = bi;
        }
        pv = bv;
        pi = bi;
    }
}

int naf_launch_peaks_topk(const float* peak, const int32_t* where, float* values, int32_t* index, int B, int N, int n_cells, int k,
                          const int64_t* peak_stride, const int64_t* where_stride, hipStream_t s) {
    const int rows = B * N;
    hipLaunchKernelGGL(peaks_topk_kernel, dim3((unsigned)((rows + PEAKS_TOPK_WAVES - 1) / PEAKS_TOPK_WAVES)), dim3(PEAKS_TOPK_WAVES * 64), 0, s, peak, where,
                       values, index, rows, N, n_cells, k, peak_stride[0], peak_stride[1], where_stride[0], where_stride[1]);
    return naf_check_launch("peaks_topk_kernel");
}
