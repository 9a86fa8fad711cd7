// DAVIS J and F measures (include/naf_hip.h, naf_davis_jf): the integer counts behind the region similarity and the boundary measure of two
// label-map sequences, in one launch.  Replaces the per-(object, frame) host arithmetic of davis_db_eval_iou / davis_f_measure / _seg2bmap
// (evaluation/eval_video_seg.py:145-248).
//
// Decomposition ("DAVIS J and F"):
//   * one workgroup (4 waves) owns a 32 x 64 tile of one frame.  It stages the label bytes of both maps once, with a halo of R + 1 pixels
//     (R = floor(bound_pix): R for the disk, 1 for the Sobel window).  Outside the image the staged rows -1 / H and columns -1 / W hold the
//     REFLECTED pixels (row 1 / H - 2: the border rule of the boundary map), everything further out is never read
//   * while staging, the labels 1 .. N seen in the tile and the one-pixel ring around it are collected in a 32-bit mask: a label absent
//     from that ring in both maps contributes nothing to any counter of this tile and is skipped
//   * per label present: the two masks (label == o) over the staged region are packed into 64-bit words, one __ballot per 64 staged
//     columns; the two boundary maps of the tile and its R-pixel halo (a row of 64 + 2R <= 128 pixels is two words) then come from those
//     words by shifts and bitwise logic, a thread per word of 64 pixels.  The next label's masks are packed beside this one's counting
//   * a wave counts one tile row at a time, a lane per pixel: region counts are popcounts of ballots; a boundary pixel tests its disk as
//     masked-word tests against the other map's packed rows (wave-uniform LDS reads: every lane of a wave is in the same row), with
//     the half-width of each disk row, floor(sqrt(r2 - dy^2)), from a table in the kernel arguments; rows are taken nearest first and the
//     loop ends when every boundary pixel of the row has found its partner
//   * counters: wave-uniform registers -> LDS [wave][label][6] -> one 64-bit integer atomic per (label, counter, workgroup), zeros skipped.
//     Integer adds: the result does not depend on the order of arrival
#include "naf_common.h"

namespace {

constexpr int DJ_W = NAF_DAVIS_TILE_W, DJ_H = NAF_DAVIS_TILE_H, DJ_MAXR = NAF_DAVIS_MAX_HALF_WIDTH, DJ_MAXN = NAF_DAVIS_MAX_OBJECTS;
constexpr int DJ_NW = 2;   // 64-bit words of a packed row
static_assert(DJ_W == 64, "a tile row is one wave");
static_assert(DJ_W + 2 * DJ_MAXR <= 64 * DJ_NW, "a packed row with its halo fits its words");
static_assert(DJ_MAXN <= 32 && DJ_MAXN * 6 <= 256, "labels fit the presence mask, counters fit one thread each");
constexpr int DJ_MAX_DIM = 16384;

struct DavisParams {
    const uint8_t* ann;
    const uint8_t* seg;
    unsigned long long* counts;
    int T, H, W, N, R;
    int tiles_x, tiles;   // per frame
    int sp;               // bytes between two staged rows
    uint8_t hw[DJ_MAXR + 1];
};

// 64-bit words of a packed MASK row: the staged columns, 64 + 2R + 2 (three words at R = 32)
__host__ __device__ inline int davis_mask_words(int R) { return (DJ_W + 2 * R + 2 + 63) >> 6; }

__host__ __device__ inline size_t davis_lds(int R, int sp) {
    const int BR = DJ_H + 2 * R;
    return (size_t)2 * BR * DJ_NW * 8 + (size_t)2 * (BR + 2) * davis_mask_words(R) * 8 + (size_t)4 * DJ_MAXN * 6 * 4 + 16 + (size_t)2 * (BR + 2) * sp;
}

__global__ __launch_bounds__(256) void davis_jf_kernel(const DavisParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_dj[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int R = p.R, H = p.H, W = p.W, sp = p.sp;
    const int BR = DJ_H + 2 * R, BWD = DJ_W + 2 * R, SH = BR + 2, per = SH * sp, MW = davis_mask_words(R);
    const int t = (int)(blockIdx.x / (uint32_t)p.tiles), tile = (int)(blockIdx.x - (uint32_t)t * (uint32_t)p.tiles);
    const int x0 = (tile % p.tiles_x) * DJ_W, y0 = (tile / p.tiles_x) * DJ_H;

    // LDS: packed boundary rows [annotation, segmentation][BR][2] | packed mask rows [2][SH][MW] | counters [4 waves][32 labels][6] | presence |
    // labels [2][SH][sp]
    uint64_t* bm = reinterpret_cast<uint64_t*>(smem_dj);
    uint64_t* mk = bm + 2 * BR * DJ_NW;
    uint32_t* cnt = reinterpret_cast<uint32_t*>(mk + 2 * SH * MW);
    uint32_t* present = cnt + 4 * DJ_MAXN * 6;
    uint8_t* lab = reinterpret_cast<uint8_t*>(present + 4);

    if (tid == 0) *present = 0u;
    __syncthreads();

    // ---- stage both maps' tile with its halo; staged (sy, sx) is pixel (y0 - R - 1 + sy, x0 - R - 1 + sx) ----
    {
        const size_t frame = (size_t)t * H * W;
        const int dq = 256 / sp, dr = 256 % sp;
        int sy = tid / sp, sx = tid - sy * sp;
        uint32_t seen = 0u;
        while (sy < 2 * SH) {
            const int m = sy >= SH, ry = sy - m * SH;
            int y = y0 - R - 1 + ry, x = x0 - R - 1 + sx;
            uint8_t v = 0;
            if (y >= -1 && y <= H && x >= -1 && x <= W) {
                y = y < 0 ? 1 : (y >= H ? H - 2 : y);
                x = x < 0 ? 1 : (x >= W ? W - 2 : x);
                v = (m ? p.seg : p.ann)[frame + (size_t)y * W + x];
                if (ry >= R && ry < R + DJ_H + 2 && sx >= R && sx < R + DJ_W + 2 && v >= 1 && v <= p.N) seen |= 1u << (v - 1);
            }
            lab[sy * sp + sx] = v;
            sy += dq;
            sx += dr;
            if (sx >= sp) {
                sx -= sp;
                ++sy;
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) seen |= __shfl_xor(seen, off, 64);
        if (lane == 0 && seen != 0u) atomicOr(present, seen);
    }
    __syncthreads();
    const uint32_t pres = *present;
    if (pres == 0u) return;   // workgroup-uniform

    // packed rows of the two masks (label == o) over the staged region: one __ballot per 64 staged columns, bit = staged column
    auto masks = [&](int o) {
        for (int task = wv; task < 2 * SH * MW; task += 4) {
            const int row = task / MW, sx = (task - row * MW) * 64 + lane;   // row = map * SH + staged row
            const bool b = sx < sp && lab[row * sp + sx] == o;
            const uint64_t word = __ballot(b);
            if (lane == 0) mk[task] = word;
        }
    };

    // the two boundary maps over the tile and its R-pixel halo from the packed masks, a thread per 64-pixel word: the Sobel sums
    // a + 2b + c of three 0/1 values are the 3-bit numbers (a^c, (a&c)^b, a&c&b), and a response is non-zero where two of them differ
    auto boundary = [&]() {
        for (int task = tid; task < 2 * BR * DJ_NW; task += 256) {
            const int m = task >= BR * DJ_NW, rem = task - m * BR * DJ_NW, ry = rem >> 1, wi = rem & 1;
            const int y = y0 - R + ry, xw = x0 - R + wi * 64;               // the pixel of bit 0
            const int lo = max(0, -xw), hi = min(63, min(W - 1 - xw, BWD - 1 - wi * 64));
            uint64_t out = 0ull;
            if (y >= 0 && y < H && lo <= hi) {
                uint64_t l[3], c[3], r[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {                                 // staged rows ry, ry + 1, ry + 2; staged columns bx, bx + 1, bx + 2
                    const uint64_t* w = mk + (m * SH + ry + k) * MW;
                    const uint64_t w0 = w[wi], w1 = wi + 1 < MW ? w[wi + 1] : 0ull;
                    l[k] = w0;
                    c[k] = (w0 >> 1) | (w1 << 63);
                    r[k] = (w0 >> 2) | (w1 << 62);
                }
                auto differ = [](uint64_t a1, uint64_t b1, uint64_t c1, uint64_t a2, uint64_t b2, uint64_t c2) {
                    return ((a1 ^ c1) ^ (a2 ^ c2)) | (((a1 & c1) ^ b1) ^ ((a2 & c2) ^ b2)) | ((a1 & c1 & b1) ^ (a2 & c2 & b2));
                };
                const uint64_t ex = differ(r[0], r[1], r[2], l[0], l[1], l[2]);
                const uint64_t ey = differ(l[2], c[2], r[2], l[0], c[0], r[0]);
                out = (ex | ey) & (~0ull << lo) & (~0ull >> (63 - hi));
            }
            bm[task] = out;
        }
    };

    // the six counters of label o over this wave's tile rows, from the packed boundary maps
    auto count = [&](int o) {
        const uint64_t* bg = bm;
        const uint64_t* bs = bg + BR * DJ_NW;
        uint32_t inters = 0, uni = 0, n_seg = 0, n_gt = 0, seg_hits = 0, gt_hits = 0;
        const int x = x0 + lane, bx = lane + R;
        // a map without a boundary pixel anywhere in the region (an object the other map lacks) cannot be hit: nothing searches for it
        uint64_t og = 0ull, os = 0ull;
        for (int i = lane; i < BR * DJ_NW; i += 64) {
            og |= bg[i];
            os |= bs[i];
        }
        const bool any_g = __ballot(og != 0ull) != 0ull, any_s = __ballot(os != 0ull) != 0ull;   // wave-uniform
        for (int row = wv; row < DJ_H && y0 + row < H; row += 4) {
            const int si = (row + R + 1) * sp + (bx + 1), ry = row + R;
            const bool g = x < W && lab[si] == o, s = x < W && lab[per + si] == o;
            inters += __popcll(__ballot(g && s));
            uni += __popcll(__ballot(g || s));
            const bool isg = (bg[ry * DJ_NW + (bx >> 6)] >> (bx & 63)) & 1ull, iss = (bs[ry * DJ_NW + (bx >> 6)] >> (bx & 63)) & 1ull;
            const uint64_t mg = __ballot(isg), ms = __ballot(iss);
            n_gt += __popcll(mg);
            n_seg += __popcll(ms);
            const bool want_s = iss && any_g, want_g = isg && any_s;
            if (__ballot(want_s || want_g) == 0ull) continue;   // wave-uniform
            bool hit_s = false, hit_g = false;
            // rows nearest first: the loop ends as soon as every boundary pixel of the row has its partner (wave-uniform)
            for (int d = 0; d <= R; ++d) {
                const int hw = p.hw[d], lo = bx - hw, hi = bx + hw;   // 0 <= lo <= hi <= 127
                uint64_t m0 = 0ull, m1 = 0ull;
                if (lo < 64) m0 = (~0ull << lo) & (~0ull >> (63 - min(hi, 63)));
                if (hi >= 64) m1 = (~0ull << (max(lo, 64) - 64)) & (~0ull >> (127 - hi));
                for (int sgn = (d == 0 ? 1 : -1); sgn <= 1; sgn += 2) {
                    const int rr = (ry + sgn * d) * DJ_NW;
                    const uint64_t g0 = bg[rr], g1 = bg[rr + 1], s0 = bs[rr], s1 = bs[rr + 1];
                    hit_s |= ((g0 & m0) | (g1 & m1)) != 0ull;
                    hit_g |= ((s0 & m0) | (s1 & m1)) != 0ull;
                }
                if (__ballot((want_s && !hit_s) || (want_g && !hit_g)) == 0ull) break;
            }
            seg_hits += __popcll(__ballot(iss && hit_s));
            gt_hits += __popcll(__ballot(isg && hit_g));
        }
        if (lane == 0) {
            uint32_t* d = cnt + (wv * DJ_MAXN + (o - 1)) * 6;
            d[0] = inters; d[1] = uni; d[2] = n_seg; d[3] = n_gt; d[4] = seg_hits; d[5] = gt_hits;
        }
    };

    // per label: masks -> barrier -> boundary maps -> barrier -> counters; the next label's masks are packed beside this one's counting
    uint32_t rest = pres;
    int o = __ffs(rest);
    rest &= rest - 1u;
    masks(o);
    __syncthreads();
    boundary();
    __syncthreads();
    for (;;) {
        const int nxt = rest != 0u ? __ffs(rest) : 0;
        if (nxt != 0) {
            rest &= rest - 1u;
            masks(nxt);
        }
        count(o);
        __syncthreads();
        if (nxt == 0) break;
        boundary();
        __syncthreads();
        o = nxt;
    }

    if (tid < p.N * 6) {
        const int ob = tid / 6, c = tid - ob * 6;
        if ((pres >> ob) & 1u) {
            uint32_t s = 0;
#pragma unroll
            for (int w4 = 0; w4 < 4; ++w4) s += cnt[(w4 * DJ_MAXN + ob) * 6 + c];
            if (s != 0u) atomicAdd(p.counts + ((size_t)ob * p.T + t) * 6 + c, (unsigned long long)s);
        }
    }
}

}  // namespace

#define DAVIS_SERVED(cond, ...)         \
    do {                                \
        if (!(cond)) {                  \
            naf_set_error(__VA_ARGS__); \
            return NAF_ERR_UNSUPPORTED; \
        }                               \
    } while (0)

extern "C" {

int naf_davis_jf_select(const naf_davis_jf_args* a) {
    NAF_REQUIRE(a != nullptr, "naf_davis_jf: args is NULL");
    NAF_REQUIRE(a->T >= 1 && a->H >= 1 && a->W >= 1 && a->N >= 1, "naf_davis_jf: T, H, W and N must be at least 1 (got T=%d H=%d W=%d N=%d)", a->T, a->H,
                a->W, a->N);
    NAF_REQUIRE(a->half_width >= 0 && a->r2 >= 0, "naf_davis_jf: r2 and half_width must not be negative (got r2=%d half_width=%d)", a->r2, a->half_width);
    NAF_REQUIRE(a->reserved[0] == 0 && a->reserved[1] == 0, "naf_davis_jf: reserved fields must be 0");
    DAVIS_SERVED(a->half_width >= 1 && a->half_width <= DJ_MAXR,
                 "naf_davis_jf: a boundary radius of %d whole pixels is not served: 1 <= floor(bound_pix) <= 32", a->half_width);
    const int64_t hw = a->half_width;
    NAF_REQUIRE(hw * hw <= a->r2 && a->r2 < (hw + 1) * (hw + 1),
                "naf_davis_jf: r2 = %d and half_width = %d do not belong together: half_width^2 <= r2 < (half_width + 1)^2", a->r2, a->half_width);
    DAVIS_SERVED(a->N <= DJ_MAXN, "naf_davis_jf: N = %d objects are not served: 1 <= N <= 32", a->N);
    DAVIS_SERVED(a->H >= 2 && a->W >= 2, "naf_davis_jf: a %d x %d frame is not served (the reflected border needs two pixels): H, W >= 2", a->H, a->W);
    DAVIS_SERVED(a->H <= DJ_MAX_DIM && a->W <= DJ_MAX_DIM, "naf_davis_jf: a %d x %d frame is not served: H, W <= 16384", a->H, a->W);
    const int64_t tiles = (int64_t)((a->W + DJ_W - 1) / DJ_W) * ((a->H + DJ_H - 1) / DJ_H);
    DAVIS_SERVED(tiles * a->T < ((int64_t)1 << 31), "naf_davis_jf: %lld tiles in %d frames are not served: tiles * T below 2^31", (long long)tiles, a->T);
    return NAF_OK;
}

int naf_davis_jf(const naf_davis_jf_args* a, naf_stream_t stream) {
    const int rc = naf_davis_jf_select(a);
    if (rc != NAF_OK) return rc;
    NAF_REQUIRE(a->annotation && a->segmentation && a->counts, "naf_davis_jf: NULL tensor pointer");
    NAF_REQUIRE(naf_aligned(a->counts, 8), "naf_davis_jf: counts must be 8-byte aligned");
    DavisParams p;
    p.ann = a->annotation;
    p.seg = a->segmentation;
    p.counts = reinterpret_cast<unsigned long long*>(a->counts);
    p.T = a->T; p.H = a->H; p.W = a->W; p.N = a->N; p.R = a->half_width;
    p.tiles_x = (a->W + DJ_W - 1) / DJ_W;
    p.tiles = p.tiles_x * ((a->H + DJ_H - 1) / DJ_H);
    p.sp = (DJ_W + 2 * p.R + 2 + 3) & ~3;
    for (int d = 0; d <= DJ_MAXR; ++d) {
        int h = 0;
        if (d <= p.R) {
            const int v = a->r2 - d * d;   // >= 0: r2 >= R^2
            h = (int)sqrt((double)v);
            while (h * h > v) --h;
            while ((h + 1) * (h + 1) <= v) ++h;
        }
        p.hw[d] = (uint8_t)h;             // <= R: r2 < (R + 1)^2
    }
    const size_t lds = davis_lds(p.R, p.sp);
    hipLaunchKernelGGL(davis_jf_kernel, dim3((unsigned)((int64_t)p.tiles * p.T)), dim3(256), lds, static_cast<hipStream_t>(stream), p);
    return naf_check_launch("davis_jf_kernel");
}

}  // extern "C"
