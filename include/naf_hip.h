/*
 * naf_hip.h -- C ABI of libnaf_hip.so: MI355X (gfx950 / CDNA4) kernels for the NAF forward hot path.
 *
 * This is the drop-in boundary.  The reference (valeoai/NAF) is pure Python; the arithmetic of its
 * cross-scale neighbourhood attention lives behind these foreign calls:
 *
 *     natten.functional.na2d_qk / na2d_av      src/layers/attentions.py:20,24   (NATTEN <= 0.17)
 *     natten.na2d(..., backend="cutlass-fna")  src/layers/attentions.py:72      (NATTEN >= 0.20)
 *
 * plus torch-eager glue around them (nearest-exact K/V upsampling attentions.py:48-61, scale and
 * softmax :21-23, RoPE rope.py:137-174, key pooling naf.py:63-69).  Each entry point below names the
 * reference interface it replaces.  INTEGRATION.md shows the ctypes binding a maintainer would add.
 *
 * Conventions
 *   - plain C types only; every pointer marked "device" is a HIP device pointer owned by the caller.
 *   - the library allocates, retains and frees NO device memory; outputs and workspaces are the
 *     caller's.  Launches are asynchronous on the caller's hipStream_t (passed as void*), on the
 *     caller's current device.  Functions are re-entrant and the library keeps NO global mutable state beyond
 *     once-initialised kernel attributes: it owns no stream, no event, no memory.  (0.2.0 - 0.3.x kept one stream and two
 *     events per device inside naf_forward; since 0.4.0 the second stream of the forward is the caller's: naf_forward_aux.)
 *   - return value 0 = success; non-zero = error, text via naf_last_error() (thread-local).
 *     Nothing throws or aborts across the ABI.  Argument checks mirror the reference's failure modes
 *     (NATTEN: odd kernel, kernel*dilation <= extent; einops: channels divisible by heads).
 *   - strides are in ELEMENTS of the tensor's dtype.
 */
#ifndef NAF_HIP_H
#define NAF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NAF_HIP_VERSION 403 /* major*10000 + minor*100 + patch */
/* Binary compatibility: the argument structs carry no size field, so a host must be BUILT against the header of the library it
 * loads whenever the minor version differs (compare naf_version() / 100 with NAF_HIP_VERSION / 100 at start-up, as
 * examples/c_host.c does).  0.1.x appended fields to naf_xna_bwd_args (workspace) and naf_forward_args (phase_events): hosts
 * that zero-initialise the structs stay source-compatible; since 0.2.0 new capabilities arrive as new entry points with their
 * own structs (naf_stem_conv_keys_fwd / naf_key_pool_args) instead of growing existing ones.  0.3.0 changed the LAYOUT of the
 * GroupNorm-sum buffers of the stem entry points ([B][8][2] -> [NAF_STATS_SLOTS][B][8][2], see "guidance conv stem") and the order
 * of w_packed for the 3x3 layers of the default width (naf_stem_weight_index; also naf_stem_branch.conv_weight_packed of naf_forward):
 * a 0.2.x host must be rebuilt, allocate the larger buffers and repack those weights; the attention entries are unchanged.
 * 0.4.0 makes that break DETECTABLE: the entry points that read or write GroupNorm-sum buffers are exported under names that
 * carry the copy count (naf_stem_conv0_fwd -> naf_stem_conv0_fwd_s16, ...; the #defines below keep the source names and paste
 * NAF_STATS_SLOTS into the exported ones), so a binary
 * built against a 0.2.x / 0.3.x header fails to resolve them at load time instead of overrunning its [B][8][2] buffers, and
 * naf_abi_check(NAF_HIP_VERSION) lets a host compare the header it was compiled with against the library it loaded in one call.
 * 0.4.0 also appends `flags` to naf_stem_conv0_args and adds naf_forward_ex / naf_forward_aux (caller-owned second stream);
 * naf_forward itself is unchanged in signature and now runs on the caller's stream only.
 * 0.4.1 (binary compatible with 0.4.0): naf_xna_bwd_args.reserved -- documented as 0 -- becomes `path` (0 = NAF_XNA_AUTO: the
 * behaviour of 0.4.0), and the cell backward takes 13 x 13 windows at every Dv and 15 x 15 windows (channel chunks).
 * 0.4.2 (binary compatible with 0.4.x): the training-side stem entries serve every width the forward serves (multiples of 16 up to
 * 256, the reference's denoising models): naf_stem_wgrad_args and naf_stem_conv0_wgrad_args gain `channels` in what was alignment
 * padding (a zero-initialised struct of an older host reads 0 = 128, struct sizes and all other offsets unchanged), the plain mode
 * of naf_stem_conv_fwd and naf_stem_act_fwd / _bwd lose their 128- / 64-multiple restrictions; naf_forward_workspace_bytes_ex; the cell
 * backward takes cells of 14 / 15 / 28 / 30 ... pixels per row at windows up to 9 x 9 (naf_xna_bwd_supported then says NAF_XNA_MFMA where
 * 0.4.1 said NAF_XNA_ROWS: no tables / workspace needed any more).
 * 0.4.3 (binary compatible with 0.4.x: a new entry point only): naf_xna_bwd_scores / naf_xna_bwd_scores_supported -- the attention backward
 * with a gradient of the scaled scores naf_xna_fwd returns in `logits` (naf_xna_bwd_scores_args), so that a loss on the scores trains q and k.
 * After 0.4.3, same version number (binary compatible: new entry points with a struct of their own, nothing else moves): naf_xna_head_select /
 * naf_xna_head_fwd / naf_xna_head_workspace_bytes -- the attention with a linear head folded in (naf_xna_head_args).  A host detects them by symbol
 * (dlsym), not by naf_version().  Added the same way after them: naf_xna_head_ce_select / naf_xna_head_ce_fwd -- that attention with a
 * cross-entropy / argmax epilogue (naf_xna_head_ce_args, which embeds naf_xna_head_args unchanged); and after those naf_xna_head_cm_select /
 * naf_xna_head_cm_fwd -- that epilogue counting into a confusion matrix (naf_xna_head_cm_args, which embeds naf_xna_head_ce_args unchanged); and after
 * those naf_propagate_select / naf_propagate_fwd / naf_feature_inv_norm -- label propagation for video evaluation (naf_propagate_args); and after
 * those naf_denoise_objective / naf_denoise_workspace_bytes -- the denoising loss with its gradient, and the PSNR / SSIM metrics (naf_denoise_args); and after
 * those naf_feature_moments (+ _workspace_bytes, _plan) / naf_pca_project (+ _workspace_bytes) / naf_pca_minmax -- feature PCA for display; and after
 * those naf_xna_mse_supported / naf_xna_mse_workspace_bytes / naf_xna_mse_fwd -- the attention forward with the training objective (mean squared error
 * against a target) in its epilogue (naf_xna_mse_args, which embeds naf_xna_args unchanged); and after those naf_davis_jf_select / naf_davis_jf --
 * the integer counts behind the DAVIS J and F measures of two label-map sequences (naf_davis_jf_args); and after those naf_mask_labels_select /
 * naf_mask_labels / naf_nearest_resize_table -- a propagated frame's soft masks to the label map the reference writes to disk (naf_mask_labels_args);
 * and after those naf_xna_points -- the attention's scores, weights and features at N query pixels (naf_xna_points_args); and after that
 * naf_propagate_plan -- the kernel instance, key blocks, buffering and LDS naf_propagate_fwd chooses (host-only, naf_propagate_args unchanged); and
 * after that naf_image_prep_select / naf_image_prep -- resized, normalised views of one decoded frame from one launch (naf_image_prep_args); and
 * after those naf_xna_cos_select / naf_xna_cos_fwd -- the attention with a cosine head folded in: scaled cosines between the upsampled feature
 * and N embeddings, and the feature's norm (naf_xna_cos_args); and after those naf_xna_cos_ce_select / naf_xna_cos_ce_fwd -- that
 * attention with a cross-entropy on the scaled cosines in its epilogue: loss, labels, the gradient for the embeddings' projection and
 * for the scale (naf_xna_cos_ce_args, which embeds naf_xna_cos_args unchanged); and, the same way, naf_xna_head_reg_select /
 * naf_xna_head_reg_workspace_bytes / naf_xna_head_reg_fwd -- the attention with a linear head and a dense regression objective in its
 * epilogue: L1 / MSE / smooth-L1 loss map, its gradient, and the error statistics of depth evaluation (naf_xna_head_reg_args, which embeds
 * naf_xna_head_args unchanged). */
/* The copy count is part of the ABI and the export names are DERIVED from it (round 6): a library built with another value
 * (-DNAF_STATS_SLOTS=8) exports naf_stem_conv0_fwd_s8, ..., so that a host holding [16][B][8][2] buffers cannot resolve them. */
#ifndef NAF_STATS_SLOTS
#define NAF_STATS_SLOTS 16 /* copies of every GroupNorm-sum buffer (see "guidance conv stem" below) */
#endif
#define NAF_ABI_PASTE2(name, slots) name##_s##slots
#define NAF_ABI_PASTE(name, slots) NAF_ABI_PASTE2(name, slots)
#define naf_stem_conv0_fwd NAF_ABI_PASTE(naf_stem_conv0_fwd, NAF_STATS_SLOTS)
#define naf_stem_conv_fwd NAF_ABI_PASTE(naf_stem_conv_fwd, NAF_STATS_SLOTS)
#define naf_stem_conv_keys_fwd NAF_ABI_PASTE(naf_stem_conv_keys_fwd, NAF_STATS_SLOTS)
#define naf_stem_act_fwd NAF_ABI_PASTE(naf_stem_act_fwd, NAF_STATS_SLOTS)
#define naf_stem_act_bwd NAF_ABI_PASTE(naf_stem_act_bwd, NAF_STATS_SLOTS)
#define naf_stem_wgrad NAF_ABI_PASTE(naf_stem_wgrad, NAF_STATS_SLOTS)

typedef void* naf_stream_t; /* hipStream_t */

/* NAF_F16 (IEEE half): only where naf_dtype_supported says so -- the VALUES and the output of the attention forward.  Every other
 * dtype field of this header keeps taking NAF_BF16 / NAF_F32 and rejects it. */
enum naf_dtype { NAF_BF16 = 0, NAF_F32 = 1, NAF_F16 = 2 };

enum naf_status {
    NAF_OK = 0,
    NAF_ERR_INVALID = 1,     /* bad argument (shape / dtype / alignment / NULL) */
    NAF_ERR_UNSUPPORTED = 2, /* valid request this build has no kernel for */
    NAF_ERR_LAUNCH = 3       /* HIP runtime reported an error */
};

enum naf_xna_path {
    NAF_XNA_AUTO = 0,    /* pick: MFMA cell kernel, else table-driven MFMA kernel, else generic kernel */
    NAF_XNA_MFMA = 1,    /* integer ratio Ho = dy*h, Wo = dx*w; one workgroup per (cell, head) */
    NAF_XNA_GENERIC = 2, /* any sizes, head dims, rectangular windows; needs idx_y / idx_x (any tables) */
    NAF_XNA_UNION = 3,   /* any ratio >= 1 on the matrix cores (Dq = 64, Dv % 16 == 0, square window <= 15); needs
                            idx_y / idx_x and they MUST be the canonical tables of naf_axis_index_table: the library
                            sizes its LDS windows from the same rule.  Other tables: NAF_XNA_GENERIC. */
    NAF_XNA_ROWS = 4     /* row-streaming matrix-core kernel for the head shapes the others do not take: Dq any of
                            {64, 96, 128, 192, 256, 384, 512}, Dv <= 64 (the denoising call: one head, C = 3), square
                            window <= 15, any ratio >= 1; needs the canonical idx_y / idx_x like NAF_XNA_UNION */
};

/* ---- library ------------------------------------------------------------------------------- */
int naf_version(void);
const char* naf_last_error(void);
/* NAF_OK when a host compiled against a header of version `header_version` (pass NAF_HIP_VERSION) may call this library:
 * same major and minor version.  NAF_ERR_INVALID (with the two versions in naf_last_error()) otherwise.  0.4.0. */
int naf_abi_check(int header_version);
/* Which dtypes an argument takes (new entry point; detect by symbol, version number unchanged): 1 when argument `what` accepts
 * naf_dtype `dtype`, 0 when it does not (or `what` is unknown).  A library without this symbol knows no NAF_F16 anywhere.
 * Half values through the attention forward (naf_xna_fwd with out_dtype NAF_F16; naf_forward with feat_dtype = out_dtype = NAF_F16):
 * the values are read as IEEE half and never rounded to bf16, the PV product runs on v_mfma_f32_16x16x32_f16 with fp32
 * accumulation and the output is stored as half.  Queries, keys, the stem, RoPE and the scores are bf16 / fp32 as for the other dtypes.
 * No subnormal OPERAND is relied on: the softmax weights are multiplied by 2^8 before they are rounded to half and the fp32
 * accumulator (or normaliser) by 2^-8 before the store, both exact, so a weight only vanishes below 2^-22.  Per element, against the
 * exact result on the same half values: |err| <= 1.25 * 2^-11 * (sum_j p_j |v_j| + |ref|) + k*k * 2^-22 * max|v| + 2^-14 (one rounding
 * of P plus the store; every window weight flushed; subnormal values flushed).  Half and bf16 / fp32 never mix in one call. */
enum naf_dtype_arg {
    NAF_DT_XNA_VALUES = 0,   /* naf_xna_args.v_lr: NAF_BF16, or NAF_F16 (then out_dtype must be NAF_F16 too) */
    NAF_DT_XNA_OUT = 1,      /* naf_xna_args.out_dtype: NAF_BF16 / NAF_F32 (bf16 values), NAF_F16 (half values) */
    NAF_DT_PACK_SRC = 2,     /* naf_pack_values v_dtype: NAF_BF16 / NAF_F32 -> bf16, NAF_F16 -> half (an exact copy) */
    NAF_DT_FWD_FEAT = 3,     /* naf_forward_args.feat_dtype */
    NAF_DT_FWD_OUT = 4       /* naf_forward_args.out_dtype (NAF_F16 exactly when feat_dtype is) */
};
int naf_dtype_supported(int what, int dtype);

/* ---- host helper: which low-res rows/cols a hi-res query attends to (one axis) ------------------
 * Replaces, for one axis, NATTEN's neighbourhood rule composed with the reference's nearest-exact
 * upsampling of K/V (attentions.py:48-61 + NATTEN get_window_start, dilation = L_out / L_in).
 * out_host[L_out * k] (HOST memory).  Errors like NATTEN: k even, k*dilation > L_out, L_out < L_in. */
int naf_axis_index_table(int32_t* out_host, int32_t L_out, int32_t L_in, int32_t k);
/* The same table computed on the device (out_dev: device int32 [L_out * k]), bit-identical to the host one:
 * for hosts that stay off the CPU path (naf_forward builds its tables this way; capturable in a hipGraph). */
int naf_axis_index_table_device(int32_t* out_dev, int32_t L_out, int32_t L_in, int32_t k, naf_stream_t stream);

/* ---- guidance conv stem ----------------------------------------------------------------------------
 * Replaces the reference's encoder() branches (convolutions.py:6-92, built at naf.py:26-27 with
 * hidden = dim/2 = 128 channels, GroupNorm(8), SiLU, reflect padding, no residual) for the default
 * width.  Activations are channels-last bf16 [B, H, W, 128]; GroupNorm statistics travel as fp64
 * {sum, sum of squares} per (batch, group) in `stats` buffers [NAF_STATS_SLOTS][B][8][2] that the CALLER
 * zeroes before the producing launch (hipMemsetAsync on the same stream): NAF_STATS_SLOTS partial copies -- a
 * producing workgroup adds into copy (workgroup index mod NAF_STATS_SLOTS), a consumer adds the copies up; the sums
 * of (b, g) are the sum over the first axis.  (One copy per image is one 128-byte line; device-scope atomics to one line
 * are served one after another, and with a single copy the 4096 atomics of a 256-workgroup launch held its end back by
 * 17-20 us: profiles/r04_stats_atomics.txt.)  Since 0.3.0; 0.2.x had one copy.
 *
 * naf_stem_conv0_fwd : Conv2d(3 -> 128, ksize 1 or 3, reflect) + bias         (convolutions.py:68-75)
 *   fp32 accumulation; products exact in fp32 for ksize 1, carried to 16 mantissa bits for ksize 3 at the default width (the sum
 *   is within 2^-15 * sum |x||w| of the fp32 convolution before its one rounding to bf16; flags & NAF_CONV0_EXACT: exact products);
 *   image device [B, 3, H, W] f32/bf16, element strides {b, c, y, x}; weight device f32 [128][3][k][k]
 *   (the module's own parameter), bias f32 [128]; y device bf16, strides {b, y, x}, 128 ch contiguous;
 *   stats_out accumulates sum / sum^2 of y per GroupNorm group (zeroed by the caller).  y may be NULL: statistics only
 *   (for naf_stem_conv_args.first below); with ksize 1 they are then computed from the image's first and second
 *   moments (y is linear in the image), which agrees with the sums of the stored pass to ~1e-7 relative.
 * Both entries take `channels` = the hidden width C (convolutions.py:67-92 with dim / 2 channels per branch; the
 *   reference's denoising models use dim 96 ... 512, denoising.py:213): 128 (or 0) selects the hand-scheduled kernels of
 *   the default model, any other multiple of 16 up to 256 the general kernels of stem_generic.hip; "128" below reads C.
 * naf_stem_conv_fwd  : GroupNorm(8,128) -> SiLU -> Conv2d(128 -> 128, ksize 1 or 3, reflect) + bias
 *   (one norm/act/conv triple of EncBlock.forward, convolutions.py:52-61).  x device bf16 with its
 *   stats_in; gn_weight/gn_bias f32 [128]; w_packed device bf16, k*k*C*C elements, element (tap, oc, ic) at
 *   naf_stem_weight_index(ksize, C, tap, oc, ic): [k*k][C oc][C ic] (= weight.permute(2,3,0,1)) except for the 3x3 layers of
 *   the default width (ksize 3, C = 128; since 0.3.0), whose kernel keeps all 288 KB of weights in registers and wants them in the
 *   order its lanes hold them -- [9 taps][4 blocks of 32 oc][8 steps of 16 ic][2 halves of 8 ic][32 oc][8 ic], every load
 *   instruction of a wave one contiguous KB (the [oc][ic] order cost each launch 4.7 us more, profiles/r04_stats_atomics.txt);
 *   y / stats_out as above (stats_out may be NULL).
 *   `first` (optional, ksize 1 only): the layer is the FIRST residual-block convolution of the 1x1 branch and
 *   recomputes its input bf16(conv0(image)) from `first` (image, weight, bias of the 1x1 conv0; first->y and
 *   first->stats_out are ignored) instead of reading x, so that the conv0 activation never exists in memory;
 *   128 channels only;
 *   stats_in then are the sums a naf_stem_conv0_fwd(y = NULL) call produced.  Given the same stats_in the results
 *   are bit-identical to the two-call sequence. */
/* NAF_STATS_SLOTS (defined at the top, beside the export names it versions) = copies of every GroupNorm-sum buffer. */
/* Bytes of ONE GroupNorm-sum buffer for a batch of B images as THIS library lays it out ([NAF_STATS_SLOTS][B][8][2] fp64): what a
 * host allocates per `stats` pointer instead of hard-coding the shape (0 for B <= 0).  0.4.0. */
size_t naf_stem_stats_bytes(int32_t B);
/* naf_stem_conv0_args.flags */
#define NAF_CONV0_EXACT 1 /* ksize 3, default width: all six bf16-split terms (products exact in fp32) instead of the default three */
typedef struct naf_stem_conv0_args {
    const void* image;
    void* y;
    const float* weight;
    const float* bias;
    double* stats_out;
    int32_t image_dtype; /* naf_dtype */
    int32_t ksize;       /* 1 or 3 */
    int32_t B, H, W;
    int32_t channels;    /* output channels: 0 or 128 = the default width's kernels; any multiple of 16 in [16, 256] otherwise */
    int64_t image_stride[4];
    int64_t y_stride[3];
    int32_t flags;       /* 0.4.0: NAF_CONV0_* bits; 0 = defaults */
    int32_t reserved;
} naf_stem_conv0_args;
int naf_stem_conv0_fwd(const naf_stem_conv0_args* a, naf_stream_t stream);

typedef struct naf_stem_conv_args {
    const void* x;
    void* y;
    const void* w_packed;
    const float* bias;
    const float* gn_weight;
    const float* gn_bias;
    const double* stats_in;
    double* stats_out;
    int32_t ksize; /* 1 or 3 */
    int32_t B, H, W;
    float eps;
    int32_t channels;    /* channels of x and y: 0 or 128 = the default width's kernels; any multiple of 16 in [16, 256] otherwise */
    int64_t x_stride[3];
    int64_t y_stride[3];
    const naf_stem_conv0_args* first; /* optional, see above */
} naf_stem_conv_args;
int naf_stem_conv_fwd(const naf_stem_conv_args* a, naf_stream_t stream);
/* Index of element (tap = ty * ksize + tx, oc, ic) in w_packed for a layer of `channels` channels (host function, no device
 * work; -1 for arguments out of range).  0.3.0. */
int64_t naf_stem_weight_index(int32_t ksize, int32_t channels, int32_t tap, int32_t oc, int32_t ic);
/* Plain mode: stats_in == gn_weight == gn_bias == NULL (bias may be NULL too) -> y = conv(x) (+ bias), no GroupNorm, no SiLU,
 * 128 channels.  It is the DATA GRADIENT of a layer (the backward train.py:127-137 needs): x = the gradient of the layer's
 * output, w_packed = the flipped, transposed weights (those of Conv2d with weight.flip(2,3).transpose(0,1), packed as above).  For the
 * 3x3 layers (reflect padding) run it over the output gradient embedded in a 2-pixel ZERO border ((H+4) x (W+4)): rows /
 * columns 1 .. H+2 of the result are the gradient on the padded domain, whose border naf_stem_act_bwd(fold) folds back. */

/* naf_stem_conv_keys_fwd (0.2.0): naf_stem_conv_fwd for the LAST block layer of a branch, which ALSO writes that branch's
 * slice of the pooled keys -- KeyEncoder's adaptive_avg_pool2d of the RoPE'd guidance (naf.py:63-69 after rope.py:139-153) --
 * so that no pass re-reads the guidance.  It uses that the rotation is AXIAL (rope.py:139-143: inside a 64-wide head, dims
 * [0,16) u [32,48) turn by the ROW angle only, [16,32) u [48,64) by the COLUMN angle only) and that pooling is linear:
 * the mean of the rotated pixels of a cell = the rotation, by row r's angle, of the cell's un-rotated sum over its columns in row r
 * (row-angle dims), resp. by column c's angle of the sum over its rows in column c (column-angle dims).  The kernel takes those
 * sums of the bf16 outputs it has just produced (on the matrix pipe, from the tile that is in the LDS for the row stores),
 * rotates the 16 + 16 sums per channel pair in fp32 and writes bf16 keys: the same guidance values the queries are read from.
 *   a        as for naf_stem_conv_fwd: 128 channels, stats_out == NULL, first == NULL, GroupNorm / SiLU mode
 *   kp->k_lr device bf16, the branch's 128 key channels: [B, h, w, >= 128] by k_stride = {b, y, x} (pointer at the slice's
 *            first channel); tab_y / tab_x the tables of naf_rope_tables for (H, W) with 16 periods (heads of 64 channels)
 *   16 x 16 pixel cells only: H == 16 h, W == 16 w, W a multiple of 32 for ksize 3.
 * naf_stem_conv_keys_supported: 1 when this call would be served, 0 when the caller has to run naf_stem_conv_fwd and
 * naf_rope_pool_fwd instead, negative naf_status on invalid arguments. */
typedef struct naf_key_pool_args {
    void* k_lr;
    const float* tab_y; /* [H][2][16] */
    const float* tab_x; /* [W][2][16] */
    int32_t h, w;
    int64_t k_stride[3];
} naf_key_pool_args;
int naf_stem_conv_keys_supported(const naf_stem_conv_args* a, const naf_key_pool_args* kp);
int naf_stem_conv_keys_fwd(const naf_stem_conv_args* a, const naf_key_pool_args* kp, naf_stream_t stream);

/* ---- training companions of the conv stem --------------------------------------------------------------
 * naf_stem_act_fwd : a = SiLU(GroupNorm(8, C)(x)) in bf16 (convolutions.py:52-55 / :58-59, the tensor naf_stem_conv_fwd never
 *   stores), written with a reflected border of `pad` pixels (0 or 1): a is [B, H + 2 pad, W + 2 pad, C] by a_stride =
 *   {b, y, x}.  It is the input of the layer's weight gradient.
 * naf_stem_act_bwd : backward of the same function.  da = gradient wrt a (bf16; with fold = 1 the gradient on the PADDED
 *   domain [B, H + 2, W + 2, C], pointer at its first element: the adjoint of the reflect padding is applied on load), x and
 *   stats_in = the forward's input and its GroupNorm sums; dx (bf16) = gradient wrt x.  sums [B][C][2] (fp64, zeroed by the
 *   caller) receives per sample and channel {sum dz, sum dz * xhat} = the contributions to the gradients of gn_bias /
 *   gn_weight.  phase 1 = sums only, 2 = dx only (sums must be complete), 0 = both.  C a multiple of 64 up to 256. */
typedef struct naf_stem_act_args {
    const void* x;
    void* a;
    const float* gn_weight;
    const float* gn_bias;
    const double* stats_in;
    int32_t B, H, W;
    int32_t channels; /* 0 = 128 */
    int32_t pad;      /* 0 or 1 */
    float eps;
    int64_t x_stride[3];
    int64_t a_stride[3];
} naf_stem_act_args;
int naf_stem_act_fwd(const naf_stem_act_args* a, naf_stream_t stream);

typedef struct naf_stem_act_bwd_args {
    const void* da;
    const void* x;
    void* dx;
    const float* gn_weight;
    const float* gn_bias;
    const double* stats_in;
    double* sums;
    int32_t B, H, W;
    int32_t channels; /* 0 = 128 */
    int32_t fold;     /* 1: da lives on the padded domain, fold its border back */
    int32_t phase;    /* 0 both, 1 sums, 2 dx */
    float eps;
    int64_t da_stride[3];
    int64_t x_stride[3];
    int64_t dx_stride[3];
} naf_stem_act_bwd_args;
int naf_stem_act_bwd(const naf_stem_act_bwd_args* a, naf_stream_t stream);

/* naf_stem_wgrad : weight gradient of a layer y = conv(SiLU(GroupNorm(x))) + bias (convolutions.py:52-61), 128 channels:
 *   dw[ty][tx][oc][ic] += sum over pixels of dy[., oc] * a_reflect_padded[. + (ty, tx), ic], a recomputed from x / stats_in on the
 *   fly (never materialised).  dy, x device bf16 [B, H, W, 128] by strides {b, y, x}; dw device f32 [k][k][128 oc][128 ic]
 *   (= weight.grad.permute(2, 3, 0, 1): taps outermost keeps the atomics coalesced), ACCUMULATED: zero it first.  ksize 1 or 3.
 *   stats_in == NULL: x already IS a (the unpadded output of naf_stem_act_fwd) -- the faster sequence: the activation arithmetic
 *   runs once in a bandwidth-bound kernel instead of three times in front of the matrix instructions. */
typedef struct naf_stem_wgrad_args {
    const void* dy;
    const void* x;
    float* dw;
    float* db;        /* optional f32 [128], ACCUMULATED (zero it first): sum of dy over pixels = the bias gradient */
    const float* gn_weight;
    const float* gn_bias;
    const double* stats_in;
    int32_t ksize;
    int32_t B, H, W;
    float eps;
    int32_t channels; /* 0.4.2 (was alignment padding): C, a multiple of 16 up to 256; 0 = 128.  dw is f32 [k][k][C oc][C ic], db [C] */
    int64_t dy_stride[3];
    int64_t x_stride[3];
} naf_stem_wgrad_args;
int naf_stem_wgrad(const naf_stem_wgrad_args* a, naf_stream_t stream);

/* naf_stem_conv0_wgrad : weight and bias gradient of the first convolution (3 -> 128, ksize 1 or 3, reflect; convolutions.py:68-75):
 *   dw[(c * k + ty) * k + tx][oc] += sum over pixels of dy[., oc] * image_reflect_padded[. + (ty, tx), c]   (f32 [3*k*k][128] =
 *   weight.grad.permute(1, 2, 3, 0)), db[oc] += sum of dy; both ACCUMULATED (zero them first).  dy device bf16 [B, H, W, 128] by
 *   strides {b, y, x}; image device f32 / bf16 by strides {b, c, y, x} as in naf_stem_conv0_fwd. */
typedef struct naf_stem_conv0_wgrad_args {
    const void* dy;
    const void* image;
    float* dw;
    float* db;
    int32_t image_dtype; /* naf_dtype */
    int32_t ksize;
    int32_t B, H, W;
    int32_t channels; /* 0.4.2 (was alignment padding): C of the convolution 3 -> C, a multiple of 16 up to 256; 0 = 128.  dw [3*k*k][C], db [C] */
    int64_t dy_stride[3];
    int64_t image_stride[4];
} naf_stem_conv0_wgrad_args;
int naf_stem_conv0_wgrad(const naf_stem_conv0_wgrad_args* a, naf_stream_t stream);

/* naf_stem_conv0_dgrad (0.4.2) : gradient of the first convolution w.r.t. the IMAGE (what autograd runs through Conv2d(3 -> C,
 *   padding_mode="reflect") of convolutions.py:68-75 when the image requires a gradient): dimage[b, c, y, x] (= or +=, `accumulate`)
 *   sum over output pixels and taps that read (y, x) -- through the reflection too -- of dy[., oc] * weight[oc][c][ty][tx].
 *   dy device bf16 [B, H, W, C] by strides {b, y, x} (channels contiguous); weight device f32 [C][3][k][k] contiguous (the
 *   parameter); dimage device f32 by element strides {b, c, y, x}.  ksize 1 or 3; channels a multiple of 16 up to 256 (0 = 128). */
typedef struct naf_stem_conv0_dgrad_args {
    const void* dy;
    const float* weight;
    float* dimage;
    int32_t ksize;
    int32_t B, H, W;
    int32_t channels;
    int32_t accumulate; /* 0: dimage is written; 1: added to (the second branch of the stem) */
    int64_t dy_stride[3];
    int64_t dimage_stride[4];
} naf_stem_conv0_dgrad_args;
int naf_stem_conv0_dgrad(const naf_stem_conv0_dgrad_args* a, naf_stream_t stream);

/* ---- RoPE tables --------------------------------------------------------------------------------
 * Replaces RoPE.create_coordinate + the angle/sin/cos part of RoPE.rotate (rope.py:84-105,137-146),
 * eval mode.  tab_y device float [Ho][2][n_periods] (cos then sin), tab_x device float [Wo][2][..].
 * periods: device float [n_periods] (the module's persistent buffer, rope.py:77-81). */
int naf_rope_tables(float* tab_y, float* tab_x, const float* periods, int32_t n_periods, int32_t Ho,
                    int32_t Wo, naf_stream_t stream);

/* ---- RoPE + query write + key pooling, one pass ----------------------------------------------------
 * Replaces RoPE.forward's rotation (rope.py:147-174), the identity QueryEncoder (naf.py:55-60) and
 * KeyEncoder's adaptive_avg_pool2d of the ROTATED guidance (naf.py:63-69).
 *   x      device, x_dtype, logical [B, Cq, Ho, Wo], element strides x_stride = {b, c, y, x}
 *   q      device bf16, logical [B, heads, Ho, Wo, Dh], strides q_stride = {b, head, y, x}, Dh contiguous
 *   k_lr   device bf16, logical [B, heads, h, w, Dh],   strides k_stride = {b, head, y, x}, Dh contiguous
 * Dh = Cq / heads, Dh % 4 == 0.  Pool window of low-res row i: [floor(i*Ho/h), ceil((i+1)*Ho/h)).
 * q may be NULL: keys only (the queries are then rotated on load by naf_xna_fwd, see rope_tab_y there).
 * Layouts.  Any strides of x, q and k_lr are honoured, each operand's on its own.  The VECTOR path (8 channels per 16-byte
 * access) serves a call when ALL of these hold:
 *   - Dh is a multiple of 32;
 *   - x, q (where it is not NULL), tab_y and tab_x are 16-byte aligned;
 *   - the four strides of q are multiples of 8 elements;
 *   - where the channels of x are contiguous (x_stride[1] == 1), its strides {b, y, x} are multiples of 16 bytes (8 bf16 or 4
 *     float elements); with any other channel stride x is loaded element by element inside the vector path.
 * Every other call is served element by element: the same queries bit for bit, the keys up to the order of their fp32 sums, slower
 * (and refused with NAF_ERR_UNSUPPORTED when Cq / 2 exceeds 256, the pair-chunks a pixel has threads for).  k_lr is stored element
 * by element on both paths: no alignment. */
typedef struct naf_rope_pool_args {
    const void* x;
    void* q;
    void* k_lr;
    const float* tab_y; /* [Ho][2][Dh/4] */
    const float* tab_x; /* [Wo][2][Dh/4] */
    int32_t x_dtype;    /* naf_dtype */
    int32_t B, Cq, heads, Ho, Wo, h, w;
    int64_t x_stride[4];
    int64_t q_stride[4];
    int64_t k_stride[4];
} naf_rope_pool_args;
int naf_rope_pool_fwd(const naf_rope_pool_args* a, naf_stream_t stream);

/* Backward of naf_rope_pool_fwd (train.py:127-137 differentiates rope.py:147-174 and naf.py:63-69):
 *   dx = R^T (dq + sum over the cells whose pooling window holds the pixel of dk / window size), R^T = rotation by the negative angle.
 *   dq device bf16 [B, heads, Ho, Wo, Dh], dk_lr device f32 [B, heads, h, w, Dh], strides {b, head, y, x} with Dh contiguous;
 *   dx device bf16, strides {b, c, y, x} with c contiguous (dx_stride[1] == 1); Dh a multiple of 32; tables as in the forward. */
typedef struct naf_rope_pool_bwd_args {
    const void* dq;
    const float* dk_lr;
    void* dx;
    const float* tab_y;
    const float* tab_x;
    int32_t B, Cq, heads, Ho, Wo, h, w;
    int64_t dq_stride[4];
    int64_t dk_stride[4];
    int64_t dx_stride[4];
} naf_rope_pool_bwd_args;
int naf_rope_pool_bwd(const naf_rope_pool_bwd_args* a, naf_stream_t stream);

/* ---- image pre-shrink -----------------------------------------------------------------------------------
 * Replaces the F.interpolate(mode="bilinear", align_corners=False) of ImageEncoder.forward (naf.py:39-48) that the
 * reference applies to images more than 4x the output size: image device f32 / bf16 [B, 3, H, W], strides {b, c, y, x}
 * -> out device float dense [B, 3, Hs, Ws]; ATen's arithmetic, no antialiasing.  The target size
 * (min(H, 4*Ho, 4*Wo), min(W, 4*Wo, 4*Ho)) is the caller's to compute (naf_forward does it itself). */
int naf_preshrink_image(float* out, const void* image, int32_t image_dtype, int32_t B, int32_t H, int32_t W, int32_t Hs,
                        int32_t Ws, const int64_t image_stride[4], naf_stream_t stream);

/* ---- guidance pooling ---------------------------------------------------------------------------------
 * Replaces F.adaptive_avg_pool2d(x, output_size) of ImageEncoder.encode (naf.py:34) when image and output size differ: x device bf16 dense channels-last [B, H, W, C] -> y device bf16 dense channels-last [B, Ho, Wo, C],
 * C % 8 == 0, both 16-byte aligned; windows [floor(i*H/Ho), ceil((i+1)*H/Ho)) like torch, fp32 accumulation. */
int naf_pool_guidance(void* y, const void* x, int32_t B, int32_t H, int32_t W, int32_t Ho, int32_t Wo, int32_t C,
                      naf_stream_t stream);

/* ---- backward of the guidance pooling and of the image pre-shrink (new entry points; detect by symbol, version number unchanged) ----
 * What train.py:126-137 differentiates when the guidance image is larger than the output (its own call: 4x per axis).
 * naf_pool_guidance_bwd is the adjoint of naf_pool_guidance: dy device bf16 dense channels-last [B, Ho, Wo, C] -> dx device bf16 dense
 * channels-last [B, H, W, C], C % 8 == 0, both 16-byte aligned.  Gather form: dx[y, x] = sum over the windows that hold (y, x) of
 * float(dy) * (1.0f / area), output rows floor(y*Ho/H) .. ceil((y+1)*Ho/H) - 1 ascending, then columns ascending, fp32, one rounding to
 * bf16; no atomics, bit-reproducible.  Any H, Ho (an output larger than the image too).
 * naf_preshrink_image_bwd is the adjoint of naf_preshrink_image with respect to the image: dout device float dense [B, 3, Hs, Ws] ->
 * dimage device f32 / bf16 [B, 3, H, W], strides {b, c, y, x}; every element is written, zeros included.  The weights are the forward's own
 * fp32 expressions; each term is fl(fl(h * w) * g), summed in fp32 in a fixed order (output rows ascending, columns ascending); no atomics,
 * bit-reproducible.  Serves Hs <= H and Ws <= W (all naf.py:39-48 produces); NAF_ERR_UNSUPPORTED otherwise.
 * Both: NAF_ERR_INVALID, before any device work and with naf_last_error() set, for NULL pointers, sizes <= 0, C % 8 != 0, a misaligned
 * buffer, an unknown dtype or more than 2^31 - 1 workgroups.  Caller-owned memory and stream; capturable; no workspace. */
int naf_pool_guidance_bwd(void* dx, const void* dy, int32_t B, int32_t H, int32_t W, int32_t Ho, int32_t Wo, int32_t C,
                          naf_stream_t stream);
int naf_preshrink_image_bwd(void* dimage, const float* dout, int32_t image_dtype, int32_t B, int32_t H, int32_t W, int32_t Hs,
                            int32_t Ws, const int64_t image_stride[4], naf_stream_t stream);

/* ---- value packing --------------------------------------------------------------------------------
 * Replaces the rearrange + dtype cast of the value tensor in CrossAttention._resize
 * (attentions.py:50-51) WITHOUT the nearest-exact upsampling (values stay low-res).
 *   v  device, v_dtype, logical [B, C, h, w], strides {b, c, y, x};   vp device bf16 [B, h, w, C] dense.
 *   v_dtype NAF_F16: vp is IEEE half [B, h, w, C] dense, an exact copy (what naf_xna_fwd reads with out_dtype NAF_F16). */
int naf_pack_values(void* vp, const void* v, int32_t v_dtype, int32_t B, int32_t C, int32_t h, int32_t w,
                    const int64_t v_stride[4], naf_stream_t stream);

/* ---- LAYOUT CONTRACT OF THE ATTENTION ENTRIES ------------------------------------------------------
 * naf_xna_fwd, naf_xna_head_fwd, naf_xna_head_ce_fwd, naf_xna_cos_fwd, naf_xna_mse_fwd, naf_xna_bwd (and naf_xna_bwd_scores) take every 5-D operand as
 * a pointer plus four ELEMENT strides {b, head, y, x}; the last dim is contiguous.  Each stride of each operand is honoured on its own:
 * nothing is derived from another stride, from a size or from another operand, so dense head-major and channels-last buffers, gaps
 * between pixels, rows, heads or images, windows of a larger canvas, channel slices, a batch axis that is not the outermost, y stride <
 * x stride and stride 0 on a READ-ONLY operand (an operand expanded over the batch or the head axis) are all the same call.  Strides
 * are non-negative and outputs must not overlap themselves.  A call writes the elements of its outputs and nothing else -- no byte
 * between or next to them, partial tiles included -- and never writes an input; what lies between or next to the elements of an input
 * is never read into a result.  Dense by contract: `logits` of naf_xna_fwd, dk_lr / dv_lr and the workspace of naf_xna_bwd, `loss` and
 * the workspace of naf_xna_mse_fwd; the call stays inside the sizes the header gives for them.
 *
 * The matrix-core kernels read 16-byte chunks: they are ELIGIBLE for operands whose pointer is 16-byte aligned and whose four strides
 * are multiples of 8 elements ("vectorisable"; `out` of naf_xna_fwd: 16-byte aligned, strides multiples of 4).  What a layout outside
 * that gets, per entry (tests/test_layout_contract_cpu.py holds this table against the *_select / *_supported queries):
 *   naf_xna_fwd    q or k_lr not vectorisable: NAF_XNA_GENERIC under AUTO (rotate-on-load: -NAF_ERR_UNSUPPORTED, no other kernel rotates).
 *                  v_lr or out not vectorisable: NAF_XNA_ROWS where the shape is that kernel's (it reads values and writes the output
 *                  element by element: any alignment, any strides), else NAF_XNA_GENERIC.  An insisted NAF_XNA_MFMA / NAF_XNA_UNION (and
 *                  NAF_XNA_ROWS for q / k_lr) answers -NAF_ERR_UNSUPPORTED; NAF_XNA_GENERIC serves every layout.
 *   naf_xna_bwd    NAF_XNA_MFMA needs q, k_lr, v_lr, dout and dq vectorisable.  NAF_XNA_ROWS needs q and k_lr, and v_lr and dout too
 *                  unless Dv <= 32 (the gather form reads them element by element); it stores dq element by element.  Under AUTO the
 *                  first of NAF_XNA_MFMA, NAF_XNA_ROWS, NAF_XNA_GENERIC that admits the layout runs; an insisted kernel that does not
 *                  answers -NAF_ERR_UNSUPPORTED.
 *   naf_xna_head_fwd / _ce_fwd   q, k_lr, pv_lr (and dlogits) not vectorisable: -NAF_ERR_UNSUPPORTED under AUTO and FUSED alike, the
 *                  caller composes naf_xna_fwd.  out, loss and labels are stored element by element: any alignment of their element
 *                  size, any strides {b, y, x} (out: x stride >= N).
 *   naf_xna_mse_fwd              the rules of NAF_XNA_UNION for q, k_lr, v_lr and out (the gradient); otherwise -NAF_ERR_UNSUPPORTED.
 *   naf_xna_cos_fwd              as naf_xna_head_fwd, with v_lr held to the rule of q, k_lr and pv_lr; out and norms are stored element by
 *                  element: 4-byte aligned, any strides {b, y, x} (out: x stride >= N).
 *   naf_xna_cos_ce_fwd           as naf_xna_cos_fwd; dlogits held to the rule of naf_xna_head_ce_fwd's (16-byte aligned, strides {b, y, x}
 *                  multiples of 8 elements, else -NAF_ERR_UNSUPPORTED; x stride >= dlogits_channels); target, loss, labels and dscale are
 *                  read / stored element by element: aligned to their element size, any strides {b, y, x}.
 *                  A row too short for what is stored in it (out: x stride < N, dlogits: x stride < dlogits_channels) is no layout any
 *                  kernel could serve: -NAF_ERR_INVALID, for these two entries as for the head's. */

/* ---- cross-scale neighbourhood attention forward -------------------------------------------------
 * Replaces legacy_attention (attentions.py:16-29: na2d_qk -> *scale -> softmax -> na2d_av), the fused
 * na2d call (attentions.py:72) and the K/V nearest-exact upsampling feeding them (attentions.py:60-61),
 * evaluated directly on the low-res grid.
 *   q      device bf16 [B, heads, Ho, Wo, Dq]   strides {b, head, y, x}, Dq contiguous
 *   k_lr   device bf16 [B, heads, h, w, Dq]     strides {b, head, y, x}, Dq contiguous
 *   v_lr   device bf16 [B, heads, h, w, Dv]     strides {b, head, y, x}, Dv contiguous
 *   out    device out_dtype [B, heads, Ho, Wo, Dv] strides {b, head, y, x}, Dv contiguous
 *          (a channels-last [B, Ho, Wo, heads*Dv] buffer is {Ho*Wo*C, Dv, Wo*C, C})
 *   logits optional device float [B, heads, Ho, Wo, ky*kx] dense: scaled pre-softmax scores, i.e. what
 *          the reference's return_weights=True hands back (attentions.py:27-28); NULL to skip.  Both paths
 *          produce them (the MFMA kernel writes them from its S^T accumulators).
 *   idx_y  optional device int32 [Ho][ky], idx_x [Wo][kx] from naf_axis_index_table; required by the two
 *          table-driven paths (NAF_XNA_UNION, NAF_XNA_ROWS, NAF_XNA_GENERIC), ignored by the cell kernels (closed
 *          form, integer ratio).  AUTO may pick NAF_XNA_UNION / NAF_XNA_ROWS, so callers that pass tables of their own making must
 *          ask for NAF_XNA_GENERIC.
 *   rope_tab_y / rope_tab_x  optional device float [Ho][2][Dq/4] / [Wo][2][Dq/4] from naf_rope_tables.  When
 *          both are given, `q` holds the UN-rotated guidance and the kernel applies RoPE (rope.py:15-34,139-153,
 *          same arithmetic and bf16 rounding as naf_rope_pool_fwd) to every query as it is loaded, so the
 *          rotated queries never make a round trip through HBM (pair with naf_rope_pool_fwd(q = NULL) for the
 *          keys).  Only the MFMA path with Wo/w a multiple of 16 serves this; naf_xna_select reports
 *          NAF_ERR_UNSUPPORTED otherwise and the caller falls back to materialised queries.  NULL = off.
 * out_dtype NAF_F16 (naf_dtype_supported): v_lr holds IEEE half and `out` receives half -- the struct has no value dtype of its own,
 *          half values with any other out_dtype cannot be expressed and hosts must reject them.  Every path serves it, and
 *          naf_xna_select picks the kernel it picks for NAF_BF16 output of the same geometry.  q, k_lr, logits: as above.
 * scale <= 0 selects the reference default Dq^-0.5 (attentions.py:46). */
typedef struct naf_xna_args {
    const void* q;
    const void* k_lr;
    const void* v_lr;
    void* out;
    float* logits;
    const int32_t* idx_y;
    const int32_t* idx_x;
    const float* rope_tab_y;
    const float* rope_tab_x;
    int32_t B, heads, Ho, Wo, h, w, Dq, Dv, ky, kx;
    int32_t out_dtype; /* naf_dtype */
    int32_t path;      /* naf_xna_path */
    float scale;
    int32_t reserved;
    int64_t q_stride[4];
    int64_t k_stride[4];
    int64_t v_stride[4];
    int64_t o_stride[4];
} naf_xna_args;

/* Which kernel naf_xna_fwd would run for these arguments (NAF_XNA_MFMA, NAF_XNA_UNION, NAF_XNA_ROWS or NAF_XNA_GENERIC), or a
 * negative naf_status on invalid arguments.  Lets the caller skip building index tables (MFMA needs none). */
int naf_xna_select(const naf_xna_args* a);
/* Diagnostics: the workgroup plan of the NAF_XNA_UNION path for these arguments, out = {slots per window row
 * (16/32), output rows per workgroup, output pixels per workgroup, staged low-res rows, staged low-res columns,
 * value channels per pass, LDS bytes}.  Returns 1 when that path can serve the request, 0 otherwise. */
int naf_xna_union_plan(const naf_xna_args* a, int32_t out[7]);
/* Scratch bytes the call needs (currently always 0; kept so callers need not change later). */
size_t naf_workspace_bytes(const naf_xna_args* a);
int naf_xna_fwd(const naf_xna_args* a, naf_stream_t stream);

/* ---- attention with a linear head folded in (added after 0.4.3; detect by symbol) -----------------------
 * What the reference's users put on the upsampled features is a 1x1 convolution (evaluation/eval_seg_probing.py:56,104-111:
 * nn.Conv2d(embed_dim, num_classes, 1) on model(image, feats, (H, W))).  The attention is linear in the values and its weights sum to
 * one, so with W [N, C], b [N] and attention head g owning channels [g*Dv, (g+1)*Dv):
 *     head(naf(V))[n, px] = b[n] + sum_g sum_slot P_g[px, slot] * PV_g[n, cell(slot)],      PV_g = W[:, g*Dv:(g+1)*Dv] @ V_g
 * PV lives on the low-res grid; this entry runs the attention of every head on it and SUMS the heads into one N-channel output, so the
 * [B, C, Ho, Wo] tensor is never written.
 *   q, k_lr   as in naf_xna_args (bf16, strides {b, head, y, x}, last dim contiguous, Dq = 64)
 *   pv_lr     device bf16 [B, heads, h, w, Npad], Npad = N rounded up to a multiple of 16, strides {b, head, y, x}, last dim contiguous;
 *             channels N .. Npad-1 are read and must be finite (the caller zeroes them); they are never stored
 *   bias      device float [N] added in fp32, or NULL
 *   out       device [B, Ho, Wo, N] of out_dtype (NAF_BF16 / NAF_F32), element strides {b, y, x}, channel axis contiguous
 *   rope_tab_y / rope_tab_x   rotate-on-load exactly as in naf_xna_args (q is then the un-rotated channels-last guidance)
 * Kernel (xna_head_kernel.h): one workgroup per (batch, low-res cell) loops over the heads; each head's softmax is normalised in fp32
 * BEFORE its weights are rounded to bf16 (what naf_xna_fwd's cell kernel does per head), and the heads add up in fp32 accumulators.
 * Served: square odd window 3 .. 15, Dq = 64, integer ratio whose cell rows are row tiles (Wo/w a multiple of 16, or 14, 15, 28, 30 ...),
 * h, w >= window, any head count, 1 <= N <= 256, 16-byte aligned q / k_lr / pv_lr with strides that are multiples of 8 elements.
 * naf_xna_head_select: NAF_XNA_HEAD_FUSED when naf_xna_head_fwd serves the arguments, else a negative naf_status (with naf_last_error):
 * -NAF_ERR_INVALID for arguments no kernel could serve (NULL, N outside 1 .. 256, even window ...), -NAF_ERR_UNSUPPORTED for a valid
 * request outside the list above -- the caller then composes naf_xna_fwd on pv_lr (fp32 output) with a sum over the heads.  A pure
 * host-side query: pointers are checked, never read.  path: NAF_XNA_HEAD_AUTO or NAF_XNA_HEAD_FUSED (the same answer today; AUTO is where a
 * measured "the composition is faster here" would go).  scale <= 0 selects Dq^-0.5.  Caller-owned memory and stream; capturable. */
enum naf_xna_head_path {
    NAF_XNA_HEAD_AUTO = 0,
    NAF_XNA_HEAD_FUSED = 1
};
typedef struct naf_xna_head_args {
    const void* q;
    const void* k_lr;
    const void* pv_lr;
    const float* bias;
    void* out;
    const float* rope_tab_y;
    const float* rope_tab_x;
    int32_t B, heads, Ho, Wo, h, w, Dq, N, ky, kx;
    int32_t out_dtype; /* naf_dtype */
    int32_t path;      /* naf_xna_head_path */
    float scale;
    int32_t reserved;
    int64_t q_stride[4];
    int64_t k_stride[4];
    int64_t pv_stride[4];
    int64_t o_stride[3];
} naf_xna_head_args;
int naf_xna_head_select(const naf_xna_head_args* a);
/* Scratch bytes the call needs (0 today; kept so callers need not change later). */
size_t naf_xna_head_workspace_bytes(const naf_xna_head_args* a);
int naf_xna_head_fwd(const naf_xna_head_args* a, naf_stream_t stream);

/* ---- ... with a classification objective in the epilogue (added after the head entries; detect by symbol) ------------
 * What the reference does with the probe's logits (evaluation/eval_seg_probing.py:94-135 and its train / validate loops): a
 * cross-entropy over the pixels whose target is not IGNORE = 255, or an argmax for accuracy / IoU.  The logits of a pixel are in the
 * registers of four lanes when naf_xna_head_fwd's kernel is done, so this entry computes, per pixel and in fp32, over the N channels,
 *     lse = max z + ln sum exp(z - max z),  label = argmax z,  loss = lse - z[t],  dlogits[n] = exp(z[n] - lse) - (n == t)
 * and stores only what is asked for; the [B, Ho, Wo, N] logits need not exist.
 *   head      naf_xna_head_args as for naf_xna_head_fwd, except that `out` may be NULL; when given it receives the logits, fp32
 *             (out_dtype must be NAF_F32), bit for bit what naf_xna_head_fwd stores
 *   target    device int64 [B, Ho, Wo], element strides t_stride {b, y, x}; NULL when only labels / logits are wanted.  A pixel is
 *             IGNORED when target == ignore_index or target is outside [0, N)
 *   loss      device float [B, Ho, Wo] (loss_stride), or NULL: lse - z[t], 0 for an ignored pixel.  Needs target.  The caller reduces
 *             the map (sum, or sum / number of valid pixels): no floating-point atomics anywhere in this entry or the next, so every
 *             output is deterministic, bit for bit
 *   labels    device uint8 [B, Ho, Wo] (labels_stride), or NULL: the lowest index among equal maxima (torch.argmax's documented choice)
 *   dlogits   device bf16 [B, Ho, Wo, dlogits_channels] (dlogits_stride {b, y, x}, channel axis contiguous), or NULL: softmax - onehot of a
 *             valid pixel, zeros for an ignored one, rounded once to bf16 and NOT divided by the number of valid pixels (the caller scales
 *             the low-res result of naf_xna_bwd, which is linear in it).  The kernel writes EVERY one of the dlogits_channels channels
 *             (zeros from N up), so the buffer needs no clearing: it is the `dout` of naf_xna_bwd for all heads at once (head stride 0),
 *             dlogits_channels being a value width that entry serves.  Needs target.
 * naf_xna_head_ce_select answers as naf_xna_head_select does (NAF_XNA_HEAD_FUSED, -NAF_ERR_INVALID, -NAF_ERR_UNSUPPORTED, with
 * naf_last_error) and additionally refuses: no output requested; loss / dlogits without target; dlogits_channels not a multiple of 8,
 * smaller than N rounded up to 16, or above 256 (all -NAF_ERR_INVALID); a dlogits that is not 16-byte aligned or whose strides are not
 * multiples of 8 elements (-NAF_ERR_UNSUPPORTED).  Served geometries: exactly naf_xna_head_fwd's.
 * NOT what torch.nn.functional.cross_entropy does: (1) a target outside [0, N) that is not ignore_index is ignored (loss 0, zero
 * gradient, not to be counted by the caller) where torch raises a device-side assert -- the target is only ever compared with channel
 * indices, never used to form an address; (2) no reduction: the mean over zero valid pixels (torch: nan) is the caller's division;
 * (3) no class weights, label smoothing or soft targets.  Caller-owned memory and stream; capturable; no workspace. */
typedef struct naf_xna_head_ce_args {
    naf_xna_head_args head; /* head.out may be NULL */
    const int64_t* target;
    float* loss;
    uint8_t* labels;
    void* dlogits;
    int64_t ignore_index;
    int32_t dlogits_channels;
    int32_t reserved;
    int64_t t_stride[3];
    int64_t loss_stride[3];
    int64_t labels_stride[3];
    int64_t dlogits_stride[3];
} naf_xna_head_ce_args;
int naf_xna_head_ce_select(const naf_xna_head_ce_args* a);
int naf_xna_head_ce_fwd(const naf_xna_head_ce_args* a, naf_stream_t stream);

/* ---- ... and a confusion matrix counted in that epilogue (added after the classification entries; detect by symbol) ------------
 * What the reference's evaluate() reports (evaluation/eval_seg_probing.py:221-257: accuracy and Jaccard index of the masked predictions)
 * is a function of one N x N confusion matrix summed over the validation set.  label and target of a pixel are in registers when the
 * classification epilogue is done, so this entry adds, for every pixel that is not IGNORED (as defined for naf_xna_head_ce_args),
 *     confusion[target * cm_stride + label] += 1                 (row = target, column = prediction)
 *   ce         naf_xna_head_ce_args as for naf_xna_head_ce_fwd; every output of that entry stays available in the same launch, bit for bit
 *              what naf_xna_head_ce_fwd stores for the same arguments, and all of them may be NULL here (the matrix is an output).
 *              ce.target is required
 *   confusion  device int64, N rows of cm_stride elements (cm_stride >= N), 8-byte aligned, caller-owned.  The call ACCUMULATES: the
 *              library never clears it, so one matrix passed for every batch of a validation set ends up as the set's matrix without a
 *              label map written or a host synchronisation; over several devices, each accumulates its own and the caller sums them
 *              once.  Elements [row][N .. cm_stride) are not touched
 * The counts are aggregated within a wave before they are added with integer atomics (vector memory, no return value).  Integer adds
 * commute exactly, so the matrix -- like every other output -- is deterministic, bit for bit, whatever the order the workgroups run in.
 * t * cm_stride + label is the one address this library ever forms from a target value, after t and label have been checked to lie in
 * [0, N); a pixel whose logits are NaN (no maximum) is not counted.
 * naf_xna_head_cm_select answers as naf_xna_head_ce_select does and additionally refuses (-NAF_ERR_INVALID): a NULL or not 8-byte
 * aligned confusion, a NULL ce.target, cm_stride < N, non-zero reserved fields.  Served geometries: exactly naf_xna_head_ce_fwd's (at
 * most 256 classes; beyond, the caller counts the labels of the composed path).  Caller-owned memory and stream; capturable; no workspace. */
typedef struct naf_xna_head_cm_args {
    naf_xna_head_ce_args ce; /* ce.target required; every output of ce may be NULL */
    int64_t* confusion;
    int64_t cm_stride;
    int64_t reserved[2]; /* must be 0 */
} naf_xna_head_cm_args;
int naf_xna_head_cm_select(const naf_xna_head_cm_args* a);
int naf_xna_head_cm_fwd(const naf_xna_head_cm_args* a, naf_stream_t stream);

/* ---- ... or a dense regression objective in the epilogue (added after the k-means entries; detect by symbol) ------------
 * The other dense probing protocol the upsampler literature reports with the same linear probe: a 1x1 Conv2d(C, N) trained on a dense
 * target (N = 1 depth; N = 2, 3 flow, normals, colour) under a validity mask and, for depth, scored with RMSE, abs-rel and delta < 1.25^k.
 * A pixel's N logits z are in the registers of four lanes when naf_xna_head_fwd's kernel is done, so this entry computes, per pixel and
 * in fp32, with r[n] = z[n] - target[n] (the bias added exactly as naf_xna_head_fwd adds it),
 *     loss[px]       = sum_n l(r[n]), 0 where the pixel is not valid
 *     dlogits[px, n] = l'(r[n]),      0 where the pixel is not valid and for the pad channels n >= N
 *     NAF_HEAD_REG_L1         l = |r|                                                   l' = sign(r)   (0 at r = 0)
 *     NAF_HEAD_REG_MSE        l = r * r                                                 l' = 2 r, formed as (bf16)(2.f * r)
 *     NAF_HEAD_REG_SMOOTH_L1  l = |r| < beta ? 0.5 r r / beta : |r| - 0.5 beta          l' = |r| < beta ? r / beta : sign(r)     (torch's, beta > 0)
 * and stores only what is asked for; the [B, Ho, Wo, N] logits need not exist.
 *   head      naf_xna_head_args as for naf_xna_head_fwd, except that `out` may be NULL; when given it receives the logits, fp32
 *             (out_dtype must be NAF_F32), bit for bit what naf_xna_head_fwd stores.  1 <= N <= 32 here
 *   target    device float [B, N, Ho, Wo] read at ELEMENT strides t_stride {b, n, y, x}: any layout (NCHW, channels-last, a view).  NULL when
 *             only the logits are wanted.  Target and mask are only read as values; no address is formed from them
 *   valid     device uint8 [B, Ho, Wo] (valid_stride {b, y, x}), or NULL = every pixel valid: a pixel is valid when its byte is not 0, for
 *             all N channels alike
 *   loss      device float [B, Ho, Wo] (loss_stride), or NULL.  A lane adds its channels in ascending order, the pixel's four lanes add in a
 *             two-level tree: N - 1 additions.  The caller reduces the map (sum, or sum / (valid pixels * N))
 *   dlogits   device bf16 [B, Ho, Wo, dlogits_channels] (dlogits_stride {b, y, x}, channel axis contiguous), or NULL: rounded once to bf16,
 *             NOT divided by anything; EVERY one of the dlogits_channels channels is written, so the buffer needs no clearing: it is the
 *             `dout` of naf_xna_bwd for all heads at once (head stride 0), as naf_xna_head_ce_args' is
 *   errors    device double[NAF_HEAD_REG_STATS], 8-byte aligned, or NULL; N == 1 only.  The call ADDS to it (the library never clears it), so
 *             one accumulator passed for every batch of a validation set ends up as the set's sums without a host synchronisation.  With
 *             p = min(max(z, clamp_lo), clamp_hi) (clamp_lo > 0; both bounds are the floats given) a pixel is COUNTED when it is valid,
 *             target > 0 and target and z are finite; over the counted pixels, with d = ln p - ln target:
 *               [0] n   [1] sum |p - t|   [2] sum (p - t)^2   [3] sum |p - t| / t   [4] sum (p - t)^2 / t   [5] sum d   [6] sum d^2
 *               [7], [8], [9] number of pixels with max(p / t, t / p) < 1.25, 1.25^2, 1.25^3
 *             The clamp applies to these statistics only.
 *   workspace device, naf_xna_head_reg_workspace_bytes(a) bytes (0 without errors), 8-byte aligned; contents need no initialisation
 * Summation of the statistics: no floating-point atomics.  Per round of its workgroup (xna_head_kernel.h) a lane adds at most two pixels'
 * terms in fp32, the 16 lanes of a row add theirs in a four-level tree, and from there on every addition is fp64: the wave's sums over
 * the rounds, the eight waves in wave order, one row of ten fp64 partials per workgroup in `workspace`, and a one-workgroup finishing
 * kernel launched by the same call on the same stream that adds the rows in a fixed order and adds the ten totals to `errors`.  The
 * LONGEST FP32 ADDITION CHAIN between a pixel's term and the fp64 sums is 6 (this interface promises at most 64); counts are exact.
 * Two runs give the same bits.  No cross-workgroup dependency, no spin-wait.
 * naf_xna_head_reg_select answers as naf_xna_head_ce_select does (NAF_XNA_HEAD_FUSED, -NAF_ERR_INVALID, -NAF_ERR_UNSUPPORTED, with
 * naf_last_error) and additionally refuses, -NAF_ERR_INVALID: nothing asked for (out, loss, dlogits and errors all NULL); a NULL target with
 * loss, dlogits or errors; errors with N != 1; errors that is not 8-byte aligned; beta <= 0 with NAF_HEAD_REG_SMOOTH_L1; clamp_lo <= 0 or
 * clamp_hi < clamp_lo with errors; an unknown kind; non-zero reserved fields; dlogits_channels as for naf_xna_head_ce_args;
 * -NAF_ERR_UNSUPPORTED: N > 32 (the caller composes naf_xna_head_fwd's fp32 logits with the loss); a dlogits that is not 16-byte
 * aligned, whose strides are not multiples of 8 elements, or whose channel count is not a value width naf_xna_bwd serves (32, 64, 96,
 * 128, 192, 256).  A pure host-side query: pointers are checked, never read.  naf_xna_head_reg_fwd additionally refuses
 * (-NAF_ERR_INVALID) a NULL, misaligned or too small workspace when errors is given.  Served geometries: exactly naf_xna_head_fwd's.
 * The struct must be zero-initialised by the caller (reserved fields are checked).  Caller-owned memory, workspace and stream; nothing
 * is allocated or kept; capturable. */
#define NAF_HEAD_REG_STATS 10
enum naf_head_reg_kind { NAF_HEAD_REG_L1 = 0, NAF_HEAD_REG_MSE = 1, NAF_HEAD_REG_SMOOTH_L1 = 2 };
typedef struct naf_xna_head_reg_args {
    naf_xna_head_args head; /* head.out may be NULL */
    const float* target;
    const uint8_t* valid;
    float* loss;
    void* dlogits;
    double* errors;
    void* workspace;
    size_t workspace_bytes;
    int32_t dlogits_channels;
    int32_t kind; /* naf_head_reg_kind */
    float beta;
    float clamp_lo, clamp_hi;
    int32_t reserved[3]; /* must be 0 */
    int64_t t_stride[4]; /* {b, n, y, x} */
    int64_t valid_stride[3];
    int64_t loss_stride[3];
    int64_t dlogits_stride[3];
} naf_xna_head_reg_args;
int naf_xna_head_reg_select(const naf_xna_head_reg_args* a);
size_t naf_xna_head_reg_workspace_bytes(const naf_xna_head_reg_args* a);
int naf_xna_head_reg_fwd(const naf_xna_head_reg_args* a, naf_stream_t stream);

/* ---- label propagation: windowed top-k affinity over a queue of context frames (added after the confusion entries; detect by symbol) ----
 * Replaces label_propagation (evaluation/eval_video_seg.py:499-561) after feature extraction: the reference materialises
 * exp(bmm(feat_tar, feat_sources) / T) as a dense [n * h*w, h*w] matrix, multiplies it by restrict_neighborhood's mask, takes topk along the
 * source axis, thresholds, normalises and multiplies by the label maps.  Here the affinities are never written.  For a target pixel p = (i, j):
 *   candidates  every (frame f, pixel (i', j')) with |i - i'| <= radius and |j - j'| <= radius inside the image (window clipped, not shifted)
 *   score       s = cos(target[p], context[f][i', j']): the raw bf16 dot product on the matrix cores (fp32 accumulation) times the two
 *               per-pixel inverse norms of naf_feature_inv_norm; on bf16 inputs within (C + 8) * 2^-24 of exact arithmetic
 *   threshold   the topk-th largest score among the candidates; with fewer than topk candidates all of them are kept
 *   kept        every candidate with s >= threshold: TIES AT THE THRESHOLD ARE ALL KEPT (as `aff[aff < tk_val_min] = 0` keeps them)
 *   out[:, p]   sum_kept w * segs[f, i', j', :] / sum_kept w,  w = exp((s - s_max) / temperature), s_max the pixel's largest score
 * Features are consumed as bf16: a caller holding fp32 features rounds them to bf16 ONCE (no normalise-then-round).
 *   target, context[f]          bf16, dense channels-last [h, w, C], 16-byte aligned: context frames are separate pointers passed by value,
 *                               so a caller's frame queue is never stacked or copied
 *   target_inv, context_inv[f]  fp32 [h, w]: 1 / max(||x||_2, 1e-12) per pixel (naf_feature_inv_norm; F.normalize's eps)
 *   segs                        fp32, dense channels-last [n, h, w, K]: the context frames' soft label maps
 *   out                         fp32, dense [K, h, w]
 * Served: C % 32 == 0 and 32 <= C <= 1024, 1 <= K <= 64, 1 <= topk <= 16, 1 <= radius <= 15, 1 <= n <= 16, any h, w >= 1 (h * w * max(C, K)
 * below 2^31 elements per frame); anything else that is well formed is NAF_ERR_UNSUPPORTED with the limit named in naf_last_error().
 * radius = 0 is the reference's "no mask", the dense case: not served.  No atomics: the output is bit-reproducible from run to run.
 * Every point of that range launches: the key rows stream through LDS double-buffered where two halo rows fit in 160 KiB beside the
 * (K + 1) * 512 bytes of sums, single-buffered where they do not (which therefore depends on C, radius AND K: C = 768, radius = 15 is
 * double-buffered at K <= 27 and single-buffered above; C = 1024 is single-buffered from radius = 1 at K = 64), and the largest request
 * (C = 1024, radius = 15, K = 64) takes 132 544 bytes.  naf_propagate_plan names the choice.
 * naf_propagate_select is a host-only query (it reads the scalar fields only and touches no device): NAF_OK, NAF_ERR_UNSUPPORTED or
 * NAF_ERR_INVALID (NULL args, non-positive sizes, negative radius, temperature not > 0, non-zero reserved).  naf_propagate_fwd additionally
 * refuses NULL or misaligned pointers.  Caller-owned memory and stream; capturable; no workspace. */
#define NAF_PROPAGATE_MAX_FRAMES 16
typedef struct naf_propagate_args {
    const void* target;
    const float* target_inv;
    const void* context[NAF_PROPAGATE_MAX_FRAMES];      /* entries [n .. 16) are ignored */
    const float* context_inv[NAF_PROPAGATE_MAX_FRAMES];
    const float* segs;
    float* out;
    int32_t n, C, h, w, K, radius, topk;
    float temperature;
    int32_t reserved[2]; /* must be 0 */
} naf_propagate_args;
int naf_propagate_select(const naf_propagate_args* a);
int naf_propagate_fwd(const naf_propagate_args* a, naf_stream_t stream);
/* What naf_propagate_fwd would launch for these scalar fields (added after naf_xna_points; detect by symbol).  Host-only like
 * naf_propagate_select, whose status it returns (NAF_ERR_INVALID also for a NULL `out`); on NAF_OK out = {KSMAX, nkb, nbuf, LDS bytes}:
 * the kernel instantiation's query fragments (4, 8, 12, 16, 24 or 32: the smallest that holds C / 32), the 16-key blocks per halo row
 * (ceil((16 + 2 radius) / 16)), 2 where two halo rows fit in 160 KiB of LDS beside the sums (double-buffered) and 1 where they do not, and
 * the dynamic LDS of the launch.  The launch takes its choices from the same function. */
int naf_propagate_plan(const naf_propagate_args* a, int32_t out[4]);
/* inv[p] = 1 / max(sqrt(sum_c x[p][c]^2), 1e-12) from an fp32 sum of squares.  x: bf16 dense channels-last [h, w, C], 16-byte aligned,
 * C % 8 == 0; inv: fp32 [h, w].  NAF_ERR_INVALID on NULL / misaligned pointers or non-positive sizes. */
int naf_feature_inv_norm(const void* x, float* inv, int32_t h, int32_t w, int32_t C, naf_stream_t stream);

/* ---- denoising objective: L1 / L2 / SSIM loss with its gradient, PSNR / SSIM metrics (added after the propagation entries; detect by symbol) ----
 * Replaces DenoisingLoss (denoising.py:129-177) with the backward autograd runs through it, and MetricsCalculator (denoising.py:61-126) with
 * the clamp in front of it (denoising.py:302): one tile kernel plus a one-workgroup finishing kernel instead of a chain of pools, grouped
 * convolutions and elementwise passes.  pred and target are [B, C, H, W] given by four ELEMENT strides {b, c, y, x} each (any layout: pred is
 * usually the logical-NCHW view of a channels-last buffer), fp32 or bf16 independently; any C, H, W >= 1, images smaller than the window
 * included.  Every (b, c) plane is independent.  All arithmetic is fp32 on the values as given (bf16 is widened, never re-rounded).
 *
 * mode NAF_DENOISE_LOSS, per plane, with box(x) = zero-padded 3 x 3 sum / 9 (F.avg_pool2d(x, 3, 1, 1): the divisor is always 9):
 *     mu1 = box(p), mu2 = box(t), s1 = box(p^2) - mu1^2, s2 = box(t^2) - mu2^2, s12 = box(p t) - mu1 mu2        C1 = 1e-4, C2 = 9e-4
 *     n1 = 2 mu1 mu2 + C1, n2 = 2 s12 + C2, d1 = mu1^2 + mu2^2 + C1, d2 = s1 + s2 + C2, S = n1 n2 / (d1 d2)
 *   The (co)variances are evaluated in their centred form, box((p - mu1)(t - mu2)) over the same nine samples (padding zeros included),
 *   which is the same number without the cancellation of box(p t) - mu1 mu2.
 *   out[0] = mean |p - t|, out[1] = mean (p - t)^2, out[2] = mean S            (N = B C H W)
 *   out[3] = l1_weight * out[0], out[4] = l2_weight * out[1], out[5] = ssim_weight * (1 - out[2]), out[6] = out[3] + out[4] + out[5]:
 *   the reference's dict entries, formed in fp64 from the fp64 sums and rounded once; out[7] = 0
 *   grad (optional): d out[6] / d pred, ONE map, written in the same launch:
 *     a = 2 mu2 (n2 - n1) / (d1 d2) - 2 mu1 S (1/d1 - 1/d2),  b = -S / d2,  c = 2 n1 / (d1 d2)
 *     g = [ l1_weight sign(p - t) + 2 l2_weight (p - t) - ssim_weight ( box(a) + 2 p box(b) + t box(c) ) ] / N,      sign(0) = 0
 *   in grad_dtype (bf16: rounded once, to nearest even) at grad_stride.
 * mode NAF_DENOISE_METRICS (forward only; grad must be NULL, the weights are ignored): pred is clamped to [0, 1] on load when clamp != 0; the
 *   windowed means go through the 11 x 11 window w[i][j] = g[i] g[j], g the fp32 vector exp(-(i - 5)^2 / (2 (11/6)^2)) normalised in fp32,
 *   with zero padding, evaluated separably; S as above.
 *   out[0] = PSNR = -10 log10(mse) in dB (+inf for mse = 0), out[1] = mean S, out[2] = mse = mean (p - t)^2, out[3..7] = 0
 * Summation: no floating-point atomics.  A workgroup owns one 32 x 32 tile of one plane; a thread adds at most five terms, the workgroup's
 * 256 threads add theirs in a binary tree (at most 13 fp32 additions between a pixel's term and the workgroup's partial), the partial goes to
 * `workspace`, and the finishing kernel adds all partials in fp64 in a fixed order: two runs give the same bits.
 *   out        device float[8]
 *   workspace  device, naf_denoise_workspace_bytes(a) bytes, 16-byte aligned; contents need no initialisation
 * Argument checks happen before any HIP call: NAF_ERR_INVALID for NULL args / pred / target / out / workspace, B, C, H or W <= 0, an unknown
 * dtype or mode, a negative (or NaN) weight, a workspace that is too small, grad in metrics mode, non-zero reserved; NAF_ERR_UNSUPPORTED for
 * 2^24 tiles of 32 x 32 or more.  naf_denoise_workspace_bytes reads B, C, H, W only and returns 0 for arguments that are not valid.
 * Caller-owned memory, workspace and stream; nothing is allocated or kept; capturable. */
enum naf_denoise_mode { NAF_DENOISE_LOSS = 0, NAF_DENOISE_METRICS = 1 };
typedef struct naf_denoise_args {
    const void* pred;
    const void* target;
    void* grad;             /* optional, loss mode: [B, C, H, W] at grad_stride */
    float* out;             /* float[8] */
    void* workspace;
    size_t workspace_bytes;
    int32_t pred_dtype, target_dtype, grad_dtype; /* naf_dtype */
    int32_t mode;                                 /* naf_denoise_mode */
    int32_t B, C, H, W;
    int32_t clamp;    /* metrics mode: clamp pred to [0, 1] on load */
    int32_t reserved; /* must be 0 */
    double l1_weight, l2_weight, ssim_weight;
    int64_t pred_stride[4], target_stride[4], grad_stride[4]; /* {b, c, y, x} */
} naf_denoise_args;
size_t naf_denoise_workspace_bytes(const naf_denoise_args* a);
int naf_denoise_objective(const naf_denoise_args* a, naf_stream_t stream);

/* ---- feature PCA for display: second moments, projection, min-max (added after the denoising entries; detect by symbol) ----
 * The device side of the reference's pca() (utils/visualization.py:135-190: every map copied to the host, torch.pca_lowrank(niter=20) on the
 * CPU, a projection on three components, a min-max per component).  Here the fit needs the Gram matrix and the channel sums of each map
 * (naf_feature_moments; the C x C eigen-decomposition is the caller's), a map's picture is its projection (naf_pca_project) scaled by the
 * minima and maxima the same call returns.  A projection that came out of the head kernel (naf_xna_head_fwd with weight = V^T and
 * bias = -mean V) gets its minima and maxima from naf_pca_minmax.
 *
 * A map is P rows ("pixels") of C contiguous bf16 values -- dense channels-last memory, what naf_forward writes -- at a constant row stride
 * `ld` in elements, ld >= C and ld % 8 == 0, base pointer 16-byte aligned.  Served: C % 32 == 0 and 32 <= C <= NAF_PCA_MAX_C, any
 * 1 <= P < 2^31, 1 <= n <= NAF_PCA_MAX_COMPONENTS.  Inputs are assumed finite.
 *
 * naf_feature_moments:   gram[i][j] = sum_p x[p][i] x[p][j]  (fp64 [C][C], the FULL matrix: gram[i][j] and gram[j][i] are the same bits)
 *                        sum[i]     = sum_p x[p][i]          (fp64 [C])
 * Summation contract.  The pixels are cut into `nsplit` slabs of `slab_pixels` consecutive pixels (the last one may be shorter;
 * naf_feature_moments_plan names both numbers, from P and C alone).  A product x[p][i] x[p][j] of two bf16 values is exact in fp32.  Within a
 * slab the products of one entry are added in fp32 on the matrix cores (v_mfma_f32_16x16x32_bf16 chains, pixels in order); the channel sums are
 * products with 1.0 on the same path.  The slabs' fp32 partials go to `workspace`, and a finishing kernel adds them in fp64 in slab order.  So
 * at most L = min(P, NAF_MOMENTS_CHAIN) fp32 additions lie between a product and the fp64 sum (slab_pixels <= NAF_MOMENTS_CHAIN always), the
 * fp64 stage adds at most nsplit terms, and |gram[i][j] - exact| <= L 2^-24 sum_p |x[p][i] x[p][j]| to first order (likewise for sum).
 * No floating-point atomics: two runs give the same bits.  An entry and its mirror image are written from one register.
 * Slab count: the library aims at 512 workgroups (one per 128 x 128 block of the upper triangle and slab) with slabs of at least 256 pixels,
 * keeps the workspace at or below NAF_MOMENTS_WORKSPACE_CAP bytes, and -- taking precedence over that cap -- never lets a slab exceed
 * NAF_MOMENTS_CHAIN pixels.  (At C = 4096 a slab's partials are 34.6 MB, so the cap holds up to P = 7 * 65536 there; at C <= 2048 up to 2^21 pixels.)
 *   workspace  device, naf_feature_moments_workspace_bytes(a) bytes, 16-byte aligned; contents need no initialisation
 *
 * naf_pca_project:       y[p][r] = b[r] + sum_c x[p][c] V[c][r],  r < n         V fp32 [C][n] dense, b fp32 [n], y fp32 [P][n] dense
 *                        minmax[0][r] = min_p y[p][r], minmax[1][r] = max_p y[p][r]            fp32 [2][n]
 * fp32 fused multiply-adds in a fixed order: lane k of the 16 lanes that share a pixel takes the 8-channel chunks k, k + 16, ... in ascending
 * channel order, the 16 lane sums are added in a four-step butterfly, the bias comes last: at most C / 16 + 5 roundings per element.
 * The minima and maxima are exact (of the y written).  Two launches: the projection with per-workgroup minima and maxima, a one-workgroup finish.
 *   workspace  device, naf_pca_project_workspace_bytes(a) bytes (it reads P only; at most 64 KiB), 16-byte aligned; no initialisation needed
 * naf_pca_minmax:        the same minima and maxima of an existing fp32 buffer y[p * ld + r], r < n, ld >= n in elements (so a [.., Npad] logits
 *                        buffer of the head kernel is read in place).  workspace: as naf_pca_project_workspace_bytes says for the same P.
 * Normalisation, (y - min) / (max - min) per component as visualization.py:166-167 does, is left to the caller (two elementwise operations); a
 * constant component divides by zero there as it does in the reference.
 * Argument checks happen before any HIP call: NAF_ERR_INVALID for NULL args or pointers, misaligned pointers, P, C or n <= 0, ld < C (ld < n) or
 * ld % 8 != 0, a workspace that is too small, non-zero reserved; NAF_ERR_UNSUPPORTED, with the limit named in naf_last_error(), for C or n
 * outside the served range.  The _workspace_bytes queries return 0 for arguments that are not valid.  naf_feature_moments_plan is host-only
 * (it reads P, C, ld and reserved). Caller-owned memory, workspace and stream; nothing is allocated or kept; capturable. */
#define NAF_MOMENTS_CHAIN 65536                        /* L: most fp32 additions between a product and the fp64 sum */
#define NAF_MOMENTS_WORKSPACE_CAP ((size_t)256 << 20) /* bytes */
#define NAF_PCA_MAX_C 4096
#define NAF_PCA_MAX_COMPONENTS 8
typedef struct naf_feature_moments_args {
    const void* x; /* bf16 [P][ld] */
    double* gram;  /* [C][C] */
    double* sum;   /* [C] */
    void* workspace;
    size_t workspace_bytes;
    int64_t P, ld;
    int32_t C;
    int32_t reserved; /* must be 0 */
} naf_feature_moments_args;
size_t naf_feature_moments_workspace_bytes(const naf_feature_moments_args* a);
int naf_feature_moments_plan(const naf_feature_moments_args* a, int32_t* nsplit, int32_t* slab_pixels);
int naf_feature_moments(const naf_feature_moments_args* a, naf_stream_t stream);
typedef struct naf_pca_project_args {
    const void* x;  /* bf16 [P][ld] */
    const float* V; /* [C][n] */
    const float* b; /* [n] */
    float* y;       /* [P][n] */
    float* minmax;  /* [2][n] */
    void* workspace;
    size_t workspace_bytes;
    int64_t P, ld;
    int32_t C, n;
    int32_t reserved[2]; /* must be 0 */
} naf_pca_project_args;
size_t naf_pca_project_workspace_bytes(const naf_pca_project_args* a);
int naf_pca_project(const naf_pca_project_args* a, naf_stream_t stream);
typedef struct naf_pca_minmax_args {
    const float* y; /* y[p * ld + r] */
    float* minmax;  /* [2][n] */
    void* workspace;
    size_t workspace_bytes;
    int64_t P, ld;
    int32_t n;
    int32_t reserved; /* must be 0 */
} naf_pca_minmax_args;
int naf_pca_minmax(const naf_pca_minmax_args* a, naf_stream_t stream);

/* ---- cross-scale neighbourhood attention backward --------------------------------------------------
 * Replaces what autograd runs through legacy_attention (attentions.py:16-29: the backward of na2d_qk, the
 * scale, the softmax and na2d_av) and through the K/V nearest-exact upsampling (attentions.py:60-61) in the
 * reference's training step (train.py:127-137, test/backward_speed.py:22-69), on the low-res grid.
 *   q, k_lr, v_lr   as in naf_xna_args (bf16, strides {b, head, y, x}, last dim contiguous)
 *   dout   device bf16 [B, heads, Ho, Wo, Dv]   gradient of the output, strides {b, head, y, x}
 *   dq     device bf16 [B, heads, Ho, Wo, Dq]   gradient of q, strides {b, head, y, x}
 *   dk_lr  device float [B, h, w, heads, Dq] dense, dv_lr device float [B, h, w, heads, Dv] dense: the caller
 *          ZEROES them on the same stream before the call; the kernel adds every cell's window sums (fp32 atomics).
 *   idx_y, idx_x   optional device int32 tables from naf_axis_index_table, required by the table-driven path.
 * Kernels, like the forward: the MFMA cell kernels (what the MFMA forward serves with ky = kx <= 15, Wo/w a
 * multiple of 16 -- since 0.4.2, for windows up to 9 x 9, also the widths the forward's row tiles take with a partial last tile: 14
 * (patch-14 backbones), 15, 28, 30 ... -- and Dv in {32, 64, 96, 128, 192, 256}: windows up to 9 x 9 at every Dv and 11 x 11 up to Dv = 128 on
 * the wave-specialised eight-wave kernel, wider heads at 11 x 11 and every head at 13 x 13 / 15 x 15 on the same kernel in
 * CHANNEL CHUNKS of at most 128 / 64 / 64 value channels per launch -- the softmax does not depend on V, dV splits by channel and dQ / dK are
 * sums over channels, so each launch is a complete backward for its slice and later launches add their dQ to the earlier ones'), the
 * row-streaming matrix-core kernel below, and a table-driven one for everything else (any ratio,
 * head dims, rectangular windows; one wave per query, atomics per key).  naf_xna_bwd_supported returns which
 * (NAF_XNA_MFMA / NAF_XNA_ROWS / NAF_XNA_GENERIC) so that the caller knows whether to build the tables.  scale <= 0 selects Dq^-0.5. */
typedef struct naf_xna_bwd_args {
    const void* q;
    const void* k_lr;
    const void* v_lr;
    const void* dout;
    void* dq;
    float* dk_lr;
    float* dv_lr;
    const int32_t* idx_y;
    const int32_t* idx_x;
    int32_t B, heads, Ho, Wo, h, w, Dq, Dv, ky, kx;
    float scale;
    int32_t path;            /* 0.4.1 (was `reserved`, 0): NAF_XNA_AUTO, or insist on NAF_XNA_MFMA / NAF_XNA_ROWS / NAF_XNA_GENERIC -- GENERIC
                                runs the table-driven scalar kernel on ANY shape (the independent reference of the parity tests) */
    int64_t q_stride[4];
    int64_t k_stride[4];
    int64_t v_stride[4];
    int64_t dout_stride[4];
    int64_t dq_stride[4];
    void* workspace;         /* version >= 104: device scratch of naf_xna_bwd_workspace_bytes() bytes, 16-byte aligned (NAF_XNA_ROWS) */
    int64_t workspace_bytes;
} naf_xna_bwd_args;
/* NAF_XNA_MFMA, NAF_XNA_ROWS or NAF_XNA_GENERIC: the kernel naf_xna_bwd would run under a->path; negative naf_status on invalid arguments
 * (-NAF_ERR_UNSUPPORTED when a->path insists on a kernel that does not serve the shape).
 * NAF_XNA_ROWS (round 3) is the matrix-core backward of the square windows <= 15 the cell kernel does not take, at any integer
 * ratio and at non-integer ratios whose 16-query tiles stay within 32 low-res columns (tap multiplicities as in the forward): the denoising call (denoising.py:213,301: ratio 1, one head of Dq = 64 ... 512 as in naf_xna_fwd's
 * NAF_XNA_ROWS, Dv <= 32) and heads of 64 with Dv in {32, 64, 96, 128, 192, 256} at any integer ratio -- the reference's own
 * training step (train.py:113-133: 16^2 -> 32^2, ratio 2), patch-14 backbones (ratio 14), 15 x 15 windows.  It needs idx_y /
 * idx_x like the table-driven kernel AND `workspace` (per-query softmax statistics, 16 bytes per query); without a workspace
 * the call runs the table-driven kernel instead.  It adds into the zeroed dk_lr / dv_lr like the other kernels (one read-add-write per key, or fp32
 * atomics where a key tile's rows are shared between waves).
 * Non-finite inputs on the NAF_XNA_ROWS kernel: a tile of 16 queries (keys) contracts over the whole 32-column chunks that hold its
 * neighbourhoods, non-neighbours with zero weights, so an Inf / NaN in q, k_lr, v_lr or dout surfaces (as NaN) in the gradients of
 * every element whose tile's chunk rows hold it -- a superset of the neighbourhoods the reference and the table-driven kernel
 * confine it to, but never further: since 0.4.0 a chunk that skips its upper 16 slots clears them, so nothing of an earlier tile
 * (0.3.x: stale LDS rows of the wave's previous tile, anywhere in the image) can reach the products. */
int naf_xna_bwd_supported(const naf_xna_bwd_args* a);
size_t naf_xna_bwd_workspace_bytes(const naf_xna_bwd_args* a);
/* 0.4.1: the launches of the NAF_XNA_MFMA backward for these arguments -- the widths of the channel chunks in launch order, at most `cap` of them written
 * to out (out may be NULL with cap 0).  Returns their number: 1 = the whole head in one launch, 0 = another kernel serves the call
 * (naf_xna_bwd_supported), negative naf_status on invalid arguments.  A pure host-side query (no device call); pointers are only checked, not read.
 * NUMERICS OF A CHUNKED CALL: dV splits by channel and dK_lr is accumulated in fp32, so neither depends on the plan; dQ is a sum over the
 * chunks that travels through the caller's bf16 dq buffer -- launch n > 1 reads dq back, adds its fp32 partial and rounds to bf16 again -- so dq
 * carries one bf16 rounding PER CHUNK (n * 2^-9 relative to the running sum, worst case) instead of one: with the plans in force (at most 4
 * chunks: 15 x 15 at Dv 256) that is <= 0.8 % of |dq| in the worst case and 0.2-0.3 % measured against the one-launch kernel on the same
 * inputs (tests/test_gpu_parity.py::test_chunked_backward_dq_against_the_one_launch_kernel).  A host that needs the single rounding calls the
 * backward per chunk itself with fp32-accumulating glue, or uses windows / widths that run whole (k <= 9, or Dv <= 128 at 11 x 11). */
int naf_xna_bwd_chunk_plan(const naf_xna_bwd_args* a, int32_t* out, int cap);
int naf_xna_bwd(const naf_xna_bwd_args* a, naf_stream_t stream);

/* 0.4.3: the backward with a gradient of the scores.  naf_xna_fwd's `logits` are L[i, j] = scale * q_i . k_j (window slot j = ty * kx + tx,
 * the taps of idx_y / idx_x); a loss that uses them as well as the output gives, with G = dL,
 *     dS[i, j] = scale * (P[i, j] * (dP[i, j] - delta[i]) + G[i, j])      dQ[i] = sum_j dS[i, j] k_j      dK[j] += sum_i dS[i, j] q_i
 * (P, delta and dV do not depend on G).  Every kernel adds G with one fma onto the dS it already forms, so a zero G gives naf_xna_bwd's
 * results bit for bit.  The kernel is chosen as naf_xna_bwd chooses it, except that non-integer ratios (repeated taps: a (query, key) pair is
 * several slots) run the table-driven kernel instead of NAF_XNA_ROWS, and so do cell shapes whose dlogits_stride[3] * (Wo / w) + ky * kx
 * reaches 2^29; naf_xna_bwd_scores_supported says which, and the caller brings tables / workspace accordingly (naf_xna_bwd_workspace_bytes
 * may name bytes for a shape that then runs the table-driven kernel, which needs none).  Any non-negative strides serve (0 included: a
 * gradient expanded over an axis).  The chunked cell backward adds G in its first channel chunk only.  s == NULL or s->dlogits == NULL: exactly naf_xna_bwd. */
typedef struct naf_xna_bwd_scores_args {
    const float* dlogits;        /* device fp32 [B, heads, Ho, Wo, ky*kx], slot axis contiguous, 4-byte aligned: the gradient of `logits` */
    int64_t dlogits_stride[4];   /* {b, head, y, x} in elements, any non-negative values */
} naf_xna_bwd_scores_args;
/* NAF_XNA_MFMA / NAF_XNA_ROWS / NAF_XNA_GENERIC: the kernel naf_xna_bwd_scores would run under a->path, negative naf_status on invalid
 * arguments (of either struct; -NAF_ERR_UNSUPPORTED where a->path insists on a kernel that does not serve the request).  A pure host-side
 * query (no device call); pointers are only checked, not read. */
int naf_xna_bwd_scores_supported(const naf_xna_bwd_args* a, const naf_xna_bwd_scores_args* s);
int naf_xna_bwd_scores(const naf_xna_bwd_args* a, const naf_xna_bwd_scores_args* s, naf_stream_t stream);

/* ---- whole forward in one call ----------------------------------------------------------------------
 * Replaces NAF.forward (src/model/naf.py:104-116) for the default architecture (dim 256 = two 128-channel
 * encoder branches with img_layers blocks, any RoPE / attention head counts dividing it, any image and output size): every launch
 * of the path above -- conv stem, key pooling, value packing, attention -- is issued from one host call on the
 * caller's stream, so a C/C++ host needs nothing else and a Python host pays one foreign call per forward instead
 * of fourteen.  Any geometry naf_xna_fwd accepts is served: with an integer ratio and Wo/w a multiple of 16 the
 * queries are rotated on load (no query buffer); otherwise they are materialised in the workspace, and when the
 * attention runs on a table-driven kernel the index tables are built in the workspace by
 * naf_axis_index_table_device.  The call is capturable in a hipGraph (no host-side copies, no allocation).
 *   image     device [B, 3, H, W] f32/bf16, strides {b, c, y, x}
 *   features  device [B, C, h, w] f32/bf16/half, strides {b, c, y, x}
 *   out       device out_dtype, dense channels-last [B, Ho, Wo, C] (logical [B, C, Ho, Wo] view for the caller);
 *             feat_dtype NAF_F16 goes with out_dtype NAF_F16 and only with it (NAF_ERR_INVALID otherwise): the packed values in
 *             the workspace are half (same bytes), see naf_dtype_supported
 *   branch[i] parameters of encoder / sem_encoder (naf.py:26-27): conv0 weight f32 [128][3][k0][k0] + bias, then
 *             per block layer l < nlayer: GroupNorm weight / bias f32 [128], conv weight packed bf16
 *             [k*k][128][128] (= weight.permute(2,3,0,1)) and bias f32 [128]
 *   tab_y / tab_x  RoPE tables from naf_rope_tables for the OUTPUT size (Ho, Wo)
 *   workspace device scratch of naf_forward_workspace_bytes() bytes (activations, GroupNorm sums, keys, packed
 *             values, queries / index tables where needed); the library still owns no memory
 *   events    optional hipEvent_t handles recorded on the stream around the attention kernel
 *             (events[0] before, events[1] after) so that a caller can time it; NULL entries are skipped
 *             (phase_events, at the end of the struct, does the same for every phase of the call)
 * An image more than 4x the output is first shrunk (naf_preshrink_image), an image larger than the output has its
 * guidance pooled (naf_pool_guidance; an output larger than the image is the same adaptive pooling), exactly as
 * naf.py:37-49 does; `logits` adds the reference's return_weights output.  Other widths return
 * NAF_ERR_UNSUPPORTED: compose the individual entry points instead. */
#define NAF_MAX_STEM_LAYERS 8
typedef struct naf_stem_branch {
    const float* conv0_weight;
    const float* conv0_bias;
    int32_t conv0_ksize; /* 1 or 3 */
    int32_t ksize;       /* block convolutions: 1 or 3 */
    const float* gn_weight[NAF_MAX_STEM_LAYERS];
    const float* gn_bias[NAF_MAX_STEM_LAYERS];
    const void* conv_weight_packed[NAF_MAX_STEM_LAYERS];
    const float* conv_bias[NAF_MAX_STEM_LAYERS];
} naf_stem_branch;
typedef struct naf_forward_args {
    const void* image;
    const void* features;
    void* out;
    const float* tab_y;
    const float* tab_x;
    void* workspace;
    size_t workspace_bytes;
    void* events[2];
    float* logits; /* optional: return_weights (attentions.py:27-28), dense [B, heads, Ho, Wo, ksize*ksize]; NULL = none */
    naf_stem_branch branch[2];
    int32_t nlayer; /* GroupNorm/SiLU/conv layers per branch = 2 * img_layers */
    int32_t image_dtype, feat_dtype, out_dtype; /* naf_dtype */
    int32_t B, H, W, h, w, C, heads, ksize;
    int32_t Ho, Wo; /* output size; 0 = the image size.  Different from the image: the guidance is pooled (naf.py:34) */
    int32_t heads_rope, reserved; /* RoPE heads (naf.py:73-85 heads_rope); 0 = the attention heads */
    float gn_eps;
    float scale; /* <= 0: Dq^-0.5 */
    int64_t image_stride[4];
    int64_t feat_stride[4];
    /* optional hipEvent_t handles recorded on the stream at the phase boundaries of the forward (NULL entries skipped), so that a
     * caller can time the parts of the ONE call.  Appended in 0.1.3 (naf_version() >= 103): callers that zero-initialise the struct
     * need no change.  Since 0.1.5 (>= 105) the two branches' layers alternate -- first convolutions, block layer 0 of both
     * branches, layer 1 of both, ...; within a stage the branch with 1x1 block layers goes first -- and the entries are:
     * [0] start, [1] after both first convolutions, [2] before block-layer stage 1 (stage 0 when there is one layer), [3] after
     * that stage's first launch (the 1x1 layer), [7] after its second launch (the 3x3 layer), [4] end of the conv stem (guidance
     * pooled to the output size where needed), [5] after RoPE / key pooling, value packing and index tables (= start of the
     * attention kernel), [6] after the attention kernel.  [3]-[2] and [7]-[3] time ONE launch of each layer kernel inside the
     * call.  (103-104: [1] / [2] after branch 0's first convolution / block layers, [3] after branch 1's first convolution.)
     * With two streams (naf_forward_ex below; 0.2.0 - 0.3.x: naf_forward itself, on a library-owned stream) the two branches'
     * block layers run side by side -- the caller's stream (3x3 branch) and the lent one (1x1 branch), forked by an event after
     * the first convolutions and joined before the attention; the call stays capturable -- and [2] / [7] bracket one 3x3 launch on
     * the caller's stream (1x1 launches run beside it), [3] is recorded behind one 1x1 launch on the second stream; [0], [1], [4],
     * [5], [6] as before.  On 16 x 16 pixel cells the key pooling rides on the last block layers (naf_stem_conv_keys_fwd) and
     * the value packing runs on the second stream beside the first convolutions, so nothing is left between [4] and [5]. */
    void* phase_events[8];
} naf_forward_args;
size_t naf_forward_workspace_bytes(const naf_forward_args* a);
/* 0.4.2: the same for a given naf_forward_ex `flags`: with NAF_FWD_ONE_STREAM the fourth activation buffer ([B, H, W, 128] bf16, a quarter
 * of the workspace at 1024^2) is left out -- a call that cannot fork (naf_forward, naf_forward_ex without a lent stream or with
 * NAF_FWD_ONE_STREAM) accepts that smaller workspace; every other buffer keeps its offset (naf_forward_workspace_view). */
size_t naf_forward_workspace_bytes_ex(const naf_forward_args* a, uint32_t flags);
/* 1 when naf_forward serves these arguments, 0 when not (then NAF_ERR_UNSUPPORTED), negative naf_status if invalid. */
int naf_forward_supported(const naf_forward_args* a);
/* Every launch on the caller's stream, the two branches' layers alternating (= naf_forward_ex(a, NULL, 0, stream)). */
int naf_forward(const naf_forward_args* a, naf_stream_t stream);

/* Where naf_forward keeps its intermediate tensors in the caller's workspace (0.4.0), for hosts that want them after a call -- the
 * guidance and keys of an image to inspect or to compare (tests/test_gpu_fullsize.py holds the keys the stem's last layers pooled
 * against the oracle this way) -- valid from the completion of one call on the workspace until the next one starts:
 *   NAF_FWD_BUF_GUIDANCE  bf16 [B, Ho, Wo, 256] channels-last: the conv stem's output at the output size, UN-rotated (what the
 *                         attention kernel reads as queries when it rotates on load)
 *   NAF_FWD_BUF_KEYS      bf16 [B, h, w, 256]: pool(RoPE(guidance)) (naf.py:63-69)
 *   NAF_FWD_BUF_VALUES    bf16 [B, h, w, C]: the packed features
 * *offset is in bytes from a->workspace.  Returns NAF_OK, or NAF_ERR_INVALID for a bad `which` / arguments. */
enum naf_forward_buffer { NAF_FWD_BUF_GUIDANCE = 0, NAF_FWD_BUF_KEYS = 1, NAF_FWD_BUF_VALUES = 2 };
int naf_forward_workspace_view(const naf_forward_args* a, int32_t which, size_t* offset, size_t* bytes);

/* naf_forward_ex (0.4.0): the same forward with the two encoder branches side by side on TWO streams -- the caller's (3x3 branch)
 * and a second one the CALLER owns and lends for the duration of the call (1x1 branch, value packing): forked from `stream` by
 * fork_event after the first convolutions, joined back into `stream` through join_event before the attention kernel AND ON
 * EVERY ERROR RETURN after the fork, so that when the call returns -- with any status -- everything it queued on aux->stream is
 * ordered before whatever the caller queues on `stream` next (the workspace may be reused or freed in stream order).
 * Same kernels, bit-identical output; -2.5 % per step at 1024^2 (the HBM-bound 1x1 workgroups fill the CUs a 3x3 launch's tail
 * leaves idle).  The library keeps nothing: one naf_forward_aux serves one call at a time -- give every host thread / caller
 * stream that issues forwards concurrently its own (naf_forward_aux_create is a convenience constructor; any non-blocking stream
 * and two hipEventDisableTiming events of the same device do).  Capturable: a capture on `stream` pulls aux->stream in through
 * the fork and releases it at the join, like any fork / join inside a hipGraph capture; use an aux that no other thread uses
 * eagerly meanwhile.  aux == NULL (or aux->stream == NULL): one stream.
 * flags: NAF_FWD_CONV0_EXACT   the 3x3 first convolution with exact fp32 products (NAF_CONV0_EXACT)
 *        NAF_FWD_ONE_STREAM    ignore aux;  NAF_FWD_TWO_STREAMS  use aux whenever it is given.  Neither: the library's plan --
 *        two streams unless the 3x3 layer launch takes every CU in one round of short segments (12 .. 40 rows per workgroup:
 *        512^2 at batch 1, 256^2 at batch 2 or 4), where nothing of the 1x1 branch can run beside it and its workgroups then
 *        stand in the next 3x3 launch's way: one stream -2 ... -4.5 % there, two streams -1.5 ... -13 % everywhere else
 *        (interleaved sweep over sizes and batches, profiles/r05_streams_rule.txt).
 * phase_events with two streams: [2] / [7] bracket one 3x3 launch on `stream`, [3] is recorded behind one 1x1 launch on
 * aux->stream; the others as documented above. */
typedef struct naf_forward_aux {
    naf_stream_t stream; /* hipStream_t on the device of the call; created non-blocking by naf_forward_aux_create */
    void* fork_event;    /* hipEvent_t */
    void* join_event;    /* hipEvent_t */
} naf_forward_aux;
#define NAF_FWD_CONV0_EXACT 1u
#define NAF_FWD_ONE_STREAM 2u
#define NAF_FWD_TWO_STREAMS 4u
/* Creates a non-blocking stream and two timing-less events on the CURRENT device into *out (the caller owns them and destroys them
 * with naf_forward_aux_destroy, which also zeroes the struct; destroying an all-NULL struct is a no-op).  On failure nothing is
 * left behind and *out is all NULL. */
int naf_forward_aux_create(naf_forward_aux* out);
int naf_forward_aux_destroy(naf_forward_aux* aux);
/* 2 when naf_forward_ex(a, aux, flags, .) with a non-NULL aux would fork onto the second stream, 1 when it would run on one
 * stream, 0 / negative as naf_forward_supported. */
int naf_forward_streams(const naf_forward_args* a, uint32_t flags);
int naf_forward_ex(const naf_forward_args* a, const naf_forward_aux* aux, uint32_t flags, naf_stream_t stream);

/* ---- attention forward with the training objective in its epilogue (added after the PCA entries; detect by symbol) ----------------
 * The reference's training step (train.py:127-132) is
 *     pred = model(img, lr_feats, hr_feats.shape[-2:]);  loss = mse(pred.float(), hr_feats.float())
 * and the gradient of that loss with respect to pred is (2/N)(pred - hr_feats), N = B*C*Ho*Wo.  The table-driven MFMA kernel
 * (NAF_XNA_UNION) holds every output element in an fp32 accumulator just before it stores it; this entry subtracts the target there,
 *     e = acc - target (fp32),   loss = sum e^2 / N,   dout = bf16(e * (2/N))      (2/N applied in fp32, ONE rounding to bf16)
 * and writes dout where naf_xna_fwd writes out: the prediction, its fp32 copy and the fp32 gradient never exist, and dout -- computed
 * from the UNROUNDED prediction -- is the `dout` of naf_xna_bwd as it stands.
 *   a          naf_xna_args as for naf_xna_fwd on the NAF_XNA_UNION path (a.path is ignored: this entry has no other kernel; idx_y / idx_x
 *              required and canonical; logits and rope_tab_* must be NULL).  a.out is the GRADIENT buffer: [B, heads, Ho, Wo, Dv] by
 *              o_stride, a.out_dtype must be NAF_BF16.  a.out == NULL: loss only (validation), nothing but loss / workspace is written
 *   target     device, target_dtype (NAF_F32 / NAF_BF16), logical [B, C, Ho, Wo] with C = heads * Dv (head g owns channels [g*Dv, (g+1)*Dv)),
 *              ELEMENT strides target_stride = {b, c, y, x}, any values: plain NCHW, a channels-last view (c stride 1: what a ViT wrapper's
 *              "b (h w) c -> b c h w" gives), a channel slice of a wider tensor.  With c stride 1, the other strides multiples of 4 and the
 *              pointer 16-byte (fp32) / 8-byte (bf16) aligned a lane's four channels are one load; every other target is read element by
 *              element.  The pointer must be aligned to its element size (NAF_ERR_INVALID otherwise).  Never written
 *   loss       device float[1]: sum e^2 / N
 *   workspace  device, naf_xna_mse_workspace_bytes(a) bytes, 4-byte aligned, caller-owned, needs no clearing: one fp32 partial sum per
 *              wave of the attention launch.  A second, one-workgroup launch adds them in fp64 in a fixed order and writes loss.  No
 *              atomics anywhere: two calls on the same inputs give bit-equal loss and dout
 * naf_xna_mse_supported: 1 when naf_xna_mse_fwd serves the arguments (Dq = 64, Dv % 16 == 0, square odd window 3 .. 15, Ho >= h, Wo >= w,
 * 16-byte aligned q / k_lr / v_lr / out with the stride rules of NAF_XNA_UNION), else a negative naf_status with naf_last_error():
 * -NAF_ERR_INVALID for arguments no kernel could serve (NULL q / k_lr / v_lr / target, bad sizes or dtypes, a gradient buffer that is
 * not bf16, logits or rope_tab_* given, a misaligned target), -NAF_ERR_UNSUPPORTED for a valid request outside the list -- the caller
 * then composes naf_xna_fwd with its own loss.  A pure host-side query: pointers are checked, never read; idx_y / idx_x, loss and the
 * workspace are not looked at.  naf_xna_mse_fwd additionally wants idx_y / idx_x, loss and a workspace of at least
 * naf_xna_mse_workspace_bytes(a) bytes (NAF_ERR_INVALID).  naf_xna_mse_workspace_bytes is 0 for arguments that are not served.
 * scale <= 0 selects Dq^-0.5.  Caller-owned memory and stream; capturable. */
typedef struct naf_xna_mse_args {
    naf_xna_args a; /* a.out: the gradient (bf16) or NULL */
    const void* target;
    float* loss;
    void* workspace;
    size_t workspace_bytes;
    int32_t target_dtype; /* naf_dtype */
    int32_t reserved;     /* must be 0 */
    int64_t target_stride[4];
} naf_xna_mse_args;
int naf_xna_mse_supported(const naf_xna_mse_args* a);
size_t naf_xna_mse_workspace_bytes(const naf_xna_mse_args* a);
int naf_xna_mse_fwd(const naf_xna_mse_args* a, naf_stream_t stream);

/* ---- DAVIS region similarity J and boundary measure F: the integer counts behind both (added after the objective entries; detect by symbol) ----
 * Replaces the device-side arithmetic of davis_db_eval_iou / davis_f_measure / _seg2bmap (evaluation/eval_video_seg.py:145-248), which the
 * reference runs on the host per (object, frame) on float64 one-hot arrays read back from PNG files.  annotation and segmentation are label
 * maps: 0 is background, 1 .. N are objects, anything above N belongs to no object.  For object o and frame t, with g = (annotation[t] == o)
 * and s = (segmentation[t] == o), the call ADDS into counts[o - 1][t][0 .. 5]:
 *   [0] inters    |g and s|                  [1] union     |g or s|
 *   [2] n_seg     |B(s)|                     [3] n_gt      |B(g)|
 *   [4] seg_hits  pixels p of B(s) with a pixel q of B(g) at |p - q|^2 <= r2         [5] gt_hits  the converse
 * B(m), the boundary map of a 0/1 mask, is the 3 x 3 Sobel pair on m with the border rule "reflect without repeating the edge" (row -1 is
 * row 1, row H is row H - 2; OpenCV's BORDER_REFLECT_101): a pixel is set when either response is non-zero.  Against an empty boundary
 * there are 0 hits.  J = inters / union and F = 2PR / (P + R), P = seg_hits / (n_seg + 1e-10), R = gt_hits / (n_gt + 1e-10), are the caller's
 * (fp64).  Squared distances are integers, so `distance <= bound_pix` is `|p - q|^2 <= r2` with r2 = floor(bound_pix^2), exactly.
 *   annotation, segmentation   device uint8, dense [T][H][W]
 *   counts                     device int64 [N][T][6], ZEROED by the caller on the same stream before the call
 *   r2, half_width             floor(bound_pix^2) and floor(bound_pix): half_width^2 <= r2 < (half_width + 1)^2 (NAF_ERR_INVALID otherwise)
 * One launch for the sequence; a workgroup owns one NAF_DAVIS_TILE_H x NAF_DAVIS_TILE_W tile of one frame, stages both maps' tile with its halo
 * once, and for every label present in the tile packs the two boundary maps into 64-bit words and tests each boundary pixel's disk row by
 * row.  Counters are reduced per wave and per workgroup; a workgroup adds at most one 64-bit integer atomic per (object, counter).  Integer
 * adds: two runs give the same bits.
 * Served: 1 <= N <= 32, 2 <= H, W <= 16384, T >= 1, 1 <= half_width <= 32, tiles * T below 2^31; anything else that is well formed is
 * NAF_ERR_UNSUPPORTED with the limit named in naf_last_error().  naf_davis_jf_select is a host-only query (it reads the scalar fields only
 * and touches no device): NAF_OK, NAF_ERR_UNSUPPORTED or NAF_ERR_INVALID (NULL args, N, T, H or W < 1, half_width < 0, r2 and half_width
 * that do not belong together, non-zero reserved).  naf_davis_jf additionally refuses NULL pointers and counts not 8-byte aligned.
 * Caller-owned memory and stream; nothing is allocated; capturable. */
#define NAF_DAVIS_TILE_W 64
#define NAF_DAVIS_TILE_H 32
#define NAF_DAVIS_MAX_OBJECTS 32
#define NAF_DAVIS_MAX_HALF_WIDTH 32
typedef struct naf_davis_jf_args {
    const uint8_t* annotation;
    const uint8_t* segmentation;
    int64_t* counts;
    int32_t T, H, W, N;
    int32_t r2, half_width;
    int32_t reserved[2]; /* must be 0 */
} naf_davis_jf_args;
int naf_davis_jf_select(const naf_davis_jf_args* a);
int naf_davis_jf(const naf_davis_jf_args* a, naf_stream_t stream);

/* ---- soft masks to a label map: upsample, norm_mask, argmax, nearest resize (added after the DAVIS entries; detect by symbol) ----
 * Replaces what the reference does with a propagated frame before it scores it (evaluation/eval_video_seg.py:444-457): F.interpolate
 * (bilinear, align_corners = False) of the K soft masks [h, w] to the mid grid [mid_h, mid_w], norm_mask per channel, torch.max over the
 * channels, .cpu() and Image.resize((out_w, out_h), 0).  With u[c] the upsampled channel (ATen's fp32 arithmetic, every operation rounded on
 * its own: scale = float(in) / float(out), src = max(scale * (dst + 0.5f) - 0.5f, 0), i0 = (int)src, i1 = i0 + (i0 < in - 1), l1 = src - i0,
 * l0 = 1 - l1, value = h0 * (w0 * v00 + w1 * v01) + h1 * (w0 * v10 + w1 * v11)) and mx, mn its maximum and minimum over the mid grid:
 *   n[c] = (u[c] - mn) / (mx - mn) where mx > 0 (subtract, then a correctly rounded divide), u[c] where not;
 *   mx > 0 with mx == mn divides 0 by 0: the channel is NaN everywhere, as in the reference;
 *   label = the first channel holding the maximum of n, a NaN counting above every number (torch.max on the CPU);
 *   out[oy][ox] = label at mid pixel (tab_y[oy], tab_x[ox]).  NaN inputs are unspecified.
 *   seg          device fp32, K channels of h x w; seg_stride = elements between channels, rows, columns (any values, 0 and negative included)
 *   tab_y, tab_x device int32 [out_h], [out_w]: the mid row / column each output row / column reads; naf_nearest_resize_table(mid, out) for
 *                Pillow's nearest resize.  Entries are clamped to the mid grid
 *   out          device uint8, out_h rows of out_w bytes, out_stride (>= out_w) bytes between rows; nothing else is written
 *   workspace    device, 4-byte aligned, at least NAF_MASK_LABELS_WORKSPACE_BYTES; need not be initialised
 * Two launches on the caller's stream: pass 1 evaluates u at every mid pixel and leaves one (min, max) pair per workgroup and channel in the
 * workspace; pass 2 finishes the pairs, evaluates the K values at each OUTPUT pixel's source, normalises and stores the label.  Both passes
 * get u from one inline function, so the extreme pixels normalise to exactly 1 and 0; no atomics, no float order that depends on scheduling:
 * two runs give the same bits.  The [K, mid_h, mid_w] map is never written.
 * Served: 1 <= K <= NAF_MASK_LABELS_MAX_CHANNELS, every size 1 .. NAF_MASK_LABELS_MAX_SIZE; anything else that is well formed is
 * NAF_ERR_UNSUPPORTED with the limit named in naf_last_error().  naf_mask_labels_select is a host-only query (it reads the scalar fields only
 * and touches no device): NAF_OK, NAF_ERR_UNSUPPORTED or NAF_ERR_INVALID (NULL args, K or a size < 1, non-zero reserved).  naf_mask_labels
 * additionally refuses NULL or misaligned pointers, a workspace that is too small and out_stride < out_w.
 * Caller-owned memory and stream; nothing is allocated; capturable.
 *
 * naf_nearest_resize_table (host only) writes the n_out source indices Pillow's Image.resize(size, 0) reads along an axis of n_in pixels:
 * with s = (double)n_in / n_out, xo = 0.5 * s; out[x] = min((int)xo, n_in - 1); xo += s.  The ACCUMULATION in doubles is the definition:
 * floor((2x + 1) n_in / (2 n_out)) differs from it (at 64 of the 854 columns of 976 -> 854). */
#define NAF_MASK_LABELS_MAX_CHANNELS 64
#define NAF_MASK_LABELS_MAX_SIZE 16384
#define NAF_MASK_LABELS_WORKSPACE_BYTES 8192
typedef struct naf_mask_labels_args {
    const float* seg;
    const int32_t* tab_y;
    const int32_t* tab_x;
    uint8_t* out;
    float* workspace;
    size_t workspace_bytes;
    int64_t seg_stride[3];
    int64_t out_stride;
    int32_t K, h, w, mid_h, mid_w, out_h, out_w;
    int32_t reserved; /* must be 0 */
} naf_mask_labels_args;
int naf_mask_labels_select(const naf_mask_labels_args* a);
int naf_mask_labels(const naf_mask_labels_args* a, naf_stream_t stream);
int naf_nearest_resize_table(int32_t* out, int32_t n_in, int32_t n_out);

/* ---- point queries: the attention at N pixels (added after the label-map entries; detect by symbol) ----
 * What the reference's attention viewer reads out of model(image, feats, size, return_weights=True) (notebooks/attention_maps.ipynb, cell 11:
 * one pixel's ky*kx scores per head out of the [B, heads, Ho, Wo, ky*kx] tensor) and what a sparse consumer (keypoints, correspondences) wants of
 * the feature map, for N points (b, y, x) in OUTPUT coordinates, without either dense tensor.  Three optional outputs, each skipped when NULL:
 *   logits  device float [N][heads][ky*kx] dense: the scaled pre-softmax scores, i.e. the rows of naf_xna_fwd's `logits`
 *   probs   device float [N][heads][ky*kx] dense: their softmax
 *   out     device float [N][heads*Dv] dense: the upsampled feature vectors; needs v_lr (v_lr NULL with out NULL: weights only)
 * Operands:
 *   k_lr, v_lr  as naf_xna_fwd's (layout contract above: pointer plus {b, head, y, x} element strides, last dim contiguous, stride 0 allowed);
 *               v_dtype NAF_BF16 or NAF_F16 says what v_lr holds
 *   idx_y, idx_x  device int32 [Ho][ky], [Wo][kx] from naf_axis_index_table (entries are clamped to the low-res grid)
 *   points  device int32 [N][3] = (b, y, x), dense
 *   q       device bf16 [B, heads, Ho, Wo, Dq], strides {b, head, y, x}, Dq contiguous: the rotated queries of naf_rope_pool_fwd -- or, with
 *           rope_tab_y / rope_tab_x (device float [Ho][2][Dq/4] / [Wo][2][Dq/4] from naf_rope_tables, both or neither; Dq % 4 == 0), the
 *           UN-rotated guidance: the kernel rotates the N * heads vectors it reads, same arithmetic and bf16 rounding as naf_rope_pool_fwd
 *           (both forms give the same bits), so no query tensor is written for a handful of points
 * One wave per (point, head), the loop order and the reductions of the table-driven scalar kernel (NAF_XNA_GENERIC): for a point's
 * (b, head, y, x), logits and out are bit-identical to what naf_xna_fwd(path = NAF_XNA_GENERIC, out_dtype = NAF_F32) writes for that pixel (half
 * values: to that kernel's accumulator before its rounding to half).  Any Dq, Dv, ky, kx with 16 * (ky*kx + Dq) bytes <= 64 KB
 * (NAF_ERR_UNSUPPORTED beyond).
 * A coordinate is compared with the sizes before it is used in an address: a point outside [0, B) x [0, Ho) x [0, Wo) reads nothing and gets
 * NaN in its rows of every output; the other rows are unaffected.  Nothing is written outside the N rows.  N = 0 launches nothing.
 * scale <= 0: Dq^-0.5.  Caller-owned memory and stream; nothing is allocated; capturable. */
typedef struct naf_xna_points_args {
    const void* q;
    const void* k_lr;
    const void* v_lr;
    const int32_t* points;
    const int32_t* idx_y;
    const int32_t* idx_x;
    const float* rope_tab_y;
    const float* rope_tab_x;
    float* logits;
    float* probs;
    float* out;
    int32_t N, B, heads, Ho, Wo, h, w, Dq, Dv, ky, kx;
    int32_t v_dtype; /* naf_dtype of v_lr: NAF_BF16 or NAF_F16 */
    float scale;
    int32_t reserved; /* must be 0 */
    int64_t q_stride[4];
    int64_t k_stride[4];
    int64_t v_stride[4];
} naf_xna_points_args;
int naf_xna_points(const naf_xna_points_args* a, naf_stream_t stream);

/* ---- frame preparation: resized, normalised views of one image from one launch (added after the point queries; detect by symbol) ----
 * Replaces the torch-eager work the reference's callers do before anything reaches the model: evaluation/eval_video_seg.py:577-597 (ToTensor,
 * bilinear resize to a multiple of the patch size, two normalisations, bicubic resize of the upsampler's image), train.py:115-126 with
 * utils/training.py:47 (bilinear resize, two normalisations, two bilinear resizes of the results), evaluation/eval_seg_probing.py:97-98 (two
 * normalisations, a horizontal flip in training).  One call writes up to NAF_IMAGE_PREP_MAX_VIEWS derived images ("views") of ONE source; no
 * intermediate image is written.
 *
 * A view is: first resize -> normalise -> second resize -> store.  Every step is optional.  All arithmetic is fp32 and every operation is
 * rounded on its own (no fused multiply-add); fl() below is that rounding.
 *   source value   NAF_IMAGE_PREP_U8: fl(float(u) / 255), a correctly rounded divide (ToTensor on the host); NAF_F32: the value as it is;
 *                  NAF_BF16: widened.  With hflip, source column x reads column W - 1 - x.
 *   resize n_in -> n_out, per axis (align_corners = False, no antialiasing): scale = fl(float(n_in) / float(n_out)),
 *                  real = fl(fl(scale * fl(dst + 0.5)) - 0.5) -- ATen's DEVICE arithmetic, as for naf_preshrink_image.
 *     NAF_PREP_BILINEAR  src = max(real, 0), i0 = (int)src, i1 = min(i0 + 1, n_in - 1), l1 = fl(src - i0), l0 = fl(1 - l1);
 *                  value = h0 * (w0 * v00 + w1 * v01) + h1 * (w0 * v10 + w1 * v11), each product and sum rounded, in this order.
 *     NAF_PREP_BICUBIC   (ATen's, A = -0.75) i = floor(real), t = fl(real - i), u = fl(1 - t);
 *                  c1(x) = (((A + 2) x - (A + 3)) x) x + 1, c2(x) = ((A x - 5A) x + 8A) x - 4A, each operation rounded (1.25, 2.25, -3.75, -6,
 *                  -3 are exact); the weights [c2(fl(t + 1)), c1(t), c1(u), c2(fl(u + 1))] go on taps i - 1 .. i + 2, every tap index clamped
 *                  into [0, n_in - 1] (2 - t is taken as (1 - t) + 1, as ATen does).  Row pass first: ((v0 cx0 + v1 cx1) + v2 cx2) + v3 cx3,
 *                  left to right; then the same form with the y weights over the four row results.
 *     NAF_PREP_NONE      the sizes must be equal and the value passes through.
 *                  An equal-size bilinear or bicubic resize returns the value exactly for finite inputs.
 *   normalise      fl(fl(v - mean[c]) / std[c]), the divide correctly rounded (no reciprocal); mean and std are the caller's fp32 values.
 *                  normalise = 0 skips the step (it is not "subtract 0").  std[c] == 0 is NAF_ERR_INVALID.
 *   second resize  reads the normalised first-stage image exactly as if that fp32 image had been written to memory; it is not written.
 *   store          NAF_F32 as it is; NAF_BF16 rounded to nearest even.
 * Operands:
 *   src          device; 3 channels of B images of H x W; src_stride = ELEMENTS between images, channels, rows, columns (any values: an HWC
 *                uint8 frame is {H*W*3, 1, W*3, 3}, a CHW tensor {3*H*W, H*W, W, 1}, a crop of either keeps the parent's strides)
 *   view[i].out  device; [B][3][h2][w2] through out_stride = elements between images, channels, rows, columns; nothing outside the
 *                B x 3 x h2 x w2 elements those strides address is written.  Views must not overlap each other or the source.
 *   (h1, w1, mode1) the first resize H x W -> h1 x w1; (h2, w2, mode2) the second h1 x w1 -> h2 x w2, which is the view's size
 * One launch on the caller's stream: a flat list of 256-pixel workgroups over the views' output pixels, a thread per output pixel and its
 * three channels; pure gather -- no workspace, no atomics, no host synchronisation -- so two runs give the same bits.
 * Served: 1 <= n_views <= NAF_IMAGE_PREP_MAX_VIEWS, every size 1 .. NAF_IMAGE_PREP_MAX_SIZE, B >= 1 with B * h2 * w2 < 2^31 per view and fewer
 * than 2^31 workgroups in all; anything else that is well formed is NAF_ERR_UNSUPPORTED with the limit named in naf_last_error().
 * naf_image_prep_select is a host-only query (it reads the scalar fields only and touches no device): NAF_OK, NAF_ERR_UNSUPPORTED or
 * NAF_ERR_INVALID (NULL args, n_views, B or a size < 1, an unknown dtype or mode, NAF_PREP_NONE between different sizes, std == 0 or NaN
 * statistics on a normalised view, non-zero reserved).  naf_image_prep additionally refuses NULL pointers and pointers not aligned to their
 * element (4 bytes for fp32, 2 for bf16).  Caller-owned memory and stream; nothing is allocated; capturable. */
#define NAF_IMAGE_PREP_MAX_VIEWS 4
#define NAF_IMAGE_PREP_MAX_SIZE 16384
#define NAF_IMAGE_PREP_U8 3 /* src_dtype only: uint8, value u / 255 */
enum naf_prep_mode { NAF_PREP_NONE = 0, NAF_PREP_BILINEAR = 1, NAF_PREP_BICUBIC = 2 };
typedef struct naf_image_prep_view {
    void* out;
    int64_t out_stride[4]; /* elements between images, channels, rows, columns */
    int32_t out_dtype;     /* NAF_F32 or NAF_BF16 */
    int32_t h1, w1, mode1;
    int32_t normalise;
    int32_t h2, w2, mode2;
    float mean[3];
    float std[3];
    int32_t reserved[2]; /* must be 0 */
} naf_image_prep_view;
typedef struct naf_image_prep_args {
    const void* src;
    int64_t src_stride[4]; /* elements between images, channels, rows, columns */
    int32_t src_dtype;     /* NAF_IMAGE_PREP_U8, NAF_F32 or NAF_BF16 */
    int32_t B, H, W;
    int32_t hflip, n_views;
    int32_t reserved[2]; /* must be 0 */
    naf_image_prep_view view[NAF_IMAGE_PREP_MAX_VIEWS];
} naf_image_prep_args;
int naf_image_prep_select(const naf_image_prep_args* a);
int naf_image_prep(const naf_image_prep_args* a, naf_stream_t stream);

/* ---- attention with a COSINE head folded in (added after the image-preparation entries; detect by symbol) ------------
 * Open-vocabulary segmentation and "click a pixel, see what looks like it" heat maps compare the upsampled feature of every pixel with N
 * embeddings by their cosine (the reference normalises its upsampled maps the same way before comparing, evaluation/eval_video_seg.py:539-540).
 * With E [N, C], E^ = its rows divided by max(||row||, 1e-12), f[px] the C channels of naf(V) at the pixel, head g owning channels
 * [g*Dv, (g+1)*Dv):
 *     out[n, px]  = logit_scale * (E^[n] . f[px]) / max(||f[px]||_2, 1e-12)
 *     norms[px]   = ||f[px]||_2                                                       (fp32, unclamped)
 * A linear head cannot give this: the norm is quadratic in the attention's output.  The numerator is the head identity of
 * naf_xna_head_fwd on pv_lr = E^[:, g*Dv:(g+1)*Dv] @ V_g (no bias); for the denominator the kernel forms f_g = P_g . V_g on the matrix
 * cores from the SAME bf16 weights P_g, adds the squares of its fp32 results per pixel and drops them.  The [B, C, Ho, Wo] tensor is never
 * written.  A pixel whose feature is zero gets exactly 0 for every n (never NaN) and norm 0.
 *   q, k_lr   as in naf_xna_args (bf16, strides {b, head, y, x}, last dim contiguous, Dq = 64)
 *   pv_lr     device bf16 [B, heads, h, w, Npad] as for naf_xna_head_fwd, formed from the NORMALISED rows E^ (the caller normalises)
 *   v_lr      device bf16 [B, heads, h, w, Dv], strides v_stride {b, head, y, x}, last dim contiguous: the values pv_lr was formed from
 *   out       device float [B, Ho, Wo, N], element strides o_stride {b, y, x}, channel axis contiguous
 *   norms     device float [B, Ho, Wo], element strides norms_stride {b, y, x}, or NULL
 *   rope_tab_y / rope_tab_x   rotate-on-load exactly as in naf_xna_args (q is then the un-rotated channels-last guidance)
 *   logit_scale   multiplies the cosine, used as given (a zero-initialised struct yields zeros: set it, 1 for plain cosines); finite
 *   scale     the softmax scale; <= 0 selects Dq^-0.5
 * Kernel (xna_cos_kernel.h): naf_xna_head_fwd's -- one workgroup per (batch, low-res cell) loops over the heads, each head's softmax is
 * normalised in fp32 before its weights are rounded to bf16, the heads add up in fp32 -- with the head's value window staged next to
 * the K and PV windows in chunks of 64 channels.  No atomics: every output is deterministic, bit for bit.  A power-of-two factor on
 * the values changes no bit of out and scales norms exactly.
 * Served: the geometries of naf_xna_head_fwd (square odd window 3 .. 15, Dq = 64, integer ratio whose cell rows are row tiles, h, w >=
 * window, any head count, 1 <= N <= 256), Dv a multiple of 16, 16-byte aligned q / k_lr / pv_lr / v_lr with strides that are multiples
 * of 8 elements -- EXCEPT windows 13 and 15 with N > 64 (those instantiations would spill registers or exceed the LDS).
 * naf_xna_cos_select: NAF_XNA_HEAD_FUSED when naf_xna_cos_fwd serves the arguments, else a negative naf_status (with naf_last_error):
 * -NAF_ERR_INVALID for arguments no kernel could serve (NULL, N outside 1 .. 256, even window, non-finite logit_scale, non-zero reserved
 * ...), -NAF_ERR_UNSUPPORTED for a valid request outside the list above -- the caller then normalises the output of naf_xna_fwd.  A pure
 * host-side query: pointers are checked, never read.  path: naf_xna_head_path (the same answer for both today).  The struct must be
 * zero-initialised.  Caller-owned memory and stream; capturable; no workspace. */
typedef struct naf_xna_cos_args {
    const void* q;
    const void* k_lr;
    const void* pv_lr;
    const void* v_lr;
    float* out;
    float* norms; /* or NULL */
    const float* rope_tab_y;
    const float* rope_tab_x;
    int32_t B, heads, Ho, Wo, h, w, Dq, Dv, N, ky, kx;
    int32_t path; /* naf_xna_head_path */
    float scale;
    float logit_scale;
    int32_t reserved[2]; /* must be 0 */
    int64_t q_stride[4];
    int64_t k_stride[4];
    int64_t pv_stride[4];
    int64_t v_stride[4];
    int64_t o_stride[3];
    int64_t norms_stride[3];
} naf_xna_cos_args;
int naf_xna_cos_select(const naf_xna_cos_args* a);
int naf_xna_cos_fwd(const naf_xna_cos_args* a, naf_stream_t stream);

/* ---- ... with a classification objective on the scaled cosines (added after the cosine entries; detect by symbol) ------------
 * Training against cosines -- a cosine classifier as a dense probe, prompt / embedding tuning for open-vocabulary segmentation, a
 * learnable CLIP-style temperature: a cross-entropy on z[n] = s * cos[n] of naf_xna_cos_fwd.  A pixel's N cosines are in the registers
 * of four lanes when that kernel is done, so this entry computes, per pixel and in fp32, over the N channels, with
 * inv = 1 / max(||f||, 1e-12) and c[n] = (E^[n] . f) * inv the unscaled cosine,
 *     lse = max z + ln sum exp(z - max z),   label = argmax z (lowest index among equal maxima),   loss = lse - z[t]
 *     dlogits[n] = (s * inv) * (exp(z[n] - lse) - (n == t))       the gradient with respect to E^[n] . f
 *     dscale     = sum_n (exp(z[n] - lse) - (n == t)) * c[n]      the pixel's share of dloss / ds
 * and stores only what is asked for; neither the [B, C, Ho, Wo] features nor the [B, N, Ho, Wo] cosines need exist.  ||f|| does not depend
 * on the embeddings, so dlogits is the whole gradient of the loss with respect to pv_lr's attention output: it is the `dout` of
 * naf_xna_bwd for all heads at once (head stride 0) and that entry's dv_lr is dloss / dpv_lr; the caller carries it to E through the
 * low-res projection and the normalisation.  dloss / ds is the sum of the dscale map.
 *   cos        naf_xna_cos_args as for naf_xna_cos_fwd, except that `out` may be NULL; when given it receives the scaled cosines, bit for
 *              bit what naf_xna_cos_fwd stores for the same scale; norms as there
 *   target     device int64 [B, Ho, Wo], element strides t_stride {b, y, x}; NULL when only labels / cosines are wanted.  A pixel is
 *              IGNORED when target == ignore_index or target is outside [0, N) (the rule of naf_xna_head_ce_args)
 *   loss       device float [B, Ho, Wo] (loss_stride), or NULL: lse - z[t], 0 for an ignored pixel.  Needs target.  The caller reduces it
 *   labels     device uint8 [B, Ho, Wo] (labels_stride), or NULL; written for ignored pixels too
 *   dlogits    device bf16 [B, Ho, Wo, dlogits_channels] (dlogits_stride {b, y, x}, channel axis contiguous), 16-byte aligned, strides
 *              multiples of 8 elements, or NULL: rounded once to bf16, NOT divided by the number of valid pixels; a zero row for an ignored
 *              pixel AND for a pixel with ||f|| = 0 (every cosine is 0 there, the loss of a counted pixel is ln N and its exact gradient
 *              is 0 because f = 0; s * 1e12 * (softmax - onehot) is never stored).  EVERY one of the dlogits_channels channels is written
 *              (zeros from N up), so the buffer needs no clearing.  dlogits_channels: a multiple of 8, >= N rounded up to 16, <= 256.  Needs target
 *   dscale     device float [B, Ho, Wo] (dscale_stride), or NULL: 0 for an ignored pixel.  Needs target
 *   logit_scale_ptr   NULL, or one fp32 device value that is used in place of cos.logit_scale (read once by every workgroup, after
 *              its attention): a learnable temperature costs no host synchronisation per step.  cos.logit_scale must still be finite
 * No atomics, nothing crosses a workgroup: every output is deterministic, bit for bit.  A power-of-two factor on the values changes no
 * bit of loss or labels.
 * Served: what naf_xna_cos_fwd serves (profiles/cosine_objective.txt holds the compiler's figures of every instantiation).
 * naf_xna_cos_ce_select answers as naf_xna_cos_select does and additionally refuses: no output requested; loss / dlogits / dscale without
 * target; a bad dlogits_channels or a dlogits x stride below it; a loss / dscale that is not 4-byte aligned; non-zero reserved fields
 * (all -NAF_ERR_INVALID); a dlogits that is not 16-byte aligned or whose strides are not multiples of 8 elements (-NAF_ERR_UNSUPPORTED).
 * The differences from torch.nn.functional.cross_entropy are those listed for naf_xna_head_ce_args.  The struct must be
 * zero-initialised.  Caller-owned memory and stream; capturable; no workspace. */
typedef struct naf_xna_cos_ce_args {
    naf_xna_cos_args cos; /* cos.out may be NULL */
    const int64_t* target;
    float* loss;
    uint8_t* labels;
    void* dlogits;
    float* dscale;
    const float* logit_scale_ptr;
    int64_t ignore_index;
    int32_t dlogits_channels;
    int32_t reserved; /* must be 0 */
    int64_t t_stride[3];
    int64_t loss_stride[3];
    int64_t labels_stride[3];
    int64_t dlogits_stride[3];
    int64_t dscale_stride[3];
} naf_xna_cos_ce_args;
int naf_xna_cos_ce_select(const naf_xna_cos_ce_args* a);
int naf_xna_cos_ce_fwd(const naf_xna_cos_ce_args* a, naf_stream_t stream);

/* ---- mask pooling: the attention summed under K masks (added after the cosine entries; detect by symbol) ------------
 * Masked average pooling of the upsampled features -- region embeddings for mask proposals, prototypes for few-shot segmentation --
 * is linear in the values, and the attention's weights depend on the guidance only:
 *     pooled[b, k, c] = sum_px M[b, k, px] * sum_j P_g(c)[px, j] * V[b, c, j] = sum_j A[b, g(c), k, j] * V[b, c, j]
 *     A[b, g, k, j]   = sum_px M[b, k, px] * P_g[px, j]
 * naf_xna_maskpool_fwd computes A on the low-res grid and mass[b, k] = sum_px M[b, k, px] without reading V; naf_maskpool_apply is the
 * small contraction that follows.  The [B, C, Ho, Wo] tensor is never written.
 *   q, k_lr   exactly as in naf_xna_head_args (bf16, strides {b, head, y, x}, last dim contiguous, Dq = 64), rope_tab_* as there
 *   masks     device [B, K, Ho, Wo] of mask_dtype: NAF_MASK_BF16 (soft masks) or NAF_MASK_U8 (bytes: bool / uint8, read as their
 *             integer value); element strides m_stride = {b, k, y, x} with x stride 1.  Cells a multiple of 8 pixels wide are read
 *             with vector loads: the pointer must be 16-byte aligned and the b, k and y strides multiples of 8 elements
 *             (-NAF_ERR_UNSUPPORTED otherwise: the caller copies); other cells (14, 15, 30 ... pixels) are read element by element
 *   A         device float [B, heads, K, h, w] dense
 *   mass      device float [B, K] dense
 *   workspace device, naf_xna_maskpool_workspace_bytes(a) bytes, 16-byte aligned: per-cell partials
 *             [B][h*w][heads][NSLOT][Kpad] fp32 (NSLOT = ky*kx, Kpad = K rounded up to 16) and per-cell masses [B][h*w][Kpad]
 * Kernels (xna_pool_kernel.h): one workgroup per (batch, low-res cell) loops over the heads; scores and softmax are
 * naf_xna_head_fwd's instruction for instruction, so the bf16 P is bit for bit that kernel's; P goes through LDS transposed and
 * A_cell[slot, k] = sum_px P[px, slot] * M[k, px] runs on the matrix cores with the mask rows as operand fragments straight from
 * memory.  A gather kernel then sums, for every key j, the partials of the cells whose clamped window holds j in ascending cell
 * order.  No float atomics anywhere: two launches on the same inputs give the same bits.
 * Served: what naf_xna_head_fwd serves (square odd window 3 .. 15, Dq = 64, integer ratio whose cell rows are row tiles, h, w >= window),
 * 1 <= K <= 64 per launch (the caller chunks).  naf_xna_maskpool_select answers as naf_xna_head_select does: NAF_XNA_HEAD_FUSED,
 * -NAF_ERR_INVALID for arguments no kernel could serve, -NAF_ERR_UNSUPPORTED (with naf_last_error) for a valid request outside the list.
 * A pure host-side query.  Caller-owned memory and stream; capturable.  The struct must be zero-initialised (reserved fields). */
enum naf_mask_dtype {
    NAF_MASK_BF16 = 0,
    NAF_MASK_U8 = 1
};
typedef struct naf_xna_maskpool_args {
    const void* q;
    const void* k_lr;
    const void* masks;
    float* A;
    float* mass;
    void* workspace;
    size_t workspace_bytes;
    const float* rope_tab_y;
    const float* rope_tab_x;
    int32_t B, heads, Ho, Wo, h, w, Dq, K, ky, kx;
    int32_t mask_dtype; /* naf_mask_dtype */
    int32_t path;       /* naf_xna_head_path */
    float scale;
    int32_t reserved;
    int64_t q_stride[4];
    int64_t k_stride[4];
    int64_t m_stride[4];
} naf_xna_maskpool_args;
int naf_xna_maskpool_select(const naf_xna_maskpool_args* a);
size_t naf_xna_maskpool_workspace_bytes(const naf_xna_maskpool_args* a);
int naf_xna_maskpool_fwd(const naf_xna_maskpool_args* a, naf_stream_t stream);

/* pooled[b, k, c] = sum_j A[b, c / (C / heads), k, j] * v[b, c, j]  (fp32 products and sums, one wave per output in a fixed order),
 * divided by mass[b, k] when `mean` is non-zero; a mask of zero mass gives a row of exact zeros.
 *   A      device float [B, heads, K, h*w] dense (naf_xna_maskpool_fwd's)
 *   v      device bf16 [B, C, h*w], element strides v_stride = {b, c} with the grid contiguous (a dense [B, C, h, w] feature map)
 *   mass   device float [B, K] dense (read only when mean != 0; may be NULL otherwise)
 *   pooled device float [B, K, C] dense */
int naf_maskpool_apply(const float* A, const void* v, const float* mass, float* pooled, int32_t B, int32_t heads, int32_t K, int32_t C,
                       int32_t hw, const int64_t* v_stride, int32_t mean, naf_stream_t stream);

/* ---- peak search on the scaled cosines (added after the mask-pooling entries; detect by symbol) ------------
 * "Where is the best match": with cos the [B, N, Ho, Wo] result of naf_xna_cos_fwd, an integer ratio dy = Ho / h, dx = Wo / w, and cell
 * (cy, cx) the pixel block [cy*dy, (cy+1)*dy) x [cx*dx, (cx+1)*dx),
 *     peak[b, cy, cx, n]  = max of cos[b, n] over the cell              (fp32: the bits of an element of cos)
 *     where[b, cy, cx, n] = the lowest flat index y * Wo + x (output coordinates) among the cell's pixels that attain it   (int32)
 * from the epilogue of the cosine kernel: the N-channel map need not exist.  A pixel whose feature is zero has cosine exactly 0 and takes
 * part like any other.  Non-finite inputs are out of contract.
 *   cos           naf_xna_cos_args as for naf_xna_cos_fwd, except that `out` may be NULL; when given it receives the scaled cosines, bit for
 *                 bit what naf_xna_cos_fwd stores; norms as there
 *   peak          device float [B, h, w, N], element strides peak_stride {b, cy, cx}, channel axis contiguous
 *   where         device int32 [B, h, w, N], element strides where_stride {b, cy, cx}, channel axis contiguous
 * No atomics, nothing crosses a workgroup: every output is deterministic, bit for bit.  The comparator on (value, flat index) -- greater
 * value, or equal value and lower index -- is a total order, so the result does not depend on the order of the reduction.
 * Served: what naf_xna_cos_fwd serves (profiles/cosine_peaks.txt holds the compiler's figures of every instantiation), Ho * Wo < 2^31.
 * naf_xna_cos_peaks_select answers as naf_xna_cos_select does and additionally refuses: a NULL peak / where, an x stride below N, a
 * pointer that is not 4-byte aligned, Ho * Wo >= 2^31, non-zero reserved fields (all -NAF_ERR_INVALID).  The struct must be
 * zero-initialised.  Caller-owned memory and stream; capturable; no workspace. */
typedef struct naf_xna_cos_peaks_args {
    naf_xna_cos_args cos; /* cos.out may be NULL */
    float* peak;
    int32_t* where;
    int64_t peak_stride[3];
    int64_t where_stride[3];
    int64_t reserved[2]; /* must be 0 */
} naf_xna_cos_peaks_args;
int naf_xna_cos_peaks_select(const naf_xna_cos_peaks_args* a);
int naf_xna_cos_peaks_fwd(const naf_xna_cos_peaks_args* a, naf_stream_t stream);

/* The k best cells of every (b, n): the n_cells candidates (peak, where) ordered by value descending, then by flat index ascending; the
 * first k are returned.  One candidate per low-res cell -- a non-maximum suppression at the cell grid, not the k best pixels; k = 1 is
 * the global maximum of cos[b, n] with the lowest flat index among ties.  One wave per (b, n), k selection passes in a fixed order.
 *   peak / where  device float / int32 [B, n_cells, N] by the element strides peak_stride / where_stride {b, cell}, channel axis
 *                 contiguous (naf_xna_cos_peaks_fwd's outputs with a cell stride: x stride, and y stride = w * x stride)
 *   values / index   device float / int32 [B, N, k] dense
 * 1 <= k <= min(n_cells, 64); indices must be non-negative (Ho * Wo < 2^31).  No workspace; capturable. */
int naf_peaks_topk(const float* peak, const int32_t* where, float* values, int32_t* index, int32_t B, int32_t N, int32_t n_cells, int32_t k,
                   const int64_t peak_stride[2], const int64_t where_stride[2], naf_stream_t stream);

/* ---- k-means step: assign and accumulate in one launch (added after the peak-search entries; detect by symbol) ------------
 * One Lloyd iteration over the upsampled features f(px) without writing them.  Both halves are entries above:
 *     label(px)     = argmin_k |f(px) - c_k|^2 = argmax_k (c_k . f(px) - |c_k|^2 / 2)      a linear head with a bias and an argmax
 *     A[b, g, k, j] = sum_px [label(px) = k] * P_g[px, j],   mass[b, k] = #{px: label(px) = k}   mask pooling under one-hot masks
 * followed by naf_maskpool_apply(A, v_lr, ..., mean = 0) / mass on the low-res grid.  naf_xna_kmeans_fwd runs both in one cell kernel:
 * per round of 256 pixels it runs naf_xna_head_ce_fwd's head loop and argmax, keeps the 256 labels in LDS, and runs
 * naf_xna_maskpool_fwd's head loop with the mask operand built in registers from those labels.  No label map, no one-hot tensor.
 *   q, k_lr   exactly as in naf_xna_head_args (bf16, strides {b, head, y, x}, last dim contiguous, Dq = 64), rope_tab_* as there
 *   pv_lr     device bf16 [B, heads, h, w, Kpad] (Kpad = K rounded up to 16), as naf_xna_head_args.pv_lr: the centroids projected on the
 *             low-res features, PV_g[j, k] = c_k[g] . V_g[j]; channels K .. Kpad-1 are read and must be finite
 *   bias      device float [B, K]: row b starts bias_stride_b elements after row b-1 (0: one row for all images); or NULL
 *   labels    device uint8 [B, Ho, Wo] (labels_stride {b, y, x}), or NULL: the label map is an optional output
 *   A, mass   device float [B, heads, K, h, w] and [B, K], dense, as naf_xna_maskpool_args
 *   workspace device, naf_xna_kmeans_workspace_bytes(a) bytes, 16-byte aligned (naf_xna_maskpool_fwd's per-cell partials)
 * Two bit-identities define the entry (tests/test_gpu_kmeans.py):
 *   (1) labels are, bit for bit, what naf_xna_head_ce_fwd stores for image b with (pv_lr[b], bias[b]): the lowest index among equal maxima;
 *   (2) A and mass are, bit for bit, what naf_xna_maskpool_fwd returns for the NAF_MASK_U8 masks [label == k]; mass is an exact count.
 * A pixel counts in at most one cluster.  No float atomics anywhere: two launches on the same inputs give the same bits.
 * Served: exactly what naf_xna_maskpool_fwd serves, 1 <= K <= 64, pv_lr laid out as naf_xna_head_fwd asks.  naf_xna_kmeans_select answers
 * as naf_xna_head_select does: NAF_XNA_HEAD_FUSED, -NAF_ERR_INVALID for arguments no kernel could serve, -NAF_ERR_UNSUPPORTED (with
 * naf_last_error) for a valid request outside the list -- the caller then composes the two entries above.  A pure host-side query.
 * Caller-owned memory and stream; capturable.  The struct must be zero-initialised (reserved fields). */
typedef struct naf_xna_kmeans_args {
    const void* q;
    const void* k_lr;
    const void* pv_lr;
    const float* bias;
    uint8_t* labels;
    float* A;
    float* mass;
    void* workspace;
    size_t workspace_bytes;
    const float* rope_tab_y;
    const float* rope_tab_x;
    int32_t B, heads, Ho, Wo, h, w, Dq, K, ky, kx;
    int32_t path; /* naf_xna_head_path */
    float scale;
    int64_t bias_stride_b;
    int64_t q_stride[4];
    int64_t k_stride[4];
    int64_t pv_stride[4];
    int64_t labels_stride[3];
    int64_t reserved[2]; /* must be 0 */
} naf_xna_kmeans_args;
int naf_xna_kmeans_select(const naf_xna_kmeans_args* a);
size_t naf_xna_kmeans_workspace_bytes(const naf_xna_kmeans_args* a);
int naf_xna_kmeans_fwd(const naf_xna_kmeans_args* a, naf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NAF_HIP_H */
