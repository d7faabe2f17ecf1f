/*
 * dynamask_hip.h -- C ABI of libdynamask_hip.so, the MI355X (gfx950) operator
 * library behind the DynaMask mask-head hot path.
 *
 * Contract:
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer to fp32
 *     (or int32 / int64 where stated), NCHW-contiguous, owned by the caller;
 *   - no allocation; no state that a caller can observe or has to manage; work is
 *     enqueued on `stream` (a hipStream_t passed as void*; NULL = the null
 *     stream) on the CURRENT device and the call returns without synchronising.
 *     What the library does keep, per device and only as a cache: the device's
 *     compute-unit count and "this kernel's dynamic-LDS limit has been raised"
 *     flags (hipFuncSetAttribute once per device).  A few knobs are read from
 *     the environment on first use, eight in all, none of which changes what is
 *     computed but DM_GN_WIDE, which changes a rounding: DM_CONV_TAIL / DM_DCN_TAIL (0: no separate launch for the last,
 *     underfull round of workgroups), DM_CONV1_SMALL_WGS (up to how many 128 x 128
 *     tiles a 1x1 launch takes 128 x 32 tiles instead; default 1.25 per CU, 0: never),
 *     DM_WGRAD_WGS (split-K workgroups of the
 *     weight gradients), DM_ROI_SORT / DM_ROI_SORT_MIN (the RoI ordering launch of
 *     dm_roi_align_fwd_ws; re-read by dm_reload_env_knobs()), DM_GN_WIDE (0: the
 *     narrow build of dm_group_norm_fwd for every group length; re-read by
 *     dm_reload_env_knobs() too), DM_CONV_SPLITK is the
 *     host binding's.  (Rounds 2-4 had twenty more -- first-generation kernels and
 *     rejected variants kept for A/B timing; their measurements are in
 *     docs/HISTORY.md and profiles/, the kernels are gone.)
 *     Calls from several host threads are safe (a race only repeats an
 *     idempotent attribute call);
 *   - LDS scatter-accumulators (dm_deform_col2im_coord, the scatter form of
 *     dm_point_sample_bwd) are 64-bit fixed point: integer sums are associative,
 *     so a plane's result does not depend on the order of arrival.  Resolution,
 *     range and poison rules: "Fixed-point accumulators" below (one contract for
 *     these and for the *_fx entry points);
 *   - return value: 0 = enqueued, negative = error (DM_ERR_*); the host binding
 *     raises on any non-zero code (dm_error_string()).
 *
 * Each entry point cites the reference interface it replaces (paths relative to
 * the reference tree, lslrh/DynaMask).
 */
#ifndef DYNAMASK_HIP_H
#define DYNAMASK_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DM_OK 0
#define DM_ERR_INVALID_ARG (-1)   /* bad shape / null pointer / unsupported parameter */
#define DM_ERR_LAUNCH (-2)        /* hipLaunch / hipGetLastError reported a failure   */
#define DM_ERR_UNSUPPORTED (-3)   /* valid request the library has no kernel for      */

#define DM_MAX_LEVELS 4
#define DM_MAX_SOURCES 4

typedef void* dm_stream_t; /* hipStream_t */

const char* dm_error_string(int code);
/* ABI version: bumped whenever a signature or the meaning of an argument changes (8: flag bit 3 of dm_conv2d_fwd; 9: RoI assignment / bbox training entry points; 10: dm_detail_target takes the fuse weights from device memory; 11: FCNMaskHead upsample backward; 12: dm_fc_fwd takes a scratch slab, deterministic split-K; 13: dm_deform_coord_grad / dm_deform_col2im, dm_conv2d_fwd_masked, dm_scale, dm_polygon_mask_targets, dm_ignore_columns, dm_upsample2x_bilinear_bwd overwrites; 14: dm_random_sample, dm_bn_relu_maxpool_argmax, the *_fx deterministic accumulators + dm_fx_to_float, dm_mask_loss_fwd_bwd takes a scratch, dm_conv2d_wgrad takes the bias gradient, dm_conv_pack_weight_batch, dm_mask_loss_stage; 15: dm_class_logits_up2x_fwd; 16: dm_conv2d_wgrad_slab / dm_conv2d_wgrad_scratch_floats; 17: dm_class_logits_bwd_slab / dm_class_logits_bwd_scratch_floats; 18: dm_reload_env_knobs, dm_roi_align_fwd_ws / dm_roi_align_workspace_bytes, dm_conv_pack_weight_split / dm_conv_packed_floats_split and flag bits 4, 5 of dm_conv2d_fwd; 19: dm_dcn_bwd_data_fused and its pack; 20: dm_conv2d_fwd_ws / dm_conv2d_splitk_floats; 21: dm_deform_conv_fwd_ws / dm_deform_conv_splitk_floats; 22: the bf16-split layouts (dm_conv_pack_weight_split, dm_conv_packed_floats_split, flag bits 4 / 5 of dm_conv2d_fwd) and the one-kernel DCN data gradient (dm_dcn_bwd_*) REMOVED -- measured, never the parity path, see docs/HISTORY.md; 23: dm_bn_stats takes mean_shift, dm_roi_align_bwd takes the gather form for 16 < P <= 64; 24: dm_build_info; 25: dm_boundary_merge_chain, dm_stage_head_fwd; 26: dm_conv1x1_group_fwd; 27: dm_deform_conv_tout_fwd / dm_deform_conv_tout_supported; 28: the opt-in bf16x3 mode -- dm_conv_pack_weight_bf16x3 / dm_conv_packed_floats_bf16x3 and flag bit 4 of dm_conv2d_fwd, dm_conv2d_fwd_ws and dm_conv1x1_group_fwd; dm_deconv_pack_weight_bf16x3 and flag bit 4 of dm_deconv2x2_fwd; 29: dm_roi_align_workspace_bytes answers 0 wherever no call with these N, P orders its RoIs, dm_roi_align_plan).  Entry points ADDED without a signature or meaning change leave the number as it is (the loader resolves every symbol of _lib.SIGNATURES by name, so an older library fails at load; that table is derived from this file, dynamask_amd/_abi.py): the multi-image post-processing dm_nms_mask_segmented / dm_nms_reduce_segmented, dm_paste_masks_multi, dm_paste_rle_multi / dm_rle_multi_scratch_ints; the test-time augmentation dm_bbox_mapping_multi, dm_merge_aug_bboxes, dm_merge_aug_masks; RefineMask's dilated / any-width 3x3 convolutions and the sigmoid of its semantic map (section K21); PointRend's point
 * selection, point gather, point MLP and scatter (section K22); Mask Scoring R-CNN's stride-2 3x3 convolution, IoU-head
 * input and mask scores (section K23); PointRefine's descending point selection, point-feature gather, point MLP and
 * multi-row scatter (section K24); Cascade Mask R-CNN's stage-grouped convolutions / deconvolutions and stage step
 * (section K25); Hybrid Task Cascade's resize, post-activation addend and RoIAlign-add (section K26); Grid R-CNN's
 * GroupNorm, neighbour fusion, grouped 4x4 stride-2 deconvolution and box vote (section K27); the convolution launcher's
 * own report of its launches, dm_conv2d_plan (section K5/K6) and dm_conv2d_group_plan (section K25); Double-Head R-CNN's
 * rescaled RoIAlign and global average pool (section K28); the DCN forward launcher's route, dm_deform_conv_plan
 * (section K8); the weight-gradient launcher's route, dm_conv2d_wgrad_plan, and that of
 * the other training-side launchers, dm_bwd_plan and dm_mask_pre_plan; RPN inference's selection, decode and merge
 * (section K30); the FPN neck's gathered addend and stride-2 subsample (section K31); ResNeXt's grouped
 * 3x3 convolution (section K34); Res2Net's sliced 3x3 convolution, 2x2 ceil-mode average pool and deep-stem convolution
 * (section K35). */
#define DM_ABI_VERSION 29 /* the one definition: dm_abi_version(), dm_build_info() and _lib.ABI_VERSION read it */
int dm_abi_version(void);
/* "libdynamask_hip abi=N arch=gfx950 compiler=<clang version> flags=<the product-wide flags of dynamask_amd/build.py>"
 * (static storage).  The library must be compiled WITHOUT packed fp32 instructions (flag "-packed-fp32-ops", see
 * build.py); the host binding checks this string at load time and refuses a library that does not say so.  A build
 * recipe other than build.py passes its flag set as -DDM_BUILD_FLAGS="..."; without it the string says flags=unknown. */
const char* dm_build_info(void);
/* Re-read the DM_ROI_* experiment knobs and DM_GN_WIDE from the environment (they are otherwise read once, at the first
 * launch, and clamped to validated ranges).  For measurement tools that sweep settings inside one process; no DM_ROI_* knob
 * changes a result, DM_GN_WIDE chooses between two builds that differ in rounding (section K27). */
int dm_reload_env_knobs(void);

/* ---------------------------------------------------------------------------
 * K1/K2  multi-level RoIAlign forward (avg pooling, aligned=True, adaptive grid)
 * replaces: SingleRoIExtractor.forward + map_roi_levels
 *           (mmdet/models/roi_heads/roi_extractors/single_level_roi_extractor.py:32-81)
 *           and the per-level mmcv.ops.RoIAlign it builds
 *           (roi_extractors/base_roi_extractor.py:49-55).
 * feats[l]   : [B, C, H[l], W[l]]   l < num_levels (1..4); feats, H, W and
 *              spatial_scales are HOST arrays (feats holds device pointers)
 * rois       : [N, 5] = (batch_idx, x1, y1, x2, y2) in image pixels
 * out        : [N, C, P, P]
 * levels_out : optional [N] int32, the FPN level chosen per RoI (NULL to skip)
 * level = clamp(floor(log2(sqrt(w*h)/finest_scale + 1e-6)), 0, num_levels-1);
 * num_levels == 1 skips the mapping (single-level extractor, base_roi_head.py:53-57).
 * ------------------------------------------------------------------------- */
int dm_roi_align_fwd(const float* const* feats, const int* H, const int* W, const float* spatial_scales,
                     int num_levels, int B, int C, const float* rois, int N, int P, int sampling_ratio,
                     float finest_scale, float* out, int32_t* levels_out, dm_stream_t stream);

/* The same extraction with a caller-provided workspace of dm_roi_align_workspace_bytes(N, P) bytes (device memory,
 * 16-byte aligned, contents irrelevant before and after the call).  0 bytes = no call with these N, P orders its RoIs:
 * DM_ROI_SORT off, P * P < 128 or > 256, N below DM_ROI_SORT_MIN or above 1024 (ABI 29; before, 0 only for N <= 0, P < 2
 * or P * P > 256 -- the one deliberate narrowing of an answer: a caller allocates exactly where it pays).  It stays an
 * upper bound on what the call uses; a call that would order may still not (C % 4 != 0, a map above 2^23 pixels).  For the
 * 14x14 extraction of 192 .. 1024 RoIs a first kernel ranks the RoIs by (image, level, 32-pixel row, column) into the
 * workspace and the extraction walks them in that order -- workgroups that run side by side then share their footprints
 * in the XCD's L2 (fabric traffic 261 -> 193 MB per 512 RoIs, 57 -> 50.7 us with the ranking kernel) -- and writes every
 * RoI's rows where dm_roi_align_fwd writes them: the same bits (knob DM_ROI_SORT, default 1).
 * A null / too small workspace falls back to dm_roi_align_fwd's kernels. */
long long dm_roi_align_workspace_bytes(int N, int P);
int dm_roi_align_fwd_ws(const float* const* feats, const int* H, const int* W, const float* spatial_scales,
                        int num_levels, int B, int C, const float* rois, int N, int P, int sampling_ratio,
                        float finest_scale, float* out, int32_t* levels_out, void* workspace,
                        long long workspace_bytes, dm_stream_t stream);

/* K3  RoIAlign backward: scatter-add (float atomics) of grad_out into the
 * per-level feature gradients, which the caller has zero-filled. */
int dm_roi_align_bwd(const float* grad_out, float* const* grad_feats, const int* H, const int* W,
                     const float* spatial_scales, int num_levels, int B, int C, const float* rois, int N,
                     int P, int sampling_ratio, float finest_scale, dm_stream_t stream);

/* (ABI 29) The launches dm_roi_align_fwd / dm_roi_align_scaled_fwd / dm_roi_align_fwd_ws (entry 0), dm_roi_align_add_fwd
 * (entry 1, with its `pool`; H and W then point at its one map's sizes, num_levels = 1) or dm_roi_align_bwd (entry 2) would
 * make for these HOST arguments: the route the launcher decides on, the very value it then enqueues.  Nothing is launched
 * and no device is needed: unlike the DCN route, nothing in this one reads the compute-unit count.  Arguments as the
 * entry's, without the device pointers, the scales and roi_scale_factor (none enters the route).  workspace: 0 = none
 * (NULL), 1 = a 16-byte aligned pointer, 2 = a misaligned one, with workspace_bytes behind it; entries 1 and 2 take none
 * (DM_ERR_INVALID_ARG otherwise); `pool` is read for entry 1 only.  The DM_ROI_SORT / DM_ROI_SORT_MIN knobs apply as they do
 * to launches (dm_reload_env_knobs re-reads them).
 * records: HOST array of max_records (>= DM_ROI_PLAN_MAX_LAUNCHES) x DM_ROI_PLAN_INTS ints.  Returns the number of launches
 * (0: N = 0; 1; 2: the order kernel + the tile kernel that walks its records, or roi_align_kernel<false, 1> + <false, 2>) or
 * the error code the call would return for these numbers, and then writes nothing.  Record l, ints [l * DM_ROI_PLAN_INTS ..):
 *   0 kernel: 0 roi_order_kernel, 1 roi_align_tile_kernel, 2 roi_align_band_kernel, 3 roi_align_kernel,
 *     4 roi_align_bwd_gather_kernel;
 *   (entry 3, dm_roi_align_strided_fwd with its bin_step in `pool`: section K29; kernel 1 with parameters 3, bin_step)
 *   1, 2 its template parameters: MODE, 0 (kernel 1: 0 stores, 1 adds, 2 adds the 2 x 2 block means); TB, WPC (kernel 2);
 *     BWD, GCLS (kernel 3); zeros (kernels 0, 4);
 *   3 grid x (RoIs x channel chunks; kernel 0: ceil(N / 16));  4 threads per workgroup;  5 dynamic LDS bytes;
 *   6 CT: channels per workgroup (0: kernel 0);  7 order: 1 = the XCD-aware workgroup order (kernel 1 with a multiple of 8
 *     chunks);  8 lds_floats: LDS budget of roi_align_kernel's planar tile (0: every other launch);
 *   9 levels: 1 when this launch is the one that writes levels_out (an ordered call: the order kernel, not the tile kernel). */
#define DM_ROI_PLAN_INTS 10
#define DM_ROI_PLAN_MAX_LAUNCHES 2
int dm_roi_align_plan(int entry, int pool, int num_levels, const int* H, const int* W, int B, int C, int N, int P,
                      int sampling_ratio, long long workspace_bytes, int workspace, int* records, int max_records);

/* ---------------------------------------------------------------------------
 * Weight packing for the implicit-GEMM convolutions: OIHW [Cout, Cin, k, k] ->
 * [k*k][KQ][CoutP][4]: input channels in quads, CoutP = dm_conv_packed_cout(Cout)
 * (zero padded).  The input channels are the concatenation of `num_srcs`
 * sources (src_channels[], HOST array, sum = Cin); each source is padded with
 * zero rows to a multiple of 8 channels, KQ = sum(roundup(Cs, 8)) / 4, total
 * size dm_conv_packed_floats() floats.
 * transpose_flip != 0 packs the weights of the data-gradient convolution
 * (in/out channels swapped, taps rotated by 180 degrees): input is still the
 * forward OIHW tensor, the packed tensor then has "Cout" = Cin of the forward
 * and src_channels must sum to the forward's Cout.
 * ------------------------------------------------------------------------- */
int dm_conv_packed_cout(int Cout);
long long dm_conv_packed_floats(int Cout, int ksize, int num_srcs, const int* src_channels);
int dm_conv_pack_weight(const float* w_oihw, int Cout, int Cin, int ksize, int transpose_flip,
                        int num_srcs, const int* src_channels, float* w_packed, dm_stream_t stream);

/* All the packs of a training step in one launch (the weights change with every optimizer step).  A job is
 * dm_conv_pack_weight's arguments plus a window: the packed [Cout][Cin] tensor may be the input-channel slice
 * [c0, c0 + Cin) of a [Cout][ld][k][k] tensor (the data gradient towards one concat source); ld = Cin, c0 = 0 for
 * a whole tensor.  `jobs_device`: num_jobs structs in DEVICE memory (the caller uploads the table once and reuses
 * it while the tensors stay where they are). */
typedef struct dm_pack_job {
  const float* w;
  float* w_packed;
  int Cout, Cin, ksize, transpose_flip;
  int num_srcs, src_channels[DM_MAX_SOURCES];
  int ld, c0;
} dm_pack_job;
int dm_conv_pack_weight_batch(const dm_pack_job* jobs_device, int num_jobs, dm_stream_t stream);

/* (ABI 28) The bf16x3 layout of the same weights, for the opt-in split mode of the forward convolutions (flag bit 4 of
 * dm_conv2d_fwd / dm_conv2d_fwd_ws / dm_conv1x1_group_fwd).  Every weight w is stored as three bf16 numbers rounded to
 * nearest, hi = bf16(w), mid = bf16(w - hi), lo = bf16(w - hi - mid) (mid = lo = 0 when hi is not finite):
 * [k*k][KQ][CoutP][16 bytes], each source padded with zero rows to a multiple of 16 channels, KQ = sum(roundup(Cs, 16))
 * / 16 * 6 words, dm_conv_packed_floats_bf16x3() floats.  Arguments as dm_conv_pack_weight's. */
long long dm_conv_packed_floats_bf16x3(int Cout, int ksize, int num_srcs, const int* src_channels);
int dm_conv_pack_weight_bf16x3(const float* w_oihw, int Cout, int Cin, int ksize, int transpose_flip,
                               int num_srcs, const int* src_channels, float* w_packed, dm_stream_t stream);

/* ---------------------------------------------------------------------------
 * K5/K6  dense convolution forward, stride 1, "same" padding, ksize in {1,3},
 * fp32 in / fp32 accumulate on the MFMA units, fused concat + bias + ReLU.
 * replaces: mmcv ConvModule / nn.Conv2d calls of
 *           mask_heads/dynamask_head.py:73,83,86,104,117-121,203-213,221-222,
 *           mask_heads/fcn_mask_head.py:59-71,119-120,102,125.
 * srcs[s]  : [NB, src_channels[s], H, W]; the channel-concatenation of the
 *            sources is the conv input (torch.cat at dynamask_head.py:107-116
 *            is folded into the K loop), sum(src_channels) = Cin.
 *            src_batch_strides[s] (floats; NULL = dense) lets a source be a
 *            channel slice of a wider tensor.  srcs / src_channels /
 *            src_batch_strides are HOST arrays (of device pointers / ints).
 * w_packed : dm_conv_pack_weight layout, bias: [Cout] or NULL
 * relu     : flags -- bit 0: fused ReLU; bit 1: accumulate (out += result; used
 *            for gradient sums in the backward); bit 3: the caller overlaps this
 *            launch with work on another stream (a scheduling hint: the 3x3
 *            kernel then does not split off its last round of workgroups;
 *            results are the same bits either way); bit 4 (ABI 28): w_packed is
 *            the dm_conv_pack_weight_bf16x3 layout and the products run as six
 *            bf16 MFMA cross products of the split operands, fp32 accumulation
 *            (error at fp32 level, not the exact fp32 chain; the same bits every
 *            run); 3x3 launches whose staged plane exceeds 256 positions (maps
 *            wider than ~16 pixels) return DM_ERR_UNSUPPORTED under it;
 *            any other bit (bit 2 included: it is the launcher's own
 *            store-policy bit, never the caller's): DM_ERR_INVALID_ARG
 * 3x3 maps : every exact build stages the input plane of a pixel tile in LDS, at
 *            most 1024 positions: maps wider than 168 pixels return
 *            DM_ERR_UNSUPPORTED whatever Cout and NB.  A 1 x 1 map overflows the
 *            plane of the 128-pixel tiles (128 images of 3 x 3 padded positions):
 *            Cout <= 64 returns DM_ERR_UNSUPPORTED; Cout > 64 runs the 128-cout x
 *            32-pixel build for every NB (the answer does not depend on NB).
 * out      : written at channels [out_ch_offset, out_ch_offset+Cout) of a
 *            tensor [NB, out_ch_total, H, W]
 * ------------------------------------------------------------------------- */
int dm_conv2d_fwd(const float* const* srcs, const int* src_channels, const long long* src_batch_strides,
                  int num_srcs, int NB, int H, int W,
                  const float* w_packed, const float* bias, int Cout, int ksize, int relu, float* out,
                  int out_ch_total, int out_ch_offset, dm_stream_t stream);
/* (ABI 20) dm_conv2d_fwd with a caller-owned workspace, for the calls of real inference (the reference runs the head on at
 * most 100 RoIs, dynamask_roi_head.py:132-135): a launch that would leave most of the chip idle splits its K loop over up
 * to eight workgroups per tile; the splits store bare sums to the workspace ([split][NB][Cout][HW]) and a second kernel
 * adds them in split order and applies bias / accumulate / ReLU.  The same bits every run; they differ from dm_conv2d_fwd's
 * in rounding only (another association of the same products).  dm_conv2d_splitk_floats: the workspace with which this
 * shape splits as far as it wants to, 0 when it would not split (then call dm_conv2d_fwd). */
long long dm_conv2d_splitk_floats(int NB, int H, int W, int Cout, int ksize);
int dm_conv2d_fwd_ws(const float* const* srcs, const int* src_channels, const long long* src_batch_strides,
                     int num_srcs, int NB, int H, int W, const float* w_packed, const float* bias, int Cout, int ksize,
                     int relu, float* out, int out_ch_total, int out_ch_offset, float* workspace,
                     long long workspace_floats, dm_stream_t stream);

/* (added to ABI 28) The launches dm_conv2d_fwd / dm_conv2d_fwd_ws / dm_conv2d_fwd_masked / dm_conv2d_post_add_fwd would
 * make for these HOST arguments, reported by the launcher itself (the same code runs with a recorder instead of launching:
 * nothing is launched, no device is needed -- without one the compute-unit count is taken as 256).  Arguments as
 * dm_conv2d_fwd_ws's, without the pointers: workspace_floats = 0 for the entry points without a workspace; has_mask /
 * has_addend != 0: the _masked / _post_add call (neither takes a workspace: DM_ERR_INVALID_ARG with one).  The
 * DM_CONV_TAIL / DM_CONV1_SMALL_WGS knobs apply as they do to launches (read once per process).
 * records: HOST array of max_records (>= DM_CONV_PLAN_MAX_LAUNCHES) x DM_CONV_PLAN_INTS ints.  Returns the number of
 * launches (0: NB = 0; 1; 2: a 3x3 launch that sends its underfull last round of workgroups to a second launch) or the
 * error code the call would return, and then writes nothing.  Record l, ints [l * DM_CONV_PLAN_INTS ..):
 *   0 KS, 1 WGM, 2 WGN, 3 WM, 4 WN, 5 CK, 6 TAIL, 7 PREC, 8 POST: the build (a workgroup is WGM x WGN waves of WM x WN
 *     32 x 32 blocks: 32 WGM WM couts (+ TAIL) x 32 WGN WN pixels, CK-channel chunks; PREC 1 = bf16x3, POST 1 = addend);
 *   9 MAXPOS: staged plane positions per thread (3x3; 1 for 1x1);
 *   10 ksplit, 11 kchunks: K splits (1: none) and chunks per split (0 without a split);
 *   12 q_begin, 13 Q: the flat pixels [q_begin, Q) of the batch this launch covers;
 *   14 grid x (cout tiles x pixel tiles), 15 grid y (= ksplit);
 *   16: 1 when the output is written with nontemporal stores. */
#define DM_CONV_PLAN_INTS 17
#define DM_CONV_PLAN_MAX_LAUNCHES 2
int dm_conv2d_plan(const int* src_channels, const long long* src_batch_strides, int num_srcs, int NB, int H, int W, int Cout,
                   int ksize, int relu, int out_ch_total, int out_ch_offset, long long workspace_floats, int has_mask,
                   int has_addend, int* records, int max_records);

/* (ABI 26) Up to three independent single-source 1x1 convolutions (+ bias, + ReLU) as ONE launch -- the FPN-wide
 * semantic_transform_in convolutions of the three SFM stages (mmdet/models/roi_heads/mask_heads/dynamask_head.py:104,
 * relu(conv1x1(P4 / P3 / P2))), which no RoI enters and which otherwise head the inference chain as three launches.
 * x, Cin, H, W, w_packed, bias, Cout, out: HOST arrays of `count` entries (device pointers inside); w_packed[i] as
 * dm_conv_pack_weight(ksize 1, one source) lays it out; bias[i] may be NULL.  Same bits as dm_conv2d_fwd per problem.
 * relu: bit 0 ReLU; bit 4 (ABI 28): every w_packed[i] is the dm_conv_pack_weight_bf16x3 layout (the bf16x3 mode of
 * dm_conv2d_fwd, same bits as its launches); any other bit: DM_ERR_INVALID_ARG. */
int dm_conv1x1_group_fwd(int count, const float* const* x, const int* Cin, const int* H, const int* W, int NB,
                         const float* const* w_packed, const float* const* bias, const int* Cout, int relu, float* const* out,
                         dm_stream_t stream);

/* dm_conv2d_fwd whose epilogue also applies a ReLU adjoint: outputs where `mask` (same layout, channel count and
 * channel offset as `out`) is <= 0 are stored as 0 (autograd's threshold_backward: a NaN activation passes the gradient).  Used for data gradients: the mask is the activation the
 * gradient flows into, so the separate mask pass (read gradient + activation, write gradient) disappears.  Flag bit 4
 * (the bf16x3 mode) returns DM_ERR_UNSUPPORTED here, as it does on the DCN entry points: those stay exact fp32. */
int dm_conv2d_fwd_masked(const float* const* srcs, const int* src_channels, const long long* src_batch_strides,
                         int num_srcs, int NB, int H, int W, const float* w_packed, const float* bias, int Cout,
                         int ksize, int relu, float* out, int out_ch_total, int out_ch_offset, const float* mask,
                         dm_stream_t stream);

/* ---------------------------------------------------------------------------
 * K4  SimpleRoIAlign / point_sample forward (grid_sample bilinear, zero
 * padding, align_corners=False at RoI-relative pixel centres).
 * replaces: mmcv.ops.SimpleRoIAlign at mask_heads/dynamask_head.py:74,105.
 * feat [B, C, H, W], rois [N,5] -> out [N, C, S, S]
 * ------------------------------------------------------------------------- */
int dm_point_sample_fwd(const float* feat, int B, int C, int H, int W, const float* rois, int N, int S,
                        float spatial_scale, float* out, dm_stream_t stream);

/* ---------------------------------------------------------------------------
 * K7  per-RoI class-gathered 1x1 logits, two branches at once.
 * replaces: instance_logits(x)[arange(N), labels][:, None] and the detail twin
 *           (mask_heads/dynamask_head.py:110-113, 236-237).
 * x [N, C, HW]; w_inst/w_det [num_classes, C]; b_* [num_classes];
 * labels [N] int64 (values clamped to [0, num_classes-1] by the caller's contract)
 * inst/det      : [N, HW] raw logits
 * sig_out       : optional; sigmoid(inst), sigmoid(det) written to channels
 *                 sig_ch_offset, sig_ch_offset+1 of a [N, sig_ch_total, HW] tensor
 * ------------------------------------------------------------------------- */
int dm_class_logits_fwd(const float* x, int N, int C, int HW, const float* w_inst, const float* b_inst,
                        const float* w_det, const float* b_det, int num_classes, const int64_t* labels,
                        float* inst, float* det, float* sig_out, int sig_ch_total, int sig_ch_offset,
                        dm_stream_t stream);

/* (ABI 25) One SFM stage's head in one launch: dm_point_sample_fwd(sem, rois -> sampled [N,Cs,S,S]) and
 * dm_class_logits_fwd(x [N,C,S,S] -> inst, det (+ sigmoid slices of sig_out)) -- mmdet/models/roi_heads/mask_heads/
 * dynamask_head.py:104-116; the two share no data, the kernel runs the two bodies in disjoint workgroup ranges (same bits). */
int dm_stage_head_fwd(const float* sem, int B, int Cs, int H, int W, const float* rois, int N, int S, float spatial_scale,
                      float* sampled, const float* x, int C, const float* w_inst, const float* b_inst, const float* w_det,
                      const float* b_det, int num_classes, const int64_t* labels, float* inst, float* det, float* sig_out,
                      int sig_ch_total, int sig_ch_offset, dm_stream_t stream);

/* K7 on relu(upsample2x(x)) (bilinear, align_corners=False) without the upsampled tensor: the logits an exit needs when
 * the stage before it would only have been upsampled for them -- dynamask_head.py:120-122 (F.interpolate + relu) followed
 * by :110-113 of the next stage / :236-237.  x [N, C, H, W] (W even, H, W >= 2: else DM_ERR_UNSUPPORTED and the caller
 * runs the two kernels); inst/det [N, 2H, 2W].  The interpolated values are those of dm_upsample2x_bilinear_fwd bit for
 * bit, and the channel sum runs in the four interleaved subsets of dm_class_logits_fwd. */
int dm_class_logits_up2x_fwd(const float* x, int N, int C, int H, int W, const float* w_inst, const float* b_inst,
                             const float* w_det, const float* b_det, int num_classes, const int64_t* labels,
                             float* inst, float* det, dm_stream_t stream);

/* ---------------------------------------------------------------------------
 * K8  deformable convolution v1 forward, 3x3, stride 1, pad 1, dilation 1,
 * groups 1, no bias, fused ReLU option.
 * replaces: mmcv.ops.DeformConv2dPack (DCN) at mask_heads/dynamask_head.py:84,118-119;
 *           arithmetic spec mmdet/ops/dcn/src/deform_conv_cuda_kernel.cu:84-115,190-243,
 *           mmdet/ops/dcn/src/deform_conv_cuda.cpp:152-260.
 * x [NB, C, H, W]; offset [NB, deform_groups*18, H, W] (dh,dw interleaved per tap);
 * w_packed: dm_conv_pack_weight(ksize=3, one source) of the [Cout, C, 3, 3] weight; out [NB, Cout, H, W]
 * relu: bit 0 fused ReLU; bit 3 the same scheduling hint as in dm_conv2d_fwd
 * ------------------------------------------------------------------------- */
int dm_deform_conv_fwd(const float* x, const float* offset, int NB, int C, int H, int W,
                       const float* w_packed, int Cout, int deform_groups, int relu, float* out,
                       dm_stream_t stream);
/* (ABI 27) K8 + the 1x1 behind it in one launch: relu(DCN 3x3) -> 1x1 conv + bias + ReLU, i.e. SFMStage.fuse_conv[1]
 * followed by fuse_transform_out (mmdet/models/roi_heads/mask_heads/dynamask_head.py:117-121), for the 28 x 28 / 56 x 56
 * stages at more than a handful of RoIs (dm_deform_conv_tout_supported: 1 = this shape takes the kernel build in which a
 * wave holds every output channel of its pixels; the 1x1 then runs on the accumulators in registers).
 *   w2t  [Cout][M2P]  the 1x1 weight [M2, Cout] transposed, M2P = M2 rounded up to 32, zeros in the padding
 *   out2 [NB, out2_ch_total, H, W]: channels [0, M2) are written;   out_dcn: NULL (the DCN output is not stored) or
 *   [NB, Cout, H, W].  Returns DM_ERR_UNSUPPORTED for other shapes.  Bits: those of dm_deform_conv_fwd + dm_conv2d_fwd. */
int dm_deform_conv_tout_supported(int NB, int C, int H, int W, int Cout, int M2);
int dm_deform_conv_tout_fwd(const float* x, const float* offset, int NB, int C, int H, int W, const float* w_packed, int Cout,
                            int deform_groups, const float* w2t, const float* b2, int M2, float* out2, int out2_ch_total,
                            float* out_dcn, dm_stream_t stream);

/* (ABI 21) dm_deform_conv_fwd with a caller-owned workspace: a launch that leaves most of the chip idle (the <= 100-RoI
 * inference calls) splits its channel loop over up to eight workgroups per tile; a second kernel adds the splits in index
 * order (+ ReLU).  Same bits every run; they differ from dm_deform_conv_fwd's by the association of the channel sums.
 * dm_deform_conv_splitk_floats: an upper bound on the workspace a split of this shape uses, which dm_deform_conv_plan honours
 * (0: no launch of this shape splits; more than this changes nothing). */
long long dm_deform_conv_splitk_floats(int NB, int C, int H, int W, int Cout);
int dm_deform_conv_fwd_ws(const float* x, const float* offset, int NB, int C, int H, int W, const float* w_packed, int Cout,
                          int deform_groups, int relu, float* out, float* workspace, long long workspace_floats,
                          dm_stream_t stream);

/* (added to ABI 28) The launches dm_deform_conv_fwd / dm_deform_conv_fwd_ws / dm_deform_conv_tout_fwd would make for these
 * HOST arguments: the route the launcher decides on, the very value it then enqueues (nothing is launched, no device is
 * needed -- without one the compute-unit count is taken as 256).  Arguments as dm_deform_conv_fwd_ws's, without the
 * pointers: workspace_floats = 0 for the call without a workspace; M2 = 0: the plain DCN, M2 > 0: the dm_deform_conv_tout_fwd
 * call with that M2 (it has neither flags nor a workspace: `relu` is ignored, DM_ERR_INVALID_ARG with a workspace).  The
 * DM_DCN_TAIL knob applies as it does to launches (read once per process).
 * records: HOST array of max_records (>= DM_DCN_PLAN_MAX_LAUNCHES) x DM_DCN_PLAN_INTS ints.  Returns the number of launches
 * (0: NB = 0; 1; 2: a launch on a 14 x 14-sized map that sends its underfull last round of workgroups to a second launch) or
 * the error code the call would return, and then writes nothing.  Record l, ints [l * DM_DCN_PLAN_INTS ..):
 *   0 kernel: 0 deform_conv_kernel, 1 deform_conv_lds_kernel, 2 deform_conv_c256_kernel, 3 deform_conv_band_kernel;
 *   1 .. 4 its template parameters: WGM, WGN, WM, WN (kernel 0); WM, WGM, XR, 0 (kernel 3); zeros (kernels 1, 2);
 *   5 threads per workgroup;  6 MT: cout tiles (1 where a workgroup holds every cout: kernels 2 and 3);
 *   7 q_begin, 8 Q: the flat pixels [q_begin, Q) of the batch this launch covers;
 *   9 grid x (cout tiles x pixel tiles), 10 grid y (= ksplit);
 *   11 ksplit, 12 kchan: K splits (1: none) and channels per split (0 without a split);
 *   13 dynamic LDS bytes;  14: 1 when the split-K reduction follows this launch. */
#define DM_DCN_PLAN_INTS 15
#define DM_DCN_PLAN_MAX_LAUNCHES 2
int dm_deform_conv_plan(int NB, int C, int H, int W, int Cout, int deform_groups, int relu, long long workspace_floats, int M2,
                        int* records, int max_records);

/* ---------------------------------------------------------------------------
 * K11  x2 bilinear upsampling.
 * replaces: nn.Upsample(scale_factor=2, mode='bilinear') + ReLU
 *           (mask_heads/dynamask_head.py:87,123; align_corners=False) and
 *           F.interpolate(scale_factor=2, 'bilinear', align_corners=True)
 *           (mask_heads/dynamask_head.py:239-243).
 * in [NC, H, W] -> out [NC, 2H, 2W]
 * ------------------------------------------------------------------------- */
int dm_upsample2x_bilinear_fwd(const float* in, int NC, int H, int W, int align_corners, int relu,
                               float* out, dm_stream_t stream);

/* ---------------------------------------------------------------------------
 * K15  inference boundary-aware merge of one coarse->fine stage pair.
 * replaces: the loop body of DynaMaskRoIHead.simple_test_mask
 *           (roi_heads/dynamask_roi_head.py:138-149) incl. generate_block_target
 *           (losses/cross_entropy_loss.py:123-154) with boundary_width=1.
 * coarse [n, S, S] logits, fine [n, 2S, 2S] logits (overwritten in place where
 * the x2 align_corners=True upsampled non-boundary mask is >= 0.5).
 * ------------------------------------------------------------------------- */
int dm_boundary_merge(const float* coarse, float* fine, int n, int S, dm_stream_t stream);
/* (ABI 25) The whole inference tail of dynamask_roi_head.py:138-149 in ONE launch: the two dependent merges
 * S -> 2S -> 4S and, when final_2s is given, the align_corners x2 upsample (dynamask_head.py:240-243,
 * F.interpolate(..., scale_factor=2, align_corners=True)) that produces the 4S x 4S logits the second merge overwrites:
 *   p_s [n,S,S], p_2s [n,2S,2S] (read only: the merged 2S logits are temporaries and are not written back),
 *   final_2s [n,2S,2S] or NULL (then out_4s holds the fine logits on entry and is merged in place),  out_4s [n,4S,4S].
 * Bits: those of dm_upsample2x_bilinear_fwd + dm_boundary_merge(S) + dm_boundary_merge(2S). */
int dm_boundary_merge_chain(const float* p_s, const float* p_2s, const float* final_2s, float* out_4s, int n, int S,
                            dm_stream_t stream);

/* ---------------------------------------------------------------------------
 * K16  deconv 2x2 stride 2 (+bias, +ReLU): nn.ConvTranspose2d(C, Cout, 2, 2)
 * replaces: FCNMaskHead.upsample 'deconv' (mask_heads/fcn_mask_head.py:77-83,121-124).
 * x [NB, C, H, W]; w_packed = dm_deconv_pack_weight of the [C, Cout, 2, 2] weight;
 * out [NB, Cout, 2H, 2W].  relu: bit 0 ReLU; bit 4 (ABI 28): w_packed is dm_deconv_pack_weight_bf16x3's layout (the
 * bf16x3 mode of dm_conv2d_fwd; dm_conv_packed_floats_bf16x3(4 * Cout, 1, 1, &Cin) floats).
 * ------------------------------------------------------------------------- */
int dm_deconv_pack_weight(const float* w_iohw, int Cin, int Cout, float* w_packed, dm_stream_t stream);
int dm_deconv_pack_weight_bf16x3(const float* w_iohw, int Cin, int Cout, float* w_packed, dm_stream_t stream);
int dm_deconv2x2_fwd(const float* x, int NB, int C, int H, int W, const float* w_packed, const float* bias,
                     int Cout, int relu, float* out, dm_stream_t stream);

/* ---------------------------------------------------------------------------
 * K17  CARAFE: kernel normaliser (pixel_shuffle + softmax over k*k) fused with
 * the reassembly.  replaces: mmcv CARAFEPack.kernel_normalizer +
 * feature_reassemble (mask_heads/fcn_mask_head.py:84-87,121).
 * x [NB, C, H, W]; enc [NB, k*k*group*scale*scale, H, W] (content encoder
 * output, before pixel shuffle); out [NB, C, scale*H, scale*W]
 * ------------------------------------------------------------------------- */
int dm_carafe_fwd(const float* x, const float* enc, int NB, int C, int H, int W, int up_kernel, int group,
                  int scale, float* out, dm_stream_t stream);

/* ---------------------------------------------------------------------------
 * K10  resolution selector: straight-through Gumbel-softmax (hard), T = 0.5.
 * replaces: DynaMaskRoIHead.get_mask_label / gumbel_softmax
 *           (roi_heads/dynamask_roi_head.py:84-114); U is the explicit uniform
 *           noise the reference draws at :90.
 * logits, U [N, 4] -> y_soft [N,4] (softmax((logits+g)/T)), index [N] int32
 * (first maximum, as torch.max), one_hot [N,4]
 * ------------------------------------------------------------------------- */
int dm_gumbel_select_fwd(const float* logits, const float* U, int N, int K, float temperature,
                         float* y_soft, float* one_hot, int32_t* index, dm_stream_t stream);

/* ---------------------------------------------------------------------------
 * K13  DetailTarget: Laplacian boundary pyramid target, bit-exact {0,1}.
 * replaces: DetailTarget.forward (losses/cross_entropy_loss.py:363-418).
 * masks [N, S, S] in {0,1} -> out [N, S, S]; fuse = the two fuse_kernel weights, either as host
 * values or (fuse_dev != NULL: two floats in device memory, read by the kernel -- the reference keeps
 * them as an nn.Parameter that weight decay changes every step, Quirk Q7; no host round trip)
 * ------------------------------------------------------------------------- */
int dm_detail_target(const float* masks, int N, int S, float fuse0, float fuse1, const float* fuse_dev, float* out,
                     dm_stream_t stream);

/* ---------------------------------------------------------------------------
 * K12  mask losses of one stage, forward + gradients in one pass.
 * replaces: binary_cross_entropy (losses/cross_entropy_loss.py:56-87) and the
 *           fork's eps-BCE mask_cross_entropy (:90-120) as used at :458-462.
 * inst_pred, det_pred, inst_tgt, det_tgt : [N, HW]; weight [N] (mask_labels[:,idx])
 * sums (device, 2 floats, caller zero-fills): sums[0] += sum of BCE-with-logits,
 *   sums[1] += sum_n weight[n] * sum_p -(t log(s+eps) + (1-t) log(1-s+eps))
 * per_roi_det [N] (optional): the un-weighted per-RoI eps-BCE sums (for d/dweight)
 * grad_inst / grad_det (optional): d sums[0]/d inst_pred, d(eps-BCE)/d det_pred
 *   scaled by weight[n]; the host applies the scalar normalisers.
 * ------------------------------------------------------------------------- */
/* scratch: dm_mask_loss_scratch_floats(N) floats (per-workgroup partial sums, added in a fixed order: the loss and
 * d loss / d weight have the same bits on every run). */
long long dm_mask_loss_scratch_floats(int N);
int dm_mask_loss_fwd_bwd(const float* inst_pred, const float* det_pred, const float* inst_tgt,
                         const float* det_tgt, const float* weight, int N, int HW, float* sums,
                         float* per_roi_det, float* grad_inst, float* grad_det, float* scratch, dm_stream_t stream);

/* One stage of DynaCrossEntropyLoss.forward (cross_entropy_loss.py:455-476) with its normalisers applied in the kernel:
 * w_n = mask_labels[n, stage] ([N, num_stages]), den = sum_n w_n + 1e-5 (detached, :462), n_el = N * HW.
 *   loss_terms[0]  = mean BCE-with-logits of this stage (overwritten: only the last stage's reaches the loss, Quirk Q2)
 *   loss_terms[1] += detail_weight * (N / n_el) / den * sum_n w_n * epsBCE_n
 *   grad_mask_labels[n, stage] = detail_weight / (HW * den) * epsBCE_n           (d loss / d mask_labels, den detached)
 *   grad_inst (optional) = (sigmoid(x) - t) / n_el;  grad_det (optional) = d(detail term) / d det_pred
 * scratch: dm_mask_loss_scratch_floats(N).  Replaces dm_mask_loss_fwd_bwd + ~30 host-side tensor operations per stage. */
int dm_mask_loss_stage(const float* inst_pred, const float* det_pred, const float* inst_tgt, const float* det_tgt,
                       const float* mask_labels, int num_stages, int stage, int N, int HW, float detail_weight,
                       float* loss_terms, float* grad_mask_labels, float* grad_inst, float* grad_det, float* scratch,
                       dm_stream_t stream);

/* ---------------------------------------------------------------------------
 * K9  resolution predictor MaskPre (roi_heads/base_roi_head.py:10-27): BatchNorm
 * batch statistics (train mode; biased variance for normalisation, running
 * stats updated with the unbiased one when the pointers are non-NULL) and the
 * fused BN -> ReLU -> max_pool2d(kernel 3, stride 2, pad 1).  The convs / FCs
 * of MaskPre run through dm_conv2d_fwd.
 * x [NB, C, H, W]; mean/var/gamma/beta [C]; out [NB, C, (H-1)/2+1, (W-1)/2+1]
 * ------------------------------------------------------------------------- */
/* mean_shift (ABI 23; [C] or NULL): the running mean is updated with mean + mean_shift.  Used when x is the activation
 * WITHOUT a per-channel bias that train-mode BatchNorm cancels anyway: MaskPre's conv1 applied to the P2 map before the
 * 56 x 56 extraction (conv1 is 1x1, RoIAlign linear: conv1(RoIAlign(x)) = RoIAlign(W1 x) + b1), base_roi_head.py:13-16. */
int dm_bn_stats(const float* x, int NB, int C, int HW, float* mean, float* var, float* running_mean,
                float* running_var, float momentum, const float* mean_shift, float* scratch, dm_stream_t stream);
/* scratch for dm_bn_stats / dm_bn_relu_maxpool_bwd (may be null: one workgroup per channel) */
long long dm_bn_scratch_floats(int C);
int dm_bn_relu_maxpool_fwd(const float* x, int NB, int C, int H, int W, const float* mean, const float* var,
                           const float* gamma, const float* beta, float eps, float* out, dm_stream_t stream);
/* diagnostic: argmax [NB, C, OH, OW] int32 = plane index (y * W + x) of the tap each pooled output took (first
 * maximum in scan order, the choice dm_bn_relu_maxpool_bwd routes the gradient to) -- what
 * F.max_pool2d(..., return_indices=True) returns in the reference (roi_heads/base_roi_head.py:16,19). */
int dm_bn_relu_maxpool_argmax(const float* x, int NB, int C, int H, int W, const float* mean, const float* var,
                              const float* gamma, const float* beta, float eps, int32_t* argmax, dm_stream_t stream);

/* backward of dm_bn_relu_maxpool_fwd with train-mode statistics (mean/var as
 * returned by dm_bn_stats): grad_x [NB,C,H,W] (overwritten), grad_gamma/grad_beta [C]. */
int dm_bn_relu_maxpool_bwd(const float* x, int NB, int C, int H, int W, const float* mean, const float* var,
                           const float* gamma, const float* beta, float eps, const float* grad_out, float* grad_x,
                           float* grad_gamma, float* grad_beta, float* scratch, dm_stream_t stream);

/* The launches dm_bn_stats (DM_MASK_PRE_STATS; its HW is H * W here), dm_bn_relu_maxpool_fwd (DM_MASK_PRE_FWD) and
 * dm_bn_relu_maxpool_bwd (DM_MASK_PRE_BWD) would make for these HOST numbers: the route each launcher decides on, the very
 * value it then enqueues (nothing is launched, no device is needed).  NB, C, H, W as the call's, and facts in place of its
 * pointers: scratch (one is given; ignored by the forward), align (16, 8 or 4: the bytes x -- for the backward x AND grad_x --
 * is aligned to; a float pointer has 4), and cus, the compute-unit count the backward routes by (<= 0: the current
 * device's, 256 without one).  The routes ask for the alignment of a kernel's widest access: 16 bytes for the vector loop of
 * the split statistics and for both plane kernels of the backward, 8 for the rows forward; a call that lacks it takes the
 * scalar kernels (the scalar loop of the split statistics, the generic forward, the atomic scatter).  LDS is counted static
 * plus dynamic against 64 KB: at exactly 64 KB of plane (1 x 8192) the sums kernel's 16 static bytes take the call to kernel 6.
 * records: HOST array of max_records (>= DM_MASK_PRE_PLAN_MAX_LAUNCHES) x DM_MASK_PRE_PLAN_INTS ints.  Returns the number of
 * launches (0: the forward's empty call, NB = 0) or the error code the call would return for these numbers -- also for an
 * unknown op or align -- and then writes nothing.  Record l, ints [l * DM_MASK_PRE_PLAN_INTS ..):
 *   0 kernel: 0 bn_stats_kernel, 1 bn_stats_split_kernel, 2 bn_stats_finalize_kernel, 3 bn_relu_maxpool_kernel (generic),
 *     4 bn_relu_maxpool_rows_kernel, 5 maxpool_relu_bwd_kernel (the atomic scatter), 6 maxpool_relu_bwd_lds_kernel (plane in
 *     LDS), 7 maxpool_relu_bwd_sums_kernel (plane in LDS, keeps BatchNorm's sums), 8 bn_bwd_kernel, 9 bn_bwd_split_kernel;
 *   1 .. 3 its build: PASS, VEC (1: 16-byte loads), 0 (kernel 1); EVEN (1: 2 x 2 blocks, 0: the element form), PRE (1: a plane
 *     is prefetched into registers), 0 (kernel 7); PASS, 0, 0 (kernel 9); zeros otherwise;
 *   4 grid x, 5 grid y, 6 threads per workgroup, 7 LDS bytes of a workgroup, static plus dynamic;
 *   8 clear: 1 where grad_x is zero-filled (hipMemsetAsync) before the launch. */
#define DM_MASK_PRE_STATS 0
#define DM_MASK_PRE_FWD 1
#define DM_MASK_PRE_BWD 2
#define DM_MASK_PRE_PLAN_INTS 9
#define DM_MASK_PRE_PLAN_MAX_LAUNCHES 3
int dm_mask_pre_plan(int op, int NB, int C, int H, int W, int scratch, int align, int cus, int* records, int max_records);

/* K10 backward: gradient of the soft branch of the straight-through estimator
 * (y_hard = (one_hot - y).detach() + y, dynamask_roi_head.py:112-113). */
int dm_gumbel_select_bwd(const float* y_soft, const float* grad_y, int N, int K, float temperature,
                         float* grad_logits, dm_stream_t stream);

/* ---------------------------------------------------------------------------
 * K14  class-balance entropy of the selector and its gradient.
 * replaces: losses/cross_entropy_loss.py:478-481.
 * mask_labels [N, K] -> loss[0] = sum_k p_k log(p_k + 1e-10), p = colsum/total;
 * grad [N, K] (optional) = d loss / d mask_labels
 * ------------------------------------------------------------------------- */
int dm_class_balance_fwd_bwd(const float* mask_labels, int N, int K, float* loss, float* grad,
                             dm_stream_t stream);

/* ===========================================================================
 * Callers either side of the path ("next" rows 1 and 2).
 * =========================================================================== */

/* Mask-target RoIs: (gt_index, box clipped to the mask canvas).
 * replaces: the numpy clip of DynaMaskHead.get_targets (mask_heads/dynamask_head.py:248-256)
 * and the rois assembly of BitmapMasks.crop_and_resize (core/mask/structures.py:270-276);
 * the crop itself is dm_roi_align_fwd on the GT bitmaps (scale 1, adaptive grid),
 * then dm_threshold_ge(0.5) (structures.py:281-284). */
int dm_mask_target_rois(const float* boxes, const int64_t* gt_inds, int N, float max_w, float max_h, float* rois,
                        dm_stream_t stream);
int dm_threshold_ge(const float* x, long long count, float thr, float* out, dm_stream_t stream);

/* Mask targets from POLYGON annotations: out[n] = S x S bitmap (0 / 1) of object inds[n] in the frame of boxes[n].
 * replaces: PolygonMasks.crop_and_resize + to_ndarray -> polygon_to_bitmap -> pycocotools frPyObjects / merge / decode
 * (core/mask/structures.py:469-503, 544-552, 583-599) as DynaMaskHead.get_targets calls them per image and size
 * (mask_heads/dynamask_head.py:248-262), bit-identical to cocoapi's rleFrPoly arithmetic.
 * verts: [V][2] float64 (x, y) of all polygons of the image; poly_start: [P + 1] first vertex of each polygon;
 * inst_start: [num_objects + 1] first polygon of each object; boxes: [N][4] float32 already clipped to the image;
 * inds: [N]; S <= 256.  One workgroup per RoI. */
int dm_polygon_mask_targets(const double* verts, const int* poly_start, const int* inst_start, int num_objects,
                            const float* boxes, const int64_t* inds, int N, int S, float* out, dm_stream_t stream);

/* K18  paste N masks [N, mask_h, mask_w] into their boxes on an [img_h, img_w] canvas
 * and binarise: out[n, y, x] = (grid_sample(mask_n) >= threshold) as uint8.
 * replaces: _do_paste_mask (mask_heads/fcn_mask_head.py:240-308, skip_empty=False) +
 * the threshold of get_seg_masks (mask_heads/dynamask_head.py:325-339).
 * apply_sigmoid != 0 takes logits (mask_pred.sigmoid() of dynamask_head.py:281).
 * N <= 65535 (the masks are the grid's y dimension): more returns DM_ERR_INVALID_ARG before anything is launched. */
int dm_paste_masks(const float* masks, const float* boxes, int N, int mask_h, int mask_w, int img_h, int img_w,
                   float threshold, int apply_sigmoid, uint8_t* out, dm_stream_t stream);

/* K19  COCO run-length encoding on the device.
 * replaces: encode_mask_results (mmdet/core/mask/utils.py:36-63: pycocotools rleEncode of a
 * column-major host copy of every bitmap) and, in the fused form, the [N, img_h, img_w]
 * canvas of get_seg_masks (mask_heads/dynamask_head.py:325-342) together with its
 * device->host copy.  Outputs: mask_runs[n] = number of run boundaries of mask n,
 * mask_start[n] (N+1 entries) = offset of its boundaries in `positions` (packed, column-major
 * pixel indices j = x*img_h + y where the value changes; the value before j = 0 is 0).
 * Boundaries past `capacity` are counted but not stored (caller re-runs with a larger buffer).
 * seg_scratch: dm_rle_scratch_ints(N, img_h, img_w) int32.
 * dm_rle_string (host code, no GPU work): boundaries -> run lengths -> the printable
 * `counts` string of the COCO RLE format; returns its length, or -(needed) if cap is short.
 * dm_rle_encode_canvas and dm_paste_rle: N <= 65535 (the masks are the grid's y dimension); more returns
 * DM_ERR_INVALID_ARG before anything is launched. */
long long dm_rle_scratch_ints(int N, int img_h, int img_w);
int dm_rle_encode_canvas(const uint8_t* canvas, int N, int img_h, int img_w, int* seg_scratch, int* mask_runs,
                         int* mask_start, int* positions, int capacity, dm_stream_t stream);
int dm_paste_rle(const float* masks, const float* boxes, int N, int mask_h, int mask_w, int img_h, int img_w,
                 float threshold, int apply_sigmoid, int* seg_scratch, int* mask_runs, int* mask_start,
                 int* positions, int capacity, dm_stream_t stream);
long long dm_rle_string(const int* positions, int runs, long long total_pixels, char* out, long long cap);

/* (added to ABI 28) K18 / K19 for the detections of SEVERAL images in one launch (DynaMaskRoIHead.batch_simple_test_mask).
 * Detection n [0, N) belongs to image det_img[n] (int32, device) and the detections of one image are consecutive;
 * img_tab (int64, device) [B][4] = (img_h, img_w, index of the image's first detection, byte offset of its first canvas
 * in `out`); max_pixels = the largest img_h * img_w of the images that have detections.  A detection's pixels are
 * exactly what dm_paste_masks / dm_paste_rle give for it on its own image (same arithmetic).
 * dm_paste_masks_multi: detection n's row-major [img_h, img_w] uint8 bitmap at out + off_b + (n - first_b) * h * w.
 * dm_paste_rle_multi: as dm_paste_rle, with positions local to each detection's own canvas (j = x * img_h + y); the
 * boundaries of all detections are packed into one `positions` buffer (mask_start [N + 1]); boundaries past `capacity`
 * are counted, not stored.  seg_scratch: dm_rle_multi_scratch_ints(N, max_pixels) int32.  A detection whose image index
 * is outside [0, B) is skipped (no pixels written, no runs). */
long long dm_rle_multi_scratch_ints(int N, long long max_pixels);
int dm_paste_masks_multi(const float* masks, const float* boxes, int N, int mask_h, int mask_w, const int* det_img, int B,
                         const long long* img_tab, long long max_pixels, float threshold, int apply_sigmoid, uint8_t* out,
                         dm_stream_t stream);
int dm_paste_rle_multi(const float* masks, const float* boxes, int N, int mask_h, int mask_w, const int* det_img, int B,
                       const long long* img_tab, long long max_pixels, float threshold, int apply_sigmoid, int* seg_scratch,
                       int* mask_runs, int* mask_start, int* positions, int capacity, dm_stream_t stream);

/* K22  fully connected layer out[N, M] = x[N, K] . w[M, K]^T + bias (nn.Linear layouts), optional
 * ReLU; fp32 MFMA.  replaces: the nn.Linear stack of Shared2FCBBoxHead
 * (roi_heads/bbox_heads/convfc_bbox_head.py:101-108,143-186) and MaskPre's fc1 / fc2
 * (roi_heads/base_roi_head.py:17-18,24-26).  K % 4 == 0 (else DM_ERR_UNSUPPORTED).  K is split over workgroups in segments
 * whose length depends on K alone (256 elements up to K = 4096, 1024 above; dm_fc_scratch_floats = segments x N x M, 0
 * for a single segment); the partial sums go to `scratch` (dm_fc_scratch_floats() floats; may be NULL when that
 * is 0) and are added in a fixed order: an output row has the same bits whatever N is, run to run. */
long long dm_fc_scratch_floats(int N, int K, int M);
int dm_fc_fwd(const float* x, const float* w, const float* bias, int N, int K, int M, int relu, float* out,
              float* scratch, dm_stream_t stream);

/* K20  bbox branch post-processing: softmax over the class logits, DeltaXYWH decode, clip to
 * the image, rescale.  replaces: BBoxHead.get_bboxes up to the NMS
 * (roi_heads/bbox_heads/bbox_head.py:186-217) and delta2bbox
 * (core/bbox/coder/delta_xywh_bbox_coder.py:165-204).  rois [N, roi_stride] with x1 at column
 * roi_x0 (5 / 1 for the reference's [batch, x1, y1, x2, y2] rows); cls_score [N, num_classes+1]
 * or null; bbox_pred [N, 4*num_classes] ([N, 4] if class_agnostic) or null (then the rois
 * themselves are clipped); clip_h/clip_w <= 0: no clipping; scale_x/scale_y: divide the boxes
 * (rescale=True), 1 otherwise.  Outputs scores [N, num_classes+1], bboxes like bbox_pred.
 * K21  dm_nms_mask: suppression bit matrix of M score-sorted boxes [M, 4] (bit j of row i,
 * j > i, set when IoU > iou_threshold; offset 0/1 as mmcv.ops.nms) -- replaces the device half of
 * mmcv.ops.nms as called by multiclass_nms (core/post_processing/bbox_nms.py:5-68);
 * dm_nms_reduce is the host half (greedy pass), returns the number of kept indices. */
int dm_bbox_decode(const float* rois, int roi_stride, int roi_x0, const float* cls_score, const float* bbox_pred,
                   int N, int num_classes, int class_agnostic, const float* means, const float* stds,
                   float wh_ratio_clip, float clip_h, float clip_w, float scale_x, float scale_y, float* scores,
                   float* bboxes, dm_stream_t stream);
int dm_nms_mask(const float* boxes_sorted, int M, float iou_threshold, int offset, unsigned long long* mask,
                dm_stream_t stream);
int dm_nms_reduce(const unsigned long long* mask_host, int M, int* keep, int max_keep);
/* (added to ABI 28) K21 over B segments (images) at once, greedy pass on the device.  boxes_sorted [sum M_b, 4]: the segments
 * one after the other, each score-sorted on its own; seg_tab (int64, device) [B][3] = (first row, M_b, offset in
 * unsigned long longs of the segment's matrix in `mask`).  Segment b's matrix is [M_b][ceil(M_b / 64)] (the rows of
 * dm_nms_mask for those M_b boxes alone): the block-diagonal layout, mask_words = sum M_b * ceil(M_b / 64) in all.
 * max_words = the largest ceil(M_b / 64).  No bit compares boxes of two segments.
 * dm_nms_reduce_segmented: dm_nms_reduce of every segment, one wave per segment: keep[first_b + k] (int32) = the k-th
 * kept box of segment b (index within the segment's sorted rows), counts[b] (int32) = number kept (<= max_keep when
 * max_keep >= 0).  max_words <= 20480 (the removed bits live in LDS). */
int dm_nms_mask_segmented(const float* boxes_sorted, int B, const long long* seg_tab, int max_words, float iou_threshold,
                          int offset, unsigned long long* mask, long long mask_words, dm_stream_t stream);
int dm_nms_reduce_segmented(const unsigned long long* mask, int B, const long long* seg_tab, int max_words, int max_keep,
                            int* keep, int* counts, dm_stream_t stream);

/* (added to ABI 28) Test-time augmentation over V views of one image (DynaMaskRoIHead.aug_test: bbox_mapping,
 * merge_aug_bboxes and merge_aug_masks of core/bbox/transforms.py and core/post_processing/merge_augs.py).
 * view_tab (float, device) [V][DM_AUG_VIEW_FLOATS] = (scale factor of x1, y1, x2, y2; img_h, img_w of the view; flip code
 * DM_AUG_FLIP_*; unused).  Every element is the reference's fp32 operations in its order.
 * dm_bbox_mapping_multi: boxes [n, box_stride >= 4] (x1 y1 x2 y2 in the first four columns) -> out_rois [V][n][5], the
 *   RoI rows of view v (batch column 0, then b * sf, then the flip: x = img_w - x' for 'horizontal', y = img_h - y' for
 *   'vertical', the two coordinates swapped).
 * dm_merge_aug_bboxes: ptr_tab (int64, device) [V][2] = addresses of view v's boxes [n, box_cols] (box_cols % 4 == 0,
 *   box_cols / 4 boxes per row) and scores [n, score_cols] (fp32, row-major).  Each box coordinate is flipped back (same
 *   formula as the mapping) and divided by the view's scale factor; boxes and scores are then summed over the views in
 *   order and divided by V: out_boxes [n, box_cols], out_scores [n, score_cols].  n <= 65535.
 * dm_merge_aug_masks: logit_tab (int64, device) [V] = address of view v's logits [n, K, S, S] (fp32); labels (int64,
 *   device) [n], read only when K > 1 (clamped into [0, K)).  out [n, 1, S, S] = the mean over the views, in order, of
 *   dm_sigmoid of the label's channel read at the un-flipped position ('horizontal': column S - 1 - x, 'vertical': row
 *   S - 1 - y).  The sigmoid is the paste kernels' apply_sigmoid, so one view gives the probabilities dm_paste_masks
 *   computes from the logits, bit for bit. */
#define DM_AUG_VIEW_FLOATS 8
#define DM_AUG_FLIP_NONE 0
#define DM_AUG_FLIP_HORIZONTAL 1
#define DM_AUG_FLIP_VERTICAL 2
int dm_bbox_mapping_multi(const float* boxes, int box_stride, int n, int V, const float* view_tab, float* out_rois,
                          dm_stream_t stream);
int dm_merge_aug_bboxes(const long long* ptr_tab, const float* view_tab, int V, int n, int box_cols, int score_cols,
                        float* out_boxes, float* out_scores, dm_stream_t stream);
int dm_merge_aug_masks(const long long* logit_tab, const float* view_tab, int V, int n, int K, int S, const long long* labels,
                       float* out, dm_stream_t stream);

/* (added to ABI 29) RPNHead.aug_test_rpn: the first half of merge_aug_proposals (merge_augs.py:27-38) for every image and
 * view in one launch.  Segment s is one (image, view): seg_tab (int64, device) [S][3] = (address of its proposals [n, 5]
 * fp32, dense rows; n; its first row of `out`), view_tab (float, device) [S][DM_AUG_VIEW_FLOATS] its view row as above.
 * out [sum n, 5]: x1 y1 x2 y2 mapped back to the original image (bbox_mapping_back: the flip against the view's
 * img_shape, then a true fp32 division by the scale factor, never a multiply by a reciprocal) and the score copied.
 * max_rows >= every n; num_segments <= 65535.  The caller lays the segments out image after image, so `out` is the
 * reference's torch.cat per image. */
int dm_proposals_mapping_back(const long long* seg_tab, const float* view_tab, int num_segments, int max_rows, float* out,
                              dm_stream_t stream);

/* ===========================================================================
 * Backward (training step).  Replaces what autograd derives for the reference
 * modules above plus mmcv's DeformConv2d backward
 * (mmdet/ops/dcn/src/deform_conv_cuda.cpp:262-486, deform_conv_cuda_kernel.cu:117-188,279-436).
 * The conv DATA gradient is dm_conv2d_fwd with dm_conv_pack_weight(transpose_flip=1).
 * =========================================================================== */

/* grad[i] = 0 where out[i] <= 0 (in place). */
int dm_relu_bwd(float* grad, const float* out, long long count, dm_stream_t stream);

/* g_logit[n,p] (+)= (ga[n,p] + gb[n,p]) * s(1-s), s = sig[n,p]; sig / ga / gb may be
 * channel slices of wider tensors (batch strides in floats); gb may be NULL. */
int dm_sigmoid_bwd(const float* sig, long long sig_bs, const float* ga, long long ga_bs, const float* gb,
                   long long gb_bs, int N, int HW, float* g_logit, int accumulate, dm_stream_t stream);

/* out[c] (+)= sum_{n,p} g[n, c, p]  (bias gradient). */
int dm_channel_sum(const float* g, long long batch_stride, int NB, int C, int HW, float* out, int accumulate,
                   dm_stream_t stream);

/* conv weight gradient, fp32 MFMA GEMM over the pixel dimension, atomically
 * accumulated: dw[co*ldw + col_offset + ci*k*k + tap] += sum_{n,y,x} dy[n,co,y,x] *
 * x[n,ci,y+dy-1,x+dx-1].  One call per concat source (col_offset = channel base * k*k);
 * the caller zero-fills dw.  db (optional, [Cout]): the bias gradient db[co] += sum_{n,y,x} dy[n,co,y,x], taken from
 * the dy values the kernel stages anyway (pass it with ONE of the sources of a concat). */
int dm_conv2d_wgrad(const float* dy, long long dy_batch_stride, int Cout, const float* x, long long x_batch_stride,
                    int Cs, int NB, int H, int W, int ksize, float* dw, int ldw, int col_offset, float* db,
                    dm_stream_t stream);

/* The same sums without atomics: every split of the pixel axis writes its partial tile to a slab of `scratch`, a second
 * kernel adds the slabs in index order into dw (and the splits' bias rows into db) -- bit-identical from run to run, as the
 * reference's weight gradient is (a deterministic addmm_, mmdet/ops/dcn/src/deform_conv_cuda.cpp:460-465).  scratch:
 * 16-byte aligned, scratch_floats > 0; contents undefined afterwards; not shared between streams.  dw / db are accumulated
 * into, as above.  A call whose slabs do not fit the scratch, or whose scratch is not aligned, is NOT refused: it returns
 * DM_OK and adds with the float atomics of dm_conv2d_wgrad (not the same bits every run).  dm_conv2d_wgrad_plan says which
 * a call takes (record field 17), and a caller that needs the same bits asks it first.
 * dm_conv2d_wgrad_scratch_floats(): target x (16384 + 256) floats, target = two workgroups per compute unit (or
 * DM_WGRAD_WGS).  It suffices for every call whose output tiles (field 9 x field 10 of the plan: cout tiles x column tiles,
 * or 1 x channel groups of the narrow 3x3 kernel) number at most `target`: such a launch is split into at most target
 * workgroups of at most 16384 slab floats each.  A call with more tiles is not split and needs a slab as large as its
 * padded dw (K-waves x cout tiles x 64 WGM x column tiles x 64 WGN floats), which may exceed the bound: 1024 -> 1024
 * channels 3x3 at 256 compute units is 8 x 72 = 576 tiles, 9.44 M floats against 8.52 M. */
long long dm_conv2d_wgrad_scratch_floats(void);
int dm_conv2d_wgrad_slab(const float* dy, long long dy_batch_stride, int Cout, const float* x, long long x_batch_stride,
                         int Cs, int NB, int H, int W, int ksize, float* dw, int ldw, int col_offset, float* db,
                         float* scratch, long long scratch_floats, dm_stream_t stream);

/* (added to ABI 29) The launches dm_conv2d_wgrad / dm_conv2d_wgrad_slab / dm_conv2d_wgrad_fx would make for these HOST
 * arguments: the route the launcher decides on, the very value it then enqueues (nothing is launched, no device is needed --
 * without one the compute-unit count is taken as 256).  Arguments as dm_conv2d_wgrad_slab's, with facts in place of the
 * pointers: has_bias (db given), mode (0 dm_conv2d_wgrad, 1 dm_conv2d_wgrad_slab, 2 dm_conv2d_wgrad_fx), scratch_floats
 * (mode 1 only), io_aligned8 (dy and x are both 8-byte aligned), scratch_aligned16.  The DM_WGRAD_WGS knob applies as it does
 * to launches (read once per process).
 * records: HOST array of max_records (>= DM_WGRAD_PLAN_MAX_LAUNCHES) x DM_WGRAD_PLAN_INTS ints.  Returns the number of
 * launches (1; 2: the slab reduce follows) or the error code the call would return for these numbers, and then writes
 * nothing.  Record l, ints [l * DM_WGRAD_PLAN_INTS ..):
 *   0 kernel: 0 conv_wgrad_kernel (the GEMM), 1 conv_wgrad3_narrow_kernel, 2 wgrad_slab_reduce_kernel;
 *   1 .. 5 its template parameters: KS, WGM, WGN, WGK, TAIL (kernel 0); 3, 0, 0, 0, TAIL (kernel 1); P, 0, 0, 0, 0 (kernel 2);
 *   6 grid x, 7 threads per workgroup, 8 dynamic LDS bytes;
 *   9 MT, 10 JT: cout tiles and column tiles (kernel 1: 1 and groups of 32 input channels; kernel 2: zeros);
 *   11 splits of the pixel axis, 12 what a split walks: chunks of 32 pixels (kernel 0), (image, row band) units (kernel 1),
 *      0 (kernel 2);
 *   13 slabs (0: none), 14 slab row length, 15 rows of a split's bias row block, 16 floats per slab (saturates at INT_MAX);
 *   17 the accumulation TAKEN: 0 float atomics, 1 slabs + reduce, 2 fixed point.  Mode 1 with 0 here is the fallback. */
#define DM_WGRAD_PLAN_INTS 18
#define DM_WGRAD_PLAN_MAX_LAUNCHES 2
int dm_conv2d_wgrad_plan(long long dy_batch_stride, int Cout, long long x_batch_stride, int Cs, int NB, int H, int W, int ksize,
                         int has_bias, int mode, long long scratch_floats, int io_aligned8, int scratch_aligned16, int* records,
                         int max_records);

/* adjoint of dm_upsample2x_bilinear_fwd; fwd_out_for_relu (optional) masks the
 * fused ReLU; grad_in is overwritten (no zero-fill needed).  Which kernel a shape gets: dm_bwd_plan, DM_BWD_UPSAMPLE. */
int dm_upsample2x_bilinear_bwd(const float* grad_out, const float* fwd_out_for_relu, int NC, int H, int W,
                               int align_corners, float* grad_in, dm_stream_t stream);

/* adjoint of dm_point_sample_fwd, scatter-add into grad_feat (caller zero-fills).  Launch: dm_bwd_plan,
 * DM_BWD_POINT_SAMPLE. */
int dm_point_sample_bwd(const float* grad_out, int B, int C, int H, int W, const float* rois, int N, int S,
                        float spatial_scale, float* grad_feat, dm_stream_t stream);

/* backward of dm_class_logits_fwd: grad_x (+)= W[label] * grad; grad_w/grad_b rows of
 * the RoI's class accumulated atomically (caller zero-fills them).  Launches of this and of its _slab and _fx forms:
 * dm_bwd_plan, DM_BWD_CLASS_LOGITS. */
int dm_class_logits_bwd(const float* x, int N, int C, int HW, const float* w_inst, const float* w_det,
                        int num_classes, const int64_t* labels, const float* grad_inst, const float* grad_det,
                        float* grad_x, int accumulate_x, float* grad_w_inst, float* grad_b_inst, float* grad_w_det,
                        float* grad_b_det, dm_stream_t stream);
/* The same gradients without contended atomics: every RoI's sums go to `scratch` (dm_class_logits_bwd_scratch_floats(N, C)
 * floats, contents undefined afterwards) and a second launch adds, per class, the RoIs of that class in RoI order.  The RoIs
 * of an image share a few classes: 256 RoIs of one class are 256 serialised atomics per address in dm_class_logits_bwd
 * (27 -> 130 us at 256 x 256 x 14 x 14).  Deterministic (fixed order of additions; the reference's autograd accumulates the
 * gathered rows unordered: mmdet/models/roi_heads/mask_heads/dynamask_head.py:112-113 `[torch.arange(n), labels]`). */
long long dm_class_logits_bwd_scratch_floats(int N, int C);
int dm_class_logits_bwd_slab(const float* x, int N, int C, int HW, const float* w_inst, const float* w_det,
                             int num_classes, const int64_t* labels, const float* grad_inst, const float* grad_det,
                             float* grad_x, int accumulate_x, float* grad_w_inst, float* grad_b_inst, float* grad_w_det,
                             float* grad_b_det, float* scratch, long long scratch_floats, dm_stream_t stream);

/* DCNv1 backward pieces.  col / colgrad: [NB, 9*C, H, W] with rows tap-major
 * (row = tap*C + ci).  dm_dcn_weight_permute converts W[co][ci][tap] <->
 * Wt[(tap*C+ci)][co] so that both GEMMs run as 1x1 convs over the column matrix.
 * dm_deform_col2im_coord overwrites grad_x and grad_offset (no zero-fill needed):
 * the scatter-adds of one (image, channel) plane are accumulated in LDS.  Which build a shape gets, and the shapes
 * dm_deform_im2col (W < 2) and dm_deform_col2im (a plane of accumulators beyond 64 KB) refuse as DM_ERR_UNSUPPORTED:
 * dm_bwd_plan. */
int dm_deform_im2col(const float* x, const float* offset, int NB, int C, int H, int W, int deform_groups,
                     float* col, dm_stream_t stream);
int dm_deform_col2im_coord(const float* colgrad, const float* x, const float* offset, int NB, int C, int H, int W,
                           int deform_groups, float* grad_x, float* grad_offset, dm_stream_t stream);
/* the two halves of dm_deform_col2im_coord as separate launches (ABI 13): they share only their inputs, so a caller
 * may issue them on two streams -- the coordinate gradient is bound by its gathers, col2im by LDS atomics. */
int dm_deform_coord_grad(const float* colgrad, const float* x, const float* offset, int NB, int C, int H, int W,
                         int deform_groups, float* grad_offset, dm_stream_t stream);
int dm_deform_col2im(const float* colgrad, const float* offset, int NB, int C, int H, int W, int deform_groups,
                     float* grad_x, dm_stream_t stream);
int dm_dcn_weight_permute(const float* src, float* dst, int Cout, int C, int to_colmajor, int accumulate,
                          dm_stream_t stream);

/* The launches of the six training-side launchers above for these HOST numbers: the route each decides on, the very value
 * it then enqueues (nothing is launched, no device is needed -- without one the compute-unit count is taken as 256).
 * op and its `numbers` (count of them), the call's int arguments with facts in place of the pointers:
 *   DM_BWD_IM2COL dm_deform_im2col, DM_BWD_COORD_GRAD dm_deform_coord_grad, DM_BWD_COL2IM dm_deform_col2im (5; the launches
 *     of dm_deform_col2im_coord are those of the last two, in that order): NB, C, H, W, deform_groups;
 *   DM_BWD_UPSAMPLE dm_upsample2x_bilinear_bwd (4): NC, H, W, align_corners;
 *   DM_BWD_POINT_SAMPLE dm_point_sample_bwd / _fx (7): B, C, H, W, N, S, fx (1: dm_point_sample_bwd_fx);
 *   DM_BWD_CLASS_LOGITS dm_class_logits_bwd / _slab / _fx (7): N, C, HW, num_classes, mode (0 dm_class_logits_bwd, 1 _slab,
 *     2 _fx), aligned16 (x, grad_x, grad_inst and grad_det are all 16-byte aligned), scratch_floats (mode 1 only).
 * records: HOST array of max_records (>= DM_BWD_PLAN_MAX_LAUNCHES) x DM_BWD_PLAN_INTS ints.  Returns the number of launches
 * (0: an empty call; 2: the class-logit reduce follows) or the error code the call would return for these numbers -- also
 * for an unknown op, a wrong count or a number that is no int -- and then writes nothing.  Record l, ints
 * [l * DM_BWD_PLAN_INTS ..):
 *   0 kernel: 0 deform_im2col_lds_kernel, 1 deform_im2col_kernel, 2 dcn_coord_grad_lds_kernel, 3 dcn_coord_grad_kernel,
 *     4 dcn_col2im_lds_kernel, 5 upsample2x_bwd_lds_kernel, 6 upsample2x_bwd_gather_kernel, 7 upsample2x_bwd_ac_lds_kernel,
 *     8 upsample2x_bwd_kernel (the scatter), 9 point_sample_bwd_gather_kernel, 10 point_sample_bwd_kernel (the scatter),
 *     11 class_logits_bwd_wave_kernel, 12 class_logits_bwd_kernel, 13 class_logits_bwd_reduce_kernel;
 *   1 .. 3 its build: CT, 0, 0 (kernels 0, 4: planes per workgroup; 1: channels per chunk, an argument); IT, XS, NT (2);
 *     NT, 0, 0 (7); CT, 0, accumulation (9, 10); CPW, IT, accumulation (11); 0, 0, accumulation (12, 13); zeros otherwise.
 *     Accumulation TAKEN: 0 float atomics, 1 per-RoI slabs + reduce, 2 fixed point;
 *   4 grid x, 5 grid y, 6 threads per workgroup, 7 dynamic LDS bytes;
 *   8 clear: 1 where the output is zero-filled (hipMemsetAsync) before the launch. */
#define DM_BWD_IM2COL 0
#define DM_BWD_COORD_GRAD 1
#define DM_BWD_COL2IM 2
#define DM_BWD_UPSAMPLE 3
#define DM_BWD_POINT_SAMPLE 4
#define DM_BWD_CLASS_LOGITS 5
#define DM_BWD_PLAN_INTS 9
#define DM_BWD_PLAN_MAX_LAUNCHES 2
int dm_bwd_plan(int op, const long long* numbers, int count, int* records, int max_records);

/* SGD(momentum, weight decay) step on a flat fp32 buffer; grad_scale folds the
 * 1/world_size of the gradient all-reduce (apis/train.py:75-79 DDP averaging). */
int dm_sgd_momentum_step(float* params, const float* grads, float* momentum_buf, long long count, float lr,
                         float momentum, float weight_decay, float grad_scale, int first_step, dm_stream_t stream);

/* Backward of the FCNMaskHead upsample layers (mask_heads/fcn_mask_head.py:84-96; the forward of the
 * deconv / CARAFE / bilinear forms is above).
 * dm_carafe_bwd: gradients of dm_carafe_fwd with respect to x and enc (mmcv carafe backward +
 *   kernel_normalizer backward), for scale 2, H*W <= 256 (the mask head: 14x14 -> 28x28), up_kernel 3 or 5,
 *   (C / group) % 4 == 0 and a padded x tile of CT channels (CT = 32, 16 or 4, the largest that divides C / group)
 *   within 64 KB of LDS; any H and W under that, odd ones included.  Other shapes return DM_ERR_UNSUPPORTED and
 *   write nothing.  scratch: dm_carafe_bwd_scratch_floats() floats.
 * dm_upsample2x_nearest_fwd / _bwd: nn.Upsample(scale_factor=2, mode='nearest') and its adjoint.
 * dm_pixel_unshuffle2x: out[n, (dy*2+dx)*C + c, y, x] = in[n, c, 2y+dy, 2x+dx]: with it the backward of the
 *   2x2 stride-2 ConvTranspose2d is dm_conv2d_fwd (data) + dm_conv2d_wgrad (weights) on 1x1 GEMMs. */
long long dm_carafe_bwd_scratch_floats(int NB, int H, int W, int up_kernel, int group);
int dm_carafe_bwd(const float* x, const float* enc, const float* grad_out, int NB, int C, int H, int W, int up_kernel,
                  int group, int scale, float* grad_x, float* grad_enc, float* scratch, dm_stream_t stream);
int dm_upsample2x_nearest_fwd(const float* in, int NC, int H, int W, float* out, dm_stream_t stream);
int dm_upsample2x_nearest_bwd(const float* grad_out, int NC, int H, int W, float* grad_in, dm_stream_t stream);
int dm_pixel_unshuffle2x(const float* in, int NB, int C, int H, int W, float* out, dm_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Training side of the RoI head around the mask path (SURVEY 8b "forward_train", 8f rank 4):
 * RoI assignment / sampling inputs, bbox regression targets and the two bbox-branch losses.
 * ------------------------------------------------------------------------------------------ */

/* bbox_overlaps(bboxes1 [n1,4], bboxes2 [n2,4], mode, is_aligned=False, eps) -> [n1, n2]
 * (core/bbox/iou_calculators/iou2d_calculator.py:37-131); mode_iof: 0 = 'iou', 1 = 'iof'.
 * Rounded exactly like the reference's separate torch ops (no fused multiply-add). */
int dm_bbox_overlaps(const float* bboxes1, int n1, const float* bboxes2, int n2, int mode_iof, float eps, float* out,
                     dm_stream_t stream);

/* MaxIoUAssigner.assign_wrt_overlaps (core/bbox/assigners/max_iou_assigner.py:129-212) for
 * num_gts > 0 and num_bboxes > 0: overlaps [num_gts, num_bboxes] -> gt_inds [n] (-1 ignore,
 * 0 negative, i+1 = gt i), max_overlaps [n], labels [n] (gt label or -1; NULL with gt_labels
 * NULL).  A float neg_iou_thr t is (neg_iou_lo, neg_iou_hi) = (0, t).  scratch: 2*num_gts floats. */
int dm_max_iou_assign(const float* overlaps, int num_gts, int num_bboxes, float pos_iou_thr, float neg_iou_lo,
                      float neg_iou_hi, float min_pos_iou, int match_low_quality, int gt_max_assign_all,
                      const int64_t* gt_labels, float* scratch, int64_t* gt_inds, float* max_overlaps, int64_t* labels,
                      dm_stream_t stream);

/* RoI sampling: BaseSampler.sample + RandomSampler._sample_pos / _sample_neg + SamplingResult
 * (core/bbox/samplers/base_sampler.py:35-101, random_sampler.py:31-75, sampling_result.py:21-49),
 * stated as a selection by key.  Candidate boxes bboxes [M,4] (the n_prepended ground-truth boxes first
 * when the sampler adds them as proposals) with AssignResult.gt_inds [M] (i+1 = gt i, 0 negative,
 * -1 ignored) and optional labels [M].  quota_pos = int(num * pos_fraction) positives at most, then
 * num - (positives kept) negatives at most, further limited to int(neg_pos_ub * max(1, positives kept))
 * when neg_pos_ub >= 0.  A class within its quota is kept whole; a larger one keeps the boxes with
 * the quota's smallest keys (ties: lower index) -- a uniformly random subset when the keys are
 * i.i.d. noise.  keys_by_class_rank = 0: pos_keys / neg_keys are [M], indexed by box (both may be the
 * same noise tensor); 1: pos_keys[r] / neg_keys[r] belong to the r-th positive / negative in index
 * order (the inverse of the reference's torch.randperm(count) reproduces its choice: test hook).
 * Keys must be finite.  Kept boxes leave in ascending index order (the reference's .unique()).
 * Outputs have capacity `num` rows; counts[4] = (positives kept, negatives kept, positive candidates,
 * negative candidates).  pos_gt_bboxes[o] = gt_bboxes[gt_inds - 1], pos_assigned_gt_inds = gt_inds - 1,
 * pos_is_gt[o] = index < n_prepended, pos_gt_labels (NULL with labels NULL) = labels[index].
 * scratch: 3 * M int32.  One workgroup; O(M^2 / 1024) compares per thread when a class is over quota. */
int dm_random_sample(const int64_t* gt_inds, const float* bboxes, int M, int n_prepended, const float* gt_bboxes,
                     int num_gts, const int64_t* labels, const float* pos_keys, const float* neg_keys,
                     int keys_by_class_rank, int num, int quota_pos, double neg_pos_ub, int32_t* scratch,
                     int64_t* pos_inds, int64_t* neg_inds, int32_t* counts, float* pos_bboxes, float* neg_bboxes,
                     float* pos_gt_bboxes, int64_t* pos_assigned_gt_inds, int64_t* pos_gt_labels, uint8_t* pos_is_gt,
                     dm_stream_t stream);
/* the gt_bboxes_ignore branch of MaxIoUAssigner.assign (max_iou_assigner.py:107-118): overlaps[:, n] = -1 where
 * box n's largest IoF with an ignore region exceeds thr.  iof = dm_bbox_overlaps(mode_iof = 1) of (boxes, regions)
 * [N][I] (boxes_major = 1, ignore_wrt_candidates) or of (regions, boxes) [I][N] (boxes_major = 0). */
int dm_ignore_columns(float* overlaps, int G, int N, const float* iof, int I, int boxes_major, float thr,
                      dm_stream_t stream);

/* bbox2delta (core/bbox/coder/delta_xywh_bbox_coder.py:74-116): proposals, gt [n,4] -> deltas [n,4]. */
int dm_bbox_encode(const float* proposals, const float* gt, int n, const float* means, const float* stds, float* deltas,
                   dm_stream_t stream);

/* cross_entropy(pred, label, weight, reduction='mean', avg_factor) * loss_weight, forward and
 * backward in one pass (losses/cross_entropy_loss.py:9-38, utils.py:26-52), plus
 * accuracy(pred, label) top-1 in percent (losses/accuracy.py:4-49):
 *   loss[0]    = scale * sum_i weight_i * (logsumexp(score_i) - score_i[label_i]),  scale = loss_weight / avg_factor
 *   grad[i, c] = scale * weight_i * (softmax(score_i)[c] - [c == label_i])          (NULL: forward only)
 *   correct[0] = 100 / N * #{i : argmax_c score_i[c] == label_i}                     (NULL: skipped)
 * weight NULL = all ones.  scratch: 2*N floats.  Row sums are added in a fixed order. */
int dm_softmax_ce_fwd_bwd(const float* cls_score, const int64_t* labels, const float* weight, int N, int C, float scale,
                          float* scratch, float* loss, float* correct, float* grad, dm_stream_t stream);

/* BBoxHead.loss, regression half (roi_heads/bbox_heads/bbox_head.py:159-182) with L1Loss
 * (losses/smooth_l1_loss.py:29-42,104-136): rows with 0 <= label < num_classes are positive;
 * their prediction is bbox_pred[i, label_i, :] (num_boxes_per_row = num_classes) or
 * bbox_pred[i, 0, :] (class agnostic, num_boxes_per_row = 1):
 *   loss[0] = scale * sum_pos sum_c |pred - target| * weight,   scale = loss_weight / avg_factor
 *   grad    = d loss / d bbox_pred [N, num_boxes_per_row*4] (overwritten; NULL: forward only)
 * No positive row: loss 0, grad 0 (the reference's `bbox_pred.sum() * 0`).  scratch: N floats. */
int dm_l1_loss_fwd_bwd(const float* bbox_pred, const int64_t* labels, const float* targets, const float* weights, int N,
                       int num_boxes_per_row, int num_classes, float scale, float* scratch, float* loss, float* grad,
                       dm_stream_t stream);

/* Gradient clipping of the flat gradient buffer (optimizer_config grad_clip,
 * configs/dynamask/coco/r50-dynamask-1x.py:274; OptimizerHook.py:10-14 -> clip_grad_norm_):
 * dm_sumsq: out[0] = sum x^2 (fixed-order two-stage sum; scratch dm_sumsq_scratch_floats());
 * dm_clip_scale: x *= min(1, max_norm / (sqrt(sumsq[0]) + 1e-6)) with sumsq read on the device
 * (the caller may have added the other parameter groups' sums into it). */
long long dm_sumsq_scratch_floats(void);
int dm_sumsq(const float* x, long long count, float* scratch, float* out, dm_stream_t stream);
int dm_clip_scale(float* x, long long count, const float* sumsq, float max_norm, dm_stream_t stream);
/* x *= factor: a parameter group's gradient scale (the reference's optional OptimizerHook_ multiplies the
 * gradients of roi_head.mask_predictor by 0.05 between clipping and the step, OptimizerHook.py:27-29). */
int dm_scale(float* x, long long count, float factor, dm_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Deterministic accumulation (SURVEY 7 "hard parts": a deterministic mode for parity tests; the
 * reference's weight gradient is a deterministic addmm_, mmdet/ops/dcn/src/deform_conv_cuda.cpp:460-465).
 * The entry points above that accumulate across workgroups -- dm_conv2d_wgrad, dm_channel_sum,
 * dm_class_logits_bwd (its four parameter gradients), dm_point_sample_bwd -- add with float atomics, so the
 * last bits of their sums depend on the order in which workgroups arrive.  Each has an *_fx twin with the
 * same arguments whose accumulation target is a buffer of 64-bit FIXED-POINT cells (value * 2^36, two's
 * complement; same indexing as the float target, the caller zero-fills it): integer addition is associative,
 * so the sum is exact in that format and identical on every run.  dm_fx_to_float converts
 * (out[i] (+)= fx[i] * 2^-36, NaN for a poisoned cell; `clear` re-zeroes fx).
 *
 * Fixed-point accumulators: the contract (these cells and the LDS cells of dm_deform_col2im[_coord] and of the
 * scatter form of dm_point_sample_bwd).
 *  - Resolution.  ABSOLUTE, 2^-36 (1.5e-11) per ADDEND, whatever the scale of the gradients: an addend is the fp32
 *    value the float path would add (gradient * bilinear weight, or a workgroup's partial sum) put on the 2^-36 grid
 *      - cut towards zero in dm_deform_col2im (error < 2^-36 per addend, <= 2 * 2^-36 where H * W % 4 != 0);
 *      - rounded to nearest everywhere else (error <= 2^-37 per addend; the scatter form of dm_point_sample_bwd rounds
 *        the exact product, not the fp32 one).
 *    So a cell that K addends reach is within K grid units of the sum of its fp32 addends, and a gradient of 1e-9 is
 *    held to about 1 %: there is no relative accuracy below the grid.  (Losses normalised by the element count give
 *    peaks of 1e-5 .. 1e-3 here: 5 to 7 digits per addend.)
 *  - Range.  LDS cells: every addend |g * w| < 2^27 (1.3e8), ensured by |g| < 2^27, and |sum| < 2^27 at any
 *    moment.  *_fx cells: every addend |v| < 2^25 (3.3e7), and |sum| < 2^25 at any moment.  A sum of in-range addends that leaves the range is
 *    UNSPECIFIED (it may wrap, or read as poison).
 *  - Poison.  An addend outside the range -- NaN, Inf, or finite and too large -- is not dropped and not saturated: it
 *    poisons its target, which then reads NaN.  LDS kernels poison the whole output plane (image, channel) of the bad
 *    gradient; into a float target every cell of the plane's footprint becomes NaN, into an fx target every such cell
 *    is poisoned.  An fx cell is poisoned by a signed maximum with 2^63 - 1, which absorbs: any number of bad addends,
 *    mixed in any order with in-range ones, leaves |cell| >= 2^61, and dm_fx_to_float turns exactly those cells into
 *    NaN.  The bits of every other cell are those of the run without the bad addends.
 * Everything else in the training step is deterministic by construction (fixed-order partial sums, LDS
 * fixed-point scatter, gather-form adjoints) except dm_roi_align_bwd (float atomics into the FPN-map
 * gradients, as in the reference's RoIAlign backward).  The host switch is DM_DETERMINISTIC=1
 * (dynamask_amd.ops.DETERMINISTIC).
 * ------------------------------------------------------------------------------------------ */
int dm_conv2d_wgrad_fx(const float* dy, long long dy_batch_stride, int Cout, const float* x, long long x_batch_stride,
                       int Cs, int NB, int H, int W, int ksize, long long* dw_fx, int ldw, int col_offset,
                       long long* db_fx, dm_stream_t stream);
int dm_channel_sum_fx(const float* g, long long batch_stride, int NB, int C, int HW, long long* out_fx, dm_stream_t stream);
int dm_class_logits_bwd_fx(const float* x, int N, int C, int HW, const float* w_inst, const float* w_det, int num_classes,
                           const int64_t* labels, const float* grad_inst, const float* grad_det, float* grad_x,
                           int accumulate_x, long long* grad_w_inst_fx, long long* grad_b_inst_fx,
                           long long* grad_w_det_fx, long long* grad_b_det_fx, dm_stream_t stream);
int dm_point_sample_bwd_fx(const float* grad_out, int B, int C, int H, int W, const float* rois, int N, int S,
                           float spatial_scale, long long* grad_feat_fx, dm_stream_t stream);
int dm_fx_to_float(long long* fx, long long n, float* out, int accumulate, int clear, dm_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * K21  RefineMask: 3x3 convolutions with a dilation, on maps of any width (csrc/conv_dilated.hip), and a sigmoid.
 * replaces: ConvModule(3x3, padding = dilation = d) of refine_mask_head.py -- the semantic_convs on the whole stride-4
 *           FPN map (d = 1) and MultiBranchFusion's dilation_conv_{1,2,3} (d = 1, 3, 5; refine_mask_head.py:17-33).
 * x [NB, C, H, W]; w_packed: dm_conv_pack_weight(ksize = 3, one source) of the [Cout, C, 3, 3] weight (the layout
 * dm_conv2d_fwd reads); bias [Cout] or NULL; out [NB, Cout, H, W].  Exact fp32 (v_mfma_f32_32x32x2_f32) only.
 * flags: bit 0 ReLU; bit 2 ADD: out = out + v, where v is the value the call would otherwise store (i.e. after the
 * ReLU -- NOT dm_conv2d_fwd's bit 1, which adds before the ReLU and is refused here with DM_ERR_INVALID_ARG); bit 3 is
 * accepted and ignored; bit 4 (the bf16x3 layout) returns DM_ERR_UNSUPPORTED.
 * dm_conv3x3_dil_supported: 1 exactly when NB >= 1, C >= 8 with C % 8 == 0, H >= 1, W >= 1 (no upper bound on
 * either: a workgroup stages an 8 x 16 pixel block plus a halo of d), Cout >= 1, 1 <= dilation <= 8, and the grid
 * (NB * ceil(H / 8) * ceil(W / 16) pixel blocks times ceil(roundup(Cout, 32) / (Cout <= 64 ? 64 : 128)) cout tiles)
 * has at most 2^31 - 1 workgroups.  dm_conv3x3_dil_fwd returns DM_ERR_UNSUPPORTED for anything else.
 * ------------------------------------------------------------------------------------------------------------------ */
int dm_conv3x3_dil_supported(int NB, int C, int H, int W, int Cout, int dilation);
int dm_conv3x3_dil_fwd(const float* x, int NB, int C, int H, int W, const float* w_packed, const float* bias, int Cout,
                       int dilation, int flags, float* out, dm_stream_t stream);
/* MultiBranchFusion's branch sum in ONE launch: out (+)= sum_b act(conv3x3_{dilations[b]}(x, w_packed[b]) + bias[b]),
 * act = ReLU when flag bit 0 is set.  w_packed / bias / dilations: host arrays of num_branches entries (bias may be NULL,
 * or hold NULL entries).  The branches are added as ((t_0 + t_1) + t_2): bit for bit what three dm_conv3x3_dil_fwd
 * calls give, the second and third with bit 2.  Flags as dm_conv3x3_dil_fwd.  dm_conv3x3_multidil_supported: 1 exactly
 * when num_branches == 3, every dilation is in [1, 8] and dm_conv3x3_dil_supported accepts the shape. */
int dm_conv3x3_multidil_supported(int NB, int C, int H, int W, int Cout, int num_branches, const int* dilations);
int dm_conv3x3_multidil_fwd(const float* x, int NB, int C, int H, int W, const float* const* w_packed,
                            const float* const* bias, int Cout, int num_branches, const int* dilations, int flags,
                            float* out, dm_stream_t stream);
/* out[i] = 1 / (1 + exp(-x[i])) for i < n (the paste kernels' logistic, bit for bit): RefineMask's sigmoid(semantic_pred)
 * (refine_mask_head.py:115-117), n = B * H * W.  out may equal x. */
int dm_sigmoid_fwd(const float* x, long long n, float* out, dm_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * K22  PointRend inference: the subdivision step of PointRendRoIHead._mask_point_forward_test
 * (mmdet/models/roi_heads/point_rend_roi_head.py:96-128) on the label channel of the refined map (csrc/point_refine.hip).
 *
 * dm_point_select: map [n, HW] (the label channel of the upsampled map) -> idx [n, P] int32: per row the P cells of
 * smallest |v| -- topk(-|v|, P) of MaskPointHead.get_roi_rel_points_test -- in ASCENDING index order.  Tie rule: among
 * cells of equal |v| at the cut, the lower flat index is taken (torch.topk promises no order).  |v| is compared as the
 * bit pattern of the magnitude (+0 and -0 are equal; a NaN ranks above +inf, i.e. is never preferred).
 * dm_point_select_supported: 1 exactly when n >= 0, 1 <= HW <= 2^24 and 1 <= P <= HW.  n == 0 enqueues nothing.
 * ------------------------------------------------------------------------------------------------------------------ */
int dm_point_select_supported(int n, int HW, int P);
int dm_point_select(const float* map, int n, int HW, int P, int* idx, dm_stream_t stream);
/* dm_point_gather_fwd: for every RoI r and selected cell idx[r, p] of an MH x MW grid, the cell centre
 * (px, py) = (w_step / 2 + col * w_step, h_step / 2 + row * h_step), w_step = (float)(1.0 / MW) (get_roi_rel_points_test's
 * fp32 chain), and
 *   out[r, c, p]      = point_sample(feat[rois[r, 0]], rel_roi_point_to_rel_img_point(rois[r], (px, py), (H, W),
 *                       spatial_scale))[c]    for c < C  (abs = rel * (x2 - x1) + x1, then abs / W * spatial_scale),
 *   out[r, C + k, p]  = point_sample(coarse[r], (px, py))[k]   for k < NC  (the RoI's CH x CW coarse logits),
 * point_sample = mmcv's: grid_sample(bilinear, zeros, align_corners=False) at 2 * point - 1, in the fp32 operations of
 * PyTorch's CPU grid sampler.  feat [B, C, H, W]; rois [n, 5] (batch index, x1, y1, x2, y2; a batch index outside
 * [0, B) gives zero fine channels); coarse [n, NC, CH, CW]; idx [n, P] in [0, MH * MW); out [n, C + NC, P].
 * dm_point_gather_supported: 1 exactly when B >= 1, C >= 8 and NC >= 8 are multiples of 8, H, W, CH, CW, MH, MW >= 1,
 * MH * MW < 2^31, n >= 0, 1 <= P <= MH * MW and ceil(n * P / 256) < 2^31. */
int dm_point_gather_supported(int B, int C, int H, int W, int n, int NC, int CH, int CW, int P, int MH, int MW);
int dm_point_gather_fwd(const float* feat, int B, int C, int H, int W, const float* rois, int n, const float* coarse,
                        int NC, int CH, int CW, const int* idx, int P, int MH, int MW, float spatial_scale, float* out,
                        dm_stream_t stream);
/* dm_point_mlp_fwd: MaskPointHead.forward (mask_point_head.py:85-104, coarse_pred_each_layer) on x [n, C + NC, P]
 * (dm_point_gather_fwd's layout): h_0 = x[:, :C], h_{l+1} = relu(W_l [h_l; x[:, C:]] + b_l) for l < num_fcs, then
 * v = w_logits[label] . [h; x[:, C:]] + b_logits[label] and refined[r, idx[r, p]] = v (the scatter_ of
 * point_rend_roi_head.py:121-124, label channel only).  w_packed[l]: dm_conv_pack_weight(ksize 1, Cin = C + NC, one
 * source) of the [F, C + NC] weight; bias[l] [F] (the host array, or an entry, may be NULL); w_logits [NCL, C + NC],
 * b_logits [NCL] or NULL; labels [n] int64, clamped to [0, NCL - 1] (NCL = 1: class-agnostic); refined [n, HW].
 * Exact fp32 (v_mfma_f32_32x32x2_f32 for the layers, fmaf for the logit row).  flags: bit 3 accepted and ignored; bit 4
 * (the bf16x3 mode) returns DM_ERR_UNSUPPORTED; any other bit DM_ERR_INVALID_ARG.
 * dm_point_mlp_supported: 1 exactly when n >= 0, 1 <= P <= HW, C == F == 256, 8 <= NC <= 96 with NC % 8 == 0,
 * 1 <= num_fcs <= 4, NCL >= 1 and n * ceil(P / 64) < 2^31. */
int dm_point_mlp_supported(int n, int P, int C, int NC, int F, int num_fcs, int NCL, int HW);
int dm_point_mlp_fwd(const float* x, int n, int P, int C, int NC, int F, int num_fcs, const float* const* w_packed,
                     const float* const* bias, const float* w_logits, const float* b_logits, int NCL,
                     const long long* labels, const int* idx, int flags, float* refined, int HW, dm_stream_t stream);
/* map[r, idx[r, p]] = vals[r, p] for r < n, p < P (the unfused sequence's scatter); vals [n, P], idx [n, P] in [0, HW),
 * map [n, HW].  DM_ERR_UNSUPPORTED unless n >= 0 and 1 <= P <= HW. */
int dm_point_scatter(const float* vals, const int* idx, int n, int P, float* map, int HW, dm_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * K23  Mask Scoring R-CNN inference: MaskIoUHead (mmdet/models/roi_heads/mask_heads/maskiou_head.py) behind the mask
 * branch of MaskScoringRoIHead.simple_test_mask (mask_scoring_roi_head.py:58-90), csrc/conv_strided.hip.
 *
 * dm_conv3x3_s2_fwd: the IoU head's last conv, Conv2d(C, Cout, 3, stride = 2, padding = 1) + bias (+ ReLU).
 * x [NB, C, H, W]; w_packed: dm_conv_pack_weight(ksize = 3, one source) of the [Cout, C, 3, 3] weight (the layout
 * dm_conv2d_fwd reads); bias [Cout] or NULL; out [NB, Cout, ceil(H / 2), ceil(W / 2)].  Exact fp32
 * (v_mfma_f32_32x32x2_f32) only.  splits: how many workgroups share a tile's K loop -- 1, 2, 4 or 8 (at most C / 8), or 0:
 * the library's choice (the smallest that puts two workgroups on every CU).  With more than one split the partial sums go
 * to `workspace` (dm_conv3x3_s2_workspace_floats() floats; may be NULL when that is 0) and a second launch adds them in
 * split order, then the bias: the same bits every run, which differ between split counts in rounding only.
 * flags: bit 0 ReLU; bit 3 accepted and ignored; bit 4 (the bf16x3 layout) returns DM_ERR_UNSUPPORTED; any other bit
 * DM_ERR_INVALID_ARG.  A workspace smaller than needed: DM_ERR_INVALID_ARG.
 * dm_conv3x3_s2_supported: 1 exactly when NB >= 1, C >= 8 with C % 8 == 0, H >= 1, W >= 1, Cout >= 1, splits is 0 or
 * one of 1, 2, 4, 8 not above C / 8, and the grid (ceil(NB * ceil(H / 2) * ceil(W / 2) / 64) pixel tiles times
 * ceil(roundup(Cout, 32) / (Cout <= 64 ? 64 : 128)) cout tiles times the resolved split count) has at most 2^31 - 1
 * workgroups.  dm_conv3x3_s2_fwd returns DM_ERR_UNSUPPORTED for anything else; dm_conv3x3_s2_workspace_floats -1.
 * ------------------------------------------------------------------------------------------------------------------ */
int dm_conv3x3_s2_supported(int NB, int C, int H, int W, int Cout, int splits);
long long dm_conv3x3_s2_workspace_floats(int NB, int C, int H, int W, int Cout, int splits);
int dm_conv3x3_s2_fwd(const float* x, int NB, int C, int H, int W, const float* w_packed, const float* bias, int Cout,
                      int splits, int flags, float* out, float* workspace, long long workspace_floats, dm_stream_t stream);
/* dm_mask_iou_input: max_pool2d(sigmoid(mask_pred[i, c_i]), 2, 2) -> out [n, 1, H / 2, W / 2] (floor), the IoU head's
 * second input (maskiou_head.py:80-81).  mask_pred [n, C, H, W] logits; c_i = labels[i] (int64) clamped to [0, C - 1],
 * 0 when C == 1 (labels may then be NULL).  The sigmoid is the paste kernels' expression; the window's maximum follows
 * max_pool2d (row-major, a later element wins when larger or NaN).  dm_mask_iou_input_supported: 1 exactly when n >= 0,
 * C >= 1, H >= 2 and W >= 2.  n == 0 enqueues nothing. */
int dm_mask_iou_input_supported(int n, int C, int H, int W);
int dm_mask_iou_input(const float* mask_pred, int n, int C, int H, int W, const long long* labels, float* out,
                      dm_stream_t stream);
/* dm_mask_iou_scores: out[i] = mask_iou_pred[i, c_i] * dets[i, D - 1] (MaskIoUHead.get_mask_scores, one fp32 product);
 * mask_iou_pred [n, NC], labels [n] int64 clamped to [0, NC - 1], dets [n, D] (the detections with their score last).
 * DM_ERR_UNSUPPORTED unless n >= 0, NC >= 1 and D >= 1.  n == 0 enqueues nothing. */
int dm_mask_iou_scores(const float* mask_iou_pred, int n, int NC, const long long* labels, const float* dets, int D,
                       float* out, dm_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * K24  PointRefine inference: one SFMStage of mmdet/models/roi_heads/mask_heads/mask_point_refine.py (:95-132) on the
 * stage features f [n, C, S, S], csrc/point_refine.hip.  Exact fp32 in every precision mode.  A NULL idx means every
 * cell in order (P == S * S): the selection is skipped, and the MLP is per point, so the order does not matter.
 *
 * dm_point_topk_select: map [n, HW] (the label row of the detail logits) -> idx [n, P] int32: per row the P cells of
 * LARGEST key (get_roi_rel_points_train's topk), key = 1 / (1 + expf(-v)) (mode 1, mask_use_sigmoid; the paste kernels'
 * sigmoid, so saturated cells tie at 1.0f) or v (mode 0); indices in ascending order; among cells of equal key at the
 * cut, the lower flat index is taken (keys are equal when they compare equal as floats: +0 and -0 are one key).
 * dm_point_topk_select_supported: 1 exactly when mode is 0 or 1 and
 * dm_point_select_supported(n, HW, P).  n == 0 enqueues nothing.
 * ------------------------------------------------------------------------------------------------------------------ */
int dm_point_topk_select_supported(int n, int HW, int P, int mode);
int dm_point_topk_select(const float* map, int n, int HW, int P, int mode, int* idx, dm_stream_t stream);
/* dm_point_feat_gather: the point MLP's input out [n, C + NC, P]: for the cell c = idx[r, p] (c = p when idx is NULL)
 * of the S x S grid, out[r, ch, p] for ch < C is dm_point_gather_fwd's fine channel (same expressions, equal within
 * rounding: point_sample of feat[rois[r, 0]]
 * [B, C, H, W] at rel_roi_point_to_rel_img_point of the cell centre, spatial_scale), and out[r, C + k, p] =
 * coarse[r, k, c] exactly (torch.gather of the [n, NC, S * S] logit maps).  dm_point_feat_gather_supported: 1 exactly when
 * B >= 1, C >= 8 and NC >= 8 are multiples of 8, (C + NC) / 8 <= 65535, H, W, S >= 1, S * S < 2^31, n >= 0,
 * 1 <= P <= S * S (P == S * S without idx) and ceil(n * P / 256) < 2^31. */
int dm_point_feat_gather_supported(int B, int C, int H, int W, int n, int NC, int P, int S, int has_idx);
int dm_point_feat_gather(const float* feat, int B, int C, int H, int W, const float* rois, int n, const float* coarse,
                         int NC, const int* idx, int P, int S, float spatial_scale, float* out, dm_stream_t stream);
/* dm_point_refine_mlp: SFMStage's point MLP (coarse_pred_each_layer) on x [n, C + NC, P]: h_0 = x[:, :C],
 * h_{l+1} = relu(W_l [h_l; x[:, C:]] + b_l) for l < num_fcs, then v = W_L [h; x[:, C:]] + b_L (fc_logits, no ReLU) and
 * feat[r, :, idx[r, p]] = v[:, p] for all C rows.  w_packed[0 .. num_fcs]: dm_conv_pack_weight(ksize 1, Cin = C + NC, one
 * source) of the [C, C + NC] weights, fc_logits last; bias[0 .. num_fcs] (the host array, or an entry, may be NULL);
 * feat [n, C, HW].  Exact fp32 (v_mfma_f32_32x32x2_f32).  flags: bit 3 accepted and ignored; bit 4 (the bf16x3 mode)
 * returns DM_ERR_UNSUPPORTED; any other bit DM_ERR_INVALID_ARG.  dm_point_refine_mlp_supported: 1 exactly when n >= 0,
 * 1 <= P <= HW (P == HW without idx), C is 64, 128 or 256, 8 <= NC <= 160 with (C + NC) % 8 == 0,
 * 1 <= num_fcs <= 4 and n * ceil(P / 64) < 2^31. */
int dm_point_refine_mlp_supported(int n, int P, int C, int NC, int num_fcs, int HW, int has_idx);
int dm_point_refine_mlp(const float* x, int n, int P, int C, int NC, int num_fcs, const float* const* w_packed,
                        const float* const* bias, const int* idx, int flags, float* feat, int HW, dm_stream_t stream);
/* map[r, c, idx[r, p]] = vals[r, c, p] for r < n, c < C, p < P (the unfused sequence's scatter); vals [n, C, P], idx [n, P]
 * in [0, HW), map [n, C, HW].  DM_ERR_UNSUPPORTED unless n >= 0, C >= 1, 1 <= P <= HW and ceil(n * C * P / 256) < 2^31. */
int dm_point_scatter_rows(const float* vals, const int* idx, int n, int C, int P, float* map, int HW, dm_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * K25  Cascade Mask R-CNN inference (mmdet/models/roi_heads/cascade_roi_head.py:294-448).
 *
 * dm_conv2d_group_fwd: count (1..3) independent single-source "same" convolutions of ONE shape in ONE launch:
 * out[i] [NB, Cout, H, W] = act(conv_ksize(x[i] [NB, Cin, H, W], w_packed[i]) + bias[i]), ksize 1 or 3, weights packed by
 * dm_conv_pack_weight (one source); several x[i] may be the same pointer; bias (the host array, or an entry) may be NULL.
 * relu: bit 0 ReLU, bit 3 accepted and ignored; bit 4 (the bf16x3 layout) returns DM_ERR_UNSUPPORTED: the grouped launch is
 * exact fp32 only; any other bit DM_ERR_INVALID_ARG.  ksize 3 with 32 < Cout <= 36 (the tail build) is DM_ERR_UNSUPPORTED.
 * workspace (optional, workspace_floats of them): a 3x3 launch of few workgroups splits its K loop as dm_conv2d_fwd_ws
 * does, the split decided on the GROUPED workgroup count; dm_conv2d_group_splits gives the split count S of a call
 * (1: none).  Contract: out[i] has the bits of dm_conv2d_fwd_ws(x[i], ...) given a workspace of S * NB * Cout * H * W
 * floats (S = 1: of dm_conv2d_fwd).  dm_conv2d_group_splitk_floats: the workspace that lets the call split as far as it
 * would (0: it would not).  NB == 0 enqueues nothing.
 *
 * dm_conv2d_group_plan: the launch dm_conv2d_group_fwd would make for these HOST arguments, reported by the launcher itself
 * as dm_conv2d_plan reports a lone call's (the same code with a recorder: nothing is launched, no device is needed).
 * records: HOST array of max_records (>= DM_CONV_GROUP_PLAN_MAX) x DM_CONV_PLAN_INTS ints.  Returns the number of records --
 * `count`, ONE PER PROBLEM of the one launch, in dm_conv2d_plan's layout: grid x is that problem's share of the grid, grid
 * y / ksplit / kchunks the split all problems share, q_begin 0 -- 0 for NB = 0, or the error code the call would return,
 * and then writes nothing.
 *
 * dm_deconv2x2_group_fwd: count (1..3) dm_deconv2x2_fwd problems of one shape in one launch (weights of
 * dm_deconv_pack_weight; relu bit 0 ReLU, bit 4 DM_ERR_UNSUPPORTED); each out[i] has the bits of its dm_deconv2x2_fwd.
 *
 * dm_cascade_refine: one cascade stage boundary, one wave per RoI row i < n:
 *   score_sum[i, :] = (first_stage ? 0 : score_sum[i, :]) + cls_score[i, :]   ([n, NC + 1]; sum(ms_scores) in fp32);
 *   label = the first maximum of cls_score[i, :NC] (torch argmax: NaN is the maximum);
 *   out_rois[i] = [rois[i, 0], delta2bbox(rois[i, 1:5], d)] clipped to img_shapes[rois[i, 0]] = (h, w), where d is
 *   bbox_pred[i, 0:4] (class_agnostic, [n, 4]) or bbox_pred[i, 4 label : 4 label + 4] ([n, 4 NC]): regress_by_class
 *   with the same decode as dm_bbox_decode (means, stds, wh_ratio_clip).  The image index is clamped to
 *   [0, num_images - 1].  score_sum NULL: no sum; out_rois NULL: the sum only (the last stage; rois / bbox_pred unread).
 *   out_rois may not be rois.  n == 0 enqueues nothing.
 * ------------------------------------------------------------------------------------------------------------------ */
int dm_conv2d_group_splits(int count, int NB, int H, int W, int Cin, int Cout, int ksize, long long workspace_floats);
long long dm_conv2d_group_splitk_floats(int count, int NB, int H, int W, int Cin, int Cout, int ksize);
int dm_conv2d_group_fwd(int count, const float* const* x, int NB, int H, int W, int Cin, int Cout, int ksize,
                        const float* const* w_packed, const float* const* bias, int relu, float* const* out, float* workspace,
                        long long workspace_floats, dm_stream_t stream);
#define DM_CONV_GROUP_PLAN_MAX 3
int dm_conv2d_group_plan(int count, int NB, int H, int W, int Cin, int Cout, int ksize, int relu, long long workspace_floats,
                         int* records, int max_records);
int dm_deconv2x2_group_fwd(int count, const float* const* x, int NB, int C, int H, int W, const float* const* w_packed,
                           const float* const* bias, int Cout, int relu, float* const* out, dm_stream_t stream);
int dm_cascade_refine(const float* rois, const float* cls_score, const float* bbox_pred, int n, int num_classes,
                      int class_agnostic, const float* means, const float* stds, float wh_ratio_clip, const float* img_shapes,
                      int num_images, float* score_sum, int first_stage, float* out_rois, dm_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * K26  Hybrid Task Cascade inference (mmdet/models/roi_heads/htc_roi_head.py, mask_heads/fused_semantic_head.py,
 *      mask_heads/htc_mask_head.py).  All exact fp32, deterministic.
 *
 * dm_resize_bilinear_fwd: F.interpolate(size=(OH, OW), mode='bilinear', align_corners=True) of in [NC, H, W] ->
 * out [NC, OH, OW], up or down, no antialiasing (fused_semantic_head.py:91-92).  Source coordinate of output o along
 * an axis: o * ((in - 1) / (out - 1)), the factor computed in fp32 and 0 when out == 1; low tap floor(.), high tap low + 1
 * clamped to in - 1.  At OH = 2 H, OW = 2 W the bits are dm_upsample2x_bilinear_fwd(align_corners = 1)'s.
 *
 * dm_conv2d_post_add_fwd: out = addend + act(conv(srcs) + bias) -- the addend joins AFTER the activation (dm_conv2d_fwd's
 * accumulate flag gives act(out + conv + bias)): FusedSemanticHead's lateral sum x += relu(conv1x1(resized level))
 * (fused_semantic_head.py:93) and HTCMaskHead's x = mask_feats + relu(conv_res(res_feat)) (htc_mask_head.py:28-30).
 * Arguments as dm_conv2d_fwd's; addend has out's layout (channels [out_ch_offset, out_ch_offset + Cout) of
 * [NB, out_ch_total, H, W]) and may be out itself; no source may overlap out.  relu: bit 0 only (any other bit
 * DM_ERR_INVALID_ARG); ksize 3 and the bf16x3 layout: DM_ERR_UNSUPPORTED.  The launch is dm_conv2d_fwd's launch of the
 * shape with one more epilogue step: every output has the bits of dm_conv2d_fwd followed by an fp32 add.
 *
 * dm_roi_align_add_fwd: RoIAlign (aligned, avg, dm_roi_align_fwd's arithmetic with num_levels == 1: no level mapping) of
 * ONE map feat [B, C, H, W] at P x P bins per RoI, added into RoI features without the [N, C, P, P] intermediate
 * (htc_roi_head.py:170-176 for the box branch, :339-342 / :137-141 for the mask branch):
 *   pool == 1: out [N, C, P, P]         out[n, c, y, x] += bin(n, c, y, x)   -- the bits of the extraction + an fp32 add,
 *              the extraction being dm_roi_align_fwd_ws with the workspace it asks for where that call orders the RoIs
 *              (P * P >= 128, DM_ROI_SORT_MIN <= N <= 1024), else dm_roi_align_fwd: the launch takes that call's channels
 *              per workgroup (the launcher asks its own forward route: dm_roi_align_plan entry 1 against entry 0), because
 *              bins of sampling grids above 4 x 4 differ in the last bit between the two;
 *   pool == 2: out [N, C, P / 2, P / 2]  out[n, c, y, x] += ((b00 + b01) + (b10 + b11)) * 0.25 of the 2 x 2 block of bins
 *              (adaptive_avg_pool2d P -> P / 2, P even): bin averages first, then the block mean, then the add.
 * rois [N, 5] as dm_roi_align_fwd's (the batch column picks the image of feat; an index outside [0, B) adds zeros).
 * P * P <= 256, P >= 2, C % 4 == 0 and H * W <= 2^23, else DM_ERR_UNSUPPORTED; N == 0 enqueues nothing.
 * ------------------------------------------------------------------------------------------------------------------ */
int dm_resize_bilinear_fwd(const float* in, long long NC, int H, int W, int OH, int OW, float* out, dm_stream_t stream);
int dm_conv2d_post_add_fwd(const float* const* srcs, const int* src_channels, const long long* src_batch_strides,
                           int num_srcs, int NB, int H, int W, const float* w_packed, const float* bias, int Cout,
                           int ksize, int relu, const float* addend, float* out, int out_ch_total, int out_ch_offset,
                           dm_stream_t stream);
int dm_roi_align_add_fwd(const float* feat, int B, int C, int H, int W, float spatial_scale, const float* rois, int N,
                         int P, int sampling_ratio, int pool, float* out, dm_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * K27  Grid R-CNN inference: GridHead (mmdet/models/roi_heads/mask_heads/grid_head.py:151-187, :294-359),
 *      csrc/grid_head.hip.  All exact fp32 in every precision mode, one fixed summation order, no atomics: the same bits
 *      on every run, and a sample's result does not depend on the other samples of the call.
 *
 * dm_group_norm_fwd: y = GroupNorm(G groups, eps, per-channel gamma / beta)(x) (+ ReLU when relu == 1) of x [N, C, H, W];
 * biased variance; y may be x (in place).  The statistics are two passes over the group on values shifted by its first
 * element (never E[x^2] - E[x]^2): a constant group gives exactly beta.  dm_group_norm_supported: 1 exactly when N >= 0,
 * C, G, H, W >= 1, C % G == 0, (C / G) * H * W <= 2^24 and N * G < 2^31.  N == 0 enqueues nothing; relu other than 0 / 1
 * or eps <= 0: DM_ERR_INVALID_ARG.  Two builds, one contract: groups of up to 16384 floats (every group of the Grid head)
 * run 256 threads a group with scalar loads; from a host constant above that (csrc/grid_head.hip GN_WIDE_MIN_L, chosen by
 * measurement) a group runs 1024 threads with 16-byte loads on its aligned middle -- the groups of a dense head's towers
 * (FCOSHead: 8 x 100 x 168 floats).  They associate the same sums differently (a rounding apart); each gives the same bits
 * on every run, and a sample's bits do not depend on the batch.  DM_GN_WIDE=0 runs the first for every length.
 *
 * dm_grid_fusion_fwd: one order of the neighbour fusion (grid_head.py:157-170) in one launch.  x, src, out
 * [N, P * c, S, S] (point i = channels [i c, (i + 1) c)); for every sample and point i
 *   out_i = x_i + sum_j (W1_ij * dw5x5_ij(src_{nb(i, j)}) + b1_ij),
 * dw5x5 the depthwise 5 x 5 convolution (padding 2) with its bias, W1 the 1x1 convolution c -> c, nb(i, j) the j-th
 * neighbour of point i = column * sqrt(P) + row in the reference's order (left, up, down, right: grid_head.py:88-102), the
 * terms added in that order.  First order: src = x; second order: src = the first order's out.  out may be neither x nor
 * src.  table: [P][4][E] floats, E = 25 c + c + c c + c, slot (i, j) = [dw weight [c][25]][dw bias [c]][W1 transposed
 * [k][o]][b1 [c]]; slots past a point's neighbour count are not read.  dm_grid_fusion_table_floats: P * 4 * E (-1 for an
 * unsupported P, c).  dm_grid_fusion_supported: 1 exactly when N >= 0, P is 4 or 9, c is 8 or 64, S is 3 or 7.
 *
 * dm_deconv4x4_s2_grouped_fwd: ConvTranspose2d(G ci, G co, kernel 4, stride 2, padding 1, groups = G) + bias:
 * x [N, G ci, S, S], w [G ci, co, 4, 4] (torch's layout), bias [G co] or NULL, out [N, G co, 2 S, 2 S].  Four output
 * phases of 2 x 2 taps each.  dm_deconv4x4_s2_grouped_supported: 1 exactly when N >= 0, G is 4 or 9, ci is 8 or 64,
 * co is 1, 8 or 64 and S is 1, 3, 7 or 14.
 *
 * dm_grid_get_bboxes: GridHead.get_bboxes on the device.  heat [n, P, HS, HS] logits, det [n, D] (x1, y1, x2, y2, ...,
 * score last), sub_x / sub_y: HOST arrays of P ints (calc_sub_regions' x1, y1 per point), out [n, 5].  Per (sample,
 * point): the maximum of sigmoid(heat) (the paste kernels' expression) and its FIRST cell among equal sigmoid values --
 * not the argmax of the logits: saturated cells tie -- then, one fp32 rounding per operation as in the reference:
 * xs = cell % HS + sub_x, ys = cell / HS + sub_y; abs = (xs + 0.5) / HS * width + (x1 - width / 2) on the box expanded by
 * half its size each side; each box side = sum(abs * score) / sum(score) over the sqrt(P) points of that side;
 * out[:, 4] = det[:, D - 1]; cells (int32 [n, P], may be NULL) receives each point's cell.  The box is NOT clipped to the image (the reference clamps a copy).
 * dm_grid_get_bboxes_supported: 1 exactly when n >= 0, P is 4 or 9, 1 <= HS <= 1024 and D >= 5.  n == 0 enqueues nothing.
 * ------------------------------------------------------------------------------------------------------------------ */
int dm_group_norm_supported(long long N, int C, int G, int H, int W);
int dm_group_norm_fwd(const float* x, long long N, int C, int G, int H, int W, const float* gamma, const float* beta,
                      float eps, int relu, float* y, dm_stream_t stream);
int dm_grid_fusion_supported(int N, int P, int c, int S);
long long dm_grid_fusion_table_floats(int P, int c);
int dm_grid_fusion_fwd(const float* x, const float* src, int N, int P, int c, int S, const float* table, float* out,
                       dm_stream_t stream);
int dm_deconv4x4_s2_grouped_supported(int N, int G, int ci, int co, int S);
int dm_deconv4x4_s2_grouped_fwd(const float* x, int N, int G, int ci, int co, int S, const float* w, const float* bias,
                                float* out, dm_stream_t stream);
int dm_grid_get_bboxes_supported(int n, int P, int HS, int D);
int dm_grid_get_bboxes(const float* heat, int n, int P, int HS, const float* det, int D, const int* sub_x, const int* sub_y,
                       float* out, int* cells, dm_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * K28  Double-Head R-CNN inference (mmdet/models/roi_heads/double_roi_head.py, bbox_heads/double_bbox_head.py).  The
 *      head's convolutions are dm_conv2d_fwd launches (BatchNorm in eval mode folded into weights and bias on the host),
 *      its fully connected layers dm_fc_fwd; these two entry points are what it adds.  Exact fp32, deterministic.
 *
 * dm_roi_align_scaled_fwd: dm_roi_align_fwd with the RoIs rescaled about their centres by roi_scale_factor
 * (base_roi_extractor.py:57-80) AFTER the level map (single_level_roi_extractor.py:69-71): the FPN level -- and
 * levels_out -- is the box's as given; the samples are those of
 *   cx = (x1 + x2) * 0.5, w = x2 - x1, new_w = w * roi_scale_factor, x1' = cx - new_w * 0.5, x2' = cx + new_w * 0.5
 * (the same in y), one fp32 rounding per operation: per RoI the bits of dm_roi_align_fwd with num_levels == 1 on that
 * level's map and the box rescaled on the host.  roi_scale_factor == 1 skips the rescale: dm_roi_align_fwd's bits.
 * roi_scale_factor <= 0 (or not finite): DM_ERR_INVALID_ARG.  No workspace form: the RoIs are walked in their own order.
 *
 * dm_global_avg_pool_fwd: out [N, C] = the mean of every plane of x [N, C, HW] (nn.AvgPool2d(S) on an S x S map).  One
 * wave per plane: lane l adds the elements l, l + 64, ... in order, a xor butterfly adds the 64 partial sums, one division
 * by HW -- an order fixed by HW alone: a sample's bits do not depend on the other samples of the call.
 * dm_global_avg_pool_supported: 1 exactly when N >= 0, C >= 1, 1 <= HW <= 2^24 and N * C < 2^31.  N == 0 enqueues nothing.
 * ------------------------------------------------------------------------------------------------------------------ */
int dm_roi_align_scaled_fwd(const float* const* feats, const int* H, const int* W, const float* spatial_scales,
                            int num_levels, int B, int C, const float* rois, int N, int P, int sampling_ratio,
                            float finest_scale, float roi_scale_factor, float* out, int32_t* levels_out, dm_stream_t stream);
int dm_global_avg_pool_supported(int N, int C, int HW);
int dm_global_avg_pool_fwd(const float* x, int N, int C, int HW, float* out, dm_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * K29  Mask R-CNN / Faster R-CNN C4 inference (configs/_base_/models/{mask,faster}_rcnn_r50_caffe_c4.py): the shared
 *      head (ResNet layer4 per RoI, roi_heads/shared_heads/res_layer.py) is nine dm_conv2d_fwd launches with eval-mode
 *      BatchNorm folded on the host, the plain BBoxHead dm_global_avg_pool_fwd + dm_fc_fwd.  With style='caffe' the
 *      stride of layer4 sits in two 1x1 convolutions that read only the even rows and columns of the 14 x 14 RoI
 *      features; this entry point produces only those bins.
 *
 * dm_roi_align_strided_fwd: the arguments of dm_roi_align_fwd and bin_step >= 1.  out [N, C, Po, Po], Po = ceil(P / bin_step):
 * out[n, c, i, j] is bin (i * bin_step, j * bin_step) of the P x P extraction of RoI n, and no other bin is sampled or
 * stored (no [N, C, P, P] intermediate).  A kept bin has the samples, products and summation order of dm_roi_align_fwd
 * without a workspace (the tile kernel at 16 channels per workgroup): its bits do not depend on N, on the other RoIs of
 * the call or on the DM_ROI_SORT* knobs.  The RoIs are walked in their own order.  levels_out as the forward's.
 * dm_roi_align_strided_supported: 1 exactly where the call is taken: 1 <= num_levels <= 4, every map non-empty and of
 * at most 2^23 pixels, C % 4 == 0, 2 <= P, P * P <= 256 (where dm_roi_align_fwd takes its tile kernel) and
 * 1 <= bin_step <= P.  Anything else: DM_ERR_UNSUPPORTED (bin_step < 1: DM_ERR_INVALID_ARG).  N == 0 enqueues nothing.
 * dm_roi_align_plan reports the launch under entry 3, with bin_step in `pool`: one record, kernel 1 with MODE 3 and
 * bin_step as its parameters, CT 16, levels 1; it takes no workspace.
 * ------------------------------------------------------------------------------------------------------------------ */
int dm_roi_align_strided_supported(int num_levels, const int* H, const int* W, int C, int P, int bin_step);
int dm_roi_align_strided_fwd(const float* const* feats, const int* H, const int* W, const float* spatial_scales,
                             int num_levels, int B, int C, const float* rois, int N, int P, int sampling_ratio,
                             float finest_scale, int bin_step, float* out, int32_t* levels_out, dm_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * K30  RPN inference: the post-processing of RPNHead.get_bboxes (mmdet/models/dense_heads/rpn_head.py:79-168,
 *      anchor_head.py:500-576), csrc/rpn.hip.  The head's convolutions are dm_conv2d_fwd launches, the suppression
 *      dm_nms_mask_segmented + dm_nms_reduce_segmented; these entry points are what lies between and after.  Exact
 *      fp32, integer arithmetic only after the scores, no atomics on floats: the same bits on every run.
 *
 * A SEGMENT is one (image, level).  All three entry points read one device table seg_tab [S][DM_RPN_SEG_WORDS] of 64-bit
 * words, segment s = image * L + level:
 *    0 logits   address of the segment's [A, H, W] logits (dense NCHW block), as rpn_cls writes them
 *    1 deltas   address of its [4 A, H, W] deltas, as rpn_reg writes them
 *    2 A  3 H  4 W
 *    5 rows     K = min(nms_pre, A H W), or A H W when nms_pre <= 0: the segment's rows of idx / score / boxes
 *    6 key_off  the sum of A H W over the segments before it
 *    7 row0     the sum of `rows` over the segments before it
 *    8 base_row the level's first row in base_anchors   9 stride_x   10 stride_y   11 image
 * Candidate i = (h * W + w) * A + a is the reference's permute(1, 2, 0).reshape(-1) order.
 *
 * dm_rpn_select: per segment, the K candidates of largest key in descending key order, the lower i first among equal
 * keys; key = 1 / (1 + expf(-logit)), the expression of dm_sigmoid_fwd (saturated logits tie as they do there; a NaN
 * sorts first).  idx[row0 + r] = i and score[row0 + r] = key of rank r: bit for bit
 * torch.sort(sigmoid(permuted logits), descending=True, stable=True) cut at K.  A segment is cut into chunks of
 * DM_RPN_SELECT_CHUNK candidates, one workgroup each; the last pass ranks the K survivors by counting (K^2 / 256
 * comparisons per workgroup of 256 survivors).  workspace: dm_rpn_select_workspace_bytes bytes, 8-byte aligned,
 * contents undefined before and after.  max_candidates / total_candidates: the largest and the sum of A H W;
 * total_rows: the sum of `rows`.
 * dm_rpn_select_supported: 1 exactly when 0 <= num_segments <= 65535, 0 <= max_candidates <= 2^20 and
 * 0 <= total_candidates <= num_segments * max_candidates; else DM_ERR_UNSUPPORTED.  No segment or no candidate
 * enqueues nothing; an empty segment among others enqueues nothing for itself.
 *
 * dm_rpn_decode: boxes[row0 + r] = delta2bbox(anchor, deltas) clipped to the image, for every row r < rows of every
 * segment: anchor = base_anchors[base_row + a] + (w stride_x, h stride_y, w stride_x, h stride_y) (the integer product
 * converted to fp32, one fp32 add per coordinate: single_level_grid_anchors), deltas = channels 4a .. 4a + 3 at (h, w),
 * i = idx[row0 + r]; the device function of dm_bbox_decode with the coder's means / stds / wh_ratio_clip, clipped to
 * img_shapes[image] = (h, w) when w > 0: bit for bit dm_bbox_decode (class agnostic, no scores, scale 1) on the
 * materialised anchors and gathered deltas.  An idx outside [0, A H W) gives a zero box.
 * dm_rpn_decode_supported: 1 exactly when 0 <= num_segments <= 65535, 0 <= max_rows <= 2^20 and num_images >= 1.
 * max_rows: the largest `rows`.  No segment or no row enqueues nothing.
 *
 * dm_rpn_merge: per image, the first nms_post of the union of its L kept lists in descending score order; equal scores:
 * the lower level first, then the earlier rank (a NaN first; -0 == +0): bit for bit the concatenation of the kept rows
 * and a stable descending sort cut at nms_post.  keep / kept as dm_nms_reduce_segmented leaves them for the same
 * segments (keep[row0 + k] = the k-th kept row within the segment's rows, kept[s] their number); boxes [total rows, 4],
 * score [total rows].  out [B, nms_post, 5] = (box, score), rows past counts[b] untouched; counts[b] =
 * min(kept of the image, nms_post).
 * dm_rpn_merge_supported: 1 exactly when 0 <= num_images <= 65535, 1 <= num_levels <= 64, 0 <= max_rows <= 2^20 and
 * nms_post >= 1.  num_images == 0 enqueues nothing.
 * ------------------------------------------------------------------------------------------------------------------ */
#define DM_RPN_SEG_WORDS 12
#define DM_RPN_SELECT_CHUNK 4096
int dm_rpn_select_supported(int num_segments, int max_candidates, long long total_candidates);
long long dm_rpn_select_workspace_bytes(int num_segments, int max_candidates, long long total_candidates,
                                        long long total_rows);
int dm_rpn_select(const long long* seg_tab, int num_segments, int max_candidates, long long total_candidates,
                  long long total_rows, int nms_pre, void* workspace, long long workspace_bytes, int32_t* idx,
                  float* score, dm_stream_t stream);
int dm_rpn_decode_supported(int num_segments, int max_rows, int num_images);
int dm_rpn_decode(const long long* seg_tab, int num_segments, int max_rows, const int32_t* idx,
                  const float* base_anchors, const float* img_shapes, int num_images, const float* means,
                  const float* stds, float wh_ratio_clip, float* boxes, dm_stream_t stream);
int dm_rpn_merge_supported(int num_images, int num_levels, int max_rows, int nms_post);
int dm_rpn_merge(const long long* seg_tab, int num_images, int num_levels, int max_rows, const int32_t* keep,
                 const int32_t* kept, const float* boxes, const float* score, int nms_post, float* out, int32_t* counts,
                 dm_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * K31  FPN neck inference (mmdet/models/necks/fpn.py:164-216).  The lateral 1x1 convolutions are dm_conv2d_fwd launches
 *      (any Cin), the 3x3 level convolutions dm_conv2d_fwd / dm_conv3x3_dil_fwd (any width), the extra stride-2 ones
 *      dm_conv3x3_s2_fwd; these two entry points are what the neck adds.  Exact fp32, deterministic, no atomics.
 *
 * dm_conv2d_up_add_fwd: out[n, c, y, x] = addend[n, c, iy[y], ix[x]] + act(conv1x1(srcs) + bias) -- the top-down merge
 * laterals[i - 1] += F.interpolate(laterals[i], mode='nearest') (fpn.py:177-186) inside the lateral convolution of level
 * i - 1: the merged lateral is written once and the upsampled map never exists.  addend: a dense [NB, Cout, Hs, Ws]
 * tensor (the merged lateral above); iy [H] and ix [W]: DEVICE int32 tables with values in [0, Hs) and [0, Ws) -- the
 * source row / column of every output row / column (not checked on the device: a value outside reads outside addend).
 * addend may not overlap out.  Everything else as dm_conv2d_post_add_fwd: exact fp32 only, ksize == 1 only (3 and the
 * bf16x3 layout: DM_ERR_UNSUPPORTED), relu bit 0 only (any other bit DM_ERR_INVALID_ARG), no workspace and no K split,
 * and the tile build the plain launch of the shape takes (dm_conv2d_plan with has_addend reports it: POST 1 there stands
 * for either addend form).  Every output has the bits of dm_conv2d_fwd followed by one fp32 add of the gathered addend.
 * Hs, Ws <= 0, Hs * Ws >= 2^31 or a null addend / table: DM_ERR_INVALID_ARG.  NB == 0 enqueues nothing.
 *
 * dm_subsample2_fwd: out[nc, y, x] = in[nc, 2 y, 2 x], out [NC, ceil(H / 2), ceil(W / 2)] -- F.max_pool2d(x, 1, stride=2),
 * FPN's extra levels without extra convolutions (fpn.py:197-199).  Any H, W >= 1; NC == 0 enqueues nothing.
 * ------------------------------------------------------------------------------------------------------------------ */
int dm_conv2d_up_add_fwd(const float* const* srcs, const int* src_channels, const long long* src_batch_strides,
                         int num_srcs, int NB, int H, int W, const float* w_packed, const float* bias, int Cout,
                         int ksize, int relu, const float* addend, int Hs, int Ws, const int32_t* iy, const int32_t* ix,
                         float* out, int out_ch_total, int out_ch_offset, dm_stream_t stream);
int dm_subsample2_fwd(const float* in, long long NC, int H, int W, float* out, dm_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * K32  ResNet backbone inference (mmdet/models/backbones/resnet.py).  The stages are the launches that exist
 *      (dm_conv2d_fwd, dm_conv3x3_dil_fwd, dm_conv3x3_s2_fwd, dm_subsample2_fwd); these entry points are the stem.
 *      Exact fp32, deterministic, no atomics, no workspace.
 *
 * dm_conv7x7_s2_fwd: out = act(conv2d(x, w, stride = 2, padding = 3) + bias), x [NB, C, H, W], out
 * [NB, Cout, ceil(H / 2), ceil(W / 2)]; bias [Cout] or NULL.  w_packed: the [Cout, C, 7, 7] weight as the matrix
 * [Cout, C * 7 * 8] -- column (c * 7 + ky) * 8 + kx, the columns kx == 7 zero -- in dm_conv_pack_weight's layout for
 * ksize 1 and one source of C * 56 channels (dm_conv_packed_floats(Cout, 1, 1, {C * 56}) floats).  flags: bit 0 ReLU
 * (NaN stays NaN); bit 3 is accepted and ignored; bit 4 (the bf16x3 layout): DM_ERR_UNSUPPORTED; any other bit:
 * DM_ERR_INVALID_ARG.  The sum of an output runs over (c, ky) in order and, in a row, over kx = 0, 4, 1, 5, 2, 6, 3 as
 * one fp32 fma chain: it does not depend on NB, H, W, the output's position or which taps fall in the padding (those
 * multiply zeros), so an image's bits do not depend on the other images of the call.
 * dm_conv7x7_s2_supported: 1 exactly when NB >= 1, C == 3, 1 <= H, W, Cout <= 2^24 (any such Cout: the couts past a
 * multiple of 32 are dm_conv_packed_cout's padding) and the launch has fewer than 2^31 workgroups
 * (NB * ceil(Ho / 8) * ceil(Wo / 16) * ceil(CoutP / 64)).  dm_conv7x7_s2_fwd returns DM_ERR_UNSUPPORTED for anything
 * else, DM_ERR_INVALID_ARG for a null x, w_packed or out.
 *
 * dm_maxpool3x3_s2_fwd: F.max_pool2d(in, 3, stride = 2, padding = 1), in [NC, H, W] -> out [NC, ceil(H / 2),
 * ceil(W / 2)].  Padding taps take no part (a window's result does not depend on the sign of its inputs); the taps of
 * a window are met row by row and a later one replaces the running maximum when it is larger or NaN (torch's rule), so
 * a window of -inf gives -inf and a NaN in a window gives NaN.  dm_maxpool3x3_s2_supported: 1 exactly when NC >= 0,
 * H >= 1, W >= 1 and NC * H * W <= 2^40; anything else: DM_ERR_UNSUPPORTED.  NC == 0 enqueues nothing.
 * ------------------------------------------------------------------------------------------------------------------ */
int dm_conv7x7_s2_supported(int NB, int C, int H, int W, int Cout);
int dm_conv7x7_s2_fwd(const float* x, int NB, int C, int H, int W, const float* w_packed, const float* bias, int Cout,
                      int flags, float* out, dm_stream_t stream);
int dm_maxpool3x3_s2_supported(long long NC, int H, int W);
int dm_maxpool3x3_s2_fwd(const float* in, long long NC, int H, int W, float* out, dm_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * K33  (added to ABI 29) Image pre-processing: the reference's test pipeline Resize(keep_ratio) -> RandomFlip ->
 *      Normalize(to_rgb) -> Pad(size_divisor) -> ImageToTensor -> collate (mmdet/datasets/pipelines/transforms.py,
 *      done there by cv2 on the host) as one launch over B decoded images.  No resized image exists in memory, the
 *      sources are only read, `out` is written completely (it may be uninitialised).
 *
 * srcs: host array of B device addresses of uint8 HWC images, 3 channels, pixel stride 3.  dims: host
 * [B][DM_PREPROCESS_DIMS] = (h, w, row stride in bytes >= 3 w, resized nh, resized nw, flip code DM_AUG_FLIP_*, first
 * row of the image's column taps, first row of its row taps).  taps (int32, device, 16-byte aligned) [tap_rows][4]: one
 * row (i0, i1, c0, c1) per destination index of an axis -- the two source indices and their 11-bit coefficients,
 * c0 + c1 == 2048, built on the host:
 *     f = float32((d + 0.5) * (1.0 / (n_dst / n_src)) - 0.5)   (inner arithmetic in float64)
 *     i = floor(f), t = float32(f - i);  i < 0: i = 0, t = 0;  i >= n_src - 1: i = n_src - 1, t = 0
 *     i0 = i, i1 = min(i + 1, n_src - 1), c0 = rint(float32(1 - t) * 2048), c1 = rint(t * 2048)   (half to even, int16)
 * (an index outside its axis is clamped into it by the kernel).  Per output pixel (y < nh, x < nw) and channel c, with
 * (x0, x1, a0, a1) the column taps of x -- of nw - 1 - x under a horizontal flip -- and (y0, y1, b0, b1) the row taps
 * of y -- of nh - 1 - y under a vertical flip -- and sc = to_rgb ? 2 - c : c, all in int32:
 *     r_top = S[y0][x0][sc] * a0 + S[y0][x1][sc] * a1,  r_bot likewise on row y1
 *     v = clamp((((b0 * (r_top >> 4)) >> 16) + ((b1 * (r_bot >> 4)) >> 16) + 2) >> 2, 0, 255)
 *     out[b][c][y][x] = (float(v) - mean[c]) * stdinv[c]        (two fp32 roundings, no contraction)
 * and out = 0 where y >= nh or x >= nw (the padding to [Hp, Wp], right and bottom).  nh == h and nw == w pass the
 * source bytes through exactly.  mean, stdinv: host float[3].  This is 8-bit INTER_LINEAR as cv2 is recalled to do it;
 * parity with cv2 itself is unverified, and cv2's switch to area averaging at exact 2x decimation is not made.
 * dm_preprocess_u8_supported: 1 exactly when 0 <= B <= DM_PREPROCESS_MAX_IMAGES (the image table travels in the kernel
 * arguments), 1 <= Hp, Wp <= 2^24, Hp <= 4 * 65535, and for every image 1 <= h, w <= 2^24, 1 <= nh <= Hp,
 * 1 <= nw <= Wp, row stride >= 3 w, a flip code of the three, and both tap ranges inside [0, tap_rows).
 * dm_preprocess_u8_fwd returns DM_ERR_UNSUPPORTED for anything else, DM_ERR_INVALID_ARG for a null pointer or
 * misaligned taps.  B == 0 enqueues nothing.
 * ------------------------------------------------------------------------------------------------------------------ */
#define DM_PREPROCESS_MAX_IMAGES 32
#define DM_PREPROCESS_DIMS 8
int dm_preprocess_u8_supported(int B, const int* dims, long long tap_rows, int Hp, int Wp);
int dm_preprocess_u8_fwd(const uint8_t* const* srcs, const int* dims, int B, const int32_t* taps, long long tap_rows,
                         const float* mean, const float* stdinv, int to_rgb, float* out, int Hp, int Wp,
                         dm_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * K34  (added to ABI 29) ResNeXt backbone inference: the grouped 3x3 convolution that is conv2 of every block
 *      (mmdet/models/backbones/resnext.py:54-63: build_conv_layer(..., kernel_size=3, stride, padding=1, groups)).
 *      Everything else of a ResNeXt stage is the launches of K32.  Exact fp32 in every precision mode, deterministic,
 *      no atomics, no workspace.
 *
 * dm_conv3x3_grouped_fwd: out = act(Conv2d(C, C, 3, stride, padding = 1, groups)(x) + bias): x [NB, C, H, W], out
 * [NB, C, Ho, Wo] with Ho = ceil(H / stride), Wo = ceil(W / stride); bias [C] or NULL; x is only read.  Output channel
 * co belongs to group co / (C / groups) and reads the C / groups input channels of that group ONLY: no value of another
 * group's input enters any product, so a NaN or an Inf stays in its group.  flags: bit 0 ReLU (NaN stays NaN); bit 3 is
 * accepted and ignored; bit 4 (the bf16x3 layout): DM_ERR_UNSUPPORTED; any other bit: DM_ERR_INVALID_ARG.  The sum of
 * an output is one fp32 fma chain from zero over its group's input channels in order and, in a channel, ky = 0 .. 2,
 * kx = 0 .. 2 (a tap in the padding multiplies a zero), the bias added last: it does not depend on NB, H, W or the
 * output's position, so an image's bits do not depend on the other images of the call.
 * w_packed: the [C, C / groups, 3, 3] weight as [C / T][C / groups][9][T] -- T = dm_conv3x3_grouped_couts_per_wave(C,
 * groups) neighbouring output channels side by side per (input channel, tap) -- dm_conv3x3_grouped_packed_floats(C,
 * groups) = 9 C C / groups floats.  dm_conv3x3_grouped_pack writes that layout from HOST memory to HOST memory (the
 * Python side makes the same permutation on the device, ops.pack_grouped_conv_weight).
 * dm_conv3x3_grouped_supported: 1 exactly when NB >= 1, groups >= 1, C / groups is one of 4, 8, 16, 32, 64 (C a
 * multiple of groups), stride is 1 or 2, 1 <= H, W, C <= 2^24 and the launch has fewer than 2^31 workgroups (NB * groups
 * * ceil(Ho / TH) * ceil(Wo / 32), TH = 32 / 16 / 8 rows at 4 / 8 / >= 16 channels per group).  One build per (C /
 * groups, stride); nothing else decides.  dm_conv3x3_grouped_fwd returns DM_ERR_UNSUPPORTED for anything else -- from
 * the host arguments alone --, DM_OK without a launch for NB == 0 (pointers unread), DM_ERR_INVALID_ARG for a null x,
 * w_packed or out.  dm_conv3x3_grouped_couts_per_wave: 0, dm_conv3x3_grouped_packed_floats: -1 and
 * dm_conv3x3_grouped_pack: DM_ERR_UNSUPPORTED for channels per group outside the five.
 * ------------------------------------------------------------------------------------------------------------------ */
int dm_conv3x3_grouped_couts_per_wave(int C, int groups);
long long dm_conv3x3_grouped_packed_floats(int C, int groups);
int dm_conv3x3_grouped_pack(const float* w, int C, int groups, float* w_packed);
int dm_conv3x3_grouped_supported(int NB, int C, int H, int W, int groups, int stride);
int dm_conv3x3_grouped_fwd(const float* x, int NB, int C, int H, int W, const float* w_packed, const float* bias,
                           int groups, int stride, int flags, float* out, dm_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * K35  (added to ABI 29) Res2Net backbone inference (mmdet/models/backbones/res2net.py; the deep stem and avg_down of
 *      resnet.py:525-571, :623-631): the sliced 3x3 convolution that stands where conv2 stood in every Bottle2neck, the
 *      2x2 ceil-mode average pool of the downsample path and the first convolution of the deep stem.  Everything else of
 *      a Res2Net is the launches of K32 and dm_conv3x3_dil_fwd.  Exact fp32 in every precision mode, deterministic, no
 *      atomics, no workspace.
 *
 * dm_conv3x3_slices_fwd: ONE launch of G independent act(Conv2d(w, w, 3, stride, padding = 1)(.) + bias).  x
 * [NB, Cx, H, W], addend [NB, Ca, H, W] or NULL, out [NB, Co, Ho, Wo] with Ho = ceil(H / stride), Wo = ceil(W / stride);
 * bias [G * w] or NULL.  Slice g = 0 .. G - 1 reads the channels [x_ch0 + g w, + w) of x -- with an addend the sum
 * x + addend[a_ch0 + g w ..], ONE fp32 add per element before any product (torch's `sp + spx[i]`); the zero padding
 * stays zero -- and writes the channels [o_ch0 + g w, + w) of out.  Nothing else of out is written; x and addend are
 * only read.  A slice forms products with its own w input channels ONLY: K is not padded, neither with foreign channels
 * nor with anything else, so a NaN or an Inf stays in its slice.  flags: bit 0 ReLU (NaN stays NaN); bit 3 is accepted
 * and ignored; bit 4 (the bf16x3 layout): DM_ERR_UNSUPPORTED; any other bit: DM_ERR_INVALID_ARG.  The sum of an output is
 * one fp32 fma chain from zero over its slice's input channels in order and, in a channel, ky = 0 .. 2, kx = 0 .. 2 (a
 * tap in the padding multiplies a zero), the bias added last: it does not depend on NB, G, H, W or the output's
 * position, so an image's bits do not depend on the other images of the call.  Maps of any width run (no row staging).
 * tail: extra workgroups of the same grid.  0: none.  1: the w channels [tail_x_ch0, + w) of x are copied to
 * [tail_o_ch0, + w) of out (stride 1 only).  2: AvgPool2d(3, stride, padding = 1) of them: THE DIVISOR IS ALWAYS 9 -- the
 * elements of the window that lie inside the map are added row-major from zero and the sum is divided once by 9,
 * whatever the window covers (torch's count_include_pad=True).  The addend does not enter the tail.
 * w_packed: the folded weights [G, w, w, 3, 3] as [G][ceil(w / 8)][w][9][8] -- 8 neighbouring output channels of a slice
 * side by side per (input channel, tap), zeros for the output channels from w on (their results are not stored) --
 * dm_conv3x3_slices_packed_floats(G, w) = 72 G w ceil(w / 8) floats.  dm_conv3x3_slices_pack writes that layout from HOST
 * memory to HOST memory (the Python side makes the same permutation on the device, ops.pack_conv_slices_weight).
 * dm_conv3x3_slices_supported: 1 exactly when NB >= 1, 1 <= w, G, H, W <= 2^24, Cx, Co <= 2^24, stride is 1 or 2, tail is
 * 0, 1 (at stride 1) or 2, Cx >= G w, Co >= (G + (tail ? 1 : 0)) w, and the launch has fewer than 2^31 workgroups:
 * NB * (G * ceil(ceil(w / 8) / WCO) * ceil(Ho / TH) * ceil(Wo / 32) + (tail ? ceil(w Ho Wo / 256) : 0)) with WCO = 1,
 * TH = 32 for w <= 8 and WCO = 4, TH = 8 above.  Two builds per stride (w <= 8, w > 8); nothing else decides.
 * dm_conv3x3_slices_fwd returns DM_ERR_INVALID_ARG for a stride outside {1, 2}, DM_ERR_UNSUPPORTED for anything else
 * dm_conv3x3_slices_supported refuses (NB == 0 apart) -- from the host arguments alone --, DM_ERR_INVALID_ARG for a
 * slice range (or, with a tail, a tail range) that leaves Cx / Ca / Co or is negative, for a tail whose output channels
 * meet a slice's, DM_OK without a launch for NB == 0 (pointers unread), DM_ERR_INVALID_ARG for a null x, w_packed or out.
 *
 * dm_avgpool2x2_ceil_fwd: AvgPool2d(2, 2, ceil_mode=True, count_include_pad=False), in [NC, H, W] -> out [NC,
 * ceil(H / 2), ceil(W / 2)]: the elements of the window inside the map are added row-major and divided once by their
 * number (4, 2 or 1).  dm_avgpool2x2_ceil_supported: 1 exactly when NC >= 0, H >= 1, W >= 1 and NC * H * W <= 2^40;
 * anything else: DM_ERR_UNSUPPORTED.  NC == 0 enqueues nothing; a null in / out: DM_ERR_INVALID_ARG.
 *
 * dm_conv3x3_s2_c3_fwd: out = act(Conv2d(3, Cout, 3, stride = 2, padding = 1)(x) + bias), x [NB, 3, H, W], out
 * [NB, Cout, ceil(H / 2), ceil(W / 2)]; w: the [Cout, 3, 3, 3] weight in torch's own layout, bias [Cout] or NULL.  An
 * output reads its own 27 taps and nothing else (a tap in the padding is a zero operand); its sum is one fp32 fma chain
 * from zero over c = 0 .. 2, ky = 0 .. 2, kx = 0 .. 2, the bias added last.  flags as above.
 * dm_conv3x3_s2_c3_supported: 1 exactly when NB >= 1, C == 3, 1 <= H, W, Cout <= 2^24 and the launch has fewer than 2^31
 * workgroups (NB * ceil(Ho Wo / 256) * ceil(Cout / 32)); dm_conv3x3_s2_c3_fwd returns DM_ERR_UNSUPPORTED for anything
 * else, DM_ERR_INVALID_ARG for a null x, w or out.
 * ------------------------------------------------------------------------------------------------------------------ */
long long dm_conv3x3_slices_packed_floats(int G, int w);
int dm_conv3x3_slices_pack(const float* w_folded, int G, int w, float* w_packed);
int dm_conv3x3_slices_supported(int NB, int w, int G, int H, int W, int stride, int Cx, int Co, int tail);
int dm_conv3x3_slices_fwd(const float* x, int Cx, int x_ch0, const float* addend, int Ca, int a_ch0, int NB, int w, int G,
                          int H, int W, int stride, const float* w_packed, const float* bias, int flags, float* out, int Co,
                          int o_ch0, int tail, int tail_x_ch0, int tail_o_ch0, dm_stream_t stream);
int dm_avgpool2x2_ceil_supported(long long NC, int H, int W);
int dm_avgpool2x2_ceil_fwd(const float* in, long long NC, int H, int W, float* out, dm_stream_t stream);
int dm_conv3x3_s2_c3_supported(int NB, int C, int H, int W, int Cout);
int dm_conv3x3_s2_c3_fwd(const float* x, int NB, int C, int H, int W, const float* w, const float* bias, int Cout,
                         int flags, float* out, dm_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * K36  CARAFE on whole feature maps, merged into the lateral below (csrc/carafe_map.hip; added entry points, the ABI
 *      number stays).  replaces: FPN_CARAFE's top-down step (mmdet/models/necks/fpn_carafe.py:211-259):
 *      tensor_add(laterals[i - 1], CARAFEPack.kernel_normalizer + feature_reassemble (laterals[i])) with slice_as.
 *
 * dm_carafe_map_fwd: out = addend + carafe(x, softmax_taps(pixel_shuffle(enc)))[:, :, :OH, :OW] at scale 2.  x
 * [NB, C, H, W]; enc [NB, group * K * K * 4, H, W], the RAW content-encoder output in dm_carafe_fwd's layout (channel
 * ((g K K + tap) * 4 + dy * 2 + dx)); out and addend [NB, C, OH, OW] with 2H - 1 <= OH <= 2H and 2W - 1 <= OW <= 2W.
 * addend may be NULL (nothing is added) and out may be the addend's own memory (every element is read by the thread
 * that writes it); x and enc are only read and may not overlap out.  The upsampled map is never stored, the cropped row
 * and column are neither loaded nor stored.  An output's value: the maximum of its K K raw taps in tap order (fmaxf),
 * expf(v - max) per tap and their sum in tap order, each weight times 1 / sum, ONE fmaf chain over the taps in order
 * i * K + j from zero, then ONE fp32 add of the addend.  A tap outside the image is a zero operand of a zero-padded tile
 * (never another pixel's value times 0): a NaN or an Inf of x reaches exactly the outputs whose window holds its pixel,
 * in its channel; a NaN of enc reaches its one output pixel in every channel of its group.  The bits do not depend on
 * NB, on the position in the grid or on chan_split.  Deterministic, no atomics, no workspace.
 * chan_split: the workgroups a group's channel quads (C / group / 4) are dealt over per pixel tile; 0: the launcher
 * chooses (whole chunks of 2 quads per workgroup, the split that fills the compute units in the fewest rounds).
 * dm_carafe_map_supported: a pure host function; 1 exactly when NB >= 0, C, H, W, group >= 1, up_kernel is 3 or 5,
 * C % group == 0, (C / group) % 4 == 0, OH and OW are in the ranges above and x, enc and out have fewer than 2^31
 * elements each.  dm_carafe_map_fwd returns DM_ERR_INVALID_ARG for a negative NB or chan_split, a non-positive C, H, W or
 * group and a chan_split above C / group / 4; DM_ERR_UNSUPPORTED for anything else dm_carafe_map_supported refuses; then
 * DM_OK without a launch for NB == 0 (pointers unread); DM_ERR_INVALID_ARG for a null x, enc or out.
 * ------------------------------------------------------------------------------------------------------------------ */
int dm_carafe_map_supported(int NB, int C, int H, int W, int up_kernel, int group, int OH, int OW);
int dm_carafe_map_fwd(const float* x, const float* enc, int NB, int C, int H, int W, int up_kernel, int group,
                      const float* addend, int OH, int OW, int chan_split, float* out, dm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DYNAMASK_HIP_H */
