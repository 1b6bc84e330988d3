/*
 * tiatoolbox_amd -- C ABI of the MI355X (gfx950) hot-path library  (libtiatoolbox_amd.so)
 *
 * Every entry point takes raw DEVICE pointers + sizes + a hipStream_t (passed as void*).
 * Naming convention: `d_*` arguments are device pointers (data planes, workspaces, outputs);
 * small parameter blocks that are read on the host while the call is being enqueued are
 * passed by `const` pointer WITHOUT the prefix (`params`, `h_target_stain`, `target_means`,
 * `target_stds`; each is marked "host" where it is declared) -- they play the role of
 * by-value arguments and are copied at launch.
 * No allocation, no synchronisation, no exceptions cross this boundary; each call
 * enqueues kernels on `stream` and returns 0 (TIA_OK) or a negative TIA_E* code.
 *
 * The reference (tiatoolbox v2.0.1) is pure Python; the "FFI" a maintainer would add is
 * a ctypes binding.  Each entry point cites the reference call
 * site(s) it replaces as `file:line` relative to /root/reference/tiatoolbox/.
 */
#ifndef TIATOOLBOX_AMD_H
#define TIATOOLBOX_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TIA_OK 0
#define TIA_EINVAL (-1)   /* bad argument (null pointer, non-positive size, bad mode)   */
#define TIA_ELAUNCH (-2)  /* hipLaunch / runtime failure (hipGetLastError() != success)  */
#define TIA_ESIZE (-3)    /* size outside what the kernel supports                        */

/* Version 3 (round 3): + tia_stem_pack_weights_f32 / tia_stem_conv7x7_pool_nhwc, tia_conv_pack_weights_h / tia_conv2d_nhwc_h,
 * tia_stem_pack_weights_h / tia_stem_conv7x7_pool_nhwc_h, tia_conv2d_thin_nhwc_f32, tia_conv1x1_head_nhwc_f32, tia_lut_apply_u8, tia_box_downsample_u8; the workspace of
 * tia_stain_stats_u8 grew by one int32 flag per patch (tia_stain_stats_workspace_bytes_mode reports it). */
/* Version 4 (round 4): + tia_rgb2od_u8 (the stand-alone OD transform, with the reference's in-place side effect on request),
 * tia_clear_last_error; TIA_MATH_F64 of tia_stain_apply_u8 evaluates exp() with the library's own float64 kernel
 * (TIA_MATH_F64_REF keeps the device libm's exp); tia_conv3x3_geometry, tia_stain_stats_path (dispatch diagnostics). */
/* Version 6 (round 6): + tia_gray_hist_u8 / tia_otsu_threshold_u32 / tia_otsu_fit_u8 / tia_threshold_lt_dev_u8 (one-pass, one-launch
 * Otsu fit whose threshold stays on the device), tia_morph_mask_u8 (the morphological masker in one launch), tia_reinhard_transform_u8 /
 * tia_reinhard_workspace_bytes / tia_lab_moments_u8 (one-launch Reinhard); tia_luminosity_mask_u8 and the float64 form of
 * tia_stain_augment_u8 (now a product of per-patch tables) take 16-byte accesses where the shape allows.
 * Additive, same version: tia_gather_area_patches_u8 (patch reads below the slide's resolution), tia_gather_area_resize_u8
 * (the same at any down-sampling ratio), tia_gather_cubic_resize_u8 (patch reads above the slide's resolution),
 * tia_conv3x3_grouped_nhwc_f32 (the grouped 3x3 of ResNeXt), tia_stem_pack_weights_bf16x3 / tia_stem_conv7x7_pool_nhwc_u8x3 (the
 * uint8 stem on the bf16 matrix cores with exactly split float32 weights); tia_mha_fwd_h, tia_layernorm_rows_h, tia_gelu_rows_h,
 * tia_vit_patchify_h, tia_vit_assemble_tokens_h (the Vision Transformer backbones in fp16 / bf16); tia_swiglu_rows_h,
 * tia_vit_patchify_pad_h, tia_vit_assemble_prefix_h (UNI2, H-optimus and prov-gigapath on the same graph); tia_vit_cls_mean_pool_h
 * and head_dim 80 in tia_mha_fwd_h (Virchow, Virchow2); tia_vit_patchify_norm_u8_h, tia_linear_softmax_rows_f32 (Vision Transformer
 * classifiers from uint8 patches to probabilities); tia_linear_fp8_rows, tia_linear_fp8_pack_weights, tia_linear_fp8_serves,
 * tia_layernorm_rows_q8, tia_gelu_rows_q8, tia_swiglu_rows_q8 (the Vision Transformer linear layers on the FP8 matrix instruction); tia_add_layernorm_rows_f32,
 * tia_vit_assemble_rows_f32, tia_vit_cls_mean_pool_f32 (the same graph with a float32 residual stream); tia_mha_fwd_f32,
 * tia_gelu_rows_f32, tia_swiglu_rows_f32, tia_vit_patchify_f32, tia_vit_assemble_f32 (the float32 route of that graph);
 * tia_linear_int8_rows, tia_linear_int8_pack_weights, tia_linear_int8_serves, tia_layernorm_rows_qi8, tia_gelu_rows_qi8,
 * tia_swiglu_rows_qi8 (the Vision Transformer linear layers on the INT8 matrix instruction); tia_gelu_rows_qi8_smooth,
 * tia_swiglu_rows_qi8_smooth, tia_layernorm_rows_absmax_h, tia_gelu_rows_absmax_h, tia_swiglu_rows_absmax_h (per-input-channel
 * smoothing of those layers and its calibration statistics); tia_mha_probs_h, tia_rollout_step_f32 (attention maps of the Vision
 * Transformer runs: the probabilities tia_mha_fwd_h does not materialise, and attention rollout); tia_merge_patch_grids_f32 (those maps resampled into a
 * whole-slide heat map); tia_mha_probs_fused_h, tia_rollout_discard_normalize_f32, tia_rollout_product_f32 (rollout with max / min
 * head fusion and a discard ratio); tia_cam_nhwc_f32, tia_cam_nhwc_h (class activation maps of the CNN classifiers); tia_peak_chunks,
 * tia_peak_scan_f32, tia_peak_write_f32, tia_peak_resolve_host (peak_local_max on probability maps). */
#define TIA_ABI_VERSION 6
int tia_abi_version(void);

/* Reads-and-clears the HIP runtime's sticky last-error value as THIS library sees it (every entry point returns
 * `hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH`).  Call it after a host-side HIP call that is allowed to be
 * refused (hipHostRegister of already-pinned memory) so that the refusal does not surface as a later TIA_ELAUNCH.
 * Returns the value that was pending (0 = none). */
int tia_clear_last_error(void);

/* ---------------------------------------------------------------------------------------
 * Stain tables (device buffer, built once by the host; layout = struct tia_stain_tables).
 * od_lut[v]      = max(-ln(max(v,1)/255), 1e-6)            utils/transforms.py:229-231
 * ty[c][v]       = C[3+c] * sRGBGammaTab_b[v]   (Y row of OpenCV's 8-bit RGB2Lab)
 *                  -> L channel for get_luminosity_tissue_mask, utils/misc.py:281-283
 * ------------------------------------------------------------------------------------- */
typedef struct tia_stain_tables {
    double od_lut[256];
    float od_lut_f32[256];
    int32_t ty[3][256];
} tia_stain_tables;

/* Per-patch statistics record: TIA_STATS_STRIDE doubles per patch (512 B, cache-line aligned). */
#define TIA_STATS_STRIDE 64
#define TIA_ST_STAIN 0    /* [6]  source stain matrix, rows H,E unit norm  (stainextract.py:177-227) */
#define TIA_ST_MAXC 6     /* [2]  99th pct of source concentrations        (stainnorm.py:103)        */
#define TIA_ST_NTISSUE 8  /*      tissue pixel count                                                   */
#define TIA_ST_PLOW 9     /*      contrast-enhancer p_low                   (utils/misc.py:434-437)   */
#define TIA_ST_PHIGH 10   /*      contrast-enhancer p_high                                             */
#define TIA_ST_MINPHI 11  /*      percentile(phi, 100-ap)                   (stainextract.py:217)     */
#define TIA_ST_MAXPHI 12  /*      percentile(phi, ap)                       (stainextract.py:218)     */
#define TIA_ST_COV 13     /* [6]  OD covariance xx,xy,xz,yy,yz,zz (ddof=1)  (stainextract.py:202)     */
#define TIA_ST_EVEC 19    /* [6]  principal eigenvectors v1[3], v2[3] after sign fix (:205-208)       */
#define TIA_ST_FLAGS 25   /*      bit0: empty tissue mask; bit1: degenerate (n<2 / non-finite)        */
#define TIA_ST_PINV 26    /* [6]  pinv(S^T) as P[j*2+i], C_i = sum_j OD_j P[j][i] (stainnorm.py:65)   */
#define TIA_ST_M 32       /* [9]  M[j*3+c] = sum_i P[j][i]*(maxC_t[i]/maxC_s[i])*S_t[i][c]            */
#define TIA_ST_SCALE 41   /* [2]  maxC_target / maxC_source                 (stainnorm.py:104)        */
#define TIA_ST_CYCLES 48  /* [16] shader-clock cycles per phase (instrumentation: -DTIA_STATS_TIMING=1 builds of stain_stats_*.hip) */

#define TIA_FLAG_EMPTY_MASK 1
#define TIA_FLAG_DEGENERATE 2

#define TIA_MODE_MACENKO 0 /* estimate the stain matrix per patch (MacenkoExtractor)       */
#define TIA_MODE_FIXED 1   /* stain matrix given (Custom / Ruifrok)                         */
#define TIA_MODE_GIVEN 3   /* as TIA_MODE_FIXED, but every patch brings its own stain matrix: d_stats[i][TIA_ST_STAIN..+5]
                              is read on entry (StainAugmentor.fit on a batch, stainaugment.py:141-175) */
#define TIA_MODE_VAHADANE 2 /* per-patch dictionary learning (VahadaneExtractor, stainextract.py:281-322): X = tissue
                              OD transposed (3 x N), sklearn DictionaryLearning(n_components=2, alpha, fit_algorithm="lars",
                              positive_dict=True, max_iter) restated -- SVD initialisation, two-atom lasso codes, in-place
                              dictionary update with the 1e-6 unused-atom rule, cost-based stopping; the stain matrix is
                              the code transposed, H row first, unit rows */

typedef struct tia_stain_params {
    double q_img_lo;        /* contrast_enhancer low percentile / 100   (0.02) */
    double q_img_hi;        /* contrast_enhancer high percentile / 100  (0.98) */
    double q_phi_lo;        /* (100 - angular_percentile) / 100          (0.01) */
    double q_phi_hi;        /* angular_percentile / 100                  (0.99) */
    double q_conc;          /* concentration percentile / 100            (0.99) */
    double stain_fixed[6];  /* TIA_MODE_FIXED: the 2x3 stain matrix                          */
    double target_stain[6]; /* fitted target stain matrix (for TIA_ST_M); ignored if !has_target */
    double target_maxc[2];  /* fitted target maxC                                            */
    int32_t y_thr;          /* tissue <=> descaled Y index < y_thr (from luminosity threshold) */
    int32_t mode;           /* TIA_MODE_*                                                    */
    int32_t has_target;     /* 1: also emit TIA_ST_M / TIA_ST_SCALE                          */
    int32_t zero_to_one;    /* 1: treat byte 0 as 1 in the mask path (rgb2od's in-place edit
                               seen by StainAugmentor.fit, stainaugment.py:163-175)          */
    double dl_alpha;        /* TIA_MODE_VAHADANE: regularizer (alpha = transform_alpha, 0.1; stainextract.py:307-308) */
    double dl_tol;          /* DictionaryLearning.tol (1e-8)                                  */
    int32_t dl_max_iter;    /* DictionaryLearning.max_iter (3; stainextract.py:313)           */
    int32_t dl_seed;        /* stream of the unused-atom re-draw (the reference is unseeded)  */
    int32_t select_mode;    /* order statistics: 0 = sample-placed windows (one float32 sweep + exact candidates) with the
                               histogram path as fall-back, on the register-resident kernel where the patch fits;
                               1 = histogram path only; 2 = windows on the streaming kernel only (same results bit for bit
                               in all three; 1 and 2 are parity audits) */
    int32_t dl_one_kernel;  /* TIA_MODE_VAHADANE, parity audit: 0 = the kernel pair (dictionary learning by per-pixel replay of
                               the atom updates -- no dictionary in memory -- followed by the common tail); 1 = the one-kernel form
                               that keeps the 2 x N float64 dictionary in the workspace.  Same results bit for bit.  (Was
                               `reserved`, 0, before ABI version 4.) */
} tia_stain_params;

/*
 * Per-patch stain statistics for a batch of NHWC uint8 patches (one workgroup per patch).
 * Replaces, per patch: MacenkoExtractor.get_stain_matrix (tools/stainextract.py:177-227,
 * incl. utils/misc.py:261-290,405-444 and utils/transforms.py:209-231), the lstsq of
 * StainNormalizer.get_concentrations (tools/stainnorm.py:49-66) as a closed-form
 * pseudo-inverse, and np.percentile(C, 99, axis=0) (tools/stainnorm.py:81-85,103).
 *   d_img    [n,h,w,3] uint8     d_tables  tia_stain_tables     d_stats [n,TIA_STATS_STRIDE] f64
 *   d_ws     optional scratch of tia_stain_stats_workspace_bytes(n,h,w) bytes (8-byte aligned): a
 *            per-pixel histogram-bin cache that lets the selection's collect passes skip the value
 *            computation; with NULL / too little space the kernel recomputes (same results).
 *            TIA_MODE_VAHADANE needs tia_stain_stats_workspace_bytes_mode(n,h,w,mode) bytes, 16-byte aligned
 *            (bin cache + the 2 x N float64 dictionary of every patch); too little -> TIA_ESIZE.
 */
size_t tia_stain_stats_workspace_bytes(int64_t n, int64_t h, int64_t w);
size_t tia_stain_stats_workspace_bytes_mode(int64_t n, int64_t h, int64_t w, int32_t mode);
int tia_stain_stats_u8(const uint8_t* d_img, int64_t n, int64_t h, int64_t w,
                       const tia_stain_tables* d_tables, const tia_stain_params* params,
                       double* d_stats, void* d_ws, size_t ws_bytes, void* stream);
/* Which of the two statistics kernels serves patches of h x w with these parameters, given an aligned, full-size workspace
 * (diagnostics for tests and profiles; host only): 0 = the streaming kernel (the patch is re-read per sweep), 1 = the
 * register-resident kernel (one read; patches it hands back go through the streaming kernel).  Same bits either way. */
int tia_stain_stats_path(int64_t h, int64_t w, const tia_stain_params* params /* host */);

/* Output kinds of tia_stain_apply_u8 */
#define TIA_OUT_U8 0       /* uint8 NHWC, astype(uint8) truncation   (stainnorm.py:110-113)          */
#define TIA_OUT_F32 1      /* float32 NHWC: the pre-cast float in [0,255] (parity instrumentation)   */
#define TIA_OUT_F64 2      /* float64 NHWC: idem, f64                                                  */
#define TIA_OUT_UNIT_F16 3 /* half NHWC = uint8(trunc)/255 : ToTensor() of the normalised patch       */
#define TIA_OUT_UNIT_BF16 4
#define TIA_OUT_UNIT_F32 5

#define TIA_MATH_F64 0 /* float64 throughout, 3x3 matrix TIA_ST_M fused in float64; 255 exp(-OD') evaluated as the
                          product of three per-patch table entries T_j[c][v] = exp(-LUT[v] m[j][c]) built with libm
                          (16-byte-access kernels, round 5; relative error <= ~1e-15) or by the kernel's own table +
                          cubic (12-byte-access kernels; <= 4e-15): < 1e-12 on the 0..255 scale either way */
#define TIA_MATH_F32 1 /* fused 3x3 matrix in f32: |err| <= 1e-4 on the pre-cast float            */
#define TIA_MATH_F64_REF 2 /* the reference's order of operations in f64 (stainnorm.py:102-107) with the device
                              library's exp(): parity audit of TIA_MATH_F64, and its in-kernel fall-back for patches
                              whose matrix is not finite / outside the table arithmetic's safe range    */

/*
 * out = 255*exp(-(OD(img) . pinv . diag(scale) . S_target)), clipped to [0,255].
 * Streaming kernel: 1 read + 1 write per pixel.  Replaces tools/stainnorm.py:102-113.
 * Reads TIA_ST_M / TIA_ST_PINV / TIA_ST_SCALE from d_stats (produced with has_target=1).
 */
int tia_stain_apply_u8(const uint8_t* d_img, int64_t n, int64_t h, int64_t w,
                       const tia_stain_tables* d_tables, const double* d_stats,
                       const double* h_target_stain /* host parameter block, double[6] */, void* d_out, int32_t out_kind,
                       int32_t math, void* stream);

/*
 * Concentrations C[n*h*w, 2] (f64) of every pixel w.r.t. the per-patch TIA_ST_PINV.
 * Replaces StainNormalizer.get_concentrations (tools/stainnorm.py:49-66).
 */
int tia_stain_concentrations_f64(const uint8_t* d_img, int64_t n, int64_t h, int64_t w,
                                 const tia_stain_tables* d_tables, const double* d_stats,
                                 double* d_conc, void* stream);

/*
 * StainAugmentor.augment (tools/stainaugment.py:177-206): C[mask,i] = C[mask,i]*alpha[i]+beta[i]
 * (all pixels if augment_background), out = uint8(clip(255*exp(-C.S),0,255)).  S = per-patch
 * TIA_ST_STAIN, mask from TIA_ST_PLOW/PHIGH + tables.  d_alpha_beta: [n,4] f64 = a0,a1,b0,b1.
 * math = TIA_MATH_F64: float64 -- for whole 3072-byte chunks and 16-byte aligned buffers as a product of per-patch tables (the
 * augmented optical density is affine in the three input optical densities: two sets of nine 256-entry tables replace three
 * exponentials per pixel; < 1e-13 from the per-pixel arithmetic on the 0..255 scale), else / for degenerate stain matrices the
 * reference's per-pixel arithmetic with the device libm's exp; TIA_MATH_F32: float32 with hardware exp2 and
 * 16-byte global accesses (needs h*w*3 % 3072 == 0 and 16-byte aligned buffers, else TIA_ESIZE).
 */
int tia_stain_augment_u8(const uint8_t* d_img, int64_t n, int64_t h, int64_t w,
                         const tia_stain_tables* d_tables, const double* d_stats,
                         const double* d_alpha_beta, int32_t y_thr, int32_t augment_background,
                         int32_t zero_to_one, uint8_t* d_out, int32_t math, void* stream);

/* Luminosity tissue mask (utils/misc.py:261-290) as uint8 0/1 [n,h,w]; needs TIA_ST_PLOW/PHIGH. */
int tia_luminosity_mask_u8(const uint8_t* d_img, int64_t n, int64_t h, int64_t w,
                           const tia_stain_tables* d_tables, const double* d_stats, int32_t y_thr,
                           int32_t zero_to_one, uint8_t* d_mask, void* stream);

/*
 * rgb2od (utils/transforms.py:209-231) of `nbytes` uint8 values of any shape: d_od[i] = max(-ln(max(d_img[i],1)/255), 1e-6)
 * as float64 (table look-up: the 256 possible results, computed on the host with NumPy's own log).  mutate = 1 also
 * performs the reference's side effect on its argument, `img[img == 0] = 1` (:229-230), in place on d_img.
 */
int tia_rgb2od_u8(uint8_t* d_img, int64_t nbytes, const tia_stain_tables* d_tables, int32_t mutate, double* d_od, void* stream);


/* =======================================================================================
 * Image primitives shared by the tissue maskers (tools/tissuemask.py) and the HoVer-Net
 * post-processing (models/architecture/hovernet.py:502-616).  All images are [n,h,w] planes.
 * ===================================================================================== */

/* cv2.cvtColor(COLOR_RGB2GRAY) 8-bit: (R*9798 + G*19235 + B*3735 + 2^14) >> 15
 * (tools/tissuemask.py:129,160,291).  d_img [npix,3] -> d_gray [npix]. */
int tia_rgb2gray_u8(const uint8_t* d_img, int64_t npix, uint8_t* d_gray, void* stream);

/* 256-bin histogram of bytes, ACCUMULATED into d_hist[256] (zero it first); feeds
 * skimage.filters.threshold_otsu (tools/tissuemask.py:131-134). */
int tia_hist256_u8(const uint8_t* d_data, int64_t n, uint32_t* d_hist, void* stream);

/* mask = (gray < thr) as 0/1 bytes; with is_rgb the grey conversion is fused
 * (tools/tissuemask.py:156-162, 288-296). */
int tia_threshold_lt_u8(const uint8_t* d_src, int64_t npix, int32_t is_rgb, int32_t thr,
                        uint8_t* d_mask, void* stream);

/* OtsuTissueMasker.fit in one pass (tools/tissuemask.py:127-137): the grey conversion of tia_rgb2gray_u8 (channels == 3; a grey
 * plane with channels == 1) fused with the 256-bin histogram, ACCUMULATED into d_hist[256] (zero it first; several calls add
 * several images).  Nothing is written but the counts: 3 bytes read per pixel. */
int tia_gray_hist_u8(const uint8_t* d_img, int64_t npix, int32_t channels, uint32_t* d_hist, void* stream);

/* skimage.filters.threshold_otsu of a 256-bin byte histogram on the device (tools/tissuemask.py:131-134): d_out[0] = threshold
 * (bin centre of the first maximum of the between-class variance over the occupied range; the only occupied bin when there is one),
 * d_out[1] = number of occupied bins.  Bit-identical to the float64 NumPy arithmetic (all partial sums are exact integers). */
int tia_otsu_threshold_u32(const uint32_t* d_hist, int32_t* d_out, void* stream);

/* OtsuTissueMasker.fit in ONE launch: tia_gray_hist_u8 whose last-finishing workgroup runs tia_otsu_threshold_u32's arithmetic on
 * the completed counts.  d_hist: 257 uint32 -- the 256 bins and a ticket counter -- zeroed by the caller before the first image
 * (the kernel leaves the counter at zero, so a later call that adds another image to the same counts recomputes d_out). */
int tia_otsu_fit_u8(const uint8_t* d_img, int64_t npix, int32_t channels, uint32_t* d_hist, int32_t* d_out, void* stream);

/* tia_threshold_lt_u8 with the threshold read from device memory (d_thr[0], e.g. tia_otsu_threshold_u32's output): fit and
 * transform enqueue back to back without a host round trip (tools/tissuemask.py:139-164). */
int tia_threshold_lt_dev_u8(const uint8_t* d_src, int64_t npix, int32_t is_rgb, const int32_t* d_thr, uint8_t* d_mask,
                            void* stream);

/* MorphologicalMasker.transform in one launch (tools/tissuemask.py:270-306): grey < thr (thr from d_thr[0] when d_thr is given),
 * skimage remove_small_objects(min_size = min_region, connectivity 8), cv2.dilate with the element whose non-zero entries are
 * d_offsets [n_off,2] = (dy, dx) relative to the anchor (`reach` = max |dy|, |dx|).  d_img [n,h,w,channels] (3: RGB, the grey
 * conversion fused; 1: grey plane) -> d_mask [n,h,w] 0/1.  Tiles of 256 x 128 pixels with a halo of reach + min_region - 1 are
 * labelled in LDS; a halo above 40 pixels returns TIA_ESIZE (use tia_threshold_lt_u8 + tia_ccl_label_i32 +
 * tia_label_area_filter_i32 + tia_binary_morph_u8). */
int tia_morph_mask_u8(const uint8_t* d_img, int64_t n, int64_t h, int64_t w, int32_t channels, int32_t thr, const int32_t* d_thr,
                      int32_t min_region, const int32_t* d_offsets, int32_t n_off, int32_t reach, uint8_t* d_mask, void* stream);

/* Connected-component labelling of n binary planes (non-zero = foreground), connectivity 4 or 8.
 * Labels are 1..K per plane, numbered in raster order of each component's first pixel
 * (= scipy.ndimage.label, hovernet.py:543,607; cv2.connectedComponentsWithStats labelling,
 * tissuemask.py:297).  d_labels [n,h,w] i32, d_count [n] i32, d_ws: n*h*w i32 scratch. */
int tia_ccl_label_i32(const uint8_t* d_mask, int64_t n, int64_t h, int64_t w, int32_t connectivity,
                      int32_t* d_labels, int32_t* d_count, int32_t* d_ws, void* stream);

/* Zero every label whose pixel count is < min_keep (no relabelling):
 * skimage remove_small_objects(max_size=s) == min_keep = s+1 (hovernet.py:544,614);
 * MorphologicalMasker min_region_size == min_keep (tissuemask.py:297-301).
 * d_ws: n*(h*w+1) i32 scratch (per-label areas). */
int tia_label_area_filter_i32(int32_t* d_labels, int64_t n, int64_t h, int64_t w, int32_t min_keep,
                              int32_t* d_ws, void* stream);

/* Binary morphology with an arbitrary structuring element given as n_off (dy,dx) int32 pairs
 * relative to the anchor.  op 0 = dilate (outside = 0), 1 = erode (outside = 1), i.e. OpenCV's
 * morphologyEx with the default border value (tissuemask.py:303; hovernet.py:605-606). */
int tia_binary_morph_u8(const uint8_t* d_src, int64_t n, int64_t h, int64_t w, const int32_t* d_offsets,
                        int32_t n_off, int32_t op, uint8_t* d_dst, void* stream);

/* scipy.ndimage.binary_fill_holes with the default (4-connected) structure (hovernet.py:604):
 * background components not connected to the border become foreground.
 * d_ws: (2*n*h*w + n) i32 scratch. */
int tia_fill_holes_u8(const uint8_t* d_mask, int64_t n, int64_t h, int64_t w, uint8_t* d_out,
                      int32_t* d_ws, void* stream);


/* =======================================================================================
 * HoVer-Net post-processing (models/architecture/hovernet.py:502-748)
 * ===================================================================================== */

/* Bytes of scratch tia_hover_proc_np_hv_f32 needs for n planes of h x w. */
size_t tia_hover_workspace_bytes(int64_t n, int64_t h, int64_t w);

/*
 * HoVerNet._proc_np_hv (hovernet.py:502-616) for n patches/tiles at once:
 * binarise np>=0.5 -> 4-connected labelling -> drop objects <= 9 px -> min-max normalise the
 * h/v maps (f32) -> Sobel ksize (CV_64F, separable, REFLECT_101) -> normalise (f32) ->
 * energy / distance maps (f64) -> 3x3 Gaussian -> marker = blb - (overall>=0.4), fill holes,
 * 5x5 elliptical opening, labelling, drop objects < obj_size -> marker-controlled watershed
 * (priority flood, one independent flood per mask blob).
 *   d_np [n,h,w] f32   d_hv [n,h,w,2] f32   d_inst [n,h,w] i32 (instance ids = marker ids)
 *   d_ninst [n] i32 (number of marker labels = max possible id)
 */
int tia_hover_proc_np_hv_f32(const float* d_np, const float* d_hv, int64_t n, int64_t h, int64_t w,
                             int32_t ksize, int32_t obj_size, int32_t* d_inst, int32_t* d_ninst,
                             void* d_ws, size_t ws_bytes, void* stream);

/*
 * Same pipeline with optional copies of its intermediate planes (any of the five may be NULL), so each stage can be
 * compared with the reference's corresponding local (hovernet.py:547-614) instead of only the final label map:
 *   d_sobel_h / d_sobel_v [n,h,w] f64 = cv2.Sobel(normalised h|v, CV_64F, ksize) before the second normalisation (:554-555)
 *   d_dist [n,h,w] f64 = -cv2.GaussianBlur((1 - overall) * blb, (3,3), 0)                                      (:599-600)
 *   d_markers [n,h,w] i32 = labelled, size-filtered markers fed to the watershed                             (:607-614)
 *   d_blobs [n,h,w] i32 = blb (0/1) after remove_small_objects                                               (:543-545)
 */
int tia_hover_proc_np_hv_stages_f32(const float* d_np, const float* d_hv, int64_t n, int64_t h, int64_t w,
                                    int32_t ksize, int32_t obj_size, int32_t* d_inst, int32_t* d_ninst,
                                    double* d_sobel_h, double* d_sobel_v, double* d_dist, int32_t* d_markers,
                                    int32_t* d_blobs, void* d_ws, size_t ws_bytes, void* stream);

/* Bytes of scratch tia_watershed_blobs_f64 needs for n planes of h x w. */
size_t tia_watershed_workspace_bytes(int64_t n, int64_t h, int64_t w);

/*
 * skimage.segmentation.watershed(image, markers, mask=mask) with connectivity 1, no compactness, no watershed line
 * (the call at hovernet.py:616), for n planes: priority flood ordered by (value, insertion age) with skimage's own
 * binary-heap procedures (heap_general.pxi), neighbours visited up / left / right / down, a pixel labelled when it is
 * pushed.  Floods of different 4-connected mask components are independent and run concurrently, one wave each.
 *   d_image [n,h,w] f64   d_markers [n,h,w] i32 (>= 0; 0 = no marker)   d_mask [n,h,w] u8 (non-zero = flood here)
 *   d_out [n,h,w] i32: label of the marker whose flood reached the pixel; 0 outside the mask and in unreached blobs
 */
int tia_watershed_blobs_f64(const double* d_image, const int32_t* d_markers, const uint8_t* d_mask, int64_t n,
                            int64_t h, int64_t w, int32_t* d_out, void* d_ws, size_t ws_bytes, void* stream);

/*
 * Per-instance statistics for HoVerNet.get_instance_info (hovernet.py:670-748): for every id in
 * 1..max_inst of every plane: pixel count, bounding box (x_min,y_min,x_max,y_max inclusive),
 * sum of x, sum of y, and the histogram of d_type (uint8, may be NULL) over its pixels.
 *   d_stats [n, max_inst+1, 8] i64 = area, xmin, ymin, xmax, ymax, sumx, sumy, 0
 *   d_types [n, max_inst+1, num_types] i32
 * Both must be zero-initialised except xmin/ymin which the call initialises itself.
 */
int tia_hover_instance_stats(const int32_t* d_inst, const uint8_t* d_type, int64_t n, int64_t h, int64_t w,
                             int32_t max_inst, int32_t num_types, int64_t* d_stats, int32_t* d_types,
                             void* stream);

/*
 * Contour polygon of every instance: cv2.findContours(mask, RETR_TREE, CHAIN_APPROX_SIMPLE)[0][0]
 * of the instance's binary mask (hovernet.py:685-692) = the top-level outer border found last in
 * raster order, vertices where the 8-connected chain code changes, counter-clockwise on screen
 * starting at the border's first pixel in raster order.  One lane follows the borders of one instance.
 *   scan : d_stats from tia_hover_instance_stats; d_mark = n*h*w bytes of scratch;
 *          d_meta [n, max_inst+1, 4] i32 = start x, start y, vertex count, offset of the first vertex
 *          (exclusive prefix sum over the whole table); d_total[0] = number of vertices of all instances.
 *   write: d_points [capacity, 2] i32 (x, y) in image coordinates; instances whose vertices would not
 *          fit in `capacity` are left unwritten (pass capacity = *d_total).
 * The reference drops instances with fewer than 3 vertices (hovernet.py:695-699); that is the caller's job.
 */
int tia_hover_contour_scan(const int32_t* d_inst, int64_t n, int64_t h, int64_t w, int32_t max_inst,
                           const int64_t* d_stats, int8_t* d_mark, int32_t* d_meta, int64_t* d_total,
                           void* stream);
int tia_hover_contour_write(const int32_t* d_inst, int64_t n, int64_t h, int64_t w, int32_t max_inst,
                            const int64_t* d_stats, const int32_t* d_meta, int64_t capacity,
                            int32_t* d_points, void* stream);


/* =======================================================================================
 * Semantic-segmentation stitching (models/engine/semantic_segmentor.py:1141-1263,1398-1534)
 * ===================================================================================== */

/*
 * Horizontal merge of one patch row (merge_batch_to_canvas / merge_horizontal): every pixel of the
 * row canvas sums, in patch order, the blocks covering it; all-zero blocks are skipped
 * (:1178-1179); x-extents are clipped to the canvas width.
 *   d_blocks [n,oh,ow,c] f32   d_xs [n] i32 (output x0 of each block, in any order: a pixel adds its
 *   blocks in the order they are given, as the reference's loop does); c <= 8, n <= 65535
 *   d_row [oh,W,c] f32 (overwritten)   d_cnt [oh,W] u8 (overwritten)   d_flags [n] i32 scratch
 */
int tia_canvas_row_merge_f32(const float* d_blocks, const int32_t* d_xs, int64_t n, int64_t oh, int64_t ow,
                             int64_t c, int64_t width, float* d_row, uint8_t* d_cnt, int32_t* d_flags,
                             void* stream);

/*
 * Vertical merge + normalisation + argmax for canvas rows [y_begin, y_end)
 * (merge_vertical_chunkwise + post_process_wsi): value = rowA[y-ysA] (+ rowB[y-ysB] where the next
 * patch row overlaps), prob = value / max(count,1) (f32; the count is the uint8 sum of the two
 * counts, which wraps), prediction = np.argmax over channels (uint8): the first NaN, else the first
 * maximum.  d_row_b may be NULL.  d_probs ([H,W,c] f32) may be NULL.
 */
int tia_canvas_finalize_f32(const float* d_row_a, const uint8_t* d_cnt_a, int64_t ys_a, const float* d_row_b,
                            const uint8_t* d_cnt_b, int64_t ys_b, int64_t oh, int64_t width, int64_t c,
                            int64_t y_begin, int64_t y_end, float* d_probs, uint8_t* d_pred, void* stream);

/*
 * Patch predictions painted into a whole-slide map (PatchPredictor.merge_predictions; additive at version 6): for every map
 * pixel (Y, X) of the h x w canvas, sum[Y,X,k] = the float32 sum of d_values[i,k] over the patches i whose rectangle
 * d_rects[i] = (x0, y0, x1, y1) (map pixels, half-open, clipped to the canvas; x1 <= x0 or y1 <= y0 covers nothing) holds the
 * pixel, added one at a time in ascending i -- `out[y0:y1, x0:x1] += values[i]` in a loop over i, bit for bit; count[Y,X] = the
 * number of such patches; raw = float32(float64(sum) / (float64(count) + 1e-8)); label = 1 + the first maximum over k of
 * sum[Y,X,:] where count > 0, else 0.  Gather by tiles, no atomics: the map is cut into tiles of tile_h x tile_w pixels (row-major,
 * tiles_x = ceil(w / tile_w)); d_tile_items[d_tile_offsets[t] .. d_tile_offsets[t + 1]) lists every patch whose rectangle meets tile
 * t, in ASCENDING order (the caller's contract; an item outside [0, n) is skipped).  Any of the four outputs may be NULL, not all.
 *   d_rects [n,4] i32   d_values [n,c] f32   d_tile_offsets [tiles_y*tiles_x+1] i32   d_tile_items [d_tile_offsets[last]] i32
 *   d_sum, d_raw [h,w,c] f32   d_count [h,w] i32   d_labels [h,w] u8 (label_bytes 1, c <= 254) or i32 (label_bytes 4)
 * TIA_EINVAL: a null input or list pointer, all outputs NULL, n / c / h / w / tile_h / tile_w <= 0, label_bytes not 1 or 4, or
 * label_bytes 1 with c > 254.  TIA_ESIZE: h * w >= 2^31, n >= 2^31, or 2^24 tiles or more.  Nothing is launched on an error.
 */
int tia_merge_patch_rects_f32(const int32_t* d_rects, const float* d_values, int64_t n, int64_t c, int64_t h, int64_t w,
                              const int32_t* d_tile_offsets, const int32_t* d_tile_items, int64_t tile_h, int64_t tile_w,
                              float* d_sum, float* d_raw, int32_t* d_count, void* d_labels, int32_t label_bytes, void* stream);

/*
 * Per-patch attention grids resampled into a whole-slide map (PatchPredictor.merge_attention; additive at version 6).  The
 * arithmetic is stated once, in the docstring of models/engine/_attention_merge.py.  Patch i covers the rectangle d_rects[i] as in
 * tia_merge_patch_rects_f32 and brings d_maps[i] = c grids of gh x gw cells; a covered pixel (Y, X) samples them at
 * gx = ax * float(X - x0) + cx, gy = ay * float(Y - y0) + cy with d_affine[i] = (ax, cx, ay, cy), clamped to [0, gw - 1] x
 * [0, gh - 1], every float32 operation rounded on its own: mode 0 the nearest cell (floor(g + 0.5)), mode 1 bilinear between the
 * four cells around (j0 = floor(g), weight g - j0, j1 = min(j0 + 1, g* - 1); top and bottom lerp in x, then one lerp in y, each
 * a + t * (b - a)).  sum[k,Y,X] = the float32 sum of the samples over the covering patches, added one at a time in ascending i;
 * count[Y,X] = their number; raw = float32(float64(sum) / (float64(count) + 1e-8)).  The tile lists are those of
 * tia_merge_patch_rects_f32 (ASCENDING per tile: the caller's contract; an item outside [0, n) is skipped).  Outputs are planar.
 * No atomics: two launches give the same bits.  Any of the three outputs may be NULL, not all.
 *   d_rects [n,4] i32   d_affine [n,4] f32   d_maps [n,c,gh,gw] f32   d_tile_offsets [tiles_y*tiles_x+1] i32
 *   d_tile_items [d_tile_offsets[last]] i32   d_sum, d_raw [c,h,w] f32   d_count [h,w] i32
 * TIA_EINVAL: a null input or list pointer, all outputs NULL, n / c / gh / gw / h / w / tile_h / tile_w <= 0, mode not 0 or 1.
 * TIA_ESIZE: h * w >= 2^31, n >= 2^31, c >= 2^31, gh * gw >= 2^31, gh or gw > 2^24 (the clamp's upper end must be a float32
 * number), or 2^24 tiles or more.  Nothing is launched on an error.  With d_sum and d_raw both NULL nothing is sampled: the
 * coverage count takes one walk of each list whatever c is.
 */
int tia_merge_patch_grids_f32(const int32_t* d_rects, const float* d_affine, const float* d_maps, int64_t n, int64_t c, int64_t gh,
                              int64_t gw, int64_t h, int64_t w, const int32_t* d_tile_offsets, const int32_t* d_tile_items,
                              int64_t tile_h, int64_t tile_w, int32_t mode, float* d_sum, float* d_raw, int32_t* d_count, void* stream);


/* =======================================================================================
 * Reinhard colour normalisation (tools/stainnorm.py:222-367): OpenCV 8-bit RGB<->Lab
 * ===================================================================================== */

/* Fixed-point tables of OpenCV's RGB2Lab_b / Lab2RGBinteger (built on the host once). */
typedef struct tia_lab_tables {
    uint16_t gamma[256];      /* sRGBGammaTab_b                                   */
    uint16_t cbrt[3072];      /* LabCbrtTab_b                                     */
    uint16_t lab_y[256];      /* LabToYF_b[2*i]                                   */
    uint16_t lab_ify[256];    /* LabToYF_b[2*i+1]                                 */
    uint8_t inv_gamma[4096];  /* sRGBInvGammaTab_b                                */
    int32_t c_fwd[9];         /* 12-bit sRGB->XYZ/whitepoint                      */
    int32_t c_inv[9];         /* 12-bit XYZ*whitepoint->sRGB                      */
} tia_lab_tables;

/* Per-image histograms of the 8-bit Lab channels, ACCUMULATED into d_hist [n,3,256] u32
 * (cv2.cvtColor(RGB2LAB) + cv2.meanStdDev, stainnorm.py:309-315,362-364). */
int tia_lab_hist_u8(const uint8_t* d_img, int64_t n, int64_t h, int64_t w, const tia_lab_tables* d_tables,
                    uint32_t* d_hist, void* stream);

/* out = LAB2RGB(lut[c][ RGB2LAB(img)[c] ]) with one 3x256 uint8 LUT per image: the whole
 * ReinhardNormalizer.transform per-pixel chain (stainnorm.py:272-340) folded into tables. */
int tia_reinhard_apply_u8(const uint8_t* d_img, int64_t n, int64_t h, int64_t w, const tia_lab_tables* d_tables,
                          const uint8_t* d_lut /* [n,3,256] */, uint8_t* d_out, void* stream);

/* Per-image Lab statistics and the 3x256 LUTs of tia_reinhard_apply_u8 from the histograms of
 * tia_lab_hist_u8, entirely on the device (stainnorm.py:277-292,336-339,362-367):
 * mean / population std of the float32 channels (cv2.meanStdDev) in f64, then the reference's float32
 * chain per Lab byte.  d_chan_vals [3,256] f32 = channel value of every Lab byte (L/2.55, a-128, b-128);
 * target_means / target_stds: host pointers to 3 doubles each (copied at launch).
 * d_meanstd [n,6] f64 (means then stds) and d_flags [n] i32 (bit 0: a zero std, where the reference raises
 * ZeroDivisionError) are optional outputs; d_flags must be zero-initialised. */
int tia_reinhard_luts(const uint32_t* d_hist, int64_t n, const float* d_chan_vals, const double* target_means,
                      const double* target_stds, uint8_t* d_lut, double* d_meanstd, int32_t* d_flags, void* stream);

/* cv2.cvtColor 8-bit RGB2LAB (dir 0) / LAB2RGB (dir 1) of npix pixels. */
int tia_lab_convert_u8(const uint8_t* d_src, int64_t npix, const tia_lab_tables* d_tables, int32_t dir,
                       uint8_t* d_dst, void* stream);

/* ReinhardNormalizer.transform in ONE launch for a batch of patches (stainnorm.py:272-367): per patch RGB->Lab, the channel
 * moments (cv2.meanStdDev, float64 in NumPy's pairwise order), the three float32 byte tables, table -> Lab->RGB.  Up to 65536
 * pixels with h*w a multiple of 4 the Lab image stays in registers (no workspace: tia_reinhard_workspace_bytes returns 0); up to
 * 2^18 pixels with h*w a multiple of 256 it is parked as one dword per pixel in a per-workgroup slot of d_workspace
 * (tia_reinhard_workspace_bytes, 16-byte aligned; it stays in L2 / Infinity Cache).  Either way HBM carries 3 bytes in + 3 bytes
 * out per pixel.  d_img and d_out need 4-byte alignment.  Anything else (another h*w, a d_img or d_out that is not 4-byte aligned)
 * returns TIA_ESIZE with nothing launched: use tia_lab_hist_u8 + tia_reinhard_luts + tia_reinhard_apply_u8, which split a large
 * image over many workgroups (16-byte accesses when h*w is a multiple of 1024 and the buffers are 16-byte aligned, bytes
 * otherwise).  d_chan_vals: float32 [3,256] channel value of every Lab byte (host-built, :295-315);
 * target_means / target_stds: host double[3]; d_meanstd (nullable) [n,6]; d_flags (nullable) [n]: bit 0 = zero std (the reference
 * raises ZeroDivisionError). */
size_t tia_reinhard_workspace_bytes(int64_t n, int64_t h, int64_t w);
int tia_reinhard_transform_u8(const uint8_t* d_img, int64_t n, int64_t h, int64_t w, const tia_lab_tables* d_tables,
                              const float* d_chan_vals, const double* target_means, const double* target_stds, uint8_t* d_out,
                              double* d_meanstd, int32_t* d_flags, void* d_workspace, size_t workspace_bytes, void* stream);

/* ReinhardNormalizer.get_mean_std of n images in one launch (stainnorm.py:343-367): d_meanstd [n,6] = means of L/2.55, a-128, b-128,
 * then the population standard deviations.  Same shape limits as tia_reinhard_transform_u8 (TIA_ESIZE otherwise). */
int tia_lab_moments_u8(const uint8_t* d_img, int64_t n, int64_t h, int64_t w, const tia_lab_tables* d_tables,
                       const float* d_chan_vals, double* d_meanstd, int32_t* d_flags, void* stream);


/* out[i, j] = lut[i, img[i, j]]: one 256-byte table per image -- the intensity map of contrast_enhancer
 * (utils/misc.py:436-444: rescale_intensity over the [p2, p98] window, truncated to uint8) applied to a batch.
 *   d_img, d_out [n, len] u8   d_lut [n, 256] u8   n <= 65535 */
int tia_lut_apply_u8(const uint8_t* d_img, int64_t n, int64_t len, const uint8_t* d_lut, uint8_t* d_out, void* stream);

/* Box down-sampling of an HWC uint8 image by an integer factor: integer box sum * (1.0f / area), rounded half to even --
 * cv2.INTER_AREA at an integer scale, which is what the reference's slide thumbnail goes through
 * (utils/transforms.py imresize; wsicore/wsireader.py:1735-1786 tissue_mask -> slide_thumbnail).
 *   d_src [h,w,c]   d_out [h/factor, w/factor, c] */
int tia_box_downsample_u8(const uint8_t* d_src, int64_t h, int64_t w, int64_t c, int64_t factor, uint8_t* d_out, void* stream);

/* =======================================================================================
 * CNN epilogues (NHWC activations).  The convolutions themselves run on the MFMA kernels below, which
 * fuse this epilogue; these stand-alone passes serve a convolution output that has none.  With BatchNorm
 * folded into the weights every conv is followed by bias (+ residual) + ReLU, which PyTorch
 * executes as 2-3 separate full-tensor passes (models/architecture/vanilla.py:300-316 forward).
 * ===================================================================================== */
#define TIA_DT_F32 0
#define TIA_DT_F16 1
#define TIA_DT_BF16 2

/* In place: x[r,c] = act(x[r,c] + bias[c] (+ residual[r,c])), one pass.  c % 8 == 0. */
int tia_bias_act_nhwc(void* d_x, const void* d_bias, const void* d_residual, int64_t rows, int64_t c,
                      int32_t dtype, int32_t relu, void* stream);

/* out = maxpool3x3/s2/p1(relu(x + bias)) for the ResNet stem, one pass.
 * x [n,h,w,c] -> out [n,(h+1)/2,(w+1)/2,c].  c % 8 == 0. */
int tia_bias_relu_maxpool_nhwc(const void* d_x, const void* d_bias, int64_t n, int64_t h, int64_t w,
                               int64_t c, int32_t dtype, void* d_out, void* stream);

/* Patch reads from an in-memory slide level (WSIPatchDataset.__getitem__, models/dataset/dataset_abc.py:418-448;
 * tools/patchextraction.py:356-461 supplies the bounds): out[i] = slide[y0:y0+ph, x0:x0+pw] for d_bounds[i] =
 * (x0, y0, x1, y1) in baseline pixels, with `pad` (255) wherever the region leaves the slide.
 *   d_slide [sh,sw,c] u8   d_bounds [m,4] i32   d_out [m,ph,pw,c] u8 (ph*pw*c % 4 == 0, m <= 65535) */
int tia_gather_patches_u8(const uint8_t* d_slide, int64_t sh, int64_t sw, int64_t c, const int32_t* d_bounds,
                          int64_t m, int64_t ph, int64_t pw, int32_t pad, uint8_t* d_out, void* stream);

/* The same reads below the slide's resolution (VirtualWSIReader.read_bounds(..., resolution, units,
 * coord_space="resolution", pad_constant_values=255), wsicore/wsireader.py): d_bounds[i] = (x0, y0, x1, y1) in baseline
 * pixels with x1 - x0 == factor * pw and y1 - y0 == factor * ph; out[i] = the factor x factor box average of the region, `pad`
 * standing in for every source byte outside the slide (padding before averaging).  Rounding is cv2.INTER_AREA's at an
 * integer scale (resizeAreaFast): factor 2 -> (a + b + c + d + 2) >> 2, factor >= 3 -> integer box sum * (1.0f / factor^2)
 * rounded half to even (as tia_box_downsample_u8), factor 1 -> tia_gather_patches_u8 byte for byte.
 *   d_slide [sh,sw,c] u8, c in {1, 3}   d_bounds [m,4] i32   d_out [m,ph,pw,c] u8 (any ph*pw*c, any m)   1 <= factor <= 64 */
int tia_gather_area_patches_u8(const uint8_t* d_slide, int64_t sh, int64_t sw, int64_t c, const int32_t* d_bounds,
                               int64_t m, int64_t ph, int64_t pw, int64_t factor, int32_t pad, uint8_t* d_out, void* stream);

/* The same reads at any down-sampling ratio: out[i] = cv::resize(region_i, (pw, ph), INTER_AREA) of the hb x wb baseline region
 * whose top-left is (d_bounds[i][0], d_bounds[i][1]), `pad` standing in for every source byte outside the slide (padding before
 * resampling); x1, y1 are not read (every region is wb x hb).  Per axis scale = 1.0 / ((double)p / b), as cv::resize.  Both
 * scales integers within DBL_EPSILON (resizeAreaFast): equal -> tia_gather_area_patches_u8 byte for byte; unequal kx != ky ->
 * rint(float(box sum) * (1.0f / (kx * ky))).  Otherwise computeResizeAreaTab's taps (double, weights rounded to float once)
 * and ResizeArea_Invoker's float accumulation without fused multiply-add (horizontal per source row, then vertical), rint
 * half to even, saturated.
 *   d_slide [sh,sw,c] u8, c in {1, 3}   d_bounds [m,4] i32   d_out [m,ph,pw,c] u8 (any m)   1 <= wb / pw, hb / ph <= 64 */
int tia_gather_area_resize_u8(const uint8_t* d_slide, int64_t sh, int64_t sw, int64_t c, const int32_t* d_bounds, int64_t m,
                              int64_t hb, int64_t wb, int64_t ph, int64_t pw, int32_t pad, uint8_t* d_out, void* stream);

/* Reads above the slide's resolution: out[i] = cv::resize(region_i, (pw, ph), INTER_CUBIC) of the hb x wb baseline region whose
 * top-left is (d_bounds[i][0], d_bounds[i][1]), `pad` standing in for every source byte outside the slide (padding before
 * resampling); x1, y1 are not read.  resizeGeneric_'s fixed-point 8-bit path: per axis scale = 1.0 / ((double)p / b),
 * fx = (float)((d + 0.5) * scale - 0.5), s = floor(fx), f = fx - s; interpolateCubic's float coefficients (A = -0.75, no fused
 * multiply-add) each rounded half to even to a short of 2048 * coef; taps s - 1 .. s + 2 clamped to the region, not the slide;
 * int32 horizontal then vertical sums, (v + (1 << 21)) >> 22 saturated to [0, 255].
 *   d_slide [sh,sw,c] u8, c in {1, 3}   d_bounds [m,4] i32   d_out [m,ph,pw,c] u8 (any m, any pw * c)   pw >= wb, ph >= hb */
int tia_gather_cubic_resize_u8(const uint8_t* d_slide, int64_t sh, int64_t sw, int64_t c, const int32_t* d_bounds, int64_t m,
                               int64_t hb, int64_t wb, int64_t ph, int64_t pw, int32_t pad, uint8_t* d_out, void* stream);

/* =======================================================================================
 * ResNet convolutions on the matrix cores (models/architecture/vanilla.py:300-316 -> torchvision BasicBlock)
 * ===================================================================================== */

/* OIHW float32 weights -> the implicit GEMM's B matrix [kh][kw][cin][cout] (done once per model). */
int tia_conv_pack_weights_f32(const float* d_w_oihw, int64_t cout, int64_t cin, int64_t kh, int64_t kw,
                              float* d_packed, void* stream);

/* y = act(conv2d(x, w) + bias [+ residual]) for NHWC float32 tensors: implicit GEMM on v_mfma_f32_32x32x2_f32 (f32 in,
 * f32 accumulate: the reference's float32 arithmetic, vanilla.py:242), BatchNorm already folded into w / bias.
 *   d_x [n,h,w,cin]   d_w_packed [kh,kw,cin,cout]   d_bias [cout] or NULL   d_residual [n,ho,wo,cout] or NULL
 *   d_y [n,ho,wo,cout], ho = (h + 2 pad - kh) / stride + 1.   cin % 32 == 0, cout % 64 == 0, 16-byte aligned x / w. */
int tia_conv2d_nhwc_f32(const float* d_x, const float* d_w_packed, const float* d_bias, const float* d_residual,
                        float* d_y, int64_t n, int64_t h, int64_t w, int64_t cin, int64_t cout, int64_t kh,
                        int64_t kw, int64_t stride, int64_t pad, int32_t relu, void* stream);

/* The same convolution with the zero border given explicitly: `pad_top` / `pad_left` rows / columns of zeros in front,
 * and as many behind as the requested output size [ho, wo] reaches (taps outside the image read as zeros).  This is how
 * TensorFlow-style "same" padding of a strided convolution (0 in front, 1 behind: HoVer-Net's TFSamepaddingLayer,
 * models/architecture/hovernet.py:30-69) and "valid" convolutions (pad 0, ho = (h - kh) / stride + 1) are expressed.
 * Requires pad_top < kh, pad_left < kw and (ho - 1) * stride - pad_top < h (likewise for columns). */
int tia_conv2d_nhwc_f32_ex(const float* d_x, const float* d_w_packed, const float* d_bias, const float* d_residual,
                           float* d_y, int64_t n, int64_t h, int64_t w, int64_t cin, int64_t cout, int64_t kh,
                           int64_t kw, int64_t stride, int64_t pad_top, int64_t pad_left, int64_t ho, int64_t wo,
                           int32_t relu, void* stream);

/* Which block geometry tia_conv2d_nhwc_f32(_ex) / tia_conv2d_nhwc_h use for a 3x3 / stride-1 convolution of an [h, w] map to
 * [ho, wo] in float32 (diagnostics for tests and profiles; host only, no launch).  Returns 0: the slice implicit-GEMM kernel;
 * 1: tap reuse on 16 x 16 pixel blocks; 2: tap reuse, two images of at most 8 x 8 per block; 3: tap reuse on bands of geom[1]
 * rows of a geom[0]-column strip of the batch stacked into one tall image with a zero row between neighbours; 4: the same with
 * bands of geom[1] REAL rows (the zero rows are in the block's LDS patch, not among its GEMM rows).
 * geom[0..3] = strip width, rows per band, LDS row pitch (16-byte units), strips per image row (zeros unless 3 / 4). */
int tia_conv3x3_geometry(int64_t h, int64_t w, int64_t ho, int64_t wo, int64_t pad_top, int64_t pad_left, int32_t geom[4]);

/* Convolution over a THIN input (c * kw <= 32, e.g. the 3-channel 7x7 stem of HoVer-Net, models/architecture/hovernet.py:
 * 287-300 `conv0`): d_x [n,h,w,c] float32 NHWC, ALREADY padded horizontally by the caller ((wo-1)*stride + kw <= w, and at least 32 floats from the last output
 * column's first tap to the end of its row: (w - (wo-1)*stride) * c >= 32); rows are
 * padded by pad_top / ho like tia_conv2d_nhwc_f32_ex.  d_w_packed: [kh][32][cout] float32 with row kx * c + ch = w[o][ch][ky][kx]
 * and zero rows from kw * c on.  Same kernel and arithmetic as tia_conv2d_nhwc_f32 (K = 32 * kh). */
int tia_conv2d_thin_nhwc_f32(const float* d_x, const float* d_w_packed, const float* d_bias, float* d_y, int64_t n, int64_t h,
                             int64_t w, int64_t c, int64_t cout, int64_t kh, int64_t kw, int64_t stride, int64_t pad_top,
                             int64_t ho, int64_t wo, int32_t relu, void* stream);

/* The thin-input convolution with its output in y_dtype (additive at version 6): the same kernel and the same float32 arithmetic;
 * d_y [n,ho,wo,cout] of y_dtype, 16-byte aligned -- for TIA_DT_F16 / TIA_DT_BF16 the float32 value rounded once (nearest even), i.e.
 * exactly tia_conv2d_thin_nhwc_f32's output passed through one conversion: the 7x7 stem of the half-precision HoVer-Net.
 * TIA_DT_F32 is tia_conv2d_thin_nhwc_f32 itself. */
int tia_conv2d_thin_nhwc(const float* d_x, const float* d_w_packed, const float* d_bias, void* d_y, int32_t y_dtype, int64_t n,
                         int64_t h, int64_t w, int64_t c, int64_t cout, int64_t kh, int64_t kw, int64_t stride, int64_t pad_top,
                         int64_t ho, int64_t wo, int32_t relu, void* stream);

/* 1x1 convolution with FEW output channels (the class heads: cin = 64 -> cout <= 8; hovernet.py:196-199 `u0/conv`,
 * unet.py:336 `clf`), optionally with the BatchNorm + ReLU that precedes it applied on load:
 *   y[p][o] = bias[o] + sum_c w[o][c] * pre(x[p][c]),  pre(v) = relu(v * pre_scale[c] + pre_shift[c]) or v (both NULL).
 * d_x [npix,64], d_w [cout][64] (the OIHW tensor), d_y [npix,cout], all float32; HBM-bound (one read of x). */
int tia_conv1x1_head_nhwc_f32(const float* d_x, int64_t npix, const float* d_w, const float* d_bias, const float* d_pre_scale,
                              const float* d_pre_shift, int32_t cout, float* d_y, void* stream);
/* The same head on HALF activations (additive at version 6): d_x [npix,64] of `dtype` (TIA_DT_F16 | TIA_DT_BF16), 16-byte
 * aligned; weights, bias, pre_scale / pre_shift float32; pre(v) with product and sum rounded separately in float32; float32
 * accumulation; d_y [npix,cout] FLOAT32 logits, cout <= 8.  HBM-bound: 2 * 64 + 4 * cout bytes per pixel. */
int tia_conv1x1_head_nhwc_h(const void* d_x, int64_t npix, const float* d_w, const float* d_bias, const float* d_pre_scale,
                            const float* d_pre_shift, int32_t cout, int32_t dtype, float* d_y, void* stream);

/* tia_conv2d_nhwc_f32_ex with a second, post-activated output produced in the same epilogue:
 *   v  = act(conv(x, w) + bias [+ residual])      -> d_y   (may be NULL when only d_y2 is wanted)
 *   y2 = relu(v * post_scale[c] + post_shift[c])   -> d_y2  (required)
 * i.e. the BatchNorm + ReLU that follows a residual sum in a pre-activation network (HoVer-Net's next-unit "preact" /
 * "blk_bna", models/architecture/hovernet.py:100-147), applied while the sum is still in registers. */
int tia_conv2d_post_nhwc_f32(const float* d_x, const float* d_w_packed, const float* d_bias, const float* d_residual,
                             float* d_y, int64_t n, int64_t h, int64_t w, int64_t cin, int64_t cout, int64_t kh,
                             int64_t kw, int64_t stride, int64_t pad_top, int64_t pad_left, int64_t ho, int64_t wo,
                             int32_t relu, const float* d_post_scale, const float* d_post_shift, float* d_y2,
                             void* stream);

/* Winograd F(2x2, 3x3) form of the 3x3 / stride-1 float32 convolution (conv3x3_wino.hip; reference call sites: the 3x3 layers
 * behind CNNModel.forward, models/architecture/vanilla.py:242-253,300-316): 16 instead of 36 multiplies per 2 x 2 outputs on the same
 * float32 MFMA instruction, input transform in registers, weights transformed once at pack time in float64.  Same contract as
 * tia_conv2d_nhwc_f32_ex for kh = kw = 3, stride = 1 (pad_top / pad_left in 0..2, ho / wo given; bias + residual + ReLU fused), but
 * NOT bit-identical to it: float32 Winograd rounds differently from a direct float32 convolution (<= ~1e-5 relative, asserted in
 * tests/test_engine.py) -- which is why nothing dispatches to it implicitly.  cin % 16 == 0, cout % 64 == 0.
 *   tia_conv_pack_weights_wino_f32: OIHW [cout][cin][3][3] -> U = G g G^T, 16 * cin * cout floats in the kernel's stage layout
 *   ([pos 16][cin/16][h8 2][cout/64][hi 2][64 cout][4 channels], channel = 16 cs + 8 h8 + 4 hi + c4). */
int tia_conv_pack_weights_wino_f32(const float* d_w_oihw, int64_t cout, int64_t cin, float* d_packed, void* stream);
int tia_conv3x3_wino_nhwc_f32(const float* d_x, const float* d_u_packed, const float* d_bias, const float* d_residual, float* d_y,
                              int64_t n, int64_t h, int64_t w, int64_t cin, int64_t cout, int64_t pad_top, int64_t pad_left,
                              int64_t ho, int64_t wo, int32_t relu, void* stream);
/* Which block geometry tia_conv3x3_wino_nhwc_f32 uses for ONE launch over n images of [ho, wo] outputs (host only, no launch;
 * diagnostics for tests, like tia_conv3x3_geometry): 0 blocks of 16 x 16 outputs, 1 four images of at most 8 x 8 per block,
 * 2 windows of wty x wtx tiles of 2 x 2 outputs, wg windows per block, blocks running across images (chosen by the MFMA rows
 * kept busy over the whole batch, so it depends on n).  geom (may be NULL) = wg, wty, wtx, windows per image (zeros unless 2).
 * TIA_EINVAL for non-positive arguments.  Additive, same version (6). */
int tia_conv3x3_wino_geometry(int64_t n, int64_t ho, int64_t wo, int32_t geom[4]);

/* Winograd F(4x2, 3x3) form of the same convolution (conv3x3_wino42.hip): F(4, 3) over rows x F(2, 3) over columns, 24 instead of
 * 36 multiplies per 4 x 2 outputs (3 per output against F(2x2)'s 4), same contract and fused epilogue as tia_conv3x3_wino_nhwc_f32,
 * within the same 1e-5 (relative) of a direct float32 convolution.  cin % 16 == 0, cout % 64 == 0.
 *   tia_conv_pack_weights_wino42_f32: OIHW [cout][cin][3][3] -> U = G4 g G2^T (float64, rounded once), 24 * cin * cout floats
 *   ([pos 24][cin/16][h8 2][cout/64][hi 2][64 cout][4 channels], pos = 4 i + j, i: F(4, 3) row, j: F(2, 3) column).
 *   A batch beyond 2 GiB of input runs in equal groups like tia_conv2d_nhwc_f32's (ceil(n / k) images for the smallest k that fits),
 *   rounded up to whole blocks of four images for maps of at most 8 x 8 outputs.
 *   tia_conv3x3_wino_form: host-only route query (no launch) -- which form the fused resnet blocks take for a 3x3 / stride-1
 *   layer of this shape ("same" padding `pad`): 1 F(4x2), 0 F(2x2); TIA_EINVAL / TIA_ESIZE for shapes no Winograd form serves. */
int tia_conv_pack_weights_wino42_f32(const float* d_w_oihw, int64_t cout, int64_t cin, float* d_packed, void* stream);
int tia_conv3x3_wino42_nhwc_f32(const float* d_x, const float* d_u_packed, const float* d_bias, const float* d_residual, float* d_y,
                                int64_t n, int64_t h, int64_t w, int64_t cin, int64_t cout, int64_t pad_top, int64_t pad_left,
                                int64_t ho, int64_t wo, int32_t relu, void* stream);
int tia_conv3x3_wino_form(int64_t n, int64_t h, int64_t w, int64_t cin, int64_t cout, int64_t pad);

/* Winograd F(2x2, 3x3) with the 16 per-position GEMMs on the bf16 matrix cores, both operands split into three bf16 numbers
 * (conv3x3_wino_bf16x3.hip; additive, same version 6): float32 in, float32 accumulate, V = B^T d B in float32 and U = G g G^T
 * rounded once to float32 exactly as in tia_conv3x3_wino_nhwc_f32; only the multiplication differs (six exact bf16 products per
 * float32 product, another summation order).  Contract, checks and return codes of tia_conv3x3_wino_nhwc_f32; cin % 16 == 0,
 * cout % 64 == 0; blocks of 16 x 16 outputs, or of four images for maps of at most 8 x 8 outputs (bit-identical results).
 *   tia_conv_pack_weights_wino_bf16x3: d_parts [3][cout][cin][4][4] float32 holding bf16 VALUES (the planes hi, mid, lo of
 *   U[o][c][i][j]; the split and its check are the caller's, fused.pack_conv_weights_wino_split) -> 48 * cin * cout bf16 in the
 *   kernel's stage layout [cin/16][2 jh][cout/64][8 positions 2 i + jl][3 planes][2 k-chunks][64 cout][8 channels]
 *   (position (i, 2 jh + jl), channel = 16 cs + 8 chunk + e).
 *   tia_conv3x3_wino_bf16x3_serves: host-only route query (no launch) -- 1 where the fused resnet blocks take this form for a
 *   "same"-padded 3x3 / stride-1 layer under conv_algo="auto" (the layer classes that measured faster than the float32 form
 *   serving them, see the table at its definition), 0 otherwise; the negative code of tia_conv3x3_wino_form for shapes no
 *   Winograd form serves.  It answers for the classes that run on 16 x 16 blocks only.
 *   tia_conv3x3_wino_bf16x3_form (additive, same version 6): the route query the fused resnet blocks go by -- 1 where
 *   tia_conv3x3_wino_bf16x3_serves answers 1, 2 for the layer class taken on blocks of FOUR images of at most 8 x 8 outputs
 *   (tia_conv3x3_wino_bf16x3_nhwc_f32 takes that geometry by itself for such maps), 0 otherwise, negative as above;
 *   0 under the developer switch TIA_WINO_NO_SPLIT, and never 2 under TIA_WINO_SPLIT_NO_W8, which keeps the kernel on 16 x 16
 *   blocks for every map (both with TIA_DEV=1). */
int tia_conv_pack_weights_wino_bf16x3(const float* d_parts, int64_t cout, int64_t cin, void* d_packed, void* stream);
int tia_conv3x3_wino_bf16x3_nhwc_f32(const float* d_x, const void* d_u_packed3, const float* d_bias, const float* d_residual,
                                     float* d_y, int64_t n, int64_t h, int64_t w, int64_t cin, int64_t cout, int64_t pad_top,
                                     int64_t pad_left, int64_t ho, int64_t wo, int32_t relu, void* stream);
int tia_conv3x3_wino_bf16x3_serves(int64_t n, int64_t h, int64_t w, int64_t cin, int64_t cout, int64_t pad);
int tia_conv3x3_wino_bf16x3_form(int64_t n, int64_t h, int64_t w, int64_t cin, int64_t cout, int64_t pad);

/* Host-only query (no launch): which kernel tia_conv2d_nhwc_f32[_ex] runs a float32 convolution of this shape on --
 * 0: conv_mfma_f32_kernel (register-staged 128-pixel slices), 1: conv3x3_spatial_kernel (tap reuse; tia_conv3x3_geometry says
 * which block geometry), 2: conv1x1_ring_kernel (LDS-DMA ring over 256-pixel blocks: 1x1, and kh x kw taps gathered).  For
 * tests and bench.py (they ask instead of mirroring the dispatch rule).  It runs the entry point's own shape checks, batch split
 * (< 2 GiB of input per launch) and decision function: shapes the entry point rejects return the same negative code (TIA_EINVAL /
 * TIA_ESIZE, e.g. cin % 32 != 0); a batch that is split goes in EQUAL groups (ceil(n / k) images for the smallest k that fits:
 * 4096 images of 1 MiB run as 1366 + 1366 + 1364) and the answer is the route of that group size.  The ring's and the bands' fill
 * rules use the CU count of the calling thread's current device (256 without a device). */
int tia_conv2d_route_f32(int64_t n, int64_t h, int64_t w, int64_t cin, int64_t cout, int64_t kh, int64_t kw, int64_t stride,
                         int64_t pad_top, int64_t pad_left, int64_t ho, int64_t wo);

/* kh x kw float32 convolution on the BF16 matrix cores with BOTH operands split into three bf16 numbers (additive at version 6):
 * float32 in, float32 accumulate -- the arithmetic class of tia_conv2d_nhwc_f32 in another summation order.  a = hi + mid + lo
 * and w = hi + mid + lo exactly (round to nearest), every bf16 x bf16 product is exact in the float32 accumulator, and six of
 * the nine products (all but mid * lo, lo * mid, lo * lo: below 2^-23 |a w|) are accumulated per 16-channel step in the order
 * lo * hi, hi * lo, mid * mid, mid * hi, hi * mid, hi * hi (activation part x weight part).  The activations are split by the
 * kernel, the weights by the caller:
 *   tia_conv_pack_weights_bf16x3: d_parts_oihw [3][cout][cin][kh][kw] float32 holding hi, mid, lo -- the contract is that every
 *     part is a bf16 number (low 16 bits zero), that hi + mid + lo == w exactly and that every non-zero part is finite and
 *     normal (fused.split_stem_weights checks it) -> d_packed [kh][kw][cin/16][cout/128][3][2][128][8] bf16 (plane, 8-channel
 *     k-chunk, column, channel): cin % 16 == 0, cout % 128 == 0 (TIA_ESIZE otherwise).
 *   tia_conv2d_bf16x3_nhwc_f32: the arguments, checks and return codes of tia_conv2d_nhwc_f32 with cin % 16 == 0 and
 *     cout % 128 == 0, padding (pad_top, pad_left) on both sides, every pointer 16-byte aligned; batches beyond 2 GiB of input run
 *     in equal groups.  It runs at ANY batch size: routing is the caller's decision.  Non-finite activations, and activations
 *     with |a| >= 2^127 (2 - 2^-8) = 3.3961e38 (bf16(a) is infinite), make every output that reads them non-finite; parts below 2^-126 may be flushed to zero.
 *   tia_conv2d_bf16x3_serves (host only, no device needed): 1 where the engines' conv_algo="auto" takes this kernel -- the shape
 *     is one tia_conv2d_route_f32 puts on the LDS-DMA ring (2) AND its layer class measured faster than the float32 ring kernel
 *     (stride 2 and kh * kw * cin >= 64: DESIGN 4.27); 0 otherwise, and 0 under the developer switch TIA_CONV_NO_SPLIT (with TIA_DEV=1). */
int tia_conv_pack_weights_bf16x3(const float* d_parts_oihw, int64_t cout, int64_t cin, int64_t kh, int64_t kw, void* d_packed,
                                 void* stream);
int tia_conv2d_bf16x3_nhwc_f32(const float* d_x, const void* d_w_packed3, const float* d_bias, const float* d_residual, float* d_y,
                               int64_t n, int64_t h, int64_t w, int64_t cin, int64_t cout, int64_t kh, int64_t kw, int64_t stride,
                               int64_t pad_top, int64_t pad_left, int32_t relu, void* stream);
int tia_conv2d_bf16x3_serves(int64_t n, int64_t h, int64_t w, int64_t cin, int64_t cout, int64_t kh, int64_t kw, int64_t stride,
                             int64_t pad_top, int64_t pad_left, int64_t ho, int64_t wo);

/* 1x1 convolution (any stride, no padding) whose INPUT is activated on load:
 *   y = act(conv1x1(relu(x * pre_scale[c] + pre_shift[c]), w) + bias [+ residual])
 * -- the "preact/bn" + ReLU in front of conv1 of HoVer-Net's residual units 2..n (models/architecture/hovernet.py:100-147),
 * applied between the global load and the LDS store of the GEMM's A operand (product and sum rounded separately, like
 * batch_norm + relu): the unit reads the raw residual sum of the previous unit and the activated copy is never written.
 * pre_scale / pre_shift [cin], 16-byte aligned; other arguments as tia_conv2d_nhwc_f32_ex (ho = ceil(h / stride)). */
int tia_conv1x1_pre_nhwc_f32(const float* d_x, const float* d_pre_scale, const float* d_pre_shift, const float* d_w_packed,
                             const float* d_bias, const float* d_residual, float* d_y, int64_t n, int64_t h, int64_t w,
                             int64_t cin, int64_t cout, int64_t stride, int32_t relu, void* stream);

/* The ResNet stem in one kernel: y = maxpool3x3/s2/p1(relu(conv7x7/s2/p3(X) + bias)), 3 -> 64 channels, BatchNorm folded
 * into w / bias (CNNModel.forward -> torchvision conv1 / bn1 / relu / maxpool, models/architecture/vanilla.py:300-316).
 *   x_is_u8 != 0: d_x is the uint8 NHWC patch batch and X = x / 255 in float32 (correctly rounded division) -- `ToTensor`
 *   (models/dataset/classification.py:27-32) and the float32 cast of `_infer_batch` (vanilla.py:242-245) happen on load;
 *   x_is_u8 == 0: d_x is float32 NHWC and X = x.
 *   d_x [n,h,w,3]   d_w_packed [148,64] from tia_stem_pack_weights_f32   d_bias [64]
 *   d_y [n,hp,wp,64] of y_dtype (TIA_DT_F32; TIA_DT_F16 / TIA_DT_BF16: rounded once, for the half-precision trunk),
 *   hp = ((h-1)/2)/2 + 1 (likewise wp); arithmetic: a float32 fmaf chain in (ky, kx, c) order on the matrix cores.
 *   d_conv_out (may be NULL): also write relu(conv + bias) BEFORE the pooling, [n,ho,wo,64] float32, ho = (h-1)/2 + 1 -- the
 *   first skip connection of the UNet decoder (models/architecture/unet.py:356-372, ResNetEncoder features).
 * Limits of every tia_stem_conv7x7_pool_* entry point (tests/test_stem_reference.py): TIA_EINVAL for a null d_x / d_w_packed /
 * d_bias / d_y, n, h or w <= 0, a y_dtype that is no TIA_DT_* value, d_y or the packed weights not 16-byte aligned, a float32 d_x
 * not 4-byte aligned (a uint8 d_x may start at any byte); TIA_ESIZE for ONE image of more than 2^31 - 1 bytes (h * w * 3 uint8,
 * h * w * 12 float32), refused before any launch.  Any image size below that is served (also below the 7x7 window); a batch of
 * more than 2^31 - 1 bytes runs in equal groups of whole images, one launch each. */
int tia_stem_conv7x7_pool_nhwc(const void* d_x, int32_t x_is_u8, const float* d_w_packed, const float* d_bias, void* d_y,
                               int32_t y_dtype, float* d_conv_out, int64_t n, int64_t h, int64_t w, void* stream);
/* The same kernel and the same float32 arithmetic with the pre-pool output in y_dtype as well (additive at version 6):
 *   d_conv_out (may be NULL) [n,ho,wo,64] of y_dtype, 16-byte aligned -- for TIA_DT_F16 / TIA_DT_BF16 the float32 value rounded
 *   once (round to nearest even), i.e. exactly tia_stem_conv7x7_pool_nhwc's float32 output passed through one conversion: the
 *   first skip connection of the half-precision UNet.  tia_stem_conv7x7_pool_nhwc is this entry point with a float32 d_conv_out. */
int tia_stem_conv7x7_pool_conv_nhwc(const void* d_x, int32_t x_is_u8, const float* d_w_packed, const float* d_bias, void* d_y,
                                    int32_t y_dtype, void* d_conv_out, int64_t n, int64_t h, int64_t w, void* stream);

/* The same stem on the HALF matrix cores, for compute_dtype = float16 | bfloat16 of the engines (an extension: the reference runs
 * float32; `model.half()(ToTensor(x).half())` is what it mirrors): x / 255 and the weights rounded to `dtype`, float32
 * accumulation (v_mfma_f32_32x32x16_f16 / _bf16, K = 7 * 24 = 168 padded to 176), bias + ReLU + max-pool in float32, one rounding
 * of the pooled result.  d_w_packed_h: [22][64][8] halves from tia_stem_pack_weights_h (row k = 24 ky + 3 kx + c of the
 * OIHW float32 tensor); d_y [n,hp,wp,64] of `dtype` (TIA_DT_F16 | TIA_DT_BF16). */
int tia_stem_pack_weights_h(const float* d_w_oihw, int32_t dtype, void* d_packed, void* stream);
int tia_stem_conv7x7_pool_nhwc_h(const void* d_x, int32_t x_is_u8, const void* d_w_packed_h, const float* d_bias, void* d_y,
                                 int32_t dtype, int64_t n, int64_t h, int64_t w, void* stream);
/* OIHW [64,3,7,7] float32 -> [148,64]: rows (ky, kx, c), one zero row at the end. */
int tia_stem_pack_weights_f32(const float* d_w_oihw, float* d_packed, void* stream);

/* The uint8 stem on the bf16 matrix cores with EXACTLY SPLIT float32 weights (additive at version 6): float32 in, float32
 * accumulate -- the arithmetic class of tia_stem_conv7x7_pool_nhwc, another summation order, several times less matrix time.
 *   - a byte 0..255 is a bf16 number; a float32 weight is the sum of three bf16 numbers, w = hi + mid + lo (hi = bf16(w),
 *     mid = bf16(w - hi), lo = bf16(w - hi - mid), round to nearest); every product byte * part has at most 16 significant
 *     bits and is exact in the float32 accumulator of v_mfma_f32_32x32x16_bf16.  S = sum(byte * w) is therefore formed with no
 *     rounding other than that of the float32 accumulation (order: k-steps of 16 with k = 24 ky + 3 kx + c, planes hi, mid, lo
 *     within a step, one accumulator);
 *   - y = maxpool3x3/2(relu(fl(S / 255) + bias)): the quotient correctly rounded, the bias a separate float32 addition.
 * THE CALLER SPLITS AND CHECKS: d_parts_oihw is [3][64][3][7][7] float32 holding hi, mid, lo; the contract is that every part
 * is a bf16 number (low 16 bits zero), that hi + mid + lo == w exactly and that every non-zero part is finite and normal.
 * Weights without such a split (non-finite, next to overflow, |w| < ~1e-33) belong on tia_stem_conv7x7_pool_nhwc.
 *   d_packed / d_w_packed3: [3][22][64][8] bf16 (the layout of tia_stem_pack_weights_h per plane), 16-byte aligned
 *   d_x [n,h,w,3] uint8 (any byte alignment)   d_bias [64]   d_y [n,hp,wp,64] float32, 16-byte aligned. */
int tia_stem_pack_weights_bf16x3(const float* d_parts_oihw, void* d_packed, void* stream);
int tia_stem_conv7x7_pool_nhwc_u8x3(const uint8_t* d_x, const void* d_w_packed3, const float* d_bias, float* d_y, int64_t n,
                                    int64_t h, int64_t w, void* stream);

/* Half-precision sibling of tia_conv2d_nhwc_f32 for `compute_dtype="float16"|"bfloat16"` runs of the engines (an extension:
 * the reference computes in float32, vanilla.py:242; results are held to its own 1e-3 tolerance on the probabilities,
 * tests/engines/test_patch_predictor.py:712-722): implicit GEMM on v_mfma_f32_32x32x16_f16 / _bf16, float32 accumulate;
 * bias + residual + ReLU in float32, ONE rounding to half on the way out.
 *   d_x [n,h,w,cin] half   d_w_packed from tia_conv_pack_weights_h   d_bias [cout] float32 or NULL
 *   d_residual [n,ho,wo,cout] half or NULL   d_y [n,ho,wo,cout] half.   cin % 32 == 0, cout % 64 == 0, 16-byte aligned.
 * Argument codes: null pointers, a dtype that is not a half type and scale / shift without d_y2 are TIA_EINVAL; then the shape
 * checks of tia_conv2d_nhwc_f32 in its order -- a non-positive size (cin and cout included), stride or a negative pad TIA_EINVAL,
 * channel multiples TIA_ESIZE, kernel size / padding TIA_EINVAL, output range TIA_EINVAL -- then misaligned pointers TIA_EINVAL,
 * then an image or weight tensor beyond 2 GiB TIA_ESIZE.  Where two faults coincide the first in this order is reported. */
int tia_conv2d_nhwc_h(const void* d_x, const void* d_w_packed, const float* d_bias, const void* d_residual, void* d_y,
                      int64_t n, int64_t h, int64_t w, int64_t cin, int64_t cout, int64_t kh, int64_t kw, int64_t stride,
                      int64_t pad, int32_t dtype, int32_t relu, void* stream);
/* The extended form (additive at version 6), the half sibling of tia_conv2d_nhwc_f32_ex + tia_conv2d_post_nhwc_f32:
 *   - the zero border given explicitly: pad_top / pad_left rows / columns in front and as many behind as [ho, wo] reaches
 *     (pad_top < kh, pad_left < kw, (ho - 1) * stride - pad_top < h, likewise for columns) -- TensorFlow "same" padding of
 *     HoVer-Net's strided 3x3 layers (0 in front, 1 behind on even maps);
 *   - an optional second output from the same epilogue: with v = act(conv + bias [+ residual]) in float32,
 *       d_y  (may be NULL when d_y2 is given) = half(v)
 *       d_y2 (may be NULL)                    = half(relu(v * post_scale[c] + post_shift[c]))
 *     computed from v BEFORE it is rounded, product and sum rounded separately in float32, then ONE rounding to half.
 *     post_scale / post_shift: float32 [cout], 16-byte aligned, required with d_y2 and refused (TIA_EINVAL) without it.
 * tia_conv2d_nhwc_h is this entry point with symmetric pads and no second output (and may take the tap-reuse kernel for a
 * 3x3 / stride-1 layer, which this one never does).  Channel counts as there (TIA_ESIZE); misaligned pointers TIA_EINVAL. */
int tia_conv2d_nhwc_h_ex(const void* d_x, const void* d_w_packed, const float* d_bias, const void* d_residual, void* d_y,
                         int64_t n, int64_t h, int64_t w, int64_t cin, int64_t cout, int64_t kh, int64_t kw, int64_t stride,
                         int64_t pad_top, int64_t pad_left, int64_t ho, int64_t wo, int32_t dtype, int32_t relu,
                         const float* d_post_scale, const float* d_post_shift, void* d_y2, void* stream);
/* OIHW float32 weights -> [kh][kw][cin/8][cout][8] halves of `dtype` (a lane's 8 k-values of its column contiguous). */
int tia_conv_pack_weights_h(const float* d_w_oihw, int64_t cout, int64_t cin, int64_t kh, int64_t kw, int32_t dtype,
                            void* d_packed, void* stream);

/* y = act(x * scale[c] + shift[c]) on NHWC float32 ([rows, c], c % 4 == 0; y may alias x): an inference-mode
 * BatchNorm (+ ReLU) that sits in FRONT of a convolution and therefore cannot be folded into one -- the pre-activation
 * units of HoVer-Net (models/architecture/hovernet.py:72-261: "preact_bna" / "blk_bna"). */
int tia_scale_shift_act_nhwc_f32(const float* d_x, const float* d_scale, const float* d_shift, float* d_y, int64_t rows,
                                 int64_t c, int32_t relu, void* stream);

/* The same on a view: d_x points at element [0,0,0,0] of a window of a wider NHWC buffer (a channel prefix and a spatial
 * crop), strides in elements (multiples of 4, 16-byte aligned base, x_pixel_stride >= c); y [n,h,w,c] dense.  Lets the
 * dense units of HoVer-Net (hovernet.py:72-98) grow their feature stack in place instead of re-concatenating it. */
int tia_scale_shift_act_view_nhwc_f32(const float* d_x, int64_t x_image_stride, int64_t x_row_stride, int64_t x_pixel_stride,
                                      const float* d_scale, const float* d_shift, float* d_y, int64_t n, int64_t h,
                                      int64_t w, int64_t c, int32_t relu, void* stream);

/* The half form (additive at version 6): d_x a view of an NHWC buffer of `dtype` (TIA_DT_F16 | TIA_DT_BF16), strides in elements
 * (multiples of 8, 16-byte aligned base, x_pixel_stride >= c, else TIA_EINVAL); c % 8 == 0 (else TIA_ESIZE); scale / shift
 * float32 [c]; d_y [n,h,w,c] dense of `dtype`.  p = float(x) * scale; a = p + shift; max(a, 0) (relu != 0), each step rounded on
 * its own in float32, ONE rounding to half.  The pre-activations and `blk_bna` of HoVer-Net's dense blocks in half. */
int tia_scale_shift_act_view_nhwc_h(const void* d_x, int64_t x_image_stride, int64_t x_row_stride, int64_t x_pixel_stride,
                                    const float* d_scale, const float* d_shift, void* d_y, int64_t n, int64_t h, int64_t w,
                                    int64_t c, int32_t relu, int32_t dtype, void* stream);

/* Grouped "valid" k x k convolution, stride 1, 32 input and 8 output channels per group (the second convolution of
 * HoVer-Net's dense units, hovernet.py:86-88: Conv2d(128, 32, k, groups=4)); float32 NHWC.
 *   d_x [n,h,w,groups*32] dense;  d_w_packed [groups][k][k][32][8] (from OIHW [groups*8, 32, k, k]);
 *   y: element [b, oy, ox, c] at d_y + b*y_image_stride + oy*y_row_stride + ox*y_pixel_stride + c (strides in
 *   elements, multiples of 4), ho = h - k + 1 -- so the result can land in a channel slice of a wider buffer.
 * Other channel counts -> TIA_ESIZE. */
int tia_grouped_conv_valid_nhwc_f32(const float* d_x, const float* d_w_packed, float* d_y, int64_t y_image_stride,
                                    int64_t y_row_stride, int64_t y_pixel_stride, int64_t n, int64_t h, int64_t w,
                                    int64_t groups, int64_t cin_per_group, int64_t cout_per_group, int64_t k, void* stream);

/* The half form (additive at version 6), on v_mfma_f32_16x16x32_f16 / _bf16 (one tap of one group is its K = 32):
 *   d_x [n,h,w,groups*32] dense of `dtype` (TIA_DT_F16 | TIA_DT_BF16);
 *   d_w_packed from tia_grouped_conv_pack_weights_h: OIHW float32 [groups*8, 32, k, k] rounded ONCE to `dtype`, laid out
 *   [groups][k][k][4 chunks of 8 input channels][8 outputs][8 halves];
 *   float32 accumulation, ONE rounding; y of `dtype` through y_image_stride / y_row_stride / y_pixel_stride in elements
 *   (multiples of 8, base 16-byte aligned, else TIA_EINVAL), so the result lands in its 32-channel slice and window of a dense
 *   block's feature buffer.  k in {3, 5} (HoVer-Net's two modes: the taps are unrolled); other k and other channel counts per
 *   group -> TIA_ESIZE.  Nothing is launched on an error. */
int tia_grouped_conv_pack_weights_h(const float* d_w_oihw, int64_t groups, int64_t k, int32_t dtype, void* d_packed, void* stream);
int tia_grouped_conv_valid_nhwc_h(const void* d_x, const void* d_w_packed, void* d_y, int64_t y_image_stride, int64_t y_row_stride,
                                  int64_t y_pixel_stride, int64_t n, int64_t h, int64_t w, int64_t groups, int64_t cin_per_group,
                                  int64_t cout_per_group, int64_t k, int32_t dtype, void* stream);

/* Grouped 3x3 convolution, padding 1, stride 1 or 2, with the bias and ReLU fused: the grouped conv2 of the ResNeXt Bottleneck
 * (models/architecture/resnet.py: Conv2d(width, width, 3, stride, 1, groups=32)); float32 NHWC, on the vector ALU.
 *   d_x [n,h,w,groups*cg] dense;  d_w_packed [groups][3][3][cg][cg] (in-group input channel, then output channel: from OIHW
 *   [groups*cg, cg, 3, 3]);  d_bias [groups*cg] float32 or NULL;  d_y [n,ho,wo,groups*cg], ho = (h - 1) / stride + 1.
 *   relu != 0: y = max(conv + bias, 0).  cg = channels per group in {4, 8, 16, 32, 64} (other widths -> TIA_ESIZE); 16-byte
 *   aligned pointers.
 * Additive, same version (6). */
int tia_conv3x3_grouped_nhwc_f32(const float* d_x, const float* d_w_packed, const float* d_bias, float* d_y, int64_t n, int64_t h,
                                 int64_t w, int64_t groups, int64_t channels_per_group, int64_t stride, int32_t relu, void* stream);

/* out[b, Y, X, :] = x[b, Y/2, X/2, :] + y[b, Y, X, :] on NHWC float32: nearest x2 upsampling fused with the decoder's
 * skip-connection add (models/architecture/hovernet.py:447-449, utils.py:202-243).  x [n,h,w,c]; y a (possibly
 * centre-cropped) view of an NHWC tensor with contiguous channels: d_y points at its first element,
 * y_image_stride / y_row_stride in elements (multiples of 4, 16-byte aligned base); out [n,2h,2w,c]; c % 4 == 0. */
int tia_upsample2x_add_nhwc_f32(const float* d_x, const float* d_y, int64_t y_image_stride, int64_t y_row_stride,
                                float* d_out, int64_t n, int64_t h, int64_t w, int64_t c, void* stream);
/* The same followed by relu(. * scale[c] + shift[c]) (both NULL: plain sum): up-sampling, skip add and the pre-activation of
 * a UNet decoder block (models/architecture/unet.py:193-240, 356-417) in one pass. */
int tia_upsample2x_add_act_nhwc_f32(const float* d_x, const float* d_y, int64_t y_image_stride, int64_t y_row_stride,
                                    const float* d_scale, const float* d_shift, float* d_out, int64_t n, int64_t h,
                                    int64_t w, int64_t c, void* stream);
/* The half form (additive at version 6): x [n,h,w,c] and out [n,2h,2w,c] dense NHWC of `dtype` (TIA_DT_F16 | TIA_DT_BF16), y a
 * (cropped) view of that type with y_image_stride / y_row_stride in elements; scale / shift float32 [c] (both NULL: plain sum).
 * float32 arithmetic, every step rounded on its own: s = float(x) + float(y); p = s * scale; a = p + shift; max(a, 0); ONE
 * rounding to half (nearest even).  Every x vector is read once for its 2 x 2 output block: 4.5 bytes per output element.
 * c % 8 == 0 (else TIA_ESIZE); bases 16-byte aligned and strides multiples of 8 elements (else TIA_EINVAL); 64-bit offsets. */
int tia_upsample2x_add_act_nhwc_h(const void* d_x, const void* d_y, int64_t y_image_stride, int64_t y_row_stride,
                                  const float* d_scale, const float* d_shift, void* d_out, int64_t n, int64_t h, int64_t w,
                                  int64_t c, int32_t dtype, void* stream);

/* y[b, oy, ox, :] = mean of the 2 x 2 window of x at rows 2 oy, 2 oy + 1 and columns 2 ox, 2 ox + 1 on NHWC float32: AvgPool2d(2,
 * stride=2) of the plain UNet encoder (models/architecture/unet.py: UnetEncoder).  x [n,h,w,c] dense; y [n,h/2,w/2,c] dense (floor
 * division: a last odd row or column is not read).  The arithmetic is fixed: s = ((x00 + x01) + x10) + x11 with xrc = row r, column c
 * of the window, every sum rounded in float32, then y = s * 0.25f -- the order of torch's avg_pool2d, bit for bit.
 * c % 4 == 0 (else TIA_ESIZE); h >= 2, w >= 2, n > 0, non-null 16-byte aligned pointers (else TIA_EINVAL); 64-bit offsets; nothing is
 * launched on an error return.  Additive, same version (6). */
int tia_avgpool2x2_nhwc_f32(const float* d_x, float* d_y, int64_t n, int64_t h, int64_t w, int64_t c, void* stream);
/* The half form (additive at version 6): x and y of `dtype` (TIA_DT_F16 | TIA_DT_BF16); the four inputs widened to float32, the same
 * three sums and product, ONE rounding to half (nearest even).  c % 8 == 0 (else TIA_ESIZE); otherwise as above. */
int tia_avgpool2x2_nhwc_h(const void* d_x, void* d_y, int64_t n, int64_t h, int64_t w, int64_t c, int32_t dtype, void* stream);

/* out[b, Y, X, 0:cx] = act(x[b, Y/2, X/2, :]), out[b, Y, X, cx:cx+cy] = act(y[b, Y, X, :]) on NHWC float32: nearest x2 upsampling
 * fused with the channel concatenation of a UNet decoder's skip connection (models/architecture/unet.py: skip_type="concat") and,
 * with scale / shift, the BatchNorm + ReLU of a pre-activation decoder block.  x [n,h,w,cx], y [n,2h,2w,cy], out [n,2h,2w,cx+cy], all
 * dense; scale / shift float32 [cx+cy], both given or both NULL.  NULL: act is the identity and the pass is a pure copy (bit-equal
 * outputs).  Given: p = v * scale[ch]; a = p + shift[ch]; max(a, 0), product and sum rounded separately (no fused multiply-add).
 * Every x vector is read once for its 2 x 2 outputs.  cx % 4 == 0 and cy % 4 == 0 (else TIA_ESIZE); positive sizes, non-null 16-byte
 * aligned pointers (else TIA_EINVAL); 64-bit offsets; nothing is launched on an error return.  Additive, same version (6). */
int tia_upsample2x_concat_act_nhwc_f32(const float* d_x, const float* d_y, const float* d_scale, const float* d_shift, float* d_out,
                                       int64_t n, int64_t h, int64_t w, int64_t cx, int64_t cy, void* stream);
/* The half form (additive at version 6): x, y and out of `dtype` (TIA_DT_F16 | TIA_DT_BF16), scale / shift float32.  With an affine
 * v is widened to float32 first and the result rounded ONCE to half (nearest even); without, the halves are copied as they are.
 * cx % 8 == 0 and cy % 8 == 0 (else TIA_ESIZE); otherwise as above. */
int tia_upsample2x_concat_act_nhwc_h(const void* d_x, const void* d_y, const float* d_scale, const float* d_shift, void* d_out,
                                     int64_t n, int64_t h, int64_t w, int64_t cx, int64_t cy, int32_t dtype, void* stream);

/* =======================================================================================
 * Vision Transformer backbones in fp16 / bf16 (models/architecture/vit.py, vit_fused.py: timm's VisionTransformer as
 * the reference's TimmBackbone builds it -- UNI = ViT-L/16).  The Linear layers are tia_conv2d_nhwc_h with kh = kw = 1 on the
 * tokens as an [n, S, 1, C] map; these entry points are everything around them.  Additive, same version (6).  `dtype` is
 * TIA_DT_F16 | TIA_DT_BF16 (anything else TIA_EINVAL); null pointers, non-positive sizes and pointers that are not 16-byte aligned
 * are TIA_EINVAL, sizes a kernel does not take TIA_ESIZE; nothing is launched on an error return; 64-bit offsets.
 * ===================================================================================== */

/* Fused multi-head attention, forward: out[b,i,h,:] = softmax_j(scale * q[b,i,h,:] . k[b,j,h,:]) v[b,:,h,:] on
 * v_mfma_f32_16x16x32_f16 / _bf16 without materialising the scores (online softmax, 64 queries x 64 keys per step).
 *   d_qkv [n, s, 3, heads, head_dim] of `dtype` -- the qkv Linear's own output order   d_out [n, s, heads * head_dim] of `dtype`
 * float32 scores, maximum and sum (the sum over the unrounded probabilities); the probabilities are rounded once to `dtype` for
 * the second product, the output O / l once.  Any s >= 1: keys beyond s contribute exactly 0, query rows beyond s are not stored.
 * head_dim is 64 or 80 (Virchow / Virchow2), anything else TIA_ESIZE; scale must be positive and finite (TIA_EINVAL). */
int tia_mha_fwd_h(const void* d_qkv, void* d_out, int64_t n, int64_t s, int64_t heads, int64_t head_dim, float scale, int32_t dtype,
                  void* stream);

/* LayerNorm over the last axis: y[r,:] = (x[r,:] - mean) / sqrt(var + eps) * gamma + beta, mean first and then the variance of
 * the centred values, float32 throughout, ONE rounding.
 *   d_x: row r starts at element r * row_stride of `dtype` (row_stride >= c, % 8 == 0: the final norm reads the class tokens
 *   only, row_stride = S * D)   d_gamma, d_beta [c] float32   d_y [rows, c] dense, of `dtype` or (out_f32 != 0) float32.
 * c % 8 == 0 and c <= 8192 (else TIA_ESIZE). */
int tia_layernorm_rows_h(const void* d_x, int64_t row_stride, const float* d_gamma, const float* d_beta, float eps, void* d_y,
                         int64_t rows, int64_t c, int32_t dtype, int32_t out_f32, void* stream);

/* Exact GELU in place on `count` halves: 0.5 x (1 + erf(x / sqrt 2)) in float32, ONE rounding.  count % 8 == 0 (else TIA_ESIZE). */
int tia_gelu_rows_h(void* d_x, int64_t count, int32_t dtype, void* stream);

/* The patch embedding's im2col: d_x [n,h,w,3] NHWC of x_dtype (TIA_DT_F32, or `dtype` itself: copied as it is) ->
 * d_tokens [n, (h/patch) * (w/patch), patch * patch * 3] of `dtype`, patches in raster order, the values of a patch in
 * (ky, kx, channel) order -- the k order of a [D,3,p,p] weight permuted to [D,p,p,3], so that the embedding is one 1x1
 * GEMM with cin = 3 p^2.  patch % 8 == 0, h % patch == 0 and w % patch == 0 (else TIA_ESIZE). */
int tia_vit_patchify_h(const void* d_x, int32_t x_dtype, void* d_tokens, int64_t n, int64_t h, int64_t w, int64_t patch,
                       int32_t dtype, void* stream);

/* Token assembly: d_out [n, 1+g, d] of `dtype` with out[b,0] = cls + pos[0] and out[b,1+i] = tokens[b,i] + pos[1+i];
 *   d_tokens [n,g,d] of `dtype`   d_cls [d], d_pos [1+g, d] float32.   float32 add, ONE rounding.  d % 8 == 0 (else TIA_ESIZE). */
int tia_vit_assemble_tokens_h(const void* d_tokens, const float* d_cls, const float* d_pos, void* d_out, int64_t n, int64_t g,
                              int64_t d, int32_t dtype, void* stream);

/* The foundation models' additions (UNI2, H-optimus-0 / -1, prov-gigapath: register tokens, a position table without a class
 * entry, a 14-pixel patch, timm's SwiGLUPacked).  Additive, same version (6); the contract of the family above. */

/* Packed SwiGLU on the fc1 output: y[r,j] = silu(x[r,j]) * x[r,H+j] with silu(t) = t / (1 + exp(-t)) -- the FIRST half is the gate.
 *   d_x [rows, 2H], d_y [rows, H] of `dtype`; not in place.  float32 arithmetic, ONE rounding; evaluated through exp(-|t|), so no
 * gate overflows: a large negative gate gives the tiny product (or a signed zero), a large positive one x[r,j] * x[r,H+j].
 * H % 8 == 0 (else TIA_ESIZE). */
int tia_swiglu_rows_h(const void* d_x, void* d_y, int64_t rows, int64_t hidden, int32_t dtype, void* stream);

/* tia_vit_patchify_h for any patch >= 1, with padded rows: d_tokens [n, (h/patch) * (w/patch), k_pad] of `dtype`; columns
 * 0 .. 3 patch^2 - 1 are the patch in (ky, kx, channel) order, columns 3 patch^2 .. k_pad - 1 exact zeros, so that the embedding
 * stays one 1x1 GEMM (cin = k_pad, weight rows zero-padded alike) when 3 patch^2 is no multiple of 32 (patch 14: 588 -> 608).
 *   d_x [n,h,w,3] NHWC of x_dtype (TIA_DT_F32, or `dtype` itself: copied as it is).
 * h % patch == 0, w % patch == 0, k_pad % 32 == 0 and k_pad >= 3 patch^2 (else TIA_ESIZE). */
int tia_vit_patchify_pad_h(const void* d_x, int32_t x_dtype, void* d_tokens, int64_t n, int64_t h, int64_t w, int64_t patch,
                           int64_t k_pad, int32_t dtype, void* stream);

/* Token assembly with register tokens: d_out [n, 1+R+g, d] of `dtype` with out[b,0] = cls (+ pos[0] if pos_has_cls),
 * out[b,1+r] = reg[r], out[b,1+R+i] = tokens[b,i] + pos[i + pos_has_cls].
 *   d_tokens [n,g,d] of `dtype`   d_cls [d], d_reg [R,d] (NULL exactly when R == 0), d_pos [g + pos_has_cls, d] float32
 *   pos_has_cls 0 | 1 (anything else TIA_EINVAL).   float32 add, ONE rounding; R = 0 with pos_has_cls = 1 is
 * tia_vit_assemble_tokens_h bit for bit.  d % 8 == 0 (else TIA_ESIZE). */
int tia_vit_assemble_prefix_h(const void* d_tokens, const float* d_cls, const float* d_reg, const float* d_pos, int32_t pos_has_cls,
                              void* d_out, int64_t n, int64_t g, int64_t reg_tokens, int64_t d, int32_t dtype, void* stream);

/* Virchow / Virchow2 (1280 / 16 = 80 per head, a class + mean-patch output): tia_mha_fwd_h takes head_dim 80 (above), and the last
 * step of the graph is the pooled final norm.  Additive, same version (6); the contract of the family above. */

/* Class + mean-patch pooling of the final LayerNorm: out[b, :d] = LN(x[b,0]), out[b, d:] = mean_{i = skip .. s-1} LN(x[b,i])
 * (timm's global_pool="token" beside the mean of the patch tokens, the register tokens 1 .. skip-1 left out).
 *   d_x [n,s,d] of `dtype`   d_gamma, d_beta [d] float32   d_out [n, 2d] float32
 * Every row is normalised in float32 as in tia_layernorm_rows_h (mean first, then the variance of the centred values) and NOT rounded
 * to `dtype`; the normalised rows are summed in float32 in a fixed order (no atomics; one workgroup per image, so an image's result
 * is bit-identical whatever n is) and the affine is applied once to the mean (g mean(y) + b == mean(g y + b)).
 * skip < 1 or skip >= s is TIA_EINVAL; d % 8 == 0 and d <= 8192 (else TIA_ESIZE). */
int tia_vit_cls_mean_pool_h(const void* d_x, const float* d_gamma, const float* d_beta, float eps, float* d_out, int64_t n, int64_t s,
                            int64_t skip, int64_t d, int32_t dtype, void* stream);

/* residual_dtype="float32" (FusedViT with autocast's residual stream): x is a float32 [n,S,D] tensor from token assembly to the final
 * norm, the proj / fc2 GEMMs write half BRANCHES without a residual, and the three entry points below are the float32-stream forms of
 * tia_layernorm_rows_h, tia_vit_assemble_prefix_h and tia_vit_cls_mean_pool_h.  Additive, same version (6); the contract of the
 * family above: 16-byte accesses, 64-bit offsets, float32 arithmetic, no atomics; the entry launches and neither allocates nor syncs.
 * `dtype` is the half type of the branch / tokens (TIA_DT_F16 | TIA_DT_BF16, else TIA_EINVAL). */

/* x[r,:] += float(branch[r,:]) in place, then y[r,:] = LN(x[r,:]) * gamma + beta -- either part optional, one pass over x.
 *   d_x float32, row r at element r * x_row_stride (>= c, % 4 == 0)
 *   d_branch of `dtype`, row r at element r * branch_row_stride (>= c, % 8 == 0), or NULL: x is only read and stays bit-identical
 *   d_y [rows,c] dense, of y_dtype (`dtype` itself: ONE rounding; or TIA_DT_F32), or NULL: the add alone (gamma, beta, eps, y_dtype
 *     are not looked at)
 * The add is ONE IEEE float32 add per element, written back by the lane that read it; the LayerNorm is tia_layernorm_rows_h's,
 * operation for operation, on the float32 sum (mean first, then the variance of the centred values, folded by lane exchanges).
 * TIA_EINVAL: d_branch and d_y both NULL, a null d_x (or affine beside a d_y), a misaligned pointer, a bad stride or dtype, eps < 0.
 * c % 8 == 0 and c <= 8192 (else TIA_ESIZE). */
int tia_add_layernorm_rows_f32(float* d_x, int64_t x_row_stride, const void* d_branch, int64_t branch_row_stride, const float* d_gamma,
                               const float* d_beta, float eps, void* d_y, int32_t y_dtype, int64_t rows, int64_t c, int32_t dtype,
                               void* stream);

/* tia_vit_assemble_prefix_h with a float32 result: d_out [n, 1+R+g, d] float32 with out[b,0] = cls (+ pos[0] if pos_has_cls),
 * out[b,1+r] = reg[r], out[b,1+R+i] = float(tokens[b,i]) + pos[i + pos_has_cls] -- the same single float32 add, NOT rounded.
 * Arguments and refusals as there (R = 0 with pos_has_cls = 1 is the plain form); d % 8 == 0 and d <= 8192 (else TIA_ESIZE). */
int tia_vit_assemble_rows_f32(const void* d_tokens, const float* d_cls, const float* d_reg, const float* d_pos, int32_t pos_has_cls,
                              float* d_out, int64_t n, int64_t g, int64_t reg_tokens, int64_t d, int32_t dtype, void* stream);

/* tia_vit_cls_mean_pool_h of the float32 stream: out[b, :d] = LN(x'[b,0]), out[b, d:] = mean_{i = skip .. s-1} LN(x'[b,i]) with
 * x' = x + float(branch) (one float32 add on load, nothing written back) or x' = x when d_branch is NULL.
 *   d_x [n,s,d] float32   d_branch [n,s,d] of `dtype` or NULL   d_gamma, d_beta [d] float32   d_out [n, 2d] float32
 * The same wave-to-row assignment, fixed summation order and single affine as the half form: an image's result is bit-identical
 * whatever n is.  skip < 1 or skip >= s is TIA_EINVAL; d % 8 == 0 and d <= 8192 (else TIA_ESIZE). */
int tia_vit_cls_mean_pool_f32(const float* d_x, const void* d_branch, const float* d_gamma, const float* d_beta, float eps, float* d_out,
                              int64_t n, int64_t s, int64_t skip, int64_t d, int32_t dtype, void* stream);

/* Vision Transformer classifiers (the reference's TimmModel: backbone -> Linear -> softmax) from uint8 patches to probabilities:
 * the input normalisation inside the im2col, and the head on the graph's float32 features.  Additive, same version (6). */

/* tia_vit_patchify_pad_h on uint8 patches with ToTensor + Normalize(mean, std) applied as a table: token value = d_table[byte][c].
 *   d_x [n,h,w,3] uint8 NHWC, dense; it may start at ANY byte (a view into a larger buffer)
 *   d_table [256][3] of `dtype`, 16-byte aligned: entry [v][c] is ((v / 255) - mean[c]) / std[c], worked out by the caller in
 *     float32 and rounded once to `dtype` (models/dataset/classification.py: TimmNormPreproc)
 *   d_tokens [n, (h/patch) * (w/patch), k_pad] of `dtype`, 16-byte aligned; columns in (ky, kx, channel) order, columns
 *     3 patch^2 .. k_pad - 1 exact zeros.  k_pad == 3 patch^2 is allowed when that is a multiple of 32 (patch 16: 768), so the one
 *     entry point serves every patch size.
 * A pure gather (no arithmetic): the result equals tia_vit_patchify_h / tia_vit_patchify_pad_h applied to the table looked up
 * per byte, bit for bit.  The table is kept in LDS; the bytes are read as aligned dwords and shifted together wherever 8 of them are
 * contiguous.  TIA_ESIZE: h % patch, w % patch, k_pad % 32, k_pad < 3 patch^2.  TIA_EINVAL: a null pointer, a non-positive size, a
 * dtype other than TIA_DT_F16 | TIA_DT_BF16, d_table or d_tokens not 16-byte aligned.  Nothing is launched on an error. */
int tia_vit_patchify_norm_u8_h(const uint8_t* d_x, const void* d_table, void* d_tokens, int64_t n, int64_t h, int64_t w, int64_t patch,
                               int64_t k_pad, int32_t dtype, void* stream);

/* The classifier head: p[r,:] = softmax(x[r,:f] . W^T + b), float32 throughout.
 *   d_x float32, row r at element r * row_stride (row_stride >= f, % 4 == 0), 16-byte aligned   d_w [c,f] float32 (nn.Linear's own
 *   layout), 16-byte aligned   d_bias [c] float32 or NULL   d_p [rows,c] dense float32.
 * One wave per row; every logit is summed with fmaf in an order fixed by f alone (no atomics: a row's probabilities are bit-identical
 * in any batch); the row maximum is subtracted, exp is expf (not the fast intrinsic), ONE division per element; c == 1 gives 1.0.
 * 1 <= c <= 64, f % 4 == 0 and f <= 8192 (else TIA_ESIZE); null d_x / d_w / d_p, non-positive sizes, row_stride < f or % 4 != 0 and
 * misaligned pointers are TIA_EINVAL.  Nothing is launched on an error. */
int tia_linear_softmax_rows_f32(const float* d_x, int64_t row_stride, const float* d_w, const float* d_bias, float* d_p, int64_t rows,
                                int64_t f, int64_t c, void* stream);

/* =======================================================================================
 * Vision Transformer linear layers on the FP8 matrix instruction (vit_fused.py, linear_dtype="float8_e4m3").
 * Additive, same version (6); the contract of the family above (16-byte aligned pointers, nothing launched on an error).
 *
 * The numeric contract -- row x column scaled FP8, not MXFP8:
 *   format       OCP e4m3fn: largest finite value 448, no infinities (NOT the MI300 fnuz encoding).  float32 -> code rounds to
 *                nearest even and saturates at +-448.
 *   a row        v[0..K) float32: amax = max |v|; inv = 448 / amax and s = amax / 448, one float32 division each (amax == 0:
 *                inv = s = 1); q[k] = e4m3(v[k] * inv), the product in float32.  Stored as q (K bytes) and s (one float32).
 *   weights      one row per output channel, quantised once from the float32 weights (after the LayerScale fold and the SwiGLU
 *                padding: where the half path rounds).
 *   activations  one row per token, quantised from the float32 value the producing kernel holds, before any rounding to half.
 *   GEMM         acc[r,o] = sum_k qa[r,k] qw[o,k]: exact products, float32 accumulation in any order;
 *                y[r,o] = half_rne(acc * sa[r] * sw[o] + bias[o] (+ float32(residual[r,o]))).
 *                v_mfma_scale_f32_16x16x128_f8f6f4 with both block-scale operands the constant 1.0 (E8M0 127).
 * ===================================================================================== */

/* The GEMM.  d_a [rows,K] e4m3 codes with d_sa [rows]; d_w [N,K] e4m3 codes with d_sw [N] (tia_linear_fp8_pack_weights);
 * d_bias [N] float32 or NULL; d_residual [rows,N] of `dtype` or NULL; d_y [rows,N] of `dtype` (TIA_DT_F16 | TIA_DT_BF16).
 * K % 128 == 0 and N % 16 == 0 (else TIA_ESIZE), any rows >= 1 (rows <= 0: TIA_EINVAL). */
int tia_linear_fp8_rows(const void* d_a, const float* d_sa, const void* d_w, const float* d_sw, const float* d_bias,
                        const void* d_residual, void* d_y, int64_t rows, int64_t n, int64_t k, int32_t dtype, void* stream);

/* Weights for tia_linear_fp8_rows from float32 d_w [N,K] (nn.Linear's own layout): d_q [N,K] codes, d_scale [N], quantised per
 * output channel on the device by the recipe above.  The shape limits of the GEMM. */
int tia_linear_fp8_pack_weights(const float* d_w, int64_t n, int64_t k, void* d_q, float* d_scale, void* stream);

/* Host-only: 1 when tia_linear_fp8_rows takes (and the graph routes) a layer of this shape, 0 when the layer stays on the half
 * GEMM (a size outside the kernel's), TIA_EINVAL for a non-positive size.  No device call. */
int tia_linear_fp8_serves(int64_t rows, int64_t n, int64_t k);

/* The quantising producers: the arithmetic of tia_layernorm_rows_h / tia_gelu_rows_h / tia_swiglu_rows_h up to the float32
 * value, which is then quantised per row by the recipe above instead of being rounded to half -- no extra pass over the
 * activations.  d_q [rows, c | hidden] codes, d_scale [rows] float32.  c, hidden % 16 == 0 and <= 8192 (else TIA_ESIZE).
 * tia_swiglu_rows_q8 reads d_x [rows, 2 hidden], the first half the gate; a zero gate and value (a pad lane) gives code 0. */
int tia_layernorm_rows_q8(const void* d_x, int64_t row_stride, const float* d_gamma, const float* d_beta, float eps, void* d_q,
                          float* d_scale, int64_t rows, int64_t c, int32_t dtype, void* stream);
int tia_gelu_rows_q8(const void* d_x, void* d_q, float* d_scale, int64_t rows, int64_t hidden, int32_t dtype, void* stream);
int tia_swiglu_rows_q8(const void* d_x, void* d_q, float* d_scale, int64_t rows, int64_t hidden, int32_t dtype, void* stream);

/* =======================================================================================
 * Vision Transformer linear layers on the INT8 matrix instruction (vit_fused.py, linear_dtype="int8").
 * Additive, same version (6); the contract of the family above (16-byte aligned pointers, nothing launched on an error).
 *
 * The numeric contract -- W8A8, symmetric, one scale per token and one per output channel:
 *   a row        v[0..K) float32: amax = max |v|; inv = 127 / amax and s = amax / 127, one float32 division each (amax == 0:
 *                inv = s = 1); q[k] = clamp(rne(v[k] * inv), -127, 127), the product in float32, rounding to nearest even.  The
 *                code -128 is never produced.  Stored as q (K bytes of int8) and s (one float32).
 *   non-finite   the row maximum propagates NaN.  A row holding NaN has s = NaN, a row holding +-inf (and no NaN) has s = +inf;
 *                a NaN product v[k] * inv gives the code 0, so every code stays inside [-127, 127].  Every output of that token
 *                is then non-finite, never a finite wrong value; other tokens are untouched.
 *   weights      one row per output channel, quantised once from the float32 weights (after the LayerScale fold and the SwiGLU
 *                padding: where the FP8 route quantises).
 *   activations  one row per token, quantised from the float32 value the producing kernel holds, before any rounding to half.
 *   GEMM         acc[r,o] = sum_k qa[r,k] qw[o,k] exactly, in int32: the result does not depend on summation order, tiling or run.
 *                K <= 65536 keeps K 127^2 inside int32; a larger K is TIA_ESIZE.
 *                y[r,o] = half_rne(float(acc) * sa[r] * sw[o] + bias[o] (+ float32(residual[r,o]))); float(acc) is the
 *                round-to-nearest-even conversion (exact below 2^24), the float32 epilogue is tia_linear_fp8_rows's.
 *                v_mfma_i32_16x16x64_i8, two instructions per 128-deep K-step.
 * ===================================================================================== */

/* The GEMM.  d_a [rows,K] int8 codes with d_sa [rows]; d_w [N,K] int8 codes with d_sw [N] (tia_linear_int8_pack_weights);
 * d_bias [N] float32 or NULL; d_residual [rows,N] of `dtype` or NULL; d_y [rows,N] of `dtype` (TIA_DT_F16 | TIA_DT_BF16).
 * K % 128 == 0, K <= 65536 and N % 16 == 0 (else TIA_ESIZE), any rows >= 1 (rows <= 0: TIA_EINVAL). */
int tia_linear_int8_rows(const void* d_a, const float* d_sa, const void* d_w, const float* d_sw, const float* d_bias,
                         const void* d_residual, void* d_y, int64_t rows, int64_t n, int64_t k, int32_t dtype, void* stream);

/* Weights for tia_linear_int8_rows from float32 d_w [N,K] (nn.Linear's own layout): d_q [N,K] codes, d_scale [N], quantised per
 * output channel on the device by the recipe above.  The shape limits of the GEMM. */
int tia_linear_int8_pack_weights(const float* d_w, int64_t n, int64_t k, void* d_q, float* d_scale, void* stream);

/* Host-only: 1 when tia_linear_int8_rows takes (and the graph routes) a layer of this shape, 0 when the layer stays on the half
 * GEMM (a size outside the kernel's), TIA_EINVAL for a non-positive size.  No device call. */
int tia_linear_int8_serves(int64_t rows, int64_t n, int64_t k);

/* The quantising producers: the arithmetic of tia_layernorm_rows_h / tia_gelu_rows_h / tia_swiglu_rows_h up to the float32
 * value, which is then quantised per row by the INT8 recipe above.  d_q [rows, c | hidden] int8 codes, d_scale [rows] float32.
 * c, hidden % 16 == 0 and <= 8192 (else TIA_ESIZE).  tia_swiglu_rows_qi8 reads d_x [rows, 2 hidden], the first half the gate;
 * a zero gate and value (a pad lane) gives code 0. */
int tia_layernorm_rows_qi8(const void* d_x, int64_t row_stride, const float* d_gamma, const float* d_beta, float eps, void* d_q,
                           float* d_scale, int64_t rows, int64_t c, int32_t dtype, void* stream);
int tia_gelu_rows_qi8(const void* d_x, void* d_q, float* d_scale, int64_t rows, int64_t hidden, int32_t dtype, void* stream);
int tia_swiglu_rows_qi8(const void* d_x, void* d_q, float* d_scale, int64_t rows, int64_t hidden, int32_t dtype, void* stream);

/* ---------------------------------------------------------------------------------------
 * Per-input-channel smoothing of the INT8 layers (vit_fused.py, prepare(..., linear_dtype="int8", smoothing=scales), the engines'
 * int8_smoothing).  Additive, same version (6); opt-in: nothing above changes.
 *
 * The recipe -- for a layer y = x W^T + b that the graph routes to tia_linear_int8_rows (attn.qkv, mlp.fc1, mlp.fc2) and input
 * channel j:
 *   a[j]   the calibrated abs-max, over every token of the calibration set, of the float32 value the producing kernel holds for
 *          channel j (the LayerNorm output for qkv and fc1, the GELU / SwiGLU output for fc2): the statistics entries below
 *   w[j]   max_o |W[o,j]| of the float32 weights that are packed (after the LayerScale fold and the SwiGLU padding)
 *   s[j]   2^clamp(round(alpha log2 a[j] - (1 - alpha) log2 w[j]), -24, 24), evaluated in float64 on the host, alpha in (0, 1];
 *          s[j] = 1 where a[j] == 0 or w[j] == 0 (the SwiGLU pad lanes among them).  A non-finite a[j] is refused.
 * A power of two makes x / s and W s exact in float32: smoothing adds no rounding of its own, x W^T is unchanged as a real-valued
 * function, and all-ones scales reproduce the unsmoothed graph bit for bit.
 *   weights   W'[o,j] = W[o,j] s[j] in float32, then tia_linear_int8_pack_weights
 *   qkv, fc1  the float32 LayerNorm affine is folded on the host, gamma' = gamma / s and beta' = beta / s, and
 *             tia_layernorm_rows_qi8 runs with the folded pair
 *   fc2       tia_gelu_rows_qi8_smooth / tia_swiglu_rows_qi8_smooth multiply the float32 value by inv_smooth[j] = 1 / s[j] (one
 *             float32 multiplication per element) before the row maximum and the codes
 * ------------------------------------------------------------------------------------- */

/* tia_gelu_rows_qi8 / tia_swiglu_rows_qi8 with d_inv_smooth [hidden] float32 (16-byte aligned, non-NULL) applied to the float32
 * value before it is quantised; the sizes, the errors and the NaN / inf contract of those entries.  A pad lane stays code 0. */
int tia_gelu_rows_qi8_smooth(const void* d_x, const float* d_inv_smooth, void* d_q, float* d_scale, int64_t rows, int64_t hidden,
                             int32_t dtype, void* stream);
int tia_swiglu_rows_qi8_smooth(const void* d_x, const float* d_inv_smooth, void* d_q, float* d_scale, int64_t rows, int64_t hidden,
                               int32_t dtype, void* stream);

/* The calibration statistics: the arithmetic of the _qi8 producers up to the float32 value v, then
 * d_amax[j] = max(d_amax[j], max_r |v[r,j]|) for every column j.  d_amax [c | hidden] float32: the caller zeroes it, and the result
 * accumulates over calls.  Magnitudes are compared as the bit patterns of non-negative floats: a NaN sorts above +inf and stays in
 * its column (and only there).  The sizes and errors of the _qi8 entries; nothing is launched on an error.  Run once per model. */
int tia_layernorm_rows_absmax_h(const void* d_x, int64_t row_stride, const float* d_gamma, const float* d_beta, float eps,
                                float* d_amax, int64_t rows, int64_t c, int32_t dtype, void* stream);
int tia_gelu_rows_absmax_h(const void* d_x, float* d_amax, int64_t rows, int64_t hidden, int32_t dtype, void* stream);
int tia_swiglu_rows_absmax_h(const void* d_x, float* d_amax, int64_t rows, int64_t hidden, int32_t dtype, void* stream);

/* =======================================================================================
 * The float32 route of the Vision Transformer graph (vit_fused.py, prepare(torch.float32, linear_dtype="bfloat16x3"), the engines'
 * compute_dtype="bfloat16x3").  Additive, same version (6).
 *
 * Activations, the residual stream and all row arithmetic are float32.  Every Linear is tia_conv2d_bf16x3_nhwc_f32 on the
 * [n,S,1,cin] map (both operands split into three bf16 numbers, six exact products per float32 product, float32 accumulation; bias
 * and the float32 residual in its epilogue) or, for a layer off that kernel's shapes or without an exact normal split of its weights,
 * tia_conv2d_nhwc_f32.  The LayerNorm is tia_add_layernorm_rows_f32 with a NULL branch and TIA_DT_F32 output, the pooled norm
 * tia_vit_cls_mean_pool_f32 with a NULL branch, the classifier head tia_linear_softmax_rows_f32.  The five entry points below are
 * the rest.  The family's contract: null / misaligned (16 bytes) / non-positive arguments TIA_EINVAL, unsupported sizes TIA_ESIZE,
 * nothing launched on an error; 64-bit offsets, 16-byte accesses, no atomics; the entry launches and neither allocates nor syncs.
 *
 * Numeric contract: every value is float32 and nothing is rounded to a half type.  A matrix product's error is a float32 matmul's
 * (the split kernel drops terms below 2^-23 |a w|); attention is exact float32 products in float32 fma chains.
 * Invalid-input domain: the split kernel's -- a non-finite activation, or one with |a| >= 2^127 (2 - 2^-8) = 3.3961e38, makes every
 * output that reads it non-finite, never a finite wrong value.
 * ===================================================================================== */

/* Attention, float32: d_qkv [n,s,3,heads,head_dim] (the qkv Linear's own output order) -> d_out [n,s,heads*head_dim],
 *   out[b,i,h,:] = softmax_j(scale * q[b,i,h,:] . k[b,j,h,:]) @ v[b,:,h,:]
 * on v_mfma_f32_16x16x4_f32: exact float32 products, float32 fma chains (a score is eight chains over the dims 16 j + 4 q + e, one
 * per (j & 1, e), q then j in order, added pairwise; an output sums its keys tile by tile in one chain, key 16 kt + 4 q + r with
 * (kt, r) the step and q the order inside a step).  Online softmax
 * with p = exp2((score - max) * scale * log2 e): the probabilities are never rounded below float32 and only O / l is written.
 * Keys beyond s take no part (their scores are -inf before the maximum; there is never inf - inf).
 * head_dim 64 or 80 (else TIA_ESIZE), any s >= 1; `dtype` must be TIA_DT_F32 (a half code is TIA_EINVAL: tia_mha_fwd_h is that
 * entry); scale finite and > 0. */
int tia_mha_fwd_f32(const float* d_qkv, float* d_out, int64_t n, int64_t s, int64_t heads, int64_t head_dim, float scale, int32_t dtype,
                    void* stream);

/* Exact (erf) GELU in place on `count` float32 values (count % 4 == 0, else TIA_ESIZE): 0.5 x (1 + erf(x / sqrt 2)) for x >= 0 and
 * the same value as 0.5 x erfc(-x / sqrt 2) for x < 0 (no cancellation in the tail); -0.0 stays -0.0. */
int tia_gelu_rows_f32(float* d_x, int64_t count, void* stream);

/* Packed SwiGLU: d_x [rows, 2 hidden] float32, the first half the gate -> d_y [rows, hidden] = silu(gate) * value, silu through
 * e = exp(-|t|) as tia_swiglu_rows_h (no overflow for any gate; a zero gate and value gives 0).  hidden % 4 == 0 (else TIA_ESIZE). */
int tia_swiglu_rows_f32(const float* d_x, float* d_y, int64_t rows, int64_t hidden, void* stream);

/* The patch embedding's im2col in float32: d_x [n,h,w,3] float32 NHWC -> d_tokens [n, (h/patch)*(w/patch), k_pad] float32, columns in
 * (ky, kx, channel) order, columns 3 patch^2 .. k_pad - 1 exact zeros.  Any patch size; a pure gather (bit for bit).  d_x is read with
 * 4-byte loads and needs only 4-byte alignment (a batch may be a slice that starts at any float of a larger buffer); d_tokens 16 bytes.
 * TIA_ESIZE: h % patch, w % patch, k_pad % 16 (the GEMMs' smallest multiple), k_pad < 3 patch^2 (k_pad == 3 patch^2 is allowed). */
int tia_vit_patchify_f32(const float* d_x, float* d_tokens, int64_t n, int64_t h, int64_t w, int64_t patch, int64_t k_pad, void* stream);

/* tia_vit_assemble_rows_f32 for float32 tokens: d_out [n, 1+R+g, d] with out[b,0] = cls (+ pos[0] if pos_has_cls), out[b,1+r] = reg[r],
 * out[b,1+R+i] = tokens[b,i] + pos[i + pos_has_cls] -- ONE float32 add per element.  d_reg NULL exactly when reg_tokens == 0;
 * pos_has_cls = 0 with host-folded cls / reg rows is the prefix_pos_embed form.  d % 4 == 0 and d <= 8192 (else TIA_ESIZE). */
int tia_vit_assemble_f32(const float* d_tokens, const float* d_cls, const float* d_reg, const float* d_pos, int32_t pos_has_cls,
                         float* d_out, int64_t n, int64_t g, int64_t reg_tokens, int64_t d, void* stream);

/* =======================================================================================
 * Attention maps of the Vision Transformers (vit_attention_maps.hip; the engines' run kwarg return_attention).  Additive, same
 * version (6).  Neither entry is launched by a run that asks for no maps; both are deterministic (no atomics).
 * ===================================================================================== */

/* The attention probabilities that tia_mha_fwd_h does not materialise, for the first q_rows queries:
 *   p[b,h,i,j] = softmax_j(scale * q[b,i,h,:] . k[b,j,h,:]),  i < q_rows,  j < s
 *   d_qkv [n, s, 3, heads, head_dim] of `dtype` (TIA_DT_F16 | TIA_DT_BF16; anything else TIA_EINVAL) -- tia_mha_fwd_h's input
 *   d_out float32: head_mean = 0: [n, heads, q_rows, s];  head_mean = 1: [n, q_rows, s], (1 / heads) sum_h p, the heads added in
 *   ascending order in float32 by the workgroup that owns the query tile and divided by heads once.
 * Scores on v_mfma_f32_16x16x32_f16 / _bf16 with float32 accumulation; softmax in float32 in the base-2 domain over all s keys:
 * t = score * (scale * log2 e), m = max_j t, e_j = exp2(t_j - m), l = sum_j e_j (an online sum over 64-key tiles, rescaled when m
 * moves); every stored probability is e_j / l with ONE correctly rounded division.  Keys >= s contribute exactly 0.  Two passes
 * over the keys (m and l, then the probabilities), so s has no ceiling: any s >= 1, 64-bit offsets.
 * head_dim 64 or 80 (else TIA_ESIZE); head_mean = 1 takes at most 64 heads (TIA_ESIZE beyond: their (m, l) wait in LDS);
 * 1 <= q_rows <= s, head_mean 0 | 1, scale finite and > 0, 16-byte aligned non-null pointers (else TIA_EINVAL). */
int tia_mha_probs_h(const void* d_qkv, float* d_out, int64_t n, int64_t s, int64_t heads, int64_t head_dim, float scale, int64_t q_rows,
                    int32_t head_mean, int32_t dtype, void* stream);

/* One step of attention rollout (Abnar & Zuidema 2020) on n float32 [s, s] matrices:  R_out = 1/2 (A R_in) + 1/2 R_in.
 * A R_in on v_mfma_f32_16x16x4_f32: every element is ONE float32 fma chain over k = 0 .. s - 1 in ascending order (exact products,
 * one rounding per step); both halvings are exact and the final add rounds once.  d_r_in NULL means R_in = I.  Any s >= 1 (tails
 * are zero-filled operands: exact).  Pointers 4-byte aligned; d_r_out overlapping d_a or d_r_in is TIA_EINVAL. */
int tia_rollout_step_f32(const float* d_a, const float* d_r_in, float* d_r_out, int64_t n, int64_t s, void* stream);

/* ---- rollout with another head fusion or a discard ratio (the engines' attention_head_fusion / attention_discard_ratio; additive,
 * same version 6; models/engine/_rollout_options.py states the arithmetic).  A run with the default options launches none of these. */
#define TIA_FUSE_MEAN 0
#define TIA_FUSE_MAX 1
#define TIA_FUSE_MIN 2

/* The probabilities of ALL s query rows fused over the heads: d_out float32 [n, s, s].
 *   TIA_FUSE_MEAN: tia_mha_probs_h(q_rows = s, head_mean = 1), the same kernel: bit for bit.
 *   TIA_FUSE_MAX / _MIN: the exact element-wise maximum / minimum over the heads of the values tia_mha_probs_h(head_mean = 0) writes
 *   (the same two passes, e_j / l with one division per head and element).
 * The limits and codes of tia_mha_probs_h with head_mean = 1 (head_dim 64 or 80, at most 64 heads: TIA_ESIZE); fusion outside the
 * three values is TIA_EINVAL. */
int tia_mha_probs_fused_h(const void* d_qkv, float* d_out, int64_t n, int64_t s, int64_t heads, int64_t head_dim, float scale,
                          int32_t fusion, int32_t dtype, void* stream);

/* Discard and normalise n float32 [s, s] matrices F of finite values >= 0 (one or two launches):
 *   k >= 1: v[b] = the k-th smallest (1-based, duplicates counted) of the s * s entries of F[b] -- an exact order statistic, found by
 *   a radix select on the bit patterns (digits of 12, 10, 10 bits, histograms in LDS; integer atomics only, so the result does not
 *   depend on scheduling) and written to d_v [n]; F'[i][j] = 0 where F[i][j] <= v and (i, j) != (0, 0), F elsewhere.  k = 0: F' = F,
 *   nothing is selected and d_v may be NULL.
 *   A^ = (F' + I) / 2 (the halving exact);  s_i = sum_j A^[i][j] in this order of float32 additions: 64 partial sums p[l] = entries
 *   j = l, l + 64, ... added in ascending order to 0, folded by p[l] += p[l ^ 32], then ^ 16, 8, 4, 2, 1;  d_out[i][j] = A^[i][j] / s_i,
 *   one correctly rounded division each.
 * Any n >= 1 and 1 <= s <= 65535 (TIA_ESIZE beyond: the counts are 32-bit), 64-bit offsets.  Values outside the domain (negative,
 * NaN) give unspecified values, never an access outside the buffers.  TIA_EINVAL, with nothing launched: a null d_f / d_out, d_v null
 * with k >= 1, k < 0 or k >= s * s, pointers not 4-byte aligned, d_out overlapping d_f, d_v overlapping either. */
int tia_rollout_discard_normalize_f32(const float* d_f, float* d_out, float* d_v, int64_t n, int64_t s, int64_t k, void* stream);

/* R_out = A R_in on n float32 [s, s] matrices: tia_rollout_step_f32's product (v_mfma_f32_16x16x4_f32, one float32 fma chain over
 * k = 0 .. s - 1 in ascending order per element, zero-filled tails) without its blend.  d_r_in NULL means R_out = A.  The same
 * limits, alignment and overlap rules. */
int tia_rollout_product_f32(const float* d_a, const float* d_r_in, float* d_r_out, int64_t n, int64_t s, void* stream);

/* =======================================================================================
 * Class activation maps of the CNN classifiers (cnn_cam.hip; the engines' run kwargs return_cam / merge_cam;
 * models/engine/_cam.py states the quantity).  Additive, same version (6).  A run that asks for no maps launches neither.
 * ===================================================================================== */

/* The classifier applied at every position of the trunk's last feature map (Zhou et al. 2016):
 *   d_out[b, j, p] = sum_c d_w[j, c] * d_x[b, p, c]          no bias, no ReLU, nothing renormalised
 *   d_x [n, hw, c] channels-last: float32 (tia_cam_nhwc_f32) or `dtype` = TIA_DT_F16 | TIA_DT_BF16 (tia_cam_nhwc_h; anything
 *   else TIA_EINVAL), widened exactly;   d_w [k, c] float32;   d_out [n, k, hw] float32.
 * float32 multiply-adds (fmaf): lane l of a wave takes the 16-byte vectors l, l + 64, ... of a row in ascending c, the 64 partial
 * sums are added as v[l] + v[l ^ 32], then ^ 16, 8, 4, 2, 1.  That order depends on c alone -- not on n, the row's place in the batch
 * or the grid -- so a patch gives the same bits in any batch.  d_x is read once per tile of classes (12 classes, fewer where
 * k * c * 4 bytes exceed 144 KB of LDS).  No atomics, no allocation, no synchronisation; 64-bit offsets.
 * TIA_EINVAL: a null pointer, n / hw / c / k <= 0, d_x or d_w not 16-byte aligned, d_out not 4-byte aligned.
 * TIA_ESIZE: c % 64 != 0 or c > 8192; n >= 2^31 or hw * k >= 2^31.  Nothing is launched on an error. */
int tia_cam_nhwc_f32(const float* d_x, const float* d_w, float* d_out, int64_t n, int32_t hw, int32_t c, int32_t k, void* stream);
int tia_cam_nhwc_h(const void* d_x, const float* d_w, float* d_out, int64_t n, int32_t hw, int32_t c, int32_t k, int32_t dtype,
                   void* stream);

/* =======================================================================================
 * All borders of binary planes: cv2.findContours(layer, RETR_TREE, CHAIN_APPROX_NONE | _SIMPLE)
 * (models/architecture/hovernetplus.py:222-226, HoVerNetPlus._get_layer_info)
 * ===================================================================================== */

/* Raster-first pixel (flat index, 0x7f7f7f7f if absent) and frame contact of every label 1..kmax of every plane:
 * with tia_ccl_label_i32 (8-connected foreground, 4-connected background) this yields the start pixel of every outer
 * border (a component's first pixel) and of every hole border (left of an enclosed background component's first pixel).
 *   d_labels [n,h,w] i32   d_first, d_edge [n, kmax+1] i32 */
int tia_label_first_pixel_i32(const int32_t* d_labels, int64_t n, int64_t h, int64_t w, int32_t kmax,
                              int32_t* d_first, int32_t* d_edge, void* stream);

/* Border following (Suzuki & Abe 1985, step 3 = OpenCV icvFetchContour), one lane per border.
 *   d_starts [nb,4] i32 = plane, x0, y0, is_hole.  d_points == NULL: count pass, d_counts[nb] = points per border.
 *   Otherwise border e writes its (x, y) pairs at d_points + 2*d_offsets[e] (capacity = total pairs allocated).
 *   simple != 0: CHAIN_APPROX_SIMPLE (direction changes only); 0: CHAIN_APPROX_NONE (every border pixel). */
int tia_border_trace_u8(const uint8_t* d_mask, int64_t n, int64_t h, int64_t w, const int32_t* d_starts, int64_t nb,
                        int32_t simple, int32_t* d_counts, const int64_t* d_offsets, int64_t capacity,
                        int32_t* d_points, void* stream);

/* =======================================================================================
 * Peak detection on probability maps: skimage.feature.peak_local_max with a square footprint, p_norm = inf, no labels
 * (what the reference's detection models call in postproc; additive at version 6).  tiatoolbox_amd/utils/_peaks.py
 * states the result and is the contract.
 * ===================================================================================== */

/* Candidates of n float32 planes [n,h,w], in two calls around one read of d_totals (the count pass and the write pass of
 * tia_hover_contour_scan / _write: raster order without order-dependent atomics).
 *   scan : threshold t = threshold_abs if has_threshold_abs else the plane's minimum; with has_threshold_rel
 *          t = max(t, threshold_rel * the plane's maximum) (float32).  A pixel is a candidate when it equals the maximum of its
 *          (2 min_distance + 1)^2 window (edge-replicated), the plane is not constant (a 1-pixel plane: no such condition),
 *          it is > t (strict) and it lies outside the first and last `border` rows and columns.
 *          d_state [n,h,w] u8 = 0 no candidate, 1 candidate, 2 contested candidate: another candidate lies at Chebyshev distance
 *          < min_distance (only these take part in the spacing walk, see tia_peak_resolve_host).
 *          d_minmax [n,2] u32, d_flags [n,h,w] u8: scratch.  d_offsets [n, tia_peak_chunks(h, w)] i32: for the write pass.
 *          d_totals [n] i64 = candidates per plane.
 *   write: d_bases [n] i64 = row of each plane's first candidate in the outputs (the exclusive prefix sum of d_totals);
 *          candidate j of plane p in raster order goes to row d_bases[p] + j of d_yx [capacity,2] i32 (row, column),
 *          d_value [capacity] f32 and d_contested [capacity] u8; rows at or beyond `capacity` are not written.
 * 1 <= min_distance <= 64 and h * w < 2^31, else TIA_ESIZE (also: n * tiles of 32 x 32 pixels >= 2^31).  TIA_EINVAL: a null
 * pointer, n / h / w <= 0, border < 0, capacity < 0.  Nothing is launched on an error.  Offsets into the batch are 64-bit.
 * NaN is outside the domain: with a NaN in a plane its result is unspecified, but every access stays in bounds (no index
 * depends on a pixel's value).  +-inf and +-0 are inside it (-0 == +0). */
size_t tia_peak_chunks(int64_t h, int64_t w);
int tia_peak_scan_f32(const float* d_image, int64_t n, int64_t h, int64_t w, int32_t min_distance,
                      int32_t has_threshold_abs, float threshold_abs, int32_t has_threshold_rel, float threshold_rel,
                      int32_t border, uint32_t* d_minmax, uint8_t* d_flags, uint8_t* d_state, int32_t* d_offsets,
                      int64_t* d_totals, void* stream);
int tia_peak_write_f32(const float* d_image, const uint8_t* d_state, int64_t n, int64_t h, int64_t w,
                       const int32_t* d_offsets, const int64_t* d_bases, int64_t capacity, int32_t* d_yx,
                       float* d_value, uint8_t* d_contested, void* stream);

/* The spacing walk of peak_local_max over the contested candidates of ONE plane, on the HOST (no device call; all pointers
 * are host memory): yx [k,2] i32 (row, column) in strictly ascending raster order, plane width w; accept[i] = 1 when no
 * candidate accepted before it lies at Chebyshev distance < min_distance, else 0.  Two candidates that close have equal
 * values, so raster order is the statement's order among them.  TIA_EINVAL: k < 0, w <= 0, min_distance < 1, a null
 * pointer with k > 0, a column outside [0, w), a negative row, or rows not in raster order. */
int tia_peak_resolve_host(const int32_t* yx, int64_t k, int64_t w, int32_t min_distance, uint8_t* accept);

#ifdef __cplusplus
}
#endif
#endif /* TIATOOLBOX_AMD_H */
