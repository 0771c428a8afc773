/*
 * esahrnet.h — C-ABI of libesahrnet.so: the MI355X (gfx950) HRNet keypoint-heatmap path.
 *
 * The reference (bonjour-l/esa-pose-estimation) has no FFI seam for this path: its seam is
 * the torch.nn.Module protocol.  This header is therefore what a binding for
 * the path would bind, entry point by entry point:
 *
 *   esahrnet_create / _conv_count / _conv_desc   <- models/seg_hrnet.py:260-340, 343-423
 *                                                   (HighResolutionNet.__init__ and the _make_*
 *                                                   builders: cfg -> list of Conv2d/BatchNorm2d)
 *   esahrnet_set_conv / _commit                  <- models/seg_hrnet.py:475-493 init_weights /
 *                                                   val.py:64-66 load_model -> load_state_dict
 *   esahrnet_forward                             <- models/seg_hrnet.py:425-473
 *                                                   HighResolutionNet.forward (val.py:146 call)
 *   esahrnet_keypoints                           <- demo.py:172-185 / val.py:151-164 two-stage
 *                                                   torch.max + inference.py:136-152 get_final
 *                                                   (inference.py:75-94 my_taylor)
 *
 * Conventions: plain C types only; every function returns 0 on success, non-zero on error
 * with a message in esahrnet_last_error() (thread-local); nothing throws across the ABI.
 * All device buffers are CALLER-OWNED (in the Python host: torch tensors, so the caching
 * allocator and stream semantics stay intact).  The handle owns only the packed weights.
 * Kernels are enqueued on the stream passed in and never synchronise it.  One handle per
 * device; calls on one handle are not re-entrant.
 */
#ifndef ESAHRNET_H
#define ESAHRNET_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ESAHRNET_MAX_BRANCHES 4
#define ESAHRNET_ABI_VERSION 6      /* 5: esahrnet_cfg.precision 2 (fp32-grade bf16x6); 6: precision 1 for variant 1,
                                       esahrnet_op_cbam */

typedef struct esahrnet_ctx* esahrnet_handle;
typedef void* esahrnet_stream; /* hipStream_t */

/* Stage table of config/default.py:39-74 as plain ints. */
typedef struct esahrnet_cfg {
    int32_t cin;                 /* 1 (seg_hrnet2.py:265) or 3 (seg_hrnet.py:265)            */
    int32_t num_keypoints;       /* 11 (seg_hrnet2.py:324) or 32 (seg_hrnet.py:324)           */
    int32_t stem_width;          /* 64 (seg_hrnet.py:265-270)                                  */
    int32_t widths[ESAHRNET_MAX_BRANCHES];          /* NUM_CHANNELS of STAGE4: 32,64,128,256   */
    int32_t blocks[4][ESAHRNET_MAX_BRANCHES];       /* NUM_BLOCKS per stage (stage1 uses [0][0]) */
    int32_t modules[4];          /* NUM_MODULES per stage (stage1 entry unused)                */
    int32_t final_conv_kernel;   /* FINAL_CONV_KERNEL, must be 1 (config/default.py:43)        */
    int32_t variant;             /* 0: seg_hrnet.py / seg_hrnet2.py;  1: seg_hrnet3.py (CBAM in every
                                    BasicBlock and on the 64-ch pre-BN stem skip, 3x3 last_layer[0],
                                    output_layer over [heatmaps, skip]; models/seg_hrnet3.py)         */
    int32_t precision;           /* arithmetic of the convolutions (not a reference knob: BASELINE.json configs):
                                    2: "bf16x6" — fp32-grade, THE MODE OF configs[1] / configs[2] (the reference computes in
                                       fp32, models/seg_hrnet.py:425-473): f32 NHWC activations, every operand split exactly
                                       into three bf16 terms, 6 MFMAs per product, f32 accumulate; error vs fp64 at or below
                                       that of an f32 FMA chain; both variants;
                                    0: "bf16x3" — split-bf16 hi/lo operands (~16 significand bits), 3 MFMAs per product, f32
                                       accumulate: heatmap L_inf ~1e-5 of the heat-map scale; opt-in fast mode, NOT fp32;
                                    1: bf16 activations and weights stored ONCE (half the bytes, one MFMA per
                                       product), f32 accumulate, f32 folded-BN bias epilogue — configs[3]
                                       (heatmap L_inf ~1e-2); both variants (variant 1: CBAM statistics, MLP,
                                       maps and sigmoids in f32 from the stored bf16 values, its output rounded
                                       once; the heat-maps leave the output layer in f32);
                                    3: "fp16" — the plan, layout and cost of mode 1 with IEEE binary16 elements (11
                                       significand bits for 8, v_mfma_f32_16x16x32_f16): activations and weights stored
                                       once as fp16, rounded to nearest even, stores SATURATED at +-65504 (never inf),
                                       f32 accumulate and bias, f32 heat-maps; heatmap L_inf ~7e-4, nine times closer to
                                       the reference than mode 1 inside fp16's range; variant 0 only (esahrnet_create
                                       refuses variant 1); esahrnet_commit refuses a folded weight that is not finite in
                                       fp16.  A checkpoint whose tensors leave fp16's range is brought into it by per-tensor
                                       power-of-two scales (esahrnet_set_scale_exponents, below), at no cost per forward.
                                       A value of this field, not a new field or symbol: the ABI version stays */
} esahrnet_cfg;

/* A parameter tensor that is not a convolution of the main graph (variant 1: the CBAM weights). */
typedef struct esahrnet_aux_desc {
    char name[96];               /* state_dict key, e.g. "layer1.0.ca.fc.0.weight"               */
    int32_t shape[4];            /* Conv2d weight shape [out][in][kh][kw]                          */
} esahrnet_aux_desc;

/* One Conv2d of the reference module tree, by its state_dict prefix. */
typedef struct esahrnet_conv_desc {
    char name[96];               /* e.g. "stage3.0.fuse_layers.2.0.1.0" (conv: name + ".weight") */
    char bn[96];                 /* partner BatchNorm2d prefix, "" if none (output_layer.0)    */
    int32_t cin, cout, k, stride;
    int32_t has_bias;            /* conv carries its own bias (last_layer.0/3, output_layer.0) */
    int32_t relu;                /* a ReLU follows conv(+BN) directly                           */
} esahrnet_conv_desc;

const char* esahrnet_last_error(void);
int esahrnet_abi_version(void);

/* Build the static plan for a stage table.  `device` is the HIP device ordinal the weights
 * will live on; nothing touches the device until esahrnet_commit. */
int esahrnet_create(const esahrnet_cfg* cfg, int device, esahrnet_handle* out);
int esahrnet_destroy(esahrnet_handle h);
/* Device ordinal the handle was created for. */
int esahrnet_handle_device(esahrnet_handle h);

int esahrnet_conv_count(esahrnet_handle h);
int esahrnet_conv_desc_get(esahrnet_handle h, int index, esahrnet_conv_desc* out);

/* Hand over one convolution with BatchNorm ALREADY FOLDED (eval mode, eps 1e-5):
 * w: host f32 [cout][cin][k][k], b: host f32 [cout] (never NULL). */
int esahrnet_set_conv(esahrnet_handle h, int index, const float* w, const float* b);
int esahrnet_aux_count(esahrnet_handle h);
int esahrnet_aux_desc_get(esahrnet_handle h, int index, esahrnet_aux_desc* out);
/* w: host f32, prod(shape) elements, exactly the state_dict tensor (no folding applies). */
int esahrnet_set_aux(esahrnet_handle h, int index, const float* w);
/* Pack (split-bf16, MFMA fragment order) and upload every convolution.  Synchronous. */
int esahrnet_commit(esahrnet_handle h);

/* Bytes of caller-owned device scratch esahrnet_forward needs for a batch of n crops of h x w. */
int esahrnet_workspace_bytes(esahrnet_handle h, int n, int height, int width, size_t* bytes);

/* x_dev: f32 [n][cin][height][width] NCHW contiguous (already normalised, data_load_val.py:86).
 * heat_dev: f32 [n][K][height][width] NCHW, fully overwritten.  x_dev is not modified.
 * ws_dev (here and in every entry point below that takes one): what it holds on entry is irrelevant — zeros, NaN bit patterns
 * and the leftovers of another call give the same bits; what it holds on exit is unspecified; nothing outside
 * [ws_dev, ws_dev + ws_bytes) and the documented outputs is written; inputs are not modified. */
int esahrnet_forward(esahrnet_handle h, const void* x_dev, int n, int height, int width,
                     void* heat_dev, void* ws_dev, size_t ws_bytes, esahrnet_stream stream);

/* heat_dev: f32 [n][k][height][width] -> kp_dev: f32 [n][k][3] = (x, y, peak):
 * first-occurrence arg-max, log-quadratic sub-pixel refine, raw peak value. */
int esahrnet_keypoints(const void* heat_dev, int n, int k, int height, int width,
                       void* kp_dev, esahrnet_stream stream);
/* Same, and additionally idx_dev: int32 [n][k] = row * width + column of the arg-max (the integer coordinates
 * inference.py:22-51 get_max_preds returns; NULL: not written).  A NaN in a plane is the maximum, as for
 * np.argmax / torch.max: first NaN's index, peak NaN, no refinement. */
int esahrnet_keypoints_ex(const void* heat_dev, int n, int k, int height, int width,
                          void* kp_dev, void* idx_dev, esahrnet_stream stream);

/* ---- runner-up peaks: the M best local maxima of every heat-map (csrc/keypoints_candidates.hip) -------------------------------
 * heat_dev f32 [n][k][height][width], candidates = M in 1..ESAHRNET_MAX_CANDIDATES, nms_radius = r >= 0 ->
 *   cand_dev f32 [n][k][M][3]  (x, y, peak) per candidate, best first.
 *   cidx_dev int32 [n][k][M]   row * width + column of each candidate's pixel, -1 where there is none (NULL: not written).
 * Candidate 0 is the row and the index of esahrnet_keypoints_ex, bit for bit (first row-major arg-max, NaN counts as the
 * maximum, all-NaN and all -inf planes give index 0).  Candidate m >= 1 is the largest value among the pixels that (a) are
 * neither NaN nor -inf, (b) are local maxima: at least as large as each of their 8 neighbours — neighbours outside the plane
 * are ignored, a NaN neighbour disqualifies —, and (c) lie at Chebyshev distance greater than r from every candidate 0..m-1;
 * ties go to the lower index.  Each candidate gets the sub-pixel step of esahrnet_keypoints at its own pixel; its peak is the
 * raw value there.  When no pixel qualifies, that row and all later rows are NaN x 3 with index -1.
 * One launch, one workgroup per plane, the M sweeps of a plane back to back (the later ones read it from L2); a plane's result
 * does not depend on its batch.  No workspace.  Allocates nothing, does not synchronise, may be captured into a graph; argument
 * errors (NULL heat_dev or cand_dev, a shape that is not positive, M outside 1..4, r < 0, a pointer that is not 4-byte aligned)
 * are reported before anything is enqueued. */
#define ESAHRNET_MAX_CANDIDATES 4
int esahrnet_keypoints_candidates(const void* heat_dev, int n, int k, int height, int width, int candidates, int nms_radius,
                                  void* cand_dev, void* cidx_dev, esahrnet_stream stream);

/* ---- the second decoder: get_final2 (inference.py:154-169) ---------------------------------------------------------
 * Same arg-max, peak and idx_dev as esahrnet_keypoints_ex (bit-identical), but the sub-pixel step of get_final2: each plane
 * blurred by the 11x11 Gaussian of cv2.GaussianBlur(., (11, 11), 0) (sigma 2, zero padding, f64 sums, rounded to f32),
 * rescaled to the plane's raw maximum, clamped at 1e-10 and logged (inference.py:96-111), then one Newton step with the
 * full 2x2 Hessian, dxy included (taylor, :54-73).  The step is applied when the peak is at least 2 px inside the plane,
 * the Hessian's determinant is non-zero, and the raw maximum, the blurred maximum, the rescale factor and the offset are
 * all finite; otherwise the keypoint keeps its integer coordinates (the reference would write NaN or raise).  The blurred
 * planes are never stored: ws_dev (esahrnet_keypoints_final2_workspace_bytes bytes, 256-byte aligned) holds per-tile
 * maxima only.  The heat-maps are read once.  Allocates nothing, does not synchronise, may be captured into a graph. */
int esahrnet_keypoints_final2_workspace_bytes(int n, int k, int height, int width, size_t* bytes);
int esahrnet_keypoints_final2(const void* heat_dev, int n, int k, int height, int width, void* kp_dev, void* idx_dev,
                              void* ws_dev, size_t ws_bytes, esahrnet_stream stream);

/* esahrnet_keypoints_final2 with one more output: hess_dev f64 [n][k][3] = (dxx, dxy, dyy), the Hessian of the blurred log
 * heat-map at the peak — the very values the Newton step used (central differences of the 13 f32 log values, in f64) — or
 * NaN x 3 for a keypoint whose step was not taken (peak within 2 px of the border, det = 0, anything non-finite).  For a
 * Gaussian blob -H is the keypoint's information matrix in crop pixels (esahrnet_correspondences, mode 1).  The finish kernel
 * is instantiated with and without the output: hess_dev == NULL launches the kernels of esahrnet_keypoints_final2, and
 * kp_dev / idx_dev are bit-identical to its in either case. */
int esahrnet_keypoints_final2_hess(const void* heat_dev, int n, int k, int height, int width, void* kp_dev, void* idx_dev,
                                   void* hess_dev, void* ws_dev, size_t ws_bytes, esahrnet_stream stream);

/* ---- the third decoder: a 2-D Gaussian fitted around each peak ----------------------------------------------------------
 * The decoder the reference's test.py sketches with scipy.optimize.curve_fit: g = off + A exp(-(a dx^2 + 2 b dx dy + c dy^2)),
 * test.py's family parametrised by (a, b, c) instead of (sigma_x, sigma_y, theta), fitted to the pixels within 6 px of the
 * integer arg-max in x and in y (at most 13 x 13, clipped to the plane), one wave per plane (csrc/keypoints_gaussfit.hip).
 * esahrnet_keypoints_ex's kernel is enqueued first, unchanged; then the fit: start off = window minimum, A = peak - off,
 * centre = arg-max, a = c = 1/8, b = 0; Levenberg-Marquardt in f64 (lambda 1e-3, x 4 on a rejected step, / 3 with floor 1e-9
 * on an accepted one, at most 10 tries per iteration and 50 iterations, stop at a relative cost decrease below 1e-14); sums
 * in a fixed order, so that a plane's result does not depend on its batch.
 *   status_dev int32 [n][k]  0: accepted — every parameter and the cost finite, A > 0, a > 0, a c - b^2 > 0, and the centre
 *                            inside the window (its first to its last pixel centre, in x and in y); 1: the solver ended on a
 *                            parameter or a cost that is not finite; 2: finite, but one of the other rules fails (a constant
 *                            plane: A = 0); 3: a value in the window that is not finite (a NaN peak included).
 *   kp_dev f32 [n][k][3]     accepted: (x0, y0, raw peak); rejected: the row of esahrnet_keypoints_ex, bit for bit.  The peak
 *                            is the raw maximum either way, so the selection of keypoints does not change.
 *   idx_dev int32 [n][k]     as esahrnet_keypoints_ex writes it (NULL: not written; the fit needs the index, which then passes
 *                            through status_dev: the first kernel leaves it there, the fit reads it and stores the status).
 *   fit_dev f64 [n][k][8]    (A, x0, y0, a, b, c, off, cost), cost the sum of squared residuals; NaN x 8 when rejected (NULL:
 *                            not written).
 *   hess_dev f64 [n][k][3]   (-2a, -2b, -2c), NaN x 3 when rejected (NULL: not written).  For this model the inverse
 *                            covariance of the blob is 2 [[a, b], [b, c]], so hess_dev is, as it stands, the hess_dev of
 *                            esahrnet_correspondences(mode 1): w = rate (-H)^(1/2).
 * No workspace.  Allocates nothing, does not synchronise, may be captured into a graph; argument errors (NULL heat_dev, kp_dev
 * or status_dev, a shape that is not positive, a pointer that is not aligned to its element) are reported before anything is
 * enqueued. */
int esahrnet_keypoints_gaussfit(const void* heat_dev, int n, int k, int height, int width,
                                void* kp_dev, void* idx_dev, void* fit_dev, void* status_dev,
                                void* hess_dev, esahrnet_stream stream);

/* ---- forward + keypoints without re-reading the heat-maps -------------------------------------------------
 * The output-layer kernel can leave, beside the heat-maps, the first row-major maximum of each of its tiles:
 * part_dev = 8 bytes x [n * K][ntiles] (f32 value, int32 index row * width + column).  esahrnet_keypoints_finish reduces
 * those instead of sweeping n*K*height*width floats; its results are bit-identical to esahrnet_keypoints_ex on the same
 * heat-maps (same ordering of ties and NaNs, same refinement).  Replaces: `net(x)` followed by get_final / the host peak
 * search (val.py:151-166, inference.py:136-152).
 * esahrnet_partial_tiles: ntiles for a crop size; 0 = this handle cannot (seg_hrnet / seg_hrnet2 with a VALU output layer):
 * use esahrnet_forward + esahrnet_keypoints.  seg_hrnet3 reports them in every precision (its heat-map conversion to NCHW:
 * runs of 256 row-major pixels per tile).  part_dev == NULL makes esahrnet_forward_partials plain esahrnet_forward. */
int esahrnet_partial_tiles(esahrnet_handle h, int height, int width, int* ntiles);
int esahrnet_forward_partials(esahrnet_handle h, const void* x_dev, int n, int height, int width, void* heat_dev,
                              void* part_dev, void* ws_dev, size_t ws_bytes, esahrnet_stream stream);
int esahrnet_keypoints_finish(const void* heat_dev, const void* part_dev, int ntiles, int n, int k, int height, int width,
                              void* kp_dev, void* idx_dev, esahrnet_stream stream);

/* ---- forward straight to keypoints, without heat-maps ------------------------------------------------------
 * esahrnet_forward_keypoints runs the forward of esahrnet_forward with its last launch (the output layer, or seg_hrnet3's
 * conversion of its heat-maps to NCHW) replaced, so that no heat-map reaches caller memory: kp_dev f32 [n][K][3] = (x, y,
 * peak) and idx_dev int32 [n][K] (NULL: not written) are bit-identical to esahrnet_forward followed by esahrnet_keypoints_ex
 * on the same input and weights (same ties, NaN rule and refinement).  Replaces `net(x)` + get_final and the host peak search
 * (val.py:151-180, inference.py:136-152).  ws_dev: esahrnet_keypoints_workspace_bytes bytes (at least esahrnet_workspace_bytes
 * for the same shape), 256-byte aligned.  Like esahrnet_forward it allocates nothing, does not synchronise, may be captured
 * into a graph, and follows esahrnet_set_debug_keep and the multi-lane schedule.
 *   seg_hrnet / seg_hrnet2, VALU output layer: each tile's first maximum per heat-map, nothing stored; the finish evaluates
 *     the output layer again at the <= 9 pixels the refinement reads.
 *   seg_hrnet / seg_hrnet2, matrix-core output layer: the heat-maps go to the workspace instead of caller memory, then
 *     esahrnet_keypoints_finish's kernel (no new arithmetic: the gain is caller memory).
 *   seg_hrnet3: the tile maxima of the NHWC heat-maps already in the workspace; the refinement reads them there. */
int esahrnet_keypoints_workspace_bytes(esahrnet_handle h, int n, int height, int width, size_t* bytes);
int esahrnet_forward_keypoints(esahrnet_handle h, const void* x_dev, int n, int height, int width,
                               void* kp_dev, void* idx_dev, void* ws_dev, size_t ws_bytes, esahrnet_stream stream);

/* ---- forward straight to get_final2 keypoints ----------------------------------------------------------------
 * esahrnet_forward_keypoints_final2 is esahrnet_forward_keypoints with the second decoder: kp_dev and idx_dev are
 * bit-identical to esahrnet_forward followed by esahrnet_keypoints_final2 (same arg-max, peak, step rule, NaN, ties and
 * non-finite handling).  ws_dev: esahrnet_keypoints_final2_forward_workspace_bytes bytes, 256-byte aligned.  Same contract:
 * no allocation, no synchronisation, graph-capturable, esahrnet_set_debug_keep and the multi-lane schedule apply.
 *   seg_hrnet / seg_hrnet2, VALU output layer: the output layer is evaluated over each 22 x 22 tile and the blur's 5-pixel
 *     halo, blurred in LDS, and only the tile's raw and blurred maxima are kept (12 bytes per tile and heat-map); the finish
 *     evaluates the output layer again at the 15 x 15 pixels around the peak that the 13 blurred values read.
 *   seg_hrnet / seg_hrnet2, matrix-core output layer: the heat-maps go to the workspace instead of caller memory, then
 *     esahrnet_keypoints_final2's kernels (no new arithmetic: the gain is one call and no caller buffer).
 *   seg_hrnet3: esahrnet_keypoints_final2's kernels read the NHWC heat-maps already in the workspace; no NCHW copy is made.
 * Except for the matrix-core form, the workspace has no n * K * height * width term beyond esahrnet_workspace_bytes'. */
int esahrnet_keypoints_final2_forward_workspace_bytes(esahrnet_handle h, int n, int height, int width, size_t* bytes);
int esahrnet_forward_keypoints_final2(esahrnet_handle h, const void* x_dev, int n, int height, int width,
                                      void* kp_dev, void* idx_dev, void* ws_dev, size_t ws_bytes, esahrnet_stream stream);

/* The same with hess_dev f64 [n][K][3] as esahrnet_keypoints_final2_hess writes it, in all three forms (VALU re-evaluation,
 * matrix-core, seg_hrnet3 NHWC): bit-identical to esahrnet_forward + esahrnet_keypoints_final2_hess.  hess_dev == NULL is
 * esahrnet_forward_keypoints_final2; same workspace query. */
int esahrnet_forward_keypoints_final2_hess(esahrnet_handle h, const void* x_dev, int n, int height, int width,
                                           void* kp_dev, void* idx_dev, void* hess_dev, void* ws_dev, size_t ws_bytes,
                                           esahrnet_stream stream);

/* ---- forward straight to Gaussian-fit keypoints -------------------------------------------------------------------
 * esahrnet_forward_keypoints_gaussfit is esahrnet_forward_keypoints with the third decoder: kp_dev, idx_dev, fit_dev, status_dev
 * and hess_dev have the shapes and types of esahrnet_keypoints_gaussfit (k = K) and are bit-identical to esahrnet_forward
 * followed by esahrnet_keypoints_gaussfit on the same input and weights: the same arg-max, ties and NaN rule, the same
 * get_final row for a rejected fit, the same statuses, the same fit to the last bit.  idx_dev, fit_dev and hess_dev may be NULL.
 * No heat-map reaches caller memory.  ws_dev: esahrnet_keypoints_gaussfit_forward_workspace_bytes bytes (what
 * esahrnet_keypoints_workspace_bytes reports), 256-byte aligned; its contents on entry do not matter.  Same contract as
 * esahrnet_forward_keypoints_final2: no allocation, no synchronisation, graph-capturable, esahrnet_set_debug_keep and the
 * multi-lane schedule apply.  Argument errors (a NULL handle, x_dev, kp_dev, status_dev or ws_dev, a handle that is not
 * committed, a shape that is not positive, a workspace that is too small or not 256-byte aligned, an output pointer that is not
 * aligned to its element) are reported before anything is enqueued.
 *   seg_hrnet / seg_hrnet2, VALU output layer: each tile's first maximum per heat-map, nothing stored; the finish, one wave
 *     per heat-map, evaluates the output layer again at the <= 13 x 13 pixels of the fit's window (15 x 15 staged inputs, the
 *     arithmetic of the output layer, fma for fma), keeps them in LDS, writes the get_final row from them and runs the fit on
 *     them.  Input channels: at most 8.
 *   seg_hrnet / seg_hrnet2, matrix-core output layer: the heat-maps go to the workspace instead of caller memory, then
 *     esahrnet_keypoints_finish's kernel and the fit kernel of esahrnet_keypoints_gaussfit (no new arithmetic).
 *   seg_hrnet3: the tile maxima and the refinement of esahrnet_forward_keypoints on the NHWC heat-maps in the workspace, then
 *     the fit with its window read from them; no NCHW copy is made.
 * Except for the matrix-core form, the workspace has no n * K * height * width term beyond esahrnet_workspace_bytes'. */
int esahrnet_keypoints_gaussfit_forward_workspace_bytes(esahrnet_handle h, int n, int height, int width, size_t* bytes);
int esahrnet_forward_keypoints_gaussfit(esahrnet_handle h, const void* x_dev, int n, int height, int width,
                                        void* kp_dev, void* idx_dev, void* fit_dev, void* status_dev, void* hess_dev,
                                        void* ws_dev, size_t ws_bytes, esahrnet_stream stream);

/* Loader stage in front of the path (data_load_val.py:139-187): for each of n 8-bit frames
 * [frame_h][frame_w] take the clamped box boxes[i] = (x0, y0, x1, y1) (int32, device), edge-pad it the
 * way the reference does, resize to scale x scale (OpenCV 8-bit INTER_LINEAR arithmetic) and write
 * (v/255 - mean)/std into out_dev f32 [n][1][scale][scale] — the tensor esahrnet_forward takes. */
int esahrnet_crops(const void* frames_dev, int n, int frame_h, int frame_w, const void* boxes_dev, int scale,
                   float mean, float stdv, void* out_dev, esahrnet_stream stream);

/* ---- the loader on the device: detector boxes and frames to keypoints ------------------------------------------------
 * The box rule, the crops and the forward in one call, so that nothing between the camera frame and the keypoints passes
 * through the host (data_load_val.py:103-195 / data_load4.py:103-165 + val.py:146-180).  All four allocate nothing, do not
 * synchronise and may be captured into a graph; every argument error is reported before anything is enqueued.
 *
 * esahrnet_boxes: det_boxes_dev int32 [m][4] detector boxes (x, y, x2, y2) -> crop_boxes_dev int32 [m][4] = (x_new, y_new,
 *   w_new, h_new) ((w_new, h_new) the far corner), rates_dev f64 [m] (1.0 when the crop's size equals scale, else scale /
 *   size; size = max(w_new - x_new, h_new - y_new), IEEE division: inf for size 0), valid_dev int32 [m] (0: w_new <= x_new
 *   or h_new <= y_new, the empty crop).  rule 0: ESAValDataSet (data_load_val.py:127-158); rule 1: ESADataSet
 *   (data_load4.py:112-141: the box is forced square before the clamps).  Python's arithmetic: centre and half size by true
 *   division in f64, 1.05 * size rounded before it is added, int() truncating toward zero.
 * esahrnet_crops_ex: esahrnet_crops with (a) frame_idx_dev int32 [m] (NULL: identity, m == nframes): crop i reads frame
 *   frame_idx[i]; (b) pixel_format 0: gray8 [nframes][frame_h][frame_w], 1: RGB8 interleaved [nframes][frame_h][frame_w][3],
 *   each source pixel reduced as PIL's convert('L') does (data_load_val.py:110-117): L = (R*19595 + G*38470 + B*7471 +
 *   0x8000) >> 16, before the resize; (c) valid_dev int32 [m] (NULL: all valid).  A crop with valid[i] == 0, a frame index
 *   outside [0, nframes) or a box that is empty or leaves the frame is written as zeros.  crop_boxes_dev as esahrnet_boxes
 *   wrote it.  On gray frames with the identity index out_dev f32 [m][1][scale][scale] is bit-identical to esahrnet_crops'.
 * esahrnet_frames_keypoints: esahrnet_boxes -> esahrnet_crops_ex into the head of the workspace -> esahrnet_forward_keypoints
 *   (decoder 0) or esahrnet_forward_keypoints_final2 (decoder 1) on the rest -> the rows of kp_dev f32 [m][K][3] (and of
 *   idx_dev int32 [m][K], NULL: not written) whose crop is invalid become NaN (-1); valid rows are bit-identical to the calls it
 *   is built from.  valid_dev here also is 0 for a frame index out of range.  crop_boxes_dev, rates_dev, valid_dev are outputs
 *   the host pose stage needs (esahrnet_pnp_batch: boxes_xy, rates).  ws_dev: esahrnet_frames_keypoints_workspace_bytes bytes
 *   (the chosen decoder's query for m crops of scale x scale plus the crop tensor), 256-byte aligned.  Handles with cin != 1
 *   are refused: the reference has no loader for 3-channel crops. */
int esahrnet_boxes(const void* det_boxes_dev, int m, int frame_h, int frame_w, int scale, int rule,
                   void* crop_boxes_dev, void* rates_dev, void* valid_dev, esahrnet_stream stream);
int esahrnet_crops_ex(const void* frames_dev, int nframes, int frame_h, int frame_w, int pixel_format,
                      const void* frame_idx_dev, const void* crop_boxes_dev, const void* valid_dev, int m,
                      int scale, float mean, float stdv, void* out_dev, esahrnet_stream stream);
int esahrnet_frames_keypoints_workspace_bytes(esahrnet_handle h, int m, int scale, int decoder, size_t* bytes);
int esahrnet_frames_keypoints(esahrnet_handle h, const void* frames_dev, int nframes, int frame_h, int frame_w,
                              int pixel_format, const void* det_boxes_dev, const void* frame_idx_dev, int m,
                              int scale, int rule, float mean, float stdv, int decoder,
                              void* kp_dev, void* idx_dev, void* crop_boxes_dev, void* rates_dev, void* valid_dev,
                              void* ws_dev, size_t ws_bytes, esahrnet_stream stream);

/* esahrnet_frames_keypoints_gaussfit: esahrnet_frames_keypoints with the third decoder, a symbol of its own (decoder = 2 is not
 * a value of esahrnet_frames_keypoints): esahrnet_boxes -> esahrnet_crops_ex into the head of the workspace ->
 * esahrnet_forward_keypoints_gaussfit on the rest -> the rows of an invalid crop (valid == 0) become kp NaN, idx -1, fit and hess
 * NaN, status -1; valid rows are bit-identical to the calls it is built from.  idx_dev, fit_dev and hess_dev may be NULL.  ws_dev:
 * esahrnet_frames_keypoints_gaussfit_workspace_bytes bytes, 256-byte aligned.  The refusals (cin != 1 among them) and the
 * graph-capture contract are esahrnet_frames_keypoints', with the alignment rules of esahrnet_keypoints_gaussfit.  hess_dev is, as
 * it stands, the hess_dev of esahrnet_correspondences(mode 1): enqueue that call behind this one on the same stream for
 * Hessian-weighted correspondences. */
int esahrnet_frames_keypoints_gaussfit_workspace_bytes(esahrnet_handle h, int m, int scale, size_t* bytes);
int esahrnet_frames_keypoints_gaussfit(esahrnet_handle h, const void* frames_dev, int nframes, int frame_h, int frame_w,
                                       int pixel_format, const void* det_boxes_dev, const void* frame_idx_dev, int m,
                                       int scale, int rule, float mean, float stdv,
                                       void* kp_dev, void* idx_dev, void* fit_dev, void* status_dev, void* hess_dev,
                                       void* crop_boxes_dev, void* rates_dev, void* valid_dev,
                                       void* ws_dev, size_t ws_bytes, esahrnet_stream stream);

/* ---- the Gaussian fit with the covariance of the fitted centre ------------------------------------------------------------------
 * What scipy's curve_fit returns beside the parameters (the reference's test.py:43 `popt, pcov`), for the centre: the (x0, y0)
 * block of pcov = s^2 (J^T J)^-1, s^2 = cost / (n - 7).  Unlike hess_dev, which describes the shape of the blob, it grows with the
 * residual noise and shrinks with the amplitude; evaluation.py:471-487 turns such a covariance into the PnP weight inv(sqrtm(covar))
 * and gives weight zero where covar[0, 0] < 1e-6 or NaN.  Each of the three entries below is its sibling without _cov with three
 * more arguments; an accepted fit (status 0) goes on as follows, every lane the same, contraction off, sums in the fit's order:
 *   1. residuals and the analytic Jacobian once more, at the returned parameters; N = J^T J (7 x 7) with the per-lane slot order
 *      and the butterfly of the iteration, so that a plane's result does not depend on its batch;
 *   2. dof = n - 7, n the number of window pixels; s^2 = cost / dof, cost the value in fit_dev[7];
 *   3. N factored by the iteration's Cholesky with lambda = 0 (no damping); the x0 and the y0 column of N^-1 by its two
 *      triangular solves;
 *   4. cov = s^2 (N^-1[1][1], N^-1[2][1], N^-1[2][2]) = (cxx, cxy, cyy), in crop px^2;
 *   5. det = cxx cyy - cxy cxy;  info = (-(cyy / det), cxy / det, -(cxx / det)) = -cov^-1, plain IEEE operations in this order.
 *   cov_dev  f64 [n][k][3]   NaN x 3 when the fit is rejected, dof <= 0, a pivot is not positive or a value of cov is not finite
 *                            (NULL: not written).
 *   info_dev f64 [n][k][3]   NaN x 3 where cov is NaN, det is not positive, or cxx < cov_floor (the reference's guard looks at
 *                            covar[0, 0] only) (NULL: not written).  It is, as it stands, a hess_dev of
 *                            esahrnet_correspondences(mode 1): w = rate (-info)^(1/2) = rate cov^(-1/2), inv(sqrtm(covar)) in image
 *                            pixels, and weight zero where it is NaN, as for a rejected fit.
 *   cov_floor                a number >= 0 (the reference: 1e-6); NaN or a negative value is an argument error.
 * The status is not changed by any of this: it describes the fit only.  With both pointers NULL a call launches exactly the
 * kernels of its sibling; with either given, kp_dev, idx_dev, fit_dev, status_dev and hess_dev are bit-identical to the sibling's
 * (the fit kernel is instantiated with the covariance pass behind the same code).  cov_dev and info_dev must be 8-byte aligned.
 * Every argument error, the sibling's included, is reported before anything is enqueued; the calls allocate nothing, do not
 * synchronise and may be captured into a graph.  esahrnet_forward_keypoints_gaussfit_cov takes the workspace of
 * esahrnet_keypoints_gaussfit_forward_workspace_bytes, esahrnet_frames_keypoints_gaussfit_cov that of
 * esahrnet_frames_keypoints_gaussfit_workspace_bytes; in the latter the rows of an invalid crop are NaN in cov_dev and info_dev too. */
int esahrnet_keypoints_gaussfit_cov(const void* heat_dev, int n, int k, int height, int width,
                                    void* kp_dev, void* idx_dev, void* fit_dev, void* status_dev, void* hess_dev,
                                    void* cov_dev, void* info_dev, double cov_floor, esahrnet_stream stream);
int esahrnet_forward_keypoints_gaussfit_cov(esahrnet_handle h, const void* x_dev, int n, int height, int width,
                                            void* kp_dev, void* idx_dev, void* fit_dev, void* status_dev, void* hess_dev,
                                            void* cov_dev, void* info_dev, double cov_floor,
                                            void* ws_dev, size_t ws_bytes, esahrnet_stream stream);
int esahrnet_frames_keypoints_gaussfit_cov(esahrnet_handle h, const void* frames_dev, int nframes, int frame_h, int frame_w,
                                           int pixel_format, const void* det_boxes_dev, const void* frame_idx_dev, int m,
                                           int scale, int rule, float mean, float stdv,
                                           void* kp_dev, void* idx_dev, void* fit_dev, void* status_dev, void* hess_dev,
                                           void* crop_boxes_dev, void* rates_dev, void* valid_dev,
                                           void* cov_dev, void* info_dev, double cov_floor,
                                           void* ws_dev, size_t ws_bytes, esahrnet_stream stream);

/* ---- runner-up peaks in one sweep, in the forward and behind the loader (csrc/keypoints_candidates_onepass.hip) ----------------
 * esahrnet_keypoints_candidates_form: esahrnet_keypoints_candidates with the kernel named.  form 0: the multi-sweep kernel of
 * esahrnet_keypoints_candidates (one sweep of the plane per candidate).  form 1: the one-sweep kernel: one sweep finds every
 * qualifying local maximum and keeps the best of each 8 x 8 cell in an LDS table, and each runner-up rescans only the cells its
 * predecessor's suppression square touches; cand_dev and cidx_dev are bit-identical to form 0's.  It serves planes with heat_dev
 * 16-byte aligned, width a multiple of 4 and at most 4096 cells (ceil(height / 8) * ceil(width / 8): 512 x 512); on any other
 * plane form 1 is an argument error.  form -1: what the fused entries below launch: the one-sweep kernel where it serves and is
 * the faster one (M >= 2), the multi-sweep kernel otherwise, so every plane has a result.  The other argument errors
 * and their texts are esahrnet_keypoints_candidates'; all are reported before anything is enqueued.  No workspace, no allocation,
 * no synchronisation; a plane's result does not depend on its batch. */
int esahrnet_keypoints_candidates_form(const void* heat_dev, int n, int k, int height, int width, int candidates, int nms_radius,
                                       int form, void* cand_dev, void* cidx_dev, esahrnet_stream stream);

/* esahrnet_forward_keypoints_candidates: the forward with the candidate decoder in place of its last launch.  cand_dev f32
 * [n][K][M][3] and cidx_dev int32 [n][K][M] (NULL: not written) are bit-identical to esahrnet_forward followed by
 * esahrnet_keypoints_candidates on its heat-maps; no heat-map reaches caller memory.  The runner-up rule needs whole planes, so
 * the output layer (or seg_hrnet3's conversion) writes them into the workspace: esahrnet_keypoints_candidates_forward_workspace_bytes
 * is esahrnet_workspace_bytes plus n * K * height * width * 4 bytes, padded to 256.  Allocates nothing, does not synchronise, may
 * be captured into a graph.  The refusals, in their order: a NULL handle or cand_dev; M outside 1..ESAHRNET_MAX_CANDIDATES; r < 0; a
 * cand_dev or cidx_dev that is not 4-byte aligned; then those of esahrnet_forward_keypoints (NULL x_dev or ws_dev, a handle
 * without esahrnet_commit, the shape, the workspace's size and alignment) -- all before anything is enqueued. */
int esahrnet_keypoints_candidates_forward_workspace_bytes(esahrnet_handle h, int n, int height, int width, size_t* bytes);
int esahrnet_forward_keypoints_candidates(esahrnet_handle h, const void* x_dev, int n, int height, int width, int candidates,
                                          int nms_radius, void* cand_dev, void* cidx_dev, void* ws_dev, size_t ws_bytes,
                                          esahrnet_stream stream);

/* esahrnet_frames_keypoints_candidates: esahrnet_frames_keypoints with the candidate decoder: esahrnet_boxes -> esahrnet_crops_ex
 * into the head of the workspace -> esahrnet_forward_keypoints_candidates on the rest -> the rows of an invalid crop (valid == 0)
 * become NaN in cand_dev and -1 in cidx_dev (NULL: not written); valid rows are bit-identical to the calls it is built from.
 * ws_dev: esahrnet_frames_keypoints_candidates_workspace_bytes bytes, 256-byte aligned.  The refusals (cin != 1 among them) and
 * the graph-capture contract are esahrnet_frames_keypoints'; M, r and the alignment of cand_dev / cidx_dev are checked behind
 * the frames' and boxes' arguments and before the handle's commit. */
int esahrnet_frames_keypoints_candidates_workspace_bytes(esahrnet_handle h, int m, int scale, size_t* bytes);
int esahrnet_frames_keypoints_candidates(esahrnet_handle h, const void* frames_dev, int nframes, int frame_h, int frame_w,
                                         int pixel_format, const void* det_boxes_dev, const void* frame_idx_dev, int m,
                                         int scale, int rule, float mean, float stdv, int candidates, int nms_radius,
                                         void* cand_dev, void* cidx_dev, void* crop_boxes_dev, void* rates_dev, void* valid_dev,
                                         void* ws_dev, size_t ws_bytes, esahrnet_stream stream);

/* ---- keypoints to the record the pose solver consumes, on the device (val.py:172-180) -------------------------------------
 * esahrnet_correspondences (correspond_kernel, one wave per crop, k <= 32): kp_dev f32 [m][k][3] keypoint rows, crop_boxes_dev /
 *   rates_dev / valid_dev as esahrnet_boxes wrote them ->
 *     count_dev int32 [m]       keypoints handed to the solver: max(#(peak > thresh), min_k), at most k;
 *     order_dev int32 [m][k]    their indices, largest peak first, equal peaks by lower index (heapq.nlargest); -1 beyond count;
 *     pts_dev   f64 [m][k][2]   image pixels in that order: p * (1 / rate) + (x_new, y_new), bit-identical to what
 *                               esahrnet_pnp_batch computes for its image points (one shared header, csrc/correspond.h);
 *     w_dev     f64 [m][k][3]   (wxx, wxy, wyy), the symmetric 2x2 weight of uncertainty_pnp.cpp:30-31, in that order.
 *   pts and w are zero beyond count.  mode 0 "peak": w = (peak, 0, peak), the scalar weight of val.py:194-209; hess_dev unused
 *   (may be NULL).  mode 1 "hessian": w = rate * (-H)^(1/2), H = hess_dev f64 [m][k][3] from the get_final2 decoder
 *   (esahrnet_keypoints_final2_hess): the closed-form symmetric square root of the 2x2 information matrix, scaled to image
 *   pixels (d_img = d_crop / rate); w = 0 when -H is not positive definite, H is NaN or the weight is not finite — the point
 *   still reaches EPnP / RANSAC but carries no weight in the refinement.  An invalid crop (valid == 0) has count 0.  A NaN
 *   peak in a valid crop is never selected (count is at most the number of peaks that are numbers).
 * esahrnet_frames_correspondences: esahrnet_frames_keypoints (same arguments, same kp_dev / idx_dev / crop_boxes_dev /
 *   rates_dev / valid_dev outputs, bit-identical) followed by esahrnet_correspondences on its outputs, the Hessian passing
 *   through the workspace.  decoder 0 with mode 1 is refused: get_final computes no Hessian.  ws_dev:
 *   esahrnet_frames_correspondences_workspace_bytes bytes, 256-byte aligned.
 * All three allocate nothing, do not synchronise and may be captured into a graph.  Argument errors are reported before
 * anything is enqueued (esahrnet_frames_correspondences: as far as esahrnet_frames_keypoints does — its checks and its
 * workspace query, which plans the shape, run first; a failure inside the forward after that would come behind the box
 * and crop launches). */
int esahrnet_correspondences(const void* kp_dev, const void* hess_dev, const void* crop_boxes_dev, const void* rates_dev,
                             const void* valid_dev, int m, int k, double thresh, int min_k, int mode, void* count_dev,
                             void* order_dev, void* pts_dev, void* w_dev, esahrnet_stream stream);
int esahrnet_frames_correspondences_workspace_bytes(esahrnet_handle h, int m, int scale, int decoder, int mode, size_t* bytes);
int esahrnet_frames_correspondences(esahrnet_handle h, const void* frames_dev, int nframes, int frame_h, int frame_w,
                                    int pixel_format, const void* det_boxes_dev, const void* frame_idx_dev, int m, int scale,
                                    int rule, float mean, float stdv, int decoder, double thresh, int min_k, int mode,
                                    void* kp_dev, void* idx_dev, void* crop_boxes_dev, void* rates_dev, void* valid_dev,
                                    void* count_dev, void* order_dev, void* pts_dev, void* w_dev, void* ws_dev, size_t ws_bytes,
                                    esahrnet_stream stream);

/* Host pose solve behind the path, for a batch (pnp.py:46-90 + cpnp.cpnp_m of val.py:194-209 + val.py:172-180,
 * 221-224): kp = host f32 [n][k][3] keypoint rows (x, y, peak) in crop coordinates as esahrnet_keypoints wrote
 * them; kp3d = f64 [k][3] model points; K9 = f64 row-major camera matrix; boxes_xy = int32 [n][2] crop origins;
 * rates = f64 [n] crop scale factors.  Per image: keypoints with peak > thresh (at least min_k, largest first),
 * mapped back to image pixels — selection and back-projection are the functions of csrc/correspond.h, the header the device
 * stage esahrnet_correspondences shares —, EPnP + RANSAC (5 px, 100 iterations, 0.99), peak-weighted LM refinement,
 * -> q_out f64 [n][4] = [w, x, y, z], t_out f64 [n][3] (NaN when fewer than 4 keypoints or no solution).
 * Pure host code, `threads` worker threads; needs no GPU.  Returns 0, or 1 on a bad argument. */
int esahrnet_pnp_batch(const float* kp, int n, int k, const double* kp3d, const double* K9, const int* boxes_xy,
                       const double* rates, double thresh, int min_k, int threads, double* q_out, double* t_out);
/* The same solver on records esahrnet_correspondences wrote (host copies): pts f64 [m][k][2], w f64 [m][k][3], count int32
 * [m], order int32 [m][k]; image i solves on its first count[i] points, model point kp3d[order[i][j]] for point j: EPnP +
 * RANSAC on pts, then the LM refinement with the full 2x2 weight, r = [wxx dx + wxy dy, wxy dx + wyy dy]
 * (uncertainty_pnp.cpp:30-31).  With w = (peak, 0, peak) the poses are bit-identical to esahrnet_pnp_batch's (which runs
 * this code with those weights).  count outside 0..k or an order entry outside 0..k-1 is refused. */
int esahrnet_pnp_batch_w(const double* pts, const double* w, const int* count, int m, int k, const double* kp3d,
                         const int* order, const double* K9, int threads, double* q_out, double* t_out);

/* What a solve reports about its pose: one row of ESAHRNET_POSE_REPORT_DOUBLES f64 per image, integer-valued fields stored
 * as exact doubles.  Without a pose (status 1 or 2; q and t are NaN) every field but STATUS and N is NaN. */
enum esahrnet_pose_report {
    ESAHRNET_REPORT_STATUS = 0,        /* 0 = solved; 1 = no pose, fewer than 4 correspondences; 2 = no pose, EPnP found no model
                                          on the consensus set */
    ESAHRNET_REPORT_FLAGS = 1,         /* bit 0: RANSAC found no consensus of >= 4 points and all points were used; bit 1: no
                                          covariance, J^T J is not positive definite (a Cholesky pivot at or below 1e-12 of its
                                          diagonal entry); COV is NaN then and the pose is still returned */
    ESAHRNET_REPORT_N = 2,             /* correspondences given */
    ESAHRNET_REPORT_INLIERS = 3,       /* size of the best consensus set (5 px); N when flag bit 0 is set */
    ESAHRNET_REPORT_RANSAC_ITERS = 4,  /* minimal sets drawn, 1..100 */
    ESAHRNET_REPORT_LM_ITERS = 5,      /* outer Levenberg-Marquardt iterations run (one Jacobian each), 1..50 */
    ESAHRNET_REPORT_COST = 6,          /* final sum r^2 of the weighted residuals r = [wxx dx + wxy dy, wxy dx + wyy dy] */
    ESAHRNET_REPORT_RMS_PX = 7,        /* sqrt(mean_i |proj_i - obs_i|^2) over the N points, unweighted, image pixels */
    ESAHRNET_REPORT_MAX_PX = 8,        /* largest unweighted reprojection distance */
    ESAHRNET_REPORT_ARGMAX = 9,        /* position of that point in the record's rank order (0..N-1; the first of equals) */
    ESAHRNET_REPORT_MIN_DEPTH = 10,    /* smallest camera-frame Z over the N model points at the pose; <= 0: a point lies behind
                                          the camera */
    ESAHRNET_REPORT_S2 = 11,           /* COST / (2 N - 6): the residual variance per degree of freedom */
    ESAHRNET_REPORT_COV = 12,          /* 21 doubles: upper triangle, row-major, of the 6x6 inverse of J^T J (by Cholesky), J the
                                          weighted Jacobian of r at the returned pose.  NOT scaled by S2.  Parameter order
                                          (dw_x, dw_y, dw_z, dt_x, dt_y, dt_z): dw the left-multiplicative rotation increment
                                          R <- exp([dw]x) R in radians, camera frame; dt in the units of kp3d */
    ESAHRNET_POSE_REPORT_DOUBLES = 33
};
/* esahrnet_pnp_batch / esahrnet_pnp_batch_w with a report: report = f64 [n or m][ESAHRNET_POSE_REPORT_DOUBLES], or null.  The
 * same solve: q_out and t_out are bit-identical to the entries above for every input and thread count (those entries are
 * these with report = null), and a report row depends on its image alone, so it has the same bits for any `threads`.  The
 * row is computed from the finished pose — one more Jacobian evaluation and one 6x6 factorisation per image. */
int esahrnet_pnp_batch_ex(const float* kp, int n, int k, const double* kp3d, const double* K9, const int* boxes_xy,
                          const double* rates, double thresh, int min_k, int threads, double* q_out, double* t_out,
                          double* report);
int esahrnet_pnp_batch_w_ex(const double* pts, const double* w, const int* count, int m, int k, const double* kp3d,
                            const int* order, const double* K9, int threads, double* q_out, double* t_out, double* report);

/* esahrnet_pnp_batch_ex on the candidates esahrnet_keypoints_candidates wrote (a host copy), with one repair step: cand = f32
 * [n][k][M][3], M = candidates in 1..ESAHRNET_MAX_CANDIDATES; kp3d, K9, boxes_xy, rates, thresh, min_k as above; min_ratio a
 * number >= 0.  Per image:
 *   1. the solve of esahrnet_pnp_batch_ex on candidate 0 of every keypoint: pose P1, report row R1;
 *   2. done, with P1, when M = 1, R1's status is not 0 or its flag bit 0 is set (no consensus of at least 4);
 *   3. the judge is the RANSAC consensus pose — EPnP on the best consensus set, BEFORE the LM refinement, which an outlier has
 *      already pulled;
 *   4. for every selected keypoint whose candidate 0 lies >= 5 px (the RANSAC threshold) from its projection under the judge:
 *      a candidate m >= 1 of that keypoint qualifies when its coordinates are finite, peak_m >= min_ratio * peak_0 and its own
 *      distance to the projection is < 5 px; the qualifying candidate with the smallest distance (ties: the lower m) replaces
 *      candidate 0, as point and as weight;
 *   5. done, with P1, when nothing was replaced;
 *   6. otherwise the same solve (same selection order, same seed) on the repaired points: P2, R2, taken iff R2's status is 0
 *      and R2.INLIERS > R1.INLIERS; else P1 and R1.
 * used = int32 [n][k]: the candidate each keypoint entered the returned pose's solve with, -1 for a keypoint that was not
 * selected (all of them in an image without a pose keep what the selection gave them: 0 or -1).  report: f64
 * [n][ESAHRNET_POSE_REPORT_DOUBLES] of the returned pose, or null.  With M = 1, and for every image in which nothing is
 * replaced or P2 is not taken, q_out, t_out and the report row are bit-identical to esahrnet_pnp_batch_ex on candidate 0.  A row
 * depends on its image alone: the same bits for any `threads`.  Refused: a null pointer but report, n < 0, k outside 1..64, M
 * outside 1..4, a min_ratio that is negative or NaN. */
int esahrnet_pnp_batch_cand(const float* cand, int n, int k, int candidates, const double* kp3d, const double* K9,
                            const int* boxes_xy, const double* rates, double thresh, int min_k, double min_ratio, int threads,
                            double* q_out, double* t_out, double* report, int* used);

/* ---- the decoders at pixels the caller names (csrc/keypoints_at.hip) ---------------------------------------------
 * esahrnet_keypoints_at: heat_dev f32 [n][k][height][width] and at_dev int32 [n][k][m], m >= 1 pixels per heat-map as row * width +
 * column (what idx_dev and cidx_dev of the other decoders hold) -> kp_dev f32 [n][k][m][3] = (x, y, raw value at the pixel), slot
 * (plane, j) decoded at at_dev[plane][j] by one wave:
 *   decoder 0  get_final: the row esahrnet_keypoints_ex writes for a plane whose arg-max is that pixel, the row
 *              esahrnet_keypoints_candidates writes for a candidate there, bit for bit; a row of the reference's
 *              get_final(hm, coords) (inference.py:136-152) plus the raw value.  Optional outputs: none.
 *   decoder 1  get_final2 (inference.py:154-169).  The rescale factor stays a quantity of the whole plane, raw maximum over blurred
 *              maximum (inference.py:104-109): the tile pass of esahrnet_keypoints_final2 runs once per plane, whatever m, and the
 *              finish of a slot evaluates the 13 blurred points around its own pixel, then the guards and the Newton step of
 *              esahrnet_keypoints_final2_hess.  When no step is taken (a pixel within 2 px of the border, det == 0, a maximum, factor
 *              or offset that is not finite) the row keeps the integer pixel and hess is NaN x 3.  The third column is the raw value
 *              at the pixel, not the plane's maximum.  Optional output: hess_dev f64 [n][k][m][3] = (dxx, dxy, dyy).  At the plane's
 *              arg-max kp and hess have the bits of esahrnet_keypoints_final2_hess.  ws_dev: esahrnet_keypoints_at_workspace_bytes
 *              bytes (what esahrnet_keypoints_final2_workspace_bytes asks for: it does not grow with m), 256-byte aligned; the
 *              result does not depend on what it held.
 *   decoder 2  gaussfit: decoder 0's row at the pixel, then the fit of esahrnet_keypoints_gaussfit_cov on the 13 x 13 window around
 *              that pixel; an accepted fit replaces x and y, a rejected one keeps decoder 0's row.  status_dev is required; optional
 *              outputs: fit_dev f64 [n][k][m][8], hess_dev, cov_dev and info_dev f64 [n][k][m][3], with the meaning they have in
 *              esahrnet_keypoints_gaussfit_cov (cov_floor too); at the plane's arg-max every output has that entry's bits.
 * Decoders 0 and 2 need no workspace (0 bytes; ws_dev may be NULL).  status_dev int32 [n][k][m] (NULL with decoders 0 and 1: not
 * written): decoder 2's fit status, 0 with decoders 0 and 1; -1 for a pixel outside the plane.
 * A pixel outside [0, height * width) cannot be refused from inside a kernel (-1 is what cidx_dev holds where a heat-map has no
 * candidate): that slot gets NaN x 3 in kp_dev, NaN in every f64 output and status -1, and nothing of the plane is read for it.
 * Every output is written whole; heat_dev and at_dev are only read.  A slot's result depends on its plane and its pixel alone, not
 * on n, k, m or its place among them.  The call allocates nothing, does not synchronise and may be captured into a graph.
 * Refused, in this order and before anything is enqueued: a NULL heat_dev, at_dev or kp_dev; a size that is not positive, height *
 * width or n * k beyond int32; m < 1 (or n * k * m beyond int32); a decoder outside 0..2; an output the decoder does not write that
 * is not NULL (decoder 0: hess_dev, fit_dev, cov_dev, info_dev; decoder 1: fit_dev, cov_dev, info_dev); decoder 2 without
 * status_dev; a cov_floor that is negative or not finite (every decoder); heat_dev, at_dev, kp_dev or status_dev not 4-byte aligned;
 * hess_dev, fit_dev, cov_dev or info_dev not 8-byte aligned; decoder 1: more than 2^23 - 1 tiles, a workspace that is NULL or too
 * small, a workspace that is not 256-byte aligned.
 *
 * esahrnet_keypoints_candidates_refined: esahrnet_keypoints_candidates_form(form -1) into cand_dev f32 [n][k][M][3] and cidx_dev int32
 * [n][k][M] (required here), then the kernels above with at_dev = cidx_dev and kp_dev = cand_dev: the refined (x, y) of every
 * candidate go into cand_dev, the peak column keeps the candidate kernel's value (the raw value at the pixel), rows without a
 * candidate stay NaN.  With decoder 0 cand_dev and cidx_dev are esahrnet_keypoints_candidates', bit for bit (nothing more is launched
 * unless status_dev is given); with decoders 1 and 2 every output has the bits of the two calls made one after the other.  Refused:
 * a NULL heat_dev, cand_dev or cidx_dev, the shape, M outside 1..ESAHRNET_MAX_CANDIDATES, r < 0, then everything above with m = M. */
int esahrnet_keypoints_at_workspace_bytes(int n, int k, int height, int width, int decoder, size_t* bytes);
int esahrnet_keypoints_at(const void* heat_dev, int n, int k, int height, int width, const void* at_dev, int m, int decoder,
                          void* kp_dev, void* hess_dev, void* fit_dev, void* status_dev, void* cov_dev, void* info_dev,
                          double cov_floor, void* ws_dev, size_t ws_bytes, esahrnet_stream stream);
int esahrnet_keypoints_candidates_refined(const void* heat_dev, int n, int k, int height, int width, int candidates, int nms_radius,
                                          int decoder, void* cand_dev, void* cidx_dev, void* hess_dev, void* fit_dev,
                                          void* status_dev, void* cov_dev, void* info_dev, double cov_floor, void* ws_dev,
                                          size_t ws_bytes, esahrnet_stream stream);

/* ---- the refined candidates in the forward and behind the loader (csrc/plan.hip) ------------------------------
 * esahrnet_forward_keypoints_candidates_refined: the forward with its heat-maps written into the workspace, as
 * esahrnet_forward_keypoints_candidates does, then esahrnet_keypoints_candidates_refined on them: the search of form -1, then the
 * kernels of esahrnet_keypoints_at with at_dev = the candidates' pixels and kp_dev = cand_dev.  The outputs have the shapes and
 * meanings they have there (cand_dev f32 [n][K][M][3], cidx_dev int32 [n][K][M], hess_dev / cov_dev / info_dev f64 [n][K][M][3],
 * fit_dev f64 [n][K][M][8], status_dev int32 [n][K][M]) and every one is bit-identical to esahrnet_forward followed by
 * esahrnet_keypoints_candidates_refined on its heat-maps.  cidx_dev may be NULL here (the stand-alone entry requires it): the
 * pixels then stay in the workspace and the other outputs keep their bits.  decoder 0: the bits of
 * esahrnet_forward_keypoints_candidates, and nothing more is launched unless status_dev is given.
 * Workspace: esahrnet_keypoints_candidates_refined_forward_workspace_bytes(decoder) =
 *     esahrnet_keypoints_candidates_forward_workspace_bytes
 *   + n * K * ESAHRNET_MAX_CANDIDATES * 4 bytes padded to 256 (the pixels; always, the query knows no M)
 *   + decoder 1 only: esahrnet_keypoints_at_workspace_bytes(n, K, height, width, 1);
 * 256-byte aligned; the result does not depend on what it held on entry.  Allocates nothing, does not synchronise, may be captured
 * into a graph; every output is written whole.  No heat-map reaches caller memory.
 * Refused, in this order and before anything is enqueued (a handle without weights or a device answers): a NULL handle or
 * cand_dev; M outside 1..ESAHRNET_MAX_CANDIDATES; r < 0; a decoder outside 0..2; an output the decoder does not write that is not
 * NULL (decoder 0: hess_dev, fit_dev, cov_dev, info_dev; decoder 1: fit_dev, cov_dev, info_dev); decoder 2 without status_dev; a
 * cov_floor that is negative or not finite; cand_dev, cidx_dev or status_dev not 4-byte aligned; hess_dev, fit_dev, cov_dev or
 * info_dev not 8-byte aligned; then those of esahrnet_forward_keypoints (NULL x_dev or ws_dev, a handle without esahrnet_commit, the
 * shape, the workspace's size and alignment).  The query refuses a NULL argument, then a decoder outside 0..2, then the shape. */
int esahrnet_keypoints_candidates_refined_forward_workspace_bytes(esahrnet_handle h, int n, int height, int width, int decoder,
                                                                  size_t* bytes);
int esahrnet_forward_keypoints_candidates_refined(esahrnet_handle h, const void* x_dev, int n, int height, int width, int candidates,
                                                  int nms_radius, int decoder, void* cand_dev, void* cidx_dev, void* hess_dev,
                                                  void* fit_dev, void* status_dev, void* cov_dev, void* info_dev, double cov_floor,
                                                  void* ws_dev, size_t ws_bytes, esahrnet_stream stream);

/* esahrnet_frames_keypoints_candidates_refined: esahrnet_frames_keypoints_candidates with the entry above in the place of
 * esahrnet_forward_keypoints_candidates: esahrnet_boxes -> esahrnet_crops_ex into the head of the workspace -> the refined
 * candidates' forward on the rest.  The rows of a valid crop are bit-identical to the calls it is built from; the rows of an
 * invalid crop (valid == 0: an empty box, a frame index out of range) are NaN in cand_dev and in every f64 output and -1 in cidx_dev
 * and status_dev (mark_invalid_refined_kernel; NULL outputs are not written).  ws_dev:
 * esahrnet_frames_keypoints_candidates_refined_workspace_bytes(decoder) bytes = the crops (m * scale * scale * 4 padded to 256) plus
 * the entry above's workspace for m crops of scale x scale; 256-byte aligned.  The graph-capture contract is
 * esahrnet_frames_keypoints'.  Refused, before anything is enqueued: a NULL handle, frames, boxes, cand_dev, crop_boxes_dev,
 * rates_dev, valid_dev or ws_dev; the frames' and boxes' arguments as esahrnet_frames_keypoints refuses them; then the entry above's
 * own checks from M to the alignment of the outputs; then a handle without esahrnet_commit; a handle that takes cin != 1 channels;
 * the workspace's size and alignment. */
int esahrnet_frames_keypoints_candidates_refined_workspace_bytes(esahrnet_handle h, int m, int scale, int decoder, size_t* bytes);
int esahrnet_frames_keypoints_candidates_refined(esahrnet_handle h, const void* frames_dev, int nframes, int frame_h, int frame_w,
                                                 int pixel_format, const void* det_boxes_dev, const void* frame_idx_dev, int m,
                                                 int scale, int rule, float mean, float stdv, int candidates, int nms_radius,
                                                 int decoder, void* cand_dev, void* cidx_dev, void* hess_dev, void* fit_dev,
                                                 void* status_dev, void* cov_dev, void* info_dev, double cov_floor,
                                                 void* crop_boxes_dev, void* rates_dev, void* valid_dev, void* ws_dev, size_t ws_bytes,
                                                 esahrnet_stream stream);

/* esahrnet_pnp_batch_cand with the 2x2 weights of esahrnet_correspondences(mode 1) in the refinement: hess = f64 [n][k][M][3], for
 * every candidate the Hessian (hess_dev of esahrnet_keypoints_at / _candidates_refined with decoder 1 or 2) or gaussfit's info_dev
 * (decoder 2), a host copy.  The same steps 1-6: selection and back-projection (csrc/correspond.h), the RANSAC consensus pose as the
 * judge, the swap rule on distances and peak ratios, acceptance iff the consensus grew.  One thing differs: in both solves the LM
 * weight of every point, a primary or a runner-up that was swapped in, is rate * (-hess[i][j][m])^(1/2) (corr_hessian_weight, the
 * weight esahrnet_correspondences(mode 1) gives), which is zero where -H is not positive definite or holds a NaN -- such a point
 * still reaches EPnP / RANSAC.  hess == NULL: the peak weights, esahrnet_pnp_batch_cand's outputs bit for bit.  A row depends on
 * its image alone: the same bits for any `threads`.  Refused: what esahrnet_pnp_batch_cand refuses, with this entry's name. */
int esahrnet_pnp_batch_cand_w(const float* cand, const double* hess, int n, int k, int candidates, const double* kp3d,
                              const double* K9, const int* boxes_xy, const double* rates, double thresh, int min_k,
                              double min_ratio, int threads, double* q_out, double* t_out, double* report, int* used);

/* ---- the candidates as the record the repairing solve consumes, on the device (csrc/correspond.hip) ---------
 * esahrnet_correspondences_cand (correspond_cand_kernel, one wave per crop, k <= 32): esahrnet_correspondences for candidate rows.
 * cand_dev f32 [m][k][M][3] as esahrnet_keypoints_candidates* / _refined write it, M = candidates in 1..ESAHRNET_MAX_CANDIDATES;
 * hess_dev f64 [m][k][M][3], a Hessian or gaussfit's info per candidate (mode 1; may be NULL with mode 0); crop_boxes_dev /
 * rates_dev / valid_dev as esahrnet_boxes wrote them ->
 *     count_dev int32 [m], order_dev int32 [m][k]   what esahrnet_correspondences gives on the candidate-0 rows: the selection is
 *                                  by candidate 0's peak, a NaN primary peak is never selected, -1 beyond count;
 *     cpts_dev  f64 [m][k][M][2]   rank slot i (keypoint order[i]), candidate mm: that candidate's (x, y) in image pixels,
 *                                  p * (1 / rate) + (x_new, y_new) (csrc/correspond.h, the bits the host solvers compute); (NaN,
 *                                  NaN) when either crop coordinate is not finite -- the NaN row of an absent runner-up;
 *     cw_dev    f64 [m][k][M][3]   its weight (wxx, wxy, wyy): mode 0 (peak_mm, 0, peak_mm); mode 1 rate * (-hess[c][j][mm])^(1/2),
 *                                  zeros where esahrnet_correspondences(mode 1) gives zeros; zeros where the coordinates are not
 *                                  finite;
 *     cpeak_dev f32 [m][k][M]      the candidate's peak column, copied.
 * Slot (i, 0) is the primary: cpts[.][.][0] and cw[.][.][0] are the pts and w of esahrnet_correspondences on the candidate-0 rows
 * (with hess[.][.][0]), bit for bit, for finite primaries.  Slots at and beyond count are zero in cpts, cw and cpeak; an invalid
 * crop has count 0.  Every output element is written exactly once; nothing is allocated or synchronised, and the call may be
 * captured into a graph.  Refused before anything is enqueued, in this order: a NULL pointer (hess_dev only with mode 1); m <= 0;
 * k outside 1..32; M outside 1..ESAHRNET_MAX_CANDIDATES; mode outside 0..1; a pointer that is not aligned to its element (4 bytes
 * for f32 and int32, 8 for f64). */
int esahrnet_correspondences_cand(const void* cand_dev, const void* hess_dev, const void* crop_boxes_dev, const void* rates_dev,
                                  const void* valid_dev, int m, int k, int candidates, double thresh, int min_k, int mode,
                                  void* count_dev, void* order_dev, void* cpts_dev, void* cw_dev, void* cpeak_dev,
                                  esahrnet_stream stream);
/* Steps 1-6 of esahrnet_pnp_batch_cand on records esahrnet_correspondences_cand wrote (host copies): image i solves on its first
 * count[i] rank slots, model point kp3d[order[i][j]] for slot j, slot (j, 0) the primary as point and weight.  A runner-up mm >= 1
 * qualifies when its cpts are finite, cpeak[i][j][mm] >= min_ratio * cpeak[i][j][0] and it lies < 5 px from the judge's projection;
 * a swap replaces the point and the weight by those of slot (j, mm).  used = int32 [m][k], indexed by KEYPOINT through order, -1 for
 * a keypoint that was not selected.  On the record of the same candidates, boxes and rates the outputs are those of
 * esahrnet_pnp_batch_cand (mode 0) / esahrnet_pnp_batch_cand_w (mode 1), bit for bit: one body solves all three.  count[i] = 0 (an
 * invalid crop): the NaN pose and a report row of status 1 with n = 0.  Refused: what esahrnet_pnp_batch_cand refuses, then a
 * count outside 0..k or an order entry outside 0..k-1 among the first count, as esahrnet_pnp_batch_w does. */
int esahrnet_pnp_batch_cand_pts(const double* cpts, const double* cw, const float* cpeak, const int* count, const int* order,
                                int m, int k, int candidates, const double* kp3d, const double* K9, double min_ratio, int threads,
                                double* q_out, double* t_out, double* report, int* used);

/* The packed records of the device path after the all-gather of a sharded batch (csrc/records.hip).  A packed record is
 * field-major: field f holds field_bytes[f] bytes per crop, all crops of field 0 first, then field 1, ..., so field f of a
 * record laid out for m crops starts at off_f(m) = m * (field_bytes[0] + ... + field_bytes[f-1]).  gathered_dev: `world`
 * blocks, as all_gather_into_tensor leaves them, each a record laid out for n_max = ceil(n_total / world) crops; rank r's
 * block holds its shard in the first hi_r - lo_r crop slots of every field.  Shard rule: a contiguous split in which the
 * first n_total % world ranks get one crop more — with base = n_total / world and extra = n_total % world,
 * lo_r = r * base + min(r, extra) and hi_r = lo_r + base + (r < extra ? 1 : 0); it is recomputed on the device from world
 * and n_total.  out_dev: the record laid out for n_total crops,
 *     out[off_f(n_total) + i * b_f ... + b_f] = block_r[off_f(n_max) + (i - lo_r) * b_f ... + b_f]   for lo_r <= i < hi_r.
 * One launch of a copy kernel (dword loads and stores), nothing allocated, nothing synchronised, capturable into a graph.
 * Every byte of out_dev is written exactly once; the padding slots of a block and the whole block of a rank without crops
 * are never read (they may be uninitialised).  field_bytes is a HOST array, passed on by value.  Refused before anything is
 * enqueued: world < 1, n_total < 1, nfields outside 1..16, a field that is no positive multiple of 4, a null pointer,
 * gathered_dev or out_dev not 8-byte aligned, a block of more than 2^31 - 1 bytes. */
int esahrnet_gather_records(const void* gathered_dev, int world, int n_total, const int* field_bytes, int nfields,
                            void* out_dev, esahrnet_stream stream);

/* ---- introspection / per-operator entry points (used by the parity tests) ------------- */

/* Algorithmic (direct-convolution) FLOPs of one forward of one crop: 2 * MACs of every conv. */
int esahrnet_flops_per_crop(esahrnet_handle h, int height, int width, double* flops);
/* Number of kernel launches one forward enqueues. */
int esahrnet_launch_count(esahrnet_handle h);
/* One kernel launch of the forward plan, for measurement (bench.py roofline leg). */
typedef struct esahrnet_op_desc {
    char kernel[64];             /* kernel template instance, e.g. "conv_mfma<3,1,16,2>"        */
    char label[96];              /* reference layer it implements, e.g. "stage4.0.branches.3.1.conv2" */
    double flops;                /* algorithmic FLOPs (2*MAC of the direct convolution) for n crops */
    double bytes;                /* compulsory HBM bytes of this launch: inputs + outputs + weights */
} esahrnet_op_desc;
int esahrnet_op_desc_get(esahrnet_handle h, int index, int n, int height, int width,
                         esahrnet_op_desc* out);
/* Same as esahrnet_forward but brackets every launch with hipEvents ON `stream` and returns the
 * per-launch durations in milliseconds (ms_out[esahrnet_launch_count]), with the duration of an
 * empty event bracket on the same stream subtracted.  Synchronises `stream`. */
int esahrnet_forward_timed(esahrnet_handle h, const void* x_dev, int n, int height, int width,
                           void* heat_dev, void* ws_dev, size_t ws_bytes, esahrnet_stream stream,
                           float* ms_out);
/* Names of the intermediate tensors that can be dumped ("stem2", "layer1", "stage3.1", ...). */
int esahrnet_tap_count(esahrnet_handle h);
int esahrnet_tap_name(esahrnet_handle h, int index, char* out, size_t cap);
/* keep != 0: every intermediate tensor gets its own workspace region (no recycling) so that
 * esahrnet_tap_read can be used after a forward; changes esahrnet_workspace_bytes. */
int esahrnet_set_debug_keep(esahrnet_handle h, int keep);
/* After a forward on (n,height,width) with the same workspace: convert intermediate tensor
 * `name` from the internal split-bf16 NHWC layout to f32 NCHW [n][c][th][tw] in out_dev. */
int esahrnet_tap_shape(esahrnet_handle h, const char* name, int height, int width,
                       int* c, int* th, int* tw);
int esahrnet_tap_read(esahrnet_handle h, const char* name, int n, int height, int width,
                      const void* ws_dev, void* out_dev, esahrnet_stream stream);

/* ---- activation range report ---------------------------------------------------------------------------------------------
 * Which precision can a checkpoint afford?  precision 3 (fp16) saturates every stored value at +-65504 and precision 0's error
 * grows with the activation scale; the report shows, tensor by tensor, how far a forward's values are from either.
 *
 * One record per (row, image), 64 bytes.  ESAHRNET_STATS_FIELDS is the one description of its layout (the struct below, the
 * ctypes / numpy forms of the Python binding and the tests all come from it): X(C type, name), in memory order, no holes.
 *   sum_abs                 sum of |x| over the finite values
 *   max_abs, min, max       over the finite values; 0, +inf, -inf when there is none
 *   n_finite, n_nan, n_inf  of the real channels (padding channels are read but never counted)
 *   n_zero                  +0 and -0
 *   n_ge_f16max             finite values with |x| >= 65504.  In an fp16 tensor these are the saturated stores (a genuine
 *                           65504 cannot be told apart from a saturated one); in the other formats, the values fp16 would clamp
 *   n_f16_tiny              non-zero finite values with |x| < 2^-14 (fp16's subnormal range)
 *   reserved                zero
 * The records are bit-reproducible and an image's record does not depend on the batch it is in: a workgroup owns a fixed pixel
 * range of one image, the finish adds an image's partials in index order, and there are no atomics. */
#define ESAHRNET_STATS_RECORD_BYTES 64
#define ESAHRNET_STATS_FIELDS(X) \
    X(double, sum_abs)           \
    X(float, max_abs)            \
    X(float, min)                \
    X(float, max)                \
    X(uint32_t, n_finite)        \
    X(uint32_t, n_nan)           \
    X(uint32_t, n_inf)           \
    X(uint32_t, n_zero)          \
    X(uint32_t, n_ge_f16max)     \
    X(uint32_t, n_f16_tiny)
typedef struct esahrnet_stats_record {
#define ESAHRNET_STATS_X(type, name) type name;
    ESAHRNET_STATS_FIELDS(ESAHRNET_STATS_X)
#undef ESAHRNET_STATS_X
    uint32_t reserved[5];
} esahrnet_stats_record;

/* The rows of a handle's report: every tensor of its plan in plan order, then a last row "heatmaps" (the output in caller
 * memory).  Both queries work on an uncommitted handle and change nothing. */
typedef struct esahrnet_stats_row_desc {
    char name[96];               /* the tap name where the tensor has one, else the label of the op that defines it */
    int def_op;                  /* index of that op (esahrnet_op_desc_get); "heatmaps": the last op */
    int c, h, w;                 /* real channels and extent at this crop size (0, 0, 0 for flat scratch) */
    int fmt;                     /* storage: 0 split bf16, 1 bf16, 2 f32 NHWC, 3 fp16, -1 f32 NCHW (the heat-maps) */
    int scanned;                 /* 0: not read at this shape, the row's records stay all zero: plain f32 scratch without the
                                  * padded-channel layout (CBAM's pooled vectors, channel weights and two-plane maps), the head
                                  * terms in the transposed T layout, and the tensors of the head alternative that does not run */
} esahrnet_stats_row_desc;
int esahrnet_stats_rows(esahrnet_handle h, int* rows);
int esahrnet_stats_row_get(esahrnet_handle h, int row, int n, int height, int width, esahrnet_stats_row_desc* out);
/* The forward with every buffer kept (the plan and the launches of esahrnet_forward under esahrnet_set_debug_keep(h, 1)), then
 * the scan of every scanned row where it lies.  heat_dev: the heat-maps, as esahrnet_forward writes them.  stats_dev:
 * esahrnet_stats_record [rows][n], every byte written.  Nothing is allocated, nothing synchronised; the handle's keep state is
 * left as found.  Refused before the first launch, in esahrnet_forward's order: null argument, not committed, shape,
 * workspace size (esahrnet_forward_stats_workspace_bytes), workspace alignment (256), stats_dev alignment (8). */
int esahrnet_forward_stats_workspace_bytes(esahrnet_handle h, int n, int height, int width, size_t* bytes);
int esahrnet_forward_stats(esahrnet_handle h, const void* x_dev, int n, int height, int width, void* heat_dev, void* ws_dev,
                           size_t ws_bytes, void* stats_dev, esahrnet_stream stream);
/* The scan alone, of one raw tensor t_dev [n][h][w][cp] in format fmt (0..3 as above; real channels 0..c-1), or, fmt == -1,
 * plain f32 [n][c][h][w] (cp ignored): n records into stats_dev.  ws_dev: 8-byte aligned scratch for the partials. */
int esahrnet_tensor_stats_workspace_bytes(int fmt, int n, int c, int cp, int h, int w, size_t* bytes);
int esahrnet_tensor_stats(const void* t_dev, int fmt, int n, int c, int cp, int h, int w, void* ws_dev, size_t ws_bytes,
                          void* stats_dev, esahrnet_stream stream);

/* ---- precision report: the error of a handle against a reference handle, tensor by tensor ---------------------
 * What does a fast precision cost on these weights and these crops?  The same crops go through two handles that differ in
 * nothing but `precision`, every tensor is kept, and a two-operand scan reads tensor A (tested) and tensor B (reference) where
 * the two forwards left them.
 *
 * One record per (row, image), 64 bytes; ESAHRNET_DIFF_FIELDS is the one description of its layout, as ESAHRNET_STATS_FIELDS is
 * of the range report's.  Per element, in f32: d = a - b (one rounding), err = |d|; an element is COMPARED only if a and b are
 * both finite.  A tensor stored as T * 2^-e (fp16 scale exponents) enters as ldexpf(a, e).
 *   sum_abs_err, sum_sq_err   sums of err and err^2 over the compared elements
 *   sum_sq_ref                sum of b^2 over the compared elements
 *   max_abs_err, max_abs_ref, max_abs_test   over the compared elements; 0 when there is none
 *   at                        smallest NHWC index pixel * c + channel among the elements that reach max_abs_err (f32 NCHW
 *                             operands: the flat index inside the image); 0xFFFFFFFF when nothing was compared
 *   n_compared                elements with a and b both finite
 *   n_nonfinite_test, n_nonfinite_ref        elements of A / of B that are not finite
 *   n_class_differs           elements where exactly one side is finite, or the sides are different kinds of non-finite
 *                             (NaN / +inf / -inf)
 *   reserved                  zero
 * Padding channels are read and never counted, whatever they hold.  The records have the determinism of the range report's: a
 * workgroup owns a fixed pixel range of one image, the finish merges an image's partials in index order, no atomics. */
#define ESAHRNET_DIFF_RECORD_BYTES 64
#define ESAHRNET_DIFF_FIELDS(X)   \
    X(double, sum_abs_err)        \
    X(double, sum_sq_err)         \
    X(double, sum_sq_ref)         \
    X(float, max_abs_err)         \
    X(float, max_abs_ref)         \
    X(float, max_abs_test)        \
    X(uint32_t, at)               \
    X(uint32_t, n_compared)       \
    X(uint32_t, n_nonfinite_test) \
    X(uint32_t, n_nonfinite_ref)  \
    X(uint32_t, n_class_differs)
typedef struct esahrnet_diff_record {
#define ESAHRNET_DIFF_X(type, name) type name;
    ESAHRNET_DIFF_FIELDS(ESAHRNET_DIFF_X)
#undef ESAHRNET_DIFF_X
    uint32_t reserved[2];
} esahrnet_diff_record;

/* The scan alone on raw tensors, beside esahrnet_tensor_stats.  a_dev [n][h][w][cp_a] in fmt_a (0 split bf16, 1 bf16, 2 f32
 * NHWC, 3 fp16) against b_dev [n][h][w][cp_b] in fmt_b = 2; or fmt_a = fmt_b = -1: plain f32 [n][c][h][w] on both sides (cp
 * ignored).  Channel padding: a multiple of 8, and at least c.  A enters as ldexpf(a, exponent), |exponent| <= 32.  n records
 * into diff_dev; ws_dev: 8-byte aligned scratch for the partials.  Refused before any launch: null pointers, a format pair
 * outside the five above, c / cp / h / w out of range, the exponent, workspace size, alignment (tensors 16, the rest 8). */
int esahrnet_tensor_diff_workspace_bytes(int fmt_a, int cp_a, int fmt_b, int cp_b, int n, int c, int h, int w, size_t* bytes);
int esahrnet_tensor_diff(const void* a_dev, int fmt_a, int cp_a, const void* b_dev, int fmt_b, int cp_b, int exponent,
                         int n, int c, int h, int w, void* ws_dev, size_t ws_bytes, void* diff_dev, esahrnet_stream stream);

/* Row `row` of h's report (esahrnet_stats_rows(h)) and the row of href's report that holds the same tensor.  The key says what
 * the tensor is: its tap name where it has one, else the name of the convolution whose output it is (with its input-channel
 * slice, where it reads one), "<block>.cbam" / "<module>.fuse.<branch>" for the anonymous results of seg_hrnet3's blocks and of
 * the fuse sums, "heatmaps" for the last row; it does not depend on how the plan merges launches.  Works on uncommitted handles
 * and needs no device. */
typedef struct esahrnet_diff_row_desc {
    char key[96];
    int ref_row;                 /* the row of href with the same key; -1: none, or the key is not unique in either handle */
    int c, h, w;                 /* of h's row, as esahrnet_stats_row_get */
    int fmt, ref_fmt;            /* storage formats (ref_fmt 0 when ref_row < 0) */
    int exponent;                /* h's scale exponent for the row's group, else 0: the tensor is stored times 2^-exponent */
    int compared;                /* 1 only if the key is unique in both handles, the shapes agree, both rows are scanned at this
                                  * shape and the format pair is one esahrnet_tensor_diff serves */
} esahrnet_diff_row_desc;
int esahrnet_diff_row_get(esahrnet_handle h, esahrnet_handle href, int row, int n, int height, int width,
                          esahrnet_diff_row_desc* out);
/* The keep-mode forward of h, then the keep-mode forward of href (each the plan and the launches of esahrnet_forward under
 * esahrnet_set_debug_keep, each in its own part of the one workspace), then the scan of every compared row, the heat-maps last.
 * heat_dev / heat_ref_dev: the two heat-map tensors, f32 [n][K][height][width].  diff_dev: esahrnet_diff_record [rows of h][n],
 * every byte written, uncompared rows all zero.  Nothing is allocated, nothing synchronised; both handles' keep states are left
 * as found.  h == href is allowed: the forward runs once and every error is zero.  Refused before the first launch, in
 * esahrnet_forward's order: null argument, either handle uncommitted, handles on different devices, configurations that differ
 * in anything but `precision` (the message names the first differing field), shape, workspace size, workspace alignment (256),
 * diff_dev alignment (8). */
int esahrnet_forward_diff_workspace_bytes(esahrnet_handle h, esahrnet_handle href, int n, int height, int width, size_t* bytes);
int esahrnet_forward_diff(esahrnet_handle h, esahrnet_handle href, const void* x_dev, int n, int height, int width,
                          void* heat_dev, void* heat_ref_dev, void* ws_dev, size_t ws_bytes, void* diff_dev, esahrnet_stream stream);

/* ---- fp16 scale groups: per-tensor power-of-two scales for precision 3 ---------------------------------------
 * precision 3 holds only inside fp16's range: stores saturate at +-65504, values below 2^-14 lose bits.  With BatchNorm folded,
 * seg_hrnet / seg_hrnet2 is convolution, bias, ReLU, sums and bilinear interpolation, which all commute exactly with a power of
 * two.  So tensor T may be STORED as T * 2^-e: esahrnet_commit gives the next convolution's weights 2^(e_in - e_out) per range
 * of input channels and its bias 2^-e_out, in f32 (exact) before the packers run; conv1 keeps its f32 weights and gets
 * 2^-e(stem1); the output layer gets 2^+e(head3) on its K heat-map input channels.  The forward is the same launches on the same
 * plan and the heat-maps come out at true scale.
 * A scale GROUP is a set of stored tensors that must share one exponent, because one reaches the other, or both enter one sum,
 * without convolution weights in between: a branch stream (its identity residuals, the terms and the results of its fuse sums,
 * the output of layer1.0.downsample), stem1, stem2, each BasicBlock's conv1 output, each non-final link of a fuse-down chain,
 * head0 (the slices of last_layer[0] and the h0 the fused head forms from them in registers), head3.  The groups are derived
 * from the handle's plan, numbered by their first tensor in plan order.  Handles of variant 0 with precision 1 or 3 have them
 * (precision 1: the same plan, for calibration; its exponents must stay zero); every other handle has 0 groups.  The f32 crop
 * and the heat-maps belong to no group (-1, exponent 0).  All of these are host calls that work on an uncommitted handle. */
#define ESAHRNET_SCALE_MAX_RANGES 4
#define ESAHRNET_SCALE_MAX_EXPONENT 32
typedef struct esahrnet_scale_conv {
    int32_t out_group;                           /* group the convolution's output is stored in, -1: none (output_layer.0) */
    int32_t nranges;                             /* ranges of input channels [c0, c1), in channel order, covering 0 .. cin */
    int32_t c0[ESAHRNET_SCALE_MAX_RANGES], c1[ESAHRNET_SCALE_MAX_RANGES];
    int32_t in_group[ESAHRNET_SCALE_MAX_RANGES]; /* group of the tensor a range reads, -1: the f32 crop.  last_layer.0 reads four
                                                    ranges (one per branch), output_layer.0 two (head3, the crop) */
} esahrnet_scale_conv;
int esahrnet_scale_groups(esahrnet_handle h, int* groups);
/* "stream0".."stream3", "stem1", "stem2", "head0", "head3", else the name of the convolution that writes the group's first tensor */
int esahrnet_scale_group_name(esahrnet_handle h, int group, char* out, size_t cap);
int esahrnet_scale_conv_get(esahrnet_handle h, int index, esahrnet_scale_conv* out);   /* index as esahrnet_conv_desc_get */
int esahrnet_scale_row_group(esahrnet_handle h, int row, int* group);                  /* row as esahrnet_stats_row_get; -1: none */
/* exponents int32 [count], count = esahrnet_scale_groups, each in [-32, 32]; all zero after esahrnet_create, and with all zero
 * every byte esahrnet_commit uploads and every launch is what it is without this call.  Refused, with esahrnet_last_error set and
 * nothing changed: a wrong count, an exponent out of range, a non-zero exponent on a handle whose precision is not 3.  A
 * successful set un-commits the handle: call esahrnet_commit again (the weights the host handed over are kept).  A weight the
 * shift pushes out of fp16's range is refused by esahrnet_commit, as without a shift; nothing constrains the exponents by the
 * weights beforehand. */
int esahrnet_set_scale_exponents(esahrnet_handle h, const int32_t* exponents, int count);
int esahrnet_get_scale_exponents(esahrnet_handle h, int32_t* exponents, int count);
/* Test use: convolution `index` as esahrnet_commit would pack it under the current exponents — w f32 [cout][cin][k][k] and b f32
 * [cout], the arrays of esahrnet_set_conv with the shifts applied.  Host only. */
int esahrnet_debug_scaled_conv(esahrnet_handle h, int index, float* w, float* b);
/* esahrnet_forward_stats plus the range of the one fp16-rounded tensor the plan never stores: h0 of the fused head (head_fused_bf
 * rounds and saturates it in registers).  h0_dev: esahrnet_stats_record [n].  Where the fused head runs at the shape, it runs in
 * its range form — the same kernel instantiated a second time, same heat-maps and head3 bit for bit — and a record holds max_abs
 * (= max) over the finite h0 BEFORE the rounding and n_ge_f16max, the values at or above 65504 (+inf included), the other fields
 * zero; per-lane maxima and counts, DPP and LDS inside the workgroup, one plainly stored partial per workgroup, a finish kernel
 * per crop, no atomics: bit-reproducible and independent of the batch like the rows.  Where the materialised head runs, the
 * record is the stored row "head0".  stats_dev is what esahrnet_forward_stats writes.  Variant 0 with precision 1 or 3. */
int esahrnet_forward_stats_h0_workspace_bytes(esahrnet_handle h, int n, int height, int width, size_t* bytes);
int esahrnet_forward_stats_h0(esahrnet_handle h, const void* x_dev, int n, int height, int width, void* heat_dev, void* ws_dev,
                              size_t ws_bytes, void* stats_dev, void* h0_dev, esahrnet_stream stream);
/* Exponents from records (host): records = esahrnet_stats_record [rows][n_total] (host copies; the crops of several batches side
 * by side), h0_records [n_total] or NULL.  Per group, M = the largest finite max_abs over its rows and crops (head0: h0 too); the
 * exponent e puts M * 2^-e into (2^(14 - headroom_bits), 2^(15 - headroom_bits)] — headroom_bits in 0..14, 3 leaves a factor 8
 * to 65504 —, clamped to [-32, 32]; a group whose rows are all zero keeps 0.  Any record with n_nan or n_inf above zero is an
 * error that names its row.  Taken on a precision-1 twin of an fp16 handle (same plan, row for row; bf16 has f32's exponent
 * range, so nothing saturates or underflows there), one pass yields the exponents of the fp16 handle. */
int esahrnet_scale_exponents_from_stats(esahrnet_handle h, const void* records, int rows, int n_total, const void* h0_records,
                                        int headroom_bits, int32_t* exponents, int count);

/* ---- stand-alone operator entries (esahrnet_op_conv .. esahrnet_op_tile_max; csrc/op_abi.hip): test use only, no handle ----
 * Stand-alone convolution on f32 NCHW device tensors through the same MFMA kernels:
 * y = [relu]( conv_{k,stride,pad=(k-1)/2}(x; w) + b [+ res] ).  w,b are HOST pointers
 * (packed and uploaded on the spot; synchronous; test use only). */
int esahrnet_op_conv(const void* x_dev, int n, int cin, int height, int width,
                     const float* w, const float* b, int cout, int k, int stride, int relu,
                     const void* res_dev, void* y_dev, esahrnet_stream stream);
/* y = [relu]( sum_i up_bilinear_align_corners_false(x_i -> (height,width)) ), f32 NCHW. */
int esahrnet_op_fuse(const void* const* xs_dev, const int* hs, const int* ws, int nterms,
                     int n, int c, int height, int width, int relu, void* y_dev,
                     esahrnet_stream stream);
/* The same two operators in the arithmetic of esahrnet_cfg.precision (0: split-bf16, 1: single bf16, 2: bf16x6, 3: fp16): inputs are
 * converted to the internal format, the kernel of that mode runs, the result is converted back to f32. */
int esahrnet_op_conv_ex(const void* x_dev, int n, int cin, int height, int width,
                        const float* w, const float* b, int cout, int k, int stride, int relu,
                        const void* res_dev, void* y_dev, int precision, esahrnet_stream stream);
int esahrnet_op_fuse_ex(const void* const* xs_dev, const int* hs, const int* ws, int nterms,
                        int n, int c, int height, int width, int relu, void* y_dev, int precision,
                        esahrnet_stream stream);
/* One CBAM of seg_hrnet3 (ChannelAttention + SpatialAttention, models/seg_hrnet3.py:32-61, 90-91) in the format of `precision`:
 * y[:, c0 : c0 + C'] = [relu]( sa(ca*x) * ca*x [+ res] ), C' = c padded to the mode's channel multiple (32; bf16: 64), the
 * padding written as zeros.  x_dev / res_dev: f32 NCHW [n][c][height][width] (res_dev may be NULL); w_fc0 [c/16][c],
 * w_fc2 [c][c/16], w_sa [2][7][7]: host f32.  y_dev: f32 NCHW [n][cy][height][width], read (converted to the internal
 * format) and written back whole: channels outside the slice come back as they went in (exactly, if the format holds them
 * exactly).  c0 a multiple of 8, c0 + C' <= cy padded.  fused: 1 = maps and attention in one pass (cbam_spatial; c padded / 8
 * must be a power of two <= 32), 0 = cbam_maps + cbam_apply. */
int esahrnet_op_cbam(const void* x_dev, const void* res_dev, int n, int c, int height, int width, const float* w_fc0,
                     const float* w_fc2, const float* w_sa, int relu, void* y_dev, int cy, int c0, int fused, int precision,
                     esahrnet_stream stream);
/* esahrnet_op_cbam with its steps shown (esahrnet_op_cbam is this call with slabs = 0 and the three outputs NULL): the same
 * launches, and afterwards the buffers the steps left, copied to optional DEVICE outputs.
 *   slabs        0: the plan's rule P = min(64, height * width); otherwise P itself, 1 <= P <= min(1024, height * width) —
 *                pool_partial and ca_mlp at the slab counts the pooling stem produces.  Slab s of an image holds the pixels
 *                [s * S, min(HW, s * S + S)), S = ceil(HW / P), in row-major order; a slab past the last pixel holds (0, -inf).
 *   partial_out  f32 [n][P][C'][2]: (sum, max) of every channel over every slab (pool_partial)
 *   ca_out       f32 [n][C']: the channel attention (ca_mlp), zero in the padding channels
 *   maps_out     f32 [n][height][width][2]: (mean, max) over the c real channels of ca * x (cbam_maps); with fused = 1 the maps
 *                never leave the workgroup, and passing maps_out is refused.
 * C' = c padded (32; bf16: 64) and at most 512 (ca_mlp's limit).  Every argument is checked before anything is enqueued.
 * Synchronous; test use only. */
int esahrnet_op_cbam_steps(const void* x_dev, const void* res_dev, int n, int c, int height, int width, const float* w_fc0,
                           const float* w_fc2, const float* w_sa, int relu, void* y_dev, int cy, int c0, int fused, int precision,
                           int slabs, void* partial_out, void* ca_out, void* maps_out, esahrnet_stream stream);
/* conv1 of the stem on its own, cin = 1 and cout = 64: y = [relu]( conv3x3_pad1(x; w) + b ) in the format of `precision`
 * (0, 1 or 2), converted back exactly to f32 NCHW.  x_dev: f32 [n][1][height][width]; w [64][1][3][3] and b [64]: host f32,
 * packed as esahrnet_commit packs conv1; y_dev: f32 [n][64][height][width].  pooled = 0: launch_stem.  pooled = 1:
 * launch_stem_pool, which also leaves the per-channel (sum, max) of its output over slabs of pixels: partial_out (device) f32
 * [n][slabs][64][2] and *slabs_out = height * ceil(width / 256), both required then.  Slab `row * pieces + piece`, pieces =
 * ceil(width / 256), holds the pixels [256 * piece, min(width, 256 * piece + 256)) of that row; in the bf16 format the partials
 * are those of the rounded values y holds.  Checked before anything is enqueued; synchronous; test use only. */
int esahrnet_op_stem(const void* x_dev, int n, int height, int width, const float* w, const float* b, int relu, int pooled,
                     int precision, void* y_dev, void* partial_out, int* slabs_out, esahrnet_stream stream);
/* resample_slice on its own, in the format of `precision` (0, 1 or 2; 3 is refused: the kernel does not serve fp16):
 * y[:, c0 : c0 + c] = bilinear(x -> (height, width)) under F.interpolate's rule for align (0: align_corners=False, 1: True);
 * h == height and w == width is the copy path.  x_dev: f32 NCHW [n][c][h][w]; y_dev: f32 NCHW [n][cy][height][width], read
 * and written back whole as esahrnet_op_cbam does: channels outside the slice come back as they went in.  The kernel writes
 * whole 8-channel groups: with c not a multiple of 8 the channels c0 + c .. c0 + 8*ceil(c/8) - 1 of y receive the source's
 * channel padding (zeros).  c0 a multiple of 8, c0 + 8*ceil(c/8) <= cy padded (32; bf16: 64); checked before anything is
 * enqueued.  Synchronous; test use only. */
int esahrnet_op_resample(const void* x_dev, int n, int c, int h, int w, void* y_dev, int cy, int c0, int height, int width,
                         int align, int precision, esahrnet_stream stream);
/* zero_slice on its own, the same round trip of y_dev (f32 NCHW [n][cy][height][width]): y[:, c0 : c0 + nchan] = +0, the
 * rest comes back as it went in.  c0 and nchan multiples of 8, c0 + nchan <= cy padded; precision 0, 1 or 2. */
int esahrnet_op_zero_slice(void* y_dev, int n, int cy, int height, int width, int c0, int nchan, int precision,
                           esahrnet_stream stream);

/* ---- every convolution launcher on its own (test use only; none of these is on a forward path) --------------------------
 * All are synchronous, check every argument before anything is enqueued (a refusal returns non-zero with esahrnet_last_error
 * set, launches nothing and leaves the outputs as they were), take w / b as HOST f32 pointers and pack them on the spot, and
 * take `precision` as esahrnet_op_conv_ex does (0: split-bf16, 1: bf16, 2: bf16x6, 3: fp16).  Outputs are f32 NCHW with
 * C' = cout padded to the mode's channel multiple (32; bf16 / fp16: 64) channels: the padding channels come back too. */
/* Name of the kernel esahrnet_op_conv_ex / esahrnet_op_conv_group(count = 1) runs for these parameters ("none": no kernel of
 * the precision serves them).  Host only: no device call is made. */
int esahrnet_op_conv_kernel(int n, int cin, int cout, int height, int width, int k, int stride, int has_res, int precision,
                            char* out, size_t cap);
/* `count` convolutions of one kernel size, stride and precision, member j on its own tensors: x [ns[j]][cins[j]][heights[j]]
 * [widths[j]] -> y [ns[j]][C'][oh][ow], y = [relu]( conv(x; w) + b [+ res] ); res_dev may be NULL, or hold NULL for a member
 * without residual.  count == 1: launch_conv of the member (esahrnet_op_conv_ex with the padded output).  count 2 .. 6: ONE
 * merged launch under the rule the plan applies to an HRModule's job groups — launch_conv_x6_jobs (precision 2),
 * launch_conv1x1_jobs (k = 1) or launch_conv_jobs (k = 3; a stride-1 member must be a stream-kernel launch on its own);
 * a group that rule rejects is refused.  kernel_out (optional): the kernel's name as esahrnet_op_desc_get reports it. */
int esahrnet_op_conv_group(int count, const void* const* xs_dev, const int* ns, const int* cins, const int* heights, const int* widths,
                           const float* const* ws, const float* const* bs, const int* couts, int k, int stride, const int* relus,
                           const void* const* res_dev, void* const* ys_dev, int precision, char* kernel_out, size_t kernel_cap,
                           esahrnet_stream stream);
/* launch_conv_s2c32_multi: 2 or 3 3x3 stride-2 convolutions of ONE input in one launch (split-bf16 only), head h with couts[h]
 * (a multiple of 32) output channels, its own ReLU flag and its own output ys_dev[h] f32 [n][couts[h]][oh][ow]. */
int esahrnet_op_conv_multi(const void* x_dev, int n, int cin, int height, int width, int nheads, const float* const* ws,
                           const float* const* bs, const int* couts, const int* relus, void* const* ys_dev, esahrnet_stream stream);
/* launch_bblock32 (split-bf16): y = relu( conv3x3(relu(conv3x3(x; w1) + b1); w2) + b2 + x ), x and y f32 [n][32][height][width],
 * w1 / w2 [32][32][3][3], b1 / b2 [32]. */
int esahrnet_op_block32(const void* x_dev, int n, int height, int width, const float* w1, const float* b1, const float* w2,
                        const float* b2, void* y_dev, esahrnet_stream stream);
/* The fused stem: y = relu( conv3x3_s2( relu(conv3x3(x; w1) + b1); w2 ) + b2 ), x f32 [n][cin][height][width], w1 [cmid][cin][3][3],
 * w2 [cout][cmid][3][3], y f32 [n][C'][ceil(height/2)][ceil(width/2)].  precision 0: launch_stem_fused (cin 1 .. 4, cmid a
 * multiple of 32); precision 2: launch_stem_fused_x6 where stem_fused_x6_supported (cin 1, cmid 64, C' a multiple of 64).
 * Weights are packed as esahrnet_commit packs them. */
int esahrnet_op_stem2(const void* x_dev, int n, int cin, int height, int width, const float* w1, const float* b1, int cmid,
                      const float* w2, const float* b2, int cout, int precision, void* y_dev, esahrnet_stream stream);

/* ---- the stem, the layout conversions and the tile-maximum kernels on their own (test use only; none of these is on a
 * forward path) ------------------------------------------------------------------------------------------------------------
 * All are synchronous and check every argument before anything is allocated or enqueued: a refusal returns non-zero with
 * esahrnet_last_error set and leaves the outputs as they were.  `precision` as above (0: split-bf16, 1: bf16, 2: f32, 3: fp16). */
/* conv1 of a stem through launch_stem, any cin 1 .. 4 and any cout the launcher takes (a multiple of 32; of 64 in the two
 * 16-bit formats): y = [relu]( conv3x3_pad1(x; w) + b ) in the format of `precision`, converted back exactly to f32 NCHW.
 * x_dev f32 [n][cin][height][width]; w [cout][cin][3][3] and b [cout]: host f32, packed by the function esahrnet_commit packs
 * conv1 with; y_dev f32 [n][cout][height][width].  cin == 1 runs stem1_kernel / stem1_hf_kernel, cin 2 .. 4 stem_kernel. */
int esahrnet_op_stem_ex(const void* x_dev, int n, int cin, int height, int width, const float* w, const float* b, int cout,
                        int relu, int precision, void* y_dev, esahrnet_stream stream);
/* The conversions of layout.hip.  raw_dev: the tensor [n][height][width][cp] in the format of `precision`, n * height * width *
 * cp * (2 in the 16-bit formats, else 4) bytes the caller owns, 16-byte aligned; c <= cp, cp a multiple of 8.
 * dir 0: launch_nchw_to_fmt from x_dev (f32 [n][c][height][width]) into raw_dev — every byte of it is written, the channels
 * c .. cp-1 as +0 —, then launch_fmt_to_nchw from raw_dev into y_dev (f32 [n][c][height][width]).  dir 1: only the second
 * step, on the bytes raw_dev holds (x_dev is not used). */
int esahrnet_op_layout(int dir, const void* x_dev, int n, int c, int height, int width, int cp, int precision, void* raw_dev,
                       void* y_dev, esahrnet_stream stream);
/* The tile maxima of heat-maps raw_dev [n][height][width][cp] (precision 0: split-bf16, 2: f32; c <= 32, c <= cp, cp a multiple
 * of 8): part_dev 8 bytes x [n * c][ntiles] (f32 value, int32 index row * width + column) — each tile of 256 row-major pixels'
 * first maximum, a NaN counting as the largest —, *ntiles_out = ceil(height * width / 256).  store 1: launch_to_nchw_part, which
 * also writes y_dev f32 [n][c][height][width]; store 0: launch_tile_max, y_dev is not touched and may be NULL.  kp_dev not NULL:
 * launch_keypoints_finish_nhwc over the same part, kp_dev f32 [n][c][3] and idx_dev int32 [n][c] (may be NULL). */
int esahrnet_op_tile_max(const void* raw_dev, int n, int c, int height, int width, int cp, int precision, int store, void* y_dev,
                         void* part_dev, int* ntiles_out, void* kp_dev, void* idx_dev, esahrnet_stream stream);

/* ---- test hooks ------------------------------------------------------------------------------------ */
/* Launch state is kept per DEVICE (dynamic-LDS limits raised per kernel and device, CU counts), never in
 * process-wide flags: number of (kernel, device) entries and of devices seen so far. */
int esahrnet_debug_devstate(int* kernel_device_entries, int* devices);
/* Bytes one launch of the stream convolution kernels may address (default and maximum 2^31 - 1); batches beyond it
 * are cut into image ranges on the host.  Lowered by the tests to exercise the cut at small sizes; 0 restores. */
int esahrnet_debug_set_launch_limit(long long bytes);
/* Workgroups one launch of the fp32-grade tile-stream convolution kernels may have (each member of a merged launch on its
 * own; default: two per CU).  Lowered by the tests so that a workgroup walks many items of a small tensor — the launcher
 * still rounds a grid above the number of cout slices down to a multiple of it.  workgroups <= 0 restores. */
int esahrnet_debug_set_x6_grid_limit(int workgroups);
/* An upper limit on the CU count the launchers size with (device_cus() reports min(the device's, cus)); cus <= 0 restores.
 * With a limit of 1 .. 3 a small tensor gets the launch forms of a large batch: persistent workgroups that walk many items
 * across cout slices and image boundaries (the tile and stream convolution kernels, bblock32), the single-buffered stream
 * variant, the two-groups-per-wave 1x1 kernel of the 16-bit formats, fewer cout splits of the 1x1 kernels.  Every use of the
 * count is sizing — a grid, a slice count, the choice between variants of one kernel — never an address, so every value is
 * a valid launch and the results must not depend on it.  The fp32-grade tile-stream kernels keep their own hook above
 * (both limits apply).  Process-wide; test use only. */
int esahrnet_debug_set_cu_limit(int cus);
/* Where launch `index` (0 .. esahrnet_launch_count-1) sits in the wave schedule: launches of one wave on different
 * lanes run concurrently (lane 0 = the caller's stream), waves one after another.  All zero on a one-lane handle. */
int esahrnet_debug_op_schedule(esahrnet_handle h, int index, int* wave, int* lane);
/* The workspace plan of a forward of (n, height, width), op by op, for a host check of the recycling (no device call: the
 * plan is made on the host, as for esahrnet_workspace_bytes; follows esahrnet_set_debug_keep).  esahrnet_debug_op_count:
 * the plan ops that run at that shape (the head alternative the shape does not take is left out), in launch order.
 * esahrnet_debug_op_regions: op `k` of those — its index in the plan (esahrnet_debug_op_schedule's), wave and lane, the job
 * group and multi-head group it is launched with AT THIS SHAPE (-1: a launch of its own; the members of a group are one
 * launch, made at its first member), and every workspace tensor it touches: tensor id, role (0 in, 1 res, 2..5 terms[0..3],
 * 6 out, 7 out2), write (roles 6, 7), slice (the output of an op kind that writes at a channel offset into an allocation
 * other ops may fill too: resample_slice, zero_slice, every CBAM apply), byte offset in the workspace and byte length as the
 * planner reserved it.  This is the plan as the allocator sees it: an op that launches nothing of its own at the shape (the
 * CBAM maps formed inside cbam_spatial, a group member) is reported with the tensors the plan gives it. */
#define ESAHRNET_DEBUG_MAX_REGIONS 8
typedef struct esahrnet_debug_region {
    int32_t tensor, role, write, slice;
    uint64_t offset, bytes;
} esahrnet_debug_region;
typedef struct esahrnet_debug_op {
    int32_t index, wave, lane, job, multi, nregions;
    esahrnet_debug_region regions[ESAHRNET_DEBUG_MAX_REGIONS];
} esahrnet_debug_op;
int esahrnet_debug_op_count(esahrnet_handle h, int n, int height, int width, int* count);
int esahrnet_debug_op_regions(esahrnet_handle h, int n, int height, int width, int k, esahrnet_debug_op* out);

#ifdef __cplusplus
}
#endif
#endif /* ESAHRNET_H */
