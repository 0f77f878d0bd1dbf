/*
 * d2fe.h -- C ABI of libd2fe_hip.so: the MI355X (gfx950) implementation of D2SLAM's d2frontend
 * feature hot path (SuperPoint extraction, NetVLAD global descriptor, brute-force descriptor matching).
 *
 * Every entry point below replaces one call the reference makes into TensorRT / ONNX Runtime / OpenCV;
 * the reference interface it stands in for is cited as file:line relative to the D2SLAM tree.
 * Conventions: plain pointers and sizes only; caller owns every buffer; nothing is retained past return;
 * functions return 0 (D2FE_OK) or a negative d2fe_status and never throw; d2fe_last_error() describes the
 * last failure on the calling thread.  Pointers are HOST pointers unless the parameter name starts with d_.
 */
#ifndef D2FE_H_
#define D2FE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define D2FE_API __attribute__((visibility("default")))
#else
#define D2FE_API
#endif

typedef struct d2fe_context* d2fe_handle;

typedef enum {
  D2FE_OK = 0,
  D2FE_ERR_INVALID = -1,     /* bad argument / size mismatch (reference: assert, superpoint_onnx.cpp:74-75) */
  D2FE_ERR_HIP = -2,         /* HIP runtime failure (reference: infer() returns false, superpoint_tensorrt.cpp:164-170) */
  D2FE_ERR_NOT_READY = -3,   /* weights not loaded */
  D2FE_ERR_TRUNCATED = -4,   /* output capacity too small; n_out holds what was written */
  D2FE_ERR_UNSUPPORTED = -5
} d2fe_status;

/* Post-processing variant. B is the live USE_CUDA path of the reference. */
typedef enum {
  D2FE_POSTPROC_B = 0, /* SuperPoint::processOutput, superpoint_tensorrt.cpp:327-350: threshold, borders, top-K */
  D2FE_POSTPROC_A = 1  /* SuperPointONNX: getKeyPoints + NMS2 + grid_sampler, superpoint_common.cpp:12-177 */
} d2fe_postproc;

typedef enum {
  D2FE_PREC_F32 = 0,   /* exact fp32 MFMA (v_mfma_f32_32x32x2_f32): bitwise equal to the oracle's fmaf chains */
  D2FE_PREC_F16X2 = 1, /* fp16 hi/lo split operands, 3 x v_mfma_f32_32x32x16_f16, fp32 accumulate (~2^-22 rel.).  The arithmetic of every layer from
                            conv1b on (conv1a stays the exact fp32 chain, fused into conv1b's staging), with SA = 4, SW = 8:
                              activation  xs = min(max(x * 2^SA, -65000), 65000) in fp32 (the scaling is exact; behind the fused conv1a only the upper
                                          clamp exists, its input being a ReLU output), hi_x = fp16(xs) round to nearest even, lo_x = fp16(xs - hi_x): the
                                          residual is exact in fp32 and its conversion rounds to nearest even, so hi_x + lo_x = xs whenever the residual is an fp16
                                          number; otherwise |xs - hi_x - lo_x| <= max(2^-22 |xs|, 2^-25): half a unit of lo_x, which is 2^-11 of a
                                          residual of at most 2^-11 |xs| while lo_x is normal, and half the subnormal spacing 2^-24 below that
                              weight      ws = min(max(w * 2^SW, -65000), 65000), hi_w, lo_w likewise, once, when the weights are loaded
                              sum         acc = bias * 2^(SA+SW) + sum over (ky, kx, ci) of (lo_x hi_w + hi_x lo_w + hi_x hi_w): THREE products per operand
                                          pair, each exact, accumulated in fp32 inside the matrix instruction (the order is the instruction's: no bit-exact
                                          restatement is promised); lo_x lo_w is DROPPED (<= 2^-22 relative to the product)
                              epilogue    y = acc * 2^-(SA+SW) (exact), then ReLU and the 2x2 max-pool as in every mode
                            fp16 subnormals are kept on hi and lo (nothing is flushed by the conversions or by the matrix instruction); zero padding is
                            exact.  The error of one layer against real arithmetic on the split operands is bounded by the fp32 summation bound
                            (3 K + 2) * 2^-24 * (sum (|hi hi| + |hi lo| + |lo hi|) * 2^-(SA+SW) + |bias|), K = 9 Cin (Cin for the 1x1 heads). */
  D2FE_PREC_F32_WINO = 2,/* fp32 throughout; the eight 3x3 layers with Cin >= 64 as Winograd F(2x2,3x3) on v_mfma_f32_32x32x2_f32
                            (16 instead of 36 multiplies per output and channel pair).  Bitwise equal to the oracle's restatement
                            of that evaluation order (orc_conv3x3_wino), ~1e-6 relative to the direct chains of D2FE_PREC_F32.
                            Keypoint lists are index-exact against THAT evaluation order only: scores closer than the deviation can swap list
                            positions, or cross the threshold or the K-th score.  d2fe_config::exact_order (variant B, max_keypoints >= 1) removes
                            that: count, kps_idx, kps_xy and the list order then equal D2FE_PREC_F32's position by position, PROVIDED
                            exact_order_eps bounds |Winograd score - direct score| and d2fe_exact_order_stats reports no dropped cell.  It does NOT
                            cover the descriptors (they stay the Winograd trunk's, <= 1e-5 from exact; matches whose near-ties follow from
                            descriptor bits may differ), the scores of keypoints outside re-evaluated cells (Winograd bits), variant A,
                            D2FE_PREC_F16X2, D2FE_PREC_F16 or keep-all handles. */
  D2FE_PREC_F16 = 3      /* fp16 OPERANDS, fp32 accumulation: the operand precision the reference's engine may run at (kFP16,
                            superpoint_tensorrt.cpp:118-122), one v_mfma_f32_32x32x16_f16 per k-step where D2FE_PREC_F16X2 spends three.
                            Activations between the layers stay fp32 NHWC in memory.  The arithmetic of every layer that D2FE_PREC_F16X2 evaluates
                            in split form (conv1b .. conv4b, convPa | convDa, the 1x1 heads convPb and -- dense head only -- convDb), with SA = 4, SW = 8:
                              activation  x^ = fp16(min(max(x * 2^SA, -65000), 65000))   round to nearest even; the inputs are ReLU outputs, so only the
                                                                                         upper clamp can act (x >= 4062.5)
                              weight      w^ = fp16(min(max(w * 2^SW, -65000), 65000))   round to nearest even, once, when the weights are loaded
                              sum         acc = sum over (ky, kx, ci) of x^ * w^         products exact, accumulated in fp32 inside the matrix instruction
                                                                                         (the order is the instruction's: no bit-exact restatement is promised)
                              epilogue    y = acc * 2^-(SA+SW) + bias                    the scaling is exact, the bias is the fp32 bias: ONE rounding;
                                                                                         then ReLU and the 2x2 max-pool as in every mode
                            fp16 subnormals are KEPT on both operands (gradual underflow: |x * 2^SA| or |w * 2^SW| below 2^-14 keeps fewer than 11
                            bits, down to the spacing 2^-24; nothing is flushed to zero by the conversion or by the matrix instruction); zero padding is
                            exact.  The error of one layer against real arithmetic on the ROUNDED operands is bounded by the fp32 summation bound
                            (9 Cin + 2) * 2^-24 * (sum |x^ w^| * 2^-(SA+SW) + |bias|); the operand rounding itself is 2^-11 relative per operand.
                            What D2FE_PREC_F16X2 keeps in fp32 stays fp32: conv1a (fused into conv1b's staging, bit-equal to the exact mode),
                            the sparse descriptor head (convDa, convDb at the keypoints' cells: exact fp32 chains), softmax, selection, sampling.
                            Handles of this mode take the sparse descriptor head for every call (the dense head would evaluate convDa | convDb with
                            fp16 operands: only dense_descriptors handles and calls with a capacity beyond 4 x min(max_keypoints, 1024) cells do), so
                            a frame's outputs do not depend on the entry point, the batch it travels in or the pipe that carries it.
                            Not available with exact_order. */
} d2fe_precision;

/* One more value of d2fe_config.precision (an int32_t), declared beside d2fe_precision in an enumeration of its own: the four enumerators above are pinned as
 * the whole of d2fe_precision.  4 is unassigned and refused. */
typedef enum {
  D2FE_PREC_I8 = 5       /* int8 OPERANDS, int32 accumulation (v_mfma_i32_32x32x32_i8): the precision of the reference's real-time configuration
                            (cnn_enable_tensorrt_int8, d435_multi_rt.yaml:119-122).  Activations between the layers stay fp32 NHWC in memory.  The
                            quantised layers are the ones D2FE_PREC_F16 evaluates with fp16 operands (conv1b .. conv4b, convPa, and convPa | convDa in
                            the dense head, the 1x1 heads convPb and -- dense head only -- convDb).  With T the dynamic range of the layer's INPUT tensor
                            (d2fe_set_superpoint_int8_ranges) and c the output channel:
                              r        = fl32(127 / T)                                   host, once
                              s_x      = fl32(T / 127)                                   host, once
                              amax_c   = max |w[c, :, :, :]|                             host, at load
                              q_w      = clamp(rint((double)w * 127.0 / (double)amax_c), -127, 127)     round half to even, once at load;
                                                                                         amax_c == 0: q_w = 0 and s_w[c] = 1
                              s_w[c]   = fl32(amax_c / 127)
                              d_c      = fl32(s_x * s_w[c])                              fp32 product, host
                              q_x      = (int8) rintf(fminf(fmaxf(x * r, -127.f), 127.f))  fp32 product, round half to even; +inf -> 127; the zero
                                                                                         padding is q = 0; never -128
                              acc      = sum over (ky, kx, ci) of q_x * q_w              int32, EXACT and independent of the summation order;
                                                                                         |acc| <= 1152 * 127^2 < 2^31
                              y        = fl32(fl32((float)acc * d_c) + bias[c])          TWO roundings, not a fused multiply-add; (float)acc rounds to
                                                                                         nearest even; then ReLU and the 2x2 max-pool as in every mode
                            A layer therefore has exactly one correct answer, and tests/helpers/i8_oracle.py restates it in numpy bit for bit.  NaN
                            activations are outside the contract.  What D2FE_PREC_F16 keeps in fp32 stays fp32: conv1a (fused into conv1b's staging,
                            bit-equal to the exact mode, quantised with conv1b's r on its way into LDS), the sparse descriptor head, softmax, selection,
                            sampling and the PCA tail.  As with D2FE_PREC_F16, handles of this mode take the sparse descriptor head for every call
                            (exceptions: dense_descriptors handles, and capacities beyond 4 x min(max_keypoints, 1024) cells), so a frame's bits do not
                            depend on entry point, batch or pipe.  Until the ranges are set every extract call and pipe create answers
                            D2FE_ERR_NOT_READY.  Not available with exact_order. */
} d2fe_precision_i8;

/* Mirrors SuperPointConfig (d2frontend/include/d2frontend/CNN/superpoint_tensorrt.h:17-33) plus the
 * SuperPointONNX ctor arguments (superpoint_onnx.h:17-21) and the device/batch geometry. */
typedef struct {
  int32_t struct_size;        /* sizeof(d2fe_config), for forward compatibility */
  int32_t device_id;          /* HIP device ordinal */
  int32_t max_width;          /* largest input width (>= 16)   -- SuperPointConfig::input_width  */
  int32_t max_height;         /* largest input height (>= 16)  -- SuperPointConfig::input_height */
  int32_t max_batch;          /* images per batched call (>= 1) */
  int32_t max_keypoints;      /* SuperPointConfig::max_keypoints: 1..16384 (sorted top-K), or -1 = keep every keypoint above the threshold in raster
                                 order like topKeypoints with k == -1 (superpoint_tensorrt.cpp:241-253)  [params->max_superpoint_cnt].
                                 Keep-all with MORE keypoints in an image than the call's capacity: D2FE_ERR_TRUNCATED, and the first
                                 `capacity` of them in raster order are returned (the reference's list, cut where the buffers end) */
  int32_t remove_borders;     /* SuperPointConfig::remove_borders (variant B), default 1.  With 0, keypoints of the last row and column carry the reference's NaN
                                 descriptors: their four clipped sampling weights are 0 (superpoint_tensorrt.cpp:255-317) */
  float   keypoint_threshold; /* SuperPointConfig::keypoint_threshold, default 0.015 */
  int32_t postproc;           /* d2fe_postproc */
  int32_t nms_dist;           /* variant A: NMS2 dist_thresh (SuperPointONNX::nms_dist) */
  int32_t precision;          /* d2fe_precision */
  int32_t keep_score_map;     /* 1: also write the dense H x W score map ("semi", 1.2 MB/image; read back by the development library's d2fe_debug_read);
                                 variant B does not need it (candidates are emitted by the softmax kernel) */
  int32_t dense_descriptors;  /* 0 (default): the descriptor head is evaluated (convDa, convDb) only at the corner cells of the
                                 selected keypoints when a call carries >= 4 images (below that the dense head is quicker; both give identical bits) -- 5 % fewer
                                 FLOPs; 1: always the dense descriptor map (d2fe_debug_read
                                 "desc_raw" / "convPaDa" need it). */
  int32_t async_tail;         /* 1: d2fe_superpoint_extract_device issues the convolutions on the caller's stream and the post-processing
                                 (softmax .. descriptors) on the handle's tail stream (d2fe_tail_stream), so that it runs UNDER the
                                 convolutions of the next call; outputs are complete on the tail stream -- enqueue consumers there, or
                                 call d2fe_superpoint_wait_tail(h, stream).  Host-pointer calls are unaffected.  Default 0. */
  int32_t variant_b_pca;      /* 1 (variant B only; on a variant-A handle D2FE_ERR_INVALID at create: A needs no opt-in): d2fe_set_superpoint_pca is accepted and the
                                 sampled descriptors go through variant A's PCA tail (the projection the reference's variant B loads and never applies,
                                 superpoint_tensorrt.cpp:400-448): every extract call, pipe, list, store and exchange of the handle then carries
                                 rows of pca_dims floats.  Works with every precision, exact_order, keep-all, the dense and the sparse descriptor head and
                                 async_tail.  0 (default): variant B refuses a PCA with D2FE_ERR_UNSUPPORTED, as the reference's live path ignores it.
                                 The field takes the first of the five ints that were reserved (zero in every struct d2fe_default_config has filled): the struct
                                 keeps its size, so a program compiled against an earlier header -- whose d2fe_config d2fe_default_config fills -- runs unchanged. */
  int32_t reserved[4];
  /* -- appended fields: a caller that passes the struct_size of the struct above (up to and including `reserved`) gets zeros here -- */
  int32_t exact_order;        /* 1 (D2FE_PREC_F32_WINO, variant B, max_keypoints >= 1 only; anything else: D2FE_ERR_INVALID): the keypoint list equals the
                                 one a D2FE_PREC_F32 handle produces.  Candidates whose list position the Winograd deviation could change (within
                                 exact_order_eps of the threshold, unless more than max_keypoints candidates lie clear above it; within 2 eps of a
                                 neighbour in the part of the sorted list that can reach the top K)
                                 have their 8x8 cell re-evaluated with the direct fmaf chains on an 88x88 crop of the frame; the selection then runs on the
                                 patched list.  Images must be at least 88x88 with both sizes multiples of 8.  Default 0: nothing changes. */
  float   exact_order_eps;    /* bound on |Winograd score - direct score|; 0 = the library default 9e-6 = 4 x the largest deviation measured (2.03e-6 over 1056 images at two thresholds, seeded weights).  Negative, NaN or infinite: D2FE_ERR_INVALID */
  int32_t exact_order_crops;  /* crop slots per call (one per re-evaluated cell; granted in image order, within an image in sorted-list order; a cell
                                 without a slot keeps its Winograd scores and is counted as dropped); 0 = max(66.5 * max_batch, 136): no drop in the 1056-image study.  EVERY slot
                                 runs through the direct kernels in every call (1.7 MB of activations each): a smaller count is cheaper, and
                                 d2fe_exact_order_stats tells whether it was enough */
} d2fe_config;

/* One conv layer in PyTorch layout: weight [cout][cin][k][k], bias [cout]. */
typedef struct {
  const float* weight;
  const float* bias;
  int32_t cout, cin, ksize;
} d2fe_conv_params;

/* The 12 SuperPoint layers in the order of d2frontend/superpoint.ipynb:306-321:
 * conv1a conv1b conv2a conv2b conv3a conv3b conv4a conv4b convPa convPb convDa convDb */
#define D2FE_SP_NUM_LAYERS 12
typedef struct {
  d2fe_conv_params layer[D2FE_SP_NUM_LAYERS];
} d2fe_superpoint_weights;

D2FE_API const char* d2fe_last_error(void);
D2FE_API const char* d2fe_version(void);
D2FE_API void d2fe_default_config(d2fe_config* cfg);

/* Lifecycle.  Replaces: LoopCam ctor building the networks (loop_cam.cpp:24-70),
 * SuperPoint::SuperPoint + SuperPoint::build (superpoint_tensorrt.cpp:17-107). */
D2FE_API int d2fe_create(const d2fe_config* cfg, d2fe_handle* out);
D2FE_API void d2fe_destroy(d2fe_handle h);
/* Replaces the ONNX parse / engine deserialisation (superpoint_tensorrt.cpp:109-125,376-398):
 * weights are copied, re-packed into MFMA fragment order and cached on the device. */
D2FE_API int d2fe_load_superpoint(d2fe_handle h, const d2fe_superpoint_weights* w);

/* Optional PCA of the local descriptors: variant A as in the reference (computeDescriptors, superpoint_common.cpp:76-85); variant B only on a
 * handle created with d2fe_config.variant_b_pca = 1 (the reference's variant-B path loads the matrices and never applies them, SURVEY.md F6:
 * without the opt-in a variant-B handle answers D2FE_ERR_UNSUPPORTED).  Both variants share one tail: t = d - mean, a[j] = the fp32 chain over
 * c = 0..255 ascending of t[c] * comp[j][c] from 0 (each product and sum rounded), out[j] = a[j] / sqrtf(sum a[j]^2); no guards -- a NaN row
 * (remove_borders = 0) or d == mean gives NaN in every component.  A keypoint's bits do not depend on batch, entry point or pipe shape.
 * comp: [pca_dims][256] row-major (the CSV layout read by superpoint_onnx.cpp:47-53), mean: [256].
 * pca_dims = 0 disables; variant A takes 1..256, variant B 4..256 in multiples of 4 (the matcher's row alignment; anything else D2FE_ERR_INVALID).
 * d2fe_desc_dim() returns the per-keypoint descriptor length of extract calls (256 or pca_dims).  Refused while pipes are alive. */
D2FE_API int d2fe_set_superpoint_pca(d2fe_handle h, const float* comp, const float* mean, int pca_dims);
D2FE_API int d2fe_desc_dim(d2fe_handle h);

/* D2FE_PREC_I8: the calibration ranges (per-tensor thresholds, what a calibration table holds).  n = D2FE_SP_NUM_LAYERS; range[i] is the dynamic range of
 * the OUTPUT tensor of layer i in the order of d2fe_superpoint_weights (conv1a .. convDb).  A quantised layer uses the range of the tensor it reads: convPa
 * and convDa both read conv4b's; the entries of convPb and convDb are ignored.  Every used entry must be finite and lie in [1e-30, 1e30] (r and s_x are
 * then finite normal fp32), else D2FE_ERR_INVALID naming the layer.  Valid only on a D2FE_PREC_I8 handle (else D2FE_ERR_INVALID), after
 * d2fe_load_superpoint (else D2FE_ERR_NOT_READY); a later d2fe_load_superpoint clears the ranges.  A load: refused while pipes are alive.
 * d2slam_amd/calibrate.py measures the ranges ("MinMax") offline; the calibration session below collects them on the device. */
D2FE_API int d2fe_set_superpoint_int8_ranges(d2fe_handle h, const float* range, int n);

/* Int8 calibration session: the statistics of the twelve tensors above, collected on the device, and the ranges by one of three rules on the host.
 *
 * d2fe_calib_create: h must be a D2FE_PREC_F32 handle with dense_descriptors = 1 (else D2FE_ERR_INVALID) and SuperPoint weights loaded (else
 *   D2FE_ERR_NOT_READY): the statistics are those of the exact network, and convDa / convDb exist densely.  n_bins: 128 .. 4096 in multiples of 128; 0 = 2048,
 *   the bin count of the published TensorRT calibrator.  The session counts as a user of the handle as a pipe does: d2fe_load_superpoint and the other loads are
 *   refused while it lives, d2fe_destroy is deferred to d2fe_calib_destroy.  Refused (D2FE_ERR_INVALID) while the handle has live pipes or another session.
 * d2fe_calib_collect: runs the exact network on n host images of one size (u8, `stride` bytes per row, `image_stride` bytes per image) within the handle's
 *   max_width x max_height; n may exceed max_batch (the call is sliced).  Behind the network the statistics kernels run on the handle's stream over: the outputs of
 *   conv1a .. conv4b as the next layer reads them (behind ReLU and, where the layer has one, the pool); convPa and convDa (ReLU outputs, the two channel halves of one
 *   buffer); convPb (the 65 logits) and convDb (the raw 256-channel map before normalisation) by absolute value.  No keypoints, no device-to-host copy, one host
 *   synchronisation, at the end.  Not re-entrant per handle, like the extract calls; do not interleave it with extract calls of other threads.
 * Range phase (before d2fe_calib_freeze): per tensor the running t_max = max |x| (kept as the fp32 bits of |x| under an integer max) and n_total.  NaN activations
 *   are outside the contract, as for D2FE_PREC_I8.
 * d2fe_calib_freeze: reads the maxima back and fixes per tensor T = max(t_max, 1e-30f) and scale = (float)n_bins / T (one fp32 divide); zeroes the histograms;
 *   n_total restarts.  D2FE_ERR_NOT_READY with no image collected, D2FE_ERR_INVALID a second time.
 * Histogram phase (d2fe_calib_collect after the freeze): for every value a = |x|, exactly
 *     a == 0 (either sign)  -> n_zero += 1                 (a zero quantises to 0 under any range: it is no part of the distribution)
 *     a >  T                -> n_over += 1, hist[n_bins - 1] += 1
 *     else                  -> hist[min(n_bins - 1, (int)(a * scale))] += 1      (one fp32 multiply, round to nearest even, then truncation)
 *   All counters are 64-bit integers: the statistics of a set of images do not depend on how it is split into calls or batches.  Images first seen in this
 *   phase are legal; values above T are what n_over counts.
 * d2fe_calib_stats_get: layer in 0 .. D2FE_SP_NUM_LAYERS - 1; every output may be NULL.  t_max: the running maximum (range phase) or the frozen one; hist (n_bins
 *   counters; D2FE_ERR_NOT_READY before the freeze), n_zero and n_over (0 before the freeze), n_total of the current phase.
 * d2fe_calib_ranges: range[D2FE_SP_NUM_LAYERS], every entry clamped to [1e-30, 1e30] (acceptable to d2fe_set_superpoint_int8_ranges).  Host code in double
 *   precision, plain sequential loops.  With N = the sum of hist (zeros excluded):
 *   D2FE_CALIB_MINMAX      T (param ignored); answerable in the range phase too.
 *   D2FE_CALIB_PERCENTILE  param in (0, 100] (else D2FE_ERR_INVALID): target = (uint64)ceil((double)N * (param / 100.0)); b = the first bin whose cumulative count
 *                          reaches target; range = (float)((double)(b + 1) * (double)T / n_bins).  N = 0: T.
 *   D2FE_CALIB_ENTROPY     (param ignored) the published KL-divergence calibration (NVIDIA, "8-bit inference with TensorRT"; ORT's Entropy method and MXNet follow
 *                          it), one-sided (the quantised inputs are ReLU outputs), 128 levels.  For every candidate i in 128 .. n_bins: P = hist[0 .. i) with the sum
 *                          of hist[i ..) added to P[i - 1]; level j covers the bins floor(j * i / 128) .. floor((j + 1) * i / 128) - 1; Q[b] = (the sum of the RAW hist
 *                          over b's level) / (the number of bins of the level with P[b] != 0) where P[b] != 0, else 0; p = P / sum(P), q = Q / sum(Q) (sums over b
 *                          ascending); KL(i) = the sum over b ascending with P[b] > 0 of p_b * ln(p_b / q_b).  A candidate with some p_b > 0, q_b = 0 is skipped (the
 *                          last level's raw counts all zero while outliers were folded in); no smoothing.  The smallest KL wins, among exact ties the smallest i;
 *                          range = (float)((double)i * (double)T / n_bins).  N = 0: T.  i = n_bins is always a valid candidate.
 *   The histogram phase is required for the last two (D2FE_ERR_NOT_READY before the freeze).
 * Limit: the entropy rule is this header's own statement of the published algorithm, not pinned to onnxruntime's bits (ORT's default of 128 histogram bins is
 * n_bins = 128); calibration table files of ORT or TensorRT are neither read nor written. */
typedef struct d2fe_calib_s* d2fe_calib;
typedef enum { D2FE_CALIB_MINMAX = 0, D2FE_CALIB_ENTROPY = 1, D2FE_CALIB_PERCENTILE = 2 } d2fe_calib_method;
D2FE_API int d2fe_calib_create(d2fe_handle h, int n_bins, d2fe_calib* out);
D2FE_API int d2fe_calib_collect(d2fe_calib c, const uint8_t* gray, int width, int height, int stride, long long image_stride, int n);
D2FE_API int d2fe_calib_freeze(d2fe_calib c);
D2FE_API int d2fe_calib_stats_get(d2fe_calib c, int layer, float* t_max, uint64_t* hist, uint64_t* n_zero, uint64_t* n_over, uint64_t* n_total);
D2FE_API int d2fe_calib_ranges(d2fe_calib c, int method, double param, float* range);
D2FE_API void d2fe_calib_destroy(d2fe_calib c);

/* Extractor.  Replaces: bool SuperPoint::infer(const cv::Mat&, std::vector<cv::Point2f>&, std::vector<float>&
 * descriptors, std::vector<float>& scores) (superpoint_tensorrt.h:47-48, .cpp:161-183), called from
 * LoopCam::extractorImgDescDeepnet (loop_cam.cpp:609-610).
 *   gray: u8 image, height rows of `stride` bytes.   kps_xy: cap*2 floats (x,y).   scores: cap floats.
 *   desc: cap*D floats keypoint-major, D = d2fe_desc_dim() (256 unless PCA is set).   *n_out = number of keypoints written (0 on failure).
 * Order of outputs = selection order of the chosen variant (B: raster if K<=N else score-desc; A: score-desc).
 * Not re-entrant per handle (the reference has one caller thread, d2frontend.cpp:155-169). */
D2FE_API int d2fe_superpoint_extract(d2fe_handle h, const uint8_t* gray, int width, int height, int stride,
                                     float* kps_xy, float* scores, float* desc, int cap, int* n_out);

/* Batched form of the same call: n images of identical size, image i at gray + i*image_stride bytes;
 * outputs of image i at kps_xy + i*cap*2, scores + i*cap, desc + i*cap*256, n_out[i]. */
/* async_tail mode: the stream on which the outputs of the last d2fe_superpoint_extract_device call become valid, and a helper
 * that makes another stream wait for them. */
D2FE_API void* d2fe_tail_stream(d2fe_handle h);
D2FE_API int d2fe_superpoint_wait_tail(d2fe_handle h, void* stream);
D2FE_API int d2fe_superpoint_extract_batch(d2fe_handle h, const uint8_t* gray, int n, int width, int height,
                                           int stride, size_t image_stride, float* kps_xy, float* scores,
                                           float* desc, int cap, int* n_out);

/* Device-resident form: inputs already in HBM (d_gray) and outputs left in HBM (d_*), asynchronous on
 * `stream` (a hipStream_t, or NULL for the handle's own stream).  d_n_out: n int32 counts.
 * d_kps_idx (optional, may be NULL): raster indices y*W+x of the keypoints. */
D2FE_API int d2fe_superpoint_extract_device(d2fe_handle h, const uint8_t* d_gray, int n, int width, int height,
                                            int stride, size_t image_stride, float* d_kps_xy, float* d_scores,
                                            float* d_desc, int32_t* d_kps_idx, int cap, int32_t* d_n_out,
                                            void* stream);

/* ---- NetVLAD global descriptor ---------------------------------------------------------------------------------------
 * Replaces: MobileNetVLADONNX (d2frontend/include/d2frontend/CNN/mobilenetvlad_onnx.h:18-74): ctor = ORT session + PCA
 * CSV (:35-46), inference(const cv::Mat&) -> std::vector<float> of 4096 (or PCA dims) (:49-74), called from
 * LoopCam::extractorImgDescDeepnet (loop_cam.cpp:612-616).  The reference's graph file is not in its tree:
 * the network is given as a flat layer list (kinds below), so any MobileNetV2-style trunk + NetVLAD head can be loaded;
 * d2slam_amd/netvlad.py holds the documented stand-in.  Layouts: conv [cout][1][3][3] (3x3 from the 1-channel image, in-graph
 * (x-128)/128), dw [c][3][3], pw [cout][cin]; TF "SAME" padding; act 0 none / 1 ReLU / 2 ReLU6; res = index of the layer whose
 * output is added (-1 none).  Head: 1x1 pre-projection feat_dim -> proj_dim, soft-assignment [K][proj_dim], centroids. */
typedef enum { D2FE_NV_CONV = 0, D2FE_NV_PW = 1, D2FE_NV_DW = 2 } d2fe_nv_kind;
typedef struct {
  int32_t kind, cin, cout, stride, act, res;
  const float* weight;
  const float* bias;
} d2fe_nv_layer;
typedef struct {
  int32_t n_layers;
  const d2fe_nv_layer* layers;
  int32_t feat_dim, proj_dim, n_clusters;
  const float* pre_w;      /* [proj_dim][feat_dim] */
  const float* pre_b;      /* [proj_dim] */
  const float* assign_w;   /* [n_clusters][proj_dim] */
  const float* assign_b;   /* [n_clusters] */
  const float* centroids;  /* [n_clusters][proj_dim] */
} d2fe_netvlad_weights;
D2FE_API int d2fe_load_netvlad(d2fe_handle h, const d2fe_netvlad_weights* w);
/* PCA of the global descriptor: comp [m][G], mean [G], G = n_clusters*proj_dim (the reference's CSV: row 0 = mean,
 * rows 1.. = components, mobilenetvlad_onnx.h:35-41).  m = 0 disables. */
D2FE_API int d2fe_set_netvlad_pca(d2fe_handle h, const float* comp, const float* mean, int m);
D2FE_API int d2fe_netvlad_dim(d2fe_handle h);   /* length of the descriptor written by the calls below */
/* std::vector<float> MobileNetVLADONNX::inference(const cv::Mat&): gray u8 at the network's size (the reference resizes with
 * cv::resize when needed; that stays the caller's job).  out: d2fe_netvlad_dim() floats. */
/* Like the extract calls, the NetVLAD calls are not re-entrant per handle (they reuse the handle's layer buffers and record the slab
 * layout of the call in it); the reference calls MobileNetVLADONNX::inference from its one front-end thread (d2frontend.cpp:155-169). */
D2FE_API int d2fe_netvlad(d2fe_handle h, const uint8_t* gray, int width, int height, int stride, float* out);
D2FE_API int d2fe_netvlad_batch(d2fe_handle h, const uint8_t* gray, int n, int width, int height, int stride,
                                size_t image_stride, float* out);
D2FE_API int d2fe_netvlad_device(d2fe_handle h, const uint8_t* d_gray, int n, int width, int height, int stride,
                                 size_t image_stride, float* d_out, void* stream);

/* Fused form of the two calls LoopCam::extractorImgDescDeepnet makes for one image (loop_cam.cpp:609-616: superpoint_net->infer(...) and then
 * netvlad_onnx->inference(...) on the same frame): ONE upload, SuperPoint and NetVLAD on two streams side by side (at one or two images per call
 * both are latency-bound and leave most of the chip idle), one synchronisation.  Same outputs, bit for bit, as d2fe_superpoint_extract(_batch)
 * followed by d2fe_netvlad(_batch) on the first n_netvlad images (stereo: the left image, loop_cam.cpp:446-451).  netvlad_out: n_netvlad x
 * d2fe_netvlad_dim() floats.  Needs both networks loaded and an image size both accept. */
D2FE_API int d2fe_extract_all(d2fe_handle h, const uint8_t* gray, int width, int height, int stride, float* kps_xy, float* scores, float* desc,
                              int cap, int* n_out, float* netvlad_out);
D2FE_API int d2fe_extract_all_batch(d2fe_handle h, const uint8_t* gray, int n, int width, int height, int stride, size_t image_stride,
                                    float* kps_xy, float* scores, float* desc, int cap, int* n_out, int n_netvlad, float* netvlad_out);

/* Matcher.  Replaces: std::vector<cv::DMatch> matchKNN(const cv::Mat& desc_a, const cv::Mat& desc_b,
 * double knn_match_ratio, pts_a, pts_b, double search_local_dist) (feature_matcher.h:6-11,
 * feature_matcher.cpp:4-42).  a: na x dim row-major, b: nb x dim.  pts_*: n x 2 floats or NULL.
 * radius <= 0 disables the pixel gate.  Outputs ascending in query index; *n_out matches written.
 * Re-entrant (the reference calls it from three threads). */
/* Up to 16384 rows per side (the reference is unbounded; D2FE_ERR_UNSUPPORTED above that). */
D2FE_API int d2fe_match_knn(d2fe_handle h, const float* a, int na, const float* b, int nb, int dim, double ratio,
                            const float* pts_a, const float* pts_b, double radius, int32_t* q_idx,
                            int32_t* t_idx, float* dist, int cap, int* n_out);

/* Replaces: cv::BFMatcher(cv::NORM_L2, true).match(desc_a, desc_b, matches)
 * (loop_cam.cpp:167-170, d2featuretracker.cpp:1141-1142,1175-1176, loop_detector.cpp:576-577). */
D2FE_API int d2fe_match_crosscheck(d2fe_handle h, const float* a, int na, const float* b, int nb, int dim,
                                   int32_t* q_idx, int32_t* t_idx, float* dist, int cap, int* n_out);

/* Both matchers select candidates on a Gram-trick distance (fp32 matrix pipe) whose error against the reference's (OpenCV's) arithmetic
 * is rigorously bounded: every train row that the bound cannot separate from the second-nearest one (2.0-2.3 rows per query on
 * SuperPoint descriptors) is re-ranked in the reference's arithmetic; a query with more than 16 such rows (repeated texture,
 * near-duplicate frames, degenerate sets) is re-evaluated by an exact scan of all train rows.  The result equals the reference's for any
 * input.  d2fe_match_fallback_rows returns how many candidates beyond two per query were re-ranked since the last reset and, in
 * *full_scans (may be NULL), how many queries took the exact scan (diagnostic; synchronises the device). */
D2FE_API long d2fe_match_fallback_rows(d2fe_handle h, int reset, long* full_scans);

/* Batched, device-resident matcher: npairs problems; pair p matches rows [a_off[p], a_off[p]+a_cnt[p]) of
 * d_a against rows [b_off[p], ...) of d_b.  Counts may live on the device (d_a_cnt/d_b_cnt, e.g. the d_n_out
 * of an extract call) -- pass max_n as the upper bound of any count.  mode: 0 = matchKNN, 1 = cross-check.
 * Outputs: pair p writes at most max_n matches at d_q_idx + p*max_n etc., and d_n_out[p]. */
typedef struct {
  const float* d_a; const float* d_b;             /* descriptor pools, row-major dim floats per row */
  const float* d_pts_a; const float* d_pts_b;     /* optional pools of (x,y), may be NULL */
  const int32_t* d_a_off; const int32_t* d_b_off; /* [npairs] first row of each side */
  const int32_t* d_a_cnt; const int32_t* d_b_cnt; /* [npairs] row counts (device) */
  int32_t npairs, dim, max_n, mode;
  double ratio, radius;
  int32_t* d_q_idx; int32_t* d_t_idx; float* d_dist; int32_t* d_n_out;
} d2fe_match_batch;
D2FE_API int d2fe_match_batch_device(d2fe_handle h, const d2fe_match_batch* mb, void* stream);

/* ---- Frames in flight (throughput form of the per-frame work) ------------------------------------------------------------------
 * The reference handles ONE stereo frame at a time on one thread (D2Frontend::processStereoframe, d2frontend.cpp:155-169): per image
 * SuperPoint::infer and, for the main camera, MobileNetVLADONNX::inference (LoopCam::extractorImgDescDeepnet, loop_cam.cpp:589-648,
 * both cameras: generateStereoImageDescriptor :440-470), then matchKNN left<->right and left<->previous left
 * (D2FeatureTracker::trackLocalFrames, d2featuretracker.cpp:403-456,658-695).  A pipe runs exactly that work for `frames` stereo
 * frames per submit with up to `lanes` submits in flight: d2fe_pipe_submit only enqueues (H2D, both networks, ONE matcher launch,
 * ONE D2H, on the lane's own streams), d2fe_pipe_wait returns pointers into the lane's pinned result block.  Results are bit-identical
 * to d2fe_extract_all_batch + d2fe_match_knn on the same frames.  A pipe borrows the handle's packed weights: while a pipe exists d2fe_destroy
 * of its handle is DEFERRED (the handle is released by the last d2fe_pipe_destroy; d2fe_last_error says so) and d2fe_load_* / d2fe_set_*_pca return
 * D2FE_ERR_INVALID -- destroy the pipes first.  A submit whose pass would overwrite a result block with an unreleased device view returns D2FE_ERR_NOT_READY
 * and queues nothing (release the view, submit again).  The first error of a
 * submit or wait is final for the pipe: every later call returns it (a half-enqueued pass cannot be built on); destroy the pipe and create a new one.  One submitting thread per pipe; d2fe_pipe_wait may be called from a second thread (the reference's image
 * callback and its tracker are two threads): the pipe serialises its own bookkeeping and does not hold the lock while a wait blocks.  The caller bounds the
 * frames between its two threads (a queue of at most lanes * coalesce tickets is always safe), as the result blocks are a ring of 2 * lanes passes. */
typedef struct d2fe_pipe_s* d2fe_pipe;
typedef struct {
  int32_t struct_size;      /* sizeof(d2fe_pipe_config) */
  int32_t lanes;            /* submits in flight, 1..16 (each lane owns its activations: ~58 MB per 640x480 image; lr_lk: activations for the left images
                               only, plus the lane's image pyramids, 1.3125 bytes per pixel of both images = 0.8 MB per 640x480 stereo frame) */
  int32_t frames;           /* stereo frames per submit (>= 1); consecutive in time */
  int32_t width, height;    /* frame size, within the handle's maximum */
  int32_t cap;              /* keypoint capacity per image (rows of the result arrays) */
  int32_t netvlad;          /* 1: NetVLAD of the left images (the main camera, loop_cam.cpp:446-451) */
  int32_t match_lr;         /* 1: matchKNN L_f <-> R_f */
  int32_t match_prev;       /* 1: matchKNN L_f <-> L_(f-1); f = 0: the last left frame of the previous submit (none for the first) */
  int32_t pinned_input;     /* 1: the frame pointers handed to submit are page-locked and stay valid until the ticket was waited for
                               (DMA straight from them); 0: submit copies the frames into the lane's pinned staging first */
  double ratio;             /* knn_match_ratio */
  double radius_lr;         /* search_local_max_dist_lr * width (<= 0: off), d2featuretracker.cpp:669 */
  double radius_prev;       /* search_local_max_dist * width (<= 0: off), d2featuretracker.cpp:21-28 */
  int32_t cu_partition;     /* 1: every lane launches on its own disjoint 1/lanes of the compute units (CU-masked streams): the lanes' kernels run
                               side by side instead of queueing behind each other's full-device launches.  For small `frames`: a lane then
                               behaves like a (256 / lanes)-CU device working on its own frame */
  int32_t netvlad_inline;   /* which stream a pass's NetVLAD call is launched on.  0: the lane's second stream, beside SuperPoint (shortest single pass: 0.72 ms);
                               1: the lane's one stream, in front of SuperPoint (no second streams are created);
                               2 (d2fe_pipe_default_config): auto -- decided per pass: the second stream while at most one OTHER pass is in flight, the lane's own
                               stream beyond that (one or two lanes: always the second stream).  Why: the device runs FOUR busy streams of a process side by side
                               (hardware queue i is served by hardware pipe i mod 4) and makes a fifth take turns.  Single-frame passes on a 4-lane pipe, auto:
                               1390 / 1838 / 1789 / 2044 stereo frames/s with 1 / 2 / 3 / 4 passes in flight; forced second streams: 1627 with 4
                               (profiles/r05_pipe_one_frame.txt (8)).  d2fe_pipe_create measures which streams share a hardware pipe and gives a lane two streams of
                               different pipes (d2fe_pipe_stream_placement); create the pipe on a quiet device.
                               Results are the same bits in every mode */
  int32_t coalesce;         /* > 1 (needs frames == 1): up to this many consecutive submits run as ONE launch sequence when they are submitted before
                               anybody waits for them -- submit() stages the frame (its H2D starts at once) and the pass is launched when it is full
                               or when d2fe_pipe_wait asks for one of its tickets; results per ticket are unchanged (bit-identical).  What a
                               throughput-oriented caller that receives frames one at a time would otherwise do by hand with frames = 2 */
  int32_t lane_cus;         /* > 0: a lane's persistent kernels size their grids for this many compute units (no CU mask: they may run on any CU).  A
                               full-device persistent launch occupies every CU's LDS until it ends, so other lanes' small launches wait for it;
                               with e.g. 128 of 256, two lanes run side by side on every CU.  0: the whole device */
  int32_t netvlad_group;    /* > 1 (needs frames == 1, coalesce == 1, lanes % netvlad_group == 0): the NetVLAD descriptors of this many consecutive
                               submits are computed by ONE call on the pipe's own stream when the last of them has been submitted (or when
                               d2fe_pipe_wait asks for one of them), while SuperPoint and the matches of every submit start at once.  NetVLAD of a
                               single image is ~20 launches of a few workgroups each (0.25 ms for one image, 0.28 ms for four); the descriptor feeds
                               loop detection, not the tracker, so it can trail the keypoints.  Bit-identical results */
  int32_t coalesce_depth;   /* with coalesce > 1.  0: a pass is launched when it is full (or when d2fe_pipe_wait asks).  N > 0: ALSO as soon as fewer than N
                               passes are in flight on the device -- dynamic batching: a caller that waits for every frame before it submits the next
                               gets every frame launched at once (the latency of coalesce = 1), a caller that keeps many frames in flight gets passes
                               that grow up to `coalesce` frames while the device is busy with N others (the throughput of large passes).  2 is the
                               measured choice: one pass running, one queued behind it */
  int32_t lr_lk;            /* 1: the reference's DEFAULT stereo path (lr_match_use_lk = true, d2featuretracker.h:61; trackLocalFrames, d2featuretracker.cpp:110-116):
                               SuperPoint (and NetVLAD) on the LEFT images only; the image pyramids of both images are built on the device and every left
                               keypoint is tracked left -> right with pyramidal LK (trackLK -> opticalflowTrackPyr, d2featuretracker.cpp:697-752,
                               opticaltrack_utils.cpp:173-279: forward, reverse, 0.5 px round trip, inBorder; window 21, PYR_LEVEL 2, 30 iterations), stream-ordered
                               inside the pass (levels + 1 launches whatever `frames` is, no host synchronisation); the results travel with the pass's one D2H
                               and are read with d2fe_pipe_lk_result_get.  submit() takes the same arguments (the right images are uploaded; only their
                               pyramids are built).  d2fe_pipe_result keeps its layout: rows of right images have n_kp = 0, the left rows, NetVLAD and the
                               prev_* lists are bit-identical to the same pipe with lr_lk = 0, match_lr = 0; lr_* are NULL.  Needs match_lr = 0 (the right
                               image has no descriptors: D2FE_ERR_INVALID otherwise).  Works with any lanes / frames, netvlad, match_prev, pinned_input,
                               coalesce, coalesce_depth, netvlad_inline, netvlad_group, lane_cus and cu_partition (the LK launches run on the lane's own
                               stream, CU-masked or not).  0 (d2fe_pipe_default_config): SuperPoint on both images, as before */
  int32_t sp_lk;            /* 1 (needs lr_lk = 1 or mono = 1, D2FE_ERR_INVALID otherwise; sp_lk with lr_lk are the reference's defaults): the OTHER half of the reference's stereo
                               tracker, sp_track_use_lk = true (d2featuretracker.h:63): the temporal association is the LK-carried landmark list of
                               D2FeatureTracker::trackLK(frame) (d2featuretracker.cpp:472-621), kept on the DEVICE and carried across frames, passes and lanes: per left
                               frame one d2fe_lk_carry_step_device (track the previous list, reduceVector, removeNearPoints, replenish from the frame's SuperPoint
                               keypoints, carry descriptors), in time order behind the pass's pyramids, then ONE left -> right launch over the list entries of all
                               frames.  A pass's chain starts from the last list and the last left pyramid of the previous pass (an event orders it behind that pass's
                               chain; the pyramid is copied to a pipe-owned buffer, the list is read where the previous pass left it); next_id is the pipe's.  The
                               lists travel with the pass's one D2H and are read with d2fe_pipe_track_result_get; d2fe_pipe_lk_result_get is D2FE_ERR_UNSUPPORTED (the
                               per-keypoint left -> right launch is not issued).  d2fe_pipe_result is bit-identical to the same pipe with sp_lk = 0 (match_prev stays
                               available).  Parameters: d2fe_pipe_set_track_params before the first submit (the reference's defaults otherwise).  Works with any
                               lanes / frames and every other option; frames are chained in submit order.  0 (d2fe_pipe_default_config): off.
                               With d2fe_pipe_camera::mono = 1 in place of lr_lk = 1: the same chain on the pyramids of the one image (only those are built: half the workspace); the
                               left -> right launch is not issued, d2fe_pipe_track_result::right_xy / right_status are NULL */
} d2fe_pipe_config;
typedef struct {            /* HOST pointers into the lane's pinned block; valid until 2 * lanes further submits */
  int32_t frames, cap, desc_dim, netvlad_dim;
  const float* kps_xy;      /* [2 frames][cap][2]   image order L_0 .. L_(F-1), R_0 .. R_(F-1) */
  const float* scores;      /* [2 frames][cap] */
  const float* desc;        /* [2 frames][cap][desc_dim] */
  const int32_t* n_kp;      /* [2 frames] */
  const float* netvlad;     /* [frames][netvlad_dim] or NULL */
  const int32_t* lr_q; const int32_t* lr_t; const float* lr_dist; const int32_t* lr_n;            /* [frames][cap] x3, [frames]; NULL when off */
  const int32_t* prev_q; const int32_t* prev_t; const float* prev_dist; const int32_t* prev_n;    /* prev_t indexes the previous left frame's keypoints */
} d2fe_pipe_result;
/* lr_lk = 1: the left -> right LK tracks of a ticket that d2fe_pipe_wait has returned (D2FE_ERR_NOT_READY before that, D2FE_ERR_UNSUPPORTED on a pipe without
 * lr_lk).  Every left keypoint is tracked: keypoint i of left frame f (d2fe_pipe_result::kps_xy row f, i < n_kp[f]) is at pts_xy[f][i] in the right image when
 * status[f][i] == 1; slots i >= n_kp[f] hold status 0 and (0, 0).  The reduceVector compaction and the landmark_id >= 0 filter of trackLK
 * (d2featuretracker.cpp:707-719) stay with the caller, as for d2fe_lk_track. */
typedef struct {            /* HOST pointers into the lane's pinned block, same lifetime as d2fe_pipe_result */
  int32_t frames, cap;
  const float* pts_xy;      /* [frames][cap][2]  right-image position of left keypoint i of frame f */
  const uint8_t* status;    /* [frames][cap]     1: forward && reverse && |prev - reverse| <= 0.5 && inBorder (opticaltrack_utils.cpp:260-272) */
} d2fe_pipe_lk_result;
/* The camera configurations with ONE camera per frame (the reference has five, d2basetypes.h:40-46; the stereo pipe above is STEREO_PINHOLE).  d2fe_pipe_config is a
 * closed struct of 96 bytes (its last two ints went to lr_lk and sp_lk, and its size is checked strictly), so the two options live in a struct of their own, handed to
 * d2fe_pipe_create_camera beside the pipe's configuration.  d2fe_pipe_create(h, cfg, out) is d2fe_pipe_create_camera(h, cfg, NULL, out): a stereo pipe, as before. */
typedef struct {
  int32_t struct_size;      /* sizeof(d2fe_pipe_camera), checked strictly */
  int32_t mono;             /* 1: ONE camera per frame -- the reference's MONOCULAR configuration (d2basetypes.h:40-46; config/gopro, config/visensor_f9p): SuperPoint
                               and NetVLAD on the one image (LoopCam::generateImageDescriptor, loop_cam.cpp:259-331), matchKNN against the previous frame
                               (D2FeatureTracker::track, d2featuretracker.cpp:105-107) or, with sp_lk, the LK-carried list.  Needs match_lr = 0 and lr_lk = 0
                               (D2FE_ERR_INVALID otherwise).  d2fe_pipe_submit takes right = NULL (a non-NULL right image is D2FE_ERR_INVALID; it queues nothing and does
                               not end the pipe).  A lane uploads, stages and holds activations for frames * coalesce images, not twice that.  d2fe_pipe_result and
                               d2fe_pipe_device_result keep their [2 frames] layout exactly as with lr_lk: the rows of "right" images have n_kp = 0 in every pass, on
                               the device too, lr_* are NULL, and the left rows, NetVLAD and the prev_* lists are bit-identical to the stereo pipe with match_lr = 0
                               on the same left frames -- so d2fe_exchange_*, d2fe_loop_*, d2fe_window_* and the device views work on a mono pipe unchanged.  Works
                               with lanes, frames, netvlad, match_prev, pinned_input, coalesce, coalesce_depth, netvlad_inline, netvlad_group, lane_cus and
                               cu_partition.  0 (d2fe_pipe_camera_default): a stereo pipe, as before */
  int32_t depth;            /* 1 (needs mono = 1, D2FE_ERR_INVALID otherwise): the reference's PINHOLE_DEPTH configuration -- every frame comes with a 16-bit depth
                               image of the same width x height (LoopCam::generateGrayDepthImageDescriptor, loop_cam.cpp:333-441).  Frames enter through
                               d2fe_pipe_submit_depth (plain d2fe_pipe_submit is D2FE_ERR_INVALID on such a pipe, d2fe_pipe_submit_depth on every other pipe; neither
                               refusal ends the pipe); the depth frames travel like the gray ones (pinned staging unless pinned_input, H2D on the lane's stream).  ONE
                               launch per pass behind the SuperPoint tail (with sp_lk: behind the chain) reads the depth under every keypoint and every list entry; the
                               values travel with the pass's one D2H and are read with d2fe_pipe_depth_result_get.  Every other result is bit-identical to the same
                               pipe with depth = 0.  0 (d2fe_pipe_camera_default): off */
  int32_t reserved;         /* 0 */
} d2fe_pipe_camera;
D2FE_API void d2fe_pipe_camera_default(d2fe_pipe_camera* cam);      /* struct_size, mono = 0, depth = 0 */
D2FE_API int d2fe_pipe_create_camera(d2fe_handle h, const d2fe_pipe_config* cfg, const d2fe_pipe_camera* cam /* NULL: stereo */, d2fe_pipe* out);
D2FE_API void d2fe_pipe_default_config(d2fe_pipe_config* cfg);
D2FE_API int d2fe_pipe_create(d2fe_handle h, const d2fe_pipe_config* cfg, d2fe_pipe* out);
D2FE_API void d2fe_pipe_destroy(d2fe_pipe p);
D2FE_API int d2fe_pipe_lanes(d2fe_pipe p);
/* How d2fe_pipe_create placed the lanes' streams: it measures which of its candidate streams take turns on the device (streams of one hardware pipe) and gives every
 * lane two streams of different pipes.  classes[2 k] / classes[2 k + 1] = the class of lane k's own / second stream (-1: no such stream, or CU-masked lanes),
 * *n_classes = the classes told apart (4 on an idle MI355X; 0: the device was not quiet or nothing could be told apart -- the arrangement of a fresh process was used) */
D2FE_API int d2fe_pipe_stream_placement(d2fe_pipe p, int32_t* classes /*[2 * lanes]*/, int32_t* n_classes);
/* d2fe_profile_enable / d2fe_profile_read over all lanes (sums) */
D2FE_API int d2fe_pipe_profile_enable(d2fe_pipe p, int mode);
D2FE_API int d2fe_pipe_profile_read(d2fe_pipe p, float* ms /*[D2FE_PROF_COUNT]*/, int32_t* launches /*[D2FE_PROF_COUNT]*/);
/* left / right: `frames` gray u8 images each, image f at + f * image_stride, rows `stride` bytes apart (a mono pipe, d2fe_pipe_camera::mono = 1: right is NULL).  Returns at once with a ticket
 * (0, 1, 2, ...).  Blocks only when the ticket's lane still holds the pass submitted `lanes` passes ago that nobody waited for. */
D2FE_API int d2fe_pipe_submit(d2fe_pipe p, const uint8_t* left, const uint8_t* right, int stride, size_t image_stride, int64_t* ticket);
/* Blocks until the ticket's frame is complete on the host (launching its pass first if coalescing still holds it back).  Tickets may be waited
 * for in any order, each within 2 * lanes passes (a pass = `coalesce` submits). */
D2FE_API int d2fe_pipe_wait(d2fe_pipe p, int64_t ticket, d2fe_pipe_result* out);
D2FE_API int d2fe_pipe_lk_result_get(d2fe_pipe p, int64_t ticket, d2fe_pipe_lk_result* out);
/* sp_lk = 1: the landmark lists of a ticket that d2fe_pipe_wait has returned (D2FE_ERR_NOT_READY before that, D2FE_ERR_UNSUPPORTED on a pipe without sp_lk).
 * Frame f's list is a d2fe_lk_carry_step_device list block; the per-list pointers below address frame 0's block and frame f's is `list_words` 32-bit words
 * further on for EVERY one of them (n[f * list_words], pts_xy + f * list_words, ...).  Entry i < n of frame f: position pts_xy[i] in the left image, id[i]
 * (pipe-wide, counted from 0 in order of discovery: the caller maps it to its lmanager id), src[i] = its index in the PREVIOUS frame's list (-1: discovered in
 * this frame, from SuperPoint keypoint kp[i] of d2fe_pipe_result's left row; kp = -1 for tracked entries), desc / scores = the SuperPoint row of its discovery
 * frame (d2featuretracker.cpp:509-521), right_xy[f][i] / right_status[f][i] = its left -> right track (trackLK(left, right), :697-752; semantics of
 * d2fe_pipe_lk_result).  Slots >= n hold zeros.  What stays with the caller: id -> lmanager ids, the NaN skip of createLKLandmark (an entry it rejects keeps
 * its slot here) and velocities; its liftProjective / bearings, the extrinsic prediction and the lk_lk_use_pred gate run on the device once
 * d2fe_pipe_bearings_enable has switched them on, and are the caller's otherwise. */
typedef struct {            /* HOST pointers into the lane's pinned block, same lifetime as d2fe_pipe_result */
  int32_t frames, cap_tracks, desc_dim, list_words;
  const int32_t* n;                  /* per list: entries -- frame f's count is n[f * list_words], NOT n[f]; the same stride for every "per list" pointer below */
  const int32_t* n_tracked_in;       /* per list (n_tracked_in[f * list_words]): entries of the previous list that were tracked (its n) */
  const int32_t* n_lost;             /* per list (n_lost[f * list_words]): dropped by the tracker's status (reduceVector) */
  const int32_t* n_removed_near;     /* per list (n_removed_near[f * list_words]): dropped by removeNearPoints */
  const int32_t* n_new;              /* per list (n_new[f * list_words]): appended from this frame's SuperPoint keypoints */
  const float* pts_xy;               /* per list: [cap_tracks][2] at pts_xy + f * list_words */
  const int32_t* id; const int32_t* src; const int32_t* kp;      /* per list: [cap_tracks] at + f * list_words */
  const float* desc;                 /* per list: [cap_tracks][desc_dim] at desc + f * list_words */
  const float* scores;               /* per list: [cap_tracks] at scores + f * list_words */
  const float* right_xy;             /* [frames][cap_tracks][2], contiguous (NOT strided by list_words); NULL on a mono pipe */
  const uint8_t* right_status;       /* [frames][cap_tracks], contiguous; NULL on a mono pipe */
} d2fe_pipe_track_result;
D2FE_API int d2fe_pipe_track_result_get(d2fe_pipe p, int64_t ticket, d2fe_pipe_track_result* out);
/* sp_lk = 1: replaces the reference's default tracker parameters (d2fe_track_default_params).  Accepted only before the first submit (D2FE_ERR_INVALID afterwards,
 * on a pipe without sp_lk, for levels != 2 -- the lane's pyramid workspace is PYR_LEVEL deep -- and for parameters d2fe_lk_carry_step_device refuses, e.g.
 * total_feature_num + 1 > 1024); a refusal leaves the pipe as it was. */
struct d2fe_track_params_s;
D2FE_API int d2fe_pipe_set_track_params(d2fe_pipe p, const struct d2fe_track_params_s* tp);
/* depth = 1: d2fe_pipe_submit with a depth frame per gray frame.  gray as `left` of d2fe_pipe_submit; depth: `frames` images of uint16_t, width x height, image f at
 * + f * depth_image_stride BYTES, rows depth_stride BYTES apart (both even, depth_stride >= 2 * width).  With pinned_input both pointers are page-locked and stay
 * valid until the ticket was waited for. */
D2FE_API int d2fe_pipe_submit_depth(d2fe_pipe p, const uint8_t* gray, const uint16_t* depth, int stride, int depth_stride, size_t image_stride,
                                    size_t depth_image_stride, int64_t* ticket);
/* depth = 1: the depth values of a ticket that d2fe_pipe_wait has returned (D2FE_ERR_NOT_READY before that, D2FE_ERR_UNSUPPORTED on a pipe without depth).
 * Value contract: for a point (x, y) the value is depth[iy][ix] with ix = cvRound(x), iy = cvRound(y); cvRound rounds half to even (2.5 -> 2, 3.5 -> 4,
 * -0.5 -> 0), which is what cv::Mat::at<ushort>(cv::Point2f) does through Point_<float> -> Point_<int> -> saturate_cast<int> (upstream OpenCV behaviour, not part
 * of the reference tree; the reference's reads are loop_cam.cpp:382 and d2featuretracker.cpp:790-798).  If ix or iy falls outside the image, or a coordinate is NaN,
 * the value is 0: the reference would read out of bounds there, and 0 fails its dep > DEPTH_NEAR_THRES test.  Values are raw (millimetres for a RealSense): the
 * / 1000.0, DEPTH_NEAR_THRES / DEPTH_FAR_THRES, pt3d = pose_cam * (pt2d_norm * dep) and depth = pt3dcam.norm() stay with the caller; pt2d_norm (liftProjective,
 * normalised) is d2fe_pipe_bearings_result::kp_bearing once d2fe_pipe_bearings_enable has switched the bearings on, the caller's otherwise. */
typedef struct {            /* HOST pointers into the lane's pinned block, same lifetime as d2fe_pipe_result */
  int32_t frames, cap, cap_tracks, reserved;
  const uint16_t* kp_depth_mm;       /* [frames][cap]: the value under keypoint i of frame f (d2fe_pipe_result::kps_xy row f); slots >= n_kp[f] hold 0 */
  const uint16_t* track_depth_mm;    /* sp_lk: [frames][cap_tracks], contiguous: the value under list entry i of frame f at its position in that frame
                                        (d2fe_pipe_track_result::pts_xy); slots >= n hold 0.  NULL without sp_lk */
} d2fe_pipe_depth_result;
D2FE_API int d2fe_pipe_depth_result_get(d2fe_pipe p, int64_t ticket, d2fe_pipe_depth_result* out);
/* The single-call form of the same lookup (what the pipe launches): n_lists point lists against n_lists depth images, asynchronous on `stream` (a hipStream_t; NULL:
 * the handle's stream), no host synchronisation.  List l: depth image l at d_depth + l * depth_image_stride BYTES (rows depth_stride BYTES apart, both even), points
 * d_pts_xy + l * pts_stride floats as [cap][2], count d_n[l] (read on the device, clamped to 0..cap), values to d_out[l * cap .. l * cap + cap): the value contract
 * above for slots < d_n[l], 0 for the others.  All pointers are device memory. */
D2FE_API int d2fe_depth_at_device(d2fe_handle h, const uint16_t* d_depth, int width, int height, size_t depth_stride, size_t depth_image_stride,
                                  const float* d_pts_xy, size_t pts_stride /*floats between lists*/, const int32_t* d_n, int n_lists, int cap, uint16_t* d_out,
                                  void* stream);

/* Bearings, extrinsic predictions and their gate ON THE DEVICE: the per-point pass the reference's tracker runs on everything the front end returns.
 *   bearing     liftProjective of the point's camera, then P / sqrt(x*x + y*y + z*z) (LoopCam::extractorImgDescDeepnet, loop_cam.cpp:619-645;
 *               D2FeatureTracker::createLKLandmark, d2featuretracker.cpp:777-802).  A NaN component stays NaN: the hasNaN() skip stays the caller's.
 *   prediction  predictLandmarksWithExtrinsic (:1296-1313): X = T * (bearing * distance), then spaceToPlane OF THE CAMERA THE POINT WAS LIFTED WITH -- the reference
 *               projects into the right image with cams.at(left camera_index) (:1309); that quirk is kept.  Stored as (float)u, (float)v.
 *   gate        trackLK(left, right) with lk_lk_use_pred (:742-744): pred_ok[i] = status[i] && (radius <= 0 || cv::norm(pred[i] - other[i]) < radius), cv::norm on
 *               Point2f (float differences, sqrt of the double sum of squares); a NaN prediction fails `<` and is dropped.  other_bearing = the lift of the other
 *               point with the SECOND camera (createLKLandmark(right_frame, ...)).
 * Camera models: pinhole + radtan (PinholeCamera.cc:337-418), MEI (CataCamera.cc:425-515) and the cylindrical model of the quadcam views
 * (CylindricalCamera.cc:207-238, the virtual camera of FisheyeUndist with enable_undistort_image).
 * Arithmetic contract: fp64, operation by operation in the order of the host restatements of include/d2fe.hpp (liftProjectivePinhole, liftProjectiveMEI,
 * liftProjectiveCylindrical, fillLandmarks, predictWithExtrinsic, spaceToPlanePinhole, spaceToPlaneMEI, spaceToPlaneCylindrical); no contraction.  For the first two
 * models the device's fp64 sqrt and divide are the only operations that may differ from the host's, by the last bit of their own result.
 * D2FE_CAM_CYLINDRICAL, one operation per line:
 *   lift          phi = iK11 * x + iK13;  ybr = iK22 * y + iK23;  z = fabs(phi) > M_PI / 2 ? -1.0 : 1.0;  X = z * tan(phi);  rho = sqrt(X * X + z * z);  Y = ybr * rho;
 *                 then (X, Y, z) / sqrt(X * X + Y * Y + z * z) as for the other models; iK11 = 1 / fx, iK13 = -cx / fx, iK22 = 1 / fy, iK23 = -cy / fy from the host
 *   spaceToPlane  rho = sqrt(X * X + Z * Z);  phi = atan2(X, Z);  a = rho * phi;  uh = (fx * a + 0.0 * Y) + cx * rho;  vh = (0.0 * a + fy * Y) + cy * rho;
 *                 w = (0.0 * a + 0.0 * Y) + 1.0 * rho;  u = uh / w;  v = vh / w -- K * (a, Y, rho) with the K of the constructor FisheyeUndist calls
 *                 (CylindricalCamera.cc:138-150), zero terms kept: a non-finite Y reaches u as it does through the matrix product.  A point on the axis (rho = 0) gives u = NaN and v = +-inf (NaN for Y = 0).
 *   tan and atan2 are the device math library's; like the device's sqrt and divide they may differ from the host's in the last bits of their own result, and the
 *   bound the tests hold the bearings to allows for it. */
typedef enum { D2FE_CAM_PINHOLE = 0, D2FE_CAM_MEI = 1, D2FE_CAM_CYLINDRICAL = 3 /* 2 is not a kind and is refused */ } d2fe_camera_kind;
typedef struct {
  int32_t kind, reserved;   /* d2fe_camera_kind; 0 */
  double p[9];              /* PINHOLE: fx fy cx cy k1 k2 p1 p2, p[8] = 0;  MEI: the nine doubles of d2fe_mei_camera in its order (xi k1 k2 p1 p2 gamma1 gamma2 u0 v0);
                               CYLINDRICAL: fx fy cx cy, p[4..8] = 0 */
} d2fe_camera;
/* The virtual camera d2fe_gen_cylinder_map assumes for a width x height view of fov_deg degrees (FisheyeUndist, fisheye_undistort.h:492-495): kind
 * D2FE_CAM_CYLINDRICAL, fx = fy = the generator's own focal length (double)width / (fov_deg * (pi / 180)), cx = width / 2, cy = height / 2 (integer halves).  Host
 * function, no device needed.  D2FE_ERR_INVALID: out NULL, width or height < 1, fov_deg not positive. */
D2FE_API int d2fe_cylinder_camera(int width, int height, double fov_deg, d2fe_camera* out);
/* T_b_a [3][4] row-major, the transform that takes a point of frame a into frame b, from the two poses (unit quaternion w x y z, translation) of a and b in a common
 * frame: R(q) by the standard unit-quaternion formula after q /= sqrt(w*w + x*x + y*y + z*z), T_b_a = [R_b^T R_a | R_b^T (t_a - t_b)], every dot product summed left
 * to right.  Host function, no device needed.  This is the library's OWN arithmetic: the reference takes the matrix from Swarm::Pose (swarm_msgs, not in its tree), so
 * the last bits of its extrinsic are not restated here.  For the stereo prediction: a = left camera, b = right camera. */
D2FE_API int d2fe_relative_extrinsic(const double* q_a_wxyz, const double* t_a, const double* q_b_wxyz, const double* t_b, double* T_b_a /*[12]*/);
/* The single-call form (what the pipe launches): n_lists point lists, asynchronous on `stream` (a hipStream_t; NULL: the handle's stream), no host synchronisation.
 * List l: points d_pts_xy + l * pts_stride floats as [cap][2], count d_n[l] (read on the device, clamped to 0..cap).  d_bearing [n_lists][cap][3] doubles.
 * T (HOST, [12] row-major 3 x 4; NULL: no prediction) and d_pred_xy [n_lists][cap][2] floats (NULL: no prediction).  The gate's four pointers are given together or all
 * NULL, and need d_pred_xy, T and cam_other: d_other_xy [n_lists][cap][2], d_other_status [n_lists][cap], d_other_bearing [n_lists][cap][3] doubles, d_pred_ok
 * [n_lists][cap].  Every slot >= d_n[l] is written as zero in every output.  D2FE_ERR_INVALID: null arguments, cap outside 1..16384, n_lists outside 1..32767,
 * pts_stride < 2 * cap with more than one list, an unknown kind (2 among them), fx / fy / gamma1 / gamma2 zero or not finite, a cylindrical camera with a non-zero
 * p[4..8], distance or T not finite, gate outputs without d_pred_xy. */
D2FE_API int d2fe_bearings_device(d2fe_handle h, const d2fe_camera* cam, const d2fe_camera* cam_other /*NULL*/, const double* T /*NULL: no prediction*/, double distance,
                                  const float* d_pts_xy, size_t pts_stride, const int32_t* d_n, int n_lists, int cap, double* d_bearing, float* d_pred_xy /*NULL*/,
                                  const float* d_other_xy, const uint8_t* d_other_status, double radius, double* d_other_bearing,
                                  uint8_t* d_pred_ok /* the last four NULL together */, void* stream);
/* The same pass IN THE STEREO / MONO PIPE, switched on by a call before the first submit (d2fe_pipe_config and d2fe_pipe_camera are closed structs; the precedent is
 * d2fe_pipe_flow_enable).  Works with every pipe shape and mode (lr_lk, sp_lk, the flow landmarks incl. superpoint = 0, mono, depth, coalesce), in any order with
 * d2fe_pipe_flow_enable / d2fe_pipe_set_track_params.  Refused (D2FE_ERR_INVALID, the pipe stays as it
 * was and usable): a wrong struct_size, after the first submit, a second time, what d2fe_bearings_device refuses in a camera, distance or T_right_left not finite,
 * radius_lk NaN.  On a mono pipe cam[1], T_right_left and the gate are ignored.
 * Per pass ONE more launch (bearings_kernel, D2FE_PROF_LK) behind the list chain and the left -> right launch, beside the depth launch, in front of the matcher:
 *   left keypoint rows    bearing (cam[0]) and prediction; on an lr_lk pipe without lists also the gate against its left -> right tracks (d2fe_pipe_lk_result)
 *   right keypoint rows   bearing (cam[1]); only pipes that run SuperPoint on both images
 *   list entries          (sp_lk or the flow landmarks) bearing, prediction and the gate against right_xy / right_status
 * With match_lr = 1 and radius_lr > 0 the L <-> R pairs of the matcher take the PREDICTED points as pts_a: the radius gate then is the reference's
 * (track(), d2featuretracker.cpp:666-674: enable_prediction with prediction_using_extrinsic; the comparison feature_matcher.cpp:33 is `>`, under which a NaN
 * prediction keeps the match).  The new arrays sit at the end of the region in front of d2h_words (inside the pass's one D2H); every existing offset, the device views and
 * the exchanges' reads are unchanged, every other result is bit-identical, and a pipe that never enables the mode keeps its layout, allocations and launches.
 * With the caller: the NaN skip, lmanager ids, velocities, lm.depth = (pt3d_norm * dep).norm(), motion prediction from lmanager positions
 * (use_extrinsic = false), check_essential.  The quad pipe has the same pass as d2fe_quad_bearings_enable. */
typedef struct {
  int32_t struct_size;      /* sizeof(d2fe_pipe_bearings), checked strictly */
  int32_t lk_use_pred;      /* lk_lk_use_pred (d2featuretracker.h:62), default 1; 0: pred_ok = status */
  d2fe_camera cam[2];       /* left, right */
  double T_right_left[12];  /* takes a point of the left camera into the right one (d2fe_relative_extrinsic with a = left, b = right) */
  double distance;          /* landmark_distance_assumption, default 100 */
  double radius_lk;         /* search_local_max_dist_lr * width; <= 0: pred_ok = status */
} d2fe_pipe_bearings;
D2FE_API void d2fe_pipe_bearings_default(d2fe_pipe_bearings* b);      /* struct_size, lk_use_pred = 1, distance = 100, T = identity, everything else 0 */
D2FE_API int d2fe_pipe_bearings_enable(d2fe_pipe p, const d2fe_pipe_bearings* b);
/* The bearings of a ticket that d2fe_pipe_wait has returned (D2FE_ERR_NOT_READY before that, D2FE_ERR_UNSUPPORTED on a pipe without the mode).  Whatever the pipe's
 * shape does not produce is NULL. */
typedef struct {            /* HOST pointers into the lane's pinned block, same lifetime as d2fe_pipe_result */
  int32_t frames, cap, cap_tracks, reserved;      /* cap_tracks: of the list the pipe carries (sp_lk or flow), 0 without one */
  const double* kp_bearing;          /* [2 frames][cap][3], the rows of d2fe_pipe_result::kps_xy; rows of images SuperPoint does not see hold zeros */
  const float* kp_pred_xy;           /* [frames][cap][2]: the left keypoints predicted into the right image; NULL on a mono pipe */
  const double* lk_right_bearing;    /* [frames][cap][3]: the lift of d2fe_pipe_lk_result::pts_xy with cam[1]; an lr_lk pipe without lists, NULL otherwise */
  const uint8_t* lk_pred_ok;         /* [frames][cap]: the gate on d2fe_pipe_lk_result::status; NULL as lk_right_bearing */
  const double* list_bearing;        /* [frames][cap_tracks][3], contiguous like right_xy; NULL without a list */
  const float* list_pred_xy;         /* [frames][cap_tracks][2]; NULL without a list or on a mono pipe */
  const double* list_right_bearing;  /* [frames][cap_tracks][3]: the lift of right_xy with cam[1]; NULL as list_pred_xy */
  const uint8_t* list_pred_ok;       /* [frames][cap_tracks]: the gate on right_status; NULL as list_pred_xy */
} d2fe_pipe_bearings_result;
D2FE_API int d2fe_pipe_bearings_result_get(d2fe_pipe p, int64_t ticket, d2fe_pipe_bearings_result* out);

/* Device-side consumers of a ticket's results: the cross-agent exchange (pack -> all-gather -> gate -> remote matching; the reference broadcasts
 * the frame it has just extracted, loop_net.cpp:24-87, d2featuretracker.cpp:237-310) runs on a stream of its OWN, behind the extraction of the ticket and beside the
 * pipe's later passes -- the lanes' convolutions never wait for a collective.
 *   d2fe_pipe_device_view     launches the ticket's pass if coalescing still holds it back, makes `stream` (a hipStream_t, not NULL) wait for the ticket's SuperPoint and
 *                             NetVLAD results (not for its matcher or its D2H) and returns DEVICE pointers into the lane's result block: the same arrays, in the same
 *                             row order, as d2fe_pipe_result.  Read-only.  Valid until the matching release, at most 2 * lanes passes.
 *   d2fe_pipe_device_release  everything queued on `stream` so far is what read the view: the lane's next write of that block waits for it (an event, no host wait).
 * A block whose view has not been released when its lane comes round again (2 * lanes passes later) fails that submit with D2FE_ERR_INVALID (and, like every failed
 * submit, ends the pipe).  Use ONE consumer stream per pipe (the lane waits for the LAST release recorded for a block: consumers on several streams would have to order
 * those streams among themselves).  Both calls may come from a thread other than the submitting one.  Not available with netvlad_group > 1. */
typedef struct {
  int32_t frames, cap, desc_dim, netvlad_dim;
  const float* d_kps_xy;    /* [2 frames][cap][2] */
  const float* d_scores;    /* [2 frames][cap] */
  const float* d_desc;      /* [2 frames][cap][desc_dim] */
  const int32_t* d_n_kp;    /* [2 frames] */
  const float* d_netvlad;   /* [frames][netvlad_dim] or NULL */
} d2fe_pipe_device_result;
/* Where a stream of the CALLER's sits relative to the pipe's streams (same measurement as d2fe_pipe_stream_placement, against one lane stream per class; the pipe must be
 * idle; ~1 ms): *cls = the class it takes turns with, or -1 = none of the classes the lanes use.  A consumer that may choose among several streams (torch.cuda.Stream()
 * hands out pool streams) takes one of class -1, else one that only meets second (NetVLAD) streams. */
D2FE_API int d2fe_pipe_classify_stream(d2fe_pipe p, void* stream, int32_t* cls);
D2FE_API int d2fe_pipe_device_view(d2fe_pipe p, int64_t ticket, void* stream, d2fe_pipe_device_result* out);
D2FE_API int d2fe_pipe_device_release(d2fe_pipe p, int64_t ticket, void* stream);

/* The stream of the lane that ran the ticket's pass (a hipStream_t): work queued on it now runs behind that pass's matcher and D2H and in front of the lane's next
 * pass (lanes - 1 submits later) -- where the cross-agent exchange below goes by default.  d2fe_pipe_geometry / d2fe_pipe_handle: what such a consumer sizes its
 * buffers from, and the handle whose kernels it launches. */
D2FE_API int d2fe_pipe_lane_stream(d2fe_pipe p, int64_t ticket, void** stream);
D2FE_API int d2fe_pipe_geometry(d2fe_pipe p, int32_t* frames, int32_t* cap, int32_t* desc_dim, int32_t* netvlad_dim);
D2FE_API d2fe_handle d2fe_pipe_handle(d2fe_pipe p);

/* ---- Cross-agent exchange behind a pipe -------------------------------------------------------------------------------------
 * Replaces, per submitted stereo frame set: the LCM broadcast of the frame an agent has just extracted (LoopNet::broadcastVisualImageDescArray,
 * d2frontend/src/loop_net.cpp:24-87; wire precision VisualImageDesc::toLCM, d2common/include/d2common/d2frontend_types.h:228-268) and, on every receiver,
 * D2FeatureTracker::trackRemoteFrames (d2frontend/src/d2featuretracker.cpp:237-310: the NetVLAD gate of getMatchedPrevKeyframe :185-203, then matchKNN of the
 * local frame against the remote one).  One sequence per ticket, asynchronous, on ONE stream of the exchange's own (own_stream = 1, the default and the measured best
 * beside a two-lane pipe: profiles/r06_exchange_placement_ab.txt) or on the stream of the lane that produced the ticket (own_stream = 0: no further stream, but that
 * lane's next pass waits for the sequence):
 *   device view of the ticket -> pack one block per left frame (fp32, or the reference's int8 wire form) -> ONE all-gather over the communicator -> [int8: decode
 *   as the receiving constructor does, :319-338] -> counts -> NetVLAD gate of every (local frame f, remote frame f of rank r) pair -> ONE matcher launch (local
 *   descriptors read in place in the lane's result block, remote ones in place in the gathered blocks) -> release of the view -> ONE D2H into pinned slot `slot`.
 * The communicator is an RCCL ncclComm_t made by the caller (ncclCommInitRank in D2SLAM's own start-up code, or d2fe_rccl_comm_init_rank below: librccl is loaded
 * with dlopen, only when these entry points are used); every rank must enqueue its tickets in the same order.  A caller without RCCL (tests over gloo on one GPU)
 * passes comm = NULL and an all_gather callback.  Pair p = (rank-major over the OTHER ranks r, then frame f): local left frame f against frame f of rank r. */
/* D2FE_WIRE_INT8_RENORM256: the int8 wire with every decoded descriptor re-normalised over the row (the pipe's desc_dim floats: 256 without a descriptor PCA, which is
 * where the name comes from) */
typedef enum { D2FE_WIRE_FP32 = 0, D2FE_WIRE_INT8 = 1, D2FE_WIRE_INT8_RENORM256 = 2 } d2fe_wire;
typedef int (*d2fe_all_gather_fn)(void* user, const void* d_send, void* d_recv, size_t bytes_per_rank, void* stream);   /* 0 = ok; must be complete or stream-ordered on return */
typedef struct {
  int32_t struct_size;
  int32_t world, rank;          /* of the communicator */
  int32_t wire;                 /* d2fe_wire: fp32 blocks, the reference's int8 LCM precision (hard-coded 32-float renormalisation), or int8 + 256-float renormalisation */
  int32_t loopback;             /* the rank's OWN gathered blocks count as a remote agent too (how a one-rank communicator exercises the whole sequence) */
  int32_t slots;                /* ring of pinned result slots (>= the exchanges the caller keeps in flight) */
  int32_t own_stream;           /* 1 (default): one stream of the exchange's own; 0: each ticket's sequence on its lane's stream */
  int32_t timing;               /* 1: HIP events around the five phases (d2fe_exchange_result.phase_ms) */
  double gate_thres;            /* track_remote_netvlad_thres (d2featuretracker.cpp:199) */
  double ratio;                 /* knn_match_ratio */
  d2fe_all_gather_fn all_gather; void* all_gather_user;      /* used when the communicator is NULL */
  int32_t reserved[6];
} d2fe_exchange_config;
typedef struct {
  int64_t ticket;
  int32_t npairs, cap;
  const int32_t* q_idx;         /* [npairs][cap] local keypoint index   } host pointers into the pinned slot, valid until the slot is enqueued again */
  const int32_t* t_idx;         /* [npairs][cap] remote keypoint index  } */
  const float* dist;            /* [npairs][cap] */
  const int32_t* n_match;       /* [npairs] */
  const int32_t* gate_pass;     /* [npairs] 1 = the reference would have tracked this pair (NULL without NetVLAD) */
  const float* gate_sims;       /* [npairs] */
  int32_t gate_n;               /* pairs passing the gate */
  float phase_ms[5];            /* timing = 1: pack, all-gather, decode + counts + gate, remote matchKNN, release + D2H */
} d2fe_exchange_result;
typedef struct d2fe_exchange_s* d2fe_exchange;
D2FE_API void d2fe_exchange_default_config(d2fe_exchange_config* c);
D2FE_API int d2fe_exchange_create(d2fe_pipe p, void* nccl_comm, const d2fe_exchange_config* cfg, d2fe_exchange* out);
D2FE_API void d2fe_exchange_destroy(d2fe_exchange x);      /* before the pipe */
D2FE_API int d2fe_exchange_enqueue(d2fe_exchange x, int64_t ticket, int slot);       /* asynchronous; within 2 * lanes passes of the ticket's submit */
D2FE_API int d2fe_exchange_collect(d2fe_exchange x, int slot, d2fe_exchange_result* out);      /* blocks until the slot's results are in host memory */
D2FE_API int d2fe_exchange_pairs(d2fe_exchange x);
D2FE_API int d2fe_exchange_block_bytes(d2fe_exchange x);   /* bytes one frame contributes to the all-gather */
D2FE_API void* d2fe_exchange_stream(d2fe_exchange x);      /* own_stream = 1: that stream (hipStream_t), else NULL */
/* DEVICE addresses of slot `slot`'s gathered blocks [world][frames]: the fp32 blocks the gate and the matcher read (decoded from the wire form when it is int8) and
 * the blocks as they crossed the wire (either pointer may be NULL); d2fe_quad_exchange_gathered's contract.  What d2fe_window_track_device reads in place.
 * The blocks take the pipe's descriptor width (d2fe_pipe_geometry): their size and fields are d2fe_block_words_d / d2fe_block_field_offset_d(cap, desc_dim, G, ...). */
D2FE_API int d2fe_exchange_gathered(d2fe_exchange x, int slot, const float** d_blocks, const void** d_wire_blocks);
/* RCCL without any other dependency: rank 0 makes a 128-byte id, every rank gets it by whatever channel D2SLAM has (its LCM bus, a file, MPI), then all ranks call
 * comm_init_rank.  path: a librccl to load (NULL: one the process already holds, else librccl.so.1 / librccl.so on the loader path, else /opt/rocm/lib). */
D2FE_API int d2fe_rccl_load(const char* path);
D2FE_API const char* d2fe_rccl_path(void);
D2FE_API int d2fe_rccl_unique_id(void* id128);
D2FE_API int d2fe_rccl_comm_init_rank(const void* id128, int world, int rank, int device, void** comm_out);
D2FE_API int d2fe_rccl_comm_destroy(void* comm);

/* Half-image filter for quadcam neighbour matching.  Replaces getFeatureHalfImg
 * (d2featuretracker.cpp:1051-1075): map[c] = source index of the c-th kept keypoint; returns count in *n_out. */
D2FE_API int d2fe_half_image_filter(const float* pts_xy, int n, int require_left, int width_undistort,
                                    double undistort_fov, int32_t* map, int* n_out);

/* A1, variant A / NetVLAD image prep.  Replaces the cv::cvtColor(COLOR_BGR2GRAY) + cv::resize(INTER_LINEAR) block in front of
 * SuperPointONNX::infer and MobileNetVLADONNX::inference (superpoint_onnx.cpp:76-83, mobilenetvlad_onnx.h:51-59): channels = 1
 * (gray) or 3 (BGR, interleaved); the output is dw x dh gray u8, tight rows.  Same size and 1 channel = a copy.  Fused, one
 * pass; OpenCV's 8-bit fixed-point arithmetic (incl. its silent INTER_AREA for an exact 2x decimation). */
D2FE_API int d2fe_prepare_gray(d2fe_handle h, const uint8_t* src, int channels, int sw, int sh, int sstride, int dw, int dh,
                               uint8_t* dst);
D2FE_API int d2fe_prepare_gray_device(d2fe_handle h, const uint8_t* d_src, int n, int channels, int sw, int sh, int sstride,
                                      size_t src_image_stride, int dw, int dh, uint8_t* d_dst, void* stream);

/* ---- the components either side of the hot path --------------------------------------------------
 * (f)-1 Fisheye undistort + photometric gain.  Replaces FisheyeUndist::undist_id_cuda
 * (d2common/include/d2common/fisheye_undistort.h:152-176: cv::cuda::remap(INTER_LINEAR, constant 0 border) -> convertTo(32F)
 * -> cv::cuda::multiply(gain) -> convertTo(8U)) by one fused kernel.  mapx/mapy: dh*dw floats (source coordinates, the
 * reference's undistMapsGPUX/Y); gain: dh*dw floats or NULL.  Host-pointer form and device-resident form (n frames
 * sharing the maps, frame i at d_src + i*src_image_stride, output i at d_dst + i*dh*dw). */
D2FE_API int d2fe_undistort(d2fe_handle h, const uint8_t* src, int sw, int sh, int sstride, const float* mapx,
                            const float* mapy, const float* gain, int dw, int dh, uint8_t* dst);
D2FE_API int d2fe_undistort_device(d2fe_handle h, const uint8_t* d_src, int n, int sw, int sh, int sstride,
                                   size_t src_image_stride, const float* d_mapx, const float* d_mapy, const float* d_gain,
                                   int dw, int dh, uint8_t* d_dst, void* stream);

/* (f)-1, map generation.  FisheyeUndist::generateCylinderMap + genOneUndistMap (fisheye_undistort.h:458-500,559-613): a
 * virtual camodocal::CylindricalCamera (fx = fy = width / (fov_deg * pi/180), cx = width/2, cy = height/2) is lifted
 * (CylindricalCamera.cc:207-220) and projected through the fisheye model; the pinhole form is the other genOneUndistMap
 * (:615-660, the five virtual cameras of generateAllUndistMap :346-456): objPoint = q * (x - width/2, y - height/2, f).
 * The fisheye model is camodocal's CataCamera ("omni" + "radtan" in config/quadcam/quad_cam_calib-*.yaml; spaceToPlane
 * CataCamera.cc:495-515).  Maps are width*height floats each, written to HBM (device form) or copied back (host form). */
typedef struct {
  double xi, k1, k2, p1, p2, gamma1, gamma2, u0, v0;   /* kalibr order: intrinsics [xi fu fv pu pv], distortion [k1 k2 p1 p2] */
} d2fe_mei_camera;
D2FE_API int d2fe_gen_cylinder_map(d2fe_handle h, const d2fe_mei_camera* cam, int width, int height, double fov_deg,
                                   float* mapx, float* mapy);
D2FE_API int d2fe_gen_cylinder_map_device(d2fe_handle h, const d2fe_mei_camera* cam, int width, int height, double fov_deg,
                                          float* d_mapx, float* d_mapy, void* stream);
D2FE_API int d2fe_gen_pinhole_map(d2fe_handle h, const d2fe_mei_camera* cam, const double* q_wxyz, int width, int height,
                                  double f, float* mapx, float* mapy);
D2FE_API int d2fe_gen_pinhole_map_device(d2fe_handle h, const d2fe_mei_camera* cam, const double* q_wxyz, int width, int height,
                                         double f, float* d_mapx, float* d_mapy, void* stream);

/* (f)-2 NetVLAD keyframe database.  Replaces faiss::IndexFlatIP (members d2frontend/include/d2frontend/loop_detector.h:71-72;
 * add d2frontend/src/loop_detector.cpp:254-263; search :318) and the gate of LoopDetector::queryIndexFromDatabase
 * (:300-350).  Vectors live in HBM; a search is one streaming pass over the database. */
typedef struct d2fe_db* d2fe_db_handle;
D2FE_API int d2fe_db_create(d2fe_handle h, int dim, int capacity, d2fe_db_handle* out);
D2FE_API void d2fe_db_destroy(d2fe_db_handle db);
D2FE_API int d2fe_db_ntotal(d2fe_db_handle db);
D2FE_API int d2fe_db_add(d2fe_db_handle db, const float* vecs, int n);        /* IndexFlatIP::add; returns first new label or <0 */
/* IndexFlatIP::search(nq, q, k, sims, labels): k best by inner product, descending (ties: lower label); -1 pads. */
D2FE_API int d2fe_db_search(d2fe_db_handle db, const float* q, int nq, int k, float* sims, int32_t* labels);
/* queryIndexFromDatabase (loop_detector.cpp:300-350) minus the ROS bookkeeping: k = min(5 + max_index, ntotal) nearest;
 * the first with label <= ntotal - max_index and similarity > thres is returned in *label (else -1) with its similarity. */
D2FE_API int d2fe_db_query_gated(d2fe_db_handle db, const float* q, int max_index, double thres, int32_t* label, float* sim);

/* (f)-3 int8 wire codec.  Replaces the quantisation in VisualImageDesc::toLCM (d2common/include/d2common/d2frontend_types.h:
 * 228-237 landmark descriptors, float max; 260-268 NetVLAD, double max: pass double_max = 1) and the decode of the LCM
 * constructor (:313-351): x = q/127.0; landmark_num >= 0: the first landmark_num 32-float segments are re-normalised
 * (the reference's hard-coded 32); landmark_num < 0: whole-vector L2 (global descriptor).  An all-zero tensor encodes to
 * zeros (the reference divides 0 by 0 there); an all-zero segment or vector decodes to zeros (Eigen's normalize()). */
D2FE_API int d2fe_quantize_int8(d2fe_handle h, const float* x, int n, int double_max, int8_t* out);
D2FE_API int d2fe_dequantize_int8(d2fe_handle h, const int8_t* q, int n, int landmark_num, float* out);

/* (f)-4 LK optical-flow tracker (d2frontend/src/opticaltrack_utils.cpp).  A d2fe_lk_frame is the device-resident image
 * pyramid the reference keeps in LKImageInfoGPU::pyr (opticaltrack_utils.h:16-23): level 0 = the gray frame, level l+1 =
 * cv::cuda::pyrDown(level l) (buildImagePyramid, opticaltrack_utils.cpp:526-542; PYR_LEVEL = 2, opticaltrack_utils.h:10). */
typedef struct d2fe_lk_frame_s* d2fe_lk_frame;
D2FE_API int d2fe_lk_frame_create(d2fe_handle h, const uint8_t* gray, int width, int height, int stride, int levels,
                                  d2fe_lk_frame* out);
D2FE_API int d2fe_lk_frame_create_device(d2fe_handle h, const uint8_t* d_gray, int width, int height, int stride, int levels,
                                         void* stream, d2fe_lk_frame* out);
D2FE_API void d2fe_lk_frame_destroy(d2fe_lk_frame f);
/* copy pyramid level `level` (tight rows) to the host; returns bytes or <0 */
D2FE_API long d2fe_lk_frame_read_level(d2fe_lk_frame f, int level, uint8_t* dst, size_t max_bytes, int* width, int* height);
/* The tracking block of opticalflowTrackPyr (opticaltrack_utils.cpp:236-272) in one launch: SparsePyrLKOpticalFlow(win, levels,
 * iters, useInitialFlow).calc(prev, cur) from cur_init, reverse calc(cur, prev) from the result shifted back by move_cols
 * (type 1 LEFT_RIGHT_IMG_MATCH: -move_cols, 2 RIGHT_LEFT_IMG_MATCH: +move_cols, 0 WHOLE_IMG_MATCH: none), status[i] = both
 * succeeded && |prev - reverse| <= 0.5 && inBorder(cur) (:35-41).  cur_pts[n][2] and status[n] are written for every point;
 * the reduceVector() compaction stays with the caller.  Reference constants: win 21 (WIN_SIZE, :25), iters 30 (:239). */
D2FE_API int d2fe_lk_track(d2fe_handle h, d2fe_lk_frame prev, d2fe_lk_frame cur, const float* prev_pts, const float* cur_init,
                           int n, int type, float move_cols, int win, int iters, float* cur_pts, uint8_t* status);
/* Batched form: all the tracks of one frame set in ONE launch and one H2D/D2H pair (quadcam: 4 temporal tracks + the
 * left/right neighbour tracks of trackLK, d2featuretracker.cpp:472-621).  Points are concatenated; pair p owns points
 * [first, first + count); every point must belong to exactly one pair. */
typedef struct {
  d2fe_lk_frame prev, cur;
  int32_t first, count;
  int32_t type;          /* 0 WHOLE_IMG_MATCH, 1 LEFT_RIGHT_IMG_MATCH, 2 RIGHT_LEFT_IMG_MATCH */
  float move_cols;
} d2fe_lk_pair;
D2FE_API int d2fe_lk_track_batch(d2fe_handle h, const d2fe_lk_pair* pairs, int npairs, const float* prev_pts,
                                 const float* cur_init, int n_total, int win, int iters, float* cur_pts, uint8_t* status);
/* The stereo tracks of trackLK (d2featuretracker.cpp:697-752) for callers of d2fe_superpoint_extract_device, and what a pipe with lr_lk = 1 runs: the pyramids of
 * n_frames left and n_frames right gray frames that are already in HBM (frame f at d_left / d_right + f * image_stride, rows `stride` bytes apart) are built in
 * d_workspace (d2fe_lk_stereo_workspace_bytes: 2 * n_frames pyramids in the layout of a d2fe_lk_frame, no padding) and keypoint i < d_n_kp[f] of left frame f,
 * d_kps_xy[f][i], is tracked into right frame f exactly as d2fe_lk_track(left, right, pts, pts, n, WHOLE_IMG_MATCH, 0, win, iters) does (same bits).
 * d_pts_xy [n_frames][cap][2] and d_status [n_frames][cap] are written for EVERY slot (i >= d_n_kp[f]: status 0, point (0, 0)).  Points and counts are read on
 * the device: the call only enqueues on `stream` (NULL: the handle's stream) -- max(levels, 1) + 1 launches whatever n_frames is, no allocation, no
 * synchronisation.  Parameter ranges as d2fe_lk_track_batch (win odd 3..23, levels 0..7, iters >= 1).  d2fe_lk_stereo_workspace_bytes is host arithmetic
 * (no GPU needed; 0 for a geometry the call would refuse). */
D2FE_API size_t d2fe_lk_stereo_workspace_bytes(int n_frames, int width, int height, int levels);
D2FE_API int d2fe_lk_track_stereo_device(d2fe_handle h, const uint8_t* d_left, const uint8_t* d_right, int n_frames, int width, int height, int stride,
                                         size_t image_stride, const float* d_kps_xy /*[n_frames][cap][2]*/, const int32_t* d_n_kp /*[n_frames]*/, int cap,
                                         int levels, int win, int iters, void* d_workspace, float* d_pts_xy, uint8_t* d_status, void* stream);
/* d_kps_xy, d_n_kp, d_pts_xy and d_status all NULL (cap ignored): the pyramids alone, max(levels, 1) launches -- the workspace of d2fe_lk_carry_step_device. */

/* The LK-carried landmark list of sp_track_use_lk (D2FeatureTracker::trackLK(frame), d2featuretracker.cpp:472-621) for ONE camera and ONE frame, on the device:
 *   a. every entry i < n of the previous list is tracked from the previous pyramid to the current one: opticalflowTrackPyr(..., WHOLE_IMG_MATCH)
 *      (opticaltrack_utils.cpp:173-279; cur_init = prev_pts, forward, reverse, 0.5 px round trip, inBorder) -- the bits of d2fe_lk_track(prev, cur, pts, pts, n, 0, 0, win, iters);
 *   b. order-preserving compaction by status (reduceVector, :273-276);
 *   c. removeNearPoints(info, near_lk_thread_rate) (opticaltrack_utils.h:61-89): greedy, in order, an entry is dropped when an earlier KEPT entry is nearer than the
 *      threshold; distance as cv::norm(Point2f): float difference, squares and sqrt in double, `<` against the float threshold widened to double;
 *   d. replenish (d2featuretracker.cpp:556-589) over the frame's SuperPoint keypoints i = 0 .. n_kp - 1 in list order: stop when n > total_feature_num (strict: the list
 *      can reach total_feature_num + 1 = cap_tracks), skip keypoint i if ANY current entry (those appended in this loop included) is nearer than feature_min_dist (a
 *      double), otherwise append it with id = next_id++, src = -1, kp = i and its SuperPoint descriptor row and score;
 *   e. a tracked entry keeps its id, src = its index in the previous list, kp = -1, descriptor and score carried from the previous list (:509-521).
 * A previous list with n = 0 (the first frame) skips a-c.  ONE launch: one wave per entry tracks, the last workgroup to finish does b-e.
 * A LIST is one block of d2fe_lk_carry_list_bytes(cap_tracks, desc_dim) bytes (host arithmetic; 0 for cap_tracks outside 1..1024 or desc_dim < 1), 32-bit words, every
 * array on a 64-word boundary, d2fe_lk_carry_list_offset(cap_tracks, desc_dim, field) words from its base (-1: bad field):
 *   D2FE_LKC_HDR     int32[64]: [0] n, [1] n_tracked_in (the previous list's n), [2] n_lost, [3] n_removed_near, [4] n_new, [5] the launch's arrival counter (0 between
 *                    launches), [6] next_id after this frame, rest 0
 *   D2FE_LKC_PTS     float[cap_tracks][2]      D2FE_LKC_ID / _SRC / _KP   int32[cap_tracks]      D2FE_LKC_SCORES  float[cap_tracks]
 *   D2FE_LKC_DESC    float[cap_tracks][desc_dim]
 *   D2FE_LKC_TRK_XY  float[cap_tracks][2], D2FE_LKC_TRK_STATUS uint8[cap_tracks]: step a's raw result for the PREVIOUS list's entries (before b)
 * Slots >= n of every array are written as zeros.  A block must be ZERO once before its first use as d_cur_list (the arrival counter; the launch leaves it zero), and
 * an all-zero block is the empty list.  d_prev_list != d_cur_list; the previous list's cap_tracks / desc_dim are this call's.  The pyramids are in the layout of a
 * d2fe_lk_frame / one image of the d2fe_lk_track_stereo_device workspace (tp->levels + 1 levels, no padding).  d_kps_xy [kp_cap][2], d_kp_scores [kp_cap],
 * d_kp_desc [kp_cap][desc_dim], d_n_kp [1]: the outputs of d2fe_superpoint_extract_device for the current frame (n_kp is clamped to kp_cap; kp_cap = 0: none).
 * d_next_id: one int32 in device memory, read and advanced by the launch.  Everything is read on the device: the call only enqueues on `stream` (NULL: the handle's
 * stream) -- no allocation, no synchronisation, no memset.  D2FE_ERR_INVALID: total_feature_num outside 0..1023, thresholds < 0 or NaN, LK parameters outside the
 * ranges of d2fe_lk_track_batch, bad geometry. */
typedef struct d2fe_track_params_s {
  int32_t total_feature_num;      /* 150   max_cnt (d2frontend_params.cpp:62) */
  int32_t levels, win, iters;     /* 2, 21, 30   PYR_LEVEL, WIN_SIZE, opticaltrack_utils.cpp:239 */
  float near_lk_thread_rate;      /* 5.0   d2featuretracker.h:69 */
  int32_t reserved;               /* zero */
  double feature_min_dist;        /* 20    d2frontend_params.h:65 */
} d2fe_track_params;
enum { D2FE_LKC_HDR = 0, D2FE_LKC_PTS, D2FE_LKC_ID, D2FE_LKC_SRC, D2FE_LKC_KP, D2FE_LKC_SCORES, D2FE_LKC_DESC, D2FE_LKC_TRK_XY, D2FE_LKC_TRK_STATUS, D2FE_LKC_FIELDS };
D2FE_API void d2fe_track_default_params(d2fe_track_params* tp);
D2FE_API size_t d2fe_lk_carry_list_bytes(int cap_tracks, int desc_dim);
D2FE_API long d2fe_lk_carry_list_offset(int cap_tracks, int desc_dim, int field);
D2FE_API int d2fe_lk_carry_step_device(d2fe_handle h, const uint8_t* d_prev_pyr, const uint8_t* d_cur_pyr, int width, int height, const void* d_prev_list,
                                       void* d_cur_list, int desc_dim, const float* d_kps_xy, const float* d_kp_scores, const float* d_kp_desc,
                                       const int32_t* d_n_kp, int kp_cap, const d2fe_track_params* tp, int32_t* d_next_id, void* stream);
/* The quadcam forms (trackLocalFrames with sp_track_use_lk, d2featuretracker.cpp:121-133).
 * d2fe_lk_carry_quad_step_device: the lists of the FOUR cameras of one quad frame in ONE launch of (cap_tracks / 4, 4) workgroups.  Camera c's previous / current list
 * is c * list_stride 32-bit words behind d_prev_lists / d_cur_lists (list_stride >= one list block), its previous / current pyramid c * pyr_stride bytes behind
 * d_prev_pyr / d_cur_pyr, its keypoints row c of the dense d_kps_xy [4][kp_cap][2], d_kp_scores [4][kp_cap], d_kp_desc [4][kp_cap][desc_dim], d_n_kp [4] (the rows of
 * one quad frame of d2fe_quad_device_result).  Every bit of the four lists and of *d_next_id equals four d2fe_lk_carry_step_device calls for cameras 0, 1, 2, 3 in
 * that order with the same d_next_id: a new entry's id is next_id + the new entries of the lower cameras + its rank among its own camera's new entries, whichever
 * camera's workgroups finish last.  The block-zero rule holds per list: besides word 5 of every header the launch uses header word 7 of CAMERA 0's current list
 * as its quad-level arrival counter, and leaves it zero.  No current list may overlap a previous one.  Only enqueues.
 * d2fe_lk_carry_neighbour_device: trackLK(left, right, type) (:697-752) of the four neighbour pairs (0,1) (1,2) (2,3) LEFT_RIGHT_IMG_MATCH, (0,3) RIGHT_LEFT_IMG_MATCH
 * of `quads` quad frames in ONE launch, over lists that are on the device: list and pyramid of view (q, v) are (q * 4 + v) * list_stride words / pyr_stride bytes
 * behind d_lists / d_pyr.  One wave per (q, pair, slot i of list a): the gate and shift of opticaltrack_utils.cpp:195-223 with move_cols =
 * d2fe_half_move_cols(width, undistort_fov), then forward a -> b, reverse from the result shifted back, the 0.5 px test and inBorder.  d_nb_xy [quads][4][cap_tracks][2]
 * and d_nb_status [quads][4][cap_tracks] are written for EVERY slot: i >= n or an entry the gate rejects -> (0, 0), status 0; an eligible entry -> exactly what
 * d2fe_lk_track(a, b, pt, pt +- move_cols, 1, type, move_cols, win, iters) returns for it.  Only enqueues. */
D2FE_API int d2fe_lk_carry_quad_step_device(d2fe_handle h, const uint8_t* d_prev_pyr, const uint8_t* d_cur_pyr, size_t pyr_stride, int width, int height,
                                            const void* d_prev_lists, void* d_cur_lists, size_t list_stride, int desc_dim, const float* d_kps_xy,
                                            const float* d_kp_scores, const float* d_kp_desc, const int32_t* d_n_kp, int kp_cap, const d2fe_track_params* tp,
                                            int32_t* d_next_id, void* stream);
D2FE_API int d2fe_lk_carry_neighbour_device(d2fe_handle h, const uint8_t* d_pyr, size_t pyr_stride, int quads, int width, int height, double undistort_fov,
                                            const void* d_lists, size_t list_stride, int desc_dim, const d2fe_track_params* tp, float* d_nb_xy,
                                            uint8_t* d_nb_status, void* stream);
/* The FLOW landmarks (enable_lk_optical_flow without sp_track_use_lk; the whole front end of config/gopro/gopro.yaml and config/visensor_f9p/visensor_f9p.yaml, which
 * set max_superpoint_cnt: 0) for ONE camera and ONE frame, on the device: the second list D2FeatureTracker::trackLK(frame) (d2featuretracker.cpp:472-621) keeps.
 *   a-c. as d2fe_lk_carry_step_device (the same device code): track every entry of the previous list, reduceVector, removeNearPoints; m entries survive;
 *   d.   detectPoints(img, n_pts, cur_pts, require = total_feature_num, ..., use_fast = true) (opticaltrack_utils.cpp:375-442) with cur_pts = landmarks2D() = the frame's
 *        SuperPoint keypoints kps[0 .. n_kp) followed by the m tracked entries: lack = total_feature_num - (n_kp + m); only if lack > total_feature_num / 4 (integer
 *        division, strict) num = lack, doubled when n_kp + m > 0, candidates = detectFastByRegion(img, num, cols = fast_cols, rows = fast_rows) at fast_threshold in the
 *        order d2fe_detect_fast_by_region fixes (response descending, region-major raster order ascending); a candidate is skipped when cv::norm(candidate - q) <
 *        feature_min_dist (float difference, squares and sqrt in double) for any q of cur_pts or any candidate accepted before it; stop at `lack` accepted;
 *   e.   the new list = the m tracked entries (id kept, src = index in the previous list), then the accepted candidates (id = next_id++, src = -1).  The SuperPoint
 *        keypoints only block candidates, they are not in the list; n <= total_feature_num.
 * The LIST is a block of d2fe_lk_flow_list_bytes(cap_tracks) bytes, cap_tracks = max(total_feature_num, 1) (0 outside 1..1024), laid out by the rules of the carry list
 * with the fields a flow entry has: d2fe_lk_flow_list_offset(cap_tracks, field) for D2FE_LKC_HDR, _PTS, _ID, _SRC, _TRK_XY, _TRK_STATUS; -1 for _KP, _SCORES, _DESC and
 * a bad field.  Header words 0-6 as in the carry list ([0] n, [1] n_tracked_in, [2] n_lost, [3] n_removed_near, [4] n_new, [5] arrival counter, [6] next_id after this
 * frame), then [7] lack, [8] num (0: the frame did not detect), [9] the candidates that reached the merge (min(num, what FAST found)); rest 0.  The zero-once rule, the
 * all-zero empty list and d_prev_list != d_cur_list hold as there.  d2fe_flow_params.superpoint = 0 (flow only): the keypoint arguments are ignored, n_kp = 0.
 * d_scratch: d2fe_lk_flow_scratch_bytes(width, height, cap_tracks, fast_cols, fast_rows) bytes, 16-byte aligned (host arithmetic, 0 for what the call refuses): the
 * score map and the candidate pool for num up to 2 * cap_tracks; its content between calls does not matter.
 * FIVE launches per frame whatever the list holds -- (1) track + b-c + the decision in the last workgroup to arrive, (2) score-map clear, (3) FAST scores, (4) non-max,
 * (5) selection + merge + new entries -- of which 2-5 read `num` from the header and return at once when it is 0.  Everything is read on the device: the call only
 * enqueues on `stream` (NULL: the handle's stream), no allocation, no synchronisation.  D2FE_ERR_INVALID: what d2fe_lk_carry_step_device refuses, fast_cols * fast_rows
 * outside 1..64, a region (width / fast_cols) x (height / fast_rows) below 7 x 7, fast_threshold outside 0..254, a struct_size that is not this header's.
 *
 * d2fe_detect_fast_device: detectFastByRegion without the host, launches 2-4 and the selection alone (FOUR launches): level 0 of the pyramid at d_pyr, `features` read
 * from ONE int32 in device memory and clamped to 2 * cap_tracks (what the scratch holds); d_xy [cap][2], d_response [cap] (may be NULL) and d_n [1] receive
 * min(features, found, cap) candidates in the order and with the bits of d2fe_detect_fast_by_region.  features <= 0: d_n = 0, nothing else is written, every kernel
 * returns at once.  The host sort is an exact selection on a unique key of 40 significant bits (the response in bits 32..39 -- a FAST score is at most 254 -- above ~order in
 * bits 0..31; five 8-bit passes cover bits 0..39), correct for any candidate count up to cols * rows * features. */
typedef struct d2fe_flow_params_s {
  int32_t struct_size;            /* sizeof(d2fe_flow_params), checked strictly */
  int32_t superpoint;             /* 1: beside SuperPoint (its keypoints block candidates); 0: flow only (max_superpoint_cnt: 0) */
  d2fe_track_params track;        /* total_feature_num = max_cnt, levels, win, iters, near_lk_thread_rate, feature_min_dist */
  int32_t fast_cols, fast_rows;   /* 3, 4   the detector's cols / rows: the reference hands fast_rows = 3 to the parameter named cols (opticaltrack_utils.cpp:394-396) */
  int32_t fast_threshold;         /* 10    opticaltrack_utils.cpp:451-452 */
  int32_t reserved;               /* zero */
} d2fe_flow_params;
D2FE_API void d2fe_flow_default_params(d2fe_flow_params* fp);
D2FE_API size_t d2fe_lk_flow_list_bytes(int cap_tracks);
D2FE_API long d2fe_lk_flow_list_offset(int cap_tracks, int field);
D2FE_API size_t d2fe_lk_flow_scratch_bytes(int width, int height, int cap_tracks, int cols, int rows);
D2FE_API int d2fe_detect_fast_device(d2fe_handle h, const uint8_t* d_pyr, int width, int height, const int32_t* d_features, int cap_tracks, int cols, int rows,
                                     int threshold, float* d_xy, int32_t* d_response, int cap, int32_t* d_n, void* d_scratch, void* stream);
D2FE_API int d2fe_lk_flow_step_device(d2fe_handle h, const uint8_t* d_prev_pyr, const uint8_t* d_cur_pyr, int width, int height, const void* d_prev_list,
                                      void* d_cur_list, const float* d_kps_xy, const int32_t* d_n_kp, int kp_cap, const d2fe_flow_params* fp, int32_t* d_next_id,
                                      void* d_scratch, void* stream);
/* The quadcam forms of the flow landmarks (trackLocalFrames WITHOUT sp_track_use_lk, d2featuretracker.cpp:121-133: config/quadcam/quadcam_single.yaml, quadcam_multi.yaml,
 * quadcam_multi_rt.yaml).
 * d2fe_lk_flow_quad_step_device: the flow lists of the FOUR cameras of one quad frame in FIVE launches, whatever the lists hold.  The addressing of
 * d2fe_lk_carry_quad_step_device: camera c's previous / current list is c * list_stride 32-bit words behind d_prev_lists / d_cur_lists (list_stride >= one flow list
 * block), its previous / current pyramid c * pyr_stride bytes behind d_prev_pyr / d_cur_pyr, its keypoints row c of the dense d_kps_xy [4][kp_cap][2] and d_n_kp [4] (the
 * rows of one quad frame of d2fe_quad_device_result), its detector scratch c * scratch_stride bytes behind d_scratch (scratch_stride a multiple of 16 and >=
 * d2fe_lk_flow_scratch_bytes(...)): a score map, a candidate pool and a count of its own per camera.
 *   (1) grid (cap_tracks / 4, 4): one wave per entry of camera blockIdx.y's previous list; the camera's last workgroup (ticket: header word 5 of ITS current list)
 *       finishes its list and decides its `lack` and `num`;
 *   (2)-(4) score-map clear, FAST scores, non-max with the camera as a grid dimension: every camera reads its OWN `num` and returns when it is 0;
 *   (5) four workgroups, one per camera: selection and merge of that camera; the four then take a quad-level ticket -- header word 10 of CAMERA 0's current list, one
 *       of the "rest 0" words of a flow header, zero between launches like word 5 -- and the last one hands the ids out.
 * A camera whose `num` is 0 adds nothing but keeps its place in the order; when all four are 0 (the steady state) launches 2-5 return at once.  Every byte of the
 * four list blocks and *d_next_id equal four d2fe_lk_flow_step_device calls for cameras 0, 1, 2, 3 in that order with the same d_next_id: camera c's k-th new entry
 * gets next_id + (new entries of cameras < c) + k, header word 6 of camera c is next_id after that camera, whichever workgroups finish last.  Only enqueues: no
 * allocation, no synchronisation, no memset.  D2FE_ERR_INVALID: what d2fe_lk_flow_step_device refuses, strides too small or misaligned, a current list overlapping a
 * previous one.
 * d2fe_lk_flow_neighbour_device: d2fe_lk_carry_neighbour_device (the same kernel) over FLOW lists: cap_tracks = max(tp->total_feature_num, 1), list_stride >= one flow
 * list block; d_nb_xy [quads][4][cap_tracks][2] and d_nb_status [quads][4][cap_tracks] are written for every slot.  ONE launch, only enqueues. */
D2FE_API int d2fe_lk_flow_quad_step_device(d2fe_handle h, const uint8_t* d_prev_pyr, const uint8_t* d_cur_pyr, size_t pyr_stride, int width, int height,
                                           const void* d_prev_lists, void* d_cur_lists, size_t list_stride, const float* d_kps_xy, const int32_t* d_n_kp, int kp_cap,
                                           const d2fe_flow_params* fp, int32_t* d_next_id, void* d_scratch, size_t scratch_stride, void* stream);
D2FE_API int d2fe_lk_flow_neighbour_device(d2fe_handle h, const uint8_t* d_pyr, size_t pyr_stride, int quads, int width, int height, double undistort_fov,
                                           const void* d_lists, size_t list_stride, const d2fe_track_params* tp, float* d_nb_xy, uint8_t* d_nb_status, void* stream);
/* The flow landmarks IN THE STEREO / MONO PIPE. d2fe_pipe_config and d2fe_pipe_camera are closed structs, so the mode is switched on by a call before the first
 * submit (as d2fe_quad_track_enable does for the quad pipe): d2fe_pipe_flow_enable(p, fp) (fp NULL: d2fe_flow_default_params).  It needs a pipe that builds
 * pyramids (lr_lk = 1 or mono = 1), is refused with sp_lk (the reference's two branches exclude each other, d2featuretracker.cpp:556-614), after the first submit, for
 * fp->track.levels != 2, for what d2fe_lk_flow_step_device refuses, and with fp->superpoint = 0 on a pipe created with netvlad or match_prev; a refusal
 * (D2FE_ERR_INVALID) leaves the pipe as it was and usable.  Per left frame of a pass ONE d2fe_lk_flow_step_device (five launches, D2FE_PROF_LK) in time order behind the
 * pass's pyramids, on the chain sp_lk uses: the previous list is read where the previous pass left it, the last pyramid is carried in a pipe-owned copy, the lanes
 * wait for each other's chain event, ids come from the pipe's one counter; one pipe-owned detector scratch serves all lanes because the chain serialises the steps.
 * On a stereo pipe ONE more launch tracks the flow entries of all frames of the pass left -> right (trackLK(left, right), :697-752); the per-keypoint launch of lr_lk
 * stays.  superpoint = 0 (gopro.yaml / visensor_f9p.yaml): a pass launches neither network and no matcher, every n_kp row stays 0 on the device too; the lanes'
 * activation buffers stay allocated (freeing them needs a create-time switch the closed structs do not have).  With depth the pass's one depth_gather_kernel launch
 * takes one more segment over the flow lists.  The lists [frames * coalesce], the right tracks and the depth values sit in front of d2h_words, inside the pass's one
 * D2H; a pipe that never enables the mode keeps its layout, allocations, launches and results.  d2fe_pipe_flow_result_get (after d2fe_pipe_wait; D2FE_ERR_UNSUPPORTED on
 * a pipe without the mode): the pointers address frame 0 of the ticket; frame f's list arrays are f * list_words 32-bit words further, right_xy [frames][cap_tracks][2],
 * right_status and depth_mm [frames][cap_tracks] are dense (NULL on a mono pipe / without depth). */
typedef struct {
  int32_t frames, cap_tracks, list_words, reserved;
  const int32_t *n, *n_tracked_in, *n_lost, *n_removed_near, *n_new, *lack, *num, *n_cand;
  const float* pts_xy;             /* [cap_tracks][2] */
  const int32_t *id, *src;         /* [cap_tracks] */
  const float* right_xy; const uint8_t* right_status;
  const uint16_t* depth_mm;
} d2fe_pipe_flow_result;
D2FE_API int d2fe_pipe_flow_enable(d2fe_pipe p, const d2fe_flow_params* fp);
D2FE_API int d2fe_pipe_flow_result_get(d2fe_pipe p, int64_t ticket, d2fe_pipe_flow_result* out);
/* detectFastByRegion (opticaltrack_utils.cpp:444-493): cv::cuda::FastFeatureDetector(threshold, nonmax, TYPE_9_16,
 * max_npoints = features) on each of the cols x rows regions of level 0, sorted by response, top `features`.
 * response (optional) receives the FAST scores. */
D2FE_API int d2fe_detect_fast_by_region(d2fe_handle h, d2fe_lk_frame f, int features, int cols, int rows, int threshold,
                                        float* pts_xy, int32_t* response, int cap, int* n_out);
/* cv::cuda::createGoodFeaturesToTrackDetector(type, max_corners, quality, min_dist)->detect (detectPoints,
 * opticaltrack_utils.cpp:404-412): min-eigenvalue corners (blockSize 3, Sobel 3), eig > quality * max, 3x3 local maxima,
 * sorted by eigenvalue, host min-distance grid filter. */
D2FE_API int d2fe_good_features_to_track(d2fe_handle h, d2fe_lk_frame f, int max_corners, double quality, double min_dist,
                                         float* pts_xy, int cap, int* n_out);

/* ---- cross-agent exchange --------------------------------------------------------------------------------
 * Replaces the LCM broadcast of a keyframe's image descriptor (d2frontend/src/loop_net.cpp:24-87: landmark positions, scores,
 * SuperPoint descriptors, NetVLAD descriptor) by one fixed-capacity block per frame, so that the exchange is ONE all-gather:
 *   block (float words) = desc[cap][D] | kps[cap][2] | scores[cap] | netvlad[G] | n (int32) | zero padding to a multiple of 256.
 * Descriptors come first and the size is a multiple of 256 words: a gathered block's descriptors are addressable by
 * d2fe_match_batch_device (offsets in rows of `dim` floats) without unpacking -- wherever D divides the block size (every power of two).
 * D = 256 in the plain functions; the _d forms take desc_dim = 4..256, a multiple of 4 (d2fe_desc_dim of a handle with a descriptor PCA), and
 * are the plain ones at 256: same sizes, same bits. */
D2FE_API int d2fe_block_words(int cap, int netvlad_dim);                 /* words of one block */
D2FE_API int d2fe_block_field_offset(int cap, int netvlad_dim, int field);   /* word offset of field 0 desc, 1 kps, 2 scores, 3 netvlad, 4 n */
D2FE_API int d2fe_block_words_d(int cap, int desc_dim, int netvlad_dim);
D2FE_API int d2fe_block_field_offset_d(int cap, int desc_dim, int netvlad_dim, int field);
/* Packs nframes frames of a d2fe_superpoint_extract_device result (dense [rows][cap][...] arrays; frame f is row row0 + f*row_step)
 * and of a d2fe_netvlad_device result (d_netvlad [nframes][G], may be NULL) into d_blocks [nframes][d2fe_block_words]. */
D2FE_API int d2fe_pack_blocks_device(d2fe_handle h, const float* d_desc, const float* d_kps_xy, const float* d_scores,
                                     const int32_t* d_n, const float* d_netvlad, int row0, int row_step, int nframes, int cap,
                                     int netvlad_dim, float* d_blocks, void* stream);
D2FE_API int d2fe_pack_blocks_device_d(d2fe_handle h, const float* d_desc, const float* d_kps_xy, const float* d_scores,
                                       const int32_t* d_n, const float* d_netvlad, int row0, int row_step, int nframes, int cap,
                                       int desc_dim, int netvlad_dim, float* d_blocks, void* stream);
/* The same block in the reference's WIRE precision.  VisualImageDesc::toLCM quantises the descriptors to int8 before the broadcast
 * (d2common/include/d2common/d2frontend_types.h:228-237: one float maximum over the frame's landmark descriptors; :260-268: the NetVLAD
 * vector with a double maximum; scores are not sent) and the receiving constructor decodes them (:319-338: q / 127.0, the first
 * landmark_num 32-float segments re-normalised -- the reference's hard-coded 32 --, the NetVLAD vector normalised as a whole).
 *   int8 block (bytes) = desc_q[cap][D] | netvlad_q[G] | kps f32[cap][2] | n int32 | zero padding to a multiple of 64   (3.9x smaller)
 * d2fe_pack_blocks_int8_device = the quantisation, on the sender; d2fe_unpack_blocks_int8_device expands gathered int8 blocks into the
 * fp32 block layout above (scores = 0) with the decode arithmetic: renorm 0 = as the reference (landmark_num = n: the first n 32-float segments
 * of the flat array -- at D = 64 half a descriptor each, so only the first n / 2 rows are re-normalised, the reference's bug included), 1 = every
 * descriptor re-normalised over the row (its D floats).  Gate and matcher then read exactly what a receiving agent of the reference would hold. */
D2FE_API int d2fe_block_bytes_int8(int cap, int netvlad_dim);
D2FE_API int d2fe_pack_blocks_int8_device(d2fe_handle h, const float* d_desc, const float* d_kps_xy, const int32_t* d_n,
                                          const float* d_netvlad, int row0, int row_step, int nframes, int cap, int netvlad_dim,
                                          int8_t* d_blocks, void* stream);
D2FE_API int d2fe_unpack_blocks_int8_device(d2fe_handle h, const int8_t* d_blocks_int8, int nblocks, int cap, int netvlad_dim, int renorm,
                                            float* d_blocks, void* stream);
D2FE_API int d2fe_block_bytes_int8_d(int cap, int desc_dim, int netvlad_dim);
D2FE_API int d2fe_pack_blocks_int8_device_d(d2fe_handle h, const float* d_desc, const float* d_kps_xy, const int32_t* d_n,
                                            const float* d_netvlad, int row0, int row_step, int nframes, int cap, int desc_dim, int netvlad_dim,
                                            int8_t* d_blocks, void* stream);
D2FE_API int d2fe_unpack_blocks_int8_device_d(d2fe_handle h, const int8_t* d_blocks_int8, int nblocks, int cap, int desc_dim, int netvlad_dim,
                                              int renorm, float* d_blocks, void* stream);
/* NetVLAD gate of a pair list.  Replaces the similarity test of D2FeatureTracker::getMatchedPrevKeyframe
 * (d2frontend/src/d2featuretracker.cpp:185-203: `vlad_desc.dot(vlad_desc_remote) < track_remote_netvlad_thres` rejects) and of
 * LoopDetector::queryIndexFromDatabase (loop_detector.cpp:339).  Pair p compares row d_pair_q[p] of d_q (rows q_stride words apart)
 * with row d_pair_db[p] of d_db.  Outputs (each may be NULL): d_pass[p] = 1/0, d_sims[p], *d_n_pass += passing pairs (the caller
 * zeroes it), and d_cnt_inout[p] = 0 for a rejected pair -- with the matcher's a_cnt array there, d2fe_match_batch_device returns
 * no matches for pairs the reference would not have tracked. */
D2FE_API int d2fe_gate_pairs_device(d2fe_handle h, const float* d_q, size_t q_stride, const float* d_db, size_t db_stride, int dim,
                                    const int32_t* d_pair_q, const int32_t* d_pair_db, int npairs, double thres,
                                    int32_t* d_cnt_inout, int32_t* d_pass, float* d_sims, int32_t* d_n_pass, void* stream);

/* The same gate for a FOURCORNER_FISHEYE (quadcam) agent: getMatchedPrevKeyframe's second branch (d2featuretracker.cpp:212-233) compares
 * view 2 of the REMOTE quad frame with the local keyframe's views in the order dirs = {2, 3, 0, 1} and stops at the first whose similarity
 * is not below thres (dir_b = dirs[j]); trackRemoteFrames (:282-297) then tracks the four view pairs (remote view a = (2+k)%4, local view
 * (dir_b - 2 + a) % 4).  Job j = (local quad frame, remote quad frame): the NetVLAD vector of local view v is row d_job_local_row0[j] +
 * v*local_view_step of d_local (rows local_stride words apart), of remote view v row d_job_remote_row0[j] + v*remote_view_step of d_remote.
 * Outputs (each may be NULL): d_dir_prev[j] = dir_b or -1; d_sims[j][4] = the similarities for dirs[0..3]; *d_n_pass += passing jobs;
 * d_cnt_inout[j*16 + local_view*4 + remote_view] = 0 for every view pair the reference would NOT track (the 16 view pairs of a job laid
 * out as 16 consecutive matcher problems: with the matcher's a_cnt there, only the reference's four pairs are matched). */
D2FE_API int d2fe_quad_gate_device(d2fe_handle h, const float* d_local, size_t local_stride, const float* d_remote, size_t remote_stride,
                                   int dim, const int32_t* d_job_local_row0, const int32_t* d_job_remote_row0, int local_view_step,
                                   int remote_view_step, int njobs, double thres, int32_t* d_dir_prev, float* d_sims,
                                   int32_t* d_cnt_inout, int32_t* d_n_pass, void* stream);

/* ---- quadcam neighbour matching on the device (A12) -------------------------------------------------------------------------------
 * d2fe_half_image_compact_device = getFeatureHalfImg (d2frontend/src/d2featuretracker.cpp:1051-1075) for a batch of jobs, plus the
 * a-side shift of matchLocalFeatures (:1161-1170).  Job j reads row d_job_row[j] of the dense extract outputs (d_desc [rows][cap][dim],
 * d_pts_xy [rows][cap][2], d_n [rows]), keeps x < W_u - move_cols (d_job_left[j] != 0) or x >= move_cols (move_cols = (float)(W_u * 90.0 /
 * undistort_fov), as the reference computes it), and writes, in order: d_out_desc [njobs][cap][dim], d_out_pts [njobs][cap][2] with
 * d_job_shift_x[j] added to x (pass +move_cols / -move_cols / 0), d_out_map [njobs][cap] (compacted index -> original index), d_out_n [njobs].
 * d2fe_half_move_cols returns that float.  cap <= 1024.
 * d2fe_remap_matches_device = the index remap of :1178-1181 for a batch of pairs: q_idx[p][i] = map[d_map_a_job[p]][q_idx[p][i]], same for
 * t_idx with d_map_b_job (d_maps [njobs][cap_map], match arrays [npairs][cap_match]). */
D2FE_API float d2fe_half_move_cols(int width_undistort, double undistort_fov);
D2FE_API int d2fe_half_image_compact_device(d2fe_handle h, const float* d_desc, const float* d_pts_xy, const int32_t* d_n,
                                            const int32_t* d_job_row, const int32_t* d_job_left, const float* d_job_shift_x, int njobs,
                                            int cap, int dim, int width_undistort, double undistort_fov, float* d_out_desc,
                                            float* d_out_pts, int32_t* d_out_map, int32_t* d_out_n, void* stream);
D2FE_API int d2fe_remap_matches_device(d2fe_handle h, int32_t* d_q_idx, int32_t* d_t_idx, const int32_t* d_n_match,
                                       const int32_t* d_map_a_job, const int32_t* d_map_b_job, const int32_t* d_maps, int npairs,
                                       int cap_match, int cap_map, void* stream);

/* ---- Quadcam frames in flight (BASELINE configs[2], FOURCORNER_FISHEYE) ----------------------------------------------------------------------------
 * The per-frame work of a quadcam agent -- FisheyeUndist of the four raw fisheye frames (fisheye_undistort.h:152-176), SuperPoint and NetVLAD of every
 * undistorted view (loop_cam.cpp:589-648), the four neighbour matches (0,1) (1,2) (2,3) LEFT_RIGHT and (0,3) RIGHT_LEFT of matchLocalFeatures
 * (d2featuretracker.cpp:121-133,1144-1182: half images, a-side shift by +-move_cols, radius gate, indices mapped back) and the temporal matchKNN of every
 * view against the same view of the previous quad frame (:403-456) -- as ONE submit and ONE wait per `quads` quad frames, with up to `lanes` submits in
 * flight.  Per submit, on the lane's own streams: one H2D of the raw frames -> ONE undistort launch for 4 cameras x quads frames -> [NetVLAD of the
 * 4 quads views on the lane's second stream] -> SuperPoint of the 4 quads views -> half-image compaction of the 8 quads neighbour jobs -> ONE matcher
 * launch over every neighbour and temporal pair -> index remap -> ONE D2H.  The results equal those of the building blocks (d2fe_undistort_device,
 * d2fe_netvlad_device, d2fe_superpoint_extract_device, d2fe_half_image_compact_device, d2fe_match_batch_device, d2fe_remap_matches_device) composed by
 * hand at the same image count.
 * Temporal pairs: view c of quad frame q against view c of quad frame q - 1 (q = 0: the last quad frame of the previous submit; the very first quad
 * frame of the pipe has prev_n = 0).  With quads > 1 this DIFFERS from d2slam_amd/quadcam.py's QuadcamChain, which pairs frame q of a step with frame q
 * of the previous step.
 * Lifetime and errors are the stereo pipe's (d2fe_pipe_*, above): while a quad pipe exists d2fe_destroy of its handle is DEFERRED and d2fe_load_* /
 * d2fe_set_*_pca return D2FE_ERR_INVALID; the first error of a submit or wait is final for the pipe; one submitting thread, d2fe_quad_pipe_wait may be
 * called from a second one; results stay valid for 2 * lanes further submits. */
typedef struct d2fe_quad_pipe_s* d2fe_quad_pipe;
typedef struct {
  int32_t struct_size;          /* sizeof(d2fe_quad_pipe_config) */
  int32_t lanes;                /* submits in flight, 1..16 */
  int32_t quads;                /* quad frames per submit (>= 1), consecutive in time; 4 * quads <= the handle's max_batch */
  int32_t raw_width, raw_height;      /* raw fisheye frame size (1280 x 800 in the reference) */
  int32_t width, height;        /* undistorted view size (800 x 400 in the reference), within the handle's maximum */
  int32_t cap;                  /* keypoint capacity per view: <= the handle's max_keypoints (and <= 1024 with match_neighbour) */
  int32_t netvlad;              /* 1: NetVLAD of every view */
  int32_t match_neighbour;      /* 1: the four neighbour pairs of every quad frame */
  int32_t match_prev;           /* 1: every view against the same view of the previous quad frame */
  int32_t pinned_input;         /* 1: the raw pointer handed to submit is page-locked and stays valid until the ticket was waited for (DMA straight from it);
                                   0: submit copies the frames into the lane's pinned staging first */
  double ratio;                 /* knn_match_ratio */
  double radius_neighbour;      /* search_local_max_dist_lr * width (<= 0: off), d2featuretracker.cpp:669 */
  double radius_prev;           /* pixel gate of the temporal pairs (<= 0: off -- the whole image, as QuadcamChain) */
  double undistort_fov;         /* move_cols = width * 90 / undistort_fov (d2fe_half_move_cols) */
  int32_t reserved[8];          /* zero; kept for the stereo pipe's tuning knobs */
} d2fe_quad_pipe_config;
/* The four cameras' undistortion maps (d2fe_gen_cylinder_map(_device) or the caller's own), width * height floats each.  gain[c] may be NULL
 * (calib_photometric off for that camera).  device = 1: device pointers, 0: host pointers.  d2fe_quad_pipe_create copies them into memory the pipe owns. */
typedef struct {
  const float* mapx[4];
  const float* mapy[4];
  const float* gain[4];
  int32_t device;
} d2fe_quad_maps;
typedef struct {            /* HOST pointers into the lane's pinned block, quad-major (image row q * 4 + c); valid until 2 * lanes further submits */
  int32_t quads, cap, desc_dim, netvlad_dim;
  const float* kps_xy;      /* [quads][4][cap][2] */
  const float* scores;      /* [quads][4][cap] */
  const float* desc;        /* [quads][4][cap][desc_dim] */
  const int32_t* n_kp;      /* [quads][4] */
  const float* netvlad;     /* [quads][4][netvlad_dim] or NULL */
  /* neighbour pair n = 0..3 of quad frame q in the order (0,1) (1,2) (2,3) LEFT_RIGHT, (0,3) RIGHT_LEFT: [quads][4][cap] x3, [quads][4]; NULL when off.
     nb_q / nb_t index the full keypoint lists of views a / b (after the remap) */
  const int32_t* nb_q; const int32_t* nb_t; const float* nb_dist; const int32_t* nb_n;
  /* temporal pairs, view c of quad frame q against view c of quad frame q - 1: [quads][4][cap] x3, [quads][4]; NULL when off */
  const int32_t* prev_q; const int32_t* prev_t; const float* prev_dist; const int32_t* prev_n;
} d2fe_quad_pipe_result;
/* defaults: lanes 4, quads 1, raw 1280 x 800, views 800 x 400, cap 100, netvlad / match_neighbour / match_prev 1, pinned_input 0, ratio 0.8,
 * radius_neighbour 160 (0.2 * 800), radius_prev -1, undistort_fov 200 */
D2FE_API void d2fe_quad_pipe_default_config(d2fe_quad_pipe_config* cfg);
D2FE_API int d2fe_quad_pipe_create(d2fe_handle h, const d2fe_quad_pipe_config* cfg, const d2fe_quad_maps* maps, d2fe_quad_pipe* out);
D2FE_API void d2fe_quad_pipe_destroy(d2fe_quad_pipe p);
/* raw: u8 fisheye frames, image (quad frame q, camera c) at raw + q * quad_stride + c * camera_stride, rows `stride` bytes apart.  Returns at once with
 * a ticket (0, 1, 2, ...); blocks only while the ticket's lane still runs the submit of `lanes` submits ago. */
D2FE_API int d2fe_quad_pipe_submit(d2fe_quad_pipe p, const uint8_t* raw, int stride, size_t camera_stride, size_t quad_stride, int64_t* ticket);
/* Blocks until the ticket's results are in host memory.  Tickets may be waited for in any order, each within 2 * lanes submits. */
D2FE_API int d2fe_quad_pipe_wait(d2fe_quad_pipe p, int64_t ticket, d2fe_quad_pipe_result* out);
D2FE_API int d2fe_quad_pipe_lanes(d2fe_quad_pipe p);
D2FE_API int d2fe_quad_pipe_geometry(d2fe_quad_pipe p, int32_t* quads, int32_t* cap, int32_t* desc_dim, int32_t* netvlad_dim);
/* sp_lk for the quad pipe: the reference's quadcam tracker with enable_lk_optical_flow = 1 and sp_track_use_lk = 1 (config/quadcam_drone_nxt_tmp/quadcam_single.yaml).
 * d2fe_quad_track_enable(p, tp) (tp = NULL: d2fe_track_default_params) switches the mode on and allocates what it needs.  It is accepted once, before the first
 * submit; D2FE_ERR_INVALID after the first submit, a second time, for tp->levels != 2 (the lane's pyramids are PYR_LEVEL deep) and for parameters
 * d2fe_lk_carry_step_device refuses (total_feature_num + 1 > 1024, ...); a refusal leaves the pipe as it was, and a pipe it was never called on behaves, allocates
 * and measures as before.  Per submit, behind the SuperPoint results of the pass and on the lane's own streams, with no host synchronisation:
 *   the pyramids of the 4 * quads undistorted views -> for q = 0 .. quads - 1 ONE d2fe_lk_carry_quad_step_device (track(images[c]), c = 0..3: four lists, ONE id
 *   counter in camera order; the predecessor of q = 0 is the last quad frame of the previous SUBMIT, whichever lane ran it: its lists are read in place, its four
 *   pyramids from a pipe-owned copy, behind an event the previous pass recorded) -> ONE d2fe_lk_carry_neighbour_device over the pass's lists -> the neighbour
 *   matchKNN of the LISTS (matchLocalFeatures :1144-1182 on the frames' landmarks, which in this mode are the list entries with their carried descriptors): exactly
 *   d2fe_half_image_compact_device + d2fe_match_batch_device + d2fe_remap_matches_device over dense copies of the lists' points, descriptors and counts, with the
 *   pipe's ratio, radius_neighbour, undistort_fov and a-side shift, cap = cap_tracks -> everything in the pass's ONE D2H.
 * d2fe_quad_track_result_get after d2fe_quad_pipe_wait (D2FE_ERR_NOT_READY before it, D2FE_ERR_UNSUPPORTED on a pipe without the mode): list (q, c) is the list
 * block (q * 4 + c) * list_words 32-bit words behind every per-list pointer (the conventions of d2fe_pipe_track_result: n[(q * 4 + c) * list_words], ...); the list
 * of camera a that a neighbour pair tracks and matches is the list AFTER this frame's step.  d2fe_quad_pipe_result and its nb_* / prev_* stay keypoint-based,
 * governed by match_neighbour / match_prev (the reference's configuration of this mode has both off).  Results are bit-identical for every (lanes, quads).
 * With the caller: id -> lmanager ids and velocities.  createLKLandmark / liftProjective, predictLandmarksWithExtrinsic and the lk_lk_use_pred gate
 * of the neighbour tracks run on the device once d2fe_quad_bearings_enable has switched them on (below), and are the caller's otherwise. */
typedef struct {            /* HOST pointers into the lane's pinned block, same lifetime as d2fe_quad_pipe_result */
  int32_t quads, cap_tracks, desc_dim, list_words;
  const int32_t* n;                  /* per list: list (q, c)'s count is n[(q * 4 + c) * list_words]; the same stride for every "per list" pointer below */
  const int32_t* n_tracked_in; const int32_t* n_lost; const int32_t* n_removed_near; const int32_t* n_new;      /* per list */
  const float* pts_xy;               /* per list: [cap_tracks][2] */
  const int32_t* id; const int32_t* src; const int32_t* kp;      /* per list: [cap_tracks] */
  const float* desc;                 /* per list: [cap_tracks][desc_dim] */
  const float* scores;               /* per list: [cap_tracks] */
  const float* nb_lk_xy;             /* [quads][4][cap_tracks][2], contiguous: neighbour pair n, slot i of list a */
  const uint8_t* nb_lk_status;       /* [quads][4][cap_tracks] */
  /* the neighbour matchKNN of the lists: [quads][4][cap_tracks] x3, [quads][4]; lnb_q / lnb_t index the entries of the lists of views a / b */
  const int32_t* lnb_q; const int32_t* lnb_t; const float* lnb_dist; const int32_t* lnb_n;
} d2fe_quad_track_result;
D2FE_API int d2fe_quad_track_enable(d2fe_quad_pipe p, const d2fe_track_params* tp);
D2FE_API int d2fe_quad_track_result_get(d2fe_quad_pipe p, int64_t ticket, d2fe_quad_track_result* out);
/* flow_lk for the quad pipe: the reference's quadcam tracker with enable_lk_optical_flow = 1, sp_track_use_lk = 0 and max_superpoint_cnt > 0
 * (config/quadcam/quadcam_single.yaml, quadcam_multi.yaml, quadcam_multi_rt.yaml): SuperPoint and the flow landmarks together.  d2fe_quad_flow_enable(p, fp) (fp = NULL:
 * d2fe_flow_default_params) switches the mode on and allocates what it needs; d2fe_quad_pipe_config is closed and keeps its size.  It is accepted once, before the
 * first submit; D2FE_ERR_INVALID after the first submit, a second time, together with d2fe_quad_track_enable in either order (the reference runs one of the two
 * branches, d2featuretracker.cpp:556-614), for fp->track.levels != 2, for fp->superpoint = 0 (no quadcam configuration has max_superpoint_cnt: 0; flow-only pipes are
 * the stereo / mono ones) and for what d2fe_lk_flow_quad_step_device refuses at the view size; a refusal leaves the pipe as it was and usable, and a pipe the call
 * never succeeded on keeps its layout, allocations, launches and results.  Per submit, behind the SuperPoint results of the pass and on the lane's own streams:
 *   the pyramids of the 4 * quads undistorted views -> for q = 0 .. quads - 1 ONE d2fe_lk_flow_quad_step_device (five launches) on the keypoints of quad frame q, on
 *   the chain sp_lk uses (the predecessor of q = 0 is the last quad frame of the previous SUBMIT: its lists read in place, its four pyramids from a pipe-owned copy
 *   behind the previous pass's chain event; ONE pipe-owned id counter; ONE pipe-owned scratch of four cameras that all lanes share, because the chain serialises the
 *   steps) -> ONE d2fe_lk_flow_neighbour_device over the pass's flow lists -> everything in the pass's ONE D2H.
 * No matchKNN of the lists: flow entries have no descriptors, and the keypoint-based nb_* / prev_* of d2fe_quad_pipe_result (match_neighbour / match_prev) are this
 * mode's matchKNN.  d2fe_quad_flow_result_get after d2fe_quad_pipe_wait (D2FE_ERR_NOT_READY before it, D2FE_ERR_UNSUPPORTED on a pipe without the mode): list (q, c)
 * is (q * 4 + c) * list_words 32-bit words behind every per-list pointer (the convention of d2fe_quad_track_result); the list of camera a that a neighbour pair
 * tracks is the list AFTER this frame's step.  Results are bit-identical for every (lanes, quads).
 * With the caller: id -> lmanager ids and velocities.  createLKLandmark / liftProjective, predictLandmarksWithExtrinsic and the lk_lk_use_pred gate
 * of the neighbour tracks run on the device once d2fe_quad_bearings_enable has switched them on (below), and are the caller's otherwise. */
typedef struct {            /* HOST pointers into the lane's pinned block, same lifetime as d2fe_quad_pipe_result */
  int32_t quads, cap_tracks, list_words, reserved;
  const int32_t *n, *n_tracked_in, *n_lost, *n_removed_near, *n_new, *lack, *num, *n_cand;      /* per list */
  const float* pts_xy;               /* per list: [cap_tracks][2] */
  const int32_t *id, *src;           /* per list: [cap_tracks] */
  const float* nb_lk_xy;             /* [quads][4][cap_tracks][2], contiguous: neighbour pair n, slot i of list a */
  const uint8_t* nb_lk_status;       /* [quads][4][cap_tracks] */
} d2fe_quad_flow_result;
D2FE_API int d2fe_quad_flow_enable(d2fe_quad_pipe p, const d2fe_flow_params* fp);
D2FE_API int d2fe_quad_flow_result_get(d2fe_quad_pipe p, int64_t ticket, d2fe_quad_flow_result* out);
/* Bearings, neighbour predictions and their gate IN THE QUAD PIPE: d2fe_pipe_bearings_enable's pass and contract (above) for the four cameras of the quad rig, whose
 * views with enable_undistort_image are D2FE_CAM_CYLINDRICAL (d2fe_cylinder_camera); any kind d2fe_bearings_device serves is taken.  Accepted once, before the first
 * submit, in any order with d2fe_quad_track_enable / d2fe_quad_flow_enable.  Refused (D2FE_ERR_INVALID, the pipe stays as it was and usable): a wrong struct_size,
 * after the first submit, a second time, what d2fe_bearings_device refuses in a camera, distance or T_nb not finite, radius_lk NaN, lk_use_pred not 0 or 1.
 * Per pass ONE more launch (bearings_kernel, D2FE_PROF_LK) behind the list chain and the neighbour LK launch, in front of the matcher:
 *   keypoint rows      bearing of row (q, c) with cam[c]
 *   list entries       (sp_lk or flow_lk) bearing of list (q, c) AFTER this frame's step with cam[c]
 *   neighbour pairs    (sp_lk or flow_lk) pair n = (a, b) of (0,1) (1,2) (2,3) (0,3): entry i of list (q, a) predicted into camera b through T_nb[n] and projected with
 *                      cam[a] -- the reference's cams.at(left camera_index) quirk, kept as in the stereo pipe --, the lift of nb_lk_xy with cam[b], and the gate
 *                      nb_pred_ok[i] = nb_lk_status[i] && (radius_lk <= 0 || !lk_use_pred || cv::norm(pred - nb_lk_xy) < radius_lk) (trackLK(left, right, type),
 *                      d2featuretracker.cpp:720-747).  List 0 is the left list of pairs 0 and 3 and is predicted twice: the arrays are per pair.
 * No keypoint predictions: matchLocalFeatures computes them for neighbour pairs but its half-image branch never uses them (:1144-1173); nb_* / prev_* stay as they are.
 * The new arrays sit at the end of the region in front of d2h_words (inside the pass's one D2H), behind the lists' arrays whichever enable came first; every other
 * result is bit-identical, and a pipe that never enables the mode keeps its layout, allocations and launches.
 * With the caller: the NaN skip, lmanager ids, velocities and colours, motion prediction from lmanager positions, check_essential. */
typedef struct {
  int32_t struct_size;      /* sizeof(d2fe_quad_bearings), checked strictly */
  int32_t lk_use_pred;      /* lk_lk_use_pred, default 1; 0: nb_pred_ok = nb_lk_status */
  d2fe_camera cam[4];       /* camera c of the rig */
  double T_nb[4][12];       /* pair n = (a, b) in the pipe's order (0,1) (1,2) (2,3) (0,3): takes a point of camera a into camera b (d2fe_relative_extrinsic) */
  double distance;          /* landmark_distance_assumption, default 100 */
  double radius_lk;         /* search_local_max_dist_lr * width; <= 0: nb_pred_ok = nb_lk_status */
} d2fe_quad_bearings;
D2FE_API void d2fe_quad_bearings_default(d2fe_quad_bearings* b);      /* struct_size, lk_use_pred = 1, distance = 100, every T_nb = identity, everything else 0 */
D2FE_API int d2fe_quad_bearings_enable(d2fe_quad_pipe p, const d2fe_quad_bearings* b);
/* The bearings of a ticket that d2fe_quad_pipe_wait has returned (D2FE_ERR_NOT_READY before that, D2FE_ERR_UNSUPPORTED on a pipe without the mode).  Every array is
 * contiguous; slots >= n hold zeros. */
typedef struct {            /* HOST pointers into the lane's pinned block, same lifetime as d2fe_quad_pipe_result */
  int32_t quads, cap, cap_tracks, reserved;      /* cap_tracks: of the lists the pipe carries (sp_lk or flow_lk), 0 without them */
  const double* kp_bearing;          /* [quads][4][cap][3], the rows of d2fe_quad_pipe_result::kps_xy */
  const double* list_bearing;        /* [quads][4][cap_tracks][3]: list (q, c); NULL without lists, as the three below */
  const float* nb_pred_xy;           /* [quads][4][cap_tracks][2]: pair n, entry i of list a predicted into camera b */
  const double* nb_bearing;          /* [quads][4][cap_tracks][3]: the lift of nb_lk_xy with cam[b] */
  const uint8_t* nb_pred_ok;         /* [quads][4][cap_tracks]: the gate on nb_lk_status */
} d2fe_quad_bearings_result;
D2FE_API int d2fe_quad_bearings_result_get(d2fe_quad_pipe p, int64_t ticket, d2fe_quad_bearings_result* out);
/* The pipe's undistort step on its own: ONE launch for 4 cameras x quads raw frames (image (q, c) at d_raw + q * quad_stride + c * camera_stride), maps
 * as above with device = 1 and every map pointer 16-byte aligned; view (q, c) is written to d_dst + (q * 4 + c) * dw * dh.  Same bytes as
 * d2fe_undistort_device camera by camera. */
D2FE_API int d2fe_quad_undistort_device(d2fe_handle h, const uint8_t* d_raw, int quads, int sw, int sh, int sstride, size_t camera_stride,
                                        size_t quad_stride, const d2fe_quad_maps* maps, int dw, int dh, uint8_t* d_dst, void* stream);

/* Device-side consumers of a quad ticket: the contract of d2fe_pipe_device_view / _device_release / _lane_stream / _handle above, for the quad pipe.
 *   d2fe_quad_device_view     launches nothing; makes `stream` (a hipStream_t, not NULL) wait for the ticket's SuperPoint and NetVLAD results (not for its matcher
 *                             or its D2H) and returns DEVICE pointers into the lane's result block, in the block's own quad-major row order (row q * 4 + c).
 *                             Read-only.  Valid until the matching release, at most 2 * lanes submits.
 *   d2fe_quad_device_release  everything queued on `stream` so far is what read the view: the lane's next write of that block (pass + 2 * lanes) waits for it on
 *                             the device (an event, no host wait).
 * A block whose view is still outstanding when its lane comes round again fails that submit with D2FE_ERR_INVALID (and, like every failed submit, ends the
 * pipe).  ONE consumer stream per pipe.  Both calls may come from a thread other than the submitting one.  A pipe nobody takes a view of runs as before. */
typedef struct {
  int32_t quads, cap, desc_dim, netvlad_dim;
  const float* d_kps_xy;    /* [quads][4][cap][2] */
  const float* d_scores;    /* [quads][4][cap] */
  const float* d_desc;      /* [quads][4][cap][desc_dim] */
  const int32_t* d_n_kp;    /* [quads][4] */
  const float* d_netvlad;   /* [quads][4][netvlad_dim] or NULL */
} d2fe_quad_device_result;
D2FE_API int d2fe_quad_device_view(d2fe_quad_pipe p, int64_t ticket, void* stream, d2fe_quad_device_result* out);
D2FE_API int d2fe_quad_device_release(d2fe_quad_pipe p, int64_t ticket, void* stream);
/* the stream of the lane that ran the ticket's submit (a hipStream_t): work queued on it runs behind that submit's D2H and in front of the lane's next submit */
D2FE_API int d2fe_quad_lane_stream(d2fe_quad_pipe p, int64_t ticket, void** stream);
D2FE_API d2fe_handle d2fe_quad_handle(d2fe_quad_pipe p);

/* ---- Cross-agent exchange behind a quad pipe (BASELINE configs[4]: a swarm of quadcam agents) ---------------------------------------------------------
 * d2fe_exchange_* above for a FOURCORNER_FISHEYE agent.  Replaces, per remote quad frame: LoopNet::broadcastVisualImageDescArray
 * (d2frontend/src/loop_net.cpp:24-87) in the int8 wire form of d2common/include/d2common/d2frontend_types.h:228-268,319-338, the FOURCORNER_FISHEYE branch of
 * D2FeatureTracker::getMatchedPrevKeyframe (d2frontend/src/d2featuretracker.cpp:212-233) and the four view pairs of trackRemoteFrames (:282-297).  One
 * sequence per ticket, asynchronous, on ONE stream of the exchange's own (own_stream = 1) or on the producing lane's stream (own_stream = 0):
 *   d2fe_quad_device_view -> pack 4 * quads blocks straight from the result block (fp32 or int8) -> ONE all-gather -> [int8: decode] -> ONE launch of
 *   quad_exchange_prepare_kernel (the gate of every job, the matcher's problem table, the counter) -> ONE d2fe_match_batch_device launch (local descriptors in
 *   place in the lane's block, remote ones in place in the gathered blocks) -> d2fe_quad_device_release -> ONE D2H into pinned slot `slot`.
 * No host synchronisation in d2fe_quad_exchange_enqueue (the matcher's scratch is allocated by the first launch on a stream, as everywhere); whatever fails
 * after the view was taken, the view is released.
 * Layout.  One block per VIEW; block index within a rank = q * 4 + v, the pipe's row order (d2slam_amd/swarm.py's QuadSwarm uses v * Q + q); the gathered
 * buffer is [world][4 * quads][block].  Job j = (remote rank r, quad frame q), rank-major over the OTHER ranks (all ranks with loopback), then q: local quad
 * frame q against quad frame q of rank r (d2fe_quad_exchange_job_layout, which needs no device).
 *   mode 0, all2all: 16 problems per job, index j * 16 + lv * 4 + rv (local view lv against remote view rv); the gate is evaluated and counted, nothing is zeroed.
 *   mode 1, gated  : 4 problems per job, index j * 4 + k, in trackRemoteFrames' order: remote view a = (2 + k) % 4, local view (dir_b - 2 + a) mod 4.  A job that
 *                    fails the gate has n_match = 0 for its four problems and local_view = remote_view = -1.  Needs NetVLAD (else D2FE_ERR_INVALID).
 * gate_sims / dir_prev are bit-equal to d2fe_quad_gate_device on the same vectors (local: the view's d_netvlad, remote: the netvlad field of the gathered fp32
 * blocks).  The blocks take the pipe's descriptor width (d2fe_quad_pipe_geometry: 256, or the PCA width of a variant_b_pca handle): sizes and fields are those of the
 * _d layout functions; a width that does not divide the block size (the matcher reads the blocks in place, in rows) is D2FE_ERR_UNSUPPORTED -- 64 and every other
 * power of two divide it. */
typedef enum { D2FE_QUAD_ALL2ALL = 0, D2FE_QUAD_GATED = 1 } d2fe_quad_exchange_mode;
typedef struct {
  int32_t struct_size;
  int32_t world, rank;          /* of the communicator */
  int32_t wire;                 /* d2fe_wire */
  int32_t loopback;             /* the rank's OWN gathered blocks count as a remote agent too */
  int32_t slots;                /* ring of pinned result slots */
  int32_t own_stream;           /* 1 (default): one stream of the exchange's own; 0: each ticket's sequence on its lane's stream */
  int32_t timing;               /* 1: HIP events around the five phases (d2fe_quad_exchange_result.phase_ms) */
  int32_t mode;                 /* d2fe_quad_exchange_mode */
  int32_t reserved0;
  double gate_thres;            /* track_remote_netvlad_thres */
  double ratio;                 /* knn_match_ratio */
  d2fe_all_gather_fn all_gather; void* all_gather_user;      /* used when the communicator is NULL */
  int32_t reserved[6];
} d2fe_quad_exchange_config;
typedef struct {            /* HOST pointers into the pinned slot, valid until the slot is enqueued again */
  int64_t ticket;
  int32_t njobs, npairs, pairs_per_job /* 16 or 4 */, cap;
  const int32_t* job_rank;      /* [njobs] remote rank */
  const int32_t* job_quad;      /* [njobs] quad frame */
  const int32_t* q_idx;         /* [npairs][cap] local keypoint index */
  const int32_t* t_idx;         /* [npairs][cap] remote keypoint index */
  const float* dist;            /* [npairs][cap] */
  const int32_t* n_match;       /* [npairs] */
  const int32_t* local_view;    /* [npairs] 0..3, or -1 (gated: the job failed the gate) */
  const int32_t* remote_view;   /* [npairs] */
  const int32_t* dir_prev;      /* [njobs] dir_b or -1 (NULL without NetVLAD) */
  const float* gate_sims;       /* [njobs][4] for dirs {2, 3, 0, 1} (NULL without NetVLAD) */
  int32_t gate_n;               /* jobs passing the gate */
  float phase_ms[5];            /* timing = 1: pack, all-gather, decode + prepare, remote matchKNN, release + D2H */
} d2fe_quad_exchange_result;
typedef struct d2fe_quad_exchange_s* d2fe_quad_exchange;
/* defaults: world 1, rank 0, fp32, no loopback, 4 slots, own_stream 1, timing 0, all2all, gate_thres 0.8, ratio 0.8 */
D2FE_API void d2fe_quad_exchange_default_config(d2fe_quad_exchange_config* c);
D2FE_API int d2fe_quad_exchange_create(d2fe_quad_pipe p, void* nccl_comm, const d2fe_quad_exchange_config* cfg, d2fe_quad_exchange* out);
D2FE_API void d2fe_quad_exchange_destroy(d2fe_quad_exchange x);      /* before the pipe */
D2FE_API int d2fe_quad_exchange_enqueue(d2fe_quad_exchange x, int64_t ticket, int slot);      /* asynchronous; within 2 * lanes submits of the ticket's */
D2FE_API int d2fe_quad_exchange_collect(d2fe_quad_exchange x, int slot, d2fe_quad_exchange_result* out);      /* blocks until the slot's results are in host memory */
D2FE_API int d2fe_quad_exchange_jobs(d2fe_quad_exchange x);
D2FE_API int d2fe_quad_exchange_pairs(d2fe_quad_exchange x);         /* matcher problems per enqueue: 16 or 4 per job */
D2FE_API int d2fe_quad_exchange_block_bytes(d2fe_quad_exchange x);   /* bytes one VIEW contributes to the all-gather */
D2FE_API void* d2fe_quad_exchange_stream(d2fe_quad_exchange x);      /* own_stream = 1: that stream (hipStream_t), else NULL */
/* DEVICE pointers of the slot's gathered blocks [world][4 * quads] (either may be NULL): *d_blocks = the fp32 blocks gate and matcher read (for an int8 wire: the
 * decode), *d_wire_blocks = the blocks as they crossed the wire (fp32: the same pointer).  The remote keypoints a t_idx refers to are in there
 * (d2fe_block_field_offset_d with the pipe's desc_dim; d2fe_block_field_offset at 256).  Complete once the slot was collected; valid until the slot is enqueued again. */
D2FE_API int d2fe_quad_exchange_gathered(d2fe_quad_exchange x, int slot, const float** d_blocks, const void** d_wire_blocks);
/* The job list of one rank without a device: job_rank[j] / job_quad[j] for j < min(njobs, cap_jobs) (either array may be NULL); returns njobs =
 * (world - 1, or world with loopback) * quads, or D2FE_ERR_INVALID.  d2fe_quad_exchange_create builds its table with this function. */
D2FE_API int d2fe_quad_exchange_job_layout(int world, int rank, int quads, int loopback, int32_t* job_rank, int32_t* job_quad, int cap_jobs);

/* ---- Loop query behind a pipe: device keyframe store, search and match --------------------------------------------------------------------------------
 * What LoopDetector::processImageArray (d2frontend/src/loop_detector.cpp:23-215) does with a keyframe once the tracker is done with it, per ticket of a stereo
 * pipe or a quad pipe, asynchronous, on ONE stream of the object's own and without a host synchronisation:
 *   device view of the ticket -> ONE search-gate-prepare launch (queryImageArrayFromDatabase -> queryIndexFromDatabase, :300-406, for every frame of the ticket)
 *   -> ONE matcher launch (computeCorrespondFeaturesOnImageArray -> computeCorrespondFeatures -> matchKNN, :443-578: the frame's descriptors read in place in the
 *   lane's result block, the stored keyframe's in place in the store) -> ONE append launch (addImageArrayToDatabase, :228-263, device to device) -> release of the
 *   view -> ONE D2H into pinned slot `slot`.
 * The store is on the device: the index [capacity_keyframes * V][netvlad_dim] with the keyframe ordinal and the view of every row (index_to_frame_id, imgid2dir),
 * the descriptors [capacity_keyframes][V][cap][desc_dim] with their counts, and ntotal.  V = 1 behind a stereo pipe (only the left image carries an image_desc,
 * loop_cam.cpp:446-451), V = 4 behind a quad pipe; the queried view is main_dir = 0 / 2 (:358-371).  A view gets an index row when its n_kp > 0 (:233): the DEVICE
 * decides, the host knows an upper bound.  There is ONE index: the reference's remote_index is never filled (add_to_faiss is false for remote frames, :200-206) and
 * its merge (:284, :288) returns a similarity as an index.
 * Order.  Frame f of a ticket sees the index rows [0, ntotal_f): those before the ticket and those the ticket's earlier frames add -- query, then add, frame by frame
 * (:157-207).  A frame is queried when it is flagged, its main view has keypoints (:378) and ntotal_f > max_index (:157).
 * Selection.  The best row by (similarity descending, label ascending) among the rows with label <= ntotal_f - max_index, accepted when its similarity > thres: what
 * the reference's scan of the top min(5 + max_index, ntotal) returns (:314-345), as it excludes at most max_index - 1 labels.  Similarities are bit-equal to
 * d2fe_db_search's.
 * Pairs.  A hit on (keyframe k, view dir_old) gives V matcher problems, i = 0 .. V - 1: dir_a = (main_dir + i) % V of the frame against
 * dir_b = ((dir_old - main_dir + V) % V + main_dir + i) % V of keyframe k (:461-476); an empty side gives 0 matches (:470-471).  Without a hit: n_match = 0,
 * dir_a = dir_b = -1.  Match lists are bit-equal to d2fe_match_knn (mode 0: ratio, no radius, :572-574) / d2fe_match_crosscheck (mode 1, :576-577).
 * With the caller: frame_id <-> keyframe ordinal (the k-th frame ever added has ordinal k), the landmark_db flag filter (:582-...), MIN_MATCH_PRE_DIR,
 * MIN_DIRECTION_LOOP, loop_inlier_feature_num, PnP, lazy and pre-matched frames, SuperGlue.
 * Errors are the exchanges': a refused d2fe_loop_enqueue (busy slot, ticket not after the last one, full store, a ticket older than 2 * lanes passes) queues nothing
 * and leaves the store as it was; whatever fails after the view was taken, the view is released. */
enum { D2FE_LOOP_QUERY = 1, D2FE_LOOP_ADD = 2 };
typedef struct {
  int32_t struct_size;          /* sizeof(d2fe_loop_config) */
  int32_t capacity_keyframes;   /* keyframes the store holds (V index rows each); nothing is evicted or overwritten */
  int32_t max_index;            /* match_index_dist (loop_detector.cpp:157, :339) */
  int32_t mode;                 /* 0: matchKNN with `ratio` (enable_knn_match, :572-574); 1: cross-check (:576-577) */
  int32_t slots;                /* ring of pinned result slots */
  int32_t timing;               /* 1: HIP events around the phases (d2fe_loop_result.phase_ms) */
  int32_t max_queries;          /* frames one d2fe_loop_query_device call may carry (1..256) */
  int32_t reserved0;
  double thres;                 /* loop_detection_netvlad_thres (:267, :339) */
  double ratio;                 /* knn_match_ratio */
  int32_t reserved[6];
} d2fe_loop_config;
typedef struct {            /* HOST pointers into the pinned slot, valid until the slot is enqueued again */
  int64_t ticket;               /* -1: d2fe_loop_query_device */
  int32_t frames, views, cap, reserved;
  const int32_t* queried;       /* [frames] 1: the frame was searched */
  const int32_t* label;         /* [frames] index row, or -1 */
  const float* sim;             /* [frames] its similarity (0 without a hit) */
  const int32_t* keyframe;      /* [frames] ordinal of the keyframe the row belongs to, or -1 */
  const int32_t* dir_old;       /* [frames] the view the row came from (camera_index_old), or -1 */
  const int32_t* ntotal_at_query;   /* [frames] */
  const int32_t* added_label;   /* [frames][views] the index row view v of the frame received, or -1 */
  const int32_t* dir_a;         /* [frames][views] view of the frame, or -1 */
  const int32_t* dir_b;         /* [frames][views] view of the keyframe, or -1 */
  const int32_t* n_match;       /* [frames][views] */
  const int32_t* q_idx;         /* [frames][views][cap] keypoint of the frame's view dir_a */
  const int32_t* t_idx;         /* [frames][views][cap] keypoint of the keyframe's view dir_b */
  const float* dist;            /* [frames][views][cap] */
  float phase_ms[4];            /* timing = 1: search-gate-prepare, match, append, release + D2H */
} d2fe_loop_result;
typedef struct d2fe_loop_s* d2fe_loop;
/* defaults: capacity_keyframes 4096, max_index 10, mode 0, 4 slots, timing 0, max_queries 64, thres 0.6, ratio 0.8 */
D2FE_API void d2fe_loop_default_config(d2fe_loop_config* c);
/* the pipe must have NetVLAD on (D2FE_ERR_INVALID otherwise) */
D2FE_API int d2fe_loop_create(d2fe_pipe p, const d2fe_loop_config* cfg, d2fe_loop* out);
D2FE_API int d2fe_loop_create_quad(d2fe_quad_pipe p, const d2fe_loop_config* cfg, d2fe_loop* out);
D2FE_API void d2fe_loop_destroy(d2fe_loop x);      /* before the pipe */
/* asynchronous.  is_keyframe: [frames] (quad pipe: [quads]) or NULL = every frame; flags: D2FE_LOOP_QUERY | D2FE_LOOP_ADD for the flagged frames.  Tickets in
 * submit order, each within 2 * lanes passes of its submit. */
D2FE_API int d2fe_loop_enqueue(d2fe_loop x, int64_t ticket, int slot, const uint8_t* is_keyframe, int flags);
D2FE_API int d2fe_loop_collect(d2fe_loop x, int slot, d2fe_loop_result* out);      /* blocks until the slot's results are in host memory */
D2FE_API int d2fe_loop_ntotal(d2fe_loop x);         /* index rows; synchronises the loop's stream */
D2FE_API int d2fe_loop_keyframes(d2fe_loop x);      /* keyframes in the store; synchronises the loop's stream */
D2FE_API void* d2fe_loop_stream(d2fe_loop x);       /* the loop's stream (hipStream_t) */
/* n keyframes from HOST memory in the layout of the device arrays below (netvlad [n][V][netvlad_dim], desc [n][V][cap][desc_dim], n_kp [n][V]): the append step as
 * blocking copies, for a store that does not start empty (and for tests and benchmarks).  Synchronises the loop's stream.  Returns the ordinal of the first
 * keyframe added, or D2FE_ERR_TRUNCATED (nothing added) when they do not all fit. */
D2FE_API int d2fe_loop_add_host(d2fe_loop x, const float* netvlad, const float* desc, const int32_t* n_kp, int n);
/* Query only, for frames that did not come from this pipe: a remote agent's frames query the local index with match_index_dist_remote and are never added
 * (:200-206, :294-295).  DEVICE arrays in the pipe's own row order and geometry: d_netvlad [nq][V][netvlad_dim] (16-byte aligned), d_desc [nq][V][cap][desc_dim],
 * d_n_kp [nq][V]; they are read in place and stay valid until the slot was collected.  stream: the hipStream_t that produced them (the loop's stream waits for what is
 * queued on it now), or NULL when they are complete.  Same sequence without the append; results with d2fe_loop_collect (ticket = -1). */
D2FE_API int d2fe_loop_query_device(d2fe_loop x, const float* d_netvlad, const float* d_desc, const int32_t* d_n_kp, int nq, int max_index, int slot, void* stream);

/* ---- Remote tracking against the keyframe window, behind a pipe ------------------------------------------------------------------------------------------
 * What D2FeatureTracker::trackRemoteFrames (d2frontend/src/d2featuretracker.cpp:237-310) does with a remote frame: it does not match it against the frame of the same
 * step (the all-to-all mode of d2fe_exchange_* / d2fe_quad_exchange_*) but walks the tracker's keyframe window, current_keyframes, through getMatchedPrevKeyframe
 * (:166-235) -- newest keyframe first, for a quadcam agent that keyframe's views in the order dirs = {2, 3, 0, 1} -- stops at the FIRST NetVLAD similarity that is not
 * below track_remote_netvlad_thres, and matches that keyframe against the remote frame (trackRemote -> matchLocalFeatures(prev_frame, frame) -> matchKNN, :312-387).
 * Here the window lives on the device and a batch of remote frames is tracked by ONE sequence, asynchronous, on ONE stream of the object's own, without a host
 * synchronisation:
 *   ONE gate launch (every similarity remote gate view x (keyframe, view), the selection, the per-frame records, the matcher's problem table) -> ONE matcher launch
 *   (a side: the chosen keyframe's descriptors in place in the store; b side: the remote descriptors in place where the caller left them) -> ONE D2H into pinned
 *   slot `slot`.
 * The store: `capacity` slots of NetVLAD [V][netvlad_dim], descriptors [V][cap][desc_dim] (rows >= n_kp zero), n_kp [V] and the caller's 64-bit tag (its frame_id,
 * >= 0).  V = 1 behind a stereo pipe (view 0, the left image), V = 4 behind a quad pipe.  The window's ORDER (oldest -> newest, as current_keyframes) and the free slots
 * are host bookkeeping that only the calls below change; the order travels to the gate kernel by value, so a query queued earlier keeps the order it was queued with, and
 * slot order and window order differ as soon as a freed slot was reused.
 * Selection.  With pos the position in the window (oldest = 0, n keyframes) and j the place in `dirs` (stereo: j = 0), the chosen pair is the minimum of
 * (n - 1 - pos) * V + j over the pairs with !(sim < thres) -- the first pass of the reference's walk, NOT the best similarity.  The remote gate view is view 0 (stereo) /
 * view 2 (quad); the gate looks at NetVLAD vectors only (views without keypoints take part, as in the reference).  Similarities are bit-equal to
 * d2fe_gate_pairs_device / d2fe_quad_gate_device.
 * Problems per remote frame, fixed layout: V = 1: (local view 0, remote view 0).  V = 4: k = 0..3 in trackRemoteFrames' order (:273-284): remote view
 * (2 + k) % 4 against local view (dir_b - 2 + remote view) mod 4 -- the D2FE_QUAD_GATED layout.  A problem with an empty side (:278-279) keeps its place with
 * n_match = 0; a frame without a hit has n_match = 0 and views -1.  No points and no radius: trackRemote leaves enable_search_in_local false and, without prediction,
 * passes -1.  Match lists are bit-equal to d2fe_match_knn(keyframe view, remote view) (mode 0) / d2fe_match_crosscheck (mode 1): query = local keyframe, train = remote.
 * With the caller: tag <-> frame_id, is_lazy_frame / matched_frame (:239), the early return of updatebySldWin for an empty sliding window (:41), the landmark-id and
 * solver_id bookkeeping (:340-381), remote_min_match_num (:1290), check_essential (a RANSAC), motion prediction (enable_search_local_aera_remote, default false: it
 * needs the landmark manager), the right-image pair of a stereo agent without lr_lk (:263-268: it depends on the landmark ids of the first pair), SuperGlue.
 * A refusal queues nothing and leaves the window as it was. */
typedef struct {
  int32_t struct_size;          /* sizeof(d2fe_window_config) */
  int32_t capacity;             /* slots of the window (1..64; max_sld_win_size is 11 in the shipped configs, plus the newest keyframe) */
  int32_t mode;                 /* 0: matchKNN with `ratio` (enable_knn_match); 1: cross-check (enable_knn_match = 0) */
  int32_t slots;                /* ring of pinned result slots */
  int32_t timing;               /* 1: HIP events around the phases (d2fe_window_result.phase_ms) */
  int32_t max_queries;          /* remote frames one d2fe_window_track_device call may carry (1..256) */
  double thres;                 /* track_remote_netvlad_thres */
  double ratio;                 /* knn_match_ratio */
  int32_t reserved[6];
} d2fe_window_config;
typedef struct {            /* HOST pointers into the pinned slot, valid until the slot is queued again */
  int32_t nq, views, cap, capacity;
  int32_t n_window, reserved;   /* keyframes in the window as the query was queued */
  const int64_t* keyframe_tag;  /* [nq] tag of the chosen keyframe, -1 without a hit */
  const int32_t* keyframe_pos;  /* [nq] its position in the window as queued (oldest = 0), or -1 */
  const int32_t* dir_a;         /* [nq] the remote gate view (0 / 2), or -1 */
  const int32_t* dir_b;         /* [nq] the keyframe's view that passed, or -1 */
  const float* sim;             /* [nq] its similarity (0 without a hit) */
  const float* sims;            /* [nq][capacity][views] every similarity, window order then `dirs` order; zeros beyond the window */
  const int32_t* local_view;    /* [nq][views] view of the keyframe, or -1 */
  const int32_t* remote_view;   /* [nq][views] view of the remote frame, or -1 */
  const int32_t* n_match;       /* [nq][views] */
  const int32_t* q_idx;         /* [nq][views][cap] keypoint of the keyframe's view */
  const int32_t* t_idx;         /* [nq][views][cap] keypoint of the remote view */
  const float* dist;            /* [nq][views][cap] */
  float phase_ms[3];            /* timing = 1: gate, match, D2H */
  int32_t reserved1;
} d2fe_window_result;
typedef struct d2fe_window_s* d2fe_window;
/* defaults: capacity 12, mode 0, 4 slots, timing 0, max_queries 64, thres 0.8, ratio 0.8 */
D2FE_API void d2fe_window_default_config(d2fe_window_config* c);
/* the pipe must have NetVLAD on (D2FE_ERR_INVALID otherwise) */
D2FE_API int d2fe_window_create(d2fe_pipe p, const d2fe_window_config* cfg, d2fe_window* out);
D2FE_API int d2fe_window_create_quad(d2fe_quad_pipe p, const d2fe_window_config* cfg, d2fe_window* out);
D2FE_API void d2fe_window_destroy(d2fe_window x);      /* before the pipe */
D2FE_API void* d2fe_window_stream(d2fe_window x);      /* the window's stream (hipStream_t) */
/* processFrame's emplace_back (:837), asynchronous: takes the ticket's device view, copies frame `frame` (quad pipe: quad `frame`) of it into a free slot with ONE launch
 * on the window's stream, releases the view.  A tag equal to the newest keyframe's is a no-op (:806-808, D2FE_OK).  Refused: a full window (D2FE_ERR_TRUNCATED), a tag
 * that is in the window already, a negative tag, a ticket older than 2 * lanes passes. */
D2FE_API int d2fe_window_push(d2fe_window x, int64_t ticket, int frame, int64_t tag);
/* the same from HOST arrays in the layout of the store (netvlad [V][netvlad_dim], desc [V][cap][desc_dim] or NULL when every count is 0, n_kp [V]), as blocking
 * copies behind the window's stream: for a window that does not start empty, and for tests */
D2FE_API int d2fe_window_push_host(d2fe_window x, const float* netvlad, const float* desc, const int32_t* n_kp, int64_t tag);
/* updatebySldWin's erase loop (:47-57): drops every keyframe whose tag is not among tags[0..n), except the newest; the order of the rest is kept.  Returns how many
 * were dropped.  Host bookkeeping only -- no launch, no synchronisation: a later push into a freed slot is ordered behind earlier queries by the window's stream. */
D2FE_API int d2fe_window_retain(d2fe_window x, const int64_t* tags, int n);
/* the same rule without a device: tags[0..n) oldest first, keep[0..nkeep); evict_out[i] = 1 for every keyframe that goes (may be NULL).  Returns how many go.
 * d2fe_window_retain uses it. */
D2FE_API int d2fe_window_retain_plan(const int64_t* tags, int n, const int64_t* keep, int nkeep, uint8_t* evict_out);
D2FE_API int d2fe_window_size(d2fe_window x);
D2FE_API int d2fe_window_tags(d2fe_window x, int64_t* tags, int cap_tags);      /* oldest first, at most cap_tags of them; returns the window's size */
/* Tracks nq remote frames.  DEVICE arrays: row q * V + v of each is view v of frame q; the strides count 32-bit words between consecutive rows, so the same call reads
 * the pipes' dense arrays (strides netvlad_dim, cap * desc_dim, 1) and the exchanges' gathered fp32 blocks in place (all three strides d2fe_block_words_d, the bases
 * from d2fe_block_field_offset_d: fields 3, 0, 4, with the window's desc_dim; the plain functions at 256).  Descriptor rows are 16-byte aligned; NetVLAD rows need not be (a block's are only when cap % 4 == 0).  The arrays are
 * read in place and stay valid until the slot was collected.  stream: the hipStream_t that produced them (the window's stream waits for what is queued on it now), or
 * NULL when they are complete.  Refused: a slot that has not been collected (D2FE_ERR_NOT_READY), nq outside 1..max_queries. */
D2FE_API int d2fe_window_track_device(d2fe_window x, const float* d_netvlad, size_t nv_stride, const float* d_desc, size_t desc_stride, const int32_t* d_n_kp,
                                      size_t nkp_stride, int nq, int slot, void* stream);
D2FE_API int d2fe_window_collect(d2fe_window x, int slot, d2fe_window_result* out);      /* blocks until the slot's results are in host memory */

/* Test hooks and kernel diagnostics (d2fe_debug_*) are NOT part of this library: they live in the development library
 * (lib/libd2fe_hip_dev.so, built with -DD2FE_DEVTOOLS) and are declared in include/d2fe_debug.h. */

/* Stage timing with HIP events recorded on the stream the kernels run on.
 * mode 0 = off, 1 = bracket only the dominant kernel (conv1b), 2 = bracket every stage.
 * d2fe_profile_read synchronises, returns the accumulated milliseconds and launch counts per stage since the
 * last d2fe_profile_enable call, and clears them.  Stage order: D2FE_PROF_* below. */
enum {
  D2FE_PROF_CONV1A = 0, D2FE_PROF_CONV1B, D2FE_PROF_CONV2A, D2FE_PROF_CONV2B, D2FE_PROF_CONV3A, D2FE_PROF_CONV3B,
  D2FE_PROF_CONV4A, D2FE_PROF_CONV4B, D2FE_PROF_CONVPADA, D2FE_PROF_CONVPB, D2FE_PROF_CONVDB, D2FE_PROF_SOFTMAX,
  D2FE_PROF_SELECT, D2FE_PROF_SAMPLE, D2FE_PROF_MATCH, D2FE_PROF_NETVLAD, D2FE_PROF_LK, D2FE_PROF_COUNT
};
D2FE_API int d2fe_profile_enable(d2fe_handle h, int mode);
D2FE_API int d2fe_profile_read(d2fe_handle h, float* ms /*[D2FE_PROF_COUNT]*/, int32_t* launches /*[D2FE_PROF_COUNT]*/);

/* Synchronise the handle's stream (for timing with device-resident calls). */
D2FE_API int d2fe_sync(d2fe_handle h);
/* exact_order counters since d2fe_create, over the handle and every pipe lane created from it: out[0] marked candidates, [1] cells re-evaluated,
 * [2] cells dropped for lack of crop slots (the guarantee holds for calls that dropped none), [3] calls.  Synchronises the device.  Zeros when the option is off. */
D2FE_API int d2fe_exact_order_stats(d2fe_handle h, int64_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* D2FE_H_ */
