/*
 * d2fe_debug.h -- test hooks and kernel diagnostics of the DEVELOPMENT library (d2slam_amd/lib/libd2fe_hip_dev.so: the same sources as
 * libd2fe_hip.so compiled with -DD2FE_DEVTOOLS; `python -m d2slam_amd.build --dev`).  The product library exports none of these symbols,
 * reads no environment variable and contains no ablation or trace code.  The development library additionally honours the D2FE_*
 * environment switches listed in tools/README.md (alternate kernel schedules for A/B measurements, phase stamps).
 */
#ifndef D2FE_DEBUG_H_
#define D2FE_DEBUG_H_

#include "d2fe.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Debug/inspection: copy an internal device tensor of the last extract call to the host.
 * names: "conv1a".."conv4b","convPaDa","logits","desc_raw","semi"; "convPa" (256 channels) after a call that took the sparse descriptor head.  Returns bytes copied or <0. */
D2FE_API long d2fe_debug_read(d2fe_handle h, const char* name, void* dst, size_t max_bytes);
/* NetVLAD inspection: output of layer `layer` (NHWC fp32, n_images of the handle's maximum size) of the last d2fe_netvlad* call, when the
 * execution plan materialises it -- the last layer of every fused MobileNetV2 block and every unfused layer; D2FE_ERR_NOT_READY for a
 * layer that only exists in LDS inside a fused block (D2FE_NV_LEGACY=1 in the environment of the development library: one launch per layer, everything readable). */
D2FE_API long d2fe_debug_netvlad_layer(d2fe_handle h, int layer, int n_images, void* dst, size_t max_bytes);
/* Kernel diagnostics (tools/nv_stamps.py): with D2FE_NV_STAMP_STEP=<execution-plan step> in the environment when the network was loaded, the
 * wall_clock64() phase stamps [workgroup][32] (100 MHz ticks) that step's block kernel wrote during the last d2fe_netvlad* call.  Returns the number
 * of workgroups copied (<= max_wgs) or <0. */
D2FE_API long d2fe_debug_netvlad_stamps(d2fe_handle h, unsigned long long* dst, long max_wgs);
/* The execution plan d2fe_load_netvlad builds for this layer list and proj_dim under the D2FE_NV_* switches of the environment (needs no GPU; weights may
 * be NULL).  Writes (kind, first layer, last layer, halves) for each step, at most max_steps, and returns the number of steps or <0.  Kinds: 0 / 1 / 2 one
 * conv / dw / pw layer through the generic launchers, 3 conv -> dw -> pw (nv_block_kernel), 4 pw -> dw -> pw (nv_block_kernel), 5 dw -> pw (nv_block_kernel),
 * 6 nv_xblock_kernel, 7 nv_pblock_kernel (`halves` launches), 8 nv_fpair_kernel, 9 the last pw + the pre-projection (nv_tail_kernel), 10 the same
 * through nv_block_kernel. */
D2FE_API int d2fe_debug_netvlad_plan(const d2fe_nv_layer* layers, int n_layers, int proj_dim, int* out, int max_steps);
/* The (NK = Cin / 4, NT = 16-channel output tiles) pairs nv_pblock_kernel is compiled for, generated from the X-macros its dispatch uses (needs no GPU):
 * family 0 every shape, family 1 the shapes that also exist with merged groups.  Writes (NK, NT) per shape, at most `max` shapes, and returns the number of shapes or <0. */
D2FE_API int d2fe_debug_netvlad_shapes(int family, int* out, int max);
/* NetVLAD inspection: the pre-projected features [n_images][positions][proj_dim] the VLAD stage of the last d2fe_netvlad* call read, partial slabs added in
 * slab order (images of the handle's maximum size, as for d2fe_debug_netvlad_layer).  Returns bytes copied or <0. */
D2FE_API long d2fe_debug_netvlad_features(d2fe_handle h, int n_images, void* dst, size_t max_bytes);
/* How the last d2fe_netvlad* call wrote layer `layer` (-1: the pre-projected features): out[0] = the hidden-channel groups of the step that wrote it,
 * out[1] = the partial slabs left in memory (1 once the slab-sum launch ran).  Returns 0 or <0. */
D2FE_API int d2fe_debug_netvlad_groups(d2fe_handle h, int layer, int* out);
/* nv_pblock_slots: the workgroups of the pixel-pair block shape (Cin, Cout) resident at once on a device of `ncu` compute units with `nbuf` E buffers, which
 * run_netvlad compares a launch with when it merges groups (needs no GPU).  Returns the count or <0. */
D2FE_API long d2fe_debug_netvlad_slots(int cin, int cout, int ncu, int nbuf);
/* One 3x3 / pad 1 layer (cin 64 or 128, ReLU, optional 2x2 max-pool) through the Winograd kernels of D2FE_PREC_F32_WINO, host
 * NHWC buffers in and out; iters > 0 also times `iters` back-to-back launches (HIP events on the handle's stream).  For the
 * layer-level parity tests (tests/test_wino.py, tests/test_launch_regimes.py) and tools/; the product path is d2fe_superpoint_extract*.  Like a pass
 * of the extractor, every launch gets a zeroed work counter unless D2FE_WINO_DYNAMIC=0 was set when the handle was created, so a large enough layer
 * takes the claimed walk. */
/* The host-side weight transform of that mode (U = G g G^T, packed [32-channel group][k-step][row i][lane][4]); needs no GPU.
 * Returns the number of floats written (16 * cin * cout rounded up to 64 channels). */
/* Tile shape the NetVLAD block launchers pick for an Ho x Wo output map (needs no GPU): kind 0 stride-1 blocks, 1 the first block (stride = the first
 * conv's), 2 nv_xblock_kernel (stride 1 or 2). */
D2FE_API int d2fe_debug_netvlad_tile(int kind, int Ho, int Wo, int stride, int* th, int* tw);
/* The host-side weight packing of the NetVLAD block kernels (needs no GPU; tests/test_netvlad_pack_cpu.py): kind 0..5 = expand / depthwise + project
 * records of nv_pblock_kernel, nv_xblock_kernel, nv_tail_kernel (see csrc/debug_hooks.hip).  Returns the number of floats written or <0. */
D2FE_API long d2fe_debug_pack_netvlad(int kind, const float* we, const float* be, const float* wd, const float* bd, const float* wp, int cin, int chid,
                                      int cout, float* out, long max_floats);
D2FE_API long d2fe_debug_pack_wino(const float* weight /*[cout][cin][3][3]*/, int cout, int cin, float* out, long max_floats);
D2FE_API int d2fe_debug_conv3x3_wino(d2fe_handle h, const float* in, int n, int H, int W, int cin, const float* weight,
                                     const float* bias, int cout, int pool, int relu, float* out, int iters, float* ms_per_launch);

/* The SuperPoint tail kernels (csrc/postproc.hip) on injected tensors, for tests/test_postproc_edges.py: host buffers in and out, device buffers of the
 * call's own, the handle's device and stream; no weights needed.  Each hook hands the caller's parameters to the launcher the extractor uses, unchanged.
 * All of them refuse (D2FE_ERR_INVALID) null pointers, n < 1, Hc or Wc below 2, cap < 1 and maps of more than 2^21 pixels.
 * Output buffers start as all-ones words on the device, so an entry the kernels do not write comes back as 0xFFFFFFFF.
 *   softmax_cand: logits [n][Hc*Wc][lstride >= 65] -> semi_out [n][8Hc][8Wc] (when want_semi), cand_out [n][64*Hc*Wc] u64 keys
 *                 (score_bits << 32) | (0xFFFFFFFF - raster) in no particular order, cand_count_out [n].
 *   select_b:     cand [n][cand_cap], cand_count [n] (an entry above cand_cap is refused), semi_or_null [n][H][W] -> kps_xy [n][cap][2], scores [n][cap],
 *                 kps_idx [n][cap], n_out [n]; entries at and beyond n_out are unspecified.
 *   sample_b:     desc_raw [n][Hc*Wc][dstride] read at channel offset dcoff (slotmap_or_null == NULL), or the sparse store [n][max_slots][256] with
 *                 slotmap [n][Hc*Wc] (every entry in [-1, max_slots); -1 = no slot, as the sparse head leaves a cell it did not compute; every cell the
 *                 lists look up, worked out on the host, must name a slot); kps_xy [n][cap][2], n_kp [n] -> desc_out [n][cap][256].
 *   nms2_a:       semi [n][H][W] -> variant A's keypoints: nms2_a_kernel, select_b_kernel (always_sort, no border), and nms2_wrap_fix_kernel when H*W > 65536. */
D2FE_API int d2fe_debug_softmax_cand(d2fe_handle h, const float* logits, int lstride, int n, int Hc, int Wc, float thr, int border, int want_semi,
                                     float* semi_out, unsigned long long* cand_out, int* cand_count_out);
D2FE_API int d2fe_debug_select_b(d2fe_handle h, const unsigned long long* cand, const int* cand_count, long cand_cap, int n, int W, int H, int max_kp, int cap,
                                 int always_sort, const float* semi_or_null, float thr, int border, float* kps_xy, float* scores, int32_t* kps_idx,
                                 int32_t* n_out);
D2FE_API int d2fe_debug_sample_b(d2fe_handle h, const float* desc_raw, int dstride, int dcoff, int n, int Hc, int Wc, const float* kps_xy, const int32_t* n_kp,
                                 int cap, const int32_t* slotmap_or_null, int max_slots, float* desc_out);
/* sample_b with the descriptor PCA behind it (sample_b_pca_kernel, what a d2fe_config.variant_b_pca handle launches): comp [pca_dims][256], mean [256],
 * pca_dims in 1..256 -> desc_out [n][cap][pca_dims] */
D2FE_API int d2fe_debug_sample_b_pca(d2fe_handle h, const float* desc_raw, int dstride, int dcoff, int n, int Hc, int Wc, const float* kps_xy,
                                     const int32_t* n_kp, int cap, const int32_t* slotmap_or_null, int max_slots, const float* comp, const float* mean,
                                     int pca_dims, float* desc_out);
D2FE_API int d2fe_debug_nms2_a(d2fe_handle h, const float* semi, int n, int H, int W, float thr, int dist, int max_kp, int cap, float* kps_xy, float* scores,
                               int32_t* kps_idx, int32_t* n_out);

/* The sparse descriptor head and variant A's descriptor tail (csrc/postproc.hip) on injected tensors, for tests/test_desc_head_edges.py; buffers, refusals and
 * the all-ones start of every output as for the hooks above.
 *   desc_head_sparse: launch_desc_head_sparse -- mark and compact (one launch up to 60 Ki cells, two above), then convDa + ReLU + convDb at the marked cells.
 *                 x [n][Hc*Wc][x_cstride] (a multiple of 4, at least 128; channels 128.. are padding), kps_xy [n][cap][2], n_kp [n]; w_da [256][128][3][3],
 *                 b_da [256], w_db [256][256][1][1], b_db [256], packed here as the extractor packs them.  img_w == 0: variant B's corner rule; else variant
 *                 A's for an img_w x img_h image.  with_mid != 0 hands the launcher a `mid` buffer of min(n, 4) images, 0 none: the launcher's own rule picks
 *                 the kernel form from (n, with_mid).  -> slotmap_out [n][Hc*Wc], cells_out [n][max_slots], count_out [n], store_out [n][max_slots][256].
 *                 At most 2^17 cells per call; max_slots >= 1.
 *   sample_a:     sample_a_kernel, chan_norm_a_kernel, finish_a_kernel.  desc_raw / slotmap_or_null / max_slots as for sample_b; img_w, img_h >= 1;
 *                 scap >= 1 = keypoints per image of the sampling scratch; comp_or_null [pca_dims][256] with mean [256] and pca_dims in 1..256, or NULL
 *                 -> desc_out [n][cap][pca_dims or 256]. */
D2FE_API int d2fe_debug_desc_head_sparse(d2fe_handle h, const float* x, int x_cstride, int n, int Hc, int Wc, const float* kps_xy, const int32_t* n_kp, int cap,
                                         int max_slots, int with_mid, int img_w, int img_h, const float* w_da, const float* b_da, const float* w_db,
                                         const float* b_db, int32_t* slotmap_out, int32_t* cells_out, int32_t* count_out, float* store_out);
D2FE_API int d2fe_debug_sample_a(d2fe_handle h, const float* desc_raw, int dstride, int dcoff, int n, int Hc, int Wc, int img_w, int img_h, const float* kps_xy,
                                 const int32_t* n_kp, int cap, int scap, const int32_t* slotmap_or_null, int max_slots, const float* comp_or_null,
                                 const float* mean, int pca_dims, float* desc_out);

/* ONE layer of the direct SuperPoint conv kernels (csrc/conv.hip, conv_f16.hip, conv_pc.hip, conv1x1.hip) on injected tensors, for
 * tests/test_conv_layer_edges.py: host buffers in and out, device buffers of the call's own, the handle's device and stream.  The hook packs the weights as
 * d2fe_load_superpoint does for the precision, fills ConvArgs from the caller's numbers and calls the launcher, nothing else.
 *   family     0 what the extractor's conv() does in this process (convPb's own kernel where it applies and D2FE_CONV1X1 allows, else launch_conv under
 *                D2FE_CONV_PC / D2FE_CONV64_TILE), 1 the one-tile kernels (launch_conv_tile), 2 the persistent kernels (launch_conv_pc), 3 launch_conv1x1_256_65
 *   precision  0 D2FE_PREC_F32, 1 D2FE_PREC_F16X2, 3 D2FE_PREC_F16
 *   shape      ConvShape of csrc/kernels.h: 0 Cin 64 3x3, 1 Cin 128 3x3 (32-wide tile), 2 Cin 128 3x3 (16-wide tile), 3 Cin 256 1x1, 4 conv1a fused into conv1b
 *   conv64_tile  family 1, shape 0: 1 the 4x32 tile, 0 the 8x32 tile
 *   n, H, W    images and the conv's spatial size (the output is H/2 x W/2, floor, with pool); cout real channels, padded here to whole workgroups
 *   in         the caller's WHOLE input buffer of in_floats floats: channel c of pixel (img, y, x) at img * in_img_stride + (y * W + x) * in_cstride + in_coff + c
 *   out        the caller's WHOLE pre-filled output buffer of out_floats floats, addressed likewise: it is uploaded first and downloaded whole, so what the
 *              kernels do not write keeps the caller's values
 *   frames     shape 4 only: u8 frames, byte (img, y, x) at img * img_istride + y * img_stride + x, img_bytes in all; w1a [64][1][3][3], b1a [64]
 *   ncu        copied into ConvArgs::ncu (0: the handle's device): the persistent kernels size their grids on it
 * weight [cout][cin][k][k], bias [cout].  Refused with D2FE_ERR_INVALID before anything is launched: a (family, shape, pool, relu) the launchers do not compile,
 * strides and offsets of the input that are no multiples of 4 floats (the kernels load float4), and any tensor whose last address lies outside its buffer.
 * Family 3 returns D2FE_ERR_UNSUPPORTED where the launcher answers hipErrorNotSupported (nothing launched; alignment is the launcher's own test there). */
typedef struct d2fe_debug_conv {
  int32_t family, precision, shape, conv64_tile, pool, relu;
  int32_t n, H, W, cout;
  int32_t in_cstride, in_coff;
  int32_t out_cstride, out_coff;
  int32_t img_stride, ncu;
  int64_t in_img_stride, in_floats;
  int64_t out_img_stride, out_floats;
  int64_t img_istride, img_bytes;
} d2fe_debug_conv;
D2FE_API int d2fe_debug_conv_layer(d2fe_handle h, const d2fe_debug_conv* p, const float* weight, const float* bias, const float* in, float* out,
                                   const uint8_t* frames, const float* w1a, const float* b1a);
/* d2fe_debug_conv_layer with the dynamic range of the INPUT tensor added (finite, in [1e-30, 1e30]): the only entry point that accepts precision 5
 * (D2FE_PREC_I8, csrc/conv_i8.hip), for tests/test_i8_layer_edges.py.  The hook packs the int8 weights, s_w and d_c = s_x * s_w[c] as d2fe_load_superpoint and
 * d2fe_set_superpoint_int8_ranges do.  The mode has one-tile kernels only: family 0 and 1 launch them, family 2 and 3 are refused; the pool is compiled with
 * ReLU alone.  For the shape-4 layer in_range is the range of conv1a's output.  Every other precision behaves as in d2fe_debug_conv_layer (in_range unused). */
D2FE_API int d2fe_debug_conv_layer_q(d2fe_handle h, const d2fe_debug_conv* p, const float* weight, const float* bias, const float* in, float* out,
                                     const uint8_t* frames, const float* w1a, const float* b1a, float in_range);
/* The stand-alone conv1a (1 -> 64, 3x3, ReLU) on injected frames: kernel 0 conv1a_mfma_kernel, 1 conv1a_kernel, -1 launch_conv1a's own pick (D2FE_CONV1A_VALU).
 * frames as above; out is the caller's whole pre-filled buffer of out_floats >= n * H * W * 64 floats, uploaded first and downloaded whole. */
D2FE_API int d2fe_debug_conv1a(d2fe_handle h, int kernel, const uint8_t* frames, int img_stride, long long img_istride, long long img_bytes, int n, int H, int W,
                               const float* w1a, const float* b1a, float* out, long long out_floats);

/* The int8 calibration session's parts (csrc/calib.hip; the contract is at d2fe_calib_create in d2fe.h) on injected data, for tests/test_calib_cpu.py and
 * tests/test_calib_edges.py.
 *   calib_ranges_from_hist: the host rule of d2fe_calib_ranges on one histogram; needs no GPU.  hist [n_bins]; t = the tensor's T; method and param as there.
 *                 -> *range, and *index (may be NULL): ENTROPY the winning candidate i, PERCENTILE b + 1, MINMAX and N = 0 n_bins.
 *   calib_stats:  calib_stats_kernel on a host tensor of pixels * ch_stride floats: channel c of pixel p at p * ch_stride + ch_off + c, c < channels.  phase 0:
 *                 the range phase, *t_max_bits = max(*t_max_bits, bits of max |x|).  phase 1: the histogram phase with T = t and scale = (float)n_bins / t.  Every output is
 *                 in-out: uploaded first, downloaded behind the launch, so that a second call accumulates into the first one's counts.  wgs: the launch's
 *                 workgroups, 0 = the launcher's own choice.  Refused: null pointers, t outside [1e-30, 3e38], a bad n_bins, ch_off + channels > ch_stride, more than
 *                 2^28 floats.
 *   calib_conv1a: calib_conv1a_stats_kernel on injected frames and weights (frames, w1a, b1a as for d2fe_debug_conv1a); outputs as for calib_stats. */
D2FE_API int d2fe_debug_calib_ranges_from_hist(const uint64_t* hist, int n_bins, float t, int method, double param, float* range, int* index);
D2FE_API int d2fe_debug_calib_stats(d2fe_handle h, const float* tensor, long long pixels, int ch_off, int channels, int ch_stride, float t, int n_bins, int phase,
                                    int wgs, uint32_t* t_max_bits, uint64_t* hist, uint64_t* n_zero, uint64_t* n_over);
D2FE_API int d2fe_debug_calib_conv1a(d2fe_handle h, const uint8_t* frames, int img_stride, long long img_istride, long long img_bytes, int n, int H, int W,
                                     const float* w1a, const float* b1a, float t, int n_bins, int phase, uint32_t* t_max_bits, uint64_t* hist, uint64_t* n_zero,
                                     uint64_t* n_over);

/* Host-pointer calls replay cached hipGraphs of their launch sequences from the third call with the same geometry on (D2FE_GRAPH=0 in the
 * environment turns that off).  Returns how many graphs the handle holds; *rejected (may be NULL) = geometries whose capture failed and which
 * therefore keep launching kernel by kernel (diagnostic). */
D2FE_API int d2fe_debug_graph_count(d2fe_handle h, int* rejected);

/* Launch-regime record.  Several launchers switch to another code path once a launch is large; the development library counts, process-wide,
 * how many launches each of these paths has taken, so that a test can prove that the path it means to cover ran (the count comes from the
 * launcher, the Winograd claim rule from the one function the kernel itself evaluates).  A launch is counted when the launcher is called: a
 * cached hipGraph that replays a launch sequence counts it once, at capture. */
enum d2fe_regime {
  D2FE_REGIME_WINO_NT1_ONE = 0,          /* Winograd, 32-channel items (NT = 1), one item per workgroup (grid == total) */
  D2FE_REGIME_WINO_NT1_STATIC,           /*   ... persistent workgroups striding through the items */
  D2FE_REGIME_WINO_NT1_CLAIMED,          /*   ... persistent workgroups claiming items from the device counter (only with D2FE_WINO_NT=1 forced on a large launch) */
  D2FE_REGIME_WINO_NT2_ONE,              /* Winograd, 64-channel items (NT = 2), one item per workgroup; ring kernels and the fused conv1a + conv1b kernel */
  D2FE_REGIME_WINO_NT2_STATIC,           /*   ... static walk; ring kernels and the fused kernel */
  D2FE_REGIME_WINO_NT2_CLAIMED_RING,     /*   ... claimed walk of a ring kernel (launch_conv_wino) */
  D2FE_REGIME_WINO_NT2_CLAIMED_FUSED1B,  /*   ... claimed walk of the fused conv1a + conv1b kernel (launch_conv_wino_fused1b) */
  D2FE_REGIME_MATCH_NW4,                 /* matcher, four waves per workgroup (the whole launch resident at once) */
  D2FE_REGIME_MATCH_NW2,                 /* matcher, two waves per workgroup */
  D2FE_REGIME_NV_GMERGE,                 /* NetVLAD nv_pblock_kernel launches in which a workgroup walks several channel groups (gmerge > 1) */
  D2FE_REGIME_NV_FRONT_TPW,              /* NetVLAD nv_fpair_kernel launches with several tiles per workgroup (front_tpw > 1) */
  D2FE_REGIME_WINO_LAST_GRID,            /* not a count: workgroups of the most recent Winograd launch ... */
  D2FE_REGIME_WINO_LAST_TOTAL,           /* ... and its work items */
  D2FE_REGIME_COUNT
};
/* Copies min(max, D2FE_REGIME_COUNT) entries of the record to out (may be NULL with max 0) and returns D2FE_REGIME_COUNT. */
D2FE_API int d2fe_debug_regime_counts(long long* out, int max);
D2FE_API void d2fe_debug_regime_reset(void);

/* The wall_clock64() phase stamps [workgroup][16] of the last d2fe_match_batch_device launch made with D2FE_MATCH_STAMPS=1 in the environment
 * (tools/match_stamps.py).  Returns the number of workgroups copied or <0. */
D2FE_API long d2fe_debug_match_stamps(d2fe_handle h, unsigned long long* dst, long max_wgs);

#ifdef __cplusplus
}
#endif
#endif /* D2FE_DEBUG_H_ */
