// superpoint_host.hip -- SuperPoint's host side: the buffers a context owns to run the network (SpRun), the weight check and packing of
// d2fe_load_superpoint, the descriptor PCA, the launch sequence of an extract call (run_superpoint) with exact_order's crop pass, and the tensor
// read-back of the development library.  Everything that depends on the network's shape takes it from sp_plan.h.  Host code only: api.hip calls in.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "context.h"
#ifdef D2FE_DEVTOOLS
#include "../../include/d2fe_debug.h"
#endif

using namespace d2fe;

static_assert(D2FE_PROF_CONV1A + SP_1B == D2FE_PROF_CONV1B && D2FE_PROF_CONV1A + SP_4B == D2FE_PROF_CONV4B, "a chain layer's profiling stage is D2FE_PROF_CONV1A + its plan index");

namespace {

constexpr int EO_EDGE = 88;      // exact_order's crops

// pack one row of SP_PACK (a conv, or a channel-concatenation of convs sharing the input) into the kernel's fragment order
int pack_layer(SpNet& net, int prec, int li, const d2fe_conv_params* l) {
  const SpPack& K = SP_PACK[li];
  Layer& L = net.L[li];
  const int cin = l[K.part[0]].cin, ks = l[K.part[0]].ksize, cout_pad = K.cout_pad;
  std::vector<float> w, b;
  for (int i = 0; i < K.nparts; ++i) {
    const d2fe_conv_params& p = l[K.part[i]];
    w.insert(w.end(), p.weight, p.weight + (size_t)p.cout * cin * ks * ks);
    b.insert(b.end(), p.bias, p.bias + p.cout);
  }
  const int cout = (int)b.size();
  b.resize(cout_pad, 0.f);
  L.cout = cout; L.cout_pad = cout_pad; L.cin = cin; L.ks = ks;
  net.pool.give_back(L.wpack); L.wpack = nullptr;
  net.pool.give_back(L.bias); L.bias = nullptr;
  net.pool.give_back(L.dscale); L.dscale = nullptr;
  L.s_w.clear(); L.qr = 0.f;
  if (prec == D2FE_PREC_I8 && !K.f32) {      // int8 fragments and s_w; d_c and r follow with the calibration ranges (d2fe_set_superpoint_int8_ranges)
    std::vector<int8_t> pq(packed_weight_bytes_i8(cout_pad, cin, ks));
    L.s_w.resize(cout_pad);
    pack_weights_i8(w.data(), cout, cin, ks, cout_pad, pq.data(), L.s_w.data());
    HIP_TRY(net.pool.get(&L.wpack, pq.size(), pq.data()));
    HIP_TRY(net.pool.get(&L.bias, b.size() * sizeof(float), b.data()));
    HIP_TRY(net.pool.get(&L.dscale, b.size() * sizeof(float), nullptr, 0));
    return D2FE_OK;
  }
  std::vector<float> pf;        // the fragments: fp32 words, or halves
  std::vector<uint16_t> ph;
  if (prec == D2FE_PREC_F32_WINO && ks == 3 && cin >= 64 && !K.f32) {
    pf.resize(packed_weight_floats_wino(cout_pad, cin));
    pack_weights_wino(w.data(), cout, cin, cout_pad, pf.data());
  } else if ((prec != D2FE_PREC_F16X2 && prec != D2FE_PREC_F16) || K.f32) {
    pf.resize(packed_weight_floats_f32(cout_pad, cin, ks));
    pack_weights_f32(w.data(), cout, cin, ks, cout_pad, pf.data());
  } else if (prec == D2FE_PREC_F16) {
    ph.resize(packed_weight_halfs_f16(cout_pad, cin, ks));
    pack_weights_f16(w.data(), cout, cin, ks, cout_pad, ph.data());
  } else {
    ph.resize(packed_weight_halfs_f16x2(cout_pad, cin, ks));
    pack_weights_f16x2(w.data(), cout, cin, ks, cout_pad, ph.data());
  }
  if (pf.empty()) HIP_TRY(net.pool.get(&L.wpack, ph.size() * sizeof(uint16_t), ph.data()));
  else HIP_TRY(net.pool.get(&L.wpack, pf.size() * sizeof(float), pf.data()));
  HIP_TRY(net.pool.get(&L.bias, b.size() * sizeof(float), b.data()));
  return D2FE_OK;
}

// what the launches of one pass over a batch of images share.  crops: exact_order's crop batch -- conv1a always fused, no development switches, no profiling
// stages of its own
struct Pass { d2fe_context* h; int prec; bool crops; const uint8_t* img; int img_stride; long img_istride; int n; hipStream_t s; };

ConvShape conv_shape(int cin, int ks, int level) {
  return ks == 1 ? CONV_256_1x1_T4x16 : cin == 64 ? CONV_64_T8x32 : level < SP_CELL_LEVEL ? CONV_128_T4x32 : CONV_128_T4x16;
}

hipError_t conv(const Pass& p, ConvShape shape, const Layer& L, const float* in, int ics, int ico, long iis, float* out, int ocs, long ois, int hh, int ww, bool pool,
                bool relu, int oco = 0, bool direct = false) {
  const SpNet& net = *p.h->sp_net;
  const SpRun& run = p.h->sp_run;
  ConvArgs a;
  a.in = in; a.in_cstride = ics; a.in_coff = ico;
  a.out = out; a.out_cstride = ocs; a.out_coff = oco;
  a.cout_real = L.cout; a.wpack = L.wpack; a.bias = L.bias;
  a.img = p.img; a.img_stride = p.img_stride; a.img_istride = p.img_istride; a.w1a = net.w1a; a.b1a = net.b1a;
  a.H = hh; a.W = ww; a.n_img = p.n; a.in_img_stride = iis; a.out_img_stride = ois; a.zeros = run.zeros; a.ncu = p.h->ncu;
  a.tag = (&L == &net.L[L_1B]) ? 1 : 0;
  a.qr = L.qr; a.dscale = L.dscale;
  a.work_ctr = (p.prec == D2FE_PREC_F32_WINO && run.wino_dynamic) ? run.work_ctrs + (int)(&L - &net.L[0]) : nullptr;
  { static const int ab = d2fe_dev_env("D2FE_ABLATE", 0); a.ablate = p.crops ? 0 : ab; }
  if (p.prec != D2FE_PREC_F16X2 && p.prec != D2FE_PREC_F16 && p.prec != D2FE_PREC_I8 && shape == CONV_256_1x1_T4x16 && L.cout == 65 && !pool && !relu) {      // convPb: same bits either way
    static const int on = d2fe_dev_env("D2FE_CONV1X1", 1);
    if (on || p.crops) { const hipError_t e = launch_conv1x1_256_65(a, p.s); if (e != hipErrorNotSupported) return e; }
  }
  if (p.prec == D2FE_PREC_F32_WINO)   // 3x3 layers: Winograd kernels; the 1x1 heads (and `direct`: convDa of the dense head): the exact fp32 kernels
    return shape == CONV1B_FUSED ? launch_conv_wino_fused1b(L.cout_pad, a, p.s)
           : (L.ks == 3 && !direct) ? launch_conv_wino(L.cin, pool, relu, L.cout_pad, a, p.s) : launch_conv(shape, D2FE_PREC_F32, pool, relu, L.cout_pad, a, p.s);
  return launch_conv(shape, p.prec, pool, relu, L.cout_pad, a, p.s);
}

// conv1b .. `last` of the plan on H x W images: layer i runs the packing L0[i - SP_1B], reads the output of layer i - 1 and writes act[i].  conv1b reads the
// frames through the fused conv1a, or act[SP_1A] behind the stand-alone conv1a kernel (D2FE_FUSE1A=0)
int run_chain(const Pass& p, const Layer* L0, int last, int H, int W, float* const* act) {
  const SpNet& net = *p.h->sp_net;
  for (int i = SP_1B; i <= last; ++i) {
    const SpLayer& P = SP_PLAN[i];
    const float* in = act[i - 1];
    ConvShape shape = conv_shape(P.cin, P.ks, P.level);
    if (i == SP_1B) {
      if (p.crops || p.h->sp_run.fuse1a) { in = nullptr; shape = CONV1B_FUSED; }
      else { ProfScope ps(p.h, D2FE_PROF_CONV1A, p.s); HIP_TRY(launch_conv1a(p.img, p.img_stride, p.img_istride, H, W, p.n, net.w1a, net.b1a, act[SP_1A], p.s)); }
    }
    ProfScope ps(p.h, D2FE_PROF_CONV1A + i, p.s, !p.crops);
    HIP_TRY(conv(p, shape, L0[i - SP_1B], in, P.cin, 0, in ? (long)sp_floats(P.level, P.cin, H, W) : 0, act[i], P.cout, (long)sp_out_floats(i, H, W), H >> P.level,
                 W >> P.level, P.pool, true));
  }
  return D2FE_OK;
}

// exact_order (exact_order.hip), between the candidate emission and the selection, on the tail's stream: mark -> slots + crops -> the crop batch through the
// exact mode's launches (conv1a|conv1b .. conv4b, convPa, convPb, softmax into a dense 88x88 score map per crop) -> patch.  A fixed number of fixed-shape
// launches: crop slots nobody got run on whatever they held, their scores are never read
int run_exact_order(d2fe_context* h, const uint8_t* d_gray, int n, int W, int H, int stride, size_t image_stride, int cap, hipStream_t s) {
  const SpNet& net = *h->sp_net;
  const SpRun& run = h->sp_run;
  const int C = run.eo_slots, E = EO_EDGE, Ec = E >> SP_CELL_LEVEL;
  const float thr = h->cfg.keypoint_threshold;
  const int K = h->cfg.max_keypoints < cap ? h->cfg.max_keypoints : cap;
  HIP_TRY(launch_exact_order_mark(run.cand, run.cand_count, run.cand_cap, n, W, H, K, thr, run.eo_eps, C, run.eo_cell_map, run.eo_cell_list, run.eo_cell_count,
                                  net.eo_stats, s));
  HIP_TRY(launch_exact_order_gather(d_gray, stride, (long)image_stride, n, W, H, run.eo_cell_list, run.eo_cell_count, C, run.eo_crops, net.eo_stats, s));
  float* act[SP_PB + 2] = {};      // conv1b .. convPb, and the score maps behind them
  for (int i = SP_1B; i <= SP_PB + 1; ++i) act[i] = run.eo_act + (size_t)C * sp_crop_off(i, E);
  float* const sc = act[SP_PB + 1];
  const Pass p{h, D2FE_PREC_F32, true, run.eo_crops, E, (long)E * E, C, s};
  { const int rc = run_chain(p, &net.L[L_X1B], SP_PA, E, E, act); if (rc) return rc; }
  HIP_TRY(conv(p, CONV_256_1x1_T4x16, net.L[L_PB], act[SP_PA], 256, 0, (long)sp_out_floats(SP_PA, E, E), act[SP_PB], 65, (long)sp_out_floats(SP_PB, E, E), Ec, Ec,
               false, false));
  // dense score map only: an infinite threshold emits no candidate and touches no counter
  HIP_TRY(launch_softmax_cand(act[SP_PB], 65, Ec, Ec, C, INFINITY, 0, sc, nullptr, run.eo_cell_count, 0, false, s));
  HIP_TRY(launch_exact_order_patch(run.cand, run.cand_count, run.cand_cap, n, W, H, thr, run.eo_cell_map, run.eo_cell_count, C, sc, s));
  return D2FE_OK;
}

}  // namespace

namespace d2fe {

int SpRun::alloc(const d2fe_config& cfg) {
  release();
  const size_t H = cfg.max_height, W = cfg.max_width, B = cfg.max_batch, ncell = (H / 8) * (W / 8);
  auto floats = [&](float** p, size_t per_img) { return pool.alloc(p, per_img * B * sizeof(float)); };
  // conv1a is evaluated inside conv1b's staging in every mode (the Winograd kernel runs it on the matrix pipe): the 78.6 MB/image
  // activation never exists.  D2FE_FUSE1A=0 falls back to a stand-alone conv1a kernel (bit-identical; kept for A/B measurements); debug reads allocate it on demand
  fuse1a = d2fe_dev_env("D2FE_FUSE1A", 1) != 0;
  for (int i = fuse1a ? SP_1B : SP_1A; i <= SP_PA; ++i) HIP_TRY(floats(&act[i], sp_alloc_floats(i, H, W)));
  HIP_TRY(floats(&logits, ncell * 65));
  HIP_TRY(floats(&draw, sp_alloc_floats(SP_DB, H, W)));
  HIP_TRY(floats(&semi, H * W));
  cand_cap = (long)(H * W);
  HIP_TRY(pool.alloc(&cand, sizeof(unsigned long long) * cand_cap * B));
  // the per-image candidate counters sit directly behind the 64 Winograd work counters: ONE memset clears both at the start of a pass
  const size_t ctr_bytes = (64 + (B + 63) / 64 * 64) * sizeof(int);      // counts padded to 64 ints: see the memset of a pass (run_superpoint)
  HIP_TRY(pool.get(&work_ctrs, ctr_bytes, nullptr, 0));
  cand_count = work_ctrs + 64;
  if (cfg.async_tail) {
    HIP_TRY(floats(&a4b2, sp_alloc_floats(SP_4B, H, W)));
    HIP_TRY(floats(&logits2, ncell * 65));
    HIP_TRY(floats(&draw2, sp_alloc_floats(SP_DB, H, W)));
  }
  sparse_desc = !cfg.dense_descriptors;
  // Winograd mode: both heads evaluate the descriptor branch as direct fp32 chains (run_superpoint), so the choice is free of consequences for the
  // bits; measured per call (host to host, 640x480): 1 image 0.44 ms dense / 0.47 sparse, 2 images 0.69 dense / 0.67 sparse
  if (cfg.precision == D2FE_PREC_F32_WINO) sp_min_batch = 2;
  // fp16-operand mode: the dense head would evaluate convDa | convDb with fp16 operands, the sparse head evaluates them as exact fp32 chains -- a frame's
  // descriptors must not depend on how many images travel with it, so every call takes the sparse head (1 image: 0.03 ms more per call, the figures above)
  if (cfg.precision == D2FE_PREC_F16) sp_min_batch = 1;
  // int8-operand mode: the same reasoning (the dense head would quantise convDa | convDb)
  if (cfg.precision == D2FE_PREC_I8) sp_min_batch = 1;
  sp_min_batch = d2fe_dev_env("D2FE_SPARSE_MIN_BATCH", sp_min_batch);
  if (sparse_desc) {
    sp_slots = 4 * (cfg.max_keypoints < 0 || cfg.max_keypoints > 1024 ? 1024 : cfg.max_keypoints);   // <= 4 corner cells per keypoint; larger calls take the dense head
    HIP_TRY(pool.alloc(&sp_flags, ncell * B));
    HIP_TRY(pool.alloc(&sp_slotmap, sizeof(int32_t) * ncell * B));
    HIP_TRY(pool.alloc(&sp_cells, sizeof(int32_t) * (size_t)sp_slots * B));
    HIP_TRY(pool.alloc(&sp_count, sizeof(int32_t) * B));
    HIP_TRY(pool.alloc(&sp_desc, sizeof(float) * 256 * (size_t)sp_slots * B));
    sp_mid_imgs = B < 4 ? (int)B : 4;
    HIP_TRY(pool.alloc(&sp_mid, sizeof(float) * 256 * (size_t)sp_slots * sp_mid_imgs));
  }
  HIP_TRY(pool.get(&zeros, 1024, nullptr, 0));
  wino_dynamic = d2fe_dev_env("D2FE_WINO_DYNAMIC", 1) != 0;
  if (cfg.postproc == D2FE_POSTPROC_A) {
    HIP_TRY(pool.alloc(&aconf, sizeof(float) * H * W * B));
    HIP_TRY(pool.alloc(&clist, sizeof(int) * H * W * B));
    HIP_TRY(pool.alloc(&a_ncand, sizeof(int) * B));
    a_scap = cfg.max_keypoints > 0 ? cfg.max_keypoints : 1024;   // variant A: select keeps at most min(max_keypoints, call capacity); keep-all: 1024
    HIP_TRY(pool.alloc(&a_samp, sizeof(float) * 256 * (size_t)a_scap * B));
    HIP_TRY(pool.alloc(&a_cn, sizeof(float) * 256 * B));
  }
  if (cfg.exact_order) {
    // measured: max |Winograd score - direct score| over the pixels with a direct score > thr / 2; the default is 4x that, one digit
    eo_eps = cfg.exact_order_eps > 0.f ? cfg.exact_order_eps : 9e-6f;
    // default crop slots: the smallest count in steps of max_batch / 2 at which the 1056-image study (32 images per call, N = 200) drops no cell is 66.5 per image
    // (2121 cells in its fullest call); at least 136 (134 cells in its fullest image) so that a one-image call drops none either
    const int C = cfg.exact_order_crops > 0 ? cfg.exact_order_crops : std::max((133 * (int)B + 1) / 2, 136);
    HIP_TRY(pool.get(&eo_crops, (size_t)C * EO_EDGE * EO_EDGE, nullptr, 0));
    HIP_TRY(pool.alloc(&eo_cell_map, sizeof(int) * ncell * B));
    HIP_TRY(pool.alloc(&eo_cell_list, sizeof(int) * (size_t)C * B));
    HIP_TRY(pool.alloc(&eo_cell_count, sizeof(int) * B));
    HIP_TRY(pool.alloc(&eo_act, sizeof(float) * (size_t)C * sp_crop_floats(EO_EDGE)));
    eo_slots = C;
  }
  return D2FE_OK;
}

// the launch sequence == one TensorRT executeV2 + processOutput of the reference
int run_superpoint(d2fe_context* h, const uint8_t* d_gray, int n, int W, int H, int stride, size_t image_stride,
                   float* d_kps, float* d_scores, float* d_desc, int32_t* d_idx, int cap, int32_t* d_n, hipStream_t s,
                   hipStream_t s_tail, int bs) {
  // s: the convolutions ("trunk"); s_tail (default: s): softmax, selection, descriptor head, sampling ("tail"); bs: buffer set
  const SpNet& net = *h->sp_net;
  const SpRun& run = h->sp_run;
  float* act[SP_PA + 1];
  for (int i = 0; i <= SP_PA; ++i) act[i] = run.act[i];
  if (bs) act[SP_4B] = run.a4b2;
  float* const a4b = act[SP_4B], * const aPD = act[SP_PA];
  float* const logits = bs ? run.logits2 : run.logits;
  float* const draw = bs ? run.draw2 : run.draw;
  h->last_set = bs;
  const int prec = h->cfg.precision;
  // One memset per pass: the Winograd work counters and (when the post-processing runs on this same stream) the per-image candidate
  // counters behind them.  async_tail: the previous call's tail may still be reading ITS counts, so the tail zeroes them itself, in stream order.
  const bool tail_elsewhere = s_tail && s_tail != s;
  const bool wctr = prec == D2FE_PREC_F32_WINO && run.wino_dynamic;
  if (wctr || !tail_elsewhere)
    // the cleared range is padded to a multiple of 64 ints (256 B; the allocation is): the runtime splits a memset whose size is not a multiple of its fill width
    // into an aligned fill and a tail fill -- two ~5 us kernels in front of every pass instead of one (kernel trace of a one-frame pass, round 5)
    HIP_TRY(hipMemsetAsync(wctr ? run.work_ctrs : run.cand_count, 0, ((wctr ? 64 : 0) + (tail_elsewhere ? 0 : (n + 63) / 64 * 64)) * sizeof(int), s));
  const int Hc = H >> SP_CELL_LEVEL, Wc = W >> SP_CELL_LEVEL;
  const Pass p{h, prec, false, d_gray, stride, (long)image_stride, n, s};
  { const int rc = run_chain(p, &net.L[L_1B], SP_4B, H, W, act); if (rc) return rc; }
  // a head layer, on the cells: `ics` / `ocs` channels per cell in the buffers it reads / writes
  auto head = [&](const Layer& L, const float* in, int ics, int ico, float* out, int ocs, bool relu, int oco = 0, bool direct = false) {
    return conv(p, conv_shape(L.cin, L.ks, SP_CELL_LEVEL), L, in, ics, ico, (long)Hc * Wc * ics, out, ocs, (long)Hc * Wc * ocs, Hc, Wc, false, relu, oco, direct);
  };
  // both paths give identical bits; with fewer than 4 images per call the dense head is quicker (the sparse kernels are
  // latency-bound with so few 32-cell workgroups in flight; measured per step, exact mode: 2 images 1.079 ms dense / 1.096 sparse,
  // 4 images 1.877 / 1.862, 8 images 3.42 / 3.28, 16 images 6.48 / 6.20)
  const bool sparse = run.sparse_desc && n >= run.sp_min_batch && 4 * (long)cap <= run.sp_slots;      // a larger capacity than the sparse store was sized for: dense head
  if (sparse) {
    // detector head only (convPa 128->256, convPb); the descriptor head is evaluated after keypoint selection, at the needed cells
    { ProfScope ps(h, D2FE_PROF_CONVPADA, s); HIP_TRY(head(net.L[L_PA], a4b, 128, 0, aPD, 256, true)); }
    { ProfScope ps(h, D2FE_PROF_CONVPB, s); HIP_TRY(head(net.L[L_PB], aPD, 256, 0, logits, 65, false)); }
  } else {
    if (prec == D2FE_PREC_F32_WINO && run.sparse_desc) {
      // Winograd mode, dense head (calls with fewer images than the sparse head pays for): the detector branch convPa as a Winograd layer, the
      // descriptor branch convDa as DIRECT fp32 chains -- the arithmetic of the sparse head -- so that a frame's descriptors are the same bits
      // whichever head a call takes (1-image call, 64-image batch, any pass of the frames-in-flight pipe)
      ProfScope ps(h, D2FE_PROF_CONVPADA, s);
      HIP_TRY(head(net.L[L_PA], a4b, 128, 0, aPD, 512, true));
      HIP_TRY(head(net.L[L_DA32], a4b, 128, 0, aPD, 512, true, 256, true));
    } else
    { ProfScope ps(h, D2FE_PROF_CONVPADA, s); HIP_TRY(head(net.L[L_PADA], a4b, 128, 0, aPD, 512, true)); }
    { ProfScope ps(h, D2FE_PROF_CONVPB, s); HIP_TRY(head(net.L[L_PB], aPD, 512, 0, logits, 65, false)); }
    { ProfScope ps(h, D2FE_PROF_CONVDB, s); HIP_TRY(head(net.L[L_DB], aPD, 512, 256, draw, 256, false)); }
  }
  const bool varA = h->cfg.postproc == D2FE_POSTPROC_A;
  if (s_tail && s_tail != s) {       // trunk done -> tail may start; from here on everything is issued on the tail stream
    HIP_TRY(hipEventRecord(h->ev_trunk[bs], s));
    HIP_TRY(hipStreamWaitEvent(s_tail, h->ev_trunk[bs], 0));
    s = s_tail;
  }
  const bool eo = run.eo_slots > 0 && !varA;      // exact_order: candidates down to thr - eps, the uncertain cells re-evaluated with the direct chains
  { ProfScope ps(h, D2FE_PROF_SOFTMAX, s);
  HIP_TRY(launch_softmax_cand(logits, 65, Hc, Wc, n, eo ? h->cfg.keypoint_threshold - run.eo_eps : h->cfg.keypoint_threshold, h->cfg.remove_borders,
                              (h->cfg.keep_score_map || varA || h->cfg.max_keypoints < 0) ? run.semi : nullptr,
                              run.cand, run.cand_count, varA ? 0 : run.cand_cap, /*zero_counts=*/tail_elsewhere, s)); }
  const float* const pca_comp = net.pca_dims ? net.pca_comp_t : nullptr;
  if (varA) {
    // getKeyPoints + NMS2 (superpoint_common.cpp:12-40,107-177): border = 0, sorted by confidence, max_num
    ProfScope ps(h, D2FE_PROF_SELECT, s);
    HIP_TRY(launch_nms2_a(run.semi, H, W, n, h->cfg.keypoint_threshold, h->cfg.nms_dist, run.aconf, run.clist, run.cand,
                          run.cand_count, run.cand_cap, run.a_ncand, s));
    // variant A's sampling scratch holds a_scap keypoints per image: keep-all (max_keypoints = -1) means "up to a_scap" here
    HIP_TRY(launch_select_b(run.cand, run.cand_count, run.cand_cap, n, W, h->cfg.max_keypoints < 0 ? run.a_scap : h->cfg.max_keypoints, cap, 1, nullptr, H,
                            h->cfg.keypoint_threshold, 0, d_kps, d_scores, d_idx, d_n, s));
    if ((long)H * W > 65536)     // the reference's CV_16UC1 index map wraps above 65 536 candidates; reproduced (no-op below that)
      HIP_TRY(launch_nms2_wrap_fix(run.clist, run.a_ncand, H, W, n, d_kps, d_idx, d_n, cap, s));
  } else {
    ProfScope ps(h, D2FE_PROF_SELECT, s);
    if (eo) { const int rc = run_exact_order(h, d_gray, n, W, H, stride, image_stride, cap, s); if (rc) return rc; }
    // raster indices and keypoints are in score-map coordinates: (W/8)*8 wide.  Keep-all handles also hand over the dense score map:
    // more keypoints than the in-LDS sort takes are compacted from it in raster order (any count up to the call's capacity)
    HIP_TRY(launch_select_b(run.cand, run.cand_count, run.cand_cap, n, Wc * 8, h->cfg.max_keypoints, cap, 0,
                            (h->cfg.keep_score_map || h->cfg.max_keypoints < 0) ? run.semi : nullptr, Hc * 8, h->cfg.keypoint_threshold,
                            h->cfg.remove_borders, d_kps, d_scores, d_idx, d_n, s));
  }
  // the descriptor map the sampling reads: the dense head's, or the sparse head's slots behind the cell -> slot map
  const float* dmap = draw;
  const int32_t* slotmap = nullptr;
  if (sparse) {
    ProfScope ps(h, D2FE_PROF_CONVDB, s);
    HIP_TRY(launch_desc_head_sparse(d_kps, d_n, cap, Hc, Wc, n, a4b, 128, (long)Hc * Wc * 128, net.L[L_DA32].wpack, net.L[L_DA32].bias,
                                    net.L[L_DB32].wpack, net.L[L_DB32].bias, run.sp_flags, run.sp_slotmap, run.sp_cells, run.sp_count,
                                    run.sp_slots, run.sp_desc, run.sp_mid, run.sp_mid_imgs, varA ? W : 0, varA ? H : 0, s));
    dmap = run.sp_desc; slotmap = run.sp_slotmap;
  }
  { ProfScope ps(h, D2FE_PROF_SAMPLE, s);
    if (varA)
      HIP_TRY(launch_sample_a(dmap, 256, 0, Hc, Wc, W, H, n, d_kps, d_n, cap, pca_comp, net.pca_mean, net.pca_dims, run.a_samp, run.a_scap, run.a_cn, slotmap,
                              sparse ? run.sp_slots : 0, d_desc, s));
    else
      HIP_TRY(launch_sample_b(dmap, 256, 0, Hc, Wc, n, d_kps, d_n, cap, slotmap, sparse ? run.sp_slots : 0, pca_comp, net.pca_mean, net.pca_dims, d_desc, s)); }
  h->last_w = W; h->last_h = H; h->last_n = n;
  h->last_gray = d_gray; h->last_stride = stride; h->last_istride = image_stride;
  return D2FE_OK;
}

int run_superpoint_trunk(d2fe_context* h, const uint8_t* d_gray, int n, int W, int H, int stride, size_t image_stride, hipStream_t s) {
  const SpNet& net = *h->sp_net;
  const SpRun& run = h->sp_run;
  float* act[SP_PA + 1];
  for (int i = 0; i <= SP_PA; ++i) act[i] = run.act[i];
  const int Hc = H >> SP_CELL_LEVEL, Wc = W >> SP_CELL_LEVEL;
  const Pass p{h, D2FE_PREC_F32, false, d_gray, stride, (long)image_stride, n, s};
  { const int rc = run_chain(p, &net.L[L_1B], SP_4B, H, W, act); if (rc) return rc; }
  auto head = [&](const Layer& L, const float* in, int ics, int ico, float* out, int ocs, bool relu) {
    return conv(p, conv_shape(L.cin, L.ks, SP_CELL_LEVEL), L, in, ics, ico, (long)Hc * Wc * ics, out, ocs, (long)Hc * Wc * ocs, Hc, Wc, false, relu);
  };
  HIP_TRY(head(net.L[L_PADA], act[SP_4B], 128, 0, act[SP_PA], 512, true));
  HIP_TRY(head(net.L[L_PB], act[SP_PA], 512, 0, run.logits, 65, false));
  HIP_TRY(head(net.L[L_DB], act[SP_PA], 512, 256, run.draw, 256, false));
  h->last_set = 0;
  h->last_w = W; h->last_h = H; h->last_n = n;
  h->last_gray = d_gray; h->last_stride = stride; h->last_istride = image_stride;
  return D2FE_OK;
}

// floats per descriptor row of every extract call, pipe and list of the handle: pca_dims can only be non-zero where the PCA is applied (variant A, or variant B
// with d2fe_config.variant_b_pca: d2fe_set_superpoint_pca refuses every other handle)
int desc_dim_of(const d2fe_context* h) { return h->sp_net->pca_dims ? h->sp_net->pca_dims : 256; }

const char* sp_not_ready(const d2fe_context* h) {
  if (!h->sp_net->sp_loaded) return "superpoint weights not loaded";
  if (h->cfg.precision == D2FE_PREC_I8 && !h->sp_net->i8_ranges) return "D2FE_PREC_I8: the calibration ranges are not set (d2fe_set_superpoint_int8_ranges)";
  return nullptr;
}

int check_geometry(d2fe_context* h, int n, int W, int H, int stride, int cap) {
  if (!h) return fail(D2FE_ERR_INVALID, "null handle");
  if (const char* why = sp_not_ready(h)) return fail(D2FE_ERR_NOT_READY, why);
  if (n < 1 || n > h->cfg.max_batch) return fail(D2FE_ERR_INVALID, "batch size out of range");
  if (W < 16 || H < 16 || W > h->cfg.max_width || H > h->cfg.max_height || (long)W * H > (long)h->cfg.max_width * h->cfg.max_height)
    return fail(D2FE_ERR_INVALID, "image size must be at least 16x16 and within the configured maximum");
  // Sizes that are not multiples of 8 (the reference's TensorRT profile admits 100x100 .. 1500x1500, superpoint_tensorrt.cpp:50-55): the
  // three 2x2 max-pools floor, the score map is (H/8)*8 x (W/8)*8 and keypoints live in ITS coordinates, as processOutput reads
  // semi_dims_ (:331-336).  Variant A sizes its cv::Mat views from the configured width/height (superpoint_onnx.cpp:86-94), which only
  // describes the network output for multiples of 8.
  if (((W | H) & 7) && h->cfg.postproc == D2FE_POSTPROC_A)
    return fail(D2FE_ERR_INVALID, "post-processing variant A needs image sizes that are multiples of 8");
  if (h->sp_run.eo_slots > 0 && (W < EO_EDGE || H < EO_EDGE || ((W | H) & 7)))
    return fail(D2FE_ERR_INVALID, "exact_order needs images of at least 88x88 whose width and height are multiples of 8 (the 88x88 crops share the full image's pool grids)");
  if (stride < W) return fail(D2FE_ERR_INVALID, "stride < width");
  if (cap < 1) return fail(D2FE_ERR_INVALID, "cap < 1");
  return D2FE_OK;
}

}  // namespace d2fe

extern "C" {

int d2fe_load_superpoint(d2fe_handle h, const d2fe_superpoint_weights* w) {
  if (h && h->life.pipes() > 0) return fail(D2FE_ERR_INVALID, "the handle has live pipes whose lanes read its packed weights: destroy them before loading weights or PCA matrices");
  if (h) graphs_clear(h);
  if (!h || !w) return fail(D2FE_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  for (int i = 0; i < SP_NLAYERS; ++i) {
    const d2fe_conv_params& p = w->layer[i];
    if (!p.weight || !p.bias || p.cout != SP_PLAN[i].cout || p.cin != SP_PLAN[i].cin || p.ksize != SP_PLAN[i].ks)
      return fail(D2FE_ERR_INVALID, std::string("superpoint layer ") + SP_PLAN[i].name + ": unexpected shape");
  }
  SpNet& net = *h->sp_net;
  net.sp_loaded = false;
  net.i8_ranges = false;
  // conv1a: [64][1][3][3] -> [9][64]
  {
    std::vector<float> t(9 * 64);
    for (int co = 0; co < 64; ++co)
      for (int k = 0; k < 9; ++k) t[k * 64 + co] = w->layer[SP_1A].weight[co * 9 + k];
    net.pool.give_back(net.w1a); net.w1a = nullptr;
    net.pool.give_back(net.b1a); net.b1a = nullptr;
    HIP_TRY(net.pool.get(&net.w1a, t.size() * sizeof(float), t.data()));
    HIP_TRY(net.pool.get(&net.b1a, 64 * sizeof(float), w->layer[SP_1A].bias));
  }
  for (int i = 0; i < L_COUNT; ++i) {
    if ((SP_PACK[i].when == SP_WITH_SPARSE && !h->sp_run.sparse_desc) || (SP_PACK[i].when == SP_WITH_EXACT && h->sp_run.eo_slots <= 0)) continue;
    int rc = pack_layer(net, h->cfg.precision, i, w->layer);
    if (rc) return rc;
  }
  net.sp_loaded = true;
  return D2FE_OK;
}

int d2fe_set_superpoint_int8_ranges(d2fe_handle h, const float* range, int n) {
  if (h && h->life.pipes() > 0) return fail(D2FE_ERR_INVALID, "the handle has live pipes whose lanes read its packed weights: destroy them before setting the int8 ranges");
  if (h) graphs_clear(h);
  if (!h || !range) return fail(D2FE_ERR_INVALID, "null argument");
  if (h->cfg.precision != D2FE_PREC_I8) return fail(D2FE_ERR_INVALID, "int8 ranges belong to a D2FE_PREC_I8 handle");
  if (n != SP_NLAYERS) return fail(D2FE_ERR_INVALID, "n must be D2FE_SP_NUM_LAYERS");
  SpNet& net = *h->sp_net;
  if (!net.sp_loaded) return fail(D2FE_ERR_NOT_READY, "superpoint weights not loaded");
  // the tensor a plan layer reads: the chain's predecessor; convPb reads convPa, convDa conv4b (as convPa does), convDb convDa
  auto input_of = [](int layer) { return layer == SP_PB ? SP_PA : layer == SP_DA ? SP_4B : layer == SP_DB ? SP_DA : layer - 1; };
  for (int i = 0; i < SP_NLAYERS; ++i) {
    if (i == SP_PB || i == SP_DB) continue;      // no quantised layer reads them
    if (!(range[i] >= 1e-30f && range[i] <= 1e30f)) return fail(D2FE_ERR_INVALID, std::string("int8 range of layer ") + SP_PLAN[i].name + " must be finite and in [1e-30, 1e30]");
  }
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (h->tail_stream) HIP_TRY(hipStreamSynchronize(h->tail_stream));
  net.i8_ranges = false;
  for (int i = 0; i < L_COUNT; ++i) {
    Layer& L = net.L[i];
    if (SP_PACK[i].f32 || !L.dscale) continue;
    const float T = range[input_of(SP_PACK[i].part[0])];
    const float s_x = T / 127.0f;
    L.qr = 127.0f / T;
    std::vector<float> d(L.cout_pad);
    for (int c = 0; c < L.cout_pad; ++c) d[c] = s_x * L.s_w[c];
    HIP_TRY(hipMemcpy(L.dscale, d.data(), d.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  net.i8_ranges = true;
  return D2FE_OK;
}

int d2fe_set_superpoint_pca(d2fe_handle h, const float* comp, const float* mean, int pca_dims) {
  if (h && h->life.pipes() > 0) return fail(D2FE_ERR_INVALID, "the handle has live pipes whose lanes read its packed weights: destroy them before loading weights or PCA matrices");
  if (h) graphs_clear(h);
  if (!h) return fail(D2FE_ERR_INVALID, "null handle");
  if (pca_dims < 0 || pca_dims > 256 || (pca_dims > 0 && (!comp || !mean))) return fail(D2FE_ERR_INVALID, "bad PCA arguments");
  if (pca_dims > 0 && h->cfg.postproc != D2FE_POSTPROC_A && !h->cfg.variant_b_pca)
    return fail(D2FE_ERR_UNSUPPORTED, "PCA is only applied by post-processing variant A (the reference's variant B never applies it)");
  // variant B's rows feed the matcher, the pipes and the exchange blocks directly: their length keeps the matcher's 16-byte row alignment
  if (pca_dims > 0 && h->cfg.postproc == D2FE_POSTPROC_B && (pca_dims < 4 || (pca_dims & 3)))
    return fail(D2FE_ERR_INVALID, "variant B takes pca_dims in 4..256 that are multiples of 4 (the matcher's row alignment), or 0 to switch the PCA off");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  HIP_TRY(hipStreamSynchronize(h->stream));
  SpNet& net = *h->sp_net;
  net.pool.give_back(net.pca_comp_t); net.pca_comp_t = nullptr;
  net.pool.give_back(net.pca_mean); net.pca_mean = nullptr;
  net.pca_dims = 0;
  if (pca_dims == 0) return D2FE_OK;
  std::vector<float> t((size_t)256 * pca_dims);
  for (int j = 0; j < pca_dims; ++j)
    for (int c = 0; c < 256; ++c) t[(size_t)c * pca_dims + j] = comp[(size_t)j * 256 + c];
  HIP_TRY(net.pool.get(&net.pca_comp_t, t.size() * sizeof(float), t.data()));
  HIP_TRY(net.pool.get(&net.pca_mean, 256 * sizeof(float), mean));
  net.pca_dims = pca_dims;
  return D2FE_OK;
}

int d2fe_desc_dim(d2fe_handle h) {
  if (!h) return fail(D2FE_ERR_INVALID, "null handle");
  return desc_dim_of(h);
}

#ifdef D2FE_DEVTOOLS      /* development library only: include/d2fe_debug.h */
long d2fe_debug_read(d2fe_handle h, const char* name, void* dst, size_t max_bytes) {
  if (!h || !name || !dst) return fail(D2FE_ERR_INVALID, "null argument");
  if (h->last_n == 0) return fail(D2FE_ERR_NOT_READY, "no extract call yet");
  hipSetDevice(h->cfg.device_id);
  SpRun& run = h->sp_run;
  const int H = h->last_h, W = h->last_w, n = h->last_n;
  if (!strcmp(name, "conv1a") && run.fuse1a) {
    // fused mode never materialises conv1a: evaluate it on demand from the last input frame(s)
    if (!run.act[SP_1A] &&
        run.pool.alloc(&run.act[SP_1A], sp_alloc_floats(SP_1A, h->cfg.max_height, h->cfg.max_width) * h->cfg.max_batch * sizeof(float)) != hipSuccess)
      return fail(D2FE_ERR_HIP, "hipMalloc conv1a debug buffer");
    if (launch_conv1a(h->last_gray, h->last_stride, (long)h->last_istride, H, W, n, h->sp_net->w1a, h->sp_net->b1a, run.act[SP_1A], h->stream) != hipSuccess)
      return fail(D2FE_ERR_HIP, "conv1a debug launch");
  }
  const bool sparse = run.sparse_desc && h->last_n >= run.sp_min_batch;
  if (!strcmp(name, "semi") && !h->cfg.keep_score_map) return fail(D2FE_ERR_NOT_READY, "score map not kept (set keep_score_map)");
  if (sparse && (!strcmp(name, "desc_raw") || !strcmp(name, "convPaDa")))
    return fail(D2FE_ERR_NOT_READY, "the dense descriptor map does not exist with the sparse descriptor head (set dense_descriptors)");
  if (!strcmp(name, "convPa") && !sparse)
    return fail(D2FE_ERR_NOT_READY, "convPa alone exists only behind the sparse descriptor head (the dense head writes convPaDa)");
  // a layer's output under its own name, sized by the plan (the pools floor, sizes need not be multiples of 8); convPa: the detector branch alone, what the
  // sparse descriptor head leaves in the convPa | convDa buffer; the heads' outputs under their names
  const float* src = nullptr;
  size_t per = 0;
  for (int i = SP_1A; i <= SP_PA; ++i)
    if (!strcmp(name, SP_PLAN[i].name)) { src = i == SP_4B && h->last_set ? run.a4b2 : run.act[i]; per = sp_out_floats(i, H, W); }
  const struct { const char* nm; const float* p; int ch; } heads[] = {
      {"convPaDa", run.act[SP_PA], SP_PADA_COUT}, {"logits", h->last_set ? run.logits2 : run.logits, 65}, {"desc_raw", h->last_set ? run.draw2 : run.draw, 256}, {"semi", run.semi, 64}};
  for (auto& e : heads)
    if (!strcmp(name, e.nm)) { src = e.p; per = sp_floats(SP_CELL_LEVEL, e.ch, H, W); }
  if (!src) return fail(D2FE_ERR_INVALID, "unknown tensor name");
  const size_t bytes = per * n * sizeof(float);
  if (bytes > max_bytes) return fail(D2FE_ERR_TRUNCATED, "destination too small");
  if (hipStreamSynchronize(h->stream) != hipSuccess || (h->tail_stream && hipStreamSynchronize(h->tail_stream) != hipSuccess)) return fail(D2FE_ERR_HIP, "sync");
  if (hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) != hipSuccess) return fail(D2FE_ERR_HIP, "D2H");
  return (long)bytes;
}
#endif

}  // extern "C"
