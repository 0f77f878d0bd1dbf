// debug_hooks.hip -- the development library's hooks (include/d2fe_debug.h) that need nothing of the handle but its device and stream: the launch-regime
// record, the host-side packings, one Winograd layer, one layer of the direct conv kernels and the stand-alone conv1a, the SuperPoint tail kernels, the sparse descriptor head and variant A's descriptor tail on injected
// tensors, the calibration session's kernels and range rules (calib.hip), the count of captured launch sequences.  (The hooks that read a unit's own state back live with that state: d2fe_debug_read in
// superpoint_host.hip, the NetVLAD ones in netvlad_host.hip, the matcher's stamps in match_host.hip.)  The whole unit compiles to nothing for the product library.
#ifdef D2FE_DEVTOOLS
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "context.h"
#include "conv_common.h"      // tune_conv_pc, tune_conv64: the switches launch_conv reads
#include "../../include/d2fe_debug.h"

using namespace d2fe;

// launch-regime record (kernels.h: D2FE_REGIME): process-wide, written by the launchers from any thread (pipe lanes)
namespace {
std::atomic<long long> g_regime[D2FE_REGIME_COUNT];
}  // namespace
namespace d2fe {
void regime_note(int regime) { if (regime >= 0 && regime < D2FE_REGIME_COUNT) g_regime[regime].fetch_add(1, std::memory_order_relaxed); }
void regime_set(int regime, long long value) { if (regime >= 0 && regime < D2FE_REGIME_COUNT) g_regime[regime].store(value, std::memory_order_relaxed); }
}  // namespace d2fe

extern "C" {

int d2fe_debug_regime_counts(long long* out, int max) {
  for (int i = 0; out && i < max && i < D2FE_REGIME_COUNT; ++i) out[i] = g_regime[i].load(std::memory_order_relaxed);
  return D2FE_REGIME_COUNT;
}
void d2fe_debug_regime_reset(void) {
  for (auto& c : g_regime) c.store(0, std::memory_order_relaxed);
}

// Host-side half of the Winograd mode, callable without a GPU: U = G g G^T in the kernels' fragment order (see pack_weights_wino).
long d2fe_debug_pack_wino(const float* weight, int cout, int cin, float* out, long max_floats) {
  if (!weight || !out || cout < 1 || cin < 8 || (cin & 7)) return fail(D2FE_ERR_INVALID, "bad argument");
  const int cout_pad = (cout + 63) / 64 * 64;
  const size_t n = packed_weight_floats_wino(cout_pad, cin);
  if ((long)n > max_floats) return fail(D2FE_ERR_TRUNCATED, "destination too small");
  pack_weights_wino(weight, cout, cin, cout_pad, out);
  return (long)n;
}

// Tile shape the NetVLAD block launchers pick for an Ho x Wo output map (no GPU needed; tests/test_netvlad_pack_cpu.py sweeps it against the kernels' limits):
// kind 0 nv_pblock_kernel (stride 1), kind 1 nv_fpair_kernel (first block; c0_stride = stride of the first conv), kind 2 nv_xblock_kernel (stride = 1 or 2).
int d2fe_debug_netvlad_tile(int kind, int Ho, int Wo, int stride, int* th, int* tw) {
  if (!th || !tw || Ho < 1 || Wo < 1 || stride < 1 || stride > 2) return fail(D2FE_ERR_INVALID, "bad argument");
  if (kind == 0) nv_pblock_tile(Ho, Wo, th, tw, 0);
  else if (kind == 1) nv_pblock_tile(Ho, Wo, th, tw, stride);
  else if (kind == 2) nv_xblock_tile(Ho, Wo, stride, th, tw);
  else return fail(D2FE_ERR_INVALID, "kind");
  return D2FE_OK;
}

// Host-side weight packing of the NetVLAD block kernels, callable without a GPU (tests/test_netvlad_pack_cpu.py):
//   kind 0 expand record of nv_pblock_kernel (pack_nv_expand_pair)      kind 1 depthwise + project record of nv_pblock / nv_fpair (pack_nv_dwproj_pair)
//   kind 2 expand record of nv_xblock_kernel (pack_nv_expand_perm)      kind 3 depthwise + project record of nv_xblock_kernel (pack_nv_dwproj_x)
//   kind 4 expand record of nv_tail_kernel (pack_nv_expand_tail)        kind 5 project record of nv_tail_kernel (pack_nv_proj_t)
// we [chid][cin], be [chid], wd [chid][9], bd [chid], wp [cout][chid]; returns the number of floats written or <0.
long d2fe_debug_pack_netvlad(int kind, const float* we, const float* be, const float* wd, const float* bd, const float* wp, int cin, int chid,
                             int cout, float* out, long max_floats) {
  if (!out || cin < 8 || (cin & 7) || chid < 16 || (chid & 15) || cout < 1) return fail(D2FE_ERR_INVALID, "bad argument");
  const int nt = kind <= 1 ? nv_pblock_ntiles(cout) : nv_block_ntiles(cout);
  if (nt < 0) return fail(D2FE_ERR_UNSUPPORTED, "cout");
  size_t n = 0;
  switch (kind) {
    case 0: n = pack_nv_expand_pair_floats(chid, cin); break;
    case 1: n = pack_nv_dwproj_pair_floats(chid, nt); break;
    case 2: if (!nv_xblock_supported(cin, chid, cout, 1)) return fail(D2FE_ERR_UNSUPPORTED, "shape"); n = pack_nv_expand_perm_floats(chid, cin); break;
    case 3: case 5: n = pack_nv_dwproj_floats(chid, nt); break;
    case 4: if (!nv_tail_supported(cin, cout)) return fail(D2FE_ERR_UNSUPPORTED, "shape"); n = pack_nv_expand_floats(chid, cin); break;
    default: return fail(D2FE_ERR_INVALID, "kind");
  }
  if ((long)n > max_floats) return fail(D2FE_ERR_TRUNCATED, "destination too small");
  if (((kind == 0 || kind == 2 || kind == 4) && (!we || !be)) || ((kind == 1 || kind == 3) && (!wd || !bd || !wp)) || (kind == 5 && !wp))
    return fail(D2FE_ERR_INVALID, "null weights");
  switch (kind) {
    case 0: pack_nv_expand_pair(we, be, chid, cin, out); break;
    case 1: pack_nv_dwproj_pair(wd, bd, wp, cout, chid, nt, out); break;
    case 2: pack_nv_expand_perm(we, be, chid, cin, out); break;
    case 3: pack_nv_dwproj_x(wd, bd, wp, cout, chid, nt, out); break;
    case 4: pack_nv_expand_tail(we, be, chid, cin, out); break;
    case 5: pack_nv_proj_t(wp, cout, chid, nt, out); break;
  }
  return (long)n;
}

// One 3x3 layer through the Winograd kernels, host buffers in and out (layer-level parity tests and timing; not a product path).
int d2fe_debug_conv3x3_wino(d2fe_handle h, const float* in, int n, int H, int W, int cin, const float* weight, const float* bias,
                            int cout, int pool, int relu, float* out, int iters, float* ms_per_launch) {
  if (!h || !in || !weight || !bias || !out) return fail(D2FE_ERR_INVALID, "null argument");
  if ((cin != 64 && cin != 128) || cout < 1 || n < 1 || H < 2 || W < 2 || (pool && ((H | W) & 1)) || !relu)
    return fail(D2FE_ERR_INVALID, "unsupported layer shape");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  const int cout_pad = (cout + 63) / 64 * 64;
  const int Ho = pool ? H / 2 : H, Wo = pool ? W / 2 : W;
  const size_t in_fl = (size_t)n * H * W * cin, out_fl = (size_t)n * Ho * Wo * cout;
  if ((size_t)H * W * cin * 4 >= (1ull << 31)) return fail(D2FE_ERR_INVALID, "image too large");
  std::vector<float> pk(packed_weight_floats_wino(cout_pad, cin)), bp(cout_pad, 0.f);
  pack_weights_wino(weight, cout, cin, cout_pad, pk.data());
  memcpy(bp.data(), bias, sizeof(float) * cout);
  // as a pass of run_superpoint: the work counter is zero when the launch starts (the last of the handle's 64, which no layer of the network uses)
  int* const wctr = h->sp_run.wino_dynamic ? h->sp_run.work_ctrs + 63 : nullptr;
  auto launch = [&](const ConvArgs& ca) {
    if (wctr) { const hipError_t e = hipMemsetAsync(wctr, 0, sizeof(int), h->stream); if (e != hipSuccess) return e; }
    return launch_conv_wino(cin, pool != 0, relu != 0, cout_pad, ca, h->stream);
  };
  DevPool b;
  float *d_in = nullptr, *d_out = nullptr, *d_w = nullptr, *d_b = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int rc = [&]() -> int {
    HIP_TRY(b.get(&d_in, in_fl * 4, in));
    HIP_TRY(b.get(&d_out, out_fl * 4, nullptr));
    HIP_TRY(b.get(&d_w, pk.size() * 4, pk.data()));
    HIP_TRY(b.get(&d_b, bp.size() * 4, bp.data()));
    HIP_TRY(hipDeviceSynchronize());      // the null-stream memset is not ordered with the handle's non-blocking stream
    ConvArgs a{};
    a.in = d_in; a.in_cstride = cin; a.in_coff = 0; a.out = d_out; a.out_cstride = cout; a.out_coff = 0;
    a.cout_real = cout; a.wpack = d_w; a.bias = d_b; a.H = H; a.W = W; a.n_img = n;
    a.in_img_stride = (long)H * W * cin; a.out_img_stride = (long)Ho * Wo * cout; a.zeros = h->sp_run.zeros; a.ncu = h->ncu;
    a.ablate = d2fe_dev_env("D2FE_ABLATE", 0);
    a.work_ctr = wctr;
    HIP_TRY(launch(a));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(out, d_out, out_fl * 4, hipMemcpyDeviceToHost));
    if (iters > 0 && ms_per_launch) {
      HIP_TRY(hipEventCreate(&e0));
      HIP_TRY(hipEventCreate(&e1));
      HIP_TRY(hipEventRecord(e0, h->stream));
      for (int i = 0; i < iters; ++i) HIP_TRY(launch(a));
      HIP_TRY(hipEventRecord(e1, h->stream));
      HIP_TRY(hipEventSynchronize(e1));
      float ms = 0.f;
      HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
      *ms_per_launch = ms / iters;
    }
    return D2FE_OK;
  }();
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  return rc;
}

// ---- the SuperPoint tail kernels of postproc.hip on injected tensors (tests/test_postproc_edges.py): host buffers in and out, the hook's own device
// buffers, the handle's device and stream, no weights.  Each hook calls the launch_* function of kernels.h with the caller's parameters and nothing else.
namespace {
constexpr long DEBUG_MAX_PIXELS = 1l << 21;
}  // namespace

int d2fe_debug_softmax_cand(d2fe_handle h, const float* logits, int lstride, int n, int Hc, int Wc, float thr, int border, int want_semi, float* semi_out,
                            unsigned long long* cand_out, int* cand_count_out) {
  if (!h || !logits || !cand_out || !cand_count_out || (want_semi && !semi_out)) return fail(D2FE_ERR_INVALID, "null argument");
  if (n < 1 || Hc < 2 || Wc < 2 || lstride < 65 || (long)Hc * Wc * 64 > DEBUG_MAX_PIXELS) return fail(D2FE_ERR_INVALID, "bad geometry");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  const size_t ncell = (size_t)Hc * Wc, hw = ncell * 64;
  const long cand_cap = (long)hw;
  DevPool b;
  float *d_l = nullptr, *d_semi = nullptr;
  unsigned long long* d_cand = nullptr;
  int* d_cnt = nullptr;
  HIP_TRY(b.get(&d_l, sizeof(float) * n * ncell * lstride, logits));
  if (want_semi) HIP_TRY(b.get(&d_semi, sizeof(float) * n * hw, nullptr));
  HIP_TRY(b.get(&d_cand, sizeof(unsigned long long) * n * cand_cap, nullptr));
  HIP_TRY(b.get(&d_cnt, sizeof(int) * n, nullptr));
  HIP_TRY(hipDeviceSynchronize());      // the null-stream copies and memsets are not ordered with the handle's non-blocking stream
  HIP_TRY(launch_softmax_cand(d_l, lstride, Hc, Wc, n, thr, border, d_semi, d_cand, d_cnt, cand_cap, /*zero_counts=*/true, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (want_semi) HIP_TRY(hipMemcpy(semi_out, d_semi, sizeof(float) * n * hw, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(cand_out, d_cand, sizeof(unsigned long long) * n * cand_cap, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(cand_count_out, d_cnt, sizeof(int) * n, hipMemcpyDeviceToHost));
  return D2FE_OK;
}

int d2fe_debug_select_b(d2fe_handle h, const unsigned long long* cand, const int* cand_count, long cand_cap, int n, int W, int H, int max_kp, int cap,
                        int always_sort, const float* semi_or_null, float thr, int border, float* kps_xy, float* scores, int32_t* kps_idx, int32_t* n_out) {
  if (!h || !cand || !cand_count || !kps_xy || !scores || !kps_idx || !n_out) return fail(D2FE_ERR_INVALID, "null argument");
  if (n < 1 || W < 1 || H < 1 || cap < 1 || cand_cap < 1 || (long)H * W > DEBUG_MAX_PIXELS || cand_cap > DEBUG_MAX_PIXELS || cap > DEBUG_MAX_PIXELS)
    return fail(D2FE_ERR_INVALID, "bad geometry");
  for (int i = 0; i < n; ++i)
    if (cand_count[i] < 0 || cand_count[i] > cand_cap) return fail(D2FE_ERR_INVALID, "cand_count entry outside [0, cand_cap]");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  const size_t hw = (size_t)H * W;
  DevPool b;
  unsigned long long* d_cand = nullptr;
  int* d_cnt = nullptr;
  float *d_semi = nullptr, *d_kps = nullptr, *d_sc = nullptr;
  int32_t *d_idx = nullptr, *d_n = nullptr;
  HIP_TRY(b.get(&d_cand, sizeof(unsigned long long) * n * cand_cap, cand));
  HIP_TRY(b.get(&d_cnt, sizeof(int) * n, cand_count));
  if (semi_or_null) HIP_TRY(b.get(&d_semi, sizeof(float) * n * hw, semi_or_null));
  HIP_TRY(b.get(&d_kps, sizeof(float) * 2 * n * cap, nullptr));
  HIP_TRY(b.get(&d_sc, sizeof(float) * n * cap, nullptr));
  HIP_TRY(b.get(&d_idx, sizeof(int32_t) * n * cap, nullptr));
  HIP_TRY(b.get(&d_n, sizeof(int32_t) * n, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(launch_select_b(d_cand, d_cnt, cand_cap, n, W, max_kp, cap, always_sort, d_semi, H, thr, border, d_kps, d_sc, d_idx, d_n, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(kps_xy, d_kps, sizeof(float) * 2 * n * cap, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(scores, d_sc, sizeof(float) * n * cap, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(kps_idx, d_idx, sizeof(int32_t) * n * cap, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(n_out, d_n, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  return D2FE_OK;
}

// The cells a sampler looks up for one keypoint, restated on the host from the reference lines sample_b_corners and sample_a_origin (postproc.hip) cite; host and
// device code are both compiled with -ffp-contract=off.  img_w > 0: variant A's corners, -1 where one is padding; else variant B's clipped corners.
static void lookup_cells(float x, float y, int Hc, int Wc, int img_w, int img_h, int cell[4]) {
  float ix, iy;
  if (img_w > 0) {
    const float gx = 2.0f * x / (float)img_w - 1.0f, gy = 2.0f * y / (float)img_h - 1.0f;
    ix = ((gx + 1.0f) * (float)Wc - 1.0f) / 2.0f;
    iy = ((gy + 1.0f) * (float)Hc - 1.0f) / 2.0f;
  } else {
    float k0 = (float)((double)(x - 4.0f) + 0.5), k1 = (float)((double)(y - 4.0f) + 0.5);
    k0 = (float)((double)k0 / ((double)(Wc * 8 - 4) - 0.5));
    k1 = (float)((double)k1 / ((double)(Hc * 8 - 4) - 0.5));
    k0 = k0 * 2.0f - 1.0f;
    k1 = k1 * 2.0f - 1.0f;
    ix = ((k0 + 1.0f) / 2.0f) * (float)(Wc - 1);
    iy = ((k1 + 1.0f) / 2.0f) * (float)(Hc - 1);
  }
  // (int)floorf as the device converts: NaN -> 0, out of range -> saturated (here: to just outside the map, which clips and tests the same)
  auto fl = [](float v, int n) { const float f = floorf(v); return f != f ? 0 : f < -2.f ? -2 : f > (float)(n + 1) ? n + 1 : (int)f; };
  auto clip = [](int v, int n) { return v < 0 ? 0 : (v < n - 1 ? v : n - 1); };
  int x0 = fl(ix, Wc), y0 = fl(iy, Hc);
  if (img_w <= 0) { x0 = clip(x0, Wc); y0 = clip(y0, Hc); }
  for (int q = 0; q < 4; ++q) {
    int xx = x0 + (q & 1), yy = y0 + (q >> 1);
    if (img_w <= 0) { xx = clip(xx, Wc); yy = clip(yy, Hc); }
    cell[q] = (xx >= 0 && xx < Wc && yy >= 0 && yy < Hc) ? yy * Wc + xx : -1;
  }
}

// The slot map of a sampler hook: an entry names a slot of the store or is -1 (no slot, as the sparse head leaves a cell it did not compute), and every cell the
// first kmax keypoints of a list look up names a slot.
static int check_slotmap(const int32_t* slotmap, int max_slots, int n, int Hc, int Wc, int img_w, int img_h, const float* kps_xy, const int32_t* n_kp, int cap,
                         int kmax) {
  if (max_slots < 1 || max_slots > DEBUG_MAX_PIXELS) return fail(D2FE_ERR_INVALID, "max_slots");
  const size_t ncell = (size_t)Hc * Wc;
  for (size_t i = 0; i < (size_t)n * ncell; ++i)
    if (slotmap[i] < -1 || slotmap[i] >= max_slots) return fail(D2FE_ERR_INVALID, "slot map entry outside [-1, max_slots)");
  for (int img = 0; img < n; ++img)
    for (int k = 0; k < n_kp[img] && k < kmax; ++k) {
      int cell[4];
      lookup_cells(kps_xy[2 * ((size_t)img * cap + k)], kps_xy[2 * ((size_t)img * cap + k) + 1], Hc, Wc, img_w, img_h, cell);
      for (int q = 0; q < 4; ++q)
        if (cell[q] >= 0 && slotmap[img * ncell + cell[q]] < 0) return fail(D2FE_ERR_INVALID, "a cell the sampler looks up has no slot");
    }
  return D2FE_OK;
}

// The sparse store [rows][256] of a sampler hook, uploaded behind one guard row of all-ones words (NaN): should the device look a cell up that check_slotmap did
// not foresee, its entry of -1 reads the guard row (image 0) or the previous image's last slot, not memory in front of the allocation.
static hipError_t sparse_store_upload(DevPool& b, float** out, const float* src, size_t rows) {
  float* base = nullptr;
  hipError_t e = b.alloc(&base, sizeof(float) * 256 * (rows + 1));
  if (e != hipSuccess) return e;
  e = hipMemset(base, 0xff, sizeof(float) * 256);
  if (e != hipSuccess) return e;
  *out = base + 256;
  return hipMemcpy(*out, src, sizeof(float) * 256 * rows, hipMemcpyHostToDevice);
}

// comp == nullptr: d2fe_debug_sample_b (rows of 256 floats); else d2fe_debug_sample_b_pca (rows of pca_dims floats)
static int debug_sample_b(d2fe_handle h, const float* desc_raw, int dstride, int dcoff, int n, int Hc, int Wc, const float* kps_xy, const int32_t* n_kp, int cap,
                          const int32_t* slotmap_or_null, int max_slots, const float* comp, const float* mean, int pca_dims, float* desc_out) {
  if (!h || !desc_raw || !kps_xy || !n_kp || !desc_out) return fail(D2FE_ERR_INVALID, "null argument");
  if (n < 1 || Hc < 2 || Wc < 2 || cap < 1 || (long)Hc * Wc * 64 > DEBUG_MAX_PIXELS || cap > DEBUG_MAX_PIXELS) return fail(D2FE_ERR_INVALID, "bad geometry");
  const size_t ncell = (size_t)Hc * Wc;
  if (slotmap_or_null) {      // sparse store [img][max_slots][256]
    const int rc = check_slotmap(slotmap_or_null, max_slots, n, Hc, Wc, 0, 0, kps_xy, n_kp, cap, cap);
    if (rc) return rc;
  } else if (dcoff < 0 || (dcoff & 3) || (dstride & 3) || dstride < dcoff + 256 || dstride > 4096) {
    return fail(D2FE_ERR_INVALID, "dense form: dcoff and dstride are multiples of 4 with dcoff + 256 <= dstride");
  }
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  DevPool b;
  float *d_raw = nullptr, *d_kps = nullptr, *d_desc = nullptr;
  int32_t *d_n = nullptr, *d_map = nullptr;
  if (slotmap_or_null) HIP_TRY(sparse_store_upload(b, &d_raw, desc_raw, (size_t)n * max_slots));
  else HIP_TRY(b.get(&d_raw, sizeof(float) * n * ncell * dstride, desc_raw));
  HIP_TRY(b.get(&d_kps, sizeof(float) * 2 * n * cap, kps_xy));
  HIP_TRY(b.get(&d_n, sizeof(int32_t) * n, n_kp));
  if (slotmap_or_null) HIP_TRY(b.get(&d_map, sizeof(int32_t) * n * ncell, slotmap_or_null));
  const size_t D = comp ? (size_t)pca_dims : 256;
  float *d_comp_t = nullptr, *d_mean = nullptr;
  if (comp) {      // the transposed layout d2fe_set_superpoint_pca uploads: comp_t [256][pca_dims]
    std::vector<float> t((size_t)256 * pca_dims);
    for (int j = 0; j < pca_dims; ++j)
      for (int c = 0; c < 256; ++c) t[(size_t)c * pca_dims + j] = comp[(size_t)j * 256 + c];
    HIP_TRY(b.get(&d_comp_t, sizeof(float) * t.size(), t.data()));
    HIP_TRY(b.get(&d_mean, sizeof(float) * 256, mean));
  }
  HIP_TRY(b.get(&d_desc, sizeof(float) * D * n * cap, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(launch_sample_b(d_raw, dstride, dcoff, Hc, Wc, n, d_kps, d_n, cap, d_map, max_slots, d_comp_t, d_mean, comp ? pca_dims : 0, d_desc, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(desc_out, d_desc, sizeof(float) * D * n * cap, hipMemcpyDeviceToHost));
  return D2FE_OK;
}

int d2fe_debug_sample_b(d2fe_handle h, const float* desc_raw, int dstride, int dcoff, int n, int Hc, int Wc, const float* kps_xy, const int32_t* n_kp, int cap,
                        const int32_t* slotmap_or_null, int max_slots, float* desc_out) {
  return debug_sample_b(h, desc_raw, dstride, dcoff, n, Hc, Wc, kps_xy, n_kp, cap, slotmap_or_null, max_slots, nullptr, nullptr, 0, desc_out);
}

int d2fe_debug_sample_b_pca(d2fe_handle h, const float* desc_raw, int dstride, int dcoff, int n, int Hc, int Wc, const float* kps_xy, const int32_t* n_kp, int cap,
                            const int32_t* slotmap_or_null, int max_slots, const float* comp, const float* mean, int pca_dims, float* desc_out) {
  if (!comp || !mean || pca_dims < 1 || pca_dims > 256) return fail(D2FE_ERR_INVALID, "comp, mean and pca_dims in 1..256 are required");
  return debug_sample_b(h, desc_raw, dstride, dcoff, n, Hc, Wc, kps_xy, n_kp, cap, slotmap_or_null, max_slots, comp, mean, pca_dims, desc_out);
}

int d2fe_debug_nms2_a(d2fe_handle h, const float* semi, int n, int H, int W, float thr, int dist, int max_kp, int cap, float* kps_xy, float* scores,
                      int32_t* kps_idx, int32_t* n_out) {
  if (!h || !semi || !kps_xy || !scores || !kps_idx || !n_out) return fail(D2FE_ERR_INVALID, "null argument");
  if (n < 1 || H < 1 || W < 1 || cap < 1 || dist < 0 || (long)H * W > DEBUG_MAX_PIXELS || cap > DEBUG_MAX_PIXELS) return fail(D2FE_ERR_INVALID, "bad geometry");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  const size_t hw = (size_t)H * W;
  const long cand_cap = (long)hw;
  DevPool b;
  float *d_semi = nullptr, *d_aconf = nullptr, *d_kps = nullptr, *d_sc = nullptr;
  int *d_clist = nullptr, *d_cnt = nullptr, *d_ncand = nullptr;
  unsigned long long* d_cand = nullptr;
  int32_t *d_idx = nullptr, *d_n = nullptr;
  HIP_TRY(b.get(&d_semi, sizeof(float) * n * hw, semi));
  HIP_TRY(b.get(&d_aconf, sizeof(float) * n * hw, nullptr));
  HIP_TRY(b.get(&d_clist, sizeof(int) * n * hw, nullptr, 0));
  HIP_TRY(b.get(&d_cand, sizeof(unsigned long long) * n * cand_cap, nullptr));
  HIP_TRY(b.get(&d_cnt, sizeof(int) * n, nullptr, 0));
  HIP_TRY(b.get(&d_ncand, sizeof(int) * n, nullptr, 0));
  HIP_TRY(b.get(&d_kps, sizeof(float) * 2 * n * cap, nullptr));
  HIP_TRY(b.get(&d_sc, sizeof(float) * n * cap, nullptr));
  HIP_TRY(b.get(&d_idx, sizeof(int32_t) * n * cap, nullptr));
  HIP_TRY(b.get(&d_n, sizeof(int32_t) * n, nullptr, 0));
  HIP_TRY(hipDeviceSynchronize());
  // the sequence run_superpoint issues for variant A
  HIP_TRY(launch_nms2_a(d_semi, H, W, n, thr, dist, d_aconf, d_clist, d_cand, d_cnt, cand_cap, d_ncand, h->stream));
  HIP_TRY(launch_select_b(d_cand, d_cnt, cand_cap, n, W, max_kp, cap, 1, nullptr, H, thr, 0, d_kps, d_sc, d_idx, d_n, h->stream));
  if ((long)H * W > 65536) HIP_TRY(launch_nms2_wrap_fix(d_clist, d_ncand, H, W, n, d_kps, d_idx, d_n, cap, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(kps_xy, d_kps, sizeof(float) * 2 * n * cap, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(scores, d_sc, sizeof(float) * n * cap, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(kps_idx, d_idx, sizeof(int32_t) * n * cap, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(n_out, d_n, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  return D2FE_OK;
}

// ---- the sparse descriptor head and variant A's descriptor tail on injected tensors (tests/test_desc_head_edges.py) ----
namespace {
constexpr long DEBUG_MAX_HEAD_CELLS = 1l << 17;      // cells per call: above launch_desc_head_sparse's 60 Ki threshold between its two mark / compact forms
}  // namespace

int d2fe_debug_desc_head_sparse(d2fe_handle h, const float* x, int x_cstride, int n, int Hc, int Wc, const float* kps_xy, const int32_t* n_kp, int cap,
                                int max_slots, int with_mid, int img_w, int img_h, const float* w_da, const float* b_da, const float* w_db, const float* b_db,
                                int32_t* slotmap_out, int32_t* cells_out, int32_t* count_out, float* store_out) {
  if (!h || !x || !kps_xy || !n_kp || !w_da || !b_da || !w_db || !b_db || !slotmap_out || !cells_out || !count_out || !store_out)
    return fail(D2FE_ERR_INVALID, "null argument");
  if (n < 1 || Hc < 2 || Wc < 2 || cap < 1 || cap > DEBUG_MAX_PIXELS || max_slots < 1 || max_slots > DEBUG_MAX_PIXELS || x_cstride < 128 || (x_cstride & 3) ||
      x_cstride > 4096 || (long)n * Hc * Wc > DEBUG_MAX_HEAD_CELLS || img_w < 0 || (img_w > 0 && img_h < 1))
    return fail(D2FE_ERR_INVALID, "bad geometry");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  const size_t ncell = (size_t)Hc * Wc;
  // the fragments of the L_DA32 / L_DB32 records (superpoint_host.hip)
  std::vector<float> pa(packed_weight_floats_f32(256, 128, 3)), pb(packed_weight_floats_f32(256, 256, 1));
  pack_weights_f32(w_da, 256, 128, 3, 256, pa.data());
  pack_weights_f32(w_db, 256, 256, 1, 256, pb.data());
  const int mid_imgs = with_mid ? (n < 4 ? n : 4) : 0;
  DevPool b;
  float *d_x = nullptr, *d_kps = nullptr, *d_wa = nullptr, *d_ba = nullptr, *d_wb = nullptr, *d_bb = nullptr, *d_store = nullptr, *d_mid = nullptr;
  int32_t *d_n = nullptr, *d_map = nullptr, *d_cells = nullptr, *d_cnt = nullptr;
  uint8_t* d_flags = nullptr;
  HIP_TRY(b.get(&d_x, sizeof(float) * n * ncell * x_cstride, x));
  HIP_TRY(b.get(&d_kps, sizeof(float) * 2 * n * cap, kps_xy));
  HIP_TRY(b.get(&d_n, sizeof(int32_t) * n, n_kp));
  HIP_TRY(b.get(&d_wa, sizeof(float) * pa.size(), pa.data()));
  HIP_TRY(b.get(&d_ba, sizeof(float) * 256, b_da));
  HIP_TRY(b.get(&d_wb, sizeof(float) * pb.size(), pb.data()));
  HIP_TRY(b.get(&d_bb, sizeof(float) * 256, b_db));
  HIP_TRY(b.get(&d_flags, n * ncell, nullptr));
  HIP_TRY(b.get(&d_map, sizeof(int32_t) * n * ncell, nullptr));
  HIP_TRY(b.get(&d_cells, sizeof(int32_t) * n * max_slots, nullptr));
  HIP_TRY(b.get(&d_cnt, sizeof(int32_t) * n, nullptr));
  HIP_TRY(b.get(&d_store, sizeof(float) * 256 * n * max_slots, nullptr));
  if (mid_imgs) HIP_TRY(b.get(&d_mid, sizeof(float) * 256 * mid_imgs * max_slots, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(launch_desc_head_sparse(d_kps, d_n, cap, Hc, Wc, n, d_x, x_cstride, (long)ncell * x_cstride, d_wa, d_ba, d_wb, d_bb, d_flags, d_map, d_cells, d_cnt,
                                  max_slots, d_store, d_mid, mid_imgs, img_w, img_h, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(slotmap_out, d_map, sizeof(int32_t) * n * ncell, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(cells_out, d_cells, sizeof(int32_t) * n * max_slots, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(count_out, d_cnt, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(store_out, d_store, sizeof(float) * 256 * n * max_slots, hipMemcpyDeviceToHost));
  return D2FE_OK;
}

int d2fe_debug_sample_a(d2fe_handle h, const float* desc_raw, int dstride, int dcoff, int n, int Hc, int Wc, int img_w, int img_h, const float* kps_xy,
                        const int32_t* n_kp, int cap, int scap, const int32_t* slotmap_or_null, int max_slots, const float* comp_or_null, const float* mean,
                        int pca_dims, float* desc_out) {
  if (!h || !desc_raw || !kps_xy || !n_kp || !desc_out) return fail(D2FE_ERR_INVALID, "null argument");
  if (n < 1 || Hc < 2 || Wc < 2 || cap < 1 || scap < 1 || img_w < 1 || img_h < 1 || (long)Hc * Wc * 64 > DEBUG_MAX_PIXELS || cap > DEBUG_MAX_PIXELS ||
      scap > DEBUG_MAX_PIXELS)
    return fail(D2FE_ERR_INVALID, "bad geometry");
  if (comp_or_null && (!mean || pca_dims < 1 || pca_dims > 256)) return fail(D2FE_ERR_INVALID, "comp needs mean and pca_dims in 1..256");
  const size_t ncell = (size_t)Hc * Wc;
  if (slotmap_or_null) {
    const int rc = check_slotmap(slotmap_or_null, max_slots, n, Hc, Wc, img_w, img_h, kps_xy, n_kp, cap, cap < scap ? cap : scap);
    if (rc) return rc;
  } else if (dcoff < 0 || (dcoff & 3) || (dstride & 3) || dstride < dcoff + 256 || dstride > 4096) {
    return fail(D2FE_ERR_INVALID, "dense form: dcoff and dstride are multiples of 4 with dcoff + 256 <= dstride");
  }
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  DevPool b;
  float *d_raw = nullptr, *d_kps = nullptr, *d_desc = nullptr, *d_samp = nullptr, *d_cn = nullptr, *d_comp_t = nullptr, *d_mean = nullptr;
  int32_t *d_n = nullptr, *d_map = nullptr;
  if (slotmap_or_null) HIP_TRY(sparse_store_upload(b, &d_raw, desc_raw, (size_t)n * max_slots));
  else HIP_TRY(b.get(&d_raw, sizeof(float) * n * ncell * dstride, desc_raw));
  HIP_TRY(b.get(&d_kps, sizeof(float) * 2 * n * cap, kps_xy));
  HIP_TRY(b.get(&d_n, sizeof(int32_t) * n, n_kp));
  if (slotmap_or_null) HIP_TRY(b.get(&d_map, sizeof(int32_t) * n * ncell, slotmap_or_null));
  const size_t D = comp_or_null ? (size_t)pca_dims : 256;
  if (comp_or_null) {      // the transposed layout d2fe_set_superpoint_pca uploads: comp_t [256][pca_dims]
    std::vector<float> t((size_t)256 * pca_dims);
    for (int j = 0; j < pca_dims; ++j)
      for (int c = 0; c < 256; ++c) t[(size_t)c * pca_dims + j] = comp_or_null[(size_t)j * 256 + c];
    HIP_TRY(b.get(&d_comp_t, sizeof(float) * t.size(), t.data()));
    HIP_TRY(b.get(&d_mean, sizeof(float) * 256, mean));
  }
  HIP_TRY(b.get(&d_samp, sizeof(float) * 256 * n * scap, nullptr));
  HIP_TRY(b.get(&d_cn, sizeof(float) * 256 * n, nullptr));
  HIP_TRY(b.get(&d_desc, sizeof(float) * D * n * cap, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(launch_sample_a(d_raw, dstride, dcoff, Hc, Wc, img_w, img_h, n, d_kps, d_n, cap, d_comp_t, d_mean, comp_or_null ? pca_dims : 0, d_samp, scap, d_cn,
                          d_map, max_slots, d_desc, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(desc_out, d_desc, sizeof(float) * D * n * cap, hipMemcpyDeviceToHost));
  return D2FE_OK;
}

// ---- one layer of the direct SuperPoint conv kernels on injected tensors (tests/test_conv_layer_edges.py) ----
namespace {
constexpr long DEBUG_MAX_CONV_FLOATS = 1l << 26;      // floats per caller buffer: far below the 2^31 bytes the epilogues' 32-bit offsets cover

struct ConvGeom { int cin, ks, bn; };
// Cin, kernel size and the channels per workgroup (BN: cout_pad is a multiple of it) of a shape; the same in the one-tile and the persistent kernels
ConvGeom conv_geom(int shape) {
  switch (shape) {
    case CONV_64_T8x32:      return {64, 3, 64};
    case CONV_128_T4x32:     return {128, 3, 128};
    case CONV_128_T4x16:     return {128, 3, 128};
    case CONV_256_1x1_T4x16: return {256, 1, 128};
    case CONV1B_FUSED:       return {64, 3, 64};
  }
  return {0, 0, 0};
}
// the (shape, pool, relu) combinations the launchers compile: launch_conv_tile (launch_f32 / launch_f16: pool only on the 32-wide two-m-tile shapes; the
// fused shape is pool + ReLU) and launch_pc_mode's table
bool conv_compiled(int family, int shape, bool pool, bool relu) {
  if (shape == CONV1B_FUSED) return pool && relu;
  if (family == 1) return !pool || shape == CONV_64_T8x32 || shape == CONV_128_T4x32;
  switch (shape) {
    case CONV_64_T8x32:      return relu;
    case CONV_128_T4x32:     return pool && relu;
    case CONV_128_T4x16:     return !pool && relu;
    case CONV_256_1x1_T4x16: return !pool && !relu;
  }
  return false;
}
// D2FE_PREC_I8 has the one-tile kernels alone (conv_i8.hip: launch_i8 compiles the pool only with ReLU)
bool conv_compiled_i8(int family, int shape, bool pool, bool relu) {
  if (family != 1) return false;
  if (shape == CONV1B_FUSED) return pool && relu;
  return !pool || (relu && (shape == CONV_64_T8x32 || shape == CONV_128_T4x32));
}

// quantised: d2fe_debug_conv_layer_q (precision 5 is accepted only there, with the input tensor's range)
int conv_layer_hook(d2fe_handle h, const d2fe_debug_conv* p, const float* weight, const float* bias, const float* in, float* out, const uint8_t* frames,
                    const float* w1a, const float* b1a, bool quantised, float in_range) {
  if (!h || !p || !weight || !bias || !out) return fail(D2FE_ERR_INVALID, "null argument");
  const bool i8 = quantised && p->precision == 5;
  if (p->family < 0 || p->family > 3 || (p->precision != 0 && p->precision != 1 && p->precision != 3 && !i8) || p->shape < 0 || p->shape > CONV1B_FUSED)
    return fail(D2FE_ERR_INVALID, "family, precision or shape");
  if (i8 && !(in_range >= 1e-30f && in_range <= 1e30f)) return fail(D2FE_ERR_INVALID, "in_range must be finite and in [1e-30, 1e30]");
  const bool pool = p->pool != 0, relu = p->relu != 0, fused = p->shape == CONV1B_FUSED;
  // family 0 = what conv() of superpoint_host.hip does in this process: convPb's own kernel first (fp32 modes, D2FE_CONV1X1), then launch_conv, which
  // takes the persistent or the one-tile kernels by D2FE_CONV_PC and the Cin-64 tile by D2FE_CONV64_TILE
  int family = p->family, conv64_tile = p->conv64_tile;
  if (family == 0) {
    family = (!i8 && (tune_conv_pc() == 1 || (tune_conv_pc() == 2 && !fused))) ? 2 : 1;
    conv64_tile = tune_conv64();
  }
  const bool try_1x1 = p->family == 0 && p->precision == 0 && p->shape == CONV_256_1x1_T4x16 && p->cout == 65 && !pool && !relu && d2fe_dev_env("D2FE_CONV1X1", 1);
  if (p->family == 3) {
    if (p->precision != 0 || p->shape != CONV_256_1x1_T4x16 || pool || relu) return fail(D2FE_ERR_INVALID, "family 3 is the fp32 1x1 layer without pool and ReLU");
  } else if (i8 ? !conv_compiled_i8(family, p->shape, pool, relu) : !conv_compiled(family, p->shape, pool, relu)) {
    return fail(D2FE_ERR_INVALID, "no kernel of this family is compiled for the shape with this pool / relu");
  }
  if (family == 1 && conv64_tile != 0 && conv64_tile != 1) return fail(D2FE_ERR_INVALID, "conv64_tile is 0 or 1");
  const ConvGeom g = conv_geom(p->shape);
  const int n = p->n, H = p->H, W = p->W, cout = p->cout;
  if (n < 1 || n > 64 || H < 1 || W < 1 || H > 4096 || W > 4096 || (pool && (H < 2 || W < 2)) || cout < 1 || cout > 1024 || (fused && cout > 64))
    return fail(D2FE_ERR_INVALID, "bad geometry");
  const int cout_pad = (cout + g.bn - 1) / g.bn * g.bn;      // the rule of sp_plan.h: whole workgroups of channels
  const int ncu = p->ncu > 0 ? p->ncu : h->ncu;
  if (p->ncu < 0 || ncu < 1 || ncu > 4096) return fail(D2FE_ERR_INVALID, "ncu");
  const long hw = (long)H * W, ohw = pool ? (long)(H / 2) * (W / 2) : hw;
  // every address the kernels can form lies inside the caller's buffers: pixel (img, y, x) channel c of the input is in[img * in_img_stride + (y * W + x) *
  // in_cstride + in_coff + c] for c < Cin (float4 loads of whole aligned groups of four of these), of the output out[img * out_img_stride + (y * Wo + x) *
  // out_cstride + out_coff + c] for c < cout; the frame byte (img, y, x) is frames[img * img_istride + y * img_stride + x]
  if (p->out_floats < 1 || p->out_floats > DEBUG_MAX_CONV_FLOATS || p->out_cstride < 1 || p->out_coff < 0 || p->out_img_stride < 0 ||
      p->out_img_stride > DEBUG_MAX_CONV_FLOATS || p->out_cstride > 65536 || p->out_coff > 65536 || (n > 1 && p->out_img_stride < ohw * p->out_cstride) ||
      (n - 1) * p->out_img_stride + (ohw - 1) * p->out_cstride + p->out_coff + cout > p->out_floats || ohw * p->out_cstride >= (1l << 29))
    return fail(D2FE_ERR_INVALID, "the output tensor does not fit the output buffer");
  if (fused) {
    if (!frames || !w1a || !b1a) return fail(D2FE_ERR_INVALID, "CONV1B_FUSED needs frames and the conv1a weights");
    if (p->img_bytes < 1 || p->img_bytes > 4 * DEBUG_MAX_CONV_FLOATS || p->img_stride < 1 || p->img_stride > 65536 || p->img_istride < 0 ||
        p->img_istride > 4 * DEBUG_MAX_CONV_FLOATS || (n - 1) * p->img_istride + (long)(H - 1) * p->img_stride + W > p->img_bytes)
      return fail(D2FE_ERR_INVALID, "the frames do not fit the frame buffer");
  } else {
    if (!in) return fail(D2FE_ERR_INVALID, "null input");
    if (p->in_floats < 1 || p->in_floats > DEBUG_MAX_CONV_FLOATS || p->in_cstride < 1 || p->in_coff < 0 || p->in_img_stride < 0 ||
        p->in_img_stride > DEBUG_MAX_CONV_FLOATS || p->in_cstride > 65536 || p->in_coff > 65536 ||
        (n - 1) * p->in_img_stride + (hw - 1) * p->in_cstride + p->in_coff + g.cin > p->in_floats)
      return fail(D2FE_ERR_INVALID, "the input tensor does not fit the input buffer");
    // float4 loads (launch_conv1x1_256_65 refuses a misaligned tensor itself: family 3 leaves that answer to it)
    if (p->family != 3 && ((p->in_cstride & 3) || (p->in_coff & 3) || (p->in_img_stride & 3)))
      return fail(D2FE_ERR_INVALID, "in_cstride, in_coff and in_img_stride are multiples of 4 floats");
  }
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  // weights and bias as pack_layer of superpoint_host.hip prepares them
  std::vector<float> pf, bp(cout_pad, 0.f), t1a;
  std::vector<uint16_t> ph;
  std::vector<int8_t> pq;
  std::vector<float> dsc;      // D2FE_PREC_I8: d_c = s_x * s_w[c], as d2fe_set_superpoint_int8_ranges computes it
  memcpy(bp.data(), bias, sizeof(float) * cout);
  if (i8) {
    pq.resize(packed_weight_bytes_i8(cout_pad, g.cin, g.ks)); dsc.resize(cout_pad);
    pack_weights_i8(weight, cout, g.cin, g.ks, cout_pad, pq.data(), dsc.data());
    const float s_x = in_range / 127.0f;
    for (float& d : dsc) d = s_x * d;
  }
  else if (p->precision == 0) { pf.resize(packed_weight_floats_f32(cout_pad, g.cin, g.ks)); pack_weights_f32(weight, cout, g.cin, g.ks, cout_pad, pf.data()); }
  else if (p->precision == 1) { ph.resize(packed_weight_halfs_f16x2(cout_pad, g.cin, g.ks)); pack_weights_f16x2(weight, cout, g.cin, g.ks, cout_pad, ph.data()); }
  else { ph.resize(packed_weight_halfs_f16(cout_pad, g.cin, g.ks)); pack_weights_f16(weight, cout, g.cin, g.ks, cout_pad, ph.data()); }
  DevPool b;
  float *d_in = nullptr, *d_out = nullptr, *d_b = nullptr, *d_w1a = nullptr, *d_b1a = nullptr, *d_zero = nullptr, *d_dsc = nullptr;
  void* d_w = nullptr;
  uint8_t* d_img = nullptr;
  if (fused) {
    t1a.resize(9 * 64);      // [64][1][3][3] -> [9][64], as d2fe_load_superpoint
    for (int co = 0; co < 64; ++co)
      for (int k = 0; k < 9; ++k) t1a[k * 64 + co] = w1a[co * 9 + k];
    HIP_TRY(b.get(&d_img, (size_t)p->img_bytes, frames));
    HIP_TRY(b.get(&d_w1a, sizeof(float) * t1a.size(), t1a.data()));
    HIP_TRY(b.get(&d_b1a, sizeof(float) * 64, b1a));
  } else {
    HIP_TRY(b.get(&d_in, sizeof(float) * p->in_floats, in));
  }
  HIP_TRY(b.get(&d_out, sizeof(float) * p->out_floats, out));      // the caller's pre-filled buffer: what no kernel writes comes back as it went in
  if (i8) { HIP_TRY(b.get(&d_w, pq.size(), pq.data())); HIP_TRY(b.get(&d_dsc, sizeof(float) * dsc.size(), dsc.data())); }
  else if (p->precision == 0) HIP_TRY(b.get(&d_w, sizeof(float) * pf.size(), pf.data()));
  else HIP_TRY(b.get(&d_w, sizeof(uint16_t) * ph.size(), ph.data()));
  HIP_TRY(b.get(&d_b, sizeof(float) * bp.size(), bp.data()));
  HIP_TRY(b.get(&d_zero, sizeof(float) * 256, nullptr, 0));
  HIP_TRY(hipDeviceSynchronize());      // the null-stream copies and memsets are not ordered with the handle's non-blocking stream
  ConvArgs a{};
  a.in = d_in; a.in_cstride = p->in_cstride; a.in_coff = p->in_coff; a.out = d_out; a.out_cstride = p->out_cstride; a.out_coff = p->out_coff;
  a.cout_real = cout; a.wpack = d_w; a.bias = d_b; a.H = H; a.W = W; a.n_img = n;
  a.in_img_stride = (long)p->in_img_stride; a.out_img_stride = (long)p->out_img_stride;
  a.img = d_img; a.img_stride = p->img_stride; a.img_istride = (long)p->img_istride; a.w1a = d_w1a; a.b1a = d_b1a;
  a.zeros = d_zero; a.ncu = ncu; a.tag = 0; a.ablate = 0;
  if (i8) { a.qr = 127.0f / in_range; a.dscale = d_dsc; }
  const ConvShape shape = (ConvShape)p->shape;
  hipError_t e = hipErrorNotSupported;
  if (p->family == 3 || try_1x1) e = launch_conv1x1_256_65(a, h->stream);
  if (p->family == 3 && e == hipErrorNotSupported) {      // nothing was launched: the caller gets the device copy of its buffer back all the same
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(out, d_out, sizeof(float) * p->out_floats, hipMemcpyDeviceToHost));
    return fail(D2FE_ERR_UNSUPPORTED, "launch_conv1x1_256_65 does not take these tensors");
  }
  if (p->family == 0 && e == hipErrorNotSupported) e = launch_conv(shape, p->precision, pool, relu, cout_pad, a, h->stream);
  else if (p->family == 1) e = launch_conv_tile(shape, p->precision, conv64_tile, pool, relu, cout_pad, a, h->stream);
  else if (p->family == 2) e = launch_conv_pc(shape, p->precision, pool, relu, cout_pad, a, h->stream);
  HIP_TRY(e);
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(out, d_out, sizeof(float) * p->out_floats, hipMemcpyDeviceToHost));
  return D2FE_OK;
}
}  // namespace

int d2fe_debug_conv_layer(d2fe_handle h, const d2fe_debug_conv* p, const float* weight, const float* bias, const float* in, float* out, const uint8_t* frames,
                          const float* w1a, const float* b1a) {
  return conv_layer_hook(h, p, weight, bias, in, out, frames, w1a, b1a, false, 0.f);
}

int d2fe_debug_conv_layer_q(d2fe_handle h, const d2fe_debug_conv* p, const float* weight, const float* bias, const float* in, float* out, const uint8_t* frames,
                            const float* w1a, const float* b1a, float in_range) {
  return conv_layer_hook(h, p, weight, bias, in, out, frames, w1a, b1a, true, in_range);
}

int d2fe_debug_conv1a(d2fe_handle h, int kernel, const uint8_t* frames, int img_stride, long long img_istride, long long img_bytes, int n, int H, int W,
                      const float* w1a, const float* b1a, float* out, long long out_floats) {
  if (!h || !frames || !w1a || !b1a || !out) return fail(D2FE_ERR_INVALID, "null argument");
  if (kernel < -1 || kernel > 1 || n < 1 || n > 64 || H < 1 || W < 1 || H > 4096 || W > 4096 || img_stride < 1 || img_stride > 65536 || img_istride < 0 ||
      img_bytes < 1 || img_bytes > 4 * DEBUG_MAX_CONV_FLOATS || img_istride > 4 * DEBUG_MAX_CONV_FLOATS ||
      (n - 1) * img_istride + (long long)(H - 1) * img_stride + W > img_bytes)
    return fail(D2FE_ERR_INVALID, "bad geometry, or the frames do not fit the frame buffer");
  const long long need = (long long)n * H * W * 64;      // both kernels write [n][H][W][64], dense
  if (out_floats < need || out_floats > DEBUG_MAX_CONV_FLOATS) return fail(D2FE_ERR_INVALID, "the output does not fit the output buffer");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  std::vector<float> t(9 * 64);
  for (int co = 0; co < 64; ++co)
    for (int k = 0; k < 9; ++k) t[k * 64 + co] = w1a[co * 9 + k];
  DevPool b;
  uint8_t* d_img = nullptr;
  float *d_w = nullptr, *d_b = nullptr, *d_out = nullptr;
  HIP_TRY(b.get(&d_img, (size_t)img_bytes, frames));
  HIP_TRY(b.get(&d_w, sizeof(float) * t.size(), t.data()));
  HIP_TRY(b.get(&d_b, sizeof(float) * 64, b1a));
  HIP_TRY(b.get(&d_out, sizeof(float) * out_floats, out));
  HIP_TRY(hipDeviceSynchronize());
  if (kernel < 0) HIP_TRY(launch_conv1a(d_img, img_stride, (long)img_istride, H, W, n, d_w, d_b, d_out, h->stream));
  else HIP_TRY(launch_conv1a_kernel(kernel, d_img, img_stride, (long)img_istride, H, W, n, d_w, d_b, d_out, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(out, d_out, sizeof(float) * out_floats, hipMemcpyDeviceToHost));
  return D2FE_OK;
}

// ---- the calibration session's parts (calib.hip) on injected data ----
int d2fe_debug_calib_ranges_from_hist(const uint64_t* hist, int n_bins, float t, int method, double param, float* range, int* index) {
  return calib_range_from_hist(reinterpret_cast<const unsigned long long*>(hist), n_bins, t, method, param, range, index);
}

namespace {
// the in-out counters of a calibration hook on the device: uploaded from the caller's, downloaded behind the launch
struct CalibHookOut {
  DevPool pool;
  CalibOut d{};
  int n_bins = 0;
  int up(int nb, const uint32_t* t_max_bits, const uint64_t* hist, const uint64_t* n_zero, const uint64_t* n_over) {
    n_bins = nb;
    HIP_TRY(pool.get(&d.t_max_bits, sizeof(uint32_t), t_max_bits));
    HIP_TRY(pool.get(&d.hist, sizeof(uint64_t) * nb, hist));
    HIP_TRY(pool.get(&d.n_zero, sizeof(uint64_t), n_zero));
    HIP_TRY(pool.get(&d.n_over, sizeof(uint64_t), n_over));
    return D2FE_OK;
  }
  int down(uint32_t* t_max_bits, uint64_t* hist, uint64_t* n_zero, uint64_t* n_over) {
    HIP_TRY(hipMemcpy(t_max_bits, d.t_max_bits, sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(hist, d.hist, sizeof(uint64_t) * n_bins, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(n_zero, d.n_zero, sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(n_over, d.n_over, sizeof(uint64_t), hipMemcpyDeviceToHost));
    return D2FE_OK;
  }
};
bool calib_hook_args_ok(float t, int n_bins, int phase) { return calib_bins_ok(n_bins) && (phase == 0 || phase == 1) && t >= 1e-30f && t <= 3e38f; }
}  // namespace

int d2fe_debug_calib_stats(d2fe_handle h, const float* tensor, long long pixels, int ch_off, int channels, int ch_stride, float t, int n_bins, int phase, int wgs,
                           uint32_t* t_max_bits, uint64_t* hist, uint64_t* n_zero, uint64_t* n_over) {
  if (!h || !tensor || !t_max_bits || !hist || !n_zero || !n_over) return fail(D2FE_ERR_INVALID, "null argument");
  if (!calib_hook_args_ok(t, n_bins, phase) || pixels < 1 || channels < 1 || ch_off < 0 || ch_stride < 1 || ch_off + (long long)channels > ch_stride ||
      pixels > (1ll << 28) / ch_stride || wgs < 0 || wgs > 4096)
    return fail(D2FE_ERR_INVALID, "bad calibration hook arguments");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  CalibHookOut o;
  float* d_x = nullptr;
  HIP_TRY(o.pool.get(&d_x, sizeof(float) * (size_t)pixels * ch_stride, tensor));
  { const int rc = o.up(n_bins, t_max_bits, hist, n_zero, n_over); if (rc) return rc; }
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(launch_calib_stats(d_x, pixels, ch_off, channels, ch_stride, phase == 1, t, (float)n_bins / t, n_bins, o.d, h->ncu, wgs, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return o.down(t_max_bits, hist, n_zero, n_over);
}

int d2fe_debug_calib_conv1a(d2fe_handle h, const uint8_t* frames, int img_stride, long long img_istride, long long img_bytes, int n, int H, int W, const float* w1a,
                            const float* b1a, float t, int n_bins, int phase, uint32_t* t_max_bits, uint64_t* hist, uint64_t* n_zero, uint64_t* n_over) {
  if (!h || !frames || !w1a || !b1a || !t_max_bits || !hist || !n_zero || !n_over) return fail(D2FE_ERR_INVALID, "null argument");
  if (!calib_hook_args_ok(t, n_bins, phase) || n < 1 || n > 64 || H < 1 || W < 1 || H > 4096 || W > 4096 || img_stride < W || img_stride > 65536 || img_istride < 0 ||
      img_bytes < 1 || img_bytes > 4 * DEBUG_MAX_CONV_FLOATS || img_istride > 4 * DEBUG_MAX_CONV_FLOATS ||
      (n - 1) * img_istride + (long long)(H - 1) * img_stride + W > img_bytes)
    return fail(D2FE_ERR_INVALID, "bad calibration hook arguments, or the frames do not fit the frame buffer");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  std::vector<float> w9(9 * 64);
  for (int co = 0; co < 64; ++co)
    for (int k = 0; k < 9; ++k) w9[k * 64 + co] = w1a[co * 9 + k];
  CalibHookOut o;
  uint8_t* d_img = nullptr;
  float *d_w = nullptr, *d_b = nullptr;
  HIP_TRY(o.pool.get(&d_img, (size_t)img_bytes, frames));
  HIP_TRY(o.pool.get(&d_w, sizeof(float) * w9.size(), w9.data()));
  HIP_TRY(o.pool.get(&d_b, sizeof(float) * 64, b1a));
  { const int rc = o.up(n_bins, t_max_bits, hist, n_zero, n_over); if (rc) return rc; }
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(launch_calib_conv1a_stats(d_img, img_stride, (long)img_istride, H, W, n, d_w, d_b, phase == 1, t, (float)n_bins / t, n_bins, o.d, h->ncu, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return o.down(t_max_bits, hist, n_zero, n_over);
}

int d2fe_debug_graph_count(d2fe_handle h, int* rejected) {
  if (!h) return fail(D2FE_ERR_INVALID, "null handle");
  int n = 0, bad = 0;
  for (auto& kv : h->graphs) { n += kv.second.exec != nullptr; bad += kv.second.bad; }
  if (rejected) *rejected = bad;
  return n;
}

}  // extern "C"
#endif  // D2FE_DEVTOOLS
