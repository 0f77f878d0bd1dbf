// api.hip -- C ABI (include/d2fe.h) of libd2fe_hip.so: handle lifecycle, the host and device extract entry
// points, the matcher, the "next rows", the debug hooks and profiling.  Host code only: SuperPoint's host side
// is superpoint_host.hip, NetVLAD's netvlad_host.hip, the kernels live in the other translation units
// (kernels.h lists their launchers).  There is deliberately NO CPU fallback in this library.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <array>
#include <atomic>
#include <deque>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "context.h"
#ifdef D2FE_DEVTOOLS
#include "../../include/d2fe_debug.h"
#endif

using namespace d2fe;

namespace {
thread_local std::string g_err;
}  // namespace

// accessors for the translation units that keep their own extern "C" entry points (lk.hip, netvlad_host.hip)
namespace d2fe {
int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
int ctx_fail(int code, const std::string& msg) { return fail(code, msg); }
int ctx_device(d2fe_handle h) { return h->cfg.device_id; }
hipStream_t ctx_stream(d2fe_handle h) { return h->stream; }
// grow-only device scratch owned by the handle: no hipMalloc/hipFree (a device-wide sync) per tracker call.  Not re-entrant,
// like the extract calls: one tracker thread per handle (the reference's D2FeatureTracker is single-threaded, d2frontend.cpp:155-169)
int ctx_scratch(d2fe_handle h, size_t bytes, void** out) {
  if (bytes > h->lk_scratch_bytes) {
    if (h->lk_scratch) { hipStreamSynchronize(h->stream); hipFree(h->lk_scratch); h->lk_scratch = nullptr; h->lk_scratch_bytes = 0; }
    const size_t want = bytes + bytes / 2 + 4096;
    if (hipMalloc(&h->lk_scratch, want) != hipSuccess) return fail(D2FE_ERR_HIP, "hipMalloc scratch");
    h->lk_scratch_bytes = want;
  }
  *out = h->lk_scratch;
  return D2FE_OK;
}
int upload(const void* src, size_t bytes, void** dst) {
  HIP_TRY(hipMalloc(dst, bytes));
  HIP_TRY(hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
  return D2FE_OK;
}
}  // namespace d2fe

#ifdef D2FE_DEVTOOLS
// launch-regime record (kernels.h: D2FE_REGIME): process-wide, written by the launchers from any thread (pipe lanes)
namespace {
std::atomic<long long> g_regime[D2FE_REGIME_COUNT];
}  // namespace
namespace d2fe {
void regime_note(int regime) { if (regime >= 0 && regime < D2FE_REGIME_COUNT) g_regime[regime].fetch_add(1, std::memory_order_relaxed); }
void regime_set(int regime, long long value) { if (regime >= 0 && regime < D2FE_REGIME_COUNT) g_regime[regime].store(value, std::memory_order_relaxed); }
}  // namespace d2fe
#endif

namespace d2fe {
void graphs_clear(d2fe_context* h) {
  if (h->graphs.empty()) return;
  (void)hipStreamSynchronize(h->stream);
  for (auto& kv : h->graphs) if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
  h->graphs.clear();
}

void host_state_save(const d2fe_context* h, d2fe_context::HostState& st) {
  st.last_w = h->last_w; st.last_h = h->last_h; st.last_n = h->last_n; st.last_set = h->last_set;
  st.last_gray = h->last_gray; st.last_stride = h->last_stride; st.last_istride = h->last_istride;
  st.nv = h->nv_run.last;
}
void host_state_restore(d2fe_context* h, const d2fe_context::HostState& st, bool netvlad) {
  if (netvlad) {
    h->nv_run.last = st.nv;
  } else {
    h->last_w = st.last_w; h->last_h = st.last_h; h->last_n = st.last_n; h->last_set = st.last_set;
    h->last_gray = st.last_gray; h->last_stride = st.last_stride; h->last_istride = st.last_istride;
  }
}

}  // namespace d2fe

extern "C" {

const char* d2fe_last_error(void) { return g_err.c_str(); }
const char* d2fe_version(void) { return "d2fe-hip 0.1 (gfx950)"; }

void d2fe_default_config(d2fe_config* c) {
  memset(c, 0, sizeof(*c));
  c->struct_size = (int32_t)sizeof(d2fe_config);
  c->device_id = 0;
  c->max_width = 640;
  c->max_height = 480;
  c->max_batch = 2;
  c->max_keypoints = 100;       // SuperPointConfig default, superpoint_tensorrt.h:18
  c->remove_borders = 1;        // :19
  c->keypoint_threshold = 0.015f;  // :24
  c->postproc = D2FE_POSTPROC_B;
  c->nms_dist = 10;
  c->precision = D2FE_PREC_F32;
  c->dense_descriptors = 0;
  c->async_tail = 0;
}

}  // extern "C"
namespace d2fe {
// lane = a context cloned for a pipe (clone_lane): no host-pointer staging (frame upload buffer, output block, pinned mirrors) -- a lane is only ever
// driven through run_superpoint / run_netvlad on device buffers of the pipe
static int create_context(const d2fe_config* cfg_in, d2fe_handle* out, bool lane, hipStream_t adopt = nullptr) {
  if (!cfg_in || !out) return fail(D2FE_ERR_INVALID, "null argument");
  *out = nullptr;
  // two struct versions: the one that ends behind `reserved` (the exact_order fields are then zero: off) and the current one
  if (cfg_in->struct_size != (int32_t)sizeof(d2fe_config) && cfg_in->struct_size != (int32_t)offsetof(d2fe_config, exact_order))
    return fail(D2FE_ERR_INVALID, "d2fe_config size mismatch");
  d2fe_config cfg_full;
  memset(&cfg_full, 0, sizeof(cfg_full));
  memcpy(&cfg_full, cfg_in, (size_t)cfg_in->struct_size);
  cfg_full.struct_size = (int32_t)sizeof(d2fe_config);
  const d2fe_config* cfg = &cfg_full;
  if (!(cfg->keypoint_threshold >= 0.f)) return fail(D2FE_ERR_INVALID, "keypoint_threshold must be >= 0 (scores are probabilities)");
  if (cfg->max_width < 16 || cfg->max_height < 16) return fail(D2FE_ERR_INVALID, "max_width/max_height must be at least 16");
  if (cfg->max_batch < 1) return fail(D2FE_ERR_INVALID, "max_batch < 1");
  // -1 = keep every keypoint above the threshold (SuperPoint::topKeypoints only truncates when k != -1, superpoint_tensorrt.cpp:241-253;
  // NMS2's `i < max_num` is an unsigned compare, superpoint_common.cpp:173): variant B then returns EVERY keypoint above the threshold, in
  // raster order, up to the call's capacity (any capacity up to H*W; D2FE_ERR_TRUNCATED with the first of them in raster order kept if an image had more);
  // variant A up to 1024.  A sorted top-K selection takes K <= 16384 (one workgroup's in-LDS bitonic sort); the reference's TensorRT
  // profile (1500 x 1500, superpoint_tensorrt.cpp:50-55) with max_keypoints in the thousands is inside that.
  if ((cfg->max_keypoints < 1 && cfg->max_keypoints != -1) || cfg->max_keypoints > 16384) return fail(D2FE_ERR_INVALID, "max_keypoints must be -1 (keep all) or in 1..16384");
  if (cfg->precision != D2FE_PREC_F32 && cfg->precision != D2FE_PREC_F16X2 && cfg->precision != D2FE_PREC_F32_WINO && cfg->precision != D2FE_PREC_F16) return fail(D2FE_ERR_INVALID, "bad precision");
  if (cfg->postproc != D2FE_POSTPROC_B && cfg->postproc != D2FE_POSTPROC_A) return fail(D2FE_ERR_INVALID, "bad postproc");
  if (cfg->variant_b_pca != 0 && cfg->variant_b_pca != 1) return fail(D2FE_ERR_INVALID, "variant_b_pca must be 0 or 1");
  if (cfg->variant_b_pca && cfg->postproc != D2FE_POSTPROC_B) return fail(D2FE_ERR_INVALID, "variant_b_pca is an option of post-processing variant B (variant A applies the PCA without it)");
  if (cfg->exact_order) {
    if (cfg->precision != D2FE_PREC_F32_WINO) return fail(D2FE_ERR_INVALID, "exact_order is an option of D2FE_PREC_F32_WINO (D2FE_PREC_F32 is exact already; D2FE_PREC_F16X2 and D2FE_PREC_F16 are not supported)");
    if (cfg->postproc != D2FE_POSTPROC_B) return fail(D2FE_ERR_INVALID, "exact_order needs post-processing variant B (NMS2 of variant A depends on the order in another way)");
    if (cfg->max_keypoints < 1) return fail(D2FE_ERR_INVALID, "exact_order needs max_keypoints >= 1 (keep-all handles are not supported)");
    if (!(cfg->exact_order_eps >= 0.f) || std::isinf(cfg->exact_order_eps)) return fail(D2FE_ERR_INVALID, "exact_order_eps must be finite and >= 0 (0 = the default)");
    if (cfg->exact_order_crops < 0 || cfg->exact_order_crops > 65535) return fail(D2FE_ERR_INVALID, "exact_order_crops must be in 0..65535 (0 = the default)");
    if (cfg->max_width < 88 || cfg->max_height < 88) return fail(D2FE_ERR_INVALID, "exact_order needs max_width and max_height of at least 88");
  }
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (ndev < 1) return fail(D2FE_ERR_HIP, "no HIP device visible (this library has no CPU fallback)");
  if (cfg->device_id < 0 || cfg->device_id >= ndev) return fail(D2FE_ERR_INVALID, "device_id out of range");
  HIP_TRY(hipSetDevice(cfg->device_id));
  d2fe_context* h = new d2fe_context();
  h->cfg = *cfg;
  const int rc_alloc = [&]() -> int {
    // (a lane that is handed its stream does not create one first: no stream is created that is not needed, see place_streams in pipe.hip)
    if (adopt) h->stream = adopt; else HIP_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    const size_t H = cfg->max_height, W = cfg->max_width;
    const int B = cfg->max_batch;
    { const int rc = h->sp_run.alloc(*cfg); if (rc) return rc; }
    if (!lane) {      // a lane shares its parent's network (clone_lane)
      h->sp_net = std::make_shared<SpNet>();
      if (cfg->exact_order) HIP_TRY(h->sp_net->pool.get(&h->sp_net->eo_stats, 4 * sizeof(unsigned long long), nullptr, 0));
    }
    if (cfg->async_tail) {
      HIP_TRY(hipStreamCreateWithFlags(&h->tail_stream, hipStreamNonBlocking));
      for (int i = 0; i < 2; ++i) {
        HIP_TRY(hipEventCreateWithFlags(&h->ev_trunk[i], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&h->ev_tail[i], hipEventDisableTiming));
      }
    }
    { int v = 0; if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, cfg->device_id) == hipSuccess && v > 0) h->ncu = h->ncu_dev = v; }
    HIP_TRY(hipMalloc(&h->match_stats, 4 * sizeof(int32_t)));
    HIP_TRY(hipMemset(h->match_stats, 0, 4 * sizeof(int32_t)));
    h->use_graphs = d2fe_dev_env("D2FE_GRAPH", 1) != 0;
    if (lane) { h->use_pinned = false; return D2FE_OK; }
    h->s_cap = h->cfg.max_keypoints > 1024 ? h->cfg.max_keypoints : 1024;      // initial staging capacity per image; grows with the calls (ensure_staging)
    HIP_TRY(hipMalloc(&h->s_img, H * W * B));
    h->s_out_bytes = (sizeof(float) * (size_t)h->s_cap * 260 + sizeof(int32_t)) * B;
    HIP_TRY(hipMalloc(&h->s_out, h->s_out_bytes));
    h->use_pinned = d2fe_dev_env("D2FE_PINNED", 1) != 0;
    if (h->use_pinned) {
      h->pin_in_bytes = (size_t)H * W * B;
      h->pin_out_bytes = h->s_out_bytes;
      if (h->pin_out_bytes < sizeof(float) * 8192 * (size_t)B) h->pin_out_bytes = sizeof(float) * 8192 * (size_t)B;      // NetVLAD descriptors
      if (hipHostMalloc(&h->pin_in, h->pin_in_bytes, hipHostMallocDefault) != hipSuccess ||
          hipHostMalloc(&h->pin_out, h->pin_out_bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        if (h->pin_in) { (void)hipHostFree(h->pin_in); h->pin_in = nullptr; }
        h->pin_out = nullptr; h->use_pinned = false;        // not fatal: the pageable path remains
      }
    }
    return D2FE_OK;
  }();
  // (an adopted stream stays the caller's on failure)
  if (rc_alloc != D2FE_OK) { if (adopt) h->stream = nullptr; d2fe_destroy(h); return rc_alloc; }   // everything allocated so far is released
  // the hipMemsets above ran on the null stream; the handle's work runs on non-blocking streams that do not wait for it
  if (hipDeviceSynchronize() != hipSuccess) { if (adopt) h->stream = nullptr; d2fe_destroy(h); return fail(D2FE_ERR_HIP, "hipDeviceSynchronize"); }
  *out = h;
  return D2FE_OK;
}
}  // namespace d2fe
extern "C" {
int d2fe_create(const d2fe_config* cfg, d2fe_handle* out) { return d2fe::create_context(cfg, out, false); }

void d2fe_destroy(d2fe_handle h) {
  if (!h) return;
  // pipes created from this handle run on ITS packed weights: destroying it under them would leave every lane with dangling pointers.  The destruction is
  // DEFERRED: the handle is marked and the last d2fe_pipe_destroy releases it (a silent refusal leaked the handle when a wrapper destroyed in the
  // wrong order).  Until then the handle must not be used for anything else; d2fe_last_error records what happened
  if (h->live_pipes.load() > 0) { h->doomed.store(true); fail(D2FE_ERR_INVALID, "d2fe_destroy: the handle still has live pipes; it will be released when the last of them is destroyed"); return; }
  hipSetDevice(h->cfg.device_id);
  if (h->stream) hipStreamSynchronize(h->stream);
  if (h->tail_stream) { hipStreamSynchronize(h->tail_stream); (void)hipStreamDestroy(h->tail_stream); }
  for (int i = 0; i < 2; ++i) { if (h->ev_trunk[i]) (void)hipEventDestroy(h->ev_trunk[i]); if (h->ev_tail[i]) (void)hipEventDestroy(h->ev_tail[i]); }
  h->sp_run.release();
  h->sp_net.reset();
  for (void* p : {(void*)h->s_img, h->lk_scratch, (void*)h->match_stats, (void*)h->match_stamps, (void*)h->nv_s_img, (void*)h->nv_s_out})
    if (p) hipFree(p);
  for (auto& kv : h->graphs) if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
  if (h->nv_stream) { hipStreamSynchronize(h->nv_stream); (void)hipStreamDestroy(h->nv_stream); }
  if (h->ev_up) (void)hipEventDestroy(h->ev_up);
  if (h->pin_nv) (void)hipHostFree(h->pin_nv);
  if (h->pin_in) (void)hipHostFree(h->pin_in);
  if (h->pin_out) (void)hipHostFree(h->pin_out);
  if (h->s_out) hipFree(h->s_out);
  for (auto& sc : h->m_scratch) if (sc.cand4) hipFree(sc.cand4);
  for (auto& ms : h->match_slots) { if (ms.stream) { hipStreamSynchronize(ms.stream); (void)hipStreamDestroy(ms.stream); } if (ms.buf) hipFree(ms.buf); if (ms.pin) (void)hipHostFree(ms.pin); }
  for (auto e : h->prof_pool) (void)hipEventDestroy(e);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

int d2fe_superpoint_extract_device(d2fe_handle h, const uint8_t* d_gray, int n, int width, int height, int stride,
                                   size_t image_stride, float* d_kps_xy, float* d_scores, float* d_desc,
                                   int32_t* d_kps_idx, int cap, int32_t* d_n_out, void* stream) {
  int rc = check_geometry(h, n, width, height, stride, cap);
  if (rc) return rc;
  if (!d_gray || !d_kps_xy || !d_scores || !d_desc || !d_n_out) return fail(D2FE_ERR_INVALID, "null device pointer");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  if (!h->cfg.async_tail)
    return run_superpoint(h, d_gray, n, width, height, stride, image_stride, d_kps_xy, d_scores, d_desc, d_kps_idx, cap,
                          d_n_out, s);
  // async_tail: convolutions on `s`, post-processing on the handle's tail stream.  Buffer set p was last read by the tail of
  // the call before the previous one: the trunk may only overwrite it once that tail is done.
  const int p = h->parity;
  HIP_TRY(hipStreamWaitEvent(s, h->ev_tail[p], 0));       // never-recorded event: no-op
  rc = run_superpoint(h, d_gray, n, width, height, stride, image_stride, d_kps_xy, d_scores, d_desc, d_kps_idx, cap, d_n_out, s,
                      h->tail_stream, p);
  if (rc) return rc;
  HIP_TRY(hipEventRecord(h->ev_tail[p], h->tail_stream));
  h->parity = p ^ 1;
  return D2FE_OK;
}

void* d2fe_tail_stream(d2fe_handle h) { return h ? (void*)h->tail_stream : nullptr; }

int d2fe_superpoint_wait_tail(d2fe_handle h, void* stream) {
  if (!h) return fail(D2FE_ERR_INVALID, "null handle");
  if (!h->cfg.async_tail) return D2FE_OK;
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  HIP_TRY(hipStreamWaitEvent(stream ? (hipStream_t)stream : h->stream, h->ev_tail[h->parity ^ 1], 0));
  return D2FE_OK;
}

}  // extern "C"
int d2fe::upload_frames(d2fe_context* h, uint8_t* d_dst, const uint8_t* gray, int n, int width, int height, int stride, size_t image_stride,
                        hipStream_t s) {
  const size_t bytes = (size_t)width * height * n;
  if (h->use_pinned && bytes <= h->pin_in_bytes) {
    HIP_TRY(hipStreamSynchronize(s));            // the previous call's DMA out of pin_in has completed (calls are synchronous: a no-op)
    for (int i = 0; i < n; ++i) {
      const uint8_t* src = gray + i * image_stride;
      uint8_t* dst = h->pin_in + (size_t)i * width * height;
      if (stride == width) memcpy(dst, src, (size_t)width * height);
      else for (int y = 0; y < height; ++y) memcpy(dst + (size_t)y * width, src + (size_t)y * stride, width);
    }
    HIP_TRY(hipMemcpyAsync(d_dst, h->pin_in, bytes, hipMemcpyHostToDevice, s));
    return D2FE_OK;
  }
  if (image_stride == (size_t)stride * height) {
    HIP_TRY(hipMemcpy2DAsync(d_dst, width, gray, stride, width, (size_t)height * n, hipMemcpyHostToDevice, s));
  } else {
    for (int i = 0; i < n; ++i)
      HIP_TRY(hipMemcpy2DAsync(d_dst + (size_t)i * width * height, width, gray + i * image_stride, stride, width, height,
                               hipMemcpyHostToDevice, s));
  }
  return D2FE_OK;
}
extern "C" {

// host-pointer extract of n images; n_netvlad > 0: the NetVLAD descriptors of the first n_netvlad of them as well, from the SAME uploaded frames,
// on a second stream beside SuperPoint (d2fe_extract_all*)
static int extract_host(d2fe_handle h, const uint8_t* gray, int n, int width, int height, int stride, size_t image_stride, float* kps_xy,
                        float* scores, float* desc, int cap, int* n_out, int n_netvlad, float* netvlad_out) {
  if (n_out) for (int i = 0; i < (n > 0 ? n : 0); ++i) n_out[i] = 0;
  int rc = check_geometry(h, n, width, height, stride, cap);
  if (rc) return rc;
  if (!gray || !kps_xy || !scores || !desc || !n_out) return fail(D2FE_ERR_INVALID, "null pointer");
  if (n_netvlad < 0 || n_netvlad > n || (n_netvlad > 0 && !netvlad_out)) return fail(D2FE_ERR_INVALID, "bad NetVLAD image count / null output");
  if (n_netvlad > 0) { rc = nv_check(h, n_netvlad, width, height, stride); if (rc) return rc; }
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  hipStream_t s = h->stream;
  // the call's capacity, bounded by what can exist: H*W candidates (keep-all) or the configured maximum
  const long most = h->cfg.max_keypoints > 0 ? h->cfg.max_keypoints : (long)height * width;
  const int dcap = cap < most ? cap : (int)most;
  const size_t D = (size_t)desc_dim_of(h);
  // outputs of the call, contiguous in one device block: kps [n][dcap][2] | scores [n][dcap] | desc [n][dcap][D] | counts [n] | idx [n][dcap]
  const size_t out_bytes = sizeof(float) * (size_t)n * dcap * (3 + D) + sizeof(int32_t) * n;
  const size_t need = out_bytes + sizeof(int32_t) * (size_t)n * dcap;
  if (need > h->s_out_bytes) {       // grow-only staging: a keep-all call may ask for far more than the initial 1024 per image
    HIP_TRY(hipStreamSynchronize(s));
    graphs_clear(h);                 // captured launch sequences hold the old staging pointers
    if (h->s_out) { hipFree(h->s_out); h->s_out = nullptr; h->s_out_bytes = 0; }
    HIP_TRY(hipMalloc(&h->s_out, need));
    h->s_out_bytes = need;
    if (h->use_pinned && out_bytes > h->pin_out_bytes) {
      if (h->pin_out) { (void)hipHostFree(h->pin_out); h->pin_out = nullptr; h->pin_out_bytes = 0; }
      if (hipHostMalloc(&h->pin_out, out_bytes, hipHostMallocDefault) == hipSuccess) h->pin_out_bytes = out_bytes;
      else { (void)hipGetLastError(); h->pin_out = nullptr; }     // the pageable path below serves calls the pinned buffer cannot
    }
  }
  rc = upload_frames(h, h->s_img, gray, n, width, height, stride, image_stride, s);
  if (rc) return rc;
  size_t nv_bytes = 0;
  // once NetVLAD work is queued on nv_stream, EVERY exit waits for it: its D2H may target the caller's netvlad_out, and the next call's upload
  // overwrites the frames it reads
  struct NvGuard { d2fe_context* h; bool armed = false; ~NvGuard() { if (armed && h->nv_stream) (void)hipStreamSynchronize(h->nv_stream); } } nv_guard{h};
  if (n_netvlad > 0) {
    // NetVLAD reads the frames SuperPoint reads (one upload), on its own stream: at one or two images per call both launch sequences are
    // latency-bound and leave most of the chip idle, so they overlap almost completely (the reference calls infer and then inference
    // for the same image, loop_cam.cpp:609-616)
    // (a stream on another hardware pipe than the handle's own: two busy streams on one pipe take turns, pipe.hip)
    if (!h->nv_stream) { HIP_TRY(create_stream_beside(h->cfg.device_id, h->stream, &h->nv_stream)); HIP_TRY(hipEventCreateWithFlags(&h->ev_up, hipEventDisableTiming)); }
    const int G = d2fe_netvlad_dim(h);
    nv_bytes = sizeof(float) * (size_t)G * n_netvlad;
    if (h->use_pinned && nv_bytes > h->pin_nv_bytes) {
      if (h->pin_nv) { (void)hipHostFree(h->pin_nv); h->pin_nv = nullptr; h->pin_nv_bytes = 0; }
      const size_t want = sizeof(float) * 8192 * (size_t)h->cfg.max_batch;
      if (hipHostMalloc(&h->pin_nv, want > nv_bytes ? want : nv_bytes, hipHostMallocDefault) == hipSuccess) h->pin_nv_bytes = want > nv_bytes ? want : nv_bytes;
      else { (void)hipGetLastError(); h->pin_nv = nullptr; }
    }
    HIP_TRY(hipEventRecord(h->ev_up, s));
    HIP_TRY(hipStreamWaitEvent(h->nv_stream, h->ev_up, 0));
    nv_guard.armed = true;
    rc = run_cached(h, {3, n_netvlad, width, height, (long)h->nv_net->pca_m, 0}, h->nv_stream, [&](hipStream_t st) {
      return run_netvlad(h, h->s_img, n_netvlad, width, height, width, (size_t)width * height, h->nv_s_out, st);
    });
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(h->pin_nv ? (void*)h->pin_nv : (void*)netvlad_out, h->nv_s_out, nv_bytes, hipMemcpyDeviceToHost, h->nv_stream));
  }
  // async_tail handles: a preceding d2fe_superpoint_extract_device call may still have its post-processing running on the tail
  // stream against the single-buffered scratch (candidates, score map, sparse-head slots) that this run uses too
  if (h->cfg.async_tail)
    for (int i = 0; i < 2; ++i) HIP_TRY(hipStreamWaitEvent(s, h->ev_tail[i], 0));
  float* o_kps = h->s_out;
  float* o_sc = o_kps + (size_t)n * dcap * 2;
  float* o_desc = o_sc + (size_t)n * dcap;
  int32_t* o_n = reinterpret_cast<int32_t*>(o_desc + (size_t)n * dcap * D);
  int32_t* o_idx = o_n + n;
  rc = run_cached(h, {1, n, width, height, dcap, (long)D}, s, [&](hipStream_t st) {
    return run_superpoint(h, h->s_img, n, width, height, width, (size_t)width * height, o_kps, o_sc, o_desc, o_idx, dcap, o_n, st);
  });
  if (rc) return rc;
  std::vector<int32_t> ncand(h->cfg.max_keypoints < 0 ? n : 0);
  if (!ncand.empty()) HIP_TRY(hipMemcpyAsync(ncand.data(), h->sp_run.cand_count, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s));
  if (h->use_pinned && h->pin_out && out_bytes <= h->pin_out_bytes) {
    // ONE D2H of the whole block into pinned memory, one synchronisation, then the rows that exist go to the caller's arrays
    HIP_TRY(hipMemcpyAsync(h->pin_out, h->s_out, out_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const float* p_kps = h->pin_out;
    const float* p_sc = p_kps + (size_t)n * dcap * 2;
    const float* p_desc = p_sc + (size_t)n * dcap;
    const int32_t* p_n = reinterpret_cast<const int32_t*>(p_desc + (size_t)n * dcap * D);
    for (int i = 0; i < n; ++i) {
      const int k = p_n[i] < dcap ? p_n[i] : dcap;
      n_out[i] = k;
      if (k > 0) {
        memcpy(kps_xy + (size_t)i * cap * 2, p_kps + (size_t)i * dcap * 2, sizeof(float) * 2 * k);
        memcpy(scores + (size_t)i * cap, p_sc + (size_t)i * dcap, sizeof(float) * k);
        memcpy(desc + (size_t)i * cap * D, p_desc + (size_t)i * dcap * D, sizeof(float) * D * k);
      }
    }
  } else {
    std::vector<int32_t> cnt(n);
    HIP_TRY(hipMemcpyAsync(cnt.data(), o_n, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int i = 0; i < n; ++i) {
      const int k = cnt[i];
      n_out[i] = k;
      if (k > 0) {
        HIP_TRY(hipMemcpyAsync(kps_xy + (size_t)i * cap * 2, o_kps + (size_t)i * dcap * 2, sizeof(float) * 2 * k, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(scores + (size_t)i * cap, o_sc + (size_t)i * dcap, sizeof(float) * k, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(desc + (size_t)i * cap * D, o_desc + (size_t)i * dcap * D, sizeof(float) * D * k, hipMemcpyDeviceToHost, s));
      }
    }
    HIP_TRY(hipStreamSynchronize(s));
  }
  if (n_netvlad > 0) {
    HIP_TRY(hipStreamSynchronize(h->nv_stream));
    nv_guard.armed = false;
    if (h->pin_nv) memcpy(netvlad_out, h->pin_nv, nv_bytes);
  }
  for (int32_t c : ncand)
    if (c > dcap) return fail(D2FE_ERR_TRUNCATED, "max_keypoints = -1: an image has more keypoints than the call's capacity; the first of them in raster order were kept");
  return D2FE_OK;
}

int d2fe_superpoint_extract_batch(d2fe_handle h, const uint8_t* gray, int n, int width, int height, int stride,
                                  size_t image_stride, float* kps_xy, float* scores, float* desc, int cap, int* n_out) {
  return extract_host(h, gray, n, width, height, stride, image_stride, kps_xy, scores, desc, cap, n_out, 0, nullptr);
}

int d2fe_extract_all_batch(d2fe_handle h, const uint8_t* gray, int n, int width, int height, int stride, size_t image_stride, float* kps_xy,
                           float* scores, float* desc, int cap, int* n_out, int n_netvlad, float* netvlad_out) {
  return extract_host(h, gray, n, width, height, stride, image_stride, kps_xy, scores, desc, cap, n_out, n_netvlad, netvlad_out);
}

int d2fe_extract_all(d2fe_handle h, const uint8_t* gray, int width, int height, int stride, float* kps_xy, float* scores, float* desc, int cap,
                     int* n_out, float* netvlad_out) {
  return extract_host(h, gray, 1, width, height, stride, (size_t)stride * height, kps_xy, scores, desc, cap, n_out, 1, netvlad_out);
}

int d2fe_superpoint_extract(d2fe_handle h, const uint8_t* gray, int width, int height, int stride, float* kps_xy,
                            float* scores, float* desc, int cap, int* n_out) {
  return d2fe_superpoint_extract_batch(h, gray, 1, width, height, stride, (size_t)stride * height, kps_xy, scores, desc,
                                       cap, n_out);
}

}  // extern "C"
namespace d2fe {
int clone_lane(d2fe_context* p, int max_batch, d2fe_context** out, hipStream_t stream, int ncu, bool with_netvlad) {
  *out = nullptr;
  d2fe_config cfg = p->cfg;
  cfg.max_batch = max_batch;
  cfg.async_tail = 0;
  d2fe_handle c = nullptr;
  int rc = create_context(&cfg, &c, true, stream);       // on failure the stream stays the caller's (create_context un-adopts it below)
  if (rc) return rc;
  if (ncu > 0) c->ncu = ncu;
  c->sp_net = p->sp_net;      // the network is shared, exact_order's counters with it: one set per parent handle
  c->sp_run.fuse1a = p->sp_run.fuse1a; c->sp_run.wino_dynamic = p->sp_run.wino_dynamic; c->sp_run.sp_min_batch = p->sp_run.sp_min_batch;
  if (p->nv_net && with_netvlad) {
    // the network is shared; the activations are the lane's own (no nv_s_img / nv_s_out: the host-pointer NetVLAD calls never run on a lane)
    c->nv_net = p->nv_net;
    rc = c->nv_run.alloc(*c->nv_net, max_batch);
    if (rc) { if (stream) c->stream = nullptr; d2fe_destroy(c); return rc; }       // the stream stays the caller's
  }
  *out = c;
  return D2FE_OK;
}
}  // namespace d2fe
extern "C" {

// ---- SURVEY 8(f) next rows -------------------------------------------------------------------------------------------------
struct d2fe_db {
  d2fe_context* h = nullptr;
  int dim = 0, cap = 0, ntotal = 0;
  float* vecs = nullptr;
  float* sims = nullptr;   // [maxq][cap] scratch
  float* q = nullptr;      // staged queries
  float* osims = nullptr; int32_t* olabels = nullptr;
  std::mutex mu;
};
namespace { constexpr int DB_MAXQ = 8, DB_MAXK = 1024; }

int d2fe_undistort_device(d2fe_handle h, const uint8_t* d_src, int n, int sw, int sh, int sstride, size_t src_image_stride,
                          const float* d_mapx, const float* d_mapy, const float* d_gain, int dw, int dh, uint8_t* d_dst,
                          void* stream) {
  if (!h || !d_src || !d_mapx || !d_mapy || !d_dst) return fail(D2FE_ERR_INVALID, "null argument");
  if (n < 1 || sw < 1 || sh < 1 || sstride < sw || dw < 1 || dh < 1) return fail(D2FE_ERR_INVALID, "bad geometry");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  HIP_TRY(launch_undistort(d_src, sh, sw, sstride, (long)src_image_stride, d_mapx, d_mapy, d_gain, dh, dw, n, d_dst,
                           stream ? (hipStream_t)stream : h->stream));
  return D2FE_OK;
}

int d2fe_undistort(d2fe_handle h, const uint8_t* src, int sw, int sh, int sstride, const float* mapx, const float* mapy,
                   const float* gain, int dw, int dh, uint8_t* dst) {
  if (!h || !src || !mapx || !mapy || !dst) return fail(D2FE_ERR_INVALID, "null argument");
  if (sw < 1 || sh < 1 || sstride < sw || dw < 1 || dh < 1) return fail(D2FE_ERR_INVALID, "bad geometry");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  const size_t sb = (size_t)sstride * sh, mb = sizeof(float) * (size_t)dw * dh, db = (size_t)dw * dh;
  void* raw = nullptr;
  { const int rc0 = d2fe::ctx_scratch(h, sb + 3 * mb + db + 64, &raw); if (rc0 != D2FE_OK) return rc0; }
  char* buf = static_cast<char*>(raw);
  uint8_t* d_src = reinterpret_cast<uint8_t*>(buf);
  float* d_mx = reinterpret_cast<float*>(buf + ((sb + 15) / 16) * 16);
  float* d_my = d_mx + db; float* d_g = d_my + db;
  uint8_t* d_dst = reinterpret_cast<uint8_t*>(d_g + db);
  hipStream_t s = h->stream;
  int rc = D2FE_OK;
  auto chk = [&](hipError_t e, const char* w) { if (e != hipSuccess && rc == D2FE_OK) rc = fail(D2FE_ERR_HIP, std::string(w) + ": " + hipGetErrorString(e)); };
  chk(hipMemcpyAsync(d_src, src, sb, hipMemcpyHostToDevice, s), "H2D src");
  chk(hipMemcpyAsync(d_mx, mapx, mb, hipMemcpyHostToDevice, s), "H2D mapx");
  chk(hipMemcpyAsync(d_my, mapy, mb, hipMemcpyHostToDevice, s), "H2D mapy");
  if (gain) chk(hipMemcpyAsync(d_g, gain, mb, hipMemcpyHostToDevice, s), "H2D gain");
  if (rc == D2FE_OK) chk(launch_undistort(d_src, sh, sw, sstride, 0, d_mx, d_my, gain ? d_g : nullptr, dh, dw, 1, d_dst, s), "undistort");
  if (rc == D2FE_OK) chk(hipMemcpyAsync(dst, d_dst, db, hipMemcpyDeviceToHost, s), "D2H");
  chk(hipStreamSynchronize(s), "sync");
  return rc;
}

int d2fe_prepare_gray_device(d2fe_handle h, const uint8_t* d_src, int n, int channels, int sw, int sh, int sstride,
                             size_t src_image_stride, int dw, int dh, uint8_t* d_dst, void* stream) {
  if (!h || !d_src || !d_dst) return fail(D2FE_ERR_INVALID, "null argument");
  if (n < 1 || (channels != 1 && channels != 3) || sw < 2 || sh < 2 || sstride < sw * channels || dw < 1 || dh < 1)
    return fail(D2FE_ERR_INVALID, "bad geometry (channels must be 1 or 3)");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  HIP_TRY(launch_prep_gray(d_src, channels, sw, sh, sstride, (long)src_image_stride, n, dw, dh, d_dst, stream ? (hipStream_t)stream : h->stream));
  return D2FE_OK;
}

int d2fe_prepare_gray(d2fe_handle h, const uint8_t* src, int channels, int sw, int sh, int sstride, int dw, int dh, uint8_t* dst) {
  if (!h || !src || !dst) return fail(D2FE_ERR_INVALID, "null argument");
  if ((channels != 1 && channels != 3) || sw < 2 || sh < 2 || sstride < sw * channels || dw < 1 || dh < 1)
    return fail(D2FE_ERR_INVALID, "bad geometry (channels must be 1 or 3)");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  const size_t sb = (size_t)sstride * sh, db = (size_t)dw * dh;
  void* raw = nullptr;
  { const int rc0 = d2fe::ctx_scratch(h, sb + db + 64, &raw); if (rc0 != D2FE_OK) return rc0; }
  uint8_t* d_src = static_cast<uint8_t*>(raw);
  uint8_t* d_dst = d_src + ((sb + 15) / 16) * 16;
  hipStream_t s = h->stream;
  int rc = D2FE_OK;
  auto chk = [&](hipError_t e, const char* w) { if (e != hipSuccess && rc == D2FE_OK) rc = fail(D2FE_ERR_HIP, std::string(w) + ": " + hipGetErrorString(e)); };
  chk(hipMemcpyAsync(d_src, src, sb, hipMemcpyHostToDevice, s), "H2D");
  if (rc == D2FE_OK) chk(launch_prep_gray(d_src, channels, sw, sh, sstride, 0, 1, dw, dh, d_dst, s), "prep_gray");
  if (rc == D2FE_OK) chk(hipMemcpyAsync(dst, d_dst, db, hipMemcpyDeviceToHost, s), "D2H");
  chk(hipStreamSynchronize(s), "sync");
  return rc;
}

static int gen_map(d2fe_handle h, const d2fe_mei_camera* cam, const double* q, int mode, int width, int height, double f,
                   float* mapx, float* mapy, bool device, void* stream) {
  if (!h || !cam || !mapx || !mapy || (mode == 1 && !q)) return fail(D2FE_ERR_INVALID, "null argument");
  if (width < 2 || height < 2 || (size_t)width * height > (1u << 28) || !(f > 0)) return fail(D2FE_ERR_INVALID, "bad map geometry");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  const double c9[9] = {cam->xi, cam->k1, cam->k2, cam->p1, cam->p2, cam->gamma1, cam->gamma2, cam->u0, cam->v0};
  hipStream_t s = device && stream ? (hipStream_t)stream : h->stream;
  if (device) {
    HIP_TRY(launch_gen_map(c9, q, mode, width, height, f, mapx, mapy, s));
    return D2FE_OK;
  }
  const size_t n = (size_t)width * height;
  void* raw = nullptr;
  { const int rc0 = d2fe::ctx_scratch(h, sizeof(float) * 2 * n, &raw); if (rc0 != D2FE_OK) return rc0; }
  float* buf = static_cast<float*>(raw);
  int rc = D2FE_OK;
  auto chk = [&](hipError_t e, const char* w) { if (e != hipSuccess && rc == D2FE_OK) rc = fail(D2FE_ERR_HIP, std::string(w) + ": " + hipGetErrorString(e)); };
  chk(launch_gen_map(c9, q, mode, width, height, f, buf, buf + n, s), "gen_map");
  chk(hipMemcpyAsync(mapx, buf, sizeof(float) * n, hipMemcpyDeviceToHost, s), "D2H mapx");
  chk(hipMemcpyAsync(mapy, buf + n, sizeof(float) * n, hipMemcpyDeviceToHost, s), "D2H mapy");
  chk(hipStreamSynchronize(s), "sync");
  
  return rc;
}
static double cyl_focal(int width, double fov_deg) { return (double)(unsigned)width / (fov_deg * (M_PI / 180.0)); }

int d2fe_gen_cylinder_map(d2fe_handle h, const d2fe_mei_camera* cam, int width, int height, double fov_deg, float* mapx, float* mapy) {
  if (!(fov_deg > 0)) return fail(D2FE_ERR_INVALID, "fov must be positive");
  return gen_map(h, cam, nullptr, 0, width, height, cyl_focal(width, fov_deg), mapx, mapy, false, nullptr);
}
int d2fe_gen_cylinder_map_device(d2fe_handle h, const d2fe_mei_camera* cam, int width, int height, double fov_deg, float* d_mapx,
                                 float* d_mapy, void* stream) {
  if (!(fov_deg > 0)) return fail(D2FE_ERR_INVALID, "fov must be positive");
  return gen_map(h, cam, nullptr, 0, width, height, cyl_focal(width, fov_deg), d_mapx, d_mapy, true, stream);
}
int d2fe_gen_pinhole_map(d2fe_handle h, const d2fe_mei_camera* cam, const double* q_wxyz, int width, int height, double f,
                         float* mapx, float* mapy) {
  return gen_map(h, cam, q_wxyz, 1, width, height, f, mapx, mapy, false, nullptr);
}
int d2fe_gen_pinhole_map_device(d2fe_handle h, const d2fe_mei_camera* cam, const double* q_wxyz, int width, int height, double f,
                                float* d_mapx, float* d_mapy, void* stream) {
  return gen_map(h, cam, q_wxyz, 1, width, height, f, d_mapx, d_mapy, true, stream);
}

void d2fe_db_destroy(d2fe_db_handle db);
int d2fe_db_create(d2fe_handle h, int dim, int capacity, d2fe_db_handle* out) {
  if (!h || !out) return fail(D2FE_ERR_INVALID, "null argument");
  *out = nullptr;
  if (dim < 4 || (dim & 3) || dim > 8192 || capacity < 1) return fail(D2FE_ERR_INVALID, "dim must be a multiple of 4 in 4..8192, capacity >= 1");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  d2fe_db* db = new d2fe_db();
  db->h = h; db->dim = dim; db->cap = capacity;
  const int rc = [&]() -> int {
    HIP_TRY(hipMalloc(&db->vecs, sizeof(float) * (size_t)dim * capacity));
    HIP_TRY(hipMalloc(&db->sims, sizeof(float) * (size_t)DB_MAXQ * capacity));
    HIP_TRY(hipMalloc(&db->q, sizeof(float) * (size_t)DB_MAXQ * dim));
    HIP_TRY(hipMalloc(&db->osims, sizeof(float) * DB_MAXQ * DB_MAXK));
    HIP_TRY(hipMalloc(&db->olabels, sizeof(int32_t) * DB_MAXQ * DB_MAXK));
    return D2FE_OK;
  }();
  if (rc != D2FE_OK) { d2fe_db_destroy(db); return rc; }
  *out = db;
  return D2FE_OK;
}

void d2fe_db_destroy(d2fe_db_handle db) {
  if (!db) return;
  hipSetDevice(db->h->cfg.device_id);
  for (void* p : {(void*)db->vecs, (void*)db->sims, (void*)db->q, (void*)db->osims, (void*)db->olabels}) if (p) hipFree(p);
  delete db;
}

int d2fe_db_ntotal(d2fe_db_handle db) { return db ? db->ntotal : fail(D2FE_ERR_INVALID, "null db"); }

int d2fe_db_add(d2fe_db_handle db, const float* vecs, int n) {
  if (!db || !vecs || n < 1) return fail(D2FE_ERR_INVALID, "bad argument");
  std::lock_guard<std::mutex> lk(db->mu);
  if (db->ntotal + n > db->cap) return fail(D2FE_ERR_TRUNCATED, "database capacity exceeded");
  HIP_TRY(hipSetDevice(db->h->cfg.device_id));
  HIP_TRY(hipMemcpy(db->vecs + (size_t)db->ntotal * db->dim, vecs, sizeof(float) * (size_t)n * db->dim, hipMemcpyHostToDevice));
  const int first = db->ntotal;
  db->ntotal += n;
  return first;
}

int d2fe_db_search(d2fe_db_handle db, const float* q, int nq, int k, float* sims, int32_t* labels) {
  if (!db || !q || !sims || !labels) return fail(D2FE_ERR_INVALID, "null argument");
  if (nq < 1 || nq > DB_MAXQ || k < 1 || k > DB_MAXK || (size_t)nq * db->dim * 4 > 65536) return fail(D2FE_ERR_INVALID, "nq/k out of range");
  std::lock_guard<std::mutex> lk(db->mu);
  for (int i = 0; i < nq * k; ++i) { labels[i] = -1; sims[i] = 0.f; }
  if (db->ntotal == 0) return D2FE_OK;
  HIP_TRY(hipSetDevice(db->h->cfg.device_id));
  hipStream_t s = db->h->stream;
  const int kk = k < db->ntotal ? k : db->ntotal;
  HIP_TRY(hipMemcpyAsync(db->q, q, sizeof(float) * (size_t)nq * db->dim, hipMemcpyHostToDevice, s));
  HIP_TRY(launch_db_search(db->vecs, db->ntotal, db->dim, db->q, nq, kk, db->sims, db->olabels, db->osims, s));
  std::vector<float> hs((size_t)nq * kk); std::vector<int32_t> hl((size_t)nq * kk);
  HIP_TRY(hipMemcpyAsync(hs.data(), db->osims, sizeof(float) * hs.size(), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(hl.data(), db->olabels, sizeof(int32_t) * hl.size(), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (int qi = 0; qi < nq; ++qi)
    for (int r = 0; r < kk; ++r) { sims[(size_t)qi * k + r] = hs[(size_t)qi * kk + r]; labels[(size_t)qi * k + r] = hl[(size_t)qi * kk + r]; }
  return D2FE_OK;
}

int d2fe_db_query_gated(d2fe_db_handle db, const float* q, int max_index, double thres, int32_t* label, float* sim) {
  if (!db || !q || !label || !sim || max_index < 0) return fail(D2FE_ERR_INVALID, "bad argument");
  *label = -1; *sim = 0.f;
  const int ntotal = db->ntotal;
  int k = 5 + max_index;                      // SEARCH_NEAREST_NUM, d2frontend_params.h:22
  if (k > ntotal) k = ntotal;
  if (k <= 0) return D2FE_OK;
  if (k > DB_MAXK) k = DB_MAXK;
  std::vector<float> s(k); std::vector<int32_t> l(k);
  int rc = d2fe_db_search(db, q, 1, k, s.data(), l.data());
  if (rc) return rc;
  for (int i = 0; i < k; ++i) {
    if (l[i] < 0) continue;
    if (l[i] <= ntotal - max_index && (double)s[i] > thres) { *label = l[i]; *sim = s[i]; return D2FE_OK; }
  }
  return D2FE_OK;
}

static int codec_run(d2fe_handle h, const void* in, size_t in_bytes, void* out, size_t out_bytes, int n, int arg, bool quant) {
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  void* raw = nullptr;
  { const int rc0 = d2fe::ctx_scratch(h, in_bytes + out_bytes + 64, &raw); if (rc0 != D2FE_OK) return rc0; }
  char* buf = static_cast<char*>(raw);
  char* d_out = buf + ((in_bytes + 15) / 16) * 16;
  hipStream_t s = h->stream;
  int rc = D2FE_OK;
  auto chk = [&](hipError_t e, const char* w) { if (e != hipSuccess && rc == D2FE_OK) rc = fail(D2FE_ERR_HIP, std::string(w) + ": " + hipGetErrorString(e)); };
  chk(hipMemcpyAsync(buf, in, in_bytes, hipMemcpyHostToDevice, s), "H2D");
  if (rc == D2FE_OK) {
    if (quant) chk(launch_quant_int8(reinterpret_cast<const float*>(buf), n, arg, reinterpret_cast<int8_t*>(d_out), s), "quant");
    else chk(launch_dequant_int8(reinterpret_cast<const int8_t*>(buf), n, arg, reinterpret_cast<float*>(d_out), s), "dequant");
  }
  if (rc == D2FE_OK) chk(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, s), "D2H");
  chk(hipStreamSynchronize(s), "sync");
  return rc;
}

int d2fe_quantize_int8(d2fe_handle h, const float* x, int n, int double_max, int8_t* out) {
  if (!h || !x || !out || n < 1) return fail(D2FE_ERR_INVALID, "bad argument");
  return codec_run(h, x, sizeof(float) * (size_t)n, out, (size_t)n, n, double_max ? 1 : 0, true);
}

int d2fe_dequantize_int8(d2fe_handle h, const int8_t* q, int n, int landmark_num, float* out) {
  if (!h || !q || !out || n < 1) return fail(D2FE_ERR_INVALID, "bad argument");
  if (landmark_num >= 0 && (n & 31)) return fail(D2FE_ERR_INVALID, "landmark descriptors: n must be a multiple of 32");
  return codec_run(h, q, (size_t)n, out, sizeof(float) * (size_t)n, n, landmark_num, false);
}

// desc_dim: 4..256, a multiple of 4 (rows stay 16-byte aligned behind the descriptors of a block)
static bool block_dim_ok(int desc_dim) { return desc_dim >= 4 && desc_dim <= 256 && !(desc_dim & 3); }
int d2fe_block_field_offset_d(int cap, int desc_dim, int netvlad_dim, int field) {
  if (cap < 1 || !block_dim_ok(desc_dim) || netvlad_dim < 0 || field < 0 || field > 4) return fail(D2FE_ERR_INVALID, "bad argument");
  const int off[5] = {0, cap * desc_dim, cap * (desc_dim + 2), cap * (desc_dim + 3), cap * (desc_dim + 3) + netvlad_dim};
  return off[field];
}
int d2fe_block_field_offset(int cap, int netvlad_dim, int field) { return d2fe_block_field_offset_d(cap, 256, netvlad_dim, field); }
int d2fe_block_words_d(int cap, int desc_dim, int netvlad_dim) {
  if (cap < 1 || !block_dim_ok(desc_dim) || netvlad_dim < 0 || (netvlad_dim & 3)) return fail(D2FE_ERR_INVALID, "bad argument");
  return (cap * (desc_dim + 3) + netvlad_dim + 1 + 255) / 256 * 256;
}
int d2fe_block_words(int cap, int netvlad_dim) { return d2fe_block_words_d(cap, 256, netvlad_dim); }
int d2fe_pack_blocks_device_d(d2fe_handle h, const float* d_desc, const float* d_kps_xy, const float* d_scores, const int32_t* d_n,
                              const float* d_netvlad, int row0, int row_step, int nframes, int cap, int desc_dim, int netvlad_dim, float* d_blocks,
                              void* stream) {
  if (!h || !d_desc || !d_kps_xy || !d_scores || !d_n || !d_blocks) return fail(D2FE_ERR_INVALID, "null argument");
  if (nframes < 1 || cap < 1 || row0 < 0 || row_step < 1 || !block_dim_ok(desc_dim) || netvlad_dim < 0 || (netvlad_dim & 3)) return fail(D2FE_ERR_INVALID, "bad geometry");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  HIP_TRY(launch_pack_blocks(d_desc, d_kps_xy, d_scores, d_n, d_netvlad, row0, row_step, nframes, cap, desc_dim, netvlad_dim,
                             d2fe_block_words_d(cap, desc_dim, netvlad_dim), d_blocks, stream ? (hipStream_t)stream : h->stream));
  return D2FE_OK;
}
int d2fe_pack_blocks_device(d2fe_handle h, const float* d_desc, const float* d_kps_xy, const float* d_scores, const int32_t* d_n,
                            const float* d_netvlad, int row0, int row_step, int nframes, int cap, int netvlad_dim, float* d_blocks,
                            void* stream) {
  return d2fe_pack_blocks_device_d(h, d_desc, d_kps_xy, d_scores, d_n, d_netvlad, row0, row_step, nframes, cap, 256, netvlad_dim, d_blocks, stream);
}
int d2fe_gate_pairs_device(d2fe_handle h, const float* d_q, size_t q_stride, const float* d_db, size_t db_stride, int dim,
                           const int32_t* d_pair_q, const int32_t* d_pair_db, int npairs, double thres, int32_t* d_cnt_inout,
                           int32_t* d_pass, float* d_sims, int32_t* d_n_pass, void* stream) {
  if (!h || !d_q || !d_db || !d_pair_q || !d_pair_db) return fail(D2FE_ERR_INVALID, "null argument");
  if (npairs < 1 || dim < 4 || (dim & 3)) return fail(D2FE_ERR_INVALID, "dim must be a multiple of 4");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  HIP_TRY(launch_gate_pairs(d_q, (long)q_stride, d_db, (long)db_stride, dim, d_pair_q, d_pair_db, npairs, thres, d_cnt_inout, d_pass,
                            d_sims, d_n_pass, stream ? (hipStream_t)stream : h->stream));
  return D2FE_OK;
}

int d2fe_block_bytes_int8_d(int cap, int desc_dim, int netvlad_dim) {
  if (cap < 1 || !block_dim_ok(desc_dim) || netvlad_dim < 0 || (netvlad_dim & 3)) return fail(D2FE_ERR_INVALID, "bad argument");
  return (cap * desc_dim + netvlad_dim + cap * 8 + 4 + 63) / 64 * 64;
}
int d2fe_block_bytes_int8(int cap, int netvlad_dim) { return d2fe_block_bytes_int8_d(cap, 256, netvlad_dim); }
int d2fe_pack_blocks_int8_device_d(d2fe_handle h, const float* d_desc, const float* d_kps_xy, const int32_t* d_n, const float* d_netvlad,
                                   int row0, int row_step, int nframes, int cap, int desc_dim, int netvlad_dim, int8_t* d_blocks, void* stream) {
  if (!h || !d_desc || !d_kps_xy || !d_n || !d_blocks) return fail(D2FE_ERR_INVALID, "null argument");
  if (nframes < 1 || cap < 1 || row0 < 0 || row_step < 1 || !block_dim_ok(desc_dim) || netvlad_dim < 0 || (netvlad_dim & 3)) return fail(D2FE_ERR_INVALID, "bad geometry");
  if (((uintptr_t)d_desc & 15) || ((uintptr_t)d_blocks & 3)) return fail(D2FE_ERR_INVALID, "d_desc must be 16-byte aligned, d_blocks 4-byte aligned");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  HIP_TRY(launch_pack_blocks_int8(d_desc, d_kps_xy, d_n, d_netvlad, row0, row_step, nframes, cap, desc_dim, netvlad_dim,
                                  d2fe_block_bytes_int8_d(cap, desc_dim, netvlad_dim), d_blocks, stream ? (hipStream_t)stream : h->stream));
  return D2FE_OK;
}
int d2fe_pack_blocks_int8_device(d2fe_handle h, const float* d_desc, const float* d_kps_xy, const int32_t* d_n, const float* d_netvlad,
                                 int row0, int row_step, int nframes, int cap, int netvlad_dim, int8_t* d_blocks, void* stream) {
  return d2fe_pack_blocks_int8_device_d(h, d_desc, d_kps_xy, d_n, d_netvlad, row0, row_step, nframes, cap, 256, netvlad_dim, d_blocks, stream);
}
int d2fe_unpack_blocks_int8_device_d(d2fe_handle h, const int8_t* d_blocks_int8, int nblocks, int cap, int desc_dim, int netvlad_dim, int renorm,
                                     float* d_blocks, void* stream) {
  if (!h || !d_blocks_int8 || !d_blocks) return fail(D2FE_ERR_INVALID, "null argument");
  if (nblocks < 1 || cap < 1 || !block_dim_ok(desc_dim) || netvlad_dim < 0 || (netvlad_dim & 3) || (renorm != 0 && renorm != 1)) return fail(D2FE_ERR_INVALID, "bad geometry");
  if (((uintptr_t)d_blocks & 15) || ((uintptr_t)d_blocks_int8 & 3)) return fail(D2FE_ERR_INVALID, "d_blocks must be 16-byte aligned, d_blocks_int8 4-byte aligned");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  HIP_TRY(launch_unpack_blocks_int8(d_blocks_int8, nblocks, cap, desc_dim, netvlad_dim, d2fe_block_bytes_int8_d(cap, desc_dim, netvlad_dim),
                                    d2fe_block_words_d(cap, desc_dim, netvlad_dim), renorm, d_blocks, stream ? (hipStream_t)stream : h->stream));
  return D2FE_OK;
}
int d2fe_unpack_blocks_int8_device(d2fe_handle h, const int8_t* d_blocks_int8, int nblocks, int cap, int netvlad_dim, int renorm,
                                   float* d_blocks, void* stream) {
  return d2fe_unpack_blocks_int8_device_d(h, d_blocks_int8, nblocks, cap, 256, netvlad_dim, renorm, d_blocks, stream);
}

int d2fe_quad_gate_device(d2fe_handle h, const float* d_local, size_t local_stride, const float* d_remote, size_t remote_stride, int dim,
                          const int32_t* d_job_local_row0, const int32_t* d_job_remote_row0, int local_view_step, int remote_view_step,
                          int njobs, double thres, int32_t* d_dir_prev, float* d_sims, int32_t* d_cnt_inout, int32_t* d_n_pass,
                          void* stream) {
  if (!h || !d_local || !d_remote || !d_job_local_row0 || !d_job_remote_row0) return fail(D2FE_ERR_INVALID, "null argument");
  if (njobs < 1 || dim < 4 || (dim & 3) || local_view_step < 1 || remote_view_step < 1) return fail(D2FE_ERR_INVALID, "bad geometry");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  HIP_TRY(launch_quad_gate(d_local, (long)local_stride, d_remote, (long)remote_stride, dim, d_job_local_row0, d_job_remote_row0,
                           local_view_step, remote_view_step, njobs, thres, d_dir_prev, d_sims, d_cnt_inout, d_n_pass,
                           stream ? (hipStream_t)stream : h->stream));
  return D2FE_OK;
}

float d2fe_half_move_cols(int width_undistort, double undistort_fov) { return (float)((double)width_undistort * 90.0 / undistort_fov); }
int d2fe_half_image_compact_device(d2fe_handle h, const float* d_desc, const float* d_pts_xy, const int32_t* d_n, const int32_t* d_job_row,
                                   const int32_t* d_job_left, const float* d_job_shift_x, int njobs, int cap, int dim, int width_undistort,
                                   double undistort_fov, float* d_out_desc, float* d_out_pts, int32_t* d_out_map, int32_t* d_out_n,
                                   void* stream) {
  if (!h || !d_desc || !d_pts_xy || !d_n || !d_job_row || !d_job_left || !d_job_shift_x || !d_out_desc || !d_out_pts || !d_out_map || !d_out_n)
    return fail(D2FE_ERR_INVALID, "null argument");
  if (njobs < 1 || cap < 1 || cap > 1024 || dim < 4 || (dim & 3) || width_undistort < 1 || !(undistort_fov > 0)) return fail(D2FE_ERR_INVALID, "bad geometry");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  HIP_TRY(launch_half_compact(d_desc, d_pts_xy, d_n, d_job_row, d_job_left, d_job_shift_x, njobs, cap, dim, (float)width_undistort,
                              d2fe_half_move_cols(width_undistort, undistort_fov), d_out_desc, d_out_pts, d_out_map, d_out_n,
                              stream ? (hipStream_t)stream : h->stream));
  return D2FE_OK;
}
int d2fe_remap_matches_device(d2fe_handle h, int32_t* d_q_idx, int32_t* d_t_idx, const int32_t* d_n_match, const int32_t* d_map_a_job,
                              const int32_t* d_map_b_job, const int32_t* d_maps, int npairs, int cap_match, int cap_map, void* stream) {
  if (!h || !d_q_idx || !d_t_idx || !d_n_match || !d_map_a_job || !d_map_b_job || !d_maps) return fail(D2FE_ERR_INVALID, "null argument");
  if (npairs < 1 || cap_match < 1 || cap_map < 1) return fail(D2FE_ERR_INVALID, "bad geometry");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  HIP_TRY(launch_remap_matches(d_q_idx, d_t_idx, d_n_match, d_map_a_job, d_map_b_job, d_maps, npairs, cap_match, cap_map,
                               stream ? (hipStream_t)stream : h->stream));
  return D2FE_OK;
}

int d2fe_match_batch_device(d2fe_handle h, const d2fe_match_batch* mb, void* stream) {
  if (!h || !mb) return fail(D2FE_ERR_INVALID, "null argument");
  if (mb->npairs < 1 || mb->max_n < 1 || mb->max_n > 16384) return fail(D2FE_ERR_INVALID, "npairs/max_n out of range (max_n <= 16384)");
  if (mb->dim < 4 || mb->dim > 256 || (mb->dim & 3)) return fail(D2FE_ERR_INVALID, "dim must be a multiple of 4 in 4..256");
  if (mb->mode != 0 && mb->mode != 1) return fail(D2FE_ERR_INVALID, "bad mode");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  std::lock_guard<std::mutex> lk(h->match_mu);
  // the candidate scratch is keyed by the caller's stream: two calls on different streams (main and tail, two threads) can
  // overlap on the GPU and must not share cand4[pair][dir][row]; calls on one stream are ordered by the stream itself
  d2fe_context::MatchScratch* sc = nullptr;
  for (auto& e : h->m_scratch) if (e.stream == s) { sc = &e; break; }
  if (!sc) { h->m_scratch.emplace_back(); sc = &h->m_scratch.back(); sc->stream = s; }
  // [arrival tickets | records]; the tickets are zero between launches (the kernel's last workgroup per pair resets its own), so a scratch
  // sized for more pairs serves any smaller batch
  const int tp = mb->npairs > sc->npairs ? mb->npairs : sc->npairs;
  const size_t need = match_scratch_bytes(tp, 0) + sizeof(int32_t) * 8 * (size_t)mb->max_n * mb->npairs;
  if (need > sc->bytes || mb->npairs > sc->npairs) {
    HIP_TRY(hipStreamSynchronize(s));      // the only work that can still read the old scratch is on this stream
    if (sc->cand4) hipFree(sc->cand4);
    sc->cand4 = nullptr; sc->bytes = 0; sc->npairs = 0;
    const size_t want = need > sc->bytes ? need : sc->bytes;
    HIP_TRY(hipMalloc(&sc->cand4, want));
    HIP_TRY(hipMemsetAsync(sc->cand4, 0, want, s));      // ON the caller's stream: hipMemset runs on the null stream, which a non-blocking stream does not wait for
    sc->bytes = want; sc->npairs = tp;
  }
  MatchArgs m;
  m.a = mb->d_a; m.b = mb->d_b; m.pts_a = mb->d_pts_a; m.pts_b = mb->d_pts_b;
  m.a_off = mb->d_a_off; m.b_off = mb->d_b_off; m.a_cnt = mb->d_a_cnt; m.b_cnt = mb->d_b_cnt;
  m.npairs = mb->npairs; m.dim = mb->dim; m.max_n = mb->max_n; m.mode = mb->mode;
  m.ratio = mb->ratio; m.radius = mb->radius;
  m.q_idx = mb->d_q_idx; m.t_idx = mb->d_t_idx; m.dist = mb->d_dist; m.n_out = mb->d_n_out;
  match_scratch_carve(sc->cand4, sc->npairs, &m); m.stats = h->match_stats; m.ncu = h->ncu;
#ifdef D2FE_DEVTOOLS
  if (d2fe_dev_env("D2FE_MATCH_STAMPS", 0) && (long)((mb->max_n + 31) / 32) * 2 * mb->npairs <= 4096) {
    if (!h->match_stamps) HIP_TRY(hipMalloc(&h->match_stamps, sizeof(unsigned long long) * 16 * 4096));
    HIP_TRY(hipMemsetAsync(h->match_stamps, 0, sizeof(unsigned long long) * 16 * 4096, s));
    m.stamps = h->match_stamps;
  }
#endif
  { ProfScope ps(h, D2FE_PROF_MATCH, s); HIP_TRY(launch_match(m, s)); }
  return D2FE_OK;
}

static int match_host(d2fe_handle h, int mode, const float* a, int na, const float* b, int nb, int dim, double ratio,
                      const float* pts_a, const float* pts_b, double radius, int32_t* q_idx, int32_t* t_idx, float* dist,
                      int cap, int* n_out) {
  if (n_out) *n_out = 0;
  if (!h || !n_out) return fail(D2FE_ERR_INVALID, "null argument");
  if (na < 0 || nb < 0 || cap < 0) return fail(D2FE_ERR_INVALID, "negative size");
  if (na == 0 || nb == 0) return D2FE_OK;
  if (!a || !b || !q_idx || !t_idx || !dist) return fail(D2FE_ERR_INVALID, "null pointer");
  const int max_n = na > nb ? na : nb;
  if (max_n > 16384) return fail(D2FE_ERR_UNSUPPORTED, "more than 16384 descriptors per side");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  const bool use_pts = mode == 0 && radius > 0 && pts_a && pts_b;
  const size_t fa = (size_t)na * dim, fb = (size_t)nb * dim;
  if (dim < 4 || dim > 256 || (dim & 3)) return fail(D2FE_ERR_INVALID, "dim must be a multiple of 4 in 4..256");
  // a private (stream, scratch) slot per call in flight: re-entrant; slots are created on demand and reused
  // a slot's buffers are sized for 1024 rows per side at first (every shipped configuration) and grow with the calls
  const size_t rows = (size_t)(max_n > 1024 ? max_n : 1024);
  const size_t slot_bytes = sizeof(float) * (2 * rows * 256 + 4 * rows + rows) + sizeof(int32_t) * (2 * rows + 16 + 8 * rows) + 128;
  int slot = -1;
  hipStream_t s = nullptr;
  char* buf = nullptr;
  char* pin = nullptr;
  d2fe_context::MatchSlot* msp = nullptr;       // taken under the lock: a deque never relocates its elements, but indexing it races with an append
  {
    std::lock_guard<std::mutex> lk(h->match_mu);
    for (size_t i = 0; i < h->match_slots.size(); ++i)
      if (!h->match_slots[i].busy) { slot = (int)i; break; }
    if (slot < 0) {
      d2fe_context::MatchSlot ms;
      if (hipStreamCreateWithFlags(&ms.stream, hipStreamNonBlocking) != hipSuccess) return fail(D2FE_ERR_HIP, "hipStreamCreate (match slot)");
      h->match_slots.push_back(ms);
      slot = (int)h->match_slots.size() - 1;
    }
    d2fe_context::MatchSlot& ms = h->match_slots[slot];
    ms.busy = true;      // the slot is this call's from here on: the (re)allocation below happens OUTSIDE the lock (hipFree / hipHostFree synchronise the device)
    s = ms.stream;      // read under the lock: another thread may be appending a slot right now
    msp = &ms;
  }
  struct Release { d2fe_context* h; int slot; ~Release() { std::lock_guard<std::mutex> lk(h->match_mu); h->match_slots[slot].busy = false; } } release{h, slot};
  {
    d2fe_context::MatchSlot& ms = *msp;
    if (ms.bytes < slot_bytes) {
      if (ms.buf) { hipFree(ms.buf); ms.buf = nullptr; }
      if (ms.pin) { (void)hipHostFree(ms.pin); ms.pin = nullptr; }
      ms.bytes = 0;
      if (hipMalloc(&ms.buf, slot_bytes) != hipSuccess) return fail(D2FE_ERR_HIP, "hipMalloc match scratch");
      if (h->use_pinned && hipHostMalloc(&ms.pin, slot_bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); ms.pin = nullptr; }
      ms.bytes = slot_bytes;
    }
    buf = ms.buf;
    pin = ms.pin;
  }
  // device layout (words): a | b | pts_a | pts_b | meta {a_off, b_off, a_cnt, b_cnt, arrival ticket (0), pad x3} | n_out, pad x7 | dist | q | t | cand4
  // -- the inputs are one contiguous run (ONE H2D from the slot's pinned mirror), the outputs another (ONE D2H, one synchronisation)
  const size_t w_in = fa + fb + (use_pts ? 2 * (size_t)(na + nb) : 0) + 8;
  float* d_a = reinterpret_cast<float*>(buf);
  float* d_b = d_a + fa;
  float* d_pa = d_b + fb;
  float* d_pb = d_pa + (use_pts ? 2 * (size_t)na : 0);
  int32_t* d_meta = reinterpret_cast<int32_t*>(d_pb + (use_pts ? 2 * (size_t)nb : 0));
  int32_t* d_nout = d_meta + 8;
  float* d_dist = reinterpret_cast<float*>(d_nout + 8);
  int32_t* d_q = reinterpret_cast<int32_t*>(d_dist + max_n);
  int32_t* d_t = d_q + max_n;
  int32_t* d_c4 = d_t + max_n;
  const size_t w_out = 8 + 3 * (size_t)max_n;
  const int32_t meta[8] = {0, 0, na, nb, 0, 0, 0, 0};
  int rc = D2FE_OK;
  auto chk = [&](hipError_t er, const char* what) { if (er != hipSuccess && rc == D2FE_OK) rc = fail(D2FE_ERR_HIP, std::string(what) + ": " + hipGetErrorString(er)); };
  if (pin) {
    float* p = reinterpret_cast<float*>(pin);
    memcpy(p, a, sizeof(float) * fa); memcpy(p + fa, b, sizeof(float) * fb);
    float* pm = p + fa + fb;
    if (use_pts) { memcpy(pm, pts_a, sizeof(float) * 2 * na); memcpy(pm + 2 * (size_t)na, pts_b, sizeof(float) * 2 * nb); pm += 2 * (size_t)(na + nb); }
    memcpy(pm, meta, sizeof(meta));
    chk(hipMemcpyAsync(d_a, pin, sizeof(float) * w_in, hipMemcpyHostToDevice, s), "H2D inputs");
  } else {
    chk(hipMemcpyAsync(d_a, a, sizeof(float) * fa, hipMemcpyHostToDevice, s), "H2D a");
    chk(hipMemcpyAsync(d_b, b, sizeof(float) * fb, hipMemcpyHostToDevice, s), "H2D b");
    if (use_pts) {
      chk(hipMemcpyAsync(d_pa, pts_a, sizeof(float) * 2 * na, hipMemcpyHostToDevice, s), "H2D pts_a");
      chk(hipMemcpyAsync(d_pb, pts_b, sizeof(float) * 2 * nb, hipMemcpyHostToDevice, s), "H2D pts_b");
    }
    chk(hipMemcpyAsync(d_meta, meta, sizeof(meta), hipMemcpyHostToDevice, s), "H2D meta");
  }
  MatchArgs m;
  m.a = d_a; m.b = d_b; m.pts_a = use_pts ? d_pa : nullptr; m.pts_b = use_pts ? d_pb : nullptr;
  m.a_off = d_meta; m.b_off = d_meta + 1; m.a_cnt = d_meta + 2; m.b_cnt = d_meta + 3;
  m.npairs = 1; m.dim = dim; m.max_n = max_n; m.mode = mode; m.ratio = ratio; m.radius = use_pts ? radius : -1.0;
  m.q_idx = d_q; m.t_idx = d_t; m.dist = d_dist; m.n_out = d_nout; m.cand4 = d_c4; m.stats = h->match_stats;
  m.ncu = h->ncu;
  m.ticket = d_meta + 4;      // a zero word of the meta block: uploaded with the inputs, so zero at every launch
  if (rc == D2FE_OK) chk(launch_match(m, s), "launch_match");
  if (pin) {
    // pinned mirror of the output run, behind the inputs' mirror
    int32_t* po = reinterpret_cast<int32_t*>(pin) + ((w_in + 15) & ~(size_t)15);
    if (rc == D2FE_OK) chk(hipMemcpyAsync(po, d_nout, sizeof(int32_t) * w_out, hipMemcpyDeviceToHost, s), "D2H results");
    if (rc == D2FE_OK) chk(hipStreamSynchronize(s), "sync");
    if (rc == D2FE_OK) {
      const int cnt = po[0];
      const int k = cnt < cap ? cnt : cap;
      if (k > 0) {
        memcpy(dist, po + 8, sizeof(float) * k);
        memcpy(q_idx, po + 8 + max_n, sizeof(int32_t) * k);
        memcpy(t_idx, po + 8 + 2 * (size_t)max_n, sizeof(int32_t) * k);
      }
      *n_out = k;
      if (cnt > cap) rc = fail(D2FE_ERR_TRUNCATED, "match output capacity too small");
    }
    return rc;
  }
  int32_t cnt = 0;
  if (rc == D2FE_OK) chk(hipMemcpyAsync(&cnt, d_nout, sizeof(int32_t), hipMemcpyDeviceToHost, s), "D2H n");
  if (rc == D2FE_OK) chk(hipStreamSynchronize(s), "sync");
  if (rc == D2FE_OK) {
    const int k = cnt < cap ? cnt : cap;
    if (k > 0) {
      chk(hipMemcpyAsync(q_idx, d_q, sizeof(int32_t) * k, hipMemcpyDeviceToHost, s), "D2H q");
      chk(hipMemcpyAsync(t_idx, d_t, sizeof(int32_t) * k, hipMemcpyDeviceToHost, s), "D2H t");
      chk(hipMemcpyAsync(dist, d_dist, sizeof(float) * k, hipMemcpyDeviceToHost, s), "D2H d");
      chk(hipStreamSynchronize(s), "sync2");
    }
    *n_out = k;
    if (rc == D2FE_OK && cnt > cap) rc = fail(D2FE_ERR_TRUNCATED, "match output capacity too small");
  }
  return rc;
}

int d2fe_match_knn(d2fe_handle h, const float* a, int na, const float* b, int nb, int dim, double ratio,
                   const float* pts_a, const float* pts_b, double radius, int32_t* q_idx, int32_t* t_idx, float* dist,
                   int cap, int* n_out) {
  return match_host(h, 0, a, na, b, nb, dim, ratio, pts_a, pts_b, radius, q_idx, t_idx, dist, cap, n_out);
}

int d2fe_match_crosscheck(d2fe_handle h, const float* a, int na, const float* b, int nb, int dim, int32_t* q_idx,
                          int32_t* t_idx, float* dist, int cap, int* n_out) {
  return match_host(h, 1, a, na, b, nb, dim, 0.0, nullptr, nullptr, -1.0, q_idx, t_idx, dist, cap, n_out);
}

int d2fe_half_image_filter(const float* pts_xy, int n, int require_left, int width_undistort, double undistort_fov,
                           int32_t* map, int* n_out) {
  if (!n_out) return fail(D2FE_ERR_INVALID, "null argument");
  *n_out = 0;
  if (n < 0 || (n > 0 && (!pts_xy || !map))) return fail(D2FE_ERR_INVALID, "null pointer");
  // host bookkeeping on <= N points (d2featuretracker.cpp:1058-1071); float move_cols as in the reference
  const float move_cols = (float)((double)width_undistort * 90.0 / undistort_fov);
  int c = 0;
  for (int i = 0; i < n; ++i) {
    const float x = pts_xy[2 * i];
    if ((require_left && x < (float)width_undistort - move_cols) || (!require_left && x >= move_cols)) map[c++] = i;
  }
  *n_out = c;
  return D2FE_OK;
}

#ifdef D2FE_DEVTOOLS      /* development library only: include/d2fe_debug.h */
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

// comp == nullptr: d2fe_debug_sample_b (rows of 256 floats); else d2fe_debug_sample_b_pca (rows of pca_dims floats)
static int debug_sample_b(d2fe_handle h, const float* desc_raw, int dstride, int dcoff, int n, int Hc, int Wc, const float* kps_xy, const int32_t* n_kp, int cap,
                          const int32_t* slotmap_or_null, int max_slots, const float* comp, const float* mean, int pca_dims, float* desc_out) {
  if (!h || !desc_raw || !kps_xy || !n_kp || !desc_out) return fail(D2FE_ERR_INVALID, "null argument");
  if (n < 1 || Hc < 2 || Wc < 2 || cap < 1 || (long)Hc * Wc * 64 > DEBUG_MAX_PIXELS || cap > DEBUG_MAX_PIXELS) return fail(D2FE_ERR_INVALID, "bad geometry");
  const size_t ncell = (size_t)Hc * Wc;
  if (slotmap_or_null) {      // sparse store [img][max_slots][256]: every cell the kernel may look up must name a slot of the store
    if (max_slots < 1 || max_slots > DEBUG_MAX_PIXELS) return fail(D2FE_ERR_INVALID, "max_slots");
    for (size_t i = 0; i < (size_t)n * ncell; ++i)
      if (slotmap_or_null[i] < 0 || slotmap_or_null[i] >= max_slots) return fail(D2FE_ERR_INVALID, "slot map entry outside [0, max_slots)");
  } else if (dcoff < 0 || (dcoff & 3) || (dstride & 3) || dstride < dcoff + 256 || dstride > 4096) {
    return fail(D2FE_ERR_INVALID, "dense form: dcoff and dstride are multiples of 4 with dcoff + 256 <= dstride");
  }
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  DevPool b;
  float *d_raw = nullptr, *d_kps = nullptr, *d_desc = nullptr;
  int32_t *d_n = nullptr, *d_map = nullptr;
  HIP_TRY(b.get(&d_raw, sizeof(float) * n * (slotmap_or_null ? (size_t)max_slots * 256 : ncell * dstride), desc_raw));
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

#endif  // D2FE_DEVTOOLS

int d2fe_profile_enable(d2fe_handle h, int mode) {
  if (!h || mode < 0 || mode > 2) return fail(D2FE_ERR_INVALID, "bad argument");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  HIP_TRY(hipDeviceSynchronize());
  h->prof_mode = mode;
  h->prof_used = 0;
  h->prof_recs.clear();
  return D2FE_OK;
}

int d2fe_profile_read(d2fe_handle h, float* ms, int32_t* launches) {
  if (!h || !ms || !launches) return fail(D2FE_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  HIP_TRY(hipDeviceSynchronize());
  for (int i = 0; i < D2FE_PROF_COUNT; ++i) { ms[i] = 0.f; launches[i] = 0; }
  for (auto& r : h->prof_recs) {
    float t = 0.f;
    HIP_TRY(hipEventElapsedTime(&t, r.a, r.b));
    ms[r.stage] += t;
    launches[r.stage] += 1;
  }
  h->prof_used = 0;
  h->prof_recs.clear();
  return D2FE_OK;
}

#ifdef D2FE_DEVTOOLS
int d2fe_debug_graph_count(d2fe_handle h, int* rejected) {
  if (!h) return fail(D2FE_ERR_INVALID, "null handle");
  int n = 0, bad = 0;
  for (auto& kv : h->graphs) { n += kv.second.exec != nullptr; bad += kv.second.bad; }
  if (rejected) *rejected = bad;
  return n;
}

/* development builds: the wall_clock64() phase stamps [workgroup][16] of the last d2fe_match_batch_device launch made with D2FE_MATCH_STAMPS set */
D2FE_API long d2fe_debug_match_stamps(d2fe_handle h, unsigned long long* dst, long max_wgs) {
  if (!h || !dst || !h->match_stamps) return fail(D2FE_ERR_NOT_READY, "no stamped launch yet (D2FE_MATCH_STAMPS)");
  hipSetDevice(h->cfg.device_id);
  const long nw = max_wgs < 4096 ? max_wgs : 4096;
  if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(dst, h->match_stamps, sizeof(unsigned long long) * 16 * nw, hipMemcpyDeviceToHost) != hipSuccess)
    return fail(D2FE_ERR_HIP, "D2H");
  return nw;
}
#endif

long d2fe_match_fallback_rows(d2fe_handle h, int reset, long* full_scans) {
  if (!h) return fail(D2FE_ERR_INVALID, "null handle");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  HIP_TRY(hipDeviceSynchronize());
  int32_t v[2] = {0, 0};
  HIP_TRY(hipMemcpy(v, h->match_stats, sizeof(v), hipMemcpyDeviceToHost));
  if (reset) { HIP_TRY(hipMemset(h->match_stats, 0, sizeof(v))); HIP_TRY(hipDeviceSynchronize()); }
  if (full_scans) *full_scans = v[0];
  return v[1];
}

int d2fe_exact_order_stats(d2fe_handle h, int64_t out[4]) {
  if (!h || !out) return fail(D2FE_ERR_INVALID, "null argument");
  out[0] = out[1] = out[2] = out[3] = 0;
  if (!h->sp_net->eo_stats) return D2FE_OK;
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  HIP_TRY(hipDeviceSynchronize());      // the handle's streams and those of every lane that counts into the same buffer
  unsigned long long v[4];
  HIP_TRY(hipMemcpy(v, h->sp_net->eo_stats, sizeof(v), hipMemcpyDeviceToHost));
  for (int i = 0; i < 4; ++i) out[i] = (int64_t)v[i];
  return D2FE_OK;
}

int d2fe_sync(d2fe_handle h) {
  if (h && h->tail_stream) (void)hipStreamSynchronize(h->tail_stream);
  if (!h) return fail(D2FE_ERR_INVALID, "null handle");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return D2FE_OK;
}

}  // extern "C"
