// api.hip -- C ABI (include/d2fe.h) of libd2fe_hip.so: the handle.  d2fe_last_error and the ctx_* accessors, the config defaults, create / destroy / clone_lane,
// the host and device extract entry points with their frame upload, the cached launch sequences' bookkeeping (graphs_clear, host_state_*), profiling and
// d2fe_sync.  Host code only: SuperPoint's host side is superpoint_host.hip, NetVLAD's netvlad_host.hip, the matcher's match_host.hip, the "next rows" are
// next_host.hip, the development library's hooks debug_hooks.hip; the kernels live in the other translation units (kernels.h lists their launchers).
// There is deliberately NO CPU fallback in this library.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "context.h"

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
  GrowScratch& sc = h->scratch;
  if (bytes > sc.bytes) {
    if (sc.p) { hipStreamSynchronize(h->stream); sc.release(); }
    const size_t want = bytes + bytes / 2 + 4096;
    if (hipMalloc(&sc.p, want) != hipSuccess) return fail(D2FE_ERR_HIP, "hipMalloc scratch");
    sc.bytes = want;
  }
  *out = sc.p;
  return D2FE_OK;
}
int upload(const void* src, size_t bytes, void** dst) {
  HIP_TRY(hipMalloc(dst, bytes));
  HIP_TRY(hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
  return D2FE_OK;
}

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
  if (cfg->precision != D2FE_PREC_F32 && cfg->precision != D2FE_PREC_F16X2 && cfg->precision != D2FE_PREC_F32_WINO && cfg->precision != D2FE_PREC_F16 && cfg->precision != D2FE_PREC_I8) return fail(D2FE_ERR_INVALID, "bad precision");
  if (cfg->postproc != D2FE_POSTPROC_B && cfg->postproc != D2FE_POSTPROC_A) return fail(D2FE_ERR_INVALID, "bad postproc");
  if (cfg->variant_b_pca != 0 && cfg->variant_b_pca != 1) return fail(D2FE_ERR_INVALID, "variant_b_pca must be 0 or 1");
  if (cfg->variant_b_pca && cfg->postproc != D2FE_POSTPROC_B) return fail(D2FE_ERR_INVALID, "variant_b_pca is an option of post-processing variant B (variant A applies the PCA without it)");
  if (cfg->exact_order) {
    if (cfg->precision != D2FE_PREC_F32_WINO) return fail(D2FE_ERR_INVALID, "exact_order is an option of D2FE_PREC_F32_WINO (D2FE_PREC_F32 is exact already; D2FE_PREC_F16X2, D2FE_PREC_F16 and D2FE_PREC_I8 are not supported)");
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
    HIP_TRY(hipMalloc(&h->match.stats, 4 * sizeof(int32_t)));
    HIP_TRY(hipMemset(h->match.stats, 0, 4 * sizeof(int32_t)));
    h->use_graphs = d2fe_dev_env("D2FE_GRAPH", 1) != 0;
    if (lane) { h->use_pinned = false; return D2FE_OK; }
    h->stage.reset(new HostStage());
    HostStage& stg = *h->stage;
    const size_t s_cap = h->cfg.max_keypoints > 1024 ? h->cfg.max_keypoints : 1024;      // initial staging capacity per image; grows with the calls (extract_host)
    HIP_TRY(stg.dev(&stg.s_img, H * W * B));
    stg.s_out_bytes = (sizeof(float) * s_cap * 260 + sizeof(int32_t)) * B;
    HIP_TRY(stg.dev(&stg.s_out, stg.s_out_bytes));
    h->use_pinned = d2fe_dev_env("D2FE_PINNED", 1) != 0;
    if (h->use_pinned) {
      const size_t nv_bytes = sizeof(float) * 8192 * (size_t)B;      // NetVLAD descriptors
      if (!stg.pinned(&stg.pin_in, &stg.pin_in_bytes, (size_t)H * W * B) ||
          !stg.pinned(&stg.pin_out, &stg.pin_out_bytes, stg.s_out_bytes < nv_bytes ? nv_bytes : stg.s_out_bytes)) {
        if (stg.pin_in) { (void)hipHostFree(stg.pin_in); stg.pin_in = nullptr; stg.pin_in_bytes = 0; }
        h->use_pinned = false;        // not fatal: the pageable path remains
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
  // wrong order).  Until then the handle must not be used for anything else; d2fe_last_error records what happened.  Mark and count sit under one lock
  // (handle_life.h): a pipe that goes while this call runs either is counted here or sees the mark
  if (!h->life.destroy_requested()) { fail(D2FE_ERR_INVALID, "d2fe_destroy: the handle still has live pipes; it will be released when the last of them is destroyed"); return; }
  hipSetDevice(h->cfg.device_id);
  if (h->stream) hipStreamSynchronize(h->stream);
  if (h->tail_stream) hipStreamSynchronize(h->tail_stream);
  // the owners, users before what they use: the captured sequences (they hold staging and activation pointers), the staging (drains its NetVLAD stream), the
  // matcher (drains its slot streams), the scratch, then the activations and the networks
  graphs_clear(h);
  h->stage.reset();
  h->match.release();
  h->scratch.release();
  h->sp_run.release();
  h->nv_run.release();
  h->sp_net.reset();
  h->nv_net.reset();
  // the streams and events the handle itself created
  if (h->tail_stream) (void)hipStreamDestroy(h->tail_stream);
  for (int i = 0; i < 2; ++i) { if (h->ev_trunk[i]) (void)hipEventDestroy(h->ev_trunk[i]); if (h->ev_tail[i]) (void)hipEventDestroy(h->ev_tail[i]); }
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
  if (h->use_pinned && bytes <= h->stage->pin_in_bytes) {      // (a lane has no staging and use_pinned off)
    uint8_t* const pin_in = h->stage->pin_in;
    HIP_TRY(hipStreamSynchronize(s));            // the previous call's DMA out of pin_in has completed (calls are synchronous: a no-op)
    for (int i = 0; i < n; ++i) {
      const uint8_t* src = gray + i * image_stride;
      uint8_t* dst = pin_in + (size_t)i * width * height;
      if (stride == width) memcpy(dst, src, (size_t)width * height);
      else for (int y = 0; y < height; ++y) memcpy(dst + (size_t)y * width, src + (size_t)y * stride, width);
    }
    HIP_TRY(hipMemcpyAsync(d_dst, pin_in, bytes, hipMemcpyHostToDevice, s));
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
  HostStage& stg = *h->stage;
  // the call's capacity, bounded by what can exist: H*W candidates (keep-all) or the configured maximum
  const long most = h->cfg.max_keypoints > 0 ? h->cfg.max_keypoints : (long)height * width;
  const int dcap = cap < most ? cap : (int)most;
  const size_t D = (size_t)desc_dim_of(h);
  // outputs of the call, contiguous in one device block: kps [n][dcap][2] | scores [n][dcap] | desc [n][dcap][D] | counts [n] | idx [n][dcap]
  const size_t out_bytes = sizeof(float) * (size_t)n * dcap * (3 + D) + sizeof(int32_t) * n;
  const size_t need = out_bytes + sizeof(int32_t) * (size_t)n * dcap;
  if (need > stg.s_out_bytes) {       // grow-only staging: a keep-all call may ask for far more than the initial 1024 per image
    HIP_TRY(hipStreamSynchronize(s));
    graphs_clear(h);                 // captured launch sequences hold the old staging pointers
    stg.s_out_bytes = 0;
    HIP_TRY(stg.dev(&stg.s_out, need));
    stg.s_out_bytes = need;
    if (h->use_pinned && out_bytes > stg.pin_out_bytes) stg.pinned(&stg.pin_out, &stg.pin_out_bytes, out_bytes);     // (the pageable path below serves calls the pinned buffer cannot)
  }
  rc = upload_frames(h, stg.s_img, gray, n, width, height, stride, image_stride, s);
  if (rc) return rc;
  size_t nv_bytes = 0;
  // once NetVLAD work is queued on nv_stream, EVERY exit waits for it: its D2H may target the caller's netvlad_out, and the next call's upload
  // overwrites the frames it reads
  struct NvGuard { HostStage& st; bool armed = false; ~NvGuard() { if (armed && st.nv_stream) (void)hipStreamSynchronize(st.nv_stream); } } nv_guard{stg};
  if (n_netvlad > 0) {
    // NetVLAD reads the frames SuperPoint reads (one upload), on its own stream: at one or two images per call both launch sequences are
    // latency-bound and leave most of the chip idle, so they overlap almost completely (the reference calls infer and then inference
    // for the same image, loop_cam.cpp:609-616)
    // (a stream on another hardware pipe than the handle's own: two busy streams on one pipe take turns, pipe.hip)
    if (!stg.nv_stream) { HIP_TRY(create_stream_beside(h->cfg.device_id, h->stream, &stg.nv_stream)); HIP_TRY(hipEventCreateWithFlags(&stg.ev_up, hipEventDisableTiming)); }
    const int G = d2fe_netvlad_dim(h);
    nv_bytes = sizeof(float) * (size_t)G * n_netvlad;
    if (h->use_pinned && nv_bytes > stg.pin_nv_bytes) {
      const size_t want = sizeof(float) * 8192 * (size_t)h->cfg.max_batch;
      stg.pinned(&stg.pin_nv, &stg.pin_nv_bytes, want > nv_bytes ? want : nv_bytes);
    }
    HIP_TRY(hipEventRecord(stg.ev_up, s));
    HIP_TRY(hipStreamWaitEvent(stg.nv_stream, stg.ev_up, 0));
    nv_guard.armed = true;
    rc = run_cached(h, {3, n_netvlad, width, height, (long)h->nv_net->pca_m, 0}, stg.nv_stream, [&](hipStream_t st) {
      return run_netvlad(h, stg.s_img, n_netvlad, width, height, width, (size_t)width * height, stg.nv_s_out, st);
    });
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(stg.pin_nv ? (void*)stg.pin_nv : (void*)netvlad_out, stg.nv_s_out, nv_bytes, hipMemcpyDeviceToHost, stg.nv_stream));
  }
  // async_tail handles: a preceding d2fe_superpoint_extract_device call may still have its post-processing running on the tail
  // stream against the single-buffered scratch (candidates, score map, sparse-head slots) that this run uses too
  if (h->cfg.async_tail)
    for (int i = 0; i < 2; ++i) HIP_TRY(hipStreamWaitEvent(s, h->ev_tail[i], 0));
  float* o_kps = stg.s_out;
  float* o_sc = o_kps + (size_t)n * dcap * 2;
  float* o_desc = o_sc + (size_t)n * dcap;
  int32_t* o_n = reinterpret_cast<int32_t*>(o_desc + (size_t)n * dcap * D);
  int32_t* o_idx = o_n + n;
  rc = run_cached(h, {1, n, width, height, dcap, (long)D}, s, [&](hipStream_t st) {
    return run_superpoint(h, stg.s_img, n, width, height, width, (size_t)width * height, o_kps, o_sc, o_desc, o_idx, dcap, o_n, st);
  });
  if (rc) return rc;
  std::vector<int32_t> ncand(h->cfg.max_keypoints < 0 ? n : 0);
  if (!ncand.empty()) HIP_TRY(hipMemcpyAsync(ncand.data(), h->sp_run.cand_count, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s));
  if (h->use_pinned && stg.pin_out && out_bytes <= stg.pin_out_bytes) {
    // ONE D2H of the whole block into pinned memory, one synchronisation, then the rows that exist go to the caller's arrays
    HIP_TRY(hipMemcpyAsync(stg.pin_out, stg.s_out, out_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const float* p_kps = stg.pin_out;
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
    HIP_TRY(hipStreamSynchronize(stg.nv_stream));
    nv_guard.armed = false;
    if (stg.pin_nv) memcpy(netvlad_out, stg.pin_nv, nv_bytes);
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
