// context.h -- the device context behind d2fe_handle and the launch sequences shared by the translation units that implement
// include/d2fe.h (api.hip: handle lifecycle and the extract entry points; superpoint_host.hip: SuperPoint's host side; netvlad_host.hip: NetVLAD's host side; match_host.hip: the
// matcher's; next_host.hip: the "next rows"; debug_hooks.hip: the development library's hooks on injected tensors; lk.hip, lk_carry.hip, lk_flow.hip: the trackers;
// pipe.hip, quad_pipe.hip: the frames-in-flight pipelines; exchange.hip, quad_exchange.hip, loop.hip, window.hip: the consumers behind them).  Internal.
#pragma once
#include <hip/hip_runtime.h>

#include <array>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/d2fe.h"
#include "handle_life.h"
#include "kernels.h"
#include "sp_plan.h"

namespace d2fe {
int ctx_fail(int code, const std::string& msg);
}

#define HIP_TRY(expr)                                                                                       \
  do {                                                                                                      \
    hipError_t e_ = (expr);                                                                                 \
    if (e_ != hipSuccess)                                                                                   \
      return d2fe::ctx_fail(D2FE_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_) + " @" + __FILE__ + ":" + \
                                              std::to_string(__LINE__));                                    \
  } while (0)

namespace d2fe {

struct Layer {
  void* wpack = nullptr;
  float* bias = nullptr;
  int cout = 0, cout_pad = 0, cin = 0, ks = 0;
  // D2FE_PREC_I8: s_w[c] of the int8 pack (host, from the load); d_c = s_x * s_w[c] on the device and r of the input tensor, both from d2fe_set_superpoint_int8_ranges
  std::vector<float> s_w;
  float* dscale = nullptr;
  float qr = 0.f;
};

// The one owner of a set of device buffers: hands out a pointer, remembers it and frees everything when it goes (SpNet, SpRun; a debug hook's buffers, whichever
// way the hook returns)
struct DevPool {
  std::vector<void*> owned;
  DevPool() = default; DevPool(const DevPool&) = delete; DevPool& operator=(const DevPool&) = delete;
  ~DevPool() { clear(); }
  void clear() { for (void* p : owned) (void)hipFree(p); owned.clear(); }
  // one pointer back early (a re-upload replaces it); nullptr: nothing
  void give_back(void* p) {
    for (size_t i = 0; p && i < owned.size(); ++i) if (owned[i] == p) { (void)hipFree(p); owned.erase(owned.begin() + i); return; }
  }
  template <class T>
  hipError_t alloc(T** out, size_t bytes) {
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, bytes ? bytes : 4);
    if (e == hipSuccess) owned.push_back(p);
    *out = static_cast<T*>(p);
    return e;
  }
  // bytes of device memory, filled with `fill` bytes (outputs: 0xff, so that an entry a kernel does not write is no plausible value) or with src
  template <class T>
  hipError_t get(T** out, size_t bytes, const void* src, int fill = 0xff) {
    const hipError_t e = alloc(out, bytes);
    if (e != hipSuccess || !bytes) return e;
    return src ? hipMemcpy(*out, src, bytes, hipMemcpyHostToDevice) : hipMemset(*out, fill, bytes);
  }
};

// ---- SuperPoint (superpoint_host.hip; the network itself is sp_plan.h) ----
// what d2fe_load_superpoint / d2fe_set_superpoint_pca build: a parent handle shares it with its pipeline lanes, and both calls change it in place (they refuse
// while pipes are alive); owns its device memory
struct SpNet {
  bool sp_loaded = false;
  bool i8_ranges = false;      // D2FE_PREC_I8: d2fe_set_superpoint_int8_ranges has run since the last load
  float* w1a = nullptr;  // [9][64]
  float* b1a = nullptr;
  Layer L[L_COUNT];
  float* pca_comp_t = nullptr; float* pca_mean = nullptr; int pca_dims = 0;
  unsigned long long* eo_stats = nullptr;      // exact_order: [4] marked candidates, cells re-evaluated, cells dropped, calls -- one set per parent handle
  DevPool pool;      // (makes the net non-copyable; its destructor frees the device memory)
};
// what one context owns to run the network: SpRun::pool holds every pointer below
struct SpBufs {
  bool fuse1a = true;      // conv1a fused into conv1b's staging (D2FE_FUSE1A=0 keeps the stand-alone conv1a kernel)
  bool wino_dynamic = true;    // D2FE_WINO_DYNAMIC=0: static round-robin split of the work items
  // activations (NHWC fp32), a buffer per layer so that d2fe_debug_read can inspect any of them: act[plan layer] for conv1a (the stand-alone conv1a kernel and
  // debug reads only) .. conv4b; act[SP_PA]: the heads' convPa | convDa buffer
  float* act[SP_PA + 1] = {};
  float *logits = nullptr, *draw = nullptr, *semi = nullptr;
  // async_tail: the post-processing (softmax .. descriptors) of call k runs on tail_stream under the convolutions of call k+1,
  // so the three tensors the tail reads exist twice (buffer set = call parity) and events order trunk / tail / reuse
  float *a4b2 = nullptr, *logits2 = nullptr, *draw2 = nullptr;
  unsigned long long* cand = nullptr;
  long cand_cap = 0;
  int* work_ctrs = nullptr;    // one work-item counter per Winograd layer, zeroed at the start of every network pass (ConvArgs::work_ctr)
  int* cand_count = nullptr;   // work_ctrs + 64: ONE memset clears both
  float* zeros = nullptr;      // 1 KiB of zeros (ConvArgs::zeros)
  // sparse descriptor head (variant B unless cfg.dense_descriptors): cell flags, cell -> slot map, slot -> cell list, counts, descriptors
  bool sparse_desc = false; int sp_slots = 0; int sp_min_batch = 4;
  uint8_t* sp_flags = nullptr; int32_t* sp_slotmap = nullptr; int32_t* sp_cells = nullptr; int32_t* sp_count = nullptr; float* sp_desc = nullptr;
  float* sp_mid = nullptr; int sp_mid_imgs = 0;      // ReLU(convDa) at the selected cells between the two stages of the split sparse head (passes of <= 4 images)
  float* aconf = nullptr; int* clist = nullptr; int* a_ncand = nullptr;     // variant A scratch
  float* a_samp = nullptr; float* a_cn = nullptr; int a_scap = 0;   // variant A sampling: [batch][a_scap][256] samples, [batch][256] channel norms
  // exact_order (exact_order.hip; cfg.exact_order): eo_slots crops of 88x88 per call through the direct kernels
  int eo_slots = 0; float eo_eps = 0.f;
  uint8_t* eo_crops = nullptr; int* eo_cell_map = nullptr; int* eo_cell_list = nullptr; int* eo_cell_count = nullptr;
  float* eo_act = nullptr;           // the crop batch's activations, laid out by sp_crop_layout
};
struct SpRun : SpBufs {
  DevPool pool;
  int alloc(const d2fe_config& cfg);
  void release() { pool.clear(); static_cast<SpBufs&>(*this) = SpBufs(); }
};      // (non-copyable through `pool`, whose destructor releases)

// ---- NetVLAD (netvlad_host.hip) ----
// One launch form of the execution plan over the flat layer list: fused MobileNetV2 blocks (netvlad_fused.hip, netvlad_pair.hip) where the pattern
// matches, single layers otherwise.  Only the LAST layer of a step is materialised in HBM (NvRun::out); everything inside a fused block lives in LDS
enum class NvKind : int {
  Conv0, Dw, Pw,              // one layer through the generic launchers (launch_nv_conv0 / launch_nv_dw / launch_nv_pw)
  Front, Expand, Block,       // nv_block_kernel: conv0 -> dw -> pw (mode 1), pw -> dw -> pw (mode 0 with its expand stage), dw -> pw (mode 0)
  XBlock, PBlock, FPair,      // pw -> dw -> pw: nv_xblock_kernel (input in registers), nv_pblock_kernel (pixel pairs; one launch per output-channel half);
                              // conv0 -> dw -> pw: nv_fpair_kernel (pixel pairs)
  Tail, TailBlock,            // the trunk's last pw + the NetVLAD pre-projection: nv_tail_kernel, nv_block_kernel mode 2
};
inline bool nv_fused(NvKind k) { return k != NvKind::Conv0 && k != NvKind::Dw && k != NvKind::Pw; }
inline bool nv_is_tail(NvKind k) { return k == NvKind::Tail || k == NvKind::TailBlock; }

struct NvLayer {
  int kind, cin, cout, cout_pad, stride, act, res; int oh = 0, ow = 0;   // oh, ow: at the handle's maximum image size
  int gmax = 1;                      // slabs the output has room for (a fused block may split its hidden channels over workgroup groups)
  bool materialised = false;         // the last layer of a step: its output exists in HBM
  float* w = nullptr; float* b = nullptr;      // packed weights of a layer that runs as a single step
};
struct NvStep {
  NvKind kind = NvKind::Pw; int l0 = 0, l1 = 0;
  int halves = 1;                    // PBlock: launches over output-channel halves (more than 128 output channels: 2)
  bool one_slab_out = false;         // the consumer reads ONE plain tensor (a single step, or a kernel that reads one input slab): partial slabs are summed here
  float* w0 = nullptr; float* we = nullptr; float* wp = nullptr; float* bp = nullptr;   // packed first-conv / expand / depthwise + project records and bias
  float* wp2 = nullptr; float* bp2 = nullptr;                                            // PBlock in two halves: the second half's project record and bias
};
// schedule knobs, read when constructed: the D2FE_NV_* switches of the development library (A/B measurements, tools/README.md); the product library's
// d2fe_dev_env returns the defaults, the measured best
struct NvKnobs {
  static int positive(int v, int dflt) { return v > 0 ? v : dflt; }
  bool legacy = d2fe_dev_env("D2FE_NV_LEGACY", 0) != 0;     // one launch per layer
  bool pair = d2fe_dev_env("D2FE_NV_PAIR", 1) != 0, xblock = d2fe_dev_env("D2FE_NV_XBLOCK", 1) != 0;     // the pixel-pair kernels, nv_xblock_kernel
  int blocks_target = positive(d2fe_dev_env("D2FE_NV_BLOCKS", 0), 512);     // workgroups per IMAGE the hidden-channel split of a block aims at
  int tail_blocks = positive(d2fe_dev_env("D2FE_NV_TAIL_BLOCKS", 0), 30);   // the same for the tail (3 pixel tiles x 10 groups at 15 x 20)
  int slabsum = d2fe_dev_env("D2FE_NV_SLABSUM", 3);        // partial slabs from which they are summed once instead of by every consumer (0 = never)
  bool group_rule = d2fe_dev_env("D2FE_NV_GROUP_RULE", 1) != 0;   // nv_groups() stops splitting where the slab-sum launch costs more than the chunks it saves
  bool merge = d2fe_dev_env("D2FE_NV_MERGE", 1) != 0;     // a batch lets one workgroup walk a run of hidden-channel groups (NvBlockArgs::gmerge): same bits
  int front_tpw = d2fe_dev_env("D2FE_NV_FRONT_TPW", 0), nbuf = d2fe_dev_env("D2FE_NV_NBUF", 0);      // 0: the launchers decide
  int stamp_step = d2fe_dev_env("D2FE_NV_STAMP_STEP", -1);     // the plan step whose kernel writes phase stamps (diagnostics)
};
// what d2fe_load_netvlad builds: read-only while pipeline lanes share it (d2fe_load_netvlad / d2fe_set_netvlad_pca refuse while pipes are alive); owns its device memory
struct NvNet {
  std::vector<NvLayer> layers;
  std::vector<NvStep> plan;
  int feat = 0, proj = 0, k = 0, feat_gmax = 1;       // feat_gmax: slabs of the pre-projected features (input of the VLAD stage)
  float *pre_w = nullptr, *pre_b = nullptr, *aw = nullptr, *aw_pack = nullptr, *ab = nullptr, *cen = nullptr;
  float *pca_comp = nullptr, *pca_mean = nullptr; int pca_m = 0;
  NvKnobs knobs;
  NvNet() = default; NvNet(const NvNet&) = delete; NvNet& operator=(const NvNet&) = delete; ~NvNet();
};
// a tensor of the last call = the sum of `n` partial slabs `stride` floats apart
struct NvSlabs { int n = 1; long stride = 0; int groups = 1; };     // groups: the hidden-channel groups that wrote it (n = 1 again once the slab sum ran)
// the host-side bookkeeping a NetVLAD call leaves behind (what the next step of the call and the debug reads consult)
struct NvLast { std::vector<NvSlabs> layer; NvSlabs feat; int stamp_wgs = 0; };
// what one context owns to run the network: its activations and the bookkeeping of its last call
struct NvRun {
  std::vector<float*> out;           // [layer]: output of a materialised layer (nullptr: the layer lives inside a fused block)
  float *feat_buf = nullptr, *raw = nullptr, *part = nullptr;
  unsigned long long* stamps = nullptr;     // D2FE_NV_STAMP_STEP: [32768][32] phase stamps (the loading handle only)
  NvLast last;
  int alloc(const NvNet& net, int max_batch);
  void release();
  NvRun() = default; NvRun(const NvRun&) = delete; NvRun& operator=(const NvRun&) = delete; ~NvRun() { release(); }
};

// ---- the matcher's host side (match_host.hip) ----
struct MatchHost {
  // host-pointer matcher: pool of (stream, scratch) slots so that concurrent callers (the reference calls matchKNN from three
  // threads) neither share state nor pay hipStreamCreate / hipMalloc / hipFree (a device-wide sync) per call
  struct Slot {
    hipStream_t stream = nullptr; char* buf = nullptr; char* pin = nullptr; size_t bytes = 0; bool busy = false;
    int grow(size_t want, bool pinned);      // by the call that holds the slot, OUTSIDE the lock (hipFree / hipHostFree synchronise the device)
  };
  // one call's hold on a slot: a free one or a new one (with its stream) under the lock, given back on scope exit.  slot == nullptr: no stream could be created
  struct Lease {
    MatchHost& m; Slot* slot = nullptr;
    explicit Lease(MatchHost& m_);
    ~Lease() { if (slot) { std::lock_guard<std::mutex> lk(m.mu); slot->busy = false; } }
  };
  // device-API matcher scratch (cand4), one per caller stream: calls on different streams may overlap on the GPU
  struct Scratch { hipStream_t stream = nullptr; int32_t* cand4 = nullptr; size_t bytes = 0; int npairs = 0; };
  std::deque<Slot> slots;          // deque: growing it never relocates the slots other threads are using
  std::deque<Scratch> scratch;
  std::mutex mu;
  int32_t* stats = nullptr;        // [4] matcher counters: [0] queries that took the exact fallback scan (MatchArgs::stats)
  unsigned long long* stamps = nullptr;   // development builds: [4096][16] phase stamps of the last d2fe_match_batch_device launch
  void release();                  // drains and destroys the slot streams, frees every buffer
  ~MatchHost() { release(); }
};

// ---- what only a handle of d2fe_create has (a pipe lane is driven through run_superpoint / run_netvlad on device buffers of the pipe) ----
// staging of the host-pointer extract and NetVLAD calls: the frame upload buffers and output blocks on the device (pool), their pinned mirrors (one DMA in, one
// DMA out per call), and d2fe_extract_all*'s second stream.  The reference calls infer / inference with ONE image at 15-30 Hz (loop_cam.cpp:609-616): at that
// batch the per-copy latency of pageable D2H copies is a sizeable part of a call
struct HostStage {
  DevPool pool;
  uint8_t* s_img = nullptr;
  float* s_out = nullptr;      // [kps | scores | desc | n | idx] of a host-pointer extract call, contiguous -> ONE D2H of the first four
  size_t s_out_bytes = 0;
  uint8_t* nv_s_img = nullptr; float* nv_s_out = nullptr;      // d2fe_netvlad(_batch): from d2fe_load_netvlad on
  uint8_t* pin_in = nullptr; size_t pin_in_bytes = 0;
  float* pin_out = nullptr; size_t pin_out_bytes = 0;
  float* pin_nv = nullptr; size_t pin_nv_bytes = 0;
  // d2fe_extract_all*: NetVLAD of the same uploaded frame(s) on a second stream, beside SuperPoint
  hipStream_t nv_stream = nullptr; hipEvent_t ev_up = nullptr;
  // *p becomes a device buffer of `bytes` (the old one is freed first)
  template <class T>
  hipError_t dev(T** p, size_t bytes) { pool.give_back(*p); *p = nullptr; return pool.alloc(p, bytes); }
  // *p becomes a pinned buffer of `bytes`, *have its size.  Not fatal: false leaves nullptr and 0, and the pageable path serves the call
  template <class T>
  bool pinned(T** p, size_t* have, size_t bytes) {
    if (*p) (void)hipHostFree(*p);
    *p = nullptr; *have = 0;
    if (hipHostMalloc(p, bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); *p = nullptr; return false; }
    *have = bytes;
    return true;
  }
  ~HostStage() {      // (the device buffers go with `pool`)
    if (nv_stream) { (void)hipStreamSynchronize(nv_stream); (void)hipStreamDestroy(nv_stream); }
    if (ev_up) (void)hipEventDestroy(ev_up);
    for (void* p : {(void*)pin_in, (void*)pin_out, (void*)pin_nv}) if (p) (void)hipHostFree(p);
  }
};

// grow-only device scratch of the LK / detector and "next rows" host-pointer entry points (ctx_scratch)
struct GrowScratch {
  void* p = nullptr; size_t bytes = 0;
  void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
  ~GrowScratch() { release(); }
};

}  // namespace d2fe

struct d2fe_context {
  d2fe_config cfg;
  hipStream_t stream = nullptr;
  d2fe::HandleLife life;       // pipes created from this handle and not destroyed yet: their lanes read THIS handle's packed weights, so d2fe_load_* and
                               // d2fe_set_*_pca refuse (D2FE_ERR_INVALID) while there are any, and d2fe_destroy is deferred to the last of them
  // SuperPoint: the network (shared with the pipeline lanes) and this context's buffers
  std::shared_ptr<d2fe::SpNet> sp_net;
  d2fe::SpRun sp_run;
  // async_tail: the handle's second stream and the events that order trunk / tail / buffer reuse (SpBufs)
  hipStream_t tail_stream = nullptr;
  hipEvent_t ev_trunk[2] = {nullptr, nullptr}, ev_tail[2] = {nullptr, nullptr};
  int parity = 0, last_set = 0;
  std::unique_ptr<d2fe::HostStage> stage;      // staging for the host-pointer API (null on a lane)
  // last call geometry (for debug reads)
  int last_w = 0, last_h = 0, last_n = 0;
  const uint8_t* last_gray = nullptr; int last_stride = 0; size_t last_istride = 0;
  // host-pointer calls: cached hipGraphs of the launch sequences (at one image per call the ~10 us the command processor spends between two dependent
  // launches are a sizeable part of a call) and pinned staging
  bool use_graphs = true, use_pinned = true;       // D2FE_GRAPH=0 / D2FE_PINNED=0 switch them off (A/B measurements)
  // host-side bookkeeping a launch sequence leaves behind (what the debug reads and the next NetVLAD step consult): saved when a sequence is
  // captured, restored on every replay, so that a replay leaves the handle exactly as a direct run of the same geometry would
  struct HostState { int last_w = 0, last_h = 0, last_n = 0, last_set = 0; const uint8_t* last_gray = nullptr; int last_stride = 0; size_t last_istride = 0;
                     d2fe::NvLast nv; };
  struct GraphEntry { hipGraphExec_t exec = nullptr; int seen = 0; bool bad = false; HostState st; };
  std::map<std::array<long, 6>, GraphEntry> graphs;
  int ncu = 256;               // compute units this context sizes its persistent grids for: the device's (d2fe_create) or a pipeline lane's share
  int ncu_dev = 256;           // compute units of cfg.device_id: decisions that fix an arithmetic order use this one
  d2fe::MatchHost match;
  d2fe::GrowScratch scratch;
  // NetVLAD: the network (shared with the pipeline lanes) and this context's buffers
  std::shared_ptr<d2fe::NvNet> nv_net;
  d2fe::NvRun nv_run;
  // profiling (HIP events on the launch stream)
  int prof_mode = 0;
  std::vector<hipEvent_t> prof_pool;
  size_t prof_used = 0;
  struct ProfRec { int stage; hipEvent_t a, b; };
  std::vector<ProfRec> prof_recs;
};


namespace d2fe {
// launch sequences (superpoint_host.hip, netvlad_host.hip).  run_superpoint == one TensorRT executeV2 + processOutput of the reference; run_netvlad == one
// MobileNetVLADONNX::inference.  Both only enqueue work on the given stream(s)
int run_superpoint(d2fe_context* h, const uint8_t* d_gray, int n, int W, int H, int stride, size_t image_stride, float* d_kps, float* d_scores,
                   float* d_desc, int32_t* d_idx, int cap, int32_t* d_n, hipStream_t s, hipStream_t s_tail = nullptr, int bs = 0);
// the network alone on a D2FE_PREC_F32 handle with the dense head (the calibration session, calib.hip): conv1b .. conv4b, convPa | convDa, convPb, convDb into the
// handle's buffers -- the launches run_superpoint makes there -- and no tail.  Leaves the geometry for the debug reads as a call does
int run_superpoint_trunk(d2fe_context* h, const uint8_t* d_gray, int n, int W, int H, int stride, size_t image_stride, hipStream_t s);
int run_netvlad(d2fe_context* h, const uint8_t* d_gray, int n, int W, int H, int stride, size_t image_stride, float* d_out, hipStream_t s);
int check_geometry(d2fe_context* h, int n, int W, int H, int stride, int cap);
// why the handle's SuperPoint cannot run yet (weights not loaded; D2FE_PREC_I8: calibration ranges not set), nullptr when it can: D2FE_ERR_NOT_READY of every
// extract call and pipe create
const char* sp_not_ready(const d2fe_context* h);
int desc_dim_of(const d2fe_context* h);      // floats per descriptor row: 256, or pca_dims where a PCA is set (d2fe_desc_dim)
int nv_check(d2fe_context* h, int n, int W, int H, int stride);
// a second context on the same device that SHARES the parent's networks (SpNet, NvNet: packed weights, PCA matrices) and owns its own
// activations, scratch, counters and streams: one lane of the frames-in-flight pipeline.  The parent must not reload weights while lanes exist
// `stream` (optional): the lane's launch stream, e.g. one created with a CU mask (the lane then owns it); `ncu` (optional): the compute units that
// stream may use -- the persistent kernels size their grids on it
// with_netvlad: the lane will run NetVLAD itself (its own activation buffers); a lane never gets the host-pointer staging of d2fe_create
int clone_lane(d2fe_context* parent, int max_batch, d2fe_context** out, hipStream_t stream = nullptr, int ncu = 0, bool with_netvlad = true);
// a new non-blocking stream that does NOT take turns with `beside` on the device (pipe.hip: the same measurement as d2fe_pipe_create's stream placement, on up to four
// candidates; the first candidate if none can be told apart).  hipSuccess or the failing call's error
hipError_t create_stream_beside(int device_id, hipStream_t beside, hipStream_t* out);
// n_first + n_second non-blocking streams placed by measurement (pipe.hip): a lane's own and second stream on different hardware pipes, consecutive lanes' streams
// on different ones too -- the lanes of d2fe_pipe_create and d2fe_quad_pipe_create.  first_class / second_class / n_classes: what was measured (-1 / 0: nothing)
int place_streams(int device_id, int n_first, int n_second, std::vector<hipStream_t>& first, std::vector<hipStream_t>& second, std::vector<int>& first_class,
                  std::vector<int>& second_class, int* n_classes, long long* probe_ticks, double* probe_turns_us);
// helpers of the entry points (api.hip) that the other host units share
int fail(int code, const std::string& msg);      // records d2fe_last_error(), returns `code`
int upload(const void* src, size_t bytes, void** dst);
int ctx_scratch(d2fe_handle h, size_t bytes, void** out);      // at least `bytes` of the handle's grow-only device scratch (GrowScratch)
// host image(s) -> the handle's device staging, tight rows: through the pinned staging buffer (CPU row copy + ONE DMA) or, when that
// is off, with pageable 2D copies
int upload_frames(d2fe_context* h, uint8_t* d_dst, const uint8_t* gray, int n, int width, int height, int stride, size_t image_stride, hipStream_t s);
// weights / PCA matrices were (re)loaded: the captured launch sequences hold the old device pointers
void graphs_clear(d2fe_context* h);
void host_state_save(const d2fe_context* h, d2fe_context::HostState& st);
void host_state_restore(d2fe_context* h, const d2fe_context::HostState& st, bool netvlad);

// lk_carry.hip, for the pipe's sp_lk mode: what d2fe_lk_carry_step_device would refuse (nullptr: nothing), and trackLK(left, right) over the lists of a pass --
// n_frames list blocks, consecutive in d_lists, against the pass's stereo workspace (d2fe_lk_track_stereo_device), ONE launch
const char* lk_carry_check_params(const d2fe_track_params* tp);
// the capacity of a flow list: detectPoints fills it up to total_feature_num, and a list block holds at least one slot
inline int flow_cap_tracks(const d2fe_track_params& tp) { return tp.total_feature_num > 1 ? tp.total_feature_num : 1; }
// (desc_dim = 0: flow lists, cap_tracks = flow_cap_tracks)
int lk_carry_right_launch(d2fe_context* h, const uint8_t* ws, int n_frames, int width, int height, const d2fe_track_params& tp, const float* d_lists, int desc_dim,
                          float* d_right_xy, uint8_t* d_right_status, hipStream_t s);

// lk_flow.hip, for the pipe's flow mode: what d2fe_lk_flow_step_device would refuse for these parameters and this geometry, as a message (nullptr: nothing)
const char* lk_flow_check_params(const d2fe_flow_params* fp, int width, int height);

// lk.hip, for the mono pipe's sp_lk mode: the pyramids of n_frames images alone (no right images), image f's at f * (half of d2fe_lk_stereo_workspace_bytes(1, ..))
int lk_pyramids_launch(d2fe_context* h, const uint8_t* d_img, int n_frames, int width, int height, int stride, size_t image_stride, int levels, void* d_workspace,
                       hipStream_t s);

// depth.hip: depth_gather_kernel over up to two segments of point lists (the pipe: the pass's keypoint rows and, with sp_lk, its landmark lists) in ONE launch.
// List l of a segment reads depth image l, its points at pts + l * pts_stride floats, its count at n[l * n_stride], and writes out[l * cap .. + cap)
struct DepthSeg { const float* pts; size_t pts_stride; const int32_t* n; size_t n_stride; int cap; uint16_t* out; };
int depth_gather_launch(d2fe_context* h, const uint16_t* d_depth, int W, int H, size_t depth_stride_px, size_t depth_image_stride_px, int n_lists, const DepthSeg* segs,
                        int n_segs, hipStream_t s);

// bearings.hip: bearings_kernel over up to three segments of point lists in ONE launch (the stereo pipe: the pass's left keypoint rows, its right keypoint rows, its
// landmark lists; the quad pipe: the keypoint rows, the four lists of every quad frame, its four neighbour pairs).  List l of a segment reads its points at
// pts + s * pts_stride floats and its count at n[s * n_stride], s = l, or with by4 the list (l & ~3) + src[l & 3] (a neighbour pair reads the list of its camera a).
// It lifts them with camera cam[j] of BearCams, j = 0, or l & 3 with by4, and writes bearing[(l * bearing_step) * cap * 3 ..) (bearing may be null when pred is
// not).  pred != null: the prediction through extrinsic ext[j], dense [list][cap][2].  pred_ok != null (needs pred): the gate against other[l * other_stride ..) /
// status[l * status_stride ..), other_bearing (lifted with camera ocam[j]) and pred_ok dense.  Slots >= n are written as zero everywhere
struct BearCam { int kind, distort; double p[9]; double iK11, iK13, iK22, iK23; };
struct BearCams { BearCam cam[4]; double T[4][12]; double distance, radius; };
struct BearSeg {
  const float* pts; size_t pts_stride; const int32_t* n; size_t n_stride; int cap, by4;
  unsigned char cam[4], ocam[4], ext[4], src[4];
  double* bearing; size_t bearing_step; float* pred;
  const float* other; size_t other_stride; const uint8_t* status; size_t status_stride; double* other_bearing; uint8_t* pred_ok;
};
const char* bearings_check_camera(const d2fe_camera* c);      // what d2fe_bearings_device refuses in a camera, as a message (nullptr: nothing)
BearCam bearings_make_camera(const d2fe_camera& c);
int bearings_launch(d2fe_context* h, const BearCams& cams, int n_lists, const BearSeg* segs, int n_segs, hipStream_t s);

struct ProfScope {
  d2fe_context* h; int stage; hipStream_t s; hipEvent_t a = nullptr, b = nullptr; bool on = false;
  ProfScope(d2fe_context* h_, int stage_, hipStream_t s_, bool want = true) : h(h_), stage(stage_), s(s_) {      // want = false: a scope that records nothing
    on = want && (h->prof_mode == 2 || (h->prof_mode == 1 && (stage == D2FE_PROF_CONV1B || stage == D2FE_PROF_NETVLAD)));
    if (!on) return;
    if (h->prof_used + 2 > h->prof_pool.size()) {
      for (int i = 0; i < 64; ++i) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) { on = false; return; } h->prof_pool.push_back(e); }
    }
    a = h->prof_pool[h->prof_used++]; b = h->prof_pool[h->prof_used++];
    (void)hipEventRecord(a, s);
  }
  ~ProfScope() {
    if (!on) return;
    (void)hipEventRecord(b, s);
    h->prof_recs.push_back({stage, a, b});
  }
};

// Runs `fn(s)` -- a launch sequence on `s` whose arguments are a pure function of `key` (handle-owned buffers only) -- directly the
// first time a key is seen (module loads, function attributes, lazy allocations happen there), captures it into a hipGraph the second
// time and replays the instantiated graph from then on.  Anything that cannot be captured marks the key bad and runs directly.
template <class F>
int run_cached(d2fe_context* h, const std::array<long, 6>& key, hipStream_t s, F&& fn) {
  if (!h->use_graphs || h->prof_mode != 0) return fn(s);
  auto& e = h->graphs[key];
  if (e.bad) return fn(s);
  const bool netvlad = key[0] != 1;       // key[0]: 1 = the SuperPoint sequence, 2 / 3 = NetVLAD (own frames / the frames SuperPoint reads)
  if (e.exec) { HIP_TRY(hipGraphLaunch(e.exec, s)); host_state_restore(h, e.st, netvlad); return D2FE_OK; }
  if (e.seen++ < 1) return fn(s);
  if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) != hipSuccess) { (void)hipGetLastError(); e.bad = true; return fn(s); }
  const int rc = fn(s);
  hipGraph_t g = nullptr;
  const hipError_t er = hipStreamEndCapture(s, &g);
  if (rc != D2FE_OK || er != hipSuccess || !g) {
    if (g) (void)hipGraphDestroy(g);
    (void)hipGetLastError();
    e.bad = true;
    return rc != D2FE_OK ? rc : fn(s);
  }
  hipGraphExec_t ex = nullptr;
  const hipError_t ei = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  if (ei != hipSuccess || !ex) { (void)hipGetLastError(); e.bad = true; return fn(s); }
  e.exec = ex;
  host_state_save(h, e.st);               // fn(s) ran its host code during the capture: this is the state a direct run leaves
  HIP_TRY(hipGraphLaunch(e.exec, s));
  return D2FE_OK;
}
}  // namespace d2fe
