// window.hip -- d2fe_window_*: remote tracking against the tracker's keyframe window, behind a stereo pipe or a quad pipe, inside the library.
// Replaces what D2FeatureTracker::trackRemoteFrames (d2frontend/src/d2featuretracker.cpp:237-310) does with a remote frame: the walk through current_keyframes of
// getMatchedPrevKeyframe (:166-235: newest keyframe first, for a quadcam agent the keyframe's views in the order dirs = {2, 3, 0, 1}, stop at the first NetVLAD similarity
// that is not below track_remote_netvlad_thres) and trackRemote's matchLocalFeatures(prev_frame, frame) -> matchKNN (:312-387: one pair for stereo, the four rotated view
// pairs of :270-291 for quadcam), for a batch of remote frames by ONE sequence:
//
//   ONE window_gate_kernel launch (every similarity, the selection, the per-frame records, the matcher's problem table)
//   -> ONE matcher launch (a side: the chosen keyframe's descriptors in place in the store; b side: the remote descriptors in place where the caller left them)
//   -> ONE D2H into a pinned slot
//
// on ONE stream of the object's own and without a host synchronisation.  The window's CONTENTS live on the device: `capacity` slots of NetVLAD [V][G], descriptors
// [V][cap][D] and counts [V].  Its ORDER (oldest -> newest, the order of current_keyframes), the tags and the free slots are host bookkeeping: processFrame's emplace_back
// (:837) is d2fe_window_push (one copy launch, device to device), updatebySldWin's erase loop (:47-57) is d2fe_window_retain (no launch at all).  The order reaches the gate
// kernel BY VALUE (WinOrder, a kernel argument as loop.hip's LoopFlags): nothing is uploaded, and a query queued earlier keeps the order it was queued with.
//
// Selection.  The reference returns at the FIRST pass of its walk, so with the window positions pos = 0 (oldest) .. n - 1 and j the place in `dirs`, the chosen pair is the
// minimum of (n - 1 - pos) * V + j over the passing pairs -- not the best similarity: an older keyframe that resembles the remote frame more loses to a newer one that
// merely passes.  The similarity arithmetic is gate_pairs_kernel's / quad_gate_kernel's (swarm.hip), operation by operation.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "consumer.h"

using namespace d2fe;

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int WIN_MAXKF = 64;                  // slots of a window
constexpr int WIN_MAXNQ = 256;                 // remote frames of one query

__device__ __forceinline__ f32x4 win_ld4(const float* p, bool vec) {      // swarm.hip's ld4: a gathered block's NetVLAD field is 16-byte aligned only when cap % 4 == 0
  if (vec) return *reinterpret_cast<const f32x4*>(p);
  return f32x4{p[0], p[1], p[2], p[3]};
}

struct WinOrder { int32_t n, pad; int64_t tag[WIN_MAXKF]; uint8_t slot[WIN_MAXKF]; };      // window position (oldest = 0) -> tag, slot (kernel argument: no upload)

struct WinArgs {
  // the store
  const float* store_nv; const float* store_desc; const int32_t* store_nkp;
  // the remote frames: row q * V + v of every array, rows `*_stride` 32-bit words apart
  const float* q_nv; const float* q_desc; const int32_t* q_nkp;
  long nv_stride, desc_stride, nkp_stride;
  int nq, G, cap, D, capacity, vec;
  double thres;
  // launch state, zero between launches
  unsigned long long* best; int32_t* ticket;
  // outputs
  MatchPairDesc* pairs; const int32_t* zero;
  int64_t* o_tag; int32_t* o_pos; int32_t* o_da; int32_t* o_db; float* o_sim;      // [nq]
  float* o_sims;                                                                       // [nq][capacity][V]
  int32_t* o_lv; int32_t* o_rv;                                                        // [nq][V]
};

// One launch for all nq remote frames.  One wave per (remote frame q, window position pos): the V dot products of the remote gate view (0 / 2) with the keyframe's views
// dirs[j] = (2 + j) & 3 (stereo: view 0) -- lane l takes the elements 4l + 256t in ascending order as one fmaf chain per view, then the xor butterfly 32..1 -- compared in
// double as !(sim < thres) (:189-190, :220).  A wave proposes its first passing j under the key (n - 1 - pos) * V + j; the smallest key of a frame wins (an atomic maximum of
// its complement, with the similarity's bits in the low word).  The workgroup that arrives last writes the records and the matcher's table and zeroes the launch state.
template <int V>
__global__ __launch_bounds__(256) void window_gate_kernel(WinArgs a, WinOrder w) {
  __shared__ int s_last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = w.n, nq = a.nq, G = a.G;
  const long job = (long)blockIdx.x * 4 + wave;
  if (job < (long)nq * n) {
    const int q = (int)(job / n), pos = (int)(job - (long)q * n);
    const float* r = a.q_nv + (size_t)(q * V + (V == 4 ? 2 : 0)) * a.nv_stride;
    const float* k0 = a.store_nv + (size_t)w.slot[pos] * V * G;
    float s[V];
#pragma unroll
    for (int j = 0; j < V; ++j) s[j] = 0.f;
    for (int e = lane * 4; e < G; e += 256) {
      const f32x4 y = win_ld4(r + e, a.vec != 0);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(k0 + (size_t)(V == 4 ? ((2 + j) & 3) : 0) * G + e);
#pragma unroll
        for (int c = 0; c < 4; ++c) s[j] = __builtin_fmaf(x[c], y[c], s[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < V; ++j)
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s[j] += __shfl_xor(s[j], o, 64);
    if (lane == 0) {
      int first = -1;
      float sf = 0.f;
#pragma unroll
      for (int j = V - 1; j >= 0; --j) {
        a.o_sims[((size_t)q * a.capacity + pos) * V + j] = s[j];
        if (!((double)s[j] < a.thres)) { first = j; sf = s[j]; }      // the FIRST j that passes wins
      }
      if (first >= 0) {
        const unsigned key = (unsigned)((n - 1 - pos) * V + first);
        atomicMax(a.best + q, ((unsigned long long)(0xFFFFFFFFu - key) << 32) | (unsigned long long)__float_as_uint(sf));
      }
    }
  }
  __threadfence();
  __syncthreads();
  if (tid == 0) s_last = (atomicAdd(a.ticket, 1) == (int)gridDim.x - 1) ? 1 : 0;
  __syncthreads();
  if (!s_last) return;
  __threadfence();
  for (int q = tid; q < nq; q += blockDim.x) {
    const unsigned long long key = __hip_atomic_load(a.best + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(a.best + q, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // ready for the next launch
    int pos = -1, da = -1, db = -1, slot = 0;
    int64_t tag = -1;
    float sim = 0.f;
    if (key) {
      const int k = (int)(0xFFFFFFFFu - (unsigned)(key >> 32));
      pos = n - 1 - k / V;
      da = V == 4 ? 2 : 0; db = V == 4 ? ((2 + k % V) & 3) : 0;
      sim = __uint_as_float((unsigned)(key & 0xFFFFFFFFull));
      tag = w.tag[pos]; slot = w.slot[pos];
    }
    a.o_tag[q] = tag; a.o_pos[q] = pos; a.o_da[q] = da; a.o_db[q] = db; a.o_sim[q] = sim;
    for (int i = 0; i < V; ++i) {
      MatchPairDesc d;
      d.pts_a = nullptr; d.pts_b = nullptr; d.radius = -1.0;      // trackRemote without prediction: no points, no radius (:316-323)
      int lv = -1, rv = -1;
      if (pos >= 0) {
        // trackRemoteFrames (:273-284) with dir_cur = da, dir_prev = db: remote view (da + i) % V against local view (db - da + V) % V + da + i
        rv = (da + i) % V; lv = ((db - da + V) % V + da + i) % V;
        d.a = a.store_desc + ((size_t)slot * V + lv) * a.cap * a.D; d.na = a.store_nkp + (size_t)slot * V + lv;
        d.b = a.q_desc + (size_t)(q * V + rv) * a.desc_stride; d.nb = a.q_nkp + (size_t)(q * V + rv) * a.nkp_stride;
      } else {
        d.a = a.store_desc; d.b = a.store_desc; d.na = a.zero; d.nb = a.zero;
      }
      a.pairs[q * V + i] = d; a.o_lv[q * V + i] = lv; a.o_rv[q * V + i] = rv;
    }
  }
  // the similarities beyond the window: a slot's record is a pure function of the query
  const int tail = (a.capacity - n) * V;
  for (long t = tid; t < (long)nq * tail; t += blockDim.x) {
    const long q = t / tail, r = t - q * tail;
    a.o_sims[((size_t)q * a.capacity + n) * V + r] = 0.f;
  }
  if (tid == 0) __hip_atomic_store(a.ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// processFrame's emplace_back, device to device: workgroup (v, part) copies its share of view v's descriptors -- rows >= n_kp as zeros, so that a slot is a pure function
// of the frame -- and, part 0, the count and the view's NetVLAD row
__global__ __launch_bounds__(256) void window_copy_kernel(const float* __restrict__ src_nv, const float* __restrict__ src_desc, const int32_t* __restrict__ src_nkp,
                                                          float* __restrict__ dst_nv, float* __restrict__ dst_desc, int32_t* __restrict__ dst_nkp, int G, int cap, int D) {
  const int v = blockIdx.x, tid = threadIdx.x;
  const int n_raw = src_nkp[v], n = n_raw < 0 ? 0 : (n_raw > cap ? cap : n_raw);
  const int d4 = D / 4;
  const f32x4* s4 = reinterpret_cast<const f32x4*>(src_desc + (size_t)v * cap * D);
  f32x4* t4 = reinterpret_cast<f32x4*>(dst_desc + (size_t)v * cap * D);
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  for (int i = blockIdx.y * 256 + tid; i < cap * d4; i += gridDim.y * 256) t4[i] = (i / d4) < n ? s4[i] : z;
  if (blockIdx.y) return;
  for (int i = tid; i < G; i += 256) dst_nv[(size_t)v * G + i] = src_nv[(size_t)v * G + i];
  if (tid == 0) dst_nkp[v] = n;
}

}  // namespace

struct d2fe_window_s {
  PipeRef pipe;
  d2fe_handle h = nullptr;
  d2fe_window_config cfg{};
  int F = 0, V = 1, cap = 0, D = 0, G = 0, NQ = 0;
  // the store
  float* d_nv = nullptr; float* d_desc = nullptr; int32_t* d_nkp = nullptr;
  int32_t* d_state = nullptr;      // [0] the zero word, [1] the gate's ticket
  unsigned long long* d_best = nullptr;
  int32_t* d_match_scratch = nullptr;
  // host bookkeeping: the window oldest first, the tag of every slot, the free slots
  std::vector<int> order; std::vector<int64_t> slot_tag; std::vector<int> free_slots;
  struct Lay { size_t mq = 0, mt = 0, md = 0, mn = 0, lv = 0, rv = 0, tag = 0, pos = 0, da = 0, db = 0, sim = 0, sims = 0, words = 0; };
  struct Slot : SlotBase { MatchPairDesc* d_pairs = nullptr; int nq = 0, n_window = 0; Lay lay; };
  std::vector<Slot> slots;
  size_t out_words = 0;
  hipStream_t st = nullptr;
  hipEvent_t ev_in = nullptr;      // orders the window's stream behind the producer's
};

namespace {

// one result record for nq frames: the words in use are contiguous, so the D2H carries what the query wrote and nothing else
d2fe_window_s::Lay win_layout(int nq, int V, int cap, int capacity) {
  auto up = [](size_t w) { return (w + 15) / 16 * 16; };
  d2fe_window_s::Lay l;
  const size_t np = (size_t)nq * V;
  size_t o = 0;
  l.tag = o; o += up(2 * (size_t)nq);      // int64: first, 8-byte aligned
  l.pos = o; o += up(nq); l.da = o; o += up(nq); l.db = o; o += up(nq); l.sim = o; o += up(nq);
  l.sims = o; o += up((size_t)nq * capacity * V);
  l.lv = o; o += up(np); l.rv = o; o += up(np); l.mn = o; o += up(np);
  l.mq = o; o += up(np * cap); l.mt = o; o += up(np * cap); l.md = o; o += up(np * cap);
  l.words = o;
  return l;
}

void window_destroy(d2fe_window_s* x) {
  if (!x) return;
  if (x->h) (void)hipSetDevice(x->h->cfg.device_id);
  if (x->st) (void)hipStreamSynchronize(x->st);
  for (auto& S : x->slots) {
    if (S.d_pairs) (void)hipFree(S.d_pairs);
    S.free();
  }
  for (void* q : {(void*)x->d_nv, (void*)x->d_desc, (void*)x->d_nkp, (void*)x->d_state, (void*)x->d_best, (void*)x->d_match_scratch})
    if (q) (void)hipFree(q);
  if (x->ev_in) (void)hipEventDestroy(x->ev_in);
  if (x->st) (void)hipStreamDestroy(x->st);
  delete x;
}

int window_create(PipeRef pipe, const d2fe_window_config* cfg_in, d2fe_window* out) {
  if (!pipe || !cfg_in || !out) return ctx_fail(D2FE_ERR_INVALID, "null argument");
  *out = nullptr;
  d2fe_window_config cfg;
  d2fe_window_default_config(&cfg);
  take_config(cfg, cfg_in);
  if (cfg.capacity < 1 || cfg.capacity > WIN_MAXKF || cfg.slots < 1 || cfg.slots > 64 || (cfg.mode != 0 && cfg.mode != 1) || cfg.max_queries < 1 || cfg.max_queries > WIN_MAXNQ)
    return ctx_fail(D2FE_ERR_INVALID, "bad window configuration");
  int pf = 0, pcap = 0, pdim = 0, pg = 0;
  { const int rc = pipe.geometry(&pf, &pcap, &pdim, &pg); if (rc) return rc; }
  if (pg <= 0) return ctx_fail(D2FE_ERR_INVALID, "the keyframe window needs the pipe's NetVLAD (netvlad = 1)");
  if ((pg & 3) || (pdim & 3)) return ctx_fail(D2FE_ERR_UNSUPPORTED, "the NetVLAD and descriptor lengths must be multiples of 4");
  auto* x = new (std::nothrow) d2fe_window_s();
  if (!x) return ctx_fail(D2FE_ERR_HIP, "out of memory");
  struct Guard { d2fe_window_s* x; bool ok = false; ~Guard() { if (!ok) window_destroy(x); } } guard{x};
  x->pipe = pipe; x->h = pipe.handle(); x->cfg = cfg;
  x->F = pf; x->cap = pcap; x->D = pdim; x->G = pg; x->V = pipe.views(); x->NQ = cfg.max_queries;
  const int V = x->V, NQ = x->NQ, K = cfg.capacity;
  x->slot_tag.assign(K, -1);
  for (int s = K - 1; s >= 0; --s) x->free_slots.push_back(s);      // slot 0 is taken first
  HIP_TRY(hipSetDevice(x->h->cfg.device_id));
  HIP_TRY(hipStreamCreateWithFlags(&x->st, hipStreamNonBlocking));
  HIP_TRY(hipEventCreateWithFlags(&x->ev_in, hipEventDisableTiming));
  HIP_TRY(hipMalloc(&x->d_nv, sizeof(float) * (size_t)K * V * pg)); HIP_TRY(hipMemset(x->d_nv, 0, sizeof(float) * (size_t)K * V * pg));
  HIP_TRY(hipMalloc(&x->d_desc, sizeof(float) * (size_t)K * V * pcap * pdim)); HIP_TRY(hipMemset(x->d_desc, 0, sizeof(float) * (size_t)K * V * pcap * pdim));
  HIP_TRY(hipMalloc(&x->d_nkp, sizeof(int32_t) * (size_t)K * V)); HIP_TRY(hipMemset(x->d_nkp, 0, sizeof(int32_t) * (size_t)K * V));
  HIP_TRY(hipMalloc(&x->d_state, sizeof(int32_t) * 16)); HIP_TRY(hipMemset(x->d_state, 0, sizeof(int32_t) * 16));
  HIP_TRY(hipMalloc(&x->d_best, sizeof(unsigned long long) * WIN_MAXNQ)); HIP_TRY(hipMemset(x->d_best, 0, sizeof(unsigned long long) * WIN_MAXNQ));
  const size_t msb = match_scratch_bytes(NQ * V, pcap);
  HIP_TRY(hipMalloc(&x->d_match_scratch, msb)); HIP_TRY(hipMemset(x->d_match_scratch, 0, msb));
  x->out_words = win_layout(NQ, V, pcap, K).words;
  x->slots.resize(cfg.slots);
  for (auto& S : x->slots) {
    { const int rc = S.alloc(x->out_words, x->out_words, cfg.timing != 0); if (rc) return rc; }
    HIP_TRY(hipMalloc(&S.d_pairs, sizeof(MatchPairDesc) * (size_t)NQ * V));
  }
  HIP_TRY(hipDeviceSynchronize());
  guard.ok = true;
  *out = x;
  return D2FE_OK;
}

// what a push has to decide before anything is queued: 1 = the newest tag again (a no-op, :806-808), 0 = go on, else the refusal
int window_push_check(d2fe_window_s* x, int64_t tag) {
  if (tag < 0) return ctx_fail(D2FE_ERR_INVALID, "a tag is a non-negative frame_id (-1 marks a frame without a hit)");
  if (!x->order.empty() && x->slot_tag[x->order.back()] == tag) return 1;
  for (int s : x->order)
    if (x->slot_tag[s] == tag) return ctx_fail(D2FE_ERR_INVALID, "this tag is in the window already: nothing was queued");
  if (x->free_slots.empty()) return ctx_fail(D2FE_ERR_TRUNCATED, "the keyframe window is full (d2fe_window_retain frees slots): nothing was queued");
  return 0;
}

void window_commit(d2fe_window_s* x, int64_t tag) {
  const int s = x->free_slots.back();
  x->free_slots.pop_back();
  x->slot_tag[s] = tag;
  x->order.push_back(s);
}

}  // namespace

extern "C" {

void d2fe_window_default_config(d2fe_window_config* c) {
  if (!c) return;
  memset(c, 0, sizeof(*c));
  c->struct_size = (int32_t)sizeof(*c);
  c->capacity = 12; c->mode = 0; c->slots = 4; c->timing = 0; c->max_queries = 64; c->thres = 0.8; c->ratio = 0.8;
}

int d2fe_window_create(d2fe_pipe p, const d2fe_window_config* cfg, d2fe_window* out) {
  if (!p) return ctx_fail(D2FE_ERR_INVALID, "null argument");
  return window_create(p, cfg, out);
}
int d2fe_window_create_quad(d2fe_quad_pipe p, const d2fe_window_config* cfg, d2fe_window* out) {
  if (!p) return ctx_fail(D2FE_ERR_INVALID, "null argument");
  return window_create(p, cfg, out);
}
void d2fe_window_destroy(d2fe_window x) { window_destroy(x); }
void* d2fe_window_stream(d2fe_window x) { return x ? x->st : nullptr; }
int d2fe_window_size(d2fe_window x) { return x ? (int)x->order.size() : ctx_fail(D2FE_ERR_INVALID, "null window"); }
int d2fe_window_tags(d2fe_window x, int64_t* tags, int cap_tags) {
  if (!x || (cap_tags > 0 && !tags) || cap_tags < 0) return ctx_fail(D2FE_ERR_INVALID, "bad argument");
  for (int i = 0; i < (int)x->order.size() && i < cap_tags; ++i) tags[i] = x->slot_tag[x->order[i]];
  return (int)x->order.size();
}

int d2fe_window_retain_plan(const int64_t* tags, int n, const int64_t* keep, int nkeep, uint8_t* evict_out) {
  if (n < 0 || nkeep < 0 || (n > 0 && !tags) || (nkeep > 0 && !keep)) return ctx_fail(D2FE_ERR_INVALID, "bad argument");
  int dropped = 0;
  for (int i = 0; i < n; ++i) {
    // :49-50: not in the sliding window and not the newest keyframe
    const bool listed = std::find(keep, keep + nkeep, tags[i]) != keep + nkeep;
    const bool drop = !listed && tags[i] != tags[n - 1];
    if (evict_out) evict_out[i] = drop ? 1 : 0;
    dropped += drop ? 1 : 0;
  }
  return dropped;
}

int d2fe_window_retain(d2fe_window x, const int64_t* tags, int n) {
  if (!x || n < 0 || (n > 0 && !tags)) return ctx_fail(D2FE_ERR_INVALID, "bad argument");
  const int nw = (int)x->order.size();
  std::vector<int64_t> cur(nw);
  std::vector<uint8_t> ev(nw);
  for (int i = 0; i < nw; ++i) cur[i] = x->slot_tag[x->order[i]];
  const int dropped = d2fe_window_retain_plan(cur.data(), nw, tags, n, ev.data());
  if (dropped <= 0) return dropped;
  std::vector<int> kept;
  for (int i = 0; i < nw; ++i) {
    const int s = x->order[i];
    if (ev[i]) { x->slot_tag[s] = -1; x->free_slots.push_back(s); } else kept.push_back(s);
  }
  x->order.swap(kept);
  return dropped;
}

int d2fe_window_push(d2fe_window x, int64_t ticket, int frame, int64_t tag) {
  if (!x || frame < 0 || frame >= x->F) return ctx_fail(D2FE_ERR_INVALID, "bad argument");
  { const int c = window_push_check(x, tag); if (c) return c < 0 ? c : D2FE_OK; }
  HIP_TRY(hipSetDevice(x->h->cfg.device_id));
  hipStream_t st = x->st;
  const int V = x->V, s = x->free_slots.back();
  const int rc = with_view(x->pipe, ticket, st, [&](const TicketView& v) -> int {
    if (v.frames != x->F || v.cap != x->cap || v.desc_dim != x->D || v.netvlad_dim != x->G || !v.d_netvlad)
      return ctx_fail(D2FE_ERR_INVALID, "the pipe's geometry changed under the keyframe window");
    const size_t row = (size_t)frame * V, blk = (size_t)x->cap * x->D;
    const int parts = (int)std::min<size_t>(16, std::max<size_t>(1, blk / 4096));
    hipLaunchKernelGGL(window_copy_kernel, dim3((unsigned)V, (unsigned)parts), dim3(256), 0, st, v.d_netvlad + row * x->G, v.d_desc + row * blk, v.d_n_kp + row,
                       x->d_nv + (size_t)s * V * x->G, x->d_desc + (size_t)s * V * blk, x->d_nkp + (size_t)s * V, x->G, x->cap, x->D);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? ctx_fail(D2FE_ERR_HIP, std::string("window_copy_kernel: ") + hipGetErrorString(e)) : D2FE_OK;
  });
  if (rc) return rc;
  window_commit(x, tag);
  return D2FE_OK;
}

int d2fe_window_push_host(d2fe_window x, const float* netvlad, const float* desc, const int32_t* n_kp, int64_t tag) {
  if (!x || !netvlad || !n_kp) return ctx_fail(D2FE_ERR_INVALID, "bad argument");
  const int V = x->V;
  for (int v = 0; v < V; ++v)
    if (n_kp[v] < 0 || (n_kp[v] > 0 && !desc)) return ctx_fail(D2FE_ERR_INVALID, "negative count, or keypoints without descriptors");
  { const int c = window_push_check(x, tag); if (c) return c < 0 ? c : D2FE_OK; }
  HIP_TRY(hipSetDevice(x->h->cfg.device_id));
  HIP_TRY(hipStreamSynchronize(x->st));      // an earlier query may still read the slot this keyframe goes to
  const int s = x->free_slots.back();
  const size_t blk = (size_t)x->cap * x->D;
  std::vector<float> stage((size_t)V * blk, 0.f);
  std::vector<int32_t> cnt(V);
  for (int v = 0; v < V; ++v) {
    cnt[v] = std::min(n_kp[v], x->cap);
    if (cnt[v] > 0) memcpy(stage.data() + v * blk, desc + v * blk, sizeof(float) * (size_t)cnt[v] * x->D);
  }
  HIP_TRY(hipMemcpy(x->d_desc + (size_t)s * V * blk, stage.data(), sizeof(float) * stage.size(), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(x->d_nv + (size_t)s * V * x->G, netvlad, sizeof(float) * (size_t)V * x->G, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(x->d_nkp + (size_t)s * V, cnt.data(), sizeof(int32_t) * (size_t)V, hipMemcpyHostToDevice));
  window_commit(x, tag);
  return D2FE_OK;
}

int d2fe_window_track_device(d2fe_window x, const float* d_netvlad, size_t nv_stride, const float* d_desc, size_t desc_stride, const int32_t* d_n_kp, size_t nkp_stride,
                             int nq, int slot, void* stream) {
  if (!x || !d_netvlad || !d_desc || !d_n_kp || slot < 0 || slot >= (int)x->slots.size()) return ctx_fail(D2FE_ERR_INVALID, "bad argument");
  if (nq < 1 || nq > x->NQ) return ctx_fail(D2FE_ERR_INVALID, "nq out of range (d2fe_window_config.max_queries)");
  if (nv_stride < (size_t)x->G || desc_stride < (size_t)x->cap * x->D || nkp_stride < 1) return ctx_fail(D2FE_ERR_INVALID, "a stride is shorter than its row");
  if ((reinterpret_cast<uintptr_t>(d_desc) & 15) || (desc_stride & 3)) return ctx_fail(D2FE_ERR_INVALID, "descriptor rows must be 16-byte aligned");
  if ((reinterpret_cast<uintptr_t>(d_netvlad) & 3) || (reinterpret_cast<uintptr_t>(d_n_kp) & 3)) return ctx_fail(D2FE_ERR_INVALID, "misaligned array");
  auto& S = x->slots[slot];
  if (S.busy) return ctx_fail(D2FE_ERR_NOT_READY, "this slot's previous window query has not been collected");
  HIP_TRY(hipSetDevice(x->h->cfg.device_id));
  hipStream_t st = x->st;
  if (stream) { HIP_TRY(hipEventRecord(x->ev_in, static_cast<hipStream_t>(stream))); HIP_TRY(hipStreamWaitEvent(st, x->ev_in, 0)); }
  const int V = x->V, n = (int)x->order.size();
  WinOrder w{};
  w.n = n;
  for (int i = 0; i < n; ++i) { w.slot[i] = (uint8_t)x->order[i]; w.tag[i] = x->slot_tag[x->order[i]]; }
  const auto lay = win_layout(nq, V, x->cap, x->cfg.capacity);
  int32_t* O = reinterpret_cast<int32_t*>(S.d_out);
  WinArgs a{};
  a.store_nv = x->d_nv; a.store_desc = x->d_desc; a.store_nkp = x->d_nkp;
  a.q_nv = d_netvlad; a.q_desc = d_desc; a.q_nkp = d_n_kp; a.nv_stride = (long)nv_stride; a.desc_stride = (long)desc_stride; a.nkp_stride = (long)nkp_stride;
  a.nq = nq; a.G = x->G; a.cap = x->cap; a.D = x->D; a.capacity = x->cfg.capacity; a.thres = x->cfg.thres;
  a.vec = (!(reinterpret_cast<uintptr_t>(d_netvlad) & 15) && !(nv_stride & 3)) ? 1 : 0;
  a.best = x->d_best; a.ticket = x->d_state + 1; a.zero = x->d_state; a.pairs = S.d_pairs;
  a.o_tag = reinterpret_cast<int64_t*>(O + lay.tag); a.o_pos = O + lay.pos; a.o_da = O + lay.da; a.o_db = O + lay.db; a.o_sim = S.d_out + lay.sim; a.o_sims = S.d_out + lay.sims;
  a.o_lv = O + lay.lv; a.o_rv = O + lay.rv;
  auto mark = [&](int i) { return S.mark(i, st); };
  int r = mark(0); if (r) return r;
  const unsigned nwg = (unsigned)std::max<long>(1, ((long)nq * n + 3) / 4);
  if (V == 4) hipLaunchKernelGGL(window_gate_kernel<4>, dim3(nwg), dim3(256), 0, st, a, w);
  else hipLaunchKernelGGL(window_gate_kernel<1>, dim3(nwg), dim3(256), 0, st, a, w);
  HIP_TRY(hipGetLastError());
  r = mark(1); if (r) return r;
  MatchArgs m{};
  m.pairs = S.d_pairs; m.npairs = nq * V; m.dim = x->D; m.max_n = x->cap; m.mode = x->cfg.mode; m.ratio = x->cfg.ratio; m.radius = -1.0;
  match_outputs(m, O + lay.mq, O + lay.mt, S.d_out + lay.md, O + lay.mn, x->d_match_scratch, x->NQ * V, x->h);
  HIP_TRY(launch_match(m, st));
  r = mark(2); if (r) return r;
  r = S.finish(st, lay.words, 3); if (r) return r;      // the words in use: the D2H carries what the query wrote and nothing else
  S.nq = nq; S.n_window = n; S.lay = lay;
  return D2FE_OK;
}

int d2fe_window_collect(d2fe_window x, int slot, d2fe_window_result* out) {
  if (!x || !out || slot < 0 || slot >= (int)x->slots.size()) return ctx_fail(D2FE_ERR_INVALID, "bad argument");
  auto& S = x->slots[slot];
  if (!S.busy) return ctx_fail(D2FE_ERR_INVALID, "nothing was queued on this slot");
  HIP_TRY(hipSetDevice(x->h->cfg.device_id));
  { const int rc = S.collect_begin(); if (rc) return rc; }
  memset(out, 0, sizeof(*out));
  const int32_t* I = reinterpret_cast<const int32_t*>(S.pin);
  const auto& l = S.lay;
  out->nq = S.nq; out->views = x->V; out->cap = x->cap; out->capacity = x->cfg.capacity; out->n_window = S.n_window;
  out->keyframe_tag = reinterpret_cast<const int64_t*>(I + l.tag); out->keyframe_pos = I + l.pos; out->dir_a = I + l.da; out->dir_b = I + l.db;
  out->sim = S.pin + l.sim; out->sims = S.pin + l.sims; out->local_view = I + l.lv; out->remote_view = I + l.rv; out->n_match = I + l.mn;
  out->q_idx = I + l.mq; out->t_idx = I + l.mt; out->dist = S.pin + l.md;
  S.phase_ms(out->phase_ms, 3);
  return D2FE_OK;
}

}  // extern "C"
