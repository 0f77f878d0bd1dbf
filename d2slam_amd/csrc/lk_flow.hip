// lk_flow.hip -- the flow landmarks of enable_lk_optical_flow without sp_track_use_lk on the device (include/d2fe.h, d2fe_lk_flow_step_device, d2fe_detect_fast_device).
//   D2FeatureTracker::trackLK(frame)   d2frontend/src/d2featuretracker.cpp:472-621: track the previous list (opticalflowTrackPyr, opticaltrack_utils.cpp:173-279), reduceVector,
//                                      removeNearPoints, then detectPoints(..., use_fast = true) (:375-442) against landmarks2D() = the SuperPoint keypoints + the tracked entries
//   detectFastByRegion                 opticaltrack_utils.cpp:444-493: FAST per region, sorted by response, the first `features`
//
// MI355X mapping.  One frame = FIVE launches, whatever the list holds:
//   1. lk_flow_step_kernel   one 64-lane wave per entry of the previous list tracks it and the workgroups take the list's ticket (list_track_and_arrive); the last
//                            workgroup to arrive runs b-c (list_reduce_prune), writes the tracked entries and decides `lack` and `num` into the list header.  Both
//                            functions, the per-camera view of the arguments (ListCamera), the quad-level id hand-out and the entry points' shared refusals are
//                            lk_list_device.h's: one copy for this list and the SuperPoint list (lk_carry.hip)
//   2. fast_clear_kernel     score map and candidate count to zero
//   3. fast_region_kernel    } fast_device.h, the kernels of d2fe_detect_fast_by_region; `features` is header word `num`, read on the device
//   4. fast_nonmax_kernel    }
//   5. lk_flow_merge_kernel  ONE workgroup: exact top-`num` of the candidate pool in (response, order) order, the distance filter of detectPoints, the new entries
// Launches 2-5 read `num` first and return when it is 0 (the steady state: the list is full enough), so a frame that does not detect costs launch 1 and four empty grids.
// The host sort of d2fe_detect_fast_by_region becomes fast_select_sorted: the candidates carry a unique key of 40 significant bits -- the response in bits 32..39 (a FAST score is at most 254, so 8 bits hold it) above ~order in bits 0..31 --
// and five 8-bit histogram passes, which cover exactly bits 0..39, find the K-th largest key over the pool exactly; the K candidates at or above it are compacted into LDS (ballot + one LDS atomic per wave) and each
// is ranked by counting the larger keys (K <= 2048: 2 x 2048 broadcast LDS reads a thread).  The merge then tests every selected candidate against the keypoints and the
// tracked entries in parallel (a thread per candidate) and only the test against the candidates accepted before it runs in order, on one wave, as the replenish loop of
// lk_carry.hip does.  LDS of launch 5: 16 KB keys + 8 KB indices + 8 KB order + 8 KB list + 2 KB flags + 1 KB histogram = 43 KB of the CU's 160 KB.
//
// The quadcam form (d2fe_lk_flow_quad_step_device; trackLocalFrames without sp_track_use_lk): the same five launches with the camera as a grid dimension -- launch 1 is
// (slots / 4, 4 cameras) workgroups with a ticket per camera, launches 2-4 run fast_device.h's bodies on the camera's own image, `num`, score map, pool and count,
// launch 5 is four workgroups of 1024 (43 KB of LDS each) that select and merge side by side and then take a quad-level ticket (header word 10 of camera 0's list), whose
// last arrival hands the ids out in camera order from the one counter.  Every byte equals four single steps in camera order; a quad frame in which no camera detects
// costs launch 1 and four empty grids.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/d2fe.h"
#include "context.h"
#include "kernels.h"
#include "fast_device.h"
#include "lk_device.h"
#include "lk_list_device.h"

namespace d2fe {

namespace {

constexpr int FLOW_KMAX = 2 * LKC_MAX;      // candidates the selection keeps: num <= 2 * total_feature_num

// header words of a flow list behind the seven of the carry list (include/d2fe.h)
enum { FLOW_HDR_LACK = 7, FLOW_HDR_NUM = 8, FLOW_HDR_CAND = 9 };

struct FlowScratch {
  int* score; int4* pool; int* count;
  int pool_cap;
  size_t bytes;
};
inline FlowScratch flow_scratch(void* base, int width, int height, int cap_tracks, int cols, int rows) {
  FlowScratch f{};
  const size_t sbytes = (sizeof(int) * (size_t)width * height + 15) / 16 * 16;      // keeps the int4 pool 16-byte aligned
  f.pool_cap = cols * rows * 2 * cap_tracks;
  char* b = static_cast<char*>(base);
  f.score = reinterpret_cast<int*>(b);
  f.pool = reinterpret_cast<int4*>(b + sbytes);
  f.count = reinterpret_cast<int*>(b + sbytes + sizeof(int4) * (size_t)f.pool_cap);
  f.bytes = sbytes + sizeof(int4) * (size_t)f.pool_cap + 16;
  return f;
}

__global__ __launch_bounds__(256) void fast_clear_kernel(const int* __restrict__ d_features, int4* __restrict__ score4, int n4, int* __restrict__ count) {
  if (d_features[0] <= 0) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n4) score4[i] = int4{0, 0, 0, 0};
  if (i == 0) count[0] = 0;
}

// 40 significant bits (response <= 254 in bits 32..39, ~order in bits 0..31): larger = earlier, response descending, then order ascending
__device__ __forceinline__ unsigned long long fast_key(const int4& c) {
  return ((unsigned long long)(unsigned)c.z << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)c.w);
}

// LDS of the selection (one workgroup of 1024 threads)
struct SelectLds {
  unsigned long long key[FLOW_KMAX];
  int idx[FLOW_KMAX], ord[FLOW_KMAX];
  int hist[256];
  unsigned long long prefix;
  int need, cnt;
};

// The first K = min(features, N, FLOW_KMAX) of the pool's N candidates in the order of detectFastByRegion's sort: L.ord[0 .. K) are their pool indices.  Exact for any
// N: the keys are unique (order is the pixel), so exactly K keys are >= the K-th largest.  Every thread of the workgroup calls it; the result is visible on return
__device__ __forceinline__ int fast_select_sorted(const int4* __restrict__ pool, int N, int features, SelectLds& L) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int K = min(min(features, N), FLOW_KMAX);
  unsigned long long T = 0ull;
  if (K < N) {
    if (tid == 0) { L.prefix = 0ull; L.need = K; }
    for (int shift = 32; shift >= 0; shift -= 8) {
      if (tid < 256) L.hist[tid] = 0;
      __syncthreads();
      const unsigned long long prefix = L.prefix;
      for (int i = tid; i < N; i += 1024) {
        const unsigned long long k = fast_key(pool[i]);
        if ((k >> (shift + 8)) == prefix) atomicAdd(&L.hist[(int)((k >> shift) & 255ull)], 1);
      }
      __syncthreads();
      if (tid < 64) {      // wave 0: the bin, from the top, in which the cumulative count reaches `need`; lane l owns bins 255 - 4 l .. 252 - 4 l
        int c[4], s = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) { c[j] = L.hist[255 - (4 * lane + j)]; s += c[j]; }
        int incl = s;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(incl, o, 64); if (lane >= o) incl += v; }
        const int need = L.need;
        int above = incl - s;
        if (above < need && need <= incl) {      // exactly one lane
          int j = 0;
          while (above + c[j] < need) { above += c[j]; ++j; }
          L.prefix = (prefix << 8) | (unsigned long long)(255 - (4 * lane + j));
          L.need = need - above;
        }
      }
      __syncthreads();
    }
    T = L.prefix;
  }
  // compaction of the K selected candidates (any order), then the rank of each among them
  if (tid == 0) L.cnt = 0;
  __syncthreads();
  for (int base = 0; base < N; base += 1024) {
    const int i = base + tid;
    unsigned long long k = 0ull;
    bool sel = false;
    if (i < N) { k = fast_key(pool[i]); sel = k >= T; }
    const unsigned long long bal = __ballot(sel);
    int wbase = 0;
    if (lane == 0 && bal) wbase = atomicAdd(&L.cnt, __popcll(bal));
    wbase = __shfl(wbase, 0, 64);
    const int slot = wbase + __popcll(bal & ((1ull << lane) - 1ull));
    if (sel && slot < K) { L.key[slot] = k; L.idx[slot] = i; }
  }
  __syncthreads();
  for (int i = tid; i < K; i += 1024) {
    const unsigned long long mine = L.key[i];
    int r = 0;
    for (int j = 0; j < K; ++j) r += L.key[j] > mine ? 1 : 0;
    L.ord[r] = L.idx[i];
  }
  __syncthreads();
  return K;
}

// launch 4 of d2fe_detect_fast_device: the selection alone, into the caller's arrays
__global__ __launch_bounds__(1024) void fast_select_kernel(const int* __restrict__ d_features, const int4* __restrict__ pool, const int* __restrict__ count, int pool_cap,
                                                           int max_features, float* __restrict__ xy, int* __restrict__ response, int cap, int* __restrict__ n_out) {
  __shared__ SelectLds L;
  const int features = min(d_features[0], max_features);
  if (features <= 0) {
    if (threadIdx.x == 0) n_out[0] = 0;
    return;
  }
  const int K = fast_select_sorted(pool, min(count[0], pool_cap), min(features, cap), L);
  for (int k = threadIdx.x; k < K; k += 1024) {
    const int4 c = pool[L.ord[k]];
    xy[2 * k] = (float)c.x; xy[2 * k + 1] = (float)c.y;
    if (response) response[k] = c.z;
  }
  if (threadIdx.x == 0) n_out[0] = K;
}

struct LkFlowArgs : LkListArgs { const int4* pool; const int* count; int pool_cap; };      // lay.D = 0; the detector's candidate pool beside LkListArgs

// the camera's view (lk_list_device.h) with its candidate pool and count, which lie in the camera's own detector scratch
struct FlowCamera : ListCamera { const int4* pool; const int* count; };
__device__ __forceinline__ FlowCamera flow_camera(const LkFlowArgs& c, int cam, long list_stride, size_t pyr_stride, size_t scratch_stride) {
  return FlowCamera{list_camera(c, cam, list_stride, pyr_stride), reinterpret_cast<const int4*>(reinterpret_cast<const char*>(c.pool) + (size_t)cam * scratch_stride),
                    reinterpret_cast<const int*>(reinterpret_cast<const char*>(c.count) + (size_t)cam * scratch_stride)};
}

// launch 1: steps a-c and the decision of detectPoints, for workgroup bx of the nblocks that step this list
__device__ __forceinline__ void flow_step_body(const LkFlowArgs& c, const ListCamera& v, int bx, int nblocks) {
  __shared__ float s_x[LKC_MAX], s_y[LKC_MAX];
  __shared__ int s_src[LKC_MAX];
  __shared__ int s_cnt[4];          // [1] survivors of the tracker, [2] survivors of removeNearPoints, [3] this workgroup arrived last
  int n_prev;
  if (!list_track_and_arrive(c, v, bx, nblocks, s_cnt + 3, n_prev)) return;      // step a and the ticket (lk_list_device.h)
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cap = c.lay.cap;
  int* hdr = reinterpret_cast<int*>(v.cur);
  float* trk_xy = v.cur + c.lay.off[D2FE_LKC_TRK_XY];
  uint8_t* trk_st = reinterpret_cast<uint8_t*>(v.cur + c.lay.off[D2FE_LKC_TRK_STATUS]);

  // ---- b-c on wave 0
  if (wave == 0) {
    int cnt = 0;
    const int m = list_reduce_prune(trk_xy, trk_st, n_prev, c.near_thr, s_x, s_y, s_src, lane, cnt);
    if (lane == 0) { s_cnt[1] = cnt; s_cnt[2] = m; }
  }
  __syncthreads();
  // ---- the tracked entries (step e's first half), zeros behind them
  const int cnt = s_cnt[1], m = s_cnt[2];
  float* pts = v.cur + c.lay.off[D2FE_LKC_PTS];
  int* id = reinterpret_cast<int*>(v.cur + c.lay.off[D2FE_LKC_ID]);
  int* src = reinterpret_cast<int*>(v.cur + c.lay.off[D2FE_LKC_SRC]);
  const int* pid = reinterpret_cast<const int*>(v.prev + c.lay.off[D2FE_LKC_ID]);
  for (int k = tid; k < cap; k += 256) {
    const bool live = k < m;
    const int sk = live ? s_src[k] : 0;
    pts[2 * k] = live ? s_x[k] : 0.f; pts[2 * k + 1] = live ? s_y[k] : 0.f;
    id[k] = live ? pid[sk] : 0;
    src[k] = sk;
    if (k >= n_prev) { trk_xy[2 * k] = 0.f; trk_xy[2 * k + 1] = 0.f; trk_st[k] = 0; }
  }
  // ---- d, the decision (opticaltrack_utils.cpp:379-392): detect when more than a quarter is missing, twice the shortfall when anything exists
  if (tid == 0) {
    const int have = list_n_kp(c, v) + m;
    const int lack = c.total - have;
    const int num = lack > c.total / 4 ? (have > 0 ? 2 * lack : lack) : 0;
    hdr[0] = m; hdr[1] = n_prev; hdr[2] = n_prev - cnt; hdr[3] = cnt - m; hdr[4] = 0;
    hdr[6] = *c.next_id;
    hdr[FLOW_HDR_LACK] = lack; hdr[FLOW_HDR_NUM] = num; hdr[FLOW_HDR_CAND] = 0;
  }
  if (tid >= 10 && tid < 64) hdr[tid] = 0;
}

__global__ __launch_bounds__(256) void lk_flow_step_kernel(LkFlowArgs c) { flow_step_body(c, list_camera(c, 0, 0, 0), blockIdx.x, gridDim.x); }

// launch 5: the rest of step d and the new entries of step e, for a list whose `num` is > 0.  QUAD (the four-camera launch, lk_flow_quad_merge_kernel): the ids of the new
// entries, header word 6 and *next_id belong to the launch's last finisher, which knows the new entries of the lower cameras; they are left alone here
template <bool QUAD>
__device__ __forceinline__ void flow_merge_body(const LkFlowArgs& c, const FlowCamera& v) {
  __shared__ SelectLds L;
  __shared__ float s_x[LKC_MAX], s_y[LKC_MAX];      // the tracked entries, then the accepted candidates
  __shared__ uint8_t s_blocked[FLOW_KMAX];
  __shared__ int s_acc;
  int* hdr = reinterpret_cast<int*>(v.cur);
  const int num = hdr[FLOW_HDR_NUM];
  const int tid = threadIdx.x, lane = tid & 63;
  const int m = hdr[0], lack = hdr[FLOW_HDR_LACK], n_kp = list_n_kp(c, v);
  const int id0 = QUAD ? 0 : *c.next_id;
  float* pts = v.cur + c.lay.off[D2FE_LKC_PTS];
  const int K = fast_select_sorted(v.pool, min(v.count[0], c.pool_cap), num, L);
  // the selected candidates in order (over the keys, which the ranking no longer needs) and the tracked entries
  float* s_cx = reinterpret_cast<float*>(L.key);
  float* s_cy = s_cx + FLOW_KMAX;
  for (int k = tid; k < K; k += 1024) {
    const int4 p = v.pool[L.ord[k]];
    s_cx[k] = (float)p.x; s_cy[k] = (float)p.y;
  }
  for (int k = tid; k < m; k += 1024) { s_x[k] = pts[2 * k]; s_y[k] = pts[2 * k + 1]; }
  __syncthreads();
  // a candidate nearer than feature_min_dist to a keypoint or to a tracked entry is out whatever the order: a thread per candidate
  const double thr = c.min_dist, t2 = thr * thr, lo = t2 * (1.0 - 1e-12), hi = t2 * (1.0 + 1e-12);
  for (int k = tid; k < K; k += 1024) {
    const float px = s_cx[k], py = s_cy[k];
    bool hit = false;
    for (int j = 0; j < n_kp && !hit; ++j) hit = nearer(px, py, v.kps[2 * j], v.kps[2 * j + 1], thr, lo, hi);
    for (int j = 0; j < m && !hit; ++j) hit = nearer(px, py, s_x[j], s_y[j], thr, lo, hi);
    s_blocked[k] = hit ? 1 : 0;
  }
  __syncthreads();
  // the candidates accepted before it: in order, on one wave, until `lack` are in (m + lack <= total_feature_num <= cap_tracks)
  if (tid < 64) {
    int acc = 0;
    for (int k = 0; k < K && acc < lack; ++k) {
      if (s_blocked[k]) continue;
      const float px = s_cx[k], py = s_cy[k];
      bool hit = false;
      for (int j = lane; j < acc; j += 64) hit = hit || nearer(px, py, s_x[m + j], s_y[m + j], thr, lo, hi);
      if (__ballot(hit) == 0ull) {
        if (lane == 0) { s_x[m + acc] = px; s_y[m + acc] = py; }
        ++acc;
        wave_lds_sync();
      }
    }
    if (lane == 0) s_acc = acc;
  }
  __syncthreads();       // also: every thread has read *next_id
  const int acc = s_acc;
  int* id = reinterpret_cast<int*>(v.cur + c.lay.off[D2FE_LKC_ID]);
  int* src = reinterpret_cast<int*>(v.cur + c.lay.off[D2FE_LKC_SRC]);
  for (int e = tid; e < acc; e += 1024) {
    pts[2 * (m + e)] = s_x[m + e]; pts[2 * (m + e) + 1] = s_y[m + e];
    if (!QUAD) id[m + e] = id0 + e;
    src[m + e] = -1;
  }
  if (tid == 0) {
    hdr[0] = m + acc; hdr[4] = acc; hdr[FLOW_HDR_CAND] = K;
    if (!QUAD) { hdr[6] = id0 + acc; *c.next_id = id0 + acc; }
  }
}

__global__ __launch_bounds__(1024) void lk_flow_merge_kernel(LkFlowArgs c) {
  if (reinterpret_cast<const int*>(c.cur)[FLOW_HDR_NUM] <= 0) return;
  flow_merge_body<false>(c, flow_camera(c, 0, 0, 0, 0));
}

// ---- the quadcam form ---------------------------------------------------------------------------------------------------------------------------------------
// trackLocalFrames without sp_track_use_lk (d2featuretracker.cpp:121-133): track(images[c]) for c = 0..3 steps four flow lists per quad frame, and every new landmark
// takes its id from ONE counter in camera order.  Four single steps are twenty launches on a chain that is serial by the algorithm; here the five launches each take
// the camera as a grid dimension.  Camera c's lists, pyramids, keypoint row and detector scratch (its own score map, pool and count) are c strides behind camera 0's
struct LkFlowQuadArgs {
  LkFlowArgs c;                     // camera 0
  long list_stride;                 // words between the cameras' lists (previous and current)
  size_t pyr_stride;                // bytes between the cameras' pyramids (previous and current)
  size_t scratch_stride;            // bytes between the cameras' detector scratches
};
constexpr int FLOW_HDR_QUAD = 10;   // header word of CAMERA 0's current list: the quad-level arrival counter of launch 5 (a "rest 0" word of include/d2fe.h; left zero)

// launch 1, grid (cap_tracks / 4, 4): camera blockIdx.y's workgroups take that camera's ticket (header word 5 of ITS list); word 6 of every header is next_id BEFORE the
// quad frame, which is what four single steps leave when no camera detects
__global__ __launch_bounds__(256) void lk_flow_quad_step_kernel(LkFlowQuadArgs q) {
  flow_step_body(q.c, list_camera(q.c, blockIdx.y, q.list_stride, q.pyr_stride), blockIdx.x, gridDim.x);
}

// launches 2-4 over four cameras: fast_clear_kernel, fast_region_kernel and fast_nonmax_kernel with the camera as a grid dimension; each camera reads its OWN `num`
struct FastQuadArgs {
  const uint8_t* pyr; size_t pyr_stride;        // level 0 of camera 0's current pyramid
  const int* num; long list_stride;             // header word `num` of camera 0's current list
  int* score; int4* pool; int* count; size_t scratch_stride;
  int width, height, sw, sh, cols, rows, features, threshold, pool_cap, n4;
};
template <typename T>
__device__ __forceinline__ T* fast_quad_at(T* p, int cam, size_t stride) { return reinterpret_cast<T*>(reinterpret_cast<char*>(p) + (size_t)cam * stride); }

__global__ __launch_bounds__(256) void fast_quad_clear_kernel(FastQuadArgs a) {
  const int cam = blockIdx.y;
  if (a.num[(size_t)cam * a.list_stride] <= 0) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < a.n4) reinterpret_cast<int4*>(fast_quad_at(a.score, cam, a.scratch_stride))[i] = int4{0, 0, 0, 0};
  if (i == 0) fast_quad_at(a.count, cam, a.scratch_stride)[0] = 0;
}

__global__ __launch_bounds__(1024) void fast_quad_region_kernel(FastQuadArgs a) {
  const int cam = blockIdx.y;
  const int features = min(a.features, __builtin_amdgcn_readfirstlane(a.num[(size_t)cam * a.list_stride]));
  if (features <= 0) return;
  fast_region_body(a.pyr + (size_t)cam * a.pyr_stride, a.width, a.sw, a.sh, a.rows, features, a.threshold, fast_quad_at(a.score, cam, a.scratch_stride), a.width, blockIdx.x);
}

__global__ __launch_bounds__(256) void fast_quad_nonmax_kernel(FastQuadArgs a) {
  const int cam = blockIdx.z;
  if (a.num[(size_t)cam * a.list_stride] <= 0) return;
  fast_nonmax_body(fast_quad_at(a.score, cam, a.scratch_stride), a.width, a.height, a.sw, a.sh, a.cols, a.rows, fast_quad_at(a.pool, cam, a.scratch_stride), a.pool_cap,
                   fast_quad_at(a.count, cam, a.scratch_stride), blockIdx.x * 64 + (threadIdx.x & 63), blockIdx.y * 4 + (threadIdx.x >> 6));
}

// launch 5, four workgroups: workgroup c selects and merges for camera c (nothing when its `num` is 0), then the four take the quad-level ticket and the last one hands
// the ids out in camera order (quad_hand_out_ids, lk_list_device.h), as four single steps in camera order leave them
__global__ __launch_bounds__(1024) void lk_flow_quad_merge_kernel(LkFlowQuadArgs q) {
  __shared__ int s_last;
  float* cur0 = q.c.cur;
  int any = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) any |= reinterpret_cast<const int*>(cur0 + (size_t)k * q.list_stride)[FLOW_HDR_NUM] > 0 ? 1 : 0;
  if (!any) return;                 // the steady state: launch 1 left every header as four single steps do
  const FlowCamera v = flow_camera(q.c, blockIdx.x, q.list_stride, q.pyr_stride, q.scratch_stride);
  if (reinterpret_cast<const int*>(v.cur)[FLOW_HDR_NUM] > 0) flow_merge_body<true>(q.c, v);
  quad_hand_out_ids(cur0, q.list_stride, FLOW_HDR_QUAD, q.c.lay.off[D2FE_LKC_ID], q.c.next_id, &s_last);
}

const char* flow_check_geometry(int width, int height, int cap_tracks, int cols, int rows, int threshold) {
  if (width < 16 || height < 16 || (size_t)width * height > (1u << 28)) return "bad pyramid geometry";
  if (cap_tracks < 1 || cap_tracks > LKC_MAX) return "cap_tracks must be 1..1024";
  if (cols < 1 || rows < 1 || cols * rows > 64 || threshold < 0 || threshold > 254) return "bad FAST parameters (cols * rows 1..64, threshold 0..254)";
  if (width / cols < 7 || height / rows < 7) return "a FAST region must be at least 7 x 7";
  return nullptr;
}

// launches 2-5 of the step (score clear, FAST scores, non-max; the caller adds the selection) on level 0 of a pyramid; d_features is read on the device
void fast_device_launch(d2fe_context* h, const uint8_t* d_pyr, int width, int height, const int* d_features, int cap_tracks, int cols, int rows, int threshold,
                        const FlowScratch& f, hipStream_t s) {
  const int sw = width / cols, sh = height / rows;
  const int n4 = (int)(((size_t)width * height + 3) / 4);
  {
    ProfScope ps(h, D2FE_PROF_LK, s);
    hipLaunchKernelGGL(fast_clear_kernel, dim3((n4 + 255) / 256), dim3(256), 0, s, d_features, reinterpret_cast<int4*>(f.score), n4, f.count);
  }
  {
    ProfScope ps(h, D2FE_PROF_LK, s);
    hipLaunchKernelGGL(fast_region_kernel, dim3(cols * rows), dim3(1024), 0, s, d_pyr, width, sw, sh, rows, d_features, 2 * cap_tracks, threshold, f.score, width);
  }
  {
    ProfScope ps(h, D2FE_PROF_LK, s);
    hipLaunchKernelGGL(fast_nonmax_kernel, dim3((width + 63) / 64, (height + 3) / 4), dim3(256), 0, s, f.score, width, height, sw, sh, cols, rows, f.pool, f.pool_cap, f.count,
                       d_features);
  }
}

// launches 2-4 of the quad step: one grid each over the four cameras
void fast_quad_launch(d2fe_context* h, const FastQuadArgs& a, hipStream_t s) {
  {
    ProfScope ps(h, D2FE_PROF_LK, s);
    hipLaunchKernelGGL(fast_quad_clear_kernel, dim3((a.n4 + 255) / 256, 4), dim3(256), 0, s, a);
  }
  {
    ProfScope ps(h, D2FE_PROF_LK, s);
    hipLaunchKernelGGL(fast_quad_region_kernel, dim3(a.cols * a.rows, 4), dim3(1024), 0, s, a);
  }
  {
    ProfScope ps(h, D2FE_PROF_LK, s);
    hipLaunchKernelGGL(fast_quad_nonmax_kernel, dim3((a.width + 63) / 64, (a.height + 3) / 4, 4), dim3(256), 0, s, a);
  }
}

}  // namespace

hipStream_t ctx_stream(d2fe_handle h);
int ctx_device(d2fe_handle h);

const char* lk_flow_check_params(const d2fe_flow_params* fp, int width, int height) {
  if (!fp) return "null flow parameters";
  if (fp->struct_size != (int32_t)sizeof(d2fe_flow_params)) return "d2fe_flow_params.struct_size";
  if (const char* why = lk_carry_check_params(&fp->track)) return why;
  if (fp->superpoint != 0 && fp->superpoint != 1) return "superpoint must be 0 or 1";
  return flow_check_geometry(width, height, flow_cap_tracks(fp->track), fp->fast_cols, fp->fast_rows, fp->fast_threshold);
}

}  // namespace d2fe

using namespace d2fe;

extern "C" {

void d2fe_flow_default_params(d2fe_flow_params* fp) {
  if (!fp) return;
  fp->struct_size = (int32_t)sizeof(d2fe_flow_params);
  fp->superpoint = 1;
  d2fe_track_default_params(&fp->track);
  fp->fast_cols = 3; fp->fast_rows = 4; fp->fast_threshold = 10; fp->reserved = 0;
}

size_t d2fe_lk_flow_list_bytes(int cap_tracks) {
  if (cap_tracks < 1 || cap_tracks > LKC_MAX) return 0;
  return sizeof(float) * (size_t)carry_layout(cap_tracks, 0).words;
}

long d2fe_lk_flow_list_offset(int cap_tracks, int field) {
  if (cap_tracks < 1 || cap_tracks > LKC_MAX || field < 0 || field >= D2FE_LKC_FIELDS) return -1;
  return carry_layout(cap_tracks, 0).off[field];
}

size_t d2fe_lk_flow_scratch_bytes(int width, int height, int cap_tracks, int cols, int rows) {
  if (flow_check_geometry(width, height, cap_tracks, cols, rows, 0)) return 0;
  return flow_scratch(nullptr, width, height, cap_tracks, cols, rows).bytes;
}

int d2fe_detect_fast_device(d2fe_handle h, const uint8_t* d_pyr, int width, int height, const int32_t* d_features, int cap_tracks, int cols, int rows, int threshold,
                            float* d_xy, int32_t* d_response, int cap, int32_t* d_n, void* d_scratch, void* stream) {
  if (!h || !d_pyr || !d_features || !d_xy || !d_n || !d_scratch) return ctx_fail(D2FE_ERR_INVALID, "null argument");
  if (const char* why = flow_check_geometry(width, height, cap_tracks, cols, rows, threshold)) return ctx_fail(D2FE_ERR_INVALID, why);
  if (cap < 1 || ((uintptr_t)d_scratch & 15u)) return ctx_fail(D2FE_ERR_INVALID, "cap must be >= 1, the scratch 16-byte aligned");
  HIP_TRY(hipSetDevice(ctx_device(h)));
  hipStream_t s = stream ? (hipStream_t)stream : ctx_stream(h);
  const FlowScratch f = flow_scratch(d_scratch, width, height, cap_tracks, cols, rows);
  fast_device_launch(h, d_pyr, width, height, d_features, cap_tracks, cols, rows, threshold, f, s);
  {
    ProfScope ps(h, D2FE_PROF_LK, s);
    hipLaunchKernelGGL(fast_select_kernel, dim3(1), dim3(1024), 0, s, d_features, f.pool, f.count, f.pool_cap, 2 * cap_tracks, d_xy, d_response, cap, d_n);
  }
  HIP_TRY(hipGetLastError());
  return D2FE_OK;
}

namespace {
// what the two step entry points share: their refusals, the detector scratch of camera 0 and the kernel's arguments
int flow_step_args(d2fe_handle h, const uint8_t* d_prev_pyr, const uint8_t* d_cur_pyr, int width, int height, const void* d_prev, void* d_cur, const float* d_kps_xy,
                   const int32_t* d_n_kp, int kp_cap, const d2fe_flow_params* fp, int32_t* d_next_id, void* d_scratch, LkFlowArgs& c, FlowScratch& f, size_t* pyr_total) {
  if (!fp || !d_scratch) return ctx_fail(D2FE_ERR_INVALID, "null argument");
  if (const char* why = lk_flow_check_params(fp, width, height)) return ctx_fail(D2FE_ERR_INVALID, why);
  if ((uintptr_t)d_scratch & 15u) return ctx_fail(D2FE_ERR_INVALID, "the scratch must be 16-byte aligned");
  const CarryLayout lay = list_layout(fp->track, 0);
  f = flow_scratch(d_scratch, width, height, lay.cap, fp->fast_cols, fp->fast_rows);
  c.pool = f.pool; c.count = f.count; c.pool_cap = f.pool_cap;
  return list_step_args(h, d_prev_pyr, d_cur_pyr, width, height, d_prev, d_cur, lay, d_kps_xy, d_n_kp, kp_cap, fp->superpoint != 0, fp->track, d_next_id, c, pyr_total);
}
}  // namespace

int d2fe_lk_flow_step_device(d2fe_handle h, const uint8_t* d_prev_pyr, const uint8_t* d_cur_pyr, int width, int height, const void* d_prev_list, void* d_cur_list,
                             const float* d_kps_xy, const int32_t* d_n_kp, int kp_cap, const d2fe_flow_params* fp, int32_t* d_next_id, void* d_scratch, void* stream) {
  LkFlowArgs c{};
  FlowScratch f{};
  if (const int rc = flow_step_args(h, d_prev_pyr, d_cur_pyr, width, height, d_prev_list, d_cur_list, d_kps_xy, d_n_kp, kp_cap, fp, d_next_id, d_scratch, c, f, nullptr)) return rc;
  const int cap_tracks = c.lay.cap;
  HIP_TRY(hipSetDevice(ctx_device(h)));
  hipStream_t s = stream ? (hipStream_t)stream : ctx_stream(h);
  {
    ProfScope ps(h, D2FE_PROF_LK, s);
    hipLaunchKernelGGL(lk_flow_step_kernel, dim3((cap_tracks + 3) / 4), dim3(256), 0, s, c);
  }
  // detectFastByRegion(img, num, cols = fast_rows', rows = fast_cols'): the caller's fast_cols / fast_rows are already the detector's cols / rows (3, 4)
  const int* d_num = reinterpret_cast<const int*>(d_cur_list) + FLOW_HDR_NUM;
  fast_device_launch(h, d_cur_pyr, width, height, d_num, cap_tracks, fp->fast_cols, fp->fast_rows, fp->fast_threshold, f, s);
  {
    ProfScope ps(h, D2FE_PROF_LK, s);
    hipLaunchKernelGGL(lk_flow_merge_kernel, dim3(1), dim3(1024), 0, s, c);
  }
  HIP_TRY(hipGetLastError());
  return D2FE_OK;
}

int d2fe_lk_flow_quad_step_device(d2fe_handle h, const uint8_t* d_prev_pyr, const uint8_t* d_cur_pyr, size_t pyr_stride, int width, int height, const void* d_prev_lists,
                                  void* d_cur_lists, size_t list_stride, const float* d_kps_xy, const int32_t* d_n_kp, int kp_cap, const d2fe_flow_params* fp,
                                  int32_t* d_next_id, void* d_scratch, size_t scratch_stride, void* stream) {
  LkFlowQuadArgs q{};
  LkFlowArgs& c = q.c;
  FlowScratch f{};
  size_t total = 0;
  if (const int rc = flow_step_args(h, d_prev_pyr, d_cur_pyr, width, height, d_prev_lists, d_cur_lists, d_kps_xy, d_n_kp, kp_cap, fp, d_next_id, d_scratch, c, f, &total)) return rc;
  if (const int rc = list_quad_check(c, list_stride, pyr_stride, total)) return rc;
  if ((scratch_stride & 15u) || scratch_stride < f.bytes || scratch_stride > (1ul << 40))
    return ctx_fail(D2FE_ERR_INVALID, "the scratch must be 16-byte aligned, scratch_stride (bytes) a multiple of 16 and at least d2fe_lk_flow_scratch_bytes");
  const int cap_tracks = c.lay.cap;
  q.list_stride = (long)list_stride; q.pyr_stride = pyr_stride; q.scratch_stride = scratch_stride;
  HIP_TRY(hipSetDevice(ctx_device(h)));
  hipStream_t s = stream ? (hipStream_t)stream : ctx_stream(h);
  {
    ProfScope ps(h, D2FE_PROF_LK, s);
    hipLaunchKernelGGL(lk_flow_quad_step_kernel, dim3((cap_tracks + 3) / 4, 4), dim3(256), 0, s, q);
  }
  FastQuadArgs a{};
  a.pyr = d_cur_pyr; a.pyr_stride = pyr_stride;
  a.num = reinterpret_cast<const int*>(d_cur_lists) + FLOW_HDR_NUM; a.list_stride = (long)list_stride;
  a.score = f.score; a.pool = f.pool; a.count = f.count; a.scratch_stride = scratch_stride;
  a.width = width; a.height = height; a.sw = width / fp->fast_cols; a.sh = height / fp->fast_rows; a.cols = fp->fast_cols; a.rows = fp->fast_rows;
  a.features = 2 * cap_tracks; a.threshold = fp->fast_threshold; a.pool_cap = f.pool_cap; a.n4 = (int)(((size_t)width * height + 3) / 4);
  fast_quad_launch(h, a, s);
  {
    ProfScope ps(h, D2FE_PROF_LK, s);
    hipLaunchKernelGGL(lk_flow_quad_merge_kernel, dim3(4), dim3(1024), 0, s, q);
  }
  HIP_TRY(hipGetLastError());
  return D2FE_OK;
}

}  // extern "C"
