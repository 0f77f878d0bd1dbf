// lk_list_device.h -- what the two landmark lists of D2FeatureTracker::trackLK(frame) share: the block layout and its capacity rule, the kernel arguments both lists
// carry (LkListArgs) and the per-camera view of them (ListCamera), the distance test of cv::norm, step a with the per-list ticket (list_track_and_arrive), steps b-c
// (list_reduce_prune: reduceVector, removeNearPoints), the quad-level ticket with the id hand-out in camera order (quad_hand_out_ids), and on the host the refusals and
// the argument assignments of the step entry points (list_step_args, list_quad_check).  lk_carry.hip (the LK-carried SuperPoint list of sp_track_use_lk) and lk_flow.hip
// (the FAST-replenished flow list) include it; each replenishes in its own way.  Internal.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/d2fe.h"
#include "context.h"
#include "lk_device.h"

namespace d2fe {
namespace {

constexpr int LKC_MAX = 1024;      // cap_tracks the finishing workgroup's LDS is sized for

// list block layout (words from the block base; include/d2fe.h).  D = 0: a flow list, which has no KP, SCORES and DESC arrays (offset -1)
struct CarryLayout {
  int cap, D;
  long off[D2FE_LKC_FIELDS];
  long words;
};
__host__ __device__ inline long lkc_up64(long w) { return (w + 63) / 64 * 64; }
inline CarryLayout carry_layout(int cap, int D) {
  CarryLayout l{};
  l.cap = cap; l.D = D;
  long o = 0;
  l.off[D2FE_LKC_HDR] = o; o += 64;
  l.off[D2FE_LKC_PTS] = o; o += lkc_up64(2L * cap);
  l.off[D2FE_LKC_ID] = o; o += lkc_up64(cap);
  l.off[D2FE_LKC_SRC] = o; o += lkc_up64(cap);
  l.off[D2FE_LKC_KP] = l.off[D2FE_LKC_SCORES] = l.off[D2FE_LKC_DESC] = -1;
  if (D > 0) {
    l.off[D2FE_LKC_KP] = o; o += lkc_up64(cap);
    l.off[D2FE_LKC_SCORES] = o; o += lkc_up64(cap);
    l.off[D2FE_LKC_DESC] = o; o += lkc_up64((long)cap * D);
  }
  l.off[D2FE_LKC_TRK_XY] = o; o += lkc_up64(2L * cap);
  l.off[D2FE_LKC_TRK_STATUS] = o; o += lkc_up64((cap + 3) / 4);
  l.words = o;
  return l;
}
// the capacity rule: a list with descriptors holds total_feature_num + 1 entries (the replenish loop overshoots by one), a flow list (desc_dim = 0) flow_cap_tracks
inline CarryLayout list_layout(const d2fe_track_params& tp, int desc_dim) {
  return desc_dim > 0 ? carry_layout(tp.total_feature_num + 1, desc_dim) : carry_layout(flow_cap_tracks(tp), 0);
}

// what the step kernels of both lists take: LkCarryArgs and LkFlowArgs extend it.  In the quad forms the pointers are camera 0's
struct LkListArgs {
  const uint8_t* prev_pyr; const uint8_t* cur_pyr;
  LkPairDev P;                      // geometry only
  int win, iters;
  const float* prev; float* cur;    // list blocks
  CarryLayout lay;
  const float* kps; const int* n_kp; int kp_cap;      // kp_cap = 0: no SuperPoint keypoints
  int total;                        // total_feature_num
  double near_thr, min_dist;        // near_lk_thread_rate widened to double; feature_min_dist
  int* next_id;
};

// what differs per camera and nothing else; the geometry, the layout and the scalars are read from the kernel's arguments
struct ListCamera {
  const uint8_t* prev_pyr; const uint8_t* cur_pyr;
  const float* prev; float* cur;
  const float* kps; const int* n_kp;
};
// camera `cam` of a quad step: its lists and pyramids are cam strides behind camera 0's, its keypoints row cam of the dense [4][kp_cap] extract outputs.  (c, 0, 0, 0): the single step
__device__ __forceinline__ ListCamera list_camera(const LkListArgs& c, int cam, long list_stride, size_t pyr_stride) {
  ListCamera v{c.prev_pyr + (size_t)cam * pyr_stride, c.cur_pyr + (size_t)cam * pyr_stride, c.prev + (size_t)cam * list_stride, c.cur + (size_t)cam * list_stride, c.kps, c.n_kp};
  if (c.kp_cap > 0) { v.kps += (size_t)cam * c.kp_cap * 2; v.n_kp += cam; }
  return v;
}
__device__ __forceinline__ int list_n_kp(const LkListArgs& c, const ListCamera& v) {
  int n_kp = c.kp_cap > 0 ? __builtin_amdgcn_readfirstlane(v.n_kp[0]) : 0;
  return n_kp < 0 ? 0 : n_kp > c.kp_cap ? c.kp_cap : n_kp;
}

// cv::norm(a - b) < thr for Point2f a, b: float differences, sqrt((double)dx * dx + (double)dy * dy) < thr.  The products are exact in double and the sum is rounded once,
// so s is the reference's number whatever its compiler contracts.  sqrt is correctly rounded and monotonic: s >= thr^2 (real) gives sqrt(s) >= thr, and an s below
// thr^2 by more than a few ulps cannot round up to thr -- only the band around thr^2 needs the double-precision square root itself
__device__ __forceinline__ bool nearer(float ax, float ay, float bx, float by, double thr, double lo, double hi) {
  const float dx = ax - bx, dy = ay - by;
  const double s = (double)dx * (double)dx + (double)dy * (double)dy;
  if (s < lo) return true;
  if (s > hi) return false;
  return __builtin_sqrt(s) < thr;
}

// LDS writes of one lane, read by the other lanes of the SAME wave in the next step: the wave runs in lockstep and its LDS operations complete in order; this keeps
// the compiler from moving accesses across the point
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Steps b and c on ONE wave, for the workgroup that arrived last: the tracker's raw output for the n_prev entries of the previous list (other workgroups' stores,
// behind the caller's agent-scope acquire) is compacted by status into s_x / s_y / s_src (src = index in the previous list), then thinned in place by
// removeNearPoints(near_thr).  cnt = the survivors of b, the return value m = the survivors of c, which are entries 0 .. m - 1
__device__ __forceinline__ int list_reduce_prune(const float* trk_xy, const uint8_t* trk_st, int n_prev, double near_thr, float* s_x, float* s_y, int* s_src, int lane,
                                                 int& cnt) {
  // b. reduceVector: order-preserving compaction by status, 64 entries a round
  cnt = 0;
  for (int base = 0; base < n_prev; base += 64) {
    const int i = base + lane;
    bool ok = false;
    float x = 0.f, y = 0.f;
    if (i < n_prev) {
      ok = __hip_atomic_load(trk_st + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
      x = __hip_atomic_load(trk_xy + 2 * i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      y = __hip_atomic_load(trk_xy + 2 * i + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const unsigned long long bal = __ballot(ok);
    if (ok) {
      const int k = cnt + __popcll(bal & ((1ull << lane) - 1ull));
      s_x[k] = x; s_y[k] = y; s_src[k] = i;
    }
    cnt += __popcll(bal);
  }
  wave_lds_sync();
  // c. removeNearPoints, in place (the kept prefix never passes the candidate)
  int m = 0;
  const double thr = near_thr, t2 = thr * thr, lo = t2 * (1.0 - 1e-12), hi = t2 * (1.0 + 1e-12);
  for (int i = 0; i < cnt; ++i) {
    const float px = s_x[i], py = s_y[i];
    const int src = s_src[i];
    bool hit = false;
    for (int j = lane; j < m; j += 64) hit = hit || nearer(px, py, s_x[j], s_y[j], thr, lo, hi);
    if (__ballot(hit) == 0ull) {
      wave_lds_sync();        // every lane has read entry i before slot m <= i is rewritten
      if (lane == 0) { s_x[m] = px; s_y[m] = py; s_src[m] = src; }
      ++m;
      wave_lds_sync();
    }
  }
  return m;
}

// Step a and the per-list ticket (the pattern of match.hip), for workgroup bx of the nblocks that step this list: one 64-lane wave per entry of the previous list runs
// the bidirectional track (the body of lk_track_stereo_kernel, lk.hip) into the current list's TRK arrays; every workgroup then takes an agent-scope ticket in header
// word 5 of the current list.  true: this workgroup arrived last, has acquired everybody's stores and finishes the list; the word is zero again for the next launch
// that writes this block.  s_last: one LDS word
__device__ __forceinline__ bool list_track_and_arrive(const LkListArgs& c, const ListCamera& v, int bx, int nblocks, int* s_last, int& n_prev) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int* hdr = reinterpret_cast<int*>(v.cur);
  n_prev = __builtin_amdgcn_readfirstlane(reinterpret_cast<const int*>(v.prev)[0]);
  n_prev = n_prev < 0 ? 0 : n_prev > c.lay.cap ? c.lay.cap : n_prev;
  const int slot = bx * 4 + wave;
  if (slot < n_prev) {
    float* trk_xy = v.cur + c.lay.off[D2FE_LKC_TRK_XY];
    uint8_t* trk_st = reinterpret_cast<uint8_t*>(v.cur + c.lay.off[D2FE_LKC_TRK_STATUS]);
    const float* ppts = v.prev + c.lay.off[D2FE_LKC_PTS];
    LkArgs a{};
    a.win = c.win; a.iters = c.iters;
    const float ppx = ppts[2 * slot], ppy = ppts[2 * slot + 1];
    float cx, cy;
    const int ok = lk_bidir(a, c.P, v.prev_pyr, v.cur_pyr, ppx, ppy, cx, cy, lane);
    if (lane == 0) { trk_xy[2 * slot] = cx; trk_xy[2 * slot + 1] = cy; trk_st[slot] = (uint8_t)ok; }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");      // the wave's stores have left before its workgroup arrives
  }
  __syncthreads();
  if (tid == 0) {
    const int old = __hip_atomic_fetch_add(hdr + 5, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    const int last = old == nblocks - 1;
    if (last) __hip_atomic_store(hdr + 5, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *s_last = last;
  }
  __syncthreads();
  if (!*s_last) return false;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  return true;
}

// The quad-level ticket and the ids, for a workgroup that has finished its camera's list (every thread of it calls): the list has left before the workgroup arrives
// at header word `word` of CAMERA 0's current list cur0 (zero between launches, like word 5); the last of the four reads the four counts of new entries and hands the
// ids out -- camera c's k-th new entry gets *next_id + (new entries of cameras < c) + k, header word 6 of camera c is next_id after that camera, as four single steps
// in camera order leave them.  The workgroups can sit on different XCDs: agent-scope release / acquire around the ticket.  s_last: one LDS word
__device__ __forceinline__ void quad_hand_out_ids(float* cur0, long list_stride, int word, long off_id, int* next_id, int* s_last) {
  const int tid = threadIdx.x;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  __syncthreads();
  int* qt = reinterpret_cast<int*>(cur0) + word;
  if (tid == 0) {
    const int old = __hip_atomic_fetch_add(qt, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    const int last = old == 3;
    if (last) __hip_atomic_store(qt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *s_last = last;
  }
  __syncthreads();
  if (!*s_last) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  int base = *next_id;
  for (int k = 0; k < 4; ++k) {
    int* h = reinterpret_cast<int*>(cur0 + (size_t)k * list_stride);
    const int len = __hip_atomic_load(h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), fresh = __hip_atomic_load(h + 4, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    int* id = h + off_id;
    for (int e = len - fresh + tid; e < len; e += blockDim.x) id[e] = base + (e - (len - fresh));
    base += fresh;
    if (tid == 0) h[6] = base;
  }
  __syncthreads();       // every thread has read *next_id
  if (tid == 0) *next_id = base;
}

// the pyramid of a d2fe_lk_frame / one image of the stereo workspace: levels + 1 tight images one after the other
inline void lk_pyr_geometry(LkPairDev& P, int width, int height, int levels, size_t* total) {
  int o = 0;
  for (int l = 0, w = width, hh = height; l <= levels; ++l) { P.off[l] = o; P.ws[l] = w; P.hs[l] = hh; o += w * hh; w = (w + 1) / 2; hh = (hh + 1) / 2; }
  P.levels = levels; P.w = width; P.h = height; P.type = 0; P.move_cols = 0.f;
  if (total) *total = (size_t)o;
}

// ---- the host side of the step entry points ----------------------------------------------------------------------------------------------------------------
// What d2fe_lk_carry_step_device, d2fe_lk_flow_step_device and their quad forms refuse alike (after their own parameter checks), and the kernel arguments they share.
// use_kps = false: the step reads no keypoints whatever kp_cap says (a flow list without SuperPoint).  pyr_total: the bytes of one pyramid
inline int list_step_args(d2fe_handle h, const uint8_t* d_prev_pyr, const uint8_t* d_cur_pyr, int width, int height, const void* d_prev, void* d_cur, const CarryLayout& lay,
                          const float* d_kps_xy, const int32_t* d_n_kp, int kp_cap, bool use_kps, const d2fe_track_params& tp, int32_t* d_next_id, LkListArgs& c,
                          size_t* pyr_total) {
  if (!h || !d_prev_pyr || !d_cur_pyr || !d_prev || !d_cur || !d_next_id) return ctx_fail(D2FE_ERR_INVALID, "null argument");
  if (d_prev == d_cur) return ctx_fail(D2FE_ERR_INVALID, "the previous and the current list must be different blocks");
  if (width < 16 || height < 16 || (size_t)width * height > (1u << 28)) return ctx_fail(D2FE_ERR_INVALID, "bad pyramid geometry");
  if (kp_cap < 0 || kp_cap > 16384) return ctx_fail(D2FE_ERR_INVALID, "kp_cap must be 0..16384");
  if (!use_kps) kp_cap = 0;
  if (kp_cap > 0 && (!d_kps_xy || !d_n_kp)) return ctx_fail(D2FE_ERR_INVALID, "null keypoint arrays with kp_cap > 0");
  lk_pyr_geometry(c.P, width, height, tp.levels, pyr_total);
  c.prev_pyr = d_prev_pyr; c.cur_pyr = d_cur_pyr; c.win = tp.win; c.iters = tp.iters;
  c.prev = static_cast<const float*>(d_prev); c.cur = static_cast<float*>(d_cur);
  c.lay = lay;
  c.kps = d_kps_xy; c.n_kp = d_n_kp; c.kp_cap = kp_cap;
  c.total = tp.total_feature_num; c.near_thr = (double)tp.near_lk_thread_rate; c.min_dist = tp.feature_min_dist;
  c.next_id = d_next_id;
  return D2FE_OK;
}

// the quad forms only: the strides, and the four previous lists against the four current ones -- no block may be both
inline int list_quad_check(const LkListArgs& c, size_t list_stride, size_t pyr_stride, size_t pyr_total) {
  if (list_stride < (size_t)c.lay.words || list_stride > (1ul << 40))
    return ctx_fail(D2FE_ERR_INVALID, c.lay.D > 0 ? "list_stride (words) must be at least one list block" : "list_stride (words) must be at least one flow list block");
  if (pyr_stride < pyr_total) return ctx_fail(D2FE_ERR_INVALID, "pyr_stride (bytes) must be at least one pyramid");
  const char* a = reinterpret_cast<const char*>(c.prev); const char* b = reinterpret_cast<const char*>(c.cur);
  const size_t span = sizeof(float) * (3 * list_stride + (size_t)c.lay.words);
  if (a < b + span && b < a + span) return ctx_fail(D2FE_ERR_INVALID, "the previous and the current lists must not overlap");
  return D2FE_OK;
}

}  // namespace
}  // namespace d2fe
