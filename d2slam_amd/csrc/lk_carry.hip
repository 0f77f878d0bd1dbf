// lk_carry.hip -- the LK-carried landmark list of sp_track_use_lk on the device (include/d2fe.h, d2fe_lk_carry_step_device).
//   D2FeatureTracker::trackLK(frame)   d2frontend/src/d2featuretracker.cpp:472-621: track the previous list (opticalflowTrackPyr, opticaltrack_utils.cpp:173-279),
//                                      reduceVector (:273-276), removeNearPoints (opticaltrack_utils.h:61-89), copy the descriptors of the survivors (:509-521),
//                                      replenish from the frame's SuperPoint keypoints (:556-589)
//   trackLK(left, right)               :697-752 with sp_track_use_lk: the LIST entries (not the SuperPoint keypoints) are tracked left -> right
//
// MI355X mapping.  One frame = ONE launch (lk_carry_step_kernel): one 64-lane wave per list slot runs the bidirectional track (lk_bidir over lk.hip's lk_calc, lk_device.h), four
// waves to a workgroup; every workgroup then takes an agent-scope ticket in the output list's header and the last one to arrive runs steps b-e for the whole list.  The
// alternative, a second launch of one workgroup, puts one more dependent launch per frame on a chain that is serial by the algorithm (frame f + 1 needs frame f's
// list), against one atomic per workgroup here; the gap between two dependent launches was not measured for this kernel, and the
// two-launch form was not built.
// Steps b-d are sequential over at most cap_tracks (prune) and cap (replenish) candidates, each with a parallel distance test against the kept entries.  They run on
// ONE wave with the list in LDS: a candidate is tested by the 64 lanes against entries lane, lane + 64, ... and a ballot decides, so a step costs a few LDS reads and no
// workgroup barrier (a 256-thread version would need barriers around every candidate; not built, not measured).  Step e (ids, descriptor rows, zero fill) is parallel over the
// workgroup's four waves.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/d2fe.h"
#include "context.h"
#include "kernels.h"
#include "lk_device.h"

namespace d2fe {

namespace {

constexpr int LKC_MAX = 1024;      // cap_tracks the finishing workgroup's LDS is sized for

// list block layout (words from the block base; include/d2fe.h)
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
  l.off[D2FE_LKC_KP] = o; o += lkc_up64(cap);
  l.off[D2FE_LKC_SCORES] = o; o += lkc_up64(cap);
  l.off[D2FE_LKC_DESC] = o; o += lkc_up64((long)cap * D);
  l.off[D2FE_LKC_TRK_XY] = o; o += lkc_up64(2L * cap);
  l.off[D2FE_LKC_TRK_STATUS] = o; o += lkc_up64((cap + 3) / 4);
  l.words = o;
  return l;
}

struct LkCarryArgs {
  const uint8_t* prev_pyr; const uint8_t* cur_pyr;
  LkPairDev P;                      // geometry only
  int win, iters;
  const float* prev; float* cur;    // list blocks
  CarryLayout lay;
  const float* kps; const float* kp_scores; const float* kp_desc; const int* n_kp; int kp_cap;
  int total;                        // total_feature_num
  double near_thr, min_dist;        // near_lk_thread_rate widened to double; feature_min_dist
  int* next_id;
};

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

__global__ __launch_bounds__(256) void lk_carry_step_kernel(LkCarryArgs c) {
  __shared__ float s_x[LKC_MAX], s_y[LKC_MAX];
  __shared__ int s_src[LKC_MAX], s_kp[LKC_MAX];
  __shared__ int s_cnt[4];          // [0] list length, [1] survivors of the tracker, [2] survivors of removeNearPoints, [3] this workgroup arrived last
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cap = c.lay.cap, D = c.lay.D;
  const int* phdr = reinterpret_cast<const int*>(c.prev);
  int* hdr = reinterpret_cast<int*>(c.cur);
  float* trk_xy = c.cur + c.lay.off[D2FE_LKC_TRK_XY];
  uint8_t* trk_st = reinterpret_cast<uint8_t*>(c.cur + c.lay.off[D2FE_LKC_TRK_STATUS]);
  const float* ppts = c.prev + c.lay.off[D2FE_LKC_PTS];
  int n_prev = __builtin_amdgcn_readfirstlane(phdr[0]);
  n_prev = n_prev < 0 ? 0 : n_prev > cap ? cap : n_prev;

  // ---- a. track: one wave per entry of the previous list (the body of lk_track_stereo_kernel, lk.hip)
  const int slot = blockIdx.x * 4 + wave;
  if (slot < n_prev) {
    LkArgs a{};
    a.win = c.win; a.iters = c.iters;
    const LkPairDev& P = c.P;
    const float ppx = ppts[2 * slot], ppy = ppts[2 * slot + 1];
    float cx, cy;
    const int ok = lk_bidir(a, P, c.prev_pyr, c.cur_pyr, ppx, ppy, cx, cy, lane);
    if (lane == 0) { trk_xy[2 * slot] = cx; trk_xy[2 * slot + 1] = cy; trk_st[slot] = (uint8_t)ok; }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");      // the wave's stores have left before its workgroup arrives
  }
  // ---- ticket (the pattern of match.hip): the last workgroup to arrive acquires everybody's stores and finishes the list
  __syncthreads();
  if (tid == 0) {
    const int old = __hip_atomic_fetch_add(hdr + 5, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    const int last = old == (int)gridDim.x - 1;
    if (last) __hip_atomic_store(hdr + 5, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // ready for the next launch that writes this block
    s_cnt[3] = last;
  }
  __syncthreads();
  if (!s_cnt[3]) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");

  // ---- b-d on wave 0
  if (wave == 0) {
    // b. reduceVector: order-preserving compaction by status, 64 entries a round
    int cnt = 0;
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
        s_x[k] = x; s_y[k] = y; s_src[k] = i; s_kp[k] = -1;
      }
      cnt += __popcll(bal);
    }
    wave_lds_sync();
    // c. removeNearPoints, in place (the kept prefix never passes the candidate)
    int m = 0;
    {
      const double thr = c.near_thr, t2 = thr * thr, lo = t2 * (1.0 - 1e-12), hi = t2 * (1.0 + 1e-12);
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
    }
    // d. replenish from the frame's SuperPoint keypoints
    int len = m;
    {
      int n_kp = c.kp_cap > 0 ? __builtin_amdgcn_readfirstlane(c.n_kp[0]) : 0;
      n_kp = n_kp < 0 ? 0 : n_kp > c.kp_cap ? c.kp_cap : n_kp;
      const double thr = c.min_dist, t2 = thr * thr, lo = t2 * (1.0 - 1e-12), hi = t2 * (1.0 + 1e-12);
      for (int i = 0; i < n_kp; ++i) {
        if (len > c.total) break;
        const float kx = c.kps[2 * i], ky = c.kps[2 * i + 1];
        bool hit = false;
        for (int j = lane; j < len; j += 64) hit = hit || nearer(s_x[j], s_y[j], kx, ky, thr, lo, hi);
        if (__ballot(hit) == 0ull) {
          if (lane == 0) { s_x[len] = kx; s_y[len] = ky; s_src[len] = -1; s_kp[len] = i; }
          ++len;
          wave_lds_sync();
        }
      }
    }
    if (lane == 0) { s_cnt[0] = len; s_cnt[1] = cnt; s_cnt[2] = m; }
  }
  __syncthreads();
  // ---- e. the list: ids, descriptors and scores of the discovery frame, zeros behind the end
  const int len = s_cnt[0], cnt = s_cnt[1], m = s_cnt[2];
  const int id0 = *c.next_id;
  float* pts = c.cur + c.lay.off[D2FE_LKC_PTS];
  int* id = reinterpret_cast<int*>(c.cur + c.lay.off[D2FE_LKC_ID]);
  int* src = reinterpret_cast<int*>(c.cur + c.lay.off[D2FE_LKC_SRC]);
  int* kp = reinterpret_cast<int*>(c.cur + c.lay.off[D2FE_LKC_KP]);
  float* scores = c.cur + c.lay.off[D2FE_LKC_SCORES];
  float* desc = c.cur + c.lay.off[D2FE_LKC_DESC];
  const int* pid = reinterpret_cast<const int*>(c.prev + c.lay.off[D2FE_LKC_ID]);
  const float* pscores = c.prev + c.lay.off[D2FE_LKC_SCORES];
  const float* pdesc = c.prev + c.lay.off[D2FE_LKC_DESC];
  for (int k = tid; k < cap; k += 256) {
    const bool live = k < len, old = k < m;
    const int sk = live ? s_src[k] : 0, kk = live ? s_kp[k] : 0;
    pts[2 * k] = live ? s_x[k] : 0.f; pts[2 * k + 1] = live ? s_y[k] : 0.f;
    id[k] = !live ? 0 : old ? pid[sk] : id0 + (k - m);
    src[k] = sk; kp[k] = kk;
    scores[k] = !live ? 0.f : old ? pscores[sk] : c.kp_scores[kk];
    if (k >= n_prev) { trk_xy[2 * k] = 0.f; trk_xy[2 * k + 1] = 0.f; trk_st[k] = 0; }
  }
  for (int k = wave; k < cap; k += 4) {          // a descriptor row per wave
    float* dst = desc + (size_t)k * D;
    if (k < len) {
      const float* from = k < m ? pdesc + (size_t)s_src[k] * D : c.kp_desc + (size_t)s_kp[k] * D;
      for (int e = lane; e < D; e += 64) dst[e] = from[e];
    } else {
      for (int e = lane; e < D; e += 64) dst[e] = 0.f;
    }
  }
  __syncthreads();       // every thread has read *next_id
  if (tid == 0) {
    hdr[0] = len; hdr[1] = n_prev; hdr[2] = n_prev - cnt; hdr[3] = cnt - m; hdr[4] = len - m;
    hdr[6] = id0 + (len - m);
    *c.next_id = id0 + (len - m);
  }
  if (tid >= 7 && tid < 64) hdr[tid] = 0;
}

// trackLK(left, right) on the lists of a pass: one wave per (frame, list slot); frame f's list is f * list_words further on, its pyramids are images f and n_frames + f
// of the stereo workspace.  Slots >= n are written too (status 0, point (0, 0)), as lk_track_stereo_kernel does
struct LkCarryRightArgs {
  const uint8_t* ws; size_t total;
  LkPairDev P;
  int n_frames, cap, win, iters;
  const float* lists; long list_words, off_pts;
  float* cur_pts; uint8_t* status;
};

__global__ __launch_bounds__(256) void lk_carry_right_kernel(LkCarryRightArgs s) {
  const int lane = threadIdx.x & 63;
  const int slot = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), f = blockIdx.y;
  if (slot >= s.cap) return;
  const size_t i = (size_t)f * s.cap + slot;
  const float* list = s.lists + (size_t)f * s.list_words;
  if (slot >= reinterpret_cast<const int*>(list)[0]) {
    if (lane == 0) { s.cur_pts[2 * i] = 0.f; s.cur_pts[2 * i + 1] = 0.f; s.status[i] = 0; }
    return;
  }
  LkArgs a{};
  a.win = s.win; a.iters = s.iters;
  const LkPairDev& P = s.P;
  const uint8_t* L = s.ws + (size_t)f * s.total;
  const uint8_t* R = s.ws + (size_t)(s.n_frames + f) * s.total;
  const float ppx = list[s.off_pts + 2 * slot], ppy = list[s.off_pts + 2 * slot + 1];
  float cx, cy;
  const int ok = lk_bidir(a, P, L, R, ppx, ppy, cx, cy, lane);
  if (lane == 0) {
    s.cur_pts[2 * i] = cx; s.cur_pts[2 * i + 1] = cy;
    s.status[i] = (uint8_t)ok;
  }
}

void pyr_geometry(LkPairDev& P, int width, int height, int levels, size_t* total) {
  int o = 0;
  for (int l = 0, w = width, hh = height; l <= levels; ++l) { P.off[l] = o; P.ws[l] = w; P.hs[l] = hh; o += w * hh; w = (w + 1) / 2; hh = (hh + 1) / 2; }
  P.levels = levels; P.w = width; P.h = height; P.type = 0; P.move_cols = 0.f;
  if (total) *total = (size_t)o;
}

}  // namespace

hipStream_t ctx_stream(d2fe_handle h);
int ctx_device(d2fe_handle h);

// what d2fe_lk_carry_step_device refuses, as a message (nullptr: fine); also the check of d2fe_pipe_set_track_params
const char* lk_carry_check_params(const d2fe_track_params* tp) {
  if (!tp) return "null track parameters";
  if (tp->total_feature_num < 0 || tp->total_feature_num + 1 > LKC_MAX) return "total_feature_num + 1 (cap_tracks) must be 1..1024";
  if (tp->levels < 0 || tp->levels > 7 || tp->win < 3 || tp->win > 24 || !(tp->win & 1) || tp->iters < 1) return "bad LK parameters (levels 0..7, win odd 3..23, iters >= 1)";
  if (!(tp->near_lk_thread_rate >= 0.f) || !(tp->feature_min_dist >= 0.0)) return "near_lk_thread_rate and feature_min_dist must be >= 0";
  return nullptr;
}

// the pipe's form of trackLK(left, right): the lists of n_frames consecutive frames (list_words apart) against the stereo workspace of the pass, ONE launch
int lk_carry_right_launch(d2fe_context* h, const uint8_t* ws, int n_frames, int width, int height, const d2fe_track_params& tp, const float* d_lists, int desc_dim,
                          float* d_right_xy, uint8_t* d_right_status, hipStream_t s) {
  LkCarryRightArgs r{};
  pyr_geometry(r.P, width, height, tp.levels, &r.total);
  const CarryLayout lay = carry_layout(tp.total_feature_num + 1, desc_dim);
  r.ws = ws; r.n_frames = n_frames; r.cap = lay.cap; r.win = tp.win; r.iters = tp.iters;
  r.lists = d_lists; r.list_words = lay.words; r.off_pts = lay.off[D2FE_LKC_PTS];
  r.cur_pts = d_right_xy; r.status = d_right_status;
  {
    ProfScope ps(h, D2FE_PROF_LK, s);
    hipLaunchKernelGGL(lk_carry_right_kernel, dim3((lay.cap + 3) / 4, n_frames), dim3(256), 0, s, r);
  }
  HIP_TRY(hipGetLastError());
  return D2FE_OK;
}

}  // namespace d2fe

using namespace d2fe;

extern "C" {

void d2fe_track_default_params(d2fe_track_params* tp) {
  if (!tp) return;
  tp->total_feature_num = 150; tp->levels = 2; tp->win = 21; tp->iters = 30;
  tp->near_lk_thread_rate = 5.0f; tp->reserved = 0; tp->feature_min_dist = 20.0;
}

size_t d2fe_lk_carry_list_bytes(int cap_tracks, int desc_dim) {
  if (cap_tracks < 1 || cap_tracks > LKC_MAX || desc_dim < 1 || desc_dim > 65536) return 0;
  return sizeof(float) * (size_t)carry_layout(cap_tracks, desc_dim).words;
}

long d2fe_lk_carry_list_offset(int cap_tracks, int desc_dim, int field) {
  if (cap_tracks < 1 || cap_tracks > LKC_MAX || desc_dim < 1 || desc_dim > 65536 || field < 0 || field >= D2FE_LKC_FIELDS) return -1;
  return carry_layout(cap_tracks, desc_dim).off[field];
}

int d2fe_lk_carry_step_device(d2fe_handle h, const uint8_t* d_prev_pyr, const uint8_t* d_cur_pyr, int width, int height, const void* d_prev_list, void* d_cur_list,
                              int desc_dim, const float* d_kps_xy, const float* d_kp_scores, const float* d_kp_desc, const int32_t* d_n_kp, int kp_cap,
                              const d2fe_track_params* tp, int32_t* d_next_id, void* stream) {
  if (!h || !d_prev_pyr || !d_cur_pyr || !d_prev_list || !d_cur_list || !tp || !d_next_id) return ctx_fail(D2FE_ERR_INVALID, "null argument");
  if (const char* why = lk_carry_check_params(tp)) return ctx_fail(D2FE_ERR_INVALID, why);
  if (d_prev_list == d_cur_list) return ctx_fail(D2FE_ERR_INVALID, "the previous and the current list must be different blocks");
  if (width < 16 || height < 16 || (size_t)width * height > (1u << 28)) return ctx_fail(D2FE_ERR_INVALID, "bad pyramid geometry");
  if (desc_dim < 1 || desc_dim > 65536 || kp_cap < 0 || kp_cap > 16384) return ctx_fail(D2FE_ERR_INVALID, "desc_dim must be 1..65536, kp_cap 0..16384");
  if (kp_cap > 0 && (!d_kps_xy || !d_kp_scores || !d_kp_desc || !d_n_kp)) return ctx_fail(D2FE_ERR_INVALID, "null keypoint arrays with kp_cap > 0");
  HIP_TRY(hipSetDevice(ctx_device(h)));
  hipStream_t s = stream ? (hipStream_t)stream : ctx_stream(h);
  LkCarryArgs c{};
  pyr_geometry(c.P, width, height, tp->levels, nullptr);
  c.prev_pyr = d_prev_pyr; c.cur_pyr = d_cur_pyr; c.win = tp->win; c.iters = tp->iters;
  c.prev = static_cast<const float*>(d_prev_list); c.cur = static_cast<float*>(d_cur_list);
  c.lay = carry_layout(tp->total_feature_num + 1, desc_dim);
  c.kps = d_kps_xy; c.kp_scores = d_kp_scores; c.kp_desc = d_kp_desc; c.n_kp = d_n_kp; c.kp_cap = kp_cap;
  c.total = tp->total_feature_num; c.near_thr = (double)tp->near_lk_thread_rate; c.min_dist = tp->feature_min_dist;
  c.next_id = d_next_id;
  {
    ProfScope ps(h, D2FE_PROF_LK, s);
    hipLaunchKernelGGL(lk_carry_step_kernel, dim3((c.lay.cap + 3) / 4), dim3(256), 0, s, c);
  }
  HIP_TRY(hipGetLastError());
  return D2FE_OK;
}

}  // extern "C"
