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
#include "lk_list_device.h"

namespace d2fe {

namespace {

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

// Steps b-e for one list, run by the workgroup whose ticket said it arrived last (256 threads, the list's scratch in the caller's LDS).  QUAD (the four-camera launch,
// lk_carry_quad_step_kernel): the ids of the NEW entries, header word 6 and *next_id belong to the launch's last finisher, which knows the new entries of the lower
// cameras; they are left alone here, and so is header word 7 of camera 0's list (keep7), the quad-level ticket
template <bool QUAD>
__device__ __forceinline__ void carry_finish(const LkCarryArgs& c, int n_prev, float* s_x, float* s_y, int* s_src, int* s_kp, int* s_cnt, bool keep7) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cap = c.lay.cap, D = c.lay.D;
  int* hdr = reinterpret_cast<int*>(c.cur);
  float* trk_xy = c.cur + c.lay.off[D2FE_LKC_TRK_XY];
  uint8_t* trk_st = reinterpret_cast<uint8_t*>(c.cur + c.lay.off[D2FE_LKC_TRK_STATUS]);
  // ---- b-d on wave 0
  if (wave == 0) {
    // b-c. reduceVector and removeNearPoints (lk_list_device.h, shared with the flow list)
    int cnt = 0;
    const int m = list_reduce_prune(trk_xy, trk_st, n_prev, c.near_thr, s_x, s_y, s_src, lane, cnt);
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
  const int id0 = QUAD ? 0 : *c.next_id;
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
    const int sk = live ? s_src[k] : 0, kk = !live ? 0 : old ? -1 : s_kp[k];
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
    if (!QUAD) {
      hdr[6] = id0 + (len - m);
      *c.next_id = id0 + (len - m);
    }
  }
  if (tid >= (keep7 ? 8 : 7) && tid < 64) hdr[tid] = 0;
}

__global__ __launch_bounds__(256) void lk_carry_step_kernel(LkCarryArgs c) {
  __shared__ float s_x[LKC_MAX], s_y[LKC_MAX];
  __shared__ int s_src[LKC_MAX], s_kp[LKC_MAX];
  __shared__ int s_cnt[4];          // [0] list length, [1] survivors of the tracker, [2] survivors of removeNearPoints, [3] this workgroup arrived last
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cap = c.lay.cap;
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

  // ---- b-e
  carry_finish<false>(c, n_prev, s_x, s_y, s_src, s_kp, s_cnt, false);
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
  lk_pyr_geometry(P, width, height, levels, total);
}


// ---- the quadcam forms -------------------------------------------------------------------------------------------------------------------------------------
// trackLocalFrames with sp_track_use_lk (d2featuretracker.cpp:121-133): track(images[c]) for c = 0..3 steps four lists per quad frame, and every new landmark takes
// its id from ONE counter in camera order.  Four launches of lk_carry_step_kernel are four links of a chain that is serial by the algorithm; here ONE launch of
// (slots / 4, 4 cameras) workgroups steps the four lists side by side (4 * cap_tracks waves: 604 for the reference's 151 slots, fewer than the card holds).  Camera c's
// workgroups take that camera's ticket (header word 5 of ITS list) and its last workgroup runs b-e for its list, all but the ids of the new entries.  The four
// finishers then take a second ticket, header word 7 of CAMERA 0's current list (zero between launches, like word 5; camera 0's finisher leaves it alone), and the
// last of them reads the four counts of new entries and hands the ids out: camera c's k-th new entry gets next_id + (new entries of cameras < c) + k, header word 6
// of camera c is next_id after that camera, as four launches in camera order would leave them
struct LkCarryQuadArgs {
  LkCarryArgs c;                    // camera 0
  long list_stride;                 // words between the cameras' lists (previous and current)
  size_t pyr_stride;                // bytes between the cameras' pyramids (previous and current)
};

__global__ __launch_bounds__(256) void lk_carry_quad_step_kernel(LkCarryQuadArgs q) {
  __shared__ float s_x[LKC_MAX], s_y[LKC_MAX];
  __shared__ int s_src[LKC_MAX], s_kp[LKC_MAX];
  __shared__ int s_cnt[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cam = blockIdx.y;
  LkCarryArgs c = q.c;
  const int cap = c.lay.cap, D = c.lay.D;
  float* cur0 = q.c.cur;
  c.prev += (size_t)cam * q.list_stride; c.cur += (size_t)cam * q.list_stride;
  c.prev_pyr += (size_t)cam * q.pyr_stride; c.cur_pyr += (size_t)cam * q.pyr_stride;
  if (c.kp_cap > 0) {               // rows of the dense [4][kp_cap] extract outputs
    c.kps += (size_t)cam * c.kp_cap * 2; c.kp_scores += (size_t)cam * c.kp_cap; c.kp_desc += (size_t)cam * c.kp_cap * D; c.n_kp += cam;
  }
  const int* phdr = reinterpret_cast<const int*>(c.prev);
  int* hdr = reinterpret_cast<int*>(c.cur);
  float* trk_xy = c.cur + c.lay.off[D2FE_LKC_TRK_XY];
  uint8_t* trk_st = reinterpret_cast<uint8_t*>(c.cur + c.lay.off[D2FE_LKC_TRK_STATUS]);
  const float* ppts = c.prev + c.lay.off[D2FE_LKC_PTS];
  int n_prev = __builtin_amdgcn_readfirstlane(phdr[0]);
  n_prev = n_prev < 0 ? 0 : n_prev > cap ? cap : n_prev;

  // ---- a. track: one wave per entry of the camera's previous list
  const int slot = blockIdx.x * 4 + wave;
  if (slot < n_prev) {
    LkArgs a{};
    a.win = c.win; a.iters = c.iters;
    const float ppx = ppts[2 * slot], ppy = ppts[2 * slot + 1];
    float cx, cy;
    const int ok = lk_bidir(a, c.P, c.prev_pyr, c.cur_pyr, ppx, ppy, cx, cy, lane);
    if (lane == 0) { trk_xy[2 * slot] = cx; trk_xy[2 * slot + 1] = cy; trk_st[slot] = (uint8_t)ok; }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  }
  // ---- the camera's ticket
  __syncthreads();
  if (tid == 0) {
    const int old = __hip_atomic_fetch_add(hdr + 5, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    const int last = old == (int)gridDim.x - 1;
    if (last) __hip_atomic_store(hdr + 5, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_cnt[3] = last;
  }
  __syncthreads();
  if (!s_cnt[3]) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  carry_finish<true>(c, n_prev, s_x, s_y, s_src, s_kp, s_cnt, cam == 0);

  // ---- the quad-level ticket: the list of this camera has left before its finisher arrives
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  __syncthreads();
  int* qt = reinterpret_cast<int*>(cur0) + 7;
  if (tid == 0) {
    const int old = __hip_atomic_fetch_add(qt, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    const int last = old == 3;
    if (last) __hip_atomic_store(qt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_cnt[3] = last;
  }
  __syncthreads();
  if (!s_cnt[3]) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  int base = *c.next_id;
  for (int k = 0; k < 4; ++k) {
    int* h = reinterpret_cast<int*>(cur0 + (size_t)k * q.list_stride);
    const int len = __hip_atomic_load(h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), fresh = __hip_atomic_load(h + 4, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    int* id = h + c.lay.off[D2FE_LKC_ID];
    for (int e = len - fresh + tid; e < len; e += 256) id[e] = base + (e - (len - fresh));
    base += fresh;
    if (tid == 0) h[6] = base;
  }
  __syncthreads();       // every thread has read *next_id
  if (tid == 0) *c.next_id = base;
}

// trackLK(left, right, type) of trackLocalFrames (d2featuretracker.cpp:128-132,697-752) for the lists of `quads` quad frames: one wave per (quad frame, neighbour pair,
// slot of list a).  List and pyramid of view (q, v) are (q * 4 + v) strides from the bases.  The gate and the shift of opticaltrack_utils.cpp:195-223: LEFT_RIGHT keeps
// x < cols - move_cols and starts at x + move_cols, RIGHT_LEFT keeps x >= move_cols and starts at x - move_cols.  Every slot is written
struct LkCarryNbArgs {
  const uint8_t* pyr; size_t pyr_stride;
  LkPairDev P;
  int quads, cap, win, iters;
  float move_cols;
  const float* lists; long list_stride, off_pts;
  float* xy; uint8_t* status;
};

__global__ __launch_bounds__(256) void lk_carry_neighbour_kernel(LkCarryNbArgs s) {
  // (view a, view b, type): (0,1) (1,2) (2,3) LEFT_RIGHT_IMG_MATCH = 1, (0,3) RIGHT_LEFT_IMG_MATCH = 2
  const int pair = blockIdx.y, qf = blockIdx.z;
  const int va = pair < 3 ? pair : 0, vb = pair < 3 ? pair + 1 : 3, type = pair < 3 ? 1 : 2;
  const int lane = threadIdx.x & 63;
  const int slot = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (slot >= s.cap) return;
  const size_t i = ((size_t)qf * 4 + pair) * s.cap + slot;
  const float* list = s.lists + ((size_t)qf * 4 + va) * s.list_stride;
  bool live = slot < reinterpret_cast<const int*>(list)[0];
  float ppx = 0.f, ppy = 0.f;
  if (live) {
    ppx = list[s.off_pts + 2 * slot]; ppy = list[s.off_pts + 2 * slot + 1];
    live = type == 1 ? ppx < (float)s.P.w - s.move_cols : ppx >= s.move_cols;
  }
  if (!live) {                      // wave-uniform
    if (lane == 0) { s.xy[2 * i] = 0.f; s.xy[2 * i + 1] = 0.f; s.status[i] = 0; }
    return;
  }
  LkArgs a{};
  a.win = s.win; a.iters = s.iters;
  const uint8_t* A = s.pyr + ((size_t)qf * 4 + va) * s.pyr_stride;
  const uint8_t* B = s.pyr + ((size_t)qf * 4 + vb) * s.pyr_stride;
  float cx, cy;
  const int ok = lk_bidir_half(a, s.P, A, B, ppx, ppy, type, s.move_cols, cx, cy, lane);
  if (lane == 0) { s.xy[2 * i] = cx; s.xy[2 * i + 1] = cy; s.status[i] = (uint8_t)ok; }
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
  const CarryLayout lay = desc_dim > 0 ? carry_layout(tp.total_feature_num + 1, desc_dim) : carry_layout(tp.total_feature_num > 1 ? tp.total_feature_num : 1, 0);
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

int d2fe_lk_carry_quad_step_device(d2fe_handle h, const uint8_t* d_prev_pyr, const uint8_t* d_cur_pyr, size_t pyr_stride, int width, int height, const void* d_prev_lists,
                                   void* d_cur_lists, size_t list_stride, int desc_dim, const float* d_kps_xy, const float* d_kp_scores, const float* d_kp_desc,
                                   const int32_t* d_n_kp, int kp_cap, const d2fe_track_params* tp, int32_t* d_next_id, void* stream) {
  if (!h || !d_prev_pyr || !d_cur_pyr || !d_prev_lists || !d_cur_lists || !tp || !d_next_id) return ctx_fail(D2FE_ERR_INVALID, "null argument");
  if (const char* why = lk_carry_check_params(tp)) return ctx_fail(D2FE_ERR_INVALID, why);
  if (width < 16 || height < 16 || (size_t)width * height > (1u << 28)) return ctx_fail(D2FE_ERR_INVALID, "bad pyramid geometry");
  if (desc_dim < 1 || desc_dim > 65536 || kp_cap < 0 || kp_cap > 16384) return ctx_fail(D2FE_ERR_INVALID, "desc_dim must be 1..65536, kp_cap 0..16384");
  if (kp_cap > 0 && (!d_kps_xy || !d_kp_scores || !d_kp_desc || !d_n_kp)) return ctx_fail(D2FE_ERR_INVALID, "null keypoint arrays with kp_cap > 0");
  LkCarryQuadArgs q{};
  LkCarryArgs& c = q.c;
  size_t total = 0;
  pyr_geometry(c.P, width, height, tp->levels, &total);
  c.lay = carry_layout(tp->total_feature_num + 1, desc_dim);
  if (list_stride < (size_t)c.lay.words || list_stride > (1ul << 40)) return ctx_fail(D2FE_ERR_INVALID, "list_stride (words) must be at least one list block");
  if (pyr_stride < total) return ctx_fail(D2FE_ERR_INVALID, "pyr_stride (bytes) must be at least one pyramid");
  {   // the four previous lists against the four current ones: no block may be both
    const char* a = static_cast<const char*>(d_prev_lists); const char* b = static_cast<const char*>(d_cur_lists);
    const size_t span = sizeof(float) * (3 * list_stride + (size_t)c.lay.words);
    if (a < b + span && b < a + span) return ctx_fail(D2FE_ERR_INVALID, "the previous and the current lists must not overlap");
  }
  HIP_TRY(hipSetDevice(ctx_device(h)));
  hipStream_t s = stream ? (hipStream_t)stream : ctx_stream(h);
  c.prev_pyr = d_prev_pyr; c.cur_pyr = d_cur_pyr; c.win = tp->win; c.iters = tp->iters;
  c.prev = static_cast<const float*>(d_prev_lists); c.cur = static_cast<float*>(d_cur_lists);
  c.kps = d_kps_xy; c.kp_scores = d_kp_scores; c.kp_desc = d_kp_desc; c.n_kp = d_n_kp; c.kp_cap = kp_cap;
  c.total = tp->total_feature_num; c.near_thr = (double)tp->near_lk_thread_rate; c.min_dist = tp->feature_min_dist;
  c.next_id = d_next_id;
  q.list_stride = (long)list_stride; q.pyr_stride = pyr_stride;
  {
    ProfScope ps(h, D2FE_PROF_LK, s);
    hipLaunchKernelGGL(lk_carry_quad_step_kernel, dim3((c.lay.cap + 3) / 4, 4), dim3(256), 0, s, q);
  }
  HIP_TRY(hipGetLastError());
  return D2FE_OK;
}

namespace {
// what the two neighbour launches share: the checks and the kernel's arguments; desc_dim = 0: flow lists (cap_tracks = max(total_feature_num, 1), no descriptors)
int neighbour_args(d2fe_handle h, const uint8_t* d_pyr, size_t pyr_stride, int quads, int width, int height, double undistort_fov, const void* d_lists, size_t list_stride,
                   int desc_dim, const d2fe_track_params* tp, float* d_nb_xy, uint8_t* d_nb_status, LkCarryNbArgs& r) {
  if (!h || !d_pyr || !d_lists || !tp || !d_nb_xy || !d_nb_status) return ctx_fail(D2FE_ERR_INVALID, "null argument");
  if (const char* why = lk_carry_check_params(tp)) return ctx_fail(D2FE_ERR_INVALID, why);
  if (width < 16 || height < 16 || (size_t)width * height > (1u << 28)) return ctx_fail(D2FE_ERR_INVALID, "bad pyramid geometry");
  if (quads < 1 || quads > 16383 || desc_dim < 0 || desc_dim > 65536 || !(undistort_fov > 0.0)) return ctx_fail(D2FE_ERR_INVALID, "quads must be 1..16383, desc_dim 1..65536, undistort_fov > 0");
  size_t total = 0;
  pyr_geometry(r.P, width, height, tp->levels, &total);
  const CarryLayout lay = desc_dim > 0 ? carry_layout(tp->total_feature_num + 1, desc_dim) : carry_layout(tp->total_feature_num > 1 ? tp->total_feature_num : 1, 0);
  if (list_stride < (size_t)lay.words || list_stride > (1ul << 40)) return ctx_fail(D2FE_ERR_INVALID, "list_stride (words) must be at least one list block");
  if (pyr_stride < total) return ctx_fail(D2FE_ERR_INVALID, "pyr_stride (bytes) must be at least one pyramid");
  r.pyr = d_pyr; r.pyr_stride = pyr_stride; r.quads = quads; r.cap = lay.cap; r.win = tp->win; r.iters = tp->iters;
  r.move_cols = d2fe_half_move_cols(width, undistort_fov);
  r.lists = static_cast<const float*>(d_lists); r.list_stride = (long)list_stride; r.off_pts = lay.off[D2FE_LKC_PTS];
  r.xy = d_nb_xy; r.status = d_nb_status;
  return D2FE_OK;
}
}  // namespace

int d2fe_lk_carry_neighbour_device(d2fe_handle h, const uint8_t* d_pyr, size_t pyr_stride, int quads, int width, int height, double undistort_fov, const void* d_lists,
                                   size_t list_stride, int desc_dim, const d2fe_track_params* tp, float* d_nb_xy, uint8_t* d_nb_status, void* stream) {
  if (desc_dim < 1) return ctx_fail(D2FE_ERR_INVALID, "quads must be 1..16383, desc_dim 1..65536, undistort_fov > 0");
  LkCarryNbArgs r{};
  if (const int rc = neighbour_args(h, d_pyr, pyr_stride, quads, width, height, undistort_fov, d_lists, list_stride, desc_dim, tp, d_nb_xy, d_nb_status, r)) return rc;
  HIP_TRY(hipSetDevice(ctx_device(h)));
  hipStream_t s = stream ? (hipStream_t)stream : ctx_stream(h);
  {
    ProfScope ps(h, D2FE_PROF_LK, s);
    hipLaunchKernelGGL(lk_carry_neighbour_kernel, dim3((r.cap + 3) / 4, 4, quads), dim3(256), 0, s, r);
  }
  HIP_TRY(hipGetLastError());
  return D2FE_OK;
}

// the same kernel over flow lists (lk_flow.hip), which carry no descriptors
int d2fe_lk_flow_neighbour_device(d2fe_handle h, const uint8_t* d_pyr, size_t pyr_stride, int quads, int width, int height, double undistort_fov, const void* d_lists,
                                  size_t list_stride, const d2fe_track_params* tp, float* d_nb_xy, uint8_t* d_nb_status, void* stream) {
  LkCarryNbArgs r{};
  if (const int rc = neighbour_args(h, d_pyr, pyr_stride, quads, width, height, undistort_fov, d_lists, list_stride, 0, tp, d_nb_xy, d_nb_status, r)) return rc;
  HIP_TRY(hipSetDevice(ctx_device(h)));
  hipStream_t s = stream ? (hipStream_t)stream : ctx_stream(h);
  {
    ProfScope ps(h, D2FE_PROF_LK, s);
    hipLaunchKernelGGL(lk_carry_neighbour_kernel, dim3((r.cap + 3) / 4, 4, quads), dim3(256), 0, s, r);
  }
  HIP_TRY(hipGetLastError());
  return D2FE_OK;
}

}  // extern "C"
