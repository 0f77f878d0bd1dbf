// lk_carry.hip -- the LK-carried landmark list of sp_track_use_lk on the device (include/d2fe.h, d2fe_lk_carry_step_device).
//   D2FeatureTracker::trackLK(frame)   d2frontend/src/d2featuretracker.cpp:472-621: track the previous list (opticalflowTrackPyr, opticaltrack_utils.cpp:173-279),
//                                      reduceVector (:273-276), removeNearPoints (opticaltrack_utils.h:61-89), copy the descriptors of the survivors (:509-521),
//                                      replenish from the frame's SuperPoint keypoints (:556-589)
//   trackLK(left, right)               :697-752 with sp_track_use_lk: the LIST entries (not the SuperPoint keypoints) are tracked left -> right
//
// MI355X mapping.  One frame = ONE launch (lk_carry_step_kernel): one 64-lane wave per list slot runs the bidirectional track (lk_bidir over lk.hip's lk_calc, lk_device.h), four
// waves to a workgroup; every workgroup then takes an agent-scope ticket in the output list's header and the last one to arrive runs steps b-e for the whole list.
// The split: step a with the ticket, steps b-c, the per-camera view of the kernel's arguments, the quad-level id hand-out and the entry points' shared refusals are
// lk_list_device.h's, one copy for this list and the flow list (lk_flow.hip); here are step d (the replenishment from the SuperPoint keypoints) and step e in
// carry_step_body, which the single kernel runs on camera 0's view and the quad kernel on blockIdx.y's, and the left -> right and neighbour launches over the lists.  The
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

struct LkCarryArgs : LkListArgs { const float* kp_scores; const float* kp_desc; };       // the keypoints' scores and descriptor rows beside LkListArgs::kps

// the camera's view (lk_list_device.h) with its rows of the scores and the descriptors
struct CarryCamera : ListCamera { const float* kp_scores; const float* kp_desc; };
__device__ __forceinline__ CarryCamera carry_camera(const LkCarryArgs& c, int cam, long list_stride, size_t pyr_stride) {
  CarryCamera v{list_camera(c, cam, list_stride, pyr_stride), c.kp_scores, c.kp_desc};
  if (c.kp_cap > 0) { v.kp_scores += (size_t)cam * c.kp_cap; v.kp_desc += (size_t)cam * c.kp_cap * c.lay.D; }
  return v;
}

// One list's step for workgroup bx of the nblocks that step it (256 threads): step a and the ticket (list_track_and_arrive, lk_list_device.h), then steps b-e on the
// workgroup that arrived last, which alone returns true.  s_cnt: [0] list length, [1] survivors of the tracker, [2] survivors of removeNearPoints, [3] the ticket's flag.
// QUAD (the four-camera launch, lk_carry_quad_step_kernel): the ids of the NEW entries, header word 6 and *next_id belong to the launch's last finisher, which knows the
// new entries of the lower cameras; they are left alone here, and so is header word 7 of camera 0's list (keep7), the quad-level ticket
template <bool QUAD>
__device__ __forceinline__ bool carry_step_body(const LkCarryArgs& c, const CarryCamera& v, int bx, int nblocks, bool keep7, int* s_cnt) {
  __shared__ float s_x[LKC_MAX], s_y[LKC_MAX];
  __shared__ int s_src[LKC_MAX], s_kp[LKC_MAX];
  int n_prev;
  if (!list_track_and_arrive(c, v, bx, nblocks, s_cnt + 3, n_prev)) return false;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cap = c.lay.cap, D = c.lay.D;
  int* hdr = reinterpret_cast<int*>(v.cur);
  float* trk_xy = v.cur + c.lay.off[D2FE_LKC_TRK_XY];
  uint8_t* trk_st = reinterpret_cast<uint8_t*>(v.cur + c.lay.off[D2FE_LKC_TRK_STATUS]);
  // ---- b-d on wave 0
  if (wave == 0) {
    // b-c. reduceVector and removeNearPoints (lk_list_device.h, shared with the flow list)
    int cnt = 0;
    const int m = list_reduce_prune(trk_xy, trk_st, n_prev, c.near_thr, s_x, s_y, s_src, lane, cnt);
    // d. replenish from the frame's SuperPoint keypoints
    int len = m;
    {
      const int n_kp = list_n_kp(c, v);
      const double thr = c.min_dist, t2 = thr * thr, lo = t2 * (1.0 - 1e-12), hi = t2 * (1.0 + 1e-12);
      for (int i = 0; i < n_kp; ++i) {
        if (len > c.total) break;
        const float kx = v.kps[2 * i], ky = v.kps[2 * i + 1];
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
  float* pts = v.cur + c.lay.off[D2FE_LKC_PTS];
  int* id = reinterpret_cast<int*>(v.cur + c.lay.off[D2FE_LKC_ID]);
  int* src = reinterpret_cast<int*>(v.cur + c.lay.off[D2FE_LKC_SRC]);
  int* kp = reinterpret_cast<int*>(v.cur + c.lay.off[D2FE_LKC_KP]);
  float* scores = v.cur + c.lay.off[D2FE_LKC_SCORES];
  float* desc = v.cur + c.lay.off[D2FE_LKC_DESC];
  const int* pid = reinterpret_cast<const int*>(v.prev + c.lay.off[D2FE_LKC_ID]);
  const float* pscores = v.prev + c.lay.off[D2FE_LKC_SCORES];
  const float* pdesc = v.prev + c.lay.off[D2FE_LKC_DESC];
  for (int k = tid; k < cap; k += 256) {
    const bool live = k < len, old = k < m;
    const int sk = live ? s_src[k] : 0, kk = !live ? 0 : old ? -1 : s_kp[k];
    pts[2 * k] = live ? s_x[k] : 0.f; pts[2 * k + 1] = live ? s_y[k] : 0.f;
    id[k] = !live ? 0 : old ? pid[sk] : id0 + (k - m);
    src[k] = sk; kp[k] = kk;
    scores[k] = !live ? 0.f : old ? pscores[sk] : v.kp_scores[kk];
    if (k >= n_prev) { trk_xy[2 * k] = 0.f; trk_xy[2 * k + 1] = 0.f; trk_st[k] = 0; }
  }
  for (int k = wave; k < cap; k += 4) {          // a descriptor row per wave
    float* dst = desc + (size_t)k * D;
    if (k < len) {
      const float* from = k < m ? pdesc + (size_t)s_src[k] * D : v.kp_desc + (size_t)s_kp[k] * D;
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
  return true;
}

__global__ __launch_bounds__(256) void lk_carry_step_kernel(LkCarryArgs c) {
  __shared__ int s_cnt[4];
  carry_step_body<false>(c, carry_camera(c, 0, 0, 0), blockIdx.x, gridDim.x, false, s_cnt);
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

// ---- the quadcam forms -------------------------------------------------------------------------------------------------------------------------------------
// trackLocalFrames with sp_track_use_lk (d2featuretracker.cpp:121-133): track(images[c]) for c = 0..3 steps four lists per quad frame, and every new landmark takes
// its id from ONE counter in camera order.  Four launches of lk_carry_step_kernel are four links of a chain that is serial by the algorithm; here ONE launch of
// (slots / 4, 4 cameras) workgroups steps the four lists side by side (4 * cap_tracks waves: 604 for the reference's 151 slots, fewer than the card holds).  Camera c's
// workgroups run carry_step_body on that camera's view: they take its ticket (header word 5 of ITS list) and its last workgroup runs b-e for its list, all but the ids
// of the new entries.  The four finishers then take a second ticket, header word 7 of CAMERA 0's current list (camera 0's finisher leaves it alone), and the last of
// them hands the ids out (quad_hand_out_ids, lk_list_device.h)
struct LkCarryQuadArgs {
  LkCarryArgs c;                    // camera 0
  long list_stride;                 // words between the cameras' lists (previous and current)
  size_t pyr_stride;                // bytes between the cameras' pyramids (previous and current)
};

__global__ __launch_bounds__(256) void lk_carry_quad_step_kernel(LkCarryQuadArgs q) {
  __shared__ int s_cnt[4];
  if (!carry_step_body<true>(q.c, carry_camera(q.c, blockIdx.y, q.list_stride, q.pyr_stride), blockIdx.x, gridDim.x, blockIdx.y == 0, s_cnt)) return;
  quad_hand_out_ids(q.c.cur, q.list_stride, 7, q.c.lay.off[D2FE_LKC_ID], q.c.next_id, s_cnt + 3);
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
  lk_pyr_geometry(r.P, width, height, tp.levels, &r.total);
  const CarryLayout lay = list_layout(tp, desc_dim);
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

namespace {
// what the two step entry points share: their refusals and the kernel's arguments
int carry_step_args(d2fe_handle h, const uint8_t* d_prev_pyr, const uint8_t* d_cur_pyr, int width, int height, const void* d_prev, void* d_cur, int desc_dim,
                    const float* d_kps_xy, const float* d_kp_scores, const float* d_kp_desc, const int32_t* d_n_kp, int kp_cap, const d2fe_track_params* tp,
                    int32_t* d_next_id, LkCarryArgs& c, size_t* pyr_total) {
  if (!tp) return ctx_fail(D2FE_ERR_INVALID, "null argument");
  if (const char* why = lk_carry_check_params(tp)) return ctx_fail(D2FE_ERR_INVALID, why);
  if (desc_dim < 1 || desc_dim > 65536 || kp_cap < 0 || kp_cap > 16384) return ctx_fail(D2FE_ERR_INVALID, "desc_dim must be 1..65536, kp_cap 0..16384");
  if (kp_cap > 0 && (!d_kp_scores || !d_kp_desc)) return ctx_fail(D2FE_ERR_INVALID, "null keypoint arrays with kp_cap > 0");
  c.kp_scores = d_kp_scores; c.kp_desc = d_kp_desc;
  return list_step_args(h, d_prev_pyr, d_cur_pyr, width, height, d_prev, d_cur, list_layout(*tp, desc_dim), d_kps_xy, d_n_kp, kp_cap, true, *tp, d_next_id, c, pyr_total);
}

// what the two neighbour launches share: the checks, the kernel's arguments and the launch; desc_dim = 0: flow lists (no descriptors)
int lk_neighbour_launch(d2fe_handle h, const uint8_t* d_pyr, size_t pyr_stride, int quads, int width, int height, double undistort_fov, const void* d_lists,
                        size_t list_stride, int desc_dim, const d2fe_track_params* tp, float* d_nb_xy, uint8_t* d_nb_status, void* stream) {
  if (!h || !d_pyr || !d_lists || !tp || !d_nb_xy || !d_nb_status) return ctx_fail(D2FE_ERR_INVALID, "null argument");
  if (const char* why = lk_carry_check_params(tp)) return ctx_fail(D2FE_ERR_INVALID, why);
  if (width < 16 || height < 16 || (size_t)width * height > (1u << 28)) return ctx_fail(D2FE_ERR_INVALID, "bad pyramid geometry");
  if (quads < 1 || quads > 16383 || desc_dim < 0 || desc_dim > 65536 || !(undistort_fov > 0.0)) return ctx_fail(D2FE_ERR_INVALID, "quads must be 1..16383, desc_dim 1..65536, undistort_fov > 0");
  LkCarryNbArgs r{};
  size_t total = 0;
  lk_pyr_geometry(r.P, width, height, tp->levels, &total);
  const CarryLayout lay = list_layout(*tp, desc_dim);
  if (list_stride < (size_t)lay.words || list_stride > (1ul << 40)) return ctx_fail(D2FE_ERR_INVALID, "list_stride (words) must be at least one list block");
  if (pyr_stride < total) return ctx_fail(D2FE_ERR_INVALID, "pyr_stride (bytes) must be at least one pyramid");
  r.pyr = d_pyr; r.pyr_stride = pyr_stride; r.quads = quads; r.cap = lay.cap; r.win = tp->win; r.iters = tp->iters;
  r.move_cols = d2fe_half_move_cols(width, undistort_fov);
  r.lists = static_cast<const float*>(d_lists); r.list_stride = (long)list_stride; r.off_pts = lay.off[D2FE_LKC_PTS];
  r.xy = d_nb_xy; r.status = d_nb_status;
  HIP_TRY(hipSetDevice(ctx_device(h)));
  hipStream_t s = stream ? (hipStream_t)stream : ctx_stream(h);
  {
    ProfScope ps(h, D2FE_PROF_LK, s);
    hipLaunchKernelGGL(lk_carry_neighbour_kernel, dim3((r.cap + 3) / 4, 4, quads), dim3(256), 0, s, r);
  }
  HIP_TRY(hipGetLastError());
  return D2FE_OK;
}
}  // namespace

int d2fe_lk_carry_step_device(d2fe_handle h, const uint8_t* d_prev_pyr, const uint8_t* d_cur_pyr, int width, int height, const void* d_prev_list, void* d_cur_list,
                              int desc_dim, const float* d_kps_xy, const float* d_kp_scores, const float* d_kp_desc, const int32_t* d_n_kp, int kp_cap,
                              const d2fe_track_params* tp, int32_t* d_next_id, void* stream) {
  LkCarryArgs c{};
  if (const int rc = carry_step_args(h, d_prev_pyr, d_cur_pyr, width, height, d_prev_list, d_cur_list, desc_dim, d_kps_xy, d_kp_scores, d_kp_desc, d_n_kp, kp_cap, tp,
                                     d_next_id, c, nullptr)) return rc;
  HIP_TRY(hipSetDevice(ctx_device(h)));
  hipStream_t s = stream ? (hipStream_t)stream : ctx_stream(h);
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
  LkCarryQuadArgs q{};
  LkCarryArgs& c = q.c;
  size_t total = 0;
  if (const int rc = carry_step_args(h, d_prev_pyr, d_cur_pyr, width, height, d_prev_lists, d_cur_lists, desc_dim, d_kps_xy, d_kp_scores, d_kp_desc, d_n_kp, kp_cap, tp,
                                     d_next_id, c, &total)) return rc;
  if (const int rc = list_quad_check(c, list_stride, pyr_stride, total)) return rc;
  q.list_stride = (long)list_stride; q.pyr_stride = pyr_stride;
  HIP_TRY(hipSetDevice(ctx_device(h)));
  hipStream_t s = stream ? (hipStream_t)stream : ctx_stream(h);
  {
    ProfScope ps(h, D2FE_PROF_LK, s);
    hipLaunchKernelGGL(lk_carry_quad_step_kernel, dim3((c.lay.cap + 3) / 4, 4), dim3(256), 0, s, q);
  }
  HIP_TRY(hipGetLastError());
  return D2FE_OK;
}

int d2fe_lk_carry_neighbour_device(d2fe_handle h, const uint8_t* d_pyr, size_t pyr_stride, int quads, int width, int height, double undistort_fov, const void* d_lists,
                                   size_t list_stride, int desc_dim, const d2fe_track_params* tp, float* d_nb_xy, uint8_t* d_nb_status, void* stream) {
  if (desc_dim < 1) return ctx_fail(D2FE_ERR_INVALID, "quads must be 1..16383, desc_dim 1..65536, undistort_fov > 0");
  return lk_neighbour_launch(h, d_pyr, pyr_stride, quads, width, height, undistort_fov, d_lists, list_stride, desc_dim, tp, d_nb_xy, d_nb_status, stream);
}

// the same kernel over flow lists (lk_flow.hip), which carry no descriptors
int d2fe_lk_flow_neighbour_device(d2fe_handle h, const uint8_t* d_pyr, size_t pyr_stride, int quads, int width, int height, double undistort_fov, const void* d_lists,
                                  size_t list_stride, const d2fe_track_params* tp, float* d_nb_xy, uint8_t* d_nb_status, void* stream) {
  return lk_neighbour_launch(h, d_pyr, pyr_stride, quads, width, height, undistort_fov, d_lists, list_stride, 0, tp, d_nb_xy, d_nb_status, stream);
}

}  // extern "C"
