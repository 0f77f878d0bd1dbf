// lk_list_device.h -- what the two landmark lists of D2FeatureTracker::trackLK(frame) share on the device: the block layout, the distance test of cv::norm and steps
// b-c (reduceVector, removeNearPoints).  lk_carry.hip (the LK-carried SuperPoint list of sp_track_use_lk) and lk_flow.hip (the FAST-replenished flow list) include it;
// each replenishes in its own way.  Internal.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/d2fe.h"
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

// the pyramid of a d2fe_lk_frame / one image of the stereo workspace: levels + 1 tight images one after the other
inline void lk_pyr_geometry(LkPairDev& P, int width, int height, int levels, size_t* total) {
  int o = 0;
  for (int l = 0, w = width, hh = height; l <= levels; ++l) { P.off[l] = o; P.ws[l] = w; P.hs[l] = hh; o += w * hh; w = (w + 1) / 2; hh = (hh + 1) / 2; }
  P.levels = levels; P.w = width; P.h = height; P.type = 0; P.move_cols = 0.f;
  if (total) *total = (size_t)o;
}

}  // namespace
}  // namespace d2fe
