// lk_device.h -- the device functions of the sparse pyramidal LK tracker (cv::cuda::SparsePyrLKOpticalFlow, evaluation order of oracle/d2fe_oracle_lk.c), shared by
// the translation units that launch them: lk.hip (d2fe_lk_track*, the stereo tracks), lk_carry.hip (the LK-carried landmark list) and lk_flow.hip (the flow list).
// One 64-lane wave per point.  Internal.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace d2fe {
namespace {

// ---- sparse pyramidal LK ---------------------------------------------------------------------------------------------------------
// one (previous frame, current frame) pair of a batched call; a point carries the index of its pair
struct LkPairDev {
  const uint8_t* prev; const uint8_t* cur;
  int off[8], ws[8], hs[8];
  int levels, w, h, type;
  float move_cols;
  int pad_[3];
};
struct LkArgs {
  const LkPairDev* pairs; const int* pair_of;
  int n, win, iters;
  const float* prev_pts; const float* cur_init;
  float* cur_pts; uint8_t* status;
};

__device__ __forceinline__ float tex(const uint8_t* __restrict__ im, int w, int h, float x, float y) {
  const float xs = x - 0.5f, ys = y - 0.5f;
  const float xf = __builtin_floorf(xs), yf = __builtin_floorf(ys);
  const float fx = xs - xf, fy = ys - yf;
  int x0 = (int)xf, y0 = (int)yf, x1 = x0 + 1, y1 = y0 + 1;
  x0 = min(max(x0, 0), w - 1); x1 = min(max(x1, 0), w - 1);
  y0 = min(max(y0, 0), h - 1); y1 = min(max(y1, 0), h - 1);
  const float s = 1.0f / 255.0f;
  const float p00 = (float)im[(size_t)y0 * w + x0] * s, p10 = (float)im[(size_t)y0 * w + x1] * s;
  const float p01 = (float)im[(size_t)y1 * w + x0] * s, p11 = (float)im[(size_t)y1 * w + x1] * s;
  const float gx = 1.0f - fx, gy = 1.0f - fy;
  float v = (gx * gy) * p00;
  v = v + (fx * gy) * p10;
  v = v + (gx * fy) * p01;
  v = v + (fx * fy) * p11;
  return v;
}

// the shared-memory tree of OpenCV's block reduce, v[t] += v[t+s] for s = 32..1, result broadcast from lane 0
__device__ __forceinline__ float tree64(float v) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v = v + __shfl_down(v, s, 64);
  return __shfl(v, 0, 64);
}

// one pyramid level for one point, executed by a whole wave with uniform control flow
__device__ void lk_level(const uint8_t* __restrict__ I, const uint8_t* __restrict__ J, int cols, int rows, int level, int win,
                         int iters, float ppx, float ppy, float& npx, float& npy, int& status, int lane) {
  const float half = (float)((win - 1) / 2);
  float px = ppx * (1.0f / (float)(1 << level)), py = ppy * (1.0f / (float)(1 << level));
  if (px < 0 || px >= (float)cols || py < 0 || py >= (float)rows) {
    if (level == 0) status = 0;
    return;
  }
  px -= half; py -= half;
  const int tx = lane & 7, ty = lane >> 3;
  float Ip[3][3], Dx[3][3], Dy[3][3];
  float s11 = 0.f, s12 = 0.f, s22 = 0.f;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int xb = tx + 8 * j, yb = ty + 8 * i;
      Ip[i][j] = 0.f; Dx[i][j] = 0.f; Dy[i][j] = 0.f;
      if (xb < win && yb < win) {
        const float x = px + (float)xb + 0.5f, y = py + (float)yb + 0.5f;
        Ip[i][j] = tex(I, cols, rows, x, y);
        const float tmm = tex(I, cols, rows, x - 1, y - 1), tpm = tex(I, cols, rows, x + 1, y - 1);
        const float tmp = tex(I, cols, rows, x - 1, y + 1), tpp = tex(I, cols, rows, x + 1, y + 1);
        float dx = 3.0f * tpm;
        dx = dx + 10.0f * tex(I, cols, rows, x + 1, y);
        dx = dx + 3.0f * tpp;
        float mx = 3.0f * tmm;
        mx = mx + 10.0f * tex(I, cols, rows, x - 1, y);
        mx = mx + 3.0f * tmp;
        dx = dx - mx;
        float dy = 3.0f * tmp;
        dy = dy + 10.0f * tex(I, cols, rows, x, y + 1);
        dy = dy + 3.0f * tpp;
        float my = 3.0f * tmm;
        my = my + 10.0f * tex(I, cols, rows, x, y - 1);
        my = my + 3.0f * tpm;
        dy = dy - my;
        Dx[i][j] = dx; Dy[i][j] = dy;
        s11 = s11 + dx * dx; s12 = s12 + dx * dy; s22 = s22 + dy * dy;
      }
    }
  float A11 = tree64(s11), A12 = tree64(s12), A22 = tree64(s22);
  float D = A11 * A22 - A12 * A12;
  if (D < 1.1920928955078125e-07f) {
    if (level == 0) status = 0;
    return;
  }
  D = 1.0f / D;
  A11 = A11 * D; A12 = A12 * D; A22 = A22 * D;
  float nx = npx * 2.0f, ny = npy * 2.0f;
  nx -= half; ny -= half;
  for (int k = 0; k < iters; ++k) {
    if (nx < -half || nx >= (float)cols || ny < -half || ny >= (float)rows) {
      if (level == 0) status = 0;
      return;
    }
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int xb = tx + 8 * j, yb = ty + 8 * i;
        if (xb < win && yb < win) {
          const float Jv = tex(J, cols, rows, nx + (float)xb + 0.5f, ny + (float)yb + 0.5f);
          const float diff = (Jv - Ip[i][j]) * 32.0f;
          s1 = s1 + diff * Dx[i][j];
          s2 = s2 + diff * Dy[i][j];
        }
      }
    const float B1 = tree64(s1), B2 = tree64(s2);
    const float ddx = A12 * B2 - A22 * B1;
    const float ddy = A12 * B1 - A11 * B2;
    nx = nx + ddx; ny = ny + ddy;
    if (__builtin_fabsf(ddx) < 0.01f && __builtin_fabsf(ddy) < 0.01f) break;
  }
  npx = nx + half; npy = ny + half;
}

__device__ __forceinline__ void lk_calc(const LkArgs& a, const LkPairDev& P, const uint8_t* Ip, const uint8_t* Jp, float ppx,
                                        float ppy, float& npx, float& npy, int& status, int lane) {
  const float sc = (float)(1.0 / (double)(1 << P.levels) / 2.0);
  npx = npx * sc; npy = npy * sc;
  status = 1;
  for (int l = P.levels; l >= 0; --l)
    lk_level(Ip + P.off[l], Jp + P.off[l], P.ws[l], P.hs[l], l, a.win, a.iters, ppx, ppy, npx, npy, status, lane);
}

// opticalflowTrackPyr with WHOLE_IMG_MATCH and cur_init = the point itself (opticaltrack_utils.cpp:173-279) for one point on one wave: forward Ip -> Jp, reverse from
// the result, status = forward && reverse && |point - reverse| <= 0.5 && inBorder (:260-272).  (cx, cy) is the forward result whatever the status.  The landmark-list
// kernels of lk_carry.hip share it; lk_track_stereo_kernel keeps its own spelling of the same lines (a test pins that kernel's text)
__device__ __forceinline__ int lk_bidir(const LkArgs& a, const LkPairDev& P, const uint8_t* Ip, const uint8_t* Jp, float ppx, float ppy, float& cx, float& cy, int lane) {
  cx = ppx; cy = ppy;
  int st = 1, rst = 1;
  lk_calc(a, P, Ip, Jp, ppx, ppy, cx, cy, st, lane);
  float rx = cx, ry = cy;
  lk_calc(a, P, Jp, Ip, cx, cy, rx, ry, rst, lane);
  const float dx = ppx - rx, dy = ppy - ry;
  const double nrm = __builtin_sqrt((double)dx * dx + (double)dy * dy);
  int ok = (st && rst && nrm <= 0.5) ? 1 : 0;
  if (ok) {
    const int ix = (int)__builtin_rint((double)cx), iy = (int)__builtin_rint((double)cy);
    if (!(1 <= ix && ix < P.w - 1 && 1 <= iy && iy < P.h - 1)) ok = 0;
  }
  return ok;
}

// The half-image form (LEFT_RIGHT_IMG_MATCH type 1 / RIGHT_LEFT_IMG_MATCH type 2, opticaltrack_utils.cpp:197-253) for one point that has passed the gate: the
// initial guess is the point shifted by +move_cols (type 1) or -move_cols (type 2), the reverse track starts from the forward result shifted back when the
// forward status is 1.  The arithmetic of lk_track_kernel (lk.hip) with P.type 1 / 2 and cur_init = (ppx +- move_cols, ppy)
__device__ __forceinline__ int lk_bidir_half(const LkArgs& a, const LkPairDev& P, const uint8_t* Ip, const uint8_t* Jp, float ppx, float ppy, int type, float move_cols,
                                             float& cx, float& cy, int lane) {
  cx = type == 1 ? ppx + move_cols : ppx - move_cols; cy = ppy;
  int st = 1, rst = 1;
  lk_calc(a, P, Ip, Jp, ppx, ppy, cx, cy, st, lane);
  float rx = cx, ry = cy;
  if (type == 1 && st == 1) rx -= move_cols;
  if (type == 2 && st == 1) rx += move_cols;
  lk_calc(a, P, Jp, Ip, cx, cy, rx, ry, rst, lane);
  const float dx = ppx - rx, dy = ppy - ry;
  const double nrm = __builtin_sqrt((double)dx * dx + (double)dy * dy);
  int ok = (st && rst && nrm <= 0.5) ? 1 : 0;
  if (ok) {
    const int ix = (int)__builtin_rint((double)cx), iy = (int)__builtin_rint((double)cy);
    if (!(1 <= ix && ix < P.w - 1 && 1 <= iy && iy < P.h - 1)) ok = 0;
  }
  return ok;
}

}  // namespace
}  // namespace d2fe
