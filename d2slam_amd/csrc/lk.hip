// lk.hip -- SURVEY.md section 8(f)-4: the LK optical-flow tracker of d2frontend on the device.
//   buildImagePyramid   d2frontend/src/opticaltrack_utils.cpp:526-542 (cv::cuda::pyrDown)
//   opticalflowTrackPyr :173-279 (cv::cuda::SparsePyrLKOpticalFlow forward + reverse, 0.5 px check, inBorder)
//   detectFastByRegion  :444-493 (cv::cuda::FastFeatureDetector per region), detectPoints :375-442 (good features)
// The arithmetic is OpenCV 4.10's (not in the reference tree); the evaluation orders fixed by the oracle
// (oracle/d2fe_oracle_lk.c, header) are reproduced operation by operation, so every output is compared bitwise.
//
// MI355X mapping: one 64-lane wave per tracked point = OpenCV's 8x8 thread block; the whole bidirectional track of a
// point (3 pyramid levels forward, 3 back, the 0.5 px test and the border test) is ONE kernel launch instead of
// 6 launches + 4 PCIe round trips; the 21x21 window lives in 27 registers per lane; reductions are 6 DPP/shuffle steps.
// All of it is latency-bound byte/float work (150 points x 441 px): no MFMA, no LDS staging needed.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/d2fe.h"
#include "context.h"
#include "kernels.h"
#include "fast_device.h"
#include "lk_device.h"

namespace d2fe {

namespace {

__device__ __forceinline__ int reflect101(int p, int n) {
  if (n == 1) return 0;
  while (p < 0 || p >= n) p = p < 0 ? -p : 2 * n - 2 - p;
  return p;
}

// ---- pyrDown: 5x5 [1 4 6 4 1]^2 / 256, reflect-101 border, round half to even --------------------------------------------
__device__ __forceinline__ uint8_t pyr_down_px(const uint8_t* __restrict__ src, size_t stride, int w, int h, int x, int y) {
  const int k[5] = {1, 4, 6, 4, 1};
  int xs[5];
#pragma unroll
  for (int j = 0; j < 5; ++j) xs[j] = reflect101(2 * x + j - 2, w);
  int s = 0;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const uint8_t* row = src + (size_t)reflect101(2 * y + i - 2, h) * stride;
    int r = 0;
#pragma unroll
    for (int j = 0; j < 5; ++j) r += k[j] * row[xs[j]];
    s += k[i] * r;
  }
  int q = s >> 8;
  const int rem = s & 255;
  if (rem > 128 || (rem == 128 && (q & 1))) ++q;
  return (uint8_t)(q > 255 ? 255 : q);
}

__global__ __launch_bounds__(256) void pyr_down_kernel(const uint8_t* __restrict__ src, int w, int h, uint8_t* __restrict__ dst,
                                                       int dw, int dh) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= dw || y >= dh) return;
  dst[(size_t)y * dw + x] = pyr_down_px(src, (size_t)w, w, h, x, y);
}

// Batched form for the stereo tracker: pyramids of 2 n frames (n left, n right images that are already in HBM) side by side in one workspace,
// image i at i * total, each in the layout of d2fe_lk_frame_s.  ONE launch per level over all images (blockIdx.z = image).  The launch of level 1
// reads the caller's frames (any row stride) and also writes level 0, the tight copy: thread (x, y) of level 1 owns the 2 x 2 pixels under it.
// levels == 0: the same launch with dst_off < 0 only copies
struct PyrBatchArgs {
  const uint8_t* left; const uint8_t* right;      // level 1: the frames; deeper levels: unused
  size_t src_stride, src_image_stride;
  uint8_t* ws; size_t total;
  int n, first;                                   // images per side; first != 0: this launch reads the caller's frames and writes level 0
  int src_off, sw, sh, dst_off, dw, dh;           // source / destination level inside a pyramid
};

__global__ __launch_bounds__(256) void pyr_down_batch_kernel(PyrBatchArgs a) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  const int i = blockIdx.z;
  uint8_t* pyr = a.ws + (size_t)i * a.total;
  const uint8_t* src = pyr + a.src_off;
  size_t stride = (size_t)a.sw;
  if (a.first) {
    src = (i < a.n ? a.left + (size_t)i * a.src_image_stride : a.right + (size_t)(i - a.n) * a.src_image_stride);
    stride = a.src_stride;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        const int px = 2 * x + dx, py = 2 * y + dy;
        if (px < a.sw && py < a.sh) pyr[(size_t)py * a.sw + px] = src[(size_t)py * stride + px];
      }
  }
  if (a.dst_off < 0 || x >= a.dw || y >= a.dh) return;
  pyr[(size_t)a.dst_off + (size_t)y * a.dw + x] = pyr_down_px(src, stride, a.sw, a.sh, x, y);
}

// ---- sparse pyramidal LK: the device functions (tex, lk_level, lk_calc) and LkPairDev / LkArgs live in lk_device.h ------------------------------------------
__global__ __launch_bounds__(256) void lk_track_kernel(LkArgs a) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (i >= a.n) return;
  const LkPairDev& P = a.pairs[__builtin_amdgcn_readfirstlane(a.pair_of[i])];   // wave-uniform: scalar loads
  const float ppx = a.prev_pts[2 * i], ppy = a.prev_pts[2 * i + 1];
  float cx = a.cur_init[2 * i], cy = a.cur_init[2 * i + 1];
  int st = 1, rst = 1;
  lk_calc(a, P, P.prev, P.cur, ppx, ppy, cx, cy, st, lane);
  float rx = cx, ry = cy;
  if (P.type == 1 && st == 1) rx -= P.move_cols;
  if (P.type == 2 && st == 1) rx += P.move_cols;
  lk_calc(a, P, P.cur, P.prev, cx, cy, rx, ry, rst, lane);
  const float dx = ppx - rx, dy = ppy - ry;
  const double nrm = __builtin_sqrt((double)dx * dx + (double)dy * dy);
  int ok = (st && rst && nrm <= 0.5) ? 1 : 0;
  if (ok) {
    const int ix = (int)__builtin_rint((double)cx), iy = (int)__builtin_rint((double)cy);
    if (!(1 <= ix && ix < P.w - 1 && 1 <= iy && iy < P.h - 1)) ok = 0;
  }
  if (lane == 0) {
    a.cur_pts[2 * i] = cx; a.cur_pts[2 * i + 1] = cy;
    a.status[i] = (uint8_t)ok;
  }
}

// The stereo form (trackLK left -> right, d2featuretracker.cpp:697-752): points and their number come from DEVICE memory -- the keypoints SuperPoint left
// for image f (d2fe_superpoint_extract_device / the pipe) -- so nothing of it needs the host.  One wave per (frame, keypoint slot); (prev, cur) = (left,
// right) pyramid of the frame in the workspace of pyr_down_batch_kernel; cur_init = prev_pts (opticaltrack_utils.cpp:195-196); WHOLE_IMG_MATCH.
// Slots >= n_kp[f] are written too (status 0, point (0, 0)): the result block never carries stale data and needs no memset
struct LkStereoArgs {
  const uint8_t* ws; size_t total;
  LkPairDev P;                      // geometry only (prev / cur are per frame)
  int n_frames, cap, win, iters;
  const float* kps; const int* n_kp;
  float* cur_pts; uint8_t* status;
};

__global__ __launch_bounds__(256) void lk_track_stereo_kernel(LkStereoArgs s) {
  const int lane = threadIdx.x & 63;
  const int slot = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), f = blockIdx.y;
  if (slot >= s.cap) return;
  const size_t i = (size_t)f * s.cap + slot;
  if (slot >= s.n_kp[f]) {          // wave-uniform: dead slots leave before touching an image
    if (lane == 0) { s.cur_pts[2 * i] = 0.f; s.cur_pts[2 * i + 1] = 0.f; s.status[i] = 0; }
    return;
  }
  LkArgs a{};
  a.win = s.win; a.iters = s.iters;
  const LkPairDev& P = s.P;
  const uint8_t* L = s.ws + (size_t)f * s.total;
  const uint8_t* R = s.ws + (size_t)(s.n_frames + f) * s.total;
  const float ppx = s.kps[2 * i], ppy = s.kps[2 * i + 1];
  float cx = ppx, cy = ppy;
  int st = 1, rst = 1;
  lk_calc(a, P, L, R, ppx, ppy, cx, cy, st, lane);
  float rx = cx, ry = cy;
  lk_calc(a, P, R, L, cx, cy, rx, ry, rst, lane);
  const float dx = ppx - rx, dy = ppy - ry;
  const double nrm = __builtin_sqrt((double)dx * dx + (double)dy * dy);
  int ok = (st && rst && nrm <= 0.5) ? 1 : 0;
  if (ok) {
    const int ix = (int)__builtin_rint((double)cx), iy = (int)__builtin_rint((double)cy);
    if (!(1 <= ix && ix < P.w - 1 && 1 <= iy && iy < P.h - 1)) ok = 0;
  }
  if (lane == 0) {
    s.cur_pts[2 * i] = cx; s.cur_pts[2 * i + 1] = cy;
    s.status[i] = (uint8_t)ok;
  }
}

// ---- FAST-9/16 ---------------------------------------------------------------------------------------------------------------------
// fast_strength, fast_region_kernel and fast_nonmax_kernel live in fast_device.h: the device detector of lk_flow.hip launches the same two kernels

// ---- good features to track -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sobel_kernel(const uint8_t* __restrict__ img, int stride, int w, int h, float k0, float k1,
                                                    float* __restrict__ dx, float* __restrict__ dy) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= w || y >= h) return;
  const int xm = reflect101(x - 1, w), xp = reflect101(x + 1, w);
  const int ys[3] = {reflect101(y - 1, h), y, reflect101(y + 1, h)};
  float t0[3], t1[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const uint8_t* row = img + (size_t)ys[r] * stride;
    const float a = (float)row[xm], b = (float)row[x], c = (float)row[xp];
    t0[r] = c - a;
    t1[r] = (a + 2.0f * b) + c;
  }
  float s = k0 * t0[0];
  s = s + k1 * t0[1];
  s = s + k0 * t0[2];
  dx[(size_t)y * w + x] = s;
  dy[(size_t)y * w + x] = k0 * t1[2] - k0 * t1[0];
}

__global__ __launch_bounds__(256) void min_eigen_kernel(const float* __restrict__ dx, const float* __restrict__ dy, int w, int h,
                                                        float* __restrict__ eig, unsigned* __restrict__ maxbits) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  float e = 0.f;
  if (x < w && y < h) {
    float a = 0.f, b = 0.f, c = 0.f;
#pragma unroll
    for (int i = -1; i <= 1; ++i) {
      const size_t ro = (size_t)reflect101(y + i, h) * w;
#pragma unroll
      for (int j = -1; j <= 1; ++j) {
        const size_t o = ro + reflect101(x + j, w);
        const float gx = dx[o], gy = dy[o];
        a = a + gx * gx; b = b + gx * gy; c = c + gy * gy;
      }
    }
    a = a * 0.5f; c = c * 0.5f;
    e = (a + c) - __builtin_sqrtf((a - c) * (a - c) + b * b);
    eig[(size_t)y * w + x] = e;
  }
  // max over the image: non-negative floats order like their bit patterns (negative / NaN values never win against 0)
  float m = e > 0.f ? e : 0.f;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0 && m > 0.f) atomicMax(maxbits, __float_as_uint(m));
}

__global__ __launch_bounds__(256) void corners_kernel(const float* __restrict__ eig, int w, int h, const unsigned* __restrict__ maxbits,
                                                      double quality, unsigned long long* __restrict__ out, int cap,
                                                      int* __restrict__ count) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x < 1 || y < 1 || x >= w - 1 || y >= h - 1) return;
  const float thr = (float)((double)__uint_as_float(*maxbits) * quality);
  const float v = eig[(size_t)y * w + x];
  if (!(v > thr)) return;
  float m = v;
#pragma unroll
  for (int i = -1; i <= 1; ++i)
#pragma unroll
    for (int j = -1; j <= 1; ++j) m = fmaxf(m, eig[(size_t)(y + i) * w + x + j]);
  if (v == m) {
    const int k = atomicAdd(count, 1);
    // v > thr >= 0: the bit pattern orders like the value; low word = ~raster index (ties: lower index first)
    if (k < cap) out[k] = ((unsigned long long)__float_as_uint(v) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)(y * w + x));
  }
}

}  // namespace

// internal accessors of the context (api.hip)
int ctx_fail(int code, const std::string& msg);
int ctx_device(d2fe_handle h);
hipStream_t ctx_stream(d2fe_handle h);
int ctx_scratch(d2fe_handle h, size_t bytes, void** out);

}  // namespace d2fe

using namespace d2fe;

struct d2fe_lk_frame_s {
  int device = 0;                 // the frame outlives nothing but must not touch the handle after creation
  int w = 0, hgt = 0, levels = 0, total = 0;
  int off[8], ws[8], hs[8];
  uint8_t* pyr = nullptr;
};

#define LK_TRY(expr)                                                                                                         \
  do {                                                                                                                       \
    hipError_t e_ = (expr);                                                                                                  \
    if (e_ != hipSuccess) return ctx_fail(D2FE_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_) + " @lk.hip:" + std::to_string(__LINE__)); \
  } while (0)

namespace {

int frame_alloc(d2fe_handle h, int width, int height, int levels, d2fe_lk_frame* out) {
  if (!h || !out) return ctx_fail(D2FE_ERR_INVALID, "null argument");
  *out = nullptr;
  if (width < 16 || height < 16 || levels < 0 || levels > 7) return ctx_fail(D2FE_ERR_INVALID, "bad pyramid geometry");
  LK_TRY(hipSetDevice(ctx_device(h)));
  d2fe_lk_frame f = new d2fe_lk_frame_s();
  f->device = ctx_device(h); f->w = width; f->hgt = height; f->levels = levels;
  int o = 0, w = width, hh = height;
  for (int l = 0; l <= levels; ++l) {
    f->off[l] = o; f->ws[l] = w; f->hs[l] = hh;
    o += w * hh; w = (w + 1) / 2; hh = (hh + 1) / 2;
  }
  f->total = o;
  if (hipMalloc(&f->pyr, (size_t)o) != hipSuccess) { delete f; return ctx_fail(D2FE_ERR_HIP, "hipMalloc pyramid"); }
  *out = f;
  return D2FE_OK;
}

hipError_t frame_build(d2fe_lk_frame f, hipStream_t s) {
  for (int l = 1; l <= f->levels; ++l) {
    hipLaunchKernelGGL(pyr_down_kernel, dim3((f->ws[l] + 63) / 64, (f->hs[l] + 3) / 4), dim3(256), 0, s, f->pyr + f->off[l - 1],
                       f->ws[l - 1], f->hs[l - 1], f->pyr + f->off[l], f->ws[l], f->hs[l]);
  }
  return hipGetLastError();
}

}  // namespace

extern "C" {

int d2fe_lk_frame_create(d2fe_handle h, const uint8_t* gray, int width, int height, int stride, int levels, d2fe_lk_frame* out) {
  if (!gray || stride < width) return ctx_fail(D2FE_ERR_INVALID, "null image / bad stride");
  const int rc = frame_alloc(h, width, height, levels, out);
  if (rc != D2FE_OK) return rc;
  d2fe_lk_frame f = *out;
  hipStream_t s = ctx_stream(h);
  hipError_t e = hipMemcpy2DAsync(f->pyr, (size_t)width, gray, (size_t)stride, (size_t)width, (size_t)height, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = frame_build(f, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) { d2fe_lk_frame_destroy(f); *out = nullptr; return ctx_fail(D2FE_ERR_HIP, std::string("lk frame: ") + hipGetErrorString(e)); }
  return D2FE_OK;
}

int d2fe_lk_frame_create_device(d2fe_handle h, const uint8_t* d_gray, int width, int height, int stride, int levels, void* stream,
                                d2fe_lk_frame* out) {
  if (!d_gray || stride < width) return ctx_fail(D2FE_ERR_INVALID, "null image / bad stride");
  const int rc = frame_alloc(h, width, height, levels, out);
  if (rc != D2FE_OK) return rc;
  d2fe_lk_frame f = *out;
  hipStream_t s = stream ? (hipStream_t)stream : ctx_stream(h);
  hipError_t e = hipMemcpy2DAsync(f->pyr, (size_t)width, d_gray, (size_t)stride, (size_t)width, (size_t)height, hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess) e = frame_build(f, s);
  if (e != hipSuccess) { d2fe_lk_frame_destroy(f); *out = nullptr; return ctx_fail(D2FE_ERR_HIP, std::string("lk frame: ") + hipGetErrorString(e)); }
  return D2FE_OK;
}

void d2fe_lk_frame_destroy(d2fe_lk_frame f) {
  if (!f) return;
  hipSetDevice(f->device);
  if (f->pyr) hipFree(f->pyr);
  delete f;
}

long d2fe_lk_frame_read_level(d2fe_lk_frame f, int level, uint8_t* dst, size_t max_bytes, int* width, int* height) {
  if (!f || !dst || level < 0 || level > f->levels) return ctx_fail(D2FE_ERR_INVALID, "bad argument");
  const size_t bytes = (size_t)f->ws[level] * f->hs[level];
  if (bytes > max_bytes) return ctx_fail(D2FE_ERR_TRUNCATED, "destination too small");
  LK_TRY(hipSetDevice(f->device));
  LK_TRY(hipDeviceSynchronize());
  LK_TRY(hipMemcpy(dst, f->pyr + f->off[level], bytes, hipMemcpyDeviceToHost));
  if (width) *width = f->ws[level];
  if (height) *height = f->hs[level];
  return (long)bytes;
}

int d2fe_lk_track_batch(d2fe_handle h, const d2fe_lk_pair* pairs, int npairs, const float* prev_pts, const float* cur_init,
                        int n_total, int win, int iters, float* cur_pts, uint8_t* status) {
  if (!h || (npairs > 0 && !pairs) || (n_total > 0 && (!prev_pts || !cur_init || !cur_pts || !status))) return ctx_fail(D2FE_ERR_INVALID, "null argument");
  if (npairs < 0 || npairs > 4096 || n_total < 0 || win < 3 || win > 24 || !(win & 1) || iters < 1) return ctx_fail(D2FE_ERR_INVALID, "bad LK parameters (win odd, 3..23)");
  if (n_total == 0 || npairs == 0) return D2FE_OK;
  // host staging block: [pairs table | pair index per point | prev_pts | cur_init]  -> one H2D; [cur_pts | status] <- one D2H
  const size_t n = (size_t)n_total;
  const size_t o_pairs = 0, o_idx = sizeof(LkPairDev) * (size_t)npairs, o_prev = o_idx + sizeof(int) * n, o_init = o_prev + sizeof(float) * 2 * n;
  const size_t in_bytes = o_init + sizeof(float) * 2 * n;
  const size_t o_cur = (in_bytes + 15) / 16 * 16, o_st = o_cur + sizeof(float) * 2 * n, total = o_st + n;
  std::vector<char> stage(in_bytes);
  LkPairDev* tp = reinterpret_cast<LkPairDev*>(stage.data() + o_pairs);
  int* ti = reinterpret_cast<int*>(stage.data() + o_idx);
  std::vector<char> seen(n, 0);
  for (int p = 0; p < npairs; ++p) {
    const d2fe_lk_pair& q = pairs[p];
    if (!q.prev || !q.cur) return ctx_fail(D2FE_ERR_INVALID, "null frame in pair");
    if (q.prev->w != q.cur->w || q.prev->hgt != q.cur->hgt || q.prev->levels != q.cur->levels) return ctx_fail(D2FE_ERR_INVALID, "pyramid geometry mismatch");
    if (q.type < 0 || q.type > 2 || q.first < 0 || q.count < 0 || (size_t)q.first + (size_t)q.count > n) return ctx_fail(D2FE_ERR_INVALID, "bad pair (type / point range)");
    LkPairDev& d = tp[p];
    memset(&d, 0, sizeof(d));
    d.prev = q.prev->pyr; d.cur = q.cur->pyr;
    for (int l = 0; l < 8; ++l) { d.off[l] = q.prev->off[l]; d.ws[l] = q.prev->ws[l]; d.hs[l] = q.prev->hs[l]; }
    d.levels = q.prev->levels; d.w = q.prev->w; d.h = q.prev->hgt; d.type = q.type; d.move_cols = q.move_cols;
    for (int i = q.first; i < q.first + q.count; ++i) { ti[i] = p; seen[i] = 1; }
  }
  for (size_t i = 0; i < n; ++i) if (!seen[i]) return ctx_fail(D2FE_ERR_INVALID, "point not covered by any pair");
  memcpy(stage.data() + o_prev, prev_pts, sizeof(float) * 2 * n);
  memcpy(stage.data() + o_init, cur_init, sizeof(float) * 2 * n);
  LK_TRY(hipSetDevice(ctx_device(h)));
  hipStream_t s = ctx_stream(h);
  void* raw = nullptr;
  { const int rc0 = ctx_scratch(h, total + 16, &raw); if (rc0 != D2FE_OK) return rc0; }
  char* dev = static_cast<char*>(raw);
  LkArgs a;
  a.pairs = reinterpret_cast<const LkPairDev*>(dev + o_pairs); a.pair_of = reinterpret_cast<const int*>(dev + o_idx);
  a.n = n_total; a.win = win; a.iters = iters;
  a.prev_pts = reinterpret_cast<const float*>(dev + o_prev); a.cur_init = reinterpret_cast<const float*>(dev + o_init);
  a.cur_pts = reinterpret_cast<float*>(dev + o_cur); a.status = reinterpret_cast<uint8_t*>(dev + o_st);
  std::vector<char> back(total - o_cur);
  int rc = D2FE_OK;
  auto chk = [&](hipError_t e, const char* w) { if (e != hipSuccess && rc == D2FE_OK) rc = ctx_fail(D2FE_ERR_HIP, std::string(w) + ": " + hipGetErrorString(e)); };
  chk(hipMemcpyAsync(dev, stage.data(), in_bytes, hipMemcpyHostToDevice, s), "H2D");
  if (rc == D2FE_OK) {
    hipLaunchKernelGGL(lk_track_kernel, dim3((n_total + 3) / 4), dim3(256), 0, s, a);
    chk(hipGetLastError(), "lk_track_kernel");
  }
  chk(hipMemcpyAsync(back.data(), dev + o_cur, back.size(), hipMemcpyDeviceToHost, s), "D2H");
  chk(hipStreamSynchronize(s), "sync");
  if (rc == D2FE_OK) {
    memcpy(cur_pts, back.data(), sizeof(float) * 2 * n);
    memcpy(status, back.data() + (o_st - o_cur), n);
  }
  return rc;
}

size_t d2fe_lk_stereo_workspace_bytes(int n_frames, int width, int height, int levels) {
  if (n_frames < 1 || width < 16 || height < 16 || levels < 0 || levels > 7) return 0;
  size_t total = 0;
  for (int l = 0, w = width, hh = height; l <= levels; ++l) { total += (size_t)w * hh; w = (w + 1) / 2; hh = (hh + 1) / 2; }
  return 2 * (size_t)n_frames * total;
}

// the pyramids of n_frames images alone (the mono pipe's sp_lk chain): the launches d2fe_lk_track_stereo_device issues for its left half, image f's pyramid at
// f * total in d_workspace (half of d2fe_lk_stereo_workspace_bytes); arguments as checked there
extern "C++" {
namespace d2fe {
int lk_pyramids_launch(d2fe_context* h, const uint8_t* d_img, int n_frames, int width, int height, int stride, size_t image_stride, int levels, void* d_workspace,
                       hipStream_t s) {
  if (!h || !d_img || !d_workspace) return ctx_fail(D2FE_ERR_INVALID, "null argument");
  if (width < 16 || height < 16 || levels < 0 || levels > 7 || (size_t)width * height > (1u << 28)) return ctx_fail(D2FE_ERR_INVALID, "bad pyramid geometry");
  if (stride < width || (n_frames > 1 && image_stride < (size_t)stride * (height - 1) + width)) return ctx_fail(D2FE_ERR_INVALID, "bad stride / image stride");
  if (n_frames < 1 || n_frames > 65535) return ctx_fail(D2FE_ERR_INVALID, "n_frames must be 1..65535");
  LK_TRY(hipSetDevice(ctx_device(h)));
  int off[9], ws[9], hs[9], o = 0;
  for (int l = 0, w = width, hh = height; l <= levels; ++l) { off[l] = o; ws[l] = w; hs[l] = hh; o += w * hh; w = (w + 1) / 2; hh = (hh + 1) / 2; }
  PyrBatchArgs a{};
  a.left = d_img; a.right = nullptr; a.src_stride = (size_t)stride; a.src_image_stride = image_stride;      // blockIdx.z < n: the kernel never reads a.right
  a.ws = static_cast<uint8_t*>(d_workspace); a.total = (size_t)o; a.n = n_frames;
  for (int l = 1; l <= (levels > 0 ? levels : 1); ++l) {
    a.first = l == 1;
    a.src_off = off[l - 1]; a.sw = ws[l - 1]; a.sh = hs[l - 1];
    a.dw = (a.sw + 1) / 2; a.dh = (a.sh + 1) / 2; a.dst_off = l <= levels ? off[l] : -1;
    ProfScope ps(h, D2FE_PROF_LK, s);
    hipLaunchKernelGGL(pyr_down_batch_kernel, dim3((a.dw + 63) / 64, (a.dh + 3) / 4, n_frames), dim3(256), 0, s, a);
  }
  LK_TRY(hipGetLastError());
  return D2FE_OK;
}
}  // namespace d2fe
}  // extern "C++"

int d2fe_lk_track_stereo_device(d2fe_handle h, const uint8_t* d_left, const uint8_t* d_right, int n_frames, int width, int height, int stride,
                                size_t image_stride, const float* d_kps_xy, const int32_t* d_n_kp, int cap, int levels, int win, int iters,
                                void* d_workspace, float* d_pts_xy, uint8_t* d_status, void* stream) {
  // d_kps_xy, d_n_kp, d_pts_xy and d_status all NULL: the pyramids alone (the workspace a caller of d2fe_lk_carry_step_device needs)
  const bool tracks = d_kps_xy || d_n_kp || d_pts_xy || d_status;
  if (!h || !d_left || !d_right || !d_workspace || (tracks && (!d_kps_xy || !d_n_kp || !d_pts_xy || !d_status))) return ctx_fail(D2FE_ERR_INVALID, "null argument");
  if (width < 16 || height < 16 || levels < 0 || levels > 7 || (size_t)width * height > (1u << 28)) return ctx_fail(D2FE_ERR_INVALID, "bad pyramid geometry");
  if (stride < width || (n_frames > 1 && image_stride < (size_t)stride * (height - 1) + width)) return ctx_fail(D2FE_ERR_INVALID, "bad stride / image stride");
  if (n_frames < 1 || n_frames > 32767 || (tracks && (cap < 1 || cap > 16384))) return ctx_fail(D2FE_ERR_INVALID, "n_frames must be 1..32767, cap 1..16384");
  if (win < 3 || win > 24 || !(win & 1) || iters < 1) return ctx_fail(D2FE_ERR_INVALID, "bad LK parameters (win odd, 3..23)");
  LK_TRY(hipSetDevice(ctx_device(h)));
  hipStream_t s = stream ? (hipStream_t)stream : ctx_stream(h);
  LkStereoArgs t{};
  LkPairDev& P = t.P;
  int o = 0;
  for (int l = 0, w = width, hh = height; l <= levels; ++l) { P.off[l] = o; P.ws[l] = w; P.hs[l] = hh; o += w * hh; w = (w + 1) / 2; hh = (hh + 1) / 2; }
  P.levels = levels; P.w = width; P.h = height; P.type = 0; P.move_cols = 0.f;
  PyrBatchArgs a{};
  a.left = d_left; a.right = d_right; a.src_stride = (size_t)stride; a.src_image_stride = image_stride;
  a.ws = static_cast<uint8_t*>(d_workspace); a.total = (size_t)o; a.n = n_frames;
  // level 0 (the tight copy) and level 1 in one launch, one launch per deeper level: `levels` launches (levels == 0: the copy alone)
  for (int l = 1; l <= (levels > 0 ? levels : 1); ++l) {
    a.first = l == 1;
    a.src_off = P.off[l - 1]; a.sw = P.ws[l - 1]; a.sh = P.hs[l - 1];
    a.dw = (a.sw + 1) / 2; a.dh = (a.sh + 1) / 2; a.dst_off = l <= levels ? P.off[l] : -1;
    ProfScope ps(h, D2FE_PROF_LK, s);
    hipLaunchKernelGGL(pyr_down_batch_kernel, dim3((a.dw + 63) / 64, (a.dh + 3) / 4, 2 * n_frames), dim3(256), 0, s, a);
  }
  t.ws = a.ws; t.total = a.total; t.n_frames = n_frames; t.cap = cap; t.win = win; t.iters = iters;
  t.kps = d_kps_xy; t.n_kp = d_n_kp; t.cur_pts = d_pts_xy; t.status = d_status;
  if (tracks) {
    ProfScope ps(h, D2FE_PROF_LK, s);
    hipLaunchKernelGGL(lk_track_stereo_kernel, dim3((cap + 3) / 4, n_frames), dim3(256), 0, s, t);
  }
  LK_TRY(hipGetLastError());
  return D2FE_OK;
}

int d2fe_lk_track(d2fe_handle h, d2fe_lk_frame prev, d2fe_lk_frame cur, const float* prev_pts, const float* cur_init, int n,
                  int type, float move_cols, int win, int iters, float* cur_pts, uint8_t* status) {
  if (!prev || !cur) return ctx_fail(D2FE_ERR_INVALID, "null argument");
  d2fe_lk_pair p;
  p.prev = prev; p.cur = cur; p.first = 0; p.count = n; p.type = type; p.move_cols = move_cols;
  return d2fe_lk_track_batch(h, &p, 1, prev_pts, cur_init, n, win, iters, cur_pts, status);
}

int d2fe_detect_fast_by_region(d2fe_handle h, d2fe_lk_frame f, int features, int cols, int rows, int threshold, float* pts_xy,
                               int32_t* response, int cap, int* n_out) {
  if (n_out) *n_out = 0;
  if (!h || !f || !pts_xy || !n_out) return ctx_fail(D2FE_ERR_INVALID, "null argument");
  if (features < 1 || cols < 1 || rows < 1 || cols * rows > 4096 || threshold < 0 || threshold > 254 || cap < 1) return ctx_fail(D2FE_ERR_INVALID, "bad FAST parameters");
  const int w = f->w, hh = f->hgt, sw = w / cols, sh = hh / rows;
  LK_TRY(hipSetDevice(ctx_device(h)));
  hipStream_t s = ctx_stream(h);
  const size_t ocap = (size_t)cols * rows * features;
  const size_t sbytes = (sizeof(int) * (size_t)w * hh + 15) / 16 * 16;   // keeps the int4 list 16-byte aligned
  void* raw = nullptr;
  { const int rc0 = ctx_scratch(h, sbytes + sizeof(int4) * ocap + 16, &raw); if (rc0 != D2FE_OK) return rc0; }
  char* buf = static_cast<char*>(raw);
  int* d_score = reinterpret_cast<int*>(buf);
  int4* d_out = reinterpret_cast<int4*>(buf + sbytes);
  int* d_cnt = reinterpret_cast<int*>(buf + sbytes + sizeof(int4) * ocap);
  int rc = D2FE_OK;
  auto chk = [&](hipError_t e, const char* wh) { if (e != hipSuccess && rc == D2FE_OK) rc = ctx_fail(D2FE_ERR_HIP, std::string(wh) + ": " + hipGetErrorString(e)); };
  chk(hipMemsetAsync(buf, 0, sbytes, s), "memset score");
  chk(hipMemsetAsync(d_cnt, 0, sizeof(int), s), "memset count");
  int cnt = 0;
  std::vector<int4> host;
  if (rc == D2FE_OK && sw > 6 && sh > 6) {
    hipLaunchKernelGGL(fast_region_kernel, dim3(cols * rows), dim3(1024), 0, s, f->pyr, w, sw, sh, rows, (const int*)nullptr, features, threshold, d_score, w);
    hipLaunchKernelGGL(fast_nonmax_kernel, dim3((w + 63) / 64, (hh + 3) / 4), dim3(256), 0, s, d_score, w, hh, sw, sh, cols, rows, d_out, (int)ocap, d_cnt, (const int*)nullptr);
    chk(hipGetLastError(), "fast kernels");
    chk(hipMemcpyAsync(&cnt, d_cnt, sizeof(int), hipMemcpyDeviceToHost, s), "D2H count");
    chk(hipStreamSynchronize(s), "sync");
    if (rc == D2FE_OK && cnt > 0) {
      cnt = std::min<int>(cnt, (int)ocap);
      host.resize(cnt);
      chk(hipMemcpy(host.data(), d_out, sizeof(int4) * (size_t)cnt, hipMemcpyDeviceToHost), "D2H keypoints");
    }
  }
  if (rc != D2FE_OK) return rc;
  // host part of detectFastByRegion (:476-492): sort by response, keep the top `features`
  std::sort(host.begin(), host.end(), [](const int4& p, const int4& q) { return p.z != q.z ? p.z > q.z : p.w < q.w; });
  int n = 0;
  for (const int4& k : host) {
    if (n >= features) break;
    if (n >= cap) { *n_out = n; return ctx_fail(D2FE_ERR_TRUNCATED, "output capacity too small"); }
    pts_xy[2 * n] = (float)k.x; pts_xy[2 * n + 1] = (float)k.y;
    if (response) response[n] = k.z;
    ++n;
  }
  *n_out = n;
  return D2FE_OK;
}

int d2fe_good_features_to_track(d2fe_handle h, d2fe_lk_frame f, int max_corners, double quality, double min_dist, float* pts_xy,
                                int cap, int* n_out) {
  if (n_out) *n_out = 0;
  if (!h || !f || !pts_xy || !n_out) return ctx_fail(D2FE_ERR_INVALID, "null argument");
  if (!(quality > 0) || cap < 1) return ctx_fail(D2FE_ERR_INVALID, "bad parameters");
  const int w = f->w, hh = f->hgt;
  LK_TRY(hipSetDevice(ctx_device(h)));
  hipStream_t s = ctx_stream(h);
  const size_t npix = (size_t)w * hh, np = (npix + 3) / 4 * 4, ccap = npix / 2 + 1024;   // np: plane stride, keeps the 64-bit list aligned
  void* raw = nullptr;
  { const int rc0 = ctx_scratch(h, sizeof(float) * 3 * np + sizeof(unsigned long long) * ccap + 16, &raw); if (rc0 != D2FE_OK) return rc0; }
  char* buf = static_cast<char*>(raw);
  float* d_dx = reinterpret_cast<float*>(buf); float* d_dy = d_dx + np; float* d_eig = d_dy + np;
  unsigned long long* d_c = reinterpret_cast<unsigned long long*>(d_eig + np);
  unsigned* d_max = reinterpret_cast<unsigned*>(d_c + ccap);
  int* d_cnt = reinterpret_cast<int*>(d_max + 1);
  int rc = D2FE_OK;
  auto chk = [&](hipError_t e, const char* wh) { if (e != hipSuccess && rc == D2FE_OK) rc = ctx_fail(D2FE_ERR_HIP, std::string(wh) + ": " + hipGetErrorString(e)); };
  chk(hipMemsetAsync(d_max, 0, 8, s), "memset");
  const double scd = 1.0 / ((double)(1 << 2) * 3.0 * 255.0);
  const dim3 grid((w + 63) / 64, (hh + 3) / 4);
  int cnt = 0;
  std::vector<unsigned long long> keys;
  if (rc == D2FE_OK) {
    hipLaunchKernelGGL(sobel_kernel, grid, dim3(256), 0, s, f->pyr, w, w, hh, (float)scd, (float)(2.0 * scd), d_dx, d_dy);
    hipLaunchKernelGGL(min_eigen_kernel, grid, dim3(256), 0, s, d_dx, d_dy, w, hh, d_eig, d_max);
    hipLaunchKernelGGL(corners_kernel, grid, dim3(256), 0, s, d_eig, w, hh, d_max, quality, d_c, (int)ccap, d_cnt);
    chk(hipGetLastError(), "good-features kernels");
    chk(hipMemcpyAsync(&cnt, d_cnt, sizeof(int), hipMemcpyDeviceToHost, s), "D2H count");
    chk(hipStreamSynchronize(s), "sync");
    if (rc == D2FE_OK && cnt > (int)ccap) rc = ctx_fail(D2FE_ERR_TRUNCATED, "corner candidate buffer overflow");
    if (rc == D2FE_OK && cnt > 0) {
      keys.resize(cnt);
      chk(hipMemcpy(keys.data(), d_c, sizeof(unsigned long long) * (size_t)cnt, hipMemcpyDeviceToHost), "D2H corners");
    }
  }
  if (rc != D2FE_OK) return rc;
  std::sort(keys.begin(), keys.end(), [](unsigned long long p, unsigned long long q) { return p > q; });
  // host min-distance filter of cv::goodFeaturesToTrack / cv::cuda::GoodFeaturesToTrackDetector (grid of cell = round(minDistance))
  int n = 0;
  auto emit = [&](int x, int y) -> bool {
    if (n >= cap) return false;
    pts_xy[2 * n] = (float)x; pts_xy[2 * n + 1] = (float)y;
    ++n;
    return true;
  };
  if (min_dist >= 1) {
    const int cell = (int)std::lrint(min_dist);
    const int gw = (w + cell - 1) / cell, gh = (hh + cell - 1) / cell;
    std::vector<std::vector<int>> grid2((size_t)gw * gh);
    const double md2 = min_dist * min_dist;
    for (unsigned long long k : keys) {
      const int idx = (int)(0xFFFFFFFFu - (unsigned)(k & 0xFFFFFFFFull));
      const int y = idx / w, x = idx % w;
      const int xc = x / cell, yc = y / cell;
      const int x1 = std::max(xc - 1, 0), y1 = std::max(yc - 1, 0), x2 = std::min(xc + 1, gw - 1), y2 = std::min(yc + 1, gh - 1);
      bool good = true;
      for (int yy = y1; yy <= y2 && good; ++yy)
        for (int xx = x1; xx <= x2 && good; ++xx)
          for (int e : grid2[(size_t)yy * gw + xx]) {
            const float ddx = (float)x - (float)(e % w), ddy = (float)y - (float)(e / w);
            if ((double)(ddx * ddx + ddy * ddy) < md2) { good = false; break; }
          }
      if (good) {
        grid2[(size_t)yc * gw + xc].push_back(idx);
        if (!emit(x, y)) { *n_out = n; return ctx_fail(D2FE_ERR_TRUNCATED, "output capacity too small"); }
        if (max_corners > 0 && n == max_corners) break;
      }
    }
  } else {
    for (unsigned long long k : keys) {
      if (max_corners > 0 && n >= max_corners) break;
      const int idx = (int)(0xFFFFFFFFu - (unsigned)(k & 0xFFFFFFFFull));
      if (!emit(idx % w, idx / w)) { *n_out = n; return ctx_fail(D2FE_ERR_TRUNCATED, "output capacity too small"); }
    }
  }
  *n_out = n;
  return D2FE_OK;
}

}  // extern "C"
