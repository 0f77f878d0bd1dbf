// fast_device.h -- the FAST-9/16 kernels of detectFastByRegion (opticaltrack_utils.cpp:444-493; cv::cuda::FastFeatureDetector, evaluation order of
// oracle/d2fe_oracle_lk.c), shared by the translation units that launch them: lk.hip (d2fe_detect_fast_by_region, the count a host argument) and lk_flow.hip
// (d2fe_detect_fast_device and the flow list, the count one int32 in device memory).  Internal.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace d2fe {
namespace {

// m = max over the 16 arcs of 9 contiguous circle pixels of min(q - v) (bright) and of min(v - q) (dark):
// the pixel is a corner at threshold t iff m > t, and OpenCV's CUDA cornerScore (largest passing threshold) is m - 1.
__device__ __forceinline__ int fast_strength(const uint8_t* __restrict__ p, int stride) {
  const int DX[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
  const int DY[16] = {3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3};
  const int v = p[0];
  int d[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) d[k] = (int)p[DY[k] * stride + DX[k]] - v;
  int best = -256;
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    int mn = 256, mx = -256;
#pragma unroll
    for (int k = 0; k < 9; ++k) { const int q = d[(s + k) & 15]; mn = min(mn, q); mx = max(mx, q); }
    best = max(best, max(mn, -mx));
  }
  return best;
}

// one workgroup per region: raster scan of the region interior in chunks of 1024 pixels; the first `features` corners (raster
// order -- the deterministic stand-in for the CUDA detector's atomics-ordered max_npoints cap) get their score written.  The bodies are device functions so that
// lk_flow.hip's four-camera launches run them with one camera's image, count and score map; the single-image kernels below only call them
__device__ __forceinline__ void fast_region_body(const uint8_t* __restrict__ img, int stride, int sw, int sh, int rows, int features, int threshold,
                                                 int* __restrict__ score, int w, int region) {
  __shared__ int wsum[16];
  __shared__ int s_base;
  const int ri = region / rows, rj = region % rows;
  const int x0 = sw * ri, y0 = sh * rj;
  const int iw = sw - 6, ih = sh - 6;
  if (iw <= 0 || ih <= 0) return;
  const int total = iw * ih;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (tid == 0) s_base = 0;
  __syncthreads();
  for (int c0 = 0; c0 < total; c0 += 1024) {
    const int idx = c0 + tid;
    int m = -256, gx = 0, gy = 0;
    if (idx < total) {
      gx = x0 + 3 + idx % iw; gy = y0 + 3 + idx / iw;
      m = fast_strength(img + (size_t)gy * stride + gx, stride);
    }
    const bool flag = m > threshold;
    const unsigned long long bal = __ballot(flag);
    const int inw = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[wv] = __popcll(bal);
    __syncthreads();
    int pre = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) { const int c = wsum[k]; pre += k < wv ? c : 0; tot += c; }
    const int base = s_base;
    if (flag && base + pre + inw < features) score[(size_t)gy * w + gx] = m - 1;
    __syncthreads();
    if (tid == 0) s_base = base + tot;
    __syncthreads();
    if (base + tot >= features) break;
  }
}

__global__ __launch_bounds__(1024) void fast_region_kernel(const uint8_t* __restrict__ img, int stride, int sw, int sh, int rows,
                                                           const int* __restrict__ d_features, int features, int threshold, int* __restrict__ score, int w) {
  // the count of the device detector: read where the step before left it, never above the `features` its candidate pool was sized for; <= 0: nothing to do
  if (d_features) features = min(features, __builtin_amdgcn_readfirstlane(d_features[0]));
  if (features <= 0) return;
  fast_region_body(img, stride, sw, sh, rows, features, threshold, score, w, blockIdx.x);
}

// non-max suppression (strictly greater than the 8 neighbours) + emit {x, y, response, order}: pixel (x, y) of one score map
__device__ __forceinline__ void fast_nonmax_body(const int* __restrict__ score, int w, int h, int sw, int sh, int cols, int rows, int4* __restrict__ out, int cap,
                                                 int* __restrict__ count, int x, int y) {
  if (x < 1 || y < 1 || x >= w - 1 || y >= h - 1) return;
  const int s = score[(size_t)y * w + x];
  if (s <= 0) return;
  const int* r0 = score + (size_t)(y - 1) * w + x; const int* r1 = r0 + w; const int* r2 = r1 + w;
  if (s > r0[-1] && s > r0[0] && s > r0[1] && s > r1[-1] && s > r1[1] && s > r2[-1] && s > r2[0] && s > r2[1]) {
    const int ri = x / sw, rj = y / sh;
    if (ri >= cols || rj >= rows) return;
    const int order = (ri * rows + rj) * (sw * sh) + (y - sh * rj) * sw + (x - sw * ri);
    const int k = atomicAdd(count, 1);
    if (k < cap) out[k] = int4{x, y, s, order};
  }
}

__global__ __launch_bounds__(256) void fast_nonmax_kernel(const int* __restrict__ score, int w, int h, int sw, int sh, int cols,
                                                          int rows, int4* __restrict__ out, int cap, int* __restrict__ count,
                                                          const int* __restrict__ d_features) {
  if (d_features && d_features[0] <= 0) return;
  fast_nonmax_body(score, w, h, sw, sh, cols, rows, out, cap, count, blockIdx.x * 64 + (threadIdx.x & 63), blockIdx.y * 4 + (threadIdx.x >> 6));
}

}  // namespace
}  // namespace d2fe
