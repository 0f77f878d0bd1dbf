// calib.hip -- the int8 calibration session of include/d2fe.h (d2fe_calib_*): the statistics kernels, the session's host side and the three range rules.
// The session runs the exact network through run_superpoint_trunk (superpoint_host.hip) and, behind it on the same stream, one statistics launch per tensor:
// the twelve tensors differ in T, scale and size, a launch costs microseconds against the milliseconds of the network, and one launch per tensor keeps
// one histogram per workgroup in LDS -- a table of tensors in one launch would buy nothing measurable and cost a second level of indexing.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "context.h"

using namespace d2fe;

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int CALIB_THREADS = 256, CALIB_UNROLL = 4;

// one value into the statistics of the thread / the workgroup.  Range phase: mx.  Histogram phase: zeros and over-range values are counted in registers, every
// non-zero value takes one LDS add.  |x| == 0 is tested on the bits (both zeros, and nothing else: subnormals are values)
template <bool HIST>
__device__ __forceinline__ void calib_take(float x, float T, float scale, int last, unsigned* bins, unsigned& mx, unsigned& nz, unsigned& nov) {
  const unsigned bits = __float_as_uint(x) & 0x7fffffffu;
  if (!HIST) { mx = bits > mx ? bits : mx; return; }
  if (bits == 0u) { ++nz; return; }
  const float a = __uint_as_float(bits);
  int b;
  if (a > T) { ++nov; b = last; }
  else { b = (int)(a * scale); b = b < 0 ? 0 : (b > last ? last : b); }      // (the lower clamp: a NaN, outside the contract, must not leave the histogram)
  atomicAdd(&bins[b], 1u);
}

__device__ __forceinline__ unsigned wave_max(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const unsigned w = (unsigned)__shfl_xor((int)v, o, 64); v = w > v ? w : v; }
  return v;
}
__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o, 64);
  return v;
}

// what a workgroup does with its registers and its LDS histogram at the end.  Every wave reduces with shuffles and hands its result to LDS; the workgroup then
// issues ONE global atomic per word it has something for: the integer max (skipped when the word already holds as much: a maximum only grows), n_zero and n_over
// (bins[n_bins], bins[n_bins + 1]) and every non-zero bin, 64-bit adds that return nothing.  One atomic per WAVE on the three shared words was measured first: 4096
// of them to one address held every launch at about 50 us whatever the tensor's size.  A workgroup sees fewer than 2^31 values (the launchers check), so no 32-bit
// counter of it wraps
template <bool HIST>
__device__ __forceinline__ void calib_finish(unsigned* bins, int n_bins, unsigned mx, unsigned nz, unsigned nov, const CalibOut& out) {
  const int lane = threadIdx.x & 63;
  if (!HIST) {
    __shared__ unsigned wg_max;
    if (threadIdx.x == 0) wg_max = 0u;
    __syncthreads();
    mx = wave_max(mx);
    if (lane == 0 && mx) atomicMax(&wg_max, mx);
    __syncthreads();
    if (threadIdx.x == 0 && wg_max > __hip_atomic_load(out.t_max_bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(out.t_max_bits, wg_max);
    return;
  }
  nz = wave_sum(nz); nov = wave_sum(nov);
  if (lane == 0 && nz) atomicAdd(&bins[n_bins], nz);
  if (lane == 0 && nov) atomicAdd(&bins[n_bins + 1], nov);
  __syncthreads();
  for (int b = threadIdx.x; b < n_bins; b += CALIB_THREADS) {
    const unsigned c = bins[b];
    if (c) atomicAdd(out.hist + b, (unsigned long long)c);
  }
  if (threadIdx.x < 2) {
    const unsigned c = bins[n_bins + threadIdx.x];
    if (c) atomicAdd(threadIdx.x ? out.n_over : out.n_zero, (unsigned long long)c);
  }
}

// The statistics of an NHWC fp32 tensor view: value (p, c) at base[p * ch_stride + ch_off + c].  VEC: channels, offset and stride are multiples of 4 and the base
// is 16-byte aligned -- 16-byte loads; else (the 65 logits) scalar loads.  Thread t of the launch takes the units t, t + threads, ...: consecutive lanes read
// consecutive addresses, and (pixel, unit in pixel) advance by a constant step with one carry, no division in the loop
template <bool HIST, bool VEC>
__global__ __launch_bounds__(CALIB_THREADS) void calib_stats_kernel(const float* __restrict__ base, long long pixels, int ch_off, int channels, int ch_stride, float T,
                                                                    float scale, int n_bins, CalibOut out) {
  extern __shared__ unsigned bins[];
  if (HIST) {
    for (int b = threadIdx.x; b < n_bins + 2; b += CALIB_THREADS) bins[b] = 0u;      // the histogram, n_zero, n_over
    __syncthreads();
  }
  unsigned mx = 0u, nz = 0u, nov = 0u;
  const int last = n_bins - 1;
  const unsigned upp = (unsigned)(VEC ? channels >> 2 : channels);      // units per pixel
  const unsigned long long units = (unsigned long long)pixels * upp, step = (unsigned long long)gridDim.x * CALIB_THREADS;
  unsigned long long u = (unsigned long long)blockIdx.x * CALIB_THREADS + threadIdx.x;
  unsigned long long p = u / upp;
  unsigned q = (unsigned)(u % upp);
  const unsigned long long dp = step / upp;
  const unsigned dq = (unsigned)(step % upp);
  // CALIB_UNROLL independent loads are issued per thread before the first of their values is binned
  while (u < units) {
    f32x4 v[CALIB_UNROLL];
    bool have[CALIB_UNROLL];
#pragma unroll
    for (int k = 0; k < CALIB_UNROLL; ++k) {
      have[k] = u < units;
      if (have[k]) {
        const float* src = base + p * (unsigned long long)ch_stride + ch_off + (VEC ? 4u * q : q);
        if (VEC) v[k] = *reinterpret_cast<const f32x4*>(src);
        else v[k][0] = *src;
      }
      u += step; p += dp; q += dq;
      if (q >= upp) { q -= upp; ++p; }
    }
#pragma unroll
    for (int k = 0; k < CALIB_UNROLL; ++k) {
      if (!have[k]) continue;
#pragma unroll
      for (int j = 0; j < (VEC ? 4 : 1); ++j) calib_take<HIST>(v[k][j], T, scale, last, bins, mx, nz, nov);
    }
  }
  calib_finish<HIST>(bins, n_bins, mx, nz, nov, out);
}

// conv1a + ReLU from the u8 frames into the same statistics; the activation is never written.  The arithmetic is conv1a_kernel's (conv.hip): thread = (pixel,
// group of 16 output channels), (float)u8 * (1/255), the fmaf chain in (ky, kx) order from the bias -- the bits of launch_conv1a's output, whichever of its two
// kernels runs.  Persistent workgroups walk the (image, row, 64-pixel block) items, so a workgroup flushes its histogram once
template <bool HIST>
__global__ __launch_bounds__(CALIB_THREADS) void calib_conv1a_stats_kernel(const uint8_t* __restrict__ img, int stride, long img_stride, int H, int W, int xblocks,
                                                                           long items, const float* __restrict__ w9x64, const float* __restrict__ bias, float T,
                                                                           float scale, int n_bins, CalibOut out) {
  extern __shared__ unsigned bins[];
  if (HIST) {
    for (int b = threadIdx.x; b < n_bins + 2; b += CALIB_THREADS) bins[b] = 0u;      // the histogram, n_zero, n_over
    __syncthreads();
  }
  unsigned mx = 0u, nz = 0u, nov = 0u;
  const int last = n_bins - 1;
  const int g = threadIdx.x & 3;
  // this thread's 16 channels of the nine taps and the bias stay in registers over the whole walk: 160 of them, two waves per SIMD, which VALU work does not mind
  float wr[9][16], br[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) br[c] = bias[g * 16 + c];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int c = 0; c < 16; ++c) wr[t][c] = w9x64[t * 64 + g * 16 + c];
  const float s255 = (float)(1.0 / 255.0);
  for (long item = blockIdx.x; item < items; item += gridDim.x) {
    const int x = (int)(item % xblocks) * 64 + (threadIdx.x >> 2);
    const long row = item / xblocks;      // n * H + y
    const int y = (int)(row % H);
    if (x >= W) continue;
    const uint8_t* ip = img + (size_t)(row / H) * img_stride;
    float v[9];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int yy = y + ky - 1, xx = x + kx - 1;
        v[ky * 3 + kx] = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? (float)ip[(size_t)yy * stride + xx] * s255 : 0.f;
      }
    float acc[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) acc[c] = br[c];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int c = 0; c < 16; ++c) acc[c] = __builtin_fmaf(v[t], wr[t][c], acc[c]);
#pragma unroll
    for (int c = 0; c < 16; ++c) calib_take<HIST>(acc[c] > 0.f ? acc[c] : 0.f, T, scale, last, bins, mx, nz, nov);
  }
  calib_finish<HIST>(bins, n_bins, mx, nz, nov, out);
}

// workgroups of a launch over `units` thread-iterations: enough to fill the device four deep, no more than the work has
int calib_grid(unsigned long long units, int ncu) {
  const unsigned long long want = (units + CALIB_THREADS - 1) / CALIB_THREADS, most = (unsigned long long)(ncu > 0 ? ncu : 256) * 4;
  return (int)(want < 1 ? 1 : (want < most ? want : most));
}

}  // namespace

namespace d2fe {

hipError_t launch_calib_stats(const float* base, long long pixels, int ch_off, int channels, int ch_stride, bool hist_phase, float T, float scale, int n_bins,
                              const CalibOut& out, int ncu, int wgs, hipStream_t s) {
  if (!base || pixels < 1 || channels < 1 || ch_off < 0 || ch_off + channels > ch_stride || !calib_bins_ok(n_bins) || wgs < 0 || wgs > 65536) return hipErrorInvalidValue;
  const bool vec = !((channels | ch_off | ch_stride) & 3) && !((uintptr_t)base & 15);
  const unsigned long long units = (unsigned long long)pixels * (vec ? channels >> 2 : channels);
  const int grid = wgs ? wgs : calib_grid(units, ncu);
  // a workgroup's 32-bit counters: its share of the values stays below 2^32
  if (((unsigned long long)pixels * channels) / grid >= (1ull << 31)) return hipErrorInvalidValue;
  const size_t lds = hist_phase ? sizeof(unsigned) * (n_bins + 2) : 0;
#define CALIB_LAUNCH(H_, V_) hipLaunchKernelGGL((calib_stats_kernel<H_, V_>), dim3(grid), dim3(CALIB_THREADS), lds, s, base, pixels, ch_off, channels, ch_stride, T, scale, n_bins, out)
  if (hist_phase) { if (vec) CALIB_LAUNCH(true, true); else CALIB_LAUNCH(true, false); }
  else { if (vec) CALIB_LAUNCH(false, true); else CALIB_LAUNCH(false, false); }
#undef CALIB_LAUNCH
  return hipGetLastError();
}

hipError_t launch_calib_conv1a_stats(const uint8_t* img, int stride, long img_stride_bytes, int H, int W, int n, const float* w9x64, const float* bias,
                                     bool hist_phase, float T, float scale, int n_bins, const CalibOut& out, int ncu, hipStream_t s) {
  if (!img || !w9x64 || !bias || H < 1 || W < 1 || n < 1 || stride < W || !calib_bins_ok(n_bins)) return hipErrorInvalidValue;
  const int xblocks = (W + 63) / 64;
  const long items = (long)xblocks * H * n;
  const int grid = calib_grid((unsigned long long)items * CALIB_THREADS, ncu);      // one workgroup per item up to four per compute unit (two are resident)
  if ((unsigned long long)items * 4096 / grid >= (1ull << 31)) return hipErrorInvalidValue;
  const size_t lds = hist_phase ? sizeof(unsigned) * (n_bins + 2) : 0;
  if (hist_phase)
    hipLaunchKernelGGL((calib_conv1a_stats_kernel<true>), dim3(grid), dim3(CALIB_THREADS), lds, s, img, stride, img_stride_bytes, H, W, xblocks, items, w9x64, bias, T,
                       scale, n_bins, out);
  else
    hipLaunchKernelGGL((calib_conv1a_stats_kernel<false>), dim3(grid), dim3(CALIB_THREADS), lds, s, img, stride, img_stride_bytes, H, W, xblocks, items, w9x64, bias, T,
                       scale, n_bins, out);
  return hipGetLastError();
}

// ---- the range rules (host, double precision, sequential loops: tests/helpers/calib_oracle.py follows the same order) ----
namespace {
float calib_clamp(float r) { return r < 1e-30f ? 1e-30f : (r > 1e30f ? 1e30f : r); }
float calib_edge(int k, float T, int n_bins) { return calib_clamp((float)((double)k * (double)T / (double)n_bins)); }

// the winning candidate i of the entropy rule; N > 0
int calib_entropy_index(const unsigned long long* hist, int n_bins) {
  std::vector<unsigned long long> tail(n_bins + 1, 0);      // tail[i] = the sum of hist[i ..)
  for (int b = n_bins - 1; b >= 0; --b) tail[b] = tail[b + 1] + hist[b];
  std::vector<double> P(n_bins), Q(n_bins);
  int best = n_bins;
  double best_kl = INFINITY;
  bool have = false;
  for (int i = CALIB_LEVELS; i <= n_bins; ++i) {
    for (int b = 0; b < i; ++b) P[b] = (double)hist[b];
    P[i - 1] = (double)(hist[i - 1] + tail[i]);
    for (int j = 0; j < CALIB_LEVELS; ++j) {
      const int lo = (int)((long long)j * i / CALIB_LEVELS), hi = (int)((long long)(j + 1) * i / CALIB_LEVELS);      // [lo, hi)
      unsigned long long raw = 0;
      int nz = 0;
      for (int b = lo; b < hi; ++b) { raw += hist[b]; nz += P[b] != 0.0; }
      for (int b = lo; b < hi; ++b) Q[b] = P[b] != 0.0 ? (double)raw / (double)nz : 0.0;
    }
    double sp = 0.0, sq = 0.0;
    for (int b = 0; b < i; ++b) sp += P[b];
    for (int b = 0; b < i; ++b) sq += Q[b];
    bool ok = sq > 0.0;
    double kl = 0.0;
    for (int b = 0; ok && b < i; ++b) {
      if (!(P[b] > 0.0)) continue;
      if (!(Q[b] > 0.0)) { ok = false; break; }
      const double p = P[b] / sp, q = Q[b] / sq;
      kl += p * std::log(p / q);
    }
    if (!ok) continue;
    if (!have || kl < best_kl) { have = true; best_kl = kl; best = i; }
  }
  return best;
}
}  // namespace

int calib_range_from_hist(const unsigned long long* hist, int n_bins, float T, int method, double param, float* range, int* index) {
  if (!range || !calib_bins_ok(n_bins) || !(T >= 1e-30f) || std::isinf(T)) return fail(D2FE_ERR_INVALID, "calibration: null range, a bad n_bins or a T that is not finite and at least 1e-30");
  if (method != D2FE_CALIB_MINMAX && method != D2FE_CALIB_ENTROPY && method != D2FE_CALIB_PERCENTILE) return fail(D2FE_ERR_INVALID, "calibration: unknown method");
  if (method == D2FE_CALIB_PERCENTILE && !(param > 0.0 && param <= 100.0)) return fail(D2FE_ERR_INVALID, "calibration: the percentile must lie in (0, 100]");
  if (method != D2FE_CALIB_MINMAX && !hist) return fail(D2FE_ERR_INVALID, "calibration: null histogram");
  int k = n_bins;
  if (method != D2FE_CALIB_MINMAX) {
    unsigned long long N = 0;
    for (int b = 0; b < n_bins; ++b) N += hist[b];
    if (N > 0 && method == D2FE_CALIB_PERCENTILE) {
      const unsigned long long target = (unsigned long long)std::ceil((double)N * (param / 100.0));
      unsigned long long cum = 0;
      for (int b = 0; b < n_bins; ++b) { cum += hist[b]; if (cum >= target) { k = b + 1; break; } }
    } else if (N > 0) {
      k = calib_entropy_index(hist, n_bins);
    }
  }
  *range = k == n_bins ? calib_clamp(T) : calib_edge(k, T, n_bins);
  if (index) *index = k;
  return D2FE_OK;
}

}  // namespace d2fe

// ---- the session ----
struct d2fe_calib_s {
  d2fe_context* h = nullptr;
  int n_bins = 0;
  bool frozen = false;
  long long images = 0;                        // collected in the current phase
  unsigned long long n_total[SP_NLAYERS] = {};      // values seen in the current phase: a count the host knows, no counter on the device
  float t_max[SP_NLAYERS] = {}, T[SP_NLAYERS] = {}, scale[SP_NLAYERS] = {};      // from the freeze on
  // device: [layer] max bits | [layer][2] n_zero, n_over | [layer][n_bins] histograms
  unsigned int* d_max = nullptr;
  unsigned long long* d_cnt = nullptr;
  unsigned long long* d_hist = nullptr;
  DevPool pool;
  CalibOut out(int layer) const { return CalibOut{d_max + layer, d_hist + (size_t)layer * n_bins, d_cnt + 2 * layer, d_cnt + 2 * layer + 1}; }
};

namespace {

// the statistics launches of one network pass over n images of H x W, behind it on s
int calib_launch_all(d2fe_calib c, const uint8_t* d_gray, int n, int W, int H, hipStream_t s) {
  d2fe_context* h = c->h;
  const SpRun& run = h->sp_run;
  const long cells = (long)n * (H >> SP_CELL_LEVEL) * (W >> SP_CELL_LEVEL);
  struct View { const float* base; long long pixels; int off, ch, cs; } v[SP_NLAYERS];
  for (int i = SP_1B; i <= SP_4B; ++i) v[i] = {run.act[i], (long long)n * sp_out_h(i, H) * sp_out_w(i, W), 0, SP_PLAN[i].cout, SP_PLAN[i].cout};
  v[SP_PA] = {run.act[SP_PA], cells, 0, SP_PLAN[SP_PA].cout, SP_PADA_COUT};
  v[SP_DA] = {run.act[SP_PA], cells, SP_PLAN[SP_PA].cout, SP_PLAN[SP_DA].cout, SP_PADA_COUT};
  v[SP_PB] = {run.logits, cells, 0, 65, 65};
  v[SP_DB] = {run.draw, cells, 0, 256, 256};
  HIP_TRY(launch_calib_conv1a_stats(d_gray, W, (long)W * H, H, W, n, h->sp_net->w1a, h->sp_net->b1a, c->frozen, c->T[SP_1A], c->scale[SP_1A], c->n_bins, c->out(SP_1A),
                                    h->ncu, s));
  c->n_total[SP_1A] += (unsigned long long)n * H * W * 64;
  for (int i = SP_1B; i < SP_NLAYERS; ++i) {
    HIP_TRY(launch_calib_stats(v[i].base, v[i].pixels, v[i].off, v[i].ch, v[i].cs, c->frozen, c->T[i], c->scale[i], c->n_bins, c->out(i), h->ncu, 0, s));
    c->n_total[i] += (unsigned long long)v[i].pixels * v[i].ch;
  }
  return D2FE_OK;
}

int calib_read_max(d2fe_calib c, float* t_max) {      // synchronises
  unsigned int bits[SP_NLAYERS];
  HIP_TRY(hipSetDevice(c->h->cfg.device_id));
  HIP_TRY(hipStreamSynchronize(c->h->stream));
  HIP_TRY(hipMemcpy(bits, c->d_max, sizeof(bits), hipMemcpyDeviceToHost));
  memcpy(t_max, bits, sizeof(bits));
  return D2FE_OK;
}

}  // namespace

extern "C" {

int d2fe_calib_create(d2fe_handle h, int n_bins, d2fe_calib* out) {
  if (out) *out = nullptr;
  if (n_bins == 0) n_bins = CALIB_BINS_DEFAULT;
  if (!calib_bins_ok(n_bins)) return fail(D2FE_ERR_INVALID, "n_bins must be 0 (2048) or 128 .. 4096 in multiples of 128");
  if (!h || !out) return fail(D2FE_ERR_INVALID, "null argument");
  if (h->cfg.precision != D2FE_PREC_F32 || !h->cfg.dense_descriptors)
    return fail(D2FE_ERR_INVALID, "a calibration session needs a D2FE_PREC_F32 handle with dense_descriptors = 1 (the statistics are those of the exact network)");
  if (!h->stage) return fail(D2FE_ERR_INVALID, "a calibration session needs a handle of d2fe_create");
  if (!h->sp_net->sp_loaded) return fail(D2FE_ERR_NOT_READY, "superpoint weights not loaded");
  if (h->life.pipes() > 0) return fail(D2FE_ERR_INVALID, "the handle has live pipes or a live calibration session: destroy them first");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  d2fe_calib c = new d2fe_calib_s();
  c->h = h; c->n_bins = n_bins;
  const int rc = [&]() -> int {
    HIP_TRY(c->pool.get(&c->d_max, sizeof(unsigned int) * SP_NLAYERS, nullptr, 0));
    HIP_TRY(c->pool.get(&c->d_cnt, sizeof(unsigned long long) * 2 * SP_NLAYERS, nullptr, 0));
    HIP_TRY(c->pool.get(&c->d_hist, sizeof(unsigned long long) * (size_t)n_bins * SP_NLAYERS, nullptr, 0));
    HIP_TRY(hipDeviceSynchronize());      // the fills ran on the null stream, the handle's stream does not wait for it
    return D2FE_OK;
  }();
  if (rc) { delete c; return rc; }
  h->life.pipe_added();
  *out = c;
  return D2FE_OK;
}

void d2fe_calib_destroy(d2fe_calib c) {
  if (!c) return;
  d2fe_context* h = c->h;
  (void)hipSetDevice(h->cfg.device_id);
  (void)hipStreamSynchronize(h->stream);
  delete c;
  if (h->life.pipe_gone()) d2fe_destroy(h);      // a handle destroyed under the session was only marked, as under a pipe
}

int d2fe_calib_collect(d2fe_calib c, const uint8_t* gray, int width, int height, int stride, long long image_stride, int n) {
  if (!c || !gray) return fail(D2FE_ERR_INVALID, "null argument");
  d2fe_context* h = c->h;
  if (n < 1) return fail(D2FE_ERR_INVALID, "n < 1");
  { const int rc = check_geometry(h, 1, width, height, stride, 1); if (rc) return rc; }
  if (image_stride < (long long)stride * (height - 1) + width) return fail(D2FE_ERR_INVALID, "image_stride smaller than an image");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  hipStream_t s = h->stream;
  if (h->cfg.async_tail)      // an extract call's tail may still read the buffers the network writes
    for (int i = 0; i < 2; ++i) HIP_TRY(hipStreamWaitEvent(s, h->ev_tail[i], 0));
  uint8_t* const d_img = h->stage->s_img;      // max_batch images of the handle's maximum size; the slices reuse it in stream order
  int rc = D2FE_OK;
  for (int i0 = 0; i0 < n && rc == D2FE_OK; i0 += h->cfg.max_batch) {
    const int m = n - i0 < h->cfg.max_batch ? n - i0 : h->cfg.max_batch;
    for (int i = 0; i < m && rc == D2FE_OK; ++i)
      if (hipMemcpy2DAsync(d_img + (size_t)i * width * height, width, gray + (size_t)(i0 + i) * image_stride, stride, width, height, hipMemcpyHostToDevice, s) != hipSuccess)
        rc = fail(D2FE_ERR_HIP, "calibration: frame upload");
    if (rc == D2FE_OK) rc = run_superpoint_trunk(h, d_img, m, width, height, width, (size_t)width * height, s);
    if (rc == D2FE_OK) rc = calib_launch_all(c, d_img, m, width, height, s);
    if (rc == D2FE_OK) c->images += m;
  }
  if (hipStreamSynchronize(s) != hipSuccess && rc == D2FE_OK) rc = fail(D2FE_ERR_HIP, "calibration: hipStreamSynchronize");
  return rc;
}

int d2fe_calib_freeze(d2fe_calib c) {
  if (!c) return fail(D2FE_ERR_INVALID, "null session");
  if (c->frozen) return fail(D2FE_ERR_INVALID, "the session is frozen already");
  if (c->images < 1) return fail(D2FE_ERR_NOT_READY, "no image collected yet");
  { const int rc = calib_read_max(c, c->t_max); if (rc) return rc; }
  for (int i = 0; i < SP_NLAYERS; ++i) {
    c->T[i] = c->t_max[i] > 1e-30f ? c->t_max[i] : 1e-30f;
    c->scale[i] = (float)c->n_bins / c->T[i];
    c->n_total[i] = 0;
  }
  HIP_TRY(hipMemset(c->d_cnt, 0, sizeof(unsigned long long) * 2 * SP_NLAYERS));
  HIP_TRY(hipMemset(c->d_hist, 0, sizeof(unsigned long long) * (size_t)c->n_bins * SP_NLAYERS));
  HIP_TRY(hipDeviceSynchronize());
  c->images = 0;
  c->frozen = true;
  return D2FE_OK;
}

int d2fe_calib_stats_get(d2fe_calib c, int layer, float* t_max, uint64_t* hist, uint64_t* n_zero, uint64_t* n_over, uint64_t* n_total) {
  if (layer < 0 || layer >= SP_NLAYERS) return fail(D2FE_ERR_INVALID, "layer out of range");
  if (!c) return fail(D2FE_ERR_INVALID, "null session");
  if (hist && !c->frozen) return fail(D2FE_ERR_NOT_READY, "the histograms exist from d2fe_calib_freeze on");
  HIP_TRY(hipSetDevice(c->h->cfg.device_id));
  HIP_TRY(hipStreamSynchronize(c->h->stream));
  if (t_max) {
    if (c->frozen) *t_max = c->t_max[layer];
    else { float m[SP_NLAYERS]; const int rc = calib_read_max(c, m); if (rc) return rc; *t_max = m[layer]; }
  }
  unsigned long long cnt[2] = {0, 0};
  if (c->frozen && (n_zero || n_over)) HIP_TRY(hipMemcpy(cnt, c->d_cnt + 2 * layer, sizeof(cnt), hipMemcpyDeviceToHost));
  if (n_zero) *n_zero = cnt[0];
  if (n_over) *n_over = cnt[1];
  if (n_total) *n_total = c->n_total[layer];
  static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "the counters are 64-bit");
  if (hist) HIP_TRY(hipMemcpy(hist, c->d_hist + (size_t)layer * c->n_bins, sizeof(uint64_t) * c->n_bins, hipMemcpyDeviceToHost));
  return D2FE_OK;
}

int d2fe_calib_ranges(d2fe_calib c, int method, double param, float* range) {
  if (method != D2FE_CALIB_MINMAX && method != D2FE_CALIB_ENTROPY && method != D2FE_CALIB_PERCENTILE) return fail(D2FE_ERR_INVALID, "calibration: unknown method");
  if (method == D2FE_CALIB_PERCENTILE && !(param > 0.0 && param <= 100.0)) return fail(D2FE_ERR_INVALID, "calibration: the percentile must lie in (0, 100]");
  if (!c || !range) return fail(D2FE_ERR_INVALID, "null session or range");
  if (method != D2FE_CALIB_MINMAX && !c->frozen) return fail(D2FE_ERR_NOT_READY, "the entropy and percentile rules need the histogram phase (d2fe_calib_freeze, then collect)");
  if (c->images < 1 && !c->frozen) return fail(D2FE_ERR_NOT_READY, "no image collected yet");
  float T[SP_NLAYERS];
  if (c->frozen) memcpy(T, c->T, sizeof(T));
  else {
    const int rc = calib_read_max(c, T); if (rc) return rc;
    for (float& t : T) t = t > 1e-30f ? t : 1e-30f;
  }
  std::vector<unsigned long long> hist(method == D2FE_CALIB_MINMAX ? 0 : (size_t)c->n_bins * SP_NLAYERS);
  if (!hist.empty()) {
    HIP_TRY(hipSetDevice(c->h->cfg.device_id));
    HIP_TRY(hipStreamSynchronize(c->h->stream));
    HIP_TRY(hipMemcpy(hist.data(), c->d_hist, sizeof(unsigned long long) * hist.size(), hipMemcpyDeviceToHost));
  }
  for (int i = 0; i < SP_NLAYERS; ++i) {
    const int rc = calib_range_from_hist(hist.empty() ? nullptr : hist.data() + (size_t)i * c->n_bins, c->n_bins, T[i], method, param, range + i, nullptr);
    if (rc) return rc;
  }
  return D2FE_OK;
}

}  // extern "C"
