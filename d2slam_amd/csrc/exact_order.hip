// exact_order.hip -- the exact_order option of D2FE_PREC_F32_WINO handles (include/d2fe.h): the keypoint list of the Winograd mode made
// position-by-position equal to the list of D2FE_PREC_F32 ("exact_order").
//
// The Winograd scores s_w differ from the direct fmaf chains' s_d by at most eps.  Candidates are emitted with s_w > thr - eps; the kernels here
//   1. MARK the candidates whose place in the list the deviation could change: |s_w - thr| <= eps (unless more than K candidates lie above thr + eps: the
//      threshold then decides neither the count's side of K nor a place in the top K), and, inside the prefix of the sorted list that can reach the top K
//      (s_w >= s_w[K-1] - 2 eps, or everything when there are fewer than K), every candidate within 2 eps of a sorted neighbour;
//   2. collect the distinct 8x8 cells of the marked candidates, in sorted-list order, and hand out the call's crop slots in image order;
//   3. GATHER an 88x88 crop of the u8 frame around every cell that got a slot (84 pixels is the receptive field of a score cell);
//      ... the crops run through the direct convolution kernels as one batch of 88x88 images (superpoint_host.hip) ...
//   4. PATCH the direct scores of the re-evaluated cells onto the candidates and drop those whose final score is not > thr.
// The ordinary selection (select_b_kernel) then runs on the patched list.  Fixed launch shapes, no host synchronisation.
#include <limits.h>

#include "kernels.h"

namespace d2fe {

namespace {
constexpr int EO_THREADS = 1024;
constexpr int EO_MAXSORT = 16384;     // keys the in-LDS bitonic sort takes (128 KiB of the 160 KiB LDS), as in select_b_kernel
constexpr int EO_CROP = 88;           // crop edge: the cell's 8 pixels + 40 on each side (38 needed), origin a multiple of 8
constexpr int EO_NONE = INT_MAX;      // cell map: no slot

__device__ __forceinline__ int eo_origin(int c8, int extent) {      // crop origin along one axis for cell coordinate c8 (extent: W or H, a multiple of 8, >= 88)
  const int o = 8 * c8 - 40;
  return o < 0 ? 0 : (o > extent - EO_CROP ? extent - EO_CROP : o);
}

// a load that sees what the other waves of the workgroup wrote to HBM (their atomics and stores land in L2; a plain load may be served by the CU's L1)
__device__ __forceinline__ int eo_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// exclusive rank of the threads with `flag` among all threads of the block, in thread order; *total: the block's count.  Two barriers inside.
__device__ __forceinline__ int eo_block_rank(bool flag, int* s_wcnt, int* total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const unsigned long long m = __ballot(flag);
  __syncthreads();      // the previous round's readers of s_wcnt are done
  if (lane == 0) s_wcnt[wv] = __popcll(m);
  __syncthreads();
  int off = 0, tot = 0;
  for (int w = 0; w < EO_THREADS / 64; ++w) { const int c = s_wcnt[w]; if (w < wv) off += c; tot += c; }
  *total = tot;
  return off + __popcll(m & ((1ull << lane) - 1ull));
}

// slots handed to the images in front of `img` (each image asks for min(its distinct marked cells, slots))
__device__ __forceinline__ int eo_slot_base(const int* __restrict__ cell_count, int img, int slots) {
  int base = 0;
  for (int j = 0; j < img && base < slots; ++j) base += min(cell_count[j], slots);
  return min(base, slots);
}
}  // namespace

// One workgroup per image.  cell_map [img][ncell]: on return the rank (0 .. slots-1) of a cell among the image's marked cells, EO_NONE for every other cell;
// cell_list [img][slots]: rank -> cell; cell_count [img]: distinct marked cells (may exceed `slots`); stats[0] += marked candidates.
// More than EO_MAXSORT keys in the part of the list that matters (prefix + threshold band; eps far beyond the measured deviation): every candidate of
// that part is marked and the cells are ranked by cell index instead of sorted-list position -- more cells than the rule asks for, never fewer.
__global__ __launch_bounds__(EO_THREADS) void exact_order_mark_kernel(const unsigned long long* __restrict__ cand, const int* __restrict__ cand_count, long cand_cap,
                                                                     int W, int Wc, int ncell, int K, float thr, float eps, int slots,
                                                                     int* __restrict__ cell_map, int* __restrict__ cell_list, int* __restrict__ cell_count,
                                                                     unsigned long long* __restrict__ stats) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long keys[];      // [EO_MAXSORT]
  __shared__ int hist[256];
  __shared__ int s_digit, s_need, s_cnt, s_marked, s_sure;
  __shared__ int s_wcnt[EO_THREADS / 64];
  const int img = blockIdx.x, tid = threadIdx.x;
  const unsigned long long* c = cand + (size_t)img * cand_cap;
  long n = cand_count[img];
  if (n > cand_cap) n = cand_cap;
  int* cmap = cell_map + (size_t)img * ncell;
  int* clist = cell_list + (size_t)img * slots;
  for (int i = tid; i < ncell; i += EO_THREADS) cmap[i] = EO_NONE;
  __threadfence();      // in L2 before the barriers in front of the first atomicMin on them
  if (tid == 0) { s_cnt = 0; s_marked = 0; s_sure = 0; }
  __syncthreads();
  // Candidates that pass the threshold whatever the deviation (s_w > thr + eps).  More than K of them: the exact list is a sorted top K of more than K
  // candidates whichever way the candidates near the threshold fall, and those rank below all of these -- the threshold band is then left alone
  {
    const float sure_lo = thr + eps;
    int mine = 0;
    for (long i = tid; i < n; i += EO_THREADS) mine += __uint_as_float((unsigned)(c[i] >> 32)) > sure_lo ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
    if ((tid & 63) == 0 && mine) atomicAdd(&s_sure, mine);
  }
  __syncthreads();
  const bool band_on = s_sure <= K;
  // the K-th largest score: MSB-first radix select on the score bits (scores are probabilities: the bit patterns order like the values)
  float lo = -1.f;      // prefix = candidates with s_w >= lo; fewer than K candidates: all of them
  if (n >= K) {
    unsigned prefix = 0, mask = 0;
    int need = K;
    for (int pass = 3; pass >= 0; --pass) {
      const int shift = pass * 8;
      for (int i = tid; i < 256; i += EO_THREADS) hist[i] = 0;
      __syncthreads();
      for (long i = tid; i < n; i += EO_THREADS) {
        const unsigned sb = (unsigned)(c[i] >> 32);
        if ((sb & mask) == prefix) atomicAdd(&hist[(sb >> shift) & 0xFF], 1);
      }
      __syncthreads();
      if (tid < 64) {
        // the largest digit d whose suffix count S(d) = sum_{x >= d} hist[x] reaches `need`: lane l owns digits 4l .. 4l+3 (the scan of select_b_kernel)
        const int h0 = hist[4 * tid], h1 = hist[4 * tid + 1], h2 = hist[4 * tid + 2], h3 = hist[4 * tid + 3];
        int above = h0 + h1 + h2 + h3;
        int incl = above;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_down(incl, o, 64); if (tid + o < 64) incl += t; }
        above = incl - above;
        const int S3 = above + h3, S2 = S3 + h2, S1 = S2 + h1, S0 = S1 + h0;
        int best = -1;
        if (S3 >= need) best = 4 * tid + 3; else if (S2 >= need) best = 4 * tid + 2; else if (S1 >= need) best = 4 * tid + 1; else if (S0 >= need) best = 4 * tid;
        int gb = best;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) gb = max(gb, __shfl_xor(gb, o, 64));
        const int d = gb < 0 ? 0 : gb;
        if (4 * tid <= d && d < 4 * tid + 4) {
          const int k = d - 4 * tid;
          const int Sd = k == 3 ? S3 : k == 2 ? S2 : k == 1 ? S1 : S0;
          const int hd = k == 3 ? h3 : k == 2 ? h2 : k == 1 ? h1 : h0;
          s_digit = d;
          s_need = need - (Sd - hd);
        }
      }
      __syncthreads();
      prefix |= ((unsigned)s_digit) << shift;
      mask |= 0xFFu << shift;
      need = s_need;
      __syncthreads();
    }
    lo = __uint_as_float(prefix) - 2.f * eps;
  }
  // the part of the list that matters: the prefix and the threshold band
  for (int i = tid; i < EO_MAXSORT; i += EO_THREADS) keys[i] = 0;
  __syncthreads();
  for (long i = tid; i < n; i += EO_THREADS) {
    const unsigned long long k = c[i];
    const float sc = __uint_as_float((unsigned)(k >> 32));
    if (sc >= lo || (band_on && fabsf(sc - thr) <= eps)) {
      const int slot = atomicAdd(&s_cnt, 1);
      if (slot < EO_MAXSORT) keys[slot] = k;
    }
  }
  __syncthreads();
  const int m = s_cnt;
  int ncells = 0;
  if (m > EO_MAXSORT) {
    for (long i = tid; i < n; i += EO_THREADS) {
      const unsigned long long k = c[i];
      const float sc = __uint_as_float((unsigned)(k >> 32));
      if (sc >= lo || (band_on && fabsf(sc - thr) <= eps)) {
        const unsigned idx = 0xFFFFFFFFu - (unsigned)(k & 0xFFFFFFFFull);
        const int cell = (int)((idx / (unsigned)W) >> 3) * Wc + (int)((idx % (unsigned)W) >> 3);
        if (cell < ncell) cmap[cell] = 0;
      }
    }
    __threadfence();
    __syncthreads();
    for (int c0 = 0; c0 < ncell; c0 += EO_THREADS) {
      const int cell = c0 + tid;
      const bool on = cell < ncell && eo_ld(cmap + cell) == 0;
      int tot;
      const int r = ncells + eo_block_rank(on, s_wcnt, &tot);
      if (cell < ncell) cmap[cell] = (on && r < slots) ? r : EO_NONE;
      if (on && r < slots) clist[r] = cell;
      ncells += tot;
    }
    if (tid == 0) { cell_count[img] = ncells; if (m > 0) atomicAdd(stats, (unsigned long long)m); }
    return;
  }
  // bitonic sort, descending (score desc, raster asc on ties; zeros sink to the end): only the stages the occupied power of two needs
  // (the sort of select_b_kernel, with its unpadded strides: 8-byte keys at power-of-two distances conflict in LDS.  Typically a few hundred keys sit in the
  // 1024-key minimum; the whole kernel takes 64 us for a 64-image call, 3 % of the option's GPU time -- profiles/exact_order_rocprofv3_kernel_stats.csv)
  int sn = 1024;
  while (sn < m) sn <<= 1;
  for (int k2 = 2; k2 <= sn; k2 <<= 1)
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < sn; i += EO_THREADS) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const unsigned long long x = keys[i], y = keys[ixj];
          const bool desc = ((i & k2) == 0);
          if (desc ? (x < y) : (x > y)) { keys[i] = y; keys[ixj] = x; }
        }
      }
      __syncthreads();
    }
  // rule 3; a marked candidate claims its cell with its list position (the smallest position wins)
  const float two_eps = 2.f * eps;
  int mine = 0;
  for (int t = tid; t < m; t += EO_THREADS) {
    const unsigned long long k = keys[t];
    const float sc = __uint_as_float((unsigned)(k >> 32));
    bool mark = band_on && fabsf(sc - thr) <= eps;
    if (!mark && sc >= lo) {
      if (t > 0) mark = __uint_as_float((unsigned)(keys[t - 1] >> 32)) - sc <= two_eps;
      if (!mark && t + 1 < m) { const float nx = __uint_as_float((unsigned)(keys[t + 1] >> 32)); mark = nx >= lo && sc - nx <= two_eps; }
    }
    if (mark) {
      const unsigned idx = 0xFFFFFFFFu - (unsigned)(k & 0xFFFFFFFFull);
      const int cell = (int)((idx / (unsigned)W) >> 3) * Wc + (int)((idx % (unsigned)W) >> 3);
      if (cell < ncell) { atomicMin(&cmap[cell], t); ++mine; }
    }
  }
  if (mine) atomicAdd(&s_marked, mine);
  __threadfence();
  __syncthreads();
  // the cells in the order of their first marked candidate: ordered compaction of the owners.  A cell's entry turns from the owner's position t into its
  // rank r <= t (or EO_NONE) while later candidates of the same cell (positions > t) still compare against it: neither value equals their position
  for (int t0 = 0; t0 < m; t0 += EO_THREADS) {
    const int t = t0 + tid;
    int cell = -1;
    if (t < m) {
      const unsigned long long k = keys[t];
      const unsigned idx = 0xFFFFFFFFu - (unsigned)(k & 0xFFFFFFFFull);
      cell = (int)((idx / (unsigned)W) >> 3) * Wc + (int)((idx % (unsigned)W) >> 3);
      if (cell >= ncell) cell = -1;
    }
    const bool owner = cell >= 0 && eo_ld(cmap + cell) == t;
    int tot;
    const int r = ncells + eo_block_rank(owner, s_wcnt, &tot);
    if (owner) { cmap[cell] = r < slots ? r : EO_NONE; if (r < slots) clist[r] = cell; }
    ncells += tot;
  }
  if (tid == 0) { cell_count[img] = ncells; if (s_marked > 0) atomicAdd(stats, (unsigned long long)s_marked); }
}

// One workgroup per crop slot: the slot's (image, cell) from the prefix over the images' cell counts, then the 88x88 u8 crop.  A slot nobody got keeps
// whatever it held (its scores are never read).  Workgroup 0 also books the call: stats[1] += cells re-evaluated, [2] += cells dropped, [3] += 1.
__global__ __launch_bounds__(256) void exact_order_gather_kernel(const uint8_t* __restrict__ gray, int stride, long image_stride, int n_img, int W, int H, int Wc,
                                                                const int* __restrict__ cell_list, const int* __restrict__ cell_count, int slots,
                                                                uint8_t* __restrict__ crops, unsigned long long* __restrict__ stats) {
  __shared__ int s_img, s_cell;
  const int slot = blockIdx.x;
  if (threadIdx.x == 0) {
    int base = 0, img = -1, cell = -1;
    long total = 0;
    for (int j = 0; j < n_img; ++j) {
      const int cnt = cell_count[j];
      const int g = min(cnt, slots);
      if (img < 0 && slot < base + g && slot >= base) { img = j; cell = cell_list[(size_t)j * slots + (slot - base)]; }
      base += g;
      total += cnt;
    }
    s_img = img; s_cell = cell;
    if (slot == 0) {
      const long granted = total < slots ? total : slots;
      if (granted > 0) atomicAdd(stats + 1, (unsigned long long)granted);
      if (total > granted) atomicAdd(stats + 2, (unsigned long long)(total - granted));
      atomicAdd(stats + 3, 1ull);
    }
  }
  __syncthreads();
  const int img = s_img, cell = s_cell;
  if (img < 0 || cell < 0) return;
  const int x0 = eo_origin(cell % Wc, W), y0 = eo_origin(cell / Wc, H);
  const uint8_t* src = gray + (size_t)img * image_stride + (size_t)y0 * stride + x0;
  uint8_t* dst = crops + (size_t)slot * EO_CROP * EO_CROP;
  for (int i = threadIdx.x; i < EO_CROP * EO_CROP; i += 256) {
    const int y = i / EO_CROP, x = i - y * EO_CROP;
    dst[i] = src[(size_t)y * stride + x];
  }
}

// One workgroup per image: every candidate of a re-evaluated cell takes the cell's direct score from the crop's score map; candidates whose final score is
// not > thr leave the list.  The compaction is in place and keeps the list order (a chunk is read completely before it is written, at or below where it was read).
__global__ __launch_bounds__(EO_THREADS) void exact_order_patch_kernel(unsigned long long* __restrict__ cand, int* __restrict__ cand_count, long cand_cap, int W, int H,
                                                                      int Wc, int ncell, float thr, const int* __restrict__ cell_map,
                                                                      const int* __restrict__ cell_count, int slots, const float* __restrict__ crop_scores) {
  __shared__ int s_base;
  __shared__ int s_wcnt[EO_THREADS / 64];
  const int img = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) s_base = eo_slot_base(cell_count, img, slots);
  __syncthreads();
  const int room = slots - s_base;      // ranks below this one got a slot
  const int base = s_base;
  unsigned long long* c = cand + (size_t)img * cand_cap;
  const int* cmap = cell_map + (size_t)img * ncell;
  long n = cand_count[img];
  if (n > cand_cap) n = cand_cap;
  int out = 0;
  for (long i0 = 0; i0 < n; i0 += EO_THREADS) {
    const long i = i0 + tid;
    unsigned long long k = 0;
    bool keep = false;
    if (i < n) {
      k = c[i];
      const unsigned idx = 0xFFFFFFFFu - (unsigned)(k & 0xFFFFFFFFull);
      const int y = (int)(idx / (unsigned)W), x = (int)(idx % (unsigned)W);
      const int cell = (y >> 3) * Wc + (x >> 3);
      float sc = __uint_as_float((unsigned)(k >> 32));
      if (cell < ncell) {
        const int r = cmap[cell];
        if (r >= 0 && r < room) {
          const int x0 = eo_origin(x >> 3, W), y0 = eo_origin(y >> 3, H);
          sc = crop_scores[(size_t)(base + r) * EO_CROP * EO_CROP + (size_t)(y - y0) * EO_CROP + (x - x0)];
          k = ((unsigned long long)__float_as_uint(sc) << 32) | (k & 0xFFFFFFFFull);
        }
      }
      keep = sc > thr;
    }
    int tot;
    const int r = out + eo_block_rank(keep, s_wcnt, &tot);      // its barriers separate the chunk's reads from its writes
    if (keep) c[r] = k;
    out += tot;
  }
  if (tid == 0) cand_count[img] = out;
}

hipError_t launch_exact_order_mark(const unsigned long long* cand, const int* cand_count, long cand_cap, int n_img, int W, int H, int K, float thr, float eps,
                                   int slots, int* cell_map, int* cell_list, int* cell_count, unsigned long long* stats, hipStream_t s) {
  const int Wc = W / 8, ncell = (H / 8) * Wc;
  const size_t lds = sizeof(unsigned long long) * EO_MAXSORT;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(exact_order_mark_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(exact_order_mark_kernel, dim3(n_img), dim3(EO_THREADS), lds, s, cand, cand_count, cand_cap, W, Wc, ncell, K, thr, eps, slots, cell_map,
                     cell_list, cell_count, stats);
  return hipGetLastError();
}

hipError_t launch_exact_order_gather(const uint8_t* gray, int stride, long image_stride, int n_img, int W, int H, const int* cell_list, const int* cell_count,
                                     int slots, uint8_t* crops, unsigned long long* stats, hipStream_t s) {
  if (W < EO_CROP || H < EO_CROP || ((W | H) & 7)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(exact_order_gather_kernel, dim3(slots), dim3(256), 0, s, gray, stride, image_stride, n_img, W, H, W / 8, cell_list, cell_count, slots, crops,
                     stats);
  return hipGetLastError();
}

hipError_t launch_exact_order_patch(unsigned long long* cand, int* cand_count, long cand_cap, int n_img, int W, int H, float thr, const int* cell_map,
                                    const int* cell_count, int slots, const float* crop_scores, hipStream_t s) {
  if (W < EO_CROP || H < EO_CROP || ((W | H) & 7)) return hipErrorInvalidValue;
  const int Wc = W / 8, ncell = (H / 8) * Wc;
  hipLaunchKernelGGL(exact_order_patch_kernel, dim3(n_img), dim3(EO_THREADS), 0, s, cand, cand_count, cand_cap, W, H, Wc, ncell, thr, cell_map, cell_count, slots,
                     crop_scores);
  return hipGetLastError();
}

}  // namespace d2fe
