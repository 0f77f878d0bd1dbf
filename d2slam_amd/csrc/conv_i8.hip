// conv_i8.hip -- D2FE_PREC_I8 (contract in include/d2fe.h): the SuperPoint conv stack with int8 operands on v_mfma_i32_32x32x32_i8, int32 accumulation.
//
// The tilings, the B-fragment groups and the epilogue addressing are those of conv_f16x2_kernel<..., SPLIT = false> (conv_f16.hip).  What differs:
//  * staging quantises: q = (int8) rintf(clamp(x * r, -127, 127)) with the layer's r = fl32(127 / T) (ConvArgs::qr), 16 channels per thread and one
//    ds_write_b128; a pixel takes CIN + 16 bytes, an odd count of 16-byte slots (5, 9, 17), so the 16-lane groups of the ds_read_b128 A fragments hit
//    distinct slots.  The fused conv1a prologue is the fp32 chain of every mode, quantised with conv1b's r on its way into LDS.
//  * one MFMA covers K = 32: lane half h holds channels 16 h .. 16 h + 15 of the k-step in BOTH operands (the A fragment is 16 consecutive bytes of the patch
//    pixel, the B fragment is packed by pack_weights_i8 from the same rule).  The int32 sum is exact, so its order is free.
//  * the epilogue is y = fl32(fl32((float)acc * d_c) + bias_c), two roundings (__fmul_rn / __fadd_rn: no contraction), d_c = s_x * s_w[c] from ConvArgs::dscale.
// The pool is only compiled with ReLU (the network has no other pooled layer): max and ReLU commute, so "ReLU, then pool" of the contract is what it computes.
#include "conv_common.h"

#include <cmath>
#include <vector>

namespace d2fe {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ int quant_i8(float x, float r) {
  return (int)rintf(fminf(fmaxf(__fmul_rn(x, r), -127.f), 127.f));
}
__device__ __forceinline__ int quant_pack4(float x0, float x1, float x2, float x3, float r) {
  const unsigned q0 = (unsigned)quant_i8(x0, r) & 0xffu, q1 = (unsigned)quant_i8(x1, r) & 0xffu, q2 = (unsigned)quant_i8(x2, r) & 0xffu, q3 = (unsigned)quant_i8(x3, r) & 0xffu;
  return (int)(q0 | (q1 << 8) | (q2 << 16) | (q3 << 24));
}

template <int CIN, int KS, int TH, int TW, int WM, int WN, int MT, int NT, bool POOL, bool RELU, bool FUSE1A = false>
__global__ __launch_bounds__(WM * WN * 64) void conv_i8_kernel(ConvArgs a) {
  constexpr int P = KS / 2;
  constexpr int PH = TH + KS - 1, PW = TW + KS - 1;
  constexpr int CPB = CIN + 16;  // bytes per pixel
  constexpr int NPIX = PH * PW;
  constexpr int NTHREADS = WM * WN * 64;
  constexpr int TAPS = KS * KS;
  constexpr int KST = CIN / 32;
  static_assert(TH * TW == WM * MT * 32, "tile / wave mismatch");
  extern __shared__ __attribute__((aligned(16))) signed char lds8[];

  const int tiles_x = (a.W + TW - 1) / TW;
  const int tx0 = (blockIdx.x % tiles_x) * TW;
  const int ty0 = (blockIdx.x / tiles_x) * TH;
  const int img = blockIdx.z;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const float qr = a.qr;

  // ---- stage + quantise the input patch ------------------------------------------------------------------
  if constexpr (FUSE1A) {
    // conv1a as in conv_f16x2_kernel: five v_mfma_f32_32x32x2_f32 with the weights as the A operand, the fmaf chain of conv1a_octet bit for bit; a lane
    // (= patch pixel) ends up with 4 x 4 consecutive channels, quantised with conv1b's r and stored as 4-byte runs
    static_assert(CIN == 64 && KS == 3 && NTHREADS == 256, "fused prologue is conv1a -> conv1b, four waves");
    constexpr int FR = PH + 2, FC = PW + 2, NMT = (NPIX + 31) / 32;
    unsigned char* u8p = reinterpret_cast<unsigned char*>(lds8 + NPIX * CPB);
    const uint8_t* ip = a.img + (size_t)img * a.img_istride;
    for (int i = tid; i < FR * FC; i += NTHREADS) {
      const int r = i / FC, c = i - r * FC;
      const int gy = ty0 - P - 1 + r, gx = tx0 - P - 1 + c;
      u8p[i] = (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) ? ip[(size_t)gy * a.img_stride + gx] : (unsigned char)0;
    }
    const int hh = lane >> 5, nt = wave & 1;
    float c1a[5];
    int koff[5];
#pragma unroll
    for (int st = 0; st < 5; ++st) {
      const int k = 2 * st + hh;
      c1a[st] = k == 0 ? a.b1a[nt * 32 + (lane & 31)] : a.w1a[(k - 1) * 64 + nt * 32 + (lane & 31)];
      koff[st] = k == 0 ? 0 : ((k - 1) / 3) * FC + (k - 1) % 3;
    }
    const float scale = (float)(1.0 / 255.0);
    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    __syncthreads();
    for (int u = wave; u < 2 * NMT; u += 4) {             // u & 1 == wave & 1: a wave only ever needs one half of the weights
      const int pidx = (u >> 1) * 32 + (lane & 31);
      const int py = pidx / PW, px = pidx - py * PW;
      const int gy = ty0 + py - P, gx = tx0 + px - P;
      const bool inpatch = pidx < NPIX;
      const bool pvalid = inpatch && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
      const int tb = inpatch ? py * FC + px : 0;
      float tap[5];
#pragma unroll
      for (int st = 0; st < 5; ++st) {
        float v = (float)u8p[tb + koff[st]] * scale;
        if (st == 0) v = hh ? v : 1.0f;
        tap[st] = pvalid ? v : 0.f;
      }
      f32x16 d = __builtin_amdgcn_mfma_f32_32x32x2f32(c1a[0], tap[0], zero, 0, 0, 0);
#pragma unroll
      for (int st = 1; st < 5; ++st) d = __builtin_amdgcn_mfma_f32_32x32x2f32(c1a[st], tap[st], d, 0, 0, 0);
      if (inpatch) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {                       // rows (channels) 8 q + 4 hh + (0..3) of half nt
          float o[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = d[4 * q + e] > 0.f ? d[4 * q + e] : 0.f;
          *reinterpret_cast<int*>(lds8 + pidx * CPB + nt * 32 + 8 * q + 4 * hh) = quant_pack4(o[0], o[1], o[2], o[3], qr);
        }
      }
    }
  } else {
    const float* in = a.in + (size_t)img * a.in_img_stride + a.in_coff;
    constexpr int C16 = CIN / 16;
    constexpr int TOTAL = NPIX * C16;
    constexpr int ITERS = (TOTAL + NTHREADS - 1) / NTHREADS;
    constexpr int UNR = 2;
    for (int it0 = 0; it0 < ITERS; it0 += UNR) {
      f32x4 v[UNR][4];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const int idx = (it0 + u) * NTHREADS + tid;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[u][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (it0 + u < ITERS && idx < TOTAL) {
          const int pix = idx / C16, c16 = idx % C16;
          const int gy = ty0 + pix / PW - P, gx = tx0 + pix % PW - P;
          if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W && !D2FE_ABL(a, 1)) {
            const float* src = in + ((size_t)gy * a.W + gx) * a.in_cstride + c16 * 16;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[u][j] = *reinterpret_cast<const f32x4*>(src + 4 * j);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const int idx = (it0 + u) * NTHREADS + tid;
        if (it0 + u < ITERS && idx < TOTAL) {
          const int pix = idx / C16, c16 = idx % C16;
          i32x4 q;
#pragma unroll
          for (int j = 0; j < 4; ++j) q[j] = quant_pack4(v[u][j][0], v[u][j][1], v[u][j][2], v[u][j][3], qr);
          *reinterpret_cast<i32x4*>(lds8 + pix * CPB + c16 * 16) = q;
        }
      }
    }
  }
  __syncthreads();

  const int ntile0 = blockIdx.y * (WN * NT) + wn * NT;
  i32x16 acc[MT][NT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][n][r] = 0;

  int aoff[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    int py, px;
    mtile_pixel<TW>(wm * MT + m, lane & 31, py, px);
    aoff[m] = (py * PW + px) * CPB + 16 * (lane >> 5);
  }

  // packed weights: [ntile][tap][kstep][lane] 16 x int8;  element e = q_w[co = ntile*32 + (lane&31)][ci = kstep*32 + 16*(lane>>5) + e][tap]
  const i32x4* wp = reinterpret_cast<const i32x4*>(a.wpack);
  const i32x4* wbase[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) wbase[n] = wp + (size_t)(ntile0 + n) * TAPS * KST * 64 + lane;

  // B fragments double-buffered in registers in groups of G k-steps, as in conv_f16x2_kernel
  constexpr int G = KST < 4 ? KST : 4;   // k-steps (of 32 channels) per group; divides KST
  constexpr int GPT = KST / G;
  constexpr int NG = TAPS * GPT;
  static_assert(KST % G == 0, "group size must divide the steps per tap");
  i32x4 bq[2][G][NT];
  auto load_grp = [&](int buf, int grp) {
    if (D2FE_ABL(a, 2)) grp = 0;
#pragma unroll
    for (int j = 0; j < G; ++j)
#pragma unroll
      for (int n = 0; n < NT; ++n) bq[buf][j][n] = wbase[n][(size_t)(grp * G + j) * 64];
  };
  auto compute_grp = [&](int buf, int grp) {
    const int tap = grp / GPT, ks0 = (grp % GPT) * G;
    const int tap_off = ((tap / KS) * PW + (tap % KS)) * CPB + ks0 * 32;
#pragma unroll
    for (int j = 0; j < G; ++j) {
      i32x4 av[MT];
#pragma unroll
      for (int m = 0; m < MT; ++m) av[m] = *reinterpret_cast<const i32x4*>(lds8 + aoff[m] + tap_off + j * 32);
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[m][n] = __builtin_amdgcn_mfma_i32_32x32x32_i8(av[m], bq[buf][j][n], acc[m][n], 0, 0, 0);
    }
  };
  load_grp(0, 0);
#pragma unroll 1
  for (int g = 0; g + 1 < NG; g += 2) {
    load_grp(1, g + 1);
    __builtin_amdgcn_sched_barrier(0);
    compute_grp(0, g);
    load_grp(0, g + 2 < NG ? g + 2 : NG - 1);
    __builtin_amdgcn_sched_barrier(0);
    compute_grp(1, g + 1);
  }
  if constexpr (NG & 1) compute_grp(0, NG - 1);

  // (float)acc (round to nearest even), * d_c, + bias: two roundings
  f32x16 y[MT][NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const float dc = a.dscale[(ntile0 + n) * 32 + (lane & 31)];
    const float b = a.bias[(ntile0 + n) * 32 + (lane & 31)];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) y[m][n][r] = __fadd_rn(__fmul_rn((float)acc[m][n][r], dc), b);
  }
  conv_epilogue<TW, MT, NT, POOL, RELU>(a, y, 1.0f, img, ty0, tx0, wm, ntile0, lane);
}

template <int CIN, int KS, int TH, int TW, int WM, int WN, int MT, int NT>
static hipError_t launch_i8(bool pool, bool relu, int cout_pad, const ConvArgs& a, hipStream_t s) {
  constexpr int BN = WN * NT * 32;
  constexpr size_t lds = (size_t)(TH + KS - 1) * (TW + KS - 1) * (CIN + 16);
  const int tiles_x = (a.W + TW - 1) / TW, tiles_y = (a.H + TH - 1) / TH;
  dim3 grid(tiles_x * tiles_y, cout_pad / BN, a.n_img), block(WM * WN * 64);
  if (cout_pad % BN || !a.dscale) return hipErrorInvalidValue;
#define D2FE_LAUNCH(PL, RL)                                                                          \
  do {                                                                                               \
    auto k = conv_i8_kernel<CIN, KS, TH, TW, WM, WN, MT, NT, PL, RL, false>;                         \
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k),                             \
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);        \
    if (e != hipSuccess) return e;                                                                   \
    hipLaunchKernelGGL(k, grid, block, lds, s, a);                                                   \
  } while (0)
  if constexpr (MT == 2 && TW == 32) {
    if (pool) { if (!relu) return hipErrorInvalidValue; D2FE_LAUNCH(true, true); return hipGetLastError(); }
  } else {
    if (pool) return hipErrorInvalidValue;
  }
  if (relu) D2FE_LAUNCH(false, true); else D2FE_LAUNCH(false, false);
#undef D2FE_LAUNCH
  return hipGetLastError();
}

static hipError_t launch_i8_fused1b(int cout_pad, const ConvArgs& a, hipStream_t s) {
  constexpr int TH = 4, TW = 32;
  constexpr size_t lds = (size_t)(TH + 2) * (TW + 2) * 80 + (TH + 4) * (TW + 4);      // the int8 patch + the frame bytes
  if (cout_pad != 64 || !a.img || !a.w1a || !a.b1a || !a.dscale) return hipErrorInvalidValue;
  auto k = conv_i8_kernel<64, 3, TH, TW, 2, 2, 2, 1, true, true, true>;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  dim3 grid(((a.W + TW - 1) / TW) * ((a.H + TH - 1) / TH), 1, a.n_img), block(256);
  hipLaunchKernelGGL(k, grid, block, lds, s, a);
  return hipGetLastError();
}

hipError_t launch_conv_i8(ConvShape shape, int conv64_tile, bool pool, bool relu, int cout_pad, const ConvArgs& a, hipStream_t s) {
  switch (shape) {
    case CONV1B_FUSED:       return launch_i8_fused1b(cout_pad, a, s);
    case CONV_64_T8x32:
      if (conv64_tile == 1) return launch_i8<64, 3, 4, 32, 2, 2, 2, 1>(pool, relu, cout_pad, a, s);
      return launch_i8<64, 3, 8, 32, 4, 1, 2, 2>(pool, relu, cout_pad, a, s);
    case CONV_128_T4x32:     return launch_i8<128, 3, 4, 32, 2, 2, 2, 2>(pool, relu, cout_pad, a, s);
    case CONV_128_T4x16:     return launch_i8<128, 3, 4, 16, 1, 4, 2, 1>(pool, relu, cout_pad, a, s);
    case CONV_256_1x1_T4x16: return launch_i8<256, 1, 4, 16, 1, 4, 2, 1>(pool, relu, cout_pad, a, s);
  }
  return hipErrorInvalidValue;
}

// host-side packing: q_w = clamp(rint(w * 127 / amax_c), -127, 127) per output channel in double, round half to even (the default rounding mode of
// nearbyint), in fragment order [ntile][tap][kstep][lane][16]; s_w[c] = fl32(amax_c / 127), 1 for an all-zero or a padding channel
size_t packed_weight_bytes_i8(int cout_pad, int cin, int ks) { return (size_t)cout_pad * cin * ks * ks; }

void pack_weights_i8(const float* w, int cout, int cin, int ks, int cout_pad, int8_t* dst, float* s_w) {
  const int taps = ks * ks, kst = cin / 32;
  const size_t per = (size_t)cin * taps;
  std::vector<float> amax(cout_pad, 0.f);
  for (int co = 0; co < cout; ++co)
    for (size_t i = 0; i < per; ++i) { const float v = fabsf(w[co * per + i]); if (v > amax[co]) amax[co] = v; }
  for (int co = 0; co < cout_pad; ++co) s_w[co] = amax[co] > 0.f ? amax[co] / 127.0f : 1.0f;
  for (int nt = 0; nt < cout_pad / 32; ++nt)
    for (int tap = 0; tap < taps; ++tap)
      for (int k = 0; k < kst; ++k)
        for (int lane = 0; lane < 64; ++lane)
          for (int e = 0; e < 16; ++e) {
            const int co = nt * 32 + (lane & 31);
            const int ci = k * 32 + 16 * (lane >> 5) + e;
            double q = 0.0;
            if (co < cout && amax[co] > 0.f) {
              q = nearbyint((double)w[((size_t)co * cin + ci) * taps + tap] * 127.0 / (double)amax[co]);
              q = q < -127.0 ? -127.0 : (q > 127.0 ? 127.0 : q);
            }
            dst[((((size_t)nt * taps + tap) * kst + k) * 64 + lane) * 16 + e] = (int8_t)q;
          }
}

}  // namespace d2fe
