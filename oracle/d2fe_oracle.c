/*
 * d2fe_oracle.c -- CPU restatement ("oracle") of the D2SLAM d2frontend feature hot path.
 *
 * THIS IS TEST INFRASTRUCTURE, NOT PRODUCT CODE.  Only tests/, __graft_entry__.smoke() and
 * bench.py's cpu_baseline leg may load it.  The shipped path (the HIP sources in d2slam_amd/csrc behind
 * include/d2fe.h) never calls into this file and has no CPU fallback.
 *
 * PARITY STATUS: pinned in part, to the reference's OWN code in two ways.
 *  (1) oracle/_ref/libspref.so (oracle/build_ref.py): the reference's own C++ line ranges -- SuperPoint::infer / processOutput and
 *      everything they call (superpoint_tensorrt.cpp:161-183,200-350), getKeyPoints / NMS2 (superpoint_common.cpp:8-40,101-178),
 *      matchKNN (feature_matcher.cpp), getFeatureHalfImg and the quadcam neighbour branch of matchLocalFeatures
 *      (d2featuretracker.cpp:1051-1075,1146-1181) -- compiled from /root/reference against stand-in Eigen/OpenCV headers
 *      (oracle/ref_shim/).  tests/test_ref_pin.py holds orc_select_b, orc_sample_b, orc_nms2_a, orc_match_knn, orc_half_img and the
 *      neighbour chain to it, bit for bit, at the BASELINE geometries.  Third-party arithmetic under that code stays a restatement
 *      (cv::BFMatcher's normL2Sqr_ order and K-best insertion, Eigen's norm() order, libstdc++'s order among equal scores).
 *  (2) The network and the variant-A sampling are also defined in PYTHON in the reference (d2frontend/superpoint.ipynb, modules
 *      SuperPointNetHalf / SuperPointNet): tests/golden/make_golden_ref.py and make_golden_headline.py execute those modules verbatim
 *      and commit their outputs (incl. 640x480 / 800x400 / 512x512), and tests/test_reference_golden.py holds orc_prep_u8 ..
 *      orc_softmax_semi (3x3 layers through orc_conv as well as orc_conv3x3_wino), orc_l2norm_rows and orc_sample_a to them (and
 *      orc_sample_a's PCA convention to sklearn, the tool behind the CSVs).
 * Still **parity unpinned** (restatements of third-party code that is not in the reference tree, cross-checked against independent
 * implementations only): cv::BFMatcher(NORM_L2, true).match (A11), NetVLAD (graph not in the tree), undistort (cv::remap), the int8
 * codec's consumers, the database, and everything in d2fe_oracle_lk.c (OpenCV-CUDA).
 *
 * Numerical definition.  Where the reference leaves floating-point evaluation order to a
 * third-party engine (TensorRT conv kernels, OpenCV SIMD reductions, Eigen reductions) the
 * oracle fixes one order and says so:
 *   - convolutions: one k-ordered fp32 fmaf chain per output, k = (ky, kx, ci) ascending,
 *     accumulator initialised with the bias.  (This is also bit-for-bit what gfx950's
 *     v_mfma_f32_32x32x2_f32 computes, so the HIP "exact" mode can be compared bitwise.)
 *   - softmax: max, then e = exp(x - max) with the fma-only expf below, sequential sum over
 *     c = 0..64, IEEE division.
 *   - unstable std::sort calls in the reference get the deterministic tie-break
 *     "equal score -> lower raster index first" (marked there).
 *
 * Layouts: activations are NHWC fp32; weights are passed in PyTorch layout
 * [cout][cin][kh][kw] (the layout of the SuperPointNet state_dict in
 * d2frontend/superpoint.ipynb cell 1, /root/reference) and re-ordered internally.
 *
 * Build: see oracle/Makefile  (gcc -O2 -mavx2 -mfma -ffp-contract=off -fopenmp).
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define ORC_API __attribute__((visibility("default")))

/* ------------------------------------------------------------------------------------------
 * A1  image prep.  Reference: SuperPoint::processInput, d2frontend/src/CNN/superpoint_tensorrt.cpp:185-198
 *     image.convertTo(mono, CV_32FC1, 1.0/255.0)  -> OpenCV cvt for 8U->32F evaluates
 *     (float)src * (float)alpha in single precision.
 * ---------------------------------------------------------------------------------------- */
ORC_API void orc_prep_u8(const uint8_t* img, int h, int w, int stride, float* out) {
  const float a = (float)(1.0 / 255.0);
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) out[(size_t)y * w + x] = (float)img[(size_t)y * stride + x] * a;
}

/* ------------------------------------------------------------------------------------------
 * A2  SuperPoint network.  Reference: d2frontend/superpoint.ipynb:300-374 (class SuperPointNetHalf)
 * ---------------------------------------------------------------------------------------- */

/* KxK conv (K = 1 or 3), stride 1, zero pad K/2, NHWC in/out, optional ReLU.
 * wgt: [cout][cin][K][K] (PyTorch).  One fmaf chain per output in (ky,kx,ci) order, acc0 = bias.
 * Out-of-image taps are skipped (== fmaf(0, w, acc) up to the sign of zero). */
ORC_API void orc_conv(const float* in, int h, int w, int cin, const float* wgt, const float* bias,
                      int cout, int ksize, int relu, float* out) {
  const int K = ksize, P = K / 2;
  /* re-order weights to [ky][kx][ci][co] so the co loop vectorises */
  float* wt = (float*)malloc(sizeof(float) * (size_t)K * K * cin * cout);
  for (int co = 0; co < cout; ++co)
    for (int ci = 0; ci < cin; ++ci)
      for (int ky = 0; ky < K; ++ky)
        for (int kx = 0; kx < K; ++kx)
          wt[(((size_t)ky * K + kx) * cin + ci) * cout + co] =
              wgt[(((size_t)co * cin + ci) * K + ky) * K + kx];
#pragma omp parallel for schedule(static)
  for (int y = 0; y < h; ++y) {
    float* acc = (float*)malloc(sizeof(float) * cout);
    for (int x = 0; x < w; ++x) {
      for (int co = 0; co < cout; ++co) acc[co] = bias[co];
      for (int ky = 0; ky < K; ++ky) {
        const int yy = y + ky - P;
        if (yy < 0 || yy >= h) continue;
        for (int kx = 0; kx < K; ++kx) {
          const int xx = x + kx - P;
          if (xx < 0 || xx >= w) continue;
          const float* ip = in + ((size_t)yy * w + xx) * cin;
          const float* wp = wt + ((size_t)ky * K + kx) * cin * cout;
          for (int ci = 0; ci < cin; ++ci) {
            const float a = ip[ci];
            const float* wr = wp + (size_t)ci * cout;
            for (int co = 0; co < cout; ++co) acc[co] = fmaf(a, wr[co], acc[co]);
          }
        }
      }
      float* op = out + ((size_t)y * w + x) * cout;
      if (relu)
        for (int co = 0; co < cout; ++co) op[co] = acc[co] > 0.f ? acc[co] : 0.f;
      else
        for (int co = 0; co < cout; ++co) op[co] = acc[co];
    }
    free(acc);
  }
  free(wt);
}

/* 3x3 / stride 1 / pad 1 convolution evaluated as Winograd F(2x2,3x3) in fp32 -- the restatement of the HIP library's
 * precision mode 2 (d2slam_amd/csrc/conv_wino.hip).  The reference leaves the algorithm and the accumulation order of its
 * convolutions to TensorRT (superpoint_tensorrt.cpp:150), which itself selects Winograd kernels for such layers; this
 * function fixes ONE order so that the GPU result can be compared bit for bit, and tests/ hold it to orc_conv (the direct
 * chain) within a few 1e-6 relative:
 *   U[xi=(i,j)][ci][co] = (float) sum_{a,b ascending} G[i][a] G[j][b] g[co][ci][a][b]   (double)
 *   V = B^T d B per 4x4 input window d (zero outside the image): down the columns first
 *       t0 = d0 - d2, t1 = d1 + d2, t2 = d2 - d1, t3 = d1 - d3, then the same along each row
 *   M[xi][co] = fmaf chain from +0 over ci in the order 0,4,1,5,2,6,3,7 of each block of 8
 *   A^T M A: s_i0 = (m_i0 + m_i1) + m_i2, s_i1 = (m_i1 - m_i2) - m_i3; y_0b = (s_0b + s_1b) + s_2b, y_1b = (s_1b - s_2b) - s_3b
 *   out = y + bias, optional ReLU.            cin must be a multiple of 8. */
ORC_API void orc_conv3x3_wino(const float* in, int h, int w, int cin, const float* wgt, const float* bias, int cout, int relu,
                              float* out) {
  static const double G[4][3] = {{1.0, 0.0, 0.0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0.0, 0.0, 1.0}};
  float* U = (float*)malloc(sizeof(float) * 16 * (size_t)cin * cout);   /* [xi][ci][co] */
  for (int xi = 0; xi < 16; ++xi)
    for (int ci = 0; ci < cin; ++ci)
      for (int co = 0; co < cout; ++co) {
        const float* g = wgt + ((size_t)co * cin + ci) * 9;
        double s = 0.0;
        for (int a = 0; a < 3; ++a)
          for (int b = 0; b < 3; ++b) s += G[xi >> 2][a] * G[xi & 3][b] * (double)g[a * 3 + b];
        U[((size_t)xi * cin + ci) * cout + co] = (float)s;
      }
  const int th = (h + 1) / 2, tw = (w + 1) / 2;
#pragma omp parallel for schedule(static)
  for (int ty = 0; ty < th; ++ty) {
    float* V = (float*)malloc(sizeof(float) * 16 * cin);
    float* M = (float*)malloc(sizeof(float) * 16 * cout);
    for (int tx = 0; tx < tw; ++tx) {
      for (int ci = 0; ci < cin; ++ci) {
        float d[4][4], t[4][4];
        for (int r = 0; r < 4; ++r)
          for (int c = 0; c < 4; ++c) {
            const int yy = 2 * ty - 1 + r, xx = 2 * tx - 1 + c;
            d[r][c] = (yy >= 0 && yy < h && xx >= 0 && xx < w) ? in[((size_t)yy * w + xx) * cin + ci] : 0.f;
          }
        for (int c = 0; c < 4; ++c) {
          t[0][c] = d[0][c] - d[2][c]; t[1][c] = d[1][c] + d[2][c];
          t[2][c] = d[2][c] - d[1][c]; t[3][c] = d[1][c] - d[3][c];
        }
        for (int i = 0; i < 4; ++i) {
          V[(i * 4 + 0) * cin + ci] = t[i][0] - t[i][2]; V[(i * 4 + 1) * cin + ci] = t[i][1] + t[i][2];
          V[(i * 4 + 2) * cin + ci] = t[i][2] - t[i][1]; V[(i * 4 + 3) * cin + ci] = t[i][1] - t[i][3];
        }
      }
      for (int xi = 0; xi < 16; ++xi) {
        float* m = M + (size_t)xi * cout;
        for (int co = 0; co < cout; ++co) m[co] = 0.f;
        for (int c8 = 0; c8 < cin; c8 += 8)
          for (int j = 0; j < 4; ++j)
            for (int hh = 0; hh < 2; ++hh) {
              const int ci = c8 + 4 * hh + j;
              const float v = V[xi * cin + ci];
              const float* u = U + ((size_t)xi * cin + ci) * cout;
              for (int co = 0; co < cout; ++co) m[co] = fmaf(v, u[co], m[co]);
            }
      }
      for (int co = 0; co < cout; ++co) {
        float s[4][2], y[2][2];
        for (int i = 0; i < 4; ++i) {
          const float m0 = M[(i * 4 + 0) * cout + co], m1 = M[(i * 4 + 1) * cout + co], m2 = M[(i * 4 + 2) * cout + co],
                      m3 = M[(i * 4 + 3) * cout + co];
          s[i][0] = (m0 + m1) + m2;
          s[i][1] = (m1 - m2) - m3;
        }
        for (int b = 0; b < 2; ++b) {
          y[0][b] = (s[0][b] + s[1][b]) + s[2][b];
          y[1][b] = (s[1][b] - s[2][b]) - s[3][b];
        }
        for (int p = 0; p < 2; ++p)
          for (int b = 0; b < 2; ++b) {
            const int oy = 2 * ty + p, ox = 2 * tx + b;
            if (oy >= h || ox >= w) continue;
            float v = y[p][b] + bias[co];
            if (relu) v = v > 0.f ? v : 0.f;
            out[((size_t)oy * w + ox) * cout + co] = v;
          }
      }
    }
    free(V);
    free(M);
  }
  free(U);
}

/* MaxPool2d(kernel 2, stride 2), NHWC.  superpoint.ipynb:304,336,339,342 */
ORC_API void orc_maxpool2(const float* in, int h, int w, int c, float* out) {
  const int ho = h / 2, wo = w / 2;
  for (int y = 0; y < ho; ++y)
    for (int x = 0; x < wo; ++x)
      for (int k = 0; k < c; ++k) {
        const float a = in[((size_t)(2 * y) * w + 2 * x) * c + k];
        const float b = in[((size_t)(2 * y) * w + 2 * x + 1) * c + k];
        const float d = in[((size_t)(2 * y + 1) * w + 2 * x) * c + k];
        const float e = in[((size_t)(2 * y + 1) * w + 2 * x + 1) * c + k];
        const float m0 = a > b ? a : b, m1 = d > e ? d : e;
        out[((size_t)y * wo + x) * c + k] = m0 > m1 ? m0 : m1;
      }
}

/* fma-only expf, identical instruction sequence on CPU (this file) and GPU (postproc.hip):
 * range reduction x = n ln2 + r, degree-6 polynomial (Cephes coefficients), ldexp.
 * Max error vs libm expf: <= 2 ulp on [-87, 0] (checked in tests/test_oracle.py). */
ORC_API float orc_expf(float x) {
  if (x < -87.0f) x = -87.0f;
  const float t = x * 1.44269504088896341f;
  const float n = rintf(t);
  float r = fmaf(n, -0.693359375f, x);
  r = fmaf(n, 2.12194440e-4f, r);
  float p = 1.9875691500E-4f;
  p = fmaf(p, r, 1.3981999507E-3f);
  p = fmaf(p, r, 8.3334519073E-3f);
  p = fmaf(p, r, 4.1665795894E-2f);
  p = fmaf(p, r, 1.6666665459E-1f);
  p = fmaf(p, r, 5.0000001201E-1f);
  const float r2 = r * r;
  const float y = fmaf(p, r2, r) + 1.0f;
  return ldexpf(y, (int)n);
}

/* softmax over 65 channels, drop dustbin (ch 64), unfold 8x8 cells to [H][W].
 * superpoint.ipynb:355-364.  logits: [hc][wc][65] (NHWC).  semi: [hc*8][wc*8]. */
ORC_API void orc_softmax_semi(const float* logits, int hc, int wc, float* semi) {
  const int W = wc * 8;
  for (int cy = 0; cy < hc; ++cy)
    for (int cx = 0; cx < wc; ++cx) {
      const float* l = logits + ((size_t)cy * wc + cx) * 65;
      float m = l[0];
      for (int c = 1; c < 65; ++c) m = l[c] > m ? l[c] : m;
      float e[65], s = 0.f;
      for (int c = 0; c < 65; ++c) {
        e[c] = orc_expf(l[c] - m);
        s += e[c];
      }
      for (int c = 0; c < 64; ++c)
        semi[(size_t)(cy * 8 + c / 8) * W + cx * 8 + (c % 8)] = e[c] / s;
    }
}

/* channel L2 normalisation of the dense descriptor map, NHWC [n][c].
 * superpoint.ipynb:352-353  (dn = norm(desc,2,dim=1); desc = desc / dn) */
ORC_API void orc_l2norm_rows(const float* in, int n, int c, float* out) {
  for (int i = 0; i < n; ++i) {
    float s = 0.f;
    for (int k = 0; k < c; ++k) s = fmaf(in[(size_t)i * c + k], in[(size_t)i * c + k], s);
    const float nrm = sqrtf(s);
    for (int k = 0; k < c; ++k) out[(size_t)i * c + k] = in[(size_t)i * c + k] / nrm;
  }
}

/* ------------------------------------------------------------------------------------------
 * A3/A4  Variant-B selection.  Reference: SuperPoint::processOutput :327-350,
 *        findHighScoreIndex :201-212, removeBorders :215-230, sortIndexes/topKeypoints :233-253
 *        (d2frontend/src/CNN/superpoint_tensorrt.cpp).  SURVEY.md Appendix B.1.
 * Returns number of keypoints (<= cap); kps_xy[2*i] = x, kps_xy[2*i+1] = y; idx_out = raster index.
 * ---------------------------------------------------------------------------------------- */
typedef struct { float s; int idx; } orc_cand;
static int orc_cand_cmp(const void* a, const void* b) {
  const orc_cand* p = (const orc_cand*)a; const orc_cand* q = (const orc_cand*)b;
  if (p->s > q->s) return -1;
  if (p->s < q->s) return 1;
  return p->idx < q->idx ? -1 : (p->idx > q->idx ? 1 : 0); /* deterministic tie-break */
}
ORC_API int orc_select_b(const float* semi, int h, int w, float thr, int border, int max_kp,
                         float* kps_xy, float* scores, int32_t* idx_out, int cap) {
  orc_cand* c = (orc_cand*)malloc(sizeof(orc_cand) * (size_t)h * w);
  int n = 0;
  for (int i = 0; i < h * w; ++i) {
    if (!(semi[i] > thr)) continue;                /* strict >  (:205) */
    const int x = i % w, y = i / w;
    if (!(y >= border && y < h - border && x >= border && x < w - border)) continue; /* :221-222 */
    c[n].s = semi[i]; c[n].idx = i; ++n;
  }
  if (max_kp != -1 && max_kp < n) {                /* :242  only then is anything sorted */
    qsort(c, n, sizeof(orc_cand), orc_cand_cmp);
    n = max_kp;
  }
  if (n > cap) n = cap;
  for (int i = 0; i < n; ++i) {
    kps_xy[2 * i] = (float)(c[i].idx % w);
    kps_xy[2 * i + 1] = (float)(c[i].idx / w);
    scores[i] = c[i].s;
    if (idx_out) idx_out[i] = c[i].idx;
  }
  free(c);
  return n;
}

/* ------------------------------------------------------------------------------------------
 * A5  Variant-B descriptor sampling.  Reference: normalize_keypoints :255-265, grid_sample :272-310,
 *     normalize_descriptors :312-317 (superpoint_tensorrt.cpp).  desc_map: NHWC [hc][wc][dim],
 *     already channel-L2-normalised (the engine's "desc" output).  s = 8.
 *     The mixed float/double arithmetic of the C++ source is reproduced literally.
 * ---------------------------------------------------------------------------------------- */
static int orc_clip(int v, int mx) { if (v < 0) return 0; return v < mx - 1 ? v : mx - 1; }
ORC_API void orc_sample_b(const float* desc_map, int hc, int wc, int dim, const float* kps_xy, int n,
                          float* out) {
  const int s = 8;
  for (int i = 0; i < n; ++i) {
    /* kp = {x - s/2 + 0.5, ...}: float - int -> float, + 0.5 (double) -> double -> stored float */
    float k0 = (float)((double)(kps_xy[2 * i] - (float)(s / 2)) + 0.5);
    float k1 = (float)((double)(kps_xy[2 * i + 1] - (float)(s / 2)) + 0.5);
    k0 = (float)((double)k0 / ((double)(wc * s - s / 2) - 0.5));
    k1 = (float)((double)k1 / ((double)(hc * s - s / 2) - 0.5));
    k0 = k0 * 2.0f - 1.0f;
    k1 = k1 * 2.0f - 1.0f;
    const float ix = ((k0 + 1.0f) / 2.0f) * (float)(wc - 1);
    const float iy = ((k1 + 1.0f) / 2.0f) * (float)(hc - 1);
    const int ix_nw = orc_clip((int)floorf(ix), wc), iy_nw = orc_clip((int)floorf(iy), hc);
    const int ix_ne = orc_clip(ix_nw + 1, wc), iy_ne = orc_clip(iy_nw, hc);
    const int ix_sw = orc_clip(ix_nw, wc), iy_sw = orc_clip(iy_nw + 1, hc);
    const int ix_se = orc_clip(ix_nw + 1, wc), iy_se = orc_clip(iy_nw + 1, hc);
    const float nw = ((float)ix_se - ix) * ((float)iy_se - iy);
    const float ne = (ix - (float)ix_sw) * ((float)iy_sw - iy);
    const float sw = ((float)ix_ne - ix) * (iy - (float)iy_ne);
    const float se = (ix - (float)ix_nw) * (iy - (float)iy_nw);
    const float* pnw = desc_map + ((size_t)iy_nw * wc + ix_nw) * dim;
    const float* pne = desc_map + ((size_t)iy_ne * wc + ix_ne) * dim;
    const float* psw = desc_map + ((size_t)iy_sw * wc + ix_sw) * dim;
    const float* pse = desc_map + ((size_t)iy_se * wc + ix_se) * dim;
    float* d = out + (size_t)i * dim;
    float ss = 0.f;
    for (int k = 0; k < dim; ++k) {
      float v = pnw[k] * nw;
      v = v + pne[k] * ne;
      v = v + psw[k] * sw;
      v = v + pse[k] * se;
      d[k] = v;
      ss += v * v;                                   /* Eigen norm(): sqrt(sum sq) in float */
    }
    const float ninv = (float)(1.0 / (double)sqrtf(ss)); /* double reciprocal, float scale (:314-315) */
    for (int k = 0; k < dim; ++k) d[k] = d[k] * ninv;
  }
}

/* ------------------------------------------------------------------------------------------
 * A6  Variant-A candidates + NMS2.  Reference: getKeyPoints superpoint_common.cpp:12-40,
 *     NMS2 :107-177.  SURVEY.md Appendix B.2.  CV_16UC1 index-map wraparound reproduced.
 * ---------------------------------------------------------------------------------------- */
ORC_API int orc_nms2_a(const float* prob, int h, int w, float thr, int dist_thresh, int border,
                       int max_num, float* kps_xy, float* scores, int cap) {
  const size_t hw = (size_t)h * w;
  int* cand = (int*)malloc(sizeof(int) * hw);
  uint8_t* grid = (uint8_t*)calloc(hw, 1);
  uint16_t* inds = (uint16_t*)calloc(hw, 2);
  float* conf = (float*)calloc(hw, 4);
  int n = 0;
  for (size_t i = 0; i < hw; ++i)
    if (prob[i] > thr) cand[n++] = (int)i;           /* cv::findNonZero raster order (:17-19) */
  for (int i = 0; i < n; ++i) {
    grid[cand[i]] = 1; inds[cand[i]] = (uint16_t)i; conf[cand[i]] = prob[cand[i]];
  }
  for (int i = 0; i < n; ++i) {
    const int uu = cand[i] % w, vv = cand[i] / w;
    if (grid[cand[i]] != 1) continue;
    for (int k = -dist_thresh; k < dist_thresh + 1; ++k)
      for (int j = -dist_thresh; j < dist_thresh + 1; ++j) {
        if (j == 0 && k == 0) continue;
        if (uu + j < 0 || uu + j >= w || vv + k < 0 || vv + k >= h) continue;
        if (conf[(size_t)(vv + k) * w + uu + j] < conf[cand[i]]) grid[(size_t)(vv + k) * w + uu + j] = 0;
      }
    grid[cand[i]] = 2;
  }
  orc_cand* kept = (orc_cand*)malloc(sizeof(orc_cand) * (size_t)(n > 0 ? n : 1));
  orc_cand* dec = (orc_cand*)malloc(sizeof(orc_cand) * (size_t)(n > 0 ? n : 1));
  int m = 0;
  for (int v = 0; v < h; ++v)
    for (int u = 0; u < w; ++u) {
      if (u >= w - border || u < border || v >= h - border || v < border) continue;
      if (grid[(size_t)v * w + u] == 2) {
        const int sel = inds[(size_t)v * w + u];      /* u16 wrap: pts_raw[select_ind] */
        kept[m].idx = cand[sel]; kept[m].s = conf[(size_t)v * w + u]; ++m;
      }
    }
  /* std::sort by confidence desc (:172); oracle tie-break = raster-scan position (stable) */
  for (int i = 0; i < m; ++i) { dec[i].s = kept[i].s; dec[i].idx = i; }
  qsort(dec, m, sizeof(orc_cand), orc_cand_cmp);
  {
    int nout = m < max_num ? m : max_num;
    if (nout > cap) nout = cap;
    for (int i = 0; i < nout; ++i) {
      const int src = kept[dec[i].idx].idx;
      kps_xy[2 * i] = (float)(src % w);
      kps_xy[2 * i + 1] = (float)(src / w);
      scores[i] = dec[i].s;
    }
    m = nout;
  }
  free(dec);
  free(kept); free(cand); free(grid); free(inds); free(conf);
  return m;
}

/* ------------------------------------------------------------------------------------------
 * A7  Variant-A descriptor sampling.  Reference: computeDescriptors superpoint_common.cpp:42-99.
 *     grid = 2*x/W - 1 ; torch::grid_sampler(bilinear, zeros padding, align_corners=false)
 *     => ix = ((g+1)*wc - 1)/2.  The sampled tensor is squeezed to [256, n_keypoints] and then
 *     `dn = torch::norm(desc, 2, 1); desc = desc.div(unsqueeze(dn, 1))` (:68-69) -- dim 1 of that tensor is
 *     the KEYPOINT axis, so every CHANNEL is divided by its L2 norm over the image's keypoints (the
 *     notebook module the C++ was written from does the same, superpoint.ipynb cell 1; pinned by
 *     tests/golden/reference_notebook.npz).  Only then: optional PCA (d - mean) * comp_T (:76-78), and the
 *     per-keypoint L2 normalisation (:79-81 / :87-89).  Reproduced as written.
 *     Order fixed here: the channel norm sums over keypoints in list order, fp32.
 *     desc_map NHWC [hc][wc][dim] already channel-normalised.  pca_comp: [pca_dims][dim] (the CSV
 *     layout, superpoint_onnx.cpp:47-53) or NULL.
 * ---------------------------------------------------------------------------------------- */
ORC_API void orc_sample_a(const float* desc_map, int hc, int wc, int dim, int img_w, int img_h,
                          const float* kps_xy, int n, const float* pca_comp, const float* pca_mean,
                          int pca_dims, float* out) {
  if (n <= 0) return;
  float* S = (float*)malloc(sizeof(float) * (size_t)n * dim);
  float* cn = (float*)malloc(sizeof(float) * dim);
  for (int i = 0; i < n; ++i) {
    /* grid built in float tensors: 2.0 * x / width - 1 */
    const float gx = 2.0f * kps_xy[2 * i] / (float)img_w - 1.0f;
    const float gy = 2.0f * kps_xy[2 * i + 1] / (float)img_h - 1.0f;
    /* ATen grid_sampler_unnormalize, align_corners=false: ((coord + 1) * size - 1) / 2 */
    const float ix = ((gx + 1.0f) * (float)wc - 1.0f) / 2.0f;
    const float iy = ((gy + 1.0f) * (float)hc - 1.0f) / 2.0f;
    const float fx = floorf(ix), fy = floorf(iy);
    const int x0 = (int)fx, y0 = (int)fy, x1 = x0 + 1, y1 = y0 + 1;
    /* ATen: nw = (ix_se - ix)*(iy_se - iy) ... */
    const float nw = ((float)x1 - ix) * ((float)y1 - iy);
    const float ne = (ix - (float)x0) * ((float)y1 - iy);
    const float sw = ((float)x1 - ix) * (iy - (float)y0);
    const float se = (ix - (float)x0) * (iy - (float)y0);
    for (int k = 0; k < dim; ++k) {
      float v = 0.f;
      if (y0 >= 0 && y0 < hc && x0 >= 0 && x0 < wc) v += desc_map[((size_t)y0 * wc + x0) * dim + k] * nw;
      if (y0 >= 0 && y0 < hc && x1 >= 0 && x1 < wc) v += desc_map[((size_t)y0 * wc + x1) * dim + k] * ne;
      if (y1 >= 0 && y1 < hc && x0 >= 0 && x0 < wc) v += desc_map[((size_t)y1 * wc + x0) * dim + k] * sw;
      if (y1 >= 0 && y1 < hc && x1 >= 0 && x1 < wc) v += desc_map[((size_t)y1 * wc + x1) * dim + k] * se;
      S[(size_t)i * dim + k] = v;
    }
  }
  for (int k = 0; k < dim; ++k) {                 /* :68 torch::norm(desc [dim, n], 2, 1) */
    float ss = 0.f;
    for (int i = 0; i < n; ++i) ss += S[(size_t)i * dim + k] * S[(size_t)i * dim + k];
    cn[k] = sqrtf(ss);
  }
  for (int i = 0; i < n; ++i) {
    float* t = S + (size_t)i * dim;
    for (int k = 0; k < dim; ++k) t[k] = t[k] / cn[k];   /* :69 */
    if (pca_comp) {
      float s2 = 0.f;
      float* o = out + (size_t)i * pca_dims;
      for (int j = 0; j < pca_dims; ++j) {
        float a = 0.f;
        for (int k = 0; k < dim; ++k) a += (t[k] - pca_mean[k]) * pca_comp[(size_t)j * dim + k];
        o[j] = a; s2 += a * a;
      }
      const float n2 = sqrtf(s2);
      for (int j = 0; j < pca_dims; ++j) o[j] = o[j] / n2;
    } else {
      float s2 = 0.f;
      for (int k = 0; k < dim; ++k) s2 += t[k] * t[k];
      const float n2 = sqrtf(s2);
      for (int k = 0; k < dim; ++k) out[(size_t)i * dim + k] = t[k] / n2;
    }
  }
  free(S); free(cn);
}

/* ------------------------------------------------------------------------------------------
 * A10  matchKNN.  Reference: d2frontend/src/feature_matcher.cpp:4-42.   SURVEY.md Appendix B.3.
 * Third-party arithmetic restated: OpenCV 4.10.0 (docker/Dockerfile.x86:6) cv::BFMatcher(NORM_L2)
 * -> batchDistance -> normL2Sqr_(float) then std::sqrt.  The accumulation order fixed here is that
 * of the x86-64 baseline (SSE2, 128-bit universal intrinsics) build of
 * modules/core/src/norm.cpp normL2Sqr_: four 4-lane accumulators over 16-element strides,
 * v_muladd = separate mul and add, d = reduce_sum((d0+d1)+d2)+d3), scalar tail.
 * knn ordering: ascending distance, ties keep the lower train index (strict '<' insertion).
 * ---------------------------------------------------------------------------------------- */
ORC_API float orc_l2_dist(const float* a, const float* b, int n) {
  float acc[4][4];
  memset(acc, 0, sizeof(acc));
  int j = 0;
  for (; j <= n - 16; j += 16)
    for (int v = 0; v < 4; ++v)
      for (int l = 0; l < 4; ++l) {
        const float t = a[j + 4 * v + l] - b[j + 4 * v + l];
        const float tt = t * t;
        acc[v][l] = acc[v][l] + tt;
      }
  float r[4];
  for (int l = 0; l < 4; ++l) r[l] = ((acc[0][l] + acc[1][l]) + acc[2][l]) + acc[3][l];
  /* v_reduce_sum (SSE): (r0 + r2) + (r1 + r3) */
  float d = (r[0] + r[2]) + (r[1] + r[3]);
  for (; j < n; ++j) { const float t = a[j] - b[j]; d += t * t; }
  return sqrtf(d);
}

static void orc_knn2(const float* q, int nq, const float* t, int nt, int dim, int* i0, float* d0,
                     int* i1, float* d1) {
#pragma omp parallel for schedule(static)
  for (int i = 0; i < nq; ++i) {
    int b0 = -1, b1 = -1; float e0 = INFINITY, e1 = INFINITY;
    for (int j = 0; j < nt; ++j) {
      const float d = orc_l2_dist(q + (size_t)i * dim, t + (size_t)j * dim, dim);
      if (d < e0) { e1 = e0; b1 = b0; e0 = d; b0 = j; }
      else if (d < e1) { e1 = d; b1 = j; }
    }
    i0[i] = b0; d0[i] = e0; i1[i] = b1; d1[i] = e1;
  }
}

ORC_API int orc_match_knn(const float* a, int na, const float* b, int nb, int dim, double ratio,
                          const float* pts_a, const float* pts_b, double radius, int32_t* q_idx,
                          int32_t* t_idx, float* dist, int cap) {
  if (na <= 0 || nb <= 0) return 0;
  int *f0 = (int*)malloc(sizeof(int) * na), *f1 = (int*)malloc(sizeof(int) * na);
  float *fd0 = (float*)malloc(sizeof(float) * na), *fd1 = (float*)malloc(sizeof(float) * na);
  int *g0 = (int*)malloc(sizeof(int) * nb), *g1 = (int*)malloc(sizeof(int) * nb);
  float *gd0 = (float*)malloc(sizeof(float) * nb), *gd1 = (float*)malloc(sizeof(float) * nb);
  int* inv = (int*)malloc(sizeof(int) * nb);
  orc_knn2(a, na, b, nb, dim, f0, fd0, f1, fd1);
  orc_knn2(b, nb, a, na, dim, g0, gd0, g1, gd1);
  for (int j = 0; j < nb; ++j) {
    inv[j] = -1;
    if (na < 2) continue;                                    /* match.size() < 2 (:18-20) */
    if ((double)gd0[j] < ratio * (double)gd1[j]) inv[j] = g0[j];   /* :21-23 */
  }
  int n = 0;
  for (int i = 0; i < na; ++i) {
    if (nb < 2) continue;                                    /* :27-29 */
    if ((double)fd0[i] < ratio * (double)fd1[i] && inv[f0[i]] == i) {
      if (radius > 0) {
        /* cv::norm(Point2f) = sqrt((double)x*x + (double)y*y) */
        const float dx = pts_a[2 * i] - pts_b[2 * f0[i]], dy = pts_a[2 * i + 1] - pts_b[2 * f0[i] + 1];
        const double nr = sqrt((double)dx * dx + (double)dy * dy);
        if (nr > radius) continue;
      }
      if (n < cap) { q_idx[n] = i; t_idx[n] = f0[i]; dist[n] = fd0[i]; }
      ++n;
    }
  }
  free(f0); free(f1); free(fd0); free(fd1); free(g0); free(g1); free(gd0); free(gd1); free(inv);
  return n < cap ? n : cap;
}

/* A11 cross-check matcher: cv::BFMatcher(NORM_L2, true).match  (loop_cam.cpp:167-170,
 * d2featuretracker.cpp:1141-1142).  OpenCV crossCheck semantics: knnMatch(k=1) both ways; keep (i,j)
 * iff j = argmin_j d(i,j) and i = argmin_i d(i,j) (first minimum on ties).  Output ascending i. */
ORC_API int orc_match_crosscheck(const float* a, int na, const float* b, int nb, int dim, int32_t* q_idx,
                                 int32_t* t_idx, float* dist, int cap) {
  if (na <= 0 || nb <= 0) return 0;
  int *f0 = (int*)malloc(sizeof(int) * na), *f1 = (int*)malloc(sizeof(int) * na);
  float *fd0 = (float*)malloc(sizeof(float) * na), *fd1 = (float*)malloc(sizeof(float) * na);
  int *g0 = (int*)malloc(sizeof(int) * nb), *g1 = (int*)malloc(sizeof(int) * nb);
  float *gd0 = (float*)malloc(sizeof(float) * nb), *gd1 = (float*)malloc(sizeof(float) * nb);
  orc_knn2(a, na, b, nb, dim, f0, fd0, f1, fd1);
  orc_knn2(b, nb, a, na, dim, g0, gd0, g1, gd1);
  int n = 0;
  for (int i = 0; i < na; ++i)
    if (f0[i] >= 0 && g0[f0[i]] == i) {
      if (n < cap) { q_idx[n] = i; t_idx[n] = f0[i]; dist[n] = fd0[i]; }
      ++n;
    }
  free(f0); free(f1); free(fd0); free(fd1); free(g0); free(g1); free(gd0); free(gd1);
  return n < cap ? n : cap;
}

/* A12 half-image filter.  Reference: getFeatureHalfImg d2featuretracker.cpp:1051-1075.
 * move_cols = width_undistort * 90.0 / undistort_fov (float).  Returns count; map[c] = source index. */
ORC_API int orc_half_img(const float* pts_xy, int n, int require_left, int width_undistort,
                         double undistort_fov, int32_t* map) {
  const float move_cols = (float)((double)width_undistort * 90.0 / undistort_fov);
  int c = 0;
  for (int i = 0; i < n; ++i) {
    const float x = pts_xy[2 * i];
    if ((require_left && x < (float)width_undistort - move_cols) || (!require_left && x >= move_cols))
      map[c++] = i;
  }
  return c;
}

/* ------------------------------------------------------------------------------------------
 * A9  NetVLAD global descriptor.  Reference call site: MobileNetVLADONNX::inference,
 *     d2frontend/include/d2frontend/CNN/mobilenetvlad_onnx.h:49-74 (input: gray, resized, float, NOT scaled (:60),
 *     NHWC [1,H,W,1] "image:0" -> "descriptor:0" [1,4096]; optional PCA y = comp (x - mean), y/|y| (:66-71)).
 *     THE GRAPH ITSELF IS NOT IN THE REFERENCE TREE (mobilenetvlad_dyn_size.onnx is a missing blob):
 *     the network below is a documented STAND-IN of the HF-Net MobileNetVLAD lineage (MobileNetV2 trunk, in-graph
 *     (x-128)/128 normalisation, 1x1 pre-projection, NetVLAD soft-assignment/aggregation, intra + global L2).
 *     Parity for A9 is therefore unpinned twice over: no golden vectors AND no pinned architecture.
 *     Generic layer primitives (TensorFlow "SAME" padding, BatchNorm folded into weight/bias):
 * ---------------------------------------------------------------------------------------- */
static float orc_act(float v, int act) { /* 0 none, 1 relu, 2 relu6 */
  if (act >= 1 && v < 0.f) v = 0.f;
  if (act == 2 && v > 6.f) v = 6.f;
  return v;
}
/* TF SAME: out = ceil(in/stride); pad_total = max((out-1)*stride + k - in, 0); pad_before = pad_total/2 */
static int orc_same_pad(int in, int k, int stride, int* out) {
  *out = (in + stride - 1) / stride;
  int pt = (*out - 1) * stride + k - in;
  if (pt < 0) pt = 0;
  return pt / 2;
}

/* full conv, NHWC, wgt [cout][cin][k][k], stride, TF-SAME padding, activation */
ORC_API void orc_conv2d_same(const float* in, int h, int w, int cin, const float* wgt, const float* bias, int cout,
                             int k, int stride, int act, float* out) {
  int ho, wo;
  const int pt = orc_same_pad(h, k, stride, &ho), pl = orc_same_pad(w, k, stride, &wo);
#pragma omp parallel for schedule(static)
  for (int y = 0; y < ho; ++y)
    for (int x = 0; x < wo; ++x)
      for (int co = 0; co < cout; ++co) {
        float acc = bias[co];
        for (int ky = 0; ky < k; ++ky) {
          const int yy = y * stride + ky - pt;
          if (yy < 0 || yy >= h) continue;
          for (int kx = 0; kx < k; ++kx) {
            const int xx = x * stride + kx - pl;
            if (xx < 0 || xx >= w) continue;
            for (int ci = 0; ci < cin; ++ci)
              acc = fmaf(in[((size_t)yy * w + xx) * cin + ci], wgt[(((size_t)co * cin + ci) * k + ky) * k + kx], acc);
          }
        }
        out[((size_t)y * wo + x) * cout + co] = orc_act(acc, act);
      }
}

/* depthwise 3x3, NHWC, wgt [c][3][3], stride, TF-SAME, activation */
ORC_API void orc_dwconv3x3_same(const float* in, int h, int w, int c, const float* wgt, const float* bias, int stride,
                                int act, float* out) {
  int ho, wo;
  const int pt = orc_same_pad(h, 3, stride, &ho), pl = orc_same_pad(w, 3, stride, &wo);
#pragma omp parallel for schedule(static)
  for (int y = 0; y < ho; ++y)
    for (int x = 0; x < wo; ++x)
      for (int k = 0; k < c; ++k) {
        float acc = bias[k];
        for (int ky = 0; ky < 3; ++ky) {
          const int yy = y * stride + ky - pt;
          if (yy < 0 || yy >= h) continue;
          for (int kx = 0; kx < 3; ++kx) {
            const int xx = x * stride + kx - pl;
            if (xx < 0 || xx >= w) continue;
            acc = fmaf(in[((size_t)yy * w + xx) * c + k], wgt[(k * 3 + ky) * 3 + kx], acc);
          }
        }
        out[((size_t)y * wo + x) * c + k] = orc_act(acc, act);
      }
}

/* NetVLAD head on a feature map x [np][d] (already pre-projected): soft-assignment a = softmax_k(x W_a + b_a),
 * V[k][:] = sum_p a[p][k] (c[k][:] - x[p][:])  (HF-Net sign convention), intra-normalise each V[k], flatten k-major,
 * global L2.  assign_w [K][d], centroids [K][d].  out [K*d]. */
ORC_API void orc_netvlad_head(const float* x, int np, int d, const float* assign_w, const float* assign_b,
                              const float* centroids, int K, float* out) {
  double* V = (double*)calloc((size_t)K * d, sizeof(double));
  float* a = (float*)malloc(sizeof(float) * K);
  for (int p = 0; p < np; ++p) {
    float m = -INFINITY;
    for (int k = 0; k < K; ++k) {
      float s = assign_b[k];
      for (int j = 0; j < d; ++j) s = fmaf(x[(size_t)p * d + j], assign_w[(size_t)k * d + j], s);
      a[k] = s; if (s > m) m = s;
    }
    float sum = 0.f;
    for (int k = 0; k < K; ++k) { a[k] = expf(a[k] - m); sum += a[k]; }
    for (int k = 0; k < K; ++k) {
      const float ak = a[k] / sum;
      for (int j = 0; j < d; ++j) V[(size_t)k * d + j] += (double)ak * ((double)centroids[(size_t)k * d + j] - (double)x[(size_t)p * d + j]);
    }
  }
  double tot = 0.0;
  for (int k = 0; k < K; ++k) {
    double s = 0.0;
    for (int j = 0; j < d; ++j) s += V[(size_t)k * d + j] * V[(size_t)k * d + j];
    const double n = sqrt(s) > 1e-12 ? sqrt(s) : 1e-12;
    for (int j = 0; j < d; ++j) { V[(size_t)k * d + j] /= n; tot += V[(size_t)k * d + j] * V[(size_t)k * d + j]; }
  }
  const double nt = sqrt(tot) > 1e-12 ? sqrt(tot) : 1e-12;
  for (size_t i = 0; i < (size_t)K * d; ++i) out[i] = (float)(V[i] / nt);
  free(V); free(a);
}

/* PCA of the global descriptor: y = comp (x - mean); y /= |y|   (mobilenetvlad_onnx.h:66-71).  comp [m][n]. */
ORC_API void orc_netvlad_pca(const float* x, int n, const float* comp, const float* mean, int m, float* out) {
  double tot = 0.0;
  double* y = (double*)malloc(sizeof(double) * m);
  for (int i = 0; i < m; ++i) {
    double s = 0.0;
    for (int j = 0; j < n; ++j) s += (double)comp[(size_t)i * n + j] * ((double)x[j] - (double)mean[j]);
    y[i] = s; tot += s * s;
  }
  const double nt = sqrt(tot);
  for (int i = 0; i < m; ++i) out[i] = (float)(y[i] / nt);
  free(y);
}

/* ==========================================================================================
 * SURVEY.md section 8(f) "next" rows
 * ========================================================================================== */

/* (f)-1 fisheye undistort + photometric gain.  Reference: FisheyeUndist::undist_id_cuda,
 * d2common/include/d2common/fisheye_undistort.h:152-176: cv::cuda::remap(INTER_LINEAR (:28), BORDER_CONSTANT 0) ->
 * convertTo(CV_32F) -> cv::cuda::multiply(gain) -> convertTo(CV_8U).
 * Third-party arithmetic restated (OpenCV 4.10 cudev LinearFilter + saturate_cast, not in /root/reference):
 * x1 = floor(x), x2 = x1+1; out = 0; out += src(y1,x1)*((x2-x)*(y2-y)); += src(y1,x2)*((x-x1)*(y2-y));
 * += src(y2,x1)*((x2-x)*(y-y1)); += src(y2,x2)*((x-x1)*(y-y1)) with zero outside the image, separate mul and add;
 * saturate_cast<uchar>(float) = round-to-nearest-even, clamped to [0,255]. */
static uint8_t orc_sat_u8(float v) {
  if (!(v > 0.f)) return 0;
  if (v >= 255.f) return 255;
  return (uint8_t)rintf(v);
}
ORC_API void orc_undistort(const uint8_t* src, int sh, int sw, int sstride, const float* mapx, const float* mapy,
                           const float* gain, int dh, int dw, uint8_t* dst) {
  for (int i = 0; i < dh * dw; ++i) {
    const float x = mapx[i], y = mapy[i];
    const float fx = floorf(x), fy = floorf(y);
    const int x1 = (int)fx, y1 = (int)fy, x2 = x1 + 1, y2 = y1 + 1;
#define ORC_S(yy, xx) (((yy) >= 0 && (yy) < sh && (xx) >= 0 && (xx) < sw) ? (float)src[(size_t)(yy) * sstride + (xx)] : 0.f)
    float out = 0.f;
    out = out + ORC_S(y1, x1) * (((float)x2 - x) * ((float)y2 - y));
    out = out + ORC_S(y1, x2) * ((x - (float)x1) * ((float)y2 - y));
    out = out + ORC_S(y2, x1) * (((float)x2 - x) * (y - (float)y1));
    out = out + ORC_S(y2, x2) * ((x - (float)x1) * (y - (float)y1));
#undef ORC_S
    uint8_t u = orc_sat_u8(out);
    if (gain) u = orc_sat_u8((float)u * gain[i]);
    dst[i] = u;
  }
}

/* (f)-2 NetVLAD database: faiss::IndexFlatIP add/search (d2frontend/src/loop_detector.cpp:254-263,318) and the gate of
 * LoopDetector::queryIndexFromDatabase (:300-350): k = min(SEARCH_NEAREST_NUM(5) + max_index, ntotal) nearest by inner
 * product, descending; the first one with label <= ntotal - max_index and similarity > thres wins.
 * faiss 1.7.4's SIMD summation order and heap tie order are unspecified; the oracle uses a sequential fmaf dot and
 * breaks similarity ties by the lower label.  Returns the gated label (or -1); fills the k labels / similarities. */
ORC_API int orc_db_query(const float* db, int ntotal, int dim, const float* q, int search_nearest, int max_index,
                         double thres, int32_t* labels, float* sims, int* k_out, float* sim_out) {
  int k = search_nearest + max_index;
  if (k > ntotal) k = ntotal;
  *k_out = k > 0 ? k : 0;
  if (k <= 0) return -1;
  float* s = (float*)malloc(sizeof(float) * ntotal);
  for (int i = 0; i < ntotal; ++i) {
    float a = 0.f;
    for (int j = 0; j < dim; ++j) a = fmaf(db[(size_t)i * dim + j], q[j], a);
    s[i] = a;
  }
  uint8_t* used = (uint8_t*)calloc(ntotal, 1);
  for (int r = 0; r < k; ++r) {
    int best = -1;
    for (int i = 0; i < ntotal; ++i)
      if (!used[i] && (best < 0 || s[i] > s[best])) best = i;
    used[best] = 1; labels[r] = best; sims[r] = s[best];
  }
  free(used); free(s);
  for (int r = 0; r < k; ++r)
    if (labels[r] <= ntotal - max_index && (double)sims[r] > thres) { *sim_out = sims[r]; return labels[r]; }
  return -1;
}

/* (f)-3 int8 wire codec of descriptors.  Reference: VisualImageDesc::toLCM
 * (d2common/include/d2common/d2frontend_types.h:228-237 landmark descriptors: float max; :260-268 NetVLAD: double max)
 * and the LCM constructor (:313-351): x = q/127.0, landmark descriptors re-normalised in hard-coded 32-float segments
 * for i < landmark_num (:326-328), the global descriptor normalised as a whole (:337). */
ORC_API void orc_quant_int8(const float* x, int n, int double_max, int8_t* out) {
  float m = 0.f;
  for (int i = 0; i < n; ++i) { const float a = fabsf(x[i]); if (a > m) m = a; }
  if (!(m > 0.f)) {                      /* an all-zero tensor: the reference divides 0 by 0 and casts the NaN (undefined); defined as zeros here */
    for (int i = 0; i < n; ++i) out[i] = 0;
  } else if (double_max) {
    const double md = (double)m;
    for (int i = 0; i < n; ++i) out[i] = (int8_t)((double)x[i] / md * 127);
  } else {
    for (int i = 0; i < n; ++i) out[i] = (int8_t)(x[i] / m * 127);
  }
}
ORC_API void orc_dequant_int8(const int8_t* q, int n, int landmark_num, float* out) {
  for (int i = 0; i < n; ++i) out[i] = (float)((double)q[i] / 127.0);
  if (landmark_num >= 0) {
    for (int i = 0; i < landmark_num && (i + 1) * 32 <= n; ++i) {
      float s = 0.f;
      for (int j = 0; j < 32; ++j) s += out[i * 32 + j] * out[i * 32 + j];
      if (!(s > 0.f)) continue;            /* Eigen's normalize(): z = squaredNorm(); if (z > 0) derived() /= sqrt(z)  (Dot.h) */
      const float nr = sqrtf(s);
      for (int j = 0; j < 32; ++j) out[i * 32 + j] = out[i * 32 + j] / nr;
    }
  } else {
    float s = 0.f;
    for (int i = 0; i < n; ++i) s += out[i] * out[i];
    if (!(s > 0.f)) return;
    const float nr = sqrtf(s);
    for (int i = 0; i < n; ++i) out[i] = out[i] / nr;
  }
}

/* NetVLAD gate of the feature tracker: D2FeatureTracker::getMatchedPrevKeyframe (d2frontend/src/d2featuretracker.cpp:166-235) and, for
 * FOURCORNER_FISHEYE, the view pairing of trackRemoteFrames (:270-284).
 *   quadcam == 0 (STEREO_PINHOLE / PINHOLE_DEPTH / MONOCULAR, :173-205): keyframes newest first; view 0 of the remote frame against view 0
 *     of the keyframe; the first keyframe with !(sim < thres) wins, dir_a = dir_b = 0.
 *   quadcam != 0 (:206-233): dir_a = 2; remote view 2 against the keyframe's views dirs = {2,3,0,1} in that order; first pass wins,
 *     dir_b = dirs[j]; then the pairs (dir_a = (2+k)%4, dir_b = ((dir_b0 - 2 + 4)%4 + 2 + k)%4), k = 0..3, kept when both views have
 *     SuperPoint landmarks (sp counts may be NULL = all non-empty).
 * remote [n_views][dim], keyframes [n_kf][n_views][dim] (oldest first, as current_keyframes).  The similarity is an fp32 dot product
 * (Eigen::VectorXf::dot; sequential sum here, Eigen reduces in packets) compared in double.  Returns 1 when a keyframe matched. */
ORC_API int orc_tracker_gate(int quadcam, const float* remote, const int* sp_remote, const float* keyframes, const int* sp_kf, int n_kf,
                             int n_views, int dim, double thres, int* kf_idx, int* dir_a, int* dir_b, int* pairs_cur, int* pairs_prev,
                             int* n_pairs, float* sims4) {
  static const int dirs[4] = {2, 3, 0, 1};
  *n_pairs = 0; *kf_idx = -1; *dir_a = 0; *dir_b = 0;
  if (n_kf == 0) return 0;
  for (int k = n_kf - 1; k >= 0; --k) {
    const float* kf = keyframes + (size_t)k * n_views * dim;
    if (!quadcam) {
      float s = 0.f;
      for (int j = 0; j < dim; ++j) s += kf[j] * remote[j];
      if (sims4) sims4[0] = s;
      if (!((double)s < thres)) { *kf_idx = k; return 1; }
    } else {
      const float* r2 = remote + (size_t)2 * dim;
      for (int j = 0; j < n_views && j < 4; ++j) {
        const float* v = kf + (size_t)dirs[j] * dim;
        float s = 0.f;
        for (int e = 0; e < dim; ++e) s += v[e] * r2[e];
        if (sims4) sims4[j] = s;
        if (!((double)s < thres)) {
          *kf_idx = k; *dir_a = 2; *dir_b = dirs[j];
          for (int _a = 2; _a < 6; ++_a) {
            const int a = _a % 4, b = ((dirs[j] - 2 + 4) % 4 + _a) % 4;
            if (a < n_views && b < n_views && (!sp_kf || sp_kf[k * n_views + b] > 0) && (!sp_remote || sp_remote[a] > 0)) {
              pairs_cur[*n_pairs] = a; pairs_prev[*n_pairs] = b; ++*n_pairs;
            }
          }
          return 1;
        }
      }
    }
  }
  return 0;
}

/* ------------------------------------------------------------------------------------------
 * Section 8(f)-1, map generation: FisheyeUndist::generateCylinderMap + genOneUndistMap
 * (d2common/include/d2common/fisheye_undistort.h:458-500,559-613) and the pinhole variant of genOneUndistMap
 * (:615-660, used by generateAllUndistMap :346-456).  The fisheye camera is camodocal's CataCamera (MEI model,
 * "omni" + "radtan" in config/quadcam/quad_cam_calib-*.yaml): spaceToPlane camera_models/src/camera_models/CataCamera.cc:495-515,
 * distortion :617-633.  The virtual camera is CylindricalCamera::liftProjective (CylindricalCamera.cc:207-220) with
 * fx = fy = width / fov_rad, cx = width/2, cy = height/2 (integer divisions of the unsigned sizes, as in the reference).
 * All arithmetic in double; the map stores (float)x, (float)y.  cam[9] = xi k1 k2 p1 p2 gamma1 gamma2 u0 v0.
 * ------------------------------------------------------------------------------------------ */
static void mei_space_to_plane(const double* cam, double X, double Y, double Z, double* u, double* v) {
  const double xi = cam[0], k1 = cam[1], k2 = cam[2], p1 = cam[3], p2 = cam[4];
  const double nrm = sqrt(X * X + (Y * Y + Z * Z));          /* Eigen's 3-vector redux: x^2 + (y^2 + z^2) */
  const double z = Z + xi * nrm;
  const double pu0 = X / z, pu1 = Y / z;
  const double mx2 = pu0 * pu0, my2 = pu1 * pu1, mxy = pu0 * pu1, rho2 = mx2 + my2;
  const double rad = k1 * rho2 + k2 * rho2 * rho2;
  const double d0 = pu0 * rad + 2.0 * p1 * mxy + p2 * (rho2 + 2.0 * mx2);
  const double d1 = pu1 * rad + 2.0 * p2 * mxy + p1 * (rho2 + 2.0 * my2);
  *u = cam[5] * (pu0 + d0) + cam[7];
  *v = cam[6] * (pu1 + d1) + cam[8];
}

ORC_API void orc_gen_cylinder_map(const double* cam, int width, int height, double fov_deg, float* mapx, float* mapy) {
  const double fov = fov_deg * (M_PI / 180.0);
  const double f = (double)(unsigned)width / fov;
  const double cx = (double)((unsigned)width / 2), cy = (double)((unsigned)height / 2);
  const double iK11 = 1.0 / f, iK13 = -cx / f, iK22 = 1.0 / f, iK23 = -cy / f;
  for (int y = 0; y < height; ++y)
    for (int x = 0; x < width; ++x) {
      const double phi = iK11 * (double)x + iK13;
      const double ybr = iK22 * (double)y + iK23;
      const double z = fabs(phi) > M_PI / 2 ? -1.0 : 1.0;
      const double X = z * tan(phi);
      const double rho = sqrt(X * X + z * z);
      double u, v;
      mei_space_to_plane(cam, X, ybr * rho, z, &u, &v);
      mapx[(size_t)y * width + x] = (float)u;
      mapy[(size_t)y * width + x] = (float)v;
    }
}

/* q = (w, x, y, z); Eigen::Quaterniond * Vector3d: uv = 2 (q.vec x v); v + w uv + q.vec x uv */
ORC_API void orc_gen_pinhole_map(const double* cam, const double* q, int width, int height, double f, float* mapx, float* mapy) {
  const double w = q[0], qx = q[1], qy = q[2], qz = q[3];
  for (int y = 0; y < height; ++y)
    for (int x = 0; x < width; ++x) {
      const double vx = (double)x - (double)(unsigned)width / 2, vy = (double)y - (double)(unsigned)height / 2, vz = f;
      double ux = qy * vz - qz * vy, uy = qz * vx - qx * vz, uz = qx * vy - qy * vx;
      ux = ux + ux; uy = uy + uy; uz = uz + uz;
      const double cx = qy * uz - qz * uy, cy = qz * ux - qx * uz, cz = qx * uy - qy * ux;
      double u, v;
      mei_space_to_plane(cam, (vx + w * ux) + cx, (vy + w * uy) + cy, (vz + w * uz) + cz, &u, &v);
      mapx[(size_t)y * width + x] = (float)u;
      mapy[(size_t)y * width + x] = (float)v;
    }
}

/* ------------------------------------------------------------------------------------------
 * A1, variant A / NetVLAD image prep: cv::cvtColor(COLOR_BGR2GRAY) when the frame has 3 channels and cv::resize(INTER_LINEAR)
 * when its size differs from the network's (superpoint_onnx.cpp:76-83, mobilenetvlad_onnx.h:51-59).  Third-party arithmetic
 * (OpenCV 4.10.0, docker/Dockerfile.x86:6) restated -- parity unpinned:
 *   gray = (B*3735 + G*19235 + R*9798 + 2^14) >> 15                       (color_rgb: BY15, GY15, RY15, gray_shift 15)
 *   resize 8U INTER_LINEAR: 11-bit fixed-point weights saturate_cast<short>(w * 2048), horizontal pass in int,
 *   vertical pass ((b0*(S0>>4))>>16) + ((b1*(S1>>4))>>16) + 2) >> 2; source coordinate (d + 0.5)*scale - 0.5 in float;
 *   an exact 2x decimation is silently computed as INTER_AREA: (s00 + s01 + s10 + s11 + 2) >> 2.
 * ------------------------------------------------------------------------------------------ */
ORC_API void orc_bgr2gray(const uint8_t* bgr, int w, int h, int stride, uint8_t* gray) {
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      const uint8_t* p = bgr + (size_t)y * stride + 3 * x;
      gray[(size_t)y * w + x] = (uint8_t)((p[0] * 3735 + p[1] * 19235 + p[2] * 9798 + (1 << 14)) >> 15);
    }
}

static void resize_coef(int d, int ssize, int dsize, int* ofs, int* c0, int* c1, int clamp_ofs) {
  const double scale = 1.0 / ((double)dsize / (double)ssize);
  float f = (float)(((double)d + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  if (clamp_ofs) {
    if (s < 0) { f = 0.f; s = 0; }
    if (s >= ssize - 1) { f = 0.f; s = ssize - 1; }
  }
  *ofs = s;
  *c0 = (int)lrintf((1.f - f) * 2048.f);
  *c1 = (int)lrintf(f * 2048.f);
}

ORC_API void orc_resize_linear_u8(const uint8_t* src, int sw, int sh, int sstride, uint8_t* dst, int dw, int dh) {
  if (sw == 2 * dw && sh == 2 * dh) {
    for (int y = 0; y < dh; ++y)
      for (int x = 0; x < dw; ++x) {
        const uint8_t* p = src + (size_t)(2 * y) * sstride + 2 * x;
        dst[(size_t)y * dw + x] = (uint8_t)((p[0] + p[1] + p[sstride] + p[sstride + 1] + 2) >> 2);
      }
    return;
  }
  for (int y = 0; y < dh; ++y) {
    int sy, b0, b1;
    resize_coef(y, sh, dh, &sy, &b0, &b1, 0);
    int y0 = sy, y1 = sy + 1;
    y0 = y0 >= 0 ? (y0 < sh ? y0 : sh - 1) : 0;
    y1 = y1 >= 0 ? (y1 < sh ? y1 : sh - 1) : 0;
    for (int x = 0; x < dw; ++x) {
      int sx, a0, a1;
      resize_coef(x, sw, dw, &sx, &a0, &a1, 1);
      const int x1 = sx + 1 < sw ? sx + 1 : sx;            /* dx >= xmax: only S[sx] (its weight is 2048, the other 0) */
      const int S0 = src[(size_t)y0 * sstride + sx] * a0 + src[(size_t)y0 * sstride + x1] * a1;
      const int S1 = src[(size_t)y1 * sstride + sx] * a0 + src[(size_t)y1 * sstride + x1] * a1;
      dst[(size_t)y * dw + x] = (uint8_t)((((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2);
    }
  }
}
