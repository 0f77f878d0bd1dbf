// The int8 calibration session through the C++ mirror (include/d2fe.hpp: Int8Calibrator over d2fe_calib_*): an exact-precision SuperPoint with the dense head,
// two passes over the frames, the twelve ranges by the three rules -- then an int8_operands SuperPoint takes the entropy ranges and extracts.  From frames to a
// working D2FE_PREC_I8 handle with libd2fe_hip.so alone.  Dumps the ranges for tests/test_cpp_calib.py.  Usage: calib_test <in.bin> <out.bin>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "d2fe.hpp"

using namespace D2FrontEnd;

template <typename T>
static bool rd(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* fi = fopen(argv[1], "rb");
  if (!fi) return 2;
  int32_t H, W, n_img, n_bins;
  if (!rd(fi, &H, 1) || !rd(fi, &W, 1) || !rd(fi, &n_img, 1) || !rd(fi, &n_bins, 1)) return 2;
  std::vector<std::vector<float>> ws(D2FE_SP_NUM_LAYERS), bs(D2FE_SP_NUM_LAYERS);
  d2fe_superpoint_weights w;
  for (int l = 0; l < D2FE_SP_NUM_LAYERS; ++l) {
    int32_t dims[3];
    if (!rd(fi, dims, 3)) return 2;
    ws[l].resize((size_t)dims[0] * dims[1] * dims[2] * dims[2]); bs[l].resize(dims[0]);
    if (!rd(fi, ws[l].data(), ws[l].size()) || !rd(fi, bs[l].data(), bs[l].size())) return 2;
    w.layer[l].weight = ws[l].data(); w.layer[l].bias = bs[l].data();
    w.layer[l].cout = dims[0]; w.layer[l].cin = dims[1]; w.layer[l].ksize = dims[2];
  }
  std::vector<uint8_t> imgs((size_t)H * W * n_img);
  if (!rd(fi, imgs.data(), imgs.size())) return 2;
  fclose(fi);

  float r_minmax[D2FE_SP_NUM_LAYERS], r_early[D2FE_SP_NUM_LAYERS], r_entropy[D2FE_SP_NUM_LAYERS], r_pct[D2FE_SP_NUM_LAYERS];
  {
    SuperPointConfig cfg;
    cfg.input_width = W; cfg.input_height = H; cfg.max_batch = 2;
    {
      SuperPoint sparse(cfg);      // without the dense head: refused
      if (!sparse.build(w)) return 3;
      Int8Calibrator no(sparse);
      if (no.ok()) return 4;
    }
    cfg.dense_descriptors = true;
    SuperPoint sp(cfg);
    if (!sp.build(w)) return 3;
    Int8Calibrator cal(sp, n_bins);
    if (!cal.ok()) return 4;
    if (cal.freeze()) return 5;      // no image yet
    if (!cal.collect(ImageView(imgs.data(), H, W), n_img)) return 6;      // n_img > max_batch: sliced
    if (cal.ranges(D2FE_CALIB_ENTROPY, r_entropy)) return 5;      // needs the histogram phase
    if (!cal.ranges(D2FE_CALIB_MINMAX, r_early)) return 7;
    if (!cal.freeze()) return 6;
    for (int i = 0; i < n_img; ++i)
      if (!cal.collect(ImageView(imgs.data() + (size_t)i * H * W, H, W))) return 6;
    if (!cal.ranges(D2FE_CALIB_MINMAX, r_minmax) || !cal.ranges(D2FE_CALIB_ENTROPY, r_entropy) || !cal.ranges(D2FE_CALIB_PERCENTILE, r_pct, 99.9)) return 7;
    if (memcmp(r_early, r_minmax, sizeof(r_minmax))) return 8;
    float t_max;
    uint64_t nz, nov, ntot, sum = 0;
    std::vector<uint64_t> hist;
    if (!cal.stats(0, t_max, nz, nov, ntot, &hist)) return 9;
    for (uint64_t v : hist) sum += v;
    if (t_max != r_minmax[0] || nov != 0 || sum + nz != ntot || ntot != (uint64_t)n_img * H * W * 64) return 9;
  }
  SuperPointConfig q;
  q.input_width = W; q.input_height = H; q.max_batch = 1; q.int8_operands = true;
  SuperPoint sp8(q);
  if (!sp8.build(w) || !sp8.setInt8Ranges(r_entropy)) return 10;
  std::vector<Point2f> k;
  std::vector<float> d, s;
  if (!sp8.infer(ImageView(imgs.data(), H, W), k, d, s) || k.empty()) return 11;

  FILE* fo = fopen(argv[2], "wb");
  if (!fo) return 2;
  fwrite(r_minmax, sizeof(float), D2FE_SP_NUM_LAYERS, fo);
  fwrite(r_entropy, sizeof(float), D2FE_SP_NUM_LAYERS, fo);
  fwrite(r_pct, sizeof(float), D2FE_SP_NUM_LAYERS, fo);
  fclose(fo);
  return 0;
}
