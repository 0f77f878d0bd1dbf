// D2FE_PREC_I8 through the C++ mirror (include/d2fe.hpp): SuperPointConfig::int8_operands, build, infer refused until setInt8Ranges, two infer calls that
// must agree.  Dumps the first call's outputs for tests/test_cpp_i8_mode.py.  Usage: i8_mode_test <in.bin> <out.bin>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "d2fe.hpp"

using namespace D2FrontEnd;

template <typename T>
static bool rd(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }
template <typename T>
static void wr(FILE* f, const std::vector<T>& v) {
  const int32_t n = (int32_t)v.size();
  fwrite(&n, 4, 1, f);
  if (n) fwrite(v.data(), sizeof(T), v.size(), f);
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* fi = fopen(argv[1], "rb");
  if (!fi) return 2;
  int32_t H, W, maxkp;
  if (!rd(fi, &H, 1) || !rd(fi, &W, 1) || !rd(fi, &maxkp, 1)) return 2;
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
  float ranges[D2FE_SP_NUM_LAYERS];
  std::vector<uint8_t> img((size_t)H * W);
  if (!rd(fi, ranges, D2FE_SP_NUM_LAYERS) || !rd(fi, img.data(), img.size())) return 2;
  fclose(fi);

  SuperPointConfig cfg;
  cfg.max_keypoints = maxkp; cfg.input_width = W; cfg.input_height = H; cfg.max_batch = 1;
  cfg.int8_operands = true;
  SuperPoint sp(cfg);
  if (!sp.build(w)) return 3;
  std::vector<Point2f> k0, k1;
  std::vector<float> d0, d1, s0, s1;
  if (sp.infer(ImageView(img.data(), H, W), k0, d0, s0)) return 4;      // no ranges yet: D2FE_ERR_NOT_READY, reported as false
  if (!k0.empty() || !d0.empty() || !s0.empty()) return 4;
  float bad[D2FE_SP_NUM_LAYERS];
  memcpy(bad, ranges, sizeof(bad));
  bad[3] = 0.f;
  if (sp.setInt8Ranges(bad)) return 5;
  if (!sp.setInt8Ranges(ranges)) return 6;
  if (!sp.infer(ImageView(img.data(), H, W), k0, d0, s0)) return 7;
  if (!sp.infer(ImageView(img.data(), H, W), k1, d1, s1)) return 7;
  if (k0.size() != k1.size() || k0.empty() || d0.size() != 256 * k0.size()) return 8;
  for (size_t i = 0; i < k0.size(); ++i)
    if (k0[i].x != k1[i].x || k0[i].y != k1[i].y) return 8;
  if (memcmp(d0.data(), d1.data(), d0.size() * sizeof(float)) || memcmp(s0.data(), s1.data(), s0.size() * sizeof(float))) return 8;
  FILE* fo = fopen(argv[2], "wb");
  if (!fo) return 2;
  std::vector<float> kf;
  for (auto& q : k0) { kf.push_back(q.x); kf.push_back(q.y); }
  wr(fo, kf); wr(fo, s0); wr(fo, d0);
  fclose(fo);
  return 0;
}
