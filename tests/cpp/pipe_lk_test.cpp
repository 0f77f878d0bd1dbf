// The stereo pipe's lr_lk mode (lr_match_use_lk, the reference's default stereo path) through the C++ mirror (include/d2fe.hpp): StereoPipe with cfg.lr_lk = 1 must
// deliver infer()'s left keypoints and, for every one of them, the track of d2fe_lk_track(left, right, pts, pts, WHOLE_IMG_MATCH) -- bit for bit.
// Usage: pipe_lk_test <in.bin>   (the input file of mirror_test: H, W, max keypoints, the 12 SuperPoint layers, two gray frames).  Exit code 0 = all equal.
#include <cstdio>
#include <cstring>
#include <vector>

#include "d2fe.hpp"

using namespace D2FrontEnd;

template <typename T>
static bool rd(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* fi = fopen(argv[1], "rb");
  if (!fi) return 2;
  int32_t H, W, maxkp;
  if (!rd(fi, &H, 1) || !rd(fi, &W, 1) || !rd(fi, &maxkp, 1)) return 2;
  std::vector<std::vector<float>> ws(12), bs(12);
  d2fe_superpoint_weights w;
  for (int l = 0; l < 12; ++l) {
    int32_t dims[3];
    if (!rd(fi, dims, 3)) return 2;
    ws[l].resize((size_t)dims[0] * dims[1] * dims[2] * dims[2]); bs[l].resize(dims[0]);
    if (!rd(fi, ws[l].data(), ws[l].size()) || !rd(fi, bs[l].data(), bs[l].size())) return 2;
    w.layer[l].weight = ws[l].data(); w.layer[l].bias = bs[l].data();
    w.layer[l].cout = dims[0]; w.layer[l].cin = dims[1]; w.layer[l].ksize = dims[2];
  }
  std::vector<uint8_t> img0((size_t)H * W), img1((size_t)H * W);
  if (!rd(fi, img0.data(), img0.size()) || !rd(fi, img1.data(), img1.size())) return 2;
  fclose(fi);

  SuperPointConfig cfg;
  cfg.max_keypoints = maxkp; cfg.input_width = W; cfg.input_height = H;
  SuperPoint sp(cfg);
  if (!sp.build(w)) return 3;
  std::vector<Point2f> k0;
  std::vector<float> d0, s0;
  if (!sp.infer(ImageView(img0.data(), H, W), k0, d0, s0) || k0.empty()) return 4;
  // the existing tracker calls on the same keypoints
  const int n = (int)k0.size();
  d2fe_lk_frame fl = nullptr, fr = nullptr;
  if (d2fe_lk_frame_create(sp.handle(), img0.data(), W, H, W, 2, &fl) != D2FE_OK || d2fe_lk_frame_create(sp.handle(), img1.data(), W, H, W, 2, &fr) != D2FE_OK) return 5;
  std::vector<float> pts((size_t)2 * n), ref((size_t)2 * n);
  std::vector<uint8_t> rst(n);
  for (int i = 0; i < n; ++i) { pts[2 * i] = k0[i].x; pts[2 * i + 1] = k0[i].y; }
  if (d2fe_lk_track(sp.handle(), fl, fr, pts.data(), pts.data(), n, 0, 0.f, 21, 30, ref.data(), rst.data()) != D2FE_OK) return 5;
  d2fe_lk_frame_destroy(fl); d2fe_lk_frame_destroy(fr);

  d2fe_pipe_config pc;
  d2fe_pipe_default_config(&pc);
  if (pc.lr_lk != 0) return 6;
  pc.lanes = 2; pc.width = W; pc.height = H; pc.cap = maxkp; pc.netvlad = 0; pc.match_prev = 1; pc.ratio = 0.8;
  pc.lr_lk = 1;
  {
    StereoPipe refused(sp.handle(), pc);        // match_lr is still 1
    if (refused.ok()) return 6;
  }
  pc.match_lr = 0;
  StereoPipe pipe(sp.handle(), pc);
  if (!pipe.ok()) return 6;
  int64_t t[3];
  for (int i = 0; i < 3; ++i) { t[i] = pipe.submit(ImageView(img0.data(), H, W), ImageView(img1.data(), H, W)); if (t[i] < 0) return 6; }
  int tracked = 0;
  for (int i = 0; i < 3; ++i) {
    StereoFrameResult r;
    if (!pipe.wait(t[i], r)) return 7;
    if ((int)r.kps_left.size() != n || std::memcmp(r.kps_left.data(), k0.data(), sizeof(Point2f) * n) || std::memcmp(r.desc_left.data(), d0.data(), d0.size() * 4)) return 7;
    if (!r.kps_right.empty() || !r.desc_right.empty() || !r.left_right.empty()) return 8;
    if ((int)r.lk_right.size() != n || (int)r.lk_status.size() != n) return 9;
    if (std::memcmp(r.lk_right.data(), ref.data(), sizeof(float) * 2 * n) || std::memcmp(r.lk_status.data(), rst.data(), n)) return 9;
    if ((i == 0) != r.left_prev.empty()) return 10;      // the same frame again: every later one matches its predecessor
    tracked = 0;
    for (uint8_t s : r.lk_status) tracked += s;
  }
  std::printf("%d keypoints, %d tracked\n", n, tracked);
  return tracked > 0 ? 0 : 11;
}
