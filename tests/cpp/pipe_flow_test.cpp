// The flow landmarks of the stereo pipe (d2fe_pipe_flow_enable) through the C++ mirror (include/d2fe.hpp): StereoPipe::flowEnable and StereoFrameResult::flow.  The
// SAME stereo frame is submitted three times, so the chain is known without a second implementation: frame 0 tracks nothing and detects its list with FAST (src = -1,
// ids 0 .. n - 1, no entry nearer than feature_min_dist to a SuperPoint keypoint of the frame or to another entry); every later frame tracks that list onto an
// identical image, where the tracker's first iteration already stands still -- every entry that is tracked at all keeps its position bit for bit and its id; and for
// every entry the right track is the bits of d2fe_lk_track(left, right, pts, pts, WHOLE_IMG_MATCH).  The refusals of the mode do not end a pipe.
// Usage: pipe_flow_test <in.bin>   (the input file of mirror_test: H, W, max keypoints, the 12 SuperPoint layers, two gray frames).  Exit code 0 = all equal.
#include <cmath>
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

  d2fe_flow_params fp;
  d2fe_flow_default_params(&fp);
  if (fp.struct_size != (int32_t)sizeof(fp) || fp.superpoint != 1 || fp.track.total_feature_num != 150 || fp.track.levels != 2 || fp.track.win != 21 || fp.track.iters != 30 ||
      fp.track.near_lk_thread_rate != 5.0f || fp.track.feature_min_dist != 20.0 || fp.fast_cols != 3 || fp.fast_rows != 4 || fp.fast_threshold != 10) return 6;
  d2fe_pipe_config pc;
  d2fe_pipe_default_config(&pc);
  pc.lanes = 2; pc.width = W; pc.height = H; pc.cap = maxkp; pc.netvlad = 0; pc.match_lr = 0; pc.match_prev = 1; pc.ratio = 0.8;
  {
    StereoPipe plain(sp.handle(), pc);          // no pyramids: refused, and the pipe works on
    if (!plain.ok() || plain.flowEnable()) return 6;
    d2fe_pipe_flow_result none;
    const int64_t t = plain.submit(ImageView(img0.data(), H, W), ImageView(img1.data(), H, W));
    StereoFrameResult r;
    if (t < 0 || !plain.wait(t, r) || r.kps_left.size() != k0.size() || !r.flow.pts.empty()) return 6;
    if (d2fe_pipe_flow_result_get(plain.get(), t, &none) != D2FE_ERR_UNSUPPORTED) return 6;
  }
  pc.lr_lk = 1;
  StereoPipe pipe(sp.handle(), pc);
  if (!pipe.ok()) return 6;
  fp.superpoint = 0;
  if (pipe.flowEnable(&fp)) return 6;            // superpoint = 0 beside match_prev
  fp.superpoint = 1; fp.track.total_feature_num = 1024;
  if (pipe.flowEnable(&fp)) return 6;            // cap_tracks beyond 1024
  fp.track.total_feature_num = 60;
  if (!pipe.flowEnable(&fp)) return 6;
  int64_t t[3];
  for (int i = 0; i < 3; ++i) { t[i] = pipe.submit(ImageView(img0.data(), H, W), ImageView(img1.data(), H, W)); if (t[i] < 0) return 6; }
  if (pipe.flowEnable(&fp)) return 6;            // after a submit
  d2fe_lk_frame fl = nullptr, fr = nullptr;
  if (d2fe_lk_frame_create(sp.handle(), img0.data(), W, H, W, 2, &fl) != D2FE_OK || d2fe_lk_frame_create(sp.handle(), img1.data(), W, H, W, 2, &fr) != D2FE_OK) return 5;
  auto dist = [](const Point2f& a, const Point2f& b) { const float dx = a.x - b.x, dy = a.y - b.y; return std::sqrt((double)dx * dx + (double)dy * dy); };
  StereoFlowList prev;
  int right_ok = 0, next_id = 0;
  for (int i = 0; i < 3; ++i) {
    StereoFrameResult r;
    if (!pipe.wait(t[i], r)) return 7;
    if (r.kps_left.size() != k0.size() || std::memcmp(r.kps_left.data(), k0.data(), sizeof(Point2f) * k0.size()) || std::memcmp(r.desc_left.data(), d0.data(), d0.size() * 4)) return 7;
    if (r.lk_right.size() != k0.size() || !r.tracks.pts.empty()) return 8;      // the per-keypoint tracks of lr_lk stay
    const StereoFlowList& f = r.flow;
    const int n = (int)f.pts.size();
    if (n < 1 || n > 60 || (int)f.id.size() != n || (int)f.src.size() != n || (int)f.right.size() != n || (int)f.right_status.size() != n || !f.depth_mm.empty()) return 9;
    if (f.n_new + (f.n_tracked_in - f.n_lost - f.n_removed_near) != n || f.n_tracked_in != (int)prev.pts.size()) return 9;
    if (f.lack != 60 - (int)k0.size() - (n - f.n_new)) return 9;
    if ((f.num > 0) != (f.lack > 15) || (f.num > 0 && f.num != 2 * f.lack) || f.n_cand > f.num || f.n_new > (f.lack > 0 ? f.lack : 0)) return 10;
    for (int j = 0; j < n; ++j) {
      const int s = f.src[j];
      if (s < 0) {                              // detected in this frame: the next ids in order, clear of the keypoints and of every earlier entry
        if (j < n - f.n_new || f.id[j] != next_id++) return 11;
        for (const Point2f& k : k0) if (dist(f.pts[j], k) < 20.0) return 12;
        for (int e = 0; e < j; ++e) if (dist(f.pts[j], f.pts[e]) < 20.0) return 12;
      } else {                                  // identical images: a tracked entry stands still and keeps its id
        if (s >= (int)prev.pts.size() || f.id[j] != prev.id[s] || std::memcmp(&f.pts[j], &prev.pts[s], sizeof(Point2f))) return 13;
      }
    }
    if (i == 0 && (f.n_tracked_in != 0 || f.n_new != n)) return 10;
    std::vector<float> ref((size_t)2 * n);
    std::vector<uint8_t> rst(n);
    if (d2fe_lk_track(sp.handle(), fl, fr, &f.pts[0].x, &f.pts[0].x, n, 0, 0.f, 21, 30, ref.data(), rst.data()) != D2FE_OK) return 5;
    if (std::memcmp(&f.right[0].x, ref.data(), sizeof(float) * 2 * n) || std::memcmp(f.right_status.data(), rst.data(), n)) return 14;
    right_ok = 0;
    for (uint8_t s : rst) right_ok += s;
    std::printf("frame %d: %d flow entries (%d tracked in, %d lost, %d near, %d new; lack %d, num %d, %d candidates), %d tracked into the right image\n", i, n, f.n_tracked_in,
                f.n_lost, f.n_removed_near, f.n_new, f.lack, f.num, f.n_cand, right_ok);
    prev = f;
  }
  d2fe_lk_frame_destroy(fl); d2fe_lk_frame_destroy(fr);
  return right_ok > 0 ? 0 : 15;
}
