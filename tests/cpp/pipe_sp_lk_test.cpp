// The stereo pipe's sp_lk mode (sp_track_use_lk + lr_match_use_lk, the reference's default stereo tracker) through the C++ mirror (include/d2fe.hpp): StereoPipe
// with cfg.lr_lk = cfg.sp_lk = 1 must deliver infer()'s left keypoints and StereoFrameResult::tracks, the LK-carried landmark list.  The SAME stereo frame is
// submitted three times, so the chain is known without a second implementation: frame 0 discovers its list from the SuperPoint keypoints (src = -1, kp ascending,
// ids 0 .. n - 1, the keypoints' own descriptor rows); every later frame tracks that list onto an identical image, where the tracker's first iteration already
// stands still -- every entry that is tracked at all keeps its position bit for bit, its id and the descriptor of frame 0; and for every entry the right track is
// the bits of d2fe_lk_track(left, right, pts, pts, WHOLE_IMG_MATCH).
// Usage: pipe_sp_lk_test <in.bin>   (the input file of mirror_test: H, W, max keypoints, the 12 SuperPoint layers, two gray frames).  Exit code 0 = all equal.
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
  const size_t D = d0.size() / k0.size();

  d2fe_pipe_config pc;
  d2fe_pipe_default_config(&pc);
  if (pc.sp_lk != 0 || sizeof(pc) != 96) return 6;
  pc.lanes = 2; pc.width = W; pc.height = H; pc.cap = maxkp; pc.netvlad = 0; pc.match_lr = 0; pc.match_prev = 1; pc.ratio = 0.8;
  pc.sp_lk = 1;
  {
    StereoPipe refused(sp.handle(), pc);        // lr_lk is still 0
    if (refused.ok()) return 6;
  }
  pc.lr_lk = 1;
  d2fe_track_params tp;
  d2fe_track_default_params(&tp);
  if (tp.total_feature_num != 150 || tp.levels != 2 || tp.win != 21 || tp.iters != 30 || tp.near_lk_thread_rate != 5.0f || tp.feature_min_dist != 20.0) return 6;
  tp.total_feature_num = 1024;
  {
    StereoPipe refused(sp.handle(), pc, &tp);   // cap_tracks = 1025
    if (refused.ok()) return 6;
  }
  tp.total_feature_num = 60;
  StereoPipe pipe(sp.handle(), pc, &tp);
  if (!pipe.ok()) return 6;
  int64_t t[3];
  for (int i = 0; i < 3; ++i) { t[i] = pipe.submit(ImageView(img0.data(), H, W), ImageView(img1.data(), H, W)); if (t[i] < 0) return 6; }
  d2fe_lk_frame fl = nullptr, fr = nullptr;
  if (d2fe_lk_frame_create(sp.handle(), img0.data(), W, H, W, 2, &fl) != D2FE_OK || d2fe_lk_frame_create(sp.handle(), img1.data(), W, H, W, 2, &fr) != D2FE_OK) return 5;
  StereoTrackList first, prev;
  int right_ok = 0;
  for (int i = 0; i < 3; ++i) {
    StereoFrameResult r;
    if (!pipe.wait(t[i], r)) return 7;
    if (r.kps_left.size() != k0.size() || std::memcmp(r.kps_left.data(), k0.data(), sizeof(Point2f) * k0.size()) || std::memcmp(r.desc_left.data(), d0.data(), d0.size() * 4)) return 7;
    if (!r.lk_right.empty() || !r.lk_status.empty() || !r.kps_right.empty()) return 8;
    const StereoTrackList& tr = r.tracks;
    const int n = (int)tr.pts.size();
    if (n < 1 || n > 61 || (int)tr.id.size() != n || (int)tr.right.size() != n || tr.desc.size() != (size_t)n * D) return 9;
    if (tr.n_new + (tr.n_tracked_in - tr.n_lost - tr.n_removed_near) != n) return 9;
    if (i == 0) {
      if (tr.n_tracked_in != 0 || tr.n_new != n) return 10;
      for (int j = 0; j < n; ++j) {
        const int kp = tr.kp[j];
        if (tr.id[j] != j || tr.src[j] != -1 || kp < 0 || kp >= (int)k0.size() || (j > 0 && kp <= tr.kp[j - 1])) return 10;
        if (std::memcmp(&tr.pts[j], &k0[kp], sizeof(Point2f)) || tr.scores[j] != s0[kp] || std::memcmp(&tr.desc[(size_t)j * D], &d0[(size_t)kp * D], D * 4)) return 10;
      }
      first = tr;
    } else {
      if (tr.n_tracked_in != (int)prev.pts.size()) return 11;
      for (int j = 0; j < n; ++j) {
        const int s = tr.src[j];
        if (s < 0) { if (tr.kp[j] < 0) return 11; continue; }       // a keypoint that took a lost entry's place
        if (s >= (int)prev.pts.size() || tr.kp[j] != -1 || tr.id[j] != prev.id[s]) return 11;
        if (std::memcmp(&tr.pts[j], &prev.pts[s], sizeof(Point2f))) return 12;      // identical images: a tracked entry stands still
        if (std::memcmp(&tr.desc[(size_t)j * D], &prev.desc[(size_t)s * D], D * 4) || tr.scores[j] != prev.scores[s]) return 13;      // carried from the previous list
        const int id = tr.id[j];                                                                                                   // ... i.e. from the discovery frame
        if (id < (int)first.pts.size() && std::memcmp(&tr.desc[(size_t)j * D], &first.desc[(size_t)id * D], D * 4)) return 13;
      }
    }
    std::vector<float> ref((size_t)2 * n);
    std::vector<uint8_t> rst(n);
    if (d2fe_lk_track(sp.handle(), fl, fr, &tr.pts[0].x, &tr.pts[0].x, n, 0, 0.f, 21, 30, ref.data(), rst.data()) != D2FE_OK) return 5;
    if (std::memcmp(&tr.right[0].x, ref.data(), sizeof(float) * 2 * n) || std::memcmp(tr.right_status.data(), rst.data(), n)) return 14;
    right_ok = 0;
    for (uint8_t s : rst) right_ok += s;
    std::printf("frame %d: %d entries (%d tracked in, %d lost, %d near, %d new), %d tracked into the right image\n", i, n, tr.n_tracked_in, tr.n_lost, tr.n_removed_near, tr.n_new, right_ok);
    prev = tr;
  }
  d2fe_lk_frame_destroy(fl); d2fe_lk_frame_destroy(fr);
  return right_ok > 0 ? 0 : 15;
}
