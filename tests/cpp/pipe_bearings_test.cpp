// The bearings of the stereo pipe through the C++ mirror (include/d2fe.hpp): StereoPipe::bearingsEnable on an lr_lk + sp_lk pipe, StereoFrameResult::bearings against the
// host restatements of the same header (liftProjectivePinhole, unitBearing, predictWithExtrinsic, spaceToPlanePinhole) on the returned points.  This program checks the
// sizes, the refusals and the gate (exactly: on the device's own predictions); the bearings and predictions of both sides go to the output file, where
// tests/test_cpp_pipe_bearings.py holds them to the derived bound (the device's sqrt and divide need not return the host's last bit).
// Usage: pipe_bearings_test <in.bin> <out.bin>   in: the input file of mirror_test (H, W, max keypoints, the 12 SuperPoint layers, two gray frames) followed by 8 + 8
// doubles (the left and right pinhole cameras: fx fy cx cy k1 k2 p1 p2), T_right_left [12], distance, radius_lk.  Exit code 0 = all checks passed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "d2fe.hpp"

using namespace D2FrontEnd;

template <typename T>
static bool rd(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }
template <typename T>
static void wr(FILE* f, const std::vector<T>& v) { int32_t m = (int32_t)v.size(); fwrite(&m, 4, 1, f); if (m) fwrite(v.data(), sizeof(T), v.size(), f); }

static d2fe_camera camera_of(const double* p) {
  d2fe_camera c;
  std::memset(&c, 0, sizeof(c));
  c.kind = D2FE_CAM_PINHOLE;
  for (int i = 0; i < 8; ++i) c.p[i] = p[i];
  return c;
}
static RadTan radtan_of(const double* p) { RadTan d; d.k1 = p[4]; d.k2 = p[5]; d.p1 = p[6]; d.p2 = p[7]; return d; }

// the host restatement: unit bearings [n][3] and, with T, the predictions
static void host_side(const double* cam, const double* T, double distance, const std::vector<Point2f>& pts, std::vector<double>& b, std::vector<float>* pred) {
  b.clear();
  if (pred) pred->clear();
  for (const Point2f& p : pts) {
    const Vec3d u = unitBearing(liftProjectivePinhole(cam[0], cam[1], cam[2], cam[3], radtan_of(cam), p));
    b.push_back(u.x); b.push_back(u.y); b.push_back(u.z);
    if (pred) {
      double pu, pv;
      spaceToPlanePinhole(cam[0], cam[1], cam[2], cam[3], radtan_of(cam), predictWithExtrinsic(T, u, distance), pu, pv);
      pred->push_back((float)pu); pred->push_back((float)pv);
    }
  }
}
static std::vector<float> flat(const std::vector<Point2f>& v) { std::vector<float> o; for (const Point2f& p : v) { o.push_back(p.x); o.push_back(p.y); } return o; }

int main(int argc, char** argv) {
  if (argc != 3) return 2;
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
  std::vector<uint8_t> img[2] = {std::vector<uint8_t>((size_t)H * W), std::vector<uint8_t>((size_t)H * W)};
  double camL[8], camR[8], T[12], distance, radius;
  if (!rd(fi, img[0].data(), img[0].size()) || !rd(fi, img[1].data(), img[1].size()) || !rd(fi, camL, 8) || !rd(fi, camR, 8) || !rd(fi, T, 12) || !rd(fi, &distance, 1) ||
      !rd(fi, &radius, 1)) return 2;
  fclose(fi);

  SuperPointConfig cfg;
  cfg.max_keypoints = maxkp; cfg.input_width = W; cfg.input_height = H;
  SuperPoint sp(cfg);
  if (!sp.build(w)) return 3;

  d2fe_pipe_config pc;
  d2fe_pipe_default_config(&pc);
  pc.lanes = 2; pc.width = W; pc.height = H; pc.cap = maxkp; pc.netvlad = 0; pc.match_lr = 0; pc.match_prev = 1; pc.lr_lk = 1; pc.sp_lk = 1;
  d2fe_track_params tp;
  d2fe_track_default_params(&tp);
  tp.total_feature_num = 60;
  StereoPipe pipe(sp.handle(), pc, &tp);
  if (!pipe.ok()) return 4;
  d2fe_pipe_bearings bp;
  d2fe_pipe_bearings_default(&bp);
  if (bp.struct_size != (int32_t)sizeof(bp) || bp.lk_use_pred != 1 || bp.distance != 100.0 || bp.T_right_left[0] != 1.0 || bp.T_right_left[3] != 0.0) return 5;
  bp.cam[0] = camera_of(camL); bp.cam[1] = camera_of(camR);
  for (int i = 0; i < 12; ++i) bp.T_right_left[i] = T[i];
  bp.distance = distance; bp.radius_lk = radius;
  {
    d2fe_pipe_bearings bad = bp;
    bad.cam[1].kind = 5;
    if (pipe.bearingsEnable(bad)) return 5;              // refused ...
    bad = bp; bad.cam[0].p[0] = 0.0;
    if (pipe.bearingsEnable(bad)) return 5;
  }
  if (!pipe.bearingsEnable(bp)) return 5;                // ... and the pipe is as it was
  if (pipe.bearingsEnable(bp)) return 5;                 // twice
  FILE* fo = fopen(argv[2], "wb");
  if (!fo) return 2;
  int rc = 0;
  int64_t tk[3];
  for (int i = 0; i < 3 && !rc; ++i) {
    tk[i] = pipe.submit(ImageView(img[i & 1].data(), H, W), ImageView(img[(i & 1) ^ 1].data(), H, W));
    if (tk[i] < 0) rc = 6;
  }
  for (int i = 0; i < 3 && !rc; ++i) {
    StereoFrameResult r;
    d2fe_pipe_bearings_result br;
    if (d2fe_pipe_bearings_result_get(pipe.get(), tk[i], &br) != D2FE_ERR_NOT_READY) { rc = 7; break; }
    if (!pipe.wait(tk[i], r)) { rc = 7; break; }
    const StereoBearings& b = r.bearings;
    const size_t n = r.kps_left.size(), m = r.tracks.pts.size();
    if (n == 0 || m == 0 || r.tracks.right.size() != m || r.tracks.right_status.size() != m) { rc = 8; break; }
    if (b.kp_left.size() != 3 * n || !b.kp_right.empty() || b.kp_pred.size() != n || !b.lk_right.empty() || !b.lk_pred_ok.empty()) { rc = 9; break; }
    if (b.list.size() != 3 * m || b.list_pred.size() != m || b.list_right.size() != 3 * m || b.list_pred_ok.size() != m) { rc = 9; break; }
    // the gate, exactly, on the device's own predictions: status && cv::norm(pred - right) < radius
    size_t kept = 0;
    for (size_t j = 0; j < m; ++j) {
      const float dx = b.list_pred[j].x - r.tracks.right[j].x, dy = b.list_pred[j].y - r.tracks.right[j].y;
      const bool ok = r.tracks.right_status[j] && (radius <= 0 || std::sqrt((double)dx * dx + (double)dy * dy) < radius);
      if ((b.list_pred_ok[j] != 0) != ok) rc = 10;
      kept += ok;
    }
    std::vector<double> hb;
    std::vector<float> hp;
    host_side(camL, T, distance, r.kps_left, hb, &hp);
    wr(fo, flat(r.kps_left)); wr(fo, b.kp_left); wr(fo, hb); wr(fo, flat(b.kp_pred)); wr(fo, hp);
    host_side(camL, T, distance, r.tracks.pts, hb, &hp);
    wr(fo, flat(r.tracks.pts)); wr(fo, b.list); wr(fo, hb); wr(fo, flat(b.list_pred)); wr(fo, hp);
    host_side(camR, T, distance, r.tracks.right, hb, nullptr);
    wr(fo, flat(r.tracks.right)); wr(fo, b.list_right); wr(fo, hb);
    std::printf("frame %d: %zu keypoints, %zu list entries, the gate keeps %zu\n", i, n, m, kept);
  }
  fclose(fo);
  return rc;
}
