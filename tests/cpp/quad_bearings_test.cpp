// quad_bearings_test.cpp -- the bearings of the quad pipe through the C++ mirror (include/d2fe.hpp): QuadPipe::bearingsEnable on a flow_lk pipe, QuadPipe::bearings
// against the host restatements of the same header (liftProjectiveCylindrical, unitBearing, predictWithExtrinsic, spaceToPlaneCylindrical) on the returned points.
// Plain C++ (g++), only the C ABI behind the header; no Python, no torch, no HIP call of its own.  This program checks the sizes, the refusals and the gate (exactly: on
// the device's own predictions); the bearings and predictions of both sides go to the output file, where tests/test_cpp_quad_bearings.py holds them to the derived bound
// (the device's tan, atan2, sqrt and divide need not return the host's last bits).
//   usage: quad_bearings_test <sp.d2fw> <in.bin> <out.bin>
//   in.bin : int32 n (quad frames: one per submit), H, W (raw frame = view), cap, total_feature_num, 0; double feature_min_dist; double cams[4][4] (fx fy cx cy),
//            T_nb[4][12], distance, radius_lk; float maps[4][2][H][W] (mapx, mapy; no gain); u8 frames[n][4][H][W]
//   out.bin: per quad frame and view c: keypoints, device bearings, host bearings, list points, device bearings, host bearings; then per pair n: device predictions, host
//            predictions, neighbour tracks, device bearings, host bearings -- each as int32 count + data
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "d2fe.hpp"
#include "d2fe_weights_file.hpp"

using namespace D2FrontEnd;

#define CHECK(x) do { int e_ = (x); if (e_ != D2FE_OK) { fprintf(stderr, "%s: %d %s\n", #x, e_, d2fe_last_error()); return 5; } } while (0)

template <typename T>
static void wr(FILE* f, const std::vector<T>& v) { int32_t m = (int32_t)v.size(); fwrite(&m, 4, 1, f); if (m) fwrite(v.data(), sizeof(T), v.size(), f); }
static std::vector<float> flat(const std::vector<Point2f>& v) { std::vector<float> o; for (const Point2f& p : v) { o.push_back(p.x); o.push_back(p.y); } return o; }

// the host restatement: unit bearings [n][3] and, with T, the predictions
static void host_side(const double* cam, const double* T, double distance, const std::vector<Point2f>& pts, std::vector<double>& b, std::vector<float>* pred) {
  b.clear();
  if (pred) pred->clear();
  for (const Point2f& p : pts) {
    const Vec3d u = unitBearing(liftProjectiveCylindrical(cam[0], cam[1], cam[2], cam[3], p));
    b.push_back(u.x); b.push_back(u.y); b.push_back(u.z);
    if (pred) {
      double pu, pv;
      spaceToPlaneCylindrical(cam[0], cam[1], cam[2], cam[3], predictWithExtrinsic(T, u, distance), pu, pv);
      pred->push_back((float)pu); pred->push_back((float)pv);
    }
  }
}

static int run(d2fe_handle h, const char* out_path, int n, int H, int W, int cap, const d2fe_flow_params& fp, const double (*cams)[4], const double (*T_nb)[12],
               double distance, double radius, const std::vector<float>& maps, const std::vector<uint8_t>& frames) {
  static const int view_a[4] = {0, 1, 2, 0}, view_b[4] = {1, 2, 3, 3};
  d2fe_quad_pipe_config pc;
  d2fe_quad_pipe_default_config(&pc);
  pc.lanes = 2; pc.quads = 1; pc.raw_width = W; pc.raw_height = H; pc.width = W; pc.height = H; pc.cap = cap; pc.radius_neighbour = 0.2 * W;
  pc.netvlad = 0; pc.match_neighbour = 1; pc.match_prev = 0;
  d2fe_quad_maps qm{};
  const size_t npix = (size_t)H * W;
  for (int c = 0; c < 4; ++c) { qm.mapx[c] = &maps[(2 * c) * npix]; qm.mapy[c] = &maps[(2 * c + 1) * npix]; qm.gain[c] = nullptr; }
  QuadPipe pipe(h, pc, qm);
  if (!pipe.ok()) return 4;
  d2fe_quad_bearings bp;
  d2fe_quad_bearings_default(&bp);
  if (bp.struct_size != (int32_t)sizeof(bp) || bp.lk_use_pred != 1 || bp.distance != 100.0 || bp.T_nb[3][0] != 1.0 || bp.T_nb[3][3] != 0.0 || bp.T_nb[2][10] != 1.0) return 5;
  for (int c = 0; c < 4; ++c) {
    bp.cam[c].kind = D2FE_CAM_CYLINDRICAL;
    for (int i = 0; i < 4; ++i) bp.cam[c].p[i] = cams[c][i];
    for (int i = 0; i < 12; ++i) bp.T_nb[c][i] = T_nb[c][i];
  }
  bp.distance = distance; bp.radius_lk = radius;
  {
    d2fe_quad_bearings bad = bp;
    bad.cam[3].kind = 2;
    if (pipe.bearingsEnable(bad)) return 5;              // refused ...
    bad = bp; bad.cam[1].p[0] = 0.0;
    if (pipe.bearingsEnable(bad)) return 5;
    bad = bp; bad.cam[2].p[4] = 1e-3;
    if (pipe.bearingsEnable(bad)) return 5;
    bad = bp; bad.T_nb[1][5] = NAN;
    if (pipe.bearingsEnable(bad)) return 5;
    bad = bp; bad.struct_size += 8;
    if (pipe.bearingsEnable(bad)) return 5;
  }
  if (!pipe.bearingsEnable(bp)) return 5;                // ... and the pipe is as it was; the list mode comes AFTER the bearings here
  if (pipe.bearingsEnable(bp)) return 5;                 // twice
  if (!pipe.flowEnable(&fp)) return 5;
  FILE* fo = fopen(out_path, "wb");
  if (!fo) return 2;
  std::vector<int64_t> tk(n);
  for (int i = 0; i < n; ++i) CHECK(d2fe_quad_pipe_submit(pipe.get(), frames.data() + (size_t)i * 4 * npix, W, npix, 4 * npix, &tk[i]));
  int rc = 0;
  size_t tracked = 0, kept = 0;
  for (int i = 0; i < n && !rc; ++i) {
    d2fe_quad_bearings_result br;
    if (d2fe_quad_bearings_result_get(pipe.get(), tk[i], &br) != D2FE_ERR_NOT_READY) { rc = 7; break; }
    d2fe_quad_pipe_result r;
    CHECK(d2fe_quad_pipe_wait(pipe.get(), tk[i], &r));
    d2fe_quad_flow_result fr;
    CHECK(d2fe_quad_flow_result_get(pipe.get(), tk[i], &fr));
    std::vector<QuadFlowList> lists;
    std::vector<QuadFlowNeighbourTracks> nb;
    std::vector<QuadViewBearings> views;
    std::vector<QuadNeighbourBearings> pairs;
    if (!pipe.flow(tk[i], lists, nb) || !pipe.bearings(tk[i], r.n_kp, fr.n, (size_t)fr.list_words, views, pairs)) { rc = 8; break; }
    if (views.size() != 4 || pairs.size() != 4 || lists.size() != 4) { rc = 9; break; }
    std::vector<double> hb;
    std::vector<float> hp;
    for (int c = 0; c < 4; ++c) {
      std::vector<Point2f> kps;
      for (int j = 0; j < r.n_kp[c]; ++j) kps.emplace_back(r.kps_xy[((size_t)c * r.cap + j) * 2], r.kps_xy[((size_t)c * r.cap + j) * 2 + 1]);
      if (views[c].kp.size() != 3 * kps.size() || views[c].list.size() != 3 * lists[c].pts.size()) { rc = 9; break; }
      host_side(cams[c], nullptr, 0.0, kps, hb, nullptr);
      wr(fo, flat(kps)); wr(fo, views[c].kp); wr(fo, hb);
      host_side(cams[c], nullptr, 0.0, lists[c].pts, hb, nullptr);
      wr(fo, flat(lists[c].pts)); wr(fo, views[c].list); wr(fo, hb);
    }
    for (int p = 0; p < 4 && !rc; ++p) {
      const std::vector<Point2f>& src = lists[view_a[p]].pts;
      const QuadNeighbourBearings& q = pairs[p];
      const size_t m = src.size();
      if (q.pred.size() != m || q.nb.size() != 3 * m || q.pred_ok.size() != m || nb[p].lk.size() != m) { rc = 9; break; }
      // the gate, exactly, on the device's own predictions: status && cv::norm(pred - track) < radius
      for (size_t j = 0; j < m; ++j) {
        const float dx = q.pred[j].x - nb[p].lk[j].x, dy = q.pred[j].y - nb[p].lk[j].y;
        const bool ok = nb[p].lk_status[j] && (radius <= 0 || std::sqrt((double)dx * dx + (double)dy * dy) < radius);
        if ((q.pred_ok[j] != 0) != ok) rc = 10;
        tracked += nb[p].lk_status[j] != 0; kept += ok;
      }
      host_side(cams[view_a[p]], T_nb[p], distance, src, hb, &hp);
      wr(fo, flat(q.pred)); wr(fo, hp);
      host_side(cams[view_b[p]], nullptr, 0.0, nb[p].lk, hb, nullptr);
      wr(fo, flat(nb[p].lk)); wr(fo, q.nb); wr(fo, hb);
    }
  }
  fclose(fo);
  std::printf("quad_bearings_test: %d quad frames, the gate keeps %zu of %zu neighbour tracks\n", n, kept, tracked);
  if (!rc && !(kept > 0 && kept < tracked)) rc = 11;
  return rc;
}

int main(int argc, char** argv) {
  if (argc != 4) { fprintf(stderr, "usage: quad_bearings_test <sp.d2fw> <in.bin> <out.bin>\n"); return 2; }
  FILE* fi = fopen(argv[2], "rb");
  if (!fi) return 2;
  int32_t hd[6];
  double min_dist = 0.0, cams[4][4], T_nb[4][12], distance = 0.0, radius = 0.0;
  if (fread(hd, 4, 6, fi) != 6 || fread(&min_dist, 8, 1, fi) != 1 || fread(cams, 8, 16, fi) != 16 || fread(T_nb, 8, 48, fi) != 48 || fread(&distance, 8, 1, fi) != 1 ||
      fread(&radius, 8, 1, fi) != 1) return 2;
  const int n = hd[0], H = hd[1], W = hd[2], cap = hd[3];
  std::vector<float> maps((size_t)8 * H * W);
  std::vector<uint8_t> frames((size_t)n * 4 * H * W);
  if (fread(maps.data(), 4, maps.size(), fi) != maps.size() || fread(frames.data(), 1, frames.size(), fi) != frames.size()) return 2;
  fclose(fi);
  d2fe_flow_params fp;
  d2fe_flow_default_params(&fp);
  fp.track.total_feature_num = hd[4]; fp.track.feature_min_dist = min_dist;
  {      // the host helper needs no device: the view's virtual camera
    d2fe_camera vc;
    if (d2fe_cylinder_camera(W, H, 200.0, &vc) != D2FE_OK || vc.kind != D2FE_CAM_CYLINDRICAL || vc.p[0] != (double)W / (200.0 * (M_PI / 180.0)) || vc.p[1] != vc.p[0] ||
        vc.p[2] != W / 2 || vc.p[3] != H / 2 || vc.p[4] != 0.0) return 5;
  }
  d2fe_config c;
  d2fe_default_config(&c);
  c.max_width = W; c.max_height = H; c.max_batch = 4; c.max_keypoints = cap; c.keypoint_threshold = 0.15f; c.precision = D2FE_PREC_F32_WINO;
  d2fe_handle h = nullptr;
  CHECK(d2fe_create(&c, &h));
  {
    d2fe_weights::File f; d2fe_superpoint_weights w; std::string err;
    if (!f.load(argv[1]) || !d2fe_weights::superpoint(f, &w, &err)) { fprintf(stderr, "%s%s\n", f.error.c_str(), err.c_str()); return 3; }
    CHECK(d2fe_load_superpoint(h, &w));
  }
  const int rc = run(h, argv[3], n, H, W, cap, fp, cams, T_nb, distance, radius, maps, frames);      // the pipe is gone when run() returns
  d2fe_destroy(h);
  if (rc) return rc;
  printf("quad_bearings_test OK\n");
  return 0;
}
