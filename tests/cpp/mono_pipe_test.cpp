// The single-camera pipe (d2fe_pipe_camera::mono, ::depth through d2fe_pipe_create_camera: the reference's MONOCULAR and PINHOLE_DEPTH configurations) through the C++ mirror (include/d2fe.hpp):
// StereoPipe::submit(left) and submit(left, depth) -> wait must deliver the same bytes as the C ABI (d2fe_pipe_submit / d2fe_pipe_submit_depth, d2fe_pipe_wait,
// d2fe_pipe_track_result_get, d2fe_pipe_depth_result_get) on a second pipe of the same configuration fed the same frames, and the left keypoints must be infer()'s.
// Three frames (gray 0, gray 1, gray 0) with sp_lk, so that the list is carried; the depth frame has rows further apart than it is wide.
// Usage: mono_pipe_test <in.bin> <out.bin>   in: the input file of mirror_test (H, W, max keypoints, the 12 SuperPoint layers, two gray frames) followed by the depth
// frame as uint16 [H][W + 8].  out: per frame the keypoints, their depth values, the list positions and their depth values.  Exit code 0 = all equal.
#include <cstdio>
#include <cstring>
#include <vector>

#include "d2fe.hpp"

using namespace D2FrontEnd;

template <typename T>
static bool rd(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }
template <typename T>
static void wr(FILE* f, const T* p, size_t n) { int32_t m = (int32_t)n; fwrite(&m, 4, 1, f); if (n) fwrite(p, sizeof(T), n, f); }

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
  const int DW = W + 8;       // depth row pitch in pixels
  std::vector<uint8_t> img[2] = {std::vector<uint8_t>((size_t)H * W), std::vector<uint8_t>((size_t)H * W)};
  std::vector<uint16_t> dep((size_t)H * DW);
  if (!rd(fi, img[0].data(), img[0].size()) || !rd(fi, img[1].data(), img[1].size()) || !rd(fi, dep.data(), dep.size())) return 2;
  fclose(fi);

  SuperPointConfig cfg;
  cfg.max_keypoints = maxkp; cfg.input_width = W; cfg.input_height = H;
  SuperPoint sp(cfg);
  if (!sp.build(w)) return 3;
  std::vector<Point2f> k0;
  std::vector<float> d0, s0;
  if (!sp.infer(ImageView(img[0].data(), H, W), k0, d0, s0) || k0.empty()) return 4;

  d2fe_pipe_config pc;
  d2fe_pipe_default_config(&pc);
  d2fe_pipe_camera cam;
  d2fe_pipe_camera_default(&cam);
  if (cam.mono != 0 || cam.depth != 0 || cam.struct_size != (int32_t)sizeof(cam) || pc.struct_size != (int32_t)sizeof(pc)) return 6;
  pc.lanes = 2; pc.width = W; pc.height = H; pc.cap = maxkp; pc.netvlad = 0; pc.match_prev = 1; pc.ratio = 0.8;
  cam.mono = 1;
  {
    StereoPipe refused(sp.handle(), pc, nullptr, &cam);        // match_lr is still 1
    if (refused.ok()) return 6;
  }
  pc.match_lr = 0;
  {
    d2fe_pipe_camera bad = cam;
    bad.mono = 0; bad.depth = 1;
    StereoPipe refused(sp.handle(), pc, nullptr, &bad);        // depth without mono
    if (refused.ok()) return 6;
  }
  // (a) mono alone: the one image in, the left row out, nothing on the right
  {
    StereoPipe mono(sp.handle(), pc, nullptr, &cam);
    if (!mono.ok()) return 6;
    if (mono.submit(ImageView(img[0].data(), H, W), ImageView(img[1].data(), H, W)) >= 0) return 7;       // a right image is refused ...
    const int64_t t = mono.submit(ImageView(img[0].data(), H, W));                                      // ... and the pipe goes on
    StereoFrameResult r;
    if (t < 0 || !mono.wait(t, r)) return 7;
    if (r.kps_left.size() != k0.size() || std::memcmp(r.kps_left.data(), k0.data(), sizeof(Point2f) * k0.size()) || std::memcmp(r.desc_left.data(), d0.data(), d0.size() * 4)) return 7;
    if (!r.kps_right.empty() || !r.left_right.empty() || !r.depth_mm.empty() || !r.tracks.pts.empty()) return 7;
  }
  // (b) mono + depth + sp_lk: the mirror against the C ABI
  cam.depth = 1; pc.sp_lk = 1;
  d2fe_track_params tp;
  d2fe_track_default_params(&tp);
  tp.total_feature_num = 60;
  StereoPipe pipe(sp.handle(), pc, &tp, &cam);
  if (!pipe.ok()) return 8;
  if (pipe.submit(ImageView(img[0].data(), H, W)) >= 0) return 8;          // a depth pipe refuses a frame without depth
  d2fe_pipe cp = nullptr;
  d2fe_pipe_config cc = pc;
  cc.frames = 1;
  if (d2fe_pipe_create_camera(sp.handle(), &cc, &cam, &cp) != D2FE_OK || d2fe_pipe_set_track_params(cp, &tp) != D2FE_OK) return 8;
  FILE* fo = fopen(argv[2], "wb");
  if (!fo) return 2;
  int rc = 0;
  int64_t tm[3], tc[3];
  for (int i = 0; i < 3 && !rc; ++i) {
    const uint8_t* g = img[i & 1].data();
    tm[i] = pipe.submit(ImageView(g, H, W), DepthView(dep.data(), H, W, (size_t)DW * 2));
    if (tm[i] < 0 || d2fe_pipe_submit_depth(cp, g, dep.data(), W, DW * 2, 0, 0, &tc[i]) != D2FE_OK) rc = 9;
  }
  for (int i = 0; i < 3 && !rc; ++i) {
    StereoFrameResult r;
    d2fe_pipe_result cr;
    d2fe_pipe_track_result ct;
    d2fe_pipe_depth_result cd;
    if (d2fe_pipe_depth_result_get(cp, tc[i], &cd) != D2FE_ERR_NOT_READY) { rc = 10; break; }
    if (!pipe.wait(tm[i], r) || d2fe_pipe_wait(cp, tc[i], &cr) != D2FE_OK || d2fe_pipe_track_result_get(cp, tc[i], &ct) != D2FE_OK ||
        d2fe_pipe_depth_result_get(cp, tc[i], &cd) != D2FE_OK) { rc = 10; break; }
    const size_t n = (size_t)cr.n_kp[0], m = (size_t)ct.n[0];
    if (cr.n_kp[1] != 0 || ct.right_xy || ct.right_status || !cd.track_depth_mm || cd.cap != cr.cap || cd.cap_tracks != ct.cap_tracks) { rc = 11; break; }
    if (r.kps_left.size() != n || r.depth_mm.size() != n || r.tracks.pts.size() != m || r.tracks.depth_mm.size() != m || !r.tracks.right.empty() || !r.tracks.right_status.empty()) { rc = 12; break; }
    if (n == 0 || m == 0) { rc = 12; break; }
    if (std::memcmp(r.kps_left.data(), cr.kps_xy, n * 8) || std::memcmp(r.desc_left.data(), cr.desc, n * cr.desc_dim * 4) || std::memcmp(r.depth_mm.data(), cd.kp_depth_mm, n * 2)) { rc = 13; break; }
    if (std::memcmp(r.tracks.pts.data(), ct.pts_xy, m * 8) || std::memcmp(r.tracks.id.data(), ct.id, m * 4) || std::memcmp(r.tracks.depth_mm.data(), cd.track_depth_mm, m * 2)) { rc = 14; break; }
    for (size_t j = n; j < (size_t)cd.cap; ++j) if (cd.kp_depth_mm[j]) rc = 15;
    for (size_t j = m; j < (size_t)cd.cap_tracks; ++j) if (cd.track_depth_mm[j]) rc = 15;
    if (i == 0 && (n != k0.size() || std::memcmp(r.kps_left.data(), k0.data(), n * 8))) rc = 16;
    wr(fo, &r.kps_left[0].x, 2 * n); wr(fo, r.depth_mm.data(), n); wr(fo, &r.tracks.pts[0].x, 2 * m); wr(fo, r.tracks.depth_mm.data(), m);
    std::printf("frame %d: %zu keypoints, %zu list entries (%d tracked in)\n", i, n, m, r.tracks.n_tracked_in);
  }
  fclose(fo);
  d2fe_pipe_destroy(cp);
  return rc;
}
