// quad_flow_test.cpp -- the quad pipe's flow_lk mode as D2SLAM's C++ would drive it: plain C++ (g++), only the C ABI of include/d2fe.h behind include/d2fe.hpp
// (D2FrontEnd::QuadPipe::flowEnable / flow); no Python, no torch, no HIP call of its own.  tests/test_quad_pipe_flow.py compares every output with a one-lane,
// one-quad-frame pipe of the Python binding.
//   usage: quad_flow_test <sp.d2fw> <in.bin> <out.bin> <lanes> <quads>
//   in.bin : int32 n (quad frames, a multiple of quads), H, W (raw frame = view), cap, total_feature_num, 0; double feature_min_dist;
//            float maps[4][2][H][W] (mapx, mapy; no gain); u8 frames[n][4][H][W]
//   out.bin: per quad frame, with T = max(total_feature_num, 1) slots, zeros behind the end of a list: int32 n[4], n_new[4], num[4], n_cand[4], float pts[4][T][2],
//            int32 id[4][T], src[4][T], float nb_lk[4][T][2], u8 nb_lk_status[4][T], int32 nb_n[4] (the keypoint-based neighbour matches beside the mode)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "d2fe.hpp"
#include "d2fe_weights_file.hpp"

#define CHECK(x) do { int e_ = (x); if (e_ != D2FE_OK) { fprintf(stderr, "%s: %d %s\n", #x, e_, d2fe_last_error()); return 5; } } while (0)

namespace {

int run(d2fe_handle h, const char* out_path, int lanes, int quads, int n, int H, int W, int cap, const d2fe_flow_params& fp, const std::vector<float>& maps,
        const std::vector<uint8_t>& frames) {
  d2fe_quad_pipe_config pc;
  d2fe_quad_pipe_default_config(&pc);
  pc.lanes = lanes; pc.quads = quads; pc.raw_width = W; pc.raw_height = H; pc.width = W; pc.height = H; pc.cap = cap; pc.radius_neighbour = 0.2 * W;
  pc.netvlad = 0; pc.match_neighbour = 1; pc.match_prev = 0;      // the keypoint-based neighbour matchKNN is this mode's matchKNN
  d2fe_quad_maps qm{};
  const size_t npix = (size_t)H * W;
  for (int c = 0; c < 4; ++c) { qm.mapx[c] = &maps[(2 * c) * npix]; qm.mapy[c] = &maps[(2 * c + 1) * npix]; qm.gain[c] = nullptr; }
  qm.device = 0;
  D2FrontEnd::QuadPipe pipe(h, pc, qm);
  if (!pipe.ok() || !pipe.flowEnable(&fp)) return 5;
  if (pipe.flowEnable(&fp)) { fprintf(stderr, "a second enable was accepted\n"); return 6; }
  if (pipe.trackEnable(nullptr)) { fprintf(stderr, "sp_lk was accepted beside the flow landmarks\n"); return 6; }
  FILE* fo = fopen(out_path, "wb");
  if (!fo) return 2;
  const int steps = n / quads, T = fp.track.total_feature_num > 1 ? fp.track.total_feature_num : 1;
  const size_t rimg = npix;
  std::vector<int64_t> tk(steps);
  std::vector<D2FrontEnd::QuadFlowList> lists;
  std::vector<D2FrontEnd::QuadFlowNeighbourTracks> nb;
  auto finish = [&](int j) -> int {
    d2fe_quad_pipe_result r;
    CHECK(d2fe_quad_pipe_wait(pipe.get(), tk[j], &r));
    if (!r.nb_n || r.prev_n || !pipe.flow(tk[j], lists, nb) || (int)lists.size() != 4 * quads) return 6;
    for (int q = 0; q < quads; ++q) {
      std::vector<int32_t> cnt(16), id(4 * T, 0), src(4 * T, 0);
      std::vector<float> pts(8 * T, 0.f), xy(8 * T, 0.f);
      std::vector<uint8_t> st(4 * T, 0);
      for (int c = 0; c < 4; ++c) {
        const D2FrontEnd::QuadFlowList& l = lists[q * 4 + c];
        const D2FrontEnd::QuadFlowNeighbourTracks& t = nb[q * 4 + c];
        const int m = (int)l.pts.size();
        if (m > T || (int)l.id.size() != m || (int)l.src.size() != m || t.lk.size() != t.lk_status.size()) return 6;
        cnt[c] = m; cnt[4 + c] = l.n_new; cnt[8 + c] = l.num; cnt[12 + c] = l.n_cand;
        for (int i = 0; i < m; ++i) {
          pts[(c * T + i) * 2] = l.pts[i].x; pts[(c * T + i) * 2 + 1] = l.pts[i].y;
          id[c * T + i] = l.id[i]; src[c * T + i] = l.src[i];
        }
        for (size_t i = 0; i < t.lk.size(); ++i) { xy[(c * T + i) * 2] = t.lk[i].x; xy[(c * T + i) * 2 + 1] = t.lk[i].y; st[c * T + i] = t.lk_status[i]; }
      }
      fwrite(cnt.data(), 4, 16, fo); fwrite(pts.data(), 4, pts.size(), fo); fwrite(id.data(), 4, id.size(), fo); fwrite(src.data(), 4, src.size(), fo);
      fwrite(xy.data(), 4, xy.size(), fo); fwrite(st.data(), 1, st.size(), fo); fwrite(r.nb_n + (size_t)q * 4, 4, 4, fo);
    }
    return 0;
  };
  for (int i = 0; i < steps; ++i) {      // the tracker waits `lanes` submits behind the image callback
    CHECK(d2fe_quad_pipe_submit(pipe.get(), frames.data() + (size_t)i * quads * 4 * rimg, W, rimg, 4 * rimg, &tk[i]));
    if (i == 0) {                        // nobody has waited for the ticket: D2FE_ERR_NOT_READY; and the other mode's result does not exist
      d2fe_quad_flow_result fr;
      if (d2fe_quad_flow_result_get(pipe.get(), tk[0], &fr) != D2FE_ERR_NOT_READY) { fprintf(stderr, "lists before the wait\n"); return 6; }
      d2fe_quad_track_result tr;
      if (d2fe_quad_track_result_get(pipe.get(), tk[0], &tr) != D2FE_ERR_UNSUPPORTED) { fprintf(stderr, "sp_lk lists on a flow pipe\n"); return 6; }
    }
    if (i >= lanes) { const int rc = finish(i - lanes); if (rc) return rc; }
  }
  for (int j = steps > lanes ? steps - lanes : 0; j < steps; ++j) { const int rc = finish(j); if (rc) return rc; }
  fclose(fo);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 6) { fprintf(stderr, "usage: quad_flow_test <sp.d2fw> <in.bin> <out.bin> <lanes> <quads>\n"); return 2; }
  const int lanes = atoi(argv[4]), quads = atoi(argv[5]);
  FILE* fi = fopen(argv[2], "rb");
  if (!fi) return 2;
  int32_t hd[6];
  double min_dist = 0.0;
  if (fread(hd, 4, 6, fi) != 6 || fread(&min_dist, 8, 1, fi) != 1) return 2;
  const int n = hd[0], H = hd[1], W = hd[2], cap = hd[3];
  if (quads < 1 || n % quads) return 2;
  std::vector<float> maps((size_t)8 * H * W);
  std::vector<uint8_t> frames((size_t)n * 4 * H * W);
  if (fread(maps.data(), 4, maps.size(), fi) != maps.size() || fread(frames.data(), 1, frames.size(), fi) != frames.size()) return 2;
  fclose(fi);
  d2fe_flow_params fp;
  d2fe_flow_default_params(&fp);
  fp.track.total_feature_num = hd[4]; fp.track.feature_min_dist = min_dist;

  d2fe_config c;
  d2fe_default_config(&c);
  c.max_width = W; c.max_height = H; c.max_batch = 4 * quads; c.max_keypoints = cap; c.keypoint_threshold = 0.15f; c.precision = D2FE_PREC_F32_WINO;
  d2fe_handle h = nullptr;
  CHECK(d2fe_create(&c, &h));
  {
    d2fe_weights::File f; d2fe_superpoint_weights w; std::string err;
    if (!f.load(argv[1]) || !d2fe_weights::superpoint(f, &w, &err)) { fprintf(stderr, "%s%s\n", f.error.c_str(), err.c_str()); return 3; }
    CHECK(d2fe_load_superpoint(h, &w));
  }
  const int rc = run(h, argv[3], lanes, quads, n, H, W, cap, fp, maps, frames);      // the pipe is gone when run() returns
  d2fe_destroy(h);
  if (rc) return rc;
  printf("quad_flow_test OK: %d quad frames, %d per submit, %d lanes\n", n, quads, lanes);
  return 0;
}
