// keyframe_window_test.cpp -- remote tracking against the keyframe window as D2SLAM's C++ would drive it: plain C++ (g++), only the C ABI of include/d2fe.h behind
// the RAII wrappers of include/d2fe.hpp (StereoPipe + KeyframeWindow); no Python, no torch in the process.  The first frames of a sequence become keyframes (push),
// the sliding window drops some of them (retain), the later frames are tracked against the window in place in the lane's result block (device view -> track -> collect);
// tests/test_cpp_keyframe_window.py holds what it writes to the Python binding.  Replaces D2FeatureTracker::trackRemoteFrames (d2featuretracker.cpp:237-310).
//   usage: keyframe_window_test <sp.d2fw> <nv.d2fw> <in.bin> <out.bin> <lanes> <keyframes> <thres>
//   in.bin : int32 n (frames), H, W, cap; float keypoint_threshold; u8 images[n][2][H][W]
//   out.bin: per tracked frame: int64 keyframe_tag; int32 keyframe_pos, dir_a, dir_b, n_window; float sim; float sims[capacity]; int32 local_view, remote_view,
//            n_match; int32 q[cap], t[cap]; float dist[cap] (entries behind n_match are zeros); then int32 size and int64 tags[size] of the window
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "d2fe.hpp"
#include "d2fe_weights_file.hpp"

#define CHECK(x) do { int e_ = (x); if (e_ != D2FE_OK) { fprintf(stderr, "%s: %d %s\n", #x, e_, d2fe_last_error()); return 5; } } while (0)

namespace {
void put(std::vector<char>& b, const void* p, size_t n) { const char* c = static_cast<const char*>(p); b.insert(b.end(), c, c + n); }
}  // namespace

int main(int argc, char** argv) {
  if (argc != 8) { fprintf(stderr, "usage: keyframe_window_test <sp.d2fw> <nv.d2fw> <in.bin> <out.bin> <lanes> <keyframes> <thres>\n"); return 2; }
  const int lanes = atoi(argv[5]), nk = atoi(argv[6]);
  const double thres = atof(argv[7]);
  FILE* fi = fopen(argv[3], "rb");
  if (!fi) return 2;
  int32_t hd[4]; float kthr = 0.f;
  if (fread(hd, 4, 4, fi) != 4 || fread(&kthr, 4, 1, fi) != 1) return 2;
  const int n = hd[0], H = hd[1], W = hd[2], cap = hd[3];
  if (n < 1 || nk < 3 || nk >= n || lanes < 1) return 2;
  std::vector<uint8_t> img((size_t)n * 2 * H * W);
  if (fread(img.data(), 1, img.size(), fi) != img.size()) return 2;
  fclose(fi);

  d2fe_config c;
  d2fe_default_config(&c);
  c.max_width = W; c.max_height = H; c.max_batch = 2; c.max_keypoints = cap; c.precision = D2FE_PREC_F32_WINO; c.keypoint_threshold = kthr;
  d2fe_handle h = nullptr;
  CHECK(d2fe_create(&c, &h));
  {
    d2fe_weights::File f; d2fe_superpoint_weights w; std::string err;
    if (!f.load(argv[1]) || !d2fe_weights::superpoint(f, &w, &err)) { fprintf(stderr, "%s%s\n", f.error.c_str(), err.c_str()); return 3; }
    CHECK(d2fe_load_superpoint(h, &w));
  }
  {
    d2fe_weights::File f; std::vector<d2fe_nv_layer> layers; d2fe_netvlad_weights w; std::string err;
    if (!f.load(argv[2]) || !d2fe_weights::netvlad(f, &layers, &w, &err)) { fprintf(stderr, "%s%s\n", f.error.c_str(), err.c_str()); return 3; }
    CHECK(d2fe_load_netvlad(h, &w));
  }
  const size_t npix = (size_t)H * W;
  std::vector<char> out;
  int hits = 0, tracked = 0;
  {
    d2fe_pipe_config pc;
    d2fe_pipe_default_config(&pc);
    pc.lanes = lanes; pc.frames = 1; pc.width = W; pc.height = H; pc.cap = cap; pc.netvlad = 1;
    D2FrontEnd::StereoPipe pipe(h, pc);
    if (!pipe.ok()) return 5;
    d2fe_window_config wc;
    d2fe_window_default_config(&wc);
    wc.capacity = nk; wc.thres = thres; wc.slots = 2; wc.max_queries = 1;
    D2FrontEnd::KeyframeWindow win(pipe, wc);      // declared after the pipe: destroyed before it
    if (!win.ok()) return 5;
    int32_t g[4];
    CHECK(d2fe_pipe_geometry(pipe.get(), &g[0], &g[1], &g[2], &g[3]));
    D2FrontEnd::StereoFrameResult fr;
    for (int i = 0; i < n; ++i) {
      D2FrontEnd::ImageView L, R;
      L.data = &img[((size_t)i * 2) * npix]; R.data = &img[((size_t)i * 2 + 1) * npix];
      L.rows = R.rows = H; L.cols = R.cols = W; L.step = R.step = (size_t)W; L.channels = R.channels = 1;
      const int64_t tk = pipe.submit(L, R);
      if (tk < 0) return 5;
      if (i < nk) {
        // processFrame: the frame becomes the newest keyframe; a second call with the same frame_id changes nothing
        if (!win.push(tk, 0, 100 + i) || !win.push(tk, 0, 100 + i) || win.size() != i + 1) return 6;
        if (i == nk - 1) {
          // updatebySldWin: the sliding window holds keyframes 0 and 2 (and one the tracker never saw); the newest stays although it is not listed
          if (win.retain({100, 102, 77}) != nk - 3 || win.size() != 3) return 6;
        }
        if (!pipe.wait(tk, fr)) return 5;
        continue;
      }
      d2fe_pipe_device_result v;
      CHECK(d2fe_pipe_device_view(pipe.get(), tk, win.stream(), &v));
      const bool ok = win.track_device(v.d_netvlad, (size_t)g[3], v.d_desc, (size_t)g[1] * g[2], v.d_n_kp, 1, 1, i % 2, nullptr);      // the window's own stream: no other to wait for
      CHECK(d2fe_pipe_device_release(pipe.get(), tk, win.stream()));
      if (!ok || !pipe.wait(tk, fr)) return 5;
      d2fe_window_result r;
      if (!win.collect(i % 2, r)) return 5;
      if (r.nq != 1 || r.views != 1 || r.cap != cap || r.capacity != nk || r.n_window != 3) { fprintf(stderr, "slot geometry\n"); return 7; }
      const D2FrontEnd::RemoteTrack t = D2FrontEnd::KeyframeWindow::track(r, 0);
      const int32_t head[4] = {t.keyframe_pos, t.dir_a, t.dir_b, r.n_window};
      put(out, &t.keyframe_tag, 8); put(out, head, sizeof(head)); put(out, &t.similarity, 4); put(out, r.sims, 4 * (size_t)nk);
      const int32_t pv[3] = {t.local_view[0], t.remote_view[0], (int32_t)t.matches[0].size()};
      put(out, pv, sizeof(pv));
      std::vector<int32_t> q((size_t)cap, 0), tt((size_t)cap, 0);
      std::vector<float> d((size_t)cap, 0.f);
      for (size_t j = 0; j < t.matches[0].size(); ++j) { q[j] = t.matches[0][j].queryIdx; tt[j] = t.matches[0][j].trainIdx; d[j] = t.matches[0][j].distance; }
      put(out, q.data(), 4 * q.size()); put(out, tt.data(), 4 * tt.size()); put(out, d.data(), 4 * d.size());
      ++tracked; hits += t.keyframe_pos >= 0;
    }
    const std::vector<int64_t> tags = win.tags();
    const int32_t sz = (int32_t)tags.size();
    put(out, &sz, 4); put(out, tags.data(), 8 * tags.size());
  }
  FILE* fo = fopen(argv[4], "wb");
  if (!fo) return 2;
  fwrite(out.data(), 1, out.size(), fo);
  fclose(fo);
  d2fe_destroy(h);
  printf("keyframe_window_test OK: %d keyframes pushed, 3 retained, %d frames tracked, %d hits\n", nk, tracked, hits);
  return 0;
}
