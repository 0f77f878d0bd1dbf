// loop_query_test.cpp -- the loop query behind a pipe as D2SLAM's C++ would drive it: plain C++ (g++), only the C ABI of include/d2fe.h behind the RAII wrappers
// of include/d2fe.hpp (StereoPipe / QuadPipe + LoopQuery); no Python, no torch in the process.  One sequence of frames through a stereo pipe (kind 0) or a quad
// pipe (kind 1, identity undistortion maps) with the loop sequence on every ticket; tests/test_cpp_loop_query.py holds what it writes to the Python binding.
// Replaces LoopDetector::processImageArray (loop_detector.cpp:23-215) of the reference.
//   usage: loop_query_test <sp.d2fw> <nv.d2fw> <in.bin> <out.bin> <kind 0|1> <lanes> <frames per submit> <thres> <max_index>
//   in.bin : int32 n (frames, a multiple of frames per submit), H, W, cap; float keypoint_threshold; u8 is_keyframe[n]; u8 images[n][2 or 4][H][W]
//   out.bin: per frame: int32 queried, label, keyframe, dir_old, ntotal_at_query; float sim; int32 added_label[V], dir_a[V], dir_b[V], n_match[V];
//            int32 q[V][cap], t[V][cap]; float dist[V][cap] (entries behind n_match are zeros); then int32 ntotal, keyframes
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

// the frames of one collected slot, appended to `b`
int record(const d2fe_loop_result& r, int frames, int V, int cap, std::vector<char>& b) {
  if (r.frames != frames || r.views != V || r.cap != cap) { fprintf(stderr, "slot geometry %d %d %d\n", r.frames, r.views, r.cap); return 7; }
  for (int f = 0; f < frames; ++f) {
    const D2FrontEnd::LoopHit h = D2FrontEnd::LoopQuery::hit(r, f);
    const int32_t head[5] = {h.queried ? 1 : 0, h.label, h.keyframe, h.dir_old, h.ntotal_at_query};
    put(b, head, sizeof(head)); put(b, &h.similarity, 4);
    std::vector<int32_t> nm(V);
    for (int i = 0; i < V; ++i) nm[i] = (int32_t)h.matches[i].size();
    put(b, h.added_label.data(), 4 * (size_t)V); put(b, h.dir_a.data(), 4 * (size_t)V); put(b, h.dir_b.data(), 4 * (size_t)V); put(b, nm.data(), 4 * (size_t)V);
    std::vector<int32_t> q((size_t)V * cap, 0), t((size_t)V * cap, 0);
    std::vector<float> d((size_t)V * cap, 0.f);
    for (int i = 0; i < V; ++i)
      for (size_t j = 0; j < h.matches[i].size(); ++j) {
        q[(size_t)i * cap + j] = h.matches[i][j].queryIdx; t[(size_t)i * cap + j] = h.matches[i][j].trainIdx; d[(size_t)i * cap + j] = h.matches[i][j].distance;
      }
    put(b, q.data(), 4 * q.size()); put(b, t.data(), 4 * t.size()); put(b, d.data(), 4 * d.size());
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 10) { fprintf(stderr, "usage: loop_query_test <sp.d2fw> <nv.d2fw> <in.bin> <out.bin> <kind> <lanes> <frames> <thres> <max_index>\n"); return 2; }
  const int kind = atoi(argv[5]), lanes = atoi(argv[6]), F = atoi(argv[7]), max_index = atoi(argv[9]);
  const double thres = atof(argv[8]);
  FILE* fi = fopen(argv[3], "rb");
  if (!fi) return 2;
  int32_t hd[4]; float kthr = 0.f;
  if (fread(hd, 4, 4, fi) != 4 || fread(&kthr, 4, 1, fi) != 1) return 2;
  const int n = hd[0], H = hd[1], W = hd[2], cap = hd[3], V = kind ? 4 : 1, NI = kind ? 4 : 2;
  if (F < 1 || n < 1 || n % F || (kind != 0 && kind != 1) || (kind == 0 && F != 1)) return 2;      // the StereoPipe wrapper carries one frame per submit
  std::vector<uint8_t> key((size_t)n), img((size_t)n * NI * H * W);
  if (fread(key.data(), 1, key.size(), fi) != key.size() || fread(img.data(), 1, img.size(), fi) != img.size()) return 2;
  fclose(fi);

  d2fe_config c;
  d2fe_default_config(&c);
  c.max_width = W; c.max_height = H; c.max_batch = NI * F; c.max_keypoints = cap; c.precision = D2FE_PREC_F32_WINO; c.keypoint_threshold = kthr;
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
  d2fe_loop_config lc;
  d2fe_loop_default_config(&lc);
  const int NS = lanes + 1, steps = n / F;
  lc.capacity_keyframes = n; lc.max_index = max_index; lc.thres = thres; lc.slots = NS;
  const size_t npix = (size_t)H * W;
  std::vector<char> out;
  std::vector<int64_t> tk(steps);
  int32_t tail[2] = {0, 0};
  int rc = 0;
  if (kind == 0) {
    d2fe_pipe_config pc;
    d2fe_pipe_default_config(&pc);
    pc.lanes = lanes; pc.frames = F; pc.width = W; pc.height = H; pc.cap = cap; pc.netvlad = 1;
    D2FrontEnd::StereoPipe pipe(h, pc);      // the wrapper is the one-frame form
    if (!pipe.ok()) return 5;
    D2FrontEnd::LoopQuery x(pipe, lc);       // declared after the pipe: destroyed before it
    if (!x.ok()) return 5;
    D2FrontEnd::StereoFrameResult fr;
    auto finish = [&](int j) -> int {
      d2fe_loop_result r;
      if (!pipe.wait(tk[j], fr) || !x.collect(j % NS, r)) return 5;
      if (r.ticket != tk[j]) return 7;
      return record(r, 1, V, cap, out);
    };
    for (int i = 0; i < steps && !rc; ++i) {
      D2FrontEnd::ImageView L, R;
      L.data = &img[((size_t)i * 2) * npix]; R.data = &img[((size_t)i * 2 + 1) * npix];
      L.rows = R.rows = H; L.cols = R.cols = W; L.step = R.step = (size_t)W; L.channels = R.channels = 1;
      tk[i] = pipe.submit(L, R);
      if (tk[i] < 0 || !x.enqueue(tk[i], i % NS, &key[(size_t)i])) return 5;
      if (i >= lanes - 1) rc = finish(i - (lanes - 1));
    }
    for (int j = steps > lanes - 1 ? steps - (lanes - 1) : 0; j < steps && !rc; ++j) rc = finish(j);
    tail[0] = x.ntotal(); tail[1] = x.keyframes();
  } else {
    d2fe_quad_pipe_config pc;
    d2fe_quad_pipe_default_config(&pc);
    pc.lanes = lanes; pc.quads = F; pc.raw_width = W; pc.raw_height = H; pc.width = W; pc.height = H; pc.cap = cap; pc.netvlad = 1; pc.match_neighbour = 0; pc.match_prev = 0;
    pc.radius_neighbour = 0.2 * W;
    std::vector<float> mx(npix), my(npix);
    for (int y = 0; y < H; ++y) for (int xx = 0; xx < W; ++xx) { mx[(size_t)y * W + xx] = (float)xx; my[(size_t)y * W + xx] = (float)y; }
    d2fe_quad_maps qm{};
    for (int cam = 0; cam < 4; ++cam) { qm.mapx[cam] = mx.data(); qm.mapy[cam] = my.data(); qm.gain[cam] = nullptr; }
    D2FrontEnd::QuadPipe pipe(h, pc, qm);
    if (!pipe.ok()) return 5;
    D2FrontEnd::LoopQuery x(pipe, lc);      // declared after the pipe: destroyed before it
    if (!x.ok()) return 5;
    auto finish = [&](int j) -> int {
      d2fe_quad_pipe_result o; d2fe_loop_result r;
      CHECK(d2fe_quad_pipe_wait(pipe.get(), tk[j], &o));
      if (!x.collect(j % NS, r)) return 5;
      if (r.ticket != tk[j]) return 7;
      return record(r, F, V, cap, out);
    };
    for (int i = 0; i < steps && !rc; ++i) {
      CHECK(d2fe_quad_pipe_submit(pipe.get(), img.data() + (size_t)i * F * 4 * npix, W, npix, 4 * npix, &tk[i]));
      if (!x.enqueue(tk[i], i % NS, &key[(size_t)i * F])) return 5;
      if (i >= lanes - 1) rc = finish(i - (lanes - 1));
    }
    for (int j = steps > lanes - 1 ? steps - (lanes - 1) : 0; j < steps && !rc; ++j) rc = finish(j);
    tail[0] = x.ntotal(); tail[1] = x.keyframes();
  }
  if (rc) return rc;
  put(out, tail, sizeof(tail));
  FILE* fo = fopen(argv[4], "wb");
  if (!fo) return 2;
  fwrite(out.data(), 1, out.size(), fo);
  fclose(fo);
  d2fe_destroy(h);
  printf("loop_query_test OK: %s pipe, %d submits of %d frames, %d lanes, %d index rows, %d keyframes\n", kind ? "quad" : "stereo", steps, F, lanes, tail[0], tail[1]);
  return 0;
}
