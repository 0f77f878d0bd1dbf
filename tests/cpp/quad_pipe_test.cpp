// quad_pipe_test.cpp -- quadcam frames in flight as D2SLAM's C++ would drive them: plain C++ (g++), only the C ABI of include/d2fe.h (d2fe_quad_pipe_*)
// behind the RAII wrapper of include/d2fe.hpp; no Python, no torch, no HIP call of its own.  Weights come from D2FW containers (include/d2fe_weights_file.hpp),
// maps and frames from a raw file; tests/test_quad_pipe.py compares every output with a one-lane, one-quad-frame pipe of the Python binding.
//   usage: quad_pipe_test <sp.d2fw> <nv.d2fw> <in.bin> <out.bin> <lanes> <quads>
//   in.bin : int32 n (quad frames, a multiple of quads), RH, RW, UH, UW, cap; float maps[4][3][UH][UW] (mapx, mapy, gain); u8 frames[n][4][RH][RW]
//   out.bin: per quad frame: int32 n_kp[4], float kps[4][cap][2], int32 nb_n[4], nb_q[4][cap], nb_t[4][cap], prev_n[4], prev_q[4][cap], prev_t[4][cap]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "d2fe.hpp"
#include "d2fe_weights_file.hpp"

#define CHECK(x) do { int e_ = (x); if (e_ != D2FE_OK) { fprintf(stderr, "%s: %d %s\n", #x, e_, d2fe_last_error()); return 5; } } while (0)

namespace {

int run(d2fe_handle h, const char* out_path, int lanes, int quads, int n, int RH, int RW, int UH, int UW, int cap, const std::vector<float>& maps,
        const std::vector<uint8_t>& frames) {
  d2fe_quad_pipe_config pc;
  d2fe_quad_pipe_default_config(&pc);
  pc.lanes = lanes; pc.quads = quads; pc.raw_width = RW; pc.raw_height = RH; pc.width = UW; pc.height = UH; pc.cap = cap; pc.radius_neighbour = 0.2 * UW;
  d2fe_quad_maps qm{};
  const size_t npix = (size_t)UH * UW;
  for (int c = 0; c < 4; ++c) { qm.mapx[c] = &maps[(3 * c) * npix]; qm.mapy[c] = &maps[(3 * c + 1) * npix]; qm.gain[c] = &maps[(3 * c + 2) * npix]; }
  qm.device = 0;
  D2FrontEnd::QuadPipe pipe(h, pc, qm);
  if (!pipe.ok()) return 5;
  int32_t gq = 0, gcap = 0, gd = 0, gg = 0;
  CHECK(d2fe_quad_pipe_geometry(pipe.get(), &gq, &gcap, &gd, &gg));
  if (gq != quads || gcap != cap || gd != 256 || gg <= 0 || d2fe_quad_pipe_lanes(pipe.get()) != lanes) { fprintf(stderr, "geometry\n"); return 6; }
  FILE* fo = fopen(out_path, "wb");
  if (!fo) return 2;
  const int steps = n / quads;
  const size_t rimg = (size_t)RH * RW, cq = (size_t)4 * cap;
  std::vector<int64_t> tk(steps);
  auto finish = [&](int j) -> int {
    d2fe_quad_pipe_result r;
    CHECK(d2fe_quad_pipe_wait(pipe.get(), tk[j], &r));
    for (int q = 0; q < quads; ++q) {
      fwrite(r.n_kp + 4 * q, 4, 4, fo);
      fwrite(r.kps_xy + q * cq * 2, 4, cq * 2, fo);
      fwrite(r.nb_n + 4 * q, 4, 4, fo); fwrite(r.nb_q + q * cq, 4, cq, fo); fwrite(r.nb_t + q * cq, 4, cq, fo);
      fwrite(r.prev_n + 4 * q, 4, 4, fo); fwrite(r.prev_q + q * cq, 4, cq, fo); fwrite(r.prev_t + q * cq, 4, cq, fo);
    }
    return 0;
  };
  for (int i = 0; i < steps; ++i) {      // the tracker waits `lanes` submits behind the image callback
    CHECK(d2fe_quad_pipe_submit(pipe.get(), frames.data() + (size_t)i * quads * 4 * rimg, RW, rimg, 4 * rimg, &tk[i]));
    if (i >= lanes) { const int rc = finish(i - lanes); if (rc) return rc; }
  }
  for (int j = steps > lanes ? steps - lanes : 0; j < steps; ++j) { const int rc = finish(j); if (rc) return rc; }
  fclose(fo);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 7) { fprintf(stderr, "usage: quad_pipe_test <sp.d2fw> <nv.d2fw> <in.bin> <out.bin> <lanes> <quads>\n"); return 2; }
  const int lanes = atoi(argv[5]), quads = atoi(argv[6]);
  FILE* fi = fopen(argv[3], "rb");
  if (!fi) return 2;
  int32_t hd[6];
  if (fread(hd, 4, 6, fi) != 6) return 2;
  const int n = hd[0], RH = hd[1], RW = hd[2], UH = hd[3], UW = hd[4], cap = hd[5];
  if (quads < 1 || n % quads) return 2;
  std::vector<float> maps((size_t)12 * UH * UW);
  std::vector<uint8_t> frames((size_t)n * 4 * RH * RW);
  if (fread(maps.data(), 4, maps.size(), fi) != maps.size() || fread(frames.data(), 1, frames.size(), fi) != frames.size()) return 2;
  fclose(fi);

  d2fe_config c;
  d2fe_default_config(&c);
  c.max_width = UW; c.max_height = UH; c.max_batch = 4 * quads; c.max_keypoints = cap; c.keypoint_threshold = 0.15f; c.precision = D2FE_PREC_F32_WINO;
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
  const int rc = run(h, argv[4], lanes, quads, n, RH, RW, UH, UW, cap, maps, frames);      // the pipe is gone when run() returns
  d2fe_destroy(h);
  if (rc) return rc;
  printf("quad_pipe_test OK: %d quad frames, %d per submit, %d lanes\n", n, quads, lanes);
  return 0;
}
