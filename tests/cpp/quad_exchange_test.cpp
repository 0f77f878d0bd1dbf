// quad_exchange_test.cpp -- the cross-agent exchange behind the quad pipe as D2SLAM's C++ would drive it: plain C++ (g++), only the C ABI of include/d2fe.h
// (d2fe_quad_pipe_* for the frames, d2fe_quad_exchange_* for the sequence) behind the RAII wrappers of include/d2fe.hpp; no Python, no torch in the process.
// ONE rank with loopback (the rank's own blocks as the remote agent): what a 1-GPU box can run of it.  Leg 1: the collective is a callback that copies the
// blocks on the given stream (hipMemcpyAsync of the runtime the library has already loaded, found with dlsym: this program links no HIP).  Leg 2, where
// d2fe_rccl_load succeeds: the same frames over a one-rank RCCL communicator; its results must equal leg 1's byte for byte.  tests/test_quad_exchange.py checks
// what leg 1 wrote.  Replaces loop_net.cpp:24-87 + d2featuretracker.cpp:212-233,282-297 of the reference.
//   usage: quad_exchange_test <sp.d2fw> <nv.d2fw> <in.bin> <out.bin> <lanes> <quads> <mode 0|1> <wire 0|1|2> <own_stream 0|1> <gate_thres>
//   in.bin : int32 n (quad frames, a multiple of quads), RH, RW, UH, UW, cap; float maps[4][3][UH][UW] (mapx, mapy, gain); u8 frames[n][4][RH][RW]
//   out.bin: per submit: int32 n_kp[4 quads], njobs, npairs, pairs_per_job, gate_n, job_rank[njobs], job_quad[njobs], dir_prev[njobs], float sims[njobs][4],
//            int32 n_match[npairs], local_view[npairs], remote_view[npairs], q[npairs][cap], t[npairs][cap], float dist[npairs][cap]
#include <dlfcn.h>

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

typedef int (*memcpy_async_fn)(void*, const void*, size_t, int, void*);
memcpy_async_fn g_copy = nullptr;
int g_calls = 0;

int gather_copy(void*, const void* d_send, void* d_recv, size_t bytes, void* stream) {      // world = 1: the gathered buffer IS the rank's blocks
  ++g_calls;
  return g_copy(d_recv, d_send, bytes, 3 /* hipMemcpyDeviceToDevice */, stream);
}

struct Geometry { int n, RH, RW, UH, UW, cap; };

// one leg: every submit of the file through a pipe with the exchange one submit behind it; the per-submit records go to `rec`
int run(d2fe_handle h, void* comm, const Geometry& g, int lanes, int quads, int mode, int wire, int own_stream, double thres, const std::vector<float>& maps,
        const std::vector<uint8_t>& frames, std::vector<std::vector<char>>& rec) {
  d2fe_quad_pipe_config pc;
  d2fe_quad_pipe_default_config(&pc);
  pc.lanes = lanes; pc.quads = quads; pc.raw_width = g.RW; pc.raw_height = g.RH; pc.width = g.UW; pc.height = g.UH; pc.cap = g.cap; pc.radius_neighbour = 0.2 * g.UW;
  d2fe_quad_maps qm{};
  const size_t npix = (size_t)g.UH * g.UW;
  for (int c = 0; c < 4; ++c) { qm.mapx[c] = &maps[(3 * c) * npix]; qm.mapy[c] = &maps[(3 * c + 1) * npix]; qm.gain[c] = &maps[(3 * c + 2) * npix]; }
  D2FrontEnd::QuadPipe pipe(h, pc, qm);
  if (!pipe.ok()) return 5;
  d2fe_quad_exchange_config xc;
  d2fe_quad_exchange_default_config(&xc);
  const int NS = lanes + 2;
  xc.world = 1; xc.rank = 0; xc.wire = wire; xc.loopback = 1; xc.slots = NS; xc.own_stream = own_stream; xc.timing = 1; xc.mode = mode; xc.gate_thres = thres;
  if (!comm) xc.all_gather = gather_copy;
  D2FrontEnd::QuadExchange x(pipe, comm, xc);
  if (!x.ok()) return 5;
  const int ppj = mode ? 4 : 16;
  if (x.jobs() != quads || x.pairs() != quads * ppj) { fprintf(stderr, "jobs %d pairs %d\n", x.jobs(), x.pairs()); return 6; }
  int32_t jr[64], jq[64];
  if (d2fe_quad_exchange_job_layout(1, 0, quads, 1, jr, jq, 64) != quads) return 6;
  const int steps = g.n / quads;
  const size_t rimg = (size_t)g.RH * g.RW;
  std::vector<int64_t> tk(steps);
  rec.assign(steps, {});
  auto finish = [&](int j) -> int {
    d2fe_quad_pipe_result o; d2fe_quad_exchange_result r;
    CHECK(d2fe_quad_pipe_wait(pipe.get(), tk[j], &o));
    if (!x.collect(j % NS, r)) return 5;
    if (r.ticket != tk[j] || r.njobs != quads || r.npairs != quads * ppj || r.pairs_per_job != ppj || r.cap != g.cap) { fprintf(stderr, "slot %d holds ticket %ld\n", j % NS, (long)r.ticket); return 7; }
    for (int q = 0; q < quads; ++q) if (r.job_rank[q] != jr[q] || r.job_quad[q] != jq[q]) { fprintf(stderr, "job layout\n"); return 7; }
    std::vector<char>& b = rec[j];
    auto put = [&](const void* p, size_t n) { const char* c = static_cast<const char*>(p); b.insert(b.end(), c, c + n); };
    const size_t NP = (size_t)r.npairs, NJ = (size_t)r.njobs;
    put(o.n_kp, 4 * 4 * (size_t)quads);
    put(&r.njobs, 4); put(&r.npairs, 4); put(&r.pairs_per_job, 4); put(&r.gate_n, 4);
    put(r.job_rank, 4 * NJ); put(r.job_quad, 4 * NJ); put(r.dir_prev, 4 * NJ); put(r.gate_sims, 16 * NJ);
    put(r.n_match, 4 * NP); put(r.local_view, 4 * NP); put(r.remote_view, 4 * NP);
    // entries behind a problem's n_match are not part of the result: written as zeros
    for (const void* arr : {(const void*)r.q_idx, (const void*)r.t_idx, (const void*)r.dist}) {
      std::vector<int32_t> t(NP * g.cap, 0);
      for (size_t p = 0; p < NP; ++p) memcpy(&t[p * g.cap], static_cast<const int32_t*>(arr) + p * g.cap, 4 * (size_t)r.n_match[p]);
      put(t.data(), 4 * t.size());
    }
    return 0;
  };
  int enq = 0;
  for (int i = 0; i < steps; ++i) {
    CHECK(d2fe_quad_pipe_submit(pipe.get(), frames.data() + (size_t)i * quads * 4 * rimg, g.RW, rimg, 4 * rimg, &tk[i]));
    for (; enq <= i - 1; ++enq) if (!x.enqueue(tk[enq], enq % NS)) return 5;        // one submit behind the pipe
    if (i >= lanes) { const int rc = finish(i - lanes); if (rc) return rc; }
  }
  for (; enq < steps; ++enq) if (!x.enqueue(tk[enq], enq % NS)) return 5;
  for (int j = steps > lanes ? steps - lanes : 0; j < steps; ++j) { const int rc = finish(j); if (rc) return rc; }
  return 0;      // the exchange goes before the pipe (declaration order)
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 11) { fprintf(stderr, "usage: quad_exchange_test <sp.d2fw> <nv.d2fw> <in.bin> <out.bin> <lanes> <quads> <mode> <wire> <own_stream> <gate_thres>\n"); return 2; }
  const int lanes = atoi(argv[5]), quads = atoi(argv[6]), mode = atoi(argv[7]), wire = atoi(argv[8]), own_stream = atoi(argv[9]);
  const double thres = atof(argv[10]);
  FILE* fi = fopen(argv[3], "rb");
  if (!fi) return 2;
  int32_t hd[6];
  if (fread(hd, 4, 6, fi) != 6) return 2;
  const Geometry g{hd[0], hd[1], hd[2], hd[3], hd[4], hd[5]};
  if (quads < 1 || quads > 64 || g.n % quads) return 2;
  std::vector<float> maps((size_t)12 * g.UH * g.UW);
  std::vector<uint8_t> frames((size_t)g.n * 4 * g.RH * g.RW);
  if (fread(maps.data(), 4, maps.size(), fi) != maps.size() || fread(frames.data(), 1, frames.size(), fi) != frames.size()) return 2;
  fclose(fi);

  d2fe_config c;
  d2fe_default_config(&c);
  c.max_width = g.UW; c.max_height = g.UH; c.max_batch = 4 * quads; c.max_keypoints = g.cap; c.precision = D2FE_PREC_F32;
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
  // the device copy of the callback leg: the HIP runtime is in the process already (libd2fe_hip.so depends on it)
  g_copy = reinterpret_cast<memcpy_async_fn>(dlsym(RTLD_DEFAULT, "hipMemcpyAsync"));
  if (!g_copy) { fprintf(stderr, "hipMemcpyAsync not found in the process\n"); return 4; }

  std::vector<std::vector<char>> cb, rc;
  int e = run(h, nullptr, g, lanes, quads, mode, wire, own_stream, thres, maps, frames, cb);
  if (e) return e;
  if (g_calls != g.n / quads) { fprintf(stderr, "the callback ran %d times for %d submits\n", g_calls, g.n / quads); return 8; }
  FILE* fo = fopen(argv[4], "wb");
  if (!fo) return 2;
  for (auto& b : cb) fwrite(b.data(), 1, b.size(), fo);
  fclose(fo);
  printf("quad_exchange_test callback leg OK: %d submits of %d quad frames, %d lanes, mode %d, wire %d, %s\n", g.n / quads, quads, lanes, mode, wire,
         own_stream ? "a stream of its own" : "the lanes' streams");

  if (d2fe_rccl_load(nullptr) == D2FE_OK) {
    char uid[128];
    void* comm = nullptr;
    CHECK(d2fe_rccl_unique_id(uid));
    CHECK(d2fe_rccl_comm_init_rank(uid, 1, 0, 0, &comm));
    e = run(h, comm, g, lanes, quads, mode, wire, own_stream, thres, maps, frames, rc);
    CHECK(d2fe_rccl_comm_destroy(comm));
    if (e) return e;
    for (size_t i = 0; i < cb.size(); ++i)
      if (cb[i].size() != rc[i].size() || memcmp(cb[i].data(), rc[i].data(), cb[i].size())) { fprintf(stderr, "RCCL leg differs from the callback leg at submit %zu\n", i); return 9; }
    printf("quad_exchange_test RCCL leg OK: one-rank ncclAllGather through %s, results equal the callback leg's\n", d2fe_rccl_path());
  } else {
    printf("quad_exchange_test RCCL leg skipped: %s\n", d2fe_last_error());
  }
  d2fe_destroy(h);
  printf("quad_exchange_test OK\n");
  return 0;
}
