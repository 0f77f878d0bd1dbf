// match_host.hip -- host side of the descriptor matcher (include/d2fe.h: d2fe_match_batch_device, d2fe_match_knn, d2fe_match_crosscheck,
// d2fe_match_fallback_rows): MatchHost (context.h), the handle's slots for the host-pointer calls, its per-stream scratch for the device call and the
// counters.  The kernels are match.hip.  Host code only.
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>
#include <string>

#include "context.h"
#ifdef D2FE_DEVTOOLS
#include "../../include/d2fe_debug.h"
#endif

using namespace d2fe;

namespace d2fe {
MatchHost::Lease::Lease(MatchHost& m_) : m(m_) {
  std::lock_guard<std::mutex> lk(m.mu);
  for (auto& sl : m.slots) if (!sl.busy) { slot = &sl; break; }
  if (!slot) {
    Slot sl;
    if (hipStreamCreateWithFlags(&sl.stream, hipStreamNonBlocking) != hipSuccess) return;
    m.slots.push_back(sl);
    slot = &m.slots.back();      // (a deque never relocates its elements)
  }
  slot->busy = true;      // the slot is this call's from here on
}

int MatchHost::Slot::grow(size_t want, bool pinned) {
  if (bytes >= want) return D2FE_OK;
  if (buf) { hipFree(buf); buf = nullptr; }
  if (pin) { (void)hipHostFree(pin); pin = nullptr; }
  bytes = 0;
  if (hipMalloc(&buf, want) != hipSuccess) return fail(D2FE_ERR_HIP, "hipMalloc match scratch");
  if (pinned && hipHostMalloc(&pin, want, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); pin = nullptr; }
  bytes = want;
  return D2FE_OK;
}

void MatchHost::release() {
  for (auto& sl : slots) { if (sl.stream) { hipStreamSynchronize(sl.stream); (void)hipStreamDestroy(sl.stream); } if (sl.buf) hipFree(sl.buf); if (sl.pin) (void)hipHostFree(sl.pin); }
  for (auto& sc : scratch) if (sc.cand4) hipFree(sc.cand4);
  for (void* p : {(void*)stats, (void*)stamps}) if (p) hipFree(p);
  slots.clear(); scratch.clear(); stats = nullptr; stamps = nullptr;
}
}  // namespace d2fe

extern "C" {

int d2fe_match_batch_device(d2fe_handle h, const d2fe_match_batch* mb, void* stream) {
  if (!h || !mb) return fail(D2FE_ERR_INVALID, "null argument");
  if (mb->npairs < 1 || mb->max_n < 1 || mb->max_n > 16384) return fail(D2FE_ERR_INVALID, "npairs/max_n out of range (max_n <= 16384)");
  if (mb->dim < 4 || mb->dim > 256 || (mb->dim & 3)) return fail(D2FE_ERR_INVALID, "dim must be a multiple of 4 in 4..256");
  if (mb->mode != 0 && mb->mode != 1) return fail(D2FE_ERR_INVALID, "bad mode");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  std::lock_guard<std::mutex> lk(h->match.mu);
  // the candidate scratch is keyed by the caller's stream: two calls on different streams (main and tail, two threads) can
  // overlap on the GPU and must not share cand4[pair][dir][row]; calls on one stream are ordered by the stream itself
  MatchHost::Scratch* sc = nullptr;
  for (auto& e : h->match.scratch) if (e.stream == s) { sc = &e; break; }
  if (!sc) { h->match.scratch.emplace_back(); sc = &h->match.scratch.back(); sc->stream = s; }
  // [arrival tickets | records]; the tickets are zero between launches (the kernel's last workgroup per pair resets its own), so a scratch
  // sized for more pairs serves any smaller batch
  const int tp = mb->npairs > sc->npairs ? mb->npairs : sc->npairs;
  const size_t need = match_scratch_bytes(tp, 0) + sizeof(int32_t) * 8 * (size_t)mb->max_n * mb->npairs;
  if (need > sc->bytes || mb->npairs > sc->npairs) {
    HIP_TRY(hipStreamSynchronize(s));      // the only work that can still read the old scratch is on this stream
    if (sc->cand4) hipFree(sc->cand4);
    sc->cand4 = nullptr; sc->bytes = 0; sc->npairs = 0;
    const size_t want = need > sc->bytes ? need : sc->bytes;
    HIP_TRY(hipMalloc(&sc->cand4, want));
    HIP_TRY(hipMemsetAsync(sc->cand4, 0, want, s));      // ON the caller's stream: hipMemset runs on the null stream, which a non-blocking stream does not wait for
    sc->bytes = want; sc->npairs = tp;
  }
  MatchArgs m;
  m.a = mb->d_a; m.b = mb->d_b; m.pts_a = mb->d_pts_a; m.pts_b = mb->d_pts_b;
  m.a_off = mb->d_a_off; m.b_off = mb->d_b_off; m.a_cnt = mb->d_a_cnt; m.b_cnt = mb->d_b_cnt;
  m.npairs = mb->npairs; m.dim = mb->dim; m.max_n = mb->max_n; m.mode = mb->mode;
  m.ratio = mb->ratio; m.radius = mb->radius;
  m.q_idx = mb->d_q_idx; m.t_idx = mb->d_t_idx; m.dist = mb->d_dist; m.n_out = mb->d_n_out;
  match_scratch_carve(sc->cand4, sc->npairs, &m); m.stats = h->match.stats; m.ncu = h->ncu;
#ifdef D2FE_DEVTOOLS
  if (d2fe_dev_env("D2FE_MATCH_STAMPS", 0) && (long)((mb->max_n + 31) / 32) * 2 * mb->npairs <= 4096) {
    if (!h->match.stamps) HIP_TRY(hipMalloc(&h->match.stamps, sizeof(unsigned long long) * 16 * 4096));
    HIP_TRY(hipMemsetAsync(h->match.stamps, 0, sizeof(unsigned long long) * 16 * 4096, s));
    m.stamps = h->match.stamps;
  }
#endif
  { ProfScope ps(h, D2FE_PROF_MATCH, s); HIP_TRY(launch_match(m, s)); }
  return D2FE_OK;
}

static int match_host(d2fe_handle h, int mode, const float* a, int na, const float* b, int nb, int dim, double ratio,
                      const float* pts_a, const float* pts_b, double radius, int32_t* q_idx, int32_t* t_idx, float* dist,
                      int cap, int* n_out) {
  if (n_out) *n_out = 0;
  if (!h || !n_out) return fail(D2FE_ERR_INVALID, "null argument");
  if (na < 0 || nb < 0 || cap < 0) return fail(D2FE_ERR_INVALID, "negative size");
  if (na == 0 || nb == 0) return D2FE_OK;
  if (!a || !b || !q_idx || !t_idx || !dist) return fail(D2FE_ERR_INVALID, "null pointer");
  const int max_n = na > nb ? na : nb;
  if (max_n > 16384) return fail(D2FE_ERR_UNSUPPORTED, "more than 16384 descriptors per side");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  const bool use_pts = mode == 0 && radius > 0 && pts_a && pts_b;
  const size_t fa = (size_t)na * dim, fb = (size_t)nb * dim;
  if (dim < 4 || dim > 256 || (dim & 3)) return fail(D2FE_ERR_INVALID, "dim must be a multiple of 4 in 4..256");
  // a private (stream, scratch) slot per call in flight: re-entrant; slots are created on demand and reused
  // a slot's buffers are sized for 1024 rows per side at first (every shipped configuration) and grow with the calls
  const size_t rows = (size_t)(max_n > 1024 ? max_n : 1024);
  const size_t slot_bytes = sizeof(float) * (2 * rows * 256 + 4 * rows + rows) + sizeof(int32_t) * (2 * rows + 16 + 8 * rows) + 128;
  MatchHost::Lease lease(h->match);
  if (!lease.slot) return fail(D2FE_ERR_HIP, "hipStreamCreate (match slot)");
  { const int rcg = lease.slot->grow(slot_bytes, h->use_pinned); if (rcg) return rcg; }
  hipStream_t s = lease.slot->stream;
  char* buf = lease.slot->buf;
  char* pin = lease.slot->pin;
  // device layout (words): a | b | pts_a | pts_b | meta {a_off, b_off, a_cnt, b_cnt, arrival ticket (0), pad x3} | n_out, pad x7 | dist | q | t | cand4
  // -- the inputs are one contiguous run (ONE H2D from the slot's pinned mirror), the outputs another (ONE D2H, one synchronisation)
  const size_t w_in = fa + fb + (use_pts ? 2 * (size_t)(na + nb) : 0) + 8;
  float* d_a = reinterpret_cast<float*>(buf);
  float* d_b = d_a + fa;
  float* d_pa = d_b + fb;
  float* d_pb = d_pa + (use_pts ? 2 * (size_t)na : 0);
  int32_t* d_meta = reinterpret_cast<int32_t*>(d_pb + (use_pts ? 2 * (size_t)nb : 0));
  int32_t* d_nout = d_meta + 8;
  float* d_dist = reinterpret_cast<float*>(d_nout + 8);
  int32_t* d_q = reinterpret_cast<int32_t*>(d_dist + max_n);
  int32_t* d_t = d_q + max_n;
  int32_t* d_c4 = d_t + max_n;
  const size_t w_out = 8 + 3 * (size_t)max_n;
  const int32_t meta[8] = {0, 0, na, nb, 0, 0, 0, 0};
  int rc = D2FE_OK;
  auto chk = [&](hipError_t er, const char* what) { if (er != hipSuccess && rc == D2FE_OK) rc = fail(D2FE_ERR_HIP, std::string(what) + ": " + hipGetErrorString(er)); };
  if (pin) {
    float* p = reinterpret_cast<float*>(pin);
    memcpy(p, a, sizeof(float) * fa); memcpy(p + fa, b, sizeof(float) * fb);
    float* pm = p + fa + fb;
    if (use_pts) { memcpy(pm, pts_a, sizeof(float) * 2 * na); memcpy(pm + 2 * (size_t)na, pts_b, sizeof(float) * 2 * nb); pm += 2 * (size_t)(na + nb); }
    memcpy(pm, meta, sizeof(meta));
    chk(hipMemcpyAsync(d_a, pin, sizeof(float) * w_in, hipMemcpyHostToDevice, s), "H2D inputs");
  } else {
    chk(hipMemcpyAsync(d_a, a, sizeof(float) * fa, hipMemcpyHostToDevice, s), "H2D a");
    chk(hipMemcpyAsync(d_b, b, sizeof(float) * fb, hipMemcpyHostToDevice, s), "H2D b");
    if (use_pts) {
      chk(hipMemcpyAsync(d_pa, pts_a, sizeof(float) * 2 * na, hipMemcpyHostToDevice, s), "H2D pts_a");
      chk(hipMemcpyAsync(d_pb, pts_b, sizeof(float) * 2 * nb, hipMemcpyHostToDevice, s), "H2D pts_b");
    }
    chk(hipMemcpyAsync(d_meta, meta, sizeof(meta), hipMemcpyHostToDevice, s), "H2D meta");
  }
  MatchArgs m;
  m.a = d_a; m.b = d_b; m.pts_a = use_pts ? d_pa : nullptr; m.pts_b = use_pts ? d_pb : nullptr;
  m.a_off = d_meta; m.b_off = d_meta + 1; m.a_cnt = d_meta + 2; m.b_cnt = d_meta + 3;
  m.npairs = 1; m.dim = dim; m.max_n = max_n; m.mode = mode; m.ratio = ratio; m.radius = use_pts ? radius : -1.0;
  m.q_idx = d_q; m.t_idx = d_t; m.dist = d_dist; m.n_out = d_nout; m.cand4 = d_c4; m.stats = h->match.stats;
  m.ncu = h->ncu;
  m.ticket = d_meta + 4;      // a zero word of the meta block: uploaded with the inputs, so zero at every launch
  if (rc == D2FE_OK) chk(launch_match(m, s), "launch_match");
  if (pin) {
    // pinned mirror of the output run, behind the inputs' mirror
    int32_t* po = reinterpret_cast<int32_t*>(pin) + ((w_in + 15) & ~(size_t)15);
    if (rc == D2FE_OK) chk(hipMemcpyAsync(po, d_nout, sizeof(int32_t) * w_out, hipMemcpyDeviceToHost, s), "D2H results");
    if (rc == D2FE_OK) chk(hipStreamSynchronize(s), "sync");
    if (rc == D2FE_OK) {
      const int cnt = po[0];
      const int k = cnt < cap ? cnt : cap;
      if (k > 0) {
        memcpy(dist, po + 8, sizeof(float) * k);
        memcpy(q_idx, po + 8 + max_n, sizeof(int32_t) * k);
        memcpy(t_idx, po + 8 + 2 * (size_t)max_n, sizeof(int32_t) * k);
      }
      *n_out = k;
      if (cnt > cap) rc = fail(D2FE_ERR_TRUNCATED, "match output capacity too small");
    }
    return rc;
  }
  int32_t cnt = 0;
  if (rc == D2FE_OK) chk(hipMemcpyAsync(&cnt, d_nout, sizeof(int32_t), hipMemcpyDeviceToHost, s), "D2H n");
  if (rc == D2FE_OK) chk(hipStreamSynchronize(s), "sync");
  if (rc == D2FE_OK) {
    const int k = cnt < cap ? cnt : cap;
    if (k > 0) {
      chk(hipMemcpyAsync(q_idx, d_q, sizeof(int32_t) * k, hipMemcpyDeviceToHost, s), "D2H q");
      chk(hipMemcpyAsync(t_idx, d_t, sizeof(int32_t) * k, hipMemcpyDeviceToHost, s), "D2H t");
      chk(hipMemcpyAsync(dist, d_dist, sizeof(float) * k, hipMemcpyDeviceToHost, s), "D2H d");
      chk(hipStreamSynchronize(s), "sync2");
    }
    *n_out = k;
    if (rc == D2FE_OK && cnt > cap) rc = fail(D2FE_ERR_TRUNCATED, "match output capacity too small");
  }
  return rc;
}

int d2fe_match_knn(d2fe_handle h, const float* a, int na, const float* b, int nb, int dim, double ratio,
                   const float* pts_a, const float* pts_b, double radius, int32_t* q_idx, int32_t* t_idx, float* dist,
                   int cap, int* n_out) {
  return match_host(h, 0, a, na, b, nb, dim, ratio, pts_a, pts_b, radius, q_idx, t_idx, dist, cap, n_out);
}

int d2fe_match_crosscheck(d2fe_handle h, const float* a, int na, const float* b, int nb, int dim, int32_t* q_idx,
                          int32_t* t_idx, float* dist, int cap, int* n_out) {
  return match_host(h, 1, a, na, b, nb, dim, 0.0, nullptr, nullptr, -1.0, q_idx, t_idx, dist, cap, n_out);
}

#ifdef D2FE_DEVTOOLS
/* development builds: the wall_clock64() phase stamps [workgroup][16] of the last d2fe_match_batch_device launch made with D2FE_MATCH_STAMPS set */
D2FE_API long d2fe_debug_match_stamps(d2fe_handle h, unsigned long long* dst, long max_wgs) {
  if (!h || !dst || !h->match.stamps) return fail(D2FE_ERR_NOT_READY, "no stamped launch yet (D2FE_MATCH_STAMPS)");
  hipSetDevice(h->cfg.device_id);
  const long nw = max_wgs < 4096 ? max_wgs : 4096;
  if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(dst, h->match.stamps, sizeof(unsigned long long) * 16 * nw, hipMemcpyDeviceToHost) != hipSuccess)
    return fail(D2FE_ERR_HIP, "D2H");
  return nw;
}
#endif

long d2fe_match_fallback_rows(d2fe_handle h, int reset, long* full_scans) {
  if (!h) return fail(D2FE_ERR_INVALID, "null handle");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  HIP_TRY(hipDeviceSynchronize());
  int32_t v[2] = {0, 0};
  HIP_TRY(hipMemcpy(v, h->match.stats, sizeof(v), hipMemcpyDeviceToHost));
  if (reset) { HIP_TRY(hipMemset(h->match.stats, 0, sizeof(v))); HIP_TRY(hipDeviceSynchronize()); }
  if (full_scans) *full_scans = v[0];
  return v[1];
}

}  // extern "C"
