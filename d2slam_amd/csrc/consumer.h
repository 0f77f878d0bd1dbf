// consumer.h -- what every stage behind a pipe needs (exchange.hip, quad_exchange.hip, loop.hip, window.hip): the pipe it reads from behind ONE type (PipeRef), the
// protocol of a ticket's device view (with_view), the pinned result slot with its events (SlotBase), and the small helpers these stages and the pipes share.
// Everything here goes through the exported d2fe_pipe_* / d2fe_quad_* calls: the pipes' locking and their view bookkeeping stay in pipe.hip and quad_pipe.hip.  Internal.
#pragma once
#include <algorithm>
#include <cstring>

#include "context.h"

namespace d2fe {

inline size_t up64(size_t w) { return (w + 63) / 64 * 64; }      // every array of a block or record starts on a 64-word boundary

// An older caller's shorter struct keeps the defaults `cfg` already holds for the fields it does not know; struct_size <= 0 means the full struct
template <class Cfg>
void take_config(Cfg& cfg, const Cfg* cfg_in) {
  memcpy(&cfg, cfg_in, (size_t)std::min<int32_t>(cfg_in->struct_size > 0 ? cfg_in->struct_size : (int32_t)sizeof(cfg), (int32_t)sizeof(cfg)));
}

// The output side of a matcher launch: the four result arrays, the [tickets | records] scratch carved for `pair_cap` pairs, the counters of `h`; the launch shape is
// sized for `ncu` compute units (0: those of `h`; a pipe passes its lane's share)
inline void match_outputs(MatchArgs& m, int32_t* q_idx, int32_t* t_idx, float* dist, int32_t* n_out, void* scratch, int pair_cap, const d2fe_context* h, int ncu = 0) {
  m.q_idx = q_idx; m.t_idx = t_idx; m.dist = dist; m.n_out = n_out;
  match_scratch_carve(scratch, pair_cap, &m);
  m.stats = h->match.stats; m.ncu = ncu ? ncu : h->ncu;
}

// what d2fe_pipe_device_result and d2fe_quad_device_result share; frames: stereo frames or quad frames, the arrays hold frames * views rows
struct TicketView {
  int frames = 0, cap = 0, desc_dim = 0, netvlad_dim = 0;
  const float *d_kps_xy = nullptr, *d_scores = nullptr, *d_desc = nullptr, *d_netvlad = nullptr;
  const int32_t* d_n_kp = nullptr;
};

// a stereo pipe or a quad pipe: the ONE place that tells them apart
struct PipeRef {
  d2fe_pipe p = nullptr; d2fe_quad_pipe qp = nullptr;
  PipeRef() = default;
  PipeRef(d2fe_pipe p_) : p(p_) {}
  PipeRef(d2fe_quad_pipe qp_) : qp(qp_) {}
  explicit operator bool() const { return p || qp; }
  d2fe_handle handle() const { return p ? d2fe_pipe_handle(p) : d2fe_quad_handle(qp); }
  int lanes() const { return p ? d2fe_pipe_lanes(p) : d2fe_quad_pipe_lanes(qp); }
  int views() const { return p ? 1 : 4; }      // rows per frame of a view's arrays
  int geometry(int* frames, int* cap, int* desc_dim, int* netvlad_dim) const {
    return p ? d2fe_pipe_geometry(p, frames, cap, desc_dim, netvlad_dim) : d2fe_quad_pipe_geometry(qp, frames, cap, desc_dim, netvlad_dim);
  }
  int view(int64_t ticket, hipStream_t st, TicketView* out) const {
    auto take = [&](const auto& v, int frames) {
      out->frames = frames; out->cap = v.cap; out->desc_dim = v.desc_dim; out->netvlad_dim = v.netvlad_dim;
      out->d_kps_xy = v.d_kps_xy; out->d_scores = v.d_scores; out->d_desc = v.d_desc; out->d_netvlad = v.d_netvlad; out->d_n_kp = v.d_n_kp;
    };
    if (p) {
      d2fe_pipe_device_result v{};
      const int rc = d2fe_pipe_device_view(p, ticket, st, &v);
      if (rc == D2FE_OK) take(v, v.frames);
      return rc;
    }
    d2fe_quad_device_result v{};
    const int rc = d2fe_quad_device_view(qp, ticket, st, &v);
    if (rc == D2FE_OK) take(v, v.quads);
    return rc;
  }
  int release(int64_t ticket, hipStream_t st) const { return p ? d2fe_pipe_device_release(p, ticket, st) : d2fe_quad_device_release(qp, ticket, st); }
  int lane_stream(int64_t ticket, void** stream) const { return p ? d2fe_pipe_lane_stream(p, ticket, stream) : d2fe_quad_lane_stream(qp, ticket, stream); }
};

// The view protocol: take the ticket's device view on `st`, run fn(view), release the view WHATEVER fn returned (a block with an outstanding view ends the pipe
// 2 * lanes passes later), and report fn's error before the release's
template <class F>
int with_view(const PipeRef& ref, int64_t ticket, hipStream_t st, F&& fn) {
  TicketView v;
  int rc = ref.view(ticket, st, &v);
  if (rc) return rc;
  rc = fn(v);
  const int rr = ref.release(ticket, st);
  return rc ? rc : rr;
}

// One result slot of a stage: the device record, its pinned copy, the timing events around the phases (only with cfg.timing) and the event behind the D2H.
// A stage's Slot derives from it and adds its own members
struct SlotBase {
  float* d_out = nullptr; float* pin = nullptr;
  hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}; hipEvent_t done = nullptr;
  bool busy = false; int64_t ticket = -1;

  int alloc(size_t dev_words, size_t pin_words, bool timing) {      // both copies zeroed
    HIP_TRY(hipMalloc(&d_out, sizeof(float) * dev_words)); HIP_TRY(hipMemset(d_out, 0, sizeof(float) * dev_words));
    HIP_TRY(hipHostMalloc(&pin, sizeof(float) * pin_words, hipHostMallocDefault));
    memset(pin, 0, sizeof(float) * pin_words);
    if (timing) for (auto& e : ev) HIP_TRY(hipEventCreate(&e));
    HIP_TRY(hipEventCreateWithFlags(&done, hipEventDisableTiming));
    return D2FE_OK;
  }
  void free() {
    if (d_out) (void)hipFree(d_out);
    if (pin) (void)hipHostFree(pin);
    for (auto& e : ev) if (e) (void)hipEventDestroy(e);
    if (done) (void)hipEventDestroy(done);
  }
  // timing mark i of the sequence on `st` (nothing without timing)
  int mark(int i, hipStream_t st) { if (ev[i]) HIP_TRY(hipEventRecord(ev[i], st)); return D2FE_OK; }
  // the end of every sequence: ONE D2H of the record's first d2h_words, the last timing mark, the event collect() waits for
  int finish(hipStream_t st, size_t d2h_words, int last_mark) {
    HIP_TRY(hipMemcpyAsync(pin, d_out, sizeof(float) * d2h_words, hipMemcpyDeviceToHost, st));
    const int rc = mark(last_mark, st);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(done, st));
    busy = true;
    return D2FE_OK;
  }
  // collect(): the pinned record is complete and the slot free again on return
  int collect_begin() {
    HIP_TRY(hipEventSynchronize(done));
    busy = false;
    return D2FE_OK;
  }
  void phase_ms(float* out, int n) const {      // out[i] = ms between marks i and i + 1; left alone without timing
    if (!ev[0]) return;
    for (int i = 0; i < n; ++i) { float ms = 0.f; if (hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess) out[i] = ms; }
  }
};

}  // namespace d2fe
