// lane_ring.h -- the ring of K lanes x 2 result blocks that the stereo pipe (pipe.hip) and the quad pipe (quad_pipe.hip) share: what a lane holds whichever pipe it
// serves, and the pieces of the ring's protocol that do not depend on the pipe -- completion, the device views of a block and their release, the previous pass's block.
// The pipes themselves, their passes, tickets, block layouts and pair tables differ in substance and stay in their files.  Internal.
#pragma once
#include <mutex>
#include <string>

#include "consumer.h"

namespace d2fe {

struct LaneBase {
  d2fe_context* ctx = nullptr;
  hipStream_t s = nullptr, nv = nullptr;
  hipEvent_t ev_up = nullptr, ev_nv = nullptr, ev_ext[2] = {nullptr, nullptr}, ev_done = nullptr;
  // device views of the two result blocks (d2fe_pipe_device_view / d2fe_quad_device_view and their _release): views handed out and not released yet; ev_rel = the
  // consumers' last release
  hipEvent_t ev_rel[2] = {nullptr, nullptr};
  hipEvent_t ev_chain = nullptr;     // sp_lk / track mode: the landmark-list chain of the lane's last pass and the carry copy behind it are complete
  int views[2] = {0, 0};
  bool rel_pending[2] = {false, false};
  uint8_t* pin_in = nullptr;
  float* pin_out[2] = {nullptr, nullptr};
  long long rec = -1, synced = -1;   // the pass whose completion ev_done last recorded / the newest pass known to be complete (idle: synced >= rec)
};

// the previous pass P - 1 of the pass that writes block (k, set).  With P = i K + k the set is i & 1; P - 1 = i K + k - 1 (k > 0: same i) or (i - 1) K + K - 1
struct LaneSet { int k, set; };
inline LaneSet prev_pass_block(int k, int set, int K) { return k > 0 ? LaneSet{k - 1, set} : LaneSet{K - 1, set ^ 1}; }

inline int lane_create_events(LaneBase& L, bool chain) {
  for (hipEvent_t* e : {&L.ev_up, &L.ev_nv, &L.ev_ext[0], &L.ev_ext[1], &L.ev_done, &L.ev_rel[0], &L.ev_rel[1]}) HIP_TRY(hipEventCreateWithFlags(e, hipEventDisableTiming));
  if (chain) HIP_TRY(hipEventCreateWithFlags(&L.ev_chain, hipEventDisableTiming));
  return D2FE_OK;
}

// the lane's half of a pipe's destroy: drains its streams, then gives back what the lane owns (its own stream goes with its context)
inline void lane_destroy(LaneBase& L) {
  if (L.s) (void)hipStreamSynchronize(L.s);
  if (L.nv) { (void)hipStreamSynchronize(L.nv); (void)hipStreamDestroy(L.nv); }
  for (hipEvent_t e : {L.ev_up, L.ev_nv, L.ev_ext[0], L.ev_ext[1], L.ev_done, L.ev_rel[0], L.ev_rel[1], L.ev_chain}) if (e) (void)hipEventDestroy(e);
  if (L.pin_in) (void)hipHostFree(L.pin_in);
  for (float* q : L.pin_out) if (q) (void)hipHostFree(q);
  if (L.ctx) d2fe_destroy(L.ctx);
}

// the end of a pipe's destroy, behind `delete p`: a handle destroyed while this pipe was alive was only MARKED (d2fe_destroy): the last pipe to go releases it
inline void pipe_gone(d2fe_context* parent) {
  if (parent->life.pipe_gone()) d2fe_destroy(parent);
}

inline int lane_sync(LaneBase& L) {       // called with the pipe's mutex held for the whole wait
  if (L.synced < L.rec) {
    HIP_TRY(hipEventSynchronize(L.ev_done));
    L.synced = L.rec;
  }
  return D2FE_OK;
}

// wait() for a lane's pass WITHOUT the mutex, so that the other thread can go on submitting.  The event may be recorded again meanwhile (a later pass of this lane):
// the wait then covers that record too, and everything the lane recorded up to `rec` is complete either way (one stream, in order).  What a failure means for the
// pipe is the caller's policy
inline hipError_t lane_wait_unlocked(LaneBase& L, std::unique_lock<std::mutex>& lk) {
  const long long rec = L.rec;
  hipEvent_t ev = L.ev_done;
  lk.unlock();
  const hipError_t e = hipEventSynchronize(ev);
  lk.lock();
  if (e == hipSuccess && L.synced < rec) L.synced = rec;
  return e;
}

// Before a pass writes block `set` of its lane: device views of this block (handed out 2 K passes ago) must have been released, and the consumers' stream must be
// through with it.  The lane's NetVLAD stream is ordered behind this wait through ev_up.  release_fn / unit: the caller's words for the message
inline int lane_block_guard(LaneBase& L, int set, const char* release_fn, const char* unit) {
  if (L.views[set] > 0)
    return ctx_fail(D2FE_ERR_INVALID, std::string("a device view of this lane's result block was not released (") + release_fn + ") within 2 * lanes " + unit);
  if (L.rel_pending[set]) { HIP_TRY(hipStreamWaitEvent(L.s, L.ev_rel[set], 0)); L.rel_pending[set] = false; }
  return D2FE_OK;
}

// A consumer's stream `cs` takes a view of block `set`.  SuperPoint of the pass: ev_ext[set] (re-recorded only by the pass that rewrites this block, which the caller
// has excluded).  NetVLAD on the lane's second stream (wait_nv): ev_nv -- a later pass of the lane may have re-recorded it; waiting for that later record is merely
// later, never earlier
inline int lane_view_acquire(LaneBase& L, int set, bool wait_nv, hipStream_t cs) {
  HIP_TRY(hipStreamWaitEvent(cs, L.ev_ext[set], 0));
  if (wait_nv) HIP_TRY(hipStreamWaitEvent(cs, L.ev_nv, 0));
  ++L.views[set];
  return D2FE_OK;
}

// Several consumers may share a block (coalesced submits): the event is re-recorded by each release; the lane waits for the last record, and consumers that
// release on DIFFERENT streams must order those streams themselves (documented: one consumer stream per pipe)
inline int lane_view_release(LaneBase& L, int set, hipStream_t cs) {
  if (L.views[set] <= 0) return ctx_fail(D2FE_ERR_INVALID, "no device view of this ticket's block is outstanding");
  HIP_TRY(hipEventRecord(L.ev_rel[set], cs));
  L.rel_pending[set] = true;
  --L.views[set];
  return D2FE_OK;
}

// the landmark-list fields that d2fe_pipe_track_result and d2fe_quad_track_result share, from the list block(s) at `list` in the pinned copy of a result block
template <class Out>
void track_list_view(Out* out, const float* list, int cap_tracks, int desc_dim, size_t list_words) {
  auto at = [&](int field) { return list + d2fe_lk_carry_list_offset(cap_tracks, desc_dim, field); };
  const int32_t* hdr = reinterpret_cast<const int32_t*>(at(D2FE_LKC_HDR));
  out->cap_tracks = cap_tracks; out->desc_dim = desc_dim; out->list_words = (int32_t)list_words;
  out->n = hdr; out->n_tracked_in = hdr + 1; out->n_lost = hdr + 2; out->n_removed_near = hdr + 3; out->n_new = hdr + 4;
  out->pts_xy = at(D2FE_LKC_PTS);
  out->id = reinterpret_cast<const int32_t*>(at(D2FE_LKC_ID)); out->src = reinterpret_cast<const int32_t*>(at(D2FE_LKC_SRC));
  out->kp = reinterpret_cast<const int32_t*>(at(D2FE_LKC_KP));
  out->desc = at(D2FE_LKC_DESC); out->scores = at(D2FE_LKC_SCORES);
}

// the same for the flow-list fields of d2fe_pipe_flow_result and d2fe_quad_flow_result
template <class Out>
void flow_list_view(Out* out, const float* list, int cap_tracks, size_t list_words) {
  const int32_t* hdr = reinterpret_cast<const int32_t*>(list);
  out->cap_tracks = cap_tracks; out->list_words = (int32_t)list_words;
  out->n = hdr; out->n_tracked_in = hdr + 1; out->n_lost = hdr + 2; out->n_removed_near = hdr + 3; out->n_new = hdr + 4;
  out->lack = hdr + 7; out->num = hdr + 8; out->n_cand = hdr + 9;
  out->pts_xy = list + d2fe_lk_flow_list_offset(cap_tracks, D2FE_LKC_PTS);
  out->id = hdr + d2fe_lk_flow_list_offset(cap_tracks, D2FE_LKC_ID);
  out->src = hdr + d2fe_lk_flow_list_offset(cap_tracks, D2FE_LKC_SRC);
}

}  // namespace d2fe
