// quad_exchange.hip -- d2fe_quad_exchange_*: the cross-agent exchange of one quadcam (FOURCORNER_FISHEYE) rank behind the quad pipe, inside the library
// (BASELINE configs[4]; include/d2fe.h has the layout).  Replaces, per remote quad frame, LoopNet::broadcastVisualImageDescArray (d2frontend/src/loop_net.cpp:24-87;
// int8 wire form d2common/include/d2common/d2frontend_types.h:228-268,319-338), the FOURCORNER_FISHEYE branch of D2FeatureTracker::getMatchedPrevKeyframe
// (d2frontend/src/d2featuretracker.cpp:212-233) and the four view pairs of trackRemoteFrames (:282-297) by ONE sequence per submitted ticket:
//
//   d2fe_quad_device_view -> pack_blocks(_int8) of the 4 Q views straight from the lane's result block -> ONE all-gather -> [int8: decode] ->
//   quad_exchange_prepare_kernel (ONE launch: gate, matcher problem table, counter) -> ONE matcher launch (a side in place in the lane's block, b side in place
//   in the gathered blocks) -> d2fe_quad_device_release -> ONE D2H into a pinned slot
//
// d2slam_amd/swarm.py's QuadSwarm does the same over QuadcamChain with torch glue: index_select / copy_ launches for the counts, a memset, the gate launch, a
// snapshot copy of the chain's buffers, and always 16 matcher problems per job (12 of them zeroed in gated mode).  Here the view replaces the snapshot, the
// prepare kernel the glue launches, and gated mode launches the matcher over the 4 tracked problems of a job only.  The structure is exchange.hip's.
#include <cstring>
#include <string>
#include <vector>

#include "exchange_wire.h"

using namespace d2fe;

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f32x4 qx_ld4(const float* p, bool vec) {      // swarm.hip's ld4: 16-byte load where base and stride allow
  if (vec) return *reinterpret_cast<const f32x4*>(p);
  return f32x4{p[0], p[1], p[2], p[3]};
}

struct QuadPrepArgs {
  const float* loc_nv;          // the view's d_netvlad [4 Q][G], null without NetVLAD
  const int32_t* loc_n;         // the view's d_n_kp [4 Q]
  const float* gath;            // gathered fp32 blocks [world][4 Q][blk_words]
  const int32_t* job_rank; const int32_t* job_quad;      // [njobs]
  int njobs, Q, cap, G, blk_words, blk_rows, g_off, n_off, gated, vec_l, vec_r;      // blk_rows: descriptor rows one block spans (blk_words / desc_dim)
  double thres;
  int32_t *a_off, *b_off, *a_cnt, *b_cnt;                // the matcher's problem table [njobs * (16 | 4)]
  int32_t *local_view, *remote_view;                     // [njobs * (16 | 4)]
  int32_t* dir_prev; float* sims; int32_t* gate_n;       // [njobs], [njobs][4], [1]: results (G > 0)
  int32_t* sync;                                         // [2] accumulator, arrival ticket: zero between launches (the last workgroup resets them)
};

// One wave per job = (remote rank r, quad frame q), ONE launch per enqueue.
//   gate: the four dot products of remote view 2 with the local views dirs = {2, 3, 0, 1}, with quad_gate_kernel's arithmetic (swarm.hip): lane l accumulates
//         elements 4 l + 256 i with fmaf in ascending order, xor-shuffle tree 32..1, !((double)s < thres), the first passing j wins -- bit-equal results.
//   table: all2all 16 problems (lv * 4 + rv), nothing zeroed; gated the 4 tracked problems in trackRemoteFrames' order (remote view a = (2 + k) % 4, local
//         view (dir_b - 2 + a) mod 4), counts 0 and views -1 when the gate fails.
//   counter: passing jobs are added to sync[0]; the last workgroup to arrive (sync[1]) stores the sum to *gate_n and zeroes both words for the next launch, so
//         no memset is queued.  Latency-bound (<= 8 Q waves): the point is one launch and no host round trip.
__global__ __launch_bounds__(256) void quad_exchange_prepare_kernel(QuadPrepArgs a) {
  const int job = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const bool active = job < a.njobs;
  if (active) {
    const int r = a.job_rank[job], q = a.job_quad[job];
    const int lrow0 = q * 4, rblk0 = r * 4 * a.Q + q * 4;      // the local rows / the remote rank's blocks of quad frame q, view-minor
    int db = -1;
    if (a.G > 0) {
      const float* r2 = a.gath + (size_t)(rblk0 + 2) * a.blk_words + a.g_off;
      const float* l0 = a.loc_nv + (size_t)lrow0 * a.G;
      float s[4] = {0.f, 0.f, 0.f, 0.f};      // s[j]: local view dirs[j] = (2 + j) & 3
      for (int e = lane * 4; e < a.G; e += 256) {
        const f32x4 y = qx_ld4(r2 + e, a.vec_r != 0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const f32x4 x = qx_ld4(l0 + (size_t)((2 + j) & 3) * a.G + e, a.vec_l != 0);
#pragma unroll
          for (int c = 0; c < 4; ++c) s[j] = __builtin_fmaf(x[c], y[c], s[j]);
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s[j] += __shfl_xor(s[j], o, 64);
#pragma unroll
      for (int j = 3; j >= 0; --j) if (!((double)s[j] < a.thres)) db = (2 + j) & 3;     // the FIRST j that passes wins
      if (lane == 0) {
        a.dir_prev[job] = db;
        a.sims[job * 4 + 0] = s[0]; a.sims[job * 4 + 1] = s[1]; a.sims[job * 4 + 2] = s[2]; a.sims[job * 4 + 3] = s[3];
        if (db >= 0) atomicAdd(a.sync, 1);
      }
    }
    const int ppj = a.gated ? 4 : 16;
    if (lane < ppj) {
      int lv, rv;
      bool on = true;
      if (a.gated) { rv = (2 + lane) & 3; lv = (db - 2 + rv + 4) & 3; on = db >= 0; }
      else { lv = lane >> 2; rv = lane & 3; }
      const size_t p = (size_t)job * ppj + lane;
      const int lrow = lrow0 + (on ? lv : 0), rblk = rblk0 + (on ? rv : 0);
      const int na = a.loc_n[lrow], nb = reinterpret_cast<const int32_t*>(a.gath)[(size_t)rblk * a.blk_words + a.n_off];
      a.a_off[p] = lrow * a.cap;
      a.b_off[p] = rblk * a.blk_rows;
      a.a_cnt[p] = on ? max(0, min(na, a.cap)) : 0;
      a.b_cnt[p] = on ? max(0, min(nb, a.cap)) : 0;
      a.local_view[p] = on ? lv : -1;
      a.remote_view[p] = on ? rv : -1;
    }
  }
  if (a.G > 0) {
    __syncthreads();
    if (threadIdx.x == 0) {
      __threadfence();
      const int t = atomicAdd(a.sync + 1, 1);
      if (t == (int)gridDim.x - 1) {
        __threadfence();
        const int n = atomicAdd(a.sync, 0);      // every passing job's add is ahead of its workgroup's ticket
        *a.gate_n = n;
        // agent-scope (write-through) stores: the words the next launch's atomics meet in L2 are zero whichever XCD this workgroup ran on
        __hip_atomic_store(a.sync, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(a.sync + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
}

}  // namespace

struct d2fe_quad_exchange_s : Wire {
  d2fe_quad_exchange_config cfg{};
  int Q = 0, NJ = 0, PPJ = 16, NP = 0;
  int32_t *d_job_rank = nullptr, *d_job_quad = nullptr;      // the job layout (fixed)
  // one result record: the device copy and the pinned slot share the layout; the words below d2h_words come from the device, the job list behind them is host-written
  size_t out_words = 0, d2h_words = 0, o_mq = 0, o_mt = 0, o_md = 0, o_mn = 0, o_lv = 0, o_rv = 0, o_dir = 0, o_sims = 0, o_np = 0, o_jr = 0, o_jq = 0;
  struct Slot : WireSlot {
    int32_t* d_tab = nullptr;        // a_off | b_off | a_cnt | b_cnt, NP words each, then the prepare kernel's two sync words
  };
  std::vector<Slot> slots;
};

extern "C" {

void d2fe_quad_exchange_default_config(d2fe_quad_exchange_config* c) {
  if (!c) return;
  memset(c, 0, sizeof(*c));
  c->struct_size = (int32_t)sizeof(*c);
  c->world = 1; c->rank = 0; c->wire = D2FE_WIRE_FP32; c->loopback = 0; c->slots = 4; c->own_stream = 1; c->timing = 0; c->mode = D2FE_QUAD_ALL2ALL;
  c->gate_thres = 0.8; c->ratio = 0.8;
}

int d2fe_quad_exchange_job_layout(int world, int rank, int quads, int loopback, int32_t* job_rank, int32_t* job_quad, int cap_jobs) {
  if (world < 1 || rank < 0 || rank >= world || quads < 1 || (long)world * quads > (1L << 20)) return ctx_fail(D2FE_ERR_INVALID, "bad job layout arguments");
  int n = 0;
  for (int r = 0; r < world; ++r) {
    if (r == rank && !loopback) continue;
    for (int q = 0; q < quads; ++q, ++n) {
      if (n >= cap_jobs) continue;
      if (job_rank) job_rank[n] = r;
      if (job_quad) job_quad[n] = q;
    }
  }
  return n;
}

void d2fe_quad_exchange_destroy(d2fe_quad_exchange x) {
  if (!x) return;
  if (x->h) (void)hipSetDevice(x->h->cfg.device_id);
  for (auto& S : x->slots) {
    wire_free_slot(S);
    if (S.d_tab) (void)hipFree(S.d_tab);
  }
  for (void* q : {(void*)x->d_job_rank, (void*)x->d_job_quad})
    if (q) (void)hipFree(q);
  wire_destroy_stream(*x);
  delete x;
}

int d2fe_quad_exchange_create(d2fe_quad_pipe p, void* nccl_comm, const d2fe_quad_exchange_config* cfg_in, d2fe_quad_exchange* out) {
  if (!cfg_in || !out) return ctx_fail(D2FE_ERR_INVALID, "null argument");
  *out = nullptr;
  d2fe_quad_exchange_config cfg;
  d2fe_quad_exchange_default_config(&cfg);
  take_config(cfg, cfg_in);
  // the configuration on its own first: none of these checks needs a pipe or a device
  { const int rc = wire_check_config(cfg, cfg.mode < 0 || cfg.mode > 1, nccl_comm, "quad exchange"); if (rc) return rc; }
  if (!p) return ctx_fail(D2FE_ERR_INVALID, "null argument");
  int pq = 0, pcap = 0, pdim = 0, pg = 0;
  {
    const int rc = d2fe_quad_pipe_geometry(p, &pq, &pcap, &pdim, &pg);
    if (rc) return rc;
  }
  if (cfg.mode == D2FE_QUAD_GATED && pg == 0) return ctx_fail(D2FE_ERR_INVALID, "gated mode needs the pipe's NetVLAD (d2fe_quad_pipe_config.netvlad = 1)");
  if (pdim < 4 || pdim > 256 || (pdim & 3)) return ctx_fail(D2FE_ERR_UNSUPPORTED, "the exchange blocks hold descriptors of 4..256 floats, a multiple of 4");
  if (nccl_comm) { const int rc = rccl_load(nullptr); if (rc) return rc; }
  auto* x = new (std::nothrow) d2fe_quad_exchange_s();
  if (!x) return ctx_fail(D2FE_ERR_HIP, "out of memory");
  struct Guard { d2fe_quad_exchange_s* x; bool ok = false; ~Guard() { if (!ok) d2fe_quad_exchange_destroy(x); } } guard{x};
  x->cfg = cfg; x->Q = pq;
  { const int rc = wire_init(*x, p, nccl_comm, cfg, 4 * pq, pcap, pdim, pg); if (rc) return rc; }
  if ((long)cfg.world * x->NB * x->rows > 0x7fffffffL / 2) return ctx_fail(D2FE_ERR_INVALID, "the gathered buffer exceeds the matcher's 32-bit row offsets");
  HIP_TRY(hipSetDevice(x->h->cfg.device_id));
  x->NJ = d2fe_quad_exchange_job_layout(cfg.world, cfg.rank, pq, cfg.loopback, nullptr, nullptr, 0);
  if (x->NJ < 1) return ctx_fail(D2FE_ERR_INVALID, "no jobs");
  std::vector<int32_t> jr(x->NJ), jq(x->NJ);
  (void)d2fe_quad_exchange_job_layout(cfg.world, cfg.rank, pq, cfg.loopback, jr.data(), jq.data(), x->NJ);
  x->PPJ = cfg.mode == D2FE_QUAD_GATED ? 4 : 16;
  x->NP = x->NJ * x->PPJ;
  const int NJ = x->NJ, NP = x->NP;
  HIP_TRY(hipMalloc(&x->d_job_rank, sizeof(int32_t) * NJ)); HIP_TRY(hipMemcpy(x->d_job_rank, jr.data(), sizeof(int32_t) * NJ, hipMemcpyHostToDevice));
  HIP_TRY(hipMalloc(&x->d_job_quad, sizeof(int32_t) * NJ)); HIP_TRY(hipMemcpy(x->d_job_quad, jq.data(), sizeof(int32_t) * NJ, hipMemcpyHostToDevice));
  size_t o = 0;
  x->o_mq = o; o += up64((size_t)NP * pcap); x->o_mt = o; o += up64((size_t)NP * pcap); x->o_md = o; o += up64((size_t)NP * pcap);
  x->o_mn = o; o += up64(NP); x->o_lv = o; o += up64(NP); x->o_rv = o; o += up64(NP);
  x->o_dir = o; o += up64(NJ); x->o_sims = o; o += up64((size_t)NJ * 4); x->o_np = o; o += 64;
  x->d2h_words = o;
  x->o_jr = o; o += up64(NJ); x->o_jq = o; o += up64(NJ);
  x->out_words = o;
  x->slots.resize(cfg.slots);
  for (auto& S : x->slots) {
    { const int rc = wire_alloc_blocks(*x, S); if (rc) return rc; }
    HIP_TRY(hipMalloc(&S.d_tab, sizeof(int32_t) * (4 * (size_t)NP + 2))); HIP_TRY(hipMemset(S.d_tab, 0, sizeof(int32_t) * (4 * (size_t)NP + 2)));
    { const int rc = S.alloc(x->d2h_words, x->out_words, cfg.timing != 0); if (rc) return rc; }
    memcpy(S.pin + x->o_jr, jr.data(), sizeof(int32_t) * NJ); memcpy(S.pin + x->o_jq, jq.data(), sizeof(int32_t) * NJ);
  }
  if (cfg.own_stream) HIP_TRY(hipStreamCreateWithFlags(&x->own, hipStreamNonBlocking));
  HIP_TRY(hipDeviceSynchronize());
  guard.ok = true;
  *out = x;
  return D2FE_OK;
}

int d2fe_quad_exchange_jobs(d2fe_quad_exchange x) { return x ? x->NJ : ctx_fail(D2FE_ERR_INVALID, "null exchange"); }
int d2fe_quad_exchange_pairs(d2fe_quad_exchange x) { return x ? x->NP : ctx_fail(D2FE_ERR_INVALID, "null exchange"); }
int d2fe_quad_exchange_block_bytes(d2fe_quad_exchange x) { return x ? (x->int8 ? x->BLKB : 4 * x->BLK) : ctx_fail(D2FE_ERR_INVALID, "null exchange"); }
void* d2fe_quad_exchange_stream(d2fe_quad_exchange x) { return x ? x->own : nullptr; }

int d2fe_quad_exchange_gathered(d2fe_quad_exchange x, int slot, const float** d_blocks, const void** d_wire_blocks) {
  if (!x || slot < 0 || slot >= (int)x->slots.size()) return ctx_fail(D2FE_ERR_INVALID, "bad argument");
  return wire_gathered(*x, x->slots[slot], d_blocks, d_wire_blocks);
}

int d2fe_quad_exchange_enqueue(d2fe_quad_exchange x, int64_t ticket, int slot) {
  if (!x || slot < 0 || slot >= (int)x->slots.size()) return ctx_fail(D2FE_ERR_INVALID, "bad argument");
  auto& S = x->slots[slot];
  if (S.busy) return ctx_fail(D2FE_ERR_NOT_READY, "this slot's previous exchange has not been collected");
  HIP_TRY(hipSetDevice(x->h->cfg.device_id));
  hipStream_t st = nullptr;
  { const int rc = wire_stream(*x, ticket, &st); if (rc) return rc; }
  const int rc = with_view(x->pipe, ticket, st, [&](const TicketView& v) -> int {
    if (v.frames != x->Q || v.cap != x->cap || v.desc_dim != x->D || v.netvlad_dim != x->G) return ctx_fail(D2FE_ERR_INVALID, "the pipe's geometry changed under the exchange");
    auto mark = [&](int i) { return S.mark(i, st); };
    int r = mark(0); if (r) return r;
    r = wire_round(*x, S, v, st); if (r) return r;
    const int cap = x->cap, G = x->G;
    int32_t* O = reinterpret_cast<int32_t*>(S.d_out);
    const int NP = x->NP;
    QuadPrepArgs a{};
    a.loc_nv = v.d_netvlad; a.loc_n = v.d_n_kp; a.gath = S.d_gath; a.job_rank = x->d_job_rank; a.job_quad = x->d_job_quad;
    a.njobs = x->NJ; a.Q = x->Q; a.cap = cap; a.G = G; a.blk_words = x->BLK; a.blk_rows = x->rows; a.g_off = x->g_off; a.n_off = x->n_off; a.gated = x->cfg.mode == D2FE_QUAD_GATED ? 1 : 0;
    a.vec_l = G && !((uintptr_t)v.d_netvlad & 15) && !(G & 3) ? 1 : 0;
    a.vec_r = G && !((uintptr_t)(S.d_gath + x->g_off) & 15) && !(x->BLK & 3) ? 1 : 0;
    a.thres = x->cfg.gate_thres;
    a.a_off = S.d_tab; a.b_off = S.d_tab + NP; a.a_cnt = S.d_tab + 2 * (size_t)NP; a.b_cnt = S.d_tab + 3 * (size_t)NP; a.sync = S.d_tab + 4 * (size_t)NP;
    a.local_view = O + x->o_lv; a.remote_view = O + x->o_rv; a.dir_prev = O + x->o_dir; a.sims = S.d_out + x->o_sims; a.gate_n = O + x->o_np;
    hipLaunchKernelGGL(quad_exchange_prepare_kernel, dim3((x->NJ + 3) / 4), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    r = mark(3); if (r) return r;
    d2fe_match_batch mb{};
    mb.d_a = v.d_desc; mb.d_b = S.d_gath; mb.d_a_off = a.a_off; mb.d_b_off = a.b_off; mb.d_a_cnt = a.a_cnt; mb.d_b_cnt = a.b_cnt;
    mb.npairs = NP; mb.dim = x->D; mb.max_n = cap; mb.mode = 0; mb.ratio = x->cfg.ratio; mb.radius = -1.0;
    mb.d_q_idx = O + x->o_mq; mb.d_t_idx = O + x->o_mt; mb.d_dist = S.d_out + x->o_md; mb.d_n_out = O + x->o_mn;
    r = d2fe_match_batch_device(x->h, &mb, st); if (r) return r;
    return mark(4);
  });
  if (rc) return rc;
  { const int r = S.finish(st, x->d2h_words, 5); if (r) return r; }
  S.ticket = ticket;
  return D2FE_OK;
}

int d2fe_quad_exchange_collect(d2fe_quad_exchange x, int slot, d2fe_quad_exchange_result* out) {
  if (!x || !out || slot < 0 || slot >= (int)x->slots.size()) return ctx_fail(D2FE_ERR_INVALID, "bad argument");
  auto& S = x->slots[slot];
  if (!S.busy) return ctx_fail(D2FE_ERR_INVALID, "nothing was enqueued on this slot");
  HIP_TRY(hipSetDevice(x->h->cfg.device_id));
  { const int rc = S.collect_begin(); if (rc) return rc; }
  memset(out, 0, sizeof(*out));
  const int32_t* I = reinterpret_cast<const int32_t*>(S.pin);
  out->ticket = S.ticket; out->njobs = x->NJ; out->npairs = x->NP; out->pairs_per_job = x->PPJ; out->cap = x->cap;
  out->job_rank = I + x->o_jr; out->job_quad = I + x->o_jq;
  out->q_idx = I + x->o_mq; out->t_idx = I + x->o_mt; out->dist = S.pin + x->o_md; out->n_match = I + x->o_mn;
  out->local_view = I + x->o_lv; out->remote_view = I + x->o_rv;
  out->dir_prev = x->G ? I + x->o_dir : nullptr; out->gate_sims = x->G ? S.pin + x->o_sims : nullptr; out->gate_n = x->G ? I[x->o_np] : 0;
  S.phase_ms(out->phase_ms, 5);
  return D2FE_OK;
}

}  // extern "C"
