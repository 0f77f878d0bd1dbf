// loop.hip -- d2fe_loop_*: the loop query of one agent behind a stereo pipe or a quad pipe, inside the library.
// Replaces, per keyframe, what LoopDetector::processImageArray (d2frontend/src/loop_detector.cpp:23-215) does after the tracker: the NetVLAD query of the frame's
// main view (queryImageArrayFromDatabase -> queryIndexFromDatabase, :300-406), the view-by-view matchKNN against the stored keyframe with the direction rotation
// (computeCorrespondFeaturesOnImageArray -> computeCorrespondFeatures -> matchKNN, :443-578) and the add (addImageArrayToDatabase, :228-263), by ONE sequence per ticket:
//
//   device view of the ticket -> ONE loop_search_kernel launch (similarities, causal gate, the matcher's problem table, the per-frame records)
//   -> ONE matcher launch (query side in place in the lane's result block, train side in place in the keyframe store) -> ONE loop_append_kernel launch
//   -> release of the view -> ONE D2H into a pinned slot
//
// on ONE stream of the object's own and without a host synchronisation.  The keyframe store lives on the device: the index [capacity_keyframes * V][dim] with the
// keyframe ordinal and the view of every row (the reference's index_to_frame_id and imgid2dir), the descriptors [capacity_keyframes][V][cap][desc_dim] with their
// counts, and ntotal itself -- which views of a keyframe get an index row (spLandmarkNum() > 0, :233) is decided on the device from n_kp.
//
// Selection.  The reference searches the top min(5 + max_index, ntotal) and returns the first entry with label <= ntotal - max_index and similarity > thres
// (:314-345).  At most max_index - 1 labels are excluded, fewer than the search takes, so that entry is the best row by (similarity descending, label ascending)
// among the rows with label <= ntotal - max_index, if its similarity exceeds thres: a masked arg-max on the order-preserving key db_topk_kernel uses, no top-k
// (tests/test_loop_query_cpu.py holds the two forms to each other and to the oracle).  The similarity arithmetic is db_sims_kernel's, operation by operation.
#include <cstring>
#include <string>
#include <vector>

#include "consumer.h"

using namespace d2fe;

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int LOOP_MAXNQ = 256;                 // frames of one search launch
constexpr int LOOP_WAVES = 8;                   // waves of a search workgroup: every wave holds its rows in registers, the staged queries are shared
constexpr int LOOP_QS_BYTES = 48 * 1024;        // LDS of the staged query chunk

__device__ __forceinline__ float loop_wsum(float v) {      // next.hip's wsum: the reduction order is part of the similarity's bits
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

struct LoopFlags { uint8_t f[LOOP_MAXNQ]; };      // per frame: D2FE_LOOP_QUERY | D2FE_LOOP_ADD (kernel argument: no upload)

struct LoopArgs {
  // the store
  float* db; int32_t* row_kf; int32_t* row_dir; int32_t* d_ntotal;
  float* store_desc; int32_t* store_nkp;
  // the frames, row f * V + v of every array
  const float* q_nv; const float* q_desc; const int32_t* q_nkp;
  int nq, V, main_dir, dim, cap, D, max_index, kf0;
  double thres;
  // launch state, zero between launches
  unsigned long long* best; int32_t* ticket;
  // outputs
  MatchPairDesc* pairs; const int32_t* zero; int32_t* plan;      // plan: [0] ntotal before the ticket, [1] rows the ticket adds, [2 + f * V + v] the row's place among them or -1
  int32_t* o_queried; int32_t* o_label; float* o_sim; int32_t* o_kf; int32_t* o_dir_old; int32_t* o_ntotal;      // [nq]
  int32_t* o_added; int32_t* o_dir_a; int32_t* o_dir_b;      // [nq][V]
};

// One launch for all nq frames of a ticket.  Query j sees the rows [0, ntotal_j): the index as it stood before the ticket and the rows the ticket's earlier frames
// add (read in place in the lane's block: the append kernel copies them behind the matcher), the reference's query-then-add order frame by frame.  The rows are
// streamed once: a wave reads RW rows into registers (NV float4 per lane and row) and walks the queries, which the workgroup stages in LDS chunk by chunk.
template <int NV, int RW>
__global__ __launch_bounds__(64 * LOOP_WAVES) void loop_search_kernel(LoopArgs a, LoopFlags fl) {
  extern __shared__ __align__(16) float qs[];      // [qc][dim]
  __shared__ int s_vslot[LOOP_MAXNQ * 4], s_vlist[LOOP_MAXNQ * 4], s_nt[LOOP_MAXNQ], s_ord[LOOP_MAXNQ], s_qok[LOOP_MAXNQ], s_meta[4];
  __shared__ unsigned long long s_best[LOOP_MAXNQ];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nq = a.nq, V = a.V, dim = a.dim;
  const int ntotal0 = *a.d_ntotal;
  for (int t = tid; t < nq * V; t += blockDim.x) s_vslot[t] = ((fl.f[t / V] & D2FE_LOOP_ADD) && a.q_nkp[t] > 0) ? 1 : 0;
  for (int t = tid; t < nq; t += blockDim.x) s_best[t] = 0ull;
  __syncthreads();
  if (tid == 0) {
    int k = 0, ord = 0;
    for (int f = 0; f < nq; ++f) {
      s_nt[f] = ntotal0 + k; s_ord[f] = ord;
      if (fl.f[f] & D2FE_LOOP_ADD) ++ord;
      for (int v = 0; v < V; ++v) {
        const int t = f * V + v;
        if (s_vslot[t]) { s_vslot[t] = k; s_vlist[k] = t; ++k; } else s_vslot[t] = -1;
      }
    }
    s_meta[0] = k;
  }
  __syncthreads();
  // the caller-side precondition databaseSize() > match_index_dist (:157) and the main view's own landmarks (:378)
  for (int t = tid; t < nq; t += blockDim.x) s_qok[t] = ((fl.f[t] & D2FE_LOOP_QUERY) && a.q_nkp[t * V + a.main_dir] > 0 && s_nt[t] > a.max_index) ? 1 : 0;
  const int nvirt = s_meta[0], total = ntotal0 + nvirt;
  int qc = LOOP_QS_BYTES / (int)(sizeof(float) * dim);
  qc = qc < 1 ? 1 : (qc > nq ? nq : qc);
  __syncthreads();
  for (int base = blockIdx.x * LOOP_WAVES * RW; base < total; base += gridDim.x * LOOP_WAVES * RW) {
    f32x4 rv[RW][NV];
#pragma unroll
    for (int k = 0; k < RW; ++k) {
      const int r = min(base + wave * RW + k, total - 1);      // a row past the end reads the last one (its similarities are never used): every load is unconditional
      const float* rp = r < ntotal0 ? a.db + (size_t)r * dim : a.q_nv + (size_t)s_vlist[r - ntotal0] * dim;
#pragma unroll
      for (int t = 0; t < NV; ++t) {
        const int j = lane * 4 + 256 * t;
        if (256 * (t + 1) <= dim) rv[k][t] = *reinterpret_cast<const f32x4*>(rp + j);      // wave-uniform
        else rv[k][t] = j < dim ? *reinterpret_cast<const f32x4*>(rp + j) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
    for (int c0 = 0; c0 < nq; c0 += qc) {
      const int cn = nq - c0 < qc ? nq - c0 : qc;
      __syncthreads();      // the previous chunk has been read
      for (int i = tid * 4; i < cn * dim; i += 4 * blockDim.x) {
        const int qi = i / dim, j = i - qi * dim;
        *reinterpret_cast<f32x4*>(qs + i) = *reinterpret_cast<const f32x4*>(a.q_nv + (size_t)((c0 + qi) * V + a.main_dir) * dim + j);
      }
      __syncthreads();
      for (int qi = 0; qi < cn; ++qi) {
        const int f = c0 + qi;
        if (!s_qok[f]) continue;
        const int nt = s_nt[f];
        const float* qq = qs + qi * dim;
        if (base + wave * RW >= nt) continue;      // wave-uniform: none of the wave's rows is in this query's range
        float acc[RW];      // db_sims_kernel's chain per (row, query): the lane's elements in ascending j, then the butterfly; a query element is read once for the RW rows
#pragma unroll
        for (int k = 0; k < RW; ++k) acc[k] = 0.f;
#pragma unroll
        for (int t = 0; t < NV; ++t) {
          const int j = lane * 4 + 256 * t;
          if (j < dim) {
            const f32x4 q4 = *reinterpret_cast<const f32x4*>(qq + j);
#pragma unroll
            for (int k = 0; k < RW; ++k) {
              acc[k] = __builtin_fmaf(rv[k][t][0], q4[0], acc[k]); acc[k] = __builtin_fmaf(rv[k][t][1], q4[1], acc[k]);
              acc[k] = __builtin_fmaf(rv[k][t][2], q4[2], acc[k]); acc[k] = __builtin_fmaf(rv[k][t][3], q4[3], acc[k]);
            }
          }
        }
#pragma unroll
        for (int k = 0; k < RW; ++k) {
          const int r = base + wave * RW + k;
          const float sim = loop_wsum(acc[k]);
          if (lane == 0 && r < nt && r <= nt - a.max_index) {
            unsigned b = __float_as_uint(sim);
            b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);      // db_topk_kernel's order-preserving map
            atomicMax(&s_best[f], ((unsigned long long)b << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)r));
          }
        }
      }
    }
  }
  __syncthreads();
  for (int t = tid; t < nq; t += blockDim.x)
    if (s_best[t]) atomicMax(a.best + t, s_best[t]);
  __threadfence();
  __syncthreads();
  if (tid == 0) s_meta[1] = (atomicAdd(a.ticket, 1) == (int)gridDim.x - 1) ? 1 : 0;
  __syncthreads();
  if (!s_meta[1]) return;
  // the workgroup that arrives last: gate, records, the matcher's table, the append kernel's plan
  __threadfence();
  for (int f = tid; f < nq; f += blockDim.x) {
    const unsigned long long key = __hip_atomic_load(a.best + f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(a.best + f, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // ready for the next launch
    int label = -1, kf = -1, dir_old = -1;
    float sim = 0.f;
    if (key && s_qok[f]) {
      const unsigned b = (unsigned)(key >> 32);
      const float s = __uint_as_float((b & 0x80000000u) ? (b & 0x7FFFFFFFu) : ~b);
      if ((double)s > a.thres) {
        label = (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull)); sim = s;
        if (label < ntotal0) { kf = a.row_kf[label]; dir_old = a.row_dir[label]; }
        else { const int t = s_vlist[label - ntotal0]; kf = a.kf0 + s_ord[t / V]; dir_old = t % V; }
      }
    }
    a.o_queried[f] = s_qok[f]; a.o_label[f] = label; a.o_sim[f] = sim; a.o_kf[f] = kf; a.o_dir_old[f] = dir_old; a.o_ntotal[f] = s_nt[f];
    for (int i = 0; i < V; ++i) {
      MatchPairDesc d;
      d.pts_a = nullptr; d.pts_b = nullptr; d.radius = -1.0;
      int da = -1, db = -1;
      if (label >= 0) {
        // computeCorrespondFeaturesOnImageArray (:461-476) with main_dir_a = main_dir, main_dir_b = dir_old
        da = (a.main_dir + i) % V; db = ((dir_old - a.main_dir + V) % V + a.main_dir + i) % V;
        d.a = a.q_desc + (size_t)(f * V + da) * a.cap * a.D; d.na = a.q_nkp + f * V + da;
        if (label < ntotal0) { d.b = a.store_desc + ((size_t)kf * V + db) * a.cap * a.D; d.nb = a.store_nkp + (size_t)kf * V + db; }
        else { const int fo = s_vlist[label - ntotal0] / V; d.b = a.q_desc + (size_t)(fo * V + db) * a.cap * a.D; d.nb = a.q_nkp + fo * V + db; }
      } else {
        d.a = a.store_desc; d.b = a.store_desc; d.na = a.zero; d.nb = a.zero;
      }
      a.pairs[f * V + i] = d; a.o_dir_a[f * V + i] = da; a.o_dir_b[f * V + i] = db;
    }
  }
  for (int t = tid; t < nq * V; t += blockDim.x) { a.plan[2 + t] = s_vslot[t]; a.o_added[t] = s_vslot[t] >= 0 ? ntotal0 + s_vslot[t] : -1; }
  if (tid == 0) { a.plan[0] = ntotal0; a.plan[1] = nvirt; __hip_atomic_store(a.ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
}

// Device-to-device add, behind the matcher: workgroup (f * V + v, part) copies its share of the view's descriptors and, part 0, the count and the view's NetVLAD row
// into the index place the search kernel's plan gave it (frame order, then view order).  ntotal moves once, by workgroup (0, 0).
__global__ __launch_bounds__(256) void loop_append_kernel(LoopArgs a, LoopFlags fl) {
  const int t = blockIdx.x, f = t / a.V, v = t - f * a.V, tid = threadIdx.x;
  if (t == 0 && blockIdx.y == 0 && tid == 0) *a.d_ntotal = a.plan[0] + a.plan[1];
  if (!(fl.f[f] & D2FE_LOOP_ADD)) return;
  int ord = 0;
  for (int g = 0; g < f; ++g) ord += (fl.f[g] & D2FE_LOOP_ADD) ? 1 : 0;
  const size_t kf = (size_t)a.kf0 + ord;
  const int n_raw = a.q_nkp[t], n = n_raw < a.cap ? (n_raw < 0 ? 0 : n_raw) : a.cap;
  const float* src = a.q_desc + (size_t)t * a.cap * a.D;
  float* dst = a.store_desc + (kf * a.V + v) * a.cap * a.D;
  const size_t words = (size_t)n * a.D;
  for (size_t i = (size_t)blockIdx.y * 256 + tid; i < words; i += (size_t)gridDim.y * 256) dst[i] = src[i];
  if (blockIdx.y) return;
  if (tid == 0) a.store_nkp[kf * a.V + v] = n_raw;
  const int slot = a.plan[2 + t];
  if (slot < 0) return;
  const size_t row = (size_t)a.plan[0] + slot;
  const float* g = a.q_nv + (size_t)t * a.dim;
  for (int i = tid; i < a.dim; i += 256) a.db[row * a.dim + i] = g[i];
  if (tid == 0) { a.row_kf[row] = (int32_t)kf; a.row_dir[row] = v; }
}

hipError_t launch_loop_search(const LoopArgs& a, const LoopFlags& fl, long rows_bound, int ncu, hipStream_t s) {
  if (a.nq < 1 || a.nq > LOOP_MAXNQ || a.V < 1 || a.V > 4 || a.dim < 4 || (a.dim & 3) || a.dim > 8192) return hipErrorInvalidValue;
  const int nv = (a.dim + 255) / 256;
  // two rows per wave share every query element read from LDS (dim <= 4096: 2 x 16 float4 per lane; beyond that one row fills the registers).  The grid is what is
  // resident at once -- one workgroup per compute unit at 16 float4 per row and more, two below -- and strides through the rows: every further workgroup costs a
  // prologue and two same-address atomics and adds no load in flight
  const int rw = nv <= 16 ? 2 : 1;
  long nwg = (rows_bound + LOOP_WAVES * rw - 1) / (LOOP_WAVES * rw);
  const long maxwg = (nv <= 4 ? 2L : 1L) * (ncu > 0 ? ncu : 256);
  nwg = nwg < 1 ? 1 : (nwg > maxwg ? maxwg : nwg);
  int qc = LOOP_QS_BYTES / (int)(sizeof(float) * a.dim);
  qc = qc < 1 ? 1 : (qc > a.nq ? a.nq : qc);
  const size_t lds = sizeof(float) * (size_t)qc * a.dim;
  const dim3 grid((unsigned)nwg), block(64 * LOOP_WAVES);
  if (nv <= 1) hipLaunchKernelGGL((loop_search_kernel<1, 2>), grid, block, lds, s, a, fl);
  else if (nv <= 4) hipLaunchKernelGGL((loop_search_kernel<4, 2>), grid, block, lds, s, a, fl);
  else if (nv <= 16) hipLaunchKernelGGL((loop_search_kernel<16, 2>), grid, block, lds, s, a, fl);
  else hipLaunchKernelGGL((loop_search_kernel<32, 1>), grid, block, lds, s, a, fl);
  return hipGetLastError();
}

hipError_t launch_loop_append(const LoopArgs& a, const LoopFlags& fl, hipStream_t s) {
  const long words = (long)a.cap * a.D;
  const int parts = (int)std::min<long>(16, std::max<long>(1, words / 4096));
  hipLaunchKernelGGL(loop_append_kernel, dim3((unsigned)(a.nq * a.V), (unsigned)parts), dim3(256), 0, s, a, fl);
  return hipGetLastError();
}

}  // namespace

struct d2fe_loop_s {
  PipeRef pipe;
  d2fe_handle h = nullptr;
  d2fe_loop_config cfg{};
  int F = 0, V = 1, main_dir = 0, cap = 0, D = 0, G = 0, NQ = 0, lanes = 0;
  long cap_rows = 0;
  // the store
  float* d_db = nullptr; int32_t* d_row_kf = nullptr; int32_t* d_row_dir = nullptr; int32_t* d_state = nullptr;      // d_state: [0] ntotal, [1] the zero word, [2] search ticket
  float* d_store_desc = nullptr; int32_t* d_store_nkp = nullptr;
  unsigned long long* d_best = nullptr;
  int32_t* d_match_scratch = nullptr;
  int keyframes = 0;            // host: exact
  long rows_bound = 0;          // host: upper bound of the device's ntotal
  int64_t last_ticket = -1;
  size_t out_words = 0, o_mq = 0, o_mt = 0, o_md = 0, o_mn = 0, o_queried = 0, o_label = 0, o_sim = 0, o_kf = 0, o_dir_old = 0, o_nt = 0, o_added = 0, o_da = 0, o_db = 0;
  struct Slot : SlotBase { MatchPairDesc* d_pairs = nullptr; int32_t* d_plan = nullptr; int frames = 0; };
  std::vector<Slot> slots;
  hipStream_t st = nullptr;
  hipEvent_t ev_in = nullptr;      // d2fe_loop_query_device: orders the loop's stream behind the producer's
};

namespace {

void loop_destroy(d2fe_loop_s* x) {
  if (!x) return;
  if (x->h) (void)hipSetDevice(x->h->cfg.device_id);
  if (x->st) (void)hipStreamSynchronize(x->st);
  for (auto& S : x->slots) {
    for (void* q : {(void*)S.d_pairs, (void*)S.d_plan}) if (q) (void)hipFree(q);
    S.free();
  }
  for (void* q : {(void*)x->d_db, (void*)x->d_row_kf, (void*)x->d_row_dir, (void*)x->d_state, (void*)x->d_store_desc, (void*)x->d_store_nkp, (void*)x->d_best,
                  (void*)x->d_match_scratch})
    if (q) (void)hipFree(q);
  if (x->ev_in) (void)hipEventDestroy(x->ev_in);
  if (x->st) (void)hipStreamDestroy(x->st);
  delete x;
}

int loop_create(PipeRef pipe, const d2fe_loop_config* cfg_in, d2fe_loop* out) {
  if (!pipe || !cfg_in || !out) return ctx_fail(D2FE_ERR_INVALID, "null argument");
  *out = nullptr;
  d2fe_loop_config cfg;
  d2fe_loop_default_config(&cfg);
  take_config(cfg, cfg_in);
  if (cfg.capacity_keyframes < 1 || cfg.max_index < 0 || cfg.slots < 1 || cfg.slots > 64 || (cfg.mode != 0 && cfg.mode != 1) || cfg.max_queries < 1 || cfg.max_queries > LOOP_MAXNQ)
    return ctx_fail(D2FE_ERR_INVALID, "bad loop configuration");
  int pf = 0, pcap = 0, pdim = 0, pg = 0;
  { const int rc = pipe.geometry(&pf, &pcap, &pdim, &pg); if (rc) return rc; }
  if (pg <= 0) return ctx_fail(D2FE_ERR_INVALID, "the loop query needs the pipe's NetVLAD (netvlad = 1)");
  if (pg & 3) return ctx_fail(D2FE_ERR_UNSUPPORTED, "the NetVLAD length must be a multiple of 4");
  if (pf > LOOP_MAXNQ) return ctx_fail(D2FE_ERR_UNSUPPORTED, "more than 256 frames per pass");
  auto* x = new (std::nothrow) d2fe_loop_s();
  if (!x) return ctx_fail(D2FE_ERR_HIP, "out of memory");
  struct Guard { d2fe_loop_s* x; bool ok = false; ~Guard() { if (!ok) loop_destroy(x); } } guard{x};
  x->pipe = pipe; x->h = pipe.handle(); x->cfg = cfg;
  x->lanes = pipe.lanes();
  x->F = pf; x->cap = pcap; x->D = pdim; x->G = pg;
  x->V = pipe.views(); x->main_dir = x->V == 4 ? 2 : 0;      // camera_index_new of queryImageArrayFromDatabase (:358-371)
  x->NQ = std::max(pf, cfg.max_queries);
  x->cap_rows = (long)cfg.capacity_keyframes * x->V;
  HIP_TRY(hipSetDevice(x->h->cfg.device_id));
  HIP_TRY(hipStreamCreateWithFlags(&x->st, hipStreamNonBlocking));
  HIP_TRY(hipEventCreateWithFlags(&x->ev_in, hipEventDisableTiming));
  const int V = x->V, NQ = x->NQ, NP = NQ * V;
  HIP_TRY(hipMalloc(&x->d_db, sizeof(float) * (size_t)x->cap_rows * pg));
  HIP_TRY(hipMalloc(&x->d_row_kf, sizeof(int32_t) * (size_t)x->cap_rows)); HIP_TRY(hipMalloc(&x->d_row_dir, sizeof(int32_t) * (size_t)x->cap_rows));
  HIP_TRY(hipMalloc(&x->d_state, sizeof(int32_t) * 16)); HIP_TRY(hipMemset(x->d_state, 0, sizeof(int32_t) * 16));
  HIP_TRY(hipMalloc(&x->d_store_desc, sizeof(float) * (size_t)x->cap_rows * pcap * pdim));
  HIP_TRY(hipMalloc(&x->d_store_nkp, sizeof(int32_t) * (size_t)x->cap_rows)); HIP_TRY(hipMemset(x->d_store_nkp, 0, sizeof(int32_t) * (size_t)x->cap_rows));
  HIP_TRY(hipMalloc(&x->d_best, sizeof(unsigned long long) * LOOP_MAXNQ)); HIP_TRY(hipMemset(x->d_best, 0, sizeof(unsigned long long) * LOOP_MAXNQ));
  const size_t msb = match_scratch_bytes(NP, pcap);
  HIP_TRY(hipMalloc(&x->d_match_scratch, msb)); HIP_TRY(hipMemset(x->d_match_scratch, 0, msb));
  size_t o = 0;
  x->o_mq = o; o += up64((size_t)NP * pcap); x->o_mt = o; o += up64((size_t)NP * pcap); x->o_md = o; o += up64((size_t)NP * pcap); x->o_mn = o; o += up64(NP);
  x->o_queried = o; o += up64(NQ); x->o_label = o; o += up64(NQ); x->o_sim = o; o += up64(NQ); x->o_kf = o; o += up64(NQ); x->o_dir_old = o; o += up64(NQ); x->o_nt = o; o += up64(NQ);
  x->o_added = o; o += up64(NP); x->o_da = o; o += up64(NP); x->o_db = o; o += up64(NP);
  x->out_words = o;
  x->slots.resize(cfg.slots);
  for (auto& S : x->slots) {
    { const int rc = S.alloc(x->out_words, x->out_words, cfg.timing != 0); if (rc) return rc; }
    HIP_TRY(hipMalloc(&S.d_pairs, sizeof(MatchPairDesc) * (size_t)NP));
    HIP_TRY(hipMalloc(&S.d_plan, sizeof(int32_t) * (size_t)(2 + NP))); HIP_TRY(hipMemset(S.d_plan, 0, sizeof(int32_t) * (size_t)(2 + NP)));
  }
  HIP_TRY(hipDeviceSynchronize());
  guard.ok = true;
  *out = x;
  return D2FE_OK;
}

// search -> match [-> append] on the loop's stream; the frames' arrays are read in place
int loop_run(d2fe_loop_s* x, d2fe_loop_s::Slot& S, const float* q_nv, const float* q_desc, const int32_t* q_nkp, int nq, int max_index, const LoopFlags& fl, bool append,
             long rows_bound) {
  hipStream_t st = x->st;
  auto mark = [&](int i) { return S.mark(i, st); };
  int32_t* O = reinterpret_cast<int32_t*>(S.d_out);
  LoopArgs a{};
  a.db = x->d_db; a.row_kf = x->d_row_kf; a.row_dir = x->d_row_dir; a.d_ntotal = x->d_state; a.store_desc = x->d_store_desc; a.store_nkp = x->d_store_nkp;
  a.q_nv = q_nv; a.q_desc = q_desc; a.q_nkp = q_nkp;
  a.nq = nq; a.V = x->V; a.main_dir = x->main_dir; a.dim = x->G; a.cap = x->cap; a.D = x->D; a.max_index = max_index; a.kf0 = x->keyframes; a.thres = x->cfg.thres;
  a.best = x->d_best; a.ticket = x->d_state + 2; a.pairs = S.d_pairs; a.zero = x->d_state + 1; a.plan = S.d_plan;
  a.o_queried = O + x->o_queried; a.o_label = O + x->o_label; a.o_sim = S.d_out + x->o_sim; a.o_kf = O + x->o_kf; a.o_dir_old = O + x->o_dir_old; a.o_ntotal = O + x->o_nt;
  a.o_added = O + x->o_added; a.o_dir_a = O + x->o_da; a.o_dir_b = O + x->o_db;
  int r = mark(0); if (r) return r;
  HIP_TRY(launch_loop_search(a, fl, rows_bound, x->h->ncu, st));
  r = mark(1); if (r) return r;
  MatchArgs m{};
  m.pairs = S.d_pairs; m.npairs = nq * x->V; m.dim = x->D; m.max_n = x->cap; m.mode = x->cfg.mode; m.ratio = x->cfg.ratio; m.radius = -1.0;
  match_outputs(m, O + x->o_mq, O + x->o_mt, S.d_out + x->o_md, O + x->o_mn, x->d_match_scratch, x->NQ * x->V, x->h);
  HIP_TRY(launch_match(m, st));
  r = mark(2); if (r) return r;
  if (append) HIP_TRY(launch_loop_append(a, fl, st));
  return mark(3);
}

int loop_finish(d2fe_loop_s* x, d2fe_loop_s::Slot& S, int64_t ticket, int nq) {
  const int rc = S.finish(x->st, x->out_words, 4);
  if (rc) return rc;
  S.ticket = ticket; S.frames = nq;
  return D2FE_OK;
}

}  // namespace

extern "C" {

void d2fe_loop_default_config(d2fe_loop_config* c) {
  if (!c) return;
  memset(c, 0, sizeof(*c));
  c->struct_size = (int32_t)sizeof(*c);
  c->capacity_keyframes = 4096; c->max_index = 10; c->mode = 0; c->slots = 4; c->timing = 0; c->max_queries = 64; c->thres = 0.6; c->ratio = 0.8;
}

int d2fe_loop_create(d2fe_pipe p, const d2fe_loop_config* cfg, d2fe_loop* out) {
  if (!p) return ctx_fail(D2FE_ERR_INVALID, "null argument");
  return loop_create(p, cfg, out);
}
int d2fe_loop_create_quad(d2fe_quad_pipe p, const d2fe_loop_config* cfg, d2fe_loop* out) {
  if (!p) return ctx_fail(D2FE_ERR_INVALID, "null argument");
  return loop_create(p, cfg, out);
}
void d2fe_loop_destroy(d2fe_loop x) { loop_destroy(x); }

int d2fe_loop_enqueue(d2fe_loop x, int64_t ticket, int slot, const uint8_t* is_keyframe, int flags) {
  if (!x || slot < 0 || slot >= (int)x->slots.size() || (flags & ~(D2FE_LOOP_QUERY | D2FE_LOOP_ADD)) || !flags) return ctx_fail(D2FE_ERR_INVALID, "bad argument");
  auto& S = x->slots[slot];
  if (S.busy) return ctx_fail(D2FE_ERR_NOT_READY, "this slot's previous loop query has not been collected");
  if (ticket <= x->last_ticket) return ctx_fail(D2FE_ERR_INVALID, "tickets are enqueued in submit order (the index grows frame by frame)");
  const int F = x->F, V = x->V;
  LoopFlags fl{};
  int adds = 0;
  for (int f = 0; f < F; ++f) {
    fl.f[f] = (uint8_t)((!is_keyframe || is_keyframe[f]) ? flags : 0);
    if (fl.f[f] & D2FE_LOOP_ADD) ++adds;
  }
  if (x->keyframes + adds > x->cfg.capacity_keyframes) return ctx_fail(D2FE_ERR_TRUNCATED, "the keyframe store is full: nothing was queued");
  HIP_TRY(hipSetDevice(x->h->cfg.device_id));
  hipStream_t st = x->st;
  const int rc = with_view(x->pipe, ticket, st, [&](const TicketView& v) -> int {
    if (v.frames != F || v.cap != x->cap || v.desc_dim != x->D || v.netvlad_dim != x->G || !v.d_netvlad)
      return ctx_fail(D2FE_ERR_INVALID, "the pipe's geometry changed under the loop query");
    return loop_run(x, S, v.d_netvlad, v.d_desc, v.d_n_kp, F, x->cfg.max_index, fl, true, x->rows_bound + (long)adds * V);
  });
  if (rc) return rc;
  x->keyframes += adds; x->rows_bound += (long)adds * V; x->last_ticket = ticket;
  return loop_finish(x, S, ticket, F);
}

int d2fe_loop_query_device(d2fe_loop x, const float* d_netvlad, const float* d_desc, const int32_t* d_n_kp, int nq, int max_index, int slot, void* stream) {
  if (!x || !d_netvlad || !d_desc || !d_n_kp || slot < 0 || slot >= (int)x->slots.size() || max_index < 0) return ctx_fail(D2FE_ERR_INVALID, "bad argument");
  if (nq < 1 || nq > x->NQ) return ctx_fail(D2FE_ERR_INVALID, "nq out of range (d2fe_loop_config.max_queries)");
  if (reinterpret_cast<uintptr_t>(d_netvlad) & 15) return ctx_fail(D2FE_ERR_INVALID, "d_netvlad must be 16-byte aligned");
  auto& S = x->slots[slot];
  if (S.busy) return ctx_fail(D2FE_ERR_NOT_READY, "this slot's previous loop query has not been collected");
  HIP_TRY(hipSetDevice(x->h->cfg.device_id));
  if (stream) { HIP_TRY(hipEventRecord(x->ev_in, static_cast<hipStream_t>(stream))); HIP_TRY(hipStreamWaitEvent(x->st, x->ev_in, 0)); }
  LoopFlags fl{};
  for (int f = 0; f < nq; ++f) fl.f[f] = D2FE_LOOP_QUERY;
  const int rc = loop_run(x, S, d_netvlad, d_desc, d_n_kp, nq, max_index, fl, false, x->rows_bound);
  if (rc) return rc;
  return loop_finish(x, S, -1, nq);
}

int d2fe_loop_collect(d2fe_loop x, int slot, d2fe_loop_result* out) {
  if (!x || !out || slot < 0 || slot >= (int)x->slots.size()) return ctx_fail(D2FE_ERR_INVALID, "bad argument");
  auto& S = x->slots[slot];
  if (!S.busy) return ctx_fail(D2FE_ERR_INVALID, "nothing was enqueued on this slot");
  HIP_TRY(hipSetDevice(x->h->cfg.device_id));
  { const int rc = S.collect_begin(); if (rc) return rc; }
  memset(out, 0, sizeof(*out));
  const int32_t* I = reinterpret_cast<const int32_t*>(S.pin);
  out->ticket = S.ticket; out->frames = S.frames; out->views = x->V; out->cap = x->cap;
  out->queried = I + x->o_queried; out->label = I + x->o_label; out->sim = S.pin + x->o_sim; out->keyframe = I + x->o_kf; out->dir_old = I + x->o_dir_old;
  out->ntotal_at_query = I + x->o_nt; out->added_label = I + x->o_added; out->dir_a = I + x->o_da; out->dir_b = I + x->o_db;
  out->n_match = I + x->o_mn; out->q_idx = I + x->o_mq; out->t_idx = I + x->o_mt; out->dist = S.pin + x->o_md;
  S.phase_ms(out->phase_ms, 4);
  return D2FE_OK;
}

int d2fe_loop_ntotal(d2fe_loop x) {
  if (!x) return ctx_fail(D2FE_ERR_INVALID, "null loop");
  HIP_TRY(hipSetDevice(x->h->cfg.device_id));
  int32_t n = 0;
  HIP_TRY(hipMemcpyAsync(&n, x->d_state, sizeof(n), hipMemcpyDeviceToHost, x->st));
  HIP_TRY(hipStreamSynchronize(x->st));
  return n;
}
int d2fe_loop_keyframes(d2fe_loop x) {
  if (!x) return ctx_fail(D2FE_ERR_INVALID, "null loop");
  HIP_TRY(hipSetDevice(x->h->cfg.device_id));
  HIP_TRY(hipStreamSynchronize(x->st));
  return x->keyframes;
}
void* d2fe_loop_stream(d2fe_loop x) { return x ? x->st : nullptr; }

/* keyframes from host memory, in the layout of the device arrays: what the append kernel does for a ticket, as blocking copies (start-up, tests, benchmarks) */
int d2fe_loop_add_host(d2fe_loop x, const float* netvlad, const float* desc, const int32_t* n_kp, int n) {
  if (!x || !netvlad || !n_kp || n < 1) return ctx_fail(D2FE_ERR_INVALID, "bad argument");
  if (x->keyframes + n > x->cfg.capacity_keyframes) return ctx_fail(D2FE_ERR_TRUNCATED, "the keyframe store is full: nothing was added");
  const int V = x->V;
  for (int i = 0; i < n * V; ++i)
    if (n_kp[i] < 0 || (n_kp[i] > 0 && !desc)) return ctx_fail(D2FE_ERR_INVALID, "negative count, or keypoints without descriptors");
  HIP_TRY(hipSetDevice(x->h->cfg.device_id));
  HIP_TRY(hipStreamSynchronize(x->st));
  int32_t ntotal = 0;
  HIP_TRY(hipMemcpy(&ntotal, x->d_state, sizeof(ntotal), hipMemcpyDeviceToHost));
  std::vector<float> rows; std::vector<int32_t> kf, dir;
  const size_t G = (size_t)x->G, blk = (size_t)x->cap * x->D;
  for (int i = 0; i < n; ++i)
    for (int v = 0; v < V; ++v) {
      const size_t t = (size_t)i * V + v, slot = ((size_t)x->keyframes + i) * V + v;
      const int cnt = std::min(n_kp[t], x->cap);
      if (cnt > 0) HIP_TRY(hipMemcpy(x->d_store_desc + slot * blk, desc + t * blk, sizeof(float) * (size_t)cnt * x->D, hipMemcpyHostToDevice));
      if (n_kp[t] > 0) { rows.insert(rows.end(), netvlad + t * G, netvlad + (t + 1) * G); kf.push_back(x->keyframes + i); dir.push_back(v); }
    }
  HIP_TRY(hipMemcpy(x->d_store_nkp + (size_t)x->keyframes * V, n_kp, sizeof(int32_t) * (size_t)n * V, hipMemcpyHostToDevice));
  if (!kf.empty()) {
    HIP_TRY(hipMemcpy(x->d_db + (size_t)ntotal * G, rows.data(), sizeof(float) * rows.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(x->d_row_kf + ntotal, kf.data(), sizeof(int32_t) * kf.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(x->d_row_dir + ntotal, dir.data(), sizeof(int32_t) * dir.size(), hipMemcpyHostToDevice));
    ntotal += (int32_t)kf.size();
    HIP_TRY(hipMemcpy(x->d_state, &ntotal, sizeof(ntotal), hipMemcpyHostToDevice));
  }
  const int first = x->keyframes;
  x->keyframes += n; x->rows_bound += (long)n * V;
  return first;
}

}  // extern "C"
