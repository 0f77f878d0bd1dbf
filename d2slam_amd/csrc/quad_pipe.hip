// quad_pipe.hip -- quadcam frames in flight: d2fe_quad_pipe_* of include/d2fe.h (BASELINE configs[2], FOURCORNER_FISHEYE).
//
// The quadcam per-frame work that d2slam_amd/quadcam.py's QuadcamChain sequences from Python (four undistort launches, torch.index_select of the pair
// counts, a torch copy of the previous views, two matcher launches, one stream, one step at a time) as the stereo pipe's lanes (pipe.hip).  A submit =
// Q quad frames = one pass on lane P % K, on the lane's own streams:
//     ONE H2D of the 4 Q raw frames -> quad_undistort_kernel (4 cameras x Q frames in ONE launch, quad-major views) -> [NetVLAD of the 4 Q views on the
//     lane's second stream] -> SuperPoint of the 4 Q views -> half_compact_kernel over the 8 Q neighbour jobs -> ONE matcher launch over the 4 Q neighbour
//     pairs and the 4 Q temporal pairs (pair tables per lane and result block: the temporal pairs of quad frame 0 read the previous pass's block in place)
//     -> remap_matches_kernel of the neighbour pairs -> ONE D2H of the result block into pinned memory.
// Only the undistort launch is new device code; extraction, NetVLAD, compaction, matcher and remap are the kernels the single calls launch.  Result blocks,
// tickets and their lifetime are the stereo pipe's with one submit per pass: two blocks per lane, a ticket's block is written again 2 K passes later.
//
// d2fe_quad_track_enable (sp_lk: enable_lk_optical_flow + sp_track_use_lk of the reference's quadcam tracker, trackLocalFrames d2featuretracker.cpp:121-133): behind the
// pass's SuperPoint the lane builds the pyramids of its 4 Q views, then the landmark lists (lk_carry.hip) are stepped once per quad frame -- ONE launch for the four
// cameras, d2fe_lk_carry_quad_step_device.  The lists are a chain across quad frames, passes and lanes: quad frame 0 of a pass reads the last four lists of the
// previous pass in that pass's result block and its four pyramids from d_carry_pyr, which the previous pass copied there on its own stream; the lane's ev_chain,
// recorded behind the copy, is what the next pass's first step waits for (pipe.hip's scheme).  ONE launch then tracks the list entries of every neighbour pair
// (d2fe_lk_carry_neighbour_device), and the lists go through the half-image compaction (reading the list blocks in place), ONE matcher launch and the remap, like the
// keypoints.  The mode's arrays are appended to the result block in front of d2h_words, so they travel in the pass's one D2H; a pipe that never enables the mode
// keeps the layout and the allocations it had.
//
// d2fe_quad_flow_enable (flow_lk: enable_lk_optical_flow without sp_track_use_lk, the reference's config/quadcam/quadcam_single.yaml, quadcam_multi.yaml and
// quadcam_multi_rt.yaml; excludes the mode above): the same pyramids and the same chain, but the lists are the FLOW lists of lk_flow.hip -- per quad frame ONE
// d2fe_lk_flow_quad_step_device (five launches for the four cameras) on the keypoints of that quad frame, with ONE pipe-owned detector scratch of four cameras that all
// lanes share because the chain serialises the steps -- and ONE d2fe_lk_flow_neighbour_device over the pass's lists.  No matchKNN of the lists: flow entries carry no
// descriptors.  The lists and the neighbour tracks sit where sp_lk puts its own (o_list, o_nbxy, o_nbst), in front of d2h_words.
//
// d2fe_quad_bearings_enable (with or without one of the two modes above, in any order): ONE bearings_kernel launch (bearings.hip) per pass behind the neighbour LK
// launch and in front of the matcher -- the unit bearings of the 4 Q keypoint rows and, with lists, of the 4 Q lists, the prediction of every list entry through its
// neighbour pair's extrinsic, the bearings of the neighbour tracks and the lk_lk_use_pred gate.  Its arrays are the last ones in front of d2h_words: the lists' arrays
// keep the offsets they have without it.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "lane_ring.h"

using namespace d2fe;

namespace {

// ---- the undistort step: 4 cameras x Q raw frames in ONE launch ---------------------------------------------------------------------------------------
// undistort_kernel (next.hip) is one pixel per thread and one launch per camera, and every image of a launch re-reads the 12 B/pixel of map and gain.  Here
// a workgroup owns a tile of QU_TILE pixels of ONE camera's maps, loads mapx / mapy / gain once (16 B per lane and array) and writes that tile of every quad
// frame of the pass, 4 output bytes per lane and frame.  The arithmetic is undistort_kernel's operation for operation (the same bilinear weights in the
// same order, zero outside the frame, both saturate_cast roundings; the library is built with -ffp-contract=off): the same bytes, which
// tests/test_quad_pipe.py checks against d2fe_undistort_device.  HBM bytes of a launch: the maps once (4 cameras x 8 or 12 B per pixel), the raw taps
// (neighbouring lanes' taps share cache lines: at most the raw frames once) and 1 B per pixel and view out -- tools/bench_quad_pipe.py counts them.
constexpr int QU_THREADS = 256, QU_PX = 4, QU_TILE = QU_THREADS * QU_PX;
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct QuadUndistortArgs {
  const uint8_t* raw; long cam_stride, quad_stride; int sh, sw, sstride;
  const float* mapx[4]; const float* mapy[4]; const float* gain[4];      // gain[c] may be null
  int npix, quads, vec_out;                                               // vec_out: every view starts 4-byte aligned (npix % 4 == 0, aligned dst)
  uint8_t* dst;                                                           // view (q, c) at dst + (q * 4 + c) * npix
};

__device__ __forceinline__ unsigned qu_sat_u8(float v) {   // saturate_cast<uchar>(float): round-to-nearest-even, clamp (next.hip: sat_u8)
  if (!(v > 0.f)) return 0u;
  if (v >= 255.f) return 255u;
  return (unsigned)__builtin_rintf(v);
}

// cv::remap(INTER_LINEAR, BORDER_CONSTANT 0) of one pixel + the first rounding: undistort_kernel's expression
__device__ __forceinline__ unsigned qu_remap(const uint8_t* __restrict__ s, int sh, int sw, int sstride, float x, float y) {
  const int x1 = (int)__builtin_floorf(x), y1 = (int)__builtin_floorf(y), x2 = x1 + 1, y2 = y1 + 1;
  auto S = [&](int yy, int xx) -> float {
    return (yy >= 0 && yy < sh && xx >= 0 && xx < sw) ? (float)s[(size_t)yy * sstride + xx] : 0.f;
  };
  float out = 0.f;
  out = out + S(y1, x1) * (((float)x2 - x) * ((float)y2 - y));
  out = out + S(y1, x2) * ((x - (float)x1) * ((float)y2 - y));
  out = out + S(y2, x1) * (((float)x2 - x) * (y - (float)y1));
  out = out + S(y2, x2) * ((x - (float)x1) * (y - (float)y1));
  return qu_sat_u8(out);
}

__global__ __launch_bounds__(QU_THREADS) void quad_undistort_kernel(QuadUndistortArgs a) {
  const int c = blockIdx.y;
  const int i0 = (blockIdx.x * QU_THREADS + threadIdx.x) * QU_PX;
  if (i0 >= a.npix) return;
  const float* __restrict__ mx = a.mapx[c];
  const float* __restrict__ my = a.mapy[c];
  const float* __restrict__ mg = a.gain[c];
  const int m = min(QU_PX, a.npix - i0);
  float x[QU_PX], y[QU_PX], g[QU_PX];
  if (m == QU_PX) {      // the maps are 16-byte aligned (d2fe_quad_undistort_device checks; the pipe's own maps come from hipMalloc)
    const f32x4 vx = *reinterpret_cast<const f32x4*>(mx + i0), vy = *reinterpret_cast<const f32x4*>(my + i0);
    const f32x4 vg = mg ? *reinterpret_cast<const f32x4*>(mg + i0) : f32x4{1.f, 1.f, 1.f, 1.f};
#pragma unroll
    for (int k = 0; k < QU_PX; ++k) { x[k] = vx[k]; y[k] = vy[k]; g[k] = vg[k]; }
  } else {
#pragma unroll
    for (int k = 0; k < QU_PX; ++k) {
      x[k] = k < m ? mx[i0 + k] : 0.f; y[k] = k < m ? my[i0 + k] : 0.f; g[k] = mg && k < m ? mg[i0 + k] : 1.f;
    }
  }
  for (int q = 0; q < a.quads; ++q) {
    const uint8_t* s = a.raw + q * a.quad_stride + c * a.cam_stride;
    uint8_t* d = a.dst + ((size_t)q * 4 + c) * a.npix + i0;
    unsigned u[QU_PX];
#pragma unroll
    for (int k = 0; k < QU_PX; ++k) {
      u[k] = qu_remap(s, a.sh, a.sw, a.sstride, x[k], y[k]);
      if (mg) u[k] = qu_sat_u8((float)u[k] * g[k]);
    }
    if (m == QU_PX && a.vec_out) *reinterpret_cast<uint32_t*>(d) = u[0] | (u[1] << 8) | (u[2] << 16) | (u[3] << 24);
    else for (int k = 0; k < m; ++k) d[k] = (uint8_t)u[k];
  }
}

hipError_t launch_quad_undistort(const QuadUndistortArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(quad_undistort_kernel, dim3((a.npix + QU_TILE - 1) / QU_TILE, 4), dim3(QU_THREADS), 0, s, a);
  return hipGetLastError();
}

constexpr int NB[4][3] = {{0, 1, 1}, {1, 2, 1}, {2, 3, 1}, {0, 3, 2}};     // quadcam.NEIGHBOURS: (view a, view b, type) 1 LEFT_RIGHT, 2 RIGHT_LEFT

}  // namespace

struct d2fe_quad_pipe_s {
  d2fe_context* parent = nullptr;
  d2fe_quad_pipe_config cfg{};
  int K = 0, Q = 0, NI = 0, RW = 0, RH = 0, W = 0, H = 0, cap = 0, D = 256, G = 0;
  int n_nb = 0, n_pr = 0, NP = 0;      // neighbour pairs, temporal pairs, all pairs of a pass (neighbour pairs first)
  float move_cols = 0.f;
  // result block (float words from its base; every array starts on a 64-word boundary); the words below d2h_words go to the host
  size_t o_desc = 0, o_kps = 0, o_scores = 0, o_nv = 0, o_cnt = 0, o_mn = 0, o_mq = 0, o_mt = 0, o_md = 0, o_idx = 0, blk_words = 0, d2h_words = 0;
  // lane scratch (float words): the undistorted views and the half-image jobs' pools, read only by the lane's own pass
  size_t x_und = 0, x_jdesc = 0, x_jpts = 0, x_jmap = 0, x_jn = 0, scr_words = 0;
  float* d_all = nullptr;              // [64 zero words | K lanes x 2 sets x block]
  float* d_scr = nullptr;              // [K][scr_words]
  uint8_t* d_raw_all = nullptr;        // [K][4 Q raw frames], quad-major, tight rows
  float* d_maps = nullptr;             // [4 cameras][mapx | mapy | gain], W * H floats each
  int32_t* d_jobs = nullptr;           // job_row [8 Q] | job_left [8 Q] | job_shift (float) [8 Q] | map_a_job [4 Q] | map_b_job [4 Q]
  MatchPairDesc* d_pairs = nullptr;    // [K][2][NP]
  int32_t* d_match_scratch = nullptr; size_t match_scratch_lane = 0;
  QuadUndistortArgs ua{};              // everything but the lane's raw frames and views
  // d2fe_quad_track_enable: per pass 4 Q list blocks at o_list (list (q, c) at (q * 4 + c) * list_words), the neighbour tracks [4 Q][capT][2] floats and [4 Q][capT]
  // bytes, the list matches (o_lm*), all inside d2h_words.  Lane scratch of the mode (float words from tscratch(k)): the half-image pools of the lists
  bool trk = false;
  bool trk_split = false;              // D2FE_QUAD_TRACK_SPLIT of the development library: four single-camera steps per quad frame (a measurement, not an option)
  d2fe_track_params tp{};
  int capT = 0;
  size_t list_words = 0, pyr_total = 0;
  size_t o_list = 0, o_nbxy = 0, o_nbst = 0, o_lmn = 0, o_lmq = 0, o_lmt = 0, o_lmd = 0;
  size_t t_jdesc = 0, t_jpts = 0, t_jmap = 0, t_jn = 0, tscr_words = 0;
  float* d_trk = nullptr;              // [4 empty lists | 64 words: next_id | K lanes x tscr_words]
  uint8_t* d_trk_pyr = nullptr;        // [4 carried pyramids | K lanes x 4 Q pyramids], pyr_total bytes each
  MatchPairDesc* d_lpairs = nullptr;   // [K][4 Q]: the neighbour pairs of the lists, on the lane's pools
  // d2fe_quad_flow_enable: 4 Q flow-list blocks at o_list and the neighbour tracks at o_nbxy / o_nbst (capT = max(total_feature_num, 1)); d_trk is [4 empty lists | 64
  // words: next_id], d_trk_pyr as above.  trk and flow exclude each other
  bool flow = false;
  bool flow_split = false;             // D2FE_QUAD_FLOW_SPLIT of the development library: four single-camera steps per quad frame (a measurement, not an option)
  d2fe_flow_params fp{};
  uint8_t* d_flow_scratch = nullptr;   // [4 cameras][flow_scratch_stride]: score map, candidate pool and count of each camera
  size_t flow_scratch_stride = 0;
  int32_t* d_lmatch_scratch = nullptr; size_t lmatch_scratch_lane = 0;
  // d2fe_quad_bearings_enable: doubles [4 Q][cap][3] of the keypoint rows and, with lists, doubles [4 Q][capT][3] of the list entries, per neighbour pair the
  // predictions floats [4 Q][capT][2], the neighbour tracks' bearings doubles [4 Q][capT][3] and the gate bytes [4 Q][capT] -- behind the lists' arrays (lists_end),
  // inside d2h_words.  base_words: d2h_words of the pipe as created, where the lists' arrays start
  bool bear = false;
  BearCams bcams{};
  size_t base_words = 0, lists_end = 0;
  size_t o_bkb = 0, o_blb = 0, o_bnp = 0, o_bnb = 0, o_bno = 0;
  struct Lane : LaneBase { uint8_t* d_raw = nullptr; };
  std::vector<Lane> lanes;
  std::vector<int> first_class, second_class;
  int n_classes = 0; long long probe_ticks = 0; double probe_turns_us = 0.0;
  std::mutex mu;                       // submit() and wait() may come from different threads; wait() drops it while it blocks
  long long next_ticket = 0;           // one submit = one pass: ticket == pass
  int failed = D2FE_OK;                // sticky: the first error of an enqueue leaves a pass half-queued
  std::string failed_msg;
  float* block(int lane, int set) const { return d_all + 64 + ((size_t)lane * 2 + set) * blk_words; }
  float* scratch(int lane) const { return d_scr + (size_t)lane * scr_words; }
  float* tscratch(int lane) const { return d_trk + 4 * list_words + 64 + (size_t)lane * tscr_words; }
  int32_t* next_id() const { return reinterpret_cast<int32_t*>(d_trk + 4 * list_words); }
  uint8_t* carry_pyr() const { return d_trk_pyr; }
  uint8_t* lane_pyr(int lane) const { return d_trk_pyr + (4 + (size_t)lane * NI) * pyr_total; }
};

namespace {

// the matcher's pair tables of the keypoints; they hold addresses inside the result blocks (d2fe_quad_track_enable moves those and fills the table again)
void quad_fill_pairs(const d2fe_quad_pipe_s* p, std::vector<MatchPairDesc>& tab) {
  const size_t cap = p->cap, D = p->D, NP = p->NP;
  const int Q = p->Q;
  const d2fe_quad_pipe_config* cfg = &p->cfg;
  // pair tables [lane][set][NP]: the 4 Q neighbour pairs on the lane's compacted pools, then the 4 Q temporal pairs (view c of quad frame q against view c
  // of quad frame q - 1; q = 0: the last quad frame of the previous pass P - 1 = lane k - 1 of the same set, or lane K - 1 of the other set when k = 0)
  tab.assign((size_t)p->K * 2 * NP, MatchPairDesc{});
  for (int k = 0; k < p->K; ++k)
    for (int set = 0; set < 2; ++set) {
      float* B = p->block(k, set);
      const auto [pk, pset] = prev_pass_block(k, set, p->K);
      float* PB = p->block(pk, pset);
      float* X = p->scratch(k);
      MatchPairDesc* row = tab.data() + ((size_t)k * 2 + set) * NP;
      int pi = 0;
      for (int j = 0; p->n_nb && j < 4 * Q; ++j) {
        MatchPairDesc& d = row[pi++];
        const size_t ja = 2 * (size_t)j, jb = ja + 1;
        d.a = X + p->x_jdesc + ja * cap * D; d.b = X + p->x_jdesc + jb * cap * D;
        d.pts_a = X + p->x_jpts + ja * cap * 2; d.pts_b = X + p->x_jpts + jb * cap * 2;
        d.na = reinterpret_cast<int32_t*>(X + p->x_jn) + ja; d.nb = reinterpret_cast<int32_t*>(X + p->x_jn) + jb;
        d.radius = cfg->radius_neighbour;
      }
      for (int v = 0; p->n_pr && v < 4 * Q; ++v) {
        MatchPairDesc& d = row[pi++];
        float* BB = v >= 4 ? B : PB;
        const size_t ra = v, rb = v >= 4 ? v - 4 : (size_t)(4 * (Q - 1) + v);
        d.a = B + p->o_desc + ra * cap * D; d.b = BB + p->o_desc + rb * cap * D;
        d.pts_a = B + p->o_kps + ra * cap * 2; d.pts_b = BB + p->o_kps + rb * cap * 2;
        d.na = reinterpret_cast<int32_t*>(B + p->o_cnt) + ra; d.nb = reinterpret_cast<int32_t*>(BB + p->o_cnt) + rb;
        d.radius = cfg->radius_prev;
      }
    }
}

// the bearings' arrays from word o on (T = 0: no lists); a double = two words, every array on a 64-word boundary, so the doubles are 8-byte aligned
struct QuadBearLayout { size_t o_bkb, o_blb, o_bnp, o_bnb, o_bno, end; };
QuadBearLayout quad_bear_layout(size_t o, size_t NI, size_t cap, size_t T) {
  QuadBearLayout b{};
  o = up64(o);
  b.o_bkb = o; o += up64(NI * cap * 6);
  if (T) {
    b.o_blb = o; o += up64(NI * T * 6);
    b.o_bnp = o; o += up64(NI * T * 2);
    b.o_bnb = o; o += up64(NI * T * 6);
    b.o_bno = o; o += up64((NI * T + 3) / 4);
  }
  b.end = o;
  return b;
}

// the keypoints' pair table holds addresses inside the result blocks: filled again when they have moved.  A failure here is final, like a failed submit
int quad_refill_pairs(d2fe_quad_pipe_s* p) {
  if (!p->NP) return D2FE_OK;
  std::vector<MatchPairDesc> tab;
  quad_fill_pairs(p, tab);
  if (hipMemcpy(p->d_pairs, tab.data(), sizeof(MatchPairDesc) * tab.size(), hipMemcpyHostToDevice) != hipSuccess) {
    p->failed = D2FE_ERR_HIP; p->failed_msg = "hipMemcpy of the pair table";
    return ctx_fail(D2FE_ERR_HIP, p->failed_msg);
  }
  return D2FE_OK;
}

// What d2fe_quad_track_enable and d2fe_quad_flow_enable share (called with the pipe's mutex held, before the first submit): the mode's arrays in the result blocks,
// everything the mode owns on the device and the host, and the pair tables that address the moved blocks.  The caller sets its mode flags when this returns D2FE_OK or
// has set p->failed
struct QuadListMode {
  int cap;                 // slots of a list block (capT)
  size_t list_words;       // words of a list block
  size_t pyr_total;        // bytes of a view's pyramid
  bool matches;            // sp_lk: the list matches (o_lm*, d_lpairs, d_lmatch_scratch) and the lanes' half-image pools of the lists (t_j*)
  size_t fast_scratch;     // flow: bytes of one camera's detector scratch (0: none)
};
int quad_lists_enable(d2fe_quad_pipe_s* p, const QuadListMode& m) {
  const int Q = p->Q, K = p->K;
  const size_t T = (size_t)m.cap, D = (size_t)p->D, NI = (size_t)p->NI, NJ = 8 * (size_t)Q, lw = m.list_words, pyr_total = m.pyr_total;
  // the mode's arrays go between the keypoint results and d2h_words: every earlier offset stays, the bearings' arrays (if they are on already) and the extraction's
  // index scratch (o_idx) move behind them
  size_t o = p->base_words;
  const size_t o_list = o; o += NI * lw;
  const size_t o_nbxy = o; o += up64(NI * T * 2);
  const size_t o_nbst = o; o += up64((NI * T + 3) / 4);
  size_t o_lmn = 0, o_lmq = 0, o_lmt = 0, o_lmd = 0, t_jdesc = 0, t_jpts = 0, t_jmap = 0, t_jn = 0, t = 0;
  if (m.matches) {
    o_lmn = o; o += up64(NI);
    o_lmq = o; o += up64(NI * T);
    o_lmt = o; o += up64(NI * T);
    o_lmd = o; o += up64(NI * T);
    t_jdesc = t; t += up64(NJ * T * D);
    t_jpts = t; t += up64(NJ * T * 2);
    t_jmap = t; t += up64(NJ * T);
    t_jn = t; t += up64(NJ);
  }
  const size_t lists_end = o;
  QuadBearLayout bl{};
  if (p->bear) { bl = quad_bear_layout(o, NI, (size_t)p->cap, T); o = bl.end; }
  const size_t d2h_words = o, o_idx = o, blk_words = o + up64(NI * (size_t)p->cap), tscr_words = t;
  // everything new first; the pipe changes only when all of it is there
  struct Fresh {
    float* d_all = nullptr; float* d_trk = nullptr; uint8_t* d_pyr = nullptr; MatchPairDesc* d_lpairs = nullptr; int32_t* d_lms = nullptr; uint8_t* d_scr = nullptr;
    std::vector<float*> pin; std::vector<hipEvent_t> ev; bool keep = false;
    ~Fresh() {
      if (keep) return;
      for (void* q : {(void*)d_all, (void*)d_trk, (void*)d_pyr, (void*)d_lpairs, (void*)d_lms, (void*)d_scr}) if (q) (void)hipFree(q);
      for (float* q : pin) if (q) (void)hipHostFree(q);
      for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    }
  } f;
  const size_t all_words = 64 + (size_t)K * 2 * blk_words, trk_words = 4 * lw + 64 + (size_t)K * tscr_words;
  const size_t pyr_bytes = (4 + (size_t)K * NI) * pyr_total, lms_lane = m.matches ? match_scratch_bytes(4 * Q, m.cap) : 0;
  HIP_TRY(hipMalloc(&f.d_all, sizeof(float) * all_words));
  HIP_TRY(hipMemset(f.d_all, 0, sizeof(float) * all_words));        // no keypoints, empty lists, every arrival counter zero
  HIP_TRY(hipMalloc(&f.d_trk, sizeof(float) * trk_words));
  HIP_TRY(hipMemset(f.d_trk, 0, sizeof(float) * trk_words));        // the four empty lists in front of the first quad frame, next_id = 0
  HIP_TRY(hipMalloc(&f.d_pyr, pyr_bytes));
  HIP_TRY(hipMemset(f.d_pyr, 0, pyr_bytes));
  if (m.fast_scratch) HIP_TRY(hipMalloc(&f.d_scr, 4 * m.fast_scratch));      // its content between steps does not matter
  f.pin.assign((size_t)2 * K, nullptr); f.ev.assign((size_t)K, nullptr);
  for (int i = 0; i < 2 * K; ++i) HIP_TRY(hipHostMalloc(&f.pin[i], sizeof(float) * d2h_words, hipHostMallocDefault));
  for (int k = 0; k < K; ++k) HIP_TRY(hipEventCreateWithFlags(&f.ev[k], hipEventDisableTiming));
  if (m.matches) {      // the neighbour pairs of the lists, on the lanes' pools
    HIP_TRY(hipMalloc(&f.d_lpairs, sizeof(MatchPairDesc) * (size_t)K * 4 * Q));
    HIP_TRY(hipMalloc(&f.d_lms, lms_lane * K));
    HIP_TRY(hipMemset(f.d_lms, 0, lms_lane * K));
    std::vector<MatchPairDesc> lt((size_t)K * 4 * Q);
    for (int k = 0; k < K; ++k) {
      float* X = f.d_trk + 4 * lw + 64 + (size_t)k * tscr_words;
      for (int j = 0; j < 4 * Q; ++j) {
        MatchPairDesc& d = lt[(size_t)k * 4 * Q + j];
        const size_t ja = 2 * (size_t)j, jb = ja + 1;
        d.a = X + t_jdesc + ja * T * D; d.b = X + t_jdesc + jb * T * D;
        d.pts_a = X + t_jpts + ja * T * 2; d.pts_b = X + t_jpts + jb * T * 2;
        d.na = reinterpret_cast<int32_t*>(X + t_jn) + ja; d.nb = reinterpret_cast<int32_t*>(X + t_jn) + jb;
        d.radius = p->cfg.radius_neighbour;
      }
    }
    HIP_TRY(hipMemcpy(f.d_lpairs, lt.data(), sizeof(MatchPairDesc) * lt.size(), hipMemcpyHostToDevice));
  }
  HIP_TRY(hipDeviceSynchronize());        // the memsets ran on the null stream, which the lanes' streams do not wait for
  // ---- commit: nothing has been submitted, so no stream holds an address of the old blocks
  f.keep = true;
  (void)hipFree(p->d_all);
  p->d_all = f.d_all; p->d_trk = f.d_trk; p->d_trk_pyr = f.d_pyr; p->d_lpairs = f.d_lpairs; p->d_lmatch_scratch = f.d_lms; p->lmatch_scratch_lane = lms_lane;
  p->d_flow_scratch = f.d_scr; p->flow_scratch_stride = m.fast_scratch;
  for (int k = 0; k < K; ++k) {
    auto& L = p->lanes[k];
    for (int set = 0; set < 2; ++set) { (void)hipHostFree(L.pin_out[set]); L.pin_out[set] = f.pin[(size_t)2 * k + set]; }
    L.ev_chain = f.ev[k];
  }
  p->capT = m.cap; p->list_words = lw; p->pyr_total = pyr_total;
  p->o_list = o_list; p->o_nbxy = o_nbxy; p->o_nbst = o_nbst; p->o_lmn = o_lmn; p->o_lmq = o_lmq; p->o_lmt = o_lmt; p->o_lmd = o_lmd;
  p->lists_end = lists_end;
  if (p->bear) { p->o_bkb = bl.o_bkb; p->o_blb = bl.o_blb; p->o_bnp = bl.o_bnp; p->o_bnb = bl.o_bnb; p->o_bno = bl.o_bno; }
  p->d2h_words = d2h_words; p->o_idx = o_idx; p->blk_words = blk_words;
  p->t_jdesc = t_jdesc; p->t_jpts = t_jpts; p->t_jmap = t_jmap; p->t_jn = t_jn; p->tscr_words = tscr_words;
  return quad_refill_pairs(p);
}

// d2fe_quad_bearings_enable with the pipe's mutex held, before the first submit: the bearings' arrays behind the lists' (or the keypoint results), new blocks and new
// pinned copies of the larger d2h_words; the pipe changes only when all of it is there
int quad_bear_blocks(d2fe_quad_pipe_s* p) {
  const int K = p->K;
  const size_t NI = (size_t)p->NI;
  const QuadBearLayout bl = quad_bear_layout(p->lists_end, NI, (size_t)p->cap, p->trk || p->flow ? (size_t)p->capT : 0);
  const size_t d2h_words = bl.end, blk_words = bl.end + up64(NI * (size_t)p->cap), all_words = 64 + (size_t)K * 2 * blk_words;
  struct Fresh {
    float* d_all = nullptr; std::vector<float*> pin; bool keep = false;
    ~Fresh() {
      if (keep) return;
      if (d_all) (void)hipFree(d_all);
      for (float* q : pin) if (q) (void)hipHostFree(q);
    }
  } f;
  HIP_TRY(hipMalloc(&f.d_all, sizeof(float) * all_words));
  HIP_TRY(hipMemset(f.d_all, 0, sizeof(float) * all_words));        // as the blocks it replaces: no keypoints, empty lists, every arrival counter zero
  f.pin.assign((size_t)2 * K, nullptr);
  for (int i = 0; i < 2 * K; ++i) HIP_TRY(hipHostMalloc(&f.pin[i], sizeof(float) * d2h_words, hipHostMallocDefault));
  HIP_TRY(hipDeviceSynchronize());        // the memset ran on the null stream, which the lanes' streams do not wait for
  f.keep = true;
  (void)hipFree(p->d_all);
  p->d_all = f.d_all;
  for (int k = 0; k < K; ++k)
    for (int set = 0; set < 2; ++set) { (void)hipHostFree(p->lanes[k].pin_out[set]); p->lanes[k].pin_out[set] = f.pin[(size_t)2 * k + set]; }
  p->o_bkb = bl.o_bkb; p->o_blb = bl.o_blb; p->o_bnp = bl.o_bnp; p->o_bnb = bl.o_bnb; p->o_bno = bl.o_bno;
  p->d2h_words = d2h_words; p->o_idx = d2h_words; p->blk_words = blk_words;
  return quad_refill_pairs(p);
}

// one submit: H2D, undistort, NetVLAD beside SuperPoint, compaction, ONE matcher launch, remap, ONE D2H -- all on the lane's streams
int quad_pass(d2fe_quad_pipe_s* p, const uint8_t* raw, int stride, size_t cam_stride, size_t quad_stride, int64_t* ticket) {
  const long long P = p->next_ticket;
  const int k = (int)(P % p->K), set = (int)((P / p->K) & 1);
  auto& L = p->lanes[k];
  // the lane's previous pass (P - K) must be complete before its input, staging and scratch are reused.  The result block this pass writes was last read
  // by pass P - 2 K + 1 (its temporal pairs), which is complete too: the submit of pass P - K + 1 synchronised with it
  int rc = lane_sync(L);
  if (rc) return rc;
  rc = lane_block_guard(L, set, "d2fe_quad_device_release", "submits");
  if (rc) return rc;
  const size_t rimg = (size_t)p->RW * p->RH, img = (size_t)p->W * p->H;
  const int Q = p->Q, NI = p->NI, W = p->W, H = p->H, RW = p->RW, RH = p->RH;
  hipStream_t s = L.s;
  // 1. the raw frames -> the lane's input buffer, quad-major and tight: ONE DMA unless pinned input comes in scattered images
  const bool tight = stride == RW && cam_stride == rimg && quad_stride == 4 * rimg;
  if (p->cfg.pinned_input) {
    if (tight) HIP_TRY(hipMemcpyAsync(L.d_raw, raw, rimg * NI, hipMemcpyHostToDevice, s));
    else if (cam_stride == (size_t)stride * RH && quad_stride == 4 * cam_stride)
      HIP_TRY(hipMemcpy2DAsync(L.d_raw, RW, raw, stride, RW, (size_t)RH * NI, hipMemcpyHostToDevice, s));
    else
      for (int q = 0; q < Q; ++q)
        for (int c = 0; c < 4; ++c)
          HIP_TRY(hipMemcpy2DAsync(L.d_raw + (size_t)(q * 4 + c) * rimg, RW, raw + q * quad_stride + c * cam_stride, stride, RW, RH, hipMemcpyHostToDevice, s));
  } else {
    if (tight) memcpy(L.pin_in, raw, rimg * NI);
    else
      for (int q = 0; q < Q; ++q)
        for (int c = 0; c < 4; ++c) {
          const uint8_t* src = raw + q * quad_stride + c * cam_stride;
          uint8_t* dst = L.pin_in + (size_t)(q * 4 + c) * rimg;
          if (stride == RW) memcpy(dst, src, rimg);
          else for (int y = 0; y < RH; ++y) memcpy(dst + (size_t)y * RW, src + (size_t)y * stride, RW);
        }
    HIP_TRY(hipMemcpyAsync(L.d_raw, L.pin_in, rimg * NI, hipMemcpyHostToDevice, s));
  }
  float* B = p->block(k, set);
  float* X = p->scratch(k);
  uint8_t* und = reinterpret_cast<uint8_t*>(X + p->x_und);
  int32_t* cnt = reinterpret_cast<int32_t*>(B + p->o_cnt);
  // 2. the 4 Q views in ONE launch
  QuadUndistortArgs ua = p->ua;
  ua.raw = L.d_raw; ua.dst = und;
  HIP_TRY(launch_quad_undistort(ua, s));
  // 3-4. SuperPoint on the lane's stream, NetVLAD beside it on the lane's second stream (the stereo pipe's netvlad_inline = 0); SuperPoint is issued first:
  // it is the long pole of a pass
  const bool nv = p->G > 0;
  if (nv) HIP_TRY(hipEventRecord(L.ev_up, s));
  rc = run_superpoint(L.ctx, und, NI, W, H, W, img, B + p->o_kps, B + p->o_scores, B + p->o_desc, reinterpret_cast<int32_t*>(B + p->o_idx), p->cap, cnt, s);
  if (rc) return rc;
  HIP_TRY(hipEventRecord(L.ev_ext[set], s));
  if (nv) {
    HIP_TRY(hipStreamWaitEvent(L.nv, L.ev_up, 0));
    rc = run_netvlad(L.ctx, und, NI, W, H, W, img, B + p->o_nv, L.nv);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(L.ev_nv, L.nv));
  }
  const int32_t* job_row = p->d_jobs;
  const int32_t* job_left = job_row + 8 * Q;
  const float* job_shift = reinterpret_cast<const float*>(job_left + 8 * Q);
  const int32_t* map_a = job_left + 16 * Q;
  const int32_t* map_b = map_a + 4 * Q;
  int32_t* jmap = reinterpret_cast<int32_t*>(X + p->x_jmap);
  if (p->trk || p->flow) {
    // the pyramids of the pass's 4 Q views (view i of the lane's scratch = image i of the workspace), then the landmark lists: ONE step per quad frame in time order,
    // the carry copy, ONE launch for the neighbour tracks of every list
    const d2fe_track_params& tp = p->flow ? p->fp.track : p->tp;
    uint8_t* pyr = p->lane_pyr(k);
    rc = d2fe_lk_track_stereo_device(L.ctx, und, und + (size_t)2 * Q * img, 2 * Q, W, H, W, img, nullptr, nullptr, 0, tp.levels, tp.win, tp.iters, pyr, nullptr,
                                     nullptr, s);
    if (rc) return rc;
    const auto [pk, pset] = prev_pass_block(k, set, p->K);
    if (P > 0 && p->K > 1) HIP_TRY(hipStreamWaitEvent(s, p->lanes[pk].ev_chain, 0));
    float* lists = B + p->o_list;
    for (int q = 0; q < Q; ++q) {
      // the predecessor: the quad frame before in this pass; q = 0: the last quad frame of the previous pass (its block, the carried pyramids); the very first quad
      // frame reads four empty lists and tracks nothing
      const float* prev_lists = q > 0 ? lists + (size_t)(q - 1) * 4 * p->list_words : P > 0 ? p->block(pk, pset) + p->o_list + (size_t)(Q - 1) * 4 * p->list_words : p->d_trk;
      const uint8_t* prev_pyr = q > 0 ? pyr + (size_t)(q - 1) * 4 * p->pyr_total : p->carry_pyr();
      const size_t r = (size_t)q * 4;
      if (p->trk_split) {        // development library only (tools/bench_quad_pipe_sp_lk.py): the chain composed from four single-camera launches, the same bits
        for (int c = 0; c < 4 && !rc; ++c)
          rc = d2fe_lk_carry_step_device(L.ctx, prev_pyr + c * p->pyr_total, pyr + (r + c) * p->pyr_total, W, H, prev_lists + c * p->list_words,
                                         lists + (r + c) * p->list_words, p->D, B + p->o_kps + (r + c) * p->cap * 2, B + p->o_scores + (r + c) * p->cap,
                                         B + p->o_desc + (r + c) * p->cap * p->D, cnt + r + c, p->cap, &p->tp, p->next_id(), s);
        if (rc) return rc;
        continue;
      }
      if (p->flow && p->flow_split) {      // development library only (tools/bench_quad_pipe_flow.py): the chain composed from four single-camera steps, the same bits
        for (int c = 0; c < 4 && !rc; ++c)
          rc = d2fe_lk_flow_step_device(L.ctx, prev_pyr + c * p->pyr_total, pyr + (r + c) * p->pyr_total, W, H, prev_lists + c * p->list_words,
                                        lists + (r + c) * p->list_words, B + p->o_kps + (r + c) * p->cap * 2, cnt + r + c, p->cap, &p->fp, p->next_id(),
                                        p->d_flow_scratch + c * p->flow_scratch_stride, s);
      } else if (p->flow) {
        rc = d2fe_lk_flow_quad_step_device(L.ctx, prev_pyr, pyr + r * p->pyr_total, p->pyr_total, W, H, prev_lists, lists + r * p->list_words, p->list_words,
                                           B + p->o_kps + r * p->cap * 2, cnt + r, p->cap, &p->fp, p->next_id(), p->d_flow_scratch, p->flow_scratch_stride, s);
      } else {
        rc = d2fe_lk_carry_quad_step_device(L.ctx, prev_pyr, pyr + r * p->pyr_total, p->pyr_total, W, H, prev_lists, lists + r * p->list_words, p->list_words, p->D,
                                            B + p->o_kps + r * p->cap * 2, B + p->o_scores + r * p->cap, B + p->o_desc + r * p->cap * p->D, cnt + r, p->cap, &p->tp,
                                            p->next_id(), s);
      }
      if (rc) return rc;
    }
    HIP_TRY(hipMemcpyAsync(p->carry_pyr(), pyr + (size_t)(Q - 1) * 4 * p->pyr_total, 4 * p->pyr_total, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipEventRecord(L.ev_chain, s));
    rc = p->flow ? d2fe_lk_flow_neighbour_device(L.ctx, pyr, p->pyr_total, Q, W, H, p->cfg.undistort_fov, lists, p->list_words, &tp, B + p->o_nbxy,
                                                 reinterpret_cast<uint8_t*>(B + p->o_nbst), s)
                 : d2fe_lk_carry_neighbour_device(L.ctx, pyr, p->pyr_total, Q, W, H, p->cfg.undistort_fov, lists, p->list_words, p->D, &p->tp, B + p->o_nbxy,
                                                  reinterpret_cast<uint8_t*>(B + p->o_nbst), s);
    if (rc) return rc;
  }
  if (p->bear) {
    // the bearings of the pass's keypoint rows and list entries, the neighbour predictions and their gates: ONE launch over 4 Q lists per segment; row / list
    // (q, c) takes camera c, pair (q, n) the list of its camera a, cameras a and b and extrinsic n
    const size_t cap = (size_t)p->cap, T = (size_t)p->capT;
    BearSeg seg[3];
    int ns = 0;
    BearSeg& kp = seg[ns++];
    kp = BearSeg{};
    kp.pts = B + p->o_kps; kp.pts_stride = cap * 2; kp.n = cnt; kp.n_stride = 1; kp.cap = p->cap; kp.by4 = 1;
    for (int c = 0; c < 4; ++c) { kp.cam[c] = (unsigned char)c; kp.src[c] = (unsigned char)c; }
    kp.bearing = reinterpret_cast<double*>(B + p->o_bkb); kp.bearing_step = 1;
    if (p->trk || p->flow) {
      const float* lists = B + p->o_list;
      BearSeg& tl = seg[ns++];
      tl = kp;
      tl.pts = lists + (p->flow ? d2fe_lk_flow_list_offset(p->capT, D2FE_LKC_PTS) : d2fe_lk_carry_list_offset(p->capT, p->D, D2FE_LKC_PTS)); tl.pts_stride = p->list_words;
      tl.n = reinterpret_cast<const int32_t*>(lists + (p->flow ? 0 : d2fe_lk_carry_list_offset(p->capT, p->D, D2FE_LKC_HDR))); tl.n_stride = p->list_words;
      tl.cap = p->capT;
      tl.bearing = reinterpret_cast<double*>(B + p->o_blb);
      BearSeg& nb = seg[ns++];
      nb = tl;
      for (int n = 0; n < 4; ++n) { nb.cam[n] = nb.src[n] = (unsigned char)NB[n][0]; nb.ocam[n] = (unsigned char)NB[n][1]; nb.ext[n] = (unsigned char)n; }
      nb.bearing = nullptr; nb.pred = B + p->o_bnp;
      nb.other = B + p->o_nbxy; nb.other_stride = T * 2; nb.status = reinterpret_cast<const uint8_t*>(B + p->o_nbst); nb.status_stride = T;
      nb.other_bearing = reinterpret_cast<double*>(B + p->o_bnb); nb.pred_ok = reinterpret_cast<uint8_t*>(B + p->o_bno);
    }
    rc = bearings_launch(L.ctx, p->bcams, NI, seg, ns, s);
    if (rc) return rc;
  }
  if (p->trk) {
    float* lists = B + p->o_list;
    // matchLocalFeatures on the lists: the compaction reads the list blocks in place (descriptors, points and count of list r are r * list_words further on), the
    // same jobs and shifts as the keypoints'; ONE matcher launch over the 4 Q pairs, then the remap
    float* T = p->tscratch(k);
    int32_t* tmap = reinterpret_cast<int32_t*>(T + p->t_jmap);
    HIP_TRY(launch_half_compact_strided(lists + d2fe_lk_carry_list_offset(p->capT, p->D, D2FE_LKC_DESC), lists + d2fe_lk_carry_list_offset(p->capT, p->D, D2FE_LKC_PTS),
                                        reinterpret_cast<const int32_t*>(lists), p->list_words, p->list_words, p->list_words, job_row, job_left, job_shift, 8 * Q, p->capT,
                                        p->D, (float)W, p->move_cols, T + p->t_jdesc, T + p->t_jpts, tmap, reinterpret_cast<int32_t*>(T + p->t_jn), s));
    MatchArgs m{};
    m.pairs = p->d_lpairs + (size_t)k * 4 * Q;
    m.npairs = 4 * Q; m.dim = p->D; m.max_n = p->capT; m.mode = 0; m.ratio = p->cfg.ratio; m.radius = -1.0;
    match_outputs(m, reinterpret_cast<int32_t*>(B + p->o_lmq), reinterpret_cast<int32_t*>(B + p->o_lmt), B + p->o_lmd, reinterpret_cast<int32_t*>(B + p->o_lmn),
                  reinterpret_cast<char*>(p->d_lmatch_scratch) + p->lmatch_scratch_lane * k, 4 * Q, p->parent, L.ctx->ncu);
    HIP_TRY(launch_match(m, s));
    HIP_TRY(launch_remap_matches(m.q_idx, m.t_idx, m.n_out, map_a, map_b, tmap, 4 * Q, p->capT, p->capT, s));
  }
  // 5. getFeatureHalfImg of both views of every neighbour pair + the a-side shift
  if (p->n_nb)
    HIP_TRY(launch_half_compact(B + p->o_desc, B + p->o_kps, cnt, job_row, job_left, job_shift, 8 * Q, p->cap, p->D, (float)W, p->move_cols, X + p->x_jdesc,
                                X + p->x_jpts, jmap, reinterpret_cast<int32_t*>(X + p->x_jn), s));
  // 6. ONE matcher launch over the neighbour and the temporal pairs (the counts are read where compaction and extraction wrote them)
  if (p->NP) {
    if (p->n_pr && P > 0 && p->K > 1) {      // the temporal pairs of quad frame 0 read the previous pass's block: wait for ITS extraction only
      const auto [pk, pset] = prev_pass_block(k, set, p->K);
      HIP_TRY(hipStreamWaitEvent(s, p->lanes[pk].ev_ext[pset], 0));
    }
    MatchArgs m{};
    m.pairs = p->d_pairs + ((size_t)k * 2 + set) * p->NP;
    m.npairs = p->NP; m.dim = p->D; m.max_n = p->cap; m.mode = 0; m.ratio = p->cfg.ratio; m.radius = -1.0;
    match_outputs(m, reinterpret_cast<int32_t*>(B + p->o_mq), reinterpret_cast<int32_t*>(B + p->o_mt), B + p->o_md, reinterpret_cast<int32_t*>(B + p->o_mn),
                  reinterpret_cast<char*>(p->d_match_scratch) + p->match_scratch_lane * k, p->NP, p->parent, L.ctx->ncu);
    HIP_TRY(launch_match(m, s));
  }
  // 7. neighbour indices back into the full view lists, then ONE D2H
  if (p->n_nb)
    HIP_TRY(launch_remap_matches(reinterpret_cast<int32_t*>(B + p->o_mq), reinterpret_cast<int32_t*>(B + p->o_mt), reinterpret_cast<int32_t*>(B + p->o_mn), map_a,
                                 map_b, jmap, p->n_nb, p->cap, p->cap, s));
  if (nv) HIP_TRY(hipStreamWaitEvent(s, L.ev_nv, 0));
  HIP_TRY(hipMemcpyAsync(L.pin_out[set], B, sizeof(float) * p->d2h_words, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipEventRecord(L.ev_done, s));
  L.rec = P;
  p->next_ticket = P + 1;
  *ticket = P;
  return D2FE_OK;
}

}  // namespace

extern "C" {

void d2fe_quad_pipe_default_config(d2fe_quad_pipe_config* c) {
  memset(c, 0, sizeof(*c));
  c->struct_size = (int32_t)sizeof(d2fe_quad_pipe_config);
  c->lanes = 4; c->quads = 1; c->raw_width = 1280; c->raw_height = 800; c->width = 800; c->height = 400; c->cap = 100;
  c->netvlad = 1; c->match_neighbour = 1; c->match_prev = 1; c->pinned_input = 0;
  c->ratio = 0.8; c->radius_neighbour = 0.2 * 800; c->radius_prev = -1.0; c->undistort_fov = 200.0;
}

int d2fe_quad_undistort_device(d2fe_handle h, const uint8_t* d_raw, int quads, int sw, int sh, int sstride, size_t camera_stride, size_t quad_stride,
                               const d2fe_quad_maps* maps, int dw, int dh, uint8_t* d_dst, void* stream) {
  if (!h || !d_raw || !maps || !d_dst) return ctx_fail(D2FE_ERR_INVALID, "null argument");
  if (!maps->device) return ctx_fail(D2FE_ERR_INVALID, "d2fe_quad_undistort_device takes device maps (maps->device = 1)");
  if (quads < 1 || sw < 1 || sh < 1 || sstride < sw || dw < 1 || dh < 1 || (long)dw * dh > (1L << 30)) return ctx_fail(D2FE_ERR_INVALID, "bad geometry");
  QuadUndistortArgs a{};
  for (int c = 0; c < 4; ++c) {
    if (!maps->mapx[c] || !maps->mapy[c]) return ctx_fail(D2FE_ERR_INVALID, "maps: mapx / mapy of every camera");
    if (((uintptr_t)maps->mapx[c] | (uintptr_t)maps->mapy[c] | (uintptr_t)maps->gain[c]) & 15) return ctx_fail(D2FE_ERR_INVALID, "maps must be 16-byte aligned");
    a.mapx[c] = maps->mapx[c]; a.mapy[c] = maps->mapy[c]; a.gain[c] = maps->gain[c];
  }
  a.raw = d_raw; a.cam_stride = (long)camera_stride; a.quad_stride = (long)quad_stride; a.sh = sh; a.sw = sw; a.sstride = sstride;
  a.npix = dw * dh; a.quads = quads; a.vec_out = (a.npix % 4 == 0 && ((uintptr_t)d_dst & 3) == 0) ? 1 : 0; a.dst = d_dst;
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  HIP_TRY(launch_quad_undistort(a, stream ? (hipStream_t)stream : h->stream));
  return D2FE_OK;
}

int d2fe_quad_pipe_create(d2fe_handle h, const d2fe_quad_pipe_config* cfg, const d2fe_quad_maps* maps, d2fe_quad_pipe* out) {
  if (!h || !cfg || !maps || !out) return ctx_fail(D2FE_ERR_INVALID, "null argument");
  *out = nullptr;
  if (cfg->struct_size != (int32_t)sizeof(d2fe_quad_pipe_config)) return ctx_fail(D2FE_ERR_INVALID, "d2fe_quad_pipe_config size mismatch");
  if (const char* why = sp_not_ready(h)) return ctx_fail(D2FE_ERR_NOT_READY, why);
  if (cfg->netvlad && !h->nv_net) return ctx_fail(D2FE_ERR_NOT_READY, "netvlad weights not loaded");
  if (cfg->lanes < 1 || cfg->lanes > 16 || cfg->quads < 1) return ctx_fail(D2FE_ERR_INVALID, "lanes must be 1..16, quads >= 1");
  if (4L * cfg->quads > h->cfg.max_batch) return ctx_fail(D2FE_ERR_INVALID, "4 * quads views exceed the handle's max_batch");
  if (h->cfg.max_keypoints < 0) return ctx_fail(D2FE_ERR_UNSUPPORTED, "keep-all handles (max_keypoints = -1) are served by the single-call entry points");
  if (cfg->cap < 1 || cfg->cap > h->cfg.max_keypoints) return ctx_fail(D2FE_ERR_INVALID, "cap must be 1..the handle's max_keypoints");
  if (cfg->match_neighbour && cfg->cap > 1024) return ctx_fail(D2FE_ERR_INVALID, "neighbour matching takes cap <= 1024 (the half-image compaction)");
  if (cfg->raw_width < 1 || cfg->raw_height < 1) return ctx_fail(D2FE_ERR_INVALID, "raw frame size");
  if (cfg->width > h->cfg.max_width || cfg->height > h->cfg.max_height) return ctx_fail(D2FE_ERR_INVALID, "view size exceeds the handle's maximum");
  if (((long)cfg->width * cfg->height) % 4) return ctx_fail(D2FE_ERR_INVALID, "width * height must be a multiple of 4 (the maps' 16-byte loads)");
  if (cfg->match_neighbour && !(cfg->undistort_fov > 0.0)) return ctx_fail(D2FE_ERR_INVALID, "undistort_fov must be > 0");
  for (int c = 0; c < 4; ++c)
    if (!maps->mapx[c] || !maps->mapy[c]) return ctx_fail(D2FE_ERR_INVALID, "maps: mapx / mapy of every camera");
  const int NI = 4 * cfg->quads;
  int rc = check_geometry(h, NI, cfg->width, cfg->height, cfg->width, cfg->cap);
  if (rc) return rc;
  if (cfg->netvlad && (rc = nv_check(h, NI, cfg->width, cfg->height, cfg->width)) != D2FE_OK) return rc;
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  d2fe_quad_pipe_s* p = new d2fe_quad_pipe_s();
  p->parent = h; p->cfg = *cfg;
  h->life.pipe_added();        // the stereo pipes' accounting: d2fe_quad_pipe_destroy (every failure path below goes through it) gives it back
  p->K = cfg->lanes; p->Q = cfg->quads; p->NI = NI; p->RW = cfg->raw_width; p->RH = cfg->raw_height; p->W = cfg->width; p->H = cfg->height;
  p->cap = cfg->cap; p->D = d2fe_desc_dim(h); p->G = cfg->netvlad ? d2fe_netvlad_dim(h) : 0;
  p->n_nb = cfg->match_neighbour ? 4 * p->Q : 0; p->n_pr = cfg->match_prev ? 4 * p->Q : 0; p->NP = p->n_nb + p->n_pr;
  p->move_cols = d2fe_half_move_cols(p->W, cfg->undistort_fov);
  const size_t cap = p->cap, D = p->D, img = (size_t)p->W * p->H, NJ = 8 * (size_t)p->Q, NP = p->NP;
  size_t o = 0;
  p->o_desc = o; o += up64(NI * cap * D);
  p->o_kps = o; o += up64(NI * cap * 2);
  p->o_scores = o; o += up64(NI * cap);
  p->o_nv = o; o += up64(NI * (size_t)p->G);
  p->o_cnt = o; o += up64(NI);
  p->o_mn = o; o += up64(NP);
  p->o_mq = o; o += up64(NP * cap);
  p->o_mt = o; o += up64(NP * cap);
  p->o_md = o; o += up64(NP * cap);
  p->d2h_words = p->base_words = p->lists_end = o;
  p->o_idx = o; o += up64(NI * cap);
  p->blk_words = o;
  o = 0;
  p->x_und = o; o += up64((NI * img + 3) / 4);
  p->x_jdesc = o; o += up64(p->n_nb ? NJ * cap * D : 0);
  p->x_jpts = o; o += up64(p->n_nb ? NJ * cap * 2 : 0);
  p->x_jmap = o; o += up64(p->n_nb ? NJ * cap : 0);
  p->x_jn = o; o += up64(p->n_nb ? NJ : 0);
  p->scr_words = o;
  rc = [&]() -> int {
    const size_t all_words = 64 + (size_t)p->K * 2 * p->blk_words;
    HIP_TRY(hipMalloc(&p->d_all, sizeof(float) * all_words));
    HIP_TRY(hipMemset(p->d_all, 0, sizeof(float) * all_words));      // the blocks the first passes' temporal pairs read: no keypoints
    HIP_TRY(hipMalloc(&p->d_scr, sizeof(float) * p->scr_words * p->K));
    const size_t rimg = (size_t)p->RW * p->RH;
    HIP_TRY(hipMalloc(&p->d_raw_all, rimg * NI * p->K));
    // the maps, copied into memory the pipe owns
    HIP_TRY(hipMalloc(&p->d_maps, sizeof(float) * 12 * img));
    const hipMemcpyKind kind = maps->device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    for (int c = 0; c < 4; ++c) {
      float* mc = p->d_maps + (size_t)c * 3 * img;
      HIP_TRY(hipMemcpy(mc, maps->mapx[c], sizeof(float) * img, kind));
      HIP_TRY(hipMemcpy(mc + img, maps->mapy[c], sizeof(float) * img, kind));
      if (maps->gain[c]) HIP_TRY(hipMemcpy(mc + 2 * img, maps->gain[c], sizeof(float) * img, kind));
      p->ua.mapx[c] = mc; p->ua.mapy[c] = mc + img; p->ua.gain[c] = maps->gain[c] ? mc + 2 * img : nullptr;
    }
    p->ua.cam_stride = (long)rimg; p->ua.quad_stride = (long)(4 * rimg); p->ua.sh = p->RH; p->ua.sw = p->RW; p->ua.sstride = p->RW;
    p->ua.npix = (int)img; p->ua.quads = p->Q; p->ua.vec_out = 1;      // img % 4 == 0 and the views start at 256-byte boundaries of the lane scratch
    // the half-image jobs of quad frame q: 2 (q * 4 + n) reads view a of neighbour pair n, 2 (q * 4 + n) + 1 view b
    const int Q = p->Q;
    std::vector<int32_t> jobs((size_t)32 * Q, 0);
    int32_t* jrow = jobs.data(); int32_t* jleft = jrow + 8 * Q; float* jshift = reinterpret_cast<float*>(jleft + 8 * Q);
    int32_t* ma = jleft + 16 * Q; int32_t* mb = ma + 4 * Q;
    for (int q = 0; q < Q; ++q)
      for (int n = 0; n < 4; ++n) {
        const int ja = 2 * (q * 4 + n), jb = ja + 1;
        const bool lr = NB[n][2] == 1;
        jrow[ja] = q * 4 + NB[n][0]; jleft[ja] = lr ? 1 : 0; jshift[ja] = lr ? p->move_cols : -p->move_cols;
        jrow[jb] = q * 4 + NB[n][1]; jleft[jb] = lr ? 0 : 1; jshift[jb] = 0.f;
        ma[q * 4 + n] = ja; mb[q * 4 + n] = jb;
      }
    HIP_TRY(hipMalloc(&p->d_jobs, sizeof(int32_t) * jobs.size()));
    HIP_TRY(hipMemcpy(p->d_jobs, jobs.data(), sizeof(int32_t) * jobs.size(), hipMemcpyHostToDevice));
    p->lanes.resize(p->K);
    // the stereo pipe's measured stream placement: a lane's two streams on different hardware pipes, consecutive lanes' streams on different ones too
    struct Spare { std::vector<hipStream_t> first, second; ~Spare() { for (auto& v : {&first, &second}) for (hipStream_t q : *v) if (q) (void)hipStreamDestroy(q); } } spare;
    const int rcs = place_streams(h->cfg.device_id, p->K, p->G ? p->K : 0, spare.first, spare.second, p->first_class, p->second_class, &p->n_classes, &p->probe_ticks,
                                  &p->probe_turns_us);
    if (rcs) return rcs;
    for (int k = 0; k < p->K; ++k) {
      auto& L = p->lanes[k];
      hipStream_t ms = spare.first[k]; spare.first[k] = nullptr;
      if (p->G) { L.nv = spare.second[k]; spare.second[k] = nullptr; }
      const int rc2 = clone_lane(h, NI, &L.ctx, ms, 0, p->G > 0);
      if (rc2) { (void)hipStreamDestroy(ms); return rc2; }
      L.s = L.ctx->stream;
      { const int rce = lane_create_events(L, false); if (rce) return rce; }      // ev_chain comes with d2fe_quad_track_enable
      L.d_raw = p->d_raw_all + (size_t)k * NI * rimg;
      if (!cfg->pinned_input) HIP_TRY(hipHostMalloc(&L.pin_in, rimg * NI, hipHostMallocDefault));
      for (int set = 0; set < 2; ++set) HIP_TRY(hipHostMalloc(&L.pin_out[set], sizeof(float) * p->d2h_words, hipHostMallocDefault));
    }
    if (p->NP) {
      std::vector<MatchPairDesc> tab;
      quad_fill_pairs(p, tab);
      HIP_TRY(hipMalloc(&p->d_pairs, sizeof(MatchPairDesc) * tab.size()));
      HIP_TRY(hipMemcpy(p->d_pairs, tab.data(), sizeof(MatchPairDesc) * tab.size(), hipMemcpyHostToDevice));
      p->match_scratch_lane = match_scratch_bytes((int)NP, p->cap);
      HIP_TRY(hipMalloc(&p->d_match_scratch, p->match_scratch_lane * p->K));
      HIP_TRY(hipMemset(p->d_match_scratch, 0, p->match_scratch_lane * p->K));
    }
    return D2FE_OK;
  }();
  if (rc != D2FE_OK) { d2fe_quad_pipe_destroy(p); return rc; }
  // the copies and memsets above ran on the null stream; the lanes' non-blocking streams do not wait for it
  if (hipDeviceSynchronize() != hipSuccess) { d2fe_quad_pipe_destroy(p); return ctx_fail(D2FE_ERR_HIP, "hipDeviceSynchronize"); }
  *out = p;
  return D2FE_OK;
}

void d2fe_quad_pipe_destroy(d2fe_quad_pipe p) {
  if (!p) return;
  (void)hipSetDevice(p->parent->cfg.device_id);
  for (auto& L : p->lanes) lane_destroy(L);
  for (void* q : {(void*)p->d_all, (void*)p->d_scr, (void*)p->d_raw_all, (void*)p->d_maps, (void*)p->d_jobs, (void*)p->d_pairs, (void*)p->d_match_scratch,
                  (void*)p->d_trk, (void*)p->d_trk_pyr, (void*)p->d_lpairs, (void*)p->d_lmatch_scratch, (void*)p->d_flow_scratch})
    if (q) (void)hipFree(q);
  d2fe_context* parent = p->parent;
  delete p;
  pipe_gone(parent);
}

int d2fe_quad_pipe_submit(d2fe_quad_pipe p, const uint8_t* raw, int stride, size_t camera_stride, size_t quad_stride, int64_t* ticket) {
  if (!p || !raw || !ticket) return ctx_fail(D2FE_ERR_INVALID, "null argument");
  if (stride < p->RW) return ctx_fail(D2FE_ERR_INVALID, "stride < raw_width");
  HIP_TRY(hipSetDevice(p->parent->cfg.device_id));
  std::lock_guard<std::mutex> lk(p->mu);
  if (p->failed) return ctx_fail(p->failed, "the quad pipe failed in an earlier call and accepts no more work (destroy it): " + p->failed_msg);
  // an error below leaves the pass half-enqueued: no later pass can build on it, so the first error is final for the pipe
  const int rc = quad_pass(p, raw, stride, camera_stride, quad_stride, ticket);
  if (rc != D2FE_OK) { p->failed = rc; p->failed_msg = d2fe_last_error(); }
  return rc;
}

int d2fe_quad_pipe_wait(d2fe_quad_pipe p, int64_t ticket, d2fe_quad_pipe_result* out) {
  if (!p || !out) return ctx_fail(D2FE_ERR_INVALID, "null argument");
  memset(out, 0, sizeof(*out));
  std::unique_lock<std::mutex> lk(p->mu);
  if (p->failed) return ctx_fail(p->failed, "the quad pipe failed in an earlier call (destroy it): " + p->failed_msg);
  if (ticket < 0 || ticket >= p->next_ticket) return ctx_fail(D2FE_ERR_INVALID, "unknown ticket");
  // the ticket's result block is written again by the pass 2 K submits later
  if (ticket + 2 * p->K < p->next_ticket) return ctx_fail(D2FE_ERR_INVALID, "the ticket's result block has been reused: wait for a ticket within 2 * lanes submits");
  HIP_TRY(hipSetDevice(p->parent->cfg.device_id));
  const int k = (int)(ticket % p->K), set = (int)((ticket / p->K) & 1);
  auto& L = p->lanes[k];
  if (L.synced < ticket) {
    const hipError_t e = lane_wait_unlocked(L, lk);
    if (e != hipSuccess) {
      p->failed = D2FE_ERR_HIP; p->failed_msg = std::string("hipEventSynchronize: ") + hipGetErrorString(e);
      return ctx_fail(D2FE_ERR_HIP, p->failed_msg);
    }
    if (ticket + 2 * p->K < p->next_ticket) return ctx_fail(D2FE_ERR_INVALID, "the ticket's result block was reused while this call waited for it");
  }
  const float* B = L.pin_out[set];
  const size_t cap = p->cap;
  out->quads = p->Q; out->cap = p->cap; out->desc_dim = p->D; out->netvlad_dim = p->G;
  out->kps_xy = B + p->o_kps; out->scores = B + p->o_scores; out->desc = B + p->o_desc;
  out->n_kp = reinterpret_cast<const int32_t*>(B + p->o_cnt);
  out->netvlad = p->G ? B + p->o_nv : nullptr;
  const int32_t* mq = reinterpret_cast<const int32_t*>(B + p->o_mq);
  const int32_t* mt = reinterpret_cast<const int32_t*>(B + p->o_mt);
  const int32_t* mn = reinterpret_cast<const int32_t*>(B + p->o_mn);
  const float* md = B + p->o_md;
  if (p->n_nb) { out->nb_q = mq; out->nb_t = mt; out->nb_dist = md; out->nb_n = mn; }
  if (p->n_pr) {
    const size_t pi = p->n_nb;
    out->prev_q = mq + pi * cap; out->prev_t = mt + pi * cap; out->prev_dist = md + pi * cap; out->prev_n = mn + pi;
  }
  return D2FE_OK;
}

int d2fe_quad_track_enable(d2fe_quad_pipe p, const d2fe_track_params* tp_in) {
  if (!p) return ctx_fail(D2FE_ERR_INVALID, "null pipe");
  d2fe_track_params tp;
  if (tp_in) tp = *tp_in; else d2fe_track_default_params(&tp);
  tp.reserved = 0;
  if (const char* why = lk_carry_check_params(&tp)) return ctx_fail(D2FE_ERR_INVALID, why);
  if (tp.levels != 2) return ctx_fail(D2FE_ERR_INVALID, "levels must be 2 (PYR_LEVEL): the lanes' pyramids are that deep");
  if (!(p->cfg.undistort_fov > 0.0)) return ctx_fail(D2FE_ERR_INVALID, "undistort_fov must be > 0 (move_cols of the neighbour tracks)");
  if (p->W < 16 || p->H < 16) return ctx_fail(D2FE_ERR_INVALID, "views smaller than 16 x 16 have no pyramid");
  std::lock_guard<std::mutex> lk(p->mu);
  if (p->failed) return ctx_fail(p->failed, "the quad pipe failed in an earlier call (destroy it): " + p->failed_msg);
  if (p->trk) return ctx_fail(D2FE_ERR_INVALID, "the mode is already on");
  if (p->flow) return ctx_fail(D2FE_ERR_INVALID, "sp_lk excludes the flow landmarks: the reference runs one of the two branches (d2featuretracker.cpp:556-614)");
  if (p->next_ticket > 0) return ctx_fail(D2FE_ERR_INVALID, "d2fe_quad_track_enable comes before the first submit");
  HIP_TRY(hipSetDevice(p->parent->cfg.device_id));
  const int capT = tp.total_feature_num + 1;
  QuadListMode m{capT, d2fe_lk_carry_list_bytes(capT, p->D) / sizeof(float), d2fe_lk_stereo_workspace_bytes(1, p->W, p->H, tp.levels) / 2, true, 0};
  if (!m.list_words || !m.pyr_total) return ctx_fail(D2FE_ERR_INVALID, "bad list or pyramid geometry");
  const int rc = quad_lists_enable(p, m);
  if (rc != D2FE_OK && !p->failed) return rc;      // nothing has changed
  p->tp = tp;
  p->trk = true;
  p->trk_split = d2fe_dev_env("D2FE_QUAD_TRACK_SPLIT", 0) != 0;
  return rc;
}

int d2fe_quad_track_result_get(d2fe_quad_pipe p, int64_t ticket, d2fe_quad_track_result* out) {
  if (!p || !out) return ctx_fail(D2FE_ERR_INVALID, "null argument");
  memset(out, 0, sizeof(*out));
  std::lock_guard<std::mutex> lk(p->mu);
  if (!p->trk) return ctx_fail(D2FE_ERR_UNSUPPORTED, "d2fe_quad_track_enable was not called on this pipe: it carries no landmark lists");
  if (p->failed) return ctx_fail(p->failed, "the quad pipe failed in an earlier call (destroy it): " + p->failed_msg);
  if (ticket < 0 || ticket >= p->next_ticket) return ctx_fail(D2FE_ERR_INVALID, "unknown ticket");
  if (ticket + 2 * p->K < p->next_ticket) return ctx_fail(D2FE_ERR_INVALID, "the ticket's result block has been reused: read the lists within 2 * lanes submits");
  const int k = (int)(ticket % p->K), set = (int)((ticket / p->K) & 1);
  const auto& L = p->lanes[k];
  if (L.synced < ticket) return ctx_fail(D2FE_ERR_NOT_READY, "d2fe_quad_pipe_wait has not returned this ticket yet");
  const float* B = L.pin_out[set];
  out->quads = p->Q;
  track_list_view(out, B + p->o_list, p->capT, p->D, p->list_words);
  out->nb_lk_xy = B + p->o_nbxy; out->nb_lk_status = reinterpret_cast<const uint8_t*>(B + p->o_nbst);
  out->lnb_q = reinterpret_cast<const int32_t*>(B + p->o_lmq); out->lnb_t = reinterpret_cast<const int32_t*>(B + p->o_lmt);
  out->lnb_dist = B + p->o_lmd; out->lnb_n = reinterpret_cast<const int32_t*>(B + p->o_lmn);
  return D2FE_OK;
}

int d2fe_quad_flow_enable(d2fe_quad_pipe p, const d2fe_flow_params* fp_in) {
  if (!p) return ctx_fail(D2FE_ERR_INVALID, "null pipe");
  d2fe_flow_params fp;
  if (fp_in) fp = *fp_in; else d2fe_flow_default_params(&fp);
  if (const char* why = lk_flow_check_params(&fp, p->W, p->H)) return ctx_fail(D2FE_ERR_INVALID, why);
  fp.reserved = 0; fp.track.reserved = 0;
  if (fp.track.levels != 2) return ctx_fail(D2FE_ERR_INVALID, "levels must be 2 (PYR_LEVEL): the lanes' pyramids are that deep");
  if (!fp.superpoint)
    return ctx_fail(D2FE_ERR_INVALID, "superpoint must be 1: no quadcam configuration of the reference sets max_superpoint_cnt: 0 (flow-only pipes are the stereo / mono ones)");
  if (!(p->cfg.undistort_fov > 0.0)) return ctx_fail(D2FE_ERR_INVALID, "undistort_fov must be > 0 (move_cols of the neighbour tracks)");
  std::lock_guard<std::mutex> lk(p->mu);
  if (p->failed) return ctx_fail(p->failed, "the quad pipe failed in an earlier call (destroy it): " + p->failed_msg);
  if (p->flow) return ctx_fail(D2FE_ERR_INVALID, "the flow landmarks are already switched on");
  if (p->trk) return ctx_fail(D2FE_ERR_INVALID, "the flow landmarks exclude sp_lk: the reference runs one of the two branches (d2featuretracker.cpp:556-614)");
  if (p->next_ticket > 0) return ctx_fail(D2FE_ERR_INVALID, "d2fe_quad_flow_enable comes before the first submit");
  HIP_TRY(hipSetDevice(p->parent->cfg.device_id));
  const int capF = flow_cap_tracks(fp.track);
  QuadListMode m{capF, d2fe_lk_flow_list_bytes(capF) / sizeof(float), d2fe_lk_stereo_workspace_bytes(1, p->W, p->H, fp.track.levels) / 2, false,
                 d2fe_lk_flow_scratch_bytes(p->W, p->H, capF, fp.fast_cols, fp.fast_rows)};
  if (!m.list_words || !m.pyr_total || !m.fast_scratch) return ctx_fail(D2FE_ERR_INVALID, "bad list, pyramid or detector geometry");
  const int rc = quad_lists_enable(p, m);
  if (rc != D2FE_OK && !p->failed) return rc;      // nothing has changed
  p->fp = fp;
  p->flow = true;
  p->flow_split = d2fe_dev_env("D2FE_QUAD_FLOW_SPLIT", 0) != 0;
  return rc;
}

int d2fe_quad_flow_result_get(d2fe_quad_pipe p, int64_t ticket, d2fe_quad_flow_result* out) {
  if (!p || !out) return ctx_fail(D2FE_ERR_INVALID, "null argument");
  memset(out, 0, sizeof(*out));
  std::lock_guard<std::mutex> lk(p->mu);
  if (!p->flow) return ctx_fail(D2FE_ERR_UNSUPPORTED, "d2fe_quad_flow_enable was not called on this pipe: it carries no flow landmarks");
  if (p->failed) return ctx_fail(p->failed, "the quad pipe failed in an earlier call (destroy it): " + p->failed_msg);
  if (ticket < 0 || ticket >= p->next_ticket) return ctx_fail(D2FE_ERR_INVALID, "unknown ticket");
  if (ticket + 2 * p->K < p->next_ticket) return ctx_fail(D2FE_ERR_INVALID, "the ticket's result block has been reused: read the lists within 2 * lanes submits");
  const int k = (int)(ticket % p->K), set = (int)((ticket / p->K) & 1);
  const auto& L = p->lanes[k];
  if (L.synced < ticket) return ctx_fail(D2FE_ERR_NOT_READY, "d2fe_quad_pipe_wait has not returned this ticket yet");
  const float* B = L.pin_out[set];
  out->quads = p->Q;
  flow_list_view(out, B + p->o_list, p->capT, p->list_words);
  out->nb_lk_xy = B + p->o_nbxy; out->nb_lk_status = reinterpret_cast<const uint8_t*>(B + p->o_nbst);
  return D2FE_OK;
}

void d2fe_quad_bearings_default(d2fe_quad_bearings* b) {
  memset(b, 0, sizeof(*b));
  b->struct_size = (int32_t)sizeof(d2fe_quad_bearings);
  b->lk_use_pred = 1;
  b->distance = 100.0;
  for (int n = 0; n < 4; ++n) b->T_nb[n][0] = b->T_nb[n][5] = b->T_nb[n][10] = 1.0;
}

int d2fe_quad_bearings_enable(d2fe_quad_pipe p, const d2fe_quad_bearings* b) {
  if (!p || !b) return ctx_fail(D2FE_ERR_INVALID, "null argument");
  if (b->struct_size != (int32_t)sizeof(d2fe_quad_bearings)) return ctx_fail(D2FE_ERR_INVALID, "d2fe_quad_bearings size mismatch");
  for (int c = 0; c < 4; ++c)
    if (const char* why = bearings_check_camera(&b->cam[c])) return ctx_fail(D2FE_ERR_INVALID, "cam[" + std::to_string(c) + "]: " + why);
  if (!(b->distance - b->distance == 0.0)) return ctx_fail(D2FE_ERR_INVALID, "distance must be finite");
  for (int n = 0; n < 4; ++n)
    for (int i = 0; i < 12; ++i) if (!(b->T_nb[n][i] - b->T_nb[n][i] == 0.0)) return ctx_fail(D2FE_ERR_INVALID, "T_nb must be finite");
  if (b->radius_lk != b->radius_lk) return ctx_fail(D2FE_ERR_INVALID, "radius_lk must not be NaN");
  if (b->lk_use_pred != 0 && b->lk_use_pred != 1) return ctx_fail(D2FE_ERR_INVALID, "lk_use_pred must be 0 or 1");
  std::lock_guard<std::mutex> lk(p->mu);
  if (p->failed) return ctx_fail(p->failed, "the quad pipe failed in an earlier call (destroy it): " + p->failed_msg);
  if (p->next_ticket > 0) return ctx_fail(D2FE_ERR_INVALID, "the bearings are switched on before the first submit");
  if (p->bear) return ctx_fail(D2FE_ERR_INVALID, "the bearings are already switched on");
  HIP_TRY(hipSetDevice(p->parent->cfg.device_id));
  const int rc = quad_bear_blocks(p);
  if (rc != D2FE_OK && !p->failed) return rc;      // nothing has changed
  p->bear = true;
  p->bcams = BearCams{};
  for (int c = 0; c < 4; ++c) p->bcams.cam[c] = bearings_make_camera(b->cam[c]);
  for (int n = 0; n < 4; ++n)
    for (int i = 0; i < 12; ++i) p->bcams.T[n][i] = b->T_nb[n][i];
  p->bcams.distance = b->distance;
  p->bcams.radius = b->lk_use_pred ? b->radius_lk : 0.0;
  return rc;
}

int d2fe_quad_bearings_result_get(d2fe_quad_pipe p, int64_t ticket, d2fe_quad_bearings_result* out) {
  if (!p || !out) return ctx_fail(D2FE_ERR_INVALID, "null argument");
  memset(out, 0, sizeof(*out));
  std::lock_guard<std::mutex> lk(p->mu);
  if (!p->bear) return ctx_fail(D2FE_ERR_UNSUPPORTED, "d2fe_quad_bearings_enable was not called on this pipe: it computes no bearings");
  if (p->failed) return ctx_fail(p->failed, "the quad pipe failed in an earlier call (destroy it): " + p->failed_msg);
  if (ticket < 0 || ticket >= p->next_ticket) return ctx_fail(D2FE_ERR_INVALID, "unknown ticket");
  if (ticket + 2 * p->K < p->next_ticket) return ctx_fail(D2FE_ERR_INVALID, "the ticket's result block has been reused: read the bearings within 2 * lanes submits");
  const int k = (int)(ticket % p->K), set = (int)((ticket / p->K) & 1);
  const auto& L = p->lanes[k];
  if (L.synced < ticket) return ctx_fail(D2FE_ERR_NOT_READY, "d2fe_quad_pipe_wait has not returned this ticket yet");
  const float* B = L.pin_out[set];
  const bool lists = p->trk || p->flow;
  out->quads = p->Q; out->cap = p->cap; out->cap_tracks = lists ? p->capT : 0;
  out->kp_bearing = reinterpret_cast<const double*>(B + p->o_bkb);
  if (lists) {
    out->list_bearing = reinterpret_cast<const double*>(B + p->o_blb);
    out->nb_pred_xy = B + p->o_bnp;
    out->nb_bearing = reinterpret_cast<const double*>(B + p->o_bnb);
    out->nb_pred_ok = reinterpret_cast<const uint8_t*>(B + p->o_bno);
  }
  return D2FE_OK;
}

int d2fe_quad_pipe_lanes(d2fe_quad_pipe p) { return p ? p->K : ctx_fail(D2FE_ERR_INVALID, "null pipe"); }

int d2fe_quad_pipe_geometry(d2fe_quad_pipe p, int32_t* quads, int32_t* cap, int32_t* desc_dim, int32_t* netvlad_dim) {
  if (!p) return ctx_fail(D2FE_ERR_INVALID, "null pipe");
  if (quads) *quads = p->Q;
  if (cap) *cap = p->cap;
  if (desc_dim) *desc_dim = p->D;
  if (netvlad_dim) *netvlad_dim = p->G;
  return D2FE_OK;
}

// ---- device-side consumers of a ticket (the cross-agent exchange, quad_exchange.hip) ------------------------------------------------------------------
namespace {
// the ticket's (lane, set) while its result block is still the one the ticket wrote (called with the pipe's mutex held)
int quad_view_locate(d2fe_quad_pipe_s* p, int64_t ticket, int* k, int* set) {
  if (ticket < 0 || ticket >= p->next_ticket) return ctx_fail(D2FE_ERR_INVALID, "unknown ticket");
  if (ticket + 2 * p->K < p->next_ticket) return ctx_fail(D2FE_ERR_INVALID, "the ticket's result block has been reused: take the view within 2 * lanes submits");
  *k = (int)(ticket % p->K); *set = (int)((ticket / p->K) & 1);
  return D2FE_OK;
}
}  // namespace

int d2fe_quad_device_view(d2fe_quad_pipe p, int64_t ticket, void* stream, d2fe_quad_device_result* out) {
  if (!p || !out || !stream) return ctx_fail(D2FE_ERR_INVALID, "null argument (the consumer's stream must be a real hipStream_t)");
  memset(out, 0, sizeof(*out));
  std::lock_guard<std::mutex> lk(p->mu);
  if (p->failed) return ctx_fail(p->failed, "the quad pipe failed in an earlier call (destroy it): " + p->failed_msg);
  HIP_TRY(hipSetDevice(p->parent->cfg.device_id));
  int k, set;
  const int rc = quad_view_locate(p, ticket, &k, &set);
  if (rc) return rc;
  auto& L = p->lanes[k];
  const int rcv = lane_view_acquire(L, set, p->G > 0, static_cast<hipStream_t>(stream));      // (quad_view_locate has excluded a block that is being rewritten)
  if (rcv) return rcv;
  const float* B = p->block(k, set);
  out->quads = p->Q; out->cap = p->cap; out->desc_dim = p->D; out->netvlad_dim = p->G;
  out->d_kps_xy = B + p->o_kps; out->d_scores = B + p->o_scores; out->d_desc = B + p->o_desc;
  out->d_n_kp = reinterpret_cast<const int32_t*>(B + p->o_cnt);
  out->d_netvlad = p->G ? B + p->o_nv : nullptr;
  return D2FE_OK;
}

int d2fe_quad_device_release(d2fe_quad_pipe p, int64_t ticket, void* stream) {
  if (!p || !stream) return ctx_fail(D2FE_ERR_INVALID, "null argument");
  std::lock_guard<std::mutex> lk(p->mu);
  HIP_TRY(hipSetDevice(p->parent->cfg.device_id));
  int k, set;
  const int rc = quad_view_locate(p, ticket, &k, &set);
  if (rc) return rc;
  return lane_view_release(p->lanes[k], set, static_cast<hipStream_t>(stream));
}

int d2fe_quad_lane_stream(d2fe_quad_pipe p, int64_t ticket, void** stream) {
  if (!p || !stream) return ctx_fail(D2FE_ERR_INVALID, "null argument");
  std::lock_guard<std::mutex> lk(p->mu);
  int k, set;
  const int rc = quad_view_locate(p, ticket, &k, &set);
  if (rc) return rc;
  *stream = p->lanes[k].s;
  return D2FE_OK;
}

d2fe_handle d2fe_quad_handle(d2fe_quad_pipe p) { return p ? p->parent : nullptr; }

}  // extern "C"
