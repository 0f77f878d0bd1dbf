// next_host.hip -- the "next rows" of the C ABI (include/d2fe.h): undistort, prepare_gray, the map generators, the descriptor database
// (d2fe_db_*), the int8 codec, the block pack / unpack / gate wrappers, half-image compact and remap.  Argument checks in front of the launchers of next.hip
// and swarm.hip; the host-pointer forms stage through the handle's scratch (ctx_scratch).  Host code only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <mutex>
#include <string>
#include <vector>

#include "context.h"

using namespace d2fe;

extern "C" {

struct d2fe_db {
  d2fe_context* h = nullptr;
  int dim = 0, cap = 0, ntotal = 0;
  DevPool pool;            // holds the five buffers below
  float* vecs = nullptr;
  float* sims = nullptr;   // [maxq][cap] scratch
  float* q = nullptr;      // staged queries
  float* osims = nullptr; int32_t* olabels = nullptr;
  std::mutex mu;
};
namespace { constexpr int DB_MAXQ = 8, DB_MAXK = 1024; }

int d2fe_undistort_device(d2fe_handle h, const uint8_t* d_src, int n, int sw, int sh, int sstride, size_t src_image_stride,
                          const float* d_mapx, const float* d_mapy, const float* d_gain, int dw, int dh, uint8_t* d_dst,
                          void* stream) {
  if (!h || !d_src || !d_mapx || !d_mapy || !d_dst) return fail(D2FE_ERR_INVALID, "null argument");
  if (n < 1 || sw < 1 || sh < 1 || sstride < sw || dw < 1 || dh < 1) return fail(D2FE_ERR_INVALID, "bad geometry");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  HIP_TRY(launch_undistort(d_src, sh, sw, sstride, (long)src_image_stride, d_mapx, d_mapy, d_gain, dh, dw, n, d_dst,
                           stream ? (hipStream_t)stream : h->stream));
  return D2FE_OK;
}

int d2fe_undistort(d2fe_handle h, const uint8_t* src, int sw, int sh, int sstride, const float* mapx, const float* mapy,
                   const float* gain, int dw, int dh, uint8_t* dst) {
  if (!h || !src || !mapx || !mapy || !dst) return fail(D2FE_ERR_INVALID, "null argument");
  if (sw < 1 || sh < 1 || sstride < sw || dw < 1 || dh < 1) return fail(D2FE_ERR_INVALID, "bad geometry");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  const size_t sb = (size_t)sstride * sh, mb = sizeof(float) * (size_t)dw * dh, db = (size_t)dw * dh;
  void* raw = nullptr;
  { const int rc0 = d2fe::ctx_scratch(h, sb + 3 * mb + db + 64, &raw); if (rc0 != D2FE_OK) return rc0; }
  char* buf = static_cast<char*>(raw);
  uint8_t* d_src = reinterpret_cast<uint8_t*>(buf);
  float* d_mx = reinterpret_cast<float*>(buf + ((sb + 15) / 16) * 16);
  float* d_my = d_mx + db; float* d_g = d_my + db;
  uint8_t* d_dst = reinterpret_cast<uint8_t*>(d_g + db);
  hipStream_t s = h->stream;
  int rc = D2FE_OK;
  auto chk = [&](hipError_t e, const char* w) { if (e != hipSuccess && rc == D2FE_OK) rc = fail(D2FE_ERR_HIP, std::string(w) + ": " + hipGetErrorString(e)); };
  chk(hipMemcpyAsync(d_src, src, sb, hipMemcpyHostToDevice, s), "H2D src");
  chk(hipMemcpyAsync(d_mx, mapx, mb, hipMemcpyHostToDevice, s), "H2D mapx");
  chk(hipMemcpyAsync(d_my, mapy, mb, hipMemcpyHostToDevice, s), "H2D mapy");
  if (gain) chk(hipMemcpyAsync(d_g, gain, mb, hipMemcpyHostToDevice, s), "H2D gain");
  if (rc == D2FE_OK) chk(launch_undistort(d_src, sh, sw, sstride, 0, d_mx, d_my, gain ? d_g : nullptr, dh, dw, 1, d_dst, s), "undistort");
  if (rc == D2FE_OK) chk(hipMemcpyAsync(dst, d_dst, db, hipMemcpyDeviceToHost, s), "D2H");
  chk(hipStreamSynchronize(s), "sync");
  return rc;
}

int d2fe_prepare_gray_device(d2fe_handle h, const uint8_t* d_src, int n, int channels, int sw, int sh, int sstride,
                             size_t src_image_stride, int dw, int dh, uint8_t* d_dst, void* stream) {
  if (!h || !d_src || !d_dst) return fail(D2FE_ERR_INVALID, "null argument");
  if (n < 1 || (channels != 1 && channels != 3) || sw < 2 || sh < 2 || sstride < sw * channels || dw < 1 || dh < 1)
    return fail(D2FE_ERR_INVALID, "bad geometry (channels must be 1 or 3)");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  HIP_TRY(launch_prep_gray(d_src, channels, sw, sh, sstride, (long)src_image_stride, n, dw, dh, d_dst, stream ? (hipStream_t)stream : h->stream));
  return D2FE_OK;
}

int d2fe_prepare_gray(d2fe_handle h, const uint8_t* src, int channels, int sw, int sh, int sstride, int dw, int dh, uint8_t* dst) {
  if (!h || !src || !dst) return fail(D2FE_ERR_INVALID, "null argument");
  if ((channels != 1 && channels != 3) || sw < 2 || sh < 2 || sstride < sw * channels || dw < 1 || dh < 1)
    return fail(D2FE_ERR_INVALID, "bad geometry (channels must be 1 or 3)");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  const size_t sb = (size_t)sstride * sh, db = (size_t)dw * dh;
  void* raw = nullptr;
  { const int rc0 = d2fe::ctx_scratch(h, sb + db + 64, &raw); if (rc0 != D2FE_OK) return rc0; }
  uint8_t* d_src = static_cast<uint8_t*>(raw);
  uint8_t* d_dst = d_src + ((sb + 15) / 16) * 16;
  hipStream_t s = h->stream;
  int rc = D2FE_OK;
  auto chk = [&](hipError_t e, const char* w) { if (e != hipSuccess && rc == D2FE_OK) rc = fail(D2FE_ERR_HIP, std::string(w) + ": " + hipGetErrorString(e)); };
  chk(hipMemcpyAsync(d_src, src, sb, hipMemcpyHostToDevice, s), "H2D");
  if (rc == D2FE_OK) chk(launch_prep_gray(d_src, channels, sw, sh, sstride, 0, 1, dw, dh, d_dst, s), "prep_gray");
  if (rc == D2FE_OK) chk(hipMemcpyAsync(dst, d_dst, db, hipMemcpyDeviceToHost, s), "D2H");
  chk(hipStreamSynchronize(s), "sync");
  return rc;
}

static int gen_map(d2fe_handle h, const d2fe_mei_camera* cam, const double* q, int mode, int width, int height, double f,
                   float* mapx, float* mapy, bool device, void* stream) {
  if (!h || !cam || !mapx || !mapy || (mode == 1 && !q)) return fail(D2FE_ERR_INVALID, "null argument");
  if (width < 2 || height < 2 || (size_t)width * height > (1u << 28) || !(f > 0)) return fail(D2FE_ERR_INVALID, "bad map geometry");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  const double c9[9] = {cam->xi, cam->k1, cam->k2, cam->p1, cam->p2, cam->gamma1, cam->gamma2, cam->u0, cam->v0};
  hipStream_t s = device && stream ? (hipStream_t)stream : h->stream;
  if (device) {
    HIP_TRY(launch_gen_map(c9, q, mode, width, height, f, mapx, mapy, s));
    return D2FE_OK;
  }
  const size_t n = (size_t)width * height;
  void* raw = nullptr;
  { const int rc0 = d2fe::ctx_scratch(h, sizeof(float) * 2 * n, &raw); if (rc0 != D2FE_OK) return rc0; }
  float* buf = static_cast<float*>(raw);
  int rc = D2FE_OK;
  auto chk = [&](hipError_t e, const char* w) { if (e != hipSuccess && rc == D2FE_OK) rc = fail(D2FE_ERR_HIP, std::string(w) + ": " + hipGetErrorString(e)); };
  chk(launch_gen_map(c9, q, mode, width, height, f, buf, buf + n, s), "gen_map");
  chk(hipMemcpyAsync(mapx, buf, sizeof(float) * n, hipMemcpyDeviceToHost, s), "D2H mapx");
  chk(hipMemcpyAsync(mapy, buf + n, sizeof(float) * n, hipMemcpyDeviceToHost, s), "D2H mapy");
  chk(hipStreamSynchronize(s), "sync");
  return rc;
}
static double cyl_focal(int width, double fov_deg) { return (double)(unsigned)width / (fov_deg * (M_PI / 180.0)); }

int d2fe_gen_cylinder_map(d2fe_handle h, const d2fe_mei_camera* cam, int width, int height, double fov_deg, float* mapx, float* mapy) {
  if (!(fov_deg > 0)) return fail(D2FE_ERR_INVALID, "fov must be positive");
  return gen_map(h, cam, nullptr, 0, width, height, cyl_focal(width, fov_deg), mapx, mapy, false, nullptr);
}
int d2fe_gen_cylinder_map_device(d2fe_handle h, const d2fe_mei_camera* cam, int width, int height, double fov_deg, float* d_mapx,
                                 float* d_mapy, void* stream) {
  if (!(fov_deg > 0)) return fail(D2FE_ERR_INVALID, "fov must be positive");
  return gen_map(h, cam, nullptr, 0, width, height, cyl_focal(width, fov_deg), d_mapx, d_mapy, true, stream);
}
// the virtual camera the two generators above assume (FisheyeUndist's CylindricalCamera, fisheye_undistort.h:492-495): the same focal length, the integer centre
int d2fe_cylinder_camera(int width, int height, double fov_deg, d2fe_camera* out) {
  if (!out) return fail(D2FE_ERR_INVALID, "null argument");
  if (width < 1 || height < 1 || !(fov_deg > 0)) return fail(D2FE_ERR_INVALID, "width and height must be >= 1, fov positive");
  *out = d2fe_camera{};
  out->kind = D2FE_CAM_CYLINDRICAL;
  out->p[0] = out->p[1] = cyl_focal(width, fov_deg);
  out->p[2] = (double)((unsigned)width / 2); out->p[3] = (double)((unsigned)height / 2);
  return D2FE_OK;
}
int d2fe_gen_pinhole_map(d2fe_handle h, const d2fe_mei_camera* cam, const double* q_wxyz, int width, int height, double f,
                         float* mapx, float* mapy) {
  return gen_map(h, cam, q_wxyz, 1, width, height, f, mapx, mapy, false, nullptr);
}
int d2fe_gen_pinhole_map_device(d2fe_handle h, const d2fe_mei_camera* cam, const double* q_wxyz, int width, int height, double f,
                                float* d_mapx, float* d_mapy, void* stream) {
  return gen_map(h, cam, q_wxyz, 1, width, height, f, d_mapx, d_mapy, true, stream);
}

void d2fe_db_destroy(d2fe_db_handle db);
int d2fe_db_create(d2fe_handle h, int dim, int capacity, d2fe_db_handle* out) {
  if (!h || !out) return fail(D2FE_ERR_INVALID, "null argument");
  *out = nullptr;
  if (dim < 4 || (dim & 3) || dim > 8192 || capacity < 1) return fail(D2FE_ERR_INVALID, "dim must be a multiple of 4 in 4..8192, capacity >= 1");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  d2fe_db* db = new d2fe_db();
  db->h = h; db->dim = dim; db->cap = capacity;
  const int rc = [&]() -> int {
    HIP_TRY(db->pool.alloc(&db->vecs, sizeof(float) * (size_t)dim * capacity));
    HIP_TRY(db->pool.alloc(&db->sims, sizeof(float) * (size_t)DB_MAXQ * capacity));
    HIP_TRY(db->pool.alloc(&db->q, sizeof(float) * (size_t)DB_MAXQ * dim));
    HIP_TRY(db->pool.alloc(&db->osims, sizeof(float) * DB_MAXQ * DB_MAXK));
    HIP_TRY(db->pool.alloc(&db->olabels, sizeof(int32_t) * DB_MAXQ * DB_MAXK));
    return D2FE_OK;
  }();
  if (rc != D2FE_OK) { d2fe_db_destroy(db); return rc; }
  *out = db;
  return D2FE_OK;
}

void d2fe_db_destroy(d2fe_db_handle db) {
  if (!db) return;
  hipSetDevice(db->h->cfg.device_id);
  delete db;
}

int d2fe_db_ntotal(d2fe_db_handle db) { return db ? db->ntotal : fail(D2FE_ERR_INVALID, "null db"); }

int d2fe_db_add(d2fe_db_handle db, const float* vecs, int n) {
  if (!db || !vecs || n < 1) return fail(D2FE_ERR_INVALID, "bad argument");
  std::lock_guard<std::mutex> lk(db->mu);
  if (db->ntotal + n > db->cap) return fail(D2FE_ERR_TRUNCATED, "database capacity exceeded");
  HIP_TRY(hipSetDevice(db->h->cfg.device_id));
  HIP_TRY(hipMemcpy(db->vecs + (size_t)db->ntotal * db->dim, vecs, sizeof(float) * (size_t)n * db->dim, hipMemcpyHostToDevice));
  const int first = db->ntotal;
  db->ntotal += n;
  return first;
}

int d2fe_db_search(d2fe_db_handle db, const float* q, int nq, int k, float* sims, int32_t* labels) {
  if (!db || !q || !sims || !labels) return fail(D2FE_ERR_INVALID, "null argument");
  if (nq < 1 || nq > DB_MAXQ || k < 1 || k > DB_MAXK || (size_t)nq * db->dim * 4 > 65536) return fail(D2FE_ERR_INVALID, "nq/k out of range");
  std::lock_guard<std::mutex> lk(db->mu);
  for (int i = 0; i < nq * k; ++i) { labels[i] = -1; sims[i] = 0.f; }
  if (db->ntotal == 0) return D2FE_OK;
  HIP_TRY(hipSetDevice(db->h->cfg.device_id));
  hipStream_t s = db->h->stream;
  const int kk = k < db->ntotal ? k : db->ntotal;
  HIP_TRY(hipMemcpyAsync(db->q, q, sizeof(float) * (size_t)nq * db->dim, hipMemcpyHostToDevice, s));
  HIP_TRY(launch_db_search(db->vecs, db->ntotal, db->dim, db->q, nq, kk, db->sims, db->olabels, db->osims, s));
  std::vector<float> hs((size_t)nq * kk); std::vector<int32_t> hl((size_t)nq * kk);
  HIP_TRY(hipMemcpyAsync(hs.data(), db->osims, sizeof(float) * hs.size(), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(hl.data(), db->olabels, sizeof(int32_t) * hl.size(), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (int qi = 0; qi < nq; ++qi)
    for (int r = 0; r < kk; ++r) { sims[(size_t)qi * k + r] = hs[(size_t)qi * kk + r]; labels[(size_t)qi * k + r] = hl[(size_t)qi * kk + r]; }
  return D2FE_OK;
}

int d2fe_db_query_gated(d2fe_db_handle db, const float* q, int max_index, double thres, int32_t* label, float* sim) {
  if (!db || !q || !label || !sim || max_index < 0) return fail(D2FE_ERR_INVALID, "bad argument");
  *label = -1; *sim = 0.f;
  const int ntotal = db->ntotal;
  int k = 5 + max_index;                      // SEARCH_NEAREST_NUM, d2frontend_params.h:22
  if (k > ntotal) k = ntotal;
  if (k <= 0) return D2FE_OK;
  if (k > DB_MAXK) k = DB_MAXK;
  std::vector<float> s(k); std::vector<int32_t> l(k);
  int rc = d2fe_db_search(db, q, 1, k, s.data(), l.data());
  if (rc) return rc;
  for (int i = 0; i < k; ++i) {
    if (l[i] < 0) continue;
    if (l[i] <= ntotal - max_index && (double)s[i] > thres) { *label = l[i]; *sim = s[i]; return D2FE_OK; }
  }
  return D2FE_OK;
}

static int codec_run(d2fe_handle h, const void* in, size_t in_bytes, void* out, size_t out_bytes, int n, int arg, bool quant) {
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  void* raw = nullptr;
  { const int rc0 = d2fe::ctx_scratch(h, in_bytes + out_bytes + 64, &raw); if (rc0 != D2FE_OK) return rc0; }
  char* buf = static_cast<char*>(raw);
  char* d_out = buf + ((in_bytes + 15) / 16) * 16;
  hipStream_t s = h->stream;
  int rc = D2FE_OK;
  auto chk = [&](hipError_t e, const char* w) { if (e != hipSuccess && rc == D2FE_OK) rc = fail(D2FE_ERR_HIP, std::string(w) + ": " + hipGetErrorString(e)); };
  chk(hipMemcpyAsync(buf, in, in_bytes, hipMemcpyHostToDevice, s), "H2D");
  if (rc == D2FE_OK) {
    if (quant) chk(launch_quant_int8(reinterpret_cast<const float*>(buf), n, arg, reinterpret_cast<int8_t*>(d_out), s), "quant");
    else chk(launch_dequant_int8(reinterpret_cast<const int8_t*>(buf), n, arg, reinterpret_cast<float*>(d_out), s), "dequant");
  }
  if (rc == D2FE_OK) chk(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, s), "D2H");
  chk(hipStreamSynchronize(s), "sync");
  return rc;
}

int d2fe_quantize_int8(d2fe_handle h, const float* x, int n, int double_max, int8_t* out) {
  if (!h || !x || !out || n < 1) return fail(D2FE_ERR_INVALID, "bad argument");
  return codec_run(h, x, sizeof(float) * (size_t)n, out, (size_t)n, n, double_max ? 1 : 0, true);
}

int d2fe_dequantize_int8(d2fe_handle h, const int8_t* q, int n, int landmark_num, float* out) {
  if (!h || !q || !out || n < 1) return fail(D2FE_ERR_INVALID, "bad argument");
  if (landmark_num >= 0 && (n & 31)) return fail(D2FE_ERR_INVALID, "landmark descriptors: n must be a multiple of 32");
  return codec_run(h, q, (size_t)n, out, sizeof(float) * (size_t)n, n, landmark_num, false);
}

// desc_dim: 4..256, a multiple of 4 (rows stay 16-byte aligned behind the descriptors of a block)
static bool block_dim_ok(int desc_dim) { return desc_dim >= 4 && desc_dim <= 256 && !(desc_dim & 3); }
int d2fe_block_field_offset_d(int cap, int desc_dim, int netvlad_dim, int field) {
  if (cap < 1 || !block_dim_ok(desc_dim) || netvlad_dim < 0 || field < 0 || field > 4) return fail(D2FE_ERR_INVALID, "bad argument");
  const int off[5] = {0, cap * desc_dim, cap * (desc_dim + 2), cap * (desc_dim + 3), cap * (desc_dim + 3) + netvlad_dim};
  return off[field];
}
int d2fe_block_field_offset(int cap, int netvlad_dim, int field) { return d2fe_block_field_offset_d(cap, 256, netvlad_dim, field); }
int d2fe_block_words_d(int cap, int desc_dim, int netvlad_dim) {
  if (cap < 1 || !block_dim_ok(desc_dim) || netvlad_dim < 0 || (netvlad_dim & 3)) return fail(D2FE_ERR_INVALID, "bad argument");
  return (cap * (desc_dim + 3) + netvlad_dim + 1 + 255) / 256 * 256;
}
int d2fe_block_words(int cap, int netvlad_dim) { return d2fe_block_words_d(cap, 256, netvlad_dim); }
int d2fe_pack_blocks_device_d(d2fe_handle h, const float* d_desc, const float* d_kps_xy, const float* d_scores, const int32_t* d_n,
                              const float* d_netvlad, int row0, int row_step, int nframes, int cap, int desc_dim, int netvlad_dim, float* d_blocks,
                              void* stream) {
  if (!h || !d_desc || !d_kps_xy || !d_scores || !d_n || !d_blocks) return fail(D2FE_ERR_INVALID, "null argument");
  if (nframes < 1 || cap < 1 || row0 < 0 || row_step < 1 || !block_dim_ok(desc_dim) || netvlad_dim < 0 || (netvlad_dim & 3)) return fail(D2FE_ERR_INVALID, "bad geometry");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  HIP_TRY(launch_pack_blocks(d_desc, d_kps_xy, d_scores, d_n, d_netvlad, row0, row_step, nframes, cap, desc_dim, netvlad_dim,
                             d2fe_block_words_d(cap, desc_dim, netvlad_dim), d_blocks, stream ? (hipStream_t)stream : h->stream));
  return D2FE_OK;
}
int d2fe_pack_blocks_device(d2fe_handle h, const float* d_desc, const float* d_kps_xy, const float* d_scores, const int32_t* d_n,
                            const float* d_netvlad, int row0, int row_step, int nframes, int cap, int netvlad_dim, float* d_blocks,
                            void* stream) {
  return d2fe_pack_blocks_device_d(h, d_desc, d_kps_xy, d_scores, d_n, d_netvlad, row0, row_step, nframes, cap, 256, netvlad_dim, d_blocks, stream);
}
int d2fe_gate_pairs_device(d2fe_handle h, const float* d_q, size_t q_stride, const float* d_db, size_t db_stride, int dim,
                           const int32_t* d_pair_q, const int32_t* d_pair_db, int npairs, double thres, int32_t* d_cnt_inout,
                           int32_t* d_pass, float* d_sims, int32_t* d_n_pass, void* stream) {
  if (!h || !d_q || !d_db || !d_pair_q || !d_pair_db) return fail(D2FE_ERR_INVALID, "null argument");
  if (npairs < 1 || dim < 4 || (dim & 3)) return fail(D2FE_ERR_INVALID, "dim must be a multiple of 4");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  HIP_TRY(launch_gate_pairs(d_q, (long)q_stride, d_db, (long)db_stride, dim, d_pair_q, d_pair_db, npairs, thres, d_cnt_inout, d_pass,
                            d_sims, d_n_pass, stream ? (hipStream_t)stream : h->stream));
  return D2FE_OK;
}

int d2fe_block_bytes_int8_d(int cap, int desc_dim, int netvlad_dim) {
  if (cap < 1 || !block_dim_ok(desc_dim) || netvlad_dim < 0 || (netvlad_dim & 3)) return fail(D2FE_ERR_INVALID, "bad argument");
  return (cap * desc_dim + netvlad_dim + cap * 8 + 4 + 63) / 64 * 64;
}
int d2fe_block_bytes_int8(int cap, int netvlad_dim) { return d2fe_block_bytes_int8_d(cap, 256, netvlad_dim); }
int d2fe_pack_blocks_int8_device_d(d2fe_handle h, const float* d_desc, const float* d_kps_xy, const int32_t* d_n, const float* d_netvlad,
                                   int row0, int row_step, int nframes, int cap, int desc_dim, int netvlad_dim, int8_t* d_blocks, void* stream) {
  if (!h || !d_desc || !d_kps_xy || !d_n || !d_blocks) return fail(D2FE_ERR_INVALID, "null argument");
  if (nframes < 1 || cap < 1 || row0 < 0 || row_step < 1 || !block_dim_ok(desc_dim) || netvlad_dim < 0 || (netvlad_dim & 3)) return fail(D2FE_ERR_INVALID, "bad geometry");
  if (((uintptr_t)d_desc & 15) || ((uintptr_t)d_blocks & 3)) return fail(D2FE_ERR_INVALID, "d_desc must be 16-byte aligned, d_blocks 4-byte aligned");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  HIP_TRY(launch_pack_blocks_int8(d_desc, d_kps_xy, d_n, d_netvlad, row0, row_step, nframes, cap, desc_dim, netvlad_dim,
                                  d2fe_block_bytes_int8_d(cap, desc_dim, netvlad_dim), d_blocks, stream ? (hipStream_t)stream : h->stream));
  return D2FE_OK;
}
int d2fe_pack_blocks_int8_device(d2fe_handle h, const float* d_desc, const float* d_kps_xy, const int32_t* d_n, const float* d_netvlad,
                                 int row0, int row_step, int nframes, int cap, int netvlad_dim, int8_t* d_blocks, void* stream) {
  return d2fe_pack_blocks_int8_device_d(h, d_desc, d_kps_xy, d_n, d_netvlad, row0, row_step, nframes, cap, 256, netvlad_dim, d_blocks, stream);
}
int d2fe_unpack_blocks_int8_device_d(d2fe_handle h, const int8_t* d_blocks_int8, int nblocks, int cap, int desc_dim, int netvlad_dim, int renorm,
                                     float* d_blocks, void* stream) {
  if (!h || !d_blocks_int8 || !d_blocks) return fail(D2FE_ERR_INVALID, "null argument");
  if (nblocks < 1 || cap < 1 || !block_dim_ok(desc_dim) || netvlad_dim < 0 || (netvlad_dim & 3) || (renorm != 0 && renorm != 1)) return fail(D2FE_ERR_INVALID, "bad geometry");
  if (((uintptr_t)d_blocks & 15) || ((uintptr_t)d_blocks_int8 & 3)) return fail(D2FE_ERR_INVALID, "d_blocks must be 16-byte aligned, d_blocks_int8 4-byte aligned");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  HIP_TRY(launch_unpack_blocks_int8(d_blocks_int8, nblocks, cap, desc_dim, netvlad_dim, d2fe_block_bytes_int8_d(cap, desc_dim, netvlad_dim),
                                    d2fe_block_words_d(cap, desc_dim, netvlad_dim), renorm, d_blocks, stream ? (hipStream_t)stream : h->stream));
  return D2FE_OK;
}
int d2fe_unpack_blocks_int8_device(d2fe_handle h, const int8_t* d_blocks_int8, int nblocks, int cap, int netvlad_dim, int renorm,
                                   float* d_blocks, void* stream) {
  return d2fe_unpack_blocks_int8_device_d(h, d_blocks_int8, nblocks, cap, 256, netvlad_dim, renorm, d_blocks, stream);
}

int d2fe_quad_gate_device(d2fe_handle h, const float* d_local, size_t local_stride, const float* d_remote, size_t remote_stride, int dim,
                          const int32_t* d_job_local_row0, const int32_t* d_job_remote_row0, int local_view_step, int remote_view_step,
                          int njobs, double thres, int32_t* d_dir_prev, float* d_sims, int32_t* d_cnt_inout, int32_t* d_n_pass,
                          void* stream) {
  if (!h || !d_local || !d_remote || !d_job_local_row0 || !d_job_remote_row0) return fail(D2FE_ERR_INVALID, "null argument");
  if (njobs < 1 || dim < 4 || (dim & 3) || local_view_step < 1 || remote_view_step < 1) return fail(D2FE_ERR_INVALID, "bad geometry");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  HIP_TRY(launch_quad_gate(d_local, (long)local_stride, d_remote, (long)remote_stride, dim, d_job_local_row0, d_job_remote_row0,
                           local_view_step, remote_view_step, njobs, thres, d_dir_prev, d_sims, d_cnt_inout, d_n_pass,
                           stream ? (hipStream_t)stream : h->stream));
  return D2FE_OK;
}

float d2fe_half_move_cols(int width_undistort, double undistort_fov) { return (float)((double)width_undistort * 90.0 / undistort_fov); }
int d2fe_half_image_compact_device(d2fe_handle h, const float* d_desc, const float* d_pts_xy, const int32_t* d_n, const int32_t* d_job_row,
                                   const int32_t* d_job_left, const float* d_job_shift_x, int njobs, int cap, int dim, int width_undistort,
                                   double undistort_fov, float* d_out_desc, float* d_out_pts, int32_t* d_out_map, int32_t* d_out_n,
                                   void* stream) {
  if (!h || !d_desc || !d_pts_xy || !d_n || !d_job_row || !d_job_left || !d_job_shift_x || !d_out_desc || !d_out_pts || !d_out_map || !d_out_n)
    return fail(D2FE_ERR_INVALID, "null argument");
  if (njobs < 1 || cap < 1 || cap > 1024 || dim < 4 || (dim & 3) || width_undistort < 1 || !(undistort_fov > 0)) return fail(D2FE_ERR_INVALID, "bad geometry");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  HIP_TRY(launch_half_compact(d_desc, d_pts_xy, d_n, d_job_row, d_job_left, d_job_shift_x, njobs, cap, dim, (float)width_undistort,
                              d2fe_half_move_cols(width_undistort, undistort_fov), d_out_desc, d_out_pts, d_out_map, d_out_n,
                              stream ? (hipStream_t)stream : h->stream));
  return D2FE_OK;
}
int d2fe_remap_matches_device(d2fe_handle h, int32_t* d_q_idx, int32_t* d_t_idx, const int32_t* d_n_match, const int32_t* d_map_a_job,
                              const int32_t* d_map_b_job, const int32_t* d_maps, int npairs, int cap_match, int cap_map, void* stream) {
  if (!h || !d_q_idx || !d_t_idx || !d_n_match || !d_map_a_job || !d_map_b_job || !d_maps) return fail(D2FE_ERR_INVALID, "null argument");
  if (npairs < 1 || cap_match < 1 || cap_map < 1) return fail(D2FE_ERR_INVALID, "bad geometry");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  HIP_TRY(launch_remap_matches(d_q_idx, d_t_idx, d_n_match, d_map_a_job, d_map_b_job, d_maps, npairs, cap_match, cap_map,
                               stream ? (hipStream_t)stream : h->stream));
  return D2FE_OK;
}

int d2fe_half_image_filter(const float* pts_xy, int n, int require_left, int width_undistort, double undistort_fov,
                           int32_t* map, int* n_out) {
  if (!n_out) return fail(D2FE_ERR_INVALID, "null argument");
  *n_out = 0;
  if (n < 0 || (n > 0 && (!pts_xy || !map))) return fail(D2FE_ERR_INVALID, "null pointer");
  // host bookkeeping on <= N points (d2featuretracker.cpp:1058-1071); float move_cols as in the reference
  const float move_cols = (float)((double)width_undistort * 90.0 / undistort_fov);
  int c = 0;
  for (int i = 0; i < n; ++i) {
    const float x = pts_xy[2 * i];
    if ((require_left && x < (float)width_undistort - move_cols) || (!require_left && x >= move_cols)) map[c++] = i;
  }
  *n_out = c;
  return D2FE_OK;
}

}  // extern "C"
