// bearings.hip -- the per-point pass the reference's tracker runs on everything the front end returns: the unit bearing of every keypoint and list entry
// (LoopCam::extractorImgDescDeepnet, loop_cam.cpp:619-645; D2FeatureTracker::createLKLandmark, d2featuretracker.cpp:777-802), the prediction of a left point in the right
// image through the stereo extrinsic (predictLandmarksWithExtrinsic, :1296-1313) and the lk_lk_use_pred gate of trackLK(left, right) (:742-744).  For the pipe
// (d2fe_pipe_bearings_enable, pipe.hip), the quad pipe (d2fe_quad_bearings_enable, quad_pipe.hip) and for callers of d2fe_bearings_device.
//
// Arithmetic contract: fp64, one operation per operation of the host restatement in include/d2fe.hpp (liftProjectivePinhole, liftProjectiveMEI,
// liftProjectiveCylindrical, fillLandmarks, predictWithExtrinsic, spaceToPlanePinhole, spaceToPlaneMEI, spaceToPlaneCylindrical), in that order; the library is built
// with -ffp-contract=off.  The projection of the prediction uses the camera the point was LIFTED with, as the reference does (cams.at(left camera_index), :1309).
//
// One small launch, shaped like depth_gather_kernel: blockIdx.y = (segment, list), 64 threads stride over the list's `cap` slots; counts are read on the device and
// clamped to 0..cap, slots >= n are written as zero in every output.  The kernel is instantiated on "some camera of this launch is cylindrical": tan and atan2 of the
// device math library (and the private segment their large-argument reduction may take) exist in that instantiation alone, the pinhole / MEI launch has neither.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "../../include/d2fe.h"
#include "camera_device.h"
#include "context.h"

using namespace d2fe;

namespace {

struct BearArgs {
  BearCams c;
  int n_lists, n_segs;
  BearSeg seg[3];
};

// PinholeCamera::distortion / CataCamera::distortion (the same polynomial); k = k1 k2 p1 p2
__device__ __forceinline__ void radtan_distortion(const double* k, double mx, double my, double& dx, double& dy) {
  const double mx2 = mx * mx, my2 = my * my, mxy = mx * my, rho2 = mx2 + my2;
  const double rad = k[0] * rho2 + k[1] * rho2 * rho2;
  dx = mx * rad + 2.0 * k[2] * mxy + k[3] * (rho2 + 2.0 * mx2);
  dy = my * rad + 2.0 * k[3] * mxy + k[2] * (rho2 + 2.0 * my2);
}

__device__ __forceinline__ const double* radtan_of(const BearCam& c) { return c.kind == D2FE_CAM_MEI ? c.p + 1 : c.p + 4; }

// liftProjective + the normalisation of fillLandmarks: b = P / |P|
template <bool CYL>
__device__ __forceinline__ void lift_unit(const BearCam& c, float x, float y, double* b) {
  const double mx_d = c.iK11 * (double)x + c.iK13, my_d = c.iK22 * (double)y + c.iK23;
  if (CYL && c.kind == D2FE_CAM_CYLINDRICAL) {      // CylindricalCamera::liftProjective (CylindricalCamera.cc:207-220): mx_d = phi, my_d = y / rho
    const double z = __builtin_fabs(mx_d) > M_PI / 2 ? -1.0 : 1.0;
    const double X = z * tan(mx_d);
    const double rho = __builtin_sqrt(X * X + z * z);
    const double Y = my_d * rho;
    const double n = __builtin_sqrt(X * X + Y * Y + z * z);
    b[0] = X / n; b[1] = Y / n; b[2] = z / n;
    return;
  }
  double mx_u = mx_d, my_u = my_d;
  if (c.distort) {      // the recursive distortion model, n = 8
    const double* k = radtan_of(c);
    double dx, dy;
    radtan_distortion(k, mx_d, my_d, dx, dy);
    mx_u = mx_d - dx; my_u = my_d - dy;
    for (int i = 1; i < 8; ++i) {
      radtan_distortion(k, mx_u, my_u, dx, dy);
      mx_u = mx_d - dx; my_u = my_d - dy;
    }
  }
  double z = 1.0;
  if (c.kind == D2FE_CAM_MEI) {
    const double xi = c.p[0];
    if (xi == 1.0) {
      z = (1.0 - mx_u * mx_u - my_u * my_u) / 2.0;
    } else {
      const double rho2 = mx_u * mx_u + my_u * my_u;
      z = 1.0 - xi * (rho2 + 1.0) / (xi + __builtin_sqrt(1.0 + (1.0 - xi * xi) * rho2));
    }
  }
  const double n = __builtin_sqrt(mx_u * mx_u + my_u * my_u + z * z);
  b[0] = mx_u / n; b[1] = my_u / n; b[2] = z / n;
}

// predictLandmarksWithExtrinsic: T * (b * distance), then spaceToPlane of the lifting camera
template <bool CYL>
__device__ __forceinline__ void predict(const double* T, double distance, const BearCam& c, const double* b, float& pu, float& pv) {
  const double Lx = b[0] * distance, Ly = b[1] * distance, Lz = b[2] * distance;
  const double X = ((T[0] * Lx + T[1] * Ly) + T[2] * Lz) + T[3];
  const double Y = ((T[4] * Lx + T[5] * Ly) + T[6] * Lz) + T[7];
  const double Z = ((T[8] * Lx + T[9] * Ly) + T[10] * Lz) + T[11];
  double u, v;
  if (CYL && c.kind == D2FE_CAM_CYLINDRICAL) {
    // CylindricalCamera::spaceToPlane (CylindricalCamera.cc:228-238): K * (rho * phi, Y, rho) with the K of the constructor FisheyeUndist calls (:138-150), its zero
    // entries multiplied out as the matrix product does (a non-finite Y reaches u as well), then the division by the third row
    const double rho = __builtin_sqrt(X * X + Z * Z);
    const double phi = atan2(X, Z);
    const double ar = rho * phi;
    const double uh = (c.p[0] * ar + 0.0 * Y) + c.p[2] * rho;
    const double vh = (0.0 * ar + c.p[1] * Y) + c.p[3] * rho;
    const double w = (0.0 * ar + 0.0 * Y) + 1.0 * rho;
    u = uh / w;
    v = vh / w;
  } else if (c.kind == D2FE_CAM_MEI) {
    mei_space_to_plane(c.p, X, Y, Z, u, v);
  } else {      // PinholeCamera::spaceToPlane (PinholeCamera.cc:399-418)
    const double pu0 = X / Z, pu1 = Y / Z;
    double pd0 = pu0, pd1 = pu1;
    if (c.distort) {
      double dx, dy;
      radtan_distortion(c.p + 4, pu0, pu1, dx, dy);
      pd0 = pu0 + dx; pd1 = pu1 + dy;
    }
    u = c.p[0] * pd0 + c.p[2];
    v = c.p[1] * pd1 + c.p[3];
  }
  pu = (float)u; pv = (float)v;
}

template <bool CYL>
__global__ __launch_bounds__(64) void bearings_kernel(BearArgs a) {
  const int sl = blockIdx.y, sg = sl / a.n_lists, l = sl - sg * a.n_lists;
  if (sg >= a.n_segs) return;
  const BearSeg& S = a.seg[sg];
  const int j = S.by4 ? l & 3 : 0, ls = S.by4 ? (l & ~3) + S.src[j] : l;      // the list's cameras and extrinsic; the list its points come from
  int n = S.n[(size_t)ls * S.n_stride];
  n = n < 0 ? 0 : n > S.cap ? S.cap : n;
  const size_t cap = (size_t)S.cap;
  const float* pts = S.pts + (size_t)ls * S.pts_stride;
  double* bearing = S.bearing ? S.bearing + (size_t)l * S.bearing_step * cap * 3 : nullptr;
  float* pred = S.pred ? S.pred + (size_t)l * cap * 2 : nullptr;
  const bool gate = S.pred_ok != nullptr;
  const float* other = gate ? S.other + (size_t)l * S.other_stride : nullptr;
  const uint8_t* status = gate ? S.status + (size_t)l * S.status_stride : nullptr;
  double* other_bearing = gate ? S.other_bearing + (size_t)l * cap * 3 : nullptr;
  uint8_t* pred_ok = gate ? S.pred_ok + (size_t)l * cap : nullptr;
  const BearCam& cam = a.c.cam[S.cam[j]];
  const BearCam& ocam = a.c.cam[S.ocam[j]];
  const double* T = a.c.T[S.ext[j]];
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < S.cap; i += gridDim.x * blockDim.x) {
    double b[3] = {0.0, 0.0, 0.0}, ob[3] = {0.0, 0.0, 0.0};
    float pu = 0.f, pv = 0.f;
    uint8_t ok = 0;
    if (i < n) {
      lift_unit<CYL>(cam, pts[2 * i], pts[2 * i + 1], b);
      if (pred) predict<CYL>(T, a.c.distance, cam, b, pu, pv);
      if (gate) {
        const float ox = other[2 * i], oy = other[2 * i + 1];
        lift_unit<CYL>(ocam, ox, oy, ob);
        // cv::norm(pred - other) < radius (nearer, lk_list_device.h): float differences, the squares exact in double; false for a NaN prediction
        const float dx = pu - ox, dy = pv - oy;
        const bool near = a.c.radius <= 0.0 || __builtin_sqrt((double)dx * (double)dx + (double)dy * (double)dy) < a.c.radius;
        ok = status[i] && near ? 1 : 0;
      }
    }
    if (bearing) { bearing[3 * (size_t)i] = b[0]; bearing[3 * (size_t)i + 1] = b[1]; bearing[3 * (size_t)i + 2] = b[2]; }
    if (pred) { pred[2 * (size_t)i] = pu; pred[2 * (size_t)i + 1] = pv; }
    if (gate) {
      other_bearing[3 * (size_t)i] = ob[0]; other_bearing[3 * (size_t)i + 1] = ob[1]; other_bearing[3 * (size_t)i + 2] = ob[2];
      pred_ok[i] = ok;
    }
  }
}

bool finite_nz(double v) { return std::isfinite(v) && v != 0.0; }

}  // namespace

namespace d2fe {

const char* bearings_check_camera(const d2fe_camera* c) {
  if (c->kind != D2FE_CAM_PINHOLE && c->kind != D2FE_CAM_MEI && c->kind != D2FE_CAM_CYLINDRICAL)
    return "unknown camera kind (D2FE_CAM_PINHOLE, D2FE_CAM_MEI or D2FE_CAM_CYLINDRICAL)";
  if (c->kind == D2FE_CAM_PINHOLE && (!finite_nz(c->p[0]) || !finite_nz(c->p[1]))) return "pinhole camera: fx and fy must be finite and not zero";
  if (c->kind == D2FE_CAM_CYLINDRICAL) {
    if (!finite_nz(c->p[0]) || !finite_nz(c->p[1])) return "cylindrical camera: fx and fy must be finite and not zero";
    for (int i = 4; i < 9; ++i) if (!(c->p[i] == 0.0)) return "cylindrical camera: p[4..8] must be 0 (the model has no distortion)";
  }
  if (c->kind == D2FE_CAM_MEI && (!finite_nz(c->p[5]) || !finite_nz(c->p[6]))) return "MEI camera: gamma1 and gamma2 must be finite and not zero";
  return nullptr;
}

BearCam bearings_make_camera(const d2fe_camera& c) {
  BearCam b{};
  b.kind = c.kind;
  for (int i = 0; i < 9; ++i) b.p[i] = c.p[i];
  const bool mei = c.kind == D2FE_CAM_MEI;
  const double fx = mei ? c.p[5] : c.p[0], fy = mei ? c.p[6] : c.p[1], cx = mei ? c.p[7] : c.p[2], cy = mei ? c.p[8] : c.p[3];
  const double* k = mei ? c.p + 1 : c.p + 4;
  b.iK11 = 1.0 / fx; b.iK13 = -cx / fx; b.iK22 = 1.0 / fy; b.iK23 = -cy / fy;
  b.distort = k[0] != 0 || k[1] != 0 || k[2] != 0 || k[3] != 0;
  return b;
}

int bearings_launch(d2fe_context* h, const BearCams& cams, int n_lists, const BearSeg* segs, int n_segs, hipStream_t s) {
  if (n_lists < 1 || n_segs < 1 || n_segs > 3 || n_lists * n_segs > 65535) return ctx_fail(D2FE_ERR_INVALID, "bearings: 1..3 segments, lists * segments <= 65535");
  BearArgs a{};
  a.c = cams; a.n_lists = n_lists; a.n_segs = n_segs;
  int cap = 1;
  for (int i = 0; i < n_segs; ++i) { a.seg[i] = segs[i]; cap = segs[i].cap > cap ? segs[i].cap : cap; }
  const int bx = (cap + 63) / 64;
  ProfScope ps(h, D2FE_PROF_LK, s);
  bool cyl = false;
  for (const BearCam& c : cams.cam) cyl = cyl || c.kind == D2FE_CAM_CYLINDRICAL;
  const dim3 grid(bx < 16 ? bx : 16, n_lists * n_segs);
  if (cyl) hipLaunchKernelGGL(bearings_kernel<true>, grid, dim3(64), 0, s, a);
  else hipLaunchKernelGGL(bearings_kernel<false>, grid, dim3(64), 0, s, a);
  HIP_TRY(hipGetLastError());
  return D2FE_OK;
}

}  // namespace d2fe

extern "C" {

int d2fe_relative_extrinsic(const double* q_a_wxyz, const double* t_a, const double* q_b_wxyz, const double* t_b, double* T_b_a) {
  if (!q_a_wxyz || !t_a || !q_b_wxyz || !t_b || !T_b_a) return ctx_fail(D2FE_ERR_INVALID, "null argument");
  auto rot = [](const double* q, double* R) {
    const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double w = q[0] / n, x = q[1] / n, y = q[2] / n, z = q[3] / n;
    R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z);       R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z);       R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y);       R[7] = 2.0 * (y * z + w * x);       R[8] = 1.0 - 2.0 * (x * x + y * y);
  };
  double Ra[9], Rb[9];
  rot(q_a_wxyz, Ra); rot(q_b_wxyz, Rb);
  const double d[3] = {t_a[0] - t_b[0], t_a[1] - t_b[1], t_a[2] - t_b[2]};
  for (int i = 0; i < 3; ++i) {      // row i of R_b^T = column i of R_b
    for (int j = 0; j < 3; ++j) T_b_a[4 * i + j] = (Rb[i] * Ra[j] + Rb[3 + i] * Ra[3 + j]) + Rb[6 + i] * Ra[6 + j];
    T_b_a[4 * i + 3] = (Rb[i] * d[0] + Rb[3 + i] * d[1]) + Rb[6 + i] * d[2];
  }
  return D2FE_OK;
}

int d2fe_bearings_device(d2fe_handle h, const d2fe_camera* cam, const d2fe_camera* cam_other, const double* T, double distance, const float* d_pts_xy, size_t pts_stride,
                         const int32_t* d_n, int n_lists, int cap, double* d_bearing, float* d_pred_xy, const float* d_other_xy, const uint8_t* d_other_status,
                         double radius, double* d_other_bearing, uint8_t* d_pred_ok, void* stream) {
  if (!h || !cam || !d_pts_xy || !d_n || !d_bearing) return ctx_fail(D2FE_ERR_INVALID, "null argument");
  if (n_lists < 1 || n_lists > 32767 || cap < 1 || cap > 16384 || (n_lists > 1 && pts_stride < (size_t)2 * cap)) return ctx_fail(D2FE_ERR_INVALID, "n_lists must be 1..32767, cap 1..16384, pts_stride >= 2 * cap");
  if (const char* why = bearings_check_camera(cam)) return ctx_fail(D2FE_ERR_INVALID, why);
  const bool gate = d_other_xy || d_other_status || d_other_bearing || d_pred_ok;
  if (gate && !(d_other_xy && d_other_status && d_other_bearing && d_pred_ok)) return ctx_fail(D2FE_ERR_INVALID, "the gate's four pointers (other_xy, other_status, other_bearing, pred_ok) are given together or not at all");
  if (gate && !d_pred_xy) return ctx_fail(D2FE_ERR_INVALID, "the gate compares the predicted points: d_pred_xy is needed with the gate outputs");
  if (d_pred_xy && !T) return ctx_fail(D2FE_ERR_INVALID, "d_pred_xy needs the extrinsic T");
  if (gate && !cam_other) return ctx_fail(D2FE_ERR_INVALID, "the gate lifts the other points with cam_other");
  if (cam_other) if (const char* why = bearings_check_camera(cam_other)) return ctx_fail(D2FE_ERR_INVALID, why);
  if (T) {
    if (!std::isfinite(distance)) return ctx_fail(D2FE_ERR_INVALID, "distance must be finite");
    for (int i = 0; i < 12; ++i) if (!std::isfinite(T[i])) return ctx_fail(D2FE_ERR_INVALID, "T must be finite");
  }
  if (gate && std::isnan(radius)) return ctx_fail(D2FE_ERR_INVALID, "radius must not be NaN");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  BearCams c{};
  c.cam[0] = bearings_make_camera(*cam);
  c.cam[1] = bearings_make_camera(cam_other ? *cam_other : *cam);
  if (T) for (int i = 0; i < 12; ++i) c.T[0][i] = T[i];
  c.distance = distance; c.radius = radius;
  BearSeg seg{};
  seg.pts = d_pts_xy; seg.pts_stride = pts_stride; seg.n = d_n; seg.n_stride = 1; seg.cap = cap; seg.ocam[0] = 1;
  seg.bearing = d_bearing; seg.bearing_step = 1; seg.pred = T ? d_pred_xy : nullptr;
  if (gate) {
    seg.other = d_other_xy; seg.other_stride = (size_t)2 * cap; seg.status = d_other_status; seg.status_stride = (size_t)cap;
    seg.other_bearing = d_other_bearing; seg.pred_ok = d_pred_ok;
  }
  return bearings_launch(h, c, n_lists, &seg, 1, stream ? (hipStream_t)stream : h->stream);
}

}  // extern "C"
