// extern "C" view of the host restatements of include/d2fe.hpp that state the arithmetic of the bearings pass (liftProjectivePinhole, liftProjectiveMEI, unitBearing,
// spaceToPlanePinhole, spaceToPlaneMEI, predictWithExtrinsic), for tests/test_bearings_cpu.py: compiled with g++ -ffp-contract=off at test time, no GPU and no link
// against the library.  pin = fx fy cx cy k1 k2 p1 p2; mei = the nine doubles of d2fe_mei_camera
#include "d2fe.hpp"

using namespace D2FrontEnd;

static d2fe_mei_camera mei_of(const double* c) { return d2fe_mei_camera{c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8]}; }
static RadTan radtan_of(const double* k) { RadTan d; d.k1 = k[0]; d.k2 = k[1]; d.p1 = k[2]; d.p2 = k[3]; return d; }
static void put(const Vec3d& P, double* o) { o[0] = P.x; o[1] = P.y; o[2] = P.z; }

extern "C" void bw_lift_pinhole(const double* pin, const float* pts, int n, double* out) {
  for (int i = 0; i < n; ++i) put(liftProjectivePinhole(pin[0], pin[1], pin[2], pin[3], radtan_of(pin + 4), Point2f(pts[2 * i], pts[2 * i + 1])), out + 3 * i);
}
extern "C" void bw_lift_mei(const double* c, const float* pts, int n, double* out) {
  for (int i = 0; i < n; ++i) put(liftProjectiveMEI(mei_of(c), Point2f(pts[2 * i], pts[2 * i + 1])), out + 3 * i);
}
extern "C" void bw_unit(const double* P, int n, double* out) {
  for (int i = 0; i < n; ++i) put(unitBearing(Vec3d{P[3 * i], P[3 * i + 1], P[3 * i + 2]}), out + 3 * i);
}
extern "C" void bw_s2p_pinhole(const double* pin, const double* P, int n, double* uv) {
  for (int i = 0; i < n; ++i) spaceToPlanePinhole(pin[0], pin[1], pin[2], pin[3], radtan_of(pin + 4), Vec3d{P[3 * i], P[3 * i + 1], P[3 * i + 2]}, uv[2 * i], uv[2 * i + 1]);
}
extern "C" void bw_s2p_mei(const double* c, const double* P, int n, double* uv) {
  for (int i = 0; i < n; ++i) spaceToPlaneMEI(mei_of(c), Vec3d{P[3 * i], P[3 * i + 1], P[3 * i + 2]}, uv[2 * i], uv[2 * i + 1]);
}
extern "C" void bw_predict(const double* T, const double* b, int n, double distance, double* out) {
  for (int i = 0; i < n; ++i) put(predictWithExtrinsic(T, Vec3d{b[3 * i], b[3 * i + 1], b[3 * i + 2]}, distance), out + 3 * i);
}
