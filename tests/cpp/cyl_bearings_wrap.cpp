// extern "C" view of the host restatements of include/d2fe.hpp that state the arithmetic of the cylindrical model in the bearings pass (liftProjectiveCylindrical,
// unitBearing, predictWithExtrinsic, spaceToPlaneCylindrical), for tests/test_quad_bearings_cpu.py: compiled with g++ -O2 -ffp-contract=off at test time, no GPU and no
// link against the library.  cyl = fx fy cx cy
#include "d2fe.hpp"

using namespace D2FrontEnd;

static void put(const Vec3d& P, double* o) { o[0] = P.x; o[1] = P.y; o[2] = P.z; }

extern "C" void cw_lift(const double* cyl, const float* pts, int n, double* out) {
  for (int i = 0; i < n; ++i) put(liftProjectiveCylindrical(cyl[0], cyl[1], cyl[2], cyl[3], Point2f(pts[2 * i], pts[2 * i + 1])), out + 3 * i);
}
extern "C" void cw_unit(const double* P, int n, double* out) {
  for (int i = 0; i < n; ++i) put(unitBearing(Vec3d{P[3 * i], P[3 * i + 1], P[3 * i + 2]}), out + 3 * i);
}
extern "C" void cw_predict(const double* T, const double* b, int n, double distance, double* out) {
  for (int i = 0; i < n; ++i) put(predictWithExtrinsic(T, Vec3d{b[3 * i], b[3 * i + 1], b[3 * i + 2]}, distance), out + 3 * i);
}
extern "C" void cw_s2p(const double* cyl, const double* P, int n, double* uv) {
  for (int i = 0; i < n; ++i) spaceToPlaneCylindrical(cyl[0], cyl[1], cyl[2], cyl[3], Vec3d{P[3 * i], P[3 * i + 1], P[3 * i + 2]}, uv[2 * i], uv[2 * i + 1]);
}
