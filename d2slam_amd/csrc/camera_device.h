// camera_device.h -- the camodocal projection the map generation (next.hip) and the bearings kernel (bearings.hip) share, fp64, one operation per line of the reference
#pragma once
#include <hip/hip_runtime.h>

namespace d2fe {

// CataCamera::spaceToPlane (CataCamera.cc:495-515); cam = xi k1 k2 p1 p2 gamma1 gamma2 u0 v0
__device__ __forceinline__ void mei_space_to_plane(const double* cam, double X, double Y, double Z, double& u, double& v) {
  const double nrm = __builtin_sqrt(X * X + (Y * Y + Z * Z));
  const double z = Z + cam[0] * nrm;
  const double pu0 = X / z, pu1 = Y / z;
  const double mx2 = pu0 * pu0, my2 = pu1 * pu1, mxy = pu0 * pu1, rho2 = mx2 + my2;
  const double rad = cam[1] * rho2 + cam[2] * rho2 * rho2;
  const double d0 = pu0 * rad + 2.0 * cam[3] * mxy + cam[4] * (rho2 + 2.0 * mx2);
  const double d1 = pu1 * rad + 2.0 * cam[4] * mxy + cam[3] * (rho2 + 2.0 * my2);
  u = cam[5] * (pu0 + d0) + cam[7];
  v = cam[6] * (pu1 + d1) + cam[8];
}

}  // namespace d2fe
