"""Float64 oracle of the cylindrical camera model in the bearings pass (D2FE_CAM_CYLINDRICAL of include/d2fe.h; d2slam_amd/csrc/bearings.hip): camodocal's
CylindricalCamera::liftProjective (CylindricalCamera.cc:207-220) and ::spaceToPlane (:228-238, with the K of the constructor FisheyeUndist calls, :138-150), one operation
at a time in the order the header states.  Everything but tan / atan2 is NumPy float64 (correctly rounded IEEE operations, nothing fused); tan and atan2 are Python's
math.tan / math.atan2 PER ELEMENT -- the C library's functions, which std::tan / std::atan2 of include/d2fe.hpp also are.  (np.tan takes a vector path here whose last
bit differs from math.tan's on some arguments.)

The lift is pinned to the reference through the map generation (tests/test_quad_bearings_cpu.py: oracle.ref.gen_cylinder_map, the reference's own liftProjective compiled in
place); spaceToPlane is a restatement -- the reference's function is not compiled under oracle/_ref.

Cameras are dicts: cylindrical(fx, fy, cx, cy).  normalise, transform, gate and within_fp32_ulp are bearings_ref's and are used from there."""
import math

import numpy as np

from tests.helpers import bearings_ref as br

U = br.U
K_TAN, K_ATAN2 = 5, 6        # the OpenCL full-profile limits for double precision (tan <= 5 ulp, atan2 <= 6 ulp), which the ROCm device library is built to conform to
HALF_PI = math.pi / 2        # M_PI / 2


def cylindrical(fx, fy, cx, cy):
    return dict(kind="cylindrical", fx=float(fx), fy=float(fy), cx=float(cx), cy=float(cy))


def cylinder_camera(width, height, fov_deg):
    """the virtual camera of FisheyeUndist (fisheye_undistort.h:492-495) as d2fe_cylinder_camera states it"""
    f = float(width) / (float(fov_deg) * (math.pi / 180.0))
    return cylindrical(f, f, width // 2, height // 2)


def _tan(a):
    return np.array([math.tan(v) if math.isfinite(v) else math.nan for v in np.asarray(a, np.float64).ravel()], np.float64).reshape(np.shape(a))


def _atan2(y, x):
    return np.array([math.atan2(a, b) for a, b in zip(np.asarray(y, np.float64).ravel(), np.asarray(x, np.float64).ravel())], np.float64).reshape(np.shape(y))


def angles(cam, pts):
    """phi and y / rho of the points: IEEE multiply and add on the host's 1 / fx, -cx / fx, 1 / fy, -cy / fy"""
    p = np.asarray(pts, np.float32).reshape(-1, 2).astype(np.float64)
    fx, fy, cx, cy = (np.float64(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    with np.errstate(all="ignore"):
        ik11 = np.float64(1.0) / fx; ik13 = -cx / fx; ik22 = np.float64(1.0) / fy; ik23 = -cy / fy
        return ik11 * p[:, 0] + ik13, ik22 * p[:, 1] + ik23


def lift(cam, pts):
    """liftProjective: pts [n, 2] float32 -> rays [n, 3] float64 (not normalised)"""
    phi, ybr = angles(cam, pts)
    with np.errstate(all="ignore"):
        z = np.where(np.abs(phi) > HALF_PI, np.float64(-1.0), np.float64(1.0))
        x = z * _tan(phi)
        rho = np.sqrt(x * x + z * z)
        y = ybr * rho
    return np.stack([x, y, z], 1)


def bearings(cam, pts):
    return br.normalise(lift(cam, pts))


def space_to_plane(cam, P):
    """[n, 3] float64 -> (u, v) float64: K * (rho * phi, Y, rho), the zero entries of K multiplied out, then the division by the third row"""
    P = np.asarray(P, np.float64)
    X, Y, Z = P[:, 0], P[:, 1], P[:, 2]
    fx, fy, cx, cy = (np.float64(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    zero, one = np.float64(0.0), np.float64(1.0)
    with np.errstate(all="ignore"):
        rho = np.sqrt(X * X + Z * Z)
        phi = _atan2(X, Z)
        a = rho * phi
        uh = (fx * a + zero * Y) + cx * rho
        vh = (zero * a + fy * Y) + cy * rho
        w = (zero * a + zero * Y) + one * rho
        return uh / w, vh / w


def predict(cam, T, b, distance):
    """-> [n, 2] float32: spaceToPlane, of the camera the points were lifted with, of the transformed points"""
    u, v = space_to_plane(cam, br.transform(T, b, distance))
    with np.errstate(all="ignore"):
        return np.stack([u.astype(np.float32), v.astype(np.float32)], 1)


def cyl_bearing_bound(cam, pts):
    """Per component, the largest |device - oracle| of a cylindrical unit bearing that three assumptions allow:
      (1) every device sqrt and divide returns a value within one unit in the last place of the correctly rounded result (bearing_bound's assumption);
      (2) the device's tan is within K_TAN = 5 ulp of the true value (and its atan2 within K_ATAN2 = 6 ulp: not used by the lift);
      (3) the oracle's tan is within 1 ulp of the true value (tests/test_quad_bearings_cpu.py checks this on the tolerance set against mpmath).
    Everything else is IEEE multiplication and addition.  phi = iK11 x + iK13 and ybr = iK22 y + iK23 come from identical operands (the four constants are computed on the
    host) and agree exactly, and so does z, a comparison of phi with the same constant.  Every later step is a product, a quotient, a square root or a sum of
    non-negative terms, so the errors are RELATIVE throughout; r(q) below bounds |q_device - q_oracle| / |q| in units of U = 2^-52 (ulp(v) <= U |v|).  Two correctly
    rounded results of operands whose relative difference is d differ by at most d + U; a device sqrt or divide adds one more U.

      X = z tan(phi), z = +-1:    r(X)  = K_TAN + 1 + 1          (device error + oracle error + the slack between "ulp of the true value" and "ulp of the result")
      XX = X X:                   r(XX) = 2 r(X) + 1
      s1 = XX + z z (z z = 1):    r(s1) = r(XX) + 1              (a sum of non-negative terms: the larger relative difference, one rounding)
      rho = sqrt(s1):             r(rho) = r(s1) / 2 + 2
      Y = ybr rho:                r(Y)  = r(rho) + 1
      YY = Y Y:                   r(YY) = 2 r(Y) + 1
      s = (XX + YY) + z z:        r(s)  = max(r(XX), r(YY)) + 2
      n = sqrt(s):                r(n)  = r(s) / 2 + 2
      b_c = c / n:                r(b_c) = r(c) + r(n) + 2,  r(z) = 0

    With K_TAN = 5: r(X) = 7, r(XX) = 15, r(rho) = 10, r(Y) = 11, r(YY) = 23, r(s) = 25, r(n) = 14.5, hence 23.5, 27.5 and 16.5 units of U times |b_x|, |b_y|, |b_z|.
    The second-order terms (products of two differences) are covered by the factor (1 + 2^-20).  Being relative, the bound does not blow up on the seam columns, where
    tan(phi) is about 1e16 and b_z about 6e-17: it is 16.5 U of THAT value.  Returns [n, 3] float64 (absolute).  Nothing here is fitted to what a device returns."""
    b = np.abs(bearings(cam, pts))
    r_x = K_TAN + 2.0
    r_xx = 2 * r_x + 1
    r_rho = (r_xx + 1) / 2 + 2
    r_y = r_rho + 1
    r_yy = 2 * r_y + 1
    r_n = (max(r_xx, r_yy) + 2) / 2 + 2
    rel = np.array([r_x + r_n + 2, r_y + r_n + 2, r_n + 2], np.float64) * U
    return b * rel * (1 + 2.0 ** -20)


# ---- the tolerance set of tests/test_quad_bearings.py (its conditions are checked on the host by tests/test_quad_bearings_cpu.py) ------------------------------------------
VIEW_W, VIEW_H, VIEW_FOV = 800, 400, 200.0
# the reference's 800 x 400 / 200 degree view, and a camera with fx != fy and an off-centre principal point on the same frame (|y / rho| <= 0.88 over the frame in both)
CAMS = {"view": cylinder_camera(VIEW_W, VIEW_H, VIEW_FOV), "skew": cylindrical(226.0, 240.0, 391.25, 207.5)}
CAPS = (1, 63, 64, 65, 1100)
N_LISTS = 2
# a one-degree rotation with a 0.1 m baseline, and the quad rig's geometry: camera b yawed by 90 degrees (phi_b = phi_a + pi / 2), 0.08 m apart
T_SMALL = br.relative_extrinsic([1, 0, 0, 0], [0, 0, 0], br.quat_axis_angle([0.1, 1, 0.05], 1.0), [0.1, 0.004, -0.002]).reshape(-1)
T_YAW = br.relative_extrinsic([1, 0, 0, 0], [0, 0, 0], br.quat_axis_angle([0, 1, 0], -90.0), [0.08, 0.0, 0.0]).reshape(-1)
SETTINGS = ((100.0, T_SMALL), (1.5, T_SMALL), (100.0, T_YAW), (1.5, T_YAW))
BACK_SEAM = 1e-3             # radians from atan2's jump within which a transformed point is left out of the prediction comparison


def seam_columns(cam, width):
    """the integer columns on either side of |phi| = pi / 2 (both seams), and their neighbours"""
    cols = []
    for s in (-1.0, 1.0):
        x = cam["cx"] + s * HALF_PI * cam["fx"]
        cols += [math.floor(x) - 1, math.floor(x), math.floor(x) + 1, math.floor(x) + 2]
    return [c for c in cols if 0 <= c < width]


def tolerance_points(name, cap, n_lists=N_LISTS):
    """[n_lists, cap, 2] float32: the seam columns and their neighbours at two heights, the four corners, the principal point, seeded integer pixels (what SuperPoint
    returns) and seeded sub-pixel points (what LK returns) inside the frame; nothing is excluded from this set"""
    cam = CAMS[name]
    w, h = VIEW_W, VIEW_H
    rng = np.random.RandomState(4000 * cap + n_lists)
    seam = [[c, y] for c in seam_columns(cam, w) for y in (h // 2, 0)]
    m = n_lists * cap
    pool = np.concatenate([seam, [[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1], [cam["cx"], cam["cy"]]],
                           np.stack([rng.randint(0, w, m), rng.randint(0, h, m)], 1), rng.rand(m, 2) * [w - 1, h - 1]]).astype(np.float32)
    return np.stack([np.roll(pool, -l * 5, 0)[:cap] for l in range(n_lists)])


def counts(cap):
    """above cap (clamped to cap) and half: 0 occurs at cap = 1"""
    return np.int32([cap + 5, cap // 2])


def near_back_seam(X):
    """transformed points [n, 3] within BACK_SEAM of atan2's jump (X_b ~ 0, Z_b < 0), where u moves by 2 pi fx"""
    with np.errstate(all="ignore"):
        return np.abs(_atan2(X[:, 0], X[:, 2])) > math.pi - BACK_SEAM
