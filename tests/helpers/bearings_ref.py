"""NumPy float64 oracle of the bearings pass (d2slam_amd/csrc/bearings.hip, include/d2fe.h: d2fe_bearings_device, d2fe_relative_extrinsic): the lift of both camera
models, the normalisation, the extrinsic prediction, both spaceToPlane models and the gate, written one operation at a time in the order the header states.  NumPy neither
fuses nor reassociates, and its float64 `/` and `sqrt` are the correctly rounded IEEE operations.

Cameras are dicts: pinhole(fx, fy, cx, cy, k1, k2, p1, p2) or mei(xi, k1, k2, p1, p2, gamma1, gamma2, u0, v0).

PinholeCamera's two functions are not under oracle/_ref; they are restated here from PinholeCamera.cc:337-418.  Its distortion polynomial (:517-533) is the one the pinned
CataCamera shares (CataCamera.cc, held bit for bit to this file by tests/test_bearings_cpu.py through oracle.ref.cata_lift and gen_pinhole_map)."""
import numpy as np

U = 2.0 ** -52
MEI_KEYS = ("xi", "k1", "k2", "p1", "p2", "gamma1", "gamma2", "u0", "v0")


def pinhole(fx, fy, cx, cy, k1=0.0, k2=0.0, p1=0.0, p2=0.0):
    return dict(kind="pinhole", fx=float(fx), fy=float(fy), cx=float(cx), cy=float(cy), k1=float(k1), k2=float(k2), p1=float(p1), p2=float(p2))


def mei(xi, k1, k2, p1, p2, gamma1, gamma2, u0, v0):
    return dict(kind="mei", xi=float(xi), k1=float(k1), k2=float(k2), p1=float(p1), p2=float(p2), gamma1=float(gamma1), gamma2=float(gamma2), u0=float(u0), v0=float(v0))


def mei9(cam):
    return [cam[k] for k in MEI_KEYS]


def _f64(v):
    return np.float64(v)


def distortion(cam, mx, my):
    k1, k2, p1, p2 = _f64(cam["k1"]), _f64(cam["k2"]), _f64(cam["p1"]), _f64(cam["p2"])
    mx2 = mx * mx; my2 = my * my; mxy = mx * my; rho2 = mx2 + my2
    rad = k1 * rho2 + k2 * rho2 * rho2
    dx = mx * rad + _f64(2.0) * p1 * mxy + p2 * (rho2 + _f64(2.0) * mx2)
    dy = my * rad + _f64(2.0) * p2 * mxy + p1 * (rho2 + _f64(2.0) * my2)
    return dx, dy


def _has_distortion(cam):
    return any(cam[k] != 0 for k in ("k1", "k2", "p1", "p2"))


def lift(cam, pts, detail=None):
    """liftProjective: pts [n, 2] float32 -> rays [n, 3] float64 (not normalised).  detail (a dict): receives rho2 and, for MEI, frac = xi (rho2 + 1) / (xi + sqrt(..))"""
    p = np.asarray(pts, np.float32).reshape(-1, 2).astype(np.float64)
    with np.errstate(all="ignore"):
        if cam["kind"] == "pinhole":
            fx, fy, cx, cy = (_f64(cam[k]) for k in ("fx", "fy", "cx", "cy"))
        else:
            fx, fy, cx, cy = (_f64(cam[k]) for k in ("gamma1", "gamma2", "u0", "v0"))
        ik11 = _f64(1.0) / fx; ik13 = -cx / fx; ik22 = _f64(1.0) / fy; ik23 = -cy / fy
        mx_d = ik11 * p[:, 0] + ik13; my_d = ik22 * p[:, 1] + ik23
        mx_u, my_u = mx_d, my_d
        if _has_distortion(cam):
            dx, dy = distortion(cam, mx_d, my_d)
            mx_u = mx_d - dx; my_u = my_d - dy
            for _ in range(1, 8):
                dx, dy = distortion(cam, mx_u, my_u)
                mx_u = mx_d - dx; my_u = my_d - dy
        rho2 = mx_u * mx_u + my_u * my_u
        if cam["kind"] == "pinhole":
            z = np.ones_like(mx_u); frac = np.zeros_like(mx_u)
        else:
            xi = _f64(cam["xi"])
            if cam["xi"] == 1.0:
                frac = np.zeros_like(mx_u)
                z = (_f64(1.0) - mx_u * mx_u - my_u * my_u) / _f64(2.0)
            else:
                frac = xi * (rho2 + _f64(1.0)) / (xi + np.sqrt(_f64(1.0) + (_f64(1.0) - xi * xi) * rho2))
                z = _f64(1.0) - frac
    if detail is not None:
        detail["rho2"] = rho2; detail["frac"] = frac
    return np.stack([mx_u, my_u, z], 1)


def normalise(P):
    with np.errstate(all="ignore"):
        n = np.sqrt(P[:, 0] * P[:, 0] + P[:, 1] * P[:, 1] + P[:, 2] * P[:, 2])
        return np.stack([P[:, 0] / n, P[:, 1] / n, P[:, 2] / n], 1)


def bearings(cam, pts, detail=None):
    return normalise(lift(cam, pts, detail))


def space_to_plane(cam, P):
    """[n, 3] float64 -> (u, v) float64, PinholeCamera::spaceToPlane / CataCamera::spaceToPlane (the latter in the order of the library's mei_space_to_plane)"""
    X, Y, Z = P[:, 0], P[:, 1], P[:, 2]
    with np.errstate(all="ignore"):
        if cam["kind"] == "pinhole":
            pu0 = X / Z; pu1 = Y / Z
            pd0, pd1 = pu0, pu1
            if _has_distortion(cam):
                dx, dy = distortion(cam, pu0, pu1)
                pd0 = pu0 + dx; pd1 = pu1 + dy
            return _f64(cam["fx"]) * pd0 + _f64(cam["cx"]), _f64(cam["fy"]) * pd1 + _f64(cam["cy"])
        nrm = np.sqrt(X * X + (Y * Y + Z * Z))
        z = Z + _f64(cam["xi"]) * nrm
        pu0 = X / z; pu1 = Y / z
        dx, dy = distortion(cam, pu0, pu1)
        return _f64(cam["gamma1"]) * (pu0 + dx) + _f64(cam["u0"]), _f64(cam["gamma2"]) * (pu1 + dy) + _f64(cam["v0"])


def transform(T, b, distance):
    """predictLandmarksWithExtrinsic's point: T [12] (3 x 4 row-major) applied to b * distance"""
    T = np.asarray(T, np.float64).reshape(-1)
    with np.errstate(all="ignore"):
        L = b * _f64(distance)
        return np.stack([((T[4 * r] * L[:, 0] + T[4 * r + 1] * L[:, 1]) + T[4 * r + 2] * L[:, 2]) + T[4 * r + 3] for r in range(3)], 1)


def predict(cam, T, b, distance):
    """-> [n, 2] float32: spaceToPlane, of the camera the points were lifted with, of the transformed points"""
    u, v = space_to_plane(cam, transform(T, b, distance))
    with np.errstate(all="ignore"):
        return np.stack([u.astype(np.float32), v.astype(np.float32)], 1)


def gate(pred_xy, other_xy, status, radius):
    """pred_ok = status && (radius <= 0 || cv::norm(pred - other) < radius): float differences, the squares and their sum in double"""
    pred = np.asarray(pred_xy, np.float32).reshape(-1, 2); other = np.asarray(other_xy, np.float32).reshape(-1, 2)
    st = np.asarray(status).reshape(-1) != 0
    if radius <= 0:
        return st.astype(np.uint8)
    with np.errstate(all="ignore"):
        d = pred - other                                   # float32
        dx = d[:, 0].astype(np.float64); dy = d[:, 1].astype(np.float64)
        near = np.sqrt(dx * dx + dy * dy) < _f64(radius)      # False for NaN
    return (st & near).astype(np.uint8)


def rotation(q_wxyz):
    q = np.asarray(q_wxyz, np.float64).reshape(4)
    n = np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    w = q[0] / n; x = q[1] / n; y = q[2] / n; z = q[3] / n
    one, two = _f64(1.0), _f64(2.0)
    return np.array([[one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y)],
                     [two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x)],
                     [two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)]], np.float64)


def relative_extrinsic(q_a, t_a, q_b, t_b):
    """T_b_a [3, 4] = [R_b^T R_a | R_b^T (t_a - t_b)], dot products summed left to right"""
    Ra, Rb = rotation(q_a), rotation(q_b)
    d = np.asarray(t_a, np.float64).reshape(3) - np.asarray(t_b, np.float64).reshape(3)
    T = np.zeros((3, 4), np.float64)
    for i in range(3):
        for j in range(3):
            T[i, j] = (Rb[0, i] * Ra[0, j] + Rb[1, i] * Ra[1, j]) + Rb[2, i] * Ra[2, j]
        T[i, 3] = (Rb[0, i] * d[0] + Rb[1, i] * d[1]) + Rb[2, i] * d[2]
    return T


def quat_axis_angle(axis, deg):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    h = np.deg2rad(deg) / 2
    return np.array([np.cos(h), *(np.sin(h) * a)], np.float64)


def bearing_bound(cam, pts):
    """Per component, the largest |device - oracle| of a unit bearing that ONE assumption allows: every device sqrt and divide returns a value within one unit in the
    last place of the correctly rounded result (the oracle's `/` and sqrt ARE the correctly rounded ones).  Everything else is IEEE multiplication, addition and
    subtraction on identical operands, hence identical: in particular the whole pinhole lift and the 8-step undistortion of both models contain no divide and no sqrt
    (1 / fx and -cx / fx are computed on the host), so mx_u and my_u agree exactly.  With U = 2^-52 and ulp(v) <= U |v|:

      two correctly rounded results of operands that differ by d differ by at most d + ulp; the device adds one more ulp.  So an operation's output differs by
      (propagated input difference) + 2 U |output|.

      MEI z = 1 - frac, frac = xi (rho2 + 1) / (xi + q), q = sqrt(1 + (1 - xi^2) rho2):  dq <= U q;  den = xi + q: d_den <= U q + U den <= 2 U den (0 <= q <= den for
      xi > 0), the numerator is exact, so d_frac <= (2 U + 2 U) |frac| = 4 U |frac|;  e_z = d_z <= 4 U |frac| + U |z|.  (xi == 1: z = (..) / 2 is exact, e_z = 0; pinhole:
      z = 1, e_z = 0.)
      s = x x + y y + z z:  ds <= 2 |z| e_z + e_z^2 + U z^2 + U s  (z z differs by the propagated difference and one rounding, the last addition by one rounding)
      n = sqrt(s):          dn <= ds / (2 n) + 2 U n
      b_c = c / n:          db_c <= e_c / n + |c| dn / n^2 + 2 U |b_c|
    The second-order terms left out above (products of two differences) are covered by the factor (1 + 2^-20).  For the pinhole model this is 4 U |b_c| <= 4 U.
    Returns [n, 3] float64 (absolute).  Nothing here is fitted to what a device returns."""
    det = {}
    P = lift(cam, pts, det)
    x, y, z = np.abs(P[:, 0]), np.abs(P[:, 1]), np.abs(P[:, 2])
    e_z = 4 * U * np.abs(det["frac"]) + U * z if cam["kind"] == "mei" and cam["xi"] != 1.0 else np.zeros_like(z)
    s = x * x + y * y + z * z
    n = np.sqrt(s)
    ds = 2 * z * e_z + e_z * e_z + U * z * z + U * s
    dn = ds / (2 * n) + 2 * U * n
    out = np.stack([c * dn / (n * n) + 2 * U * c / n for c in (x, y, z)], 1)
    out[:, 2] += e_z / n
    return out * (1 + 2.0 ** -20)


def within_fp32_ulp(a, b):
    """|a - b| <= one fp32 unit in the last place of the larger magnitude (NaN only against NaN, inf only against the same inf)"""
    a = np.asarray(a, np.float32); b = np.asarray(b, np.float32)
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    with np.errstate(all="ignore"):
        close = np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)
    return same | (np.isfinite(a) & np.isfinite(b) & close)
