"""The cylindrical camera model of the bearings pass on the host (no GPU).  The oracle tests/helpers/cyl_bearings_ref.py is pinned to the reference where the reference
is compiled under oracle/_ref: its lift, through oracle.ref.gen_cylinder_map (CylindricalCamera::liftProjective -> CataCamera::spaceToPlane, compiled in place).
CylindricalCamera::spaceToPlane is NOT compiled there and is restated, in the oracle and in include/d2fe.hpp; the two restatements are held to each other bit for bit, as
are the other host restatements the mode uses.  The rest checks what tests/test_quad_bearings.py's bounds assume about the oracle and about its tolerance set."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from oracle import ref as spref
from tests.helpers import bearings_ref as br
from tests.helpers import cyl_bearings_ref as cr
from tests.test_next_rows import QUADCAM_MEI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUADCAM = br.mei(**QUADCAM_MEI)
VIEW = cr.CAMS["view"]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.skipif(not spref.available(), reason="oracle/_ref/libspref.so is absent and cannot be built here")
@pytest.mark.parametrize("w,h,fov", [(800, 400, 200.0), (200, 120, 200.0), (64, 48, 190.0)])
def test_lift_equals_the_reference_through_the_map(w, h, fov):
    """every pixel of the view lifted by the oracle and projected with the quadcam MEI camera equals the reference's own map, bit for bit after the cast to float"""
    yy, xx = np.mgrid[0:h, 0:w]
    pts = np.stack([xx.ravel(), yy.ravel()], 1).astype(np.float32)
    u, v = br.space_to_plane(QUADCAM, cr.lift(cr.cylinder_camera(w, h, fov), pts))
    mx, my = spref.gen_cylinder_map(br.mei9(QUADCAM), w, h, fov)
    assert np.array_equal(u.astype(np.float32).reshape(h, w), mx, equal_nan=True) and np.array_equal(v.astype(np.float32).reshape(h, w), my, equal_nan=True)


def test_the_seam_lies_on_integer_columns():
    """800 wide at 200 degrees: column 40 is the last one in front (z = +1, tan about -1.6e16), column 760 the first one behind (z = -1)"""
    phi, _ = cr.angles(VIEW, np.float32([[40, 200], [760, 200]]))
    assert phi[0] == -1.5707963267948966 and phi[1] == 1.5707963267948968 and not abs(phi[0]) > cr.HALF_PI and abs(phi[1]) > cr.HALF_PI
    P = cr.lift(VIEW, np.float32([[40, 200], [760, 200]]))
    assert P[0, 2] == 1.0 and P[1, 2] == -1.0 and P[0, 0] < -1e16 and 1e15 < P[1, 0] < 1e16      # x = z tan(phi): (+1)(-1.6e16) and (-1)(-6.2e15)
    assert 40 in cr.seam_columns(VIEW, 800) and 760 in cr.seam_columns(VIEW, 800)


@pytest.fixture(scope="module")
def wrap(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("cyl_bearings_wrap") / "libcyl_bearings_wrap.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "cyl_bearings_wrap.cpp"), "-o", so])
    L = C.CDLL(so)
    L.cw_predict.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p]
    return L


def _points():
    rng = np.random.RandomState(31)
    return np.concatenate([rng.rand(600, 2) * [800, 400], [[0, 0], [799, 0], [0, 399], [799, 399]], [[40, 200], [760, 200], [39, 0], [761, 399]],
                           [[-40, 460]]]).astype(np.float32)


@pytest.mark.parametrize("name", list(cr.CAMS))
def test_hpp_helpers_equal_the_oracle(wrap, name):
    """include/d2fe.hpp's liftProjectiveCylindrical, unitBearing, predictWithExtrinsic and spaceToPlaneCylindrical (g++ -O2 -ffp-contract=off) against the oracle, bit for
    bit: 600 seeded points of the 800 x 400 view, its corners, the seam columns and their neighbours, one point outside the view."""
    cam = cr.CAMS[name]
    cc = np.array([cam[k] for k in ("fx", "fy", "cx", "cy")], np.float64)
    pts = _points()
    n = len(pts)
    P = np.zeros((n, 3)); b = np.zeros((n, 3))
    wrap.cw_lift(_p(cc), _p(pts), n, _p(P))
    want = cr.lift(cam, pts)
    assert np.isfinite(want).all() and np.array_equal(P, want)
    wrap.cw_unit(_p(np.ascontiguousarray(want)), n, _p(b))
    wb = br.normalise(want)
    assert np.array_equal(b, wb)
    for dist, T in cr.SETTINGS:
        X = np.zeros((n, 3))
        wrap.cw_predict(_p(T), _p(np.ascontiguousarray(wb)), n, dist, _p(X))
        wX = br.transform(T, wb, dist)
        assert np.array_equal(X, wX)
        uv = np.zeros((n, 2))
        wrap.cw_s2p(_p(cc), _p(np.ascontiguousarray(wX)), n, _p(uv))
        u, v = cr.space_to_plane(cam, wX)
        assert np.array_equal(uv[:, 0], u, equal_nan=True) and np.array_equal(uv[:, 1], v, equal_nan=True) and np.isfinite(u).all()
    # on the camera's plane, behind it, on the axis (rho = 0: u = 0 / 0 = NaN, v = fy Y / 0 = inf -- neither is a pixel) and straight ahead
    Q = np.array([[0.3, -0.2, 0.0], [0.3, -0.2, -2.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], np.float64)
    uv = np.zeros((len(Q), 2))
    wrap.cw_s2p(_p(cc), _p(Q), len(Q), _p(uv))
    u, v = cr.space_to_plane(cam, Q)
    assert np.array_equal(uv[:, 0], u, equal_nan=True) and np.array_equal(uv[:, 1], v, equal_nan=True)
    assert np.isnan(uv[2, 0]) and np.isposinf(uv[2, 1]) and np.isfinite(uv[[0, 1, 3]]).all() and uv[3, 0] == cam["cx"] and uv[3, 1] == cam["cy"]


def _ulp_error(got, true):
    """|got - true| in units in the last place of `true` (an mpmath number), as a float"""
    import mpmath
    e = math.frexp(float(true))[1]
    return float(abs(mpmath.mpf(got) - true) / mpmath.ldexp(1, e - 53))


def test_oracle_tan_and_atan2_are_within_one_ulp():
    """what cyl_bearing_bound and the predictions' bound assume of the oracle side: math.tan on every phi of the GPU tests' tolerance set and math.atan2 on every
    transformed point, against mpmath at 200 bits"""
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.prec = 200
    worst_tan = worst_atan2 = 0.0
    for name, cam in cr.CAMS.items():
        pts = np.unique(np.concatenate([cr.tolerance_points(name, cap).reshape(-1, 2) for cap in cr.CAPS]), axis=0)
        phi, _ = cr.angles(cam, pts)
        for v in np.unique(phi):
            worst_tan = max(worst_tan, _ulp_error(math.tan(v), mpmath.tan(mpmath.mpf(float(v)))))
        b = cr.bearings(cam, pts)
        for dist, T in cr.SETTINGS:
            X = br.transform(T, b, dist)
            for x, z in zip(X[::7, 0], X[::7, 2]):
                worst_atan2 = max(worst_atan2, _ulp_error(math.atan2(x, z), mpmath.atan2(mpmath.mpf(float(x)), mpmath.mpf(float(z)))))
    print("oracle tan: %.3f ulp, atan2: %.3f ulp at worst" % (worst_tan, worst_atan2))
    assert worst_tan <= 1.0 and worst_atan2 <= 1.0


def test_tolerance_set_is_well_conditioned():
    """every bearing of the set is finite and its bound a few dozen units of 2^-52 of the component; |y / rho| <= 0.88 over the view, so after either transform at
    either distance rho_b >= 1 (the projection never divides by something small).  Points within BACK_SEAM of atan2's jump after the transform are left out of the
    prediction comparison: a condition on the inputs, at most 1 % of the set -- and under the 90-degree yaw at distance 100 exactly the points of the one seam column"""
    for name, cam in cr.CAMS.items():
        total, left_out = 0, [0] * len(cr.SETTINGS)
        for cap in cr.CAPS:
            pts = cr.tolerance_points(name, cap).reshape(-1, 2)
            total += len(pts)
            phi, ybr = cr.angles(cam, pts)
            assert np.abs(ybr).max() <= 0.88 and np.abs(phi).max() > cr.HALF_PI
            b = cr.bearings(cam, pts)
            assert np.isfinite(b).all()
            bound = cr.cyl_bearing_bound(cam, pts)
            assert (bound <= 28 * cr.U * np.abs(b) * (1 + 2.0 ** -19)).all()       # relative, on the seam columns too: the bound is not a loophole
            seam = cr.seam_columns(cam, cr.VIEW_W)
            assert all((pts[:, 0] == c).any() for c in seam) or cap < 64
            for i, (dist, T) in enumerate(cr.SETTINGS):
                X = br.transform(T, b, dist)
                assert np.sqrt(X[:, 0] * X[:, 0] + X[:, 2] * X[:, 2]).min() >= 1.0, (name, dist)
                out = cr.near_back_seam(X)
                left_out[i] += int(out.sum())
                if T is cr.T_YAW and dist == 100.0:      # phi_b = phi_a + pi / 2: the back seam of b is the column where phi_a = pi / 2
                    x_seam = cam["cx"] + cr.HALF_PI * cam["fx"]
                    assert (np.abs(pts[out, 0] - x_seam) < 0.5).all(), name
                u, v = cr.space_to_plane(cam, X[~out])
                assert np.isfinite(u).all() and np.isfinite(v).all()
        print(name, "left out of the prediction comparison:", left_out, "of", total)
        assert max(left_out) <= 0.01 * total, (name, left_out, total)
        assert left_out[0] == left_out[1] == 0, name                              # a one-degree rotation brings nothing near the back seam


@pytest.mark.parametrize("w,h,fov", [(800, 400, 200.0), (200, 120, 200.0), (64, 48, 190.0), (801, 401, 185.5)])
def test_cylinder_camera(w, h, fov):
    """d2fe_cylinder_camera (a host function: no device is touched): the focal length of the map generator, the integer centre, bit for bit"""
    from d2slam_amd import api
    c = api.cylinder_camera(w, h, fov)
    f = w / (fov * (math.pi / 180.0))
    assert c.kind == api.CAM_CYLINDRICAL == 3 and list(c.p) == [f, f, float(w // 2), float(h // 2), 0, 0, 0, 0, 0]
    want = cr.cylinder_camera(w, h, fov)
    assert [want[k] for k in ("fx", "fy", "cx", "cy")] == list(c.p)[:4]
    m = api.camera_cylindrical(1.5, 2.5, 3.5, 4.5)
    assert m.kind == 3 and list(m.p) == [1.5, 2.5, 3.5, 4.5, 0, 0, 0, 0, 0]
    for bad in ((0, h, fov), (w, 0, fov), (w, h, 0.0), (w, h, float("nan"))):
        with pytest.raises(api.D2FEError) as e:
            api.cylinder_camera(*bad)
        assert e.value.code == -1


def test_the_abi_knows_the_new_symbols():
    from d2slam_amd import api
    for n in ("d2fe_cylinder_camera", "d2fe_quad_bearings_default", "d2fe_quad_bearings_enable", "d2fe_quad_bearings_result_get"):
        assert n in api.EXPORTS and hasattr(api.load_library(), n)
    b = api._QuadBearings()
    api.load_library().d2fe_quad_bearings_default(C.byref(b))
    assert C.sizeof(api._QuadBearings) == 8 + 4 * 80 + 48 * 8 + 16 and b.struct_size == C.sizeof(api._QuadBearings)
    assert b.lk_use_pred == 1 and b.distance == 100.0 and b.radius_lk == 0.0 and list(b.T_nb) == list(np.eye(3, 4).ravel()) * 4
    assert all(b.cam[c].kind == 0 and not any(b.cam[c].p) for c in range(4))
    assert C.sizeof(api._QuadBearingsResult) == 16 + 5 * 8
