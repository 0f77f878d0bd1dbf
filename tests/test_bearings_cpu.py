"""The bearings pass on the host (no GPU): the NumPy oracle tests/helpers/bearings_ref.py is pinned to the reference's own camera code where that is compiled under
oracle/_ref (camodocal's CataCamera), the host restatements of include/d2fe.hpp are pinned to the oracle, and d2fe_relative_extrinsic -- a host function of the
library -- is pinned to the oracle.  All bit for bit: the same fp64 operations in the same order, no contraction."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import ref as spref
from tests.helpers import bearings_ref as br
from tests.test_next_rows import QUADCAM_MEI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUADCAM = br.mei(**QUADCAM_MEI)
# the pinhole camera of tests/cpp/mirror_test.cpp:100, and the same camera without distortion
PIN = br.pinhole(385.0, 386.0, 322.5, 241.0, 0.01, -0.02, 0.001, -0.0005)
PIN0 = br.pinhole(385.0, 386.0, 322.5, 241.0)
MEI0 = br.mei(QUADCAM["xi"], 0, 0, 0, 0, *[QUADCAM[k] for k in ("gamma1", "gamma2", "u0", "v0")])
MEI1 = br.mei(1.0, -0.1, 0.05, 1e-3, -1e-3, 900.0, 905.0, 630.0, 410.0)      # xi == 1: the parabolic branch


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.skipif(not spref.available(), reason="oracle/_ref/libspref.so is absent and cannot be built here")
def test_mei_lift_equals_camodocal():
    """CataCamera::liftProjective compiled in place, 4096 seeded points of a 1280 x 800 frame: bit for bit (NaN where the MEI ray does not exist, in both)"""
    pts = (np.random.RandomState(20250).rand(4096, 2) * [1280, 800]).astype(np.float32)
    want = spref.cata_lift(br.mei9(QUADCAM), pts)
    got = br.lift(QUADCAM, pts)
    assert np.array_equal(got, want, equal_nan=True)
    assert 0.2 < np.isfinite(want).all(1).mean() < 1.0


@pytest.mark.skipif(not spref.available(), reason="oracle/_ref/libspref.so is absent and cannot be built here")
def test_mei_space_to_plane_equals_camodocal():
    """gen_pinhole_map with the identity rotation is the reference's own CataCamera::spaceToPlane of (x - 32, y - 24, 300): entry by entry, bit for bit after the cast to float"""
    mx, my = spref.gen_pinhole_map(br.mei9(QUADCAM), [1, 0, 0, 0], 64, 48, 300.0)
    yy, xx = np.mgrid[0:48, 0:64].astype(np.float64)
    P = np.stack([xx.ravel() - 32.0, yy.ravel() - 24.0, np.full(64 * 48, 300.0)], 1)
    u, v = br.space_to_plane(QUADCAM, P)
    assert np.array_equal(u.astype(np.float32).reshape(48, 64), mx) and np.array_equal(v.astype(np.float32).reshape(48, 64), my)


@pytest.fixture(scope="module")
def wrap(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("bearings_wrap") / "libbearings_wrap.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "bearings_wrap.cpp"), "-o", so])
    L = C.CDLL(so)
    L.bw_predict.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p]
    return L


def _pin8(cam):
    return np.array([cam[k] for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2")], np.float64)


def _points(w, h, seed):
    rng = np.random.RandomState(seed)
    return np.concatenate([rng.rand(600, 2) * [w, h], [[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1], [-40, h + 60]]]).astype(np.float32)


@pytest.mark.parametrize("name", ["pin", "pin0", "quadcam", "mei0", "mei1"])
def test_hpp_helpers_equal_the_oracle(wrap, name):
    """include/d2fe.hpp's liftProjectivePinhole / liftProjectiveMEI, unitBearing, spaceToPlanePinhole / spaceToPlaneMEI and predictWithExtrinsic (g++, -ffp-contract=off)
    against the NumPy oracle, bit for bit.  PinholeCamera::liftProjective and ::spaceToPlane are not compiled under oracle/_ref: the oracle restates them from
    PinholeCamera.cc:337-418, and their distortion polynomial is the one the pinned CataCamera shares (the two tests above)."""
    cam = dict(pin=PIN, pin0=PIN0, quadcam=QUADCAM, mei0=MEI0, mei1=MEI1)[name]
    mei = cam["kind"] == "mei"
    pts = _points(1280, 800, 3) if mei else _points(640, 480, 4)
    cc = np.array(br.mei9(cam), np.float64) if mei else _pin8(cam)
    n = len(pts)
    P = np.zeros((n, 3)); b = np.zeros((n, 3))
    (wrap.bw_lift_mei if mei else wrap.bw_lift_pinhole)(_p(cc), _p(pts), n, _p(P))
    want = br.lift(cam, pts)
    assert np.array_equal(P, want, equal_nan=True)
    wrap.bw_unit(_p(np.ascontiguousarray(want)), n, _p(b))
    wb = br.normalise(want)
    assert np.array_equal(b, wb, equal_nan=True) and np.isfinite(wb).all(1).mean() > 0.2
    T = br.relative_extrinsic([1, 0, 0, 0], [0, 0, 0], br.quat_axis_angle([0.1, 1, 0.05], 1.0), [0.1, 0.004, -0.002]).reshape(-1)
    for dist in (100.0, 1.5):
        X = np.zeros((n, 3))
        wrap.bw_predict(_p(T), _p(np.ascontiguousarray(wb)), n, dist, _p(X))
        wX = br.transform(T, wb, dist)
        assert np.array_equal(X, wX, equal_nan=True)
        uv = np.zeros((n, 2))
        (wrap.bw_s2p_mei if mei else wrap.bw_s2p_pinhole)(_p(cc), _p(np.ascontiguousarray(wX)), n, _p(uv))
        u, v = br.space_to_plane(cam, wX)
        assert np.array_equal(uv[:, 0], u, equal_nan=True) and np.array_equal(uv[:, 1], v, equal_nan=True)
    # points behind the camera, on its plane and far off axis go through spaceToPlane too
    Q = np.array([[0.3, -0.2, 0.0], [0.3, -0.2, -2.0], [5.0, 4.0, 0.5], [0.0, 0.0, 1.0]], np.float64)
    uv = np.zeros((len(Q), 2))
    (wrap.bw_s2p_mei if mei else wrap.bw_s2p_pinhole)(_p(cc), _p(Q), len(Q), _p(uv))
    u, v = br.space_to_plane(cam, Q)
    assert np.array_equal(uv[:, 0], u, equal_nan=True) and np.array_equal(uv[:, 1], v, equal_nan=True)


@pytest.mark.parametrize("case", ["identity", "baseline", "rot3", "non_unit"])
def test_relative_extrinsic_equals_the_oracle(case):
    """d2fe_relative_extrinsic through ctypes (a host function: no device is touched) against the oracle, bit for bit"""
    from d2slam_amd import api
    qa, ta, qb, tb = dict(
        identity=([1, 0, 0, 0], [0, 0, 0], [1, 0, 0, 0], [0, 0, 0]),
        baseline=([1, 0, 0, 0], [0.02, 0, 0.1], [1, 0, 0, 0], [0.12, 0.001, 0.1]),
        rot3=(br.quat_axis_angle([0, 0, 1], 10.0), [0.3, -0.2, 1.0], br.quat_axis_angle([0.2, 1, -0.1], 3.0), [0.37, -0.21, 1.02]),
        non_unit=([2.0, 0.1, -0.3, 0.05], [1, 2, 3], [0.5, 0.5, -0.5, 0.49], [1.1, 2.0, 2.9]))[case]
    got = api.relative_extrinsic(qa, ta, qb, tb)
    want = br.relative_extrinsic(qa, ta, qb, tb)
    assert got.shape == (3, 4) and np.array_equal(got, want)
    if case == "identity":
        assert np.array_equal(got, np.eye(3, 4))
    if case == "baseline":
        assert np.array_equal(got[:, :3], np.eye(3)) and got[0, 3] == 0.02 - 0.12
    R = got[:, :3]
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-15 * 8


def test_the_abi_knows_the_new_symbols():
    from d2slam_amd import api
    for n in ("d2fe_relative_extrinsic", "d2fe_bearings_device", "d2fe_pipe_bearings_default", "d2fe_pipe_bearings_enable", "d2fe_pipe_bearings_result_get"):
        assert n in api.EXPORTS and hasattr(api.load_library(), n)
    b = api._PipeBearings()
    api.load_library().d2fe_pipe_bearings_default(C.byref(b))
    assert b.struct_size == C.sizeof(api._PipeBearings) and b.lk_use_pred == 1 and b.distance == 100.0 and list(b.T_right_left) == list(np.eye(3, 4).ravel())
