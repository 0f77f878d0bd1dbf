"""Bearings, extrinsic predictions and their gate on the device (d2fe_bearings_device, d2fe_pipe_bearings_enable; d2slam_amd/csrc/bearings.hip) against the NumPy
float64 oracle tests/helpers/bearings_ref.py, which tests/test_bearings_cpu.py pins to the reference's own camera code.

The device's fp64 sqrt and divide need not return glibc's last bit (tests/test_next_rows.py records one such case), so nothing here compares their results bit
for bit with the host: bearings are held to bearings_ref.bearing_bound (derived from "within one unit in the last place", not measured), predictions to one fp32 unit
in the last place, the gate to the oracle's decision ON THE DEVICE'S OWN predictions, and the pipe to the single call on the ticket's own points (device against
device: the same code, the same bits)."""
import ctypes as C

import numpy as np
import pytest

from tests.helpers import bearings_ref as br
from tests.helpers import lk_carry_ref as lkref

# ---- cameras ----------------------------------------------------------------------------------------------------------------------------------------------------------
# pinhole: the camera of tests/cpp/mirror_test.cpp:100 on a 640 x 480 frame, with and without distortion.  MEI on a 1280 x 800 frame: focal lengths long enough that the whole
# frame lies within 45 degrees of the axis (every |Z| of the tolerance set stays above one metre at distance 1.5), with and without distortion, and xi == 1
CAMS = {
    "pin": (br.pinhole(385.0, 386.0, 322.5, 241.0, 0.01, -0.02, 0.001, -0.0005), 640, 480),
    "pin0": (br.pinhole(385.0, 386.0, 322.5, 241.0), 640, 480),
    "mei": (br.mei(1.2, -0.05, 0.01, -0.0009, 2e-5, 2100.0, 2090.0, 645.3, 398.7), 1280, 800),
    "mei0": (br.mei(1.2, 0, 0, 0, 0, 2100.0, 2090.0, 645.3, 398.7), 1280, 800),
    "mei1": (br.mei(1.0, -0.05, 0.01, -0.0009, 2e-5, 2100.0, 2090.0, 645.3, 398.7), 1280, 800),
}
OTHER = {"pin": "pin0", "pin0": "pin", "mei": "mei0", "mei0": "mei1", "mei1": "mei"}        # the second camera of a gated call
CAPS = (1, 63, 64, 65, 1100)
# stereo extrinsics: 0.1 m and 0.06 m baselines (within 0.05 .. 0.12), a one-degree rotation
T_A = br.relative_extrinsic([1, 0, 0, 0], [0, 0, 0], br.quat_axis_angle([0.1, 1, 0.05], 1.0), [0.1, 0.004, -0.002]).reshape(-1)
T_B = br.relative_extrinsic([1, 0, 0, 0], [0, 0, 0], br.quat_axis_angle([1, -0.3, 0.2], 1.0), [0.06, -0.002, 0.001]).reshape(-1)
DISTANCES = ((100.0, T_A), (1.5, T_B))


def api_camera(api, cam):
    if cam["kind"] == "pinhole":
        return api.camera_pinhole(*[cam[k] for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2")])
    return api.camera_mei(br.mei9(cam))


def tolerance_points(name, cap, n_lists):
    """[n_lists, cap, 2] float32: the four image corners, the principal point and seeded points inside the frame; nothing is excluded from this set"""
    cam, w, h = CAMS[name]
    pp = (cam["cx"], cam["cy"]) if cam["kind"] == "pinhole" else (cam["u0"], cam["v0"])
    rng = np.random.RandomState(1000 * cap + n_lists)
    pool = np.concatenate([[[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1], pp], rng.rand(n_lists * cap, 2) * [w - 1, h - 1]]).astype(np.float32)
    return np.stack([np.roll(pool, -l * 2, 0)[:cap] for l in range(n_lists)])


def counts(cap, n_lists):
    """0, cap, cap + 5 (clamped to cap) and -3 (-> 0) all occur over the shapes, and a partly filled list"""
    if n_lists == 1:
        return np.int32([{1: 0, 63: 63, 64: 64 + 5, 65: -3, 1100: 1100}[cap]])
    return np.int32([cap + 5, cap // 2, -3])


def test_tolerance_set_is_well_conditioned():
    """CPU: every point of the tolerance set has rho2 <= 4 and a ray of length >= 1 / 4 in the oracle (what bearing_bound's magnitudes rest on), and |Z| > 1 metre after
    either transform (the predictions' one-fp32-ulp bound rests on a projection that does not divide by something small)"""
    for name, (cam, w, h) in CAMS.items():
        for cap in CAPS:
            pts = tolerance_points(name, cap, 3).reshape(-1, 2)
            det = {}
            P = br.lift(cam, pts, det)
            assert np.isfinite(P).all() and det["rho2"].max() <= 4.0, name
            assert np.sqrt((P * P).sum(1)).min() >= 0.25, name
            b = br.normalise(P)
            assert br.bearing_bound(cam, pts).max() <= 64 * br.U, name        # a few dozen units of 2^-52 at most: the bound is not a loophole
            for dist, T in DISTANCES:
                X = br.transform(T, b, dist)
                assert np.abs(X[:, 2]).min() > 1.0, (name, dist, float(np.abs(X[:, 2]).min()))
                u, v = br.space_to_plane(cam, X)
                assert np.isfinite(u).all() and np.isfinite(v).all()


# ---- the single call --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    from d2slam_amd import api
    fe = api.FrontEnd(api.SuperPointConfig(input_width=64, input_height=64, max_batch=1))
    yield api, fe
    fe.close()


def run_device(api, fe, cam, pts, n, pad=0, cam_other=None, T=None, distance=100.0, other=None, status=None, radius=0.0, pred=None):
    """d2fe_bearings_device on [nl, cap, 2] points; the outputs are pre-filled with 0xFF bytes, so every slot >= n must have been WRITTEN as zero.
    pred: None = as T says.  Returns (bearing, pred_xy | None, other_bearing | None, pred_ok | None)"""
    import torch
    dev = torch.device("cuda")
    nl, cap = pts.shape[:2]
    stride = 2 * cap + pad
    hp = np.full((nl, stride), 7.25, np.float32); hp[:, :2 * cap] = pts.reshape(nl, -1)
    d_pts = torch.from_numpy(hp).to(dev); d_n = torch.from_numpy(np.ascontiguousarray(n, np.int32)).to(dev)
    fill = lambda nbytes: torch.full((nbytes,), -1, dtype=torch.int8, device=dev)
    d_b = fill(nl * cap * 24)
    want_pred = (T is not None) if pred is None else pred
    d_p = fill(nl * cap * 8) if want_pred else None
    gate = other is not None
    if gate:
        d_o = torch.from_numpy(np.ascontiguousarray(other, np.float32)).to(dev); d_s = torch.from_numpy(np.ascontiguousarray(status, np.uint8)).to(dev)
        d_ob = fill(nl * cap * 24); d_ok = fill(nl * cap)
    torch.cuda.synchronize()
    api.bearings_device(fe, api_camera(api, cam), d_pts.data_ptr(), stride, d_n.data_ptr(), nl, cap, d_b.data_ptr(), cam_other=None if cam_other is None else api_camera(api, cam_other),
                        T=T, distance=distance, d_pred_xy=d_p.data_ptr() if want_pred else None, d_other_xy=d_o.data_ptr() if gate else None,
                        d_other_status=d_s.data_ptr() if gate else None, radius=radius, d_other_bearing=d_ob.data_ptr() if gate else None,
                        d_pred_ok=d_ok.data_ptr() if gate else None)
    fe.sync()
    out = [d_b.cpu().numpy().view(np.float64).reshape(nl, cap, 3), d_p.cpu().numpy().view(np.float32).reshape(nl, cap, 2) if want_pred else None]
    out += [d_ob.cpu().numpy().view(np.float64).reshape(nl, cap, 3), d_ok.cpu().numpy().view(np.uint8).reshape(nl, cap)] if gate else [None, None]
    return out


def clamp(n, cap):
    return np.clip(np.asarray(n, np.int64), 0, cap)


def zero_beyond(a, n):
    return all(not a[l, n[l]:].view(np.uint8).any() for l in range(len(n)))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CAMS))
def test_single_call_against_the_oracle(ctx, name):
    api, fe = ctx
    cam = CAMS[name][0]
    oth = CAMS[OTHER[name]][0]
    equal = {"bearing": [0, 0], "pred": [0, 0]}
    for cap in CAPS:
        for nl in (1, 3):
            pts = tolerance_points(name, cap, nl)
            n = counts(cap, nl); nc = clamp(n, cap)
            wb = br.bearings(cam, pts.reshape(-1, 2)).reshape(nl, cap, 3)
            bound = br.bearing_bound(cam, pts.reshape(-1, 2)).reshape(nl, cap, 3)
            rng = np.random.RandomState(cap + nl)

            def check_bearing(got, want, bnd, what):
                assert zero_beyond(got, nc), (what, cap, nl)
                for l in range(nl):
                    g, w_ = got[l, :nc[l]], want[l, :nc[l]]
                    assert np.isfinite(g).all() and (np.abs(g - w_) <= bnd[l, :nc[l]]).all(), (what, cap, nl, l, float((np.abs(g - w_) / br.U).max()))
                    equal["bearing"][0] += int((g == w_).sum()); equal["bearing"][1] += g.size
            # bearings alone (no T, no outputs beyond d_bearing), lists further apart than 2 * cap floats
            got = run_device(api, fe, cam, pts, n, pad=6)
            check_bearing(got[0], wb, bound, "alone")
            for dist, T in DISTANCES:
                wp = br.predict(cam, T, wb.reshape(-1, 3), dist).reshape(nl, cap, 2)
                # prediction, and prediction + gate against points around the predicted ones
                other = (wp + rng.uniform(-30, 30, wp.shape)).astype(np.float32)
                status = (rng.rand(nl, cap) < 0.8).astype(np.uint8)
                wob = br.bearings(oth, other.reshape(-1, 2)).reshape(nl, cap, 3)
                ob_bound = br.bearing_bound(oth, other.reshape(-1, 2)).reshape(nl, cap, 3)
                for gate in (False, True):
                    got = run_device(api, fe, cam, pts, n, pad=2, cam_other=oth if gate else None, T=T, distance=dist, other=other if gate else None,
                                     status=status if gate else None, radius=25.0)
                    check_bearing(got[0], wb, bound, "with prediction")
                    assert zero_beyond(got[1], nc)
                    for l in range(nl):
                        g, w_ = got[1][l, :nc[l]], wp[l, :nc[l]]
                        assert br.within_fp32_ulp(g, w_).all(), (cap, nl, l, dist)
                        equal["pred"][0] += int((g == w_).sum()); equal["pred"][1] += g.size
                    if gate:
                        assert zero_beyond(got[2], nc) and zero_beyond(got[3], nc)
                        for l in range(nl):
                            k = nc[l]
                            if not np.isfinite(wob[l, :k]).all():
                                continue        # (an `other` point off the MEI disc: its class is the classes test's business)
                            assert (np.abs(got[2][l, :k] - wob[l, :k]) <= ob_bound[l, :k]).all()
                            # the gate, exact: the oracle's decision on the device's own predictions
                            assert np.array_equal(got[3][l, :k], br.gate(got[1][l, :k], other[l, :k], status[l, :k], 25.0))
    for k, (a, b) in equal.items():
        print("%s: %s bit-equal share %.6f (%d of %d)" % (name, k, a / max(b, 1), a, b))


@pytest.mark.gpu
def test_classes_of_special_points(ctx):
    """NaN, +-inf, +-1e9 coordinates; pinhole predictions with Z = 0 and Z < 0; MEI rays with Z + xi * norm <= 0: isnan / isinf / sign of every output equal the oracle's"""
    api, fe = ctx
    pin, mei_wide = CAMS["pin"][0], br.mei(0.5, -0.05, 0.01, -0.0009, 2e-5, 2100.0, 2090.0, 645.3, 398.7)
    nan, inf = np.nan, np.inf
    special = np.float32([[nan, 10], [10, nan], [nan, nan], [inf, 10], [10, -inf], [-inf, inf], [1e9, 10], [10, -1e9], [-1e9, 1e9], [1e9, 1e9], [320, 240], [5, 470], [0, 0]])
    ordinary = np.float32([[320, 240], [5, 470], [600, 20], [322.5, 241.0], [100, 100], [640, 400], [1279, 799], [0, 0]])
    T_z0 = np.float64([1, 0, 0, 0.1, 0, 1, 0, 0, 0, 0, 0, 0])            # Z = 0 for every finite point
    T_neg = np.float64([1, 0, 0, 0.1, 0, 1, 0, 0, 0, 0, -1, 0])          # Z < 0: behind the camera; MEI xi = 0.5: Z + xi * norm < 0 near the axis
    T_org = np.float64([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]); T_org2 = np.float64([0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0])     # X = Y = 0

    def cls(a):
        a = np.asarray(a, np.float64)
        with np.errstate(all="ignore"):
            return np.stack([np.isnan(a), np.isinf(a), np.where(np.isnan(a), 0, np.sign(a))])
    for cam, pts, T, dist in ((pin, special, T_A, 100.0), (mei_wide, special, T_A, 100.0), (CAMS["mei"][0], special, T_B, 1.5), (pin, ordinary, T_z0, 100.0),
                              (pin, ordinary, T_neg, 100.0), (mei_wide, ordinary, T_neg, 100.0), (mei_wide, ordinary, T_z0, 1.5), (pin, ordinary, T_org2, 1.5),
                              (mei_wide, ordinary, T_org, 100.0)):
        p = pts[None]
        n = np.int32([len(pts)])
        got = run_device(api, fe, cam, p, n, T=T, distance=dist)
        wb = br.bearings(cam, pts)
        wp = br.predict(cam, T, wb, dist)
        assert np.array_equal(cls(got[0][0]), cls(wb)), (cam["kind"], T.tolist())
        assert np.array_equal(cls(got[1][0]), cls(wp)), (cam["kind"], T.tolist(), got[1][0].tolist(), wp.tolist())
    # the cases are what they claim to be
    X = br.transform(T_neg, br.bearings(mei_wide, ordinary), 100.0)
    assert ((X[:, 2] + 0.5 * np.sqrt((X * X).sum(1))) <= 0).any()
    z0, zn = (br.transform(T_, br.bearings(pin, ordinary), 100.0)[:, 2] for T_ in (T_z0, T_neg))       # (the undistortion of the far-off point diverges: NaN in both)
    assert (z0 == 0).sum() >= 6 and (zn < 0).sum() >= 6 and np.array_equal(np.isnan(z0), np.isnan(zn)) and np.isnan(z0).sum() <= 2


@pytest.mark.gpu
def test_gate_exact(ctx):
    """pred_ok against the oracle's gate on the device's own predictions; points exactly at distance `radius` are kept out by `<`, a NaN prediction is dropped, status = 0
    is dropped, radius <= 0 gives pred_ok == status.  The exact case uses dyadic numbers throughout: a T whose rotation part is zero makes every prediction the one point
    fx * tx + cx, fy * ty + cy (X / Z = tx / 1, exact on any IEEE divide), and (3, 4, 5) k triangles put `other` at exactly radius = 5 k from it"""
    api, fe = ctx
    cam = br.pinhole(256.0, 128.0, 320.0, 240.0)
    T = np.float64([0, 0, 0, 0.25, 0, 0, 0, -0.5, 0, 0, 0, 1.0])
    pu, pv = 256.0 * 0.25 + 320.0, 128.0 * -0.5 + 240.0
    cap = 70
    rng = np.random.RandomState(5)
    pts = (rng.rand(1, cap, 2) * [639, 479]).astype(np.float32)
    pts[0, 3] = (np.nan, 7.0)                                           # -> NaN bearing -> NaN prediction
    k = 2.0
    other = np.zeros((1, cap, 2), np.float32); status = np.ones((1, cap), np.uint8)
    ring = [(3, 4), (-3, 4), (4, -3), (-4, -3), (5, 0), (0, -5), (0, 5), (-5, 0)]
    for i in range(cap):
        dx, dy = ring[i % len(ring)]
        s = (1.0, 0.5, 1.5, 0.96875, 1.03125)[i % 5]                  # on the circle, well inside, well outside, just inside, just outside: all dyadic
        other[0, i] = (pu + dx * k * s, pv + dy * k * s)
    status[0, 10:14] = 0
    n = np.int32([cap - 2])
    radius = 5.0 * k
    got = run_device(api, fe, cam, pts, n, cam_other=cam, T=T, distance=100.0, other=other, status=status, radius=radius)
    pred, ok = got[1][0], got[3][0]
    m = int(n[0])
    fin = np.ones(m, bool); fin[3] = False
    assert np.array_equal(pred[:m][fin], np.broadcast_to(np.float32([pu, pv]), (m, 2))[fin]) and np.isnan(pred[3]).all()
    assert np.array_equal(ok[:m], br.gate(pred[:m], other[0, :m], status[0, :m], radius)) and not ok[m:].any()
    want = np.array([(i % 5) in (1, 3) and not (10 <= i < 14) and i != 3 for i in range(m)], np.uint8)
    assert np.array_equal(ok[:m], want), np.argwhere(ok[:m] != want).ravel().tolist()
    on_circle = [i for i in range(m) if i % 5 == 0]
    assert len(on_circle) >= 8 and not ok[on_circle].any()               # exactly at `radius`: kept out by `<`
    assert ok[3] == 0 and status[0, 3] == 1                             # the NaN prediction is dropped
    for r0 in (0.0, -1.0):                                              # radius <= 0: pred_ok == status, the NaN prediction included
        ok0 = run_device(api, fe, cam, pts, n, cam_other=cam, T=T, distance=100.0, other=other, status=status, radius=r0)[3][0]
        assert np.array_equal(ok0[:m], status[0, :m]) and not ok0[m:].any()
    # a general extrinsic: the oracle's decision on the device's own predictions, radius in the middle of the distances
    pin = CAMS["pin"][0]
    pts = tolerance_points("pin", 1100, 1)
    wp = br.predict(pin, T_A, br.bearings(pin, pts[0]), 100.0)
    other = (wp + rng.uniform(-12, 12, wp.shape)).astype(np.float32)[None]
    status = (rng.rand(1, 1100) < 0.7).astype(np.uint8)
    got = run_device(api, fe, pin, pts, np.int32([1100]), cam_other=pin, T=T_A, distance=100.0, other=other, status=status, radius=9.0)
    want = br.gate(got[1][0], other[0], status[0], 9.0)
    assert np.array_equal(got[3][0], want) and 100 < int(want.sum()) < 700


@pytest.mark.gpu
def test_single_call_refusals(ctx):
    import torch
    api, fe = ctx
    dev = torch.device("cuda")
    cap, nl = 8, 2
    d_pts = torch.zeros(nl * cap * 2, dtype=torch.float32, device=dev); d_n = torch.zeros(nl, dtype=torch.int32, device=dev)
    d_b = torch.zeros(nl * cap * 3, dtype=torch.float64, device=dev); d_p = torch.zeros(nl * cap * 2, dtype=torch.float32, device=dev)
    d_s = torch.zeros(nl * cap, dtype=torch.uint8, device=dev)
    cam = api_camera(api, CAMS["pin"][0])
    ok = dict(cam=cam, pts_stride=2 * cap, n_lists=nl, cap=cap, cam_other=cam, T=T_A, distance=100.0, d_pred_xy=d_p.data_ptr(), d_other_xy=d_p.data_ptr(),
              d_other_status=d_s.data_ptr(), radius=3.0, d_other_bearing=d_b.data_ptr(), d_pred_ok=d_s.data_ptr())

    def call(**kw):
        a = dict(ok); a.update(kw)
        api.bearings_device(fe, a["cam"], d_pts.data_ptr(), a["pts_stride"], d_n.data_ptr(), a["n_lists"], a["cap"], d_b.data_ptr(), cam_other=a["cam_other"], T=a["T"],
                            distance=a["distance"], d_pred_xy=a["d_pred_xy"], d_other_xy=a["d_other_xy"], d_other_status=a["d_other_status"], radius=a["radius"],
                            d_other_bearing=a["d_other_bearing"], d_pred_ok=a["d_pred_ok"])
    bad_kind = api_camera(api, CAMS["pin"][0]); bad_kind.kind = 2
    fx0 = api.camera_pinhole(0.0, 386.0, 322.5, 241.0); fy_nan = api.camera_pinhole(385.0, float("nan"), 322.5, 241.0)
    g0 = api.camera_mei([1.2, 0, 0, 0, 0, 0.0, 2090.0, 645.3, 398.7]); g_inf = api.camera_mei([1.2, 0, 0, 0, 0, 2100.0, float("inf"), 645.3, 398.7])
    T_nan = T_A.copy(); T_nan[7] = np.nan
    for bad in (dict(cap=0), dict(cap=16385), dict(n_lists=0), dict(n_lists=32768), dict(pts_stride=2 * cap - 1), dict(cam=bad_kind), dict(cam=fx0), dict(cam=fy_nan),
                dict(cam=g0), dict(cam=g_inf), dict(cam_other=bad_kind), dict(T=T_nan), dict(distance=float("inf")), dict(d_pred_xy=None), dict(d_pred_ok=None),
                dict(d_other_xy=None)):
        with pytest.raises(api.D2FEError) as e:
            call(**bad)
        assert e.value.code == -1, bad
    call()                                                              # and the handle goes on
    fe.sync()


# ---- the pipe ---------------------------------------------------------------------------------------------------------------------------------------------------------
H, W, CAP = 128, 192, 64
SEED, DISP, STEP, NF = 7105, 12, 3, 12
TOTAL = 40
PCAM_L = br.pinhole(150.0, 151.0, 96.5, 63.0, 0.01, -0.02, 0.001, -0.0005)
PCAM_R = br.pinhole(149.0, 150.5, 95.0, 64.5, -0.015, 0.01, -0.0005, 0.001)
RADIUS_LR = 0.2 * W
# (a): a 30-degree roll moves a prediction by about half its distance from the principal point -- more than RADIUS_LR towards the corners, less near the centre
T_ROLL = br.relative_extrinsic([1, 0, 0, 0], [0, 0, 0], br.quat_axis_angle([0, 0, 1], 30.0), [0.1, 0.0, 0.0]).reshape(-1)
# (b) - (e): the stereo baseline with a 5-degree roll, which spreads |prediction - right track| around the 12-pixel disparity of the frames: the gate keeps some, drops some
T_LK = br.relative_extrinsic([1, 0, 0, 0], [0, 0, 0], br.quat_axis_angle([0, 0, 1], 5.0), [0.1, 0.004, -0.002]).reshape(-1)
SHAPES = {"l1f1": dict(lanes=1, frames=1), "l2f3": dict(lanes=2, frames=3), "l4c2": dict(lanes=4, frames=1, coalesce=2)}
MODES = {
    "a_match_lr": (dict(match_lr=True, radius_lr=RADIUS_LR), T_ROLL),
    "b_lr_lk": (dict(match_lr=False, lr_lk=True), T_LK),
    "c_sp_lk": (dict(match_lr=False, lr_lk=True, sp_lk=True, track_params=dict(total_feature_num=TOTAL)), T_LK),
    "d_flow_lk": (dict(match_lr=False, lr_lk=True, flow_lk=True, flow_params=dict(total_feature_num=150)), T_LK),      # 150 slots against 64 keypoints: detection runs
    "e_mono_depth": (dict(match_lr=False, mono=True, depth=True), T_LK),
}
RADIUS_LK = 11.0


@pytest.fixture(scope="module")
def pctx():
    from d2slam_amd import api, netvlad as nvm
    from d2slam_amd.weights import synthetic_superpoint_weights
    from tests.helpers import depth_ref
    fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=CAP, input_width=W, input_height=H, max_batch=4, precision=api.PREC_F32_WINO, keypoint_threshold=0.005))
    fe.load_superpoint(synthetic_superpoint_weights(dustbin_bias=7.5)); fe.load_netvlad(nvm.synthetic_netvlad_weights())
    yield api, fe, lkref.sliding_stereo(NF, H, W, SEED, DISP, STEP), depth_ref.seeded_depth(NF, H, W, SEED + 1)
    fe.close()


def bearings_kw(api, T):
    return dict(cam_left=api_camera(api, PCAM_L), cam_right=api_camera(api, PCAM_R), T_right_left=T, distance=100.0, lk_use_pred=True, radius_lk=RADIUS_LK)


def run_pipe(pctx, shape, kw, bearings):
    """all NF frames, lanes * coalesce submits in flight -> one dict of copies per submit"""
    api, fe, seq, depths = pctx
    kw = dict(kw); kw.update(SHAPES[shape])
    F = kw["frames"]
    pipe = api.StereoPipe(fe, width=W, height=H, cap=CAP, netvlad=False, bearings=bearings, **kw)
    inflight = pipe.lanes * kw.get("coalesce", 1)
    tk, out = [], []
    take = lambda: out.append({k: (None if v is None else np.array(v)) for k, v in pipe.wait(tk[len(out)]).items()})
    for i in range(NF // F):
        left = np.stack([f[0] for f in seq[i * F:(i + 1) * F]])
        if kw.get("depth"):
            tk.append(pipe.submit(left, depth=depths[i * F:(i + 1) * F]))
        elif kw.get("mono"):
            tk.append(pipe.submit(left))
        else:
            tk.append(pipe.submit(left, np.stack([f[1] for f in seq[i * F:(i + 1) * F]])))
        if len(tk) - len(out) >= inflight:
            take()
    while len(out) < len(tk):
        take()
    pipe.close()
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same_result(a, b, skip, where):
    """every field but `skip`, bit for bit: keypoint and match rows up to their counts (what lies behind a count is not part of the contract), everything else whole"""
    F = a["n_kp"].shape[0] // 2
    for k in b:
        if k in skip:
            continue
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, (where, k)
            continue
        x, y = a[k], b[k]
        assert x.shape == y.shape and x.dtype == y.dtype, (where, k)
        if k in ("kps_xy", "scores", "desc"):
            rows = [(r, int(b["n_kp"][r])) for r in range(2 * F)]
        elif k in ("lk_pts", "lk_status"):
            rows = [(r, int(b["n_kp"][r])) for r in range(F)]
        elif k[:3] in ("lr_", "pre") and not k.endswith("_n"):
            rows = [(r, int(b[k.split("_")[0] + "_n"][r])) for r in range(F)]
        else:
            rows = None
        if rows is None:
            assert np.array_equal(bits(x), bits(y)), (where, k)
        else:
            for r, cnt in rows:
                assert np.array_equal(bits(x[r, :cnt]), bits(y[r, :cnt])), (where, k, r)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("mode", list(MODES))
def test_pipe_equals_the_single_call(pctx, mode, shape):
    api, fe, seq, depths = pctx
    kw, T = MODES[mode]
    base = run_pipe(pctx, shape, kw, None)
    got = run_pipe(pctx, shape, kw, bearings_kw(api, T))
    F = SHAPES[shape]["frames"]
    mono = bool(kw.get("mono"))
    both = bool(kw.get("match_lr"))
    lists = "track" if kw.get("sp_lk") else "flow" if kw.get("flow_lk") else None
    assert len(got) == len(base) == NF // F
    dropped = survived = n_gate = n_ok = 0
    for i, (g, b) in enumerate(zip(got, base)):
        assert all(k.startswith("bearing_") for k in g if k not in b) and all(k in g for k in b)
        same_result(g, b, ("lr_q", "lr_t", "lr_dist", "lr_n") if both else (), (mode, shape, i))
        nk = g["n_kp"]
        # the keypoint rows: left with cam[0] (+ prediction, + the gate of an lr_lk pipe without lists), right with cam[1]
        gate_kp = bool(kw.get("lr_lk")) and lists is None
        dv = run_device(api, fe, PCAM_L, g["kps_xy"][:F], nk[:F], cam_other=PCAM_R if gate_kp else None, T=None if mono else T, distance=100.0,
                        other=g["lk_pts"] if gate_kp else None, status=g["lk_status"] if gate_kp else None, radius=RADIUS_LK)
        assert g["bearing_kp"].shape == (2 * F, CAP, 3) and np.array_equal(bits(g["bearing_kp"][:F]), bits(dv[0])), (mode, shape, i)
        assert int(nk[:F].sum()) > 0 or kw.get("flow_lk") == "only"
        if mono:
            assert g["bearing_kp_pred"] is None
        else:
            assert np.array_equal(bits(g["bearing_kp_pred"]), bits(dv[1])), (mode, shape, i)
        if both:
            dr = run_device(api, fe, PCAM_R, g["kps_xy"][F:], nk[F:])
            assert np.array_equal(bits(g["bearing_kp"][F:]), bits(dr[0])) and int(nk[F:].sum()) > 0
        else:
            assert not bits(g["bearing_kp"][F:]).any()
        if gate_kp:
            assert np.array_equal(bits(g["bearing_lk_right"]), bits(dv[2])) and np.array_equal(g["bearing_lk_pred_ok"], dv[3])
            n_gate += int(sum(g["lk_status"][f, :nk[f]].astype(bool).sum() for f in range(F))); n_ok += int(g["bearing_lk_pred_ok"].sum())
        else:
            assert g["bearing_lk_right"] is None and g["bearing_lk_pred_ok"] is None
        if lists:
            pts, n = g[lists + "_pts"], g[lists + "_n"]
            dl = run_device(api, fe, PCAM_L, pts, n, cam_other=None if mono else PCAM_R, T=None if mono else T, distance=100.0,
                            other=None if mono else g[lists + "_right_pts"], status=None if mono else g[lists + "_right_status"], radius=RADIUS_LK)
            assert np.array_equal(bits(g["bearing_list"]), bits(dl[0])) and np.array_equal(bits(g["bearing_list_pred"]), bits(dl[1]))
            assert np.array_equal(bits(g["bearing_list_right"]), bits(dl[2])) and np.array_equal(g["bearing_list_pred_ok"], dl[3])
            n_gate += int(sum(g[lists + "_right_status"][f, :n[f]].astype(bool).sum() for f in range(F))); n_ok += int(g["bearing_list_pred_ok"].sum())
        else:
            assert all(g[k] is None for k in ("bearing_list", "bearing_list_pred", "bearing_list_right", "bearing_list_pred_ok"))
        if both:
            # the L <-> R radius gate compares the PREDICTED left keypoints: d2fe_match_knn with pts_a = kp_pred_xy
            for f in range(F):
                nl_, nr_ = int(nk[f]), int(nk[F + f])
                q, t, d = fe.match_knn(g["desc"][f, :nl_], g["desc"][F + f, :nr_], 0.8, g["bearing_kp_pred"][f, :nl_], g["kps_xy"][F + f, :nr_], RADIUS_LR)
                m = int(g["lr_n"][f])
                assert m == len(q) and np.array_equal(g["lr_q"][f, :m], q) and np.array_equal(g["lr_t"][f, :m], t) and np.array_equal(bits(g["lr_dist"][f, :m]), bits(d))
                # the CPU oracle on the matches of the un-predicted gate: which of them does the predicted gate drop?
                mb = int(b["lr_n"][f])
                bq, bt = b["lr_q"][f, :mb], b["lr_t"][f, :mb]
                wp = br.predict(PCAM_L, T, br.bearings(PCAM_L, b["kps_xy"][f, :nl_]), 100.0)
                dd = wp[bq] - b["kps_xy"][F + f, :nr_][bt]
                far = np.sqrt(dd[:, 0].astype(np.float64) ** 2 + dd[:, 1].astype(np.float64) ** 2) > RADIUS_LR
                dropped += int(far.sum()); survived += int((~far).sum())
    if both:
        print("%s %s: of the un-predicted gate's matches the predicted gate drops %d and keeps %d" % (mode, shape, dropped, survived))
        assert dropped >= 1 and survived >= 1            # so a pair table whose pts_a was not switched cannot pass the comparison above
    if not mono and not both:
        print("%s %s: the gate keeps %d of %d tracked points" % (mode, shape, n_ok, n_gate))
        assert 0 < n_ok < n_gate                         # both outcomes of the gate occur in the pipe


@pytest.mark.gpu
def test_pipe_refusals(pctx):
    api, fe, seq, depths = pctx
    INVALID, NOT_READY, UNSUPPORTED = -1, -3, -5
    left, right = seq[0][0][None], seq[0][1][None]
    pipe = api.StereoPipe(fe, lanes=2, width=W, height=H, cap=CAP, netvlad=False, match_lr=False, lr_lk=True)

    def refused(code, fn):
        with pytest.raises(api.D2FEError) as e:
            fn()
        assert e.value.code == code, (e.value.code, str(e.value))
    good = bearings_kw(api, T_A)
    bad_kind = api_camera(api, PCAM_L); bad_kind.kind = 7
    T_nan = T_A.copy(); T_nan[3] = np.nan
    refused(INVALID, lambda: pipe.bearings_enable(**dict(good, cam_left=bad_kind)))
    refused(INVALID, lambda: pipe.bearings_enable(**dict(good, cam_right=api.camera_pinhole(0.0, 150.0, 96.0, 64.0))))
    refused(INVALID, lambda: pipe.bearings_enable(**dict(good, T_right_left=T_nan)))
    b = api._PipeBearings()
    pipe._lib.d2fe_pipe_bearings_default(C.byref(b))
    b.cam[0] = good["cam_left"]; b.cam[1] = good["cam_right"]; b.struct_size -= 8
    assert pipe._lib.d2fe_pipe_bearings_enable(pipe._p, C.byref(b)) == INVALID
    pipe.bearings_enable(**good)                                      # none of the refusals changed the pipe
    refused(INVALID, lambda: pipe.bearings_enable(**good))            # twice
    t = pipe.submit(left, right)
    refused(NOT_READY, lambda: pipe.bearings_result_raw(t))           # before wait
    r = pipe.wait(t)
    assert r["bearing_kp"] is not None and r["bearing_lk_pred_ok"] is not None and int(r["n_kp"][0]) > 0
    assert np.isfinite(r["bearing_kp"][0, :int(r["n_kp"][0])]).all()
    refused(INVALID, lambda: pipe.bearings_result_raw(t + 5))
    pipe.close()
    plain = api.StereoPipe(fe, lanes=2, width=W, height=H, cap=CAP, netvlad=False, match_lr=False, lr_lk=True)
    t = plain.submit(left, right)
    refused(INVALID, lambda: plain.bearings_enable(**good))           # after a submit
    r = plain.wait(t)
    refused(UNSUPPORTED, lambda: plain.bearings_result_raw(t))        # a pipe without the mode
    t2 = plain.submit(left, right)                                    # none of these ended the pipe
    assert int(plain.wait(t2)["n_kp"][0]) == int(r["n_kp"][0]) and "bearing_kp" not in plain.wait(t2)
    plain.close()
