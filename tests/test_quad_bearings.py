"""The cylindrical camera model in the bearings pass (D2FE_CAM_CYLINDRICAL of d2fe_bearings_device) and the pass in the quad pipe (d2fe_quad_bearings_enable;
d2slam_amd/csrc/bearings.hip, quad_pipe.hip) against the float64 oracle tests/helpers/cyl_bearings_ref.py, which tests/test_quad_bearings_cpu.py pins to the reference's
own lift and to the restatements of include/d2fe.hpp.

The device's tan, atan2, sqrt and divide need not return the host's last bits, so nothing here compares their results bit for bit with the host: bearings are held to
cyl_bearings_ref.cyl_bearing_bound (derived from the functions' stated accuracy, not measured), predictions to one fp32 unit in the last place away from atan2's jump, the
gate to the oracle's decision ON THE DEVICE'S OWN predictions, and the pipe to the single call on the ticket's own points (device against device: the same bits)."""
import ctypes as C

import numpy as np
import pytest

from tests.helpers import bearings_ref as br
from tests.helpers import cyl_bearings_ref as cr
from tests.helpers import quad_lk_ref as qref


def api_camera(api, cam):
    if cam["kind"] == "cylindrical":
        return api.camera_cylindrical(cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    if cam["kind"] == "pinhole":
        return api.camera_pinhole(*[cam[k] for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2")])
    return api.camera_mei(br.mei9(cam))


@pytest.fixture(scope="module")
def ctx():
    from d2slam_amd import api
    fe = api.FrontEnd(api.SuperPointConfig(input_width=64, input_height=64, max_batch=1))
    yield api, fe
    fe.close()


def run_device(api, fe, cam, pts, n, pad=0, cam_other=None, T=None, distance=100.0, other=None, status=None, radius=0.0):
    """d2fe_bearings_device on [nl, cap, 2] points (cam / cam_other: oracle dicts or d2fe_camera structs); the outputs are pre-filled with 0xFF bytes, so every slot >= n
    must have been WRITTEN as zero.  Returns (bearing, pred_xy | None, other_bearing | None, pred_ok | None)"""
    import torch
    dev = torch.device("cuda")
    as_cam = lambda c: api_camera(api, c) if isinstance(c, dict) else c
    nl, cap = pts.shape[:2]
    stride = 2 * cap + pad
    hp = np.full((nl, stride), 7.25, np.float32); hp[:, :2 * cap] = pts.reshape(nl, -1)
    d_pts = torch.from_numpy(hp).to(dev); d_n = torch.from_numpy(np.ascontiguousarray(n, np.int32)).to(dev)
    fill = lambda nbytes: torch.full((nbytes,), -1, dtype=torch.int8, device=dev)
    d_b = fill(nl * cap * 24)
    want_pred = T is not None
    d_p = fill(nl * cap * 8) if want_pred else None
    gate = other is not None
    if gate:
        d_o = torch.from_numpy(np.ascontiguousarray(other, np.float32)).to(dev); d_s = torch.from_numpy(np.ascontiguousarray(status, np.uint8)).to(dev)
        d_ob = fill(nl * cap * 24); d_ok = fill(nl * cap)
    torch.cuda.synchronize()
    api.bearings_device(fe, as_cam(cam), d_pts.data_ptr(), stride, d_n.data_ptr(), nl, cap, d_b.data_ptr(), cam_other=None if cam_other is None else as_cam(cam_other),
                        T=T, distance=distance, d_pred_xy=d_p.data_ptr() if want_pred else None, d_other_xy=d_o.data_ptr() if gate else None,
                        d_other_status=d_s.data_ptr() if gate else None, radius=radius, d_other_bearing=d_ob.data_ptr() if gate else None,
                        d_pred_ok=d_ok.data_ptr() if gate else None)
    fe.sync()
    out = [d_b.cpu().numpy().view(np.float64).reshape(nl, cap, 3), d_p.cpu().numpy().view(np.float32).reshape(nl, cap, 2) if want_pred else None]
    out += [d_ob.cpu().numpy().view(np.float64).reshape(nl, cap, 3), d_ok.cpu().numpy().view(np.uint8).reshape(nl, cap)] if gate else [None, None]
    return out


def zero_beyond(a, n):
    return all(not a[l, n[l]:].view(np.uint8).any() for l in range(len(n)))


# ---- the single call ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(cr.CAMS))
def test_single_call_against_the_oracle(ctx, name):
    api, fe = ctx
    cam = cr.CAMS[name]
    oth = cr.CAMS["skew" if name == "view" else "view"]
    equal = {"bearing": [0, 0], "pred": [0, 0]}
    worst = 0.0
    for cap in cr.CAPS:
        nl = cr.N_LISTS
        pts = cr.tolerance_points(name, cap)
        n = cr.counts(cap); nc = np.clip(n.astype(np.int64), 0, cap)
        flat = pts.reshape(-1, 2)
        wb = cr.bearings(cam, flat).reshape(nl, cap, 3)
        bound = cr.cyl_bearing_bound(cam, flat).reshape(nl, cap, 3)
        rng = np.random.RandomState(cap + nl)

        def check_bearing(got, want, bnd, what):
            nonlocal worst
            assert zero_beyond(got, nc), (what, cap)
            for l in range(nl):
                g, w_ = got[l, :nc[l]], want[l, :nc[l]]
                if not g.size:
                    continue
                err = np.abs(g - w_)
                with np.errstate(all="ignore"):
                    rel = float(np.nanmax(np.where(w_ != 0, err / (cr.U * np.abs(w_)), np.where(err == 0, 0.0, np.inf))))
                worst = max(worst, rel)
                assert np.isfinite(g).all() and (err <= bnd[l, :nc[l]]).all(), (what, cap, l, rel)
                equal["bearing"][0] += int((g == w_).sum()); equal["bearing"][1] += g.size
        got = run_device(api, fe, cam, pts, n, pad=6)                  # bearings alone, lists further apart than 2 * cap floats
        check_bearing(got[0], wb, bound, "alone")
        for dist, T in cr.SETTINGS:
            X = br.transform(T, wb.reshape(-1, 3), dist)
            keep = ~cr.near_back_seam(X).reshape(nl, cap)
            wp = cr.predict(cam, T, wb.reshape(-1, 3), dist).reshape(nl, cap, 2)
            other = (wp + rng.uniform(-30, 30, wp.shape)).astype(np.float32)
            status = (rng.rand(nl, cap) < 0.8).astype(np.uint8)
            wob = cr.bearings(oth, other.reshape(-1, 2)).reshape(nl, cap, 3)
            ob_bound = cr.cyl_bearing_bound(oth, other.reshape(-1, 2)).reshape(nl, cap, 3)
            for gate in (False, True):
                got = run_device(api, fe, cam, pts, n, pad=2, cam_other=oth if gate else None, T=T, distance=dist, other=other if gate else None,
                                 status=status if gate else None, radius=25.0)
                check_bearing(got[0], wb, bound, "with prediction")
                assert zero_beyond(got[1], nc)
                for l in range(nl):
                    k = keep[l, :nc[l]]
                    g, w_ = got[1][l, :nc[l]][k], wp[l, :nc[l]][k]
                    assert br.within_fp32_ulp(g, w_).all(), (cap, l, dist)
                    assert np.isfinite(got[1][l, :nc[l]]).all()          # at the back seam too: one of the two sides of the jump
                    equal["pred"][0] += int((g == w_).sum()); equal["pred"][1] += g.size
                if gate:
                    assert zero_beyond(got[2], nc) and zero_beyond(got[3], nc)
                    for l in range(nl):
                        k = nc[l]
                        assert np.isfinite(wob[l, :k]).all() and (np.abs(got[2][l, :k] - wob[l, :k]) <= ob_bound[l, :k]).all()
                        # the gate, exact: the oracle's decision on the device's own predictions
                        assert np.array_equal(got[3][l, :k], br.gate(got[1][l, :k], other[l, :k], status[l, :k], 25.0))
    for k, (a, b) in equal.items():
        print("%s: %s bit-equal share %.6f (%d of %d)" % (name, k, a / max(b, 1), a, b))
    print("%s: largest bearing difference %.2f units of 2^-52 of the component" % (name, worst))


@pytest.mark.gpu
def test_classes_of_special_points(ctx):
    """NaN, +-inf and huge coordinates (tan's large-argument reduction), a point transformed onto the cylinder's axis (rho = 0), points transformed exactly onto and next
    to the back seam: NaN / +inf / -inf / finite of every output equal the oracle's"""
    api, fe = ctx
    cam = cr.CAMS["view"]
    nan, inf = np.nan, np.inf
    special = np.float32([[nan, 10], [10, nan], [nan, nan], [inf, 10], [10, -inf], [-inf, inf], [1e9, 10], [10, -1e9], [-1e9, 1e9], [3e38, 10], [-3e38, 3e38], [400, 200],
                          [40, 200], [760, 0], [0, 0]])
    ordinary = np.float32([[400, 200], [40, 200], [760, 200], [41, 7], [759, 390], [5, 370], [799, 399], [0, 0], [400, 0]])
    T_axis = np.float64([0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0])              # X = Z = 0: on the axis
    T_origin = np.zeros(12)                                                # X = Y = Z = 0
    T_back = np.float64([0, 0, 0, 0, 0, 1, 0, 0, 0, 0, -1, 0])             # X = 0 exactly, Z < 0 in front of the seam columns: atan2(0, negative)
    T_flip = np.float64([-1, 0, 0, 0, 0, 1, 0, 0, 0, 0, -1, 0])            # a half turn: the view's centre lands on the back seam

    def cls(a):
        a = np.asarray(a, np.float64)
        return np.stack([np.isnan(a), np.isposinf(a), np.isneginf(a)])
    for pts, T, dist in ((special, cr.T_SMALL, 100.0), (special, cr.T_YAW, 1.5), (ordinary, T_axis, 100.0), (ordinary, T_origin, 1.5), (ordinary, T_back, 100.0),
                         (ordinary, T_flip, 100.0), (ordinary, cr.T_YAW, 100.0)):
        got = run_device(api, fe, cam, pts[None], np.int32([len(pts)]), T=T, distance=dist)
        wb = cr.bearings(cam, pts)
        wp = cr.predict(cam, T, wb, dist)
        assert np.array_equal(cls(got[0][0]), cls(wb)), T.tolist()
        assert np.array_equal(cls(got[1][0]), cls(wp)), (T.tolist(), got[1][0].tolist(), wp.tolist())
    # the cases are what they claim to be
    wb = cr.bearings(cam, ordinary)
    u, v = cr.space_to_plane(cam, br.transform(T_axis, wb, 100.0))
    assert np.isnan(u).all() and (np.isinf(v) | np.isnan(v)).all() and np.isinf(v).any()
    assert cr.near_back_seam(br.transform(T_flip, wb, 100.0))[0] and cr.near_back_seam(br.transform(cr.T_YAW, wb, 100.0))[2]
    assert np.isnan(cr.bearings(cam, special)[:6]).any(1).all() and np.isfinite(cr.bearings(cam, special)[6:]).all()


@pytest.mark.gpu
def test_gate_exact(ctx):
    """pred_ok against the oracle's gate on the device's own predictions; points exactly at distance `radius` are kept out by `<`, a NaN prediction is dropped, status = 0
    is dropped, radius <= 0 gives pred_ok == status.  The exact case uses dyadic numbers throughout: a T whose rotation part is zero sends every point to (0, 0.5, 1),
    where rho = 1 and atan2(0, 1) = 0 on any implementation, so every prediction is (cx, fy / 2 + cy); (3, 4, 5) k triangles put `other` at exactly radius = 5 k from it"""
    api, fe = ctx
    cam = cr.cylindrical(256.0, 128.0, 320.0, 240.0)
    T = np.float64([0, 0, 0, 0, 0, 0, 0, 0.5, 0, 0, 0, 1.0])
    pu, pv = 320.0, 128.0 * 0.5 + 240.0
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
    # the quad rig's extrinsic: the oracle's decision on the device's own predictions, radius in the middle of the distances
    view = cr.CAMS["view"]
    pts = cr.tolerance_points("view", 1100, 1)
    wp = cr.predict(view, cr.T_YAW, cr.bearings(view, pts[0]), 100.0)
    other = (wp + rng.uniform(-12, 12, wp.shape)).astype(np.float32)[None]
    status = (rng.rand(1, 1100) < 0.7).astype(np.uint8)
    got = run_device(api, fe, view, pts, np.int32([1100]), cam_other=view, T=cr.T_YAW, distance=100.0, other=other, status=status, radius=9.0)
    want = br.gate(got[1][0], other[0], status[0], 9.0)
    assert np.array_equal(got[3][0], want) and 100 < int(want.sum()) < 700


@pytest.mark.gpu
def test_single_call_refusals(ctx):
    import torch
    api, fe = ctx
    dev = torch.device("cuda")
    cap, nl = 8, 2
    d_pts = torch.zeros(nl * cap * 2, dtype=torch.float32, device=dev); d_n = torch.zeros(nl, dtype=torch.int32, device=dev)
    d_b = torch.zeros(nl * cap * 3, dtype=torch.float64, device=dev)
    good = api.cylinder_camera(800, 400, 200.0)

    def call(cam):
        api.bearings_device(fe, cam, d_pts.data_ptr(), 2 * cap, d_n.data_ptr(), nl, cap, d_b.data_ptr())
    p4 = api.camera_cylindrical(229.0, 229.0, 400.0, 200.0); p4.p[4] = 1e-3
    p8 = api.camera_cylindrical(229.0, 229.0, 400.0, 200.0); p8.p[8] = float("nan")
    kind2 = api.cylinder_camera(800, 400, 200.0); kind2.kind = 2
    for bad in (api.camera_cylindrical(0.0, 229.0, 400.0, 200.0), api.camera_cylindrical(229.0, float("nan"), 400.0, 200.0),
                api.camera_cylindrical(float("inf"), 229.0, 400.0, 200.0), p4, p8, kind2):
        with pytest.raises(api.D2FEError) as e:
            call(bad)
        assert e.value.code == -1
    call(good)                                                          # and the handle goes on
    fe.sync()
    assert not d_b.cpu().numpy().any()                                  # two empty lists: zeros


# ---- the pipe -----------------------------------------------------------------------------------------------------------------------------------------------------------
H, W, CAP, NQ, SEED, FOV = qref.H, qref.W, 60, 8, 7106, qref.FOV
# four DIFFERENT cameras, so that a list lifted with a neighbour's camera cannot pass: view 0 has the virtual camera of the 200 x 120 / 200 degree view (seam near columns
# 10 and 190), the others are a few percent off it.  A prediction is lifted AND projected with camera a, so under the 90-degree yaw it lands at x + fx_a pi / 2 whatever
# cx_a is, while the scene's neighbour views are shifted by exactly 90 columns: the prediction misses the neighbour track by fx_a pi / 2 - 90 columns -- 0 for view 0
# (pairs 0 and 3), 1.11 for view 1 (pair 1), -2.82 for view 2 (pair 2) -- plus the tracker's own sub-pixel error.  That is what spreads the gate
PIPE_CAMS = [cr.cylinder_camera(W, H, FOV), cr.cylindrical(58.0, 57.0, 100.5, 59.5), cr.cylindrical(55.5, 58.2, 99.25, 60.75), cr.cylindrical(57.8, 57.8, 101.0, 60.0)]
# pair n = (a, b): camera b is yawed by +90 degrees against a for (0,1) (1,2) (2,3) and by -90 degrees for (0,3), 0.05 m apart
T_NB = np.stack([br.relative_extrinsic([1, 0, 0, 0], [0, 0, 0], br.quat_axis_angle([0, 1, 0], -90.0 if n < 3 else 90.0), [0.05, 0.0, 0.0]).reshape(-1) for n in range(4)])
RADIUS_LK = 1.2              # between the misses above: pairs 0 and 3 are kept, pair 2 is dropped, pair 1 is decided track by track
SHAPES = {"l1q1": (1, 1), "l2q2": (2, 2), "l4q1": (4, 1)}
MODES = {"sp_lk": ("track", dict(sp_lk=True, track_params={"total_feature_num": 40, "feature_min_dist": 3.0})),
         "flow_lk": ("flow", dict(flow_lk=True, flow_params={"total_feature_num": 100, "feature_min_dist": 20.0})),
         "plain": (None, dict(match_neighbour=True, match_prev=True))}


@pytest.fixture(scope="module")
def pctx():
    from tests.test_quad_pipe_flow import _fe
    api, fe = _fe()
    yield api, fe, qref.cyclic_quads(NQ, SEED)
    fe.close()


def bearings_kw(api, **kw):
    out = dict(cams=[api_camera(api, c) for c in PIPE_CAMS], T_nb=T_NB, distance=100.0, lk_use_pred=True, radius_lk=RADIUS_LK)
    out.update(kw)
    return out


def make_pipe(api, fe, lanes=1, Q=1, **kw):
    args = dict(lanes=lanes, quads=Q, raw_width=W, raw_height=H, width=W, height=H, cap=CAP, radius_neighbour=0.2 * W, undistort_fov=FOV, netvlad=False,
                match_neighbour=False, match_prev=False)
    args.update(kw)
    return api.QuadPipe(fe, qref.identity_maps(), **args)


def drain(pipe, frames, lanes, Q):
    """all quad frames through the pipe, Q per submit, `lanes` submits in flight; one dict of copies per SUBMIT"""
    nsub = len(frames) // Q
    tk, out = [], []
    take = lambda: out.append({k: (None if v is None else np.array(v)) for k, v in pipe.wait(tk[len(out)]).items()})
    for i in range(nsub):
        tk.append(pipe.submit(frames[i * Q:(i + 1) * Q]))
        if len(tk) > lanes - 1:
            take()
    while len(out) < nsub:
        take()
    pipe.close()
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same_result(a, b, where):
    """every field of b, bit for bit: keypoint and match rows up to their counts (what lies behind a count is not part of the contract), everything else whole"""
    for k in b:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, (where, k)
            continue
        x, y = a[k], b[k]
        assert x.shape == y.shape and x.dtype == y.dtype, (where, k)
        cnt = b["n_kp"] if k in ("kps_xy", "scores", "desc") else b[k.split("_")[0] + "_n"] if k[:3] in ("nb_", "pre") and not k.endswith("_n") else None
        if cnt is None:
            assert np.array_equal(bits(x), bits(y)), (where, k)
        else:
            for q in range(cnt.shape[0]):
                for c in range(4):
                    assert np.array_equal(bits(x[q, c, :cnt[q, c]]), bits(y[q, c, :cnt[q, c]])), (where, k, q, c)


def check_against_single_calls(api, fe, g, lists, where, bear=None):
    """one submit's bear_* arrays against d2fe_bearings_device on the submit's own points, camera by camera and pair by pair, bit for bit.  Returns (tracked, kept)"""
    kw = bearings_kw(api, **(bear or {}))
    radius = kw["radius_lk"] if kw["lk_use_pred"] else 0.0
    Q = g["n_kp"].shape[0]
    assert g["bear_kp"].shape == (Q, 4, CAP, 3)
    for c in range(4):
        dv = run_device(api, fe, PIPE_CAMS[c], g["kps_xy"][:, c], g["n_kp"][:, c])
        assert np.array_equal(bits(g["bear_kp"][:, c]), bits(dv[0])), (where, "kp", c)
        for q in range(Q):
            assert np.isfinite(g["bear_kp"][q, c, :g["n_kp"][q, c]]).all()
    if lists is None:
        assert all(g[k] is None for k in ("bear_list", "bear_nb_pred", "bear_nb", "bear_nb_pred_ok"))
        return 0, 0
    pts, n = g[lists + "_pts"], g[lists + "_n"]
    T = pts.shape[2]
    assert g["bear_list"].shape == (Q, 4, T, 3) and g["bear_nb_pred"].shape == (Q, 4, T, 2) and g["bear_nb_pred_ok"].shape == (Q, 4, T)
    for c in range(4):
        dv = run_device(api, fe, PIPE_CAMS[c], np.ascontiguousarray(pts[:, c]), n[:, c])
        assert np.array_equal(bits(g["bear_list"][:, c]), bits(dv[0])), (where, "list", c)
    tracked = kept = 0
    for i, (a, b, _) in enumerate(qref.NEIGHBOURS):
        st = g[lists + "_nb_lk_status"][:, i]
        dv = run_device(api, fe, PIPE_CAMS[a], np.ascontiguousarray(pts[:, a]), n[:, a], cam_other=PIPE_CAMS[b], T=T_NB[i], distance=kw["distance"],
                        other=g[lists + "_nb_lk_xy"][:, i], status=st, radius=radius)
        assert np.array_equal(bits(g["bear_nb_pred"][:, i]), bits(dv[1])), (where, "pred", i)
        assert np.array_equal(bits(g["bear_nb"][:, i]), bits(dv[2])), (where, "nb", i)
        assert np.array_equal(g["bear_nb_pred_ok"][:, i], dv[3]), (where, "ok", i)
        for q in range(Q):
            m = int(n[q, a])
            tracked += int(st[q, :m].astype(bool).sum()); kept += int(g["bear_nb_pred_ok"][q, i, :m].sum())
            assert not (g["bear_nb_pred_ok"][q, i, :m].astype(bool) & ~st[q, :m].astype(bool)).any()
    return tracked, kept


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("mode", list(MODES))
def test_pipe_equals_the_single_call(pctx, mode, shape):
    api, fe, quads = pctx
    lanes, Q = SHAPES[shape]
    lists, kw = MODES[mode]
    base = drain(make_pipe(api, fe, lanes, Q, **kw), quads, lanes, Q)
    got = drain(make_pipe(api, fe, lanes, Q, bearings=bearings_kw(api), **kw), quads, lanes, Q)
    assert len(got) == len(base) == NQ // Q
    tracked = kept = 0
    for i, (g, b) in enumerate(zip(got, base)):
        assert all(k.startswith("bear_") for k in g if k not in b) and all(k in g for k in b) and "bear_kp" in g
        same_result(g, b, (mode, shape, i))
        t, k = check_against_single_calls(api, fe, g, lists, (mode, shape, i))
        tracked += t; kept += k
    assert sum(int(g["n_kp"].sum()) for g in got) > 100
    if lists:
        print("%s %s: the gate keeps %d of %d neighbour tracks" % (mode, shape, kept, tracked))
        assert 0 < kept < tracked                          # both outcomes of the gate occur in the pipe


@pytest.mark.gpu
def test_enable_order_and_lk_use_pred(pctx):
    """d2fe_quad_bearings_enable BEFORE d2fe_quad_flow_enable / d2fe_quad_track_enable lays the block out as the other order does: the same results, every key, bit for
    bit.  lk_use_pred = 0 and radius_lk <= 0: nb_pred_ok is nb_lk_status"""
    api, fe, quads = pctx
    for mode in ("flow_lk", "sp_lk"):
        lists, kw = MODES[mode]
        want = drain(make_pipe(api, fe, 2, 2, bearings=bearings_kw(api), **kw), quads, 2, 2)
        pipe = make_pipe(api, fe, 2, 2)
        pipe.bearings_enable(**bearings_kw(api))
        if mode == "flow_lk":
            pipe.flow_enable(kw["flow_params"])
        else:
            pipe.track_enable(kw["track_params"])
        got = drain(pipe, quads, 2, 2)
        for i, (g, w_) in enumerate(zip(got, want)):
            assert set(g) == set(w_)
            same_result(g, {k: v for k, v in w_.items() if not k.startswith("bear_")}, (mode, i))
            for k in ("bear_kp", "bear_list", "bear_nb_pred", "bear_nb", "bear_nb_pred_ok"):
                assert np.array_equal(bits(g[k]), bits(w_[k])), (mode, i, k)
    lists, kw = MODES["flow_lk"]
    for bear in (dict(lk_use_pred=False), dict(radius_lk=0.0), dict(radius_lk=-1.0)):
        got = drain(make_pipe(api, fe, 1, 1, bearings=bearings_kw(api, **bear), **kw), quads[:3], 1, 1)
        tracked = 0
        for i, g in enumerate(got):
            t, k = check_against_single_calls(api, fe, g, lists, (bear, i), bear)
            assert t == k
            tracked += t
            n = g["flow_n"]
            for q in range(1):
                for j, (a, b, _) in enumerate(qref.NEIGHBOURS):
                    m = int(n[q, a])
                    assert np.array_equal(g["bear_nb_pred_ok"][q, j, :m] != 0, g["flow_nb_lk_status"][q, j, :m] != 0) and not g["bear_nb_pred_ok"][q, j, m:].any()
        assert tracked > 0


@pytest.mark.gpu
def test_pipe_refusals(pctx):
    api, fe, quads = pctx
    INVALID, NOT_READY, UNSUPPORTED = -1, -3, -5
    lists, kw = MODES["flow_lk"]
    pipe = make_pipe(api, fe, 2, 1, **kw)

    def refused(code, fn):
        with pytest.raises(api.D2FEError) as e:
            fn()
        assert e.value.code == code, (e.value.code, str(e.value))
    good = bearings_kw(api)
    bad_kind = api_camera(api, PIPE_CAMS[1]); bad_kind.kind = 2
    p4 = api_camera(api, PIPE_CAMS[2]); p4.p[4] = 1e-3
    T_nan = T_NB.copy(); T_nan[3, 7] = np.nan
    refused(INVALID, lambda: pipe.bearings_enable(**dict(good, cams=[good["cams"][0], bad_kind] + good["cams"][2:])))
    refused(INVALID, lambda: pipe.bearings_enable(**dict(good, cams=good["cams"][:2] + [p4, good["cams"][3]])))
    refused(INVALID, lambda: pipe.bearings_enable(**dict(good, cams=good["cams"][:3] + [api.camera_cylindrical(0.0, 57.0, 100.0, 60.0)])))
    refused(INVALID, lambda: pipe.bearings_enable(**dict(good, T_nb=T_nan)))
    refused(INVALID, lambda: pipe.bearings_enable(**dict(good, distance=float("inf"))))
    refused(INVALID, lambda: pipe.bearings_enable(**dict(good, radius_lk=float("nan"))))
    b = api._QuadBearings()
    pipe._lib.d2fe_quad_bearings_default(C.byref(b))
    for c in range(4):
        b.cam[c] = good["cams"][c]
    b.struct_size -= 8
    assert pipe._lib.d2fe_quad_bearings_enable(pipe._p, C.byref(b)) == INVALID
    pipe.bearings_enable(**good)                                      # none of the refusals changed the pipe
    refused(INVALID, lambda: pipe.bearings_enable(**good))            # twice
    t = pipe.submit(quads[:1])
    refused(NOT_READY, lambda: pipe.bearings_result_raw(t))           # before wait
    r = pipe.wait(t)
    assert r["bear_kp"] is not None and r["bear_nb_pred_ok"] is not None and int(r["n_kp"].sum()) > 0
    check_against_single_calls(api, fe, {k: (None if v is None else np.array(v)) for k, v in r.items()}, lists, "after the refusals")
    refused(INVALID, lambda: pipe.bearings_result_raw(t + 5))
    pipe.close()
    plain = make_pipe(api, fe, 2, 1, **kw)
    t = plain.submit(quads[:1])
    refused(INVALID, lambda: plain.bearings_enable(**good))           # after a submit
    r = {k: (None if v is None else np.array(v)) for k, v in plain.wait(t).items()}
    refused(UNSUPPORTED, lambda: plain.bearings_result_raw(t))        # a pipe without the mode
    t2 = plain.submit(quads[1:2])                                     # none of these ended the pipe
    r2 = plain.wait(t2)
    assert "bear_kp" not in r2 and int(r2["n_kp"].sum()) > 0 and int(r["n_kp"].sum()) > 0
    plain.close()
