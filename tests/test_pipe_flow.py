"""The flow landmarks in the stereo / mono pipe (d2fe_pipe_flow_enable, include/d2fe.h) at the geometry of tests/test_pipe_sp_lk.py: sliding_stereo(12 frames,
480 x 640, seed 7005, disparity 24), seeded weights, the Winograd mode.  Every result is held to the host composition on the pipe's OWN keypoints -- api.LKFrame +
api.lk_track + api.detectFastByRegion + tests/helpers/flow_lk_ref.py -- bit for bit, for every shape of the pipe, and everything else the pipe returns to the same pipe
without the mode."""
import numpy as np
import pytest

from tests.helpers import depth_ref
from tests.helpers import flow_lk_ref as ref
from tests.helpers.lk_carry_ref import sliding_stereo

H, W = 480, 640
SEED, DISP, STEP, NF = 7005, 24, 3, 12
SHAPES = ((1, 1, 1), (2, 1, 1), (2, 3, 1), (4, 1, 2))          # (lanes, frames, coalesce)
FLOW_KEYS = ("flow_n", "flow_n_tracked_in", "flow_n_lost", "flow_n_removed_near", "flow_n_new", "flow_lack", "flow_num", "flow_n_cand", "flow_pts", "flow_id", "flow_src",
             "flow_right_pts", "flow_right_status", "flow_depth_mm")
REST_KEYS = ("kps_xy", "scores", "desc", "n_kp", "netvlad", "prev_q", "prev_t", "prev_dist", "prev_n", "lk_pts", "lk_status", "kp_depth_mm")


@pytest.fixture(scope="module")
def frames():
    return sliding_stereo(NF, H, W, SEED, DISP, STEP)


def _fe(cap):
    from d2slam_amd import api, netvlad as nvm
    from d2slam_amd.weights import synthetic_superpoint_weights
    fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=cap, input_width=W, input_height=H, max_batch=8, precision=api.PREC_F32_WINO))
    fe.load_superpoint(synthetic_superpoint_weights(dustbin_bias=7.5)); fe.load_netvlad(nvm.synthetic_netvlad_weights())
    return api, fe


def _run(api, fe, frames, shape, cap, depths=None, n_frames=NF, **kw):
    """the first n_frames frames through one pipe of this shape; one dict per FRAME with that frame's rows of every key"""
    lanes, F, co = shape
    mono = kw.get("mono", False)
    pipe = api.StereoPipe(fe, lanes=lanes, frames=F, coalesce=co, width=W, height=H, cap=cap, match_lr=False, **kw)
    inflight = lanes * co
    nsub = n_frames // F
    tk, out = [], []
    take = lambda: out.append({k: (None if v is None else v.copy()) for k, v in pipe.wait(tk[len(out)]).items()})
    for i in range(nsub):
        fr = frames[i * F:(i + 1) * F]
        left = np.stack([f[0] for f in fr])
        if depths is not None:
            tk.append(pipe.submit(left, depth=depths[i * F:(i + 1) * F]))
        elif mono:
            tk.append(pipe.submit(left))
        else:
            tk.append(pipe.submit(left, np.stack([f[1] for f in fr])))
        if len(tk) > inflight - 1:
            take()
    while len(out) < nsub:
        take()
    pipe.close()
    res = []
    for o in out:
        for f in range(F):
            res.append({k: (None if v is None else v[f]) for k, v in o.items() if k not in ("lr_q", "lr_t", "lr_dist", "lr_n")})
    return res


def _trackers(api, fe):
    def track(prev_img, cur_img, pts):
        a, b = api.LKFrame(fe, prev_img, 2), api.LKFrame(fe, cur_img, 2)
        out = api.lk_track(fe, a, b, pts, pts, api.WHOLE_IMG_MATCH, 0.0)
        a.close(); b.close()
        return out

    def detect(img, num):
        f = api.LKFrame(fe, img, 0)
        out = api.detectFastByRegion(fe, f, num, 3, 4, 10)
        f.close()
        return out
    return track, detect


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same_frame(r, c, T, where, right):
    n = c["n"]
    for k in ("n", "n_tracked_in", "n_lost", "n_removed_near", "n_new", "lack", "num", "n_cand"):
        assert int(r["flow_" + k]) == c[k], (where, k, int(r["flow_" + k]), c[k])
    assert r["flow_pts"].shape == (T, 2) and r["flow_id"].shape == (T,)
    assert np.array_equal(_bits(r["flow_pts"][:n]), _bits(c["pts"])) and np.array_equal(r["flow_id"][:n], c["id"]) and np.array_equal(r["flow_src"][:n], c["src"]), where
    for k in ("pts", "id", "src"):
        assert not _bits(r["flow_" + k][n:]).any(), (where, k)
    if right:
        assert np.array_equal(r["flow_right_status"][:n], c["right_status"]) and np.array_equal(_bits(r["flow_right_pts"][:n]), _bits(c["right_pts"])), where
        assert not r["flow_right_status"][n:].any() and not _bits(r["flow_right_pts"][n:]).any(), where
    else:
        assert r["flow_right_pts"] is None and r["flow_right_status"] is None


def _same_results(a, b, keys, where):
    for t, (x, y) in enumerate(zip(a, b)):
        for k in keys:
            if k not in x and k not in y:
                continue
            assert (x[k] is None) == (y[k] is None), (where, t, k)
            if x[k] is not None:
                u, v = x[k], y[k]
                if k in ("prev_q", "prev_t", "prev_dist"):      # the matcher's rows are defined up to their count
                    u, v = u[:int(x["prev_n"])], v[:int(x["prev_n"])]
                assert np.array_equal(_bits(u), _bits(v)), (where, t, k)


@pytest.mark.gpu
def test_flow_beside_superpoint_on_the_stereo_pipe(frames):
    """lr_lk pipe, cap = 40 keypoints against total_feature_num = 150, so detection runs (40 + ~73 entries leave the list a quarter short in most frames) and the keypoints block candidates; the right tracks of the
    flow entries; the same bits for every shape; everything else bit-identical to the pipe without the mode"""
    api, fe = _fe(40)
    kw = dict(netvlad=True, match_prev=True, lr_lk=True)
    got = {s: _run(api, fe, frames, s, 40, flow_lk=True, **kw) for s in SHAPES}
    base = got[SHAPES[0]]
    kps = [r["kps_xy"][:int(r["n_kp"])] for r in base]
    comp = ref.compose(frames, kps, *_trackers(api, fe))
    print("beside SuperPoint: n", [c["n"] for c in comp], "num", [c["num"] for c in comp], "new", [c["n_new"] for c in comp], "n_kp", [len(k) for k in kps])
    assert sum(c["num"] > 0 for c in comp[1:]) >= 3 and sum(c["n_new"] > 0 for c in comp[1:]) >= 2 and all(len(k) > 0 for k in kps) and any(c["n_lost"] > 0 for c in comp) and any(c["right_status"].any() for c in comp)
    # the keypoints do block candidates: without them the first frame accepts other points
    assert not np.array_equal(ref.compose(frames[:1], [None], *_trackers(api, fe))[0]["pts"], comp[0]["pts"])
    for t, (r, c) in enumerate(zip(base, comp)):
        _same_frame(r, c, 150, ("beside", t), right=True)
    for s in SHAPES[1:]:
        _same_results(got[s], base, FLOW_KEYS + REST_KEYS, s)
    plain = _run(api, fe, frames, (2, 3, 1), 40, **kw)
    assert not any(k.startswith("flow_") for k in plain[0])
    _same_results(got[(2, 3, 1)], plain, REST_KEYS, "against the pipe without the mode")
    fe.close()


@pytest.mark.gpu
def test_flow_only_on_the_mono_pipe_with_depth(frames):
    """the gopro / visensor_f9p front end: mono, superpoint = 0 -- no network, no matcher, every n_kp row 0 -- with a depth frame beside every gray frame; total_feature_num = 60
    (a pass that does not detect is in test_flow_stage_launch_count)"""
    api, fe = _fe(40)
    depths = depth_ref.seeded_depth(NF, H, W, SEED + 1)
    kw = dict(netvlad=False, match_prev=False, mono=True, depth=True, flow_lk="only", flow_params=dict(total_feature_num=60))
    got = {s: _run(api, fe, frames, s, 40, depths=depths, **kw) for s in SHAPES}
    base = got[SHAPES[0]]
    comp = ref.compose([f[0] for f in frames], [None] * NF, *_trackers(api, fe), params=dict(total_feature_num=60))
    print("flow only: n", [c["n"] for c in comp], "num", [c["num"] for c in comp], "new", [c["n_new"] for c in comp])
    assert comp[0]["num"] == 60 and sum(c["n_new"] > 0 for c in comp[1:]) >= 3 and any(c["n_lost"] > 0 for c in comp)
    for t, (r, c) in enumerate(zip(base, comp)):
        _same_frame(r, c, 60, ("only", t), right=False)
        assert int(r["n_kp"]) == 0 and not _bits(r["kps_xy"]).any() and not _bits(r["desc"]).any() and r["netvlad"] is None
        n = c["n"]
        assert np.array_equal(r["flow_depth_mm"][:n], depth_ref.depth_at_np(depths[t], c["pts"])) and not r["flow_depth_mm"][n:].any(), t
        assert not r["kp_depth_mm"].any()
    for s in SHAPES[1:]:
        _same_results(got[s], base, FLOW_KEYS + REST_KEYS, s)
    fe.close()


@pytest.mark.gpu
def test_flow_stage_launch_count(frames):
    """the launches of the LK stage per pass (d2fe_pipe_profile_read) are the number the header states, whether the pass detects or not: mono 2 pyramid launches + 5 per
    frame; stereo the 3 launches of lr_lk + 5 per frame + ONE left -> right launch over the flow lists"""
    api, fe = _fe(40)
    for mono, F, want in ((True, 1, 2 + 5), (True, 3, 2 + 15), (False, 2, 3 + 10 + 1)):
        kw = dict(mono=True) if mono else dict(lr_lk=True)
        pipe = api.StereoPipe(fe, lanes=1, frames=F, width=W, height=H, cap=40, netvlad=False, match_lr=False, match_prev=False, flow_lk="only",
                              flow_params=dict(total_feature_num=24), **kw)
        nums = []
        for i in range(2):          # the first pass detects, the second (the same frames again: every entry comes back) does not
            left = np.stack([frames[0][0]] * F); right = np.stack([frames[0][1]] * F)
            pipe.profile_enable(2)
            t = pipe.submit(left) if mono else pipe.submit(left, right)
            o = pipe.wait(t)
            nums.append(o["flow_num"].copy())
            assert pipe.profile_read()["lk"][1] == want, (mono, F, i, pipe.profile_read())
            pipe.profile_enable(0)
        assert nums[0][0] == 24 and not nums[1].any(), nums
        pipe.close()
    fe.close()


@pytest.mark.gpu
def test_flow_contract(frames):
    """the refusals, none of which ends the pipe, and D2FE_ERR_UNSUPPORTED without the mode"""
    api, fe = _fe(40)
    l, r = frames[0][0][None], frames[0][1][None]

    def refused(fn, code=-1):
        with pytest.raises(api.D2FEError) as e:
            fn()
        assert e.value.code == code, e.value

    mk = lambda **kw: api.StereoPipe(fe, lanes=2, frames=1, width=W, height=H, cap=40, match_lr=False, **kw)
    # without pyramids
    p = mk(netvlad=False, match_prev=False)
    refused(lambda: p.flow_enable())
    t = p.submit(l, r); p.wait(t)
    with pytest.raises(api.D2FEError) as e:
        p.flow_result_raw(t)
    assert "flow" in str(e.value) and e.value.code not in (0, -1)          # D2FE_ERR_UNSUPPORTED
    unsupported = e.value.code
    p.close()
    # with sp_lk
    p = mk(lr_lk=True, sp_lk=True)
    refused(lambda: p.flow_enable())
    t = p.submit(l, r); assert int(p.wait(t)["track_n"][0]) > 0
    p.close()
    # superpoint = 0 beside netvlad / match_prev; bad parameters
    p = mk(lr_lk=True, netvlad=True, match_prev=False)
    refused(lambda: p.flow_enable(superpoint=0))
    refused(lambda: p.flow_enable(dict(total_feature_num=1024)))
    refused(lambda: p.flow_enable(dict(levels=3)))
    refused(lambda: p.flow_enable(dict(fast_cols=0)))
    p.flow_enable()                                                          # ... and the pipe takes the mode after all of them
    refused(lambda: p.flow_enable())                                         # twice
    t = p.submit(l, r); o = p.wait(t)
    assert int(o["flow_n"][0]) > 0 and int(o["n_kp"][0]) > 0
    p.close()
    p = mk(lr_lk=True, netvlad=False, match_prev=True)
    refused(lambda: p.flow_enable(superpoint=0))
    # after a submit
    t = p.submit(l, r)
    refused(lambda: p.flow_enable())
    assert int(p.wait(t)["n_kp"][0]) > 0
    with pytest.raises(api.D2FEError) as e:
        p.flow_result_raw(t)
    assert e.value.code == unsupported
    p.close()
    # the constructor closes the pipe it could not give the mode to
    refused(lambda: mk(flow_lk=True))
    with pytest.raises(ValueError):
        mk(lr_lk=True, flow_lk="alone")
    fe.close()


@pytest.mark.gpu
def test_flow_through_the_cpp_mirror(tmp_path, sp_weights):
    """include/d2fe.hpp: StereoPipe::flowEnable and StereoFrameResult::flow from g++ (tests/cpp/pipe_flow_test.cpp); 30 keypoints against 60 features"""
    import os
    import struct
    import subprocess
    from d2slam_amd import build as hipbuild
    from d2slam_amd.synth import synth_stereo
    from d2slam_amd.weights import SP_LAYERS
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = hipbuild.build()
    exe = str(tmp_path / "pipe_flow_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "pipe_flow_test.cpp"),
                           "-L", os.path.dirname(lib), "-ld2fe_hip", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib",
                           "-Wl,--allow-shlib-undefined", "-o", exe])
    h, w, maxkp = 240, 320, 30
    l, r = synth_stereo(h, w, seed=5000)
    fin = str(tmp_path / "in.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<iii", h, w, maxkp))
        for n in SP_LAYERS:
            wt, b = sp_weights[n]
            f.write(struct.pack("<iii", wt.shape[0], wt.shape[1], wt.shape[2]))
            f.write(np.ascontiguousarray(wt, "<f4").tobytes()); f.write(np.ascontiguousarray(b, "<f4").tobytes())
        f.write(l.tobytes()); f.write(r.tobytes())
    res = subprocess.run([exe, fin], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.returncode, res.stdout, res.stderr)
    print(res.stdout.strip())
