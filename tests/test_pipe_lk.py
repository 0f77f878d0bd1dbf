"""The stereo pipe's lr_lk mode (d2fe_pipe_config.lr_lk, include/d2fe.h): the reference's default stereo path -- lr_match_use_lk = true,
D2FeatureTracker::trackLocalFrames (d2featuretracker.cpp:110-116) -> trackLK -> opticalflowTrackPyr -- SuperPoint on the left image only, every left
keypoint tracked left -> right with pyramidal LK inside the pass.  All on the frames of synth_stereo(480, 640, seed), seeds 5000..5031, seeded weights,
200 keypoints, in the Winograd mode and in the exact mode."""
import numpy as np
import pytest

from d2slam_amd.synth import synth_stereo

H, W, CAP = 480, 640, 200
SEEDS = list(range(5000, 5032))
LEFT_KEYS = ("kps_xy", "scores", "desc")


@pytest.fixture(scope="module")
def frames():
    return [synth_stereo(H, W, s) for s in SEEDS]


def _disparity(seed):
    return int(np.random.RandomState(seed + 100003).randint(8, 41))


def _fe(prec, max_batch=8, threshold=None):
    from d2slam_amd import api, netvlad as nvm
    from d2slam_amd.weights import synthetic_superpoint_weights
    kw = {} if threshold is None else {"keypoint_threshold": threshold}
    fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=CAP, input_width=W, input_height=H, max_batch=max_batch,
                                           precision={"wino": api.PREC_F32_WINO, "f32": api.PREC_F32}[prec], **kw))
    fe.load_superpoint(synthetic_superpoint_weights(dustbin_bias=7.5)); fe.load_netvlad(nvm.synthetic_netvlad_weights())
    return api, fe


def _run(api, fe, frames, F, nsub, first=0, **kw):
    """nsub submits of F consecutive frames starting at frame `first`, lanes * coalesce submits in flight (coalesce fills its passes); copies of the results"""
    pipe = api.StereoPipe(fe, frames=F, width=W, height=H, cap=CAP, netvlad=True, match_prev=True, **kw)
    inflight = pipe.lanes * kw.get("coalesce", 1)
    tk, out = [], []
    take = lambda: out.append({k: (None if v is None else v.copy()) for k, v in pipe.wait(tk[len(out)]).items()})
    for i in range(nsub):
        fr = frames[first + i * F:first + (i + 1) * F]
        tk.append(pipe.submit(np.stack([f[0] for f in fr]), np.stack([f[1] for f in fr])))
        if len(tk) > inflight - 1:
            take()
    while len(out) < nsub:
        take()
    pipe.close()
    return out


def _same_left(a, b, F):
    """left rows, NetVLAD and the temporal matches of an lr_lk result `b` against the plain pipe's `a`; right rows of b are empty"""
    for f in range(F):
        n = int(a["n_kp"][f])
        assert n == int(b["n_kp"][f]) and n > 0
        for k in LEFT_KEYS:
            assert np.array_equal(a[k][f, :n], b[k][f, :n]), k
        assert int(b["n_kp"][F + f]) == 0
        m = int(a["prev_n"][f])
        assert m == int(b["prev_n"][f])
        for k in ("prev_q", "prev_t", "prev_dist"):
            assert np.array_equal(a[k][f, :m], b[k][f, :m]), k
    assert np.array_equal(a["netvlad"], b["netvlad"])
    assert all(b[k] is None for k in ("lr_q", "lr_t", "lr_dist", "lr_n")) and all(a[k] is None for k in ("lr_q", "lr_n"))
    assert "lk_pts" not in a and "lk_status" not in a


def _check_tracks(api, fe, o, fr, seeds):
    """items 2 and 4 for one result: the existing LK calls on the same keypoints give the same bits; the tracks sit at the seed's disparity"""
    F = len(fr)
    assert o["lk_pts"].shape == (F, CAP, 2) and o["lk_status"].shape == (F, CAP) and o["lk_status"].dtype == np.uint8
    for f in range(F):
        n = int(o["n_kp"][f])
        kps = o["kps_xy"][f, :n]
        fl, frr = api.LKFrame(fe, fr[f][0], 2), api.LKFrame(fe, fr[f][1], 2)
        ref, rst = api.lk_track(fe, fl, frr, kps, kps, api.WHOLE_IMG_MATCH, 0.0)
        fl.close(); frr.close()
        assert np.array_equal(o["lk_status"][f, :n], rst)
        assert np.array_equal(np.ascontiguousarray(o["lk_pts"][f, :n]).view(np.uint32), ref.view(np.uint32))
        assert not o["lk_status"][f, n:].any() and not o["lk_pts"][f, n:].view(np.uint32).any()
        # it tracks: the right image is the left one shifted by the seed's disparity
        d = _disparity(seeds[f])
        ok = o["lk_status"][f, :n] == 1
        dist = np.linalg.norm(o["lk_pts"][f, :n][ok].astype(np.float64) - (kps[ok].astype(np.float64) + np.array([d, 0.0])), axis=1)
        print("seed %d: %d keypoints, %d tracked, largest distance to (x + %d, y) %.3f px" % (seeds[f], n, int(ok.sum()), d, float(dist.max()) if len(dist) else -1.0))
        assert int(ok.sum()) >= 150
        assert dist.max() <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["wino", "f32"])
def test_lr_lk_pipe_left_results_tracks_and_oracle(prec, frames, orc):
    """Items 1-4: (1) left rows, NetVLAD, prev_* of the lr_lk pipe equal the pipe with lr_lk = 0, match_lr = 0; (2) its tracks are the bits of LKFrame + lk_track on the
    same keypoints; (3) and of the oracle; (4) at least 150 of the 200 keypoints of EVERY frame are tracked, each within 1 px of (x + disparity, y).  The oracle alone
    (CPU) tracks at least 163 of 200 in every one of the 32 frames with a largest distance of 0.60 px, so both floors have room."""
    api, fe = _fe(prec)
    # frames = 4, lanes = 2: 8 submits = all 32 frames (the first 4 submits are the case of 16 frames)
    a = _run(api, fe, frames, 4, 8, lanes=2, match_lr=False)
    b = _run(api, fe, frames, 4, 8, lanes=2, match_lr=False, lr_lk=True)
    for s in range(8):
        _same_left(a[s], b[s], 4)
        _check_tracks(api, fe, b[s], frames[4 * s:4 * s + 4], SEEDS[4 * s:4 * s + 4])
    # (3) the oracle, one submit
    o = b[1]
    for f in range(4):
        l, r = frames[4 + f]
        n = int(o["n_kp"][f])
        ref, rst = orc.lk_track(orc.pyr_build(l, 2), orc.pyr_build(r, 2), W, H, o["kps_xy"][f, :n], o["kps_xy"][f, :n], levels=2, win=21, iters=30)
        assert np.array_equal(o["lk_status"][f, :n], rst)
        assert np.array_equal(np.ascontiguousarray(o["lk_pts"][f, :n]).view(np.uint32), ref.view(np.uint32))
    # frames = 1, coalesce = 4: 8 submits, passes of four stereo frames (rows L, R, L, R in the lane)
    a1 = _run(api, fe, frames, 1, 8, lanes=2, match_lr=False, coalesce=4)
    b1 = _run(api, fe, frames, 1, 8, lanes=2, match_lr=False, coalesce=4, lr_lk=True)
    for s in range(8):
        _same_left(a1[s], b1[s], 1)
        _check_tracks(api, fe, b1[s], frames[s:s + 1], SEEDS[s:s + 1])
        # the same frame through either shape of the pipe: same keypoints, same tracks
        assert np.array_equal(b1[s]["lk_pts"][0].view(np.uint32), b[s // 4]["lk_pts"][s % 4].view(np.uint32)) and np.array_equal(b1[s]["lk_status"][0], b[s // 4]["lk_status"][s % 4])
    fe.close()


@pytest.mark.gpu
def test_lr_lk_with_the_other_pipe_options(frames):
    """cu_partition, lane_cus, netvlad_group, coalesce_depth, pinned staging off / NetVLAD off: none of them is refused with lr_lk, all give the same tracks"""
    api, fe = _fe("wino", max_batch=2)
    base = _run(api, fe, frames, 1, 6, lanes=3, match_lr=False, lr_lk=True)
    for kw in ({"cu_partition": True}, {"lane_cus": 128}, {"netvlad_group": 3}, {"coalesce": 2, "coalesce_depth": 1}, {"netvlad_inline": True}):
        got = _run(api, fe, frames, 1, 6, lanes=3, match_lr=False, lr_lk=True, **kw)
        for g, b in zip(got, base):
            n = int(b["n_kp"][0])
            assert int(g["n_kp"][0]) == n and int(g["n_kp"][1]) == 0, kw
            assert np.array_equal(g["kps_xy"][0, :n], b["kps_xy"][0, :n]) and np.array_equal(g["desc"][0, :n], b["desc"][0, :n]), kw
            assert np.array_equal(g["lk_pts"].view(np.uint32), b["lk_pts"].view(np.uint32)) and np.array_equal(g["lk_status"], b["lk_status"]), kw
            assert np.array_equal(g["netvlad"], b["netvlad"]) and np.array_equal(g["prev_n"], b["prev_n"]), kw
    # pinned_input: DMA straight from the caller's page-locked frames ([L | R] of two stereo frames in one run, and as two separate runs)
    import torch
    host = torch.from_numpy(np.stack([np.stack([frames[f][side] for f in range(2)]) for side in range(2)])).pin_memory()       # [side][frame][H][W]
    apart = torch.from_numpy(np.stack([frames[f][1] for f in range(2)])).pin_memory()
    pipe = api.StereoPipe(fe, lanes=2, frames=2, width=W, height=H, cap=CAP, match_lr=False, lr_lk=True, pinned_input=True)
    t0 = pipe.submit_ptr(host.data_ptr(), host.data_ptr() + 2 * H * W)
    t1 = pipe.submit_ptr(host.data_ptr(), apart.data_ptr())
    for t in (t0, t1):
        o = pipe.wait(t)
        for f in range(2):
            assert np.array_equal(o["lk_pts"][f].view(np.uint32), base[f]["lk_pts"][0].view(np.uint32)) and np.array_equal(o["lk_status"][f], base[f]["lk_status"][0])
        assert o["n_kp"][2:].tolist() == [0, 0]
    pipe.close()
    # without NetVLAD and without the temporal match
    pipe = api.StereoPipe(fe, lanes=2, frames=1, width=W, height=H, cap=CAP, netvlad=False, match_lr=False, match_prev=False, lr_lk=True)
    o = pipe.wait(pipe.submit(frames[0][0][None], frames[0][1][None]))
    assert o["netvlad"] is None and o["prev_n"] is None
    assert np.array_equal(o["lk_pts"].view(np.uint32), base[0]["lk_pts"].view(np.uint32)) and np.array_equal(o["lk_status"], base[0]["lk_status"])
    pipe.close(); fe.close()


@pytest.mark.gpu
def test_lk_track_stereo_device_alone(frames):
    """Item 5: d2fe_superpoint_extract_device on a stream, then d2fe_lk_track_stereo_device on the same stream with a workspace of exactly
    d2fe_lk_stereo_workspace_bytes; 1 and 5 frames; rows wider than the image with poisoned padding; one image without keypoints (threshold 0.99)."""
    import torch
    api, fe = _fe("wino", max_batch=5)
    _, fe99 = _fe("wino", max_batch=1, threshold=0.99)
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    stride = W + 48
    for n, empty in ((1, None), (5, 2)):
        host = np.full((2, n, H, stride), 201, np.uint8)          # poisoned padding
        for f in range(n):
            host[0, f, :, :W], host[1, f, :, :W] = frames[f]
        imgs = torch.from_numpy(host).to(dev)
        kps = torch.full((n, CAP, 2), -7.0, device=dev); scores = torch.empty((n, CAP), device=dev); desc = torch.empty((n, CAP, 256), device=dev)
        idx = torch.empty((n, CAP), dtype=torch.int32, device=dev); cnt = torch.full((n,), -1, dtype=torch.int32, device=dev)
        nbytes = api.lk_stereo_workspace_bytes(n, W, H, 2)
        ws = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=dev)
        pts = torch.full((n, CAP, 2), 123.0, device=dev); status = torch.full((n, CAP), 9, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        left, right = imgs[0].data_ptr(), imgs[1].data_ptr()
        fe.extract_device(left, n, W, H, kps.data_ptr(), scores.data_ptr(), desc.data_ptr(), idx.data_ptr(), CAP, cnt.data_ptr(), stream=st.cuda_stream,
                          stride=stride, image_stride=H * stride)
        if empty is not None:      # row `empty` again, by the handle whose threshold no score reaches, on the same stream
            fe99.extract_device(left + empty * H * stride, 1, W, H, kps[empty].data_ptr(), scores[empty].data_ptr(), desc[empty].data_ptr(), idx[empty].data_ptr(), CAP,
                                cnt[empty:].data_ptr(), stream=st.cuda_stream, stride=stride, image_stride=H * stride)
        api.lk_track_stereo_device(fe, left, right, n, W, H, kps.data_ptr(), cnt.data_ptr(), CAP, ws.data_ptr(), pts.data_ptr(), status.data_ptr(),
                                   stream=st.cuda_stream, stride=stride, image_stride=H * stride)
        st.synchronize()
        cnt_h, kps_h, pts_h, st_h = cnt.cpu().numpy(), kps.cpu().numpy(), pts.cpu().numpy(), status.cpu().numpy()
        total = nbytes // (2 * n)
        ws_h = ws.cpu().numpy()
        for f in range(n):
            k = int(cnt_h[f])
            if f == empty:
                assert k == 0
            else:
                assert k == CAP
            fl, frr = api.LKFrame(fe, frames[f][0], 2), api.LKFrame(fe, frames[f][1], 2)
            # the workspace holds the pyramids of d2fe_lk_frame_create, left ones first
            for side, lf in ((0, fl), (1, frr)):
                pyr = ws_h[(side * n + f) * total:(side * n + f + 1) * total]
                off = 0
                for l in range(3):
                    lv = lf.level(l)
                    assert np.array_equal(pyr[off:off + lv.size].reshape(lv.shape), lv)
                    off += lv.size
            ref, rst = api.lk_track(fe, fl, frr, kps_h[f, :k], kps_h[f, :k], api.WHOLE_IMG_MATCH, 0.0)
            fl.close(); frr.close()
            assert np.array_equal(st_h[f, :k], rst) and np.array_equal(np.ascontiguousarray(pts_h[f, :k]).view(np.uint32), ref.view(np.uint32))
            assert not st_h[f, k:].any() and not pts_h[f, k:].view(np.uint32).any()
            assert k == 0 or st_h[f, :k].sum() >= 150
    # parameter checks as d2fe_lk_track_batch
    for bad in ({"win": 20}, {"win": 25}, {"levels": 8}, {"iters": 0}):
        with pytest.raises(api.D2FEError) as e:
            api.lk_track_stereo_device(fe, left, right, n, W, H, kps.data_ptr(), cnt.data_ptr(), CAP, ws.data_ptr(), pts.data_ptr(), status.data_ptr(),
                                       stream=st.cuda_stream, stride=stride, image_stride=H * stride, **bad)
        assert e.value.code == -1
    fe99.close(); fe.close()


@pytest.mark.gpu
def test_lr_lk_contract(frames):
    """Item 6"""
    api, fe = _fe("wino", max_batch=2)
    with pytest.raises(api.D2FEError) as e:
        api.StereoPipe(fe, lanes=2, frames=1, width=W, height=H, cap=CAP, match_lr=True, lr_lk=True)
    assert e.value.code == -1 and "match_lr" in str(e.value)
    plain = api.StereoPipe(fe, lanes=2, frames=1, width=W, height=H, cap=CAP, match_lr=False)
    t = plain.submit(frames[0][0][None], frames[0][1][None])
    o = plain.wait(t)
    assert "lk_pts" not in o and "lk_status" not in o
    with pytest.raises(api.D2FEError) as e:
        plain.lk_result_raw(t)
    assert e.value.code == -5                         # D2FE_ERR_UNSUPPORTED
    plain.close()
    pipe = api.StereoPipe(fe, lanes=2, frames=1, width=W, height=H, cap=CAP, match_lr=False, lr_lk=True)
    t = pipe.submit(frames[0][0][None], frames[0][1][None])
    with pytest.raises(api.D2FEError) as e:
        pipe.lk_result_raw(t)
    assert e.value.code == -3                         # D2FE_ERR_NOT_READY: not waited for yet
    o = pipe.wait(t)
    assert int(o["n_kp"][0]) == CAP and int(o["n_kp"][1]) == 0 and o["lk_status"][0].sum() >= 150
    lk = pipe.lk_result_raw(t)
    assert (lk.frames, lk.cap) == (1, CAP)
    with pytest.raises(api.D2FEError) as e:
        pipe.lk_result_raw(t + 1)
    assert e.value.code == -1                         # unknown ticket
    pipe.close(); fe.close()


@pytest.mark.gpu
@pytest.mark.parametrize("F", [1, 8])
def test_lk_stage_launch_count(F, frames):
    """Item 7: the LK stage of a pass is levels + 1 = 3 launches whether the pass carries 1 or 8 stereo frames (d2fe_pipe_profile_read, stage "lk":
    one event pair per launch), and a pipe without the mode launches none."""
    api, fe = _fe("wino", max_batch=2 * F)
    L = np.stack([f[0] for f in frames[:F]]); R = np.stack([f[1] for f in frames[:F]])
    for lr_lk, want in ((True, 3), (False, 0)):
        pipe = api.StereoPipe(fe, lanes=2, frames=F, width=W, height=H, cap=CAP, match_lr=False, lr_lk=lr_lk)
        pipe.wait(pipe.submit(L, R))
        pipe.profile_enable(2)
        passes = 4
        for t in [pipe.submit(L, R) for _ in range(passes)]:
            pipe.wait_raw(t)
        prof = pipe.profile_read()
        assert list(prof)[-1] == "lk" and prof["lk"][1] == want * passes
        assert prof["conv1b"][1] == passes
        pipe.profile_enable(0)
        pipe.close()
    fe.close()


@pytest.mark.gpu
def test_lr_lk_through_the_cpp_mirror(tmp_path, sp_weights):
    """include/d2fe.hpp: StereoPipe with cfg.lr_lk = 1 from g++ (tests/cpp/pipe_lk_test.cpp): infer()'s left keypoints, and for each the bits of d2fe_lk_track"""
    import os
    import struct
    import subprocess
    from d2slam_amd import build as hipbuild
    from d2slam_amd.weights import SP_LAYERS
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = hipbuild.build()
    exe = str(tmp_path / "pipe_lk_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "pipe_lk_test.cpp"),
                           "-L", os.path.dirname(lib), "-ld2fe_hip", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib",
                           "-Wl,--allow-shlib-undefined", "-o", exe])
    h, w, maxkp = 240, 320, 150
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
