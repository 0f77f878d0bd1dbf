"""The stereo pipe's sp_lk mode (d2fe_pipe_config.sp_lk with lr_lk, include/d2fe.h): the reference's default stereo tracker -- sp_track_use_lk = true,
D2FeatureTracker::trackLK(frame) (d2featuretracker.cpp:472-621) then trackLK(left, right) (:697-752) -- with the LK-carried landmark list kept on the device and
carried across frames, passes and lanes.  All on sliding_stereo(24 frames, 480 x 640, seed 7005, disparity 24): one wide synth_image, left frame t = the window at
24 + 3 t px, right frame t = the window at 3 t, independent sigma-3 noise on every frame; seeded weights, 200 keypoints, the Winograd mode and the exact mode.
The host composition every result is held to: api.LKFrame + api.lk_track on the pipe's own keypoints + tests/helpers/lk_carry_ref.py (NumPy, itself held to a
naive transcription of the reference lines in tests/test_pipe_sp_lk_cpu.py)."""
import numpy as np
import pytest

from tests.helpers import lk_carry_ref as ref

H, W, CAP = 480, 640, 200
SEED, DISP, STEP, NF = 7005, 24, 3, 24
TRACK_KEYS = ("track_n", "track_pts", "track_id", "track_src", "track_kp", "track_desc", "track_scores", "track_right_pts", "track_right_status",
              "track_n_tracked_in", "track_n_lost", "track_n_removed_near", "track_n_new")
LEFT_KEYS = ("kps_xy", "scores", "desc")


@pytest.fixture(scope="module")
def frames():
    return ref.sliding_stereo(NF, H, W, SEED, DISP, STEP)


def _fe(prec, max_batch=8):
    from d2slam_amd import api, netvlad as nvm
    from d2slam_amd.weights import synthetic_superpoint_weights
    fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=CAP, input_width=W, input_height=H, max_batch=max_batch,
                                           precision={"wino": api.PREC_F32_WINO, "f32": api.PREC_F32}[prec]))
    fe.load_superpoint(synthetic_superpoint_weights(dustbin_bias=7.5)); fe.load_netvlad(nvm.synthetic_netvlad_weights())
    return api, fe


def _run(api, fe, frames, F, n_frames=NF, per_frame=True, **kw):
    """the first n_frames frames through one pipe, F per submit, lanes * coalesce submits in flight; copies of the results, one dict per FRAME (or per submit)"""
    kw.setdefault("match_lr", False); kw.setdefault("lr_lk", True); kw.setdefault("sp_lk", True)
    pipe = api.StereoPipe(fe, frames=F, width=W, height=H, cap=CAP, netvlad=kw.pop("netvlad", True), match_prev=kw.pop("match_prev", True), **kw)
    inflight = pipe.lanes * kw.get("coalesce", 1)
    nsub = n_frames // F
    tk, out = [], []
    take = lambda: out.append({k: (None if v is None else v.copy()) for k, v in pipe.wait(tk[len(out)]).items()})
    for i in range(nsub):
        fr = frames[i * F:(i + 1) * F]
        tk.append(pipe.submit(np.stack([f[0] for f in fr]), np.stack([f[1] for f in fr])))
        if len(tk) > inflight - 1:
            take()
    while len(out) < nsub:
        take()
    pipe.close()
    if not per_frame:
        return out
    res = []
    for o in out:
        for f in range(F):
            r = {k: o[k][f] for k in TRACK_KEYS}
            r.update({k: o[k][f] for k in LEFT_KEYS}); r["n_kp"] = int(o["n_kp"][f])
            res.append(r)
    return res


def _keypoints(res):
    return [(r["kps_xy"][:r["n_kp"]], r["scores"][:r["n_kp"]], r["desc"][:r["n_kp"]]) for r in res]


def _api_tracker(api, fe):
    def track(prev_img, cur_img, pts):
        a, b = api.LKFrame(fe, prev_img, 2), api.LKFrame(fe, cur_img, 2)
        out = api.lk_track(fe, a, b, pts, pts, api.WHOLE_IMG_MATCH, 0.0)
        a.close(); b.close()
        return out
    return track


def _orc_tracker(orc):
    return lambda prev_img, cur_img, pts: orc.lk_track(orc.pyr_build(prev_img, 2), orc.pyr_build(cur_img, 2), W, H, pts, pts, levels=2, win=21, iters=30)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same_frame(r, c, T, where):
    """one frame of the pipe (r) against the composition (c): every array bit for bit, zeros behind the end"""
    n = c["n"]
    assert int(r["track_n"]) == n, where
    for k in ("n_tracked_in", "n_lost", "n_removed_near", "n_new"):
        assert int(r["track_" + k]) == c[k], (where, k)
    assert r["track_pts"].shape == (T, 2) and r["track_desc"].shape == (T, 256) and r["track_right_status"].shape == (T,) and r["track_right_status"].dtype == np.uint8
    assert np.array_equal(_bits(r["track_pts"][:n]), _bits(c["pts"])), where
    for k in ("id", "src", "kp"):
        assert np.array_equal(r["track_" + k][:n], c[k]), (where, k)
    assert np.array_equal(_bits(r["track_desc"][:n]), _bits(c["desc"])) and np.array_equal(_bits(r["track_scores"][:n]), _bits(c["scores"])), where
    assert np.array_equal(r["track_right_status"][:n], c["right_status"]) and np.array_equal(_bits(r["track_right_pts"][:n]), _bits(c["right_pts"])), where
    for k in ("pts", "id", "src", "kp", "desc", "scores", "right_pts", "right_status"):
        assert not np.ascontiguousarray(r["track_" + k][n:]).view(np.uint8).any(), (where, k)


def _discovery_rows(res, comp):
    """the descriptor of every entry is the SuperPoint row of the frame that discovered it -- followed through the src chain, independently of compose()'s carry"""
    origin = {}
    for t, c in enumerate(comp):
        for i in range(c["n"]):
            if c["src"][i] < 0:
                origin[int(c["id"][i])] = (t, int(c["kp"][i]))
            t0, kp = origin[int(c["id"][i])]
            assert np.array_equal(_bits(res[t]["track_desc"][i]), _bits(res[t0]["desc"][kp])) and res[t]["track_scores"][i] == res[t0]["scores"][kp]
    assert sorted(origin) == list(range(len(origin)))          # ids are handed out in order of discovery, without gaps


def _tracking_figures(comp, what):
    """(smallest share of a frame's previous list that the tracker keeps, largest distance of a kept entry to (x - 3, y); the same for the right tracks at (x + D, y))"""
    share, dist, rshare, rdist = [], 0.0, [], 0.0
    for t, c in enumerate(comp):
        if t > 0 and len(c["trk_status"]):
            ok = c["trk_status"] != 0
            share.append(ok.mean())
            d = np.linalg.norm(c["trk_pts"][ok].astype(np.float64) - (comp[t - 1]["pts"][ok].astype(np.float64) + [-STEP, 0.0]), axis=1)
            dist = max(dist, float(d.max()) if len(d) else 0.0)
        ok = c["right_status"] != 0
        rshare.append(ok.mean())
        d = np.linalg.norm(c["right_pts"][ok].astype(np.float64) - (c["pts"][ok].astype(np.float64) + [DISP, 0.0]), axis=1)
        rdist = max(rdist, float(d.max()) if len(d) else 0.0)
    fig = (min(share), dist, min(rshare), rdist)
    print("%s: temporal share >= %.4f, largest distance %.4f px; right share >= %.4f, largest distance %.4f px" % ((what,) + fig))
    return fig


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["wino", "f32"])
def test_sp_lk_pipe_is_the_host_composition(prec, frames, orc):
    """Items 1, 6, 7.  (1) per frame the pipe's list, id, src, kp, counts, descriptors, scores and right tracks equal the host composition bit for bit, the
    descriptors are the discovery frame's SuperPoint rows, and frames 4..7 also equal the composition with the ORACLE's pyramids and tracker.  (6) every branch
    fires, asserted on the composition first: default parameters lose a track and append after frame 0; near_lk_thread_rate = 30 removes near points;
    total_feature_num = 40 overshoots to 41.  (7) it tracks: kept entries sit at (x - 3, y), right tracks at (x + 24, y).
    Floors of (7): the CPU oracle composition (oracle SuperPoint + oracle LK + the NumPy list logic) on the same 24 frames, identical in both modes, keeps at least
    0.9683 of every frame's previous list with a largest distance of 0.7177 px to (x - 3, y), and tracks at least 0.9206 of every list into the right image with a
    largest distance of 0.4507 px to (x + 24, y).  Margin: a tenth of the share, 0.25 px on the distance."""
    api, fe = _fe(prec)
    track = _api_tracker(api, fe)
    runs = {}
    for name, prm in (("default", {}), ("near30", {"near_lk_thread_rate": 30.0}), ("total40", {"total_feature_num": 40})):
        res = _run(api, fe, frames, 4, lanes=2, track_params=prm or None)
        comp = ref.compose(frames, _keypoints(res), track, prm)
        print(name, "n", [c["n"] for c in comp], "lost", [c["n_lost"] for c in comp], "near", [c["n_removed_near"] for c in comp], "new", [c["n_new"] for c in comp])
        # (6) conditions on the inputs
        if name == "default":
            assert any(c["n_lost"] > 0 for c in comp) and any(c["n_new"] > 0 for c in comp[1:])
        elif name == "near30":
            assert any(c["n_removed_near"] > 0 for c in comp)
        else:
            assert any(c["n"] == 41 for c in comp) and all(c["n"] <= 41 for c in comp)
        T = (prm.get("total_feature_num", 150)) + 1
        for t in range(NF):
            _same_frame(res[t], comp[t], T, (name, t))
        _discovery_rows(res, comp)
        runs[name] = (res, comp)
    res, comp = runs["default"]
    # (1) the oracle on one stretch of four frames, from the state the chain had reached
    oc = ref.compose(frames[4:8], _keypoints(res[4:8]), _orc_tracker(orc), {}, state=comp[3]["state"])
    for t in range(4, 8):
        _same_frame(res[t], oc[t - 4], 151, ("oracle", t))
    # (7)
    share, dist, rshare, rdist = _tracking_figures(comp, prec)
    assert share >= 0.9683 * 0.9 and dist <= 0.7177 + 0.25
    assert rshare >= 0.9206 * 0.9 and rdist <= 0.4507 + 0.25
    fe.close()


@pytest.mark.gpu
def test_sp_lk_lists_longer_than_two_waves(frames):
    """The finishing workgroup works 64 entries at a time (the rounds of step b, the `j += 64` strides of steps c and d, step e and the left -> right launch past
    slot 64), and the runs above never hold more than 64 entries.  Here feature_min_dist = 6 lets the list fill up to total_feature_num + 1 = 151, the reference's
    default size; a second run with near_lk_thread_rate = 9 > feature_min_dist prunes with more than 64 kept entries in front of the candidate.  The conditions are
    asserted on the host composition before the pipe is compared: a list longer than 128, more than 128 survivors of the tracker in one frame (three rounds of
    step b), and in the second run a frame that removes near points out of more than 64 survivors."""
    api, fe = _fe("wino")
    track = _api_tracker(api, fe)
    for name, prm in (("dense", {"feature_min_dist": 6.0}), ("dense_near9", {"feature_min_dist": 6.0, "near_lk_thread_rate": 9.0})):
        res = _run(api, fe, frames, 4, n_frames=12, lanes=2, track_params=prm)
        comp = ref.compose(frames[:12], _keypoints(res), track, prm)
        print(name, "n", [c["n"] for c in comp], "lost", [c["n_lost"] for c in comp], "near", [c["n_removed_near"] for c in comp], "new", [c["n_new"] for c in comp])
        assert max(c["n"] for c in comp) > 128
        assert any(c["n_tracked_in"] - c["n_lost"] > 128 for c in comp)
        assert any(c["n_new"] > 0 and c["n"] - c["n_new"] > 64 for c in comp[1:])           # replenishment tested against more than 64 entries
        if name == "dense_near9":
            assert any(c["n_removed_near"] > 0 and c["n_tracked_in"] - c["n_lost"] > 64 for c in comp)
        for t in range(12):
            _same_frame(res[t], comp[t], 151, (name, t))
            assert (res[t]["track_right_status"][64:comp[t]["n"]] != 0).any() or comp[t]["n"] <= 64      # right tracks past slot 64 are live
        _discovery_rows(res, comp)
    fe.close()


@pytest.mark.gpu
def test_sp_lk_results_do_not_depend_on_the_shape_of_the_pipe(frames):
    """Item 2: the same 24 frames through frames = 1 / lanes = 1 (the carried pyramid lives in the workspace the next pass overwrites), frames = 4 / lanes = 2,
    frames = 1 / coalesce = 4 / lanes = 2, frames = 3 / lanes = 4 (pass boundaries aligned with nothing), and with the other options of the pipe: identical per frame"""
    api, fe = _fe("wino", max_batch=4)
    base = _run(api, fe, frames, 1, lanes=1)
    assert any(int(r["track_n_lost"]) > 0 for r in base) and any(int(r["track_n_new"]) > 0 for r in base[1:])
    shapes = [dict(F=4, lanes=2), dict(F=1, lanes=2, coalesce=4), dict(F=3, lanes=4), dict(F=1, lanes=3, cu_partition=True), dict(F=1, lanes=2, lane_cus=128),
              dict(F=1, lanes=4, netvlad_group=2), dict(F=1, lanes=3, coalesce=2, coalesce_depth=1), dict(F=2, lanes=2, netvlad_inline=True),
              dict(F=2, lanes=2, netvlad=False, match_prev=False)]
    for kw in shapes:
        kw = dict(kw)
        got = _run(api, fe, frames, kw.pop("F"), **kw)
        assert len(got) == len(base)
        for t, (g, b) in enumerate(zip(got, base)):
            assert g["n_kp"] == b["n_kp"]
            for k in TRACK_KEYS + LEFT_KEYS:
                assert np.array_equal(np.ascontiguousarray(g[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)), (kw, t, k)
    # pinned_input: DMA straight from the caller's page-locked frames
    import torch
    host = torch.from_numpy(np.stack([np.stack([frames[f][side] for f in range(4)]) for side in range(2)])).pin_memory()       # [side][frame][H][W]
    pipe = api.StereoPipe(fe, lanes=2, frames=2, width=W, height=H, cap=CAP, match_lr=False, lr_lk=True, sp_lk=True, pinned_input=True)
    tk = [pipe.submit_ptr(host.data_ptr() + 2 * i * H * W, host.data_ptr() + (4 + 2 * i) * H * W) for i in range(2)]
    for i, t in enumerate(tk):
        o = pipe.wait(t)
        for f in range(2):
            for k in TRACK_KEYS:
                assert np.array_equal(np.ascontiguousarray(o[k][f]).view(np.uint8), np.ascontiguousarray(base[2 * i + f][k]).view(np.uint8)), k
    pipe.close(); fe.close()


@pytest.mark.gpu
def test_sp_lk_leaves_the_rest_of_the_result_alone(frames):
    """Item 3: left rows, NetVLAD and prev_* equal the lr_lk pipe's; lr_* are NULL, right rows empty, no lk_* keys (the per-keypoint launch is not issued)"""
    api, fe = _fe("wino")
    for F, kw in ((4, dict(lanes=2)), (1, dict(lanes=2, coalesce=4))):
        a = _run(api, fe, frames, F, n_frames=16, per_frame=False, sp_lk=False, **kw)
        b = _run(api, fe, frames, F, n_frames=16, per_frame=False, **kw)
        for oa, ob in zip(a, b):
            for f in range(F):
                n = int(oa["n_kp"][f])
                assert n == int(ob["n_kp"][f]) and n > 0 and int(ob["n_kp"][F + f]) == 0
                m = int(oa["prev_n"][f])
                assert m == int(ob["prev_n"][f])
                for k in LEFT_KEYS + ("prev_q", "prev_t", "prev_dist"):          # whole rows, the tails behind n / m included, as bytes
                    assert np.array_equal(_bytes(oa[k][f]), _bytes(ob[k][f])), k
            assert np.array_equal(_bytes(oa["netvlad"]), _bytes(ob["netvlad"]))
            assert all(ob[k] is None for k in ("lr_q", "lr_t", "lr_dist", "lr_n"))
            assert "lk_pts" in oa and "lk_pts" not in ob and "lk_status" not in ob and "track_n" not in oa
    fe.close()


@pytest.mark.gpu
def test_lk_carry_step_device_alone(frames):
    """Item 4: d2fe_lk_carry_step_device on a stream of the caller's, on pyramids built by the pyramids-only form of d2fe_lk_track_stereo_device, against the
    composition: 640 x 480 with the keypoints of d2fe_superpoint_extract_device, and a geometry that is no multiple of 8 (326 x 243, synthetic keypoints, 64-dim
    descriptors, total_feature_num = 30), and 640 x 480 again at feature_min_dist = 6, near_lk_thread_rate = 9, whose lists pass 128 entries; the first call of
    each has n_prev = 0, one call has n_kp = 0; poisoned list blocks apart from the documented zero header"""
    import torch
    api, fe = _fe("wino", max_batch=4)
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    rng = np.random.RandomState(3)
    for (w, h, D, prm, nfr, empty, nk_range) in ((W, H, 256, {}, 4, None, None), (326, 243, 64, {"total_feature_num": 30, "feature_min_dist": 12.5}, 5, 2, (60, 120)),
                                                 (W, H, 256, {"feature_min_dist": 6.0, "near_lk_thread_rate": 9.0}, 4, None, None)):
        seq = [(l[:h, :w].copy(), r[:h, :w].copy()) for l, r in frames[:nfr]]
        imgs = torch.from_numpy(np.stack([np.stack([s[side] for s in seq]) for side in range(2)])).to(dev)      # [side][frame][h][w]
        kps = torch.zeros((nfr, CAP, 2), device=dev); scores = torch.zeros((nfr, CAP), device=dev); desc = torch.zeros((nfr, CAP, D), device=dev)
        cnt = torch.zeros((nfr,), dtype=torch.int32, device=dev)
        if D == 256:
            idx = torch.empty((nfr, CAP), dtype=torch.int32, device=dev)
            fe.extract_device(imgs[0].data_ptr(), nfr, w, h, kps.data_ptr(), scores.data_ptr(), desc.data_ptr(), idx.data_ptr(), CAP, cnt.data_ptr(), stream=st.cuda_stream)
        else:
            nk = rng.randint(nk_range[0], nk_range[1], nfr)
            if empty is not None:
                nk[empty] = 0
            k_h = np.zeros((nfr, CAP, 2), np.float32)
            for f in range(nfr):
                k_h[f, :nk[f]] = np.stack([rng.randint(4, w - 4, nk[f]), rng.randint(4, h - 4, nk[f])], axis=1)
            kps.copy_(torch.from_numpy(k_h)); scores.copy_(torch.from_numpy(rng.rand(nfr, CAP).astype(np.float32)))
            desc.copy_(torch.from_numpy(rng.randn(nfr, CAP, D).astype(np.float32))); cnt.copy_(torch.from_numpy(nk.astype(np.int32)))
        tp = api.track_params(**prm)
        T = tp.total_feature_num + 1
        lb = api.lk_carry_list_bytes(T, D)
        lists = torch.full((nfr + 1, lb // 4), -77.0, device=dev)
        lists[0] = 0.0                                          # the empty list
        lists[:, :64] = 0.0                                     # the documented contract: the header (arrival counter) of a block is zero before its first use
        nbytes = api.lk_stereo_workspace_bytes(nfr, w, h, 2)
        ws = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=dev)
        next_id = torch.full((1,), 1000, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        api.lk_track_stereo_device(fe, imgs[0].data_ptr(), imgs[1].data_ptr(), nfr, w, h, None, None, 0, ws.data_ptr(), None, None, stream=st.cuda_stream)
        total = nbytes // (2 * nfr)
        for f in range(nfr):
            api.lk_carry_step(fe, ws.data_ptr() + max(f - 1, 0) * total, ws.data_ptr() + f * total, w, h, lists[f].data_ptr(), lists[f + 1].data_ptr(),
                              kps[f].data_ptr(), scores[f].data_ptr(), desc[f].data_ptr(), cnt[f:].data_ptr(), CAP, next_id.data_ptr(), tp=tp, desc_dim=D,
                              stream=st.cuda_stream)
        st.synchronize()
        cnt_h, kps_h, sc_h, d_h = cnt.cpu().numpy(), kps.cpu().numpy(), scores.cpu().numpy(), desc.cpu().numpy()
        kp_list = [(kps_h[f, :cnt_h[f]], sc_h[f, :cnt_h[f]], d_h[f, :cnt_h[f]]) for f in range(nfr)]
        full = {k: getattr(tp, k) for k in ("total_feature_num", "feature_min_dist", "near_lk_thread_rate")}
        comp = ref.compose(seq, kp_list, _api_tracker(api, fe), full)
        if empty is not None:
            assert cnt_h[empty] == 0 and comp[empty]["n_new"] == 0 and comp[empty]["n_tracked_in"] > 0
        assert comp[0]["n_tracked_in"] == 0 and comp[0]["n"] > 0 and any(c["n"] - c["n_new"] > 0 for c in comp[1:])
        if prm.get("feature_min_dist") == 6.0:       # the third run: lists longer than two waves (every 64-entry round and stride of the finishing workgroup)
            print("step alone, dense: n", [c["n"] for c in comp], "lost", [c["n_lost"] for c in comp], "near", [c["n_removed_near"] for c in comp])
            assert max(c["n"] for c in comp) > 128 and any(c["n_tracked_in"] - c["n_lost"] > 64 for c in comp)
        lists_h = lists.cpu().numpy()
        nid = 1000
        for f in range(nfr):
            v = api.lk_carry_list_views(lists_h[f + 1], T, D)
            c = comp[f]
            n = c["n"]
            assert (v["n"], v["n_tracked_in"], v["n_lost"], v["n_removed_near"], v["n_new"]) == (n, c["n_tracked_in"], c["n_lost"], c["n_removed_near"], c["n_new"]), f
            nid += c["n_new"]
            assert v["hdr"][5] == 0 and v["hdr"][6] == nid and not v["hdr"][7:].any()
            assert np.array_equal(_bits(v["pts"][:n]), _bits(c["pts"])) and np.array_equal(v["src"][:n], c["src"]) and np.array_equal(v["kp"][:n], c["kp"])
            assert np.array_equal(v["id"][:n], c["id"] + 1000)
            assert np.array_equal(_bits(v["desc"][:n]), _bits(c["desc"])) and np.array_equal(_bits(v["scores"][:n]), _bits(c["scores"]))
            m = c["n_tracked_in"]
            assert np.array_equal(_bits(v["trk_xy"][:m]), _bits(c["trk_pts"])) and np.array_equal(v["trk_status"][:m], c["trk_status"])
            for k in ("pts", "id", "src", "kp", "desc", "scores"):
                assert not np.ascontiguousarray(v[k][n:]).view(np.uint8).any(), k
            assert not v["trk_xy"][m:].view(np.uint8).any() and not v["trk_status"][m:].any()
        assert int(next_id.cpu()[0]) == nid
        # refusals of the call: D2FE_ERR_INVALID, nothing is launched
        args = (fe, ws.data_ptr(), ws.data_ptr() + total, w, h, lists[0].data_ptr(), lists[1].data_ptr(), kps[0].data_ptr(), scores[0].data_ptr(), desc[0].data_ptr(),
                cnt.data_ptr(), CAP, next_id.data_ptr())
        for bad in ({"total_feature_num": 1024}, {"total_feature_num": -1}, {"win": 20}, {"levels": 8}, {"iters": 0}, {"near_lk_thread_rate": -1.0}):
            with pytest.raises(api.D2FEError) as e:
                api.lk_carry_step(*args, tp=api.track_params(**bad), desc_dim=D, stream=st.cuda_stream)
            assert e.value.code == -1
        with pytest.raises(api.D2FEError) as e:
            api.lk_carry_step(*(args[:5] + (lists[1].data_ptr(),) + args[6:]), tp=tp, desc_dim=D, stream=st.cuda_stream)       # previous == current
        assert e.value.code == -1
    fe.close()


@pytest.mark.gpu
def test_sp_lk_contract(frames):
    """Item 5: the refusals, each with the documented status, and the pipe stays usable where the header says so"""
    api, fe = _fe("wino", max_batch=2)
    l, r = frames[0][0][None], frames[0][1][None]
    with pytest.raises(api.D2FEError) as e:
        api.StereoPipe(fe, lanes=2, frames=1, width=W, height=H, cap=CAP, match_lr=False, sp_lk=True)
    assert e.value.code == -1 and "lr_lk" in str(e.value)
    with pytest.raises(api.D2FEError) as e:        # total_feature_num + 1 > 1024, at creation through the Python constructor
        api.StereoPipe(fe, lanes=2, frames=1, width=W, height=H, cap=CAP, match_lr=False, lr_lk=True, sp_lk=True, track_params={"total_feature_num": 1024})
    assert e.value.code == -1 and "1024" in str(e.value)
    plain = api.StereoPipe(fe, lanes=2, frames=1, width=W, height=H, cap=CAP, match_lr=False, lr_lk=True)
    with pytest.raises(api.D2FEError) as e:
        plain.set_track_params({})
    assert e.value.code == -1
    t = plain.submit(l, r)
    assert "track_n" not in plain.wait(t)
    with pytest.raises(api.D2FEError) as e:
        plain.track_result_raw(t)
    assert e.value.code == -5                         # D2FE_ERR_UNSUPPORTED
    plain.close()
    pipe = api.StereoPipe(fe, lanes=2, frames=1, width=W, height=H, cap=CAP, match_lr=False, lr_lk=True, sp_lk=True)
    for bad in ({"total_feature_num": 1024}, {"levels": 3}, {"win": 22}, {"feature_min_dist": -1.0}):
        with pytest.raises(api.D2FEError) as e:
            pipe.set_track_params(bad)
        assert e.value.code == -1
    pipe.set_track_params({"total_feature_num": 1023})      # the largest list
    pipe.set_track_params({"total_feature_num": 40})        # ... and still before the first submit
    t = pipe.submit(l, r)
    with pytest.raises(api.D2FEError) as e:
        pipe.set_track_params({"total_feature_num": 50})
    assert e.value.code == -1 and "first submit" in str(e.value)
    with pytest.raises(api.D2FEError) as e:
        pipe.track_result_raw(t)
    assert e.value.code == -3                         # D2FE_ERR_NOT_READY: not waited for yet
    o = pipe.wait(t)                                  # the refusals left the pipe usable
    assert int(o["track_n"][0]) == 41 and o["track_pts"].shape == (1, 41, 2) and "lk_pts" not in o
    with pytest.raises(api.D2FEError) as e:
        pipe.lk_result_raw(t)
    assert e.value.code == -5 and "d2fe_pipe_track_result_get" in str(e.value)
    tr = pipe.track_result_raw(t)
    assert (tr.frames, tr.cap_tracks, tr.desc_dim, tr.list_words * 4) == (1, 41, 256, api.lk_carry_list_bytes(41, 256))
    with pytest.raises(api.D2FEError) as e:
        pipe.track_result_raw(t + 1)
    assert e.value.code == -1                         # unknown ticket
    o2 = pipe.wait(pipe.submit(l, r))
    assert int(o2["track_n_tracked_in"][0]) == 41
    pipe.close(); fe.close()


@pytest.mark.gpu
@pytest.mark.parametrize("F", [1, 8])
def test_sp_lk_stage_launch_count(F, frames):
    """the LK stage of a pass with F frames: the two pyramid launches, ONE launch per frame of the chain, ONE left -> right launch = F + 3 (d2fe_pipe_profile_read,
    stage "lk": one event pair per launch), against 3 of the lr_lk pipe; no stage was added"""
    api, fe = _fe("wino", max_batch=F)
    L = np.stack([f[0] for f in frames[:F]]); R = np.stack([f[1] for f in frames[:F]])
    for sp_lk, want in ((True, F + 3), (False, 3)):
        pipe = api.StereoPipe(fe, lanes=2, frames=F, width=W, height=H, cap=CAP, match_lr=False, lr_lk=True, sp_lk=sp_lk)
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
def test_sp_lk_through_the_cpp_mirror(tmp_path, sp_weights):
    """include/d2fe.hpp: StereoPipe with cfg.lr_lk = cfg.sp_lk = 1 and StereoFrameResult::tracks from g++ (tests/cpp/pipe_sp_lk_test.cpp)"""
    import os
    import struct
    import subprocess
    from d2slam_amd import build as hipbuild
    from d2slam_amd.synth import synth_stereo
    from d2slam_amd.weights import SP_LAYERS
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = hipbuild.build()
    exe = str(tmp_path / "pipe_sp_lk_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "pipe_sp_lk_test.cpp"),
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
