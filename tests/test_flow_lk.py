"""The flow landmarks on the device (include/d2fe.h): d2fe_detect_fast_device against d2fe_detect_fast_by_region and the oracle, bit for bit, and
d2fe_lk_flow_step_device against the host composition api.LKFrame + api.lk_track + api.detectFastByRegion + tests/helpers/flow_lk_ref.py (NumPy, itself held to a naive
transcription of the reference lines in tests/test_flow_lk_cpu.py), every field and header word.  The dot sequences are static images (the tracker returns every entry
where it was, exactly), so keypoints and brightness decide what each frame does; what they are built to do is asserted on the composition before anything is compared."""
import numpy as np
import pytest

from tests.helpers import flow_lk_ref as ref
from tests.helpers.lk_carry_ref import sliding_stereo


def _fe():
    from d2slam_amd import api
    return api, api.FrontEnd(api.SuperPointConfig(input_width=64, input_height=64, max_batch=1))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- d2fe_detect_fast_device ----------------------------------------------------------------------------------------------------------------------------------------
def _detect_dev(api, fe, img, features, cap_tracks, cap=None, cols=3, rows=4, thr=10):
    """one call on a fresh scratch; returns (xy [cap, 2], response [cap], n) as the device left them over a -7 fill"""
    import torch
    dev = torch.device("cuda", 0)
    h, w = img.shape
    cap = cap or max(features, 1)
    d_img = torch.from_numpy(img).to(dev)
    d_feat = torch.tensor([features], dtype=torch.int32, device=dev)
    xy = torch.full((cap, 2), -7.0, device=dev); resp = torch.full((cap,), -7, dtype=torch.int32, device=dev); n = torch.full((1,), -7, dtype=torch.int32, device=dev)
    scratch = torch.full((api.lk_flow_scratch_bytes(w, h, cap_tracks, cols, rows),), 0xAB, dtype=torch.uint8, device=dev)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    api.detect_fast_device(fe, d_img.data_ptr(), w, h, d_feat.data_ptr(), cap_tracks, xy.data_ptr(), resp.data_ptr(), cap, n.data_ptr(), scratch.data_ptr(), cols, rows, thr,
                           stream=st.cuda_stream)
    st.synchronize()
    return xy.cpu().numpy(), resp.cpu().numpy(), int(n.cpu()[0])


def _same_as_the_host_detectors(api, fe, orc, img, features, cap_tracks, where):
    xy, resp, n = _detect_dev(api, fe, img, features, cap_tracks)
    f = api.LKFrame(fe, img, 0)
    hxy, hresp = api.detectFastByRegion(fe, f, features, 3, 4, 10, with_response=True)
    f.close()
    oxy, oresp = orc.fast_by_region(img, features, 3, 4, 10)
    assert n == len(hxy) == len(oxy), (where, n, len(hxy), len(oxy))
    assert np.array_equal(_bits(xy[:n]), _bits(hxy)) and np.array_equal(resp[:n], hresp), where
    assert np.array_equal(_bits(xy[:n]), _bits(oxy)) and np.array_equal(resp[:n], oresp), where
    assert (xy[n:] == -7.0).all() and (resp[n:] == -7).all(), where          # nothing behind the end is touched
    return n


@pytest.mark.gpu
def test_detect_fast_device_on_dot_images(orc):
    api, fe = _fe()
    # 96 x 64: regions of 32 x 16.  Dots inside regions, within 3 px of region borders (never corners), of equal brightness in different regions (the order decides)
    dots = [(10, 8, 90), (50, 8, 90), (74, 9, 90), (40, 40, 200), (20, 20, 120), (75, 55, 61), (12, 56, 120), (45, 25, 90),
            (31, 8, 250), (33, 24, 250), (2, 40, 250), (60, 15, 250), (60, 17, 250), (93, 60, 250)]
    img = ref.dot_image(64, 96, dots)
    for features in (50, 8, 5, 1):
        n = _same_as_the_host_detectors(api, fe, orc, img, features, 32, ("96x64", features))
        assert n == min(features, 8)
    # 100 x 70: regions of 33 x 17, one leftover column and two leftover rows; dots in and beside them
    dots = [(10, 8, 90), (97, 10, 140), (99, 30, 250), (98, 50, 250), (50, 68, 250), (50, 69, 250), (60, 64, 130), (60, 62, 130), (95, 64, 77), (70, 40, 77), (36, 20, 99)]
    img = ref.dot_image(70, 100, dots)
    for features in (40, 3):
        _same_as_the_host_detectors(api, fe, orc, img, features, 24, ("100x70", features))
    assert _same_as_the_host_detectors(api, fe, orc, np.full((64, 96), 50, np.uint8), 30, 24, "constant") == 0
    fe.close()


@pytest.mark.gpu
def test_detect_fast_device_on_noise_up_to_the_selection_capacity(orc):
    """nearly every pixel of a uint8 noise image is a candidate: the per-region cap, thousands of candidates with few distinct responses, and at features = 2 * 1023
    the selection at the capacity its LDS is sized for"""
    api, fe = _fe()
    img = np.random.RandomState(11).randint(0, 256, (120, 160)).astype(np.uint8)
    for features in (1, 5, 300, 2 * 1023):
        n = _same_as_the_host_detectors(api, fe, orc, img, features, 1023, ("noise", features))
        assert n == min(features, 1475)          # 1475 local maxima in this image: the last case takes them all, sorted
    # a larger image, so that 2 * 1023 are selected from several thousand: the selection at the capacity its LDS is sized for
    big = np.random.RandomState(13).randint(0, 256, (243, 326)).astype(np.uint8)
    assert _same_as_the_host_detectors(api, fe, orc, big, 2 * 1023, 1023, "noise 326 x 243") == 2 * 1023
    # the count is clamped to what the scratch holds (2 * cap_tracks), and the output to its capacity
    xy, resp, n = _detect_dev(api, fe, img, 300, 24, cap=300)
    oxy, oresp = orc.fast_by_region(img, 48, 3, 4, 10)
    assert n == 48 and np.array_equal(_bits(xy[:n]), _bits(oxy)) and np.array_equal(resp[:n], oresp) and (resp[n:] == -7).all()
    xy, resp, n = _detect_dev(api, fe, img, 300, 150, cap=20)
    oxy, oresp = orc.fast_by_region(img, 300, 3, 4, 10)
    assert n == 20 and np.array_equal(_bits(xy), _bits(oxy[:20])) and np.array_equal(resp, oresp[:20])
    fe.close()


@pytest.mark.gpu
def test_detect_fast_device_with_nothing_to_detect():
    """features = 0 and -3 in device memory: n = 0, the outputs and the scratch untouched"""
    import torch
    api, fe = _fe()
    dev = torch.device("cuda", 0)
    img = np.random.RandomState(12).randint(0, 256, (120, 160)).astype(np.uint8)
    d_img = torch.from_numpy(img).to(dev)
    for features in (0, -3):
        d_feat = torch.tensor([features], dtype=torch.int32, device=dev)
        xy = torch.full((16, 2), -7.0, device=dev); resp = torch.full((16,), -7, dtype=torch.int32, device=dev); n = torch.full((1,), -7, dtype=torch.int32, device=dev)
        scratch = torch.full((api.lk_flow_scratch_bytes(160, 120, 24),), 0xAB, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        api.detect_fast_device(fe, d_img.data_ptr(), 160, 120, d_feat.data_ptr(), 24, xy.data_ptr(), resp.data_ptr(), 16, n.data_ptr(), scratch.data_ptr())
        fe.sync()
        torch.cuda.synchronize()
        assert int(n.cpu()[0]) == 0 and (xy.cpu().numpy() == -7.0).all() and (resp.cpu().numpy() == -7).all() and (scratch.cpu().numpy() == 0xAB).all()
    # refusals: D2FE_ERR_INVALID, nothing is launched
    args = lambda **kw: api.detect_fast_device(fe, d_img.data_ptr(), kw.get("w", 160), 120, d_feat.data_ptr(), kw.get("T", 24), xy.data_ptr(), resp.data_ptr(), kw.get("cap", 16),
                                               n.data_ptr(), scratch.data_ptr() + kw.get("mis", 0), cols=kw.get("cols", 3), rows=kw.get("rows", 4), threshold=kw.get("thr", 10))
    for bad in (dict(T=0), dict(T=1025), dict(cols=0), dict(cols=9, rows=9), dict(thr=255), dict(cap=0), dict(mis=4), dict(w=20)):
        with pytest.raises(api.D2FEError) as e:
            args(**bad)
        assert e.value.code == -1, bad
    fe.close()


# ---- d2fe_lk_flow_step_device alone ----------------------------------------------------------------------------------------------------------------------------------
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


def _run_steps(api, fe, seq, kps, fp, kp_cap=64, id0=1000):
    """the chain of d2fe_lk_flow_step_device over `seq` on one stream; returns (per-frame list blocks on the host, per-frame copies of the scratch, next_id).  The
    blocks start as -77 fill with a zero header (the documented contract), the scratch as 0xAB; a synchronisation between frames only serves the scratch copies"""
    import torch
    dev = torch.device("cuda", 0)
    nfr = len(seq)
    h, w = seq[0].shape
    T = api.lk_flow_cap_tracks(fp)
    imgs = torch.from_numpy(np.stack(seq)).to(dev)
    k_h = np.zeros((nfr, kp_cap, 2), np.float32); n_h = np.zeros(nfr, np.int32)
    for f in range(nfr):
        if kps[f] is not None:
            n_h[f] = len(kps[f]); k_h[f, :n_h[f]] = kps[f]
    d_kps = torch.from_numpy(k_h).to(dev); d_nkp = torch.from_numpy(n_h).to(dev)
    lists = torch.full((nfr + 1, api.lk_flow_list_bytes(T) // 4), -77.0, device=dev)
    lists[0] = 0.0; lists[:, :64] = 0.0
    nbytes = api.lk_stereo_workspace_bytes(nfr, w, h, 2)
    ws = torch.full((nbytes,), 0xCD, dtype=torch.uint8, device=dev)
    total = nbytes // (2 * nfr)
    scratch = torch.full((api.lk_flow_scratch_bytes(w, h, T, fp.fast_cols, fp.fast_rows),), 0xAB, dtype=torch.uint8, device=dev)
    next_id = torch.full((1,), id0, dtype=torch.int32, device=dev)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    api.lk_track_stereo_device(fe, imgs.data_ptr(), imgs.data_ptr(), nfr, w, h, None, None, 0, ws.data_ptr(), None, None, stream=st.cuda_stream)
    scr = []
    for f in range(nfr):
        api.lk_flow_step_device(fe, ws.data_ptr() + max(f - 1, 0) * total, ws.data_ptr() + f * total, w, h, lists[f].data_ptr(), lists[f + 1].data_ptr(),
                                d_kps[f].data_ptr() if fp.superpoint else None, d_nkp[f:].data_ptr() if fp.superpoint else None, kp_cap if fp.superpoint else 0,
                                next_id.data_ptr(), scratch.data_ptr(), fp=fp, stream=st.cuda_stream)
        st.synchronize()
        scr.append(scratch.cpu().numpy().copy())
    return lists.cpu().numpy(), scr, int(next_id.cpu()[0])


def _same_lists(api, lists_h, comp, T, id0, where):
    nid = id0
    for f, c in enumerate(comp):
        v = api.lk_flow_list_views(lists_h[f + 1], T)
        n, m = c["n"], c["n_tracked_in"]
        nid += c["n_new"]
        got = {k: v[k] for k in ("n", "n_tracked_in", "n_lost", "n_removed_near", "n_new", "lack", "num", "n_cand", "next_id")}
        want = {k: c[k] for k in ("n", "n_tracked_in", "n_lost", "n_removed_near", "n_new", "lack", "num", "n_cand")}; want["next_id"] = nid
        assert got == want, (where, f, got, want)
        assert v["hdr"][5] == 0 and not v["hdr"][10:].any(), (where, f)
        assert np.array_equal(_bits(v["pts"][:n]), _bits(c["pts"])) and np.array_equal(v["src"][:n], c["src"]) and np.array_equal(v["id"][:n], c["id"] + id0), (where, f)
        assert np.array_equal(_bits(v["trk_xy"][:m]), _bits(c["trk_pts"])) and np.array_equal(v["trk_status"][:m], c["trk_status"]), (where, f)
        for k in ("pts", "id", "src"):
            assert not np.ascontiguousarray(v[k][n:]).view(np.uint8).any(), (where, f, k)
        assert not v["trk_xy"][m:].view(np.uint8).any() and not v["trk_status"][m:].any(), (where, f)
    return nid


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,total,superpoint,near", [(160, 120, 24, 1, 5.0), (160, 120, 150, 0, 5.0), (326, 243, 150, 1, 26.0), (326, 243, 24, 0, 5.0)])
def test_flow_step_alone_on_moving_frames(w, h, total, superpoint, near):
    """5 frames of the sliding scene: an empty first list without keypoints (x1) or with some (x2), tracks lost and (at a near_lk_thread_rate above feature_min_dist)
    thinned, detection whenever a quarter is missing"""
    api, fe = _fe()
    seq = [l[:h, :w].copy() for l, _ in sliding_stereo(5, 243, 326, 7105, 24, 3)]
    rng = np.random.RandomState(5)
    kps = [np.stack([rng.randint(4, w - 4, k), rng.randint(4, h - 4, k)], axis=1).astype(np.float32) if superpoint else None for k in (9, 30, 0, 17, 5)]
    fp = api.flow_params(total_feature_num=total, superpoint=superpoint, near_lk_thread_rate=near)
    lists_h, _, next_id = _run_steps(api, fe, seq, kps, fp)
    comp = ref.compose(seq, kps, *_trackers(api, fe), params=dict(total_feature_num=total, near_lk_thread_rate=near))
    print("moving", (w, h, total, superpoint), "n", [c["n"] for c in comp], "lost", [c["n_lost"] for c in comp], "near", [c["n_removed_near"] for c in comp],
          "num", [c["num"] for c in comp], "cand", [c["n_cand"] for c in comp], "new", [c["n_new"] for c in comp])
    assert comp[0]["n_tracked_in"] == 0 and comp[0]["num"] == ((total - 9) * 2 if superpoint else total) and comp[0]["n_new"] > 0
    assert any(c["n"] - c["n_new"] > 0 for c in comp[1:]) and all(c["n"] <= total for c in comp)
    assert near == 5.0 or sum(c["n_removed_near"] for c in comp) > 0
    assert _same_lists(api, lists_h, comp, total, 1000, (w, h, total, superpoint)) == next_id
    fe.close()


# the dot scenario on 160 x 120 (regions of 53 x 30; slot s of region (ri, rj) is the pixel (53 ri + 13 or 40, 30 rj + 9)), total_feature_num = 24.  One static
# image for every frame; what changes is the keypoints.  A and B are tracked dots; E = A + (16, 12) is exactly 20 px from A (kept by `<`), F = B + (15, 12) is nearer
# (dropped); K and K2 are keypoints of frame 1 alone, G = K + (16, 12) and H = K2 + (15, 12) the dots beside them.  Frame 0's keypoints sit on E, G and H, so these three
# stay out of the first list (F is kept out by B, which is brighter and accepted before it).
def _slot(ri, rj, s):
    return (53 * ri + (13 if s == 0 else 40), 30 * rj + 9)


def _dot_scenario(n_base):
    A, B, K, K2 = _slot(0, 0, 0), _slot(1, 1, 0), _slot(2, 2, 0), _slot(0, 3, 0)
    E, F, G, H = (A[0] + 16, A[1] + 12), (B[0] + 15, B[1] + 12), (K[0] + 16, K[1] + 12), (K2[0] + 15, K2[1] + 12)
    free = [_slot(ri, rj, s) for ri in range(3) for rj in range(4) for s in range(2) if (ri, rj) not in ((0, 0), (1, 1), (2, 2), (0, 3))]
    base = [A, B] + free[:n_base - 2]
    dots = [(x, y, 100 + 3 * k) for k, (x, y) in enumerate(base)] + [(E[0], E[1], 250), (F[0], F[1], 90), (G[0], G[1], 240), (H[0], H[1], 235)]
    img = ref.dot_image(120, 160, dots)
    kps = [np.float32([E, G, H]), np.float32([K, K2]), None, None, None]
    return img, kps, dict(A=A, B=B, E=E, F=F, G=G, H=H, K=K, K2=K2)


def _check_dot_scenario(comp, n_base, P):
    """what the scenario is built to do, on the composition"""
    has = lambda c, p: any(tuple(q) == tuple(np.float32(p)) for q in c["pts"])
    c0, c1, c2, c3, c4 = comp
    assert c0["num"] == 2 * (24 - 3) and c0["n"] == n_base and not any(has(c0, P[k]) for k in "EFGH")
    assert all(c["n_lost"] == 0 and c["n_removed_near"] == 0 for c in comp)                  # a static image: every entry comes back
    assert all(np.array_equal(c["trk_pts"], comp[t]["pts"]) for t, c in enumerate(comp[1:]))  # ... exactly where it was
    assert c1["lack"] == 24 - 2 - n_base and c1["num"] == 2 * c1["lack"] and c1["n_cand"] == min(c1["num"], n_base + 4)
    assert has(c1, P["E"]) and has(c1, P["G"]) and not has(c1, P["F"]) and not has(c1, P["H"]) and c1["n_new"] == 2      # exactly 20 px: kept; 19.2 px: dropped
    assert c2["n_new"] == 1 and has(c2, P["H"]) and not has(c2, P["F"])                       # K2 is gone, B is still there
    assert c3["lack"] == 24 - (n_base + 3) and c3["n_new"] == 0 and c4["n"] == n_base + 3
    if n_base == 14:
        assert c3["lack"] == 7 and c3["num"] == 14 and c3["n_cand"] == 14                     # one more than a quarter: detects, finds nothing new
    else:
        assert c3["lack"] == 6 and c3["num"] == 0 and c3["n_cand"] == 0                       # exactly a quarter: does not detect


@pytest.mark.gpu
@pytest.mark.parametrize("n_base", [14, 15])
def test_flow_step_on_the_dot_scenario(n_base):
    """lack exactly 7 (detects) and exactly 6 (does not) at total_feature_num = 24, distances of exactly 20 px against a keypoint and against a tracked entry, and a
    frame that does not detect: the detector's scratch stays as the frame before left it and the list is the tracked entries"""
    api, fe = _fe()
    img, kps, P = _dot_scenario(n_base)
    seq = [img] * 5
    fp = api.flow_params(total_feature_num=24)
    comp = ref.compose(seq, kps, *_trackers(api, fe), params=dict(total_feature_num=24))
    _check_dot_scenario(comp, n_base, P)
    lists_h, scr, next_id = _run_steps(api, fe, seq, kps, fp)
    assert _same_lists(api, lists_h, comp, 24, 1000, ("dots", n_base)) == next_id == 1000 + n_base + 3
    for f, c in enumerate(comp):
        if c["num"] == 0:
            assert f > 0 and np.array_equal(scr[f], scr[f - 1]), f
            v = api.lk_flow_list_views(lists_h[f + 1], 24)
            assert v["n"] == v["n_tracked_in"] and np.array_equal(_bits(v["pts"][:v["n"]]), _bits(v["trk_xy"][:v["n"]])) and np.array_equal(v["src"][:v["n"]], np.arange(v["n"]))
        else:
            assert not np.array_equal(scr[f], scr[f - 1] if f else np.full_like(scr[0], 0xAB)), f
    assert (n_base == 15) == any(c["num"] == 0 for c in comp)
    fe.close()


@pytest.mark.gpu
def test_flow_step_over_a_blank_frame():
    """a constant frame in the middle: every track is lost and nothing is found; the frame after it detects the whole list again, with new ids"""
    api, fe = _fe()
    img, _, _ = _dot_scenario(15)
    seq = [img, img, np.full_like(img, 50), img, img]
    kps = [None] * 5
    fp = api.flow_params(total_feature_num=24, superpoint=0)
    comp = ref.compose(seq, kps, *_trackers(api, fe), params=dict(total_feature_num=24))
    assert comp[1]["n"] == comp[0]["n"] == 18 and comp[2]["n_lost"] == 18 and comp[2]["n"] == 0 and comp[2]["num"] == 24 and comp[2]["n_cand"] == 0      # F is blocked by B
    assert comp[3]["n_tracked_in"] == 0 and comp[3]["n_new"] == 18 and comp[3]["id"].min() == 18 and comp[4]["n_new"] == 0
    lists_h, _, next_id = _run_steps(api, fe, seq, kps, fp, id0=5)
    assert _same_lists(api, lists_h, comp, 24, 5, "blank") == next_id == 5 + 36
    fe.close()


@pytest.mark.gpu
def test_flow_step_refusals():
    """D2FE_ERR_INVALID, nothing is launched"""
    import torch
    api, fe = _fe()
    dev = torch.device("cuda", 0)
    T = 24
    ws = torch.zeros((api.lk_stereo_workspace_bytes(1, 160, 120, 2),), dtype=torch.uint8, device=dev)
    lists = torch.zeros((2, api.lk_flow_list_bytes(T) // 4), device=dev)
    scratch = torch.zeros((api.lk_flow_scratch_bytes(160, 120, T),), dtype=torch.uint8, device=dev)
    next_id = torch.zeros((1,), dtype=torch.int32, device=dev)
    kp = torch.zeros((8, 2), device=dev); nk = torch.zeros((1,), dtype=torch.int32, device=dev)

    def call(fp, prev=0, cur=1, kps=kp.data_ptr(), kp_cap=8, mis=0, w=160):
        api.lk_flow_step_device(fe, ws.data_ptr(), ws.data_ptr(), w, 120, lists[prev].data_ptr(), lists[cur].data_ptr(), kps, nk.data_ptr(), kp_cap, next_id.data_ptr(),
                                scratch.data_ptr() + mis, fp=fp)
    bad_fp = [api.flow_params(total_feature_num=T, **kw) for kw in (dict(fast_cols=0), dict(fast_cols=9, fast_rows=9), dict(fast_threshold=255), dict(superpoint=2),
                                                                    dict(win=20), dict(levels=8), dict(iters=0), dict(near_lk_thread_rate=-1.0))]
    bad_fp += [api.flow_params(total_feature_num=1024), api.flow_params(total_feature_num=-1)]
    short = api.flow_params(total_feature_num=T); short.struct_size -= 4
    ok = api.flow_params(total_feature_num=T)
    for kw in [dict(fp=f) for f in bad_fp + [short]] + [dict(fp=ok, cur=0), dict(fp=ok, kps=None), dict(fp=ok, kp_cap=-1), dict(fp=ok, mis=4), dict(fp=ok, w=20)]:
        with pytest.raises(api.D2FEError) as e:
            call(**kw)
        assert e.value.code == -1, kw
    call(ok)        # and the call they all refused runs: an empty list on a black frame stays empty
    fe.sync()
    v = api.lk_flow_list_views(lists[1].cpu().numpy(), T)
    assert v["n"] == 0 and v["lack"] == T and v["num"] == T and v["n_cand"] == 0
    fe.close()


@pytest.mark.gpu
def test_the_launches_of_a_frame_are_the_number_the_header_states():
    """FIVE launches per frame under D2FE_PROF_LK whether the frame detects or not (the dot scenario has both), FOUR for the detector alone; the pyramids of the
    sequence are the two launches of the pyramids-only call"""
    import torch
    api, fe = _fe()
    img, kps, _ = _dot_scenario(15)
    fp = api.flow_params(total_feature_num=24)
    fe.profile_enable(2)
    lists_h, _, _ = _run_steps(api, fe, [img] * 5, kps, fp)
    ms, n = fe.profile_read()["lk"]
    nums = [api.lk_flow_list_views(lists_h[f + 1], 24)["num"] for f in range(5)]
    assert any(v == 0 for v in nums) and any(v > 0 for v in nums) and n == 2 + 5 * 5, (nums, n)
    fe.profile_enable(0); fe.profile_enable(2)
    _detect_dev(api, fe, img, 30, 24)
    assert fe.profile_read()["lk"][1] == 4
    fe.profile_enable(0); fe.profile_enable(2)
    _detect_dev(api, fe, img, 0, 24, cap=4)
    assert fe.profile_read()["lk"][1] == 4
    fe.profile_enable(0)
    fe.close()
