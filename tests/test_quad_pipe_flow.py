"""The quad pipe's flow_lk mode (d2fe_quad_flow_enable, include/d2fe.h): trackLocalFrames of the reference's quadcam tracker with enable_lk_optical_flow = 1,
sp_track_use_lk = 0 and SuperPoint beside it (d2featuretracker.cpp:121-133; config/quadcam/quadcam_single.yaml) -- four FAST-replenished flow lists per quad frame
with ONE id counter in camera order and the half-image LK track of every neighbour pair over the flow lists.  The two new entry points are held on their own
(d2fe_lk_flow_quad_step_device to four d2fe_lk_flow_step_device calls byte for byte, d2fe_lk_flow_neighbour_device to api.lk_track and to the carry form), the pipe to
the host composition of tests/helpers/quad_flow_ref.py on the cyclic panorama of tests/helpers/quad_lk_ref.py: 8 quad frames of four 200 x 120 views, undistort_fov
200 (move_cols exactly 90), seeded weights at threshold 0.15, cap 60."""
import struct
import subprocess

import numpy as np
import pytest

from tests.helpers import lk_carry_ref as ref
from tests.helpers import quad_flow_ref as qfref
from tests.helpers import quad_lk_ref as qref

H, W, CAP, NQ, SEED = qref.H, qref.W, 60, 8, 7106
FOV = qref.FOV
# SuperPoint leaves about 25 keypoints in a 200 x 120 view and feature_min_dist = 20 lets a view hold a few dozen points at most: with total_feature_num = 100 more
# than a quarter is always missing, so every quad frame detects and the keypoints decide which candidates get in
BASE = {"total_feature_num": 100, "feature_min_dist": 20.0}
T_PIPE = 100
COUNT_KEYS = ("n", "n_tracked_in", "n_lost", "n_removed_near", "n_new", "lack", "num", "n_cand")
FLOW_KEYS = tuple("flow_" + k for k in COUNT_KEYS) + ("flow_pts", "flow_id", "flow_src", "flow_nb_lk_xy", "flow_nb_lk_status")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _fe(max_batch=16, netvlad=False):
    from d2slam_amd import api, netvlad as nvm
    from tests.test_quad_pipe import _weights
    fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=CAP, input_width=W, input_height=H, max_batch=max_batch, keypoint_threshold=0.15, precision=api.PREC_F32_WINO))
    fe.load_superpoint(_weights())
    if netvlad:
        fe.load_netvlad(nvm.synthetic_netvlad_weights())
    return api, fe


@pytest.fixture(scope="module")
def quads():
    return qref.cyclic_quads(NQ, SEED)


def _pipe(api, fe, **kw):
    args = dict(lanes=1, quads=1, raw_width=W, raw_height=H, width=W, height=H, cap=CAP, radius_neighbour=0.2 * W, undistort_fov=FOV, netvlad=False,
                match_neighbour=False, match_prev=False, flow_lk=True, flow_params=dict(BASE))
    args.update(kw)
    return api.QuadPipe(fe, qref.identity_maps(), **args)


def _run(api, fe, frames, lanes=1, Q=1, **kw):
    """all quad frames through one pipe, Q per submit, `lanes` submits in flight; one dict of copies per QUAD FRAME"""
    pipe = _pipe(api, fe, lanes=lanes, quads=Q, **kw)
    nsub = len(frames) // Q
    tk, out = [], []
    take = lambda: out.append({k: (None if v is None else v.copy()) for k, v in pipe.wait(tk[len(out)]).items()})
    for i in range(nsub):
        tk.append(pipe.submit(frames[i * Q:(i + 1) * Q]))
        if len(tk) > lanes - 1:
            take()
    while len(out) < nsub:
        take()
    pipe.close()
    return [{k: (None if v is None else v[q]) for k, v in o.items()} for o in out for q in range(Q)]


def _trackers(api, fe):
    def track(a_img, b_img, pts):
        a, b = api.LKFrame(fe, a_img, 2), api.LKFrame(fe, b_img, 2)
        out = api.lk_track(fe, a, b, pts, pts, api.WHOLE_IMG_MATCH, 0.0)
        a.close(); b.close()
        return out

    def track_half(a_img, b_img, pts, init, typ, mc):
        a, b = api.LKFrame(fe, a_img, 2), api.LKFrame(fe, b_img, 2)
        out = api.lk_track(fe, a, b, pts, init, typ, mc)
        a.close(); b.close()
        return out

    def detect(img, num):
        f = api.LKFrame(fe, img, 0)
        out = api.detectFastByRegion(fe, f, num, 3, 4, 10)
        f.close()
        return out
    return track, track_half, detect


def _flow_list(api, T, pts, id0):
    """one host flow-list block with the given points: ids id0.., a zero header but for n"""
    blk = np.zeros(api.lk_flow_list_bytes(T) // 4, np.float32)
    v = api.lk_flow_list_views(blk, T)
    n = len(pts)
    v["hdr"][0] = n
    v["pts"][:n] = pts; v["id"][:n] = id0 + np.arange(n); v["src"][:n] = -1
    return blk


@pytest.mark.gpu
def test_quad_flow_step_is_four_single_steps():
    """Item 1.  d2fe_lk_flow_quad_step_device against four d2fe_lk_flow_step_device calls in camera order on the same inputs and the same next_id: the whole list
    blocks (headers, both tickets, every array) and next_id, byte for byte, over four consecutive steps that swap the same two sets of blocks -- so a ticket that a
    launch did not leave zero would show in the next but one.  326 x 243 images (no multiple of 8) moving by (-3, 0), total_feature_num = 150, synthetic lists: camera 0
    holds 150 entries, 139 on a grid and 11 twins 2 px from an earlier entry (removeNearPoints among more than 64 survivors) and never detects; cameras 1 and 2 hold
    41; camera 3 is empty (the first-frame path).  The keypoint counts steer the decisions: camera 2 of step 0 is a little more than a quarter short (a small `num`
    under a large FAST pool: the histogram selection), camera 3 of step 1 has 128 keypoints and does not detect, every camera of step 3 has 120 or more and none
    detects.  Every condition is read from the single-step results."""
    import torch
    api, fe = _fe(max_batch=1)
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    w, h, T, KC, NS = 326, 243, 150, 128, 4
    rng = np.random.RandomState(5)
    seqs = [[f[0] for f in ref.sliding_stereo(NS + 1, h, w, 7300 + c, 0, 3)] for c in range(4)]                  # [camera][time]
    imgs = torch.from_numpy(np.stack([np.stack([seqs[c][t] for c in range(4)]) for t in range(NS + 1)])).to(dev)      # [time][camera][h][w]
    gx, gy = np.meshgrid(np.arange(20, w - 12, 16), np.arange(16, h - 12, 16))
    grid = np.stack([gx.ravel(), gy.ravel()], 1).astype(np.float32)
    grid = grid[rng.permutation(len(grid))]
    p0 = np.concatenate([grid[:139], grid[10:21] + np.float32([2.0, 1.0])])
    host = [_flow_list(api, T, p0, 5000), _flow_list(api, T, grid[139:180], 6000), _flow_list(api, T, grid[180:221], 7000), _flow_list(api, T, grid[:0], 0)]
    lw = len(host[0])
    fp = api.flow_params()
    assert fp.track.total_feature_num == 150 and fp.superpoint == 1 and api.lk_flow_list_bytes(T) == 4 * lw and len(p0) == T
    total = api.lk_stereo_workspace_bytes(4, w, h, 2) // 8
    ws = [torch.full((8 * total,), 0xAB, dtype=torch.uint8, device=dev) for _ in range(NS)]
    sb = api.lk_flow_scratch_bytes(w, h, T)
    assert sb % 16 == 0
    # keypoints per step: dense [4][KC] rows
    nk = np.array([[40, 30, 67, 20], [30, 0, 50, KC], [20, 25, 30, 10], [120, 128, 125, 122]], np.int32)
    k_h = np.stack([rng.randint(4, w - 4, (NS, 4, KC)), rng.randint(4, h - 4, (NS, 4, KC))], -1).astype(np.float32)
    kps = torch.from_numpy(k_h).to(dev); cnt = torch.from_numpy(nk).to(dev)

    def blocks():
        a = torch.from_numpy(np.stack(host)).to(dev)
        b = torch.full((4, lw), -77.0, device=dev); b[:, :64] = 0.0           # the documented contract: a zero header before the first use as a current list
        return [a, b], torch.full((1,), 1000, dtype=torch.int32, device=dev), torch.full((4, sb), 0xAB, dtype=torch.uint8, device=dev)
    quad, qid, qscr = blocks()
    single, sid, sscr = blocks()
    torch.cuda.synchronize()
    for s in range(NS):
        api.lk_track_stereo_device(fe, imgs[s].data_ptr(), imgs[s + 1].data_ptr(), 4, w, h, None, None, 0, ws[s].data_ptr(), None, None, stream=st.cuda_stream)
    st.synchronize()

    def quad_step(s, lists, nid, scr, fp_=fp):
        prev, cur = s % 2, (s + 1) % 2
        api.lk_flow_quad_step_device(fe, ws[s].data_ptr(), ws[s].data_ptr() + 4 * total, total, w, h, lists[prev].data_ptr(), lists[cur].data_ptr(), lw, kps[s].data_ptr(),
                                     cnt[s].data_ptr(), KC, nid.data_ptr(), scr.data_ptr(), sb, fp=fp_, stream=st.cuda_stream)

    def single_steps(s, lists, nid, scr, fp_=fp):
        prev, cur = s % 2, (s + 1) % 2
        for c in range(4):
            api.lk_flow_step_device(fe, ws[s].data_ptr() + c * total, ws[s].data_ptr() + (4 + c) * total, w, h, lists[prev][c].data_ptr(), lists[cur][c].data_ptr(),
                                    kps[s, c].data_ptr(), cnt[s, c:].data_ptr(), KC, nid.data_ptr(), scr[c].data_ptr(), fp=fp_, stream=st.cuda_stream)

    def same_blocks(q_h, s_h, where):
        hd = [api.lk_flow_list_views(s_h[c], T) for c in range(4)]
        for c in range(4):
            vq = api.lk_flow_list_views(q_h[c], T)
            for key in ("hdr", "id", "pts", "src", "trk_xy", "trk_status"):
                assert np.array_equal(_bytes(vq[key]), _bytes(hd[c][key])), (where, c, key)
            assert np.array_equal(_bytes(q_h[c]), _bytes(s_h[c])), (where, c)
            assert vq["hdr"][5] == 0 and not vq["hdr"][10:].any(), (where, c)          # both tickets are left zero
        return hd

    pool_count = lambda scr_h, c: int(scr_h[c, sb - 16:sb - 12].view(np.int32)[0])    # the candidate count: the last 16 bytes of a camera's scratch
    headers, launches, over = [], [], []
    for s in range(NS):
        cur = (s + 1) % 2
        fe.profile_enable(0); fe.profile_enable(2)
        quad_step(s, quad, qid, qscr)
        st.synchronize()
        launches.append(fe.profile_read()["lk"][1])
        fe.profile_enable(0)
        single_steps(s, single, sid, sscr)
        st.synchronize()
        hd = same_blocks(quad[cur].cpu().numpy(), single[cur].cpu().numpy(), s)
        headers.append(hd)
        print("step", s, "n", [v["n"] for v in hd], "lost", [v["n_lost"] for v in hd], "near", [v["n_removed_near"] for v in hd], "num", [v["num"] for v in hd],
              "cand", [v["n_cand"] for v in hd], "new", [v["n_new"] for v in hd], "next_id", [v["next_id"] for v in hd])
        nid = 1000 + sum(v["n_new"] for hh in headers for v in hh)
        assert int(qid.cpu()[0]) == int(sid.cpu()[0]) == nid
        # header word 6 is next_id after that camera, whether the camera added anything or not
        run = 1000 + sum(v["n_new"] for hh in headers[:-1] for v in hh)
        for c in range(4):
            run += hd[c]["n_new"]
            assert hd[c]["next_id"] == run, (s, c)
        q_s, s_s = qscr.cpu().numpy(), sscr.cpu().numpy()
        for c in range(4):
            if hd[c]["num"] > 0:          # every camera has a pool and a count of its own: what its single step counts
                assert pool_count(q_s, c) == pool_count(s_s, c), (s, c)
                over.append(pool_count(s_s, c) > hd[c]["num"])
                print("  camera", c, "pool", pool_count(s_s, c), "num", hd[c]["num"])
    # ---- the conditions on the inputs, read from the single-step results
    assert launches == [5] * NS, launches                        # five launches whether the quad frame detects or not
    h0 = headers[0]
    assert h0[0]["n_tracked_in"] == 150 and h0[0]["n_tracked_in"] - h0[0]["n_lost"] > 64 and h0[0]["n_removed_near"] > 0
    assert h0[1]["n_tracked_in"] == 41 and h0[2]["n_tracked_in"] == 41 and h0[3]["n_tracked_in"] == 0 and h0[3]["num"] == 2 * (150 - 20)
    assert any(any(v["num"] == 0 for v in hh) and any(v["num"] > 0 for v in hh) for hh in headers)
    assert h0[0]["num"] == 0 and sum(v["n_new"] > 0 for v in h0) >= 3
    assert headers[1][3]["n_tracked_in"] > 0 and headers[1][3]["num"] == 0
    assert any(over)                                              # a FAST pool larger than `num`: the histogram selection ran
    h3 = headers[3]
    assert all(v["num"] == 0 and v["n_new"] == 0 for v in h3) and any(v["num"] > 0 for v in headers[2])
    assert all(v["next_id"] == headers[2][3]["next_id"] == int(qid.cpu()[0]) for v in h3)          # nothing detected: next_id unchanged, word 6 equals it everywhere
    # ---- superpoint = 0: the keypoints are ignored (n_kp = 0), the same bytes as four single steps
    fp0 = api.flow_params(superpoint=0)
    q0, q0id, q0scr = blocks()
    s0, s0id, s0scr = blocks()
    torch.cuda.synchronize()
    quad_step(0, q0, q0id, q0scr, fp0); single_steps(0, s0, s0id, s0scr, fp0)
    st.synchronize()
    hd0 = same_blocks(q0[1].cpu().numpy(), s0[1].cpu().numpy(), "superpoint=0")
    assert int(q0id.cpu()[0]) == int(s0id.cpu()[0]) == 1000 + sum(v["n_new"] for v in hd0)
    assert all(v["lack"] == 150 - (v["n"] - v["n_new"]) for v in hd0) and hd0[3]["num"] == 150 and hd0[2]["num"] != h0[2]["num"]
    # ---- refusals: D2FE_ERR_INVALID, nothing is launched, nothing is written
    before = (quad[0].cpu().numpy().copy(), quad[1].cpu().numpy().copy(), int(qid.cpu()[0]))
    args = [fe, ws[0].data_ptr(), ws[0].data_ptr() + 4 * total, total, w, h, quad[0].data_ptr(), quad[1].data_ptr(), lw, kps[0].data_ptr(), cnt[0].data_ptr(), KC,
            qid.data_ptr(), qscr.data_ptr(), sb]
    fe.profile_enable(2)
    for bad in ({"total_feature_num": 1024}, {"win": 20}, {"levels": 8}, {"fast_cols": 0}, {"fast_threshold": 255}, {"superpoint": 2}):
        with pytest.raises(api.D2FEError) as e:
            api.lk_flow_quad_step_device(*args, fp=api.flow_params(**bad), stream=st.cuda_stream)
        assert e.value.code == -1, bad
    # pyr_stride, list_stride, scratch_stride too small; scratch_stride and scratch misaligned; current lists overlapping the previous ones; no keypoints with kp_cap > 0
    for swap in ({3: total - 1}, {8: lw - 64}, {14: sb - 16}, {14: sb + 8}, {13: qscr.data_ptr() + 4}, {7: quad[0][1].data_ptr()}, {9: None}, {11: -1}):
        a = list(args)
        for i, v in swap.items():
            a[i] = v
        with pytest.raises(api.D2FEError) as e:
            api.lk_flow_quad_step_device(*a, fp=fp, stream=st.cuda_stream)
        assert e.value.code == -1, swap
    st.synchronize()
    assert fe.profile_read()["lk"][1] == 0
    fe.profile_enable(0)
    assert np.array_equal(_bytes(quad[0].cpu().numpy()), _bytes(before[0])) and np.array_equal(_bytes(quad[1].cpu().numpy()), _bytes(before[1])) and int(qid.cpu()[0]) == before[2]
    fe.close()


@pytest.mark.gpu
def test_flow_neighbour_launch_is_lk_track_and_the_carry_form(quads):
    """Item 2.  d2fe_lk_flow_neighbour_device over two quad frames of synthetic flow lists (41 slots: a full list, an empty one, points exactly on both gate bounds
    x = 110 and x = 90) against api.lk_track with types 1 and 2 on the gate-eligible subset, scattered back, and against d2fe_lk_carry_neighbour_device on carry
    lists holding the same points: bit for bit, every other slot zero"""
    import torch
    from tests.test_quad_pipe_sp_lk import _synthetic_list
    api, fe = _fe(max_batch=1)
    dev = torch.device("cuda", 0)
    Q, T, D = 2, 41, 8
    rng = np.random.RandomState(9)
    tp_flow, tp_carry = api.track_params(total_feature_num=T), api.track_params(total_feature_num=T - 1)          # 41 slots in both layouts
    lw, clw = api.lk_flow_list_bytes(T) // 4, api.lk_carry_list_bytes(T, D) // 4
    imgs = torch.from_numpy(quads[:Q].reshape(Q * 4, H, W).copy()).to(dev)
    total = api.lk_stereo_workspace_bytes(1, W, H, 2) // 2
    ws = torch.full((Q * 4 * total,), 0xAB, dtype=torch.uint8, device=dev)
    ns = [41, 30, 0, 25, 33, 41, 17, 1]
    lists, clists = [], []
    for i, n in enumerate(ns):
        pts = np.stack([rng.uniform(2, W - 2, n), rng.uniform(2, H - 2, n)], 1).astype(np.float32)
        pts[:4, 0] = [110.0, np.nextafter(np.float32(110.0), np.float32(0)), 90.0, np.nextafter(np.float32(90.0), np.float32(0))][:min(n, 4)]
        pts[4:n:3] = np.rint(pts[4:n:3])
        lists.append(_flow_list(api, T, pts, 100 * i))
        clists.append(_synthetic_list(api, rng, T, D, pts, 100 * i))
    d_lists = torch.from_numpy(np.stack(lists)).to(dev); d_clists = torch.from_numpy(np.stack(clists)).to(dev)
    xy = torch.full((Q, 4, T, 2), -5.0, device=dev); stt = torch.full((Q, 4, T), 9, dtype=torch.uint8, device=dev)
    cxy = torch.full((Q, 4, T, 2), -6.0, device=dev); cst = torch.full((Q, 4, T), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    api.lk_track_stereo_device(fe, imgs.data_ptr(), imgs[Q * 2:].data_ptr(), Q * 2, W, H, None, None, 0, ws.data_ptr(), None, None)
    fe.profile_enable(2)
    api.lk_flow_neighbour_device(fe, ws.data_ptr(), total, Q, W, H, FOV, d_lists.data_ptr(), lw, xy.data_ptr(), stt.data_ptr(), tp=tp_flow)
    fe.sync()
    assert fe.profile_read()["lk"][1] == 1          # ONE launch
    fe.profile_enable(0)
    api.lk_carry_neighbour(fe, ws.data_ptr(), total, Q, W, H, FOV, d_clists.data_ptr(), clw, cxy.data_ptr(), cst.data_ptr(), tp=tp_carry, desc_dim=D)
    fe.sync(); torch.cuda.synchronize()
    xy_h, st_h = xy.cpu().numpy(), stt.cpu().numpy()
    assert np.array_equal(_bits(xy_h), _bits(cxy.cpu().numpy())) and np.array_equal(st_h, cst.cpu().numpy())
    _, track_half, _ = _trackers(api, fe)
    mc = fe.half_move_cols(W, FOV)
    assert mc == 90.0
    kept = 0
    for q in range(Q):
        for p, (a, b, typ) in enumerate(qref.NEIGHBOURS):
            n = ns[q * 4 + a]
            pts = api.lk_flow_list_views(lists[q * 4 + a], T)["pts"][:n]
            ok, init = qref.half_gate(pts, typ, W, FOV)
            exp_xy = np.zeros((T, 2), np.float32); exp_st = np.zeros(T, np.uint8)
            if ok.any():
                exp_xy[:n][ok], exp_st[:n][ok] = track_half(quads[q, a], quads[q, b], pts[ok], init, typ, mc)
            if n >= 4:
                assert list(ok[:4]) == ([False, True, True, True] if typ == 1 else [True, True, True, False])
            assert np.array_equal(_bits(xy_h[q, p]), _bits(exp_xy)) and np.array_equal(st_h[q, p], exp_st), (q, p)          # zeros for ineligible entries and beyond n
            kept += int(exp_st.sum())
    assert kept > 0           # the scene is the same panorama 90 px further on: some of the random points track
    with pytest.raises(api.D2FEError) as e:
        api.lk_flow_neighbour_device(fe, ws.data_ptr(), total, Q, W, H, FOV, d_lists.data_ptr(), lw, xy.data_ptr(), stt.data_ptr(), tp=api.track_params(total_feature_num=1024))
    assert e.value.code == -1
    for kw in (dict(pyr_stride=total - 1), dict(list_stride=lw - 64), dict(fov=0.0)):
        with pytest.raises(api.D2FEError) as e:
            api.lk_flow_neighbour_device(fe, ws.data_ptr(), kw.get("pyr_stride", total), Q, W, H, kw.get("fov", FOV), d_lists.data_ptr(), kw.get("list_stride", lw),
                                         xy.data_ptr(), stt.data_ptr(), tp=tp_flow)
        assert e.value.code == -1
    with pytest.raises(api.D2FEError) as e:          # the carry form keeps refusing lists without descriptors
        api.lk_carry_neighbour(fe, ws.data_ptr(), total, Q, W, H, FOV, d_lists.data_ptr(), lw, xy.data_ptr(), stt.data_ptr(), tp=tp_flow, desc_dim=0)
    assert e.value.code == -1
    fe.close()


def _compose(api, fe, frames, res, prm, with_kps=True):
    """the host composition on the pipe's own keypoints; views from the existing undistort call on the same raw frames"""
    maps = qref.identity_maps()
    views = [[fe.undistort(frames[t, c], maps[c][0], maps[c][1], None) for c in range(4)] for t in range(len(frames))]
    kps = [[r["kps_xy"][c, :r["n_kp"][c]] if with_kps else None for c in range(4)] for r in res]
    track, track_half, detect = _trackers(api, fe)
    return views, qfref.compose_quad_flow(views, kps, track, track_half, detect, prm)


def _same_quad(r, row, nb, T, where):
    """one quad frame of the pipe (r) against the composition: every list array, header count and id, the neighbour tracks, bit for bit, zeros behind the end"""
    for c in range(4):
        k = row[c]
        n = k["n"]
        for key in COUNT_KEYS:
            assert int(r["flow_" + key][c]) == k[key], (where, c, key)
        assert np.array_equal(_bits(r["flow_pts"][c, :n]), _bits(k["pts"])), (where, c)
        assert np.array_equal(r["flow_id"][c, :n], k["id"]) and np.array_equal(r["flow_src"][c, :n], k["src"]), (where, c)
        for key in ("pts", "id", "src"):
            assert not _bytes(r["flow_" + key][c, n:]).any(), (where, c, key)
    assert r["flow_nb_lk_xy"].shape == (4, T, 2) and r["flow_nb_lk_status"].shape == (4, T) and r["flow_nb_lk_status"].dtype == np.uint8
    for p, (a, b, typ) in enumerate(qref.NEIGHBOURS):
        n = row[a]["n"]
        assert np.array_equal(_bits(r["flow_nb_lk_xy"][p, :n]), _bits(nb[p]["pts"])) and np.array_equal(r["flow_nb_lk_status"][p, :n], nb[p]["status"]), (where, p)
        assert not _bytes(r["flow_nb_lk_xy"][p, n:]).any() and not r["flow_nb_lk_status"][p, n:].any(), (where, p)


@pytest.mark.gpu
def test_quad_flow_pipe_is_the_host_composition(quads):
    """Item 3.  Per quad frame and view the pipe's flow lists, header counts, ids and neighbour tracks equal the host composition on the pipe's OWN keypoints bit for
    bit: api.LKFrame + api.lk_track + api.detectFastByRegion + flow_lk_ref.compose per camera with one id counter in camera order, api.lk_track with the half-image
    types per pair.  What the parameters are chosen to exercise is asserted on the composition: detection runs in several quad frames after the first, the keypoints
    block candidates (the composition without them holds other points), tracks are lost, neighbour tracks succeed.  The same bits for (lanes, quads) = (1, 1), (2, 1),
    (2, 2), (4, 1), and with match_neighbour and match_prev on every key of d2fe_quad_pipe_result is the plain pipe's."""
    api, fe = _fe(netvlad=True)
    prm = dict(BASE)
    base = _run(api, fe, quads)
    views, (comp, nbs) = _compose(api, fe, quads, base, prm)
    for t in range(NQ):
        assert all(np.array_equal(views[t][c], quads[t, c]) for c in range(4))          # identity maps: a raw frame is its own view
    flat = [k for row in comp for k in row]
    print("n", [[k["n"] for k in row] for row in comp], "lost", [[k["n_lost"] for k in row] for row in comp], "num", [[k["num"] for k in row] for row in comp],
          "cand", [[k["n_cand"] for k in row] for row in comp], "new", [[k["n_new"] for k in row] for row in comp])
    print("n_kp", [list(r["n_kp"]) for r in base], "nb kept", [[int(p["status"].sum()) for p in row] for row in nbs])
    assert all(0 < k["n"] <= T_PIPE for k in flat) and all(int(r["n_kp"].min()) > 0 for r in base)
    assert sum(any(k["num"] > 0 and k["n_cand"] > 0 for k in row) for row in comp[1:]) >= 3          # detection runs in several quad frames after the first
    assert any(k["n_lost"] > 0 for k in flat)                                                        # tracks are lost
    assert all(any(int(p["status"].sum()) > 0 for p in row) for row in nbs)                          # neighbour tracks succeed in every quad frame
    _, (bare, _) = _compose(api, fe, quads[:1], base[:1], prm, with_kps=False)
    assert any(not np.array_equal(bare[0][c]["pts"], comp[0][c]["pts"]) for c in range(4))          # the keypoints block candidates
    ids = qref.quad_ids_naive([[k["src"] for k in row] for row in comp])
    for t in range(NQ):
        _same_quad(base[t], comp[t], nbs[t], T_PIPE, t)
        for c in range(4):
            assert list(base[t]["flow_id"][c, :comp[t][c]["n"]]) == ids[t][c]
    # ---- the shape of the pipe does not matter; the keypoint-based results beside the mode are the plain pipe's
    on = dict(match_neighbour=True, match_prev=True, netvlad=True)
    plain = _run(api, fe, quads, lanes=2, Q=2, flow_lk=False, flow_params=None, **on)
    assert "flow_n" not in plain[0]
    for lanes, Q, kw in ((2, 1, {}), (2, 2, on), (4, 1, {})):
        got = _run(api, fe, quads, lanes=lanes, Q=Q, **kw)
        assert len(got) == NQ
        for t, (g, b) in enumerate(zip(got, base)):
            assert np.array_equal(g["n_kp"], b["n_kp"])
            for k in FLOW_KEYS:
                assert np.array_equal(_bytes(g[k]), _bytes(b[k])), (lanes, Q, t, k)
            for c in range(4):          # keypoint rows behind n_kp are not part of a result (tests/test_quad_pipe.py compares the same way)
                n = int(b["n_kp"][c])
                for k in ("kps_xy", "scores", "desc"):
                    assert np.array_equal(_bytes(g[k][c, :n]), _bytes(b[k][c, :n])), (lanes, Q, t, c, k)
            if kw:
                pl = plain[t]
                assert sorted(k for k in g if not k.startswith("flow_")) == sorted(pl)
                assert np.array_equal(g["n_kp"], pl["n_kp"]) and np.array_equal(_bytes(g["netvlad"]), _bytes(pl["netvlad"]))
                for c in range(4):
                    n = int(pl["n_kp"][c])
                    for k in ("kps_xy", "scores", "desc"):
                        assert np.array_equal(_bytes(g[k][c, :n]), _bytes(pl[k][c, :n])), (t, c, k)
                for pre in ("nb", "prev"):
                    assert np.array_equal(g[pre + "_n"], pl[pre + "_n"])
                    for p in range(4):
                        m = int(g[pre + "_n"][p])
                        for k in ("_q", "_t", "_dist"):
                            assert np.array_equal(_bytes(g[pre + k][p, :m]), _bytes(pl[pre + k][p, :m])), (t, pre + k)
        if kw:
            assert sum(int(g["nb_n"].sum()) for g in got) > 0 and sum(int(g["prev_n"].sum()) for g in got) > 0
    fe.close()


@pytest.mark.gpu
def test_quad_flow_contract(quads):
    """Item 4.  The refusals, each D2FE_ERR_INVALID and none of which ends the pipe: the pipe takes the mode afterwards.  D2FE_ERR_UNSUPPORTED without the mode,
    D2FE_ERR_NOT_READY before the wait"""
    api, fe = _fe(max_batch=4)
    fr = quads[0][None]
    pipe = _pipe(api, fe, flow_lk=False, flow_params=None)
    with pytest.raises(api.D2FEError) as e:
        pipe.flow_result_raw(0)
    assert e.value.code == -5                         # D2FE_ERR_UNSUPPORTED
    for bad in ({"levels": 3}, {"superpoint": 0}, {"total_feature_num": 1024}, {"fast_cols": 0}):
        with pytest.raises(api.D2FEError) as e:
            pipe.flow_enable(dict(BASE, **bad))
        assert e.value.code == -1, bad
        if "superpoint" in bad:
            assert "max_superpoint_cnt" in str(e.value)
    pipe.flow_enable(dict(BASE))                      # ... and the pipe still takes the mode
    with pytest.raises(api.D2FEError) as e:
        pipe.flow_enable(dict(BASE))
    assert e.value.code == -1 and "already" in str(e.value)          # accepted once
    with pytest.raises(api.D2FEError) as e:
        pipe.track_enable(None)
    assert e.value.code == -1 and "one of the two branches" in str(e.value)          # sp_lk after flow
    t = pipe.submit(fr)
    with pytest.raises(api.D2FEError) as e:
        pipe.flow_result_raw(t)
    assert e.value.code == -3                         # D2FE_ERR_NOT_READY: not waited for yet
    with pytest.raises(api.D2FEError) as e:
        pipe.track_result_raw(t)
    assert e.value.code == -5
    o = pipe.wait(t)
    assert o["flow_pts"].shape == (1, 4, T_PIPE, 2) and o["flow_nb_lk_status"].shape == (1, 4, T_PIPE) and o["nb_n"] is None and "track_n" not in o
    assert (o["flow_n"] == o["flow_n_new"]).all() and int(o["flow_n"].min()) > 0 and int(o["flow_n_tracked_in"].sum()) == 0
    assert np.array_equal(o["flow_id"][0, 0, :o["flow_n"][0, 0]], np.arange(o["flow_n"][0, 0]))          # the pipe's counter starts at 0, camera 0 first
    r = pipe.flow_result_raw(t)
    assert (r.quads, r.cap_tracks, r.list_words * 4) == (1, T_PIPE, api.lk_flow_list_bytes(T_PIPE))
    with pytest.raises(api.D2FEError) as e:
        pipe.flow_result_raw(t + 1)
    assert e.value.code == -1                         # unknown ticket
    o = {k: (None if v is None else v.copy()) for k, v in o.items()}
    with pytest.raises(api.D2FEError) as e:
        pipe.flow_enable(dict(BASE))
    assert e.value.code == -1                         # after a submit: and the pipe goes on
    o2 = pipe.wait(pipe.submit(quads[1][None]))
    assert np.array_equal(o2["flow_n_tracked_in"], o["flow_n"])
    pipe.close()
    other = _pipe(api, fe, flow_lk=False, flow_params=None)          # never enabled, refused after its first submit: still a plain pipe
    other.wait(other.submit(fr))
    with pytest.raises(api.D2FEError) as e:
        other.flow_enable(None)
    assert e.value.code == -1 and "first submit" in str(e.value)
    assert "flow_n" not in other.wait(other.submit(quads[1][None]))
    other.close()
    both = _pipe(api, fe, flow_lk=False, flow_params=None, sp_lk=True, track_params={"total_feature_num": 40})          # flow after sp_lk
    with pytest.raises(api.D2FEError) as e:
        both.flow_enable(dict(BASE))
    assert e.value.code == -1 and "one of the two branches" in str(e.value)
    assert "track_n" in both.wait(both.submit(fr))
    both.close()
    with pytest.raises(api.D2FEError) as e:           # through the constructor; no pipe is left alive
        _pipe(api, fe, sp_lk=True)
    assert e.value.code == -1
    dflt = _pipe(api, fe, flow_params=None)           # the reference's defaults: 150 slots
    o = dflt.wait(dflt.submit(fr))
    assert o["flow_pts"].shape == (1, 4, 150, 2)
    dflt.close(); fe.close()


@pytest.mark.gpu
def test_quad_flow_through_the_cpp_mirror(tmp_path, quads):
    """Item 5.  tests/cpp/quad_flow_test.cpp (g++, only libd2fe_hip.so; D2FrontEnd::QuadPipe::flowEnable and flow of include/d2fe.hpp, 2 lanes x 2 quad frames per
    submit, the keypoint-based neighbour matches on) writes every flow list and neighbour track; they equal the Python binding's one-lane pipe"""
    from d2slam_amd.weights import save_superpoint_d2fw
    from tests.test_quad_pipe import _weights
    from tests.test_quad_pipe_flow_cpu import build_cpp
    exe = build_cpp(tmp_path)
    sp, fin, fout = (str(tmp_path / n) for n in ("sp.d2fw", "in.bin", "out.bin"))
    save_superpoint_d2fw(sp, _weights())
    maps = qref.identity_maps()
    T = T_PIPE
    with open(fin, "wb") as f:
        f.write(struct.pack("<6i", NQ, H, W, CAP, BASE["total_feature_num"], 0))
        f.write(struct.pack("<d", BASE["feature_min_dist"]))
        for mm in maps:
            for m in mm[:2]:
                f.write(np.ascontiguousarray(m, np.float32).tobytes())
        f.write(quads.tobytes())
    res = subprocess.run([exe, sp, fin, fout, "2", "2"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "quad_flow_test OK" in res.stdout
    data, pos = open(fout, "rb").read(), 0

    def take(dt, shape):
        nonlocal pos
        n = int(np.prod(shape))
        a = np.frombuffer(data, dt, n, pos).reshape(shape).copy(); pos += n * np.dtype(dt).itemsize
        return a
    api, fe = _fe(max_batch=4)
    base = _run(api, fe, quads, match_neighbour=True)
    for t in range(NQ):
        b = base[t]
        n = take("<i4", 4); n_new = take("<i4", 4); num = take("<i4", 4); n_cand = take("<i4", 4)
        assert np.array_equal(n, b["flow_n"]) and np.array_equal(n_new, b["flow_n_new"]) and np.array_equal(num, b["flow_num"]) and np.array_equal(n_cand, b["flow_n_cand"])
        pts = take("<f4", (4, T, 2)); ids = take("<i4", (4, T)); src = take("<i4", (4, T))
        assert np.array_equal(_bits(pts), _bits(b["flow_pts"])) and np.array_equal(ids, b["flow_id"]) and np.array_equal(src, b["flow_src"])
        nbxy = take("<f4", (4, T, 2)); nbst = take("u1", (4, T))
        assert np.array_equal(_bits(nbxy), _bits(b["flow_nb_lk_xy"])) and np.array_equal(nbst, b["flow_nb_lk_status"])
        assert np.array_equal(take("<i4", 4), b["nb_n"])
    assert pos == len(data)
    fe.close()
