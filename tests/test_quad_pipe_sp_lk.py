"""The quad pipe's sp_lk mode (d2fe_quad_track_enable, include/d2fe.h): trackLocalFrames of the reference's quadcam tracker with enable_lk_optical_flow = 1 and
sp_track_use_lk = 1 (d2featuretracker.cpp:121-133) -- four LK-carried landmark lists per quad frame with ONE id counter in camera order, the half-image LK track of
every neighbour pair over the lists, and the neighbour matchKNN of the lists.  The two new launches are held on their own (d2fe_lk_carry_quad_step_device to four
d2fe_lk_carry_step_device calls, d2fe_lk_carry_neighbour_device to api.lk_track), the pipe to a host composition on the cyclic panorama of
tests/helpers/quad_lk_ref.py: 8 quad frames of four 200 x 120 views, undistort_fov 200 (move_cols exactly 90), seeded weights at threshold 0.15, cap 60."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.helpers import lk_carry_ref as ref
from tests.helpers import quad_lk_ref as qref

H, W, CAP, NQ, SEED = qref.H, qref.W, 60, 8, 7106
FOV = qref.FOV
# SuperPoint leaves about 25 keypoints in a 200 x 120 view: feature_min_dist = 3 lets the lists fill up to total_feature_num + 1 within the 8 quad frames
BASE = {"total_feature_num": 40, "feature_min_dist": 3.0}
LIST_KEYS = ("track_n", "track_n_tracked_in", "track_n_lost", "track_n_removed_near", "track_n_new", "track_pts", "track_id", "track_src", "track_kp", "track_desc",
             "track_scores")
TRACK_KEYS = LIST_KEYS + ("track_nb_lk_xy", "track_nb_lk_status", "track_lnb_n")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _fe(prec="wino", max_batch=16, netvlad=False):
    from d2slam_amd import api, netvlad as nvm
    from tests.test_quad_pipe import _weights
    fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=CAP, input_width=W, input_height=H, max_batch=max_batch, keypoint_threshold=0.15,
                                           precision={"wino": api.PREC_F32_WINO, "f32": api.PREC_F32}[prec]))
    fe.load_superpoint(_weights())
    if netvlad:
        fe.load_netvlad(nvm.synthetic_netvlad_weights())
    return api, fe


@pytest.fixture(scope="module")
def quads():
    return qref.cyclic_quads(NQ, SEED)


def _pipe(api, fe, **kw):
    args = dict(lanes=1, quads=1, raw_width=W, raw_height=H, width=W, height=H, cap=CAP, radius_neighbour=0.2 * W, undistort_fov=FOV, netvlad=False,
                match_neighbour=False, match_prev=False, sp_lk=True, track_params=dict(BASE))
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
    return track, track_half


def _list_matches(api, fe, torch, row, T, D, ratio=0.8):
    """the neighbour matchKNN of one quad frame's four lists through the existing device calls on dense copies: compaction, matcher, remap"""
    dev = torch.device("cuda", 0)
    pts = np.zeros((4, T, 2), np.float32); desc = np.zeros((4, T, D), np.float32); n = np.zeros(4, np.int32)
    for c in range(4):
        k = row[c]["n"]
        pts[c, :k] = row[c]["pts"]; desc[c, :k] = row[c]["desc"]; n[c] = k
    mc = fe.half_move_cols(W, FOV)
    job_row, job_left, job_shift = [], [], []
    for (a, b, typ) in qref.NEIGHBOURS:
        job_row += [a, b]; job_left += [1 if typ == 1 else 0, 1 if typ == 2 else 0]; job_shift += [mc if typ == 1 else -mc, 0.0]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_desc, d_pts, d_n = t(desc), t(pts), t(n)
    d_jr, d_jl, d_js = t(np.array(job_row, np.int32)), t(np.array(job_left, np.int32)), t(np.array(job_shift, np.float32))
    od = torch.zeros((8, T, D), device=dev); op = torch.zeros((8, T, 2), device=dev)
    om = torch.zeros((8, T), dtype=torch.int32, device=dev); on = torch.zeros(8, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    fe.half_image_compact_device(d_desc.data_ptr(), d_pts.data_ptr(), d_n.data_ptr(), d_jr.data_ptr(), d_jl.data_ptr(), d_js.data_ptr(), 8, T, D, W, FOV,
                                 od.data_ptr(), op.data_ptr(), om.data_ptr(), on.data_ptr())
    a_off, b_off = t(np.arange(0, 8, 2, dtype=np.int32) * T), t(np.arange(1, 8, 2, dtype=np.int32) * T)
    fe.sync()
    cnt = on.cpu().numpy()
    a_cnt, b_cnt = t(cnt[0::2].copy()), t(cnt[1::2].copy())
    mq = torch.zeros((4, T), dtype=torch.int32, device=dev); mt = torch.zeros((4, T), dtype=torch.int32, device=dev)
    md = torch.zeros((4, T), device=dev); mn = torch.zeros(4, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    fe.match_batch_device(od.data_ptr(), od.data_ptr(), a_off.data_ptr(), b_off.data_ptr(), a_cnt.data_ptr(), b_cnt.data_ptr(), 4, D, T, mq.data_ptr(), mt.data_ptr(),
                          md.data_ptr(), mn.data_ptr(), mode=0, ratio=ratio, radius=0.2 * W, d_pts_a=op.data_ptr(), d_pts_b=op.data_ptr())
    map_a, map_b = t(np.arange(0, 8, 2, dtype=np.int32)), t(np.arange(1, 8, 2, dtype=np.int32))          # kept alive across the launch
    torch.cuda.synchronize()
    fe.remap_matches_device(mq.data_ptr(), mt.data_ptr(), mn.data_ptr(), map_a.data_ptr(), map_b.data_ptr(), om.data_ptr(), 4, T, T)
    fe.sync(); torch.cuda.synchronize()
    return mq.cpu().numpy(), mt.cpu().numpy(), md.cpu().numpy(), mn.cpu().numpy()


def _compose(api, fe, frames, res, prm):
    """the host composition on the pipe's own keypoints; views from the existing undistort call on the same raw frames"""
    maps = qref.identity_maps()
    views = [[fe.undistort(frames[t, c], maps[c][0], maps[c][1], None) for c in range(4)] for t in range(len(frames))]
    kps = [[(r["kps_xy"][c, :r["n_kp"][c]], r["scores"][c, :r["n_kp"][c]], r["desc"][c, :r["n_kp"][c]]) for c in range(4)] for r in res]
    track, track_half = _trackers(api, fe)
    return views, qref.compose_quad(views, kps, track, track_half, prm)


def _same_quad(r, row, nb, lm, T, where):
    """one quad frame of the pipe (r) against the composition: every list array, count and id, the neighbour tracks and the list matches, bit for bit, zeros
    behind the end"""
    for c in range(4):
        k = row[c]
        n = k["n"]
        assert int(r["track_n"][c]) == n, (where, c)
        for key in ("n_tracked_in", "n_lost", "n_removed_near", "n_new"):
            assert int(r["track_" + key][c]) == k[key], (where, c, key)
        assert np.array_equal(_bits(r["track_pts"][c, :n]), _bits(k["pts"])), (where, c)
        for key in ("id", "src", "kp"):
            assert np.array_equal(r["track_" + key][c, :n], k[key]), (where, c, key)
        assert np.array_equal(_bits(r["track_desc"][c, :n]), _bits(k["desc"])) and np.array_equal(_bits(r["track_scores"][c, :n]), _bits(k["scores"])), (where, c)
        for key in ("pts", "id", "src", "kp", "desc", "scores"):
            assert not _bytes(r["track_" + key][c, n:]).any(), (where, c, key)
    assert r["track_nb_lk_xy"].shape == (4, T, 2) and r["track_nb_lk_status"].shape == (4, T) and r["track_nb_lk_status"].dtype == np.uint8
    mq, mt, md, mn = lm
    for p, (a, b, typ) in enumerate(qref.NEIGHBOURS):
        n = row[a]["n"]
        assert np.array_equal(_bits(r["track_nb_lk_xy"][p, :n]), _bits(nb[p]["pts"])) and np.array_equal(r["track_nb_lk_status"][p, :n], nb[p]["status"]), (where, p)
        assert not _bytes(r["track_nb_lk_xy"][p, n:]).any() and not r["track_nb_lk_status"][p, n:].any(), (where, p)
        m = int(mn[p])
        assert int(r["track_lnb_n"][p]) == m, (where, p)
        assert np.array_equal(r["track_lnb_q"][p, :m], mq[p, :m]) and np.array_equal(r["track_lnb_t"][p, :m], mt[p, :m]), (where, p)
        assert np.array_equal(_bits(r["track_lnb_dist"][p, :m]), _bits(md[p, :m])), (where, p)
        assert (r["track_lnb_q"][p, :m] < row[a]["n"]).all() and (r["track_lnb_t"][p, :m] < row[b]["n"]).all()


def _figures(comp, nbs, what):
    """(smallest share of a previous list the temporal track keeps, largest distance of a kept entry to (x - 3, y), smallest share of the gate-eligible entries a
    neighbour track keeps, largest distance of a kept neighbour track to (x +- 90, y))"""
    share, dist, nshare, ndist = [], 0.0, [], 0.0
    for t in range(1, len(comp)):
        for c in range(4):
            k = comp[t][c]
            ok = k["trk_status"] != 0
            share.append(ok.mean())
            d = np.linalg.norm(k["trk_pts"][ok].astype(np.float64) - (comp[t - 1][c]["pts"][ok].astype(np.float64) + [-qref.STEP, 0.0]), axis=1)
            dist = max(dist, float(d.max()) if len(d) else 0.0)
    for t in range(len(comp)):
        for p, (a, b, typ) in enumerate(qref.NEIGHBOURS):
            el, ok = nbs[t][p]["eligible"], nbs[t][p]["status"] != 0
            nshare.append(ok.sum() / max(int(el.sum()), 1))
            d = np.linalg.norm(nbs[t][p]["pts"][ok].astype(np.float64) - (comp[t][a]["pts"][ok].astype(np.float64) + [qref.SHIFT if typ == 1 else -qref.SHIFT, 0.0]), axis=1)
            ndist = max(ndist, float(d.max()) if len(d) else 0.0)
    fig = (min(share), dist, min(nshare), ndist)
    print("%s: temporal share >= %.4f, largest distance %.4f px; neighbour share >= %.4f, largest distance %.4f px" % ((what,) + fig))
    return fig


def _synthetic_list(api, rng, T, D, pts, id0):
    """one host list block with the given points: ids id0.., random scores and descriptors, a zero header but for n"""
    lw = api.lk_carry_list_bytes(T, D) // 4
    blk = np.zeros(lw, np.float32)
    v = api.lk_carry_list_views(blk, T, D)
    n = len(pts)
    v["hdr"][0] = n
    v["pts"][:n] = pts; v["id"][:n] = id0 + np.arange(n); v["src"][:n] = -1; v["kp"][:n] = np.arange(n)
    v["scores"][:n] = rng.rand(n).astype(np.float32); v["desc"][:n] = rng.randn(n, D).astype(np.float32)
    return blk


@pytest.mark.gpu
def test_quad_step_is_four_single_steps():
    """Item 1.  d2fe_lk_carry_quad_step_device against four d2fe_lk_carry_step_device calls in camera order on the same inputs and the same next_id: the whole
    list blocks (headers, both tickets, every array) and next_id, byte for byte, over three consecutive steps that swap the same two sets of blocks -- so a ticket
    that a launch did not leave zero would show in the next but one.  326 x 243 images (no multiple of 8) moving by (-3, 0), 64-dim descriptors, synthetic lists:
    camera 0 holds 151 entries, 140 on a grid and 11 twins 2 px from an earlier entry (removeNearPoints among more than 64 survivors), cameras 1 and 2 hold 41,
    camera 3 is empty (the first-frame path); total_feature_num = 150, so cameras 1, 2 and 3 all append new entries and a wrong id order shows."""
    import torch
    api, fe = _fe(max_batch=1)
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    w, h, D, T, KC, NS = 326, 243, 64, 151, 60, 3
    rng = np.random.RandomState(5)
    seqs = [[f[0] for f in ref.sliding_stereo(NS + 1, h, w, 7200 + c, 0, 3)] for c in range(4)]                  # [camera][time]
    imgs = torch.from_numpy(np.stack([np.stack([seqs[c][t] for c in range(4)]) for t in range(NS + 1)])).to(dev)      # [time][camera][h][w]
    gx, gy = np.meshgrid(np.arange(20, w - 12, 16), np.arange(16, h - 12, 16))
    grid = np.stack([gx.ravel(), gy.ravel()], 1).astype(np.float32)
    grid = grid[rng.permutation(len(grid))]
    p0 = np.concatenate([grid[:140], grid[10:21] + np.float32([2.0, 1.0])])
    host = [_synthetic_list(api, rng, T, D, p0, 5000), _synthetic_list(api, rng, T, D, grid[140:181], 6000), _synthetic_list(api, rng, T, D, grid[181:222], 7000),
            _synthetic_list(api, rng, T, D, grid[:0], 0)]
    lw = len(host[0])
    tp = api.track_params()
    assert tp.total_feature_num == 150 and api.lk_carry_list_bytes(T, D) == 4 * lw
    total = api.lk_stereo_workspace_bytes(4, w, h, 2) // 8
    ws = [torch.full((8 * total,), 0xAB, dtype=torch.uint8, device=dev) for _ in range(NS)]
    # keypoints per step: dense [4][KC] rows, one camera of one step without any
    kps = torch.zeros((NS, 4, KC, 2), device=dev); scores = torch.from_numpy(rng.rand(NS, 4, KC).astype(np.float32)).to(dev)
    desc = torch.from_numpy(rng.randn(NS, 4, KC, D).astype(np.float32)).to(dev)
    nk = rng.randint(30, KC + 1, (NS, 4)).astype(np.int32); nk[1, 2] = 0; nk[0, 3] = KC
    k_h = np.stack([rng.randint(4, w - 4, (NS, 4, KC)), rng.randint(4, h - 4, (NS, 4, KC))], -1).astype(np.float32)
    kps.copy_(torch.from_numpy(k_h)); cnt = torch.from_numpy(nk).to(dev)

    def blocks():
        a = torch.from_numpy(np.stack(host)).to(dev)
        b = torch.full((4, lw), -77.0, device=dev); b[:, :64] = 0.0           # the documented contract: a zero header before the first use as a current list
        return [a, b], torch.full((1,), 1000, dtype=torch.int32, device=dev)
    quad, qid = blocks()
    single, sid = blocks()
    torch.cuda.synchronize()
    for s in range(NS):
        api.lk_track_stereo_device(fe, imgs[s].data_ptr(), imgs[s + 1].data_ptr(), 4, w, h, None, None, 0, ws[s].data_ptr(), None, None, stream=st.cuda_stream)
    headers = []
    for s in range(NS):
        prev, cur = s % 2, (s + 1) % 2
        pp, cp = ws[s].data_ptr(), ws[s].data_ptr() + 4 * total
        api.lk_carry_quad_step(fe, pp, cp, total, w, h, quad[prev].data_ptr(), quad[cur].data_ptr(), lw, kps[s].data_ptr(), scores[s].data_ptr(), desc[s].data_ptr(),
                               cnt[s].data_ptr(), KC, qid.data_ptr(), tp=tp, desc_dim=D, stream=st.cuda_stream)
        for c in range(4):
            api.lk_carry_step(fe, pp + c * total, cp + c * total, w, h, single[prev][c].data_ptr(), single[cur][c].data_ptr(), kps[s, c].data_ptr(),
                              scores[s, c].data_ptr(), desc[s, c].data_ptr(), cnt[s, c:].data_ptr(), KC, sid.data_ptr(), tp=tp, desc_dim=D, stream=st.cuda_stream)
        st.synchronize()
        q_h, s_h = quad[cur].cpu().numpy(), single[cur].cpu().numpy()
        hd = [api.lk_carry_list_views(s_h[c], T, D) for c in range(4)]
        headers.append(hd)
        print("step", s, "n", [v["n"] for v in hd], "lost", [v["n_lost"] for v in hd], "near", [v["n_removed_near"] for v in hd], "new", [v["n_new"] for v in hd])
        for c in range(4):
            vq = api.lk_carry_list_views(q_h[c], T, D)
            for key in ("hdr", "id", "pts", "src", "kp", "scores", "desc", "trk_xy", "trk_status"):
                assert np.array_equal(_bytes(vq[key]), _bytes(hd[c][key])), (s, c, key)
            assert np.array_equal(_bytes(q_h[c]), _bytes(s_h[c])), (s, c)
            assert vq["hdr"][5] == 0 and vq["hdr"][7] == 0
        assert int(qid.cpu()[0]) == int(sid.cpu()[0]) == 1000 + sum(v["n_new"] for hh in headers for v in hh)
    # the conditions on the inputs, read from the single-step results
    h0 = headers[0]
    assert h0[0]["n_tracked_in"] == 151 and h0[0]["n_tracked_in"] - h0[0]["n_lost"] > 64 and h0[0]["n_removed_near"] > 0
    assert h0[1]["n_tracked_in"] == 41 and h0[2]["n_tracked_in"] == 41 and h0[3]["n_tracked_in"] == 0
    assert sum(v["n_new"] > 0 for v in h0) >= 3
    assert headers[1][3]["n_tracked_in"] > 0
    # refusals: D2FE_ERR_INVALID, nothing is launched
    args = (fe, ws[0].data_ptr(), ws[0].data_ptr() + 4 * total, total, w, h, quad[0].data_ptr(), quad[1].data_ptr(), lw, kps[0].data_ptr(), scores[0].data_ptr(),
            desc[0].data_ptr(), cnt[0].data_ptr(), KC, qid.data_ptr())
    for bad in ({"total_feature_num": 1024}, {"win": 20}, {"levels": 8}):
        with pytest.raises(api.D2FEError) as e:
            api.lk_carry_quad_step(*args, tp=api.track_params(**bad), desc_dim=D, stream=st.cuda_stream)
        assert e.value.code == -1
    for swap in ({3: total - 1}, {8: lw - 64}, {7: quad[0][1].data_ptr()}):          # pyr_stride, list_stride too small; current lists overlapping the previous ones
        a = list(args)
        for i, v in swap.items():
            a[i] = v
        with pytest.raises(api.D2FEError) as e:
            api.lk_carry_quad_step(*a, tp=tp, desc_dim=D, stream=st.cuda_stream)
        assert e.value.code == -1
    fe.close()


@pytest.mark.gpu
def test_neighbour_launch_is_lk_track_on_the_eligible_entries(quads):
    """Item 2.  d2fe_lk_carry_neighbour_device over two quad frames of synthetic lists (41 slots: a full list, an empty one, points exactly on both gate bounds
    x = 110 and x = 90) against api.lk_track with types 1 and 2 on the gate-eligible subset, scattered back: bit for bit, every other slot zero"""
    import torch
    api, fe = _fe(max_batch=1)
    dev = torch.device("cuda", 0)
    Q, T, D = 2, 41, 64
    rng = np.random.RandomState(9)
    tp = api.track_params(total_feature_num=T - 1)
    lw = api.lk_carry_list_bytes(T, D) // 4
    imgs = torch.from_numpy(quads[:Q].reshape(Q * 4, H, W).copy()).to(dev)
    total = api.lk_stereo_workspace_bytes(1, W, H, 2) // 2
    ws = torch.full((Q * 4 * total,), 0xAB, dtype=torch.uint8, device=dev)
    ns = [41, 30, 0, 25, 33, 41, 17, 1]
    lists = []
    for i, n in enumerate(ns):
        pts = np.stack([rng.uniform(2, W - 2, n), rng.uniform(2, H - 2, n)], 1).astype(np.float32)
        pts[:4, 0] = [110.0, np.nextafter(np.float32(110.0), np.float32(0)), 90.0, np.nextafter(np.float32(90.0), np.float32(0))][:min(n, 4)]
        pts[4:n:3] = np.rint(pts[4:n:3])
        lists.append(_synthetic_list(api, rng, T, D, pts, 100 * i))
    d_lists = torch.from_numpy(np.stack(lists)).to(dev)
    xy = torch.full((Q, 4, T, 2), -5.0, device=dev); stt = torch.full((Q, 4, T), 9, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    api.lk_track_stereo_device(fe, imgs.data_ptr(), imgs[Q * 2:].data_ptr(), Q * 2, W, H, None, None, 0, ws.data_ptr(), None, None)
    api.lk_carry_neighbour(fe, ws.data_ptr(), total, Q, W, H, FOV, d_lists.data_ptr(), lw, xy.data_ptr(), stt.data_ptr(), tp=tp, desc_dim=D)
    fe.sync(); torch.cuda.synchronize()
    xy_h, st_h = xy.cpu().numpy(), stt.cpu().numpy()
    _, track_half = _trackers(api, fe)
    mc = fe.half_move_cols(W, FOV)
    assert mc == 90.0
    kept = 0
    for q in range(Q):
        for p, (a, b, typ) in enumerate(qref.NEIGHBOURS):
            n = ns[q * 4 + a]
            pts = api.lk_carry_list_views(lists[q * 4 + a], T, D)["pts"][:n]
            ok, init = qref.half_gate(pts, typ, W, FOV)
            exp_xy = np.zeros((T, 2), np.float32); exp_st = np.zeros(T, np.uint8)
            if ok.any():
                exp_xy[:n][ok], exp_st[:n][ok] = track_half(quads[q, a], quads[q, b], pts[ok], init, typ, mc)
            if n >= 4:
                assert list(ok[:4]) == ([False, True, True, True] if typ == 1 else [True, True, True, False])
            assert np.array_equal(_bits(xy_h[q, p]), _bits(exp_xy)) and np.array_equal(st_h[q, p], exp_st), (q, p)
            kept += int(exp_st.sum())
    assert kept > 0           # the scene is the same panorama 90 px further on: some of the random points track
    bad = api.track_params(total_feature_num=1024)
    with pytest.raises(api.D2FEError) as e:
        api.lk_carry_neighbour(fe, ws.data_ptr(), total, Q, W, H, FOV, d_lists.data_ptr(), lw, xy.data_ptr(), stt.data_ptr(), tp=bad, desc_dim=D)
    assert e.value.code == -1
    for kw in (dict(pyr_stride=total - 1), dict(list_stride=lw - 64), dict(fov=0.0)):
        with pytest.raises(api.D2FEError) as e:
            api.lk_carry_neighbour(fe, ws.data_ptr(), kw.get("pyr_stride", total), Q, W, H, kw.get("fov", FOV), d_lists.data_ptr(), kw.get("list_stride", lw),
                                   xy.data_ptr(), stt.data_ptr(), tp=tp, desc_dim=D)
        assert e.value.code == -1
    fe.close()


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["wino", "f32"])
def test_quad_sp_lk_pipe_is_the_host_composition(prec, quads):
    """Items 3 and 5.  Per quad frame and view the pipe's lists, counts, ids, neighbour tracks and list matches equal the host composition bit for bit: api.LKFrame
    + api.lk_track + lk_carry_ref.compose per camera with one id counter in camera order, api.lk_track with the half-image types per pair, and the existing
    compaction / matcher / remap calls on dense copies of the lists.  Every branch fires, asserted on the composition first: a lost track, near_lk_thread_rate = 30
    removes points, total_feature_num = 40 overshoots to 41, every pair has between 1 and n - 1 eligible entries, new entries appear in two or more cameras of one
    quad frame after the first, and some pair has list matches.
    It tracks: kept entries sit at (x - 3, y), neighbour tracks at (x +- 90, y).  Floors: the CPU oracle composition (oracle SuperPoint + oracle LK + the NumPy
    list logic, total_feature_num 40, feature_min_dist 3; tools/quad_sp_lk_oracle.py, identical in both modes) on the same 8 quad frames keeps at least 0.9756 of
    every previous list with a largest distance of 0.5709 px to (x - 3, y), and every neighbour track keeps at least 0.7000 of its gate-eligible entries (15 to 34 of
    30 to 41 per pair) with a largest distance of 0.3616 px to (x +- 90, y).  Margin: a tenth of the share, 0.25 px on the distance."""
    import torch
    api, fe = _fe(prec)
    for name, extra in (("total40", {}), ("near30", {"near_lk_thread_rate": 30.0})):
        prm = dict(BASE); prm.update(extra)
        res = _run(api, fe, quads, lanes=2, Q=2, track_params=prm)
        views, (comp, nbs) = _compose(api, fe, quads, res, prm)
        for t in range(NQ):
            assert all(np.array_equal(views[t][c], quads[t, c]) for c in range(4))          # identity maps: a raw frame is its own view
        flat = [k for row in comp for k in row]
        print(name, "n", [[k["n"] for k in row] for row in comp], "lost", [[k["n_lost"] for k in row] for row in comp], "near", [[k["n_removed_near"] for k in row] for row in comp],
              "new", [[k["n_new"] for k in row] for row in comp])
        assert all(k["n"] <= 41 for k in flat)
        if name == "total40":
            assert any(k["n_lost"] > 0 for k in flat) and any(k["n"] == 41 for k in flat)
        else:
            assert any(k["n_removed_near"] > 0 for k in flat)
        for t in range(NQ):
            for p, (a, b, typ) in enumerate(qref.NEIGHBOURS):
                assert 1 <= int(nbs[t][p]["eligible"].sum()) <= comp[t][a]["n"] - 1, (t, p)
        assert any(sum(k["n_new"] > 0 for k in row) >= 2 for row in comp[1:])
        ids = qref.quad_ids_naive([[k["src"] for k in row] for row in comp])
        total_lnb = 0
        for t in range(NQ):
            lm = _list_matches(api, fe, torch, comp[t], 41, 256)
            total_lnb += int(lm[3].sum())
            _same_quad(res[t], comp[t], nbs[t], lm, 41, (name, t))
            for c in range(4):
                assert list(res[t]["track_id"][c, :comp[t][c]["n"]]) == ids[t][c]
        assert total_lnb > 0
        if name == "total40":
            share, dist, nshare, ndist = _figures(comp, nbs, prec)
            assert share >= ORACLE_SHARE * 0.9 and dist <= ORACLE_DIST + 0.25
            assert nshare >= ORACLE_NB_SHARE * 0.9 and ndist <= ORACLE_NB_DIST + 0.25
    fe.close()


# the CPU oracle composition's figures for the scene of this file (the docstring above; tools/quad_sp_lk_oracle.py prints them)
ORACLE_SHARE, ORACLE_DIST, ORACLE_NB_SHARE, ORACLE_NB_DIST = 0.9756, 0.5709, 0.7000, 0.3616


@pytest.mark.gpu
def test_quad_sp_lk_results_do_not_depend_on_the_shape_of_the_pipe(quads):
    """Item 4.  (lanes, quads) = (4, 1), (2, 2), (1, 4), (4, 4) against (1, 1) over the 8 quad frames, the chain across submits and lanes included; the keypoint-based
    neighbour and temporal matches switched on beside the mode in two of the shapes, where they must equal a plain pipe's"""
    api, fe = _fe(netvlad=True)
    base = _run(api, fe, quads)
    assert any(int(r["track_n_lost"].sum()) > 0 for r in base) and any(int(r["track_n_new"].sum()) > 0 for r in base[1:]) and sum(int(r["track_lnb_n"].sum()) for r in base) > 0
    plain = _run(api, fe, quads, lanes=2, Q=2, sp_lk=False, track_params=None, match_neighbour=True, match_prev=True, netvlad=True)
    assert "track_n" not in plain[0]
    for lanes, Q, kw in ((4, 1, {}), (2, 2, dict(match_neighbour=True, match_prev=True, netvlad=True)), (1, 4, {}), (4, 4, dict(match_neighbour=True, match_prev=True))):
        got = _run(api, fe, quads, lanes=lanes, Q=Q, **kw)
        assert len(got) == NQ
        for t, (g, b) in enumerate(zip(got, base)):
            assert np.array_equal(g["n_kp"], b["n_kp"])
            for k in TRACK_KEYS:
                assert np.array_equal(_bytes(g[k]), _bytes(b[k])), (lanes, Q, t, k)
            for c in range(4):          # keypoint rows behind n_kp are not part of a result (tests/test_quad_pipe.py compares the same way)
                n = int(b["n_kp"][c])
                for k in ("kps_xy", "scores", "desc"):
                    assert np.array_equal(_bytes(g[k][c, :n]), _bytes(b[k][c, :n])), (lanes, Q, t, c, k)
            for p in range(4):
                m = int(b["track_lnb_n"][p])
                for k in ("track_lnb_q", "track_lnb_t", "track_lnb_dist"):
                    assert np.array_equal(_bytes(g[k][p, :m]), _bytes(b[k][p, :m])), (lanes, Q, t, k)
            if kw:      # the keypoint-based results beside the mode are the plain pipe's
                for pre in ("nb", "prev"):
                    assert np.array_equal(g[pre + "_n"], plain[t][pre + "_n"])
                    for p in range(4):
                        m = int(g[pre + "_n"][p])
                        for k in ("_q", "_t", "_dist"):
                            assert np.array_equal(_bytes(g[pre + k][p, :m]), _bytes(plain[t][pre + k][p, :m])), (lanes, Q, t, pre + k)
                if kw.get("netvlad"):
                    assert np.array_equal(_bytes(g["netvlad"]), _bytes(plain[t]["netvlad"]))
    fe.close()


@pytest.mark.gpu
def test_quad_sp_lk_contract(quads):
    """Item 6.  The refusals, each with the documented status; a refusal leaves the pipe as it was; a pipe without the mode returns the bits of a second plain pipe"""
    api, fe = _fe(max_batch=4)
    fr = quads[0][None]
    plain = _pipe(api, fe, sp_lk=False, track_params=None, match_neighbour=True, match_prev=True)
    other = _pipe(api, fe, sp_lk=False, track_params=None, match_neighbour=True, match_prev=True)
    for bad in ({"levels": 3}, {"total_feature_num": 1024}, {"win": 22}, {"feature_min_dist": -1.0}):
        with pytest.raises(api.D2FEError) as e:
            other.track_enable(bad)
        assert e.value.code == -1, bad
    for i in range(2):          # the refused pipe and a pipe nobody asked: the same bits
        a, b = plain.wait(plain.submit(quads[i][None])), other.wait(other.submit(quads[i][None]))
        assert sorted(a) == sorted(b) and "track_n" not in a
        for k in a:
            assert (a[k] is None and b[k] is None) or np.array_equal(_bytes(a[k]), _bytes(b[k])), k
    with pytest.raises(api.D2FEError) as e:
        other.track_enable(None)
    assert e.value.code == -1 and "first submit" in str(e.value)
    with pytest.raises(api.D2FEError) as e:
        plain.track_result_raw(0)
    assert e.value.code == -5                         # D2FE_ERR_UNSUPPORTED
    plain.close(); other.close()
    with pytest.raises(api.D2FEError) as e:           # through the constructor; no pipe is left alive
        _pipe(api, fe, track_params={"total_feature_num": 1024})
    assert e.value.code == -1 and "1024" in str(e.value)
    pipe = _pipe(api, fe, track_params=None)          # the reference's defaults: 151 slots
    with pytest.raises(api.D2FEError) as e:
        pipe.track_enable(None)
    assert e.value.code == -1                         # accepted once
    t = pipe.submit(fr)
    with pytest.raises(api.D2FEError) as e:
        pipe.track_result_raw(t)
    assert e.value.code == -3                         # D2FE_ERR_NOT_READY: not waited for yet
    o = pipe.wait(t)
    assert o["track_pts"].shape == (1, 4, 151, 2) and o["track_nb_lk_status"].shape == (1, 4, 151) and o["nb_n"] is None and o["prev_n"] is None
    assert (o["track_n"] == o["track_n_new"]).all() and int(o["track_n"].min()) > 0 and int(o["track_n_tracked_in"].sum()) == 0
    tr = pipe.track_result_raw(t)
    assert (tr.quads, tr.cap_tracks, tr.desc_dim, tr.list_words * 4) == (1, 151, 256, api.lk_carry_list_bytes(151, 256))
    with pytest.raises(api.D2FEError) as e:
        pipe.track_result_raw(t + 1)
    assert e.value.code == -1                         # unknown ticket
    o2 = pipe.wait(pipe.submit(quads[1][None]))
    assert np.array_equal(o2["track_n_tracked_in"], o["track_n"])
    pipe.close(); fe.close()


@pytest.mark.gpu
def test_quad_sp_lk_through_the_cpp_mirror(tmp_path, quads):
    """Item 7.  tests/cpp/quad_track_test.cpp (g++, only libd2fe_hip.so; d2fe::QuadPipe::trackEnable and QuadResult::tracks of include/d2fe.hpp, 2 lanes x 2 quad
    frames per submit) writes every list, neighbour track and list match; they equal the Python binding's one-lane pipe"""
    from d2slam_amd.weights import save_superpoint_d2fw
    from tests.test_quad_pipe import _weights
    from tests.test_quad_pipe_sp_lk_cpu import build_cpp
    exe = build_cpp(tmp_path)
    sp, fin, fout = (str(tmp_path / n) for n in ("sp.d2fw", "in.bin", "out.bin"))
    save_superpoint_d2fw(sp, _weights())
    maps = qref.identity_maps()
    T = 41
    with open(fin, "wb") as f:
        f.write(struct.pack("<6i", NQ, H, W, CAP, BASE["total_feature_num"], 0))
        f.write(struct.pack("<d", BASE["feature_min_dist"]))
        for mm in maps:
            for m in mm[:2]:
                f.write(np.ascontiguousarray(m, np.float32).tobytes())
        f.write(quads.tobytes())
    res = subprocess.run([exe, sp, fin, fout, "2", "2"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "quad_track_test OK" in res.stdout
    data, pos = open(fout, "rb").read(), 0

    def take(dt, shape):
        nonlocal pos
        n = int(np.prod(shape))
        a = np.frombuffer(data, dt, n, pos).reshape(shape).copy(); pos += n * np.dtype(dt).itemsize
        return a
    api, fe = _fe(max_batch=4)
    base = _run(api, fe, quads)
    for t in range(NQ):
        b = base[t]
        n = take("<i4", 4); n_new = take("<i4", 4)
        assert np.array_equal(n, b["track_n"]) and np.array_equal(n_new, b["track_n_new"])
        pts = take("<f4", (4, T, 2)); ids = take("<i4", (4, T)); src = take("<i4", (4, T)); desc0 = take("<f4", (4, T))
        assert np.array_equal(_bits(pts), _bits(b["track_pts"])) and np.array_equal(ids, b["track_id"]) and np.array_equal(src, b["track_src"])
        assert np.array_equal(_bits(desc0), _bits(b["track_desc"][:, :, 0]))
        nbxy = take("<f4", (4, T, 2)); nbst = take("u1", (4, T))
        assert np.array_equal(_bits(nbxy), _bits(b["track_nb_lk_xy"])) and np.array_equal(nbst, b["track_nb_lk_status"])
        ln = take("<i4", 4); lq = take("<i4", (4, T)); lt = take("<i4", (4, T))
        assert np.array_equal(ln, b["track_lnb_n"])
        for p in range(4):
            assert np.array_equal(lq[p, :ln[p]], b["track_lnb_q"][p, :ln[p]]) and np.array_equal(lt[p, :ln[p]], b["track_lnb_t"][p, :ln[p]])
    assert pos == len(data)
    fe.close()
