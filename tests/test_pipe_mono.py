"""The single-camera pipe (d2fe_pipe_camera.mono / .depth through d2fe_pipe_create_camera, include/d2fe.h): the reference's MONOCULAR configuration (generateImageDescriptor, loop_cam.cpp:259-331;
track(frames.images[0]), d2featuretracker.cpp:105-107) and PINHOLE_DEPTH (generateGrayDepthImageDescriptor, loop_cam.cpp:333-441; createLKLandmark's depth read,
d2featuretracker.cpp:790-798) with frames in flight.  All on the left frames of sliding_stereo(12 frames, 128 x 192, seed 7105, disparity 12): seeded weights, 64
keypoints, the Winograd mode.  The mono pipe is held bit for bit to the stereo pipe on the same left frames (whose right frames are arbitrary), to the single-call
entry points, and, for the depth values, to the NumPy restatement of the value contract (tests/helpers/depth_ref.py, pinned in tests/test_pipe_mono_cpu.py)."""
import numpy as np
import pytest

from tests.helpers import depth_ref
from tests.helpers import lk_carry_ref as ref

H, W, CAP = 128, 192, 64
SEED, DISP, STEP, NF = 7105, 12, 3, 12
TOTAL = 40                # total_feature_num: lists of up to 41 entries
TRACK_KEYS = ("track_n", "track_pts", "track_id", "track_src", "track_kp", "track_desc", "track_scores", "track_n_tracked_in", "track_n_lost", "track_n_removed_near",
              "track_n_new")
FRAME_KEYS = ("kps_xy", "scores", "desc", "n_kp", "netvlad", "prev_q", "prev_t", "prev_dist", "prev_n")
SHAPES = {"l1f1": dict(lanes=1, frames=1), "l2f2": dict(lanes=2, frames=2), "l3c2": dict(lanes=3, frames=1, coalesce=2), "l2g2": dict(lanes=2, frames=1, netvlad_group=2),
          "l2f2_bare": dict(lanes=2, frames=2, netvlad=False, match_prev=False)}


@pytest.fixture(scope="module")
def frames():
    return ref.sliding_stereo(NF, H, W, SEED, DISP, STEP)


@pytest.fixture(scope="module")
def depths():
    return depth_ref.seeded_depth(NF, H, W, SEED + 1)


@pytest.fixture(scope="module")
def ctx():
    from d2slam_amd import api, netvlad as nvm
    from d2slam_amd.weights import synthetic_superpoint_weights
    fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=CAP, input_width=W, input_height=H, max_batch=4, precision=api.PREC_F32_WINO, keypoint_threshold=0.005))
    fe.load_superpoint(synthetic_superpoint_weights(dustbin_bias=7.5)); fe.load_netvlad(nvm.synthetic_netvlad_weights())
    yield api, fe, {}
    fe.close()


def _copy(d):
    return {k: (None if v is None else v.copy()) for k, v in d.items()}


def _run(ctx, seq, depths=None, depth_pad=0, loop_kw=None, **kw):
    """all NF left frames through one pipe, lanes * coalesce submits in flight -> one dict per FRAME (copies).  Runs are cached per configuration: the tests share them."""
    api, fe, cache = ctx
    key = repr(sorted(kw.items())) + repr((depths is not None, depth_pad, loop_kw))
    if key in cache:
        return cache[key]
    kw = dict(kw)
    F = kw.setdefault("frames", 1)
    mono = kw.get("mono", False)
    kw.setdefault("match_lr", False)
    pipe = api.StereoPipe(fe, width=W, height=H, cap=CAP, **kw)
    if kw.get("sp_lk"):
        pipe.set_track_params(dict(total_feature_num=TOTAL))
    loop = api.LoopQuery(pipe, **loop_kw) if loop_kw else None
    inflight = pipe.lanes * kw.get("coalesce", 1)
    nsub = NF // F
    tk, out, col = [], [], []

    def take():
        i = len(out)
        out.append(_copy(pipe.wait(tk[i])))
        if loop is not None:
            c = loop.collect(i % loop.slots)
            assert c["ticket"] == tk[i]
            col.append({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.items() if k not in ("ticket", "phase_ms")})
    for i in range(nsub):
        fr = seq[i * F:(i + 1) * F]
        left = np.stack([f[0] for f in fr])
        if depths is not None:
            d = depths[i * F:(i + 1) * F]
            if depth_pad:                                   # rows further apart than the image is wide; the padding holds a value no lookup may return
                wide = np.full((F, H, W + depth_pad), 4242, np.uint16)
                wide[:, :, :W] = d
                d = wide[:, :, :W]
            tk.append(pipe.submit(left, depth=d))
        elif mono:
            tk.append(pipe.submit(left))
        else:
            tk.append(pipe.submit(left, np.stack([f[1] for f in fr])))
        if loop is not None:
            loop.enqueue(tk[i], i % loop.slots, np.uint8([(i * F + f) % 3 != 2 for f in range(F)]))
        if len(tk) - len(out) >= inflight:
            take()
    while len(out) < nsub:
        take()
    if loop is not None:
        loop.close()
    pipe.close()
    res = []
    for o in out:
        assert o["kps_xy"].shape == (2 * F, CAP, 2) and o["n_kp"].shape == (2 * F,)
        for f in range(F):
            r = {k: (None if o[k] is None else o[k][f]) for k in o if k not in ("lr_q", "lr_t", "lr_dist", "lr_n")}
            r["right_n_kp"] = int(o["n_kp"][F + f]); r["lr"] = [o[k] for k in ("lr_q", "lr_t", "lr_dist", "lr_n")]
            res.append(r)
    cache[key] = (res, col)
    return cache[key]


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


COUNT_OF = {"kps_xy": "n_kp", "scores": "n_kp", "desc": "n_kp", "prev_q": "prev_n", "prev_t": "prev_n", "prev_dist": "prev_n"}


def _same(a, b, keys, where):
    """bit for bit; rows of the keypoint and match arrays up to their count (what lies behind it is not part of the contract), the list arrays whole"""
    for k in keys:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, (where, k)
            continue
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, (where, k)
        if k in COUNT_OF:
            n = int(a[COUNT_OF[k]])
            assert n == int(b[COUNT_OF[k]]), (where, k)
            x, y = x[:n], y[:n]
        assert np.array_equal(_bytes(x), _bytes(y)), (where, k)


@pytest.mark.gpu
def test_mono_pipe_equals_the_stereo_pipe_and_the_single_calls(ctx, frames):
    """left rows, NetVLAD and the temporal matches: mono pipe == stereo pipe with match_lr = 0 (right frames arbitrary) == extract_all_batch + matchKNN; the rows of
    right images hold n_kp = 0 and lr_* are None"""
    api, fe, _ = ctx
    mono, _ = _run(ctx, frames, lanes=2, mono=True)
    stereo, _ = _run(ctx, frames, lanes=2)
    assert len(mono) == len(stereo) == NF
    prev, nmatch = None, 0
    for t in range(NF):
        m, s = mono[t], stereo[t]
        _same(m, s, FRAME_KEYS, t)
        assert m["right_n_kp"] == 0 and all(v is None for v in m["lr"]) and int(s["right_n_kp"]) > 0
        ext, g = fe.extract_all_batch(frames[t][0][None], 1, cap=CAP)
        k, sc, d = ext[0]
        n = int(m["n_kp"])
        assert n == len(k) and n > 20
        assert np.array_equal(_bytes(m["kps_xy"][:n]), _bytes(k)) and np.array_equal(_bytes(m["scores"][:n]), _bytes(sc)) and np.array_equal(_bytes(m["desc"][:n]), _bytes(d))
        assert np.array_equal(_bytes(m["netvlad"]), _bytes(g[0]))
        np_ = int(m["prev_n"])
        if prev is None:
            assert np_ == 0
        else:
            q, tt, dist = fe.match_knn(d, prev[2], 0.8)
            assert np_ == len(q)
            assert np.array_equal(m["prev_q"][:np_], q) and np.array_equal(m["prev_t"][:np_], tt) and np.array_equal(_bytes(m["prev_dist"][:np_]), _bytes(dist))
            nmatch += np_
        prev = (k, sc, d)
    assert nmatch > 0


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_mono_results_do_not_depend_on_the_shape_of_the_pipe(shape, ctx, frames):
    base, _ = _run(ctx, frames, lanes=2, mono=True)
    got, _ = _run(ctx, frames, mono=True, **SHAPES[shape])
    bare = SHAPES[shape].get("netvlad") is False
    for t in range(NF):
        _same(got[t], base[t], ("kps_xy", "scores", "desc", "n_kp") if bare else FRAME_KEYS, (shape, t))
        assert got[t]["right_n_kp"] == 0 and all(v is None for v in got[t]["lr"])
        if bare:
            assert got[t]["netvlad"] is None and got[t]["prev_q"] is None


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["l2f2", "l3c2"])
def test_mono_sp_lk_equals_the_stereo_sp_lk_lists(shape, ctx, frames):
    """the LK-carried list on the one image: every track_* field but the right tracks is the lr_lk + sp_lk stereo pipe's"""
    mono, _ = _run(ctx, frames, mono=True, sp_lk=True, **SHAPES[shape])
    stereo, _ = _run(ctx, frames, lr_lk=True, sp_lk=True, **SHAPES[shape])
    carried = 0
    for t in range(NF):
        _same(mono[t], stereo[t], TRACK_KEYS + FRAME_KEYS, (shape, t))
        assert mono[t]["track_right_pts"] is None and mono[t]["track_right_status"] is None and stereo[t]["track_right_pts"] is not None
        assert mono[t]["track_pts"].shape == (TOTAL + 1, 2)
        carried += int(mono[t]["track_n_tracked_in"]) - int(mono[t]["track_n_lost"])
    assert int(mono[0]["track_n"]) > 5 and carried > 0


def _check_depth(res, depths, where):
    kp_hit = tr_hit = 0
    for t, r in enumerate(res):
        n, m = int(r["n_kp"]), int(r["track_n"])
        assert r["kp_depth_mm"].dtype == np.uint16 and r["kp_depth_mm"].shape == (CAP,) and r["track_depth_mm"].shape == (TOTAL + 1,)
        assert np.array_equal(r["kp_depth_mm"][:n], depth_ref.depth_at_np(depths[t], r["kps_xy"][:n])), (where, t)
        assert np.array_equal(r["track_depth_mm"][:m], depth_ref.depth_at_np(depths[t], r["track_pts"][:m])), (where, t)
        assert not r["kp_depth_mm"][n:].any() and not r["track_depth_mm"][m:].any(), (where, t)
        kp_hit += int((r["kp_depth_mm"][:n] != 0).sum()); tr_hit += int((r["track_depth_mm"][:m] != 0).sum())
    assert kp_hit > 100 and tr_hit > 100


@pytest.mark.gpu
def test_depth_through_the_pipe(ctx, frames, depths):
    """kp_depth_mm / track_depth_mm are the restatement on the pipe's own keypoints and list positions, zeros behind the counts, also from a depth image whose rows
    are further apart than 2 * width bytes; everything else is the same pipe's without depth"""
    plain, _ = _run(ctx, frames, mono=True, sp_lk=True, **SHAPES["l2f2"])
    for pad, shape in ((0, "l2f2"), (8, "l2f2"), (0, "l3c2")):
        got, _ = _run(ctx, frames, depths=depths, depth_pad=pad, mono=True, depth=True, sp_lk=True, **SHAPES[shape])
        _check_depth(got, depths, (pad, shape))
        for t in range(NF):
            _same(got[t], plain[t], TRACK_KEYS + FRAME_KEYS, (pad, shape, t))
            assert got[t]["track_right_pts"] is None and got[t]["right_n_kp"] == 0
        frac = sum(int((np.rint(r["track_pts"][:int(r["track_n"])]) != r["track_pts"][:int(r["track_n"])]).any(1).sum()) for r in got)
        assert frac > 0                                   # list entries between pixels took part
    # without sp_lk: keypoints only, track_depth_mm is None
    got, _ = _run(ctx, frames, depths=depths, mono=True, depth=True, lanes=2)
    base, _ = _run(ctx, frames, lanes=2, mono=True)
    for t in range(NF):
        n = int(got[t]["n_kp"])
        assert got[t]["track_depth_mm"] is None and np.array_equal(got[t]["kp_depth_mm"][:n], depth_ref.depth_at_np(depths[t], got[t]["kps_xy"][:n])) and not got[t]["kp_depth_mm"][n:].any()
        _same(got[t], base[t], FRAME_KEYS, t)


@pytest.mark.gpu
@pytest.mark.parametrize("pad", [0, 8])
def test_depth_from_pinned_input(pad, ctx, frames, depths):
    """pinned_input = 1: gray and depth frames are DMAed straight from the caller's page-locked memory (tight frames in one copy, padded rows as 2D copies)"""
    import torch
    api, fe, _ = ctx
    base, _ = _run(ctx, frames, lanes=2, mono=True)
    F = 2
    pipe = api.StereoPipe(fe, lanes=2, frames=F, width=W, height=H, cap=CAP, netvlad=False, match_lr=False, mono=True, depth=True, pinned_input=True)
    gray = torch.from_numpy(np.stack([f[0] for f in frames])).pin_memory()
    wide = np.full((NF, H, W + pad), 4242, np.uint16); wide[:, :, :W] = depths
    dep = torch.from_numpy(wide.view(np.int16)).pin_memory()
    hits = 0
    for i in range(NF // F):
        t = pipe.submit_depth_ptr(gray.data_ptr() + i * F * H * W, dep.data_ptr() + i * F * H * (W + pad) * 2, depth_stride=2 * (W + pad))
        r = pipe.wait(t)
        for f in range(F):
            n = int(r["n_kp"][f]); b = base[i * F + f]
            assert n == int(b["n_kp"]) and np.array_equal(_bytes(r["kps_xy"][f, :n]), _bytes(b["kps_xy"][:n]))
            assert np.array_equal(r["kp_depth_mm"][f, :n], depth_ref.depth_at_np(depths[i * F + f], r["kps_xy"][f, :n])) and not r["kp_depth_mm"][f, n:].any()
            hits += int((r["kp_depth_mm"][f, :n] != 0).sum())
    pipe.close()
    assert hits > 100


@pytest.mark.gpu
def test_depth_at_device_alone_on_injected_points(ctx):
    """24 x 16, three lists of cap 70 (more than one wave) with 0, 1 and 70 points: the CPU test's table, the four corners and random points; the output buffer is
    pre-filled with 0xFFFF, so every slot >= n must have been WRITTEN as 0.  Also with padded rows and lists further apart than 2 * cap floats."""
    import torch
    api, fe, _ = ctx
    dw, dh, cap, nl = 24, 16, 70, 3
    rng = np.random.RandomState(99)
    depth = depth_ref.seeded_depth(nl, dh, dw, 31)
    depth[depth == 0] = 1; depth[:, 0, 0] = 0; depth[:, dh - 1, dw - 1] = 65535
    table = np.float32([p for p, _ in depth_ref.edge_table(dw, dh)])
    pts = np.full((nl, cap, 2), np.nan, np.float32)
    pts[0] = rng.uniform(-2, dw + 2, (cap, 2))                       # list 0 has no entries: none of these may be read into the output
    pts[1, 0] = (2.5, 3.5)
    pts[1, 1:] = rng.uniform(0, dh, (cap - 1, 2))
    pts[2, :len(table)] = table
    pts[2, len(table):] = rng.uniform(-1.5, dw + 1.5, (cap - len(table), 2))
    pts[2, -6:] = np.float32([[0.5, 0.5], [1.5, 1.5], [22.5, 14.5], [23.49, 15.49], [23.5, 15.5], [11.5, 7.5]])
    n = np.int32([0, 1, cap])
    want = np.zeros((nl, cap), np.uint16)
    for l in range(nl):
        want[l, :n[l]] = depth_ref.depth_at_np(depth[l], pts[l, :n[l]])
    assert (want[2] != 0).sum() > 30 and (want[2] == 0).sum() > 8 and want[1, 0] == depth[1, 4, 2]
    dev = torch.device("cuda")
    for row_pad, list_pad in ((0, 0), (6, 10)):
        dimg = np.full((nl, dh + 1, dw + row_pad), 4242, np.uint16); dimg[:, :dh, :dw] = depth
        dpts = np.full((nl, 2 * cap + list_pad), 7.0, np.float32); dpts[:, :2 * cap] = pts.reshape(nl, -1)
        d_img = torch.from_numpy(dimg.view(np.int16)).to(dev); d_pts = torch.from_numpy(dpts).to(dev); d_n = torch.from_numpy(n).to(dev)
        d_out = torch.full((nl, cap), -1, dtype=torch.int16, device=dev)
        torch.cuda.synchronize()
        api.depth_at_device(fe, d_img.data_ptr(), dw, dh, 2 * (dw + row_pad), 2 * (dw + row_pad) * (dh + 1), d_pts.data_ptr(), 2 * cap + list_pad, d_n.data_ptr(), nl, cap,
                            d_out.data_ptr())
        fe.sync()
        got = d_out.cpu().numpy().view(np.uint16)
        assert np.array_equal(got, want), (row_pad, list_pad, np.argwhere(got != want)[:8].tolist())
    for bad in (dict(width=0), dict(depth_stride=2 * dw - 2), dict(depth_stride=2 * dw + 1), dict(cap=0), dict(n_lists=0), dict(pts_stride=2 * cap - 1)):
        a = dict(width=dw, height=dh, depth_stride=2 * dw, depth_image_stride=2 * dw * dh, pts_stride=2 * cap, n_lists=nl, cap=cap); a.update(bad)
        with pytest.raises(api.D2FEError) as e:
            api.depth_at_device(fe, d_img.data_ptr(), a["width"], a["height"], a["depth_stride"], a["depth_image_stride"], d_pts.data_ptr(), a["pts_stride"], d_n.data_ptr(),
                                a["n_lists"], a["cap"], d_out.data_ptr())
        assert e.value.code == -1, bad


@pytest.mark.gpu
def test_mono_contract(ctx, frames, depths):
    api, fe, _ = ctx
    INVALID, NOT_READY, UNSUPPORTED = -1, -3, -5
    mk = lambda **kw: api.StereoPipe(fe, lanes=2, width=W, height=H, cap=CAP, netvlad=False, **kw)
    for bad in (dict(mono=True, match_lr=True), dict(mono=True, match_lr=False, lr_lk=True), dict(depth=True, match_lr=False), dict(sp_lk=True, match_lr=False),
                dict(depth=True, match_lr=False, lr_lk=True)):
        with pytest.raises(api.D2FEError) as e:
            mk(**bad)
        assert e.value.code == INVALID, bad
    left, right, dep = frames[0][0], frames[0][1], depths[0]

    def refused(fn, code=INVALID):
        with pytest.raises(api.D2FEError) as e:
            fn()
        assert e.value.code == code

    # every refused submit queues nothing and leaves the pipe usable: the ticket numbers go on without a gap and the results are the frame's
    mono = mk(mono=True, match_lr=False)
    refused(lambda: mono.submit(left, right))                            # a right image on a mono pipe
    t0 = mono.submit(left)
    refused(lambda: mono.submit(left, depth=dep))                        # submit_depth on a pipe without depth
    t1 = mono.submit(left)
    assert (t0, t1) == (0, 1)
    refused(lambda: mono.depth_result_raw(t0), UNSUPPORTED)
    a, b = _copy(mono.wait(t0)), _copy(mono.wait(t1))
    assert int(a["n_kp"][0]) > 20 and a["n_kp"][1] == 0 and np.array_equal(_bytes(a["kps_xy"][0, :int(a["n_kp"][0])]), _bytes(b["kps_xy"][0, :int(b["n_kp"][0])])) and int(b["prev_n"][0]) > 10
    refused(lambda: mono.depth_result_raw(t0), UNSUPPORTED)
    mono.close()
    stereo = mk(match_lr=False)
    refused(lambda: stereo.submit(left))                                 # NULL right on a stereo pipe, as before
    refused(lambda: stereo.submit(left, depth=dep))
    t0 = stereo.submit(left, right)
    assert t0 == 0 and int(stereo.wait(t0)["n_kp"][1]) > 20
    refused(lambda: stereo.depth_result_raw(t0), UNSUPPORTED)
    stereo.close()
    dp = mk(mono=True, depth=True, match_lr=False)
    refused(lambda: dp.submit(left))                                     # plain submit on a depth pipe
    refused(lambda: dp.submit_depth_ptr(left.ctypes.data, dep.ctypes.data, depth_stride=2 * W - 2))
    refused(lambda: dp.submit_depth_ptr(left.ctypes.data, dep.ctypes.data, depth_stride=2 * W + 1))
    t0 = dp.submit(left, depth=dep)
    assert t0 == 0
    refused(lambda: dp.depth_result_raw(t0), NOT_READY)                  # before the wait
    r = dp.wait(t0)
    n = int(r["n_kp"][0])
    assert r["track_depth_mm"] is None and np.array_equal(r["kp_depth_mm"][0, :n], depth_ref.depth_at_np(dep, r["kps_xy"][0, :n])) and np.array_equal(_bytes(r["kps_xy"][0, :n]), _bytes(a["kps_xy"][0, :int(a["n_kp"][0])]))
    refused(lambda: dp.depth_result_raw(t0 + 1))                         # unknown ticket
    dp.close()


@pytest.mark.gpu
def test_loop_query_on_a_mono_pipe(ctx, frames):
    """one consumer: api.LoopQuery behind the mono pipe gives what it gives behind the stereo pipe on the same left frames and keyframe flags"""
    kw = dict(capacity_keyframes=NF + 4, max_index=2, thres=0.0, ratio=0.8, mode=0, slots=3)
    _, mono = _run(ctx, frames, loop_kw=kw, lanes=2, mono=True)
    _, stereo = _run(ctx, frames, loop_kw=kw, lanes=2)
    assert len(mono) == len(stereo) == NF
    hits = 0
    for t in range(NF):
        assert sorted(mono[t]) == sorted(stereo[t])
        for k in mono[t]:
            a, b = mono[t][k], stereo[t][k]
            assert (np.array_equal(_bytes(a), _bytes(b)) if isinstance(a, np.ndarray) else a == b), (t, k)
        hits += int((mono[t]["label"] >= 0).sum())
    assert hits > 0
