"""Remote tracking against the keyframe window on the device (d2fe_window_*; include/d2fe.h, csrc/window.hip): D2FeatureTracker::trackRemoteFrames
(d2featuretracker.cpp:237-310) -- getMatchedPrevKeyframe's walk through current_keyframes and matchKNN(keyframe, remote) -- as gate -> match -> D2H per batch.
  (a) d2fe_window_track_device on its own: planted windows and remote frames (tests/helpers/keyframe_window_common.py) against the oracle's tracker_gate (and the
      reference-compiled one where it is available), bitwise against d2fe_gate_pairs_device / d2fe_quad_gate_device and d2fe_match_knn / d2fe_match_crosscheck;
  (b) the threshold itself, in exact arithmetic;
  (c) behind a stereo pipe and a quad pipe: push / retain over several tickets, later tickets tracked in place through the device view and as dense uploads, both
      bitwise equal to the host composition of the existing calls; then one-rank loopback exchanges (fp32 and int8 wire) read in place through track_exchange;
  (d) the refusals, each leaving the window as it was;
  (e) a configuration struct cut short by its struct_size."""
import ctypes as C

import numpy as np
import pytest

from oracle import ref as spref
from tests.helpers import keyframe_window_common as kw

H, W, CAP = 120, 160, 60
RATIO = 0.8
D = kw.D


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _copy(r):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in r.items()}


def _stereo_fe(max_batch, netvlad=True, pca=0):
    from d2slam_amd import api, netvlad as nvm
    from d2slam_amd.weights import synthetic_superpoint_weights
    fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=CAP, input_width=W, input_height=H, max_batch=max_batch, precision=api.PREC_F32_WINO))
    fe.load_superpoint(synthetic_superpoint_weights(dustbin_bias=7.5))
    if netvlad:
        fe.load_netvlad(nvm.synthetic_netvlad_weights(depth_multiplier=0.35))      # the 0.35-wide stand-in of the loop tests
        if pca:
            fe.set_netvlad_pca(*nvm.synthetic_netvlad_pca(out_dims=pca))
    return api, fe


def _mk_pipe(api, fe, V, lanes, n):
    if V == 1:
        return api.StereoPipe(fe, lanes=lanes, frames=n, width=W, height=H, cap=CAP, netvlad=True)
    from tests.helpers import quad_exchange_common as qc
    return qc.quad_pipe(fe, lanes, n)


def _pipe(V, pca=0, lanes=1, n=1):
    """(api, fe, pipe) with a stereo pipe (V = 1, n frames per submit) or a quad pipe (V = 4, n quads per submit)"""
    from d2slam_amd import api, netvlad as nvm
    if V == 1:
        _, fe = _stereo_fe(2 * n, pca=pca)
    else:
        from tests.helpers import quad_exchange_common as qc
        assert qc.CAP == CAP
        fe = qc.frontend(4 * n)
        if pca:
            fe.set_netvlad_pca(*nvm.synthetic_netvlad_pca(out_dims=pca))
    return api, fe, _mk_pipe(api, fe, V, lanes, n)


def _match(fe, mode, a, b):
    """(q, t, d) of the existing host calls; an empty side gives no matches (d2featuretracker.cpp:278-279)"""
    if len(a) == 0 or len(b) == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)
    return fe.match_knn(a, b, RATIO) if mode == 0 else fe.match_crosscheck(a, b)


def _compose(api, fe, win, rem, thres, mode):
    """The host composition of the existing calls: the gate keyframe by keyframe, newest first (d2fe_gate_pairs_device / d2fe_quad_gate_device on uploaded vectors),
    then d2fe_match_knn / d2fe_match_crosscheck of the chosen keyframe's views.  win = (netvlad [n][V][G], desc [n][V][cap][D], n_kp [n][V]) oldest first, rem the
    same for the nq remote frames.  Returns (sims [nq][n][V] in dirs order, records)."""
    torch, dev = _torch()
    wnv, wdesc, wnk = win
    rnv, rdesc, rnk = rem
    n, nq, V, G = len(wnv), len(rnv), rnv.shape[1], rnv.shape[2]
    sims = np.zeros((nq, n, V), np.float32)
    chosen = [None] * nq
    if n:
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        d_w, d_r = t(wnv.reshape(n * V, G)), t(rnv.reshape(nq * V, G))
        d_rem_rows = t(np.arange(nq, dtype=np.int32) * V)
        for pos in range(n - 1, -1, -1):
            d_loc_rows = t(np.full(nq, pos * V, np.int32))
            d_s = torch.zeros((nq, V), dtype=torch.float32, device=dev); d_p = torch.full((nq,), -7, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            if V == 1:      # q = the local keyframe, db = the remote frame, as the stereo exchange calls it
                fe.gate_pairs_device(d_w.data_ptr(), G, d_r.data_ptr(), G, G, d_loc_rows.data_ptr(), d_rem_rows.data_ptr(), nq, thres, d_pass=d_p.data_ptr(), d_sims=d_s.data_ptr())
            else:
                fe.quad_gate_device(d_w.data_ptr(), G, d_r.data_ptr(), G, G, d_loc_rows.data_ptr(), d_rem_rows.data_ptr(), 1, 1, nq, thres, d_dir_prev=d_p.data_ptr(),
                                    d_sims=d_s.data_ptr())
            fe.sync(); torch.cuda.synchronize()
            s, p = d_s.cpu().numpy(), d_p.cpu().numpy()
            sims[:, pos] = s
            for q in range(nq):
                ok = int(p[q]) == 1 if V == 1 else int(p[q]) >= 0
                if chosen[q] is None and ok:
                    chosen[q] = (pos, int(p[q]) if V == 4 else 0)
    recs = []
    for q in range(nq):
        if chosen[q] is None:
            recs.append(None)
            continue
        pos, dir_b = chosen[q]
        views = api.window_views(V, dir_b)
        j = kw.DIRS.index(dir_b) if V == 4 else 0
        recs.append(dict(pos=pos, dir_a=2 if V == 4 else 0, dir_b=dir_b, sim=sims[q, pos, j], views=views,
                         matches=[_match(fe, mode, wdesc[pos, lv, :wnk[pos, lv]], rdesc[q, rv, :rnk[q, rv]]) for rv, lv in views]))
    return sims, recs


def _check(r, sims, recs, tags, V):
    """every collected field against the composition; returns (hits, misses)"""
    nq, n, K = len(recs), len(tags), r["capacity"]
    assert r["nq"] == nq and r["views"] == V and r["cap"] == CAP and r["n_window"] == n
    assert np.array_equal(_bits(r["sims"][:, :n]), _bits(sims)) and not _bits(r["sims"][:, n:]).any()
    assert r["sims"].shape == (nq, K, V)
    hits = 0
    for q, rec in enumerate(recs):
        if rec is None:
            assert int(r["keyframe_tag"][q]) == -1 and int(r["keyframe_pos"][q]) == -1 and int(r["dir_a"][q]) == -1 and int(r["dir_b"][q]) == -1
            assert _bits(r["sim"][q:q + 1])[0] == 0 and not r["n_match"][q].any() and np.all(r["local_view"][q] == -1) and np.all(r["remote_view"][q] == -1)
            continue
        hits += 1
        assert int(r["keyframe_pos"][q]) == rec["pos"] and int(r["keyframe_tag"][q]) == tags[rec["pos"]], (q, int(r["keyframe_pos"][q]), rec["pos"])
        assert (int(r["dir_a"][q]), int(r["dir_b"][q])) == (rec["dir_a"], rec["dir_b"])
        assert _bits(r["sim"][q:q + 1])[0] == _bits(np.float32(rec["sim"]).reshape(1))[0]
        for i, (rv, lv) in enumerate(rec["views"]):
            assert (int(r["remote_view"][q, i]), int(r["local_view"][q, i])) == (rv, lv)
            mq, mt, md = rec["matches"][i]
            m = int(r["n_match"][q, i])
            assert m == len(mq) and np.array_equal(r["q_idx"][q, i, :m], mq) and np.array_equal(r["t_idx"][q, i, :m], mt), (q, i, m, len(mq))
            assert np.array_equal(_bits(r["dist"][q, i, :m]), _bits(md))
    return hits, nq - hits


def _same(a, b):
    """two collected results, field by field, bit by bit (match lists up to their counts)"""
    assert sorted(a) == sorted(b)
    for k in a:
        if k in ("q_idx", "t_idx", "dist"):
            for q in range(a["nq"]):
                for i in range(a["views"]):
                    m = int(a["n_match"][q, i])
                    assert np.array_equal(_bits(a[k][q, i, :m]), _bits(b[k][q, i, :m])), k
        elif isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
        elif k != "phase_ms":
            assert a[k] == b[k], k


def _fill(win, w, tags, scramble, rng, V, G):
    """the window's keyframes through push_host, oldest first; scramble (five keyframes): push 5, retain 2 of them, push 3 more, so that slot order and age differ"""
    wnv, wdesc, wnk = w
    n = len(wnv)
    if not scramble:
        for k in range(n):
            win.push_host(wnv[k], wdesc[k], wnk[k], tags[k])
        return
    assert n == 5
    junk = lambda: (kw.unit_rows(rng.randn(V, G)), kw.unit_rows(rng.randn(V, CAP, D)), np.full(V, CAP, np.int32))
    for tag, k in ((900, None), (tags[0], 0), (901, None), (902, None), (tags[1], 1)):
        a = junk() if k is None else (wnv[k], wdesc[k], wnk[k])
        win.push_host(a[0], a[1], a[2], tag)
    assert win.retain([tags[0], tags[1], 555]) == 3 and win.tags() == [tags[0], tags[1]]
    for k in (2, 3, 4):
        win.push_host(wnv[k], wdesc[k], wnk[k], tags[k])


def _track_dense(win, rem, slot, stream=None, misalign=False):
    """misalign: NetVLAD rows that start 4 bytes past a 16-byte boundary, G + 1 words apart (what a gathered block's rows are like when cap % 4 != 0), and counts
    3 words apart"""
    torch, dev = _torch()
    rnv, rdesc, rnk = rem
    nq, V, G = rnv.shape
    nv_s, nk_s, lead = (G + 1, 3, 1) if misalign else (G, 1, 0)
    nvb = np.zeros(lead + nq * V * nv_s, np.float32); nkb = np.full(nq * V * nk_s, -9, np.int32)
    nvb[lead:].reshape(nq * V, nv_s)[:, :G] = rnv.reshape(nq * V, G); nkb[::nk_s] = rnk.reshape(-1)
    d = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (nvb, rdesc, nkb)]
    torch.cuda.synchronize()
    assert d[0].data_ptr() % 16 == 0
    win.track_device(d[0].data_ptr() + 4 * lead, nv_s, d[1].data_ptr(), CAP * D, d[2].data_ptr(), nk_s, nq, slot, stream)
    r = _copy(win.collect(slot))
    del d
    return r


# ---- (a) the query on its own -----------------------------------------------------------------------------------------------------------------------------
# G = 64 (PCA) leaves most lanes of a wave without elements, 1024 gives every lane one float4, 4096 four of them
@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("V", [1, 4])
@pytest.mark.parametrize("G", [64, 1024, 4096])
def test_track_device_against_the_oracle_and_the_existing_calls(orc, G, V, mode):
    api, fe, pipe = _pipe(V, pca=0 if G == 4096 else G)
    assert fe.netvlad_dim == G
    K = 7
    hits = misses = newer_wins = dirs_wins = empty_side = 0
    for n in (0, 1, 5, K):
        rng = np.random.RandomState(7 * G + 10 * V + n)
        w = kw.make_window(rng, n, V, G, CAP)
        tags = [1000 + 3 * k for k in range(n)]
        win = api.KeyframeWindow(pipe, capacity=K, thres=kw.THRES, ratio=RATIO, mode=mode, slots=2, max_queries=33)
        _fill(win, w, tags, n == 5, rng, V, G)
        assert len(win) == n and win.tags() == tags
        p = kw.plant(n, V)
        for nq in (1, 5, 33):
            rem = kw.make_remote(rng, nq, w, V, G, CAP)
            s64 = kw.sims64(rem[0], w[0], V)
            assert s64.size == 0 or np.abs(s64 - kw.THRES).min() >= 1e-3      # every similarity, none left out
            r = _track_dense(win, rem, nq % 2)
            if nq == 5:
                _same(r, _track_dense(win, rem, 0, misalign=True))      # unaligned rows: four scalar loads, the same bits
            sims, recs = _compose(api, fe, w, rem, kw.THRES, mode)
            h, m = _check(r, sims, recs, tags, V)
            hits += h; misses += m
            for q in range(nq):
                want = kw.expected(orc, spref, rem[0][q], rem[2][q], w, V, kw.THRES)
                assert (want is None) == (int(r["keyframe_pos"][q]) < 0), (n, nq, q)
                if want is None:
                    continue
                assert (int(r["keyframe_pos"][q]), int(r["dir_a"][q]), int(r["dir_b"][q])) == (want["pos"], want["dir_a"], want["dir_b"]), (n, nq, q)
                print("G %d V %d n %d nq %d q %d: sim %.7f oracle %.7f" % (G, V, n, nq, q, float(r["sim"][q]), want["sim"]))
                assert abs(float(r["sim"][q]) - want["sim"]) <= 2e-5
                pos = want["pos"]
                got = [(int(r["remote_view"][q, i]), int(r["local_view"][q, i])) for i in range(V)]
                both = [(a, b) for a, b in got if int(rem[2][q, a]) > 0 and int(w[2][pos, b]) > 0]
                assert both == want["pairs"], (n, nq, q)
                empty_side += len(both) < V
                for i, (a, b) in enumerate(got):
                    if (a, b) not in both:
                        assert int(r["n_match"][q, i]) == 0      # the problem keeps its place
                # the two planted orders, wherever no NEWER keyframe passes by chance (unrelated vectors of 64 floats reach 0.5 now and then)
                if q % 6 == 0 and p["new"] is not None and not (s64[q, p["new"] + 1:] >= kw.THRES).any():
                    j = kw.DIRS.index(want["dir_b"]) if V == 4 else 0
                    assert pos == p["new"] and float(r["sims"][q, p["old"], j]) > float(r["sim"][q]) + 0.1      # the newer keyframe merely passes -- and wins
                    newer_wins += 1
                if q % 6 == 1 and p["dup"] is not None and not (s64[q, p["dup"] + 1:] >= kw.THRES).any() and s64[q, p["dup"], 0] < kw.THRES:
                    assert pos == p["dup"] and want["dir_b"] == 3 and float(r["sims"][q, pos, 2]) > float(r["sims"][q, pos, 1]) > kw.THRES      # dirs order wins
                    dirs_wins += 1
        win.close()
    assert hits >= 1 and misses >= 1 and newer_wins >= 1 and empty_side >= 1 and (dirs_wins >= 1 or V == 1)
    pipe.close(); fe.close()


# ---- (b) the threshold itself ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("V", [1, 4])
def test_a_similarity_equal_to_the_threshold_passes(orc, V):
    """integer-valued vectors (tests/test_side_kernels_edges.py): every summation order is exact.  8.0 against 8.0 is accepted, and refused one float ulp above"""
    G = 1024
    api, fe, pipe = _pipe(V, pca=G)
    idx = [0, 7, 300, 1023]                                   # different lanes, different chunks
    wnv = np.zeros((2, V, G), np.float32); rnv = np.zeros((2, V, G), np.float32)
    wnv[0, 1 if V == 4 else 0, idx] = [1, 2, 1, 2]            # quad: view 1, the LAST of dirs
    wnv[1, 0, idx] = [1, 1, 1, 1]                             # the newer keyframe reaches 6
    gv = 2 if V == 4 else 0
    rnv[0, gv, idx] = [2, 1, 2, 1]                            # 2 + 2 + 2 + 2 = 8 with keyframe 0
    rnv[1, gv, idx] = [2, 1, 2, 0]                            # 6
    rng = np.random.RandomState(3)
    wdesc = kw.unit_rows(rng.randn(2, V, CAP, D)); rdesc = kw.unit_rows(rng.randn(2, V, CAP, D))
    wnk = np.full((2, V), CAP, np.int32); rnk = np.full((2, V), CAP, np.int32)
    above = float(np.nextafter(np.float32(8.0), np.float32(9.0)))
    for thres, hit in ((8.0, True), (above, False)):
        o = orc.tracker_gate(rnv[0], wnv, thres, V == 4)
        assert (o is not None) == hit
        win = api.KeyframeWindow(pipe, capacity=2, thres=thres, ratio=RATIO, slots=1, max_queries=2)
        for k in range(2):
            win.push_host(wnv[k], wdesc[k], wnk[k], 50 + k)
        r = _track_dense(win, (rnv, rdesc, rnk), 0)
        j = V - 1
        assert float(r["sims"][0, 0, j]) == 8.0 and float(r["sims"][1, 0, j]) == 6.0
        assert int(r["keyframe_pos"][1]) == -1
        if hit:
            assert int(r["keyframe_pos"][0]) == 0 == o["kf"] and int(r["keyframe_tag"][0]) == 50 and float(r["sim"][0]) == 8.0
            assert int(r["dir_b"][0]) == (1 if V == 4 else 0) == o["dir_b"]
        else:
            assert int(r["keyframe_pos"][0]) == -1 and int(r["keyframe_tag"][0]) == -1
        win.close()
    pipe.close(); fe.close()


# ---- (c) behind the pipes -------------------------------------------------------------------------------------------------------------------------------------
def _submits(V):
    """8 submits: stereo 2 frames each (the loop tests' sequence, a scene seen before comes back with fresh noise; one black frame), quad 1 quad each (the rig turned
    by r quarter turns; the last one black)"""
    if V == 1:
        from tests.test_loop_query import _stereo_frames
        fr = _stereo_frames()
        return [(np.stack([fr[2 * i][0], fr[2 * i + 1][0]]), np.stack([fr[2 * i][1], fr[2 * i + 1][1]])) for i in range(8)]
    from tests.helpers import quad_exchange_common as qc
    out = [(np.stack(qc.raw_views(i % 4, i))[None],) for i in range(8)]
    out[7] = (np.zeros_like(out[7][0]),)
    return out


def _frames_of(o, V):
    """[(netvlad [V][G], desc [V][cap][D], n_kp [V])] of the frames of one waited ticket"""
    if V == 4:
        return [(o["netvlad"][q], o["desc"][q], o["n_kp"][q]) for q in range(o["n_kp"].shape[0])]
    F = o["netvlad"].shape[0]
    return [(o["netvlad"][k][None], o["desc"][k][None], o["n_kp"][k:k + 1]) for k in range(F)]


def _stack(frames):
    return tuple(np.stack([f[i] for f in frames]) for i in range(3))


def _copy_cb():
    from tests.helpers import quad_exchange_common as qc
    hip = qc.hip()

    def gather(user, d_send, d_recv, nbytes, stream):      # world = 1: the gathered buffer IS the rank's blocks
        return int(hip.hipMemcpyAsync(C.c_void_p(d_recv), C.c_void_p(d_send), C.c_size_t(nbytes), 3, C.c_void_p(stream)))
    return gather


@pytest.mark.gpu
@pytest.mark.parametrize("V", [1, 4])
def test_window_behind_a_pipe_equals_the_host_composition(V):
    from tests.helpers import quad_exchange_common as qc
    api, fe, pipe = _pipe(V, lanes=2, n=2 if V == 1 else 1)
    G, F = fe.netvlad_dim, 2 if V == 1 else 1
    subs = _submits(V)
    NK = 4                                                     # tickets 0 .. 3 become keyframes, 4 .. 7 are tracked
    alone = []
    for s in subs:
        alone.append(_copy(pipe.wait(pipe.submit(*s))))
    pipe.close()
    # the window the bookkeeping below leaves, and a threshold in the widest gap of the remote frames' best similarities
    kf_frames = [f for o in alone[:NK] for f in _frames_of(o, V)]
    all_tags = [10 + 7 * t for t in range(len(kf_frames))]
    first = all_tags[:3 * F]                                   # what tickets 0 .. 2 pushed: the retain comes behind ticket 2
    keep = [first[0], first[-1]] if V == 1 else [first[0]]
    model = [t for t in first if t in keep or t == first[-1]] + all_tags[3 * F:]
    assert len(model) < len(first) + F
    w = _stack([kf_frames[all_tags.index(t)] for t in model])
    rem_all = _stack([f for o in alone[NK:] for f in _frames_of(o, V)])
    best = np.sort(kw.sims64(rem_all[0], w[0], V).reshape(len(rem_all[0]), -1).max(axis=1))
    g = int(np.argmax(np.diff(best)))
    thres = float(0.5 * (best[g] + best[g + 1]))
    print("V %d: best similarities %s, threshold %.4f" % (V, np.round(best, 4).tolist(), thres))
    pipe = _mk_pipe(api, fe, V, 2, F)
    win = api.KeyframeWindow(pipe, capacity=len(first), thres=thres, ratio=RATIO, slots=3, max_queries=2 * F)
    hits = misses = 0
    for i, s in enumerate(subs):
        t = pipe.submit(*s)
        if i < NK:
            for k in range(F):
                win.push(t, k, all_tags[i * F + k])
            win.push(t, F - 1, all_tags[i * F + F - 1])        # the newest tag again: a no-op
            if i == 2:
                assert win.retain(keep + [12345]) == len(first) - len([x for x in first if x in keep or x == first[-1]])
            o = _copy(pipe.wait(t))
        else:
            v = pipe.device_view(t, win.stream)               # read in place, in the lane's result block
            win.track_device(v.d_netvlad, G, v.d_desc, CAP * D, v.d_n_kp, 1, F, 0, None)
            pipe.device_release(t, win.stream)
            o = _copy(pipe.wait(t))
            r_view = _copy(win.collect(0))
            rem = _stack(_frames_of(o, V))
            r_dense = _track_dense(win, rem, 1)
            _same(r_view, r_dense)
            sims, recs = _compose(api, fe, w, rem, thres, 0)
            h, m = _check(r_view, sims, recs, model, V)
            hits += h; misses += m
        for k in o:                                            # the pipe's own results do not notice the consumer
            assert (o[k] is None and alone[i][k] is None) or np.array_equal(_bits(o[k]), _bits(alone[i][k])), k
    assert win.tags() == model and hits >= 1 and misses >= 1
    # one-rank loopback exchanges: the gathered blocks read in place against dense copies of the same blocks' fields
    BLK = api.block_words(CAP, G)
    off = {k: api.block_field_offset(CAP, G, k) for k in ("desc", "netvlad", "n")}
    for wire in ("fp32", "int8"):
        x = (api.Exchange(pipe, world=1, loopback=True, wire=wire, slots=2, own_stream=True, all_gather=_copy_cb()) if V == 1 else
             api.QuadExchange(pipe, world=1, loopback=True, wire=wire, mode="gated", slots=2, own_stream=True, all_gather=_copy_cb()))
        t = pipe.submit(*subs[2])
        x.enqueue(t, 1)
        nq = win.track_exchange(x, 1, 2) if V == 1 else win.track_quad_exchange(x, 1, 2)
        assert nq == F
        pipe.wait(t); x.collect(1)
        r_blocks = _copy(win.collect(2))
        blocks = qc.d2h(x.gathered(1)[0], 4 * BLK * F * V).view(np.float32).reshape(F, V, BLK)
        rem = (blocks[:, :, off["netvlad"]:off["netvlad"] + G].copy(), blocks[:, :, :CAP * D].reshape(F, V, CAP, D).copy(),
               blocks[:, :, off["n"]].copy().view(np.int32))
        r_dense = _track_dense(win, rem, 0)
        _same(r_blocks, r_dense)
        sims, recs = _compose(api, fe, w, rem, thres, 0)
        h, _ = _check(r_blocks, sims, recs, model, V)
        assert h >= 1                                          # ticket 2's frames are in the window themselves
        x.close()
    win.close(); pipe.close(); fe.close()


# ---- (d) refusals -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_window_refusals_leave_the_window_unchanged():
    api, fe = _stereo_fe(2)
    plain = api.StereoPipe(fe, lanes=2, frames=1, width=W, height=H, cap=CAP, netvlad=False)
    with pytest.raises(api.D2FEError, match="NetVLAD") as e:                   # a pipe without NetVLAD
        api.KeyframeWindow(plain)
    assert e.value.code == -1
    plain.close()
    pipe = api.StereoPipe(fe, lanes=2, frames=1, width=W, height=H, cap=CAP, netvlad=True)
    for bad in (dict(capacity=0), dict(capacity=65), dict(slots=0), dict(mode=2), dict(max_queries=0), dict(max_queries=257)):
        with pytest.raises(api.D2FEError, match="bad window configuration"):
            api.KeyframeWindow(pipe, **bad)
    G = fe.netvlad_dim
    win = api.KeyframeWindow(pipe, capacity=3, thres=0.5, slots=2, max_queries=2)
    rng = np.random.RandomState(1)
    w = kw.make_window(rng, 3, 1, G, CAP)
    rem = kw.make_remote(rng, 2, w, 1, G, CAP)
    from tests.test_loop_query import _stereo_frames
    fr = _stereo_frames()
    t0 = pipe.submit(fr[0][0][None], fr[0][1][None])
    win.push_host(w[0][0], w[1][0], w[2][0], 5)
    win.push(t0, 0, 6)
    state = lambda: (len(win), win.tags())
    assert state() == (2, [5, 6])
    win.push(t0, 0, 6); win.push_host(w[0][1], w[1][1], w[2][1], 6)          # the newest tag again: a no-op, not a refusal
    assert state() == (2, [5, 6])
    for push in (lambda tag: win.push(t0, 0, tag), lambda tag: win.push_host(w[0][1], w[1][1], w[2][1], tag)):
        with pytest.raises(api.D2FEError, match="already") as e:              # a duplicate tag
            push(5)
        assert e.value.code == -1 and state() == (2, [5, 6])
        with pytest.raises(api.D2FEError) as e:                               # a negative tag
            push(-1)
        assert e.value.code == -1 and state() == (2, [5, 6])
    with pytest.raises(api.D2FEError) as e:                                    # a frame the ticket does not have
        win.push(t0, 1, 7)
    assert e.value.code == -1 and state() == (2, [5, 6])
    win.push_host(w[0][2], w[1][2], w[2][2], 7)
    for push in (lambda: win.push(t0, 0, 8), lambda: win.push_host(w[0][1], w[1][1], w[2][1], 8)):
        with pytest.raises(api.D2FEError, match="full") as e:                  # a full window
            push()
        assert e.value.code == -4 and state() == (3, [5, 6, 7])
    pipe.wait(t0)
    torch, dev = _torch()
    d = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (rem[0], rem[1], rem[2])]
    torch.cuda.synchronize()
    args = lambda nq, slot: (d[0].data_ptr(), G, d[1].data_ptr(), CAP * D, d[2].data_ptr(), 1, nq, slot)
    with pytest.raises(api.D2FEError) as e:                                    # collect before anything was queued
        win.collect(0)
    assert e.value.code == -1
    with pytest.raises(api.D2FEError, match="max_queries") as e:               # nq > max_queries
        win.track_device(*args(3, 0))
    assert e.value.code == -1 and state() == (3, [5, 6, 7])
    with pytest.raises(api.D2FEError, match="stride"):
        win.track_device(d[0].data_ptr(), G - 4, d[1].data_ptr(), CAP * D, d[2].data_ptr(), 1, 2, 0)
    win.track_device(*args(2, 0))
    with pytest.raises(api.D2FEError, match="not been collected") as e:        # a busy slot
        win.track_device(*args(2, 0))
    assert e.value.code == -3 and state() == (3, [5, 6, 7])
    a = _copy(win.collect(0))
    assert win.retain([7]) == 2 and state() == (1, [7]) and win.retain([]) == 0 and win.retain([1, 2]) == 0
    win.track_device(*args(2, 1))                                              # the refusals queued nothing: the slots still work
    b = win.collect(1)
    assert a["n_window"] == 3 and b["n_window"] == 1 and np.array_equal(_bits(a["sims"][:, 2]), _bits(b["sims"][:, 0]))
    for t in range(1, 7):                                                      # 2 * lanes + 2 more passes: a view left unreleased by a refusal would refuse one of these
        pipe.wait(pipe.submit(fr[t][0][None], fr[t][1][None]))
    win.close(); pipe.close(); fe.close()


# ---- (e) an older caller's shorter configuration struct --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_config_cut_short_by_struct_size_keeps_the_defaults_behind_it():
    """d2fe_window_create copies min(struct_size, sizeof) bytes of the caller's struct over the defaults: a caller whose struct ends in front of `slots` gets the
    default four slots, whatever lies in the memory behind its struct (here slots = 0, which a full-size struct is refused for)."""
    api, fe = _stereo_fe(2)
    pipe = api.StereoPipe(fe, lanes=2, frames=1, width=W, height=H, cap=CAP, netvlad=True)
    lib = pipe._lib
    c = api._WindowConfig()
    lib.d2fe_window_default_config(C.byref(c))
    c.slots = 0
    x = C.c_void_p()
    with pytest.raises(api.D2FEError, match="bad window configuration"):      # the whole struct is read: slots = 0 is refused
        api._check(lib.d2fe_window_create(pipe._p, C.byref(c), C.byref(x)))
    assert not x.value
    c.struct_size = api._WindowConfig.slots.offset                             # the struct of a caller that does not know `slots`
    api._check(lib.d2fe_window_create(pipe._p, C.byref(c), C.byref(x)))
    res = api._WindowResult()
    with pytest.raises(api.D2FEError, match="nothing was queued"):            # slot 3 exists: four slots
        api._check(lib.d2fe_window_collect(x, 3, C.byref(res)))
    with pytest.raises(api.D2FEError, match="bad argument"):                  # slot 4 does not
        api._check(lib.d2fe_window_collect(x, 4, C.byref(res)))
    lib.d2fe_window_destroy(x)
    pipe.close(); fe.close()
