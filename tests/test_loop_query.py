"""The loop query behind the pipes (d2fe_loop_*; include/d2fe.h, csrc/loop.hip): LoopDetector::processImageArray (loop_detector.cpp:23-215) as one launch
sequence per ticket over a device-resident keyframe store.
  (a) d2fe_loop_query_device on its own: synthetic unit vectors with planted near-copies against the oracle's gate, bitwise against d2fe_db_query_gated
      and d2fe_match_knn / d2fe_match_crosscheck;
  (b) behind a stereo pipe, (c) behind a quad pipe: every collected field bitwise against the host composition of the existing calls, frame by frame in causal
      order: d2fe_pipe_wait -> d2fe_db_query_gated -> d2fe_match_knn -> d2fe_db_add;
  (d) the refusals, each leaving the store as it was;
  (e) a configuration struct cut short by its struct_size.
The caller-side precondition of the reference, databaseSize() > match_index_dist (:157), is part of the query on both sides."""
import ctypes as C

import numpy as np
import pytest

from d2slam_amd.synth import synth_stereo
from d2slam_amd.weights import synthetic_superpoint_weights

H, W, CAP = 120, 160, 60
RATIO = 0.8


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _unit_rows(a):
    a = np.asarray(a, np.float32)
    return (a / np.linalg.norm(a, axis=-1, keepdims=True)).astype(np.float32)


def _stereo_fe(max_batch, netvlad=True, pca=0, cap=CAP):
    from d2slam_amd import api, netvlad as nvm
    fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=cap, input_width=W, input_height=H, max_batch=max_batch, precision=api.PREC_F32_WINO))
    fe.load_superpoint(synthetic_superpoint_weights(dustbin_bias=7.5))
    if netvlad:
        # the 0.35-wide trunk: its seeded random weights tell scenes apart by a wider margin than the default's (tests/helpers/quad_swarm_worker.py)
        fe.load_netvlad(nvm.synthetic_netvlad_weights(depth_multiplier=0.35))
        if pca:
            fe.set_netvlad_pca(*nvm.synthetic_netvlad_pca(out_dims=pca))
    return api, fe


def _match(api, fe, mode, a, b):
    """(q, t, d) of the existing host calls; an empty side gives no matches (loop_detector.cpp:470-471)"""
    if len(a) == 0 or len(b) == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)
    return fe.match_knn(a, b, RATIO) if mode == 0 else fe.match_crosscheck(a, b)


# ---- (a) the query on its own ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
# the last case: more rows than one pass of the resident grid takes (16 rows per workgroup, one workgroup per compute unit at this length), so workgroups stride
@pytest.mark.parametrize("dim,mode,max_index,cap,ntotals", [(64, 1, 0, CAP, (0, 3, 9, 1027)), (1024, 0, 2, CAP, (0, 3, 9, 1027)), (4096, 0, 2, CAP, (0, 3, 9, 1027)),
                                                            (1024, 0, 2, 8, (4099,))])
def test_query_device_against_the_oracle_and_the_existing_calls(orc, dim, mode, max_index, cap, ntotals):
    import torch
    api, fe = _stereo_fe(2, pca=0 if dim == 4096 else dim, cap=cap)
    assert fe.netvlad_dim == dim
    pipe = api.StereoPipe(fe, lanes=1, frames=1, width=W, height=H, cap=cap, netvlad=True)
    thres, D = 0.5, 256
    dev = torch.device("cuda", 0)
    for ntotal in ntotals:      # 1027: not a multiple of the 16 rows a workgroup takes per step, and more than one workgroup
        rng = np.random.RandomState(dim + ntotal)
        vec = _unit_rows(rng.randn(max(ntotal, 1), dim))[:ntotal]
        kdesc = _unit_rows(rng.randn(max(ntotal, 1), cap, D))[:ntotal]
        kn = rng.randint(max(cap // 3, 2), cap + 1, size=ntotal).astype(np.int32)
        loop = api.LoopQuery(pipe, capacity_keyframes=max(ntotals) + 8, max_index=10, thres=thres, ratio=RATIO, mode=mode, slots=2, max_queries=33)
        db = api.FlatIPDatabase(fe, dim, capacity=max(ntotals) + 8)
        if ntotal:
            assert loop.add_host(vec[:, None], kdesc[:, None], kn[:, None]) == 0
            db.add(vec)
        assert loop.ntotal == ntotal == db.ntotal and loop.keyframes == ntotal
        for nq in (1, 5, 33):           # 5 x 4096 floats: beyond what one d2fe_db_search call stages
            q = np.empty((nq, dim), np.float32); qdesc = np.empty((nq, cap, D), np.float32); qn = rng.randint(max(cap // 3, 2), cap + 1, size=nq).astype(np.int32)
            for j in range(nq):
                if ntotal and j % 4 != 3:      # a near-copy of a stored row (tests/test_ref_pin.py's planting): first, middle, the last allowed, the last rows
                    t = (0, ntotal // 2, max(ntotal - max_index, 0), ntotal - 1, int(rng.randint(ntotal)))[j % 5]
                    t = min(t, ntotal - 1)
                    q[j] = _unit_rows(vec[t] + (0.3 / np.sqrt(dim)) * rng.randn(dim).astype(np.float32))
                    qdesc[j] = _unit_rows(kdesc[t][rng.permutation(cap)] + 0.05 * rng.randn(cap, D).astype(np.float32))
                else:                          # an unrelated frame
                    q[j] = _unit_rows(rng.randn(dim)); qdesc[j] = _unit_rows(rng.randn(cap, D))
            if nq >= 5:
                qn[4] = 0                      # a frame whose main view has no keypoints is not queried (:378)
            d_q, d_d, d_n = (torch.from_numpy(x).to(dev) for x in (q, qdesc, qn))
            torch.cuda.synchronize()
            loop.query_device(d_q.data_ptr(), d_d.data_ptr(), d_n.data_ptr(), nq, max_index, 0)
            r = loop.collect(0)
            assert r["ticket"] == -1 and r["frames"] == nq and r["views"] == 1
            hits = 0
            for j in range(nq):
                queried = int(qn[j]) > 0 and ntotal > max_index
                assert int(r["queried"][j]) == int(queried) and int(r["ntotal_at_query"][j]) == ntotal
                if queried:
                    ol, osim = orc.db_query(vec, q[j], max_index, thres)[:2]
                    hl, hs = db.query_gated(q[j], max_index, thres)
                else:
                    ol, osim, hl, hs = -1, 0.0, -1, 0.0
                label = int(r["label"][j])
                assert label == ol == hl, (ntotal, nq, j, label, ol, hl)
                assert int(r["added_label"][j, 0]) == -1
                if label < 0:
                    assert float(r["sim"][j]) == 0.0 and int(r["keyframe"][j]) == int(r["dir_old"][j]) == int(r["dir_a"][j, 0]) == int(r["dir_b"][j, 0]) == -1
                    assert int(r["n_match"][j, 0]) == 0
                    continue
                hits += 1
                assert abs(float(r["sim"][j]) - float(osim)) <= 2e-5
                assert _bits(r["sim"][j:j + 1])[0] == _bits(np.float32(hs).reshape(1))[0]
                assert int(r["keyframe"][j]) == label and int(r["dir_old"][j]) == 0 and (int(r["dir_a"][j, 0]), int(r["dir_b"][j, 0])) == (0, 0)
                mq, mt, md = _match(api, fe, mode, qdesc[j, :qn[j]], kdesc[label, :kn[label]])
                n = int(r["n_match"][j, 0])
                assert n == len(mq) and np.array_equal(r["q_idx"][j, 0, :n], mq) and np.array_equal(r["t_idx"][j, 0, :n], mt)
                assert np.array_equal(_bits(r["dist"][j, 0, :n]), _bits(md))
            if ntotal > max_index:
                assert hits >= 1
            assert loop.ntotal == ntotal and loop.keyframes == ntotal      # a query adds nothing
        loop.close(); db.close()
    pipe.close(); fe.close()


# ---- the host composition -------------------------------------------------------------------------------------------------------------------------------------
def _compose(api, fe, frames, flags, V, main_dir, max_index, mode, G):
    """frames[t] = (netvlad [V][G], desc [V][cap][D], n_kp [V]) as the pipe returned them; flags[t]: LOOP_QUERY | LOOP_ADD bits.  The existing calls, frame by frame in
    causal order, with the gate threshold left open: per frame the best allowed row and its similarity, and what the add did."""
    db = api.FlatIPDatabase(fe, G, capacity=4 * len(frames) + 4)
    row_kf, row_dir, store, out = [], [], [], []
    for (nv, desc, n_kp), fl in zip(frames, flags):
        nt = db.ntotal
        rec = dict(ntotal=nt, queried=int(bool(fl & api.LOOP_QUERY) and int(n_kp[main_dir]) > 0 and nt > max_index), label=-1, sim=np.float32(0), added=[-1] * V)
        if rec["queried"]:
            rec["label"], s = db.query_gated(nv[main_dir], max_index, -1e30)      # the best allowed row, whatever its similarity
            rec["sim"] = np.float32(s)
        if rec["label"] >= 0:
            kf, dir_old = row_kf[rec["label"]], row_dir[rec["label"]]
            rec.update(keyframe=kf, dir_old=dir_old, dirs=api.loop_dirs(V, main_dir, dir_old))
            kd, kn = store[kf]
            rec["matches"] = [_match(api, fe, mode, desc[a, :n_kp[a]], kd[b, :kn[b]]) for a, b in rec["dirs"]]
        if fl & api.LOOP_ADD:
            store.append((desc.copy(), n_kp.copy()))
            for v in range(V):
                if int(n_kp[v]) > 0:
                    rec["added"][v] = db.add(nv[v][None])
                    row_kf.append(len(store) - 1); row_dir.append(v)
        out.append(rec)
    db.close()
    return out


def _check_frame(r, f, rec, thres, V):
    """every collected field of frame f of a slot against the composition's record, under the threshold"""
    hit = rec["label"] >= 0 and float(rec["sim"]) > thres
    assert int(r["queried"][f]) == rec["queried"] and int(r["ntotal_at_query"][f]) == rec["ntotal"]
    assert [int(v) for v in r["added_label"][f]] == rec["added"]
    if not hit:
        assert int(r["label"][f]) == -1 and float(r["sim"][f]) == 0.0 and int(r["keyframe"][f]) == -1 and int(r["dir_old"][f]) == -1
        assert not r["n_match"][f].any() and np.all(r["dir_a"][f] == -1) and np.all(r["dir_b"][f] == -1)
        return False
    assert int(r["label"][f]) == rec["label"] and _bits(r["sim"][f:f + 1])[0] == _bits(rec["sim"].reshape(1))[0]
    assert int(r["keyframe"][f]) == rec["keyframe"] and int(r["dir_old"][f]) == rec["dir_old"]
    for i in range(V):
        assert (int(r["dir_a"][f, i]), int(r["dir_b"][f, i])) == rec["dirs"][i]
        mq, mt, md = rec["matches"][i]
        n = int(r["n_match"][f, i])
        assert n == len(mq) and np.array_equal(r["q_idx"][f, i, :n], mq) and np.array_equal(r["t_idx"][f, i, :n], mt)
        assert np.array_equal(_bits(r["dist"][f, i, :n]), _bits(md))
    return True


def _drive(api, pipe, submits, loop=None, masks=None, flags=None):
    """all submits through the pipe with `lanes` in flight; copies of every pipe result and, with a loop object, of every collected slot"""
    lanes = pipe.lanes
    tk, res, col = [], [], []

    def take():
        i = len(res)
        res.append({k: (None if v is None else v.copy()) for k, v in pipe.wait(tk[i]).items()})
        if loop is not None:
            c = loop.collect(i % loop.slots)
            assert c["ticket"] == tk[i]
            col.append({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.items()})
    for i, s in enumerate(submits):
        tk.append(pipe.submit(*s))
        if loop is not None:
            loop.enqueue(tk[i], i % loop.slots, masks[i], flags[i])
        if len(tk) - len(res) >= lanes:
            take()
    while len(res) < len(submits):
        take()
    return res, col


# ---- (b) behind a stereo pipe ---------------------------------------------------------------------------------------------------------------------------------
STEREO_SCENES = [0, 1, 2, 3, 0, 4, -1, 1, 5, 2, 6, 3, 0, 7, 4, 1]      # -1: an all-black frame; a scene seen before comes back with fresh noise
STEREO_KEY = [1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 0, 1, 1]         # is_keyframe


def _stereo_frames():
    out = []
    for t, s in enumerate(STEREO_SCENES):
        if s < 0:
            out.append((np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)))
            continue
        l, r = synth_stereo(H, W, seed=900 + s)
        rng = np.random.RandomState(40 + t)
        out.append((np.clip(l.astype(np.int16) + rng.randint(-2, 3, l.shape), 0, 255).astype(np.uint8), r))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("lanes,F", [(1, 1), (2, 2), (3, 4)])
def test_stereo_pipe_loop_query_equals_the_host_composition(lanes, F):
    api, fe = _stereo_fe(2 * F)
    G, MI = fe.netvlad_dim, 2
    fr = _stereo_frames()
    N = len(fr)
    assert N >= 14 and N % F == 0
    submits = [(np.stack([fr[i * F + k][0] for k in range(F)]), np.stack([fr[i * F + k][1] for k in range(F)])) for i in range(N // F)]
    masks = [np.array(STEREO_KEY[i * F:(i + 1) * F], np.uint8) for i in range(N // F)]
    flags = [api.LOOP_QUERY | api.LOOP_ADD] * len(submits)
    flags[-1] = api.LOOP_QUERY                                           # the last ticket only asks
    # the pipe alone, and the host composition on its results
    pipe = api.StereoPipe(fe, lanes=lanes, frames=F, width=W, height=H, cap=CAP, netvlad=True)
    alone, _ = _drive(api, pipe, submits)
    pipe.close()
    per_frame = [(o["netvlad"][k][None], o["desc"][k][None], o["n_kp"][k:k + 1]) for o in alone for k in range(F)]
    fl_frame = [(flags[i] if masks[i][k] else 0) for i in range(len(submits)) for k in range(F)]
    black = STEREO_SCENES.index(-1)
    assert int(per_frame[black][2][0]) == 0 and all(int(p[2][0]) > 10 for t, p in enumerate(per_frame) if t != black)
    comp = _compose(api, fe, per_frame, fl_frame, 1, 0, MI, 0, G)
    best = [float(c["sim"]) for c in comp if c["label"] >= 0]
    assert len(best) >= 6
    thres = float(np.median(best))                                      # from the composition's own similarities
    # the pipe with the loop object on every ticket
    pipe = api.StereoPipe(fe, lanes=lanes, frames=F, width=W, height=H, cap=CAP, netvlad=True)
    loop = api.LoopQuery(pipe, capacity_keyframes=N, max_index=MI, thres=thres, ratio=RATIO, mode=0, slots=lanes + 1, timing=True)
    with_loop, col = _drive(api, pipe, submits, loop, masks, flags)
    for a, b in zip(alone, with_loop):                                   # the pipe's own results do not notice the consumer
        assert sorted(a) == sorted(b)
        for k in a:
            assert (a[k] is None and b[k] is None) or np.array_equal(_bits(a[k]), _bits(b[k])), k
    passed = failed = 0
    for i, c in enumerate(col):
        assert c["frames"] == F and c["views"] == 1 and c["cap"] == CAP and len(c["phase_ms"]) == 4
        for k in range(F):
            rec = comp[i * F + k]
            hit = _check_frame(c, k, rec, thres, 1)
            passed += hit; failed += (rec["label"] >= 0 and not hit)
    assert passed >= 1 and failed >= 1
    assert comp[black]["added"] == [-1] and fl_frame[black] & api.LOOP_ADD      # the black keyframe holds an ordinal and no index row
    assert loop.keyframes == sum(1 for f in fl_frame if f & api.LOOP_ADD)
    assert loop.ntotal == sum(1 for c in comp for a in c["added"] if a >= 0) == loop.keyframes - 1
    loop.close(); pipe.close(); fe.close()


# a stationary camera: the same image array twice inside one ticket and again in later tickets.  Bit-identical NetVLAD rows tie exactly -- stored row against stored
# row, and stored row against a row the same ticket adds -- and every repeat reports the FIRST occurrence (similarity descending, then label ascending)
STATIONARY_SCENES = [0, 0, 1, 2, 0, 0, 1, 3]


@pytest.mark.gpu
def test_stereo_pipe_loop_query_stationary_camera_reports_the_first_occurrence():
    lanes, F, MI, thres = 2, 2, 0, 0.999
    api, fe = _stereo_fe(2 * F)
    G = fe.netvlad_dim
    base = {s: synth_stereo(H, W, seed=900 + s) for s in set(STATIONARY_SCENES)}
    fr = [base[s] for s in STATIONARY_SCENES]
    N = len(fr)
    submits = [(np.stack([fr[i * F + k][0] for k in range(F)]), np.stack([fr[i * F + k][1] for k in range(F)])) for i in range(N // F)]
    masks = [np.ones(F, np.uint8) for _ in submits]                      # every frame is a keyframe
    flags = [api.LOOP_QUERY | api.LOOP_ADD] * len(submits)
    pipe = api.StereoPipe(fe, lanes=lanes, frames=F, width=W, height=H, cap=CAP, netvlad=True)
    alone, _ = _drive(api, pipe, submits)
    pipe.close()
    per_frame = [(o["netvlad"][k][None], o["desc"][k][None], o["n_kp"][k:k + 1]) for o in alone for k in range(F)]
    first = [STATIONARY_SCENES.index(s) for s in STATIONARY_SCENES]
    for t in range(N):                                                   # the premise: a repeated frame's row is its first occurrence's, bit for bit
        assert int(per_frame[t][2][0]) > 10 and np.array_equal(_bits(per_frame[t][0]), _bits(per_frame[first[t]][0])), t
    comp = _compose(api, fe, per_frame, [flags[0]] * N, 1, 0, MI, 0, G)
    pipe = api.StereoPipe(fe, lanes=lanes, frames=F, width=W, height=H, cap=CAP, netvlad=True)
    loop = api.LoopQuery(pipe, capacity_keyframes=N, max_index=MI, thres=thres, ratio=RATIO, mode=0, slots=lanes + 1)
    _, col = _drive(api, pipe, submits, loop, masks, flags)
    repeats = 0
    for i, c in enumerate(col):
        for k in range(F):
            t = i * F + k
            hit = _check_frame(c, k, comp[t], thres, 1)
            assert int(c["added_label"][k, 0]) == t                      # no black frame: label == frame index
            if first[t] < t:
                repeats += 1
                assert hit and int(c["label"][k]) == int(c["keyframe"][k]) == first[t] == comp[t]["label"], (t, int(c["label"][k]), comp[t]["label"])
    assert repeats == 4 and loop.ntotal == loop.keyframes == N
    loop.close(); pipe.close(); fe.close()


# ---- (c) behind a quad pipe -------------------------------------------------------------------------------------------------------------------------------------
# (scene, quarter turns of the rig): a scene seen before comes back turned, so that the view the query sees (main_dir 2) is the stored keyframe's view 2 + turns
QUAD_SEQ = [(0, 0), (1, 0), (2, 0), (3, 0), (0, 0), (4, 0), (1, 1), (2, 2), (5, 0), (3, 3), (6, 0), (4, 1)]


def _quad_frames():
    from tests.helpers import quad_lk_ref as qref
    base = {}
    out = np.empty((len(QUAD_SEQ), 4, qref.H, qref.W), np.uint8)
    for t, (s, turn) in enumerate(QUAD_SEQ):
        if s not in base:
            base[s] = qref.cyclic_quads(1, 3100 + 17 * s)[0]
        rng = np.random.RandomState(70 + t)
        for c in range(4):
            v = base[s][(c + turn) % 4].astype(np.int16)
            out[t, c] = np.clip(v + rng.randint(-2, 3, v.shape), 0, 255).astype(np.uint8)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("lanes,Q", [(1, 1), (2, 2), (3, 4)])
def test_quad_pipe_loop_query_equals_the_host_composition(lanes, Q):
    from d2slam_amd import api, netvlad as nvm
    from tests.helpers import quad_lk_ref as qref
    from tests.test_quad_pipe import _weights
    QH, QW, MI = qref.H, qref.W, 2
    fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=CAP, input_width=QW, input_height=QH, max_batch=4 * Q, keypoint_threshold=0.15, precision=api.PREC_F32_WINO))
    fe.load_superpoint(_weights()); fe.load_netvlad(nvm.synthetic_netvlad_weights(depth_multiplier=0.35))
    G = fe.netvlad_dim
    frames = _quad_frames()
    N = len(frames)
    assert N % Q == 0
    submits = [(frames[i * Q:(i + 1) * Q],) for i in range(N // Q)]
    key = [1] * N
    key[5] = 0                                                           # scene 4's first visit is no keyframe: its second visit (frame 11) finds nothing of it
    masks = [np.array(key[i * Q:(i + 1) * Q], np.uint8) for i in range(N // Q)]
    flags = [api.LOOP_QUERY | api.LOOP_ADD] * len(submits)

    def mk():
        return api.QuadPipe(fe, qref.identity_maps(), lanes=lanes, quads=Q, raw_width=QW, raw_height=QH, width=QW, height=QH, cap=CAP, radius_neighbour=0.2 * QW,
                            undistort_fov=qref.FOV, netvlad=True, match_neighbour=False, match_prev=False)
    pipe = mk()
    alone, _ = _drive(api, pipe, submits)
    pipe.close()
    per_frame = [(o["netvlad"][q], o["desc"][q], o["n_kp"][q]) for o in alone for q in range(Q)]
    fl_frame = [(flags[i] if masks[i][q] else 0) for i in range(len(submits)) for q in range(Q)]
    comp = _compose(api, fe, per_frame, fl_frame, 4, 2, MI, 0, G)
    best = [float(c["sim"]) for c in comp if c["label"] >= 0]
    thres = float(np.median(best))
    pipe = mk()
    loop = api.LoopQuery(pipe, capacity_keyframes=N, max_index=MI, thres=thres, ratio=RATIO, mode=0, slots=lanes + 1)
    with_loop, col = _drive(api, pipe, submits, loop, masks, flags)
    for a, b in zip(alone, with_loop):
        for k in a:
            assert (a[k] is None and b[k] is None) or np.array_equal(_bits(a[k]), _bits(b[k])), k
    passed = failed = 0
    dirs = set()
    for i, c in enumerate(col):
        assert c["frames"] == Q and c["views"] == 4
        for q in range(Q):
            rec = comp[i * Q + q]
            hit = _check_frame(c, q, rec, thres, 4)                      # the four pairs of every hit
            passed += hit; failed += (rec["label"] >= 0 and not hit)
            if hit:
                dirs.add(int(c["dir_old"][q]))
                if QUAD_SEQ[i * Q + q][0] in [s for s, _ in QUAD_SEQ[:i * Q + q]] and QUAD_SEQ[i * Q + q][0] != 4:      # a stored scene seen again: its views match
                    turn = QUAD_SEQ[i * Q + q][1]
                    assert int(c["dir_old"][q]) == (2 + turn) % 4 and int(c["n_match"][q].min()) > 5
    assert passed >= 1 and failed >= 1
    assert dirs == {0, 1, 2, 3}, dirs                                   # every rotation of the direction table occurred
    assert loop.keyframes == N - 1 and loop.ntotal == sum(1 for c in comp for a in c["added"] if a >= 0)
    loop.close(); pipe.close(); fe.close()


# ---- (d) refusals -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_loop_query_refusals_leave_the_store_unchanged():
    api, fe = _stereo_fe(2)
    fr = _stereo_frames()
    order = [5, 0, 1, 2, 4] + list(range(6, 12))                                # ticket i carries frame order[i]: scene 0 is stored by ticket 1 and comes back with ticket 4
    sub = lambda p, i: p.submit(fr[order[i]][0][None], fr[order[i]][1][None])
    plain = api.StereoPipe(fe, lanes=2, frames=1, width=W, height=H, cap=CAP, netvlad=False)
    with pytest.raises(api.D2FEError, match="NetVLAD") as e:                   # a pipe without NetVLAD
        api.LoopQuery(plain)
    assert e.value.code == -1
    plain.close()
    pipe = api.StereoPipe(fe, lanes=2, frames=1, width=W, height=H, cap=CAP, netvlad=True)
    for bad in (dict(capacity_keyframes=0), dict(slots=0), dict(mode=2), dict(max_index=-1), dict(max_queries=0)):
        with pytest.raises(api.D2FEError, match="bad loop configuration"):
            api.LoopQuery(pipe, **bad)
    loop = api.LoopQuery(pipe, capacity_keyframes=3, max_index=0, thres=0.5, slots=2)
    state = lambda: (loop.keyframes, loop.ntotal)
    with pytest.raises(api.D2FEError) as e:                                    # collect before enqueue
        loop.collect(0)
    assert e.value.code == -1 and state() == (0, 0)
    t0, t1 = sub(pipe, 0), sub(pipe, 1)
    loop.enqueue(t1, 0)
    assert state() == (1, 1)
    with pytest.raises(api.D2FEError, match="submit order") as e:              # tickets out of order
        loop.enqueue(t0, 1)
    assert e.value.code == -1 and state() == (1, 1)
    with pytest.raises(api.D2FEError) as e:                                    # the same ticket again
        loop.enqueue(t1, 1)
    assert e.value.code == -1 and state() == (1, 1)
    t2 = sub(pipe, 2)
    with pytest.raises(api.D2FEError, match="not been collected") as e:        # a slot still in flight
        loop.enqueue(t2, 0)
    assert e.value.code == -3 and state() == (1, 1)
    with pytest.raises(api.D2FEError) as e:                                    # bad flags
        loop.enqueue(t2, 1, None, 4)
    assert e.value.code == -1 and state() == (1, 1)
    pipe.wait(t0); pipe.wait(t1)
    assert loop.collect(0)["ticket"] == t1
    loop.enqueue(t2, 0); pipe.wait(t2); loop.collect(0)
    t3 = sub(pipe, 3); loop.enqueue(t3, 1); pipe.wait(t3); loop.collect(1)
    assert state() == (3, 3)
    t4 = sub(pipe, 4)
    with pytest.raises(api.D2FEError, match="full") as e:                      # a full store: reported before anything is queued
        loop.enqueue(t4, 0)
    assert e.value.code == -4 and state() == (3, 3)
    with pytest.raises(api.D2FEError, match="full"):
        loop.add_host(np.zeros((1, 1, fe.netvlad_dim), np.float32), None, np.zeros((1, 1), np.int32))
    assert state() == (3, 3)
    loop.enqueue(t4, 0, None, api.LOOP_QUERY)                                  # asking still works
    pipe.wait(t4)
    r = loop.collect(0)
    assert int(r["queried"][0]) == 1 and int(r["ntotal_at_query"][0]) == 3 and int(r["added_label"][0, 0]) == -1 and state() == (3, 3)
    assert int(r["label"][0]) == int(r["keyframe"][0]) == 0 and int(r["n_match"][0, 0]) > 10      # scene 0, stored by ticket 1, seen again
    for t in range(5, 11):                                                     # 2 * lanes + 2 more passes: a view left unreleased by a refusal would refuse one of these submits
        pipe.wait(sub(pipe, t))
    loop.close(); pipe.close(); fe.close()


# ---- (e) an older caller's shorter configuration struct --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_config_cut_short_by_struct_size_keeps_the_defaults_behind_it():
    """d2fe_loop_create copies min(struct_size, sizeof) bytes of the caller's struct over the defaults: a caller whose struct ends in front of `slots` gets the
    default four slots, whatever lies in the memory behind its struct (here slots = 0, which a full-size struct is refused for)."""
    api, fe = _stereo_fe(2)
    pipe = api.StereoPipe(fe, lanes=2, frames=1, width=W, height=H, cap=CAP, netvlad=True)
    lib = pipe._lib
    c = api._LoopConfig()
    lib.d2fe_loop_default_config(C.byref(c))
    c.slots = 0
    x = C.c_void_p()
    with pytest.raises(api.D2FEError, match="bad loop configuration"):        # the whole struct is read: slots = 0 is refused
        api._check(lib.d2fe_loop_create(pipe._p, C.byref(c), C.byref(x)))
    assert not x.value
    c.struct_size = api._LoopConfig.slots.offset                               # the struct of a caller that does not know `slots`
    api._check(lib.d2fe_loop_create(pipe._p, C.byref(c), C.byref(x)))
    res = api._LoopResult()
    with pytest.raises(api.D2FEError, match="nothing was enqueued"):          # slot 3 exists: four slots
        api._check(lib.d2fe_loop_collect(x, 3, C.byref(res)))
    with pytest.raises(api.D2FEError, match="bad argument"):                  # slot 4 does not
        api._check(lib.d2fe_loop_collect(x, 4, C.byref(res)))
    lib.d2fe_loop_destroy(x)
    pipe.close(); fe.close()
