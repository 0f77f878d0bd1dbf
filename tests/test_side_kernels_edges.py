"""Exact-arithmetic edge cases of the kernels either side of the hot path: csrc/next.hip (undistort, gray/resize, the flat inner-product database, the int8 codec),
the search kernel of csrc/loop.hip, and the gates, the int8 block codec and the half-image compaction of csrc/swarm.hip.
CPU part: on the very inputs the GPU tests use, the oracle equals an independent numpy evaluation (int64 dot products, integer / rational image arithmetic with an
explicit round-half-to-even).  GPU part (-m gpu): the device equals the oracle bit for bit; the one tolerance is the existing 1e-6 of the dequantiser's normalised
entries.  The similarity inputs are integer-valued vectors (entries in -3..3, length <= 8192): every product and partial sum is an integer below 2^24, exact in fp32
in any summation order, so ties, zeros and negative similarities are abundant and exact.
Two cases are not what their size suggests: 8 queries of length 1024 stage 32 KiB (8 is the most queries one search takes; 8 x 2048, 4 x 4096 and 2 x 8192 stage
exactly 64 KiB), and 130x9 -> 65x5 is a 2x decimation in x only, so it is bilinear on both sides (130x10 -> 65x5 is the area case across the block edges)."""
import functools

import numpy as np
import pytest

DB_MAXK = 1024                            # csrc/next_host.hip
DIMS = (4, 260, 1024, 4100, 8192)
NTOTALS = (1, 3, 5, 1029)                 # 1029: above the 1024-thread stride of the top-k scan, no multiple of the 4 rows of a workgroup
BATCHED = ((8, 1024), (8, 2048), (4, 4096), (2, 8192))      # (nq, dim): the most queries a call takes; the others stage exactly 64 KiB
NT_BATCHED = 261
MAX_INDEX = (0, 2, 7)
NQ = 8


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _fe():
    from d2slam_amd import api
    return api, api.FrontEnd(api.SuperPointConfig(input_width=64, input_height=64, max_batch=1))


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- 1. similarity search and gates ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _int_case(dim, ntotal):
    """(db [ntotal][dim], queries [NQ][dim], exact int64 similarities [ntotal][NQ]).  Query 0's best row (3 * sign(q0), the largest similarity any row can reach) sits,
    bit-identical, at the first, the middle and the last label; row 1 is all zero (ntotal 3: the middle label is the zero row); query 1 is a copy of row ntotal - 2;
    query 2 = -q0 (the copies tie at the most negative similarity); query 3 is all zero (every similarity ties at +0); the others are random."""
    rng = np.random.RandomState(1000 * dim + ntotal)
    db = rng.randint(-3, 4, size=(ntotal, dim)).astype(np.float32)
    q = rng.randint(-3, 4, size=(NQ, dim)).astype(np.float32)
    q[0, 0] = 1
    for r in sorted({0, ntotal // 2, ntotal - 1}):
        db[r] = 3 * np.sign(q[0])
    if ntotal >= 3:
        db[1] = 0
    if ntotal >= 5:
        q[1] = db[ntotal - 2]
    q[2] = -q[0]
    q[3] = 0
    s = db.astype(np.int64) @ q.astype(np.int64).T
    assert np.abs(s).max() < 2 ** 24
    return _ro(db, q, s)


def _rank(s):
    """labels by (similarity descending, label ascending)"""
    return np.lexsort((np.arange(len(s)), -s))


def _best_allowed(s, max_index):
    """the first allowed label of the ranking (label <= ntotal - max_index, loop_detector.cpp:314-345), or -1"""
    for l in _rank(s):
        if l <= len(s) - max_index:
            return int(l)
    return -1


def _gate_exact(s, max_index, thres):
    l = _best_allowed(s, max_index)
    return (l, int(s[l])) if l >= 0 and s[l] > thres else (-1, 0)


def _thresholds(s, max_index):
    """below, exactly on and above the best allowed similarity"""
    l = _best_allowed(s, max_index)
    t = int(s[l]) if l >= 0 else 0
    return (t - 1, t, t + 1)


def _search_cases():
    return [(d, n) for d in DIMS for n in NTOTALS] + [(d, NT_BATCHED) for _, d in BATCHED]


@pytest.mark.parametrize("dim", sorted(set(DIMS) | {d for _, d in BATCHED}))
def test_db_query_oracle_on_integer_vectors(orc, dim):
    for ntotal in [n for d, n in _search_cases() if d == dim]:
        db, q, s = _int_case(dim, ntotal)
        if ntotal >= 3:
            assert not db[1].any() and np.array_equal(_bits(db[0]), _bits(db[ntotal - 1]))
        if ntotal == 1029:
            neg = int((s[:, 0] < 0).sum())
            assert 0.3 * ntotal < neg < 0.7 * ntotal and (s[:, 3] == 0).all()
        for j in range(NQ):
            _, _, labels, sims = orc.db_query(db, q[j], 0, -1e30, search_nearest=ntotal)      # the whole ranking
            order = _rank(s[:, j])
            assert np.array_equal(labels, order) and np.array_equal(sims.astype(np.int64), s[order, j])
            assert not np.signbit(sims[sims == 0]).any()          # an exact zero is +0: it ranks above every negative similarity on both sides
            for mi in MAX_INDEX:
                for thres in _thresholds(s[:, j], mi):
                    ol, osim = orc.db_query(db, q[j], mi, float(thres))[:2]
                    el, es = _gate_exact(s[:, j], mi, thres)
                    assert ol == el and (ol < 0 or osim == es), (ntotal, j, mi, thres)
                assert _gate_exact(s[:, j], mi, _thresholds(s[:, j], mi)[1])[0] == -1          # exactly on the threshold: the strict > rejects


@pytest.mark.gpu
@pytest.mark.parametrize("dim", DIMS)
def test_db_search_and_gate_exact_order_ties_and_negatives(orc, dim):
    api, fe = _fe()
    for ntotal in NTOTALS:
        dbh, q, s = _int_case(dim, ntotal)
        db = api.FlatIPDatabase(fe, dim, capacity=ntotal + 3)
        assert db.add(dbh) == 0 and db.ntotal == ntotal
        for j in range(NQ):
            order = _rank(s[:, j])
            for k in sorted({min(ntotal, DB_MAXK), min(ntotal + 3, DB_MAXK)}):
                sims, labels = db.search(q[j], k)
                kk = min(k, ntotal)
                assert np.array_equal(labels[0, :kk], order[:kk]), (ntotal, j, k)
                assert np.array_equal(_bits(sims[0, :kk]), _bits(s[order[:kk], j].astype(np.float32))), (ntotal, j, k)
                assert (labels[0, kk:] == -1).all() and not _bits(sims[0, kk:]).any()
            for mi in MAX_INDEX:
                for thres in _thresholds(s[:, j], mi):
                    label, sim = db.query_gated(q[j], mi, float(thres))
                    ol, osim = orc.db_query(dbh, q[j], mi, float(thres))[:2]
                    el, es = _gate_exact(s[:, j], mi, thres)
                    assert label == ol == el, (ntotal, j, mi, thres, label, ol, el)
                    assert sim == (osim if label >= 0 else 0.0) == es
        db.close()
    fe.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nq,dim", BATCHED)
def test_db_search_batched_at_the_staging_limit(nq, dim):
    api, fe = _fe()
    assert nq * dim * 4 == (65536 if dim > 1024 else 32768)
    dbh, q, s = _int_case(dim, NT_BATCHED)
    db = api.FlatIPDatabase(fe, dim, capacity=NT_BATCHED)
    db.add(dbh)
    sims, labels = db.search(q[:nq], NT_BATCHED)
    for j in range(nq):
        s1, l1 = db.search(q[j], NT_BATCHED)
        order = _rank(s[:, j])
        assert np.array_equal(labels[j], l1[0]) and np.array_equal(_bits(sims[j]), _bits(s1[0]))
        assert np.array_equal(labels[j], order) and np.array_equal(_bits(sims[j]), _bits(s[order, j].astype(np.float32)))
    over = np.concatenate([q[:nq], q[:1]])
    with pytest.raises(api.D2FEError):          # one query over the limit: refused, not launched
        db.search(over, 1)
    assert db.search(q[0], 1)[1][0, 0] == _rank(s[:, 0])[0]
    db.close(); fe.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [8, 260, 4100])      # the tails of <1,2> and <4,2>; 4100: <32,1>, in whose last step only lane 0 holds data
def test_loop_query_device_exact_order_ties_and_threshold(orc, dim):
    import torch
    from tests.test_loop_query import H, RATIO, W, _stereo_fe
    cap, D = 8, 256
    api, fe = _stereo_fe(2, pca=dim, cap=cap)
    assert fe.netvlad_dim == dim
    pipe = api.StereoPipe(fe, lanes=1, frames=1, width=W, height=H, cap=cap, netvlad=True)
    dev = torch.device("cuda", 0)
    for ntotal in (3, 1029):
        dbh, q, s = _int_case(dim, ntotal)
        rng = np.random.RandomState(dim + ntotal)
        unit = lambda a: (a / np.linalg.norm(a, axis=-1, keepdims=True)).astype(np.float32)
        kdesc = unit(rng.randn(ntotal, cap, D)); kn = rng.randint(2, cap + 1, size=ntotal).astype(np.int32)
        qdesc = unit(rng.randn(NQ, cap, D)); qn = rng.randint(2, cap + 1, size=NQ).astype(np.int32)
        db = api.FlatIPDatabase(fe, dim, capacity=ntotal)
        db.add(dbh)
        d_q, d_d, d_n = (torch.from_numpy(np.array(x)).to(dev) for x in (q, qdesc, qn))
        torch.cuda.synchronize()
        assert _best_allowed(s[:, 0], 0) == _best_allowed(s[:, 0], 2) == 0      # the copy at the last label is allowed once and excluded once; the first wins both times
        for thres in _thresholds(s[:, 0], 0):
            loop = api.LoopQuery(pipe, capacity_keyframes=ntotal + 1, max_index=10, thres=float(thres), ratio=RATIO, mode=0, slots=1, max_queries=7)
            assert loop.add_host(dbh[:, None], kdesc[:, None], kn[:, None]) == 0 and loop.ntotal == ntotal
            for nq in (1, 7):
                for mi in (0, 2):
                    loop.query_device(d_q.data_ptr(), d_d.data_ptr(), d_n.data_ptr(), nq, mi, 0)
                    r = loop.collect(0)
                    assert r["frames"] == nq
                    for j in range(nq):
                        assert int(r["queried"][j]) == 1 and int(r["ntotal_at_query"][j]) == ntotal
                        ol = orc.db_query(dbh, q[j], mi, float(thres))[0]
                        hl, hs = db.query_gated(q[j], mi, float(thres))
                        el, es = _gate_exact(s[:, j], mi, thres)
                        label = int(r["label"][j])
                        assert label == ol == hl == el, (ntotal, thres, nq, mi, j, label, ol, hl, el)
                        assert int(r["keyframe"][j]) == label
                        assert _bits(r["sim"][j:j + 1])[0] == _bits(np.float32(hs).reshape(1))[0] == _bits(np.float32(es).reshape(1))[0]
                        assert int(r["n_match"][j, 0]) >= 0
                    if nq == 1:      # query 0: one below passes, exactly on and above reject
                        assert (int(r["label"][0]) == 0) == (thres < s[0, 0])
            loop.close()
        db.close()
    pipe.close(); fe.close()


G_GATE = 260


@functools.lru_cache(maxsize=None)
def _gate_case():
    """pairs of the stereo gate and jobs of the quad gate, integer vectors.  Quad job 0: view dirs[0] = 2 is one below the similarity of view dirs[1] = 3."""
    rng = np.random.RandomState(77)
    G = G_GATE
    q = rng.randint(-3, 4, size=(4, G)).astype(np.float32); dbv = rng.randint(-3, 4, size=(5, G)).astype(np.float32)
    pq = np.array([0, 1, 2, 3, 1, 2, 0], np.int32); pd = np.array([0, 1, 2, 3, 4, 0, 4], np.int32)
    sp =np.array([q[a].astype(np.int64) @ dbv[c].astype(np.int64) for a, c in zip(pq, pd)])
    nj = 5
    loc = rng.randint(-3, 4, size=(nj * 4, G)).astype(np.float32); rem = rng.randint(-3, 4, size=(nj * 4, G)).astype(np.float32)
    rem[2, 0] = 1; loc[3, 0] = 0; loc[2] = loc[3]; loc[2, 0] = -1
    sj = np.array([[loc[4 * j + ((2 + i) & 3)].astype(np.int64) @ rem[4 * j + 2].astype(np.int64) for i in range(4)] for j in range(nj)])
    assert sj[0, 0] == sj[0, 1] - 1
    return _ro(q, dbv, pq, pd, sp, loc, rem, sj)


def _quad_dir(s4, thres):
    for i in range(4):
        if s4[i] >= thres:          # !(s < thres): equality passes, the first view that passes wins
            return (2 + i) & 3
    return -1


def test_tracker_gate_oracle_on_integer_vectors(orc):
    q, dbv, pq, pd, sp, loc, rem, sj = _gate_case()
    for thres in (int(sp[2]), int(sp[2]) + 1):
        for p, (a, c) in enumerate(zip(pq, pd)):
            r = orc.tracker_gate(q[a][None], dbv[c][None, None], float(thres), False)
            assert (r is not None) == bool(sp[p] >= thres)
            assert r is None or int(r["sims"][0]) == sp[p]
    assert 0 < int((sp >= sp[2]).sum()) < len(sp)        # at the threshold of pair 2 some pairs pass and some fail
    for thres in (int(sj[0, 1]), int(sj[0, 1]) + 1):
        for j in range(len(sj)):
            r = orc.tracker_gate(rem[4 * j:4 * j + 4], loc[4 * j:4 * j + 4][None], float(thres), True)
            d = _quad_dir(sj[j], thres)
            assert (r is None) == (d < 0)
            if r is not None:
                n = [2, 3, 0, 1].index(d) + 1
                assert r["dir_b"] == d and np.array_equal(r["sims"][:n].astype(np.int64), sj[j, :n])
    assert _quad_dir(sj[0], int(sj[0, 1])) == 3          # decided by the boundary: view 2 fails by one, view 3 is exactly on the threshold


def _strided(rows, stride, lead):
    """rows laid out `stride` floats apart behind `lead` floats; the gaps hold a value no product survives unnoticed"""
    flat = np.full(lead + rows.shape[0] * stride + 4, 1000.0, np.float32)
    for r in range(rows.shape[0]):
        flat[lead + r * stride:lead + r * stride + rows.shape[1]] = rows[r]
    return flat


@pytest.mark.gpu
def test_gates_on_the_threshold_vector_and_scalar_loads():
    import torch
    api, fe = _fe()
    dev = torch.device("cuda", 0)
    G = G_GATE
    q, dbv, pq, pd, sp, loc, rem, sj = _gate_case()
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)
    d_pq, d_pd = t(pq), t(pd)
    rows = t(np.arange(len(sj), dtype=np.int32) * 4)
    # (lead, stride of the first array, stride of the second): 16-byte aligned float4 loads; a pointer 4 bytes off and an odd stride: four scalar loads
    for lead, st_a, st_b in ((0, G + 4, 2 * G), (1, G + 1, G + 1)):
        d_q, d_db, d_loc, d_rem = t(_strided(q, st_a, lead)), t(_strided(dbv, st_b, lead)), t(_strided(loc, st_a, lead)), t(_strided(rem, st_b, lead))
        assert all(x.data_ptr() % 16 == 0 for x in (d_q, d_db, d_loc, d_rem))
        for thres in (int(sp[2]), int(sp[2]) + 1):
            n = len(pq)
            cnt = torch.full((n,), 9, dtype=torch.int32, device=dev); pas = torch.full((n,), 5, dtype=torch.int32, device=dev)
            gs = torch.zeros(n, device=dev); gn = torch.zeros(1, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            fe.gate_pairs_device(d_q.data_ptr() + 4 * lead, st_a, d_db.data_ptr() + 4 * lead, st_b, G, d_pq.data_ptr(), d_pd.data_ptr(), n, float(thres),
                                 d_cnt_inout=cnt.data_ptr(), d_pass=pas.data_ptr(), d_sims=gs.data_ptr(), d_n_pass=gn.data_ptr())
            fe.sync(); torch.cuda.synchronize()
            exp = (sp >= thres).astype(np.int32)
            assert exp[2] == (1 if thres == sp[2] else 0)                       # exactly on the threshold passes, one above fails
            assert np.array_equal(_bits(gs.cpu().numpy()), _bits(sp.astype(np.float32))), (lead, thres)
            assert np.array_equal(pas.cpu().numpy(), exp) and int(gn.item()) == int(exp.sum())
            assert np.array_equal(cnt.cpu().numpy(), np.where(exp == 1, 9, 0))
        for thres in (int(sj[0, 1]), int(sj[0, 1]) + 1):
            nj = len(sj)
            dirp = torch.full((nj,), 7, dtype=torch.int32, device=dev); sims = torch.zeros((nj, 4), device=dev)
            cnt = torch.full((nj * 16,), 9, dtype=torch.int32, device=dev); npass = torch.zeros(1, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            fe.quad_gate_device(d_loc.data_ptr() + 4 * lead, st_a, d_rem.data_ptr() + 4 * lead, st_b, G, rows.data_ptr(), rows.data_ptr(), 1, 1, nj, float(thres),
                                d_dir_prev=dirp.data_ptr(), d_sims=sims.data_ptr(), d_cnt_inout=cnt.data_ptr(), d_n_pass=npass.data_ptr())
            fe.sync(); torch.cuda.synchronize()
            exp_dir = np.array([_quad_dir(sj[j], thres) for j in range(nj)], np.int32)
            if thres == sj[0, 1]:
                assert exp_dir[0] == 3
            assert np.array_equal(dirp.cpu().numpy(), exp_dir), (lead, thres)
            assert np.array_equal(_bits(sims.cpu().numpy()), _bits(sj.astype(np.float32)))
            assert int(npass.item()) == int((exp_dir >= 0).sum())
            keep = np.zeros((nj, 16), bool)
            for j in range(nj):
                for lv in range(4):
                    for rv in range(4):
                        keep[j, lv * 4 + rv] = exp_dir[j] >= 0 and lv == (exp_dir[j] - 2 + rv + 4) % 4
            assert np.array_equal(cnt.cpu().numpy().reshape(nj, 16), np.where(keep, 9, 0))
    fe.close()


# ---- 2. int8 codec ----------------------------------------------------------------------------------------------------------------------------------------------
QUANT_N = (1, 32, 96, 1056, 2048 + 32)
QUANT_SCALES = (1.0, 2.0 ** -7, 0.3)


@functools.lru_cache(maxsize=None)
def _quant_input(n, scale):
    """max |x| = 127 * scale at both signs (codes +-127); integers k (x / max * 127 is k in exact arithmetic) and values 2^-10 closer to zero (just below an integer);
    negative values with a fraction (the cast truncates toward zero); exact zeros; ordinary values"""
    rng = np.random.RandomState(n)
    k = rng.randint(-126, 127, size=n).astype(np.float32)
    kind = rng.randint(0, 5, size=n)
    x = k.copy()
    x[kind == 1] = (k - np.sign(k) * np.float32(2.0 ** -10))[kind == 1]
    x[kind == 2] = -(np.abs(k) - np.float32(0.25))[kind == 2]
    x[kind == 3] = 0
    x[kind == 4] = np.clip(rng.randn(n).astype(np.float32) * 40, -126, 126)[kind == 4]
    x[0] = -127
    if n > 1:
        x[-1] = 127; x[1] = 0; x[2] = 64; x[3] = -63.75
    x = (x * np.float32(scale)).astype(np.float32)
    return _ro(x)[0]


def _quant_exact(x, double_max):
    m = np.abs(x).max()
    if not m > 0:
        return np.zeros(len(x), np.int8)
    if double_max:
        return np.trunc(x.astype(np.float64) / np.float64(m) * 127.0).astype(np.int8)
    return np.trunc(x / np.float32(m) * np.float32(127)).astype(np.int8)


DEQ_N = (32, 96, 1056)


def _deq_lms(n):
    return (0, 1, n // 32, n // 32 + 5)


@functools.lru_cache(maxsize=None)
def _deq_input(n, phase):
    """bytes with every third 32-byte segment all zero, from segment `phase` on"""
    rng = np.random.RandomState(7 * n + phase)
    q = rng.randint(-127, 128, size=n).astype(np.int8).reshape(-1, 32)
    q[:, 0] = 5                                   # no other segment is all zero
    q[phase::3] = 0
    return _ro(q.reshape(-1))[0]


def _deq_check(got, q, lm, ref):
    """ref: the oracle's decode.  Entries outside the normalised range and all-zero segments carry no rounding of a division: exactly q / 127.0; the rest within 1e-6"""
    raw = (q.astype(np.float64) / 127.0).astype(np.float32)
    plain = np.ones(len(q), bool)
    if lm >= 0:
        seg = np.arange(len(q)) // 32
        plain = (seg >= lm) | ~q.reshape(-1, 32).any(axis=1)[seg]
    else:
        plain[:] = not q.any()
    assert np.array_equal(_bits(ref[plain]), _bits(raw[plain]))
    assert np.array_equal(_bits(got[plain]), _bits(raw[plain]))
    assert np.abs(got - ref).max() <= 1e-6 and np.isfinite(got).all()


def _whole_inputs():
    for n in (96, 1056):
        z = np.zeros(n, np.int8)
        one = z.copy(); one[n - 3] = -77
        yield z
        yield one


def test_int8_codec_oracle_edges(orc):
    for n in QUANT_N:
        for scale in QUANT_SCALES:
            x = _quant_input(n, scale)
            for dm in (False, True):
                got = orc.quant_int8(x, double_max=dm)
                assert np.array_equal(got, _quant_exact(x, dm)), (n, scale, dm)
                assert got[0] == -127 and (n == 1 or (got[-1] == 127 and got[1] == 0))
        for dm in (False, True):                  # an all-zero tensor encodes to zeros (the reference divides 0 by 0)
            assert not orc.quant_int8(np.zeros(n, np.float32), double_max=dm).any()
    for n in DEQ_N:
        for phase in (0, 1):
            q = _deq_input(n, phase)
            for lm in _deq_lms(n):
                ref = orc.dequant_int8(q, lm)
                x = (q.astype(np.float64) / 127.0).astype(np.float32).astype(np.float64).reshape(-1, 32)
                nr = np.linalg.norm(x, axis=1, keepdims=True)
                e = np.where((np.arange(n // 32)[:, None] < lm) & (nr > 0), x / np.where(nr > 0, nr, 1), x)
                _deq_check(e.reshape(-1).astype(np.float32), q, lm, ref)
    for q in _whole_inputs():
        ref = orc.dequant_int8(q, -1)
        x = q.astype(np.float64) / 127.0
        nr = np.linalg.norm(x)
        _deq_check((x / nr if nr > 0 else x).astype(np.float32), q, -1, ref)
        assert np.count_nonzero(ref) == np.count_nonzero(q)


@pytest.mark.gpu
def test_int8_codec_gpu_edges(orc):
    api, fe = _fe()
    for n in QUANT_N:
        for scale in QUANT_SCALES:
            x = _quant_input(n, scale)
            for dm in (False, True):
                assert np.array_equal(fe.quantize_int8(x, double_max=dm), orc.quant_int8(x, double_max=dm)), (n, scale, dm)
        for dm in (False, True):
            assert not fe.quantize_int8(np.zeros(n, np.float32), double_max=dm).any()
    for n in DEQ_N:
        for phase in (0, 1):
            q = _deq_input(n, phase)
            for lm in _deq_lms(n):
                _deq_check(fe.dequantize_int8(q, lm), q, lm, orc.dequant_int8(q, lm))
    for q in _whole_inputs():
        got = fe.dequantize_int8(q, -1)
        _deq_check(got, q, -1, orc.dequant_int8(q, -1))
        assert np.count_nonzero(got) == np.count_nonzero(q)
    fe.close()


G_BLK = 260


@functools.lru_cache(maxsize=None)
def _block_case(cap):
    """frames of the int8 exchange block: counts -3, 0, 1, cap, cap + 9 (clamped) and a full frame whose descriptors and NetVLAD vector are all zero; frame 3 holds an
    all-zero descriptor row and an all-zero 32-float segment"""
    rng = np.random.RandomState(cap)
    n = np.array([-3, 0, 1, cap, cap + 9, cap], np.int32)
    desc = rng.randn(len(n), cap, 256).astype(np.float32); desc /= np.linalg.norm(desc, axis=2, keepdims=True)
    desc[5] = 0; desc[3, 0] = 0; desc[3, min(2, cap - 1), 32:64] = 0
    kps = (rng.rand(len(n), cap, 2) * 100).astype(np.float32)
    g = rng.randn(len(n), G_BLK).astype(np.float32); g /= np.linalg.norm(g, axis=1, keepdims=True)
    g[5] = 0
    return _ro(n, desc, kps, g)


def test_int8_block_inputs_oracle(orc):
    for cap in (7, 50):
        n, desc, kps, g = _block_case(cap)
        for f in range(len(n)):
            k = max(0, min(int(n[f]), cap))
            if k:
                x = desc[f, :k].reshape(-1)
                ql = orc.quant_int8(x)
                assert np.array_equal(ql, _quant_exact(x, False)) and ql.any() == (f != 5)
                back = orc.dequant_int8(ql, k)
                assert np.isfinite(back).all() and (f != 5 or not back.any())
            assert np.array_equal(orc.quant_int8(g[f], double_max=True), _quant_exact(g[f], True))


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [7, 50])      # no multiple of 4: the last 256-thread step of every field is partial and the field offsets are odd
def test_int8_blocks_gpu_edges(orc, cap):
    import torch
    api, fe = _fe()
    dev = torch.device("cuda", 0)
    G = G_BLK
    n, desc, kps, g = _block_case(cap)
    rows = len(n)
    BB = api.block_bytes_int8(cap, G); BLK = api.block_words(cap, G)
    off = {f: api.block_field_offset(cap, G, f) for f in ("desc", "kps", "scores", "netvlad", "n")}
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)
    d_desc, d_kps, d_n, d_g = t(desc), t(kps), t(n), t(g)
    for with_g in (True, False):
        bq = torch.full((rows, BB), 7, dtype=torch.int8, device=dev)
        torch.cuda.synchronize()
        fe.pack_blocks_int8_device(d_desc.data_ptr(), d_kps.data_ptr(), d_n.data_ptr(), d_g.data_ptr() if with_g else None, 0, 1, rows, cap, G, bq.data_ptr())
        fe.sync(); torch.cuda.synchronize()
        q = bq.cpu().numpy()
        ql, qn = [], []
        for f in range(rows):
            k = max(0, min(int(n[f]), cap))
            exp = np.zeros(BB, np.int8)
            ql.append(orc.quant_int8(desc[f, :k].reshape(-1)) if k else np.zeros(0, np.int8))
            qn.append(orc.quant_int8(g[f], double_max=True) if with_g else np.zeros(G, np.int8))
            exp[:k * 256] = ql[f]; exp[cap * 256:cap * 256 + G] = qn[f]
            exp[cap * 256 + G:cap * 256 + G + 8 * cap].view(np.float32)[:2 * k] = kps[f, :k].reshape(-1)
            exp[cap * 256 + G + 8 * cap:cap * 256 + G + 8 * cap + 4].view(np.int32)[0] = k
            assert np.array_equal(q[f], exp), (with_g, f)                      # every byte, the zero padding included
            assert f != 5 or not q[f, :cap * 256 + G].any()                     # the all-zero frame: zeros, not the cast of a NaN
        for renorm in (0, 1):
            out = torch.full((rows, BLK), 7.0, device=dev)
            torch.cuda.synchronize()
            fe.unpack_blocks_int8_device(bq.data_ptr(), rows, cap, G, out.data_ptr(), renorm=renorm)
            fe.sync(); torch.cuda.synchronize()
            o = out.cpu().numpy()
            assert np.isfinite(o[:, :off["n"]]).all()
            for f in range(rows):
                k = max(0, min(int(n[f]), cap))
                od = o[f, :k * 256]
                if k and renorm == 0:
                    _deq_check(od, ql[f], k, orc.dequant_int8(ql[f], k))
                elif k:
                    x = (ql[f].astype(np.float64) / 127.0).astype(np.float32).reshape(k, 256)
                    nr = np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True)
                    assert np.abs(od.reshape(k, 256) - np.where(nr > 0, x / np.where(nr > 0, nr, 1), 0)).max() <= 1e-6
                    assert not od.reshape(k, 256)[~ql[f].reshape(k, 256).any(axis=1)].any()      # an all-zero row stays zero
                _deq_check(o[f, off["netvlad"]:off["netvlad"] + G], qn[f], -1, orc.dequant_int8(qn[f], -1))
                assert (with_g and f != 5) or not o[f, off["netvlad"]:off["netvlad"] + G].any()
                exact = np.zeros(BLK, np.float32)
                exact[off["kps"]:off["kps"] + 2 * k] = kps[f, :k].reshape(-1)
                exact.view(np.int32)[off["n"]] = k
                got = o[f].copy(); got[:k * 256] = 0; got[off["netvlad"]:off["netvlad"] + G] = 0
                assert np.array_equal(_bits(got), _bits(exact)), (with_g, renorm, f)      # the rest of the descriptors, kps, scores, n and the padding
                if f == 5:
                    assert not od.any()
    fe.close()


# ---- 3. undistort and gray/resize at the borders -------------------------------------------------------------------------------------------------------------
U_SH, U_SW, U_SSTRIDE, U_N = 9, 13, 16, 3
U_ISTRIDE = U_SSTRIDE * U_SH + 32
U_DSTS = ((7, 11), (10, 30))              # (rows, columns): one partial 256-thread block; two blocks
U_GAINS = (0.0, 0.5, 1.0, 1.5, 2.5, 300.0)


@functools.lru_cache(maxsize=None)
def _undist_case(dh, dw):
    """(source bytes with row and image padding, mapx, mapy, gain).  Every map value is a multiple of 1/4: the four weight products and their sum are exact in fp32."""
    rng = np.random.RandomState(100 * dh + dw)
    buf = rng.randint(0, 256, size=U_N * U_ISTRIDE).astype(np.uint8)          # the padding is random too: it must never be read as a pixel
    even = ((10, 11), (20, 21), (254, 255), (0, 1), (100, 101), (30, 31))    # mean k + .5 with k even: rounds down
    odd = ((11, 12), (21, 22), (1, 2), (253, 254), (101, 102), (31, 32))     # k odd: rounds up
    for i in range(U_N):
        img = buf[i * U_ISTRIDE:i * U_ISTRIDE + U_SH * U_SSTRIDE].reshape(U_SH, U_SSTRIDE)
        for c in range(6):
            img[3, 2 * c:2 * c + 2] = even[c]; img[5, 2 * c:2 * c + 2] = odd[c]
        img[0, 0], img[0, U_SW - 1], img[U_SH - 1, 0], img[U_SH - 1, U_SW - 1] = 255, 254, 1, 255
    sw, sh = float(U_SW), float(U_SH)
    edge_x = (-1.0, -0.75, -0.25, sw - 1, sw - 0.25, sw); edge_y = (-1.0, -0.75, -0.25, sh - 1, sh - 0.25, sh)
    pts = [(3.0, 4.0), (0.0, 0.0), (sw - 1, sh - 1)]                                        # exact pixel centres
    pts += [(x, 2.5) for x in edge_x] + [(6.25, y) for y in edge_y]
    pts += [(x, y) for x in (0.0, sw - 1) for y in (0.0, sh - 1)]                           # the four corners, and a quarter pixel outside them
    pts += [(x, y) for x in (-0.25, sw - 0.75) for y in (-0.25, sh - 0.75)]
    pts += [(x, y) for x in (-1.0, sw) for y in (-1.0, sh)]
    pts += [(1e6, 3.0), (-1e6, 3.0), (3.0, 1e6), (3.0, -1e6), (1e6, 1e6), (-1e6, -1e6)]
    pts += [(2 * c + 0.5, 3.0) for c in range(6)] + [(2 * c + 0.5, 5.0) for c in range(6)]  # .5 ties of the first rounding
    assert len(pts) <= dh * dw
    mx = rng.randint(-8, 4 * (U_SW + 1) + 1, size=dh * dw).astype(np.float32) / 4
    my = rng.randint(-8, 4 * (U_SH + 1) + 1, size=dh * dw).astype(np.float32) / 4
    at = rng.permutation(dh * dw)[:len(pts)]
    mx[at] = [p[0] for p in pts]; my[at] = [p[1] for p in pts]
    gain = np.array(U_GAINS, np.float32)[rng.randint(0, len(U_GAINS), size=dh * dw)]
    return _ro(buf, mx.reshape(dh, dw), my.reshape(dh, dw), gain.reshape(dh, dw))


def _undist_img(buf, i):
    return np.ascontiguousarray(buf[i * U_ISTRIDE:i * U_ISTRIDE + U_SH * U_SSTRIDE].reshape(U_SH, U_SSTRIDE)[:, :U_SW])


def _round_half_even(num, den):
    q, r = np.divmod(num, den)
    return q + ((2 * r > den) | ((2 * r == den) & (q % 2 == 1)))


def _undist_exact(img, mx, my, gain):
    """16 * (the interpolated value) in int64, then the two roundings of the reference, half to even, each clamped to 0..255.  Returns (u8 image, 16 * value)."""
    sh, sw = img.shape
    X = np.rint(mx.astype(np.float64) * 4).astype(np.int64); Y = np.rint(my.astype(np.float64) * 4).astype(np.int64)
    assert np.array_equal(X / 4.0, mx) and np.array_equal(Y / 4.0, my)
    x1, y1 = X // 4, Y // 4
    fx, fy = X - 4 * x1, Y - 4 * y1
    P = img.astype(np.int64)

    def S(y, x):
        ok = (y >= 0) & (y < sh) & (x >= 0) & (x < sw)
        return np.where(ok, P[np.clip(y, 0, sh - 1), np.clip(x, 0, sw - 1)], 0)
    N = S(y1, x1) * (4 - fx) * (4 - fy) + S(y1, x1 + 1) * fx * (4 - fy) + S(y1 + 1, x1) * (4 - fx) * fy + S(y1 + 1, x1 + 1) * fx * fy
    u = np.clip(_round_half_even(N, 16), 0, 255)
    if gain is not None:
        g2 = np.rint(gain.astype(np.float64) * 2).astype(np.int64)
        assert np.array_equal(g2 / 2.0, gain)
        u = np.clip(_round_half_even(u * g2, 2), 0, 255)
    return u.astype(np.uint8), N


@pytest.mark.parametrize("dh,dw", U_DSTS)
def test_undistort_oracle_vs_integer_arithmetic(orc, dh, dw):
    buf, mx, my, gain = _undist_case(dh, dw)
    down = up = gain_ties = saturated = 0
    for i in range(U_N):
        img = _undist_img(buf, i)
        assert {0, 1, 254, 255} <= set(img.reshape(-1).tolist())
        for g in (gain, None):
            e, N = _undist_exact(img, mx, my, g)
            assert np.array_equal(orc.undistort(img, mx, my, g), e), (i, g is None)
        tie = N % 16 == 8
        down += int((tie & (N // 16 % 2 == 0)).sum()); up += int((tie & (N // 16 % 2 == 1)).sum())
        u = _undist_exact(img, mx, my, None)[0].astype(np.int64)
        g2 = np.rint(gain * 2).astype(np.int64)
        gain_ties += int(((u * g2) % 2 == 1).sum()); saturated += int((u * g2 > 510).sum())
    assert down >= 6 * U_N and up >= 6 * U_N and gain_ties >= 6 and saturated >= 6


@pytest.mark.gpu
@pytest.mark.parametrize("dh,dw", U_DSTS)
def test_undistort_device_borders_ties_and_strides(orc, dh, dw):
    import torch
    api, fe = _fe()
    dev = torch.device("cuda", 0)
    buf, mx, my, gain = _undist_case(dh, dw)
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)
    d_src, d_mx, d_my, d_g = t(buf), t(mx), t(my), t(gain)
    for g in (gain, None):
        out = torch.full((U_N * dh * dw + 64,), 7, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        fe.undistort_device(d_src.data_ptr(), U_N, U_SW, U_SH, d_mx.data_ptr(), d_my.data_ptr(), d_g.data_ptr() if g is not None else None, dw, dh, out.data_ptr(),
                            sstride=U_SSTRIDE, src_image_stride=U_ISTRIDE)
        fe.sync(); torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert (o[U_N * dh * dw:] == 7).all()                                   # nothing behind the last image
        for i in range(U_N):
            img = _undist_img(buf, i)
            got = o[i * dh * dw:(i + 1) * dh * dw].reshape(dh, dw)
            assert np.array_equal(got, orc.undistort(img, mx, my, g)), (i, g is None)
            assert np.array_equal(got, _undist_exact(img, mx, my, g)[0])
    fe.close()


# (source width, height) -> (destination width, height)
GRAY_GEOMS = (((2, 2), (1, 1)), ((5, 3), (11, 7)), ((64, 48), (7, 5)), ((10, 6), (5, 3)), ((10, 6), (5, 6)), ((10, 6), (10, 3)), ((10, 6), (10, 6)),
              ((130, 9), (65, 5)), ((130, 10), (65, 5)))
GRAY_AREA = {((2, 2), (1, 1)), ((10, 6), (5, 3)), ((130, 10), (65, 5))}      # exact 2x in both axes: cv::resize computes INTER_AREA; 130x9 -> 65x5 is 2x in x only


@functools.lru_cache(maxsize=None)
def _gray_case(sw, sh, ch):
    """two images with a padded row stride and an image stride: (bytes, row stride, image stride)"""
    rng = np.random.RandomState(1000 * sw + 10 * sh + ch)
    stride = sw * ch + 5
    istride = stride * sh + 7
    buf = rng.randint(0, 256, size=2 * istride).astype(np.uint8)
    buf[:ch] = 255; buf[ch:2 * ch] = 0
    return _ro(buf)[0], stride, istride


def _gray_img(buf, stride, istride, sw, sh, ch, i):
    a = buf[i * istride:i * istride + sh * stride].reshape(sh, stride)[:, :sw * ch]
    return np.ascontiguousarray(a.reshape(sh, sw, ch) if ch == 3 else a)


def _gray_exact(img):
    if img.ndim == 2:
        return img.copy()
    p = img.astype(np.int64)
    return ((p[..., 0] * 3735 + p[..., 1] * 19235 + p[..., 2] * 9798 + (1 << 14)) >> 15).astype(np.uint8)


def _resize_coef(dsize, ssize, clamp):
    scale = 1.0 / (float(dsize) / float(ssize))
    f = ((np.arange(dsize, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(np.float32)
    if clamp:
        lo, hi = s < 0, s >= ssize - 1
        f[lo | hi] = 0; s[lo] = 0; s[hi] = ssize - 1
    return s, np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int64), np.rint(f * np.float32(2048)).astype(np.int64)


def _resize_exact(gray, dw, dh):
    """the 11-bit fixed-point INTER_LINEAR of cv::resize (8U) in int64; an exact 2x decimation is the 2x2 mean"""
    sh, sw = gray.shape
    g = gray.astype(np.int64)
    if sw == 2 * dw and sh == 2 * dh:
        return ((g[0::2, 0::2] + g[0::2, 1::2] + g[1::2, 0::2] + g[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    sy, b0, b1 = _resize_coef(dh, sh, False)
    sx, a0, a1 = _resize_coef(dw, sw, True)
    y0, y1 = np.clip(sy, 0, sh - 1), np.clip(sy + 1, 0, sh - 1)
    x1 = np.where(sx + 1 < sw, sx + 1, sx)
    S0 = g[y0][:, sx] * a0 + g[y0][:, x1] * a1
    S1 = g[y1][:, sx] * a0 + g[y1][:, x1] * a1
    return (((((b0[:, None] * (S0 >> 4)) >> 16) + ((b1[:, None] * (S1 >> 4)) >> 16) + 2) >> 2) & 255).astype(np.uint8)


def _resize_float(gray, dw, dh):
    """the float bilinear of test_prepare_gray_oracle_vs_float"""
    sh, sw = gray.shape
    yy, xx = np.mgrid[0:dh, 0:dw]
    fx = (xx + 0.5) * (sw / dw) - 0.5; fy = (yy + 0.5) * (sh / dh) - 0.5
    x0 = np.floor(fx).astype(int); y0 = np.floor(fy).astype(int); ax = fx - x0; ay = fy - y0
    c = lambda v, n: np.clip(v, 0, n - 1)
    a = gray.astype(np.float64)
    return (a[c(y0, sh), c(x0, sw)] * (1 - ax) * (1 - ay) + a[c(y0, sh), c(x0 + 1, sw)] * ax * (1 - ay)
            + a[c(y0 + 1, sh), c(x0, sw)] * (1 - ax) * ay + a[c(y0 + 1, sh), c(x0 + 1, sw)] * ax * ay)


def _gray_ref(orc, img, dw, dh):
    return orc.resize_linear_u8(orc.bgr2gray(img) if img.ndim == 3 else img, dw, dh)


@pytest.mark.parametrize("ch", [1, 3])
def test_prepare_gray_oracle_vs_integer_arithmetic(orc, ch):
    for (sw, sh), (dw, dh) in GRAY_GEOMS:
        assert (((sw, sh), (dw, dh)) in GRAY_AREA) == (sw == 2 * dw and sh == 2 * dh)
        buf, stride, istride = _gray_case(sw, sh, ch)
        for i in range(2):
            img = _gray_img(buf, stride, istride, sw, sh, ch, i)
            gray = _gray_exact(img)
            if ch == 3:
                assert np.array_equal(orc.bgr2gray(img), gray)
            ref = _gray_ref(orc, img, dw, dh)
            assert np.array_equal(ref, _resize_exact(gray, dw, dh)), (sw, sh, dw, dh)
            assert np.abs(ref.astype(int) - np.rint(_resize_float(gray, dw, dh)).astype(int)).max() <= 1, (sw, sh, dw, dh)
            if (sw, sh) == (dw, dh):
                assert np.array_equal(ref, gray)


@pytest.mark.gpu
@pytest.mark.parametrize("ch", [1, 3])
def test_prepare_gray_device_borders_and_strides(orc, ch):
    import torch
    api, fe = _fe()
    dev = torch.device("cuda", 0)
    for (sw, sh), (dw, dh) in GRAY_GEOMS:
        buf, stride, istride = _gray_case(sw, sh, ch)
        d_src = torch.from_numpy(buf.copy()).to(dev)
        out = torch.full((2 * dw * dh + 64,), 7, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        api._check(fe._lib.d2fe_prepare_gray_device(fe.handle, d_src.data_ptr(), 2, ch, sw, sh, stride, istride, dw, dh, out.data_ptr(), None))
        fe.sync(); torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert (o[2 * dw * dh:] == 7).all()
        for i in range(2):
            img = _gray_img(buf, stride, istride, sw, sh, ch, i)
            ref = _gray_ref(orc, img, dw, dh)
            assert np.array_equal(o[i * dw * dh:(i + 1) * dw * dh].reshape(dh, dw), ref), (sw, sh, dw, dh, i)
            assert np.abs(ref.astype(int) - np.rint(_resize_float(_gray_exact(img), dw, dh)).astype(int)).max() <= 1
            assert np.array_equal(fe.prepare_gray(img, dw, dh), ref)                          # the host entry, dense rows
            padded = np.ascontiguousarray(buf[i * istride:i * istride + sh * stride])          # the host entry through the C ABI, padded rows
            host = np.full((dh, dw), 7, np.uint8)
            api._check(fe._lib.d2fe_prepare_gray(fe.handle, api._ptr(padded), ch, sw, sh, stride, dw, dh, api._ptr(host)))
            assert np.array_equal(host, ref)
    fe.close()


# ---- 4. half-image compaction beyond one 256-chunk -----------------------------------------------------------------------------------------------------------
H_W, H_FOV, H_DIM = 800, 200.0, 12
H_MC = np.float32(H_W * 90.0 / H_FOV)           # move_cols of getFeatureHalfImg


@functools.lru_cache(maxsize=None)
def _half_case(cap):
    """(pts [rows][cap][2], desc, n, jobs).  Per 256-chunk of a row: both halves keep everything / the left half keeps nothing / random / the right half keeps nothing,
    with points exactly on move_cols and on W_u - move_cols"""
    rng = np.random.RandomState(cap)
    ns = (1024, 700, 257, 256, 0) if cap == 1024 else (300, 299, 257, 1, 0)
    mc = float(H_MC)
    on_edge = (mc, H_W - mc, np.nextafter(np.float32(mc), np.float32(0)), np.nextafter(np.float32(H_W - mc), np.float32(0)))
    pts = np.empty((len(ns), cap, 2), np.float32)
    for r in range(len(ns)):
        for c0 in range(0, cap, 256):
            m = min(256, cap - c0)
            kind = (c0 // 256 + r) % 4
            lo, hi = ((mc, H_W - mc), (H_W - mc, H_W), (0, H_W), (0, mc))[kind]
            pts[r, c0:c0 + m, 0] = rng.randint(int(lo), int(hi), size=m)
            if kind == 2:          # the edge values go into the random chunk: the dense and the empty chunks stay dense and empty
                for e, i in enumerate(range(c0 + 3, min(c0 + 256, cap), 11)):
                    pts[r, i, 0] = on_edge[e % 4]
        pts[r, :, 1] = rng.randint(0, 400, size=cap)
    desc = rng.randn(len(ns), cap, H_DIM).astype(np.float32)
    jobs = tuple((r, left, (mc if left else -mc) if r % 2 == 0 else 0.0) for r in range(len(ns)) for left in (1, 0))
    return _ro(pts, desc, np.array(ns, np.int32)) + (jobs,)


@pytest.mark.parametrize("cap", [1024, 300])
def test_half_img_oracle_vs_numpy(orc, cap):
    pts, desc, n, jobs = _half_case(cap)
    assert H_MC == 360.0
    carries = []
    for row, left, _ in jobs:
        x = pts[row, :n[row], 0]
        keep = (x < np.float32(H_W) - H_MC) if left else (x >= H_MC)
        assert np.array_equal(orc.half_img(pts[row, :n[row]], bool(left), H_W, H_FOV), np.nonzero(keep)[0])
        if n[row] >= 512:      # dense and empty chunks: the carry between the chunks runs from zero and from a full chunk
            per = [int(keep[c:c + 256].sum()) for c in range(0, int(n[row]), 256)]
            carries.append(per)
    if cap == 1024:
        assert any(p[0] == 256 and p[1] == 0 and p[2] > 0 for p in carries) and any(p[0] == 0 and p[1] > 0 for p in carries)
    x = pts[:, :, 0]
    assert (x == H_MC).any() and (x == np.float32(H_W) - H_MC).any()


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [1024, 300])
def test_half_compact_beyond_one_chunk_and_remap(orc, cap):
    import torch
    api, fe = _fe()
    dev = torch.device("cuda", 0)
    pts, desc, n, jobs = _half_case(cap)
    assert fe.half_move_cols(H_W, H_FOV) == float(H_MC)
    nj = len(jobs)
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)
    od = torch.full((nj, cap, H_DIM), 7.0, device=dev); op = torch.full((nj, cap, 2), 7.0, device=dev)
    om = torch.full((nj, cap), -1, dtype=torch.int32, device=dev); on = torch.full((nj,), -1, dtype=torch.int32, device=dev)
    d_desc, d_pts, d_n = t(desc), t(pts), t(n)
    d_jr, d_jl, d_js = t(np.array([j[0] for j in jobs], np.int32)), t(np.array([j[1] for j in jobs], np.int32)), t(np.array([j[2] for j in jobs], np.float32))
    args = lambda c: (d_desc.data_ptr(), d_pts.data_ptr(), d_n.data_ptr(), d_jr.data_ptr(), d_jl.data_ptr(), d_js.data_ptr(), nj, c, H_DIM, H_W, H_FOV,
                      od.data_ptr(), op.data_ptr(), om.data_ptr(), on.data_ptr())
    torch.cuda.synchronize()
    with pytest.raises(api.D2FEError):          # more points than the compaction's index table holds: refused, not launched
        fe.half_image_compact_device(*args(1025))
    fe.half_image_compact_device(*args(cap))
    fe.sync(); torch.cuda.synchronize()
    maps = om.cpu().numpy(); cnt = on.cpu().numpy()
    for j, (row, left, shift) in enumerate(jobs):
        ref_map = orc.half_img(pts[row, :n[row]], bool(left), H_W, H_FOV)
        k = int(cnt[j])
        assert k == len(ref_map) and np.array_equal(maps[j, :k], ref_map) and (maps[j, k:] == -1).all(), j
        assert np.array_equal(od[j, :k].cpu().numpy(), desc[row][ref_map]) and (od[j, k:] == 7).all().item()
        exp = pts[row][ref_map].copy(); exp[:, 0] = exp[:, 0] + np.float32(shift)
        assert np.array_equal(op[j, :k].cpu().numpy(), exp) and (op[j, k:] == 7).all().item()
    # the index remap over those maps: pair p maps its a-side through job ja[p] and its b-side through job jb[p]
    cap_match = 310
    rng = np.random.RandomState(cap + 1)
    ja = np.array([0, 1, 2, 3], np.int32); jb = np.array([1, 0, 3, 2], np.int32)
    assert cnt[:4].min() >= 1
    nm = np.array([0, 1, 300, cap_match + 5], np.int32)
    mq = np.stack([rng.randint(0, cnt[a], size=cap_match) for a in ja]).astype(np.int32)
    mt = np.stack([rng.randint(0, cnt[b], size=cap_match) for b in jb]).astype(np.int32)
    d_mq, d_mt, d_nm, d_ja, d_jb = t(mq), t(mt), t(nm), t(ja), t(jb)
    torch.cuda.synchronize()
    fe.remap_matches_device(d_mq.data_ptr(), d_mt.data_ptr(), d_nm.data_ptr(), d_ja.data_ptr(), d_jb.data_ptr(), om.data_ptr(), 4, cap_match, cap)
    fe.sync(); torch.cuda.synchronize()
    gq, gt = d_mq.cpu().numpy(), d_mt.cpu().numpy()
    for p in range(4):
        k = min(int(nm[p]), cap_match)                                           # a count beyond the capacity is clamped
        eq, et = mq[p].copy(), mt[p].copy()
        eq[:k] = maps[ja[p]][mq[p, :k]]; et[:k] = maps[jb[p]][mt[p, :k]]
        assert np.array_equal(gq[p], eq) and np.array_equal(gt[p], et), p
    fe.close()
