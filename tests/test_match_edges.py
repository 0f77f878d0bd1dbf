"""The matcher (csrc/match.hip) at every compiled width, at unequal norm scales and at its slot and pass boundaries, in both of its wave counts.

launch_match_nw picks one of four instantiations by width (<4,false> up to 64, <8,false> up to 128, <16,false> for 132..252, <16,true> at 256) and launch_match
one of two wave counts by launch size; the other matcher tests run widths 32, 64, 128 and 256 on unit-norm rows.  Here every test PROVES the kernel it means
to cover from the development library's launch-regime record (match_nw4 / match_nw2) and compares indices and distance bits with the oracle and, on
small-integer descriptors whose arithmetic is exact in any order, with a plain int64 brute force (tests/helpers/match_ref.py) that also gives the expected
values of the two diagnostic counters of d2fe_match_fallback_rows.  tests/test_match_edges_cpu.py checks those references and the constructions without a GPU.

A host call of at most 8192 rows takes the four-wave kernel; a two-wave launch at small shapes is ONE d2fe_match_batch_device call of P pairs whose
workgroups (2 ceil(max_n / 32) per pair) exceed twice the device's compute units."""
import json

import numpy as np
import pytest

from tests.helpers import match_ref as mr

pytestmark = pytest.mark.gpu

KNN08, KNN15, GATED, CROSS = ("matchKNN 0.8", 0, 0.8, -1.0), ("matchKNN 1.5", 0, 1.5, -1.0), ("matchKNN 0.8, radius 300", 0, 0.8, 300.0), ("cross-check", 1, 0.8, -1.0)
RUNS = [KNN08, KNN15, GATED, CROSS]


@pytest.fixture(scope="module")
def api():
    from d2slam_amd import api as a
    a.load_library(dev=True)
    return a


@pytest.fixture(scope="module")
def fe(api):
    h = api.DevFrontEnd(api.SuperPointConfig(max_keypoints=200, input_width=64, input_height=64, max_batch=1))
    yield h
    h.close()


def _ncu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _npairs(max_n):
    """the shortest batch at capacity max_n that no longer fits the device at once: 2 ceil(max_n / 32) P > 2 CUs"""
    per_pair = 2 * ((max_n + 31) // 32)
    return 2 * _ncu() // per_pair + 1


def _show(what, rec, **more):
    rec = {k: v for k, v in rec.items() if k.startswith("match_")}
    print("\n[match edges] %s: %s%s" % (what, json.dumps(rec), "".join("  %s %s" % kv for kv in more.items())), flush=True)


def _host(fe, a, b, run, pa=None, pb=None):
    _, mode, ratio, radius = run
    if mode == 1:
        return fe.match_crosscheck(a, b)
    return fe.match_knn(a, b, ratio, pa, pb, radius) if radius > 0 else fe.match_knn(a, b, ratio)


def _orc(orc, a, b, run, pa=None, pb=None):
    _, mode, ratio, radius = run
    if mode == 1:
        return orc.match_crosscheck(a, b)
    return orc.match_knn(a, b, ratio, pa, pb, radius) if radius > 0 else orc.match_knn(a, b, ratio)


def _int(a, b, run, pa=None, pb=None):
    _, mode, ratio, radius = run
    return mr.int_match_crosscheck(a, b) if mode == 1 else mr.int_match_knn(a, b, ratio, pa, pb, radius)


def _same(got, want, what):
    assert len(got[0]) == len(want[0]), "%s: %d matches, expected %d" % (what, len(got[0]), len(want[0]))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), "%s: indices differ" % what
    assert np.array_equal(np.asarray(got[2]).view(np.uint32), np.asarray(want[2]).view(np.uint32)), "%s: distance bits differ" % what


def _batch(api, fe, pairs, dim, cap, run, pts=None, **kw):
    _, mode, ratio, radius = run
    return mr.match_batch(api, fe, pairs, dim, cap, mode=mode, ratio=ratio, radius=radius, pts=pts if radius > 0 else None, **kw)


def _counters(fe):
    return tuple(fe.match_fallback_rows(reset=True, full=True))


# ---- 1. every compiled width, both wave counts -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("dim", mr.WIDTHS)
def test_every_width_in_the_four_wave_kernel(api, fe, orc, dim, kind):
    """150 x 180 rows by host call: matchKNN at ratio 0.8 and 1.5, with a radius gate, and the cross-check matcher.  Integer set: against the int64 reference and
    the oracle, and the counters of every launch as the reference predicts them; unit-norm float set with planted matches, duplicates, 1e-7 near-copies and
    a group of 12 identical rows: against the oracle (and the reference's own matchKNN where it is built) bitwise."""
    from oracle import ref
    a, b, pa, pb = mr.width_host_case(kind, dim)
    if kind == "int":
        assert mr.exact_window(a, b) < 0.5
        want_counters = mr.expected_counters(a, b, 8)
    api.DevFrontEnd.regime_reset()
    total, seen = 0, []
    for run in RUNS:
        fe.match_fallback_rows(reset=True)
        got = _host(fe, a, b, run, pa, pb)
        counters = _counters(fe)
        seen.append(counters)
        what = "%s, %s set, 150 x 180 x %d" % (run[0], kind, dim)
        _same(got, _orc(orc, a, b, run, pa, pb), what + " vs the oracle")
        if kind == "int":
            _same(got, _int(a, b, run, pa, pb), what + " vs int64")
            assert counters == want_counters, "%s: (extra, scans) %s, expected %s" % (what, counters, want_counters)
        elif run[1] == 0 and ref.available():
            _same(got, ref.match_knn(a, b, run[2], pa if run[3] > 0 else None, pb if run[3] > 0 else None, run[3]), what + " vs the reference's matchKNN")
        total += len(got[0])
    rec = api.DevFrontEnd.regime_counts()
    _show("(1) width %d, %s set, host calls" % (dim, kind), rec, measured=seen, expected=want_counters if kind == "int" else "-")
    assert total > 0
    assert rec["match_nw4"] == len(RUNS) and rec["match_nw2"] == 0, rec


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("dim", mr.WIDTHS)
def test_every_width_in_the_two_wave_kernel(api, fe, orc, dim, kind):
    """One batch per run at max_n = 64, long enough for the two-wave kernel: row counts random in 1..64 with (1, 64), (64, 1), (1, 1), (2, 2), (64, 64) and (33, 32)
    among them; the same data sets, runs and references as the four-wave test, every pair."""
    from oracle import ref
    cap = 64
    npairs = _npairs(cap)
    pairs, pts = mr.width_batch_case(kind, dim, npairs)
    if kind == "int":
        assert max(mr.exact_window(a, b) for a, b in pairs) < 0.5
        want_counters = tuple(int(v) for v in np.sum([mr.expected_counters(a, b, 4) for a, b in pairs], axis=0))
    api.DevFrontEnd.regime_reset()
    total, seen = 0, []
    for run in RUNS:
        fe.match_fallback_rows(reset=True)
        got = _batch(api, fe, pairs, dim, cap, run, pts)
        counters = _counters(fe)
        seen.append(counters)
        for p, ((a, b), (pa, pb)) in enumerate(zip(pairs, pts)):
            what = "%s, %s set, pair %d (%d x %d x %d)" % (run[0], kind, p, len(a), len(b), dim)
            _same(got[p], _orc(orc, a, b, run, pa, pb), what + " vs the oracle")
            if kind == "int":
                _same(got[p], _int(a, b, run, pa, pb), what + " vs int64")
            elif run[1] == 0 and ref.available():
                _same(got[p], ref.match_knn(a, b, run[2], pa if run[3] > 0 else None, pb if run[3] > 0 else None, run[3]), what + " vs the reference's matchKNN")
            total += len(got[p][0])
        if kind == "int":
            assert counters == want_counters, "%s, width %d: (extra, scans) %s, expected %s" % (run[0], dim, counters, want_counters)
    rec = api.DevFrontEnd.regime_counts()
    _show("(1) width %d, %s set, batches of %d pairs at max_n 64" % (dim, kind, npairs), rec, measured=seen, expected=want_counters if kind == "int" else "-")
    assert total > npairs
    assert rec["match_nw2"] == len(RUNS) and rec["match_nw4"] == 0, rec


# ---- 2. pass boundaries ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nt", mr.PASS_NT)
@pytest.mark.parametrize("dim", mr.PASS_DIMS)
def test_neighbours_and_ties_across_the_pass_boundary(api, fe, orc, dim, nt):
    """40 integer queries against nt train rows around one, two and three passes of 256: the nearest in the last row of pass 1 and the second in the first row of
    pass 2 and the reverse, both in the last tile, an exact tie of the nearest and of the second across two passes, the nearest in the last pass behind
    passes of far rows only (tests/helpers/match_ref.py: pass_cases).  Four waves by host call, as (a, b) and swapped; against the int64 reference."""
    api.DevFrontEnd.regime_reset()
    launches = 0
    for v, (a, b, plan) in enumerate(mr.pass_cases(dim, nt)):
        assert max(mr.exact_window(a, b), mr.exact_window(b, a)) < 0.5
        for x, y, order in ((a, b, "a, b"), (b, a, "b, a")):
            for run in (KNN08, KNN15, CROSS):
                got = _host(fe, x, y, run)
                launches += 1
                what = "%s, nt %d, dim %d, problem %d (%s) as (%s)" % (run[0], nt, dim, v, ", ".join(sorted({p[0] for p in plan})), order)
                want = _int(x, y, run)
                _same(got, want, what + " vs int64")
                _same(got, _orc(orc, x, y, run), what + " vs the oracle")
                if run is KNN15 and order == "a, b":      # every designated query is a match at ratio 1.5, and names its planted nearest row
                    for name, q, r0, _ in plan:
                        assert r0 in want[1][want[0] == q], (name, q, r0)
    rec = api.DevFrontEnd.regime_counts()
    _show("(2) nt %d, dim %d" % (nt, dim), rec)
    assert rec["match_nw4"] == launches and rec["match_nw2"] == 0, rec


# ---- 3. slot boundaries ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("waves", [4, 2])
@pytest.mark.parametrize("dim", mr.SLOT_DIMS)
def test_candidate_slots_at_their_limits(api, fe, orc, dim, waves):
    """256 train rows, one pass; designated queries equal a group of identical train rows laid out by the share length of the kernel under test (32 rows with four
    waves, 64 with two): 16 as 8 + 8 (no scan), 17 (scan), 8 in one share (no scan), 9 in one share (scan), 16 spread over every share (no scan).  Results equal
    the int64 reference, and (extra, scans) of every launch equal the helper's prediction from the test's own data; the two-wave batch holds the same problem
    P times, so its counters are P times one pair's."""
    tpq = 2 * waves
    a, b, plan = mr.slot_case(dim, tpq)
    assert mr.exact_window(a, b) < 0.5
    extra, scans = mr.expected_counters(a, b, tpq)
    assert scans == sum(1 for p in plan if p[3])
    npairs = 1 if waves == 4 else _npairs(256)
    api.DevFrontEnd.regime_reset()
    seen = []
    for run in (KNN08, KNN15, CROSS):
        fe.match_fallback_rows(reset=True)
        got = [_host(fe, a, b, run)] if waves == 4 else _batch(api, fe, [(a, b)] * npairs, dim, 256, run)
        counters = _counters(fe)
        seen.append(counters)
        want = _int(a, b, run)
        assert len(want[0]) >= 3
        for p, g in enumerate(got):
            _same(g, want, "%s, dim %d, %d waves, copy %d vs int64" % (run[0], dim, waves, p))
        assert counters == (npairs * extra, npairs * scans), "%s, dim %d, %d waves: (extra, scans) %s, expected %d x %s" % (run[0], dim, waves, counters, npairs, (extra, scans))
    rec = api.DevFrontEnd.regime_counts()
    _show("(3) slots, dim %d, %d waves, %d pair(s)" % (dim, waves, npairs), rec, measured=seen, expected=(npairs * extra, npairs * scans))
    assert rec["match_nw%d" % waves] == 3 and rec["match_nw%d" % (6 - waves)] == 0, rec


# ---- 4. norm scale -----------------------------------------------------------------------------------------------------------------------------------------------

def _float_runs(api, fe, orc, a, b, what):
    """the three runs by host call, each bitwise against the oracle -> their results"""
    out = []
    for run in (KNN08, KNN15, CROSS):
        got = _host(fe, a, b, run)
        _same(got, _orc(orc, a, b, run), "%s, %s vs the oracle" % (what, run[0]))
        out.append(got)
    return out


@pytest.mark.parametrize("dim", mr.NORM_DIMS)
def test_rows_of_another_scale(api, fe, orc, dim):
    """Both sets scaled by 2^12 and by 2^-12: the oracle's result, which is the unscaled problem's with every distance times the scale, exactly.  Only the queries
    scaled by 2^12: every train row is nearly equidistant from every query, and the exact scan must have run."""
    a, b = mr.norm_base(dim)
    api.DevFrontEnd.regime_reset()
    base = _float_runs(api, fe, orc, a, b, "unscaled, dim %d" % dim)
    assert len(base[0][0]) > 40
    for e in (12, -12):
        s = np.float32(2.0 ** e)
        scaled = _float_runs(api, fe, orc, a * s, b * s, "both sets x 2^%d, dim %d" % (e, dim))
        for g, w in zip(scaled, base):
            _same(g, (w[0], w[1], w[2] * s), "both sets x 2^%d, dim %d vs the unscaled problem" % (e, dim))
    fe.match_fallback_rows(reset=True)
    _float_runs(api, fe, orc, a * np.float32(4096.0), b, "queries x 2^12, dim %d" % dim)
    extra, scans = _counters(fe)
    rec = api.DevFrontEnd.regime_counts()
    _show("(4) scale, dim %d" % dim, rec, queries_x4096=(extra, scans))
    assert scans > 0, "rows of one set 4096 times the other's: the strip cannot separate the train rows, yet no query took the exact scan"
    assert rec["match_nw4"] == 12 and rec["match_nw2"] == 0, rec


@pytest.mark.parametrize("dim", mr.NORM_DIMS)
def test_common_offset_cancels_in_the_strip_not_in_the_result(api, fe, orc, dim):
    """Rows on a 2^-8 grid in [-1, 1] plus 8.0 in every element: element sums and differences are exact, so the result equals the unshifted problem's bit for bit
    while the Gram strip loses ten bits to the offset; the exact scan must have run."""
    (a, b), (a8, b8) = mr.offset_case(dim)
    api.DevFrontEnd.regime_reset()
    base = _float_runs(api, fe, orc, a, b, "unshifted, dim %d" % dim)
    assert len(base[0][0]) > 20
    fe.match_fallback_rows(reset=True)
    shifted = _float_runs(api, fe, orc, a8, b8, "shifted by 8, dim %d" % dim)
    extra, scans = _counters(fe)
    for g, w in zip(shifted, base):
        _same(g, w, "shifted by 8, dim %d vs the unshifted problem" % dim)
    rec = api.DevFrontEnd.regime_counts()
    _show("(4) offset 8, dim %d" % dim, rec, measured=(extra, scans))
    assert scans > 0
    assert rec["match_nw4"] == 6 and rec["match_nw2"] == 0, rec


@pytest.mark.parametrize("dim", mr.NORM_DIMS)
def test_passes_of_unequal_norm(api, fe, orc, dim):
    """600 train rows in three passes, rows 300..599 scaled by 32, neighbours planted among the small rows of the first pass and among the large rows: the final
    check of the header ("also covers multi-pass train sets with unequal norms"), as (a, b) and swapped."""
    a, b = mr.multipass_case(dim)
    api.DevFrontEnd.regime_reset()
    fwd = _float_runs(api, fe, orc, a, b, "600 train rows, dim %d" % dim)
    _float_runs(api, fe, orc, b, a, "600 query rows, dim %d" % dim)
    assert len(fwd[1][0]) >= 30
    rec = api.DevFrontEnd.regime_counts()
    _show("(4) three passes of unequal norm, dim %d" % dim, rec)
    assert rec["match_nw4"] == 6 and rec["match_nw2"] == 0, rec


@pytest.mark.parametrize("dim", mr.NORM_DIMS)
def test_zero_rows_and_zero_sets(api, fe, orc, dim):
    """Integer sets with all-zero rows on both sides, and two sets that are zero altogether: there slack == 0, the strip proves nothing, and the scan has to give
    the tied rows in index order (the cross-check matcher returns (0, 0) alone).  Results against int64 and the oracle, counters as predicted."""
    api.DevFrontEnd.regime_reset()
    z = np.zeros((150, dim), np.float32)
    seen = {}
    for what, a, b in (("zero rows", *mr.zero_rows_case(dim)), ("zero sets", z, z[:130])):
        assert mr.exact_window(a, b) < 0.5
        want_counters = mr.expected_counters(a, b, 8)
        for run in (KNN08, KNN15, CROSS):
            fe.match_fallback_rows(reset=True)
            got = _host(fe, a, b, run)
            counters = _counters(fe)
            _same(got, _int(a, b, run), "%s, dim %d, %s vs int64" % (what, dim, run[0]))
            _same(got, _orc(orc, a, b, run), "%s, dim %d, %s vs the oracle" % (what, dim, run[0]))
            assert counters == want_counters, "%s, dim %d, %s: (extra, scans) %s, expected %s" % (what, dim, run[0], counters, want_counters)
        seen[what] = want_counters
    assert seen["zero sets"] == (15 * 280, 280)          # every query of both directions overflows a share
    q, t, d = fe.match_crosscheck(z, z[:130])
    assert (q.tolist(), t.tolist(), d.tolist()) == ([0], [0], [0.0])
    rec = api.DevFrontEnd.regime_counts()
    _show("(4) zero rows, dim %d" % dim, rec, counters=seen)
    assert rec["match_nw4"] == 7 and rec["match_nw2"] == 0, rec


# ---- 5. counts in device memory ----------------------------------------------------------------------------------------------------------------------------------

def test_counts_of_zero_and_above_capacity_in_device_memory(api, fe, orc):
    """One two-wave batch at max_n = 64, width 68: pairs with a_cnt = 0, b_cnt = 0 and both (n_out = 0, nothing written, the neighbours unharmed) and a pair whose
    counts exceed max_n (read as max_n: the result of the first 64 rows) between ordinary pairs."""
    dim, cap = 68, 64
    npairs = _npairs(cap)
    pairs, _ = mr.width_batch_case("int", dim, npairs)
    pairs = [(a, b) for a, b in pairs]
    counts = [(len(a), len(b)) for a, b in pairs]
    rng = np.random.RandomState(77)
    zero_a, zero_b, zero_ab, over = 8, 9, 11, 13
    assert npairs > over + 2
    for p in (zero_a, zero_b, zero_ab, over, npairs - 1):
        pairs[p] = mr.int_pair(rng, cap, cap, dim)
    counts[zero_a] = (0, cap); counts[zero_b] = (cap, 0); counts[zero_ab] = (0, 0); counts[over] = (1000, cap + 1); counts[npairs - 1] = (cap + 1, 2 ** 30)
    api.DevFrontEnd.regime_reset()
    for run in (KNN08, KNN15, CROSS):
        q, t, d, n = _batch(api, fe, pairs, dim, cap, run, counts=counts, raw=True)
        for p, (a, b) in enumerate(pairs):
            what = "%s, pair %d, counts %s" % (run[0], p, counts[p])
            if p in (zero_a, zero_b, zero_ab):
                assert n[p] == 0, what            # (mr.match_batch has checked that nothing behind n_out is written)
                continue
            want = _int(a, b, run)
            _same((q[p, :n[p]], t[p, :n[p]], d[p, :n[p]]), want, what + " vs int64")
            _same((q[p, :n[p]], t[p, :n[p]], d[p, :n[p]]), _orc(orc, a, b, run), what + " vs the oracle")
            if p in (over, npairs - 1):
                assert len(want[0]) > 0
    rec = api.DevFrontEnd.regime_counts()
    _show("(5) counts in device memory, %d pairs" % npairs, rec)
    assert rec["match_nw2"] == 3 and rec["match_nw4"] == 0, rec


@pytest.mark.parametrize("npairs", [1, 2, 3, 4])
def test_small_grids_cover_every_remainder_of_the_item_mapping(api, fe, orc, npairs):
    """1, 2, 3 and 4 pairs at max_n = 32: grids of 2, 4, 6 and 8 workgroups, every remainder the XCD item mapping of match_kernel can see below one full round"""
    dim, cap = 132, 32
    rng = np.random.RandomState(880 + npairs)
    pairs = [mr.int_pair(rng, *shape, dim) for shape in [(32, 32), (17, 32), (32, 1), (5, 9)][:npairs]]
    api.DevFrontEnd.regime_reset()
    for run in (KNN08, KNN15, CROSS):
        got = _batch(api, fe, pairs, dim, cap, run)
        for p, (a, b) in enumerate(pairs):
            _same(got[p], _int(a, b, run), "%s, %d pairs, pair %d vs int64" % (run[0], npairs, p))
            _same(got[p], _orc(orc, a, b, run), "%s, %d pairs, pair %d vs the oracle" % (run[0], npairs, p))
    rec = api.DevFrontEnd.regime_counts()
    _show("(5) %d pair(s) at max_n 32" % npairs, rec)
    assert rec["match_nw4"] == 3 and rec["match_nw2"] == 0, rec


# ---- 6. the radius gate at the threshold -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("waves", [4, 2])
def test_radius_gate_at_the_threshold(api, fe, orc, waves):
    """Every mutual nearest pair has its points (3, 4) apart: radius 5.0 keeps every match (nr > radius is false), the float below 5.0 drops every one, radius 0
    and negative radii disable the gate.  Against the int64 reference and the oracle."""
    dim, n = 20, 48
    rng = np.random.RandomState(606)
    a = mr.int_set(rng, n, dim)
    perm = rng.permutation(n)
    b = np.stack([mr.bump(a[i], [int(rng.randint(0, dim))]) for i in perm])
    pa = rng.randint(0, 600, (n, 2)).astype(np.float32)
    pb = (pa[perm] + np.array([3, 4], np.float32)).astype(np.float32)
    free = mr.int_match_knn(a, b, 0.8)
    assert len(free[0]) >= 10 and np.array_equal(perm[free[1]], free[0])
    npairs = 1 if waves == 4 else _npairs(64)
    api.DevFrontEnd.regime_reset()
    for radius, kept in ((5.0, True), (float(np.nextafter(5.0, 0)), False), (0.0, True), (-1.0, True), (-5.0, True), (4.0, False), (1e9, True)):
        want = mr.int_match_knn(a, b, 0.8, pa, pb, radius)
        assert len(want[0]) == (len(free[0]) if kept else 0)
        _same(orc.match_knn(a, b, 0.8, pa, pb, radius), want, "the oracle, radius %r" % radius)
        if waves == 4:
            got = [fe.match_knn(a, b, 0.8, pa, pb, radius)]
        else:
            got = mr.match_batch(api, fe, [(a, b)] * npairs, dim, 64, ratio=0.8, radius=radius, pts=[(pa, pb)] * npairs)
        for p, g in enumerate(got):
            _same(g, want, "radius %r, %d waves, copy %d" % (radius, waves, p))
    rec = api.DevFrontEnd.regime_counts()
    _show("(6) radius gate, %d waves" % waves, rec)
    assert rec["match_nw%d" % waves] == 7 and rec["match_nw%d" % (6 - waves)] == 0, rec
