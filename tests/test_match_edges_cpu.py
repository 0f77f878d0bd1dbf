"""The references and the constructions of tests/test_match_edges.py, checked without a GPU.

For every integer case the oracle (orc.match_knn / orc.match_crosscheck, the restatement the matcher is held to bit for bit) equals a plain int64 brute force
(tests/helpers/match_ref.py) in indices and distance bits; orc.l2_dist is held to float64 at every compiled width; and every construction has the structure
its GPU test relies on: the exact window below 0.5, the tied rows of the slot cases in the intended shares, the neighbours of the pass cases in the
intended passes."""
import numpy as np
import pytest

from tests.helpers import match_ref as mr

NPAIRS_CPU = 10      # the first pairs of a two-wave batch (the GPU test's batch length follows the device's compute units)


def _same(got, want, what):
    assert len(got[0]) == len(want[0]), "%s: %d matches, the int64 reference has %d" % (what, len(got[0]), len(want[0]))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), "%s: indices differ" % what
    assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)), "%s: distance bits differ" % what


def _oracle_equals_int64(orc, a, b, pa, pb, what, radius=300.0):
    """-> number of matches compared"""
    w = mr.exact_window(a, b)
    assert w < 0.5, "%s: exact window %g" % (what, w)
    n = 0
    for ratio in (0.8, 1.5):
        want = mr.int_match_knn(a, b, ratio)
        _same(orc.match_knn(a, b, ratio), want, "%s, ratio %g" % (what, ratio)); n += len(want[0])
        if pa is not None and len(a) and len(b):
            want = mr.int_match_knn(a, b, ratio, pa, pb, radius)
            _same(orc.match_knn(a, b, ratio, pa, pb, radius), want, "%s, ratio %g, radius %g" % (what, ratio, radius)); n += len(want[0])
    if len(a) and len(b):
        want = mr.int_match_crosscheck(a, b)
        _same(orc.match_crosscheck(a, b), want, "%s, cross-check" % what); n += len(want[0])
    return n


# ---- the int64 reference itself ------------------------------------------------------------------------------------------------------------------------------

def test_int_reference_on_a_problem_worked_by_hand():
    a = np.array([[0, 0, 0, 0], [2, 2, 0, 0], [0, 0, 0, 1]], np.float32)
    b = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [2, 2, 0, 1], [0, 0, 0, 0]], np.float32)
    assert mr.int_d2(a, b).tolist() == [[1, 1, 9, 0], [5, 5, 1, 8], [2, 2, 8, 1]]
    i0, d0, i1, d1 = mr.int_knn(a, b)
    assert i0.tolist() == [3, 2, 3] and i1.tolist() == [0, 0, 0]                    # the tie 1 == 1 of query 0 and 2 == 2 of query 2 keep the lower index
    assert d0.tolist() == [0.0, 1.0, 1.0] and d1.tolist() == [1.0, np.sqrt(np.float32(5)), np.sqrt(np.float32(2))]
    # b -> a: row 0 -> (a0 1, a2 2); row 1 -> (a0 1, a2 2); row 2 -> (a1 1, a2 8); row 3 -> (a0 0, a2 1)
    q, t, d = mr.int_match_knn(a, b, 0.8)
    assert (q.tolist(), t.tolist(), d.tolist()) == ([0, 1], [3, 2], [0.0, 1.0])      # query 2 -> row 3, which names a0
    q, t, d = mr.int_match_crosscheck(a, b)
    assert (q.tolist(), t.tolist()) == ([0, 1], [3, 2])
    pa = np.array([[0, 0], [10, 10], [0, 0]], np.float32); pb = np.array([[0, 0], [0, 0], [13, 14], [0, 0]], np.float32)      # (3, 4) apart
    assert mr.int_match_knn(a, b, 0.8, pa, pb, 5.0)[0].tolist() == [0, 1]
    assert mr.int_match_knn(a, b, 0.8, pa, pb, float(np.nextafter(5.0, 0)))[0].tolist() == [0]
    assert mr.int_match_knn(a, b, 0.8, pa, pb, 0.0)[0].tolist() == [0, 1] and mr.int_match_knn(a, b, 0.8, pa, pb, -3.0)[0].tolist() == [0, 1]
    # fewer than two rows on a side: no 2-NN list has two entries (feature_matcher.cpp:18-20, :27-29)
    assert len(mr.int_match_knn(a[:1], b, 1.5)[0]) == 0 and len(mr.int_match_knn(a, b[:1], 1.5)[0]) == 0
    assert mr.int_match_crosscheck(a[:1], b)[1].tolist() == [3]
    assert len(mr.int_match_knn(a[:0], b)[0]) == 0 and len(mr.int_match_crosscheck(a, b[:0])[0]) == 0


def test_expected_counters_on_a_problem_worked_by_hand():
    """40 identical rows against 20 of the same: every query sees all rows tied.  a -> b: 20 hits (32 strip entries: four-wave shares of 4, two-wave shares of
    8) -> 20 hits, no share above 8 -> n = 20, a scan.  b -> a: 40 hits; four-wave shares of 8 (48 entries / 8 threads -> L = 8: 8 per share) -> n = 40;
    two-wave shares of 12 -> overflow -> n = 17."""
    a = np.ones((40, 8), np.float32); b = np.ones((20, 8), np.float32)
    assert (mr.share_length(20, 8), mr.share_length(20, 4), mr.share_length(40, 8), mr.share_length(40, 4), mr.share_length(256, 8), mr.share_length(256, 4)) == (4, 8, 8, 12, 32, 64)
    assert mr.expected_counters(a, b, 8) == (40 * 18 + 20 * 38, 60)
    assert mr.expected_counters(a, b, 4) == (40 * 18 + 20 * 15, 60)
    # distinct rows: two candidates per query, nothing counted; one train row: one candidate
    e = np.eye(8, dtype=np.float32) * np.arange(1, 9, dtype=np.float32)[:, None]
    assert mr.expected_counters(e, e[:5] * 2, 8) == (0, 0) and mr.expected_counters(e, e[:1], 4) == (0, 0)


# ---- every integer case: the oracle equals the int64 brute force ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", mr.WIDTHS)
def test_oracle_equals_int64_on_the_width_cases(orc, dim):
    a, b, pa, pb = mr.width_host_case("int", dim)
    n = _oracle_equals_int64(orc, a, b, pa, pb, "150 x 180 x %d" % dim)
    pairs, pts = mr.width_batch_case("int", dim, NPAIRS_CPU)
    assert [(len(x), len(y)) for x, y in pairs[:len(mr.BATCH_SHAPES)]] == mr.BATCH_SHAPES
    for p, ((x, y), (px, py)) in enumerate(zip(pairs, pts)):
        n += _oracle_equals_int64(orc, x, y, px, py, "pair %d (%d x %d x %d)" % (p, len(x), len(y), dim))
    assert n > 50


def test_width_batches_do_not_depend_on_their_length():
    for kind in ("int", "float"):
        short, _ = mr.width_batch_case(kind, 68, 7)
        long, _ = mr.width_batch_case(kind, 68, 9)
        assert all(np.array_equal(s[0], l[0]) and np.array_equal(s[1], l[1]) for s, l in zip(short, long))


@pytest.mark.parametrize("nt", mr.PASS_NT)
@pytest.mark.parametrize("dim", mr.PASS_DIMS)
def test_pass_cases_place_their_neighbours_and_equal_int64(orc, dim, nt):
    names = set()
    for a, b, plan in mr.pass_cases(dim, nt):
        assert a.shape == (mr.PASS_NQ, dim) and b.shape == (nt, dim)
        i0, d0, i1, d1 = mr.int_knn(a, b)
        d2 = mr.int_d2(a, b)
        for name, q, r0, r1 in plan:
            names.add(name)
            assert i0[q] == r0 and (r1 is None or i1[q] == r1), (name, q, int(i0[q]), int(i1[q]), r0, r1)
            p0, p1 = r0 // mr.SC, (r1 // mr.SC if r1 is not None else None)
            if name == "across_pass_1_and_2" and nt > mr.SC:
                assert {r0, r1} == {mr.SC - 1, mr.SC} and p0 != p1
            if name == "both_in_the_last_tile":
                assert r0 == nt - 1 and r0 // 16 == r1 // 16
            if name == "tie_of_the_nearest":
                assert d2[q, r0] == d2[q, r1] == 4 and r0 < r1 and (nt <= mr.SC or (p0 == 0 and p1 == (nt - 1) // mr.SC))
            if name == "tie_for_second":
                tied = np.nonzero(d2[q] == 5)[0]
                assert d2[q, r0] == 4 and len(tied) == 2 and tied[0] == r1 and (nt <= mr.SC or (tied[0] // mr.SC == 0 and tied[1] // mr.SC == (nt - 1) // mr.SC))
            if name == "nearest_in_the_last_pass":
                assert p0 == (nt - 1) // mr.SC and d2[q, :mr.SC * p0].min(initial=1 << 30) > 100
        _oracle_equals_int64(orc, a, b, None, None, "pass case %d x %d" % (nt, dim))
        _oracle_equals_int64(orc, b, a, None, None, "pass case %d x %d, swapped" % (nt, dim))
    want = {"across_pass_1_and_2", "tie_of_the_nearest", "tie_for_second", "nearest_in_the_last_pass"} | ({"both_in_the_last_tile"} if nt % 16 != 1 else set())
    assert names == want


@pytest.mark.parametrize("tpq", [8, 4])
@pytest.mark.parametrize("dim", mr.SLOT_DIMS)
def test_slot_cases_tie_the_intended_rows_in_the_intended_shares(orc, dim, tpq):
    a, b, plan = mr.slot_case(dim, tpq)
    assert a.shape == (mr.SLOT_NQ, dim) and b.shape == (mr.SLOT_NT, dim)
    L = mr.share_length(len(b), tpq)
    assert L == 256 // tpq
    d2 = mr.int_d2(a, b)
    assert [(sum(c), s) for _, _, c, s in plan] == [(16, False), (17, True), (8, False), (9, True), (16, False)]
    for name, q, per_share, scan in plan:
        hits = mr.query_hits(d2[q])
        assert np.array_equal(hits, d2[q] == 0), name                              # exactly the group ties, at distance zero
        assert np.bincount(np.nonzero(hits)[0] // L, minlength=tpq).tolist() == per_share, name
        assert scan == (max(per_share) > mr.SHMAX or sum(per_share) > mr.CMAX), name
    designated = {q for _, q, _, _ in plan}
    grouped = (d2[sorted(designated)] == 0).any(0)
    for q in range(len(a)):
        if q not in designated:
            hits = mr.query_hits(d2[q])
            assert hits.sum() <= 4 and not (hits & grouped).any()                      # an ordinary query: its two nearest and their ties, no group row among them
    extra, scans = mr.expected_counters(a, b, tpq)
    # the designated queries alone: 14 + 15 + 6 + 15 + 14 extra and two scans; the ordinary queries of both directions add their ties at second place only
    assert scans == 2 and 64 <= extra < 64 + len(a) + len(b)
    _oracle_equals_int64(orc, a, b, None, None, "slot case %d, tpq %d" % (dim, tpq))


@pytest.mark.parametrize("dim", mr.NORM_DIMS)
def test_zero_row_cases_equal_int64(orc, dim):
    a, b = mr.zero_rows_case(dim)
    assert not a[0].any() and not b[179].any()
    _oracle_equals_int64(orc, a, b, None, None, "zero rows, %d" % dim)
    z = np.zeros((150, dim), np.float32)
    assert mr.exact_window(z, z[:130]) == 0.0
    _oracle_equals_int64(orc, z, z[:130], None, None, "all zero, %d" % dim)
    assert len(orc.match_knn(z, z[:130], 1.5)[0]) == 0                              # every list is (row 0, row 1) at distance 0, and 0 < 1.5 * 0 is false
    q, t, d = orc.match_crosscheck(z, z[:130])
    assert q.tolist() == [0] and t.tolist() == [0] and d.tolist() == [0.0]          # only (0, 0) is mutual: the first of the tied rows on both sides


def test_offset_case_is_exact(orc):
    for dim in mr.NORM_DIMS:
        (a, b), (a8, b8) = mr.offset_case(dim)
        assert np.array_equal((a8.astype(np.float64) - 8.0), a.astype(np.float64)) and np.array_equal((b8.astype(np.float64) - 8.0), b.astype(np.float64))
        for ratio in (0.8, 1.5):
            r0, r8 = orc.match_knn(a, b, ratio), orc.match_knn(a8, b8, ratio)
            assert len(r0[0]) > 20 and all(np.array_equal(x, y) for x, y in zip(r0, r8))


# ---- orc.l2_dist against float64 ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", mr.WIDTHS)
def test_l2_dist_against_float64(orc, dim):
    """|d - d64| <= (dim / 16 + 24) 2^-24 d64.  Derived, not measured: in units of 2^-24 relative to the sum, every element carries 3 roundings (difference, square, its
    addition), an accumulator lane sees at most dim / 16 + 4 further additions (its own chain, the two reductions), the scalar tail at most 15; the square root
    halves the sum's relative error and adds one rounding."""
    for x, y in mr.l2_cases(dim):
        d = orc.l2_dist(x, y)
        d64 = float(np.sqrt(((x.astype(np.float64) - y.astype(np.float64)) ** 2).sum()))
        assert abs(d - d64) <= (dim / 16 + 24) * 2.0 ** -24 * d64, (dim, d, d64, abs(d - d64) / max(d64, 1e-300) * 2 ** 24)
        for s in (2.0 ** 12, 2.0 ** -12):       # a power of two scales every intermediate exactly
            assert orc.l2_dist((x * np.float32(s)).astype(np.float32), (y * np.float32(s)).astype(np.float32)) == np.float32(d) * np.float32(s)
