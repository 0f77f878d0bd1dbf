"""The host side of the int8 calibration session (include/d2fe.h, d2fe_calib_*) without a GPU: the three range rules of d2fe_calib_ranges on hand-made histograms,
through the development library's hook d2fe_debug_calib_ranges_from_hist, against tests/helpers/calib_oracle.py; and the argument checks a device is not needed for.

PERCENTILE and MINMAX are integer arithmetic plus one double product: bit for bit.  ENTROPY sums 128 .. n_bins doubles per candidate, and the library (sequential C
loops, libm's log) and the oracle (NumPy) may differ in the last bits of a KL value, so the acceptance is the one of the issue: the library's candidate must
minimise the ORACLE's KL up to the double-summation bound 4 * n_bins * 2^-53 * sum |p_b ln(p_b / q_b)| (evaluated by the oracle at both candidates), and where the
oracle's gap to the runner-up exceeds that bound the candidate must be the oracle's.  The range is then the header's edge of that candidate, bit for bit."""
import ctypes as C

import numpy as np
import pytest

from tests.helpers import calib_oracle as O

ERR_INVALID = -1


@pytest.fixture(scope="module")
def dev():
    from d2slam_amd import api, build
    build.build(dev=True)
    return api.DevFrontEnd


def _half_normal(n, seed, outliers=0, far=40.0):
    rng = np.random.RandomState(seed)
    x = np.abs(rng.randn(n)).astype(np.float32)
    if outliers:
        x[:outliers] = rng.uniform(6.0, far, outliers).astype(np.float32)
        x[0] = np.float32(far)
    return x


def _hist(x, n_bins):
    T, _ = O.frozen(O.t_max(x), n_bins)
    h, _, _ = O.binning(x, T, n_bins)
    return h, T


def _bits(v):
    return np.float32(v).view(np.uint32)


def _check_entropy(dev, hist, T):
    n_bins = len(hist)
    r, i = dev.calib_ranges_from_hist(hist, T, "entropy")
    ro, io, table = O.entropy(hist, T)
    assert i in table, "the library chose a candidate the rule skips: %d" % i
    bound = O.summation_bound(n_bins, table[i][1], table[io][1])
    print("n_bins %d: library i = %d, oracle i = %d, KL %.17g / %.17g, bound %.3g, %d of %d candidates valid" % (
        n_bins, i, io, table[i][0], table[io][0], bound, len(table), n_bins - O.LEVELS + 1))
    assert table[i][0] <= table[io][0] + bound
    others = sorted(v[0] for k, v in table.items() if k != io)
    if not others or others[0] - table[io][0] > bound:
        assert i == io
    assert _bits(r) == _bits(O.edge(i, T, n_bins))
    return r, i, table


def test_minmax_and_percentile_bit_for_bit(dev):
    x = _half_normal(200000, 1)
    for n_bins in (128, 2048, 4096):
        hist, T = _hist(x, n_bins)
        r, k = dev.calib_ranges_from_hist(hist, T, "minmax")
        assert _bits(r) == _bits(O.minmax(T)) and k == n_bins
        cum = np.cumsum(hist.astype(np.int64))
        N = int(cum[-1])
        exact = 100.0 * int(cum[n_bins // 3]) / N      # a target that lands on (or, after rounding, one above) a cumulative count
        for param in (100.0, 99.99, 99.0, 50.0, 1e-9, exact, np.nextafter(exact, 0.0), np.nextafter(exact, 200.0)):
            r, k = dev.calib_ranges_from_hist(hist, T, "percentile", param)
            ro, ko = O.percentile(hist, T, param)
            assert k == ko and _bits(r) == _bits(ro), (n_bins, param)
        r, k = dev.calib_ranges_from_hist(hist, T, "percentile", 100.0)
        assert k == n_bins and _bits(r) == _bits(T)      # the maximum itself lies in the last bin


def test_percentile_target_on_a_cumulative_count_and_a_single_bin(dev):
    n_bins, T = 256, np.float32(3.0)
    hist = np.zeros(n_bins, np.uint64)
    hist[10], hist[20], hist[255] = 50, 25, 25      # N = 100: 50 % is reached by bin 10 exactly, 50.5 % needs bin 20, 75 % is bin 20 exactly
    for param, want in ((50.0, 11), (50.5, 21), (75.0, 21), (75.5, 256), (100.0, 256), (1.0, 11)):
        r, k = dev.calib_ranges_from_hist(hist, T, "percentile", param)
        assert k == want == O.percentile(hist, T, param)[1] and _bits(r) == _bits(O.edge(want, T, n_bins)), param
    one = np.zeros(n_bins, np.uint64)
    one[77] = 12345
    for param in (0.001, 50.0, 100.0):
        r, k = dev.calib_ranges_from_hist(one, T, "percentile", param)
        assert k == 78 and _bits(r) == _bits(np.float32(78.0 * 3.0 / 256))


def test_entropy_half_normal(dev):
    hist, T = _hist(_half_normal(2000000, 2), 2048)
    r, i, table = _check_entropy(dev, hist, T)
    assert 2048 in table and i > 1024      # no outliers: the range stays near the maximum


def test_entropy_with_outliers_is_far_below_minmax(dev):
    """the property the feature exists for: 1e-4 of the mass spread out to 40 sets the MinMax range, the entropy range stays at the bulk"""
    x = _half_normal(2000000, 3, outliers=200)
    hist, T = _hist(x, 2048)
    assert T == np.float32(40.0)
    r, i, _ = _check_entropy(dev, hist, T)
    mm, _ = dev.calib_ranges_from_hist(hist, T, "minmax")
    print("entropy %.4f against minmax %.4f" % (r, mm))
    assert mm == np.float32(40.0) and r < 0.25 * mm
    p, _ = dev.calib_ranges_from_hist(hist, T, "percentile", 99.99)
    assert p < mm


def test_entropy_upper_half_empty_skips_candidates(dev):
    """the tensor's maximum always lies in the last bin: with nothing else above the middle, every candidate whose last level is empty while that one count is
    folded in has p > 0 and q = 0 there and is skipped"""
    n_bins = 2048
    x = _half_normal(300000, 4)
    x = x / x.max() * np.float32(0.45)
    x[0] = np.float32(1.0)
    hist, T = _hist(x, n_bins)
    assert T == np.float32(1.0) and hist[n_bins - 1] == 1 and hist[n_bins // 2:n_bins - 1].sum() == 0
    r, i, table = _check_entropy(dev, hist, T)
    assert len(table) < n_bins - 128 + 1 and n_bins in table


def test_entropy_empty_histogram_and_one_candidate(dev):
    T = np.float32(2.5)
    r, i = dev.calib_ranges_from_hist(np.zeros(2048, np.uint64), T, "entropy")
    assert i == 2048 and _bits(r) == _bits(T)
    r, i = dev.calib_ranges_from_hist(np.zeros(2048, np.uint64), T, "percentile", 99.0)
    assert i == 2048 and _bits(r) == _bits(T)
    hist, T = _hist(_half_normal(100000, 5, outliers=10), 128)
    r, i, table = _check_entropy(dev, hist, T)
    assert list(table) == [128] and i == 128 and _bits(r) == _bits(T)


def test_ranges_are_clamped(dev):
    one = np.zeros(128, np.uint64)
    one[0] = 1
    r, _ = dev.calib_ranges_from_hist(one, np.float32(1e-30), "percentile", 50.0)
    assert _bits(r) == _bits(np.float32(1e-30))
    r, _ = dev.calib_ranges_from_hist(one, np.float32(3e38), "minmax")
    assert _bits(r) == _bits(np.float32(1e30))


def test_argument_checks_need_no_device(dev):
    from d2slam_amd import api, build
    lib = C.CDLL(build.build())
    lib.d2fe_last_error.restype = C.c_char_p
    lib.d2fe_calib_ranges.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_void_p]
    out, r = C.c_void_p(), (C.c_float * 12)()
    for bad in (1, 127, 129, 100, 4224, -128):
        assert lib.d2fe_calib_create(None, bad, C.byref(out)) == ERR_INVALID and b"n_bins" in lib.d2fe_last_error()
    assert lib.d2fe_calib_create(None, 2048, C.byref(out)) == ERR_INVALID and not out.value
    assert lib.d2fe_calib_freeze(None) == ERR_INVALID
    assert lib.d2fe_calib_collect(None, None, 64, 64, 64, C.c_longlong(4096), 1) == ERR_INVALID
    for layer in (-1, 12):
        assert lib.d2fe_calib_stats_get(None, layer, None, None, None, None, None) == ERR_INVALID and b"layer" in lib.d2fe_last_error()
    assert lib.d2fe_calib_stats_get(None, 0, None, None, None, None, None) == ERR_INVALID
    for param in (0.0, -1.0, 100.0001, float("nan")):
        assert lib.d2fe_calib_ranges(None, 2, param, r) == ERR_INVALID and b"percentile" in lib.d2fe_last_error()
    assert lib.d2fe_calib_ranges(None, 3, 0.0, r) == ERR_INVALID and b"method" in lib.d2fe_last_error()
    assert lib.d2fe_calib_ranges(None, 0, 0.0, r) == ERR_INVALID
    lib.d2fe_calib_destroy(None)
    # the hook refuses the same
    hist = np.ones(2048, np.uint64)
    for kw in (dict(hist=hist[:100]), dict(hist=np.ones(4224, np.uint64)), dict(param=0.0), dict(param=100.5), dict(t=0.0), dict(t=float("inf")), dict(method=7)):
        a = dict(hist=hist, t=1.0, method="percentile", param=50.0)
        a.update(kw)
        with pytest.raises(api.D2FEError) as e:
            dev.calib_ranges_from_hist(a["hist"], a["t"], a["method"], a["param"])
        assert e.value.code == ERR_INVALID
