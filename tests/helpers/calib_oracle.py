"""The int8 calibration contract of include/d2fe.h (d2fe_calib_*) in NumPy: the binning in float32, the three range rules in float64.  The loops of the entropy
rule run in the header's order (np.cumsum sums sequentially, ascending); nothing here calls the library."""
import math

import numpy as np

LEVELS = 128
FLOOR, CEIL = np.float32(1e-30), np.float32(1e30)


def t_max(x):
    """max |x| as float32 (0 for an all-zero tensor)"""
    return np.float32(np.abs(np.asarray(x, np.float32)).max())


def frozen(tmax, n_bins):
    """(T, scale) of d2fe_calib_freeze"""
    T = np.float32(max(np.float32(tmax), FLOOR))
    return T, np.float32(np.float32(n_bins) / T)


def binning(x, T, n_bins):
    """-> (hist u64 [n_bins], n_zero, n_over) of the values x under T"""
    a = np.abs(np.asarray(x, np.float32)).ravel()
    T, scale = np.float32(T), np.float32(np.float32(n_bins) / np.float32(T))
    zero = a == 0
    over = (a > T) & ~zero
    rest = ~zero & ~over
    prod = a[rest] * scale      # one float32 multiply, round to nearest even
    assert prod.dtype == np.float32
    b = np.minimum(n_bins - 1, prod.astype(np.int64))      # truncation
    hist = np.bincount(b, minlength=n_bins).astype(np.uint64)
    hist[n_bins - 1] += np.uint64(int(over.sum()))
    return hist, int(zero.sum()), int(over.sum())


def _clamp(r):
    return np.float32(min(max(np.float32(r), FLOOR), CEIL))


def edge(k, T, n_bins):
    """the upper edge of bin k - 1 as the header rounds it; k = n_bins: T"""
    return _clamp(T) if k == n_bins else _clamp(np.float32(float(k) * float(np.float32(T)) / float(n_bins)))


def minmax(T):
    return _clamp(T)


def percentile(hist, T, param):
    """-> (range, b + 1)"""
    hist = [int(v) for v in hist]
    n_bins, N = len(hist), sum(hist)
    if N == 0:
        return _clamp(T), n_bins
    target = int(math.ceil(float(N) * (float(param) / 100.0)))
    cum, k = 0, n_bins
    for b, v in enumerate(hist):
        cum += v
        if cum >= target:
            k = b + 1
            break
    return edge(k, T, n_bins), k


def kl(hist, i):
    """the candidate i of the entropy rule: (KL(i), sum |p_b ln(p_b / q_b)|), or None when it is skipped"""
    hist = np.asarray(hist, np.uint64)
    n_bins = len(hist)
    P = hist[:i].astype(np.float64)
    P[i - 1] = float(int(hist[i - 1]) + int(hist[i:].astype(object).sum() if i < n_bins else 0))
    edges = (np.arange(LEVELS + 1, dtype=np.int64) * i) // LEVELS
    raw = np.add.reduceat(hist[:i].astype(np.int64), edges[:-1])      # integer sums over the raw histogram
    mask = P != 0
    cnt = np.add.reduceat(mask.astype(np.int64), edges[:-1])
    level = np.repeat(np.arange(LEVELS), np.diff(edges))
    with np.errstate(divide="ignore", invalid="ignore"):
        per = raw.astype(np.float64) / cnt.astype(np.float64)
    Q = np.where(mask, per[level], 0.0)
    sp, sq = np.cumsum(P)[-1], np.cumsum(Q)[-1]
    pos = P > 0
    if not sq > 0 or np.any(Q[pos] <= 0):
        return None
    p, q = P[pos] / sp, Q[pos] / sq
    terms = p * np.log(p / q)
    return float(np.cumsum(terms)[-1]), float(np.abs(terms).sum())


def entropy_table(hist):
    """{i: (KL, abs sum)} of every candidate that is not skipped"""
    n_bins = len(hist)
    out = {}
    for i in range(LEVELS, n_bins + 1):
        r = kl(hist, i)
        if r is not None:
            out[i] = r
    return out


def entropy(hist, T):
    """-> (range, i, table)"""
    n_bins = len(hist)
    if int(np.asarray(hist, np.uint64).astype(object).sum()) == 0:
        return _clamp(T), n_bins, {}
    table = entropy_table(hist)
    best = min(table, key=lambda i: (table[i][0], i))
    return edge(best, T, n_bins), best, table


def summation_bound(n_bins, *abs_sums):
    """the double-summation bound of the entropy acceptance: 4 * n_bins * 2^-53 * sum |p ln(p / q)|, at the larger of the candidates compared"""
    return 4.0 * n_bins * 2.0 ** -53 * max(abs_sums)
