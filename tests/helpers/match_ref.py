"""Exact references and seeded case generators for the matcher (csrc/match.hip) -- tests/test_match_edges_cpu.py and tests/test_match_edges.py.

With small-integer descriptors the matcher's arithmetic is exact: every fp32 sum of the Gram strip, of the norms and of the oracle's accumulation is an
integer below 2^24 in any order, so a plain int64 brute force gives indices and distance bits of the expected result, and -- because the threshold window
tau - n2 stays below 1 (exact_window) -- the candidate set of a query is exactly {rows with d2 <= n2}, which gives the two diagnostic counters of
d2fe_match_fallback_rows as well.  NumPy only (match_batch, the one device launcher shared with tests/test_launch_regimes.py, imports torch when called)."""
import numpy as np

WIDTHS = [4, 20, 36, 64, 68, 100, 128, 132, 200, 252, 256]      # the ends of every instantiation's range of launch_match_nw and one width per instantiation that is no multiple of 16
SC, CMAX, SHMAX = 256, 16, 8                                     # match.hip: train rows per pass, candidate slots per query and pass, slots per scan thread's share
SENTINEL_I, SENTINEL_F = -777, -777.0                            # output prefill of match_batch


# ---- the int64 reference ------------------------------------------------------------------------------------------------------------------------------------

def int_d2(a, b):
    """[na, nb] int64 squared distances of integer-valued float32 rows"""
    a = np.asarray(a); b = np.asarray(b)
    ai = a.astype(np.int64); bi = b.astype(np.int64)
    assert np.array_equal(ai, a) and np.array_equal(bi, b), "integer-valued rows only"
    return (ai * ai).sum(1)[:, None] + (bi * bi).sum(1)[None, :] - 2 * (ai @ bi.T)


def int_knn(a, b):
    """The 2-NN of every row of a among the rows of b: (i0, d0, i1, d1); ascending distance, ties keep the lower index; distances are
    np.sqrt(np.float32(d2)); a missing neighbour is (-1, inf)."""
    d2 = int_d2(a, b)
    na, nb = d2.shape
    i0 = np.full(na, -1, np.int32); i1 = np.full(na, -1, np.int32)
    d0 = np.full(na, np.inf, np.float32); d1 = np.full(na, np.inf, np.float32)
    if nb >= 1:
        order = np.argsort(d2, axis=1, kind="stable")
        rows = np.arange(na)
        i0 = order[:, 0].astype(np.int32)
        assert d2.max(initial=0) < 2 ** 24
        d0 = np.sqrt(d2[rows, i0].astype(np.float32))
        if nb >= 2:
            i1 = order[:, 1].astype(np.int32)
            d1 = np.sqrt(d2[rows, i1].astype(np.float32))
    return i0, d0, i1, d1


def int_match_knn(a, b, ratio=0.8, pts_a=None, pts_b=None, radius=-1.0):
    """matchKNN, a naive transcription of feature_matcher.cpp:16-37 (as restated above orc_match_knn in oracle/d2fe_oracle.c): the inverse dictionary of the
    b -> a 2-NN lists that pass the ratio test (a list of fewer than two entries, na < 2, is skipped), then every a -> b list (nb < 2: skipped) that passes
    the ratio test in double, is named back by its train row and lies within the pixel radius (cv::norm of a Point2f difference: float differences, double
    sum and sqrt; the gate is off for radius <= 0)."""
    na, nb = len(a), len(b)
    q, t, d = [], [], []
    if na and nb:
        f0, fd0, _, fd1 = int_knn(a, b)
        g0, gd0, _, gd1 = int_knn(b, a)
        inv = np.full(nb, -1, np.int64)
        for j in range(nb):
            if na < 2:
                continue
            if float(gd0[j]) < ratio * float(gd1[j]):
                inv[j] = g0[j]
        for i in range(na):
            if nb < 2:
                continue
            if float(fd0[i]) < ratio * float(fd1[i]) and inv[f0[i]] == i:
                if radius > 0 and pts_a is not None and pts_b is not None:
                    dx = np.float32(pts_a[i][0]) - np.float32(pts_b[f0[i]][0]); dy = np.float32(pts_a[i][1]) - np.float32(pts_b[f0[i]][1])
                    if np.sqrt(float(dx) * float(dx) + float(dy) * float(dy)) > radius:
                        continue
                q.append(i); t.append(int(f0[i])); d.append(fd0[i])
    return np.array(q, np.int32), np.array(t, np.int32), np.array(d, np.float32)


def int_match_crosscheck(a, b):
    """cv::BFMatcher(NORM_L2, true).match as stated above orc_match_crosscheck: (i, j) iff j is the first minimum of row i and i the first minimum of row j"""
    q, t, d = [], [], []
    if len(a) and len(b):
        f0, fd0, _, _ = int_knn(a, b)
        g0, _, _, _ = int_knn(b, a)
        for i in range(len(a)):
            if f0[i] >= 0 and g0[f0[i]] == i:
                q.append(i); t.append(int(f0[i])); d.append(fd0[i])
    return np.array(q, np.int32), np.array(t, np.int32), np.array(d, np.float32)


def share_length(nt, tpq):
    """entries of one scan thread's contiguous share of a strip row of nt (<= 256) train rows: match.hip section (2), `L`"""
    return -(-(16 * -(-nt // 16)) // (4 * tpq)) * 4


def query_hits(d2row):
    """bool [nt]: the candidates of one query of an exact (integer) problem in ONE pass: rows with d2 <= n2, n2 the second smallest value (every row when
    there is one row)"""
    if len(d2row) < 2:
        return np.ones(len(d2row), bool)
    return d2row <= np.partition(d2row, 1)[1]


def expected_counters(a, b, tpq):
    """(extra, scans) that d2fe_match_fallback_rows reports after ONE single-pass pair (na, nb <= 256) of an exact integer problem, both directions; tpq: scan
    threads per query, 8 in the four-wave kernel and 4 in the two-wave kernel.

    The rule is the one of match.hip's header, item (2) ("every row with S <= tau ... is a CANDIDATE ...  A query with more than CMAX candidates in a pass
    ... takes an exact scan of every train row"), and of section (2) of match_kernel: per query the hits are the rows with d2 <= n2 (exact_window < 0.5 makes
    tau cut between two integers); the strip row is cut into tpq contiguous shares of L = share_length(nt, tpq) entries; a share with more than SHMAX = 8
    hits sets the overflow flag and the query counts n = CMAX + 1 = 17, otherwise n = the number of hits; n > CMAX = 16 makes the query scan
    (scans += 1); extra += max(0, n - 2)."""
    extra = scans = 0
    for q, t in ((a, b), (b, a)):
        nq, nt = len(q), len(t)
        assert nq <= SC and nt <= SC
        if nq == 0 or nt == 0:
            continue
        L = share_length(nt, tpq)
        d2 = int_d2(q, t)
        for i in range(nq):
            hits = query_hits(d2[i])
            per_share = np.bincount(np.nonzero(hits)[0] // L, minlength=tpq)
            n = CMAX + 1 if per_share.max() > SHMAX else int(hits.sum())
            extra += max(0, n - 2)
            scans += int(n > CMAX)
    return extra, scans


def exact_window(a, b):
    """An upper bound of tau - n2 over every query of both directions: 2 slack + 2e-5 (n2 + slack) with slack = GRAM_ERR (max |q|^2 + max |t|^2) and
    GRAM_ERR = 4e-5 (match.hip: tau = (n2 + slack) 1.00002 + slack).  Below 0.5 no integer lies in (n2, tau], fp32 rounding of tau included."""
    if len(a) == 0 or len(b) == 0:
        return 0.0
    na2 = float((np.asarray(a, np.float64) ** 2).sum(1).max()); nb2 = float((np.asarray(b, np.float64) ** 2).sum(1).max())
    slack = 4e-5 * (na2 + nb2)
    n2 = 0.0
    for q, t in ((a, b), (b, a)):
        if len(t) >= 2:
            n2 = max(n2, float(np.partition(int_d2(q, t), 1, axis=1)[:, 1].max()))
    return 2 * slack + 2e-5 * (n2 + slack)


# ---- generators -----------------------------------------------------------------------------------------------------------------------------------------------

def int_set(rng, n, dim):
    return rng.randint(-2, 3, (n, dim)).astype(np.float32)


def bump(row, coords):
    """a copy of row with every coordinate of coords changed by 1 (towards zero; a zero becomes 1): squared distance len(coords) from row"""
    out = np.array(row, np.float32)
    for c in coords:
        out[c] = row[c] - 1 if row[c] > 0 else row[c] + 1
    return out


def unit(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def points(rng, n):
    return (rng.rand(n, 2) * 640).astype(np.float32)


BATCH_SHAPES = [(1, 64), (64, 1), (1, 1), (2, 2), (64, 64), (33, 32)]      # the first pairs of every two-wave batch of the width cases


def batch_shape(rng, p, cap=64):
    na, nb = int(rng.randint(1, cap + 1)), int(rng.randint(1, cap + 1))
    return BATCH_SHAPES[p] if p < len(BATCH_SHAPES) else (na, nb)


def int_pair(rng, na, nb, dim):
    """integer sets from {-2..2}; half of the shorter side is planted in b: a copy of a query with one coordinate changed by 1"""
    a = int_set(rng, na, dim); b = int_set(rng, nb, dim)
    k = min(na, nb) // 2
    for j, i in enumerate(rng.permutation(na)[:k]):
        b[j] = bump(a[i], [int(rng.randint(0, dim))])
    return a, b


def float_pair(rng, na, nb, dim):
    """unit-norm float sets built as test_match_random_shapes_with_injected_duplicates (tests/test_gpu_parity.py) builds them: planted matches, a group of up to
    12 identical rows, 1e-7 near-copies on both sides, and an exact copy of a query among the train rows, twice"""
    a = unit(rng.randn(na, dim)); b = unit(rng.randn(nb, dim))
    k = min(na, nb) // 2
    if k:
        b[:k] = unit(a[rng.permutation(na)[:k]] + 0.08 * rng.randn(k, dim))
    for side in (a, b):
        n = len(side)
        if n >= 4:
            g = min(n, 12)
            side[rng.choice(n, g, replace=False)] = side[int(rng.randint(0, n))]
            i, j = rng.choice(n, 2, replace=False)
            side[i] = (side[j] + np.float32(1e-7) * rng.randn(dim)).astype(np.float32)
    if nb >= 2:
        b[0] = a[0]; b[nb - 1] = a[0]
    return a, b


def width_host_case(kind, dim):
    """150 x 180 rows (the four-wave kernel by host call): (a, b, pts_a, pts_b); kind "int" or "float" """
    rng = np.random.RandomState(7000 + dim + (0 if kind == "int" else 500))
    a, b = (int_pair if kind == "int" else float_pair)(rng, 150, 180, dim)
    return a, b, points(rng, 150), points(rng, 180)


def width_batch_case(kind, dim, npairs):
    """npairs pairs of 1..64 rows (one two-wave batch at max_n = 64), BATCH_SHAPES first: ([(a, b)], [(pts_a, pts_b)]).  The first pairs do not depend on npairs."""
    pairs, pts = [], []
    for p in range(npairs):
        rng = np.random.RandomState(9000 + 1000 * dim + 2 * p + (0 if kind == "int" else 1))
        na, nb = batch_shape(rng, p)
        pairs.append((int_pair if kind == "int" else float_pair)(rng, na, nb, dim))
        pts.append((points(rng, na), points(rng, nb)))
    return pairs, pts


# -- pass boundaries

PASS_DIMS = [256, 68]
PASS_NT = [255, 256, 257, 511, 512, 513]
PASS_NQ = 40


def _pass_constructions(nt):
    """[(name, train rows it occupies, builder)] for a train set of nt rows.  A builder writes its train rows and its queries (from index qi on) and returns
    [(query, nearest row, second row)].  Planted rows lie 4 (nearest) and 5 (second) coordinate steps from their query: at ratio 0.8 the match exists only
    if the second neighbour is MISSED (2 < 0.8 sqrt(5) is false), at ratio 1.5 it exists and names the nearest."""
    last, npass = nt - 1, -(-nt // SC)
    first_last = SC * (npass - 1)              # first row of the last pass
    e1, s2 = (SC - 1, SC) if npass > 1 else (nt - 4, nt - 3)      # last row of pass 1 | first row of pass 2 (one pass: two adjacent rows)
    out = []

    def across(a, b, qi, rng):                 # nearest in row e1 and second in row s2, and the reverse, around one base row
        v = int_set(rng, 1, a.shape[1])[0]
        b[e1] = v; b[s2] = bump(v, range(9))
        a[qi] = bump(v, range(4)); a[qi + 1] = bump(v, range(5))
        return [(qi, e1, s2), (qi + 1, s2, e1)]
    out.append(("across_pass_1_and_2", [e1, s2], across))

    if nt % 16 != 1:
        def tile(a, b, qi, rng):               # both neighbours in the partial (or last) tile of the train set
            b[last] = bump(a[qi], range(4)); b[last - 1] = bump(a[qi], range(10, 15))
            return [(qi, last, last - 1)]
        out.append(("both_in_the_last_tile", [last, last - 1], tile))

    lo, hi = 100, (first_last + (last - first_last) // 2 if npass > 1 else 180)      # a row of pass 1 | a row of the last pass
    def tie1(a, b, qi, rng):                   # the nearest twice, in two passes: the lower index is the nearest, the other the second
        b[lo] = bump(a[qi], range(4)); b[hi] = bump(a[qi], range(10, 14))
        return [(qi, lo, hi)]
    out.append(("tie_of_the_nearest", [lo, hi], tie1))

    lo2, hi2 = 120, (first_last + (last - first_last) // 3 if npass > 1 else 200)
    def tie2(a, b, qi, rng):                   # the second twice, in two passes
        b[60] = bump(a[qi], range(4)); b[lo2] = bump(a[qi], range(10, 15)); b[hi2] = bump(a[qi], range(20, 25))
        return [(qi, 60, lo2)]
    out.append(("tie_for_second", [60, lo2, hi2], tie2))

    r5 = first_last + (2 * (last - first_last)) // 3
    def late(a, b, qi, rng):                   # both neighbours in the last pass, every earlier pass holds far rows only
        rows = [r5, r5 + 1] if r5 + 1 <= last else [r5]
        b[r5] = bump(a[qi], range(4))
        if len(rows) == 2:
            b[r5 + 1] = bump(a[qi], range(10, 15))
        return [(qi, r5, r5 + 1 if len(rows) == 2 else None)]
    out.append(("nearest_in_the_last_pass", [r5, r5 + 1] if r5 + 1 <= last else [r5], late))
    return out


def pass_cases(dim, nt):
    """[(a [40, dim], b [nt, dim], plan)]: the pass-boundary constructions for a train set of nt rows, packed into as few problems as their train rows
    allow (a last pass of one row serves one construction per problem).  plan: [(name, query, nearest row, second row or None)]."""
    rng = np.random.RandomState(31000 + 7 * dim + nt)
    variants = []
    for name, rows, build in _pass_constructions(nt):
        assert len(set(rows)) == len(rows) and all(0 <= r < nt for r in rows), (name, rows, nt)
        for v in variants:
            if not (v["used"] & set(rows)):
                break
        else:
            v = {"a": int_set(rng, PASS_NQ, dim), "b": int_set(rng, nt, dim), "used": set(), "qi": 3, "plan": []}
            variants.append(v)
        v["used"] |= set(rows)
        made = build(v["a"], v["b"], v["qi"], rng)
        v["plan"] += [(name, q, r0, r1) for q, r0, r1 in made]
        v["qi"] += len(made) + 2
    return [(v["a"], v["b"], v["plan"]) for v in variants]


# -- slot boundaries

SLOT_DIMS = [256, 132]
SLOT_NQ, SLOT_NT = 40, 256
SLOT_GROUPS = {8: [("16_as_8_8", [8, 8], False), ("17", [8, 8, 1], True), ("8_in_one_share", [8], False), ("9_in_one_share", [9], True), ("16_as_2_per_share", [2] * 8, False)],
               4: [("16_as_8_8", [8, 8], False), ("17", [8, 8, 1], True), ("8_in_one_share", [8], False), ("9_in_one_share", [9], True), ("16_as_4_per_share", [4] * 4, False)]}


def slot_case(dim, tpq):
    """(a [40, dim], b [256, dim], plan): one single-pass problem whose designated queries each equal a group of identical train rows, laid out by the share
    length of the kernel with tpq scan threads per query (256 / tpq rows).  plan: [(name, query, rows per share [tpq], scans?)]"""
    rng = np.random.RandomState(52000 + dim + tpq)
    a = int_set(rng, SLOT_NQ, dim); b = int_set(rng, SLOT_NT, dim)
    L = share_length(SLOT_NT, tpq)
    assert L * tpq == SLOT_NT
    fill = [0] * tpq                 # rows already taken at the END of every share (the groups sit against the share boundaries)
    share, plan = 0, []
    for k, (name, counts, scan) in enumerate(SLOT_GROUPS[tpq]):
        q = 2 + 3 * k
        a[q] = rng.choice([-2.0, 2.0], dim).astype(np.float32)      # |x| = 2 everywhere: about 6 dim from an ordinary row (they are 4 dim from each other), so no ordinary query ties on a group
        per_share = [0] * tpq
        for c in counts:
            s = share % tpq
            for _ in range(c):
                fill[s] += 1
                b[(s + 1) * L - fill[s]] = a[q]
            per_share[s] += c
            share += 1
        plan.append((name, q, per_share, scan))
    assert max(fill) < L - 4
    for k, q in enumerate([0, 1, 3, 4, 6, 7, 9, 10, 12, 13]):      # ordinary matches, at the front of the shares
        b[(k % tpq) * L + k // tpq] = bump(a[q], [int(rng.randint(0, dim))])
    return a, b, plan


# -- norm scale (float, against the oracle)

NORM_DIMS = [256, 132]


def norm_base(dim):
    rng = np.random.RandomState(64000 + dim)
    a = unit(rng.randn(150, dim)); b = unit(rng.randn(180, dim))
    b[:70] = unit(a[rng.permutation(150)[:70]] + 0.08 * rng.randn(70, dim))
    b[100] = a[9]; b[179] = a[9]
    return a, b


def offset_case(dim):
    """rows quantized to multiples of 2^-8 in [-1, 1]: (a, b) and (a + 8, b + 8); sums and differences of the elements are exact, so the exact distances of
    the two problems are the same numbers while the Gram strip of the shifted one cancels ten bits.  70 queries have one near row (every element moved by up
    to 12 / 256: d2 about 8e-4 dim); queries 0..3 have twenty such rows each (repeated texture).  Unshifted, |q|^2 + |t|^2 is about 2 dim / 3 and slack about
    2.7e-5 dim, of the order of the spread of the twenty d2; shifted by 8 the norms are about 129 dim and slack about 5e-3 dim, several times the d2 of ALL
    twenty: more than CMAX rows within the threshold, which only the exact scan can rank"""
    rng = np.random.RandomState(65000 + dim)
    a = (rng.randint(-256, 257, (150, dim)) / 256.0).astype(np.float32); b = (rng.randint(-256, 257, (180, dim)) / 256.0).astype(np.float32)
    k = rng.permutation(150)[:70]
    b[:70] = np.clip(a[k] + rng.randint(-12, 13, (70, dim)) / 256.0, -1, 1).astype(np.float32)
    for i in range(4):
        b[70 + 20 * i:90 + 20 * i] = np.clip(a[i] + rng.randint(-12, 13, (20, dim)) / 256.0, -1, 1).astype(np.float32)
    return (a, b), ((a + np.float32(8.0)).astype(np.float32), (b + np.float32(8.0)).astype(np.float32))


def multipass_case(dim):
    """nt = 600: rows 300..599 scaled by 32; queries 0..19 are near small rows of the first pass, queries 20..39 (scaled by 32) near large rows"""
    rng = np.random.RandomState(66000 + dim)
    a = unit(rng.randn(150, dim)); b = unit(rng.randn(600, dim))
    b[300:] *= np.float32(32.0)
    for i in range(20):
        b[5 + 11 * i] = unit(a[i:i + 1] + 0.05 * rng.randn(1, dim))[0]                 # rows 5..214: the first pass
        b[16 + 11 * i] = unit(a[i:i + 1] + 0.10 * rng.randn(1, dim))[0]
    for i in range(20, 40):
        a[i] *= np.float32(32.0)
        b[300 + 13 * (i - 20)] = unit(a[i:i + 1] + 32 * 0.05 * rng.randn(1, dim))[0] * np.float32(32.0)      # rows 300..547: second and third pass
        b[306 + 13 * (i - 20)] = unit(a[i:i + 1] + 32 * 0.10 * rng.randn(1, dim))[0] * np.float32(32.0)
    return a, b


def zero_rows_case(dim):
    """integer sets with some all-zero query rows and some all-zero train rows"""
    rng = np.random.RandomState(67000 + dim)
    a, b = int_pair(rng, 150, 180, dim)
    a[[0, 31, 32, 149]] = 0; b[[0, 15, 16, 100, 179]] = 0
    return a, b


def l2_cases(dim):
    """[(x, y)] float rows for orc.l2_dist against float64: unit rows, a near pair, a 1e-7 near-copy, a copy, and the same scaled by 2^12 and 2^-12"""
    rng = np.random.RandomState(68000 + dim)
    x = unit(rng.randn(6, dim)); y = unit(rng.randn(6, dim))
    y[1] = unit(x[1:2] + 0.05 * rng.randn(1, dim))[0]
    y[2] = (x[2] + np.float32(1e-7) * rng.randn(dim)).astype(np.float32)
    y[3] = x[3]
    out = []
    for s in (1.0, 2.0 ** 12, 2.0 ** -12):
        out += [((x[i] * np.float32(s)).astype(np.float32), (y[i] * np.float32(s)).astype(np.float32)) for i in range(6)]
    out += [((x[4] * np.float32(4096.0)).astype(np.float32), y[4])]      # rows of unequal scale
    return out


# ---- the batched device launch --------------------------------------------------------------------------------------------------------------------------------

def match_batch(api, fe, pairs, dim, cap, mode=0, ratio=0.8, radius=-1.0, pts=None, counts=None, raw=False):
    """pairs: [(a, b)] -> [(q, t, dist)] through ONE d2fe_match_batch_device launch (pool form); pts: [(pa, pb)] for the radius gate.  counts: [(a_cnt, b_cnt)]
    written to device memory instead of the row counts (rows past len(a) / len(b) are zero).  The outputs are prefilled with a sentinel and nothing behind
    n_out[p] may be written; raw=True returns (q, t, dist, n) whole instead."""
    import torch
    dev = torch.device("cuda", 0)
    npairs = len(pairs)
    pool = np.zeros((2 * npairs, cap, dim), np.float32); cnts = np.zeros(2 * npairs, np.int32)
    ppool = np.zeros((2 * npairs, cap, 2), np.float32)
    for p, (a, b) in enumerate(pairs):
        pool[2 * p, :len(a)] = a; pool[2 * p + 1, :len(b)] = b; cnts[2 * p] = len(a); cnts[2 * p + 1] = len(b)
        if counts is not None:
            cnts[2 * p], cnts[2 * p + 1] = counts[p]
        if pts is not None:
            ppool[2 * p, :len(a)] = pts[p][0]; ppool[2 * p + 1, :len(b)] = pts[p][1]
    d_pool = torch.from_numpy(pool).to(dev); d_cnt = torch.from_numpy(cnts).to(dev); d_pts = torch.from_numpy(ppool).to(dev)
    a_off = torch.arange(0, 2 * npairs, 2, dtype=torch.int32, device=dev) * cap
    b_off = a_off + cap
    a_cnt = d_cnt[0::2].contiguous(); b_cnt = d_cnt[1::2].contiguous()
    q = torch.full((npairs, cap), SENTINEL_I, dtype=torch.int32, device=dev); t = torch.full_like(q, SENTINEL_I)
    d = torch.full((npairs, cap), SENTINEL_F, dtype=torch.float32, device=dev); n = torch.full((npairs,), SENTINEL_I, dtype=torch.int32, device=dev)
    fe.match_batch_device(d_pool.data_ptr(), d_pool.data_ptr(), a_off.data_ptr(), b_off.data_ptr(), a_cnt.data_ptr(), b_cnt.data_ptr(), npairs, dim, cap,
                          q.data_ptr(), t.data_ptr(), d.data_ptr(), n.data_ptr(), mode=mode, ratio=ratio, radius=radius,
                          d_pts_a=d_pts.data_ptr() if pts is not None else None, d_pts_b=d_pts.data_ptr() if pts is not None else None,
                          stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    q, t, d, n = q.cpu().numpy(), t.cpu().numpy(), d.cpu().numpy(), n.cpu().numpy()
    for p in range(npairs):
        assert 0 <= n[p] <= cap, "pair %d: n_out = %d" % (p, n[p])
        assert np.all(q[p, n[p]:] == SENTINEL_I) and np.all(t[p, n[p]:] == SENTINEL_I) and np.all(d[p, n[p]:] == np.float32(SENTINEL_F)), \
            "pair %d: written behind n_out = %d" % (p, n[p])
    if raw:
        return q, t, d, n
    return [(q[p, :n[p]], t[p, :n[p]], d[p, :n[p]]) for p in range(npairs)]
