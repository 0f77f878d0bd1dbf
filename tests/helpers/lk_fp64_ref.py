"""Independent fp64 numpy restatements of the LK family (tests/test_lk_edges.py): pyrDown, pyramidal sparse LK, good features.

The LK part is the PUBLISHED algorithm of cv::cuda::SparsePyrLKOpticalFlow as the reference calls it (opticaltrack_utils.cpp:173-279), not the
oracle's evaluation order: no 8x8 thread layout, no summation trees, no fp32 -- one (win+2)^2 patch of bilinear samples per level, whole-window numpy
sums, a 2x2 solve.  It exists so that a misreading shared by oracle/d2fe_oracle_lk.c and lk_device.h (a Scharr sign, a window off by one, status
written above level 0) shows up as a disagreement between two programs that share no code and no structure.

Measured on the point set of tests/test_lk_edges.py::test_lk_oracle_vs_fp64 (7 geometry sets, 308 points drawn from [-1, w+1] x [-1, h+1]):
  status disagreements oracle vs fp64 ......... 0 of 308      (cap LK_STATUS_CAP = 0.5 % of the points)
  worst |oracle - fp64| over tracks both accept  3.8e-6 px  (LK_MEASURED_PX; 187 of the 224 in-image points are accepted by both)
The coordinate differences are fp32 rounding carried through at most 30 iterations on at most 4 levels; one flipped |delta| < 0.01 stop decision moves a
converged track by far less than the bound.  The bound is the measured value times LK_MARGIN, never a guess."""
import numpy as np

LK_MEASURED_PX = 3.8e-6       # worst oracle-vs-fp64 coordinate difference measured on that point set (x86-64, the oracle's fp32 without FMA)
LK_MARGIN = 8.0
LK_TOL_PX = LK_MEASURED_PX * LK_MARGIN          # 3.04e-5 px
LK_STATUS_CAP = 0.005         # share of points whose status may differ (ill-conditioned accept / reject decisions); measured: 0
FLT_EPSILON = 1.1920928955078125e-07


# ---------------------------------------------------------------------------------------------------------------- pyramid
def reflect101(i, n):
    """BORDER_REFLECT_101 index (dcb|abcd|cba), repeated until it lands in [0, n): a 5-tap filter reflects twice on a 2-pixel level; n == 1 -> 0"""
    i = np.array(i, dtype=np.int64, copy=True)
    if n == 1:
        return np.zeros_like(i)
    while True:
        bad = (i < 0) | (i >= n)
        if not bad.any():
            return i
        i = np.where(i < 0, -i, i)
        i = np.where(i >= n, 2 * n - 2 - i, i)


def pyr_down_sums(img):
    """the exact integer 5x5 binomial sums (weights sum to 256) behind one pyrDown step, [ceil(h/2), ceil(w/2)]"""
    img = np.asarray(img)
    h, w = img.shape
    dh, dw = (h + 1) // 2, (w + 1) // 2
    k = np.array([1, 4, 6, 4, 1], np.int64)
    ys = reflect101(2 * np.arange(dh)[:, None] + np.arange(-2, 3)[None, :], h)
    xs = reflect101(2 * np.arange(dw)[:, None] + np.arange(-2, 3)[None, :], w)
    a = img.astype(np.int64)
    rows = (a[:, xs] * k).sum(-1)                                   # [h, dw]
    return (rows[ys, :] * k[None, :, None]).sum(1)                  # [dh, dw]


def pyr_down(img):
    """cv::cuda::pyrDown on u8: sum / 256 rounded half to even, saturated"""
    s = pyr_down_sums(img)
    return np.minimum(np.rint(s / 256.0), 255).astype(np.uint8)     # s / 256 is exact in fp64, np.rint rounds half to even


def pyr_exact_halves(img):
    """(quotient, y, x) of every output pixel whose sum lies exactly half-way between two integers"""
    s = pyr_down_sums(img)
    y, x = np.nonzero(s % 256 == 128)
    return [(int(s[a, b] // 256), int(a), int(b)) for a, b in zip(y, x)]


def pyr_build(img, levels):
    out = [np.ascontiguousarray(img, np.uint8)]
    for _ in range(levels):
        out.append(pyr_down(out[-1]))
    return out


# ---------------------------------------------------------------------------------------------------------------- LK
def _bilinear(im, u, v):
    """im fp64 [h, w] (pixel centres at integer coordinates), clamp-to-edge"""
    h, w = im.shape
    u0, v0 = np.floor(u), np.floor(v)
    fu, fv = u - u0, v - v0
    x0 = np.clip(u0, 0, w - 1).astype(np.int64); x1 = np.clip(u0 + 1, 0, w - 1).astype(np.int64)
    y0 = np.clip(v0, 0, h - 1).astype(np.int64); y1 = np.clip(v0 + 1, 0, h - 1).astype(np.int64)
    return (im[y0, x0] * (1 - fu) + im[y0, x1] * fu) * (1 - fv) + (im[y1, x0] * (1 - fu) + im[y1, x1] * fu) * fv


def lk_level(I, J, level, win, iters, prev_pt, guess, status, trace=None):
    """One pyramid level for one point.  I, J: u8 level images; prev_pt: level-0 coordinates; guess: the carried estimate in the coordinates of the level
    ABOVE (it is doubled on entry).  Returns (guess, status): both come back untouched from every early exit, except that an exit at level 0 clears status.
    trace, if given, collects (level, what) with what in {"prev_outside", "singular", "left_image", "done"}."""
    def leave(what):
        if trace is not None:
            trace.append((level, what))
        return guess, (0 if level == 0 else status)

    rows, cols = I.shape
    half = (win - 1) // 2
    p = np.asarray(prev_pt, np.float64) / float(1 << level)
    if p[0] < 0 or p[0] >= cols or p[1] < 0 or p[1] >= rows:
        return leave("prev_outside")
    Iq, Jq = I.astype(np.float64) / 255.0, J.astype(np.float64) / 255.0
    k = np.arange(-1, win + 1, dtype=np.float64)                              # the window and a 1-pixel ring for the derivatives
    S = _bilinear(Iq, (p[0] - half + k)[None, :], (p[1] - half + k)[:, None])
    Iw = S[1:-1, 1:-1]
    dx = 3 * S[:-2, 2:] + 10 * S[1:-1, 2:] + 3 * S[2:, 2:] - (3 * S[:-2, :-2] + 10 * S[1:-1, :-2] + 3 * S[2:, :-2])     # Scharr, unnormalised
    dy = 3 * S[2:, :-2] + 10 * S[2:, 1:-1] + 3 * S[2:, 2:] - (3 * S[:-2, :-2] + 10 * S[:-2, 1:-1] + 3 * S[:-2, 2:])
    G = np.array([[(dx * dx).sum(), (dx * dy).sum()], [(dx * dy).sum(), (dy * dy).sum()]])
    D = G[0, 0] * G[1, 1] - G[0, 1] * G[0, 1]
    if D < FLT_EPSILON:
        return leave("singular")
    Ginv = np.array([[G[1, 1], -G[0, 1]], [-G[0, 1], G[0, 0]]]) / D
    q = np.asarray(guess, np.float64) * 2.0 - half                             # top-left corner of the window in J
    kw = np.arange(win, dtype=np.float64)
    for _ in range(iters):
        if q[0] < -half or q[0] >= cols or q[1] < -half or q[1] >= rows:
            return leave("left_image")
        diff = (_bilinear(Jq, (q[0] + kw)[None, :], (q[1] + kw)[:, None]) - Iw) * 32.0
        delta = -Ginv @ np.array([(diff * dx).sum(), (diff * dy).sum()])
        q = q + delta
        if abs(delta[0]) < 0.01 and abs(delta[1]) < 0.01:
            break
    if trace is not None:
        trace.append((level, "done"))
    return q + half, status


def lk_calc(Ipyr, Jpyr, win, iters, prev_pt, guess, trace=None):
    """SparsePyrLKOpticalFlow::calc with useInitialFlow for one point: pyramids are lists of u8 images, level 0 first"""
    levels = len(Ipyr) - 1
    guess = np.asarray(guess, np.float64) / float(1 << levels) / 2.0
    status = 1
    for l in range(levels, -1, -1):
        guess, status = lk_level(Ipyr[l], Jpyr[l], l, win, iters, prev_pt, guess, status, trace)
    return guess, status


def in_border(pt, w, h):
    ix, iy = int(np.rint(pt[0])), int(np.rint(pt[1]))                          # cvRound: half to even
    return 1 <= ix < w - 1 and 1 <= iy < h - 1


def lk_track(prev_pyr, cur_pyr, prev_pts, cur_init, track_type=0, move_cols=0.0, win=21, iters=30, traces=None):
    """The tracking block of opticalflowTrackPyr: forward from cur_init, reverse from the (shifted) forward result, accept iff both succeed, the reverse
    track comes back to within 0.5 px and the forward result is inBorder.  Returns (cur_pts fp64 [n, 2], status u8 [n]).
    traces, if a list, gets one (forward trace, reverse trace) per point."""
    h, w = prev_pyr[0].shape
    prev_pts = np.asarray(prev_pts, np.float32).reshape(-1, 2).astype(np.float64)
    cur_init = np.asarray(cur_init, np.float32).reshape(-1, 2).astype(np.float64)
    mv = float(np.float32(move_cols))
    out = np.zeros_like(prev_pts); st = np.zeros(len(prev_pts), np.uint8)
    for i, (p, c) in enumerate(zip(prev_pts, cur_init)):
        tf, tr = [], []
        fwd, s_f = lk_calc(prev_pyr, cur_pyr, win, iters, p, c, tf)
        back = fwd.copy()
        if s_f == 1 and track_type == 1:
            back[0] -= mv
        if s_f == 1 and track_type == 2:
            back[0] += mv
        rev, s_r = lk_calc(cur_pyr, prev_pyr, win, iters, fwd, back, tr)
        ok = bool(s_f and s_r and np.hypot(*(p - rev)) <= 0.5)
        out[i] = fwd
        st[i] = 1 if ok and in_border(fwd, w, h) else 0
        if traces is not None:
            traces.append((tf, tr))
    return out, st


# ---------------------------------------------------------------------------------------------------------------- good features
def min_eigen(img):
    """cornerMinEigenVal(blockSize 3, Sobel 3, reflect-101), fp64: the smaller eigenvalue of the 3x3 box sum of the gradient covariance"""
    a = np.asarray(img).astype(np.float64)
    h, w = a.shape
    yy = reflect101(np.arange(-1, h + 1), h); xx = reflect101(np.arange(-1, w + 1), w)
    P = a[yy][:, xx]
    sc = 1.0 / (4 * 3 * 255.0)
    dx = sc * ((P[:-2, 2:] - P[:-2, :-2]) + 2 * (P[1:-1, 2:] - P[1:-1, :-2]) + (P[2:, 2:] - P[2:, :-2]))
    dy = sc * ((P[2:, :-2] + 2 * P[2:, 1:-1] + P[2:, 2:]) - (P[:-2, :-2] + 2 * P[:-2, 1:-1] + P[:-2, 2:]))

    def box(m):
        Q = m[yy][:, xx]
        return sum(Q[i:i + h, j:j + w] for i in range(3) for j in range(3))
    A, B, Cc = box(dx * dx) * 0.5, box(dx * dy), box(dy * dy) * 0.5
    return (A + Cc) - np.sqrt((A - Cc) ** 2 + B ** 2)


def corner_candidates(eig, quality):
    """interior pixels above quality * max that equal their 3x3 maximum, sorted by (value descending, raster index ascending): [(v, y, x)]"""
    h, w = eig.shape
    thr = np.float32(np.float64(eig.max() if eig.max() > 0 else 0.0) * quality)
    out = []
    for y in range(1, h - 1):
        for x in range(1, w - 1):
            v = eig[y, x]
            if v > thr and v == eig[y - 1:y + 2, x - 1:x + 2].max():
                out.append((v, y, x))
    out.sort(key=lambda c: (-c[0], c[1] * w + c[2]))
    return out


def greedy_min_dist(cands, min_dist, max_corners):
    """the definition the grid filter implements, by brute force: walk the sorted candidates, keep one iff it lies >= min_dist from everything kept"""
    kept = []
    for v, y, x in cands:
        if min_dist < 1 or all((x - a) ** 2 + (y - b) ** 2 >= min_dist * min_dist for a, b in kept):
            kept.append((x, y))
            if max_corners > 0 and len(kept) == max_corners:
                break
    return np.array(kept, np.float32).reshape(-1, 2)
