"""The LK tracker, pyramid, FAST and corner kernels (d2slam_amd/csrc/lk.hip, lk_device.h) at their edges.

CPU part: the oracle (oracle/d2fe_oracle_lk.c) against restatements that share nothing with it -- tests/helpers/lk_fp64_ref.py (fp64 pyramidal LK written
from the published algorithm, pyrDown with a reflect-101 that handles 1- and 2-pixel levels, fp64 min-eigenvalue corners with a brute-force min-distance
walk) and tests/test_lk.py::_fast_by_region_np.  GPU part (-m gpu): the product entry points against the oracle, bit for bit, at the shapes where the
kernels change path: the 3x3-per-lane window guards (win 3..23), the last workgroup (n % 4 != 0, n = 1), levels that shrink to 2x2 and 1x1, points on
and beyond every border, the inBorder rounding, widths 64 / 65 around the 64-lane row blocks, the 1024-pixel FAST chunks and the `features` cap, ties.

Two things a reader might expect and will not find:
  * flat frames do NOT return the input guess: every level leaves on D < eps without touching the carried guess (cv::cuda::SparsePyrLKOpticalFlow does the
    same), so the guess is never doubled on the way down and the output is cur_init * 2^-(levels+1), exactly.  The test asserts status 0 and that value;
  * FAST on 14x21 with 3x2 regions runs on the CPU side only: d2fe_lk_frame_create refuses images below 16x16.  The GPU test asserts the refusal and
    runs 16x21 with 3x2 regions (7 x 8 px regions, one interior row) beside it."""
import ctypes as C
import functools

import numpy as np
import pytest

from d2slam_amd.synth import synth_image
from tests.helpers import lk_fp64_ref as ref
from tests.test_lk import _fast_by_region_np, _fast_strength_np


# ---------------------------------------------------------------------------------------------------------------- inputs
def _pair(h, w, seed, dx=1, dy=2, mx=0):
    """two crops of one synthetic image: the content of `cur` is the content of `prev` moved by (+dx, +dy); mx: margin for large horizontal moves"""
    m = 4 + abs(mx)
    base = synth_image(h + 8, w + 2 * m, seed)
    return base[4:4 + h, m:m + w].copy(), base[4 - dy:4 - dy + h, m - dx:m - dx + w].copy()


def _dots(h, w, seed, height=None):
    """isolated bright pixels every 4 px on a dark background; height None: random heights"""
    rng = np.random.RandomState(seed)
    img = np.full((h, w), 7, np.uint8)
    ys, xs = np.mgrid[1:h:4, 1:w:4]
    img[ys, xs] = height if height is not None else rng.randint(30, 256, ys.shape)
    return img


def _noise(h, w, seed):
    return (np.random.RandomState(seed).randint(0, 2, (h, w)) * 255).astype(np.uint8)


def _fast_image(kind, h, w, seed=5):
    return {"synth": lambda: synth_image(h, w, seed), "dots": lambda: _dots(h, w, seed), "flatdots": lambda: _dots(h, w, seed, 200),
            "noise": lambda: _noise(h, w, seed)}[kind]()


# the (h, w, levels, win, type) sets of the oracle-vs-fp64 comparison, 44 points each
LK_SETS = ((48, 64, 2, 21, 0), (33, 47, 3, 9, 0), (16, 16, 2, 5, 0), (40, 40, 0, 23, 0), (64, 48, 2, 21, 0), (48, 64, 2, 21, 1), (48, 64, 2, 21, 2))
LK_MOVE = 12.0


def _lk_set(k):
    h, w, levels, win, ttype = LK_SETS[k]
    rng = np.random.RandomState(100 + k)
    shift = {0: (1 + k % 2, 2 - k % 2), 1: (int(LK_MOVE) + 1, 1), 2: (-int(LK_MOVE) + 1, 2)}[ttype]
    prev, cur = _pair(h, w, 200 + k, shift[0], shift[1], mx=shift[0])
    pts = np.stack([rng.uniform(-1, w + 1, 44), rng.uniform(-1, h + 1, 44)], 1).astype(np.float32)
    init = pts.copy()
    init[:, 0] += {0: 0.0, 1: LK_MOVE, 2: -LK_MOVE}[ttype]
    return prev, cur, pts, init, levels, win, ttype, (LK_MOVE if ttype else 0.0)


# FAST / good-features shapes shared by the CPU and the GPU tests
FAST_SINGLE = ((38, 38), (38, 39), (37, 38), (45, 100))
FAST_MULTI = ((64, 64, 9, 9), (14, 21, 3, 2), (16, 21, 3, 2), (76, 77, 2, 2), (131, 67, 3, 5), (16, 16, 3, 1), (20, 40, 2, 3))   # (h, w, cols, rows)
FAST_KINDS = ("synth", "dots", "noise")
GFTT_SIZES = ((16, 16), (17, 65), (64, 21), (48, 48), (18, 64))           # widths 65 and 64: one lane into / exactly at the second row block
GFTT_DISTS = (0.0, 0.99, 1.0, 1.5, 2.5, 5.0)
GFTT_MAXC = (0, 1, 7)


def _first_chunk_corners(img, thr):
    """corners the numpy reference finds in the first 1024 interior raster pixels of a single-region image"""
    h, w = img.shape
    return int((_fast_strength_np(img)[3:h - 3, 3:w - 3].ravel()[:1024] > thr).sum())


def _fast_single_cases():
    for (h, w) in FAST_SINGLE:
        for kind in FAST_KINDS:
            img = _fast_image(kind, h, w)
            for thr in (0, 10, 254):
                k = _first_chunk_corners(img, thr)
                for feats in sorted({k, k - 1, k + 1, 1, 2000}):
                    if feats >= 1:
                        yield img, feats, 1, 1, thr


def _fast_multi_cases():
    for (h, w, cols, rows) in FAST_MULTI:
        for kind in FAST_KINDS + ("flatdots",):
            img = _fast_image(kind, h, w)
            for thr, feats in ((10, 2000), (0, 3), (254, 1), (10, 1)):
                yield img, feats, cols, rows, thr


def _gftt_image(kind, h, w):
    if kind == "flat":
        return np.full((h, w), 90, np.uint8)
    if kind == "square":
        img = np.full((h, w), 20, np.uint8); img[5:11, 6:12] = 220
        return img
    if kind == "dots":                                      # spacing 3 along x, 4 along y: (3, 4) neighbours lie exactly 5 px apart
        img = np.full((h, w), 7, np.uint8); img[2:h - 2:4, 2:w - 2:3] = 200
        return img
    return synth_image(h, w, 9)


GFTT_KINDS = ("flat", "square", "dots", "synth")


# ---------------------------------------------------------------------------------------------------------------- CPU: oracle vs independent references
def test_reflect101_repeats_and_handles_one_pixel():
    assert ref.reflect101(np.arange(-2, 3), 1).tolist() == [0, 0, 0, 0, 0]
    assert ref.reflect101(np.arange(-2, 4), 2).tolist() == [0, 1, 0, 1, 0, 1]              # -2 and 3 reflect twice
    assert ref.reflect101(np.arange(-2, 7), 5).tolist() == [2, 1, 0, 1, 2, 3, 4, 3, 2]


def test_lk_oracle_vs_fp64(orc):
    """oracle/d2fe_oracle_lk.c against the fp64 restatement of the published algorithm: status on all points, coordinates on tracks both accept"""
    n = bad = inside = accepted = 0
    worst = 0.0
    for k in range(len(LK_SETS)):
        prev, cur, pts, init, levels, win, ttype, mv = _lk_set(k)
        h, w = prev.shape
        o_xy, o_st = orc.lk_track(orc.pyr_build(prev, levels), orc.pyr_build(cur, levels), w, h, pts, init, ttype, mv, levels=levels, win=win)
        r_xy, r_st = ref.lk_track(ref.pyr_build(prev, levels), ref.pyr_build(cur, levels), pts, init, ttype, mv, win=win)
        for i in np.nonzero(o_st != r_st)[0]:
            print("status differs: set %d point %d prev %s init %s oracle %d %s fp64 %d %s" % (k, i, pts[i], init[i], o_st[i], o_xy[i], r_st[i], r_xy[i]))
        both = (o_st & r_st) > 0
        d = float(np.abs(o_xy[both].astype(np.float64) - r_xy[both]).max()) if both.any() else 0.0
        ins = (pts[:, 0] >= 2) & (pts[:, 0] < w - 2) & (pts[:, 1] >= 2) & (pts[:, 1] < h - 2) & (init[:, 0] >= 2) & (init[:, 0] < w - 2)
        print("set %d %s: accepted by both %d / %d, in-image %d, status differs %d, worst |oracle - fp64| %.3g px" % (k, LK_SETS[k], both.sum(), len(pts), ins.sum(), (o_st != r_st).sum(), d))
        assert both.any()
        n += len(pts); bad += int((o_st != r_st).sum()); worst = max(worst, d)
        inside += int(ins.sum()); accepted += int((both & ins).sum())
    print("total: %d points, %d status disagreements, worst %.3g px (bound %.3g px), %d of %d in-image points accepted" % (n, bad, worst, ref.LK_TOL_PX, accepted, inside))
    assert n >= 300
    assert bad <= ref.LK_STATUS_CAP * n
    assert worst <= ref.LK_TOL_PX
    assert accepted >= 0.5 * inside


PYR_SHAPES = ((16, 16), (17, 16), (16, 17), (129, 127), (1, 1), (2, 3), (1, 5))


def _orc_pyr_down(orc, img):
    h, w = img.shape
    dst = np.zeros(((h + 1) // 2, (w + 1) // 2), np.uint8)
    src = np.ascontiguousarray(img)
    orc.lib().orc_pyr_down(src.ctypes.data_as(C.c_void_p), w, h, dst.ctypes.data_as(C.c_void_p))
    return dst


def test_pyr_down_oracle_vs_numpy_small(orc):
    rng = np.random.RandomState(3)
    for (h, w) in PYR_SHAPES:
        for img in (rng.randint(0, 256, (h, w)).astype(np.uint8), np.full((h, w), 255, np.uint8), _checker(h, w)):
            assert np.array_equal(_orc_pyr_down(orc, img), ref.pyr_down(img)), (h, w)
    for (h, w) in ((16, 16), (17, 31)):                           # down to 1x1 (16x16) and 1x1 after a 2x1 level (17x31), level by level
        img = rng.randint(0, 256, (h, w)).astype(np.uint8)
        total, off, ws, hs = orc.pyr_layout(w, h, 7)
        pyr = orc.pyr_build(img, 7)
        mine = ref.pyr_build(img, 7)
        assert (hs[-1], ws[-1]) == (1, 1)
        for l in range(8):
            assert mine[l].shape == (hs[l], ws[l])
            assert np.array_equal(pyr[off[l]:off[l] + ws[l] * hs[l]].reshape(hs[l], ws[l]), mine[l]), (h, w, l)


def _checker(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return (((yy + xx) & 1) * 255).astype(np.uint8)


def _halves_rows(h, w):
    """rows constant along y; x = 4 holds a + 4 among a = 10 (sum 256 * 11 + 128, odd quotient), x = 12 holds a + 4 among a = 11 (even quotient 12)"""
    row = np.where(np.arange(w) < 8, 10, 11).astype(np.uint8)
    row[4] = 14; row[12] = 15
    return np.repeat(row[None, :], h, 0)


def test_halfway_patterns_hit_both_parities():
    """the inputs of the round-half-to-even checks do contain exact halves, at an even and at an odd quotient"""
    q = {c[0] & 1 for c in ref.pyr_exact_halves(_halves_rows(16, 16))}
    assert q == {0, 1}
    out = ref.pyr_down(_halves_rows(16, 16))
    assert out[0, 2] == 12 and out[0, 6] == 12                     # 11.5 -> 12 and 12.5 -> 12
    ch = ref.pyr_exact_halves(_checker(16, 16))
    assert len(ch) == 64 and {c[0] for c in ch} == {127} and (ref.pyr_down(_checker(16, 16)) == 128).all()
    assert (ref.pyr_down(np.full((17, 31), 255, np.uint8)) == 255).all()


def test_fast_oracle_vs_numpy_edges(orc):
    n = nonempty = 0
    for img, feats, cols, rows, thr in list(_fast_single_cases()) + list(_fast_multi_cases()):
        xy, resp = orc.fast_by_region(img, feats, cols, rows, thr)
        rxy, rresp = _fast_by_region_np(img, feats, cols, rows, thr)
        assert np.array_equal(xy, rxy) and np.array_equal(resp, rresp), (img.shape, feats, cols, rows, thr)
        n += 1; nonempty += len(xy) > 0
    assert n >= 36 and nonempty > n // 2
    # equal responses come out in (region, raster) order: region index runs over columns first, then rows
    img = _dots(64, 64, 1, 200)
    xy, resp = orc.fast_by_region(img, 2000, 2, 2, 10)
    assert len(set(resp.tolist())) == 1 and len(xy) > 50
    key = [((int(x) // 32) * 2 + int(y) // 32, int(y) % 32, int(x) % 32) for x, y in xy]
    assert key == sorted(key)
    # a region of 6 px or less has no interior
    assert len(orc.fast_by_region(synth_image(16, 16, 1), 100, 3, 1, 10)[0]) == 0


@functools.lru_cache(maxsize=None)
def _gftt_ref(kind, h, w):
    """(image, fp64 eigenvalue map) -- computed once, shared, never modified"""
    img = _gftt_image(kind, h, w)
    img.setflags(write=False)
    return img, ref.min_eigen(img)


def test_good_features_oracle_vs_fp64_edges(orc):
    for (h, w) in GFTT_SIZES:
        for kind in GFTT_KINDS:
            img, e64 = _gftt_ref(kind, h, w)
            eig = orc.min_eigen(img)
            assert np.abs(eig - e64).max() < 1e-6 * max(e64.max(), 1e-3) + 1e-9
            cands = ref.corner_candidates(eig, 0.01)
            thr = np.float32(np.float64(eig.max()) * 0.01)
            rank = {(x, y): r for r, (_, y, x) in enumerate(cands)}
            if kind == "flat":
                assert not cands
            for md in GFTT_DISTS:
                for mc in GFTT_MAXC:
                    pts = orc.good_features(img, mc, 0.01, md)
                    want = ref.greedy_min_dist(cands, md, mc)
                    assert np.array_equal(pts, want), (kind, h, w, md, mc)
                    got = [(int(x), int(y)) for x, y in pts]
                    r = [rank[p] for p in got]                                   # every point is a candidate: a 3x3 maximum above quality * max
                    assert r == sorted(r)                                        # descending value, raster index breaks ties
                    assert all(eig[y, x] > thr and eig[y, x] == eig[y - 1:y + 2, x - 1:x + 2].max() for x, y in got)
                    if md >= 1 and len(got) > 1:
                        p = np.array(got, np.float64)
                        d = np.linalg.norm(p[:, None] - p[None], axis=-1) + np.eye(len(p)) * 1e9
                        assert d.min() >= md
                    # completeness: a candidate left out (before the list was full) lies closer than min_dist to an accepted one that ranks above it
                    full = mc > 0 and len(got) == mc
                    last = r[-1] if full else len(cands)
                    for rr, (_, y, x) in enumerate(cands[:last]):
                        if (x, y) in rank and (x, y) not in got:
                            assert md >= 1 and any(rank[a] < rr and (a[0] - x) ** 2 + (a[1] - y) ** 2 < md * md for a in got), (kind, h, w, md, mc, x, y)
    # the bright square: four equal corners in raster order; the 3 x 4 dot grid: neighbours at exactly 5 px survive min_dist 5
    img, _ = _gftt_ref("square", 48, 48)
    eig = orc.min_eigen(img)
    assert orc.good_features(img, 0, 0.01, 0.0).tolist() == [[6, 5], [11, 5], [6, 10], [11, 10]] and len({eig[5, 6], eig[5, 11], eig[10, 6], eig[10, 11]}) == 1
    img, _ = _gftt_ref("dots", 48, 48)
    pts = orc.good_features(img, 0, 0.01, 5.0)
    d = np.linalg.norm(pts[:, None] - pts[None], axis=-1) + np.eye(len(pts)) * 1e9
    assert (d == 5.0).any() and d.min() == 5.0


# ---------------------------------------------------------------------------------------------------------------- LK point lists (CPU-built, GPU-run)
def _edge_points(h, w, win, seed, n_interior=12):
    """the list every GPU LK case tracks: corners, half-pixel and whole-pixel overshoots, -0.0, a far point, points whose window is clipped at every
    border, interior points; cur_init jitters by up to 3 px, and two points are pushed across the left / top border so the iteration leaves the image"""
    rng = np.random.RandomState(seed)
    q = max(win // 4, 1)
    ym, xm = h * 0.5 + 0.25, w * 0.5 - 0.25
    pts = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w - 0.5, h - 0.5), (w, ym), (xm, h), (-0.0, ym), (1e9, 1e9),
           (q, ym), (w - 1 - q, ym), (xm, q), (xm, h - 1 - q), (1.5, ym), (xm, 1.25)]
    pts += list(zip(rng.uniform(2, w - 2, n_interior), rng.uniform(2, h - 2, n_interior)))
    pts = np.array(pts, np.float32)
    init = pts + rng.uniform(-3, 3, pts.shape).astype(np.float32)
    init[13] = pts[13] + np.float32([-3.0, 0.5])                 # guess left of the image: leaves during iteration at every level
    init[14] = pts[14] + np.float32([0.5, -3.0])                 # guess above the image
    init[15] = pts[15]                                           # one interior point starts from itself
    return pts, init


LK_WINS = (3, 5, 7, 9, 15, 17, 21, 23)
LK_SIZES = ((16, 16), (17, 31), (33, 16), (48, 64))
LK_LEVELS = (0, 2, 3, 7)


def _orc_pyrs(orc, prev, cur, levels):
    return orc.pyr_build(prev, levels), orc.pyr_build(cur, levels)


def test_edge_point_lists_reach_both_exits(orc):
    """from the per-level trace of the fp64 restatement (whose status equals the oracle's on these lists): tracks that leave the image during iteration
    above level 0 (status kept) and at level 0 (status cleared) both occur, and accepted tracks exist that took an early exit above level 0"""
    left_above = left_zero = kept = 0
    for (h, w, levels, win) in ((48, 64, 2, 21), (48, 64, 3, 9), (16, 16, 7, 5), (17, 31, 3, 7), (48, 64, 0, 21)):
        prev, cur = _pair(h, w, 300 + h)
        pts, init = _edge_points(h, w, win, 1)
        tr = []
        r_xy, r_st = ref.lk_track(ref.pyr_build(prev, levels), ref.pyr_build(cur, levels), pts, init, win=win, traces=tr)
        o_xy, o_st = orc.lk_track(*_orc_pyrs(orc, prev, cur, levels), w, h, pts, init, levels=levels, win=win)
        assert np.array_equal(r_st, o_st), (h, w, levels, win)
        for (tf, trv), st in zip(tr, o_st):
            left_above += any(l > 0 and what == "left_image" for l, what in tf + trv)
            left_zero += any(l == 0 and what == "left_image" for l, what in tf + trv)
            kept += bool(st) and any(l > 0 and what != "done" for l, what in tf + trv)
    print("left the image above level 0: %d tracks, at level 0: %d, accepted after an early exit above level 0: %d" % (left_above, left_zero, kept))
    assert left_above > 0 and left_zero > 0 and kept > 0


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def gpu():
    from d2slam_amd import api
    fe = api.FrontEnd(api.SuperPointConfig(input_width=64, input_height=64, max_batch=1))
    yield api, fe
    fe.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("size", LK_SIZES)
def test_lk_track_gpu_windows_levels_sizes(orc, gpu, size):
    api, fe = gpu
    h, w = size
    prev, cur = _pair(h, w, 300 + h)
    accepted = 0
    for levels in LK_LEVELS:
        fp, fc = api.buildImagePyramid(fe, prev, levels), api.buildImagePyramid(fe, cur, levels)
        pp, pc = _orc_pyrs(orc, prev, cur, levels)
        for win in LK_WINS:
            pts, init = _edge_points(h, w, win, 1)
            for iters in (1, 30):
                got, st = api.lk_track(fe, fp, fc, pts, init, 0, 0.0, win, iters)
                want, wst = orc.lk_track(pp, pc, w, h, pts, init, 0, 0.0, levels, win, iters)
                assert np.array_equal(st, wst), (size, levels, win, iters, np.nonzero(st != wst)[0])
                assert np.array_equal(_bits(got), _bits(want)), (size, levels, win, iters)
                assert wst[8] == 0 and wst[5] == 0 and wst[6] == 0          # the far point and the points at x = w / y = h
                accepted += int(wst.sum())
        fp.close(); fc.close()
    assert accepted > 0


@pytest.mark.gpu
def test_lk_track_gpu_point_counts_and_types(orc, gpu):
    """n = 1, 3, 4, 5, 257: the last workgroup of 4 waves is full, partly filled, or alone; the half-image types on the same lists"""
    api, fe = gpu
    h, w = 48, 64
    prev, cur = _pair(h, w, 41)
    fp, fc = api.buildImagePyramid(fe, prev, 2), api.buildImagePyramid(fe, cur, 2)
    pp, pc = _orc_pyrs(orc, prev, cur, 2)
    pts, init = _edge_points(h, w, 21, 2, n_interior=257 - 15)
    assert len(pts) == 257
    order = np.r_[15:257, 0:15]                     # interior points first, so that the short lists are not all rejected
    for n in (1, 3, 4, 5, 257):
        p, c = pts[order][:n], init[order][:n]
        for ttype, mv in ((0, 0.0), (1, 2.5), (2, 2.5)):
            got, st = api.lk_track(fe, fp, fc, p, c, ttype, mv)
            want, wst = orc.lk_track(pp, pc, w, h, p, c, ttype, mv)
            assert got.shape == (n, 2) and np.array_equal(st, wst) and np.array_equal(_bits(got), _bits(want)), (n, ttype)
    assert orc.lk_track(pp, pc, w, h, pts[order][:1], init[order][:1])[1][0] == 1
    fp.close(); fc.close()


@pytest.mark.gpu
def test_lk_track_batch_gpu_unordered_ranges(orc, gpu):
    """five pairs of different geometry, window 9, whose point ranges tile [0, n) out of order; one pair is empty"""
    api, fe = gpu
    geo = ((16, 16, 2, 0, 0.0), (17, 31, 3, 0, 0.0), (33, 16, 0, 1, 1.5), (48, 64, 7, 2, 2.0), (40, 48, 2, 0, 0.0))
    counts = (5, 0, 9, 4, 7)
    firsts = (20, 9, 0, 16, 9)                      # ranges [20,25) [9,9) [0,9) [16,20) [9,16)
    n = sum(counts)
    allp = np.zeros((n, 2), np.float32); alli = np.zeros((n, 2), np.float32)
    want = np.zeros((n, 2), np.float32); wst = np.zeros(n, np.uint8)
    pairs = (api._LKPair * len(geo))()
    frames = []
    for k, (h, w, levels, ttype, mv) in enumerate(geo):
        prev, cur = _pair(h, w, 70 + k)
        pts, init = _edge_points(h, w, 9, 3 + k)
        sel = np.r_[15:15 + 4, 0:15][:counts[k]] if k != 2 else np.arange(counts[k])         # pair 2 takes the edge points themselves
        a = firsts[k]
        allp[a:a + counts[k]], alli[a:a + counts[k]] = pts[sel], init[sel]
        fp, fc = api.buildImagePyramid(fe, prev, levels), api.buildImagePyramid(fe, cur, levels)
        frames += [fp, fc]
        pairs[k] = api._LKPair(fp._f, fc._f, a, counts[k], ttype, mv)
        if counts[k]:
            want[a:a + counts[k]], wst[a:a + counts[k]] = orc.lk_track(*_orc_pyrs(orc, prev, cur, levels), w, h, pts[sel], init[sel], ttype, mv, levels, 9, 30)
    out = np.full((n, 2), -5.0, np.float32); st = np.full(n, 9, np.uint8)
    api._check(fe._lib.d2fe_lk_track_batch(fe.handle, pairs, len(geo), api._ptr(allp), api._ptr(alli), n, 9, 30, api._ptr(out), api._ptr(st)))
    assert np.array_equal(st, wst) and np.array_equal(_bits(out), _bits(want))
    assert wst.sum() > 0
    for f in frames:
        f.close()


@pytest.mark.gpu
def test_lk_in_border_rounds_half_to_even(orc, gpu):
    """identical frames: the forward track returns its input bit for bit, so the status is inBorder(round-half-to-even) alone: 46.5 -> 46 passes
    `< w - 1` for w = 48 (half-up would give 47 and fail), 0.5 -> 0 fails `1 <=`"""
    api, fe = gpu
    h, w = 40, 48
    img = synth_image(h, w, 17)
    f = api.buildImagePyramid(fe, img, 2)
    pyr = orc.pyr_build(img, 2)
    xs = np.float32([0.5, 1.5, 2.5, w - 2.5, w - 1.5, w - 1.75])
    ys = np.float32([0.5, 1.5, 2.5, h - 2.5, h - 1.5, h - 1.75])
    pts = np.concatenate([np.stack([xs, np.full(6, 20.0, np.float32)], 1), np.stack([np.full(6, 24.0, np.float32), ys], 1)])
    want, wst = orc.lk_track(pyr, pyr, w, h, pts, pts)
    assert np.array_equal(_bits(want), _bits(pts))
    assert wst.tolist() == [0, 1, 1, 1, 1, 1] * 2
    got, st = api.lk_track(fe, f, f, pts, pts)
    assert np.array_equal(_bits(got), _bits(pts)) and st.tolist() == [0, 1, 1, 1, 1, 1] * 2
    f.close()


@pytest.mark.gpu
def test_lk_flat_frames_gpu(orc, gpu):
    """flat frames: D < eps at every level.  Each such return leaves the status (until level 0 clears it) and the carried guess untouched, so the guess is
    never doubled on the way down: the output is cur_init * 2^-(levels + 1) exactly (what cv::cuda::SparsePyrLKOpticalFlow leaves in nextPts too)"""
    api, fe = gpu
    h, w = 33, 47
    flat = np.full((h, w), 128, np.uint8)
    for levels in (0, 2, 3):
        f = api.buildImagePyramid(fe, flat, levels)
        pyr = orc.pyr_build(flat, levels)
        pts, init = _edge_points(h, w, 21, 4)
        got, st = api.lk_track(fe, f, f, pts, init)
        want, wst = orc.lk_track(pyr, pyr, w, h, pts, init, levels=levels)
        assert not st.any() and not wst.any()
        assert np.array_equal(_bits(got), _bits(want))
        assert np.array_equal(_bits(got), _bits(init * np.float32(0.5 ** (levels + 1))))
        f.close()


@pytest.mark.gpu
def test_lk_nonfinite_points_gpu(orc, gpu):
    """NaN and +-inf coordinates, one point each, among ordinary points: status 0 on both sides, the same NaN rows, every other row bitwise equal.
    (tex clamps every index after the float -> int conversion and lk_level's range tests stop infinities before any read.)"""
    api, fe = gpu
    h, w = 48, 64
    prev, cur = _pair(h, w, 55)
    pts, init = _edge_points(h, w, 21, 5)
    n0 = len(pts)
    odd = np.float32([[np.nan, 20], [30, np.nan], [np.inf, 20], [30, -np.inf], [20, 20], [20, 20], [20, 20], [20, 20]])
    oddi = np.float32([[20, 20], [30, 20], [20, 20], [30, 20], [np.nan, 20], [20, np.inf], [-np.inf, 20], [np.nan, np.nan]])
    pts, init = np.concatenate([pts, odd]), np.concatenate([init, oddi])
    fp, fc = api.buildImagePyramid(fe, prev, 2), api.buildImagePyramid(fe, cur, 2)
    got, st = api.lk_track(fe, fp, fc, pts, init)
    want, wst = orc.lk_track(*_orc_pyrs(orc, prev, cur, 2), w, h, pts, init)
    assert np.array_equal(st, wst) and not st[n0:].any() and st[:n0].any()
    assert np.array_equal(np.isnan(got), np.isnan(want))
    fin = ~np.isnan(want).any(1)
    assert fin[:n0].all() and np.array_equal(_bits(got[fin]), _bits(want[fin]))
    fp.close(); fc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("levels", (0, 2))
def test_lk_track_stereo_device_edges(orc, gpu, levels):
    """3 frames of 33 x 47 (w x h) with padded rows and a gap between images, cap 7 (not a multiple of 4), n_kp = [0, 7, 3]: pyramids in the workspace,
    tracks, dead slots, and nothing written past n_frames * cap or past the workspace"""
    import torch
    api, fe = gpu
    dev = torch.device("cuda", 0)
    w, h, stride, nf, cap = 33, 47, 64, 3, 7
    istride = stride * h + 40
    n_kp = [0, 7, 3]
    host = np.full((2, nf * istride), 201, np.uint8)                                       # poisoned padding and gaps
    imgs = []
    for f in range(nf):
        l, r = _pair(h, w, 80 + f)
        imgs.append((l, r))
        for side, im in enumerate((l, r)):
            v = host[side, f * istride:f * istride + stride * h].reshape(h, stride)
            v[:, :w] = im
    kps = np.full((nf, cap, 2), -7.0, np.float32)
    for f in range(nf):
        p, _ = _edge_points(h, w, 21, 6 + f)
        kps[f, :n_kp[f]] = p[[0, 3, 4, 7, 9, 16, 17]][:n_kp[f]]
    d_img = torch.from_numpy(host).to(dev)
    d_kps = torch.from_numpy(kps).to(dev); d_n = torch.tensor(n_kp, dtype=torch.int32, device=dev)
    nbytes = api.lk_stereo_workspace_bytes(nf, w, h, levels)
    total = orc.pyr_layout(w, h, levels)[0]
    assert nbytes == 2 * nf * total
    d_ws = torch.full((nbytes + 64,), 0xAB, dtype=torch.uint8, device=dev)
    d_pts = torch.full((nf * cap + 1, 2), 123.0, device=dev); d_st = torch.full((nf * cap + 1,), 9, dtype=torch.uint8, device=dev)      # one guard row
    torch.cuda.synchronize()
    api.lk_track_stereo_device(fe, d_img[0].data_ptr(), d_img[1].data_ptr(), nf, w, h, d_kps.data_ptr(), d_n.data_ptr(), cap, d_ws.data_ptr(),
                               d_pts.data_ptr(), d_st.data_ptr(), stride=stride, image_stride=istride, levels=levels)
    torch.cuda.synchronize()
    ws, pts, st = d_ws.cpu().numpy(), d_pts.cpu().numpy(), d_st.cpu().numpy()
    assert (ws[nbytes:] == 0xAB).all()
    assert np.array_equal(_bits(pts[nf * cap:]), _bits(np.float32([[123.0, 123.0]]))) and st[nf * cap] == 9
    for f in range(nf):
        pl, pr = orc.pyr_build(imgs[f][0], levels), orc.pyr_build(imgs[f][1], levels)
        assert np.array_equal(ws[f * total:(f + 1) * total], pl) and np.array_equal(ws[(nf + f) * total:(nf + f + 1) * total], pr), f
        k = n_kp[f]
        got, gst = pts[f * cap:(f + 1) * cap], st[f * cap:(f + 1) * cap]
        if k:
            want, wst = orc.lk_track(pl, pr, w, h, kps[f, :k], kps[f, :k], levels=levels)
            assert np.array_equal(gst[:k], wst) and np.array_equal(_bits(got[:k]), _bits(want)), f
        assert not gst[k:].any() and np.array_equal(_bits(got[k:]), np.zeros((cap - k, 2), np.uint32))       # dead slots: (+0, +0), status 0


def _frame_create(api, fe, img, stride, levels):
    """d2fe_lk_frame_create with an explicit row stride (api.LKFrame passes stride = width); returns an api.LKFrame that owns the handle"""
    host = np.full((img.shape[0], stride), 201, np.uint8)
    host[:, :img.shape[1]] = img
    f = api.LKFrame.__new__(api.LKFrame)
    f._lib, f._fe, f._f, f.levels = fe._lib, fe, C.c_void_p(), levels
    f.height, f.width = img.shape
    api._check(fe._lib.d2fe_lk_frame_create(fe.handle, api._ptr(host), f.width, f.height, stride, levels, C.byref(f._f)))
    return f


PYR_GPU = ((16, 16, 7), (17, 31, 4), (16, 128, 2), (128, 16, 2), (16, 129, 2), (129, 16, 2), (20, 130, 2), (130, 20, 2))     # (h, w, levels)


@pytest.mark.gpu
def test_pyramid_gpu_edges(orc, gpu):
    """levels down to 2x2 and 1x1, level widths 64 and 65 around the 64-lane row block, a host stride above the width; random, saturated, and two
    patterns whose sums are exact halves (checker: 127.5 everywhere; rows pattern: 11.5 and 12.5) against the oracle and the numpy restatement"""
    api, fe = gpu
    rng = np.random.RandomState(8)
    for (h, w, levels) in PYR_GPU:
        for kind, img in (("random", rng.randint(0, 256, (h, w)).astype(np.uint8)), ("white", np.full((h, w), 255, np.uint8)), ("checker", _checker(h, w)),
                          ("halves", _halves_rows(h, w))):
            total, off, ws, hs = orc.pyr_layout(w, h, levels)
            want = orc.pyr_build(img, levels)
            mine = ref.pyr_build(img, levels)
            for f in (api.buildImagePyramid(fe, img, levels), _frame_create(api, fe, img, w + 13, levels)):
                for l in range(levels + 1):
                    lv = f.level(l)
                    assert np.array_equal(lv, want[off[l]:off[l] + ws[l] * hs[l]].reshape(hs[l], ws[l])), (h, w, kind, l)
                    assert np.array_equal(lv, mine[l]), (h, w, kind, l)
                f.close()
            if kind == "white":
                assert all((m == 255).all() for m in mine)
            if kind == "checker":
                assert (mine[1] == 128).all()


def _c_fast(api, fe, f, feats, cols, rows, thr, cap):
    xy = np.full((cap + 1, 2), -3.0, np.float32); resp = np.full(cap + 1, -3, np.int32); n = C.c_int(-1)
    rc = fe._lib.d2fe_detect_fast_by_region(fe.handle, f._f, feats, cols, rows, thr, api._ptr(xy), api._ptr(resp), cap, C.byref(n))
    assert (xy[cap] == -3.0).all() and resp[cap] == -3
    return rc, n.value, xy[:max(n.value, 0)], resp[:max(n.value, 0)]


@pytest.mark.gpu
def test_fast_gpu_chunks_and_caps(orc, gpu):
    """single regions whose interior is 1024 px, 1024 + a partial chunk, 992 px, and several chunks; `features` at, one below and one above the number of
    corners in the first chunk, 1 and 2000; thresholds 0, 10, 254"""
    api, fe = gpu
    frames = {}
    n = hit = 0
    for img, feats, cols, rows, thr in _fast_single_cases():
        key = img.tobytes()
        if key not in frames:
            frames[key] = api.buildImagePyramid(fe, img, 0)
        xy, resp = api.detectFastByRegion(fe, frames[key], feats, cols, rows, thr, with_response=True)
        rxy, rresp = orc.fast_by_region(img, feats, cols, rows, thr)
        assert np.array_equal(xy, rxy) and np.array_equal(resp, rresp), (img.shape, feats, thr)
        n += 1; hit += len(rxy) > 0
    assert hit > n // 2
    # capacity below the result: D2FE_ERR_TRUNCATED with n_out == cap and the first cap points
    img = _fast_image("noise", 38, 39)
    rxy, rresp = orc.fast_by_region(img, 2000, 1, 1, 10)
    assert len(rxy) > 8
    rc, k, xy, resp = _c_fast(api, fe, frames[img.tobytes()], 2000, 1, 1, 10, 5)
    assert rc == api.ERR_TRUNCATED and k == 5 and np.array_equal(xy, rxy[:5]) and np.array_equal(resp, rresp[:5])
    rc, k, xy, resp = _c_fast(api, fe, frames[img.tobytes()], 2000, 1, 1, 10, len(rxy))
    assert rc == 0 and k == len(rxy) and np.array_equal(xy, rxy)
    for f in frames.values():
        f.close()


@pytest.mark.gpu
def test_fast_gpu_regions(orc, gpu):
    """7 px regions (one interior pixel) with a trailing strip, widths not divisible by cols, regions without interior, equal responses across regions"""
    api, fe = gpu
    for img, feats, cols, rows, thr in _fast_multi_cases():
        h, w = img.shape
        if h < 16 or w < 16:                                    # below the smallest frame the library builds: refused, not tracked
            with pytest.raises(api.D2FEError) as e:
                api.buildImagePyramid(fe, img, 0)
            assert e.value.code == -1
            continue
        f = api.buildImagePyramid(fe, img, 0)
        xy, resp = api.detectFastByRegion(fe, f, feats, cols, rows, thr, with_response=True)
        rxy, rresp = orc.fast_by_region(img, feats, cols, rows, thr)
        assert np.array_equal(xy, rxy) and np.array_equal(resp, rresp), (img.shape, feats, cols, rows, thr)
        if w // cols <= 6 or h // rows <= 6:
            assert len(xy) == 0                                 # and the call returned D2FE_OK (no exception)
        f.close()
    img = _dots(64, 64, 1, 200)                                 # equal responses: (region, raster) order, pinned on the CPU side above
    f = api.buildImagePyramid(fe, img, 0)
    for cols, rows in ((2, 2), (9, 9), (3, 5)):
        xy, resp = api.detectFastByRegion(fe, f, 2000, cols, rows, 10, with_response=True)
        rxy, rresp = orc.fast_by_region(img, 2000, cols, rows, 10)
        assert len(rxy) >= (4 if cols == 9 else 60) and len(set(rresp.tolist())) == 1 and np.array_equal(xy, rxy) and np.array_equal(resp, rresp)
    f.close()


@pytest.mark.gpu
def test_good_features_gpu_edges(orc, gpu):
    """flat image, equal corners of a square, a dot grid full of ties, a synthetic scene; min_dist below 1, at lrint half-way values and equal to the
    3-4-5 spacing of the dot grid; max_corners 0 / 1 / 7; a capacity below the result"""
    api, fe = gpu
    seen_trunc = 0
    for (h, w) in GFTT_SIZES:
        for kind in GFTT_KINDS:
            img, _ = _gftt_ref(kind, h, w)
            f = api.buildImagePyramid(fe, img, 0)
            for md in GFTT_DISTS:
                for mc in GFTT_MAXC:
                    want = orc.good_features(img, mc, 0.01, md)
                    if mc == 0 and len(want) > w * h // 4:       # api.goodFeaturesToTrack's own capacity: the call must fail, never return a short list
                        with pytest.raises(api.D2FEError) as e:
                            api.goodFeaturesToTrack(fe, f, mc, 0.01, md)
                        assert e.value.code == api.ERR_TRUNCATED
                        seen_trunc += 1
                        continue
                    got = api.goodFeaturesToTrack(fe, f, mc, 0.01, md)
                    assert np.array_equal(got, want), (kind, h, w, md, mc)
                    if kind == "flat":
                        assert len(got) == 0
            f.close()
    print("good features: %d calls exceeded the wrapper's w*h//4 capacity" % seen_trunc)
    assert seen_trunc == 0                                       # none of these images yields more than w*h/4 corners: every call returned the full list
    # a capacity below the result, through the C call
    img, _ = _gftt_ref("dots", 48, 48)
    f = api.buildImagePyramid(fe, img, 0)
    want = orc.good_features(img, 0, 0.01, 5.0)
    assert len(want) > 6
    xy = np.full((7, 2), -3.0, np.float32); n = C.c_int(-1)
    rc = fe._lib.d2fe_good_features_to_track(fe.handle, f._f, 0, C.c_double(0.01), C.c_double(5.0), api._ptr(xy), 6, C.byref(n))
    assert rc == api.ERR_TRUNCATED and n.value == 6 and np.array_equal(xy[:6], want[:6]) and (xy[6] == -3.0).all()
    f.close()
