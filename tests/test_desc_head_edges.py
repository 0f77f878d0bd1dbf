"""The sparse descriptor head of csrc/postproc.hip -- desc_mark_compact_kernel, its two-launch form desc_mark_kernel + desc_compact_kernel, the three compiled
forms of desc_head_sparse_kernel -- and variant A's descriptor tail (sample_a_kernel, chan_norm_a_kernel, finish_a_kernel) on injected tensors at their edges,
through d2fe_debug_desc_head_sparse and d2fe_debug_sample_a of the development library (include/d2fe_debug.h).  The extractor reaches these kernels with 0 or
about 300 keypoints per image kept off the border on maps of 15x20 or 30x40 cells; the lists below put 0, 1, 31 .. 65 cells on maps of 2x2, 3x5 and 13x11
cells, keypoints into the map's corners and onto its edges, and a map of 241x255 cells behind the launcher's switch to the two-launch form.
CPU part (no marker): on the very inputs the GPU tests use, the regime each case names is computed on the host from the corner rules the kernels cite
(tests/helpers/desc_head_ref.py) and asserted; the oracle's conv chain is held to a float64 evaluation at a derived fp32 bound that four mutants miss; and
oracle.sample_a is held to a float64 statement of computeDescriptors.
GPU part (-m gpu): the head equals the oracle bit for bit (the sign of a zero apart: the oracle skips an out-of-image tap, the kernel adds 0 * w), through every
form of the launcher; the samplers read nothing the head did not compute; variant A's tail equals the oracle at the project's 1e-6 bar,
1e-5 behind the PCA (the bar of test_variant_a_batch_and_pca).

The kernel form is the launcher's choice from (n, with_mid) -- _form() restates the rule of launch_desc_head_sparse, HEAD_FORMS lists the calls and the form
each is there to reach, and the CPU part asserts that they agree."""
import functools

import numpy as np
import pytest

from tests.helpers import desc_head_ref as R

ONES = 0xFFFFFFFF                         # what the hooks' outputs hold where no kernel wrote
GRIDS = ((2, 2), (3, 5), (13, 11))        # (Hc, Wc): every tap pattern partial; 15 cells; 143 cells = two 64-cell tiles and a partial one
RULES = ("B", "A8", "Aodd")               # variant B's clipped corners; variant A's for an image of 8 Wc x 8 Hc pixels; for one that is no multiple of 8
COUNTS = (65, 0, 64, 1, 31, 32, 33, 63)   # marked cells per image of the batch of 8 (capped at the map's cells); the empty image sits between full ones
CAP = 40
MAX_SLOTS = 4 * CAP
FULL_IMAGE = 0                            # the image whose list is full and whose n_kp exceeds cap
MID_THRESHOLD = 60 * 1024                 # cells: launch_desc_head_sparse takes the two-launch mark / compact above it


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def _orc():
    from oracle import oracle
    oracle.build()
    return oracle


@pytest.fixture(scope="module")
def fe():
    from d2slam_amd import api
    f = api.DevFrontEnd(api.SuperPointConfig(input_width=64, input_height=64, max_batch=1))
    yield f
    f.close()


def _form(n, with_mid):
    """launch_desc_head_sparse's rule with mid_imgs = min(n, 4) when there is a mid, as d2fe_debug_desc_head_sparse hands it over"""
    mid_imgs = min(n, 4) if with_mid else 0
    if n >= 8:
        return "<2,8,0>"
    if with_mid and n <= mid_imgs and n <= 4:
        return "<1,4,1>+<1,4,2>"
    return "<1,8,0>"


# (images of the batch of 8, with_mid, the form the call is there to reach)
HEAD_FORMS = [(tuple(range(8)), 0, "<2,8,0>"), ((0, 1, 2, 3), 1, "<1,4,1>+<1,4,2>"), ((4, 5, 6, 7), 1, "<1,4,1>+<1,4,2>"), ((0, 1, 2, 3), 0, "<1,8,0>"),
              ((4, 5, 6, 7), 0, "<1,8,0>"), ((0, 1, 2, 3, 4), 0, "<1,8,0>"), ((3, 4, 5, 6, 7), 1, "<1,8,0>")] + [((i,), 1, "<1,4,1>+<1,4,2>") for i in range(8)]


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------------------------
def _extent(rule, Hc, Wc):
    """(img_w, img_h handed to the hook, pixel extent W, H the keypoints live in)"""
    if rule == "B":
        return 0, 0, Wc * 8, Hc * 8
    W, H = (Wc * 8, Hc * 8) if rule == "A8" else (Wc * 8 + 5, Hc * 8 + 3)
    return W, H, W, H


@functools.lru_cache(maxsize=None)
def _weights():
    """N(0, 1 / sqrt(fan_in)) weights, so that the head's values stay of order 1 whatever the depth, and biases of order 0.1"""
    rng = np.random.RandomState(4100)
    w_da = (rng.randn(256, 128, 3, 3) / np.sqrt(9 * 128)).astype(np.float32)
    w_db = (rng.randn(256, 256, 1, 1) / np.sqrt(256)).astype(np.float32)
    return _ro(w_da, (0.1 * rng.randn(256)).astype(np.float32), w_db, (0.1 * rng.randn(256)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _x(Hc, Wc):
    """[8][Hc][Wc][128], N(0, 1): both signs reach the ReLU"""
    return _ro(np.random.RandomState(97 * Hc + Wc).randn(8, Hc, Wc, 128).astype(np.float32))


def _strided(x, xs):
    """[..., 128] -> [..., xs] with NaN in the padding channels, which are never to be read"""
    out = np.full(x.shape[:-1] + (xs,), np.nan, np.float32)
    out[..., :128] = x
    return out


@functools.lru_cache(maxsize=None)
def _dense_ref(Hc, Wc, i):
    """the oracle's descriptor head over the whole map of image i: [Hc][Wc][256]"""
    orc = _orc()
    w_da, b_da, w_db, b_db = _weights()
    return _ro(orc.conv(orc.conv(_x(Hc, Wc)[i], w_da, b_da, True), w_db, b_db, False))


def _mandatory(W, H):
    """the four corners of the image and a keypoint on each edge"""
    return [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, 0), (W // 2, H - 1), (0, H // 2), (W - 1, H // 2)]


def _list_for(rule, Hc, Wc, target, seed):
    """A keypoint list (at most CAP - 3 distinct integer pixels) that reads exactly `target` cells: the image's corners and edge midpoints first, then a seeded
    shuffle of all pixels, each taken when it adds a cell and the count stays within the target.  Then three repeats of keypoints of the list."""
    img_w, img_h, W, H = _extent(rule, Hc, Wc)
    if target == 0:
        return np.zeros((0, 2), np.float32)
    rng = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:H, 0:W]
    allpx = np.stack([xs.reshape(-1), ys.reshape(-1)], 1)
    pool = np.concatenate([np.array(_mandatory(W, H)), allpx[rng.permutation(len(allpx))]]).astype(np.float32)
    cells = R.read_cells(pool, Hc, Wc, img_w, img_h)
    have, chosen = set(), []
    for i in range(len(pool)):
        new = set(int(c) for c in cells[i] if c >= 0) - have
        if (new or i < 8) and len(have) + len(new) <= target and len(chosen) < CAP - 3:
            have |= new
            chosen.append(i)
        if len(have) == target and i >= 8:
            break
    assert len(have) == target, (rule, Hc, Wc, target, len(have))
    k = pool[chosen]
    return np.concatenate([k, k[[0, len(k) - 1, 0]]])


@functools.lru_cache(maxsize=None)
def _batch(rule, Hc, Wc):
    """The batch of 8 lists: kps [8][CAP][2] (unused entries NaN: never to be read), n_kp [8] and the cells each image is to mark.  FULL_IMAGE's list is padded
    with repeats to CAP entries and its n_kp is CAP + 7: the kernels clamp it."""
    img_w, img_h, W, H = _extent(rule, Hc, Wc)
    kps = np.full((8, CAP, 2), np.nan, np.float32)
    n_kp = np.zeros(8, np.int32)
    for i, c in enumerate(COUNTS):
        k = _list_for(rule, Hc, Wc, min(c, Hc * Wc), 1000 * i + 10 * Hc + Wc + len(rule))
        if i == FULL_IMAGE:
            k = np.concatenate([k, k[np.arange(CAP - len(k)) % len(k)]])
        kps[i, :len(k)] = k
        n_kp[i] = len(k) + (7 if i == FULL_IMAGE else 0)
    cells = [R.marked_cells(kps[i, :min(int(n_kp[i]), CAP)], Hc, Wc, img_w, img_h) for i in range(8)]
    return dict(kps=_ro(kps), n_kp=_ro(n_kp), cells=cells, img_w=img_w, img_h=img_h, W=W, H=H)


def _cases():
    return [(r, g) for g in GRIDS for r in RULES]


# the map behind the threshold: 241 x 255 = 61 455 cells; raster index 61 440 is cell (240, 240)
BIG = (241, 255)
SMALL = (240, 255)                        # 61 200 cells: the one-launch form, on the first 240 rows of the same x
BIG_BOXES = ((0, 0, 3, 4), (0, 251, 3, 4), (237, 0, 4, 4), (237, 251, 4, 4),      # (first cell row, first cell column, rows, columns): the four corners,
             (3, 0, 3, 12), (239, 234, 2, 14), (120, 100, 4, 6))                 # across raster 1024 = (4, 4), across raster 61 440 = (240, 240), mid-map
BIG_PER_BOX = 45


@functools.lru_cache(maxsize=None)
def _big_kps():
    """315 integer keypoints (variant B pixel coordinates of the 241-row map) drawn inside BIG_BOXES, the corner pixels of the image among them; with their box"""
    rng = np.random.RandomState(61440)
    Hc, Wc = BIG
    out, box = [], []
    for b, (cy, cx, nr, nc) in enumerate(BIG_BOXES):
        x = rng.randint(cx * 8, min((cx + nc) * 8, Wc * 8), BIG_PER_BOX); y = rng.randint(cy * 8, min((cy + nr) * 8, Hc * 8), BIG_PER_BOX)
        if b < 4:
            x[0] = 0 if cx == 0 else Wc * 8 - 1; y[0] = 0 if cy == 0 else Hc * 8 - 1
        out.append(np.stack([x, y], 1)); box += [b] * BIG_PER_BOX
    order = rng.permutation(len(box))      # the list order is free: mix the clusters
    return _ro(np.concatenate(out).astype(np.float32)[order], np.array(box)[order])


@functools.lru_cache(maxsize=None)
def _big_x():
    """[241][255][128] N(0, 1): 31 MB"""
    return _ro(np.random.RandomState(255).randn(BIG[0], BIG[1], 128).astype(np.float32))


# variant A's tail on dense maps
TAIL_GRIDS = ((2, 2), (12, 17))
TAIL_SIZES = ("8", "odd")
TAIL_CAP = 24
TAIL_COUNTS = (TAIL_CAP + 5, 1, 0, 7, 1, 2)      # image 0: clamped to cap; 1: one keypoint; 2: none, between lists; 4: one keypoint on a cell with a zero channel
ZERO_CHANNEL = 7


@functools.lru_cache(maxsize=None)
def _tail_case(Hc, Wc, size):
    """raw [6][Hc][Wc][256] (per-cell magnitude 10^u, u in [-3, 3]; image 4 has channel ZERO_CHANNEL at exactly 0), kps [6][TAIL_CAP][2], n_kp, img_w, img_h.
    Every list begins with keypoints at x = 0, y = 0, x = W - 1, y = H - 1 (the four image corners and edge midpoints) and exact cell centres."""
    rng = np.random.RandomState(11 * Hc + Wc + len(size))
    W, H = (Wc * 8, Hc * 8) if size == "8" else (Wc * 8 + 5, Hc * 8 + 3)
    raw = (rng.randn(6, Hc, Wc, 256) * 10.0 ** rng.uniform(-3, 3, size=(6, Hc, Wc, 1))).astype(np.float32)
    raw[4, :, :, ZERO_CHANNEL] = 0.0
    kps = np.full((6, TAIL_CAP, 2), np.nan, np.float32)
    centres = [(W * (2 * cx + 1) / (2.0 * Wc), H * (2 * cy + 1) / (2.0 * Hc)) for cy, cx in ((0, 0), (Hc - 1, Wc - 1), (Hc // 2, Wc // 2))]
    for i in range(6):
        fixed = np.array(_mandatory(W, H) + centres, np.float32)
        rnd = np.stack([rng.randint(0, W, TAIL_CAP), rng.randint(0, H, TAIL_CAP)], 1).astype(np.float32)
        kps[i] = np.concatenate([fixed, rnd])[:TAIL_CAP] if i != 1 else np.roll(np.concatenate([fixed, rnd])[:TAIL_CAP], -8, axis=0)      # image 1 begins with a cell centre
    return _ro(raw, kps, np.array(TAIL_COUNTS, np.int32)) + (W, H)


@functools.lru_cache(maxsize=None)
def _pca(dims):
    rng = np.random.RandomState(dims)
    return _ro(np.linalg.qr(rng.randn(256, dims))[0].T.astype(np.float32), (rng.randn(256) * 0.01).astype(np.float32))


def _tail_oracle(raw_i, kps_i, n, W, H, pca=None):
    orc = _orc()
    if n == 0:
        return np.zeros((0, pca[0].shape[0] if pca else 256), np.float32)
    with np.errstate(all="ignore"):
        return orc.sample_a(orc.l2norm_rows(raw_i), kps_i[:n], W, H, *(pca or ()))


# ---- CPU part ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_head_forms_are_the_launchers_rule():
    for imgs, with_mid, form in HEAD_FORMS:
        assert _form(len(imgs), with_mid) == form, (imgs, with_mid)
    assert {f for _, _, f in HEAD_FORMS} == {"<2,8,0>", "<1,4,1>+<1,4,2>", "<1,8,0>"}
    n_mid = {(len(i), m) for i, m, _ in HEAD_FORMS}
    assert {(1, 1), (4, 1), (4, 0), (5, 0), (5, 1), (8, 0)} <= n_mid      # <1,8,0> with and without a mid, with 4 and with 5 images


@pytest.mark.parametrize("rule,grid", _cases())
def test_lists_reach_their_cell_counts_and_the_border(rule, grid):
    Hc, Wc = grid
    b = _batch(rule, Hc, Wc)
    ncell = Hc * Wc
    counts = [len(c) for c in b["cells"]]
    assert counts == [min(c, ncell) for c in COUNTS], counts
    assert counts[1] == 0 and counts[0] > 0 and counts[2] > 0 and int(b["n_kp"][1]) == 0      # an empty image between full ones
    assert int(b["n_kp"][FULL_IMAGE]) > CAP and np.all(np.isfinite(b["kps"][FULL_IMAGE]))      # n_kp above cap, the list full
    if ncell >= 65:      # the tile edges of 32 and 64: an empty second row tile (<= 32 of 64), a partial one (33, 63), a full one, a second workgroup (65)
        assert counts == list(COUNTS)
    for i in range(8):
        k = b["kps"][i, :min(int(b["n_kp"][i]), CAP)]
        assert counts[i] == 0 or len(np.unique(k, axis=0)) < len(k), "repeated keypoints"
        assert np.all((k[:, 0] >= 0) & (k[:, 0] <= b["W"] - 1) & (k[:, 1] >= 0) & (k[:, 1] <= b["H"] - 1))
    # the border: cells with 4 of 9 taps inside (a corner of the map: 5 outside) and with 6 (an edge: 3 outside); in a 2 x 2 map every pattern is partial
    taps = np.concatenate([R.taps_inside(c, Hc, Wc) for c in b["cells"]])
    assert set(taps) == ({4} if grid == (2, 2) else {4, 6, 9}), set(taps)
    corners = {0, Wc - 1, (Hc - 1) * Wc, ncell - 1}
    assert corners <= set(b["cells"][0]) | set(b["cells"][2]), "the four corner cells of the map are marked"
    full = b["kps"][0, :CAP]
    have = {tuple(p) for p in full}
    assert {(0.0, 0.0), (b["W"] - 1.0, b["H"] - 1.0)} <= have and any(p[1] == 0 and 0 < p[0] < b["W"] - 1 for p in have)
    if rule == "B":      # clipped corners coincide in the last row and column: such a keypoint reads 1 or 2 cells
        cx, cy, _ = R.corners_b(full, Hc, Wc)
        assert ((cx[:, 0] == cx[:, 1]) & (cy[:, 0] == cy[:, 2])).any()
    else:                # padded corners: x0 = -1 at x = 0, x1 = Wc at the right edge, and the same in y
        cx, cy, _, inside = R.corners_a(full, Hc, Wc, b["img_w"], b["img_h"])
        assert (cx[:, 0] == -1).any() and (cx[:, 1] == Wc).any() and (cy[:, 0] == -1).any() and (cy[:, 2] == Hc).any()
        assert (inside.sum(1) == 1).any() and (inside.sum(1) == 2).any()
        assert (rule == "A8") == (b["img_w"] % 8 == 0 and b["img_h"] % 8 == 0)


def _big_expect(grid, rule):
    Hc, Wc = grid
    kps, _ = _big_kps()
    img_w, img_h = (0, 0) if rule == "B" else (Wc * 8 + 5, Hc * 8 + 3)
    return R.marked_cells(kps, Hc, Wc, img_w, img_h), img_w, img_h


def test_big_map_takes_the_two_launch_form_and_crosses_its_steps():
    assert BIG[0] * BIG[1] == 61455 > MID_THRESHOLD >= SMALL[0] * SMALL[1]
    kps, box = _big_kps()
    assert len(kps) == 315 > 256      # desc_mark_kernel: two workgroups per image
    for rule in ("B", "Aodd"):
        cells, _, _ = _big_expect(BIG, rule)
        assert 150 < len(cells) <= 4 * len(kps)
        assert {0, BIG[1] - 1, 240 * 255, 61454} <= set(cells), "the four corner cells"
        assert (cells < 61440).any() and (cells >= 61440).any() and ((cells >= 61430) & (cells < 61440)).any(), "across raster index 61 440"
        steps = np.unique(cells // 1024)
        assert len(steps) >= 5 and {0, 1, 59, 60} <= set(steps), steps      # compaction steps of 1024 cells: the running base is carried across several
        assert ((cells >= 1016) & (cells < 1024)).any() and ((cells >= 1024) & (cells < 1032)).any(), "across raster index 1024"


@pytest.mark.parametrize("grid", GRIDS)
def test_oracle_head_is_inside_the_fp32_bound_of_float64_and_mutants_are_not(grid):
    """The oracle's conv chain at the marked cells against head_f64 at its derived bound (tests/helpers/desc_head_ref.py: gamma_1153 (|b| + sum |x| |w|) for
    convDa, that carried through |W_db| plus gamma_257 (|b| + sum |mid| |w|) for convDb).  The bound says something: at most 0.01 max(1, max |y|), the condition
    LAYER_LIMIT states in test_netvlad_shapes.py.  And the comparison at that bound rejects a dropped tap, a dropped input channel, a missing ReLU, a missing bias."""
    from tests.helpers import nv_f64_ref as nv
    Hc, Wc = grid
    w = _weights()
    refs = [R.head_f64(_x(Hc, Wc)[i], *w) for i in range(8)]
    # over the tensor the launch computes, the batch of 8 maps.  (One 3 x 5 map alone holds 3840 values of standard deviation 0.7 and a largest one of 2.17,
    # its largest bound is 0.0218: 1.006 %.  The bound is 3 % of a standard deviation whatever the map; what varies is how far the largest of N values lies out.)
    b_max, y_max = max(float(r["bound"].max()) for r in refs), max(float(np.abs(r["y"]).max()) for r in refs)
    assert b_max <= 0.01 * max(1.0, y_max), (b_max, y_max)
    worst = 0.0
    for rule in RULES:
        b = _batch(rule, Hc, Wc)
        for i in range(8):
            cells = b["cells"][i]
            got = _dense_ref(Hc, Wc, i).reshape(-1, 256)[cells]
            y, bound = refs[i]["y"].reshape(-1, 256)[cells], refs[i]["bound"].reshape(-1, 256)[cells]
            r = nv.compare(got, y, bound)
            worst = max(worst, r)
            assert r <= 1.0, (rule, i, r)
            if rule == "B" and i == 0:
                for mutant in (("tap", 0), ("tap", 4), ("tap", 8), ("cin", 0), ("cin", 127), "relu", "bias_da", "bias_db"):
                    m = R.head_f64(_x(Hc, Wc)[i], *w, mutant=mutant)["y"].reshape(-1, 256)[cells]
                    rm = nv.compare(got, m, bound)
                    assert rm > 1.0, (mutant, rm)
    print("oracle head vs float64, %dx%d cells: largest error / bound %.3g; largest bound %.3g, largest |y| %.3g" % (Hc, Wc, worst, b_max, y_max))


@pytest.mark.parametrize("size", TAIL_SIZES)
@pytest.mark.parametrize("Hc,Wc", TAIL_GRIDS)
def test_oracle_sample_a_is_the_float64_computeDescriptors(Hc, Wc, size):
    """1e-6 is the project's descriptor bar, 1e-5 the one test_variant_a_batch_and_pca holds the PCA form to.  One keypoint: every channel is
    S / |S| = +-1 and the row +-1/16 exactly -- or NaN in the whole row once a sample is exactly 0 (0 / 0 enters the row norm)."""
    raw, kps, n_kp, W, H = _tail_case(Hc, Wc, size)
    for pca, bar in ((None, 1e-6), (_pca(64), 1e-5), (_pca(40), 1e-5), (_pca(100), 1e-5)):
        for i in range(6):
            n = min(int(n_kp[i]), TAIL_CAP)
            if n == 0:
                continue
            got = _tail_oracle(raw[i], kps[i], n, W, H, pca)
            ref = R.sample_a_f64(raw[i], kps[i, :n], W, H, *(pca or ()))
            assert np.array_equal(np.isnan(got), np.isnan(ref)), (i, pca is not None)
            ok = ~np.isnan(ref)
            assert (i == 4) == (not ok.any()), i      # the zero channel: NaN in every component of image 4, nowhere else
            if ok.any():
                assert float(np.abs(got[ok] - ref[ok]).max()) <= bar, (i, float(np.abs(got[ok] - ref[ok]).max()))
            if pca is None and i == 1:
                assert np.array_equal(np.abs(got), np.full((1, 256), 1.0 / 16, np.float32))
    # the regimes: padded corners on every side, a cell centre hit exactly (weights 1, 0, 0, 0)
    cx, cy, wgt, inside = R.corners_a(kps[0], Hc, Wc, W, H)
    assert (cx[:, 0] == -1).any() and (cx[:, 1] == Wc).any() and (cy[:, 0] == -1).any() and (cy[:, 2] == Hc).any()
    if size == "8":      # (where 2 x / W is no fp32 number the centre is missed by an ulp, and the weights are 1 - ulp and ulp: an edge case of its own)
        assert (wgt == np.float32([1, 0, 0, 0])).all(1).any()
    assert (size == "8") == (W % 8 == 0 and H % 8 == 0)


# ---- GPU part ---------------------------------------------------------------------------------------------------------------------------------------------------
def _run_head(fe, x, kps, n_kp, img_w, img_h, with_mid=0, max_slots=MAX_SLOTS):
    return fe.debug_desc_head_sparse(x, kps, n_kp, max_slots, *_weights(), with_mid=with_mid, img_w=img_w, img_h=img_h)


def _check_structure(out, expect_cells, Hc, Wc, max_slots, tag):
    """cells = the marked set in raster order (the first max_slots of it), slotmap its inverse and -1 elsewhere, count, and all-ones words behind the count"""
    store, slotmap, cells, count = out
    for i, want in enumerate(expect_cells):
        c = min(len(want), max_slots)
        assert int(count[i]) == c, (tag, i, int(count[i]), c)
        assert np.array_equal(cells[i, :c], want[:c]), (tag, i)
        assert np.all(cells[i, c:] == -1), (tag, i, "cells behind the count")
        inv = np.full(Hc * Wc, -1, np.int32)
        inv[want[:c]] = np.arange(c)
        assert np.array_equal(slotmap[i].reshape(-1), inv), (tag, i)
        assert np.all(_bits(store[i, c:]) == ONES), (tag, i, "store rows behind the count")
        assert not np.any(_bits(store[i, :c]) == ONES), (tag, i, "an unwritten word below the count")


def _assert_rows_equal_oracle(got, ref, tag):
    """bit for bit, the sign of a zero apart"""
    bad = _bits(got) != _bits(ref)
    assert not np.any(bad & ~((got == 0) & (ref == 0))), (tag, int(bad.sum()))
    return int(bad.sum())


@pytest.mark.gpu
@pytest.mark.parametrize("rule,grid", _cases())
def test_head_equals_the_oracle_in_every_form_gpu(fe, rule, grid):
    Hc, Wc = grid
    b = _batch(rule, Hc, Wc)
    zero_signs = 0
    for xs in (128, 136):
        x = _strided(_x(Hc, Wc), xs)
        base = None
        for imgs, with_mid, form in HEAD_FORMS:
            sel = list(imgs)
            out = _run_head(fe, x[sel], b["kps"][sel], b["n_kp"][sel], b["img_w"], b["img_h"], with_mid)
            tag = (rule, grid, xs, imgs, form)
            _check_structure(out, [b["cells"][i] for i in sel], Hc, Wc, MAX_SLOTS, tag)
            if base is None:      # the batch of 8 through <2,8,0>: against the oracle
                base = out
                for i in sel:
                    c = b["cells"][i]
                    zero_signs += _assert_rows_equal_oracle(out[0][i, :len(c)], _dense_ref(Hc, Wc, i).reshape(-1, 256)[c], tag + (i,))
            else:                 # every other form: the bits of the first
                for j, i in enumerate(sel):
                    assert np.array_equal(_bits(out[0][j]), _bits(base[0][i])), tag + (i,)
    print("head %s %dx%d: equal to the oracle in every form; %d zeros of the other sign" % (rule, Hc, Wc, zero_signs))


@pytest.mark.gpu
@pytest.mark.parametrize("rule", ("B", "Aodd"))
def test_two_launch_mark_compact_on_the_big_map_gpu(fe, rule):
    """241 x 255 cells take desc_mark_kernel + desc_compact_kernel; the first 240 rows of the same x as a map of their own take desc_mark_compact_kernel.  The
    reference is the oracle on crops around the clusters, cut with a one-cell halo clipped at the map's border, so that a crop's zero padding is the map's."""
    orc = _orc()
    w = _weights()
    kps, box = _big_kps()
    xb = _big_x()
    n_kp = np.array([len(kps)], np.int32)
    outs = {}
    for grid in (BIG, SMALL):
        Hc, Wc = grid
        want, img_w, img_h = _big_expect(grid, rule)
        out = _run_head(fe, xb[None, :Hc], kps[None], n_kp, img_w, img_h, with_mid=0, max_slots=4 * len(kps))
        _check_structure(out, [want], Hc, Wc, 4 * len(kps), (rule, grid))
        outs[grid] = (out[0][0], want)
        for bx in range(len(BIG_BOXES)):      # the oracle on this cluster's crop
            cells = R.marked_cells(kps[box == bx], Hc, Wc, img_w, img_h)
            cy, cx = cells // Wc, cells % Wc
            y0, y1, x0, x1 = max(cy.min() - 1, 0), min(cy.max() + 2, Hc), max(cx.min() - 1, 0), min(cx.max() + 2, Wc)
            ref = orc.conv(orc.conv(xb[y0:y1, x0:x1], w[0], w[1], True), w[2], w[3], False)
            _assert_rows_equal_oracle(out[0][0, np.searchsorted(want, cells)], ref[cy - y0, cx - x0], (rule, grid, bx))
    # both maps: a cell above row 239 has the same neighbourhood in both, and so the same row
    (sb, cb), (ss, cs) = outs[BIG], outs[SMALL]
    common = np.intersect1d(cb[cb // 255 < 239], cs)
    assert len(common) > 60
    assert np.array_equal(_bits(sb[np.searchsorted(cb, common)]), _bits(ss[np.searchsorted(cs, common)]))


@pytest.mark.gpu
@pytest.mark.parametrize("max_slots", (1, 32, 40))
def test_max_slots_clips_the_compaction_gpu(fe, max_slots):
    """A store smaller than the marked set: count = max_slots, the first max_slots marked cells in raster order, slotmap -1 for the rest, the kept rows those of
    the unclipped run, and nothing written behind them (the next image's rows, or the words behind an image's count).  No sampler runs on a clipped store, and
    none is run here: the extractor sizes the store to 4 cap slots (sp_slots), which a list of cap keypoints cannot exceed."""
    Hc, Wc = 13, 11
    for rule in ("B", "Aodd"):
        b = _batch(rule, Hc, Wc)
        x = _x(Hc, Wc)
        assert any(len(c) > max_slots for c in b["cells"]) and (max_slots == 1 or any(0 < len(c) < max_slots for c in b["cells"]))
        for imgs, with_mid, form in HEAD_FORMS[:7]:
            sel = list(imgs)
            full = _run_head(fe, x[sel], b["kps"][sel], b["n_kp"][sel], b["img_w"], b["img_h"], with_mid)
            clip = _run_head(fe, x[sel], b["kps"][sel], b["n_kp"][sel], b["img_w"], b["img_h"], with_mid, max_slots=max_slots)
            _check_structure(clip, [b["cells"][i] for i in sel], Hc, Wc, max_slots, (rule, max_slots, imgs, form))
            for j in range(len(sel)):
                c = int(clip[3][j])
                assert np.array_equal(_bits(clip[0][j, :c]), _bits(full[0][j, :c])), (rule, max_slots, imgs, j)


def _scatter_dense(store, slotmap):
    """[n][Hc][Wc][256]: the store's rows at their cells, zeros elsewhere"""
    n, Hc, Wc = slotmap.shape
    dense = np.zeros((n, Hc * Wc, 256), np.float32)
    for i in range(n):
        at = np.flatnonzero(slotmap[i].reshape(-1) >= 0)
        dense[i, at] = store[i, slotmap[i].reshape(-1)[at]]
    return dense.reshape(n, Hc, Wc, 256)


@pytest.mark.gpu
@pytest.mark.parametrize("rule,grid", _cases())
def test_mark_and_sampler_agree_gpu(fe, rule, grid):
    """The head's own store and slot map under the sampler of the same variant, against that sampler on the dense map scattered from the store (same bits) and
    against the oracle's descriptors of the oracle's dense map.  A cell that is read but not marked has slotmap = -1: asserted absent on the host first (the
    hook refuses such a call, from a host computation of its own, and keeps a row of NaN in front of the store)."""
    orc = _orc()
    Hc, Wc = grid
    b = _batch(rule, Hc, Wc)
    store, slotmap, cells, count = _run_head(fe, _x(Hc, Wc), b["kps"], b["n_kp"], b["img_w"], b["img_h"])
    nk = np.minimum(b["n_kp"], CAP)
    for i in range(8):
        rc = R.read_cells(b["kps"][i, :nk[i]], Hc, Wc, b["img_w"], b["img_h"]).reshape(-1)
        assert np.all(slotmap[i].reshape(-1)[rc[rc >= 0]] >= 0), (i, "a cell the sampler reads has no slot")
    assert grid != (13, 11) or (slotmap == -1).any()      # cells without a slot, which no keypoint reads: the sampler hooks accept them
    dense = _scatter_dense(store, slotmap)
    forms = [(None, 1e-6)] if rule == "B" else [(None, 1e-6), (_pca(64), 1e-5)]
    for pca, bar in forms:
        if rule == "B":
            sp, dn = fe.debug_sample_b(store, b["kps"], b["n_kp"], slotmap=slotmap), fe.debug_sample_b(dense, b["kps"], b["n_kp"])
        else:
            kw = dict(comp=pca[0], mean=pca[1]) if pca else {}
            sp = fe.debug_sample_a(store, b["kps"], b["n_kp"], b["img_w"], b["img_h"], slotmap=slotmap, **kw)
            dn = fe.debug_sample_a(dense, b["kps"], b["n_kp"], b["img_w"], b["img_h"], **kw)
        assert np.array_equal(_bits(sp), _bits(dn)), (rule, grid, pca is not None)
        worst = 0.0
        for i in range(8):
            k = b["kps"][i, :nk[i]]
            assert np.all(_bits(sp[i, nk[i]:]) == ONES), i
            if nk[i] == 0:
                continue
            dmap = orc.l2norm_rows(_dense_ref(Hc, Wc, i))
            with np.errstate(all="ignore"):
                ref = orc.sample_b(dmap, k) if rule == "B" else orc.sample_a(dmap, k, b["img_w"], b["img_h"], *(pca or ()))
            got = sp[i, :nk[i]]
            assert np.array_equal(np.isnan(got), np.isnan(ref)), (rule, grid, i)
            ok = ~np.isnan(ref)
            if ok.any():
                worst = max(worst, float(np.abs(got[ok] - ref[ok]).max()))
        print("sampler behind the head, %s %dx%d%s: worst %.3g" % (rule, Hc, Wc, " pca" if pca else "", worst))
        assert worst <= bar, worst


@pytest.mark.gpu
@pytest.mark.parametrize("size", TAIL_SIZES)
@pytest.mark.parametrize("Hc,Wc", TAIL_GRIDS)
def test_variant_a_tail_on_dense_maps_gpu(fe, Hc, Wc, size):
    """sample_a, chan_norm_a, finish_a on dense maps with dstride / dcoff 256 / 0 and 264 / 4 against the oracle: six lists of different lengths in one launch
    (the channel norm must not mix them) -- clamped to cap, one keypoint (+-1/16 exactly), none, one keypoint on a zero channel (NaN where the oracle has NaN) --
    without a PCA and with 64, 40 and 100 components (pca_tail's other path above 64), and with a sampling scratch smaller than the lists (scap < n_kp)."""
    raw, kps, n_kp, W, H = _tail_case(Hc, Wc, size)
    padded = np.full((6, Hc, Wc, 264), np.nan, np.float32)
    padded[..., 4:260] = raw
    for pca, bar in ((None, 1e-6), (_pca(64), 1e-5), (_pca(40), 1e-5), (_pca(100), 1e-5)):
        kw = dict(comp=pca[0], mean=pca[1]) if pca else {}
        for scap in (TAIL_CAP, 5):
            outs = [fe.debug_sample_a(raw, kps, n_kp, W, H, scap=scap, **kw), fe.debug_sample_a(padded, kps, n_kp, W, H, scap=scap, dcoff=4, **kw)]
            assert np.array_equal(_bits(outs[0]), _bits(outs[1])), "dstride 264 / dcoff 4 differs from 256 / 0"
            got = outs[0]
            worst = 0.0
            for i in range(6):
                n = min(int(n_kp[i]), TAIL_CAP, scap)
                assert np.all(_bits(got[i, n:]) == ONES), (i, "rows behind the list are untouched")
                if n == 0:
                    continue
                ref = _tail_oracle(raw[i], kps[i], n, W, H, pca)
                assert np.array_equal(np.isnan(got[i, :n]), np.isnan(ref)), (i, scap, pca is not None)
                ok = ~np.isnan(ref)
                assert (i == 4) == (not ok.any())
                if ok.any():
                    worst = max(worst, float(np.abs(got[i, :n][ok] - ref[ok]).max()))
                if pca is None and i == 1:
                    assert np.array_equal(np.abs(got[i, :1]), np.full((1, 256), 1.0 / 16, np.float32))
            print("variant A tail %dx%d %s, pca %s, scap %d: worst %.3g" % (Hc, Wc, size, pca[0].shape[0] if pca else None, scap, worst))
            assert worst <= bar, worst


@pytest.mark.gpu
def test_new_hooks_refuse_bad_arguments_gpu(fe):
    from d2slam_amd import api
    w = _weights()
    x = np.zeros((1, 2, 2, 128), np.float32)
    k = np.zeros((1, 4, 2), np.float32)
    raw = np.ones((1, 2, 2, 256), np.float32)
    head = lambda x, k=k, n=[1], ms=16, **kw: fe.debug_desc_head_sparse(x, k, n, ms, *w, **kw)      # noqa: E731
    nul = lambda: fe._lib.d2fe_debug_desc_head_sparse(fe._h, None, 128, 1, 2, 2, None, None, 4, 16, 0, 0, 0, None, None, None, None, None, None, None, None)      # noqa: E731
    bad = [nul,
           lambda: head(np.zeros((1, 1, 2, 128), np.float32)),                      # Hc < 2
           lambda: head(np.zeros((1, 2, 1, 128), np.float32)),                      # Wc < 2
           lambda: head(np.zeros((1, 2, 2, 124), np.float32)),                      # x_cstride < 128
           lambda: head(np.zeros((1, 2, 2, 130), np.float32)),                      # x_cstride no multiple of 4
           lambda: head(x, ms=0),                                                   # max_slots < 1
           lambda: head(x, k=np.zeros((1, 0, 2), np.float32)),                      # cap < 1
           lambda: head(x, img_w=-8),
           lambda: head(x, img_w=16, img_h=0),
           lambda: fe._lib.d2fe_debug_desc_head_sparse(fe._h, x.ctypes.data, 128, 1, 512, 512, k.ctypes.data, k.ctypes.data, 4, 16, 0, 0, 0, x.ctypes.data,
                                                       x.ctypes.data, x.ctypes.data, x.ctypes.data, x.ctypes.data, x.ctypes.data, x.ctypes.data, x.ctypes.data),      # 2^18 cells
           lambda: fe.debug_sample_a(np.ones((1, 1, 2, 256), np.float32), k, [1], 16, 16),                                   # Hc < 2
           lambda: fe.debug_sample_a(raw, k, [1], 0, 16),                                                                    # img_w < 1
           lambda: fe.debug_sample_a(raw, k, [1], 16, 0),
           lambda: fe.debug_sample_a(raw, k, [1], 16, 16, scap=0),
           lambda: fe.debug_sample_a(np.ones((1, 2, 2, 260), np.float32), k, [1], 16, 16, dcoff=8),                          # dcoff + 256 > dstride
           lambda: fe.debug_sample_a(np.ones((1, 2, 2, 258), np.float32), k, [1], 16, 16),                                   # dstride no multiple of 4
           lambda: fe.debug_sample_a(np.ones((1, 6, 256), np.float32), k, [1], 16, 16, slotmap=np.full((1, 2, 2), 6, np.int32)),      # a slot beyond the store
           lambda: fe.debug_sample_a(np.ones((1, 6, 256), np.float32), k, [1], 16, 16, slotmap=np.full((1, 2, 2), -2, np.int32)),
           lambda: fe.debug_sample_b(np.ones((1, 6, 256), np.float32), k, [1], slotmap=np.full((1, 2, 2), -2, np.int32)),
           lambda: fe.debug_sample_a(np.ones((1, 6, 256), np.float32), k, [1], 16, 16, slotmap=np.int32([[[-1, 0], [1, 2]]])),      # keypoint (0, 0) looks cell 0 up
           lambda: fe.debug_sample_b(np.ones((1, 6, 256), np.float32), k, [1], slotmap=np.int32([[[0, 1], [2, -1]]])),                # ... and cells 0 .. 3 in variant B
           lambda: fe._lib.d2fe_debug_sample_a(fe._h, raw.ctypes.data, 256, 0, 1, 2, 2, 16, 16, k.ctypes.data, k.ctypes.data, 4, 4, None, 0, raw.ctypes.data, None,
                                               64, raw.ctypes.data),                                                          # comp without mean
           lambda: fe._lib.d2fe_debug_sample_a(fe._h, raw.ctypes.data, 256, 0, 1, 2, 2, 16, 16, k.ctypes.data, k.ctypes.data, 4, 4, None, 0, raw.ctypes.data,
                                               raw.ctypes.data, 257, raw.ctypes.data)]                                        # pca_dims > 256
    for i, f in enumerate(bad):
        try:
            rc = f()
        except api.D2FEError as e:
            rc = e.code
        assert rc == -1, (i, rc)      # D2FE_ERR_INVALID
