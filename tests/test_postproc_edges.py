"""The SuperPoint tail kernels of csrc/postproc.hip -- softmax_cand_kernel, select_b_kernel, sample_b_kernel, nms2_a_kernel with nms2_wrap_fix_kernel -- on
injected tensors at their edges, through the d2fe_debug_* hooks of the development library (include/d2fe_debug.h).  The seeded SuperPoint weights compress the
scores into a narrow band, so the extractor never takes the low-word radix passes, the keep-all compaction, the -87 clamp of the exponential, the strided logit
staging or a keypoint in the last row; the generators below build the tensors that do.
CPU part (no marker): on the very inputs the GPU tests use, the oracle equals a plain independent statement of the operation (float64 softmax, numpy lexsort,
float64 bilinear sampling, the two-line NMS2 definition evaluated by recursion over raster order), and the regime each case is meant to reach is computed on
the host from its inputs and asserted.  GPU part (-m gpu): the kernel equals the oracle on those inputs -- bit for bit except for the descriptors, which are
held to the project's 1e-6 bar.

Pinned here: a variant-B keypoint in the LAST row or column (x = W - 1 or y = H - 1; reachable only with remove_borders = 0) has ix = Wc - 1 exactly in the
reference's arithmetic (superpoint_tensorrt.cpp:255-317), both clipped corner pairs coincide, all four weights are 0 and the descriptor is 0/0 = NaN -- in the
reference, in the oracle and on the device, at exactly those keypoints.

Break bytes: a set of keys that agree above byte b and spread over byte b stops the radix descent after pass b.  With max_kp = 200 that holds for b = 7 .. 1 only:
after pass 1 at most 256 keys share the prefix and fewer than 200 lie above them, 455 < sort_n = 1024 in all, so no set of keys reaches pass 0 at that K.  The
b = 0 set (3000 consecutive indices) therefore stops after pass 1 at max_kp = 200, and a ninth set (900 stronger keys above a group of 256 that differ in their
last byte only, max_kp = 1000) is the one whose descent runs all eight passes."""
import functools
import time

import numpy as np
import pytest

FLT_MIN = float(np.finfo(np.float32).tiny)
SEL_MAXSORT = 16384                       # csrc/postproc.hip
M32 = np.uint64(0xFFFFFFFF)


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


# ---- 1. softmax and candidates --------------------------------------------------------------------------------------------------------------------------------
GRIDS = ((2, 2), (3, 5), (13, 11))        # 4 cells: one partly filled block; 15; 143 = two full blocks and a partial one
TIE_GRID = (33, 32)                       # 1056 cells, the tie map only
KINDS = ("gauss1", "gauss20", "gauss100", "spike", "dustbin", "tie")
BATCHES = (("gauss1", "dustbin", "gauss20"), ("gauss100", "spike", "tie"))      # three images per launch; the dustbin image has no candidate at thr 0.015
LSTRIDES = (65, 72)
THR_NAMES = ("0.015", "map", "-1")


@functools.lru_cache(maxsize=None)
def _logits(kind, Hc, Wc):
    rng = np.random.RandomState(sum(map(ord, kind)) * 1000 + 37 * Hc + Wc)
    if kind.startswith("gauss"):
        l = rng.randn(Hc, Wc, 65) * float(kind[5:])
    elif kind == "spike":      # one channel at +200 over zeros (the zeros fall below the clamp: expf(-87) / s), a second at +120 in some cells (-80: above it)
        l = np.zeros((Hc, Wc, 65))
        ch = rng.randint(0, 65, size=(Hc, Wc))
        ch[0, 0], ch[0, 1] = 5, 64      # a score channel and the dustbin, whatever the draw
        second = (ch + 1 + rng.randint(0, 64, size=(Hc, Wc))) % 65
        has2 = rng.rand(Hc, Wc) < 0.5
        has2[0, 0] = True
        for cy in range(Hc):
            for cx in range(Wc):
                l[cy, cx, ch[cy, cx]] = 200.0
                if has2[cy, cx]:
                    l[cy, cx, second[cy, cx]] = 120.0
    elif kind == "dustbin":    # a dominant dustbin: all 64 scores tiny
        l = rng.randn(Hc, Wc, 65)
        l[..., 64] += 30.0
    else:                      # one 65-vector in every cell: each score word occurs Hc * Wc times
        l = np.broadcast_to(rng.randn(65) * 1.5, (Hc, Wc, 65)).copy()
    return _ro(l.astype(np.float32))


@functools.lru_cache(maxsize=None)
def _semi(kind, Hc, Wc):
    return _ro(_orc().softmax_semi(_logits(kind, Hc, Wc)))


def _unfold(a):
    """[Hc][Wc][64] -> [8 Hc][8 Wc]"""
    Hc, Wc, _ = a.shape
    return a.reshape(Hc, Wc, 8, 8).transpose(0, 2, 1, 3).reshape(Hc * 8, Wc * 8)


def _borders(H, W):
    return sorted({0, 1, 8, 9, min(H, W) // 2 + 1})      # the last one: nothing passes


def _pass_mask(semi, thr, border):
    """the candidate predicate (superpoint_tensorrt.cpp:201-230): score > thr, inside [border, dim - border)"""
    H, W = semi.shape
    y, x = np.mgrid[0:H, 0:W]
    return (semi > np.float32(thr)) & (y >= border) & (y < H - border) & (x >= border) & (x < W - border)


def _keys_of(semi, thr, border):
    """u64 keys (score_bits << 32) | (0xFFFFFFFF - raster) of the pixels passing the predicate, in raster order"""
    idx = np.flatnonzero(_pass_mask(semi, thr, border)).astype(np.uint64)
    return (_bits(semi).reshape(-1)[idx.astype(np.int64)].astype(np.uint64) << np.uint64(32)) | (M32 - idx)


def _thr(name, semi0):
    if name == "map":      # a value of the map itself: `>` is strict, the pixels holding it do not pass
        return float(np.sort(semi0.reshape(-1))[int(0.9 * semi0.size)])
    return float(name)


def _softmax_kinds():
    return [(k, g) for g in GRIDS for k in KINDS] + [("tie", TIE_GRID)]


def _clamped(logits):
    """[H][W] mask of the scores whose fp32 l - max lies below the exponential's clamp"""
    d = logits - logits.max(-1, keepdims=True)
    return _unfold(d[..., :64] < np.float32(-87.0))


def test_oracle_softmax_is_a_float64_softmax_above_the_clamp_and_expf_of_the_clamp_below():
    orc = _orc()
    e87 = np.float32(orc.expf(-87.0))
    worst_rel = worst_abs = 0.0
    n_sub = n_clamped = 0
    for kind, (Hc, Wc) in _softmax_kinds():
        l32 = _logits(kind, Hc, Wc)
        semi = _semi(kind, Hc, Wc)
        l = l32.astype(np.float64)
        d = l - l.max(-1, keepdims=True)
        ref = _unfold((np.exp(d) / np.exp(d).sum(-1, keepdims=True))[..., :64])
        cl = _clamped(l32)
        err = np.abs(semi.astype(np.float64) - ref)
        ok = ~cl
        assert np.all(err[ok] <= 8e-6 * ref[ok] + 2.0 ** -149), (kind, Hc, Wc, float((err[ok] / ref[ok]).max()))
        nz = ok & (ref > 1e-30)
        worst_rel = max(worst_rel, float((err[nz] / ref[nz]).max()))
        worst_abs = max(worst_abs, float(err[ok].max()))
        n_sub += int(((semi > 0) & (semi < FLT_MIN)).sum())
        n_clamped += int(cl.sum())
        if cl.any():
            # below the clamp: expf(-87) / s, with s the fp32 sum of the 65 exponentials in channel order, recomputed with the oracle's expf
            d32 = (l32 - l32.max(-1, keepdims=True)).reshape(-1, 65)
            u, inv = np.unique(d32, return_inverse=True)
            e = np.array([orc.expf(v) for v in u], np.float32)[inv.reshape(d32.shape)]
            s = np.zeros(len(e), np.float32)
            for c in range(65):
                s = s + e[:, c]
            want = _unfold(np.broadcast_to((e87 / s)[:, None], (len(s), 64)).reshape(Hc, Wc, 64))
            assert np.all(np.isfinite(semi[cl])) and np.all(semi[cl] <= e87)
            assert np.array_equal(_bits(semi[cl]), _bits(want[cl])), (kind, Hc, Wc)
    print("softmax oracle vs float64: worst relative %.3g, worst absolute %.3g; %d subnormal scores, %d scores below the clamp"
          % (worst_rel, worst_abs, n_sub, n_clamped))
    assert n_sub > 0 and n_clamped > 0
    s20 = _semi("gauss20", 13, 11)
    assert ((s20 > 0) & (s20 < FLT_MIN)).any(), "sigma = 20 is the set that is meant to hold subnormal scores"


def _softmax_launches():
    return [(g, b) for g in GRIDS for b in range(len(BATCHES))] + [(TIE_GRID, 2)]


def _batch_kinds(b):
    return BATCHES[b] if b < 2 else ("tie", "tie", "tie")


@pytest.mark.parametrize("grid,batch", _softmax_launches())
def test_softmax_batches_hold_an_image_without_candidates(grid, batch):
    Hc, Wc = grid
    semis = [_semi(k, Hc, Wc) for k in _batch_kinds(batch)]
    if batch == 0:
        assert _keys_of(semis[1], 0.015, 0).size == 0 and _keys_of(semis[0], 0.015, 0).size > 0
    for name in THR_NAMES:
        thr = _thr(name, semis[0])
        assert not any(_pass_mask(s, thr, _borders(*s.shape)[-1]).any() for s in semis)
        if name == "-1":
            assert all(_pass_mask(s, thr, 0).all() for s in semis)
        if name == "map":
            assert (semis[0] == np.float32(thr)).any() and not _pass_mask(semis[0], thr, 0)[semis[0] == np.float32(thr)].any()


@pytest.mark.gpu
@pytest.mark.parametrize("grid,batch", _softmax_launches())
def test_softmax_cand_gpu(fe, grid, batch):
    Hc, Wc = grid
    kinds = _batch_kinds(batch)
    semis = np.stack([_semi(k, Hc, Wc) for k in kinds])
    H, W = semis.shape[1:]
    for lstride in LSTRIDES:
        lg = np.full((3, Hc, Wc, lstride), np.nan, np.float32)      # the padding channels of the strided form are never to be read
        for i, k in enumerate(kinds):
            lg[i, :, :, :65] = _logits(k, Hc, Wc)
        for name in THR_NAMES:
            thr = _thr(name, semis[0])
            for border in _borders(H, W):
                semi, keys, cnt = fe.debug_softmax_cand(lg, thr, border, want_semi=True)
                assert np.array_equal(_bits(semi), _bits(semis)), (lstride, name, border)
                for i in range(3):
                    want = _keys_of(semis[i], thr, border)
                    assert int(cnt[i]) == want.size, (lstride, name, border, i, int(cnt[i]), want.size)
                    assert np.array_equal(np.sort(keys[i]), np.sort(want)), (lstride, name, border, i)
        _, keys, cnt = fe.debug_softmax_cand(lg, 0.015, 1, want_semi=False)      # without the dense map, as the extractor runs it
        for i in range(3):
            assert np.array_equal(np.sort(keys[i]), np.sort(_keys_of(semis[i], 0.015, 1)))


# ---- 2. selection on injected keys ----------------------------------------------------------------------------------------------------------------------------
def _split(keys):
    """(score fp32, score as exact float64, raster index int64) of u64 keys"""
    sc = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return sc, sc.astype(np.float64), (M32 - (keys & M32)).astype(np.int64)


def _select_ref(keys, W, max_kp, cap, always_sort=False):
    """The rule orc_select_b states (topKeypoints, superpoint_tensorrt.cpp:241-253): cut to max_kp -> (score descending, raster ascending); nothing cut -> raster
    order; then at most cap.  always_sort (variant A): sorted whatever the count, max_kp < 0 = up to cap."""
    sc, s64, idx = _split(keys)
    if always_sort or (max_kp != -1 and max_kp < len(keys)):
        order = np.lexsort((idx, -s64))[:cap if max_kp < 0 else max_kp]
    else:
        order = np.argsort(idx, kind="stable")
    order = order[:cap]
    i = idx[order]
    return np.stack([i % W, i // W], 1).astype(np.float32), sc[order], i.astype(np.uint32).view(np.int32)


def _sort_n(max_kp, cap):
    K = cap if max_kp < 0 else min(max_kp, cap)
    K = min(K, SEL_MAXSORT)
    n = 1024
    while n < K:
        n <<= 1
    return n


def _regime(keys, max_kp, cap, always_sort=False, has_semi=False):
    """Which path select_b_kernel takes for these keys, worked out on the host from the keys alone: 'compaction' (keep-all from the dense map), 'by_index' (keep-all,
    sorted on the raster word), 'all' (everything fits and is sorted on the key), 'select' or 'select_by_index' (keep-all, the lowest raster indices) -- then with the last pass of the MSB-first radix descent (7 .. 0; below 4
    = the passes over 0xFFFFFFFF - raster ran), the keys left for the LDS sort and how many keys tie with the K-th score beyond sort_n."""
    n, sort_n = len(keys), _sort_n(max_kp, cap)
    K = cap if max_kp < 0 else min(max_kp, cap)
    take_all = (n <= K or max_kp < 0) and not always_sort      # keep-all never sorts by score: beyond cap it is the first cap in raster order
    if take_all and n > sort_n and has_semi:
        return dict(path="compaction", sort_n=sort_n)
    K = min(K, sort_n)
    if take_all and n <= sort_n:
        return dict(path="by_index", sort_n=sort_n)
    if n <= K:
        return dict(path="all", sort_n=sort_n)
    if take_all:      # keep-all beyond the LDS sort without a dense map: the same descent over the keys with their words swapped (raster word first)
        keys = (keys << np.uint64(32)) | (keys >> np.uint64(32))
    prefix, mask, need = np.uint64(0), np.uint64(0), K
    for p in range(7, -1, -1):
        sh = np.uint64(8 * p)
        hist = np.bincount(((keys[(keys & mask) == prefix] >> sh) & np.uint64(0xFF)).astype(np.int64), minlength=256)
        suffix = np.cumsum(hist[::-1])[::-1]                       # S(d) = keys of the group with digit >= d
        d = int(np.flatnonzero(suffix >= need).max())
        above_d = int(suffix[d] - hist[d])
        left = (K - need) + above_d + int(hist[d])                 # keys >= the prefix chosen so far
        prefix |= np.uint64(d) << sh
        mask |= np.uint64(0xFF) << sh
        need -= above_d
        if left <= sort_n:
            break
    kth = np.sort(keys)[::-1][K - 1] >> np.uint64(32)
    return dict(path="select_by_index" if take_all else "select", sort_n=sort_n, last_pass=p, left=left, tied_beyond=max(0, int(((keys >> np.uint64(32)) >= kth).sum()) - sort_n))


def _sparse_map(H, W, n, rng, values):
    """[H][W] map, zero but for n random pixels holding `values` (n of them, or a callable of n)"""
    m = np.zeros(H * W, np.float32)
    at = rng.choice(H * W, n, replace=False)
    m[at] = values(n) if callable(values) else values
    return m.reshape(H, W)


def _distinct(rng, lo, hi):
    """n distinct fp32 scores in (lo, hi)"""
    def f(n):
        v = np.unique((lo + (hi - lo) * (0.001 + 0.998 * rng.rand(4 * n + 8))).astype(np.float32))
        assert len(v) >= n
        return rng.permutation(v)[:n]
    return f


def _case(maps=None, keys=None, W=None, H=None, thr=0.0, border=0, max_kp=200, cap=None, always_sort=False, pass_semi=False, seed=1):
    """A selection launch: dense maps (the keys are their candidates, handed over in shuffled order: the list order is free) or bare keys"""
    rng = np.random.RandomState(seed)
    if maps is not None:
        maps = [np.ascontiguousarray(m, np.float32) for m in maps]
        H, W = maps[0].shape
        raster = [_keys_of(m, thr, border) for m in maps]
    else:
        raster = [np.sort(k)[::-1] for k in keys]
    cap = cap if cap is not None else max_kp
    return dict(maps=maps, raster=raster, keys=[rng.permutation(k) for k in raster], W=W, H=H, thr=thr, border=border, max_kp=max_kp, cap=cap,
                always_sort=always_sort, pass_semi=pass_semi)


def _cell_map(Hc, Wc, value=0.5):
    """one pixel of every 8x8 cell at `value`: Hc * Wc equal score words with distinct raster indices"""
    m = np.zeros((Hc * 8, Wc * 8), np.float32)
    m[3::8, 5::8] = value
    return m


def _break_keys(b, rng, n=3000):
    """n unique keys that agree above byte b and spread over byte b (7 .. 4: bytes of the score word, scores in (0, 1); 3 .. 0: bytes of 0xFFFFFFFF - raster at one
    score).  Returns (keys, W, H) with W, H a map the raster indices fit in, or W = 65536 for indices no image has (the kernel only decodes them)."""
    r = rng.randint(0, 256, n).astype(np.uint64)
    if b >= 4:
        hi = {7: 0, 6: 0x3C << 24, 5: 0x3C80 << 16, 4: 0x3C8000 << 8}[b]
        if b == 7:
            r = rng.randint(1, 0x3F, n).astype(np.uint64)      # positive, below 0.5
        low = rng.randint(0, 1 << (8 * (b - 4)), n).astype(np.uint64) if b > 4 else np.zeros(n, np.uint64)
        word = np.uint64(hi) | (r << np.uint64(8 * (b - 4))) | low
        idx = rng.choice(64 * 64, n, replace=False).astype(np.uint64)
        return (word << np.uint64(32)) | (M32 - idx), 64, 64
    word = np.uint64(_bits(np.float32([0.5]))[0])
    if b == 0:
        idx, W, H = np.arange(n, dtype=np.uint64), 64, 64
    elif b == 1:
        idx, W, H = rng.choice(1 << 16, n, replace=False).astype(np.uint64), 256, 256
    else:
        idx = np.unique((r << np.uint64(8 * b)) | rng.randint(0, 1 << (8 * b), n).astype(np.uint64))
        W, H = 65536, 1
    assert len(idx) == n
    return (word << np.uint64(32)) | (M32 - idx), W, H


def _map_of_keys(keys, W, H):
    sc, _, idx = _split(keys)
    m = np.zeros(H * W, np.float32)
    m[idx] = sc
    return m.reshape(H, W)


@functools.lru_cache(maxsize=None)
def _sel_cases():
    rng = np.random.RandomState(20240)
    c = {}
    # deep ties: one score word, more keys than sort_n
    for K in (1, 200, 1024):
        c["deep_tie_K%d" % K] = _case(maps=[_cell_map(33, 32)], max_kp=K)
    c["deep_tie_sort_n_max"] = _case(maps=[_cell_map(129, 128)], max_kp=16384)
    m = np.zeros(64 * 64, np.float32)
    at = rng.permutation(64 * 64)
    m[at[:300]] = _distinct(rng, 0.6, 0.9)(300)
    m[at[300:1800]] = 0.5
    m[at[1800:2300]] = _distinct(rng, 0.1, 0.4)(500)
    c["tie_straddles_K"] = _case(maps=[m.reshape(64, 64)], max_kp=1024)
    # the descent stops after pass b
    for b in range(7, -1, -1):
        keys, W, H = _break_keys(b, rng)
        c["break_b%d" % b] = _case(maps=[_map_of_keys(keys, W, H)], max_kp=200) if W < 65536 else _case(keys=[keys], W=W, H=H, max_kp=200)
    m = np.zeros((64, 64), np.float32)
    m.reshape(-1)[:256] = 0.5
    m.reshape(-1)[1000:1900] = 0.75
    m.reshape(-1)[2000:3844] = 0.25
    c["break_b0_K1000"] = _case(maps=[m], max_kp=1000)
    # counts around K and around sort_n
    for K in (200, 1024):
        c["counts_K%d" % K] = _case(maps=[_sparse_map(64, 64, n, rng, _distinct(rng, 0.02, 0.9)) for n in (0, 1, K - 1, K, K + 1)], max_kp=K)
    c["n_eq_K_eq_sort_n_2048"] = _case(maps=[_sparse_map(64, 64, 2048, rng, _distinct(rng, 0.02, 0.9))], max_kp=2048)
    c["max_kp_above_cap"] = _case(maps=[_sparse_map(64, 64, 1000, rng, _distinct(rng, 0.02, 0.9))], max_kp=500, cap=200)
    c["cap_1"] = _case(maps=[_sparse_map(64, 64, 300, rng, _distinct(rng, 0.02, 0.9))], max_kp=200, cap=1)
    # score words: zeros (thr = -1 admits them), subnormals, one ulp apart, exactly 1.0 -- every pixel is a candidate
    m = np.zeros(64 * 64, np.float32)
    at = rng.permutation(64 * 64)
    m[at[:1000]] = rng.randint(1, 400, 1000).astype(np.uint32).view(np.float32)                       # subnormals, with ties
    m[at[1000:2000]] = (_bits(np.float32([0.25]))[0] + rng.randint(0, 300, 1000)).astype(np.uint32).view(np.float32)      # a ladder of ulps, with ties
    m[at[2000:2003]] = 1.0
    m[at[2003:3000]] = _distinct(rng, 0.0, 1.0)(997)
    assert (m == 0).sum() == 1096
    for K in (200, 3500):      # the K-th key: among the ulp ladder / among the 1096 zeros
        c["score_words_K%d" % K] = _case(maps=[m.reshape(64, 64)], thr=-1.0, max_kp=K)
    # keep-all
    u = rng.rand(160, 160).astype(np.float32)
    thr_u = float(np.sort(u.reshape(-1))[5000])
    c["keep_all_by_index"] = _case(maps=[_sparse_map(64, 64, 700, rng, _distinct(rng, 0.02, 0.9))], max_kp=-1, cap=1024, pass_semi=True)
    c["keep_all_compaction"] = _case(maps=[u], thr=thr_u, border=3, max_kp=-1, cap=160 * 160, pass_semi=True)
    # more candidates than the capacity: still raster order, the first cap of it -- from the map, from the keys alone, and where all keys fit the LDS sort
    c["keep_all_above_cap"] = _case(maps=[u], thr=thr_u, border=3, max_kp=-1, cap=5000, pass_semi=True)
    c["keep_all_above_cap_no_map"] = _case(maps=[u], thr=thr_u, border=3, max_kp=-1, cap=5000)
    c["keep_all_above_cap_by_index"] = _case(maps=[_sparse_map(64, 64, 700, rng, _distinct(rng, 0.02, 0.9))], max_kp=-1, cap=300, pass_semi=True)
    # always_sort (variant A): sorted also when nothing is cut
    lv = lambda n: np.float32([0.2, 0.4, 0.6, 0.8])[rng.randint(0, 4, n)]      # noqa: E731
    c["always_sort_n_le_K"] = _case(maps=[_sparse_map(64, 64, 500, rng, lv)], max_kp=1024, always_sort=True)
    c["always_sort_n_gt_K"] = _case(maps=[_sparse_map(64, 64, 3000, rng, lv)], max_kp=200, always_sort=True)
    # three regimes in one launch: empty, at most K (raster order), above K with the K-th key inside a tie group larger than sort_n
    m = np.zeros(64 * 64, np.float32)
    at = rng.permutation(64 * 64)
    m[at[:100]] = _distinct(rng, 0.6, 0.9)(100)
    m[at[100:1600]] = 0.5
    c["mixed_regimes"] = _case(maps=[np.zeros((64, 64), np.float32), _sparse_map(64, 64, 150, rng, _distinct(rng, 0.02, 0.9)), m.reshape(64, 64)], max_kp=200)
    return c


SEL_NAMES = ["deep_tie_K1", "deep_tie_K200", "deep_tie_K1024", "deep_tie_sort_n_max", "tie_straddles_K"] + ["break_b%d" % b for b in range(7, -1, -1)] + [
    "break_b0_K1000", "counts_K200", "counts_K1024", "n_eq_K_eq_sort_n_2048", "max_kp_above_cap", "cap_1", "score_words_K200", "score_words_K3500",
    "keep_all_by_index", "keep_all_compaction", "keep_all_above_cap", "keep_all_above_cap_no_map", "keep_all_above_cap_by_index", "always_sort_n_le_K", "always_sort_n_gt_K", "mixed_regimes"]
# what each case is there to reach: (image, path[, last pass of the descent; "low" = one of the four passes over the raster word])
SEL_REGIMES = {"deep_tie_K1": (0, "select", "low"), "deep_tie_K200": (0, "select", "low"), "deep_tie_K1024": (0, "select", "low"),
               "deep_tie_sort_n_max": (0, "select", "low"), "tie_straddles_K": (0, "select", 0), "break_b7": (0, "select", 7), "break_b6": (0, "select", 6), "break_b5": (0, "select", 5),
               "break_b4": (0, "select", 4), "break_b3": (0, "select", 3), "break_b2": (0, "select", 2), "break_b1": (0, "select", 1), "break_b0": (0, "select", 1),
               "break_b0_K1000": (0, "select", 0), "n_eq_K_eq_sort_n_2048": (0, "by_index"), "keep_all_by_index": (0, "by_index"),
               "keep_all_compaction": (0, "compaction"), "keep_all_above_cap": (0, "compaction"), "keep_all_above_cap_no_map": (0, "select_by_index"),
               "keep_all_above_cap_by_index": (0, "by_index"), "always_sort_n_le_K": (0, "all"), "always_sort_n_gt_K": (0, "select")}


def _case_regimes(cs):
    return [_regime(k, cs["max_kp"], cs["cap"], cs["always_sort"], cs["pass_semi"]) for k in cs["raster"]]


def test_selection_cases_reach_their_regimes():
    cases = _sel_cases()
    assert sorted(cases) == sorted(SEL_NAMES)
    for name in SEL_NAMES:
        cs = cases[name]
        rg = _case_regimes(cs)
        print(name, [len(k) for k in cs["raster"]], rg)
        for k in cs["raster"]:
            assert len(np.unique(k)) == len(k)
        if name in SEL_REGIMES:
            want = SEL_REGIMES[name]
            assert rg[want[0]]["path"] == want[1], (name, rg)
            if len(want) > 2:
                assert rg[want[0]]["last_pass"] in ((0, 1, 2, 3) if want[2] == "low" else (want[2],)), (name, rg)
    r = {n: _case_regimes(cases[n]) for n in SEL_NAMES}
    assert [len(k) for k in cases["deep_tie_K1"]["raster"]] == [1056] and [len(k) for k in cases["deep_tie_sort_n_max"]["raster"]] == [16512]
    assert [r["deep_tie_K%d" % K][0]["tied_beyond"] for K in (1, 200, 1024)] == [32, 32, 32] and r["deep_tie_sort_n_max"][0]["tied_beyond"] == 128
    assert r["tie_straddles_K"][0]["tied_beyond"] == 300 + 1500 - 1024
    assert len(cases["keep_all_compaction"]["raster"][0]) > SEL_MAXSORT and len(cases["keep_all_above_cap"]["raster"][0]) > 5000
    assert [x["path"] for x in r["mixed_regimes"]] == ["by_index", "by_index", "select"] and r["mixed_regimes"][2]["last_pass"] < 4
    assert [x["path"] for x in r["counts_K200"]] == ["by_index"] * 4 + ["select"] and [x["path"] for x in r["counts_K1024"]] == ["by_index"] * 4 + ["select"]
    assert r["score_words_K3500"][0]["path"] == "select"


@pytest.mark.parametrize("name", [n for n in SEL_NAMES if n not in ("break_b3", "break_b2")])
def test_oracle_selection_is_the_lexsort_rule(name):
    """oracle.select_b on the dense maps the keys come from (always_sort: oracle.nms2_a at distance 0, which suppresses nothing) against the numpy rule.  break_b3 and
    break_b2 spread their raster indices over bits no image has: there is no dense map to give the oracle, and the GPU test holds the kernel to the numpy rule."""
    orc = _orc()
    cs = _sel_cases()[name]
    for m, k in zip(cs["maps"], cs["raster"]):
        rk, rs, ri = _select_ref(k, cs["W"], cs["max_kp"], cs["cap"], cs["always_sort"])
        if cs["always_sort"]:
            ok, os_ = orc.nms2_a(m, cs["thr"], 0, cs["max_kp"], cap=cs["cap"])
        else:
            ok, os_, oi = orc.select_b(m, cs["thr"], cs["border"], cs["max_kp"], cap=cs["cap"])
            assert np.array_equal(oi, ri)
        assert np.array_equal(ok, rk) and np.array_equal(_bits(os_), _bits(rs))


def _run_select(fe, cs):
    semi = np.stack(cs["maps"]) if cs["pass_semi"] else None
    return fe.debug_select_b(cs["keys"], cs["W"], cs["H"], cs["max_kp"], cs["cap"], always_sort=cs["always_sort"], semi=semi, thr=cs["thr"], border=cs["border"])


def _assert_select(got, cs, name):
    assert len(got) == len(cs["raster"])
    for i, ((gk, gs, gi), k) in enumerate(zip(got, cs["raster"])):
        rk, rs, ri = _select_ref(k, cs["W"], cs["max_kp"], cs["cap"], cs["always_sort"])
        assert len(gs) == len(rs), (name, i, len(gs), len(rs))
        assert np.array_equal(gi, ri), (name, i, int((gi != ri).sum()))
        assert np.array_equal(gk, rk) and np.array_equal(_bits(gs), _bits(rs)), (name, i)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SEL_NAMES)
def test_select_b_gpu(fe, name):
    cs = _sel_cases()[name]
    t0 = time.perf_counter()
    got = _run_select(fe, cs)
    dt = time.perf_counter() - t0
    print("%s: hook call %.1f ms" % (name, 1e3 * dt))
    _assert_select(got, cs, name)


@pytest.mark.gpu
@pytest.mark.parametrize("max_kp", (1, 200, 1024))
def test_softmax_then_select_on_the_tie_map_gpu(fe, max_kp):
    """debug_softmax_cand -> debug_select_b, the extractor's own chain, on the map of 1056 copies of one cell"""
    orc = _orc()
    Hc, Wc = TIE_GRID
    lg = _logits("tie", Hc, Wc)
    semi = _semi("tie", Hc, Wc)
    H, W = semi.shape
    for border in (0, 4):
        _, keys, cnt = fe.debug_softmax_cand(lg[None], 0.015, border, want_semi=False)
        rg = _regime(np.sort(keys[0]), max_kp, max_kp)      # on the host, from the keys: without a border the strongest group alone holds 1056 > sort_n keys
        assert rg["path"] == "select" and (border or rg["last_pass"] < 4), rg
        (gk, gs, gi), = fe.debug_select_b(keys, W, H, max_kp, max_kp, thr=0.015, border=border)
        rk, rs, ri = orc.select_b(semi, 0.015, border, max_kp, cap=max_kp)
        assert np.array_equal(gk, rk) and np.array_equal(_bits(gs), _bits(rs)) and np.array_equal(gi, ri)


# ---- 3. descriptor sampling -----------------------------------------------------------------------------------------------------------------------------------
SAMPLE_GRIDS = ((2, 2), (2, 3), (12, 17))


@functools.lru_cache(maxsize=None)
def _raw(Hc, Wc, n=1):
    """[n][Hc][Wc][256]: per-cell magnitude 10^u, u uniform in [-12, 12], times a Gaussian: the squares stay inside the fp32 range and no row is zero"""
    rng = np.random.RandomState(700 + 31 * Hc + Wc + n)
    r = (rng.randn(n, Hc, Wc, 256) * 10.0 ** rng.uniform(-12, 12, size=(n, Hc, Wc, 1))).astype(np.float32)
    assert np.all(np.isfinite(r)) and np.all((r.astype(np.float64) ** 2).sum(-1) < 1e38) and np.all((r != 0).any(-1))
    return _ro(r)


def _all_pixels(Hc, Wc):
    y, x = np.mgrid[0:Hc * 8, 0:Wc * 8]
    return np.stack([x.reshape(-1), y.reshape(-1)], 1).astype(np.float32)


def _repeated(Hc, Wc):
    """a list that names keypoints twice and more: the corners of the map, the last full-weight pixel, random ones"""
    H, W = Hc * 8, Wc * 8
    rng = np.random.RandomState(H + W)
    k = np.array([[0, 0], [W - 1, 0], [0, H - 1], [W - 2, H - 2], [0, 0], [W - 2, H - 2], [3, 4], [4, 3], [3, 4]], np.float32)
    r = np.stack([rng.randint(0, W, 12), rng.randint(0, H, 12)], 1).astype(np.float32)
    return np.concatenate([k, r, r[::-1], k[::-1]])


def _sample_ref64(raw, kps):
    """normalize_keypoints, grid_sample and normalize_descriptors (superpoint_tensorrt.cpp:255-317) in float64; the weights from the CLIPPED corner coordinates, as
    the reference takes them"""
    Hc, Wc, _ = raw.shape
    dn = raw.astype(np.float64)
    dn = dn / np.sqrt((dn * dn).sum(-1, keepdims=True))
    x, y = kps[:, 0].astype(np.float64), kps[:, 1].astype(np.float64)
    ix = ((((x - 4 + 0.5) / (Wc * 8 - 4 - 0.5)) * 2 - 1) + 1) / 2 * (Wc - 1)
    iy = ((((y - 4 + 0.5) / (Hc * 8 - 4 - 0.5)) * 2 - 1) + 1) / 2 * (Hc - 1)
    x0 = np.clip(np.floor(ix).astype(int), 0, Wc - 1); y0 = np.clip(np.floor(iy).astype(int), 0, Hc - 1)
    x1 = np.clip(x0 + 1, 0, Wc - 1); y1 = np.clip(y0 + 1, 0, Hc - 1)
    v = (dn[y0, x0] * ((x1 - ix) * (y1 - iy))[:, None] + dn[y0, x1] * ((ix - x0) * (y1 - iy))[:, None]
         + dn[y1, x0] * ((x1 - ix) * (iy - y0))[:, None] + dn[y1, x1] * ((ix - x0) * (iy - y0))[:, None])
    with np.errstate(invalid="ignore", divide="ignore"):
        return v / np.sqrt((v * v).sum(-1, keepdims=True))


def _last_row_or_col(kps, Hc, Wc):
    return (kps[:, 0] == Wc * 8 - 1) | (kps[:, 1] == Hc * 8 - 1)


@functools.lru_cache(maxsize=None)
def _sample_oracle(Hc, Wc, which):
    orc = _orc()
    kps = _all_pixels(Hc, Wc) if which == "all" else _repeated(Hc, Wc)
    return _ro(kps, orc.sample_b(orc.l2norm_rows(_raw(Hc, Wc)[0]), kps))


@pytest.mark.parametrize("Hc,Wc", SAMPLE_GRIDS)
def test_oracle_sampling_is_the_float64_statement_and_nan_in_the_last_row_and_column(Hc, Wc):
    for which in ("all", "repeated"):
        kps, got = _sample_oracle(Hc, Wc, which)
        ref = _sample_ref64(_raw(Hc, Wc)[0], kps)
        edge = _last_row_or_col(kps, Hc, Wc)
        assert np.array_equal(~np.isfinite(got), np.broadcast_to(edge[:, None], got.shape))
        assert np.array_equal(~np.isfinite(ref), np.broadcast_to(edge[:, None], ref.shape))
        err = float(np.abs(got[~edge] - ref[~edge]).max())
        print("sample_b oracle vs float64, %dx%d cells, %s: %d keypoints, %d in the last row or column, worst %.3g" % (Hc, Wc, which, len(kps), edge.sum(), err))
        assert err <= 1e-6
    assert int(_last_row_or_col(_all_pixels(Hc, Wc), Hc, Wc).sum()) == 8 * Hc + 8 * Wc - 1      # 31 of 256, 39 of 384, 231 of 13 056


def _sparse_store(raw, seed):
    """(store [n][max_slots][256], slot map [n][Hc][Wc]): the rows of raw scattered over a store with spare slots, by a shuffled map the test makes itself"""
    n, Hc, Wc, _ = raw.shape
    rng = np.random.RandomState(seed)
    max_slots = Hc * Wc + 5
    store = np.full((n, max_slots, 256), np.nan, np.float32)
    slotmap = np.empty((n, Hc, Wc), np.int32)
    for i in range(n):
        slots = rng.permutation(max_slots)[:Hc * Wc]
        slotmap[i] = slots.reshape(Hc, Wc)
        store[i, slots] = raw[i].reshape(-1, 256)
    return store, slotmap


def _three_forms(fe, raw, kps, n_kp):
    """dense (dstride 256), dense inside the fused convPa|convDa layout (dstride 512, channel offset 256; the detector half is never to be read), sparse"""
    n, Hc, Wc, _ = raw.shape
    fused = np.full((n, Hc, Wc, 512), np.nan, np.float32)
    fused[..., 256:] = raw
    store, slotmap = _sparse_store(raw, 5 + Hc + Wc)
    return (fe.debug_sample_b(raw, kps, n_kp), fe.debug_sample_b(fused, kps, n_kp, dcoff=256), fe.debug_sample_b(store, kps, n_kp, slotmap=slotmap))


@pytest.mark.gpu
@pytest.mark.parametrize("which", ("all", "repeated"))
@pytest.mark.parametrize("Hc,Wc", SAMPLE_GRIDS)
def test_sample_b_gpu(fe, Hc, Wc, which):
    kps, ref = _sample_oracle(Hc, Wc, which)
    edge = _last_row_or_col(kps, Hc, Wc)
    assert edge.any() and np.array_equal(~np.isfinite(ref), np.broadcast_to(edge[:, None], ref.shape))
    dense, fused, sparse = _three_forms(fe, _raw(Hc, Wc), kps[None], [len(kps)])
    for name, d in (("dense", dense), ("fused", fused), ("sparse", sparse)):
        d = d[0]
        assert np.array_equal(~np.isfinite(d), ~np.isfinite(ref)), (name, int((~np.isfinite(d)).any(1).sum()), int(edge.sum()))
        err = float(np.abs(d[~edge] - ref[~edge]).max())
        print("sample_b %s vs oracle, %dx%d cells, %s: worst %.3g" % (name, Hc, Wc, which, err))
        assert err <= 1e-6, (name, err)
        assert np.array_equal(_bits(d[~edge]), _bits(dense[0][~edge])), name + " differs from the dense form"


@pytest.mark.gpu
@pytest.mark.parametrize("Hc,Wc", SAMPLE_GRIDS)
def test_sample_b_counts_of_0_1_and_cap_gpu(fe, Hc, Wc):
    """three images, n_kp = 0, 1 and cap: rows at and beyond an image's count are not written (the hook hands out an output of all-ones words)"""
    orc = _orc()
    cap = 41
    raw = _raw(Hc, Wc, 3)
    rng = np.random.RandomState(Hc * Wc)
    kps = np.stack([rng.randint(0, Wc * 8 - 1, (3, cap)), rng.randint(0, Hc * 8 - 1, (3, cap))], -1).astype(np.float32)
    n_kp = [0, 1, cap]
    for name, d in zip(("dense", "fused", "sparse"), _three_forms(fe, raw, kps, n_kp)):
        for i in range(3):
            ref = orc.sample_b(orc.l2norm_rows(raw[i]), kps[i, :n_kp[i]])
            assert np.all(np.isfinite(d[i, :n_kp[i]])) and (n_kp[i] == 0 or float(np.abs(d[i, :n_kp[i]] - ref).max()) <= 1e-6), (name, i)
            assert np.all(_bits(d[i, n_kp[i]:]) == 0xFFFFFFFF), (name, i)


# ---- 4. NMS2 (variant A) --------------------------------------------------------------------------------------------------------------------------------------
NMS_THR = 0.05
NMS_DISTS = (0, 1, 4, 10, 40)
NMS_MAPS = ("plateau", "falling", "rising", "quantised", "uniform")


def _row_map(H, W, y, a, b):
    m = np.zeros((H, W), np.float32)
    m[y] = np.linspace(a, b, W).astype(np.float32)
    assert len(np.unique(m[y])) == W
    return m


@functools.lru_cache(maxsize=None)
def _nms_map(kind):
    rng = np.random.RandomState(sum(map(ord, kind)))
    H, W = 24, 40
    if kind == "plateau":        # equal confidences do not suppress one another: `>` against `>=`
        m = np.where(rng.rand(H, W) < 0.5, 0.5, 0.0)
    elif kind == "falling":      # every other candidate survives at dist 1: the alternating chain
        m = _row_map(H, W, 10, 0.9, 0.1)
    elif kind == "rising":       # only the last survives
        m = _row_map(H, W, 10, 0.1, 0.9)
    elif kind == "quantised":
        m = np.float32([0.0, 0.25, 0.5, 0.75])[rng.randint(0, 4, (H, W))]
    else:
        m = rng.rand(H, W)
    return _ro(np.ascontiguousarray(m, np.float32))


def _nms2_ref(m, thr, d, max_kp):
    """The definition in the comment of nms2_a_kernel, evaluated in raster order:
         active(P)  <=> no raster-earlier active Q within Chebyshev distance d with conf(Q) > conf(P)
         survive(P) <=> active(P) and no raster-later active R within d with conf(R) > conf(P)
    then confidence descending, raster ascending, at most max_kp."""
    H, W = m.shape
    act = np.zeros((H, W), np.float32)      # conf where active, 0 elsewhere (candidates have conf > thr > 0)
    cand = [(y, x) for y in range(H) for x in range(W) if m[y, x] > np.float32(thr)]
    for y, x in cand:
        p, x0, x1 = m[y, x], max(0, x - d), min(W, x + d + 1)
        if not ((act[max(0, y - d):y, x0:x1] > p).any() or (act[y, x0:x] > p).any()):
            act[y, x] = p
    keep = []
    for y, x in cand:
        p, x0, x1 = m[y, x], max(0, x - d), min(W, x + d + 1)
        if act[y, x] > 0 and not ((act[y + 1:y + d + 1, x0:x1] > p).any() or (act[y, x + 1:x1] > p).any()):
            keep.append((y * W + x, p))
    idx = np.array([k[0] for k in keep], np.int64)
    sc = np.array([k[1] for k in keep], np.float32)
    order = np.lexsort((idx, -sc.astype(np.float64)))[:max_kp]
    return np.stack([idx[order] % W, idx[order] // W], 1).astype(np.float32).reshape(-1, 2), sc[order]


@functools.lru_cache(maxsize=None)
def _nms_oracle(kind, dist, max_kp):
    return _ro(*_orc().nms2_a(_nms_map(kind), NMS_THR, dist, max_kp, cap=max_kp))


@pytest.mark.parametrize("kind", NMS_MAPS)
def test_oracle_nms2_is_the_two_line_definition(kind):
    m = _nms_map(kind)
    for dist in NMS_DISTS:
        for max_kp in (1024, 20):
            ok, os_ = _nms_oracle(kind, dist, max_kp)
            rk, rs = _nms2_ref(m, NMS_THR, dist, max_kp)
            assert np.array_equal(ok, rk) and np.array_equal(_bits(os_), _bits(rs)), (kind, dist, max_kp)
    n = int((m > NMS_THR).sum())
    if kind == "plateau":
        assert all(len(_nms_oracle(kind, d, 1024)[1]) == n for d in NMS_DISTS)
    if kind == "falling":
        assert np.array_equal(_nms_oracle(kind, 1, 1024)[0][:, 0], np.arange(0, 40, 2))
    if kind == "rising":
        assert [tuple(k) for k in _nms_oracle(kind, 1, 1024)[0]] == [(39.0, 10.0)]


@pytest.mark.gpu
@pytest.mark.parametrize("dist", NMS_DISTS)
def test_nms2_a_gpu(fe, dist):
    maps = np.stack([_nms_map(k) for k in NMS_MAPS])      # five images in one launch
    for max_kp in (1024, 20):
        got = fe.debug_nms2_a(maps, NMS_THR, dist, max_kp, max_kp)
        for kind, (gk, gs, gi) in zip(NMS_MAPS, got):
            ok, os_ = _nms_oracle(kind, dist, max_kp)
            assert len(gs) == len(os_), (kind, dist, max_kp, len(gs), len(os_))
            assert np.array_equal(gk, ok) and np.array_equal(_bits(gs), _bits(os_)), (kind, dist, max_kp)
            assert np.array_equal(gi, (ok[:, 1] * 40 + ok[:, 0]).astype(np.int32))


@pytest.mark.gpu
def test_nms2_a_long_chain_gpu(fe):
    """a falling row 640 long at dist 1: candidate k is decided by candidate k - 1, so the in-place fixpoint needs the sweeps of one wave to see those of another"""
    orc = _orc()
    m = _row_map(16, 640, 7, 0.9, 0.1)
    ok, os_ = orc.nms2_a(m, NMS_THR, 1, 1024, cap=1024)
    assert np.array_equal(np.sort(ok[:, 0]), np.arange(0, 640, 2)) and np.all(ok[:, 1] == 7)
    (gk, gs, gi), = fe.debug_nms2_a(m[None], NMS_THR, 1, 1024, 1024)
    assert np.array_equal(gk, ok) and np.array_equal(_bits(gs), _bits(os_))


@pytest.mark.gpu
def test_nms2_a_ties_past_sort_n_and_index_wrap_gpu(fe):
    """264x256 at a constant 0.5: 67 584 candidates, all survive, max_kp = 1024 -- ties past sort_n in the always_sort selection, and more candidates than the
    reference's CV_16UC1 index map holds.  A second image keeps its strongest 2048 pixels at the END of the raster, at ranks past 65 536, where the wrap moves
    the reported coordinates."""
    orc = _orc()
    H, W = 264, 256
    a = np.full((H, W), 0.5, np.float32)
    b = np.full((H, W), 0.25, np.float32)
    b.reshape(-1)[-2048:] = 0.5
    for m, dist in ((a, 4), (b, 0)):
        ok, os_ = orc.nms2_a(m, NMS_THR, dist, 1024, cap=1024)
        assert len(os_) == 1024 and np.all(os_ == 0.5)
        keys = _keys_of(m, NMS_THR, 0)
        rg = _regime(keys, 1024, 1024, always_sort=True)
        assert len(keys) == 67584 and rg["path"] == "select" and rg["last_pass"] < 4
        (gk, gs, gi), = fe.debug_nms2_a(m[None], NMS_THR, dist, 1024, 1024)
        assert np.array_equal(gk, ok) and np.array_equal(_bits(gs), _bits(os_))
        assert np.array_equal(gi, (ok[:, 1] * W + ok[:, 0]).astype(np.int32))
    assert ok[0, 1] * W + ok[0, 0] == H * W - 2048 - 65536      # the wrap is visible in the second image


# ---- 5. the hooks refuse what they cannot run -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_hooks_refuse_bad_arguments_gpu(fe):
    from d2slam_amd import api
    lg = np.zeros((1, 2, 2, 65), np.float32)
    k = [np.arange(4, dtype=np.uint64)]
    bad = [lambda: fe.debug_softmax_cand(np.zeros((1, 1, 2, 65), np.float32), 0.015, 0),
           lambda: fe.debug_softmax_cand(np.zeros((1, 2, 1, 65), np.float32), 0.015, 0),
           lambda: fe.debug_softmax_cand(np.zeros((1, 2, 2, 64), np.float32), 0.015, 0),
           lambda: fe._lib.d2fe_debug_softmax_cand(fe._h, None, 65, 1, 2, 2, 0.015, 0, 0, None, None, None),
           lambda: fe._lib.d2fe_debug_softmax_cand(fe._h, lg.ctypes.data, 65, 0, 2, 2, 0.015, 0, 0, None, lg.ctypes.data, lg.ctypes.data),
           lambda: fe.debug_select_b(k, 16, 16, 200, 0),
           lambda: fe.debug_select_b(k, 16, 16, 200, 200, counts=[5]),      # a count above cand_cap
           lambda: fe.debug_select_b(k, 2048, 2048, 200, 200),             # H * W > 2^21
           lambda: fe.debug_sample_b(np.ones((1, 1, 2, 256), np.float32), np.zeros((1, 1, 2), np.float32), [1]),
           lambda: fe.debug_sample_b(np.ones((1, 6, 256), np.float32), np.zeros((1, 1, 2), np.float32), [1], slotmap=np.full((1, 2, 2), 6, np.int32)),
           lambda: fe.debug_nms2_a(np.zeros((1, 2048, 2048), np.float32), 0.05, 1, 10, 10),
           lambda: fe.debug_nms2_a(np.zeros((1, 16, 16), np.float32), 0.05, 1, 10, 0)]
    for i, f in enumerate(bad):
        try:
            rc = f()
        except api.D2FEError as e:
            rc = e.code
        assert rc == -1, (i, rc)      # D2FE_ERR_INVALID
