"""GPU parity tests (-m gpu): the HIP path, called through the C ABI, against the oracle on identical inputs.
 * exact mode (fp32 MFMA): activations, scores, keypoint indices BIT-EXACT; descriptors <= 1e-6
 * fast mode (fp16 hi/lo split): descriptors <= 1e-4 (north_star tolerance), scores <= 1e-5; indices equal except
   at score near-ties (checked as: the symmetric difference of the keypoint sets only contains near-boundary scores)
 * matcher: indices and distances bit-exact
"""
import os

import numpy as np
import pytest

from d2slam_amd.synth import synth_descriptor_pair, synth_image, synth_stereo

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from d2slam_amd import api as a
    a.load_library()
    return a


def _fe(api, H, W, n, prec, max_kp=200, thr=0.015, dense=False, dev=False):
    fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=max_kp, input_width=W, input_height=H, max_batch=n, precision=prec,
                                           keypoint_threshold=thr, keep_score_map=True, dense_descriptors=dense), dev=dev)
    return fe


def _fe_dev(api, *a, **k):
    """a handle of the development library: the tests that read intermediate tensors back (d2fe_debug_read, include/d2fe_debug.h)"""
    return _fe(api, *a, dev=True, **k)


LAYERS = [("conv1a", 1, 64), ("conv1b", 2, 64), ("conv2a", 2, 64), ("conv2b", 4, 64), ("conv3a", 4, 128), ("conv3b", 8, 128),
          ("conv4a", 8, 128), ("conv4b", 8, 128)]


def _oracle_layers(orc, img, w):
    x = orc.prep_u8(img)[:, :, None]
    out = {}
    x = orc.conv(x, *w["conv1a"], True); out["conv1a"] = x
    x = orc.maxpool2(orc.conv(x, *w["conv1b"], True)); out["conv1b"] = x
    x = orc.conv(x, *w["conv2a"], True); out["conv2a"] = x
    x = orc.maxpool2(orc.conv(x, *w["conv2b"], True)); out["conv2b"] = x
    x = orc.conv(x, *w["conv3a"], True); out["conv3a"] = x
    x = orc.maxpool2(orc.conv(x, *w["conv3b"], True)); out["conv3b"] = x
    x = orc.conv(x, *w["conv4a"], True); out["conv4a"] = x
    x = orc.conv(x, *w["conv4b"], True); out["conv4b"] = x
    return out


@pytest.mark.parametrize("H,W", [(96, 128), (104, 136), (72, 200), (101, 99)])
def test_exact_mode_bitwise_every_layer(api, orc, sp_weights, H, W):
    """fp32 MFMA conv stack == oracle fmaf chains, bit for bit, incl. ragged tiles (sizes not multiples of the tile)."""
    n = 2
    imgs = np.stack([synth_image(H, W, 10 + s) for s in range(n)])
    fe = _fe_dev(api, H, W, n, api.PREC_F32, dense=True)          # the dense descriptor map is inspected below
    fe.load_superpoint(sp_weights)
    res = fe.extract_batch(imgs, cap=200)
    for i in range(n):
        ref = _oracle_layers(orc, imgs[i], sp_weights)
        for name, div, c in LAYERS:
            got = fe.debug_read(name, (n, H // div, W // div, c))[i]
            assert np.array_equal(got, ref[name]), "%s differs (max %g)" % (name, np.abs(got - ref[name]).max())
        f = orc.superpoint_forward(imgs[i], sp_weights)
        assert np.array_equal(fe.debug_read("logits", (n, H // 8, W // 8, 65))[i], f["logits"])
        assert np.array_equal(fe.debug_read("desc_raw", (n, H // 8, W // 8, 256))[i], f["desc_raw"])
        assert np.array_equal(fe.debug_read("semi", (n, (H // 8) * 8, (W // 8) * 8))[i], f["semi"])
        rk, rs, ri = orc.select_b(f["semi"], 0.015, 1, 200)
        kps, sc, desc = res[i]
        assert np.array_equal(kps, rk) and np.array_equal(sc, rs)
        assert np.abs(desc - orc.sample_b(f["desc"], rk)).max() <= 1e-6
    fe.close()


@pytest.mark.parametrize("prec", ["f32", "wino", "f16x2"])
@pytest.mark.parametrize("H,W", [(100, 100), (150, 134), (101, 99), (487, 645)])
def test_sizes_that_are_not_multiples_of_8(api, orc, sp_weights, H, W, prec):
    """The reference's engine profile admits any size in 100x100 .. 1500x1500 (superpoint_tensorrt.cpp:50-55).  The three max-pools floor,
    the score map is (H/8)*8 x (W/8)*8 and processOutput works in ITS coordinates (semi_dims_, :331-336): same here, bit for bit in
    the fp32 modes (incl. odd sizes at every pooling level)."""
    n = 4
    imgs = np.stack([synth_image(H, W, 20 + s) for s in range(n)])
    P = {"f32": api.PREC_F32, "wino": api.PREC_F32_WINO, "f16x2": api.PREC_F16X2}[prec]
    for dense in (True, False):
        fe = api.DevFrontEnd(api.SuperPointConfig(max_keypoints=150, input_width=W, input_height=H, max_batch=n, precision=P,
                                               keep_score_map=True, dense_descriptors=dense))
        fe.load_superpoint(sp_weights)
        res = fe.extract_batch(imgs, cap=150)
        Hs, Ws = (H // 8) * 8, (W // 8) * 8
        semi = fe.debug_read("semi", (n, Hs, Ws))
        for i in (0, n - 1):
            f = orc.superpoint_forward(imgs[i], sp_weights, wino=(prec == "wino"))
            assert f["semi"].shape == (Hs, Ws)
            kps, sc, desc = res[i]
            if prec == "f16x2":
                assert np.abs(semi[i] - f["semi"]).max() <= 1e-5
                continue
            assert np.array_equal(semi[i], f["semi"])
            rk, rs, ri = orc.select_b(f["semi"], 0.015, 1, 150)
            assert np.array_equal(kps, rk) and np.array_equal(sc, rs)
            assert np.abs(desc - orc.sample_b(f["desc"], rk)).max() <= (1e-6 if dense or prec == "f32" else 1e-5)
        fe.close()


def test_exact_mode_full_size_stereo(api, orc, sp_weights):
    """BASELINE config[1] size: 640x480 stereo pair, 200 keypoints: indices exact, descriptors <= 1e-6."""
    l, r = synth_stereo(480, 640, seed=1)
    imgs = np.stack([l, r])
    fe = _fe(api, 480, 640, 2, api.PREC_F32)
    fe.load_superpoint(sp_weights)
    res = fe.extract_batch(imgs, cap=200)
    descs = []
    for i in range(2):
        rk, rs, rd, ri, f = orc.extract_b(imgs[i], sp_weights, 0.015, 1, 200)
        kps, sc, desc = res[i]
        assert len(kps) == 200
        assert np.array_equal(kps, rk) and np.array_equal(sc, rs)
        assert np.abs(desc - rd).max() <= 1e-6
        descs.append((desc, rd, kps))
    # end to end: matches computed from the GPU descriptors equal the oracle's matches of the oracle descriptors
    q, t, d = fe.match_knn(descs[0][0], descs[1][0], 0.8, descs[0][2], descs[1][2], 0.2 * 640)
    rq, rt, rdist = orc.match_knn(descs[0][0], descs[1][0], 0.8, descs[0][2], descs[1][2], 0.2 * 640)
    assert np.array_equal(q, rq) and np.array_equal(t, rt) and np.array_equal(d, rdist)
    fe.close()


def test_raster_order_when_fewer_than_max(api, orc, sp_weights):
    """K <= N: the reference does not sort (superpoint_tensorrt.cpp:242) -> raster order; also the empty case."""
    img = synth_image(96, 128, 5)
    f = orc.superpoint_forward(img, sp_weights)
    thr = float(np.sort(f["semi"].reshape(-1))[-40])      # ~39 candidates above
    fe = _fe(api, 96, 128, 1, api.PREC_F32, max_kp=200, thr=thr)
    fe.load_superpoint(sp_weights)
    (kps, sc, desc), = fe.extract_batch(img[None], cap=200)
    rk, rs, ri = orc.select_b(f["semi"], thr, 1, 200)
    assert 0 < len(rk) < 200 and np.array_equal(kps, rk) and np.array_equal(sc, rs)
    assert np.all(np.diff(ri) > 0)
    fe.close()
    fe = _fe(api, 96, 128, 1, api.PREC_F32, max_kp=200, thr=0.99)
    fe.load_superpoint(sp_weights)
    (kps, sc, desc), = fe.extract_batch(img[None], cap=200)
    assert len(kps) == 0 and len(sc) == 0 and desc.shape == (0, 256)
    fe.close()


def test_score_ties_use_raster_tiebreak(api, orc, sp_weights):
    """A constant image makes every interior cell identical -> massive exact score ties; selection must still equal
    the oracle's (score desc, raster asc)."""
    img = np.full((96, 128), 127, np.uint8)
    f = orc.superpoint_forward(img, sp_weights)
    thr = float(np.median(f["semi"]))
    fe = _fe(api, 96, 128, 1, api.PREC_F32, max_kp=64, thr=thr)
    fe.load_superpoint(sp_weights)
    (kps, sc, desc), = fe.extract_batch(img[None], cap=64)
    rk, rs, ri = orc.select_b(f["semi"], thr, 1, 64)
    assert len(rk) == 64 and np.array_equal(kps, rk) and np.array_equal(sc, rs)
    fe.close()


# every BASELINE geometry: d435 640x480 N=200, quadcam 800x400 N=100 (threshold 0.15 there; the tolerance test keeps 0.015 so that the
# top-K boundary is exercised), TUM 512x512 N=150
@pytest.mark.parametrize("H,W,N", [(96, 128, 200), (480, 640, 200), (400, 800, 100), (512, 512, 150)])
def test_fast_mode_tolerances(api, orc, sp_weights, H, W, N):
    imgs = np.stack(synth_stereo(H, W, seed=3))
    fe = _fe_dev(api, H, W, 2, api.PREC_F16X2, dense=True, max_kp=N)
    fe.load_superpoint(sp_weights)
    res = fe.extract_batch(imgs, cap=N)
    for i in range(2):
        f = orc.superpoint_forward(imgs[i], sp_weights)
        semi = fe.debug_read("semi", (2, H, W))[i]
        assert np.abs(semi - f["semi"]).max() <= 1e-5
        assert np.abs(fe.debug_read("desc_raw", (2, H // 8, W // 8, 256))[i] - f["desc_raw"]).max() <= 1e-4
        rk, rs, ri = orc.select_b(f["semi"], 0.015, 1, N)
        kps, sc, desc = res[i]
        gi = (kps[:, 1] * W + kps[:, 0]).astype(np.int64)
        common = np.intersect1d(gi, ri)
        assert len(common) >= 0.75 * N, "fast mode keypoint set diverged: %d common" % len(common)
        # a keypoint can only enter/leave the top-K if its score is within 2*eps of the K-th score, eps = max score error
        eps = float(np.abs(semi - f["semi"]).max())
        kth = rs[-1]
        for j in np.setxor1d(gi, ri):
            assert abs(f["semi"].reshape(-1)[j] - kth) <= 2 * eps + 1e-9, (j, f["semi"].reshape(-1)[j], kth, eps)
        # descriptors of the shared keypoints: 1e-4 (north_star), actually ~1e-6
        rd = orc.sample_b(f["desc"], rk)
        pos_g = {int(v): k for k, v in enumerate(gi)}
        pos_r = {int(v): k for k, v in enumerate(ri)}
        dg = np.stack([desc[pos_g[int(c)]] for c in common]); dr = np.stack([rd[pos_r[int(c)]] for c in common])
        assert np.abs(dg - dr).max() <= 1e-4
        assert np.abs(dg - dr).max() <= 5e-6
    fe.close()


MATCH_CASES = [(200, 200, 256, 0.8, -1.0, 0.05), (150, 97, 256, 0.7, 32.0, 0.2), (33, 200, 64, 0.9, -1.0, 0.05),
               (100, 100, 256, 0.9, 19.2, 0.05), (200, 150, 32, 0.8, -1.0, 0.2), (257, 300, 256, 0.8, -1.0, 0.05),
               (1, 5, 256, 0.8, -1.0, 0.05), (5, 1, 256, 0.8, -1.0, 0.05), (2, 2, 256, 0.8, -1.0, 0.05), (1024, 1000, 128, 0.8, -1.0, 0.1)]


@pytest.mark.parametrize("na,nb,dim,ratio,radius,sigma", MATCH_CASES)
def test_match_knn_and_crosscheck_exact(api, orc, na, nb, dim, ratio, radius, sigma):
    fe = _fe(api, 64, 64, 1, api.PREC_F32)
    a, b, pa, pb = synth_descriptor_pair(na, nb, dim, seed=na * 7 + nb, sigma=sigma)
    q, t, d = fe.match_knn(a, b, ratio, pa, pb, radius)
    rq, rt, rd = orc.match_knn(a, b, ratio, pa, pb, radius)
    assert np.array_equal(q, rq) and np.array_equal(t, rt) and np.array_equal(d, rd)
    q, t, d = fe.match_crosscheck(a, b)
    rq, rt, rd = orc.match_crosscheck(a, b)
    assert np.array_equal(q, rq) and np.array_equal(t, rt) and np.array_equal(d, rd)
    fe.close()


def test_match_edge_cases(api, orc):
    fe = _fe(api, 64, 64, 1, api.PREC_F32)
    a, b, pa, pb = synth_descriptor_pair(50, 60, 256, seed=1)
    q, t, d = fe.match_knn(a[:0], b, 0.8)
    assert len(q) == 0
    q, t, d = fe.match_knn(a, b[:0], 0.8)
    assert len(q) == 0
    # duplicated train rows: exact distance ties -> lower index wins, ratio test d0 < r*d1 fails (d0 == d1)
    b2 = np.concatenate([b, b[:10]])
    q, t, d = fe.match_knn(a, b2, 0.8)
    rq, rt, rd = orc.match_knn(a, b2, 0.8)
    assert np.array_equal(q, rq) and np.array_equal(t, rt) and np.array_equal(d, rd)
    # self match: identity with zero distance (size-independent property)
    q, t, d = fe.match_knn(a, a, 0.8)
    assert np.array_equal(q, np.arange(50)) and np.array_equal(t, np.arange(50)) and np.all(d == 0)
    # too many rows -> loud error, not silence
    with pytest.raises(api.D2FEError):
        fe.match_knn(np.zeros((16385, 256), np.float32), b, 0.8)
    fe.close()


@pytest.mark.parametrize("na,nb,dim", [(1025, 1500, 256), (3000, 2000, 128), (5000, 700, 64)])
def test_match_more_than_1024_rows(api, orc, na, nb, dim):
    """The matcher takes up to 16384 rows per side (the reference's matchKNN is unbounded; keep-all extractions produce thousands of
    keypoints): exact against the oracle, as for small sets."""
    fe = _fe(api, 64, 64, 1, api.PREC_F32)
    a, b, pa, pb = synth_descriptor_pair(na, nb, dim, seed=na + nb, sigma=0.1)
    for radius in (-1.0, 60.0):
        q, t, d = fe.match_knn(a, b, 0.8, pa, pb, radius)
        rq, rt, rd = orc.match_knn(a, b, 0.8, pa, pb, radius)
        assert len(rq) > 100 and np.array_equal(q, rq) and np.array_equal(t, rt) and np.array_equal(d, rd)
    q, t, d = fe.match_crosscheck(a, b)
    rq, rt, rd = orc.match_crosscheck(a, b)
    assert np.array_equal(q, rq) and np.array_equal(t, rt) and np.array_equal(d, rd)
    fe.close()


def _unit(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


SATURATED = ["eight_identical_train_rows", "twenty_identical_train_rows", "all_equal_train_set", "self_plus_noise_1e-7", "six_near_copies_of_every_row",
             "both_sets_all_equal"]


def saturated_pair(case):
    """the descriptor sets of one SATURATED case (tests/test_launch_regimes.py runs them again as a batch of 64 pairs)"""
    rng = np.random.RandomState(11)
    a = _unit(rng.randn(150, 256)); b = _unit(rng.randn(180, 256))
    if case == "eight_identical_train_rows":
        b[20:28] = b[20]; a[5] = _unit(b[20:21] + 1e-3 * rng.randn(1, 256))[0]; a[6] = b[20]
    elif case == "twenty_identical_train_rows":
        b[20:40] = b[20]; a[5] = _unit(b[20:21] + 1e-3 * rng.randn(1, 256))[0]; a[6] = b[20]
    elif case == "all_equal_train_set":
        b[:] = b[0]
    elif case == "self_plus_noise_1e-7":
        b = (a + np.float32(1e-7) * rng.randn(*a.shape).astype(np.float32)).astype(np.float32)
        b = np.concatenate([b, b[::-1][:40]])            # and 40 rows twice, at other indices
    elif case == "six_near_copies_of_every_row":
        base = _unit(rng.randn(30, 256))
        b = np.concatenate([base + np.float32(3e-8) * rng.randn(30, 256).astype(np.float32) for _ in range(6)]).astype(np.float32)
        a = _unit(base[rng.randint(0, 30, 150)] + 0.05 * rng.randn(150, 256))
    elif case == "both_sets_all_equal":
        a[:] = a[0]; b[:] = a[0]
    return a, b


@pytest.mark.parametrize("case", SATURATED)
def test_match_saturated_candidate_lists_are_exact(api, orc, case):
    """Many train rows within fp32 round-off of the nearest distance (repeated texture, a frame against a near-copy): every row the
    Gram-trick distance cannot separate from the second neighbour must be re-ranked exactly, and beyond the kernel's 16 candidate slots
    per query the exact scan of every row must run (match.hip header).
    Indices AND distances bitwise against the oracle and, when present, the reference's own matchKNN (oracle/_ref)."""
    from oracle import ref
    a, b = saturated_pair(case)
    fe = _fe(api, 64, 64, 1, api.PREC_F32)
    fe.match_fallback_rows(reset=True)
    for ratio in (0.8, 1.5):          # 1.5: ties pass the ratio test, so a wrong index among equals would surface as a wrong match
        q, t, d = fe.match_knn(a, b, ratio)
        rq, rt, rd = orc.match_knn(a, b, ratio)
        assert np.array_equal(q, rq) and np.array_equal(t, rt) and np.array_equal(d, rd), case
        if ref.available():
            fq, ft, fd = ref.match_knn(a, b, ratio)
            assert np.array_equal(q, fq) and np.array_equal(t, ft) and np.array_equal(d, fd), case + " vs reference matchKNN"
        q, t, d = fe.match_crosscheck(a, b)
        rq, rt, rd = orc.match_crosscheck(a, b)
        assert np.array_equal(q, rq) and np.array_equal(t, rt) and np.array_equal(d, rd), case
    extra, scans = fe.match_fallback_rows(full=True)
    assert extra > 0, "the saturated rows of %s were not re-ranked beyond two candidates" % case
    if "all_equal" in case or case == "twenty_identical_train_rows":
        assert scans > 0, "more than sixteen rows within round-off (%s): the exact scan must have run" % case
    fe.close()


def test_match_random_shapes_with_injected_duplicates(api, orc):
    """40 seeded random problems (1..600 rows per side, dim 32..256, ratio 0.6..1.2, with and without a radius gate; copies, near-copies at 1e-7 and
    groups of up to 12 identical rows injected on both sides): matchKNN and the cross-check matcher bitwise against the oracle every time."""
    fe = _fe(api, 64, 64, 1, api.PREC_F32)
    rng = np.random.RandomState(2026)
    for it in range(40):
        na, nb = int(rng.randint(1, 601)), int(rng.randint(1, 601))
        dim = int(rng.choice([32, 64, 128, 256]))
        a = _unit(rng.randn(na, dim)); b = _unit(rng.randn(nb, dim))
        k = min(na, nb) // 2
        if k:                                   # shared content so that matches exist
            b[:k] = _unit(a[rng.permutation(na)[:k]] + 0.08 * rng.randn(k, dim))
        for side in (a, b):                      # degenerate structure
            n = len(side)
            if n >= 4 and rng.rand() < 0.7:
                g = int(rng.randint(2, min(n, 13)))
                side[rng.choice(n, g, replace=False)] = side[int(rng.randint(0, n))]
            if n >= 4 and rng.rand() < 0.5:
                i, j = rng.choice(n, 2, replace=False)
                side[i] = (side[j] + np.float32(1e-7) * rng.randn(dim)).astype(np.float32)
        ratio = float(rng.uniform(0.6, 1.2))
        pa = (rng.rand(na, 2) * 640).astype(np.float32); pb = (rng.rand(nb, 2) * 640).astype(np.float32)
        radius = float(rng.choice([-1.0, 80.0, 300.0]))
        q, t, d = fe.match_knn(a, b, ratio, pa, pb, radius)
        rq, rt, rd = orc.match_knn(a, b, ratio, pa, pb, radius)
        assert np.array_equal(q, rq) and np.array_equal(t, rt) and np.array_equal(d, rd), (it, na, nb, dim, ratio, radius)
        q, t, d = fe.match_crosscheck(a, b)
        rq, rt, rd = orc.match_crosscheck(a, b)
        assert np.array_equal(q, rq) and np.array_equal(t, rt) and np.array_equal(d, rd), (it, na, nb, dim)
    fe.close()


def test_match_fallback_is_rare_on_ordinary_descriptors(api, orc):
    """The fallback is a safety net: on well-separated descriptor sets only a few queries may need it."""
    fe = _fe(api, 64, 64, 1, api.PREC_F32)
    fe.match_fallback_rows(reset=True)
    a, b, _, _ = synth_descriptor_pair(200, 200, 256, seed=5)
    q, t, d = fe.match_knn(a, b, 0.8)
    rq, rt, rd = orc.match_knn(a, b, 0.8)
    assert np.array_equal(q, rq) and np.array_equal(t, rt) and np.array_equal(d, rd)
    past4, scans = fe.match_fallback_rows(full=True)
    assert past4 <= 40 and scans == 0               # of 400 queries
    fe.close()


def test_match_batch_device_equals_host_calls(api, orc):
    """The batched device-resident entry point (what bench.py times) == per-pair host calls == oracle."""
    torch = pytest.importorskip("torch")
    fe = _fe(api, 64, 64, 1, api.PREC_F32)
    dev = torch.device("cuda", 0)
    cap, npairs = 200, 6
    rng = np.random.RandomState(0)
    pool = np.zeros((2 * npairs, cap, 256), np.float32); cnts = np.zeros(2 * npairs, np.int32)
    refs = []
    for p in range(npairs):
        na, nb = int(rng.randint(1, cap + 1)), int(rng.randint(1, cap + 1))
        a, b, _, _ = synth_descriptor_pair(na, nb, 256, seed=100 + p)
        pool[2 * p, :na] = a; pool[2 * p + 1, :nb] = b; cnts[2 * p] = na; cnts[2 * p + 1] = nb
        refs.append(orc.match_knn(a, b, 0.8))
    d_pool = torch.from_numpy(pool).to(dev); d_cnt = torch.from_numpy(cnts).to(dev)
    a_off = torch.arange(0, 2 * npairs, 2, dtype=torch.int32, device=dev) * cap
    b_off = a_off + cap
    a_cnt = d_cnt[0::2].contiguous(); b_cnt = d_cnt[1::2].contiguous()
    q = torch.zeros((npairs, cap), dtype=torch.int32, device=dev); t = torch.zeros_like(q)
    d = torch.zeros((npairs, cap), dtype=torch.float32, device=dev); n = torch.zeros(npairs, dtype=torch.int32, device=dev)
    fe.match_batch_device(d_pool.data_ptr(), d_pool.data_ptr(), a_off.data_ptr(), b_off.data_ptr(), a_cnt.data_ptr(),
                          b_cnt.data_ptr(), npairs, 256, cap, q.data_ptr(), t.data_ptr(), d.data_ptr(), n.data_ptr(),
                          stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for p in range(npairs):
        k = int(n[p])
        rq, rt, rd = refs[p]
        assert k == len(rq)
        assert np.array_equal(q[p, :k].cpu().numpy(), rq) and np.array_equal(t[p, :k].cpu().numpy(), rt)
        assert np.array_equal(d[p, :k].cpu().numpy(), rd)
    fe.close()


def test_extract_device_equals_host_api(api, sp_weights):
    torch = pytest.importorskip("torch")
    H, W, n, cap = 96, 128, 4, 100
    imgs = np.stack([synth_image(H, W, 30 + s) for s in range(n)])
    fe = _fe(api, H, W, n, api.PREC_F32, max_kp=cap)
    fe.load_superpoint(sp_weights)
    host = fe.extract_batch(imgs, cap=cap)
    dev = torch.device("cuda", 0)
    d_img = torch.from_numpy(imgs).to(dev)
    kps = torch.zeros((n, cap, 2), device=dev); sc = torch.zeros((n, cap), device=dev); desc = torch.zeros((n, cap, 256), device=dev)
    idx = torch.zeros((n, cap), dtype=torch.int32, device=dev); cnt = torch.zeros(n, dtype=torch.int32, device=dev)
    fe.extract_device(d_img.data_ptr(), n, W, H, kps.data_ptr(), sc.data_ptr(), desc.data_ptr(), idx.data_ptr(), cap, cnt.data_ptr(),
                      stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for i in range(n):
        k = int(cnt[i])
        assert k == len(host[i][0])
        assert np.array_equal(kps[i, :k].cpu().numpy(), host[i][0]) and np.array_equal(desc[i, :k].cpu().numpy(), host[i][2])
        assert np.array_equal(idx[i, :k].cpu().numpy(), (host[i][0][:, 1] * W + host[i][0][:, 0]).astype(np.int32))
    fe.close()


def test_error_behaviour(api, sp_weights):
    fe = _fe(api, 96, 128, 1, api.PREC_F32)
    with pytest.raises(api.D2FEError):            # weights not loaded (reference: infer() -> false)
        fe.extract_batch(np.zeros((1, 96, 128), np.uint8))
    fe.load_superpoint(sp_weights)
    with pytest.raises(api.D2FEError):            # size not a multiple of 8 / larger than configured
        fe.extract_batch(np.zeros((1, 100, 128), np.uint8))
    with pytest.raises(api.D2FEError):
        fe.extract_batch(np.zeros((2, 96, 128), np.uint8))   # batch > max_batch
    fe.close()
    sp = api.SuperPoint(api.SuperPointConfig(input_width=128, input_height=96, max_keypoints=50), weights=sp_weights)
    assert sp.build() is True
    ok, k, d, s = sp.infer(synth_image(96, 128, 1))
    assert ok and k.shape == (50, 2) and d.shape == (50 * 256,) and s.shape == (50,)


@pytest.mark.parametrize("H,W,d,maxkp", [(96, 128, 4, 100), (120, 160, 10, 150), (480, 640, 10, 200)])
def test_variant_a_nms2_exact(api, orc, sp_weights, H, W, d, maxkp):
    """Variant A (SuperPointONNX path): getKeyPoints + NMS2 + grid_sampler sampling; indices exact vs the sequential oracle."""
    img = synth_image(H, W, 77)
    fe = api.DevFrontEnd(api.SuperPointConfig(max_keypoints=maxkp, input_width=W, input_height=H, max_batch=1,
                                           postproc=api.POSTPROC_A, nms_dist=d, keep_score_map=True))
    fe.load_superpoint(sp_weights)
    (kps, sc, desc), = fe.extract_batch(img[None], cap=maxkp)
    f = orc.superpoint_forward(img, sp_weights)
    assert np.array_equal(fe.debug_read("semi", (1, H, W))[0], f["semi"])
    rk, rs = orc.nms2_a(f["semi"], 0.015, d, maxkp)
    assert len(rk) > 10
    assert np.array_equal(kps, rk) and np.array_equal(sc, rs)
    rd = orc.sample_a(f["desc"], rk, W, H)
    assert desc.shape == rd.shape and np.abs(desc - rd).max() <= 1e-6
    # PCA branch (superpoint_common.cpp:76-85): 64-D
    rng = np.random.RandomState(0)
    comp = np.linalg.qr(rng.randn(256, 64))[0].T.astype(np.float32); mean = (rng.randn(256) * 0.01).astype(np.float32)
    fe.set_pca(comp, mean)
    assert fe.desc_dim == 64
    (kps2, sc2, desc2), = fe.extract_batch(img[None], cap=maxkp)
    assert np.array_equal(kps2, rk) and desc2.shape == (len(rk), 64)
    assert np.abs(desc2 - orc.sample_a(f["desc"], rk, W, H, comp, mean)).max() <= 1e-5
    fe.close()


def test_variant_a_u16_index_wrap(api, orc, sp_weights):
    """NMS2's index map is CV_16UC1 (superpoint_common.cpp:115,128): above 65 536 candidates a survivor of raster rank r is
    reported at the coordinates of candidate r mod 65536 (:160-163).  Oracle and device both reproduce it."""
    H, W = 256, 320                                         # 81 920 pixels
    img = synth_image(H, W, 5)
    fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=400, input_width=W, input_height=H, max_batch=1,
                                           postproc=api.POSTPROC_A, nms_dist=3, keypoint_threshold=1e-6, keep_score_map=True))
    fe.load_superpoint(sp_weights)
    (kps, sc, desc), = fe.extract_batch(img[None], cap=400)
    f = orc.superpoint_forward(img, sp_weights)
    assert int((f["semi"] > 1e-6).sum()) > 70000            # the wrap really happens
    rk, rs = orc.nms2_a(f["semi"], 1e-6, 3, 400)
    assert np.array_equal(kps, rk) and np.array_equal(sc, rs)
    # ... and it does move points: the score at the reported location is not the reported score for the wrapped ones
    moved = sum(1 for (x, y), s in zip(rk.astype(int), rs) if f["semi"][y, x] != s)
    assert moved > 0
    rd = orc.sample_a(f["desc"], rk, W, H)
    assert np.abs(desc - rd).max() <= 1e-6
    fe.close()


def test_variant_a_raster_dependence(api, orc, sp_weights):
    """NMS2 is raster-order dependent: the device fixpoint must reproduce the sequential sweep on a crafted
    score map.  Uses the NMS kernel through a frontend whose score map is replaced is not possible from outside, so this
    checks a flat image instead: every interior cell identical -> dense exact ties, which NMS2 never suppresses (strict <)."""
    img = np.full((96, 128), 90, np.uint8)
    fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=300, input_width=128, input_height=96, max_batch=1,
                                           postproc=api.POSTPROC_A, nms_dist=4, keypoint_threshold=0.001))
    fe.load_superpoint(sp_weights)
    (kps, sc, desc), = fe.extract_batch(img[None], cap=300)
    f = orc.superpoint_forward(img, sp_weights)
    rk, rs = orc.nms2_a(f["semi"], 0.001, 4, 300)
    assert np.array_equal(kps, rk) and np.array_equal(sc, rs)
    fe.close()


@pytest.mark.parametrize("H,W", [(96, 128), (480, 640), (400, 800)])
def test_netvlad_vs_oracle(api, orc, H, W):
    """A9: global descriptor (stand-in graph; parity unpinned).  HIP vs the oracle on the same layer list: <= 1e-4."""
    from d2slam_amd import netvlad as nvm
    nv = nvm.synthetic_netvlad_weights()
    imgs = np.stack([synth_image(H, W, 5 + s) for s in range(2)])
    fe = api.FrontEnd(api.SuperPointConfig(input_width=W, input_height=H, max_batch=2))
    fe.load_netvlad(nv)
    assert fe.netvlad_dim == 4096
    got = fe.netvlad(imgs)
    for i in range(2):
        ref = orc.netvlad_forward(imgs[i], nv)
        assert abs(np.linalg.norm(got[i]) - 1.0) < 1e-5          # loop_tensorrt_test.cpp:97-100 prints this norm
        assert np.abs(got[i] - ref).max() <= 1e-4, np.abs(got[i] - ref).max()
    # PCA branch: y = comp (x - mean), y/|y|  (mobilenetvlad_onnx.h:66-71), 4096 -> 1024 (netvlad_pca_dims, d435_single.yaml:118)
    comp, mean = nvm.synthetic_netvlad_pca(1024)
    fe.set_netvlad_pca(comp, mean)
    assert fe.netvlad_dim == 1024
    got2 = fe.netvlad(imgs)
    ref2 = orc.netvlad_forward(imgs[0], nv, pca=(comp, mean))
    assert np.abs(got2[0] - ref2).max() <= 1e-4
    fe.close()


@pytest.mark.parametrize("mult,H,W", [(0.35, 96, 128), (0.35, 480, 640), (0.5, 128, 160), (0.75, 128, 160), (1.0, 96, 128)])
def test_netvlad_other_trunk_widths(api, orc, mult, H, W):
    """The real mobilenetvlad_dyn_size.onnx is not in the reference tree, so its width is not known: the loader takes ANY MobileNetV2-style layer list
    (d2fe_load_netvlad).  The specialised block kernels cover the channel counts of depth multipliers 0.75 (SURVEY A9's, the default: test_netvlad_vs_oracle) and
    0.35 (rounds 2-5); other widths (Cin 64, 96, 160 ...) fall back to the generic fused block / per-layer kernels where no specialised shape exists.
    Against the oracle <= 1e-4, and the same bits alone and in a batch."""
    from d2slam_amd import netvlad as nvm
    nv = nvm.synthetic_netvlad_weights(seed=77, depth_multiplier=mult)
    imgs = np.stack([synth_image(H, W, 21 + s) for s in range(3)])
    fe = api.FrontEnd(api.SuperPointConfig(input_width=W, input_height=H, max_batch=3))
    fe.load_netvlad(nv)
    got = fe.netvlad(imgs)
    for i in range(3):
        ref = orc.netvlad_forward(imgs[i], nv)
        assert abs(np.linalg.norm(got[i]) - 1.0) < 1e-5
        assert np.abs(got[i] - ref).max() <= 1e-4, (mult, np.abs(got[i] - ref).max())
        np.testing.assert_array_equal(fe.netvlad(imgs[i:i + 1])[0], got[i])
    # a shape outside the documented limits (first convolution wider than 32 channels: MobileNetV2-1.4) is refused with a message, and the handle stays usable
    with pytest.raises(api.D2FEError, match="conv layer must be first"):
        fe.load_netvlad(nvm.synthetic_netvlad_weights(seed=78, depth_multiplier=1.4))
    fe.load_netvlad(nv)
    np.testing.assert_array_equal(fe.netvlad(imgs), got)
    fe.close()


@pytest.mark.parametrize("K,D", [(16, 64), (24, 96), (64, 128)])
def test_netvlad_general_head_is_reproducible(api, orc, K, D):
    """Heads other than 32 x 128 take nv_vlad_partial_kernel / nv_vlad_final_kernel (netvlad.hip): against the oracle, and every sum in a fixed order --
    the same bits run to run, alone and in a batch (the final kernel used to sum with multi-addend LDS float atomics)."""
    from d2slam_amd import netvlad as nvm
    H, W = 240, 320
    nv = nvm.synthetic_netvlad_weights()
    rng = np.random.RandomState(K * 1000 + D)
    hd = dict(nv["head"])
    feat = hd["pre_w"].shape[1]
    bound = np.sqrt(3.0 / feat)
    hd["pre_w"] = rng.uniform(-bound, bound, size=(D, feat)).astype(np.float32); hd["pre_b"] = rng.uniform(-0.05, 0.05, size=(D,)).astype(np.float32)
    hd["assign_w"] = rng.normal(0, 1.0 / np.sqrt(D), size=(K, D)).astype(np.float32); hd["assign_b"] = rng.uniform(-0.1, 0.1, size=(K,)).astype(np.float32)
    hd["centroids"] = rng.normal(0, 0.3, size=(K, D)).astype(np.float32)
    nv = dict(nv); nv["head"] = hd
    imgs = np.stack([synth_image(H, W, 11 + s) for s in range(3)])
    fe = api.FrontEnd(api.SuperPointConfig(input_width=W, input_height=H, max_batch=3))
    fe.load_netvlad(nv)
    assert fe.netvlad_dim == K * D
    got = fe.netvlad(imgs)
    for i in range(3):
        ref = orc.netvlad_forward(imgs[i], nv)
        assert np.abs(got[i] - ref).max() <= 1e-4, np.abs(got[i] - ref).max()
    for _ in range(5):
        np.testing.assert_array_equal(fe.netvlad(imgs), got)
    for i in range(3):
        np.testing.assert_array_equal(fe.netvlad(imgs[i:i + 1])[0], got[i])
    fe.close()


@pytest.mark.parametrize("H,W", [(96, 128), (120, 200), (480, 640)])
def test_netvlad_fused_blocks_layerwise(api, orc, H, W):
    """Every tensor the fused MobileNetV2 block kernels (netvlad_fused.hip) write to HBM -- the last layer of each block -- against
    the oracle's layer outputs: catches a wrong block long before the 4096-D descriptor would.  Sizes include a width that is not a
    multiple of the 16-pixel tile and odd intermediate sizes (TF SAME padding with pad_begin = 1 on stride-2 layers)."""
    from d2slam_amd import netvlad as nvm
    nv = nvm.synthetic_netvlad_weights()
    imgs = np.stack([synth_image(H, W, 9 + s) for s in range(2)])
    fe = api.DevFrontEnd(api.SuperPointConfig(input_width=W, input_height=H, max_batch=2))
    fe.load_netvlad(nv)
    got = fe.netvlad(imgs)
    fused = 0
    refs = [orc.netvlad_forward(imgs[i], nv, return_layers=True) for i in range(2)]
    for li, l in enumerate(nv["layers"]):
        shp = (2,) + refs[0][1][li].shape
        g = fe.debug_netvlad_layer(li, shp)
        if g is None:
            fused += 1
            continue
        for i in range(2):
            r = refs[i][1][li]
            err = np.abs(g[i] - r).max()
            assert err <= 2e-5 * max(1.0, np.abs(r).max()), (li, l["kind"], err)
    assert fused >= 30, "the fused block plan is not the one that ran (%d layers inside blocks)" % fused
    for i in range(2):
        assert np.abs(got[i] - refs[i][0]).max() <= 1e-4
    fe.close()


@pytest.mark.parametrize("env", [{"D2FE_NV_FRONT_TPW": "3"}, {"D2FE_NV_FRONT_TPW": "4", "D2FE_NV_NBUF": "1"}, {"D2FE_NV_NBUF": "2"}])
def test_netvlad_pair_kernel_variants(api, orc, monkeypatch, env):
    """Launch variants of the pixel-pair kernels (netvlad_pair.hip) that the default heuristics only pick at large batches: the first block
    walking 3 / 4 tiles per workgroup with the next tile's bytes in flight (tile counts that are not multiples of either), one / two E
    buffers in the stride-1 blocks.  Same arithmetic, same bits as the default plan; every block output within 2e-5 of the oracle."""
    from d2slam_amd import netvlad as nvm
    nv = nvm.synthetic_netvlad_weights()
    H, W = 200, 328                       # first block: 100 x 164 outputs -> tile counts not divisible by 3 or 4, odd sizes further down
    imgs = np.stack([synth_image(H, W, 70 + s) for s in range(2)])
    for k in ("D2FE_NV_FRONT_TPW", "D2FE_NV_NBUF"):
        monkeypatch.delenv(k, raising=False)
    fe0 = api.DevFrontEnd(api.SuperPointConfig(input_width=W, input_height=H, max_batch=2))
    fe0.load_netvlad(nv)
    base = fe0.netvlad(imgs)
    fe0.close()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    fe = api.DevFrontEnd(api.SuperPointConfig(input_width=W, input_height=H, max_batch=2))
    fe.load_netvlad(nv)
    api.DevFrontEnd.regime_reset()
    got = fe.netvlad(imgs)
    if "D2FE_NV_FRONT_TPW" in env:      # the launch-regime record (include/d2fe_debug.h): the forced variant is the one that ran
        assert api.DevFrontEnd.regime_counts()["nv_front_tpw"] >= 1
    assert np.array_equal(got, base), np.abs(got - base).max()
    refs = [orc.netvlad_forward(imgs[i], nv, return_layers=True) for i in range(2)]
    for li in range(len(nv["layers"])):
        g = fe.debug_netvlad_layer(li, (2,) + refs[0][1][li].shape)
        if g is None:
            continue
        for i in range(2):
            r = refs[i][1][li]
            assert np.abs(g[i] - r).max() <= 2e-5 * max(1.0, np.abs(r).max()), (li, env)
    fe.close()


def test_netvlad_phase_stamps_hook(api, monkeypatch):
    """D2FE_NV_STAMP_STEP: the block kernel of that execution-plan step writes wall_clock64() stamps per workgroup (tools/nv_stamps.py);
    they are monotonic per workgroup and the call's result does not change."""
    from d2slam_amd import netvlad as nvm
    nv = nvm.synthetic_netvlad_weights()
    H, W = 240, 320
    imgs = np.stack([synth_image(H, W, 80 + s) for s in range(2)])
    monkeypatch.delenv("D2FE_NV_STAMP_STEP", raising=False)
    fe0 = api.DevFrontEnd(api.SuperPointConfig(input_width=W, input_height=H, max_batch=2))
    fe0.load_netvlad(nv)
    base = fe0.netvlad(imgs)
    fe0.close()
    for step in (0, 2):
        monkeypatch.setenv("D2FE_NV_STAMP_STEP", str(step))
        fe = api.DevFrontEnd(api.SuperPointConfig(input_width=W, input_height=H, max_batch=2))
        fe.load_netvlad(nv)
        got = fe.netvlad(imgs)
        assert np.array_equal(got, base)
        st = fe.debug_netvlad_stamps().astype(np.int64)
        assert len(st) > 0
        st = st[st.any(axis=1)]              # (a multi-tile first block launches fewer workgroups than it has tiles)
        assert len(st) > 0
        for row in st:
            t = row[row > 0]
            assert len(t) >= 5 and np.all(np.diff(t) >= 0), (step, row[:12])
        fe.close()


def test_netvlad_plans_agree(api, orc, monkeypatch):
    """The fused plan (default), the per-pixel form of the stride-1 blocks (D2FE_NV_PAIR=0), the LDS-resident block form (D2FE_NV_XBLOCK=0), no slab sums (D2FE_NV_SLABSUM=0) and one launch per
    layer (D2FE_NV_LEGACY=1) are five schedules of the same arithmetic up to summation order: all within 1e-4 of the oracle, and a batch
    of one image equals the same image inside a batch of five (different group counts, hence different slab layouts)."""
    from d2slam_amd import netvlad as nvm
    nv = nvm.synthetic_netvlad_weights()
    H, W = 240, 320
    imgs = np.stack([synth_image(H, W, 30 + s) for s in range(5)])
    ref = orc.netvlad_forward(imgs[2], nv)
    for env in ({}, {"D2FE_NV_PAIR": "0"}, {"D2FE_NV_XBLOCK": "0"}, {"D2FE_NV_SLABSUM": "0"}, {"D2FE_NV_LEGACY": "1"}):
        for k in ("D2FE_NV_PAIR", "D2FE_NV_XBLOCK", "D2FE_NV_SLABSUM", "D2FE_NV_LEGACY"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        fe = api.DevFrontEnd(api.SuperPointConfig(input_width=W, input_height=H, max_batch=5))
        fe.load_netvlad(nv)
        got5 = fe.netvlad(imgs)
        got1 = fe.netvlad(imgs[2:3])
        assert np.abs(got5[2] - ref).max() <= 1e-4, env
        assert np.abs(got1[0] - ref).max() <= 1e-4, env
        assert np.abs(got1[0] - got5[2]).max() <= 2e-6, env
        fe.close()


def test_stride_cap_and_batch_invariance(api, orc, sp_weights):
    """Row stride > width (cv::Mat ROI), cap < max_keypoints, and batch-position independence (an image's result must not
    depend on its neighbours in the batch or on the batch size)."""
    H, W = 96, 128
    imgs = np.stack([synth_image(H, W, 50 + s) for s in range(3)])
    fe = _fe(api, H, W, 3, api.PREC_F32, max_kp=120)
    fe.load_superpoint(sp_weights)
    ref = fe.extract_batch(imgs, cap=120)
    single = [fe.extract_batch(imgs[i:i + 1], cap=120)[0] for i in range(3)]
    rev = fe.extract_batch(imgs[::-1].copy(), cap=120)[::-1]
    for i in range(3):
        for other in (single[i], rev[i]):
            assert all(np.array_equal(a, b) for a, b in zip(ref[i], other))
    # strided input through the raw C ABI
    import ctypes as C
    lib = api.load_library()
    stride = W + 40
    buf = np.zeros((H, stride), np.uint8); buf[:, :W] = imgs[0]; buf[:, W:] = 255
    kps = np.zeros((120, 2), np.float32); sc = np.zeros(120, np.float32); desc = np.zeros((120, 256), np.float32); n = C.c_int(0)
    rc = lib.d2fe_superpoint_extract(fe.handle, buf.ctypes.data, W, H, stride, kps.ctypes.data, sc.ctypes.data, desc.ctypes.data, 120, C.byref(n))
    assert rc == 0 and n.value == len(ref[0][0])
    assert np.array_equal(kps[:n.value], ref[0][0]) and np.array_equal(desc[:n.value], ref[0][2])
    # cap smaller than max_keypoints: the first `cap` of the same ordered list
    small = fe.extract_batch(imgs[:1], cap=40)[0]
    assert len(small[0]) == 40 and np.array_equal(small[0], ref[0][0][:40]) and np.array_equal(small[1], ref[0][1][:40])
    fe.close()


def test_sliding_window_batch(api, orc):
    """One new frame against an 11-keyframe sliding window (max_sld_win_size, README.md:116) in ONE batched launch."""
    torch = pytest.importorskip("torch")
    fe = _fe(api, 64, 64, 1, api.PREC_F32)
    dev = torch.device("cuda", 0)
    cap, nwin = 200, 11
    pool = np.zeros((nwin + 1, cap, 256), np.float32); cnt = np.zeros(nwin + 1, np.int32)
    base, _, _, _ = synth_descriptor_pair(200, 200, 256, seed=1)
    pool[0] = base; cnt[0] = 200
    rng = np.random.RandomState(2)
    for k in range(1, nwin + 1):
        n = int(rng.randint(120, 201))
        d = base[rng.permutation(200)[:n]] + rng.normal(0, 0.03 * k, size=(n, 256)).astype(np.float32)
        pool[k, :n] = d / np.linalg.norm(d, axis=1, keepdims=True); cnt[k] = n
    dp = torch.from_numpy(pool).to(dev); dc = torch.from_numpy(cnt).to(dev)
    a_off = torch.zeros(nwin, dtype=torch.int32, device=dev); b_off = (torch.arange(1, nwin + 1, dtype=torch.int32, device=dev) * cap)
    a_cnt = dc[:1].repeat(nwin).contiguous(); b_cnt = dc[1:].contiguous()
    q = torch.zeros((nwin, cap), dtype=torch.int32, device=dev); t = torch.zeros_like(q)
    d = torch.zeros((nwin, cap), dtype=torch.float32, device=dev); n = torch.zeros(nwin, dtype=torch.int32, device=dev)
    fe.match_batch_device(dp.data_ptr(), dp.data_ptr(), a_off.data_ptr(), b_off.data_ptr(), a_cnt.data_ptr(), b_cnt.data_ptr(), nwin, 256,
                          cap, q.data_ptr(), t.data_ptr(), d.data_ptr(), n.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for k in range(nwin):
        rq, rt, rd = orc.match_knn(pool[0, :200], pool[k + 1, :cnt[k + 1]], 0.8)
        m = int(n[k])
        assert m == len(rq) and np.array_equal(q[k, :m].cpu().numpy(), rq) and np.array_equal(t[k, :m].cpu().numpy(), rt)
        assert np.array_equal(d[k, :m].cpu().numpy(), rd)
    fe.close()


def test_exact_mode_many_full_size_frames(api, orc, sp_weights):
    """Statistical weight behind 'indices exact': 8 more 640x480 frames and 4 quadcam-sized 800x400 views, all keypoints,
    scores and match sets identical to the oracle."""
    for (H, W, n, seed0) in ((480, 640, 8, 100), (400, 800, 4, 200)):
        imgs = np.stack([synth_image(H, W, seed0 + s) for s in range(n)])
        fe = _fe(api, H, W, n, api.PREC_F32)
        fe.load_superpoint(sp_weights)
        res = fe.extract_batch(imgs, cap=200)
        descs = []
        for i in range(n):
            rk, rs, rd, ri, f = orc.extract_b(imgs[i], sp_weights, 0.015, 1, 200)
            assert np.array_equal(res[i][0], rk) and np.array_equal(res[i][1], rs), "frame %d" % i
            assert np.abs(res[i][2] - rd).max() <= 1e-6
            descs.append(rd)
        for i in range(0, n - 1, 2):
            q, t, d = fe.match_knn(res[i][2], res[i + 1][2], 0.8)
            rq, rt, rdist = orc.match_knn(res[i][2], res[i + 1][2], 0.8)
            assert np.array_equal(q, rq) and np.array_equal(t, rt) and np.array_equal(d, rdist)
        fe.close()


def test_matcher_fuzz(api, orc):
    """60 random problems (sizes 1..300, dims 32..256, ratios, radii, duplicated rows): indices and distances bit-exact."""
    fe = _fe(api, 64, 64, 1, api.PREC_F32)
    rng = np.random.RandomState(123)
    for case in range(60):
        na, nb = int(rng.randint(1, 301)), int(rng.randint(1, 301))
        dim = int(rng.choice([32, 64, 128, 256]))
        ratio = float(rng.choice([0.7, 0.8, 0.9, 0.95]))
        radius = float(rng.choice([-1.0, 20.0, 60.0]))
        a, b, pa, pb = synth_descriptor_pair(na, nb, dim, seed=1000 + case, sigma=float(rng.choice([0.02, 0.1, 0.3])))
        if case % 5 == 0 and nb > 4:
            b[nb // 2] = b[0]; b[nb - 1] = b[1]          # exact duplicates -> distance ties
        q, t, d = fe.match_knn(a, b, ratio, pa, pb, radius)
        rq, rt, rd = orc.match_knn(a, b, ratio, pa, pb, radius)
        assert np.array_equal(q, rq) and np.array_equal(t, rt) and np.array_equal(d, rd), (case, na, nb, dim)
        if case % 3 == 0:
            q, t, d = fe.match_crosscheck(a, b)
            rq, rt, rd = orc.match_crosscheck(a, b)
            assert np.array_equal(q, rq) and np.array_equal(t, rt) and np.array_equal(d, rd), (case, na, nb, dim)
    fe.close()


@pytest.mark.parametrize("H,W,maxkp,thr", [(512, 512, 150, 0.015),      # C1: TUM 512x512 (config/tum/tum_single.yaml:20-21)
                                           (400, 800, 100, 0.015),      # C3: one undistorted quadcam view, 100 keypoints
                                           (480, 640, 1024, 0.015),     # the former limit of the ABI
                                           (480, 640, 3000, 0.015),     # above it: 4096-key in-LDS sort (TensorRT profile 1500 x 1500, thousands of points)
                                           (240, 320, 16384, 0.002),    # the largest sorted budget the ABI accepts (25 611 candidates)
                                           (480, 640, 200, 0.9999)])    # a threshold nothing passes: zero keypoints, no failure
def test_other_configs_and_limits(api, orc, sp_weights, H, W, maxkp, thr):
    img = synth_image(H, W, 91)
    fe = _fe(api, H, W, 1, api.PREC_F32, max_kp=maxkp, thr=thr)
    fe.load_superpoint(sp_weights)
    kps, sc, desc = fe.extract_batch(img[None], cap=maxkp)[0][:3]
    rk, rs, rd, ri, f = orc.extract_b(img, sp_weights, thr, 1, maxkp)
    assert len(kps) == len(rk) and (thr < 0.9 or len(kps) == 0) and (thr > 0.9 or len(kps) == maxkp), (len(kps), len(rk))
    assert np.array_equal(kps, rk) and np.array_equal(sc, rs)
    if len(kps):
        assert np.abs(desc - rd).max() <= 1e-6
    fe.close()


def test_host_calls_replay_cached_graphs_with_identical_results(api, orc, sp_weights):
    """The host-pointer extract / NetVLAD calls capture their launch sequence into a hipGraph on the second call of a geometry and replay it
    afterwards (one pinned DMA in, one out): results of the plain, the capturing and the replayed calls are identical bit for bit, for two
    geometries on one handle, and a weight reload drops the graphs."""
    from d2slam_amd import netvlad as nvm
    if os.environ.get("D2FE_GRAPH", "1") == "0":
        pytest.skip("graphs switched off")
    H, W = 120, 160
    fe = _fe_dev(api, H, W, 2, api.PREC_F32_WINO, max_kp=100)
    fe.load_superpoint(sp_weights); fe.load_netvlad(nvm.synthetic_netvlad_weights())
    a = np.stack(synth_stereo(H, W, seed=5)); b = np.stack(synth_stereo(H, W, seed=6))
    outs = [fe.extract_batch(a, cap=100) for _ in range(4)]          # plain, capture, replay, replay
    for o in outs[1:]:
        for (k0, s0, d0), (k1, s1, d1) in zip(outs[0], o):
            assert np.array_equal(k0, k1) and np.array_equal(s0, s1) and np.array_equal(d0, d1)
    rk, rs, rd, _, _ = orc.extract_b(a[0], sp_weights, 0.015, 1, 100, wino=True)
    assert np.array_equal(outs[3][0][0], rk) and np.array_equal(outs[3][0][1], rs)
    ob = [fe.extract_batch(b[:1], cap=100) for _ in range(3)]         # another geometry (1 image) on the same handle, other frames
    rk, rs, rd, _, _ = orc.extract_b(b[0], sp_weights, 0.015, 1, 100, wino=True)
    assert np.array_equal(ob[2][0][0], rk) and np.array_equal(ob[2][0][1], rs) and np.abs(ob[2][0][2] - rd).max() <= 1e-6
    g = [fe.netvlad(a) for _ in range(3)]
    assert np.array_equal(g[0], g[1]) and np.array_equal(g[0], g[2])
    n, bad = fe.graph_count()
    assert n == 3 and bad == 0, (n, bad)                               # extract x 2 geometries + netvlad
    fe.load_superpoint(sp_weights)
    assert fe.graph_count()[0] == 0
    again = fe.extract_batch(a, cap=100)
    assert np.array_equal(again[0][2], outs[0][0][2])
    fe.close()


def test_extract_all_equals_the_two_separate_calls(api, sp_weights):
    """d2fe_extract_all(_batch) = SuperPoint::infer + MobileNetVLADONNX::inference of loop_cam.cpp:609-616 from one upload on two streams:
    bit-identical to the separate calls, for one image and for a stereo pair with NetVLAD on the left image only, call after call
    (plain, graph capture, graph replay)."""
    from d2slam_amd import netvlad as nvm
    H, W = 240, 320
    fe = _fe(api, H, W, 2, api.PREC_F32_WINO, max_kp=150)
    fe.load_superpoint(sp_weights); fe.load_netvlad(nvm.synthetic_netvlad_weights())
    pair = np.stack(synth_stereo(H, W, seed=12))
    sep = fe.extract_batch(pair, cap=150); gsep = fe.netvlad(pair[:1])
    for it in range(4):
        outs, g = fe.extract_all_batch(pair, 1, cap=150)
        assert g.shape == (1, fe.netvlad_dim) and np.array_equal(g, gsep), it
        for (k0, s0, d0), (k1, s1, d1) in zip(sep, outs):
            assert np.array_equal(k0, k1) and np.array_equal(s0, s1) and np.array_equal(d0, d1), it
    one = fe.extract_batch(pair[1:], cap=150); gone = fe.netvlad(pair[1:])
    for it in range(3):
        outs, g = fe.extract_all_batch(pair[1:], 1, cap=150)
        assert np.array_equal(g, gone) and np.array_equal(outs[0][0], one[0][0]) and np.array_equal(outs[0][2], one[0][2])
    outs, g = fe.extract_all_batch(pair, 2, cap=150)                 # NetVLAD on both
    assert np.array_equal(g, fe.netvlad(pair))
    with pytest.raises(api.D2FEError):
        fe.extract_all_batch(pair, 3, cap=150)                       # more NetVLAD images than images
    fe.close()


def test_matcher_is_reentrant(api, orc):
    """The reference calls matchKNN from three threads (D2FeatureTracker, LoopDetector, remote tracking).
    Four threads hammer d2fe_match_knn / d2fe_match_crosscheck on one handle (ctypes releases the GIL): every result must equal
    the oracle's, i.e. the (stream, scratch) slots of concurrent calls never overlap."""
    import threading
    fe = api.FrontEnd(api.SuperPointConfig(input_width=64, input_height=64, max_batch=1))
    cases = []
    for t in range(4):
        a, b, pa, pb = synth_descriptor_pair(150 + 10 * t, 120 + 15 * t, 256, seed=40 + t)
        cases.append((a, b, pa, pb, orc.match_knn(a, b, 0.8, pa, pb, 50.0), orc.match_crosscheck(a, b)))
    errors = []

    def work(t):
        a, b, pa, pb, (rq, rt, rd), (cq, ct, cd) = cases[t]
        try:
            for _ in range(40):
                q, tt, d = fe.match_knn(a, b, 0.8, pa, pb, 50.0)
                if not (np.array_equal(q, rq) and np.array_equal(tt, rt) and np.array_equal(d, rd)):
                    errors.append("knn mismatch in thread %d" % t); return
                q, tt, d = fe.match_crosscheck(a, b)
                if not (np.array_equal(q, cq) and np.array_equal(tt, ct) and np.array_equal(d, cd)):
                    errors.append("crosscheck mismatch in thread %d" % t); return
        except Exception as e:   # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    fe.close()


@pytest.mark.parametrize("prec", ["f32", "f16x2"])
def test_sparse_descriptor_head_equals_dense(api, orc, sp_weights, prec):
    """Default mode evaluates convDa/convDb only at the corner cells of the selected keypoints.  Exact mode: the descriptors are
    BIT-identical to the dense-map path (same fmaf chains); fast mode: the sparse head runs in exact fp32 on the fp16x2 trunk,
    so it may only be closer to the oracle than the dense fp16x2 head.  Batch with very different keypoint counts per image,
    incl. an empty image (flat frame: nothing passes the threshold... the dustbin wins everywhere)."""
    H, W = 240, 320
    p = api.PREC_F32 if prec == "f32" else api.PREC_F16X2
    imgs = np.stack([synth_image(H, W, 71), np.full((H, W), 90, np.uint8), synth_image(H, W, 72)] + [synth_image(H, W, 80 + i) for i in range(6)])
    outs = []
    for dense in (False, True):
        fe = _fe_dev(api, H, W, 9, p, max_kp=300, dense=dense)      # 9 images per call: above the sparse path's batch threshold (4)
        fe.load_superpoint(sp_weights)
        outs.append(fe.extract_batch(imgs, cap=300))
        if not dense:
            with pytest.raises(api.D2FEError):
                fe.debug_read("desc_raw", (9, H // 8, W // 8, 256))
        fe.close()
    for i in range(9):
        ks, ss, ds = outs[0][i][:3]
        kd, sd, dd = outs[1][i][:3]
        assert np.array_equal(ks, kd) and np.array_equal(ss, sd)
        if prec == "f32":
            assert np.array_equal(ds.view(np.uint32), dd.view(np.uint32))
        else:
            f = orc.superpoint_forward(imgs[i], sp_weights)
            if len(ks):
                ref = orc.sample_b(f["desc"], ks)
                assert np.abs(ds - ref).max() <= np.abs(dd - ref).max() + 1e-7 and np.abs(ds - ref).max() <= 5e-6
    assert len(outs[0][0][0]) == 300


@pytest.mark.parametrize("prec,n", [("f32", 4), ("wino", 2), ("wino", 3)])
def test_split_sparse_head_of_small_passes_is_bit_identical(api, sp_weights, prec, n):
    """Round 5: passes of <= 4 images run the sparse descriptor head as two launches over twice the workgroups (desc_head_sparse_kernel<1, 4, 1 / 2>: convDa + ReLU
    into a scratch, convDb from it, 128 output channels per workgroup).  Same fmaf chain per output: the descriptors of a frame are the same BITS as in a 9-image
    call, which runs the whole-head kernel with 64 cells per workgroup (and, exact mode, as the dense map's) -- incl. an image without keypoints."""
    H, W = 240, 320
    p = api.PREC_F32 if prec == "f32" else api.PREC_F32_WINO
    imgs = np.stack([synth_image(H, W, 71), np.full((H, W), 90, np.uint8), synth_image(H, W, 72), synth_image(H, W, 73)] + [synth_image(H, W, 80 + i) for i in range(5)])
    fe = _fe_dev(api, H, W, 9, p, max_kp=300, dense=False)
    fe.load_superpoint(sp_weights)
    big = fe.extract_batch(imgs, cap=300)                     # 9 images: desc_head_sparse_kernel<2, 8, 0>
    small = fe.extract_batch(imgs[:n], cap=300)               # n <= 4: the split form
    fe.close()
    for i in range(n):
        assert np.array_equal(small[i][0], big[i][0]) and np.array_equal(small[i][1], big[i][1])
        assert np.array_equal(small[i][2].view(np.uint32), big[i][2].view(np.uint32)), i
    assert len(small[0][0]) == 300 and len(small[1][0]) == 0
    if prec == "f32":
        fd = _fe_dev(api, H, W, 9, p, max_kp=300, dense=True)
        fd.load_superpoint(sp_weights)
        dense = fd.extract_batch(imgs[:n], cap=300)
        fd.close()
        for i in range(n):
            assert np.array_equal(small[i][2].view(np.uint32), dense[i][2].view(np.uint32)), i


@pytest.mark.parametrize("n,wino", [(2, False), (6, False), (6, True)])
def test_async_tail_equals_synchronous(api, sp_weights, n, wino):
    """async_tail: convolutions on the caller's stream, post-processing on the handle's tail stream with double-buffered inputs.
    Five back-to-back calls on different frames WITHOUT any host synchronisation in between (so call k+1's convolutions really
    run while call k's tail is pending), each into its own output buffers, must reproduce the synchronous results bit for bit;
    n = 2 exercises the dense descriptor head, n = 6 the sparse one."""
    torch = pytest.importorskip("torch")
    H, W, cap, calls = 120, 160, 120, 5
    dev = torch.device("cuda", 0)
    frames = [torch.from_numpy(np.stack([synth_image(H, W, 300 + 10 * c + s) for s in range(n)])).to(dev) for c in range(calls)]

    def run(async_tail):
        fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=cap, input_width=W, input_height=H, max_batch=n, async_tail=async_tail,
                                               precision=api.PREC_F32_WINO if wino else api.PREC_F32))
        fe.load_superpoint(sp_weights)
        assert (fe.tail_stream() != 0) == async_tail
        outs = []
        st = torch.cuda.Stream(device=dev)
        for c in range(calls):
            o = dict(kps=torch.zeros((n, cap, 2), device=dev), sc=torch.zeros((n, cap), device=dev), desc=torch.zeros((n, cap, 256), device=dev),
                     idx=torch.zeros((n, cap), dtype=torch.int32, device=dev), cnt=torch.zeros(n, dtype=torch.int32, device=dev))
            outs.append(o)
        torch.cuda.synchronize()
        for c in range(calls):
            o = outs[c]
            fe.extract_device(frames[c].data_ptr(), n, W, H, o["kps"].data_ptr(), o["sc"].data_ptr(), o["desc"].data_ptr(), o["idx"].data_ptr(),
                              cap, o["cnt"].data_ptr(), stream=st.cuda_stream)
        fe.wait_tail(st.cuda_stream)          # st now also waits for the last tail (earlier tails precede it on the tail stream)
        st.synchronize()
        res = [{k: v.cpu().numpy() for k, v in o.items()} for o in outs]
        fe.close()
        return res

    a, b = run(True), run(False)
    for c in range(calls):
        assert a[c]["cnt"].sum() > 0
        for k in ("cnt", "kps", "sc", "desc", "idx"):
            assert np.array_equal(a[c][k], b[c][k]), (c, k)


def test_variant_a_batch_and_pca(api, orc, sp_weights):
    """Variant A on a batch of 3 different frames with the 64-D PCA: every image's keypoints / descriptors equal the oracle's
    (the channel-over-keypoints normalisation of computeDescriptors is per image: batching must not mix the lists)."""
    H, W, maxkp, d = 120, 160, 80, 6
    imgs = np.stack([synth_image(H, W, 200 + s) for s in range(5)])      # 5 images per call: the sparse descriptor head runs
    rng = np.random.RandomState(1)
    comp = np.linalg.qr(rng.randn(256, 64))[0].T.astype(np.float32); mean = (rng.randn(256) * 0.01).astype(np.float32)
    fd = api.FrontEnd(api.SuperPointConfig(max_keypoints=maxkp, input_width=W, input_height=H, max_batch=5, postproc=api.POSTPROC_A, nms_dist=d,
                                           dense_descriptors=True))
    fd.load_superpoint(sp_weights)
    dense = fd.extract_batch(imgs, cap=maxkp)
    fd.close()
    fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=maxkp, input_width=W, input_height=H, max_batch=5, postproc=api.POSTPROC_A, nms_dist=d))
    fe.load_superpoint(sp_weights)
    plain = fe.extract_batch(imgs, cap=maxkp)
    for i in range(5):          # sparse head == dense map path, bit for bit
        assert np.array_equal(plain[i][0], dense[i][0]) and np.array_equal(plain[i][2].view(np.uint32), dense[i][2].view(np.uint32))
    fe.set_pca(comp, mean)
    withpca = fe.extract_batch(imgs, cap=maxkp)
    for i in range(5):
        f = orc.superpoint_forward(imgs[i], sp_weights)
        rk, rs = orc.nms2_a(f["semi"], 0.015, d, maxkp)
        assert len(rk) > 5 and np.array_equal(plain[i][0], rk) and np.array_equal(withpca[i][0], rk) and np.array_equal(plain[i][1], rs)
        assert np.abs(plain[i][2] - orc.sample_a(f["desc"], rk, W, H)).max() <= 1e-6
        assert withpca[i][2].shape == (len(rk), 64)
        assert np.abs(withpca[i][2] - orc.sample_a(f["desc"], rk, W, H, comp, mean)).max() <= 1e-5
    fe.close()


@pytest.mark.parametrize("H,W,n", [(240, 320, 5), (480, 640, 20), (400, 800, 33), (480, 752, 13)])
def test_netvlad_does_not_depend_on_the_batch(api, H, W, n):
    """The split of a block's hidden channels over workgroup groups fixes the fp32 summation order; it is decided per image, so an image's
    descriptor is the same bits alone, in a batch and at any position of it (what lets the frames-in-flight pipe batch frames freely).
    480 x 640, 20 images: the 30 x 40 layers of the batch run with merged groups (NvBlockArgs::gmerge: one workgroup walks a run of three groups), one image's
    launch does not -- the tree-ordered slab sum makes the same bits of it."""
    from d2slam_amd import netvlad as nvm
    from d2slam_amd.synth import synth_image
    fe = api.FrontEnd(api.SuperPointConfig(input_width=W, input_height=H, max_batch=n))
    fe.load_netvlad(nvm.synthetic_netvlad_weights())
    imgs = np.stack([synth_image(H, W, 40 + i) for i in range(n)])
    gn = fe.netvlad(imgs)
    for i in (0, 2, n - 1):
        assert np.array_equal(fe.netvlad(imgs[i:i + 1])[0], gn[i])
    assert np.array_equal(fe.netvlad(imgs[1:4]), gn[1:4])
    fe.close()
