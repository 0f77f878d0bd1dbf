"""The exact_order rule on the host (d2slam_amd/exact_order.py, the restatement of csrc/exact_order.hip): a keypoint list built from Winograd scores plus direct
re-evaluation of the uncertain cells must equal the exact mode's list position by position.  No GPU."""
import numpy as np
import pytest

from d2slam_amd import exact_order as eo
from d2slam_amd.synth import synth_stereo

THR, BORDER = 0.015, 1


@pytest.fixture(scope="module")
def oracle_maps(orc, sp_weights):
    """(Winograd restatement, direct) score maps of a few 160x120 images, computed once"""
    out = []
    for seed in (3, 4, 5):
        img = synth_stereo(120, 160, seed=seed)[seed & 1]
        out.append((orc.superpoint_forward(img, sp_weights, wino=True)["semi"], orc.superpoint_forward(img, sp_weights)["semi"]))
    return out


@pytest.mark.parametrize("K", [50, 200, 100000])
def test_rule_equals_the_direct_list_on_oracle_maps(orc, oracle_maps, K):
    for s_w, s_d in oracle_maps:
        dev = float(np.abs(s_w - s_d).max())
        assert 0 < dev <= 3e-6                                   # the two evaluation orders differ, by what tests/test_wino.py bounds
        rk, rs, ri = orc.select_b(s_d, THR, BORDER, K)           # the oracle's own selection == the host restatement of it
        di, ds = eo.direct_list(s_d, THR, BORDER, K)
        assert np.array_equal(di, ri) and np.array_equal(ds, rs)
        for eps in (dev, eo.DEFAULT_EPS, 1.0):
            r = eo.exact_order_list(s_w, s_d, THR, BORDER, K, eps)
            assert np.array_equal(r["idx"], di)
        full = eo.exact_order_list(s_w, s_d, THR, BORDER, K, 1.0)
        assert np.array_equal(full["scores"], ds)               # eps = 1: every candidate's cell is re-evaluated, the scores are the direct ones too


@pytest.mark.parametrize("H,W", [(96, 104), (88, 88), (480, 640)])
def test_crop_clamp(H, W):
    for cy in range(H // 8):
        for cx in range(W // 8):
            for c8, ext in ((cx, W), (cy, H)):
                o = eo.crop_origin(c8, ext)
                assert o % 8 == 0 and 0 <= o and o + eo.CROP <= ext
                assert o <= 8 * c8 and 8 * c8 + 8 <= o + eo.CROP                     # the cell lies in the crop
                assert 8 * c8 - o >= 40 or o == 0                                    # 40 pixels of margin in front of the cell, or the image edge
                assert o + eo.CROP - (8 * c8 + 8) >= 40 or o + eo.CROP == ext        # and behind it
    if (H, W) == (96, 104):
        assert {eo.crop_origin(c, W) for c in range(13)} == {0, 8, 16} and {eo.crop_origin(c, H) for c in range(12)} == {0, 8}
    if (H, W) == (88, 88):
        assert {eo.crop_origin(c, 88) for c in range(11)} == {0}


def _maps(pix_w, pix_d=None, H=32, W=32):
    """score maps that are zero but for the given {(y, x): score}; the direct map equals the Winograd one where not given"""
    s_w = np.zeros((H, W), np.float32); s_d = np.zeros((H, W), np.float32)
    for (y, x), v in pix_w.items():
        s_w[y, x] = v; s_d[y, x] = v
    for (y, x), v in (pix_d or {}).items():
        s_d[y, x] = v
    return s_w, s_d


def _check(s_w, s_d, K, eps, expect_idx=None, W=32):
    r = eo.exact_order_list(s_w, s_d, THR, BORDER, K, eps)
    di, ds = eo.direct_list(s_d, THR, BORDER, K)
    assert np.array_equal(r["idx"], di), (r["idx"], di)
    if expect_idx is not None:
        assert [int(v) for v in r["idx"]] == [y * W + x for y, x in expect_idx]
    return r


EPS = 1e-3      # large enough that every hand-built value is a float32 far from its neighbours' rounding


def test_pair_straddling_position_k():
    # K = 2; the second and third Winograd scores are 1.5 eps apart and the direct scores put them the other way round
    pw = {(2, 2): 0.5, (10, 3): 0.3, (20, 20): 0.3 - 1.5 * EPS, (27, 5): 0.1}
    pd = {(10, 3): 0.3 - 1.0 * EPS, (20, 20): 0.3 - 0.5 * EPS}
    s_w, s_d = _maps(pw, pd)
    r = _check(s_w, s_d, 2, EPS, [(2, 2), (20, 20)])
    assert r["marked"] == 2 and len(r["cells"]) == 2
    # without the rule the Winograd list keeps the wrong one
    wi, _ = eo.direct_list(s_w, THR, BORDER, 2)
    assert list(wi) == [2 * 32 + 2, 10 * 32 + 3]


def test_chain_of_three_within_two_eps():
    # a, b, c each 1.6 eps from the next (a and c 3.2 eps apart): all three are re-evaluated and the direct scores swap the first two
    pw = {(3, 3): 0.4, (12, 12): 0.4 - 1.6 * EPS, (21, 21): 0.4 - 3.2 * EPS, (28, 28): 0.2, (5, 20): 0.9}
    pd = {(3, 3): 0.4 - 0.9 * EPS, (12, 12): 0.4 - 0.8 * EPS, (21, 21): 0.4 - 2.3 * EPS}
    s_w, s_d = _maps(pw, pd)
    r = _check(s_w, s_d, 3, EPS, [(5, 20), (12, 12), (3, 3)])
    assert r["marked"] == 3
    r4 = _check(s_w, s_d, 4, EPS, [(5, 20), (12, 12), (3, 3), (21, 21)])
    assert r4["marked"] == 3                                     # 0.2 is far from everything


def test_pixel_just_below_the_threshold_whose_direct_score_passes():
    thr = np.float32(THR)
    pw = {(4, 4): 0.5, (9, 17): float(thr - np.float32(EPS / 2)), (20, 6): 0.2}
    pd = {(9, 17): float(thr + np.float32(EPS / 4))}
    s_w, s_d = _maps(pw, pd)
    r = _check(s_w, s_d, 10, EPS, [(4, 4), (9, 17), (20, 6)])    # count <= K: raster order, the recovered pixel in its raster place
    assert r["marked"] == 1 and r["scores"][1] == np.float32(pd[(9, 17)])


def test_pixel_just_above_the_threshold_whose_direct_score_fails_turns_the_list_to_raster_order():
    thr = np.float32(THR)
    # three Winograd candidates, K = 2: sorted top-2.  The weakest fails in the direct chains: two candidates <= K, raster order
    pw = {(25, 25): 0.5, (3, 9): 0.2, (14, 14): float(thr + np.float32(EPS / 2))}
    pd = {(14, 14): float(thr - np.float32(EPS / 4))}
    s_w, s_d = _maps(pw, pd)
    wi, _ = eo.direct_list(s_w, THR, BORDER, 2)
    assert list(wi) == [25 * 32 + 25, 3 * 32 + 9]                # score order without the rule
    _check(s_w, s_d, 2, EPS, [(3, 9), (25, 25)])


def test_exact_ties_fall_back_to_raster_order():
    pw = {(6, 6): 0.3, (2, 30): 0.3, (30, 2): 0.3, (15, 15): 0.3, (20, 20): 0.6}
    s_w, s_d = _maps(pw)
    r = _check(s_w, s_d, 3, EPS, [(20, 20), (2, 30), (6, 6)])
    assert r["marked"] == 4                                      # the four tied candidates (the one at 0.6 is alone)
    _check(s_w, s_d, 3, 0.0, [(20, 20), (2, 30), (6, 6)])      # eps = 0: ties are still marked (gap 0 <= 0) and change nothing


def test_slots_are_granted_in_list_order_and_a_cell_without_one_keeps_its_winograd_score():
    pw = {(3, 3): 0.4, (12, 12): 0.4 - 0.5 * EPS, (21, 21): 0.4 - 1.0 * EPS}
    pd = {(3, 3): 0.39, (12, 12): 0.41, (21, 21): 0.42}
    s_w, s_d = _maps(pw, pd)
    r = eo.exact_order_list(s_w, s_d, THR, BORDER, 2, EPS, slots=1)
    assert list(r["cells"]) == [0, 1 * 4 + 1, 2 * 4 + 2] and r["granted"] == 1
    assert [int(v) for v in r["idx"]] == [12 * 32 + 12, 21 * 32 + 21] and r["scores"][0] == np.float32(0.4 - 0.5 * EPS)     # only (3, 3) moved
    rs, dropped = eo.exact_order_batch([s_w, s_w], [s_d, s_d], THR, BORDER, 2, EPS, slots=4)
    assert dropped == 2 and rs[0]["granted"] == 3 and rs[1]["granted"] == 1


def test_more_keys_than_the_sort_takes_marks_everything(monkeypatch):
    monkeypatch.setattr(eo, "MAXSORT", 3)
    pw = {(3, 3): 0.4, (12, 12): 0.3, (21, 21): 0.2, (28, 28): 0.1}
    s_w, s_d = _maps(pw)
    r = eo.exact_order_list(s_w, s_d, THR, BORDER, 10, EPS)
    assert r["marked"] == 4 and list(r["cells"]) == [0, 5, 10, 15]


def test_threshold_band_is_left_alone_when_more_than_k_candidates_are_clear_of_it():
    thr = np.float32(THR)
    pw = {(3, 3): 0.4, (12, 12): 0.3, (21, 21): 0.2, (28, 28): float(thr + np.float32(EPS / 2)), (5, 25): float(thr - np.float32(EPS / 2))}
    pd = {(28, 28): float(thr - np.float32(EPS / 4)), (5, 25): float(thr + np.float32(EPS / 4))}
    s_w, s_d = _maps(pw, pd)
    r = _check(s_w, s_d, 2, EPS, [(3, 3), (12, 12)])            # three candidates clear of the threshold, K = 2: a sorted top 2 either way
    assert r["marked"] == 0 and len(r["cells"]) == 0
    r = _check(s_w, s_d, 3, EPS, [(3, 3), (12, 12), (21, 21)])      # K = 3: the count's side of K hangs on the band (3 or 4 candidates) -> both are re-evaluated
    assert r["marked"] == 2
