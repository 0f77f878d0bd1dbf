"""The exact_order rule (include/d2fe.h, d2fe_config::exact_order) restated on the host over two score maps: the Winograd mode's and the
direct chains'.  tests/test_exact_order_rule.py holds it to the exact mode's list; d2slam_amd/parity_study.py uses it to predict what the device re-evaluates.

It follows csrc/exact_order.hip step by step, in float32: candidates s_w > thr - eps inside the borders, sorted by the key (score desc, raster asc); marked are
the candidates with |s_w - thr| <= eps (only when at most K candidates have s_w > thr + eps; with more than K of those the exact list is a sorted top K whichever
way the candidates at the threshold fall, and they rank below all of them) and, inside the prefix s_w >= s_w[K-1] - 2 eps (everything when there are fewer than K), those within 2 eps of a sorted
neighbour in the prefix; the distinct 8x8 cells of the marked candidates, in sorted-list order, get the crop slots; every candidate of a cell with a slot takes its
direct score; candidates whose final score is not > thr leave; the ordinary selection (raster order when the count is <= K, else score-descending) runs on the rest."""
import numpy as np

CROP = 88          # crop edge: the cell's 8 pixels + 40 on each side (the receptive field needs 38), origin a multiple of 8
MAXSORT = 16384    # keys the device sorts in LDS; more than that in the part of the list that matters: everything there is marked, cells in cell-index order
DEFAULT_EPS = 9e-6


def crop_origin(c8, extent):
    """origin of the 88-pixel crop along one axis for cell coordinate c8 of an image `extent` pixels long (a multiple of 8, >= 88)"""
    return min(max(8 * c8 - 40, 0), extent - CROP)


def candidates(semi, thr, border):
    """raster indices of the pixels inside the borders with score > thr (float32 compare, as softmax_cand_kernel)"""
    H, W = semi.shape
    ok = semi > np.float32(thr)
    inside = np.zeros_like(ok)
    inside[border:H - border, border:W - border] = True
    return np.flatnonzero(ok & inside)


def select_b(idx, scores, K):
    """topKeypoints (superpoint_tensorrt.cpp:241-253) on a candidate list: everything in raster order when count <= K, else the K best, score desc / raster asc"""
    idx = np.asarray(idx, np.int64); scores = np.asarray(scores, np.float32)
    if len(idx) <= K:
        o = np.argsort(idx, kind="stable")
    else:
        o = np.lexsort((idx, -scores.astype(np.float64)))[:K]
    return idx[o], scores[o]


def direct_list(s_d, thr, border, K):
    """the exact mode's list: (raster indices, scores)"""
    idx = candidates(s_d, thr, border)
    return select_b(idx, s_d.reshape(-1)[idx], K)


def mark(s_w, thr, border, K, eps):
    """steps 1-4: (candidate indices sorted by key, their scores, marked mask over that order, distinct cells of the marked candidates in slot order)"""
    H, W = s_w.shape
    thr = np.float32(thr); eps = np.float32(eps)
    idx = candidates(s_w, thr - eps, border)
    sc = s_w.reshape(-1)[idx].astype(np.float32)
    o = np.lexsort((idx, -sc.astype(np.float64)))
    idx, sc = idx[o], sc[o]
    n = len(idx)
    lo = np.float32(sc[K - 1] - np.float32(2) * eps) if n >= K else np.float32(-1)
    band = np.abs(sc - thr) <= eps
    if int((sc > thr + eps).sum()) > K:      # more than K candidates pass whatever the deviation: the threshold band decides neither the count's side of K nor a top-K place
        band[:] = False
    pre = sc >= lo
    cells = (idx // W // 8) * (W // 8) + (idx % W) // 8
    if int((pre | band).sum()) > MAXSORT:
        marked = pre | band
        return idx, sc, marked, np.unique(cells[marked])
    gap = (sc[:-1] - sc[1:]) <= np.float32(2) * eps            # between sorted neighbours t, t + 1
    near = np.zeros(n, bool)
    near[1:] |= gap & pre[1:]                                   # the neighbour above is in the prefix whenever t is
    near[:-1] |= gap & pre[:-1] & pre[1:]
    marked = band | (pre & near)
    mc = cells[marked]
    _, first = np.unique(mc, return_index=True)
    return idx, sc, marked, mc[np.sort(first)]


def exact_order_list(s_w, s_d, thr, border, K, eps=DEFAULT_EPS, slots=None):
    """The list of the Winograd mode with exact_order on.  s_w, s_d: [H, W] float32 score maps (H, W multiples of 8).
    Returns dict(idx, scores: the final list; marked: marked candidates; cells: the marked cells in slot order; granted: how many of them got a slot)."""
    H, W = s_w.shape
    idx, sc, marked, cells = mark(s_w, thr, border, K, eps)
    granted = len(cells) if slots is None else min(len(cells), max(int(slots), 0))
    got = np.zeros((H // 8) * (W // 8), bool)
    got[cells[:granted]] = True
    cell_of = (idx // W // 8) * (W // 8) + (idx % W) // 8
    final = np.where(got[cell_of], s_d.reshape(-1)[idx], sc).astype(np.float32)
    keep = final > np.float32(thr)
    li, ls = select_b(idx[keep], final[keep], K)
    return {"idx": li, "scores": ls, "marked": int(marked.sum()), "cells": cells, "granted": granted}


def exact_order_batch(s_w, s_d, thr, border, K, eps=DEFAULT_EPS, slots=None):
    """a call of several images: the crop slots go to the images in order.  Returns (list of per-image dicts, cells dropped)"""
    out, left, dropped = [], slots, 0
    for a, b in zip(s_w, s_d):
        r = exact_order_list(a, b, thr, border, K, eps, left)
        if left is not None:
            left -= r["granted"]
        dropped += len(r["cells"]) - r["granted"]
        out.append(r)
    return out, dropped
