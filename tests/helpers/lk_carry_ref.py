"""Host restatements of the LK-carried landmark list (sp_track_use_lk; include/d2fe.h, d2fe_lk_carry_step_device) for the tests of the stereo pipe's sp_lk mode.

  sliding_stereo     the test sequence: one wide synth_image, left frame t = the window at D + step * t px, right frame t = the window at step * t, independent
                     sigma-3 noise on every frame -- the scene moves by (-step, 0) per frame and the right image shows it at (x + D, y)
  carry_step_np      steps b-d in NumPy: reduceVector (opticaltrack_utils.cpp:273-276), removeNearPoints (opticaltrack_utils.h:61-89), the replenishment loop
                     (d2featuretracker.cpp:556-589)
  carry_step_naive   the same lines transcribed one by one into plain Python loops (no NumPy arithmetic shared with the above): what carry_step_np is held to
  compose            the chain over a sequence from a tracker callback (api.lk_track, or the oracle's) + carry_step_np: lists, ids, src, kp, descriptors, right tracks
"""
import math

import numpy as np

DEFAULTS = dict(total_feature_num=150, feature_min_dist=20.0, near_lk_thread_rate=5.0)


def sliding_stereo(n, h, w, seed, disparity, step=3):
    from d2slam_amd.synth import synth_image
    wide = synth_image(h, w + disparity + step * (n - 1), seed).astype(np.float32)
    rng = np.random.RandomState(seed + 7)
    out = []
    for t in range(n):
        pair = []
        for x0 in (disparity + step * t, step * t):
            img = wide[:, x0:x0 + w] + rng.normal(0, 3.0, size=(h, w)).astype(np.float32)
            pair.append(np.clip(np.rint(img), 0, 255).astype(np.uint8))
        out.append(tuple(pair))
    return out


def _near_any(p, q, thr):
    """cv::norm(p - q_j) < thr for any j: float difference, squares and sqrt in double, `<` in double"""
    if len(q) == 0:
        return False
    d = (np.asarray(p, np.float32)[None, :] - np.asarray(q, np.float32)).astype(np.float32)
    s = d[:, 0].astype(np.float64) * d[:, 0].astype(np.float64) + d[:, 1].astype(np.float64) * d[:, 1].astype(np.float64)
    return bool((np.sqrt(s) < np.float64(thr)).any())


def carry_step_np(trk_pts, trk_status, kps, total_feature_num=150, feature_min_dist=20.0, near_lk_thread_rate=5.0):
    """trk_pts [n_prev, 2] float32, trk_status [n_prev]: the tracker's raw output for the previous list; kps [n_kp, 2]: the frame's SuperPoint keypoints.
    Returns pts [n, 2] float32, src [n] (index in the previous list, -1: new), kp [n] (keypoint index, -1: tracked) and the counts."""
    trk_pts = np.asarray(trk_pts, np.float32).reshape(-1, 2); trk_status = np.asarray(trk_status).reshape(-1)
    kps = np.asarray(kps, np.float32).reshape(-1, 2)
    near_thr = np.float64(np.float32(near_lk_thread_rate))         # a float parameter in the reference, widened by the comparison
    alive = np.nonzero(trk_status != 0)[0]                          # b. reduceVector
    pts = np.zeros((0, 2), np.float32); src = []
    for i in alive:                                                 # c. removeNearPoints
        if not _near_any(trk_pts[i], pts, near_thr):
            pts = np.concatenate([pts, trk_pts[i][None]]); src.append(int(i))
    m = len(src)
    kp = [-1] * m
    for i in range(len(kps)):                                       # d. replenish
        if len(src) > total_feature_num:
            break
        if not _near_any(kps[i], pts, np.float64(feature_min_dist)):
            pts = np.concatenate([pts, kps[i][None]]); src.append(-1); kp.append(i)
    return dict(pts=pts, src=np.array(src, np.int32), kp=np.array(kp, np.int32), n=len(src), n_tracked_in=len(trk_status),
                n_lost=len(trk_status) - len(alive), n_removed_near=len(alive) - m, n_new=len(src) - m)


def _f32(v):
    return float(np.float32(v))


def _cv_norm_diff(a, b):
    """cv::norm(a - b) for two Point2f: operator- in float, norm() = sqrt((double)x * x + (double)y * y)"""
    dx = _f32(_f32(a[0]) - _f32(b[0])); dy = _f32(_f32(a[1]) - _f32(b[1]))
    return math.sqrt(dx * dx + dy * dy)


def carry_step_naive(trk_pts, trk_status, kps, total_feature_num=150, feature_min_dist=20.0, near_lk_thread_rate=5.0):
    """line-by-line transcription of the cited reference lines; same return value as carry_step_np"""
    # reduceVector(cur_pts, status) ... (opticaltrack_utils.cpp:273-276)
    lk_pts, lk_src = [], []
    for i in range(len(trk_status)):
        if trk_status[i]:
            lk_pts.append((_f32(trk_pts[i][0]), _f32(trk_pts[i][1]))); lk_src.append(i)
    n_alive = len(lk_pts)
    # removeNearPoints(info, near_lk_thread_rate) (opticaltrack_utils.h:61-89)
    thr = _f32(near_lk_thread_rate)
    new_pts, status, remove_count = [], [], 0
    for i in range(len(lk_pts)):
        has_nearby = False
        for j in range(len(new_pts)):
            if _cv_norm_diff(lk_pts[i], new_pts[j]) < thr:
                has_nearby = True
                break
        if not has_nearby:
            new_pts.append(lk_pts[i]); status.append(True)
        else:
            status.append(False); remove_count += 1
    lk_pts = [p for p, s in zip(lk_pts, status) if s]
    lk_src = [p for p, s in zip(lk_src, status) if s]
    lk_kp = [-1] * len(lk_pts)
    # the replenishment loop (d2featuretracker.cpp:556-589)
    count_new = 0
    for i in range(len(kps)):
        if len(lk_pts) > total_feature_num:
            break
        lm = (_f32(kps[i][0]), _f32(kps[i][1]))
        has_near = False
        for pt in lk_pts:
            if _cv_norm_diff(pt, lm) < float(feature_min_dist):
                has_near = True
                break
        if not has_near:
            lk_pts.append(lm); lk_src.append(-1); lk_kp.append(i)
            count_new += 1
    return dict(pts=np.array(lk_pts, np.float32).reshape(-1, 2), src=np.array(lk_src, np.int32), kp=np.array(lk_kp, np.int32), n=len(lk_pts),
                n_tracked_in=len(trk_status), n_lost=len(trk_status) - n_alive, n_removed_near=remove_count, n_new=count_new)


def compose(frames, keypoints, track, params=None, state=None):
    """The chain over `frames` [(left, right), ...] in time order.  keypoints[t] = (kps [n, 2], scores [n], desc [n, D]) of left frame t (the pipe's own, or the
    oracle's); track(prev_img, cur_img, pts) -> (cur_pts [n, 2] float32, status [n]) is the bidirectional tracker on the pyramids of two images
    (WHOLE_IMG_MATCH, cur_init = pts).  state: what a previous call returned as out[-1]["state"], to go on from it.  Per frame: the dict of carry_step_np plus
    id, desc, scores, right_pts, right_status, trk_pts, trk_status."""
    prm = dict(DEFAULTS); prm.update(params or {})
    st = state or dict(pts=np.zeros((0, 2), np.float32), id=np.zeros(0, np.int32), desc=None, scores=np.zeros(0, np.float32), img=None, next_id=0)
    out = []
    for (left, right), (kps, scores, desc) in zip(frames, keypoints):
        n_prev = len(st["pts"])
        if n_prev:
            trk_pts, trk_st = track(st["img"], left, st["pts"])
        else:
            trk_pts, trk_st = np.zeros((0, 2), np.float32), np.zeros(0, np.uint8)
        r = carry_step_np(trk_pts, trk_st, kps, **prm)
        n, m = r["n"], r["n"] - r["n_new"]
        D = desc.shape[1]
        r["id"] = np.zeros(n, np.int32); r["desc"] = np.zeros((n, D), np.float32); r["scores"] = np.zeros(n, np.float32)
        r["id"][:m] = st["id"][r["src"][:m]]; r["id"][m:] = st["next_id"] + np.arange(n - m)
        if m:
            r["desc"][:m] = st["desc"][r["src"][:m]]; r["scores"][:m] = st["scores"][r["src"][:m]]
        r["desc"][m:] = desc[r["kp"][m:]]; r["scores"][m:] = scores[r["kp"][m:]]
        r["trk_pts"], r["trk_status"] = trk_pts, trk_st
        if n:
            r["right_pts"], r["right_status"] = track(left, right, r["pts"])
        else:
            r["right_pts"], r["right_status"] = np.zeros((0, 2), np.float32), np.zeros(0, np.uint8)
        st = dict(pts=r["pts"], id=r["id"], desc=r["desc"], scores=r["scores"], img=left, next_id=st["next_id"] + (n - m))
        r["state"] = st
        out.append(r)
    return out
