"""Host restatements of the flow landmarks (enable_lk_optical_flow without sp_track_use_lk; include/d2fe.h, d2fe_lk_flow_step_device) for the tests of the
FAST-replenished LK list.

  flow_step_np      steps b-e in NumPy: reduceVector (opticaltrack_utils.cpp:273-276), removeNearPoints (opticaltrack_utils.h:61-89), detectPoints with use_fast
                    (opticaltrack_utils.cpp:375-442) against landmarks2D() = the SuperPoint keypoints followed by the tracked entries (d2featuretracker.cpp:500-525,595-596)
  flow_step_naive   the same lines transcribed one by one into plain Python loops (no NumPy arithmetic shared with the above): what flow_step_np is held to
  compose           the chain over a sequence from a tracker callback and a detector callback: lists, ids, src, header counts, right tracks
  dot_image         a constant image of value 50 with single pixels of chosen brightness: an isolated pixel of value v is a FAST corner exactly there, response v - 51

The candidates of a step are either a callable detect(num) -> xy [k, 2] (detectFastByRegion(img, num, 3, 4): sorted, at most num) or a raw candidate list
(xy [k, 2], response [k], order [k]) in any order, which the step sorts as the detector does (response descending, order ascending) and cuts at num.
"""
import numpy as np

from tests.helpers.lk_carry_ref import _cv_norm_diff, _f32, _near_any

DEFAULTS = dict(total_feature_num=150, feature_min_dist=20.0, near_lk_thread_rate=5.0)


def dot_image(h, w, dots):
    """dots: (x, y, value) triples"""
    img = np.full((h, w), 50, np.uint8)
    for x, y, v in dots:
        img[int(y), int(x)] = v
    return img


def _candidates_np(cand, num):
    if callable(cand):
        return np.asarray(cand(num), np.float32).reshape(-1, 2)[:num]
    xy, resp, order = cand
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    k = np.lexsort((np.asarray(order, np.int64), -np.asarray(resp, np.int64)))
    return xy[k][:num]


def flow_step_np(trk_pts, trk_status, kps, cand, total_feature_num=150, feature_min_dist=20.0, near_lk_thread_rate=5.0):
    """trk_pts [n_prev, 2] float32, trk_status [n_prev]: the tracker's raw output for the previous list; kps [n_kp, 2]: the frame's SuperPoint keypoints (they block
    candidates, they are not in the list).  Returns pts [n, 2] float32, src [n] (index in the previous list, -1: new) and the counts of the list header."""
    trk_pts = np.asarray(trk_pts, np.float32).reshape(-1, 2); trk_status = np.asarray(trk_status).reshape(-1)
    kps = np.zeros((0, 2), np.float32) if kps is None else np.asarray(kps, np.float32).reshape(-1, 2)
    near_thr = np.float64(np.float32(near_lk_thread_rate))
    alive = np.nonzero(trk_status != 0)[0]                          # b. reduceVector
    pts = np.zeros((0, 2), np.float32); src = []
    for i in alive:                                                 # c. removeNearPoints
        if not _near_any(trk_pts[i], pts, near_thr):
            pts = np.concatenate([pts, trk_pts[i][None]]); src.append(int(i))
    m = len(src)
    have = len(kps) + m                                             # d. detectPoints
    lack = int(total_feature_num) - have
    num, n_cand = 0, 0
    if lack > int(total_feature_num) // 4:
        num = 2 * lack if have > 0 else lack
        c = _candidates_np(cand, num)
        n_cand = len(c)
        blockers = np.concatenate([kps, pts])
        for p in c:
            if len(src) - m >= lack:
                break
            if not _near_any(p, blockers, np.float64(feature_min_dist)):
                blockers = np.concatenate([blockers, p[None]]); pts = np.concatenate([pts, p[None]]); src.append(-1)
    return dict(pts=pts, src=np.array(src, np.int32), n=len(src), n_tracked_in=len(trk_status), n_lost=len(trk_status) - len(alive), n_removed_near=len(alive) - m,
                n_new=len(src) - m, lack=lack, num=num, n_cand=n_cand)


def _candidates_naive(cand, num):
    if callable(cand):
        return [(_f32(p[0]), _f32(p[1])) for p in list(cand(num))[:num]]
    xy, resp, order = cand
    kpts = [(_f32(xy[i][0]), _f32(xy[i][1]), int(resp[i]), int(order[i])) for i in range(len(resp))]
    # std::sort by response, descending (:480-483); the order among equal responses is the one d2fe_detect_fast_by_region fixes: `order` ascending
    done = []
    while kpts:
        best = 0
        for j in range(1, len(kpts)):
            if kpts[j][2] > kpts[best][2] or (kpts[j][2] == kpts[best][2] and kpts[j][3] < kpts[best][3]):
                best = j
        done.append(kpts.pop(best))
    ret = []
    for k in done:                                                  # :485-490
        if num <= 0:
            break
        ret.append((k[0], k[1]))
        if len(ret) >= num:
            break
    return ret


def flow_step_naive(trk_pts, trk_status, kps, cand, total_feature_num=150, feature_min_dist=20.0, near_lk_thread_rate=5.0):
    """line-by-line transcription of the cited reference lines; same return value as flow_step_np"""
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
    # cur_pts = frame.landmarks2D(): the SuperPoint landmarks, then the LK ones (d2featuretracker.cpp:500-525,595-596)
    cur_pts = [] if kps is None else [(_f32(k[0]), _f32(k[1])) for k in kps]
    cur_pts = cur_pts + list(lk_pts)
    # detectPoints (opticaltrack_utils.cpp:375-442)
    require_pts = int(total_feature_num)
    lack_up_top_pts = require_pts - len(cur_pts)
    n_pts, num_to_detect, n_cand = [], 0, 0
    if lack_up_top_pts > int(require_pts / 4):
        num_to_detect = lack_up_top_pts
        if len(cur_pts) > 0:
            num_to_detect = lack_up_top_pts * 2
        n_pts_tmp = _candidates_naive(cand, num_to_detect)
        n_cand = len(n_pts_tmp)
        all_pts = list(cur_pts)
        for pt in n_pts_tmp:
            has_nearby = False
            for pt_j in all_pts:
                if _cv_norm_diff(pt, pt_j) < float(feature_min_dist):
                    has_nearby = True
                    break
            if not has_nearby:
                n_pts.append(pt); all_pts.append(pt)
            if len(n_pts) >= lack_up_top_pts:
                break
    pts = list(lk_pts) + n_pts
    src = list(lk_src) + [-1] * len(n_pts)
    return dict(pts=np.array(pts, np.float32).reshape(-1, 2), src=np.array(src, np.int32), n=len(pts), n_tracked_in=len(trk_status), n_lost=len(trk_status) - n_alive,
                n_removed_near=remove_count, n_new=len(n_pts), lack=lack_up_top_pts, num=num_to_detect, n_cand=n_cand)


def compose(frames, keypoints, track, detect, params=None, state=None):
    """The chain over `frames` in time order: images, or (left, right) pairs (then every list is also tracked left -> right).  keypoints[t] = kps [n, 2] of (left)
    frame t, or None (flow only).  track(prev_img, cur_img, pts) -> (cur_pts [n, 2] float32, status [n]) is the bidirectional tracker (WHOLE_IMG_MATCH, cur_init = pts);
    detect(img, num) -> xy [k, 2] is detectFastByRegion(img, num, 3, 4).  state: what a previous call returned as out[-1]["state"].  Per frame: the dict of
    flow_step_np plus id, next_id, trk_pts, trk_status (and right_pts, right_status)."""
    prm = dict(DEFAULTS); prm.update(params or {})
    st = state or dict(pts=np.zeros((0, 2), np.float32), id=np.zeros(0, np.int32), img=None, next_id=0)
    out = []
    for fr, kps in zip(frames, keypoints):
        left, right = fr if isinstance(fr, (tuple, list)) else (fr, None)
        if len(st["pts"]):
            trk_pts, trk_st = track(st["img"], left, st["pts"])
        else:
            trk_pts, trk_st = np.zeros((0, 2), np.float32), np.zeros(0, np.uint8)
        r = flow_step_np(trk_pts, trk_st, kps, lambda num: detect(left, num), **prm)
        n, m = r["n"], r["n"] - r["n_new"]
        r["id"] = np.zeros(n, np.int32)
        r["id"][:m] = st["id"][r["src"][:m]]; r["id"][m:] = st["next_id"] + np.arange(n - m)
        r["next_id"] = st["next_id"] + (n - m)
        r["trk_pts"], r["trk_status"] = trk_pts, trk_st
        if right is not None:
            r["right_pts"], r["right_status"] = track(left, right, r["pts"]) if n else (np.zeros((0, 2), np.float32), np.zeros(0, np.uint8))
        st = dict(pts=r["pts"], id=r["id"], img=left, next_id=r["next_id"])
        r["state"] = st
        out.append(r)
    return out
