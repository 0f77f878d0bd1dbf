"""Host restatements for the quad pipe's sp_lk mode (d2fe_quad_track_enable, include/d2fe.h): trackLocalFrames with enable_lk_optical_flow and sp_track_use_lk
(d2frontend/src/d2featuretracker.cpp:121-133).

  cyclic_quads         the test scene: a cyclic panorama (one synth_image of 120 x 360 read with wrap-around), view c of quad frame t = the 200-column window
                       starting at (3 t - 90 c) mod 360 plus independent sigma-3 noise.  The scene moves by (-3, 0) per frame; with undistort_fov 200 move_cols is
                       exactly 90.0, a point at x in view a sits at x + 90 in view a + 1, and at x - 90 from view 0 to view 3 (3 * 90 = 270 = -90 mod 360)
  identity_maps        undistortion maps under which a raw frame is its own view (no gain)
  half_gate            the gate and the shifted initial guess of opticalflowTrackPyr's half-image types (opticaltrack_utils.cpp:195-223)
  compose_quad         the four cameras' lists over a sequence of quad frames: lk_carry_ref.compose per camera, ONE id counter handed on in camera order 0, 1, 2, 3
                       (every camera's track() of a quad frame draws its new ids from the one lmanager, :123-125 + :556-589), then trackLK(left, right, type) of the
                       four neighbour pairs (:128-132, :697-752) on the lists AFTER this frame's step
  quad_ids_naive       the id order alone, transcribed into plain loops: what compose_quad's ids are held to
"""
import numpy as np

from tests.helpers import lk_carry_ref as ref

H, W, PANO, STEP, SHIFT = 120, 200, 360, 3, 90
FOV = 200.0
NEIGHBOURS = [(0, 1, 1), (1, 2, 1), (2, 3, 1), (0, 3, 2)]      # (view a, view b, type): 1 LEFT_RIGHT_IMG_MATCH, 2 RIGHT_LEFT_IMG_MATCH


def cyclic_quads(n, seed):
    """u8 [n][4][H][W]"""
    from d2slam_amd.synth import synth_image
    pano = synth_image(H, PANO, seed).astype(np.float32)
    rng = np.random.RandomState(seed + 11)
    out = np.empty((n, 4, H, W), np.uint8)
    for t in range(n):
        for c in range(4):
            cols = (STEP * t - SHIFT * c + np.arange(W)) % PANO
            out[t, c] = np.clip(np.rint(pano[:, cols] + rng.normal(0, 3.0, size=(H, W)).astype(np.float32)), 0, 255).astype(np.uint8)
    return out


def identity_maps():
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    return [(xx.copy(), yy.copy(), None) for _ in range(4)]


def move_cols(width, fov):
    """float move_cols = cur_img.cols * 90.0 / params->undistort_fov (opticaltrack_utils.cpp:191-193): double arithmetic, stored as a float"""
    return np.float32(width * 90.0 / fov)


def half_gate(pts, track_type, width, fov):
    """(eligible [n] bool, cur_init [n, 2] float32 of the eligible points) of opticaltrack_utils.cpp:200-218: float comparisons against cols - move_cols /
    move_cols, x shifted in float"""
    p = np.asarray(pts, np.float32).reshape(-1, 2)
    mc = move_cols(width, fov)
    if track_type == 1:
        ok = p[:, 0] < np.float32(np.float32(width) - mc)
        init = p[ok].copy(); init[:, 0] = init[:, 0] + mc
    else:
        ok = p[:, 0] >= mc
        init = p[ok].copy(); init[:, 0] = init[:, 0] - mc
    return ok, init


def compose_quad(views, keypoints, track, track_half, params=None, width=W, fov=FOV):
    """views[t][c]: u8 image; keypoints[t][c] = (kps, scores, desc) of that view; track(prev_img, cur_img, pts) as for lk_carry_ref.compose;
    track_half(img_a, img_b, pts, init, track_type, move_cols) -> (cur_pts, status): the bidirectional tracker with a half-image type.
    Returns out[t][c] = compose()'s dict of camera c (without right tracks) and nb[t][n] = dict(eligible [n_a] bool, pts [n_a, 2], status [n_a]) of neighbour pair
    n, scattered back to the slots of list a (zeros elsewhere)."""
    temporal = lambda a, b, p: (np.zeros((len(p), 2), np.float32), np.zeros(len(p), np.uint8)) if a is b else track(a, b, p)      # compose()'s right track: unused
    states, next_id = [None] * 4, 0
    out, nb = [], []
    mc = float(move_cols(width, fov))
    for t in range(len(views)):
        row = []
        for c in range(4):
            st = states[c]
            if st is not None:
                st = dict(st); st["next_id"] = next_id
            elif next_id:
                st = dict(pts=np.zeros((0, 2), np.float32), id=np.zeros(0, np.int32), desc=None, scores=np.zeros(0, np.float32), img=None, next_id=next_id)
            v = views[t][c]
            r = ref.compose([(v, v)], [keypoints[t][c]], temporal, params, state=st)[0]
            states[c] = r["state"]; next_id = r["state"]["next_id"]
            row.append(r)
        out.append(row)
        pairs = []
        for (a, b, typ) in NEIGHBOURS:
            pts = row[a]["pts"]
            ok, init = half_gate(pts, typ, width, fov)
            xy = np.zeros((len(pts), 2), np.float32); stt = np.zeros(len(pts), np.uint8)
            if ok.any():
                xy[ok], stt[ok] = track_half(views[t][a], views[t][b], pts[ok], init, typ, mc)
            pairs.append(dict(eligible=ok, pts=xy, status=stt))
        nb.append(pairs)
    return out, nb


def quad_ids_naive(steps):
    """steps[t][c] = (src [n] of camera c's list in quad frame t: index in its previous list, -1 for a new entry).  The ids as trackLocalFrames hands them out:
    for every quad frame, for c = 0, 1, 2, 3 in turn (track(images[c]), :123-125), a tracked entry keeps its landmark's id and every appended keypoint takes the
    next id of the ONE landmark counter (:556-589).  Returns ids[t][c] as lists."""
    counter = 0
    prev = [[] for _ in range(4)]
    ids = []
    for frame in steps:
        row = []
        for c in range(4):
            cur = []
            for s in frame[c]:
                if s >= 0:
                    cur.append(prev[c][s])
                else:
                    cur.append(counter)
                    counter += 1
            prev[c] = cur
            row.append(cur)
        ids.append(row)
    return ids
