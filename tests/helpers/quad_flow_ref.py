"""Host restatement for the quad pipe's flow_lk mode (d2fe_quad_flow_enable, include/d2fe.h): trackLocalFrames with enable_lk_optical_flow, WITHOUT sp_track_use_lk
and beside SuperPoint (d2frontend/src/d2featuretracker.cpp:121-133; config/quadcam/quadcam_single.yaml).

  compose_quad_flow    the four cameras' FLOW lists over a sequence of quad frames: flow_lk_ref.compose per camera with a state per camera and ONE id counter handed
                       on in camera order 0, 1, 2, 3 (every camera's track() of a quad frame draws its new ids from the one lmanager, :123-125), then
                       trackLK(left, right, type) of the four neighbour pairs (:128-132, :697-752) on the flow lists AFTER this frame's step, with the gate and the
                       shifted initial guess of quad_lk_ref.half_gate / move_cols

The scene, the identity maps and the naive id order are quad_lk_ref's (cyclic_quads, identity_maps, quad_ids_naive)."""
import numpy as np

from tests.helpers import flow_lk_ref as fref
from tests.helpers import quad_lk_ref as qref


def compose_quad_flow(views, keypoints, track, track_half, detect, params=None, width=qref.W, fov=qref.FOV):
    """views[t][c]: u8 image; keypoints[t][c]: kps [n, 2] of that view (they only block candidates) or None; track(prev_img, cur_img, pts) and detect(img, num) as for
    flow_lk_ref.compose; track_half(img_a, img_b, pts, init, track_type, move_cols) -> (cur_pts, status): the bidirectional tracker with a half-image type.
    Returns out[t][c] = compose()'s dict of camera c and nb[t][n] = dict(eligible [n_a] bool, pts [n_a, 2], status [n_a]) of neighbour pair n, scattered back to
    the slots of flow list a (zeros elsewhere)."""
    states, next_id = [None] * 4, 0
    out, nb = [], []
    mc = float(qref.move_cols(width, fov))
    for t in range(len(views)):
        row = []
        for c in range(4):
            st = states[c]
            if st is None:
                st = dict(pts=np.zeros((0, 2), np.float32), id=np.zeros(0, np.int32), img=None, next_id=next_id)
            else:
                st = dict(st); st["next_id"] = next_id
            r = fref.compose([views[t][c]], [keypoints[t][c]], track, detect, params, state=st)[0]
            states[c] = r["state"]; next_id = r["next_id"]
            row.append(r)
        out.append(row)
        pairs = []
        for (a, b, typ) in qref.NEIGHBOURS:
            pts = row[a]["pts"]
            ok, init = qref.half_gate(pts, typ, width, fov)
            xy = np.zeros((len(pts), 2), np.float32); stt = np.zeros(len(pts), np.uint8)
            if ok.any():
                xy[ok], stt[ok] = track_half(views[t][a], views[t][b], pts[ok], init, typ, mc)
            pairs.append(dict(eligible=ok, pts=xy, status=stt))
        nb.append(pairs)
    return out, nb
