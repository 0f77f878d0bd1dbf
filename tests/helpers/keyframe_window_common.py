"""Shared by tests/test_keyframe_window_cpu.py and tests/test_keyframe_window.py: the planted windows and remote frames of the keyframe-window tests (unit vectors with
near-copies, tests/test_ref_pin.py's planting), the selection rule as a numpy statement, and the expected result of one remote frame from the oracle's tracker_gate.

Planting, with threshold THRES = 0.5: a near-copy (noise 0.3 / sqrt(G)) has similarity about 0.96, a looser copy (noise 1.0 / sqrt(G)) about 0.7, unrelated unit vectors
about 0 (standard deviation 1 / sqrt(G)).  Remote frame q is of kind q % 6:
  0  a near-copy of an OLDER keyframe of which a NEWER keyframe is a looser copy: the newer one merely passes and wins, with the lower similarity (n >= 2)
  1  a near-copy of view 0 of the keyframe whose view 0 resembles its own view 3: two views of one keyframe pass, view 3 comes first in dirs = {2, 3, 0, 1} (quad)
  2  unrelated: no keyframe passes
  3  a near-copy whose own gate view has no keypoints (the gate looks at NetVLAD only; the first problem has an empty side)
  4  a near-copy of the keyframe that has a view without keypoints
  5  a near-copy of a random view of a random keyframe (quad: every rotation of the view table)"""
import numpy as np

THRES = 0.5
DIRS = (2, 3, 0, 1)
D = 256


def unit_rows(a):
    a = np.asarray(a, np.float32)
    return (a / np.linalg.norm(a, axis=-1, keepdims=True)).astype(np.float32)


def near(rng, v, amount):
    return unit_rows(v + (amount / np.sqrt(v.shape[-1])) * rng.randn(*v.shape).astype(np.float32))


def plant(n, V):
    """which keyframes carry what: old / new (new's views are looser copies of old's), dup (V = 4: its view 0 resembles its view 3), empty (a view without keypoints)"""
    if n == 0:
        return dict(old=None, new=None, dup=None, empty=None)
    if n == 1:
        return dict(old=None, new=None, dup=0 if V == 4 else None, empty=0)
    if n == 2:
        return dict(old=0, new=1, dup=None, empty=1)
    return dict(old=0, new=n - 2, dup=(1 if n >= 4 else 2) if V == 4 else None, empty=2)


def make_window(rng, n, V, G, cap, with_desc=True):
    """n keyframes, oldest first: netvlad [n][V][G], desc [n][V][cap][D], n_kp [n][V], planted as plant(n, V) says"""
    nv = unit_rows(rng.randn(max(n, 1), V, G))[:n]
    desc = unit_rows(rng.randn(max(n, 1), V, cap, D))[:n] if with_desc else None
    nk = rng.randint(max(cap // 3, 2), cap + 1, size=(n, V)).astype(np.int32)
    p = plant(n, V)
    if p["dup"] is not None:
        nv[p["dup"], 0] = near(rng, nv[p["dup"], 3], 0.6)
    if p["new"] is not None:
        nv[p["new"]] = near(rng, nv[p["old"]], 1.0)
    if p["empty"] is not None:
        nk[p["empty"], 3 if V == 4 else 0] = 0
    return nv, desc, nk


def make_remote(rng, nq, win, V, G, cap, with_desc=True):
    """nq remote frames against a window: netvlad [nq][V][G], desc [nq][V][cap][D], n_kp [nq][V]"""
    wnv, wdesc, wnk = win
    n = len(wnv)
    p = plant(n, V)
    gv = 2 if V == 4 else 0
    nv = unit_rows(rng.randn(nq, V, G))
    desc = unit_rows(rng.randn(nq, V, cap, D)) if with_desc else None
    nk = rng.randint(max(cap // 3, 2), cap + 1, size=(nq, V)).astype(np.int32)
    for q in range(nq):
        kind = q % 6
        if n == 0 or kind == 2:
            continue
        k, b = int(rng.randint(n)), gv                     # the keyframe, and its view, that the remote gate view is a near-copy of
        kd = k                                             # the keyframe whose landmarks the remote views see
        if kind == 0 and p["new"] is not None:
            k, kd = p["old"], p["new"]                     # about 0.96 with the older keyframe, about 0.68 with the newer one, which wins
        elif kind == 1 and p["dup"] is not None:
            k = kd = p["dup"]; b = 0
        elif kind == 4:
            k = kd = p["empty"]
        elif kind == 5 and V == 4:
            b = int(rng.randint(4))
        nv[q, gv] = near(rng, wnv[k, b], 0.3)
        if kind == 3:
            nk[q, gv] = 0
        if with_desc:
            bb = 3 if (kind == 1 and p["dup"] is not None) else b      # the view that wins the walk
            for a in range(V):                               # the views that will be paired see the same landmarks
                lv = (bb - gv + a) % V
                desc[q, a] = unit_rows(wdesc[kd, lv][rng.permutation(cap)] + 0.05 * rng.randn(cap, D).astype(np.float32))
    return nv, desc, nk


def sims64(rnv, wnv, V):
    """every (remote gate view) . (keyframe, dirs[j]) in float64: [nq][n][V]"""
    gv = 2 if V == 4 else 0
    order = list(DIRS) if V == 4 else [0]
    return np.einsum("qg,kjg->qkj", rnv[:, gv].astype(np.float64), wnv[:, order].astype(np.float64)) if len(wnv) else np.zeros((len(rnv), 0, V))


def select(sims, thres):
    """The selection rule, stated once: sims [n][V] in window order (oldest first) and dirs order.  Among the pairs with !(sim < thres) the one with the smallest
    (n - 1 - pos) * V + j -> (pos, j), or None."""
    sims = np.asarray(sims)
    n = sims.shape[0]
    V = sims.shape[1] if sims.ndim == 2 else 1
    keys = [(n - 1 - pos) * V + j for pos in range(n) for j in range(V) if not (sims[pos, j] < thres)]
    if not keys:
        return None
    return n - 1 - min(keys) // V, min(keys) % V


def expected(orc, spref, rnv, rnk, win, V, thres):
    """One remote frame against the oracle's tracker_gate (and the reference-compiled gate where it is available): None, or dict(pos, dir_a, dir_b, pairs, sim) with
    pairs = [(remote view, local view)] of the problems with both sides non-empty"""
    wnv, _, wnk = win
    quad = V == 4
    o = orc.tracker_gate(rnv, wnv, thres, quad, rnk, wnk)
    if spref is not None and spref.available():
        r = spref.tracker_gate(rnv, wnv, thres, quad, rnk, wnk)
        assert (o is None) == (r is None)
        if o is not None:
            assert (o["kf"], o["dir_a"], o["dir_b"]) == (r["kf"], r["dir_a"], r["dir_b"])
            if quad:
                assert o["pairs"] == r["pairs"]
    if o is None:
        return None
    pairs = o["pairs"] if quad else ([(0, 0)] if int(rnk[0]) > 0 and int(wnk[o["kf"], 0]) > 0 else [])
    j = DIRS.index(o["dir_b"]) if quad else 0
    return dict(pos=o["kf"], dir_a=o["dir_a"], dir_b=o["dir_b"], pairs=pairs, sim=float(o["sims"][j]))
