"""The CPU oracle composition of the quad pipe's sp_lk mode on the scene of tests/test_quad_pipe_sp_lk.py: oracle SuperPoint + oracle LK + the NumPy list logic
(tests/helpers/quad_lk_ref.py).  Prints the tracking figures that test takes its floors from.  No GPU.
    python tools/quad_sp_lk_oracle.py [--wino]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from oracle import oracle as orc
    from tests.helpers import quad_lk_ref as qref
    from tests import test_quad_pipe_sp_lk as T
    from tests.test_quad_pipe import _weights
    orc.build()
    wino = "--wino" in sys.argv
    frames = qref.cyclic_quads(T.NQ, T.SEED)
    w = _weights()
    views = [[frames[t, c] for c in range(4)] for t in range(T.NQ)]           # identity maps: a raw frame is its own view
    kps = []
    for t in range(T.NQ):
        row = []
        for c in range(4):
            k, s, d, _, _ = orc.extract_b(views[t][c], w, 0.15, 1, T.CAP, wino=wino)
            row.append((k, s, d))
        kps.append(row)
    print("keypoints per view", [[len(r[0]) for r in row] for row in kps])
    pyr = lambda img: orc.pyr_build(img, 2)
    track = lambda a, b, p: orc.lk_track(pyr(a), pyr(b), qref.W, qref.H, p, p, levels=2, win=21, iters=30)
    half = lambda a, b, p, init, typ, mc: orc.lk_track(pyr(a), pyr(b), qref.W, qref.H, p, init, levels=2, win=21, iters=30, track_type=typ, move_cols=mc)
    comp, nbs = qref.compose_quad(views, kps, track, half, dict(T.BASE))
    print("n", [[k["n"] for k in row] for row in comp])
    print("lost", [[k["n_lost"] for k in row] for row in comp])
    print("new", [[k["n_new"] for k in row] for row in comp])
    print("eligible", [[int(p["eligible"].sum()) for p in row] for row in nbs])
    T._figures(comp, nbs, "oracle" + (" (wino)" if wino else ""))


if __name__ == "__main__":
    main()
