"""Child process of tests/test_launch_regimes.py::test_wino_walk_boundaries: single Winograd layers (d2fe_debug_conv3x3_wino of the development library)
whose work-item counts sit just below, at and just above one round of persistent workgroups and just above two, against orc.conv_wino, bit for bit.
A process of its own because D2FE_WINO_NT (which forces the 32- or the 64-channel item form) is read once per process.

With H = 8, W = 16, cout = 64 one image is ONE 64-channel item (NT = 2) or TWO 32-channel items (NT = 1), so the image count sets the item count.
The parent starts it with D2FE_WINO_NT = 1 and = 2.  The size of a round is the launcher's business: the worker learns it from the launch-regime record (a
probe launch of 2 ncu + 1 images is past one round in either form; the record's grid of that launch is the round, its item count tells the items per image),
not from a copy of the launch rule.

Prints one JSON line: {"ncu", "grid", "items_per_image", "cases": [{"kind", "n", "cin", "pool", "equal", "max_diff", "regimes": {name: count, nonzero only},
"grid", "total"}]}."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

H, W, COUT = 8, 16, 64


def _layer(rng, n, cin):
    x = np.maximum(rng.standard_normal((n, H, W, cin)).astype(np.float32), 0.0)    # post-ReLU activations
    wg = (rng.standard_normal((COUT, cin, 3, 3)) * (0.6 / np.sqrt(cin))).astype(np.float32)
    b = (rng.standard_normal(COUT) * 0.1).astype(np.float32)
    return x, wg, b


def run_case(api, orc, fe, kind, n, cin, pool):
    x, wg, b = _layer(np.random.default_rng(1000 * n + cin + int(pool)), n, cin)
    api.DevFrontEnd.regime_reset()
    out, _ = fe.debug_conv3x3_wino(x, wg, b, pool=pool)
    rec = api.DevFrontEnd.regime_counts()
    equal, worst = True, 0.0
    for i in range(n):
        ref = orc.conv_wino(x[i], wg, b, True)
        if pool:
            ref = orc.maxpool2(ref)
        if not np.array_equal(out[i], ref):
            equal = False
            worst = max(worst, float(np.nanmax(np.abs(out[i] - ref))))
    return {"kind": kind, "n": n, "cin": cin, "pool": bool(pool), "equal": equal, "max_diff": worst, "grid": rec["wino_last_grid"], "total": rec["wino_last_total"],
            "regimes": {k: v for k, v in rec.items() if v and not k.startswith("wino_last")}}


def main():
    import torch
    from d2slam_amd import api
    from oracle import oracle as orc
    ncu = int(torch.cuda.get_device_properties(0).multi_processor_count)
    fe = api.DevFrontEnd(api.SuperPointConfig(max_keypoints=16, input_width=64, input_height=64, max_batch=1))
    probe = run_case(api, orc, fe, "probe", 2 * ncu + 1, 64, False)
    grid, per_img = probe["grid"], probe["total"] // probe["n"]      # workgroups of one round; items one image makes in the form this process runs
    assert probe["grid"] < probe["total"] and per_img in (1, 2), probe

    def images(items_at_least):      # the smallest image count with at least that many items
        return -(-items_at_least // per_img)
    below, at, above, two = (grid - 1) // per_img, images(grid), images(grid + 1), images(2 * grid + 1)
    cases = [probe]
    for kind, n, cin, pool in [("below", below, 64, False), ("at", at, 64, False), ("above", above, 64, False), ("two", two, 64, False),
                               ("above", above, 128, True), ("two", two, 64, True), ("two", two, 128, False), ("at", at, 128, True)]:
        cases.append(run_case(api, orc, fe, kind, n, cin, pool))
    fe.close()
    print(json.dumps({"ncu": ncu, "grid": grid, "items_per_image": per_img, "forced_nt": os.environ.get("D2FE_WINO_NT", ""), "cases": cases}))


if __name__ == "__main__":
    main()
