#!/usr/bin/env python3
"""What the bearings mode of the stereo pipe costs and what it replaces, in ONE process, rounds alternating A, B, C, A, B, C, ...:
  A  the lr_lk + sp_lk pipe as it is (the reference's default stereo path): the caller still owes the per-point pass
  B  A with d2fe_pipe_bearings_enable: bearings, extrinsic predictions and the lk_lk_use_pred gate inside the pass, read with d2fe_pipe_bearings_result_get
  C  A plus the host composition on every waited result: the NumPy lift, prediction and gate of tests/helpers/bearings_ref.py over the keypoints, the list entries
     and their right tracks, standing in for the caller's loop (createLKLandmark / predictLandmarksWithExtrinsic in the tracker thread)
All three as benchlib/pipe_legs.py sets the pipe up for bench.py's `value`: 640x480, 200 keypoints, NetVLAD, the temporal match, frames from pinned host memory, every
result back in pinned host memory inside the timed window, the same synthetic frames and seeded weights.  Two operating points: 32 frames per submit with four submits
in flight, and one frame per submit on four lanes with four in flight.  Prints (and writes to --out) one JSON object: frames/s medians, the min..max of each, B/A,
B/C, and the time of the one more launch from HIP events (profile mode 2: stage `lk` of B minus stage `lk` of A, per pass).  Nothing is gated on these numbers.
Usage: python tools/bench_pipe_bearings.py [--rounds 5] [--precision wino] [--out profiles/pipe_bearings.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--precision", default="wino")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pipe_bearings.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from benchlib.common import CAP, H, W
    from benchlib.pipe_legs import pipe_frames
    from d2slam_amd import api, netvlad as nvm
    from d2slam_amd.weights import synthetic_superpoint_weights
    from tests.helpers import bearings_ref as br
    prec = {"f32": api.PREC_F32, "f16x2": api.PREC_F16X2, "wino": api.PREC_F32_WINO, "f16": api.PREC_F16}[args.precision]
    fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=CAP, input_width=W, input_height=H, max_batch=1, precision=prec))
    fe.load_superpoint(synthetic_superpoint_weights(dustbin_bias=7.5)); fe.load_netvlad(nvm.synthetic_netvlad_weights())
    cam_l = br.pinhole(385.0, 386.0, 322.5, 241.0, 0.01, -0.02, 0.001, -0.0005)
    cam_r = br.pinhole(384.0, 385.5, 320.0, 242.0, -0.015, 0.01, -0.0005, 0.001)
    T = br.relative_extrinsic([1, 0, 0, 0], [0, 0, 0], br.quat_axis_angle([0.1, 1, 0.05], 1.0), [0.1, 0.004, -0.002]).reshape(-1)
    radius = 0.08 * W
    pin = lambda c: api.camera_pinhole(*[c[k] for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2")])
    bearings = dict(cam_left=pin(cam_l), cam_right=pin(cam_r), T_right_left=T, distance=100.0, lk_use_pred=True, radius_lk=radius)

    def host_composition(o, F):
        """the caller's per-point pass on one waited result: bearings of the keypoints, of the list entries and of their right tracks, predictions, the gate"""
        kept = 0
        for f in range(F):
            n, m = int(o["n_kp"][f]), int(o["track_n"][f])
            kb = br.bearings(cam_l, o["kps_xy"][f, :n]); br.predict(cam_l, T, kb, 100.0)
            lb = br.bearings(cam_l, o["track_pts"][f, :m]); br.bearings(cam_r, o["track_right_pts"][f, :m])
            kept += int(br.gate(br.predict(cam_l, T, lb, 100.0), o["track_right_pts"][f, :m], o["track_right_status"][f, :m], radius).sum())
        return kept

    def one(F, lanes, steps, warmup, host, mode, profile=False):
        """frames/s of `steps` submits with `lanes` in flight on a fresh pipe (profile: the per-stage HIP-event times of the same window instead)"""
        pipe = api.StereoPipe(fe, lanes=lanes, frames=F, width=W, height=H, cap=CAP, netvlad=True, match_lr=False, match_prev=True, ratio=0.8, pinned_input=True, lr_lk=True,
                              sp_lk=True, bearings=bearings if mode == "B" else None)
        base, per_set = host.data_ptr(), 2 * F * H * W        # [2 sets][L | R][F][H][W]
        kept = [0]

        def collect(t):
            if mode == "C":
                kept[0] += host_composition(pipe.wait(t), F)
            else:
                pipe.wait_raw(t)
                if mode == "B":
                    pipe.bearings_result_raw(t)

        def drive(n):
            tk = []
            for i in range(n):
                if i >= lanes:
                    collect(tk[i - lanes])
                o = base + (i & 1) * per_set
                tk.append(pipe.submit_ptr(o, o + F * H * W))
            for t in tk[-lanes:]:
                collect(t)
            return tk
        drive(warmup + (warmup & 1))
        torch.cuda.synchronize()
        if profile:
            pipe.profile_enable(2)
        t0 = time.perf_counter()
        tk = drive(steps)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if profile:
            prof = pipe.profile_read()
            pipe.profile_enable(0)
            pipe.close()
            return {k: {"ms_per_pass": round(ms / steps, 4), "launches_per_pass": n / steps} for k, (ms, n) in prof.items() if n}
        o = pipe.wait(tk[-1])
        one.last = {"avg_kp": round(float(o["n_kp"][:F].mean()), 1), "avg_list_entries": round(float(o["track_n"].mean()), 1),
                    "avg_right_tracked": round(float(np.mean([o["track_right_status"][f, :int(o["track_n"][f])].sum() for f in range(F)])), 1)}
        if mode == "B":
            one.last["avg_gate_kept"] = round(float(o["bearing_list_pred_ok"].sum(1).mean()), 1)
        pipe.close()
        return F * steps / dt

    modes = ("A", "B", "C")
    res = {"geometry": {"height": H, "width": W, "cap": CAP, "precision": args.precision, "netvlad": True, "lr_lk": True, "sp_lk": True, "match_prev": True, "pinned_input": True},
           "A": "lr_lk + sp_lk pipe", "B": "A with d2fe_pipe_bearings_enable", "C": "A plus the NumPy lift, prediction and gate on every waited result", "unit": "frames/s",
           "points": []}
    for name, F, lanes, steps, warmup in (("32 frames per submit, 4 submits in flight", 32, 4, 20, 4), ("1 frame per submit, 4 lanes, 4 in flight", 1, 4, 600, 16)):
        host = torch.from_numpy(pipe_frames(F, 0)).pin_memory()
        fps = {m: [] for m in modes}
        what = {}
        for m in modes:                                                  # warm-up round: module loads, allocator
            one(F, lanes, max(steps // 4, 8), warmup, host, m)
        for _ in range(max(args.rounds, 5)):
            for m in modes:
                fps[m].append(one(F, lanes, steps, warmup, host, m))
                what[m] = one.last
        med = {m: statistics.median(v) for m, v in fps.items()}
        rec = {"point": name, "frames": F, "lanes": lanes, "submits_per_round": steps, "rounds": len(fps["A"])}
        for m in modes:
            rec[m + "_fps_median"] = round(med[m], 1); rec[m + "_min_max"] = [round(min(fps[m]), 1), round(max(fps[m]), 1)]; rec[m + "_results"] = what[m]
        rec["B_over_A"] = round(med["B"] / med["A"], 3); rec["B_over_C"] = round(med["B"] / med["C"], 3)
        rec["B_range_overlaps_A_range"] = bool(max(fps["B"]) >= min(fps["A"]) and max(fps["A"]) >= min(fps["B"]))
        pa, pb = (one(F, lanes, steps, warmup, host, m, profile=True).get("lk") for m in ("A", "B"))
        rec["A_stage_lk"], rec["B_stage_lk"] = pa, pb
        if pa and pb:
            rec["bearings_launch_ms_per_pass"] = round(pb["ms_per_pass"] - pa["ms_per_pass"], 4)
            rec["bearings_launches_per_pass"] = round(pb["launches_per_pass"] - pa["launches_per_pass"], 3)
        rec["bearings_launch_note"] = ("HIP events around every launch of stage `lk` on the lanes' streams (profile mode 2), B minus A: wall time beside the other lanes' "
                                       "launches, per pass; the difference of two sums, so it carries both runs' noise")
        res["points"].append(rec)
        print(json.dumps(rec), flush=True)
    fe.close()
    print(json.dumps({"bench_pipe_bearings": res}))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
