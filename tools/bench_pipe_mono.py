#!/usr/bin/env python3
"""What a one-camera user pays, in ONE process, rounds alternating A, B, C, A, B, C, ...:
  A  the stereo pipe with match_lr = 0, lr_lk = 0 and a copy of the left image as right image: what such a user had to do before the mono mode (SuperPoint twice)
  B  mono = 1:            the one image per frame (the reference's MONOCULAR configuration)
  C  mono = 1, depth = 1: the one image and its 16-bit depth frame, the depth under every keypoint inside the pass (PINHOLE_DEPTH)
All three as benchlib/pipe_legs.py sets the pipe up for bench.py's `value`: 640x480, 200 keypoints, NetVLAD, the temporal match, frames from pinned host memory, every
result back in pinned host memory inside the timed window, the same synthetic frames and seeded weights.  Two operating points: 32 frames per submit with four submits
in flight, and one frame per submit on four lanes with four in flight.  Prints (and writes to --out) one JSON object: frames/s medians, the min..max of each, B/A,
C/B, and whether B's range lies above A's.
Usage: python tools/bench_pipe_mono.py [--rounds 5] [--precision wino] [--out profiles/pipe_mono.json]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pipe_mono.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from benchlib.common import CAP, H, W
    from benchlib.pipe_legs import pipe_frames
    from d2slam_amd import api, netvlad as nvm
    from d2slam_amd.weights import synthetic_superpoint_weights
    prec = {"f32": api.PREC_F32, "f16x2": api.PREC_F16X2, "wino": api.PREC_F32_WINO, "f16": api.PREC_F16}[args.precision]
    fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=CAP, input_width=W, input_height=H, max_batch=1, precision=prec))
    fe.load_superpoint(synthetic_superpoint_weights(dustbin_bias=7.5)); fe.load_netvlad(nvm.synthetic_netvlad_weights())
    modes = {"A": dict(), "B": dict(mono=True), "C": dict(mono=True, depth=True)}

    def one(F, lanes, steps, warmup, host, dep, mode, profile=False):
        """frames/s of `steps` submits with `lanes` in flight on a fresh pipe (profile: the per-stage HIP-event times of the same window instead)"""
        pipe = api.StereoPipe(fe, lanes=lanes, frames=F, width=W, height=H, cap=CAP, netvlad=True, match_lr=False, match_prev=True, ratio=0.8, pinned_input=True, **modes[mode])
        base, per_set = host.data_ptr(), 2 * F * H * W        # [2 sets][L | R][F][H][W]: the left half of a set is what every mode reads
        dbase, dper_set = dep.data_ptr(), 2 * F * H * W       # [2 sets][F][H][W] uint16

        def drive(n):
            tk = []
            for i in range(n):
                if i >= lanes:
                    pipe.wait_raw(tk[i - lanes])
                o = base + (i & 1) * per_set
                if mode == "A":
                    tk.append(pipe.submit_ptr(o, o))                     # the left images again as right images
                elif mode == "B":
                    tk.append(pipe.submit_ptr(o, None))
                else:
                    tk.append(pipe.submit_depth_ptr(o, dbase + (i & 1) * dper_set))
            for t in tk[-lanes:]:
                pipe.wait_raw(t)
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
        one.last = {"avg_kp": round(float(o["n_kp"][:F].mean()), 1), "avg_prev_matches": round(float(o["prev_n"].mean()), 1), "kp_right_rows": int(o["n_kp"][F:].sum())}
        if mode == "C":
            one.last["avg_nonzero_depths"] = round(float((o["kp_depth_mm"] != 0).sum(1).mean()), 1)
        pipe.close()
        return F * steps / dt

    res = {"geometry": {"height": H, "width": W, "cap": CAP, "precision": args.precision, "netvlad": True, "match_lr": False, "match_prev": True, "pinned_input": True},
           "A": "stereo pipe, match_lr = 0, lr_lk = 0, the left image again as right image", "B": "mono = 1", "C": "mono = 1, depth = 1", "unit": "frames/s", "points": []}
    for name, F, lanes, steps, warmup in (("32 frames per submit, 4 submits in flight", 32, 4, 20, 4), ("1 frame per submit, 4 lanes, 4 in flight", 1, 4, 600, 16)):
        host = torch.from_numpy(pipe_frames(F, 0)).pin_memory()
        dep = torch.from_numpy(np.random.RandomState(3).randint(0, 65536, (2, F, H, W)).astype(np.uint16).view(np.int16)).pin_memory()
        fps = {m: [] for m in modes}
        what = {}
        for m in modes:                                                  # warm-up round: module loads, allocator
            one(F, lanes, max(steps // 4, 8), warmup, host, dep, m)
        for _ in range(max(args.rounds, 5)):
            for m in modes:
                fps[m].append(one(F, lanes, steps, warmup, host, dep, m))
                what[m] = one.last
        med = {m: statistics.median(v) for m, v in fps.items()}
        rec = {"point": name, "frames": F, "lanes": lanes, "submits_per_round": steps, "rounds": len(fps["A"])}
        for m in modes:
            rec[m + "_fps_median"] = round(med[m], 1); rec[m + "_min_max"] = [round(min(fps[m]), 1), round(max(fps[m]), 1)]; rec[m + "_results"] = what[m]
        rec["B_over_A"] = round(med["B"] / med["A"], 3); rec["C_over_B"] = round(med["C"] / med["B"], 3)
        rec["B_range_above_A_range"] = bool(min(fps["B"]) > max(fps["A"]))
        rec["C_range_overlaps_B_range"] = bool(max(fps["C"]) >= min(fps["B"]) and max(fps["B"]) >= min(fps["C"]))
        # without sp_lk the depth lookup is the only launch of stage `lk` on a mono pipe
        rec["C_depth_gather_launch"] = one(F, lanes, steps, warmup, host, dep, "C", profile=True).get("lk")
        rec["C_depth_gather_launch_note"] = ("HIP events around the one depth_gather_kernel launch of a pass on the lane's stream (profile mode 2): wall time beside the other "
                                             "lanes' launches, per pass")
        res["points"].append(rec)
        print(json.dumps(rec), flush=True)
    fe.close()
    print(json.dumps({"bench_pipe_mono": res}))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
