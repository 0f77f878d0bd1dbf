#!/usr/bin/env python3
"""The flow landmarks in the pipes, in ONE process, rounds alternating A, B, C, D, A, B, ...:
  A  lr_lk = 1:                   SuperPoint on the F left images, pyramids of both, every left keypoint tracked left -> right (lr_match_use_lk)
  B  A + d2fe_pipe_flow_enable:   the same plus the flow landmarks beside SuperPoint (one d2fe_lk_flow_step_device per left frame, chained across passes and lanes,
                                  ONE left -> right launch over the flow entries); 100 keypoints against total_feature_num = 150, so that detection runs
  C  mono, flow only:             superpoint = 0 (gopro.yaml / visensor_f9p.yaml): no network, no matcher; pyramids and the chain
  D  the host composition of C:   per frame api.LKFrame + api.lk_track + removeNearPoints + api.detectPoints(use_fast) -- two stalls a frame, and its thinning and merge
                                  loops run in Python, so C/D overstates what a C++ caller of the host calls would gain
A and B as benchlib/pipe_legs.py sets the pipe up for bench.py's `value` (640x480, NetVLAD of the left images, the temporal match, frames from pinned host memory,
every result back in pinned host memory inside the timed window), with 100 keypoints; C without NetVLAD and matcher.  The frames of pipe_legs are unrelated images:
nearly every track is lost from frame to frame and every frame detects its list again -- the expensive case of the step.  Two operating points: 32 frames per submit
with four submits in flight, and one frame per submit on four lanes.  Prints (and writes to --out) one JSON object: frames/s medians with min..max, B/A and C/D.
Usage: python tools/bench_pipe_flow.py [--rounds 5] [--out profiles/pipe_flow.json]
       rocprofv3 --kernel-trace --stats ... -- python tools/bench_pipe_flow.py --trace-c 32      (C alone, for a kernel trace; no alternation, no JSON file)"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CAP_B = 100


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--precision", default="wino")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pipe_flow.json"))
    ap.add_argument("--trace-c", type=int, default=0, help="run only C at this many frames per submit (four lanes, four in flight) and print its frames/s")
    args = ap.parse_args()
    import numpy as np
    import torch
    from benchlib.common import H, W
    from benchlib.pipe_legs import pipe_frames
    from d2slam_amd import api, netvlad as nvm
    from d2slam_amd.weights import synthetic_superpoint_weights
    prec = {"f32": api.PREC_F32, "f16x2": api.PREC_F16X2, "wino": api.PREC_F32_WINO, "f16": api.PREC_F16}[args.precision]
    fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=CAP_B, input_width=W, input_height=H, max_batch=1, precision=prec))
    fe.load_superpoint(synthetic_superpoint_weights(dustbin_bias=7.5)); fe.load_netvlad(nvm.synthetic_netvlad_weights())
    modes = {"A": dict(lr_lk=True, netvlad=True, match_prev=True), "B": dict(lr_lk=True, netvlad=True, match_prev=True, flow_lk=True),
             "C": dict(mono=True, netvlad=False, match_prev=False, flow_lk="only")}

    def one(F, lanes, steps, warmup, host, mode):
        """frames/s of `steps` submits with `lanes` in flight on a fresh pipe"""
        pipe = api.StereoPipe(fe, lanes=lanes, frames=F, width=W, height=H, cap=CAP_B, match_lr=False, ratio=0.8, pinned_input=True, **modes[mode])
        base, per_set, per_side = host.data_ptr(), 2 * F * H * W, F * H * W

        def drive(n):
            tk = []
            for i in range(n):
                if i >= lanes:
                    pipe.wait_raw(tk[i - lanes])
                o = base + (i & 1) * per_set
                tk.append(pipe.submit_ptr(o, None if mode == "C" else o + per_side))
            for t in tk[-lanes:]:
                pipe.wait_raw(t)
            return tk
        drive(warmup + (warmup & 1))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tk = drive(steps)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        o = pipe.wait(tk[-1])
        one.last = {"avg_kp_left": round(float(o["n_kp"][:F].mean()), 1)}
        if mode != "A":
            one.last.update(avg_list=round(float(o["flow_n"].mean()), 1), avg_lost=round(float(o["flow_n_lost"].mean()), 1), avg_new=round(float(o["flow_n_new"].mean()), 1),
                            frames_that_detected=int((o["flow_num"] > 0).sum()))
        pipe.close()
        return F * steps / dt

    def host_leg(imgs, T=150):
        """D: the composition on the host, frame by frame"""
        prev, pts = None, np.zeros((0, 2), np.float32)
        t0 = time.perf_counter()
        for img in imgs:
            frame = api.LKFrame(fe, img, 2)
            if len(pts):
                q, ok = api.lk_track(fe, prev, frame, pts, pts)
                keep = []
                for p in q[ok != 0]:
                    if not any(np.hypot(*(p - k)) < 5.0 for k in keep):
                        keep.append(p)
                pts = np.asarray(keep, np.float32).reshape(-1, 2)
            new = api.detectPoints(fe, frame, pts, T, use_fast=True)
            pts = np.concatenate([pts, new]) if len(new) else pts
            if prev is not None:
                prev.close()
            prev = frame
        prev.close()
        return len(imgs) / (time.perf_counter() - t0)

    if args.trace_c:
        F = args.trace_c
        host = torch.from_numpy(pipe_frames(F, 0)).pin_memory()
        print(json.dumps({"C_fps": round(one(F, 4, max(20, 600 // F), 16 if F == 1 else 4, host, "C"), 1), "frames": F, "lanes": 4}))
        fe.close()
        return
    res = {"geometry": {"height": H, "width": W, "cap": CAP_B, "total_feature_num": 150, "precision": args.precision, "pinned_input": True},
           "A": "lr_lk = 1", "B": "lr_lk = 1 + flow landmarks beside SuperPoint", "C": "mono, flow only (superpoint = 0)", "D": "host composition of C (Python loops included)",
           "points": []}
    for name, F, lanes, steps, warmup in (("32 frames per submit, 4 submits in flight", 32, 4, 20, 4), ("1 frame per submit, 4 lanes, 4 in flight", 1, 4, 600, 16)):
        frames_np = pipe_frames(F, 0)
        host = torch.from_numpy(frames_np).pin_memory()
        lefts = frames_np[0, 0] if F > 1 else np.stack([frames_np[i & 1, 0, 0] for i in range(32)])      # D sees the left frames the pipe sees, in its order
        fps = {m: [] for m in "ABCD"}
        what = {}
        for m in "ABC":
            one(F, lanes, max(steps // 4, 8), warmup, host, m)          # warm-up round: module loads, allocator
        host_leg(lefts[:4])
        for _ in range(max(args.rounds, 5)):
            for m in "ABC":
                fps[m].append(one(F, lanes, steps, warmup, host, m))
                what[m] = one.last
            fps["D"].append(host_leg(lefts))
        med = {m: statistics.median(v) for m, v in fps.items()}
        rec = {"point": name, "frames": F, "lanes": lanes, "submits_per_round": steps, "rounds": len(fps["A"])}
        for m in "ABCD":
            rec[m + "_fps_median"] = round(med[m], 1); rec[m + "_min_max"] = [round(min(fps[m]), 1), round(max(fps[m]), 1)]
        rec.update(B_over_A=round(med["B"] / med["A"], 3), C_over_D=round(med["C"] / med["D"], 2), C_above_D=bool(min(fps["C"]) > max(fps["D"])),
                   A_results=what["A"], B_results=what["B"], C_results=what["C"])
        res["points"].append(rec)
        print(json.dumps(rec), flush=True)
    fe.close()
    print(json.dumps({"bench_pipe_flow": res}))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
