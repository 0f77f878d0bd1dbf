#!/usr/bin/env python3
"""What D2FE_PREC_I8 delivers: the stereo pipe in ONE process, rounds alternating A, B, C, A, B, C, ...:
  A  D2FE_PREC_F16          (fp16 operands, fp32 accumulation: the fastest mode so far)
  B  D2FE_PREC_I8           (int8 operands, int32 accumulation; ranges from calibrate.measure_ranges on eight synthetic 640x480 frames)
  C  D2FE_PREC_F32_WINO     (bench.py's `value` mode)
All three as bench.py sets the pipe up (the protocol of tools/bench_f16.py): 640x480, 200 keypoints, NetVLAD of the left images, both matches, frames from pinned
host memory, every result back in pinned host memory inside the timed window, the same synthetic frames and seeded weights.  Two operating points: 32 stereo
frames per submit with four submits in flight, and one frame per submit on four lanes with four in flight.  Prints (and writes to --out) one JSON object: stereo
frames/s medians, the min..max of each, B/A and B/C with their ranges, and whether B's range lies above A's.  No threshold: a measurement.
Usage: python tools/bench_i8.py [--rounds 5] [--out profiles/i8.json]
       rocprofv3 --kernel-trace --stats ... -- python tools/bench_i8.py --trace-b 32      (B alone at F frames per submit, for a kernel trace; no JSON file)"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "i8.json"))
    ap.add_argument("--trace-b", type=int, default=0, help="run only B at this many stereo frames per submit (four lanes, four in flight) and print its frames/s")
    args = ap.parse_args()
    import numpy as np
    import torch
    from benchlib.common import CAP, H, W
    from benchlib.pipe_legs import pipe_frames
    from d2slam_amd import api, calibrate, netvlad as nvm
    from d2slam_amd.synth import synth_stereo
    from d2slam_amd.weights import synthetic_superpoint_weights
    w, nv = synthetic_superpoint_weights(dustbin_bias=7.5), nvm.synthetic_netvlad_weights()
    ranges = calibrate.measure_ranges(w, np.stack([f for s in range(4) for f in synth_stereo(H, W, seed=900 + s)]))

    PREC = {"A": api.PREC_F16, "B": api.PREC_I8, "C": api.PREC_F32_WINO}

    def frontend(mode):
        fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=CAP, input_width=W, input_height=H, max_batch=1, precision=PREC[mode]))
        fe.load_superpoint(w); fe.load_netvlad(nv)
        if mode == "B":
            fe.set_int8_ranges(ranges)
        return fe
    fes = {m: frontend(m) for m in (("B",) if args.trace_b else ("A", "B", "C"))}

    def one(F, lanes, steps, warmup, host, mode):
        """stereo frames/s of `steps` submits with `lanes` in flight on a fresh pipe"""
        fe = fes[mode]
        pipe = api.StereoPipe(fe, lanes=lanes, frames=F, width=W, height=H, cap=CAP, netvlad=True, match_prev=True, ratio=0.8, pinned_input=True)
        base, per_set, per_side = host.data_ptr(), 2 * F * H * W, F * H * W

        def drive(n):
            tk = []
            for i in range(n):
                if i >= lanes:
                    pipe.wait_raw(tk[i - lanes])
                o = base + (i & 1) * per_set
                tk.append(pipe.submit_ptr(o, o + per_side))
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
        one.last = {"avg_kp": round(float(o["n_kp"].mean()), 1), "avg_lr_matches": round(float(o["lr_n"].mean()), 1)}
        pipe.close()
        return F * steps / dt

    if args.trace_b:
        F = args.trace_b
        host = torch.from_numpy(pipe_frames(F, 0)).pin_memory()
        print(json.dumps({"B_stereo_fps": round(one(F, 4, max(20, 600 // F), 16 if F == 1 else 4, host, "B"), 1), "frames": F, "lanes": 4, "B_results": one.last}))
        for fe in fes.values():
            fe.close()
        return
    res = {"geometry": {"height": H, "width": W, "cap": CAP, "netvlad": True, "match_lr": True, "match_prev": True, "pinned_input": True},
           "A": "D2FE_PREC_F16", "B": "D2FE_PREC_I8", "C": "D2FE_PREC_F32_WINO", "int8_ranges": ranges, "points": []}
    for name, F, lanes, steps, warmup in (("32 stereo frames per submit, 4 submits in flight", 32, 4, 20, 4), ("1 stereo frame per submit, 4 lanes, 4 in flight", 1, 4, 600, 16)):
        host = torch.from_numpy(pipe_frames(F, 0)).pin_memory()
        fps = {"A": [], "B": [], "C": []}
        what = {}
        for m in fps:
            one(F, lanes, max(steps // 4, 8), warmup, host, m)          # warm-up round: module loads, allocator
        for _ in range(max(args.rounds, 3)):
            for m in fps:
                fps[m].append(one(F, lanes, steps, warmup, host, m))
                what[m] = one.last
        med = {m: statistics.median(v) for m, v in fps.items()}
        rec = {"point": name, "frames": F, "lanes": lanes, "submits_per_round": steps, "rounds": len(fps["A"])}
        for m in fps:
            rec[m + "_stereo_fps_median"] = round(med[m], 1); rec[m + "_min_max"] = [round(min(fps[m]), 1), round(max(fps[m]), 1)]
            rec[m + "_results"] = what[m]
        rec["B_over_A"] = round(med["B"] / med["A"], 3); rec["B_over_A_range"] = [round(min(fps["B"]) / max(fps["A"]), 3), round(max(fps["B"]) / min(fps["A"]), 3)]
        rec["B_over_C"] = round(med["B"] / med["C"], 3); rec["B_over_C_range"] = [round(min(fps["B"]) / max(fps["C"]), 3), round(max(fps["B"]) / min(fps["C"]), 3)]
        rec["B_above_A"] = bool(min(fps["B"]) > max(fps["A"]))
        res["points"].append(rec)
        print(json.dumps(rec), flush=True)
    for fe in fes.values():
        fe.close()
    print(json.dumps({"bench_i8": res}))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
