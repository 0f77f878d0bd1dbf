#!/usr/bin/env python3
"""The stereo pipe's lr_lk mode against the same pipe with SuperPoint on both images, in ONE process, rounds alternating A, B, A, B, ...:
  A  lr_lk = 0, match_lr = 1: SuperPoint on the 2F images, matchKNN L <-> R (the non-default stereo path of the reference)
  B  lr_lk = 1:               SuperPoint on the F left images, pyramids of both, every left keypoint tracked left -> right with LK (lr_match_use_lk, its default)
Both as benchlib/pipe_legs.py sets the pipe up for bench.py's `value`: 640x480, 200 keypoints, NetVLAD of the left images, the temporal match, frames from pinned host
memory, every result back in pinned host memory inside the timed window, the same synthetic frames and seeded weights.  Two operating points: 32 stereo frames per
submit with four submits in flight, and one frame per submit on four lanes with four in flight.  Prints (and writes to --out) one JSON object: stereo frames/s medians,
the min..max of each, B/A, whether B's median is above A's by more than the larger spread, and B's per-stage d2fe_pipe_profile_read times.
Usage: python tools/bench_pipe_lk.py [--rounds 5] [--precision wino] [--out profiles/pipe_lr_lk.json]
       rocprofv3 --kernel-trace --stats ... -- python tools/bench_pipe_lk.py --trace-b 1      (B alone at F frames per submit, for a kernel trace: no alternation, no JSON file)"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pipe_lr_lk.json"))
    ap.add_argument("--trace-b", type=int, default=0, help="run only B at this many stereo frames per submit (four lanes, four in flight) and print its frames/s")
    args = ap.parse_args()
    import torch
    from benchlib.common import CAP, H, W
    from benchlib.pipe_legs import pipe_frames
    from d2slam_amd import api, netvlad as nvm
    from d2slam_amd.weights import synthetic_superpoint_weights
    prec = {"f32": api.PREC_F32, "f16x2": api.PREC_F16X2, "wino": api.PREC_F32_WINO, "f16": api.PREC_F16}[args.precision]
    fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=CAP, input_width=W, input_height=H, max_batch=1, precision=prec))
    fe.load_superpoint(synthetic_superpoint_weights(dustbin_bias=7.5)); fe.load_netvlad(nvm.synthetic_netvlad_weights())
    modes = {"A": dict(lr_lk=False, match_lr=True), "B": dict(lr_lk=True, match_lr=False)}

    def one(F, lanes, steps, warmup, host, mode, profile=False):
        """stereo frames/s of `steps` submits with `lanes` in flight on a fresh pipe (profile: the per-stage HIP-event times of the same window instead)"""
        pipe = api.StereoPipe(fe, lanes=lanes, frames=F, width=W, height=H, cap=CAP, netvlad=True, match_prev=True, ratio=0.8, pinned_input=True, **modes[mode])
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
        if profile:
            pipe.profile_enable(2)
        t0 = time.perf_counter()
        tk = drive(steps)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out = F * steps / dt
        if profile:
            prof = pipe.profile_read()
            pipe.profile_enable(0)
            out = {k: {"ms_per_pass": round(ms / steps, 4), "launches_per_pass": n / steps} for k, (ms, n) in prof.items() if n}
        else:
            o = pipe.wait(tk[-1])
            one.last = {"avg_kp_left": round(float(o["n_kp"][:F].mean()), 1), "avg_prev_matches": round(float(o["prev_n"].mean()), 1)}
            if mode == "B":
                one.last["avg_lk_tracked"] = round(float(o["lk_status"].sum(1).mean()), 1)
            else:
                one.last["avg_lr_matches"] = round(float(o["lr_n"].mean()), 1)
        pipe.close()
        return out

    if args.trace_b:
        F = args.trace_b
        host = torch.from_numpy(pipe_frames(F, 0)).pin_memory()
        print(json.dumps({"B_stereo_fps": round(one(F, 4, max(20, 600 // F), 16 if F == 1 else 4, host, "B"), 1), "frames": F, "lanes": 4}))
        fe.close()
        return
    res = {"geometry": {"height": H, "width": W, "cap": CAP, "precision": args.precision, "netvlad": True, "match_prev": True, "pinned_input": True},
           "A": "lr_lk = 0, match_lr = 1 (SuperPoint on both images, matchKNN L <-> R)", "B": "lr_lk = 1 (SuperPoint on the left image, LK left -> right)", "points": []}
    for name, F, lanes, steps, warmup in (("32 stereo frames per submit, 4 submits in flight", 32, 4, 20, 4), ("1 stereo frame per submit, 4 lanes, 4 in flight", 1, 4, 600, 16)):
        host = torch.from_numpy(pipe_frames(F, 0)).pin_memory()
        fps = {"A": [], "B": []}
        what = {}
        one(F, lanes, max(steps // 4, 8), warmup, host, "A"); one(F, lanes, max(steps // 4, 8), warmup, host, "B")          # warm-up round: module loads, allocator
        for _ in range(max(args.rounds, 5)):
            for m in ("A", "B"):
                fps[m].append(one(F, lanes, steps, warmup, host, m))
                what[m] = one.last
        med = {m: statistics.median(v) for m, v in fps.items()}
        spread = {m: max(v) - min(v) for m, v in fps.items()}
        rec = {"point": name, "frames": F, "lanes": lanes, "submits_per_round": steps, "rounds": len(fps["A"]),
               "A_stereo_fps_median": round(med["A"], 1), "A_min_max": [round(min(fps["A"]), 1), round(max(fps["A"]), 1)],
               "B_stereo_fps_median": round(med["B"], 1), "B_min_max": [round(min(fps["B"]), 1), round(max(fps["B"]), 1)],
               "B_over_A": round(med["B"] / med["A"], 3), "larger_spread": round(max(spread.values()), 1),
               "B_above_A_by_more_than_the_larger_spread": bool(med["B"] - med["A"] > max(spread.values())),
               "A_results": what["A"], "B_results": what["B"],
               "B_stages": one(F, lanes, steps, warmup, host, "B", profile=True),
               "B_stages_note": "HIP events around every stage on the lanes' streams (profile mode 2, which serialises nothing but adds two event records per stage): wall time "
                                "of the stage beside the other lanes' launches, summed over lanes, per pass; stage lk = the LK launches (pyramid levels + track)"}
        res["points"].append(rec)
        print(json.dumps(rec), flush=True)
    fe.close()
    print(json.dumps({"bench_pipe_lk": res}))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
