#!/usr/bin/env python3
"""What exact_order costs: the stereo pipe in ONE process, rounds alternating A, B, C, A, B, C, ...:
  A  D2FE_PREC_F32_WINO                  (bench.py's `value` mode)
  B  D2FE_PREC_F32_WINO + exact_order    (default eps and crop slots unless --eps / --crops)
  C  D2FE_PREC_F32                       (the exact mode, whose keypoint lists B reproduces)
All three as the protocol of tools/bench_pipe_sp_lk.py sets the pipe up: 640x480, 200 keypoints, NetVLAD of the left images, both matches, frames from pinned host
memory, every result back in pinned host memory inside the timed window, the same synthetic frames and seeded weights.  Two operating points: 32 stereo frames per
submit with four submits in flight, and one frame per submit on four lanes with four in flight.  Prints (and writes to --out) one JSON object: stereo frames/s medians,
the min..max of each, B/A and B/C, and B's exact_order counters per call.
Usage: python tools/bench_exact_order.py [--rounds 5] [--out profiles/exact_order.json]
       rocprofv3 --kernel-trace --stats ... -- python tools/bench_exact_order.py --trace-b 32      (B alone at F frames per submit, for a kernel trace; no JSON file)"""
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
    ap.add_argument("--eps", type=float, default=0.0)
    ap.add_argument("--crops", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact_order.json"))
    ap.add_argument("--trace-b", type=int, default=0, help="run only B at this many stereo frames per submit (four lanes, four in flight) and print its frames/s")
    args = ap.parse_args()
    import torch
    from benchlib.common import CAP, H, W
    from benchlib.pipe_legs import pipe_frames
    from d2slam_amd import api, netvlad as nvm
    from d2slam_amd.weights import synthetic_superpoint_weights
    w, nv = synthetic_superpoint_weights(dustbin_bias=7.5), nvm.synthetic_netvlad_weights()

    def frontend(mode):
        eo = dict(exact_order=True, exact_order_eps=args.eps, exact_order_crops=args.crops) if mode == "B" else {}
        fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=CAP, input_width=W, input_height=H, max_batch=1, precision=api.PREC_F32 if mode == "C" else api.PREC_F32_WINO), **eo)
        fe.load_superpoint(w); fe.load_netvlad(nv)
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
        s0 = fe.exact_order_stats()
        t0 = time.perf_counter()
        tk = drive(steps)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        s1 = fe.exact_order_stats()
        o = pipe.wait(tk[-1])
        one.last = {"avg_kp": round(float(o["n_kp"].mean()), 1), "avg_lr_matches": round(float(o["lr_n"].mean()), 1)}
        if mode == "B":
            calls = max(s1["calls"] - s0["calls"], 1)
            one.last.update(marked_per_call=round((s1["marked"] - s0["marked"]) / calls, 1), cells_per_call=round((s1["cells"] - s0["cells"]) / calls, 1),
                            dropped=s1["dropped"] - s0["dropped"], images_per_call=2 * F)
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
           "A": "D2FE_PREC_F32_WINO", "B": "D2FE_PREC_F32_WINO + exact_order (eps %g, crop slots %s)" % (args.eps or 9e-6, args.crops or "default"), "C": "D2FE_PREC_F32",
           "points": []}
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
        rec["B_above_C"] = bool(min(fps["B"]) > max(fps["C"]))
        res["points"].append(rec)
        print(json.dumps(rec), flush=True)
    for fe in fes.values():
        fe.close()
    print(json.dumps({"bench_exact_order": res}))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
