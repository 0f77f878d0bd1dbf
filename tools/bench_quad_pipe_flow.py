#!/usr/bin/env python3
"""The quad pipe's flow_lk mode (d2fe_quad_flow_enable) against the same quad pipe without it, in ONE process, rounds alternating A, B, C, A, B, C, ...:
  A  the quad pipe as bench.py's quadcam leg sets it up, without the mode
  B  the same pipe with the mode: pyramids of the 4 Q views, ONE d2fe_lk_flow_quad_step_device (five launches) per quad frame chained across submits and lanes, ONE
     d2fe_lk_flow_neighbour_device; reference default parameters (150 features, 20 px, 5 px, FAST 3 x 4 regions at threshold 10)
  C  B with the chain composed from four d2fe_lk_flow_step_device calls (twenty launches) per quad frame instead of the fused step (D2FE_QUAD_FLOW_SPLIT of the
     development library, read by d2fe_quad_flow_enable: a measurement switch, not a product option; the same bits)
All on the development library, at the settings of tools/bench_quad_pipe.py: 4 x 1280x800 raw fisheye frames -> 800x400 views through the seeded maps, 100 keypoints,
threshold 0.15, NetVLAD of every view, keypoint neighbour and temporal matches on, raw frames from pinned host memory, every result back in pinned host memory inside
the timed window.  Two operating points on four lanes: one and four quad frames per submit.  Prints (and writes to --out) one JSON object: quad frames/s medians and
min..max of each, B/A, C/A, B/C, and what the lists held (with 100 keypoints beside 150 features a view detects only while its flow list holds fewer than 13
entries: the timed window is the steady state, in which launches 2-5 of a step return at once -- `detecting` is the share of lists whose `num` is > 0).
Usage: python tools/bench_quad_pipe_flow.py [--rounds 5] [--out profiles/quad_pipe_flow.json]
       rocprofv3 --kernel-trace --stats ... -- python tools/bench_quad_pipe_flow.py --trace 4      (B alone at Q quad frames per submit, for a kernel trace; no
       alternation, no JSON file)"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RH, RW, UH, UW, CAP = 800, 1280, 400, 800, 100


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quad_pipe_flow.json"))
    ap.add_argument("--trace", type=int, default=0, help="run only B at this many quad frames per submit (four lanes) and print its quad frames/s")
    args = ap.parse_args()
    import torch
    from d2slam_amd import api, netvlad as nvm, quadcam
    from d2slam_amd.synth import synth_image
    from d2slam_amd.weights import synthetic_superpoint_weights
    w = dict(synthetic_superpoint_weights(dustbin_bias=7.5))
    Wt, b = w["convPb"]; b = b.copy(); b[64] -= np.float32(3.5); w["convPb"] = (Wt, b)
    fe = api.DevFrontEnd(api.SuperPointConfig(max_keypoints=CAP, input_width=UW, input_height=UH, max_batch=16, keypoint_threshold=0.15, precision=api.PREC_F32_WINO))
    fe.load_superpoint(w); fe.load_netvlad(nvm.synthetic_netvlad_weights())
    maps_h = [quadcam.synthetic_maps(c, RH, RW, UH, UW) for c in range(4)]
    NS = 8
    scenes = [synth_image(RH + 8, RW + 8, 40 + c) for c in range(4)]
    host = torch.empty((NS, 4, RH, RW), dtype=torch.uint8).pin_memory()
    hn = host.numpy()
    for s in range(NS):
        for c in range(4):
            hn[s, c] = scenes[c][s % 5:s % 5 + RH, (2 * s) % 7:(2 * s) % 7 + RW]
    per = 4 * RH * RW

    def one(mode, K, Q):
        os.environ["D2FE_QUAD_FLOW_SPLIT"] = "1" if mode == "C" else "0"
        pipe = api.QuadPipe(fe, maps_h, lanes=K, quads=Q, raw_width=RW, raw_height=RH, width=UW, height=UH, cap=CAP, pinned_input=True, flow_lk=mode != "A")
        nsets = NS // Q
        submit = lambda i: pipe.submit_ptr(host.data_ptr() + (i % nsets) * Q * per)
        tk = [submit(i) for i in range(K)]
        for i in range(K, 3 * K + 2):
            pipe.wait_raw(tk[i - K]); tk.append(submit(i))
        for t in tk[-K:]:
            pipe.wait_raw(t)
        steps = max(4 * K, int(args.seconds * 1000 / Q))
        tk = []
        t0 = time.perf_counter()
        for i in range(steps):
            if i >= K:
                pipe.wait_raw(tk[i - K])
            tk.append(submit(i))
        for t in tk[-K:]:
            pipe.wait_raw(t)
        dt = time.perf_counter() - t0
        o = pipe.wait(tk[-1])
        one.last = {"avg_kp": round(float(o["n_kp"].mean()), 1), "avg_nb_matches": round(float(o["nb_n"].mean()), 1)}
        if mode != "A":
            one.last.update(avg_list=round(float(o["flow_n"].mean()), 1), avg_tracked_in=round(float(o["flow_n_tracked_in"].mean()), 1),
                            avg_lost=round(float(o["flow_n_lost"].mean()), 1), avg_new=round(float(o["flow_n_new"].mean()), 1),
                            detecting=round(float((o["flow_num"] > 0).mean()), 2), avg_nb_lk_tracked=round(float(o["flow_nb_lk_status"].sum(-1).mean()), 1))
        pipe.close()
        return steps * Q / dt

    if args.trace:
        print(json.dumps({"B_quad_fps": round(one("B", 4, args.trace), 1), "quads": args.trace, "lanes": 4}))
        fe.close()
        return
    res = {"geometry": {"raw": [RH, RW], "view": [UH, UW], "cap": CAP, "threshold": 0.15, "precision": "wino", "netvlad": True, "lanes": 4},
           "A": "the quad pipe without the mode", "B": "d2fe_quad_flow_enable, reference default parameters: ONE fused step (five launches) per quad frame",
           "C": "B with four single-camera steps (twenty launches) per quad frame (D2FE_QUAD_FLOW_SPLIT, development library)", "points": []}
    for Q in (1, 4):
        fps = {"A": [], "B": [], "C": []}
        what = {}
        for m in fps:
            one(m, 4, Q)                                    # warm-up round: module loads, allocator
        for _ in range(max(args.rounds, 5)):
            for m in fps:
                fps[m].append(one(m, 4, Q))
                what[m] = one.last
        med = {m: statistics.median(v) for m, v in fps.items()}
        rec = {"quads": Q, "lanes": 4, "rounds": len(fps["A"])}
        for m in fps:
            rec[m + "_quad_fps_median"] = round(med[m], 1); rec[m + "_min_max"] = [round(min(fps[m]), 1), round(max(fps[m]), 1)]
            rec[m + "_ms_per_quad_frame"] = round(1e3 / med[m], 4); rec[m + "_results"] = what[m]
        rec["B_over_A"] = round(med["B"] / med["A"], 3); rec["C_over_A"] = round(med["C"] / med["A"], 3); rec["B_over_C"] = round(med["B"] / med["C"], 3)
        res["points"].append(rec)
        print(json.dumps(rec), flush=True)
    fe.close()
    print(json.dumps({"bench_quad_pipe_flow": res}))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
