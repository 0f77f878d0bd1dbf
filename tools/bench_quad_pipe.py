#!/usr/bin/env python3
"""Quadcam frames in flight (d2fe_quad_pipe_*, include/d2fe.h) against the Python-sequenced QuadcamChain, in one process, at the settings of bench.py's quadcam
leg: 4 x 1280x800 raw fisheye frames -> 800x400 views through the seeded quadcam.synthetic_maps (photometric gain on), 100 keypoints, threshold 0.15, NetVLAD
of every view, neighbour pairs with the radius 0.2 * 800, temporal pairs.
  pipe       quad frames/s for lanes x quads per submit: raw frames from pinned host memory, the H2D and the D2H of every result inside the timed window
  chain      QuadcamChain.step with the raw frames already in HBM, one stream (what bench.py --workload quadcam times)
  undistort  the pipe's one-launch undistort (quad_undistort_kernel, d2fe_quad_undistort_device) against the chain's four undistort_kernel launches:
             HIP-event time per pass (alternating A/B windows, best of three) and the HBM bytes each has to move, over the 8 TB/s peak
Usage: python tools/bench_quad_pipe.py [--sweep 1x1,2x1,4x1,...] [--seconds 1.0] [--out FILE]      (LxQ = lanes x quad frames per submit)"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
RH, RW, UH, UW, CAP = 800, 1280, 400, 800, 100
HBM_PEAK = 8.0e12          # B/s, MI355X spec (6.29e12 measured with a float4 copy, MI355X_MICROARCH)


def undistort_bytes(Q, gain=True):
    """HBM bytes a pass must move.  One launch: the maps once, the raw frames once (the taps of neighbouring pixels share cache lines; the maps reach most
    of the frame), 1 B per view pixel out.  Four launches: every image of a launch reads its camera's maps again."""
    npix, m = UH * UW, (12 if gain else 8)
    one = 4 * npix * m + Q * 4 * (RH * RW + npix)
    four = 4 * Q * (npix * m + RH * RW + npix)
    return one, four


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweep", default="1x1,2x1,4x1,1x2,2x2,4x2,1x4,2x4,4x4")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--precision", default="wino")
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-chain", action="store_true")
    ap.add_argument("--skip-undistort", action="store_true")
    args = ap.parse_args()
    import torch
    from d2slam_amd import api, netvlad as nvm, quadcam
    from d2slam_amd.synth import synth_image
    from d2slam_amd.weights import synthetic_superpoint_weights
    prec = {"f32": api.PREC_F32, "f16x2": api.PREC_F16X2, "wino": api.PREC_F32_WINO, "f16": api.PREC_F16}[args.precision]
    sweep = [tuple(int(x) for x in p.split("x")) for p in args.sweep.split(",")]
    qs = sorted({q for _, q in sweep})
    w = dict(synthetic_superpoint_weights(dustbin_bias=7.5))
    Wt, b = w["convPb"]; b = b.copy(); b[64] -= np.float32(3.5); w["convPb"] = (Wt, b)      # as bench.py's quadcam leg: threshold 0.15 finds keypoints
    fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=CAP, input_width=UW, input_height=UH, max_batch=4 * max(qs), keypoint_threshold=0.15, precision=prec))
    fe.load_superpoint(w); fe.load_netvlad(nvm.synthetic_netvlad_weights())
    maps_h = [quadcam.synthetic_maps(c, RH, RW, UH, UW) for c in range(4)]
    NS = 8                                                                  # distinct quad frames the submits cycle through
    scenes = [synth_image(RH + 8, RW + 8, 40 + c) for c in range(4)]
    host = torch.empty((NS, 4, RH, RW), dtype=torch.uint8).pin_memory()
    hn = host.numpy()
    for s in range(NS):
        for c in range(4):
            hn[s, c] = scenes[c][s % 5:s % 5 + RH, (2 * s) % 7:(2 * s) % 7 + RW]
    res = {"geometry": {"raw": [RH, RW], "view": [UH, UW], "cap": CAP, "threshold": 0.15, "precision": args.precision}, "pipe": [], "chain": [], "undistort": []}

    def emit(key, rec):
        res[key].append(rec)
        print(json.dumps({key: rec}), flush=True)

    dev = torch.device("cuda", 0)
    per = 4 * RH * RW
    for K, Q in sweep:
        pipe = api.QuadPipe(fe, maps_h, lanes=K, quads=Q, raw_width=RW, raw_height=RH, width=UW, height=UH, cap=CAP, pinned_input=True)
        nsets = NS // Q
        submit = lambda i: pipe.submit_ptr(host.data_ptr() + (i % nsets) * Q * per)
        tk = [submit(i) for i in range(K)]                                  # warm-up: every lane's pass shape, twice
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
        emit("pipe", {"lanes": K, "quads": Q, "quad_fps": round(steps * Q / dt, 1), "ms_per_submit": round(dt / steps * 1e3, 3), "submits": steps,
                      "avg_kp": round(float(o["n_kp"].mean()), 1), "avg_nb_matches": round(float(o["nb_n"].mean()), 1), "avg_prev_matches": round(float(o["prev_n"].mean()), 1)})
        pipe.close()
    maps_d = [tuple(torch.from_numpy(m).to(dev) for m in mm) for mm in maps_h]
    st = torch.cuda.Stream(device=dev)
    if not args.skip_chain:
        for Q in qs:
            raw = torch.from_numpy(np.ascontiguousarray(hn[:Q].transpose(1, 0, 2, 3).reshape(4 * Q, RH, RW))).to(dev)     # the chain is camera-major
            chain = quadcam.QuadcamChain(fe, torch, dev, Q, UH, UW, CAP, undistort_fov=200.0, knn_ratio=0.8, search_local_max_dist=0.2)
            torch.cuda.synchronize()
            with torch.cuda.stream(st):
                for _ in range(5):
                    chain.step(raw, RH, RW, maps_d, st.cuda_stream)
                torch.cuda.synchronize()
                steps = max(10, int(args.seconds * 900 / Q))
                t0 = time.perf_counter()
                for _ in range(steps):
                    chain.step(raw, RH, RW, maps_d, st.cuda_stream)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
            emit("chain", {"quads": Q, "quad_fps": round(steps * Q / dt, 1), "ms_per_step": round(dt / steps * 1e3, 3), "steps": steps})
    if not args.skip_undistort:
        sp = st.cuda_stream
        ptrs = [(mx.data_ptr(), my.data_ptr(), g.data_ptr()) for mx, my, g in maps_d]
        for Q in (1, 2, 4):
            raw = torch.from_numpy(np.ascontiguousarray(hn[:Q])).to(dev)                        # quad-major [Q][4][RH][RW]
            one_out = torch.empty((Q, 4, UH, UW), dtype=torch.uint8, device=dev)
            four_out = torch.empty((4, Q, UH, UW), dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()

            def one():
                fe.quad_undistort_device(raw.data_ptr(), Q, RW, RH, ptrs, UW, UH, one_out.data_ptr(), stream=sp)

            def four():
                for c in range(4):
                    fe.undistort_device(raw.data_ptr() + c * RH * RW, Q, RW, RH, *ptrs[c], UW, UH, four_out[c].data_ptr(), stream=sp, src_image_stride=4 * RH * RW)
            one(); four(); torch.cuda.synchronize()
            assert torch.equal(one_out.permute(1, 0, 2, 3), four_out), "the one-launch undistort differs from the four launches"
            N = 200
            best = {"one_launch": 1e9, "four_launches": 1e9}
            for _ in range(3):                                                                   # alternating windows
                for name, fn in (("one_launch", one), ("four_launches", four)):
                    for _ in range(10):
                        fn()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(st)
                    for _ in range(N):
                        fn()
                    e1.record(st); e1.synchronize()
                    best[name] = min(best[name], e0.elapsed_time(e1) / N)
            b1, b4 = undistort_bytes(Q)
            emit("undistort", {"quads": Q, "one_launch_us": round(best["one_launch"] * 1e3, 2), "four_launches_us": round(best["four_launches"] * 1e3, 2),
                               "one_launch_bytes": b1, "four_launches_bytes": b4,
                               "one_launch_frac_hbm_peak": round(b1 / (best["one_launch"] * 1e-3) / HBM_PEAK, 3),
                               "four_launches_frac_hbm_peak": round(b4 / (best["four_launches"] * 1e-3) / HBM_PEAK, 3)})
    fe.close()
    print(json.dumps({"bench_quad_pipe": res}))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
