#!/usr/bin/env python3
"""What the bearings mode of the quad pipe costs and what it replaces, in ONE process, rounds alternating A, B, C, A, B, C, ...:
  A  the quad pipe with flow_lk (the reference's main configuration, config/quadcam/quadcam_single.yaml): the caller still owes the per-point pass
  B  A with d2fe_quad_bearings_enable: bearings of the keypoints and list entries, neighbour predictions and the lk_lk_use_pred gate inside the pass, read with
     d2fe_quad_bearings_result_get
  C  A plus the host composition on every waited result: the NumPy lift, prediction and gate (vectorised np.tan / np.arctan2, the arithmetic of
     tests/helpers/cyl_bearings_ref.py) over the keypoints, the list entries and the neighbour tracks, standing in for the caller's loop (createLKLandmark /
     predictLandmarksWithExtrinsic / the gate of trackLK(left, right, type) in the tracker thread)
All three at the settings of tools/bench_quad_pipe_flow.py: 4 x 1280x800 raw fisheye frames -> 800x400 views through the seeded maps, 100 keypoints, threshold 0.15,
NetVLAD of every view, keypoint neighbour and temporal matches on, flow landmarks with the reference's default parameters, raw frames from pinned host memory, every
result back in pinned host memory inside the timed window.  Two operating points on four lanes: one and four quad frames per submit.  Prints (and writes to --out) one
JSON object: quad frames/s medians, the min..max of each, B/A, B/C, whether B's range overlaps A's and lies above C's; the time of the pass's arithmetic from HIP events
(the single-call form d2fe_bearings_device on the three segments of a pass, one after the other -- an upper bound of the pipe's ONE launch); and the observed maximum
error of the device's cylindrical bearings against the correctly rounded true value (mpmath, 200 bits) in units in the last place of the component.  Nothing is gated
on these numbers.
Usage: python tools/bench_quad_pipe_bearings.py [--rounds 5] [--out profiles/quad_pipe_bearings.json]"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RH, RW, UH, UW, CAP, FOV = 800, 1280, 400, 800, 100, 200.0
NEIGHBOURS = ((0, 1), (1, 2), (2, 3), (0, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quad_pipe_bearings.json"))
    args = ap.parse_args()
    import torch
    from d2slam_amd import api, netvlad as nvm, quadcam
    from d2slam_amd.synth import synth_image
    from d2slam_amd.weights import synthetic_superpoint_weights
    from tests.helpers import bearings_ref as br
    from tests.helpers import cyl_bearings_ref as cr
    w = dict(synthetic_superpoint_weights(dustbin_bias=7.5))
    Wt, b = w["convPb"]; b = b.copy(); b[64] -= np.float32(3.5); w["convPb"] = (Wt, b)
    fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=CAP, input_width=UW, input_height=UH, max_batch=16, keypoint_threshold=0.15, precision=api.PREC_F32_WINO))
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
    cam = cr.cylinder_camera(UW, UH, FOV)
    T_nb = np.stack([br.relative_extrinsic([1, 0, 0, 0], [0, 0, 0], br.quat_axis_angle([0, 1, 0], -90.0 if n < 3 else 90.0), [0.05, 0.0, 0.0]).reshape(-1) for n in range(4)])
    radius, distance = 0.2 * UW, 100.0
    bearings = dict(cams=[api.cylinder_camera(UW, UH, FOV)] * 4, T_nb=T_nb, distance=distance, lk_use_pred=True, radius_lk=radius)
    fx, fy, cx, cy = (np.float64(cam[k]) for k in ("fx", "fy", "cx", "cy"))

    def np_bearings(pts):
        p = np.asarray(pts, np.float32).reshape(-1, 2).astype(np.float64)
        with np.errstate(all="ignore"):
            phi = (1.0 / fx) * p[:, 0] + (-cx / fx); ybr = (1.0 / fy) * p[:, 1] + (-cy / fy)
            z = np.where(np.abs(phi) > math.pi / 2, -1.0, 1.0)
            x = z * np.tan(phi)
            y = ybr * np.sqrt(x * x + z * z)
            n = np.sqrt(x * x + y * y + z * z)
            return np.stack([x / n, y / n, z / n], 1)

    def np_predict(T, bb):
        with np.errstate(all="ignore"):
            X = br.transform(T, bb, distance)
            rho = np.sqrt(X[:, 0] * X[:, 0] + X[:, 2] * X[:, 2])
            a = rho * np.arctan2(X[:, 0], X[:, 2])
            return np.stack([((fx * a + cx * rho) / rho).astype(np.float32), ((fy * X[:, 1] + cy * rho) / rho).astype(np.float32)], 1)

    def host_composition(o, Q):
        """the caller's per-point pass on one waited result"""
        kept = 0
        for q in range(Q):
            lb = []
            for c in range(4):
                np_bearings(o["kps_xy"][q, c, :int(o["n_kp"][q, c])])
                lb.append(np_bearings(o["flow_pts"][q, c, :int(o["flow_n"][q, c])]))
            for n, (a, b_) in enumerate(NEIGHBOURS):
                m = int(o["flow_n"][q, a])
                np_bearings(o["flow_nb_lk_xy"][q, n, :m])
                kept += int(br.gate(np_predict(T_nb[n], lb[a]), o["flow_nb_lk_xy"][q, n, :m], o["flow_nb_lk_status"][q, n, :m], radius).sum())
        return kept

    def one(mode, K, Q):
        pipe = api.QuadPipe(fe, maps_h, lanes=K, quads=Q, raw_width=RW, raw_height=RH, width=UW, height=UH, cap=CAP, pinned_input=True, flow_lk=True,
                            bearings=bearings if mode == "B" else None)
        nsets = NS // Q
        submit = lambda i: pipe.submit_ptr(host.data_ptr() + (i % nsets) * Q * per)
        kept = [0]

        def collect(t):
            if mode == "C":
                kept[0] += host_composition(pipe.wait(t), Q)
            else:
                pipe.wait_raw(t)
                pipe.flow_result_raw(t)
                if mode == "B":
                    pipe.bearings_result_raw(t)

        def drive(n):
            tk = []
            for i in range(n):
                if i >= K:
                    collect(tk[i - K])
                tk.append(submit(i))
            for t in tk[-K:]:
                collect(t)
            return tk
        drive(3 * K + 2)
        steps = max(4 * K, int(args.seconds * 1000 / Q))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tk = drive(steps)
        dt = time.perf_counter() - t0
        o = pipe.wait(tk[-1])
        one.last = {"avg_kp": round(float(o["n_kp"].mean()), 1), "avg_list": round(float(o["flow_n"].mean()), 1),
                    "avg_nb_lk_tracked": round(float(o["flow_nb_lk_status"].sum(-1).mean()), 1)}
        if mode == "B":
            one.last["avg_gate_kept"] = round(float(o["bear_nb_pred_ok"].sum(-1).mean()), 1)
        if mode == "C":
            one.last["gate_kept_total"] = kept[0]
        one.shape = (o["flow_pts"].shape[2],)
        pipe.close()
        return steps * Q / dt

    def launch_time(Q, T):
        """HIP events around the three segments of a pass as three single calls (keypoint rows, lists, one neighbour pair's worth of gated lists for all 4 Q), median of 50"""
        dev = torch.device("cuda")
        st = torch.cuda.current_stream()
        rng = np.random.RandomState(3)
        NI = 4 * Q
        c = api.cylinder_camera(UW, UH, FOV)

        def pts(cap):
            return torch.from_numpy((rng.rand(NI, cap, 2) * [UW - 1, UH - 1]).astype(np.float32)).to(dev)
        kp, lp, op = pts(CAP), pts(T), pts(T)
        nk = torch.full((NI,), CAP, dtype=torch.int32, device=dev); nl = torch.full((NI,), T, dtype=torch.int32, device=dev)
        bk = torch.empty(NI * CAP * 3, dtype=torch.float64, device=dev); bl = torch.empty(NI * T * 3, dtype=torch.float64, device=dev); bo = torch.empty_like(bl)
        pr = torch.empty(NI * T * 2, dtype=torch.float32, device=dev); ok = torch.empty(NI * T, dtype=torch.uint8, device=dev); stt = torch.ones(NI * T, dtype=torch.uint8, device=dev)

        def go():
            s = st.cuda_stream
            api.bearings_device(fe, c, kp.data_ptr(), 2 * CAP, nk.data_ptr(), NI, CAP, bk.data_ptr(), stream=s)
            api.bearings_device(fe, c, lp.data_ptr(), 2 * T, nl.data_ptr(), NI, T, bl.data_ptr(), stream=s)
            api.bearings_device(fe, c, lp.data_ptr(), 2 * T, nl.data_ptr(), NI, T, bl.data_ptr(), cam_other=c, T=T_nb[0], distance=distance, d_pred_xy=pr.data_ptr(),
                                d_other_xy=op.data_ptr(), d_other_status=stt.data_ptr(), radius=radius, d_other_bearing=bo.data_ptr(), d_pred_ok=ok.data_ptr(), stream=s)
        for _ in range(5):
            go()
        torch.cuda.synchronize()
        ms = []
        for _ in range(50):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st); go(); e1.record(st)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return {"median_ms": round(statistics.median(ms), 4), "min_max_ms": [round(min(ms), 4), round(max(ms), 4)], "lists_per_segment": NI, "cap": CAP, "cap_tracks": T,
                "every_list_full": True}

    def device_error():
        """device bearings of the tests' tolerance set (the 800 x 400 / 200 degree view, seam columns included) against the true value of the contract's formula
        evaluated on the exact phi and y / rho, rounded once; in units in the last place of the true component"""
        import mpmath
        mpmath.mp.prec = 200
        dev = torch.device("cuda")
        pts = np.unique(np.concatenate([cr.tolerance_points("view", cap).reshape(-1, 2) for cap in (64, 1100)]), axis=0).astype(np.float32)
        n = len(pts)
        d_p = torch.from_numpy(pts).to(dev); d_n = torch.full((1,), n, dtype=torch.int32, device=dev); d_b = torch.empty(n * 3, dtype=torch.float64, device=dev)
        api.bearings_device(fe, api.cylinder_camera(UW, UH, FOV), d_p.data_ptr(), 2 * n, d_n.data_ptr(), 1, n, d_b.data_ptr())
        fe.sync()
        got = d_b.cpu().numpy().reshape(n, 3)
        oracle = cr.bearings(cr.CAMS["view"], pts)
        phi, ybr = cr.angles(cr.CAMS["view"], pts)
        worst = [0.0, 0.0]
        for i in range(n):
            z = -1 if abs(phi[i]) > cr.HALF_PI else 1
            X = z * mpmath.tan(mpmath.mpf(float(phi[i])))
            Y = mpmath.mpf(float(ybr[i])) * mpmath.sqrt(X * X + 1)
            nn = mpmath.sqrt(X * X + Y * Y + 1)
            for j, t in enumerate((X / nn, Y / nn, z / nn)):
                if t == 0:
                    continue
                ulp = mpmath.ldexp(1, math.frexp(float(t))[1] - 53)
                worst[0] = max(worst[0], float(abs(mpmath.mpf(float(got[i, j])) - t) / ulp)); worst[1] = max(worst[1], float(abs(mpmath.mpf(float(oracle[i, j])) - t) / ulp))
        return {"points": n, "device_max_ulp": round(worst[0], 3), "host_oracle_max_ulp": round(worst[1], 3),
                "device_equals_host_oracle_share": round(float((got == oracle).mean()), 6),
                "note": "the true value of the contract's formula on the exact phi and y / rho (mpmath, 200 bits); ulp of the true component; recorded, not gated"}

    modes = ("A", "B", "C")
    res = {"geometry": {"raw": [RH, RW], "view": [UH, UW], "cap": CAP, "threshold": 0.15, "precision": "wino", "netvlad": True, "lanes": 4, "flow_lk": True,
                        "fov": FOV, "radius_lk": radius, "distance": distance},
           "A": "the quad pipe with flow_lk", "B": "A with d2fe_quad_bearings_enable", "C": "A plus the NumPy lift, prediction and gate on every waited result",
           "unit": "quad frames/s", "points": []}
    for Q in (1, 4):
        fps = {m: [] for m in modes}
        what = {}
        for m in modes:
            one(m, 4, Q)                                    # warm-up round: module loads, allocator
        for _ in range(max(args.rounds, 5)):
            for m in modes:
                fps[m].append(one(m, 4, Q))
                what[m] = one.last
        med = {m: statistics.median(v) for m, v in fps.items()}
        rec = {"quads": Q, "lanes": 4, "rounds": len(fps["A"])}
        for m in modes:
            rec[m + "_quad_fps_median"] = round(med[m], 1); rec[m + "_min_max"] = [round(min(fps[m]), 1), round(max(fps[m]), 1)]; rec[m + "_results"] = what[m]
        rec["B_over_A"] = round(med["B"] / med["A"], 3); rec["B_over_C"] = round(med["B"] / med["C"], 3)
        rec["B_range_overlaps_A_range"] = bool(max(fps["B"]) >= min(fps["A"]) and max(fps["A"]) >= min(fps["B"]))
        rec["B_range_lies_above_C_range"] = bool(min(fps["B"]) > max(fps["C"]))
        rec["bearings_arithmetic_hip_events"] = launch_time(Q, one.shape[0])
        rec["bearings_arithmetic_note"] = ("HIP events around d2fe_bearings_device on the three segments of a pass (4 Q keypoint rows, 4 Q lists, 4 Q gated pair lists), "
                                           "every list FULL, as three launches: an upper bound of the pipe's one launch, which also sees shorter lists")
        res["points"].append(rec)
        print(json.dumps(rec), flush=True)
    res["device_bearing_error"] = device_error()
    print(json.dumps(res["device_bearing_error"]), flush=True)
    fe.close()
    print(json.dumps({"bench_quad_pipe_bearings": res}))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
