#!/usr/bin/env python3
"""The flow landmarks as a device chain against their host composition, in ONE process, rounds alternating C, D, C, D, ...:
  C  d2fe_lk_flow_step_device, flow only (superpoint = 0): the frames of a pass go up in one copy from pinned memory, the pyramids of all of them are built by the
     pyramids-only form of d2fe_lk_track_stereo_device (which builds each twice: it takes a stereo pair), then ONE step per frame in time order on one stream
     (five launches each), the list blocks come back in one copy, ONE synchronisation per pass
  D  the host composition of the same chain, what a caller had before: per frame api.LKFrame (upload + pyramid), api.lk_track on the previous list, reduceVector,
     removeNearPoints and api.detectPoints(use_fast) -- two stalls a frame (the tracker's and the detector's), a host sort and a host merge loop
on 640 x 480 frames, reference default parameters (150 features, 20 px, 5 px, FAST 3 x 4 regions at threshold 10), 32 frames per pass.  Three points: `sliding` (one
scene moving 3 px a frame: tracks persist, but the scene holds fewer than 113 corners 20 px apart, so every frame still detects), `sliding, 24 features` (the same
frames with total_feature_num = 24: the list is full and no frame after the first detects -- the steady state, launch 1 and four empty grids) and `unrelated` (every
frame another image: every track is lost and every frame detects its whole list).
Prints (and writes to --out) one JSON object: frames/s medians with min..max, C/D, how many frames of the pass detected, and C's D2FE_PROF_LK time per frame.
Usage: python tools/bench_lk_flow.py [--rounds 5] [--out profiles/lk_flow.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H, W, NF = 480, 640, 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lk_flow.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from d2slam_amd import api
    from d2slam_amd.synth import synth_image
    dev = torch.device("cuda", 0)
    fe = api.FrontEnd(api.SuperPointConfig(input_width=64, input_height=64, max_batch=1))
    wide = synth_image(H, W + 3 * (NF - 1), 9001).astype(np.float32)
    rng = np.random.RandomState(9)
    noise = lambda a: np.clip(np.rint(a + rng.normal(0, 3.0, a.shape)), 0, 255).astype(np.uint8)
    sliding = np.stack([noise(wide[:, 3 * t:3 * t + W]) for t in range(NF)])
    points = [("sliding", sliding, 150), ("sliding, 24 features", sliding, 24), ("unrelated", np.stack([synth_image(H, W, 9100 + t) for t in range(NF)]), 150)]
    nbytes = api.lk_stereo_workspace_bytes(NF, W, H, 2)
    total = nbytes // (2 * NF)
    d_img = torch.empty((NF, H, W), dtype=torch.uint8, device=dev)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    next_id = torch.zeros((1,), dtype=torch.int32, device=dev)
    st = torch.cuda.Stream(device=dev)
    cur = {}

    def leg_c(host):
        """one pass of NF frames from an empty list"""
        fp, lists, scratch, out = cur["fp"], cur["lists"], cur["scratch"], cur["out"]
        with torch.cuda.stream(st):
            d_img.copy_(host, non_blocking=True)
            api.lk_track_stereo_device(fe, d_img.data_ptr(), d_img.data_ptr(), NF, W, H, None, None, 0, ws.data_ptr(), None, None, stream=st.cuda_stream)
            for f in range(NF):
                api.lk_flow_step_device(fe, ws.data_ptr() + max(f - 1, 0) * total, ws.data_ptr() + f * total, W, H, lists[f].data_ptr(), lists[f + 1].data_ptr(), None, None, 0,
                                        next_id.data_ptr(), scratch.data_ptr(), fp=fp, stream=st.cuda_stream)
            out.copy_(lists[1:], non_blocking=True)
        st.synchronize()
        return out

    def leg_d(imgs):
        T = cur["T"]
        prev, pts, det = None, np.zeros((0, 2), np.float32), 0
        for img in imgs:
            frame = api.LKFrame(fe, img, 2)
            if len(pts):
                q, ok = api.lk_track(fe, prev, frame, pts, pts)
                q = q[ok != 0]
                keep = []
                for p in q:          # removeNearPoints
                    if not any(np.hypot(*(p - k)) < 5.0 for k in keep):
                        keep.append(p)
                pts = np.asarray(keep, np.float32).reshape(-1, 2)
            det += T - len(pts) > T // 4
            new = api.detectPoints(fe, frame, pts, T, use_fast=True)
            pts = np.concatenate([pts, new]) if len(new) else pts
            if prev is not None:
                prev.close()
            prev = frame
        prev.close()
        return det

    res = {"geometry": {"height": H, "width": W, "frames_per_pass": NF}, "points": [],
           "C": "d2fe_lk_flow_step_device chain, one synchronisation per pass of 32 frames", "D": "api.LKFrame + api.lk_track + api.detectPoints per frame on the host"}
    for name, imgs, feats in points:
        host = torch.from_numpy(imgs).pin_memory()
        fp = api.flow_params(superpoint=0, total_feature_num=feats)
        T = api.lk_flow_cap_tracks(fp)
        lw = api.lk_flow_list_bytes(T) // 4
        lists = torch.zeros((NF + 1, lw), device=dev)
        cur.update(fp=fp, T=T, lists=lists, scratch=torch.empty((api.lk_flow_scratch_bytes(W, H, T),), dtype=torch.uint8, device=dev),
                   out=torch.empty((NF, lw), dtype=torch.float32).pin_memory())
        lists.zero_(); next_id.zero_()
        leg_c(host); leg_d(imgs)          # warm-up round: module loads, allocator
        fps = {"C": [], "D": []}
        for _ in range(max(args.rounds, 5)):
            lists.zero_(); next_id.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter(); o = leg_c(host); fps["C"].append(NF / (time.perf_counter() - t0))
            hdr = o.numpy().view(np.int32)[:, :10].copy()
            t0 = time.perf_counter(); det_d = leg_d(imgs); fps["D"].append(NF / (time.perf_counter() - t0))
        fe.profile_enable(2)
        lists.zero_(); next_id.zero_(); leg_c(host)
        ms, n = fe.profile_read()["lk"]
        fe.profile_enable(0)
        med = {m: statistics.median(v) for m, v in fps.items()}
        rec = {"sequence": name, "total_feature_num": T, "rounds": len(fps["C"]), "C_fps_median": round(med["C"], 1), "C_min_max": [round(min(fps["C"]), 1), round(max(fps["C"]), 1)],
               "D_fps_median": round(med["D"], 1), "D_min_max": [round(min(fps["D"]), 1), round(max(fps["D"]), 1)], "C_over_D": round(med["C"] / med["D"], 2),
               "C_frames_that_detected": int((hdr[:, 8] > 0).sum()), "C_avg_list": round(float(hdr[:, 0].mean()), 1), "C_avg_lost": round(float(hdr[:, 2].mean()), 1),
               "C_avg_new": round(float(hdr[:, 4].mean()), 1), "D_frames_that_detected": int(det_d),
               "C_lk_stage_ms_per_frame": round(ms / NF, 4), "C_lk_stage_launches_per_pass": int(n),
               "C_lk_stage_note": "HIP events around every launch of the pass (profile mode 2): 2 pyramid levels + 5 launches per frame, summed, divided by the frames"}
        res["points"].append(rec)
        print(json.dumps(rec), flush=True)
    fe.close()
    print(json.dumps({"bench_lk_flow": res}))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
