#!/usr/bin/env python3
"""Remote tracking against the keyframe window (d2fe_window_*, csrc/window.hip) behind a pipe with a one-rank loopback exchange, against the exchange alone and
against the host composition it replaces, in ONE process, rounds alternating A, B, C, A, B, C, ...:
  A  the pipe plus a loopback exchange on every ticket (d2fe_exchange_* / d2fe_quad_exchange_* gated, fp32 wire)
  B  A, plus d2fe_window_push of the ticket's first frame every K-th ticket, d2fe_window_retain to 11 keyframes, and track_exchange (d2fe_window_track_device on the
     gathered blocks, in place) on every ticket, collected `lanes` tickets later
  C  A, plus the host composition of the same result behind the exchange's collect: the gathered blocks read back, the gate keyframe by keyframe, newest first, with
     d2fe_gate_pairs_device / d2fe_quad_gate_device (the keyframes' NetVLAD kept on the device by the caller, one call and one read-back per keyframe until every frame
     has its keyframe), then d2fe_match_knn of the chosen keyframe's views from the caller's host copies
Stereo: the pipe as benchlib/pipe_legs.py sets it up for bench.py's `value` (640x480, 200 keypoints, NetVLAD of the left images, both matches, pinned input).  Quad: the
geometry of tools/bench_quad_exchange.py (4 x 1280x800 -> 800x400 views, 100 keypoints).  Four lanes.  Prints (and writes to --out) one JSON object: frames/s medians
and min..max of A, B and C, B/A, B/C, whether B's range lies above C's, B's phase times, and the hits and matches B and C found (they must agree).
Usage: python tools/bench_keyframe_window.py [--rounds 5] [--points stereo:1,stereo:32,quad:1,quad:32] [--seconds 1.0] [--out profiles/keyframe_window.json]
       rocprofv3 --kernel-trace --stats ... -- python tools/bench_keyframe_window.py --trace      (one round of B at stereo:1, nothing else)"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LANES, K_PUSH, SLD_WIN, CAPACITY, THRES, RATIO = 4, 4, 11, 12, 0.8, 0.8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--points", default="stereo:1,stereo:32,quad:1,quad:32")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keyframe_window.json"))
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    import torch
    from benchlib import common as bc
    from benchlib.pipe_legs import pipe_frames
    from d2slam_amd import api, netvlad as nvm, quadcam, swarm
    from d2slam_amd.synth import synth_image
    from d2slam_amd.weights import synthetic_superpoint_weights
    dev = torch.device("cuda", 0)
    hip = swarm._hip_runtime()
    comm, collective = None, "device copy on the exchange's stream (callback)"
    try:
        comm = api.rccl_comm_init_rank(api.rccl_unique_id(), 1, 0, 0)
        collective = "one-rank ncclAllGather"
    except api.D2FEError as e:
        print("librccl not usable (%s): the collective is a device copy" % e, flush=True)

    def copy_cb(user, d_send, d_recv, nbytes, stream):
        return int(hip.hipMemcpyAsync(C.c_void_p(d_recv), C.c_void_p(d_send), C.c_size_t(nbytes), 3, C.c_void_p(stream)))

    def setup(kind, F):
        """(fe, make_pipe, make_exchange, submit, V, cap)"""
        if kind == "stereo":
            H, W, cap = bc.H, bc.W, bc.CAP
            fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=cap, input_width=W, input_height=H, max_batch=1, precision=api.PREC_F32_WINO))
            fe.load_superpoint(synthetic_superpoint_weights(dustbin_bias=7.5)); fe.load_netvlad(nvm.synthetic_netvlad_weights())
            host = torch.from_numpy(pipe_frames(F, 0)).pin_memory()
            base, per_set, per_side = host.data_ptr(), 2 * F * H * W, F * H * W
            mkp = lambda: api.StereoPipe(fe, lanes=LANES, frames=F, width=W, height=H, cap=cap, netvlad=True, match_prev=True, ratio=0.8, pinned_input=True)
            mkx = lambda p, ns: api.Exchange(p, comm=comm, world=1, rank=0, wire="fp32", loopback=True, slots=ns, own_stream=True, gate_thres=THRES,
                                             all_gather=None if comm else copy_cb)
            sub = lambda p, i: p.submit_ptr(base + (i & 1) * per_set, base + (i & 1) * per_set + per_side)
            return fe, mkp, mkx, sub, 1, cap, host
        RH, RW, UH, UW, cap = 800, 1280, 400, 800, 100
        w = dict(synthetic_superpoint_weights(dustbin_bias=7.5))
        Wt, b = w["convPb"]; b = b.copy(); b[64] -= np.float32(3.5); w["convPb"] = (Wt, b)      # as bench.py's quadcam leg: threshold 0.15 finds keypoints
        fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=cap, input_width=UW, input_height=UH, max_batch=4 * F, keypoint_threshold=0.15, precision=api.PREC_F32_WINO))
        fe.load_superpoint(w); fe.load_netvlad(nvm.synthetic_netvlad_weights())
        maps_h = [quadcam.synthetic_maps(c, RH, RW, UH, UW) for c in range(4)]
        scenes = [synth_image(RH + 8, RW + 8, 40 + c) for c in range(4)]
        host = torch.empty((2, F, 4, RH, RW), dtype=torch.uint8).pin_memory()
        hn = host.numpy()
        for s in range(2):
            for q in range(F):
                for c in range(4):
                    o = (s + 2 * q) % 8
                    hn[s, q, c] = scenes[c][o % 5:o % 5 + RH, (2 * o) % 7:(2 * o) % 7 + RW]
        per = F * 4 * RH * RW
        mkp = lambda: api.QuadPipe(fe, maps_h, lanes=LANES, quads=F, raw_width=RW, raw_height=RH, width=UW, height=UH, cap=cap, pinned_input=True)
        mkx = lambda p, ns: api.QuadExchange(p, comm=comm, world=1, rank=0, wire="fp32", mode="gated", loopback=True, slots=ns, own_stream=True, gate_thres=THRES,
                                             all_gather=None if comm else copy_cb)
        sub = lambda p, i: p.submit_ptr(host.data_ptr() + (i & 1) * per)
        return fe, mkp, mkx, sub, 4, cap, host

    def one(S, F, steps, warmup, leg):
        """frames/s (stereo frames or quad frames) of `steps` submits with four in flight, on a fresh pipe, exchange and window"""
        fe, mkp, mkx, sub, V, cap, _ = S
        G = fe.netvlad_dim
        NS = LANES + 1
        pipe = mkp(); x = mkx(pipe, NS)
        win = api.KeyframeWindow(pipe, capacity=CAPACITY, thres=THRES, ratio=RATIO, slots=NS, timing=True, max_queries=F) if leg == "B" else None
        BLK = api.block_words(cap, G)
        off_nv, off_n = api.block_field_offset(cap, G, "netvlad"), api.block_field_offset(cap, G, "n")
        stat = {"hits": 0, "matches": 0, "pushes": 0, "dropped": 0}
        phases = []
        tags = []                                   # the window, oldest first (B: a mirror of the device's; C: the caller's own)
        kf_host = {}                                # C: tag -> (desc [V][cap][256], n_kp [V])
        NSLOT = CAPACITY + 4                        # C: an evicted keyframe stays until the tickets queued before its eviction have been composed
        d_kf = torch.zeros((NSLOT, V, G), device=dev) if leg == "C" else None      # C: the keyframes' NetVLAD, slot by slot
        kf_slot, free, limbo, snap = {}, list(range(NSLOT - 1, -1, -1)), [], {}
        blocks = np.empty((F * V, BLK), np.float32)
        d_rows = torch.arange(F, dtype=torch.int32, device=dev) * V
        d_pass = torch.zeros(F, dtype=torch.int32, device=dev)

        def retain(now):
            if len(tags) > SLD_WIN:
                keep = tags[-SLD_WIN:]
                if leg == "B":
                    stat["dropped"] += win.retain(keep)
                else:
                    limbo.extend((now, t) for t in tags[:-SLD_WIN])
                    while limbo and now - limbo[0][0] > LANES:
                        t = limbo.pop(0)[1]
                        free.append(kf_slot.pop(t)); kf_host.pop(t)
                    stat["dropped"] += len(tags) - SLD_WIN
                del tags[:-SLD_WIN]

        def enqueue(i, t):
            x.enqueue(t, i % NS)
            if leg == "B":
                (win.track_exchange if V == 1 else win.track_quad_exchange)(x, i % NS, i % NS)      # the window as it stands now: keyframes up to ticket i - lanes
            elif leg == "C":
                snap[i] = list(tags)

        def finish(i, t):
            if leg == "C":
                o = pipe.wait(t)
            else:
                pipe.wait_raw(t)
            x.collect(i % NS)
            if leg == "A":
                return
            if leg == "B":
                r = win.collect(i % NS)
                stat["hits"] += int((r["keyframe_pos"] >= 0).sum()); stat["matches"] += int(r["n_match"].sum())
                phases.append(r["phase_ms"])
                if i % K_PUSH == 0:                 # processFrame behind the tracker: the exchange has been collected, so the window's release is the view's last
                    win.push(t, 0, i); tags.append(i); stat["pushes"] += 1
                    retain(i)
                return
            # C: the host composition behind the collect
            d_blocks = x.gathered(i % NS)[0]
            assert hip.hipMemcpy(C.c_void_p(blocks.ctypes.data), C.c_void_p(d_blocks), C.c_size_t(blocks.nbytes), 2) == 0
            chosen = [None] * F
            wtags = snap.pop(i)                     # the window as it stood when B queued its query for this ticket
            for pos in range(len(wtags) - 1, -1, -1):
                if all(c is not None for c in chosen):
                    break
                d_loc = torch.full((F,), kf_slot[wtags[pos]] * V, dtype=torch.int32, device=dev)
                if V == 1:
                    fe.gate_pairs_device(d_kf.data_ptr(), G, d_blocks + 4 * off_nv, BLK, G, d_loc.data_ptr(), d_rows.data_ptr(), F, THRES, d_pass=d_pass.data_ptr())
                else:
                    fe.quad_gate_device(d_kf.data_ptr(), G, d_blocks + 4 * off_nv, BLK, G, d_loc.data_ptr(), d_rows.data_ptr(), 1, 1, F, THRES, d_dir_prev=d_pass.data_ptr())
                fe.sync()
                p = d_pass.cpu().numpy()
                for q in range(F):
                    if chosen[q] is None and (int(p[q]) == 1 if V == 1 else int(p[q]) >= 0):
                        chosen[q] = (wtags[pos], int(p[q]) if V == 4 else 0)
            nk = blocks[:, off_n].view(np.int32)
            for q in range(F):
                if chosen[q] is None:
                    continue
                stat["hits"] += 1
                kd, kn = kf_host[chosen[q][0]]
                for rv, lv in api.window_views(V, chosen[q][1]):
                    a, b = kd[lv, :kn[lv]], blocks[q * V + rv, :cap * 256].reshape(cap, 256)[:nk[q * V + rv]]
                    if len(a) and len(b):
                        stat["matches"] += len(fe.match_knn(a, b, RATIO)[0])
            if i % K_PUSH == 0:                     # the caller's own emplace_back: host copies of the descriptors, the NetVLAD rows to the device
                s = free.pop(); kf_slot[i] = s
                if V == 1:
                    kf_host[i] = (o["desc"][0:1].copy(), o["n_kp"][0:1].copy()); d_kf[s].copy_(torch.from_numpy(o["netvlad"][0:1]))
                else:
                    kf_host[i] = (o["desc"][0].copy(), o["n_kp"][0].copy()); d_kf[s].copy_(torch.from_numpy(o["netvlad"][0]))
                tags.append(i); stat["pushes"] += 1
                retain(i)

        def drive(n, i0):
            tk = []
            for i in range(n):
                if i >= LANES:
                    finish(i0 + i - LANES, tk[i - LANES])
                tk.append(sub(pipe, i0 + i))
                enqueue(i0 + i, tk[i])
            for k in range(max(n - LANES, 0), n):
                finish(i0 + k, tk[k])
        w = (warmup + K_PUSH - 1) // K_PUSH * K_PUSH
        drive(w, 0)
        torch.cuda.synchronize()
        for k in stat:
            stat[k] = 0
        del phases[:]
        t0 = time.perf_counter()
        drive(steps, w)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        one.last = dict(stat, frames=F * steps, window_at_end=len(tags))
        if leg == "B":
            one.last["phase_ms_per_ticket"] = dict(zip(api.WINDOW_PHASES, [round(float(v), 4) for v in np.mean(np.array(phases), axis=0)]))
            assert win.tags() == tags
            win.close()
        x.close(); pipe.close()
        return F * steps / dt

    if args.trace:
        S = setup("stereo", 1)
        one(S, 1, 64, 8, "B")
        print(json.dumps({"trace": dict(one.last, leg="B", point="stereo:1")}))
        S[0].close()
        return
    res = {"lanes": LANES, "push_every": K_PUSH, "retain_to": SLD_WIN, "capacity": CAPACITY, "thres": THRES, "ratio": RATIO, "collective": collective,
           "A": "the pipe plus a one-rank loopback exchange on every ticket", "B": "A plus d2fe_window_push every %d-th ticket, d2fe_window_retain to %d, track_exchange on every ticket" % (K_PUSH, SLD_WIN),
           "C": "A plus the host composition: gathered blocks read back, gate keyframe by keyframe with the existing device calls, d2fe_match_knn from host copies", "points": []}
    for pt in args.points.split(","):
        kind, F = pt.split(":"); F = int(F)
        S = setup(kind, F)
        rate = {"stereo": 2000.0, "quad": 150.0}[kind]      # frames/s, roughly: sizes a round to --seconds
        steps = max(4 * LANES, int(args.seconds * rate / F) // K_PUSH * K_PUSH)
        warmup = 16 if F == 1 else 8
        fps = {"A": [], "B": [], "C": []}
        what = {}
        for m in fps:
            one(S, F, 2 * LANES, warmup, m)          # warm-up round: module loads, allocator
        for _ in range(max(args.rounds, 1)):
            for m in fps:
                fps[m].append(one(S, F, steps, warmup, m))
                what[m] = one.last
        med = {m: statistics.median(v) for m, v in fps.items()}
        rec = {"kind": kind, "frames_per_submit": F, "submits_per_round": steps, "rounds": len(fps["A"]), "netvlad_dim": S[0].netvlad_dim, "cap": S[5]}
        for m in fps:
            rec[m + "_fps_median"] = round(med[m], 1); rec[m + "_min_max"] = [round(min(fps[m]), 1), round(max(fps[m]), 1)]
        rec.update(B_over_A=round(med["B"] / med["A"], 3), B_over_C=round(med["B"] / med["C"], 3), B_range_above_C_range=bool(min(fps["B"]) > max(fps["C"])),
                   B_results=what["B"], C_results=what["C"],
                   B_and_C_agree=bool(what["B"]["hits"] == what["C"]["hits"] and what["B"]["matches"] == what["C"]["matches"]))
        res["points"].append(rec)
        print(json.dumps(rec), flush=True)
        S[0].close()
    if comm:
        api.rccl_comm_destroy(comm)
    print(json.dumps({"bench_keyframe_window": res}))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
