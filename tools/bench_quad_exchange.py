#!/usr/bin/env python3
"""The cross-agent exchange behind the quad pipe (d2fe_quad_exchange_*, include/d2fe.h) against the quad pipe alone, in one process, at the reference geometry:
4 x 1280x800 raw fisheye frames -> 800x400 views, 100 keypoints, threshold 0.15, PREC_F32_WINO, the 0.75-wide NetVLAD stand-in, 4 lanes, 1 and 4 quad frames per
submit.  One rank in loopback (its own blocks as the remote agent): the collective is a one-rank ncclAllGather where librccl loads, else a stream-ordered device copy.
  pipe          (a) quad frames/s of the pipe alone and (b) with the exchange enqueued on every ticket, one submit behind: all2all / gated x fp32 / int8;
                alternating rounds (a), (b1) .. (b4), (a), ...; medians and min..max over the rounds, (b) / (a) per round
  phases        HIP-event time of the five phases of an enqueue (pack, all-gather, decode + prepare, remote matchKNN, release + D2H), medians over one extra round
                with timing on (the throughput rounds run with timing off), and the kernel launches an enqueue queues (counted from the sequence)
  quadswarm     the path this replaces: QuadcamChain.step alone against QuadcamChain.step + QuadSwarm.step_overlapped (swarm.py; world 2 with the collective replaced
                by a device copy of the rank's own blocks into both places, so that one process can run it), alternating rounds.  bench.py's quadcam leg builds its
                QuadSwarm only for world > 1, so `bench.py --workload quadcam --force-dist` on one GPU has no cross_agent figure to quote.
Usage: python tools/bench_quad_exchange.py [--rounds 5] [--seconds 1.0] [--quads 1,4] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
RH, RW, UH, UW, CAP, LANES = 800, 1280, 400, 800, 100, 4
VARIANTS = [("all2all", "fp32"), ("gated", "fp32"), ("all2all", "int8"), ("gated", "int8")]


def med_range(v):
    v = [float(x) for x in v]
    return {"median": round(float(np.median(v)), 3), "min": round(min(v), 3), "max": round(max(v), 3), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--quads", default="1,4")
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-quadswarm", action="store_true")
    args = ap.parse_args()
    assert args.rounds >= 1
    import torch
    from d2slam_amd import api, netvlad as nvm, quadcam, swarm
    from d2slam_amd.synth import synth_image
    from d2slam_amd.weights import synthetic_superpoint_weights
    qlist = [int(q) for q in args.quads.split(",")]
    w = dict(synthetic_superpoint_weights(dustbin_bias=7.5))
    Wt, b = w["convPb"]; b = b.copy(); b[64] -= np.float32(3.5); w["convPb"] = (Wt, b)      # as bench.py's quadcam leg: threshold 0.15 finds keypoints
    fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=CAP, input_width=UW, input_height=UH, max_batch=4 * max(qlist), keypoint_threshold=0.15,
                                           precision=api.PREC_F32_WINO))
    fe.load_superpoint(w); fe.load_netvlad(nvm.synthetic_netvlad_weights())
    lib = fe._lib
    maps_h = [quadcam.synthetic_maps(c, RH, RW, UH, UW) for c in range(4)]
    NSETS = 8
    scenes = [synth_image(RH + 8, RW + 8, 40 + c) for c in range(4)]
    host = torch.empty((NSETS, 4, RH, RW), dtype=torch.uint8).pin_memory()
    hn = host.numpy()
    for s in range(NSETS):
        for c in range(4):
            hn[s, c] = scenes[c][s % 5:s % 5 + RH, (2 * s) % 7:(2 * s) % 7 + RW]
    per = 4 * RH * RW
    dev = torch.device("cuda", 0)

    # the collective of the one-rank loopback
    comm, collective = None, "device copy on the exchange's stream (callback)"
    try:
        comm = api.rccl_comm_init_rank(api.rccl_unique_id(), 1, 0, 0)
        collective = "one-rank ncclAllGather (%s)" % lib.d2fe_rccl_path().decode()
    except api.D2FEError as e:
        print("librccl not usable (%s): the collective is a device copy" % e, flush=True)
    hip = swarm._hip_runtime()

    def copy_cb(user, d_send, d_recv, nbytes, stream):
        return int(hip.hipMemcpyAsync(C.c_void_p(d_recv), C.c_void_p(d_send), C.c_size_t(nbytes), 3, C.c_void_p(stream)))

    res = {"geometry": {"raw": [RH, RW], "view": [UH, UW], "cap": CAP, "threshold": 0.15, "precision": "wino", "lanes": LANES, "netvlad": "0.75-wide stand-in"},
           "collective": collective, "rounds": args.rounds, "pipe": [], "phases": [], "quadswarm": []}

    def emit(key, rec):
        res[key].append(rec)
        print(json.dumps({key: rec}), flush=True)

    NS = LANES + 2
    raw_res = api._QuadExchangeResult()
    for Q in qlist:
        pipe = api.QuadPipe(fe, maps_h, lanes=LANES, quads=Q, raw_width=RW, raw_height=RH, width=UW, height=UH, cap=CAP, pinned_input=True)
        nsets = NSETS // Q
        submit = lambda i: pipe.submit_ptr(host.data_ptr() + (i % nsets) * Q * per)
        mk = lambda mode, wire, timing: api.QuadExchange(pipe, comm=comm, world=1, rank=0, wire=wire, mode=mode, loopback=True, slots=NS, own_stream=True, timing=timing,
                                                         gate_thres=0.8, all_gather=None if comm else copy_cb)
        xs = {v: mk(v[0], v[1], False) for v in VARIANTS}
        xt = {v: mk(v[0], v[1], True) for v in VARIANTS}
        steps = max(6 * LANES, int(args.seconds * 900 / Q))

        def run(x, n, phases=None):
            """n submits with the pipe kept full; the exchange one submit behind the pipe, wait and collect `lanes` behind; quad frames/s"""
            tk = []
            t0 = time.perf_counter()
            for i in range(n):
                if i >= LANES:
                    pipe.wait_raw(tk[i - LANES])
                    if x:
                        api._check(lib.d2fe_quad_exchange_collect(x._x, (i - LANES) % NS, C.byref(raw_res)))
                        if phases is not None:
                            phases.append(list(raw_res.phase_ms))
                tk.append(submit(i))
                if x and i >= 1:
                    x.enqueue(tk[i - 1], (i - 1) % NS)
            if x:
                x.enqueue(tk[n - 1], (n - 1) % NS)
            for j in range(max(n - LANES, 0), n):
                pipe.wait_raw(tk[j])
                if x:
                    api._check(lib.d2fe_quad_exchange_collect(x._x, j % NS, C.byref(raw_res)))
                    if phases is not None:
                        phases.append(list(raw_res.phase_ms))
            return n * Q / (time.perf_counter() - t0)

        for x in [None] + list(xs.values()) + list(xt.values()):      # warm-up: every lane's pass shape, every exchange's buffers and matcher scratch
            run(x, 3 * LANES)
        fps = {"alone": []}
        fps.update({v: [] for v in VARIANTS})
        for _ in range(args.rounds):
            fps["alone"].append(run(None, steps))
            for v in VARIANTS:
                fps[v].append(run(xs[v], steps))
        rec = {"quads": Q, "submits_per_round": steps, "pipe_alone_quad_fps": med_range(fps["alone"])}
        for v in VARIANTS:
            rec["%s_%s" % v] = {"quad_fps": med_range(fps[v]), "over_pipe_alone": med_range([b_ / a_ for a_, b_ in zip(fps["alone"], fps[v])]),
                                "jobs": xs[v].njobs, "matcher_problems": xs[v].npairs, "block_bytes": xs[v].block_bytes}
        emit("pipe", rec)
        for v in VARIANTS:
            ph = []
            run(xt[v], steps, ph)
            ph = np.array(ph)
            emit("phases", {"quads": Q, "mode": v[0], "wire": v[1], **{n: round(float(np.median(ph[:, i])), 4) for i, n in enumerate(api.QUAD_EXCHANGE_PHASES)},
                            "stream_busy_ms_per_enqueue": round(float(np.median(ph.sum(1))), 4), "enqueues": len(ph), "gate_n_last": int(raw_res.gate_n),
                            "kernel_launches_per_enqueue": 3 + (1 if v[1] != "fp32" else 0),
                            "launches_note": "pack, [int8: decode], prepare, matcher; beside them one collective and one D2H copy"})
        for x in list(xs.values()) + list(xt.values()):
            x.close()
        pipe.close()

    if not args.skip_quadswarm:
        # the path this replaces, in one process: QuadSwarm of "world 2" whose collective copies the rank's own blocks into both places
        def fake_gather(gath, blocks, group=None):
            for r in range(gath.shape[0]):
                gath[r].copy_(blocks, non_blocking=True)
        swarm.all_gather_blocks = fake_gather
        maps_d = [tuple(torch.from_numpy(m).to(dev) for m in mm) for mm in maps_h]
        main_s = torch.cuda.Stream(device=dev); side = torch.cuda.Stream(device=dev)
        for Q in qlist:
            raw = torch.from_numpy(np.ascontiguousarray(hn[:Q].transpose(1, 0, 2, 3).reshape(4 * Q, RH, RW))).to(dev)     # the chain is camera-major
            with torch.cuda.stream(main_s):
                chain = quadcam.QuadcamChain(fe, torch, dev, Q, UH, UW, CAP, undistort_fov=200.0, knn_ratio=0.8, search_local_max_dist=0.2)
                sw = {m: swarm.QuadSwarm(chain, torch, dev, 2, 0, fe.netvlad_dim, 0.8, mode=m) for m in ("all2all", "gated")}
                torch.cuda.synchronize()
                steps = max(10, int(args.seconds * 700 / Q))

                def run_chain(qs, n):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(n):
                        chain.step(raw, RH, RW, maps_d, main_s.cuda_stream)
                        if qs:
                            qs.step_overlapped(main_s, side)
                    torch.cuda.synchronize()
                    return n * Q / (time.perf_counter() - t0)
                for qs in (None, sw["all2all"], sw["gated"]):
                    run_chain(qs, 5)
                f = {"alone": [], "all2all": [], "gated": []}
                for _ in range(args.rounds):
                    f["alone"].append(run_chain(None, steps))
                    for m in ("all2all", "gated"):
                        f[m].append(run_chain(sw[m], steps))
            emit("quadswarm", {"quads": Q, "steps_per_round": steps, "chain_alone_quad_fps": med_range(f["alone"]),
                               **{m: {"quad_fps": med_range(f[m]), "over_chain_alone": med_range([b_ / a_ for a_, b_ in zip(f["alone"], f[m])]),
                                      "matcher_problems": sw[m].NP} for m in ("all2all", "gated")}})
    if comm:
        api.rccl_comm_destroy(comm)
    fe.close()
    print(json.dumps({"bench_quad_exchange": res}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
