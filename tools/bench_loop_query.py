#!/usr/bin/env python3
"""The loop query behind the stereo pipe (d2fe_loop_*, csrc/loop.hip) against the pipe alone and against the host composition it replaces, in ONE process, rounds
alternating A, B, C, A, B, C, ...:
  A  the pipe alone
  B  the pipe with the loop sequence on every ticket: d2fe_loop_enqueue behind every submit (every frame a keyframe, QUERY | ADD), d2fe_loop_collect behind every wait
  C  the pipe with the host composition on every ticket, frame by frame behind d2fe_pipe_wait: d2fe_db_query_gated -> d2fe_match_knn against the stored keyframe's
     descriptors (kept by the caller) -> d2fe_db_add -- driven from this script, as B is
The pipe as benchlib/pipe_legs.py sets it up for bench.py's `value` (640x480, 200 keypoints, NetVLAD of the left images, both matches, frames from pinned host memory), four
lanes, at 1 and at 32 stereo frames per submit; the store preloaded with 4096 and with 16384 random unit rows at NetVLAD length 4096 (one descriptor per preloaded
keyframe: the frames of a run find each other, not the preload -- what the preload costs is the search).  match_index_dist and the thresholds are the defaults of
d2fe_loop_default_config.  Prints (and writes to --out) one JSON object: stereo frames/s medians and min..max of A, B and C, B/A, B/C, whether B's range lies at or
above C's, and B's phase times.
Usage: python tools/bench_loop_query.py [--rounds 5] [--out profiles/loop_query.json]
       rocprofv3 --kernel-trace --stats ... -- python tools/bench_loop_query.py --trace NQ      (no pipe traffic: 20 d2fe_loop_query_device calls of NQ queries against
       16384 x 4096 and, beside them, d2fe_db_search of the same queries in calls of at most 4 -- loop_search_kernel against db_sims_kernel + db_topk_kernel)"""
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
DIM = 4096


def unit_rows(n, seed):
    rng = np.random.RandomState(seed)
    a = rng.standard_normal((n, DIM)).astype(np.float32)
    return a / np.linalg.norm(a, axis=1, keepdims=True)


def preload(loop, rows, cap, D):
    """one keypoint per preloaded keyframe, in chunks (the descriptor array of a call is [n][1][cap][D])"""
    CH = 256
    desc = np.zeros((CH, 1, cap, D), np.float32); desc[:, 0, 0, 0] = 1.0
    for i in range(0, len(rows), CH):
        n = min(CH, len(rows) - i)
        loop.add_host(rows[i:i + n, None], desc[:n], np.ones((n, 1), np.int32))


def trace(nq):
    import torch
    from d2slam_amd import api, netvlad as nvm
    from d2slam_amd.weights import synthetic_superpoint_weights
    H, W, CAP, NT = 120, 160, 60, 16384
    fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=CAP, input_width=W, input_height=H, max_batch=2))
    fe.load_superpoint(synthetic_superpoint_weights(dustbin_bias=7.5)); fe.load_netvlad(nvm.synthetic_netvlad_weights())
    assert fe.netvlad_dim == DIM
    pipe = api.StereoPipe(fe, lanes=1, frames=1, width=W, height=H, cap=CAP, netvlad=True)
    rows = unit_rows(NT, 1)
    loop = api.LoopQuery(pipe, capacity_keyframes=NT, max_index=10, thres=0.5, slots=2, max_queries=64)
    preload(loop, rows, CAP, 256)
    db = api.FlatIPDatabase(fe, DIM, capacity=NT); db.add(rows)
    q = unit_rows(nq, 2)
    dev = torch.device("cuda", 0)
    d_q = torch.from_numpy(q).to(dev); d_d = torch.zeros((nq, CAP, 256), device=dev); d_n = torch.ones((nq,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    REP = 20
    for _ in range(REP):
        loop.query_device(d_q.data_ptr(), d_d.data_ptr(), d_n.data_ptr(), nq, 10, 0); loop.collect(0)
    for _ in range(REP):
        for i in range(0, nq, 4):
            db.search(q[i:i + 4], 15)
    print(json.dumps({"trace": {"nq": nq, "ntotal": NT, "dim": DIM, "loop_query_device_calls": REP, "db_search_calls": REP * ((nq + 3) // 4),
                                "compulsory_bytes_per_search": NT * DIM * 4}}))
    loop.close(); db.close(); pipe.close(); fe.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loop_query.json"))
    ap.add_argument("--trace", type=int, default=0)
    args = ap.parse_args()
    if args.trace:
        return trace(args.trace)
    import torch
    from benchlib.common import CAP, H, W
    from benchlib.pipe_legs import pipe_frames
    from d2slam_amd import api, netvlad as nvm
    from d2slam_amd.weights import synthetic_superpoint_weights
    fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=CAP, input_width=W, input_height=H, max_batch=1, precision=api.PREC_F32_WINO))
    fe.load_superpoint(synthetic_superpoint_weights(dustbin_bias=7.5)); fe.load_netvlad(nvm.synthetic_netvlad_weights())
    assert fe.netvlad_dim == DIM
    lc = api._LoopConfig(); api.load_library().d2fe_loop_default_config(C.byref(lc))
    MI, THRES, RATIO = int(lc.max_index), float(lc.thres), float(lc.ratio)
    LANES = 4
    rows_all = unit_rows(16384, 1)

    def one(F, steps, warmup, host, leg, nrows):
        """stereo frames/s of `steps` submits with four in flight on a fresh pipe (and a fresh, preloaded store)"""
        pipe = api.StereoPipe(fe, lanes=LANES, frames=F, width=W, height=H, cap=CAP, netvlad=True, match_prev=True, ratio=0.8, pinned_input=True)
        base, per_set, per_side = host.data_ptr(), 2 * F * H * W, F * H * W
        total = (warmup + (warmup & 1) + steps) * F
        loop = db = None
        store, row_kf = [], []
        stat = {"queried": 0, "hits": 0, "matches": 0}
        if leg == "B":
            loop = api.LoopQuery(pipe, capacity_keyframes=nrows + total, max_index=MI, thres=THRES, ratio=RATIO, slots=LANES + 1, timing=True)
            preload(loop, rows_all[:nrows], CAP, 256)
        elif leg == "C":
            db = api.FlatIPDatabase(fe, DIM, capacity=nrows + total); db.add(rows_all[:nrows])
            one_row = np.zeros((1, 256), np.float32); one_row[0, 0] = 1.0
            store = [one_row] * nrows; row_kf = list(range(nrows))
        phases = []

        def finish(i, t):
            if leg == "A":
                pipe.wait_raw(t)
                return
            if leg == "B":
                pipe.wait_raw(t)
                r = loop.collect(i % loop.slots)
                stat["queried"] += int(r["queried"].sum()); stat["hits"] += int((r["label"] >= 0).sum()); stat["matches"] += int(r["n_match"].sum())
                phases.append(r["phase_ms"])
                return
            o = pipe.wait(t)
            for f in range(F):
                nv, n = o["netvlad"][f], int(o["n_kp"][f])
                d = o["desc"][f, :n]
                if n > 0 and db.ntotal > MI:
                    stat["queried"] += 1
                    label, _ = db.query_gated(nv, MI, THRES)
                    if label >= 0:
                        stat["hits"] += 1
                        stat["matches"] += len(fe.match_knn(d, store[row_kf[label]], RATIO)[0])
                store.append(d.copy())
                if n > 0:
                    row_kf.append(len(store) - 1); db.add(nv[None])

        def drive(n, i0):
            tk = []
            for i in range(n):
                if i >= LANES:
                    finish(i0 + i - LANES, tk[i - LANES])
                o = base + (i & 1) * per_set
                tk.append(pipe.submit_ptr(o, o + per_side))
                if leg == "B":
                    loop.enqueue(tk[i], (i0 + i) % loop.slots)
            for k in range(max(n - LANES, 0), n):
                finish(i0 + k, tk[k])
        w = warmup + (warmup & 1)
        drive(w, 0)
        torch.cuda.synchronize()
        for k in stat:
            stat[k] = 0
        del phases[:]
        t0 = time.perf_counter()
        drive(steps, w)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        one.last = dict(stat, frames=F * steps)
        if leg == "B":
            one.last["phase_ms_per_ticket"] = dict(zip(api.LOOP_PHASES, [round(float(v), 4) for v in np.mean(np.array(phases), axis=0)]))
            one.last["ntotal_end"] = loop.ntotal
            loop.close()
        if db is not None:
            db.close()
        pipe.close()
        return F * steps / dt

    res = {"geometry": {"height": H, "width": W, "cap": CAP, "lanes": LANES, "netvlad_dim": DIM, "max_index": MI, "thres": THRES, "ratio": RATIO},
           "A": "the pipe alone", "B": "the pipe with d2fe_loop_enqueue / d2fe_loop_collect on every ticket",
           "C": "the pipe with d2fe_pipe_wait -> d2fe_db_query_gated -> d2fe_match_knn -> d2fe_db_add per frame on every ticket", "points": []}
    for F, steps, warmup in ((1, 400, 16), (32, 16, 4)):
        host = torch.from_numpy(pipe_frames(F, 0)).pin_memory()
        for nrows in (4096, 16384):
            fps = {"A": [], "B": [], "C": []}
            what = {}
            for m in fps:
                one(F, max(steps // 4, 8), warmup, host, m, nrows)          # warm-up round: module loads, allocator
            for _ in range(max(args.rounds, 5)):
                for m in fps:
                    fps[m].append(one(F, steps, warmup, host, m, nrows))
                    what[m] = one.last
            med = {m: statistics.median(v) for m, v in fps.items()}
            rec = {"frames_per_submit": F, "preloaded_rows": nrows, "submits_per_round": steps, "rounds": len(fps["A"])}
            for m in fps:
                rec[m + "_stereo_fps_median"] = round(med[m], 1); rec[m + "_min_max"] = [round(min(fps[m]), 1), round(max(fps[m]), 1)]
            rec.update(B_over_A=round(med["B"] / med["A"], 3), B_over_C=round(med["B"] / med["C"], 3),
                       B_range_at_or_above_C_range=bool(min(fps["B"]) >= max(fps["C"])), B_results=what["B"], C_results=what["C"])
            res["points"].append(rec)
            print(json.dumps(rec), flush=True)
    fe.close()
    print(json.dumps({"bench_loop_query": res}))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
