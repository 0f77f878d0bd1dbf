"""One rank of the world-2 test of the quad exchange BEHIND the quad pipe (tests/test_quad_exchange.py launches two of these on ONE GPU over gloo): each rank
submits its own rig (rank 1's turned by one quarter turn, two quad frames per submit) to a QuadPipe and runs swarm.QuadPipeExchange -- d2fe_quad_exchange_* with a
torch.distributed all-gather callback, host-staged under gloo -- in both modes.  Every gate decision, view pairing and match list is compared with the building
blocks and the oracle (quad_exchange_common.check_result), all2all and gated with each other on the four tracked pairs, and both with swarm.QuadSwarm over
QuadcamChain on the same frames after reindexing its view-major rows (v * Q + q) to the pipe's quad-major ones (q * 4 + v).
Exit code 0 = all assertions held."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    import torch
    import torch.distributed as dist
    from d2slam_amd import quadcam, swarm
    from tests.helpers import quad_exchange_common as qc

    rank = int(os.environ["RANK"]); world = int(os.environ["WORLD_SIZE"])
    wire = os.environ.get("QUAD_XCHG_WIRE", "fp32")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda", 0); torch.cuda.set_device(0)
    Q, CAP = 2, qc.CAP
    other = 1 - rank
    fe = qc.frontend(4 * Q)
    G = fe.netvlad_dim
    pipe = qc.quad_pipe(fe, 2, Q)
    # this rank's ticket, and -- for the expected values only -- the other agent's frames through the same pipe (same code, same GPU: what the other rank computes)
    tk = pipe.submit(qc.rig(rank, Q))
    o = qc.copy_result(pipe.wait(tk))
    o_other = qc.copy_result(pipe.wait(pipe.submit(qc.rig(other, Q))))
    hb = {rank: qc.hand_blocks(fe, torch, dev, o, wire), other: qc.hand_blocks(fe, torch, dev, o_other, wire)}
    gath = np.stack([hb[r][1] for r in range(world)])
    lay = swarm.quad_remote_job_layout(world, rank, Q)
    thres = qc.halfway_threshold(qc.job_sims(o, gath, lay, Q), [(other - rank) % 4] * Q)

    res = {}
    for mode in ("all2all", "gated"):
        x = swarm.QuadPipeExchange(torch, pipe, dev, world, rank, exchange=wire, mode=mode, gate_thres=thres, slots=2)
        assert x.njobs == Q and x.npairs == Q * (16 if mode == "all2all" else 4)
        x.enqueue(tk, 0)
        r = x.collect(0)
        tracked = qc.check_result(fe, torch, dev, r, o, gath, world, rank, Q, mode, thres, False, expect_rot=lambda rr: (2 + rr - rank) % 4)
        assert r["gate_n"] == Q and (not qc.expects_matches(wire) or min(tracked) >= 8), tracked
        # what crossed the wire: this rank's and the other rank's hand-composed blocks
        d_f32, d_wire = x.x.gathered(0)
        wire_all = np.stack([hb[rr][0] for rr in range(world)])
        assert np.array_equal(qc.d2h(d_wire, wire_all.size), wire_all.reshape(-1)), "the gathered blocks differ from the two ranks' hand-composed ones"
        res[mode] = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in r.items()}
        assert x.timeline_ms() is not None
        x.close()
    # all2all and gated agree on the four tracked pairs
    a, g = res["all2all"], res["gated"]
    np.testing.assert_array_equal(a["dir_prev"], g["dir_prev"]); np.testing.assert_array_equal(a["sims"].view(np.uint32), g["sims"].view(np.uint32))
    n_tracked = 0
    for j in range(Q):
        for k in range(4):
            lv, rv = int(g["local_view"][j * 4 + k]), int(g["remote_view"][j * 4 + k])
            pa, pg = j * 16 + lv * 4 + rv, j * 4 + k
            n = int(g["mn"][pg])
            assert n == int(a["mn"][pa])
            for f in ("mq", "mt", "md"):
                np.testing.assert_array_equal(a[f][pa, :n], g[f][pg, :n])
            n_tracked += n

    # ---- swarm.QuadSwarm over QuadcamChain on the same frames -----------------------------------------------------------------------
    st = torch.cuda.Stream(device=dev); torch.cuda.set_stream(st); s = st.cuda_stream
    raw_cm = torch.from_numpy(np.ascontiguousarray(qc.rig(rank, Q).transpose(1, 0, 2, 3)).reshape(4 * Q, qc.RH, qc.RW)).to(dev)      # camera-major
    maps = [tuple(torch.from_numpy(m).to(dev) for m in mm) for mm in qc.maps()]
    for mode in ("all2all", "gated"):
        chain = quadcam.QuadcamChain(fe, torch, dev, Q, qc.UH, qc.UW, CAP, undistort_fov=qc.FOV, knn_ratio=0.8, search_local_max_dist=0.2)
        qs = swarm.QuadSwarm(chain, torch, dev, world, rank, G, thres, mode=mode, exchange=wire)
        chain.step(raw_cm, qc.RH, qc.RW, maps, s)
        qs.step(s)
        torch.cuda.synchronize()
        assert qs.njobs == Q and [rq for rq in qs.jobs] == list(zip(lay["job_rank"], lay["job_quad"]))
        # QuadSwarm's blocks are view-major (v * Q + q); the pipe's quad-major (q * 4 + v)
        gs = qs.gath.cpu().numpy()
        for rr in range(world):
            for q in range(Q):
                for v in range(4):
                    assert np.array_equal(gs[rr, v * Q + q].view(np.uint32), gath[rr, q * 4 + v].view(np.uint32)), (rr, q, v)
        np.testing.assert_array_equal(qs.dir_prev.cpu().numpy(), a["dir_prev"])
        np.testing.assert_array_equal(qs.sims.cpu().numpy().view(np.uint32), a["sims"].view(np.uint32))
        assert int(qs.n_pass.item()) == a["gate_n"]
        mn, mq, mt, md = (t.cpu().numpy() for t in (qs.mn, qs.mq, qs.mt, qs.md))
        for j in range(Q):
            for lv in range(4):
                for rv in range(4):
                    p = j * 16 + lv * 4 + rv      # the same problem index in both (job-major, then lv * 4 + rv)
                    n = int(mn[p])
                    if mode == "gated":
                        on = [k for k in range(4) if (int(g["local_view"][j * 4 + k]), int(g["remote_view"][j * 4 + k])) == (lv, rv)]
                        if not on:
                            assert n == 0
                            continue
                        pg = j * 4 + on[0]
                        assert n == int(g["mn"][pg])
                        for f, arr in (("mq", mq), ("mt", mt), ("md", md)):
                            np.testing.assert_array_equal(arr[p, :n], g[f][pg, :n])
                    else:
                        assert n == int(a["mn"][p])
                        for f, arr in (("mq", mq), ("mt", mt), ("md", md)):
                            np.testing.assert_array_equal(arr[p, :n], a[f][p, :n])
    pipe.close(); fe.close()
    dist.barrier()
    dist.destroy_process_group()
    print("rank %d OK: wire %s, rotation dir_b %s, %d matches on the tracked view pairs" % (rank, wire, a["dir_prev"].tolist(), n_tracked))


if __name__ == "__main__":
    main()
