"""d2fe_quad_exchange_* (include/d2fe.h, csrc/quad_exchange.hip) on the GPU: the cross-agent exchange of a quadcam rank behind the quad pipe -- device view -> pack
one block per view -> ONE all-gather -> [int8: decode] -> ONE prepare launch (gate, matcher table, counter) -> ONE matcher launch -> release -> ONE D2H -- held to
the building blocks composed by hand (d2fe_pack_blocks(_int8)_device, d2fe_unpack_blocks_int8_device, d2fe_quad_gate_device) and to the oracle (tracker_gate,
match_knn; the reference's own tracker_gate where it was compiled), in one-rank loopback, at worlds 2, 4 and 8 with the emulated ranks taking turns in one process,
over gloo with two processes, beside an undisturbed pipe, and driven from g++.  Scene and guards: tests/helpers/quad_swarm_worker.py (quad_exchange_common.py)."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import quad_exchange_common as qc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = qc.CAP


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _copy_cb(calls):
    """world = 1: the gathered buffer IS the rank's blocks -- a stream-ordered device copy as the collective"""
    hip = qc.hip()

    def gather(user, d_send, d_recv, nbytes, stream):
        calls.append(nbytes)
        return int(hip.hipMemcpyAsync(C.c_void_p(d_recv), C.c_void_p(d_send), C.c_size_t(nbytes), 3, C.c_void_p(stream)))      # hipMemcpyDeviceToDevice
    return gather


@pytest.mark.parametrize("quads", [1, 2])
@pytest.mark.parametrize("wire", ["fp32", "int8", "int8-renorm256"])
@pytest.mark.parametrize("mode", ["all2all", "gated"])
def test_loopback_equals_the_building_blocks_and_the_oracle(mode, wire, quads):
    """one rank, its own blocks as the remote agent: gathered blocks byte-equal to the hand-composed pack (and decode), gate bit-equal to d2fe_quad_gate_device and
    equal to the oracle's, every match list equal to orc.match_knn, the gated pairs in trackRemoteFrames' order; then a threshold no similarity reaches"""
    from d2slam_amd import api, swarm
    torch, dev = _torch()
    Q, LANES = quads, 2
    fe = qc.frontend(4 * Q)
    G = fe.netvlad_dim
    pipe = qc.quad_pipe(fe, LANES, Q)
    frames = qc.rig(0, Q)
    tk = pipe.submit(frames)
    o = qc.copy_result(pipe.wait(tk))
    wire_h, f32_h = qc.hand_blocks(fe, torch, dev, o, wire)
    gath = f32_h[None]                                           # [world = 1][4 Q][BLK]
    lay = swarm.quad_remote_job_layout(1, 0, Q, True)
    sims = qc.job_sims(o, gath, lay, Q)
    print("loopback %s %s Q=%d: similarities per job %s" % (mode, wire, Q, sims.tolist()))
    thres = qc.halfway_threshold(sims)
    for th, forced in ((thres, False), (2.0, True)):
        calls = []
        x = api.QuadExchange(pipe, comm=None, world=1, rank=0, wire=wire, mode=mode, loopback=True, slots=2, timing=True, gate_thres=th, all_gather=_copy_cb(calls))
        assert x.njobs == Q and x.npairs == Q * (4 if mode == "gated" else 16) and x.stream is not None
        assert x.block_bytes == (4 * api.block_words(CAP, G) if wire == "fp32" else api.block_bytes_int8(CAP, G))
        x.enqueue(tk, 1)
        with pytest.raises(api.D2FEError) as ei:                  # the slot's previous exchange has not been collected
            x.enqueue(tk, 1)
        assert ei.value.code == -3
        r = x.collect(1)
        assert r["ticket"] == tk and len(r["phase_ms"]) == 5 and calls == [4 * Q * x.block_bytes]
        with pytest.raises(api.D2FEError):                        # nothing enqueued on this slot
            x.collect(0)
        d_f32, d_wire = x.gathered(1)
        assert np.array_equal(qc.d2h(d_wire, wire_h.size), wire_h.reshape(-1)), "the gathered blocks differ from the hand-composed pack"
        assert np.array_equal(qc.d2h(d_f32, f32_h.nbytes), f32_h.view(np.uint8).reshape(-1)), "the decoded blocks differ from d2fe_unpack_blocks_int8_device"
        tracked = qc.check_result(fe, torch, dev, r, o, gath, 1, 0, Q, mode, th, True, expect_rot=(lambda rr: -1) if forced else (lambda rr: 2))
        if forced:
            assert r["gate_n"] == 0 and np.all(r["dir_prev"] == -1)
            if mode == "gated":
                assert np.all(r["mn"] == 0) and np.all(r["local_view"] == -1) and np.all(r["remote_view"] == -1)
            elif qc.expects_matches(wire):                        # all2all: the gate is evaluated and counted, nothing is zeroed
                assert all(int(r["mn"][j * 16 + v * 5]) >= 8 for j in range(Q) for v in range(4)), r["mn"]
        else:
            assert r["gate_n"] == Q
            assert not qc.expects_matches(wire) or min(tracked) >= 8, "the views that look at the same scene must produce cross-agent matches (%s)" % tracked
        x.close()
    pipe.close(); fe.close()


def test_refused_configurations_and_a_failing_collective():
    from d2slam_amd import api
    ok = lambda *a: 0
    fe = qc.frontend(4)
    pipe_nv = qc.quad_pipe(fe, 2, 1)
    pipe_plain = qc.quad_pipe(fe, 2, 1, netvlad=False)
    with pytest.raises(api.D2FEError, match="gated mode needs the pipe's NetVLAD") as ei:
        api.QuadExchange(pipe_plain, world=2, rank=0, mode="gated", all_gather=ok)
    assert ei.value.code == -1
    for kw, what in ((dict(world=1, loopback=False, all_gather=ok), "nothing to exchange"), (dict(world=2, rank=2, all_gather=ok), "bad quad exchange configuration"),
                     (dict(world=2, rank=0), "neither an RCCL communicator nor"), (dict(world=2, rank=0, slots=0, all_gather=ok), "bad quad exchange configuration")):
        with pytest.raises(api.D2FEError, match=what):
            api.QuadExchange(pipe_nv, comm=None, **kw)
    # without NetVLAD, all2all: only the table is written -- 16 problems, no gate outputs
    calls = []
    x = api.QuadExchange(pipe_plain, world=1, loopback=True, all_gather=_copy_cb(calls))
    t = pipe_plain.submit(qc.rig(0, 1))
    x.enqueue(t, 0)
    o = qc.copy_result(pipe_plain.wait(t)); r = x.collect(0)
    assert r["dir_prev"] is None and r["sims"] is None and r["gate_n"] == 0 and r["npairs"] == 16
    for lv in range(4):
        for rv in range(4):
            p = lv * 4 + rv
            assert (int(r["local_view"][p]), int(r["remote_view"][p])) == (lv, rv)
            if lv == rv:                                          # a view against itself: keypoint i matches keypoint i at distance 0
                n = int(o["n_kp"][0, lv])
                assert int(r["mn"][p]) == n and np.array_equal(r["mq"][p, :n], np.arange(n)) and np.array_equal(r["mt"][p, :n], np.arange(n)) and not r["md"][p, :n].any()
    x.close()
    # a failing collective: reported, the view released, the pipe unharmed
    x = api.QuadExchange(pipe_nv, world=1, loopback=True, all_gather=lambda *a: 7)
    t = pipe_nv.submit(qc.rig(0, 1))
    with pytest.raises(api.D2FEError, match="all-gather callback failed"):
        x.enqueue(t, 0)
    assert int(pipe_nv.wait(t)["n_kp"].min()) > 10
    for i in range(6):                                            # 2 * lanes + 2 more submits: an unreleased view would refuse one of these
        pipe_nv.wait(pipe_nv.submit(qc.rig(i % 4, 1)))
    x.close(); pipe_nv.close(); pipe_plain.close(); fe.close()


@pytest.mark.parametrize("world,mode,wire,quads", [(2, "all2all", "fp32", 1), (2, "gated", "fp32", 2), (4, "all2all", "fp32", 1), (4, "gated", "int8", 1),
                                                   (8, "gated", "fp32", 1), (8, "all2all", "fp32", 2)])
def test_worlds_2_4_8_with_the_emulated_ranks_taking_turns(world, mode, wire, quads):
    """The first execution of a world > 2 pair layout by the C code: agent r is ticket r of ONE quad pipe, holding rank r's turned rig; rank r's exchange is created
    with (world, rank = r) and a callback that hands it the hand-composed blocks of every agent.  The rotation for the job against rank r' is (2 + r' - r) % 4.
    The four cameras of every rig share camera 0's maps here: measured with the oracle's NetVLAD, the seeded stand-in tells the helper's four camera maps apart more
    strongly than its four scenes once a rig is turned by two or three quarter turns (world 4, rank 0 against rank 3: similarities 0.98116 0.98045 0.98379 0.98204
    for the views {2, 3, 0, 1}, the scene's view being the last), so the guard `the two largest similarities differ by > 2e-3` fails on that input whatever the code
    does; with one camera model the same scenes give 0.9991-0.9995 for the scene's view against at most 0.9889 for any other, at every offset."""
    from d2slam_amd import api, swarm
    torch, dev = _torch()
    hip = qc.hip()
    Q = quads
    fe = qc.frontend(4 * Q)
    pipe = qc.quad_pipe(fe, max(world // 2, 1), Q, shared_maps=True)
    tks = [pipe.submit(qc.rig(r, Q)) for r in range(world)]
    outs = [qc.copy_result(pipe.wait(t)) for t in tks]
    hb = [qc.hand_blocks(fe, torch, dev, o, wire) for o in outs]
    wire_all = np.stack([h[0] for h in hb]); gath = np.stack([h[1] for h in hb])      # u8 [world][4 Q][block bytes], f32 [world][4 Q][BLK]
    G_all = torch.from_numpy(wire_all).to(dev)
    per_rank = wire_all[0].size
    torch.cuda.synchronize()
    for r in range(world):
        sent = torch.zeros(per_rank, dtype=torch.uint8, device=dev)
        seen = []

        def gather(user, d_send, d_recv, nbytes, stream, r=r, sent=sent, seen=seen):
            seen.append(nbytes)
            V = C.c_void_p
            e = hip.hipMemcpyAsync(V(d_recv), V(G_all.data_ptr()), C.c_size_t(world * per_rank), 3, V(stream))
            e = e or hip.hipMemcpyAsync(V(d_recv + r * per_rank), V(d_send), C.c_size_t(nbytes), 3, V(stream))      # the rank's own blocks into its own place
            return int(e or hip.hipMemcpyAsync(V(sent.data_ptr()), V(d_send), C.c_size_t(nbytes), 3, V(stream)))
        lay = swarm.quad_remote_job_layout(world, r, Q)
        sims = qc.job_sims(outs[r], gath, lay, Q)
        print("world %d rank %d %s %s: similarities per job %s" % (world, r, mode, wire, np.round(sims, 5).tolist()))
        thres = qc.halfway_threshold(sims, [(rr - r) % 4 for rr in lay["job_rank"]])
        x = api.QuadExchange(pipe, comm=None, world=world, rank=r, wire=wire, mode=mode, slots=1, gate_thres=thres, all_gather=gather)
        assert x.njobs == (world - 1) * Q
        x.enqueue(tks[r], 0)
        res = x.collect(0)
        assert seen == [per_rank] and np.array_equal(sent.cpu().numpy(), wire_all[r].reshape(-1)), "rank %d sent other blocks than the hand-composed ones" % r
        tracked = qc.check_result(fe, torch, dev, res, outs[r], gath, world, r, Q, mode, thres, False, expect_rot=lambda rr, r=r: (2 + rr - r) % 4)
        assert res["gate_n"] == x.njobs and (not qc.expects_matches(wire) or min(tracked) >= 8), tracked
        x.close()
    pipe.close(); fe.close()


def _same(a, b, what):
    for k in a:
        if a[k] is None:
            assert b[k] is None, k
        else:
            assert a[k].tobytes() == b[k].tobytes(), "%s: %s differs" % (what, k)


@pytest.mark.parametrize("own_stream", [True, False])
def test_the_pipe_is_undisturbed_by_an_exchange_on_every_ticket(own_stream):
    """the same raw frames through two quad pipes, one with an exchange enqueued on every ticket: every field of d2fe_quad_pipe_result byte-equal, the temporal
    matches of the following submits (which read the viewed block) included; 3 * lanes + 2 submits, so every result block is viewed and rewritten"""
    from d2slam_amd import api
    LANES, Q = 2, 2
    N = 3 * LANES + 2
    fe = qc.frontend(4 * Q)
    frames = [np.stack([np.stack(qc.raw_views(i % 4, 2 * i + f)) for f in range(Q)]) for i in range(N)]
    plain = qc.quad_pipe(fe, LANES, Q)
    ref = [qc.copy_result(plain.wait(plain.submit(f))) for f in frames]
    plain.close()
    assert sum(int(o["prev_n"].sum()) for o in ref) > 0 and sum(int(o["nb_n"].sum()) for o in ref) >= 0
    pipe = qc.quad_pipe(fe, LANES, Q)
    calls = []
    NS = LANES + 1
    x = api.QuadExchange(pipe, world=1, loopback=True, mode="gated", wire="int8", slots=NS, own_stream=own_stream, gate_thres=0.5, all_gather=_copy_cb(calls))
    assert (x.stream is not None) == own_stream
    tk = []
    for i in range(N):                                            # the pipe kept full: the exchange one submit behind it, the wait `lanes` behind
        tk.append(pipe.submit(frames[i]))
        if i >= 1:
            x.enqueue(tk[i - 1], (i - 1) % NS)
        if i >= LANES:
            j = i - LANES
            _same(ref[j], pipe.wait(tk[j]), "submit %d" % j)
            assert x.collect(j % NS)["ticket"] == tk[j]
    x.enqueue(tk[N - 1], (N - 1) % NS)
    for j in range(N - LANES, N):
        _same(ref[j], pipe.wait(tk[j]), "submit %d" % j)
        assert x.collect(j % NS)["ticket"] == tk[j]
    assert len(calls) == N
    x.close(); pipe.close(); fe.close()


def test_a_view_that_is_never_released_ends_the_pipe():
    """a block whose view is outstanding when its lane comes round again (2 * lanes submits later) fails that submit with D2FE_ERR_INVALID; the pipe then reports its
    sticky error and nothing hangs"""
    from d2slam_amd import api
    torch, dev = _torch()
    LANES = 2
    fe = qc.frontend(4)
    pipe = qc.quad_pipe(fe, LANES, 1)
    st = torch.cuda.Stream(device=dev)
    frame = qc.rig(0, 1)
    t0 = pipe.submit(frame)
    with pytest.raises(api.D2FEError):                            # no view is outstanding yet
        pipe.device_release(t0, st.cuda_stream)
    v = pipe.device_view(t0, st.cuda_stream)
    assert (v.quads, v.cap, v.desc_dim, v.netvlad_dim) == (1, CAP, 256, fe.netvlad_dim) and v.d_desc and v.d_kps_xy and v.d_scores and v.d_n_kp and v.d_netvlad
    assert pipe.lane_stream(t0)
    n0 = pipe.wait(t0)["n_kp"][0].copy()                          # the ticket is complete: the view's memory may be read from the host
    assert np.array_equal(np.frombuffer(qc.d2h(v.d_n_kp, 16).tobytes(), np.int32), n0)
    for i in range(2 * LANES - 1):
        pipe.wait(pipe.submit(frame))
    with pytest.raises(api.D2FEError, match="was not released") as ei:
        pipe.submit(frame)
    assert ei.value.code == -1
    for call in (lambda: pipe.submit(frame), lambda: pipe.wait(t0 + 2 * LANES - 1), lambda: pipe.device_view(t0 + 2 * LANES - 1, st.cuda_stream)):
        with pytest.raises(api.D2FEError, match="failed in an earlier call") as ei:
            call()
        assert ei.value.code == -1
    torch.cuda.synchronize()
    pipe.close(); fe.close()


def test_a_released_view_lets_the_lane_write_its_block_again():
    """view + release by hand on a stream of the caller's: 3 * lanes further submits go through, and their results equal a pipe nobody looked into"""
    from d2slam_amd import api      # noqa: F401
    torch, dev = _torch()
    LANES = 2
    fe = qc.frontend(4)
    frames = [qc.rig(i % 4, 1) for i in range(3 * LANES + 1)]
    plain = qc.quad_pipe(fe, LANES, 1)
    ref = [qc.copy_result(plain.wait(plain.submit(f))) for f in frames]
    plain.close()
    pipe = qc.quad_pipe(fe, LANES, 1)
    st = torch.cuda.Stream(device=dev)
    for i, f in enumerate(frames):
        t = pipe.submit(f)
        pipe.device_view(t, st.cuda_stream)
        pipe.device_release(t, st.cuda_stream)
        _same(ref[i], pipe.wait(t), "submit %d" % i)
    pipe.close(); fe.close()


def _torchrun(script, env_extra, timeout=900):
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ); env.update(env_extra)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port), script]
    return subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)


@pytest.mark.parametrize("wire", ["fp32", "int8"])
def test_world2_over_gloo_equals_quadswarm_and_the_oracle(wire):
    """two processes on the one GPU over gloo, through swarm.QuadPipeExchange: both modes, against each other, the oracle and QuadSwarm (tests/helpers/quad_pipe_exchange_worker.py)"""
    r = _torchrun(os.path.join(ROOT, "tests", "helpers", "quad_pipe_exchange_worker.py"), {"QUAD_XCHG_WIRE": wire})
    errs = "\n".join([l for l in (r.stdout + "\n" + r.stderr).splitlines() if l.startswith("[rank") or "Error" in l or "assert" in l][:60])
    assert r.returncode == 0, errs
    assert r.stdout.count(" OK: ") == 2, r.stdout[-2000:]


@pytest.mark.parametrize("mode,wire,own_stream", [(0, 0, 1), (1, 2, 0)])
def test_cpp_driver_equals_the_python_binding(tmp_path, mode, wire, own_stream):
    """tests/cpp/quad_exchange_test.cpp (g++, only libd2fe_hip.so, no Python in the process): the callback leg must run; the one-rank RCCL leg runs where librccl
    loads and must equal the callback leg (the program checks), else the program says that it skipped it.  Every record of the callback leg against the binding."""
    from d2slam_amd import api, netvlad as nvm
    from d2slam_amd.weights import save_superpoint_d2fw, save_netvlad_d2fw, synthetic_superpoint_weights
    from tests.test_quad_exchange_cpu import _build_cpp
    exe = _build_cpp(tmp_path)
    sp, nvp, fin, fout = (str(tmp_path / n) for n in ("sp.d2fw", "nv.d2fw", "in.bin", "out.bin"))
    save_superpoint_d2fw(sp, synthetic_superpoint_weights(dustbin_bias=7.5)); save_netvlad_d2fw(nvp, nvm.synthetic_netvlad_weights(depth_multiplier=0.35))
    Q, LANES, N = 2, 2, 6
    frames = np.concatenate([np.stack([np.stack(qc.raw_views(i % 4, 2 * i + f)) for f in range(Q)]) for i in range(N // Q)])      # [N][4][RH][RW]
    with open(fin, "wb") as f:
        f.write(struct.pack("<6i", N, qc.RH, qc.RW, qc.UH, qc.UW, CAP))
        for mm in qc.maps():
            for m in mm:
                f.write(np.ascontiguousarray(m, np.float32).tobytes())
        f.write(frames.tobytes())
    thres = 0.9
    res = subprocess.run([exe, sp, nvp, fin, fout, str(LANES), str(Q), str(mode), str(wire), str(own_stream), repr(thres)], capture_output=True, text=True, timeout=600)
    print(res.stdout)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "quad_exchange_test callback leg OK" in res.stdout and "quad_exchange_test OK" in res.stdout
    assert ("RCCL leg OK" in res.stdout) != ("RCCL leg skipped" in res.stdout)
    data, pos = open(fout, "rb").read(), 0

    def take(dt, n):
        nonlocal pos
        a = np.frombuffer(data, dt, n, pos).copy(); pos += n * np.dtype(dt).itemsize
        return a
    fe = qc.frontend(4 * Q)
    pipe = qc.quad_pipe(fe, 1, Q)
    x = api.QuadExchange(pipe, world=1, loopback=True, mode=("all2all", "gated")[mode], wire=("fp32", "int8", "int8-renorm256")[wire], slots=1, gate_thres=thres,
                         all_gather=_copy_cb([]))
    ppj = 4 if mode else 16
    for i in range(N // Q):
        t = pipe.submit(frames[i * Q:(i + 1) * Q])
        x.enqueue(t, 0)
        o = pipe.wait(t); r = x.collect(0)
        np.testing.assert_array_equal(take("<i4", 4 * Q), o["n_kp"].reshape(-1))
        assert take("<i4", 4).tolist() == [Q, Q * ppj, ppj, r["gate_n"]]
        np.testing.assert_array_equal(take("<i4", Q), r["job_rank"]); np.testing.assert_array_equal(take("<i4", Q), r["job_quad"])
        np.testing.assert_array_equal(take("<i4", Q), r["dir_prev"])
        np.testing.assert_array_equal(take("<u4", 4 * Q), r["sims"].view(np.uint32).reshape(-1))
        mn = take("<i4", Q * ppj)
        np.testing.assert_array_equal(mn, r["mn"])
        np.testing.assert_array_equal(take("<i4", Q * ppj), r["local_view"]); np.testing.assert_array_equal(take("<i4", Q * ppj), r["remote_view"])
        mq = take("<i4", Q * ppj * CAP).reshape(-1, CAP); mt = take("<i4", Q * ppj * CAP).reshape(-1, CAP); md = take("<f4", Q * ppj * CAP).reshape(-1, CAP)
        for p in range(Q * ppj):
            n = int(mn[p])
            np.testing.assert_array_equal(mq[p, :n], r["mq"][p, :n]); np.testing.assert_array_equal(mt[p, :n], r["mt"][p, :n]); np.testing.assert_array_equal(md[p, :n], r["md"][p, :n])
        assert int(mn.sum()) > 0
    assert pos == len(data)
    x.close(); pipe.close(); fe.close()
