"""What tests/test_quad_exchange.py and tests/helpers/quad_pipe_exchange_worker.py share: the scene of tests/helpers/quad_swarm_worker.py (raw 160 x 256 ->
views 96 x 160, cap 60, PREC_F32, the 0.35-wide NetVLAD stand-in, rank r's rig turned by r quarter turns), the hand-composed blocks, and the checks of one
collected d2fe_quad_exchange_result against the building blocks (d2fe_quad_gate_device) and the oracle (tracker_gate, match_knn)."""
import ctypes as C

import numpy as np

RH, RW, UH, UW, CAP = 160, 256, 96, 160, 60
FOV = 200.0


def raw_views(r, f=0):
    """the four raw frames of rank r's rig (its view v looks at scene (v + r) % 4); f: the quad frame of a submit (other sensor noise)"""
    from d2slam_amd.synth import synth_image
    out = []
    for v in range(4):
        scene = (v + r) % 4
        im = synth_image(RH, RW, 300 + scene).astype(np.float32) * (0.7 + 0.1 * scene)
        rng = np.random.RandomState(50 * r + v + 1000 * f)
        out.append(np.clip(np.rint(im) + rng.randint(-2, 3, im.shape), 0, 255).astype(np.uint8))
    return out


def rig(r, Q):
    return np.stack([np.stack(raw_views(r, f)) for f in range(Q)])      # u8 [Q][4][RH][RW]


def maps(shared=False):
    """the helper's four camera maps; shared: all four cameras have camera 0's intrinsics (see test_worlds_2_4_8...: with a rig turned by two or three quarter
    turns the seeded NetVLAD stand-in tells the CAMERA apart rather than the scene, so a rig of four different maps gives the gate nothing to find there)"""
    from d2slam_amd import quadcam
    return [quadcam.synthetic_maps(0 if shared else c, RH, RW, UH, UW) for c in range(4)]


def frontend(max_batch, netvlad=True):
    from d2slam_amd import api, netvlad as nvm
    from d2slam_amd.weights import synthetic_superpoint_weights
    fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=CAP, input_width=UW, input_height=UH, max_batch=max_batch, precision=api.PREC_F32))
    fe.load_superpoint(synthetic_superpoint_weights(dustbin_bias=7.5))
    if netvlad:
        fe.load_netvlad(nvm.synthetic_netvlad_weights(depth_multiplier=0.35))
    return fe


def quad_pipe(fe, lanes, quads, shared_maps=False, **kw):
    from d2slam_amd import api
    args = dict(lanes=lanes, quads=quads, raw_width=RW, raw_height=RH, width=UW, height=UH, cap=CAP, radius_neighbour=0.2 * UW, undistort_fov=FOV)
    args.update(kw)
    return api.QuadPipe(fe, maps(shared_maps), **args)


def copy_result(o):
    return {k: (None if v is None else v.copy()) for k, v in o.items()}


def hip():
    from d2slam_amd import swarm
    return swarm._hip_runtime()


def d2h(addr, nbytes):
    """bytes at a raw device address (the device is idle or the producing stream was waited for)"""
    buf = np.empty(nbytes, np.uint8)
    assert hip().hipMemcpy(C.c_void_p(buf.ctypes.data), C.c_void_p(addr), C.c_size_t(nbytes), 2) == 0
    return buf


def hand_blocks(fe, torch, dev, o, wire):
    """the blocks of one waited quad ticket composed by hand with the existing building blocks: (wire blocks u8 [4 Q][block bytes], fp32 blocks f32 [4 Q][BLK]);
    for an int8 wire the fp32 blocks are the decode (d2fe_unpack_blocks_int8_device) of the int8 ones"""
    from d2slam_amd import api
    Q = o["n_kp"].shape[0]
    NI, G = 4 * Q, (o["netvlad"].shape[-1] if o["netvlad"] is not None else 0)
    BLK, BLKB = api.block_words(CAP, G), api.block_bytes_int8(CAP, G)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    desc, kps, sc, n = t(o["desc"].reshape(NI, CAP, 256)), t(o["kps_xy"].reshape(NI, CAP, 2)), t(o["scores"].reshape(NI, CAP)), t(o["n_kp"].reshape(NI))
    nv = t(o["netvlad"].reshape(NI, G)) if G else None
    nvp = nv.data_ptr() if G else None
    f32 = torch.zeros((NI, BLK), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    if wire == "fp32":
        fe.pack_blocks_device(desc.data_ptr(), kps.data_ptr(), sc.data_ptr(), n.data_ptr(), nvp, 0, 1, NI, CAP, G, f32.data_ptr())
        fe.sync()
        h = f32.cpu().numpy()
        return h.view(np.uint8).reshape(NI, 4 * BLK).copy(), h
    q = torch.zeros((NI, BLKB), dtype=torch.int8, device=dev)
    torch.cuda.synchronize()
    fe.pack_blocks_int8_device(desc.data_ptr(), kps.data_ptr(), n.data_ptr(), nvp, 0, 1, NI, CAP, G, q.data_ptr())
    fe.unpack_blocks_int8_device(q.data_ptr(), NI, CAP, G, f32.data_ptr(), renorm=1 if wire == "int8-renorm256" else 0)
    fe.sync()
    return q.cpu().numpy().view(np.uint8).copy(), f32.cpu().numpy()


def block_fields(G):
    from d2slam_amd import api
    return {f: api.block_field_offset(CAP, G, f) for f in ("desc", "kps", "scores", "netvlad", "n")}


def job_sims(o_local, gath, lay, Q):
    """numpy similarities [njobs][4] of remote view 2 with the local views {2, 3, 0, 1} (for the guard and the threshold; the assertions use the device's)"""
    G = o_local["netvlad"].shape[-1]
    off = block_fields(G)
    out = []
    for r, q in zip(lay["job_rank"], lay["job_quad"]):
        rem2 = gath[r, 4 * q + 2][off["netvlad"]:off["netvlad"] + G]
        out.append([float(o_local["netvlad"][q, (2 + j) % 4] @ rem2) for j in range(4)])
    return np.array(out)


def halfway_threshold(sims, expected=None):
    """The helper's guard and threshold.  One job: its two largest similarities differ by > 2e-3 and the threshold lies halfway between them.  Several jobs share
    ONE threshold, and the gate takes the FIRST of the views {2, 3, 0, 1} that reaches it: with expected[j] = the index into that order the scene calls for,
    every job's two largest similarities differ by > 2e-3, the largest is the expected one, and the threshold lies halfway between the smallest expected
    similarity and the largest similarity the gate examines BEFORE an expected one (none examined before: the largest runner-up) -- which differ by > 2e-3 too."""
    srt = np.sort(sims, axis=1)
    assert np.all(srt[:, -1] - srt[:, -2] > 2e-3), "the scene must single out one local view for the remote view 2 in every job (%s)" % srt
    if len(sims) == 1:
        return float(0.5 * (srt[0, -1] + srt[0, -2]))
    expected = [int(np.argmax(s)) for s in sims] if expected is None else list(expected)
    assert [int(np.argmax(s)) for s in sims] == expected, "the largest similarity of every job must be the one the scene calls for (%s, %s)" % (sims, expected)
    hi = float(min(s[e] for s, e in zip(sims, expected)))
    before = [float(s[:e].max()) for s, e in zip(sims, expected) if e > 0]
    lo = max(before) if before else float(srt[:, -2].max())
    assert hi - lo > 2e-3, "one threshold must separate the expected view from every view examined before it, in every job (%s)" % sims
    return 0.5 * (hi + lo)


def expects_matches(wire):
    """the helper's guard `the tracked pairs yield >= 8 matches` is a condition on what the matcher is GIVEN.  fp32 blocks and int8 blocks decoded with the 256-float
    re-normalisation give it the scene's descriptors; the reference's own decode (wire "int8": the first n 32-float segments re-normalised, d2frontend_types.h:319-338)
    leaves most rows un-normalised, and matchKNN's ratio test then rejects every pair (0.0 matches per view pair) -- there the lists are held to
    the oracle on the decoded descriptors, and their emptiness is what the oracle says too."""
    return wire != "int8"


def check_result(fe, torch, dev, res, o_local, gath, world, rank, Q, mode, thres, loopback, expect_rot=None):
    """one collected result (api.QuadExchange.collect) of `rank` against d2fe_quad_gate_device and the oracle.  o_local: the waited quad pipe result of the
    ticket; gath: the gathered fp32 blocks f32 [world][4 Q][BLK] (hand-composed).  expect_rot(remote rank) -> the rotation the scene calls for, or None.
    Returns the matches on the tracked pairs of every job."""
    from d2slam_amd import swarm
    from oracle import oracle as orc, ref as spref
    G = o_local["netvlad"].shape[-1] if o_local["netvlad"] is not None else 0
    off = block_fields(G)
    BLK = gath.shape[-1]
    lay = swarm.quad_remote_job_layout(world, rank, Q, loopback)
    nj = len(lay["job_rank"])
    ppj = 4 if mode == "gated" else 16
    assert res["njobs"] == nj and res["pairs_per_job"] == ppj and res["npairs"] == nj * ppj and res["cap"] == CAP
    assert list(res["job_rank"]) == lay["job_rank"] and list(res["job_quad"]) == lay["job_quad"]
    dirs = [-1] * nj
    if G:
        # the gate: bit-equal to d2fe_quad_gate_device on the same vectors
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
        loc = t(o_local["netvlad"].reshape(4 * Q, G), np.float32); rem = t(gath.reshape(world * 4 * Q, BLK), np.float32)
        jl, jr = t(lay["local_row0"], np.int32), t(lay["remote_block0"], np.int32)
        dp = torch.full((nj,), -9, dtype=torch.int32, device=dev); sm = torch.zeros((nj, 4), dtype=torch.float32, device=dev)
        npass = torch.zeros(1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        fe.quad_gate_device(loc.data_ptr(), G, rem.data_ptr() + 4 * off["netvlad"], BLK, G, jl.data_ptr(), jr.data_ptr(), 1, 1, nj, thres, d_dir_prev=dp.data_ptr(),
                            d_sims=sm.data_ptr(), d_n_pass=npass.data_ptr())
        fe.sync()
        np.testing.assert_array_equal(res["sims"].view(np.uint32), sm.cpu().numpy().view(np.uint32), err_msg="gate_sims differ from d2fe_quad_gate_device")
        np.testing.assert_array_equal(res["dir_prev"], dp.cpu().numpy())
        assert res["gate_n"] == int(npass.item()) == int((res["dir_prev"] >= 0).sum())
        # ... and the oracle's (and the reference's own) decision on the same vectors
        for j, (r, q) in enumerate(zip(lay["job_rank"], lay["job_quad"])):
            rem_g = np.stack([gath[r, 4 * q + v][off["netvlad"]:off["netvlad"] + G] for v in range(4)])
            loc_g = o_local["netvlad"][q]
            o = orc.tracker_gate(rem_g, loc_g[None], thres, True)
            dirs[j] = o["dir_b"] if o is not None else -1
            assert int(res["dir_prev"][j]) == dirs[j], (j, res["dir_prev"][j], o)
            if o is not None:
                assert [(b, a) for a, b in o["pairs"]] == lay["gated"](dirs[j])
            if spref.available():
                f = spref.tracker_gate(rem_g, loc_g[None], thres, True)
                assert (f["dir_b"] if f is not None else -1) == dirs[j]
                if f is not None:
                    assert f["pairs"] == o["pairs"]
            if expect_rot is not None:
                assert dirs[j] == expect_rot(r), (rank, r, q, dirs[j], expect_rot(r))
    else:
        assert res["dir_prev"] is None and res["sims"] is None and res["gate_n"] == 0
    # the view pairs and every match list
    tracked = []
    for j, (r, q) in enumerate(zip(lay["job_rank"], lay["job_quad"])):
        pairs = lay["gated"](dirs[j]) if mode == "gated" else lay["all2all"][j * 16:(j + 1) * 16]
        on = set(lay["gated"](dirs[j])) if dirs[j] >= 0 else set()
        nt = 0
        for k, (lv, rv) in enumerate(pairs):
            p = j * ppj + k
            assert (int(res["local_view"][p]), int(res["remote_view"][p])) == (lv, rv), (j, k)
            n = int(res["mn"][p])
            if lv < 0:
                assert n == 0, "a job that fails the gate must not be matched"
                continue
            na = int(o_local["n_kp"][q, lv])
            blk = gath[r, 4 * q + rv]
            nb = int(blk.view(np.int32)[off["n"]])
            assert na >= 20 and nb >= 20, "the test scene must give every view keypoints (%d, %d)" % (na, nb)
            da = o_local["desc"][q, lv, :na]
            db = blk[off["desc"]:off["desc"] + 256 * nb].reshape(nb, 256)
            gq, gt, gd = orc.match_knn(da, db, 0.8)
            assert n == len(gq), (j, lv, rv, n, len(gq))
            np.testing.assert_array_equal(res["mq"][p, :n], gq); np.testing.assert_array_equal(res["mt"][p, :n], gt); np.testing.assert_array_equal(res["md"][p, :n], gd)
            if (lv, rv) in on:
                nt += n
        tracked.append(nt)
    return tracked
