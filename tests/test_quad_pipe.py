"""Quadcam frames in flight (d2fe_quad_pipe_*, include/d2fe.h, csrc/quad_pipe.hip): one submit and one wait per `quads` quad frames -- raw fisheye frames ->
ONE undistort launch -> SuperPoint + NetVLAD of every view -> neighbour and temporal matches -- held to QuadcamChain (d2slam_amd/quadcam.py), to the
per-camera undistort call, to a one-lane one-quad-frame pipe, to the oracle's neighbour chain, and driven from g++ (tests/cpp/quad_pipe_test.cpp)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from d2slam_amd.synth import synth_image

RH, RW, UH, UW, CAP = 240, 384, 120, 192, 60
FOV = 200.0


def _weights():
    from d2slam_amd.weights import synthetic_superpoint_weights
    w = dict(synthetic_superpoint_weights(dustbin_bias=7.5))
    Wt, b = w["convPb"]
    b = b.copy(); b[64] -= np.float32(3.5); w["convPb"] = (Wt, b)      # threshold 0.15 (the bench's quadcam leg) still finds keypoints
    return w


def _frontend(max_batch, prec=None, netvlad=True):
    from d2slam_amd import api, netvlad as nvm
    fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=CAP, input_width=UW, input_height=UH, max_batch=max_batch, keypoint_threshold=0.15,
                                           precision=api.PREC_F32_WINO if prec is None else prec))
    fe.load_superpoint(_weights())
    if netvlad:
        fe.load_netvlad(nvm.synthetic_netvlad_weights())
    return fe


def _maps():
    from d2slam_amd import quadcam
    return [quadcam.synthetic_maps(c, RH, RW, UH, UW) for c in range(4)]


def _quads(n, seed=0):
    """n consecutive quad frames u8 [n][4][RH][RW]: four scenes under a small camera motion, so that temporal matches exist"""
    scenes = [synth_image(RH + 16, RW + 16, 300 + 4 * seed + c) for c in range(4)]
    rng = np.random.RandomState(seed)
    out = np.empty((n, 4, RH, RW), np.uint8)
    for i in range(n):
        dy, dx = i % 5, (3 * i) % 7
        for c in range(4):
            out[i, c] = np.clip(scenes[c][dy:dy + RH, dx:dx + RW].astype(np.int16) + rng.randint(-2, 3, (RH, RW)), 0, 255)
    return out


def _pipe(fe, maps, **kw):
    from d2slam_amd import api
    args = dict(lanes=1, quads=1, raw_width=RW, raw_height=RH, width=UW, height=UH, cap=CAP, radius_neighbour=0.2 * UW, undistort_fov=FOV)
    args.update(kw)
    return api.QuadPipe(fe, maps, **args)


def _copy(o):
    return {k: (None if v is None else v.copy()) for k, v in o.items()}


def _assert_same(a, qa, b, qb, what=""):
    """quad frame qa of result a == quad frame qb of result b (rows beyond a count are not part of a result)"""
    np.testing.assert_array_equal(a["n_kp"][qa], b["n_kp"][qb], err_msg=what)
    for v in range(4):
        n = int(a["n_kp"][qa, v])
        for k in ("kps_xy", "scores", "desc"):
            np.testing.assert_array_equal(a[k][qa, v, :n], b[k][qb, v, :n], err_msg="%s %s view %d" % (what, k, v))
    if a["netvlad"] is not None:
        np.testing.assert_array_equal(a["netvlad"][qa], b["netvlad"][qb], err_msg=what)
    for pre in ("nb", "prev"):
        np.testing.assert_array_equal(a[pre + "_n"][qa], b[pre + "_n"][qb], err_msg="%s %s_n" % (what, pre))
        for p in range(4):
            n = int(a[pre + "_n"][qa, p])
            for k in ("_q", "_t", "_dist"):
                np.testing.assert_array_equal(a[pre + k][qa, p, :n], b[pre + k][qb, p, :n], err_msg="%s %s pair %d" % (what, pre + k, p))


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["wino", "f32"])
def test_quad_pipe_equals_quadcam_chain(prec):
    """Q = 1, one lane, four consecutive submits: every output bit-identical to QuadcamChain.step on the same raw frames and maps"""
    import torch
    from d2slam_amd import api, quadcam
    dev = torch.device("cuda", 0)
    fe = _frontend(4, api.PREC_F32_WINO if prec == "wino" else api.PREC_F32)
    maps_h = _maps()
    pipe = _pipe(fe, maps_h)
    maps = [tuple(torch.from_numpy(np.ascontiguousarray(m)).to(dev) for m in mm) for mm in maps_h]
    chain = quadcam.QuadcamChain(fe, torch, dev, 1, UH, UW, CAP, undistort_fov=FOV, knn_ratio=0.8, search_local_max_dist=0.2)
    st = torch.cuda.Stream(device=dev)
    frames = _quads(4, seed=1)
    total_nb = total_prev = 0
    for i in range(4):
        o = _copy(pipe.wait(pipe.submit(frames[i][None])))
        raw = torch.from_numpy(frames[i]).to(dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            chain.step(raw, RH, RW, maps, st.cuda_stream)
        torch.cuda.synchronize()
        cnt = chain.cnt[:4].cpu().numpy()
        ref = {"n_kp": cnt[None], "kps_xy": chain.pts[:4].cpu().numpy()[None], "scores": chain.scores.cpu().numpy()[None],
               "desc": chain.desc[:4].cpu().numpy()[None], "netvlad": chain.gdesc.cpu().numpy()[None]}
        mq, mt, md, mn = (x.cpu().numpy() for x in (chain.mq, chain.mt, chain.md, chain.mn))
        ref.update({"nb_q": mq[None, :4], "nb_t": mt[None, :4], "nb_dist": md[None, :4], "nb_n": mn[None, :4],
                    "prev_q": mq[None, 4:], "prev_t": mt[None, 4:], "prev_dist": md[None, 4:], "prev_n": mn[None, 4:]})
        _assert_same(o, 0, ref, 0, "submit %d" % i)
        assert int(o["n_kp"].min()) > 10
        if i == 0:
            assert int(o["prev_n"].sum()) == 0                     # the very first quad frame has no predecessor
        total_nb += int(o["nb_n"].sum()); total_prev += int(o["prev_n"].sum())
    assert total_prev > 0
    pipe.close(); fe.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dh,dw", [(UH, UW), (37, 101)])
def test_quad_undistort_kernel_equals_the_single_calls(dh, dw):
    """d2fe_quad_undistort_device (ONE launch, 4 cameras x 3 frames) == d2fe_undistort_device camera by camera, byte for byte: with gain, without, mixed;
    maps that point outside the frame, at negative coordinates, straddle the last row / column and hit exact integers; a view size that is not a
    multiple of 4 pixels (the kernel's scalar tail)"""
    import torch
    from d2slam_amd import api, quadcam
    dev = torch.device("cuda", 0)
    fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=CAP, input_width=UW, input_height=UH, max_batch=4))
    Q = 3
    rng = np.random.RandomState(7)
    raw = np.clip(np.stack([[synth_image(RH, RW, 50 + 4 * q + c) for c in range(4)] for q in range(Q)]).astype(np.int16) + 60, 0, 255).astype(np.uint8)
    maps = []
    for c in range(4):
        mx, my, g = (m.copy() for m in quadcam.synthetic_maps(c, RH, RW, dh, dw))
        fx, fy, fg = mx.reshape(-1), my.reshape(-1), g.reshape(-1)
        sel = np.arange(fx.size) % 13
        fx[sel == 1] = -0.75; fy[sel == 2] = -1.0                     # left of / above the frame
        fx[sel == 3] = RW - 0.5; fy[sel == 4] = RH - 0.75            # straddling the last column / row
        fx[sel == 5] = RW + 3.0; fy[sel == 6] = -7.5                  # outside
        fx[sel == 7] = np.floor(fx[sel == 7]); fy[sel == 7] = np.floor(fy[sel == 7])      # exact integers
        fx[sel == 8] = 0.0; fy[sel == 8] = 0.0
        fx[sel == 9] = RW - 1.0; fy[sel == 9] = RH - 1.0
        fg[sel == 10] = 3.0                                           # saturates
        fx[sel == 11] = rng.uniform(-2, RW + 2, (sel == 11).sum()); fy[sel == 11] = rng.uniform(-2, RH + 2, (sel == 11).sum())
        maps.append((mx, my, g))
    d_raw = torch.from_numpy(raw).to(dev)
    d_maps = [tuple(torch.from_numpy(np.ascontiguousarray(m)).to(dev) for m in mm) for mm in maps]
    torch.cuda.synchronize()
    for mode in ("all", "none", "mixed"):
        use = [mode == "all" or (mode == "mixed" and c % 2 == 0) for c in range(4)]
        ptrs = [(d_maps[c][0].data_ptr(), d_maps[c][1].data_ptr(), d_maps[c][2].data_ptr() if use[c] else None) for c in range(4)]
        out = torch.full((Q, 4, dh, dw), 7, dtype=torch.uint8, device=dev)
        ref = torch.full((4, Q, dh, dw), 9, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        fe.quad_undistort_device(d_raw.data_ptr(), Q, RW, RH, ptrs, dw, dh, out.data_ptr())
        for c in range(4):
            fe.undistort_device(d_raw.data_ptr() + c * RH * RW, Q, RW, RH, ptrs[c][0], ptrs[c][1], ptrs[c][2], dw, dh, ref[c].data_ptr(),
                                src_image_stride=4 * RH * RW)
        fe.sync(); torch.cuda.synchronize()
        o, r = out.cpu().numpy(), ref.cpu().numpy()
        for c in range(4):
            np.testing.assert_array_equal(o[:, c], r[c], err_msg="gain %s camera %d" % (mode, c))
        assert (o == 0).any()                                        # the taps outside the frame
        if mode != "none":
            assert (o == 255).any()                                  # gain 3 saturates
    fe.close()


@pytest.fixture(scope="module")
def fif():
    """one front end (max_batch 16), the maps, 32 consecutive quad frames and what a one-lane, one-quad-frame pipe returns for them"""
    fe = _frontend(16)
    maps = _maps()
    frames = _quads(32, seed=2)
    ref_pipe = _pipe(fe, maps)
    ref = [_copy(ref_pipe.wait(ref_pipe.submit(frames[i][None]))) for i in range(32)]
    ref_pipe.close()
    yield fe, maps, frames, ref
    fe.close()


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [1, 2, 4])
@pytest.mark.parametrize("quads", [1, 2, 4])
def test_quad_pipe_frames_in_flight_equal_one_lane(fif, quads, lanes):
    """8 submits of `quads` quad frames on `lanes` lanes, waited for in order and out of order: every ticket bit-identical to the one-lane one-quad-frame
    pipe on the same sequence -- the temporal pairs across submit and lane-wrap boundaries included"""
    fe, maps, frames, ref = fif
    nsub = 8
    assert int(ref[0]["prev_n"].sum()) == 0 and sum(int(r["prev_n"].sum()) for r in ref) > 0
    for order in ("in_order", "out_of_order"):
        pipe = _pipe(fe, maps, lanes=lanes, quads=quads)
        got, tickets = {}, []
        for i in range(nsub):
            tickets.append(pipe.submit(frames[i * quads:(i + 1) * quads]))
            if order == "in_order":
                if i >= lanes - 1:
                    got[i - lanes + 1] = _copy(pipe.wait(tickets[i - lanes + 1]))
            elif (i + 1) % lanes == 0:                               # a window of `lanes` submits, newest first
                for j in range(i, i - lanes, -1):
                    got[j] = _copy(pipe.wait(tickets[j]))
        for j in range(nsub):
            if j not in got:
                got[j] = _copy(pipe.wait(tickets[j]))
        pipe.close()
        for j in range(nsub):
            for qq in range(quads):
                _assert_same(got[j], qq, ref[j * quads + qq], 0, "%s ticket %d quad %d" % (order, j, qq))


@pytest.mark.gpu
def test_quad_pipe_pinned_input_gives_the_same_bits(fif):
    import torch
    fe, maps, frames, ref = fif
    host = torch.from_numpy(frames[:16].copy()).pin_memory()
    pipe = _pipe(fe, maps, lanes=2, quads=2, pinned_input=True)
    with pytest.raises(ValueError):
        pipe.submit(frames[:2])
    per = 2 * 4 * RH * RW
    tk = []
    for i in range(8):
        tk.append(pipe.submit_ptr(host.data_ptr() + i * per))
        if i >= 1:
            o = _copy(pipe.wait(tk[i - 1]))
            for qq in range(2):
                _assert_same(o, qq, ref[(i - 1) * 2 + qq], 0, "pinned ticket %d" % (i - 1))
    o = _copy(pipe.wait(tk[7]))
    for qq in range(2):
        _assert_same(o, qq, ref[14 + qq], 0, "pinned ticket 7")
    pipe.close()


@pytest.mark.gpu
def test_quad_pipe_lists_equal_the_oracle_chain(orc):
    """one quad frame after one predecessor: the four neighbour lists equal the oracle's statement of matchLocalFeatures on the pipe's own keypoints and
    descriptors (and the reference's own branch where it is built); the temporal lists equal the oracle's matchKNN against the previous quad frame"""
    from oracle import ref as spref
    from d2slam_amd import quadcam
    from tests.test_ref_pin import orc_neighbour_chain
    fe = _frontend(4)
    # neighbouring views see one panorama shifted by move_cols (test_quadcam_chain.py's scene): identity-like 2x maps keep the shift, so the neighbour
    # lists are not empty
    yy, xx = np.mgrid[0:UH, 0:UW].astype(np.float32)
    maps = [(xx * np.float32(RW / UW), yy * np.float32(RH / UH), np.ones((UH, UW), np.float32)) for _ in range(4)]
    step_raw = int(round(fe.half_move_cols(UW, FOV))) * (RW // UW)
    frames = np.empty((2, 4, RH, RW), np.uint8)
    for i in range(2):
        pano = synth_image(RH, RW + 3 * step_raw + 8, 910)
        for c in range(4):
            x0 = (3 - c) * step_raw + 3 * i
            frames[i, c] = pano[:, x0:x0 + RW]
    pipe = _pipe(fe, maps)
    o0 = _copy(pipe.wait(pipe.submit(frames[0][None])))
    o1 = _copy(pipe.wait(pipe.submit(frames[1][None])))
    pipe.close(); fe.close()
    assert int(o1["nb_n"].sum()) >= 10 and int(o1["prev_n"].sum()) >= 10
    for p, (ca, cb, typ) in enumerate(quadcam.NEIGHBOURS):
        na, nb = int(o1["n_kp"][0, ca]), int(o1["n_kp"][0, cb])
        pa, da, pb, db = o1["kps_xy"][0, ca, :na], o1["desc"][0, ca, :na], o1["kps_xy"][0, cb, :nb], o1["desc"][0, cb, :nb]
        exp = orc_neighbour_chain(orc, pa, da, pb, db, typ, 0.8, True, 0.2 * UW, UW, FOV)
        if spref.available():
            r2 = spref.match_neighbour(pa, da, pb, db, typ, 0.8, True, 0.2 * UW, UW, FOV)
            assert (exp is None) == (r2 is None)
            if exp is not None:
                assert all(np.array_equal(x, y) for x, y in zip(exp, r2))
        n = int(o1["nb_n"][0, p])
        if exp is None:
            assert n == 0
        else:
            assert n == len(exp[0])
            assert np.array_equal(o1["nb_q"][0, p, :n], exp[0]) and np.array_equal(o1["nb_t"][0, p, :n], exp[1]) and np.array_equal(o1["nb_dist"][0, p, :n], exp[2])
    for c in range(4):
        n1, n0 = int(o1["n_kp"][0, c]), int(o0["n_kp"][0, c])
        rq, rt, rd = orc.match_knn(o1["desc"][0, c, :n1], o0["desc"][0, c, :n0], 0.8)
        n = int(o1["prev_n"][0, c])
        assert n == len(rq) and np.array_equal(o1["prev_q"][0, c, :n], rq) and np.array_equal(o1["prev_t"][0, c, :n], rt)
        assert np.array_equal(o1["prev_dist"][0, c, :n], rd)


@pytest.mark.gpu
def test_quad_pipe_contract():
    """invalid configurations create no pipe; while a quad pipe lives the handle refuses reloads and its destroy is deferred; a black view is empty"""
    from d2slam_amd import api, netvlad as nvm, quadcam
    fe = _frontend(4)
    lib = fe._lib
    maps = _maps()
    for kw in (dict(lanes=0), dict(lanes=17), dict(quads=0), dict(quads=2), dict(width=UW + 8), dict(height=UH + 8), dict(cap=CAP + 1)):
        mk = [quadcam.synthetic_maps(c, RH, RW, kw.get("height", UH), kw.get("width", UW)) for c in range(4)]      # maps of the size asked for
        with pytest.raises(api.D2FEError) as ei:
            _pipe(fe, mk, **kw)
        assert ei.value.code == -1, kw
    c = api._QuadPipeConfig()
    lib.d2fe_quad_pipe_default_config(C.byref(c))
    c.lanes, c.raw_width, c.raw_height, c.width, c.height, c.cap = 1, RW, RH, UW, UH, CAP
    p = C.c_void_p()
    assert lib.d2fe_quad_pipe_create(fe.handle, C.byref(c), None, C.byref(p)) == -1 and not p.value
    keep = [np.ascontiguousarray(m, np.float32) for mm in maps for m in mm]
    m = api._quad_maps([(keep[3 * k].ctypes.data, keep[3 * k + 1].ctypes.data, None) for k in range(4)], False)
    m.mapy[2] = None
    assert lib.d2fe_quad_pipe_create(fe.handle, C.byref(c), C.byref(m), C.byref(p)) == -1 and not p.value
    fe.load_superpoint(_weights())                                   # no pipe was left alive by the refusals
    pipe = _pipe(fe, maps)
    with pytest.raises(api.D2FEError) as ei:
        fe.load_superpoint(_weights())
    assert ei.value.code == -1
    with pytest.raises(api.D2FEError) as ei:
        fe.load_netvlad(nvm.synthetic_netvlad_weights())
    assert ei.value.code == -1
    fr = _quads(2, seed=4)
    fr[1, 2] = 0                                                     # a black view
    o0 = _copy(pipe.wait(pipe.submit(fr[0][None])))
    o = _copy(pipe.wait(pipe.submit(fr[1][None])))
    assert int(o["n_kp"][0, 2]) == 0 and int(o["prev_n"][0, 2]) == 0
    assert int(o["nb_n"][0, 1]) == 0 and int(o["nb_n"][0, 2]) == 0     # (1,2) and (2,3)
    assert int(o["n_kp"][0, 0]) > 10
    # d2fe_destroy under a live quad pipe is DEFERRED: the pipe keeps working on the handle's weights, the last pipe destroy releases the handle
    lib.d2fe_destroy(fe.handle)
    assert b"live pipes" in lib.d2fe_last_error()
    o2 = _copy(pipe.wait(pipe.submit(fr[0][None])))
    np.testing.assert_array_equal(o2["n_kp"], o0["n_kp"])
    pipe.close()
    fe._h = C.c_void_p()                                             # released by the pipe: the wrapper must not destroy it again


@pytest.mark.gpu
def test_cpp_quad_pipe_equals_the_python_binding(tmp_path):
    """tests/cpp/quad_pipe_test.cpp (g++, only libd2fe_hip.so, 2 lanes x 2 quad frames per submit) against a one-lane one-quad-frame pipe of the binding"""
    from d2slam_amd import netvlad as nvm
    from d2slam_amd.weights import save_superpoint_d2fw, save_netvlad_d2fw
    from tests.test_quad_pipe_cpu import _build_cpp
    exe = _build_cpp(tmp_path)
    sp, nvp, fin, fout = (str(tmp_path / n) for n in ("sp.d2fw", "nv.d2fw", "in.bin", "out.bin"))
    save_superpoint_d2fw(sp, _weights()); save_netvlad_d2fw(nvp, nvm.synthetic_netvlad_weights())
    maps = _maps()
    N = 8
    frames = _quads(N, seed=5)
    with open(fin, "wb") as f:
        f.write(struct.pack("<6i", N, RH, RW, UH, UW, CAP))
        for mm in maps:
            for m in mm:
                f.write(np.ascontiguousarray(m, np.float32).tobytes())
        f.write(frames.tobytes())
    res = subprocess.run([exe, sp, nvp, fin, fout, "2", "2"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "quad_pipe_test OK" in res.stdout
    data, pos = open(fout, "rb").read(), 0

    def take(dt, n):
        nonlocal pos
        a = np.frombuffer(data, dt, n, pos).copy(); pos += n * np.dtype(dt).itemsize
        return a
    fe = _frontend(4)
    pipe = _pipe(fe, maps)
    for i in range(N):
        o = _copy(pipe.wait(pipe.submit(frames[i][None])))
        nkp = take("<i4", 4); kps = take("<f4", 4 * CAP * 2).reshape(4, CAP, 2)
        nbn = take("<i4", 4); nbq = take("<i4", 4 * CAP).reshape(4, CAP); nbt = take("<i4", 4 * CAP).reshape(4, CAP)
        pvn = take("<i4", 4); pvq = take("<i4", 4 * CAP).reshape(4, CAP); pvt = take("<i4", 4 * CAP).reshape(4, CAP)
        np.testing.assert_array_equal(nkp, o["n_kp"][0])
        for v in range(4):
            np.testing.assert_array_equal(kps[v, :nkp[v]], o["kps_xy"][0, v, :nkp[v]])
        np.testing.assert_array_equal(nbn, o["nb_n"][0]); np.testing.assert_array_equal(pvn, o["prev_n"][0])
        for p in range(4):
            np.testing.assert_array_equal(nbq[p, :nbn[p]], o["nb_q"][0, p, :nbn[p]]); np.testing.assert_array_equal(nbt[p, :nbn[p]], o["nb_t"][0, p, :nbn[p]])
            np.testing.assert_array_equal(pvq[p, :pvn[p]], o["prev_q"][0, p, :pvn[p]]); np.testing.assert_array_equal(pvt[p, :pvn[p]], o["prev_t"][0, p, :pvn[p]])
    assert pos == len(data)
    pipe.close(); fe.close()
