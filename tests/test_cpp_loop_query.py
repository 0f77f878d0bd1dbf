"""tests/cpp/loop_query_test.cpp: the loop query (d2fe_loop_*, include/d2fe.h) driven from g++ through include/d2fe.hpp (StereoPipe / QuadPipe + LoopQuery), no
Python and no torch in the process -- one stereo and one quad sequence, every record held to the Python binding on the same frames (which tests/test_loop_query.py
holds to the host composition of the existing calls)."""
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_cpp(tmp_path):
    """loop_query_test.cpp links ONLY libd2fe_hip.so"""
    from d2slam_amd import build as hipbuild
    libpath = hipbuild.build()
    exe = str(tmp_path / "loop_query_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-result", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "loop_query_test.cpp"), "-L", os.path.dirname(libpath), "-ld2fe_hip",
                           "-Wl,-rpath," + os.path.dirname(libpath), "-Wl,--allow-shlib-undefined", "-o", exe])
    return exe


def test_cpp_loop_query_compiles_against_the_c_abi_alone(tmp_path):
    exe = _build_cpp(tmp_path)
    assert subprocess.run([exe], capture_output=True).returncode == 2          # usage error path: runs without touching the GPU
    ldd = subprocess.run(["ldd", exe], capture_output=True, text=True).stdout
    assert "libd2fe_hip" in ldd and "torch" not in ldd


def _binding(api, pipe, submits, masks, thres, max_index, N):
    from tests.test_loop_query import _drive
    loop = api.LoopQuery(pipe, capacity_keyframes=N, max_index=max_index, thres=thres, slots=pipe.lanes + 1)
    _, col = _drive(api, pipe, submits, loop, masks, [api.LOOP_QUERY | api.LOOP_ADD] * len(submits))
    tail = (loop.ntotal, loop.keyframes)
    loop.close()
    return col, tail


def _compare(data, col, tail, F, V, cap):
    pos = 0

    def take(dt, n):
        nonlocal pos
        a = np.frombuffer(data, dtype=dt, count=n, offset=pos)
        pos += 4 * n
        return a
    hits = 0
    for c in col:
        for f in range(F):
            head = take(np.int32, 5)
            assert list(head) == [int(c[k][f]) for k in ("queried", "label", "keyframe", "dir_old", "ntotal_at_query")]
            assert take(np.uint32, 1)[0] == np.ascontiguousarray(c["sim"][f:f + 1]).view(np.uint32)[0]
            for k in ("added_label", "dir_a", "dir_b", "n_match"):
                assert np.array_equal(take(np.int32, V), c[k][f]), k
            nm = c["n_match"][f]
            for k, dt in (("q_idx", np.int32), ("t_idx", np.int32), ("dist", np.uint32)):
                got = take(dt, V * cap).reshape(V, cap)
                for i in range(V):
                    assert np.array_equal(got[i, :nm[i]], np.ascontiguousarray(c[k][f, i, :nm[i]]).view(dt)) and not got[i, nm[i]:].any(), k
            hits += int(head[1]) >= 0
    assert tuple(take(np.int32, 2)) == tail and pos == len(data)
    return hits


@pytest.mark.gpu
@pytest.mark.parametrize("kind,lanes,F", [(0, 2, 1), (1, 2, 2)])
def test_cpp_driver_equals_the_python_binding(tmp_path, kind, lanes, F):
    from d2slam_amd import api, netvlad as nvm
    from d2slam_amd.weights import save_netvlad_d2fw, save_superpoint_d2fw
    from tests import test_loop_query as tl
    exe = _build_cpp(tmp_path)
    sp, nvp, fin, fout = (str(tmp_path / n) for n in ("sp.d2fw", "nv.d2fw", "in.bin", "out.bin"))
    nv = nvm.synthetic_netvlad_weights(depth_multiplier=0.35)
    save_netvlad_d2fw(nvp, nv)
    MI, thres = 2, -1.0                                                         # every queried frame with an allowed row is a hit: the matcher runs for all of them
    if kind == 0:
        from d2slam_amd.weights import synthetic_superpoint_weights
        w, kthr, H, W = synthetic_superpoint_weights(dustbin_bias=7.5), 0.015, tl.H, tl.W
        fr = tl._stereo_frames()
        imgs = np.stack([np.stack(p) for p in fr])                              # [N][2][H][W]
        key = np.array(tl.STEREO_KEY, np.uint8)
        api_, fe = tl._stereo_fe(2 * F)
        pipe = api.StereoPipe(fe, lanes=lanes, frames=F, width=W, height=H, cap=tl.CAP, netvlad=True)
        submits = [(imgs[i * F:(i + 1) * F, 0], imgs[i * F:(i + 1) * F, 1]) for i in range(len(imgs) // F)]
    else:
        from tests.helpers import quad_lk_ref as qref
        from tests.test_quad_pipe import _weights
        w, kthr, H, W = _weights(), 0.15, qref.H, qref.W
        imgs = tl._quad_frames()                                                # [N][4][H][W]
        key = np.ones(len(imgs), np.uint8); key[5] = 0
        fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=tl.CAP, input_width=W, input_height=H, max_batch=4 * F, keypoint_threshold=kthr, precision=api.PREC_F32_WINO))
        fe.load_superpoint(w); fe.load_netvlad(nv)
        pipe = api.QuadPipe(fe, qref.identity_maps(), lanes=lanes, quads=F, raw_width=W, raw_height=H, width=W, height=H, cap=tl.CAP, radius_neighbour=0.2 * W,
                            undistort_fov=qref.FOV, netvlad=True, match_neighbour=False, match_prev=False)
        submits = [(imgs[i * F:(i + 1) * F],) for i in range(len(imgs) // F)]
    save_superpoint_d2fw(sp, w)
    N, V = len(imgs), 4 if kind else 1
    masks = [key[i * F:(i + 1) * F] for i in range(N // F)]
    col, tail = _binding(api, pipe, submits, masks, thres, MI, N)
    pipe.close(); fe.close()
    with open(fin, "wb") as f:
        f.write(struct.pack("<4if", N, H, W, tl.CAP, kthr))
        f.write(key.tobytes()); f.write(np.ascontiguousarray(imgs).tobytes())
    res = subprocess.run([exe, sp, nvp, fin, fout, str(kind), str(lanes), str(F), repr(thres), str(MI)], capture_output=True, text=True, timeout=300)
    print(res.stdout)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "loop_query_test OK" in res.stdout
    hits = _compare(open(fout, "rb").read(), col, tail, F, V, tl.CAP)
    assert hits >= 1                                                            # a scene seen again was found
