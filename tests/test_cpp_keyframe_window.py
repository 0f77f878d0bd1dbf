"""tests/cpp/keyframe_window_test.cpp: the keyframe window (d2fe_window_*, include/d2fe.h) driven from g++ through include/d2fe.hpp (StereoPipe + KeyframeWindow),
no Python and no torch in the process -- push, retain, track in place through the device view, collect; every record held to the Python binding on the same frames
(which tests/test_keyframe_window.py holds to the host composition of the existing calls)."""
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, NK, LANES = 10, 5, 2


def _build_cpp(tmp_path):
    """keyframe_window_test.cpp links ONLY libd2fe_hip.so"""
    from d2slam_amd import build as hipbuild
    libpath = hipbuild.build()
    exe = str(tmp_path / "keyframe_window_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-result", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "keyframe_window_test.cpp"), "-L", os.path.dirname(libpath), "-ld2fe_hip",
                           "-Wl,-rpath," + os.path.dirname(libpath), "-Wl,--allow-shlib-undefined", "-o", exe])
    return exe


def test_cpp_keyframe_window_compiles_against_the_c_abi_alone(tmp_path):
    exe = _build_cpp(tmp_path)
    assert subprocess.run([exe], capture_output=True).returncode == 2          # usage error path: runs without touching the GPU
    ldd = subprocess.run(["ldd", exe], capture_output=True, text=True).stdout
    assert "libd2fe_hip" in ldd and "torch" not in ldd


@pytest.mark.gpu
def test_cpp_driver_equals_the_python_binding(tmp_path):
    from d2slam_amd import netvlad as nvm
    from d2slam_amd.weights import save_netvlad_d2fw, save_superpoint_d2fw, synthetic_superpoint_weights
    from tests import test_keyframe_window as tw
    from tests.helpers import keyframe_window_common as kw
    from tests.test_loop_query import _stereo_frames
    exe = _build_cpp(tmp_path)
    sp, nvp, fin, fout = (str(tmp_path / n) for n in ("sp.d2fw", "nv.d2fw", "in.bin", "out.bin"))
    save_netvlad_d2fw(nvp, nvm.synthetic_netvlad_weights(depth_multiplier=0.35))
    save_superpoint_d2fw(sp, synthetic_superpoint_weights(dustbin_bias=7.5))
    fr = _stereo_frames()[:N]
    imgs = np.stack([np.stack(p) for p in fr])                                  # [N][2][H][W]
    api, fe = tw._stereo_fe(2)
    G, cap = fe.netvlad_dim, tw.CAP
    mk = lambda: api.StereoPipe(fe, lanes=LANES, frames=1, width=tw.W, height=tw.H, cap=cap, netvlad=True)
    # the pipe alone: the NetVLAD vectors, and a threshold in the widest gap of the tracked frames' best similarities
    pipe = mk()
    nv = np.stack([pipe.wait(pipe.submit(imgs[i, 0][None], imgs[i, 1][None]))["netvlad"][0].copy() for i in range(N)])
    pipe.close()
    kept = [0, 2, NK - 1]
    best = np.sort(kw.sims64(nv[NK:, None], nv[kept][:, None], 1).reshape(N - NK, -1).max(axis=1))
    g = int(np.argmax(np.diff(best)))
    thres = float(0.5 * (best[g] + best[g + 1]))
    # the Python binding, the same calls in the same order
    pipe = mk()
    win = api.KeyframeWindow(pipe, capacity=NK, thres=thres, slots=2, max_queries=1)
    col = []
    for i in range(N):
        t = pipe.submit(imgs[i, 0][None], imgs[i, 1][None])
        if i < NK:
            win.push(t, 0, 100 + i); win.push(t, 0, 100 + i)
            if i == NK - 1:
                assert win.retain([100, 102, 77]) == NK - 3
            pipe.wait(t)
            continue
        v = pipe.device_view(t, win.stream)
        win.track_device(v.d_netvlad, G, v.d_desc, cap * tw.D, v.d_n_kp, 1, 1, i % 2, None)
        pipe.device_release(t, win.stream)
        pipe.wait(t)
        col.append(tw._copy(win.collect(i % 2)))
    tags = win.tags()
    assert tags == [100, 102, 100 + NK - 1]
    win.close(); pipe.close(); fe.close()
    with open(fin, "wb") as f:
        f.write(struct.pack("<4if", N, tw.H, tw.W, cap, 0.015))
        f.write(np.ascontiguousarray(imgs).tobytes())
    res = subprocess.run([exe, sp, nvp, fin, fout, str(LANES), str(NK), repr(thres)], capture_output=True, text=True, timeout=300)
    print(res.stdout)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "keyframe_window_test OK" in res.stdout
    data = open(fout, "rb").read()
    pos = 0

    def take(dt, n):
        nonlocal pos
        a = np.frombuffer(data, dtype=dt, count=n, offset=pos)
        pos += a.itemsize * n
        return a
    hits = 0
    for c in col:
        assert take(np.int64, 1)[0] == c["keyframe_tag"][0]
        assert list(take(np.int32, 4)) == [int(c["keyframe_pos"][0]), int(c["dir_a"][0]), int(c["dir_b"][0]), c["n_window"]]
        assert take(np.uint32, 1)[0] == tw._bits(c["sim"])[0]
        assert np.array_equal(take(np.uint32, NK), tw._bits(c["sims"][0, :, 0]))
        m = int(c["n_match"][0, 0])
        assert list(take(np.int32, 3)) == [int(c["local_view"][0, 0]), int(c["remote_view"][0, 0]), m]
        for k, dt in (("q_idx", np.int32), ("t_idx", np.int32), ("dist", np.uint32)):
            got = take(dt, cap)
            assert np.array_equal(got[:m], np.ascontiguousarray(c[k][0, 0, :m]).view(dt)) and not got[m:].any(), k
        hits += int(c["keyframe_pos"][0]) >= 0
    assert take(np.int32, 1)[0] == len(tags) and list(take(np.int64, len(tags))) == tags and pos == len(data)
    assert 1 <= hits < len(col)                                                 # a scene seen again was found, an unseen one was not
