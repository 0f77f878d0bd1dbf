"""D2FE_PREC_I8 through the C++ mirror (include/d2fe.hpp: SuperPointConfig::int8_operands, SuperPoint::setInt8Ranges), built with g++ against the C ABI
library as tests/test_cpp_mirror.py builds its driver: compiles and links everywhere; on a GPU box tests/cpp/i8_mode_test.cpp creates, loads, is refused
until the ranges are set, extracts twice, and its outputs are compared bit for bit with the Python binding's on the same image."""
import os
import struct
import subprocess

import numpy as np
import pytest

from d2slam_amd.synth import synth_image
from d2slam_amd.weights import SP_LAYERS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    from d2slam_amd import build as hipbuild
    lib = hipbuild.build()
    exe = str(tmp_path / "i8_mode_test")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "i8_mode_test.cpp"),
           "-L", os.path.dirname(lib), "-ld2fe_hip", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib",
           "-Wl,--allow-shlib-undefined", "-o", exe]
    subprocess.check_call(cmd)
    return exe


def test_cpp_i8_mode_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    assert os.path.exists(exe)
    assert subprocess.run([exe], capture_output=True).returncode == 2          # usage error path: runs without touching the GPU


def _read_vecs(path, dtypes):
    out, data, pos = [], open(path, "rb").read(), 0
    for dt in dtypes:
        n = struct.unpack_from("<i", data, pos)[0]; pos += 4
        out.append(np.frombuffer(data, dt, n, pos).copy()); pos += n * np.dtype(dt).itemsize
    assert pos == len(data)
    return out


@pytest.mark.gpu
def test_cpp_i8_mode_equals_the_python_binding(tmp_path, sp_weights):
    from d2slam_amd import api, calibrate
    exe = _build(tmp_path)
    H, W, maxkp = 96, 128, 100
    img = synth_image(H, W, 33)
    ranges = calibrate.measure_ranges(sp_weights, img[None])
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<iii", H, W, maxkp))
        for n in SP_LAYERS:
            wt, b = sp_weights[n]
            f.write(struct.pack("<iii", wt.shape[0], wt.shape[1], wt.shape[2]))
            f.write(np.ascontiguousarray(wt, "<f4").tobytes()); f.write(np.ascontiguousarray(b, "<f4").tobytes())
        f.write(np.array([ranges[n] for n in SP_LAYERS], "<f4").tobytes())
        f.write(img.tobytes())
    res = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.returncode, res.stderr[-1500:])
    assert "d2fe_set_superpoint_int8_ranges" in res.stderr and "conv2b" in res.stderr      # the refused table names its layer (index 3)
    kf, sc, de = _read_vecs(fout, ["<f4", "<f4", "<f4"])
    fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=maxkp, input_width=W, input_height=H, max_batch=1, precision=api.PREC_I8))
    fe.load_superpoint(sp_weights)
    fe.set_int8_ranges(ranges)
    (kps, s, d), = fe.extract_batch(img[None], cap=maxkp)
    fe.close()
    assert len(s) > 10
    assert np.array_equal(kf.reshape(-1, 2), kps) and np.array_equal(sc.view(np.uint32), s.view(np.uint32))
    assert np.array_equal(de.reshape(-1, 256).view(np.uint32), d.view(np.uint32))
