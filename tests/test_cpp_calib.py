"""The int8 calibration session through the C++ mirror (include/d2fe.hpp: D2FrontEnd::Int8Calibrator), built with g++ against the C ABI library as
tests/test_cpp_i8_mode.py builds its driver: compiles and links everywhere; on a GPU box tests/cpp/calib_test.cpp goes from frames to a working D2FE_PREC_I8
handle with the product library alone, and its twelve ranges per rule are compared bit for bit with the Python binding's on the same images."""
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
    exe = str(tmp_path / "calib_test")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "calib_test.cpp"),
           "-L", os.path.dirname(lib), "-ld2fe_hip", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib",
           "-Wl,--allow-shlib-undefined", "-o", exe]
    subprocess.check_call(cmd)
    return exe


def test_cpp_calib_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    assert os.path.exists(exe)
    assert subprocess.run([exe], capture_output=True).returncode == 2          # usage error path: runs without touching the GPU


@pytest.mark.gpu
def test_cpp_calib_equals_the_python_binding(tmp_path, sp_weights):
    from d2slam_amd import api
    exe = _build(tmp_path)
    H, W, n_img, n_bins = 96, 128, 3, 1024
    imgs = np.stack([synth_image(H, W, 50 + i) for i in range(n_img)]).astype(np.uint8)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<iiii", H, W, n_img, n_bins))
        for n in SP_LAYERS:
            wt, b = sp_weights[n]
            f.write(struct.pack("<iii", wt.shape[0], wt.shape[1], wt.shape[2]))
            f.write(np.ascontiguousarray(wt, "<f4").tobytes()); f.write(np.ascontiguousarray(b, "<f4").tobytes())
        f.write(imgs.tobytes())
    res = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.returncode, res.stderr[-1500:])
    assert "d2fe_calib_create" in res.stderr and "d2fe_calib_freeze" in res.stderr      # the refusals were reported
    got = np.fromfile(fout, "<f4").reshape(3, 12)
    fe = api.FrontEnd(api.SuperPointConfig(input_width=W, input_height=H, max_batch=2, precision=api.PREC_F32, dense_descriptors=True))
    fe.load_superpoint(sp_weights)
    cal = api.Int8Calibrator(fe, n_bins)
    cal.collect(imgs); cal.freeze(); cal.collect(imgs)
    want = [cal.ranges("minmax"), cal.ranges("entropy"), cal.ranges("percentile", 99.9)]
    fe.close()
    for row, r in zip(got, want):
        assert np.array_equal(row.view(np.uint32), np.array([r[n] for n in SP_LAYERS], np.float32).view(np.uint32))
