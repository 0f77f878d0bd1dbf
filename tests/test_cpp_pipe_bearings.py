"""The bearings of the stereo pipe through the C++ mirror (include/d2fe.hpp: StereoPipe::bearingsEnable, StereoFrameResult::bearings), built with g++ against the C ABI
library as the other tests/cpp drivers are.  tests/cpp/pipe_bearings_test.cpp runs an lr_lk + sp_lk pipe, checks sizes, refusals and the gate (exactly, on the device's own
predictions) and writes the device's bearings and predictions beside the header's host restatements on the same points; here the two are held to the bound of
tests/helpers/bearings_ref.py (bearings) and to one fp32 unit in the last place (predictions), as tests/test_bearings.py holds the device to the NumPy oracle."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.helpers import bearings_ref as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bearings_through_the_cpp_mirror(tmp_path, sp_weights):
    from d2slam_amd import build as hipbuild
    from d2slam_amd.synth import synth_stereo
    from d2slam_amd.weights import SP_LAYERS
    lib = hipbuild.build()
    exe = str(tmp_path / "pipe_bearings_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "pipe_bearings_test.cpp"), "-L", os.path.dirname(lib), "-ld2fe_hip", "-Wl,-rpath," + os.path.dirname(lib),
                           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-Wl,--allow-shlib-undefined", "-o", exe])
    h, w, maxkp = 128, 192, 64
    l, r = synth_stereo(h, w, seed=5100)
    cam_l = br.pinhole(150.0, 151.0, 96.5, 63.0, 0.01, -0.02, 0.001, -0.0005)
    cam_r = br.pinhole(149.0, 150.5, 95.0, 64.5, -0.015, 0.01, -0.0005, 0.001)
    T = br.relative_extrinsic([1, 0, 0, 0], [0, 0, 0], br.quat_axis_angle([0.1, 1, 0.05], 1.0), [0.1, 0.004, -0.002]).reshape(-1)
    distance, radius = 100.0, 11.0
    pin8 = lambda c: np.float64([c[k] for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2")])
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<iii", h, w, maxkp))
        for n in SP_LAYERS:
            wt, b = sp_weights[n]
            f.write(struct.pack("<iii", wt.shape[0], wt.shape[1], wt.shape[2]))
            f.write(np.ascontiguousarray(wt, "<f4").tobytes()); f.write(np.ascontiguousarray(b, "<f4").tobytes())
        f.write(l.tobytes()); f.write(r.tobytes())
        f.write(pin8(cam_l).tobytes()); f.write(pin8(cam_r).tobytes()); f.write(T.tobytes()); f.write(struct.pack("<dd", distance, radius))
    res = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.returncode, res.stdout, res.stderr)
    print(res.stdout.strip())
    data, pos = open(fout, "rb").read(), [0]

    def take(dt, cols):
        n = struct.unpack_from("<i", data, pos[0])[0]; pos[0] += 4
        a = np.frombuffer(data, dt, n, pos[0]).reshape(-1, cols); pos[0] += a.nbytes
        return a

    def hold(cam, pts, dev, host, what):
        assert len(pts) == len(dev) == len(host) > 0, what
        want = br.bearings(cam, pts)
        assert np.array_equal(host, want, equal_nan=True), what          # the header's restatement IS the oracle's arithmetic (tests/test_bearings_cpu.py)
        ok = np.isfinite(want).all(1)
        assert np.array_equal(np.isnan(dev), np.isnan(want)) and (np.abs(dev[ok] - want[ok]) <= br.bearing_bound(cam, pts[ok])).all(), what
    for frame in range(3):
        pts, dev, host, dpred, hpred = take("<f4", 2), take("<f8", 3), take("<f8", 3), take("<f4", 2), take("<f4", 2)
        hold(cam_l, pts, dev, host, (frame, "keypoints"))
        assert br.within_fp32_ulp(dpred, hpred).all() and np.array_equal(hpred, br.predict(cam_l, T, br.bearings(cam_l, pts), distance)), frame
        pts, dev, host, dpred, hpred = take("<f4", 2), take("<f8", 3), take("<f8", 3), take("<f4", 2), take("<f4", 2)
        hold(cam_l, pts, dev, host, (frame, "list"))
        assert br.within_fp32_ulp(dpred, hpred).all() and np.array_equal(hpred, br.predict(cam_l, T, br.bearings(cam_l, pts), distance)), frame
        pts, dev, host = take("<f4", 2), take("<f8", 3), take("<f8", 3)
        hold(cam_r, pts, dev, host, (frame, "right tracks"))
    assert pos[0] == len(data)
