"""The bearings of the quad pipe through the C++ mirror (include/d2fe.hpp: QuadPipe::bearingsEnable, QuadPipe::bearings), built with g++ against the C ABI library as the
other tests/cpp drivers are, with no Python in the process.  tests/cpp/quad_bearings_test.cpp runs a flow_lk pipe (the bearings enabled BEFORE the list mode), two submits
in flight, checks sizes, refusals and the gate (exactly, on the device's own predictions) and writes the device's bearings and predictions beside the header's host
restatements on the same points; here the two are held to the bound of tests/helpers/cyl_bearings_ref.py (bearings) and to one fp32 unit in the last place (predictions,
away from atan2's jump), as tests/test_quad_bearings.py holds the device to the oracle."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.helpers import bearings_ref as br
from tests.helpers import cyl_bearings_ref as cr
from tests.helpers import quad_lk_ref as qref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_quad_bearings_through_the_cpp_mirror(tmp_path):
    from d2slam_amd import build as hipbuild
    from d2slam_amd.weights import save_superpoint_d2fw
    from tests.test_quad_bearings import CAP, FOV, H, PIPE_CAMS, RADIUS_LK, SEED, T_NB, W
    from tests.test_quad_pipe import _weights
    lib = hipbuild.build()
    exe = str(tmp_path / "quad_bearings_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "quad_bearings_test.cpp"), "-L", os.path.dirname(lib), "-ld2fe_hip", "-Wl,-rpath," + os.path.dirname(lib),
                           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-Wl,--allow-shlib-undefined", "-o", exe])
    assert FOV == 200.0
    nq, distance = 2, 100.0
    quads = qref.cyclic_quads(nq, SEED)
    sp, fin, fout = (str(tmp_path / n) for n in ("sp.d2fw", "in.bin", "out.bin"))
    save_superpoint_d2fw(sp, _weights())
    cam4 = lambda c: np.float64([c[k] for k in ("fx", "fy", "cx", "cy")])
    with open(fin, "wb") as f:
        f.write(struct.pack("<6i", nq, H, W, CAP, 100, 0))
        f.write(struct.pack("<d", 20.0))
        for c in PIPE_CAMS:
            f.write(cam4(c).tobytes())
        f.write(np.ascontiguousarray(T_NB, np.float64).tobytes()); f.write(struct.pack("<dd", distance, RADIUS_LK))
        for mm in qref.identity_maps():
            for m in mm[:2]:
                f.write(np.ascontiguousarray(m, np.float32).tobytes())
        f.write(quads.tobytes())
    res = subprocess.run([exe, sp, fin, fout], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.returncode, res.stdout, res.stderr)
    assert "quad_bearings_test OK" in res.stdout
    print(res.stdout.strip())
    data, pos = open(fout, "rb").read(), [0]

    def take(dt, cols):
        n = struct.unpack_from("<i", data, pos[0])[0]; pos[0] += 4
        a = np.frombuffer(data, dt, n, pos[0]).reshape(-1, cols); pos[0] += a.nbytes
        return a

    def hold(cam, pts, dev, host, what):
        assert len(pts) == len(dev) == len(host), what
        want = cr.bearings(cam, pts)
        assert np.array_equal(host, want, equal_nan=True), what          # the header's restatement IS the oracle's arithmetic (tests/test_quad_bearings_cpu.py)
        assert np.isfinite(want).all() and (np.abs(dev - want) <= cr.cyl_bearing_bound(cam, pts)).all(), what
        return len(pts)
    seen = 0
    for frame in range(nq):
        lists = []
        for c in range(4):
            pts, dev, host = take("<f4", 2), take("<f8", 3), take("<f8", 3)
            seen += hold(PIPE_CAMS[c], pts, dev, host, (frame, c, "keypoints"))
            pts, dev, host = take("<f4", 2), take("<f8", 3), take("<f8", 3)
            seen += hold(PIPE_CAMS[c], pts, dev, host, (frame, c, "list"))
            lists.append(pts)
        for n, (a, b, _) in enumerate(qref.NEIGHBOURS):
            dpred, hpred = take("<f4", 2), take("<f4", 2)
            wb = cr.bearings(PIPE_CAMS[a], lists[a])
            assert np.array_equal(hpred, cr.predict(PIPE_CAMS[a], T_NB[n], wb, distance), equal_nan=True), (frame, n)
            keep = ~cr.near_back_seam(br.transform(T_NB[n], wb, distance))
            assert len(dpred) == len(lists[a]) and br.within_fp32_ulp(dpred[keep], hpred[keep]).all(), (frame, n)
            pts, dev, host = take("<f4", 2), take("<f8", 3), take("<f8", 3)
            hold(PIPE_CAMS[b], pts, dev, host, (frame, n, "neighbour tracks"))
    assert pos[0] == len(data) and seen > 100
