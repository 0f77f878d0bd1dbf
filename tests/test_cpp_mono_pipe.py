"""The single-camera pipe through the C++ mirror (include/d2fe.hpp: StereoPipe::submit(left), submit(left, depth), StereoFrameResult::depth_mm,
StereoTrackList::depth_mm), built with g++ against the C ABI library as the other tests/cpp drivers are: tests/cpp/mono_pipe_test.cpp holds the mirror's results
to the C ABI's byte for byte (no Python in that process); here its depth values are held to the NumPy restatement of the value contract."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.helpers import depth_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_mono_and_depth_through_the_cpp_mirror(tmp_path, sp_weights):
    from d2slam_amd import build as hipbuild
    from d2slam_amd.synth import synth_stereo
    from d2slam_amd.weights import SP_LAYERS
    lib = hipbuild.build()
    exe = str(tmp_path / "mono_pipe_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "mono_pipe_test.cpp"),
                           "-L", os.path.dirname(lib), "-ld2fe_hip", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib",
                           "-Wl,--allow-shlib-undefined", "-o", exe])
    h, w, maxkp = 128, 192, 64
    l, r = synth_stereo(h, w, seed=5100)
    wide = np.zeros((h, w + 8), np.uint16)
    wide[:, :w] = depth_ref.seeded_depth(1, h, w, 77)[0]
    wide[:, w:] = 4242                                     # the padding of a row: never a valid answer
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<iii", h, w, maxkp))
        for n in SP_LAYERS:
            wt, b = sp_weights[n]
            f.write(struct.pack("<iii", wt.shape[0], wt.shape[1], wt.shape[2]))
            f.write(np.ascontiguousarray(wt, "<f4").tobytes()); f.write(np.ascontiguousarray(b, "<f4").tobytes())
        f.write(l.tobytes()); f.write(r.tobytes()); f.write(wide.tobytes())
    res = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.returncode, res.stdout, res.stderr)
    print(res.stdout.strip())
    data, pos = open(fout, "rb").read(), 0
    for frame in range(3):
        for what in ("keypoints", "list"):
            n = struct.unpack_from("<i", data, pos)[0]; pos += 4
            pts = np.frombuffer(data, "<f4", n, pos).reshape(-1, 2); pos += 4 * n
            m = struct.unpack_from("<i", data, pos)[0]; pos += 4
            dep = np.frombuffer(data, "<u2", m, pos); pos += 2 * m
            assert m == len(pts) > 0
            assert np.array_equal(dep, depth_ref.depth_at_np(wide[:, :w], pts)), (frame, what)
    assert pos == len(data)
