"""CPU checks of the single-camera pipe (include/d2fe.h: d2fe_pipe_camera.mono / .depth, d2fe_pipe_create_camera, d2fe_pipe_submit_depth, d2fe_pipe_depth_result_get, d2fe_depth_at_device):
the two options live in a struct of their own beside the closed d2fe_pipe_config and default to off, the new entry points are exported, and the NumPy restatement of the depth lookup's value
contract that the GPU tests hold the device to (tests/helpers/depth_ref.py) is pinned on a hand-written table."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.helpers import depth_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from d2slam_amd import build
    return C.CDLL(build.build())


def test_the_camera_struct_defaults_to_stereo_and_the_pipe_config_keeps_its_size(lib):
    """d2fe_pipe_config is closed at 96 bytes (its last ints are lr_lk and sp_lk): mono and depth live in d2fe_pipe_camera, which defaults to a stereo pipe"""
    from d2slam_amd.api import _PipeCamera, _PipeConfig
    c = _PipeConfig()
    for name, _ in _PipeConfig._fields_:        # poison: the defaults must be WRITTEN
        setattr(c, name, 77)
    lib.d2fe_pipe_default_config.restype = None
    lib.d2fe_pipe_default_config(C.byref(c))
    assert c.struct_size == C.sizeof(_PipeConfig) == 96 and c.lr_lk == 0 and c.sp_lk == 0 and not hasattr(c, "mono") and not hasattr(c, "depth")
    cam = _PipeCamera()
    for name, _ in _PipeCamera._fields_:
        setattr(cam, name, 77)
    lib.d2fe_pipe_camera_default.restype = None
    lib.d2fe_pipe_camera_default(C.byref(cam))
    assert cam.struct_size == C.sizeof(_PipeCamera) == 16 and cam.mono == 0 and cam.depth == 0 and cam.reserved == 0
    assert [n for n, _ in _PipeCamera._fields_] == ["struct_size", "mono", "depth", "reserved"]
    hdr = open(os.path.join(ROOT, "include", "d2fe.h")).read()
    body = hdr[hdr.index("/* sizeof(d2fe_pipe_camera), checked strictly */"):hdr.index("} d2fe_pipe_camera;")]
    assert body.index("int32_t mono;") < body.index("int32_t depth;") < body.index("int32_t reserved;")


def test_new_entry_points_are_exported(lib):
    from d2slam_amd import api
    for n in ("d2fe_pipe_camera_default", "d2fe_pipe_create_camera", "d2fe_pipe_submit_depth", "d2fe_pipe_depth_result_get", "d2fe_depth_at_device"):
        assert hasattr(lib, n) and n in api.EXPORTS
    assert C.sizeof(api._PipeDepthResult) == 16 + 2 * 8
    assert api.PROF_STAGES[-1] == "lk"          # no stage was added for the lookup


def test_header_layout_of_the_new_structs(tmp_path):
    """sizeof / offsetof as g++ sees include/d2fe.h against the ctypes mirrors"""
    import subprocess
    from d2slam_amd import api
    src = tmp_path / "probe.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "d2fe.h"\nint main() {\n'
                   '  std::printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(d2fe_pipe_camera), offsetof(d2fe_pipe_camera, mono), offsetof(d2fe_pipe_camera, depth),\n'
                   '              sizeof(d2fe_pipe_depth_result), offsetof(d2fe_pipe_depth_result, kp_depth_mm), offsetof(d2fe_pipe_depth_result, track_depth_mm));\n'
                   '  return 0;\n}\n')
    exe = str(tmp_path / "probe")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    P, R = api._PipeCamera, api._PipeDepthResult
    assert got == [C.sizeof(P), P.mono.offset, P.depth.offset, C.sizeof(R), R.kp_depth_mm.offset, R.track_depth_mm.offset]


def test_depth_restatement_on_a_hand_written_table():
    """np.rint is cvRound: 2.5 -> 2, 3.5 -> 4, -0.5 -> 0, -0.51 -> outside, W - 0.5 -> outside, NaN -> 0"""
    W, H = 24, 16
    depth = (np.arange(H * W, dtype=np.uint32).reshape(H, W) * 131 + 7).astype(np.uint16)      # every pixel its own value, none of them 0
    depth[H - 1, W - 1] = 65535
    assert (depth != 0).all() and len(np.unique(depth)) == H * W
    table = depth_ref.edge_table(W, H)
    pts = np.float32([p for p, _ in table])
    want = np.uint16([0 if at is None else depth[at[1], at[0]] for _, at in table])
    got = depth_ref.depth_at_np(depth, pts)
    assert got.dtype == np.uint16 and np.array_equal(got, want), [(table[i][0], int(got[i]), int(want[i])) for i in np.nonzero(got != want)[0]]
    by = {p: at for p, at in table}
    assert by[(2.5, 1.0)] == (2, 1) and by[(3.5, 1.0)] == (4, 1) and by[(-0.5, 0.0)] == (0, 0) and by[(-0.51, 0.0)] is None and by[(W - 0.5, 0.0)] is None
    assert depth_ref.depth_at_np(depth, np.zeros((0, 2), np.float32)).shape == (0,)
    d = depth_ref.seeded_depth(2, H, W, 5)
    assert d.dtype == np.uint16 and d.min() == 0 and d.max() == 65535


def test_the_lookup_neither_synchronises_nor_allocates():
    """d2fe_depth_at_device and the launcher the pipe calls only enqueue ONE launch; every read of the kernel is behind a bounds check"""
    src = open(os.path.join(ROOT, "d2slam_amd", "csrc", "depth.hip")).read()
    pipe = open(os.path.join(ROOT, "d2slam_amd", "csrc", "pipe.hip")).read()
    assert src.count("hipLaunchKernelGGL") == 1 and "depth_gather_kernel" in src
    for word in ("hipStreamSynchronize", "hipDeviceSynchronize", "hipEventSynchronize", "hipMalloc", "hipHostMalloc", "hipFree", "hipMemset"):
        assert word not in src, word
    i = pipe.index("int pipe_flush(d2fe_pipe_s* p) {")
    flush = pipe[i:pipe.index("\n}\n", i)]
    assert flush.count("depth_gather_launch(") == 1 and flush.index("depth_gather_launch(") < flush.index("hipMemcpyAsync(L.pin_out[set]")


def test_cpp_driver_compiles_and_links(tmp_path):
    """tests/cpp/mono_pipe_test.cpp (StereoPipe::submit(left) / submit(left, depth) through include/d2fe.hpp) builds with g++ -Wall -Werror; without arguments it
    leaves with 2 before touching a GPU"""
    import subprocess
    from d2slam_amd import build as hipbuild
    lib = hipbuild.build()
    exe = str(tmp_path / "mono_pipe_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "mono_pipe_test.cpp"),
                           "-L", os.path.dirname(lib), "-ld2fe_hip", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib",
                           "-Wl,--allow-shlib-undefined", "-o", exe])
    assert subprocess.run([exe], capture_output=True).returncode == 2
