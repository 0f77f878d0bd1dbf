"""CPU checks of the stereo pipe's lr_lk mode (include/d2fe.h): the option takes one of d2fe_pipe_config's reserved ints, the new entry points are
exported, and the workspace arithmetic of d2fe_lk_track_stereo_device is the oracle's pyramid layout."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def lib():
    from d2slam_amd import build
    return C.CDLL(build.build())


def test_pipe_config_keeps_its_size_and_defaults_to_superpoint_on_both_images(lib):
    from d2slam_amd.api import _PipeConfig
    c = _PipeConfig()
    for name, _ in _PipeConfig._fields_:        # poison: the default must be WRITTEN
        if name != "reserved":
            setattr(c, name, 77)
    lib.d2fe_pipe_default_config.restype = None
    lib.d2fe_pipe_default_config(C.byref(c))
    assert c.lr_lk == 0
    assert c.struct_size == C.sizeof(_PipeConfig)
    # the struct before the option existed: 10 int32, 3 doubles, 6 int32, reserved[2] = 96 bytes; lr_lk took one of the two reserved ints
    assert C.sizeof(_PipeConfig) == 96
    assert _PipeConfig.lr_lk.offset == 88 and _PipeConfig.coalesce_depth.offset == 84 and _PipeConfig.ratio.offset == 40
    assert (c.match_lr, c.match_prev, c.netvlad, c.coalesce, c.netvlad_inline) == (1, 1, 1, 1, 2)


def test_new_entry_points_are_exported(lib):
    from d2slam_amd import api
    for n in ("d2fe_pipe_lk_result_get", "d2fe_lk_track_stereo_device", "d2fe_lk_stereo_workspace_bytes"):
        assert hasattr(lib, n) and n in api.EXPORTS
    assert api.PROF_STAGES[-1] == "lk" and api.PROF_STAGES[-2] == "netvlad" and api.PROF_STAGES.index("match") == 14


def test_stereo_workspace_bytes_is_two_pyramids_per_frame(lib, orc):
    """no GPU needed; the header documents no padding: exactly 2 * n_frames pyramids in the layout of a d2fe_lk_frame"""
    from d2slam_amd import api
    lib.d2fe_lk_stereo_workspace_bytes.restype = C.c_size_t
    lib.d2fe_lk_stereo_workspace_bytes.argtypes = [C.c_int] * 4
    for w, h, levels in ((640, 480, 2), (800, 400, 2), (33, 17, 3)):
        total = orc.pyr_layout(w, h, levels)[0]
        for n in (1, 5, 32):
            assert lib.d2fe_lk_stereo_workspace_bytes(n, w, h, levels) == 2 * n * total
            assert api.lk_stereo_workspace_bytes(n, w, h, levels) == 2 * n * total
    assert orc.pyr_layout(640, 480, 2)[0] == 640 * 480 + 320 * 240 + 160 * 120
    # what d2fe_lk_track_stereo_device would refuse
    for bad in ((0, 640, 480, 2), (1, 8, 480, 2), (1, 640, 480, 8), (1, 640, 480, -1)):
        assert lib.d2fe_lk_stereo_workspace_bytes(*bad) == 0


def _body(src, head):
    """text of the function whose definition starts with `head`, up to the closing brace in column 0"""
    i = src.index(head)
    return src[i:src.index("\n}\n", i)]


def test_the_lk_stage_neither_synchronises_nor_allocates():
    """the submit path of the mode: d2fe_lk_track_stereo_device (what the pipe calls) and pipe_flush (where it calls it) only enqueue"""
    import os
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "d2slam_amd", "csrc")
    lk = open(os.path.join(csrc, "lk.hip")).read()
    pipe = open(os.path.join(csrc, "pipe.hip")).read()
    track = _body(lk, "int d2fe_lk_track_stereo_device(")
    flush = _body(pipe, "int pipe_flush(d2fe_pipe_s* p) {")
    assert "lk_track_stereo_kernel" in track and "pyr_down_batch_kernel" in track and "d2fe_lk_track_stereo_device(" in flush
    for text in (track, flush, _body(lk, "size_t d2fe_lk_stereo_workspace_bytes(")):
        for word in ("hipStreamSynchronize", "hipDeviceSynchronize", "hipEventSynchronize", "hipMalloc", "hipHostMalloc", "hipFree", "hipMemset", "ctx_scratch"):
            assert word not in text, word
    # the kernels of the stage call the tracker's device functions, not copies of them
    kern = lk[lk.index("void lk_track_stereo_kernel("):lk.index("// ---- FAST-9/16")]
    assert kern.count("lk_calc(") == 2 and "tex(" not in kern


def test_cpp_driver_of_the_mode_compiles_and_links(tmp_path):
    """tests/cpp/pipe_lk_test.cpp (StereoPipe with cfg.lr_lk through include/d2fe.hpp) builds with g++ -Werror; without arguments it leaves before touching a GPU"""
    import os
    import subprocess
    from d2slam_amd import build as hipbuild
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = hipbuild.build()
    exe = str(tmp_path / "pipe_lk_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "pipe_lk_test.cpp"),
                           "-L", os.path.dirname(lib), "-ld2fe_hip", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib",
                           "-Wl,--allow-shlib-undefined", "-o", exe])
    assert subprocess.run([exe], capture_output=True).returncode == 2
