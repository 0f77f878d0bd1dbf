"""CPU checks of the quad pipe's C ABI (d2fe_quad_pipe_*, include/d2fe.h): every declared entry point is exported, the ctypes mirrors of d2slam_amd/api.py
have the header's layout (sizeof / offsetof printed by a g++ probe built here), the documented defaults, the argument checks that need no device, and the
C++ driver tests/cpp/quad_pipe_test.cpp compiles against the header and links only libd2fe_hip.so."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUAD = ["d2fe_quad_pipe_default_config", "d2fe_quad_pipe_create", "d2fe_quad_pipe_destroy", "d2fe_quad_pipe_submit", "d2fe_quad_pipe_wait",
        "d2fe_quad_pipe_lanes", "d2fe_quad_pipe_geometry", "d2fe_quad_undistort_device"]


@pytest.fixture(scope="module")
def lib():
    from d2slam_amd import build
    return C.CDLL(build.build())


def test_every_quad_entry_point_is_declared_and_exported(lib):
    src = open(os.path.join(ROOT, "include", "d2fe.h")).read()
    declared = sorted(n for n in set(re.findall(r"D2FE_API\s+[\w\s\*]+?\b(d2fe_\w+)\s*\(", src)) if n.startswith("d2fe_quad_pipe_") or n == "d2fe_quad_undistort_device")
    assert declared == sorted(QUAD)
    from d2slam_amd import api
    for n in declared:
        assert hasattr(lib, n), n
        assert n in api.EXPORTS, n


_PROBE = r"""
#include <cstddef>
#include <cstdio>
#include "d2fe.h"
#define F(T, f) std::printf("%s %s %zu\n", #T, #f, offsetof(T, f));
int main() {
  std::printf("d2fe_quad_pipe_config sizeof %zu\n", sizeof(d2fe_quad_pipe_config));
  std::printf("d2fe_quad_maps sizeof %zu\n", sizeof(d2fe_quad_maps));
  std::printf("d2fe_quad_pipe_result sizeof %zu\n", sizeof(d2fe_quad_pipe_result));
@FIELDS@
  return 0;
}
"""


def test_ctypes_mirrors_match_the_header(tmp_path):
    from d2slam_amd import api
    structs = {"d2fe_quad_pipe_config": api._QuadPipeConfig, "d2fe_quad_maps": api._QuadMaps, "d2fe_quad_pipe_result": api._QuadPipeResult}
    fields = "".join("  F(%s, %s)\n" % (t, f[0]) for t, s in structs.items() for f in s._fields_)
    src = tmp_path / "probe.cpp"
    src.write_text(_PROBE.replace("@FIELDS@", fields))
    exe = str(tmp_path / "probe")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    got = {(a, b): int(c) for a, b, c in (l.split() for l in out.splitlines() if l.strip())}
    for t, s in structs.items():
        assert got[(t, "sizeof")] == C.sizeof(s), t
        for f in s._fields_:
            assert got[(t, f[0])] == getattr(s, f[0]).offset, (t, f[0])


def test_default_config(lib):
    from d2slam_amd import api
    c = api._QuadPipeConfig()
    lib.d2fe_quad_pipe_default_config(C.byref(c))
    assert c.struct_size == C.sizeof(api._QuadPipeConfig)
    assert (c.lanes, c.quads, c.raw_width, c.raw_height, c.width, c.height, c.cap) == (4, 1, 1280, 800, 800, 400, 100)
    assert (c.netvlad, c.match_neighbour, c.match_prev, c.pinned_input) == (1, 1, 1, 0)
    assert (c.ratio, c.radius_neighbour, c.radius_prev, c.undistort_fov) == (0.8, 160.0, -1.0, 200.0)
    assert list(c.reserved) == [0] * 8


def test_null_arguments_are_refused_without_a_device(lib):
    from d2slam_amd import api
    lib.d2fe_last_error.restype = C.c_char_p
    c = api._QuadPipeConfig()
    lib.d2fe_quad_pipe_default_config(C.byref(c))
    m = api._QuadMaps()
    p = C.c_void_p()
    assert lib.d2fe_quad_pipe_create(None, C.byref(c), C.byref(m), C.byref(p)) == -1 and not p.value
    assert b"null argument" in lib.d2fe_last_error()
    assert lib.d2fe_quad_pipe_lanes(None) == -1
    t = C.c_int64(-1)
    assert lib.d2fe_quad_pipe_submit(None, None, 0, C.c_size_t(0), C.c_size_t(0), C.byref(t)) == -1
    assert lib.d2fe_quad_undistort_device(None, None, 1, 8, 8, 8, C.c_size_t(64), C.c_size_t(256), C.byref(m), 4, 4, None, None) == -1
    lib.d2fe_quad_pipe_destroy(None)


def _build_cpp(tmp_path):
    """quad_pipe_test.cpp links ONLY libd2fe_hip.so"""
    from d2slam_amd import build as hipbuild
    libpath = hipbuild.build()
    exe = str(tmp_path / "quad_pipe_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-result", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "quad_pipe_test.cpp"), "-L", os.path.dirname(libpath), "-ld2fe_hip",
                           "-Wl,-rpath," + os.path.dirname(libpath), "-Wl,--allow-shlib-undefined", "-o", exe])
    return exe


def test_cpp_quad_pipe_compiles_against_the_c_abi_alone(tmp_path):
    exe = _build_cpp(tmp_path)
    assert subprocess.run([exe], capture_output=True).returncode == 2          # usage error path: runs without touching the GPU
    ldd = subprocess.run(["ldd", exe], capture_output=True, text=True).stdout
    assert "libd2fe_hip" in ldd and "torch" not in ldd
