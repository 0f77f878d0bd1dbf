"""CPU checks of the quad exchange's C ABI (d2fe_quad_exchange_*, d2fe_quad_device_*, d2fe_quad_lane_stream, d2fe_quad_handle; include/d2fe.h,
csrc/quad_exchange.hip): every declared entry point is exported and listed, the ctypes mirrors have the header's layout (sizeof / offsetof printed by a g++ probe
built here), the documented defaults, the argument checks that need no device, the job layout of the C code against its Python statement
(swarm.quad_remote_job_layout) at world 1 + loopback, 2, 4 and 8, and the C++ driver tests/cpp/quad_exchange_test.cpp compiles against include/ alone."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["d2fe_quad_device_view", "d2fe_quad_device_release", "d2fe_quad_lane_stream", "d2fe_quad_handle",
         "d2fe_quad_exchange_default_config", "d2fe_quad_exchange_create", "d2fe_quad_exchange_destroy", "d2fe_quad_exchange_enqueue",
         "d2fe_quad_exchange_collect", "d2fe_quad_exchange_jobs", "d2fe_quad_exchange_pairs", "d2fe_quad_exchange_block_bytes", "d2fe_quad_exchange_stream",
         "d2fe_quad_exchange_gathered", "d2fe_quad_exchange_job_layout"]
INVALID = -1


@pytest.fixture(scope="module")
def lib():
    from d2slam_amd import build
    l = C.CDLL(build.build())
    l.d2fe_last_error.restype = C.c_char_p
    return l


def test_every_quad_exchange_entry_point_is_declared_exported_and_listed(lib):
    src = open(os.path.join(ROOT, "include", "d2fe.h")).read()
    declared = sorted(n for n in set(re.findall(r"D2FE_API\s+[\w\s\*]+?\b(d2fe_\w+)\s*\(", src))
                      if n.startswith(("d2fe_quad_exchange_", "d2fe_quad_device_")) or n in ("d2fe_quad_lane_stream", "d2fe_quad_handle"))
    assert declared == sorted(NAMES)
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
  std::printf("d2fe_quad_exchange_config sizeof %zu\n", sizeof(d2fe_quad_exchange_config));
  std::printf("d2fe_quad_exchange_result sizeof %zu\n", sizeof(d2fe_quad_exchange_result));
  std::printf("d2fe_quad_device_result sizeof %zu\n", sizeof(d2fe_quad_device_result));
@FIELDS@
  return 0;
}
"""


def test_ctypes_mirrors_match_the_header(tmp_path):
    from d2slam_amd import api
    structs = {"d2fe_quad_exchange_config": api._QuadExchangeConfig, "d2fe_quad_exchange_result": api._QuadExchangeResult,
               "d2fe_quad_device_result": api._QuadDeviceResult}
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
    # the field lists are complete: every member the header declares has a mirror
    hdr = open(os.path.join(ROOT, "include", "d2fe.h")).read()
    for t, s in structs.items():
        body = hdr[:hdr.index("} %s;" % t)]
        body = re.sub(r"/\*.*?\*/", "", body[body.rindex("typedef struct {"):].replace("typedef struct {", ""), flags=re.S)
        names = []
        for decl in body.split(";"):
            decl = re.sub(r"^\s*(const\s+)?(int64_t|int32_t|float|double|d2fe_all_gather_fn|void)\s*\**\s*", "", decl.strip())
            names += [re.sub(r"\[.*\]|\*", "", n).strip() for n in decl.split(",") if n.strip()]
        assert names == [f[0] for f in s._fields_], (t, names)


def test_default_config(lib):
    from d2slam_amd import api
    c = api._QuadExchangeConfig()
    lib.d2fe_quad_exchange_default_config(C.byref(c))
    assert c.struct_size == C.sizeof(api._QuadExchangeConfig)
    assert (c.world, c.rank, c.wire, c.loopback, c.slots, c.own_stream, c.timing, c.mode) == (1, 0, 0, 0, 4, 1, 0, 0)
    assert (c.gate_thres, c.ratio) == (0.8, 0.8)
    assert not c.all_gather and not c.all_gather_user and list(c.reserved) == [0] * 6 and c.reserved0 == 0
    lib.d2fe_quad_exchange_default_config(None)


def test_bad_arguments_are_refused_without_a_device(lib):
    from d2slam_amd import api
    ok = api.ALL_GATHER_FN(lambda *a: 0)

    def create(pipe=None, **kw):
        c = api._QuadExchangeConfig()
        lib.d2fe_quad_exchange_default_config(C.byref(c))
        for k, v in kw.items():
            setattr(c, k, v)
        x = C.c_void_p()
        rc = lib.d2fe_quad_exchange_create(pipe, None, C.byref(c), C.byref(x))
        assert not x.value
        return rc, lib.d2fe_last_error()
    rc, msg = create(world=1, loopback=0, all_gather=ok)
    assert rc == INVALID and b"nothing to exchange" in msg                   # world 1 without loopback
    rc, msg = create(world=2, rank=0)
    assert rc == INVALID and b"neither an RCCL communicator nor" in msg       # neither communicator nor callback
    rc, msg = create(world=2, rank=2, all_gather=ok)
    assert rc == INVALID and b"bad quad exchange configuration" in msg
    rc, msg = create(world=2, rank=0, mode=2, all_gather=ok)
    assert rc == INVALID and b"bad quad exchange configuration" in msg
    rc, msg = create(world=2, rank=0, mode=1, all_gather=ok)                  # gated mode and no pipe that has NetVLAD (no pipe at all: the GPU suite has the real case)
    assert rc == INVALID
    x = C.c_void_p()
    assert lib.d2fe_quad_exchange_create(None, None, None, C.byref(x)) == INVALID
    # bad slot / null exchange
    r = api._QuadExchangeResult()
    assert lib.d2fe_quad_exchange_enqueue(None, C.c_int64(0), -1) == INVALID
    assert lib.d2fe_quad_exchange_enqueue(None, C.c_int64(0), 0) == INVALID
    assert lib.d2fe_quad_exchange_collect(None, -1, C.byref(r)) == INVALID
    for nm in ("d2fe_quad_exchange_jobs", "d2fe_quad_exchange_pairs", "d2fe_quad_exchange_block_bytes"):
        getattr(lib, nm).argtypes = [C.c_void_p]
        assert getattr(lib, nm)(None) == INVALID
    lib.d2fe_quad_exchange_stream.restype = C.c_void_p
    assert lib.d2fe_quad_exchange_stream(None) is None
    assert lib.d2fe_quad_exchange_gathered(None, 0, None, None) == INVALID
    lib.d2fe_quad_exchange_destroy(None)
    # the device view's entry points
    v = api._QuadDeviceResult()
    st = C.c_void_p()
    assert lib.d2fe_quad_device_view(None, C.c_int64(0), C.c_void_p(1), C.byref(v)) == INVALID
    assert lib.d2fe_quad_device_release(None, C.c_int64(0), C.c_void_p(1)) == INVALID
    assert lib.d2fe_quad_lane_stream(None, C.c_int64(0), C.byref(st)) == INVALID
    lib.d2fe_quad_handle.restype = C.c_void_p
    assert lib.d2fe_quad_handle(None) is None
    # the layout helper
    for bad in ((0, 0, 1, 0), (2, 2, 1, 0), (2, -1, 1, 0), (2, 0, 0, 0)):
        assert lib.d2fe_quad_exchange_job_layout(*bad, None, None, 0) == INVALID


@pytest.mark.parametrize("world,loopback", [(1, True), (2, False), (4, False), (8, False), (4, True)])
@pytest.mark.parametrize("quads", [1, 2, 4])
def test_job_layout_of_the_c_code_equals_the_python_table(lib, world, loopback, quads):
    """VERDICT weak point 10 for the quadcam case: the job / problem layout at world 1 (loopback), 2, 4 and 8 as the C code builds it, against its Python statement"""
    from d2slam_amd import api, swarm
    for rank in range(world):
        lay = swarm.quad_remote_job_layout(world, rank, quads, loopback)
        njobs = (world if loopback else world - 1) * quads
        assert lib.d2fe_quad_exchange_job_layout(world, rank, quads, int(loopback), None, None, 0) == njobs
        jr, jq = (C.c_int32 * njobs)(), (C.c_int32 * njobs)()
        assert lib.d2fe_quad_exchange_job_layout(world, rank, quads, int(loopback), jr, jq, njobs) == njobs
        assert list(jr) == lay["job_rank"] and list(jq) == lay["job_quad"]
        assert api.quad_exchange_job_layout(world, rank, quads, loopback) == (lay["job_rank"], lay["job_quad"])
        # a short buffer is not overrun
        if njobs > 1:
            sr = (C.c_int32 * njobs)(*([-7] * njobs))
            assert lib.d2fe_quad_exchange_job_layout(world, rank, quads, int(loopback), sr, None, njobs - 1) == njobs
            assert list(sr)[:njobs - 1] == lay["job_rank"][:njobs - 1] and sr[njobs - 1] == -7
        # rank-major over the other ranks, then the quad frame
        others = [r for r in range(world) if loopback or r != rank]
        assert lay["job_rank"] == [r for r in others for _ in range(quads)] and lay["job_quad"] == list(range(quads)) * len(others)
        assert lay["local_row0"] == [4 * q for q in lay["job_quad"]]
        assert lay["remote_block0"] == [r * 4 * quads + 4 * q for r, q in zip(lay["job_rank"], lay["job_quad"])]
        # the documented problem indexing
        assert len(lay["all2all"]) == 16 * njobs
        for j in range(njobs):
            for lv in range(4):
                for rv in range(4):
                    assert lay["all2all"][j * 16 + lv * 4 + rv] == (lv, rv)
        for dir_b in range(4):
            pairs = lay["gated"](dir_b)
            assert [p[1] for p in pairs] == [2, 3, 0, 1]                       # remote view a = (2 + k) % 4
            assert all(lv == (dir_b - 2 + a) % 4 for lv, a in pairs)
            assert pairs[0] == (dir_b, 2)                                      # the pair the gate compared
        assert lay["gated"](-1) == [(-1, -1)] * 4


def test_gated_view_pairs_equal_the_oracles():
    """the four tracked pairs of quad_remote_job_layout against the oracle's restatement of trackRemoteFrames (d2featuretracker.cpp:282-297)"""
    import numpy as np
    from d2slam_amd import swarm
    from oracle import oracle as orc
    lay = swarm.quad_remote_job_layout(2, 0, 1)
    for dir_b in range(4):
        loc = np.zeros((4, 8), np.float32); rem = np.zeros((4, 8), np.float32)
        for v in range(4):
            loc[v, v] = 1.0
        rem[2, dir_b] = 1.0                                                    # remote view 2 looks where local view dir_b looks
        o = orc.tracker_gate(rem, loc[None], 0.5, True)
        assert o is not None and o["dir_b"] == dir_b
        assert [(b, a) for a, b in o["pairs"]] == lay["gated"](dir_b)          # the oracle lists (remote view, local view)


def _build_cpp(tmp_path):
    """quad_exchange_test.cpp links ONLY libd2fe_hip.so"""
    from d2slam_amd import build as hipbuild
    libpath = hipbuild.build()
    exe = str(tmp_path / "quad_exchange_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-result", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "quad_exchange_test.cpp"), "-L", os.path.dirname(libpath), "-ld2fe_hip",
                           "-Wl,-rpath," + os.path.dirname(libpath), "-Wl,--allow-shlib-undefined", "-o", exe])
    return exe


def test_cpp_quad_exchange_compiles_against_the_c_abi_alone(tmp_path):
    exe = _build_cpp(tmp_path)
    assert subprocess.run([exe], capture_output=True).returncode == 2          # usage error path: runs without touching the GPU
    ldd = subprocess.run(["ldd", exe], capture_output=True, text=True).stdout
    assert "libd2fe_hip" in ldd and "torch" not in ldd and "rccl" not in ldd
