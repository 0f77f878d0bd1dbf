"""CPU checks of the quad pipe's flow_lk mode (d2fe_quad_flow_*, d2fe_lk_flow_quad_step_device, d2fe_lk_flow_neighbour_device; include/d2fe.h): the entry points are
declared, exported and listed, the ctypes mirror of d2fe_quad_flow_result has the header's layout, d2fe_quad_pipe_config keeps its size, null arguments are refused
without a device, the C++ driver links against the library alone, the step and the chain only enqueue, and the host restatement the GPU tests compare with
(tests/helpers/quad_flow_ref.py) hands its ids out in the order of quad_lk_ref.quad_ids_naive."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests.helpers import flow_lk_ref as fref
from tests.helpers import quad_flow_ref as qfref
from tests.helpers import quad_lk_ref as qref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["d2fe_lk_flow_quad_step_device", "d2fe_lk_flow_neighbour_device", "d2fe_quad_flow_enable", "d2fe_quad_flow_result_get"]


@pytest.fixture(scope="module")
def lib():
    from d2slam_amd import build
    return C.CDLL(build.build())


def test_the_new_entry_points_are_declared_exported_and_listed(lib):
    from d2slam_amd import api
    src = open(os.path.join(ROOT, "include", "d2fe.h")).read()
    declared = set(re.findall(r"D2FE_API\s+[\w\s\*]+?\b(d2fe_\w+)\s*\(", src))
    assert sorted(n for n in declared if n.startswith("d2fe_quad_flow_")) == ["d2fe_quad_flow_enable", "d2fe_quad_flow_result_get"]
    for n in NEW:
        assert n in declared and hasattr(lib, n) and n in api.EXPORTS, n
    hpp = open(os.path.join(ROOT, "include", "d2fe.hpp")).read()
    assert "d2fe_quad_flow_enable(" in hpp and "d2fe_quad_flow_result_get(" in hpp and "bool flowEnable(" in hpp
    for f in ("lk_flow_quad_step_device", "lk_flow_neighbour_device"):
        assert callable(getattr(api, f))
    assert callable(api.QuadPipe.flow_enable) and callable(api.QuadPipe.flow_result_raw)


_PROBE = r"""
#include <cstddef>
#include <cstdio>
#include "d2fe.h"
#define F(T, f) std::printf("%s %s %zu\n", #T, #f, offsetof(T, f));
int main() {
  std::printf("d2fe_quad_flow_result sizeof %zu\n", sizeof(d2fe_quad_flow_result));
  std::printf("d2fe_quad_pipe_config sizeof %zu\n", sizeof(d2fe_quad_pipe_config));
  std::printf("d2fe_flow_params sizeof %zu\n", sizeof(d2fe_flow_params));
@FIELDS@
  return 0;
}
"""


def test_ctypes_mirror_matches_the_header_and_the_config_keeps_its_size(tmp_path):
    from d2slam_amd import api
    structs = {"d2fe_quad_flow_result": api._QuadFlowResult, "d2fe_quad_pipe_config": api._QuadPipeConfig, "d2fe_flow_params": api._FlowParams}
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
    # the mode is switched on by a call: the configuration is the one the quad pipe had (12 ints, 4 doubles, 8 reserved ints)
    assert got[("d2fe_quad_pipe_config", "sizeof")] == 12 * 4 + 4 * 8 + 8 * 4
    assert [f[0] for f in api._QuadFlowResult._fields_[:4]] == ["quads", "cap_tracks", "list_words", "reserved"]
    assert [f[0] for f in api._QuadFlowResult._fields_[4:15]] == ["n", "n_tracked_in", "n_lost", "n_removed_near", "n_new", "lack", "num", "n_cand", "pts_xy", "id", "src"]


def test_null_arguments_are_refused_without_a_device(lib):
    from d2slam_amd import api
    fp = api.flow_params()
    r = api._QuadFlowResult()
    assert lib.d2fe_quad_flow_enable(None, C.byref(fp)) == -1 and lib.d2fe_quad_flow_enable(None, None) == -1
    assert lib.d2fe_quad_flow_result_get(None, C.c_int64(0), C.byref(r)) == -1
    Z = C.c_size_t(0)
    assert lib.d2fe_lk_flow_quad_step_device(None, None, None, Z, 64, 64, None, None, Z, None, None, 0, C.byref(fp), None, None, Z, None) == -1
    assert lib.d2fe_lk_flow_neighbour_device(None, None, Z, 1, 64, 64, C.c_double(200.0), None, Z, C.byref(fp.track), None, None, None) == -1
    # the carry form keeps refusing lists without descriptors
    assert lib.d2fe_lk_carry_neighbour_device(None, None, Z, 1, 64, 64, C.c_double(200.0), None, Z, 0, C.byref(fp.track), None, None, None) == -1


def build_cpp(tmp_path):
    """tests/cpp/quad_flow_test.cpp links ONLY libd2fe_hip.so"""
    from d2slam_amd import build as hipbuild
    libpath = hipbuild.build()
    exe = str(tmp_path / "quad_flow_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-result", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "quad_flow_test.cpp"), "-L", os.path.dirname(libpath), "-ld2fe_hip",
                           "-Wl,-rpath," + os.path.dirname(libpath), "-Wl,--allow-shlib-undefined", "-o", exe])
    return exe


def test_cpp_driver_compiles_against_the_c_abi_alone(tmp_path):
    exe = build_cpp(tmp_path)
    assert subprocess.run([exe], capture_output=True).returncode == 2          # usage error path: runs without touching the GPU
    ldd = subprocess.run(["ldd", exe], capture_output=True, text=True).stdout
    assert "libd2fe_hip" in ldd and "torch" not in ldd


def _body(src, head):
    """text of the function whose definition starts with `head`, up to the closing brace in column 0"""
    i = src.index(head)
    return src[i:src.index("\n}\n", i)]


def test_the_step_and_the_chain_neither_synchronise_nor_allocate():
    """d2fe_lk_flow_quad_step_device is FIVE launches and nothing else; quad_pass calls it once per quad frame and the neighbour launch once per pass; the four
    single steps appear once, behind the development library's switch; allocation and the zeroing of the blocks belong to d2fe_quad_flow_enable"""
    csrc = os.path.join(ROOT, "d2slam_amd", "csrc")
    flow = open(os.path.join(csrc, "lk_flow.hip")).read()
    carry = open(os.path.join(csrc, "lk_carry.hip")).read()
    pipe = open(os.path.join(csrc, "quad_pipe.hip")).read()
    step = _body(flow, "int d2fe_lk_flow_quad_step_device(")
    fast = _body(flow, "void fast_quad_launch(")
    # the flow entry point of the neighbour tracks calls the ONE launch function of both list kinds and launches nothing beside
    entry = _body(carry, "int d2fe_lk_flow_neighbour_device(")
    assert entry.count("lk_neighbour_launch(") == 1 and "hipLaunchKernelGGL" not in entry
    nb = _body(carry, "int lk_neighbour_launch(")
    chain = _body(pipe, "int quad_pass(d2fe_quad_pipe_s* p")
    assert step.count("hipLaunchKernelGGL") == 2 and step.count("fast_quad_launch(") == 1 and fast.count("hipLaunchKernelGGL") == 3
    assert step.count("ProfScope") == 2 and fast.count("ProfScope") == 3 and nb.count("hipLaunchKernelGGL") == 1 and "lk_carry_neighbour_kernel" in nb
    assert chain.count("d2fe_lk_flow_quad_step_device(") == 1 and chain.count("d2fe_lk_flow_neighbour_device(") == 1
    assert chain.count("d2fe_lk_flow_step_device(") == 1 and chain.index("if (p->flow && p->flow_split)") < chain.index("d2fe_lk_flow_step_device(") < chain.index("d2fe_lk_flow_quad_step_device(")
    assert pipe.count("flow_split = ") == 2 and 'p->flow_split = d2fe_dev_env("D2FE_QUAD_FLOW_SPLIT", 0) != 0;' in pipe
    for text in (step, fast, nb, chain):
        for word in ("hipStreamSynchronize", "hipDeviceSynchronize", "hipEventSynchronize", "hipMalloc", "hipHostMalloc", "hipFree", "hipMemset", "ctx_scratch"):
            assert word not in text, word
    enable = _body(pipe, "int d2fe_quad_flow_enable(")
    shared = _body(pipe, "int quad_lists_enable(")      # the one enable path of both modes
    assert enable.count("quad_lists_enable(") == 1 and "hipMalloc" in shared and "hipMemset" in shared
    assert 'p->flow_split = d2fe_dev_env("D2FE_QUAD_FLOW_SPLIT", 0) != 0;' in enable
    # the quad-level ticket and the id hand-out: lk_list_device.h's, called once with the flow header's word
    assert flow.count("quad_hand_out_ids(") == 1 and "quad_hand_out_ids(cur0, q.list_stride, FLOW_HDR_QUAD," in _body(flow, "void lk_flow_quad_merge_kernel(")
    # the quad-level ticket is a word the flow header documents as "rest 0": behind lack / num / n_cand (7-9)
    assert re.search(r"constexpr int FLOW_HDR_QUAD = (\d+);", flow).group(1) == "10"
    hdr = open(os.path.join(ROOT, "include", "d2fe.h")).read()
    assert "header word 10 of CAMERA 0's current list" in hdr
    # the product library reads no environment variable
    kern = open(os.path.join(csrc, "kernels.h")).read()
    assert "static inline int d2fe_dev_env(const char*, int dflt) { return dflt; }" in kern and "getenv" not in pipe and "getenv" not in flow


def _fake_tracker(seed):
    """a deterministic stand-in for the LK tracker: the scene's motion plus a little noise, some tracks lost"""
    def track(prev_img, cur_img, pts):
        rng = np.random.RandomState(seed + 31 * len(pts) + int(prev_img[0, 0]))
        out = (np.asarray(pts, np.float32) + np.float32([-3.0, 0.0]) + rng.uniform(-0.3, 0.3, (len(pts), 2)).astype(np.float32)).astype(np.float32)
        return out, (rng.rand(len(pts)) > 0.2).astype(np.uint8)
    return track


def _fake_detector(seed):
    """a deterministic stand-in for detectFastByRegion: a shuffled subset of a 13 px grid, at most num; view (t, c) = (3, 2) finds nothing"""
    gx, gy = np.meshgrid(np.arange(6, 196, 13), np.arange(6, 116, 13))
    grid = np.stack([gx.ravel(), gy.ravel()], 1).astype(np.float32)

    def detect(img, num):
        tag = int(img[0, 0])
        if tag == 16 * 3 + 2:
            return np.zeros((0, 2), np.float32)
        rng = np.random.RandomState(seed + tag)
        return grid[rng.permutation(len(grid))[:int(rng.randint(10, len(grid)))]][:num]
    return detect


def test_shared_counter_composition_against_the_naive_id_order():
    """compose_quad_flow hands ONE id counter through the cameras in the order 0, 1, 2, 3 of every quad frame (trackLocalFrames, d2featuretracker.cpp:121-133).  Its
    ids, over 7 quad frames of random `src` patterns -- lost tracks, new entries in several cameras of one frame, cameras that do not detect (enough keypoints) and a
    camera that detects and finds nothing -- equal quad_ids_naive's, which sees only which entries are new; every camera's list equals flow_step_naive's on the
    same tracker output and candidates"""
    rng = np.random.RandomState(6)
    NT = 7
    views = [[np.full((4, 4), 16 * t + c, np.uint8) for c in range(4)] for t in range(NT)]
    kps = []
    for t in range(NT):
        row = []
        for c in range(4):
            n = int(rng.randint(0, 12)) if (t, c) not in ((2, 1), (4, 0), (4, 3)) else 40          # 40 keypoints: lack = 0, no detection whatever the list holds
            row.append(np.stack([rng.randint(4, 196, n), rng.randint(4, 116, n)], 1).astype(np.float32) if (t + c) % 5 else None)
        kps.append(row)
    prm = {"total_feature_num": 40, "feature_min_dist": 12.0, "near_lk_thread_rate": 6.0}
    half = lambda a, b, p, init, typ, mc: (np.asarray(init, np.float32), np.ones(len(p), np.uint8))
    track, detect = _fake_tracker(3), _fake_detector(9)
    comp, nbs = qfref.compose_quad_flow(views, kps, track, half, detect, prm)
    ids = qref.quad_ids_naive([[k["src"] for k in row] for row in comp])
    seen = 0
    for t in range(NT):
        for c in range(4):
            k = comp[t][c]
            assert list(k["id"]) == ids[t][c], (t, c)
            nv = fref.flow_step_naive(k["trk_pts"], k["trk_status"], kps[t][c], lambda num: detect(views[t][c], num), **prm)
            for key in ("n", "n_new", "lack", "num", "n_cand"):
                assert nv[key] == k[key], (t, c, key)
            assert np.array_equal(nv["src"], k["src"]) and np.array_equal(nv["pts"], k["pts"])
            new = k["id"][k["src"] < 0]
            assert list(new) == list(range(seen, seen + len(new)))            # camera order, without gaps
            seen += len(new)
            assert k["next_id"] == seen
    flat = [k for row in comp for k in row]
    assert any(k["n_lost"] > 0 for k in flat) and any(sum(k["n_new"] > 0 for k in row) >= 3 for row in comp[1:])
    assert comp[2][1]["num"] == 0 and comp[4][0]["num"] == 0 and comp[4][3]["num"] == 0 and comp[3][2]["num"] > 0 and comp[3][2]["n_cand"] == 0
    assert any(any(k["n_new"] == 0 for k in row) and any(k["n_new"] > 0 for k in row) for row in comp[1:])      # cameras that add nothing between cameras that do
    # the neighbour tracks are taken on the list AFTER the frame's step, scattered to the slots of list a
    for t in range(NT):
        for p, (a, b, typ) in enumerate(qref.NEIGHBOURS):
            ok, init = qref.half_gate(comp[t][a]["pts"], typ, qref.W, qref.FOV)
            assert len(nbs[t][p]["status"]) == comp[t][a]["n"] and np.array_equal(nbs[t][p]["status"] != 0, ok)
            assert np.array_equal(nbs[t][p]["pts"][ok], init) and not nbs[t][p]["pts"][~ok].any()
