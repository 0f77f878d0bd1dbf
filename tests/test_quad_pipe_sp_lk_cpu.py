"""CPU checks of the quad pipe's sp_lk mode (d2fe_quad_track_*, d2fe_lk_carry_quad_step_device, d2fe_lk_carry_neighbour_device; include/d2fe.h): the entry points
are declared, exported and listed, the ctypes mirror of d2fe_quad_track_result has the header's layout, d2fe_quad_pipe_config keeps its size, the C++ driver links
against the library alone, the launch functions and the pipe's chain only enqueue, and the host restatements the GPU tests compare with
(tests/helpers/quad_lk_ref.py) are themselves held to transcriptions of the reference's lines and to the reference's own opticalflowTrackPyr."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests.helpers import lk_carry_ref as ref
from tests.helpers import quad_lk_ref as qref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["d2fe_lk_carry_quad_step_device", "d2fe_lk_carry_neighbour_device", "d2fe_quad_track_enable", "d2fe_quad_track_result_get"]


@pytest.fixture(scope="module")
def lib():
    from d2slam_amd import build
    return C.CDLL(build.build())


def test_the_new_entry_points_are_declared_exported_and_listed(lib):
    from d2slam_amd import api
    src = open(os.path.join(ROOT, "include", "d2fe.h")).read()
    declared = set(re.findall(r"D2FE_API\s+[\w\s\*]+?\b(d2fe_\w+)\s*\(", src))
    assert sorted(n for n in declared if n.startswith("d2fe_quad_track_")) == ["d2fe_quad_track_enable", "d2fe_quad_track_result_get"]
    for n in NEW:
        assert n in declared and hasattr(lib, n) and n in api.EXPORTS, n
    hpp = open(os.path.join(ROOT, "include", "d2fe.hpp")).read()
    assert "d2fe_quad_track_enable(" in hpp and "d2fe_quad_track_result_get(" in hpp


_PROBE = r"""
#include <cstddef>
#include <cstdio>
#include "d2fe.h"
#define F(T, f) std::printf("%s %s %zu\n", #T, #f, offsetof(T, f));
int main() {
  std::printf("d2fe_quad_track_result sizeof %zu\n", sizeof(d2fe_quad_track_result));
  std::printf("d2fe_quad_pipe_config sizeof %zu\n", sizeof(d2fe_quad_pipe_config));
  std::printf("d2fe_track_params sizeof %zu\n", sizeof(d2fe_track_params));
@FIELDS@
  return 0;
}
"""


def test_ctypes_mirror_matches_the_header_and_the_config_keeps_its_size(tmp_path):
    from d2slam_amd import api
    structs = {"d2fe_quad_track_result": api._QuadTrackResult, "d2fe_quad_pipe_config": api._QuadPipeConfig, "d2fe_track_params": api._TrackParams}
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
    assert [f[0] for f in api._QuadTrackResult._fields_[:4]] == ["quads", "cap_tracks", "desc_dim", "list_words"]


def test_null_arguments_are_refused_without_a_device(lib):
    from d2slam_amd import api
    tp = api.track_params()
    r = api._QuadTrackResult()
    assert lib.d2fe_quad_track_enable(None, C.byref(tp)) == -1
    assert lib.d2fe_quad_track_result_get(None, C.c_int64(0), C.byref(r)) == -1
    Z = C.c_size_t(0)
    assert lib.d2fe_lk_carry_quad_step_device(None, None, None, Z, 64, 64, None, None, Z, 256, None, None, None, None, 0, C.byref(tp), None, None) == -1
    assert lib.d2fe_lk_carry_neighbour_device(None, None, Z, 1, 64, 64, C.c_double(200.0), None, Z, 256, C.byref(tp), None, None, None) == -1


def build_cpp(tmp_path):
    """tests/cpp/quad_track_test.cpp links ONLY libd2fe_hip.so"""
    from d2slam_amd import build as hipbuild
    libpath = hipbuild.build()
    exe = str(tmp_path / "quad_track_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-result", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "quad_track_test.cpp"), "-L", os.path.dirname(libpath), "-ld2fe_hip",
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


def test_the_launches_and_the_chain_neither_synchronise_nor_allocate():
    """d2fe_lk_carry_quad_step_device, d2fe_lk_carry_neighbour_device and quad_pass (where the pipe calls them) only enqueue: ONE launch each, the carry copy is a
    hipMemcpyAsync, the chain across lanes is an event wait; allocation and the zeroing of the blocks belong to d2fe_quad_track_enable"""
    csrc = os.path.join(ROOT, "d2slam_amd", "csrc")
    carry = open(os.path.join(csrc, "lk_carry.hip")).read()
    pipe = open(os.path.join(csrc, "quad_pipe.hip")).read()
    step = _body(carry, "int d2fe_lk_carry_quad_step_device(")
    # the neighbour launch of both list kinds is ONE internal function, which each entry point calls once and launches nothing beside
    nb = _body(carry, "int lk_neighbour_launch(")
    for entry in ("int d2fe_lk_carry_neighbour_device(", "int d2fe_lk_flow_neighbour_device("):
        assert _body(carry, entry).count("lk_neighbour_launch(") == 1 and "hipLaunchKernelGGL" not in _body(carry, entry), entry
    assert carry.count("lk_neighbour_launch(") == 3
    chain = _body(pipe, "int quad_pass(d2fe_quad_pipe_s* p")
    assert "lk_carry_quad_step_kernel" in step and "lk_carry_neighbour_kernel" in nb
    assert step.count("hipLaunchKernelGGL") == 1 and nb.count("hipLaunchKernelGGL") == 1
    assert "d2fe_lk_carry_quad_step_device(" in chain and "d2fe_lk_carry_neighbour_device(" in chain and "hipMemcpyAsync(p->carry_pyr()" in chain
    assert "hipStreamWaitEvent(s, p->lanes[pk].ev_chain, 0)" in chain and "hipEventRecord(L.ev_chain, s)" in chain
    assert chain.count("d2fe_lk_carry_neighbour_device(") == 1 and chain.count("d2fe_lk_carry_quad_step_device(") == 1
    # the single-camera step appears once, behind the development library's measurement switch (the product library's d2fe_dev_env returns the default, 0)
    assert chain.count("d2fe_lk_carry_step_device(") == 1 and chain.index("if (p->trk_split)") < chain.index("d2fe_lk_carry_step_device(") < chain.index("continue;")
    assert pipe.count("trk_split = ") == 2 and 'p->trk_split = d2fe_dev_env("D2FE_QUAD_TRACK_SPLIT", 0) != 0;' in pipe
    for text in (step, nb, chain):
        for word in ("hipStreamSynchronize", "hipDeviceSynchronize", "hipEventSynchronize", "hipMalloc", "hipHostMalloc", "hipFree", "hipMemset", "ctx_scratch"):
            assert word not in text, word
    assert "D2FE_PROF_LK" in step and "D2FE_PROF_LK" in nb
    # the kernels call the tracker's device functions of lk_device.h: the half-image form exists once, next to lk_bidir, with a forward and a reverse lk_calc
    dev = open(os.path.join(csrc, "lk_device.h")).read()
    assert dev.count("int lk_bidir_half(") == 1 and _body(dev, "int lk_bidir_half(").count("lk_calc(") == 2
    # the quad step kernel is the single kernel's body on the camera's view plus the id hand-out: step a (the one lk_bidir( of the list steps) is list_track_and_arrive
    # in lk_list_device.h; the neighbour kernel holds the unit's one lk_bidir_half(
    lst = open(os.path.join(csrc, "lk_list_device.h")).read()
    quad = _body(carry, "void lk_carry_quad_step_kernel(")
    assert "carry_step_body<true>(" in quad and quad.count("quad_hand_out_ids(") == 1 and "carry_step_body<false>(" in _body(carry, "void lk_carry_step_kernel(")
    assert _body(carry, "bool carry_step_body(").count("list_track_and_arrive(") == 1 and _body(lst, "bool list_track_and_arrive(").count("lk_bidir(") == 1
    kern = carry[carry.index("bool carry_step_body("):carry.index("hipStream_t ctx_stream(d2fe_handle h);")]
    assert kern.count("lk_bidir(") == 1 and kern.count("lk_bidir_half(") == 1 and "lk_bidir_half(" in _body(carry, "void lk_carry_neighbour_kernel(")
    for unit in (kern, lst):
        assert "lk_calc(" not in unit and "tex(" not in unit and "lk_level(" not in unit
    # allocation and zeroing: in the one enable path of both modes, which d2fe_quad_track_enable calls
    enable = _body(pipe, "int d2fe_quad_track_enable(")
    shared = _body(pipe, "int quad_lists_enable(")
    assert enable.count("quad_lists_enable(") == 1 and "hipMalloc" in shared and "hipMemset" in shared and pipe.count("quad_lists_enable(") == 3
    assert 'p->trk_split = d2fe_dev_env("D2FE_QUAD_TRACK_SPLIT", 0) != 0;' in enable


def _fake_tracker(seed):
    """a deterministic stand-in for the LK tracker: the scene's motion plus a little noise, some tracks lost"""
    def track(prev_img, cur_img, pts):
        rng = np.random.RandomState(seed + 31 * len(pts) + int(prev_img[0, 0]))
        out = (np.asarray(pts, np.float32) + np.float32([-3.0, 0.0]) + rng.uniform(-0.3, 0.3, (len(pts), 2)).astype(np.float32)).astype(np.float32)
        return out, (rng.rand(len(pts)) > 0.15).astype(np.uint8)
    return track


def test_shared_counter_composition_against_the_naive_id_order():
    """compose_quad hands ONE id counter through the cameras in the order 0, 1, 2, 3 of every quad frame (trackLocalFrames, d2featuretracker.cpp:121-133; every
    new entry of the replenishment loop :556-589 takes the next landmark id).  Its ids, over 6 quad frames with lost tracks and new entries in several cameras of
    one frame, equal quad_ids_naive's, which sees only which entries are new; and every camera's list equals carry_step_naive's on the same tracker output"""
    rng = np.random.RandomState(4)
    NT = 6
    views = [[np.full((4, 4), 16 * t + c, np.uint8) for c in range(4)] for t in range(NT)]
    kps = []
    for t in range(NT):
        row = []
        for c in range(4):
            n = int(rng.randint(20, 60)) if (t, c) != (2, 1) else 0
            k = np.stack([rng.randint(4, 196, n), rng.randint(4, 116, n)], 1).astype(np.float32)
            row.append((k, rng.rand(n).astype(np.float32), rng.randn(n, 8).astype(np.float32)))
        kps.append(row)
    prm = {"total_feature_num": 40, "feature_min_dist": 12.0, "near_lk_thread_rate": 6.0}
    half = lambda a, b, p, init, typ, mc: (np.asarray(init, np.float32), np.ones(len(p), np.uint8))
    comp, nbs = qref.compose_quad(views, kps, _fake_tracker(3), half, prm)
    ids = qref.quad_ids_naive([[k["src"] for k in row] for row in comp])
    seen = 0
    for t in range(NT):
        for c in range(4):
            k = comp[t][c]
            assert list(k["id"]) == ids[t][c], (t, c)
            nv = ref.carry_step_naive(k["trk_pts"], k["trk_status"], kps[t][c][0], **prm)
            assert nv["n"] == k["n"] and np.array_equal(nv["src"], k["src"]) and np.array_equal(nv["kp"], k["kp"]) and np.array_equal(nv["pts"], k["pts"])
            new = k["id"][k["src"] < 0]
            assert list(new) == list(range(seen, seen + len(new)))            # camera order, without gaps
            seen += len(new)
            assert np.array_equal(k["desc"][k["src"] < 0], kps[t][c][2][k["kp"][k["src"] < 0]])
    assert any(k["n_lost"] > 0 for row in comp for k in row) and any(sum(k["n_new"] > 0 for k in row) >= 2 for row in comp[1:])
    assert comp[2][1]["n_new"] == 0
    # the neighbour tracks are taken on the list AFTER the frame's step, scattered to the slots of list a
    for t in range(NT):
        for p, (a, b, typ) in enumerate(qref.NEIGHBOURS):
            ok, init = qref.half_gate(comp[t][a]["pts"], typ, qref.W, qref.FOV)
            assert len(nbs[t][p]["status"]) == comp[t][a]["n"] and np.array_equal(nbs[t][p]["status"] != 0, ok)
            assert np.array_equal(nbs[t][p]["pts"][ok], init) and not nbs[t][p]["pts"][~ok].any()


def test_move_cols_and_the_scene():
    assert qref.move_cols(qref.W, qref.FOV) == np.float32(90.0)
    q = qref.cyclic_quads(2, 11)
    assert q.shape == (2, 4, qref.H, qref.W) and q.dtype == np.uint8
    # the panorama 90 columns further on, and 3 columns per frame: equal up to the independent noise (sigma 3, rounded: a difference of sigma-4.3 values)
    d1 = q[0, 0, :, :110].astype(np.int32) - q[0, 1, :, 90:].astype(np.int32)
    d2 = q[0, 0, :, 90:].astype(np.int32) - q[0, 3, :, :110].astype(np.int32)
    d3 = q[0, 2, :, 3:].astype(np.int32) - q[1, 2, :, :-3].astype(np.int32)
    for d in (d1, d2, d3):
        assert abs(d).mean() < 5.0
    assert abs(q[0, 0].astype(np.int32) - q[0, 2].astype(np.int32)).mean() > 10.0


_GATE_CASES = [(1, 2.0, 0.5, 800, 400), (2, -1.5, 1.0, 800, 400), (1, 0.0, 0.0, 200, 120), (2, 0.0, 0.0, 200, 120)]


@pytest.mark.parametrize("ttype,dx,dy,W,H", _GATE_CASES)
def test_half_gate_against_the_reference_lines(orc, ttype, dx, dy, W, H):
    """half_gate + the oracle's bidirectional track give the surviving points and indices of the reference's own opticalflowTrackPyr (opticaltrack_utils.cpp:173-278,
    compiled where it lies: oracle/ref.py::lk_track_pyr), with points exactly on and next to both gate bounds"""
    from oracle import ref as spref
    from d2slam_amd.synth import synth_image
    if not spref.available():
        pytest.skip("oracle/_ref/libspref.so absent and the reference tree not present")
    from tests.test_ref_pin import _shift
    fov = 200.0
    move = float(qref.move_cols(W, fov))
    img = synth_image(H, W, 41 + ttype)
    cur = _shift(img, dx + (move if ttype == 1 else -move), dy)
    pts, _ = orc.fast_by_region(img, 150)
    f32 = np.float32
    edge = [[W - move, H / 2], [np.nextafter(f32(W - move), f32(0)), H / 3], [move, H / 2], [np.nextafter(f32(move), f32(0)), H / 3], [0.4, 0.4], [W - 1.2, H - 1.3]]
    pts = np.concatenate([pts, edge]).astype(np.float32)
    rp, rid = spref.lk_track_pyr(img, cur, pts, ttype, fov)
    ok, init = qref.half_gate(pts, ttype, W, fov)
    n = len(pts) - len(edge)
    assert list(ok[n:n + 4]) == ([False, True, True, True] if ttype == 1 else [True, True, True, False])
    p0, p1 = orc.pyr_build(img), orc.pyr_build(cur)
    out, st = orc.lk_track(p0, p1, W, H, pts[ok], init, track_type=ttype, move_cols=move)
    ids = np.nonzero(ok)[0][st > 0]
    assert len(rid) > 10 and np.array_equal(rid, ids) and np.array_equal(rp, out[st > 0])
