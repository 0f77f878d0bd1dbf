"""CPU checks of the stereo pipe's sp_lk mode (include/d2fe.h): the option takes the last reserved int of d2fe_pipe_config, the new entry points are exported, the
list-block arithmetic is what the header documents, the submit path only enqueues, and the NumPy restatement of the list logic that the GPU tests compare the
device against (tests/helpers/lk_carry_ref.py) is the reference's."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.helpers import lk_carry_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from d2slam_amd import build
    return C.CDLL(build.build())


def test_pipe_config_keeps_its_size_and_sp_lk_defaults_to_off(lib):
    from d2slam_amd.api import _PipeConfig
    c = _PipeConfig()
    for name, _ in _PipeConfig._fields_:        # poison: the default must be WRITTEN
        setattr(c, name, 77)
    lib.d2fe_pipe_default_config.restype = None
    lib.d2fe_pipe_default_config(C.byref(c))
    assert c.sp_lk == 0 and c.lr_lk == 0
    assert C.sizeof(_PipeConfig) == 96 and c.struct_size == 96
    assert _PipeConfig.lr_lk.offset == 88 and _PipeConfig.sp_lk.offset == 92
    assert [n for n, _ in _PipeConfig._fields_][-2:] == ["lr_lk", "sp_lk"]      # no reserved int is left
    hdr = open(os.path.join(ROOT, "include", "d2fe.h")).read()
    cfg = hdr[hdr.index("typedef struct {\n  int32_t struct_size;      /* sizeof(d2fe_pipe_config) */"):hdr.index("} d2fe_pipe_config;")]
    assert "int32_t sp_lk;" in cfg and "reserved" not in cfg and cfg.index("int32_t lr_lk;") < cfg.index("int32_t sp_lk;")


def test_new_entry_points_are_exported_and_the_defaults_are_the_references(lib):
    from d2slam_amd import api
    for n in ("d2fe_lk_carry_step_device", "d2fe_lk_carry_list_bytes", "d2fe_lk_carry_list_offset", "d2fe_track_default_params", "d2fe_pipe_track_result_get",
              "d2fe_pipe_set_track_params"):
        assert hasattr(lib, n) and n in api.EXPORTS
    assert api.PROF_STAGES[-1] == "lk"          # no stage was added for the chain
    tp = api.track_params()
    # max_cnt 150 (d2frontend_params.h:66), feature_min_dist 20 (:65), near_lk_thread_rate 5.0 (d2featuretracker.h:69), PYR_LEVEL 2, WIN_SIZE 21, 30 iterations
    assert (tp.total_feature_num, tp.levels, tp.win, tp.iters, tp.near_lk_thread_rate, tp.feature_min_dist, tp.reserved) == (150, 2, 21, 30, 5.0, 20.0, 0)
    assert C.sizeof(api._TrackParams) == 32 and api._TrackParams.feature_min_dist.offset == 24
    assert api.track_params(total_feature_num=40).total_feature_num == 40
    with pytest.raises(TypeError):
        api.track_params(max_cnt=3)
    assert C.sizeof(api._PipeTrackResult) == 16 + 13 * 8


def test_list_bytes_and_offsets_are_the_documented_layout(lib):
    """32-bit words, every array on a 64-word boundary, in the order of the D2FE_LKC_* enum"""
    from d2slam_amd import api
    up = lambda w: (w + 63) // 64 * 64
    for T, D in ((151, 256), (1, 256), (41, 256), (1024, 256), (151, 64), (77, 33)):
        sizes = [64, up(2 * T), up(T), up(T), up(T), up(T), up(T * D), up(2 * T), up((T + 3) // 4)]
        assert len(sizes) == len(api.LKC_FIELDS)
        o = 0
        for name, sz in zip(api.LKC_FIELDS, sizes):
            assert api.lk_carry_list_offset(T, D, name) == o, (T, D, name)
            o += sz
        assert api.lk_carry_list_bytes(T, D) == 4 * o
    assert api.lk_carry_list_offset(151, 256, len(api.LKC_FIELDS)) == -1 and api.lk_carry_list_offset(151, 256, -1) == -1
    # what d2fe_lk_carry_step_device would refuse: cap_tracks = total_feature_num + 1 outside 1..1024
    for bad in ((0, 256), (1025, 256), (151, 0), (-3, 256)):
        assert api.lk_carry_list_bytes(*bad) == 0 and api.lk_carry_list_offset(bad[0], bad[1], 0) == -1
    v = api.lk_carry_list_views(np.zeros(api.lk_carry_list_bytes(151, 256), np.uint8), 151, 256)
    assert v["n"] == 0 and v["pts"].shape == (151, 2) and v["desc"].shape == (151, 256) and v["trk_status"].shape == (151,)


def _body(src, head):
    """text of the function whose definition starts with `head`, up to the closing brace in column 0"""
    i = src.index(head)
    return src[i:src.index("\n}\n", i)]


def test_the_chain_neither_synchronises_nor_allocates():
    """d2fe_lk_carry_step_device, the left -> right launch of the lists and pipe_flush (where the pipe calls them) only enqueue; the carry copy is a hipMemcpyAsync"""
    csrc = os.path.join(ROOT, "d2slam_amd", "csrc")
    carry = open(os.path.join(csrc, "lk_carry.hip")).read()
    pipe = open(os.path.join(csrc, "pipe.hip")).read()
    step = _body(carry, "int d2fe_lk_carry_step_device(")
    right = _body(carry, "int lk_carry_right_launch(")
    flush = _body(pipe, "int pipe_flush(d2fe_pipe_s* p) {")
    assert "lk_carry_step_kernel" in step and "lk_carry_right_kernel" in right
    assert "d2fe_lk_carry_step_device(" in flush and "lk_carry_right_launch(" in flush and "hipMemcpyAsync(p->d_carry_pyr" in flush
    assert step.count("hipLaunchKernelGGL") == 1 and right.count("hipLaunchKernelGGL") == 1          # one launch per frame, one for all the right tracks
    for text in (step, right, flush, _body(carry, "size_t d2fe_lk_carry_list_bytes("), _body(carry, "long d2fe_lk_carry_list_offset(")):
        for word in ("hipStreamSynchronize", "hipDeviceSynchronize", "hipEventSynchronize", "hipMalloc", "hipHostMalloc", "hipFree", "hipMemset", "ctx_scratch"):
            assert word not in text, word
    assert "D2FE_PROF_LK" in step and "D2FE_PROF_LK" in right
    # the new kernels call the tracker's device functions (lk_device.h, shared with lk.hip), not copies of them
    # -- the list kernels of both units reach the tracker only through lk_bidir / lk_bidir_half: step a of every list is list_track_and_arrive (lk_list_device.h), the one
    # lk_bidir( of the landmark-list step code; lk_carry.hip keeps one for the left -> right launch and the lk_bidir_half( of the neighbour launch
    lst = open(os.path.join(csrc, "lk_list_device.h")).read()
    flow = open(os.path.join(csrc, "lk_flow.hip")).read()
    for unit in (carry, flow, lst):
        assert "lk_calc(" not in unit and "tex(" not in unit and "lk_level(" not in unit
    assert _body(lst, "bool list_track_and_arrive(").count("lk_bidir(") == 1 and lst.count("lk_bidir(") == 1 and "lk_bidir_half(" not in lst
    assert carry.count("lk_bidir(") == 1 and "lk_bidir(" in _body(carry, "void lk_carry_right_kernel(") and carry.count("lk_bidir_half(") == 1
    assert "lk_bidir(" not in flow and "lk_bidir_half(" not in flow
    # the ticket's protocol and the id hand-out exist once, and both units call them
    for name in ("bool list_track_and_arrive(", "void quad_hand_out_ids("):
        assert sum(open(os.path.join(csrc, f)).read().count(name) for f in os.listdir(csrc)) == 1 and lst.count(name) == 1, name
        call = name.split(" ")[1]
        assert carry.count(call) == 1 and flow.count(call) == 1, name
    for unit in (carry, flow):
        assert "__hip_atomic_fetch_add(" not in unit and "hdr + 5" not in unit
    assert lst.count("__hip_atomic_fetch_add(hdr + 5, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT)") == 1 and lst.count("__hip_atomic_fetch_add(") == 2
    assert '#include "lk_device.h"' in carry and '#include "lk_device.h"' in open(os.path.join(csrc, "lk.hip")).read()
    dev = open(os.path.join(csrc, "lk_device.h")).read()
    assert dev.count("int lk_bidir(") == 1 and _body(dev, "int lk_bidir(").count("lk_calc(") == 2        # forward and reverse, in one place for both kernels
    assert dev.count("void lk_calc(") == 1 and sum(open(os.path.join(csrc, f)).read().count("void lk_calc(") for f in os.listdir(csrc)) == 1


def test_cpp_driver_of_the_mode_compiles_and_links(tmp_path):
    """tests/cpp/pipe_sp_lk_test.cpp (StereoPipe with cfg.sp_lk, StereoFrameResult::tracks through include/d2fe.hpp) builds with g++ -Wall -Werror; without arguments
    it leaves with 2 before touching a GPU"""
    import subprocess
    from d2slam_amd import build as hipbuild
    lib = hipbuild.build()
    exe = str(tmp_path / "pipe_sp_lk_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "pipe_sp_lk_test.cpp"),
                           "-L", os.path.dirname(lib), "-ld2fe_hip", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib",
                           "-Wl,--allow-shlib-undefined", "-o", exe])
    assert subprocess.run([exe], capture_output=True).returncode == 2


def _same(a, b):
    for k in ("n", "n_tracked_in", "n_lost", "n_removed_near", "n_new"):
        assert a[k] == b[k], k
    assert a["pts"].dtype == np.float32 and np.array_equal(a["pts"].view(np.uint32), b["pts"].view(np.uint32))
    assert np.array_equal(a["src"], b["src"]) and np.array_equal(a["kp"], b["kp"])


def _grid_points(rng, n, pitch, lo=40, hi=600):
    """points on a lattice of `pitch` pixels (plus a few exact duplicates): neighbours at EXACTLY pitch and pitch * sqrt(2), i.e. ties at a threshold of `pitch`"""
    g = np.arange(lo, hi, pitch, dtype=np.float32)
    pts = np.stack([rng.choice(g, n), rng.choice(g[:len(g) * 3 // 4], n)], axis=1).astype(np.float32)
    return pts


def test_numpy_restatement_against_a_naive_transcription_of_the_reference_lines():
    """carry_step_np (what the GPU tests hold the device to) against carry_step_naive, a deliberately plain loop-by-loop transcription of reduceVector
    (opticaltrack_utils.cpp:273-276), removeNearPoints (opticaltrack_utils.h:61-89) and the replenishment loop (d2featuretracker.cpp:556-589), on random point sets:
    uniform ones, lattices whose pitch IS a threshold (distance exactly 5, exactly 20, and 3-4-5 triangles: `<` must keep them), thresholds that are not
    representable floats, and keypoint lists long enough for the strict `>` of the loop's exit to overshoot to total + 1.
    oracle/ is frozen, so these reference lines cannot be pinned by compiling them into oracle/_ref as tests/test_ref_pin.py does for others: the second
    transcription, written from the cited lines alone, is what stands in for the pin."""
    rng = np.random.RandomState(20260)
    cases = 0
    overshoot = ties5 = ties20 = removed = lost = 0
    for trial in range(160):
        kind = trial % 4
        n_prev, n_kp = int(rng.randint(0, 90)), int(rng.randint(0, 120))
        prm = dict(total_feature_num=int(rng.choice([0, 1, 7, 40, 150])), feature_min_dist=20.0, near_lk_thread_rate=5.0)
        if kind == 0:
            trk = rng.uniform(0, 640, (n_prev, 2)).astype(np.float32); kps = np.floor(rng.uniform(0, 640, (n_kp, 2))).astype(np.float32)
        elif kind == 1:        # lattice of pitch 5: tracked entries exactly near_lk_thread_rate apart; keypoints on the pitch-20 lattice
            trk = _grid_points(rng, n_prev, 5.0, 100, 160); kps = _grid_points(rng, n_kp, 20.0)
        elif kind == 2:        # 3-4-5: (x + 3, y + 4) is at distance exactly 5, (x + 12, y + 16) at exactly 20
            base = _grid_points(rng, max(n_prev // 2, 1), 7.0, 100, 200)
            trk = np.concatenate([base, base + np.float32([3, 4])])[:n_prev].astype(np.float32)
            kps = np.concatenate([trk[:n_kp // 2] + np.float32([12, 16]), trk[:n_kp // 2] + np.float32([12, 15.99])]).astype(np.float32)
        else:                  # thresholds that are not floats / that exceed each other
            prm.update(feature_min_dist=float(rng.choice([0.0, 7.3, 20.000001, 19.999999])), near_lk_thread_rate=float(rng.choice([0.0, 0.1, 30.0, 4.9999999])))
            trk = (np.floor(rng.uniform(0, 200, (n_prev, 2))) + rng.choice([0.0, 0.5, 0.1], (n_prev, 2))).astype(np.float32)
            kps = np.floor(rng.uniform(0, 200, (n_kp, 2))).astype(np.float32)
        status = (rng.uniform(size=len(trk)) < 0.8).astype(np.uint8)
        a = ref.carry_step_np(trk, status, kps, **prm); b = ref.carry_step_naive(trk, status, kps, **prm)
        _same(a, b)
        cases += 1
        # bookkeeping of what the sets exercised
        assert a["n"] <= max(prm["total_feature_num"] + 1, a["n"] - a["n_new"])
        overshoot += a["n_new"] > 0 and a["n"] == prm["total_feature_num"] + 1
        removed += a["n_removed_near"] > 0; lost += a["n_lost"] > 0
        alive = trk[status != 0]
        if len(alive) > 1:
            d = np.sqrt(((alive[:, None, :].astype(np.float64) - alive[None, :, :]) ** 2).sum(-1))
            ties5 += bool((d == 5.0).any())
        if len(kps) and a["n"]:
            d = np.sqrt(((kps[:, None, :].astype(np.float64) - a["pts"][None, :, :]) ** 2).sum(-1))
            ties20 += bool((d == 20.0).any())
    assert cases == 160 and overshoot >= 10 and ties5 >= 10 and ties20 >= 10 and removed >= 10 and lost >= 10, (overshoot, ties5, ties20, removed, lost)


def test_the_two_thresholds_are_strict_and_the_exit_overshoots_by_one():
    """hand-made: distance == threshold is NOT near (`<`); the loop's `>` lets the list reach total_feature_num + 1; appended keypoints block later ones"""
    for f in (ref.carry_step_np, ref.carry_step_naive):
        r = f(np.float32([[100, 100], [103, 104], [103, 103.99], [300, 300]]), [1, 1, 1, 0], np.zeros((0, 2), np.float32))
        assert r["src"].tolist() == [0, 1] and (r["n_lost"], r["n_removed_near"], r["n_new"]) == (1, 1, 0)      # [1] at exactly 5 stays, [2] at 4.99.. of [0] goes
        # the greedy order: [1] is removed by [0], so [2] (near [1] only) stays
        r = f(np.float32([[0, 0], [4, 0], [8, 0]]), [1, 1, 1], np.zeros((0, 2), np.float32))
        assert r["src"].tolist() == [0, 2]
        kps = np.float32([[112, 116], [112, 115], [200, 200], [212, 216], [400, 400], [500, 100], [50, 400]])
        r = f(np.float32([[100, 100]]), [1], kps, total_feature_num=3)
        # [0] at exactly 20 is appended; [1] at 19.2 is not; [2] is; [3] at exactly 20 of the APPENDED [2] is -> 4 = total + 1 entries, then the loop stops
        assert r["kp"].tolist() == [-1, 0, 2, 3] and r["src"].tolist() == [0, -1, -1, -1] and r["n"] == 4 and r["n_new"] == 3
        r = f(np.zeros((0, 2), np.float32), [], kps, total_feature_num=0)
        assert r["n"] == 1 and r["kp"].tolist() == [0]
        # a previous list longer than total + 1 is not cut, it only takes no keypoint
        r = f(np.float32([[10 * i, 0] for i in range(6)]), [1] * 6, kps, total_feature_num=3)
        assert r["n"] == 6 and r["n_new"] == 0
