"""CPU checks of the flow landmarks (enable_lk_optical_flow without sp_track_use_lk; include/d2fe.h: d2fe_lk_flow_step_device, d2fe_detect_fast_device): exports and
struct layouts, the list and scratch arithmetic, the reference's defaults, the NumPy restatement of the step against a line-by-line transcription of the reference
on random cases that count what they exercised, the oracle's FAST on dot images (what the GPU tests build their exact cases from), and the source of the new unit."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.helpers import flow_lk_ref as ref
from tests.helpers.lk_carry_ref import _cv_norm_diff

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("d2fe_flow_default_params", "d2fe_lk_flow_list_bytes", "d2fe_lk_flow_list_offset", "d2fe_lk_flow_scratch_bytes", "d2fe_detect_fast_device",
       "d2fe_lk_flow_step_device")


@pytest.fixture(scope="module")
def lib():
    from d2slam_amd import build
    return C.CDLL(build.build())


def test_new_entry_points_are_exported_and_the_defaults_are_the_references(lib):
    from d2slam_amd import api
    hdr = open(os.path.join(ROOT, "include", "d2fe.h")).read()
    for n in NEW:
        assert hasattr(lib, n) and n in api.EXPORTS and ("D2FE_API" in hdr and n + "(" in hdr), n
    for n in ("detect_fast_device", "lk_flow_step_device", "lk_flow_list_views", "flow_params"):
        assert callable(getattr(api, n)), n
    assert api.PROF_STAGES[-1] == "lk"          # no stage was added for the step
    fp = api.flow_params()
    t = fp.track
    # max_cnt 150, PYR_LEVEL 2, WIN_SIZE 21, 30 iterations, near_lk_thread_rate 5.0, feature_min_dist 20, detectFastByRegion(img, num, 3, 4) at threshold 10
    assert (t.total_feature_num, t.levels, t.win, t.iters, t.near_lk_thread_rate, t.feature_min_dist, fp.fast_cols, fp.fast_rows, fp.fast_threshold) == \
        (150, 2, 21, 30, 5.0, 20.0, 3, 4, 10)
    assert fp.superpoint == 1 and fp.reserved == 0 and fp.struct_size == C.sizeof(api._FlowParams)
    g = api.flow_params(total_feature_num=24, superpoint=0, fast_threshold=12, feature_min_dist=7.5)
    assert (g.track.total_feature_num, g.superpoint, g.fast_threshold, g.track.feature_min_dist) == (24, 0, 12, 7.5)
    with pytest.raises(TypeError):
        api.flow_params(max_cnt=3)
    assert api.lk_flow_cap_tracks(g) == 24 and api.lk_flow_cap_tracks(api.flow_params(total_feature_num=0)) == 1


def test_header_layout_of_the_new_struct(tmp_path):
    """sizeof / offsetof as g++ sees include/d2fe.h against the ctypes mirror"""
    import subprocess
    from d2slam_amd import api
    fields = ("superpoint", "track", "fast_cols", "fast_rows", "fast_threshold", "reserved")
    src = tmp_path / "probe.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "d2fe.h"\nint main() {\n  std::printf("%zu", sizeof(d2fe_flow_params));\n'
                   + "".join('  std::printf(" %%zu", offsetof(d2fe_flow_params, %s));\n' % f for f in fields) + '  return 0;\n}\n')
    exe = str(tmp_path / "probe")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    P = api._FlowParams
    assert got == [C.sizeof(P)] + [getattr(P, f).offset for f in fields]
    assert C.sizeof(P) == 56 and P.track.offset == 8 and C.sizeof(api._TrackParams) == 32


def test_list_and_scratch_arithmetic(lib):
    """a flow list: the carry list's rules (32-bit words, 64-word boundaries, enum order) over the fields a flow entry has; the fields it lacks return -1"""
    from d2slam_amd import api
    up = lambda w: (w + 63) // 64 * 64
    for T in (150, 1, 24, 1024, 77):
        sizes = {"hdr": 64, "pts": up(2 * T), "id": up(T), "src": up(T), "trk_xy": up(2 * T), "trk_status": up((T + 3) // 4)}
        o = 0
        for name in api.LKC_FIELDS:
            if name in sizes:
                assert name in api.FLOW_FIELDS and api.lk_flow_list_offset(T, name) == o, (T, name)
                o += sizes[name]
            else:
                assert api.lk_flow_list_offset(T, name) == -1, (T, name)
        assert api.lk_flow_list_bytes(T) == 4 * o
    assert api.lk_flow_list_offset(150, len(api.LKC_FIELDS)) == -1 and api.lk_flow_list_offset(150, -1) == -1
    for bad in (0, 1025, -3):
        assert api.lk_flow_list_bytes(bad) == 0 and api.lk_flow_list_offset(bad, 0) == -1
    # the carry list keeps refusing a list without descriptors
    assert api.lk_carry_list_bytes(151, 0) == 0 and api.lk_carry_list_bytes(151, -1) == 0 and api.lk_carry_list_offset(151, 0, 0) == -1
    v = api.lk_flow_list_views(np.zeros(api.lk_flow_list_bytes(150), np.uint8), 150)
    assert v["n"] == 0 and v["num"] == 0 and v["pts"].shape == (150, 2) and v["trk_status"].shape == (150,) and "desc" not in v
    # scratch: the score map (int32 per pixel, rounded up to 16 bytes), the pool of cols * rows * 2 * cap_tracks int4 candidates, the count
    for (w, h, T, c, r) in ((640, 480, 150, 3, 4), (100, 70, 24, 3, 4), (326, 243, 1024, 3, 4), (163, 121, 1, 2, 5)):
        assert api.lk_flow_scratch_bytes(w, h, T, c, r) == (4 * w * h + 15) // 16 * 16 + 16 * c * r * 2 * T + 16
    for bad in ((8, 480, 150, 3, 4), (640, 480, 0, 3, 4), (640, 480, 1025, 3, 4), (640, 480, 150, 0, 4), (640, 480, 150, 3, -1), (640, 480, 150, 9, 9),
                (20, 480, 150, 3, 4), (640, 27, 150, 3, 4)):      # the last two: regions of 6 px
        assert api.lk_flow_scratch_bytes(*bad) == 0, bad


# ---- flow_step_np against flow_step_naive on random cases that count what they exercised ----
THR, NEAR = 20.0, 5.0


def _case(rng, i):
    """one random step on a 40 px lattice (everything far from everything) with the ingredients of the issue placed on purpose"""
    T = int(rng.choice([8, 12, 16, 24]))
    kind = ("eq", "eq1", "x1", "rand")[i % 4]
    have = {"eq": T - T // 4, "eq1": T - T // 4 - 1, "x1": 0, "rand": int(rng.randint(0, T + 3))}[kind]
    n_kp = int(rng.randint(0, have + 1)); m = have - n_kp
    cells = rng.permutation(144)
    cell = lambda k: np.float32([20 + 40 * (cells[k] % 12), 20 + 40 * (cells[k] // 12)])
    nxt = 0
    kps = np.zeros((n_kp, 2), np.float32)
    for k in range(n_kp):
        kps[k] = cell(nxt); nxt += 1
    trk, st = [], []
    for k in range(m):
        p = cell(nxt) + rng.uniform(-0.4, 0.4, 2).astype(np.float32); nxt += 1
        trk.append(p); st.append(1)
        if rng.rand() < 0.2:
            trk.append(p + np.float32([3.0, 0.0])); st.append(1)         # removeNearPoints drops it
        if rng.rand() < 0.2:
            trk.append(cell(nxt)); nxt += 1; st.append(0)                 # lost
    trk = np.array(trk, np.float32).reshape(-1, 2); st = np.array(st, np.uint8)
    nc = int(rng.randint(0, 40))
    xy, resp = [], []
    for k in range(nc):
        xy.append(cell(nxt)); nxt += 1; resp.append(int(rng.randint(20, 24)))      # four values: ties everywhere
    def beside(q, off, r):
        xy.append(np.float32(np.rint(q)) + np.float32(off)); resp.append(r)
    for k in range(n_kp):
        if rng.rand() < 0.35:
            beside(kps[k], (12, 16) if rng.rand() < 0.5 else (12, 15), int(rng.randint(20, 60)))
    integer_trk = [k for k in range(len(trk)) if st[k]]
    for k in integer_trk:
        if rng.rand() < 0.3:
            trk[k] = np.rint(trk[k])                                      # an integer position, so that (12, 16) is exactly 20 away
            beside(trk[k], (12, 16) if rng.rand() < 0.5 else (12, 15), int(rng.randint(20, 60)))
    for k in range(nc):
        if rng.rand() < 0.25:
            beside(xy[k], (12, 16) if rng.rand() < 0.5 else (-12, 15), resp[k] - int(rng.randint(0, 3)))      # behind xy[k] unless the order says otherwise
    order = rng.permutation(100000)[:len(xy)]
    return T, kps, trk, st, (np.array(xy, np.float32).reshape(-1, 2), np.array(resp, np.int32), order)


def _what_it_exercised(T, kps, trk, st, cand, r, seen):
    lack, num = r["lack"], r["num"]
    seen["lack == total / 4"] += lack == T // 4 and num == 0
    seen["lack == total / 4 + 1"] += lack == T // 4 + 1 and num > 0
    seen["x2"] += num > 0 and num == 2 * lack
    seen["x1"] += num > 0 and num == lack and len(kps) + (r["n"] - r["n_new"]) == 0
    if num <= 0:
        return
    xy, resp, order = cand
    k = sorted(range(len(resp)), key=lambda j: (-int(resp[j]), int(order[j])))[:num]
    seen["response ties"] += any(resp[a] == resp[b] for a, b in zip(k, k[1:]))
    m = r["n"] - r["n_new"]
    tracked = [tuple(p) for p in r["pts"][:m]]
    acc, exact, by = [], False, set()
    stopped_early = False
    for pos, j in enumerate(k):
        if len(acc) >= lack:
            stopped_early = True
            break
        p = tuple(xy[j])
        why = None
        for name, group in (("kp", [tuple(q) for q in kps]), ("trk", tracked), ("acc", acc)):
            for q in group:
                d = _cv_norm_diff(p, q)
                exact = exact or d == THR
                if d < THR and why is None:
                    why = name
        if why is None:
            acc.append(p)
        else:
            by.add(why)
    assert len(acc) == r["n_new"]
    seen["the merge stops at lack"] += stopped_early
    seen["a distance exactly at the threshold"] += exact
    for name in ("kp", "trk", "acc"):
        seen["blocked by " + name] += name in by


def test_flow_step_np_equals_the_naive_transcription():
    rng = np.random.RandomState(20261)
    seen = {k: 0 for k in ("lack == total / 4", "lack == total / 4 + 1", "x2", "x1", "the merge stops at lack", "a distance exactly at the threshold", "blocked by kp",
                           "blocked by trk", "blocked by acc", "response ties")}
    for i in range(160):
        T, kps, trk, st, cand = _case(rng, i)
        a = ref.flow_step_np(trk, st, kps, cand, T, THR, NEAR)
        b = ref.flow_step_naive(trk, st, kps, cand, T, THR, NEAR)
        assert sorted(a) == sorted(b)
        for key in a:
            if key in ("pts", "src"):
                assert a[key].dtype == b[key].dtype and np.array_equal(a[key].view(np.uint32) if key == "pts" else a[key], b[key].view(np.uint32) if key == "pts" else b[key]), (i, key)
            else:
                assert a[key] == b[key], (i, key)
        assert a["n"] <= max(T, a["n"] - a["n_new"])          # the invariant: detection never takes the list beyond total_feature_num
        # a callable detector gives the same step as the raw candidate list
        xy, resp, order = cand
        srt = xy[np.lexsort((order, -resp.astype(np.int64)))]
        c = ref.flow_step_np(trk, st, kps, lambda num: srt[:num], T, THR, NEAR)
        assert np.array_equal(c["pts"], a["pts"]) and c["n_cand"] == a["n_cand"]
        _what_it_exercised(T, kps, trk, st, cand, b, seen)
    print("exercised:", seen)
    assert all(v >= 10 for v in seen.values()), seen


def test_compose_carries_ids_and_src_over_a_fake_sequence():
    """the chain with a tracker that shifts by (-3, 0) and loses every fifth entry, a detector that serves a fixed lattice: ids are ordinals in order of discovery,
    a tracked entry keeps its id, src points into the previous list"""
    lattice = np.float32([[30 + 40 * (k % 7), 30 + 40 * (k // 7)] for k in range(42)])
    track = lambda a, b, pts: ((pts + np.float32([-3, 0])).astype(np.float32), (np.arange(len(pts)) % 5 != 4).astype(np.uint8))
    detect = lambda img, num: lattice[:num]
    out = ref.compose([np.zeros((4, 4), np.uint8)] * 5, [None] * 5, track, detect, dict(total_feature_num=24))
    assert out[0]["n_tracked_in"] == 0 and out[0]["num"] == 24 and out[0]["n"] == 24 and np.array_equal(out[0]["id"], np.arange(24))
    prev = out[0]
    for r in out[1:]:
        m = r["n"] - r["n_new"]
        assert np.array_equal(r["id"][:m], prev["id"][r["src"][:m]]) and np.array_equal(r["id"][m:], prev["next_id"] + np.arange(r["n_new"]))
        assert r["n"] <= 24 and (r["num"] == 0) == (r["lack"] <= 6)
        prev = r
    assert any(r["num"] == 0 for r in out[1:]) and any(r["num"] > 0 for r in out[1:])


def test_dot_images_give_the_detector_exactly_their_dots(orc):
    """what the GPU cases are built from, checked on the oracle's FAST: an isolated pixel of value v on 50 is a corner exactly there with response v - 51, its
    neighbours are not corners, and nothing within 3 px of a region's edge is found (the regions are scanned on their interior)"""
    h, w = 64, 96                                   # regions of 32 x 16
    dots = [(10, 8, 90), (50, 8, 90), (40, 40, 200), (20, 20, 120), (75, 55, 61)]
    edge = [(31, 8, 250), (33, 24, 250), (2, 40, 250), (60, 15, 250), (60, 17, 250), (93, 60, 250)]      # within 3 px of a region edge (x: 0 / 32 / 64 / 96, y: 0 / 16 / ..)
    xy, resp = orc.fast_by_region(ref.dot_image(h, w, dots + edge), 50, 3, 4, 10)
    # response descending; the two of 39 in region order: (10, 8) is region (0, 0), (50, 8) region (1, 0)
    assert xy.tolist() == [[40, 40], [20, 20], [10, 8], [50, 8], [75, 55]] and resp.tolist() == [149, 69, 39, 39, 10]
    assert len(orc.fast_by_region(ref.dot_image(h, w, [(20, 20, 61)]), 50, 3, 4, 10)[0]) == 1       # 61 - 50 = 11 > 10
    assert len(orc.fast_by_region(ref.dot_image(h, w, [(20, 20, 60)]), 50, 3, 4, 10)[0]) == 0       # 10 is not above the threshold
    # (12, 16) apart is exactly feature_min_dist = 20, which `<` keeps; (12, 15) is nearer
    assert _cv_norm_diff((12.0, 16.0), (0.0, 0.0)) == 20.0 and _cv_norm_diff((12.0, 15.0), (0.0, 0.0)) < 20.0


def _body(src, head):
    """text of the function whose definition starts with `head`, up to the closing brace in column 0"""
    i = src.index(head)
    return src[i:src.index("\n}\n", i)]


def test_the_step_neither_synchronises_nor_allocates_and_shares_its_kernels():
    csrc = os.path.join(ROOT, "d2slam_amd", "csrc")
    flow = open(os.path.join(csrc, "lk_flow.hip")).read()
    det = _body(flow, "int d2fe_detect_fast_device(")
    step = _body(flow, "int d2fe_lk_flow_step_device(")
    launch = _body(flow, "void fast_device_launch(")
    flush = _body(open(os.path.join(csrc, "pipe.hip")).read(), "int pipe_flush(d2fe_pipe_s* p) {")
    for text in (det, step, launch, flush, _body(flow, "size_t d2fe_lk_flow_scratch_bytes("), _body(flow, "size_t d2fe_lk_flow_list_bytes(")):
        for word in ("hipStreamSynchronize", "hipDeviceSynchronize", "hipEventSynchronize", "hipMalloc", "hipHostMalloc", "hipFree", "hipMemset", "ctx_scratch"):
            assert word not in text, word
    # the number of launches the header states: five a frame, four for the detector alone
    hdr = open(os.path.join(ROOT, "include", "d2fe.h")).read()
    assert "FIVE launches per frame" in hdr and "(FOUR launches)" in hdr
    assert launch.count("hipLaunchKernelGGL") == 3 and step.count("hipLaunchKernelGGL") == 2 and step.count("fast_device_launch(") == 1
    assert det.count("hipLaunchKernelGGL") == 1 and det.count("fast_device_launch(") == 1
    assert "D2FE_PROF_LK" in step and "D2FE_PROF_LK" in det and launch.count("D2FE_PROF_LK") == 3
    # one tracker, one detector, one b-c: the unit defines no second copy of what it shares
    for name in ("void lk_calc(", "int lk_bidir(", "int fast_strength(", "void fast_region_kernel(", "void fast_nonmax_kernel(", "bool nearer(", "int list_reduce_prune(",
                 "bool list_track_and_arrive(", "void quad_hand_out_ids("):
        assert name not in flow, name
        assert sum(open(os.path.join(csrc, f)).read().count(name) for f in os.listdir(csrc)) == 1, name
    # the step reaches the tracker through step a of both lists, list_track_and_arrive (lk_list_device.h), whose body holds the lk_bidir( call
    lst = open(os.path.join(csrc, "lk_list_device.h")).read()
    assert "list_track_and_arrive(" in _body(flow, "void flow_step_body(") and "lk_bidir(" in _body(lst, "bool list_track_and_arrive(")
    assert "list_reduce_prune(" in flow and "nearer(" in flow and "fast_region_kernel," in flow and "fast_nonmax_kernel," in flow
    for word in ("lk_calc(", "tex(", "lk_level("):
        assert word not in flow and word not in lst, word
    carry = open(os.path.join(csrc, "lk_carry.hip")).read()
    assert "list_reduce_prune(" in carry and '#include "lk_list_device.h"' in carry and '#include "fast_device.h"' in open(os.path.join(csrc, "lk.hip")).read()
    assert "list_track_and_arrive(" in carry and "quad_hand_out_ids(" in carry and "quad_hand_out_ids(" in flow
    # no selection is left to an option
    for word in ("getenv", "d2fe_dev_env"):
        assert word not in flow, word


def test_the_pipe_mode_is_exported_and_mirrored(lib, tmp_path):
    """d2fe_pipe_flow_enable / d2fe_pipe_flow_result_get and d2fe_pipe_flow_result as g++ sees it against the ctypes mirror; the chain of pipe_flush serves both list kinds"""
    import subprocess
    from d2slam_amd import api
    for n in ("d2fe_pipe_flow_enable", "d2fe_pipe_flow_result_get"):
        assert hasattr(lib, n) and n in api.EXPORTS
    R = api._PipeFlowResult
    fields = [f for f, _ in R._fields_ if f != "reserved"]
    src = tmp_path / "probe.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "d2fe.h"\nint main() {\n  std::printf("%zu", sizeof(d2fe_pipe_flow_result));\n'
                   + "".join('  std::printf(" %%zu", offsetof(d2fe_pipe_flow_result, %s));\n' % f for f in fields) + '  return 0;\n}\n')
    exe = str(tmp_path / "probe")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(R)] + [getattr(R, f).offset for f in fields]
    flush = _body(open(os.path.join(ROOT, "d2slam_amd", "csrc", "pipe.hip")).read(), "int pipe_flush(d2fe_pipe_s* p) {")
    # ONE chain: one event wait, one carry copy, one event record and one left -> right launch over the lists, whichever list kind the pipe carries
    assert flush.count("ev_chain") == 2 and flush.count("hipMemcpyAsync(p->d_carry_pyr") == 1 and flush.count("lk_carry_right_launch(") == 1
    assert flush.count("d2fe_lk_flow_step_device(") == 1 and flush.count("d2fe_lk_carry_step_device(") == 1
    assert flush.index("if (p->sp_lk || p->flow)") < flush.index("d2fe_lk_flow_step_device(") < flush.index("hipMemcpyAsync(p->d_carry_pyr")
    sig = __import__("inspect").signature(api.StereoPipe.__init__).parameters
    assert "flow_lk" in sig and "flow_params" in sig


def test_cpp_driver_of_the_pipe_mode_compiles_and_links(tmp_path):
    """tests/cpp/pipe_flow_test.cpp (StereoPipe::flowEnable, StereoFrameResult::flow through include/d2fe.hpp) builds with g++ -Wall -Werror; without arguments it
    leaves with 2 before touching a GPU"""
    import subprocess
    from d2slam_amd import build as hipbuild
    lib = hipbuild.build()
    exe = str(tmp_path / "pipe_flow_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "pipe_flow_test.cpp"),
                           "-L", os.path.dirname(lib), "-ld2fe_hip", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib",
                           "-Wl,--allow-shlib-undefined", "-o", exe])
    assert subprocess.run([exe], capture_output=True).returncode == 2
