"""CPU checks of the keyframe window's C ABI (d2fe_window_*, d2fe_exchange_gathered; include/d2fe.h, csrc/window.hip): every entry point is declared, exported and
listed, the ctypes mirrors have the header's layout, the argument checks that need no device, and the two pieces of host reasoning the feature rests on:
  * d2fe_window_retain_plan against a transcription of updatebySldWin's erase loop (d2featuretracker.cpp:47-57);
  * the gate kernel's selection -- the minimum of (n - 1 - pos) * V + j over the passing pairs -- against the oracle's tracker_gate (and the reference's own
    getMatchedPrevKeyframe where it was compiled), for windows of 0, 1 and 5 keyframes, stereo and quad."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import ref as spref
from tests.helpers import keyframe_window_common as kw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["d2fe_window_default_config", "d2fe_window_create", "d2fe_window_create_quad", "d2fe_window_destroy", "d2fe_window_stream", "d2fe_window_push",
         "d2fe_window_push_host", "d2fe_window_retain", "d2fe_window_retain_plan", "d2fe_window_size", "d2fe_window_tags", "d2fe_window_track_device",
         "d2fe_window_collect", "d2fe_exchange_gathered"]
INVALID = -1


@pytest.fixture(scope="module")
def lib():
    from d2slam_amd import build
    l = C.CDLL(build.build())
    l.d2fe_last_error.restype = C.c_char_p
    return l


def test_every_window_entry_point_is_declared_exported_and_listed(lib):
    src = open(os.path.join(ROOT, "include", "d2fe.h")).read()
    declared = sorted(n for n in set(re.findall(r"D2FE_API\s+[\w\s\*]+?\b(d2fe_\w+)\s*\(", src)) if n.startswith("d2fe_window_") or n == "d2fe_exchange_gathered")
    assert declared == sorted(NAMES)
    from d2slam_amd import api
    for n in declared:
        assert hasattr(lib, n), n
        assert n in api.EXPORTS, n


def test_the_headers_exports_equal_the_librarys(lib):
    from d2slam_amd import api, build
    src = open(os.path.join(ROOT, "include", "d2fe.h")).read()
    declared = set(re.findall(r"D2FE_API\s+[\w\s\*]+?\b(d2fe_\w+)\s*\(", src))
    out = subprocess.run(["nm", "-D", "--defined-only", build.build()], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.split() and l.split()[-1].startswith("d2fe_")}
    assert declared == exported == set(api.EXPORTS)


_PROBE = r"""
#include <cstddef>
#include <cstdio>
#include "d2fe.h"
#define F(T, f) std::printf("%s %s %zu\n", #T, #f, offsetof(T, f));
int main() {
  std::printf("d2fe_window_config sizeof %zu\n", sizeof(d2fe_window_config));
  std::printf("d2fe_window_result sizeof %zu\n", sizeof(d2fe_window_result));
@FIELDS@
  return 0;
}
"""


def test_window_config_and_result_structs_match_the_header(tmp_path, lib):
    """field by field: names and order from the header's text, offsets and sizes from a g++ probe"""
    from d2slam_amd import api
    structs = {"d2fe_window_config": api._WindowConfig, "d2fe_window_result": api._WindowResult}
    hdr = open(os.path.join(ROOT, "include", "d2fe.h")).read()
    for t, s in structs.items():
        body = hdr[:hdr.index("} %s;" % t)]
        body = re.sub(r"/\*.*?\*/", "", body[body.rindex("typedef struct {"):].replace("typedef struct {", ""), flags=re.S)
        names = []
        for decl in body.split(";"):
            decl = re.sub(r"^\s*(const\s+)?(int64_t|int32_t|float|double|void)\s*\**\s*", "", decl.strip())
            names += [re.sub(r"\[.*\]|\*", "", n).strip() for n in decl.split(",") if n.strip()]
        assert names == [f[0] for f in s._fields_], (t, names)
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
    c = api._WindowConfig()
    lib.d2fe_window_default_config(C.byref(c))
    assert c.struct_size == C.sizeof(api._WindowConfig)
    assert (c.capacity, c.mode, c.slots, c.timing, c.max_queries) == (12, 0, 4, 0, 64)
    assert (c.thres, c.ratio) == (0.8, 0.8) and list(c.reserved) == [0] * 6
    lib.d2fe_window_default_config(None)


def test_the_cpp_wrapper_compiles(tmp_path):
    src = tmp_path / "w.cpp"
    src.write_text('#include "d2fe.hpp"\nint main() { D2FrontEnd::RemoteTrack t; return (int)t.matches.size() + (int)sizeof(D2FrontEnd::KeyframeWindow) * 0; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_bad_arguments_are_refused_without_a_device(lib):
    from d2slam_amd import api
    api.load_library()
    c = api._WindowConfig()
    lib.d2fe_window_default_config(C.byref(c))
    x = C.c_void_p()
    assert lib.d2fe_window_create(None, C.byref(c), C.byref(x)) == INVALID and not x.value
    assert lib.d2fe_window_create_quad(None, C.byref(c), C.byref(x)) == INVALID and not x.value
    r = api._WindowResult()
    lib.d2fe_window_push.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int64]
    assert lib.d2fe_window_push(None, 0, 0, 1) == INVALID
    lib.d2fe_window_push_host.argtypes = [C.c_void_p] * 4 + [C.c_int64]
    assert lib.d2fe_window_push_host(None, None, None, None, 1) == INVALID
    assert lib.d2fe_window_retain(None, None, 0) == INVALID
    assert lib.d2fe_window_size(None) == INVALID and lib.d2fe_window_tags(None, None, 0) == INVALID
    lib.d2fe_window_track_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p]
    assert lib.d2fe_window_track_device(None, None, 0, None, 0, None, 0, 1, 0, None) == INVALID
    assert lib.d2fe_window_collect(None, 0, C.byref(r)) == INVALID
    lib.d2fe_window_stream.restype = C.c_void_p
    assert lib.d2fe_window_stream(None) is None
    lib.d2fe_window_destroy(None)
    assert lib.d2fe_exchange_gathered(None, 0, None, None) == INVALID
    lib.d2fe_window_retain_plan.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    assert lib.d2fe_window_retain_plan(None, 1, None, 0, None) == INVALID and lib.d2fe_window_retain_plan(None, -1, None, 0, None) == INVALID
    assert lib.d2fe_window_retain_plan(None, 0, None, 0, None) == 0


def _upd_by_sld_win(current_keyframes, sld_win):
    """d2featuretracker.cpp:47-57, statement by statement, on a list of frame ids"""
    current_keyframes = list(current_keyframes)
    it = 0
    while it != len(current_keyframes):
        if current_keyframes[it] not in sld_win and current_keyframes[it] != current_keyframes[-1]:
            if len(current_keyframes) <= 1:
                it += 1
            else:
                del current_keyframes[it]
        else:
            it += 1
    return current_keyframes


def test_retain_plan_against_the_references_erase_loop():
    from d2slam_amd import api
    win = [7, 3, 11, 5, 9]
    cases = [(win, []),                      # an empty keep list: only the newest stays
             (win, [7, 11]),                 # the newest not listed
             ([4], []), ([4], [4]), ([4], [5]),      # a single keyframe
             (win, win), (win, list(reversed(win))),      # everything listed
             (win, [3, 100, 5, -2, 42]),     # tags listed that are not in the window
             ([], [1, 2]), (win, [9]), (win, [7]), (list(range(64)), list(range(0, 64, 3)))]
    for tags, keep in cases:
        ev = api.window_retain_plan(tags, keep)
        want = _upd_by_sld_win(tags, set(keep))
        assert [t for t, e in zip(tags, ev) if not e] == want, (tags, keep)
        if tags:
            assert not ev[-1]                # the newest never goes
    assert [t for t, e in zip(win, api.window_retain_plan(win, [])) if not e] == [9]
    assert [t for t, e in zip(win, api.window_retain_plan(win, [7, 11])) if not e] == [7, 11, 9]


@pytest.mark.parametrize("V", [1, 4])
@pytest.mark.parametrize("n", [0, 1, 5])
def test_selection_rule_equals_the_oracles_walk(orc, V, n):
    from d2slam_amd import api
    G, cap, nq = 256, 60, 24
    rng = np.random.RandomState(100 * V + n)
    win = kw.make_window(rng, n, V, G, cap, with_desc=False)
    rnv, _, rnk = kw.make_remote(rng, nq, win, V, G, cap, with_desc=False)
    s64 = kw.sims64(rnv, win[0], V)
    assert s64.size == 0 or np.abs(s64 - kw.THRES).min() >= 1e-3
    hits = misses = newer_wins = dirs_wins = 0
    p = kw.plant(n, V)
    for q in range(nq):
        want = kw.expected(orc, spref, rnv[q], rnk[q], win, V, kw.THRES)
        s32 = s64[q].astype(np.float32)
        got = kw.select(s32, kw.THRES)
        assert got == api.window_select(s32, kw.THRES)
        assert (got is None) == (want is None), (V, n, q)
        if got is None:
            misses += 1
            continue
        hits += 1
        pos, j = got
        dir_b = kw.DIRS[j] if V == 4 else 0
        assert (pos, 2 if V == 4 else 0, dir_b) == (want["pos"], want["dir_a"], want["dir_b"]), (V, n, q)
        assert abs(float(s32[pos, j]) - want["sim"]) <= 2e-5
        pairs = [(a, b) for a, b in api.window_views(V, dir_b) if int(rnk[q, a]) > 0 and int(win[2][pos, b]) > 0]
        assert pairs == want["pairs"], (V, n, q)
        if q % 6 == 0 and p["new"] is not None:      # the older keyframe resembles the remote frame more, the newer one merely passes -- and wins
            assert pos == p["new"] and s32[p["old"], j] > s32[pos, j] + 0.1
            newer_wins += 1
        if q % 6 == 1 and p["dup"] is not None:      # two passing views of one keyframe: the first in dirs order, not the better one
            assert pos == p["dup"] and dir_b == 3 and s32[pos, 2] > s32[pos, 1] > kw.THRES
            dirs_wins += 1
    assert misses >= 1 and (hits >= 1 or n == 0)
    if n == 5:
        assert newer_wins >= 1 and (dirs_wins >= 1 or V == 1)
    # exact arithmetic: a similarity equal to the threshold passes, one ulp below it does not
    e = np.zeros((1, V), np.float32); e[0, -1] = 8.0
    assert kw.select(e, 8.0) == (0, V - 1) and kw.select(e, float(np.nextafter(np.float32(8.0), np.float32(9.0)))) is None
