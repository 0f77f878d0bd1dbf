"""CPU checks of the loop query's C ABI (d2fe_loop_*; include/d2fe.h, csrc/loop.hip): the ctypes mirrors have the header's layout, every entry point is
exported and listed, the argument checks that need no device, and the two pieces of reasoning the search kernel rests on, held to the oracle (and, when it has been
built, to the reference's own queryIndexFromDatabase compiled in place):
  * the masked arg-max -- best row by (similarity descending, label ascending) among label <= ntotal - max_index, accepted above thres -- returns what the
    reference's scan of the top min(5 + max_index, ntotal) returns (loop_detector.cpp:314-345);
  * the direction table of computeCorrespondFeaturesOnImageArray (:461-476)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import ref as spref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["d2fe_loop_default_config", "d2fe_loop_create", "d2fe_loop_create_quad", "d2fe_loop_destroy", "d2fe_loop_enqueue", "d2fe_loop_collect", "d2fe_loop_ntotal",
         "d2fe_loop_keyframes", "d2fe_loop_stream", "d2fe_loop_query_device", "d2fe_loop_add_host"]
INVALID = -1


@pytest.fixture(scope="module")
def lib():
    from d2slam_amd import build
    l = C.CDLL(build.build())
    l.d2fe_last_error.restype = C.c_char_p
    return l


def test_every_loop_entry_point_is_declared_exported_and_listed(lib):
    src = open(os.path.join(ROOT, "include", "d2fe.h")).read()
    declared = sorted(n for n in set(re.findall(r"D2FE_API\s+[\w\s\*]+?\b(d2fe_\w+)\s*\(", src)) if n.startswith("d2fe_loop_"))
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
  std::printf("d2fe_loop_config sizeof %zu\n", sizeof(d2fe_loop_config));
  std::printf("d2fe_loop_result sizeof %zu\n", sizeof(d2fe_loop_result));
@FIELDS@
  return 0;
}
"""


def test_loop_config_and_result_structs_match_the_header(tmp_path, lib):
    """field by field: names and order from the header's text, offsets and sizes from a g++ probe"""
    from d2slam_amd import api
    structs = {"d2fe_loop_config": api._LoopConfig, "d2fe_loop_result": api._LoopResult}
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
    c = api._LoopConfig()
    lib.d2fe_loop_default_config(C.byref(c))
    assert c.struct_size == C.sizeof(api._LoopConfig)
    assert (c.capacity_keyframes, c.max_index, c.mode, c.slots, c.timing, c.max_queries) == (4096, 10, 0, 4, 0, 64)
    assert (c.thres, c.ratio) == (0.6, 0.8) and list(c.reserved) == [0] * 6 and c.reserved0 == 0
    lib.d2fe_loop_default_config(None)
    assert (api.LOOP_QUERY, api.LOOP_ADD) == tuple(int(v) for v in re.search(r"D2FE_LOOP_QUERY = (\d+), D2FE_LOOP_ADD = (\d+)", hdr).groups())


def test_bad_arguments_are_refused_without_a_device(lib):
    from d2slam_amd import api
    c = api._LoopConfig()
    lib.d2fe_loop_default_config(C.byref(c))
    x = C.c_void_p()
    assert lib.d2fe_loop_create(None, C.byref(c), C.byref(x)) == INVALID and not x.value
    assert lib.d2fe_loop_create_quad(None, C.byref(c), C.byref(x)) == INVALID and not x.value
    r = api._LoopResult()
    lib.d2fe_loop_enqueue.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int]
    assert lib.d2fe_loop_enqueue(None, 0, 0, None, 3) == INVALID
    assert lib.d2fe_loop_collect(None, 0, C.byref(r)) == INVALID
    assert lib.d2fe_loop_ntotal(None) == INVALID and lib.d2fe_loop_keyframes(None) == INVALID
    lib.d2fe_loop_query_device.argtypes = [C.c_void_p] * 4 + [C.c_int] * 3 + [C.c_void_p]
    assert lib.d2fe_loop_query_device(None, None, None, None, 1, 0, 0, None) == INVALID
    assert lib.d2fe_loop_add_host(None, None, None, None, 1) == INVALID
    lib.d2fe_loop_stream.restype = C.c_void_p
    assert lib.d2fe_loop_stream(None) is None
    lib.d2fe_loop_destroy(None)


def _unit_rows(a):
    a = np.asarray(a, np.float32)
    return (a / np.linalg.norm(a, axis=-1, keepdims=True)).astype(np.float32)


def _select(sims, ntotal, max_index, thres):
    """the search kernel's selection, restated: masked arg-max on (similarity descending, label ascending), then the threshold"""
    best = -1
    for i in range(ntotal):
        if i <= ntotal - max_index and (best < 0 or sims[i] > sims[best]):      # strict: the lower label keeps a tie
            best = i
    return best if best >= 0 and float(sims[best]) > thres else -1


def _cases():
    """(name, db, q, max_index, thres) over ntotal x max_index, each with: a plain near-copy, a duplicate of the target at a lower and at a higher label, a
    better row planted one past the allowed range, and a threshold just above / just below the target's similarity"""
    dim = 64
    out = []
    for max_index in (0, 1, 10):
        for ntotal in (0, 1, 3, max_index, max_index + 1, 300):
            rng = np.random.RandomState(1000 * max_index + ntotal)
            db = _unit_rows(rng.randn(max(ntotal, 1), dim))[:ntotal]
            if ntotal == 0:
                out.append(("empty", db, _unit_rows(rng.randn(dim)), max_index, 0.5))
                continue
            last_ok = min(max(ntotal - max_index, 0), ntotal - 1)
            for target in sorted({0, ntotal // 2, last_ok, ntotal - 1}):
                q = _unit_rows(db[target] + (0.3 / np.sqrt(dim)) * rng.randn(dim).astype(np.float32))
                s_t = float(np.float32(db[target] @ q))
                out.append(("plain t%d" % target, db, q, max_index, 0.5))
                out.append(("thres below t%d" % target, db, q, max_index, s_t - 1e-3))
                out.append(("thres above t%d" % target, db, q, max_index, s_t + 1e-3))
                for other in (target - 1, target + 1):      # the same row twice: the lower label wins
                    if 0 <= other < ntotal:
                        d2 = db.copy(); d2[other] = db[target]
                        out.append(("duplicate t%d o%d" % (target, other), d2, q, max_index, 0.5))
            if max_index >= 1 and ntotal - max_index >= 0 and ntotal - max_index + 1 < ntotal:
                # the target at the last allowed label, the query itself (similarity 1) planted at the first excluded one
                t = ntotal - max_index
                q = _unit_rows(db[t] + (0.3 / np.sqrt(dim)) * rng.randn(dim).astype(np.float32))
                d2 = db.copy(); d2[t + 1] = q
                out.append(("excluded better row", d2, q, max_index, 0.5))
    return out


def test_masked_argmax_selection_equals_the_oracles_gate(orc):
    from d2slam_amd import api
    cases = _cases()
    assert len(cases) > 100
    hits = 0
    for name, db, q, max_index, thres in cases:
        ntotal = len(db)
        sims = (db @ q).astype(np.float32) if ntotal else np.zeros(0, np.float32)
        want = orc.db_query(db, q, max_index, thres)[0] if ntotal else -1
        got = _select(sims, ntotal, max_index, thres)
        assert got == want, (name, ntotal, max_index, thres, got, want)
        assert api.loop_select(sims, ntotal, max_index, thres)[0] == want, (name, ntotal, max_index)
        hits += want >= 0
        if name.startswith("duplicate"):
            lo = min(int(n) for n in re.findall(r"\d+", name))
            if lo <= ntotal - max_index:
                assert want == lo, (name, ntotal, max_index, want)                  # of two equal rows the lower label wins
        if name == "excluded better row":
            assert want == ntotal - max_index
        if spref.available():
            assert got == spref.db_query(db, q, max_index, thres)[0], (name, ntotal, max_index, thres)
    assert hits > 30


def test_direction_table():
    """dir_a / dir_b of the V problems of a hit against the loop of loop_detector.cpp:461-476, written out with its own variable names"""
    from d2slam_amd import api
    for V, main_dir in ((4, 2), (1, 0)):
        for dir_old in range(V):
            want = []
            MAX_DIRS, main_dir_a, main_dir_b = V, main_dir, dir_old
            for _dir_a in range(main_dir_a, main_dir_a + MAX_DIRS):
                dir_a = _dir_a % MAX_DIRS
                dir_b = ((main_dir_b - main_dir_a + MAX_DIRS) % MAX_DIRS + _dir_a) % MAX_DIRS
                want.append((dir_a, dir_b))
            got = api.loop_dirs(V, main_dir, dir_old)
            assert got == want
            assert got[0] == (main_dir, dir_old)                                     # the pair the search compared
            assert sorted(a for a, _ in got) == sorted(b for _, b in got) == list(range(V))
            assert all((b - a) % V == (dir_old - main_dir) % V for a, b in got)       # one rotation for all views
    assert api.loop_dirs(1, 0, 0) == [(0, 0)]
    assert api.loop_dirs(4, 2, 0) == [(2, 0), (3, 1), (0, 2), (1, 3)]
