"""The handle's "pipes alive / destroy requested" state (d2slam_amd/csrc/handle_life.h: one mutex, a pipe count, the doomed flag; d2fe_destroy, the pipes' create
and destroy use it) compiled with g++ and run on the host (tests/cpp/handle_life_test.cpp), plain and under the thread sanitizer.  For P in {1, 2, 8} live pipes, P
threads call pipe_gone() and one calls destroy_requested() behind a common start flag: exactly one call per round says "destroy now"; without a request none does;
a repeated request under live pipes is deferred again."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDS = 2000


@pytest.fixture(scope="module", params=["plain", "tsan"])
def life_lines(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("handle_life") / ("handle_life_test_" + request.param))
    flags = ["-fsanitize=thread", "-g"] if request.param == "tsan" else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread"] + flags + ["-I", os.path.join(ROOT, "d2slam_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "handle_life_test.cpp"), "-o", exe])
    r = subprocess.run([exe, str(ROUNDS)], capture_output=True, text=True, timeout=300, env=dict(os.environ, TSAN_OPTIONS="halt_on_error=1"))
    assert r.returncode == 0, r.stdout + r.stderr
    return [l.split() for l in r.stdout.splitlines()]


def test_exactly_one_call_per_round_destroys(life_lines):
    rows = {int(l[1]): [int(v) for v in l[2:]] for l in life_lines if l[0] == "ok" and l[1] != "sequence"}
    assert sorted(rows) == [1, 2, 8]
    for P, (rounds, by_request, by_pipe) in rows.items():
        # the program has checked every round; both outcomes together are all of them
        assert rounds == ROUNDS and by_request + by_pipe == ROUNDS, (P, rows[P])


def test_repeated_request_under_live_pipes_stays_deferred(life_lines):
    assert ["ok", "sequence"] in life_lines
