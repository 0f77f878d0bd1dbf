"""The SuperPoint layer plan (d2slam_amd/csrc/sp_plan.h: the network's layers, activation and allocation sizes, exact_order's crop layout and the weight packings
as data; superpoint_host.hip allocates, packs, launches and reads back from it)
compiled with g++ and run on the host (tests/cpp/sp_plan_test.cpp), plain and under the address and undefined-behaviour sanitizers, against arithmetic written out here from
d2slam_amd.weights: the layer shapes and the output sizes behind three flooring 2x2 pools; and against the numbers the host code carried as literals before the plan stated them."""
import os
import subprocess

import pytest

from d2slam_amd.weights import SP_LAYERS, SP_SHAPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 16x16: the smallest image check_geometry admits; 88x88: exact_order's crop; 101x99: floors at every pool level
SIZES = [(16, 16), (88, 88), (101, 99), (104, 136), (480, 640), (1500, 1500)]
POOLED = ("conv1b", "conv2b", "conv3b")      # the layers with a 2x2 max-pool behind them (SuperPoint's encoder)


def _expected(H, W):
    """name -> (out height, out width, channels): every layer follows its predecessor, the two heads both read conv4b"""
    out, h, w = {}, H, W
    for name in SP_LAYERS:
        if name in POOLED:
            h, w = h // 2, w // 2
        out[name] = (h, w, SP_SHAPES[name][0])
    return out


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def plan_lines(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sp_plan") / ("sp_plan_test_" + request.param))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags + ["-I", os.path.join(ROOT, "d2slam_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "sp_plan_test.cpp"), "-o", exe])
    # the program allocates nothing: leak checking (which needs ptrace rights some sandboxes withhold) has nothing to find
    r = subprocess.run([exe] + [str(v) for hw in SIZES for v in hw], capture_output=True, text=True, timeout=60,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stderr
    return [l.split() for l in r.stdout.splitlines()]


def test_layer_shapes_and_floored_output_sizes(plan_lines):
    rows = {(int(l[1]), int(l[2]), l[3]): l for l in plan_lines if l[0] == "layer"}
    heads = {(int(l[1]), int(l[2])): l for l in plan_lines if l[0] == "head"}
    assert len(rows) == len(SIZES) * len(SP_LAYERS)
    for H, W in SIZES:
        exp = _expected(H, W)
        for name in SP_LAYERS:
            l = rows[(H, W, name)]
            h, w, c = exp[name]
            assert (int(l[4]), int(l[5]), int(l[6]), int(l[7])) == (h, w, c, h * w * c), (H, W, name, l)
            assert (int(l[9]), int(l[10]), int(l[11])) == tuple(SP_SHAPES[name]), (name, l)
        # the dense head writes convPa | convDa, 512 channels, on the 8x8 cells
        assert (int(heads[(H, W)][4]), int(heads[(H, W)][5])) == (512, (H // 8) * (W // 8) * 512)


def test_allocation_sizes_are_the_written_out_multiples_of_the_image_area(plan_lines):
    """floats per image a handle allocates per activation buffer: H*W*64 for conv1a, then H*W times 16, 16, 4, 8, 2, 2, 2 and 8 (the heads' 512-channel buffer)"""
    rows = {(int(l[1]), int(l[2]), l[3]): int(l[4]) for l in plan_lines if l[0] == "alloc"}
    names = ["conv1a", "conv1b", "conv2a", "conv2b", "conv3a", "conv3b", "conv4a", "conv4b", "convPa"]
    assert len(rows) == len(SIZES) * len(names)
    for H, W in SIZES:
        assert [rows[(H, W, nm)] for nm in names] == [H * W * k for k in (64, 16, 16, 4, 8, 2, 2, 2, 8)], (H, W)


def test_crop_chain_layout_at_88(plan_lines):
    """exact_order's crop batch, floats per crop in front of each tensor: the ladder conv1b 44*44*64 | conv2a 44*44*64 | conv2b 22*22*64 | conv3a 22*22*128 |
    conv3b, conv4a, conv4b 11*11*128 | convPa 11*11*256 | convPb 121*65 | scores 88*88"""
    rows = [(l[1], int(l[2])) for l in plan_lines if l[0] == "crop"]
    sizes = [("conv1b", 44 * 44 * 64), ("conv2a", 44 * 44 * 64), ("conv2b", 22 * 22 * 64), ("conv3a", 22 * 22 * 128), ("conv3b", 121 * 128), ("conv4a", 121 * 128),
             ("conv4b", 121 * 128), ("convPa", 121 * 256), ("convPb", 121 * 65), ("scores", 88 * 88)]
    exp, off = [], 0
    for nm, n in sizes:
        exp.append((nm, off))
        off += n
    assert off == 2 * 44 * 44 * 64 + 22 * 22 * 64 + 22 * 22 * 128 + 3 * 121 * 128 + 121 * 256 + 121 * 65 + 88 * 88
    assert rows == exp + [("total", off)]


def test_packing_table(plan_lines):
    """one row per packing: parts, cout_pad, forced fp32 fragments, condition (0 always, 1 with the sparse descriptor head, 2 with exact_order)"""
    rows = [(int(l[1]), l[2], l[3], int(l[4]), int(l[5]), int(l[6])) for l in plan_lines if l[0] == "pack"]
    chain = [("conv1b", 64), ("conv2a", 64), ("conv2b", 64), ("conv3a", 128), ("conv3b", 128), ("conv4a", 128), ("conv4b", 128)]
    exp = [(nm, "-", pad, 0, 0) for nm, pad in chain]
    exp += [("convPa", "convDa", 512, 0, 0), ("convPb", "-", 128, 0, 0), ("convDb", "-", 256, 0, 0)]
    exp += [("convPa", "-", 256, 0, 1), ("convDa", "-", 256, 1, 1), ("convDb", "-", 256, 1, 1)]
    exp += [(nm, "-", pad, 1, 2) for nm, pad in chain + [("convPa", 256)]]
    assert len(exp) == 21
    assert rows == [(i,) + e for i, e in enumerate(exp)]
