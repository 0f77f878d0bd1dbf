"""D2FE_PREC_F16 without a GPU: the operand rounding of the contract (include/d2fe.h) as the test oracle restates it, and the mode's declarations."""
import os
import re

import numpy as np

from tests.helpers import f16_oracle as fo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(h):
    return int(np.asarray(h, np.float16).view(np.uint16))


def test_operand_rounding_hand_cases():
    """ties go to the even fp16, the clamp acts at 65000, subnormals are kept"""
    r = lambda v, s=0: float(fo.round_operand(np.float32(v), s))
    # fp16 has 11 significant bits: spacing 2^-10 in [1, 2), 2 in [2048, 4096)
    assert r(1.0 + 2.0 ** -11) == 1.0                              # tie between 1 and 1 + 2^-10: even mantissa (0) wins
    assert r(1.0 + 3 * 2.0 ** -11) == 1.0 + 2 * 2.0 ** -10         # tie between 1 + 2^-10 (odd) and 1 + 2^-9 (even)
    assert r(1.0 + 2.0 ** -11 + 2.0 ** -20) == 1.0 + 2.0 ** -10    # just above the tie: up
    assert r(2049.0) == 2048.0 and r(2051.0) == 2052.0             # ties at spacing 2
    assert r(-2049.0) == -2048.0
    # the scaling is part of the helper: activations by 2^4, weights by 2^8
    assert r(0.5, fo.SA) == 8.0 and r(0.5, fo.SW) == 128.0
    assert r((1.0 + 2.0 ** -11) / 16.0, fo.SA) == 1.0              # the tie is a tie of the SCALED value, 1 + 2^-11
    # clamp: 65000 is not an fp16 number (spacing 32 up there); the nearest is 64992, and nothing becomes infinite
    assert r(65000.0) == 64992.0 and r(1e9) == 64992.0 and r(-1e9) == -64992.0
    assert r(4062.5, fo.SA) == 64992.0 and r(5000.0, fo.SA) == 64992.0
    assert np.isfinite(fo.round_operand(np.array([3e38, -3e38], np.float32), fo.SW).astype(np.float32)).all()
    # subnormals: below 2^-14 the spacing stays 2^-24 -- gradual underflow, nothing flushed
    assert _bits(fo.round_operand(np.float32(2.0 ** -24), 0)) == 0x0001
    assert _bits(fo.round_operand(np.float32(3 * 2.0 ** -24), 0)) == 0x0003
    assert _bits(fo.round_operand(np.float32(2.0 ** -25), 0)) == 0x0000          # tie between 0 and the smallest subnormal: even (0)
    assert _bits(fo.round_operand(np.float32(3 * 2.0 ** -25), 0)) == 0x0002      # tie between 1 and 2 units: even
    assert _bits(fo.round_operand(np.float32(2.0 ** -24 / 256.0), fo.SW)) == 0x0001   # a weight of 2^-32 survives as the smallest subnormal
    assert r(0.0) == 0.0


def test_oracle_layer_on_a_hand_case():
    """one 1x1 layer, two channels: value and S by hand, with a product that only exists because the subnormal weight is kept"""
    x = np.array([[[1.0 + 2.0 ** -11 / 1.0, 3.0]]], np.float32)       # x^ = 16 (tie to even), 48
    w = np.array([[[[0.25]], [[2.0 ** -32]]]], np.float32)             # w^ = 64, 2^-24
    b = np.array([-1.5], np.float32)
    y, S = fo.layer(x, w, b, relu=False, pool=False)
    want = (16.0 * 64.0 + 48.0 * 2.0 ** -24) * 2.0 ** -12 - 1.5
    assert y.shape == (1, 1, 1) and y[0, 0, 0] == want
    assert S[0, 0, 0] == (16.0 * 64.0 + 48.0 * 2.0 ** -24) * 2.0 ** -12 + 1.5
    y, _ = fo.layer(x, w, b, relu=True, pool=False)
    assert y[0, 0, 0] == 0.0


def test_python_constant():
    from d2slam_amd import api
    assert api.PREC_F16 == 3
    assert (api.PREC_F32, api.PREC_F16X2, api.PREC_F32_WINO) == (0, 1, 2)      # no existing mode moved


def test_header_declares_the_mode():
    src = open(os.path.join(ROOT, "include", "d2fe.h")).read()
    body = re.search(r"typedef enum \{([^}]*)\} d2fe_precision;", src, re.S).group(1)
    code = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    vals = dict((k, int(v)) for k, v in re.findall(r"(D2FE_PREC_\w+)\s*=\s*(\d+)", code))
    assert vals == {"D2FE_PREC_F32": 0, "D2FE_PREC_F16X2": 1, "D2FE_PREC_F32_WINO": 2, "D2FE_PREC_F16": 3}
    hpp = open(os.path.join(ROOT, "include", "d2fe.hpp")).read()
    assert "D2FE_PREC_F16 " in hpp or "D2FE_PREC_F16:" in hpp
