"""D2FE_PREC_I8 without a GPU: the numpy oracle (tests/helpers/i8_oracle.py) against an independent float64 evaluation of the same quantised operands, the
quantiser cases of tests/helpers/i8_cases.py shown to be what they claim, and the bitwise comparison shown to reject mutants.

Oracle against float64.  Before the epilogue the two are EQUAL (integers below 2^31).  Behind it the oracle rounds three times: (float)acc (only when
|acc| > 2^24), t = fl32(acc * d_c) and y = fl32(t + bias), so with u = 2^-24
    |y_oracle - y_float64| <= ulp(t) / 2 + [|acc| > 2^24] u |t| + ulp(y) / 2        (+ 2^-40 |t| for the float64 side's own roundings).
Where |acc| <= 2^24 and the bias does not cancel the product (|y| >= |t|) this is within ONE fp32 ulp of y, asserted as such; under cancellation ulp(t) exceeds
ulp(y) and no bound in ulps of y exists -- the first term is the contract's own second rounding, not an error of the oracle."""
import numpy as np
import pytest

from tests.helpers import conv_layer_ref as R
from tests.helpers import i8_cases as K
from tests.helpers import i8_oracle as O

F32 = np.float32


def _ulp(v):
    return np.spacing(np.abs(np.asarray(v, np.float64)).astype(F32)).astype(np.float64)


def _pre(x, w, b, T):
    """the oracle before ReLU and pool: (acc int64, y fp32)"""
    r, s_x = O.input_scales(T)
    qw, s_w = O.quant_weights(w)
    acc = O.isum(O.quant_act(x, r), qw)
    return acc, O.epilogue(acc, s_x * s_w, b)


CASES = [(R.S64, 5, 33, 72), (R.S128_16, 5, 17, 136), (R.S1X1, 5, 17, 65)]


@pytest.mark.parametrize("shape,H,W,cout", CASES)
def test_oracle_against_float64(shape, H, W, cout):
    x, _, w, b = R.case_inputs(shape, 1, H, W, cout)
    acc, y = _pre(x[0], w, b, K.T_RAND)
    acc64, t64, y64 = K.float64_layer(x[0], w, b, K.T_RAND)
    assert np.array_equal(acc.astype(np.float64), acc64) and np.abs(acc).max() > 1000
    big = np.abs(acc64) > 2.0 ** 24
    bound = _ulp(t64) / 2 + big * 2.0 ** -24 * np.abs(t64) + _ulp(y) / 2 + 2.0 ** -40 * np.abs(t64)
    err = np.abs(y.astype(np.float64) - y64)
    assert np.all(err <= bound), float((err / bound).max())
    plain = ~big & (np.abs(y64) >= np.abs(t64))
    assert plain.mean() > 0.2 and np.all(err[plain] <= _ulp(y)[plain])      # "within 1 ulp" where nothing cancels
    assert y.dtype == F32 and O.layer(x[0], w, b, K.T_RAND, True, False).dtype == F32


def test_oracle_against_float64_above_2_24():
    x, w, b = K.quant_case("big_acc", 128, 3, 128)
    acc, y = _pre(x, w, b, K.T_UNIT)
    acc64, t64, y64 = K.float64_layer(x, w, b, K.T_UNIT)
    assert np.array_equal(acc.astype(np.float64), acc64)
    bound = _ulp(t64) / 2 + 2.0 ** -24 * np.abs(t64) + _ulp(y) / 2 + 2.0 ** -40 * np.abs(t64)
    assert np.all(np.abs(y.astype(np.float64) - y64) <= bound)


def test_scales_are_float32_and_weights_round_half_to_even():
    r, s_x = O.input_scales(3.0)
    assert type(r) is F32 and type(s_x) is F32 and r == F32(127) / F32(3) and s_x == F32(3) / F32(127)
    w = np.zeros((3, 1, 1, 4), F32)
    w[0, 0, 0] = [127, 0.5, 1.5, -2.5]        # amax 127: w * 127 / amax = w, ties go to the even neighbour
    w[1, 0, 0] = [0.25, -0.25, 0.125, 0]      # amax 0.25: 127, -127, 63.5 -> 64
    q, s_w = O.quant_weights(w)
    assert q[0, 0, 0].tolist() == [127, 0, 2, -2] and q[1, 0, 0].tolist() == [127, -127, 64, 0]
    assert q[2].tolist() == [[[0, 0, 0, 0]]] and s_w[2] == 1 and s_w.dtype == F32      # the all-zero channel
    assert s_w[0] == F32(1) and s_w[1] == F32(0.25) / F32(127)


def test_quantiser_ties_clamp_and_negative_inputs():
    q = lambda v: O.quant_act(np.array(v, F32), F32(1)).tolist()
    assert q([0.5, 1.5, 2.5, 3.5, 124.5, 125.5]) == [0, 2, 2, 4, 124, 126]               # k + 0.5: even k down, odd k up
    assert q([126.5, 127.0, 127.49, 127.5, 1e9, np.inf]) == [126, 127, 127, 127, 127, 127]
    assert q([-0.5, -1.5, -126.5, -127.0, -127.5, -128.0, -1e9, -np.inf]) == [0, -2, -126, -127, -127, -127, -127, -127]      # never -128
    # the product x * r is an fp32 product: 0.1f * (127 / 3)f, not the real-number one
    r, _ = O.input_scales(3.0)
    assert O.quant_act(np.array([0.1], F32), r)[0] == int(np.rint(F32(0.1) * r))


@pytest.mark.parametrize("kind", K.QUANT_KINDS)
def test_quantiser_cases_are_what_they_claim(kind):
    for shape, cout, pool, relu in K.quant_shapes(kind):
        cin, ks = R.SHAPE_GEOM[shape]
        x, w, b = K.quant_case(kind, cin, ks, cout)
        assert x.shape == (6, 34, cin)
        r, s_x = O.input_scales(K.T_UNIT)
        assert r == 1 and s_x == 1
        qx = O.quant_act(x, r)
        assert qx.min() >= -127 and qx.max() <= 127
        acc, y = _pre(x, w, b, K.T_UNIT)
        if kind == "ties":
            frac = x - np.floor(x)
            k = np.floor(x[frac == 0.5]).astype(int)
            assert (k % 2 == 0).sum() > 50 and (k % 2 == 1).sum() > 50
            assert np.array_equal(qx[frac == 0.5], k + (k % 2))
        elif kind == "clamp":
            for v in (127.5, 1e9, np.inf):
                assert (x == F32(v)).sum() > 10 and np.all(qx[x == F32(v)] == 127)
        elif kind == "negative":
            assert (x == F32(-127.5)).sum() > 10 and (x == -np.inf).sum() > 10 and qx.min() == -127
            assert np.all(qx[x <= -127] == -127)
        elif kind == "zero_channel":
            for c in (0, cout // 2, cout - 1):
                assert np.all(acc[:, :, c] == 0) and np.all(y[:, :, c] == b[c])      # y = bias, bit for bit
            assert np.abs(acc[:, :, 1]).max() > 0
        elif kind == "big_acc":
            assert acc[2, 3, 0] == K.BIG_ACC == 18580608 and K.BIG_ACC > 2 ** 24
            odd = (acc % 2 == 1) & (acc > 2 ** 24)
            assert odd.sum() > 100      # no fp32 number: (float)acc rounds
            a32 = acc.astype(F32).astype(np.int64)
            assert np.all(np.abs(a32[odd] - acc[odd]) == 1) and np.all(a32[odd] % 4 == 0)      # to the even significand, both ways
            assert (a32[odd] > acc[odd]).any() and (a32[odd] < acc[odd]).any()


# (mutant, quantiser kind or None for a random case, shape, cout, pool, relu, H, W)
REJECT = [("trunc_quant", "ties", R.S64, 64, True, True), ("trunc_quant", None, R.S128_16, 128, False, True), ("per_tensor_w", None, R.S64, 64, False, True),
          ("per_tensor_w", "big_acc", R.S128_16, 128, False, True), ("clamp_m128", "negative", R.S1X1, 65, False, False),
          ("clamp_m128", "negative", R.S64, 64, True, True), ("dropped_tap", None, R.S128_32, 128, True, True), ("dropped_tap", "ties", R.S1X1, 65, False, False),
          ("dropped_bias", None, R.S64, 64, True, True), ("dropped_bias", "zero_channel", R.S1X1, 65, False, False), ("pool_anchor", None, R.S64, 64, True, True),
          ("pool_anchor", None, R.S128_32, 128, True, True)]


@pytest.mark.parametrize("mutant,kind,shape,cout,pool,relu", REJECT)
def test_the_bitwise_comparison_rejects_mutants(mutant, kind, shape, cout, pool, relu):
    cin, ks = R.SHAPE_GEOM[shape]
    if kind is None:
        x, w, b, T = R.rand_act(1, 7, 47, cin)[0], *R.rand_weights(cin, ks, cout), K.T_RAND      # 7 x 47: odd both ways, the pool's floor drops a row and a column
    else:
        x, w, b = K.quant_case(kind, cin, ks, cout)
        T = K.T_UNIT
    want = O.layer(x, w, b, T, relu, pool)
    got = K.mutant_layer(mutant, x, w, b, T, relu, pool)
    assert got.shape == want.shape and not R.same_bits(got, want)
    assert R.same_bits(O.layer(x.copy(), w.copy(), b.copy(), T, relu, pool), want)      # and the oracle repeats itself


def test_sign_of_zero_and_relu():
    """ReLU writes +0 for every non-positive value, as the kernels do (v > 0 ? v : 0.f); without ReLU a negative zero survives"""
    y = np.array([[[-0.0, -1.0, 0.0, 2.0]]], F32)
    assert R.bits(O.finish(y, True, False)).tolist() == [[[0, 0, 0, 0x40000000]]]
    assert R.bits(O.finish(y, False, False))[0, 0, 0] == 0x80000000
    assert not R.same_bits(np.array([-0.0], F32), np.array([0.0], F32))


def test_compiled_table_and_ranges():
    c = K.compiled()
    assert len(c) == len(set(c)) == 14 and all(r for (_, _, p, r) in c if p)      # the pool only with ReLU
    assert {s for s, _, _, _ in c} == {R.S64, R.S128_32, R.S128_16, R.S1X1, R.SFUSED}
    # the ranges of the random cases clamp a few activations and leave most alone
    x = R.rand_act(3, 7, 47, 64)
    assert 0 < (x > K.T_RAND).mean() < 0.01
    assert O.INPUT_OF["convPa"] == O.INPUT_OF["convDa"] == "conv4b" and set(O.INPUT_OF) | {"conv1a"} == set(O.SP_LAYERS)


def test_calibration_dict_covers_the_plan():
    from d2slam_amd import calibrate
    from d2slam_amd.weights import SP_LAYERS
    assert tuple(SP_LAYERS) == O.SP_LAYERS
    names = {"convPa", "convDa"} | {{"logits": "convPb", "desc_raw": "convDb"}.get(n, n) for n, _, _ in calibrate._TENSORS if n != "convPaDa"}
    assert names == set(SP_LAYERS)
