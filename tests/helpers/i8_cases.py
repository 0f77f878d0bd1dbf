"""Cases, references and mutants for ONE layer of D2FE_PREC_I8 (csrc/conv_i8.hip), shared by tests/test_i8_mode_cpu.py (no GPU: the cases are what they claim,
the comparison rejects mutants) and tests/test_i8_layer_edges.py (GPU, through d2fe_debug_conv_layer_q).  The reference is tests/helpers/i8_oracle.py and the
comparison is bit for bit (conv_layer_ref.same_bits: the sign of a zero included); buffers, layouts, sizes and random inputs are conv_layer_ref's.

Ranges of the random cases are fixed numbers BELOW the tensors' largest values, so that the upper clamp acts on a few activations of every case:
max(N(0, 1), 0) activations against T = 3, conv1a outputs of rand_frames against T = 1.5."""
import functools

import numpy as np

from tests.helpers import conv_layer_ref as R
from tests.helpers import i8_oracle as O

PREC_I8 = 5
T_RAND = 3.0       # rand_act: about 0.13 % of the activations lie above it
T_FUSED = 1.5      # conv1a outputs of rand_frames under conv1a_weights reach about 2
T_UNIT = 127.0     # the quantiser cases: r = s_x = 1, so q_x = rint(clamp(x))


def compiled():
    """every (shape, conv64_tile, pool, relu) launch_conv_i8 compiles: the one-tile family alone; the pool only with ReLU (the network has no other pooled layer)"""
    out = []
    for tile in (1, 0):
        out += [(R.S64, tile, False, False), (R.S64, tile, False, True), (R.S64, tile, True, True)]
    out += [(R.S128_32, 1, False, False), (R.S128_32, 1, False, True), (R.S128_32, 1, True, True)]
    out += [(R.S128_16, 1, False, r) for r in (False, True)] + [(R.S1X1, 1, False, r) for r in (False, True)]
    out += [(R.SFUSED, 1, True, True)]
    return out


def range_of(shape):
    return T_FUSED if shape == R.SFUSED else T_RAND


@functools.lru_cache(maxsize=None)
def case_refs(shape, n, H, W, cout, pool, relu, variant="rand"):
    """the oracle's output of every image of a conv_layer_ref case"""
    x, frames, w, b = R.case_inputs(shape, n, H, W, cout, variant)
    refs = []
    for i in range(n):
        xi = R.conv1a_act(R._oracle(), frames[i], *R.conv1a_weights()) if shape == R.SFUSED else x[i]
        y = O.layer(xi, w, b, range_of(shape), relu, pool)
        y.setflags(write=False)
        refs.append(y)
    return tuple(refs)


# ---- the quantiser cases (T = 127: r = 1) -----------------------------------------------------------------------------------------------------------------------
QUANT_KINDS = ("ties", "clamp", "negative", "zero_channel", "big_acc")
BIG_ACC = 9 * 128 * 127 * 127      # 18 580 608 > 2^24


@functools.lru_cache(maxsize=None)
def quant_case(kind, cin, ks, cout, H=6, W=34):
    """(x [H, W, cin], w [cout, cin, ks, ks], b [cout]) fp32"""
    rng = np.random.RandomState(919 + 23 * QUANT_KINDS.index(kind) + cin + ks + cout)
    w, b = [a.copy() for a in R.rand_weights(cin, ks, cout, seed=5)]
    x = rng.randint(0, 40, (H, W, cin)).astype(np.float32) * (rng.rand(H, W, cin) < 0.4)
    hot = rng.rand(H, W, cin) < 0.3
    m = int(hot.sum())
    if kind == "ties":           # k + 0.5 for even and odd k: round half to even takes k for even k, k + 1 for odd k
        x[hot] = rng.randint(0, 126, m) + 0.5
    elif kind == "clamp":        # at and beyond the clamp: all become 127
        x[hot] = rng.choice(np.array([126.5, 127.0, 127.49, 127.5, 128.0, 1e9, np.inf], np.float32), m)
    elif kind == "negative":     # negative inputs down to -127, never -128: rint(-127.5) would be -128 without the clamp in front of it
        x[hot] = rng.choice(np.array([-0.5, -1.5, -2.5, -63.0, -126.5, -127.0, -127.5, -128.0, -200.0, -1e9, -np.inf], np.float32), m)
    elif kind == "zero_channel":     # all-zero weight channels (the first, one in the middle, the last): s_w = 1, acc = 0, y = bias
        for c in (0, cout // 2, cout - 1):
            w[c] = 0
    elif kind == "big_acc":
        # every q_x = q_w = 127: acc = 9 Cin 127^2 at the interior pixels (18 580 608 for Cin 128, above 2^24 and even: exact); in the right half channel 0
        # holds 126 at random places, so that acc = 18 580 608 - 127 j is ODD for odd j: no fp32 number, the conversion must round to nearest even
        x = np.full((H, W, cin), 127.0, np.float32)
        x[:, W // 2:, 0] = np.where(rng.rand(H, W - W // 2) < 0.4, 126.0, 127.0)
        w = np.full((cout, cin, ks, ks), 0.75, np.float32)
        w[1::2] = 0.375      # another amax: d_c differs between the channels
    else:
        raise KeyError(kind)
    return R._ro(x.astype(np.float32), w.astype(np.float32), b.astype(np.float32))


# (shape, cout, pool, relu) the quantiser cases run on, as conv_layer_ref's exact cases; big_acc needs 9 * 128 products per output
QUANT_SHAPES = [(R.S64, 64, True, True), (R.S128_32, 128, True, True), (R.S128_16, 128, False, True), (R.S1X1, 65, False, False)]


def quant_shapes(kind):
    return [s for s in QUANT_SHAPES if kind != "big_acc" or s[0] in (R.S128_32, R.S128_16)]


# ---- mutants: what a wrong kernel or a wrong packing would compute ---------------------------------------------------------------------------------------------
MUTANTS = ("trunc_quant", "per_tensor_w", "clamp_m128", "dropped_tap", "dropped_bias", "pool_anchor")


def mutant_layer(name, x, w, b, T, relu, pool):
    r, s_x = O.input_scales(T)
    qw, s_w = O.quant_weights(w)
    qx = O.quant_act(x, r)
    anchor = False
    if name == "trunc_quant":          # a truncating conversion in place of round half to even
        with np.errstate(over="ignore", invalid="ignore"):
            v = np.minimum(np.maximum(np.asarray(x, np.float32) * r, np.float32(-127)), np.float32(127))
        qx = np.trunc(v).astype(np.int64)
    elif name == "per_tensor_w":       # ONE weight scale for the layer
        amax = np.float32(np.abs(w).max())
        qw = np.clip(np.rint(np.asarray(w, np.float64) * 127.0 / float(amax)), -127, 127).astype(np.int64)
        s_w = np.full(w.shape[0], amax / np.float32(127), np.float32)
    elif name == "clamp_m128":         # the int8 range's own lower end
        with np.errstate(over="ignore", invalid="ignore"):
            v = np.minimum(np.maximum(np.asarray(x, np.float32) * r, np.float32(-128)), np.float32(127))
        qx = np.rint(v).astype(np.int64)
    elif name == "dropped_tap":        # the last (ky, kx, ci)
        qw = qw.copy()
        qw[:, -1, -1, -1] = 0
    elif name == "dropped_bias":
        b = np.zeros_like(b)
    elif name == "pool_anchor":
        anchor = True
    else:
        raise KeyError(name)
    return O.finish(O.epilogue(O.isum(qx, qw), s_x * s_w, b), relu, pool, anchor)


def float64_layer(x, w, b, T):
    """an independent evaluation of the same operands (q_x, q_w, d_c, bias): float64 products and sums through conv_layer_ref.corr, then t = acc * d_c and t + bias
    in float64.  The sum is exact there (|acc| < 2^31, every product an integer); the two float64 roundings behind it are 2^-53 relative, 2^-29 of an fp32
    ulp.  -> (acc, t, y) float64, before ReLU and pool"""
    r, s_x = O.input_scales(T)
    qw, s_w = O.quant_weights(w)
    d = (s_x * s_w).astype(np.float64)
    acc = R.corr(O.quant_act(x, r).astype(np.float64), qw.astype(np.float64))
    t = acc * d
    return acc, t, t + np.asarray(b, np.float64)
