"""The D2FE_PREC_I8 conv kernels (csrc/conv_i8.hip: conv_i8_kernel, every tiling, the fused conv1a prologue included) one layer at a time on injected tensors,
through d2fe_debug_conv_layer_q of the development library, BIT FOR BIT against the numpy oracle (tests/helpers/i8_oracle.py), the sign of a zero included.

Every compiled (family, shape, pool, ReLU) of the mode -- it has the one-tile family alone -- runs conv_layer_ref's sweep: maps of 2x2 pixels, exactly one tile,
one past the tile and 7x47 on one image, 3 images of 7x47 in the padded layout (NaN around the input, poison around the output) with channel counts that leave
the last 32-channel tile partial, -0.0 / subnormal inputs, an all-zero input, and the two halves of a 512-channel tensor for the 1x1 head.  The quantiser
cases (ties, clamps, negative inputs, an all-zero weight channel, |acc| above 2^24) run on 6x34.  tests/test_i8_mode_cpu.py shows on the CPU that the cases are
what they claim and that this comparison rejects a wrong kernel.  Random weights are asymmetric in every index, so a swapped operand map cannot pass."""
import numpy as np
import pytest

from tests.helpers import conv_layer_ref as R
from tests.helpers import i8_cases as K
from tests.helpers import i8_oracle as O

pytestmark = pytest.mark.gpu

ERR_INVALID = -1      # include/d2fe.h
SHAPE_NAME = {R.S64: "cin64", R.S128_32: "cin128_t32", R.S128_16: "cin128_t16", R.S1X1: "1x1", R.SFUSED: "fused1b"}


@pytest.fixture(scope="module")
def fe():
    from d2slam_amd import api
    f = api.DevFrontEnd(api.SuperPointConfig(input_width=64, input_height=64, max_batch=1))
    yield f
    f.close()


def _run(fe, family, shape, n, H, W, cout, pool, relu, T, lay="tight", variant="rand", tile=1, inputs=None):
    """one launch on the caller's padded buffers -> (y [n, H', W', cout], True when nothing outside the output tensor was written)"""
    cin, _ = R.SHAPE_GEOM[shape]
    x, frames, w, b = inputs if inputs is not None else R.case_inputs(shape, n, H, W, cout, variant)
    ics, icoff, igap, ocs, ocoff, ogap = R.layout(lay, cin, cout)
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    out, ois = R.make_out(n, Ho, Wo, cout, ocs, ocoff, ogap)
    kw = dict(pool=pool, relu=relu, conv64_tile=tile)
    if shape == R.SFUSED:
        rs = W if lay == "tight" else W + 5
        fb, fis = R.pack_frames(frames, rs, 0 if lay == "tight" else 11)
        w1a, b1a = R.conv1a_weights()
        got = fe.debug_conv_layer_q(family, K.PREC_I8, shape, w, b, n, H, W, out, ocs, ocoff, ois, T, frames=fb, img_stride=rs, img_istride=fis, w1a=w1a, b1a=b1a, **kw)
    else:
        nb = None
        if lay.startswith("head"):      # real numbers in the other half of the 512 channels: a wrong in_coff reads plausible values, not NaN
            nb = np.maximum(np.random.RandomState(11).randn(n, H, W, ics), 0).astype(np.float32)
        xb, iis = R.pack_in(x, ics, icoff, igap, neighbours=nb)
        got = fe.debug_conv_layer_q(family, K.PREC_I8, shape, w, b, n, H, W, out, ocs, ocoff, ois, T, x=xb, in_cstride=ics, in_coff=icoff, in_img_stride=iis, **kw)
    return R.unpack_out(got, n, Ho, Wo, cout, ocs, ocoff, ois)


def _same(y, want, what):
    bad = R.bits(y) != R.bits(want)
    assert y.shape == want.shape and not bad.any(), "%s: %d of %d outputs differ from the oracle in bits, first %s: %r != %r" % (
        what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), y[tuple(np.argwhere(bad)[0])], want[tuple(np.argwhere(bad)[0])])


def _check(fe, family, shape, n, H, W, cout, pool, relu, lay="tight", variant="rand", tile=1):
    what = "family %d %s tile %d %dx%dx%d cout %d pool %d relu %d %s %s" % (family, SHAPE_NAME[shape], tile, n, H, W, cout, pool, relu, lay, variant)
    y, clean = _run(fe, family, shape, n, H, W, cout, pool, relu, K.range_of(shape), lay, variant, tile)
    assert clean, what + ": a float outside the output tensor was written"
    refs = K.case_refs(shape, n, H, W, cout, pool, relu, variant)
    for i in range(n):
        _same(y[i], refs[i], "%s image %d" % (what, i))
    return y


@pytest.mark.parametrize("shape,tile,pool,relu", K.compiled())
def test_every_compiled_kernel_at_its_edges(fe, shape, tile, pool, relu):
    for n, H, W, cout, lay, variant in R.sweep_cases(1, shape, tile):
        y = _check(fe, 1, shape, n, H, W, cout, pool, relu, lay, variant, tile)
        if variant == "zero" and shape != R.SFUSED:      # all-zero input: acc = 0, the output is max(bias, 0) exactly (the bias itself without ReLU)
            b = R.rand_weights(*R.SHAPE_GEOM[shape], cout)[1]
            assert np.array_equal(y, np.broadcast_to(np.maximum(b, 0) if relu else b, y.shape))


@pytest.mark.parametrize("shape,pool,relu", [(R.S64, True, True), (R.S64, False, True), (R.S128_32, True, True), (R.S128_16, False, True), (R.S1X1, False, False),
                                             (R.SFUSED, True, True)])
def test_what_the_extractor_would_launch(fe, shape, pool, relu):
    """family 0 = conv() of superpoint_host.hip in this process: launch_conv, which takes the one-tile kernels for this mode whatever D2FE_CONV_PC says"""
    th, tw, _ = R.tile_of(1, shape)
    for n, H, W, cout, lay, variant in [c for c in R.sweep_cases(1, shape) if (c[1], c[2]) in ((th + 1, tw + 1), (7, 47))]:
        _check(fe, 0, shape, n, H, W, cout, pool, relu, lay, variant)


def test_fused_shape_on_random_frames(fe):
    """conv1a inside the staging: 3 frames whose rows and images have padding bytes behind them, two tiles across and three down, both channel counts"""
    for cout in R.COUTS[R.SFUSED]:
        _check(fe, 1, R.SFUSED, 3, 9, 41, cout, True, True, "padded")


@pytest.mark.parametrize("kind", K.QUANT_KINDS)
def test_quantiser_cases_bit_for_bit(fe, kind):
    for shape, cout, pool, relu in K.quant_shapes(kind):
        cin, ks = R.SHAPE_GEOM[shape]
        x, w, b = K.quant_case(kind, cin, ks, cout)
        H, W = x.shape[:2]
        want = O.layer(x, w, b, K.T_UNIT, relu, pool)
        for family, tile in [(1, 1), (0, 1)] + ([(1, 0)] if shape == R.S64 else []):
            y, clean = _run(fe, family, shape, 1, H, W, cout, pool, relu, K.T_UNIT, "padded", tile=tile, inputs=(x[None], None, w, b))
            assert clean
            _same(y[0], want, "%s %s family %d tile %d" % (kind, SHAPE_NAME[shape], family, tile))


def test_hook_refusals_leave_the_handle_usable(fe):
    from d2slam_amd.api import D2FEError
    n, H, W, cout = 1, 4, 16, 128
    x, _, w, b = R.case_inputs(R.S128_16, n, H, W, cout)
    xb, iis = R.pack_in(x, 128, 0, 0)
    out, ois = R.make_out(n, H, W, cout, cout, 0, 0)
    good = dict(family=1, precision=K.PREC_I8, shape=R.S128_16, weight=w, bias=b, n=n, H=H, W=W, out=out, out_cstride=cout, out_coff=0, out_img_stride=ois, x=xb,
                in_cstride=128, in_coff=0, in_img_stride=iis, pool=False, relu=True, in_range=K.T_RAND)
    # the persistent family and convPb's own kernel do not exist in this mode; no pool on the 16-wide tile, and none without ReLU on the 32-wide one (same Cin);
    # the range must be finite and inside its limits; precision 4 stays unassigned; and the entry point without a range still refuses the mode
    bad = [dict(family=2), dict(family=3), dict(pool=True), dict(shape=R.S128_32, pool=True, relu=False), dict(in_range=0.0), dict(in_range=-1.0), dict(in_range=float("inf")), dict(in_range=float("nan")),
           dict(in_range=1e-31), dict(in_range=1e31), dict(precision=4), dict(in_range=None)]
    for change in bad:
        with pytest.raises(D2FEError) as e:
            fe.debug_conv_layer(**dict(good, **change))
        assert e.value.code == ERR_INVALID, change
    got = fe.debug_conv_layer(**good)
    _same(got[:H * W * cout].reshape(H, W, cout), K.case_refs(R.S128_16, n, H, W, cout, False, True)[0], "after the refusals")
