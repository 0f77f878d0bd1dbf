"""The direct SuperPoint conv kernels -- conv_f32_kernel, conv1a_kernel, conv1a_mfma_kernel (conv.hip), conv_f16x2_kernel split and plain (conv_f16.hip),
conv_pc_kernel MODE 0 / 1 / 2 (conv_pc.hip), conv1x1_256_65_kernel (conv1x1.hip) -- one layer at a time on injected tensors, through d2fe_debug_conv_layer and
d2fe_debug_conv1a of the development library (include/d2fe_debug.h).  The extractor reaches these kernels with the network's own sizes, tight tensors and
activations of order 1; here every compiled (family, precision, shape, pool, ReLU) runs on maps of 2x2 pixels, exactly one tile, one past the tile and 7x47, on
1 and 3 images with gaps, with channel counts that leave the last 32-channel tile partial, and with poisoned padding around both tensors.

References and bounds: tests/helpers/conv_layer_ref.py (its docstring derives them); tests/test_conv_layer_edges_cpu.py shows on the CPU that the cases are what
they claim and that these comparisons reject a wrong kernel.
  D2FE_PREC_F32    the oracle's fmaf chains, bit for bit (-0.0, fp32 subnormal operands and products that underflow into the subnormal range included)
  D2FE_PREC_F16    f16_oracle.layer at (K + 2) 2^-24 S on random inputs; bit for bit on the exact cases (ties, clamps, fp16 subnormals)
  D2FE_PREC_F16X2  the contract of include/d2fe.h in float64 at (3 K + 2) 2^-24 S3 on random inputs; bit for bit on the exact cases (wide operands)

With D2FE_CONV_EDGES_REPORT=<file> in the environment the largest error / bound per (family, precision, shape) is written there when the module ends."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import conv_layer_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID, ERR_UNSUPPORTED = -1, -5      # include/d2fe.h
PREC_NAME = {R.PREC_F32: "f32", R.PREC_F16X2: "f16x2", R.PREC_F16: "f16"}
SHAPE_NAME = {R.S64: "cin64", R.S128_32: "cin128_t32", R.S128_16: "cin128_t16", R.S1X1: "1x1", R.SFUSED: "fused1b"}


@pytest.fixture(scope="module")
def fe():
    from d2slam_amd import api
    f = api.DevFrontEnd(api.SuperPointConfig(input_width=64, input_height=64, max_batch=1))
    yield f
    f.close()


@pytest.fixture(scope="module")
def worst():
    """largest error / bound seen per (family, precision, shape); 0 for the bitwise comparisons"""
    w = {}
    yield w
    path = os.environ.get("D2FE_CONV_EDGES_REPORT")
    if path:
        old = {}
        if os.path.exists(path):
            with open(path) as f:
                old = json.load(f)
        for k, v in w.items():
            old[k] = max(v, old.get(k, 0.0))
        with open(path, "w") as f:
            json.dump(old, f, indent=1, sort_keys=True)


def _note(worst, family, prec, shape, q):
    key = "family%d/%s/%s" % (family, PREC_NAME[prec], SHAPE_NAME[shape])
    worst[key] = max(worst.get(key, 0.0), 0.0 if q is None else q)


def _run(fe, family, prec, shape, n, H, W, cout, pool, relu, lay="tight", variant="rand", tile=1, ncu=0, inputs=None):
    """one launch on the caller's padded buffers -> (y [n, H', W', cout], True when nothing outside the output tensor was written)"""
    cin, _ = R.SHAPE_GEOM[shape]
    x, frames, w, b = inputs if inputs is not None else R.case_inputs(shape, n, H, W, cout, variant)
    ics, icoff, igap, ocs, ocoff, ogap = R.layout(lay, cin, cout)
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    out, ois = R.make_out(n, Ho, Wo, cout, ocs, ocoff, ogap)
    kw = dict(pool=pool, relu=relu, conv64_tile=tile, ncu=ncu)
    if shape == R.SFUSED:
        rs = W if lay == "tight" else W + 5
        fb, fis = R.pack_frames(frames, rs, 0 if lay == "tight" else 11)
        w1a, b1a = R.conv1a_weights()
        got = fe.debug_conv_layer(family, prec, shape, w, b, n, H, W, out, ocs, ocoff, ois, frames=fb, img_stride=rs, img_istride=fis, w1a=w1a, b1a=b1a, **kw)
    else:
        nb = None
        if lay.startswith("head"):      # real numbers in the other half of the 512 channels: a wrong in_coff reads plausible values, not NaN
            nb = np.maximum(np.random.RandomState(11).randn(n, H, W, ics), 0).astype(np.float32)
        xb, iis = R.pack_in(x, ics, icoff, igap, neighbours=nb)
        got = fe.debug_conv_layer(family, prec, shape, w, b, n, H, W, out, ocs, ocoff, ois, x=xb, in_cstride=ics, in_coff=icoff, in_img_stride=iis, **kw)
    return R.unpack_out(got, n, Ho, Wo, cout, ocs, ocoff, ois)


def _check(worst, fe, family, prec, shape, n, H, W, cout, pool, relu, lay="tight", variant="rand", tile=1, ncu=0):
    what = "family %d %s %s tile %d %dx%dx%d cout %d pool %d relu %d %s %s ncu %d" % (family, PREC_NAME[prec], SHAPE_NAME[shape], tile, n, H, W, cout, pool, relu,
                                                                                    lay, variant, ncu)
    y, clean = _run(fe, family, prec, shape, n, H, W, cout, pool, relu, lay, variant, tile, ncu)
    assert clean, what + ": a float outside the output tensor was written"
    refs = R.case_refs(prec, shape, n, H, W, cout, pool, relu, variant)
    for i in range(n):
        if refs[i][0] == "bound":      # the stated condition of the random-input cases, on every case compared
            assert R.layer_limit_ok(refs[i]), what + ": the bound exceeds 1 % of the tensor's largest |y|"
        ok, q, txt = R.compare(y[i], refs[i])
        if q is not None:
            print("%s image %d: largest error / bound = %.3g" % (what, i, q))
        _note(worst, family, prec, shape, q)
        assert ok, "%s image %d: %s" % (what, i, txt)
    return y


def _variants(prec, cases):
    """the -0.0 / subnormal / all-zero inputs belong to the bitwise mode; the fp16 modes get their operand edges from the exact cases"""
    return [c for c in cases if prec == R.PREC_F32 or c[5] == "rand"]


SWEEP = [(f, p, s, t, pl, rl) for f in (1, 2) for p in R.PRECS for (s, t, pl, rl) in R.compiled(f)]


@pytest.mark.parametrize("family,prec,shape,tile,pool,relu", SWEEP)
def test_every_compiled_kernel_at_its_edges(fe, worst, family, prec, shape, tile, pool, relu):
    for n, H, W, cout, lay, variant in _variants(prec, R.sweep_cases(family, shape, tile)):
        y = _check(worst, fe, family, prec, shape, n, H, W, cout, pool, relu, lay, variant, tile)
        if variant == "zero" and shape != R.SFUSED:      # all-zero input: the output is max(bias, 0) exactly (the bias itself without ReLU)
            b = R.rand_weights(*R.SHAPE_GEOM[shape], cout)[1]
            want = np.maximum(b, 0) if relu else b
            assert np.array_equal(y, np.broadcast_to(want, y.shape))


@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("shape,pool,relu", [(s, pl, rl) for (s, t, pl, rl) in R.compiled(2)])
def test_what_the_extractor_would_launch(fe, worst, prec, shape, pool, relu):
    """family 0 = conv() of superpoint_host.hip in this process: convPb's own kernel for the fp32 65-channel head, else launch_conv under the default switches"""
    th, tw, _ = R.tile_of(2, shape)
    picked = [c for c in _variants(prec, R.sweep_cases(2, shape)) if (c[1], c[2]) in ((th + 1, tw + 1), (7, 47))]
    assert {c[4] for c in picked} >= {"tight", "padded"} and len({c[3] for c in picked}) == len(R.COUTS[shape])      # one past the tile; 7x47 at every cout
    for n, H, W, cout, lay, variant in picked:
        _check(worst, fe, 0, prec, shape, n, H, W, cout, pool, relu, lay, variant)


@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("shape,cout,pool,relu", [(R.S64, 64, True, True), (R.SFUSED, 64, True, True), (R.S128_32, 128, True, True), (R.S128_16, 256, False, True),
                                                  (R.S1X1, 256, False, False)])
def test_persistent_walks(fe, worst, prec, shape, cout, pool, relu):
    """conv_pc_kernel: grid = min(items, ncu).  Fewer items than compute units, as many, one more, three rounds with a remainder, one workgroup walking everything."""
    n, H, W = R.WALK_GEOM
    total = R.pc_items(shape, n, H, W, cout)
    for ncu in R.walk_ncus(total):
        _check(worst, fe, 2, prec, shape, n, H, W, cout, pool, relu, "padded", "rand", ncu=ncu)


def test_conv1x1_256_65_walk_and_bit_identity(fe, worst):
    """ncu = 1: a grid of two workgroups walks the 31 m-tiles of 987 pixels in four rounds; equal to both generic 1x1 kernels and to the oracle, bit for bit"""
    n, H, W = R.WALK_GEOM
    lay = "head256"
    a = _check(worst, fe, 3, R.PREC_F32, R.S1X1, n, H, W, 65, False, False, "tight", ncu=1)
    for ncu, l in ((1, lay), (0, lay), (3, "head0"), (0, "tight")):
        y, clean = _run(fe, 3, R.PREC_F32, R.S1X1, n, H, W, 65, False, False, l, ncu=ncu)
        assert clean and R.same_bits(y, a), "ncu %d layout %s" % (ncu, l)
    for family in (1, 2):
        y, clean = _run(fe, family, R.PREC_F32, R.S1X1, n, H, W, 65, False, False, lay)
        assert clean and R.same_bits(y, a), "family %d" % family
    for hw in ((2, 2), (4, 16), (5, 17), (1, 128), (1, 129)):      # fewer pixels than one wave's 32; one workgroup's 128 and one more
        _check(worst, fe, 3, R.PREC_F32, R.S1X1, 1, hw[0], hw[1], 65, False, False, "tight")
    _check(worst, fe, 3, R.PREC_F32, R.S1X1, 3, 5, 33, 65, False, False, "tight", "special")


def test_conv1x1_256_65_refusals(fe):
    """every condition of launch_conv1x1_256_65's own test answers hipErrorNotSupported: the hook reports D2FE_ERR_UNSUPPORTED, nothing is written, and family 0
    falls back to the generic kernel with the same bits"""
    n, H, W = 2, 3, 5
    hw = H * W
    x, _, w65, b65 = R.case_inputs(R.S1X1, n, H, W, 65)
    w64, b64 = R.rand_weights(256, 1, 64)
    xin = np.full(n * hw * 520 + 64, R.NAN_IN, np.float32)
    base = dict(w=w65, b=b65, ics=256, icoff=0, iis=hw * 256, ocs=65, ois=hw * 65)
    bad = {"cout is not 65": dict(w=w64, b=b64, ocs=64, ois=hw * 64), "a gap between input images": dict(iis=hw * 256 + 4),
           "a gap between output images": dict(ois=hw * 65 + 1), "out_cstride below 65": dict(ocs=64, ois=hw * 64),
           "in_cstride no multiple of 4": dict(ics=258, iis=hw * 258), "in_coff no multiple of 4": dict(ics=260, icoff=2, iis=hw * 260),
           "in_coff + 256 beyond in_cstride": dict(ics=256, icoff=4, iis=hw * 256)}
    for what, change in bad.items():
        c = dict(base, **change)
        out = np.full(n * hw * 80 + 80, R.POISON, np.float32)
        rc, got = fe.debug_conv_layer(3, R.PREC_F32, R.S1X1, c["w"], c["b"], n, H, W, out, c["ocs"], 0, c["ois"], x=xin, in_cstride=c["ics"], in_coff=c["icoff"],
                                      in_img_stride=c["iis"], pool=False, relu=False, status=True)
        assert rc == ERR_UNSUPPORTED, "%s: status %d" % (what, rc)
        assert np.all(R.bits(got) == R.bits(R.POISON)), what + ": the output was written"
    # the same tensors with a gap between the images through family 0: refused by convPb's kernel, taken by the generic one; and the handle is still usable
    ref = R.case_refs(R.PREC_F32, R.S1X1, n, H, W, 65, False, False)
    y, clean = _run(fe, 0, R.PREC_F32, R.S1X1, n, H, W, 65, False, False, "padded")
    assert clean and all(R.same_bits(y[i], ref[i][1]) for i in range(n))
    y, clean = _run(fe, 3, R.PREC_F32, R.S1X1, n, H, W, 65, False, False, "tight")
    assert clean and all(R.same_bits(y[i], ref[i][1]) for i in range(n))


EXACT_SHAPES = [(R.S64, 64, True, True), (R.S128_32, 128, True, True), (R.S128_16, 128, False, True), (R.S1X1, 65, False, False)]


@pytest.mark.parametrize("prec,kind", [(p, k) for p in (R.PREC_F16, R.PREC_F16X2) for k in R.EXACT_FOR[p]])
@pytest.mark.parametrize("shape,cout,pool,relu", EXACT_SHAPES)
def test_exact_cases_bit_for_bit_in_every_family(fe, worst, prec, kind, shape, cout, pool, relu):
    """operands on a grid on which no fp32 addition can round (conv_layer_ref.exact_guard): every family returns the integer result bit for bit, hence the
    families agree with each other"""
    cin, ks = R.SHAPE_GEOM[shape]
    x, w, b = R.exact_case(kind, cin, ks, cout)
    H, W = x.shape[:2]
    R.exact_guard(prec, x, w, b)
    want = R.exact_value(prec, x, w, b, relu, pool, "f64")
    fams = [(1, 1), (2, 1), (0, 1)] + ([(1, 0)] if shape == R.S64 else [])
    for family, tile in fams:
        y, clean = _run(fe, family, prec, shape, 1, H, W, cout, pool, relu, "padded", tile=tile, inputs=(x[None], None, w, b))
        assert clean
        bad = R.bits(y[0]) != R.bits(want)
        assert not bad.any(), "family %d tile %d %s %s: %d of %d outputs differ from the exact value, first %s: %r != %r" % (
            family, tile, PREC_NAME[prec], kind, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), y[0][tuple(np.argwhere(bad)[0])],
            want[tuple(np.argwhere(bad)[0])])
        _note(worst, family, prec, shape, None)


@pytest.mark.parametrize("kernel", [0, 1, -1])
def test_conv1a_kernels(fe, orc, kernel):
    """conv1a_mfma_kernel (0), conv1a_kernel (1) and launch_conv1a's pick (-1) against the oracle bit for bit: widths around the 32-pixel m-tile and the 64-pixel
    block, rows with padding bytes behind them, 3 images with a gap, a guard behind the output"""
    w1a, b1a = R.conv1a_weights()
    for W in (1, 31, 32, 33, 65):
        n, H = 3, 5
        frames = R.rand_frames(n, H, W, seed=W)
        fb, fis = R.pack_frames(frames, W + 3, 11)
        out = np.full(n * H * W * 64 + 256, R.POISON, np.float32)
        got = fe.debug_conv1a(kernel, fb, W + 3, fis, n, H, W, w1a, b1a, out)
        assert np.all(R.bits(got[n * H * W * 64:]) == R.bits(R.POISON)), "W %d: written behind the output" % W
        y = got[:n * H * W * 64].reshape(n, H, W, 64)
        for i in range(n):
            assert R.same_bits(y[i], R.conv1a_act(orc, frames[i], w1a, b1a)), "kernel %d W %d image %d" % (kernel, W, i)


def test_hook_refusals_leave_the_handle_usable(fe):
    from d2slam_amd.api import D2FEError
    n, H, W, cout = 1, 4, 16, 128
    x, _, w, b = R.case_inputs(R.S128_16, n, H, W, cout)
    xb, iis = R.pack_in(x, 128, 0, 0)
    out, ois = R.make_out(n, H, W, cout, cout, 0, 0)
    good = dict(family=1, precision=0, shape=R.S128_16, weight=w, bias=b, n=n, H=H, W=W, out=out, out_cstride=cout, out_coff=0, out_img_stride=ois, x=xb,
                in_cstride=128, in_coff=0, in_img_stride=iis, pool=False, relu=True)
    w1a, b1a = R.conv1a_weights()
    w64, b64 = R.rand_weights(64, 3, 64)
    w72, b72 = R.rand_weights(64, 3, 72)
    bad = [dict(family=4), dict(family=-1), dict(precision=2), dict(shape=5), dict(pool=True), dict(family=2, relu=False), dict(family=2, pool=True),
           dict(conv64_tile=2, shape=R.S64, weight=w64, bias=b64, x=np.zeros(H * W * 64 + 8, np.float32), in_cstride=64, in_img_stride=H * W * 64, out_cstride=64),
           dict(in_cstride=130), dict(in_coff=2, in_cstride=132), dict(in_img_stride=iis + 2, n=1), dict(x=xb[:H * W * 128 - 1]), dict(out=out[:H * W * cout - 1]),
           # the last channels of the last pixel would lie behind the buffers (their 8 floats of slack included)
           dict(in_coff=12), dict(out_coff=9), dict(n=2), dict(H=5), dict(W=17), dict(ncu=-1), dict(ncu=5000), dict(n=0), dict(H=0), dict(x=None),
           dict(shape=R.SFUSED, pool=True, weight=w64, bias=b64, out_cstride=64),      # the fused shape without frames
           dict(shape=R.SFUSED, pool=True, weight=w72, bias=b72, out_cstride=72, frames=np.zeros(H * W + 8, np.uint8), img_stride=W, w1a=w1a, b1a=b1a),
           dict(shape=R.SFUSED, pool=True, weight=w64, bias=b64, out_cstride=64, frames=np.zeros(H * W - 1, np.uint8), img_stride=W, w1a=w1a, b1a=b1a),
           dict(family=3), dict(family=3, shape=R.S1X1, precision=1)]
    for change in bad:
        with pytest.raises(D2FEError) as e:
            fe.debug_conv_layer(**dict(good, **change))
        assert e.value.code == ERR_INVALID, change
    with pytest.raises(D2FEError) as e:
        fe.debug_conv1a(0, np.zeros(10, np.uint8), 4, 0, 1, 3, 4, w1a, b1a, np.zeros(3 * 4 * 64, np.float32))      # the frame buffer is too small
    assert e.value.code == ERR_INVALID
    with pytest.raises(D2FEError) as e:
        fe.debug_conv1a(2, np.zeros(12, np.uint8), 4, 0, 1, 3, 4, w1a, b1a, np.zeros(3 * 4 * 64, np.float32))
    assert e.value.code == ERR_INVALID
    with pytest.raises(D2FEError) as e:
        fe.debug_conv1a(0, np.zeros(12, np.uint8), 4, 0, 1, 3, 4, w1a, b1a, np.zeros(3 * 4 * 64 - 1, np.float32))
    assert e.value.code == ERR_INVALID
    got = fe.debug_conv_layer(**good)
    ref = R.case_refs(R.PREC_F32, R.S128_16, n, H, W, cout, False, True)
    assert R.same_bits(got[:H * W * cout].reshape(H, W, cout), ref[0][1])


SWITCHES = [{"D2FE_CONV_PC": "0"}, {"D2FE_CONV_PC": "1"}, {"D2FE_CONV64_TILE": "0"}, {"D2FE_CONV1X1": "0"}, {"D2FE_CONV1A_VALU": "1", "D2FE_FUSE1A": "0"}]


@pytest.mark.parametrize("switch", SWITCHES, ids=lambda s: ",".join("%s=%s" % kv for kv in s.items()))
def test_whole_network_under_every_non_default_switch(switch):
    """the development library reads its schedule switches once per process, hence one child process per non-default value (tests/helpers/conv_switch_worker.py):
    D2FE_PREC_F32 bit for bit against the oracle at every layer, D2FE_PREC_F16X2 at the end-to-end tolerances"""
    env = dict(os.environ, **switch)
    r = subprocess.run([sys.executable, "-m", "tests.helpers.conv_switch_worker"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=180)
    print(r.stdout)
    assert r.returncode == 0 and "CONV_SWITCH_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
