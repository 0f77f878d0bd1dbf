"""D2FE_PREC_I8 on the GPU (include/d2fe.h, d2fe_precision): int8 operands, int32 accumulation.

The reference of every numeric check is tests/helpers/i8_oracle.py -- the contract in numpy -- never another mode of the library and never the mode itself.
An integer sum is exact and order-free, so the comparisons are BIT FOR BIT.

  1. every quantised layer against the oracle fed with the GPU's OWN input of that layer (ranges: calibrate.measure_ranges on the same images), also in a child
     process with D2FE_CONV_PC=0: the mode has no persistent kernels, the switch changes nothing;
  2. end to end against a CPU chain: the oracle's exact conv1a, the int8 oracle for conv1b .. convPb, then the oracle's softmax, selection and sampling.  The
     D2FE_PREC_F32 tests (tests/test_gpu_parity.py) hold the logits, the score map, the keypoint lists and the scores to the oracle bit for bit, so they are held
     bit for bit here; the descriptors there have the tolerance 1e-6 against the oracle's sampling, and here (as in tests/test_f16_mode.py) the same 1e-6 against
     the oracle's exact fp32 descriptor chains on the GPU's own conv4b -- the descriptor head stays fp32;
  3. bit identity of a frame's outputs across entry points, batch sizes, both pipes and with variant_b_pca;
  4. the ranges matter, and the changed output still equals the oracle;
  5. refusals and the life cycle of the ranges."""
import os
import subprocess
import sys

import numpy as np
import pytest

from d2slam_amd.synth import synth_image, synth_stereo
from tests.helpers import conv_layer_ref as R
from tests.helpers import i8_layers as il
from tests.helpers import i8_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR = 0.015
ERR_INVALID, ERR_NOT_READY = -1, -3      # include/d2fe.h


@pytest.fixture(scope="module")
def api():
    from d2slam_amd import api as a
    a.load_library()
    return a


@pytest.fixture(scope="module")
def ranges(api, sp_weights):
    """MinMax ranges of the per-layer images: every test of this module uses them (another image may exceed them: the clamp is part of the contract)"""
    from d2slam_amd import calibrate
    r = calibrate.measure_ranges(sp_weights, il.images())
    assert list(r) == list(O.SP_LAYERS) and all(np.isfinite(v) and v > 0 for v in r.values())
    return r


@pytest.fixture(scope="module")
def layer_tensors(api, sp_weights, ranges):
    return il.read_tensors(api, sp_weights, ranges)


# ---- 1. per layer --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layer", [l[0] for l in il.LAYERS])
def test_layer_equals_the_oracle_on_the_gpus_own_input(layer_tensors, sp_weights, ranges, layer):
    print("%s: %d outputs bit-equal" % (layer, il.check_layer(layer_tensors, sp_weights, ranges, layer)))


def test_layers_with_the_persistent_family_switched_off():
    """D2FE_CONV_PC=0 (the default is 2): the development library reads the switch once per process, hence the child process; same check, same images"""
    env = dict(os.environ, D2FE_CONV_PC="0")
    r = subprocess.run([sys.executable, "-m", "tests.helpers.i8_layers"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "I8_LAYERS_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_dense_head_layers_equal_the_oracle(api, sp_weights, ranges):
    """dense_descriptors handles evaluate convPa | convDa in one launch (512 channels, per-channel weight scales across both) and convDb on the second half of
    that buffer with convDa's range; convPb reads the first half"""
    n, Hc, Wc = 2, il.H // 8, il.W // 8
    fe = il.make_fe(api, sp_weights, ranges, n=n, dense_descriptors=True)
    fe.extract_batch(il.images()[:n], cap=200)
    a4b = fe.debug_read("conv4b", (n, Hc, Wc, 128)).copy()
    pada = fe.debug_read("convPaDa", (n, Hc, Wc, 512)).copy()
    logits = fe.debug_read("logits", (n, Hc, Wc, 65)).copy()
    draw = fe.debug_read("desc_raw", (n, Hc, Wc, 256)).copy()
    fe.close()
    for i in range(n):
        assert R.same_bits(pada[i][..., :256], O.layer(a4b[i], *sp_weights["convPa"], ranges["conv4b"], True, False)), "convPa, image %d" % i
        assert R.same_bits(pada[i][..., 256:], O.layer(a4b[i], *sp_weights["convDa"], ranges["conv4b"], True, False)), "convDa, image %d" % i
        assert R.same_bits(logits[i], O.layer(pada[i][..., :256], *sp_weights["convPb"], ranges["convPa"], False, False)), "convPb, image %d" % i
        assert R.same_bits(draw[i], O.layer(pada[i][..., 256:], *sp_weights["convDb"], ranges["convDa"], False, False)), "convDb, image %d" % i
    assert np.abs(draw).max() > 0


# ---- 2. end to end -------------------------------------------------------------------------------------------------------------------------------------------
def test_end_to_end_against_the_cpu_chain(api, orc, sp_weights, ranges):
    H, W, N = 96, 128, 200
    imgs = np.stack(synth_stereo(H, W, seed=3))
    fe = il.make_fe(api, sp_weights, ranges, H, W, 2, N=N, keypoint_threshold=THR, keep_score_map=True)
    res = fe.extract_batch(imgs, cap=N)
    semi = fe.debug_read("semi", (2, H, W)).copy()
    logits = fe.debug_read("logits", (2, H // 8, W // 8, 65)).copy()
    a4b = fe.debug_read("conv4b", (2, H // 8, W // 8, 128)).copy()
    fe.close()
    for i in range(2):
        c1a = orc.conv(orc.prep_u8(imgs[i])[:, :, None], *sp_weights["conv1a"], True)      # exact fp32 in every mode
        ref = O.chain(c1a, sp_weights, ranges)
        assert R.same_bits(a4b[i], ref["conv4b"]), "image %d: conv4b" % i
        assert R.same_bits(logits[i], ref["convPb"]), "image %d: logits" % i
        s = orc.softmax_semi(ref["convPb"])
        assert np.array_equal(semi[i], s), "image %d: score map" % i
        rk, rs, ri = orc.select_b(s, THR, 1, N)
        kps, sc, desc = res[i]
        assert len(kps) > 20
        assert np.array_equal(kps, rk) and np.array_equal(sc, rs), "image %d: keypoint list" % i
        # the descriptor head stays fp32: the oracle's exact chains on the GPU's own trunk, at the exact mode's descriptor tolerance
        cda = orc.conv(a4b[i], *sp_weights["convDa"], True)
        dmap = orc.l2norm_rows(orc.conv(cda, *sp_weights["convDb"], False))
        assert np.abs(desc - orc.sample_b(dmap, kps)).max() <= 1e-6


# ---- 3. bit identity across entry points ---------------------------------------------------------------------------------------------------------------------
def _same(a, b, what):
    assert len(a[0]) == len(b[0]) and len(a[0]) > 0, what
    for k, name in enumerate(("kps_xy", "scores", "desc")):
        assert R.same_bits(a[k], b[k]), "%s %s" % (what, name)


def test_one_image_equals_the_same_image_in_a_batch_of_five(api, sp_weights, ranges):
    H, W = 96, 128
    imgs = np.stack([synth_image(H, W, 60 + s) for s in range(5)])
    fe = il.make_fe(api, sp_weights, ranges, H, W, 5, N=100, dev=False)
    five = [tuple(x.copy() for x in r) for r in fe.extract_batch(imgs, cap=100)]
    for i in (0, 2, 4):
        one, = fe.extract_batch(imgs[i:i + 1], cap=100)
        _same(one, five[i], "image %d alone / in the batch" % i)
    fe.close()


def _stereo_pipe_equals_extract_batch(api, fe, H, W, CAP, F):
    pipe = api.StereoPipe(fe, lanes=2, frames=F, width=W, height=H, cap=CAP, netvlad=False)
    subs = []
    for s in range(3):
        pairs = [synth_stereo(H, W, seed=80 + 2 * s + f) for f in range(F)]
        subs.append((np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])))
    tickets = [pipe.submit(L, Rt) for L, Rt in subs[:2]]
    got = [{k: (None if v is None else v.copy()) for k, v in pipe.wait(t).items()} for t in tickets]
    got.append({k: (None if v is None else v.copy()) for k, v in pipe.wait(pipe.submit(*subs[2])).items()})
    for s, (L, Rt) in enumerate(subs):
        ext = fe.extract_batch(np.concatenate([L, Rt]), cap=CAP)
        for i in range(2 * F):
            n = int(got[s]["n_kp"][i])
            _same((got[s]["kps_xy"][i, :n], got[s]["scores"][i, :n], got[s]["desc"][i, :n]), ext[i], "submit %d image %d" % (s, i))
    pipe.close()


def test_stereo_pipe_equals_extract_batch(api, sp_weights, ranges):
    H, W, CAP, F = 96, 128, 100, 2
    fe = il.make_fe(api, sp_weights, ranges, H, W, 2 * F, N=CAP, dev=False)
    _stereo_pipe_equals_extract_batch(api, fe, H, W, CAP, F)
    fe.close()


def test_stereo_pipe_with_variant_b_pca_equals_extract_batch(api, sp_weights, ranges):
    from tests.test_pca_b_cpu import qr_pca
    H, W, CAP, F = 96, 128, 100, 2
    fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=CAP, input_width=W, input_height=H, max_batch=2 * F, precision=api.PREC_I8), variant_b_pca=True)
    fe.load_superpoint(sp_weights)
    fe.set_int8_ranges(ranges)
    fe.set_pca(*qr_pca(64))
    assert fe.desc_dim == 64
    _stereo_pipe_equals_extract_batch(api, fe, H, W, CAP, F)
    assert fe.extract_batch(synth_image(H, W, 5)[None], cap=CAP)[0][2].shape[1] == 64
    fe.close()


def test_quad_pipe_ticket_equals_extract_batch(api, sp_weights, ranges):
    from d2slam_amd import quadcam
    RH, RW, UH, UW, CAP = 240, 384, 120, 192, 60
    w = dict(sp_weights)
    Wt, b = w["convPb"]
    b = b.copy(); b[64] -= np.float32(3.5); w["convPb"] = (Wt, b)      # threshold 0.15 (the quadcam configuration) still finds keypoints
    fe = il.make_fe(api, w, ranges, UH, UW, 8, N=CAP, dev=False, keypoint_threshold=0.15)
    maps = [quadcam.synthetic_maps(c, RH, RW, UH, UW) for c in range(4)]
    pipe = api.QuadPipe(fe, maps, lanes=2, quads=2, raw_width=RW, raw_height=RH, width=UW, height=UH, cap=CAP, netvlad=False, radius_neighbour=0.2 * UW)
    raw = np.stack([np.stack([synth_image(RH, RW, 300 + 4 * q + c) for c in range(4)]) for q in range(2)])
    o = {k: (None if v is None else v.copy()) for k, v in pipe.wait(pipe.submit(raw)).items()}
    for q in range(2):
        views = np.stack([fe.undistort(raw[q, c], *maps[c]) for c in range(4)])
        ext = fe.extract_batch(views, cap=CAP)
        for c in range(4):
            n = int(o["n_kp"][q, c])
            _same((o["kps_xy"][q, c, :n], o["scores"][q, c, :n], o["desc"][q, c, :n]), ext[c], "quad frame %d view %d" % (q, c))
    pipe.close(); fe.close()


# ---- 4. the ranges matter ------------------------------------------------------------------------------------------------------------------------------------
def test_halving_a_range_changes_the_next_layer_and_still_equals_the_oracle(api, sp_weights, ranges, layer_tensors):
    half = dict(ranges, conv2a=ranges["conv2a"] / 2)
    t = il.read_tensors(api, sp_weights, half)
    assert R.same_bits(t["conv2a"], layer_tensors["conv2a"])                # conv2a itself reads conv1b's range
    assert not R.same_bits(t["conv2b"], layer_tensors["conv2b"])
    il.check_layer(t, sp_weights, half, "conv2b")
    with pytest.raises(AssertionError):
        il.check_layer(t, sp_weights, ranges, "conv2b")                      # and the comparison sees the difference


# ---- 5. refusals and life cycle --------------------------------------------------------------------------------------------------------------------------------
def _raises(code, fn, *needles):
    from d2slam_amd.api import D2FEError
    with pytest.raises(D2FEError) as e:
        fn()
    assert e.value.code == code, str(e.value)
    for s in needles:
        assert s in str(e.value), str(e.value)


def test_refusals_and_the_life_of_the_ranges(api, sp_weights, ranges):
    H, W, CAP = 96, 128, 50
    img = synth_image(H, W, 9)[None]
    cfg = api.SuperPointConfig(max_keypoints=CAP, input_width=W, input_height=H, max_batch=2, precision=api.PREC_I8)
    _raises(ERR_INVALID, lambda: api.FrontEnd(cfg, exact_order=True), "D2FE_PREC_I8")
    fe = api.FrontEnd(cfg)
    _raises(ERR_NOT_READY, lambda: fe.set_int8_ranges(ranges))                                       # before the weights
    fe.load_superpoint(sp_weights)
    _raises(ERR_NOT_READY, lambda: fe.extract_batch(img, cap=CAP), "ranges")                         # before the ranges
    _raises(ERR_NOT_READY, lambda: api.StereoPipe(fe, lanes=1, frames=1, width=W, height=H, cap=CAP, netvlad=False), "ranges")
    for bad, name in ((0.0, "conv2a"), (float("nan"), "conv4b"), (float("inf"), "conv1a"), (-1.0, "convPa"), (1e-31, "conv3b"), (1e31, "convDa")):
        _raises(ERR_INVALID, lambda: fe.set_int8_ranges(dict(ranges, **{name: bad})), name)
    _raises(ERR_NOT_READY, lambda: fe.extract_batch(img, cap=CAP))                                   # a refused call sets nothing
    _raises(ERR_INVALID, lambda: fe.set_int8_ranges([1.0] * 11))
    fe.set_int8_ranges(dict(ranges, convPb=float("nan"), convDb=0.0))                                # the two ignored entries may hold anything
    first = tuple(x.copy() for x in fe.extract_batch(img, cap=CAP)[0])
    assert len(first[0]) > 0
    pipe = api.StereoPipe(fe, lanes=1, frames=1, width=W, height=H, cap=CAP, netvlad=False)
    _raises(ERR_INVALID, lambda: fe.set_int8_ranges(ranges), "pipes")                                # a load: refused while pipes are alive
    pipe.close()
    fe.load_superpoint(sp_weights)                                                                   # a reload clears the ranges
    _raises(ERR_NOT_READY, lambda: fe.extract_batch(img, cap=CAP), "ranges")
    fe.set_int8_ranges(ranges)
    _same(tuple(fe.extract_batch(img, cap=CAP)[0]), first, "after the reload")
    fe.close()
    other = api.FrontEnd(api.SuperPointConfig(max_keypoints=CAP, input_width=W, input_height=H, max_batch=1, precision=api.PREC_F16))
    other.load_superpoint(sp_weights)
    _raises(ERR_INVALID, lambda: other.set_int8_ranges(ranges), "D2FE_PREC_I8")                      # not an int8 handle
    other.close()


def test_host_pointer_calls_after_new_ranges_return_the_new_bits(api, sp_weights, ranges):
    """three calls per geometry: the second captures the launch sequence, the third replays it -- a graph kept across set_int8_ranges would replay the old r"""
    H, W, CAP = 96, 128, 100
    img = synth_image(H, W, 21)[None]
    new = {k: v * 0.6 for k, v in ranges.items()}
    fresh = il.make_fe(api, sp_weights, new, H, W, 1, N=CAP, dev=False)
    want = tuple(x.copy() for x in fresh.extract_batch(img, cap=CAP)[0])
    fresh.close()
    fe = il.make_fe(api, sp_weights, ranges, H, W, 1, N=CAP, dev=False)
    old = [tuple(x.copy() for x in fe.extract_batch(img, cap=CAP)[0]) for _ in range(3)]
    _same(old[1], old[0], "second call"); _same(old[2], old[0], "third call (replay)")
    fe.set_int8_ranges(new)
    for k in range(3):
        _same(tuple(fe.extract_batch(img, cap=CAP)[0]), want, "call %d after the new ranges" % k)
    assert not (len(old[0][1]) == len(want[1]) and R.same_bits(old[0][1], want[1])), "the new ranges changed nothing: the test shows nothing"
    fe.close()
