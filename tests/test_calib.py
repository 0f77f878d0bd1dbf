"""The int8 calibration session (include/d2fe.h, d2fe_calib_*; api.Int8Calibrator) on the product library.

Yardsticks: the maxima are those of calibrate.measure_ranges (the existing MinMax path) on the same images, bit for bit; the histograms are the oracle's binning
(tests/helpers/calib_oracle.py) of the tensors a development handle reads back with debug_read, bit for bit -- counts are integers.  Then: the statistics do not
depend on how the images are split into calls and batches, an image first seen in the histogram phase is counted in n_over, the refusals carry their documented
codes, the entropy ranges drive a D2FE_PREC_I8 handle, and one saturated blob does not set the entropy range of conv1a."""
import numpy as np
import pytest

from d2slam_amd.synth import synth_image
from tests.helpers import calib_oracle as O

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_NOT_READY = -1, -3      # include/d2fe.h
SIZES = [(96, 128), (90, 122)]           # the second: no multiple of 8, the pools floor
N_IMG = 6
# debug_read name, channel slice, channels of the buffer, pool divisor of every layer's output, in SP_LAYERS order
TENSORS = {"conv1a": ("conv1a", 0, 64, 64, 1), "conv1b": ("conv1b", 0, 64, 64, 2), "conv2a": ("conv2a", 0, 64, 64, 2), "conv2b": ("conv2b", 0, 64, 64, 4),
           "conv3a": ("conv3a", 0, 128, 128, 4), "conv3b": ("conv3b", 0, 128, 128, 8), "conv4a": ("conv4a", 0, 128, 128, 8), "conv4b": ("conv4b", 0, 128, 128, 8),
           "convPa": ("convPaDa", 0, 256, 512, 8), "convPb": ("logits", 0, 65, 65, 8), "convDa": ("convPaDa", 256, 256, 512, 8), "convDb": ("desc_raw", 0, 256, 256, 8)}


@pytest.fixture(scope="module")
def api():
    from d2slam_amd import api as a
    a.load_library()
    return a


def _images(H, W):
    return np.stack([synth_image(H, W, 70 + s) for s in range(N_IMG)])


def _fe(api, weights, H, W, batch, **kw):
    cfg = dict(max_keypoints=100, input_width=W, input_height=H, max_batch=batch, precision=api.PREC_F32, dense_descriptors=True)
    dev = kw.pop("dev", False)
    cfg.update(kw)
    fe = api.FrontEnd(api.SuperPointConfig(**cfg), dev=dev)
    if weights is not None:
        fe.load_superpoint(weights)
    return fe


def _two_pass(api, fe, chunks, n_bins=0, second=None):
    """a session over the image chunks (range phase), then over `second` or the same chunks (histogram phase) -> {layer: stats}, {method: ranges}"""
    cal = api.Int8Calibrator(fe, n_bins)
    try:
        for c in chunks:
            cal.collect(c)
        first = {name: cal.stats(name) for name in api.SP_LAYERS}
        mm0 = cal.ranges("minmax")
        cal.freeze()
        for c in (second if second is not None else chunks):
            cal.collect(c)
        stats = {name: cal.stats(name) for name in api.SP_LAYERS}
        ranges = {m: cal.ranges(m) for m in ("minmax", "entropy", "percentile")}
        assert ranges["minmax"] == mm0
        for name in api.SP_LAYERS:
            assert first[name]["hist"] is None and first[name]["n_zero"] == 0 and first[name]["t_max"] == stats[name]["t_max"]
        return stats, ranges
    finally:
        cal.close()


_CASES = {}


def _case(api, sp_weights, H, W):
    """per size, computed once: the images, measure_ranges on them, the tensors of a development handle, and one session's statistics (six images, max_batch 2,
    one call)"""
    if (H, W) in _CASES:
        return _CASES[(H, W)]
    from d2slam_amd import calibrate
    imgs = _images(H, W)
    mm = calibrate.measure_ranges(sp_weights, imgs)
    dev = _fe(api, sp_weights, H, W, N_IMG, dev=True)
    dev.extract_batch(imgs, cap=100)
    tensors = {}
    for name, (rd, off, ch, cs, div) in TENSORS.items():
        tensors[name] = dev.debug_read(rd, (N_IMG, H // div, W // div, cs))[..., off:off + ch].copy()
    dev.close()
    fe = _fe(api, sp_weights, H, W, 2)
    stats, ranges = _two_pass(api, fe, [imgs])
    fe.close()
    _CASES[(H, W)] = dict(H=H, W=W, imgs=imgs, mm=mm, tensors=tensors, stats=stats, ranges=ranges)
    return _CASES[(H, W)]


@pytest.fixture(scope="module", params=SIZES, ids=lambda s: "%dx%d" % s)
def case(request, api, sp_weights):
    return _case(api, sp_weights, *request.param)


@pytest.fixture(scope="module")
def case0(api, sp_weights):
    return _case(api, sp_weights, *SIZES[0])


def test_maxima_equal_measure_ranges(api, case):
    for name in api.SP_LAYERS:
        assert np.float32(case["stats"][name]["t_max"]).view(np.uint32) == np.float32(case["mm"][name]).view(np.uint32), name
        assert np.float32(case["ranges"]["minmax"][name]).view(np.uint32) == np.float32(case["mm"][name]).view(np.uint32), name


def test_histograms_equal_the_oracles_binning_of_the_read_back_tensors(api, case):
    for name in api.SP_LAYERS:
        x, s = case["tensors"][name], case["stats"][name]
        T, _ = O.frozen(O.t_max(x), 2048)
        assert T.view(np.uint32) == np.float32(s["t_max"]).view(np.uint32), name
        h, z, o = O.binning(x, T, 2048)
        assert s["n_total"] == x.size and (s["n_zero"], s["n_over"]) == (z, 0) and o == 0, name
        assert np.array_equal(s["hist"], h), (name, np.flatnonzero(s["hist"] != h)[:8])
        assert s["hist"][2047] >= 1      # the maximum itself


def test_ranges_follow_the_oracles_rules_on_the_devices_histograms(api, case0):
    case = case0
    for name in api.SP_LAYERS:
        s = case["stats"][name]
        T, _ = O.frozen(s["t_max"], 2048)
        assert np.float32(case["ranges"]["percentile"][name]).view(np.uint32) == O.percentile(s["hist"], T, 99.99)[0].view(np.uint32), name
        ent = np.float32(case["ranges"]["entropy"][name])
        assert 1e-30 <= ent <= T
        if name not in ("conv1a", "conv4b", "convDb"):      # the oracle's all-candidates loop takes a second per tensor: a ReLU tensor early and late, and a signed one
            continue
        table = O.entropy_table(s["hist"])
        mine = [i for i in table if O.edge(i, T, 2048).view(np.uint32) == ent.view(np.uint32)]
        best = min(table, key=lambda i: (table[i][0], i))
        assert mine, name
        i = mine[0]
        assert table[i][0] <= table[best][0] + O.summation_bound(2048, table[i][1], table[best][1]), name


def test_statistics_do_not_depend_on_calls_and_batches(api, sp_weights, case0):
    case = case0
    imgs = case["imgs"]
    fe = _fe(api, sp_weights, case["H"], case["W"], 2)
    try:
        for chunks in ([imgs[i:i + 1] for i in range(6)], [imgs[0:3], imgs[3:6]]):      # 6 x 1, 2 x 3 (sliced 2 + 1); the case itself is 1 x 6 (sliced 2 + 2 + 2)
            stats, ranges = _two_pass(api, fe, chunks)
            assert ranges == case["ranges"]
            for name in api.SP_LAYERS:
                a, b = stats[name], case["stats"][name]
                assert np.array_equal(a["hist"], b["hist"]) and {k: a[k] for k in a if k != "hist"} == {k: b[k] for k in b if k != "hist"}, name
    finally:
        fe.close()


def test_an_image_first_seen_in_the_histogram_phase_is_counted_in_n_over(api, sp_weights):
    H, W = SIZES[0]
    dark = (synth_image(H, W, 5) // 4).astype(np.uint8)
    bright = synth_image(H, W, 6)
    fe = _fe(api, sp_weights, H, W, 2)
    try:
        stats, _ = _two_pass(api, fe, [dark[None]], second=[np.stack([dark, bright])])
        only, _ = _two_pass(api, fe, [dark[None]])
    finally:
        fe.close()
    assert stats["conv1a"]["n_over"] > 0 and only["conv1a"]["n_over"] == 0
    for name in api.SP_LAYERS:
        s = stats[name]
        assert s["n_total"] == 2 * only[name]["n_total"] and int(s["hist"].sum()) + s["n_zero"] == s["n_total"] and s["hist"][2047] >= s["n_over"]


def test_refusals(api, sp_weights):
    H, W = SIZES[0]
    img = synth_image(H, W, 1)

    def refused(code, fn):
        with pytest.raises(api.D2FEError) as e:
            fn()
        assert e.value.code == code, (e.value.code, str(e.value))

    for kw in (dict(precision=api.PREC_I8), dict(precision=api.PREC_F16), dict(precision=api.PREC_F32_WINO), dict(dense_descriptors=False)):
        fe = _fe(api, sp_weights, H, W, 2, **kw)
        refused(ERR_INVALID, lambda: api.Int8Calibrator(fe))
        fe.close()
    fe = _fe(api, None, H, W, 2)
    refused(ERR_NOT_READY, lambda: api.Int8Calibrator(fe))      # no weights
    fe.load_superpoint(sp_weights)
    refused(ERR_INVALID, lambda: api.Int8Calibrator(fe, 100))
    cal = api.Int8Calibrator(fe, 128)
    refused(ERR_NOT_READY, cal.freeze)                            # no image yet
    refused(ERR_NOT_READY, lambda: cal.ranges("minmax"))
    refused(ERR_INVALID, lambda: cal.collect(np.zeros((H + 8, W), np.uint8)))      # larger than the handle
    refused(ERR_INVALID, lambda: cal.collect(np.zeros((8, 8), np.uint8)))
    cal.collect(img)
    refused(ERR_NOT_READY, lambda: cal.ranges("entropy"))         # needs the histogram phase
    refused(ERR_INVALID, lambda: cal.stats(12))
    assert cal.stats("conv1a")["hist"] is None
    refused(ERR_INVALID, lambda: fe.load_superpoint(sp_weights))  # the session is a user of the handle, as a pipe is
    refused(ERR_INVALID, lambda: api.Int8Calibrator(fe))          # one session at a time
    cal.freeze()
    refused(ERR_INVALID, cal.freeze)
    refused(ERR_INVALID, lambda: cal.ranges("percentile", 0.0))
    cal.collect(img)
    assert cal.stats("conv1a")["hist"].shape == (128,) and len(cal.ranges("entropy")) == 12
    cal.close()
    fe.load_superpoint(sp_weights)                                 # free again
    pipe = api.StereoPipe(fe, lanes=2, frames=1, width=W, height=H, cap=100, netvlad=False)
    refused(ERR_INVALID, lambda: api.Int8Calibrator(fe))          # beside a live pipe
    pipe.close()
    api.Int8Calibrator(fe).close()
    fe.close()


def test_entropy_ranges_drive_an_i8_handle(api, sp_weights, case):
    H, W = case["H"], case["W"]
    for method in ("entropy", "percentile", "minmax"):
        fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=100, input_width=W, input_height=H, max_batch=2, precision=api.PREC_I8))
        fe.load_superpoint(sp_weights)
        fe.set_int8_ranges(case["ranges"][method])
        out = fe.extract_batch(case["imgs"][:2], cap=100)
        fe.close()
        assert all(len(o[1]) > 10 and np.isfinite(o[2]).all() for o in out), method


def test_collect_ranges_equals_the_session(case0, sp_weights):
    from d2slam_amd import calibrate
    case = case0
    assert calibrate.collect_ranges(sp_weights, case["imgs"], batch=2) == case["ranges"]["entropy"]
    assert calibrate.collect_ranges(sp_weights, case["imgs"], method="minmax", batch=4) == case["mm"]
    assert calibrate.collect_ranges(sp_weights, case["imgs"], method="percentile", param=99.99, batch=6) == case["ranges"]["percentile"]


def test_one_saturated_blob_does_not_set_the_entropy_range_of_conv1a(api, sp_weights):
    H, W = SIZES[0]
    img = (synth_image(H, W, 9) // 4).astype(np.uint8)      # a dark scene ...
    img[40:43, 60:63] = 255                                  # ... with one saturated 3 x 3 blob
    fe = _fe(api, sp_weights, H, W, 1)
    try:
        _, ranges = _two_pass(api, fe, [img[None]])
    finally:
        fe.close()
    print("conv1a: entropy %.5f, minmax %.5f" % (ranges["entropy"]["conv1a"], ranges["minmax"]["conv1a"]))
    assert ranges["entropy"]["conv1a"] < ranges["minmax"]["conv1a"]
