"""The int8 calibration kernels (csrc/calib.hip: calib_stats_kernel, calib_conv1a_stats_kernel) on injected tensors, through d2fe_debug_calib_stats and
d2fe_debug_calib_conv1a of the development library.  Counts are integers: every histogram bin, n_zero, n_over and the bits of t_max are compared with
tests/helpers/calib_oracle.py BIT FOR BIT.

Values: exactly on the bin edges k * T / n_bins and one fp32 ulp either side, a == T (last bin, not over) and nextafter(T) (over), both zeros, negative values, fp32
subnormals, +inf.  Shapes: an element count that is no multiple of the launch's threads nor of 4, channel sub-ranges (offset 256 of 512: 16-byte loads with a
stride; the 65 logits: scalar loads), 128 / 2048 / 4096 bins, forced grids of 1, 3 and many workgroups, an all-zero tensor, every value in one bin (the worst case
for the atomics), two launches into one histogram, and the largest tensor of the suite, 64 x 96 x 512 floats.  conv1a: the histogram must equal the oracle's binning
of the stand-alone conv1a's output (d2fe_debug_conv1a), so values and counts are both exact."""
import numpy as np
import pytest

from tests.helpers import calib_oracle as O
from tests.helpers import conv_layer_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fe():
    from d2slam_amd import api
    f = api.DevFrontEnd(api.SuperPointConfig(input_width=64, input_height=64, max_batch=1))
    yield f
    f.close()


def _check(fe, x2d, ch_off, channels, n_bins, T=None, wgs=0, what=""):
    """both phases on tensor [pixels, ch_stride] against the oracle; T: the frozen range (default: the tensor's own)"""
    view = x2d[:, ch_off:ch_off + channels]
    bits, _, _, _ = fe.debug_calib_stats(x2d, ch_off, channels, 1.0, n_bins, 0, wgs)
    assert bits == int(O.t_max(view).view(np.uint32)), what
    if T is None:
        T, _ = O.frozen(O.t_max(view), n_bins)
    _, hist, nz, nov = fe.debug_calib_stats(x2d, ch_off, channels, T, n_bins, 1, wgs)
    h, z, o = O.binning(view, T, n_bins)
    assert (nz, nov) == (z, o), what
    assert np.array_equal(hist, h), (what, np.flatnonzero(hist != h)[:8])
    assert int(hist.sum()) + nz == view.size, what
    return hist, nz, nov


def _edge_values(T, n_bins):
    """k * T / n_bins as float32 for every k, one ulp below and above; T, nextafter(T); zeros, negatives, subnormals, inf"""
    T = np.float32(T)
    k = np.arange(0, n_bins + 1, dtype=np.float64)
    e = (k * float(T) / n_bins).astype(np.float32)
    v = np.concatenate([e, np.nextafter(e, np.float32(-1)), np.nextafter(e, np.float32(np.inf)), -e[1:50],
                        [T, np.nextafter(T, np.float32(np.inf)), np.float32(0.0), np.float32(-0.0), np.float32(np.inf), np.float32(-np.inf)],
                        np.array([1, 2, 0x7fffff, 0x800000, 0x80000001], np.uint32).view(np.float32)]).astype(np.float32)
    return v


@pytest.mark.parametrize("n_bins", [128, 2048, 4096])
@pytest.mark.parametrize("T", [1.0, 3.7, 1e-30, 6e4])
def test_bin_edges_zeros_subnormals_and_over_range(fe, n_bins, T):
    v = _edge_values(T, n_bins)
    v = v[np.abs(v) >= 0]      # (no NaN: outside the contract)
    pad = (-v.size) % 4
    x = np.concatenate([v, np.zeros(pad, np.float32)]).reshape(-1, 4)
    hist, nz, nov = _check(fe, x, 0, 4, n_bins, T=np.float32(T), what="vec")
    assert nov >= 3 and nz >= 3 + pad      # nextafter(T), both infinities; both zeros, nextafter(0, -1) = -tiny is no zero
    x1 = v.reshape(-1, 1)      # one channel: the scalar path on the same values
    assert np.array_equal(_check(fe, x1, 0, 1, n_bins, T=np.float32(T), what="scalar")[0], hist)


def test_t_itself_is_in_the_last_bin_and_the_next_float_is_over(fe):
    for T in (np.float32(0.3), np.float32(7.0), np.float32(1e-30)):
        x = np.array([[T, np.nextafter(T, np.float32(np.inf)), -T, 0.0]], np.float32)
        _, hist, nz, nov = fe.debug_calib_stats(x, 0, 4, T, 2048, 1)
        assert hist[2047] == 3 and hist.sum() == 3 and nov == 1 and nz == 1


@pytest.mark.parametrize("shape,ch_off,channels", [((1237, 1), 0, 1), ((997, 65), 0, 65), ((333, 512), 256, 256), ((333, 512), 0, 256), ((301, 64), 0, 64),
                                                   ((129, 68), 4, 60), ((129, 67), 3, 64)])
@pytest.mark.parametrize("wgs", [0, 1, 3])
def test_shapes_sub_ranges_and_grids(fe, shape, ch_off, channels, wgs):
    rng = np.random.RandomState(shape[0] + channels)
    x = np.maximum(rng.randn(*shape), 0).astype(np.float32) * np.float32(2.5)      # a ReLU tensor: about half zeros
    x[rng.randint(shape[0]), ch_off + rng.randint(channels)] = np.float32(11.0)
    x[:, :ch_off] = np.float32(99.0); x[:, ch_off + channels:] = np.float32(99.0)      # outside the view: must not be seen
    _check(fe, x, ch_off, channels, 2048, wgs=wgs, what=str((shape, ch_off, channels, wgs)))


def test_all_zero_and_all_in_one_bin(fe):
    x = np.zeros((4099, 64), np.float32)
    x[1::2] = np.float32(-0.0)
    hist, nz, nov = _check(fe, x, 0, 64, 2048)
    assert nz == x.size and hist.sum() == 0 and nov == 0
    one = np.full((4099, 64), np.float32(0.5), np.float32)      # every value in bin 1024 of T = 1: every lane of every wave adds to one LDS word
    hist, nz, nov = _check(fe, one, 0, 64, 2048, T=np.float32(1.0))
    assert hist[1024] == one.size and nz == 0


def test_two_launches_accumulate(fe):
    rng = np.random.RandomState(9)
    a = np.abs(rng.randn(777, 128)).astype(np.float32)
    b = np.abs(rng.randn(555, 65)).astype(np.float32) * np.float32(2.0)
    acc = fe.debug_calib_stats(a, 0, 128, 1.0, 2048, 0)
    acc = fe.debug_calib_stats(b, 0, 65, 1.0, 2048, 0, acc=acc)
    assert acc[0] == int(max(O.t_max(a), O.t_max(b)).view(np.uint32))
    T = np.float32(2.0)      # below both maxima: n_over accumulates too
    acc = fe.debug_calib_stats(a, 0, 128, T, 2048, 1)
    acc = fe.debug_calib_stats(b, 0, 65, T, 2048, 1, acc=acc)
    ha, za, oa = O.binning(a, T, 2048)
    hb, zb, ob = O.binning(b, T, 2048)
    assert np.array_equal(acc[1], ha + hb) and acc[2] == za + zb and acc[3] == oa + ob and oa + ob > 0


def test_largest_tensor(fe):
    rng = np.random.RandomState(10)
    x = np.maximum(rng.randn(64 * 96, 512), 0).astype(np.float32)
    _check(fe, x, 256, 256, 4096, what="convDa half")
    _check(fe, x, 0, 512, 2048, what="whole")


@pytest.mark.parametrize("H,W", [(24, 40), (17, 33)])
def test_conv1a_statistics_equal_the_binning_of_the_conv1a_output(fe, H, W):
    n = 3
    w1a, b1a = R.conv1a_weights()
    frames = np.array(R.rand_frames(n, H, W, seed=1))
    frames[1] = 0
    frames[2] = 255
    fb, fis = R.pack_frames(frames, W + 5, 13)
    act = fe.debug_conv1a(-1, fb, W + 5, fis, n, H, W, w1a, b1a, np.zeros(n * H * W * 64, np.float32)).reshape(n, H, W, 64)
    for n_bins in (128, 2048):
        bits, _, _, _ = fe.debug_calib_conv1a(fb, W + 5, fis, n, H, W, w1a, b1a, 1.0, n_bins, 0)
        assert bits == int(O.t_max(act).view(np.uint32))
        for T in (O.frozen(O.t_max(act), n_bins)[0], np.float32(0.5) * O.t_max(act)):      # the tensor's own range, and one it exceeds
            _, hist, nz, nov = fe.debug_calib_conv1a(fb, W + 5, fis, n, H, W, w1a, b1a, T, n_bins, 1)
            h, z, o = O.binning(act, T, n_bins)
            assert np.array_equal(hist, h) and (nz, nov) == (z, o), (n_bins, float(T))
            assert int(hist.sum()) + nz == act.size
    assert nov > 0 and nz > 0


def test_hook_refusals(fe):
    from d2slam_amd.api import D2FEError
    x = np.ones((8, 8), np.float32)
    for kw in (dict(n_bins=100), dict(n_bins=8192), dict(t=0.0), dict(t=float("inf")), dict(ch_off=4, channels=8), dict(channels=0), dict(phase=2), dict(wgs=-1)):
        a = dict(ch_off=0, channels=8, t=1.0, n_bins=2048, phase=1, wgs=0)
        a.update(kw)
        with pytest.raises(D2FEError) as e:
            fe.debug_calib_stats(x, a["ch_off"], a["channels"], a["t"], a["n_bins"], a["phase"], a["wgs"])
        assert e.value.code == -1, kw
