"""The per-layer check of D2FE_PREC_I8 shared by tests/test_i8_mode.py and its worker process: one call on a development handle, every layer's input and
output read back, every quantised layer held BIT FOR BIT to the numpy oracle (tests/helpers/i8_oracle.py) on the GPU's own input.  The ranges are those
calibrate.measure_ranges finds on the same images.

Run as a module (python -m tests.helpers.i8_layers) it checks every layer in THIS process -- the development library reads D2FE_CONV_PC once per process.  The
mode has one-tile kernels only, so the switch must change nothing: the worker shows that a non-default value reaches the same kernels."""
import sys

import numpy as np

from tests.helpers import conv_layer_ref as R
from tests.helpers import i8_oracle as O
from tests.helpers.f16_layers import LAYERS, SHAPES, N_IMG, H, W      # the same layers, tensors and geometry as the fp16 mode's check


def images():
    from d2slam_amd.synth import synth_image
    return np.stack([synth_image(H, W, 40 + s) for s in range(N_IMG)])


def make_fe(api, weights, ranges, Hh=H, Ww=W, n=N_IMG, N=200, dev=True, **kw):
    fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=N, input_width=Ww, input_height=Hh, max_batch=n, precision=api.PREC_I8, **kw), dev=dev)
    fe.load_superpoint(weights)
    if ranges is not None:
        fe.set_int8_ranges(ranges)
    return fe


def read_tensors(api, weights, ranges):
    """one call of 8 images of 48 x 72 on a development handle of the mode; every layer's input and output as the GPU left them"""
    fe = make_fe(api, weights, ranges)
    fe.extract_batch(images(), cap=200)
    t = {name: fe.debug_read(name, (N_IMG, H // div, W // div, c)).copy() for name, (div, c) in SHAPES.items()}
    fe.close()
    return t


def check_layer(tensors, weights, ranges, layer):
    """asserts bit equality for every output of `layer`; returns the number of outputs compared"""
    _, src, dst, relu, pool = [l for l in LAYERS if l[0] == layer][0]
    wgt, bias = weights[layer]
    x, y = tensors[src], tensors[dst]
    for i in range(x.shape[0]):
        ref = O.layer(x[i], wgt, bias, ranges[O.INPUT_OF[layer]], relu, pool)
        bad = R.bits(y[i]) != R.bits(ref)
        assert ref.shape == y[i].shape and not bad.any(), "%s image %d: %d of %d outputs differ from the oracle in bits, first %s: %r != %r" % (
            layer, i, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), y[i][tuple(np.argwhere(bad)[0])], ref[tuple(np.argwhere(bad)[0])])
    assert np.abs(y).max() > 0      # the layer wrote something
    return int(y.size)


def main():
    from d2slam_amd import api, calibrate
    from d2slam_amd.weights import synthetic_superpoint_weights
    w = synthetic_superpoint_weights(dustbin_bias=7.5)
    ranges = calibrate.measure_ranges(w, images())
    t = read_tensors(api, w, ranges)
    for l in LAYERS:
        print("%s: %d outputs bit-equal" % (l[0], check_layer(t, w, ranges, l[0])), flush=True)
    print("I8_LAYERS_OK")


if __name__ == "__main__":
    sys.exit(main())
