"""The per-layer check of D2FE_PREC_F16 shared by tests/test_f16_mode.py and its worker process: one call on a development handle, every layer's input and
output read back, each layer held to the float64 oracle (tests/helpers/f16_oracle.py) on the GPU's own input at the fp32 summation bound

    |y_gpu - y_ref| <= (K + 2) * 2^-24 * S,     K = 9 Cin (Cin for the 1x1 head),   S = sum |x^ w^| 2^-(SA+SW) + |bias|.

Run as a module (python -m tests.helpers.f16_layers) it checks every layer in THIS process -- the development library reads its schedule switches
(D2FE_CONV_PC: which kernel family takes which layer) from the environment once per process, so the other families need a process of their own."""
import sys

import numpy as np

from tests.helpers import f16_oracle as fo

# (layer, debug_read name of its input, of its output, ReLU, pool): the fused conv1a|conv1b; 64->64; 64->64 + pool; 64->128; 128->128 + pool; 128->128 (twice);
# 128->256; the 1x1 256->65
LAYERS = [("conv1b", "conv1a", "conv1b", True, True), ("conv2a", "conv1b", "conv2a", True, False), ("conv2b", "conv2a", "conv2b", True, True),
          ("conv3a", "conv2b", "conv3a", True, False), ("conv3b", "conv3a", "conv3b", True, True), ("conv4a", "conv3b", "conv4a", True, False),
          ("conv4b", "conv4a", "conv4b", True, False), ("convPa", "conv4b", "convPa", True, False), ("convPb", "convPa", "logits", False, False)]
SHAPES = {"conv1a": (1, 64), "conv1b": (2, 64), "conv2a": (2, 64), "conv2b": (4, 64), "conv3a": (4, 128), "conv3b": (8, 128), "conv4a": (8, 128),
          "conv4b": (8, 128), "convPa": (8, 256), "logits": (8, 65)}
N_IMG, H, W = 8, 48, 72      # partial 32- and 16-wide tiles, even extents at every pool, 288 conv1b tiles: the persistent loops wrap and the image strides matter


def read_tensors(api, weights):
    """one call of 8 images of 48 x 72 on a development handle of the mode; every layer's input and output as the GPU left them"""
    from d2slam_amd.synth import synth_image
    imgs = np.stack([synth_image(H, W, 40 + s) for s in range(N_IMG)])
    fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=200, input_width=W, input_height=H, max_batch=N_IMG, precision=api.PREC_F16), dev=True)
    fe.load_superpoint(weights)
    fe.extract_batch(imgs, cap=200)
    t = {name: fe.debug_read(name, (N_IMG, H // div, W // div, c)).copy() for name, (div, c) in SHAPES.items()}
    fe.close()
    return t


def check_layer(tensors, weights, layer):
    """asserts the bound for every output of `layer`; returns the largest error / bound"""
    _, src, dst, relu, pool = [l for l in LAYERS if l[0] == layer][0]
    wgt, bias = weights[layer]
    K = wgt.shape[1] * wgt.shape[2] * wgt.shape[3]
    x, y = tensors[src], tensors[dst]
    worst = 0.0
    for i in range(x.shape[0]):
        ref, S = fo.layer(x[i], wgt, bias, relu, pool)
        assert ref.shape == y[i].shape
        err = np.abs(y[i].astype(np.float64) - ref)
        bound = (K + 2) * 2.0 ** -24 * S
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        bad = np.argwhere(err > bound)
        assert len(bad) == 0, "%s image %d: %d outputs beyond the bound, first %s: |%g - %g| > %g" % (
            layer, i, len(bad), tuple(bad[0]), y[i][tuple(bad[0])], ref[tuple(bad[0])], bound[tuple(bad[0])])
    assert np.abs(y).max() > 0      # the layer wrote something
    return worst


def main():
    from d2slam_amd import api
    from d2slam_amd.weights import synthetic_superpoint_weights
    w = synthetic_superpoint_weights(dustbin_bias=7.5)
    t = read_tensors(api, w)
    for l in LAYERS:
        print("%s: largest error / bound = %.3g" % (l[0], check_layer(t, w, l[0])), flush=True)
    print("F16_LAYERS_OK")


if __name__ == "__main__":
    sys.exit(main())
