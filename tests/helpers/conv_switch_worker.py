"""The whole network under ONE setting of the development library's conv schedule switches, in a process of its own: the library reads D2FE_CONV_PC,
D2FE_CONV64_TILE, D2FE_CONV1X1, D2FE_CONV1A_VALU and D2FE_FUSE1A from the environment once per process (tests/test_conv_layer_edges.py starts one child per
non-default value, one after the other; the pattern of tests/helpers/f16_layers.py).

On 8 images of 48 x 72 (partial 32- and 16-wide tiles, even extents at every pool, 288 conv1b tiles: the persistent loops wrap and the image strides matter):
  D2FE_PREC_F32    every layer, the logits and desc_raw equal the oracle bit for bit;
  D2FE_PREC_F16X2  the score map within 1e-5 and desc_raw within 1e-4 of the oracle (the tolerances of test_fast_mode_tolerances)."""
import sys

import numpy as np

N_IMG, H, W = 8, 48, 72
LAYERS = [("conv1a", 1, 64), ("conv1b", 2, 64), ("conv2a", 2, 64), ("conv2b", 4, 64), ("conv3a", 4, 128), ("conv3b", 8, 128), ("conv4a", 8, 128),
          ("conv4b", 8, 128)]


def oracle_layers(orc, img, w):
    x = orc.conv(orc.prep_u8(img)[:, :, None], *w["conv1a"], True)
    out = {"conv1a": x}
    for name, pool in (("conv1b", True), ("conv2a", False), ("conv2b", True), ("conv3a", False), ("conv3b", True), ("conv4a", False), ("conv4b", False)):
        x = orc.conv(x, *w[name], True)
        x = orc.maxpool2(x) if pool else x
        out[name] = x
    return out


def main():
    from d2slam_amd import api
    from d2slam_amd.synth import synth_image
    from d2slam_amd.weights import synthetic_superpoint_weights
    from oracle import oracle as orc
    orc.build()
    w = synthetic_superpoint_weights(dustbin_bias=7.5)
    imgs = np.stack([synth_image(H, W, 40 + s) for s in range(N_IMG)])
    full = [orc.superpoint_forward(imgs[i], w) for i in range(N_IMG)]
    for prec in (api.PREC_F32, api.PREC_F16X2):
        fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=200, input_width=W, input_height=H, max_batch=N_IMG, precision=prec, keep_score_map=True,
                                               dense_descriptors=True), dev=True)
        fe.load_superpoint(w)
        fe.extract_batch(imgs, cap=200)
        logits = fe.debug_read("logits", (N_IMG, H // 8, W // 8, 65)).copy()
        draw = fe.debug_read("desc_raw", (N_IMG, H // 8, W // 8, 256)).copy()
        semi = fe.debug_read("semi", (N_IMG, H, W)).copy()
        if prec == api.PREC_F32:
            acts = {name: fe.debug_read(name, (N_IMG, H // div, W // div, c)).copy() for name, div, c in LAYERS}
            for i in range(N_IMG):
                ref = oracle_layers(orc, imgs[i], w)
                for name, _, _ in LAYERS:
                    assert np.array_equal(acts[name][i].view(np.uint32), ref[name].view(np.uint32)), "%s image %d differs from the oracle" % (name, i)
                assert np.array_equal(logits[i].view(np.uint32), full[i]["logits"].view(np.uint32)), "logits image %d" % i
                assert np.array_equal(draw[i].view(np.uint32), full[i]["desc_raw"].view(np.uint32)), "desc_raw image %d" % i
            print("PREC_F32: every layer, the logits and desc_raw equal the oracle bit for bit", flush=True)
        else:
            e_semi = max(float(np.abs(semi[i] - full[i]["semi"]).max()) for i in range(N_IMG))
            e_desc = max(float(np.abs(draw[i] - full[i]["desc_raw"]).max()) for i in range(N_IMG))
            print("PREC_F16X2: largest score difference %.3g, desc_raw difference %.3g" % (e_semi, e_desc), flush=True)
            assert e_semi <= 1e-5 and e_desc <= 1e-4
        fe.close()
    print("CONV_SWITCH_OK")


if __name__ == "__main__":
    sys.exit(main())
