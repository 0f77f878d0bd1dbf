#!/usr/bin/env python3
"""Offline calibration for D2FE_PREC_I8: the twelve per-tensor dynamic ranges ("MinMax": the largest |value| of every layer's output over the images) as JSON, in
the form FrontEnd.set_int8_ranges and d2fe_set_superpoint_int8_ranges take (d2slam_amd/calibrate.py).  Run on the GPU:
  python tools/calibrate_i8.py --weights superpoint.npz --images frames.npy [--out int8_ranges.json]
--weights: .npz / .pth / .onnx as d2slam_amd/weights.py reads them (default: the seeded synthetic weights); --images: a .npy of u8 [n, H, W] (default: eight
synthetic 640x480 frames)."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--weights", default="")
    ap.add_argument("--images", default="")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    from d2slam_amd import calibrate, weights as wm
    from d2slam_amd.synth import synth_stereo
    loaders = {".npz": wm.load_superpoint_npz, ".pth": wm.load_superpoint_pth, ".onnx": wm.load_superpoint_onnx}
    w = loaders[os.path.splitext(args.weights)[1]](args.weights) if args.weights else wm.synthetic_superpoint_weights(dustbin_bias=7.5)
    imgs = np.load(args.images) if args.images else np.stack([f for s in range(4) for f in synth_stereo(480, 640, seed=900 + s)])
    ranges = calibrate.measure_ranges(w, imgs, args.batch)
    out = {"calibrator": "MinMax", "images": int(len(imgs)), "layers": list(wm.SP_LAYERS), "ranges": [ranges[n] for n in wm.SP_LAYERS]}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
