#!/usr/bin/env python3
"""Offline calibration for D2FE_PREC_I8: the twelve per-tensor dynamic ranges ("MinMax": the largest |value| of every layer's output over the images) as JSON, in
the form FrontEnd.set_int8_ranges and d2fe_set_superpoint_int8_ranges take (d2slam_amd/calibrate.py).  Run on the GPU:
  python tools/calibrate_i8.py --weights superpoint.npz --images frames.npy [--method entropy|percentile|minmax [--param 99.99]] [--out int8_ranges.json]
--method: the ranges by a calibration session of the product library (statistics on the device; d2fe_calib_* of include/d2fe.h), Entropy being the reference's
calibrator; without it the MinMax ranges of calibrate.measure_ranges, as before.
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
    ap.add_argument("--method", default="", choices=["", "minmax", "entropy", "percentile"],
                    help="a calibration session of the product library (calibrate.collect_ranges); without it: calibrate.measure_ranges, MinMax")
    ap.add_argument("--param", type=float, default=None, help="--method percentile: the percentile (default 99.99)")
    ap.add_argument("--bins", type=int, default=0, help="--method: histogram bins, 128 .. 4096 in multiples of 128 (default 2048)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    from d2slam_amd import calibrate, weights as wm
    from d2slam_amd.synth import synth_stereo
    loaders = {".npz": wm.load_superpoint_npz, ".pth": wm.load_superpoint_pth, ".onnx": wm.load_superpoint_onnx}
    w = loaders[os.path.splitext(args.weights)[1]](args.weights) if args.weights else wm.synthetic_superpoint_weights(dustbin_bias=7.5)
    imgs = np.load(args.images) if args.images else np.stack([f for s in range(4) for f in synth_stereo(480, 640, seed=900 + s)])
    if args.method:
        ranges = calibrate.collect_ranges(w, imgs, method=args.method, param=args.param, n_bins=args.bins, batch=args.batch)
    else:
        ranges = calibrate.measure_ranges(w, imgs, args.batch)
    names = {"": "MinMax", "minmax": "MinMax", "entropy": "Entropy", "percentile": "Percentile"}
    out = {"calibrator": names[args.method], "images": int(len(imgs)), "layers": list(wm.SP_LAYERS), "ranges": [ranges[n] for n in wm.SP_LAYERS]}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
