#!/usr/bin/env python3
"""D2FE_PREC_I8 (int8 operands, int32 accumulation) against the exact mode over the 1056-image set of tools/mode_disagreement.py (d2slam_amd/parity_study.py,
i8_study): keypoints and matches in one mode only, list positions differing -- with D2FE_PREC_F16 beside it for scale.  The ranges are the MinMax ranges of the
first 64 images (d2slam_amd/calibrate.py); --calibrators adds the mode with the ranges of a calibration session (MinMax, Entropy, Percentile) over the same
images.  Figures to report, nothing is asserted.  Run on the GPU:
  python tools/i8_study.py [--calibrators minmax,entropy,percentile:99.99] [--out profiles/i8_study.json]
"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=496, help="synthetic stereo pairs (2 images each)")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--configs", default="0.015:200,0.015:100,0.15:100", help="threshold:max_keypoints, comma separated")
    ap.add_argument("--calibrators", default="", help='also with the ranges of a calibration session (calibrate.collect_ranges): names among minmax, entropy, '
                    'percentile[:p], comma separated, e.g. "minmax,entropy,percentile:99.99"')
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "i8_study.json"))
    args = ap.parse_args()
    from d2slam_amd import api, parity_study as ps
    t0 = time.time()
    imgs, pairs, n_syn = ps.frames(args.pairs)
    out = {"images": len(imgs), "synthetic_images": n_syn, "real_derived_images": len(imgs) - n_syn, "pairs": len(pairs), "geometry": "640x480", "configs": []}
    for cfg in args.configs.split(","):
        thr, N = cfg.split(":")
        rec = ps.i8_study(api, imgs, pairs, n_syn, float(thr), int(N), args.batch, calibrators=[c for c in args.calibrators.split(",") if c])
        out["configs"].append(rec)
        print("thr %s N %s: i8 %s positions %s" % (thr, N, rec["i8_vs_f32_all"], rec["i8_vs_f32_positions"]), file=sys.stderr, flush=True)
    out["seconds"] = round(time.time() - t0, 1)
    out["note"] = ("symmetric differences of raster-index sets (keypoints per image; matches per pair as (index, index) pairs) and list positions against the exact fp32 mode; "
                   "per-tensor MinMax ranges of the first 64 images; seeded random-init weights compress the score distribution, so an 8-bit network moves far more "
                   "keypoints across the top-K cut than it would with a trained network")
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
