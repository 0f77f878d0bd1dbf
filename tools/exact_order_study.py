#!/usr/bin/env python3
"""Order-aware index parity of the Winograd mode, plain and with exact_order, against the exact mode over the 1056-image set of tools/mode_disagreement.py
(d2slam_amd/parity_study.py, order_study): list positions differing, images listed in another order, the deviation of the Winograd score maps from the direct
ones (the measurement behind the default exact_order_eps) and what exact_order marks, re-evaluates and drops.  Run on the GPU:
  python tools/exact_order_study.py > profiles/exact_order_study.json
"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=496, help="synthetic stereo pairs (2 images each)")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--eps", type=float, default=0.0, help="exact_order_eps (0: the library default)")
    ap.add_argument("--crops", type=int, default=0, help="exact_order_crops (0: the library default, one per image of a call)")
    ap.add_argument("--configs", default="0.015:200,0.015:100,0.15:200", help="threshold:max_keypoints, comma separated")
    args = ap.parse_args()
    from d2slam_amd import api, parity_study as ps
    t0 = time.time()
    imgs, pairs, n_syn = ps.frames(args.pairs)
    out = {"images": len(imgs), "synthetic_images": n_syn, "geometry": "640x480", "configs": []}
    for cfg in args.configs.split(","):
        thr, N = cfg.split(":")
        rec = ps.order_study(api, imgs, float(thr), int(N), args.batch, eps=args.eps, crops=args.crops)
        out["configs"].append(rec)
        brief = {k: v for k, v in rec.items() if k not in ("wino_vs_f32", "exact_order_vs_f32")}
        for k in ("wino_vs_f32", "exact_order_vs_f32"):
            brief[k] = {a: b for a, b in rec[k].items() if a != "images_differing"}
        print(json.dumps(brief), file=sys.stderr, flush=True)
    out["seconds"] = round(time.time() - t0, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
