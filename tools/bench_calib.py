#!/usr/bin/env python3
"""The int8 calibration session (d2fe_calib_*, calibrate.collect_ranges) against the existing path (calibrate.measure_ranges) on the same 640x480 images, batch 8:
images per second of a whole two-pass entropy calibration (A) and of the MinMax read-back path (B), alternating rounds in one process, every round timed host to
host around the whole call -- handle, weight upload, passes, the ranges.  B is the yardstick: it exists without the session.  The JSON records both ranges
(min .. max over the rounds) and whether A's lies above B's; nothing is asserted.
  python tools/bench_calib.py [--images 16] [--rounds 5] [--out profiles/calib.json]
  rocprofv3 --kernel-trace --stats ... -- python tools/bench_calib.py --trace      (one two-pass session over 8 images and one stand-alone conv1a launch over two
                                                                                     of them, for a kernel trace; no alternation, no JSON file)
  python tools/bench_calib.py --kernel-stats <..._kernel_stats.csv> [--out ...]      (adds the per-image times of the statistics launches from such a trace to the JSON)"""
import argparse, csv, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, BATCH = 480, 640, 8
ALONE = 2      # images of the stand-alone conv1a launch of --trace: the hook's output buffer holds no more at this size
HBM_GBPS = 6290.0      # MI355X HBM3E as measured with a float4 copy (8000 is the specification); what the statistics launches must read is set against it


def images(n):
    import numpy as np
    from d2slam_amd.synth import synth_stereo
    return np.stack([f for s in range((n + 1) // 2) for f in synth_stereo(H, W, seed=900 + s)])[:n]


def stats_bytes_per_image():
    """bytes the statistics launches must read per image and phase: every tensor once, conv1a from the u8 frame"""
    from d2slam_amd import calibrate
    b = {"conv1a": H * W}
    for name, ch, div in calibrate._TENSORS[1:]:
        b[name] = (H // div) * (W // div) * ch * 4
    return b


def trace(n):
    import numpy as np
    from d2slam_amd import api, calibrate
    from d2slam_amd.weights import synthetic_superpoint_weights
    w, imgs = synthetic_superpoint_weights(dustbin_bias=7.5), images(n)
    calibrate.collect_ranges(w, imgs, "entropy", batch=BATCH)
    fe = api.DevFrontEnd(api.SuperPointConfig(input_width=W, input_height=H, max_batch=ALONE))
    fe.debug_conv1a(-1, imgs[:ALONE].reshape(-1), W, H * W, ALONE, H, W, w["conv1a"][0], w["conv1a"][1], np.zeros(ALONE * H * W * 64, np.float32))
    fe.close()


def kernel_stats(path, n):
    """per-image microseconds of the session's launches from a rocprofv3 kernel-stats CSV of --trace over n images (two passes: the range and the histogram phase)"""
    rows = {r["Name"]: r for r in csv.DictReader(open(path))}
    out = {}
    for name, r in rows.items():
        key = None
        if "calib_conv1a_stats_kernel<false>" in name: key = "conv1a_stats_range"
        elif "calib_conv1a_stats_kernel<true>" in name: key = "conv1a_stats_hist"
        elif "calib_stats_kernel<false" in name: key = "tensor_stats_range"
        elif "calib_stats_kernel<true" in name: key = "tensor_stats_hist"
        elif "conv1a_mfma_kernel" in name or "conv1a_kernel" in name: key = "launch_conv1a_alone"
        if key:
            per = ALONE if key == "launch_conv1a_alone" else n
            out[key + "_us_per_image"] = round(out.get(key + "_us_per_image", 0.0) + float(r["TotalDurationNs"]) / 1e3 / per, 2)
    total = sum(float(r["TotalDurationNs"]) for r in rows.values())
    calib = sum(float(r["TotalDurationNs"]) for nm, r in rows.items() if "calib_" in nm)
    alone = sum(float(r["TotalDurationNs"]) for nm, r in rows.items() if "conv1a_mfma_kernel" in nm or "d2fe::conv1a_kernel" in nm)
    out["statistics_share_of_session_kernel_time"] = round(calib / (total - alone), 4)
    b = stats_bytes_per_image()
    rest = sum(v for k, v in b.items() if k != "conv1a")
    out["tensor_stats_bytes_per_image"] = rest
    out["tensor_stats_us_per_image_at_hbm_rate"] = round(rest / (HBM_GBPS * 1e3), 2)
    out["hbm_gbps_measured_copy_rate"] = HBM_GBPS
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--kernel-stats", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "calib.json"))
    args = ap.parse_args()
    if args.trace:
        return trace(BATCH)
    rec = json.load(open(args.out)) if args.kernel_stats and os.path.exists(args.out) else {}
    if args.kernel_stats:
        rec["statistics_launches"] = kernel_stats(args.kernel_stats, BATCH)
    else:
        from d2slam_amd import calibrate
        from d2slam_amd.weights import synthetic_superpoint_weights
        w, imgs = synthetic_superpoint_weights(dustbin_bias=7.5), images(args.images)
        run = {"A": lambda: calibrate.collect_ranges(w, imgs, "entropy", batch=BATCH), "B": lambda: calibrate.measure_ranges(w, imgs, BATCH)}
        for f in run.values():      # warm-up: module loads, first allocations
            f()
        ips, last = {"A": [], "B": []}, {}
        for _ in range(args.rounds):
            for k in ("A", "B"):
                t0 = time.perf_counter()
                last[k] = run[k]()
                ips[k].append(round(len(imgs) / (time.perf_counter() - t0), 2))
        rec.update({"geometry": "%dx%d" % (W, H), "images": len(imgs), "batch": BATCH, "rounds": args.rounds,
                    "A": "calibrate.collect_ranges(method='entropy'): two passes of a calibration session, 2048 bins, statistics on the device",
                    "B": "calibrate.measure_ranges: one pass, every activation tensor read back through d2fe_debug_read (MinMax)",
                    "A_images_per_s": ips["A"], "B_images_per_s": ips["B"],
                    "A_min_max": [min(ips["A"]), max(ips["A"])], "B_min_max": [min(ips["B"]), max(ips["B"])],
                    "A_range_above_B_range": min(ips["A"]) > max(ips["B"]),
                    "entropy_ranges": last["A"], "minmax_ranges": last["B"],
                    "note": "host to host around the whole call (handle creation and weight upload included in both); seeded random weights, synthetic frames"})
    print(json.dumps(rec))
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
