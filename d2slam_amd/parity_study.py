"""Index-parity study of the arithmetic modes (host logic shared by tools/mode_disagreement.py -- the 1056-image run behind profiles/r04_mode_disagreement.json -- and
bench.py, which runs a 128-image subset of it inside every default run: `index_parity_in_run`).

Keypoint and match index sets of the Winograd fp32 mode (`value`) and of the fp16 hi/lo mode against the bitwise-exact direct-convolution fp32 mode on 640x480 frames:
synthetic stereo pairs plus frames derived from the three real crops of the reference's sample_data/fisheye.jpg that tests/golden/reference_headline.npz carries (flips,
mirror-padded re-crops, gain changes: real image statistics, no new reference content).  Pairs: synthetic L<->R, real frame <-> the frame shifted by (3, 5) px.
Symmetric differences of raster-index sets (keypoints per image; matches per pair as (index, index) pairs).

order_study(): the ORDER-aware comparison (list positions, not sets) of the plain Winograd mode and of the Winograd mode with exact_order against the exact mode,
the deviation of the Winograd score maps from the direct ones (what exact_order_eps has to bound) and what exact_order re-evaluates.

f16_study(): the fp16-operand mode (PREC_F16) against the exact mode -- sets, matches and list positions (tools/f16_study.py, profiles/f16_study.json).  study() is
unchanged by it: bench.py's in-run subset compares what it always compared.

i8_study(): the int8-operand mode (PREC_I8, ranges from calibrate.measure_ranges on the first 64 images) against the exact mode, the same figures, with PREC_F16 beside it
for scale (tools/i8_study.py, profiles/i8_study.json)."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 480, 640


def real_frames():
    z = np.load(os.path.join(ROOT, "tests", "golden", "reference_headline.npz"))
    d435, quad, tum = z["img_d435"], z["img_quad"], z["img_tum"]
    out = []
    for g in (1.0, 0.8, 1.25):
        base = np.clip(np.rint(d435.astype(np.float32) * g), 0, 255).astype(np.uint8)
        out += [base, base[:, ::-1].copy(), base[::-1].copy(), base[::-1, ::-1].copy()]
    q = np.pad(quad, ((40, 40), (0, 0)), mode="reflect")                      # 480 x 800
    for x0 in (0, 40, 80, 120, 160):
        out += [q[:, x0:x0 + W].copy(), q[::-1, x0:x0 + W].copy()]
    t = np.pad(tum, ((0, 0), (64, 64)), mode="reflect")                       # 512 x 640
    for y0 in (0, 8, 16, 24, 32):
        out += [t[y0:y0 + H].copy(), t[y0:y0 + H, ::-1].copy()]
    return out


def frames(n_synthetic_pairs, n_real=None, seed0=5000):
    """(images [NI,H,W] u8, pairs [(ia, ib)], number of synthetic images)"""
    from d2slam_amd.synth import synth_stereo
    imgs, pairs = [], []
    for s in range(n_synthetic_pairs):
        l, r = synth_stereo(H, W, seed=seed0 + s)
        pairs.append((len(imgs), len(imgs) + 1)); imgs += [l, r]
    n_syn = len(imgs)
    real = real_frames()
    for f in (real if n_real is None else real[:n_real]):
        pairs.append((len(imgs), len(imgs) + 1)); imgs += [f, np.roll(f, (3, 5), (0, 1))]
    return np.ascontiguousarray(np.stack(imgs)), pairs, n_syn


def weights_for(thr):
    """the seeded weights with a dustbin bias that leaves enough candidates above `thr` (0.15: as bench.py's quadcam leg)"""
    from d2slam_amd.weights import synthetic_superpoint_weights
    w = synthetic_superpoint_weights(dustbin_bias=7.5)
    if thr >= 0.1:
        Wt, b = w["convPb"]; b = b.copy(); b[64] -= np.float32(3.5); w["convPb"] = (Wt, b)
    return w


def select(api, imgs, pairs, thr, N, prec, batch=32, device_id=0):
    """(per-image raster-index sets, per-pair sets of (index, index) matches) of one arithmetic mode"""
    fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=N, input_width=W, input_height=H, max_batch=batch, precision=prec, keypoint_threshold=thr, device_id=device_id))
    fe.load_superpoint(weights_for(thr))
    kp, ds = [], []
    for i0 in range(0, len(imgs), batch):
        for k, s, d in fe.extract_batch(imgs[i0:i0 + batch], cap=N):
            kp.append(k); ds.append(d)
    mt = []
    for ia, ib in pairs:
        q, t, _ = fe.match_knn(ds[ia], ds[ib], 0.8)
        ra = (kp[ia][:, 1].astype(np.int64) * W + kp[ia][:, 0].astype(np.int64)); rb = (kp[ib][:, 1].astype(np.int64) * W + kp[ib][:, 0].astype(np.int64))
        mt.append(set(zip(ra[q].tolist(), rb[t].tolist())))
    fe.close()
    return [set((k[:, 1].astype(np.int64) * W + k[:, 0].astype(np.int64)).tolist()) for k in kp], mt


def compare(ref, other, lo, hi, plo, phi):
    kt = sum(len(ref[0][i]) for i in range(lo, hi)); kd = sum(len(ref[0][i] ^ other[0][i]) for i in range(lo, hi))
    ki = sum(1 for i in range(lo, hi) if ref[0][i] ^ other[0][i])
    mtot = sum(len(ref[1][p]) for p in range(plo, phi)); md = sum(len(ref[1][p] ^ other[1][p]) for p in range(plo, phi))
    return {"keypoints": kt, "keypoints_in_one_mode_only": kd, "per_1e4_keypoints": round(1e4 * kd / max(kt, 1), 3), "images_with_a_difference": ki,
            "matches": mtot, "matches_in_one_mode_only": md, "per_1e4_matches": round(1e4 * md / max(mtot, 1), 3)}


def study(api, imgs, pairs, n_syn, thr, N, batch=32, device_id=0):
    """one configuration: both fast modes against the exact mode, over all / synthetic / real-derived frames"""
    modes = {"f32": api.PREC_F32, "wino": api.PREC_F32_WINO, "f16x2": api.PREC_F16X2}
    sel = {name: select(api, imgs, pairs, thr, N, prec, batch, device_id) for name, prec in modes.items()}
    NI = len(imgs)
    rec = {"threshold": thr, "max_keypoints": N}
    for name in ("wino", "f16x2"):
        for part, lo, hi in (("all", 0, NI), ("synthetic", 0, n_syn), ("real_derived", n_syn, NI)):
            plo, phi = (0, len(pairs)) if part == "all" else ((0, n_syn // 2) if part == "synthetic" else (n_syn // 2, len(pairs)))
            rec["%s_vs_f32_%s" % (name, part)] = compare(sel["f32"], sel[name], lo, hi, plo, phi)
    return rec


def _lists_and_matches(api, imgs, pairs, thr, N, prec, batch=32, device_id=0, ranges=None):
    """(per-image raster-index lists in list order, per-pair sets of (index, index) matches) of one arithmetic mode; ranges: PREC_I8's calibration ranges"""
    fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=N, input_width=W, input_height=H, max_batch=batch, precision=prec, keypoint_threshold=thr, device_id=device_id))
    fe.load_superpoint(weights_for(thr))
    if ranges is not None:
        fe.set_int8_ranges(ranges)
    idx, ds = [], []
    for i0 in range(0, len(imgs), batch):
        for k, s, d in fe.extract_batch(imgs[i0:i0 + batch], cap=N):
            idx.append(k[:, 1].astype(np.int64) * W + k[:, 0].astype(np.int64)); ds.append(d)
    mt = []
    for ia, ib in pairs:
        q, t, _ = fe.match_knn(ds[ia], ds[ib], 0.8)
        mt.append(set(zip(idx[ia][q].tolist(), idx[ib][t].tolist())))
    fe.close()
    return idx, mt


def f16_study(api, imgs, pairs, n_syn, thr, N, batch=32, device_id=0):
    """one configuration: the fp16-operand mode (PREC_F16) -- and, for scale, the two other fast modes -- against the exact mode: keypoint SETS and match sets
    (compare) and list POSITIONS (compare_order).  Figures to report, not bounds: fp16 operands carry 11 bits, near-ties far beyond the top-K cut move."""
    modes = {"f32": api.PREC_F32, "f16": api.PREC_F16, "f16x2": api.PREC_F16X2, "wino": api.PREC_F32_WINO}
    got = {name: _lists_and_matches(api, imgs, pairs, thr, N, prec, batch, device_id) for name, prec in modes.items()}
    as_sets = lambda g: ([set(a.tolist()) for a in g[0]], g[1])
    NI = len(imgs)
    rec = {"threshold": thr, "max_keypoints": N, "images": NI, "images_per_call": batch}
    for name in ("f16", "f16x2", "wino"):
        for part, lo, hi in (("all", 0, NI), ("synthetic", 0, n_syn), ("real_derived", n_syn, NI)):
            plo, phi = (0, len(pairs)) if part == "all" else ((0, n_syn // 2) if part == "synthetic" else (n_syn // 2, len(pairs)))
            rec["%s_vs_f32_%s" % (name, part)] = compare(as_sets(got["f32"]), as_sets(got[name]), lo, hi, plo, phi)
        order = compare_order(got["f32"][0], got[name][0])
        order["images_differing"] = len(order["images_differing"])
        rec["%s_vs_f32_positions" % name] = order
    return rec


def i8_study(api, imgs, pairs, n_syn, thr, N, batch=32, device_id=0, calib_images=64, calibrators=None):
    """one configuration: the int8-operand mode (PREC_I8) -- and, for scale, the fp16-operand mode -- against the exact mode: keypoint SETS and match sets (compare)
    and list POSITIONS (compare_order).  The ranges are the MinMax ranges of the first `calib_images` images.  Figures to report, not bounds: an 8-bit network on
    seeded random weights moves far more near-ties than fp16's 11 bits do.
    calibrators: names among "minmax", "entropy", "percentile" or "percentile:<p>" -- the int8 mode once more per name with the ranges of a calibration session over
    the same images (calibrate.collect_ranges); the record gains "i8_<name>_vs_f32_*" and "ranges_<name>"."""
    from d2slam_amd import calibrate
    ranges = calibrate.measure_ranges(weights_for(thr), imgs[:calib_images])
    modes = {"f32": (api.PREC_F32, None), "i8": (api.PREC_I8, ranges), "f16": (api.PREC_F16, None)}
    session = {}
    for cal in calibrators or ():
        method, _, p = cal.partition(":")
        session[cal] = calibrate.collect_ranges(weights_for(thr), imgs[:calib_images], method=method, param=float(p) if p else None, batch=min(batch, 8))
        modes["i8_" + cal] = (api.PREC_I8, session[cal])
    got = {name: _lists_and_matches(api, imgs, pairs, thr, N, prec, batch, device_id, r) for name, (prec, r) in modes.items()}
    as_sets = lambda g: ([set(a.tolist()) for a in g[0]], g[1])
    NI = len(imgs)
    rec = {"threshold": thr, "max_keypoints": N, "images": NI, "images_per_call": batch, "calibration_images": min(calib_images, NI), "ranges": ranges}
    for cal, r in session.items():
        rec["ranges_" + cal] = r
    for name in [m for m in modes if m != "f32"]:
        for part, lo, hi in (("all", 0, NI), ("synthetic", 0, n_syn), ("real_derived", n_syn, NI)):
            plo, phi = (0, len(pairs)) if part == "all" else ((0, n_syn // 2) if part == "synthetic" else (n_syn // 2, len(pairs)))
            rec["%s_vs_f32_%s" % (name, part)] = compare(as_sets(got["f32"]), as_sets(got[name]), lo, hi, plo, phi)
        order = compare_order(got["f32"][0], got[name][0])
        order["images_differing"] = len(order["images_differing"])
        rec["%s_vs_f32_positions" % name] = order
    return rec


def _lists_and_maps(api, imgs, thr, N, prec, batch, device_id=0, maps=True, **eo):
    """per-image raster-index LISTS (in list order) of one mode and, with maps, its dense score maps [NI, H, W] (development library: keep_score_map + debug_read)"""
    fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=N, input_width=W, input_height=H, max_batch=batch, precision=prec, keypoint_threshold=thr, device_id=device_id,
                                           keep_score_map=maps), dev=maps, **eo)
    fe.load_superpoint(weights_for(thr))
    lists, semi = [], []
    for i0 in range(0, len(imgs), batch):
        chunk = imgs[i0:i0 + batch]
        for k, s, d in fe.extract_batch(chunk, cap=N):
            lists.append(k[:, 1].astype(np.int64) * W + k[:, 0].astype(np.int64))
        if maps:
            semi.append(fe.debug_read("semi", (batch, H, W))[:len(chunk)].copy())
    stats = fe.exact_order_stats()
    fe.close()
    return lists, (np.concatenate(semi) if maps else None), stats


def compare_order(ref, other):
    """position-by-position comparison of per-image index lists against the reference mode's"""
    pos = imgs_order = imgs_set = 0
    differing = []
    for i, (a, b) in enumerate(zip(ref, other)):
        if len(a) == len(b) and np.array_equal(a, b):
            continue
        differing.append(i)
        if set(a.tolist()) != set(b.tolist()):
            imgs_set += 1
        else:
            imgs_order += 1
        m = min(len(a), len(b))
        pos += int((a[:m] != b[:m]).sum()) + abs(len(a) - len(b))
    return {"keypoints": int(sum(len(a) for a in ref)), "positions_differing": pos, "images_with_an_order_difference_only": imgs_order,
            "images_with_a_set_difference": imgs_set, "images_differing": differing}


def order_study(api, imgs, thr, N, batch=32, device_id=0, eps=0.0, crops=0):
    """one configuration on the GPU.  The reference of every figure is the exact mode (PREC_F32)."""
    from d2slam_amd import exact_order as eo
    l_d, s_d, _ = _lists_and_maps(api, imgs, thr, N, api.PREC_F32, batch, device_id)
    l_w, s_w, _ = _lists_and_maps(api, imgs, thr, N, api.PREC_F32_WINO, batch, device_id)
    l_x, _, st = _lists_and_maps(api, imgs, thr, N, api.PREC_F32_WINO, batch, device_id, maps=False, exact_order=True, exact_order_eps=eps, exact_order_crops=crops)
    strong = s_d > np.float32(thr / 2)
    dev = np.abs(s_w - s_d)
    eps_used = eps if eps > 0 else eo.DEFAULT_EPS
    marked, cells, per_call = [], [], []
    for i in range(len(imgs)):
        _, _, m, c = eo.mark(s_w[i], thr, 1, N, eps_used)
        marked.append(int(m.sum())); cells.append(len(c))
    for i0 in range(0, len(imgs), batch):
        per_call.append(sum(cells[i0:i0 + batch]))
    return {"threshold": thr, "max_keypoints": N, "images": len(imgs), "images_per_call": batch,
            "score_deviation_max_where_direct_above_half_threshold": float(dev[strong].max()), "score_deviation_max_all_pixels": float(dev.max()),
            "exact_order_eps": eps_used, "exact_order_crops": crops if crops > 0 else "default",
            "wino_vs_f32": compare_order(l_d, l_w), "exact_order_vs_f32": compare_order(l_d, l_x),
            "host_rule": {"marked_per_image_mean": float(np.mean(marked)), "marked_per_image_max": int(max(marked)), "cells_per_image_mean": float(np.mean(cells)),
                          "cells_per_image_max": int(max(cells)), "cells_per_call_max": int(max(per_call))},
            "device_stats": st}
