"""Offline calibration of D2FE_PREC_I8 (include/d2fe.h): the per-tensor dynamic ranges FrontEnd.set_int8_ranges takes.

collect_ranges runs a calibration session of the product library (MinMax, Entropy or Percentile; statistics on the device).  measure_ranges is the "MinMax" calibrator: the largest |value| of every layer's output tensor over a set of images, read from an exact-mode (PREC_F32) handle of
the development library with the dense descriptor head through debug_read.  The reference calibrates offline as well (quadcam_tools/quantonnx.py:54-96 writes
the table its engine loads); a caller who has such a table passes its thresholds to set_int8_ranges instead."""
import numpy as np

from . import api

# debug_read name, channels and pool divisor of every layer's output; convPa | convDa share one buffer behind the dense head
_TENSORS = (("conv1a", 64, 1), ("conv1b", 64, 2), ("conv2a", 64, 2), ("conv2b", 64, 4), ("conv3a", 128, 4), ("conv3b", 128, 8), ("conv4a", 128, 8),
            ("conv4b", 128, 8), ("convPaDa", 512, 8), ("logits", 65, 8), ("desc_raw", 256, 8))
RANGE_FLOOR = 1e-30      # an all-zero tensor still needs a range the library accepts


def measure_ranges(weights, images, batch=8):
    """weights: {layer: (W, b)} as FrontEnd.load_superpoint takes them; images: u8 [n, H, W].  -> {layer name: range} for the twelve layers of api.SP_LAYERS."""
    images = np.ascontiguousarray(images, np.uint8)
    if images.ndim == 2:
        images = images[None]
    n, H, W = images.shape
    B = max(1, min(int(batch), n))
    fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=100, input_width=W, input_height=H, max_batch=B, precision=api.PREC_F32, dense_descriptors=True), dev=True)
    top = {}
    try:
        fe.load_superpoint(weights)
        for i0 in range(0, n, B):
            chunk = images[i0:i0 + B]
            fe.extract_batch(chunk, cap=100)
            for name, ch, div in _TENSORS:
                t = np.abs(fe.debug_read(name, (len(chunk), H // div, W // div, ch)))
                if name == "convPaDa":
                    top["convPa"] = max(top.get("convPa", 0.0), float(t[..., :256].max()))
                    top["convDa"] = max(top.get("convDa", 0.0), float(t[..., 256:].max()))
                else:
                    key = {"logits": "convPb", "desc_raw": "convDb"}.get(name, name)
                    top[key] = max(top.get(key, 0.0), float(t.max()))
    finally:
        fe.close()
    return {name: max(float(np.float32(top[name])), RANGE_FLOOR) for name in api.SP_LAYERS}


def collect_ranges(weights, images, method="entropy", param=None, n_bins=0, batch=8):
    """The ranges by an int8 calibration session of the product library (api.Int8Calibrator; include/d2fe.h, d2fe_calib_*): the statistics are collected on the
    device, two passes over `images` (the maxima, then the histograms; "minmax" needs the first alone), and turned into ranges by `method`: "minmax", "entropy" (the
    reference's calibrator, quadcam_tools/quantonnx.py:66-67,84-85) or "percentile" (param: the percentile, default 99.99).  n_bins 0: 2048.
    weights, images, batch and the result as for measure_ranges."""
    images = np.ascontiguousarray(images, np.uint8)
    if images.ndim == 2:
        images = images[None]
    n, H, W = images.shape
    B = max(1, min(int(batch), n))
    fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=100, input_width=W, input_height=H, max_batch=B, precision=api.PREC_F32, dense_descriptors=True))
    try:
        fe.load_superpoint(weights)
        cal = api.Int8Calibrator(fe, n_bins)
        cal.collect(images)
        if api.calib_method(method) != api.CALIB_METHODS["minmax"]:
            cal.freeze()
            cal.collect(images)
        return cal.ranges(method, param)
    finally:
        fe.close()
