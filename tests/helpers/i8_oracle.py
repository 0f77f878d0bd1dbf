"""D2FE_PREC_I8 restated in numpy (the contract at the enum in include/d2fe.h): float32 for r, s_x, s_w, d_c, x * r and the two epilogue roundings, float64
for q_w, int64 for the sum.  An int8 x int8 product summed in integers is exact and order-free, so a layer has ONE correct answer and the device is held to it
bit for bit.  Never another mode of the library and never the mode itself."""
import numpy as np

F32 = np.float32
QMAX = 127
# the plan's layers (csrc/sp_plan.h) and, per quantised layer, the tensor it reads
SP_LAYERS = ("conv1a", "conv1b", "conv2a", "conv2b", "conv3a", "conv3b", "conv4a", "conv4b", "convPa", "convPb", "convDa", "convDb")
INPUT_OF = {"conv1b": "conv1a", "conv2a": "conv1b", "conv2b": "conv2a", "conv3a": "conv2b", "conv3b": "conv3a", "conv4a": "conv3b", "conv4b": "conv4a",
            "convPa": "conv4b", "convPb": "convPa", "convDa": "conv4b", "convDb": "convDa"}
# the detector path behind conv1a: (layer, ReLU, pool)
CHAIN = (("conv1b", True, True), ("conv2a", True, False), ("conv2b", True, True), ("conv3a", True, False), ("conv3b", True, True), ("conv4a", True, False),
         ("conv4b", True, False), ("convPa", True, False), ("convPb", False, False))


def input_scales(T):
    """(r, s_x) = (fl32(127 / T), fl32(T / 127))"""
    T = F32(T)
    return F32(QMAX) / T, T / F32(QMAX)


def quant_weights(w):
    """(q_w int64 [cout, cin, k, k], s_w float32 [cout]): per output channel, round half to even in float64; an all-zero channel: q = 0, s_w = 1"""
    w = np.asarray(w, F32)
    amax = np.abs(w).reshape(w.shape[0], -1).max(axis=1)
    live = amax > 0
    safe = np.where(live, amax, F32(1)).astype(np.float64)
    q = np.clip(np.rint(w.astype(np.float64) * 127.0 / safe[:, None, None, None]), -QMAX, QMAX)
    q[~live] = 0
    s_w = np.where(live, amax / F32(QMAX), F32(1)).astype(F32)
    return q.astype(np.int64), s_w


def quant_act(x, r):
    """q_x = rint(min(max(fl32(x * r), -127), 127)): int64.  +inf -> 127"""
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.asarray(x, F32) * F32(r)
    assert v.dtype == F32
    return np.rint(np.minimum(np.maximum(v, F32(-QMAX)), F32(QMAX))).astype(np.int64)


def isum(qx, qw):
    """sum over (ky, kx, ci) of qx[y + ky - p, x + kx - p, ci] * qw[co, ci, ky, kx], zero padding: int64 [H, W, cout]"""
    H, W, C = qx.shape
    co, ci, k, _ = qw.shape
    assert ci == C and qx.dtype == np.int64 and qw.dtype == np.int64
    p = k // 2
    xp = np.zeros((H + 2 * p, W + 2 * p, C), np.int64)
    xp[p:p + H, p:p + W] = qx
    acc = np.zeros((H * W, co), np.int64)
    for ky in range(k):
        for kx in range(k):
            acc += xp[ky:ky + H, kx:kx + W].reshape(H * W, C) @ np.ascontiguousarray(qw[:, :, ky, kx].T)
    return acc.reshape(H, W, co)


def epilogue(acc, d, b):
    """fl32(fl32((float)acc * d_c) + bias_c): two float32 roundings"""
    a = acc.astype(F32)                      # int64 -> float32 rounds to nearest even
    with np.errstate(under="ignore"):
        t = a * np.asarray(d, F32)
    y = t + np.asarray(b, F32)
    assert a.dtype == F32 and t.dtype == F32 and y.dtype == F32
    return y


def finish(y, relu, pool, anchor_end=False):
    """ReLU as the kernels write it (v > 0 ? v : +0), then the 2x2 max-pool with floor.  anchor_end (a MUTANT): windows anchored at the far end"""
    if relu:
        y = np.where(y > 0, y, F32(0))
    if pool:
        H, W = y.shape[:2]
        Ho, Wo = H // 2, W // 2
        oy, ox = (H - 2 * Ho, W - 2 * Wo) if anchor_end else (0, 0)
        y = y[oy:oy + 2 * Ho, ox:ox + 2 * Wo].reshape(Ho, 2, Wo, 2, -1).max(axis=(1, 3))
    return np.ascontiguousarray(y, F32)


def layer(x, w, b, T, relu, pool):
    """one quantised layer on one image: x [H, W, cin] fp32 (the layer's input, range T), w [cout, cin, k, k], b [cout] -> fp32 [H', W', cout]"""
    r, s_x = input_scales(T)
    qw, s_w = quant_weights(w)
    d = s_x * s_w
    assert d.dtype == F32
    return finish(epilogue(isum(quant_act(x, r), qw), d, b), relu, pool)


def chain(c1a, weights, ranges, last="convPb"):
    """conv1b .. `last` of the detector path on conv1a's output [H, W, 64]; ranges: {layer: range of its output}.  -> {layer: output}"""
    out, x = {}, c1a
    src = "conv1a"
    for name, relu, pool in CHAIN:
        x = layer(x, *weights[name], ranges[src], relu, pool)
        out[name] = x
        src = name
        if name == last:
            break
    return out
