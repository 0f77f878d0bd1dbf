"""numpy restatement of ONE layer of D2FE_PREC_F16 (include/d2fe.h, d2fe_precision): fp16 operands, real-number products and sum, fp32 bias.

    x^ = fp16(clamp(x * 2^SA, +-65000))      w^ = fp16(clamp(w * 2^SW, +-65000))      round to nearest even, fp16 subnormals KEPT (numpy's
    float16 conversion underflows gradually, as the device's conversion and matrix instruction do)
    y  = sum over (ky, kx, ci) of x^ w^ * 2^-(SA+SW) + bias,  then ReLU, then the 2x2 max-pool (floor)

The products of two fp16 numbers are exact in float64 and so, to ~1e-16 relative, is their sum: `layer` is the real-number value of the contract on
the ROUNDED operands, the thing the fp32 summation bound of the library is stated against.  It also returns
    S = sum |x^ w^| * 2^-(SA+SW) + |bias|
per output (pooled outputs: the largest S of the four, ReLU and max being 1-Lipschitz).  accumulate=np.float32 takes the same sum in fp32
(operands still exact; the order is the BLAS's): two chains that differ in nothing but the accumulation."""
import numpy as np

SA, SW = 4, 8
CLAMP = 65000.0


def round_operand(v, shift):
    """fp16(clamp(v * 2^shift, +-65000)), round to nearest even; returned as float16"""
    with np.errstate(over="ignore"):
        s = np.asarray(v, np.float32) * np.float32(2.0 ** shift)      # a power of two: exact in fp32 (an overflow to infinity meets the clamp)
    return np.clip(s, np.float32(-CLAMP), np.float32(CLAMP)).astype(np.float16)


def layer(x, wgt, bias, relu, pool, accumulate=np.float64):
    """x [H, W, Cin] fp32, wgt [Cout, Cin, k, k], bias [Cout] -> (y, S), both [H', W', Cout] float64 (accumulate=float32: y is what fp32 sums give)"""
    x = np.asarray(x, np.float32); wgt = np.asarray(wgt, np.float32); bias = np.asarray(bias, np.float32)
    H, W, cin = x.shape
    cout, cin2, k, _ = wgt.shape
    assert cin == cin2 and k in (1, 3)
    p = k // 2
    xh = np.zeros((H + 2 * p, W + 2 * p, cin), accumulate)
    xh[p:p + H, p:p + W] = round_operand(x, SA).astype(accumulate)
    wh = round_operand(wgt, SW).astype(accumulate)
    acc = np.zeros((H * W, cout), accumulate)
    S = np.zeros((H * W, cout), np.float64)
    for ky in range(k):
        for kx in range(k):
            a = xh[ky:ky + H, kx:kx + W].reshape(H * W, cin)
            b = np.ascontiguousarray(wh[:, :, ky, kx].T)
            acc += a @ b
            S += np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64)
    inv = accumulate(2.0 ** -(SA + SW))
    y = (acc * inv + bias.astype(accumulate)[None, :]).reshape(H, W, cout)
    S = (S * 2.0 ** -(SA + SW) + np.abs(bias.astype(np.float64))[None, :]).reshape(H, W, cout)
    if relu:
        y = np.maximum(y, 0)
    if pool:
        Ho, Wo = H // 2, W // 2
        y = y[:2 * Ho, :2 * Wo].reshape(Ho, 2, Wo, 2, cout).max(axis=(1, 3))
        S = S[:2 * Ho, :2 * Wo].reshape(Ho, 2, Wo, 2, cout).max(axis=(1, 3))
    return y.astype(np.float64), S


# the layers D2FE_PREC_F16 evaluates with fp16 operands on the detector path, in order: (name, relu, pool); conv1a in front of them is exact fp32
CHAIN = [("conv1b", True, True), ("conv2a", True, False), ("conv2b", True, True), ("conv3a", True, False), ("conv3b", True, True),
         ("conv4a", True, False), ("conv4b", True, False), ("convPa", True, False), ("convPb", False, False)]


def chain_logits(conv1a, weights, accumulate=np.float64):
    """the detector path from the exact conv1a activation [H, W, 64] to the logits [H/8, W/8, 65]; every layer's output is stored as fp32, as on the device.
    Also returns the trunk (conv4b) as fp32."""
    x = np.asarray(conv1a, np.float32)
    trunk = None
    for name, relu, pool in CHAIN:
        y, _ = layer(x, weights[name][0], weights[name][1], relu, pool, accumulate)
        x = y.astype(np.float32)
        if name == "conv4b":
            trunk = x
    return x, trunk
