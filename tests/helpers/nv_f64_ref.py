"""Float64 reference of the NetVLAD layers and head (numpy only) with a derived fp32 error bound for every output, for tests/test_netvlad_shapes*.py.

Error model (the one of tests/helpers/f16_layers.py::check_layer): a sum of K terms formed in fp32 in ANY order differs from the exact sum by at most

    (K + 2) * 2^-24 * S,        S = the sum of the absolute values of the terms.

Every function returns the value and, elementwise, the quantities the bound needs.  A fused block is held to the reference as a whole, on the GPU's own input
to that block (chain()): ReLU / ReLU6 are 1-Lipschitz and pass an error through unchanged, a linear stage maps an input error e to |W| e, zero padding is exact,
and the last stage counts one more term per partial slab its output or its residual is summed from.  S of a later stage is formed from |input| + its error,
so the bound also holds for the values the GPU actually multiplied.

The head's bound follows the formulation of the kernel that ran: nv_vlad_mfma_kernel forms c S - P (S = sum_p a, P = sum_p a x), the general kernel
sum_p a (c - x); both divide by the cluster norm and the global norm (floored at 1e-12), and so does the bound."""
import numpy as np

U = 2.0 ** -24
ACT_NONE, ACT_RELU, ACT_RELU6 = 0, 1, 2


def same_out(n, s):
    return (n + s - 1) // s


def same_pad_begin(n, s, out):
    """TF "SAME", 3x3"""
    return max(0, (out - 1) * s + 3 - n) // 2


def act(z, a, no_hi=False):
    if a == ACT_NONE:
        return z
    z = np.maximum(z, 0.0)
    return z if (a == ACT_RELU or no_hi) else np.minimum(z, 6.0)


def _taps(x, stride):
    """x [H, W, C] -> the nine zero-padded tap views [Ho, Wo, C] of a 3x3 SAME window, in (ky, kx) order"""
    H, W, C = x.shape
    Ho, Wo = same_out(H, stride), same_out(W, stride)
    pt, pl = same_pad_begin(H, stride, Ho), same_pad_begin(W, stride, Wo)
    xp = np.zeros(((Ho - 1) * stride + 3 + pt, (Wo - 1) * stride + 3 + pl, C), np.float64)
    xp[pt:pt + H, pl:pl + W] = x
    return [xp[ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride] for ky in range(3) for kx in range(3)]


def conv0(img_u8, w, b, stride):
    """3x3 from the u8 frame, input (x - 128) / 128 (exact in fp32).  w [cout, 1, 3, 3].  -> (z, S, E = 0, K = 9)"""
    x = ((img_u8.astype(np.float64) - 128.0) / 128.0)[:, :, None]
    w9 = np.asarray(w, np.float64).reshape(-1, 9)
    t = _taps(x, stride)
    z = sum(t[k] * w9[:, k] for k in range(9)) + np.asarray(b, np.float64)
    S = sum(np.abs(t[k]) * np.abs(w9[:, k]) for k in range(9)) + np.abs(np.asarray(b, np.float64))
    return z, S, np.zeros_like(z), 9


def dw(x, e, w, b, stride, wrong_tap_lastcol=False):
    """depthwise 3x3.  w [C, 3, 3]; e: error bound of x (array or 0).  -> (z, S, E, K = 9)"""
    w9 = np.asarray(w, np.float64).reshape(-1, 9)
    t = _taps(x, stride)
    if wrong_tap_lastcol:      # mutant: the (., +1) taps of the LAST output column read the centre column
        t = [v.copy() for v in t]
        for ky in range(3):
            t[ky * 3 + 2][:, -1] = t[ky * 3 + 1][:, -1]
    te = _taps(np.abs(x) + e, stride)
    ee = _taps(np.zeros_like(x) + e, stride)
    z = sum(t[k] * w9[:, k] for k in range(9)) + np.asarray(b, np.float64)
    S = sum(te[k] * np.abs(w9[:, k]) for k in range(9)) + np.abs(np.asarray(b, np.float64))
    E = sum(ee[k] * np.abs(w9[:, k]) for k in range(9))
    return z, S, E, 9


def pw(x, e, w, b, skip_hidden=None, skip_bias=None, only_hidden=None):
    """1x1.  w [cout, cin].  -> (z, S, E, K = cin).  The keyword arguments are the mutants of the comparator test: one input channel left out of the sums of
    output channels skip_hidden[1] (a 16-channel tile), one bias omitted, only the input channels `only_hidden` summed."""
    w = np.asarray(w, np.float64)
    bb = np.asarray(b, np.float64).copy()
    wz = w
    if skip_hidden is not None:
        wz = w.copy(); wz[skip_hidden[1], skip_hidden[0]] = 0.0
    if only_hidden is not None:
        wz = np.zeros_like(w); wz[:, only_hidden] = w[:, only_hidden]
    if skip_bias is not None:
        bb[skip_bias] = 0.0
    z = x @ wz.T + bb
    S = (np.abs(x) + e) @ np.abs(w).T + np.abs(np.asarray(b, np.float64))
    E = (np.zeros_like(x) + e) @ np.abs(w).T
    return z, S, E, w.shape[1]


def chain(layers, x, e_x=0.0, res=None, res_S=None, res_e=0.0, res_terms=1, out_terms=1, mut=None):
    """One plan step -- one layer, or a fused run of up to three -- on its input x: the u8 frame [H, W] for a step that begins with the first conv, else the
    fp64 tensor [H, W, C] with elementwise error bound e_x.  res: the tensor added to the last layer's output (res_S >= the sum of the absolute values of the
    res_terms partial slabs it is summed from, res_e its own error); out_terms: partial slabs the output is summed from.
    Returns dict(y, bound, S, pre): pre[i] = what enters layer i's activation (the clamp-share test reads it).  mut: see the comparator test."""
    mut = mut or {}
    cur, e = x, e_x
    pre = []
    for i, l in enumerate(layers):
        last = i == len(layers) - 1
        if l["kind"] == "conv":
            z, S, E, K = conv0(cur, l["weight"], l["bias"], l["stride"])
        elif l["kind"] == "dw":
            z, S, E, K = dw(cur, e, l["weight"], l["bias"], l["stride"], wrong_tap_lastcol=bool(mut.get("dw_wrong_tap")))
        else:
            kw = {k: mut[k] for k in ("skip_hidden", "skip_bias", "only_hidden") if k in mut} if last else {}
            z, S, E, K = pw(cur, e, l["weight"], l["bias"], **kw)
        K += 1                                           # the bias
        if last:
            K += out_terms
            if res is not None:
                z = z + res
                S = S + (np.abs(res) if res_S is None else np.maximum(res_S, np.abs(res)))
                E = E + res_e
                K += res_terms
        pre.append(z)
        cur = act(z, l["act"], no_hi=bool(mut.get("no_hi_clamp")) and i == 0)
        e = (K + 2) * U * S + E
    if mut.get("lastcol_from_neighbour"):                # mutant: the last column of an odd-width map takes its neighbour's result
        cur = cur.copy(); cur[:, -1] = cur[:, -2]
    return dict(y=cur, bound=e, S=S, pre=pre)


def compare(got, ref, bound):
    """largest |got - ref| / bound (0 / 0 counts as 0); the caller asserts <= 1"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bound)
    return float(np.max(r)) if r.size else 0.0


# ---- the head --------------------------------------------------------------------------------------------------------------------------------
def _normalise(v, e, axis, n_terms):
    """v / max(|v|_2, 1e-12) along `axis` and its bound: the norm errs by at most |e|_2 (triangle inequality) plus the fp32 rounding of a sum of n_terms
    squares, a square root and the squares themselves ((n_terms + 2) / 2 + 2 relative roundings); the quotient adds one rounding."""
    n = np.sqrt(np.sum(v * v, axis=axis, keepdims=True))
    en = np.sqrt(np.sum(e * e, axis=axis, keepdims=True)) + ((n_terms + 2) / 2.0 + 2.0) * U * n
    nf = np.maximum(n, 1e-12)
    lo = np.maximum(nf - en, 1e-12)                      # the smallest norm the GPU can have divided by
    y = v / nf
    eb = e / lo + np.abs(v) * en / (nf * lo) + U * np.abs(y)
    return y, eb


def head(x, assign_w, assign_b, centroids, mfma, chunk=64):
    """x [np, D] pre-projected features -> (descriptor [K * D], bound, mass [K] = total assignment per cluster).
    Softmax assignment a = softmax(x Wa^T + ba) with the maximum subtracted; V[k] = sum_p a[p][k] (c[k] - x[p]); intra-normalisation; global L2.
    The kernels evaluate exp as exp2(t * log2 e) on the hardware's exp2 (1 ulp): relative error (2 |t| + 4) 2^-24 on top of the logits' own error."""
    x = np.asarray(x, np.float64)
    Wa, ba, c = (np.asarray(v, np.float64) for v in (assign_w, assign_b, centroids))
    npos, D = x.shape
    K = Wa.shape[0]
    nchunk = (npos + chunk - 1) // chunk
    lg = x @ Wa.T + ba
    e_l = (D + 1 + 2) * U * (np.abs(x) @ np.abs(Wa).T + np.abs(ba))
    m = lg.max(axis=1, keepdims=True)
    t = lg - m
    d_t = e_l + e_l.max(axis=1, keepdims=True) + U * np.abs(t)
    ex = np.exp(t)
    rel_e = np.expm1(d_t + (2.0 * np.abs(t) + 4.0) * U)                   # exp(t + d) / exp(t) - 1: not linearised, the logits may be large
    sm = ex.sum(axis=1, keepdims=True)
    rel_s = (ex * rel_e).sum(axis=1, keepdims=True) / sm + (K + 2 + 1) * U   # the sum of the K exponentials, and the quotient's rounding
    a = ex / sm
    d_a = a * ((1.0 + rel_e) / (1.0 - np.minimum(rel_s, 0.5)) - 1.0) + 1e-37      # 1e-37: an exponential flushed to zero
    Kt = npos + nchunk                                   # terms of a sum over the positions of the chunks, then over the chunks
    mass = a.sum(axis=0)
    if mfma:
        Ssum = mass[:, None]
        P = a.T @ x
        V = c * Ssum - P
        e_S = (Kt + 2) * U * Ssum + d_a.sum(axis=0)[:, None]
        e_P = (Kt + 2) * U * (a.T @ np.abs(x)) + d_a.T @ np.abs(x)
        e_V = np.abs(c) * e_S + e_P + 2 * U * (np.abs(c) * Ssum + np.abs(P))
    else:
        diff = np.abs(c[None, :, :] - x[:, None, :])                       # [np, K, D]
        V = (a[:, :, None] * (c[None, :, :] - x[:, None, :])).sum(axis=0)
        S_V = (a[:, :, None] * diff).sum(axis=0)
        e_V = (Kt + 2 + 1) * U * S_V + (d_a[:, :, None] * diff).sum(axis=0)      # + 1: the rounding of c - x
    v1, e1 = _normalise(V, e_V, 1, D)
    v2, e2 = _normalise(v1.reshape(-1), e1.reshape(-1), 0, K * D)
    return v2, e2, mass


def pca(v, e_v, comp, mean):
    """y = comp (v - mean), y / |y|.  -> (y, bound)"""
    comp, mean = np.asarray(comp, np.float64), np.asarray(mean, np.float64)
    n = v.shape[0]
    d = v - mean
    y = comp @ d
    S = np.abs(comp) @ (np.abs(d) + e_v)
    e = (n + 1 + 2) * U * S + np.abs(comp) @ e_v         # + 1: the rounding of v - mean
    return _normalise(y, e, 0, y.shape[0])


def forward(img_u8, nv, pca_mats=None):
    """the whole network in float64 (no bounds): (descriptor, [layer outputs], features)"""
    outs = []
    cur = img_u8
    for l in nv["layers"]:
        r = chain([l], cur, res=outs[l["res"]] if l["res"] >= 0 else None)
        outs.append(r["y"]); cur = r["y"]
    hd = nv["head"]
    feat = cur @ np.asarray(hd["pre_w"], np.float64).T + np.asarray(hd["pre_b"], np.float64)
    K, D = hd["assign_w"].shape
    d, e, _ = head(feat.reshape(-1, D), hd["assign_w"], hd["assign_b"], hd["centroids"], mfma=False)
    if pca_mats is not None:
        d, e = pca(d, e, pca_mats[0], pca_mats[1])
    return d, outs, feat
