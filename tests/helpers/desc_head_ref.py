"""Plain NumPy statements of what the sparse descriptor head and variant A's descriptor tail (csrc/postproc.hip) compute, for tests/test_desc_head_edges.py:
the cells a keypoint list reads under either corner rule, the descriptor head (convDa, ReLU, convDb) in float64 with a derived fp32 summation bound, and
computeDescriptors in float64.  Nothing here imports the library or the oracle."""
import numpy as np

U = 2.0 ** -24                            # unit roundoff of fp32 (tests/helpers/nv_f64_ref.py)
F = np.float32


def gamma(n):
    """gamma_n = n u / (1 - n u): a sum of n terms formed in fp32, in any order and with or without fused multiply-adds, differs from the exact sum by at most
    gamma_n times the sum of the absolute values of the terms (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1)"""
    return n * U / (1.0 - n * U)


# ---- the cells a keypoint reads -------------------------------------------------------------------------------------------------------------------------------
def corners_b(kps, Hc, Wc):
    """Variant B (normalize_keypoints + grid_sample, superpoint_tensorrt.cpp:255-310): the four CLIPPED corner cells and their weights, in the reference's mixed
    float / double arithmetic.  kps [n, 2] -> (ix [n, 4], iy [n, 4], w [n, 4]) in the order nw, ne, sw, se."""
    kps = np.asarray(kps, F).reshape(-1, 2)

    def origin(v, size, cells):
        k = ((v - F(4)).astype(np.float64) + 0.5).astype(F)                  # kp - s / 2 + 0.5: float - int, + double, stored as float
        k = (k.astype(np.float64) / (float(size - 4) - 0.5)).astype(F)       # / (w * s - s / 2 - 0.5)
        k = k * F(2) - F(1)
        return ((k + F(1)) / F(2)) * F(cells - 1)

    ix, iy = origin(kps[:, 0], Wc * 8, Wc), origin(kps[:, 1], Hc * 8, Hc)
    x0 = np.clip(np.floor(ix).astype(np.int64), 0, Wc - 1); y0 = np.clip(np.floor(iy).astype(np.int64), 0, Hc - 1)
    x1 = np.clip(x0 + 1, 0, Wc - 1); y1 = np.clip(y0 + 1, 0, Hc - 1)
    cx = np.stack([x0, x1, x0, x1], 1); cy = np.stack([y0, y0, y1, y1], 1)
    fx0, fx1, fy0, fy1 = x0.astype(F), x1.astype(F), y0.astype(F), y1.astype(F)
    w = np.stack([(fx1 - ix) * (fy1 - iy), (ix - fx0) * (fy1 - iy), (fx1 - ix) * (iy - fy0), (ix - fx0) * (iy - fy0)], 1)
    return cx, cy, w


def corners_a(kps, Hc, Wc, img_w, img_h):
    """Variant A (computeDescriptors, superpoint_common.cpp:42-66: grid = 2 x / W - 1, then ATen's grid_sampler_unnormalize with align_corners = false,
    ((g + 1) size - 1) / 2, zeros padding): the four UNCLIPPED corner cells, their weights and which of them lie inside the map."""
    kps = np.asarray(kps, F).reshape(-1, 2)
    gx = F(2) * kps[:, 0] / F(img_w) - F(1); gy = F(2) * kps[:, 1] / F(img_h) - F(1)
    ix = ((gx + F(1)) * F(Wc) - F(1)) / F(2); iy = ((gy + F(1)) * F(Hc) - F(1)) / F(2)
    x0 = np.floor(ix).astype(np.int64); y0 = np.floor(iy).astype(np.int64)
    x1, y1 = x0 + 1, y0 + 1
    cx = np.stack([x0, x1, x0, x1], 1); cy = np.stack([y0, y0, y1, y1], 1)
    fx0, fx1, fy0, fy1 = x0.astype(F), x1.astype(F), y0.astype(F), y1.astype(F)
    w = np.stack([(fx1 - ix) * (fy1 - iy), (ix - fx0) * (fy1 - iy), (fx1 - ix) * (iy - fy0), (ix - fx0) * (iy - fy0)], 1)
    inside = (cx >= 0) & (cx < Wc) & (cy >= 0) & (cy < Hc)
    return cx, cy, w, inside


def read_cells(kps, Hc, Wc, img_w=0, img_h=0):
    """[n, 4] raster indices of the cells each keypoint's sampler reads, -1 where variant A's corner is padding (img_w = 0: variant B)"""
    if img_w:
        cx, cy, _, inside = corners_a(kps, Hc, Wc, img_w, img_h)
        return np.where(inside, cy * Wc + cx, -1)
    cx, cy, _ = corners_b(kps, Hc, Wc)
    return cy * Wc + cx


def marked_cells(kps, Hc, Wc, img_w=0, img_h=0):
    """the set of cells a keypoint list reads, ascending: what the mark / compact kernels must list"""
    c = read_cells(kps, Hc, Wc, img_w, img_h).reshape(-1)
    return np.unique(c[c >= 0])


def taps_inside(cells, Hc, Wc):
    """how many of convDa's nine taps fall inside the map, per cell"""
    cy, cx = np.asarray(cells) // Wc, np.asarray(cells) % Wc
    ny = 3 - (cy == 0) - (cy == Hc - 1); nx = 3 - (cx == 0) - (cx == Wc - 1)
    return ny * nx


# ---- the head in float64 ----------------------------------------------------------------------------------------------------------------------------------------
def head_f64(x, w_da, b_da, w_db, b_db, mutant=None):
    """x [Hc, Wc, 128] -> dict(mid, y, e_mid, bound) over the whole map: mid = ReLU(convDa x), y = convDb mid, in float64, and the fp32 summation bounds
         e_mid = gamma_1153 (|b_da| + sum |x| |w_da|)                        (9 * 128 products and the bias)
         bound = |W_db| e_mid + gamma_257 (|b_db| + sum |mid| |w_db|)        (ReLU is 1-Lipschitz: it passes e_mid through unchanged)
    mutant: None, or one of ("tap", t) convDa without tap t, ("cin", c) without input channel c, "relu" no ReLU, "bias_da" / "bias_db" without that bias."""
    x = np.asarray(x, np.float64)
    Hc, Wc, cin = x.shape
    wa = np.asarray(w_da, np.float64); wb = np.asarray(w_db, np.float64).reshape(256, 256)
    ba = np.asarray(b_da, np.float64); bb = np.asarray(b_db, np.float64)
    xp = np.zeros((Hc + 2, Wc + 2, cin))
    xp[1:-1, 1:-1] = x
    z = np.zeros((Hc, Wc, 256)); S = np.zeros((Hc, Wc, 256))
    for t in range(9):
        v = xp[t // 3:t // 3 + Hc, t % 3:t % 3 + Wc]
        wt = wa[:, :, t // 3, t % 3]
        S += np.abs(v) @ np.abs(wt).T
        if mutant == ("tap", t):
            continue
        if mutant is not None and mutant[0] == "cin":
            wt = wt.copy(); wt[:, mutant[1]] = 0.0
        z += v @ wt.T
    z = z + (0.0 if mutant == "bias_da" else ba)
    S = S + np.abs(ba)
    e_mid = gamma(9 * cin + 1) * S
    mid = z if mutant == "relu" else np.maximum(z, 0.0)
    y = mid @ wb.T + (0.0 if mutant == "bias_db" else bb)
    S2 = np.abs(mid) @ np.abs(wb).T + np.abs(bb)
    return dict(mid=mid, y=y, e_mid=e_mid, bound=e_mid @ np.abs(wb).T + gamma(257) * S2)


# ---- computeDescriptors in float64 ---------------------------------------------------------------------------------------------------------------------------
def sample_a_f64(desc_raw, kps, img_w, img_h, comp=None, mean=None):
    """desc_raw [Hc, Wc, 256] raw descriptors, kps [n, 2] (n >= 1) -> [n, 256 or pca_dims]: the dense channel L2 norm of the network's output, bilinear sampling
    at the corners and weights of corners_a with zeros padding, every CHANNEL divided by its L2 norm over the keypoints of the list, optional
    (T - mean) comp^T, row L2 norm.  The corner cells and weights are the fp32 ones (that is the operation's definition); everything behind them is float64."""
    Hc, Wc, _ = desc_raw.shape
    d = np.asarray(desc_raw, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        d = d / np.sqrt((d * d).sum(-1, keepdims=True))
        cx, cy, w, inside = corners_a(kps, Hc, Wc, img_w, img_h)
        S = np.zeros((len(cx), 256))
        for q in range(4):
            v = d[np.clip(cy[:, q], 0, Hc - 1), np.clip(cx[:, q], 0, Wc - 1)]
            S += np.where(inside[:, q, None], v * w[:, q, None].astype(np.float64), 0.0)
        T = S / np.sqrt((S * S).sum(0, keepdims=True))
        if comp is not None:
            T = (T - np.asarray(mean, np.float64)) @ np.asarray(comp, np.float64).T
        return T / np.sqrt((T * T).sum(-1, keepdims=True))
