"""References, inputs and comparisons for ONE layer of the direct SuperPoint conv kernels (csrc/conv.hip, conv_f16.hip, conv_pc.hip, conv1x1.hip), shared by
tests/test_conv_layer_edges_cpu.py (no GPU: the cases are what they claim, the comparisons reject mutants) and tests/test_conv_layer_edges.py (GPU).

A layer is y = pool2(relu(conv(x, w) + b)) on NHWC fp32 tensors, zero padding k / 2, the pool 2x2 with floor.  Per precision (include/d2fe.h, d2fe_precision):

  D2FE_PREC_F32    the oracle's fmaf chain (oracle.conv, oracle.maxpool2); the device is held to it BIT FOR BIT.
  D2FE_PREC_F16    tests/helpers/f16_oracle.layer: real arithmetic on the rounded operands x^ = fp16(clamp(16 x)), w^ = fp16(clamp(256 w)); the device is held to
                   |y - ref| <= (K + 2) * 2^-24 * S,  S = sum |x^ w^| 2^-12 + |b|,  K = k * k * Cin  (the library's stated bound).
  D2FE_PREC_F16X2  x2_layer below: xs = clamp(16 x) in fp32, hi = fp16(xs), lo = fp16(xs - hi) (the residual is exact in fp32, its conversion rounds), likewise
                   the weights with 256; real arithmetic on  sum (hi_x hi_w + hi_x lo_w + lo_x hi_w) 2^-12 + b  -- lo_x lo_w is NOT part of the mode.
                   Bound.  Every product of two fp16 numbers is exact in fp32 (11 + 11 bits), and 4096 b is exact.  The device adds n = 3 K + 1 exact terms (3 K
                   products and the scaled bias it starts from) in fp32, in an order of the matrix instruction's own.  Any order of n - 1 fp32 additions, each
                   with relative error at most u = 2^-24, leaves |err| <= ((1 + u)^(n - 1) - 1) * sum |t_i| <= (n - 1) u S3 (1 + O(n u)); the final scaling
                   by 2^-12 is exact.  With one term of margin for the O(n u) tail (n u < 2.1e-4 for the largest K = 1152), as the F16 bound keeps it:
                       |y - ref| <= (3 K + 2) * 2^-24 * S3,   S3 = sum (|hi hi| + |hi lo| + |lo hi|) 2^-12 + |b|.
                   ReLU and max are 1-Lipschitz: a pooled output inherits the largest of its four bounds.

EXACT cases.  Operands sit on a grid such that every term the device adds is an integer multiple of one unit q and sum |terms| < 2^24 q for every output: every
partial sum, in any order and any grouping, is then an integer multiple of q below 2^24 q, i.e. exactly representable in fp32, no addition rounds, and the device
must return the integer result bit for bit (exact_guard asserts the premise per output).  Only such inputs can see a dropped cross term or a wrong operand
rounding: on random data these stay far inside the summation bound."""
import functools

import numpy as np

from tests.helpers import f16_oracle as fo

SA, SW = fo.SA, fo.SW
SCALE = 2.0 ** -(SA + SW)
U = 2.0 ** -24
LAYER_LIMIT = 0.01      # random-input cases: the bound is at most 1 % of the tensor's largest |y| (the NetVLAD suite's LAYER_LIMIT)
PREC_F32, PREC_F16X2, PREC_F16 = 0, 1, 3
PRECS = (PREC_F32, PREC_F16X2, PREC_F16)
# ConvShape of csrc/kernels.h -> (Cin, k)
S64, S128_32, S128_16, S1X1, SFUSED = 0, 1, 2, 3, 4
SHAPE_GEOM = {S64: (64, 3), S128_32: (128, 3), S128_16: (128, 3), S1X1: (256, 1), SFUSED: (64, 3)}
NAN_IN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]      # input padding: a kernel that reads it poisons its output
POISON = np.array([0x7FC0BEEF], np.uint32).view(np.float32)[0]      # output pre-fill: compared as bits


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- which kernels exist --------------------------------------------------------------------------------------------------------------------------------------
def tile_of(family, shape, conv64_tile=1):
    """(TH, TW, BN) of the kernel a (family, shape) launches: family 1 one-tile (launch_conv_tile), 2 persistent (launch_conv_pc)"""
    if shape in (S64, SFUSED):
        return (8, 32, 64) if (family == 1 and shape == S64 and conv64_tile == 0) else (4, 32, 64)
    if shape == S128_32:
        return (4, 32, 128) if family == 1 else (4, 16, 128)
    return (4, 16, 128)


def compiled(family):
    """every (shape, conv64_tile, pool, relu) the launchers of a family compile"""
    out = []
    if family == 1:
        for tile in (1, 0):
            out += [(S64, tile, p, r) for p in (False, True) for r in (False, True)]
        out += [(S128_32, 1, p, r) for p in (False, True) for r in (False, True)]
        out += [(S128_16, 1, False, r) for r in (False, True)] + [(S1X1, 1, False, r) for r in (False, True)]
        out += [(SFUSED, 1, True, True)]
    elif family == 2:
        out = [(S64, 1, True, True), (S64, 1, False, True), (S128_32, 1, True, True), (S128_16, 1, False, True), (S1X1, 1, False, False), (SFUSED, 1, True, True)]
    return out


def pc_items(shape, n, H, W, cout):
    """work items of launch_conv_pc: tiles x channel groups x images"""
    th, tw, bn = tile_of(2, shape)
    return -(-W // tw) * -(-H // th) * (-(-cout // bn)) * n


# ---- arithmetic -----------------------------------------------------------------------------------------------------------------------------------------------
def corr(x, w, dtype=np.float64):
    """sum over (ky, kx, ci) of x[y + ky - p, x + kx - p, ci] * w[co, ci, ky, kx], zero outside: [H, W, Cout] in `dtype` (products and sums in `dtype`)"""
    H, W, C = x.shape
    co, ci, k, _ = w.shape
    assert ci == C
    p = k // 2
    xp = np.zeros((H + 2 * p, W + 2 * p, C), dtype)
    xp[p:p + H, p:p + W] = x
    acc = np.zeros((H * W, co), dtype)
    for ky in range(k):
        for kx in range(k):
            acc += xp[ky:ky + H, kx:kx + W].reshape(H * W, C) @ np.ascontiguousarray(w[:, :, ky, kx].T.astype(dtype))
    return acc.reshape(H, W, co)


def pool2(y, anchor_end=False):
    """2x2 max with floor; anchor_end (a MUTANT): the windows end at the last row / column instead of starting at the first"""
    H, W = y.shape[:2]
    Ho, Wo = H // 2, W // 2
    oy, ox = (H - 2 * Ho, W - 2 * Wo) if anchor_end else (0, 0)
    return y[oy:oy + 2 * Ho, ox:ox + 2 * Wo].reshape(Ho, 2, Wo, 2, -1).max(axis=(1, 3))


def finish(y, relu, pool, anchor_end=False):
    if relu:
        y = np.maximum(y, 0)
    return pool2(y, anchor_end) if pool else y


def trunc16(s):
    """fp16 conversion that truncates towards zero (a MUTANT of round-to-nearest-even)"""
    with np.errstate(over="ignore"):
        h = np.asarray(s, np.float32).astype(np.float16)
    over = np.abs(h.astype(np.float32)) > np.abs(s)
    h[over] = np.nextafter(h[over], np.float16(0))
    return h


def operand16(v, shift, mutant=None):
    """the F16 contract's operand, or a mutant of it: 'trunc', 'noclamp', 'flush'"""
    with np.errstate(over="ignore"):
        s = np.asarray(v, np.float32) * np.float32(2.0 ** shift)
        if mutant != "noclamp":
            s = np.clip(s, np.float32(-fo.CLAMP), np.float32(fo.CLAMP))
        h = trunc16(s) if mutant == "trunc" else s.astype(np.float16)
    if mutant == "flush":
        h = np.where(np.abs(h.astype(np.float32)) < 2.0 ** -14, np.float16(0), h)
    return h


def f16_layer(x, w, b, relu, pool, mutant=None):
    """f16_oracle.layer restated on corr() so that the operand mutants can be evaluated: (y, S) float64"""
    xh, wh = operand16(x, SA, mutant).astype(np.float64), operand16(w, SW, mutant).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        y = corr(xh, wh) * SCALE + np.asarray(b, np.float64)
    S = corr(np.abs(np.nan_to_num(xh, posinf=0, neginf=0)), np.abs(np.nan_to_num(wh, posinf=0, neginf=0))) * SCALE + np.abs(np.asarray(b, np.float64))
    return finish(y, relu, pool), finish(S, False, pool)


def split16(v, shift, trunc_hi=False):
    """the F16X2 operand: (hi, lo) as float16"""
    with np.errstate(over="ignore"):
        s = np.clip(np.asarray(v, np.float32) * np.float32(2.0 ** shift), np.float32(-fo.CLAMP), np.float32(fo.CLAMP))
    hi = trunc16(s) if trunc_hi else s.astype(np.float16)
    lo = (s - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


X2_TERMS = ("hh", "hl", "lh")


def x2_layer(x, w, b, relu, pool, terms=X2_TERMS, trunc_hi=False):
    """the D2FE_PREC_F16X2 contract in float64: (y, S3).  terms / trunc_hi evaluate MUTANTS (a dropped cross term, a kept lo * lo, a truncating hi)."""
    xh, xl = [a.astype(np.float64) for a in split16(x, SA, trunc_hi)]
    wh, wl = [a.astype(np.float64) for a in split16(w, SW, trunc_hi)]
    part = {"hh": (xh, wh), "hl": (xh, wl), "lh": (xl, wh), "ll": (xl, wl)}
    acc = sum(corr(*part[t]) for t in terms)
    S3 = sum(corr(np.abs(a), np.abs(c)) for a, c in (part[t] for t in X2_TERMS))
    b = np.asarray(b, np.float64)
    return finish(acc * SCALE + b, relu, pool), finish(S3 * SCALE + np.abs(b), False, pool)


def kdim(w):
    return w.shape[1] * w.shape[2] * w.shape[3]


def conv1a_act(orc, frame, w1a, b1a):
    """relu(conv1a(u8 / 255)): exact fp32 in every mode, [H, W, 64]"""
    return orc.conv(orc.prep_u8(frame)[:, :, None], w1a, b1a, True)


def reference(prec, orc, x, w, b, relu, pool):
    """one image: ('bits', y fp32) for D2FE_PREC_F32, ('bound', y float64, bound float64) for the fp16 modes"""
    if prec == PREC_F32:
        y = orc.conv(x, w, b, relu)
        return ("bits", orc.maxpool2(y) if pool else y)
    if prec == PREC_F16:
        y, S = fo.layer(x, w, b, relu, pool)
        return ("bound", y, (kdim(w) + 2) * U * S)
    y, S3 = x2_layer(x, w, b, relu, pool)
    return ("bound", y, (3 * kdim(w) + 2) * U * S3)


def same_bits(got, want):
    """bit equality, the sign of a zero included"""
    g, t = bits(got), bits(want)
    return g.shape == t.shape and bool(np.array_equal(g, t))


def compare(got, ref):
    """(ok, largest error / bound or None, text).  got: fp32 [H', W', Cout] of one image."""
    if ref[0] == "bits":
        ok = same_bits(got, ref[1])
        txt = "" if ok else "%d of %d outputs differ in bits, largest |difference| %g" % (
            int((bits(got) != bits(ref[1])).sum()), got.size, float(np.nanmax(np.abs(got.astype(np.float64) - ref[1]))) if got.shape == ref[1].shape else -1)
        return ok, None, txt
    _, y, bound = ref
    if got.shape != y.shape or not np.all(np.isfinite(got)):
        return False, np.inf, "shape or non-finite output"
    err = np.abs(got.astype(np.float64) - y)
    q = float((err / np.maximum(bound, 1e-300)).max())
    bad = np.argwhere(err > bound)
    return len(bad) == 0, q, "" if len(bad) == 0 else "%d outputs beyond the bound, first %s: |%g - %g| > %g" % (
        len(bad), tuple(bad[0]), got[tuple(bad[0])], y[tuple(bad[0])], bound[tuple(bad[0])])


def layer_limit_ok(ref):
    """the stated condition of the random-input cases: the bound at every output is at most LAYER_LIMIT of the tensor's largest |y|"""
    _, y, bound = ref
    return float(bound.max()) <= LAYER_LIMIT * float(np.abs(y).max())


# ---- buffers: the caller's whole padded tensors ----------------------------------------------------------------------------------------------------------------
def pack_in(x, cstride, coff, gap, fill=NAN_IN, neighbours=None):
    """x [n, H, W, C] -> (flat buffer, in_img_stride): pixel stride cstride, channel offset coff, `gap` floats between images, everything else `fill`
    (neighbours [n, H, W, cstride]: real numbers in the other channels instead, for the heads that read one half of a 512-channel tensor)"""
    n, H, W, C = x.shape
    assert cstride >= coff + C
    istride = H * W * cstride + gap
    buf = np.full(n * istride + 8, fill, np.float32)
    for i in range(n):
        v = buf[i * istride:i * istride + H * W * cstride].reshape(H, W, cstride)
        if neighbours is not None:
            v[:] = neighbours[i]
        v[:, :, coff:coff + C] = x[i]
    return buf, istride


def make_out(n, Ho, Wo, cout, cstride, coff, gap):
    assert cstride >= coff + cout
    istride = Ho * Wo * cstride + gap
    return np.full(n * istride + 8, POISON, np.float32), istride


def unpack_out(buf, n, Ho, Wo, cout, cstride, coff, istride):
    """-> (y [n, Ho, Wo, cout], True when every float outside the tensor still holds the poison)"""
    mask = np.ones(buf.size, bool)
    y = np.empty((n, Ho, Wo, cout), np.float32)
    for i in range(n):
        sl = slice(i * istride, i * istride + Ho * Wo * cstride)
        y[i] = buf[sl].reshape(Ho, Wo, cstride)[:, :, coff:coff + cout]
        m = mask[sl].reshape(Ho, Wo, cstride)
        m[:, :, coff:coff + cout] = False
    return y, bool(np.all(bits(buf)[mask] == bits(POISON)))


def pack_frames(frames, row_stride, gap, fill=0xA5):
    """frames [n, H, W] u8 -> (flat buffer, img_istride), row stride > W and `gap` bytes between images filled with `fill`"""
    n, H, W = frames.shape
    assert row_stride >= W
    istride = H * row_stride + gap
    buf = np.full(n * istride + 8, fill, np.uint8)
    for i in range(n):
        buf[i * istride:i * istride + H * row_stride].reshape(H, row_stride)[:, :W] = frames[i]
    return buf, istride


# ---- random inputs --------------------------------------------------------------------------------------------------------------------------------------------
def _ro(*a):
    for v in a:
        v.setflags(write=False)
    return a if len(a) > 1 else a[0]


@functools.lru_cache(maxsize=None)
def rand_weights(cin, ks, cout, seed=0):
    """N(0, 1 / sqrt(K)) weights, biases of order 0.1 with both signs: pre-ReLU sums of both signs, outputs of order 1"""
    rng = np.random.RandomState(7000 + 13 * cin + ks + 131 * cout + seed)
    return _ro((rng.randn(cout, cin, ks, ks) / np.sqrt(cin * ks * ks)).astype(np.float32), (0.1 * rng.randn(cout)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def rand_act(n, H, W, cin, seed=0):
    """post-ReLU activations: max(N(0, 1), 0), about half of them zero"""
    rng = np.random.RandomState(9000 + 7 * H + W + 1009 * cin + 31 * n + seed)
    return _ro(np.maximum(rng.randn(n, H, W, cin), 0).astype(np.float32))


@functools.lru_cache(maxsize=None)
def rand_frames(n, H, W, seed=0):
    return _ro(np.random.RandomState(5000 + 3 * H + W + seed).randint(0, 256, (n, H, W)).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def conv1a_weights():
    """conv1a [64, 1, 3, 3] with biases of both signs: about half the channels of a patch pixel are cut by the ReLU"""
    rng = np.random.RandomState(77)
    return _ro((rng.randn(64, 1, 3, 3) / 3.0).astype(np.float32), (0.2 * rng.randn(64)).astype(np.float32))


def f32_specials(x, w, seed=0):
    """D2FE_PREC_F32 only: copies of (x, w) with -0.0, fp32 subnormal activations and weights, and normal pairs whose product underflows into the
    subnormal range (the mode promises the oracle's fmaf chains bit for bit, gradual underflow included)"""
    rng = np.random.RandomState(100 + seed)
    x, w = x.copy(), w.copy()
    fx, fw = x.reshape(-1), w.reshape(-1)
    ix = rng.permutation(fx.size)
    k = max(4, fx.size // 16)
    fx[ix[:k]] = -0.0
    fx[ix[k:2 * k]] = (rng.randint(1, 1 << 22, k).astype(np.uint32)).view(np.float32)                    # subnormal activations
    fx[ix[2 * k:3 * k]] = np.float32(2.0 ** -80) * (1 + rng.rand(k).astype(np.float32))                 # x w ~ 2^-140: the product is subnormal
    iw = rng.permutation(fw.size)
    kw = max(4, fw.size // 16)
    fw[iw[:kw]] = (rng.randint(1, 1 << 22, kw).astype(np.uint32)).view(np.float32) * rng.choice([-1, 1], kw).astype(np.float32)
    fw[iw[kw:2 * kw]] = np.float32(2.0 ** -60) * rng.choice([-1, 1], kw).astype(np.float32)
    fw[iw[2 * kw:3 * kw]] = -0.0
    return x, w


# ---- exact cases ----------------------------------------------------------------------------------------------------------------------------------------------
def grid_unit(v):
    """the largest power of two q such that every entry of v is an integer multiple of q (v finite, float64)"""
    v = np.asarray(v, np.float64).reshape(-1)
    v = v[v != 0]
    if v.size == 0:
        return np.inf
    for e in range(80, -200, -1):
        s = v * 2.0 ** -e
        if np.all(s == np.rint(s)):
            return 2.0 ** e
    raise AssertionError("no grid")


def exact_terms(prec, x, w, b):
    """the operand pairs the device multiplies (already rounded, float64) and the unit q of its terms in accumulator scale (before the 2^-12)"""
    if prec == PREC_F16:
        xh, wh = fo.round_operand(x, SA).astype(np.float64), fo.round_operand(w, SW).astype(np.float64)
        pairs = [(xh, wh)]
    else:
        xh, xl = [a.astype(np.float64) for a in split16(x, SA)]
        wh, wl = [a.astype(np.float64) for a in split16(w, SW)]
        pairs = [(xh, wh), (xh, wl), (xl, wh)]
    # a product pairs an activation with a weight of the SAME input channel: the unit of the products is the smallest over the channels
    q = grid_unit(np.asarray(b, np.float64) / SCALE)
    for a, c in pairs:
        for ci in range(a.shape[2]):
            qa, qc = grid_unit(a[:, :, ci]), grid_unit(c[:, ci])
            if np.isfinite(qa) and np.isfinite(qc):
                q = min(q, qa * qc)
    return pairs, q


def exact_guard(prec, x, w, b):
    """asserts the premise of an exact case for one image: sum |terms| / q < 2^24 at every output.  Returns (largest ratio / 2^24, q)."""
    pairs, q = exact_terms(prec, x, w, b)
    tot = sum(corr(np.abs(a), np.abs(c)) for a, c in pairs) + np.abs(np.asarray(b, np.float64)) / SCALE
    r = float(tot.max() / q)
    assert np.isfinite(q) and r < 2.0 ** 24, "not an exact case: sum |terms| spans %g units of %g" % (r, q)
    return r / 2.0 ** 24, q


def exact_value(prec, x, w, b, relu, pool, how="int"):
    """the value an exact case must return, fp32 [H', W', Cout], three ways: 'int' (int64 arithmetic on the operands in units of their grids), 'f64'
    (float64), 'f32shuffle' (fp32 products and sums with the taps and channels in a shuffled order)"""
    pairs, q = exact_terms(prec, x, w, b)
    bq = np.asarray(b, np.float64) / SCALE
    if how == "int":
        acc = np.zeros(x.shape[:2] + (w.shape[0],), np.int64)
        for a, c in pairs:
            ai, ci_ = np.zeros(a.shape, np.int64), np.zeros(c.shape, np.int64)
            for ch in range(a.shape[2]):      # per input channel: activations in units of their grid, weights in units of q / that grid
                qa, qc = grid_unit(a[:, :, ch]), grid_unit(c[:, ch])
                if not (np.isfinite(qa) and np.isfinite(qc)):
                    continue
                m = qa * qc / q
                assert m == int(m) and m >= 1
                ai[:, :, ch] = np.rint(a[:, :, ch] / qa)
                ci_[:, ch] = np.rint(c[:, ch] / qc) * int(m)
            acc += corr(ai, ci_, np.int64)
        acc += np.rint(bq / q).astype(np.int64)
        y = acc.astype(np.float64) * q * SCALE
    elif how == "f64":
        y = (sum(corr(a, c) for a, c in pairs) + bq) * SCALE
    else:
        rng = np.random.RandomState(5)
        pc, pt = rng.permutation(x.shape[2]), rng.permutation(w.shape[2] * w.shape[3])
        acc = np.zeros(x.shape[:2] + (w.shape[0],), np.float32)
        k = w.shape[2]
        for a, c in pairs[::-1]:
            a32, c32 = a.astype(np.float32)[:, :, pc], c.astype(np.float32)[:, pc]
            for t in pt:      # one tap at a time, fp32 throughout
                wt = np.zeros_like(c32)
                wt[:, :, t // k, t % k] = c32[:, :, t // k, t % k]
                acc += corr(a32, wt, np.float32)
        y = ((acc + bq.astype(np.float32)) * np.float32(SCALE)).astype(np.float64)
    out = finish(y, relu, pool)
    assert np.array_equal(out.astype(np.float32).astype(np.float64), out)      # representable: the guard's consequence
    return out.astype(np.float32)


def _sparse_int(rng, shape, lo, hi, density, signed=True):
    v = rng.randint(lo, hi + 1, shape).astype(np.float64)
    if signed:
        v *= rng.choice([-1.0, 1.0], shape)
    return v * (rng.rand(*shape) < density)


@functools.lru_cache(maxsize=None)
def exact_case(kind, cin, ks, cout, H=6, W=34):
    """(x [H, W, cin], w [cout, cin, ks, ks], b [cout]) fp32, every value on a grid; see EXACT_KINDS.  The bias is k / 16 with both signs."""
    rng = np.random.RandomState(4242 + 17 * EXACT_KINDS.index(kind) + cin + ks + cout)
    K = cin * ks * ks
    wsh = (cout, cin, ks, ks)
    b = rng.randint(-24, 25, cout) / 16.0
    dens = min(1.0, 96.0 / K)      # about 96 non-zero weights per output: the sums stay far below 2^24 units
    if kind == "ties":
        # 16 x = an odd integer in [2049, 4095]: exactly between two fp16 neighbours (spacing 2); RNE takes the even significand: down for 1 mod 4, up for 3 mod 4
        X = 2049.0 + 2 * rng.randint(0, 1024, (H, W, cin))
        X *= rng.rand(H, W, cin) < 0.5
        Wt = _sparse_int(rng, wsh, 1, 3, dens)
        # ... and weights with 256 w an odd integer of the same range on a few positions, against the exactly representable activations of channel 0
        X[:, :, 0] = rng.randint(0, 4, (H, W))
        Wt[:, 0] = (2049.0 + 2 * rng.randint(0, 1024, (cout, ks, ks))) * rng.choice([-1.0, 1.0], (cout, ks, ks)) * (rng.rand(cout, ks, ks) < 0.34)
    elif kind == "clamp":
        # activations at and beyond the clamp (all become 65000 -> fp16 64992), weights beyond +-65000 / 256
        X = _sparse_int(rng, (H, W, cin), 0, 48, 0.5, signed=False)
        hot = rng.rand(H, W, cin) < 0.02
        X[hot] = rng.choice([4062.5 * 16, 5000.0 * 16, 1e9 * 16, np.inf], int(hot.sum()))
        Wt = _sparse_int(rng, wsh, 1, 2, dens / 4)
        X[:, :, 1] = rng.randint(0, 3, (H, W))
        Wt[:, 1] = rng.choice([300.0 * 256, -1000.0 * 256, 254.0 * 256, -65000.0], (cout, ks, ks)) * (rng.rand(cout, ks, ks) < 0.34)
    elif kind == "subnormal":
        # 16 x = k 2^-24 (an fp16 subnormal) against 256 w = +-2^15: the products k 2^-9 are all there is (the bias is zero): flushing returns max(0, 0)
        X = rng.randint(1, 1024, (H, W, cin)) * 2.0 ** -24 * (rng.rand(H, W, cin) < 0.5)
        Wt = 32768.0 * rng.choice([-1.0, 1.0, 1.0], wsh) * (rng.rand(*wsh) < dens)
        # and the same on the weight side: 256 w = k 2^-24 against 16 x = 2^15 in channel 0
        X[:, :, 0] = 32768.0 * (rng.rand(H, W) < 0.5)
        Wt[:, 0] = rng.randint(1, 1024, (cout, ks, ks)) * 2.0 ** -24 * rng.choice([-1.0, 1.0, 1.0], (cout, ks, ks))
        b = np.zeros(cout)
    elif kind == "wide_x":
        X = rng.randint(4097, 16384, (H, W, cin)).astype(np.float64) * (rng.rand(H, W, cin) < 0.6)      # 13-14 significant bits: lo = -4 .. 4
        Wt = _sparse_int(rng, wsh, 1, 2, dens)
    elif kind == "wide_w":
        X = _sparse_int(rng, (H, W, cin), 1, 3, 0.6, signed=False)
        Wt = _sparse_int(rng, wsh, 4097, 16383, dens)
    elif kind == "wide_both":
        # 12 significant bits on both sides (odd integers in [2049, 2599]: lo = +-1), three non-zero weights per output: lo_x lo_w = +-1 per product
        X = np.zeros((H, W, cin))
        X[:, :, :3] = 2049.0 + 2 * rng.randint(0, 276, (H, W, 3))
        Wt = np.zeros(wsh)
        for co in range(cout):
            for c in range(3):
                Wt[co, c, rng.randint(ks), rng.randint(ks)] = (2049.0 + 2 * rng.randint(0, 276)) * rng.choice([-1.0, 1.0])
    else:
        raise KeyError(kind)
    with np.errstate(over="ignore"):
        x, w = (X / 2.0 ** SA).astype(np.float32), (Wt / 2.0 ** SW).astype(np.float32)
    return _ro(x, w, b.astype(np.float32))


EXACT_KINDS = ("ties", "clamp", "subnormal", "wide_x", "wide_w", "wide_both")
EXACT_FOR = {PREC_F16: ("ties", "clamp", "subnormal"), PREC_F16X2: ("wide_x", "wide_w", "wide_both", "clamp")}


# ---- structural mutants of a reference: what a wrong kernel would compute ---------------------------------------------------------------------------------------
STRUCT_MUTANTS = ("dropped_tap", "border_read", "in_coff_plus_4", "dropped_bias", "pool_anchor")


def mutant_inputs(name, xfull, coff, cin, w, b):
    """(x, w, b, edge, anchor_end) a kernel with the named defect would effectively evaluate.  xfull [H, W, cstride] holds real numbers around the layer's channels."""
    x = xfull[:, :, coff:coff + cin]
    edge = anchor = False
    if name == "dropped_tap":
        w = w.copy()
        w[:, -1, -1, -1] = 0      # the last (ky, kx, ci) of the chain
    elif name == "border_read":
        edge = True
    elif name == "in_coff_plus_4":
        x = xfull[:, :, coff + 4:coff + 4 + cin]
    elif name == "dropped_bias":
        b = np.zeros_like(b)
    elif name == "pool_anchor":
        anchor = True
    else:
        raise KeyError(name)
    return np.ascontiguousarray(x), w, b, edge, anchor


def evaluate(prec, orc, x, w, b, relu, pool, edge=False, anchor_end=False, **kw):
    """the precision's arithmetic as fp32 output, with the structural defects: edge = the border pixel replicated where the padding is zero; anchor_end = the pool
    windows anchored at the far end.  kw goes to f16_layer / x2_layer (operand and term mutants)."""
    p = w.shape[2] // 2
    if edge and p:
        x = np.pad(x, ((p, p), (p, p), (0, 0)), mode="edge")
    if prec == PREC_F32:
        y = orc.conv(x, w, b, False).astype(np.float64)
    elif prec == PREC_F16:
        y = f16_layer(x, w, b, False, False, **kw)[0]
    else:
        y = x2_layer(x, w, b, False, False, **kw)[0]
    if edge and p:
        y = y[p:-p, p:-p]
    return finish(y, relu, pool, anchor_end).astype(np.float32)


# ---- the GPU sweep's tables (tests/test_conv_layer_edges.py runs them, tests/test_conv_layer_edges_cpu.py asserts what they reach) ------------------------------
# real output channels per shape: one and two channel groups of the persistent kernels (BN 64 / 128), and one that leaves the last 32-channel tile partial
COUTS = {S64: (64, 128, 72), S128_32: (128, 256, 136), S128_16: (128, 256, 136), S1X1: (65, 256, 40), SFUSED: (64, 40)}
WALK_GEOM = (3, 7, 47)      # images, H, W of the walk cases


def spatial_sizes(family, shape, conv64_tile=1):
    """2x2; exactly one tile; one past the tile in both directions (odd under a pool: the floor drops the last row and column); 7x47 (partial 16- and 32-wide tiles)"""
    th, tw, _ = tile_of(family, shape, conv64_tile)
    return [(2, 2), (th, tw), (th + 1, tw + 1), (7, 47)]


def layout(name, cin, cout):
    """how the caller's buffers hold the tensors: (in_cstride, in_coff, in_gap, out_cstride, out_coff, out_gap); gaps in floats between images"""
    if name == "tight":
        return (cin, 0, 0, cout, 0, 0)
    if name == "padded":      # padding channels on both sides of both tensors, a gap between images; the input side in multiples of 4 floats (float4 loads)
        return (cin + 12, 8, 20, cout + 9, 5, 7)
    if name in ("head0", "head256"):      # one half of a 512-channel tensor, as the heads read convPa | convDa
        return (512, 0 if name == "head0" else 256, 0, cout + 3, 3, 0)
    raise KeyError(name)


def sweep_cases(family, shape, conv64_tile=1):
    """[(n, H, W, cout, layout, variant)] of one kernel: every spatial size on one image, then 3 images of 7x47 with gaps for the other channel counts"""
    c = COUTS[shape]
    out = [(1, H, W, c[0], "tight", "rand") for H, W in spatial_sizes(family, shape, conv64_tile)]
    out += [(3, 7, 47, co, "padded", "rand") for co in c[1:]]
    out += [(3, 5, 33, c[0], "padded", "special"), (1, 5, 33, c[0], "tight", "zero")]
    if shape == S1X1:
        out += [(2, 5, 17, c[0], "head0", "rand"), (2, 5, 17, c[1], "head256", "rand")]
    return out


def walk_ncus(total):
    """ConvArgs::ncu values that make `total` items: fewer than the grid could hold; exactly the grid; grid + 1; three rounds with a remainder; one workgroup"""
    three = [g for g in range(2, total) if -(-total // g) == 3 and total % g]
    return [total + 4, total, total - 1, three[0], 1]


def _oracle():
    from oracle import oracle
    oracle.build()
    return oracle


@functools.lru_cache(maxsize=None)
def case_inputs(shape, n, H, W, cout, variant="rand"):
    """(x [n, H, W, cin] or None, frames [n, H, W] or None, w, b); the 'special' and 'zero' variants are for D2FE_PREC_F32's bitwise comparison"""
    cin, ks = SHAPE_GEOM[shape]
    w, b = rand_weights(cin, ks, cout)
    if shape == SFUSED:
        f = rand_frames(n, H, W)
        if variant == "zero":
            f = np.zeros_like(f)
        elif variant == "special":      # frames with saturated and black regions: conv1a outputs that the ReLU cuts, and exact zeros
            f = f.copy(); f[:, : H // 2, : W // 2] = 255; f[:, H // 2:, W // 2:] = 0
        return None, _ro(f), w, b
    x = rand_act(n, H, W, cin)
    if variant == "special":
        x, w = f32_specials(x, w)
    elif variant == "zero":
        x = np.zeros_like(x)
    return _ro(np.ascontiguousarray(x)), None, _ro(w), b


@functools.lru_cache(maxsize=None)
def case_refs(prec, shape, n, H, W, cout, pool, relu, variant="rand"):
    """the reference of every image of a case (see reference())"""
    orc = _oracle()
    x, frames, w, b = case_inputs(shape, n, H, W, cout, variant)
    refs = []
    for i in range(n):
        xi = conv1a_act(orc, frames[i], *conv1a_weights()) if shape == SFUSED else x[i]
        refs.append(reference(prec, orc, xi, w, b, relu, pool))
    return tuple(refs)
