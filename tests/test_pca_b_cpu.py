"""Variant B's descriptor PCA (d2fe_config.variant_b_pca) without a GPU: the exchange-block layout functions that take the descriptor width, the ctypes mirror of the
configuration, and the numpy statement of the PCA tail that tests/test_pca_b.py holds the kernel to -- checked here against the oracle's orc_netvlad_pca, which
evaluates the same expression y = comp (x - mean), y / |y| in double (mobilenetvlad_onnx.h:66-71 and superpoint_common.cpp:76-85 are one formula).

The bound (pca_bound).  Inputs d, mean, comp are fp32 and taken as exact; u = 2^-24; t_c = d_c - mean_c, a_j = sum_c t_c comp_jc, o_j = a_j / |a|.
  the kernel rounds t_c once, each product once and adds 256 times:   |a^_j - a_j| <= e_j = 258 u sum_c |t_c comp_jc|
  the norm: |  |a^| - |a|  | <= |e|_2; its evaluation (P squares, P - 1 additions in any order, one square root) adds a relative h = g(P + 1) / 2 + u,   g(k) = k u / (1 - k u)
  the division rounds once more
  =>  |o^_j - o_j| <= ( e_j + |a_j| (|e|_2 / |a| + h + u) ) / |a|   to first order; the second-order terms are covered by the factor 1.01."""
import ctypes as C
import os

import numpy as np
import pytest

U = 2.0 ** -24
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_notebook.npz")


def gamma(k):
    return k * U / (1.0 - k * U)


def tail64(d, mean, comp):
    """(o [n][P], a [n][P], sum_c |t_c comp_jc| [n][P]) in float64 from fp32 inputs"""
    t = np.asarray(d, np.float32).astype(np.float64) - np.asarray(mean, np.float32).astype(np.float64)
    c = np.asarray(comp, np.float32).astype(np.float64)
    a = t @ c.T
    mag = np.abs(t) @ np.abs(c).T
    with np.errstate(invalid="ignore", divide="ignore"):
        return a / np.sqrt((a * a).sum(-1, keepdims=True)), a, mag


def tail32(d, mean, comp):
    """the kernel's chain in numpy fp32: t rounded, a_j = ((0 + t_0 comp_j0) + t_1 comp_j1) + ..., every product and sum rounded; norm and division in fp32"""
    d, mean, comp = (np.asarray(x, np.float32) for x in (d, mean, comp))
    t = d - mean
    a = np.zeros((d.shape[0], comp.shape[0]), np.float32)
    for c in range(256):
        a = a + t[:, c:c + 1] * comp[None, :, c]
    assert a.dtype == np.float32
    s2 = np.zeros(d.shape[0], np.float32)
    for j in range(comp.shape[0]):
        s2 = s2 + a[:, j] * a[:, j]
    with np.errstate(invalid="ignore", divide="ignore"):
        return a / np.sqrt(s2)[:, None]


def pca_bound(d, mean, comp):
    """per-component bound on |kernel - tail64| (module docstring)"""
    _, a, mag = tail64(d, mean, comp)
    P = a.shape[1]
    e = 258 * U * mag
    na = np.sqrt((a * a).sum(-1, keepdims=True))
    h = gamma(P + 1) / 2 + U
    with np.errstate(invalid="ignore", divide="ignore"):
        return 1.01 * (e + np.abs(a) * (np.sqrt((e * e).sum(-1, keepdims=True)) / na + h + U)) / na


def qr_pca(pca_dims, seed=5):
    """(comp [pca_dims][256] with orthonormal rows, mean [256]) from a seeded QR"""
    rng = np.random.RandomState(seed)
    q, _ = np.linalg.qr(rng.randn(256, 256))
    return np.ascontiguousarray(q[:pca_dims], np.float32), (0.02 * rng.randn(256)).astype(np.float32)


def _lib():
    from d2slam_amd import api
    return api, api.load_library()


GEOMETRIES = [(1, 0), (3, 4), (60, 0), (60, 4096), (61, 64), (200, 4096), (1024, 1024)]


def test_d_layout_functions_are_the_old_ones_at_256():
    api, lib = _lib()
    for cap, G in GEOMETRIES:
        assert lib.d2fe_block_words_d(cap, 256, G) == lib.d2fe_block_words(cap, G) == api.block_words(cap, G) == api.block_words(cap, G, 256)
        assert lib.d2fe_block_bytes_int8_d(cap, 256, G) == lib.d2fe_block_bytes_int8(cap, G) == api.block_bytes_int8(cap, G)
        for f, name in enumerate(("desc", "kps", "scores", "netvlad", "n")):
            assert lib.d2fe_block_field_offset_d(cap, 256, G, f) == lib.d2fe_block_field_offset(cap, G, f) == api.block_field_offset(cap, G, name)


@pytest.mark.parametrize("D", [4, 32, 64, 68, 128, 252, 256])
def test_d_layout_fields_are_ordered_and_descriptor_rows_stay_16_byte_aligned(D):
    api, lib = _lib()
    from d2slam_amd import swarm
    for cap, G in GEOMETRIES:
        off = [lib.d2fe_block_field_offset_d(cap, D, G, f) for f in range(5)]
        words, nbytes = lib.d2fe_block_words_d(cap, D, G), lib.d2fe_block_bytes_int8_d(cap, D, G)
        assert off == [0, cap * D, cap * (D + 2), cap * (D + 3), cap * (D + 3) + G]
        assert off[0] < off[1] < off[2] < off[3] <= off[4] < words and words % 256 == 0 and words - off[4] - 1 < 256
        assert all((4 * r * D) % 16 == 0 for r in range(cap)) and (4 * off[1]) % 16 == 0      # every descriptor row, and the field behind them
        assert nbytes % 64 == 0 and 0 <= nbytes - (cap * D + G + cap * 8 + 4) < 64
        assert (cap * D + G + cap * 8) % 4 == 0                                                 # the count word of an int8 block is a word
        assert words == api.block_words(cap, G, D) == swarm.block_words(cap, G, D)
        assert nbytes == api.block_bytes_int8(cap, G, D) == swarm.block_bytes_int8(cap, G, D)
        for f, name in enumerate(("desc", "kps", "scores", "netvlad", "n")):
            assert off[f] == api.block_field_offset(cap, G, name, D) == swarm.block_field_offset(cap, G, name, D)
    assert lib.d2fe_block_bytes_int8_d(60, 64, 0) * 3 < lib.d2fe_block_bytes_int8(60, 0)           # what the narrow blocks are for
    assert 4 * lib.d2fe_block_words_d(200, 64, 4096) < 0.33 * 4 * lib.d2fe_block_words(200, 4096)


def test_d_layout_functions_refuse_what_would_misalign_a_block():
    """descriptor widths that are no multiple of 4 or outside 4..256, and a NetVLAD size that is no multiple of 4 (the int8 block's float fields and its count word
    come behind desc_q[cap][D] | netvlad_q[G]: they are words only then)"""
    _, lib = _lib()
    INVALID = -1
    for D in (0, 2, 3, 63, 66, 257, 260, -4):
        assert lib.d2fe_block_words_d(60, D, 0) == INVALID and lib.d2fe_block_bytes_int8_d(60, D, 0) == INVALID and lib.d2fe_block_field_offset_d(60, D, 0, 1) == INVALID
    for G in (1, 2, 6, 4095):
        assert lib.d2fe_block_bytes_int8_d(60, 64, G) == INVALID and lib.d2fe_block_words_d(60, 64, G) == INVALID
    assert lib.d2fe_block_bytes_int8_d(0, 64, 0) == INVALID and lib.d2fe_block_field_offset_d(60, 64, 0, 5) == INVALID
    assert b"bad argument" in lib.d2fe_last_error()


def test_config_mirror_has_the_library_s_size_and_the_field_is_off_by_default():
    api, lib = _lib()
    buf = (C.c_int32 * 256)()                       # room for any struct the library may write
    lib.d2fe_default_config(buf)
    assert buf[0] == C.sizeof(api._Config)
    # the field takes the first of the five reserved ints: the struct keeps the size it had (22 words), so d2fe_default_config writes no byte more into the
    # d2fe_config of a program compiled against the earlier header
    assert C.sizeof(api._Config) == 22 * 4 and not any(buf[22:])
    names = [n for n, _ in api._Config._fields_]
    assert names[names.index("async_tail") + 1:names.index("exact_order")] == ["variant_b_pca", "reserved"] and api._Config.reserved.size == 16
    assert api._Config.variant_b_pca.offset == api._Config.async_tail.offset + 4 and api._Config.exact_order.offset == api._Config.variant_b_pca.offset + 20
    c = api._Config()
    lib.d2fe_default_config(C.byref(c))
    assert c.struct_size == C.sizeof(api._Config) and c.variant_b_pca == 0 and list(c.reserved) == [0] * 4
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "d2fe.h")).read()
    body = hdr[hdr.index("int32_t async_tail;"):hdr.index("int32_t exact_order;")]
    assert body.index("int32_t variant_b_pca;") < body.index("int32_t reserved[4];")


def _oracle_pca(orc, x, comp, mean):
    o = np.zeros(comp.shape[0], np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    orc.lib().orc_netvlad_pca(p(x), 256, p(comp), p(mean), comp.shape[0], p(o))
    return o


@pytest.mark.parametrize("which", ["sklearn", "qr"])
def test_the_numpy_tail_agrees_with_the_oracle_within_the_bound(orc, which):
    """256 -> 64: tail64 is the oracle's value up to its rounding to fp32, tail32 is within pca_bound of it"""
    if which == "sklearn":
        g = np.load(GOLD)
        comp, mean = np.ascontiguousarray(g["pca_components"], np.float32), np.ascontiguousarray(g["pca_mean"], np.float32)
        x = np.ascontiguousarray(g["pca_probe"], np.float32)
    else:
        comp, mean = qr_pca(64)
        rng = np.random.RandomState(9)
        x = rng.randn(40, 256).astype(np.float32)
        x /= np.linalg.norm(x, axis=1, keepdims=True)
    assert comp.shape == (64, 256)
    ref = np.stack([_oracle_pca(orc, np.ascontiguousarray(r), comp, mean) for r in x]).astype(np.float64)
    o64, _, _ = tail64(x, mean, comp)
    o32 = tail32(x, mean, comp).astype(np.float64)
    b = pca_bound(x, mean, comp)
    assert np.all(np.isfinite(b)) and float(b.max()) < 1e-4
    assert np.all(np.abs(o64 - ref) <= U * np.abs(o64) + 1e-12)
    worst = float((np.abs(o32 - o64) / b).max())
    print("%s: fp32 chain against float64, worst |error| / bound = %.3f (bound up to %.3g)" % (which, worst, float(b.max())))
    assert np.all(np.abs(o32 - o64) <= b)
    assert np.all(np.abs(o32 - ref) <= b + U * np.abs(o64) + 1e-12)


def test_the_numpy_tail_gives_nan_rows_where_the_reference_expression_does():
    comp, mean = qr_pca(8)
    d = np.stack([mean, np.full(256, np.nan, np.float32), np.ones(256, np.float32)])
    o = tail32(d, mean, comp)
    assert np.all(np.isnan(o[0])) and np.all(np.isnan(o[1])) and np.all(np.isfinite(o[2]))
    o64, _, _ = tail64(d, mean, comp)
    assert np.all(np.isnan(o64[0])) and np.all(np.isnan(o64[1])) and np.all(np.isfinite(o64[2]))
