"""Variant B's descriptor PCA (d2fe_config.variant_b_pca, sample_b_pca_kernel in csrc/postproc.hip) on the GPU: the kernel on injected tensors, a handle with the
PCA against a handle without it, the 64-float rows through every entry point, both pipes and their lists, the exchanges in every wire form, the loop store and the
keyframe window.

The bound every descriptor is held to (tests/test_pca_b_cpu.py derives it and checks the numpy statement against the oracle): with the fp32 inputs d (the 256
values a handle WITHOUT the PCA writes -- the same bits the kernel holds), mean and comp taken as exact, u = 2^-24, t_c = d_c - mean_c, a_j = sum_c t_c comp_jc:
    |a^_j - a_j| <= e_j = 258 * 2^-24 * sum_c |t_c comp_jc|     (t rounded once, 256 rounded products, 256 rounded additions)
    |out_j - a_j / |a|| <= 1.01 (e_j + |a_j| (|e|_2 / |a| + g(P + 1) / 2 + 2 u)) / |a|,   g(k) = k u / (1 - k u): the norm's P squares, P - 1 sums and root, the division
against a float64 evaluation of the same fp32 d, mean and comp.  If the GPU exceeds it, the kernel is wrong, not the bound."""
import ctypes as C

import numpy as np
import pytest

from d2slam_amd.synth import synth_stereo
from d2slam_amd.weights import synthetic_superpoint_weights
from tests.test_pca_b_cpu import pca_bound, qr_pca, tail64

H, W, CAP, PD = 120, 160, 60, 64
K = 16                                     # PCAB_K: keypoints per workgroup of sample_b_pca_kernel
RATIO = 0.8


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _copy(o):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in o.items()}


def _fe(max_batch, pd=PD, netvlad=False, b_pca=True, width=W, height=H, exact_order=False, **cfg):
    """a variant-B handle; b_pca: created with variant_b_pca and the seeded QR projection of pd dimensions set"""
    from d2slam_amd import api, netvlad as nvm
    cfg.setdefault("precision", api.PREC_F32_WINO); cfg.setdefault("max_keypoints", CAP)
    eo = dict(exact_order=True, exact_order_eps=2e-4, exact_order_crops=256) if exact_order else {}
    fe = api.FrontEnd(api.SuperPointConfig(input_width=width, input_height=height, max_batch=max_batch, **cfg), variant_b_pca=b_pca, **eo)
    fe.load_superpoint(synthetic_superpoint_weights(dustbin_bias=7.5))
    if netvlad:
        fe.load_netvlad(nvm.synthetic_netvlad_weights(depth_multiplier=0.35))
    if b_pca and pd:
        fe.set_pca(*qr_pca(pd))
        assert fe.desc_dim == pd
    return fe


def _images(n, seed=300):
    out = []
    for i in range((n + 1) // 2):
        out += list(synth_stereo(H, W, seed=seed + i))
    return np.stack(out[:n])


def _within_bound(got, d256, pd=PD, what=""):
    """rows of `got` [n][pd] against the float64 projection of the fp32 rows d256 [n][256]"""
    comp, mean = qr_pca(pd)
    ref, _, _ = tail64(d256, mean, comp)
    b = pca_bound(d256, mean, comp)
    err = np.abs(got.astype(np.float64) - ref)
    assert np.all(np.isfinite(got)) and np.all(err <= b), (what, float((err / b).max()))
    return float((err / b).max()) if len(got) else 0.0


@pytest.fixture(scope="module")
def dev():
    from d2slam_amd import api
    f = api.DevFrontEnd(api.SuperPointConfig(input_width=64, input_height=64, max_batch=1))
    yield f
    f.close()


# ---- 1. the kernel on injected tensors ------------------------------------------------------------------------------------------------------------------
HC, WC = 2, 3
COUNTS = [0, 1, K - 1, K, K + 1, 2 * K + 3]       # per image; the last one is the capacity: three workgroups, the third partly filled
NAN_IMG, NAN_KP = 5, 7


def _injected():
    rng = np.random.RandomState(11)
    n, cap = len(COUNTS), COUNTS[-1]
    raw = rng.randn(n, HC, WC, 256).astype(np.float32)
    kps = np.empty((n, cap, 2), np.float32)
    for i in range(n):                            # distinct pixels inside the full-weight region: every row finite and no two rows equal
        p = rng.permutation((8 * WC - 1) * (8 * HC - 1))[:cap]
        kps[i, :, 0] = p % (8 * WC - 1); kps[i, :, 1] = p // (8 * WC - 1)
    kps[NAN_IMG, NAN_KP] = (8 * WC - 1, 3)        # the last column: its clipped corners carry weight 0 / 0 -- a NaN row
    store = np.full((n, HC * WC + 5, 256), np.nan, np.float32)
    slotmap = np.empty((n, HC, WC), np.int32)
    for i in range(n):
        s = rng.permutation(HC * WC + 5)[:HC * WC]
        slotmap[i] = s.reshape(HC, WC); store[i, s] = raw[i].reshape(-1, 256)
    fused = np.full((n, HC, WC, 512), np.nan, np.float32)
    fused[..., 256:] = raw
    return raw, kps, store, slotmap, fused


@pytest.mark.gpu
@pytest.mark.parametrize("pd", [4, 64, 68, 256])
def test_kernel_on_injected_tensors_gpu(dev, pd):
    """a 2 x 3 cell map, counts 0, 1, K - 1, K, K + 1 and cap; both branches of the norm (pd <= 64 and above, 68 = one full column tile and a 4-wide one); the
    dense map, the fused layout and the slot map give equal bits; rows at and beyond a count are not written; a NaN row and mean == d give all-NaN rows"""
    raw, kps, store, slotmap, fused = _injected()
    comp, mean = qr_pca(pd)
    d256 = dev.debug_sample_b(raw, kps, COUNTS)
    got = dev.debug_sample_b_pca(raw, kps, COUNTS, comp, mean)
    assert got.shape == (len(COUNTS), COUNTS[-1], pd)
    worst = 0.0
    for i, n in enumerate(COUNTS):
        assert np.all(_bits(got[i, n:]) == 0xFFFFFFFF), i
        fin = np.ones(n, bool)
        if i == NAN_IMG:
            fin[NAN_KP] = False
            assert np.all(np.isnan(d256[i, NAN_KP])) and np.all(np.isnan(got[i, NAN_KP]))
        assert np.all(np.isfinite(d256[i, :n][fin]))
        worst = max(worst, _within_bound(got[i, :n][fin], d256[i, :n][fin], pd, "image %d" % i))
    print("pca_dims %d: worst |error| / bound = %.3f" % (pd, worst))
    for name, other in (("fused", dev.debug_sample_b_pca(fused, kps, COUNTS, comp, mean, dcoff=256)),
                        ("sparse", dev.debug_sample_b_pca(store, kps, COUNTS, comp, mean, slotmap=slotmap))):
        assert np.array_equal(np.isnan(other), np.isnan(got)), name
        assert np.array_equal(_bits(other)[~np.isnan(got)], _bits(got)[~np.isnan(got)]), name + " differs from the dense form"
    # mean equal to one row's d: t == 0, a == 0, 0 / 0 in every component of that row and of no other
    i, k = 3, 5
    got0 = dev.debug_sample_b_pca(raw, kps, COUNTS, comp, d256[i, k].copy())
    assert np.all(np.isnan(got0[i, k]))
    others = np.delete(got0[i, :COUNTS[i]], k, axis=0)
    assert np.all(np.isfinite(others)) and np.all(np.isfinite(got0[4, :COUNTS[4]]))


@pytest.mark.gpu
def test_hook_refuses_bad_arguments_gpu(dev):
    from d2slam_amd import api
    raw, kps, _, _, _ = _injected()
    for pd in (0, 257):
        with pytest.raises(api.D2FEError) as e:
            dev.debug_sample_b_pca(raw, kps, COUNTS, np.zeros((pd, 256), np.float32), np.zeros(256, np.float32))
        assert e.value.code == -1


# ---- 2. a handle with the PCA against a handle without it -----------------------------------------------------------------------------------------------
def _mode_cfg(api, mode):
    return {"wino": dict(), "f32_dense": dict(precision=api.PREC_F32, dense_descriptors=True), "f16x2": dict(precision=api.PREC_F16X2),
            "f16": dict(precision=api.PREC_F16), "exact_order": dict(exact_order=True), "keep_all": dict(max_keypoints=-1),
            "borders0": dict(remove_borders=0)}[mode]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["wino", "f32_dense", "f16x2", "f16", "exact_order", "keep_all", "borders0"])
def test_handle_with_pca_against_handle_without_gpu(mode):
    """same frames, same configuration: keypoints, scores and counts bit-identical; the 64 floats within the bound of the float64 projection of the 256"""
    from d2slam_amd import api
    imgs = _images(5)
    cfg = _mode_cfg(api, mode)
    plain = _fe(5, b_pca=False, **cfg)
    with_pca = _fe(5, **cfg)
    assert plain.desc_dim == 256 and with_pca.desc_dim == PD
    a, b = plain.extract_batch(imgs), with_pca.extract_batch(imgs)
    worst, nan_rows = 0.0, 0
    for (ka, sa, da), (kb, sb, db) in zip(a, b):
        assert len(ka) > 10 and np.array_equal(_bits(ka), _bits(kb)) and np.array_equal(_bits(sa), _bits(sb))
        assert da.shape == (len(ka), 256) and db.shape == (len(ka), PD)
        fin = np.isfinite(da).all(1)
        assert np.all(np.isnan(db[~fin]))                               # remove_borders = 0: the last row and column keep the reference's NaN rows
        nan_rows += int((~fin).sum())
        worst = max(worst, _within_bound(db[fin], da[fin], PD, mode))
    print("%s: worst |error| / bound = %.3f, %d NaN rows" % (mode, worst, nan_rows))
    with_pca.set_pca(None, None)                                         # off again: the 256-float rows of the plain handle
    assert with_pca.desc_dim == 256
    for (ka, sa, da), (kb, sb, db) in zip(a, with_pca.extract_batch(imgs)):
        assert np.array_equal(_bits(ka), _bits(kb)) and np.array_equal(_bits(da[np.isfinite(da)]), _bits(db[np.isfinite(db)]))
    plain.close(); with_pca.close()


# ---- 4. defaults and refusals ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_defaults_and_refusals_gpu():
    from d2slam_amd import api
    comp, mean = qr_pca(PD)
    fe = _fe(2, b_pca=False)
    with pytest.raises(api.D2FEError, match="PCA is only applied by post-processing variant A") as e:      # today's refusal and its message
        fe.set_pca(comp, mean)
    assert e.value.code == -5 and fe.desc_dim == 256
    fe.close()
    with pytest.raises(api.D2FEError) as e:                            # variant A needs no opt-in
        api.FrontEnd(api.SuperPointConfig(input_width=W, input_height=H, postproc=api.POSTPROC_A), variant_b_pca=True)
    assert e.value.code == -1
    fe = _fe(2, pd=0)
    lib = fe._lib
    for bad in (2, 3, 6, 63, 66, 257, 260, -4):
        assert lib.d2fe_set_superpoint_pca(fe.handle, comp.ctypes.data_as(C.c_void_p), mean.ctypes.data_as(C.c_void_p), bad) == -1, bad
        assert fe.desc_dim == 256
    for good in (4, 68, 256, 0, PD):
        c, m = qr_pca(max(good, 4))
        assert lib.d2fe_set_superpoint_pca(fe.handle, c.ctypes.data_as(C.c_void_p), m.ctypes.data_as(C.c_void_p), good) == 0, good
        assert fe.desc_dim == (good or 256)
    # the struct as it was before the exact_order fields (it ends behind `reserved`): what d2fe_default_config left there is "off"; the field lies inside it
    for opt_in, want in ((0, -5), (1, 0)):
        c = api._Config()
        lib.d2fe_default_config(C.byref(c))
        assert c.variant_b_pca == 0
        c.max_width, c.max_height, c.variant_b_pca = W, H, opt_in
        c.struct_size = api._Config.exact_order.offset
        h = C.c_void_p()
        assert lib.d2fe_create(C.byref(c), C.byref(h)) == 0
        assert lib.d2fe_set_superpoint_pca(h, comp.ctypes.data_as(C.c_void_p), mean.ctypes.data_as(C.c_void_p), PD) == want
        lib.d2fe_destroy(h)
    c.variant_b_pca = 2                                              # neither 0 nor 1
    assert lib.d2fe_create(C.byref(c), C.byref(h)) == -1
    # live pipes: d2fe_set_* stays refused
    pipe = api.StereoPipe(fe, lanes=1, frames=1, width=W, height=H, cap=CAP, netvlad=False)
    with pytest.raises(api.D2FEError, match="live pipes"):
        fe.set_pca(comp, mean)
    pipe.close(); fe.close()


# ---- 3. the 64-float rows through every entry point ---------------------------------------------------------------------------------------------------
def _same_rows(got, ref, what):
    (k, s, d), (rk, rs, rd) = got, ref
    assert len(k) == len(rk) and np.array_equal(_bits(k), _bits(rk)) and np.array_equal(_bits(s), _bits(rs)), what
    assert d.shape == rd.shape and np.array_equal(_bits(d), _bits(rd)), what + ": descriptor bits differ"


@pytest.mark.gpu
def test_rows_are_bit_identical_across_the_host_and_device_entry_points_gpu():
    """extract of one image, the batch of five (dense and sparse descriptor head), the device form with and without async_tail, extract_all"""
    import torch
    imgs = _images(5)
    fe = _fe(5, netvlad=True)
    ref = fe.extract_batch(imgs)
    assert all(r[2].shape[1] == PD and len(r[0]) > 10 for r in ref)
    for i in range(5):
        _same_rows(fe.extract_batch(imgs[i])[0], ref[i], "single %d" % i)
    both, _ = fe.extract_all_batch(imgs[:2], 2)
    for i in range(2):
        _same_rows(both[i], ref[i], "extract_all %d" % i)
    fe.close()
    dev = torch.device("cuda", 0)
    for async_tail in (False, True):
        fd = _fe(5, async_tail=async_tail)
        g = torch.from_numpy(imgs).to(dev)
        kps = torch.zeros((5, CAP, 2), dtype=torch.float32, device=dev); sc = torch.zeros((5, CAP), dtype=torch.float32, device=dev)
        desc = torch.zeros((5, CAP, PD), dtype=torch.float32, device=dev); idx = torch.zeros((5, CAP), dtype=torch.int32, device=dev)
        cnt = torch.zeros(5, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        fd.extract_device(g.data_ptr(), 5, W, H, kps.data_ptr(), sc.data_ptr(), desc.data_ptr(), idx.data_ptr(), CAP, cnt.data_ptr())
        if async_tail:
            fd.wait_tail()
        fd.sync(); torch.cuda.synchronize()
        for i in range(5):
            n = int(cnt[i])
            _same_rows((kps[i, :n].cpu().numpy(), sc[i, :n].cpu().numpy(), desc[i, :n].cpu().numpy()), ref[i], "device %d async_tail %d" % (i, async_tail))
        fd.close()


@pytest.mark.gpu
def test_stereo_pipe_carries_the_rows_and_matches_them_gpu(orc):
    """2 lanes x 2 frames: rows equal the batch's; the lr / prev lists equal d2fe_match_knn and the oracle's matchKNN on the delivered 64-float rows"""
    from d2slam_amd import api
    imgs = _images(8)
    fe = _fe(4)
    ref = fe.extract_batch(imgs[:4]) + fe.extract_batch(imgs[4:])
    pipe = api.StereoPipe(fe, lanes=2, frames=2, width=W, height=H, cap=CAP, netvlad=False)
    geo = [C.c_int32() for _ in range(4)]
    assert fe._lib.d2fe_pipe_geometry(pipe._p, *[C.byref(g) for g in geo]) == 0 and geo[2].value == PD
    tk = [pipe.submit(imgs[[0, 2]], imgs[[1, 3]]), pipe.submit(imgs[[4, 6]], imgs[[5, 7]])]
    res = [_copy(pipe.wait(t)) for t in tk]
    order = [[0, 2, 1, 3], [4, 6, 5, 7]]                              # rows L_0 L_1 R_0 R_1
    total = 0
    for s, o in enumerate(res):
        assert o["desc"].shape == (4, CAP, PD)
        for row, i in enumerate(order[s]):
            n = int(o["n_kp"][row])
            _same_rows((o["kps_xy"][row, :n], o["scores"][row, :n], o["desc"][row, :n]), ref[i], "submit %d row %d" % (s, row))
        for f in range(2):
            left = o["desc"][f, :int(o["n_kp"][f])]
            prev = None if (s == 0 and f == 0) else (o["desc"][f - 1, :int(o["n_kp"][f - 1])] if f else res[s - 1]["desc"][1, :int(res[s - 1]["n_kp"][1])])
            for pre, other in (("lr", o["desc"][2 + f, :int(o["n_kp"][2 + f])]), ("prev", prev)):
                n = int(o[pre + "_n"][f])
                if other is None:
                    assert n == 0
                    continue
                q, t, d = fe.match_knn(left, other, RATIO)
                oq, ot, od = orc.match_knn(left, other, RATIO)
                assert n == len(q) == len(oq), (s, f, pre)
                for got, a, b in ((o[pre + "_q"][f, :n], q, oq), (o[pre + "_t"][f, :n], t, ot)):
                    assert np.array_equal(got, a) and np.array_equal(got, b), (s, f, pre)
                assert np.array_equal(_bits(o[pre + "_dist"][f, :n]), _bits(d)) and np.array_equal(_bits(d), _bits(od)), (s, f, pre)
                total += n
    assert total > 20
    pipe.close(); fe.close()


@pytest.mark.gpu
def test_sp_lk_list_carries_the_rows_gpu():
    """the LK-carried landmark list (sp_lk): an entry discovered in a frame carries that frame's 64-float SuperPoint row"""
    from d2slam_amd import api
    imgs = _images(4)
    fe = _fe(2)
    ref = fe.extract_batch(imgs[[0, 2]])
    pipe = api.StereoPipe(fe, lanes=1, frames=1, width=W, height=H, cap=CAP, netvlad=False, match_lr=False, lr_lk=True, sp_lk=True)
    new = 0
    for s in range(2):
        o = pipe.wait(pipe.submit(imgs[2 * s][None], imgs[2 * s + 1][None]))
        n = int(o["n_kp"][0])
        _same_rows((o["kps_xy"][0, :n], o["scores"][0, :n], o["desc"][0, :n]), ref[s], "sp_lk frame %d" % s)
        T = int(o["track_n"][0])
        assert o["track_desc"].shape[-1] == PD and T > 5
        for i in range(T):
            if int(o["track_src"][0, i]) < 0:
                kp = int(o["track_kp"][0, i])
                assert 0 <= kp < n and np.array_equal(_bits(o["track_desc"][0, i]), _bits(o["desc"][0, kp]))
                new += 1
    assert new > 5
    pipe.close(); fe.close()


def _quad_fe(max_batch):
    from tests.helpers import quad_exchange_common as qc
    assert qc.CAP == CAP
    from d2slam_amd import api
    return _fe(max_batch, netvlad=True, width=qc.UW, height=qc.UH, precision=api.PREC_F32)


@pytest.mark.gpu
def test_quad_pipe_ticket_and_its_lists_carry_the_rows_gpu():
    """one quad-pipe ticket: every view's rows equal extract on the undistorted view; with sp_lk the four lists carry them"""
    from tests.helpers import quad_exchange_common as qc
    fe = _quad_fe(4)
    maps = qc.maps()
    raw = qc.rig(0, 1)
    views = np.stack([fe.undistort(raw[0, c], *maps[c]) for c in range(4)])
    ref = fe.extract_batch(views)
    for sp_lk in (False, True):
        pipe = qc.quad_pipe(fe, 1, 1, sp_lk=sp_lk)
        o = pipe.wait(pipe.submit(raw))
        assert o["desc"].shape == (1, 4, CAP, PD)
        for c in range(4):
            n = int(o["n_kp"][0, c])
            _same_rows((o["kps_xy"][0, c, :n], o["scores"][0, c, :n], o["desc"][0, c, :n]), ref[c], "view %d" % c)
            if sp_lk:
                T = int(o["track_n"][0, c])
                assert T > 5 and o["track_desc"].shape[-1] == PD
                for i in range(T):                                      # the first frame: every entry is new
                    kp = int(o["track_kp"][0, c, i])
                    assert int(o["track_src"][0, c, i]) < 0 and np.array_equal(_bits(o["track_desc"][0, c, i]), _bits(o["desc"][0, c, kp]))
        pipe.close()
    fe.close()


# ---- 5. the exchanges -------------------------------------------------------------------------------------------------------------------------------------
def _copy_cb():
    from tests.helpers import quad_exchange_common as qc
    hip = qc.hip()

    def gather(user, d_send, d_recv, nbytes, stream):      # world = 1: the gathered buffer IS the rank's blocks; a stream-ordered device copy
        return int(hip.hipMemcpyAsync(C.c_void_p(d_recv), C.c_void_p(d_send), C.c_size_t(nbytes), 3, C.c_void_p(stream)))
    return gather


def _tree(s):
    """the xor butterfly over the last axis (a power of two): pairwise fp32 sums"""
    s = s.astype(np.float32)
    while s.shape[-1] > 1:
        s = s[..., 0::2] + s[..., 1::2]
    return s[..., 0]


def _int8_codec_np(desc, n, D, renorm):
    """toLCM's quantisation of the first n rows and the decode of d2fe_unpack_blocks_int8_device, operation by operation in fp32 -> (q int8 [n][D], x f32 [n][D])"""
    x = np.ascontiguousarray(desc[:n], np.float32)
    if n == 0:
        return np.zeros((0, D), np.int8), np.zeros((0, D), np.float32)
    m = np.float32(np.abs(x).max())
    q = (x / m * np.float32(127.0)).astype(np.int32).astype(np.int8)      # C cast: truncation toward zero
    v = (q.astype(np.float64) / 127.0).astype(np.float32)
    s4 = v.reshape(-1, 4)
    s4 = ((s4[:, 0] * s4[:, 0] + s4[:, 1] * s4[:, 1]) + s4[:, 2] * s4[:, 2]) + s4[:, 3] * s4[:, 3]      # one thread's four values
    if renorm:                                                             # every row over its D floats: one wave per row, lanes beyond D / 4 hold zeros
        lanes = np.zeros((n, 64), np.float32); lanes[:, :D // 4] = s4.reshape(n, D // 4)
        s = np.repeat(_tree(lanes), D).reshape(n, D)
        rows = np.ones(n * D, bool)
    else:                                                                  # the reference: the first n 32-float segments of the flat array
        s = np.repeat(_tree(s4.reshape(-1, 8)), 32).reshape(n, D)
        rows = np.arange(n * D) // 32 < n
    out = v.copy().reshape(-1)
    sf = s.reshape(-1)
    sel = rows & (sf > 0)
    out[sel] = out[sel] / np.sqrt(sf[sel])
    return q, out.reshape(n, D)


@pytest.mark.gpu
@pytest.mark.parametrize("wire", ["fp32", "int8", "int8-renorm256"])
def test_stereo_exchange_at_64_floats_gpu(orc, wire):
    """loopback with a device copy as the collective: block sizes and fields of the _d layout, the match lists equal the host composition (d2fe_match_knn and the
    oracle on the rows of the gathered blocks), the int8 codec equals its numpy statement and the reference's compiled codec"""
    from d2slam_amd import api
    from oracle import ref as spref
    from tests.helpers import quad_exchange_common as qc
    F = 2
    fe = _fe(2 * F, netvlad=True)
    G = fe.netvlad_dim
    pipe = api.StereoPipe(fe, lanes=2, frames=F, width=W, height=H, cap=CAP, netvlad=True)
    x = api.Exchange(pipe, comm=None, world=1, rank=0, wire=wire, loopback=True, slots=2, own_stream=True, all_gather=_copy_cb())
    BLK, BLKB = api.block_words(CAP, G, PD), api.block_bytes_int8(CAP, G, PD)
    assert x.npairs == F and x.block_bytes == (4 * BLK if wire == "fp32" else BLKB)
    off = {k: api.block_field_offset(CAP, G, k, PD) for k in ("desc", "kps", "scores", "netvlad", "n")}
    imgs = _images(4, seed=710)
    t = pipe.submit(imgs[[0, 2]], imgs[[1, 3]])
    x.enqueue(t, 1)
    o = _copy(pipe.wait(t))
    r = x.collect(1)
    d_f32, d_wire = x.gathered(1)
    blocks = qc.d2h(d_f32, 4 * BLK * F).view(np.float32).reshape(F, BLK)
    wire_b = qc.d2h(d_wire, x.block_bytes * F).reshape(F, x.block_bytes)
    for f in range(F):
        n = int(o["n_kp"][f])
        blk = blocks[f]
        assert n > 10 and int(blk.view(np.int32)[off["n"]]) == n and not blk[off["n"] + 1:].any()
        rows = blk[:CAP * PD].reshape(CAP, PD)
        assert np.array_equal(_bits(blk[off["kps"]:off["kps"] + 2 * n]), _bits(o["kps_xy"][f, :n].reshape(-1))) and not rows[n:].any()
        if wire == "fp32":
            assert np.array_equal(_bits(rows[:n]), _bits(o["desc"][f, :n])) and np.array_equal(_bits(blk[off["scores"]:off["scores"] + n]), _bits(o["scores"][f, :n]))
            assert np.array_equal(_bits(blk[off["netvlad"]:off["netvlad"] + G]), _bits(o["netvlad"][f]))
        else:
            q, dec = _int8_codec_np(o["desc"][f], n, PD, wire == "int8-renorm256")
            assert np.array_equal(wire_b[f][:CAP * PD].view(np.int8).reshape(CAP, PD)[:n], q) and not wire_b[f][n * PD:CAP * PD].any()
            assert wire_b[f][CAP * PD + G + 8 * CAP:].view(np.int32)[0] == n
            assert np.array_equal(_bits(rows[:n]), _bits(dec)), "the decode differs from its numpy statement"
            g = blk[off["netvlad"]:off["netvlad"] + G]
            assert abs(float(np.linalg.norm(g)) - 1.0) < 1e-5 and float(np.abs(g - o["netvlad"][f]).max()) < 0.02
            if wire == "int8":                                          # the reference's bug, kept: 32-float segments, so only the first n / 2 rows are unit
                nrm = np.linalg.norm(rows[:n], axis=1)
                assert np.all(np.abs(nrm[:n // 2] - np.sqrt(2.0)) < 1e-5)
                assert np.array_equal(rows[(n + 1) // 2:n], (q[(n + 1) // 2:].astype(np.float64) / 127.0).astype(np.float32))      # q / 127 and nothing else
            else:
                assert np.all(np.abs(np.linalg.norm(rows[:n], axis=1) - 1.0) < 1e-6)
            if spref.available():                                       # the reference's own toLCM / LCM constructor, compiled
                assert np.array_equal(spref.quant_landmarks(o["desc"][f, :n].reshape(-1)).reshape(n, PD), q)
                if wire == "int8":
                    rl, _ = spref.dequant(q.reshape(-1), n, np.zeros(4, np.int8))
                    assert float(np.abs(rl.reshape(n, PD) - rows[:n]).max()) < 1e-6
        da = o["desc"][f, :n]
        for name, (q_, t_, d_) in (("d2fe_match_knn", fe.match_knn(da, rows[:n], RATIO)), ("oracle", orc.match_knn(da, rows[:n], RATIO))):
            k = int(r["mn"][f])
            assert k == len(q_) and np.array_equal(r["mq"][f, :k], q_) and np.array_equal(r["mt"][f, :k], t_) and np.array_equal(_bits(r["md"][f, :k]), _bits(d_)), (name, f)
        if wire == "fp32":                                              # a frame against itself
            assert int(r["mn"][f]) == n and np.array_equal(r["mq"][f, :n], np.arange(n)) and not r["md"][f, :n].any()
        elif wire == "int8-renorm256":
            assert int(r["mn"][f]) > 0.5 * n
        s = float(o["netvlad"][f] @ blk[off["netvlad"]:off["netvlad"] + G])
        assert abs(float(r["sims"][f]) - s) < 1e-5 and int(r["gate_pass"][f]) == 1
    assert r["gate_n"] == F
    x.close(); pipe.close(); fe.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode,wire", [("all2all", "fp32"), ("gated", "int8-renorm256"), ("gated", "int8")])
def test_quad_exchange_at_64_floats_gpu(orc, mode, wire):
    """loopback: the gathered blocks byte-equal to the hand-composed pack (and decode) of the _d functions, the gate on the blocks' NetVLAD fields, every match
    list equal to d2fe_match_knn and the oracle on the blocks' rows, the gated pairs in trackRemoteFrames' order"""
    import torch
    from d2slam_amd import api
    from tests.helpers import quad_exchange_common as qc
    dev = torch.device("cuda", 0)
    fe = _quad_fe(4)
    G = fe.netvlad_dim
    pipe = qc.quad_pipe(fe, 2, 1)
    tk = pipe.submit(qc.rig(0, 1))
    o = _copy(pipe.wait(tk))
    BLK, BLKB = api.block_words(CAP, G, PD), api.block_bytes_int8(CAP, G, PD)
    off = {k: api.block_field_offset(CAP, G, k, PD) for k in ("desc", "netvlad", "n")}
    # the blocks by hand
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    desc, kps, sc, n_kp, nv = t(o["desc"].reshape(4, CAP, PD)), t(o["kps_xy"].reshape(4, CAP, 2)), t(o["scores"].reshape(4, CAP)), t(o["n_kp"].reshape(4)), t(o["netvlad"].reshape(4, G))
    f32 = torch.zeros((4, BLK), dtype=torch.float32, device=dev); q8 = torch.zeros((4, BLKB), dtype=torch.int8, device=dev)
    torch.cuda.synchronize()
    if wire == "fp32":
        fe.pack_blocks_device(desc.data_ptr(), kps.data_ptr(), sc.data_ptr(), n_kp.data_ptr(), nv.data_ptr(), 0, 1, 4, CAP, G, f32.data_ptr(), desc_dim=PD)
    else:
        fe.pack_blocks_int8_device(desc.data_ptr(), kps.data_ptr(), n_kp.data_ptr(), nv.data_ptr(), 0, 1, 4, CAP, G, q8.data_ptr(), desc_dim=PD)
        fe.unpack_blocks_int8_device(q8.data_ptr(), 4, CAP, G, f32.data_ptr(), renorm=1 if wire == "int8-renorm256" else 0, desc_dim=PD)
    fe.sync(); torch.cuda.synchronize()
    gath = f32.cpu().numpy()
    wire_h = gath.view(np.uint8).reshape(-1) if wire == "fp32" else q8.cpu().numpy().view(np.uint8).reshape(-1)
    sims = np.array([float(o["netvlad"][0, (2 + j) % 4] @ gath[2][off["netvlad"]:off["netvlad"] + G]) for j in range(4)])
    thres = qc.halfway_threshold(sims[None])
    x = api.QuadExchange(pipe, comm=None, world=1, rank=0, wire=wire, mode=mode, loopback=True, slots=2, gate_thres=thres, all_gather=_copy_cb())
    assert x.block_bytes == (4 * BLK if wire == "fp32" else BLKB)
    x.enqueue(tk, 0)
    r = x.collect(0)
    d_f32, d_wire = x.gathered(0)
    assert np.array_equal(qc.d2h(d_wire, wire_h.size), wire_h), "the gathered blocks differ from the hand-composed pack"
    assert np.array_equal(qc.d2h(d_f32, gath.nbytes), gath.view(np.uint8).reshape(-1)), "the decoded blocks differ from d2fe_unpack_blocks_int8_device_d"
    assert float(np.abs(r["sims"][0] - sims).max()) < 1e-5
    db = int(r["dir_prev"][0])
    assert db == 2 and r["gate_n"] == 1                                   # the rig against itself: view 2 meets view 2
    pairs = [((db - 2 + (2 + k) % 4 + 4) % 4, (2 + k) % 4) for k in range(4)] if mode == "gated" else [(lv, rv) for lv in range(4) for rv in range(4)]
    assert r["npairs"] == len(pairs)
    total = 0
    for p, (lv, rv) in enumerate(pairs):
        assert (int(r["local_view"][p]), int(r["remote_view"][p])) == (lv, rv)
        na, nb = int(o["n_kp"][0, lv]), int(gath[rv].view(np.int32)[off["n"]])
        assert na >= 20 and nb == int(o["n_kp"][0, rv])
        da, dbk = o["desc"][0, lv, :na], gath[rv][:nb * PD].reshape(nb, PD)
        k = int(r["mn"][p])
        for name, (q_, t_, d_) in (("d2fe_match_knn", fe.match_knn(da, dbk, RATIO)), ("oracle", orc.match_knn(da, dbk, RATIO))):
            assert k == len(q_) and np.array_equal(r["mq"][p, :k], q_) and np.array_equal(r["mt"][p, :k], t_) and np.array_equal(_bits(r["md"][p, :k]), _bits(d_)), (name, p)
        total += k if lv == rv else 0
    assert wire == "int8" or total >= 8
    x.close(); pipe.close(); fe.close()


@pytest.mark.gpu
def test_exchange_refuses_a_width_the_matcher_cannot_read_in_place_gpu():
    """68 floats, capacity 50: the 3584-word blocks do not start on a row of 68 -- refused at create, with the reason"""
    from d2slam_amd import api
    cap = 50
    fe = _fe(2, pd=68, max_keypoints=cap)
    pipe = api.StereoPipe(fe, lanes=1, frames=1, width=W, height=H, cap=cap, netvlad=False)
    assert api.block_words(cap, 0, 68) % 68 != 0
    with pytest.raises(api.D2FEError, match="do not start on a descriptor row") as e:
        api.Exchange(pipe, comm=None, world=1, loopback=True, all_gather=_copy_cb())
    assert e.value.code == -5
    o = pipe.wait(pipe.submit(*[im[None] for im in _images(2)]))       # the pipe itself carries 68-float rows
    assert o["desc"].shape == (2, cap, 68) and int(o["n_kp"][0]) > 10 and int(o["lr_n"][0]) > 0
    pipe.close(); fe.close()


# ---- 6. loop query and keyframe window ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_loop_query_behind_a_64d_pipe_equals_the_host_composition_gpu():
    from d2slam_amd import api
    from tests import test_loop_query as tl
    assert (tl.H, tl.W, tl.CAP) == (H, W, CAP)
    lanes, F, MI = 2, 2, 2
    fe = _fe(2 * F, netvlad=True)
    G = fe.netvlad_dim
    fr = tl._stereo_frames()
    N = len(fr)
    submits = [(np.stack([fr[i * F + k][0] for k in range(F)]), np.stack([fr[i * F + k][1] for k in range(F)])) for i in range(N // F)]
    masks = [np.array(tl.STEREO_KEY[i * F:(i + 1) * F], np.uint8) for i in range(N // F)]
    flags = [api.LOOP_QUERY | api.LOOP_ADD] * len(submits)
    pipe = api.StereoPipe(fe, lanes=lanes, frames=F, width=W, height=H, cap=CAP, netvlad=True)
    alone, _ = tl._drive(api, pipe, submits)
    pipe.close()
    assert alone[0]["desc"].shape[-1] == PD
    per_frame = [(o["netvlad"][k][None], o["desc"][k][None], o["n_kp"][k:k + 1]) for o in alone for k in range(F)]
    fl_frame = [(flags[i] if masks[i][k] else 0) for i in range(len(submits)) for k in range(F)]
    comp = tl._compose(api, fe, per_frame, fl_frame, 1, 0, MI, 0, G)
    best = [float(c["sim"]) for c in comp if c["label"] >= 0]
    thres = float(np.median(best))
    pipe = api.StereoPipe(fe, lanes=lanes, frames=F, width=W, height=H, cap=CAP, netvlad=True)
    loop = api.LoopQuery(pipe, capacity_keyframes=N, max_index=MI, thres=thres, ratio=RATIO, mode=0, slots=lanes + 1)
    _, col = tl._drive(api, pipe, submits, loop, masks, flags)
    passed = matched = 0
    for i, c in enumerate(col):
        for k in range(F):
            hit = tl._check_frame(c, k, comp[i * F + k], thres, 1)
            passed += hit
            matched += int(c["n_match"][k].sum()) if hit else 0
    assert passed >= 1 and matched >= 1
    loop.close(); pipe.close(); fe.close()


@pytest.mark.gpu
def test_keyframe_window_behind_a_64d_pipe_equals_the_host_composition_gpu():
    """the window fed from a 64-float pipe; remote frames read in place in the lane's result block and in the gathered 64-float blocks of a loopback exchange"""
    from d2slam_amd import api
    from tests import test_keyframe_window as tw
    from tests.helpers import keyframe_window_common as kw, quad_exchange_common as qc
    assert tw.CAP == CAP
    F, NK = 2, 2
    fe = _fe(2 * F, netvlad=True)
    G = fe.netvlad_dim
    subs = tw._submits(1)[:4]
    pipe = api.StereoPipe(fe, lanes=2, frames=F, width=W, height=H, cap=CAP, netvlad=True)
    alone = [_copy(pipe.wait(pipe.submit(*s))) for s in subs]
    kf = [f for o in alone[:NK] for f in tw._frames_of(o, 1)]
    tags = [10 + 7 * i for i in range(len(kf))]
    w = tw._stack(kf)
    assert w[1].shape == (NK * F, 1, CAP, PD)
    rem_all = tw._stack([f for o in alone[NK:] for f in tw._frames_of(o, 1)])
    best = np.sort(kw.sims64(rem_all[0], w[0], 1).reshape(len(rem_all[0]), -1).max(axis=1))
    g = int(np.argmax(np.diff(best)))
    thres = float(0.5 * (best[g] + best[g + 1]))
    win = api.KeyframeWindow(pipe, capacity=NK * F, thres=thres, ratio=RATIO, slots=3, max_queries=F)
    assert win.desc_dim == PD
    hits = 0
    for i, s in enumerate(subs):
        t = pipe.submit(*s)
        if i < NK:
            for k in range(F):
                win.push(t, k, tags[i * F + k])
            pipe.wait(t)
            continue
        v = pipe.device_view(t, win.stream)                         # in place, in the lane's result block: rows of 64 floats
        win.track_device(v.d_netvlad, G, v.d_desc, CAP * PD, v.d_n_kp, 1, F, 0, None)
        pipe.device_release(t, win.stream)
        o = _copy(pipe.wait(t))
        r = tw._copy(win.collect(0))
        rem = tw._stack(tw._frames_of(o, 1))
        sims, recs = tw._compose(api, fe, w, rem, thres, 0)
        hits += tw._check(r, sims, recs, tags, 1)[0]
    # gathered 64-float blocks, read in place: ticket 1's frames are the newest keyframes of the window themselves -- the last one meets itself first
    BLK = api.block_words(CAP, G, PD)
    off = {k: api.block_field_offset(CAP, G, k, PD) for k in ("desc", "netvlad", "n")}
    x = api.Exchange(pipe, world=1, loopback=True, wire="fp32", slots=2, own_stream=True, all_gather=_copy_cb())
    t = pipe.submit(*subs[1])
    x.enqueue(t, 1)
    assert win.track_exchange(x, 1, 2) == F
    pipe.wait(t); x.collect(1)
    r = tw._copy(win.collect(2))
    blocks = qc.d2h(x.gathered(1)[0], 4 * BLK * F).view(np.float32).reshape(F, 1, BLK)
    rem = (blocks[:, :, off["netvlad"]:off["netvlad"] + G].copy(), blocks[:, :, :CAP * PD].reshape(F, 1, CAP, PD).copy(), blocks[:, :, off["n"]].copy().view(np.int32))
    sims, recs = tw._compose(api, fe, w, rem, thres, 0)
    h, _ = tw._check(r, sims, recs, tags, 1)
    assert h >= 1 and int(r["n_match"].sum()) > 10
    x.close(); win.close(); pipe.close(); fe.close()
