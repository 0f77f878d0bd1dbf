"""exact_order (include/d2fe.h, d2fe_config::exact_order; csrc/exact_order.hip): the keypoint list of a D2FE_PREC_F32_WINO handle with the option on must equal,
position by position, the list a D2FE_PREC_F32 handle produces on the same images with the same weights -- count, kps_idx, kps_xy, order.  The reference of
every comparison here is the exact mode, never the mode under test."""
import ctypes as C

import numpy as np
import pytest

from d2slam_amd.synth import synth_stereo

THR = 0.015


def _imgs(H, W, n, seed0):
    return np.ascontiguousarray(np.stack([synth_stereo(H, W, seed=seed0 + i // 2)[i & 1] for i in range(n)]))


def _fe(api, w, H, W, n, N, prec, **eo):
    fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=N, input_width=W, input_height=H, max_batch=n, precision=prec, keypoint_threshold=THR), **eo)
    fe.load_superpoint(w)
    return fe


def _device(fe, imgs, cap):
    """d2fe_superpoint_extract_device: per image (kps_xy, scores, desc, kps_idx)"""
    import torch
    dev = torch.device("cuda", 0)
    n, H, W = imgs.shape
    g = torch.from_numpy(imgs).to(dev)
    kps = torch.zeros((n, cap, 2), dtype=torch.float32, device=dev); sc = torch.zeros((n, cap), dtype=torch.float32, device=dev)
    desc = torch.zeros((n, cap, 256), dtype=torch.float32, device=dev); idx = torch.zeros((n, cap), dtype=torch.int32, device=dev)
    cnt = torch.zeros(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    fe.extract_device(g.data_ptr(), n, W, H, kps.data_ptr(), sc.data_ptr(), desc.data_ptr(), idx.data_ptr(), cap, cnt.data_ptr())
    fe.sync()
    c = cnt.cpu().numpy()
    return [(kps[i, :c[i]].cpu().numpy(), sc[i, :c[i]].cpu().numpy(), desc[i, :c[i]].cpu().numpy(), idx[i, :c[i]].cpu().numpy()) for i in range(n)]


def _same_list(a, b, what, scores=True):
    assert len(a[0]) == len(b[0]), "%s: %d keypoints against the exact mode's %d" % (what, len(a[0]), len(b[0]))
    np.testing.assert_array_equal(a[0], b[0], err_msg=what + " kps_xy")
    if scores:
        np.testing.assert_array_equal(a[1], b[1], err_msg=what + " scores")
    if len(a) > 3 and len(b) > 3:
        np.testing.assert_array_equal(a[3], b[3], err_msg=what + " kps_idx")


SIZES = [(96, 104), (88, 88), (120, 160)]      # H, W: all four edges, corners and interior cells (x0 in {0, 8, 16}, y0 in {0, 8}); the crop that is the image; and more
                                               # keys than the in-LDS sort takes (eps = 1 makes every pixel inside the borders a candidate: 19 200 > 16 384)


@pytest.fixture(scope="module")
def exact_lists(sp_weights):
    """the exact mode's lists of the small inputs, computed once: {(H, W): (images, per-image (kps, scores, desc, idx))}"""
    from d2slam_amd import api
    out = {}
    for H, W in SIZES:
        imgs = _imgs(H, W, 2, 70 + H)
        fe = _fe(api, sp_weights, H, W, 2, 50, api.PREC_F32)
        out[(H, W)] = (imgs, _device(fe, imgs, 50))
        fe.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", SIZES)
def test_everything_re_evaluated_is_the_exact_mode_bit_for_bit(sp_weights, exact_lists, H, W):
    from d2slam_amd import api
    imgs, ref = exact_lists[(H, W)]
    cells = (H // 8) * (W // 8)
    fe = _fe(api, sp_weights, H, W, 2, 50, api.PREC_F32_WINO, exact_order=True, exact_order_eps=1.0, exact_order_crops=2 * cells)
    got = _device(fe, imgs, 50)
    host = fe.extract_batch(imgs, cap=50)
    st = fe.exact_order_stats()
    fe.close()
    assert min(len(r[0]) for r in ref) == 50                     # sorted top-K lists: the order is the score order
    for i in range(2):
        _same_list(got[i], ref[i], "%dx%d image %d (device call)" % (W, H, i))
        _same_list(host[i], ref[i], "%dx%d image %d (host call)" % (W, H, i))
    assert st["dropped"] == 0 and st["calls"] == 2 and st["cells"] == 2 * 2 * cells, st
    assert st["marked"] == 2 * 2 * (H - 2) * (W - 2), st        # every pixel inside the borders, both calls


@pytest.mark.gpu
def test_plain_winograd_differs_in_bits_on_these_inputs(sp_weights, exact_lists):
    """what the test above would see without the option: the Winograd scores are other bits"""
    from d2slam_amd import api
    imgs, ref = exact_lists[(96, 104)]
    fe = _fe(api, sp_weights, 96, 104, 2, 50, api.PREC_F32_WINO)
    got = fe.extract_batch(imgs, cap=50)
    fe.close()
    assert any(len(g[1]) != len(r[1]) or not np.array_equal(g[1], r[1]) for g, r in zip(got, ref))


# 16 seeded 640x480 images (synth_stereo seed, side): chosen with tools/exact_order_study.py so that the plain Winograd mode lists several of them in another order
NEAR_TIE_SET = [(5007, 0), (5007, 1), (5010, 0), (5010, 1), (5012, 0), (5012, 1), (5026, 0), (5026, 1),
                (5030, 0), (5030, 1), (5034, 0), (5034, 1), (5036, 0), (5036, 1), (5037, 0), (5037, 1)]


@pytest.mark.gpu
def test_natural_near_ties(sp_weights):
    from d2slam_amd import api
    H, W, N = 480, 640, 200
    imgs = np.ascontiguousarray(np.stack([synth_stereo(H, W, seed=s)[side] for s, side in NEAR_TIE_SET]))
    lists = {}
    for name, prec, eo in (("f32", api.PREC_F32, {}), ("wino", api.PREC_F32_WINO, {}), ("exact_order", api.PREC_F32_WINO, {"exact_order": True})):
        fe = _fe(api, sp_weights, H, W, 16, N, prec, **eo)
        lists[name] = _device(fe, imgs, N)
        st = fe.exact_order_stats()
        fe.close()
    differ = [i for i in range(16) if len(lists["wino"][i][3]) != len(lists["f32"][i][3]) or not np.array_equal(lists["wino"][i][3], lists["f32"][i][3])]
    print("plain Winograd lists differ from the exact mode's in images", differ, "exact_order stats", st)
    assert len(differ) >= 2, "precondition: the set must hold at least two images the plain Winograd mode lists differently (found %s)" % differ
    for i in range(16):
        _same_list(lists["exact_order"][i], lists["f32"][i], "image %d" % i, scores=False)
    assert st["dropped"] == 0 and st["calls"] == 1, st


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", SIZES)
def test_slot_starvation(sp_weights, exact_lists, H, W):
    from d2slam_amd import api
    imgs, ref = exact_lists[(H, W)]
    plain = _fe(api, sp_weights, H, W, 2, 50, api.PREC_F32_WINO)
    wl = _device(plain, imgs, 50)
    plain.close()
    fe = _fe(api, sp_weights, H, W, 2, 50, api.PREC_F32_WINO, exact_order=True, exact_order_eps=1.0, exact_order_crops=1)
    a = _device(fe, imgs, 50)
    b = _device(fe, imgs, 50)
    st = fe.exact_order_stats()
    fe.close()
    assert st["dropped"] > 0 and st["cells"] == 2 and st["calls"] == 2, st
    for i in range(2):
        for x, y in zip(a[i], b[i]):
            np.testing.assert_array_equal(x, y)                  # two calls, identical bits
        kps, sc, desc, idx = a[i]
        assert len(idx) <= 50 and len(np.unique(idx)) == len(idx)
        assert np.array_equal(idx, kps[:, 1].astype(np.int64) * W + kps[:, 0].astype(np.int64))
        assert kps[:, 0].min() >= 1 and kps[:, 0].max() < W - 1 and kps[:, 1].min() >= 1 and kps[:, 1].max() < H - 1
        assert (sc > np.float32(THR)).all()
    # the one slot goes to the first marked cell of image 0: the cell of the strongest Winograd candidate (list order), or cell 0 when the candidates
    # outnumber the in-LDS sort (cell order).  Its keypoints carry the exact mode's score bits; image 1 got nothing and equals the plain Winograd list
    Wc = W // 8
    first = 0 if (H - 2) * (W - 2) > 16384 else int(wl[0][3][0]) // W // 8 * Wc + int(wl[0][3][0]) % W // 8
    kps, sc, desc, idx = a[0]
    exact = dict(zip(ref[0][3].tolist(), ref[0][1].tolist()))
    in_cell = [j for j in range(len(idx)) if int(idx[j]) // W // 8 * Wc + int(idx[j]) % W // 8 == first]
    if (H - 2) * (W - 2) <= 16384:
        assert in_cell and int(idx[in_cell[0]]) in exact
    for j in in_cell:
        if int(idx[j]) in exact:
            assert np.float32(exact[int(idx[j])]) == sc[j]
    for x, y in zip(a[1], wl[1]):
        np.testing.assert_array_equal(x, y)


@pytest.mark.gpu
def test_every_entry_point_gives_the_same_bits(sp_weights):
    """a few 160x120 stereo frames, an eps large enough to keep the path busy: the stereo pipe at 1 and 4 frames per submit on 1 and 4 lanes and the three
    extract calls all deliver the exact mode's lists"""
    from d2slam_amd import api
    H, W, N, F = 120, 160, 30, 8
    eo = dict(exact_order=True, exact_order_eps=2e-4, exact_order_crops=256)
    left = _imgs(H, W, 2 * F, 300)[0::2]; right = _imgs(H, W, 2 * F, 300)[1::2]
    allimgs = np.ascontiguousarray(np.concatenate([left, right]))
    f32 = _fe(api, sp_weights, H, W, 2 * F, N, api.PREC_F32)
    ref = _device(f32, allimgs, N)
    f32.close()
    fe = _fe(api, sp_weights, H, W, 2 * F, N, api.PREC_F32_WINO, **eo)
    dev = _device(fe, allimgs, N)
    batch = fe.extract_batch(allimgs, cap=N)
    kps = np.zeros((N, 2), np.float32); sc = np.zeros(N, np.float32); desc = np.zeros((N, 256), np.float32); k = C.c_int(0)
    for i in (0, F + 1):
        rc = fe._lib.d2fe_superpoint_extract(fe.handle, allimgs[i].ctypes.data, W, H, W, kps.ctypes.data, sc.ctypes.data, desc.ctypes.data, N, C.byref(k))
        assert rc == 0
        _same_list((kps[:k.value], sc[:k.value]), ref[i], "single call, image %d" % i, scores=False)
        np.testing.assert_array_equal(sc[:k.value], dev[i][1]); np.testing.assert_array_equal(desc[:k.value], dev[i][2])
    for i in range(2 * F):
        _same_list(dev[i], ref[i], "device call, image %d" % i, scores=False)
        for x, y in zip(batch[i], dev[i]):
            np.testing.assert_array_equal(x, y)                  # the host-pointer batch call: the device call's bits, descriptors included
    busy = fe.exact_order_stats()
    assert busy["cells"] > 0 and busy["dropped"] == 0, busy
    for lanes, frames in ((1, 1), (4, 1), (1, 4), (4, 4)):
        pipe = api.StereoPipe(fe, lanes=lanes, frames=frames, width=W, height=H, cap=N, netvlad=False)
        pending = []

        def check(t, f0):
            o = pipe.wait(t)
            for f in range(frames):
                for side, row in ((0, f), (1, frames + f)):
                    n = int(o["n_kp"][row]); i = side * F + f0 + f
                    what = "stereo pipe %d lanes x %d frames, frame %d side %d" % (lanes, frames, f0 + f, side)
                    _same_list((o["kps_xy"][row, :n], o["scores"][row, :n]), ref[i], what, scores=False)
                    np.testing.assert_array_equal(o["scores"][row, :n], dev[i][1], err_msg=what)
        for f0 in range(0, F, frames):
            pending.append((pipe.submit(left[f0:f0 + frames], right[f0:f0 + frames]), f0))
            if len(pending) == lanes:                            # `lanes` submits in flight
                check(*pending.pop(0))
        for p in pending:
            check(*p)
        pipe.close()
    st = fe.exact_order_stats()
    fe.close()
    assert st["dropped"] == 0 and st["cells"] > busy["cells"] and st["calls"] > busy["calls"], st      # the lanes count into the parent's buffer


@pytest.mark.gpu
def test_quad_pipe_gives_the_exact_modes_lists(sp_weights):
    from d2slam_amd import api, quadcam
    from d2slam_amd.synth import synth_image
    RH, RW, UH, UW, N = 240, 384, 120, 192, 30
    maps = [quadcam.synthetic_maps(c, RH, RW, UH, UW) for c in range(4)]
    raw = np.stack([np.stack([synth_image(RH, RW, 900 + 4 * q + c) for c in range(4)]) for q in range(4)])
    outs = {}
    for name, prec, eo in (("f32", api.PREC_F32, {}), ("eo", api.PREC_F32_WINO, dict(exact_order=True, exact_order_eps=2e-4, exact_order_crops=256))):
        fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=N, input_width=UW, input_height=UH, max_batch=16, precision=prec, keypoint_threshold=THR), **eo)
        fe.load_superpoint(sp_weights)
        res = []
        for lanes, quads in ((1, 1), (4, 1), (1, 4), (4, 4)) if name == "eo" else ((1, 1),):
            pipe = api.QuadPipe(fe, maps, lanes=lanes, quads=quads, raw_width=RW, raw_height=RH, width=UW, height=UH, cap=N, netvlad=False, match_neighbour=False,
                                match_prev=False)
            got, pending = [], []

            def collect(t):
                o = pipe.wait(t)
                for q in range(quads):
                    got.append([(o["kps_xy"][q, v, :int(o["n_kp"][q, v])].copy(), o["scores"][q, v, :int(o["n_kp"][q, v])].copy()) for v in range(4)])
            for q0 in range(0, 4, quads):
                pending.append(pipe.submit(raw[q0:q0 + quads]))
                if len(pending) == lanes:
                    collect(pending.pop(0))
            for t in pending:
                collect(t)
            res.append(got)
            pipe.close()
        st = fe.exact_order_stats()
        fe.close()
        outs[name] = res
    assert st["cells"] > 0 and st["dropped"] == 0, st
    for got in outs["eo"]:
        for q in range(4):
            for v in range(4):
                _same_list(got[q][v], outs["f32"][0][q][v], "quad frame %d view %d" % (q, v), scores=False)
                np.testing.assert_array_equal(got[q][v][1], outs["eo"][0][q][v][1])      # and the same score bits whatever the lanes and quads per submit


@pytest.mark.gpu
def test_refusals_and_the_old_struct_size(sp_weights):
    from d2slam_amd import api
    lib = api.load_library()
    lib.d2fe_last_error.restype = C.c_char_p

    def create(**kw):
        c = api._Config()
        lib.d2fe_default_config(C.byref(c))
        c.max_width, c.max_height, c.max_batch, c.max_keypoints, c.precision, c.exact_order = 160, 120, 2, 50, api.PREC_F32_WINO, 1
        for k, v in kw.items():
            setattr(c, k, v)
        h = C.c_void_p()
        return lib.d2fe_create(C.byref(c), C.byref(h)), h, lib.d2fe_last_error()
    for kw, word in ((dict(precision=api.PREC_F32), b"D2FE_PREC_F32_WINO"), (dict(precision=api.PREC_F16X2), b"D2FE_PREC_F32_WINO"),
                     (dict(postproc=api.POSTPROC_A), b"variant B"), (dict(max_keypoints=-1), b"max_keypoints"), (dict(exact_order_eps=-1e-6), b"exact_order_eps"),
                     (dict(exact_order_eps=float("nan")), b"exact_order_eps"), (dict(exact_order_eps=float("inf")), b"exact_order_eps")):
        rc, h, msg = create(**kw)
        assert rc == -1 and not h.value and word in msg, (kw, rc, msg)
    # image sizes: at least 88x88, multiples of 8
    fe = _fe(api, sp_weights, 120, 160, 2, 50, api.PREC_F32_WINO, exact_order=True)
    for H, W in ((80, 160), (120, 80), (100, 104), (96, 100)):
        with pytest.raises(api.D2FEError) as e:
            fe.extract_batch(np.zeros((1, H, W), np.uint8), cap=50)
        assert e.value.code == -1 and "exact_order" in str(e.value)
    fe.close()
    # the struct of a caller that does not know the fields: whatever lies behind its struct_size is not read, the handle is a plain Winograd one
    imgs = _imgs(120, 160, 2, 40)
    plain = _fe(api, sp_weights, 120, 160, 2, 50, api.PREC_F32_WINO)
    want = plain.extract_batch(imgs, cap=50)
    assert plain.exact_order_stats() == dict(marked=0, cells=0, dropped=0, calls=0)      # option off: zeros
    plain.close()
    rc, h, msg = create(struct_size=api._Config.exact_order.offset, exact_order_eps=float("nan"))
    assert rc == 0 and h.value, msg
    old = api.FrontEnd.__new__(api.FrontEnd)
    old._lib, old._h, old.dev, old._keep = lib, h, False, None
    old.cfg = api.SuperPointConfig(max_keypoints=50, input_width=160, input_height=120, max_batch=2, precision=api.PREC_F32_WINO)
    old.load_superpoint(sp_weights)
    got = old.extract_batch(imgs, cap=50)
    assert old.exact_order_stats() == dict(marked=0, cells=0, dropped=0, calls=0)
    old.close()
    for g, w in zip(got, want):
        for x, y in zip(g, w):
            np.testing.assert_array_equal(x, y)
    rc, h, msg = create(struct_size=api._Config.exact_order.offset - 4)
    assert rc == -1 and b"size mismatch" in msg
