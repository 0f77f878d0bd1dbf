"""The launch regimes of the benchmark's headline configuration (640 x 480 stereo, 32 stereo frames per submit: 64 images per pass, 64 descriptor pairs per
matcher launch, Winograd fp32) against the oracle.

Several launchers switch to another code path once a launch is large: the persistent Winograd kernels CLAIM their work items from a device counter instead
of striding through them (conv_wino.hip; at 640 x 480 from 11 images on for conv1b and from 41 on for conv2a / conv2b), and the matcher runs two-wave
workgroups once the launch no longer fits the device at once (match.hip; 64 pairs of 200 rows, or one pair beyond 8192 rows).  Every other GPU test stays
below those sizes.  Each test here PROVES the path it means to cover from the development library's launch-regime record (d2fe_debug_regime_counts,
include/d2fe_debug.h: counted by the launchers, the claim rule being the one function the kernel itself evaluates) and compares the results with the
oracle bit for bit, or at a bar that already exists in tests/test_wino.py / tests/test_gpu_parity.py.

A claimed walk makes the item -> workgroup mapping depend on timing, and activations persist in HBM between calls: a skipped tile would silently keep the
previous call's values.  So every call under test is preceded by a call on OTHER images."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from d2slam_amd.synth import synth_descriptor_pair, synth_stereo
from tests.helpers.match_ref import match_batch as _match_batch      # ONE d2fe_match_batch_device launch of a list of pairs (shared with tests/test_match_edges.py)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Hb, Wb, CAP, NIMG = 480, 640, 200, 64
SEEDS = {"A": range(5000, 5032), "B": range(5100, 5132), "C": range(5200, 5232), "D": range(5300, 5332), "E": range(5400, 5432)}


@pytest.fixture(scope="module")
def api():
    from d2slam_amd import api as a
    a.load_library(dev=True)
    return a


def _show(what, rec):
    print("\n[launch regimes] %s: %s" % (what, json.dumps(rec)), flush=True)


class _Headline:
    """frames and oracle results of the 64-image sets, computed once per module and on demand (the oracle is ~0.7 s per 640 x 480 forward pass)"""

    def __init__(self, orc, w):
        self.orc, self.w = orc, w
        self._frames, self._wino, self._direct = {}, {}, {}

    def frames(self, key):
        """[64, H, W] u8: the 32 left frames of the set, then the 32 right frames"""
        if key not in self._frames:
            pairs = [synth_stereo(Hb, Wb, s) for s in SEEDS[key]]
            self._frames[key] = np.stack([l for l, _ in pairs] + [r for _, r in pairs])
        return self._frames[key]

    def _forward(self, key, wino):
        keep_maps = key == "A"      # the set whose score and descriptor maps are compared as well
        out = []
        for img in self.frames(key):
            f = self.orc.superpoint_forward(img, self.w, wino=wino)
            kps, sc, idx = self.orc.select_b(f["semi"], 0.015, 1, CAP)
            r = {"kps": kps, "sc": sc, "idx": idx, "desc": self.orc.sample_b(f["desc"], kps)}
            if keep_maps:
                r["semi"] = f["semi"]
                if wino:
                    r["desc_raw"] = f["desc_raw"]
            out.append(r)
        return out

    def wino(self, key):
        """per image: the Winograd oracle's keypoints, scores, sampled descriptors (set A: and its semi / desc_raw maps)"""
        if key not in self._wino:
            self._wino[key] = self._forward(key, True)
        return self._wino[key]

    def direct(self, key):
        """per image: the direct-convolution oracle's semi map, keypoints, scores, indices, sampled descriptors"""
        if key not in self._direct:
            self._direct[key] = self._forward(key, False)
        return self._direct[key]


@pytest.fixture(scope="module")
def headline(orc, sp_weights):
    return _Headline(orc, sp_weights)


def _cfg(api, prec, **kw):
    return api.SuperPointConfig(max_keypoints=CAP, input_width=Wb, input_height=Hb, max_batch=NIMG, precision=prec, **kw)


def _assert_same_results(got, want, what):
    assert len(got) == len(want)
    for i, ((k0, s0, d0), (k1, s1, d1)) in enumerate(zip(got, want)):
        assert np.array_equal(k0, k1) and np.array_equal(s0, s1) and np.array_equal(d0, d1), "%s: image %d differs" % (what, i)


# ---- (a) the headline pass against the oracle ------------------------------------------------------------------------------------------------------------

def test_headline_pass_wino_against_the_oracle(api, sp_weights, headline):
    """64 images of 640 x 480 in ONE Winograd-mode call in the product configuration (sparse descriptor head, no score map), after a call on 64 other
    images: keypoints and scores bitwise equal to the Winograd oracle's, descriptors within the sparse-head bar of tests/test_wino.py (1e-5); every image
    bitwise equal to the same image through a 1-image call (static walk); the product library gives the bits of the development library; and the
    record shows that the fused conv1b kernel and a ring kernel took the claimed walk in the call under test."""
    imgs, other, ref = headline.frames("A"), headline.frames("B"), headline.wino("A")
    fe = api.DevFrontEnd(_cfg(api, api.PREC_F32_WINO))
    fe.load_superpoint(sp_weights)
    fe.extract_batch(other, cap=CAP)                   # every activation buffer now holds foreign data
    api.DevFrontEnd.regime_reset()
    res = fe.extract_batch(imgs, cap=CAP)
    rec = api.DevFrontEnd.regime_counts()
    _show("(a) 64-image Winograd call, sparse head", rec)
    singles = [fe.extract_batch(imgs[i:i + 1], cap=CAP)[0] for i in range(NIMG)]
    fe.close()
    prod = api.FrontEnd(_cfg(api, api.PREC_F32_WINO))
    prod.load_superpoint(sp_weights)
    prod.extract_batch(other, cap=CAP)
    res_prod = prod.extract_batch(imgs, cap=CAP)
    prod.close()
    for i in range(NIMG):
        kps, sc, desc = res[i]
        assert len(kps) == CAP, "image %d: %d keypoints" % (i, len(kps))
        assert np.array_equal(kps, ref[i]["kps"]) and np.array_equal(sc, ref[i]["sc"]), "image %d: keypoints / scores differ from the Winograd oracle" % i
        err = float(np.abs(desc - ref[i]["desc"]).max())
        assert err <= 1e-5, "image %d: descriptors off by %g" % (i, err)
    _assert_same_results(res, singles, "64-image call vs 1-image calls")
    _assert_same_results(res_prod, res, "product library vs development library")
    assert rec["wino_nt2_claimed_fused1b"] >= 1, "the fused conv1b kernel did not take the claimed walk: %s" % rec
    assert rec["wino_nt2_claimed_ring"] >= 1, "no ring kernel took the claimed walk: %s" % rec


def test_headline_pass_wino_dense_maps_against_both_oracles(api, orc, sp_weights, headline):
    """The same call on a handle that keeps the score map and the dense descriptor map: semi and desc_raw of all 64 images bitwise equal to the Winograd
    oracle's, and the bars of test_wino_extract_vs_oracles against the direct-convolution oracle (semi <= 3e-6, keypoints exact up to score near-ties,
    descriptors of shared keypoints 1e-5)."""
    imgs, other = headline.frames("A"), headline.frames("B")
    fw, fd = headline.wino("A"), headline.direct("A")
    fe = api.DevFrontEnd(_cfg(api, api.PREC_F32_WINO, keep_score_map=True, dense_descriptors=True))
    fe.load_superpoint(sp_weights)
    fe.extract_batch(other, cap=CAP)
    api.DevFrontEnd.regime_reset()
    res = fe.extract_batch(imgs, cap=CAP)
    rec = api.DevFrontEnd.regime_counts()
    _show("(a) 64-image Winograd call, dense maps", rec)
    semi = fe.debug_read("semi", (NIMG, Hb, Wb))
    draw = fe.debug_read("desc_raw", (NIMG, Hb // 8, Wb // 8, 256))
    fe.close()
    for i in range(NIMG):
        # bit for bit against the restatement of the mode's evaluation order
        assert np.array_equal(semi[i], fw[i]["semi"]), "image %d: semi differs in %d pixels" % (i, int((semi[i] != fw[i]["semi"]).sum()))
        assert np.array_equal(draw[i], fw[i]["desc_raw"]), "image %d: desc_raw differs in %d cells" % (i, int((draw[i] != fw[i]["desc_raw"]).any(axis=2).sum()))
        kps, sc, desc = res[i]
        assert np.array_equal(kps, fw[i]["kps"]) and np.array_equal(sc, fw[i]["sc"])
        assert np.abs(desc - fw[i]["desc"]).max() <= 1e-6
        # the bars against the direct-convolution oracle, as in tests/test_wino.py
        eps = float(np.abs(fd[i]["semi"] - fw[i]["semi"]).max())
        assert eps <= 3e-6
        dk, ds, di = fd[i]["kps"], fd[i]["sc"], fd[i]["idx"]
        gi = (kps[:, 1] * Wb + kps[:, 0]).astype(np.int64)
        flat = fd[i]["semi"].reshape(-1)
        kth = ds[-1] if len(ds) == CAP else 0.015
        for j in np.setxor1d(gi, di):
            assert abs(flat[j] - kth) <= 2 * eps + 1e-9 or abs(flat[j] - 0.015) <= 2 * eps + 1e-9
        common, ia, ib = np.intersect1d(gi, di, return_indices=True)
        assert len(common) >= len(di) - 2
        assert np.abs(desc[ia] - fd[i]["desc"][ib]).max() <= 1e-5
    assert rec["wino_nt2_claimed_fused1b"] >= 1 and rec["wino_nt2_claimed_ring"] >= 1, rec


def test_headline_pass_exact_mode_against_the_oracle(api, sp_weights, headline):
    """precision = PREC_F32 at 64 images (no claiming in this mode, but its persistent conv_pc walk is not run beyond 8 full-size images elsewhere):
    keypoints and scores bitwise equal to the direct oracle's, descriptors at the exact mode's 1e-6, every image equal to its 1-image call."""
    imgs, other, ref = headline.frames("A"), headline.frames("B"), headline.direct("A")
    fe = api.DevFrontEnd(_cfg(api, api.PREC_F32))
    fe.load_superpoint(sp_weights)
    fe.extract_batch(other, cap=CAP)
    api.DevFrontEnd.regime_reset()
    res = fe.extract_batch(imgs, cap=CAP)
    _show("(a) 64-image exact-mode call", api.DevFrontEnd.regime_counts())
    singles = [fe.extract_batch(imgs[i:i + 1], cap=CAP)[0] for i in range(NIMG)]
    fe.close()
    for i in range(NIMG):
        kps, sc, desc = res[i]
        assert np.array_equal(kps, ref[i]["kps"]) and np.array_equal(sc, ref[i]["sc"]), "image %d: keypoints / scores differ from the direct oracle" % i
        assert np.abs(desc - ref[i]["desc"]).max() <= 1e-6
    _assert_same_results(res, singles, "64-image call vs 1-image calls")


# ---- (b) graph replay with changing input ------------------------------------------------------------------------------------------------------------------

def test_graph_replay_with_changing_frames(api, sp_weights, headline):
    """Five 64-image host calls on one handle, a different frame set each time: from the third call on the cached hipGraph is replayed, the memset that
    zeroes the work counters being one of its nodes.  A counter that a replay does not zero leaves tiles of the previous call in place: every call's
    keypoints and scores must be the oracle's for THAT call's frames."""
    fe = api.DevFrontEnd(_cfg(api, api.PREC_F32_WINO))
    fe.load_superpoint(sp_weights)
    api.DevFrontEnd.regime_reset()
    results = [(key, fe.extract_batch(headline.frames(key), cap=CAP)) for key in ("A", "B", "C", "A", "B")]
    graphs, rejected = fe.graph_count()
    rec = api.DevFrontEnd.regime_counts()
    fe.close()
    _show("(b) five 64-image calls (launchers run in the first two; then the graph replays)", rec)
    assert graphs >= 1 and rejected == 0, (graphs, rejected)
    assert rec["wino_nt2_claimed_fused1b"] >= 1 and rec["wino_nt2_claimed_ring"] >= 1, rec
    for call, (key, res) in enumerate(results):
        ref = headline.wino(key)
        for i in range(NIMG):
            kps, sc, desc = res[i]
            assert np.array_equal(kps, ref[i]["kps"]) and np.array_equal(sc, ref[i]["sc"]), "call %d (set %s), image %d" % (call, key, i)
            assert np.abs(desc - ref[i]["desc"]).max() <= 1e-5


# ---- (c), (d) the pipe ----------------------------------------------------------------------------------------------------------------------------------------

def _run_pipe(api, fe, lanes, frames, cap, sets, H, W, **kw):
    """submits every set ([2 * frames, H, W]: lefts, then rights) with `lanes` passes in flight; returns copies of the results"""
    pipe = api.StereoPipe(fe, lanes=lanes, frames=frames, width=W, height=H, cap=cap, ratio=0.8, **kw)
    nsub = len(sets)
    tickets = [pipe.submit(sets[s][:frames], sets[s][frames:]) for s in range(min(nsub, lanes))]
    got = []
    for s in range(nsub):
        got.append({k: (None if v is None else v.copy()) for k, v in pipe.wait(tickets[s]).items()})
        if len(tickets) < nsub:
            tickets.append(pipe.submit(sets[len(tickets)][:frames], sets[len(tickets)][frames:]))
    pipe.close()
    return got


def _check_pipe_vs_single_calls(fe, got, sets, frames, cap, netvlad, full_cap):
    """the comparisons of test_pipe_at_the_baseline_geometry: every submit against extract_all_batch / extract_batch and match_knn of the same handle"""
    prev, nprev, nlr = None, 0, 0
    for s, o in enumerate(got):
        if netvlad:
            ext, g = fe.extract_all_batch(sets[s], frames, cap=cap)
            np.testing.assert_array_equal(o["netvlad"], g)
        else:
            ext = fe.extract_batch(sets[s], cap=cap)
        for i, (kps, sc, desc) in enumerate(ext):
            n = int(o["n_kp"][i]); assert n == len(kps)
            if full_cap:
                assert n == cap
            np.testing.assert_array_equal(o["kps_xy"][i, :n], kps); np.testing.assert_array_equal(o["scores"][i, :n], sc); np.testing.assert_array_equal(o["desc"][i, :n], desc)
        for f in range(frames):
            q, t, d = fe.match_knn(ext[f][2], ext[frames + f][2], 0.8)
            n = int(o["lr_n"][f]); assert n == len(q)
            nlr += n
            np.testing.assert_array_equal(o["lr_q"][f, :n], q); np.testing.assert_array_equal(o["lr_t"][f, :n], t); np.testing.assert_array_equal(o["lr_dist"][f, :n], d)
            pv = ext[f - 1] if f > 0 else prev
            if pv is not None:
                q, t, d = fe.match_knn(ext[f][2], pv[2], 0.8)
                n = int(o["prev_n"][f]); assert n == len(q)
                np.testing.assert_array_equal(o["prev_q"][f, :n], q); np.testing.assert_array_equal(o["prev_t"][f, :n], t); np.testing.assert_array_equal(o["prev_dist"][f, :n], d)
                nprev += n
        prev = ext[frames - 1]
    assert nprev > 0 and nlr > 0


def _check_submit_vs_oracle(orc, o, o_before, ref, frames, desc_tol):
    """one whole submit: keypoints and scores against the oracle's (ref: per image), and its 2 * frames match lists (L -> R, L -> previous L) against
    orc.match_knn on the pipe's OWN descriptors, bitwise"""
    for i in range(2 * frames):
        n = int(o["n_kp"][i])
        assert n == len(ref[i]["kps"]), "image %d: %d keypoints, the oracle has %d" % (i, n, len(ref[i]["kps"]))
        assert np.array_equal(o["kps_xy"][i, :n], ref[i]["kps"]) and np.array_equal(o["scores"][i, :n], ref[i]["sc"]), "image %d differs from the oracle" % i
        assert np.abs(o["desc"][i, :n] - ref[i]["desc"]).max() <= desc_tol
    nmatch = 0
    for f in range(frames):
        nl, nr = int(o["n_kp"][f]), int(o["n_kp"][frames + f])
        rq, rt, rd = orc.match_knn(o["desc"][f, :nl], o["desc"][frames + f, :nr], 0.8)
        n = int(o["lr_n"][f]); assert n == len(rq), "L -> R list %d: %d matches, the oracle has %d" % (f, n, len(rq))
        assert np.array_equal(o["lr_q"][f, :n], rq) and np.array_equal(o["lr_t"][f, :n], rt) and np.array_equal(o["lr_dist"][f, :n], rd), "L -> R list %d" % f
        if f > 0:
            pd = o["desc"][f - 1, :int(o["n_kp"][f - 1])]
        else:
            pd = o_before["desc"][frames - 1, :int(o_before["n_kp"][frames - 1])]      # the last left frame of the previous submit
        rq, rt, rd = orc.match_knn(o["desc"][f, :nl], pd, 0.8)
        n = int(o["prev_n"][f]); assert n == len(rq), "L -> previous L list %d: %d matches, the oracle has %d" % (f, n, len(rq))
        assert np.array_equal(o["prev_q"][f, :n], rq) and np.array_equal(o["prev_t"][f, :n], rt) and np.array_equal(o["prev_dist"][f, :n], rd), "L -> previous L list %d" % f
        nmatch += len(rq)
    assert nmatch > 0


def test_pipe_in_the_benchmark_shape(api, orc, sp_weights, headline):
    """lanes = 2, frames = 32 at the baseline geometry (what bench.py times), 2 * lanes + 1 submits of different frame sets: the assertions of
    test_pipe_at_the_baseline_geometry (pipe == single calls of the same handle, which take the claimed walk themselves), and -- so that the comparison
    is not self-referential -- one whole submit against the oracle: keypoints, scores, and its 64 match lists against orc.match_knn.  The record must show
    claimed Winograd walks and a two-wave matcher launch made by the PIPE (it is read before the single calls run)."""
    from d2slam_amd import netvlad as nvm
    frames, lanes = 32, 2
    order = ["B", "C", "A", "D", "E"]                  # submit 2 (set A, the one with the cached oracle results) follows a pass of the same lane on set B
    sets = [headline.frames(k) for k in order]
    ref = headline.wino("A")
    fe = api.DevFrontEnd(_cfg(api, api.PREC_F32_WINO))
    fe.load_superpoint(sp_weights); fe.load_netvlad(nvm.synthetic_netvlad_weights())
    api.DevFrontEnd.regime_reset()
    got = _run_pipe(api, fe, lanes, frames, CAP, sets, Hb, Wb, netvlad=True)
    rec = api.DevFrontEnd.regime_counts()
    _show("(c) pipe, lanes 2 x 32 stereo frames, 5 submits", rec)
    _check_submit_vs_oracle(orc, got[2], got[1], ref, frames, 1e-5)
    _check_pipe_vs_single_calls(fe, got, sets, frames, CAP, True, True)
    fe.close()
    assert rec["match_nw2"] >= 1, "the pipe's matcher launch did not take the two-wave kernel: %s" % rec
    assert rec["wino_nt2_claimed_fused1b"] >= 1 and rec["wino_nt2_claimed_ring"] >= 1, "no claimed Winograd walk in the pipe's passes: %s" % rec
    # NetVLAD of the 32 left frames: the batch forms of its launchers (merged channel groups, several tiles per workgroup in the first block)
    assert rec["nv_gmerge"] >= 1 and rec["nv_front_tpw"] >= 1, rec


def _small_frames(n, H, W):
    """consecutive frames of one scene under a small camera motion (as tests/test_pipe.py), so that the temporal matches exist"""
    l0, r0 = synth_stereo(H, W, seed=100)
    rng = np.random.RandomState(5)
    out = []
    for i in range(n):
        sh = (i % 4, (2 * i) % 5)
        noise = rng.randint(-2, 3, (2, H, W))
        out.append((np.clip(np.roll(l0, sh, (0, 1)).astype(np.int16) + noise[0], 0, 255).astype(np.uint8),
                    np.clip(np.roll(r0, sh, (0, 1)).astype(np.int16) + noise[1], 0, 255).astype(np.uint8)))
    return out


def test_claimed_walk_on_a_cu_limited_lane(api, orc, sp_weights):
    """The seconds-long guard of the same paths: lanes sized for 16 compute units (lane_cus) at 120 x 160 with 6 stereo frames per submit -- 12 images x 150
    conv1b items against a claim threshold of 48 x 32, and 12 matcher pairs of 3 x 2 workgroups against 2 x 16 -- so the fused conv1b kernel claims and the
    matcher runs two-wave workgroups.  Pipe == single calls bitwise; one submit against the oracle (keypoints, scores, match lists)."""
    H, W, cap, frames, lanes = 120, 160, 80, 6, 2
    nsub = 2 * lanes + 1
    fr = _small_frames(nsub * frames, H, W)
    sets = [np.stack([fr[s * frames + f][0] for f in range(frames)] + [fr[s * frames + f][1] for f in range(frames)]) for s in range(nsub)]
    fe = api.DevFrontEnd(api.SuperPointConfig(max_keypoints=cap, input_width=W, input_height=H, max_batch=2 * frames, precision=api.PREC_F32_WINO,
                                              keypoint_threshold=0.005))
    fe.load_superpoint(sp_weights)
    api.DevFrontEnd.regime_reset()
    got = _run_pipe(api, fe, lanes, frames, cap, sets, H, W, netvlad=False, lane_cus=16)
    rec = api.DevFrontEnd.regime_counts()
    _show("(d) pipe with lane_cus = 16, 12 images of 120 x 160 per pass", rec)
    ref = []
    for img in sets[3]:
        f = orc.superpoint_forward(img, sp_weights, wino=True)
        kps, sc, _ = orc.select_b(f["semi"], 0.005, 1, cap)
        ref.append({"kps": kps, "sc": sc, "desc": orc.sample_b(f["desc"], kps)})
    _check_submit_vs_oracle(orc, got[3], got[2], ref, frames, 1e-5)
    _check_pipe_vs_single_calls(fe, got, sets, frames, cap, False, False)
    fe.close()
    assert rec["wino_nt2_claimed_fused1b"] + rec["wino_nt2_claimed_ring"] >= 1, "no claimed Winograd walk on the 16-CU lane: %s" % rec
    assert rec["match_nw2"] >= 1, "the lane's matcher launch did not take the two-wave kernel: %s" % rec


# ---- (e) walk boundaries at layer level ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nt", [1, 2])
def test_wino_walk_boundaries(nt):
    """Single layers whose item count is one round of persistent workgroups minus one, exactly one round, one round plus one and two rounds plus one
    (tests/helpers/wino_walk_worker.py; NT = 1: two items per image, so the nearest even counts), in the 32-channel (NT = 1) and the 64-channel (NT = 2) item
    form, cin 64 and 128, with and without the pool: bitwise against orc.conv_wino, and the walk each launch took as the record names it."""
    env = dict(os.environ, D2FE_WINO_NT=str(nt))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "wino_walk_worker.py")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "worker failed (exit %d):\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    grid = out["grid"]
    print("\n[launch regimes] (e) forced NT = %d on %d CUs: a round is %d workgroups, %d item(s) per image" % (nt, out["ncu"], grid, out["items_per_image"]), flush=True)
    one, static = "wino_nt%d_one" % nt, "wino_nt%d_static" % nt
    assert out["items_per_image"] == 3 - nt
    kinds = set()
    for c in out["cases"]:
        print("    %-5s n %4d cin %3d pool %d: grid %4d items %4d  %s" % (c["kind"], c["n"], c["cin"], c["pool"], c["grid"], c["total"], c["regimes"]), flush=True)
        assert c["equal"], "NT = %d, %s: differs from orc.conv_wino, max |diff| %g" % (nt, c, c["max_diff"])
        assert c["total"] == c["n"] * out["items_per_image"]
        lo, hi = {"probe": (grid + 1, 2 * grid + 2), "below": (grid - 2, grid - 1), "at": (grid, grid + 1), "above": (grid + 1, grid + 2), "two": (2 * grid + 1, 2 * grid + 2)}[c["kind"]]
        assert lo <= c["total"] <= hi, c
        if c["total"] <= grid:       # one round or less: every workgroup has one item
            assert c["regimes"] == {one: 1} and c["grid"] == c["total"], c
        else:                        # persistent workgroups stride through the items (no layer here is large enough to claim)
            assert c["regimes"] == {static: 1} and c["grid"] == grid, c
        kinds.add((c["kind"], c["cin"], c["pool"]))
    assert {k for k, _, _ in kinds} == {"probe", "below", "at", "above", "two"} and any(cin == 128 for _, cin, _ in kinds) and any(p for _, _, p in kinds)


def _ncu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.mark.parametrize("cin,cout,pool", [(64, 256, False), (128, 256, True)])
def test_wino_layer_past_the_claim_threshold(api, orc, cin, cout, pool):
    """One layer large enough to claim: 32 x 64 pixels x 256 output channels are 64 items per image, and enough images for 48 items per workgroup of a full
    grid plus some (400 images on 256 compute units).  d2fe_debug_conv3x3_wino gives the launch a zeroed work counter, as a pass of the extractor does.
    Bitwise against orc.conv_wino for every image; the regime comes from the record."""
    H, W = 32, 64
    n = (48 * 2 * _ncu() + 63) // 64 + 16
    rng = np.random.default_rng(cin + cout + int(pool))
    x = np.maximum(rng.standard_normal((n, H, W, cin), dtype=np.float32), 0.0)
    wg = (rng.standard_normal((cout, cin, 3, 3)) * (0.6 / np.sqrt(cin))).astype(np.float32)
    b = (rng.standard_normal(cout) * 0.1).astype(np.float32)
    fe = api.DevFrontEnd(api.SuperPointConfig(max_keypoints=16, input_width=64, input_height=64, max_batch=1))
    api.DevFrontEnd.regime_reset()
    out, _ = fe.debug_conv3x3_wino(x, wg, b, pool=pool)
    rec = api.DevFrontEnd.regime_counts()
    fe.close()
    _show("(e) %d images of 32 x 64 x %d -> %d%s" % (n, cin, cout, ", pooled" if pool else ""), rec)
    for i in range(n):
        ref = orc.conv_wino(x[i], wg, b, True)
        if pool:
            ref = orc.maxpool2(ref)
        assert out[i].shape == ref.shape
        assert np.array_equal(out[i], ref), "image %d: %d values differ, max |diff| %g" % (i, int((out[i] != ref).sum()), np.nanmax(np.abs(out[i] - ref)))
    assert rec["wino_nt2_claimed_ring"] == 1, "the layer did not take the claimed walk: %s" % rec
    assert rec["wino_last_total"] == 64 * n and rec["wino_last_total"] >= 48 * rec["wino_last_grid"], rec


# ---- (f) the two-wave matcher ----------------------------------------------------------------------------------------------------------------------------------

def _unit(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def _match_handle(api):
    return api.DevFrontEnd(api.SuperPointConfig(max_keypoints=200, input_width=64, input_height=64, max_batch=1))


@pytest.mark.parametrize("dim", [256, 64])
def test_match_batch_of_64_pairs_takes_the_two_wave_kernel(api, orc, dim):
    """64 pairs at capacity 200 in one launch -- 7 x 2 x 64 workgroups, the benchmark's matcher launch: random row counts 1..200 (1 and 200 among them), exact
    duplicates, near-copies at 1e-7 and groups of identical rows injected as in test_match_random_shapes_with_injected_duplicates; matchKNN without and with a
    radius gate and the cross-check matcher, indices and distances bitwise equal to the oracle's for every pair."""
    pytest.importorskip("torch")
    cap, npairs = 200, 64
    rng = np.random.RandomState(640 + dim)
    pairs, pts = [], []
    for p in range(npairs):
        na, nb = int(rng.randint(1, cap + 1)), int(rng.randint(1, cap + 1))
        if p == 0:
            na, nb = 1, cap
        elif p == 1:
            na, nb = cap, 1
        elif p == 2:
            na, nb = cap, cap
        elif p == 3:
            na, nb = 1, 1
        a = _unit(rng.randn(na, dim)); b = _unit(rng.randn(nb, dim))
        k = min(na, nb) // 2
        if k:                                   # shared content so that matches exist
            b[:k] = _unit(a[rng.permutation(na)[:k]] + 0.08 * rng.randn(k, dim))
        for side in (a, b):                      # degenerate structure
            m = len(side)
            if m >= 4 and rng.rand() < 0.7:
                g = int(rng.randint(2, min(m, 13)))
                side[rng.choice(m, g, replace=False)] = side[int(rng.randint(0, m))]
            if m >= 4 and rng.rand() < 0.5:
                i, j = rng.choice(m, 2, replace=False)
                side[i] = (side[j] + np.float32(1e-7) * rng.randn(dim)).astype(np.float32)
        if p % 3 == 0 and nb >= 2:               # an exact copy of a query among the train rows, twice
            b[0] = a[0]; b[nb - 1] = a[0]
        pairs.append((a, b))
        pts.append(((rng.rand(na, 2) * 640).astype(np.float32), (rng.rand(nb, 2) * 640).astype(np.float32)))
    fe = _match_handle(api)
    api.DevFrontEnd.regime_reset()
    runs = [("matchKNN", _match_batch(api, fe, pairs, dim, cap, ratio=0.8), lambda p: orc.match_knn(pairs[p][0], pairs[p][1], 0.8)),
            ("matchKNN, ratio 1.1", _match_batch(api, fe, pairs, dim, cap, ratio=1.1), lambda p: orc.match_knn(pairs[p][0], pairs[p][1], 1.1)),
            ("matchKNN, radius 150", _match_batch(api, fe, pairs, dim, cap, ratio=0.8, radius=150.0, pts=pts),
             lambda p: orc.match_knn(pairs[p][0], pairs[p][1], 0.8, pts[p][0], pts[p][1], 150.0)),
            ("cross-check", _match_batch(api, fe, pairs, dim, cap, mode=1), lambda p: orc.match_crosscheck(pairs[p][0], pairs[p][1]))]
    rec = api.DevFrontEnd.regime_counts()
    fe.close()
    _show("(f) 64 pairs x 200 rows x %d, four launches" % dim, rec)
    total = 0
    for what, got, ref in runs:
        for p in range(npairs):
            rq, rt, rd = ref(p)
            q, t, d = got[p]
            assert len(q) == len(rq), "%s, pair %d (%d x %d rows): %d matches, the oracle has %d" % (what, p, len(pairs[p][0]), len(pairs[p][1]), len(q), len(rq))
            assert np.array_equal(q, rq) and np.array_equal(t, rt) and np.array_equal(d, rd), "%s, pair %d (%d x %d rows)" % (what, p, len(pairs[p][0]), len(pairs[p][1]))
            total += len(rq)
    assert total > 1000
    assert rec["match_nw2"] == 4 and rec["match_nw4"] == 0, "the launches did not take the two-wave kernel: %s" % rec


@pytest.mark.parametrize("na,nb,dim", [(16384, 9000, 256), (16384, 16384, 64)])
def test_match_at_the_row_limit(api, orc, na, nb, dim):
    """One pair at the documented row limit (MATCH_MAXN = 16384; 512 x 2 workgroups, the two-wave kernel): matchKNN with and without a radius gate and the
    cross-check matcher bitwise equal to the oracle."""
    a, b, pa, pb = synth_descriptor_pair(na, nb, dim, seed=na + nb + dim, sigma=0.1)
    fe = _match_handle(api)
    api.DevFrontEnd.regime_reset()
    for radius in (-1.0, 60.0):
        q, t, d = fe.match_knn(a, b, 0.8, pa, pb, radius)
        rq, rt, rd = orc.match_knn(a, b, 0.8, pa, pb, radius)
        assert len(rq) > 100 and np.array_equal(q, rq) and np.array_equal(t, rt) and np.array_equal(d, rd), "radius %g: %d matches, the oracle has %d" % (radius, len(q), len(rq))
    q, t, d = fe.match_crosscheck(a, b)
    rq, rt, rd = orc.match_crosscheck(a, b)
    assert len(rq) > 100 and np.array_equal(q, rq) and np.array_equal(t, rt) and np.array_equal(d, rd)
    rec = api.DevFrontEnd.regime_counts()
    fe.close()
    _show("(f) one pair of %d x %d x %d" % (na, nb, dim), rec)
    assert rec["match_nw2"] == 3 and rec["match_nw4"] == 0, rec


def test_match_saturated_batch_in_the_two_wave_kernel(api, orc):
    """The SATURATED cases of tests/test_gpu_parity.py as 64 copies in one batched launch each, so that the exact re-ranking and the exact scan of every
    train row run inside the two-wave kernel: every copy bitwise equal to the oracle, matchKNN at ratio 0.8 and 1.5 and the cross-check matcher."""
    pytest.importorskip("torch")
    from tests.test_gpu_parity import SATURATED, saturated_pair
    fe = _match_handle(api)
    api.DevFrontEnd.regime_reset()
    launches = 0
    for case in SATURATED:
        a, b = saturated_pair(case)
        cap = 200
        assert len(a) <= cap and len(b) <= cap
        fe.match_fallback_rows(reset=True)
        for mode, ratio in ((0, 0.8), (0, 1.5), (1, 0.8)):
            got = _match_batch(api, fe, [(a, b)] * 64, 256, cap, mode=mode, ratio=ratio)
            launches += 1
            rq, rt, rd = orc.match_knn(a, b, ratio) if mode == 0 else orc.match_crosscheck(a, b)
            for p, (q, t, d) in enumerate(got):
                assert np.array_equal(q, rq) and np.array_equal(t, rt) and np.array_equal(d, rd), "%s, mode %d, ratio %g, copy %d" % (case, mode, ratio, p)
        extra, scans = fe.match_fallback_rows(full=True)
        assert extra > 0, "the saturated rows of %s were not re-ranked beyond two candidates" % case
        if "all_equal" in case or case == "twenty_identical_train_rows":
            assert scans > 0, "more than sixteen rows within round-off (%s): the exact scan must have run" % case
    rec = api.DevFrontEnd.regime_counts()
    fe.close()
    _show("(f) saturated cases, 64 copies per launch", rec)
    assert rec["match_nw2"] == launches and rec["match_nw4"] == 0, rec
