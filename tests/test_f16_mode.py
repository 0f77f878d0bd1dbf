"""D2FE_PREC_F16 on the GPU (include/d2fe.h, d2fe_precision): fp16 operands, fp32 accumulation.

The reference of every numeric check is tests/helpers/f16_oracle.py -- the contract's operand rounding, then real-number (float64) products and sums -- never
another mode of the library and never the mode itself.

  1. every distinct layer shape against the oracle fed with the GPU's OWN input of that layer, at the fp32 summation bound
         |y_gpu - y_ref| <= (K + 2) * 2^-24 * S,     K = 9 Cin (Cin for the 1x1 head),   S = sum |x^ w^| 2^-(SA+SW) + |bias|
     (fp16 x fp16 is exact in fp32, so the only error of a layer is the fp32 summation's: K - 1 additions of the products, the bias, one conversion of
     margin; any summation order obeys (K - 1) u S to first order.  ReLU and max are 1-Lipschitz: a pooled output inherits the largest of its four bounds);
  2. end to end against a CPU chain of the oracle layers: score differences, and keypoint lists that may differ only where scores are within 2 eps of the
     threshold, of the K-th score or of a neighbour in the sorted list -- with eps capped by what a change of the accumulation alone does to that chain;
  3. bit identity of a frame's outputs across entry points, batch sizes and both pipes;
  4. refusals."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from d2slam_amd.synth import synth_image, synth_stereo
from tests.helpers import f16_layers as fl
from tests.helpers import f16_oracle as fo

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR = 0.015


@pytest.fixture(scope="module")
def api():
    from d2slam_amd import api as a
    a.load_library()
    return a


def _fe(api, w, H, W, n, N=200, dev=False, thr=THR, **kw):
    fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=N, input_width=W, input_height=H, max_batch=n, precision=api.PREC_F16, keypoint_threshold=thr, **kw), dev=dev)
    fe.load_superpoint(w)
    return fe


@pytest.fixture(scope="module")
def layer_tensors(api, sp_weights):
    return fl.read_tensors(api, sp_weights)


@pytest.mark.parametrize("layer", [l[0] for l in fl.LAYERS])
def test_layer_within_the_fp32_summation_bound(layer_tensors, sp_weights, layer):
    """the default schedule: the fused conv1a|conv1b as a one-tile kernel (conv_f16.hip), every other layer as a persistent kernel (conv_pc.hip)"""
    print("%s: largest error / bound = %.3g" % (layer, fl.check_layer(layer_tensors, sp_weights, layer)))


@pytest.mark.parametrize("conv_pc", ["0", "1"])
def test_layers_in_the_other_kernel_families(conv_pc):
    """D2FE_CONV_PC = 0: every layer through the one-tile kernels; 1: every layer, the fused one included, through the persistent kernels.  The development
    library reads the switch once per process, hence the child process; it runs the same check on the same images."""
    env = dict(os.environ, D2FE_CONV_PC=conv_pc)
    r = subprocess.run([sys.executable, "-m", "tests.helpers.f16_layers"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "F16_LAYERS_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def _lists_may_differ_only_at_near_ties(gi, ri, ref_scores, eps, thr, N, what):
    """gi / ri: raster indices in list order (GPU / reference); ref_scores: the reference's flat score map"""
    kth = float(ref_scores[ri[-1]]) if len(ri) == N else None
    for j in np.setxor1d(gi, ri):
        s = float(ref_scores[j])
        near_thr = abs(s - thr) <= 2 * eps + 1e-9
        near_kth = kth is not None and abs(s - kth) <= 2 * eps + 1e-9
        assert near_thr or near_kth, "%s: keypoint %d (reference score %.9g) is in one list only; threshold %.9g, K-th %s, eps %.3g" % (what, j, s, thr, kth, eps)
    if len(gi) == N:      # a sorted list: two keypoints may only swap places when the reference scores them within 2 eps of each other
        s = ref_scores[gi]
        assert np.all(s[:-1] >= s[1:] - (2 * eps + 1e-9)), "%s: list order differs beyond 2 eps" % what
    else:                 # fewer than N: raster order
        assert np.all(np.diff(gi) > 0), "%s: not in raster order" % what


def test_end_to_end_against_the_cpu_chain(api, orc, sp_weights):
    H, W, N = 96, 128, 200
    imgs = np.stack(synth_stereo(H, W, seed=3))
    fe = _fe(api, sp_weights, H, W, 2, N=N, dev=True, keep_score_map=True)
    res = fe.extract_batch(imgs, cap=N)
    semi = fe.debug_read("semi", (2, H, W)).copy()
    a4b = fe.debug_read("conv4b", (2, H // 8, W // 8, 128)).copy()
    fe.close()
    eps = acc_dev = 0.0
    refs = []
    for i in range(2):
        c1a = orc.conv(orc.prep_u8(imgs[i])[:, :, None], *sp_weights["conv1a"], True)      # exact fp32 in every mode
        lg64, _ = fo.chain_logits(c1a, sp_weights, np.float64)
        lg32, _ = fo.chain_logits(c1a, sp_weights, np.float32)
        s64, s32 = orc.softmax_semi(lg64), orc.softmax_semi(lg32)
        refs.append(s64)
        eps = max(eps, float(np.abs(semi[i] - s64).max()))
        acc_dev = max(acc_dev, float(np.abs(s64 - s32).max()))
    print("largest score difference GPU - CPU chain: %.4g; between the float64- and the float32-accumulating CPU chain: %.4g" % (eps, acc_dev))
    try:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "f16_tolerances.json"), "w") as f:
            json.dump({"geometry": [H, W], "images": 2, "max_keypoints": N, "threshold": THR,
                       "eps_gpu_vs_cpu_chain": eps, "cpu_float64_vs_float32_accumulation": acc_dev, "cap_on_eps": 8 * acc_dev}, f, indent=1)
            f.write("\n")
    except OSError:
        pass
    assert acc_dev > 0
    assert eps <= 8 * acc_dev, "scores differ from the CPU chain by %.4g, more than 8 x what the accumulation alone changes (%.4g)" % (eps, acc_dev)
    for i in range(2):
        s64 = refs[i]
        rk, rs, ri = orc.select_b(s64, THR, 1, N)
        kps, sc, desc = res[i]
        assert len(kps) > 20
        gi = (kps[:, 1] * W + kps[:, 0]).astype(np.int64)
        _lists_may_differ_only_at_near_ties(gi, ri.astype(np.int64), s64.reshape(-1), eps, THR, N, "image %d" % i)
        assert np.abs(sc - s64.reshape(-1)[gi]).max() <= eps
        # the descriptor head stays fp32: the oracle's exact chains on the GPU's own trunk, at the exact mode's descriptor tolerance
        cda = orc.conv(a4b[i], *sp_weights["convDa"], True)
        dmap = orc.l2norm_rows(orc.conv(cda, *sp_weights["convDb"], False))
        assert np.abs(desc - orc.sample_b(dmap, kps)).max() <= 1e-6


def _same(a, b, what):
    assert len(a[0]) == len(b[0]) and len(a[0]) > 0, what
    for k, name in enumerate(("kps_xy", "scores", "desc")):
        np.testing.assert_array_equal(a[k], b[k], err_msg="%s %s" % (what, name))


def test_one_image_equals_the_same_image_in_a_batch_of_five(api, sp_weights):
    H, W = 96, 128
    imgs = np.stack([synth_image(H, W, 60 + s) for s in range(5)])
    fe = _fe(api, sp_weights, H, W, 5, N=100)
    five = [tuple(x.copy() for x in r) for r in fe.extract_batch(imgs, cap=100)]
    for i in (0, 2, 4):
        one, = fe.extract_batch(imgs[i:i + 1], cap=100)
        _same(one, five[i], "image %d alone / in the batch" % i)
    fe.close()


def test_stereo_pipe_equals_extract_batch(api, sp_weights):
    H, W, CAP, F = 96, 128, 100, 2
    fe = _fe(api, sp_weights, H, W, 2 * F, N=CAP)
    pipe = api.StereoPipe(fe, lanes=2, frames=F, width=W, height=H, cap=CAP, netvlad=False)
    subs = []
    for s in range(3):
        pairs = [synth_stereo(H, W, seed=80 + 2 * s + f) for f in range(F)]
        subs.append((np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])))
    tickets = [pipe.submit(L, R) for L, R in subs[:2]]
    got = [{k: (None if v is None else v.copy()) for k, v in pipe.wait(t).items()} for t in tickets]
    got.append({k: (None if v is None else v.copy()) for k, v in pipe.wait(pipe.submit(*subs[2])).items()})
    for s, (L, R) in enumerate(subs):
        ext = fe.extract_batch(np.concatenate([L, R]), cap=CAP)
        for i in range(2 * F):
            n = int(got[s]["n_kp"][i])
            _same((got[s]["kps_xy"][i, :n], got[s]["scores"][i, :n], got[s]["desc"][i, :n]), ext[i], "submit %d image %d" % (s, i))
    pipe.close(); fe.close()


def test_quad_pipe_ticket_equals_extract_batch(api, sp_weights):
    from d2slam_amd import quadcam
    RH, RW, UH, UW, CAP = 240, 384, 120, 192, 60
    w = dict(sp_weights)
    Wt, b = w["convPb"]
    b = b.copy(); b[64] -= np.float32(3.5); w["convPb"] = (Wt, b)      # threshold 0.15 (the quadcam configuration) still finds keypoints
    fe = _fe(api, w, UH, UW, 8, N=CAP, thr=0.15)
    maps = [quadcam.synthetic_maps(c, RH, RW, UH, UW) for c in range(4)]
    pipe = api.QuadPipe(fe, maps, lanes=2, quads=2, raw_width=RW, raw_height=RH, width=UW, height=UH, cap=CAP, netvlad=False, radius_neighbour=0.2 * UW)
    raw = np.stack([np.stack([synth_image(RH, RW, 300 + 4 * q + c) for c in range(4)]) for q in range(2)])
    o = {k: (None if v is None else v.copy()) for k, v in pipe.wait(pipe.submit(raw)).items()}
    for q in range(2):
        views = np.stack([fe.undistort(raw[q, c], *maps[c]) for c in range(4)])
        ext = fe.extract_batch(views, cap=CAP)
        for c in range(4):
            n = int(o["n_kp"][q, c])
            _same((o["kps_xy"][q, c, :n], o["scores"][q, c, :n], o["desc"][q, c, :n]), ext[c], "quad frame %d view %d" % (q, c))
    pipe.close(); fe.close()


def test_refusals(api):
    from d2slam_amd.api import D2FEError
    ERR_INVALID = -1      # D2FE_ERR_INVALID (include/d2fe.h)
    cfg = api.SuperPointConfig(max_keypoints=50, input_width=128, input_height=96, max_batch=1, precision=api.PREC_F16)
    with pytest.raises(D2FEError) as e:
        api.FrontEnd(cfg, exact_order=True)
    assert e.value.code == ERR_INVALID and "D2FE_PREC_F16 " in str(e.value).replace("D2FE_PREC_F16X2", "")
    with pytest.raises(D2FEError) as e:
        api.FrontEnd(api.SuperPointConfig(max_keypoints=50, input_width=128, input_height=96, max_batch=1, precision=4))
    assert e.value.code == ERR_INVALID
