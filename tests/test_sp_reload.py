"""d2fe_load_superpoint on a handle that already ran: the network a handle shares with its lanes (SpNet, csrc/context.h) is changed in place.  Weights A, then B,
then A again on one handle, two extract calls after each load (the second one goes through the captured launch sequence): the last result equals the first bit
for bit, the B result equals that of a fresh handle that only ever saw B, and the descriptor PCA set BEFORE the first load stays set throughout.  So a reload
leaves nothing of the old weights behind, keeps the PCA, and no launch sequence captured over the old device pointers is replayed.

96x96: the smallest multiple of 8 that admits exact_order's 88x88 crops.  Two images per call: the exact mode takes the dense descriptor head, the Winograd mode
the sparse one."""
import numpy as np
import pytest

from d2slam_amd.synth import synth_stereo
from d2slam_amd.weights import synthetic_superpoint_weights
from tests.test_pca_b_cpu import qr_pca

H = W = 96
CAP, PD = 40, 64
CELLS = 2 * (H // 8) * (W // 8)      # a crop slot for every cell of a call: exact_order drops none


def _same(a, b, what):
    assert len(a) == len(b), what
    for i, ((k0, s0, d0), (k1, s1, d1)) in enumerate(zip(a, b)):
        assert np.array_equal(k0, k1) and np.array_equal(s0.view(np.uint32), s1.view(np.uint32)) and np.array_equal(d0.view(np.uint32), d1.view(np.uint32)), (what, i)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f32", "wino_exact_order"])
def test_reload_in_place_keeps_pca_and_replays_no_stale_graph(mode):
    from d2slam_amd import api
    kw = dict(variant_b_pca=True)
    if mode == "wino_exact_order":
        kw.update(exact_order=True, exact_order_eps=2e-4, exact_order_crops=CELLS)
    prec = api.PREC_F32 if mode == "f32" else api.PREC_F32_WINO

    def handle():
        fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=CAP, input_width=W, input_height=H, max_batch=2, precision=prec), **kw)
        fe.set_pca(*qr_pca(PD))          # before any weights exist
        assert fe.desc_dim == PD
        return fe

    wa, wb = synthetic_superpoint_weights(seed=1234, dustbin_bias=7.5), synthetic_superpoint_weights(seed=77, dustbin_bias=7.5)
    imgs = np.stack(synth_stereo(H, W, seed=41))

    def twice(fe, what):
        first, second = fe.extract_batch(imgs, cap=CAP), fe.extract_batch(imgs, cap=CAP)
        assert fe.desc_dim == PD and all(d.shape[1] == PD for _, _, d in second), what
        _same(first, second, what + ": second call")
        return second

    fe = handle()
    try:
        fe.load_superpoint(wa)
        assert fe.desc_dim == PD
        a0 = twice(fe, "A")
        assert min(len(k) for k, _, _ in a0) > 0
        fe.load_superpoint(wb)
        assert fe.desc_dim == PD
        b0 = twice(fe, "B")
        assert any(len(x[0]) != len(y[0]) or not np.array_equal(x[0], y[0]) or not np.array_equal(x[2], y[2]) for x, y in zip(a0, b0)), "A and B give the same result"
        fe.load_superpoint(wa)
        a1 = fe.extract_batch(imgs, cap=CAP)
        assert fe.desc_dim == PD
        _same(a1, a0, "A after B against the first A")
    finally:
        fe.close()
    fresh = handle()
    try:
        fresh.load_superpoint(wb)
        _same(b0, fresh.extract_batch(imgs, cap=CAP), "B after A against a fresh handle with B")
    finally:
        fresh.close()
