"""The growth paths of what a handle owns for the host-pointer calls (csrc/context.h: HostStage, MatchHost::Slot::grow), which every other test leaves at their
initial sizes: a keep-all handle whose extract call asks for more rows per image than the initial 1024 (the device output block and its pinned mirror are
replaced and the captured launch sequences, which hold the old pointers, are dropped), extract_all on the grown handle (its second stream, event and pinned
NetVLAD buffer appear), and a match of more than 1024 rows per side (the slot's buffers are replaced).  Every result is compared bit for bit with the same call
on a fresh handle, whose buffers have the final size from its first call on."""
import numpy as np
import pytest

from d2slam_amd.synth import synth_stereo
from d2slam_amd.weights import synthetic_superpoint_weights

H, W = 64, 64                  # NetVLAD takes 32 x 32 and up
CAP0, CAP1 = 1024, 2048        # the initial staging capacity per image, and a call above it (at most H * W = 4096 rows exist)
ROWS0, ROWS1, DIM = 100, 1025, 4      # a slot is sized for 1024 rows per side at first


def _fe():
    from d2slam_amd import api, netvlad as nvm
    fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=-1, input_width=64, input_height=64, max_batch=1, keypoint_threshold=0.0005))
    fe.load_superpoint(synthetic_superpoint_weights(dustbin_bias=7.5))
    fe.load_netvlad(nvm.synthetic_netvlad_weights(depth_multiplier=0.35))
    return fe


def _same(a, b, what):
    assert len(a) == len(b), what
    for x, y in zip(a, b):
        assert x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32)), what


def _rows(n, seed):
    d = np.random.RandomState(seed).randn(n, DIM).astype(np.float32)
    return d / np.linalg.norm(d, axis=1, keepdims=True)


@pytest.mark.gpu
def test_grown_staging_and_slot_give_a_fresh_handles_bits():
    img = synth_stereo(H, W, seed=5)[0][None]
    grown, fresh = _fe(), _fe()
    try:
        # the launch sequence of the initial capacity: direct, captured, replayed -- on the initial buffers
        small = [grown.extract_batch(img, cap=CAP0) for _ in range(3)]
        for s in small[1:]:
            _same(s[0], small[0][0], "cap %d, call after call" % CAP0)
        # above the initial capacity: the output block and its pinned mirror grow
        big = grown.extract_batch(img, cap=CAP1)
        ref_big = fresh.extract_batch(img, cap=CAP1)
        print("keypoints: %d at cap %d, %d at cap %d (truncated: %s)" % (len(small[0][0][0]), CAP0, len(big[0][0]), CAP1, grown.last_truncated))
        assert len(big[0][0]) > 0
        _same(big[0], ref_big[0], "cap %d on the grown handle" % CAP1)
        # the first geometry again: its captured sequence held the old block, so it runs direct, is captured and replayed once more, on the new one
        ref_small = fresh.extract_batch(img, cap=CAP0)
        _same(ref_small[0], small[0][0], "cap %d on the fresh handle" % CAP0)
        for it in range(3):
            _same(grown.extract_batch(img, cap=CAP0)[0], small[0][0], "cap %d after the growth, call %d" % (CAP0, it))
        # extract_all on the same handle: the second stream beside the grown staging
        for it in range(3):
            outs, g = grown.extract_all_batch(img, 1, cap=CAP1)
            routs, rg = fresh.extract_all_batch(img, 1, cap=CAP1)
            _same(outs[0], big[0], "extract_all SuperPoint rows, call %d" % it)
            _same(routs[0], big[0], "extract_all SuperPoint rows on the fresh handle, call %d" % it)
            _same([g], [rg], "extract_all NetVLAD, call %d" % it)
            _same([g], [fresh.netvlad(img)], "extract_all NetVLAD against d2fe_netvlad, call %d" % it)
        # the matcher: a slot at its initial size, then a call that needs more
        a0, b0, a1, b1 = _rows(ROWS0, 1), _rows(ROWS0, 2), _rows(ROWS1, 3), _rows(ROWS1, 4)
        m0 = grown.match_knn(a0, b0, 0.95)
        m1 = grown.match_knn(a1, b1, 0.95)
        r1 = fresh.match_knn(a1, b1, 0.95)
        print("matches: %d of %d rows, %d of %d rows" % (len(m0[0]), ROWS0, len(m1[0]), ROWS1))
        assert len(m1[0]) > 0
        _same(m1, r1, "%d rows per side on the grown slot" % ROWS1)
        _same(grown.match_knn(a0, b0, 0.95), m0, "%d rows per side after the growth" % ROWS0)
        _same(grown.match_crosscheck(a1, b1), fresh.match_crosscheck(a1, b1), "crosscheck, %d rows per side" % ROWS1)
    finally:
        grown.close(); fresh.close()
