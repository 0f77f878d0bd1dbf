"""The value contract of the depth lookup (include/d2fe.h, d2fe_pipe_depth_result) restated in NumPy, for the CPU pin (tests/test_pipe_mono_cpu.py) and the GPU tests
(tests/test_pipe_mono.py): depth[cvRound(y)][cvRound(x)], cvRound = round half to even (np.rint), 0 when the rounded index is outside the image or a coordinate is
NaN -- what cv::Mat::at<ushort>(cv::Point2f) reads inside the image (loop_cam.cpp:382, d2featuretracker.cpp:790-798)."""
import numpy as np


def depth_at_np(depth, pts):
    """depth [H, W] uint16, pts [n, 2] float32 (x, y) -> [n] uint16"""
    depth = np.asarray(depth)
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    H, W = depth.shape
    with np.errstate(invalid="ignore"):
        r = np.rint(pts)
        ok = (r[:, 0] >= 0) & (r[:, 0] < W) & (r[:, 1] >= 0) & (r[:, 1] < H)        # False for NaN
    out = np.zeros(len(pts), np.uint16)
    out[ok] = depth[r[ok, 1].astype(np.int64), r[ok, 0].astype(np.int64)]
    return out


def seeded_depth(n, h, w, seed):
    """n depth frames [n, h, w] uint16 that contain both ends of the range"""
    d = np.random.RandomState(seed).randint(0, 65536, (n, h, w)).astype(np.uint16)
    d[:, 0, 0] = 0; d[:, 0, 1] = 65535; d[:, h - 1, w - 1] = 65535; d[:, h // 2, w // 2] = 0
    return d


def edge_table(w, h):
    """hand-written points of a w x h image: ((x, y), (ix, iy) or None = outside -> 0)"""
    nan = float("nan")
    return [((2.5, 1.0), (2, 1)), ((3.5, 1.0), (4, 1)), ((1.0, 2.5), (1, 2)), ((1.0, 3.5), (1, 4)),          # halves go to the even neighbour
            ((-0.5, 0.0), (0, 0)), ((0.0, -0.5), (0, 0)), ((-0.51, 0.0), None), ((0.0, -0.51), None),          # -0.5 rounds to (minus) zero, -0.51 to -1
            ((w - 0.5, 0.0), None), ((0.0, h - 0.5), None),                                                    # w - 0.5 rounds up to w for even w (23.5 -> 24)
            ((w - 1.0, 0.0), (w - 1, 0)), ((w - 0.51, 0.0), (w - 1, 0)), ((w - 1.5, 0.0), (w - 2, 0)),         # 22.5 -> 22
            ((nan, 1.0), None), ((1.0, nan), None), ((nan, nan), None),
            ((1e9, 1.0), None), ((-1e9, 1.0), None), ((float("inf"), 0.0), None), ((3e38, -3e38), None),
            ((0.0, 0.0), (0, 0)), ((w - 1.0, 0.0), (w - 1, 0)), ((0.0, h - 1.0), (0, h - 1)), ((w - 1.0, h - 1.0), (w - 1, h - 1)),      # the four corners
            ((0.49, 0.5), (0, 0)), ((0.51, 1.5), (1, 2)), ((7.25, 9.75), (7, 10))]
