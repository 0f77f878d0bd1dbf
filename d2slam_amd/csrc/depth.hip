// depth.hip -- PINHOLE_DEPTH: the 16-bit depth value under a point, for the keypoints and the landmark-list entries of a mono pipe (d2fe_pipe_camera::depth, pipe.hip) and for
// callers of d2fe_depth_at_device.
//
// The reference reads msg.depth_images[vcam_id].at<unsigned short>(pt_up) per keypoint (LoopCam::generateGrayDepthImageDescriptor, loop_cam.cpp:382) and
// frame.raw_depth_image.at<unsigned short>(pt) per list entry (D2FeatureTracker::createLKLandmark, d2featuretracker.cpp:790-798).  cv::Mat::at(cv::Point2f) goes
// through Point_<float> -> Point_<int>, i.e. saturate_cast<int> = cvRound, round-half-to-even (upstream OpenCV, not in the reference tree): the value at (x, y) is
// depth[cvRound(y)][cvRound(x)].  A rounded index outside the image, or a NaN coordinate, gives 0 here (the reference would read out of bounds); 0 fails its
// dep > DEPTH_NEAR_THRES test.  The / 1000.0, the thresholds and liftProjective stay with the caller.
//
// One small launch, bound by the latency of one dependent load per point (counts, points and depth are all read on the device): blockIdx.y = list, the x dimension
// strides over the list's `cap` slots; slots >= n are written as 0 so that the result never carries stale values.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/d2fe.h"
#include "context.h"

using namespace d2fe;

namespace {

struct DepthArgs {
  const uint16_t* depth; size_t row_px, image_px;      // row / image strides in pixels
  int W, H, n_lists, n_segs;
  DepthSeg seg[2];
};

__global__ __launch_bounds__(64) void depth_gather_kernel(DepthArgs a) {
  const int sl = blockIdx.y, sg = sl / a.n_lists, l = sl - sg * a.n_lists;
  if (sg >= a.n_segs) return;
  const DepthSeg& S = a.seg[sg];
  int n = S.n[(size_t)l * S.n_stride];
  n = n < 0 ? 0 : n > S.cap ? S.cap : n;
  const float* pts = S.pts + (size_t)l * S.pts_stride;
  const uint16_t* img = a.depth + (size_t)l * a.image_px;
  uint16_t* out = S.out + (size_t)l * S.cap;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < S.cap; i += gridDim.x * blockDim.x) {
    uint16_t v = 0;
    if (i < n) {
      // rintf: round-half-to-even in the default rounding mode = cvRound; the comparisons are false for NaN
      const float rx = rintf(pts[2 * i]), ry = rintf(pts[2 * i + 1]);
      if (rx >= 0.f && rx < (float)a.W && ry >= 0.f && ry < (float)a.H) v = img[(size_t)(int)ry * a.row_px + (size_t)(int)rx];
    }
    out[i] = v;
  }
}

}  // namespace

namespace d2fe {
int depth_gather_launch(d2fe_context* h, const uint16_t* d_depth, int W, int H, size_t depth_stride_px, size_t depth_image_stride_px, int n_lists, const DepthSeg* segs,
                        int n_segs, hipStream_t s) {
  if (n_lists < 1 || n_segs < 1 || n_segs > 2 || n_lists * n_segs > 65535) return ctx_fail(D2FE_ERR_INVALID, "depth gather: 1..2 segments, lists * segments <= 65535");
  DepthArgs a{};
  a.depth = d_depth; a.row_px = depth_stride_px; a.image_px = depth_image_stride_px; a.W = W; a.H = H; a.n_lists = n_lists; a.n_segs = n_segs;
  int cap = 1;
  for (int i = 0; i < n_segs; ++i) { a.seg[i] = segs[i]; cap = segs[i].cap > cap ? segs[i].cap : cap; }
  const int bx = (cap + 63) / 64;
  ProfScope ps(h, D2FE_PROF_LK, s);
  hipLaunchKernelGGL(depth_gather_kernel, dim3(bx < 16 ? bx : 16, n_lists * n_segs), dim3(64), 0, s, a);
  HIP_TRY(hipGetLastError());
  return D2FE_OK;
}
}  // namespace d2fe

extern "C" {

int d2fe_depth_at_device(d2fe_handle h, const uint16_t* d_depth, int width, int height, size_t depth_stride, size_t depth_image_stride, const float* d_pts_xy,
                         size_t pts_stride, const int32_t* d_n, int n_lists, int cap, uint16_t* d_out, void* stream) {
  if (!h || !d_depth || !d_pts_xy || !d_n || !d_out) return ctx_fail(D2FE_ERR_INVALID, "null argument");
  if (width < 1 || height < 1 || (size_t)width * height > (1u << 28)) return ctx_fail(D2FE_ERR_INVALID, "bad depth image size");
  if (depth_stride % 2 || depth_image_stride % 2 || depth_stride < (size_t)2 * width || (n_lists > 1 && depth_image_stride < depth_stride * (height - 1) + (size_t)2 * width))
    return ctx_fail(D2FE_ERR_INVALID, "bad depth stride / image stride (bytes, even, stride >= 2 * width)");
  if (n_lists < 1 || n_lists > 32767 || cap < 1 || cap > 16384 || (n_lists > 1 && pts_stride < (size_t)2 * cap)) return ctx_fail(D2FE_ERR_INVALID, "n_lists must be 1..32767, cap 1..16384, pts_stride >= 2 * cap");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  const DepthSeg seg{d_pts_xy, pts_stride, d_n, 1, cap, d_out};
  return depth_gather_launch(h, d_depth, width, height, depth_stride / 2, depth_image_stride / 2, n_lists, &seg, 1, stream ? (hipStream_t)stream : h->stream);
}

}  // extern "C"
