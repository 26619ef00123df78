"""CPU restatement of the two tensor conversions around the depth network (include/dmslam_depthnet.h) in numpy: what
DepthPrediction::predict (GUI/src/Tools/DepthPrediction.cpp:106-169) does to a frame before and after the inference call.  Test
infrastructure, like oracle/.

  pack    :112  im.convertTo(im_f, CV_32FC3, 1.0/255.0)          float(byte) * float(1.0/255.0), one fp32 multiply
          :114-121  cv::split + three plane copies                [3, H, W] in the input's channel order
          :124-131  Eigen::half_impl::float_to_half_rtne          round to nearest even (numpy's astype(float16))
  unpack  :151-160  Eigen::half_impl::half_to_float               exact
          :166  im_d.convertTo(im_d_s, CV_16UC1, 1000.0)          saturate_cast<ushort>(cvRound(x * 1000.0f))
cvRound on x86 is the SSE float -> int32 conversion (round to nearest even; INT_MIN for NaN, +-inf and whatever does not fit an
int32) and saturate_cast<ushort>(INT_MIN) is 0: so a value that cannot be an int32 becomes 0, not 65535.  This rule is read from
OpenCV's documented x86 behaviour; the library is not on the build machine, so no fixture pins it.

TRUNCATE is the reference's offline converter (logs/kitti/kitti_odom_to_lcm.py:223):
`np.array(depth*1000.0).clip(0.0, 65535.0).astype(np.uint16)`, with NaN -> 0.
"""
import numpy as np

F = np.float32
RUNTIME, TRUNCATE = 0, 1
INV255 = F(1.0 / 255.0)  # the single nearest to the double 1.0/255.0: 0x3B808081
THOUSAND = F(1000.0)


def pack(rgb, half=False):
    """(H, W, 3 or 4) u8 -> (3, H, W) float32, or float16 with `half`; a fourth byte is ignored"""
    rgb = np.asarray(rgb, np.uint8)
    assert rgb.ndim == 3 and rgb.shape[2] in (3, 4), rgb.shape
    t = (rgb[..., :3].astype(F) * INV255).astype(F)  # one fp32 product per value
    t = np.ascontiguousarray(t.transpose(2, 0, 1))
    return t.astype(np.float16) if half else t


def unpack(x, mode=RUNTIME):
    """metres, float32 or float16, any shape -> uint16 millimetres of the same shape"""
    x = np.asarray(x)
    assert x.dtype in (np.float32, np.float16), x.dtype
    with np.errstate(over="ignore", invalid="ignore"):
        r = (x.astype(F) * THOUSAND).astype(F)  # fp16 -> fp32 is exact; one fp32 product
        if mode == TRUNCATE:
            c = np.clip(r, F(0), F(65535))
            return np.where(np.isnan(r), 0, np.trunc(np.where(np.isnan(r), F(0), c))).astype(np.uint16)
        assert mode == RUNTIME, mode
        v = np.rint(r)  # nearest, ties to even
        fits = np.isfinite(v) & (np.abs(v) < F(2147483648.0))  # else cvtps2dq answers INT_MIN, and saturate_cast<ushort> of that 0
        return np.where(fits, np.clip(np.where(fits, v, F(0)), F(0), F(65535)), F(0)).astype(np.uint16)
