"""Python mirror of the reference's surfel-map API over the C ABI (include/dmslam_fusion.h).

Names follow the reference: `GlobalModel` (Core/src/GlobalModel.h:43-141), `IndexMap`
(Core/src/IndexMap.h:33-205), `ElasticFusion.processFrame` (Core/src/ElasticFusion.h:92-100).
All work happens on the GPU inside libdmslam_hip.so; numpy only crosses at upload / download.
"""
import ctypes as C
import os

import numpy as np

from . import capi
from .capi import Camera, DeviceBuffer, DeviceImage, Image2D, TrackResult, check, lib

MAX_SENSORS = capi.MAX_SENSORS
SURFEL_DTYPE = np.dtype([("pos", "<f4", (4,)), ("col", "<f4", (4,)), ("nrm", "<f4", (4,)), ("times", "<f4", (MAX_SENSORS,))])


class PoseBlock(C.Structure):
    _fields_ = [("pose", C.c_float * 16), ("t_inv", C.c_float * 16)]


class IndexMapOut(C.Structure):
    _fields_ = [("index", Image2D), ("vertConf", Image2D), ("colorTime", Image2D), ("normRad", Image2D)]


class PredictOut(C.Structure):
    _fields_ = [("image", Image2D), ("vertex", Image2D), ("normal", Image2D), ("time", Image2D)]


class FusionParams(C.Structure):
    _fields_ = [
        ("width", C.c_int), ("height", C.c_int),
        ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
        ("timeDelta", C.c_int), ("confidence", C.c_float), ("depthCut", C.c_float), ("icpWeight", C.c_float),
        ("fastOdom", C.c_int), ("so3", C.c_int), ("frameToFrameRGB", C.c_int), ("pyramid", C.c_int),
        ("hybrid_tracking", C.c_int), ("rgbOnly", C.c_int), ("timeIdx", C.c_int),
        ("maxDepthProcessed", C.c_float), ("model_capacity", C.c_size_t),
        ("pipeline_ingest", C.c_int), ("global_predict", C.c_int),
        ("nid_keyframing", C.c_int), ("nid_threshold", C.c_float), ("nid_depth_lambda", C.c_float), ("nid_bins_img", C.c_int),
        ("nid_bins_depth", C.c_int), ("nid_pyramid_level", C.c_int),
        ("local_loop_closure", C.c_int), ("reloc", C.c_int), ("num_sensors", C.c_int), ("share_projection", C.c_int),
        ("fused_fill_in", C.c_int), ("hybrid_loops", C.c_int), ("lazy_final_prediction", C.c_int),
        ("fused_associate", C.c_int), ("fused_model_prediction", C.c_int), ("fused_clean_projection", C.c_int),
    ]


class FrameResult(C.Structure):
    _fields_ = [
        ("pose", C.c_float * 16), ("surfels", C.c_uint), ("tick", C.c_int), ("fused", C.c_int), ("fill_in", C.c_int),
        ("weighting", C.c_float), ("nid_score", C.c_float), ("track", TrackResult),
        ("loop_ok", C.c_int), ("loop_constraints", C.c_int), ("loop_icp_error", C.c_float), ("loop_icp_count", C.c_float),
        ("loop_pose", C.c_float * 16), ("loop_cov_diag", C.c_double * 6),
        ("tracking_ok", C.c_int), ("lost", C.c_int),
    ]


Z_CLEAR = (0xFFFFFF << 32) | 0xFFFFFFFF  # an empty z-buffer cell: depth 1.0 (24 bits), no surfel (csrc/surfel.hpp: kZClear)

_P, _I, _F = C.c_void_p, C.c_int, C.c_float
_I2 = C.POINTER(Image2D)
_K = C.POINTER(Camera)
lib.dms_model_create.argtypes = [C.POINTER(_P), C.c_size_t, _I, _I]
lib.dms_model_destroy.argtypes = [_P]
lib.dms_model_count.argtypes = [_P, C.POINTER(C.c_uint), _P]
lib.dms_model_capacity.argtypes = [_P]
lib.dms_model_set_num_sensors.argtypes = [_P, _I]
lib.dms_model_set_clean_suffix_min.argtypes = [_P, C.c_size_t]
lib.dms_model_consume.argtypes = [_P, _P, C.POINTER(C.c_float), _P]
lib.dms_model_export_records.argtypes = [_P, _P, C.c_uint, C.POINTER(C.c_uint), _P]
lib.dms_model_consume_records.argtypes = [_P, _P, C.c_uint, C.POINTER(C.c_float), _P]
lib.dms_model_capacity.restype = C.c_size_t
lib.dms_model_download.argtypes = [_P, _P, C.c_uint, C.POINTER(C.c_uint), _P]
lib.dms_model_upload.argtypes = [_P, _P, C.c_uint, _P]
lib.dms_model_download_ref.argtypes = [_P, _P, C.c_uint, C.POINTER(C.c_uint), _P]
lib.dms_model_upload_ref.argtypes = [_P, _P, C.c_uint, _P]
lib.dms_depth_bilateral.argtypes = [_I2, _I2, _F, _P]
lib.dms_depth_metric.argtypes = [_I2, _I2, _F, _P]
lib.dms_model_initialise.argtypes = [_P, _I2, _I2, _I2, _K, _I, _I, _F, _P]
lib.dms_pose_block_set.argtypes = [_P, C.POINTER(C.c_float), _P]
lib.dms_index_map.argtypes = [_P, _P, _K, _I, _I, _F, _I, _P, C.POINTER(IndexMapOut), _P]
lib.dms_splat_predict.argtypes = [_P, _P, _K, _F, _F, _I, _I, _I, _I, _I, _P, C.POINTER(PredictOut), _P]
lib.dms_splat_depth.argtypes = [_P, _P, _K, _F, _F, _I, _I, _I, _I, _P, _I2, _P]
lib.dms_model_fuse.argtypes = [_P, _P, _I, _I, _I2, _I2, _I2, C.POINTER(IndexMapOut), _K, _F, _F, _P, _P]
lib.dms_index_project.argtypes = [_P, _P, _K, _I, _I, _F, _I, _P, _P]
lib.dms_model_fuse_ex.argtypes = [_P, _P, _I, _I, _I2, _I2, _I2, C.POINTER(IndexMapOut), _P, _K, _F, _F, _P, _I, _P]
lib.dms_model_apply_pending.argtypes = [_P, _P]
lib.dms_model_fuse_scratch.argtypes = [_P, _P, _P, _P, _P, _P, _P, C.c_size_t, _P]
lib.dms_fusion_debug_keep_assoc_zbuf.argtypes = [_P, _I]
lib.dms_model_clean.argtypes = [_P, _P, _I, _I, C.POINTER(IndexMapOut), _I2, _K, _F, C.POINTER(C.c_float), _I, _I, _F, _I, _P]
lib.dms_model_clean_project.argtypes = [_P, _P, _I, _I, C.POINTER(IndexMapOut), _K, _F, _I, _F, _F, _I, _I, _I, _I, _P, C.POINTER(C.c_int), _P]
lib.dms_splat_project_only.argtypes = [_P, _P, _K, _F, _F, _I, _I, _I, _I, _I, _P, _P]
lib.dms_fill_in.argtypes =[C.POINTER(PredictOut), _I2, _I2, _K, _I, _I, C.POINTER(PredictOut), _P]
lib.dms_resize_nn.argtypes = [_I2, _I2, _I, _P]
lib.dms_fusion_default_params.argtypes = [C.POINTER(FusionParams), _I, _I, _F, _F, _F, _F]
lib.dms_fusion_default_params.restype = None
lib.dms_fusion_create.argtypes = [C.POINTER(_P), C.POINTER(FusionParams)]
lib.dms_fusion_destroy.argtypes = [_P]
lib.dms_fusion_process_frame.argtypes = [_P, _P, _I, _P, C.POINTER(C.c_float), _F, _P]
lib.dms_fusion_fetch.argtypes = [_P, C.POINTER(FrameResult), _P]
lib.dms_fusion_inputs_ready.argtypes = [_P, _P]
lib.dms_fusion_inputs_consumed.argtypes = [_P, _P]
lib.dms_fusion_model.argtypes = [_P]
lib.dms_fusion_set_orb_loop.argtypes = [_P, C.POINTER(C.c_float), C.POINTER(C.c_float)]
lib.dms_fusion_get_global_loop_constraints.argtypes = [_P, C.POINTER(C.c_float), _I, C.POINTER(C.c_int), _P]
lib.dms_fusion_apply_global_loop_begin.argtypes = [_P, C.POINTER(C.c_float), C.POINTER(C.c_float), _P]
lib.dms_fusion_apply_global_loop_end.argtypes = [_P, C.POINTER(C.c_float), _I, _I, _P]
lib.dms_fusion_model.restype = _P
lib.dms_fusion_odometry.argtypes = [_P]
lib.dms_fusion_odometry.restype = _P
lib.dms_fusion_pose_device.argtypes = [_P]
lib.dms_fusion_pose_device.restype = _P
lib.dms_model_sample_graph.argtypes = [_P, _I, C.POINTER(C.c_float), _I, C.POINTER(C.c_int), _P]
lib.dms_fusion_thumbnails.argtypes = [_P, _P, _P]
lib.dms_fusion_frame_block.argtypes = [_P, _P, _P, _P, C.c_int, _P]
lib.dms_fusion_arm_frame_block.argtypes = [_P, _P, _P, _P, C.c_int]
lib.dms_fusion_frame_block_written.argtypes = [_P]
lib.dms_fusion_get_image.argtypes = [_P, _I, _I2]
lib.dms_fusion_process_frame_begin.argtypes = [_P, _P, _I, _P, C.POINTER(C.c_float), _F, _P]
lib.dms_fusion_fetch_loop.argtypes = [_P, C.POINTER(FrameResult), _P]
lib.dms_fusion_process_frame_end.argtypes = [_P, C.POINTER(C.c_float), _I, C.POINTER(C.c_float), _P]
lib.dms_fusion_get_loop_constraints.argtypes = [_P, C.POINTER(C.c_float), _I, C.POINTER(C.c_int)]
lib.dms_fusion_join_map.argtypes = [_P, _P, C.POINTER(C.c_float), _P]
lib.dms_fusion_set_cluster.argtypes = [_P, C.c_int]
lib.dms_fusion_compute_feedback.argtypes = [_P, _P]
lib.dms_fusion_clusters.argtypes = [_P, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
lib.dms_fusion_cluster_model.argtypes = [_P, C.c_int]
lib.dms_fusion_cluster_model.restype = _P
lib.dms_fusion_import_camera.argtypes = [_P, _P, C.POINTER(C.c_float), _I, _P, _I, _P, _P]
lib.dms_relative_transform.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]
lib.dms_pose_compose.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]
lib.dms_fusion_set_profiling.argtypes = [_P, _I]
lib.dms_fusion_get_lazy_stats.argtypes = [_P, C.POINTER(C.c_int), C.POINTER(C.c_long), C.POINTER(C.c_long), C.POINTER(C.c_long)]
lib.dms_fusion_get_predict_stats.argtypes = [_P, C.POINTER(C.c_long), C.POINTER(C.c_long)]
lib.dms_fusion_get_clean_project_stats.argtypes = [_P, C.POINTER(C.c_long), C.POINTER(C.c_long)]


class InterMapResult(C.Structure):
    """dms_intermap_result (include/dmslam_fusion.h)"""
    _fields_ = [("accepted", C.c_int), ("cov_ok", C.c_int), ("relativeTransform", C.c_float * 16), ("refinedPose", C.c_float * 16),
                ("cov_diag", C.c_double * 6), ("lastICPError", C.c_float), ("lastICPCount", C.c_float), ("lastRGBError", C.c_float),
                ("lastRGBCount", C.c_float), ("iterations_run", C.c_int * 3), ("so3_iterations_run", C.c_int)]


lib.dms_refframe_create.argtypes = [C.POINTER(_P), _I, _I, _F, _F, _F, _F]
lib.dms_refframe_destroy.argtypes = [_P]
lib.dms_refframe_refine.argtypes = [_P, _P, C.POINTER(C.c_float), C.POINTER(C.c_float), _P, _P, _P, _I, _F, _I, _I, _I, _F, _F, _F,
                                    C.POINTER(InterMapResult), _P]
lib.dms_refframe_odometry.argtypes = [_P]
lib.dms_refframe_odometry.restype = _P
lib.dms_refframe_get_prediction.argtypes = [_P, C.POINTER(PredictOut)]
lib.dms_fusion_get_kernel_time.argtypes = [_P, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]


def _cam(K):
    return Camera(*[float(v) for v in K])  # (fx, fy, cx, cy)


def _img(a, dtype=None):
    if isinstance(a, DeviceImage):
        return a
    return DeviceImage.from_array(a if dtype is None else np.asarray(a, dtype))


def _f16(a):
    a = np.ascontiguousarray(a, np.float32).reshape(16)
    return a, a.ctypes.data_as(C.POINTER(C.c_float))


def relative_transform(recoveryPose, currPose):
    """relativeTransform = recoveryPose * currPose.inverse() (ReferenceFrame.h:98), the library's fixed float order."""
    a, ap = _f16(recoveryPose)
    b, bp = _f16(currPose)
    o, op = _f16(np.zeros(16, np.float32))
    check(lib.dms_relative_transform(ap, bp, op), "dms_relative_transform")
    return o.reshape(4, 4)


def pose_compose(a, b):
    """a * b for 4 x 4 float matrices in the library's fixed float order (poseGraph / relativeCons re-basing after a merge)."""
    a, ap = _f16(a)
    b, bp = _f16(b)
    o, op = _f16(np.zeros(16, np.float32))
    check(lib.dms_pose_compose(ap, bp, op), "dms_pose_compose")
    return o.reshape(4, 4)


class DevicePose:
    """dms_pose_block in HBM: pose + its inverse (Eigen Matrix4f::inverse on the reference side)."""

    def __init__(self, pose=None):
        self.buf = DeviceBuffer(C.sizeof(PoseBlock))
        self.set(np.eye(4, dtype=np.float32) if pose is None else pose)

    def set(self, pose):
        p = np.ascontiguousarray(pose, np.float32).reshape(16)
        check(lib.dms_pose_block_set(C.c_void_p(self.buf.ptr), p.ctypes.data_as(C.POINTER(C.c_float)), None), "dms_pose_block_set")
        return self

    @property
    def ptr(self):
        return C.c_void_p(self.buf.ptr)

    def download(self):
        raw = self.buf.download(np.float32, (32,))
        return raw[:16].reshape(4, 4), raw[16:].reshape(4, 4)


# ---- image-stage operators -------------------------------------------------------------------
def depth_bilateral(depth_u16, maxD):
    d = _img(depth_u16, np.uint16)
    out = DeviceImage(d.rows, d.cols, np.uint16)
    check(lib.dms_depth_bilateral(d.ref, out.ref, maxD, None), "dms_depth_bilateral")
    return out


def depth_metric(depth_u16, maxD):
    d = _img(depth_u16, np.uint16)
    out = DeviceImage(d.rows, d.cols, np.float32)
    check(lib.dms_depth_metric(d.ref, out.ref, maxD, None), "dms_depth_metric")
    return out


def resize_nn(src, drows, dcols):
    s = _img(src)
    elem = s.dtype.itemsize
    out = DeviceImage(drows, dcols, s.dtype)
    check(lib.dms_resize_nn(s.ref, out.ref, elem, None), "dms_resize_nn")
    return out


class PredictionImages:
    """image RGBA8 + vertex/normal RGBA32F + time u16 (IndexMap combined / old framebuffers)."""

    def __init__(self, rows, cols):
        self.image = DeviceImage(rows, cols, np.dtype((np.uint8, (4,))))
        self.vertex = DeviceImage(rows, cols, np.dtype((np.float32, (4,))))
        self.normal = DeviceImage(rows, cols, np.dtype((np.float32, (4,))))
        self.time = DeviceImage(rows, cols, np.uint16)
        self.c = PredictOut(self.image.view, self.vertex.view, self.normal.view, self.time.view)

    def download(self):
        return self.image.download(), self.vertex.download(), self.normal.download(), self.time.download()


def fill_in(existing, depth_filtered_u16, rgba, K, passthrough_geom=False, passthrough_rgb=False):
    d, c = _img(depth_filtered_u16, np.uint16), _img(rgba, np.uint8)
    out = PredictionImages(d.rows, d.cols)
    k = _cam(K)
    check(lib.dms_fill_in(C.byref(existing.c), d.ref, c.ref, C.byref(k), int(passthrough_geom), int(passthrough_rgb), C.byref(out.c), None),
          "dms_fill_in")
    return out


class GlobalModel:
    """Surfel map in HBM (reference class GlobalModel)."""

    def __init__(self, width, height, capacity=1 << 20, handle=None):
        self.width, self.height = width, height
        self._owned = handle is None
        if handle is None:
            h = C.c_void_p()
            check(lib.dms_model_create(C.byref(h), capacity, width, height), "dms_model_create")
            self.h = h
        else:
            self.h = C.c_void_p(handle)
        self.zbuf = DeviceBuffer(width * height * 8)

    def close(self):
        if getattr(self, "h", None) and self._owned:
            lib.dms_model_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def setNumSensors(self, n):
        check(lib.dms_model_set_num_sensors(self.h, int(n)), "dms_model_set_num_sensors")

    def setCleanSuffixMin(self, n):
        check(lib.dms_model_set_clean_suffix_min(self.h, int(n)), "dms_model_set_clean_suffix_min")

    def lastCount(self):
        n = C.c_uint(0)
        check(lib.dms_model_count(self.h, C.byref(n), None), "dms_model_count")
        return n.value

    def upload(self, surfels):
        s = np.ascontiguousarray(surfels, SURFEL_DTYPE)
        check(lib.dms_model_upload(self.h, s.ctypes.data_as(C.c_void_p), len(s), None), "dms_model_upload")

    def downloadMap(self):
        n = self.lastCount()
        out = np.zeros(max(n, 1), SURFEL_DTYPE)
        got = C.c_uint(0)
        check(lib.dms_model_download(self.h, out.ctypes.data_as(C.c_void_p), n, C.byref(got), None), "dms_model_download")
        return out[:got.value].copy()

    def downloadMapRef(self):
        """The reference's 15-float / 60-byte records (Shaders/Vertex.cpp:21-50)."""
        n = self.lastCount()
        out = np.zeros((max(n, 1), 15), np.float32)
        got = C.c_uint(0)
        check(lib.dms_model_download_ref(self.h, out.ctypes.data_as(C.c_void_p), n, C.byref(got), None), "dms_model_download_ref")
        return out[:got.value].copy()

    def savePly(self, path, confidenceThreshold, reference_offsets=False):
        """ElasticFusion::savePly for this map (ElasticFusion.cpp:781-885); returns the number of vertices written."""
        n = C.c_uint(0)
        check(lib.dms_model_save_ply(self.h, os.fsencode(path), C.c_float(confidenceThreshold), int(bool(reference_offsets)), C.byref(n)),
              "dms_model_save_ply")
        return n.value

    # -- map merge (GlobalModel::consume) ----------------------------------------------------
    @staticmethod
    def _T(relativeTransform):
        t = np.ascontiguousarray(relativeTransform, np.float32).reshape(16)
        return t, t.ctypes.data_as(C.POINTER(C.c_float))

    def consume(self, other, relativeTransform):
        """Append `other`'s surfels moved by relativeTransform (4x4); `other` is left untouched."""
        keep, tp = self._T(relativeTransform)
        check(lib.dms_model_consume(self.h, other.h, tp, None), "dms_model_consume")
        check(lib.dms_stream_sync(None))

    def sampleGraph(self, sampleRate=5000):
        """Deformation::sampleGraphModel's samples: n x 4 float32 {pos.xyz, init time}, sorted by init time."""
        cap = int(self.lastCount()) // sampleRate + 2
        out = np.zeros((cap, 4), np.float32)
        n = C.c_int(0)
        check(lib.dms_model_sample_graph(self.h, sampleRate, out.ctypes.data_as(C.POINTER(C.c_float)), cap, C.byref(n), None),
              "dms_model_sample_graph")
        return out[:n.value].copy()

    def exportRecords(self, max_count=None):
        """(DeviceBuffer of 20-float records, count): the device-side form of downloadMap, for p2p transfers."""
        cap = int(lib.dms_model_capacity(self.h)) if max_count is None else int(max_count)
        n_now = min(self.lastCount(), cap)
        buf = DeviceBuffer(max(n_now, 1) * SURFEL_DTYPE.itemsize)
        n = C.c_uint(0)
        check(lib.dms_model_export_records(self.h, C.c_void_p(buf.ptr), n_now, C.byref(n), None), "dms_model_export_records")
        return buf, n.value

    def consumeRecords(self, records_ptr, count, relativeTransform):
        keep, tp = self._T(relativeTransform)
        check(lib.dms_model_consume_records(self.h, C.c_void_p(records_ptr), count, tp, None), "dms_model_consume_records")
        check(lib.dms_stream_sync(None))

    def initialise(self, rgba, depth_metric, depth_metric_filtered, K, time, timeIdx, maxDepth):
        c, dm, dmf = _img(rgba, np.uint8), _img(depth_metric, np.float32), _img(depth_metric_filtered, np.float32)
        k = _cam(K)
        check(lib.dms_model_initialise(self.h, c.ref, dm.ref, dmf.ref, C.byref(k), time, timeIdx, maxDepth, None), "dms_model_initialise")

    def fuse(self, pose, time, timeIdx, rgba, depth_metric, depth_metric_filtered, indexmap, K, depthCutoff, weighting):
        c, dm, dmf = _img(rgba, np.uint8), _img(depth_metric, np.float32), _img(depth_metric_filtered, np.float32)
        k = _cam(K)
        check(lib.dms_model_fuse(self.h, pose.ptr, time, timeIdx, c.ref, dm.ref, dmf.ref, C.byref(indexmap.c), C.byref(k), depthCutoff,
                                 weighting, None, None), "dms_model_fuse")

    def projectIndices(self, pose, time, timeIdx, K, depthCutoff, timeDelta):
        """The index map's z-buffer alone (column-major, in self.zbuf): what fuse(zbuf=True) associates from."""
        k = _cam(K)
        check(lib.dms_index_project(self.h, pose.ptr, C.byref(k), time, timeIdx, depthCutoff, timeDelta, C.c_void_p(self.zbuf.ptr), None),
              "dms_index_project")

    def fuseEx(self, pose, time, timeIdx, rgba, depth_metric, depth_metric_filtered, indexmap, K, depthCutoff, weighting, defer_update=False):
        """fuse() from the index map's images (indexmap) or, with indexmap None, from the z-buffer projectIndices left in self.zbuf.
        defer_update: the association only; applyPending() runs the update pass."""
        c, dm, dmf = _img(rgba, np.uint8), _img(depth_metric, np.float32), _img(depth_metric_filtered, np.float32)
        k = _cam(K)
        im = C.byref(indexmap.c) if indexmap is not None else None
        zb = None if indexmap is not None else C.c_void_p(self.zbuf.ptr)
        check(lib.dms_model_fuse_ex(self.h, pose.ptr, time, timeIdx, c.ref, dm.ref, dmf.ref, im, zb, C.byref(k), depthCutoff, weighting, None,
                                    int(bool(defer_update)), None), "dms_model_fuse_ex")

    def applyPending(self):
        check(lib.dms_model_apply_pending(self.h, None), "dms_model_apply_pending")

    def fuseScratch(self, winners):
        """What the last association left: dict of slot_pos / slot_col / slot_nrm (n x 4 float32), slot_best (uint32), slot_flag
        (uint8) over the (W+1)//2 x (H+1)//2 candidate slots (column-major) and the first `winners` entries of the winner array."""
        n = ((self.width + 1) // 2) * ((self.height + 1) // 2)
        o = {"slot_pos": np.zeros((n, 4), np.float32), "slot_col": np.zeros((n, 4), np.float32), "slot_nrm": np.zeros((n, 4), np.float32),
             "slot_best": np.zeros(n, np.uint32), "slot_flag": np.zeros(n, np.uint8), "winner": np.zeros(max(int(winners), 1), np.uint32)}
        check(lib.dms_model_fuse_scratch(self.h, *[o[k].ctypes.data_as(C.c_void_p) for k in
                                                   ("slot_pos", "slot_col", "slot_nrm", "slot_best", "slot_flag", "winner")],
                                         int(winners), None), "dms_model_fuse_scratch")
        o["winner"] = o["winner"][:int(winners)]
        return o

    def clean(self, pose, time, timeIdx, indexmap, K, confThreshold, timeDelta, maxDepth, graph=None, depth_synth=None, isFern=False):
        k = _cam(K)
        gptr, gn = None, 0
        if graph is not None and len(graph):
            g = np.ascontiguousarray(graph, np.float32).reshape(-1, 16)
            gptr, gn = g.ctypes.data_as(C.POINTER(C.c_float)), len(g)
        dref = None
        if depth_synth is not None:
            self._ds = _img(depth_synth, np.float32)
            dref = self._ds.ref
        check(lib.dms_model_clean(self.h, pose.ptr, time, timeIdx, C.byref(indexmap.c), dref, C.byref(k), confThreshold, gptr, gn, timeDelta,
                                  maxDepth, int(isFern), None), "dms_model_clean")
        check(lib.dms_stream_sync(None))

    def projectOnly(self, pose, K, maxDepth, confThreshold, time, timeIdx, maxTime, timeDelta, active=True):
        """The project pass of a splat prediction alone, into self.zbuf (cleared first); returns the raw 64-bit cells (column-major)."""
        k = _cam(K)
        self.zbuf.upload(np.full(self.width * self.height, Z_CLEAR, np.uint64))
        check(lib.dms_splat_project_only(self.h, pose.ptr, C.byref(k), maxDepth, confThreshold, time, timeIdx, maxTime, timeDelta,
                                         int(bool(active)), C.c_void_p(self.zbuf.ptr), None), "dms_splat_project_only")
        check(lib.dms_stream_sync(None))
        return self.zbuf.download(np.uint64, self.width * self.height)

    def cleanProject(self, pose, time, timeIdx, indexmap, K, confThreshold, timeDelta, maxDepth, projConfThreshold, projTime, projMaxTime,
                     projTimeDelta, active=True):
        """clean() whose scatter pass also projects the new map (dms_model_clean_project) into self.zbuf (cleared first); returns
        (raw 64-bit cells, whether the scatter carried the projection)."""
        k = _cam(K)
        self.zbuf.upload(np.full(self.width * self.height, Z_CLEAR, np.uint64))
        took = C.c_int(0)
        check(lib.dms_model_clean_project(self.h, pose.ptr, time, timeIdx, C.byref(indexmap.c), C.byref(k), confThreshold, timeDelta, maxDepth,
                                          projConfThreshold, projTime, projMaxTime, projTimeDelta, int(bool(active)),
                                          C.c_void_p(self.zbuf.ptr), C.byref(took), None), "dms_model_clean_project")
        check(lib.dms_stream_sync(None))
        return self.zbuf.download(np.uint64, self.width * self.height), bool(took.value)

    def renderPointCloud(self, mvp, threshold, drawUnstable, drawNormals, drawColors, drawPoints, drawWindow, drawTimes,
                         drawContributions, time, timeIdx, timeDelta, clusters=None, drawClusters=False, cluster_colors=None,
                         target=None, size=None, clear_rgba=(0.0, 0.0, 0.0, 0.0), image_order=False, pose_dev=None, stream=None,
                         context=None):
        """GlobalModel::renderPointCloud (GlobalModel.cpp:419-505) with the reference's parameters in the reference's order.

        clusters: the clusters drawn, one draw each into one target (the reference's loop over cluster_vbos; default: this map alone).
        As in the reference they are cluster ids, resolved through `context` (the ElasticFusion whose map this is: its
        globalModel(id); an id without buffers draws nothing) - or GlobalModel objects, drawn as they are.
        cluster_colors[i] colours clusters[i] when drawClusters.  target: a RenderTarget drawn into as it is; without one a target of
        `size` = (width, height) (default: the map's camera size) is created and cleared to clear_rgba.  Returns the numpy images of
        RenderTarget.images (window rows unless image_order)."""
        models = [self] if clusters is None else list(clusters)
        own = target is None
        if own:
            w, h = size if size is not None else (self.width, self.height)
            target = RenderTarget(w, h)
            target.clear(clear_rgba, stream)
        ct = color_type(drawNormals, drawColors, drawTimes, drawContributions)
        for i, m in enumerate(models):
            if not isinstance(m, GlobalModel):
                if context is None:
                    raise TypeError("cluster ids need the context that owns the clusters (context=)")
                m = context.globalModel(int(m))
                if m is None:
                    continue
            cc = cluster_colors[i] if drawClusters else None
            target.draw(m, mvp, threshold, drawUnstable, drawPoints, drawWindow, ct, time, timeIdx, timeDelta, cc, pose_dev, stream)
        out = target.images(image_order, stream)
        if own:
            target.close()
        return out


class IndexMap:
    """Model rendering into the camera (reference class IndexMap)."""

    def __init__(self, width, height):
        self.width, self.height = width, height
        f4 = np.dtype((np.float32, (4,)))
        self.index = DeviceImage(height, width, np.uint32)
        self.vertConf = DeviceImage(height, width, f4)
        self.colorTime = DeviceImage(height, width, f4)
        self.normRad = DeviceImage(height, width, f4)
        self.c = IndexMapOut(self.index.view, self.vertConf.view, self.colorTime.view, self.normRad.view)
        self.active = PredictionImages(height, width)
        self.inactive = PredictionImages(height, width)
        self.depth = DeviceImage(height, width, np.float32)

    def predictIndices(self, pose, time, timeIdx, model, K, depthCutoff, timeDelta):
        k = _cam(K)
        check(lib.dms_index_map(model.h, pose.ptr, C.byref(k), time, timeIdx, depthCutoff, timeDelta, C.c_void_p(model.zbuf.ptr),
                                C.byref(self.c), None), "dms_index_map")

    def combinedPredict(self, pose, model, K, depthCutoff, confThreshold, time, timeIdx, maxTime, timeDelta, active=True):
        k = _cam(K)
        tgt = self.active if active else self.inactive
        check(lib.dms_splat_predict(model.h, pose.ptr, C.byref(k), depthCutoff, confThreshold, time, timeIdx, maxTime, timeDelta,
                                    1 if active else 0, C.c_void_p(model.zbuf.ptr), C.byref(tgt.c), None), "dms_splat_predict")
        return tgt

    def synthesizeDepth(self, pose, model, K, depthCutoff, confThreshold, time, timeIdx, maxTime, timeDelta):
        k = _cam(K)
        check(lib.dms_splat_depth(model.h, pose.ptr, C.byref(k), depthCutoff, confThreshold, time, timeIdx, maxTime, timeDelta,
                                  C.c_void_p(model.zbuf.ptr), self.depth.ref, None), "dms_splat_depth")
        return self.depth

    def download_index(self):
        return self.index.download(), self.vertConf.download(), self.colorTime.download(), self.normRad.download()


_IMG_TYPES = {0: (np.uint8, 4), 1: (np.uint16, 1), 2: (np.uint16, 1), 3: (np.float32, 1), 4: (np.float32, 1), 5: (np.uint32, 1),
              6: (np.float32, 4), 7: (np.float32, 4), 8: (np.float32, 4), 9: (np.uint8, 4), 10: (np.float32, 4), 11: (np.float32, 4),
              12: (np.uint16, 1), 13: (np.uint8, 4), 14: (np.float32, 4), 15: (np.float32, 4),
              16: (np.uint8, 4), 17: (np.float32, 4), 18: (np.float32, 4), 19: (np.uint16, 1)}


class ElasticFusion:
    """One camera's frame step (ElasticFusion::processFrame with --o --nkf)."""

    def __init__(self, width, height, K, **opts):
        p = FusionParams()
        lib.dms_fusion_default_params(C.byref(p), width, height, K[0], K[1], K[2], K[3])
        for k, v in opts.items():
            if not hasattr(p, k):
                raise TypeError("unknown option %r" % k)
            setattr(p, k, v)
        self.params = p
        h = C.c_void_p()
        check(lib.dms_fusion_create(C.byref(h), C.byref(p)), "dms_fusion_create")
        self.h = h
        self.width, self.height = width, height
        self._rgb = DeviceBuffer(width * height * 4)
        self._depth = DeviceBuffer(width * height * 2)

    def close(self):
        if getattr(self, "h", None):
            lib.dms_fusion_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload_frame(self, rgb, depth, stream=None):
        # the previous frame's ingest (internal prep stream) may not have read the staging buffers yet
        check(lib.dms_fusion_inputs_consumed(self.h, stream), "dms_fusion_inputs_consumed")
        rgb = np.ascontiguousarray(rgb, np.uint8)
        self._rgb.upload(rgb)
        self._depth.upload(np.ascontiguousarray(depth, np.uint16))
        return rgb.shape[2]

    def inputsReady(self, producer_stream=None):
        """The next frame's input buffers are produced by work enqueued on `producer_stream` so far."""
        check(lib.dms_fusion_inputs_ready(self.h, producer_stream), "dms_fusion_inputs_ready")

    def processFrameAsync(self, rgb_ptr, channels, depth_ptr, inPose=None, weightMultiplier=1.0, stream=None):
        pp = None
        if inPose is not None:
            self._pose = np.ascontiguousarray(inPose, np.float32).reshape(16)
            pp = self._pose.ctypes.data_as(C.POINTER(C.c_float))
        check(lib.dms_fusion_process_frame(self.h, C.c_void_p(rgb_ptr), channels, C.c_void_p(depth_ptr), pp, weightMultiplier, stream),
              "dms_fusion_process_frame")

    def processFrameBegin(self, rgb, depth, inPose=None, weightMultiplier=1.0, stream=None):
        ch = self.upload_frame(rgb, depth, stream)
        pp = None
        if inPose is not None:
            self._pose = np.ascontiguousarray(inPose, np.float32).reshape(16)
            pp = self._pose.ctypes.data_as(C.POINTER(C.c_float))
        check(lib.dms_fusion_process_frame_begin(self.h, C.c_void_p(self._rgb.ptr), ch, C.c_void_p(self._depth.ptr), pp, weightMultiplier,
                                                 stream), "dms_fusion_process_frame_begin")

    # -- after a map merge (ReferenceFrame::consumeReferenceFrame): several cameras, one map ------------------
    def joinMap(self, owner, relativeTransform, stream=None):
        """`owner`'s map consumes this camera's map (moved by relativeTransform); this camera's pose is re-based and its later
        frames track against / fuse into owner's map.  Both contexts in this process, driven from one thread and stream."""
        t, tp = _f16(relativeTransform)
        check(lib.dms_fusion_join_map(self.h, owner.h, tp, stream), "dms_fusion_join_map")
        self._owner = owner  # must outlive this context

    def importCamera(self, owner, pose, tick, last_rgb_ptr, channels, last_depth_ptr, stream=None):
        """This fresh context becomes a camera that arrives from another rank: `pose` (already in owner's frame), `tick`, and the
        last frame it processed (device pointers), from which the live state is rebuilt.  Joins owner's map; fuses nothing."""
        t, tp = _f16(pose)
        check(lib.dms_fusion_import_camera(self.h, owner.h, tp, int(tick), C.c_void_p(last_rgb_ptr), int(channels), C.c_void_p(last_depth_ptr),
                                           stream), "dms_fusion_import_camera")
        self._owner = owner

    def setOrbLoop(self, orbTcwOld, orbTcwNew):
        """Arm the next processFrameBegin with an ORB loop closure (ElasticFusion.cpp:292-350); None, None disarms."""
        if orbTcwOld is None or orbTcwNew is None:
            check(lib.dms_fusion_set_orb_loop(self.h, None, None), "dms_fusion_set_orb_loop")
            return
        self._orb = (np.ascontiguousarray(orbTcwOld, np.float32).reshape(16), np.ascontiguousarray(orbTcwNew, np.float32).reshape(16))
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        check(lib.dms_fusion_set_orb_loop(self.h, fp(self._orb[0]), fp(self._orb[1])), "dms_fusion_set_orb_loop")

    def globalLoopConstraints(self, stream=None):
        """Constraint rows of the last ORB loop closure: n x 7 float32 {orbTcwOld * p, orbTcwNew * p, INACTIVE time}."""
        n = C.c_int(0)
        cap = (self.width // 20) * (self.height // 20)
        out = np.zeros((cap, 7), np.float32)
        check(lib.dms_fusion_get_global_loop_constraints(self.h, out.ctypes.data_as(C.POINTER(C.c_float)), cap, C.byref(n), stream),
              "dms_fusion_get_global_loop_constraints")
        return out[:n.value].copy()

    def applyGlobalLoopBegin(self, orbTcwOld, orbTcwNew, stream=None):
        """ElasticFusion::applyGlobalLoop up to the constraints (ElasticFusion.cpp:1148-1200)"""
        a = np.ascontiguousarray(orbTcwOld, np.float32).reshape(16)
        b = np.ascontiguousarray(orbTcwNew, np.float32).reshape(16)
        fp = lambda v: v.ctypes.data_as(C.POINTER(C.c_float))
        check(lib.dms_fusion_apply_global_loop_begin(self.h, fp(a), fp(b), stream), "dms_fusion_apply_global_loop_begin")

    def applyGlobalLoopEnd(self, graph=None, accepted=False, stream=None):
        """... and from Deformation::constrain's outcome on: predict, predictIndices, clean with the graph (:1222-1239)"""
        gp, nn = None, 0
        if graph is not None and len(graph):
            self._graph = np.ascontiguousarray(graph, np.float32).reshape(-1, 16)
            gp, nn = self._graph.ctypes.data_as(C.POINTER(C.c_float)), len(self._graph)
        check(lib.dms_fusion_apply_global_loop_end(self.h, gp, nn, int(bool(accepted)), stream), "dms_fusion_apply_global_loop_end")

    def fetchLoop(self, stream=None):
        r = FrameResult()
        check(lib.dms_fusion_fetch_loop(self.h, C.byref(r), stream), "dms_fusion_fetch_loop")
        return r

    def processFrameEnd(self, graph=None, newPose=None, stream=None):
        gp, nn, pp = None, 0, None
        if graph is not None and len(graph):
            self._graph = np.ascontiguousarray(graph, np.float32).reshape(-1, 16)
            gp, nn = self._graph.ctypes.data_as(C.POINTER(C.c_float)), len(self._graph)
        if newPose is not None:
            self._newpose = np.ascontiguousarray(newPose, np.float32).reshape(16)
            pp = self._newpose.ctypes.data_as(C.POINTER(C.c_float))
        check(lib.dms_fusion_process_frame_end(self.h, gp, nn, pp, stream), "dms_fusion_process_frame_end")

    def fetch(self, stream=None):
        r = FrameResult()
        check(lib.dms_fusion_fetch(self.h, C.byref(r), stream), "dms_fusion_fetch")
        return r

    def fetch_rc(self, stream=None):
        """(status, result): like fetch, but hands DMS_ERR_CAPACITY / DMS_ERR_TIMEOUT back with the (valid) result."""
        r = FrameResult()
        return int(lib.dms_fusion_fetch(self.h, C.byref(r), stream)), r

    def poseDevice(self):
        """device address of the 4x4 pose the frame step keeps in HBM"""
        return int(lib.dms_fusion_pose_device(self.h))

    def exportPose(self, dst_ptr, stream=None):
        """copy the pose (16 floats) from its place in HBM to device memory at dst_ptr, stream ordered"""
        check(lib.dms_memcpy_d2d_async(C.c_void_p(dst_ptr), C.c_void_p(self.poseDevice()), 64, stream), "dms_memcpy_d2d_async")

    def odometryHandle(self):
        return C.c_void_p(lib.dms_fusion_odometry(self.h))

    def processFrame(self, rgb, depth, inPose=None, weightMultiplier=1.0, cluster=None):
        if cluster is not None:
            self.setCluster(cluster)
        ch = self.upload_frame(rgb, depth)
        self.processFrameAsync(self._rgb.ptr, ch, self._depth.ptr, inPose, weightMultiplier)
        return self.fetch()

    def globalModel(self, cluster=None):
        """The current cluster's map (GlobalModel::model()), or the map of `cluster` (None if it has no buffers)."""
        if cluster is None:
            return GlobalModel(self.width, self.height, handle=lib.dms_fusion_model(self.h))
        h = lib.dms_fusion_cluster_model(self.h, int(cluster))
        return GlobalModel(self.width, self.height, handle=h) if h else None

    # -- per-cluster surfel buffers (processFrame's `cluster`, GlobalModel::isCluster / clusters) ------------
    def setCluster(self, cluster):
        check(lib.dms_fusion_set_cluster(self.h, int(cluster)), "dms_fusion_set_cluster")

    def computeFeedbackBuffers(self, stream=None):
        check(lib.dms_fusion_compute_feedback(self.h, stream), "dms_fusion_compute_feedback")

    def renderCloud(self, target, which, mvp=None, model_pose=None, color_type=0, pose_dev=None, model_pose_dev=None, stream=None):
        """One live-frame cloud (dms_fusion_render_cloud) into `target` (a RenderTarget): which = CLOUD_RAW / CLOUD_FILTERED of the
        feedback inputs; model_pose (host 4 x 4, default identity) or model_pose_dev (device address, e.g. poseDevice()) is the
        program's `pose`; mvp / pose_dev are the view as in RenderTarget.draw."""
        p = _cloud_params(mvp, model_pose, color_type, pose_dev, model_pose_dev)
        check(lib.dms_fusion_render_cloud(target.h, self.h, int(which), C.byref(p), stream), "dms_fusion_render_cloud")

    def drawPanels(self, target, panels, viewports, depth_cutoff, which_mask=15, stream=None):
        """The GUI's image column in one launch (dms_fusion_draw_panels): viewports = four (x, y, w, h) for DEPTH_NORM, Model, RGB,
        ModelImage; depth_cutoff is gui->depthCutoff."""
        vps = (Viewport * 4)(*[Viewport(*[int(v) for v in vp]) for vp in viewports])
        check(lib.dms_fusion_draw_panels(target.h, panels.h, self.h, vps, float(depth_cutoff), int(which_mask), stream), "dms_fusion_draw_panels")


    def drawPanelsSeparately(self, target, panels, viewports, depth_cutoff, which_mask=15, stream=None):
        """The same column as the reference issues it (MainController.cpp:649-664): normaliseDepth, renderDepth and one displayImg per
        panel, six launches."""
        views = {}
        for k, img in ((PANEL_DEPTH_NORM, 1), (PANEL_MODEL, 10), (PANEL_RGB, 0), (PANEL_MODEL_IMAGE, 9)):
            views[k] = Image2D()
            check(lib.dms_fusion_get_image(self.h, img, C.byref(views[k])), "dms_fusion_get_image")
        cut = np.float32(depth_cutoff)
        check(lib.dms_depth_norm(panels.h, C.byref(views[PANEL_DEPTH_NORM]), float(np.float32(0.3) * np.float32(1000.0)), float(cut * np.float32(1000.0)),
                                 stream), "dms_depth_norm")
        check(lib.dms_model_depth_image(panels.h, C.byref(views[PANEL_MODEL]), float(cut), stream), "dms_model_depth_image")
        white = (C.c_float * 3)(1.0, 1.0, 1.0)
        for k in range(4):
            if not (which_mask >> k) & 1:
                continue
            vp = Viewport(*[int(v) for v in viewports[k]])
            if k in (PANEL_DEPTH_NORM, PANEL_MODEL):
                panels.blit(target, k, viewports[k], stream=stream)
            else:
                check(lib.dms_render_blit(target.h, C.byref(views[k]), PANEL_RGBA8, PANEL_LINEAR if k == PANEL_RGB else PANEL_NEAREST, C.byref(vp),
                                          white, stream), "dms_render_blit")

    def feedbackBuffers(self):
        """Context::feedbackBuffers(): {FeedbackBuffer.RAW: ..., FeedbackBuffer.FILTERED: ...}"""
        return {FeedbackBuffer.RAW: FeedbackBuffer(self, CLOUD_RAW), FeedbackBuffer.FILTERED: FeedbackBuffer(self, CLOUD_FILTERED)}

    def clusters(self):
        """(ids, current id)"""
        ids = (C.c_int * 64)()
        n, cur = C.c_int(0), C.c_int(0)
        check(lib.dms_fusion_clusters(self.h, ids, 64, C.byref(n), C.byref(cur)), "dms_fusion_clusters")
        return [int(ids[i]) for i in range(min(n.value, 64))], int(cur.value)

    def image(self, which):
        v = Image2D()
        check(lib.dms_fusion_get_image(self.h, which, C.byref(v)), "dms_fusion_get_image")
        dt, k = _IMG_TYPES[which]
        return capi.download_view(v, dt, k)

    def imagePtr(self, which):
        """device pointer of one of the context's dense images (dms_fusion_get_image ids; 13 / 14 / 15 = fill-in colour / vertex / normal)"""
        v = Image2D()
        check(lib.dms_fusion_get_image(self.h, which, C.byref(v)), "dms_fusion_get_image")
        return int(v.data)

    def thumbnails(self, block_ptr, stream=None):
        """Pack this frame's W/8 x H/8 fill-in thumbnails [image | vertex | normal] into device memory at block_ptr."""
        check(lib.dms_fusion_thumbnails(self.h, C.c_void_p(block_ptr), stream), "dms_fusion_thumbnails")

    def frameBlock(self, block_ptr, pose_ptr, tick_ptr, tick, stream=None):
        """thumbnails + pose (16 floats) + tick of this frame into device memory, one launch"""
        check(lib.dms_fusion_frame_block(self.h, C.c_void_p(block_ptr), C.c_void_p(pose_ptr), C.c_void_p(tick_ptr), int(tick), stream),
              "dms_fusion_frame_block")

    def armFrameBlock(self, block_ptr, pose_ptr, tick_ptr, tick):
        """the same block written by the NEXT frame's own last kernel (no launch of its own); frameBlockWritten() tells whether it was"""
        check(lib.dms_fusion_arm_frame_block(self.h, C.c_void_p(block_ptr), C.c_void_p(pose_ptr), C.c_void_p(tick_ptr), int(tick)),
              "dms_fusion_arm_frame_block")

    def frameBlockWritten(self):
        return bool(lib.dms_fusion_frame_block_written(self.h))

    def lazyStats(self):
        """lazy_final_prediction: {eager, deferred, materialised, stale} (dms_fusion_get_lazy_stats)"""
        e, d, m, st = C.c_int(0), C.c_long(0), C.c_long(0), C.c_long(0)
        check(lib.dms_fusion_get_lazy_stats(self.h, C.byref(e), C.byref(d), C.byref(m), C.byref(st)), "dms_fusion_get_lazy_stats")
        return {"eager": bool(e.value), "deferred": int(d.value), "materialised": int(m.value), "stale": int(st.value)}

    def cleanProjectStats(self):
        """fused_clean_projection: {fused, separate} cleans of the frame step so far (dms_fusion_get_clean_project_stats)"""
        a, b = C.c_long(0), C.c_long(0)
        check(lib.dms_fusion_get_clean_project_stats(self.h, C.byref(a), C.byref(b)), "dms_fusion_get_clean_project_stats")
        return {"fused": int(a.value), "separate": int(b.value)}

    def predictStats(self):
        """fused_model_prediction: {fused, plain} tracking predictions so far (dms_fusion_get_predict_stats)"""
        a, b = C.c_long(0), C.c_long(0)
        check(lib.dms_fusion_get_predict_stats(self.h, C.byref(a), C.byref(b)), "dms_fusion_get_predict_stats")
        return {"fused": int(a.value), "plain": int(b.value)}

    def loopConstraints(self):
        """Surface constraints of the last fetched frame's loop candidate: n x 7 float32
        {worldRawPoint, worldModelPoint, source time} (ElasticFusion.cpp:446-474)."""
        n = C.c_int(0)
        cap = (self.width // 20) * (self.height // 20)
        out = np.zeros((cap, 7), np.float32)
        check(lib.dms_fusion_get_loop_constraints(self.h, out.ctypes.data_as(C.POINTER(C.c_float)), cap, C.byref(n)),
              "dms_fusion_get_loop_constraints")
        return out[:n.value].copy()

    def setLoopSolver(self, on=True, sampleRate=5000):
        """processFrame closes its local loops itself (dms_fusion_set_loop_solver): Deformation::constrain runs on the GPU"""
        lib.dms_fusion_set_loop_solver.argtypes = [_P, _I, _I]
        check(lib.dms_fusion_set_loop_solver(self.h, int(bool(on)), int(sampleRate)), "dms_fusion_set_loop_solver")

    def deformation(self):
        """The context's solver as a deform.Deformation view (None until the loop solver was first switched on)"""
        from . import deform

        lib.dms_fusion_deformation.restype = C.c_void_p
        lib.dms_fusion_deformation.argtypes = [_P]
        h = lib.dms_fusion_deformation(self.h)
        return deform.Deformation.view(h, (self.width // 20) * (self.height // 20)) if h else None

    def deforms(self):
        """ElasticFusion::getDeforms: frames whose local loop was closed by the loop solver"""
        lib.dms_fusion_get_deforms.argtypes = [_P]
        return int(lib.dms_fusion_get_deforms(self.h))

    def relativeConstraints(self):
        """context.relativeCons(): n x 8 float32 {deformed source, target, source time, target time}"""
        lib.dms_fusion_get_relative_constraints.argtypes = [_P, C.POINTER(C.c_float), _I, C.POINTER(C.c_int)]
        n = C.c_int(0)
        check(lib.dms_fusion_get_relative_constraints(self.h, None, 0, C.byref(n)), "dms_fusion_get_relative_constraints")
        out = np.zeros((max(1, n.value), 8), np.float32)
        check(lib.dms_fusion_get_relative_constraints(self.h, out.ctypes.data_as(C.POINTER(C.c_float)), n.value, C.byref(n)),
              "dms_fusion_get_relative_constraints")
        return out[:n.value].copy()

    def setGlobalLoopSolver(self, on=True, max_poses=4096):
        """A processFrame armed by setOrbLoop, and applyGlobalLoop, close the ORB loop themselves (dms_fusion_set_global_loop_solver);
        the context keeps its pose graph while this is on"""
        lib.dms_fusion_set_global_loop_solver.argtypes = [_P, _I, _I]
        check(lib.dms_fusion_set_global_loop_solver(self.h, int(bool(on)), int(max_poses)), "dms_fusion_set_global_loop_solver")
        self._max_poses = int(max_poses)

    def applyGlobalLoop(self, orbTcwOld, orbTcwNew, stream=None):
        """ElasticFusion::applyGlobalLoop (ElasticFusion.cpp:1148-1240) in one call, the solve on the GPU"""
        a = np.ascontiguousarray(orbTcwOld, np.float32).reshape(16)
        b = np.ascontiguousarray(orbTcwNew, np.float32).reshape(16)
        fp = lambda v: v.ctypes.data_as(C.POINTER(C.c_float))
        lib.dms_fusion_apply_global_loop.argtypes = [_P, C.POINTER(C.c_float), C.POINTER(C.c_float), _P]
        check(lib.dms_fusion_apply_global_loop(self.h, fp(a), fp(b), stream), "dms_fusion_apply_global_loop")

    def globalDeformation(self):
        """The context's global solver as a deform.GlobalDeformation view (None until the global loop solver was first switched on)"""
        from . import deform

        lib.dms_fusion_global_deformation.restype = C.c_void_p
        lib.dms_fusion_global_deformation.argtypes = [_P]
        h = lib.dms_fusion_global_deformation(self.h)
        if not h:
            return None
        d = deform.GlobalDeformation.view(h, (self.width // 20) * (self.height // 20), deform.MAX_GLOBAL_NODES)
        d.max_relative, d.max_poses = deform.MAX_RELATIVE, self._max_poses
        return d

    def fernDeforms(self):
        """ElasticFusion::getFernDeforms: ORB loops the global loop solver closed"""
        lib.dms_fusion_get_fern_deforms.argtypes = [_P]
        return int(lib.dms_fusion_get_fern_deforms(self.h))

    def poseGraph(self):
        """Context::poseGraph(): (ticks int64, poses n x 4 x 4 float32)"""
        lib.dms_fusion_get_pose_graph.argtypes = [_P, C.POINTER(C.c_longlong), C.POINTER(C.c_float), _I, C.POINTER(C.c_int)]
        n = C.c_int(0)
        check(lib.dms_fusion_get_pose_graph(self.h, None, None, 0, C.byref(n)), "dms_fusion_get_pose_graph")
        t, p = np.zeros(max(1, n.value), np.int64), np.zeros((max(1, n.value), 4, 4), np.float32)
        check(lib.dms_fusion_get_pose_graph(self.h, t.ctypes.data_as(C.POINTER(C.c_longlong)), p.ctypes.data_as(C.POINTER(C.c_float)), n.value,
                                            C.byref(n)), "dms_fusion_get_pose_graph")
        return t[:n.value].copy(), p[:n.value].copy()

    OPTIONS = {"rgbOnly": 0, "icpWeight": 1, "pyramid": 2, "fastOdom": 3, "so3": 4, "frameToFrameRGB": 5, "confidence": 6, "depthCut": 7}

    def setOption(self, name, value):
        """The reference's run-time setters (ElasticFusion.cpp:1023-1043): setRgbOnly, setIcpWeight, setPyramid, ..."""
        check(lib.dms_fusion_set_option(self.h, self.OPTIONS[name], C.c_double(float(value))), "dms_fusion_set_option")

    def getOption(self, name):
        v = C.c_double(0.0)
        check(lib.dms_fusion_get_option(self.h, self.OPTIONS[name], C.byref(v)), "dms_fusion_get_option")
        return v.value

    def set_profiling(self, on):
        check(lib.dms_fusion_set_profiling(self.h, int(on)))

    def kernel_time(self, name):
        ms, n = C.c_double(0), C.c_int(0)
        check(lib.dms_fusion_get_kernel_time(self.h, name.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value


class ReferenceFrameRefiner:
    """ReferenceFrame's m_index + m_rgbd and the second half of resolveRelativeTransformationFern (ReferenceFrame.h:66-110):
    dms_refframe_* (include/dmslam_fusion.h)."""

    def __init__(self, width, height, K):
        h = C.c_void_p()
        check(lib.dms_refframe_create(C.byref(h), width, height, float(K[2]), float(K[3]), float(K[0]), float(K[1])), "dms_refframe_create")
        self.h, self.width, self.height = h, width, height

    def close(self):
        if getattr(self, "h", None):
            lib.dms_refframe_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def refine(self, owner, recoveryPose, currPose, vertex_ptr, normal_ptr, image_ptr, timeIdx, maxTime, covThresh=1e-05, icpErrThresh=2e-05,
               icpCountThresh=35000, stream=None):
        """owner: the fusion.ElasticFusion whose map was matched (its maxDepthProcessed - truncated to int like the reference's
        `const int depthCutoff` -, confidence and timeDelta are the call's); vertex / normal / image: device pointers to the
        querying camera's dense fill-in textures (RGBA32F, RGBA32F, RGBA8)."""
        r = InterMapResult()
        p = owner.params
        (_ra, rp), (_ca, cp) = _f16(recoveryPose), _f16(currPose)
        check(lib.dms_refframe_refine(self.h, lib.dms_fusion_model(owner.h), rp, cp, C.c_void_p(vertex_ptr),
                                      C.c_void_p(normal_ptr), C.c_void_p(image_ptr), int(p.maxDepthProcessed), float(owner.getOption("confidence")),
                                      int(timeIdx), int(p.timeDelta), int(maxTime), float(covThresh), float(icpErrThresh), float(icpCountThresh),
                                      C.byref(r), stream), "dms_refframe_refine")
        return r

    def prediction(self):
        """the INACTIVE prediction of the last refinement: (image u8 HxWx4, vertex f32 HxWx4, normal f32 HxWx4)"""
        v = PredictOut()
        check(lib.dms_refframe_get_prediction(self.h, C.byref(v)), "dms_refframe_get_prediction")
        return capi.download_view(v.image, np.uint8, 4), capi.download_view(v.vertex, np.float32, 4), capi.download_view(v.normal, np.float32, 4)


# ---- the map draw: GlobalModel::renderPointCloud (include/dmslam_render.h) ------------------------------------------------
class RenderParams(C.Structure):
    """dms_render_params"""
    _fields_ = [("mvp", C.c_float * 16), ("pose_dev", _P), ("threshold", C.c_float), ("draw_unstable", _I), ("draw_points", _I),
                ("draw_window", _I), ("color_type", _I), ("time", _I), ("time_idx", _I), ("time_delta", _I),
                ("use_cluster_color", _I), ("cluster_color", C.c_float * 3)]


lib.dms_render_target_create.argtypes = [C.POINTER(_P), _I, _I]
lib.dms_render_target_destroy.argtypes = [_P]
lib.dms_render_clear.argtypes = [_P, C.POINTER(C.c_float), _P]
lib.dms_render_draw.argtypes = [_P, _P, C.POINTER(RenderParams), _P]
lib.dms_render_images.argtypes = [_P, _I2, _I2, _I2]
lib.dms_render_frustum.argtypes = [_I, _I, _F, _F, _F, _F, _F, _F, C.POINTER(C.c_float)]
lib.dms_render_mvp_from_pose.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]


def render_frustum(w, h, fu, fv, u0, v0, znear, zfar):
    """pangolin::ProjectionMatrix(w, h, fu, fv, u0, v0, znear, zfar) as a row-major float 4 x 4 (dms_render_frustum)."""
    o, op = _f16(np.zeros(16, np.float32))
    check(lib.dms_render_frustum(int(w), int(h), fu, fv, u0, v0, znear, zfar, op), "dms_render_frustum")
    return o.reshape(4, 4)


def render_mvp_from_pose(proj, pose):
    """proj * diag(1, -1, -1, 1) * inverse(pose) in the draw's fp32 order (dms_render_mvp_from_pose)."""
    (_a, ap), (_b, bp) = _f16(proj), _f16(pose)
    o, op = _f16(np.zeros(16, np.float32))
    check(lib.dms_render_mvp_from_pose(ap, bp, op), "dms_render_mvp_from_pose")
    return o.reshape(4, 4)


def color_type(drawNormals=False, drawColors=False, drawTimes=False, drawContributions=False):
    """renderPointCloud's colorType precedence (GlobalModel.cpp:436-440)."""
    return 4 if drawContributions else 1 if drawNormals else 2 if drawColors else 3 if drawTimes else 0


class RenderTarget:
    """A W x H render target in HBM (colour RGBA8, 24-bit depth, winner key); rows are window rows (row 0 = bottom)."""

    def __init__(self, width, height):
        self.width, self.height = int(width), int(height)
        h = C.c_void_p()
        check(lib.dms_render_target_create(C.byref(h), self.width, self.height), "dms_render_target_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            lib.dms_render_target_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def clear(self, rgba=(0.0, 0.0, 0.0, 0.0), stream=None):
        c = (C.c_float * 4)(*[float(v) for v in rgba])
        check(lib.dms_render_clear(self.h, c, stream), "dms_render_clear")

    def draw(self, model, mvp=None, threshold=0.0, draw_unstable=False, draw_points=False, draw_window=False, color_type=0, time=0,
             time_idx=0, time_delta=0, cluster_color=None, pose_dev=None, stream=None):
        """One draw of `model` (a GlobalModel or a dms_model handle).  With pose_dev (device address of a camera-to-world pose),
        `mvp` is the projection and the view is built on the device."""
        p = RenderParams()
        m = np.ascontiguousarray(np.eye(4, dtype=np.float32) if mvp is None else mvp, np.float32).reshape(16)
        for k in range(16):
            p.mvp[k] = float(m[k])
        p.pose_dev = pose_dev
        p.threshold = float(threshold)
        p.draw_unstable, p.draw_points, p.draw_window = int(bool(draw_unstable)), int(bool(draw_points)), int(bool(draw_window))
        p.color_type, p.time, p.time_idx, p.time_delta = int(color_type), int(time), int(time_idx), int(time_delta)
        if cluster_color is not None:
            p.use_cluster_color = 1
            for k in range(3):
                p.cluster_color[k] = float(cluster_color[k])
        h = model.h if isinstance(model, GlobalModel) else C.c_void_p(model)
        check(lib.dms_render_draw(self.h, h, C.byref(p), stream), "dms_render_draw")

    def images(self, image_order=False, stream=None):
        """(rgba u8 HxWx4, depth24 u32 HxW, winner key u64 HxW) after the work enqueued on `stream`; image_order flips the rows
        so that row 0 is the top of the view."""
        check(lib.dms_stream_sync(stream), "dms_stream_sync")
        c, d, w = Image2D(), Image2D(), Image2D()
        check(lib.dms_render_images(self.h, C.byref(c), C.byref(d), C.byref(w)), "dms_render_images")
        out = (capi.download_view(c, np.uint8, 4), capi.download_view(d, np.uint32), capi.download_view(w, np.uint64))
        return tuple(a[::-1].copy() for a in out) if image_order else out


# ---- the shaded view: GUI::drawFXAA (include/dmslam_render_shaded.h) -----------------------------------------------------
lib.dms_render_offscreen_create.argtypes = [C.POINTER(_P), _I, _I]
lib.dms_render_offscreen_destroy.argtypes = [_P]
lib.dms_render_shaded_draw.argtypes = [_P, _P, C.POINTER(RenderParams), C.POINTER(C.c_float), _F, C.POINTER(C.c_float), _P]
lib.dms_render_fxaa.argtypes = [_P, _P, _P]
lib.dms_render_offscreen_images.argtypes = [_P, _I2, _I2, _I2]
OFFSCREEN_SIZE = (3840, 2160)  # the GUI's offscreen buffer (GUI.h:57)


def fxaa_clear_colour(showcaseMode=False):
    """drawFXAA's clear colour (GUI.h:374-377)"""
    return (1.0, 1.0, 1.0, 0.0) if showcaseMode else (0.05, 0.05, 0.3, 0.0)


class ShadedView:
    """GUI::drawFXAA (GUI/src/Tools/GUI.h:365-478): an offscreen float buffer (default the GUI's 3840 x 2160) and the W x H view it
    is resolved into (a RenderTarget, `self.target`).  draw() is stage A (Phong into the buffer), fxaa() stage B (FXAA into the view,
    then the depth blit); drawFXAA() is the GUI's call.  Rows are window rows (row 0 = bottom)."""

    def __init__(self, width, height, offscreen=OFFSCREEN_SIZE):
        self.target = RenderTarget(width, height)
        self.width, self.height = self.target.width, self.target.height
        self.off_width, self.off_height = int(offscreen[0]), int(offscreen[1])
        h = C.c_void_p()
        check(lib.dms_render_offscreen_create(C.byref(h), self.off_width, self.off_height), "dms_render_offscreen_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            lib.dms_render_offscreen_destroy(self.h)
            self.h = None
        if getattr(self, "target", None) is not None:
            self.target.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def clear(self, rgba=(0.0, 0.0, 0.0, 0.0), stream=None):
        """glClear of the view (the GUI clears it before the maps are drawn)"""
        self.target.clear(rgba, stream)

    def draw(self, model, mvp=None, light_pos=(0.0, 0.0, 0.0), sign_mult=-1.0, clear_rgba=fxaa_clear_colour(), threshold=0.0,
             draw_unstable=False, draw_window=False, color_type=0, time=0, time_idx=0, time_delta=0, pose_dev=None, stream=None):
        """Stage A (dms_render_shaded_draw): clear the buffer, draw `model` with the Phong program.  With pose_dev, `mvp` is the
        projection and the view is built on the device."""
        p = RenderParams()
        m = np.ascontiguousarray(np.eye(4, dtype=np.float32) if mvp is None else mvp, np.float32).reshape(16)
        for k in range(16):
            p.mvp[k] = float(m[k])
        p.pose_dev = pose_dev
        p.threshold = float(threshold)
        p.draw_unstable, p.draw_window = int(bool(draw_unstable)), int(bool(draw_window))
        p.color_type, p.time, p.time_idx, p.time_delta = int(color_type), int(time), int(time_idx), int(time_delta)
        lp = (C.c_float * 3)(*[float(v) for v in light_pos])
        cc = (C.c_float * 4)(*[float(v) for v in clear_rgba])
        h = model.h if isinstance(model, GlobalModel) else C.c_void_p(model)
        check(lib.dms_render_shaded_draw(self.h, h, C.byref(p), lp, float(sign_mult), cc, stream), "dms_render_shaded_draw")

    def fxaa(self, stream=None):
        """Stage B (dms_render_fxaa): the buffer through FXAA into the view, then its depth and winners blitted over the view's"""
        check(lib.dms_render_fxaa(self.target.h, self.h, stream), "dms_render_fxaa")

    def drawFXAA(self, mvp, mv, model, threshold, time, timeIdx, timeDelta, invertNormals, drawNormals=False, drawColors=False,
                 drawTimes=False, drawUnstable=False, drawWindow=False, showcaseMode=False, stream=None):
        """GUI::drawFXAA with the reference's arguments in the reference's order, then the GUI's toggles.  mvp and mv are row-major
        (pangolin's OpenGlMatrix transposed); lightpos is mv's translation column (GUI.h:404-408), signMult +1 with invertNormals,
        else -1 (:393).  timeIdx is the call's own (GUI.h:389 passes `time`)."""
        mv = np.asarray(mv, np.float32).reshape(4, 4)
        ct = color_type(drawNormals, drawColors, drawTimes)
        self.draw(model, mvp, mv[:3, 3], 1.0 if invertNormals else -1.0, fxaa_clear_colour(showcaseMode), threshold, drawUnstable,
                  drawWindow, ct, time, timeIdx, timeDelta, stream=stream)
        self.fxaa(stream)

    def offscreen_images(self, stream=None):
        """(rgba f32 HxWx4, depth24 u32 HxW, winner key u64 HxW) of the offscreen buffer"""
        check(lib.dms_stream_sync(stream), "dms_stream_sync")
        c, d, w = Image2D(), Image2D(), Image2D()
        check(lib.dms_render_offscreen_images(self.h, C.byref(c), C.byref(d), C.byref(w)), "dms_render_offscreen_images")
        return capi.download_view(c, np.float32, 4), capi.download_view(d, np.uint32), capi.download_view(w, np.uint64)

    def images(self, image_order=False, stream=None):
        """the view's (rgba u8, depth24 u32, winner key u64), as RenderTarget.images"""
        return self.target.images(image_order, stream)


# ---- the live-frame clouds: FeedbackBuffer::render (include/dmslam_render_cloud.h) ------------------------------------------
CLOUD_RAW, CLOUD_FILTERED = 0, 1


class RenderCloudParams(C.Structure):
    """dms_render_cloud_params"""
    _fields_ = [("mvp", C.c_float * 16), ("pose_dev", _P), ("model_pose", C.c_float * 16), ("model_pose_dev", _P), ("color_type", _I)]


lib.dms_render_cloud_clip.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]
lib.dms_render_cloud.argtypes = [_P, _I2, _I2, _K, _F, C.POINTER(RenderCloudParams), _P]
lib.dms_fusion_render_cloud.argtypes = [_P, _P, _I, C.POINTER(RenderCloudParams), _P]


def _cloud_params(mvp, model_pose, color_type, pose_dev, model_pose_dev):
    p = RenderCloudParams()
    m = np.ascontiguousarray(np.eye(4, dtype=np.float32) if mvp is None else mvp, np.float32).reshape(16)
    t = np.ascontiguousarray(np.eye(4, dtype=np.float32) if model_pose is None else model_pose, np.float32).reshape(16)
    for k in range(16):
        p.mvp[k], p.model_pose[k] = float(m[k]), float(t[k])
    p.pose_dev, p.model_pose_dev, p.color_type = pose_dev, model_pose_dev, int(color_type)
    return p


def render_cloud_clip(mvp_eff, model_pose, point):
    """mvp_eff * (model_pose * (point, 1)) in the draw's fp32 order (dms_render_cloud_clip): the clip position (x, y, z, w)."""
    (_a, ap), (_b, bp) = _f16(mvp_eff), _f16(model_pose)
    pt = (C.c_float * 3)(*[float(v) for v in point])
    out = (C.c_float * 4)()
    check(lib.dms_render_cloud_clip(ap, bp, pt, out), "dms_render_cloud_clip")
    return np.array(out[:], np.float32)


def render_cloud(target, rgba, depth_metric, K, max_depth, mvp=None, model_pose=None, color_type=0, pose_dev=None, model_pose_dev=None,
                 stream=None):
    """One cloud over any colour (H x W x 4 u8) and metric depth (H x W f32) image - arrays or DeviceImages - with intrinsics
    K = (fx, fy, cx, cy): dms_render_cloud."""
    c, dm = _img(rgba, np.uint8), _img(depth_metric, np.float32)
    k = _cam(K)
    p = _cloud_params(mvp, model_pose, color_type, pose_dev, model_pose_dev)
    check(lib.dms_render_cloud(target.h, c.ref, dm.ref, C.byref(k), float(max_depth), C.byref(p), stream), "dms_render_cloud")
    if not isinstance(rgba, DeviceImage) or not isinstance(depth_metric, DeviceImage):
        check(lib.dms_stream_sync(stream))  # the temporary uploads must outlive the draw


class FeedbackBuffer:
    """FeedbackBuffer (Shaders/FeedbackBuffer.h) of a context, for its render(): ctx.feedbackBuffers()[FeedbackBuffer.RAW]."""
    RAW, FILTERED = "RAW", "FILTERED"

    def __init__(self, context, which):
        self.context, self.which = context, which

    def render(self, mvp, pose, drawNormals, drawColors, target, pose_dev=None, model_pose_dev=None, stream=None):
        """FeedbackBuffer::render(mvp, pose, drawNormals, drawColors) into `target` (mvp row-major: transpose pangolin's)."""
        self.context.renderCloud(target, self.which, mvp, pose, 1 if drawNormals else 2 if drawColors else 0, pose_dev, model_pose_dev, stream)


# ---- the image panels: GUI::displayImg of DEPTH_NORM, Model, RGB, ModelImage (include/dmslam_render_panels.h) -----------------
PANEL_RGBA8, PANEL_L8 = 0, 1
PANEL_NEAREST, PANEL_LINEAR = 0, 1
PANEL_DEPTH_NORM, PANEL_MODEL, PANEL_RGB, PANEL_MODEL_IMAGE, PANEL_ALL = 0, 1, 2, 3, 15


class Viewport(C.Structure):
    """dms_viewport: x, y of the bottom-left pixel in window coordinates, width, height"""
    _fields_ = [("x", _I), ("y", _I), ("w", _I), ("h", _I)]


lib.dms_panels_create.argtypes = [C.POINTER(_P), _I, _I]
lib.dms_panels_destroy.argtypes = [_P]
lib.dms_panels_images.argtypes = [_P, _I2, _I2]
lib.dms_depth_norm.argtypes = [_P, _I2, _F, _F, _P]
lib.dms_model_depth_image.argtypes = [_P, _I2, _F, _P]
lib.dms_render_blit.argtypes = [_P, _I2, _I, _I, C.POINTER(Viewport), C.POINTER(C.c_float), _P]
lib.dms_fusion_draw_panels.argtypes = [_P, _P, _P, C.POINTER(Viewport), _F, _I, _P]


def render_blit(target, image, fmt, filt, viewport, color=(1.0, 1.0, 1.0), stream=None):
    """RenderToViewport(true) with the depth test off (dms_render_blit): `image` (H x W x 4 u8 for PANEL_RGBA8, H x W u8 for PANEL_L8,
    image order; an array or a DeviceImage) stretched upside down over viewport = (x, y, w, h) of `target`, times `color`."""
    im = _img(image, np.uint8)
    vp = Viewport(*[int(v) for v in viewport])
    c = (C.c_float * 3)(*[float(v) for v in color])
    check(lib.dms_render_blit(target.h, im.ref, int(fmt), int(filt), C.byref(vp), c, stream), "dms_render_blit")
    if not isinstance(image, DeviceImage):
        check(lib.dms_stream_sync(stream))  # the temporary upload must outlive the blit


class Panels:
    """dms_panels: the DEPTH_NORM (L8) and Model (RGBA8) images of one camera size, with the two passes that fill them."""

    def __init__(self, width, height):
        self.width, self.height = int(width), int(height)
        h = C.c_void_p()
        check(lib.dms_panels_create(C.byref(h), self.width, self.height), "dms_panels_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            lib.dms_panels_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def normaliseDepth(self, depth_u16, min_val, max_val, stream=None):
        """depth_norm.frag (dms_depth_norm); min_val / max_val already scaled (the reference: 0.3f * 1000.f, depthCutoff * 1000.f)"""
        d = _img(depth_u16, np.uint16)
        check(lib.dms_depth_norm(self.h, d.ref, float(min_val), float(max_val), stream), "dms_depth_norm")
        if not isinstance(depth_u16, DeviceImage):
            check(lib.dms_stream_sync(stream))

    def renderDepth(self, vertex, max_depth, stream=None):
        """visualise_textures.frag (dms_model_depth_image) over an H x W x 4 f32 vertex image"""
        v = _img(vertex, np.float32)
        check(lib.dms_model_depth_image(self.h, v.ref, float(max_depth), stream), "dms_model_depth_image")
        if not isinstance(vertex, DeviceImage):
            check(lib.dms_stream_sync(stream))

    def views(self):
        """(DEPTH_NORM, Model image) as dms_image2d device views"""
        n, m = Image2D(), Image2D()
        check(lib.dms_panels_images(self.h, C.byref(n), C.byref(m)), "dms_panels_images")
        return n, m

    def images(self, stream=None):
        """(DEPTH_NORM u8 HxW, Model image u8 HxWx4), image order, after the work enqueued on `stream`"""
        check(lib.dms_stream_sync(stream), "dms_stream_sync")
        n, m = self.views()
        return capi.download_view(n, np.uint8), capi.download_view(m, np.uint8, 4)

    def blit(self, target, which, viewport, color=(1.0, 1.0, 1.0), stream=None):
        """GUI::displayImg of one of the two intermediates: PANEL_DEPTH_NORM (LINEAR) or PANEL_MODEL (NEAREST)"""
        n, m = self.views()
        vp = Viewport(*[int(v) for v in viewport])
        c = (C.c_float * 3)(*[float(v) for v in color])
        if which == PANEL_DEPTH_NORM:
            check(lib.dms_render_blit(target.h, C.byref(n), PANEL_L8, PANEL_LINEAR, C.byref(vp), c, stream), "dms_render_blit")
        else:
            check(lib.dms_render_blit(target.h, C.byref(m), PANEL_RGBA8, PANEL_NEAREST, C.byref(vp), c, stream), "dms_render_blit")
