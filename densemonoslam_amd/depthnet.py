"""Python mirror of the reference's DepthPrediction (GUI/src/Tools/DepthPrediction.h) over the C ABI of include/dmslam_depthnet.h.

The network is the caller's: any callable that maps the [1, 3, H, W] input tensor to a [1, 1, H, W] (or [H, W]) tensor of metres on the
same device.  The two conversions around it run in libdmslam_hip.so on torch's current stream, with the reference's bits; nothing
crosses to the host and nothing here synchronises it.

torch brings its own copy of the HIP runtime: import torch before this package (tests/conftest.py does), so that the library and
torch share one.
"""
import ctypes as C

import numpy as np
import torch

from . import fusion as _fusion  # noqa: F401  (declares the argument types of the dms_fusion_* calls used below)
from .capi import check, lib

RUNTIME, TRUNCATE = 0, 1  # DMS_DEPTHNET_RUNTIME, DMS_DEPTHNET_TRUNCATE

_P, _I = C.c_void_p, C.c_int
lib.dms_depthnet_pack.argtypes = [_P, _I, _I, _I, _P, _I, _P]
lib.dms_depthnet_unpack.argtypes = [_P, _I, _I, _I, _P, _I, _P]


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def pack(rgb_ptr, channels, width, height, tensor_ptr, half=False, stream=None):
    """dms_depthnet_pack on device addresses; `stream` is a HIP stream handle (None: the null stream)"""
    check(lib.dms_depthnet_pack(C.c_void_p(rgb_ptr), int(channels), int(width), int(height), C.c_void_p(tensor_ptr), int(bool(half)), stream),
          "dms_depthnet_pack")


def unpack(tensor_ptr, half, width, height, depth_ptr, mode=RUNTIME, stream=None):
    """dms_depthnet_unpack on device addresses"""
    check(lib.dms_depthnet_unpack(C.c_void_p(tensor_ptr), int(bool(half)), int(width), int(height), C.c_void_p(depth_ptr), int(mode), stream),
          "dms_depthnet_unpack")


class DepthPrediction:
    """predict(rgb, net) = DepthPrediction::predict (DepthPrediction.cpp:106-169) with `net` in the place of the ONNX session.

    Owns the network's input tensor (`input`, [1, 3, H, W], float32 or float16 with half_float) and the 16-bit millimetre depth image
    (`depth`, [H, W] uint16), both on `device`."""

    def __init__(self, width, height, half_float=False, mode=RUNTIME, device="cuda"):
        if mode not in (RUNTIME, TRUNCATE):
            raise ValueError("unknown mode %r" % (mode,))
        self.width, self.height = int(width), int(height)
        self.half_float, self.mode = bool(half_float), int(mode)
        self.dtype = torch.float16 if self.half_float else torch.float32
        self.input = torch.zeros((1, 3, self.height, self.width), dtype=self.dtype, device=device)
        self.depth = torch.zeros((self.height, self.width), dtype=torch.uint16, device=device)
        self._rgb = None  # the last frame's colour image on the device: the frame step reads it after predict() has returned

    def _image(self, rgb):
        if not isinstance(rgb, torch.Tensor):
            rgb = torch.from_numpy(np.ascontiguousarray(rgb, np.uint8))
        if rgb.dtype != torch.uint8 or rgb.dim() != 3 or tuple(rgb.shape[:2]) != (self.height, self.width) or rgb.shape[2] not in (3, 4):
            raise ValueError("rgb must be uint8 [%d, %d, 3 or 4], got %s %s" % (self.height, self.width, rgb.dtype, tuple(rgb.shape)))
        if rgb.device != self.input.device:  # a host image: staged through an owned device tensor, on the current stream
            if self._rgb is None or self._rgb.shape != rgb.shape:
                self._rgb = torch.empty(rgb.shape, dtype=torch.uint8, device=self.input.device)
            self._rgb.copy_(rgb, non_blocking=True)
            return self._rgb
        if not rgb.is_contiguous():
            raise ValueError("rgb must be contiguous")
        self._rgb = rgb
        return rgb

    def pack(self, rgb):
        """rgb (uint8 [H, W, 3 or 4], a device tensor or a host array) -> self.input, on torch's current stream"""
        img = self._image(rgb)
        pack(img.data_ptr(), img.shape[2], self.width, self.height, self.input.data_ptr(), self.half_float, _stream())
        return self.input

    def unpack(self, out):
        """out (contiguous [1, 1, H, W] or [H, W] metres of the input's dtype, on the device) -> self.depth, on torch's current stream"""
        if not isinstance(out, torch.Tensor) or out.dtype != self.dtype or out.device != self.input.device:
            raise ValueError("the network's output must be a %s tensor on %s" % (self.dtype, self.input.device))
        if out.numel() != self.width * self.height or tuple(out.shape[-2:]) != (self.height, self.width) or not out.is_contiguous():
            raise ValueError("the network's output must be contiguous [1, 1, %d, %d] or [%d, %d], got %s"
                             % (self.height, self.width, self.height, self.width, tuple(out.shape)))
        unpack(out.data_ptr(), self.half_float, self.width, self.height, self.depth.data_ptr(), self.mode, _stream())
        return self.depth

    def predict(self, rgb, net):
        """pack, net(input), unpack: returns the depth image (self.depth), valid in stream order on torch's current stream"""
        out = net(self.pack(rgb))
        return self.unpack(out)

    def processFrame(self, fusion, rgb, net, inPose=None, weightMultiplier=1.0, stream=None):
        """One camera-loop iteration under predict_depth (MainController.cpp:315-326, :373): the frame's depth from `net`, then
        `fusion` (a fusion.ElasticFusion) steps on it; asynchronous, fusion.fetch() returns the frame's result.

        The conversions and the network run on torch's current stream, the frame on `stream` (a HIP stream handle, None: the null
        stream).  With pipeline_ingest the frame reads its inputs on a stream of its own, which dms_fusion_inputs_ready orders behind
        the producer; the previous frame must have read the depth image before this one's is written (dms_fusion_inputs_consumed:
        a short host wait for the previous frame's ingest, the only one)."""
        check(lib.dms_fusion_inputs_consumed(fusion.h, stream), "dms_fusion_inputs_consumed")
        self.predict(rgb, net)
        if fusion.params.pipeline_ingest:
            fusion.inputsReady(_stream())
        elif ((stream.value if isinstance(stream, C.c_void_p) else stream) or 0) != torch.cuda.current_stream().cuda_stream:
            raise ValueError("with pipeline_ingest off the frame's stream must be torch's current stream")
        fusion.processFrameAsync(self._rgb.data_ptr(), self._rgb.shape[2], self.depth.data_ptr(), inPose, weightMultiplier, stream)
