"""ctypes mirror of include/dmslam_io.h: eflcm.Frame messages, LCM event logs and .klg logs
(the reference's LcmHandler / RawLcmLogReader / RawLogReader); and of include/dmslam_io_device.h: the same readers
with both destinations in device memory, JPEG colour decoded on the GPU; and of the writers (include/dmslam_io.h second half,
include/dmslam_io_write.h): JPEG colour encoded on the host or on the GPU, zlib depth, .klg and LCM-log writers."""
import ctypes as C

import numpy as np

from .capi import check, lib

DMS_EOF = 1


class FrameMsg(C.Structure):
    _fields_ = [("trackOnly", C.c_int), ("compressed", C.c_int), ("last", C.c_int), ("depthSize", C.c_int32), ("imageSize", C.c_int32),
                ("depth", C.c_void_p), ("image", C.c_void_p), ("timestamp", C.c_int64), ("frameNumber", C.c_int32),
                ("senderName", C.c_char * 128)]


_P = C.c_void_p
DMS_ERR_UNSUPPORTED, DMS_ERR_FORMAT = -7, -8  # include/dmslam_io.h
lib.dms_eflcm_frame_encoded_size.argtypes = [C.POINTER(FrameMsg)]
lib.dms_eflcm_frame_encoded_size.restype = C.c_size_t
lib.dms_eflcm_frame_encode.argtypes = [C.POINTER(FrameMsg), _P, C.c_size_t, C.POINTER(C.c_size_t)]
lib.dms_eflcm_frame_decode.argtypes = [_P, C.c_size_t, C.POINTER(FrameMsg)]
lib.dms_frame_unpack.argtypes = [C.POINTER(FrameMsg), C.c_int, C.c_int, C.c_int, _P, _P]
lib.dms_lcmlog_open.argtypes = [C.POINTER(_P), C.c_char_p]
lib.dms_lcmlog_next.argtypes = [_P, C.c_char_p, C.c_size_t, C.POINTER(_P), C.POINTER(C.c_size_t), C.POINTER(C.c_int64)]
lib.dms_lcmlog_rewind.argtypes = [_P]
lib.dms_lcmlog_close.argtypes = [_P]
lib.dms_jpeg_decode.argtypes = [_P, C.c_size_t, C.c_int, C.c_int, _P]
lib.dms_klg_open.argtypes = [C.POINTER(_P), C.c_char_p, C.c_int, C.c_int, C.c_int]
lib.dms_klg_num_frames.argtypes = [_P]
lib.dms_klg_next.argtypes = [_P, _P, _P, C.POINTER(C.c_int64)]
lib.dms_klg_rewind.argtypes = [_P]
lib.dms_klg_close.argtypes = [_P]


class Frame:
    """eflcm.Frame (same attribute names as the generated class, logs/rgbd/eflcm/Frame.py)."""

    def __init__(self, depth=b"", image=b"", timestamp=0, frameNumber=0, senderName="", trackOnly=False, compressed=False, last=False):
        self.trackOnly, self.compressed, self.last = bool(trackOnly), bool(compressed), bool(last)
        self.depth, self.image = bytes(depth), bytes(image)
        self.depthSize, self.imageSize = len(self.depth), len(self.image)
        self.timestamp, self.frameNumber, self.senderName = int(timestamp), int(frameNumber), senderName

    def _msg(self):
        m = FrameMsg()
        m.trackOnly, m.compressed, m.last = int(self.trackOnly), int(self.compressed), int(self.last)
        m.depthSize, m.imageSize = len(self.depth), len(self.image)
        self._keep = (C.create_string_buffer(self.depth, len(self.depth)), C.create_string_buffer(self.image, len(self.image)))
        m.depth = C.cast(self._keep[0], C.c_void_p)
        m.image = C.cast(self._keep[1], C.c_void_p)
        m.timestamp, m.frameNumber = self.timestamp, self.frameNumber
        m.senderName = self.senderName.encode("utf-8")
        return m

    def encode(self):
        m = self._msg()
        n = lib.dms_eflcm_frame_encoded_size(C.byref(m))
        buf = C.create_string_buffer(n)
        w = C.c_size_t(0)
        check(lib.dms_eflcm_frame_encode(C.byref(m), buf, n, C.byref(w)), "dms_eflcm_frame_encode")
        return buf.raw[:w.value]

    @staticmethod
    def decode(data):
        data = bytes(data)
        m = FrameMsg()
        check(lib.dms_eflcm_frame_decode(data, len(data), C.byref(m)), "dms_eflcm_frame_decode")
        f = Frame(C.string_at(m.depth, m.depthSize), C.string_at(m.image, m.imageSize), m.timestamp, m.frameNumber,
                  m.senderName.decode("utf-8", "replace"), m.trackOnly, m.compressed, m.last)
        return f

    def unpack(self, width, height, flipColors=False):
        """(depth u16 HxW, rgb u8 HxWx3) as RawLcmLogReader::getNext produces them."""
        m = self._msg()
        d = np.zeros((height, width), np.uint16)
        rgb = np.zeros((height, width, 3), np.uint8)
        check(lib.dms_frame_unpack(C.byref(m), width, height, int(flipColors), d.ctypes.data_as(_P), rgb.ctypes.data_as(_P)), "dms_frame_unpack")
        return d, rgb

    def unpack_device(self, jd, depth_dev, rgb_dev, flipColors=False, stream=None):
        """unpack() with both destinations in device memory (dms_frame_unpack_device): jd is a JpegDevice, depth_dev / rgb_dev are
        device pointers; everything is enqueued on `stream`."""
        m = self._msg()
        check(lib.dms_frame_unpack_device(jd.h, C.byref(m), jd.width, jd.height, int(bool(flipColors)), _P(depth_dev), _P(rgb_dev), _P(stream)),
              "dms_frame_unpack_device")


def jpeg_decode(data, width, height):
    """Baseline JPEG -> (H, W, 3) u8 in libjpeg's R, G, B order (dms_jpeg_decode)."""
    data = bytes(data)
    rgb = np.zeros((height, width, 3), np.uint8)
    check(lib.dms_jpeg_decode(data, len(data), width, height, rgb.ctypes.data_as(_P)), "dms_jpeg_decode")
    return rgb


class LcmLogReader:
    """Events of an LCM log (lcm::LogFile): iterate (channel, data bytes, timestamp_us)."""

    def __init__(self, path):
        self.h = _P()
        check(lib.dms_lcmlog_open(C.byref(self.h), path.encode()), "dms_lcmlog_open")

    def __iter__(self):
        ch = C.create_string_buffer(256)
        data, n, ts = _P(), C.c_size_t(0), C.c_int64(0)
        while True:
            rc = lib.dms_lcmlog_next(self.h, ch, 256, C.byref(data), C.byref(n), C.byref(ts))
            if rc == DMS_EOF:
                return
            check(rc, "dms_lcmlog_next")
            yield ch.value.decode(), C.string_at(data, n.value), ts.value

    def rewind(self):
        check(lib.dms_lcmlog_rewind(self.h))

    def close(self):
        if self.h:
            lib.dms_lcmlog_close(self.h)
            self.h = None


class KlgReader:
    """.klg log (RawLogReader): iterate (timestamp, depth u16 HxW, rgb u8 HxWx3)."""

    def __init__(self, path, width, height, flipColors=False):
        self.h = _P()
        self.width, self.height = width, height
        check(lib.dms_klg_open(C.byref(self.h), path.encode(), width, height, int(flipColors)), "dms_klg_open")
        self.numFrames = lib.dms_klg_num_frames(self.h)

    def __iter__(self):
        ts = C.c_int64(0)
        while True:
            d = np.zeros((self.height, self.width), np.uint16)
            rgb = np.zeros((self.height, self.width, 3), np.uint8)
            rc = lib.dms_klg_next(self.h, d.ctypes.data_as(_P), rgb.ctypes.data_as(_P), C.byref(ts))
            if rc == DMS_EOF:
                return
            check(rc, "dms_klg_next")
            yield ts.value, d, rgb

    def next_device(self, jd, depth_dev, rgb_dev, stream=None):
        """The next frame into device memory (dms_klg_next_device), enqueued on `stream`: its timestamp, or None at the end."""
        ts = C.c_int64(0)
        rc = lib.dms_klg_next_device(self.h, jd.h, _P(depth_dev), _P(rgb_dev), C.byref(ts), _P(stream))
        if rc == DMS_EOF:
            return None
        check(rc, "dms_klg_next_device")
        return ts.value

    def rewind(self):
        check(lib.dms_klg_rewind(self.h))

    def close(self):
        if self.h:
            lib.dms_klg_close(self.h)
            self.h = None


# ---- include/dmslam_io_device.h: JPEG colour decoded on the GPU, readers with both destinations in device memory ----

class JpegDevInfo(C.Structure):
    _fields_ = [("entropy_on_host", C.c_int), ("subsequence_bytes", C.c_int), ("segments", C.c_int), ("subsequences", C.c_int),
                ("rounds", C.c_int), ("settled_lanes", C.c_int), ("blocks", C.c_int)]


JPEG_DEV_DEFAULT_SUBSEQUENCE, JPEG_DEV_ROUNDS = 64, 12
lib.dms_jpeg_dev_create.argtypes = [C.POINTER(_P), C.c_int, C.c_int, C.c_size_t, C.c_int]
lib.dms_jpeg_dev_destroy.argtypes = [_P]
lib.dms_jpeg_dev_set_subsequence_bytes.argtypes = [_P, C.c_int]
lib.dms_jpeg_dev_set_entropy_on_host.argtypes = [_P, C.c_int]
lib.dms_jpeg_dev_set_image_size.argtypes = [_P, C.c_int, C.c_int]
lib.dms_jpeg_dev_decode.argtypes = [_P, _P, C.c_size_t, C.c_int, C.c_int, _P, _P]
lib.dms_jpeg_dev_status.argtypes = [_P, C.POINTER(JpegDevInfo)]
lib.dms_jpeg_dev_get_coefficients.argtypes = [_P, _P, C.c_size_t, C.POINTER(C.c_int)]
lib.dms_frame_unpack_device.argtypes = [_P, C.POINTER(FrameMsg), C.c_int, C.c_int, C.c_int, _P, _P, _P]
lib.dms_klg_next_device.argtypes = [_P, _P, _P, _P, C.POINTER(C.c_int64), _P]


class JpegDevice:
    """dms_jpeg_dev: baseline JPEG -> RGB8 in device memory; `rgb_dev` arguments are device pointers (int) of
    width * height * 3 bytes, `stream` a stream handle (int) or None."""

    def __init__(self, width, height, max_stream_bytes=1 << 20, slots=3):
        self.h = _P()
        self.width, self.height, self.slots = width, height, slots
        check(lib.dms_jpeg_dev_create(C.byref(self.h), width, height, max_stream_bytes, slots), "dms_jpeg_dev_create")

    def set_subsequence_bytes(self, n):
        check(lib.dms_jpeg_dev_set_subsequence_bytes(self.h, int(n)), "dms_jpeg_dev_set_subsequence_bytes")

    def set_image_size(self, width, height):
        """streams of another size, no larger than the one the object was created for"""
        check(lib.dms_jpeg_dev_set_image_size(self.h, width, height), "dms_jpeg_dev_set_image_size")
        self.width, self.height = width, height

    def set_entropy_on_host(self, on):
        """the mode Frame.unpack_device / KlgReader.next_device decode in (default: on the host, the measured winner)"""
        check(lib.dms_jpeg_dev_set_entropy_on_host(self.h, int(bool(on))), "dms_jpeg_dev_set_entropy_on_host")

    def decode(self, data, rgb_dev, flipColors=False, entropy_on_host=True, stream=None):
        """enqueues the decode on `stream` and returns; parse-stage refusals raise at once"""
        data = bytes(data)
        check(lib.dms_jpeg_dev_decode(self.h, data, len(data), int(bool(flipColors)), int(bool(entropy_on_host)), _P(rgb_dev), _P(stream)),
              "dms_jpeg_dev_decode")

    def status(self):
        """waits for the last decode; raises DmsError (DMS_ERR_FORMAT) where the device met a malformed block"""
        info = JpegDevInfo()
        rc = lib.dms_jpeg_dev_status(self.h, C.byref(info))
        self.info = info
        check(rc, "dms_jpeg_dev_status")
        return info

    def coefficients(self):
        """(blocks, 64) int16 of the last decode: natural order, the scan's MCU order, DC values summed"""
        cap = 6 * ((self.width + 7) // 8) * ((self.height + 7) // 8) + 6
        out = np.zeros((cap, 64), np.int16)
        n = C.c_int(0)
        check(lib.dms_jpeg_dev_get_coefficients(self.h, out.ctypes.data_as(_P), cap, C.byref(n)), "dms_jpeg_dev_get_coefficients")
        return out[:n.value].copy()

    def close(self):
        if self.h:
            lib.dms_jpeg_dev_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- recording (include/dmslam_io.h writers' half, include/dmslam_io_write.h): JPEG colour encoded on the host or on the GPU, zlib
# depth, .klg and LCM-log writers ----

JPEG_444, JPEG_420 = 0, 2
DMS_ERR_CAPACITY = -4
JPEG_ENC_DEFAULT_ENTROPY_ON_HOST = 0  # DMS_JPEG_ENC_DEFAULT_ENTROPY_ON_HOST
RECORD_DEFAULT_DEPTH_ON_DEVICE = 0  # DMS_RECORD_DEFAULT_DEPTH_ON_DEVICE
lib.dms_jpeg_encode_bound.argtypes = [C.c_int, C.c_int, C.c_int]
lib.dms_jpeg_encode_bound.restype = C.c_size_t
lib.dms_jpeg_encode.argtypes = [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_size_t, C.POINTER(C.c_size_t)]
lib.dms_deflate_bound.argtypes = [C.c_size_t]
lib.dms_deflate_bound.restype = C.c_size_t
lib.dms_deflate.argtypes = [_P, C.c_size_t, _P, C.c_size_t, C.POINTER(C.c_size_t)]
lib.dms_deflate_blocks_block_size.argtypes = []
lib.dms_deflate_blocks_block_size.restype = C.c_size_t
lib.dms_deflate_blocks_bound.argtypes = [C.c_size_t]
lib.dms_deflate_blocks_bound.restype = C.c_size_t
lib.dms_deflate_blocks.argtypes = [_P, C.c_size_t, _P, C.c_size_t, C.POINTER(C.c_size_t)]
lib.dms_deflate_dev_create.argtypes = [C.POINTER(_P), C.c_size_t, C.c_int]
lib.dms_deflate_dev_destroy.argtypes = [_P]
lib.dms_deflate_dev_encode.argtypes = [_P, _P, C.c_size_t, _P]
lib.dms_deflate_dev_result.argtypes = [_P, C.POINTER(_P), C.POINTER(C.c_size_t)]
lib.dms_deflate_dev_result_at.argtypes = [_P, C.c_int, C.POINTER(_P), C.POINTER(C.c_size_t)]
lib.dms_jpeg_enc_set_depth_on_device.argtypes = [_P, C.c_int]
lib.dms_frame_pack.argtypes = [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int32, C.c_char_p, C.POINTER(FrameMsg),
                               C.POINTER(_P)]
lib.dms_frame_pack_free.argtypes = [_P]
lib.dms_frame_pack_free.restype = None
lib.dms_klg_writer_open.argtypes = [C.POINTER(_P), C.c_char_p]
lib.dms_klg_writer_append.argtypes = [_P, C.c_int64, _P, C.c_int32, _P, C.c_int32]
lib.dms_klg_writer_close.argtypes = [_P]
lib.dms_lcmlog_writer_open.argtypes = [C.POINTER(_P), C.c_char_p]
lib.dms_lcmlog_writer_append.argtypes = [_P, C.c_int64, C.c_char_p, _P, C.c_size_t]
lib.dms_lcmlog_writer_close.argtypes = [_P]
lib.dms_jpeg_enc_create.argtypes = [C.POINTER(_P), C.c_int, C.c_int, C.c_int]
lib.dms_jpeg_enc_destroy.argtypes = [_P]
lib.dms_jpeg_enc_set_image_size.argtypes = [_P, C.c_int, C.c_int]
lib.dms_jpeg_enc_set_entropy_on_host.argtypes = [_P, C.c_int]
lib.dms_jpeg_enc_encode.argtypes = [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]
lib.dms_jpeg_enc_result.argtypes = [_P, C.POINTER(_P), C.POINTER(C.c_size_t)]
lib.dms_jpeg_enc_result_at.argtypes = [_P, C.c_int, C.POINTER(_P), C.POINTER(C.c_size_t)]
lib.dms_frame_pack_device.argtypes = [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int32, C.c_char_p, C.POINTER(FrameMsg), _P]
lib.dms_klg_writer_append_device.argtypes = [_P, _P, _P, _P, C.c_int64, C.c_int, C.c_int, _P]
lib.dms_lcmlog_writer_append_frame_device.argtypes = [_P, _P, C.c_char_p, _P, _P, C.c_int64, C.c_int32, C.c_char_p, C.c_int, C.c_int, _P]


def jpeg_encode_bound(width, height, subsampling=JPEG_420):
    """the most bytes dms_jpeg_encode can write for this size (dms_jpeg_encode_bound); 0 for bad arguments"""
    return int(lib.dms_jpeg_encode_bound(width, height, subsampling))


def jpeg_encode(rgb, quality=90, subsampling=JPEG_420, flipColors=False, cap=None):
    """(H, W, 3) u8 -> the bytes of a baseline JPEG file, libjpeg's (dms_jpeg_encode).  `cap`: the size of the output buffer, for
    tests of the refusal; the default is jpeg_encode_bound."""
    rgb = np.ascontiguousarray(rgb, np.uint8)
    h, w = rgb.shape[:2]
    n = jpeg_encode_bound(w, h, subsampling) if cap is None else cap
    buf = C.create_string_buffer(max(n, 1))
    written = C.c_size_t(0)
    rc = lib.dms_jpeg_encode(rgb.ctypes.data_as(_P), w, h, int(quality), int(subsampling), int(bool(flipColors)), buf, n, C.byref(written))
    jpeg_encode.last_written = written.value
    check(rc, "dms_jpeg_encode")
    return buf.raw[:written.value]


def deflate(data):
    """zlib's compress2 at its default level, resolved at run time (dms_deflate)"""
    data = bytes(data)
    n = lib.dms_deflate_bound(len(data))
    buf = C.create_string_buffer(n)
    written = C.c_size_t(0)
    check(lib.dms_deflate(data, len(data), buf, n, C.byref(written)), "dms_deflate")
    return buf.raw[:written.value]


def deflate_blocks_block_size():
    """input bytes per deflate block of deflate_blocks (dms_deflate_blocks_block_size)"""
    return int(lib.dms_deflate_blocks_block_size())


def deflate_blocks_bound(n):
    """the most bytes deflate_blocks can write for n input bytes (dms_deflate_blocks_bound)"""
    return int(lib.dms_deflate_blocks_bound(n))


def deflate_blocks(data, cap=None):
    """a zlib stream of blocks that can all be made at once, the bytes DeflateDeviceEncoder writes (dms_deflate_blocks); no libz
    needed.  `cap`: the size of the output buffer, for tests of the refusal; the default is deflate_blocks_bound."""
    data = bytes(data)
    n = deflate_blocks_bound(len(data)) if cap is None else cap
    buf = C.create_string_buffer(max(n, 1))
    written = C.c_size_t(0)
    rc = lib.dms_deflate_blocks(data, len(data), buf, n, C.byref(written))
    deflate_blocks.last_written = written.value
    check(rc, "dms_deflate_blocks")
    return buf.raw[:written.value]


class DeflateDeviceEncoder:
    """dms_deflate_dev: bytes in device memory -> a zlib stream in a pinned slot; `data_dev` is a device pointer (int), `stream` a
    stream handle (int) or None."""

    def __init__(self, max_len, slots=3):
        self.h = _P()
        self.max_len, self.slots = max_len, slots
        check(lib.dms_deflate_dev_create(C.byref(self.h), max_len, slots), "dms_deflate_dev_create")

    def encode(self, data_dev, n, stream=None):
        """enqueues the encode of n bytes on `stream` and returns; refusals raise at once, with nothing enqueued"""
        check(lib.dms_deflate_dev_encode(self.h, _P(data_dev), int(n), _P(stream)), "dms_deflate_dev_encode")

    def result(self, back=0):
        """waits for the last encode (or the one `back` before it) and returns its stream"""
        data, n = _P(), C.c_size_t(0)
        check(lib.dms_deflate_dev_result_at(self.h, int(back), C.byref(data), C.byref(n)), "dms_deflate_dev_result_at")
        return C.string_at(data, n.value)

    def close(self):
        if self.h:
            lib.dms_deflate_dev_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _frame_of(m):
    return Frame(C.string_at(m.depth, m.depthSize), C.string_at(m.image, m.imageSize), m.timestamp, m.frameNumber,
                 m.senderName.decode("utf-8", "replace"), m.trackOnly, m.compressed, m.last)


def frame_pack(depth, rgb, compressed=True, quality=90, flipColors=False, timestamp=0, frameNumber=0, senderName=""):
    """depth (H, W) u16 + rgb (H, W, 3) u8 -> a Frame (dms_frame_pack): raw, or zlib depth + JPEG colour as the reference's
    converters write them."""
    depth = np.ascontiguousarray(depth, np.uint16)
    rgb = np.ascontiguousarray(rgb, np.uint8)
    h, w = depth.shape
    m, owned = FrameMsg(), _P()
    check(lib.dms_frame_pack(depth.ctypes.data_as(_P), rgb.ctypes.data_as(_P), w, h, int(bool(compressed)), int(quality), int(bool(flipColors)),
                             int(timestamp), int(frameNumber), senderName.encode("utf-8"), C.byref(m), C.byref(owned)), "dms_frame_pack")
    try:
        return _frame_of(m)
    finally:
        lib.dms_frame_pack_free(owned)


class JpegDeviceEncoder:
    """dms_jpeg_enc: RGB8 in device memory -> JPEG bytes in a pinned slot; `rgb_dev` / `depth_dev` arguments are device pointers
    (int), `stream` a stream handle (int) or None."""

    def __init__(self, max_width, max_height, slots=3):
        self.h = _P()
        self.width, self.height, self.slots = max_width, max_height, slots
        check(lib.dms_jpeg_enc_create(C.byref(self.h), max_width, max_height, slots), "dms_jpeg_enc_create")

    def set_image_size(self, width, height):
        """frames of another size, no larger than the one the object was created for"""
        check(lib.dms_jpeg_enc_set_image_size(self.h, width, height), "dms_jpeg_enc_set_image_size")
        self.width, self.height = width, height

    def set_entropy_on_host(self, on):
        """the mode pack() and the writers' device forms encode in (default: the measured winner)"""
        check(lib.dms_jpeg_enc_set_entropy_on_host(self.h, int(bool(on))), "dms_jpeg_enc_set_entropy_on_host")

    def set_depth_on_device(self, on):
        """pack() and the writers' device forms deflate the depth with kernels (deflate_blocks' bytes) instead of zlib on the host"""
        check(lib.dms_jpeg_enc_set_depth_on_device(self.h, int(bool(on))), "dms_jpeg_enc_set_depth_on_device")

    def encode(self, rgb_dev, quality=90, subsampling=JPEG_420, flipColors=False, entropy_on_host=False, stream=None):
        """enqueues the encode on `stream` and returns; refusals raise at once, with nothing enqueued"""
        check(lib.dms_jpeg_enc_encode(self.h, _P(rgb_dev), int(quality), int(subsampling), int(bool(flipColors)), int(bool(entropy_on_host)),
                                      _P(stream)), "dms_jpeg_enc_encode")

    def result(self, back=0):
        """waits for the last encode (or the one `back` before it) and returns its bytes"""
        data, n = _P(), C.c_size_t(0)
        check(lib.dms_jpeg_enc_result_at(self.h, int(back), C.byref(data), C.byref(n)), "dms_jpeg_enc_result_at")
        return C.string_at(data, n.value)

    def pack(self, depth_dev, rgb_dev, compressed=True, quality=90, timestamp=0, frameNumber=0, senderName="", stream=None):
        """one frame from device memory -> a Frame (dms_frame_pack_device)"""
        m = FrameMsg()
        check(lib.dms_frame_pack_device(self.h, _P(depth_dev), _P(rgb_dev), self.width, self.height, int(bool(compressed)), int(quality), int(timestamp),
                                        int(frameNumber), senderName.encode("utf-8"), C.byref(m), _P(stream)), "dms_frame_pack_device")
        return _frame_of(m)

    def close(self):
        if self.h:
            lib.dms_jpeg_enc_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class KlgWriter:
    """.klg writer (dms_klg_writer): append(timestamp, depth bytes, image bytes) takes the payloads as they go into the file."""

    def __init__(self, path):
        self.h = _P()
        check(lib.dms_klg_writer_open(C.byref(self.h), path.encode()), "dms_klg_writer_open")

    def append(self, timestamp, depth_bytes, image_bytes=b""):
        d, i = bytes(depth_bytes), bytes(image_bytes)
        check(lib.dms_klg_writer_append(self.h, int(timestamp), d, len(d), i, len(i)), "dms_klg_writer_append")

    def append_device(self, je, depth_dev, rgb_dev, timestamp, compressed=True, quality=90, stream=None):
        """one frame of je's size from device memory (dms_klg_writer_append_device)"""
        check(lib.dms_klg_writer_append_device(self.h, je.h, _P(depth_dev), _P(rgb_dev), int(timestamp), int(bool(compressed)), int(quality), _P(stream)),
              "dms_klg_writer_append_device")

    def close(self):
        if self.h:
            h, self.h = self.h, None
            check(lib.dms_klg_writer_close(h), "dms_klg_writer_close")


class LcmLogWriter:
    """LCM event log writer (dms_lcmlog_writer)."""

    def __init__(self, path):
        self.h = _P()
        check(lib.dms_lcmlog_writer_open(C.byref(self.h), path.encode()), "dms_lcmlog_writer_open")

    def append(self, timestamp_us, channel, data):
        data = bytes(data)
        check(lib.dms_lcmlog_writer_append(self.h, int(timestamp_us), channel.encode(), data, len(data)), "dms_lcmlog_writer_append")

    def append_frame_device(self, je, channel, depth_dev, rgb_dev, timestamp, frameNumber=0, senderName="", compressed=True, quality=90, stream=None):
        """one frame of je's size from device memory as an eflcm.Frame event (dms_lcmlog_writer_append_frame_device)"""
        check(lib.dms_lcmlog_writer_append_frame_device(self.h, je.h, channel.encode(), _P(depth_dev), _P(rgb_dev), int(timestamp), int(frameNumber),
                                                        senderName.encode("utf-8"), int(bool(compressed)), int(quality), _P(stream)),
              "dms_lcmlog_writer_append_frame_device")

    def close(self):
        if self.h:
            h, self.h = self.h, None
            check(lib.dms_lcmlog_writer_close(h), "dms_lcmlog_writer_close")
