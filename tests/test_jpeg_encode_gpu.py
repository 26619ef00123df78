"""JPEG colour encoded on the GPU (include/dmslam_io_write.h, csrc/jpeg_enc_dev.hip): the bytes in the pinned slot must be libjpeg's,
the whole file from SOI to EOI, for every case of tests/golden/jpeg_encode_cases.npz, in both entropy modes, with and without
flipColors - no tolerance anywhere; one object must serve frames of several sizes and several encodes in flight; the writers' device
forms must produce logs the device readers read back."""
import hashlib
import struct
import zlib

import numpy as np
import pytest

from tests import jpeg_encode_cases as jc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ing():
    from densemonoslam_amd import capi, ingest

    assert capi.device_count() >= 1, "no MI355X visible"
    return ingest


def upload(arr):
    from densemonoslam_amd import capi

    arr = np.ascontiguousarray(arr)
    buf = capi.DeviceBuffer(arr.nbytes)
    buf.upload(arr)
    return buf


def test_device_encoder_writes_libjpegs_bytes(ing):
    """every case x entropy on the device / on the host x flipColors 0 / 1 (flipped: the channel-swapped input gives the same file)"""
    checked = 0
    for c in jc.cases():
        je = ing.JpegDeviceEncoder(c.width, c.height, slots=2)
        src = {False: upload(c.rgb), True: upload(c.rgb[..., ::-1])}
        for on_host in (False, True):
            for flip in (False, True):
                je.encode(src[flip].ptr, c.quality, c.subsampling, flipColors=flip, entropy_on_host=on_host)
                got = je.result()
                assert got == c.jpeg, "%s entropy_on_host=%s flip=%s: %d bytes, %d wanted" % (c.name, on_host, flip, len(got), len(c.jpeg))
                checked += 1
        je.close()
    assert checked == 12 * 4


def test_one_object_frames_of_several_sizes_leave_no_stale_bits_or_planes(ing):
    """an object made for 640x480 encodes the 640x480 case, then 17x33, then 45x23, then 640x480 again, in both modes"""
    from densemonoslam_amd import capi

    order = [jc.by_name(n) for n in (jc.VGA, "noise_17x33_q100_420", "smooth_45x23_q90_420", jc.VGA)]
    je = ing.JpegDeviceEncoder(640, 480, slots=2)
    for on_host in (False, True):
        for c in order:
            je.set_image_size(c.width, c.height)
            buf = upload(c.rgb)
            je.encode(buf.ptr, c.quality, c.subsampling, entropy_on_host=on_host)
            assert je.result() == c.jpeg, (on_host, c.name)
    with pytest.raises(capi.DmsError, match="larger"):
        je.set_image_size(641, 480)
    je.close()


def test_two_encodes_in_flight_on_a_ring_of_two_slots(ing):
    """enqueued back to back on a stream of their own, results read afterwards; then the ring comes round (a third and fourth encode)"""
    from densemonoslam_amd import capi

    a, b = jc.by_name("noise_64x48_q90_420"), jc.by_name("smooth_96x64_q30_420")
    je = ing.JpegDeviceEncoder(96, 64, slots=2)
    st = capi.create_stream()
    ba, bb = upload(a.rgb), upload(b.rgb)
    for modes in ((False, False), (False, True), (True, False)):
        je.set_image_size(a.width, a.height)
        je.encode(ba.ptr, a.quality, a.subsampling, entropy_on_host=modes[0], stream=st)
        je.set_image_size(b.width, b.height)
        je.encode(bb.ptr, b.quality, b.subsampling, entropy_on_host=modes[1], stream=st)
        assert je.result(back=1) == a.jpeg, modes
        assert je.result(back=0) == b.jpeg, modes
        assert je.result(back=1) == a.jpeg  # still there
    with pytest.raises(capi.DmsError, match="slots"):
        je.result(back=2)
    je.close()
    capi.destroy_stream(st)


def test_encoding_what_the_device_decoder_wrote(ing):
    """dms_jpeg_dev_decode of a fixture stream into a device buffer, then dms_jpeg_enc_encode of that buffer: the host encoder's bytes
    for the same pixels"""
    from densemonoslam_amd import capi

    for name in ("smooth_45x23_q90_420", "noise_70x37_q90_420", "smooth_50x40_q90_444"):
        c = jc.by_name(name)
        jd = ing.JpegDevice(c.width, c.height, max_stream_bytes=max(len(c.jpeg), 64), slots=1)
        buf = capi.DeviceBuffer(c.width * c.height * 3)
        jd.decode(c.jpeg, buf.ptr)
        jd.status()
        pixels = buf.download(np.uint8, (c.height, c.width, 3))
        assert hashlib.sha256(pixels.tobytes()).digest() == c.decoded_sha256
        je = ing.JpegDeviceEncoder(c.width, c.height, slots=1)
        for on_host in (False, True):
            je.encode(buf.ptr, 75, c.subsampling, entropy_on_host=on_host)
            assert je.result() == ing.jpeg_encode(pixels, 75, c.subsampling), (name, on_host)
        je.close()
        jd.close()


def test_log_round_trip_from_device_memory(ing, tmp_path):
    """dms_klg_writer_append_device of three 640x480 frames (compressed, quality 90), close, dms_klg_next_device reads them back: depth
    identical, colour = the fixture's Pillow decode, the file's JPEG payload = the fixture's stream.  The same frames through
    dms_lcmlog_writer_append_frame_device and a raw frame through both."""
    from densemonoslam_amd import capi

    c = jc.by_name(jc.VGA)
    W, H = c.width, c.height
    rng = np.random.default_rng(17)
    depths = [(rng.integers(400, 4000, (H // 8, W // 8)).astype(np.uint16)).repeat(8, 0).repeat(8, 1) for _ in range(3)]
    d_dev = [upload(d) for d in depths]
    rgb_dev = upload(c.rgb)
    st = capi.create_stream()
    for on_host in (ing.JPEG_ENC_DEFAULT_ENTROPY_ON_HOST, 1 - ing.JPEG_ENC_DEFAULT_ENTROPY_ON_HOST):
        je = ing.JpegDeviceEncoder(W, H, slots=2)
        if on_host != ing.JPEG_ENC_DEFAULT_ENTROPY_ON_HOST:
            je.set_entropy_on_host(on_host)
        path = str(tmp_path / ("rec%d.klg" % on_host))
        w = ing.KlgWriter(path)
        for k in range(3):
            w.append_device(je, d_dev[k].ptr, rgb_dev.ptr, 1000 + k, compressed=True, quality=90, stream=st)
        w.append_device(je, d_dev[0].ptr, rgb_dev.ptr, 2000, compressed=False, stream=st)
        w.close()
        data = open(path, "rb").read()
        assert struct.unpack("<i", data[:4])[0] == 4
        p = 4
        for k in range(3):
            ts, ds, isz = struct.unpack("<qii", data[p:p + 16])
            assert ts == 1000 + k and zlib.decompress(data[p + 16:p + 16 + ds]) == depths[k].tobytes()
            assert data[p + 16 + ds:p + 16 + ds + isz] == c.jpeg, (on_host, k)
            p += 16 + ds + isz
        assert struct.unpack("<qii", data[p:p + 16]) == (2000, W * H * 2, W * H * 3) and data[p + 16 + W * H * 2:] == c.rgb.tobytes()
        # back through the device reader; flipColors undoes the loader's R <-> B exchange of JPEG colour
        jd = ing.JpegDevice(W, H, slots=2)
        rd = ing.KlgReader(path, W, H, flipColors=True)
        assert rd.numFrames == 4
        dd, dc = capi.DeviceBuffer(W * H * 2), capi.DeviceBuffer(W * H * 3)
        for k in range(3):
            assert rd.next_device(jd, dd.ptr, dc.ptr, stream=st) == 1000 + k
            jd.status()
            assert np.array_equal(dd.download(np.uint16, (H, W)), depths[k]), (on_host, k)
            assert hashlib.sha256(dc.download(np.uint8, (H, W, 3)).tobytes()).digest() == c.decoded_sha256, (on_host, k)
        rd.close()
        jd.close()
        # the LCM log
        lpath = str(tmp_path / ("rec%d.lcm" % on_host))
        lw = ing.LcmLogWriter(lpath)
        lw.append_frame_device(je, "EFUSION_FRAMES", d_dev[1].ptr, rgb_dev.ptr, 555, frameNumber=3, senderName="rec", compressed=True, quality=90, stream=st)
        lw.close()
        rl = ing.LcmLogReader(lpath)
        events = list(rl)
        rl.close()
        assert len(events) == 1 and events[0][0] == "EFUSION_FRAMES" and events[0][2] == 555
        f = ing.Frame.decode(events[0][1])
        assert f.compressed and f.image == c.jpeg and zlib.decompress(f.depth) == depths[1].tobytes()
        assert (f.timestamp, f.frameNumber, f.senderName) == (555, 3, "rec")
        je.close()
    capi.destroy_stream(st)


def test_refusals_enqueue_nothing(ing):
    """a frame larger than the object, a null device pointer, a quality of 0: refused at once; the object is still usable and the slot
    of the last good encode is untouched"""
    from densemonoslam_amd import capi

    c = jc.by_name("noise_64x48_q90_420")
    je = ing.JpegDeviceEncoder(c.width, c.height, slots=1)
    buf = upload(c.rgb)
    dep = capi.DeviceBuffer(c.width * c.height * 2)
    je.encode(buf.ptr, c.quality, c.subsampling)
    assert je.result() == c.jpeg
    with pytest.raises(capi.DmsError, match="larger") as e:
        je.set_image_size(c.width + 1, c.height)
    assert e.value.code == -1
    with pytest.raises(capi.DmsError, match="null") as e:
        je.encode(None, c.quality, c.subsampling)
    assert e.value.code == -1
    with pytest.raises(capi.DmsError, match="quality") as e:
        je.encode(buf.ptr, 0, c.subsampling)
    assert e.value.code == -1
    with pytest.raises(capi.DmsError, match="subsampling"):
        je.encode(buf.ptr, 90, 1)
    with pytest.raises(capi.DmsError, match="another image size"):
        ing.lib.dms_frame_pack_device  # noqa: B018  (the symbol exists)
        m = ing.FrameMsg()
        capi.check(ing.lib.dms_frame_pack_device(je.h, dep.ptr, buf.ptr, c.width * 2, c.height, 1, 90, 0, 0, b"", ing.C.byref(m), None), "dms_frame_pack_device")
    with pytest.raises(capi.DmsError, match="quality"):
        je.pack(dep.ptr, buf.ptr, quality=0)
    with pytest.raises(capi.DmsError, match="null"):
        je.pack(None, buf.ptr)
    assert je.result() == c.jpeg  # nothing took the slot
    je.encode(buf.ptr, c.quality, c.subsampling, entropy_on_host=True)
    assert je.result() == c.jpeg
    je.close()
