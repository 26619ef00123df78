"""zlib depth deflated on the GPU (include/dmslam_io_write.h, csrc/deflate_dev.hip): the stream in the pinned slot must be the bytes of
the host's dms_deflate_blocks (both compile csrc/deflate_core.hpp) for every case of tests/deflate_cases.py - no tolerance - and
zlib must inflate it to the input; one object must serve inputs of several lengths and several encodes in flight; with the depth
on the device the writers' device forms must produce logs the readers read back, and with it off what they produced before."""
import hashlib
import struct
import zlib

import numpy as np
import pytest

from tests import deflate_cases as dc
from tests import jpeg_encode_cases as jc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ing():
    from densemonoslam_amd import capi, ingest

    assert capi.device_count() >= 1, "no MI355X visible"
    return ingest


@pytest.fixture(scope="module")
def host(ing):
    """the host encoder's stream of every case, computed once"""
    return {name: ing.deflate_blocks(x) for name, x in dc.cases()}


def upload(data):
    from densemonoslam_amd import capi

    arr = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data)
    buf = capi.DeviceBuffer(arr.nbytes)
    buf.upload(arr)
    return buf


def same(got, want, what):
    if hashlib.sha256(got).digest() == hashlib.sha256(want).digest():
        return
    first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    raise AssertionError("%s: %d bytes from the device, %d from the host, first difference at offset %d" % (what, len(got), len(want), first))


def test_device_stream_is_the_hosts_and_inflates_to_the_input(ing, host):
    cases = dc.cases()
    dd = ing.DeflateDeviceEncoder(max(len(x) for _, x in cases), slots=2)
    for name, x in cases:
        buf = upload(x)
        dd.encode(buf.ptr, len(x))
        got = dd.result()
        same(got, host[name], name)
        assert zlib.decompress(got) == x, name
    dd.close()


def test_one_object_inputs_of_several_lengths_leave_nothing_stale(ing, host):
    """longest first: tokens, histograms, block records and output bytes of the longer input lie behind the shorter one's"""
    names = [dc.VGA, "zeros_70001", "random_3B+17", "rows_1280", "one_match", "run_259", "len_1", "skewed_21_values", dc.VGA]
    dd = ing.DeflateDeviceEncoder(len(dc.by_name(dc.VGA)), slots=1)
    for name in names:
        x = dc.by_name(name)
        buf = upload(x)
        dd.encode(buf.ptr, len(x))
        same(dd.result(), host[name], name)
    dd.close()


def test_ring_of_two_slots_and_repeatability(ing, host):
    from densemonoslam_amd import capi

    st = capi.create_stream()
    a, b, c = "depth_160x120", "rows_1280", "skewed_21_values"
    bufs = {n: upload(dc.by_name(n)) for n in (a, b, c)}
    dd = ing.DeflateDeviceEncoder(40000, slots=2)
    dd.encode(bufs[a].ptr, len(dc.by_name(a)), stream=st)
    dd.encode(bufs[b].ptr, len(dc.by_name(b)), stream=st)  # two in flight
    same(dd.result(1), host[a], a)
    same(dd.result(0), host[b], b)
    dd.encode(bufs[c].ptr, len(dc.by_name(c)), stream=st)  # slot 0 again, now free
    same(dd.result(0), host[c], c)
    same(dd.result(1), host[b], b)
    dd.encode(bufs[a].ptr, len(dc.by_name(a)), stream=st)  # the same input again: the same bytes
    same(dd.result(), host[a], a + " again")
    dd.close()
    capi.destroy_stream(st)


def test_refusals_enqueue_nothing(ing, host):
    from densemonoslam_amd.capi import DmsError, lib

    x = dc.by_name("rows_1280")
    buf = upload(x)
    dd = ing.DeflateDeviceEncoder(len(x), slots=2)
    for bad_len in (0, len(x) + 1):
        with pytest.raises(DmsError) as e:
            dd.encode(buf.ptr, bad_len)
        assert e.value.code == -1
    with pytest.raises(DmsError):
        dd.encode(None, len(x))
    with pytest.raises(DmsError):
        dd.result()  # nothing was enqueued: no encode in any slot
    data, n = ing.C.c_void_p(), ing.C.c_size_t(0)
    assert lib.dms_deflate_dev_encode(None, buf.ptr, len(x), None) == -1
    assert lib.dms_deflate_dev_result(dd.h, None, ing.C.byref(n)) == -1 and lib.dms_deflate_dev_result(dd.h, ing.C.byref(data), None) == -1
    assert lib.dms_deflate_dev_create(None, 100, 2) == -1
    h = ing.C.c_void_p()
    for max_len, slots in ((0, 2), (100, 0), (100, 17), ((1 << 31) + 1, 2)):
        assert lib.dms_deflate_dev_create(ing.C.byref(h), max_len, slots) == -1
    dd.encode(buf.ptr, len(x))
    same(dd.result(), host["rows_1280"], "after the refusals")
    dd.close()


def test_recording_with_the_depth_on_the_device_and_off(ing, tmp_path):
    """three 64x48 frames through dms_klg_writer_append_device, dms_frame_pack_device and the LCM form: on the device the depth's
    stream is dms_deflate_blocks'; off, it is what dms_deflate writes (the parent commit's path).  Both inflate to the depth and read
    back through the device reader."""
    from densemonoslam_amd import capi

    c = jc.by_name("noise_64x48_q90_420")
    W, H = c.width, c.height
    rng = np.random.default_rng(17)
    depths = [(rng.integers(400, 4000, (H // 8, W // 8)).astype(np.uint16)).repeat(8, 0).repeat(8, 1) for _ in range(3)]
    d_dev = [upload(d) for d in depths]
    rgb_dev = upload(c.rgb)
    st = capi.create_stream()
    assert ing.RECORD_DEFAULT_DEPTH_ON_DEVICE == 0
    for on in (1, 0, None):  # None: the default, which is off
        je = ing.JpegDeviceEncoder(W, H, slots=2)
        if on is not None:
            je.set_depth_on_device(on)
        want = [ing.deflate_blocks(d.tobytes()) if on else ing.deflate(d.tobytes()) for d in depths]
        path = str(tmp_path / ("rec_%s.klg" % on))
        w = ing.KlgWriter(path)
        for k in range(3):
            w.append_device(je, d_dev[k].ptr, rgb_dev.ptr, 1000 + k, compressed=True, quality=90, stream=st)
        w.close()
        data = open(path, "rb").read()
        assert struct.unpack("<i", data[:4])[0] == 3
        p = 4
        for k in range(3):
            ts, ds, isz = struct.unpack("<qii", data[p:p + 16])
            z = data[p + 16:p + 16 + ds]
            assert ts == 1000 + k and zlib.decompress(z) == depths[k].tobytes(), (on, k)
            assert ds == len(want[k]) and z == want[k], (on, k)
            assert data[p + 16 + ds:p + 16 + ds + isz] == c.jpeg, (on, k)
            p += 16 + ds + isz
        assert p == len(data)
        jd = ing.JpegDevice(W, H, slots=2)
        rd = ing.KlgReader(path, W, H, flipColors=True)
        dd, dcol = capi.DeviceBuffer(W * H * 2), capi.DeviceBuffer(W * H * 3)
        for k in range(3):
            assert rd.next_device(jd, dd.ptr, dcol.ptr, stream=st) == 1000 + k
            jd.status()
            assert np.array_equal(dd.download(np.uint16, (H, W)), depths[k]), (on, k)
        rd.close()
        jd.close()
        # dms_frame_pack_device -> dms_eflcm_frame_encode -> dms_eflcm_frame_decode
        f = ing.Frame.decode(je.pack(d_dev[2].ptr, rgb_dev.ptr, compressed=True, quality=90, timestamp=77, frameNumber=5, senderName="rec", stream=st).encode())
        assert f.compressed and f.depth == want[2] and f.image == c.jpeg and (f.timestamp, f.frameNumber, f.senderName) == (77, 5, "rec")
        d, _ = f.unpack(W, H, flipColors=True)
        assert np.array_equal(d, depths[2]), on
        raw = je.pack(d_dev[0].ptr, rgb_dev.ptr, compressed=False, stream=st)  # a raw frame is copied in either mode
        assert not raw.compressed and raw.depth == depths[0].tobytes() and raw.image == c.rgb.tobytes()
        lpath = str(tmp_path / ("rec_%s.lcm" % on))
        lw = ing.LcmLogWriter(lpath)
        lw.append_frame_device(je, "EFUSION_FRAMES", d_dev[1].ptr, rgb_dev.ptr, 555, frameNumber=3, senderName="rec", compressed=True, quality=90, stream=st)
        lw.close()
        rl = ing.LcmLogReader(lpath)
        events = list(rl)
        rl.close()
        assert len(events) == 1 and events[0][0] == "EFUSION_FRAMES" and events[0][2] == 555
        f = ing.Frame.decode(events[0][1])
        assert f.compressed and f.image == c.jpeg and f.depth == want[1] and zlib.decompress(f.depth) == depths[1].tobytes()
        je.close()
    capi.destroy_stream(st)
