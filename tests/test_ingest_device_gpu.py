"""JPEG colour decoded on the GPU (include/dmslam_io_device.h, csrc/jpeg_dev.hip): the RGB8 bytes in device memory must be those of
the host's sequential decoder (dms_jpeg_decode, itself pinned to libjpeg's bytes) for every stream it accepts, in both entropy
modes; the device entropy decode must report the subsequences, rounds and refusals that the host restatement of the same lanes
printed (tests/jpeg_lanes_host.cpp -> tests/golden/jpeg_lane_rounds.json); the device readers must feed the frame step the bytes
the host readers do."""
import ctypes as C
import hashlib
import io
import json
import os
import struct
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEFAULT_S = 64


@pytest.fixture(scope="module")
def ing():
    from densemonoslam_amd import capi, ingest

    assert capi.device_count() >= 1, "no MI355X visible"
    return ingest


@pytest.fixture(scope="module")
def streams(ing):
    """name -> (width, height, bytes, refusal text or '', the host decoder's RGB or None, recorded digest or None): both fixtures"""
    out = {}
    for fn in ("jpeg_cases.npz", "jpeg_device_cases.npz"):
        z = np.load(os.path.join(GOLDEN, fn))
        for name in [str(n) for n in z["names"]]:
            w, h = [int(v) for v in z[name + "_shape"]]
            data = z[name + "_jpeg"].tobytes()
            refusal = str(z[name + "_refusal"][0]) if name + "_refusal" in z else ""
            host = None if refusal else ing.jpeg_decode(data, w, h)
            out[name] = (w, h, data, refusal, host, z[name + "_sha256"].tobytes() if name + "_sha256" in z else None)
    return out


@pytest.fixture(scope="module")
def rounds():
    return json.load(open(os.path.join(GOLDEN, "jpeg_lane_rounds.json")))


def decode_to_host(ing, jd, data, w, h, **kw):
    from densemonoslam_amd import capi

    buf = capi.DeviceBuffer(w * h * 3)
    jd.decode(data, buf.ptr, **kw)
    jd.status()
    return buf.download(np.uint8, (h, w, 3))


def host_coefficients(ing, jd, data, w, h):
    """the sequential entropy stage's coefficients: the host-entropy mode uploads exactly them"""
    from densemonoslam_amd import capi

    buf = capi.DeviceBuffer(w * h * 3)
    jd.decode(data, buf.ptr, entropy_on_host=True)
    jd.status()
    return jd.coefficients()


def test_device_decode_equals_the_host_decoder(ing, streams):
    """Every decodable stream (2x3 .. 640x480; the cut stream included: missing bits are zeros), host entropy and device entropy with
    S = 32 and the default, flipColors 0 and 1: the RGB8 in device memory equals dms_jpeg_decode's bytes (exchanged where flipped),
    the 640x480 one also its recorded libjpeg digest; the coefficient buffer equals the sequential entropy stage's."""
    checked = 0
    for name, (w, h, data, refusal, host, digest) in streams.items():
        if refusal:
            continue
        jd = ing.JpegDevice(w, h, max_stream_bytes=max(len(data), 64), slots=2)
        want_coefs = host_coefficients(ing, jd, data, w, h)
        for on_host, S in ((True, DEFAULT_S), (False, 32), (False, DEFAULT_S)):
            jd.set_subsequence_bytes(S)
            for flip in (False, True):
                got = decode_to_host(ing, jd, data, w, h, flipColors=flip, entropy_on_host=on_host)
                what = "%s host_entropy=%s S=%d flip=%s" % (name, on_host, S, flip)
                assert np.array_equal(got, host[..., ::-1] if flip else host), what
                if digest is not None and not flip:
                    assert hashlib.sha256(got.tobytes()).digest() == digest, what
                assert np.array_equal(jd.coefficients(), want_coefs), what
                checked += 1
        jd.close()
    assert checked >= 17 * 6


def test_status_reports_lanes_rounds_and_refusals(ing, streams, rounds):
    """More than one subsequence on every stream longer than S; lanes, rounds and settled lanes are those the host restatement of
    the lanes printed for the same stream and S; the three altered streams end in DMS_ERR_FORMAT with the sequential decoder's
    reason; the parse stage's refusals come back from the decode call itself, with dms_jpeg_decode's code and text."""
    from densemonoslam_amd import capi

    assert ing.JPEG_DEV_DEFAULT_SUBSEQUENCE == DEFAULT_S
    refused = 0
    for name, (w, h, data, refusal, host, _) in streams.items():
        jd = ing.JpegDevice(w, h, max_stream_bytes=max(len(data), 64), slots=2)
        buf = capi.DeviceBuffer(w * h * 3)
        for S in (32, 64, 128, 256):
            jd.set_subsequence_bytes(S)
            jd.decode(data, buf.ptr, entropy_on_host=False)
            want = rounds[name][str(S)]
            if refusal:
                with pytest.raises(capi.DmsError, match=refusal) as e:
                    jd.status()
                assert e.value.code == ing.DMS_ERR_FORMAT and want["verdict"] == refusal
                refused += 1
            else:
                jd.status()
            info = jd.info
            what = "%s S=%d" % (name, S)
            assert (info.subsequences, info.rounds, info.settled_lanes) == (want["lanes"], want["rounds"], want["settled"]), what
            assert info.subsequence_bytes == S and info.entropy_on_host == 0 and 1 <= info.rounds <= ing.JPEG_DEV_ROUNDS, what
            scan = len(data) - data.find(b"\xff\xda")
            if scan > S + 64:
                assert info.subsequences > 1, what
        jd.close()
    assert refused == 3 * 4
    z = np.load(os.path.join(GOLDEN, "jpeg_cases.npz"))
    jd = ing.JpegDevice(64, 48)
    buf = capi.DeviceBuffer(64 * 48 * 3)
    good = streams["q95_420"][2]
    for data, code, text in ((z["progressive_jpeg"].tobytes(), ing.DMS_ERR_UNSUPPORTED, "progressive"), (b"\x00" * 64, ing.DMS_ERR_FORMAT, "not a JPEG"),
                             (streams["q85_444"][2], ing.DMS_ERR_FORMAT, "image size differs"),
                             (good.replace(b"\xff\xc4", b"\xff\xe4"), ing.DMS_ERR_FORMAT, "missing table")):
        for on_host in (False, True):
            with pytest.raises(capi.DmsError, match=text) as e:
                jd.decode(data, buf.ptr, entropy_on_host=on_host)
            assert e.value.code == code
    jd.decode(good, buf.ptr, entropy_on_host=False)  # the object is still usable
    jd.status()
    assert np.array_equal(buf.download(np.uint8, (48, 64, 3)), streams["q95_420"][4])
    jd.close()


def test_one_object_many_decodes(ing, streams):
    """The 640x480 stream, then the 2x3 one, then a restart stream on one object (dms_jpeg_dev_set_image_size between them), in both
    entropy modes: the bytes equal a fresh object's and the host decoder's; slots + 2 decodes enqueued with no synchronisation in
    between are all right; two runs give identical bytes."""
    from densemonoslam_amd import capi

    vga, tiny, q95, rst, cut = (streams[n] for n in ("q95_420_vga", "q80_420_2x3", "q95_420", "q50_420_restart", "restart_mcu_420"))
    jd = ing.JpegDevice(640, 480, slots=2)
    for on_host in (False, True):
        for s in (vga, tiny, rst, cut, vga):
            jd.set_image_size(s[0], s[1])
            fresh = ing.JpegDevice(s[0], s[1], max_stream_bytes=len(s[2]), slots=1)
            want = decode_to_host(ing, fresh, s[2], s[0], s[1], entropy_on_host=on_host)
            fresh.close()
            got = decode_to_host(ing, jd, s[2], s[0], s[1], entropy_on_host=on_host)
            assert np.array_equal(got, want) and np.array_equal(got, s[4]), (on_host, s[0], s[1])
    with pytest.raises(capi.DmsError):
        jd.set_image_size(641, 480)
    jd.close()
    # slots + 2 decodes in flight, on a stream of their own, alternating streams and modes
    slots = 3
    jd = ing.JpegDevice(64, 48, slots=slots)
    st = capi.create_stream()
    order = [q95, rst, cut, q95, rst]
    assert len(order) == slots + 2
    runs = []
    for _ in range(2):
        bufs = [capi.DeviceBuffer(64 * 48 * 3) for _ in order]
        for k, (s, b) in enumerate(zip(order, bufs)):
            jd.decode(s[2], b.ptr, flipColors=bool(k & 1), entropy_on_host=(k == 3), stream=st)
        jd.status()
        got = [b.download(np.uint8, (48, 64, 3)) for b in bufs]
        for k, (s, g) in enumerate(zip(order, got)):
            assert np.array_equal(g, s[4][..., ::-1] if k & 1 else s[4]), k
        runs.append(b"".join(g.tobytes() for g in got))
    assert runs[0] == runs[1]
    jd.close()
    capi.destroy_stream(st)


def test_device_readers_feed_the_frame_step_the_host_readers_bytes(ing, tmp_path):
    """A .klg and an LCM log of three 320x240 frames each (compressed, raw, compressed) through dms_klg_next_device /
    dms_frame_unpack_device: depth and colour equal the host readers'; fed to dms_fusion_process_frame behind
    dms_fusion_inputs_ready(f, producer), with pipeline_ingest 1 and 0, the pose, the frame result and the surfel map are byte for
    byte those of the same frames decoded on the host and copied."""
    Image = pytest.importorskip("PIL.Image")
    from densemonoslam_amd import capi, fusion, synth
    from oracle import orc_frame

    W, H, K = 320, 240, (264.0, 264.0, 160.0, 120.0)
    frames = [synth.frame(k, width=W, height=H, K=K, noise=True) for k in range(3)]
    klg = str(tmp_path / "log.klg")
    msgs = []
    with open(klg, "wb") as f:
        f.write(struct.pack("<i", 3))
        for k, (d, rgb, _) in enumerate(frames):
            d = np.ascontiguousarray(d, np.uint16)
            rgb = np.ascontiguousarray(rgb, np.uint8)
            if k == 1:
                db, ib = d.tobytes(), rgb.tobytes()
            else:
                bio = io.BytesIO()
                Image.fromarray(rgb, "RGB").save(bio, "JPEG", quality=90)
                db, ib = zlib.compress(d.tobytes(), 6), bio.getvalue()
            f.write(struct.pack("<qii", 100 + k, len(db), len(ib)) + db + ib)
            msgs.append(ing.Frame(db, ib, 100 + k, k, "cam", False, k != 1, k == 2).encode())
    lcm = str(tmp_path / "log.lcm")
    orc_frame.lcmlog_write(lcm, [(1000 * (k + 1), "EFUSION_FRAMES", m) for k, m in enumerate(msgs)])

    for flip in (False, True):
        r = ing.KlgReader(klg, W, H, flipColors=flip)
        host = list(r)
        r.close()
        assert len(host) == 3
        for on_host in (False, True):
            jd = ing.JpegDevice(W, H, slots=2)
            jd.set_entropy_on_host(on_host)
            st = capi.create_stream()
            deps = [capi.DeviceBuffer(W * H * 2) for _ in host]
            rgbs = [capi.DeviceBuffer(W * H * 3) for _ in host]
            # .klg
            r = ing.KlgReader(klg, W, H, flipColors=flip)
            ts = [r.next_device(jd, d.ptr, c.ptr, stream=st) for d, c in zip(deps, rgbs)]
            assert r.next_device(jd, deps[0].ptr, rgbs[0].ptr, stream=st) is None
            r.close()
            jd.status()
            assert ts == [h[0] for h in host]
            for k, (d, c) in enumerate(zip(deps, rgbs)):
                assert np.array_equal(d.download(np.uint16, (H, W)), host[k][1]), (flip, on_host, k)
                assert np.array_equal(c.download(np.uint8, (H, W, 3)), host[k][2]), (flip, on_host, k)
            # LCM log
            rd = ing.LcmLogReader(lcm)
            for k, (_, data, _) in enumerate(rd):
                m = ing.Frame.decode(data)
                hd, hc = m.unpack(W, H, flipColors=flip)
                dd, dc = capi.DeviceBuffer(W * H * 2), capi.DeviceBuffer(W * H * 3)
                m.unpack_device(jd, dd.ptr, dc.ptr, flipColors=flip, stream=st)
                jd.status()
                assert np.array_equal(dd.download(np.uint16, (H, W)), hd) and np.array_equal(hd, host[k][1]), (flip, on_host, k)
                assert np.array_equal(dc.download(np.uint8, (H, W, 3)), hc) and np.array_equal(hc, host[k][2]), (flip, on_host, k)
            rd.close()
            jd.close()
            capi.destroy_stream(st)

    # the frame step
    r = ing.KlgReader(klg, W, H, flipColors=True)
    host = list(r)
    r.close()

    def result_bytes(res):
        return C.string_at(C.addressof(res), C.sizeof(res))

    def run(device, pipe):
        g = fusion.ElasticFusion(W, H, K, model_capacity=300000, pipeline_ingest=pipe)
        deps = [capi.DeviceBuffer(W * H * 2) for _ in host]
        rgbs = [capi.DeviceBuffer(W * H * 3) for _ in host]
        producer = capi.create_stream() if pipe else None  # pipeline_ingest = 0: the ingest runs on the frame's own stream
        jd = ing.JpegDevice(W, H, slots=2)
        jd.set_entropy_on_host(pipe == 0)  # one run with the entropy decode on the device, one with the host's
        rd = ing.KlgReader(klg, W, H, flipColors=True)
        for k in range(3):
            if device:
                assert rd.next_device(jd, deps[k].ptr, rgbs[k].ptr, stream=producer) == host[k][0]
            else:
                deps[k].upload(host[k][1])
                rgbs[k].upload(host[k][2])
            g.inputsReady(producer)
            g.processFrameAsync(rgbs[k].ptr, 3, deps[k].ptr)
        res = g.fetch()
        check = capi.check
        check(capi.lib.dms_fusion_inputs_consumed(g.h, None), "dms_fusion_inputs_consumed")
        m = g.globalModel().downloadMap()
        rd.close()
        jd.close()
        if producer:
            capi.destroy_stream(producer)
        return result_bytes(res), m

    for pipe in (1, 0):
        ref_res, ref_map = run(False, pipe)
        got_res, got_map = run(True, pipe)
        assert got_res == ref_res, pipe
        assert len(got_map) == len(ref_map) and len(ref_map) > 10000
        for f in got_map.dtype.names:
            assert got_map[f].tobytes() == ref_map[f].tobytes(), (pipe, f)
