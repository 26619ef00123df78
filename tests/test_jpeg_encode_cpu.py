"""Recording, CPU side (include/dmslam_io.h writers' half): the host JPEG encoder (csrc/jpeg_enc.hpp over csrc/jpeg_enc_core.hpp)
must write libjpeg's bytes, the whole file from SOI to EOI, for every case of tests/golden/jpeg_encode_cases.npz - no tolerance; the
.klg and LCM-log writers must write the oracle writers' bytes; the device entropy stage's per-block functions, run one block after
another under the sanitizers (tests/jpeg_enc_host.cpp), must give the sequential stage's bytes."""
import hashlib
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

from tests import jpeg_encode_cases as jc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ing():
    from densemonoslam_amd import ingest

    return ingest


def test_fixture_has_the_cases_the_encoder_can_go_wrong_on():
    cases = jc.cases()
    assert len(cases) == 12
    shapes = {(c.width, c.height, c.quality, c.subsampling) for c in cases}
    for want in ((64, 48, 90, 2), (45, 23, 90, 2), (70, 37, 90, 2), (50, 40, 90, 0), (17, 33, 100, 2), (96, 64, 30, 2), (16, 16, 90, 2), (1, 1, 90, 2),
                 (8, 8, 90, 2), (9, 9, 90, 2), (640, 480, 90, 2)):
        assert want in shapes, want
    assert any(c.jpeg[-4:] == b"\xff\x00\xff\xd9" for c in cases)  # a stuffed 00 right before EOI
    assert sum(c.jpeg.count(b"\xff\x00") for c in cases) > 100
    assert os.path.getsize(os.path.join(jc.GOLDEN, "jpeg_encode_cases.npz")) < 1 << 20


def test_host_encoder_writes_libjpegs_bytes(ing):
    """every case, SOI to EOI; with flipColors, the bytes of the channel-swapped input"""
    for c in jc.cases():
        assert ing.jpeg_encode(c.rgb, c.quality, c.subsampling) == c.jpeg, c.name
        assert ing.jpeg_encode(c.rgb[..., ::-1], c.quality, c.subsampling, flipColors=True) == c.jpeg, c.name + " flipped"


def test_decoding_the_encoders_output_gives_the_fixtures_pixels(ing):
    for c in jc.cases():
        got = ing.jpeg_decode(ing.jpeg_encode(c.rgb, c.quality, c.subsampling), c.width, c.height)
        assert hashlib.sha256(got.tobytes()).digest() == c.decoded_sha256, c.name
        if c.decoded is not None:
            assert np.array_equal(got, c.decoded), c.name


def test_encoder_refusals(ing):
    from densemonoslam_amd.capi import DmsError, lib

    img = np.zeros((8, 8, 3), np.uint8)
    for q in (0, 101, -5):
        with pytest.raises(DmsError, match="quality") as e:
            ing.jpeg_encode(img, q)
        assert e.value.code == -1
    with pytest.raises(DmsError, match="subsampling"):
        ing.jpeg_encode(img, 90, 1)  # 4:2:2 is out of scope
    out = np.zeros(1 << 16, np.uint8)
    w = ing.C.c_size_t(0)
    for (wd, ht) in ((0, 8), (8, 0), (65536, 8), (8, 65536), (-1, -1)):
        assert lib.dms_jpeg_encode(img.ctypes.data_as(ing.C.c_void_p), wd, ht, 90, 2, 0, out.ctypes.data_as(ing.C.c_void_p), out.size, ing.C.byref(w)) == -1
        assert b"image size" in lib.dms_last_error()
        assert ing.jpeg_encode_bound(wd, ht) == 0
    assert lib.dms_jpeg_encode(None, 8, 8, 90, 2, 0, out.ctypes.data_as(ing.C.c_void_p), out.size, ing.C.byref(w)) == -1
    # a buffer below the worst case: DMS_ERR_CAPACITY, and the worst-case size comes back
    c = jc.cases()[0]
    bound = ing.jpeg_encode_bound(c.width, c.height, c.subsampling)
    for cap in (0, len(c.jpeg), bound - 1):
        with pytest.raises(DmsError, match="needed") as e:
            ing.jpeg_encode(c.rgb, c.quality, c.subsampling, cap=cap)
        assert e.value.code == ing.DMS_ERR_CAPACITY and ing.jpeg_encode.last_written == bound
    assert ing.jpeg_encode(c.rgb, c.quality, c.subsampling, cap=bound) == c.jpeg
    # a 65535-wide strip is accepted
    assert ing.jpeg_encode(np.zeros((1, 65535, 3), np.uint8), 50)[:2] == b"\xff\xd8"


def test_bound_holds_every_fixture_and_quality_100_noise(ing):
    for c in jc.cases():
        assert ing.jpeg_encode_bound(c.width, c.height, c.subsampling) >= len(c.jpeg), c.name
    c = jc.by_name("noise_17x33_q100_420")
    assert c.quality == 100 and ing.jpeg_encode_bound(17, 33, 2) >= len(c.jpeg)
    # the arithmetic of the bound: header + 64 symbols of 16 + 11 bits per block, doubled, + EOI
    assert ing.jpeg_encode_bound(16, 16, 2) == 623 + 6 * 216 * 2 + 2 and ing.jpeg_encode_bound(16, 16, 0) == 623 + 12 * 216 * 2 + 2
    rng = np.random.default_rng(5)
    for (w, h, s) in ((64, 64, 0), (33, 17, 2)):
        worst = ing.jpeg_encode(rng.integers(0, 256, (h, w, 3)).astype(np.uint8), 100, s)
        assert len(worst) <= ing.jpeg_encode_bound(w, h, s)


def test_writers_write_the_oracle_writers_bytes_and_the_readers_read_them_back(ing, tmp_path):
    from oracle import orc_frame

    c = jc.by_name("noise_64x48_q90_420")
    W, H = c.width, c.height
    rng = np.random.default_rng(11)
    depths = [rng.integers(0, 5000, (H, W)).astype(np.uint16) for _ in range(3)]
    rgbs = [c.rgb, c.rgb[::-1].copy(), c.rgb[:, ::-1].copy()]
    # raw frames, and compressed frames with the zlib and JPEG bytes handed in
    raw = [(100 + k, d, r) for k, (d, r) in enumerate(zip(depths, rgbs))]
    packed = [(200 + k, np.frombuffer(zlib.compress(d.tobytes(), 6), np.uint8), np.frombuffer(ing.jpeg_encode(r), np.uint8))
              for k, (d, r) in enumerate(zip(depths, rgbs))]
    for tag, frames in (("raw", raw), ("packed", packed), ("none", [])):
        want, got = str(tmp_path / (tag + "_want.klg")), str(tmp_path / (tag + "_got.klg"))
        orc_frame.klg_write(want, frames)
        w = ing.KlgWriter(got)
        for ts, d, r in frames:
            w.append(ts, d.tobytes(), r.tobytes())
        w.close()
        assert open(got, "rb").read() == open(want, "rb").read(), tag
        rd = ing.KlgReader(got, W, H, flipColors=(tag == "packed"))  # the loader exchanges R and B of JPEG colour; flipColors undoes it
        assert rd.numFrames == len(frames)
        back = list(rd)
        rd.close()
        assert len(back) == len(frames)
        for k, (ts, d, r) in enumerate(back):
            assert ts == frames[k][0] and np.array_equal(d, depths[k])
            assert np.array_equal(r, rgbs[k] if tag == "raw" else ing.jpeg_decode(packed[k][2].tobytes(), W, H)), (tag, k)
    # a frame without an image
    w = ing.KlgWriter(str(tmp_path / "noimg.klg"))
    w.append(7, depths[0].tobytes())
    w.close()
    orc_frame.klg_write(str(tmp_path / "noimg_want.klg"), [(7, depths[0], None)])
    assert open(str(tmp_path / "noimg.klg"), "rb").read() == open(str(tmp_path / "noimg_want.klg"), "rb").read()

    events = [(1000 * (k + 1), "EFUSION_FRAMES" if k != 1 else "OTHER", ing.Frame(f[1].tobytes(), f[2].tobytes(), f[0], k, "cam", False, k >= 3, k == 5).encode())
              for k, f in enumerate(raw + packed)]
    events.append((9, "EMPTY", b""))
    want, got = str(tmp_path / "want.lcm"), str(tmp_path / "got.lcm")
    orc_frame.lcmlog_write(want, events)
    w = ing.LcmLogWriter(got)
    for ts, ch, data in events:
        w.append(ts, ch, data)
    w.close()
    assert open(got, "rb").read() == open(want, "rb").read()
    rd = ing.LcmLogReader(got)
    back = list(rd)
    rd.close()
    assert back == [(ch, data, ts) for ts, ch, data in events]
    from densemonoslam_amd.capi import DmsError

    with pytest.raises(DmsError):
        ing.KlgWriter(str(tmp_path / "no_such_dir" / "x.klg"))
    with pytest.raises(DmsError):
        ing.LcmLogWriter(str(tmp_path / "no_such_dir" / "x.lcm"))


def test_frame_pack_compressed_round_trip(ing):
    """zlib.decompress returns the depth exactly; dms_frame_unpack returns the depth and the fixture's decoded pixels; the JPEG bytes
    are the fixture's (deflate's own bytes depend on the zlib build and are not pinned)"""
    from oracle import orc_frame

    rng = np.random.default_rng(3)
    for name in ("smooth_45x23_q90_420", "noise_64x48_q90_420"):
        c = jc.by_name(name)
        depth = rng.integers(0, 6000, (c.height, c.width)).astype(np.uint16)
        f = ing.frame_pack(depth, c.rgb, compressed=True, quality=c.quality, timestamp=123456789012, frameNumber=7, senderName="rec")
        assert f.compressed and f.image == c.jpeg and (f.timestamp, f.frameNumber, f.senderName) == (123456789012, 7, "rec")
        assert zlib.decompress(f.depth) == depth.tobytes()
        d, rgb = f.unpack(c.width, c.height, flipColors=True)  # libjpeg's R, G, B order
        assert np.array_equal(d, depth) and np.array_equal(rgb, c.decoded)
        # R and B exchanged on the way in, as OpenCV's encoder reads the loggers' buffers: unpack without the flag returns the input's order
        g = ing.frame_pack(depth, c.rgb[..., ::-1], compressed=True, quality=c.quality, flipColors=True)
        assert g.image == c.jpeg
        assert orc_frame.frame_decode(f.encode())["image"] == c.jpeg
        raw = ing.frame_pack(depth, c.rgb, compressed=False, timestamp=5)
        assert not raw.compressed and raw.depth == depth.tobytes() and raw.image == c.rgb.tobytes()
        d, rgb = raw.unpack(c.width, c.height)
        assert np.array_equal(d, depth) and np.array_equal(rgb, c.rgb)
    assert zlib.decompress(ing.deflate(b"abc" * 1000)) == b"abc" * 1000


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_blocks_run_one_after_another_equal_the_sequential_entropy_stage(tmp_path):
    """tests/jpeg_enc_host.cpp over every fixture case, built with the address and undefined-behaviour sanitizers: the program
    compares the per-block stage with the sequential one and with libjpeg's file; here: exit 0, no sanitizer report, one line a case."""
    exe = str(tmp_path / "jpeg_enc_host")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + ROOT, os.path.join(ROOT, "tests", "jpeg_enc_host.cpp"), "-o", exe])
    args = []
    for c in jc.cases():
        rgb, jpg = tmp_path / (c.name + ".rgb"), tmp_path / (c.name + ".jpg")
        rgb.write_bytes(c.rgb.tobytes())
        jpg.write_bytes(c.jpeg)
        args += [c.name, str(c.width), str(c.height), str(c.quality), str(c.subsampling), str(rgb), str(jpg)]
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and not out.stderr.strip(), (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    lines = out.stdout.splitlines()
    assert len(lines) == len(jc.cases()) and all(l.endswith(" ok") for l in lines), out.stdout
    by = {l.split()[0]: l.split() for l in lines}
    assert int(by[jc.VGA][1]) == 7200 and int(by["noise_70x37_q90_420"][1]) == 5 * 3 * 6  # dummy blocks are blocks of the scan


def test_write_header_is_plain_c_and_declares_the_device_encoder(tmp_path):
    src = tmp_path / "abi_check.c"
    src.write_text('#include "dmslam_io_write.h"\n'
                   "int main(void) { dms_jpeg_enc* e = 0; dms_klg_writer* k = 0; dms_lcmlog_writer* l = 0; (void)e; (void)k; (void)l; return DMS_JPEG_420; }\n")
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", inc, "-fsyntax-only", str(src)])
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-I", inc, "-fsyntax-only", "-x", "c++", str(src)])
    from densemonoslam_amd import capi, ingest

    for n in ("dms_jpeg_enc_create", "dms_jpeg_enc_destroy", "dms_jpeg_enc_set_image_size", "dms_jpeg_enc_encode", "dms_jpeg_enc_result",
              "dms_jpeg_enc_result_at", "dms_jpeg_enc_set_entropy_on_host", "dms_frame_pack_device", "dms_klg_writer_append_device",
              "dms_lcmlog_writer_append_frame_device"):
        assert hasattr(capi.lib, n), n
    assert capi.lib.dms_jpeg_enc_create(None, 640, 480, 2) == -1  # argument validation happens before any device access
    hdr = open(os.path.join(inc, "dmslam_io_write.h")).read()
    assert "#define DMS_JPEG_ENC_DEFAULT_ENTROPY_ON_HOST %d" % ingest.JPEG_ENC_DEFAULT_ENTROPY_ON_HOST in hdr
