"""CPU side of the device JPEG decoder (include/dmslam_io_device.h, csrc/jpeg_dev.hip): the sequential decoder rebuilt as three
stages over the arithmetic both sides compile (csrc/jpeg_core.hpp), the parallel entropy algorithm restated with its lanes run
one after another (tests/jpeg_lanes_host.cpp, under the address and undefined-behaviour sanitizers), and the new header."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def all_streams():
    """(name, width, height, bytes, fixture) of every stream of both fixtures that passes the parse stage"""
    out = []
    for fn in ("jpeg_cases.npz", "jpeg_device_cases.npz"):
        z = np.load(os.path.join(GOLDEN, fn))
        for name in [str(n) for n in z["names"]]:
            w, h = [int(v) for v in z[name + "_shape"]]
            out.append((name, w, h, z[name + "_jpeg"].tobytes(), z))
    return out


def test_three_stage_decoder_reproduces_libjpeg_bytes():
    """parse -> entropy -> back half (csrc/jpeg.hpp decode_rgb, through dms_jpeg_decode): libjpeg's bytes for every stream of both
    fixtures that libjpeg decoded, the recorded refusal for the altered ones, and the progressive stream is still unsupported."""
    from densemonoslam_amd import ingest as ing
    from densemonoslam_amd.capi import DmsError

    checked = 0
    for name, w, h, data, z in all_streams():
        refusal = str(z[name + "_refusal"][0]) if name + "_refusal" in z else ""
        if refusal:
            with pytest.raises(DmsError, match=refusal):
                ing.jpeg_decode(data, w, h)
            continue
        got = ing.jpeg_decode(data, w, h)
        if name + "_sha256" in z:
            assert hashlib.sha256(got.tobytes()).digest() == z[name + "_sha256"].tobytes(), name
            want = z[name + "_rgb"]
            assert np.array_equal(got[:want.shape[0]], want), name
            checked += 1
    assert checked >= 16
    z = np.load(os.path.join(GOLDEN, "jpeg_cases.npz"))
    with pytest.raises(DmsError) as e:
        ing.jpeg_decode(z["progressive_jpeg"].tobytes(), 32, 24)
    assert e.value.code == ing.DMS_ERR_UNSUPPORTED and "progressive" in str(e.value)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_lanes_run_one_after_another_equal_the_sequential_entropy_stage(tmp_path):
    """tests/jpeg_lanes_host.cpp: S = 32, 64, 128, 256 on every stream, the malformed ones included.  The program itself compares
    coefficients and refusals with the sequential entropy stage; here: no sanitizer report, and the lanes, rounds and settled lanes
    it prints are the recorded ones (tests/golden/jpeg_lane_rounds.json, which the GPU test holds the device to)."""
    exe = str(tmp_path / "jpeg_lanes_host")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + ROOT, os.path.join(ROOT, "tests", "jpeg_lanes_host.cpp"), "-o", exe])
    args = []
    for name, w, h, data, _ in all_streams():
        p = tmp_path / (name + ".jpg")
        p.write_bytes(data)
        args += [name, str(w), str(h), str(p)]
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and not out.stderr.strip(), (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    got = {}
    for line in out.stdout.splitlines():
        name, S, lanes, rounds, settled, verdict = line.split(" ", 5)
        got.setdefault(name, {})[S] = {"lanes": int(lanes), "rounds": int(rounds), "settled": int(settled), "verdict": verdict}
    want = json.load(open(os.path.join(GOLDEN, "jpeg_lane_rounds.json")))
    assert got == want
    assert len(got) == len(all_streams()) and all(sorted(v) == ["128", "256", "32", "64"] for v in got.values())


def test_device_header_is_plain_c_and_declared_symbols_exist(tmp_path):
    """include/dmslam_io_device.h compiles as C99 and as C++11 on its own and declares the device decoder's entry points."""
    src = tmp_path / "abi_check.c"
    src.write_text('#include "dmslam_io_device.h"\n'
                   "int main(void) { dms_jpeg_dev_info i; dms_jpeg_dev* d = 0; (void)i; (void)d; return 0; }\n")
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", inc, "-fsyntax-only", str(src)])
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-I", inc, "-fsyntax-only", "-x", "c++", str(src)])
    from densemonoslam_amd import capi

    for n in ("dms_jpeg_dev_create", "dms_jpeg_dev_destroy", "dms_jpeg_dev_decode", "dms_jpeg_dev_set_subsequence_bytes", "dms_jpeg_dev_set_image_size", "dms_jpeg_dev_status",
              "dms_jpeg_dev_get_coefficients", "dms_frame_unpack_device", "dms_klg_next_device"):
        assert hasattr(capi.lib, n), n
    # argument validation happens before any device access
    assert capi.lib.dms_jpeg_dev_create(None, 640, 480, 1 << 20, 2) == -1
