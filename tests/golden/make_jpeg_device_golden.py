#!/usr/bin/env python3
"""Golden vectors for the device JPEG decoder (csrc/jpeg_dev.hip): streams chosen for what a PARALLEL entropy decoder gets
wrong, encoded and - where they decode - decoded by Pillow's bundled libjpeg-turbo, as make_jpeg_golden.py does.

    python tests/golden/make_jpeg_device_golden.py     # writes tests/golden/jpeg_device_cases.npz (needs the built library)

  noise_q100_444       64x48 noise, quality 100, 4:4:4     long codes and dense FF 00
  smooth_q30_420       160x120 smooth, quality 30, 4:2:0   many blocks of a few bits each per subsequence
  restart_mcu_420      64x48, 4:2:0, restart interval 1    segments shorter than a subsequence
  restart_rows_422     45x23, 4:2:2, restart rows
  cut_420              a valid stream cut in the middle of its scan: the decoder pads the missing bits with zeros (no libjpeg
                       pixels: Pillow does not hand out libjpeg's padded rows)
  bad_ac_run           one byte of the scan altered so that the sequential decoder (dms_jpeg_decode) refuses the stream with
                       "AC run past the block"
  bad_code             the same for "bad Huffman code"
  bad_dc_size          "bad DC size".  No alteration of a SCAN byte can produce it: the DC tables libjpeg writes hold the symbols
                       0..11 only, so a DC size above 15 never decodes.  The altered byte is a symbol of the DC table in the
                       DHT segment instead (found by the same search).
For the altered streams the generator searches for the byte and records offset, new value and the refusal in the fixture."""
import hashlib
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_jpeg_golden import scene  # noqa: E402


def encode(img, **kw):
    buf = io.BytesIO()
    Image.fromarray(img, "RGB").save(buf, "JPEG", **kw)
    return buf.getvalue()


def scan_offset(data):
    """offset of the first byte behind the SOS header"""
    i = 2
    while True:
        assert data[i] == 0xFF
        m = data[i + 1]
        n = (data[i + 2] << 8) | data[i + 3]
        if m == 0xDA:
            return i + 2 + n
        i += 2 + n


def dc_table_symbols(data):
    """offsets of the symbol bytes of the DC tables (DHT, class 0)"""
    out = []
    i = 2
    while data[i + 1] != 0xDA:
        m = data[i + 1]
        n = (data[i + 2] << 8) | data[i + 3]
        if m == 0xC4:
            s, e = i + 4, i + 2 + n
            while s < e:
                cnt = sum(data[s + 1:s + 17])
                if data[s] >> 4 == 0:
                    out += list(range(s + 17, s + 17 + cnt))
                s += 17 + cnt
        i += 2 + n
    return out


def refusal(ing, data, w, h):
    from densemonoslam_amd.capi import DmsError
    try:
        ing.jpeg_decode(data, w, h)
    except DmsError as e:
        return str(e)
    return ""


def search(ing, data, w, h, offsets, values, text):
    for off in offsets:
        for v in values:
            if v == data[off]:
                continue
            bad = bytearray(data)
            bad[off] = v
            # no new marker and no broken stuffing: only the entropy decode may object
            if v == 0xFF or (off > 0 and bad[off - 1] == 0xFF):
                continue
            if text in refusal(ing, bytes(bad), w, h):
                return bytes(bad), off, v
    raise SystemExit("no single-byte alteration gives '%s'" % text)


def main():
    from densemonoslam_amd import ingest as ing

    rng = np.random.default_rng(20261020)
    cases = [
        ("noise_q100_444", 64, 48, "noise", dict(quality=100, subsampling=0)),
        ("smooth_q30_420", 160, 120, "smooth", dict(quality=30, subsampling=2)),
        ("restart_mcu_420", 64, 48, "edges", dict(quality=85, subsampling=2, restart_marker_blocks=1)),
        ("restart_rows_422", 45, 23, "smooth", dict(quality=60, subsampling=1, restart_marker_rows=1)),
    ]
    names, out = [], {}

    def put(name, data, w, h, rgb=None, refuses=""):
        names.append(name)
        out[name + "_jpeg"] = np.frombuffer(data, np.uint8)
        out[name + "_shape"] = np.array([w, h], np.int32)
        out[name + "_refusal"] = np.array([refuses])
        if rgb is not None:
            out[name + "_rgb"] = rgb
            out[name + "_sha256"] = np.frombuffer(hashlib.sha256(rgb.tobytes()).digest(), np.uint8)
        print(name, len(data), "bytes", refuses)

    for name, w, h, kind, kw in cases:
        data = encode(scene(w, h, rng, kind), **kw)
        im = Image.open(io.BytesIO(data))
        assert im.mode == "RGB" and im.size == (w, h)
        put(name, data, w, h, np.asarray(im).copy())

    w, h = 64, 48
    base = encode(scene(w, h, rng, "noise"), quality=90, subsampling=2)
    so = scan_offset(base)
    put("cut_420", base[:so + (len(base) - so) // 2], w, h)
    scan = range(so + 8, len(base) - 2)
    for name, text, offsets in [("bad_ac_run", "AC run past the block", scan), ("bad_code", "bad Huffman code", scan),
                                ("bad_dc_size", "bad DC size", dc_table_symbols(base))]:
        bad, off, v = search(ing, base, w, h, offsets, [0x10, 0x1F, 0x3C, 0xF0, 0xFE, 0x00, 0x55, 0xAA], text)
        put(name, bad, w, h, refuses=text)
        out[name + "_altered"] = np.array([off, base[off], v], np.int32)
    out["names"] = np.array(names)
    np.savez_compressed(os.path.join(HERE, "jpeg_device_cases.npz"), **out)
    write_lane_rounds()


def write_lane_rounds():
    """tests/golden/jpeg_lane_rounds.json: per stream of both fixtures and subsequence size, what tests/jpeg_lanes_host.cpp prints -
    lanes, relaxation rounds, lanes left to the single-lane pass, verdict.  The CPU test holds the program to it, the GPU test the
    device."""
    import json
    import subprocess
    import tempfile

    root = os.path.dirname(os.path.dirname(HERE))
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "jpeg_lanes_host")
        subprocess.check_call(["g++", "-std=c++14", "-O1", "-I" + root, os.path.join(root, "tests", "jpeg_lanes_host.cpp"), "-o", exe])
        args = []
        for fn in ("jpeg_cases.npz", "jpeg_device_cases.npz"):
            z = np.load(os.path.join(HERE, fn))
            for name in [str(n) for n in z["names"]]:
                p = os.path.join(td, name + ".jpg")
                with open(p, "wb") as f:
                    f.write(z[name + "_jpeg"].tobytes())
                args += [name, str(int(z[name + "_shape"][0])), str(int(z[name + "_shape"][1])), p]
        text = subprocess.run([exe] + args, check=True, capture_output=True, text=True).stdout
    got = {}
    for line in text.splitlines():
        name, S, lanes, rounds, settled, verdict = line.split(" ", 5)
        got.setdefault(name, {})[S] = {"lanes": int(lanes), "rounds": int(rounds), "settled": int(settled), "verdict": verdict}
    with open(os.path.join(HERE, "jpeg_lane_rounds.json"), "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
