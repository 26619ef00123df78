#!/usr/bin/env python3
"""Golden vectors of JPEG colour ENCODING: every case is encoded by libjpeg itself (Pillow's bundled libjpeg-turbo, the library
behind jpeg_cases.npz) with Image.save(buf, "JPEG", quality=q, subsampling=s) and decoded again by Pillow.  Run where Pillow is:

    python tests/golden/make_jpeg_encode_golden.py     # writes tests/golden/jpeg_encode_cases.npz

Stored per case: the input (cases up to 160x120; larger ones are regenerated from their recorded seed by scene(), and the
SHA-256 of the input says whether that worked), Pillow's whole file, and its decode (small cases in full, the SHA-256 always).
csrc/jpeg_enc.hpp and csrc/jpeg_enc_dev.hip must reproduce every byte of every file (tests/test_jpeg_encode_cpu.py, _gpu.py;
tests/jpeg_encode_cases.py loads this file without Pillow).

At least one case must end its entropy-coded data with FF (so that a stuffed 00 stands right before EOI): the seed of the
9x9 case is searched for that, and `ends_with_ff` records the case."""
import hashlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

SEED = 20261021
STORE_INPUT_UP_TO = 160 * 120

# name, width, height, kind, quality, subsampling (Pillow's numbering: 0 = 4:4:4, 2 = 4:2:0)
CASES = [
    ("noise_64x48_q90_420", 64, 48, "noise", 90, 2),      # baseline; many FF bytes
    ("smooth_45x23_q90_420", 45, 23, "smooth", 90, 2),    # ragged both ways, odd chroma width, dummy blocks in the last MCU column and row
    ("noise_70x37_q90_420", 70, 37, "noise", 90, 2),      # ragged with one whole dummy block row
    ("smooth_50x40_q90_444", 50, 40, "smooth", 90, 0),    # the other sampling
    ("noise_17x33_q100_420", 17, 33, "noise", 100, 2),    # all divisors 8
    ("smooth_96x64_q30_420", 96, 64, "smooth", 30, 2),    # long zero runs (ZRL), EOB-only blocks
    ("grey_16x16_q90_420", 16, 16, "grey", 90, 2),        # zero DC differences
    ("checker_16x16_q90_420", 16, 16, "checker", 90, 2),  # DC category extremes, signs
    ("noise_1x1_q90_420", 1, 1, "noise", 90, 2),          # one MCU that is mostly padding
    ("noise_8x8_q90_420", 8, 8, "noise", 90, 2),
    ("noise_9x9_q90_420", 9, 9, "noise", 90, 2),          # its seed is searched: the stream ends FF 00 FF D9
    ("smooth_640x480_q90_420", 640, 480, "smooth", 90, 2),  # the reference converters' setting at the workload's size
]
FF_CASE = "noise_9x9_q90_420"


def make_input(kind, w, h, seed):
    from make_jpeg_golden import scene

    if kind == "grey":
        return np.full((h, w, 3), 128, np.uint8)
    if kind == "checker":  # 8x8 squares of (0,0,0) / (255,255,255): every block flat, the DC jumps between the extremes
        y, x = np.mgrid[0:h, 0:w]
        return np.repeat((((x // 8 + y // 8) % 2) * 255).astype(np.uint8)[..., None], 3, -1)
    return scene(w, h, np.random.default_rng(seed), kind)


def pillow(img, q, s):
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(img, "RGB").save(buf, "JPEG", quality=q, subsampling=s)
    data = buf.getvalue()
    dec = np.asarray(Image.open(io.BytesIO(data)).convert("RGB")).copy()
    return data, dec


def main():
    import PIL
    from PIL import features

    out = {"names": np.array([c[0] for c in CASES])}
    for k, (name, w, h, kind, q, s) in enumerate(CASES):
        seed = SEED + k
        img = make_input(kind, w, h, seed)
        data, dec = pillow(img, q, s)
        if name == FF_CASE:
            while data[-4:] != b"\xff\x00\xff\xd9":
                seed += 1000
                img = make_input(kind, w, h, seed)
                data, dec = pillow(img, q, s)
        out[name + "_shape"] = np.array([w, h], np.int32)
        out[name + "_params"] = np.array([q, s], np.int32)
        out[name + "_kind"] = np.array([kind])
        out[name + "_seed"] = np.array([seed], np.int64)
        out[name + "_input_sha256"] = np.frombuffer(hashlib.sha256(img.tobytes()).digest(), np.uint8)
        if w * h <= STORE_INPUT_UP_TO:
            out[name + "_input"] = img
            out[name + "_rgb"] = dec
        out[name + "_jpeg"] = np.frombuffer(data, np.uint8)
        out[name + "_sha256"] = np.frombuffer(hashlib.sha256(dec.tobytes()).digest(), np.uint8)
        print(name, len(data), "bytes, seed", seed, "FF bytes in the scan:", data.count(b"\xff\x00"), "ends", data[-4:].hex())
    assert out[FF_CASE + "_jpeg"].tobytes()[-4:] == b"\xff\x00\xff\xd9"
    out["ends_with_ff"] = np.array([FF_CASE])
    out["libjpeg"] = np.array(["Pillow %s, libjpeg API %s, libjpeg-turbo %s" % (PIL.__version__, features.version_codec("jpg"),
                                                                                features.version_feature("libjpeg_turbo"))])
    print(out["libjpeg"])
    np.savez_compressed(os.path.join(HERE, "jpeg_encode_cases.npz"), **out)


if __name__ == "__main__":
    main()
