"""tests/golden/jpeg_encode_cases.npz (tests/golden/make_jpeg_encode_golden.py) for the encoder tests, without Pillow: per case the
input pixels, Pillow's file and the digest of Pillow's decode.  Inputs larger than the generator stores are regenerated from the
recorded seed with its scene() restated here; the recorded SHA-256 of the input says that the regeneration is exact."""
import hashlib
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def smooth_scene(w, h, seed):
    """make_jpeg_golden.scene(w, h, default_rng(seed), "smooth")"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([128 + 100 * np.sin(x / 7.0) * np.cos(y / 5.0), 40 + 200 * x / max(w - 1, 1), 255 - 220 * y / max(h - 1, 1)], -1)
    img = img + rng.normal(0, 3.0, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


class Case:
    def __init__(self, z, name):
        self.name = name
        self.width, self.height = [int(v) for v in z[name + "_shape"]]
        self.quality, self.subsampling = [int(v) for v in z[name + "_params"]]
        self.jpeg = z[name + "_jpeg"].tobytes()
        self.decoded_sha256 = z[name + "_sha256"].tobytes()
        self.decoded = z[name + "_rgb"] if name + "_rgb" in z else None
        if name + "_input" in z:
            self.rgb = np.ascontiguousarray(z[name + "_input"])
        else:
            assert str(z[name + "_kind"][0]) == "smooth", name
            self.rgb = smooth_scene(self.width, self.height, int(z[name + "_seed"][0]))
        assert hashlib.sha256(self.rgb.tobytes()).digest() == z[name + "_input_sha256"].tobytes(), "input of %s not reproduced" % name


_cases = None


def cases():
    """every case of the fixture, loaded once and shared"""
    global _cases
    if _cases is None:
        z = np.load(os.path.join(GOLDEN, "jpeg_encode_cases.npz"))
        _cases = [Case(z, str(n)) for n in z["names"]]
        _cases_ff = str(z["ends_with_ff"][0])
        assert [c for c in _cases if c.name == _cases_ff][0].jpeg[-4:] == b"\xff\x00\xff\xd9"
    return _cases


def by_name(name):
    return [c for c in cases() if c.name == name][0]


VGA = "smooth_640x480_q90_420"
