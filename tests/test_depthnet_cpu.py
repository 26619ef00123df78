"""The restatement of the depth network's two tensor conversions (tests/depthnet_ref.py, the specification of
include/dmslam_depthnet.h) against vectors worked out by hand from DepthPrediction.cpp:106-169: the fp32 product by the single nearest
to 1/255, the plane order, round-half-even on exact ties of the fp32 product x * 1000, saturation, and what happens to the values
the x86 float -> int32 conversion cannot represent."""
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depthnet_ref as D  # noqa: E402

F = np.float32
INF, NAN = float("inf"), float("nan")

# metres (rounded to fp32 first) -> the fp32 product with 1000 -> RUNTIME, TRUNCATE.  The four ties are exact in fp32:
# float(0.0005) = 0x3A03126F and 0x3A03126F * 1000.0f = 0.5 exactly, and so on (the decimals themselves are not ties).
UNPACK_F32 = [
    (0.0005, 0.5, 0, 0),          # tie -> even (down)
    (0.0015, 1.5, 2, 1),          # tie -> even (up)
    (0.0025, 2.5, 2, 2),          # tie -> even (down)
    (2.0005, 2000.5, 2000, 2000),  # tie -> even (down)
    (0.0019, None, 2, 1),         # an ordinary value between: rounds up, truncates down
    (-0.001, -1.0, 0, 0),
    (-0.0, -0.0, 0, 0),
    (65.535, 65535.00390625, 65535, 65535),
    (65.5354, 65535.3984375, 65535, 65535),
    (65.536, 65536.0, 65535, 65535),       # saturates
    (1e6, 1e9, 65535, 65535),              # below 2^31: still an int32, saturates
    (3e6, 3e9, 0, 65535),                  # beyond 2^31: INT_MIN -> 0 at run time; the offline clip keeps 65535
    (INF, INF, 0, 65535),
    (-INF, -INF, 0, 0),
    (NAN, NAN, 0, 0),
]
# fp16 bit patterns: the largest finite half (65504 m) and +inf
UNPACK_F16 = [(0x7BFF, 65535, 65535), (0x7C00, 0, 65535), (0xFC00, 0, 0), (0x7E00, 0, 0), (0x8000, 0, 0),
              (0x3C00, 1000, 1000),   # 1 m
              (0x3E00, 1500, 1500),   # 1.5 m
              (0x0001, 0, 0)]         # the smallest subnormal, 2^-24 m


def bits32(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def test_pack_is_one_single_multiply_by_the_single_nearest_to_1_over_255():
    assert bits32(D.INV255) == 0x3B808081
    img = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, axis=2)
    got = D.pack(img)
    assert got.dtype == np.float32 and got.shape == (3, 16, 16)
    want = np.array([np.float32(v) * np.float32(1 / 255) for v in range(256)], np.float32)
    for c in range(3):
        assert np.array_equal(got[c].reshape(-1).view(np.uint32), want.view(np.uint32))
    # by hand: exact ends, and bytes where the product differs from the division byte / 255 in the last bit
    for v, b in [(0, 0x00000000), (1, 0x3B808081), (2, 0x3C008081), (3, 0x3C40C0C2), (127, 0x3EFEFF00), (128, 0x3F008081),
                 (254, 0x3F7EFF00), (255, 0x3F800000)]:
        assert int(got[0].reshape(-1).view(np.uint32)[v]) == b, (v, hex(b))
    division = (np.arange(256, dtype=np.float32) / np.float32(255)).astype(np.float32)
    assert int((division.view(np.uint32) != want.view(np.uint32)).sum()) == 126  # not a division: 126 of the 256 bytes tell


def test_pack_half_is_round_to_nearest_even_of_the_fp32_value():
    img = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, axis=2)
    got = D.pack(img, half=True)
    assert got.dtype == np.float16 and got.shape == (3, 16, 16)
    want = np.array([np.float32(v) * np.float32(1 / 255) for v in range(256)], np.float32).astype(np.float16)
    assert np.array_equal(got[1].reshape(-1).view(np.uint16), want.view(np.uint16))
    for v, b in [(0, 0x0000), (1, 0x1C04), (3, 0x2206), (128, 0x3804), (255, 0x3C00)]:
        assert int(got[2].reshape(-1).view(np.uint16)[v]) == b, (v, hex(b))


def test_pack_plane_order_at_3_and_4_bytes_per_pixel():
    W, H = 3, 2
    px = np.arange(W * H, dtype=np.uint8).reshape(H, W)
    rgb = np.stack([10 + px, 100 + px, 200 + px], -1)  # distinct channels
    for img in (rgb, np.concatenate([rgb, np.full((H, W, 1), 77, np.uint8)], -1)):
        got = D.pack(img)
        assert got.shape == (3, H, W)
        for c, base in enumerate((10, 100, 200)):
            for y in range(H):
                for x in range(W):
                    assert got[c, y, x] == np.float32(base + y * W + x) * np.float32(1 / 255)
        assert not np.any(got == np.float32(77) * np.float32(1 / 255))  # the fourth byte goes nowhere


def test_unpack_table_fp32_both_modes():
    x = np.array([m for m, _, _, _ in UNPACK_F32], np.float32)
    for (m, r, _, _), xi in zip(UNPACK_F32, x):
        if r is not None and r == r:  # the product itself, where the table states it
            assert np.float32(xi) * np.float32(1000.0) == np.float32(r) and float(np.float32(r)) == r, (m, r)
    assert bits32(np.float32(0.0005)) == 0x3A03126F
    got_r, got_t = D.unpack(x, D.RUNTIME), D.unpack(x, D.TRUNCATE)
    assert got_r.dtype == np.uint16 and got_t.dtype == np.uint16
    assert [int(v) for v in got_r] == [w for _, _, w, _ in UNPACK_F32]
    assert [int(v) for v in got_t] == [w for _, _, _, w in UNPACK_F32]
    assert np.array_equal(D.unpack(x), got_r)  # the run-time rule is the default
    assert np.array_equal(D.unpack(x.reshape(3, 5)), got_r.reshape(3, 5))


def test_unpack_table_fp16_both_modes():
    h = np.array([b for b, _, _ in UNPACK_F16], np.uint16).view(np.float16)
    assert float(h[0]) == 65504.0 and np.isposinf(h[1]) and np.isneginf(h[2]) and np.isnan(h[3])
    assert [int(v) for v in D.unpack(h, D.RUNTIME)] == [w for _, w, _ in UNPACK_F16]
    assert [int(v) for v in D.unpack(h, D.TRUNCATE)] == [w for _, _, w in UNPACK_F16]
    # every fp16 value, against the same rule spelt out value by value in Python's exact arithmetic
    allh = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)
    got_r, got_t = D.unpack(allh, D.RUNTIME), D.unpack(allh, D.TRUNCATE)
    for i in range(0, 65536, 97):
        r = float(np.float32(float(allh[i])) * np.float32(1000.0))
        if r != r:
            wr = wt = 0
        else:
            wt = int(min(max(r, 0.0), 65535.0))
            wr = 0 if abs(r) == INF or abs(round(r)) >= 2 ** 31 else min(max(round(r), 0), 65535)  # Python's round: half to even
        assert (int(got_r[i]), int(got_t[i])) == (wr, wt), (i, r)
