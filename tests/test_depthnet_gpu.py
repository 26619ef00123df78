"""The depth network's two tensor conversions (include/dmslam_depthnet.h) on the MI355X through the C ABI, bit for bit against the CPU
restatement tests/depthnet_ref.py: both sides are one IEEE multiply and one rounding, so there is no tolerance.  Shapes are the
smallest at which the kernels' head / 16-byte groups / tail split and the choice between the grouped and the element-wise pack can
go wrong, plus the camera size once per kernel and precision."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depthnet_ref as D  # noqa: E402
from test_depthnet_cpu import UNPACK_F16, UNPACK_F32  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
SMALL = [(1, 1), (3, 2), (5, 3), (7, 1), (17, 5), (64, 4), (67, 3)]  # (width, height)
REAL = (640, 480)
GUARD = 64       # bytes on either side of every output
FILL = 0xA5
INVALID_ARG = -1


@pytest.fixture(scope="module")
def dn():
    from densemonoslam_amd import capi, depthnet

    assert capi.device_count() >= 1, "no MI355X visible"
    return depthnet


def _eq(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    bad = np.argwhere(a != b)
    assert len(bad) == 0, "%s differs at %d places, first %s: %s vs %s" % (what, len(bad), bad[:3].tolist(), a[tuple(bad[0])], b[tuple(bad[0])])


class Guarded:
    """An output of `nbytes` bytes, `offset` bytes into an allocation, with GUARD bytes of FILL before and after it"""

    def __init__(self, nbytes, offset):
        from densemonoslam_amd import capi

        self.nbytes, self.lead = nbytes, GUARD + offset
        self.total = self.lead + nbytes + GUARD
        self.buf = capi.DeviceBuffer(self.total)
        self.buf.upload(np.full(self.total, FILL, np.uint8))
        self.ptr = self.buf.ptr + self.lead

    def result(self, dtype, what=""):
        raw = self.buf.download(np.uint8, (self.total,))
        assert np.all(raw[:self.lead] == FILL) and np.all(raw[self.lead + self.nbytes:] == FILL), "%s: wrote outside its output" % what
        return raw[self.lead:self.lead + self.nbytes].copy().view(dtype)

    def untouched(self):
        return bool(np.all(self.buf.download(np.uint8, (self.total,)) == FILL))


def _input(arr, offset_bytes):
    from densemonoslam_amd import capi

    raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    buf = capi.DeviceBuffer(offset_bytes + raw.size + 16)
    buf.upload(np.concatenate([np.zeros(offset_bytes, np.uint8), raw]))
    return buf, buf.ptr + offset_bytes


def run_pack(dn, rgb, half, in_off=0, out_off=0, what=""):
    H, W, ch = rgb.shape
    es = 2 if half else 4
    keep, src = _input(rgb, in_off)
    out = Guarded(3 * W * H * es, out_off * es)
    dn.pack(src, ch, W, H, out.ptr, half)
    return out.result(np.uint16 if half else np.uint32, what).reshape(3, H, W)


def run_unpack(dn, x, mode, in_off=0, out_off=0, what=""):
    H, W = x.shape
    half = x.dtype == np.float16
    keep, src = _input(x, in_off * x.dtype.itemsize)
    out = Guarded(W * H * 2, out_off * 2)
    dn.unpack(src, half, W, H, out.ptr, mode)
    return out.result(np.uint16, what).reshape(H, W)


def _bits(t):
    return t.view(np.uint16 if t.dtype == np.float16 else np.uint32)


def _image(rng, W, H, ch):
    """random bytes, with all 256 values in it where they fit"""
    img = rng.integers(0, 256, (H, W, ch), dtype=np.uint8)
    flat = img.reshape(-1)
    k = min(256, flat.size)
    flat[:k] = np.arange(k, dtype=np.uint8)
    return img


def _field(rng, W, H, half):
    """random metres from [-1, 70] with the CPU test's table at its start (as much of it as fits) and again at its end"""
    x = rng.uniform(-1.0, 70.0, W * H).astype(F)
    if half:
        x = x.astype(np.float16)
        table = np.array([b for b, _, _ in UNPACK_F16], np.uint16).view(np.float16)
    else:
        table = np.array([m for m, _, _, _ in UNPACK_F32], F)
    k = min(len(table), x.size)
    x[:k] = table[:k]
    x[x.size - k:] = table[len(table) - k:]
    return x.reshape(H, W)


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("ch", [3, 4])
def test_pack_small_shapes(dn, ch, half):
    rng = np.random.default_rng(100 + ch + 10 * half)
    for (W, H) in SMALL:
        img = _image(rng, W, H, ch)
        what = "pack %dx%d ch %d half %d" % (W, H, ch, half)
        _eq(run_pack(dn, img, half, what=what), _bits(D.pack(img, half)), what)


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
def test_pack_all_256_values(dn, half):
    for ch in (3, 4):
        img = np.arange(256, dtype=np.uint8).reshape(8, 32, 1).repeat(ch, axis=2).copy()
        img[..., 1] = img[..., 0][::-1, ::-1]  # distinct planes
        img[..., 2] = np.roll(img[..., 0], 7)
        got = run_pack(dn, img, half)
        _eq(got, _bits(D.pack(img, half)), "pack 256 values ch %d half %d" % (ch, half))
        want = np.array([F(v) * F(1 / 255) for v in range(256)], F)
        _eq(got[0].reshape(-1), _bits(want.astype(np.float16) if half else want), "plane 0 against the product itself")


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
def test_pack_offset_bases(dn, half):
    """device pointers 1, 2, 3 elements into an allocation, input and output, on a grouped shape (17 x 8, 64 x 4) and an element-wise one"""
    rng = np.random.default_rng(7 + half)
    for (W, H) in [(17, 8), (64, 4), (67, 3)]:
        for ch in (3, 4):
            img = _image(rng, W, H, ch)
            want = _bits(D.pack(img, half))
            for in_off in (0, 1, 2, 3):
                for out_off in (0, 1, 2, 3):
                    what = "pack %dx%d ch %d half %d in+%d out+%d" % (W, H, ch, half, in_off, out_off)
                    _eq(run_pack(dn, img, half, in_off, out_off, what), want, what)


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("mode", [D.RUNTIME, D.TRUNCATE], ids=["runtime", "truncate"])
def test_unpack_small_shapes_and_offsets(dn, mode, half):
    rng = np.random.default_rng(200 + mode + 10 * half)
    for (W, H) in SMALL:
        x = _field(rng, W, H, half)
        what = "unpack %dx%d half %d mode %d" % (W, H, half, mode)
        _eq(run_unpack(dn, x, mode, what=what), D.unpack(x, mode), what)
    for (W, H) in [(17, 5), (64, 4)]:
        x = _field(rng, W, H, half)
        want = D.unpack(x, mode)
        for in_off in (0, 1, 2, 3):
            for out_off in (0, 1, 2, 3):
                what = "unpack %dx%d half %d mode %d in+%d out+%d" % (W, H, half, mode, in_off, out_off)
                _eq(run_unpack(dn, x, mode, in_off, out_off, what), want, what)


def test_unpack_table(dn):
    """the CPU test's table, value by value against its hand-computed columns"""
    x = np.array([m for m, _, _, _ in UNPACK_F32], F).reshape(1, -1)
    assert run_unpack(dn, x, D.RUNTIME).reshape(-1).tolist() == [w for _, _, w, _ in UNPACK_F32]
    assert run_unpack(dn, x, D.TRUNCATE).reshape(-1).tolist() == [w for _, _, _, w in UNPACK_F32]
    h = np.array([b for b, _, _ in UNPACK_F16], np.uint16).view(np.float16).reshape(1, -1)
    assert run_unpack(dn, h, D.RUNTIME).reshape(-1).tolist() == [w for _, w, _ in UNPACK_F16]
    assert run_unpack(dn, h, D.TRUNCATE).reshape(-1).tolist() == [w for _, _, w in UNPACK_F16]


def test_unpack_what_is_no_int32_gives_zero(dn):
    """every NaN, both infinities and every |x * 1000| >= 2^31 -> 0 under the run-time rule; just below 2^31 saturates instead"""
    nans = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF], np.uint32).view(F)
    big = np.array([np.inf, -np.inf, 2147484.0, -2147484.0, 3e6, -3e6, 1e30, -1e30, 3.4e38, -3.4e38, 3.4e36], F)
    x = np.concatenate([nans, big]).astype(F)
    x = np.concatenate([x, x, x])[:48].reshape(3, 16)  # head, group and tail lanes all see them
    got = run_unpack(dn, x, D.RUNTIME, out_off=3)
    assert not got.any(), got
    _eq(run_unpack(dn, x, D.TRUNCATE), D.unpack(x, D.TRUNCATE), "truncate on the same values")
    below = np.array([[2147483.5, 1e6, 65.536, -2147483.5]], F)  # 2147483.5 * 1000 rounds to 2^31 - 128: still an int32
    assert run_unpack(dn, below, D.RUNTIME).reshape(-1).tolist() == [65535, 65535, 65535, 0]
    hx = np.array([0x7C00, 0xFC00, 0x7E00, 0xFE00, 0x7C01, 0xFFFF, 0x7DFF, 0x7C00], np.uint16).view(np.float16).reshape(1, 8)
    assert not run_unpack(dn, hx, D.RUNTIME).any()
    every = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16).reshape(256, 256)  # all of fp16
    for mode in (D.RUNTIME, D.TRUNCATE):
        _eq(run_unpack(dn, every, mode), D.unpack(every, mode), "every fp16 value, mode %d" % mode)


@pytest.fixture(scope="module")
def real_image():
    rng = np.random.default_rng(31)
    return _image(rng, REAL[0], REAL[1], 3)


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
def test_pack_camera_size(dn, real_image, half):
    _eq(run_pack(dn, real_image, half), _bits(D.pack(real_image, half)), "pack 640x480")


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
def test_unpack_camera_size(dn, half):
    x = _field(np.random.default_rng(32 + half), REAL[0], REAL[1], half)
    _eq(run_unpack(dn, x, D.RUNTIME), D.unpack(x, D.RUNTIME), "unpack 640x480")


def test_invalid_arguments_write_nothing(dn):
    from densemonoslam_amd import capi

    lib = capi.lib
    W, H = 8, 4
    img = np.zeros((H, W, 4), np.uint8)
    keep, src = _input(img, 0)
    xin = np.ones((H, W), F)
    keep2, xsrc = _input(xin, 0)
    out = Guarded(3 * W * H * 4, 0)
    P = C.c_void_p
    bad_pack = [(None, 3, W, H, P(out.ptr), 0), (P(src), 3, W, H, None, 0), (P(src), 3, 0, H, P(out.ptr), 0), (P(src), 3, W, -1, P(out.ptr), 0),
                (P(src), 2, W, H, P(out.ptr), 0), (P(src), 5, W, H, P(out.ptr), 0), (P(src), 1, W, H, P(out.ptr), 1),
                (P(src), 3, 65536, 65536, P(out.ptr), 0), (P(src), 3, W, H, P(out.ptr + 2), 0), (P(src), 3, W, H, P(out.ptr + 1), 1)]
    for a in bad_pack:
        assert lib.dms_depthnet_pack(*a, None) == INVALID_ARG, a
        assert lib.dms_last_error()
    bad_unpack = [(None, 0, W, H, P(out.ptr), 0), (P(xsrc), 0, W, H, None, 0), (P(xsrc), 0, 0, H, P(out.ptr), 0), (P(xsrc), 0, W, 0, P(out.ptr), 0),
                  (P(xsrc), 0, -W, H, P(out.ptr), 0), (P(xsrc), 0, W, H, P(out.ptr), 2), (P(xsrc), 0, W, H, P(out.ptr), -1),
                  (P(xsrc), 1, W, H, P(out.ptr), 7), (P(xsrc), 0, 65536, 65536, P(out.ptr), 0), (P(xsrc), 0, W, H, P(out.ptr + 1), 0),
                  (P(xsrc + 2), 0, W, H, P(out.ptr), 0)]
    for a in bad_unpack:
        assert lib.dms_depthnet_unpack(*a, None) == INVALID_ARG, a
    capi.check(lib.dms_stream_sync(None))
    assert out.untouched()
    # the Python class refuses what the ABI would
    with pytest.raises(ValueError):
        dn.DepthPrediction(W, H, mode=5)


def test_predict_hands_the_depth_to_the_frame_step_in_stream_order(dn):
    """DepthPrediction.processFrame with a stand-in network, the producer on a non-default torch stream and pipeline_ingest on: three
    frames give the poses and surfel counts, bit for bit, of the same frames fed with the u16 depth images computed beforehand on
    the host by the restatement."""
    import torch

    from densemonoslam_amd import fusion, synth

    W, H = 320, 240
    K = (264.0, 264.0, 160.0, 120.0)

    def net(t):  # the mean over the channels times 3 plus 0.5 m, as explicit single fp32 operations: 0.5 - 3.5 m
        x = t[:, 0:1] + t[:, 1:2]
        x = x + t[:, 2:3]
        return (x + 0.5).contiguous()

    def net_host(p):
        x = (p[0] + p[1]).astype(F)
        x = (x + p[2]).astype(F)
        return (x + F(0.5)).astype(F)

    frames = [synth.frame(k, width=W, height=H, K=K, noise=True)[1] for k in range(3)]
    depths = [D.unpack(net_host(D.pack(rgb))) for rgb in frames]
    assert all(d.min() >= 500 and d.max() <= 3500 and len(np.unique(d)) > 100 for d in depths)

    ref = fusion.ElasticFusion(W, H, K, model_capacity=300000)
    assert ref.params.pipeline_ingest == 1
    want = []
    for rgb, d in zip(frames, depths):
        r = ref.processFrame(rgb, d)
        want.append((np.array(r.pose, F).view(np.uint32).copy(), int(r.surfels), int(r.tick), int(r.fused)))
    ref.close()
    assert want[-1][1] > 10000

    ef = fusion.ElasticFusion(W, H, K, model_capacity=300000)
    side = torch.cuda.Stream()
    got = []
    with torch.cuda.stream(side):
        dp = dn.DepthPrediction(W, H)  # its tensors are filled on the stream that then writes them
        for k, rgb in enumerate(frames):
            dp.processFrame(ef, rgb, net)
            r = ef.fetch()
            got.append((np.array(r.pose, F).view(np.uint32).copy(), int(r.surfels), int(r.tick), int(r.fused)))
            _eq(dp.depth.cpu().numpy(), depths[k], "frame %d depth image" % k)
    ef.close()
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g[0], w[0]) and g[1:] == w[1:], (k, g, w)
