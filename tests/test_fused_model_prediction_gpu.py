"""fused_model_prediction (include/dmslam_fusion.h): the tracking prediction of an eligible frame is resolved straight into the
tracker's model pyramid (fusion_map.hip: k_predict_model) instead of resolve + fill-in images, then the model pyramid kernel.

Bar: the new kernel resolves, fills, selects and stores with the functions the two kernels it replaces use (resolved_image /
resolved_geometry, fill_pixel_values, model_level0_store, model_level_down, store_transformed), the depth / intensity pyramid steps
are the same bodies on the same level-0 values, the denseEnough count is an integer, and the build contracts no multiply-add: nothing
may differ.  Everything is compared for equal BITS against the option off - no tolerance anywhere.

Sizes (an 8 x 8 pixel tile per wave holds 4 x 4 level-1 and 2 x 2 level-2 pixels): 40 x 40 (the frame step's minimum; 5 x 5 tiles, two
denseEnough samples a side), 77 x 47 (odd at every level, ragged tiles both ways), 130 x 98 (level 1 is 65 x 49: odd, so the last
level-1 column and row have no level-2 pixel), 640 x 480 (1 200 blocks of four waves, 768 samples)."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SWITCH = "DMS_FUSED_MODEL_PREDICTION"
SIZES = {"40x40": (40, 40, 7), "77x47": (77, 47, 7), "130x98": (130, 98, 7), "640x480": (640, 480, 4)}  # W, H, frames (the first one bootstraps)
VMAP, NMAP, DEPTH, IMAGE = 2, 3, 4, 6  # dms_odometry_get_buffer: vmaps_g_prev, nmaps_g_prev, lastDepth, lastImage
PRED_IMAGES = (9, 10, 11, 12, 13, 14, 15)


@pytest.fixture(autouse=True)
def _no_override(monkeypatch):
    for v in (SWITCH, "DMS_TRACK_MODE", "DMS_PREDICT_MODEL_THREADS"):
        monkeypatch.delenv(v, raising=False)  # (the switches would override what the cases set)


@pytest.fixture(scope="module")
def fus():
    from densemonoslam_amd import capi, fusion

    assert capi.device_count() >= 1, "no MI355X visible"
    return fusion


def cam_of(W, H):
    return (0.825 * W, 0.825 * W, W / 2.0, H / 2.0)  # (264 at 320 x 240)


@functools.lru_cache(maxsize=None)
def frames_of(W, H, n):
    from densemonoslam_amd import synth

    return tuple(synth.frame(k, width=W, height=H, K=cam_of(W, H), noise=True)[:2] for k in range(n))


def yaw(deg):
    a = np.radians(deg)
    R = np.eye(4, dtype=np.float32)
    R[0, 0] = R[2, 2] = np.cos(a)
    R[0, 2] = np.sin(a)
    R[2, 0] = -np.sin(a)
    return R


def model_buffers(g):
    """The tracker's twelve model buffers as they stand: {(which, level): array}"""
    from densemonoslam_amd import capi
    from densemonoslam_amd.fusion import Image2D, lib

    out = {}
    h = g.odometryHandle()
    for which, dt in ((VMAP, np.float32), (NMAP, np.float32), (DEPTH, np.float32), (IMAGE, np.uint8)):
        for level in range(3):
            v = Image2D()
            assert lib.dms_odometry_get_buffer(h, which, level, C.byref(v)) == 0
            out[(which, level)] = np.ascontiguousarray(capi.download_view(v, dt, 1))
    return out


def same_model_buffers(a, b, what):
    for (which, level), x in a.items():
        y = b[(which, level)]
        assert x.shape == y.shape
        if which in (VMAP, NMAP):  # stacked planes x | y | z: y and z are never written where x is NaN
            rows = x.shape[0] // 3
            xb, yb = x.view(np.uint32), y.view(np.uint32)
            assert np.array_equal(xb[:rows], yb[:rows]), "%s: buffer %d level %d, x plane differs" % (what, which, level)
            ok = ~np.isnan(x[:rows])
            for p in (1, 2):
                assert np.array_equal(xb[p * rows:(p + 1) * rows][ok], yb[p * rows:(p + 1) * rows][ok]), \
                    "%s: buffer %d level %d, plane %d differs" % (what, which, level, p)
        elif which == DEPTH:
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), "%s: depth level %d differs" % (what, level)
        else:
            assert np.array_equal(x, y), "%s: intensity level %d differs" % (what, level)


def result_bytes(r):
    t = r.track
    scal = np.array([r.surfels, r.tick, r.fused, r.fill_in, r.weighting, r.nid_score, r.tracking_ok, r.lost, r.loop_ok, r.loop_constraints,
                     r.loop_icp_error, r.loop_icp_count], np.float64)
    parts = [np.array(r.pose, np.float32), scal, np.array(r.loop_pose, np.float32), np.array(r.loop_cov_diag, np.float64),
             np.array([t.lastICPError, t.lastICPCount, t.lastRGBError, t.lastRGBCount, t.lastSO3Error, t.lastSO3Count], np.float32),
             np.array(t.lastA, np.float64), np.array(t.lastb, np.float64), np.array(t.iterations_run, np.float64)]
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


def run(fus, W, H, frames, priors=None, buffers=False, maps=False, images_after=(), arm=False, **opts):
    """One context over `frames` (one-call frames): per frame (result bytes, fill_in, model buffers or None, map or None,
    prediction images or None, armed frame block or None); and the predict stats at the end."""
    from densemonoslam_amd import capi, collab

    g = fus.ElasticFusion(W, H, cam_of(W, H), model_capacity=max(200000, 2 * W * H), **opts)
    blk = None
    if arm:
        T = collab.thumbnail_bytes(W, H)
        blk = capi.DeviceBuffer(T + 128)
        blk.upload(np.full(T + 128, 0xAB, np.uint8))
    per = []
    for k, (d, rgb) in enumerate(frames):
        if arm:
            g.armFrameBlock(blk.ptr, blk.ptr + T, blk.ptr + T + 64, 100 + k)
        r = g.processFrame(rgb, d, inPose=(priors or {}).get(k))
        per.append((result_bytes(r), int(r.fill_in), model_buffers(g) if buffers and k > 0 else None,
                    g.globalModel().downloadMap() if maps else None,
                    tuple(g.image(i).copy() for i in PRED_IMAGES) if k in images_after else None,
                    blk.download(np.uint8, (T + 128,)).tobytes() if arm else None))
    stats = g.predictStats()
    g.close()
    return per, stats


def same_runs(a, b, what):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        w = "%s, frame %d" % (what, k)
        assert x[1] == y[1], "%s: fill_in %d vs %d" % (w, x[1], y[1])
        if x[2] is not None:
            same_model_buffers(x[2], y[2], w)
        assert x[0] == y[0], "%s: frame result differs" % w
        if x[3] is not None:
            assert len(x[3]) == len(y[3]), "%s: surfel count %d vs %d" % (w, len(x[3]), len(y[3]))
            for f in x[3].dtype.names:
                assert x[3][f].tobytes() == y[3][f].tobytes(), "%s: map field %s differs" % (w, f)
        if x[4] is not None:
            for i, p, q in zip(PRED_IMAGES, x[4], y[4]):
                assert p.tobytes() == q.tobytes(), "%s: image %d differs" % (w, i)
        assert x[5] == y[5], "%s: armed frame block differs" % w


# ---- 1. the model pyramid ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", list(SIZES))
def test_model_pyramid_same_bits(fus, size):
    """All twelve model buffers after every tracked one-call frame, option 1 against option 0."""
    W, H, n = SIZES[size]
    frames = frames_of(W, H, n)
    on, s_on = run(fus, W, H, frames, buffers=True, fused_model_prediction=1)
    off, s_off = run(fus, W, H, frames, buffers=True, fused_model_prediction=0)
    assert s_on == {"fused": n - 1, "plain": 0} and s_off == {"fused": 0, "plain": n - 1}
    same_runs(on, off, size)
    v0 = on[-1][2][(VMAP, 0)]
    assert (~np.isnan(v0[:H])).mean() > 0.5, "hardly any model vertex: the comparison says little"


# ---- 2. both decisions ------------------------------------------------------------------------------------------------------------
def test_both_dense_decisions(fus):
    """A caller-supplied prior turns the camera 25 degrees onto unmapped wall at frame 3: the view is dense before (fill_in 0) and
    not dense from there on (fill_in 1) - chosen with the oracle pipeline on the CPU (orc_pipeline: fill_in 0, 0, 0, 1, 1, 1), so
    both source selections of the fused kernel run, the second with the stale-projection branch in front of it."""
    W, H = 160, 120
    frames = frames_of(W, H, 6)
    priors = {3: yaw(25.0)}
    on, s_on = run(fus, W, H, frames, priors=priors, buffers=True, maps=True, fused_model_prediction=1)
    off, _ = run(fus, W, H, frames, priors=priors, buffers=True, maps=True, fused_model_prediction=0)
    assert s_on["fused"] == 5 and s_on["plain"] == 0
    flags = [p[1] for p in on[1:]]
    assert 0 in flags and 1 in flags, "fill_in takes one value only on this stream: %r" % flags
    same_runs(on, off, "both decisions")


# ---- 3. sessions ------------------------------------------------------------------------------------------------------------------
SW, SH, SN = 160, 120, 10


@pytest.mark.parametrize("case", ["lazy", "eager", "armed"])
def test_sessions_same_bits(fus, case):
    """Ten frames: poses, result scalars, tracker side outputs and the map after every frame.  A sampled z-buffer cell left behind
    would show as a different next prediction (lazy: the next frame resolves that very z-buffer)."""
    opts = {"lazy": dict(lazy_final_prediction=1), "eager": dict(lazy_final_prediction=0), "armed": dict(lazy_final_prediction=1)}[case]
    frames = frames_of(SW, SH, SN)
    on, s_on = run(fus, SW, SH, frames, maps=True, arm=case == "armed", fused_model_prediction=1, **opts)
    off, s_off = run(fus, SW, SH, frames, maps=True, arm=case == "armed", fused_model_prediction=0, **opts)
    assert s_on == {"fused": SN - 1, "plain": 0}, "an armed frame block must not disqualify"
    assert s_off["fused"] == 0
    same_runs(on, off, case)


# ---- 4. what a caller sees --------------------------------------------------------------------------------------------------------
def test_images_after_a_frame(fus):
    """dms_fusion_get_image 9 - 15 after frames on the new path: the final prediction, the same bits as with the option off."""
    frames = frames_of(SW, SH, 5)
    on, s_on = run(fus, SW, SH, frames, images_after=(2, 4), fused_model_prediction=1)
    off, _ = run(fus, SW, SH, frames, images_after=(2, 4), fused_model_prediction=0)
    assert s_on["fused"] == 4
    same_runs(on, off, "images")
    assert on[2][4][4].any() and on[4][4][5].any(), "the filled images are empty"  # (the map is younger than the final prediction's confidence threshold: only the fill-in shows)


def test_two_phase_form_is_plain(fus):
    """Between _begin and _end the caller may look: the images are the tracking prediction, and the frame counts as plain."""
    frames = frames_of(SW, SH, 3)
    seen = []
    for opt in (1, 0):
        g = fus.ElasticFusion(SW, SH, cam_of(SW, SH), model_capacity=200000, fused_model_prediction=opt)
        imgs = None
        for d, rgb in frames:
            g.processFrameBegin(rgb, d)
            imgs = tuple(g.image(i).copy() for i in PRED_IMAGES)
            g.processFrameEnd()
            r = g.fetch()
        seen.append((imgs, result_bytes(r), g.predictStats()))
        g.close()
    assert seen[0][2] == {"fused": 0, "plain": 2} and seen[1][2] == {"fused": 0, "plain": 2}
    for i, p, q in zip(PRED_IMAGES, seen[0][0], seen[1][0]):
        assert p.tobytes() == q.tobytes(), "image %d between the halves differs" % i
    assert seen[0][0][0].any(), "no tracking prediction between the halves"
    assert seen[0][1] == seen[1][1]


# ---- 5. fallbacks -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["nid_keyframing", "local_loop_closure", "frameToFrameRGB", "so3=0", "DMS_TRACK_MODE=launches"])
def test_fallbacks(fus, case, monkeypatch):
    """Every disqualifying setting takes the two launches (fused == 0) and stays bit-identical to the option off."""
    opts = {}
    if "=" in case and case.startswith("DMS_"):
        k, v = case.split("=")
        monkeypatch.setenv(k, v)
    elif case == "so3=0":
        opts["so3"] = 0
    else:
        opts[case] = 1
    frames = frames_of(SW, SH, 4)
    on, s_on = run(fus, SW, SH, frames, buffers=True, maps=True, fused_model_prediction=1, **opts)
    off, _ = run(fus, SW, SH, frames, buffers=True, maps=True, fused_model_prediction=0, **opts)
    assert s_on == {"fused": 0, "plain": 3}, case
    same_runs(on, off, case)


def test_lost_camera_is_plain(fus):
    """A lost camera (reloc on; two frames of garbage depth, then none at all: the frames fail the error test and after more than ten
    of them the camera is lost) takes the pass-through fill-in: plain frames, the same bits; while it is not lost the frames are fused."""
    W, H = 320, 240
    rng = np.random.default_rng(5)
    frames = []
    for k, (d, rgb) in enumerate(frames_of(W, H, 16)):
        if 3 <= k <= 4:
            d = rng.integers(500, 3000, d.shape).astype(np.uint16)
        elif k >= 5:
            d = np.zeros_like(d)
        frames.append((d, rgb))
    on, s_on = run(fus, W, H, frames, reloc=1, fused_model_prediction=1)
    off, _ = run(fus, W, H, frames, reloc=1, fused_model_prediction=0)
    same_runs(on, off, "lost camera")
    lost = [np.frombuffer(p[0][64:64 + 12 * 8], np.float64)[7] != 0 for p in on]
    assert any(lost), "the camera never got lost: the case says nothing"
    n_lost_tracked = sum(1 for k in range(1, len(frames)) if lost[k - 1])  # (a frame that BEGINS lost predicts with the pass-through)
    assert s_on["plain"] == n_lost_tracked and s_on["fused"] == len(frames) - 1 - n_lost_tracked


# ---- 6. the switch beats the parameter --------------------------------------------------------------------------------------------
def test_switch_beats_parameter(fus, monkeypatch):
    frames = frames_of(SW, SH, 3)
    g = fus.ElasticFusion(SW, SH, cam_of(SW, SH), model_capacity=200000)
    assert g.params.fused_model_prediction == 1
    g.close()
    ref, _ = run(fus, SW, SH, frames, buffers=True, fused_model_prediction=0)
    monkeypatch.setenv(SWITCH, "0")
    a, s = run(fus, SW, SH, frames, buffers=True, fused_model_prediction=1)
    assert s == {"fused": 0, "plain": 2}
    same_runs(a, ref, SWITCH + "=0")
    monkeypatch.setenv(SWITCH, "1")
    b, s = run(fus, SW, SH, frames, buffers=True, fused_model_prediction=0)
    assert s == {"fused": 2, "plain": 0}
    same_runs(b, ref, SWITCH + "=1")
