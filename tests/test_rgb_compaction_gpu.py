"""The resident level kernels' photometric lists (csrc/track.hip gn_level_body: interleaved ownership, block-local compaction of the
gated pixels, waves that skip the slots they hold no entry for) against the CPU oracle, BIT FOR BIT, the way tests/test_tracking_gpu.py
compares whole tracker calls: pose, lastA, lastb, errors and counts, iterations run.

Small images (128 x 96 and the ragged 97 x 61) with the handle's resident budget capped so that level 0 runs several blocks at 2, 3 and
4 pixels per thread, and crafted intensity images that drive the number of compacted slots Q = ceil(list length / 512) of a block:
  flat       nothing passes the gate: every list is empty, Q = 0 everywhere;
  noise      everything passes: Q = pixels per thread;
  stripes_q1 / stripes_q2   column stripes whose edges gate a fraction of the pixels such that the longest list has Q = 1 / Q = 2
             (run lengths per pixels-per-thread in STRIPE_RUN; the oracle's own gradients decide, see _gate);
  tail_rows  gated pixels only in the first rows - the pixels that the masked lanes past the end of the ragged image shadow;
  nan_depth  pixels with window and gradient open whose depth is NaN: the gate's last term keeps them out of the list.
Every case predicts the list length of every block on the CPU - the oracle's gradient images through the gate's definition, the
ownership mapping restated here - and asserts the library's counters against it exactly, then repeats the call with both switches off
(contiguous ownership, every owned pixel in the list) and must get the same bits again.

Then the free-running frame step at 160 x 120 over 6 frames, switches on against switches off: identical poses, results and maps."""
import numpy as np
import pytest

from tests import helpers

pytestmark = pytest.mark.gpu

KPB = 512  # threads per block of the level kernels
CFG = dict(rgbOnly=False, icpWeight=10.0, pyramid=True, fastOdom=False, so3=True)
# (W, H) -> {pixels per thread at level 0: (budget cap that makes the residency rule choose it, blocks)}
SHAPES = {(128, 96): {2: (12, 12), 3: (8, 8), 4: (6, 6)}, (97, 61): {2: (6, 6), 3: (4, 4), 4: (3, 3)}}
CASES = ("flat", "noise", "stripes_q1", "stripes_q2", "tail_rows", "nan_depth")
# column run length of the stripes (two gated columns per edge, so about 2 / run of the pixels are gated) for Q = 1 / Q = 2 of the
# longest list, per pixels-per-thread.  Chosen on the CPU with _gate / _lists below; the test asserts that they give those Q.
STRIPE_RUN = {2: (6, 3), 3: (8, 4), 4: (12, 5)}


@pytest.fixture(scope="module")
def dms():
    from densemonoslam_amd import capi, odometry

    assert capi.device_count() >= 1, "no MI355X visible"
    return odometry


def _K(W, H):
    return (0.825 * W, 0.825 * W, W / 2.0 - 0.25, H / 2.0 + 0.25)


def _image(case, W, H, P):
    """grey image (H, W) uint8 of a case; 0 only where the gate is to stay closed (a zero in the 4 x 4 window closes it whatever the gradient)"""
    rng = np.random.RandomState(1234 + W + 7 * len(case))
    if case == "flat":
        # (the reference's Sobel pads the image with zeros, so the first row and column of a flat image have a gradient; a black
        # pixel in the 4 x 4 window closes the gate there)
        img = np.full((H, W), 128, np.uint8)
        img[0, :] = 0
        img[:, 0] = 0
        return img
    if case in ("noise", "nan_depth"):
        return rng.randint(0, 2, (H, W)).astype(np.uint8) * 180 + 40  # 40 | 220: every Sobel response is far above the gate
    if case in ("stripes_q1", "stripes_q2"):
        run = STRIPE_RUN[P][0 if case == "stripes_q1" else 1]
        cols = ((np.arange(W) // run) % 2).astype(np.uint8) * 140 + 60
        return np.repeat(cols[None, :], H, axis=0)
    if case == "tail_rows":
        img = np.full((H, W), 128, np.uint8)
        img[:2] = rng.randint(0, 2, (2, W)).astype(np.uint8) * 180 + 40
        img[:, 0] = 0  # (closes the gate along the first column, as in the flat image)
        return img
    raise KeyError(case)


_inputs = {}


def _case_inputs(orc, W, H, case, P):
    """Inputs and the oracle's answer for a case; computed once (the stripes depend on P, the rest does not)."""
    key = (W, H, case, P if case.startswith("stripes") else 0)
    if key in _inputs:
        return _inputs[key]
    from densemonoslam_amd import synth

    K = _K(W, H)
    d1, _, T1 = synth.frame(10, width=W, height=H, K=K, noise=False)
    d2, _, _ = synth.frame(11, width=W, height=H, K=K, noise=False)
    vo = orc.createVMap(K, d1, 20.0)
    no = orc.createNMap(vo)
    verts = np.zeros((H, W, 4), np.float32)
    norms = np.zeros((H, W, 4), np.float32)
    ok = ~np.isnan(vo[:H]) & ~np.isnan(no[:H])
    for c in range(3):
        verts[..., c] = np.where(ok, vo[c * H:(c + 1) * H], 0)
        norms[..., c] = np.where(ok, no[c * H:(c + 1) * H], 0)
    if case == "nan_depth":
        # the photometric term's own depth image is made from the vertex map handed to initICPModel (RGBDOdometry::populateRGBDData):
        # a hole there is NaN in that image
        verts[H // 4:H // 2, W // 8:W // 2] = 0
        norms[H // 4:H // 2, W // 8:W // 2] = 0
    grey = _image(case, W, H, P)
    rgba = synth.rgba(np.repeat(grey[:, :, None], 3, axis=2))
    inp = dict(K=K, verts=verts, norms=norms, rgba=rgba, d2=d2, P1=T1.astype(np.float32))
    o = _init(orc.Odometry(W, H, K[2], K[3], K[0], K[1]), inp)
    to, Ro, ro = o.getIncrementalTransformation(inp["P1"][:3, 3], inp["P1"][:3, :3], **CFG)
    inp["oracle"] = (to, Ro, ro)
    inp["keep"], inp["open"] = _gate(o, W, H)
    _inputs[key] = inp
    return inp


def _init(trk, inp):
    trk.initICPModel(inp["verts"], inp["norms"], 20.0, inp["P1"])
    trk.initRGBModel(inp["rgba"])
    trk.initICP(inp["d2"], 20.0)
    trk.initRGB(inp["rgba"])
    trk.initFirstRGB(inp["rgba"])
    return trk


def _gate(o, W, H):
    """The level-0 photometric gate (csrc/pixel_ops.hpp rgb_load_own) from the ORACLE's images after its call: inside the border, the
    clipped 4 x 4 window all non-zero, squared Sobel magnitude >= 1600 (minimum gradient 5 over the Sobel scale 1 / 8), depth not NaN."""
    img, gx, gy, d = o.buffer(7, 0), o.buffer(9, 0).astype(np.int64), o.buffer(10, 0).astype(np.int64), o.buffer(5, 0)
    assert img.shape == (H, W)
    nz = img > 0
    win = np.ones((H, W), bool)
    for du in range(-2, 2):
        for dv in range(-2, 2):
            yy = np.clip(np.arange(H) + du, 0, H - 1)
            xx = np.clip(np.arange(W) + dv, 0, W - 1)
            win &= nz[yy][:, xx]
    inside = (np.arange(W)[None, :] < W - 5) & (np.arange(H)[:, None] < H - 1)
    is_open = inside & win & ((gx * gx + gy * gy).astype(np.float32) >= np.float32(1600.0))
    return is_open & ~np.isnan(d), is_open  # (the gate; the gate without its depth term)


def _lists(keep, P, nb, interleave):
    """list length of every block: the kept pixels among those it owns (csrc/track_ownership.hpp, restated)"""
    N = keep.size
    flat = keep.reshape(-1)
    n = np.zeros(nb, np.int64)
    for b in range(nb):
        for p in range(P):
            for w in range(KPB // 64):
                seg = (p * (KPB // 64) + w) * nb + b if interleave else (b * P + p) * (KPB // 64) + w
                lo, hi = seg * 64, min(seg * 64 + 64, N)
                if lo < N:
                    n[b] += int(flat[lo:hi].sum())
    assert int(n.sum()) == int(flat.sum())  # every pixel owned once
    return n


def _slots(n):
    return int(((n + KPB - 1) // KPB).max())


def _assert_same(got, want, g, what):
    (tg, Rg, rg), (to, Ro, ro) = got, want
    helpers.assert_pose_identical(tg, Rg, to, Ro, what=what)
    assert list(rg.iterations_run) == list(ro.iterations_run), what
    assert rg.so3_iterations_run == ro.so3_iterations_run, what
    assert rg.rejected_jump == ro.rejected_jump, what
    for f in ("lastICPError", "lastICPCount", "lastRGBError", "lastRGBCount", "lastSO3Error", "lastSO3Count"):
        a, b = np.float32(getattr(rg, f)), np.float32(getattr(ro, f))
        assert a.tobytes() == b.tobytes() or (np.isnan(a) and np.isnan(b)), (what, f, a, b)
    assert helpers.nan_equal(np.array(rg.lastA), np.array(ro.lastA)), what + " lastA"
    assert helpers.nan_equal(np.array(rg.lastb), np.array(ro.lastb)), what + " lastb"
    assert g.canonRetries() == ro.canon_retries, (what, g.canonRetries(), ro.canon_retries)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("P", [2, 3, 4])
@pytest.mark.parametrize("size", sorted(SHAPES), ids=lambda s: "%dx%d" % s)
def test_lists_reach_their_slot_counts_and_bits_equal_the_oracle(dms, orc, size, P, case, monkeypatch):
    from densemonoslam_amd.capi import lib

    for v in ("DMS_TRACK_MODE", "DMS_PERSIST_MAX_BLOCKS", "DMS_PERSIST_BLOCKS", "DMS_RGB_COMPACT", "DMS_TRACK_INTERLEAVE"):
        monkeypatch.delenv(v, raising=False)
    W, H = size
    cap, nb = SHAPES[size][P]
    inp = _case_inputs(orc, W, H, case, P)
    keep = inp["keep"]
    live = np.ones_like(keep)
    # ---- what the case was built for, decided on the CPU from the oracle's gate
    n_on = _lists(keep, P, nb, True)
    want_slots = {"flat": 0, "noise": P, "stripes_q1": 1, "stripes_q2": 2}.get(case)
    if want_slots is not None:
        assert _slots(n_on) == want_slots, (case, n_on)
    if case == "flat":
        assert not keep.any()
    if case == "tail_rows":
        # gated pixels exist, and all of them lie where the lanes past the end of a ragged image shadow pixels (index % N: the first rows)
        assert keep.any() and not keep[4:].any()
        if W * H % KPB:
            assert nb * P * KPB - W * H >= W  # the tail shadows at least the first row
    if case == "nan_depth":
        hole = (inp["open"] & ~keep)[H // 4:H // 2, W // 8:W // 2]
        assert hole.sum() >= hole.size // 2  # window and gradient open, depth NaN: out of the list

    K = inp["K"]
    g = dms.RGBDOdometry(W, H, K[2], K[3], K[0], K[1])
    try:
        assert lib.dms_odometry_set_resident_budget(g.h, cap, 0) == 0
        for interleave, compact in ((1, 1), (0, 0), (1, 0), (0, 1)):
            g.setOwnership(interleave=interleave, compact=compact)
            _init(g, inp)
            got = g.getIncrementalTransformation(inp["P1"][:3, 3], inp["P1"][:3, :3], **CFG)
            what = "%dx%d P=%d %s interleave=%d compact=%d" % (W, H, P, case, interleave, compact)
            assert g.levelShape(0)[:2] == (P, nb), (what, g.levelShape(0))
            _assert_same(got, inp["oracle"], g, what)
            n = _lists(keep if compact else live, P, nb, bool(interleave))
            assert g.rgbCompaction(0) == (_slots(n), int(n.sum())), (what, g.rgbCompaction(0), n)
            if not compact:
                assert g.rgbCompaction(0) == (P, W * H), what  # every owned pixel: the work of the uncompacted kernel
        # the small levels run one pixel per thread: their lists hold at most one slot
        for lvl in (1, 2):
            q, n = g.rgbCompaction(lvl)
            assert g.levelShape(lvl)[0] == 1 and q <= 1 and n <= (W >> lvl) * (H >> lvl), (lvl, q, n)
    finally:
        g.close()


def test_frame_step_same_with_switches_on_and_off(monkeypatch):
    """The free-running frame step, 160 x 120, 6 frames: interleaved ownership and compaction on (the default) against both off give
    identical poses, frame results and surfel maps."""
    from densemonoslam_amd import fusion, synth

    W, H = 160, 120
    K = (132.0, 132.0, 80.0, 60.0)
    runs = []
    for on in ("1", "0"):
        monkeypatch.setenv("DMS_RGB_COMPACT", on)
        monkeypatch.setenv("DMS_TRACK_INTERLEAVE", on)
        ef = fusion.ElasticFusion(W, H, K, model_capacity=100000)
        out = []
        for k in range(6):
            d, rgb, _ = synth.frame(k, width=W, height=H, K=K, noise=True)
            r = ef.processFrame(rgb, d)
            t = r.track
            out.append((np.array(r.pose, np.float32).tobytes(), int(r.surfels), int(r.tick), bool(r.fused), int(r.tracking_ok), int(r.lost),
                        list(t.iterations_run), t.so3_iterations_run, t.rejected_jump, np.array(t.lastA).tobytes(), np.array(t.lastb).tobytes(),
                        np.array([t.lastICPError, t.lastICPCount, t.lastRGBError, t.lastRGBCount], np.float32).tobytes()))
            if k >= 1:
                assert list(t.iterations_run) == [10, 5, 4], (on, k, list(t.iterations_run))  # the resident levels ran: no timeout, no fallback
        m = ef.globalModel().downloadMap()
        out.append(tuple(m[f].view(np.uint32).tobytes() for f in m.dtype.names))
        runs.append(out)
        del ef
    assert len(runs[0][-1][0]) > 0
    for k in range(6):
        assert runs[0][k] == runs[1][k], "frame %d differs between switches on and off" % k
    assert runs[0][-1] == runs[1][-1], "surfel maps differ between switches on and off"
