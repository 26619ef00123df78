"""fused_associate (include/dmslam_fusion.h): a fusing frame projects its first index map into a z-buffer only and the association
resolves the texels it needs from there (k_fuse_associate_zbuf), instead of index map images + k_fuse_associate.

Bar: both paths resolve a texel with one function (surfel.hpp resolve_texel) and associate with one body (fuse_associate_body), on
the same z-buffer winners; nothing in between is a floating-point reduction.  So everything is compared for equal BITS: the
association's slot planes, associated surfels, flags and the per-surfel winners at kernel level; poses, frame results and maps at
frame level.

Kernel-level sizes (a block of the new kernel owns 8 x 16 candidates = 16 x 32 pixels and a 17 x 33 texel tile): 64 x 48 (a multiple
of the tile in x, ragged in y), 70 x 46 and 33 x 17 (ragged both ways, odd sizes; with both tick parities the windows of the first
and last candidate column / row are clipped at all four borders), 16 x 32 (one tile, one block), 32 x 64 (2 x 2 tiles: every halo
crosses a block boundary)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EMPTY = 0xFFFFFFFF
SIZES = {
    "64x48": (64, 48),
    "70x46": (70, 46),
    "33x17": (33, 17),
    "16x32": (16, 32),
    "32x64": (32, 64),
}


@pytest.fixture(autouse=True)
def _no_override(monkeypatch):
    monkeypatch.delenv("DMS_FUSED_ASSOCIATE", raising=False)  # (the A/B switch would override the parameter under test)


@pytest.fixture(scope="module")
def fus():
    from densemonoslam_amd import capi, fusion

    assert capi.device_count() >= 1, "no MI355X visible"
    return fusion


def cam_of(W, H):
    return (0.825 * W, 0.825 * W, W / 2.0, H / 2.0)  # (264 at 320 x 240)


@functools.lru_cache(maxsize=None)
def scene_of(size):
    """Two synthetic frames at this size: (K, [(depth u16, rgba, pose relative to the first)])"""
    from densemonoslam_amd import synth

    W, H = SIZES[size]
    K = cam_of(W, H)
    out, T0 = [], None
    for k in (0, 1):
        d, rgb, T = synth.frame(k, width=W, height=H, K=K, noise=True)
        T0 = T if T0 is None else T0
        out.append((d, synth.rgba(rgb), (np.linalg.inv(T0) @ T).astype(np.float32)))
    return K, out


@functools.lru_cache(maxsize=None)
def boot_map(size):
    """The map the first frame initialises, downloaded (shared by the cases of this size; never changed)"""
    from densemonoslam_amd import fusion as fus

    W, H = SIZES[size]
    K, frames = scene_of(size)
    d, rgba, _ = frames[0]
    df = fus.depth_bilateral(d, 3.0)
    gm = fus.GlobalModel(W, H, capacity=4 * W * H)
    gm.initialise(rgba, fus.depth_metric(d, 3.0), fus.depth_metric(df, 3.0), K, 1, 0, 25.0)
    m = gm.downloadMap()
    gm.close()
    m.setflags(write=False)
    return m


def associate_both(fus, size, time, surfels, pose=None):
    """The association of frame 1 against `surfels` at tick `time`, by index map images + k_fuse_associate and by z-buffer +
    k_fuse_associate_zbuf: per path (scratch after the association, map after the update pass, row-major index map or None)."""
    W, H = SIZES[size]
    K, frames = scene_of(size)
    d, rgba, P = frames[1]
    P = P if pose is None else pose
    df = fus.depth_bilateral(d, 3.0)
    dm, dmf = fus.depth_metric(d, 3.0), fus.depth_metric(df, 3.0)
    dp = fus.DevicePose(P)
    out = []
    for zbuf in (False, True):
        gm = fus.GlobalModel(W, H, capacity=4 * W * H)
        if len(surfels):
            gm.upload(surfels)
        im = None
        if zbuf:
            gm.projectIndices(dp, time, 0, K, 25.0, 200)
        else:
            im = fus.IndexMap(W, H)
            im.predictIndices(dp, time, 0, gm, K, 25.0, 200)
        gm.fuseEx(dp, time, 0, rgba, dm, dmf, im, K, 25.0, 0.75, defer_update=True)
        s = gm.fuseScratch(max(len(surfels), 1))
        gm.applyPending()
        after = gm.downloadMap() if len(surfels) else surfels
        out.append((s, after, im.download_index() if im is not None else None))
        gm.close()
    return out


def same_association(a, b, what):
    (sa, ma, _), (sb, mb, _) = a, b
    assert sa["slot_flag"].tobytes() == sb["slot_flag"].tobytes(), "%s: slot_flag differs" % what
    live = sa["slot_flag"] != 0  # (a slot with flag 0 holds nothing: nobody reads its planes)
    for f in ("slot_pos", "slot_col", "slot_nrm", "slot_best"):
        assert sa[f][live].tobytes() == sb[f][live].tobytes(), "%s: %s differs" % (what, f)
    assert sa["winner"].tobytes() == sb["winner"].tobytes(), "%s: winner differs" % what
    assert len(ma) == len(mb)
    for f in ma.dtype.names:
        assert ma[f].tobytes() == mb[f].tobytes(), "%s: map field %s after the update pass differs" % (what, f)


@pytest.mark.parametrize("time", [2, 3])
@pytest.mark.parametrize("size", list(SIZES))
def test_association_same_bits(fus, size, time):
    """Every size at both tick parities: slots, flags, associated surfels, winners and the updated map."""
    m = boot_map(size)
    a, b = associate_both(fus, size, time, m)
    same_association(a, b, "%s tick %d" % (size, time))
    s = b[0]
    W, H = SIZES[size]
    assert (s["slot_flag"] == 1).sum() > 0.2 * (W // 2) * (H // 2), "hardly anything associated: the comparison says little"
    won = s["winner"] != EMPTY
    assert won.sum() > 0 and (s["winner"][won] < len(s["slot_flag"])).all()
    # the clipped windows: candidates of the first and last column and row of this parity are measured
    sw, sh = (W + 1) // 2, (H + 1) // 2
    fl = s["slot_flag"].reshape(sw, sh)  # column-major slots: [i][j]
    last_i = (W - 1 - time % 2) // 2
    last_j = (H - 1 - time % 2) // 2
    assert fl[0].any() and fl[last_i].any() and fl[:, 0].any() and fl[:, last_j].any(), "a border of the candidate grid is empty"


def test_empty_zbuffer(fus):
    """Nothing projects (the camera looks away from the map): every measurement is new, nobody wins."""
    size = "70x46"
    m = boot_map(size)
    away = np.diag([-1.0, 1.0, -1.0, 1.0]).astype(np.float32)  # half a turn about y
    a, b = associate_both(fus, size, 2, m, pose=away)
    same_association(a, b, "empty z-buffer")
    assert (a[2][0] == 0).all() and (a[2][1] == 0).all(), "the index map is not empty"
    assert (b[0]["slot_flag"] == 1).sum() == 0 and (b[0]["slot_flag"] == 2).sum() > 0
    assert (b[0]["winner"] == EMPTY).all()
    # and an empty map
    a, b = associate_both(fus, size, 3, m[:0])
    same_association(a, b, "empty map")
    assert (b[0]["slot_flag"] == 2).sum() > 0


@pytest.mark.parametrize("time", [2, 3])
def test_surfel_zero_wins_a_pixel(fus, time):
    """Surfel 0 is indistinguishable from "no surfel" in the index image (`current > 0u`): a map whose surfel 0 is visible in the
    middle of the image gives index 0 with a live vertex there, and nothing associates with it on either path."""
    size = "32x64"
    W, H = SIZES[size]
    m = boot_map(size).copy()
    c = len(m) // 2 + H // 4  # (bootstrap order is column-major: about the middle of the image)
    m[[0, c]] = m[[c, 0]]
    a, b = associate_both(fus, size, time, m)
    same_association(a, b, "surfel 0 tick %d" % time)
    idx, vc = a[2][0], a[2][1]
    assert ((idx == 0) & (vc[..., 3] > 0)).any(), "surfel 0 does not win a pixel"
    assert b[0]["winner"][0] == EMPTY and not ((b[0]["slot_flag"] == 1) & (b[0]["slot_best"] == 0)).any()


# ---- frame level ----------------------------------------------------------------------------------------------------------------
FW, FH, FK = 160, 120, (132.0, 132.0, 80.0, 60.0)
N_FRAMES = 7  # the bootstrap frame and six tracked, fusing ones


@functools.lru_cache(maxsize=None)
def session_frames():
    from densemonoslam_amd import synth

    return tuple(synth.frame(k, width=FW, height=FH, K=FK, noise=True) for k in range(N_FRAMES))


def result_bytes(r):
    t = r.track
    scal = np.array([r.surfels, r.tick, r.fused, r.fill_in, r.weighting, r.nid_score, r.tracking_ok, r.lost, r.loop_ok, r.loop_constraints,
                     r.loop_icp_error, r.loop_icp_count], np.float64)
    parts = [np.array(r.pose, np.float32), scal, np.array(r.loop_pose, np.float32), np.array(r.loop_cov_diag, np.float64),
             np.array([t.lastICPError, t.lastICPCount, t.lastRGBError, t.lastRGBCount, t.lastSO3Error, t.lastSO3Count], np.float32),
             np.array(t.lastA, np.float64), np.array(t.lastb, np.float64), np.array(t.iterations_run, np.float64)]
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


def run_session(fus, keep_dirty=False, **opts):
    """(per frame: result bytes, fused, downloaded map)"""
    from densemonoslam_amd.fusion import lib

    g = fus.ElasticFusion(FW, FH, FK, model_capacity=200000, **opts)
    if keep_dirty:
        assert lib.dms_fusion_debug_keep_assoc_zbuf(g.h, 1) == 0
    per = []
    for d, rgb, _ in session_frames():
        r = g.processFrame(rgb, d)
        per.append((result_bytes(r), bool(r.fused), g.globalModel().downloadMap()))
    g.close()
    return per


def same_session(a, b, what):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert x[0] == y[0], "%s: frame result of frame %d differs" % (what, k)
        assert len(x[2]) == len(y[2]), "%s: frame %d, surfel count %d vs %d" % (what, k, len(x[2]), len(y[2]))
        for f in x[2].dtype.names:
            assert x[2][f].tobytes() == y[2][f].tobytes(), "%s: frame %d, map field %s differs" % (what, k, f)


@pytest.fixture(scope="module")
def unfused_session(fus):
    import os

    old = os.environ.pop("DMS_FUSED_ASSOCIATE", None)
    os.environ["DMS_FUSED_ASSOCIATE"] = "0"
    try:
        per = run_session(fus)
    finally:
        del os.environ["DMS_FUSED_ASSOCIATE"]
        if old is not None:
            os.environ["DMS_FUSED_ASSOCIATE"] = old
    assert sum(f for _, f, _ in per[1:]) == N_FRAMES - 1, "not every tracked frame fused"
    return per


def test_frames_same_bits_switch_on_and_off(fus, unfused_session, monkeypatch):
    """Six tracked frames with DMS_FUSED_ASSOCIATE=1 against =0: poses, results and the map after every frame.  A key left behind in
    the association's z-buffer would change the next frame's association, and with it that frame's map."""
    monkeypatch.setenv("DMS_FUSED_ASSOCIATE", "1")
    same_session(run_session(fus, fused_associate=0), unfused_session, "DMS_FUSED_ASSOCIATE=1")  # (the switch beats the parameter)


def test_parameter_defaults_on_and_can_be_switched_off(fus, unfused_session):
    g = fus.ElasticFusion(FW, FH, FK, model_capacity=200000)
    assert g.params.fused_associate == 1
    g.close()
    same_session(run_session(fus, fused_associate=0), unfused_session, "fused_associate=0")
    same_session(run_session(fus), unfused_session, "default")


def test_hand_back_path(fus, unfused_session):
    """The z-buffer is not handed back empty (test hook: as after an error return between a frame's two index maps): every fusing
    frame finds it in use, full of the previous frame's keys, and clears it itself first."""
    same_session(run_session(fus, keep_dirty=True), unfused_session, "dirty z-buffer")

