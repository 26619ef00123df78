"""fused_clean_projection (include/dmslam_fusion.h): on a fusing frame whose final prediction is deferred, the clean's scatter pass
projects every survivor for the next frame's tracking prediction from the registers that have just stored it, under its new id,
instead of a project launch reading the new map back.

Bar: the same BITS.  Both sides run the same vertex and fragment functions on the same values, and a z-buffer cell's winner is the
minimum of the same 64-bit keys whatever the order of work - so every comparison here is for equality: the raw z-buffer cells, every
plane of the map, the count, every field of a frame's result, every image a caller can ask for.

Stand-alone cases use a 97 x 61 view (no multiple of the sprite groups of four, of the 8 x 8 tiles or of anything else) and crafted
maps uploaded as records; the map and the (W+1)/2 x (H+1)/2 = 1519 measurement slots form the clean's element list, 256 per block."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, K = 97, 61, (66.0, 66.0, 48.5, 30.5)
SLOTS = ((W + 1) // 2) * ((H + 1) // 2)
TIME, DELTA, CUT, CONF = 300, 200, 25.0, 10.0
PROJ = dict(projConfThreshold=0.7, projTime=TIME + 1, projMaxTime=TIME + 1, projTimeDelta=DELTA)  # the next frame's tracking prediction

SIZES = {
    "80x60": (80, 60, (66.0, 66.0, 40.0, 30.0)),
    "97x61": (97, 61, (66.0, 66.0, 48.5, 30.5)),
    "320x240": (320, 240, (264.0, 264.0, 160.0, 120.0)),
}
N_FRAMES = 7  # the bootstrap frame and six tracked ones
PRED_IMAGES = tuple(range(9, 16))


@pytest.fixture(autouse=True)
def _no_override(monkeypatch):
    for v in ("DMS_FUSED_CLEAN_PROJECTION", "DMS_LAZY_FINAL_PREDICTION", "DMS_CLEAN_SUFFIX_MIN", "DMS_CLEAN_INLINE_SCAN_MAX"):
        monkeypatch.delenv(v, raising=False)  # (the A/B switches would override what is under test)


@pytest.fixture(scope="module")
def fus():
    from densemonoslam_amd import capi, fusion

    assert capi.device_count() >= 1, "no MI355X visible"
    return fusion


# ------------------------------------------------------------------------------------------
# stand-alone: dms_model_clean_project against dms_model_clean + dms_splat_project_only
# ------------------------------------------------------------------------------------------
def crafted(fus, n, seed, in_view=1.0, remove_every=0):
    """n surfels in front of an identity camera: stable (confidence 20), seen 5 ticks ago, facing the camera.  in_view: the share
    placed inside the frustum (the rest lies far to the side).  remove_every = r: every r-th surfel is unstable and last seen long
    ago by every sensor - the clean removes it (copy_unstable.vert:137-150), so every later id shifts."""
    rng = np.random.default_rng(seed)
    s = np.zeros(n, fus.SURFEL_DTYPE)
    z = rng.uniform(1.0, 4.0, n).astype(np.float32)
    s["pos"][:, 0] = rng.uniform(-0.7, 0.7, n).astype(np.float32) * z
    s["pos"][:, 1] = rng.uniform(-0.45, 0.45, n).astype(np.float32) * z
    s["pos"][:, 2] = z
    s["pos"][:, 3] = 20.0
    out = rng.uniform(0, 1, n) >= in_view
    s["pos"][out, 0] += 400.0
    nr = rng.normal(0, 0.3, (n, 3)).astype(np.float32)
    nr[:, 2] = -1.0
    s["nrm"][:, :3] = nr / np.linalg.norm(nr, axis=1, keepdims=True)
    s["nrm"][:, 3] = rng.uniform(0.01, 0.08, n).astype(np.float32)
    s["col"][:, 0] = rng.integers(0, 1 << 24, n).astype(np.float32)
    s["col"][:, 2] = 1.0
    s["col"][:, 3] = TIME - 5
    s["times"][:] = -3.0
    s["times"][:, 0] = TIME - 5
    if remove_every:
        gone = np.arange(n) % remove_every == remove_every - 1
        s["pos"][gone, 3] = 2.0
        s["times"][gone, 0] = TIME - 50  # (more than 20 ticks ago, but inside the time window: outside it the clean keeps everything)
        s["col"][gone, 3] = TIME - 50
    return s


def both_ways(fus, surfels, capacity=None, fuse_plane=False):
    """The same map through the fused entry and through clean + project-only: ((cells, map, count, carried), (cells, map, count))."""
    cap = max(len(surfels), 1) + 64 if capacity is None else capacity
    pose = fus.DevicePose(np.eye(4, dtype=np.float32))
    got = []
    for fused in (True, False):
        gm = fus.GlobalModel(W, H, capacity=cap)
        gm.upload(surfels)
        im = fus.IndexMap(W, H)
        if fuse_plane:  # a wall 2 m ahead that the map does not know: every candidate pixel parks a new measurement
            im.predictIndices(pose, TIME, 0, gm, K, CUT, DELTA)
            rgba = np.full((H, W, 4), 180, np.uint8)
            dm = np.full((H, W), 2.0, np.float32)
            gm.fuse(pose, TIME, 0, rgba, dm, dm, im, K, CUT, 1.0)
        im.predictIndices(pose, TIME, 0, gm, K, CUT, DELTA)
        if fused:
            cells, carried = gm.cleanProject(pose, TIME, 0, im, K, CONF, DELTA, CUT, **PROJ)
        else:
            gm.clean(pose, TIME, 0, im, K, CONF, DELTA, CUT)
            cells, carried = gm.projectOnly(pose, K, CUT, PROJ["projConfThreshold"], PROJ["projTime"], 0, PROJ["projMaxTime"], PROJ["projTimeDelta"]), None
        got.append((cells, gm.downloadMap(), gm.lastCount(), carried))
        gm.close()
    return got


def same_bits(got, what, carried=True):
    (ca, ma, na, took), (cb, mb, nb, _) = got
    assert took == carried, "%s: the scatter %s the projection" % (what, "did not carry" if carried else "carried")
    assert na == nb, "%s: count %d vs %d" % (what, na, nb)
    for f in ma.dtype.names:
        assert ma[f].tobytes() == mb[f].tobytes(), "%s: map plane %s differs" % (what, f)
    assert ca.tobytes() == cb.tobytes(), "%s: %d z-buffer cells differ" % (what, int((ca != cb).sum()))
    return ca, ma


def hit(cells):
    return int((cells != np.uint64(((0xFFFFFF) << 32) | 0xFFFFFFFF)).sum())


def test_removals_in_every_block_shift_every_id(fus):
    s = crafted(fus, 1000, 1, remove_every=7)
    cells, m = same_bits(both_ways(fus, s), "1000 surfels")
    assert len(m) == 1000 - 1000 // 7
    ids = cells[cells != cells.max()] & np.uint64(0xFFFFFFFF)
    assert hit(cells) > 500 and ids.max() < len(m) and len(np.unique(ids)) > 100  # (the winners carry the NEW ids)


@pytest.mark.parametrize("extra", [0, 1])
def test_exactly_full_blocks_and_one_element_more(fus, extra):
    n = 256 * 8 - SLOTS + extra  # map + slots = 256 * 8 (+ 1) elements
    cells, m = same_bits(both_ways(fus, crafted(fus, n, 2 + extra, remove_every=5)), "256 k + %d elements" % extra)
    assert hit(cells) > 1000


def test_offsets_from_the_scan_launch_on_a_large_map(fus):
    """2049 * 256 + 1 elements: more blocks than sum the counts themselves, so the offsets come from the scan launch.  Nearly all
    of the map lies outside the frustum (the blocks that are culled as a whole)."""
    n = 2049 * 256 + 1 - SLOTS
    cells, m = same_bits(both_ways(fus, crafted(fus, n, 4, in_view=0.002, remove_every=11)), "2049 blocks")
    assert len(m) == n - n // 11 and hit(cells) > 500


def test_a_capacity_that_cuts_survivors_off(fus):
    """A full map plus the measurements a fuse parked: the survivors beyond the capacity are neither stored nor projected."""
    s = crafted(fus, 700, 5)
    cells, m = same_bits(both_ways(fus, s, capacity=700 + 300, fuse_plane=True), "capacity")
    assert len(m) == 1000  # (the wall alone parks more than 300 measurements)
    ids = cells[cells != cells.max()] & np.uint64(0xFFFFFFFF)
    assert ids.max() < 1000 and (ids >= 700).any()  # parked measurements were projected too, up to the cut


def test_parked_measurements_are_projected_with_their_new_time(fus):
    """Room for everything: the new points of a fuse carry the -2 marker as their time; the clean stores the tick, and so projects."""
    s = crafted(fus, 700, 6, remove_every=9)
    cells, m = same_bits(both_ways(fus, s, capacity=4000, fuse_plane=True), "parked")
    assert len(m) > 700 and (m["times"][:, 0] == TIME).any()


def test_surfels_that_fail_each_cull_in_turn(fus):
    s = crafted(fus, 600, 7)
    k = np.arange(600) % 8
    s["pos"][k == 1, 2] *= -1.0                # behind the camera
    s["pos"][k == 2, 2] = 30.0                 # beyond the depth cut
    s["pos"][k == 3, 3] = 0.5                  # below the 0.7 threshold (recently seen: the clean keeps it)
    s["times"][k == 4, 0] = 50.0               # outside the time window of the prediction
    s["col"][k == 4, 3] = 50.0
    s["times"][k == 5, 0] = -3.0               # never seen by this sensor
    s["pos"][k == 6, 0] = np.nan               # NaN position
    s["times"][k == 7, 0] = -2.0               # the new-point marker on a map surfel: becomes the tick
    cells, m = same_bits(both_ways(fus, s), "culls")
    assert len(m) == 600 and (m["times"][k == 7, 0] == TIME).all()
    ids = (cells[cells != cells.max()] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert set(np.unique(k[ids])) == {0, 7}, sorted(set(np.unique(k[ids])))  # only the plain surfels and the re-timed ones are drawn


def test_suffix_mode_launches_separately(fus):
    s = crafted(fus, 3000, 8, remove_every=13)
    pose = fus.DevicePose(np.eye(4, dtype=np.float32))
    got = []
    for fused in (True, False):
        gm = fus.GlobalModel(W, H, capacity=4000)
        gm.setCleanSuffixMin(1000)
        gm.upload(s)
        im = fus.IndexMap(W, H)
        im.predictIndices(pose, TIME, 0, gm, K, CUT, DELTA)
        if fused:
            cells, carried = gm.cleanProject(pose, TIME, 0, im, K, CONF, DELTA, CUT, **PROJ)
        else:
            gm.clean(pose, TIME, 0, im, K, CONF, DELTA, CUT)
            cells, carried = gm.projectOnly(pose, K, CUT, 0.7, TIME + 1, 0, TIME + 1, DELTA), None
        got.append((cells, gm.downloadMap(), gm.lastCount(), carried))
        gm.close()
    same_bits(got, "suffix mode", carried=False)


# ------------------------------------------------------------------------------------------
# the frame step, switch 0 against 1
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def frames_of(size, n=N_FRAMES):
    from densemonoslam_amd import synth

    w, h, k = SIZES[size]
    return tuple(synth.frame(i, width=w, height=h, K=k, noise=True) for i in range(n))


def result_bytes(r):
    """pose and every field of the FrameResult a caller receives, as bytes (`surfels` among them: a result block mirrored before
    the new count is in it would show here)"""
    t = r.track
    scal = np.array([r.surfels, r.tick, r.fused, r.fill_in, r.weighting, r.nid_score, r.tracking_ok, r.lost, r.loop_ok, r.loop_constraints,
                     r.loop_icp_error, r.loop_icp_count], np.float64)
    parts = [np.array(r.pose, np.float32), scal, np.array(r.loop_pose, np.float32), np.array(r.loop_cov_diag, np.float64),
             np.array([t.lastICPError, t.lastICPCount, t.lastRGBError, t.lastRGBCount, t.lastSO3Error, t.lastSO3Count], np.float32),
             np.array(t.lastA, np.float64), np.array(t.lastb, np.float64), np.array(t.iterations_run, np.float64)]
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


def small_graph():
    """a deformation graph of near-identity nodes (16 floats each, column-major rotation, sorted by time)"""
    rng = np.random.default_rng(3)
    nn = 24
    nodes = np.zeros((nn, 16), np.float32)
    nodes[:, 0:3] = rng.uniform([-0.8, -0.6, 0.9], [0.8, 0.6, 1.4], (nn, 3))
    nodes[:, 3] = nodes[:, 7] = nodes[:, 11] = 1.0
    nodes[:, 12:15] = rng.normal(0, 0.002, (nn, 3))
    nodes[:, 15] = np.sort(rng.integers(1, 5, nn))
    return nodes


def run(fus, size, switch, ask=(), frames=None, prior_at=None, upload_at=None, arm=False, two_phase=False, graph_at=None, suffix_min=None,
        **opts):
    """One context over the frames: per frame (result bytes, clean / project stats after it, images if asked, frame block, lost, fused),
    then the map."""
    from densemonoslam_amd import capi, collab

    w, h, k = SIZES[size]
    frames = frames_of(size) if frames is None else frames
    g = fus.ElasticFusion(w, h, k, model_capacity=400000, fused_clean_projection=switch, **opts)
    if suffix_min is not None:
        g.globalModel().setCleanSuffixMin(suffix_min)
    blk = None
    if arm:
        T = collab.thumbnail_bytes(w, h)
        blk = capi.DeviceBuffer(T + 128)
        blk.upload(np.full(T + 128, 0xAB, np.uint8))
    per = []
    for i, (d, rgb, _) in enumerate(frames):
        prior = None
        if prior_at == i:
            prior = np.frombuffer(per[-1][0][:64], np.float32).reshape(4, 4).copy()
            prior[:3, 3] += np.float32([0.002, -0.001, 0.001])
        if upload_at == i:
            m = g.globalModel().downloadMap()
            g.globalModel().upload(m[:len(m) - 50])
        if arm:
            g.armFrameBlock(blk.ptr, blk.ptr + T, blk.ptr + T + 64, 100 + i)
        if two_phase or graph_at == i:
            g.processFrameBegin(rgb, d, inPose=prior)
            g.processFrameEnd(graph=small_graph() if graph_at == i else None)
            r = g.fetch()
        else:
            r = g.processFrame(rgb, d, inPose=prior)
        block = blk.download(np.uint8, (T + 128,)).tobytes() if arm else None
        imgs = tuple(g.image(j).copy() for j in PRED_IMAGES) if i in ask else None
        per.append((result_bytes(r), g.cleanProjectStats(), imgs, block, bool(r.lost), bool(r.fused)))
    m = g.globalModel().downloadMap()
    g.close()
    return per, m


def same_results(a, b, what):
    (pa, ma), (pb, mb) = a, b
    assert len(pa) == len(pb)
    for i, (x, y) in enumerate(zip(pa, pb)):
        assert x[0] == y[0], "%s: frame result of frame %d differs" % (what, i)
        assert x[3] == y[3], "%s: frame block of frame %d differs" % (what, i)
        if x[2] is not None:
            for j, u, v in zip(PRED_IMAGES, x[2], y[2]):
                assert u.shape == v.shape and u.tobytes() == v.tobytes(), "%s: image %d after frame %d differs" % (what, j, i)
    assert len(ma) == len(mb), "%s: surfel count %d vs %d" % (what, len(ma), len(mb))
    for f in ma.dtype.names:
        assert ma[f].tobytes() == mb[f].tobytes(), "%s: map field %s differs" % (what, f)


@pytest.mark.parametrize("size", list(SIZES))
def test_frame_step_same_results_and_every_tracked_fusing_frame_fused(fus, size):
    off = run(fus, size, 0)
    on = run(fus, size, 1)
    same_results(on, off, size)
    for i, x in enumerate(on[0]):
        assert x[5], "frame %d did not fuse" % i
        assert x[1] == {"fused": i, "separate": 0}, (i, x[1])  # (the bootstrap frame has no clean)
    for i, x in enumerate(off[0]):
        assert x[1] == {"fused": 0, "separate": i}, (i, x[1])


@pytest.mark.parametrize("size", list(SIZES))
def test_images_asked_for_after_chosen_frames(fus, size):
    """The final prediction's images after frames 2 and 5: the first request renders the skipped prediction from the record the
    fused frame kept, and makes the context eager - the frames after it render their final prediction and launch separately."""
    off = run(fus, size, 0, ask=(2, 5))
    on = run(fus, size, 1, ask=(2, 5))
    same_results(on, off, size)
    stats = [x[1] for x in on[0]]
    assert stats[2] == {"fused": 2, "separate": 0}
    assert stats[-1] == {"fused": 2, "separate": N_FRAMES - 3}, stats[-1]


@pytest.mark.parametrize("case", ["local_loop_closure", "nid_keyframing", "armed_frame_block", "two_phase", "lazy_off"])
def test_ineligible_frames_launch_separately(fus, case):
    opts = {"local_loop_closure": dict(local_loop_closure=1), "nid_keyframing": dict(nid_keyframing=1), "armed_frame_block": dict(arm=True),
            "two_phase": dict(two_phase=True), "lazy_off": dict(lazy_final_prediction=0)}[case]
    off = run(fus, "80x60", 0, **opts)
    on = run(fus, "80x60", 1, **opts)
    same_results(on, off, case)
    assert all(x[1]["fused"] == 0 for x in on[0]), [x[1] for x in on[0]]
    assert on[0][-1][1]["separate"] == sum(1 for x in on[0][1:] if x[5]) > 0


def test_a_frame_with_a_graph_launches_separately(fus):
    """Frame 3 comes through _begin / _end with a deformation graph: its clean applies the graph and runs alone; the one-call
    frames around it take the fused launch."""
    off = run(fus, "97x61", 0, graph_at=3)
    on = run(fus, "97x61", 1, graph_at=3)
    same_results(on, off, "graph")
    assert [x[1]["fused"] for x in on[0]] == [0, 1, 2, 2, 3, 4, 5] and on[0][-1][1]["separate"] == 1


def test_suffix_mode_in_the_frame_step_launches_separately(fus):
    off = run(fus, "97x61", 0, suffix_min=1000)
    on = run(fus, "97x61", 1, suffix_min=1000)
    same_results(on, off, "suffix")
    assert on[0][-1][1] == {"fused": 0, "separate": N_FRAMES - 1}, on[0][-1][1]
    same_results(on, run(fus, "97x61", 1), "suffix against whole-map")  # (and suffix mode itself changes no result)


def test_a_lost_camera(fus):
    """reloc on, garbage then empty depth: the frames fail the error test and the camera is lost.  Untracked frames do not fuse: no
    clean at all; the frames before them took the fused launch.  Same results throughout."""
    from densemonoslam_amd import synth

    size = "320x240"
    w, h, k = SIZES[size]
    rng = np.random.default_rng(5)
    frames = []
    for i in range(16):
        d, rgb, T = synth.frame(i, width=w, height=h, K=k, noise=True)
        if 3 <= i <= 4:
            d = rng.integers(500, 3000, d.shape).astype(np.uint16)
        elif i >= 5:
            d = np.zeros_like(d)
        frames.append((d, rgb, T))
    off = run(fus, size, 0, frames=frames, reloc=1)
    on = run(fus, size, 1, frames=frames, reloc=1)
    same_results(on, off, "lost camera")
    assert on[0][-1][4] and not on[0][5][4]
    want = 0
    for i, x in enumerate(on[0]):
        want += 1 if (i > 0 and x[5]) else 0
        assert x[1] == {"fused": want, "separate": 0}, (i, x[1])
    assert 0 < want < len(frames) - 1


@pytest.mark.parametrize("size", ["97x61", "320x240"])
def test_a_pose_prior_and_a_map_upload_fall_back_to_a_fresh_projection(fus, size):
    """Frame 3 brings a pose prior, the map is replaced between frames 4 and 5: both find the projection the fused clean rendered
    ahead and must not use it.  Same bits on those frames, on the ones after them and in the images asked for at the end."""
    kw = dict(prior_at=3, upload_at=5, ask=(N_FRAMES - 1,))
    off = run(fus, size, 0, **kw)
    on = run(fus, size, 1, **kw)
    same_results(on, off, size)
    assert on[0][-1][1] == {"fused": N_FRAMES - 1, "separate": 0}, on[0][-1][1]
