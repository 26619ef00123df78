"""Maps, draws and take-ins beyond the reference's three time slots.

A surfel carries DMS_MAX_SENSORS = 8 per-camera time slots (the reference: 3, Shaders/Vertex.cpp:49, size.glsl:2) and the map code
treats them unevenly on purpose: dms_model::live_planes (csrc/surfel.hpp) says how many time planes can hold anything but the
"never seen by this sensor" marker -3; the clean reads and moves only those, synthesises -3 for the others and relies on the other
planes of whichever buffer becomes current holding -3 already.  Five writers raise it (fuse, clean, upload, consume, consume-records)
and the health rule loops over a runtime num_sensors that can be smaller or larger.  Here: slots that become live out of order
(5, then 2, then 7), the health rule over mixed slots, maps taken in whose only high slot sits in one record, and window draws whose
time_idx is not 0.

Bar: bit for bit against the CPU oracle (oracle/orc.py) and, for the draws, against the restatements tests/render_ref.py and
tests/render_shaded_ref.py; nothing compares the HIP path with itself.  The draws have no GLSL golden: the reference's programs
have three slots (vTimes[3]), so a draw whose time_idx is above 2, or a map with surfels that only slots above 2 have seen, cannot
be produced with them.

Size: 97 x 61 (no multiple of any tile; tests/test_lazy_prediction_gpu.py), depth cut-off 3.0, confidence threshold 10, weighting
0.75."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_ref as R  # noqa: E402
import render_shaded_ref as S  # noqa: E402

from tests.test_fusion_gpu import assert_bits, surfels_equal  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 97, 61
K = (66.0, 66.0, 48.5, 30.5)
CUT, CONF, WEIGHT, DELTA = 3.0, 10.0, 0.75, 200
SENSORS = 8
INIT = (5, 1)  # (timeIdx, time) of the initialise
SCRIPT = ((2, 2), (7, 3), (5, 4), (2, 5), (0, 17), (7, 29), (3, 41))  # (timeIdx, time) of rounds 1..7: planes go live out of order
BINDING_DELTA, LATER = 10, 12  # a window below the gaps 5 -> 17 -> 29 -> 41 of rounds 5..7, looked through 12 ticks after the round
CAP = 40000


@pytest.fixture(scope="module")
def fus():
    from densemonoslam_amd import capi, fusion

    assert capi.device_count() >= 1, "no MI355X visible"
    return fusion


@pytest.fixture(autouse=True)
def _three_slots_afterwards(orc):
    yield
    orc.set_num_sensors(3)


# ---- the oracle's side, computed once ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def frames():
    """frames 0..7: (rgba, metric depth, filtered metric depth, pose relative to frame 0 in float32)"""
    from densemonoslam_amd import synth
    from oracle import orc

    out, T0 = [], None
    for k in range(8):
        d, rgb, T = synth.frame(k, width=W, height=H, K=K, noise=True)
        T0 = T if T0 is None else T0
        df = orc.depth_bilateral(d, CUT)
        out.append((synth.rgba(rgb), orc.depth_metric(d, CUT), orc.depth_metric(df, CUT), (np.linalg.inv(T0) @ T).astype(np.float32)))
    return tuple(out)


def orc_round(so, rgba, dm, dmf, pose, time, idx):
    """predictIndices -> fuse -> predictIndices -> clean on the oracle (num_sensors as set by the caller)"""
    from oracle import orc

    io = orc.index_map(so, pose, K, H, W, time, idx, CUT, DELTA)
    fused, newU, merged = orc.model_fuse(so, pose, time, idx, rgba, dm, dmf, io[0], io[1], io[3], K, CUT, WEIGHT)
    io2 = orc.index_map(fused, pose, K, H, W, time, idx, CUT, DELTA)
    cleaned = orc.model_clean(fused, newU, pose, time, idx, io2[0], io2[1], io2[2], K, CONF, DELTA, CUT)
    return dict(idx=idx, time=time, pose=pose, io=io, fused=fused, io2=io2, cleaned=cleaned, merged=merged, new=len(newU),
                removed=len(fused) + len(newU) - len(cleaned))


@functools.lru_cache(maxsize=None)
def life():
    """the scripted life of a many-camera map on the oracle: (map after the initialise, the seven rounds)"""
    from oracle import orc

    orc.set_num_sensors(SENSORS)
    try:
        fr = frames()
        so = orc.model_initialise(fr[0][0], fr[0][1], fr[0][2], K, INIT[1], INIT[0], CUT)
        rounds = []
        for r, (idx, time) in enumerate(SCRIPT, start=1):
            rounds.append(orc_round(so, *fr[r], time, idx))
            so = rounds[-1]["cleaned"]
    finally:
        orc.set_num_sensors(3)
    init = orc.model_initialise(fr[0][0], fr[0][1], fr[0][2], K, INIT[1], INIT[0], CUT)
    return init, tuple(rounds)


def gpu_round(fus, gm, im, rgba, dm, dmf, pose, time, idx, want=None, what=""):
    """the same four operators on the GPU; with `want` (an orc_round result) the index image and the map are compared after each"""
    dp = fus.DevicePose(pose)
    im.predictIndices(dp, time, idx, gm, K, CUT, DELTA)
    if want is not None:
        _index_equal(im, want["io"], what + " index map before the fuse")
    gm.fuse(dp, time, idx, rgba, dm, dmf, im, K, CUT, WEIGHT)
    if want is not None:
        surfels_equal(gm.downloadMap(), want["fused"], what + " after fuse")
    im.predictIndices(dp, time, idx, gm, K, CUT, DELTA)
    if want is not None:
        _index_equal(im, want["io2"], what + " index map before the clean")
    gm.clean(dp, time, idx, im, K, CONF, DELTA, CUT)
    if want is not None:
        surfels_equal(gm.downloadMap(), want["cleaned"], what + " after clean")


def _index_equal(im, io, what):
    ig, vg, cg, ng = im.download_index()
    assert (ig == io[0]).all(), "%s: index ids differ at %d pixels" % (what, int((ig != io[0]).sum()))
    assert_bits(vg, io[1], what + " vertConf")
    assert_bits(cg, io[2], what + " colorTime")
    assert_bits(ng, io[3], what + " normRad")


def replay(fus, rounds, suffix_min=None, check=False, extra=None):
    """A GlobalModel taken through the initialise and the first `rounds` rounds of the script."""
    init, rr = life()
    fr = frames()
    gm = fus.GlobalModel(W, H, capacity=CAP)
    gm.setNumSensors(SENSORS)
    if suffix_min is not None:
        gm.setCleanSuffixMin(suffix_min)
    im = fus.IndexMap(W, H)
    gm.initialise(fr[0][0], fr[0][1], fr[0][2], K, INIT[1], INIT[0], CUT)
    if check:
        surfels_equal(gm.downloadMap(), init, "initialise at timeIdx %d" % INIT[0])
    for r in range(1, rounds + 1):
        want = rr[r - 1]
        gpu_round(fus, gm, im, *fr[r], want["time"], want["idx"], want if check else None, "round %d" % r)
        if extra is not None:
            extra(r, gm, im, want)
    return gm, im


# ---- a. the scripted life ---------------------------------------------------------------------------------------------------------
def test_the_script_exercises_merges_and_the_health_rule():
    """On the oracle's own results, so that the script cannot silently stop exercising what it is for: every round merges at least
    500 measurements, rounds 6 and 7 (ticks 29 and 41: slots last stamped more than 20 ticks ago, confidence below the threshold)
    each remove at least 1000 surfels; and the binding time window drops between 10 % and 90 % of the pixel-to-surfel associations
    the wide one makes (the pixel goes to another surfel or to none).

    The window is looked through LATER = 12 ticks after the round: at the round's own tick no timeDelta binds in rounds 5 and 7,
    whose slot then holds nothing but -3 (exempt from the window, index_map / splat_predict) and the tick itself.  And the measure
    counts a pixel that falls to a surfel behind the dropped one: in round 5 the 9552 surfels slot 0 has never seen cover the image
    under every window, so the number of associated pixels hardly moves (5421 -> 5145) while 1039 of them change hands."""
    from oracle import orc

    init, rr = life()
    assert len(init) > 5000 and (init["times"][:, INIT[0]] == INIT[1]).all() and (np.delete(init["times"], INIT[0], 1) == -3).all()
    print("after the initialise: %d surfels" % len(init))
    for r, x in enumerate(rr, start=1):
        print("round %d: timeIdx %d time %d merged %d new %d removed %d -> %d surfels" % (r, x["idx"], x["time"], x["merged"], x["new"],
                                                                                      x["removed"], len(x["cleaned"])))
    for r, x in enumerate(rr, start=1):
        assert x["merged"] >= 500, (r, x["merged"])
    assert rr[5]["removed"] >= 1000 and rr[6]["removed"] >= 1000, (rr[5]["removed"], rr[6]["removed"])
    for r in (5, 6, 7):
        x = rr[r - 1]
        wide = orc.index_map(x["cleaned"], x["pose"], K, H, W, x["time"] + LATER, x["idx"], CUT, DELTA)[0]
        tight = orc.index_map(x["cleaned"], x["pose"], K, H, W, x["time"] + LATER, x["idx"], CUT, BINDING_DELTA)[0]
        dropped = int(((wide > 0) & (tight != wide)).sum())
        print("round %d, tick %d: timeDelta %d associates %d pixels, timeDelta %d drops %d of these associations (%d pixels keep none)"
              % (r, x["time"] + LATER, DELTA, (wide > 0).sum(), BINDING_DELTA, dropped, ((wide > 0) & (tight == 0)).sum()))
        assert (wide > 0).sum() > 1000 and 0.1 <= dropped / (wide > 0).sum() <= 0.9, (r, (wide > 0).sum(), dropped)


def _predictions_at_the_rounds_slot(fus):
    from oracle import orc

    def extra(r, gm, im, x):
        if r < 5:
            return
        so, pose, time, idx = x["cleaned"], x["pose"], x["time"] + LATER, x["idx"]
        dp = fus.DevicePose(pose)
        what = "round %d (timeIdx %d, tick %d, timeDelta %d)" % (r, idx, time, BINDING_DELTA)
        im.predictIndices(dp, time, idx, gm, K, CUT, BINDING_DELTA)
        _index_equal(im, orc.index_map(so, pose, K, H, W, time, idx, CUT, BINDING_DELTA), what + " index map")
        # the active view drops what this sensor has never seen (times[timeIdx] == -3) and what fell out of the window: under the
        # binding window that is everything, so it takes the wide one; the inactive view and the synthesised depth take the binding one
        for active, conf, delta in ((True, 0.0, DELTA), (True, 2.0, DELTA), (False, 0.0, BINDING_DELTA)):
            tgt = im.combinedPredict(dp, gm, K, CUT, conf, time, idx, time, delta, active)
            ig, vg, ng, tg = tgt.download()
            io, vo, no, to = orc.splat_predict(so, pose, K, H, W, CUT, conf, time, idx, time, delta, active)
            assert (vo[..., 2] > 0).sum() > 100, what + ": the prediction is empty"
            assert_bits(vg, vo, what + " pred vertex")
            assert_bits(ng, no, what + " pred normal")
            assert_bits(ig, io, what + " pred image")
            assert_bits(tg, to, what + " pred time")
        dg = im.synthesizeDepth(dp, gm, K, CUT, 0.0, time, idx, time, BINDING_DELTA).download()
        do = orc.splat_predict(so, pose, K, H, W, CUT, 0.0, time, idx, time, BINDING_DELTA, False, depth_only=True)
        assert (do > 0).sum() > 100
        assert_bits(dg, do, what + " synth depth")

    return extra


@pytest.mark.parametrize("suffix_min", [None, 0], ids=["default_clean", "suffix_clean"])
def test_scripted_life_of_a_many_camera_map(fus, suffix_min):
    """initialise at timeIdx 5, then seven rounds of predictIndices -> fuse -> predictIndices -> clean at timeIdx 2, 7, 5, 2, 0, 7, 3
    (ticks 2, 3, 4, 5, 17, 29, 41) with num_sensors = 8 on both sides: index image and map equal the oracle's after every operator.
    Once as is, once with every clean on the suffix path (k_clean_scatter_suffix + k_clean_copy_back over 22 - 47 scan chunks).  At
    rounds 5 - 7 the index map, both predictions and the synthesised depth at the round's slot under a time window that binds: a
    kernel that reads another plane changes the image."""
    gm, _ = replay(fus, len(SCRIPT), suffix_min, check=True, extra=_predictions_at_the_rounds_slot(fus))
    gm.close()


# ---- b. the health rule over 3, 4, 5 and 8 slots ------------------------------------------------------------------------------------
N_HEALTH = 4096 + 77  # whole scan chunks (256) and a ragged tail


@functools.lru_cache(maxsize=None)
def health_map(time, low_top):
    """All surfels behind the camera (identity pose: no window test applies); confidence 1 for 70 %, 12 for the rest; every slot drawn
    independently from {-3, -1, time - 2, time - 25}.  low_top: slots 5..7 all -3 (the map then has five live planes)."""
    from oracle import orc

    rng = np.random.default_rng(11)
    n = N_HEALTH
    vals = np.array([-3.0, -1.0, time - 2.0, time - 25.0], np.float32)
    so = np.zeros(n, orc.SURFEL_DTYPE)
    so["times"] = vals[rng.choice(4, size=(n, orc.MAX_SENSORS), p=(0.08, 0.62, 0.10, 0.20))]
    so["pos"][:, 3] = np.where(rng.random(n) < 0.7, 1.0, 12.0)
    so["pos"][:, 0:2] = rng.uniform(-1.0, 1.0, (n, 2))
    so["pos"][:, 2] = rng.uniform(-2.0, -1.0, n)
    nr = rng.normal(0.0, 1.0, (n, 3))
    so["nrm"][:, :3] = nr / np.linalg.norm(nr, axis=1, keepdims=True)
    so["nrm"][:, 3] = 0.02
    so["col"] = np.float32([(100 << 16) + (100 << 8) + 100, 0, 1, 1])
    if low_top:
        so["times"][:, 5:] = -3.0
    return so


def health_rule_keeps(so, time, time_idx, sensors):
    """copy_unstable.vert:137-150 in float32, for surfels no window test applies to: removed when EVERY one of the first `sensors`
    slots is unhealthy (-1, or older than 20 ticks at a confidence below the threshold), unless this sensor's own time is too old."""
    t, own = so["times"][:, :sensors], so["times"][:, time_idx]
    unhealthy = (t == np.float32(-1)) | (((np.float32(time) - t) > np.float32(20)) & (so["pos"][:, 3:4] < np.float32(CONF)))
    return ~unhealthy.all(1) | ((own > 0) & ((np.float32(time) - own) > np.float32(DELTA)))


HEALTH_CASES = [(t, ns, ti) for t in (5, 30) for ns in (3, 4, 5, 8) for ti in (0, 4, 7) if ti < ns]


@pytest.mark.parametrize("time,sensors,time_idx", HEALTH_CASES)
def test_health_rule_over_mixed_slots(fus, orc, time, sensors, time_idx):
    """The clean's health rule with num_sensors below the number of live planes (3, 4, 5 of 8: the slots that take no part must still
    be moved intact) and above it (8 over a map whose slots 5..7 are all -3: the planes the clean does not read count as -3).
    Survivors from the oracle and from the numpy restatement of the shader rule: the two agree, and the GPU map equals them in
    content and order, on the default path and with the clean forced onto the suffix path."""
    assert len(HEALTH_CASES) == 14
    pose = np.eye(4, dtype=np.float32)
    for low_top in ((False, True) if sensors > 5 else (False,)):
        so = health_map(time, low_top)
        io = orc.index_map(so, pose, K, H, W, time, time_idx, CUT, DELTA)
        assert io[0].max() == 0  # behind the camera
        orc.set_num_sensors(sensors)
        try:
            want = orc.model_clean(so, so[:0], pose, time, time_idx, io[0], io[1], io[2], K, CONF, DELTA, CUT)
        finally:
            orc.set_num_sensors(3)
        surfels_equal(want, so[health_rule_keeps(so, time, time_idx, sensors)], "oracle against the shader rule")
        print("time %d, %d slots, timeIdx %d, slots 5..7 %s: %d of %d kept" % (time, sensors, time_idx, "-3" if low_top else "mixed",
                                                                              len(want), len(so)))
        if low_top and time == 5:  # at tick 5 a slot that holds -3 is healthy (8 ticks): the three unread planes keep every surfel
            assert len(want) == len(so)
        else:
            assert 0.1 <= len(want) / len(so) <= 0.9, (len(want), len(so))
        for suffix_min in (None, 0):
            gm = fus.GlobalModel(W, H, capacity=CAP)
            gm.setNumSensors(sensors)
            if suffix_min is not None:
                gm.setCleanSuffixMin(suffix_min)
            gm.upload(so)
            im = fus.IndexMap(W, H)
            dp = fus.DevicePose(pose)
            im.predictIndices(dp, time, time_idx, gm, K, CUT, DELTA)
            gm.clean(dp, time, time_idx, im, K, CONF, DELTA, CUT)
            surfels_equal(gm.downloadMap(), want, "GPU, %d slots, timeIdx %d, low_top %s, suffix_min %s" % (sensors, time_idx, low_top, suffix_min))
            gm.close()


# ---- c. taking maps in ------------------------------------------------------------------------------------------------------------
def _transform():
    ang = 0.3
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]], np.float32)
    T[:3, 3] = (0.4, -0.1, 0.25)
    return T


def small_map():
    """the other map: one initialise at timeIdx 0 (frame 3 of the stream)"""
    from oracle import orc

    fr = frames()
    return orc.model_initialise(fr[3][0], fr[3][1], fr[3][2], K, 1, 0, CUT)


def _blank_round_time():
    return SCRIPT[1][1] + 1


@functools.lru_cache(maxsize=None)
def taken_in(direction):
    """oracle: (map after the take-in, map after one more round at timeIdx 0 with a blank depth frame)"""
    from oracle import orc

    big, small = life()[1][1]["cleaned"], small_map()
    dst, src = {"many_takes_one": (big, small), "one_takes_many": (small, big), "empty_takes_many": (big[:0], big),
                "empty_takes_one": (small[:0], small)}[direction]
    merged = orc.model_consume(dst, src, _transform())
    return merged, _orc_blank_round(merged, _blank_round_time())


def _orc_blank_round(so, time, sensors=SENSORS):
    from oracle import orc

    rgba = frames()[0][0]
    blank = np.zeros((H, W), np.float32)
    orc.set_num_sensors(sensors)
    try:
        x = orc_round(so, rgba, blank, blank, np.eye(4, dtype=np.float32), time, 0)
    finally:
        orc.set_num_sensors(3)
    assert x["merged"] == 0 and x["new"] == 0
    return x["cleaned"]


def _gpu_blank_round(fus, gm, time):
    blank = np.zeros((H, W), np.float32)
    gpu_round(fus, gm, fus.IndexMap(W, H), frames()[0][0], blank, blank, np.eye(4, dtype=np.float32), time, 0)


def _gpu_small(fus):
    fr = frames()
    gm = fus.GlobalModel(W, H, capacity=CAP)
    gm.setNumSensors(SENSORS)
    gm.initialise(fr[3][0], fr[3][1], fr[3][2], K, 1, 0, CUT)
    return gm


TAKE_INS = [("many_takes_one", "model"), ("many_takes_one", "records"), ("one_takes_many", "model"), ("one_takes_many", "records"),
            ("empty_takes_many", "records"), ("empty_takes_one", "records")]


@pytest.mark.parametrize("direction,source", TAKE_INS)
def test_taking_a_map_in_keeps_every_live_slot(fus, direction, source):
    """A map with slots 5, 2 and 7 live (the script up to round 2) and a map from one initialise at timeIdx 0, taken in either
    direction: model to model, through exportRecords / consumeRecords, and by consumeRecords into a map whose count is 0.  Equal to
    orc.model_consume; then one round at timeIdx 0 with a blank depth frame (nothing fuses) and equal again - a consuming map whose
    live_planes came out too low shows only there, where the high slots would read -3."""
    want, want_cleaned = taken_in(direction)
    big, _ = replay(fus, 2)
    small = _gpu_small(fus)
    if direction.startswith("empty"):
        dst = fus.GlobalModel(W, H, capacity=CAP)
        dst.setNumSensors(SENSORS)
        src = big if direction == "empty_takes_many" else small
    else:
        dst, src = (big, small) if direction == "many_takes_one" else (small, big)
    before = src.downloadMap()
    if source == "model":
        dst.consume(src, _transform())
    else:
        rec, n = src.exportRecords()
        assert n == len(before)
        assert_bits(rec.download(np.float32, (n, 20)), before.view(np.float32).reshape(n, 20), "exported records")
        dst.consumeRecords(rec.ptr, n, _transform())
    surfels_equal(dst.downloadMap(), want, "%s through %s" % (direction, source))
    surfels_equal(src.downloadMap(), before, "the map taken in is left as it was")
    live = [s for s in range(SENSORS) if (want["times"][:, s] != -3).any()]
    assert live == {"many_takes_one": [0, 2, 5, 7], "one_takes_many": [0, 2, 5, 7], "empty_takes_many": [2, 5, 7], "empty_takes_one": [0]}[direction], live
    _gpu_blank_round(fus, dst, _blank_round_time())
    surfels_equal(dst.downloadMap(), want_cleaned, "%s through %s, after the next clean" % (direction, source))
    assert len(want_cleaned) > 0.5 * len(want)
    for m in {id(big): big, id(small): small, id(dst): dst}.values():
        m.close()


N_LONE = 70001
LONE_TIME = 30


@functools.lru_cache(maxsize=None)
def lone_records(slot, where):
    """70 001 records behind the camera at a confidence below the threshold; slot 0 holds -1 (unhealthy) or 28 (healthy) in turn, every
    other slot -3 (older than 20 ticks at tick 30: unhealthy) - except in ONE record, first or last, whose slot 0 is -1 and whose slot
    `slot` holds 28: with eight slots counted it survives the clean only if that slot is read."""
    from oracle import orc

    base = health_map(LONE_TIME, False)
    so = np.tile(base, N_LONE // len(base) + 1)[:N_LONE].copy()
    so["pos"][:, 3] = 1.0
    so["times"][:] = -3.0
    so["times"][:, 0] = np.where(np.arange(N_LONE) % 2 == 0, -1.0, LONE_TIME - 2.0)
    i = 0 if where == "first" else N_LONE - 1
    so["times"][i, 0] = -1.0
    so["times"][i, slot] = LONE_TIME - 2.0
    so["pos"][i, :3] = (0.125, -0.25, -1.5)
    want = _orc_blank_round(so, LONE_TIME)
    lone = (want["pos"][:, :3] == so["pos"][i, :3]).all(1)
    assert lone.sum() == 1 and want["times"][lone, slot] == LONE_TIME - 2.0, "the oracle must keep the lone record for its high slot"
    assert 0.4 * N_LONE < len(want) < 0.6 * N_LONE
    return so, want


@pytest.mark.parametrize("where", ["last", "first"])
@pytest.mark.parametrize("slot", [7, 6])
@pytest.mark.parametrize("source", ["upload", "records"])
def test_one_record_with_a_high_slot_makes_its_plane_live(fus, slot, where, source):
    """Exactly one of 70 001 records carries anything but -3 above slot 0 - in slot 7 or 6, as the last record or the first, so in
    another block than most: dms_model_upload (host scan) and dms_model_consume_records into an empty map (k_records_live_planes)
    must both find it.  After the next clean the record is there with its slot intact, as on the oracle."""
    so, want = lone_records(slot, where)
    gm = fus.GlobalModel(W, H, capacity=N_LONE + 4096)
    gm.setNumSensors(SENSORS)
    gm.upload(so)
    if source == "records":
        rec, n = gm.exportRecords()
        assert n == N_LONE
        dst = fus.GlobalModel(W, H, capacity=N_LONE + 4096)
        dst.setNumSensors(SENSORS)
        dst.consumeRecords(rec.ptr, n, np.eye(4, dtype=np.float32))
        gm.close()
        gm = dst
    surfels_equal(gm.downloadMap(), so, "taken in")
    _gpu_blank_round(fus, gm, LONE_TIME)
    surfels_equal(gm.downloadMap(), want, "slot %d in the %s record through %s, after the clean" % (slot, where, source))
    gm.close()


def test_reference_layout_download_of_an_eight_slot_map(fus):
    """dms_model_download_ref of a map with slots 0, 2, 3, 5 and 7 live: the reference's 15-float records keep slots 0..2 only
    (oracle/orc_export.ref_records)."""
    from oracle import orc_export

    gm, _ = replay(fus, len(SCRIPT))
    want = life()[1][-1]["cleaned"]
    assert all((want["times"][:, s] > 0).any() for s in (0, 2, 3, 5, 7))
    assert_bits(gm.downloadMapRef(), orc_export.ref_records(want), "reference-layout records")
    gm.close()


# ---- d. draws -----------------------------------------------------------------------------------------------------------------------
VW, VH = 160, 120


@pytest.fixture(scope="module")
def final_map(fus):
    gm, _ = replay(fus, len(SCRIPT))
    recs = gm.downloadMap()
    surfels_equal(recs, life()[1][-1]["cleaned"], "final map of the script")
    yield gm, recs
    gm.close()


def _view(w=VW, h=VH):
    from densemonoslam_amd import fusion

    f = K[0] * w / W
    proj = fusion.render_frustum(w, h, f, f, w / 2.0, h / 2.0, 0.1, 1000.0)
    pose = frames()[7][3]
    return R.mvp_from_pose(proj, pose), R.mvp_from_pose(np.eye(4, dtype=np.float32), pose)


def _winner_outcomes(key, recs, time, time_idx, time_delta):
    ids = (key[key != R.CLEARED] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    dt = np.float32(time) - recs["times"][ids, time_idx]
    return int((dt > time_delta).sum()), int((dt < time_delta).sum()), int((dt == time_delta).sum())


# (time, time_delta) per slot, from the stamps the script leaves there.  Slot 2: ticks 2 and 5, slot 7: ticks 3 and 29 - the older
# stamp on the boundary (dt == time_delta), the newer inside, the slot's -3 outside.  Slot 3 holds one stamp only (tick 41): a draw
# sees two values of dt, so the three outcomes need two windows - the stamp on the boundary in one, inside in the other.
WINDOWS = {2: [(7, 5)], 3: [(44, 3), (50, 10)], 7: [(32, 29)]}


@pytest.mark.parametrize("time_idx", [2, 3, 7])
@pytest.mark.parametrize("points", [False, True], ids=["discs", "points"])
def test_window_draw_at_a_high_slot(fus, final_map, time_idx, points):
    """RenderTarget.draw with draw_window at time_idx 2, 3 and 7 against render_ref, which indexes times[:, time_idx].  Over the two
    windows of a slot all three outcomes occur among the winners of the restatement: darkened (dt > time_delta), green
    (dt < time_delta) and untouched (dt == time_delta).  (The point program has no window: its draws must ignore the slot.)"""
    gm, recs = final_map
    mvp, _ = _view()
    seen = np.zeros(3, np.int64)
    for time, delta in WINDOWS[time_idx]:
        for ct in (2, 0):
            p = dict(color_type=ct, draw_window=True, time=time, time_idx=time_idx, time_delta=delta, draw_unstable=True, draw_points=points)
            t = fus.RenderTarget(VW, VH)
            t.clear((0.1, 0.2, 0.3, 1.0))
            t.draw(gm, mvp, **p)
            got = t.images()
            t.close()
            ref = R.Target(VW, VH, (0.1, 0.2, 0.3, 1.0))
            ref.draw(recs, mvp, **p)
            exp = ref.images()
            for name, a, b in zip(("colour", "depth24", "winner"), got, exp):
                assert np.array_equal(a, b), "%s differs at %d places (slot %d, time %d, delta %d)" % (name, int((a != b).sum()), time_idx, time, delta)
            # the slot matters: the restatement itself gives another image for plane 0
            if not points:
                other = R.Target(VW, VH, (0.1, 0.2, 0.3, 1.0))
                other.draw(recs, mvp, **dict(p, time_idx=0))
                assert not np.array_equal(other.images()[0], exp[0])
        seen += _winner_outcomes(exp[2], recs, time, time_idx, delta)
    print("slot %d: winners outside / inside / on the boundary: %s" % (time_idx, seen.tolist()))
    assert points or (seen > 0).all(), seen.tolist()


@pytest.mark.parametrize("time_idx", [2, 3, 7])
def test_shaded_window_draw_at_a_high_slot(fus, final_map, time_idx):
    """ShadedView.draw + fxaa and ShadedView.drawFXAA with drawWindow at time_idx 2, 3 and 7 against render_shaded_ref."""
    gm, recs = final_map
    sw, sh = 240, 180
    mvp, mv = _view(sw, sh)
    seen = np.zeros(3, np.int64)
    for time, delta in WINDOWS[time_idx]:
        p = dict(color_type=2, draw_window=True, time=time, time_idx=time_idx, time_delta=delta, draw_unstable=True, sign_mult=-1.0,
                 clear_rgba=(0.05, 0.05, 0.3, 0.0), light_pos=mv[:3, 3])
        v = fus.ShadedView(VW, VH, offscreen=(sw, sh))
        v.clear((0.1, 0.2, 0.3, 1.0))
        v.draw(gm, mvp, **p)
        v.fxaa()
        off, img = v.offscreen_images(), v.images()
        ref_off = S.Offscreen(sw, sh)
        ref_off.draw(recs, mvp, **p)
        ref = R.Target(VW, VH, (0.1, 0.2, 0.3, 1.0))
        S.composite(ref, ref_off)
        _same_images(off, ref_off.images(), "offscreen (slot %d, time %d, delta %d)" % (time_idx, time, delta))
        _same_images(img, ref.images(), "view (slot %d, time %d, delta %d)" % (time_idx, time, delta))
        seen += _winner_outcomes(ref_off.images()[2], recs, time, time_idx, delta)
        # the GUI's call
        v.clear((0, 0, 0, 1))
        v.drawFXAA(mvp, mv, gm, 2.0, time, time_idx, delta, True, drawColors=True, drawUnstable=True, drawWindow=True)
        got = v.images()
        v.close()
        t = R.Target(VW, VH, (0, 0, 0, 1))
        S.drawFXAA(t, S.Offscreen(sw, sh), recs, mvp, mv, 2.0, time, time_idx, delta, True, drawColors=True, drawUnstable=True, drawWindow=True)
        _same_images(got, t.images(), "drawFXAA (slot %d, time %d, delta %d)" % (time_idx, time, delta))
    assert (seen > 0).all(), seen.tolist()


def _same_images(got, exp, what):
    for a, b in zip(got, exp):
        assert a.shape == b.shape and a.dtype == b.dtype, what
        same = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b)) if a.dtype == np.float32 else a == b
        assert same.all(), "%s: %d differing values" % (what, int((~same).sum()))


def test_contribution_colours_of_surfels_no_reference_slot_has_seen(fus, final_map):
    """color_type 4 ("by contribution", draw_global_surface.geom:123-145) sums over the reference's three slots.  A surfel only slots
    above 2 have seen has none of them: total = 0, the colour is 0 / 0 * s + 0.1 = NaN in every channel, and a channel that is not
    finite is written as 0 (R9, the isfinite test of unorm8 - no NaN reaches a float-to-integer conversion).  Pinned here: such a
    surfel is drawn black with alpha 255, by the kernel and by the restatement; with the window on it stays black (NaN * 0.25, NaN * 0)."""
    gm, recs = final_map
    mvp, _ = _view()
    unseen = (recs["times"][:, :3] == -3).all(1)
    assert unseen.any() and (~unseen).any()
    for window in (False, True):
        p = dict(color_type=4, draw_unstable=True, time=44, time_idx=3, time_delta=3, draw_window=window)
        t = fus.RenderTarget(VW, VH)
        t.clear((0.1, 0.2, 0.3, 1.0))
        t.draw(gm, mvp, **p)
        got = t.images()
        t.close()
        ref = R.Target(VW, VH, (0.1, 0.2, 0.3, 1.0))
        ref.draw(recs, mvp, **p)
        exp = ref.images()
        for name, a, b in zip(("colour", "depth24", "winner"), got, exp):
            assert np.array_equal(a, b), "%s differs at %d places" % (name, int((a != b).sum()))
        key = exp[2]
        won = key != R.CLEARED
        ids = (key[won] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        px = got[0][won]
        assert unseen[ids].sum() > 20 and (~unseen[ids]).sum() > 20, "both kinds of surfel must win pixels"
        assert (px[unseen[ids]] == np.array([0, 0, 0, 255], np.uint8)).all()
        if not window:
            assert (px[~unseen[ids]][:, :3].max(1) >= 26).all()  # the 0.1 base colour at least
