"""The collaborative session past the merge (densemonoslam_amd/session.py) over gloo, world size 2, without a GPU:
publish -> match -> verify -> merge across ranks (surfel records, key-frame records, camera state point to point) -> more frames
with both cameras fusing into ONE map on the consuming rank, the consumed rank forwarding its camera's frames.

The engines are stand-ins with the product's call surface built on the oracle, so what is under test is the PROTOCOL: who sends what
to whom, the decision rule, the re-basing of poses / pose graphs / relative constraints.  The checker is oracle/orc_pipeline.Session,
the same session played in one process the way the reference runs its cameras (MainController.cpp:262-400): merged map, both
trajectories and the merge transform must be the same bits."""
import multiprocessing as mp
import os
import socket

import numpy as np
import pytest

W, H = 320, 240
K = (264.0, 264.0, 160.0, 120.0)


class Scenario:
    def __init__(self, name, scene, offset, query_from, n_ticks, fern_photo, **session_opts):
        self.name, self.scene, self.offset, self.query_from, self.n_ticks, self.fern_photo = name, scene, offset, query_from, n_ticks, fern_photo
        self.opts = dict(query_from=query_from, **session_opts)

    def frames(self, synth, k):
        """camera 1 runs `offset` frames ahead of camera 0 on the same trajectory"""
        sc = getattr(synth, self.scene) if self.scene else None
        out = {}
        for c, off in ((0, 0), (1, self.offset)):
            d, rgb, _ = synth.frame(k + off, width=W, height=H, K=K, noise=True, scene=sc)
            out[c] = (rgb, d)
        return out


# "reference_rule": the merge is triggered by the reference's OWN rule - Ferns::findFrame with interMap = 1 (Ferns.cpp:277-423: SO3 +
# 3 x 50 point-to-plane iterations on the 40 x 30 thumbnails, photometric check at Options' 115) followed by the full-resolution
# refinement and acceptance of ReferenceFrame.h:72-110 at Options' default thresholds - in the cluttered-corner scene, whose geometry
# constrains point-to-plane ICP down to the coarsest thumbnail level (synth.CORNER_SCENE).
# "thumbnail_only" (rounds 3-4, kept as an extra): inter_map = 2 has no reference counterpart (dmslam_ferns.h) and no refinement; in
# the default box room the reference's rule never verifies (the thumbnail ICP slides along the walls and diverges).
SCENARIOS = {
    "reference_rule": Scenario("reference_rule", "CORNER_SCENE", 8, 6, 15, 115.0, inter_map=1, full_refine=True),
    "thumbnail_only": Scenario("thumbnail_only", None, 14, 4, 14, 1000.0, inter_map=2, full_refine=False),
}
# (the colour check rejects ICP-only poses in the default room: tests/test_ferns_gpu.py - hence 1000 there)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


# ---- oracle-backed stand-ins with the call surface of session.GpuBackend's engines ---------------------------------------------------
class _OrcCamera:
    def __init__(self, be, c):
        from oracle import orc_pipeline

        self.be, self.c = be, c
        self.ef = orc_pipeline.ElasticFusion(W, H, K, timeIdx=c)

    def processFrame(self, rgb, depth):
        return self.ef.processFrame(rgb, depth)

    def tick(self):
        return self.ef.tick

    def pose(self):
        return self.ef.currPose

    def lost(self):
        return bool(self.ef.lost)

    def fillTextures(self):
        fi, fv, fn = self.ef.fill
        return np.ascontiguousarray(fi), np.ascontiguousarray(fv), np.ascontiguousarray(fn)

    def thumbnails(self):
        from oracle import orc_ferns

        fi, fv, fn = self.ef.fill
        th, tw = H // 8, W // 8
        parts = [orc_ferns.resize_nearest(fi, th, tw), orc_ferns.resize_nearest(fv, th, tw), orc_ferns.resize_nearest(fn, th, tw)]
        return np.concatenate([np.ascontiguousarray(p).view(np.uint8).reshape(-1) for p in parts])

    def joinMap(self, owner, T):
        from oracle import orc, orc_ferns

        if self.ef.map is not owner.ef.map and len(self.ef.map.model) and self.c == self.be.session.frame_of[self.c]:
            owner.ef.map.model = orc.model_consume(owner.ef.map.model, self.ef.map.model, T)
        self.ef.map = owner.ef.map
        self.ef.currPose = orc_ferns._mul44(T, self.ef.currPose)

    def exportMap(self):
        return np.ascontiguousarray(self.ef.model).view(np.float32).reshape(-1, 20)

    def consumeRecords(self, rec, T):
        from oracle import orc

        if len(rec):
            src = np.ascontiguousarray(rec, np.float32).reshape(-1).view(orc.SURFEL_DTYPE)
            self.ef.map.model = orc.model_consume(self.ef.map.model, src, T)

    def importCamera(self, owner, pose, tick, rgb, depth):
        from densemonoslam_amd import synth

        self.ef.map = owner.ef.map
        self.ef.currPose = np.asarray(pose, np.float32).reshape(4, 4).copy()
        self.ef.tick = int(tick)
        self.ef.initialised = True
        # the state the camera's last frame left in its tracker: the intensity pyramid the next SO3 pre-alignment reads
        self.ef.frameToModel.initFirstRGB(synth.rgba(np.asarray(rgb)))

    def model(self):
        return self.ef.model

    def close(self):
        pass


class _OrcRefiner:
    """ReferenceFrame's m_rgbd behind the session's call surface (oracle/orc_pipeline.refine_inter_map)"""

    def __init__(self):
        from oracle import orc

        self.o = orc.Odometry(W, H, K[2], K[3], K[0], K[1])

    def refineLocal(self, owner, cam, recoveryPose, thresholds):
        return self.refineRemote(owner, cam.ef.fill, cam.c, cam.tick(), cam.pose(), recoveryPose, thresholds)

    def refineRemote(self, owner, textures, timeIdx, tick, currPose, recoveryPose, thresholds):
        from oracle import orc_pipeline

        r = orc_pipeline.refine_inter_map(owner.ef, self.o, textures, timeIdx, tick, currPose, recoveryPose, *thresholds)
        return r["accepted"], r["relativeTransform"]

    def close(self):
        pass


class _OrcFerns:
    def __init__(self, fern_photo):
        from oracle import orc, orc_ferns

        self.db = orc_ferns.Ferns(W, H, K, num=500, maxDepth_mm=3000, photoThresh=fern_photo, seed=20260929,
                                  make_odometry=lambda: orc.Odometry(W // 8, H // 8, K[2] / 8, K[3] / 8, K[0] / 8, K[1] / 8))
        self.th, self.tw = H // 8, W // 8

    def _unpack(self, blk):
        n = self.th * self.tw
        raw = np.ascontiguousarray(blk, np.uint8)
        return (raw[:n * 4].reshape(self.th, self.tw, 4).copy(), raw[n * 4:n * 20].view(np.float32).reshape(self.th, self.tw, 4).copy(),
                raw[n * 20:n * 36].view(np.float32).reshape(self.th, self.tw, 4).copy())

    def addBlock(self, blk, pose, tick, thr):
        img, v, n = self._unpack(blk)
        self.db._add(img, v, n, np.asarray(pose, np.float32).reshape(4, 4).copy(), int(tick), thr)

    def findFrameThumbs(self, blk, pose, tick, inter_map=1):
        m = self.db.findFrame(np.asarray(pose, np.float32).reshape(4, 4), None, None, None, int(tick), lost=False, interMap=inter_map,
                              thumbs=self._unpack(blk))
        return m["closest"], m["candidate"], m["estPose"]

    def searchHit(self, blk):
        return self.db.searchHit(self._unpack(blk), 0, interMap=True)

    def consume(self, other, T, thr):
        self.db.consume(other.db, T, thr)

    def exportRecords(self):
        n = self.th * self.tw
        recs = []
        for fr in self.db.frames:
            meta = np.zeros(20, np.float32)
            meta[:16] = fr.pose.reshape(16)
            meta[16:17] = np.array([fr.srcTime], np.int32).view(np.float32)
            recs.append(np.concatenate([np.ascontiguousarray(fr.initRgb).view(np.uint8).reshape(-1), np.ascontiguousarray(fr.initVerts).view(np.uint8).reshape(-1),
                                        np.ascontiguousarray(fr.initNorms).view(np.uint8).reshape(-1), meta.view(np.uint8)]))
            assert len(recs[-1]) == n * 36 + 80
        return np.concatenate(recs) if recs else np.zeros(0, np.uint8)

    def consumeRecords(self, raw, T, thr):
        from oracle import orc_ferns

        rb = self.th * self.tw * 36 + 80
        for j in range(len(raw) // rb):
            rec = np.ascontiguousarray(raw[j * rb:(j + 1) * rb])
            img, v, n = self._unpack(rec[:rb - 80])
            meta = rec[rb - 80:].view(np.float32)
            self.db._add(img, v, n, orc_ferns._mul44(T, meta[:16].reshape(4, 4)), int(meta[16:17].view(np.int32)[0]), thr)

    def __len__(self):
        return len(self.db.frames)

    def close(self):
        pass


class _OrcBackend:
    session = None

    def __init__(self, fern_photo):
        self.fern_photo = fern_photo

    def make_refiner(self):
        return _OrcRefiner()

    def block_bytes(self):
        return (W // 8) * (H // 8) * 36

    def make_camera(self, c):
        return _OrcCamera(self, c)

    def make_ferns(self):
        return _OrcFerns(self.fern_photo)

    def relative_transform(self, recoveryPose, currPose):
        from oracle import orc, orc_ferns

        return orc_ferns._mul44(recoveryPose, orc.inv4f(currPose))

    def pose_compose(self, a, b):
        from oracle import orc_ferns

        return orc_ferns._mul44(a, b)

    def transform_point(self, T, p):
        from oracle import orc_ferns

        return orc_ferns._mul4v(T, np.append(np.asarray(p, np.float32), np.float32(1)))[:3]


def frames_at(synth, k, offsets):
    """camera c runs offsets[c] frames ahead of camera 0 on the corner scene's trajectory"""
    out = {}
    for c, off in enumerate(offsets):
        d, rgb, _ = synth.frame(k + off, width=W, height=H, K=K, noise=True, scene=synth.CORNER_SCENE)
        out[c] = (rgb, d)
    return out


def _worker(rank, world, port, q, scenario, extra=None, offsets=None, ticks=None):
    sc = SCENARIOS[scenario]
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    threads = "4" if world <= 2 else "2"
    os.environ["OMP_NUM_THREADS"] = threads
    import torch.distributed as dist

    from densemonoslam_amd import session, synth
    from oracle import orc

    orc.set_threads(int(threads))
    n = len(offsets) if offsets else 2
    orc.set_num_sensors(max(3, n))  # (the stand-in cameras: the oracle's count is a global of this process)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    be = _OrcBackend(sc.fern_photo)
    s = session.CollabSession(be, n, W, H, rank=rank, world=world, **sc.opts, **(extra or {}))
    be.session = s
    for c in s.hosted():  # a constraint row the caller's solver produced before the merge
        s.relative_cons[c].append(np.arange(6, dtype=np.float32) * np.float32(0.25 + c))
    hosted_log = []
    for k in range(ticks or sc.n_ticks):
        fr = frames_at(synth, k, offsets) if offsets else sc.frames(synth, k)
        s.step(k, {c: fr[c] for c in fr if c % world == rank})
        hosted_log.append(s.hosted())
    res = dict(rank=rank, hosted=hosted_log, merges=s.merges, frame_of=s.frame_of, refinements=s.refinements,
               pose_graph={c: s.pose_graph[c] for c in s.hosted()}, relative_cons={c: s.relative_cons[c] for c in s.hosted()},
               maps={f: np.ascontiguousarray(s.cams[next(c for c in s.hosted() if s.frame_of[c] == f)].model()) for f in sorted(s.ferns)},
               fern_frames={f: len(s.ferns[f]) for f in s.ferns}, woken=s.woken)
    q.put(res)
    dist.barrier()
    dist.destroy_process_group()


def run_oracle_session(scenario, n_ticks=None, relative_cons=True, **session_opts):
    from densemonoslam_amd import synth
    from oracle import orc_pipeline

    sc = SCENARIOS[scenario]
    s = orc_pipeline.Session(2, W, H, K, fern_photo_thresh=sc.fern_photo, **sc.opts, **session_opts)
    if relative_cons:
        for c in range(2):
            s.relative_cons[c].append(np.arange(6, dtype=np.float32) * np.float32(0.25 + c))
    for k in range(n_ticks or sc.n_ticks):
        fr = sc.frames(synth, k)
        s.step([fr[0], fr[1]], k)
    return s


# wake = 3: the schedule of the pipelined step (dms_session_step_async): the descriptor half of the queries every tick, the reference's
# block three ticks after a hit - here the RULE across two ranks (the flags gathered, both ranks woken at the same tick)
@pytest.mark.parametrize("scenario,wake", [("reference_rule", None), ("thumbnail_only", None), ("reference_rule", 3)])
def test_two_rank_session_merges_and_continues_like_the_one_process_session(orc, scenario, wake):
    sc = SCENARIOS[scenario]
    N_TICKS, QUERY_FROM = sc.n_ticks, sc.query_from
    extra = {"wake_latency": wake} if wake else {}
    ref = run_oracle_session(scenario, **extra)
    assert len(ref.merges) == 1 and ref.merges[0][0] >= QUERY_FROM and N_TICKS - ref.merges[0][0] > (4 if wake else 8), ref.merges
    if wake:
        assert ref.woken == [QUERY_FROM + wake] and ref.merges[0][0] == QUERY_FROM + wake, (ref.woken, ref.merges)
    if sc.opts.get("full_refine"):
        # the merge was decided by the reference's rule: a fern match under interMap = 1, then the full-resolution refinement accepted
        # at Options' default thresholds (50 iterations on every level, SO3 pre-alignment run)
        acc = [r for r in ref.refinements if r[3]]
        assert len(acc) == 1 and acc[0][0] == ref.merges[0][0], ref.refinements
        tr = acc[0][4]["track"]
        assert list(tr.iterations_run) == [50, 50, 50] and acc[0][4]["lastICPCount"] > 35000 and acc[0][4]["lastICPError"] < 2e-05
        # ... and it is a sensible transform: camera 1's map origin is camera 1's first pose (frame `offset` of the trajectory)
        from densemonoslam_amd import synth

        scn = getattr(synth, sc.scene)
        k_m, fb_, fa_, T_ = ref.merges[0]
        first = {0: scn.pose_fn(0), 1: scn.pose_fn(sc.offset)}
        gt = np.linalg.inv(first[fb_]) @ first[fa_]  # map fa -> map fb
        assert np.abs(T_.astype(np.float64) - gt).max() < 1e-2, (T_, gt)  # (observed 4.7 mm: young maps, thumbnail-seeded refinement)
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, scenario, extra)) for r in range(world)]
    for p in procs:
        p.start()
    results = {r["rank"]: r for r in [q.get(timeout=900) for _ in range(world)]}
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    k_merge, fb, fa, T = ref.merges[0]
    hb = fb % world  # the consuming frame's rank hosts both cameras afterwards
    for r in range(world):
        res = results[r]
        assert res["woken"] == ref.woken
        assert [(m[0], m[1], m[2]) for m in res["merges"]] == [(k_merge, fb, fa)], res["merges"]
        assert res["merges"][0][3].tobytes() == T.tobytes(), "ranks / oracle disagree about the relative transform"
        assert res["frame_of"] == ref.frame_of
        assert res["refinements"] == [r[:4] for r in ref.refinements]
        # hosting: one camera each up to and including the merge tick, then both on the consuming rank
        for k, hosted in enumerate(res["hosted"]):
            want = [r] if k < k_merge else ([0, 1] if r == hb else [])
            assert hosted == want, (r, k, hosted)
    host = results[hb]
    # the merged map, bit for bit
    m_ref = ref.cams[fb].model
    m_got = host["maps"][fb]
    assert len(m_got) == len(m_ref) and all(np.array_equal(m_got[f].view(np.uint32), m_ref[f].view(np.uint32)) for f in m_ref.dtype.names)
    assert host["fern_frames"][fb] == len(ref.ferns[fb].frames)
    # both trajectories (the consumed camera's pre-merge poses re-based into the consuming frame), bit for bit
    for c in range(2):
        got, want = host["pose_graph"][c], ref.pose_graph[c]
        assert [t for t, _ in got] == [t for t, _ in want] and len(got) == N_TICKS
        for (_, a), (_, b) in zip(got, want):
            assert np.asarray(a, np.float32).tobytes() == np.asarray(b, np.float32).tobytes(), c
        assert len(host["relative_cons"][c]) == 1 and host["relative_cons"][c][0].tobytes() == ref.relative_cons[c][0].tobytes()
    # and the re-basing did something: the consumed camera's first pose is no longer the identity
    assert not np.array_equal(host["pose_graph"][fa][0][1], np.eye(4, dtype=np.float32))


# ---- BASELINE config 5 at its stated size: --n 4, four cameras, all fusing (MainController.cpp:229,262-400) -------------------------
FOUR_OFFSETS = (0, 8, 16, 24)


def run_oracle_session_n(offsets, ticks, relative_cons=True, **session_opts):
    from densemonoslam_amd import synth
    from oracle import orc_pipeline

    sc = SCENARIOS["reference_rule"]
    s = orc_pipeline.Session(len(offsets), W, H, K, fern_photo_thresh=sc.fern_photo, **sc.opts, **session_opts)
    if relative_cons:
        for c in range(len(offsets)):
            s.relative_cons[c].append(np.arange(6, dtype=np.float32) * np.float32(0.25 + c))
    for k in range(ticks):
        fr = frames_at(synth, k, offsets)
        s.step([fr[c] for c in range(len(offsets))], k)
    return s


def check_four(ref, results, world, ticks, one_map=True):
    """every rank: the same merges / transforms / refinements / placement as the one-process oracle session; the rank that hosts a
    final map (a consuming frame never moves: rank fb % world): the map, the key-frame count, its cameras' trajectories and re-based
    constraint rows, bit for bit.  one_map: the session must have ended in ONE map that holds every camera's time slot."""
    n = len(ref.cams)
    last = lambda h: h[-1] if h and isinstance(h[0], list) else h
    assert len(ref.merges) >= 2, ref.merges
    if one_map:
        assert len(set(ref.frame_of)) == 1, ref.frame_of
    for r in range(world):
        res = results[r]
        assert [(m[0], m[1], m[2]) for m in res["merges"]] == [(m[0], m[1], m[2]) for m in ref.merges], (r, res["merges"])
        for got, want in zip(res["merges"], ref.merges):
            assert np.asarray(got[3], np.float32).tobytes() == want[3].tobytes(), "rank %d: a relative transform differs from the oracle's" % r
        assert res["frame_of"] == ref.frame_of and res["refinements"] == [x[:4] for x in ref.refinements]
        if res.get("woken") is not None:
            assert res["woken"] == ref.woken
        assert last(res["hosted"]) == [c for c in range(n) if ref.frame_of[c] % world == r], (r, res["hosted"])
    for fb in sorted(set(ref.frame_of)):
        host = results[fb % world]
        m_ref = ref.cams[fb].model
        m_got = host["maps"][fb]
        assert len(m_got) == len(m_ref), (fb, len(m_got), len(m_ref))
        for f in m_ref.dtype.names:
            assert np.array_equal(m_got[f].view(np.uint32), m_ref[f].view(np.uint32)), "map of frame %d differs in field %s" % (fb, f)
        members = [c for c in range(n) if ref.frame_of[c] == fb]
        # the map holds its cameras' time slots (with four the reference overruns Vertex::MAX_SENSORS = 3, Shaders/Vertex.cpp:49)
        assert all((m_ref["times"][:, c] > 0).any() for c in members)
        assert host["fern_frames"][fb] == len(ref.ferns[fb].frames)
        for c in members:
            got, want = host["pose_graph"][c], ref.pose_graph[c]
            assert [t for t, _ in got] == [t for t, _ in want] and len(got) == ticks
            for i, ((_, a), (_, b)) in enumerate(zip(got, want)):
                assert np.asarray(a, np.float32).tobytes() == np.asarray(b, np.float32).tobytes(), "camera %d pose %d differs" % (c, i)
            rc = host["relative_cons"][c]
            assert len(rc) == 1 and np.asarray(rc[0], np.float32).tobytes() == ref.relative_cons[c][0].tobytes(), "camera %d: relative constraint differs" % c


def spawn(world, target, args):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port, q) + tuple(args)) for r in range(world)]
    for p in procs:
        p.start()
    results = {r["rank"]: r for r in [q.get(timeout=1500) for _ in range(world)]}
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    return results


FOUR_TICKS, FOUR_TICKS_PIPELINED = 11, 20  # merges at ticks 6, 7, 8 (synchronous tick) / 9, 13, 17 (three ticks after each descriptor hit)
# Eight cameras, one per time slot (tests/test_session_gpu.py).  Synchronous tick: merges (6,0,1) (6,3,4) (7,2,0) (8,3,2) (9,6,3) (12,5,6).
# Pipelined: (9,3,0) (9,4,1) (13,4,3) (17,6,4) (22,2,6) - 23 is the smallest tick count at which the oracle session with wake_latency = 3
# shows at least five merges and a map with at least six live slots (its fifth merge happens in tick 22).
EIGHT_OFFSETS = (0, 8, 16, 24, 32, 40, 48, 56)
EIGHT_TICKS, EIGHT_TICKS_PIPELINED = 16, 23


@pytest.mark.parametrize("world,wake", [(4, None), (2, 3)])
def test_four_cameras_merge_over_gloo(orc, world, wake):
    """BASELINE config 5's size: four cameras, all fusing.  World 4, one camera per rank, the synchronous tick: every merge crosses ranks,
    the third one moves a frame that holds three cameras - its founder, an imported camera and another imported one - and the session
    ends in ONE map with four time slots on one rank while the other three forward their cameras' frames.  World 2, two cameras per
    rank, the pipelined schedule (the rule: flags gathered, every rank woken at the same tick), through its first two merges.  The
    protocol (stand-ins on the oracle) against the one-process oracle session."""
    ticks = FOUR_TICKS if wake is None else 15
    extra = {"wake_latency": wake} if wake else {}
    ref = run_oracle_session_n(FOUR_OFFSETS, ticks, **extra)
    if wake:
        assert ref.woken == [9, 13] and len(ref.merges) == 2, (ref.woken, ref.merges)
    results = spawn(world, _worker, ("reference_rule", extra, FOUR_OFFSETS, ticks))
    check_four(ref, results, world, ticks, one_map=wake is None)
