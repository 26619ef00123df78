"""The key-frame database kernels (csrc/ferns.hip) on crafted databases, at the sizes and edges no walk through the synthetic room
reaches: every entry point against tests/ferns_ref.py (held to oracle/orc_ferns.py by tests/test_ferns_cases_cpu.py, which also asserts
the conditions relied on here).  Ids, counts and the float32 dissimilarity are compared as bits; there is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

from tests import ferns_cases as fc
from tests.ferns_ref import RefDB

pytestmark = pytest.mark.gpu

W, H, K = fc.W, fc.H, fc.K
FORMS = ("1", "0")  # DMS_FERNS_PUBLISH_FUSED: one launch while the database is small / always four
_keep = []  # result buffers of pipelined searches stay allocated: a handle recognises its sequence by their address
_tables = {}


def table(seed=11, num=500, w=W, h=H):
    from oracle import orc_ferns

    key = (seed, num, w, h)
    if key not in _tables:
        _tables[key] = orc_ferns.Ferns(w, h, K, seed=seed, num=num)
    return _tables[key]


def sizes():
    from densemonoslam_amd import collab

    T = collab.thumbnail_bytes(W, H)
    return T, T + collab.DESC_BYTES, T + collab.DESC_CODES, T + collab.DESC_GOOD, T + collab.DESC_POSE


def bits(x):
    return int(np.array([x], np.float32).view(np.int32)[0])


class Blocks:
    """thumbnail blocks in HBM, each followed by its descriptor area {codes 512 | good | tick | pose} (the frame block of collaborative mode)"""

    def __init__(self, thumbs, poses=None):
        from densemonoslam_amd.capi import DeviceBuffer

        T, S, oc, og, op = sizes()
        self.n, self.thumbs, self.poses = len(thumbs), list(thumbs), poses
        host = np.full((self.n, S), 0x77, np.uint8)  # (a sentinel where the library is to write)
        for i, t in enumerate(thumbs):
            host[i, :T] = fc.pack(t)
            host[i, op:op + 64] = np.ascontiguousarray(poses[i] if poses is not None else np.eye(4), np.float32).reshape(-1).view(np.uint8)
        self.buf = DeviceBuffer(host.nbytes).upload(host)
        self.ptr = self.buf.ptr

    def at(self, i, off=0):
        return self.ptr + i * sizes()[1] + off

    def encode(self, g):
        T, S, oc, og, op = sizes()
        for i in range(self.n):
            g.encodeThumbs(self.at(i), self.at(i, oc), self.at(i, og))
        return self

    def host(self):
        return self.buf.download(np.uint8, (self.n, sizes()[1]))


class Db:
    """a library database and the reference's, fed the same offers"""

    def __init__(self, fused="1", capacity=16, seed=11, num=500):
        from densemonoslam_amd import ferns

        self.o = table(seed, num)
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("DMS_FERNS_PUBLISH_FUSED", fused)  # (read at creation)
            self.g = ferns.Ferns(W, H, K, num=num, seed=seed, capacity=capacity)
        self.ref = RefDB(self.o, capacity=capacity)
        self.blocks = []

    def offer(self, how, thumb, pose, time, thr):
        """one frame through an add entry point; returns the reference's slot (and, for the synchronous form, asserts the decision)"""
        from densemonoslam_amd.capi import DmsError

        T, S, oc, og, op = sizes()
        slot = self.ref.add(thumb, pose, time, thr)
        if how == "sync":
            try:
                added = self.g.addFrame(*fc.upsample(thumb), pose, time, float(thr))
                assert slot != -2, "the synchronous add must report a full database"
                assert added == (slot >= 0)
            except DmsError as e:
                assert e.code == -4 and slot == -2, (e.code, slot)  # DMS_ERR_CAPACITY
        else:
            b = Blocks([thumb], [pose])
            self.blocks.append(b)  # (read where it lies: unchanged until the work has run)
            if how == "async":
                self.g.addFrameAsync(b.at(0), b.at(0, op), time, float(thr))
            else:
                self.g.publishBlock(b.at(0), b.at(0, oc), b.at(0, og), b.at(0, op), time, float(thr))
        return slot

    def publish_many(self, blocks, first, count, times, thr):
        T, S, oc, og, op = sizes()
        for i in range(first, first + count):
            self.ref.add(blocks.thumbs[i], blocks.poses[i], times[i], thr)
            self.g.publishBlock(blocks.at(i), blocks.at(i, oc), blocks.at(i, og), blocks.at(i, op), times[i], float(thr))

    def frames(self):
        return [self.g.frame(i) for i in range(len(self.g))]

    def check_frames(self, what=""):
        check_frames(self.ref, self.frames(), what)

    def close(self):
        self.g.close()


def check_frames(ref, frames, what):
    """every stored frame (dms_ferns_get_frame: pose, time, good count, codes) against the reference's database"""
    assert len(frames) == len(ref), "%s: %d frames stored, the reference has %d" % (what, len(frames), len(ref))
    for i, (pose, t, good, codes) in enumerate(frames):
        same_pose = pose.tobytes() == ref.pose[i].tobytes()
        assert t == ref.time[i] and good == ref.good[i] and (codes == ref.codes[i]).all() and same_pose, (
            "%s: stored frame %d differs from the reference's (time %d / %d, good %d / %d, %d codes differ, pose %s)" % (
                what, i, t, ref.time[i], good, ref.good[i], int((codes != ref.codes[i]).sum()), "equal" if same_pose else "differs"))


def run_all(g, qb, time, inter):
    """the query blocks through every search entry point"""
    from densemonoslam_amd.capi import DeviceBuffer

    T, S, oc, og, op = sizes()
    n = qb.n
    out = {}
    best = DeviceBuffer(8)
    rows = []
    for i in range(n):
        g.searchCodes(qb.at(i, oc), qb.at(i, og), time, inter, best.ptr)
        rows.append(best.download(np.int32, (2,)))
    out["codes"] = np.array(rows)
    bn = DeviceBuffer(8 * n)
    g.searchBlocks(qb.ptr, S, n, -1, oc, og, time, inter, bn.ptr)
    out["blocks"] = bn.download(np.int32, (n, 2))
    g.searchBlocks(qb.ptr, S, n, n // 2, oc, og, time, inter, bn.ptr)
    out["skip"] = bn.download(np.int32, (n, 2))
    pb, prev = DeviceBuffer(8 * n), DeviceBuffer(8 * n)
    _keep.extend([pb, prev])
    out["pipe"] = []
    for k, skip in enumerate((-1, 0, n - 1, -1)):  # each call hands the call before it over
        g.searchBlocks(qb.ptr, S, n, skip, oc, og, time, inter, pb.ptr, previous_out=prev.ptr)
        if k:
            out["pipe"].append(prev.download(np.int32, (n, 2)))
    hits = DeviceBuffer(16 * n)
    out["hd"] = []
    for _ in range(2):
        g.searchBlocksHd(qb.ptr, S, n, oc, og, time, inter, hits.ptr)
        out["hd"].append(hits.download(np.int32, (n, 4)))
    out["find"] = []
    for i in range(n):
        m, _ = g.findFrameThumbs(qb.at(i), np.eye(4, dtype=np.float32), time, interMap=inter)
        out["find"].append((m.candidate, bits(m.dissimilarity), bits(m.blockHDAware), m.closest))
    return out


def expected(ref, thumbs, time, inter):
    return np.array([ref.row(*ref.encode(t), time, inter) for t in thumbs], np.int64).reshape(len(thumbs), 4)


def compare(out, rows, what):
    n = len(rows)
    two = np.where(rows[:, :1] < 0, -1, rows[:, :2])  # the result word: {-1, -1} without a candidate

    def same(got, want, name):
        assert (np.asarray(got, np.int64) == want).all(), "%s, %s:\ngot\n%s\nthe reference gives\n%s" % (what, name, np.asarray(got), want)

    same(out["codes"], two, "dms_ferns_search_codes")
    same(out["blocks"], two, "dms_ferns_search_blocks")
    for name, got, skip in [("dms_ferns_search_blocks with a skip", out["skip"], n // 2)] + [
            ("pipelined dms_ferns_search_blocks, call %d" % (k + 1), got, skip) for k, (got, skip) in enumerate(zip(out["pipe"], (-1, 0, n - 1)))]:
        want = two.copy()
        if skip >= 0:
            want[skip] = -1
        same(got, want, name)
    for k in range(2):
        same(out["hd"][k], rows, "dms_ferns_search_blocks_hd, call %d" % (k + 1))
    for i, (cand, dis, hd, closest) in enumerate(out["find"]):
        assert cand == rows[i, 0], "%s, dms_ferns_find_frame_thumbs query %d: candidate %d, the reference gives %d" % (what, i, cand, rows[i, 0])
        if cand >= 0:
            with np.errstate(all="ignore"):
                want_hd = bits(np.float32(rows[i, 3]) / np.float32(rows[i, 2]))
            assert dis == rows[i, 1] and hd == want_hd, "%s, dms_ferns_find_frame_thumbs query %d: dissimilarity / blockHDAware bits %x %x, reference %x %x" % (
                what, i, dis, hd, rows[i, 1], want_hd)
        else:
            assert closest == -1


# ---- a, b, f: the large database, built once per form -----------------------------------------------------------------------------

_big = {}


def big_data():
    if "data" not in _big:
        o = table()
        data = fc.big_sequence(o)
        ref = RefDB(o, capacity=fc.BIG_STOPS[-1])
        want, n = {}, 0
        for stop in fc.BIG_STOPS:
            while n < stop:
                ref.add(*data["frames"][n], -1.0)
                n += 1
            want[stop] = expected(ref, [t for t, _ in data["queries"][stop]], 0, True)
        extra = [fc.variant(o, fc.base(o), differ=100 + j, seed=8000 + j)[0] for j in range(3)]
        _big["data"] = (data, ref, want, extra)
    return _big["data"]


def big(fused):
    """the large database through dms_ferns_publish_block, every stop's queries through every entry point; then the overflow"""
    if fused not in _big:
        from densemonoslam_amd.capi import DmsError

        data, ref, want, extra = big_data()
        n_all = fc.BIG_STOPS[-1]
        db = Db(fused, capacity=n_all)  # (the capacity is the largest count used: the frames offered after it find the database full)
        db.ref = ref
        blocks = Blocks([f[0] for f in data["frames"]] + extra[:2], [f[1] for f in data["frames"]] + [fc.pose(0)] * 2)
        T, S, oc, og, op = sizes()
        res, n = {}, 0
        for stop in fc.BIG_STOPS:
            while n < stop:
                db.g.publishBlock(blocks.at(n), blocks.at(n, oc), blocks.at(n, og), blocks.at(n, op), data["frames"][n][2], -1.0)
                n += 1
            res[stop] = run_all(db.g, Blocks([t for t, _ in data["queries"][stop]]).encode(db.g), 0, 2)
        frames = db.frames()
        desc = blocks.host()[:n_all, sizes()[0]:sizes()[0] + 516].copy()
        # f, above 512: two more key frames (k_fern_decide finds the database full), then a synchronous add
        for i in (n_all, n_all + 1):
            db.g.publishBlock(blocks.at(i), blocks.at(i, oc), blocks.at(i, og), blocks.at(i, op), 7, -1.0)
        count = len(db.g)
        status = db.g.status()
        try:
            db.g.addFrame(*fc.upsample(extra[2]), fc.pose(1), 8, -1.0)
            rc = 0
        except DmsError as e:
            rc = e.code
        after = run_all(db.g, Blocks([t for t, _ in data["queries"][n_all]]).encode(db.g), 0, 2)
        _big[fused] = dict(res=res, frames=frames, desc=desc, count=count, status=status, rc=rc, status2=(len(db.g), db.g.status()), after=after, frames2=db.frames())
        db.close()
    return _big[fused]


@pytest.mark.parametrize("fused", FORMS)
def test_a_every_count_and_grid_shape(fused):
    """stored counts 1, 3, 4, 5, 8, 9, 511, 512, 513 and 519: the unique best frame at id 0, in the last wave of a full block, the first of
    the next, at the last id, at every residue mod 8; ties included (b)"""
    data, ref, want, _ = big_data()
    got = big(fused)
    for stop in fc.BIG_STOPS:
        targets = [t for _, t in data["queries"][stop]]
        compare(got["res"][stop], want[stop], "%d frames stored (queries aimed at ids %s)" % (stop, targets))
        for i, t in enumerate(targets):
            if t is not None:
                assert want[stop][i, 0] == t


@pytest.mark.parametrize("fused", FORMS)
def test_a_every_stored_frame(fused):
    data, ref, want, _ = big_data()
    got = big(fused)
    check_frames(ref, got["frames"], "the database of %d frames (ids 511, 512 and 513 straddle the end of the one-launch form)" % len(ref))
    # the descriptor publish_block wrote into each block
    for i in range(len(ref)):
        assert (got["desc"][i, :500] == ref.codes[i]).all() and (got["desc"][i, 500:512] == 255).all() and got["desc"][i, 512:516].view(np.int32)[0] == ref.good[i], i


def test_a_four_launch_form_identical():
    a, b = big("1"), big("0")
    assert a["count"] == b["count"] and a["status"] == b["status"] and a["rc"] == b["rc"] and a["status2"] == b["status2"]
    assert (a["desc"] == b["desc"]).all()
    for fa, fb in zip(a["frames"] + a["frames2"], b["frames"] + b["frames2"]):
        assert fa[1] == fb[1] and fa[2] == fb[2] and (fa[3] == fb[3]).all() and fa[0].tobytes() == fb[0].tobytes()
    for ra, rb in list(zip(a["res"].values(), b["res"].values())) + [(a["after"], b["after"])]:
        for key in ra:
            assert np.array_equal(np.array(ra[key]), np.array(rb[key])), key


@pytest.mark.parametrize("fused", FORMS)
def test_b_ties_go_to_the_lowest_id(fused):
    """one thumbnail stored at ids 10, 205 and 516: a query equal to it gets id 10 at +0; two different frames at ids 13 and 330, both at
    10 / 500 from the query: id 13 - from every entry point, at every count at which more than one of them is stored"""
    data, ref, want, _ = big_data()
    got = big(fused)
    for stop in (511, 512, 513, fc.BIG_STOPS[-1]):
        nq = len(data["queries"][stop])
        res = got["res"][stop]
        for q, (first, dbits) in ((nq - 2, (fc.TIE_ZERO_IDS[0], 0)), (nq - 1, (fc.TIE_PAIR_IDS[0], bits(np.float32(10) / np.float32(500))))):
            assert list(want[stop][q, :2]) == [first, dbits]
            rows = [res["codes"][q], res["blocks"][q], res["pipe"][0][q], res["hd"][0][q, :2], res["hd"][1][q, :2], res["find"][q][:2]]
            assert all(list(r) == [first, dbits] for r in rows), (stop, q, rows)


@pytest.mark.parametrize("fused", FORMS)
def test_f_full_above_512(fused):
    data, ref, want, _ = big_data()
    got = big(fused)
    n = fc.BIG_STOPS[-1]
    assert got["count"] == n == len(ref) and got["status"] == (n, 2), got["status"]  # both late key frames counted as dropped
    assert got["rc"] == -4 and got["status2"] == (n, (n, 3))  # DMS_ERR_CAPACITY
    check_frames(ref, got["frames2"], "after the overflow")
    compare(got["after"], want[n], "after the overflow")


# ---- c: the age gate ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fused", FORMS)
def test_c_age_gate(fused):
    ag = fc.age_gate_case(table())
    db = Db(fused, capacity=8)
    for t, pose, time in ag["frames"]:
        db.offer("publish", t, pose, time, -1.0)
    db.check_frames("age gate")
    qb = Blocks([ag["query"], ag["frames"][0][0]]).encode(db.g)
    for time, inter, first in ((ag["time"], 0, 4), (ag["time_none"], 0, -1), (ag["time"], 1, 1), (ag["time"], 2, 1), (ag["time_none"], 2, 1)):
        rows = expected(db.ref, qb.thumbs, time, inter)
        assert rows[0, 0] == first
        if first == -1:
            assert rows.tolist() == [[-1, 0, 0, 0]] * 2
        compare(run_all(db.g, qb, time, inter), rows, "ages 299 / 300 / 301 at time %d, interMap %d" % (time, inter))
    db.close()


# ---- d: valid counts ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fused", FORMS)
def test_d_valid_counts(fused):
    cases, empty = fc.valid_count_cases(table())
    for name, stored, queries, (g, gj) in cases:
        db = Db(fused, capacity=8)
        assert db.offer("publish", stored, fc.pose(1), 1, -1.0) == 0
        qb = Blocks(queries + [empty]).encode(db.g)
        assert [int(r[sizes()[3]:sizes()[3] + 4].view(np.int32)[0]) for r in qb.host()] == [g] * len(queries) + [0]
        rows = expected(db.ref, qb.thumbs, 0, True)
        assert (rows[:-1, 0] == 0).all() and rows[-1].tolist() == [-1, 0, 0, 0]
        if (g, gj) == (3, 3):
            assert rows[:, 1].tolist()[:2] == [bits(np.float32(2) / np.float32(3)), bits(np.float32(1) / np.float32(3))]
        compare(run_all(db.g, qb, 0, 1), rows, "valid ferns: query %s stored" % name)
        # the frame without a valid fern is refused by every add, and leaves the database as it was
        for how in ("sync", "async", "publish"):
            assert db.offer(how, empty, fc.pose(2), 2, -1.0) == -1
        db.check_frames("after the offers of a frame without a valid fern")
        assert db.g.status() == (1, 0)
        # the add decision takes min(g, gj) too: the same queries offered as key frames
        for how in ("sync", "async", "publish"):
            for k, t in enumerate(queries):
                db.offer(how, t, fc.pose(3 + k), 3 + k, 0.1)
        db.check_frames("key frames of %s valid ferns offered at threshold 0.1" % name)
        db.close()
    db = Db(fused, capacity=4)  # ... not even by an empty database (a stored frame never has a good count of 0)
    compare(run_all(db.g, Blocks([empty, cases[0][1]]).encode(db.g), 0, 1), np.array([[-1, 0, 0, 0]] * 2), "an empty database")
    for how in ("sync", "async", "publish"):
        assert db.offer(how, empty, fc.pose(2), 2, -1.0) == -1
    assert len(db.g) == 0
    db.close()


# ---- e: the threshold at equality ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("how", ("sync", "async", "publish"))
@pytest.mark.parametrize("fused", FORMS)
def test_e_threshold_equality(fused, how):
    for thr, stored, at, above in fc.threshold_cases(table()):
        db = Db(fused, capacity=4)
        assert db.offer(how, stored, fc.pose(0), 0, -1.0) == 0
        assert db.offer(how, at, fc.pose(1), 1, thr) == -1 and bits(db.ref.last_minimum) == bits(thr)  # minimum == threshold: not "greater"
        assert len(db.g) == 1, "a frame whose minimum dissimilarity EQUALS the threshold %r was stored" % thr
        assert db.offer(how, above, fc.pose(2), 2, thr) == 1
        assert len(db.g) == 2, "a frame one fern above the threshold %r was rejected" % thr
        db.offer(how, at, fc.pose(3), 3, np.nextafter(thr, np.float32(0)))
        db.check_frames("threshold %r" % thr)
        db.close()


@pytest.mark.parametrize("how", ("sync", "async", "publish"))
@pytest.mark.parametrize("fused", FORMS)
def test_e_mixed_sequence_of_offers(fused, how):
    """the sequence on which the reference is held to the oracle (duplicates, ties, few / one / no valid ferns, thresholds met exactly):
    every decision of every add entry point, through the database it leaves"""
    seq = fc.mixed_sequence(table())
    db = Db(fused, capacity=len(seq))
    for k, (t, pose, time, thr) in enumerate(seq):
        db.offer(how, t, pose, time, thr)
        if k % 16 == 15:
            assert len(db.g) == len(db.ref), k
    db.check_frames("the mixed sequence through %s" % how)
    assert db.g.status() == (len(db.ref), 0)
    qb = Blocks([s[0] for s in seq[::4]]).encode(db.g)
    for time, inter in ((0, 1), (640, 0)):
        compare(run_all(db.g, qb, time, inter), expected(db.ref, qb.thumbs, time, inter), "the mixed sequence, time %d, interMap %d" % (time, inter))
    db.close()


# ---- f: a database that fills below 512 ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fused", FORMS)
def test_f_full_below_512(fused):
    frames = fc.full_case(table(), 10)
    db = Db(fused, capacity=5)
    for t, pose, time in frames[:8]:
        db.offer("publish", t, pose, time, -1.0)
    assert len(db.g) == 5 == len(db.ref) and db.g.status() == (5, 3) == (len(db.ref), db.ref.dropped)
    assert db.offer("sync", frames[8][0], frames[8][1], 9, -1.0) == -2  # (asserts DMS_ERR_CAPACITY)
    assert db.offer("sync", frames[2][0], frames[2][1], 9, 0.1) == -1  # a duplicate is still just rejected
    assert db.offer("async", frames[9][0], frames[9][1], 9, -1.0) == -2
    assert len(db.g) == 5 and db.g.status() == (5, 5) == (len(db.ref), db.ref.dropped)
    db.check_frames("a full database")
    qb = Blocks([f[0] for f in frames]).encode(db.g)
    compare(run_all(db.g, qb, 0, 1), expected(db.ref, qb.thumbs, 0, True), "a full database")
    db.close()


# ---- g: rejections widen the host's bound of the count ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("fused", FORMS)
def test_g_rejections_widen_the_bound(fused):
    from densemonoslam_amd.capi import DeviceBuffer

    o = table()
    T, S, oc, og, op = sizes()
    b = fc.base(o)
    first = [(fc.variant(o, b, differ=150 + 20 * j, seed=900 + j)[0], fc.pose(j), j) for j in range(9)]
    late = [(fc.variant(o, b, differ=170 + 20 * j, seed=950 + j)[0], fc.pose(50 + j), 50 + j) for j in range(3)]
    db = Db(fused, capacity=64)
    for f in first:
        db.offer("publish", *f, -1.0)
    assert len(db.g) == 9
    blocks = Blocks([first[0][0]] * 40 + [f[0] for f in late], [fc.pose(9)] * 40 + [f[1] for f in late])
    qb = Blocks([f[0] for f in first[::3] + late] + [fc.variant(o, late[2][0], differ=9, seed=990)[0]]).encode(db.g)
    for i in range(43):  # 40 duplicates (all rejected), then 3 new key frames: no synchronisation in between
        thumb, pose, time = (first[0][0], fc.pose(9), 20 + i) if i < 40 else late[i - 40]
        slot = db.ref.add(thumb, pose, time, 0.1)
        assert slot == (-1 if i < 40 else 9 + i - 40)
        db.g.publishBlock(blocks.at(i), blocks.at(i, oc), blocks.at(i, og), blocks.at(i, op), time, 0.1)
    rows = expected(db.ref, qb.thumbs, 0, True)
    assert rows[-1, 0] == 11
    r1, h1, r2, h2 = DeviceBuffer(8 * qb.n), DeviceBuffer(16 * qb.n), DeviceBuffer(8 * qb.n), DeviceBuffer(16 * qb.n)
    db.g.searchBlocks(qb.ptr, S, qb.n, -1, oc, og, 0, True, r1.ptr)
    db.g.searchBlocksHd(qb.ptr, S, qb.n, oc, og, 0, True, h1.ptr)
    assert len(db.g) == 12  # (synchronises: the bound is exact again)
    db.g.searchBlocks(qb.ptr, S, qb.n, -1, oc, og, 0, True, r2.ptr)
    db.g.searchBlocksHd(qb.ptr, S, qb.n, oc, og, 0, True, h2.ptr)
    for r, h, when in ((r1, h1, "before"), (r2, h2, "after")):
        assert (r.download(np.int32, (qb.n, 2)) == rows[:, :2]).all() and (h.download(np.int32, (qb.n, 4)) == rows).all(), when
    db.check_frames("after 40 rejected and 3 accepted asynchronous adds")
    assert db.g.status() == (12, 0)
    db.close()


# ---- h: other tables -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("num", (1, 63, 64, 65, 512))
def test_h_other_tables(num):
    o = table(7, num)
    db = Db("1", capacity=9, seed=7, num=num)
    pos, rgbd = db.g.table()
    assert (pos == o.pos).all() and (rgbd == o.rgbd).all()
    five = fc.other_table_thumbs(o)
    qb = Blocks(five).encode(db.g)
    T, S, oc, og, op = sizes()
    for i, row in enumerate(qb.host()):
        codes, good = db.ref.encode(five[i])
        assert (row[oc:oc + num] == codes).all() and (row[oc + num:oc + 512] == 255).all() and row[og:og + 4].view(np.int32)[0] == good, (num, i)
    b = fc.base(o)
    for j in range(9):
        db.offer("publish" if j % 2 else "async", fc.variant(o, b, differ=(5 * j) % (num + 1), valid=num - (j % 3) * (num // 8), seed=j)[0], fc.pose(j), j, -1.0)
    db.check_frames("a table of %d ferns" % num)
    assert len(db.g) == 9
    compare(run_all(db.g, qb, 0, 1), expected(db.ref, five, 0, True), "a table of %d ferns" % num)
    db.close()


# ---- i: full-resolution textures whose size is no multiple of 8 -----------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", ((333, 251), (1241, 376)))
def test_i_ragged_sizes(w, h):
    from densemonoslam_amd import ferns

    o = table(13, 500, w, h)
    g = ferns.Ferns(w, h, K, seed=13, capacity=2)
    pos, rgbd = g.table()
    assert (pos == o.pos).all() and (rgbd == o.rgbd).all() and pos[:, 0].max() < w // 8 and pos[:, 1].max() < h // 8
    r = np.random.RandomState(w)
    for k in range(2):
        img = r.randint(0, 256, (h, w, 4)).astype(np.uint8)
        v = r.uniform(-1, 1, (h, w, 4)).astype(np.float32)
        v[..., 2] = r.uniform(0.2, 3.6, (h, w)).astype(np.float32) * (r.uniform(0, 1, (h, w)) > 0.3)  # holes
        n = r.uniform(-1, 1, (h, w, 4)).astype(np.float32)
        codes, good = g.encode(img, v, n)
        ti, tv, tn = o._thumbs(img, v, n)
        want, wgood, _ = o._encode(ti, tv)
        assert good == wgood and 0 < good < 500 and (codes == want).all(), (w, h, k, good, wgood, int((codes != want).sum()))
    g.close()


# ---- j: merge --------------------------------------------------------------------------------------------------------------------------

def test_j_merge():
    from densemonoslam_amd.capi import DeviceBuffer

    o_src, o_dst = table(21), table(22)
    m = fc.merge_case(o_src, o_dst)
    src = Db("1", capacity=140, seed=21)
    sb = Blocks([f[0] for f in m["src"]], [f[1] for f in m["src"]])
    src.publish_many(sb, 0, len(m["src"]), [f[2] for f in m["src"]], -1.0)
    assert len(src.g) == 130
    src.check_frames("the source of the merge")
    dsts = []
    for k in range(3):
        d = Db("1", capacity=160, seed=22)
        db_ = Blocks([f[0] for f in m["dst"]], [f[1] for f in m["dst"]])
        d.publish_many(db_, 0, len(m["dst"]), [f[2] for f in m["dst"]], -1.0)
        d.keep = db_
        dsts.append(d)
    thr = float(m["threshold"])
    # in place
    want = dsts[0].ref.consume(src.ref, m["T"], thr)
    assert dsts[0].g.consume(src.g, m["T"], thr) == want and 20 < want < 110
    dsts[0].check_frames("dms_ferns_consume")
    # as records
    rb = src.g.recordBytes()
    assert rb >= sizes()[0] + 68 and rb % 16 == 0
    rec = DeviceBuffer(130 * rb)
    assert src.g.exportRecords(0, 0) == 0
    assert src.g.exportRecords(rec.ptr, 50) == 50
    want50 = dsts[2].ref.consume(src.ref, m["T"], thr, count=50)
    assert dsts[2].g.consumeRecords(rec.ptr, 50, m["T"], thr) == want50
    dsts[2].check_frames("dms_ferns_consume_records of the first 50")
    assert src.g.exportRecords(rec.ptr, 200) == 130
    assert dsts[1].ref.consume(src.ref, m["T"], thr) == want
    assert dsts[1].g.consumeRecords(rec.ptr, 130, m["T"], thr) == want
    dsts[1].check_frames("dms_ferns_export_records -> dms_ferns_consume_records")
    src.check_frames("the source after the merge")
    for d in dsts + [src]:
        d.close()


# ---- k: mirrors ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fused", FORMS)
def test_k_mirrors(fused):
    import torch
    from densemonoslam_amd.capi import DeviceBuffer, check, lib

    P, I, Z = C.c_void_p, C.c_int, C.c_size_t
    lib.dms_ferns_publish_block_mirror.argtypes = [P, P, P, P, P, I, C.c_float, P, Z, Z, P]
    lib.dms_ferns_search_blocks_hd_mirror.argtypes = [P, P, Z, I, Z, Z, I, I, P, P, Z, Z, P]
    o = table()
    T, S, oc, og, op = sizes()
    nb = S - T  # the whole descriptor area: codes, the good-count word, tick, pose
    frames = fc.full_case(o, 4)
    db = Db(fused, capacity=8)
    blocks = Blocks([f[0] for f in frames], [f[1] for f in frames])
    host = torch.zeros(4 * nb, dtype=torch.uint8).pin_memory()
    for i, (t, pose, time) in enumerate(frames):
        db.ref.add(t, pose, time, 0.05)
        check(lib.dms_ferns_publish_block_mirror(db.g.h, P(blocks.at(i)), P(blocks.at(i, oc)), P(blocks.at(i, og)), P(blocks.at(i, op)), time, 0.05,
                                                 P(host.data_ptr() + i * nb), Z(oc), Z(nb), None), "dms_ferns_publish_block_mirror")
    assert len(db.g) == 4
    now = blocks.host()
    got = host.numpy().reshape(4, nb)
    for i in range(4):
        codes, good = db.ref.encode(frames[i][0])
        assert (now[i, oc:oc + 500] == codes).all() and now[i, og:og + 4].view(np.int32)[0] == good == 500
        assert (got[i] == now[i, oc:]).all(), "publish %d: the mirrored words differ from the block's at %s" % (i, np.flatnonzero(got[i] != now[i, oc:])[:8])
    db.check_frames("publish with a mirror")
    hits = DeviceBuffer(16 * 4)
    host.zero_()
    check(lib.dms_ferns_search_blocks_hd_mirror(db.g.h, P(blocks.ptr), Z(S), 4, Z(oc), Z(og), 0, 1, P(hits.ptr), P(host.data_ptr()), Z(oc), Z(nb), None),
          "dms_ferns_search_blocks_hd_mirror")
    rows = hits.download(np.int32, (4, 4))
    assert (rows == expected(db.ref, blocks.thumbs, 0, True)).all() and (rows[:, 0] == np.arange(4)).all()
    assert (host.numpy().reshape(4, nb) == blocks.host()[:, oc:]).all()
    db.close()
