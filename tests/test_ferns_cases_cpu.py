"""The crafted fern-database cases on the CPU: tests/ferns_ref.py (the vectorised reference the GPU tests compare with) is held to
oracle/orc_ferns.Ferns decision for decision and bit for bit, and every condition that tests/test_ferns_database_gpu.py relies on
("by the reference": which frame is the unique best, which frames tie, which is rejected by its age, which minimum equals the
threshold) is asserted here, where no GPU is needed."""
import numpy as np
import pytest

from oracle import orc_ferns
from tests import ferns_cases as fc
from tests.ferns_ref import FLT_MAX, RefDB

bits = lambda x: np.array([x], np.float32).view(np.uint32)[0]


@pytest.fixture(scope="module")
def o500():
    return orc_ferns.Ferns(fc.W, fc.H, fc.K, seed=11)


def fresh(seed=11, num=500):
    return orc_ferns.Ferns(fc.W, fc.H, fc.K, seed=seed, num=num)


def test_generator_counts_and_depth_threshold(o500):
    o = o500
    b = fc.base(o)
    for k, v in ((0, 500), (1, 500), (250, 500), (500, 500), (0, 7), (7, 7), (2, 3), (0, 1), (1, 1), (0, 0), (100, 317)):
        t, flip, dead = fc.variant(o, b, differ=k, valid=v, seed=k + v)
        c, g, _ = o._encode(t[0], t[1])
        cb, _, _ = o._encode(b[0], b[1])
        assert g == v and int(((c != cb) & (c != 255)).sum()) == k
    with pytest.raises(AssertionError):
        fc.variant(o, b, differ=8, valid=7)
    lo, hi = fc.depth_at_threshold(o, b, fern=5)
    cl, ch = o._encode(lo[0], lo[1])[0], o._encode(hi[0], hi[1])[0]
    assert cl[5] & 1 == 0 and ch[5] & 1 == 1 and (cl[5] | 1) == ch[5]
    ref = RefDB(o)
    for t in (b, lo, hi, fc.variant(o, b, differ=77, valid=200, seed=3)[0]):
        c, g, _ = o._encode(t[0], t[1])
        rc, rg = ref.encode(t)
        assert rg == g and (rc == c).all()
    # the packed block: image | vertex | normal, the image padded to 16 bytes
    blk = fc.pack(b)
    assert blk.size == 1200 * 36 and (blk[1200 * 4:1200 * 20].view(np.float32).reshape(30, 40, 4) == b[1]).all()


def test_reference_equals_the_oracle_on_the_mixed_sequence():
    o = fresh()
    seq = fc.mixed_sequence(o)
    assert 55 <= len(seq) <= 70
    ref = RefDB(o)
    outcomes = []
    for k, (t, pose, time, thr) in enumerate(seq):
        a = o._add(t[0], t[1], t[2], pose, time, thr)
        slot = ref.add(t, pose, time, thr)
        assert a == (slot >= 0), k
        outcomes.append(a)
        assert len(ref) == len(o.frames)
    assert 10 < sum(outcomes) < len(seq) - 5  # both decisions occur often
    for i, fr in enumerate(o.frames):
        assert (ref.codes[i] == fr.codes).all() and ref.good[i] == fr.goodCodes and ref.time[i] == fr.srcTime and ref.pose[i].tobytes() == fr.pose.tobytes()
    assert min(ref.good) == 1 and max(ref.good) == 500
    seen_none = seen_tie = 0
    for k, (t, _, _, _) in enumerate(seq):
        for time, inter in ((0, True), (1200, False), (640, False), (310, False), (0, False)):
            codes, minimum, minId = o._search(t[0], t[1], time, inter)
            q, g = ref.encode(t)
            i, d = ref.search(q, g, time, inter)
            assert i == minId and bits(d) == bits(minimum), (k, time, inter, i, minId)
            assert ref.hit(q, g, time, inter) == o.searchHit(t, time, inter), (k, time, inter)
            if i >= 0:
                c, e = ref.hd(q, i)
                with np.errstate(all="ignore"):
                    assert bits(np.float32(e) / np.float32(c)) == bits(o.blockHDAware(codes, o.frames[i].codes))
                dd = ref.dissimilarities(q, g)
                seen_tie += int((dd == d).sum() > 1)
            else:
                assert d == FLT_MAX
                seen_none += 1
    assert seen_none > 0 and seen_tie > 0
    # consume: the same frames, re-posed, offered to another table's database
    o2, o3 = fresh(seed=12), fresh(seed=12)
    r2 = RefDB(o2)
    for t, pose, time, thr in seq[:8]:
        assert o2._add(t[0], t[1], t[2], pose, time, thr) == (r2.add(t, pose, time, thr) >= 0)
    T = fc.pose(999)
    assert o2.consume(o, T, 0.1) == r2.consume(ref, T, 0.1) > 0
    assert len(r2) == len(o2.frames) < len(ref) + 8
    for i, fr in enumerate(o2.frames):
        assert (r2.codes[i] == fr.codes).all() and r2.good[i] == fr.goodCodes and r2.time[i] == fr.srcTime and r2.pose[i].tobytes() == fr.pose.tobytes()
    # a capacity: what the reference would have stored beyond it is counted, not stored
    rc = RefDB(o3, capacity=5)
    for k, (t, pose, time, thr) in enumerate(seq[:20]):
        _, minimum, _ = o3._search(t[0], t[1], 0, True)
        want = (minimum > thr or len(o3.frames) == 0) and o3._encode(t[0], t[1])[1] > 0
        slot = rc.add(t, pose, time, thr)
        if len(o3.frames) < 5:
            assert o3._add(t[0], t[1], t[2], pose, time, thr) == want == (slot >= 0)
        else:
            assert slot == (-2 if want else -1), k
    assert len(rc) == 5 and rc.dropped > 0


def test_conditions_of_the_large_database(o500):
    o = o500
    big = fc.big_sequence(o)
    ref = RefDB(o)
    n = 0
    assert fc.BIG_STOPS[-1] > 512 and fc.BIG_STOPS[-1] % 4 != 0 and len(big["frames"]) == fc.BIG_STOPS[-1] < 600
    for stop in fc.BIG_STOPS:
        while n < stop:
            t, pose, time = big["frames"][n]
            assert ref.add(t, pose, time, -1.0) == n  # threshold -1: every frame is stored
            n += 1
        for t, target in big["queries"][stop]:
            q, g = ref.encode(t)
            i, d = ref.search(q, g, 0, True)
            dd = ref.dissimilarities(q, g)
            if target is not None:  # the unique best frame, by the reference
                assert i == target and int((dd == d).sum()) == 1 and bits(d) == bits(np.float32(3) / np.float32(min(g, ref.good[i]))), (stop, target)
    assert len(set(ref.good)) > 20
    # ties: the same thumbnail three times at +0; two different frames at 10 / 500
    q, g = ref.encode(big["tie_zero"])
    dd = ref.dissimilarities(q, g)
    assert tuple(np.flatnonzero(dd == dd.min())) == fc.TIE_ZERO_IDS and bits(dd.min()) == 0
    assert ref.search(q, g, 0, True)[0] == fc.TIE_ZERO_IDS[0]
    assert len({i // 4 for i in fc.TIE_ZERO_IDS}) == 3 and len({i % 4 for i in fc.TIE_ZERO_IDS}) == 3 and len({i // 8 for i in fc.TIE_ZERO_IDS}) == 3
    assert fc.TIE_ZERO_IDS[-1] > 512
    q, g = ref.encode(big["tie_pair_query"])
    dd = ref.dissimilarities(q, g)
    assert tuple(np.flatnonzero(dd == dd.min())) == fc.TIE_PAIR_IDS and bits(dd.min()) == bits(np.float32(10) / np.float32(500)) != 0
    assert not (ref.codes[fc.TIE_PAIR_IDS[0]] == ref.codes[fc.TIE_PAIR_IDS[1]]).all()
    assert len({i // 4 for i in fc.TIE_PAIR_IDS}) == 2 and len({i % 4 for i in fc.TIE_PAIR_IDS}) == 2 and len({i // 8 for i in fc.TIE_PAIR_IDS}) == 2


def test_conditions_of_the_small_cases(o500):
    o = o500
    # age gate: ages 299 / 300 / 301 on the three best frames, best first
    ag = fc.age_gate_case(o)
    ref = RefDB(o)
    for t, pose, time in ag["frames"]:
        assert ref.add(t, pose, time, -1.0) >= 0
    q, g = ref.encode(ag["query"])
    order = np.argsort(ref.dissimilarities(q, g), kind="stable")[:3]
    assert [ag["time"] - ref.time[i] for i in order] == [299, 300, 301] and list(order) == [1, 2, 4]
    assert len(set(ref.dissimilarities(q, g)[order])) == 3
    assert ref.search(q, g, ag["time"], False)[0] == 4 and ref.search(q, g, ag["time"], True)[0] == 1
    assert ref.search(q, g, ag["time_none"], False) == (-1, FLT_MAX) and ref.row(q, g, ag["time_none"], False) == [-1, 0, 0, 0]
    # valid counts
    cases, empty = fc.valid_count_cases(o)
    for name, stored, queries, (g_want, gj_want) in cases:
        ref = RefDB(o)
        assert ref.add(stored, fc.pose(0), 0, -1.0) == 0 and ref.good[0] == gj_want, name
        for t in queries:
            q, g = ref.encode(t)
            assert g == g_want and ref.search(q, g, 0, True)[0] == 0, name
        if g_want == gj_want == 3:
            got = [bits(ref.search(*ref.encode(t), 0, True)[1]) for t in queries]
            assert got == [bits(np.float32(2) / np.float32(3)), bits(np.float32(1) / np.float32(3))]
        q, g = ref.encode(empty)
        assert g == 0 and (q == 255).all() and ref.search(q, g, 0, True) == (-1, FLT_MAX) and ref.add(empty, fc.pose(0), 0, -1.0) == -1
    assert RefDB(o).add(empty, fc.pose(0), 0, -1.0) == -1  # not even into an empty database
    # threshold equality
    for thr, stored, at, above in fc.threshold_cases(o):
        ref = RefDB(o)
        assert ref.add(stored, fc.pose(0), 0, -1.0) == 0
        assert ref.add(at, fc.pose(1), 1, thr) == -1 and bits(ref.last_minimum) == bits(thr)
        assert ref.add(above, fc.pose(2), 2, thr) == 1 and bits(ref.last_minimum) > bits(thr)
        ref = RefDB(o)
        assert ref.add(stored, fc.pose(0), 0, -1.0) == 0 and ref.add(at, fc.pose(3), 3, np.nextafter(thr, np.float32(0))) == 1  # the next threshold below


@pytest.mark.parametrize("num", [1, 63, 64, 65, 512])
def test_other_tables(num):
    o = fresh(seed=7, num=num)
    assert o.pos.shape == (num, 2) and o.pos[:, 0].max() < 40 and o.pos[:, 1].max() < 30
    b = fc.base(o)
    ref = RefDB(o)
    for t in fc.other_table_thumbs(o):
        c, g, _ = o._encode(t[0], t[1])
        rc, rg = ref.encode(t)
        assert (c == rc).all() and g == rg


def test_merge_case_rejects_some():
    o_src, o_dst = fresh(seed=21), fresh(seed=22)
    m = fc.merge_case(o_src, o_dst)
    src, dst = RefDB(o_src), RefDB(o_dst)
    for t, pose, time in m["src"]:
        src.add(t, pose, time, -1.0)
    for t, pose, time in m["dst"]:
        dst.add(t, pose, time, -1.0)
    assert len(src) == 130 and len(dst) == 20
    added = dst.consume(src, m["T"], m["threshold"])
    assert 20 < added < 110 and len(dst) == 20 + added
    assert not (m["T"][:3] == np.eye(4)[:3]).any()
