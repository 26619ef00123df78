"""Crafted graphs and constraints for the deformation-graph tests (CPU and GPU): time-sorted nodes along a camera path that returns to
its start, constraint points within the nodes' extent near the place where the loop closes, each with its target a few centimetres
away (a small rigid motion, as a loop's drift is) and, unless stated, its pin."""
import numpy as np


def make_nodes(n, seed):
    rng = np.random.default_rng(seed)
    s = np.linspace(0.0, 2.0 * np.pi * 1.04, n)  # a closed path with a little overlap: the last nodes lie beside the first
    pos = np.stack([1.5 * np.cos(s), 0.3 * np.sin(2 * s), 2.0 + 1.5 * np.sin(s)], 1) + rng.normal(size=(n, 3)) * 0.03
    times = 1 + np.cumsum(rng.choice([0, 0, 1, 2, 3], size=n))  # non-decreasing, with runs of equal times
    return np.concatenate([pos, times[:, None]], 1).astype(np.float32)


def make_rows(nodes4, m, seed, shift=1.0):
    """m rows {src xyz, target xyz, target time}: sources around the first nodes, targets = the sources moved by a small rigid motion"""
    rng = np.random.default_rng(seed + 1000)
    n = len(nodes4)
    near = rng.integers(0, max(3, n // 6), size=m)
    src = nodes4[near, :3].astype(np.float64) + rng.normal(size=(m, 3)) * 0.08
    a = 0.02 * shift
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    c = src.mean(0)
    tgt = (src - c) @ R.T + c + np.array([0.02, -0.01, 0.015]) * shift
    ttime = nodes4[near, 3]
    return np.concatenate([src, tgt, ttime[:, None]], 1).astype(np.float32)


class Case:
    def __init__(self, name, n, m, seed, pins=True, last_deform_time=0, shift=1.0):
        self.name = name
        self.nodes = make_nodes(n, seed)
        self.rows = make_rows(self.nodes, m, seed, shift)
        self.pins = pins
        self.src_time = int(self.nodes[-1, 3]) + 1  # the closing frame's tick
        self.time = self.src_time
        self.last_deform_time = last_deform_time
        self.relax = False

    @property
    def batches(self):
        """the addConstraints calls of the case, in order: (rows, source time, pin)"""
        return [(self.rows, self.src_time, self.pins)]

    def __repr__(self):
        return self.name


def _suffix_time(n, seed, keep):
    """a lastDeformTime that leaves exactly the last `keep` nodes enabled"""
    t = make_nodes(n, seed)[:, 3]
    k = n - keep
    while t[k - 1] == t[k]:  # the cut must fall between two different times
        k -= 1
    return int(t[k - 1]), n - k


def staged_cases():
    ldt, kept = _suffix_time(45, 5, 32)
    assert kept == 32, kept
    return [
        Case("n5_c3", 5, 3, 1, shift=40.0),        # error grows in the third iteration
        Case("n6_c7", 6, 7, 2, shift=0.05),        # small delta after one iteration
        Case("n24_c40", 24, 40, 3, shift=40.0),    # all three iterations
        Case("n45_c120", 45, 120, 4, shift=3.0),   # small error after two
        Case("n45_c120_nopins_suffix32", 45, 120, 5, pins=False, last_deform_time=ldt, shift=20.0),
        Case("n130_c768", 130, 768, 6),            # small error after one
    ]


def large_case():
    return Case("n512_c768", 512, 768, 7)


def singular_case():
    return Case("n5_c1_singular", 5, 1, 8)


def no_enabled_case():
    c = Case("n24_c40_none_enabled", 24, 40, 9)
    c.last_deform_time = int(c.nodes[-1, 3])
    return c


# ---- the edges of the solver: capacity, short enabled suffixes, batches, pool sizes at chunk boundaries, one hot node, NaN ------------------
def capacity_case():
    return Case("n2048_c2048", 2048, 2048, 7)  # the solver's capacity: pool 4096


def frame_capacity_case():
    return Case("n2047_c768", 2047, 768, 7)  # the frame step's solver


def wrap_cases():
    """the sizes around which the solver's 1024-thread setup passes wrap, and one whose disabled prefix is longer than 1024 nodes"""
    ldt, kept = _suffix_time(1300, 12, 200)
    assert 190 <= kept <= 200, kept
    return [Case("n%d_c64" % n, n, 64, 12) for n in (1023, 1024, 1025)] + [
        Case("n1300_c64_nopins_suffix%d" % kept, 1300, 64, 12, pins=False, last_deform_time=ldt)]


# shift per suffix length: the one of (0.05, 1, 3, 20, 40) that stays 1 % clear of every exit threshold and runs the most iterations
SUFFIX_SHIFT = {1: 0.05, 2: 0.05, 4: 40.0, 5: 40.0, 18: 20.0, 19: 20.0, 20: 20.0, 21: 20.0, 22: 20.0, 41: 20.0, 63: 20.0}


def suffix_cases():
    """64 nodes, 96 constraints, exactly E enabled nodes at the end of the graph, with and without pins"""
    out = []
    for e, shift in SUFFIX_SHIFT.items():
        ldt, kept = _suffix_time(64, 21, e)
        assert kept == e, (e, kept)
        for pins in (True, False):
            out.append(Case("n64_c96_suffix%d_%s" % (e, "pins" if pins else "nopins"), 64, 96, 21, pins=pins, last_deform_time=ldt, shift=shift))
    return out + [dense_suffix_case(e, seed) for e, seed in ((19, 25), (20, 23), (21, 24), (22, 23))]


def dense_suffix_case(e, seed):
    """The last 64 nodes of a 2048-node path: they lie closer together than their noise, so a vertex's four nearest of the 20 in its
    window are up to 19 nodes apart and the normal matrix fills the whole band (on make_nodes(64, .) they are neighbours and the band
    is 5 blocks wide).  Unpinned, exactly e enabled nodes, shift 20: three iterations, 2 % clear or better."""
    c = Case("n64_c96_dense_suffix%d_nopins" % e, 64, 4, seed, pins=False, shift=20.0)
    c.nodes = make_nodes(2048, seed)[-64:]
    t = c.nodes[:, 3]
    assert t[64 - e - 1] < t[64 - e], (e, seed)
    c.rows = make_rows(c.nodes[44:], 96, seed, 20.0)
    c.last_deform_time = int(t[64 - e - 1])
    c.src_time = c.time = int(t[-1]) + 1
    return c


def suffix_case(e, pins=True):
    return [c for c in suffix_cases() if c.name == "n64_c96_suffix%d_%s" % (e, "pins" if pins else "nopins")][0]


class BatchCase(Case):
    """Constraints added in several calls: sizes[i] rows with pin flag pin_flags[i] and source time src_times[i]"""

    def __init__(self, name, n, sizes, pin_flags, src_offsets, seed, shift=1.0):
        Case.__init__(self, name, n, sum(sizes), seed, pins=None, shift=shift)
        cuts = np.cumsum([0] + list(sizes))
        self._batches = [(self.rows[a:b], self.src_time + off, bool(pin)) for a, b, pin, off in zip(cuts[:-1], cuts[1:], pin_flags, src_offsets)]

    @property
    def batches(self):
        return self._batches


def batch_case():
    """four calls with mixed pin flags and two source times"""
    return BatchCase("n45_batches_30p_17_1p_50", 45, (30, 17, 1, 50), (True, False, True, False), (0, -7, -7, 0), 13, shift=20.0)


def boundary_cases():
    """pools at the wave (64) and chunk (256) boundaries of the assembly's compaction"""
    out = [Case("n45_pool%d_nopins" % m, 45, m, 14, pins=False, shift=3.0) for m in (63, 64, 65, 255, 256, 257)]
    return out + [Case("n45_pool%d_pins" % (2 * m), 45, m, 14, shift=3.0) for m in (128, 129)]


def hot_node_case(m):
    """m pinned constraints whose sources lie within 2 mm of node 60 of 64: the sources (of the closing frame's time, so
    weighted among the last 20 nodes) all touch the same four nodes"""
    c = Case("n64_c%d_hot_node" % m, 64, 4, 15)
    rng = np.random.default_rng(15 + m)
    d = rng.normal(size=(m, 3))
    d *= (0.002 * rng.random(size=(m, 1)) ** (1 / 3)) / np.linalg.norm(d, axis=1, keepdims=True)
    src = c.nodes[60, :3].astype(np.float64) + d
    tgt = src + np.array([0.02, -0.01, 0.015])
    c.rows = np.concatenate([src, tgt, np.full((m, 1), c.nodes[2, 3])], 1).astype(np.float32)  # the pins are weighted among the first nodes
    return c


def single_unpinned_case():
    return Case("n24_c1_nopins", 24, 1, 16, pins=False)


def poisoned_case(value):
    """64 nodes, 40 pinned constraints at the full staged shift (40); one more, added in a call of its own with a source time in the
    middle of the graph, has `value` (NaN or Inf) as its source x: the normal matrix is poisoned around block 30"""
    c = BatchCase("n64_c40_%s_mid_graph" % ("nan" if np.isnan(value) else "inf"), 64, (39, 1), (True, True), (0, 0), 17, shift=40.0)
    rows, _, _ = c._batches[1]
    rows = rows.copy()
    rows[0, 0] = value
    rows[0, 6] = c.nodes[30, 3]
    c._batches[1] = (rows, int(c.nodes[30, 3]), True)
    c.rows = np.concatenate([c._batches[0][0], rows])
    return c


def relax_case():
    c = staged_cases()[4]
    c.name += "_relax"
    c.relax = True
    return c


def time_edge_vertices(nodes4, seed=11):
    """Vertices (xyz, time) whose times lie before the first node, after the last, and on a run of equal node times"""
    rng = np.random.default_rng(seed)
    t = nodes4[:, 3].astype(np.int64)
    runs = [int(v) for v in np.unique(t) if (t == v).sum() >= 2]
    assert runs, "the node times need a run of equal values"
    times = [int(t[0]) - 1, 0, int(t[-1]) + 1, int(t[-1]) + 1000] + runs[:3] + [int(t[len(t) // 2])]
    pts = nodes4[rng.integers(0, len(nodes4), size=len(times)), :3] + rng.normal(size=(len(times), 3)).astype(np.float32) * 0.1
    return pts.astype(np.float32), np.array(times, np.int64)


def ulps(a, b):
    """distance in float32 steps between two arrays"""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))
