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
