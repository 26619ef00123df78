"""Crafted inputs for the global deformation object (tests/test_deform_global_cpu.py, tests/test_deform_global_gpu.py): the graphs of
tests/deform_cases.py (a camera path that returns to its start) with relative constraints between chosen nodes' times, absolute rows with
pins, and poses.  A relative row {src, tgt, srcTime, targetTime} says that the point seen at src at srcTime is the point seen at tgt at
targetTime: the two lie a few millimetres apart and are weighted among the nodes around their own times."""
import numpy as np

from tests import deform_cases as DC, deform_ref as R


def rel_row(nodes, a, b, seed, gap=0.002, spread=0.05):
    """a point beside node a at node a's time, and the same point `gap` metres off at node b's time"""
    rng = np.random.default_rng(7000 + seed)
    src = nodes[a, :3].astype(np.float64) + rng.normal(size=3) * spread
    tgt = src + rng.normal(size=3) * gap
    return np.concatenate([src, tgt, [nodes[a, 3], nodes[b, 3]]]).astype(np.float32)


def make_poses(nodes, times, seed):
    """one pose per time: beside the node nearest in time, a small rotation about a random axis"""
    rng = np.random.default_rng(9000 + seed)
    out = np.tile(np.eye(4, dtype=np.float32), (len(times), 1, 1))
    for i, t in enumerate(times):
        near = int(np.abs(nodes[:, 3].astype(np.int64) - int(t)).argmin())
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        a = rng.uniform(-0.5, 0.5)
        Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        out[i, :3, :3] = np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx
        out[i, :3, 3] = nodes[near, :3] + rng.normal(size=3) * 0.1
    return out


def pose_times(nodes):
    """(g): before the first node, between two node times, after the last, and exact ties (one on a run of equal times where there is one)"""
    t = nodes[:, 3].astype(np.int64)
    gaps = [int(a) + 1 for a, b in zip(t[:-1], t[1:]) if b - a >= 2]
    runs = [int(v) for v in np.unique(t) if (t == v).sum() >= 2]
    return np.array([0, int(t[0]) - 1] + gaps[:2] + [int(t[-1]) + 1, int(t[-1]) + 500, int(t[len(t) // 2])] + runs[:1], np.int64)


class GCase:
    """name; nodes; calls in order, ("abs", rows7, srcTime, pin) or ("rel", rows8); poses"""

    def __init__(self, name, n, seed, calls, nodes=None):
        self.name = name
        self.nodes = DC.make_nodes(n, seed) if nodes is None else nodes
        self.tick = int(self.nodes[-1, 3]) + 1
        self.calls = calls(self)
        self.pose_times = pose_times(self.nodes)
        self.poses = make_poses(self.nodes, self.pose_times, seed)

    @property
    def relative_rows(self):
        return sum(len(np.reshape(c[1], (-1, 8))) for c in self.calls if c[0] == "rel")

    @property
    def absolute_rows(self):
        return sum(len(np.reshape(c[1], (-1, 7))) for c in self.calls if c[0] == "abs")

    def __repr__(self):
        return self.name


def _abs(c, m, seed, shift, pin=True):
    return ("abs", DC.make_rows(c.nodes, m, seed, shift), c.tick, pin)


def _rels(c, pairs, seed, gap=0.002):
    return ("rel", np.stack([rel_row(c.nodes, a, b, seed + i, gap) for i, (a, b) in enumerate(pairs)]))


def _closing(c, absolute, pairs, seed, gap=0.0005):
    """Relative rows that agree with the closure the absolute rows ask for, as the rows kept from earlier closures do: the graph is
    solved for the absolute rows alone (tests/deform_ref.py), and each target is moved (four rounds of a fixed-point step) until the
    deformation at its own time takes it where the deformation at the source's time takes the source, up to `gap`."""
    nodes = c.nodes.copy()
    nodes[:, 3] = np.maximum(nodes[:, 3], 1)  # every node enabled, as with lastDeformTime = 0 and times from 1 on
    g = R.constrain_batches(nodes, [(a[1], a[2], a[3]) for a in absolute], c.tick, True, 0)["graph"]
    g.times = c.nodes[:, 3].astype(np.int64)
    rows = _rels(c, pairs, seed, gap)[1]
    for r in rows:
        off = r[3:6] - r[0:3]
        want = R.vertex_position(g, r[0:3], *R.weigh_vertex(g, r[0:3], int(r[6])))
        tgt = r[0:3].copy()
        for _ in range(4):
            tgt = tgt + (want - R.vertex_position(g, tgt, *R.weigh_vertex(g, tgt, int(r[7]))))
        r[3:6] = tgt + off
    return ("rel", rows)


# (c): spans (later node, earlier node).  40 -> 12 comes first; 52 -> 4 begins left of it (nested around it), 58 -> 30 crosses it,
# 35 -> 20 lies inside, 62 -> 0 spans everything.  Rows 45 .. 48 lie behind the tall rows around 40 and are narrow.
SPANS_C = [(40, 12), (52, 4), (58, 30), (35, 20), (62, 0)]
DISABLED_D = 30  # (d): nodes 0 .. 29 have time 0


def _nodes_d():
    nodes = DC.make_nodes(64, 34)
    nodes[:DISABLED_D, 3] = 0
    return nodes


def _closed(m, seed, shift, pairs, gap=0.0005):
    def calls(c):
        a = _abs(c, m, seed, shift)
        return [a, _closing(c, [a], pairs, seed, gap)]
    return calls


def case_a():
    return GCase("a_n5_shared_nodes", 5, 31, _closed(3, 31, 8.0, [(4, 0)]))


def case_b():
    return GCase("b_n24_first_to_last", 24, 32, _closed(12, 32, 8.0, [(23, 0)]))


def case_c():
    def calls(c):
        a = _abs(c, 40, 33, 8.0)
        b = ("abs", a[1][:8], c.tick, False)  # the first eight rows again, unpinned
        rel = _closing(c, [a, b], SPANS_C, 33)[1]
        return [a, ("rel", rel[:3]), b, ("rel", rel[3:])]
    return GCase("c_n64_crossing_spans", 64, 33, calls)


def case_d():
    # relative rows: source among the disabled nodes and target among the enabled; all eight nodes disabled (no row); both enabled
    return GCase("d_n64_disabled_prefix", 64, 34, lambda c: [_abs(c, 24, 34, 8.0), _rels(c, [(2, 50), (3, 5), (60, 40)], 34)], nodes=_nodes_d())


def case_e():
    """capacity: 410 nodes, 2048 rows with pins, relative rows between the two ends that agree with the closure, so that the solve is
    accepted and table, pool and poses are written at this size too"""
    return GCase("e_n410_c2048_r8", 410, 35, _closed(2048, 35, 8.0, [(409 - 3 * i, 2 * i) for i in range(8)]))


def staged_cases():
    return [case_a(), case_b(), case_c(), case_d()]


# ---- (f) one input per exit -------------------------------------------------------------------------------------------------------------
def exit_cases():
    """name -> (case, exit reason, applied) as the restatement must find them (tests/test_deform_global_cpu.py asserts it)"""
    met = GCase("f_constraints_met", 24, 36, lambda c: [_abs(c, 12, 36, 1.0), _rels(c, [(23, 0)], 36)])
    large = GCase("f_error_large", 24, 37, lambda c: [_abs(c, 30, 37, 120.0, pin=False), _rels(c, [(23, 0)], 37, gap=0.5)])
    big_error = GCase("f_rejected_by_error", 64, 38, _closed(40, 38, 8.0, [(63, 0), (60, 3)], gap=0.05))
    def conflicting(c):
        c.calls_so_far = _closed(40, 39, 8.0, [(63, 0)])(c)
        return c.calls_so_far + [_conflict(c, 39)]
    cons = GCase("f_rejected_by_mean_cons_err", 64, 39, conflicting)
    accepted = GCase("f_accepted", 64, 40, _closed(40, 40, 8.0, [(63, 0)]))
    return [(met, 6, False), (large, 7, False), (big_error, None, False), (cons, None, False), (accepted, None, True)]


def _conflict(c, seed):
    """ten of the case's rows twice, unpinned, the copies' targets 8 mm off: no graph meets both, the residual stays small"""
    rows = c.calls_so_far[0][1][:10]
    other = rows.copy()
    other[:, 3] += 0.008
    return ("abs", np.concatenate([rows, other]), c.tick, False)
