"""One SHA-256 per case over everything the two deformation solvers give back, to hold two builds of the library against each other
bit for bit (DMS_LIB_PATH selects the other build, as for scripts/ab_lib.sh): the lines of two builds that compute the same are equal.

  band      tests/deform_cases.py: the staged cases, the capacity case (2048 nodes, pool of 4096), and the inputs whose factorisation
            fails: the single unpinned constraint, the 5-node one, a NaN and an Inf in the middle of the graph
  global    tests/deform_global_cases.py: the staged cases, one input per exit, the capacity case (e), and a single unpinned
            constraint, which is singular in the row-envelope solver

Hashed, in this order: the result block; first residual, first Jacobian (indptr, columns, values), first delta; node table, pool;
band: the new relative constraints and lastDeformTime; global: the poses, the kept rotations and the envelope's `first`.

    python scripts/deform_bits.py
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def digest(parts):
    h = hashlib.sha256()
    for p in parts:
        h.update(p if isinstance(p, bytes) else np.ascontiguousarray(p).tobytes())
    return h.hexdigest()


def band_line(d, c):
    d.setNodes(c.nodes)
    d.setLastDeformTime(c.last_deform_time)
    d.clearConstraints()
    for rows, src_time, pin in c.batches:
        d.addConstraints(rows, src_time, pin)
    d.constrain(c.time, c.relax)
    r = d.result()
    return r, digest([bytes(r), d.firstResidual(), *d.firstJacobian(), d.firstDelta(), d.graph(), d.pool(), d.relativeConstraints(),
                      np.int64(d.lastDeformTime())])


def global_line(d, c):
    d.setNodes(c.nodes)
    d.clearConstraints()
    for call in c.calls:
        d.addConstraints(call[1], call[2], call[3]) if call[0] == "abs" else d.addRelativeConstraints(call[1])
    d.setPoses(c.pose_times, c.poses)
    d.constrainGlobal(c.tick)
    r = d.result()
    return r, digest([bytes(r), d.firstResidual(), *d.firstJacobian(), d.firstDelta(), d.graph(), d.pool(), d.poses()[1],
                      np.int32(d.keptRotations()), d.envelope()])


def main():
    from densemonoslam_amd import capi, deform
    from tests import deform_cases as DC, deform_global_cases as GC

    assert capi.device_count() >= 1, "needs a GPU"
    band = DC.staged_cases() + [DC.capacity_case(), DC.single_unpinned_case(), DC.singular_case(), DC.poisoned_case(np.nan), DC.poisoned_case(np.inf)]
    d = deform.Deformation()
    for c in band:
        r, sha = band_line(d, c)
        print("band   %-32s status %d iterations %d exit %d  %s" % (c.name, r.status, r.iterations, r.exit_reason, sha), flush=True)
    d.close()
    lone = GC.GCase("g_n24_c1_nopins", 24, 16, lambda c: [GC._abs(c, 1, 16, 8.0, pin=False)])
    d = deform.GlobalDeformation(max_nodes=410, max_constraints=2048, max_relative=16, max_poses=16)
    for c in GC.staged_cases() + [c for c, _, _ in GC.exit_cases()] + [GC.case_e(), lone]:
        r, sha = global_line(d, c)
        print("global %-32s status %d iterations %d exit %d  %s" % (c.name, r.status, r.iterations, r.exit_reason, sha), flush=True)
    d.close()


if __name__ == "__main__":
    main()
