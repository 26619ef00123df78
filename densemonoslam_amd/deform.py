"""ctypes mirror of the deformation-graph solver (reference class Deformation with DeformationGraph, Core/src/Deformation.h) —
include/dmslam_deform.h.  Deformation: absolute and pin constraints, fernMatch = false.  GlobalDeformation: also relative constraints,
fernMatch = true and the poses."""
import ctypes as C

import numpy as np

from .capi import DeviceBuffer, check, lib

MAX_NODES = 2048
MAX_CONSTRAINTS = 2048
OK, SINGULAR, NO_GRAPH = 0, 1, 2
EXIT_ITERATIONS, EXIT_ERROR_GREW, EXIT_SMALL_DELTA, EXIT_SMALL_ERROR, EXIT_SMALL_CHANGE, EXIT_NO_ENABLED_NODE = range(6)
_P, _I = C.c_void_p, C.c_int
_IP, _FP, _DP = C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_double)


class DeformResult(C.Structure):
    _fields_ = [("applied", _I), ("optimised", _I), ("status", _I), ("iterations", _I), ("exit_reason", _I), ("nodes", _I),
                ("enabled_nodes", _I), ("constraints", _I), ("rows", _I), ("relative_rows", _I), ("error", C.c_float),
                ("error_initial", C.c_float), ("mean_cons_err_before", C.c_float), ("mean_cons_err_after", C.c_float),
                ("iter_error", C.c_double * 3), ("iter_delta_norm", C.c_double * 3), ("last_deform_time", C.c_longlong)]


lib.dms_deform_create.argtypes = [C.POINTER(_P), _I, _I]
lib.dms_deform_destroy.argtypes = [_P]
lib.dms_deform_set_nodes.argtypes = [_P, _P, _I, _P]
lib.dms_deform_sample_model.argtypes = [_P, _P, _I, _P]
lib.dms_deform_add_constraints.argtypes = [_P, _P, _I, _I, _I, _I, _P]
lib.dms_deform_clear_constraints.argtypes = [_P]
lib.dms_deform_constrain.argtypes = [_P, _I, _I, _P]
lib.dms_deform_get_result.argtypes = [_P, C.POINTER(DeformResult)]
lib.dms_deform_graph_device.argtypes = [_P, C.POINTER(_P), C.POINTER(_P)]
lib.dms_deform_get_relative_constraints.argtypes = [_P, _FP, _I, _IP]
lib.dms_deform_last_deform_time.argtypes = [_P, C.POINTER(C.c_longlong)]
lib.dms_deform_set_last_deform_time.argtypes = [_P, C.c_longlong]
lib.dms_deform_get_vertex_weights.argtypes = [_P, _IP, _DP, _I, _IP]
lib.dms_deform_get_first_residual.argtypes = [_P, _DP, _I, _IP]
lib.dms_deform_get_first_jacobian.argtypes = [_P, _IP, _IP, _DP, _I, _I, _IP, _IP]
lib.dms_deform_get_first_delta.argtypes = [_P, _DP, _I, _IP]
lib.dms_deform_get_pool.argtypes = [_P, _FP, _I, _IP]


class Deformation:
    """A solver for graphs of up to max_nodes nodes and max_constraints constraint rows (each may carry a pin)."""

    def __init__(self, max_nodes=MAX_NODES, max_constraints=MAX_CONSTRAINTS):
        self.max_nodes, self.max_constraints = int(max_nodes), int(max_constraints)
        h = _P()
        check(lib.dms_deform_create(C.byref(h), self.max_nodes, self.max_constraints), "dms_deform_create")
        self.h = h
        self._keep = []

    @classmethod
    def view(cls, handle, max_constraints, max_nodes=MAX_NODES):
        """A non-owning mirror of a solver that belongs to a frame context (fusion.ElasticFusion.deformation)"""
        d = cls.__new__(cls)
        d.max_nodes, d.max_constraints, d.h, d._keep, d._owned = int(max_nodes), int(max_constraints), _P(handle), [], False
        return d

    def close(self):
        if getattr(self, "h", None) and getattr(self, "_owned", True):
            lib.dms_deform_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- the graph --------------------------------------------------------------------------------------------------------------
    def setNodesDevice(self, rows4_ptr, n, stream=None):
        check(lib.dms_deform_set_nodes(self.h, _P(rows4_ptr), int(n), _P(stream)), "dms_deform_set_nodes")

    def setNodes(self, rows4, stream=None):
        """n x 4 float32 {x, y, z, time}, sorted by time (GlobalModel.sampleGraph's)"""
        rows4 = np.ascontiguousarray(rows4, np.float32).reshape(-1, 4)
        buf = DeviceBuffer(max(16, rows4.nbytes)).upload(rows4, stream)
        self._keep = [buf]
        self.setNodesDevice(buf.ptr, len(rows4), stream)
        check(lib.dms_stream_sync(_P(stream)), "dms_stream_sync")

    def sampleModel(self, model, sampleRate=5000, stream=None):
        """Deformation::sampleGraphModel on the device: `model` is a fusion.GlobalModel (or its handle)"""
        check(lib.dms_deform_sample_model(self.h, getattr(model, "h", model), int(sampleRate), _P(stream)), "dms_deform_sample_model")

    # ---- constraints ------------------------------------------------------------------------------------------------------------
    def addConstraintsDevice(self, rows7_ptr, n, srcTime, pin, relative=False, stream=None):
        check(lib.dms_deform_add_constraints(self.h, _P(rows7_ptr), int(n), int(srcTime), int(bool(pin)), int(bool(relative)), _P(stream)),
              "dms_deform_add_constraints")

    def addConstraints(self, rows7, srcTime, pin, relative=False, stream=None):
        """n x 7 float32 {source xyz, target xyz, target time}: ElasticFusion.loopConstraints()'s rows"""
        rows7 = np.ascontiguousarray(rows7, np.float32).reshape(-1, 7)
        buf = DeviceBuffer(max(16, rows7.nbytes)).upload(rows7, stream)
        self.addConstraintsDevice(buf.ptr, len(rows7), srcTime, pin, relative, stream)
        check(lib.dms_stream_sync(_P(stream)), "dms_stream_sync")

    def clearConstraints(self):
        check(lib.dms_deform_clear_constraints(self.h), "dms_deform_clear_constraints")

    # ---- the solve --------------------------------------------------------------------------------------------------------------
    def constrain(self, time, relaxGraph=False, stream=None):
        """Enqueues Deformation::constrain; result() waits for it."""
        check(lib.dms_deform_constrain(self.h, int(time), int(bool(relaxGraph)), _P(stream)), "dms_deform_constrain")

    def result(self):
        r = DeformResult()
        check(lib.dms_deform_get_result(self.h, C.byref(r)), "dms_deform_get_result")
        return r

    def graphDevice(self):
        """(device pointer of the 16-float node table, device pointer of the node count)"""
        t, n = _P(), _P()
        check(lib.dms_deform_graph_device(self.h, C.byref(t), C.byref(n)), "dms_deform_graph_device")
        return t.value, n.value

    def graph(self):
        """The node table on the host: nodes x 16 float32, as GlobalModel.clean / processFrameEnd take it"""
        r = self.result()
        out = np.zeros((r.nodes, 16), np.float32)
        if r.nodes:
            t, _ = self.graphDevice()
            check(lib.dms_memcpy_d2h(out.ctypes.data_as(_P), _P(t), C.c_size_t(out.nbytes), None), "dms_memcpy_d2h")
        return out

    def relativeConstraints(self):
        n = _I(0)
        out = np.zeros((self.max_constraints, 8), np.float32)
        check(lib.dms_deform_get_relative_constraints(self.h, out.ctypes.data_as(_FP), len(out), C.byref(n)), "dms_deform_get_relative_constraints")
        return out[:n.value].copy()

    def lastDeformTime(self):
        t = C.c_longlong(0)
        check(lib.dms_deform_last_deform_time(self.h, C.byref(t)), "dms_deform_last_deform_time")
        return t.value

    def setLastDeformTime(self, t):
        check(lib.dms_deform_set_last_deform_time(self.h, int(t)), "dms_deform_set_last_deform_time")

    # ---- intermediate state of the last solve (tests) ---------------------------------------------------------------------------
    def vertexWeights(self):
        cap, n = 2 * self.max_constraints, _I(0)
        ids, w = np.zeros((cap, 4), np.int32), np.zeros((cap, 4))
        check(lib.dms_deform_get_vertex_weights(self.h, ids.ctypes.data_as(_IP), w.ctypes.data_as(_DP), cap, C.byref(n)), "dms_deform_get_vertex_weights")
        return ids[:n.value].copy(), w[:n.value].copy()

    def firstResidual(self):
        cap, n = 18 * self.max_nodes + 6 * self.max_constraints, _I(0)
        r = np.zeros(cap)
        check(lib.dms_deform_get_first_residual(self.h, r.ctypes.data_as(_DP), cap, C.byref(n)), "dms_deform_get_first_residual")
        return r[:n.value].copy()

    def firstJacobian(self):
        """(indptr, columns, values): CSR, columns counted from the first enabled node's first unknown"""
        rows, nnz = 18 * self.max_nodes + 6 * self.max_constraints, 87 * self.max_nodes + 96 * self.max_constraints
        indptr, cols, vals = np.zeros(rows + 1, np.int32), np.zeros(nnz, np.int32), np.zeros(nnz)
        n, z = _I(0), _I(0)
        check(lib.dms_deform_get_first_jacobian(self.h, indptr.ctypes.data_as(_IP), cols.ctypes.data_as(_IP), vals.ctypes.data_as(_DP), rows, nnz,
                                                C.byref(n), C.byref(z)), "dms_deform_get_first_jacobian")
        return indptr[:n.value + 1].copy(), cols[:z.value].copy(), vals[:z.value].copy()

    def firstDelta(self):
        cap, n = 12 * self.max_nodes, _I(0)
        x = np.zeros(cap)
        check(lib.dms_deform_get_first_delta(self.h, x.ctypes.data_as(_DP), cap, C.byref(n)), "dms_deform_get_first_delta")
        return x[:n.value].copy()

    def pool(self):
        cap, n = 2 * self.max_constraints, _I(0)
        x = np.zeros((cap, 3), np.float32)
        check(lib.dms_deform_get_pool(self.h, x.ctypes.data_as(_FP), cap, C.byref(n)), "dms_deform_get_pool")
        return x[:n.value].copy()


# ---- rf.globalDeformation(): relative constraints, fernMatch = true, the poses ------------------------------------------------------------
MAX_GLOBAL_NODES = 410
MAX_RELATIVE = 2048
EXIT_CONSTRAINTS_MET, EXIT_ERROR_LARGE = 6, 7
_LP = C.POINTER(C.c_longlong)
lib.dms_deform_create_global.argtypes = [C.POINTER(_P), _I, _I, _I, _I]
lib.dms_deform_sample_from.argtypes = [_P, _P, _P]
lib.dms_deform_add_relative_constraints.argtypes = [_P, _P, _I, _P]
lib.dms_deform_add_relative_constraints_host.argtypes = [_P, _FP, _I, _P]
lib.dms_deform_set_poses.argtypes = [_P, _P, _P, _I, _P]
lib.dms_deform_get_poses.argtypes = [_P, _LP, _FP, _I, _IP]
lib.dms_deform_constrain_global.argtypes = [_P, _I, _P]
lib.dms_deform_get_kept_rotations.argtypes = [_P, _IP]
lib.dms_deform_get_pose_weights.argtypes = [_P, _IP, _DP, _I, _IP]
lib.dms_deform_get_envelope.argtypes = [_P, _IP, _I, _IP]


class GlobalDeformation(Deformation):
    """The reference's globalDeformation: a Deformation that also takes relative constraints and poses and solves with fernMatch = true
    (constrainGlobal).  constrain() on it is the band solve of Deformation, for pools without relative constraints."""

    def __init__(self, max_nodes=MAX_GLOBAL_NODES, max_constraints=MAX_CONSTRAINTS, max_relative=MAX_RELATIVE, max_poses=4096):
        self.max_nodes, self.max_constraints = int(max_nodes), int(max_constraints)
        self.max_relative, self.max_poses = int(max_relative), int(max_poses)
        h = _P()
        check(lib.dms_deform_create_global(C.byref(h), self.max_nodes, self.max_constraints, self.max_relative, self.max_poses),
              "dms_deform_create_global")
        self.h = h
        self._keep = []

    def sampleFrom(self, local, stream=None):
        """Deformation::sampleGraphFrom: every 5th node of a Deformation's graph"""
        check(lib.dms_deform_sample_from(self.h, local.h, _P(stream)), "dms_deform_sample_from")

    def addRelativeConstraintsDevice(self, rows8_ptr, n, stream=None):
        check(lib.dms_deform_add_relative_constraints(self.h, _P(rows8_ptr), int(n), _P(stream)), "dms_deform_add_relative_constraints")

    def addRelativeConstraints(self, rows8, stream=None):
        """n x 8 float32 {source xyz, target xyz, source time, target time}: Deformation.relativeConstraints()'s rows"""
        rows8 = np.ascontiguousarray(rows8, np.float32).reshape(-1, 8)
        check(lib.dms_deform_add_relative_constraints_host(self.h, rows8.ctypes.data_as(_FP), len(rows8), _P(stream)),
              "dms_deform_add_relative_constraints_host")
        check(lib.dms_stream_sync(_P(stream)), "dms_stream_sync")

    def setPoses(self, times, poses, stream=None):
        """times (int64) and row-major 4 x 4 float32 poses the next constrainGlobal corrects"""
        times = np.ascontiguousarray(times, np.int64).reshape(-1)
        poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 16)
        assert len(times) == len(poses)
        tb = DeviceBuffer(max(16, times.nbytes)).upload(times, stream)
        pb = DeviceBuffer(max(16, poses.nbytes)).upload(poses, stream)
        check(lib.dms_deform_set_poses(self.h, _P(tb.ptr), _P(pb.ptr), len(times), _P(stream)), "dms_deform_set_poses")
        check(lib.dms_stream_sync(_P(stream)), "dms_stream_sync")

    def poses(self):
        n = _I(0)
        times, poses = np.zeros(self.max_poses, np.int64), np.zeros((self.max_poses, 4, 4), np.float32)
        check(lib.dms_deform_get_poses(self.h, times.ctypes.data_as(_LP), poses.ctypes.data_as(_FP), self.max_poses, C.byref(n)),
              "dms_deform_get_poses")
        return times[:n.value].copy(), poses[:n.value].copy()

    def constrainGlobal(self, time, stream=None):
        """Enqueues Deformation::constrain(..., fernMatch = true, poseGraph, relaxGraph = true); result() waits for it."""
        check(lib.dms_deform_constrain_global(self.h, int(time), _P(stream)), "dms_deform_constrain_global")

    def keptRotations(self):
        n = _I(0)
        check(lib.dms_deform_get_kept_rotations(self.h, C.byref(n)), "dms_deform_get_kept_rotations")
        return n.value

    def graph(self):
        """The node table of the last APPLIED solve (a solve that is not applied writes none)"""
        return Deformation.graph(self)

    # ---- intermediate state of the last global solve (tests) --------------------------------------------------------------------
    def vertexWeights(self):
        cap, n = 2 * self.max_constraints + 2 * self.max_relative, _I(0)
        ids, w = np.zeros((cap, 4), np.int32), np.zeros((cap, 4))
        check(lib.dms_deform_get_vertex_weights(self.h, ids.ctypes.data_as(_IP), w.ctypes.data_as(_DP), cap, C.byref(n)), "dms_deform_get_vertex_weights")
        return ids[:n.value].copy(), w[:n.value].copy()

    def firstResidual(self):
        cap, n = 18 * self.max_nodes + 6 * (self.max_constraints + self.max_relative), _I(0)
        r = np.zeros(cap)
        check(lib.dms_deform_get_first_residual(self.h, r.ctypes.data_as(_DP), cap, C.byref(n)), "dms_deform_get_first_residual")
        return r[:n.value].copy()

    def firstJacobian(self):
        rows, nnz = 18 * self.max_nodes + 6 * (self.max_constraints + self.max_relative), 87 * self.max_nodes + 96 * (self.max_constraints + self.max_relative)
        indptr, cols, vals = np.zeros(rows + 1, np.int32), np.zeros(nnz, np.int32), np.zeros(nnz)
        n, z = _I(0), _I(0)
        check(lib.dms_deform_get_first_jacobian(self.h, indptr.ctypes.data_as(_IP), cols.ctypes.data_as(_IP), vals.ctypes.data_as(_DP), rows, nnz,
                                                C.byref(n), C.byref(z)), "dms_deform_get_first_jacobian")
        return indptr[:n.value + 1].copy(), cols[:z.value].copy(), vals[:z.value].copy()

    def pool(self):
        cap, n = 2 * self.max_constraints + 2 * self.max_relative, _I(0)
        x = np.zeros((cap, 3), np.float32)
        check(lib.dms_deform_get_pool(self.h, x.ctypes.data_as(_FP), cap, C.byref(n)), "dms_deform_get_pool")
        return x[:n.value].copy()

    def poseWeights(self):
        n = _I(0)
        ids, w = np.zeros((self.max_poses, 4), np.int32), np.zeros((self.max_poses, 4))
        check(lib.dms_deform_get_pose_weights(self.h, ids.ctypes.data_as(_IP), w.ctypes.data_as(_DP), self.max_poses, C.byref(n)), "dms_deform_get_pose_weights")
        return ids[:n.value].copy(), w[:n.value].copy()

    def envelope(self):
        n = _I(0)
        first = np.zeros(self.max_nodes, np.int32)
        check(lib.dms_deform_get_envelope(self.h, first.ctypes.data_as(_IP), self.max_nodes, C.byref(n)), "dms_deform_get_envelope")
        return first[:n.value].copy()
