/*
 * dmslam_deform.h — C ABI of the deformation-graph solver: Deformation::constrain (Core/src/Deformation.cpp:91-220) with
 * DeformationGraph::optimiseGraphSparse (Core/src/Utils/DeformationGraph.cpp:457-535) for ABSOLUTE and PIN constraints with
 * fernMatch = false, on the GPU: graph construction (k = 4), vertex weighting, the three-iteration Gauss-Newton loop with its
 * exit tests, applyGraphToVertices, the new relative-constraint rows and the 16-float node table dms_model_clean takes.  Where the
 * reference hands J and r to CHOLMOD, A = J^T J and g = -J^T r are assembled in fp64 into block-band storage (12 x 12 blocks,
 * block half-bandwidth 19: a property of the problem) and solved by a banded block Cholesky.  Every sum has a fixed
 * order and no floating-point atomic is used: the same input gives the same bits on every run.  Row and weight arithmetic is
 * csrc/deform_rows.hpp, which states the order rules; tests/deform_ref.py is the CPU restatement the results are held against.
 *
 * Not here (the caller's solver, through dms_fusion_process_frame_begin / _end as before): relative constraints, fernMatch = true,
 * applyGraphToPoses.
 *
 * EDGE RULES
 *   no enabled node (every node's time <= lastDeformTime)   zero delta, the table of the untouched nodes, applied = 1, exit reason
 *                                                           DMS_DEFORM_EXIT_NO_ENABLED_NODE, no iteration
 *   singular system (a pivot of the factorisation at or     status DMS_DEFORM_SINGULAR, the graph is reset (identity rotations, zero
 *     below 2^-40 of its diagonal entry, NaN included)      translations), applied = 0, no NaN in the table.  (The reference would
 *                                                           hand CHOLMOD a matrix it cannot factor.)
 *   no graph yet (never more than 4 nodes given)            status DMS_DEFORM_NO_GRAPH, applied = 0 (Deformation.cpp:99)
 *   more nodes or constraints than the object was made for  DMS_ERR_CAPACITY, before any launch
 *   a relative constraint                                   DMS_ERR_INVALID_ARG
 *
 * All device pointers are HBM of the current device.  Calls on one object are ordered by the caller (one stream, or events).
 */
#ifndef DMSLAM_DEFORM_H_
#define DMSLAM_DEFORM_H_

#include "dmslam.h"
#include "dmslam_fusion.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dms_deform dms_deform;

#define DMS_DEFORM_MAX_NODES 2048       /* the reference's transform-feedback buffer, Deformation.cpp:27 */
#define DMS_DEFORM_MAX_CONSTRAINTS 2048 /* constraint rows per solve, pins not counted */

enum { DMS_DEFORM_OK = 0, DMS_DEFORM_SINGULAR = 1, DMS_DEFORM_NO_GRAPH = 2 };
/* which test of DeformationGraph.cpp:515 ended the loop (in the order it evaluates them); 0: all three iterations ran */
enum {
  DMS_DEFORM_EXIT_ITERATIONS = 0,
  DMS_DEFORM_EXIT_ERROR_GREW = 1,
  DMS_DEFORM_EXIT_SMALL_DELTA = 2,
  DMS_DEFORM_EXIT_SMALL_ERROR = 3,
  DMS_DEFORM_EXIT_SMALL_CHANGE = 4,
  DMS_DEFORM_EXIT_NO_ENABLED_NODE = 5
};

typedef struct dms_deform_result {
  int applied;       /* Deformation::constrain's return value */
  int optimised;     /* optimiseGraphSparse's */
  int status;        /* DMS_DEFORM_OK / _SINGULAR / _NO_GRAPH */
  int iterations;    /* Gauss-Newton iterations run (0..3) */
  int exit_reason;   /* DMS_DEFORM_EXIT_* */
  int nodes;         /* nodes of the graph */
  int enabled_nodes; /* nodes newer than lastDeformTime: 12 unknowns each */
  int constraints;   /* constraints solved for, pins included */
  int rows;          /* rows of the residual */
  int relative_rows; /* rows dms_deform_get_relative_constraints has */
  float error;       /* `error` of Deformation.cpp:159: the last squared residual norm */
  float error_initial;
  float mean_cons_err_before; /* nonRelativeConstraintError before the loop (:463) ... */
  float mean_cons_err_after;  /* ... and after (:530); of the reset graph when the system was singular */
  double iter_error[3];       /* per iteration: `error` as double, delta.norm() */
  double iter_delta_norm[3];
  long long last_deform_time; /* after this solve (Deformation.cpp:203-206) */
} dms_deform_result;

/* max_nodes in [5, DMS_DEFORM_MAX_NODES], max_constraints in [1, DMS_DEFORM_MAX_CONSTRAINTS] (rows; each may carry a pin). */
int dms_deform_create(dms_deform** out, int max_nodes, int max_constraints);
int dms_deform_destroy(dms_deform* d);

/* DeformationGraph::initialiseGraph (:56-91): n rows {x, y, z, time} in device memory, sorted by time (what
 * dms_model_sample_graph yields); rotations become the identity, translations zero.  n >= 5 (Deformation.cpp:311), else
 * DMS_ERR_INVALID_ARG; n > max_nodes: DMS_ERR_CAPACITY. */
int dms_deform_set_nodes(dms_deform* d, const float* rows4_dev, int n, dms_stream s);
/* The device-resident form of dms_model_sample_graph (Deformation::sampleGraphModel, Deformation.cpp:250-348): every sampleRate-th
 * surfel, at most max_nodes of them (the first in surfel order: GL stops writing at the end of the reference's buffer), stable sort
 * by init time, rows left in this object's node buffer and the count on the device.  The graph is replaced only when more than 4
 * samples were taken (:311).  Not while a fuse's deferred update pass is pending on the map; does not synchronise. */
int dms_deform_sample_model(dms_deform* d, dms_model* m, int sampleRate, dms_stream s);

/* Deformation::addConstraint (Deformation.cpp:76-89) for n device rows {source xyz, target xyz, target time} (the layout of
 * dms_fusion_get_loop_constraints) with the source time; pin != 0 adds each row's pin {target, target, target time} behind it.
 * relative != 0: DMS_ERR_INVALID_ARG.  More rows than max_constraints in all: DMS_ERR_CAPACITY, nothing added. */
int dms_deform_add_constraints(dms_deform* d, const float* rows7_dev, int n, int srcTime, int pin, int relative, dms_stream s);
int dms_deform_clear_constraints(dms_deform* d);

/* Deformation::constrain(..., time, fernMatch = false, ..., relaxGraph, &newRelativeCons): enqueues the whole solve on `s` and
 * returns; the three iterations run without the host.  The constraints are consumed (cleared) as the reference's are. */
int dms_deform_constrain(dms_deform* d, int time, int relaxGraph, dms_stream s);
/* Waits for the last dms_deform_constrain and copies its status block. */
int dms_deform_get_result(dms_deform* d, dms_deform_result* out);
/* The node table in device memory, 16 floats per node (position, rotation column-major, translation, time: Deformation.cpp:192-201)
 * as dms_model_clean takes it from the host, and the device word that holds the node count.  Valid after a dms_deform_constrain on
 * the stream it ran on. */
int dms_deform_graph_device(dms_deform* d, const float** table16_dev, const int** node_count_dev);
/* newRelativeCons (Deformation.cpp:171-187) of the last applied solve: rows {deformed source xyz, target xyz, source time, target
 * time}, one per constraint that is not a pin.  Copies min(*n, max_rows) rows of 8 floats; synchronises. */
int dms_deform_get_relative_constraints(dms_deform* d, float* rows8_host, int max_rows, int* n);
/* lastDeformTime (Deformation.cpp:32, :203-206); the getter waits for the last solve, the setter synchronises the device. */
int dms_deform_last_deform_time(dms_deform* d, long long* t);
int dms_deform_set_last_deform_time(dms_deform* d, long long t);

/* Intermediate state of the last solve, for tests (host destinations; each synchronises).  Vertices are the pool of the solve: a
 * constraint's source, then its pin's.  Counts come back in *n (and *nnz); at most max_* entries are copied. */
int dms_deform_get_vertex_weights(dms_deform* d, int* ids4_host, double* weights4_host, int max_vertices, int* n);
int dms_deform_get_first_residual(dms_deform* d, double* r_host, int max_rows, int* n);
int dms_deform_get_first_jacobian(dms_deform* d, int* indptr_host, int* cols_host, double* vals_host, int max_rows, int max_nnz, int* n,
                                  int* nnz);
int dms_deform_get_first_delta(dms_deform* d, double* delta_host, int max_unknowns, int* n);
/* the pool after applyGraphToVertices (Deformation.cpp:169): xyz per vertex */
int dms_deform_get_pool(dms_deform* d, float* xyz_host, int max_vertices, int* n);

/* ---- the frame step closes its local loops itself --------------------------------------------------------------------------------
 * With the solver on and local_loop_closure = 1, dms_fusion_process_frame does what ElasticFusion.cpp:441-493 does: after the loop
 * candidate the host reads the frame's loop_ok word (one mid-frame synchronisation, as the NID gate and --rl have and as the reference
 * has); when the loop is accepted the graph is sampled from the map as it stands (every sampleRate-th surfel; 0 = 5000,
 * Options::defGraphSampleRate), the constraints go from the frame's own device buffer into the solver (pinned while deforms == 0) and
 * the solve is enqueued; the host reads its status and node count (closing frames only); the fusion half then runs as
 * dms_fusion_process_frame_end(graph, nodes, estPose) does, with the table taken from device memory; deforms and lastDeformTime
 * advance and every (size / 3)-th new relative constraint (a step of at least 1) is kept.  If the solve was not applied the frame ends
 * as an unaccepted loop does.  Off by default; with it off nothing changes.  The two-phase calls are not affected by the switch.
 * DMS_ERR_INVALID_ARG when switched on for a context without local_loop_closure, whose map is shared by several cameras, which uses
 * clusters, or whose frames give more than DMS_DEFORM_MAX_CONSTRAINTS constraint samples (W/20 x H/20).  Between frames only. */
int dms_fusion_set_loop_solver(dms_fusion* f, int on, int sampleRate);
/* the solver of this context (NULL until it was first switched on): its result, graph and intermediate state of the last closing frame */
dms_deform* dms_fusion_deformation(dms_fusion* f);
/* ElasticFusion::deforms: the frames whose loop was closed so far */
int dms_fusion_get_deforms(dms_fusion* f);
/* context.relativeCons(): the kept rows {deformed source xyz, target xyz, source time, target time} of all closing frames so far */
int dms_fusion_get_relative_constraints(dms_fusion* f, float* rows8_host, int max_rows, int* n);

#ifdef __cplusplus
}
#endif
#endif /* DMSLAM_DEFORM_H_ */
