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
 * A second kind of object (dms_deform_create_global, at the end of this header) is rf.globalDeformation(): relative constraints,
 * fernMatch = true with its two early exits and its acceptance test, and applyGraphToPoses.  Relative constraints break the band, so
 * its factorisation is a block Cholesky over the row envelope of A.
 *
 * dms_fusion_set_global_loop_solver (last section) lets the frame step drive it: an ORB-armed frame becomes one call.
 *
 * Not here: no fern-matched closure policy (the reference compiles it out, ElasticFusion.cpp:359), no relocalisation, not several
 * cameras on one map.
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
  DMS_DEFORM_EXIT_NO_ENABLED_NODE = 5,
  /* objects of dms_deform_create_global only (fernMatch = true) */
  DMS_DEFORM_EXIT_CONSTRAINTS_MET = 6, /* meanConsErr < 0.06 before the loop (:465): optimised = 0, no iteration */
  DMS_DEFORM_EXIT_ERROR_LARGE = 7      /* error > 10 after iteration 1 (:516), the last test of :515 */
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

/* ---- rf.globalDeformation(): relative constraints, fernMatch = true, the poses -----------------------------------------------------
 * An object of dms_deform_create_global keeps every call above (dms_deform_constrain on it is the band solve, and gives a
 * dms_deform_create object's bits; not while its pool holds relative constraints: DMS_ERR_STATE) and adds the calls below.
 *
 * dms_deform_constrain_global is Deformation::constrain(..., fernMatch = true, poseGraph, relaxGraph = true): lastDeformTime is taken
 * as 0 (:161) and not advanced (:203), no newRelativeCons are made.  Enqueued whole, no host read inside.
 *   rows     a relative constraint has a row when any node of its source vertex is enabled, or else any of its target vertex
 *            (:668-680); residual (srcPos - tarPos) sqrt(wCon); Jacobian row from the two weight maps merged as csrc/deform_rows.hpp
 *            states (one entry per column where both vertices have a node).  meanConsErr sums the non-relative constraints, pins
 *            included, over the count of ALL constraints (:1011-1026).
 *   exits    DMS_DEFORM_EXIT_CONSTRAINTS_MET and _ERROR_LARGE above, besides those of the band object
 *   applied  only when optimised && meanConsErr < 0.0003 && error < 0.12 (Deformation.cpp:165).  When not applied the poses, the pool
 *            (dms_deform_get_pool then still gives the last applied solve's) and the node table are not written; the node rotations
 *            stay as the loop left them, as the reference's do, until the next dms_deform_set_nodes / _sample_from.
 *   poses    applyGraphToPoses (:102-131) with setPosesSeq's weights, one lane per pose.  U V^T of rotation * R is the orthogonal
 *            polar factor, taken in fp64 by a fixed number of Newton steps (csrc/deform_rows.hpp) and rounded to fp32 once: Eigen's
 *            fp32 Jacobi SVD cannot be pinned bit for bit; the fp64 result is closer to the exact factor than the reference's fp32
 *            rounding.  A matrix that is not finite, or whose determinant has magnitude below 2^-20, keeps the pose's old rotation
 *            and is counted (dms_deform_get_kept_rotations).
 *   solve    A = J^T J is assembled in fp64 over its row envelope (first[i] = the smallest block column any row of J couples
 *            enabled node i to) into a dense lower block triangle allocated at create time (97 MB at 410 nodes) and factored by a
 *            right-looking block Cholesky whose fill stays inside the envelope.  Fixed orders, no floating-point atomic.
 *   the singular-pivot rule and the no-graph rule are those of the EDGE RULES above. */
#define DMS_DEFORM_MAX_GLOBAL_NODES 410 /* ceil(2047 / 5): sampleGraphFrom takes every 5th node of at most 2047 */
#define DMS_DEFORM_MAX_RELATIVE 2048    /* relative constraint rows per solve (two pool vertices each) */
#define DMS_DEFORM_MAX_POSES 65536
/* max_nodes in [5, DMS_DEFORM_MAX_GLOBAL_NODES], max_constraints as above, max_relative in [0, DMS_DEFORM_MAX_RELATIVE], max_poses in
 * [0, DMS_DEFORM_MAX_POSES]. */
int dms_deform_create_global(dms_deform** out, int max_nodes, int max_constraints, int max_relative, int max_poses);
/* Deformation::sampleGraphFrom (Deformation.cpp:222-249): every 5th node row of `local` (a dms_deform_create object), counted on the
 * device; the graph is replaced (identity rotations, zero translations) only when count / 5 > 4, else kept.  A local graph that
 * gives more samples than this object was made for gives the first max_nodes of them (the rule of dms_deform_sample_model). */
int dms_deform_sample_from(dms_deform* global, dms_deform* local, dms_stream s);
/* n rows {source xyz, target xyz, source time, target time} (what dms_deform_get_relative_constraints writes), each a
 * Constraint(..., relative = true): TWO pool vertices (Deformation.cpp:131-140), source then target.  Constraints stand in the pool in
 * the order of the calls, dms_deform_add_constraints included.  More than max_relative in all: DMS_ERR_CAPACITY, nothing added. */
int dms_deform_add_relative_constraints(dms_deform* d, const float* rows8_dev, int n, dms_stream s);
/* the same from host memory (copied on `s` into the object's staging buffer; the rows may be reused once `s` has passed the call) */
int dms_deform_add_relative_constraints_host(dms_deform* d, const float* rows8_host, int n, dms_stream s);
/* The poses the next solve corrects: n times and row-major 4 x 4 matrices in device memory (copied).  n > max_poses:
 * DMS_ERR_CAPACITY, nothing changed.  dms_deform_get_poses copies them back (corrected, after an applied solve); synchronises. */
int dms_deform_set_poses(dms_deform* d, const long long* times_dev, const float* poses16_dev, int n, dms_stream s);
int dms_deform_get_poses(dms_deform* d, long long* times_host, float* poses16_host, int max_poses, int* n);
int dms_deform_constrain_global(dms_deform* d, int time, dms_stream s);
/* poses whose rotation the last global solve kept (see `poses` above) */
int dms_deform_get_kept_rotations(dms_deform* d, int* kept);
/* for tests: setPosesSeq's nodes and weights of the last global solve's poses, and the row envelope (per enabled node, its first
 * block column counted from the first enabled node; empty when no iteration ran) */
int dms_deform_get_pose_weights(dms_deform* d, int* ids4_host, double* weights4_host, int max_poses, int* n);
int dms_deform_get_envelope(dms_deform* d, int* first_host, int max_nodes, int* n);

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

/* ---- the frame step closes ORB-triggered global loops itself -----------------------------------------------------------------------
 * With the global loop solver on (needs hybrid_loops; the refusals of dms_fusion_set_loop_solver hold: a map the camera owns alone, no
 * clusters, W/20 x H/20 <= DMS_DEFORM_MAX_CONSTRAINTS; off by default, with it off nothing changes; the two-phase calls are not
 * affected otherwise) the context keeps Context::poseGraph() (ElasticFusion.cpp:571-573): behind every frame, one-call or two-phase,
 * the tick before its increment and the pose after the frame (one 64-byte copy in device memory, no synchronisation).  A frame that
 * would be pose max_poses + 1 returns DMS_ERR_CAPACITY before anything of it is enqueued.  So does an ORB-armed one-call frame, and
 * dms_fusion_apply_global_loop, once the context has kept more than DMS_DEFORM_MAX_RELATIVE relative rows (3 to 4 per local closure).
 *
 * A one-call dms_fusion_process_frame armed by dms_fusion_set_orb_loop then does what :292-355 does: after the constraint kernel the
 * host reads the row count; the local graph is sampled from the map as it stands (the local solver object is created if the local
 * solver never was; sampleRate as there, 5000 until set) and every 5th of its nodes becomes the global graph
 * (dms_deform_sample_from); the frame's rows go in with srcTime = tick and pins (:327-330), then the context's kept relative rows
 * (:335-341), the pose graph as the poses, and dms_deform_constrain_global; the host reads the status.  Applied: the corrected poses
 * replace the pose graph, fernDeforms is counted and the frame ends as dms_fusion_process_frame_end(graph, nodes, NULL) ends an
 * ORB-armed frame, the table taken from device memory.  Not applied: the frame goes on into the local block as before, with the local
 * solver if that is on.  dms_fusion_apply_global_loop is ElasticFusion::applyGlobalLoop (:1148-1240): _begin, the same solve, and
 * _end(table, nodes, accepted).
 * Known deviation: the reference re-samples both graphs at the end of every frame (:578-581), this samples when a loop arrives; the
 * two differ only when the earlier frame's sample passed count / 5 > 4 and the current one does not. */
int dms_fusion_set_global_loop_solver(dms_fusion* f, int on, int max_poses);
int dms_fusion_apply_global_loop(dms_fusion* f, const float* orbTcwOld16, const float* orbTcwNew16, dms_stream s);
/* rf.globalDeformation() of this context (NULL until first switched on); ElasticFusion::fernDeforms; Context::poseGraph() */
dms_deform* dms_fusion_global_deformation(dms_fusion* f);
int dms_fusion_get_fern_deforms(dms_fusion* f);
int dms_fusion_get_pose_graph(dms_fusion* f, long long* ticks_host, float* poses16_host, int max_poses, int* n);

#ifdef __cplusplus
}
#endif
#endif /* DMSLAM_DEFORM_H_ */
