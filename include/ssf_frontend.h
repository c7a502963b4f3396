/*
 * ssf_frontend.h -- C ABI of the MI355X (gfx950) SSF-SLAM LiDAR front-end.
 *
 * This is the drop-in boundary for the reference's hot path.  Every entry point names the
 * reference interface it replaces (file:line under YQChen8/SSF-SLAM).  Plain pointers and
 * sizes only: no C++ types, no exceptions, no torch types cross this boundary.
 *
 * Conventions
 *   - Pointers prefixed d_ are DEVICE pointers (hipMalloc'd / torch CUDA tensors) owned by the
 *     caller; pointers prefixed h_ are host pointers.  `stream` is a hipStream_t (NULL = the
 *     default stream).  All work is enqueued on `stream`; nothing synchronises unless stated.
 *   - A batch of F frames is stored back to back: frame f occupies points
 *     [d_frame_off[f], d_frame_off[f+1]) of the point arrays (int64 offsets, device).  Per-frame
 *     outputs that are point-shaped (plane clouds, ring-ordered clouds) use the SAME offsets:
 *     frame f's plane points start at d_frame_off[f] and d_plane_count[f] of them are valid.
 *   - Points are float32 x,y,z with a stride of `point_stride` floats (3 for the PointCloud2
 *     point_step 12 layout published by PointCloudOdometry*.py:84-92, 4 or 8 for padded PCL
 *     layouts).  Plane clouds are float32 x,y,z,intensity (16 B), intensity encoding
 *     indexInRow + row/100 exactly as src/frameFeature.cpp:77.
 *   - Poses are 7 doubles: q (x,y,z,w) then t (x,y,z) -- the para_q / para_t layout of
 *     src/lidarOdometry_onlyPC.cpp:62-63.
 *   - Return 0 on success, <0 on error; ssf_last_error() describes the last error of a context.
 *     HIP errors are mapped to SSF_E_HIP.  One context per host thread/stream (calls on a
 *     context are not thread-safe, different contexts are independent).
 */
#ifndef SSF_FRONTEND_H
#define SSF_FRONTEND_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SSF_ABI_VERSION 2

enum {
    SSF_OK = 0,
    SSF_E_ARG = -1,       /* bad argument / shape                                  */
    SSF_E_HIP = -2,       /* HIP runtime error                                     */
    SSF_E_NOMEM = -3,     /* device allocation failed                              */
    SSF_E_CAPACITY = -4,  /* output capacity too small                             */
    SSF_E_NODEV = -5      /* no gfx950 device                                      */
};

enum { SSF_SOLVER_CERES_LM = 0, SSF_SOLVER_GN = 1 };
enum { SSF_MASK_GMM = 0, SSF_MASK_GT = 1, SSF_MASK_GIVEN = 2 };
/* The evaluation of src/frameFeature.cpp:57 `atan(point.z / sqrt(x*x + y*y)) * 180 / M_PI` on
 * float members.  C++ overload resolution allows exactly two:
 *   SSF_RING_CHAIN_FLOAT   the float overloads std::atan(float) / std::sqrt(float) are visible at
 *                          global scope -- libstdc++'s <math.h> wrapper does `using std::atan;
 *                          using std::sqrt;`, and include/header.h:8-35 (ROS, tf, PCL, Ceres)
 *                          includes <math.h>: ratio z / sqrtf(r2), atanf, `* 180` in float,
 *                          `/ M_PI` in double, stored to float.  The default.
 *   SSF_RING_CHAIN_DOUBLE  only the C ::sqrt(double) / ::atan(double): the ratio and the angle
 *                          in double, stored to float.
 * The host libm (glibc) evaluates atanf / atan once per context into a step table; the device
 * never evaluates atan. */
enum { SSF_RING_CHAIN_FLOAT = 0, SSF_RING_CHAIN_DOUBLE = 1 };

/* Runtime replacement of the compile-time N_SCAN_ROW parameter blocks
 * (include/header.h:37-38, src/frameFeature.cpp:141-152, src/lidarOdometry_onlyPC.cpp:313-319). */
typedef struct {
    int32_t n_rows;       /* 16 or 64                                              */
    float plane_min;      /* curvature threshold (planeMin)                        */
    int32_t plane_span;   /* greedy spacing (planeSpan)                            */
    int32_t row_start;    /* rowIndexStart                                         */
    int32_t row_end;      /* rowIndexEnd                                           */
    float plane_max;      /* coplanarity gate (planeMax)                           */
    int32_t solver;       /* SSF_SOLVER_CERES_LM (reference) or SSF_SOLVER_GN      */
    int32_t max_iter;     /* 8 (ceres::Solver::Options max_num_iterations) or 10   */
    int32_t ring_chain;   /* SSF_RING_CHAIN_FLOAT (default) or SSF_RING_CHAIN_DOUBLE  */
} ssf_config;

typedef struct ssf_ctx ssf_ctx;

int32_t ssf_abi_version(void);
/* Fill `out` with the reference's parameter block for n_rows (16 or 64). */
int32_t ssf_config_default(int32_t n_rows, ssf_config* out);
/* Create a context bound to HIP device `device`. */
int32_t ssf_create(int32_t device, const ssf_config* cfg, ssf_ctx** out);
void ssf_destroy(ssf_ctx* ctx);
const char* ssf_last_error(const ssf_ctx* ctx);
/* Pre-size device scratch so later calls never allocate (graph-capture friendly). */
int32_t ssf_reserve(ssf_ctx* ctx, int32_t max_frames, int64_t max_points_per_frame);

/* Kernel timing (no reference counterpart: the reference has no timers).  While
 * enabled, every kernel this context launches is bracketed by HIP events on its stream; on a
 * stream no other stream competes with, each interval is that kernel's duration.
 * ssf_profile_read synchronises on the recorded events and returns, per kernel name, the
 * launches and total milliseconds recorded since the previous read (then clears them). */
typedef struct {
    char name[48];
    int32_t launches;
    double total_ms;
} ssf_kernel_time;
int32_t ssf_profile_enable(ssf_ctx* ctx, int32_t on);
int32_t ssf_profile_read(ssf_ctx* ctx, ssf_kernel_time* out, int32_t cap, int32_t* n_out);

/* ---------------------------------------------------------------------------------------
 * frameFeature: replaces cloudHandler() (src/frameFeature.cpp:35-139) -- ring binning
 * (:45-81), 11-tap curvature (:84-107) and greedy planar selection (:110-123) -- for a batch
 * of frames.  The VoxelGrid at :125-127 is dead work in the reference (its output is
 * discarded) and is not performed.
 *   d_pts           F frames of xyz (stride point_stride floats), offsets d_frame_off[F+1]
 *   total_points    host copy of d_frame_off[F] (extent of every point-shaped array)
 *   max_frame_points  host upper bound of points in any frame (grid sizing)
 *   d_plane_xyzi    out, plane points x,y,z,intensity (16 B) at frame offsets
 *   d_plane_count   out [F] int32, number of plane points per frame
 *   d_ring_xyzi     out, nullable: ring-ordered kept points (x,y,z,intensity) at frame offsets
 *   d_ring_off      out, nullable: [F*(n_rows+1)] int32 per-frame row offsets (frame relative)
 *   d_curv          out, nullable: curvature per ring-ordered point (0 where not computed)
 */
int32_t ssf_extract_planes_batch(ssf_ctx* ctx, void* stream, int32_t n_frames,
                                 const float* d_pts, int32_t point_stride,
                                 const int64_t* d_frame_off, int64_t total_points,
                                 int64_t max_frame_points,
                                 float* d_plane_xyzi, int32_t* d_plane_count,
                                 float* d_ring_xyzi, int32_t* d_ring_off, float* d_curv);

/* Beyond the reference (BASELINE configs[2] "mask applied before features"; parity unpinned,
 * off unless called): the same extraction on the points whose d_keep byte is non-zero -- e.g.
 * the background mask of ssf_mask_pose_batch at the same offsets.  Dropped points are treated as
 * if they were not in the cloud (the reference's frameFeature always receives every point,
 * scripts/PointCloudOdometry_noSeg.py:92-94), so the result equals ssf_extract_planes_batch on
 * the stably compacted cloud. */
int32_t ssf_extract_planes_batch_masked(ssf_ctx* ctx, void* stream, int32_t n_frames,
                                        const float* d_pts, int32_t point_stride,
                                        const int64_t* d_frame_off, int64_t total_points,
                                        int64_t max_frame_points, const uint8_t* d_keep,
                                        float* d_plane_xyzi, int32_t* d_plane_count,
                                        float* d_ring_xyzi, int32_t* d_ring_off, float* d_curv);
/* Single-frame form with the SURVEY §8(b) signature: synchronises, returns the plane count in
 * *h_out_m; SSF_E_CAPACITY if more than out_cap points were selected. */
int32_t ssf_extract_planes(ssf_ctx* ctx, void* stream, const float* d_pts, int64_t n,
                           int32_t point_step_bytes, int32_t xyz_offset_bytes,
                           float* d_out_xyzi, int64_t* h_out_m, int64_t out_cap);

/* ---------------------------------------------------------------------------------------
 * Plane table for frames that will serve as the LAST frame of a registration pair: for every
 * plane point a, the 30-NN ring-diverse 5-point pick, the 5x3 least-squares plane and the
 * coplanarity gate of src/lidarOdometry_onlyPC.cpp:173-232 (which depend only on the last
 * frame and a, so they are computed once per frame instead of once per correspondence x2).
 *   d_normal  out float32 x3 per plane point (frame offsets), d_valid out uint8 per point.
 *   d_sorted_xyzi / d_sorted_idx  out (nullable): the frame's plane points sorted by (x, index)
 *             and the permutation, the search index the k-NN walks use; pass them back to
 *             ssf_register_batch when this frame is the last frame.  When they are NULL, or
 *             max_plane_points exceeds SSF_SORTED_MAX, both calls fall back to brute-force k-NN.
 *             Use the same max_plane_points bound for a frame's table and its registration.
 *   d_strip_xyzi / d_strip_head  out (nullable, both or neither; needs the sorted buffers):
 *             float32 x4 and int32 per plane point (frame offsets).  The table's y-strip image of
 *             the frame (the association's search structure), kept so that ssf_register_batch
 *             stages it instead of rebuilding it when this frame is the last frame.  Frames of
 *             773..6144 plane points carry an image; others are rebuilt as before.
 */
#define SSF_SORTED_MAX 16384
int32_t ssf_plane_table_batch(ssf_ctx* ctx, void* stream, int32_t n_frames,
                              const float* d_plane_xyzi, const int64_t* d_frame_off,
                              const int32_t* d_plane_count, int64_t max_plane_points,
                              float* d_normal, uint8_t* d_valid, float* d_sorted_xyzi,
                              int32_t* d_sorted_idx, float* d_strip_xyzi, int32_t* d_strip_head);

/* ---------------------------------------------------------------------------------------
 * lidarOdometry_onlyPC: replaces frameRegistration() (src/lidarOdometry_onlyPC.cpp:147-252)
 * plus the pose accumulation of publishResult() (:87-90) for P independent pairs.
 *   last / curr      plane clouds (x,y,z,intensity) with their own offsets + counts
 *   d_last_normal/valid/sorted_*  plane table + search index of the last frames
 *                        (ssf_plane_table_batch); the sorted arrays are nullable (brute force)
 *   curr_total_points    host copy of d_curr_off[P] (correspondence scratch extent)
 *   max_plane_points     host upper bound of plane points in any frame (grid sizing)
 *   d_pose_rel [P*7] in: warm start q_last_curr/t_last_curr (the previous pair's solution,
 *                    :164,251-252); out: the solution.  Last frames with <= 10 points leave
 *                    it unchanged (:158).  PRECONDITION: q is a unit quaternion (the solve's
 *                    Jacobian is the parameterisation's for |q| = 1; a chain's drift of 1e-12
 *                    is inside the bars, |q| = 1 +- 1e-3 moves a step by ~1e-8 rad).
 *   d_pose_abs [P*7] nullable; in: q_0_last,t_0_last; out: q_0_curr,t_0_curr (:87-90).
 *   d_log      nullable [P*max_iter*10] doubles per iteration: q(4) t(3) cost status radius
 *   d_nlog     nullable [P] iterations logged;  d_ncorr nullable [P] correspondences used
 *              (-1 when skipped);  d_nn nullable: per curr point 1-NN index into last.
 *   d_last_strip_xyzi / d_last_strip_head  nullable (both or neither): the strip image the
 *              last frames' ssf_plane_table_batch call wrote (same max_plane_points).  The results
 *              are identical with or without it; with it the association skips its strip build.
 */
int32_t ssf_register_batch(ssf_ctx* ctx, void* stream, int32_t n_pairs,
                           const float* d_last_xyzi, const int64_t* d_last_off,
                           const int32_t* d_last_count, const float* d_last_normal,
                           const uint8_t* d_last_valid, const float* d_last_sorted_xyzi,
                           const int32_t* d_last_sorted_idx, const float* d_curr_xyzi,
                           const int64_t* d_curr_off, const int32_t* d_curr_count,
                           int64_t curr_total_points, int64_t max_plane_points,
                           double* d_pose_rel, double* d_pose_abs,
                           double* d_log, int32_t* d_nlog, int32_t* d_ncorr, int32_t* d_nn,
                           const float* d_last_strip_xyzi, const int32_t* d_last_strip_head);

/* The association launch ssf_register_batch(_edges) / ssf_register_chain make for n_pairs pairs
 * bounded by max_plane_points, given the sorted buffers of ssf_plane_table_batch (replaces: none
 * -- the launcher's own choice, exported so that a test can prove which path a launch took).
 * Host arithmetic only: no context, no HIP call.  SSF_E_ARG on n_pairs < 1, a negative bound or
 * a null out.
 *   strip_path  1: the y-strip association (max_plane_points within the LDS sort limit, 16384);
 *               0: another association kernel, the other fields are 0
 *   group_mode  1: one query per 16-lane group over qsplit work-groups per pair (launches of
 *               <= 16 pairs); 0: the lane mode, one query per lane
 *   soa         1: the last frame staged as 14-B SoA arrays (bound > 6144), 0: as 16-B points
 *   qsplit      work-groups per pair; lane mode: min(8, 256 / n_pairs, ceil(bound / 1024))
 *   lds_cap     last-frame points the launch stages in LDS (<= 10752); a longer last frame
 *               walks the sorted copy in global memory
 *   compacted   1: lane mode with qsplit == 1 and planes only -- the association writes the
 *               valid records compacted in rank order and the solve streams them in; 0: records
 *               in query order, the solve compacts them itself */
typedef struct {
    int32_t strip_path;
    int32_t group_mode;
    int32_t soa;
    int32_t qsplit;
    int32_t lds_cap;
    int32_t compacted;
} ssf_launch_plan;
int32_t ssf_register_plan(int32_t n_pairs, int64_t max_plane_points, int32_t with_edges,
                          ssf_launch_plan* out);

/* A sequence's consecutive pairs in one call (lidarOdometry_onlyPC's frame loop over a sequence:
 * every pair is warm-started from the previous pair's solution, src/lidarOdometry_onlyPC.cpp:164,
 * 251-252).  Frames 0..n_pairs of ONE plane batch (d_off / d_count: n_pairs + 2 / n_pairs + 1
 * entries, the table / search index / strip image of ssf_plane_table_batch on the same batch);
 * pair k registers frame k + 1 (curr) against frame k (last).
 *   d_pose_init [7]          warm start of pair 0 (q xyzw, t)
 *   d_pose_seq [n_pairs*7]   out: pair k's solution (the warm start of pair k + 1)
 *   d_pose_abs_init [7] / d_pose_abs_seq [n_pairs*7]  nullable (both or neither): the pose of
 *                            frame 0, and out the pose of frame k + 1 (:87-90)
 *   d_ncorr [n_pairs]        nullable: correspondences per pair (-1 when skipped, :158)
 * Results are identical to n_pairs ssf_register_batch calls of one pair each with the warm start
 * copied between them; the links read the previous output in place (no copy launches). */
int32_t ssf_register_chain(ssf_ctx* ctx, void* stream, int32_t n_pairs, const float* d_xyzi,
                           const int64_t* d_off, const int32_t* d_count, const float* d_normal,
                           const uint8_t* d_valid, const float* d_sorted_xyzi,
                           const int32_t* d_sorted_idx, int64_t total_points,
                           int64_t max_plane_points, const double* d_pose_init,
                           double* d_pose_seq, const double* d_pose_abs_init,
                           double* d_pose_abs_seq, int32_t* d_ncorr,
                           const float* d_strip_xyzi, const int32_t* d_strip_head);

/* Single-pair form with the SURVEY §8(b) signature: frameRegistration() on the globals
 * lastFramePlanePtr / currFramePlanePtr / para_q / para_t (src/lidarOdometry_onlyPC.cpp:51-71,
 * 147-252).  The plane clouds are device float4 (x, y, z, intensity) as frameFeature publishes
 * them; the warm start h_q_init (x,y,z,w) / h_t_init is the previous pair's solution (:164,
 * 251-252) and the solution comes back in h_q_out / h_t_out.  The last frame's plane table and
 * search index are built inside the call (ctx scratch).  A last frame with <= 10 points adds no
 * residual (:158): the warm start is returned unchanged, rc 0, log->n_corr = -1.  Synchronous.
 * log (nullable): per LM/GN iteration the pose after it, the Ceres cost, a status code and the
 * trust-region radius. */
enum {
    SSF_STEP_REJECTED = 0,        /* LM step computed, rho <= 1e-3, radius shrunk            */
    SSF_STEP_ACCEPTED = 1,        /* LM step accepted                                        */
    SSF_STEP_INVALID = 2,         /* LM/GN linear solve failed or non-positive model decrease */
    SSF_STEP_PARAM_TOL = 3,       /* ParameterToleranceReached (|dx| <= 1e-8 (|x| + 1e-8))   */
    SSF_STEP_FUNC_TOL = 4,        /* FunctionToleranceReached (|dcost| <= 1e-6 cost)         */
    SSF_STEP_GRAD_TOL = 5,        /* GradientToleranceReached (max-norm <= 1e-10)            */
    SSF_STEP_GN = 6               /* undamped Gauss-Newton step (SSF_SOLVER_GN)              */
};
typedef struct {
    double q[4];       /* pose after the iteration, q x,y,z,w                          */
    double t[3];
    double cost;       /* Ceres cost 1/2 sum rho(r^2) over the duplicated blocks        */
    int32_t status;    /* SSF_STEP_*                                                    */
    int32_t pad;
    double radius;     /* trust-region radius after the iteration (0 in GN mode)         */
} ssf_step;
typedef struct {
    int32_t cap;       /* in: capacity of steps[] (cfg.max_iter holds a full log)        */
    int32_t n_steps;   /* out: iterations logged                                        */
    int32_t n_corr;    /* out: valid correspondences (-1: skipped, :158)                */
    int32_t pad;
    ssf_step* steps;   /* caller-owned host array of cap entries                        */
} ssf_step_log;
int32_t ssf_register_pair(ssf_ctx* ctx, void* stream, const float* d_last_xyzi, int64_t m_last,
                          const float* d_curr_xyzi, int64_t m_curr, const double* h_q_init,
                          const double* h_t_init, double* h_q_out, double* h_t_out,
                          ssf_step_log* log);

/* ---------------------------------------------------------------------------------------
 * Edge features + point-to-line residuals: BEYOND THE REFERENCE.  SSF-SLAM's frameFeature is
 * planar only (src/frameFeature.cpp:110-123) and its registration point-to-plane only
 * (src/lidarOdometry_onlyPC.cpp:25-43); the north_star asks for edge extraction and
 * point-to-line terms, so these entry points are the build's own extension, off unless called,
 * with parity unpinned (definitions restated in oracle/edge_oracle.c):
 *   selection   per row in [row_start, n_rows - row_end), greedy in index order: curvature (the
 *               :84-107 value) > edge_min and j >= jstart -> select, jstart = j + edge_span
 *   line table  per LAST-frame edge point: exact 5-NN among that frame's edges, centroid and
 *               covariance (double), Jacobi eigen-decomposition; valid iff the 5th squared
 *               distance < max_nn_d2 and lambda1 > line_ratio * lambda2; direction u = the
 *               principal eigenvector (largest-|.| component positive)
 *   residual    e = (I - u u^T)(R p + t - c) for the 1-NN last edge of the transformed current
 *               edge point, one Huber(0.1) block on |e|^2, doubled like every :160 block
 */
typedef struct {
    float edge_min;       /* curvature threshold, m^2 (1.0)                                     */
    int32_t edge_span;    /* greedy spacing in a row (10 for 64 rows, 3 for 16)                 */
    float line_ratio;     /* lambda1 > line_ratio * lambda2 (3.0)                               */
    float max_nn_d2;      /* 5th-NN squared distance gate (1.0)                                 */
} ssf_edge_config;
int32_t ssf_edge_config_default(int32_t n_rows, ssf_edge_config* out);
int32_t ssf_set_edge_config(ssf_ctx* ctx, const ssf_edge_config* cfg);
/* ssf_extract_planes_batch(_masked) plus the edge cloud: d_edge_xyzi (x,y,z,intensity, frame
 * offsets, capacity = the points) and d_edge_count [F].  d_keep nullable. */
int32_t ssf_extract_features_batch(ssf_ctx* ctx, void* stream, int32_t n_frames,
                                   const float* d_pts, int32_t point_stride,
                                   const int64_t* d_frame_off, int64_t total_points,
                                   int64_t max_frame_points, const uint8_t* d_keep,
                                   float* d_plane_xyzi, int32_t* d_plane_count,
                                   float* d_edge_xyzi, int32_t* d_edge_count);
/* Line table of frames that will be LAST frames: d_line 6 floats per edge point (centroid x,y,z,
 * direction x,y,z) and d_line_valid u8, at the frame offsets. */
int32_t ssf_edge_table_batch(ssf_ctx* ctx, void* stream, int32_t n_frames,
                             const float* d_edge_xyzi, const int64_t* d_frame_off,
                             const int32_t* d_edge_count, int64_t max_edge_points,
                             float* d_line, uint8_t* d_line_valid);
/* ssf_register_batch with point-to-line blocks added to every pair's problem (same LM/GN loop,
 * same pose / log outputs).  Edge clouds at their own offsets; d_ncorr_edge nullable [P]; the
 * strip image as in ssf_register_batch. */
int32_t ssf_register_batch_edges(ssf_ctx* ctx, void* stream, int32_t n_pairs,
                                 const float* d_last_xyzi, const int64_t* d_last_off,
                                 const int32_t* d_last_count, const float* d_last_normal,
                                 const uint8_t* d_last_valid, const float* d_last_sorted_xyzi,
                                 const int32_t* d_last_sorted_idx, const float* d_curr_xyzi,
                                 const int64_t* d_curr_off, const int32_t* d_curr_count,
                                 int64_t curr_total_points, int64_t max_plane_points,
                                 const float* d_last_edge_xyzi, const int64_t* d_last_edge_off,
                                 const int32_t* d_last_edge_count, const float* d_last_line,
                                 const uint8_t* d_last_line_valid, const float* d_curr_edge_xyzi,
                                 const int64_t* d_curr_edge_off, const int32_t* d_curr_edge_count,
                                 int64_t curr_edge_total, int64_t max_edge_points,
                                 double* d_pose_rel, double* d_pose_abs, double* d_log,
                                 int32_t* d_nlog, int32_t* d_ncorr, int32_t* d_ncorr_edge,
                                 const float* d_last_strip_xyzi, const int32_t* d_last_strip_head);

/* ---------------------------------------------------------------------------------------
 * PointCloudOdometry{,_noSeg}.py: replaces the dynamic-point mask + slove_RT_by_SVD + Quaternion
 * block (scripts/PointCloudOdometry_noSeg.py:97-125, scripts/PointCloudOdometry.py:91-101 and the
 * identical ASF block main_sju_occ_ros.py:256-284) for F frames.
 *   d_pts / d_flow      packed float32 xyz (stride 3) per point: pos1 and the scene flow (gt).
 *   h_frame_off [F+1]   host copy of the offsets (frame sizes drive the RandomState choice()).
 *   mode SSF_MASK_GMM:  GaussianMixture(n_components=2).fit_predict([flow, xyz]) (sklearn 1.7.2
 *                       semantics), background = most common label;  h_draws [F*3] (host,
 *                       nullable) are the three numpy RandomState doubles its k-means++ init
 *                       consumes per frame; NULL draws them from the context RNG (ssf_rng_seed).
 *        SSF_MASK_GT:   background = d_mask_in == 0 (s_fg_mask, PointCloudOdometry.py:91).
 *        SSF_MASK_GIVEN: background = d_mask_in != 0.
 *   Kabsch on background rows: slove_RT_by_SVD(points + flow, points) (:114-118).
 *   reflection 0: det<0 -> status SSF_POSE_REFLECTION (the reference raises TypeError at :33);
 *              1: flip Vt[2] (the evident intent of :32-33).
 *   d_bg_mask  out, nullable: uint8 per point, 1 = background.
 *   d_out      out [F*SSF_POSE_OUT_STRIDE] doubles, see SSF_POSE_OUT_* below.
 *   A frame of more than 2^32 / 12 points (2^32 / 24 for the f64 form) fails with SSF_E_ARG
 *   before any launch: the kernel addresses a frame with 32-bit byte offsets.
 */
#define SSF_POSE_OUT_STRIDE 32
enum {
    SSF_POSE_OUT_T = 0,        /* t (3)                  -- para_t_q[0:3]                    */
    SSF_POSE_OUT_Q = 3,        /* q x,y,z,w (4)          -- para_t_q[3:7]                    */
    SSF_POSE_OUT_R = 7,        /* R row-major (9)                                            */
    SSF_POSE_OUT_STATUS = 16,  /* 0 ok, <0 SSF_POSE_* error                                  */
    SSF_POSE_OUT_NBG = 17,     /* background point count                                     */
    SSF_POSE_OUT_BGLABEL = 18, /* GMM label taken as background                              */
    SSF_POSE_OUT_KM_ITER = 19, /* KMeans n_iter_                                             */
    SSF_POSE_OUT_EM_ITER = 20, /* GaussianMixture n_iter_                                    */
    SSF_POSE_OUT_CONVERGED = 21,
    SSF_POSE_OUT_CENTER0 = 22, /* k-means++ chosen indices                                   */
    SSF_POSE_OUT_CENTER1 = 23,
    SSF_POSE_OUT_LOWER_BOUND = 24,
    SSF_POSE_OUT_PASSES = 25   /* algorithmic bytes / (24 B x points): full-pass equivalents */
};
enum { SSF_POSE_EMPTY = -1, SSF_POSE_REFLECTION = -2, SSF_POSE_NOT_ORTHOGONAL = -3,
       SSF_POSE_GMM_FAILED = -4, SSF_POSE_SYNC_FAILED = -5 };
int32_t ssf_mask_pose_batch(ssf_ctx* ctx, void* stream, int32_t n_frames, const float* d_pts,
                            const float* d_flow, const int64_t* d_frame_off,
                            const int64_t* h_frame_off, int32_t mode, const uint8_t* d_mask_in,
                            const double* h_draws, int32_t reflection, uint8_t* d_bg_mask,
                            double* d_out);
/* The same block on float64 pos / flow (the reference's own dtype when the npz arrays or the
 * ASF network output arrive as float64, PointCloudOdometry_noSeg.py:97-118): every load is exact,
 * so R / t carry no float32 rounding of the inputs.  Otherwise identical to ssf_mask_pose_batch
 * (same modes, draws, outputs and status codes); 48 B per point per pass instead of 24. */
int32_t ssf_mask_pose_batch_f64(ssf_ctx* ctx, void* stream, int32_t n_frames, const double* d_pts,
                                const double* d_flow, const int64_t* d_frame_off,
                                const int64_t* h_frame_off, int32_t mode, const uint8_t* d_mask_in,
                                const double* h_draws, int32_t reflection, uint8_t* d_bg_mask,
                                double* d_out);
/* slove_RT_by_SVD + Quaternion(matrix=R) on FLOAT32 arrays, per frame, as numpy runs them when
 * the inputs are float32: the ASF block on the network's float32 flow
 * (scripts/ActiveSceneFlow/main_sju_occ_ros.py:273-284, slove_RT_by_SVD :455-473).
 * Replaces the f64 tail that ssf_mask_pose_batch computes (the reference's behaviour on float64
 * inputs) with the reference's float32 arithmetic: f32 src = dst + flow, row-order f32 means,
 * f32 centring, R and t rounded to f32 (oracle/ssf_oracle.c orc_kabsch_f32 restates each step).
 *   source rows: d_flow != NULL -> f32(d_dst + d_flow) (target = points + move_gt, :273), with
 *                d_src ignored; d_flow == NULL -> d_src (slove_RT_by_SVD(src, dst) directly).
 *   d_mask   nullable uint8 per point: rows with mask != 0 (the background of ssf_mask_pose_batch's
 *            d_bg_mask); NULL = every row.
 *   after_mask 1: d_out holds ssf_mask_pose_batch's results for these frames (same stream, before
 *            this call); T, Q, R, NBG and STATUS are replaced, the fit fields kept, and frames with
 *            SSF_POSE_GMM_FAILED / SSF_POSE_SYNC_FAILED left as they are.  0: d_out is written whole.
 *   d_out    [F * SSF_POSE_OUT_STRIDE] doubles (SSF_POSE_OUT_* below); R / t hold float32 values.
 * Asynchronous on stream.  One work-group per frame; the two means are serial in row order. */
int32_t ssf_kabsch_f32_batch(ssf_ctx* ctx, void* stream, int32_t n_frames, const float* d_src,
                             const float* d_dst, const float* d_flow, const int64_t* d_frame_off,
                             const uint8_t* d_mask, int32_t reflection, int32_t after_mask,
                             double* d_out);
/* Work-groups per frame of the GMM fit in ssf_mask_pose_batch (no reference counterpart;
 * results do not depend on it beyond f64 summation order): 0 = automatic (as many as keep the
 * chip full: ~256 / frames, at most 32; 1 for 256 frames and more), 1..32 = fixed.  Memory: a
 * launch with G > 1 keeps frames x G x 104 KiB of exchange slots in the context (grown on
 * demand, never shrunk): a fixed 32 on a 256-frame batch is ~850 MB.  With more
 * than one, a frame's points are cut into contiguous parts whose per-pass sums are exchanged
 * in global memory; a partner that never arrives gives status SSF_POSE_SYNC_FAILED. */
int32_t ssf_set_mask_split(ssf_ctx* ctx, int32_t parts_per_frame);
/* Frame scheduling of the next ssf_mask_pose_batch / _f64 launches (no reference counterpart: a
 * frame's result does not depend on when it runs, so every schedule gives the same outputs).
 *   d_order  nullable device int32 [n_order], a permutation of 0 .. n_order - 1 (caller-owned; it
 *            must stay valid until the launches that read it have run): the k-th frame dispatched
 *            is d_order[k].  Longest-first by the previous step's SSF_POSE_OUT_PASSES of the same
 *            sequences starts the slow frames first and shortens a launch's straggler tail.  A
 *            launch of n_frames != n_order fails with SSF_E_ARG; an entry out of range is skipped.
 *   queue    > 0 (frames on one work-group each): at most `queue` work-groups, each taking the
 *            next frame when its own is done (a frame queue: a slow frame holds one CU while the
 *            others drain the batch); 0 = one work-group per frame. */
int32_t ssf_set_mask_schedule(ssf_ctx* ctx, const int32_t* d_order, int32_t n_order, int32_t queue);
/* Seed the context's numpy-legacy RandomState (MT19937) -- the `np.random.seed(s)` the reference
 * never calls; every GMM frame then consumes 3 doubles in frame order, as the reference's global
 * RandomState does across frames. */
int32_t ssf_rng_seed(ssf_ctx* ctx, uint32_t seed);

/* ---------------------------------------------------------------------------------------
 * The ASF loader's subsample: replaces the rm_ground cut, hybrid_sample_points and the
 * np.random.choice to nb_points of scripts/ActiveSceneFlow/utils/datasets/carla.py:179-200,
 * 236-250, 274-285 for F clouds in one launch.  The draw is defined here, not
 * numpy's MT19937 stream: with F(z) the SplitMix64 finaliser, g = 0x9E3779B97F4A7C15,
 *   s(stream)      = F(F(F(seed + g) + tag) + stream)
 *   key(stream, i) = (F(s(stream) + (i + 1) g) >> 32) >> (32 - key_bits)     i: index in the frame
 * so a frame's result depends on (seed, tag, its own points) only.
 *   d_pts [total, point_stride] f32 (point_stride >= 3), d_frame_off / h_frame_off [F + 1] int64
 *                 (device and host copies; a frame holds at most SSF_SAMPLE_MAX_POINTS points)
 *   d_class       nullable uint8 per point: 0 background, else foreground (the quota needs it)
 *   nb            points to return per frame, 1 .. SSF_SAMPLE_MAX_NB
 *   use_z, z_min  use_z != 0: the survivors are the points with !(z < z_min) (carla.py:237: a NaN
 *                 z survives); else every point
 *   quota         -1: off.  >= 0: k_fg = min(foreground survivors, quota, nb) smallest-key
 *                 foreground survivors first, then the nb - k_fg smallest-key background survivors;
 *                 SSF_SAMPLE_SHORT when the background holds fewer (the reference's choice raises)
 *   h_tag         nullable host [F] uint64 (read during the call): NULL = the frame's position
 *   key_bits      1 .. 32 (32: the definition; fewer truncate the keys of stream 0, so that ties
 *                 and the index tie-break occur at small sizes)
 * Without quota: survivors n > nb -> the nb survivors smallest in (key(0, i), i), ascending in that
 * order (a uniformly random ordered sample without replacement); 1 <= n <= nb -> slot j is the
 * survivor of rank (key(1, j) * n) >> 32 in index order, key_bits taken as 32 (with replacement:
 * the reference resamples unless nb < n, carla.py:274-277).  n == 0 -> SSF_SAMPLE_EMPTY.  A frame
 * whose status is not SSF_SAMPLE_OK has its d_idx / d_xyz rows zero-filled; other frames are not
 * affected.
 *   d_idx [F, nb] int32 index within the frame;  d_xyz [F, 3, nb] f32 nullable, channel-major
 *   (TFlow's input layout);  d_n [F] int32 survivors;  d_status [F] int32 SSF_SAMPLE_*.
 * Asynchronous on stream.  SSF_E_ARG before any HIP call: null context or pointer (d_pts may be
 * NULL for a batch that holds no point), n_frames < 0,
 * nb, key_bits or point_stride out of range, quota < -1, quota >= 0 without d_class, offsets that
 * decrease, a frame above SSF_SAMPLE_MAX_POINTS. */
#define SSF_SAMPLE_MAX_NB 8192
#define SSF_SAMPLE_MAX_POINTS (1 << 24)
#define SSF_SAMPLE_TAG_CHUNK 256   /* frames per launch when h_tag is given */
enum { SSF_SAMPLE_OK = 0, SSF_SAMPLE_EMPTY = -1, SSF_SAMPLE_SHORT = -2 };
int32_t ssf_subsample_batch(ssf_ctx* ctx, void* stream, int32_t n_frames, const float* d_pts,
                            int32_t point_stride, const int64_t* d_frame_off,
                            const int64_t* h_frame_off, const uint8_t* d_class, int32_t nb,
                            float z_min, int32_t use_z, int32_t quota, uint64_t seed,
                            const uint64_t* h_tag, int32_t key_bits, int32_t* d_idx, float* d_xyz,
                            int32_t* d_n, int32_t* d_status);

/* ---------------------------------------------------------------------------------------
 * lidarOdometry.cpp (SSF path): frameRegistration() (src/lidarOdometry.cpp:145-159) ingests
 * [t, q] and publishResult() (:80-83) accumulates.  Batched prefix product over a sequence of
 * n relative poses (7 doubles each, q xyzw + t): d_abs[i] = d_abs[i-1] * d_rel[i], seeded with
 * h_start (nullable = identity).  One device thread walks the chain (it is inherently serial).
 */
int32_t ssf_accumulate_sequence(ssf_ctx* ctx, void* stream, int32_t n, const double* d_rel,
                                const double* h_start, double* d_abs);

/* ---------------------------------------------------------------------------------------
 * mapOptmization loop closure.
 *
 * ssf_voxel_grid_batch replaces pcl::VoxelGrid<PointXYZI>::filter as downSizeFilterICP
 * (leaf 0.1, src/mapOptmization.cpp:214-217, 461) and downSizeFilterMap (leaf 0.4, :406-409,
 * 462) use it: per cloud, the centroid (x, y, z, intensity) of every occupied cube, in voxel
 * index order.  d_xyzi: float4 points of n_clouds clouds at d_off / h_off (int64, n_clouds + 1);
 * d_out: float4 at the SAME offsets (a cloud's output never exceeds its input);
 * d_out_count: int32 per cloud.  Asynchronous on stream.
 */
int32_t ssf_voxel_grid_batch(ssf_ctx* ctx, void* stream, int32_t n_clouds, const float* d_xyzi,
                             const int64_t* d_off, const int64_t* h_off, float leaf,
                             float* d_out, int32_t* d_out_count);

/* ssf_transform_clouds_batch replaces pcl::transformPointCloud(cloud, out, Eigen::Affine3d) as
 * updateKeyPose (src/mapOptmization.cpp:310) and getLoopLocalMap (:214) use it, for n_clouds
 * ragged clouds, each by its own pose, in one launch (the map cloud of correctPoses, :315-332).
 *   d_xyzi / d_out  float4 points; cloud c is points [off[c], off[c + 1]) of both (output at the
 *                   SAME offsets).  d_out must not alias d_xyzi.
 *   d_off / h_off   int64, n_clouds + 1, device and host copies.  off[0] may be non-zero (pass
 *                   d_off + first and h_off + first to transform clouds first ... first + n - 1);
 *                   points outside [off[0], off[n_clouds]) are not touched.
 *   d_T             12 doubles per cloud: the top three rows of the 4x4, row-major
 *                   (R[r][0], R[r][1], R[r][2], t[r]).
 * Per output row, as PCL 1.10's detail::Transformer<double>::se3 writes it:
 *   (float)(((T[r][0]*(double)x + T[r][1]*(double)y) + T[r][2]*(double)z) + T[r][3])
 * left to right in double, one rounding to float, no fused multiply-add; intensity is copied bit
 * for bit.  n_clouds == 0 and an all-empty range return SSF_OK without a launch.  Asynchronous
 * on stream.
 */
int32_t ssf_transform_clouds_batch(ssf_ctx* ctx, void* stream, int32_t n_clouds, const float* d_xyzi,
                                   const int64_t* d_off, const int64_t* h_off, const double* d_T,
                                   float* d_out);

/* ssf_icp_batch replaces pcl::IterativeClosestPoint<PointXYZI, PointXYZI>::align +
 * hasConverged + getFitnessScore + getFinalTransformation as addLoopFactor() uses them
 * (src/mapOptmization.cpp:224-238): n_prob independent (source, target) problems, float4
 * clouds at int64 offsets (device + host copies).  h_guess: n_prob row-major 4x4 float initial
 * transforms (nullable = identity).  h_out (host, n_prob * SSF_ICP_OUT_STRIDE doubles): the
 * final transformation (16, row-major, float values), fitness score, converged, iterations,
 * convergence state (SSF_ICP_*), correspondences of the last iteration.  Synchronous: the
 * iteration loop runs on device; the host only polls the per-problem done flags. */
typedef struct {
    int32_t max_iter;       /* setMaximumIterations (100)                              */
    float max_corr_dist;    /* setMaxCorrespondenceDistance (50)                       */
    double trans_eps;       /* setTransformationEpsilon (1e-6)                         */
    double fit_eps;         /* setEuclideanFitnessEpsilon (1e-6)                       */
} ssf_icp_params;
#define SSF_ICP_OUT_STRIDE 24
enum {
    SSF_ICP_OUT_T = 0, SSF_ICP_OUT_FITNESS = 16, SSF_ICP_OUT_CONVERGED = 17,
    SSF_ICP_OUT_ITERATIONS = 18, SSF_ICP_OUT_STATE = 19, SSF_ICP_OUT_NCORR = 20
};
enum {  /* pcl::registration::DefaultConvergenceCriteria::ConvergenceState */
    SSF_ICP_NOT_CONVERGED = 0, SSF_ICP_ITERATIONS = 1, SSF_ICP_TRANSFORM = 2, SSF_ICP_ABS_MSE = 3,
    SSF_ICP_REL_MSE = 4, SSF_ICP_NO_CORRESPONDENCES = 5
};
int32_t ssf_icp_params_default(ssf_icp_params* out);
int32_t ssf_icp_batch(ssf_ctx* ctx, void* stream, int32_t n_prob, const float* d_src,
                      const int64_t* d_src_off, const int64_t* h_src_off, const float* d_tgt,
                      const int64_t* d_tgt_off, const int64_t* h_tgt_off,
                      const ssf_icp_params* params, const float* h_guess, double* h_out);

/* Loop detection by appearance (beyond the reference, whose detectLoopFrameID,
 * src/mapOptmization.cpp:167-197, is a radius search over the estimated key positions and finds
 * nothing once odometry has drifted past its radius): Scan Context descriptors (Kim & Kim, IROS
 * 2018) compared exhaustively, every candidate at every column shift.  The
 * definitions are this project's own.
 *
 * ssf_scan_context_batch: the descriptor of n_clouds ragged clouds in the sensor frame, one
 * launch.
 *   d_pts [total, point_stride] f32 (point_stride 3 or 4: x, y, z first), cloud c is points
 *                 [off[c], off[c + 1]) of d_off / h_off (int64, n_clouds + 1, device and host copies)
 *   d_desc        [n_clouds, SSF_SC_RINGS, SSF_SC_SECTORS] f32
 * A point with a non-finite coordinate is skipped; with r = sqrt(x^2 + y^2), a point with
 * r >= max_range is skipped; ring = min(floor(r / (max_range / 20)), 19), sector =
 * min(floor(phi / (2 pi / 60)), 59) with phi = atan2(y, x) mapped to [0, 2 pi);
 * desc[ring][sector] = max(0, max over its points of the float sum z + lidar_height); an empty bin
 * and an empty cloud give 0.  r and phi are evaluated in float: a point within float rounding of a
 * bin edge may fall on either side of it, every other point's bin is exact and the descriptor bit
 * for bit that of the definition.
 *
 * ssf_scan_context_match: n_query query descriptors against n_db database descriptors.  A column
 * is valid when one of its bins is above 0 (descriptors are finite and non-negative).  With every
 * valid column scaled to unit length and J(s) the columns j where query column j and candidate
 * column (j + s) % 60 are both valid,
 *   d(s) = 1 - (sum over J(s) of q[:, j] . c[:, (j + s) % 60]) / |J(s)|,   1 when J(s) is empty
 *   dist = min over s of d(s), shift = the smallest s that attains it
 * so the query sensor's yaw relative to the candidate's is shift * 2 pi / 60.  Per query the best
 * candidate is the smallest of 0 .. n_eligible - 1 in the order (dist, index).
 *   d_query [n_query, 20, 60], d_db [n_db, 20, 60] f32 (d_db may be NULL when n_db == 0)
 *   d_n_eligible / h_n_eligible  int32 per query, device and host copies, 0 .. n_db
 *   d_dist, d_shift  nullable together: [n_query, n_db] f32 / int32, every pair; NULL = selection
 *                 only (then only candidates below the largest n_eligible are compared)
 *   d_best        per query: index (-1 when n_eligible is 0, then dist 1 and shift 0), dist, shift
 * Sums have a fixed order and nothing is accumulated atomically: a pair's dist and shift are the
 * same bits on every run and whatever else is in the call.
 *
 * Both are asynchronous on stream.  SSF_E_ARG before any HIP call: a null context or pointer
 * (d_pts may be NULL for a batch that holds no point), a negative count, point_stride outside
 * 3..4, offsets that are negative or decrease, max_range or lidar_height not finite, max_range
 * <= 0, only one of d_dist / d_shift, n_eligible outside 0 .. n_db, n_query * ceil(n_db / 16)
 * >= 2^31.  n_clouds == 0 and n_query == 0 return SSF_OK without a launch.
 *
 * ssf_scan_context_match_topk: the arguments of ssf_scan_context_match plus k and exclusion; per
 * query the k best candidates that are places of their own.  For a query with eligible prefix
 * [0, n_eligible), k in 1 .. SSF_SC_MAX_TOPK and exclusion E >= 0: walk the candidates in the
 * total order (dist, index), a NaN distance counting as +infinity; take a candidate when its
 * index differs by more than E from every index already taken; stop at k taken or when the prefix
 * is exhausted.
 *   d_best        [n_query * k], query-major: slot j of a query is its j-th taken candidate
 *                 (index, dist, shift), dist and shift copied from the rows; an unfilled slot is
 *                 (-1, 1.0f, 0), the record ssf_scan_context_match writes without a candidate
 * Slot 0 is ssf_scan_context_match's d_best bit for bit, for every E; E = 0 gives the plain k
 * smallest.  d_dist / d_shift as above (NULL together = selection only, the rows then live in
 * context scratch).  The rows come from the same launch as ssf_scan_context_match's.  SSF_E_ARG
 * before any HIP call, with nothing written: k < 1, k > SSF_SC_MAX_TOPK, exclusion < 0 and every
 * argument error of ssf_scan_context_match.  n_query == 0 returns SSF_OK without a launch. */
#define SSF_SC_RINGS 20
#define SSF_SC_SECTORS 60
#define SSF_SC_MAX_TOPK 8
typedef struct {
    float max_range;        /* 80 m                                                          */
    float lidar_height;     /* 2 m: added to z so that heights above the ground are positive */
    float threshold;        /* 0.13: a candidate is accepted when dist < threshold; read by
                               the caller (ssf.loop.LoopCloser), not by these entry points   */
} ssf_sc_params;
typedef struct {
    int32_t index;
    float dist;
    int32_t shift;
    int32_t reserved;
} ssf_sc_best;
int32_t ssf_sc_params_default(ssf_sc_params* out);
int32_t ssf_scan_context_batch(ssf_ctx* ctx, void* stream, int32_t n_clouds, const float* d_pts,
                               int32_t point_stride, const int64_t* d_off, const int64_t* h_off,
                               const ssf_sc_params* params, float* d_desc);
int32_t ssf_scan_context_match(ssf_ctx* ctx, void* stream, int32_t n_query, const float* d_query,
                               int32_t n_db, const float* d_db, const int32_t* d_n_eligible,
                               const int32_t* h_n_eligible, float* d_dist, int32_t* d_shift,
                               ssf_sc_best* d_best);
int32_t ssf_scan_context_match_topk(ssf_ctx* ctx, void* stream, int32_t n_query, const float* d_query,
                                    int32_t n_db, const float* d_db, const int32_t* d_n_eligible,
                                    const int32_t* h_n_eligible, float* d_dist, int32_t* d_shift,
                                    ssf_sc_best* d_best, int32_t k, int32_t exclusion);

/* ssf_pose_graph_batch replaces the pose graph of mapOptmization: the prior and odometry
 * factors of addOdomFactor (src/mapOptmization.cpp:147-165), the loop factor (:274) and
 * runOptimize (:280-293), as batched Gauss-Newton on SE(3) over n_graphs independent graphs,
 * one work-group per graph, the iteration loop on the device.
 *   d_pose        in/out, 7 doubles per node (q xyzw, t), the graphs' nodes at d_node_off /
 *                 h_node_off (int32, n_graphs + 1)
 *   d_edge_ij     int32 pairs (i, j), graph-local node indices, at d_edge_off / h_edge_off
 *   d_edge_meas   7 doubles per edge: the measured Xi^-1 Xj
 *   d_edge_var    6 variances per edge, tangent order rotation (3) then translation (3)
 *   d_prior_pose, d_prior_var   the prior on node 0 of every graph (7 and 6 doubles per graph)
 *   d_stats       n_graphs * SSF_PGO_OUT_STRIDE doubles (SSF_PGO_OUT_*), written for every graph
 *   d_cost_log    nullable; n_graphs * (max_iter + 1) doubles: the cost at every linearisation
 *                 and after the last step, NaN beyond
 * Retraction X * [Exp(w), v]; residual [Log(R_E); t_E] of E = Z^-1 Xi^-1 Xj whitened by the
 * standard deviations.  Stops when |cost_{k-1} - cost_k| <= func_tol * cost_{k-1} (func_tol 0:
 * exactly max_iter steps); steps are never rejected.  Edges with |i - j| == 1 and the prior form
 * the block-tridiagonal part; every other edge is a loop edge, at most SSF_PGO_MAX_LOOPS per
 * graph.  The host picks a graph's kernel from its counts: up to 32 edges beyond the K - 1 of a
 * chain and it is solved with a lane per right-hand side; more, and the loop edges go through in
 * passes, with a capacitance matrix of (6 min(E - (K - 1), SSF_PGO_MAX_LOOPS))^2 doubles in the
 * context scratch (18.9 MB at the cap).  One call may mix both kinds; a graph's result does not
 * depend on the rest of the batch.  A graph with more loop edges than it has edges beyond
 * K - 1 lacks a chain link and ends with SSF_PGO_NOT_PD; more than SSF_PGO_MAX_LOOPS loop edges
 * end with SSF_PGO_TOO_MANY_LOOPS and the count in SSF_PGO_OUT_LOOPS.  A graph that ends with
 * SSF_PGO_EMPTY, _BAD_INPUT, _TOO_MANY_LOOPS or _NOT_PD keeps its
 * poses bit for bit and does not affect the other graphs.  Asynchronous on stream.  SSF_E_ARG
 * (before any HIP call) on a null context or pointer, a negative count, max_iter outside
 * [0, SSF_PGO_MAX_ITER] or host offsets that do not start at 0 or decrease. */
typedef struct {
    int32_t max_iter;       /* 8: the isam->update calls of a loop closure (:281-288)  */
    double func_tol;        /* 1e-6: the front-end's Ceres function tolerance          */
} ssf_pgo_params;
#define SSF_PGO_MAX_LOOPS 256
#define SSF_PGO_MAX_ITER 1024
#define SSF_PGO_OUT_STRIDE 8
enum {
    SSF_PGO_OUT_STATUS = 0, SSF_PGO_OUT_ITERATIONS = 1, SSF_PGO_OUT_COST0 = 2, SSF_PGO_OUT_COST = 3,
    SSF_PGO_OUT_DX = 4,     /* max-norm of the last step */
    SSF_PGO_OUT_LOOPS = 5
};
enum {
    SSF_PGO_OK = 0,               /* stopped at max_iter                                       */
    SSF_PGO_CONVERGED = 1,        /* stopped by func_tol                                       */
    SSF_PGO_EMPTY = 2,            /* no nodes                                                  */
    SSF_PGO_BAD_INPUT = 3,        /* edge index outside [0, K), i == j, non-finite pose or
                                     measurement, zero quaternion, variance non-finite or <= 0 */
    SSF_PGO_TOO_MANY_LOOPS = 4,   /* more loop edges than SSF_PGO_MAX_LOOPS                    */
    SSF_PGO_NOT_PD = 5            /* Cholesky pivot <= 0 (e.g. a chain link without an edge) or
                                     a non-finite step                                         */
};
int32_t ssf_pgo_params_default(ssf_pgo_params* out);
int32_t ssf_pose_graph_batch(ssf_ctx* ctx, void* stream, int32_t n_graphs, double* d_pose,
                             const int32_t* d_node_off, const int32_t* h_node_off,
                             const int32_t* d_edge_ij, const double* d_edge_meas,
                             const double* d_edge_var, const int32_t* d_edge_off,
                             const int32_t* h_edge_off, const double* d_prior_pose,
                             const double* d_prior_var, const ssf_pgo_params* params,
                             double* d_stats, double* d_cost_log);

/* ssf_pose_graph_batch_robust is ssf_pose_graph_batch with an m-estimator on the loop edges (what
 * wrapping the loop factor's noise model in gtsam::noiseModel::Robust does) and a per-edge report.
 * With s = r^T r of an edge's whitened residual and e = sqrt(s) (GTSAM's convention):
 *   kind             weight w(s)                 2 rho(s)                          default k
 *   NONE             1                           s
 *   HUBER            1 if e <= k, else k / e     s if e <= k, else 2 k (e - k / 2)  1.345
 *   CAUCHY           k^2 / (k^2 + s)             k^2 log1p(s / k^2)                 0.1
 *   GEMAN_MCCLURE    (k^2 / (k^2 + s))^2         k^2 s / (k^2 + s)                  1.0
 * The loss applies to the loop edges (|i - j| != 1) only; chain edges and the prior stay
 * quadratic, so the block-tridiagonal part is what it is without the loss.  IRLS Gauss-Newton:
 * at every linearisation a loop edge's residual and Jacobians are scaled by sqrt(w); the cost
 * (the stop rule, SSF_PGO_OUT_COST0, SSF_PGO_OUT_COST, d_cost_log) is 0.5 * the sum of s over
 * the prior and the chain edges and of 2 rho(s) over the loop edges.  Steps are never rejected:
 * a redescending loss (Cauchy, Geman-McClure) from a far start may raise the cost.
 *   robust        nullable (NULL: kind NONE)
 *   d_edge_out    nullable; SSF_PGO_EDGE_OUT_STRIDE doubles per edge at the call's edge offsets:
 *                 the weight (1 for a chain edge) and the unweighted s, both from the evaluation
 *                 whose cost is SSF_PGO_OUT_COST; NaN for every edge of a graph that ends with
 *                 SSF_PGO_EMPTY, _BAD_INPUT, _TOO_MANY_LOOPS or _NOT_PD
 * robust NULL or of kind NONE together with d_edge_out NULL is ssf_pose_graph_batch itself (the
 * same kernels and launches).  SSF_E_ARG (before any HIP call) as ssf_pose_graph_batch, and on
 * an unknown kind or, for a kind other than NONE, k not finite or <= 0. */
typedef struct {
    int32_t kind;           /* SSF_PGO_ROBUST_*                                         */
    double k;               /* the loss's threshold / scale; unused for NONE            */
} ssf_pgo_robust;
enum {
    SSF_PGO_ROBUST_NONE = 0, SSF_PGO_ROBUST_HUBER = 1, SSF_PGO_ROBUST_CAUCHY = 2,
    SSF_PGO_ROBUST_GEMAN_MCCLURE = 3
};
#define SSF_PGO_EDGE_OUT_STRIDE 2
enum { SSF_PGO_EDGE_WEIGHT = 0, SSF_PGO_EDGE_CHI2 = 1 };
int32_t ssf_pgo_robust_default(int32_t kind, ssf_pgo_robust* out);   /* k = the table's default */
int32_t ssf_pose_graph_batch_robust(ssf_ctx* ctx, void* stream, int32_t n_graphs, double* d_pose,
                                    const int32_t* d_node_off, const int32_t* h_node_off,
                                    const int32_t* d_edge_ij, const double* d_edge_meas,
                                    const double* d_edge_var, const int32_t* d_edge_off,
                                    const int32_t* h_edge_off, const double* d_prior_pose,
                                    const double* d_prior_var, const ssf_pgo_params* params,
                                    double* d_stats, double* d_cost_log,
                                    const ssf_pgo_robust* robust, double* d_edge_out);

/* ssf_pose_graph_batch_lm is ssf_pose_graph_batch_robust with Levenberg-Marquardt step control
 * (Ceres' LevenbergMarquardtStrategy, the step rule of the front-end's solve): no step is taken
 * that does not lower the cost.  One attempt solves (H + D / radius) dx = -g, H = J^T J over every
 * factor (the loop rows scaled by the loss), D = diag(H) clamped to [1e-6, 1e32], and evaluates
 * the trial point X (+) dx.  With mcc = -(g^T dx + dx^T H dx / 2), the decrease the model promises,
 * and rho = (cost - trial cost) / mcc:
 *   rho > min_relative_decrease   accepted: radius = min(radius / max(1/3, 1 - (2 rho - 1)^3),
 *                                 max_radius), the divisor of the next rejection back to 2; stops
 *                                 with SSF_PGO_CONVERGED when func_tol > 0 and the cost fell by no
 *                                 more than func_tol * (the cost before)
 *   otherwise (a NaN trial cost too)   rejected: radius /= divisor, divisor *= 2; X stays
 *   a failed Cholesky pivot of the damped system, a non-finite step or not (mcc > 0)   invalid:
 *                                 radius and divisor as for a rejection, no trial point
 * params->max_iter bounds the attempts.  The solve also ends (SSF_PGO_OK) after more than five
 * invalid attempts in a row or when a rejection or acceptance leaves radius < min_radius.  The
 * poses written back are the last accepted point, so SSF_PGO_OUT_COST <= SSF_PGO_OUT_COST0;
 * SSF_PGO_OUT_ITERATIONS counts the attempts, SSF_PGO_OUT_DX is the max-norm of the last accepted
 * step (0: none), SSF_PGO_OUT_ACCEPTED the accepted attempts, SSF_PGO_OUT_RADIUS the final radius
 * (these two are 0 from the other entry points); d_cost_log[a] is the cost after attempt a, so it
 * never rises (a rejected or invalid attempt repeats the entry before it); d_edge_out belongs to
 * the last accepted point.  A missing chain link still ends with SSF_PGO_NOT_PD.
 *   lm        nullable: with d_lm_log NULL too this is ssf_pose_graph_batch_robust itself, launch
 *             for launch
 *   d_lm_log  nullable; n_graphs * max_iter * SSF_PGO_LM_LOG_STRIDE doubles, per attempt the trial
 *             cost (NaN for an invalid attempt), mcc (NaN when the step itself failed), the radius
 *             after the attempt and the outcome (SSF_PGO_LM_*); NaN for the attempts not made and
 *             for every attempt of a graph that ends with SSF_PGO_EMPTY, _BAD_INPUT,
 *             _TOO_MANY_LOOPS or _NOT_PD
 * SSF_E_ARG (before any HIP call) as ssf_pose_graph_batch_robust, and on radius0, max_radius or
 * min_radius not finite or <= 0, min_radius > max_radius, min_relative_decrease outside [0, 1),
 * or d_lm_log without lm. */
typedef struct {
    double radius0;                 /* 1e4: Ceres' initial_trust_region_radius                 */
    double min_relative_decrease;   /* 1e-3                                                    */
    double max_radius;              /* 1e16                                                    */
    double min_radius;              /* 1e-32                                                   */
} ssf_pgo_lm;
enum { SSF_PGO_OUT_ACCEPTED = 6, SSF_PGO_OUT_RADIUS = 7 };
#define SSF_PGO_LM_LOG_STRIDE 4
enum { SSF_PGO_LM_LOG_COST = 0, SSF_PGO_LM_LOG_MCC = 1, SSF_PGO_LM_LOG_RADIUS = 2, SSF_PGO_LM_LOG_OUTCOME = 3 };
enum { SSF_PGO_LM_REJECTED = 0, SSF_PGO_LM_ACCEPTED = 1, SSF_PGO_LM_INVALID = 2 };
int32_t ssf_pgo_lm_default(ssf_pgo_lm* out);
int32_t ssf_pose_graph_batch_lm(ssf_ctx* ctx, void* stream, int32_t n_graphs, double* d_pose,
                                const int32_t* d_node_off, const int32_t* h_node_off,
                                const int32_t* d_edge_ij, const double* d_edge_meas,
                                const double* d_edge_var, const int32_t* d_edge_off,
                                const int32_t* h_edge_off, const double* d_prior_pose,
                                const double* d_prior_var, const ssf_pgo_params* params,
                                double* d_stats, double* d_cost_log,
                                const ssf_pgo_robust* robust, double* d_edge_out,
                                const ssf_pgo_lm* lm, double* d_lm_log);

#ifdef __cplusplus
}
#endif
#endif
