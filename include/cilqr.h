/*
 * cilqr.h — C-ABI of the MI355X-native batched constrained-iLQR (CILQR) solver and costmap warp.
 *
 * Drop-in boundary for the hot path of Leo-Liao-Chao/Uncertainty-Aware-CILQR-for-Trajectory-Optimization.
 * All citations are relative to the reference tree, with I/ = CILQR/src/ilqr/include/ilqr/,
 * M/ = CILQR/src/map_engine/, G/ = CILQR/src/grid_map/.
 *
 * The reference has no FFI layer: the planner node calls C++ methods on a stateful `iLQR` object
 * (I/iLQR.h:16-59).  This header is what a binding for that path would bind instead:
 *
 *   reference interface                                      replaced by
 *   -------------------------------------------------------  ------------------------------------
 *   Parameters::Parameters()            I/Parameters.cpp:3-75   cilqr_params_default
 *   iLQR::iLQR(const Parameters&)       I/iLQR.cpp:3-19         cilqr_create (+ cilqr_default_control_seq)
 *   iLQR::get_optimal_control_seq       I/iLQR.cpp:201-245      cilqr_solve_batch / cilqr_solve_batch_device
 *   iLQR::set_Obstacle / clear_Obstacle I/iLQR.cpp:20-27        obs_* arguments of cilqr_solve_batch (M = 0 ⇒ cleared), or
 *                                                                one shared / horizon-constant set: cilqr_solve_batch_obstacles(_device)
 *   iLQR::set_uncertainty_map / clear_uncertainty_map I/iLQR.cpp:28-35   cilqr_set_uncertainty_map(_device) / cilqr_clear_uncertainty_map
 *   Constraints::get_J                  I/Constraints.cpp:534-561   J_out of cilqr_solve_batch
 *   GridMapRosConverter::from/toOccupancyGrid G/grid_map_ros/src/GridMapRosConverter.cpp:225-307
 *                                                                cilqr_occupancy_to_layer / cilqr_layer_to_occupancy(_device)
 *   LocalCostmap::odomCallback (one frame) M/src/local_costmap.cpp:172-305 cilqr_costmap_frame_device
 *   odomCallback for the node's K pose-noise candidates I/ilqr_uncertainty_node.cpp:82-113
 *                                                                cilqr_costmap_frame_batch_device (K frames, two launches)
 *   LocalPlanner::get_local_plan(_coeffs) I/LocalPlanner.cpp:25-117 cilqr_local_plan (host pre-step),
 *                                                                cilqr_local_plan_batch(_device) (B candidates on the device)
 *   LocalCostmap::odomCallback warp loop M/src/local_costmap.cpp:242-264 cilqr_warp_costmap(_device)
 *   LocalCostmap::bondingBoxHandle      M/src/local_costmap.cpp:860-922  cilqr_boxes_to_polygons (corner arithmetic, host) +
 *                                                                cilqr_rasterize_polygons(_device); fused into the warp and the
 *                                                                frame: cilqr_warp_costmap_polygons_device,
 *                                                                cilqr_costmap_frame_polygons_device
 *   thrust_propagateUncertainty     M/src/arbitrary_transformation.cu:8-157  cilqr_blur_costmap(_device),
 *                                                                cilqr_blur_costmap_batch_device (K headings per launch)
 *   (none: batch min-cost selection is new)      cilqr_argmin_device, cilqr_argmin_global_device (RCCL),
 *                                                                cilqr_create_multi / cilqr_multi_solve_batch
 *   (none: the reference never compares candidates)          cilqr_score_batch(_device), cilqr_score_batch_sampled(_device):
 *                                                                full cost, worst constraint, collision share of solved candidates
 *   iLQR::backward_pass's k, K (computed, never handed out)   cilqr_gains_batch(_device): the gains of one backward pass
 *   iLQR::forward_pass's control law from other starts (none)  cilqr_rollout_batch(_device), cilqr_score_rollouts(_device):
 *                                                                closed-loop rollouts from offset starts, collision risk per solve
 *                                                                cilqr_rollout_risk(_device): that risk in one launch, no rollout stored
 *                                                                cilqr_gains_batch_sampled, cilqr_rollout_risk_sampled(_device): both
 *                                                                for sampled obstacles in compact form
 *   (none: the reference propagates no state covariance)     cilqr_chance_risk(_device): closed-loop covariance along the plan
 *                                                                and Gaussian chance values per obstacle and step, no samples
 *                                                                cilqr_tighten_obstacles(_device): obstacles inflated by that
 *                                                                covariance for a warm-started re-solve; cilqr_chance_kappa
 *                                                                cilqr_tighten_map(_device): the costmap dilated by it instead
 *   LocalCostmap's cv::KalmanFilter on ONE bounding box  M/src/local_costmap.cpp:138-158, 351-380
 *                                                                cilqr_track_update(_device): the boxes of cilqr_map_obstacles
 *                                                                followed across ticks — association, birth and death of tracks
 *
 * Conventions
 *   - fp64 everywhere in the solver; float32 map payloads in the warp.
 *   - Per-solve layouts equal Eigen column-major as used by the reference and by
 *     vehiclepub/Experiment.msg flattening (I/ilqr_uncertainty_node.cpp:265-274):
 *       U  : [a0, w0, a1, w1, ...]               2*N doubles
 *       X  : [x0, y0, v0, th0, x1, ...]          4*(N+1) doubles
 *       obstacle pose (relative_pos_array, I/Obstacle.h:25) : 4*N doubles, column t = (x, y, v, theta)
 *       obstacle dimension (I/Obstacle.h:24)                : 2*N doubles, column t = (length, width)
 *     The batch index is outermost, then (for obstacle tables) the obstacle index.
 *   - Every function returns 0 on success and a negative cilqr_status on failure; the message is
 *     available from cilqr_last_error() (thread-local).  Nothing is printed to stdout.
 *   - One handle = one device = one host thread at a time (the reference solver is not re-entrant
 *     either: `static int iteration_times`, I/iLQR.cpp:208).
 *   - There is NO CPU fallback: every compute entry point fails with CILQR_ERR_NO_DEVICE when no
 *     gfx950 device is usable.
 */
#ifndef CILQR_H_
#define CILQR_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CILQR_NX 4
#define CILQR_NU 2
#define CILQR_POLY_COEFFS 6   /* poly_order + 1, I/Parameters.cpp:7 */
#define CILQR_MAX_HORIZON 384  /* per-solve arrays of the LDS-resident family at the default sample count: 98 KiB of 160 */
#define CILQR_ABI_VERSION 2
#define CILQR_COMM_ID_BYTES 128 /* an RCCL ncclUniqueId, carried opaquely */
#define CILQR_MAX_POLYGONS 1024        /* obstacle polygons per rasterisation call */
#define CILQR_MAX_POLYGON_VERTICES 16  /* vertices per polygon (at least 3) */

/* Field-for-field POD mirror of class Parameters (I/Parameters.h:5-91) — only the fields the
 * constructor initialises (I/Parameters.cpp:6-74) — plus the two constants iLQR::iLQR sets
 * (lamb_factor, lamb_max; I/iLQR.cpp:17-18). */
typedef struct cilqr_params {
  /* planning parameters */
  int32_t num_of_local_wpts;   /* 20  */
  int32_t poly_order;          /* 5   */
  /* iLQR parameters */
  int32_t horizon;             /* 40  */
  int32_t max_iterations;      /* 20  */
  int32_t num_states;          /* 4   */
  int32_t num_ctrls;           /* 2   */
  double desired_speed;        /* 5.0 */
  double timestep;             /* 0.1 */
  double tolerance;            /* 1e-4 */
  /* cost weights */
  double w_acc, w_yawrate;     /* 1.0, 4.0 */
  double w_pos, w_vel;         /* 0.65, 3.0 */
  double w_obstacle, w_uncertainty; /* 1.0, 1.0 */
  /* barrier q1/q2 */
  double q1_acc, q2_acc;
  double q1_yawrate, q2_yawrate;
  double q1_front, q2_front;
  double q1_rear, q2_rear;
  double q1_uncertainty, q2_uncertainty;
  /* limits */
  double acc_max, acc_min;
  double steer_angle_min, steer_angle_max;
  /* ego vehicle */
  double wheelbase, speed_max;
  double steer_control_max, steer_control_min;
  double throttle_control_max, throttle_control_min;
  /* obstacle parameters */
  double t_safe, s_safe_a, s_safe_b;
  double ego_rad, ego_front, ego_rear;
  double length, width;
  double safe_length, safe_width;
  /* iLQR::iLQR, I/iLQR.cpp:17-18 */
  double lamb_factor, lamb_max;
} cilqr_params;

typedef enum cilqr_status {
  CILQR_OK = 0,
  CILQR_ERR_ARG = -1,        /* bad argument (null pointer, size out of the range given at create) */
  CILQR_ERR_NO_DEVICE = -2,  /* no usable gfx950 device / HIP runtime error at create */
  CILQR_ERR_HIP = -3,        /* HIP runtime error during a call */
  CILQR_ERR_UNSUPPORTED = -4,/* parameter combination the kernels do not implement (e.g. num_states != 4) */
  CILQR_ERR_COMM = -5,       /* RCCL error in the cross-GPU exchange step */
  CILQR_ERR_INTERNAL = -6    /* a kernel's loop bound ran out: a defect of this library, reported instead of a hang */
} cilqr_status;

/* Per-solve exit reason written to status_out (I/iLQR.cpp:211-239). */
typedef enum cilqr_exit {
  CILQR_EXIT_TOLERANCE = 0,   /* accepted step with |J_new - J_old| < tolerance  (:225-228) */
  CILQR_EXIT_LAMBDA_MAX = 1,  /* rejected step drove lamb above lamb_max         (:232-236) */
  CILQR_EXIT_MAX_ITER = 2,    /* loop ran max_iterations times                   (:211)     */
  CILQR_EXIT_NUMERIC = 3      /* non-finite value met in the backward pass (reference: EigenSolver
                                 failure → break, :214-215); X/U of the last accepted iterate */
} cilqr_exit;

/* Flags for cilqr_solve_batch*. */
#define CILQR_FLAG_NONE 0u
/* Execute the backward/forward passes of rejected iterations exactly as the reference loop does
 * instead of stopping at the first rejection (results are identical). */
#define CILQR_FLAG_FAITHFUL_ITERS 1u
/* Test hook: every solve is handed to the GENERAL kernels (branching passes, library-range sincos of every heading, the regularised
 * Q_uu inverse in its eigenvalue-clamping form and the value update as the reference's direct product K' Q_uu) — the path
 * that otherwise only solves take which the production kernels do not cover.  Same results to rounding, several times slower. */
#define CILQR_FLAG_GENERAL_ONLY 2u

typedef struct cilqr_handle cilqr_handle;

/* Geometry of a grid_map layer (G/grid_map_core/src/GridMap.cpp:45-62): float32, column-major
 * rows×cols, cell (i,j) centre = pos + (len/2 - res/2) - res*(i,j)  (GridMapMath.cpp:114-127).
 * Fill it with cilqr_map_geom_set.  Where a geometry is the SOURCE of a warp (src_geom of cilqr_warp_costmap*, global_geom of
 * cilqr_costmap_frame*) its lengths must be exactly what setGeometry writes: len_x == (double)rows * res and
 * len_y == (double)cols * res, bit for bit.  Any other value is CILQR_ERR_ARG (the message names the field) before anything is
 * enqueued: the warp kernels' in-map test relies on that equality. */
typedef struct cilqr_map_geom {
  int32_t rows, cols;     /* size_(0), size_(1)  */
  double res;             /* resolution_ */
  double len_x, len_y;    /* length_  (= (double)size*res after setGeometry; REQUIRED of a warp's source geometry) */
  double pos_x, pos_y;    /* position_ (map centre in its parent frame) */
} cilqr_map_geom;

/* The costmap the uncertainty cost reads.  The reference constructs, every tick,
 *   Uncertainty vehicle_map(params, map_msg, grid_map_msg, x_center, y_center, SIGMA_X, SIGMA_Y, SIGMA_THETA, 0, 0, nh)
 * (I/ilqr_uncertainty_node.cpp:111-112) and hands it to iLQR::set_uncertainty_map (:113); class Uncertainty itself is ABSENT
 * from the reference repository.  What those arguments carry is mirrored here: the blurred occupancy layer
 * the map node publishes (grid_map_msg, layer "uncertainty_map" = output of cilqr_blur_costmap*, values 0..100, NaN unknown),
 * its vehicle-frame geometry with the centre at (x_center, y_center) (map_param, M/src/local_costmap.cpp:793-799), and the pose
 * of that vehicle frame in the planning frame (map_msg.info.origin = the vehicle pose at map time, :300).  The sigmas were
 * consumed upstream by the blur.  THE ARITHMETIC OF THE COST IS DEFINED BY THIS LIBRARY (below, at
 * cilqr_set_uncertainty_map): there is no reference arithmetic to match — parity unpinned. */
typedef struct cilqr_uncertainty_map {
  const float* layer;      /* rows*cols float32, column-major */
  cilqr_map_geom geom;     /* vehicle-frame geometry of the layer */
  double pose_x, pose_y, pose_theta; /* vehicle frame in the planning frame */
  const double* poses;     /* NULL, or [B][3] per-solve (pose_x, pose_y, pose_theta): then the three scalars are ignored */
  int64_t layer_stride;    /* floats from solve b's layer to solve b+1's; 0: one layer shared by the batch */
  int32_t probes_l, probes_w; /* footprint probe grid along / across the ego heading, each >= 1 */
} cilqr_uncertainty_map;

/* --- parameters ------------------------------------------------------------------------------- */
void cilqr_params_default(cilqr_params* p);             /* I/Parameters.cpp:3-75 + I/iLQR.cpp:17-18 */
int  cilqr_abi_version(void);
int  cilqr_device_count(void);  /* gfx950 devices this process can use (0: none; there is no CPU path) */
const char* cilqr_last_error(void);

/* Initial warm-start control sequence of a fresh planner (I/iLQR.cpp:9-15): row 0 = 0.5, row 1 = 0 for
 * the first N/2 steps then 0.1.  Writes 2*N doubles. */
int cilqr_default_control_seq(int N, double* U);

/* --- host pre-step (stays on the host) -------------------------------------- */
/* LocalPlanner::{closest_point_index,get_local_wpts,get_local_plan,get_local_plan_coeffs,polyfit}
 * (I/LocalPlanner.cpp:25-117).  path: 2×P column-major.  Outputs: coeffs[poly_order+1]; ref_traj 2×n_out
 * column-major (row 0 = waypoint x, row 1 = fitted y), n_out ≤ num_of_local_wpts written to *n_out. */
int cilqr_local_plan(const cilqr_params* p, const double* path, int P, const double* ego_state,
                     double* coeffs, double* ref_traj, int* n_out);

/* The same pre-step for B candidate ego poses at once, on the device, so that a batch solve can start
 * from raw (global_path, ego): candidate b reads its 2×P column-major path at path + b*path_stride doubles
 * (path_stride = 0: one path shared by all candidates, the reference's set_global_plan).  ego [B][4];
 * outputs poly [B][6] (coefficients past poly_order are 0), xplan_fl [B][2] (first and last x of the slice, the two
 * elements of x_local_plan the solve reads), ref_traj [B][2*num_of_local_wpts] or NULL (2×n column-major per candidate,
 * the tail past n untouched), n_out [B] or NULL.  The fit is the host pre-step's, sum for sum; the Vandermonde entries are
 * correctly rounded powers where the host uses libm's pow (see local_plan.hip).  Uses the handle's num_of_local_wpts and
 * poly_order (≤ 5).  The *_device form takes device pointers and is asynchronous on `stream`. */
int cilqr_local_plan_batch(cilqr_handle* h, int B, int P, const double* path, int64_t path_stride, const double* ego,
                           double* poly, double* xplan_fl, double* ref_traj, int32_t* n_out);
int cilqr_local_plan_batch_device(cilqr_handle* h, void* stream, int B, int P, const double* path, int64_t path_stride,
                                  const double* ego, double* poly, double* xplan_fl, double* ref_traj, int32_t* n_out);

/* --- solver ----------------------------------------------------------------------------------- */
/* Sizes are upper bounds; device workspaces are allocated once here, never in solve. device = HIP
 * ordinal. */
int cilqr_create(const cilqr_params* p, int max_batch, int max_horizon, int max_obstacles, int device,
                 cilqr_handle** out);
int cilqr_destroy(cilqr_handle* h);

/* Page-locked host memory for the buffers handed to the host-buffer entry points: from such memory their copies are
 * asynchronous DMA transfers; any other host memory works too (the HIP runtime then stages each copy).  Returns NULL on failure. */
void* cilqr_host_alloc(size_t bytes);
int   cilqr_host_free(void* p);

/* Batched iLQR::get_optimal_control_seq (I/iLQR.cpp:201-245) — host buffers, synchronous.
 * Nothing is allocated per call: the device arena and a pinned staging buffer are sized at cilqr_create.  A call whose arrays
 * total ≤ 1 MiB (the drop-in B = 1 tick, a handful of candidates) travels as one packed host→device and one device→host copy.
 *   x0        [B][4]            ego state (x, y, v, theta)
 *   U         [B][2*N]  in/out  warm start in, U_result out (I/iLQR.cpp:222,244)
 *   poly      [B][6]            poly_coeffs, ascending powers
 *   xplan_fl  [B][2]            first and last element of x_local_plan (the only ones read,
 *                               I/Constraints.cpp:31-33)
 *   obs_pose  [B][M][4*N], obs_dim [B][M][2*N]   (ignored when M == 0)
 *   obs_weight[B][M] or NULL    per-obstacle factor applied where the reference applies
 *                               Parameters::w_obstacle (I/Constraints.cpp:184-185); NULL ⇒ p.w_obstacle
 *   X_out     [B][4*(N+1)]      X_result
 *   J_out     [B]               Constraints::get_J(X_result, U_result)
 *   iters_out [B]               iteration_times of the reference loop (I/iLQR.cpp:212)
 *   status_out[B]               cilqr_exit
 * J_out / iters_out / status_out may be NULL. */
int cilqr_solve_batch(cilqr_handle* h, int B, int N, int M,
                      const double* x0, double* U, const double* poly, const double* xplan_fl,
                      const double* obs_pose, const double* obs_dim, const double* obs_weight,
                      double* X_out, double* J_out, int32_t* iters_out, int32_t* status_out,
                      uint32_t flags);

/* Same, with every pointer a DEVICE pointer on the handle's device and the work enqueued on `stream`
 * (a hipStream_t passed as void*; NULL = the HIP null stream, as everywhere in HIP).  Asynchronous: returns after launch.
 * The handle's device workspaces (obstacle table, grouped-family arrays, hand-over flags) serve ONE solve at a time: calls
 * enqueued on the same stream follow each other and are fine; solves that may overlap in time on different streams need
 * different handles.
 * Scheduling: a batch of more solves than the device has SIMDs is dispatched longest-first by the pass counts the solves of
 * the PREVIOUS call on this handle had (same B, same stream: a planner solves nearly the same scenes tick after tick).  This
 * only changes which solves start first — results are bit-identical for any order — and is switched off by
 * CILQR_NO_SCHEDULE_HINT in the environment at cilqr_create. */
int cilqr_solve_batch_device(cilqr_handle* h, void* stream, int B, int N, int M,
                             const double* x0, double* U, const double* poly, const double* xplan_fl,
                             const double* obs_pose, const double* obs_dim, const double* obs_weight,
                             double* X_out, double* J_out, int32_t* iters_out, int32_t* status_out,
                             uint32_t flags);

/* Obstacle inputs addressed by strides.  Units are ENTRIES: one entry = 4 pose doubles (x, y, v, theta) at pose + 4e and
 * 2 dimension doubles (length, width) at dim + 2e.  Obstacle m of solve b at step t is entry
 *     e = b*batch_stride + m*obstacle_stride + t*step_stride.
 * cilqr_solve_batch's layout is (M*N, N, 1).  One scene shared by the batch: batch_stride = 0.  Constant over the horizon:
 * step_stride = 0 (e.g. (0, 1, 0) = one static obstacle set for every solve, M entries in all). */
typedef struct cilqr_obstacles {
  const double* pose;
  const double* dim;
  const double* weight;          /* NULL => p.w_obstacle; else weight[b*weight_batch_stride + m] */
  int64_t batch_stride, obstacle_stride, step_stride;
  int64_t weight_batch_stride;   /* 0 = one weight vector [M] for the batch */
} cilqr_obstacles;

/* cilqr_solve_batch with the obstacles given by strides (above): the same results, bit for bit, as cilqr_solve_batch on the dense
 * expansion of the same inputs, for every flag and kernel family, with or without an uncertainty map.  obs may be NULL only when
 * M == 0; a negative stride is CILQR_ERR_ARG.  Only the span of entries the strides address is copied,
 * (B-1)·batch_stride + (M-1)·obstacle_stride + (N-1)·step_stride + 1 entries, which must fit the B·M·N reserved at create.
 * With one scene for the batch (batch_stride = 0 and weight_batch_stride = 0 or no weights), kernels that keep the obstacle
 * table in device memory instead of LDS build it ONCE per call, in front of the solves, and every solve reads that copy. */
int cilqr_solve_batch_obstacles(cilqr_handle* h, int B, int N, int M, const double* x0, double* U, const double* poly,
                                const double* xplan_fl, const cilqr_obstacles* obs, double* X_out, double* J_out,
                                int32_t* iters_out, int32_t* status_out, uint32_t flags);
/* The same with every pointer (those inside *obs included) a DEVICE pointer, asynchronous on `stream` as
 * cilqr_solve_batch_device.  *obs itself is a host struct, read before the call returns. */
int cilqr_solve_batch_obstacles_device(cilqr_handle* h, void* stream, int B, int N, int M, const double* x0, double* U,
                                       const double* poly, const double* xplan_fl, const cilqr_obstacles* obs, double* X_out,
                                       double* J_out, int32_t* iters_out, int32_t* status_out, uint32_t flags);

/* --- path-aligned planning frame ---------------------------------------------------------------------------------------
 * The fit above is y(x) in map coordinates: ill-conditioned at |x| of a few hundred metres, and meaningless for a road that
 * runs along y (its abscissae coincide).  The calls below plan in a frame of each solve's own instead.  Nothing in a solve,
 * score, gains, risk or check kernel changes: they are handed framed inputs and their states are taken back out.
 *
 * Frame of solve b.  first = closest_point_index and n = the slice length, both exactly as cilqr_local_plan_batch has them.
 *   origin  (ox, oy) = waypoint `first`;   chord  dx = x[first+n-1] - ox,  dy = y[first+n-1] - oy
 *   h = sqrt(dx*dx + dy*dy)   (two rounded products, one rounded sum, a correctly rounded square root)
 *   c = dx / h,  s = dy / h   (correctly rounded divisions),   phi = atan2(s, c)
 * A frame record is CILQR_FRAME_DOUBLES doubles (ox, oy, c, s, phi).  When n < 2, h == 0 or h is not finite the frame is the
 * translation alone (c = 1, s = 0, phi = 0) and the solve's info word carries CILQR_FRAME_DEGENERATE.  CILQR_FRAME_NOT_MONOTONE
 * is set when the slice's framed abscissae are not strictly increasing, x'[i+1] > x'[i] false for some i (a NaN included): the
 * slice turns by more than a quarter turn against its chord and the fit is as meaningless as the unframed one's.  It is
 * reported, not repaired.
 * Arithmetic, in this order, every product, sum and difference rounded on its own (no fused multiply-add):
 *   into the frame    ux = x - ox,  uy = y - oy;   x' = (c*ux) + (s*uy),   y' = (c*uy) - (s*ux);   theta' = theta - phi
 *   out of the frame  x = ((c*x') - (s*y')) + ox,  y = ((s*x') + (c*y')) + oy;                      theta  = theta' + phi
 * Headings are not wrapped; v is untouched.
 * NOT transformed by these calls: covariances of the EGO state (Sigma0, W of the chance risks, the rollout offsets).  A
 * covariance whose position block is isotropic (the node's sigma_x = sigma_y = 0.16) is the same in every frame. */
#define CILQR_FRAME_DOUBLES 5
#define CILQR_FRAME_DEGENERATE 1   /* info bit: translation only */
#define CILQR_FRAME_NOT_MONOTONE 2 /* info bit: framed abscissae of the slice not strictly increasing */
#define CILQR_FRAME_TO 0           /* direction of cilqr_frame_states: map -> frame */
#define CILQR_FRAME_FROM 1         /* frame -> map */
#define CILQR_FRAME_GLOBAL_INFLATION 1u /* flags of cilqr_frame_obstacles, below */

/* cilqr_local_plan_batch in the frame: the frame is chosen from the slice, every waypoint of the slice is taken into it and
 * the Vandermonde rows are formed from the framed abscissae (the fit itself is the same code).  path, path_stride, ego, poly,
 * ref_traj, n_out as there; frames [B][5], info [B], ego_out [B][4] = the ego state in the frame, the x0 of the solve;
 * xplan_fl [B][2] and ref_traj are in frame coordinates; first_out [B] or NULL = closest_point_index.  ego_out must not be ego. */
int cilqr_local_plan_frames(cilqr_handle* h, int B, int P, const double* path, int64_t path_stride, const double* ego,
                            double* frames, int32_t* info, double* ego_out, double* poly, double* xplan_fl, double* ref_traj,
                            int32_t* n_out, int32_t* first_out);
int cilqr_local_plan_frames_device(cilqr_handle* h, void* stream, int B, int P, const double* path, int64_t path_stride,
                                   const double* ego, double* frames, int32_t* info, double* ego_out, double* poly,
                                   double* xplan_fl, double* ref_traj, int32_t* n_out, int32_t* first_out);

/* Obstacle rows into the frames: the dense table pose_out [B][M][4N], dim_out [B][M][2N] (cilqr_solve_batch's layout) from
 * obstacles in any strides; solve b uses the record at frames + b*frame_stride (frame_stride 5, or 0: one frame for the batch).
 * Positions and headings as above; v is copied.  obs_cov (NULL, or (xx, xy, yy) per entry at obs_cov + 3e) is rotated to
 * cov_out [B][M][3N] as T C T' with T = (c s; -s c):  m00 = c*xx + s*xy, m01 = c*xy + s*yy, m10 = c*xy - s*xx, m11 = c*yy - s*xy;
 * xx' = m00*c + m01*s, xy' = m01*c - m00*s, yy' = m11*c - m10*s.  Obstacle weights are frame-free and not read.
 * flags.  The reference inflates an obstacle's ellipse by |v cos theta_o| t_safe along and |v sin theta_o| t_safe across with
 * theta_o in the PLANNING frame (I/Obstacle.cpp:42-43), so a moving obstacle gets a different ellipse in a turned frame.
 *   0 (default): dim_out = dim; the reference's arithmetic simply runs in the frame.
 *   CILQR_FRAME_GLOBAL_INFLATION: dim_out is compensated so that the solver forms the map frame's semi-axes:
 *     L' = L + (2 t_safe) * (|v*cos theta_o| - |v*cos theta_o'|),  W' = W + (2 t_safe) * (|v*sin theta_o| - |v*sin theta_o'|),
 *     sines and cosines by the kernels' own sincos (cilqr_debug_math, CILQR_MATH_SINCOS_FAST).
 * Static obstacles (v = 0) are the same either way.
 * pose_out, dim_out and cov_out must not overlap obs->pose, obs->dim and obs_cov: with shared strides many lanes read an entry that
 * another lane's output would overwrite.  The host form takes every B <= max_batch, whatever the strides: its table travels through
 * scratch the handle grows on first use, not through the arena of the other host forms. */
int cilqr_frame_obstacles(cilqr_handle* h, int B, int N, int M, const double* frames, int64_t frame_stride,
                          const cilqr_obstacles* obs, const double* obs_cov, uint32_t flags, double* pose_out, double* dim_out,
                          double* cov_out);
int cilqr_frame_obstacles_device(cilqr_handle* h, void* stream, int B, int N, int M, const double* frames, int64_t frame_stride,
                                 const cilqr_obstacles* obs, const double* obs_cov, uint32_t flags, double* pose_out,
                                 double* dim_out, double* cov_out);

/* Rows [B*S][4(N+1)] of states into (CILQR_FRAME_TO) or out of (CILQR_FRAME_FROM) the frame of solve row / S: the X_out of a
 * solve (S = 1), rollouts, stop rows.  X_out may be X_in.  B*S must not exceed max_batch. */
int cilqr_frame_states(cilqr_handle* h, int B, int S, int N, const double* frames, int64_t frame_stride, int direction,
                       const double* X_in, double* X_out);
int cilqr_frame_states_device(cilqr_handle* h, void* stream, int B, int S, int N, const double* frames, int64_t frame_stride,
                              int direction, const double* X_in, double* X_out);

/* Poses (x, y, theta) into the frames: pose_in [B][K][3] at pose_in + b*pose_stride (pose_stride 0: one set [K][3] for the
 * batch, else at least 3K) -> pose_out [B][K][3].  With K = 1 the map pose becomes the [B][3] `poses` of
 * cilqr_set_uncertainty_map_device: the map cost, cilqr_rollout_risk_map, cilqr_footprint_check and cilqr_map_clearance then
 * read the map from framed plans unchanged.  B*K must not exceed max_batch*max_horizon. */
int cilqr_frame_poses(cilqr_handle* h, int B, int K, const double* frames, int64_t frame_stride, const double* pose_in,
                      int64_t pose_stride, double* pose_out);
int cilqr_frame_poses_device(cilqr_handle* h, void* stream, int B, int K, const double* frames, int64_t frame_stride,
                             const double* pose_in, int64_t pose_stride, double* pose_out);

/* --- costmap-lookup uncertainty cost ------------------------------------------------------------------
 * iLQR::set_uncertainty_map / clear_uncertainty_map (I/iLQR.cpp:28-35 → I/Constraints.cpp:520-528): while a map is set, every
 * later solve on the handle adds  w_uncertainty · (vx, mx)  of the map cost to l_x, l_xx at every step, exactly where
 * Constraints::get_state_cost does (I/Constraints.cpp:188-201); get_J is unchanged (its uncertainty term is commented out in the
 * reference, :553-557).  The cost itself — Uncertainty::get_uncertainty_cost(state) → {x, vx(4), mx(4×4)} — has NO source in the
 * reference; this library defines it, using only the reference's own ingredients:
 *   footprint  probes_l × probes_w points on the rectangle safe_length × safe_width (Parameters, launch 1.1 / 0.9) centred on the
 *              state's (x, y) and turned by its heading: body offsets a_k = -safe_length/2 + k·safe_length/(probes_l-1)
 *              (0 when probes_l = 1), b_l likewise across;
 *   lookup     each probe → vehicle frame (rigid transform by the map pose) → bilinear interpolation of the layer over the four
 *              surrounding cell centres, as GridMap::atPositionLinearInterpolated does (G/grid_map_core/src/GridMap.cpp:770-837),
 *              evaluated in double, with the interpolant's own gradient; a probe whose four cells are not all inside the map
 *              and finite contributes nothing;
 *   barrier    the reference's exponential barrier and Gauss-Newton form (Obstacle::barrier_function, I/Obstacle.cpp:21-32) with
 *              c = occupancy/100 - 1:  x = q1·exp(q2·c),  vx = q2·x·∇c,  mx = q2²·x·∇c∇cᵀ,  q1 = q1_uncertainty,
 *              q2 = q2_uncertainty (I/Parameters.cpp:41-42); ∇c is taken with respect to (x, y) only — the heading's effect on the
 *              probe positions is ignored, as the reference ignores it for its ego circles (I/Obstacle.cpp:75-78);
 *   result     the mean over the probes.
 *   omitted    (stated so that nobody reads more into vx, mx than is there) vx has no heading entry: d/dθ of the cost through the
 *              turning footprint is dropped (vx[2] = vx[3] = 0); mx is the Gauss-Newton outer product only: the interpolant's own
 *              curvature (the bilinear cross term ∂²o/∂x∂y) and every θ row and column are dropped.  The x, y entries of vx ARE
 *              the exact derivative of the cost at fixed heading (checked by finite differences, tests/test_oracle.py and the
 *              -m gpu twin on the kernel's own value).
 * cilqr_set_uncertainty_map_device: every pointer in *map is a device pointer that must stay valid (and is read) during later
 * solves — e.g. the uncertainty_layer cilqr_costmap_frame_device wrote on the same stream.  cilqr_set_uncertainty_map: host
 * pointers; one shared layer (layer_stride = 0, poses = NULL) copied into a buffer the handle owns.  Both return
 * CILQR_ERR_ARG for probes < 1 or a bad geometry. */
int cilqr_set_uncertainty_map_device(cilqr_handle* h, const cilqr_uncertainty_map* map);
int cilqr_set_uncertainty_map(cilqr_handle* h, const cilqr_uncertainty_map* map);
int cilqr_clear_uncertainty_map(cilqr_handle* h);

/* Test hook: the map cost alone at n states (host buffers, [n][4]) against the map currently set (solve index 0's layer and
 * pose) → cost[n], vx[n][2] (the x, y entries; the others are zero), mx[n][3] (xx, xy, yy). */
int cilqr_debug_uncertainty_cost(cilqr_handle* h, int n, const double* states, double* cost, double* vx, double* mx);

/* Sampled obstacles (the "uncertainty-aware" batch of BASELINE config 3: n_obs moving obstacles × n_samples Gaussian pose
 * samples, every sample an Obstacle of its own with Parameters::w_obstacle = 1/n_samples, I/Constraints.cpp:177-187).
 * Exactly cilqr_solve_batch(_device) with M = n_obs·n_samples obstacles where obstacle m = o·n_samples + s has
 *   pose[t] = (x_o[t] + dx, y_o[t] + dy, v_o[t], theta_o[t] + dtheta),  dim[t] = dim_o[t],  weight = sample_weight,
 * (dx, dy, dtheta) = sample_offset[b][o][s], but taking the compact form: the materialised tables are n_samples times
 * larger and, not fitting on chip, would be streamed from HBM once per iteration.
 *   nom_pose [B][n_obs][4*N], nom_dim [B][n_obs][2*N], sample_offset [B][n_obs][n_samples][3]
 * n_obs·n_samples counts against max_obstacles of cilqr_create; n_samples ≥ 2.  Sample headings come from the angle-addition
 * formulas and the ellipse semi-axes from reciprocals refined to ≈1 ulp: results agree with the materialised call to ≈1e-12,
 * not bit for bit. */
int cilqr_solve_batch_sampled(cilqr_handle* h, int B, int N, int n_obs, int n_samples,
                              const double* x0, double* U, const double* poly, const double* xplan_fl,
                              const double* nom_pose, const double* nom_dim, const double* sample_offset,
                              double sample_weight, double* X_out, double* J_out, int32_t* iters_out,
                              int32_t* status_out, uint32_t flags);
int cilqr_solve_batch_sampled_device(cilqr_handle* h, void* stream, int B, int N, int n_obs, int n_samples,
                                     const double* x0, double* U, const double* poly, const double* xplan_fl,
                                     const double* nom_pose, const double* nom_dim, const double* sample_offset,
                                     double sample_weight, double* X_out, double* J_out, int32_t* iters_out,
                                     int32_t* status_out, uint32_t flags);

/* Local min-cost selection over a batch resident on the device (strict-< first-minimum tie-break, as in
 * I/Constraints.cpp:50): writes {J_min, (double)index} to out_pair (device, 2 doubles).  The cross-GPU step
 * is cilqr_argmin_global_device below. */
int cilqr_argmin_device(cilqr_handle* h, void* stream, int B, const double* J, double* out_pair);

/* --- scoring solved candidates (new: the reference never compares candidates) --------------------------------------------
 * J_out, the cost the pick above ranks by, is Constraints::get_J: tracking and control effort only.  The control barriers, the
 * obstacle barriers and the uncertainty-map cost the solve descends along are not in it (the reference's get_J has them commented
 * out, I/Constraints.cpp:553-557), so the cheapest J may belong to a trajectory that drives through an obstacle: the barriers are
 * soft.  One launch after the solve evaluates, per solve, every term once and the constraint values themselves: */
#define CILQR_SCORE_FIELDS 8
typedef enum cilqr_score_field {
  CILQR_SCORE_TRACK = 0,        /* Constraints::get_J(X, U), I/Constraints.cpp:534-561 */
  CILQR_SCORE_CONTROL = 1,      /* sum over t < N of the four control barriers' VALUES q1*exp(q2*c), I/Constraints.cpp:67-78, 86-137 */
  CILQR_SCORE_OBSTACLE = 2,     /* sum over t < N, m < M of weight_m * (front + rear barrier value), I/Obstacle.cpp:21-32, 39-112 */
  CILQR_SCORE_UNCERTAINTY = 3,  /* w_uncertainty * sum over t < N of the map cost (the mean barrier value defined at
                                   cilqr_set_uncertainty_map); exactly 0.0 with no map set */
  CILQR_SCORE_MAX_C = 4,        /* max over t, m, both circles of c = 1 - d'Pd;  -HUGE_VAL when M == 0 */
  CILQR_SCORE_MAX_C_ENTRY = 5,  /* (double)(m*N + t) of that maximum, the lowest such index on equal values; -1 when M == 0 */
  CILQR_SCORE_MAX_CTRL = 6,     /* max over t of the four control constraint values (> 0: a bound is exceeded) */
  CILQR_SCORE_COLLISION = 7     /* ordinary obstacles: 1.0 if MAX_C > 0 else 0.0;  sampled: max over (t, o) of the share of samples s
                                   with c > 0 on either circle, a count / n_samples */
} cilqr_score_field;
/* cilqr_score_batch_device: device pointers, asynchronous on `stream`, like cilqr_solve_batch_obstacles_device (*obs is a host
 * struct, read before the call returns; NULL only when M == 0).  X [B][4*(N+1)], U [B][2*N], poly [B][6], xplan_fl [B][2] as the
 * solve takes and returns them; score [B][CILQR_SCORE_FIELDS]; total [B] or NULL.  cilqr_score_batch: host buffers, synchronous.
 *   - States X[:, t], t = 0 … N-1, pair with obstacle column t: the steps Constraints::get_state_cost visits.  x_N carries no
 *     cost, as in the reference.  No term depends on a heading error (the reference's state cost has no theta weight).
 *   - Obstacle weights apply as in l_x: weight[b][m] through the strides of *obs, or p.w_obstacle when NULL; sample_weight for the
 *     sampled call.
 *   - The closest path point is the strict-< first minimum of the squared distance over all num_of_local_wpts*10 samples
 *     (I/Constraints.cpp:43-56), found by a full scan.
 *   - UNCERTAINTY is added while a map is set on the handle, with the layer and pose of the solve's index, as in the solve.
 *   - total[b] = ((TRACK + CONTROL) + OBSTACLE) + UNCERTAINTY, summed in that order; NaN when COLLISION > max_collision or when any
 *     of the four terms is not finite.  A NaN never wins cilqr_argmin_device / cilqr_argmin_global_device, which return index -1
 *     when every candidate is rejected: hand them `total` in place of J_out to pick among the safe.  max_collision = 1.0 rejects
 *     nothing on collision grounds, 0.0 rejects any contact (c > 0: an ego circle centre inside the inflated ellipse).
 *   - The score of a solve is a function of that solve's inputs alone: bit-identical whatever B is, whatever the solve's index in
 *     the batch and whatever strides address the same obstacle values.  (Sums run over a reduction tree fixed by (N, M); the
 *     (max c, entry) reduction is lexicographic.)
 *   - cilqr_score_batch_sampled(_device) takes the compact form of cilqr_solve_batch_sampled and equals the ordinary call on the
 *     materialised obstacles m = o*n_samples + s, pose (x + dx, y + dy, v, theta + dtheta), weight sample_weight, BIT FOR BIT in
 *     fields 0-6 (the sample pose is formed by those plain additions, not by the solve kernels' angle-addition shortcut).  Field 7
 *     differs by definition: a share there, 0 or 1 for the ordinary call.
 *   - Limits are those of cilqr_create: B <= max_batch, N <= max_horizon, M or n_obs*n_samples <= max_obstacles; beyond them, for
 *     a negative stride or a NULL X, U, poly, xplan_fl or score: CILQR_ERR_ARG.  Nothing is allocated per call.  The sampled call
 *     keeps one 4-byte counter per (t, o) on chip beside the path samples: where 16*num_of_local_wpts*10 + 16*N + 4*n_obs*N + 272
 *     bytes exceed 64 KiB it returns CILQR_ERR_UNSUPPORTED (n_obs*N beyond about 15 000 at the default sample count). */
int cilqr_score_batch_device(cilqr_handle* h, void* stream, int B, int N, int M, const double* X, const double* U, const double* poly,
                             const double* xplan_fl, const cilqr_obstacles* obs, double max_collision, double* score, double* total);
int cilqr_score_batch(cilqr_handle* h, int B, int N, int M, const double* X, const double* U, const double* poly,
                      const double* xplan_fl, const cilqr_obstacles* obs, double max_collision, double* score, double* total);
int cilqr_score_batch_sampled_device(cilqr_handle* h, void* stream, int B, int N, int n_obs, int n_samples, const double* X,
                                     const double* U, const double* poly, const double* xplan_fl, const double* nom_pose,
                                     const double* nom_dim, const double* sample_offset, double sample_weight, double max_collision,
                                     double* score, double* total);
int cilqr_score_batch_sampled(cilqr_handle* h, int B, int N, int n_obs, int n_samples, const double* X, const double* U,
                              const double* poly, const double* xplan_fl, const double* nom_pose, const double* nom_dim,
                              const double* sample_offset, double sample_weight, double max_collision, double* score, double* total);

/* --- feedback gains, closed-loop rollouts from offset starts, collision risk per solve (new) ---------------------------------
 * A solve returns U alone; the time-varying policy u = U_t + k_t + K_t (x - X_t) every backward pass computes (I/iLQR.cpp:177-178)
 * is what tracks the plan from a start other than the one it was solved for.  Three additive groups of calls, each with a
 * host-buffer form (synchronous) and a `_device` form (device pointers, asynchronous on `stream`), with the conventions of
 * cilqr_score_batch(_device).  These take ordinary obstacles; the compact sampled form of cilqr_solve_batch_sampled is taken by
 * cilqr_gains_batch_sampled and cilqr_rollout_risk_sampled below (the stored-rows pair has no sampled form).  Nothing is allocated per
 * call: the host forms travel through buffers sized at create from max_batch, so their ROW counts are bounded by max_batch.
 *
 * cilqr_gains_batch(_device): ONE backward pass, iLQR::backward_pass(X, U, coeffs, x_plan, lamb) (I/iLQR.cpp:91-195), at the given
 * trajectory X [B][4*(N+1)], U [B][2*N]: linearised at X[:, t], U[:, t] for t < N with A and B evaluated at the NEXT state, as the
 * reference does; closest path point = strict-< first minimum; obstacle weights as in the solve; the uncertainty-map term added
 * while a map is set on the handle, with the layer and pose of the solve's index.  k_out [B][2*N]; K_out [B][8*N], the 2x4 block
 * of step t column-major: K[8*t + r + 2*c]; ok_out [B] int32 or NULL: 1 where backward_pass would return true, 0 where a step's
 * Q_uu is not finite — that solve's gains are then zero from the failing step down to step 0, as in the reference.
 *   `lamb` is the regularisation of that pass.  A solve does not export its last lambda, so the caller chooses: 1.0 is the
 *   reference's starting value (I/iLQR.cpp:205); the gains of the reference's own last pass belong to the lambda of that pass.
 *   B <= max_batch, N <= max_horizon, M <= max_obstacles; NULL X, U, poly, xplan_fl, k_out or K_out, a negative stride or a lamb
 *   that is not finite: CILQR_ERR_ARG.  CILQR_ERR_UNSUPPORTED where 16*num_of_local_wpts*10 + 144*N + 16 bytes exceed 64 KiB.
 *
 * cilqr_rollout_batch(_device): S closed-loop rollouts per solve.  Nominal X, U and gains k, K in the layouts above; delta holds
 * the start offsets (dx, dy, dv, dtheta), delta[b][s] at delta + 4*(b*delta_batch_stride*S + s): delta_batch_stride is in units of
 * [S][4] blocks, 0 = one offset set shared by all solves (1 = dense).  Row b*S + s of X_roll [B*S][4*(N+1)], U_roll [B*S][2*N] —
 * the layout the score calls read — is, with x'_0 = X[:, 0] + delta:
 *     u_t = (U_t + k_scale*k_t) + K_t (x'_t - X_t)   (iLQR::forward_pass, I/iLQR.cpp:68-86; the heading difference is not wrapped)
 *     x'_{t+1} = Model::forward_simulate(x'_t, u_t)  (the clamps act on a copy: u_t is stored unclamped)
 *   k_scale = 1 with delta = 0 IS the reference's forward pass; k_scale = 0 tracks the nominal plan.  A row depends on its own
 *   inputs alone: bit-identical whatever B, S and its position are.  S < 1, a negative delta_batch_stride, a NULL pointer or a
 *   k_scale that is not finite: CILQR_ERR_ARG; so is B > max_batch and, for the host-buffer form, B*S > max_batch.  The host-buffer
 *   form takes delta_batch_stride 0 or 1.  CILQR_ERR_UNSUPPORTED where 112*N + 25632 bytes exceed 64 KiB (N above 356).
 *
 * cilqr_score_rollouts(_device): scores B*S trajectory rows (row r belongs to solve r / S: its poly, xplan_fl, obstacle entries,
 * weights and map index) as cilqr_score_batch scores a solve, into row_score [B*S][CILQR_SCORE_FIELDS]: S = 1 gives that call's rows
 * bit for bit; for S > 1 the closest path sample is found by the solve kernels' windowed search, which returns the full scan's
 * index.  It then reduces each solve's S rows to risk [B][CILQR_RISK_FIELDS] and total [B] (NULL: not written):
 *   total[b] = RISK_MEAN_TOTAL, or NaN when RISK_COLLISION > max_risk or the mean is not finite: hand it to cilqr_argmin_device /
 *   cilqr_argmin_global_device in place of J_out.  B <= max_batch; host-buffer form: B*S <= max_batch; row_score and risk are
 *   required; violations are CILQR_ERR_ARG. */
#define CILQR_RISK_FIELDS 4
typedef enum cilqr_risk_field {
  CILQR_RISK_COLLISION = 0,   /* (rows with SCORE_MAX_C > 0 or a term that is not finite) / S */
  CILQR_RISK_WORST_C = 1,     /* max over the rows of SCORE_MAX_C */
  CILQR_RISK_WORST_ROW = 2,   /* (double) row index s of that maximum, the lowest on equal values */
  CILQR_RISK_MEAN_TOTAL = 3   /* mean over the rows of ((TRACK + CONTROL) + OBSTACLE) + UNCERTAINTY, summed over a tree fixed by S */
} cilqr_risk_field;
int cilqr_gains_batch_device(cilqr_handle* h, void* stream, int B, int N, int M, const double* X, const double* U, const double* poly,
                             const double* xplan_fl, const cilqr_obstacles* obs, double lamb, double* k_out, double* K_out,
                             int32_t* ok_out);
int cilqr_gains_batch(cilqr_handle* h, int B, int N, int M, const double* X, const double* U, const double* poly,
                      const double* xplan_fl, const cilqr_obstacles* obs, double lamb, double* k_out, double* K_out, int32_t* ok_out);
int cilqr_rollout_batch_device(cilqr_handle* h, void* stream, int B, int N, int S, const double* X, const double* U, const double* k,
                               const double* K, const double* delta, int64_t delta_batch_stride, double k_scale, double* X_roll,
                               double* U_roll);
int cilqr_rollout_batch(cilqr_handle* h, int B, int N, int S, const double* X, const double* U, const double* k, const double* K,
                        const double* delta, int64_t delta_batch_stride, double k_scale, double* X_roll, double* U_roll);
int cilqr_score_rollouts_device(cilqr_handle* h, void* stream, int B, int N, int M, int S, const double* X_roll, const double* U_roll,
                                const double* poly, const double* xplan_fl, const cilqr_obstacles* obs, double max_risk,
                                double* row_score, double* risk, double* total);
int cilqr_score_rollouts(cilqr_handle* h, int B, int N, int M, int S, const double* X_roll, const double* U_roll, const double* poly,
                         const double* xplan_fl, const cilqr_obstacles* obs, double max_risk, double* row_score, double* risk,
                         double* total);

/* --- fused rollout risk: the collision share per solve with no rollout stored (new) -------------------------------------------
 * cilqr_rollout_risk(_device) runs the rollouts of cilqr_rollout_batch (same X, U, k, K, delta, delta_batch_stride, k_scale, same
 * arithmetic) and evaluates, at every state x'_t with t < N (x'_N is not visited, as in the score calls), the obstacle constraints
 * c = 1 - d'Pd of both ego circles against every obstacle entry (m, t) — the c of cilqr_score_batch — keeping only what a
 * risk-bounded pick needs.  No X_roll, U_roll or row scores exist: the three-call path's 4*(N+1) + 2*N + 8 doubles per row are
 * never written.  Ordinary obstacles only (cilqr_obstacles, strides as in cilqr_solve_batch_obstacles; weights are not read).
 * Nothing here depends on the path (poly, xplan_fl) or on the uncertainty map: neither is an argument, and a map set on the
 * handle is ignored.
 *   A row HITS at step t when max(c_front, c_rear) > 0 for some obstacle m, or when one of x', y', v', theta' of x'_t or of the two
 *   controls u_t is not finite.  A c that is NaN never wins a maximum.
 * risk [B][CILQR_ROLLOUT_RISK_FIELDS] (required), see the enum; step_hits [B][N] int32 or NULL: the rows that hit AT step t;
 * total [B] or NULL: total[b] = base[b] when RR_COLLISION <= max_risk and base[b] is finite, else NaN — hand it to
 * cilqr_argmin_device / cilqr_argmin_global_device.  base [B] is any per-solve cost the caller ranks by (J_out, or the `total` of
 * cilqr_score_batch); total without base is CILQR_ERR_ARG.
 *   Counts are integers and (max c, lowest row, lowest entry) is lexicographic, so every field is independent of the evaluation
 *   order: a solve's results depend on its own inputs and offsets alone — the same bits whatever B is and wherever the solve sits
 *   in the batch.  Fed the same inputs, RR_COLLISION, RR_WORST_C and RR_WORST_ROW equal RISK_COLLISION, RISK_WORST_C (bit for bit)
 *   and RISK_WORST_ROW of cilqr_rollout_batch + cilqr_score_rollouts whenever every row's cost terms are finite exactly when its
 *   states and controls are, and RR_WORST_ENTRY is that row's SCORE_MAX_C_ENTRY.
 * Mapping: lane = row; solve b takes ceil(S/256) workgroups, each leaving one partial record (8 doubles + max_horizon int32) in a
 * buffer the handle allocates at create for max_batch records; nothing is allocated per call.
 * CILQR_ERR_ARG: NULL X, U, k, K, delta or risk; S < 1; a negative stride; a k_scale or max_risk that is NaN; B, N or M beyond the
 * cilqr_create limits; B*ceil(S/256) > max_batch.  The host-buffer form additionally takes delta_batch_stride 0 or 1, and its
 * arrays — X, U, k, K, the obstacle span, (delta_batch_stride ? B : 1)*S*4 offsets, base, and the outputs — must fit the device
 * arena reserved at create: (delta_batch_stride ? B : 1)*S <= max_batch*max_horizon always fits (no rollout rows travel).
 * CILQR_ERR_UNSUPPORTED where the kernel's LDS, 8*(14*N + 4) + 48*M*N + 4*N + 112 bytes (nominal records, obstacle entries, step
 * counters, reduction slots), exceeds 64 KiB. */
#define CILQR_ROLLOUT_RISK_FIELDS 6
typedef enum cilqr_rollout_risk_field {
  CILQR_RR_COLLISION = 0,    /* rows that hit at any step / S */
  CILQR_RR_WORST_C = 1,      /* max over rows, t < N, m, both circles of c;  -HUGE_VAL when M == 0 */
  CILQR_RR_WORST_ROW = 2,    /* row s of that maximum, lowest on equal values;  -1 when M == 0 */
  CILQR_RR_WORST_ENTRY = 3,  /* m*N + t of that maximum within that row, lowest on equal values;  -1 when M == 0 */
  CILQR_RR_FIRST_STEP = 4,   /* lowest t at which any row hits;  -1 when none does */
  CILQR_RR_STEP_SHARE = 5    /* max over t of (rows that hit AT step t) / S */
} cilqr_rollout_risk_field;
int cilqr_rollout_risk_device(cilqr_handle* h, void* stream, int B, int N, int M, int S, const double* X, const double* U,
                              const double* k, const double* K, const double* delta, int64_t delta_batch_stride, double k_scale,
                              const cilqr_obstacles* obs, double max_risk, const double* base, double* risk, int32_t* step_hits,
                              double* total);
int cilqr_rollout_risk(cilqr_handle* h, int B, int N, int M, int S, const double* X, const double* U, const double* k,
                       const double* K, const double* delta, int64_t delta_batch_stride, double k_scale, const cilqr_obstacles* obs,
                       double max_risk, const double* base, double* risk, int32_t* step_hits, double* total);

/* --- gains and fused rollout risk for SAMPLED obstacles in compact form (new) --------------------------------------------------
 * The scene form of cilqr_solve_batch_sampled — nom_pose [B][n_obs][4*N], nom_dim [B][n_obs][2*N], sample_offset
 * [B][n_obs][n_samples][3] = (dx, dy, dtheta), sample_weight — taken as it is: no materialised table of n_obs*n_samples obstacles
 * is built, read or kept.  Materialised obstacle m = o*n_samples + s has pose (x + dx, y + dy, v, theta + dtheta), formed by those
 * plain additions (not by the solve kernels' angle-addition shortcut), the nominal dimensions, and weight sample_weight.
 *
 * cilqr_gains_batch_sampled(_device) is cilqr_gains_batch on those materialised obstacles, BIT FOR BIT: k_out, K_out, ok_out, the
 * zeroed gains below a failed step, the map term and lamb as there.  CILQR_ERR_ARG for a NULL X, U, poly, xplan_fl, nom_pose,
 * nom_dim, sample_offset, k_out or K_out, a lamb that is not finite, n_obs < 1, n_samples < 2, B > max_batch, N > max_horizon or
 * n_obs*n_samples > max_obstacles; CILQR_ERR_UNSUPPORTED where 16*num_of_local_wpts*10 + 144*N + 16 bytes exceed 64 KiB.
 *
 * cilqr_rollout_risk_sampled(_device) runs the rollouts of cilqr_rollout_risk (same X, U, k, K, delta, delta_batch_stride, k_scale,
 * same arithmetic, lane = rollout row) and evaluates c of both ego circles against every sample of every obstacle at every state
 * x'_t, t < N.  The HIT COUNT h(r, t, o) is the number of samples j of obstacle o with max(c_front, c_rear) > 0 at state x'_t of row
 * r; it is n_samples for every o when one of x', y', v', theta' of x'_t or of the two controls u_t is not finite.  A c that is NaN is
 * never > 0 and never wins a maximum.
 * risk [B][CILQR_RRS_FIELDS] (required), see the enum; step_hits [B][N] int32 or NULL: the sum over rows of max_o h(r, t, o);
 * total [B] or NULL: total[b] = base[b] when RRS_COLLISION <= max_risk and base[b] is finite, else NaN (the convention of
 * cilqr_rollout_risk; total without base is CILQR_ERR_ARG).
 *   Every count is an integer and (max c, lowest row, lowest entry) is lexicographic: a solve's results depend on its own inputs
 *   alone — the same bits whatever B is and wherever the solve sits in the batch.  RRS_ANY_SHARE, RRS_WORST_ROW, RRS_WORST_ENTRY
 *   and RRS_FIRST_STEP equal RR_COLLISION, RR_WORST_ROW, RR_WORST_ENTRY and RR_FIRST_STEP of cilqr_rollout_risk on the materialised
 *   obstacles, and RRS_WORST_C equals its RR_WORST_C bit for bit.
 * Mapping: solve b takes ceil(S/256) workgroups of 64*min(4, ceil(S/64)) lanes; each builds one step's n_obs*n_samples entries at a
 * time into a double-buffered on-chip step buffer while it evaluates the step before.  cilqr_create reserves NOTHING further for
 * this call and nothing is allocated per call: for S > 256 the workgroups' partial records (8 doubles + N*(1 + n_obs) int32 each)
 * lie in the obstacle workspace the handle holds for the solve kernels (max_batch padded to 64, x max_obstacles x max_horizon x 6
 * doubles), which no kernel of this call uses — a solve on ANOTHER stream of the same handle must not run beside it.
 * CILQR_ERR_ARG: a NULL X, U, k, K, delta, nom_pose, nom_dim, sample_offset or risk; S < 1; a negative stride; a k_scale or max_risk
 * that is NaN; n_obs < 1, n_samples < 2, B, N or n_obs*n_samples beyond the cilqr_create limits; S*n_samples, n_obs*n_samples*N or
 * B*ceil(S/256) beyond 2^31 - 1; for S > 256, B*ceil(S/256) partial records beyond that workspace.  The host-buffer form takes
 * delta_batch_stride 0 or 1, and its arrays — X, U, k, K, the offsets, the nominal tables, the sample offsets, base and the outputs —
 * must fit the device arena reserved at create (CILQR_ERR_ARG otherwise).
 * CILQR_ERR_UNSUPPORTED where the kernel's LDS, 8*(14*N + 4) + 96*n_obs*n_samples + 4*N*(1 + n_obs) + 160 bytes (nominal records,
 * the two halves of the step buffer, step and (t, o) counters, reduction slots), exceeds 64 KiB: 8 x 32 samples at N = 50 take
 * 32 168 bytes. */
#define CILQR_RRS_FIELDS 8
typedef enum cilqr_rollout_risk_sampled_field {
  CILQR_RRS_COLLISION = 0,    /* sum over rows of max over (t, o) of h / (S*n_samples): the mean over the rows of what
                                 CILQR_SCORE_COLLISION of cilqr_score_batch_sampled would be for that row */
  CILQR_RRS_WORST_C = 1,      /* max over rows, t < N, o, samples, both circles of c;  -HUGE_VAL when there is none */
  CILQR_RRS_WORST_ROW = 2,    /* row of that maximum, lowest on equal values;  -1 when there is none */
  CILQR_RRS_WORST_ENTRY = 3,  /* m*N + t of that maximum with m = o*n_samples + j, lowest within that row;  -1 when there is none */
  CILQR_RRS_FIRST_STEP = 4,   /* lowest t with any h > 0;  -1 when none */
  CILQR_RRS_STEP_SHARE = 5,   /* max over t of (sum over rows of max_o h) / (S*n_samples); step_hits[t] is that sum */
  CILQR_RRS_ANY_SHARE = 6,    /* rows with some h > 0 / S */
  CILQR_RRS_PAIR_SHARE = 7    /* max over (t, o) of (sum over rows of h) / (S*n_samples): the joint chance-constraint quantity
                                 per obstacle and step */
} cilqr_rollout_risk_sampled_field;
int cilqr_gains_batch_sampled_device(cilqr_handle* h, void* stream, int B, int N, int n_obs, int n_samples, const double* X,
                                     const double* U, const double* poly, const double* xplan_fl, const double* nom_pose,
                                     const double* nom_dim, const double* sample_offset, double sample_weight, double lamb,
                                     double* k_out, double* K_out, int32_t* ok_out);
int cilqr_gains_batch_sampled(cilqr_handle* h, int B, int N, int n_obs, int n_samples, const double* X, const double* U,
                              const double* poly, const double* xplan_fl, const double* nom_pose, const double* nom_dim,
                              const double* sample_offset, double sample_weight, double lamb, double* k_out, double* K_out,
                              int32_t* ok_out);
int cilqr_rollout_risk_sampled_device(cilqr_handle* h, void* stream, int B, int N, int n_obs, int n_samples, int S, const double* X,
                                      const double* U, const double* k, const double* K, const double* delta,
                                      int64_t delta_batch_stride, double k_scale, const double* nom_pose, const double* nom_dim,
                                      const double* sample_offset, double max_risk, const double* base, double* risk,
                                      int32_t* step_hits, double* total);
int cilqr_rollout_risk_sampled(cilqr_handle* h, int B, int N, int n_obs, int n_samples, int S, const double* X, const double* U,
                               const double* k, const double* K, const double* delta, int64_t delta_batch_stride, double k_scale,
                               const double* nom_pose, const double* nom_dim, const double* sample_offset, double max_risk,
                               const double* base, double* risk, int32_t* step_hits, double* total);

/* --- map rollout risk: the share of rollouts that enter occupied cells of the uncertainty map (new) ----------------------------
 * The map counterpart of cilqr_rollout_risk: in the reference's live node the ellipse channel is off and the blurred costmap given
 * to set_uncertainty_map is the planner's only obstacle information (I/ilqr_uncertainty_node.cpp:111-113, 151-189).
 * cilqr_rollout_risk_map(_device) runs the rollouts of cilqr_rollout_batch / cilqr_rollout_risk (same X, U, k, K, delta,
 * delta_batch_stride, k_scale, same statements) and looks the map up under every state x'_t with t < N (x'_N is not visited):
 *   probes   the probes_l x probes_w footprint probes and the bilinear lookup defined at cilqr_set_uncertainty_map — body offsets
 *            a_k, b_l on safe_length x safe_width turned by the state's heading, a rigid transform into the map frame by the pose
 *            of the solve's index, bilinear interpolation over four cell centres evaluated in double.  Layer
 *            (layer + b*layer_stride) and pose (poses[b], or the shared one) are those of the map CURRENTLY SET on the handle,
 *            indexed by the solve as the solve and score kernels index them.  Probe q = k*probes_w + l.
 *   valid    a probe is valid when its four cells are all inside the map and finite — the map cost's own rule.
 *   hit      a row HITS at step t when a valid probe's occupancy is > occ_threshold (strict), or one of x', y', v', theta' of
 *            x'_t or of the two controls u_t is not finite (as in cilqr_rollout_risk), or CILQR_MAP_RISK_UNKNOWN_HITS is set and
 *            a probe is invalid.
 *   unknown  a row is UNKNOWN at step t when at least one probe is invalid; a state that is not finite makes all its probes invalid.
 * risk [B][CILQR_MAP_RISK_FIELDS] (required), see the enum; step_hits [B][N] and unknown_hits [B][N] int32, each may be NULL: the
 * rows that hit, or are unknown, AT step t; total [B] or NULL: total[b] = base[b] when MR_COLLISION <= max_risk and base[b] is
 * finite, else NaN.  base [B] is any per-solve cost — typically the `total` of cilqr_rollout_risk or cilqr_rollout_risk_sampled,
 * whose NaN (already rejected) stays NaN; hand total to cilqr_argmin_device / cilqr_argmin_global_device.  total without base is
 * CILQR_ERR_ARG.
 *   Nothing is a floating-point sum: counts are integers and (max occupancy, lowest row, lowest entry) is lexicographic, so a
 *   solve's results are the same bits whatever B is and wherever the solve sits in the batch.  MR_WORST_OCC is the occupancy the
 *   map cost interpolates at that probe (cilqr_debug_uncertainty_cost at probes 1 x 1 gives q1*exp(q2*(occ/100 - 1))).
 * Mapping: lane = row; solve b takes ceil(S/256) workgroups of 64*min(4, ceil(S/64)) lanes.  cilqr_create reserves nothing new
 * and nothing is allocated per call: for S > 256 the workgroups' partial records (8 doubles + N int32) lie in the buffer of
 * cilqr_rollout_risk's records — a cilqr_rollout_risk with S > 256 on ANOTHER stream of the same handle must not run beside it.
 * CILQR_ERR_ARG, decided before the handle is looked at where no handle is needed: NULL X, U, k, K, delta or risk; total without
 * base; S < 1; a negative stride; a k_scale, occ_threshold or max_risk that is NaN; flag bits other than
 * CILQR_MAP_RISK_UNKNOWN_HITS; then B or N beyond the cilqr_create limits; B*ceil(S/256) > max_batch; no uncertainty map set on the
 * handle (the message says so).  The host-buffer form additionally takes delta_batch_stride 0 or 1, and its arrays — X, U, k, K,
 * (delta_batch_stride ? B : 1)*S*4 offsets, base and the outputs — must fit the device arena reserved at create:
 * (delta_batch_stride ? B : 1)*S <= max_batch*max_horizon always fits.
 * CILQR_ERR_UNSUPPORTED where the kernel's LDS, 8*(14*N + 4) + 4*N + 160 bytes (nominal records, packed step counters, reduction
 * slots), exceeds 64 KiB: N above 563, which CILQR_MAX_HORIZON = 384 keeps out of reach — every horizon a handle accepts runs. */
#define CILQR_MAP_RISK_FIELDS 7
typedef enum cilqr_map_risk_field {
  CILQR_MR_COLLISION = 0,   /* rows that hit at any step / S */
  CILQR_MR_WORST_OCC = 1,   /* max interpolated occupancy over rows, t < N, valid probes;  -HUGE_VAL when no probe is valid */
  CILQR_MR_WORST_ROW = 2,   /* its row, lowest on equal values;  -1 when none */
  CILQR_MR_WORST_ENTRY = 3, /* q*N + t of that maximum within that row, q = k*probes_w + l, lowest on equal values;  -1 when none */
  CILQR_MR_FIRST_STEP = 4,  /* lowest t at which any row hits;  -1 when none does */
  CILQR_MR_STEP_SHARE = 5,  /* max over t of (rows that hit AT step t) / S */
  CILQR_MR_UNKNOWN = 6      /* rows with an invalid probe at any step / S */
} cilqr_map_risk_field;
#define CILQR_MAP_RISK_UNKNOWN_HITS 1u /* flags: an invalid probe counts as a hit */
int cilqr_rollout_risk_map_device(cilqr_handle* h, void* stream, int B, int N, int S, const double* X, const double* U,
                                  const double* k, const double* K, const double* delta, int64_t delta_batch_stride, double k_scale,
                                  double occ_threshold, uint32_t flags, double max_risk, const double* base, double* risk,
                                  int32_t* step_hits, int32_t* unknown_hits, double* total);
int cilqr_rollout_risk_map(cilqr_handle* h, int B, int N, int S, const double* X, const double* U, const double* k, const double* K,
                           const double* delta, int64_t delta_batch_stride, double k_scale, double occ_threshold, uint32_t flags,
                           double max_risk, const double* base, double* risk, int32_t* step_hits, int32_t* unknown_hits,
                           double* total);

/* --- analytic pose-noise risk: closed-loop covariance chain and Gaussian chance values (new) -----------------------------------
 * The rollout calls above judge a solve by S sampled starts: risk in steps of 1/S, dependent on the offsets' seed, and no state
 * covariance along the plan.  cilqr_chance_risk(_device) propagates ONE 4x4 covariance per solve through the linear closed loop
 * the gains define around the plan — no samples, no seed, the work of one rollout row — and turns it into a Gaussian chance value
 * per (obstacle, step, ego circle).  X [B][4*(N+1)], U [B][2*N], K [B][8*N] in the layouts of cilqr_gains_batch (K[8*t + r + 2*c]).
 * The feedforward k is not an argument: the model is the k_scale = 0 policy u = U_t + K_t (x - X_t), whose mean is the plan X.
 * Ordinary obstacles through the strides of cilqr_obstacles (weights are not read).  Neither the path nor an uncertainty map set
 * on the handle is read.
 *
 * Covariance chain.  Every 4x4 matrix is column-major, entry (r, c) at [r + 4*c], state order (x, y, v, theta).  For t < N
 *     F_t = A_t + B_t K_t,      Sigma_{t+1} = F_t Sigma_t F_t' + W,
 *   A_t, B_t the Jacobians of Model::forward_simulate (I/Model.cpp:100-155) at the step's OWN state and control,
 *   v = X_t[2], theta = X_t[3], a = U_t[0], with adv = v*dt + a*dt^2/2:
 *     A = I + { (0,2): dt*cos theta, (1,2): dt*sin theta, (0,3): -sin theta*adv, (1,3): cos theta*adv },
 *     B = { (0,0): dt^2*cos theta/2, (1,0): dt^2*sin theta/2, (2,0): dt, (3,1): dt },  every other entry 0.
 *   They are NOT evaluated at the next state (that shift is the backward pass's, see cilqr_gains_batch), and the model's clamps
 *   (acceleration, yaw rate, speed) are treated as INACTIVE: a plan that rides a clamp has less closed-loop authority than this
 *   chain assumes.  Entries with row <= column are computed and mirrored, so every Sigma_t is exactly symmetric; only the
 *   row <= column entries of sigma0 and process_noise are read.  sigma0 [B or 1][16]: sigma0_batch_stride 1 = one per solve, 0 =
 *   one shared by the batch.  process_noise [16] = W, shared by the batch, NULL = zero.  sigma_out[b][t] = Sigma_t, t = 0 ... N.
 *
 * Chance value.  For obstacle entry (m, t), t < N, and each ego circle, lever l = +ego_front (front) or -ego_rear (rear), centre
 * (x + l cos theta, y + l sin theta) at X_t:
 *     cbar  the c = 1 - d'Pd of cilqr_score_batch at X_t: the same inflated semi-axes a, b (the stray +1 on b included);
 *     g     its gradient over (x, y, v, theta):  g_xy = -2 R(theta_o)' P d  (the first two components of the reference's c_dot,
 *           I/Obstacle.cpp:82, 101),  g_v = 0,  g_theta = g_xy . (-l sin theta, l cos theta).  The reference leaves g_theta at 0
 *           in its cost; the lever arm is kept here because heading noise moves the circles;
 *     s     sqrt(max(g' Sigma_t g, 0))   (a quadratic form that is NaN counts as 0);
 *     p     erfc(-cbar / (s*sqrt 2)) / 2, the Gaussian probability of c > 0;  with s = 0: 1 if cbar > 0, else 0.
 *   entry_p[m*N + t] = max(p_front, p_rear), evaluated as erfc of the smaller of the two arguments (erfc decreases); a NaN never
 *   wins a maximum.
 * Per step:  r_t = min(1, sum over m of entry_p[m*N + t]) — Boole's bound over the obstacles, summed in ascending m (an order fixed by
 *   M); a sum that is NaN gives 1; r_t = 1 when any of X_t, U_t, K_t or Sigma_t is not finite (the rollout calls' convention for a
 *   lost row).  step_risk[b][t] = r_t.
 * risk [B][CILQR_CHANCE_FIELDS] (required), see the enum; step_risk [B][N], entry_p [B][M*N], sigma_out [B][N+1][16], each may be
 * NULL; total [B] or NULL: total[b] = base[b] when the bounded field — CR_STEP_RISK, or CR_SUM_RISK under CILQR_CHANCE_BOUND_SUM —
 * is <= max_risk and base[b] is finite, else NaN: the convention of cilqr_rollout_risk, so the result composes with it and with
 * cilqr_rollout_risk_map through `base` and feeds cilqr_argmin_device / cilqr_argmin_global_device.  total without base is
 * CILQR_ERR_ARG.
 *   A solve's outputs depend on its own inputs alone: the same bits whatever B is, wherever the solve sits in the batch and whatever
 *   strides address the same obstacle values (sums run over trees fixed by (N, M); maxima are lexicographic, lowest index first).
 * Mapping: one workgroup per solve, one launch, nothing allocated per call.  The steps' F_t are formed in parallel, ten lanes then
 * run the serial chain (one per row <= column entry), every lane then takes obstacle entries.
 * CILQR_ERR_ARG, decided before the handle is looked at where no handle is needed: NULL X, U, K, sigma0 or risk; total without base;
 * obs NULL with M > 0; a negative stride; sigma0_batch_stride other than 0 or 1; a max_risk that is NaN; flag bits other than
 * CILQR_CHANCE_BOUND_SUM; then B, N or M beyond the cilqr_create limits.  The host-buffer form's arrays — X, U, K, sigma0,
 * process_noise, the obstacle span, base and the outputs — must fit the device arena reserved at create (CILQR_ERR_ARG otherwise).
 * Per solve that is 15*N + 6*M*N + 28 doubles, N + 1 covariances of 16 with sigma_out and M*N more with entry_p: without these two
 * outputs every B <= max_batch fits; with both, every B <= max_batch/2 does (the arena is the one the earlier calls sized: this
 * call adds nothing to it).
 * CILQR_ERR_UNSUPPORTED where the kernel's LDS, 8*(33*N + M*N + 16) bytes (F_t and Sigma_t, 16 doubles each, r_t, entry_p), exceeds
 * 64 KiB: N above 247 without obstacles, above 220 with M = 4. */
#define CILQR_CHANCE_FIELDS 6
typedef enum cilqr_chance_risk_field {
  CILQR_CR_STEP_RISK = 0,     /* max over t of r_t: what max_risk bounds by default.  The counterpart of RR_STEP_SHARE; it tracks
                                 RR_COLLISION because the steps are strongly correlated */
  CILQR_CR_WORST_STEP = 1,    /* lowest t of that maximum;  -1 when M == 0 */
  CILQR_CR_SUM_RISK = 2,      /* min(1, sum over t of r_t), over a tree fixed by N: Boole's bound over the horizon, an upper bound.
                                 Bounded instead of CR_STEP_RISK under CILQR_CHANCE_BOUND_SUM */
  CILQR_CR_MAX_P = 3,         /* max over entries of entry_p;  0 when M == 0 */
  CILQR_CR_MAX_ENTRY = 4,     /* m*N + t of that maximum, lowest on equal values;  -1 when M == 0 */
  CILQR_CR_MAX_POS_SIGMA = 5  /* max over t <= N of sqrt(lambda_max of Sigma_t's 2x2 position block), closed form */
} cilqr_chance_risk_field;
#define CILQR_CHANCE_BOUND_SUM 1u /* flags: max_risk bounds CR_SUM_RISK */
int cilqr_chance_risk_device(cilqr_handle* h, void* stream, int B, int N, int M, const double* X, const double* U, const double* K,
                             const double* sigma0, int64_t sigma0_batch_stride, const double* process_noise,
                             const cilqr_obstacles* obs, uint32_t flags, double max_risk, const double* base, double* risk,
                             double* step_risk, double* entry_p, double* sigma_out, double* total);
int cilqr_chance_risk(cilqr_handle* h, int B, int N, int M, const double* X, const double* U, const double* K, const double* sigma0,
                      int64_t sigma0_batch_stride, const double* process_noise, const cilqr_obstacles* obs, uint32_t flags,
                      double max_risk, const double* base, double* risk, double* step_risk, double* entry_p, double* sigma_out,
                      double* total);

/* --- chance-constraint tightening: obstacles inflated by Sigma_t for a re-solve (new) ---------------------------------------------
 * Every call above JUDGES a solved plan under pose uncertainty; none feeds back into the solve.  cilqr_tighten_obstacles(_device)
 * is that step: from the Sigma_t that cilqr_chance_risk left in sigma_out it grows every obstacle entry by kappa standard
 * deviations of the relative position (ego circle minus obstacle) along the ellipse's own axes, and writes a dense obstacle table
 * that cilqr_solve_batch_obstacles(_device) re-solves against, warm-started from the plan's U.  One round of the loop, all of it
 * device-resident:  solve -> cilqr_gains_batch -> cilqr_chance_risk (sigma_out) -> cilqr_tighten_obstacles -> solve on (pose_out,
 * dim_out).  Sigma is an INPUT: the chain has its kernel, and the loop wants the chance figures of the untightened plan anyway.
 * X [B][4*(N+1)], the plan; sigma [B][N+1][16], exactly sigma_out of cilqr_chance_risk (column-major, entry (r, c) at [r + 4*c]).
 * Of each Sigma_t, t < N, six entries are read: (0,0), (0,1), (0,3), (1,1), (1,3), (3,3) — row <= column, position and heading; the
 * speed row and column do not move a circle centre.  Obstacles through the strides of cilqr_obstacles (weights are not read).
 * obs_cov: NULL (zero), or the obstacle's own position covariance, 3 doubles (xx, xy, yy; world frame) at obs_cov + 3*e for the same
 * entry index e = b*batch_stride + m*obstacle_stride + t*step_stride that addresses its pose: an obstacle whose predicted position
 * is uncertain is then solved against as ONE inflated ellipse where the sampled form uses n_samples of them.
 *
 * Definition.  For entry (m, t), t < N, and each ego circle, lever l = +ego_front (front) or -ego_rear (rear), theta = X_t[3],
 * j = (-l sin theta, l cos theta) the derivative of the circle centre over theta, S = Sigma_t:
 *     Cxx = S00 + 2 jx S03 + jx^2 S33,    Cyy = S11 + 2 jy S13 + jy^2 S33,    Cxy = S01 + jx S13 + jy S03 + jx jy S33
 *   is the centre's position covariance; obs_cov is added to it; and with co = cos theta_o, so = sin theta_o of the obstacle's pose
 *     va = co^2 Cxx + 2 co so Cxy + so^2 Cyy,      vb = so^2 Cxx - 2 co so Cxy + co^2 Cyy
 *   are the variances along the ellipse's axes.  Over the two circles the larger va and the larger vb are taken, a NaN losing to a
 *   number; a negative result counts as 0; where both circles' values are NaN the result is NaN.  Then
 *     da = kappa*sqrt(va),  db = kappa*sqrt(vb),   each replaced by max_inflate when it is not finite or exceeds max_inflate: such
 *   an entry counts as CAPPED (a Sigma_t with a NaN among its six entries caps every entry of its step, kappa = 0 included);
 *     dim_out[b][m][2*t ...] = (length + 2*da, width + 2*db).  The solver's semi-axes are dim/2 + ..., so a and b grow by exactly
 *   da and db.  dim_out is dense [B][M][2*N], the layout of obs_dim and of nom_dim: it feeds both solve forms.
 *   pose_out [B][M][4*N] or NULL: the bit copy of the addressed poses, so that obstacles shared by strides become the dense table
 *   (strides M*N, N, 1) the re-solve needs beside dim_out.
 * What this is: an AXIS-WISE MARGINAL tightening — the ellipse grows along its axes by the marginal standard deviations, the
 * correlation between the two axes is dropped, and it agrees with the chance value of cilqr_chance_risk (one Gaussian of the
 * linearised constraint) to first order only.  kappa for a per-entry chance eps: cilqr_chance_kappa(eps).  The barriers are soft:
 * the loop guarantees nothing.  Where the plan has room to move it does what it should (an obstacle 12 m ahead and 1 to 3.8 m to
 * the side, eps 0.05: one round turns a candidate in contact, CR_STEP_RISK 1, into max c <= -0.08 and CR_STEP_RISK <= 1.5e-7 for
 * every candidate, both against the ORIGINAL obstacles).  Where it has none it does not help: with the ego starting beside the
 * obstacle the first steps cannot leave the inflated ellipse, a warm-started re-solve drifts with or without tightening, and
 * CR_STEP_RISK went 0.1015 -> 0.1044 re-solved without it and 0.1015 -> 0.131 with kappa 1.645.  Judge the final plan against the
 * original obstacles, always.
 * tighten [B][CILQR_TIGHTEN_FIELDS] (required), see the enum.  No floating sums: maxima are lexicographic, the count is an integer.
 *   A solve's outputs depend on its own inputs alone: the same bits whatever B is, wherever the solve sits in the batch and whatever
 *   strides address the same values.
 * Mapping: one workgroup per solve, one launch, nothing allocated per call.  Per step the two circle centres' covariances (Cxx, Cxy,
 * Cyy: what depends on the step alone) are staged in LDS, lanes then stride over the M*N entries.
 * CILQR_ERR_ARG, decided before the handle is looked at: NULL X, sigma, dim_out or tighten; obs NULL with M > 0; a negative stride;
 * a kappa or max_inflate that is negative or not finite; then B, N or M beyond the cilqr_create limits.  The host-buffer form's
 * arrays — X, sigma, the obstacle span, 3 doubles of obs_cov per entry of the span, and the outputs — must fit the device arena
 * reserved at create (CILQR_ERR_ARG otherwise; this call adds nothing to it).  With dense obstacles that is 20*N + 15*M*N + 24
 * doubles per solve with obs_cov and pose_out, 20*N + 8*M*N + 24 without them: every B <= 2*max_batch/5 always fits with both, every
 * B <= 3*max_batch/4 without; M = 0 fits for every B <= max_batch.
 * CILQR_ERR_UNSUPPORTED where the kernel's LDS, 8*(6*N + 20) bytes (six doubles per step, five per wavefront for the reduction),
 * exceeds 64 KiB: N above 1362, which CILQR_MAX_HORIZON = 384 keeps out of reach — every horizon a handle accepts runs. */
#define CILQR_TIGHTEN_FIELDS 4
typedef enum cilqr_tighten_field {
  CILQR_TG_MAX_DA = 0,    /* max over entries of da;  0 when M == 0 */
  CILQR_TG_MAX_DB = 1,    /* max over entries of db;  0 when M == 0 */
  CILQR_TG_MAX_ENTRY = 2, /* m*N + t of the largest max(da, db), lowest index on equal values;  -1 when M == 0 */
  CILQR_TG_CAPPED = 3     /* number of capped entries */
} cilqr_tighten_field;
int cilqr_tighten_obstacles_device(cilqr_handle* h, void* stream, int B, int N, int M, const double* X, const double* sigma,
                                   const cilqr_obstacles* obs, const double* obs_cov, double kappa, double max_inflate,
                                   double* pose_out, double* dim_out, double* tighten);
int cilqr_tighten_obstacles(cilqr_handle* h, int B, int N, int M, const double* X, const double* sigma, const cilqr_obstacles* obs,
                            const double* obs_cov, double kappa, double max_inflate, double* pose_out, double* dim_out,
                            double* tighten);
/* Host only: the kappa with erfc(kappa/sqrt 2)/2 = eps, the one-sided Gaussian quantile of a per-entry chance eps, by Newton's
 * iteration on (the logarithm of) erfc from the fixed start sqrt(-2 log eps) with a fixed number of steps: the same bits for the
 * same eps.  NaN outside (0, 0.5]; exactly 0 at 0.5. */
double cilqr_chance_kappa(double eps);

/* --- map tightening: the costmap dilated by Sigma_t along the plan for a re-solve (new) -------------------------------------------
 * cilqr_tighten_obstacles knows ellipses only; in the reference's live node that channel is off and the blurred costmap of
 * cilqr_set_uncertainty_map is the planner's only obstacle information, so there every check could only reject.
 * cilqr_tighten_map(_device) is the map counterpart: from the Sigma_t that cilqr_chance_risk left in sigma_out (M = 0 supplies it) it
 * writes, per solve, a tightened copy of the layer set on the handle that a warm-started re-solve runs against.  The reference's own
 * uncertainty blur (M/src/arbitrary_transformation.cu) is the same idea with three constant sigmas — a per-cell covariance whose
 * heading lever grows with the cell's offset, then a confidence ellipse; here the covariance comes from the closed loop along the
 * plan.  One round:  solve -> cilqr_gains_batch -> cilqr_chance_risk (sigma_out) -> cilqr_tighten_map -> cilqr_set_uncertainty_map_device
 * (layer_out, layer_stride = rows*cols, the same geometry, poses and probes) -> solve, warm-started from the plan's U.  No solve
 * kernel changes: the solve already reads a layer and a pose per solve.
 * X [B][4*(N+1)], the plan.  sigma [B][N+1][16], exactly sigma_out of cilqr_chance_risk (column-major, entry (r, c) at [r + 4*c]);
 * the six entries cilqr_chance_risk_map reads are read, for steps t < N: (0,0), (0,1), (1,1), (0,3), (1,3), (3,3).  Map, geometry,
 * layer_stride and poses are those CURRENTLY SET on the handle, indexed by the solve as every map call indexes them: solve b reads
 * layer + b*layer_stride and poses[b], or the shared pose.  layer_out [B][rows*cols] float32, dense, column-major like the input;
 * it must not overlap the set layer (CILQR_ERR_ARG where the two ranges meet).
 *
 * Definition for solve b and cell (i, j).  Everything is in the map frame; every formula is evaluated in double as C evaluates it
 * as written, left to right, with no fused multiply-add.
 *   frame      c, s are the cosine and sine of the solve's map pose heading, obtained as the other map calls obtain them (the shared
 *              pose's on the host, a per-solve pose's on the device).  With dx = X_t[0] - pose.x, dy = X_t[1] - pose.y:
 *                p_t = R'(X_t.xy - pose.xy) = (c*dx + s*dy,  c*dy - s*dx),   t = 0 ... N-1.
 *              The position block P of S = Sigma_t, the cross terms (S03, S13) and S33 are rotated the same way, P_m = R'PR and
 *              c_theta = R'(S03, S13):  with cc = c*c, ss = s*s, cs = c*s
 *                Pxx = cc*S00 + 2*cs*S01 + ss*S11,    Pxy = cs*(S11 - S00) + (cc - ss)*S01,    Pyy = ss*S00 - 2*cs*S01 + cc*S11,
 *                cx = c*S03 + s*S13,                  cy = c*S13 - s*S03,                      Stt = S33.
 *              A step whose X_t[0], X_t[1], X_t[3] or one of whose six entries is not finite is LOST and takes no part.
 *   cell centre    m = (x_first - i*res, y_first - j*res), with x_first = pos_x + (len_x/2 - res/2) and y_first likewise, as in the
 *              bilinear lookup; res is the geometry's, as it was set.
 *   nearest step   t* is the live step with the smallest |m - p_t|^2 = ex*ex + ey*ey of e = m - p_t, strict <, lowest t on equal
 *              values (a distance that is not finite — a plan 1e150 m away — is never the smallest).  If there is no live step,
 *              out = in for every cell of the solve, no cell is CAPPED and TM_MAX_REACH is 0.
 *   covariance at the cell   d = m - p_t*, scaled down to length r_fp = sqrt(safe_length^2 + safe_width^2)/2 where longer: with
 *              len = sqrt(dx*dx + dy*dy) > r_fp, f = r_fp/len and d = (dx*f, dy*f).  j = (-dy, dx), the footprint point's derivative
 *              over heading.
 *                Cxx = Pxx + 2 jx cx + jx^2 Stt,    Cyy = Pyy + 2 jy cy + jy^2 Stt,    Cxy = Pxy + jx cy + jy cx + jx jy Stt
 *              — the formulas of cilqr_tighten_obstacles (2*jx*cx, jx*jx*Stt, jx*jy*Stt, each product left to right), with the lever
 *              taken at the cell.
 *   reach      hx = kappa*sqrt(max(Cxx, 0)), hy = kappa*sqrt(max(Cyy, 0)) (max(C, 0): 0 where C < 0, else C).  Each is replaced by
 *              max_inflate when it is not finite or exceeds max_inflate: such a cell counts as CAPPED.  ni = floor(hx/res),
 *              nj = floor(hy/res).
 *   dilation   out = the largest finite value among the cell itself and its neighbours (i+a, j+b) that meet all of: |a| <= ni and
 *              |b| <= nj; inside the layer; and, with e = (-a*res, -b*res), det = Cxx*Cyy - Cxy*Cxy,
 *                Cyy*(ex*ex) - 2*Cxy*ex*ey + Cxx*(ey*ey) <= (kappa*kappa)*det.
 *              When det is not above 0 the box alone decides.  A neighbour replaces the running value only where it is strictly
 *              larger (b ascending, then a ascending; this matters between +0 and -0 only).  A cell whose own value is not finite is
 *              copied through: unknown stays unknown.  Every output value is therefore a bit copy of an input value.
 * What this is: the worst occupancy within kappa standard deviations of where the footprint point over that cell may really be —
 * the map form of "grow the ellipse by kappa sigma".  It is axis-capped, first order, and soft, like its sibling: it guarantees
 * nothing.  Judge the final plan against the ORIGINAL map, always.  A cell takes the covariance of the step that passes closest;
 * where a plan crosses itself, or returns to where it was, the LOWEST such step wins and the later, larger Sigma_t is not seen there.
 * tighten [B][CILQR_TIGHTEN_MAP_FIELDS] (required), see the enum.  No floating sums: maxima are lexicographic, counts are integers.
 *   A solve's bits do not depend on B, on its place in the batch, or on whether the layer is shared or one equal copy per solve.
 * Mapping: lane = cell; a solve has G = min(ceil(rows*cols/256), 64) workgroups of 256 lanes that stride over its cells; the
 * per-step records (p_t and the six map-frame entries, 8 doubles per step) are formed once per workgroup in LDS, which the search
 * over t reads at one address per wavefront; the gather reads the set layer.  Each workgroup leaves one record of 5 doubles, merged
 * by a second launch of one wavefront per solve; two launches, no atomics, no arrival order in any result.  Nothing is allocated
 * per call: the records lie in device memory of their own that the handle reserved at create (320*max_batch doubles, not part of the
 * host arena) — a cilqr_tighten_map on ANOTHER stream of the same handle must not run beside it; every other call may.
 * CILQR_ERR_ARG, decided before the handle is looked at: NULL X, sigma, layer_out or tighten; a kappa or max_inflate that is
 * negative or not finite.  Then: B or N beyond the cilqr_create limits; no uncertainty map set on the handle (the message says so);
 * layer_out overlapping the set layer; a map of 2^31 cells or more, or B*G beyond 2^31 - 1.  The host-buffer form stages layer_out through the device arena reserved at create and adds
 * nothing to it: its arrays take B*(20*N + 26 + rows*cols/2) doubles against the max_batch*(22*max_horizon + 34) doubles the arena
 * holds at least, CILQR_ERR_ARG where they do not fit (the node's 150 x 100 map at N = 50: B <= max_batch/8).  The device form is
 * the production path.
 * CILQR_ERR_UNSUPPORTED where the kernel's LDS, 8*(8*N + 20) bytes, = 64*N + 160, exceeds 64 KiB: N above 1021, which CILQR_MAX_HORIZON = 384
 * keeps out of reach — every horizon a handle accepts runs. */
#define CILQR_TIGHTEN_MAP_FIELDS 6
typedef enum cilqr_tighten_map_field {
  CILQR_TM_RAISED = 0,    /* cells with out > in (an integer count) */
  CILQR_TM_MAX_RAISE = 1, /* largest out - in, formed in double;  0 when none */
  CILQR_TM_MAX_CELL = 2,  /* i + rows*j of that maximum, lowest index on equal values;  -1 when none */
  CILQR_TM_MAX_REACH = 3, /* largest of hx, hy after the cap, in metres */
  CILQR_TM_CAPPED = 4,    /* count of capped cells */
  CILQR_TM_LOST = 5       /* number of lost steps */
} cilqr_tighten_map_field;
int cilqr_tighten_map_device(cilqr_handle* h, void* stream, int B, int N, const double* X, const double* sigma, double kappa,
                             double max_inflate, float* layer_out, double* tighten);
int cilqr_tighten_map(cilqr_handle* h, int B, int N, const double* X, const double* sigma, double kappa, double max_inflate,
                      float* layer_out, double* tighten);

/* --- predicted tracks rasterised into the costmap along each plan, for a re-solve (new) -------------------------------------------
 * cilqr_predict_obstacles predicts every tracked vehicle over the horizon with its covariance; its one consumer,
 * cilqr_chance_risk_cov, reads ellipses.  In the reference's live node that channel is off and the blurred costmap of
 * cilqr_set_uncertainty_map is the planner's only obstacle information; a tracked vehicle enters that map in one way only:
 * bondingBoxHandle (here cilqr_rasterize_polygons) paints its box where it is NOW — certain, and it does not move.  So the whole map
 * branch (the map cost in the solve, cilqr_rollout_risk_map, cilqr_chance_risk_map, cilqr_tighten_map) never sees where a mover will be
 * or how sure the tracker is of it.  cilqr_rasterize_tracks(_device) writes, per solve, a copy of the layer set on the handle in which
 * every cell is raised to 100 x the probability that a predicted vehicle covers it, taken at the steps when THAT solve's plan is near
 * the cell.  The layers go where cilqr_tighten_map's go:  predict -> solve -> cilqr_rasterize_tracks -> cilqr_set_uncertainty_map_device
 * (layer_out, layer_stride = rows*cols, the same geometry, poses and probes) -> solve, warm-started from the plan's U.  No solve kernel
 * changes.  With X == NULL the same kernel sweeps the whole horizon (swept mode): the stripe a crossing vehicle paints, for a published
 * predicted-occupancy grid; with zero covariance and inflate 0 its cells at 100 are the cells cilqr_rasterize_polygons marks for the
 * union of the boxes.
 * obs, obs_cov: exactly what cilqr_chance_risk_cov takes — pose [4N] and dim [2N] rows addressed by the strides of cilqr_obstacles,
 * obs_cov 3 doubles (xx, xy, yy) at the pose's entry index or NULL for zero; weight is not read.  Strides (0, N, 1) give one
 * predicted set for all solves: what cilqr_predict_obstacles writes at T = 1.  Entry t belongs to X_t, as that call defines it.  Map,
 * geometry, layer_stride and poses are those CURRENTLY SET on the handle, indexed by the solve as cilqr_tighten_map indexes them.
 * layer_out [B][rows*cols] float32, dense, column-major like the input; it must not overlap the set layer.  X [B][4*(N+1)], the
 * plan, or NULL: swept mode.
 *
 * Definition for solve b and cell (i, j).  Every formula is evaluated in double as C evaluates it as written, left to right, with
 * no fused multiply-add.
 *   cell centre    m = (x_first - i*res, y_first - j*res) as in cilqr_tighten_map, then taken into the planning frame with c, s the
 *              cosine and sine of the solve's map pose heading (obtained as the other map calls obtain them):
 *                w = (pose.x + (c*m.x - s*m.y),  pose.y + (s*m.x + c*m.y)).
 *   entry      e = m*N + t, t = 0 ... N-1, of track m: centre o = (pose[0], pose[1]), heading th = pose[3], co = cos th, so = sin th;
 *                hl = (length + inflate)/2,   hw = (width + inflate)/2      (bondingBoxHandle's rule, whose inflate is 0.2);
 *              with d = w - o the body-frame offsets   du = co*d.x + so*d.y,   dw = co*d.y - so*d.x;   with cc = co*co, ss = so*so,
 *              cs = co*so the variances along the body axes
 *                su2 = cc*Cxx + 2*cs*Cxy + ss*Cyy,   sw2 = ss*Cxx - 2*cs*Cxy + cc*Cyy,   su = sqrt(max(su2, 0)), sw likewise.
 *              An entry whose x, y, th, length, width, Cxx, Cxy or Cyy is not finite is LOST and takes no part.
 *   reach      the entry contributes to the cell only if |du| <= hl + z_max*su and |dw| <= hw + z_max*sw.
 *   marginals  with ku = 1/(su*sqrt 2) where su >= 1e-150:   Pu = 0.5*(erf((du + hl)*ku) - erf((du - hl)*ku));
 *              where su < 1e-150 (it counts as 0: its reciprocal would not be finite) Pu = 1 if |du| <= hl, else 0.  Pw likewise.
 *                p = Pu*Pw                 exact when the covariance is diagonal in the vehicle's frame;
 *                p = min(Pu, Pw)           under CILQR_TRACK_MAP_BOUND_MIN: an upper bound on the covered probability whatever the
 *                                          correlation (the box is inside either strip).
 *              LEFT OUT: the uncertainty of the track's heading and of its size.  The box is taken at its predicted heading.
 *   steps      X == NULL: every t takes part.  Otherwise t* is the plan's nearest live step to the cell by cilqr_tighten_map's rule:
 *              p_t = R'(X_t.xy - pose.xy) for t < N against m in the map frame, the smallest ex*ex + ey*ey, strict <, lowest t on
 *              equal values; a step whose X_t[0] or X_t[1] is not finite is LOST.  The entries with
 *              max(0, t* - window) <= t <= min(N-1, t* + window) take part.  With no live step out = in for every cell.
 *   output     v = (float)(100*max p) over the contributing entries (0 when none).  Where v is 0, out is a bit copy of in: unknown
 *              stays unknown.  Otherwise out = v where in is NaN, else the larger of in and v.
 * What this is: a soft, first-order, time-windowed occupancy.  A cell far from the plan takes the window of a step that never
 * reaches it: harmless, and it raises TKM_RAISED.  It guarantees nothing.  Judge the final plan against the tracks themselves
 * (cilqr_chance_risk_cov) and the ORIGINAL map, always.
 * fields [B][CILQR_TRACK_MAP_FIELDS] (required), see the enum.  Maxima are lexicographic, counts are integers: the largest v, at the
 * lowest cell that has it, with the entry that gave THAT cell its p (the lowest e among the cell's largest p).
 *   A solve's bits do not depend on B, on its place in the batch, or on whether layer, pose and tracks are shared or repeated per
 *   solve.  (A per-solve pose's cosine and sine are formed on the device, the shared pose's on the host, as for every map call.)
 * Mapping: three launches, no atomics, nothing allocated per call.  One lane per entry forms its record (10 doubles, in the planning
 * frame: it depends on neither the map pose nor the solve) — ONE set per call when batch_stride is 0, else one per solve — in device
 * memory the handle reserved at create (10*max_batch*max_obstacles*max_horizon doubles).  Then lane = cell: a solve has
 * G = min(ceil(rows*cols/256), 64) workgroups of 256 lanes that stride over its cells; the plan's positions are staged once per
 * workgroup in LDS, which the search over t reads at one address per wavefront; a cell then reads (2*window + 1)*M records, in swept
 * mode all M*N.  Each workgroup leaves one record of 4 doubles (256*max_batch doubles reserved at create), merged by one wavefront
 * per solve.  A cilqr_rasterize_tracks on ANOTHER stream of the same handle must not run beside it; every other call may.
 * CILQR_ERR_ARG, decided before the handle is looked at: NULL obs, obs->pose, obs->dim, layer_out or fields; B, N or M below 1; an
 * inflate or z_max that is negative or not finite; a negative window; a negative stride; a flag bit other than
 * CILQR_TRACK_MAP_BOUND_MIN.  Then: B, N or M beyond the cilqr_create limits; no uncertainty map set on the handle (the message says
 * so); layer_out overlapping the set layer; a map of 2^31 cells or more, or B*G beyond 2^31 - 1.  The host-buffer form stages
 * layer_out through the device arena reserved at create and adds nothing to it: its arrays take B*(4*N + 10 + rows*cols/2) doubles (6
 * without X) and 9 per entry of the span the strides address (6 without obs_cov), CILQR_ERR_ARG where they do not fit.  With one
 * shared set of M tracks on the node's 150 x 100 map at N = 50, M = 8: every B <= max_batch/8 fits on a handle of max_batch >= 8.
 * The device form is the production path.
 * CILQR_ERR_UNSUPPORTED where the kernel's LDS, 8*(2*N + 20) bytes, exceeds 64 KiB: N above 4086, which CILQR_MAX_HORIZON = 384 keeps
 * out of reach — every (N, M) a handle accepts runs. */
#define CILQR_TRACK_MAP_FIELDS 6
typedef enum cilqr_track_map_field {
  CILQR_TKM_RAISED = 0,       /* cells whose output differs from the input (integer count) */
  CILQR_TKM_MAX_VALUE = 1,    /* largest v of the solve (0..100), 0 when none */
  CILQR_TKM_MAX_CELL = 2,     /* i + rows*j of it, lowest on equal values; -1 when none */
  CILQR_TKM_MAX_ENTRY = 3,    /* m*N + t of the entry that gave it, lowest on equal values; -1 when none */
  CILQR_TKM_LOST_ENTRIES = 4, /* entries that took no part (not finite) */
  CILQR_TKM_LOST_STEPS = 5    /* plan steps that took no part; 0 in swept mode */
} cilqr_track_map_field;
#define CILQR_TRACK_MAP_BOUND_MIN 1u
int cilqr_rasterize_tracks_device(cilqr_handle* h, void* stream, int B, int N, int M, const double* X, const cilqr_obstacles* obs,
                                  const double* obs_cov, double inflate, double z_max, int window, uint32_t flags, float* layer_out,
                                  double* fields);
int cilqr_rasterize_tracks(cilqr_handle* h, int B, int N, int M, const double* X, const cilqr_obstacles* obs, const double* obs_cov,
                           double inflate, double z_max, int window, uint32_t flags, float* layer_out, double* fields);

/* --- analytic map risk: the pose covariance against the uncertainty map by quadrature (new) ---------------------------------------
 * cilqr_chance_risk stops at the ellipses; in the reference's live node that channel is off and the blurred costmap is the only
 * obstacle information (see cilqr_rollout_risk_map), for which the only risk call so far is the sampled one: risk in steps of 1/S,
 * dependent on the offsets' seed, every rollout a serial chain over the horizon.  cilqr_chance_risk_map(_device) is the map
 * counterpart of cilqr_chance_risk: per step it takes the pose marginal (x, y, theta) of Sigma_t, places a caller-supplied set of Q
 * weighted standard-normal nodes through its Cholesky factor around the plan's pose, and looks the footprint up under every node.
 * No rollouts, no gains, no chain over the horizon: the N*Q node poses of a solve are independent.
 * X [B][4*(N+1)], the plan.  sigma [B][N+1][16], exactly sigma_out of cilqr_chance_risk (column-major, entry (r, c) at [r + 4*c]);
 * of each Sigma_t, t < N, six entries are read: (0,0), (0,1), (1,1), (0,3), (1,3), (3,3).  Sigma_N and x_N are not visited, as in
 * cilqr_rollout_risk_map.  nodes [Q][3] = (z_x, z_y, z_theta) and weights [Q], shared by the batch, 1 <= Q <= CILQR_MAX_QUAD_NODES;
 * cilqr_pose_quadrature builds Gauss-Hermite sets, and any other set serves: S equal-weight standard-normal draws make the call
 * a sampled estimate of the same marginals.  Map, layer stride, poses and probes are those CURRENTLY SET on the handle, indexed
 * by the solve as in cilqr_rollout_risk_map.
 *
 * Definitions.
 *   factor     with c00 = S(0,0), c10 = S(0,1), c11 = S(1,1), c20 = S(0,3), c21 = S(1,3), c22 = S(3,3) of S = Sigma_t:
 *                l00 = sqrt(max(c00, 0));                     l10 = c10/l00 and l20 = c20/l00, each 0 when l00 = 0;
 *                l11 = sqrt(max(c11 - l10^2, 0));             l21 = (c21 - l20*l10)/l11, 0 when l11 = 0;
 *                l22 = sqrt(max(c22 - l20^2 - l21^2, 0)).
 *              A marginal that is singular or slightly indefinite loses the directions it does not have; nothing fails.
 *   node pose  x = X_t[0] + l00*z_x,   y = X_t[1] + l10*z_x + l11*z_y,   theta = X_t[3] + l20*z_x + l21*z_y + l22*z_theta.
 *   probes, valid, occupancy   word for word those of cilqr_rollout_risk_map: the probes_l x probes_w footprint on safe_length x
 *              safe_width turned by the node's heading, the rigid transform by the map pose of the solve's index, bilinear
 *              interpolation over four cell centres in double; a probe is valid when its four cells are inside and finite.
 *   hit        node q HITS at step t when a valid probe's occupancy is > occ_threshold (strict), or
 *              CILQR_CHANCE_MAP_UNKNOWN_HITS is set and a probe is invalid.   unknown: at least one probe is invalid.
 *   per step   r_t = min(1, sum over q of w_q [hit]),   u_t = min(1, sum over q of w_q [unknown]),   e_t = sum over q of w_q m_q
 *              with m_q the largest valid occupancy among node q's probes, 0 when it has none.  The weights are used as given and
 *              not normalised; a sum of r_t or u_t that is NaN gives 1 (a weight that is NaN, which only the device form can
 *              be handed).  r_t is a quadrature of an INDICATOR: with Gauss-Hermite nodes it resolves the mass beyond the
 *              threshold contour only as finely as the nodes sample it (7 x 7 x 3 nodes were up to 0.05 off the
 *              rollouts' share on the test scene, while equal-weight draws reproduce it).  e_t, the expected occupancy under the
 *              footprint, is smooth and converges with a few nodes per axis: both are reported.
 *   lost step  a step where X_t[0], X_t[1], X_t[3] or one of the six entries is not finite: r_t = 1, u_t = 1, e_t = 0, and the
 *              step adds nothing to CM_WORST_OCC.
 * step_risk, step_occ, step_unknown [B][N] hold r_t, e_t, u_t; each may be NULL.  risk [B][CILQR_CHANCE_MAP_FIELDS] (required),
 * see the enum; ties go to the lowest index.  total [B] or NULL: total[b] = base[b] when the bounded field — CM_STEP_RISK, or
 * CM_SUM_RISK under CILQR_CHANCE_MAP_BOUND_SUM — is <= max_risk and base[b] is finite, else NaN: the convention of
 * cilqr_chance_risk, so the call composes with it (base = its total) and with the rollout risk calls and feeds cilqr_argmin_device /
 * cilqr_argmin_global_device.  total without base is CILQR_ERR_ARG.
 *   Determinism: every sum over the nodes runs over a tree fixed by Q alone (a lane adds its nodes q = lane, lane + 64, ... in
 *   ascending order, the 64 lane sums meet in a fixed butterfly), the sum over the horizon over a tree fixed by N alone; maxima are
 *   lexicographic.  A solve's bits do not depend on B, on its place in the batch, or on whether the layer is shared or one equal
 *   copy per solve.  (A per-solve pose's cosine and sine are formed on the device, the shared pose's on the host: equal poses
 *   given the two ways may differ in the last bit, as for every call that reads the map.)
 * Mapping: lane = node, wavefront = step, a workgroup takes four consecutive steps of one solve: ceil(N/4)*B workgroups, then one
 * wavefront per solve for the reduction over the horizon; two launches, no atomics.  LDS is 32*Q + 32 bytes whatever N is: every
 * horizon a handle accepts runs, and CILQR_ERR_UNSUPPORTED is never returned.  Nothing is allocated per call.  Where the caller
 * passes NULL for a per-step output its values live in device memory the handle reserved at create (3*max_batch*max_horizon
 * doubles); each workgroup's largest occupancy lies in the buffer of cilqr_rollout_risk's partial records — a cilqr_rollout_risk,
 * cilqr_rollout_risk_map or cilqr_chance_risk_map on ANOTHER stream of the same handle must not run beside it.
 * CILQR_ERR_ARG, decided before the handle is looked at: NULL X, sigma, nodes, weights or risk; total without base; Q outside
 * 1 ... CILQR_MAX_QUAD_NODES; an occ_threshold or max_risk that is NaN; flag bits other than the two below; in the host-buffer
 * form also a weight that is negative or not finite.  Then: B or N beyond the cilqr_create limits; no uncertainty map set on the
 * handle (the message says so).  The host-buffer form's arrays must fit the device arena reserved at create (CILQR_ERR_ARG
 * otherwise; this call adds nothing to it): B*(20*N + 30) + 4*Q doubles, and 3*B*N more with the three per-step outputs, against
 * the max_batch*(22*max_horizon + 34) doubles the arena holds at least.  Without per-step outputs every B <= max_batch fits once
 * 4*Q <= max_batch*(2*max_horizon + 4); with them every B <= 7*max_batch/8 fits once 4*Q <= max_batch*(max_horizon + 7). */
#define CILQR_MAX_QUAD_NODES 1024
#define CILQR_CHANCE_MAP_FIELDS 8
typedef enum cilqr_chance_map_field {
  CILQR_CM_STEP_RISK = 0,     /* max over t of r_t: what max_risk bounds by default */
  CILQR_CM_WORST_STEP = 1,    /* lowest t of that maximum */
  CILQR_CM_SUM_RISK = 2,      /* min(1, sum over t of r_t): Boole's bound over the horizon.  Bounded instead of CM_STEP_RISK under
                                 CILQR_CHANCE_MAP_BOUND_SUM */
  CILQR_CM_FIRST_STEP = 3,    /* lowest t with r_t > 0;  -1 when none */
  CILQR_CM_MEAN_OCC = 4,      /* max over t of e_t */
  CILQR_CM_MEAN_OCC_STEP = 5, /* lowest t of that maximum */
  CILQR_CM_WORST_OCC = 6,     /* largest valid occupancy under any node, t < N;  -HUGE_VAL when no probe is valid */
  CILQR_CM_UNKNOWN = 7        /* max over t of u_t */
} cilqr_chance_map_field;
#define CILQR_CHANCE_MAP_UNKNOWN_HITS 1u /* flags: an invalid probe counts as a hit */
#define CILQR_CHANCE_MAP_BOUND_SUM 2u    /* flags: max_risk bounds CM_SUM_RISK */
int cilqr_chance_risk_map_device(cilqr_handle* h, void* stream, int B, int N, int Q, const double* X, const double* sigma,
                                 const double* nodes, const double* weights, double occ_threshold, uint32_t flags, double max_risk,
                                 const double* base, double* risk, double* step_risk, double* step_occ, double* step_unknown,
                                 double* total);
int cilqr_chance_risk_map(cilqr_handle* h, int B, int N, int Q, const double* X, const double* sigma, const double* nodes,
                          const double* weights, double occ_threshold, uint32_t flags, double max_risk, const double* base,
                          double* risk, double* step_risk, double* step_occ, double* step_unknown, double* total);
/* Host only, no device: the tensor product of probabilists' Gauss-Hermite rules (weight exp(-z^2/2), each axis' weights summing to
 * 1) with nx, ny, nth nodes per axis, each in 1 ... 9 (CILQR_ERR_ARG otherwise, or for a NULL pointer).  Writes nx*ny*nth nodes
 * (z_x, z_y, z_theta) and weights w_x*w_y*w_theta, z_theta fastest, z_x slowest, each axis ascending.  The roots of He_n come by
 * Newton's iteration inside the brackets the roots of He_(n-1) give (they interlace), mirrored about 0; the weights are
 * (n-1)! / (n He_(n-1)(z)^2), scaled to sum to 1: no table is involved and the same arguments give the same bits. */
int cilqr_pose_quadrature(int nx, int ny, int nth, double* nodes, double* weights);

/* --- analytic chance risk against sampled obstacles in compact form (new) --------------------------------------------------------
 * cilqr_chance_risk stops at ordinary obstacles: for the sampled scene form — n_obs obstacles x n_samples Gaussian pose samples —
 * the only judge under ego-pose noise so far is cilqr_rollout_risk_sampled: risk in steps of 1/(S*n_samples), dependent on the
 * offsets' seed, every rollout row a serial chain over the horizon.  cilqr_chance_risk_sampled(_device) is its analytic
 * counterpart: given Sigma_t it needs no rollouts, no gains and no chain, and the N*n_obs*n_samples entries of a solve are
 * independent.  Materialising the samples for cilqr_chance_risk is no substitute: that table has no notion of "the samples of one
 * obstacle are ONE obstacle" (its r_t would add the samples' chances where this call averages them), and its LDS formula rejects
 * 8 x 32 samples at N = 50.
 * X [B][4*(N+1)], the plan.  sigma [B][N+1][16], exactly sigma_out of cilqr_chance_risk (column-major, entry (r, c) at [r + 4*c];
 * that call with M = 0 supplies it); as in cilqr_tighten_obstacles six entries of each Sigma_t, t < N, are read: (0,0), (0,1), (0,3),
 * (1,1), (1,3), (3,3).  Sigma_N and x_N are not visited.  The scene in the compact form of cilqr_gains_batch_sampled: nom_pose
 * [B][n_obs][4*N], nom_dim [B][n_obs][2*N], sample_offset [B][n_obs][n_samples][3] = (dx, dy, dtheta).  Materialised obstacle
 * m = o*n_samples + j has the pose (x + dx, y + dy, v, theta + dtheta) of nominal obstacle o — plain additions, not the solve
 * kernels' angle-addition shortcut — and o's dimensions: its entry carries the bits of the materialised table's.  Cost weights,
 * the path and an uncertainty map set on the handle are not read.
 *
 * Definitions.
 *   entry chance   p(m, t): entry_p of cilqr_chance_risk for materialised obstacle m, word for word — cbar, g (lever arm included),
 *                  s = sqrt(max(g' Sigma_t g, 0)), p = erfc(-cbar / (s*sqrt 2)) / 2; with s = 0: 1 if cbar > 0, else 0; the larger of
 *                  the two circles' values, taken as erfc of the smaller argument; a NaN never wins a maximum.  Where Sigma_t and the
 *                  materialised entry agree, p equals that call's entry_p[m*N + t] bit for bit.
 *   pair chance    q(o, t) = (sum over j of p(o*n_samples + j, t)) / n_samples: the chance of contact with obstacle o at step t
 *                  under the ego Gaussian and the obstacle's empirical pose distribution (equal-weight samples); the analytic
 *                  counterpart of RRS_PAIR_SHARE.  The sum runs over a tree fixed by n_samples alone: with W the power of two with
 *                  n_samples <= W, at least 2 and at most 64, slot i < W holds p(j = i) + p(j = i + W) + ... added in ascending j
 *                  (one term unless n_samples > 64; +0 where i >= n_samples), and the W slots meet in an xor butterfly: at offsets
 *                  W/2, W/4, ..., 1 in turn every slot i takes slot[i] + slot[i xor offset]; q is slot 0 divided by n_samples.
 *   per step       r_t = min(1, sum over o of q(o, t)), Boole's bound over the obstacles, summed in ascending o; a sum that is NaN
 *                  gives 1.
 *   lost step      a step where X_t[0], X_t[1], X_t[3] or one of the six entries of Sigma_t is not finite: r_t = 1 (its p and q are
 *                  still formed as defined).  A U_t or K_t that is not finite reaches this call only through Sigma_{t+1}: the M = 0
 *                  cilqr_chance_risk call that supplies sigma marks that step ITSELF (its r_t = 1, so its total is NaN under any
 *                  max_risk < 1).  Pass that call's total as `base` here and composing the two loses nothing.
 *   nominal share  n(o, t) = #{j : cbar > 0 for either circle of entry (o*n_samples + j, t)} / n_samples, an integer count; with
 *                  Sigma = 0 it equals q(o, t) exactly.
 * risk [B][CILQR_CRS_FIELDS] (required), see the enum.  step_risk [B][N] = r_t, pair_p [B][n_obs][N] = q, entry_p
 * [B][n_obs*n_samples][N] = p; each may be NULL.  total [B] or NULL: total[b] = base[b] when the bounded field — CRS_STEP_RISK, or
 * CRS_SUM_RISK under CILQR_CHANCE_SAMPLED_BOUND_SUM — is <= max_risk and base[b] is finite, else NaN (a NaN base stays NaN): the
 * convention of cilqr_chance_risk, so the call composes with it, with cilqr_chance_risk_map and with the rollout risk calls
 * through `base` and feeds cilqr_argmin_device / cilqr_argmin_global_device.  total without base is CILQR_ERR_ARG.
 *   Determinism: the sum over the samples runs over the tree above, the sum over the obstacles in ascending o, the sum over the
 *   horizon over a tree fixed by N alone (lane l of 64 adds r_t for t = l, l + 64, ... ascending, the lane sums meet in the same
 *   butterfly); maxima are lexicographic, lowest index first.  A solve's bits depend on its own inputs alone: not on B, and not on
 *   its place in the batch.
 * Mapping: wavefront = step, a workgroup takes four consecutive steps of one solve: ceil(N/4)*B workgroups whose lanes take the
 * step's n_obs*n_samples entries, then one wavefront per solve for the reduction over the horizon; two launches, no atomics.
 * Nothing is allocated per call; the
 * per-step records between the two launches lie in device memory the handle reserved at create (5*max_batch*max_horizon doubles,
 * not part of the host arena) — a cilqr_chance_risk_sampled on ANOTHER stream of the same handle must not run beside it; every
 * other call may.
 * CILQR_ERR_ARG, decided before the handle is looked at: NULL X, sigma, nom_pose, nom_dim, sample_offset or risk; total without
 * base; n_obs < 1 or n_samples < 2; a max_risk that is NaN; flag bits other than CILQR_CHANCE_SAMPLED_BOUND_SUM.  Then: B, N or
 * n_obs*n_samples beyond the cilqr_create limits; n_obs*n_samples*N or B*ceil(N/4) beyond 2^31 - 1.  The host-buffer form's arrays
 * must fit the device arena reserved at create (CILQR_ERR_ARG otherwise; this call adds nothing to it): per solve 20*N +
 * 6*n_obs*N + 3*n_obs*n_samples + 30 doubles, N + n_obs*N more with step_risk and pair_p, n_obs*n_samples*N more with entry_p.
 * Without entry_p every B <= max_batch fits; with it every B <= max_batch fits on a handle of max_horizon >= 2, and every
 * B <= max_batch/2 on a handle of max_horizon 1.
 * CILQR_ERR_UNSUPPORTED where the kernel's LDS, 32*n_obs*n_samples bytes whatever N is (the erfc arguments of a step, 8 bytes per
 * entry, for the four steps of a workgroup), exceeds 64 KiB: n_obs*n_samples above 2048.  Every horizon a handle accepts runs. */
#define CILQR_CRS_FIELDS 8
typedef enum cilqr_chance_risk_sampled_field {
  CILQR_CRS_STEP_RISK = 0,     /* max over t of r_t: what max_risk bounds by default */
  CILQR_CRS_WORST_STEP = 1,    /* lowest t of that maximum */
  CILQR_CRS_SUM_RISK = 2,      /* min(1, sum over t of r_t), over a tree fixed by N: Boole's bound over the horizon.  Bounded instead
                                  of CRS_STEP_RISK under CILQR_CHANCE_SAMPLED_BOUND_SUM */
  CILQR_CRS_MAX_PAIR_P = 3,    /* max over (o, t) of q;  0 when every q is NaN */
  CILQR_CRS_MAX_PAIR = 4,      /* o*N + t of that maximum, lowest on equal values;  -1 when every q is NaN */
  CILQR_CRS_MAX_ENTRY_P = 5,   /* max over entries of p;  0 when every p is NaN */
  CILQR_CRS_MAX_ENTRY = 6,     /* m*N + t of that maximum, lowest on equal values;  -1 when every p is NaN */
  CILQR_CRS_NOMINAL_SHARE = 7  /* max over (o, t) of n(o, t): equals CILQR_SCORE_COLLISION of cilqr_score_batch_sampled on the plan */
} cilqr_chance_risk_sampled_field;
#define CILQR_CHANCE_SAMPLED_BOUND_SUM 1u /* flags: max_risk bounds CRS_SUM_RISK */
int cilqr_chance_risk_sampled_device(cilqr_handle* h, void* stream, int B, int N, int n_obs, int n_samples, const double* X,
                                     const double* sigma, const double* nom_pose, const double* nom_dim, const double* sample_offset,
                                     uint32_t flags, double max_risk, const double* base, double* risk, double* step_risk,
                                     double* pair_p, double* entry_p, double* total);
int cilqr_chance_risk_sampled(cilqr_handle* h, int B, int N, int n_obs, int n_samples, const double* X, const double* sigma,
                              const double* nom_pose, const double* nom_dim, const double* sample_offset, uint32_t flags,
                              double max_risk, const double* base, double* risk, double* step_risk, double* pair_p, double* entry_p,
                              double* total);

/* --- tracked obstacles predicted over the horizon, with their covariance (new) ----------------------------------------------------
 * Every call above that reads ordinary obstacles takes a finished table, [M][4*N] poses and [M][2*N] dimensions, and the obs_cov of
 * cilqr_tighten_obstacles had no producer.  cilqr_predict_obstacles(_device) makes both on the device from what a tracker hands
 * over once per tick: one state and one covariance per vehicle, rolled out at constant acceleration and yaw rate.
 * T track sets of M vehicles.  T = 1 is the planner's case, one set of vehicles for every candidate: the outputs are then addressed
 * with cilqr_obstacles strides (0, N, 1), and cov_out by the same entry index as obs_cov.  T = B gives one set per solve, strides
 * (M*N, N, 1).
 *   track       [T][M][6]   (x, y, v, theta, a, omega): the state in the planner's order, then a constant acceleration and yaw rate
 *   track_dim   [T][M][2]   (length, width)
 *   track_cov   [T][M][16]  or NULL (zero): P_0, column-major, entry (r, c) at [r + 4*c], state order (x, y, v, theta); only
 *                           row <= column is read, the convention of sigma0
 *   track_noise [16]        or NULL (zero): Q per step, shared by every track; only row <= column is read
 *   pose_out    [T][M][4*N] required: the predicted poses
 *   dim_out     [T][M][2*N] required: track_dim bit-copied to every step
 *   cov_out     [T][M][N][3]  or NULL: (xx, xy, yy) of P_t — exactly the obs_cov layout of cilqr_tighten_obstacles
 *   sigma_out   [T][M][N][16] or NULL: every P_t, exactly symmetric
 * Definition per track, dt = Parameters::timestep.  Entry t belongs to the ego's X_t, so entry 0 is the tracked state itself:
 *   pose[t] = (x_t, y_t, v_t, theta_t); cov[t] and sigma[t] come from P_t.  Entry 0 is a bit copy of the inputs (for P_0 the lower
 *   triangle is mirrored from the upper).  Step t -> t+1:
 *     stop = (v_t + a*dt < 0),   a_t = stop ? -v_t/dt : a,   adv = v_t*dt + a_t*dt^2/2,
 *     x_{t+1} = x_t + cos(theta_t)*adv,   y_{t+1} = y_t + sin(theta_t)*adv,
 *     v_{t+1} = stop ? 0 : v_t + a*dt     (a braking vehicle stops and does not reverse),
 *     theta_{t+1} = theta_t + omega*dt.
 *   The ego's acceleration, yaw-rate and speed clamps are NOT applied: they are the ego's limits, not the other vehicle's.
 *     P_{t+1} = A_t P_t A_t' + Q,   A_t the A of cilqr_chance_risk above (Model::get_A_matrix) at (v_t, theta_t, a_t):
 *     A = I + { (0,2): dt*cos theta, (1,2): dt*sin theta, (0,3): -sin theta*adv, (1,3): cos theta*adv }.
 *   Entries with row <= column are computed and mirrored.  The floor on v does not enter A_t: A(2,2) = 1 always, so after a stop
 *   the speed variance is carried on and the position covariance keeps growing — the conservative side.
 *   Values are not checked: a NaN propagates through its own track only.  A track's outputs depend on that track's inputs (and on
 *   track_noise and N) alone: the same bits whatever T and M are and wherever the track sits.
 * Mapping: one wavefront per track, T*M workgroups, one launch, nothing allocated per call.  Speeds and headings by their
 * recurrences, then the steps' sincos and A_t entries in parallel, then the serial chain written out for the four non-zero
 * entries of A_t - I, then coalesced stores from LDS.
 * CILQR_ERR_ARG, decided before the handle is looked at where no handle is needed: NULL track, track_dim, pose_out or dim_out; T, N
 * or M < 1; then T beyond max_batch, N beyond max_horizon, M beyond max_obstacles.  The host-buffer form's arrays must fit the
 * device arena reserved at create (CILQR_ERR_ARG otherwise; this call adds nothing to it): T*M*(24 + 25*N) + 16 doubles with every
 * output, T*M*(24 + 9*N) + 16 without sigma_out.  With every output every T <= max_batch/8 always fits; without sigma_out every
 * T <= max_batch/5 does.
 * CILQR_ERR_UNSUPPORTED where the kernel's LDS, 8*18*N bytes (per step the pose, four coefficients and ten covariance entries),
 * exceeds 64 KiB: N above 455, which CILQR_MAX_HORIZON = 384 keeps out of reach — every horizon a handle accepts runs. */
int cilqr_predict_obstacles_device(cilqr_handle* h, void* stream, int T, int N, int M, const double* track, const double* track_dim,
                                   const double* track_cov, const double* track_noise, double* pose_out, double* dim_out,
                                   double* cov_out, double* sigma_out);
int cilqr_predict_obstacles(cilqr_handle* h, int T, int N, int M, const double* track, const double* track_dim, const double* track_cov,
                            const double* track_noise, double* pose_out, double* dim_out, double* cov_out, double* sigma_out);

/* --- the analytic pose-noise risk with the obstacle's own covariance (new) -----------------------------------------------------------
 * cilqr_chance_risk takes the obstacle as certain.  cilqr_chance_risk_cov(_device) is that call with one more argument after obs:
 * obs_cov, NULL or 3 doubles (xx, xy, yy; world frame) at obs_cov + 3*e for the same entry index e = b*batch_stride +
 * m*obstacle_stride + t*step_stride that addresses the entry's pose — the convention of cilqr_tighten_obstacles, and what
 * cilqr_predict_obstacles writes to cov_out.  With gx, gy the first two components of g, the quadratic form of an entry becomes
 *     q' = g' Sigma_t g + (gx^2*Cxx + 2*gx*gy*Cxy + gy^2*Cyy),     s = sqrt(max(q', 0)),
 * and the rest is cilqr_chance_risk's.  The ego's and the obstacle's errors are taken as INDEPENDENT; the obstacle's heading and
 * size uncertainty are left out (the ellipse keeps its axes and its orientation).  An entry whose three obs_cov values are not all
 * finite gets entry_p = 1: the judge cannot vouch for it.  The fields, step_risk, entry_p, sigma_out, total / base / max_risk and
 * the flags are unchanged in meaning.  obs_cov == NULL: every output has the bits of cilqr_chance_risk; so it has with an obs_cov
 * that is all zero (q + 0 is q).  A solve's bits do not depend on the batch or on the strides.
 * Errors, limits and the LDS formula are those of cilqr_chance_risk (a second instantiation of its kernel).  The host-buffer form
 * carries 3 doubles of obs_cov per entry of the obstacle span, as cilqr_tighten_obstacles does, and adds nothing to the arena: with
 * dense obstacles 15*N + 9*M*N + 28 doubles per solve without sigma_out and entry_p, 31*N + 10*M*N + 44 with both — with obs_cov
 * every B <= max_batch/2 always fits, with or without the two outputs. */
int cilqr_chance_risk_cov_device(cilqr_handle* h, void* stream, int B, int N, int M, const double* X, const double* U, const double* K,
                                 const double* sigma0, int64_t sigma0_batch_stride, const double* process_noise,
                                 const cilqr_obstacles* obs, const double* obs_cov, uint32_t flags, double max_risk, const double* base,
                                 double* risk, double* step_risk, double* entry_p, double* sigma_out, double* total);
int cilqr_chance_risk_cov(cilqr_handle* h, int B, int N, int M, const double* X, const double* U, const double* K, const double* sigma0,
                          int64_t sigma0_batch_stride, const double* process_noise, const cilqr_obstacles* obs, const double* obs_cov,
                          uint32_t flags, double max_risk, const double* base, double* risk, double* step_risk, double* entry_p,
                          double* sigma_out, double* total);

/* --- the cross-GPU exchange step (SURVEY §8b "Entry point", §8e; new: the reference has no collective) ------------------
 * The batch shards by scene with no data-path collective; the ONE exchange is the min-cost pick: every rank's
 * {J_min, local index, index offset} (24 bytes) through one ncclAllGather (RCCL over xGMI), then the lexicographic minimum
 * on the device, lowest global index winning ties (the strict-< first-minimum convention of I/Constraints.cpp:50).
 *
 * One process per GPU: rank 0 calls cilqr_comm_unique_id (ncclGetUniqueId), the host carries the CILQR_COMM_ID_BYTES to every
 * rank by its own means (MPI_Bcast, a file, torch.distributed's store), every rank calls cilqr_comm_init_rank on its handle
 * (ncclCommInitRank: collective, blocks until all ranks arrive).  cilqr_destroy releases the communicator. */
int cilqr_comm_unique_id(void* id_bytes /* CILQR_COMM_ID_BYTES, out */);
int cilqr_comm_init_rank(cilqr_handle* h, int n_ranks, int rank, const void* id_bytes);
int cilqr_comm_destroy(cilqr_handle* h);
int cilqr_comm_size(const cilqr_handle* h); /* ranks of the handle's communicator; 1 without one */
/* Global min-cost selection, asynchronous on `stream`: argmin of this rank's J[B] (device; B = 0: the rank has no scenes) →
 * all-gather → out_pair (device, 2 doubles) = {J_min, (double)global index}, the same on every rank; global index =
 * index_offset + local index; index -1: no rank had a finite cost.  Without a communicator it is the local pick plus offset.
 * Every rank of the communicator must call it, in the same order relative to its other collective calls. */
int cilqr_argmin_global_device(cilqr_handle* h, void* stream, int B, const double* J, int64_t index_offset, double* out_pair);

/* Test hook: the cross-rank pick alone, over n gathered records {J_min, local index, index offset} given in host memory →
 * out_pair (host, 2 doubles).  Lets the device-side combine rule be checked for several ranks on a one-GPU box. */
int cilqr_debug_select(cilqr_handle* h, int n, const double* triples, double* out_pair);

/* One process driving n_devices GPUs (the host model of the reference: one C++ process): one handle, stream and RCCL
 * communicator per device (ncclCommInitAll); devices = NULL means ordinals 0..n_devices-1.  Mirrors
 * iLQR::iLQR / get_optimal_control_seq like cilqr_create / cilqr_solve_batch do, for a batch that spans devices. */
typedef struct cilqr_multi cilqr_multi;
int cilqr_create_multi(const cilqr_params* p, int max_batch_per_device, int max_horizon, int max_obstacles, int n_devices,
                       const int* devices, cilqr_multi** out);
int cilqr_multi_destroy(cilqr_multi* m);
int cilqr_multi_device_count(const cilqr_multi* m);
cilqr_handle* cilqr_multi_handle(cilqr_multi* m, int i); /* device i's handle, for the *_device entry points */
/* The shard of a batch of B solves that device (or rank) `shard` of `n_shards` owns: contiguous by scene and balanced — the first
 * B mod n shards own one solve more; shards may be empty when B < n.  Host arithmetic only (no device needed): the rule
 * cilqr_multi_solve_batch applies, exported so that a one-process-per-GPU host shards the same way. */
int cilqr_shard_range(int B, int n_shards, int shard, int* first, int* count);
/* cilqr_solve_batch over all devices: host buffers as there, solves sharded by cilqr_shard_range, followed by the exchange
 * step; best_index / best_J (may be NULL) receive the global min-cost pick.  Each device's shard is enqueued (copies in,
 * kernels, copies out, the shard's argmin) by its own host thread, so the devices overlap whatever the caller's memory is:
 * from pageable buffers a hipMemcpyAsync is a synchronous copy, and one thread walking the devices would serialise them; with
 * buffers from cilqr_host_alloc the copies are true DMA transfers on every device's own stream.  On any failure every
 * device's stream is drained before the error is returned — no copy into caller memory is left in flight — and the handles
 * are free for the next call.
 * A device list that names one device several times (shards sharing a GPU: how a one-GPU box rehearses the n-shard path) gets
 * no RCCL communicator — RCCL cannot span a device twice — and gathers the 24-byte records with device copies ordered by
 * events instead; cilqr_multi_uses_rccl tells which. */
int cilqr_multi_solve_batch(cilqr_multi* m, int B, int N, int M, const double* x0, double* U, const double* poly,
                            const double* xplan_fl, const double* obs_pose, const double* obs_dim, const double* obs_weight,
                            double* X_out, double* J_out, int32_t* iters_out, int32_t* status_out, uint32_t flags,
                            int64_t* best_index, double* best_J);
int cilqr_multi_uses_rccl(const cilqr_multi* m); /* 1: distinct devices, exchange by ncclAllGather; 0: shards share a device */
/* Test hook: the nth_call-th host-buffer solve enqueued on `h` from now on fails AFTER its input copies were enqueued
 * (nth_call = 1: the next one; 0 switches the hook off) — the error path of cilqr_solve_batch / cilqr_multi_solve_batch with
 * asynchronous copies in flight. */
int cilqr_debug_fail_enqueue(cilqr_handle* h, int nth_call);

/* Diagnostics (the reference's only tracing is std::chrono around run_step, I/ilqr_uncertainty_node.cpp:117-124): while
 * dev_buf != NULL, solves run a separately compiled, stamped instantiation of the kernel that writes, per solve, 16
 * uint64 to dev_buf[B][16] (device memory owned by the caller): shader-clock totals {prologue, linearise, Riccati, forward,
 * epilogue, #linearise, #Riccati, total}, then (one-wavefront-per-solve family; 0 elsewhere) totals inside the linearisation
 * {cos/sin columns, closest path sample, cost derivatives, record stores, cost reduction} and inside the Riccati steps
 * {products up to Q_uu in scalar registers, determinant and reciprocal, rest of the step}.  NULL restores the production
 * kernel.  Never use it when timing. */
int cilqr_set_diag_buffer(cilqr_handle* h, uint64_t* dev_buf);

/* Measurement hook: while dev_buf != NULL every solve also writes the number of backward + forward passes it actually
 * executed to dev_buf[B] (device int32, owned by the caller).  The production kernels stop at the first rejected iteration
 * (DESIGN.md §4.3), so this is smaller than iters_out, the reference loop's iteration count; bench.py prices its fp64 estimate
 * with it.  NULL switches it off. */
int cilqr_set_pass_count_buffer(cilqr_handle* h, int32_t* dev_buf);

/* Which kernel family a solve of this shape takes on this handle: the number of lanes per solve — 64 = one
 * wavefront per solve, LDS-resident (cilqr_solve.hip); 32 … 1 = the grouped family (cilqr_solve_groups.hip), 64/G solves per
 * wavefront.  The same rule cilqr_solve_batch(_device) applies (CILQR_FORCE_G in the environment at create overrides it);
 * measurement tools label their figures with it instead of restating the rule.  Negative: error code. */
int cilqr_solve_family(const cilqr_handle* h, int B, int N, int M);
/* Wavefronts per solve of cilqr_solve_batch(_device) on the one-wavefront family: 2 or 3 where further wavefronts take the obstacle,
 * Jacobian and control-barrier terms of phase L while the first searches the closest path samples (cilqr_solve_share_kernel, DESIGN.md
 * §4.2: three up to three quarters of a solve per SIMD, at least two obstacles and N ≤ 64, two up to two solves per SIMD and N ≤ 127; obstacle
 * table in LDS — a solve's LDS share grows where fewer solves share a CU; with an uncertainty map set, whose term then goes to the
 * last of the further wavefronts: three up to half a solve per SIMD, two up to one — two also where the partial sums of three would
 * take a solve with a large obstacle table past the 160 KiB of LDS of a CU; results bit-identical to the one-wavefront kernel; CILQR_NO_SHARE_KERNEL in the environment at create switches it
 * off, CILQR_SHARE_W = 2 or 3 fixes the number), else 1 (also for every shape cilqr_solve_family sends to the grouped family).
 * CILQR_FLAG_FAITHFUL_ITERS always runs on one, and under CILQR_PAIR_KERNEL (the two-wavefront experiment) the answer
 * is 1 at every batch size.  Together with cilqr_solve_family and cilqr_solve_sampled_wavefronts it reads the launch plan the solve
 * entry points themselves follow (csrc/cilqr_wave_plan.h, plan_wave: one host-side function of the batch shape and the handle's
 * environment knobs), for flags = 0 and the handle's current map.  Negative: error code. */
int cilqr_solve_wavefronts(const cilqr_handle* h, int B, int N, int M);
/* The same for cilqr_solve_batch_sampled(_device): how many wavefronts share a solve's phase L on this handle — 1 (one wavefront
 * per solve: horizons beyond 64, CILQR_NO_SPLIT_KERNEL), 2 or 4 (cilqr_solve_split_kernel, DESIGN.md
 * §4.1c).  CILQR_FLAG_FAITHFUL_ITERS always runs on one.  The answer is the rule by shape alone (there is no n_samples here to size
 * the LDS with): a call whose sample records take the split kernel's LDS beyond 64 KiB runs on one wavefront all the same.
 * Negative: error code. */
int cilqr_solve_sampled_wavefronts(const cilqr_handle* h, int B, int N, int n_obs);

/* Test hook: runs the kernels' own regularised Q_uu inverse (I/iLQR.cpp:155-175) on n column-major 2×2 matrices (host
 * buffers).  general = 0: the positive-semi-definite form of the production kernel; 1: the eigenvalue-clamping form of the
 * GENERAL kernel (NaN rows where it reports a non-finite matrix).  Lets the rarely taken branch be checked against the
 * reference's EigenSolver outputs (tests/golden/ref_quu.json) without having to provoke it through a whole solve. */
int cilqr_debug_quu_inverse(cilqr_handle* h, int n, const double* Quu, const double* lamb, double* Qinv, int general);
/* Test hook: the kernels' closest-path-sample search (Constraints::find_closest_point, I/Constraints.cpp:24-59: the strict-< first
 * minimum of the squared distance over all samples; csrc/cilqr_device.hpp::closest_sample finds it from two pruning windows and, where
 * the window is wide and the distance provably convex over it, by Newton) on n independent queries (host buffers).  queries[i] =
 * {poly[6], x_local_plan first, last, point x, y}; out[i] = {the search's index, the index a plain scan over ALL samples of the same
 * kernel finds, 1 if the Newton search decided}.  The two indices must be equal for every query. */
int cilqr_debug_closest_sample(cilqr_handle* h, int n, const double* queries, int32_t* out);

/* Test hook: the blur kernel's own covariance → confidence-ellipse step (float eigen-solve following Eigen::EigenSolver
 * <Matrix2f>, M/src/arbitrary_transformation.cu:60-83 + M/include/ARBIT.cuh:82-99) on n covariances {a, b, c} (host buffers);
 * out = {half_major, half_minor, angle} per row.  Checked bit for bit against the reference's Eigen (ref_blur.json). */
int cilqr_debug_blur_ellipse(cilqr_handle* h, int n, const double* abc, double* out);

/* Test hook: the kernels' own elementary functions (the inline routines of csrc/cilqr_device.hpp that every kernel calls, not copies
 * of them) on n rows, one lane per row (host buffers).
 *   CILQR_MATH_EXP          in: n × x                        out: n × exp_full(x): the form that carries the contract at both ends
 *   CILQR_MATH_SINCOS_FAST  in: n × x                        out: n × {sin, cos} by sincos_fast
 *   CILQR_MATH_SINCOS_LOOP  in: n × x                        out: n × {sin, cos} by sincos_loop
 *   CILQR_MATH_ROTATE       in: n × {theta0, delta_1..T}     out: n × T × {sin, cos}: sincos_loop(theta0), then one rotate_heading
 *                                                            (delta_t) per step on the forward pass's constants (make_fwd_const
 *                                                            on the handle's parameters)
 *   CILQR_MATH_EXP_FAST     in: n × x                        out: n × exp_fast(x): the form for arguments bounded below (the same bits
 *                                                            from -746 up; far below, whatever its arithmetic gives)
 * T (1 ≤ T ≤ CILQR_MAX_HORIZON) is read for CILQR_MATH_ROTATE only.  The routines are called as they stand: sincos_loop and
 * rotate_heading beyond the ranges their callers keep them to (MAX_HEADING0, MAX_TURN) return what the arithmetic gives. */
enum { CILQR_MATH_EXP = 0, CILQR_MATH_SINCOS_FAST = 1, CILQR_MATH_SINCOS_LOOP = 2, CILQR_MATH_ROTATE = 3, CILQR_MATH_EXP_FAST = 4 };
int cilqr_debug_math(cilqr_handle* h, int op, int n, int T, const double* in, double* out);

/* Blocks until everything the host-pointer entry points enqueued on the handle's own stream has finished. */
int cilqr_wait(cilqr_handle* h);

/* --- costmap warp ----------------------------------------------------------------------------- */
/* Rigid global→vehicle-frame warp (M/src/local_costmap.cpp:242-264): for every destination cell, centre C
 * → g = Rot(theta)·C + (vx, vy) → nearest source cell (GridMap::atPosition, G/grid_map_core/src/GridMap.cpp:160-166);
 * if bbox != NULL and bbox(cell) > 90 the destination takes the bbox value (:260-263).  Where the reference
 * would throw std::out_of_range the destination is set to NaN and counted in *n_out_of_range (may be NULL).
 * src: src_geom.rows×cols float32 column-major; dst/bbox: dst_geom.rows×cols float32 column-major.
 * src_geom (global_geom of the frame calls) must carry len == (double)size * res, see cilqr_map_geom: otherwise CILQR_ERR_ARG from
 * every warp and frame entry point below, with nothing enqueued and no output written. */
int cilqr_warp_costmap(cilqr_handle* h, const float* src, const cilqr_map_geom* src_geom,
                       float* dst, const cilqr_map_geom* dst_geom,
                       double vx, double vy, double vtheta, const float* bbox, int64_t* n_out_of_range);
/* Device-pointer form; n_out_of_range_dev is a device int64 counter (zeroed by the call) or NULL. */
int cilqr_warp_costmap_device(cilqr_handle* h, void* stream, const float* src, const cilqr_map_geom* src_geom,
                              float* dst, const cilqr_map_geom* dst_geom,
                              double vx, double vy, double vtheta, const float* bbox,
                              int64_t* n_out_of_range_dev);
/* K frames in one launch: the same source map warped for K poses (a backlog of odometry ticks, the node's pose-noise candidates,
 * I/ilqr_uncertainty_node.cpp:82-110) into K destination layers stored back to back (frame k at dst + k*rows*cols).
 * poses: HOST array [K][3] = (vx, vy, vtheta), read before the call returns; bbox (device, one layer shared by the frames) and
 * n_out_of_range_dev (device, K int64 counters, zeroed by the call) may be NULL.  1 <= K <= 1024.  Every frame equals what
 * cilqr_warp_costmap_device gives for its pose, bit for bit. */
int cilqr_warp_costmap_batch_device(cilqr_handle* h, void* stream, const float* src, const cilqr_map_geom* src_geom, float* dst,
                                    const cilqr_map_geom* dst_geom, int K, const double* poses, const float* bbox,
                                    int64_t* n_out_of_range_dev);
/* --- pose-uncertainty propagation over the vehicle-frame costmap ("blur") ---------- */
/* thrust_propagateUncertainty (M/src/arbitrary_transformation.cu:8-157, functors M/include/ARBIT.cuh:51-107) together with
 * the copy-through of LocalCostmap::propagateUncertainty (M/src/local_costmap.cpp:483-496): for every cell with linear
 * (column-major) index ≥ index, the pose-uncertainty covariance at the cell → 95 % confidence ellipse → Gaussian-weighted
 * average of the `src` layer over the cells inside it; an empty ellipse copies the cell through; cells before `index` are
 * NaN.  src/out: float32 column-major layers of geometry g.  count_out (optional): cells inside each ellipse.
 * vtheta: vehicle heading (the reference passes its sine and cosine). */
int cilqr_blur_costmap(cilqr_handle* h, const float* src, const cilqr_map_geom* g, int index, double vtheta, double sigma_x,
                       double sigma_y, double sigma_theta, float* out, int32_t* count_out);
int cilqr_blur_costmap_device(cilqr_handle* h, void* stream, const float* src, const cilqr_map_geom* g, int index, double vtheta,
                              double sigma_x, double sigma_y, double sigma_theta, float* out, int32_t* count_out);
/* K blurs in one launch.  Frame k = cilqr_blur_costmap_device(src + k*src_stride, g, index, vthetas[k], sigmas) written to
 * out + k*rows*cols (count_out likewise, may be NULL), bit for bit.  src_stride in floats: 0 = one layer under K headings, else
 * >= rows*cols.  vthetas: HOST [K], read before the call returns.  1 <= K <= 1024.  A null handle or pointer, K outside that
 * range, a bad geometry, index < 0 or a src_stride that is negative or between 1 and rows*cols - 1: CILQR_ERR_ARG, checked before
 * the handle or the device is touched.  K = 1 is the single-frame call. */
int cilqr_blur_costmap_batch_device(cilqr_handle* h, void* stream, const float* src, int64_t src_stride, const cilqr_map_geom* g,
                                    int index, int K, const double* vthetas, double sigma_x, double sigma_y, double sigma_theta,
                                    float* out, int32_t* count_out);

/* --- wire formats either side of the costmap path --------------------------------- */
/* GridMapRosConverter::fromOccupancyGrid's data loop (G/grid_map_ros/src/GridMapRosConverter.cpp:259-266, called at
 * M/src/local_costmap.cpp:169): layer[i] = occ[n-1-i] == -1 ? NaN : (float)occ[n-1-i], i = column-major linear index.
 * n_cells = width*height; the geometry side of the conversion is cilqr_map_geom_set(width*res, height*res, res,
 * origin + length/2). */
int cilqr_occupancy_to_layer(cilqr_handle* h, const int8_t* occ, int64_t n_cells, float* layer);
int cilqr_occupancy_to_layer_device(cilqr_handle* h, void* stream, const int8_t* occ, int64_t n_cells, float* layer);
/* GridMapRosConverter::toOccupancyGrid's data loop (:293-306, called at M/src/local_costmap.cpp:298 with range 0..100) for
 * a layer whose circular-buffer start index is zero: v = (layer[i]-data_min)/(data_max-data_min) in float; NaN → -1, else
 * the truncation of clamp(v,0,1)*100; stored at occ[n-1-i]. */
int cilqr_layer_to_occupancy(cilqr_handle* h, const float* layer, int64_t n_cells, float data_min, float data_max, int8_t* occ);
int cilqr_layer_to_occupancy_device(cilqr_handle* h, void* stream, const float* layer, int64_t n_cells, float data_min,
                                    float data_max, int8_t* occ);

/* One frame of the map node's odometry callback (M/src/local_costmap.cpp:172-305) on the device, asynchronous on `stream`:
 * warp of the global layer into the vehicle frame with the optional bounding-box override (cilqr_warp_costmap_device) →
 * pose-uncertainty blur (cilqr_blur_costmap_device, index 0) → the blurred layer as an OccupancyGrid with range 0..100
 * written by the blur kernel itself.  vehicle_layer and uncertainty_layer (device, rows*cols floats each) receive the two
 * float layers; occupancy_out (device, rows*cols int8) may be NULL. */
int cilqr_costmap_frame_device(cilqr_handle* h, void* stream, const float* global_layer, const cilqr_map_geom* global_geom,
                               const cilqr_map_geom* vehicle_geom, double vx, double vy, double vtheta, const float* bbox,
                               double sigma_x, double sigma_y, double sigma_theta, float* vehicle_layer,
                               float* uncertainty_layer, int8_t* occupancy_out, int64_t* n_out_of_range_dev);
/* K odometry-callback frames in two launches (one warp, one blur with the OccupancyGrid), for vehicle maps of any size: the node's
 * pose-noise candidates (I/ilqr_uncertainty_node.cpp:82-113).  Frame k = cilqr_costmap_frame_device for poses[k] = (vx, vy,
 * vtheta), bit for bit in all outputs.  vehicle_layers, uncertainty_layers: [K][rows*cols] floats.  occupancy_out: [K][rows*cols]
 * int8 or NULL.  n_out_of_range_dev: K int64 (zeroed by the call) or NULL.  bbox: one layer shared by the frames, or NULL.
 * poses: HOST [K][3], read before the call returns.  1 <= K <= 1024; arguments are checked as cilqr_blur_costmap_batch_device's,
 * before the handle or the device is touched; K = 1 is the single-frame call.  uncertainty_layers is what
 * cilqr_set_uncertainty_map_device takes with layer_stride = rows*cols and poses = the same K poses on the device. */
int cilqr_costmap_frame_batch_device(cilqr_handle* h, void* stream, const float* global_layer, const cilqr_map_geom* global_geom,
                                     const cilqr_map_geom* vehicle_geom, int K, const double* poses, const float* bbox,
                                     double sigma_x, double sigma_y, double sigma_theta, float* vehicle_layers,
                                     float* uncertainty_layers, int8_t* occupancy_out, int64_t* n_out_of_range_dev);

/* --- obstacle bounding boxes (LocalCostmap::bondingBoxHandle, M/src/local_costmap.cpp:860-922) ------------------------- */
/* The corner arithmetic of bondingBoxHandle (:866-913), on the host (host libm, no fused multiply-add), expression for
 * expression: a box is kept iff sqrt(dx^2 + dy^2) <= max_distance from (own_x, own_y) (:870-875; reference 100.0); its sizes
 * grow by `inflate` (:880-881; reference 0.2) and are halved (:885-886); the corners (+,+) (+,-) (-,-) (-,+) (:889-893) are turned
 * by the box's yaw and moved to its position (:899-900), then taken into the vehicle frame (own_x, own_y, own_yaw) (:903-904).
 * boxes: [n][5] = (x, y, yaw, size_x, size_y) in the planning frame — the caller applies the message's sign flips (posY =
 * -pose.position.y, yaw = -pose.orientation.z, :867,:882).  vertices: [n][4][2] out, the kept boxes packed in order, WITHOUT
 * the repeated closing vertex the reference adds (:913; it changes no cell).  *n_kept: number of boxes kept.  Needs no device. */
int cilqr_boxes_to_polygons(int n, const double* boxes, double own_x, double own_y, double own_yaw, double inflate,
                            double max_distance, double* vertices, int32_t* n_kept);
/* The PolygonIterator loop of bondingBoxHandle (:916-919, called at :232) for n_polygons polygons of n_vertices vertices each: a cell takes
 * `value` iff Polygon::isInside(cell centre) (G/grid_map_core/src/Polygon.cpp:32-44) holds for at least one polygon — for
 * i = 0..V-1, j = i-1 (mod V) a crossing counts when (y_i > p_y) != (y_j > p_y) && p_x < (x_j - x_i) * (p_y - y_i) / (y_j - y_i) + x_i,
 * inside when the count is odd; fp64 in that order, IEEE division, no contraction, on the centre the warp computes.
 * clear != 0: every other cell becomes NaN (the layer setGeometry has just cleared, :213); clear == 0: every other
 * cell is left untouched, so calls accumulate.  vertices: HOST [n_polygons][n_vertices][2] in the layer's frame, read before the
 * call returns; a repeated closing vertex is allowed and changes nothing.  0 <= n_polygons <= CILQR_MAX_POLYGONS,
 * 3 <= n_vertices <= CILQR_MAX_POLYGON_VERTICES, every vertex finite — otherwise CILQR_ERR_ARG (checked before the handle is
 * touched).  layer: g.rows*g.cols float32 column-major.
 * One difference from the iterator is possible in principle and was not seen in 40 359 cells compared against it: the iterator
 * walks the submap of the polygon's vertex bounding box, so a centre inside the polygon but within rounding of that box's edge
 * could fall outside the submap and stay unmarked there; here it is marked. */
int cilqr_rasterize_polygons_device(cilqr_handle* h, void* stream, const cilqr_map_geom* g, int n_polygons, int n_vertices,
                                    const double* vertices, float value, int clear, float* layer);
int cilqr_rasterize_polygons(cilqr_handle* h, const cilqr_map_geom* g, int n_polygons, int n_vertices, const double* vertices,
                             float value, int clear, float* layer);
/* cilqr_warp_costmap_device with bbox = cilqr_rasterize_polygons_device(dst_geom, ..., value 100, clear 1), bit for bit and
 * including the out-of-range counter (counted before the override) — but no bbox layer is written or read: the
 * warp kernel tests the polygons itself.  vertices: HOST, read before the call returns. */
int cilqr_warp_costmap_polygons_device(cilqr_handle* h, void* stream, const float* src, const cilqr_map_geom* src_geom, float* dst,
                                       const cilqr_map_geom* dst_geom, double vx, double vy, double vtheta, int n_polygons,
                                       int n_vertices, const double* vertices, int64_t* n_out_of_range_dev);
/* cilqr_costmap_frame_device with the polygons in place of the bbox layer (the warp above, then blur and OccupancyGrid): the
 * whole of odomCallback from the odometry message and the tracked vehicles to the published grid. */
int cilqr_costmap_frame_polygons_device(cilqr_handle* h, void* stream, const float* global_layer, const cilqr_map_geom* global_geom,
                                        const cilqr_map_geom* vehicle_geom, double vx, double vy, double vtheta, int n_polygons,
                                        int n_vertices, const double* vertices, double sigma_x, double sigma_y, double sigma_theta,
                                        float* vehicle_layer, float* uncertainty_layer, int8_t* occupancy_out,
                                        int64_t* n_out_of_range_dev);

/* --- exact footprint check: the vehicle's rectangle against obstacle rectangles and map cells (new) -------------------------------
 * Every other judge of a plan (cilqr_score_batch, the rollout and chance risks, both tightenings) decides "collision" with the
 * solver's surrogates: against obstacles c = 1 - d'Pd > 0, an ego circle CENTRE inside an ellipse of semi-axes dim/2 + ego_rad (+ 1
 * along); against the map the probes_l x probes_w probes on safe_length x safe_width.  cilqr_footprint_check(_device) answers
 * whether the vehicle's RECTANGLE touches anything — the separating-axis test of the reference's isCollision (I/Experiment.cpp) and,
 * where separated, the exact distance; against the map Polygon::isInside of every cell centre.  Geometry only: no speed inflation,
 * no s_safe, no weights (obs->weight is not read).
 * X [B*S][4*(N+1)]: rows.  Row r belongs to solve b = r / S and reads the obstacles, the layer and the map pose of solve b, indexed as
 * the solve and score kernels index them.  S = 1: a solved batch; S > 1: stored rollouts (X_roll of cilqr_rollout_batch).  obs by
 * strides as everywhere, NULL only when M == 0.  Steps t = 0 ... N-1 are paired with obstacle column t (the score call's
 * convention); x_N is not visited.
 *
 * Definitions.
 *   ego rectangle       centred on the state's (x, y), turned by its theta (X_t[3]); half-extents hl = length/2 + margin and
 *                       hw = width/2 + margin from cilqr_params.  (The ego circles lie symmetric about (x, y): it is the body's centre.)
 *   obstacle rectangle  centre (pose x, y), heading pose theta (pose[3]), half-extents dim/2.  The pose's speed is not read.
 *   clearance of an entry   over the four axes u (two of each rectangle, a = (cos, sin), b = (-sin, cos)):
 *                       gap_u = |u . (centre_O - centre_E)| - (r_E(u) + r_O(u)),  r_R(u) = hl_R |u . a_R| + hw_R |u . b_R|,  g = max_u gap_u.
 *                       g > 0: separated, and the clearance is the least of the eight vertex-to-rectangle distances
 *                       hypot(max(|a| - hl, 0), max(|b| - hw, 0)), each vertex in the other rectangle's body frame (exact for
 *                       disjoint convex polygons).  Otherwise the clearance is g <= 0: minus the least overlap, 0 when touching.
 *   HIT                 clearance <= 0 (isCollision's max1 < min2 is strict: touching collides).  An entry whose pose x, y, theta
 *                       or dimension is not finite, or whose dimension is negative, is a hit with no clearance value.
 *   map test            runs when a map is set on the handle and CILQR_FOOTPRINT_SKIP_MAP is not given.  The four ego corners in
 *                       bondingBoxHandle's order (hl, hw), (hl, -hw), (-hl, -hw), (-hl, hw) go into the map frame by the probes'
 *                       rigid transform (cilqr_rollout_risk_map).  Cell (i, j) of the VIRTUAL grid — centre (x_first - i*res,
 *                       y_first - j*res) for every integer i, j, in the map or not — is covered when Polygon::isInside(centre)
 *                       holds for that 4-gon, by the statements of cilqr_rasterize_polygons: the covered cells inside the map are
 *                       the cells that call marks for those vertices.  A covered cell is UNKNOWN when it is outside the map or
 *                       NaN.  A step HITS the map when a covered in-map cell is > occ_threshold (strict) or, under
 *                       CILQR_FOOTPRINT_UNKNOWN_HITS, when a covered cell is unknown.
 *   lost step           a state whose x, y or theta is not finite: an obstacle hit (whatever M is) and, where the map test runs, a
 *                       map hit and unknown; it covers no cell and adds no clearance value.  For the map test alone, so is a state
 *                       whose footprint's virtual index range (one cell wider than the corners' extremes) leaves +-2^30.
 * fp [B*S][CILQR_FOOTPRINT_FIELDS] (required): see the enum; doubles that hold a value's bits, a count or an index.
 * step_clearance [B*S][N] (double): the min over m at step t; +HUGE_VAL when no entry has a value (M == 0), -HUGE_VAL at a lost step.
 * step_occ [B*S][N] (float): the step's largest finite occupancy under the footprint, NaN when none (or no map test).  total [B*S]:
 * total[r] = base[r] when base[r] is finite, FP_HIT_STEPS == 0, FP_CLEARANCE >= min_clearance and FP_MAP_HIT_STEPS == 0; otherwise
 * NaN — the convention of cilqr_rollout_risk_map, so the call composes through base and feeds cilqr_argmin_device.  Each of the
 * three may be NULL; total without base is CILQR_ERR_ARG.  With M == 0 and no map the call succeeds and returns the empty values.
 *   Determinism: minima and maxima are lexicographic (value, then lowest index) and everything else is an integer count, so nothing
 *   depends on an order of evaluation: a row's bits depend on that row's inputs alone, whatever B, S, its place in the batch and
 *   the obstacles' strides are.  (A per-solve map pose's cosine and sine are formed on the device, the shared pose's on the host:
 *   equal poses given the two ways may differ in the last bit, as for every call that reads the map.)
 * Mapping: one workgroup per row over the M*N entries; wavefront = (row, step), four steps per workgroup, over the cells of the
 * footprint's bounding box; one wavefront per row for the fold.  Three launches (two without a map test), no global atomics.  The
 * virtual index range is formed in doubles and compared with +-2^30 before any conversion; every load of the layer is guarded by the
 * in-map test of its own cell.  Nothing is allocated per call: the per-step records live in device memory reserved at cilqr_create
 * (7*max_batch*max_horizon + 2*max_batch doubles) — two footprint checks on DIFFERENT streams of one handle must not overlap.
 * CILQR_ERR_ARG, decided before the handle is looked at: NULL X or fp; obs (or its pose or dim) NULL with M > 0; total without
 * base; S < 1; a negative stride; margin negative or not finite; a NaN min_clearance or occ_threshold; unknown flag bits.  Then the
 * cilqr_create limits: B*S <= max_batch, N, M; M*N and the map's cells below 2^31.  CILQR_ERR_UNSUPPORTED where a map test would run
 * and ceil(2*hypot(hl, hw)/res) + 2 > 1024: a footprint of more than about a million cells per step.  The host-buffer form's arrays —
 * X, the obstacles' span (6 doubles per entry), base and the outputs — must fit the arena reserved at create: B*S*(6*N + 18) + 6*span
 * doubles with every output, against max_batch*(28*max_horizon + 6*max_obstacles*max_horizon + 50) at least; every B*S <= max_batch fits. */
#define CILQR_FOOTPRINT_FIELDS 12
typedef enum cilqr_footprint_field {
  CILQR_FP_CLEARANCE = 0,          /* min signed clearance over (m, t); +HUGE_VAL when no entry has a value */
  CILQR_FP_CLEARANCE_ENTRY = 1,    /* m*N + t of it, lowest on equal values; -1 */
  CILQR_FP_HIT_STEPS = 2,          /* steps with an obstacle hit */
  CILQR_FP_FIRST_HIT = 3,          /* lowest such t; -1 */
  CILQR_FP_MAP_OCC = 4,            /* largest finite occupancy under the footprint; -HUGE_VAL when none */
  CILQR_FP_MAP_OCC_STEP = 5,       /* its step, lowest on equal; -1 */
  CILQR_FP_MAP_OCC_CELL = 6,       /* i + j*rows of it within that step, lowest on equal; -1 */
  CILQR_FP_MAP_HIT_STEPS = 7,      /* steps that hit the map */
  CILQR_FP_MAP_FIRST_HIT = 8,      /* lowest such t; -1 */
  CILQR_FP_MAP_HIT_CELLS = 9,      /* largest per-step count of covered cells above the threshold */
  CILQR_FP_MAP_UNKNOWN_STEPS = 10, /* steps with an unknown covered cell */
  CILQR_FP_MAP_CELLS = 11          /* covered cells over all steps, in the map or not */
} cilqr_footprint_field;
#define CILQR_FOOTPRINT_UNKNOWN_HITS 1u /* flags: a covered cell that is unknown counts as a map hit */
#define CILQR_FOOTPRINT_SKIP_MAP 2u     /* flags: no map test, whatever is set on the handle */
int cilqr_footprint_check_device(cilqr_handle* h, void* stream, int B, int N, int M, int S, const double* X, const cilqr_obstacles* obs,
                                 double margin, double min_clearance, double occ_threshold, uint32_t flags, const double* base,
                                 double* fp, double* step_clearance, float* step_occ, double* total);
int cilqr_footprint_check(cilqr_handle* h, int B, int N, int M, int S, const double* X, const cilqr_obstacles* obs, double margin,
                          double min_clearance, double occ_threshold, uint32_t flags, const double* base, double* fp,
                          double* step_clearance, float* step_occ, double* total);

/* --- distance to the occupied cells of a layer: exact distance field and inflation (new) -------------------------------------------
 * Every other map product raises cells (cilqr_tighten_map, cilqr_rasterize_tracks) or tests overlap (cilqr_footprint_check); these
 * two say how FAR the nearest occupied cell is — the quantity of grid_map_sdf and of costmap_2d's inflation layer.
 * Layers are float32, column-major (i + j*rows), geometry g (only rows, cols and res are read); layer l starts at layer +
 * l*layer_stride, layer_stride 0 (one shared layer, its result written L times) or >= rows*cols.  Outputs are dense, rows*cols apart.
 *
 * Definitions.
 *   seed      a cell whose value is finite and > occ_threshold (strict, as in cilqr_footprint_check).  Under
 *             CILQR_MAP_DISTANCE_UNKNOWN_SEEDS a NaN cell is a seed too.  Under CILQR_MAP_DISTANCE_TO_FREE the predicate — the
 *             unknown-seeds rule included — is complemented: the result is the distance to the nearest cell that is NOT a seed, and
 *             two calls give the signed field of grid_map_sdf.
 *   d2_out    [L][rows*cols] int32 (required): min over the seeds (i', j') of layer l of (i - i')^2 + (j - j')^2, in cells, an exact
 *             integer, 0 on a seed; INT32_MAX when the layer has no seed.
 *   dist_out  [L][rows*cols] float, or NULL: (float)(res * sqrt((double)d2)) — one correctly rounded square root, one multiply and
 *             one conversion, so it is bit-defined; +INFINITY when the layer has no seed.
 *   Determinism: everything is an integer minimum, so a layer's bits depend on that layer alone, whatever L and its place are.
 * Mapping: two launches.  Lane = row i walks the columns forward and back carrying the distance to the last seed of its row and
 * writes it into d2_out; then one workgroup per (layer, column) takes the column's rows values, squared, into LDS (4*rows bytes) and
 * lane = i searches outward over min(G[i - d], G[i + d]) + d^2 until d^2 reaches the best so far; the result replaces the column in
 * place.  Both launches are coalesced; no atomics, no scratch memory, nothing allocated per call.
 * CILQR_ERR_ARG, decided before the handle is looked at: NULL layer, g or d2_out; L < 1; rows or cols < 1 or a res that is not
 * positive and finite; a layer_stride that is negative or between 1 and rows*cols - 1; a NaN occ_threshold; unknown flag bits; L
 * beyond 2^31 - 1 workgroups (L * max(cols, ceil(rows*cols/256))).  CILQR_ERR_UNSUPPORTED for rows or cols > 8192 (d2 <= 2*8192^2
 * < 2^31, and a column of int32 is 32 KiB of LDS).  The host-buffer form's arrays — the layers' span, d2_out and dist_out, 4 bytes a
 * cell each — must fit the device arena reserved at create (CILQR_ERR_ARG otherwise, as for every host form; this call adds nothing
 * to it): large maps and batches take the device form. */
#define CILQR_MAP_DISTANCE_UNKNOWN_SEEDS 1u /* flags: NaN cells are seeds */
#define CILQR_MAP_DISTANCE_TO_FREE 2u       /* flags: the seed predicate is complemented */
int cilqr_map_distance_device(cilqr_handle* h, void* stream, int L, const float* layer, int64_t layer_stride, const cilqr_map_geom* g,
                              double occ_threshold, uint32_t flags, int32_t* d2_out, float* dist_out);
int cilqr_map_distance(cilqr_handle* h, int L, const float* layer, int64_t layer_stride, const cilqr_map_geom* g, double occ_threshold,
                       uint32_t flags, int32_t* d2_out, float* dist_out);

/* cilqr_inflate_map(_device): the layers inflated from the field d2 [L][rows*cols] of cilqr_map_distance, for the solve to read.
 * Per cell, with d = res * sqrt((double)d2) evaluated in double, in this order:
 *   v = peak                                          where d <= inscribed;
 *   v = 0                                             where d >= radius or d2 == INT32_MAX;
 *   v = peak * (radius - d) / (radius - inscribed)    otherwise (the product first, then the quotient).
 * A cell o that is not NaN becomes max(o, (float)v).  A NaN cell becomes (float)v where v > 0 and stays NaN elsewhere — the convention
 * of cilqr_rasterize_tracks: unknown stays unknown where nothing reaches it.  layer_out [L][rows*cols] goes where tightened layers go:
 * cilqr_set_uncertainty_map_device with layer_stride = rows*cols (or 0), followed by a solve.  The inflation is soft: judge the final
 * plan against the ORIGINAL map.  layer_out may be the very buffer `layer` when L == 1 or layer_stride == rows*cols; any other
 * overlap of the two ranges is CILQR_ERR_ARG (device form).  One launch, lane = cell; nothing is allocated per call.
 * CILQR_ERR_ARG, decided before the handle is looked at: NULL layer, g, d2 or layer_out; L, geometry and layer_stride as above;
 * inscribed or radius not finite, inscribed < 0 or radius <= inscribed; a peak that is not finite or not > 0.  CILQR_ERR_UNSUPPORTED
 * for rows or cols > 8192.  Host-buffer form: the layers' span, d2 and layer_out must fit the arena, as above. */
int cilqr_inflate_map_device(cilqr_handle* h, void* stream, int L, const float* layer, int64_t layer_stride, const cilqr_map_geom* g,
                             const int32_t* d2, double inscribed, double radius, double peak, float* layer_out);
int cilqr_inflate_map(cilqr_handle* h, int L, const float* layer, int64_t layer_stride, const cilqr_map_geom* g, const int32_t* d2,
                      double inscribed, double radius, double peak, float* layer_out);

/* --- obstacles from the map: connected components of occupied cells as boxes (new) ---------------------------------------------------
 * Every map call above takes boxes, tracks or covariances and raises cells; this one goes the other way.  Where the occupied cells
 * of a layer are the only obstacle information (M = 0), it labels them and returns one rectangle per component in the formats the
 * obstacle channel reads: cilqr_boxes_to_polygons rows and cilqr_obstacles pose / dim tables.
 * L layers per call, column-major (i + j*rows), geometry g as cilqr_map_distance reads it (rows, cols, res) plus its position
 * (pos_x, pos_y, len_x, len_y) for the cell centres.
 *
 * Definitions.
 *   d2          [L][rows*cols] int32 (required): the output of cilqr_map_distance for the layer, so the seed predicate (threshold,
 *               NaN flag, complement) is that call's.  A cell is a SEED where d2 == 0 and LINKED where d2 <= gap2, gap2 >= 0 an
 *               integer in cells^2; INT32_MAX (no seed in the layer) is never linked.  With gap2 = 0 the linked cells are the
 *               seeds; a larger gap2 bridges gaps between returns (the Eps of DBSCAN).
 *   component   a maximal set of linked cells connected through neighbours: 8 neighbours, or 4 under CILQR_MAP_OBSTACLES_FOUR.
 *               Every component holds at least one seed.
 *   label_out   [L][rows*cols] int32 (required): for a linked cell the lowest linear index among the linked cells of its
 *               component, -1 elsewhere.  The value is canonical: it does not depend on any order of evaluation.
 *   comp        [L][K][CILQR_MAP_OBSTACLE_FIELDS] doubles (required), see the enum: every field but FILL holds an exact integer.
 *               CELLS, the index extremes and the index sums run over the SEEDS of the component; LINKED counts its linked cells.
 *   n_out       [L][4] int32 (required): the components found; those with CELLS >= min_cells; the rows written; the seeds.
 *   rows        the components with CELLS >= min_cells, in ascending label order; the first K of them get slots; of these, the ones
 *               whose larger box size exceeds max_size (metres; HUGE_VAL: no limit — walls and buildings stay with the map channel)
 *               are dropped; the rest are compacted in order.  K CAPS THE SLOTS BEFORE THE SIZE FILTER: with more than K components
 *               of min_cells, a small one behind K large ones is not returned, and n_out[l][1] > K says that this happened.
 *   filler      rows at and beyond n_out[l][2], up to K: pose (FAR, FAR, 0, 0) with FAR = CILQR_MAP_OBSTACLES_FAR, dim (0, 0), box
 *               (FAR, FAR, 0, 0, 0), every comp field -1.  A filler row's barrier term underflows to exactly 0, so a solve with a
 *               fixed M = K needs no read-back of the count.
 *   boxes       [L][K][5] = (x, y, yaw, size_x, size_y) in the planning frame, the input of cilqr_boxes_to_polygons; pose_out
 *               [L][K][4] = (x, y, 0, yaw) and dim_out [L][K][2] = (size_x, size_y), read by cilqr_obstacles strides (K, 1, 0) — one
 *               set per layer, constant over the horizon — or (0, 1, 0) with L = 1.  Each of the three may be NULL.
 *   pose        [L or 1][3] = (x, y, theta) with pose_stride 3 or 0, or NULL for the identity: the layer's pose in the planning
 *               frame.  A point m of the map frame goes to w = (pose.x + (c*m.x - s*m.y), pose.y + (s*m.x + c*m.y)) with c, s the
 *               cosine and sine of theta, exactly as cilqr_rasterize_tracks takes a cell centre there.
 *   work        [L][rows*cols] int32 (required): scratch, contents unspecified afterwards.  Nothing is allocated per call.
 *
 * Box of a component, evaluated in double as written, no fused multiply-add.  Over the seeds (i, j) of the component: c = CELLS,
 * Si, Sj, Sii, Sij, Sjj the index sums; a = c*Sii - Si*Si, b = c*Sij - Si*Sj, d = c*Sjj - Sj*Sj in 64-bit integers, exact because
 * rows and cols <= 1024 keeps every term within 2^60.
 *   phi = 0.5*atan2(2*(double)b, (double)a - (double)d);   co = cos phi, so = sin phi;   mi = (double)Si/(double)c, mj likewise;
 *   per seed   p = (i - mi)*co + (j - mj)*so,   q = (j - mj)*co - (i - mi)*so;
 *   h = 0.5*(|co| + |so|) (the half-extent of a unit cell along either axis);  p0 = min p - h, p1 = max p + h, q0, q1 likewise;
 *   centre, in index coordinates   ci = mi + pc*co - qc*so,  cj = mj + pc*so + qc*co  with pc = 0.5*(p0 + p1), qc = 0.5*(q0 + q1);
 *   in the map frame m = (x_first - ci*res, y_first - cj*res), x_first = pos_x + (len_x/2 - res/2) and y_first likewise, then the
 *   planning frame as above;  yaw = phi + theta (both index axes are flipped against the map's: a half turn, which a rectangle
 *   does not see);  size_x = (p1 - p0)*res + 2*pad,  size_y = (q1 - q0)*res + 2*pad;  FILL = c/((p1 - p0)*(q1 - q0)).
 * The box contains the whole square of every seed of its component.  size_x lies along the axis of largest variance; it is not
 * promised to be the larger size.  A principal-axis box is NOT the minimum-area box: an L-shaped wall gets a large box with a low
 * FILL, and the caller can leave such components to the map channel.
 *   Determinism: labels are minima of indices, counts and moments integer sums, extents minima and maxima, rows ordered by label: a
 * layer's bits depend on that layer alone, whatever L and its place in the batch are.
 * Mapping: union-find per 64 x 16 tile in LDS, lane along i; a seam launch that unites across tile borders by atomic minima;
 * flatten and count the seeds at each root; one workgroup per layer ranks the roots by ballot prefix; lane = linked cell adds its
 * moments into its slot by 64-bit integer atomics; one workgroup per slot scans the slot's index window for the extents; one
 * workgroup per layer filters, compacts and writes the filler rows.  Seven launches and one 16*L-byte clear.  Every find and union
 * loop is bounded by rows*cols; should a bound ever run out, every value of n_out[l] is -1 and every row of layer l is filler, and
 * the host-buffer form returns CILQR_ERR_INTERNAL (the device form cannot read n_out without a wait; its caller sees the -1).
 * CILQR_ERR_ARG, decided before the handle is looked at: NULL d2, g, work, label_out, n_out or comp; L < 1; a geometry
 * cilqr_map_distance rejects; gap2 < 0; K outside 1 ... CILQR_MAX_POLYGONS; min_cells < 1; max_size not > 0 (NaN included); pad
 * negative or not finite; a pose_stride other than 0 or 3; unknown flag bits; L*K or L*ceil(rows*cols/256) beyond 2^31 - 1
 * workgroups.  CILQR_ERR_UNSUPPORTED for rows or cols > 1024.  The host-buffer form's arrays — d2, work and label_out, 4 bytes a cell
 * each, and 24 doubles a row with every output — must fit the device arena reserved at create (CILQR_ERR_ARG otherwise, as for every
 * host form; this call adds nothing to it). */
#define CILQR_MAP_OBSTACLE_FIELDS 13
typedef enum cilqr_map_obstacle_field {
  CILQR_MO_LABEL = 0,   /* the component's label: its lowest linked cell, i + j*rows */
  CILQR_MO_CELLS = 1,   /* its seeds */
  CILQR_MO_LINKED = 2,  /* its linked cells */
  CILQR_MO_I_MIN = 3,   /* extremes of i and j over its seeds */
  CILQR_MO_I_MAX = 4,
  CILQR_MO_J_MIN = 5,
  CILQR_MO_J_MAX = 6,
  CILQR_MO_SUM_I = 7,   /* sums of i, j, i*i, i*j, j*j over its seeds */
  CILQR_MO_SUM_J = 8,
  CILQR_MO_SUM_II = 9,
  CILQR_MO_SUM_IJ = 10,
  CILQR_MO_SUM_JJ = 11,
  CILQR_MO_FILL = 12    /* seeds per cell of the box's area, in (0, 1] */
} cilqr_map_obstacle_field;
#define CILQR_MAP_OBSTACLES_FOUR 1u     /* flags: 4-connectivity (default 8) */
#define CILQR_MAP_OBSTACLES_FAR 1.0e6   /* metres: where the filler rows stand */
int cilqr_map_obstacles_device(cilqr_handle* h, void* stream, int L, const int32_t* d2, const cilqr_map_geom* g, int gap2, uint32_t flags,
                               const double* pose, int pose_stride, int K, int min_cells, double max_size, double pad, int32_t* work,
                               int32_t* label_out, int32_t* n_out, double* comp, double* boxes, double* pose_out, double* dim_out);
int cilqr_map_obstacles(cilqr_handle* h, int L, const int32_t* d2, const cilqr_map_geom* g, int gap2, uint32_t flags, const double* pose,
                        int pose_stride, int K, int min_cells, double max_size, double pad, int32_t* work, int32_t* label_out,
                        int32_t* n_out, double* comp, double* boxes, double* pose_out, double* dim_out);

/* --- map obstacles tracked across ticks: association and Kalman update (new) ---------------------------------------------------------
 * cilqr_map_obstacles returns this tick's boxes in label order, without velocity or covariance; cilqr_predict_obstacles wants what a
 * tracker hands over.  cilqr_track_update(_device) is that tracker, one tick per call: predict, gate, associate, update, retire,
 * start new tracks, and write the track / track_dim / track_cov arrays of cilqr_predict_obstacles, slot-ordered, so that an
 * obstacle keeps its index over the ticks and nothing is read back between the map and the solve.
 *
 * Definitions.  W worlds (independent trackers; W = 1 is the node, W is the T of cilqr_predict_obstacles), M slots per world
 * (1 ... CILQR_TRACK_MAX_SLOTS, the M of cilqr_predict_obstacles), D detections per world (0 ... CILQR_TRACK_MAX_DETECTIONS).
 *   det        [W][D][5] = (x, y, yaw, size_x, size_y) in the planning frame: the `boxes` rows of cilqr_map_obstacles.  NULL is
 *              allowed when D = 0.
 *   n_det      int32 count of world w at n_det[w*n_det_stride] (n_det_stride >= 0), clamped to [0, D]; NULL: all D rows count.
 *              With n_det = n_out + 2 and n_det_stride = 4 the call reads the "rows written" of cilqr_map_obstacles where it lies.
 *              A detection below the count whose x or y is not finite is INVALID: it takes part in nothing and is counted.
 *   f          the filter, copied at the call.  dt > 0 is the time between ticks in seconds (not Parameters::timestep).  Q and
 *              P_birth are 4 x 4 for the state order (x, y, vx, vy), R is 2 x 2; all column-major, only row <= column read (the
 *              convention of sigma0); Q is the process noise of one tick of this dt.  gate2 >= 0 bounds the squared Mahalanobis
 *              distance, HUGE_VAL: no gate.  min_hits >= 1, max_misses >= 0, v_min >= 0, theta_var_slow >= 0.
 *   state      [W][M][CILQR_TRACK_STATE] doubles, see the enum; integers are stored as exact doubles.  state_in and state_out
 *              may be the same address (the call then updates in place) and may not overlap otherwise.  A slot whose ID is
 *              not >= 0 is FREE; the call writes a free slot as ID = -1 and every other value 0.  Of P only row <= column is
 *              read; what is written is exactly symmetric.
 *   world      [W][CILQR_TRACK_WORLD_FIELDS] doubles, in and out, exact integers, see the enum: NEXT_ID and TICKS are carried
 *              over the ticks, the others are counts of this tick.
 *   flags      CILQR_TRACK_RESET: every slot is free on entry and NEXT_ID = TICKS = 0; state_in (which may then be NULL) and the
 *              incoming world are not read, so a first tick needs no initialised memory.
 *   assign     [W][D] int32 or NULL: the slot the detection was matched to or born into, -1 when dropped, -2 when invalid or at
 *              or beyond the count.
 *   track_out  [W][M][6], dim_out [W][M][2], cov_out [W][M][16]: required; the track, track_dim and track_cov of
 *              cilqr_predict_obstacles.
 * One tick of one world, evaluated in double as written, no fused multiply-add:
 *   1 predict  every slot live on entry: x += dt*vx, y += dt*vy; P- = F P F' + Q with F = I + dt*{(0,2), (1,3)}, entries with
 *              row <= column computed and mirrored; AGE += 1.
 *   2 gate     S = P-[0:2, 0:2] + R, det = S00*S11 - S01*S01, nu = (det.x - x, det.y - y),
 *              d2 = (S11*nu_x^2 - 2*S01*nu_x*nu_y + S00*nu_y^2) / det.  A pair (slot m, detection d) is ADMISSIBLE when m is live
 *              on entry, d is valid and d2 <= gate2; a NaN d2 fails, and a det that is not > 0 admits nothing.
 *   3 associate  greedy global nearest neighbour: repeatedly the smallest (d2, m, d), compared in that order (-0 equals +0), among
 *              the admissible pairs whose m and d are both unassigned is assigned, until none is left.  This is NOT the optimal
 *              assignment: it can match fewer pairs, or at a larger summed d2, than the Hungarian method would.
 *   4 update   matched slots: K = P- H' S^-1 (H = [I2 0]), (x, y, vx, vy) += K nu; Joseph form
 *              P = (I - K H) P- (I - K H)' + K R K', upper triangle mirrored; SIZE_X, SIZE_Y, YAW become a bit copy of the
 *              detection; HITS += 1, MISSES = 0, DET = d.
 *   5 miss     unmatched live slots: MISSES += 1, DET = -1, the predicted state and P- stay.  A slot with MISSES > max_misses is
 *              freed; a slot freed this tick takes no birth this tick.
 *   6 birth    the unassigned valid detections in ascending d take the slots free on entry in ascending m: state
 *              (det.x, det.y, 0, 0), P = P_birth (mirrored), box copied, ID = NEXT_ID++ in that order, HITS = 1, MISSES = 0, AGE = 0,
 *              DET = d.  Those that find no slot are DROPPED.  Then TICKS += 1.
 *   7 output   row of slot m.  CONFIRMED (live after the tick and HITS >= min_hits): with v = hypot(vx, vy), if v >= v_min the row is
 *              (x, y, v, theta = atan2(vy, vx), 0, 0), its covariance J P J' with J = diag(1, 1) (+) [[vx/v, vy/v],
 *              [-vy/v^2, vx/v^2]] (upper triangle mirrored) and its dimensions (SIZE_X, SIZE_Y) when |cos(theta - YAW)| >=
 *              |sin(theta - YAW)|, else (SIZE_Y, SIZE_X): the box's principal axis knows nothing of the direction of travel.
 *              Otherwise the track is reported as standing: (x, y, 0, YAW, 0, 0), the position block of P bit-copied, speed
 *              variance P(2,2) + P(3,3), heading variance theta_var_slow, every cross term 0, dimensions as stored.  With
 *              v_min = 0 a track at rest (every newborn) divides by v = 0 and its row is not finite: choose v_min > 0.
 *              Every other slot is filler: (FAR, FAR, 0, 0, 0, 0) with FAR = CILQR_MAP_OBSTACLES_FAR, dimensions 0, covariance 0 —
 *              the filler of cilqr_map_obstacles, whose barrier term is exactly 0, so predict and solve run at a fixed M.
 *   The model is constant velocity: a and omega of every row are 0.  A turning or braking vehicle is followed only through Q, its
 *   predicted path is a straight line at its last estimated velocity, and the yaw of its box does not enter the filter.
 *   Determinism: values are not checked beyond what is said above; a NaN stays in its own slot.  A world's outputs depend on that
 *   world's inputs, f, M and D alone: the same bits whatever W is and wherever the world sits.
 * Mapping: one wavefront per world, W workgroups, one launch, nothing allocated per call.  Lane = slot for predict, gate and
 * update; each lane walks the detections in LDS for its best one; the greedy rounds are wavefront-wide minima of (d2, m, d) by DPP
 * and v_readlane, after which only the lanes that lost their detection scan again; births meet their slots through ballot ranks.
 * LDS: the detections, three 64-word lists and one [64][33] staging block through which the state rows are loaded and every output
 * is stored, coalesced.
 * CILQR_ERR_ARG, decided before the handle is looked at where no handle is needed: NULL f, state_out, world, track_out, dim_out or
 * cov_out; NULL state_in without CILQR_TRACK_RESET; NULL det with D > 0; W < 1, M < 1, D < 0, n_det_stride < 0; dt not > 0 or not
 * finite; gate2, v_min or theta_var_slow negative or NaN; min_hits < 1; max_misses < 0; unknown flag bits; then W beyond max_batch
 * or M beyond max_obstacles.  CILQR_ERR_UNSUPPORTED for M above CILQR_TRACK_MAX_SLOTS or D above CILQR_TRACK_MAX_DETECTIONS.
 * The host-buffer form's arrays must fit the device arena reserved at create (CILQR_ERR_ARG otherwise; this call adds nothing to
 * it): W*(56*M + 5.5*D + 9) doubles in place, 32*W*M more with a separate state_out, and the counts.  On a handle with
 * max_horizon >= 15 every W <= max_batch fits, whatever M <= max_obstacles and D are. */
#define CILQR_TRACK_MAX_SLOTS 64
#define CILQR_TRACK_MAX_DETECTIONS 64
#define CILQR_TRACK_STATE 32
typedef enum cilqr_track_state_field {
  CILQR_TS_X = 0,
  CILQR_TS_Y = 1,
  CILQR_TS_VX = 2,
  CILQR_TS_VY = 3,
  CILQR_TS_P = 4,        /* 4 ... 19: the covariance, column-major */
  CILQR_TS_SIZE_X = 20,  /* 20 ... 22: a bit copy of the last matched detection */
  CILQR_TS_SIZE_Y = 21,
  CILQR_TS_YAW = 22,
  CILQR_TS_ID = 23,      /* -1: the slot is free */
  CILQR_TS_HITS = 24,
  CILQR_TS_MISSES = 25,  /* consecutive */
  CILQR_TS_AGE = 26,     /* ticks since birth */
  CILQR_TS_DET = 27      /* the detection matched or born from this tick, -1 for a miss; 28 ... 31 are zero */
} cilqr_track_state_field;
#define CILQR_TRACK_WORLD_FIELDS 9
typedef enum cilqr_track_world_field {
  CILQR_TW_NEXT_ID = 0,
  CILQR_TW_TICKS = 1,
  CILQR_TW_LIVE = 2,       /* live slots after the tick */
  CILQR_TW_CONFIRMED = 3,  /* of these, HITS >= min_hits */
  CILQR_TW_MATCHED = 4,
  CILQR_TW_BORN = 5,
  CILQR_TW_DIED = 6,
  CILQR_TW_DROPPED = 7,    /* unassigned valid detections that found no free slot */
  CILQR_TW_INVALID = 8
} cilqr_track_world_field;
#define CILQR_TRACK_RESET 1u /* flags: every slot is free on entry, NEXT_ID = TICKS = 0 */
typedef struct cilqr_track_filter {
  double dt;
  double Q[16];
  double R[4];
  double P_birth[16];
  double gate2;
  double v_min;
  double theta_var_slow;
  int32_t min_hits;
  int32_t max_misses;
} cilqr_track_filter;
int cilqr_track_update_device(cilqr_handle* h, void* stream, int W, int M, int D, const double* det, const int32_t* n_det,
                              int64_t n_det_stride, const cilqr_track_filter* f, const double* state_in, double* state_out,
                              double* world, uint32_t flags, int32_t* assign, double* track_out, double* dim_out, double* cov_out);
int cilqr_track_update(cilqr_handle* h, int W, int M, int D, const double* det, const int32_t* n_det, int64_t n_det_stride,
                       const cilqr_track_filter* f, const double* state_in, double* state_out, double* world, uint32_t flags,
                       int32_t* assign, double* track_out, double* dim_out, double* cov_out);

/* --- static layer: the cells of tracked movers taken out of the map (new) --------------------------------------------------------------
 * A vehicle that cilqr_track_update has confirmed as moving is still in the layer the map calls read: a blob of occupied cells that
 * stands where it is NOW for the whole horizon, while its track predicts it somewhere else (the complaint of the
 * cilqr_rasterize_tracks section above).  cilqr_clear_movers(_device) separates static from dynamic occupancy: the cells that
 * belong to the components of moving tracks, and a halo around them, are set to `fill`; everything else is a bit copy.  Its inputs
 * are what the calls in front left in device memory; nothing is read back.
 * L layers per call, float32, column-major (i + j*rows); layer and layer_stride as cilqr_inflate_map takes them; of g only rows and
 * cols are read (res only has to pass that call's geometry check).
 *
 * Definitions.
 *   label       [L][rows*cols] int32 (required): the label_out of cilqr_map_obstacles.  A cell with a value >= 0 is LINKED.
 *   comp        [L][K][CILQR_MAP_OBSTACLE_FIELDS] (required), K in 1 ... CILQR_MAX_POLYGONS: only CILQR_MO_LABEL is read; a filler
 *               row has -1.
 *   movers      given in exactly ONE of two forms (both or neither, or half of the first: CILQR_ERR_ARG).
 *     tracker   assign [L][K] int32 and state [L][M][CILQR_TRACK_STATE]: those of cilqr_track_update run with W = L and D = K, after
 *               the tick; M in 1 ... CILQR_TRACK_MAX_SLOTS, min_hits >= 1, v_clear >= 0 (m/s).  Row k of layer l is a MOVER when its
 *               comp label is >= 0, m = assign[l][k] lies in [0, M), state[l][m][ID] >= 0, state[l][m][DET] == k,
 *               state[l][m][HITS] >= min_hits and hypot(VX, VY) >= v_clear, evaluated in double; a NaN fails.
 *     mask      mask [L][K] int32, for a caller with a tracker of their own: row k is a MOVER when mask[l][k] != 0 and its comp
 *               label is >= 0.  M, min_hits and v_clear are not read.
 *   halo2       an integer in cells^2, 0 <= halo2 <= CILQR_CLEAR_MOVERS_MAX_HALO2; r = the largest integer with r*r <= halo2 (<= 32).
 *   fill        a float, finite or NaN.
 *   ownership   per cell c = (i, j): over the linked cells q = (i', j') of the layer with |i - i'| <= r and |j - j'| <= r take the
 *               lexicographic minimum of ((i - i')^2 + (j - j')^2, label[q]).  If there is one and its squared distance is <= halo2,
 *               the component with that label OWNS c; otherwise nobody does.  A linked cell owns itself.  EVERY linked cell
 *               competes, whether or not its component got a row: a wall that max_size or K dropped keeps its own halo, and a cell
 *               nearer to it than to a mover is not cleared.  Equal distance goes to the lower label.
 *   layer_out   [L][rows*cols] float32 (required), dense.  A cell owned by a MOVER's component whose input is not NaN becomes `fill`;
 *               every other cell is a bit copy of the input: unknown stays unknown.  layer_out may be the very buffer `layer` under
 *               the rule of cilqr_inflate_map (L == 1 or layer_stride == rows*cols); any other overlap of the two is CILQR_ERR_ARG
 *               (device form).
 *   owner_out   [L][rows*cols] int32 or NULL: the owning label, -1 where nobody owns the cell.
 *   fields      [L][CILQR_CLEAR_MOVERS_FIELDS] doubles (required), see the enum: exact integers, and one largest value.  A -0 input
 *               counts as 0 for CM_MAX_VALUE and is reported as 0.
 *   Determinism: integer sums and a lexicographic maximum: a layer's bits depend on that layer alone, whatever L, its place in the
 *   batch, or layer_stride 0 against dense layers.
 * What it is NOT.  A mover whose component merged with a wall gets a different box; the tracker will most likely not match it and
 * it is not cleared — the conservative failure.  Blur that reaches beyond halo2 stays in the layer.  A cleared vehicle is GONE from
 * the map: it must come back through the tracks (cilqr_rasterize_tracks, cilqr_chance_risk_cov, cilqr_footprint_check on the
 * predicted table of cilqr_predict_obstacles), and the caller must keep those behind this call.
 * Mapping: one 64*L-byte clear of `fields` and two launches, nothing allocated per call, no float atomics.  One workgroup per
 * 64 x 16 tile, lane along i: a prologue, lane = row, decides the movers and sorts their labels into LDS; the tile's labels and an
 * apron of r cells go to LDS; one pass along i leaves (|di|, label) per column, one pass along j the owner — the rule is separable:
 * within a column the distance grows with |di|; each workgroup adds its counts into the layer's row by 64-bit integer atomics (sums
 * and one maximum), and a second launch, lane = layer, turns the row into doubles.
 * CILQR_ERR_ARG, decided before the handle is looked at: NULL layer, g, label, comp, layer_out or fields; L < 1, or a geometry or
 * layer_stride cilqr_inflate_map rejects; K outside 1 ... CILQR_MAX_POLYGONS; not exactly one mover form; in the tracker form M
 * outside 1 ... CILQR_TRACK_MAX_SLOTS, min_hits < 1, or v_clear negative or NaN; halo2 out of range; an infinite fill; a forbidden
 * overlap; L*ceil(rows/64)*ceil(cols/16) beyond 2^31 - 1 workgroups.  CILQR_ERR_UNSUPPORTED for rows or cols > 1024, the bound of
 * cilqr_map_obstacles.  The host-buffer form's arrays — the layers' span, label, layer_out and owner_out at 4 bytes a cell, 13
 * doubles a row, and the mover form's — must fit the device arena reserved at create (CILQR_ERR_ARG otherwise, as for every host
 * form; this call adds nothing to it). */
#define CILQR_CLEAR_MOVERS_MAX_HALO2 1024
#define CILQR_CLEAR_MOVERS_FIELDS 8
typedef enum cilqr_clear_movers_field {
  CILQR_CM_MOVERS = 0,        /* rows that are movers */
  CILQR_CM_CLEARED = 1,       /* cells whose output bits differ from the input */
  CILQR_CM_OWNED_LINKED = 2,  /* linked cells owned by movers */
  CILQR_CM_OWNED_HALO = 3,    /* cells that are not linked and owned by movers */
  CILQR_CM_MAX_VALUE = 4,     /* the largest finite input among the mover-owned cells, -1 when there is none */
  CILQR_CM_MAX_CELL = 5,      /* the lowest cell i + j*rows that has it, -1 when there is none */
  CILQR_CM_CONTESTED = 6,     /* cells, not linked, within halo2 of a mover's linked cell that a non-mover owns: kept */
  CILQR_CM_KEPT_UNKNOWN = 7   /* NaN cells a mover owns: kept */
} cilqr_clear_movers_field;
int cilqr_clear_movers_device(cilqr_handle* h, void* stream, int L, const float* layer, int64_t layer_stride, const cilqr_map_geom* g,
                              const int32_t* label, int K, const double* comp, int M, const int32_t* assign, const double* state,
                              int min_hits, double v_clear, const int32_t* mask, int halo2, float fill, float* layer_out,
                              int32_t* owner_out, double* fields);
int cilqr_clear_movers(cilqr_handle* h, int L, const float* layer, int64_t layer_stride, const cilqr_map_geom* g, const int32_t* label,
                       int K, const double* comp, int M, const int32_t* assign, const double* state, int min_hits, double v_clear,
                       const int32_t* mask, int halo2, float fill, float* layer_out, int32_t* owner_out, double* fields);

/* --- exact clearance of the ego rectangle to the occupied cells of the map (new) -----------------------------------------------------
 * The map counterpart of CILQR_FP_CLEARANCE: cilqr_footprint_check reports only whether the rectangle covers a cell above the
 * threshold; this call returns how far the nearest such cell is, so that min_clearance has something to act on where the map is
 * the only obstacle information (M = 0).  Rows, steps t = 0 ... N-1, the map set on the handle, the rigid transform into the map
 * frame, the layer and pose of solve b = r / S and the half-extents hl = length/2 + margin, hw = width/2 + margin are exactly those of
 * cilqr_footprint_check.
 *
 * Definitions.
 *   seed          an in-map cell whose value is finite and > occ_threshold (strict); under CILQR_MAP_CLEARANCE_UNKNOWN_SEEDS an
 *                 in-map NaN cell too.  Cells outside the map are never seeds.
 *   s of a seed   with (a, b) the body-frame coordinates of the cell's centre (x_first - i*res, y_first - j*res): where |a| > hl or
 *                 |b| > hw, s = hypot(max(|a| - hl, 0), max(|b| - hw, 0)); otherwise s = -min(hl - |a|, hw - |b|): minus the
 *                 penetration depth, 0 on the boundary — the obstacle clearance's "minus the least overlap".  This inside test,
 *                 |a| <= hl && |b| <= hw, is this call's own: for a centre within rounding of the boundary it may differ from
 *                 Polygon::isInside, so CILQR_MC_TOUCH_STEPS is not promised to equal CILQR_FP_MAP_HIT_STEPS there.
 *   step          its clearance is the minimum of s over the seeds with s <= reach, lexicographic: the value first, then the lowest
 *                 i + j*rows; +HUGE_VAL when there is none.  Seeds with s > reach never count, so the answer does not depend on
 *                 the shape of the search WINDOW: the range of virtual cell indices, one cell wider on every side than the
 *                 extremes of the four corners of the rectangle grown by reach (half-extents hl + reach, hw + reach), formed as
 *                 cilqr_footprint_check forms its range.  A step whose window leaves [0, rows) x [0, cols) is counted.
 *   lost step     a state whose x, y or theta is not finite, or whose window leaves +-2^30: clearance -HUGE_VAL, no cell; it is
 *                 below every min_clearance and counts among the steps <= 0.
 * mc [B*S][CILQR_MAP_CLEARANCE_FIELDS] (required): see the enum; doubles that hold a value's bits, a count or an index.
 * step_clearance [B*S][N] or NULL.  total [B*S] or NULL: total[r] = base[r] when base[r] is finite, there is no lost step and
 * MC_CLEARANCE >= min_clearance; otherwise NaN — the base convention, so the call composes (behind cilqr_footprint_check, say) and
 * feeds cilqr_argmin_device.  total without base is CILQR_ERR_ARG.
 *   Determinism: lexicographic minima and integer counts; a row's bits depend on that row's inputs alone.
 * Mapping: wavefront = (row, step), four steps per workgroup, lanes over the cells of the window clipped to the map, every load of
 * the layer guarded by the in-map test of its own cell; then one wavefront per row for the fold.  Two launches, no global atomics.
 * Nothing is allocated per call: the per-step records live in the region reserved at cilqr_create for cilqr_footprint_check — this
 * call and a footprint check, or two of these, on DIFFERENT streams of one handle must not overlap.
 * CILQR_ERR_ARG, decided before the handle is looked at: NULL X or mc; total without base; S < 1; margin or reach negative or not
 * finite; a NaN min_clearance or occ_threshold; unknown flag bits.  Then the cilqr_create limits (B*S <= max_batch, N), no map set on
 * the handle, a map of 2^31 cells or more.  CILQR_ERR_UNSUPPORTED where ceil(2*(hypot(hl, hw) + reach)/res) + 2 > 1024.  The host-buffer
 * form's arrays — B*S*(5*N + 14) doubles with every output — fit the arena reserved at create for every B*S <= max_batch. */
#define CILQR_MAP_CLEARANCE_FIELDS 8
typedef enum cilqr_map_clearance_field {
  CILQR_MC_CLEARANCE = 0,     /* min clearance over t; +HUGE_VAL when no step has a seed within reach; -HUGE_VAL with a lost step */
  CILQR_MC_STEP = 1,          /* its step, lowest on equal values; -1 */
  CILQR_MC_CELL = 2,          /* i + j*rows of it within that step, lowest on equal values; -1 */
  CILQR_MC_BELOW_STEPS = 3,   /* steps with clearance < min_clearance */
  CILQR_MC_FIRST_BELOW = 4,   /* lowest such t; -1 */
  CILQR_MC_TOUCH_STEPS = 5,   /* steps with clearance <= 0 */
  CILQR_MC_OFF_MAP_STEPS = 6, /* steps whose window leaves the map */
  CILQR_MC_LOST_STEPS = 7     /* lost steps */
} cilqr_map_clearance_field;
#define CILQR_MAP_CLEARANCE_UNKNOWN_SEEDS 1u /* flags: in-map NaN cells are seeds */
int cilqr_map_clearance_device(cilqr_handle* h, void* stream, int B, int N, int S, const double* X, double margin, double occ_threshold,
                               double reach, double min_clearance, uint32_t flags, const double* base, double* mc,
                               double* step_clearance, double* total);
int cilqr_map_clearance(cilqr_handle* h, int B, int N, int S, const double* X, double margin, double occ_threshold, double reach,
                        double min_clearance, uint32_t flags, const double* base, double* mc, double* step_clearance, double* total);

/* --- stop plans: a solved plan's geometry under a braking speed profile (new) ----------------------------------------------------------
 * Every check above can only reject; when all candidates are rejected there is no plan.  This call produces the usual fallback: for
 * each of B solved plans (X [B][4*(N+1)], U [B][2*N]) and each of D braking levels decel[l] > 0 (m/s^2) one row that follows the
 * plan's own path while braking.  Row r = b*D + l is plan b at level l — the row order of X_roll — so cilqr_footprint_check and
 * cilqr_map_clearance with S = D read X_stop as it lies, pair a row's step t with obstacle column t, and take `cost` as `base`.
 * The call generates; it judges nothing beyond the three conditions of `cost`.  A row is as safe as those checks say, no more.
 *
 * Definitions (dt = timestep; fs = Model::forward_simulate, I/Model.cpp:17-30; P = (x, y) of a state).
 *   path          the plan's monotone polyline: adv_t = max((P_{t+1} - P_t).(cos th_t, sin th_t), 0) for t < N; V_0 = P_0,
 *                 V_{t+1} = V_t + adv_t (cos th_t, sin th_t); s_0 = 0, s_{t+1} = s_t + adv_t.  (The clamp: the model steps backwards by
 *                 a*dt^2/2 when v = 0 and a < 0; such segments get length 0.)  The three running sums are formed on a tree fixed
 *                 by N alone: element t = 0 ... N (element N adds nothing) belongs to chunk t / ceil((N+1)/64); a chunk is summed in
 *                 order, the 64 chunk totals are scanned by doubling (offsets 1, 2, 4 ... 32), and a chunk's elements are then added
 *                 in order onto the total before it; V_t = P_0 + the sum before element t.
 *   Q(sigma)      for sigma < s_N: V_t + (sigma - s_t)(cos th_t, sin th_t) with t = max{t <= N-1 : s_t <= sigma} (a segment of length 0
 *                 is never the one chosen).  For sigma >= s_N: V_N + (sigma - s_N)(cos th_N, sin th_N), the ray that continues the
 *                 plan — an OVERRUN: the row travels farther than the plan did.
 *   acceleration  x'_0 = X_0, sigma_0 = 0.  Step j < hold: the plan's own U_j, both components, stored unchanged.  Otherwise
 *                 a'_j = -min(decel[l], v'_j/dt); on the step where decel[l] >= v'_j/dt, v'_{j+1} is exactly 0 (a stopping vehicle
 *                 stops and does not reverse); where v'_j == 0, a'_j = w'_j = 0 and the state is held.
 *   advance       adv'_j = v'_j*dt + a*dt^2/2 with a the model's clamp of a'_j: what fs moves the row by; sigma_{j+1} = sigma_j +
 *                 max(adv'_j, 0).
 *   yaw rate      steps j >= hold: pursuit of the path by arc length.  With P'_{j+1} the position fs gives and adv'_{j+1} the advance
 *                 the NEXT step will make (its speed and acceleration are decided already), the heading wanted is the direction
 *                 atan2 from P'_{j+1} to Q(sigma_{j+1} + adv'_{j+1}), and w'_j = wrap(wanted - th'_j)/dt with wrap(d) =
 *                 d - 2 pi ceil((d - pi)/(2 pi)), into (-pi, pi].  Where adv'_{j+1} < CILQR_STOP_MIN_ADVANCE, and on the last step,
 *                 w'_j = 0.  w'_j then takes the model's clamp, v'_j*tan(steer_angle_min)/wheelbase ... v'_j*tan(steer_angle_max)/
 *                 wheelbase, and U_stop holds the clamped value.  With hold >= N the row's U is the plan's U bit for bit.
 *   X_stop        exactly the chain of fs over U_stop from X_0 (up to the speed of the stopping step, which is 0, not its rounding).
 * sp [B*D][CILQR_STOP_FIELDS] (required): see the enum; doubles that hold a value's bits, a count or an index.  A LOST row — any
 * state or control of plan b is not finite, or a heading of the plan is 1e6 rad or more in magnitude (the range of the kernel's
 * sincos) — has NaN in every element of its X_stop and U_stop rows and in its values, -1 for its indices, 0 for its counts and
 * CILQR_SP_LOST = 1.  The same range holds for a row's OWN heading th'_j: only a start speed no vehicle has (the yaw clamp grows
 * with v'_0) can carry it beyond 1e6 rad, and from there on the kernel takes cos th' = 1, sin th' = 0 without marking the row.
 * cost [B*D] or NULL: decel_weight*decel[l] + (plan_cost ? plan_cost[b] : 0), or NaN where the row is lost, where CILQR_SP_DEVIATION >
 * max_deviation (+HUGE_VAL disables this), or where the row is not at rest by step N-1 (CILQR_SP_STOP_STEP < 0 or > N-1: the footprint
 * check visits steps 0 ... N-1, and a stop it never sees finished is not a verified stop; CILQR_STOP_ALLOW_MOVING drops this
 * condition).  As `base` of cilqr_footprint_check it makes the gentlest clear row win cilqr_argmin_device.
 *   Determinism: nothing is summed across rows or plans; a row's bits depend on plan b, level l, hold and the parameters alone,
 * whatever B, D and the row's place in the batch.
 * Mapping: a workgroup holds up to four plans and up to 64 rows; each of its four wavefronts forms the path of one plan in LDS, then
 * lane = row runs the chain with two segment pointers that only move forward; rows leave through LDS as whole row segments.  One
 * launch, no atomics, nothing allocated per call.
 * CILQR_ERR_ARG, decided before the handle is looked at: NULL X, U, decel, X_stop, U_stop or sp; D < 1; hold < 0; a NaN or negative
 * max_deviation; a decel_weight that is not finite; unknown flag bits; in the host-buffer form a level that is not finite or not > 0.
 * Then the cilqr_create limits (B*D <= max_batch, N <= max_horizon; every such N fits the kernel's LDS) and, in the host-buffer form, a level above -acc_min (the model
 * would clamp it).  The device form cannot read decel on the host: there a row of a level outside (0, -acc_min] is lost.  The
 * host-buffer form's arrays — at most B*D*(12*N + 19) doubles — fit the arena reserved at create for every B*D <= max_batch. */
#define CILQR_STOP_FIELDS 8
typedef enum cilqr_stop_field {
  CILQR_SP_STOP_STEP = 0,      /* lowest j in 0 ... N with v'_j == 0; -1 when none */
  CILQR_SP_DISTANCE = 1,       /* sigma_N */
  CILQR_SP_END_SPEED = 2,      /* v'_N */
  CILQR_SP_DEVIATION = 3,      /* max over j = 0 ... N of |P'_j - Q(sigma_j)| */
  CILQR_SP_DEVIATION_STEP = 4, /* its step, lowest on equal values */
  CILQR_SP_CLAMPED_STEPS = 5,  /* steps j >= hold whose yaw rate the model's clamp changed */
  CILQR_SP_OVERRUN_STEPS = 6,  /* steps whose pursuit target lay at or beyond s_N */
  CILQR_SP_LOST = 7            /* 1: a state or control of plan b (or the level, device form) is not usable */
} cilqr_stop_field;
#define CILQR_STOP_ALLOW_MOVING 1u    /* flags: a row still moving at step N-1 keeps its cost */
#define CILQR_STOP_MIN_ADVANCE 1.0e-3 /* metres: below this advance of the next step the row does not steer */
int cilqr_stop_plans_device(cilqr_handle* h, void* stream, int B, int N, int D, const double* X, const double* U, const double* decel,
                            int hold, double max_deviation, const double* plan_cost, double decel_weight, uint32_t flags,
                            double* X_stop, double* U_stop, double* sp, double* cost);
int cilqr_stop_plans(cilqr_handle* h, int B, int N, int D, const double* X, const double* U, const double* decel, int hold,
                     double max_deviation, const double* plan_cost, double decel_weight, uint32_t flags, double* X_stop, double* U_stop,
                     double* sp, double* cost);

/* setGeometry(Length(lx,ly), res, Position(px,py)) size/length rule (G/grid_map_core/src/GridMap.cpp:45-62). */
int cilqr_map_geom_set(cilqr_map_geom* g, double len_x, double len_y, double res, double pos_x, double pos_y);

#ifdef __cplusplus
}
#endif
#endif /* CILQR_H_ */
