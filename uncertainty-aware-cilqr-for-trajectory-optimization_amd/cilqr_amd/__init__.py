"""cilqr_amd — thin Python host binding (ctypes) over the C-ABI of include/cilqr.h.

The product is `lib/libcilqr_hip.so` (hand-written HIP for gfx950 + the C-ABI); this module only loads it and
marshals numpy / torch buffers into plain pointers.  There is no CPU fallback here or in the library: if the
shared object is missing or no gfx950 device is usable, calls raise.
"""
import ctypes as C
import os

import numpy as np

PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("CILQR_LIB") or os.path.join(PKG_ROOT, "lib", "libcilqr_hip.so")  # CILQR_LIB: A/B builds when tuning

NX, NU, POLY = 4, 2, 6
FLAG_FAITHFUL_ITERS = 1
FLAG_GENERAL_ONLY = 2
EXIT_TOLERANCE, EXIT_LAMBDA_MAX, EXIT_MAX_ITER, EXIT_NUMERIC = 0, 1, 2, 3
# `cilqr_score_field`: the columns of a score row
SCORE_FIELDS = 8
(SCORE_TRACK, SCORE_CONTROL, SCORE_OBSTACLE, SCORE_UNCERTAINTY, SCORE_MAX_C, SCORE_MAX_C_ENTRY, SCORE_MAX_CTRL,
 SCORE_COLLISION) = range(SCORE_FIELDS)
# `cilqr_risk_field`: the columns of a risk row (`Solver.score_rollouts`)
RISK_FIELDS = 4
RISK_COLLISION, RISK_WORST_C, RISK_WORST_ROW, RISK_MEAN_TOTAL = range(RISK_FIELDS)
# `cilqr_rollout_risk_field`: the columns of a fused risk row (`Solver.rollout_risk`)
ROLLOUT_RISK_FIELDS = 6
RR_COLLISION, RR_WORST_C, RR_WORST_ROW, RR_WORST_ENTRY, RR_FIRST_STEP, RR_STEP_SHARE = range(ROLLOUT_RISK_FIELDS)
# `cilqr_rollout_risk_sampled_field`: the columns of a fused risk row against sampled obstacles (`Solver.rollout_risk_sampled`)
RRS_FIELDS = 8
(RRS_COLLISION, RRS_WORST_C, RRS_WORST_ROW, RRS_WORST_ENTRY, RRS_FIRST_STEP, RRS_STEP_SHARE, RRS_ANY_SHARE,
 RRS_PAIR_SHARE) = range(RRS_FIELDS)
# `cilqr_map_risk_field`: the columns of a map risk row (`Solver.rollout_risk_map`)
MAP_RISK_FIELDS = 7
MR_COLLISION, MR_WORST_OCC, MR_WORST_ROW, MR_WORST_ENTRY, MR_FIRST_STEP, MR_STEP_SHARE, MR_UNKNOWN = range(MAP_RISK_FIELDS)
MAP_RISK_UNKNOWN_HITS = 1  # flags of `rollout_risk_map`: an invalid probe counts as a hit
# `cilqr_chance_risk_field`: the columns of an analytic risk row (`Solver.chance_risk`)
CHANCE_FIELDS = 6
CR_STEP_RISK, CR_WORST_STEP, CR_SUM_RISK, CR_MAX_P, CR_MAX_ENTRY, CR_MAX_POS_SIGMA = range(CHANCE_FIELDS)
CHANCE_BOUND_SUM = 1  # flags of `chance_risk`: max_risk bounds CR_SUM_RISK instead of CR_STEP_RISK
# `cilqr_tighten_field`: the columns of a tightening row (`Solver.tighten_obstacles`)
TIGHTEN_FIELDS = 4
TG_MAX_DA, TG_MAX_DB, TG_MAX_ENTRY, TG_CAPPED = range(TIGHTEN_FIELDS)
# `cilqr_tighten_map_field`: the columns of a map tightening row (`Solver.tighten_map`)
TIGHTEN_MAP_FIELDS = 6
TM_RAISED, TM_MAX_RAISE, TM_MAX_CELL, TM_MAX_REACH, TM_CAPPED, TM_LOST = range(TIGHTEN_MAP_FIELDS)
# `cilqr_track_map_field`: the columns of a track rasterisation row (`Solver.rasterize_tracks`)
TRACK_MAP_FIELDS = 6
TKM_RAISED, TKM_MAX_VALUE, TKM_MAX_CELL, TKM_MAX_ENTRY, TKM_LOST_ENTRIES, TKM_LOST_STEPS = range(TRACK_MAP_FIELDS)
TRACK_MAP_BOUND_MIN = 1  # flags of `rasterize_tracks`: p = min(Pu, Pw), an upper bound whatever the correlation

# `cilqr_chance_map_field`: the columns of an analytic map risk row (`Solver.chance_risk_map`)
CHANCE_MAP_FIELDS = 8
(CM_STEP_RISK, CM_WORST_STEP, CM_SUM_RISK, CM_FIRST_STEP, CM_MEAN_OCC, CM_MEAN_OCC_STEP, CM_WORST_OCC,
 CM_UNKNOWN) = range(CHANCE_MAP_FIELDS)
CHANCE_MAP_UNKNOWN_HITS, CHANCE_MAP_BOUND_SUM = 1, 2  # flags of `chance_risk_map`
MAX_QUAD_NODES = 1024
# `cilqr_chance_risk_sampled_field`: the columns of an analytic risk row against sampled obstacles (`Solver.chance_risk_sampled`)
CRS_FIELDS = 8
(CRS_STEP_RISK, CRS_WORST_STEP, CRS_SUM_RISK, CRS_MAX_PAIR_P, CRS_MAX_PAIR, CRS_MAX_ENTRY_P, CRS_MAX_ENTRY,
 CRS_NOMINAL_SHARE) = range(CRS_FIELDS)
CHANCE_SAMPLED_BOUND_SUM = 1  # flags of `chance_risk_sampled`: max_risk bounds CRS_SUM_RISK instead of CRS_STEP_RISK
# `cilqr_footprint_field`: the columns of a footprint row (`Solver.footprint_check`)
FOOTPRINT_FIELDS = 12
(FP_CLEARANCE, FP_CLEARANCE_ENTRY, FP_HIT_STEPS, FP_FIRST_HIT, FP_MAP_OCC, FP_MAP_OCC_STEP, FP_MAP_OCC_CELL, FP_MAP_HIT_STEPS,
 FP_MAP_FIRST_HIT, FP_MAP_HIT_CELLS, FP_MAP_UNKNOWN_STEPS, FP_MAP_CELLS) = range(FOOTPRINT_FIELDS)
FOOTPRINT_UNKNOWN_HITS, FOOTPRINT_SKIP_MAP = 1, 2  # flags of `footprint_check`
MAP_DISTANCE_UNKNOWN_SEEDS, MAP_DISTANCE_TO_FREE = 1, 2  # flags of `map_distance`
MAP_DISTANCE_NONE = 2 ** 31 - 1  # d2 of a layer without a seed
# `cilqr_map_obstacle_field`: the columns of a component row (`Solver.map_obstacles`)
MAP_OBSTACLE_FIELDS = 13
(MO_LABEL, MO_CELLS, MO_LINKED, MO_I_MIN, MO_I_MAX, MO_J_MIN, MO_J_MAX, MO_SUM_I, MO_SUM_J, MO_SUM_II, MO_SUM_IJ, MO_SUM_JJ,
 MO_FILL) = range(MAP_OBSTACLE_FIELDS)
MAP_OBSTACLES_FOUR = 1  # flags of `map_obstacles`: 4-connectivity
MAP_OBSTACLES_FAR = 1.0e6  # metres: where the filler rows stand
MAX_POLYGONS = 1024
ERR_INTERNAL = -6
# `cilqr_track_state_field` / `cilqr_track_world_field`: a slot's row and a world's record (`Solver.track_update`)
TRACK_STATE = 32
TRACK_MAX_SLOTS = TRACK_MAX_DETECTIONS = 64
TS_X, TS_Y, TS_VX, TS_VY, TS_P = 0, 1, 2, 3, 4
TS_SIZE_X, TS_SIZE_Y, TS_YAW, TS_ID, TS_HITS, TS_MISSES, TS_AGE, TS_DET = range(20, 28)
TRACK_WORLD_FIELDS = 9
(TW_NEXT_ID, TW_TICKS, TW_LIVE, TW_CONFIRMED, TW_MATCHED, TW_BORN, TW_DIED, TW_DROPPED,
 TW_INVALID) = range(TRACK_WORLD_FIELDS)
TRACK_RESET = 1  # flags of `track_update`: every slot is free on entry
# `cilqr_clear_movers_field`: a layer's record of `Solver.clear_movers`
CLEAR_MOVERS_FIELDS = 8
(CM_MOVERS, CM_CLEARED, CM_OWNED_LINKED, CM_OWNED_HALO, CM_MAX_VALUE, CM_MAX_CELL, CM_CONTESTED,
 CM_KEPT_UNKNOWN) = range(CLEAR_MOVERS_FIELDS)
CLEAR_MOVERS_MAX_HALO2 = 1024  # cells^2
# `cilqr_map_clearance_field`: the columns of a map clearance row (`Solver.map_clearance`)
MAP_CLEARANCE_FIELDS = 8
(MC_CLEARANCE, MC_STEP, MC_CELL, MC_BELOW_STEPS, MC_FIRST_BELOW, MC_TOUCH_STEPS, MC_OFF_MAP_STEPS,
 MC_LOST_STEPS) = range(MAP_CLEARANCE_FIELDS)
MAP_CLEARANCE_UNKNOWN_SEEDS = 1  # flags of `map_clearance`
# `cilqr_stop_field`: the columns of a stop-plan row (`Solver.stop_plans`)
STOP_FIELDS = 8
(SP_STOP_STEP, SP_DISTANCE, SP_END_SPEED, SP_DEVIATION, SP_DEVIATION_STEP, SP_CLAMPED_STEPS, SP_OVERRUN_STEPS,
 SP_LOST) = range(STOP_FIELDS)
STOP_ALLOW_MOVING = 1  # flags of `stop_plans`: a row still moving at step N-1 keeps its cost
STOP_MIN_ADVANCE = 1.0e-3  # metres: below this advance of the next step a row does not steer
# path-aligned planning frame (`Solver.local_plan_frames`, `frame_obstacles`, `frame_states`, `frame_poses`)
FRAME_DOUBLES = 5  # a frame record: (ox, oy, c, s, phi)
FRAME_DEGENERATE, FRAME_NOT_MONOTONE = 1, 2  # bits of the info word
FRAME_TO, FRAME_FROM = 0, 1  # direction of `frame_states`
FRAME_GLOBAL_INFLATION = 1  # flags of `frame_obstacles`
# `cilqr_debug_math`: which device routine `Solver.debug_math` runs
MATH_EXP, MATH_SINCOS_FAST, MATH_SINCOS_LOOP, MATH_ROTATE, MATH_EXP_FAST = range(5)
MAX_HORIZON = 384  # CILQR_MAX_HORIZON

# every symbol include/cilqr.h declares
ABI_SYMBOLS = (
    "cilqr_params_default", "cilqr_abi_version", "cilqr_device_count", "cilqr_last_error", "cilqr_default_control_seq",
    "cilqr_local_plan", "cilqr_local_plan_batch", "cilqr_local_plan_batch_device", "cilqr_create", "cilqr_destroy", "cilqr_host_alloc", "cilqr_host_free", "cilqr_solve_batch", "cilqr_solve_batch_device", "cilqr_solve_batch_obstacles", "cilqr_solve_batch_obstacles_device", "cilqr_solve_batch_sampled", "cilqr_solve_batch_sampled_device",
    "cilqr_argmin_device", "cilqr_wait", "cilqr_set_diag_buffer", "cilqr_set_pass_count_buffer", "cilqr_solve_family", "cilqr_solve_wavefronts", "cilqr_solve_sampled_wavefronts", "cilqr_debug_quu_inverse", "cilqr_debug_closest_sample", "cilqr_debug_blur_ellipse", "cilqr_debug_math", "cilqr_warp_costmap", "cilqr_warp_costmap_device", "cilqr_warp_costmap_batch_device", "cilqr_blur_costmap", "cilqr_blur_costmap_device", "cilqr_blur_costmap_batch_device", "cilqr_map_geom_set",
    "cilqr_occupancy_to_layer", "cilqr_occupancy_to_layer_device", "cilqr_layer_to_occupancy", "cilqr_layer_to_occupancy_device",
    "cilqr_costmap_frame_device", "cilqr_costmap_frame_batch_device",
    "cilqr_boxes_to_polygons", "cilqr_rasterize_polygons", "cilqr_rasterize_polygons_device", "cilqr_warp_costmap_polygons_device",
    "cilqr_costmap_frame_polygons_device",
    "cilqr_set_uncertainty_map", "cilqr_set_uncertainty_map_device", "cilqr_clear_uncertainty_map", "cilqr_debug_uncertainty_cost",
    "cilqr_comm_unique_id", "cilqr_comm_init_rank", "cilqr_comm_destroy", "cilqr_comm_size", "cilqr_argmin_global_device", "cilqr_debug_select",
    "cilqr_create_multi", "cilqr_multi_destroy", "cilqr_multi_device_count", "cilqr_multi_handle", "cilqr_multi_solve_batch",
    "cilqr_shard_range", "cilqr_multi_uses_rccl", "cilqr_debug_fail_enqueue",
    "cilqr_score_batch", "cilqr_score_batch_device", "cilqr_score_batch_sampled", "cilqr_score_batch_sampled_device",
    "cilqr_gains_batch", "cilqr_gains_batch_device", "cilqr_rollout_batch", "cilqr_rollout_batch_device",
    "cilqr_score_rollouts", "cilqr_score_rollouts_device",
    "cilqr_rollout_risk", "cilqr_rollout_risk_device",
    "cilqr_gains_batch_sampled", "cilqr_gains_batch_sampled_device", "cilqr_rollout_risk_sampled", "cilqr_rollout_risk_sampled_device",
    "cilqr_rollout_risk_map", "cilqr_rollout_risk_map_device",
    "cilqr_chance_risk", "cilqr_chance_risk_device",
    "cilqr_tighten_obstacles", "cilqr_tighten_obstacles_device", "cilqr_chance_kappa",
    "cilqr_tighten_map", "cilqr_tighten_map_device",
    "cilqr_rasterize_tracks", "cilqr_rasterize_tracks_device",
    "cilqr_chance_risk_map", "cilqr_chance_risk_map_device", "cilqr_pose_quadrature",
    "cilqr_chance_risk_sampled", "cilqr_chance_risk_sampled_device",
    "cilqr_predict_obstacles", "cilqr_predict_obstacles_device", "cilqr_chance_risk_cov", "cilqr_chance_risk_cov_device",
    "cilqr_footprint_check", "cilqr_footprint_check_device",
    "cilqr_map_distance", "cilqr_map_distance_device", "cilqr_inflate_map", "cilqr_inflate_map_device",
    "cilqr_map_obstacles", "cilqr_map_obstacles_device",
    "cilqr_track_update", "cilqr_track_update_device",
    "cilqr_clear_movers", "cilqr_clear_movers_device",
    "cilqr_map_clearance", "cilqr_map_clearance_device",
    "cilqr_stop_plans", "cilqr_stop_plans_device",
    "cilqr_local_plan_frames", "cilqr_local_plan_frames_device", "cilqr_frame_obstacles", "cilqr_frame_obstacles_device",
    "cilqr_frame_states", "cilqr_frame_states_device", "cilqr_frame_poses", "cilqr_frame_poses_device",
)

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_fp = C.POINTER(C.c_float)


class Params(C.Structure):
    """`cilqr_params` — POD mirror of the reference's Parameters (I/Parameters.h:5-91)."""
    _fields_ = [(n, C.c_int32) for n in
                ("num_of_local_wpts", "poly_order", "horizon", "max_iterations", "num_states", "num_ctrls")] + \
               [(n, C.c_double) for n in
                ("desired_speed", "timestep", "tolerance", "w_acc", "w_yawrate", "w_pos", "w_vel", "w_obstacle",
                 "w_uncertainty", "q1_acc", "q2_acc", "q1_yawrate", "q2_yawrate", "q1_front", "q2_front", "q1_rear",
                 "q2_rear", "q1_uncertainty", "q2_uncertainty", "acc_max", "acc_min", "steer_angle_min",
                 "steer_angle_max", "wheelbase", "speed_max", "steer_control_max", "steer_control_min",
                 "throttle_control_max", "throttle_control_min", "t_safe", "s_safe_a", "s_safe_b", "ego_rad",
                 "ego_front", "ego_rear", "length", "width", "safe_length", "safe_width", "lamb_factor", "lamb_max")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class MapGeom(C.Structure):
    """`cilqr_map_geom` — geometry of a grid_map layer."""
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("res", C.c_double), ("len_x", C.c_double),
                ("len_y", C.c_double), ("pos_x", C.c_double), ("pos_y", C.c_double)]


class UncertaintyMap(C.Structure):
    """`cilqr_uncertainty_map` — what the reference's (absent) Uncertainty object is constructed from."""
    _fields_ = [("layer", C.c_void_p), ("geom", MapGeom), ("pose_x", C.c_double), ("pose_y", C.c_double),
                ("pose_theta", C.c_double), ("poses", C.c_void_p), ("layer_stride", C.c_int64), ("probes_l", C.c_int32),
                ("probes_w", C.c_int32)]


class Obstacles(C.Structure):
    """`cilqr_obstacles` — obstacle inputs addressed by strides in entries (4 pose + 2 dimension doubles each): obstacle m of
    solve b at step t is entry b*batch_stride + m*obstacle_stride + t*step_stride; weight[b*weight_batch_stride + m]."""
    _fields_ = [("pose", C.c_void_p), ("dim", C.c_void_p), ("weight", C.c_void_p), ("batch_stride", C.c_int64),
                ("obstacle_stride", C.c_int64), ("step_stride", C.c_int64), ("weight_batch_stride", C.c_int64)]


class TrackFilter(C.Structure):
    """`cilqr_track_filter` — the constant-velocity Kalman filter and the track life cycle of `Solver.track_update`.  Q and P_birth
    are 4 x 4 over (x, y, vx, vy), R is 2 x 2, column-major, only row <= column read."""
    _fields_ = [("dt", C.c_double), ("Q", C.c_double * 16), ("R", C.c_double * 4), ("P_birth", C.c_double * 16),
                ("gate2", C.c_double), ("v_min", C.c_double), ("theta_var_slow", C.c_double), ("min_hits", C.c_int32),
                ("max_misses", C.c_int32)]


def track_filter(dt, Q, R, P_birth, gate2=float("inf"), min_hits=1, max_misses=0, v_min=0.5, theta_var_slow=1.0):
    """A `TrackFilter` from (4, 4), (2, 2) and (4, 4) arrays (symmetric: the upper triangles are what is read)."""
    f = TrackFilter()
    f.dt, f.gate2, f.v_min, f.theta_var_slow = float(dt), float(gate2), float(v_min), float(theta_var_slow)
    f.min_hits, f.max_misses = int(min_hits), int(max_misses)
    for name, a, n in (("Q", Q, 4), ("R", R, 2), ("P_birth", P_birth, 4)):
        a = np.asarray(a, dtype=np.float64).reshape(n, n)
        getattr(f, name)[:] = a.T.reshape(-1).tolist()  # column-major
    return f


def white_acceleration_noise(q, dt):
    """Q of one tick for white acceleration of intensity q on each axis: q*dt^3/3, q*dt^2/2, q*dt."""
    Q = np.zeros((4, 4))
    for a in (0, 1):
        Q[a, a], Q[a, a + 2], Q[a + 2, a], Q[a + 2, a + 2] = q * dt ** 3 / 3, q * dt ** 2 / 2, q * dt ** 2 / 2, q * dt
    return Q


class CilqrError(RuntimeError):
    pass


def obstacle_strides(pose_shape, dim_shape, weight_shape, B, N):
    """Strides of `cilqr_obstacles` from the shapes of C-contiguous pose / dim / weight arrays, as `Solver.local_plan_batch`
    derives path_stride from the path's shape.  Returns (M, batch_stride, obstacle_stride, step_stride, weight_batch_stride):
      pose (M, 4), dim (M, 2)            one static set shared by the batch   (0, 1, 0)
      pose (B, M, 4), dim (B, M, 2)      static, one set per solve             (M, 1, 0)
      pose (M, 4N), dim (M, 2N)          one moving set shared by the batch   (0, N, 1)
      pose (B, M, 4N), dim (B, M, 2N)    dense, cilqr_solve_batch's layout    (M*N, N, 1)
      weight None, (M,) (weight_batch_stride 0) or (B, M) (M).  Anything else raises CilqrError."""
    pose_shape, dim_shape = tuple(int(d) for d in pose_shape), tuple(int(d) for d in dim_shape)
    B, N = int(B), int(N)
    if len(pose_shape) not in (2, 3) or len(dim_shape) != len(pose_shape):
        raise CilqrError("obstacle_strides: pose %s / dim %s are not (M, 4[N]) or (B, M, 4[N])" % (pose_shape, dim_shape))
    per_solve = len(pose_shape) == 3
    if per_solve and (pose_shape[0] != B or dim_shape[0] != B):
        raise CilqrError("obstacle_strides: batch dimension of pose %s / dim %s is not B = %d" % (pose_shape, dim_shape, B))
    M, cols = pose_shape[-2], pose_shape[-1]
    if dim_shape[-2] != M:
        raise CilqrError("obstacle_strides: pose has %d obstacles, dim %d" % (M, dim_shape[-2]))
    if cols == 4 and dim_shape[-1] == 2:
        ms, ts = 1, 0  # constant over the horizon
    elif cols == 4 * N and dim_shape[-1] == 2 * N:
        ms, ts = N, 1  # one column per step
    else:
        raise CilqrError("obstacle_strides: pose %s / dim %s are neither (…, M, 4) / (…, M, 2) nor (…, M, %d) / (…, M, %d)"
                         % (pose_shape, dim_shape, 4 * N, 2 * N))
    bs = M * ms if per_solve else 0
    if weight_shape is None:
        wbs = 0
    else:
        weight_shape = tuple(int(d) for d in weight_shape)
        if weight_shape == (M,):
            wbs = 0
        elif weight_shape == (B, M):
            wbs = M
        else:
            raise CilqrError("obstacle_strides: weight %s is neither (%d,) nor (%d, %d)" % (weight_shape, M, B, M))
    return M, bs, ms, ts, wbs


_lib = None


def lib():
    """Loads lib/libcilqr_hip.so (raises if it has not been built: there is no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise CilqrError("%s not built — run __graft_entry__.build() (hipcc --offload-arch=gfx950)" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        L.cilqr_last_error.restype = C.c_char_p
        L.cilqr_chance_kappa.restype = C.c_double
        L.cilqr_chance_kappa.argtypes = [C.c_double]
        for name in ABI_SYMBOLS:
            getattr(L, name)  # AttributeError if a declared symbol is not exported
        _lib = L
    return _lib


COMM_ID_BYTES = 128


def comm_unique_id():
    """ncclGetUniqueId through the C-ABI: 128 opaque bytes for `Solver.comm_init_rank` on every rank."""
    buf = (C.c_char * COMM_ID_BYTES)()
    _check(lib().cilqr_comm_unique_id(buf))
    return bytes(buf.raw)


def shard_range(B, n_shards, shard):
    """`cilqr_shard_range`: (first, count) of the contiguous, balanced shard a device / rank owns (host arithmetic only)."""
    first, count = C.c_int(), C.c_int()
    _check(lib().cilqr_shard_range(int(B), int(n_shards), int(shard), C.byref(first), C.byref(count)))
    return first.value, count.value


def pinned_empty(shape, dtype=np.float64):
    """A numpy array over page-locked memory from `cilqr_host_alloc` (never freed: keep and reuse it)."""
    L = lib()
    L.cilqr_host_alloc.restype = C.c_void_p
    L.cilqr_host_alloc.argtypes = [C.c_size_t]
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    p = L.cilqr_host_alloc(max(n, 1))
    if not p:
        raise CilqrError("cilqr_host_alloc failed: %s" % L.cilqr_last_error().decode())
    buf = (C.c_char * max(n, 1)).from_address(p)
    return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)


def pinned_copy(a):
    a = np.ascontiguousarray(a)
    out = pinned_empty(a.shape, a.dtype)
    out[...] = a
    return out


def _check(rc):
    if rc != 0:
        raise CilqrError("cilqr error %d: %s" % (rc, lib().cilqr_last_error().decode()))


def chance_kappa(eps):
    """`cilqr_chance_kappa`: the kappa with erfc(kappa / sqrt 2) / 2 = eps; NaN outside (0, 0.5], exactly 0 at 0.5."""
    return float(lib().cilqr_chance_kappa(float(eps)))


def pose_quadrature(nx=5, ny=5, nth=3):
    """`cilqr_pose_quadrature`: the tensor product of probabilists' Gauss-Hermite rules, 1 ... 9 nodes per axis.  Returns (nodes
    (nx*ny*nth, 3) = (z_x, z_y, z_theta), weights (nx*ny*nth,)), z_theta fastest, z_x slowest; each axis' weights sum to 1."""
    Q = max(int(nx), 0) * max(int(ny), 0) * max(int(nth), 0)
    nodes, weights = np.zeros((max(Q, 1), 3)), np.zeros(max(Q, 1))
    _check(lib().cilqr_pose_quadrature(int(nx), int(ny), int(nth), _p(nodes), _p(weights)))
    return nodes[:Q], weights[:Q]


def default_params(horizon=None):
    p = Params()
    lib().cilqr_params_default(C.byref(p))
    if horizon is not None:
        p.horizon = horizon
    return p


def default_control_seq(N):
    U = np.zeros(2 * N)
    _check(lib().cilqr_default_control_seq(int(N), U.ctypes.data_as(_dp)))
    return U


def local_plan(p, path, ego):
    """LocalPlanner pre-step.  path: (P, 2) waypoints.  Returns (coeffs[6], ref_traj (n, 2))."""
    path = np.ascontiguousarray(path, dtype=np.float64)
    ego = np.ascontiguousarray(ego, dtype=np.float64)
    coeffs = np.zeros(p.poly_order + 1)
    ref = np.zeros(2 * p.num_of_local_wpts)
    n = C.c_int(0)
    _check(lib().cilqr_local_plan(C.byref(p), path.ctypes.data_as(_dp), int(path.size // 2), ego.ctypes.data_as(_dp),
                                  coeffs.ctypes.data_as(_dp), ref.ctypes.data_as(_dp), C.byref(n)))
    return coeffs, ref[:2 * n.value].reshape(n.value, 2)


def map_geom(len_x, len_y, res, pos_x, pos_y):
    g = MapGeom()
    _check(lib().cilqr_map_geom_set(C.byref(g), C.c_double(len_x), C.c_double(len_y), C.c_double(res),
                                    C.c_double(pos_x), C.c_double(pos_y)))
    return g


def boxes_to_polygons(boxes, own_x, own_y, own_yaw, inflate=0.2, max_distance=100.0):
    """`cilqr_boxes_to_polygons` (bondingBoxHandle's corner arithmetic, host only).  boxes: (n, 5) = (x, y, yaw, size_x, size_y) in the
    planning frame.  Returns the (n_kept, 4, 2) corners of the boxes within max_distance, in the vehicle frame."""
    boxes = np.ascontiguousarray(boxes, dtype=np.float64).reshape(-1, 5)
    out = np.zeros((boxes.shape[0], 4, 2))
    kept = C.c_int32(0)
    _check(lib().cilqr_boxes_to_polygons(int(boxes.shape[0]), boxes.ctypes.data_as(_dp), C.c_double(own_x), C.c_double(own_y),
                                         C.c_double(own_yaw), C.c_double(inflate), C.c_double(max_distance), out.ctypes.data_as(_dp),
                                         C.byref(kept)))
    return out[:kept.value].copy()


def _polygons(vertices):
    """(n, V, 2) float64 C-contiguous vertices -> (array, n, V); an empty list of polygons is (0, V, 2) or just empty (V = 4)."""
    v = np.ascontiguousarray(vertices, dtype=np.float64)
    if v.ndim != 3:
        if v.size:
            raise CilqrError("polygons must have shape (n, V, 2), not %s" % (v.shape,))
        v = v.reshape(0, 4, 2)
    if v.shape[2] != 2:
        raise CilqrError("polygons must have shape (n, V, 2), not %s" % (v.shape,))
    return v, int(v.shape[0]), int(v.shape[1])


def _np64(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def _p(a, t=_dp):
    return None if a is None else a.ctypes.data_as(t)


def _vp(ptr):
    return C.c_void_p(int(ptr)) if ptr else None


class Solver:
    """One handle = one device = one host thread at a time (mirrors one reference `iLQR` object per batch slot)."""

    def __init__(self, params=None, max_batch=1024, max_horizon=50, max_obstacles=4, device=0):
        self.params = params if params is not None else default_params()
        self.max_batch, self.max_horizon, self.max_obstacles, self.device = max_batch, max_horizon, max_obstacles, device
        self._h = C.c_void_p()
        _check(lib().cilqr_create(C.byref(self.params), int(max_batch), int(max_horizon), int(max_obstacles),
                                  int(device), C.byref(self._h)))

    def close(self):
        if self._h:
            lib().cilqr_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- host-buffer entry point (synchronous) ----
    def solve_batch(self, N, x0, U, poly, xplan_fl, obs_pose=None, obs_dim=None, obs_weight=None, flags=0, out=None):
        """out: optional dict of preallocated arrays U (in/out: holds the warm start), X, J, iters, status — e.g. over pinned
        memory (`pinned_empty`); then U is used in place instead of being copied."""
        x0 = _np64(x0).reshape(-1, 4)
        B = x0.shape[0]
        U = _np64(U).reshape(B, 2 * N).copy() if out is None else out["U"]
        poly = _np64(poly).reshape(B, POLY)
        xplan_fl = _np64(xplan_fl).reshape(B, 2)
        M = 0
        if obs_pose is not None:
            obs_pose = _np64(obs_pose).reshape(B, -1, 4 * N)
            M = obs_pose.shape[1]
            obs_dim = _np64(obs_dim).reshape(B, M, 2 * N)
            if obs_weight is not None:
                obs_weight = _np64(obs_weight).reshape(B, M)
        if out is None:
            X, J = np.zeros((B, 4 * (N + 1))), np.zeros(B)
            iters, status = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
        else:
            X, J, iters, status = out["X"], out["J"], out["iters"], out["status"]
        _check(lib().cilqr_solve_batch(self._h, B, int(N), int(M), _p(x0), _p(U), _p(poly), _p(xplan_fl), _p(obs_pose),
                                       _p(obs_dim), _p(obs_weight), _p(X), _p(J), _p(iters, _ip), _p(status, _ip),
                                       C.c_uint32(flags)))
        return dict(U=U, X=X, J=J, iters=iters, status=status)

    def solve_batch_obstacles(self, N, x0, U, poly, xplan_fl, obs_pose=None, obs_dim=None, obs_weight=None, flags=0, out=None):
        """`cilqr_solve_batch_obstacles`: solve_batch with the obstacles in any of the shapes of `obstacle_strides` — e.g. one
        static set (M, 4) / (M, 2) for the whole batch — of which only those entries travel.  Same results as solve_batch on
        the dense expansion, bit for bit."""
        x0 = _np64(x0).reshape(-1, 4)
        B = x0.shape[0]
        U = _np64(U).reshape(B, 2 * N).copy() if out is None else out["U"]
        poly = _np64(poly).reshape(B, POLY)
        xplan_fl = _np64(xplan_fl).reshape(B, 2)
        M, obs = 0, None
        if obs_pose is not None:
            obs_pose, obs_dim, obs_weight = _np64(obs_pose), _np64(obs_dim), _np64(obs_weight)
            M, bs, ms, ts, wbs = obstacle_strides(obs_pose.shape, obs_dim.shape, None if obs_weight is None else obs_weight.shape, B, N)
            obs = Obstacles(obs_pose.ctypes.data, obs_dim.ctypes.data, None if obs_weight is None else obs_weight.ctypes.data,
                            bs, ms, ts, wbs)
        if out is None:
            X, J = np.zeros((B, 4 * (N + 1))), np.zeros(B)
            iters, status = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
        else:
            X, J, iters, status = out["X"], out["J"], out["iters"], out["status"]
        _check(lib().cilqr_solve_batch_obstacles(self._h, B, int(N), int(M), _p(x0), _p(U), _p(poly), _p(xplan_fl),
                                                 None if obs is None else C.byref(obs), _p(X), _p(J), _p(iters, _ip),
                                                 _p(status, _ip), C.c_uint32(flags)))
        return dict(U=U, X=X, J=J, iters=iters, status=status)

    def solve_batch_sampled(self, N, x0, U, poly, xplan_fl, nom_pose, nom_dim, offsets, weight, flags=0):
        """Sampled obstacles in compact form: nom_pose (B, n_obs, 4N), nom_dim (B, n_obs, 2N), offsets (B, n_obs, S, 3)."""
        x0 = _np64(x0).reshape(-1, 4)
        B = x0.shape[0]
        U = _np64(U).reshape(B, 2 * N).copy()
        poly = _np64(poly).reshape(B, POLY)
        xplan_fl = _np64(xplan_fl).reshape(B, 2)
        offsets = _np64(offsets)
        n_obs, S = offsets.shape[1], offsets.shape[2]
        nom_pose = _np64(nom_pose).reshape(B, n_obs, 4 * N)
        nom_dim = _np64(nom_dim).reshape(B, n_obs, 2 * N)
        offsets = offsets.reshape(B, n_obs, S, 3)
        X = np.zeros((B, 4 * (N + 1)))
        J = np.zeros(B)
        iters = np.zeros(B, dtype=np.int32)
        status = np.zeros(B, dtype=np.int32)
        _check(lib().cilqr_solve_batch_sampled(self._h, B, int(N), int(n_obs), int(S), _p(x0), _p(U), _p(poly), _p(xplan_fl),
                                               _p(nom_pose), _p(nom_dim), _p(offsets), C.c_double(weight), _p(X), _p(J),
                                               _p(iters, _ip), _p(status, _ip), C.c_uint32(flags)))
        return dict(U=U, X=X, J=J, iters=iters, status=status)

    def solve_batch_sampled_device(self, stream, B, N, n_obs, n_samples, x0, U, poly, xplan_fl, nom_pose, nom_dim, offsets, weight,
                                   X_out, J_out, iters_out, status_out, flags=0):
        _check(lib().cilqr_solve_batch_sampled_device(self._h, _vp(stream), int(B), int(N), int(n_obs), int(n_samples), _vp(x0),
                                                      _vp(U), _vp(poly), _vp(xplan_fl), _vp(nom_pose), _vp(nom_dim), _vp(offsets),
                                                      C.c_double(weight), _vp(X_out), _vp(J_out), _vp(iters_out), _vp(status_out),
                                                      C.c_uint32(flags)))

    # ---- device-pointer entry point (asynchronous on `stream`) ----
    def solve_batch_device(self, stream, B, N, M, x0, U, poly, xplan_fl, obs_pose, obs_dim, obs_weight, X_out, J_out,
                           iters_out, status_out, flags=0):
        """All pointer arguments are integer device addresses (e.g. torch.Tensor.data_ptr()); 0/None = NULL."""
        _check(lib().cilqr_solve_batch_device(self._h, _vp(stream), int(B), int(N), int(M), _vp(x0), _vp(U), _vp(poly),
                                              _vp(xplan_fl), _vp(obs_pose), _vp(obs_dim), _vp(obs_weight), _vp(X_out),
                                              _vp(J_out), _vp(iters_out), _vp(status_out), C.c_uint32(flags)))

    def solve_batch_obstacles_device(self, stream, B, N, M, x0, U, poly, xplan_fl, obs_pose, obs_dim, obs_weight, strides, X_out,
                                     J_out, iters_out, status_out, flags=0):
        """`cilqr_solve_batch_obstacles_device`: device addresses as solve_batch_device; strides = (batch_stride,
        obstacle_stride, step_stride, weight_batch_stride) in entries (`obstacle_strides` maps shapes to them)."""
        bs, ms, ts, wbs = (int(v) for v in strides)
        obs = Obstacles(int(obs_pose) if obs_pose else None, int(obs_dim) if obs_dim else None,
                        int(obs_weight) if obs_weight else None, bs, ms, ts, wbs)
        _check(lib().cilqr_solve_batch_obstacles_device(self._h, _vp(stream), int(B), int(N), int(M), _vp(x0), _vp(U), _vp(poly),
                                                        _vp(xplan_fl), C.byref(obs), _vp(X_out), _vp(J_out), _vp(iters_out),
                                                        _vp(status_out), C.c_uint32(flags)))

    # ---- scoring solved candidates ----
    def score_batch(self, N, X, U, poly, xplan_fl, obs_pose=None, obs_dim=None, obs_weight=None, max_collision=1.0):
        """`cilqr_score_batch`: X (B, 4(N+1)), U (B, 2N) as a solve returns them, the obstacles in any of the shapes of
        `obstacle_strides`.  Returns dict(score (B, SCORE_FIELDS), total (B,)); total is NaN where the collision share
        exceeds max_collision or a term is not finite — hand it to `argmin_device` in place of J."""
        X = _np64(X)
        B = X.size // (4 * (N + 1))
        X = X.reshape(B, 4 * (N + 1))
        U = _np64(U).reshape(B, 2 * N)
        poly = _np64(poly).reshape(B, POLY)
        xplan_fl = _np64(xplan_fl).reshape(B, 2)
        M, obs = 0, None
        if obs_pose is not None:
            obs_pose, obs_dim, obs_weight = _np64(obs_pose), _np64(obs_dim), _np64(obs_weight)
            M, bs, ms, ts, wbs = obstacle_strides(obs_pose.shape, obs_dim.shape, None if obs_weight is None else obs_weight.shape, B, N)
            obs = Obstacles(obs_pose.ctypes.data, obs_dim.ctypes.data, None if obs_weight is None else obs_weight.ctypes.data,
                            bs, ms, ts, wbs)
        score, total = np.zeros((B, SCORE_FIELDS)), np.zeros(B)
        _check(lib().cilqr_score_batch(self._h, B, int(N), int(M), _p(X), _p(U), _p(poly), _p(xplan_fl),
                                       None if obs is None else C.byref(obs), C.c_double(max_collision), _p(score), _p(total)))
        return dict(score=score, total=total)

    def score_batch_device(self, stream, B, N, M, X, U, poly, xplan_fl, obs_pose, obs_dim, obs_weight, strides, score, total=0,
                           max_collision=1.0):
        """`cilqr_score_batch_device`: device addresses and strides as `solve_batch_obstacles_device`; score: B*8 doubles,
        total: B doubles or 0."""
        bs, ms, ts, wbs = (int(v) for v in strides)
        obs = Obstacles(int(obs_pose) if obs_pose else None, int(obs_dim) if obs_dim else None,
                        int(obs_weight) if obs_weight else None, bs, ms, ts, wbs)
        _check(lib().cilqr_score_batch_device(self._h, _vp(stream), int(B), int(N), int(M), _vp(X), _vp(U), _vp(poly), _vp(xplan_fl),
                                              C.byref(obs) if M else None, C.c_double(max_collision), _vp(score), _vp(total)))

    def score_batch_sampled(self, N, X, U, poly, xplan_fl, nom_pose, nom_dim, offsets, weight, max_collision=1.0):
        """`cilqr_score_batch_sampled`: the compact form of `solve_batch_sampled`; COLLISION is the largest share of an obstacle's
        pose samples hit at one step."""
        offsets = _np64(offsets)
        B, n_obs, S = offsets.shape[0], offsets.shape[1], offsets.shape[2]
        X = _np64(X).reshape(B, 4 * (N + 1))
        U = _np64(U).reshape(B, 2 * N)
        poly = _np64(poly).reshape(B, POLY)
        xplan_fl = _np64(xplan_fl).reshape(B, 2)
        nom_pose = _np64(nom_pose).reshape(B, n_obs, 4 * N)
        nom_dim = _np64(nom_dim).reshape(B, n_obs, 2 * N)
        offsets = offsets.reshape(B, n_obs, S, 3)
        score, total = np.zeros((B, SCORE_FIELDS)), np.zeros(B)
        _check(lib().cilqr_score_batch_sampled(self._h, B, int(N), int(n_obs), int(S), _p(X), _p(U), _p(poly), _p(xplan_fl),
                                               _p(nom_pose), _p(nom_dim), _p(offsets), C.c_double(weight), C.c_double(max_collision),
                                               _p(score), _p(total)))
        return dict(score=score, total=total)

    def score_batch_sampled_device(self, stream, B, N, n_obs, n_samples, X, U, poly, xplan_fl, nom_pose, nom_dim, offsets, weight,
                                   score, total=0, max_collision=1.0):
        _check(lib().cilqr_score_batch_sampled_device(self._h, _vp(stream), int(B), int(N), int(n_obs), int(n_samples), _vp(X), _vp(U),
                                                      _vp(poly), _vp(xplan_fl), _vp(nom_pose), _vp(nom_dim), _vp(offsets),
                                                      C.c_double(weight), C.c_double(max_collision), _vp(score), _vp(total)))

    # ---- feedback gains, closed-loop rollouts from offset starts, collision risk ----
    def _obstacles(self, obs_pose, obs_dim, obs_weight, B, N):
        """(M, Obstacles or None, keepalive) from host arrays in any of the shapes of `obstacle_strides`."""
        if obs_pose is None:
            return 0, None, ()
        obs_pose, obs_dim, obs_weight = _np64(obs_pose), _np64(obs_dim), _np64(obs_weight)
        M, bs, ms, ts, wbs = obstacle_strides(obs_pose.shape, obs_dim.shape, None if obs_weight is None else obs_weight.shape, B, N)
        obs = Obstacles(obs_pose.ctypes.data, obs_dim.ctypes.data, None if obs_weight is None else obs_weight.ctypes.data, bs, ms, ts, wbs)
        return M, obs, (obs_pose, obs_dim, obs_weight)

    def gains_batch(self, N, X, U, poly, xplan_fl, obs_pose=None, obs_dim=None, obs_weight=None, lamb=1.0):
        """`cilqr_gains_batch`: one backward pass at X (B, 4(N+1)), U (B, 2N) with regularisation lamb (1.0: the reference's starting
        value).  Returns dict(k (B, 2N), K (B, 8N) with K[8t + r + 2c], ok (B,) int32)."""
        X = _np64(X)
        B = X.size // (4 * (N + 1))
        X = X.reshape(B, 4 * (N + 1))
        U = _np64(U).reshape(B, 2 * N)
        poly = _np64(poly).reshape(B, POLY)
        xplan_fl = _np64(xplan_fl).reshape(B, 2)
        M, obs, keep = self._obstacles(obs_pose, obs_dim, obs_weight, B, N)
        k, K, ok = np.zeros((B, 2 * N)), np.zeros((B, 8 * N)), np.zeros(B, dtype=np.int32)
        _check(lib().cilqr_gains_batch(self._h, B, int(N), int(M), _p(X), _p(U), _p(poly), _p(xplan_fl),
                                       None if obs is None else C.byref(obs), C.c_double(lamb), _p(k), _p(K), _p(ok, _ip)))
        return dict(k=k, K=K, ok=ok)

    def gains_batch_device(self, stream, B, N, M, X, U, poly, xplan_fl, obs_pose, obs_dim, obs_weight, strides, k_out, K_out, ok_out=0,
                           lamb=1.0):
        """`cilqr_gains_batch_device`: device addresses and strides as `score_batch_device`."""
        bs, ms, ts, wbs = (int(v) for v in strides)
        obs = Obstacles(int(obs_pose) if obs_pose else None, int(obs_dim) if obs_dim else None,
                        int(obs_weight) if obs_weight else None, bs, ms, ts, wbs)
        _check(lib().cilqr_gains_batch_device(self._h, _vp(stream), int(B), int(N), int(M), _vp(X), _vp(U), _vp(poly), _vp(xplan_fl),
                                              C.byref(obs) if M else None, C.c_double(lamb), _vp(k_out), _vp(K_out), _vp(ok_out)))

    def rollout_batch(self, N, X, U, k, K, delta, k_scale=0.0):
        """`cilqr_rollout_batch`: S closed-loop rollouts per solve.  delta: (S, 4) offsets (dx, dy, dv, dtheta) shared by all solves, or
        (B, S, 4) one set per solve.  Returns dict(X (B, S, 4(N+1)), U (B, S, 2N)); B*S must not exceed max_batch."""
        X = _np64(X)
        B = X.size // (4 * (N + 1))
        X = X.reshape(B, 4 * (N + 1))
        U, k, K = _np64(U).reshape(B, 2 * N), _np64(k).reshape(B, 2 * N), _np64(K).reshape(B, 8 * N)
        delta = _np64(delta)
        if delta.ndim == 3:
            if delta.shape[0] != B or delta.shape[2] != 4:
                raise CilqrError("rollout_batch: delta %s is neither (S, 4) nor (%d, S, 4)" % (delta.shape, B))
            S, stride = delta.shape[1], 1
        else:
            delta = delta.reshape(-1, 4)
            S, stride = delta.shape[0], 0
        Xr, Ur = np.zeros((B, S, 4 * (N + 1))), np.zeros((B, S, 2 * N))
        _check(lib().cilqr_rollout_batch(self._h, B, int(N), int(S), _p(X), _p(U), _p(k), _p(K), _p(delta), C.c_int64(stride),
                                         C.c_double(k_scale), _p(Xr), _p(Ur)))
        return dict(X=Xr, U=Ur)

    def rollout_batch_device(self, stream, B, N, S, X, U, k, K, delta, delta_batch_stride, X_roll, U_roll, k_scale=0.0):
        _check(lib().cilqr_rollout_batch_device(self._h, _vp(stream), int(B), int(N), int(S), _vp(X), _vp(U), _vp(k), _vp(K), _vp(delta),
                                                C.c_int64(delta_batch_stride), C.c_double(k_scale), _vp(X_roll), _vp(U_roll)))

    def score_rollouts(self, N, X_roll, U_roll, poly, xplan_fl, obs_pose=None, obs_dim=None, obs_weight=None, max_risk=1.0):
        """`cilqr_score_rollouts`: X_roll (B, S, 4(N+1)), U_roll (B, S, 2N) as `rollout_batch` returns them, everything else per solve.
        Returns dict(row_score (B, S, SCORE_FIELDS), risk (B, RISK_FIELDS), total (B,)); total is NaN where the share of colliding
        rows exceeds max_risk — hand it to `argmin_device` in place of J."""
        X_roll = _np64(X_roll)
        if X_roll.ndim != 3 or X_roll.shape[2] != 4 * (N + 1):
            raise CilqrError("score_rollouts: X_roll %s is not (B, S, %d)" % (X_roll.shape, 4 * (N + 1)))
        B, S = X_roll.shape[0], X_roll.shape[1]
        U_roll = _np64(U_roll).reshape(B, S, 2 * N)
        poly = _np64(poly).reshape(B, POLY)
        xplan_fl = _np64(xplan_fl).reshape(B, 2)
        M, obs, keep = self._obstacles(obs_pose, obs_dim, obs_weight, B, N)
        rows, risk, total = np.zeros((B, S, SCORE_FIELDS)), np.zeros((B, RISK_FIELDS)), np.zeros(B)
        _check(lib().cilqr_score_rollouts(self._h, B, int(N), int(M), int(S), _p(X_roll), _p(U_roll), _p(poly), _p(xplan_fl),
                                          None if obs is None else C.byref(obs), C.c_double(max_risk), _p(rows), _p(risk), _p(total)))
        return dict(row_score=rows, risk=risk, total=total)

    def score_rollouts_device(self, stream, B, N, M, S, X_roll, U_roll, poly, xplan_fl, obs_pose, obs_dim, obs_weight, strides, row_score,
                              risk, total=0, max_risk=1.0):
        """`cilqr_score_rollouts_device`: device addresses; strides as `score_batch_device` (per SOLVE, not per row)."""
        bs, ms, ts, wbs = (int(v) for v in strides)
        obs = Obstacles(int(obs_pose) if obs_pose else None, int(obs_dim) if obs_dim else None,
                        int(obs_weight) if obs_weight else None, bs, ms, ts, wbs)
        _check(lib().cilqr_score_rollouts_device(self._h, _vp(stream), int(B), int(N), int(M), int(S), _vp(X_roll), _vp(U_roll), _vp(poly),
                                                 _vp(xplan_fl), C.byref(obs) if M else None, C.c_double(max_risk), _vp(row_score),
                                                 _vp(risk), _vp(total)))

    def rollout_risk(self, N, X, U, k, K, delta, obs_pose=None, obs_dim=None, obs_weight=None, k_scale=0.0, max_risk=1.0, base=None):
        """`cilqr_rollout_risk`: the collision risk of S closed-loop rollouts per solve in one launch, no rollout stored.  X, U, k, K,
        delta and k_scale as `rollout_batch`; obstacles in any shape of `obstacle_strides` (weights are accepted and not read).
        Returns (risk (B, ROLLOUT_RISK_FIELDS), step_hits (B, N) int32, total): total[b] is base[b], NaN where RR_COLLISION exceeds
        max_risk or base[b] is not finite — hand it to `argmin_device`; None without `base`."""
        X = _np64(X)
        B = X.size // (4 * (N + 1))
        X = X.reshape(B, 4 * (N + 1))
        U, k, K = _np64(U).reshape(B, 2 * N), _np64(k).reshape(B, 2 * N), _np64(K).reshape(B, 8 * N)
        delta = _np64(delta)
        if delta.ndim == 3:
            if delta.shape[0] != B or delta.shape[2] != 4:
                raise CilqrError("rollout_risk: delta %s is neither (S, 4) nor (%d, S, 4)" % (delta.shape, B))
            S, stride = delta.shape[1], 1
        else:
            delta = delta.reshape(-1, 4)
            S, stride = delta.shape[0], 0
        M, obs, keep = self._obstacles(obs_pose, obs_dim, obs_weight, B, N)
        base = None if base is None else _np64(base).reshape(B)
        risk, step_hits = np.zeros((B, ROLLOUT_RISK_FIELDS)), np.zeros((B, N), dtype=np.int32)
        total = None if base is None else np.zeros(B)
        _check(lib().cilqr_rollout_risk(self._h, B, int(N), int(M), int(S), _p(X), _p(U), _p(k), _p(K), _p(delta), C.c_int64(stride),
                                        C.c_double(k_scale), None if obs is None else C.byref(obs), C.c_double(max_risk), _p(base),
                                        _p(risk), _p(step_hits, _ip), _p(total)))
        return risk, step_hits, total

    def rollout_risk_device(self, stream, B, N, M, S, X, U, k, K, delta, delta_batch_stride, obs_pose, obs_dim, strides, risk,
                            step_hits=0, total=0, base=0, k_scale=0.0, max_risk=1.0):
        """`cilqr_rollout_risk_device`: device addresses; strides (batch, obstacle, step, weight batch) as `score_batch_device`."""
        bs, ms, ts, wbs = (int(v) for v in strides)
        obs = Obstacles(int(obs_pose) if obs_pose else None, int(obs_dim) if obs_dim else None, None, bs, ms, ts, wbs)
        _check(lib().cilqr_rollout_risk_device(self._h, _vp(stream), int(B), int(N), int(M), int(S), _vp(X), _vp(U), _vp(k), _vp(K),
                                               _vp(delta), C.c_int64(delta_batch_stride), C.c_double(k_scale),
                                               C.byref(obs) if M else None, C.c_double(max_risk), _vp(base), _vp(risk), _vp(step_hits),
                                               _vp(total)))

    # ---- gains and fused rollout risk for sampled obstacles in compact form ----
    def gains_batch_sampled(self, N, X, U, poly, xplan_fl, nom_pose, nom_dim, offsets, weight, lamb=1.0):
        """`cilqr_gains_batch_sampled`: `gains_batch` on the compact form of `solve_batch_sampled` — nom_pose (B, n_obs, 4N), nom_dim
        (B, n_obs, 2N), offsets (B, n_obs, n_samples, 3); the gains of `gains_batch` on the materialised obstacles, bit for bit."""
        offsets = _np64(offsets)
        B, n_obs, ns = offsets.shape[0], offsets.shape[1], offsets.shape[2]
        X = _np64(X).reshape(B, 4 * (N + 1))
        U = _np64(U).reshape(B, 2 * N)
        poly = _np64(poly).reshape(B, POLY)
        xplan_fl = _np64(xplan_fl).reshape(B, 2)
        nom_pose = _np64(nom_pose).reshape(B, n_obs, 4 * N)
        nom_dim = _np64(nom_dim).reshape(B, n_obs, 2 * N)
        offsets = offsets.reshape(B, n_obs, ns, 3)
        k, K, ok = np.zeros((B, 2 * N)), np.zeros((B, 8 * N)), np.zeros(B, dtype=np.int32)
        _check(lib().cilqr_gains_batch_sampled(self._h, B, int(N), int(n_obs), int(ns), _p(X), _p(U), _p(poly), _p(xplan_fl), _p(nom_pose),
                                               _p(nom_dim), _p(offsets), C.c_double(weight), C.c_double(lamb), _p(k), _p(K), _p(ok, _ip)))
        return dict(k=k, K=K, ok=ok)

    def gains_batch_sampled_device(self, stream, B, N, n_obs, n_samples, X, U, poly, xplan_fl, nom_pose, nom_dim, offsets, weight, k_out,
                                   K_out, ok_out=0, lamb=1.0):
        """`cilqr_gains_batch_sampled_device`: device addresses."""
        _check(lib().cilqr_gains_batch_sampled_device(self._h, _vp(stream), int(B), int(N), int(n_obs), int(n_samples), _vp(X), _vp(U),
                                                      _vp(poly), _vp(xplan_fl), _vp(nom_pose), _vp(nom_dim), _vp(offsets),
                                                      C.c_double(weight), C.c_double(lamb), _vp(k_out), _vp(K_out), _vp(ok_out)))

    def rollout_risk_sampled(self, N, X, U, k, K, delta, nom_pose, nom_dim, offsets, k_scale=0.0, max_risk=1.0, base=None):
        """`cilqr_rollout_risk_sampled`: `rollout_risk` against sampled obstacles in compact form.  X, U, k, K, delta and k_scale as
        `rollout_batch`; nom_pose, nom_dim, offsets as `solve_batch_sampled`.  Returns (risk (B, RRS_FIELDS), step_hits (B, N) int32,
        total): total[b] is base[b], NaN where RRS_COLLISION exceeds max_risk or base[b] is not finite; None without `base`."""
        offsets = _np64(offsets)
        B, n_obs, ns = offsets.shape[0], offsets.shape[1], offsets.shape[2]
        X = _np64(X).reshape(B, 4 * (N + 1))
        U, k, K = _np64(U).reshape(B, 2 * N), _np64(k).reshape(B, 2 * N), _np64(K).reshape(B, 8 * N)
        delta = _np64(delta)
        if delta.ndim == 3:
            if delta.shape[0] != B or delta.shape[2] != 4:
                raise CilqrError("rollout_risk_sampled: delta %s is neither (S, 4) nor (%d, S, 4)" % (delta.shape, B))
            S, stride = delta.shape[1], 1
        else:
            delta = delta.reshape(-1, 4)
            S, stride = delta.shape[0], 0
        nom_pose = _np64(nom_pose).reshape(B, n_obs, 4 * N)
        nom_dim = _np64(nom_dim).reshape(B, n_obs, 2 * N)
        offsets = offsets.reshape(B, n_obs, ns, 3)
        base = None if base is None else _np64(base).reshape(B)
        risk, step_hits = np.zeros((B, RRS_FIELDS)), np.zeros((B, N), dtype=np.int32)
        total = None if base is None else np.zeros(B)
        _check(lib().cilqr_rollout_risk_sampled(self._h, B, int(N), int(n_obs), int(ns), int(S), _p(X), _p(U), _p(k), _p(K), _p(delta),
                                                C.c_int64(stride), C.c_double(k_scale), _p(nom_pose), _p(nom_dim), _p(offsets),
                                                C.c_double(max_risk), _p(base), _p(risk), _p(step_hits, _ip), _p(total)))
        return risk, step_hits, total

    def rollout_risk_sampled_device(self, stream, B, N, n_obs, n_samples, S, X, U, k, K, delta, delta_batch_stride, nom_pose, nom_dim,
                                    offsets, risk, step_hits=0, total=0, base=0, k_scale=0.0, max_risk=1.0):
        """`cilqr_rollout_risk_sampled_device`: device addresses."""
        _check(lib().cilqr_rollout_risk_sampled_device(self._h, _vp(stream), int(B), int(N), int(n_obs), int(n_samples), int(S), _vp(X),
                                                       _vp(U), _vp(k), _vp(K), _vp(delta), C.c_int64(delta_batch_stride),
                                                       C.c_double(k_scale), _vp(nom_pose), _vp(nom_dim), _vp(offsets),
                                                       C.c_double(max_risk), _vp(base), _vp(risk), _vp(step_hits), _vp(total)))

    # ---- map rollout risk: the rollouts against the uncertainty map set on the handle ----
    def rollout_risk_map(self, N, X, U, k, K, delta, occ_threshold, k_scale=0.0, max_risk=1.0, base=None, unknown_hits=False):
        """`cilqr_rollout_risk_map`: the share of S closed-loop rollouts per solve whose footprint probes enter cells of the
        uncertainty map set on the handle above `occ_threshold`.  X, U, k, K, delta and k_scale as `rollout_batch`; unknown_hits:
        a probe outside the map or on a cell that is not finite counts as a hit (MAP_RISK_UNKNOWN_HITS).  Returns (risk
        (B, MAP_RISK_FIELDS), step_hits (B, N) int32, unknown_hits (B, N) int32, total): total[b] is base[b], NaN where MR_COLLISION
        exceeds max_risk or base[b] is not finite — `base` is typically the total of `rollout_risk`; None without `base`."""
        X = _np64(X)
        B = X.size // (4 * (N + 1))
        X = X.reshape(B, 4 * (N + 1))
        U, k, K = _np64(U).reshape(B, 2 * N), _np64(k).reshape(B, 2 * N), _np64(K).reshape(B, 8 * N)
        delta = _np64(delta)
        if delta.ndim == 3:
            if delta.shape[0] != B or delta.shape[2] != 4:
                raise CilqrError("rollout_risk_map: delta %s is neither (S, 4) nor (%d, S, 4)" % (delta.shape, B))
            S, stride = delta.shape[1], 1
        else:
            delta = delta.reshape(-1, 4)
            S, stride = delta.shape[0], 0
        base = None if base is None else _np64(base).reshape(B)
        risk = np.zeros((B, MAP_RISK_FIELDS))
        step_hits, unknown = np.zeros((B, N), dtype=np.int32), np.zeros((B, N), dtype=np.int32)
        total = None if base is None else np.zeros(B)
        _check(lib().cilqr_rollout_risk_map(self._h, B, int(N), int(S), _p(X), _p(U), _p(k), _p(K), _p(delta), C.c_int64(stride),
                                            C.c_double(k_scale), C.c_double(occ_threshold),
                                            C.c_uint32(MAP_RISK_UNKNOWN_HITS if unknown_hits else 0), C.c_double(max_risk), _p(base),
                                            _p(risk), _p(step_hits, _ip), _p(unknown, _ip), _p(total)))
        return risk, step_hits, unknown, total

    def rollout_risk_map_device(self, stream, B, N, S, X, U, k, K, delta, delta_batch_stride, occ_threshold, risk, step_hits=0,
                                unknown_hits=0, total=0, base=0, k_scale=0.0, max_risk=1.0, flags=0):
        """`cilqr_rollout_risk_map_device`: device addresses; the map is the one set by `set_uncertainty_map(_device)`."""
        _check(lib().cilqr_rollout_risk_map_device(self._h, _vp(stream), int(B), int(N), int(S), _vp(X), _vp(U), _vp(k), _vp(K),
                                                   _vp(delta), C.c_int64(delta_batch_stride), C.c_double(k_scale),
                                                   C.c_double(occ_threshold), C.c_uint32(int(flags)), C.c_double(max_risk), _vp(base),
                                                   _vp(risk), _vp(step_hits), _vp(unknown_hits), _vp(total)))

    # ---- analytic pose-noise risk: closed-loop covariance chain and Gaussian chance values ----
    def chance_risk(self, N, X, U, K, sigma0, process_noise=None, obs_pose=None, obs_dim=None, max_risk=1.0, base=None, sum_bound=False,
                    want_entry_p=True, want_sigma=True):
        """`cilqr_chance_risk`: the state covariance along each plan under u = U_t + K_t (x - X_t), from sigma0 — (4, 4) or (16,)
        shared by the solves, or (B, 4, 4) / (B, 16) one per solve, column-major, only row <= column read — and process noise W (4, 4)
        or None, and from it the Gaussian chance of each obstacle entry; obstacles in any shape of `obstacle_strides`.  Returns
        dict(risk (B, CHANCE_FIELDS), step_risk (B, N), entry_p (B, M*N) or None, sigma (B, N+1, 16) or None, total): total[b] is
        base[b], NaN where CR_STEP_RISK (CR_SUM_RISK with sum_bound) exceeds max_risk or base[b] is not finite; None without `base`."""
        X = _np64(X)
        B = X.size // (4 * (N + 1))
        X = X.reshape(B, 4 * (N + 1))
        U, K = _np64(U).reshape(B, 2 * N), _np64(K).reshape(B, 8 * N)
        sigma0 = _np64(sigma0)
        if sigma0.size == 16:
            sigma0, stride = sigma0.reshape(16), 0
        elif sigma0.size == 16 * B:
            sigma0, stride = sigma0.reshape(B, 16), 1
        else:
            raise CilqrError("chance_risk: sigma0 %s holds neither 16 nor %d x 16 values" % (sigma0.shape, B))
        W = None if process_noise is None else _np64(process_noise).reshape(16)
        M, obs, keep = self._obstacles(obs_pose, obs_dim, None, B, N)
        base = None if base is None else _np64(base).reshape(B)
        risk, step_risk = np.zeros((B, CHANCE_FIELDS)), np.zeros((B, N))
        entry_p = np.zeros((B, M * N)) if want_entry_p else None
        sigma = np.zeros((B, N + 1, 16)) if want_sigma else None
        total = None if base is None else np.zeros(B)
        _check(lib().cilqr_chance_risk(self._h, B, int(N), int(M), _p(X), _p(U), _p(K), _p(sigma0), C.c_int64(stride), _p(W),
                                       None if obs is None else C.byref(obs), C.c_uint32(CHANCE_BOUND_SUM if sum_bound else 0),
                                       C.c_double(max_risk), _p(base), _p(risk), _p(step_risk), _p(entry_p), _p(sigma), _p(total)))
        return dict(risk=risk, step_risk=step_risk, entry_p=entry_p, sigma=sigma, total=total)

    def chance_risk_device(self, stream, B, N, M, X, U, K, sigma0, sigma0_batch_stride, process_noise, obs_pose, obs_dim, strides, risk,
                           step_risk=0, entry_p=0, sigma_out=0, total=0, base=0, max_risk=1.0, flags=0):
        """`cilqr_chance_risk_device`: device addresses; strides (batch, obstacle, step, weight batch) as `score_batch_device`."""
        bs, ms, ts, wbs = (int(v) for v in strides)
        obs = Obstacles(int(obs_pose) if obs_pose else None, int(obs_dim) if obs_dim else None, None, bs, ms, ts, wbs)
        _check(lib().cilqr_chance_risk_device(self._h, _vp(stream), int(B), int(N), int(M), _vp(X), _vp(U), _vp(K), _vp(sigma0),
                                              C.c_int64(sigma0_batch_stride), _vp(process_noise), C.byref(obs) if M else None,
                                              C.c_uint32(int(flags)), C.c_double(max_risk), _vp(base), _vp(risk), _vp(step_risk),
                                              _vp(entry_p), _vp(sigma_out), _vp(total)))

    def chance_risk_cov(self, N, X, U, K, sigma0, process_noise=None, obs_pose=None, obs_dim=None, obs_cov=None, max_risk=1.0, base=None,
                        sum_bound=False, want_entry_p=True, want_sigma=True):
        """`cilqr_chance_risk_cov`: `chance_risk` with the obstacles' own position covariance, obs_cov None or (xx, xy, yy) per
        obstacle entry in the obstacles' own shape with 3 (or 3N) columns — what `predict_obstacles` returns as `cov`.  Same returns."""
        X = _np64(X)
        B = X.size // (4 * (N + 1))
        X = X.reshape(B, 4 * (N + 1))
        U, K = _np64(U).reshape(B, 2 * N), _np64(K).reshape(B, 8 * N)
        sigma0 = _np64(sigma0)
        if sigma0.size == 16:
            sigma0, stride = sigma0.reshape(16), 0
        elif sigma0.size == 16 * B:
            sigma0, stride = sigma0.reshape(B, 16), 1
        else:
            raise CilqrError("chance_risk_cov: sigma0 %s holds neither 16 nor %d x 16 values" % (sigma0.shape, B))
        W = None if process_noise is None else _np64(process_noise).reshape(16)
        M, obs, keep = self._obstacles(obs_pose, obs_dim, None, B, N)
        obs_cov = None if obs_cov is None or M == 0 else _np64(obs_cov)
        if obs_cov is not None and obs_cov.size * 4 != keep[0].size * 3:
            raise CilqrError("chance_risk_cov: obs_cov %s does not hold 3 values per entry of obs_pose %s" % (obs_cov.shape, keep[0].shape))
        base = None if base is None else _np64(base).reshape(B)
        risk, step_risk = np.zeros((B, CHANCE_FIELDS)), np.zeros((B, N))
        entry_p = np.zeros((B, M * N)) if want_entry_p else None
        sigma = np.zeros((B, N + 1, 16)) if want_sigma else None
        total = None if base is None else np.zeros(B)
        _check(lib().cilqr_chance_risk_cov(self._h, B, int(N), int(M), _p(X), _p(U), _p(K), _p(sigma0), C.c_int64(stride), _p(W),
                                           None if obs is None else C.byref(obs), _p(obs_cov),
                                           C.c_uint32(CHANCE_BOUND_SUM if sum_bound else 0), C.c_double(max_risk), _p(base), _p(risk),
                                           _p(step_risk), _p(entry_p), _p(sigma), _p(total)))
        return dict(risk=risk, step_risk=step_risk, entry_p=entry_p, sigma=sigma, total=total)

    def chance_risk_cov_device(self, stream, B, N, M, X, U, K, sigma0, sigma0_batch_stride, process_noise, obs_pose, obs_dim, strides,
                               obs_cov, risk, step_risk=0, entry_p=0, sigma_out=0, total=0, base=0, max_risk=1.0, flags=0):
        """`cilqr_chance_risk_cov_device`: device addresses; obs_cov 0 or 3 doubles per entry, addressed by the strides' entry index."""
        bs, ms, ts, wbs = (int(v) for v in strides)
        obs = Obstacles(int(obs_pose) if obs_pose else None, int(obs_dim) if obs_dim else None, None, bs, ms, ts, wbs)
        _check(lib().cilqr_chance_risk_cov_device(self._h, _vp(stream), int(B), int(N), int(M), _vp(X), _vp(U), _vp(K), _vp(sigma0),
                                                  C.c_int64(sigma0_batch_stride), _vp(process_noise), C.byref(obs) if M else None,
                                                  _vp(obs_cov), C.c_uint32(int(flags)), C.c_double(max_risk), _vp(base), _vp(risk),
                                                  _vp(step_risk), _vp(entry_p), _vp(sigma_out), _vp(total)))

    # ---- tracked obstacles predicted over the horizon, with their covariance ----
    def predict_obstacles(self, N, track, track_dim, track_cov=None, track_noise=None, want_cov=True, want_sigma=True):
        """`cilqr_predict_obstacles`: track (M, 6) — one set for every solve — or (T, M, 6), rows (x, y, v, theta, a, omega);
        track_dim the same shape with 2 columns; track_cov None or the same shape with 16 (or 4, 4) per track, column-major, only
        row <= column read; track_noise None or 16 values.  Returns dict(pose (…, M, 4N), dim (…, M, 2N), cov (…, M, 3N) or None,
        sigma (…, M, N, 16) or None): pose, dim and cov in a shape `obstacle_strides` and the obs_cov arguments take as they are."""
        track = _np64(track)
        lead = track.shape[:-1]
        if track.ndim not in (2, 3) or track.shape[-1] != 6:
            raise CilqrError("predict_obstacles: track %s is not (M, 6) or (T, M, 6)" % (track.shape,))
        T, M = (1, lead[0]) if len(lead) == 1 else lead
        track_dim = _np64(track_dim)
        if track_dim.size != T * M * 2:
            raise CilqrError("predict_obstacles: track_dim %s does not hold 2 values per track" % (track_dim.shape,))
        track_cov = None if track_cov is None else _np64(track_cov)
        if track_cov is not None and track_cov.size != T * M * 16:
            raise CilqrError("predict_obstacles: track_cov %s does not hold 16 values per track" % (track_cov.shape,))
        Q = None if track_noise is None else _np64(track_noise).reshape(16)
        pose, dim = np.zeros(lead + (4 * N,)), np.zeros(lead + (2 * N,))
        cov = np.zeros(lead + (3 * N,)) if want_cov else None
        sigma = np.zeros(lead + (N, 16)) if want_sigma else None
        _check(lib().cilqr_predict_obstacles(self._h, int(T), int(N), int(M), _p(track), _p(track_dim), _p(track_cov), _p(Q), _p(pose),
                                             _p(dim), _p(cov), _p(sigma)))
        return dict(pose=pose, dim=dim, cov=cov, sigma=sigma)

    def predict_obstacles_device(self, stream, T, N, M, track, track_dim, pose_out, dim_out, track_cov=0, track_noise=0, cov_out=0,
                                 sigma_out=0):
        """`cilqr_predict_obstacles_device`: device addresses."""
        _check(lib().cilqr_predict_obstacles_device(self._h, _vp(stream), int(T), int(N), int(M), _vp(track), _vp(track_dim),
                                                    _vp(track_cov), _vp(track_noise), _vp(pose_out), _vp(dim_out), _vp(cov_out),
                                                    _vp(sigma_out)))

    # ---- analytic map risk: the pose covariance against the uncertainty map by quadrature ----
    def chance_risk_map(self, N, X, sigma, nodes, weights, occ_threshold, max_risk=1.0, base=None, sum_bound=False, unknown_hits=False,
                        want_steps=True):
        """`cilqr_chance_risk_map`: sigma (B, N+1, 16) as `chance_risk` returns it; nodes (Q, 3) and weights (Q,) as
        `pose_quadrature` builds them (any weighted standard-normal set serves).  Returns dict(risk (B, CHANCE_MAP_FIELDS), step_risk,
        step_occ, step_unknown (B, N) each or None, total): total[b] is base[b], NaN where CM_STEP_RISK (CM_SUM_RISK with sum_bound)
        exceeds max_risk or base[b] is not finite; None without `base`."""
        X = _np64(X)
        B = X.size // (4 * (N + 1))
        X, sigma = X.reshape(B, 4 * (N + 1)), _np64(sigma).reshape(B, N + 1, 16)
        nodes, weights = _np64(nodes).reshape(-1, 3), _np64(weights).reshape(-1)
        if nodes.shape[0] != weights.shape[0]:
            raise CilqrError("chance_risk_map: %d nodes but %d weights" % (nodes.shape[0], weights.shape[0]))
        base = None if base is None else _np64(base).reshape(B)
        risk = np.zeros((B, CHANCE_MAP_FIELDS))
        step_risk, step_occ, step_unknown = (np.zeros((B, N)) if want_steps else None for _ in range(3))
        total = None if base is None else np.zeros(B)
        flags = (CHANCE_MAP_UNKNOWN_HITS if unknown_hits else 0) | (CHANCE_MAP_BOUND_SUM if sum_bound else 0)
        _check(lib().cilqr_chance_risk_map(self._h, B, int(N), int(weights.shape[0]), _p(X), _p(sigma), _p(nodes), _p(weights),
                                           C.c_double(occ_threshold), C.c_uint32(flags), C.c_double(max_risk), _p(base), _p(risk),
                                           _p(step_risk), _p(step_occ), _p(step_unknown), _p(total)))
        return dict(risk=risk, step_risk=step_risk, step_occ=step_occ, step_unknown=step_unknown, total=total)

    def chance_risk_map_device(self, stream, B, N, Q, X, sigma, nodes, weights, occ_threshold, risk, step_risk=0, step_occ=0,
                               step_unknown=0, total=0, base=0, max_risk=1.0, flags=0):
        """`cilqr_chance_risk_map_device`: device addresses; the map is the one set by `set_uncertainty_map(_device)`."""
        _check(lib().cilqr_chance_risk_map_device(self._h, _vp(stream), int(B), int(N), int(Q), _vp(X), _vp(sigma), _vp(nodes),
                                                  _vp(weights), C.c_double(occ_threshold), C.c_uint32(int(flags)), C.c_double(max_risk),
                                                  _vp(base), _vp(risk), _vp(step_risk), _vp(step_occ), _vp(step_unknown), _vp(total)))

    # ---- analytic chance risk against sampled obstacles in compact form ----
    def chance_risk_sampled(self, N, X, sigma, nom_pose, nom_dim, offsets, max_risk=1.0, base=None, sum_bound=False, want_steps=True,
                            want_pair_p=True, want_entry_p=True):
        """`cilqr_chance_risk_sampled`: sigma (B, N+1, 16) as `chance_risk` returns it (its call without obstacles supplies it);
        nom_pose, nom_dim, offsets as `solve_batch_sampled`.  Returns dict(risk (B, CRS_FIELDS), step_risk (B, N), pair_p
        (B, n_obs, N), entry_p (B, n_obs*n_samples, N), each or None, total): total[b] is base[b], NaN where CRS_STEP_RISK
        (CRS_SUM_RISK with sum_bound) exceeds max_risk or base[b] is not finite; None without `base`."""
        offsets = _np64(offsets)
        B, n_obs, ns = offsets.shape[0], offsets.shape[1], offsets.shape[2]
        X, sigma = _np64(X).reshape(B, 4 * (N + 1)), _np64(sigma).reshape(B, N + 1, 16)
        nom_pose = _np64(nom_pose).reshape(B, n_obs, 4 * N)
        nom_dim = _np64(nom_dim).reshape(B, n_obs, 2 * N)
        offsets = offsets.reshape(B, n_obs, ns, 3)
        base = None if base is None else _np64(base).reshape(B)
        risk = np.zeros((B, CRS_FIELDS))
        step_risk = np.zeros((B, N)) if want_steps else None
        pair_p = np.zeros((B, n_obs, N)) if want_pair_p else None
        entry_p = np.zeros((B, n_obs * ns, N)) if want_entry_p else None
        total = None if base is None else np.zeros(B)
        _check(lib().cilqr_chance_risk_sampled(self._h, B, int(N), int(n_obs), int(ns), _p(X), _p(sigma), _p(nom_pose), _p(nom_dim),
                                               _p(offsets), C.c_uint32(CHANCE_SAMPLED_BOUND_SUM if sum_bound else 0),
                                               C.c_double(max_risk), _p(base), _p(risk), _p(step_risk), _p(pair_p), _p(entry_p),
                                               _p(total)))
        return dict(risk=risk, step_risk=step_risk, pair_p=pair_p, entry_p=entry_p, total=total)

    def chance_risk_sampled_device(self, stream, B, N, n_obs, n_samples, X, sigma, nom_pose, nom_dim, offsets, risk, step_risk=0,
                                   pair_p=0, entry_p=0, total=0, base=0, max_risk=1.0, flags=0):
        """`cilqr_chance_risk_sampled_device`: device addresses."""
        _check(lib().cilqr_chance_risk_sampled_device(self._h, _vp(stream), int(B), int(N), int(n_obs), int(n_samples), _vp(X),
                                                      _vp(sigma), _vp(nom_pose), _vp(nom_dim), _vp(offsets), C.c_uint32(int(flags)),
                                                      C.c_double(max_risk), _vp(base), _vp(risk), _vp(step_risk), _vp(pair_p),
                                                      _vp(entry_p), _vp(total)))

    # ---- chance-constraint tightening: obstacles inflated by Sigma_t for a warm-started re-solve ----
    def tighten_obstacles(self, N, X, sigma, obs_pose=None, obs_dim=None, obs_cov=None, kappa=0.0, max_inflate=2.0, want_pose=True):
        """`cilqr_tighten_obstacles`: sigma (B, N+1, 16) as `chance_risk` returns it; obstacles in any shape of `obstacle_strides`;
        obs_cov None or (xx, xy, yy) per obstacle entry in the obstacles' own shape with 3 (or 3N) columns.  Returns dict(dim (B, M, 2N),
        pose (B, M, 4N) or None, tighten (B, TIGHTEN_FIELDS)): the dense table `solve_batch` re-solves against."""
        X = _np64(X)
        B = X.size // (4 * (N + 1))
        X = X.reshape(B, 4 * (N + 1))
        sigma = _np64(sigma).reshape(B, N + 1, 16)
        M, obs, keep = self._obstacles(obs_pose, obs_dim, None, B, N)
        obs_cov = None if obs_cov is None or M == 0 else _np64(obs_cov)
        if obs_cov is not None and obs_cov.size * 4 != keep[0].size * 3:
            raise CilqrError("tighten_obstacles: obs_cov %s does not hold 3 values per entry of obs_pose %s" % (obs_cov.shape, keep[0].shape))
        dim, tighten = np.zeros((B, M, 2 * N)), np.zeros((B, TIGHTEN_FIELDS))
        pose = np.zeros((B, M, 4 * N)) if want_pose else None
        _check(lib().cilqr_tighten_obstacles(self._h, B, int(N), int(M), _p(X), _p(sigma), None if obs is None else C.byref(obs),
                                             _p(obs_cov), C.c_double(kappa), C.c_double(max_inflate), _p(pose), _p(dim), _p(tighten)))
        return dict(dim=dim, pose=pose, tighten=tighten)

    def tighten_obstacles_device(self, stream, B, N, M, X, sigma, obs_pose, obs_dim, strides, dim_out, tighten, pose_out=0, obs_cov=0,
                                 kappa=0.0, max_inflate=2.0):
        """`cilqr_tighten_obstacles_device`: device addresses; strides (batch, obstacle, step, weight batch) as `score_batch_device`."""
        bs, ms, ts, wbs = (int(v) for v in strides)
        obs = Obstacles(int(obs_pose) if obs_pose else None, int(obs_dim) if obs_dim else None, None, bs, ms, ts, wbs)
        _check(lib().cilqr_tighten_obstacles_device(self._h, _vp(stream), int(B), int(N), int(M), _vp(X), _vp(sigma),
                                                    C.byref(obs) if M else None, _vp(obs_cov), C.c_double(kappa), C.c_double(max_inflate),
                                                    _vp(pose_out), _vp(dim_out), _vp(tighten)))

    # ---- map tightening: the set uncertainty map dilated by Sigma_t for a warm-started re-solve ----
    def tighten_map(self, N, X, sigma, shape, kappa=0.0, max_inflate=1.0):
        """`cilqr_tighten_map`: sigma (B, N+1, 16) as `chance_risk` returns it; shape = (rows, cols) of the map set on the handle by
        `set_uncertainty_map(_device)`.  Returns dict(layer (B, rows, cols) float32, each layer Fortran-ordered like the input,
        tighten (B, TIGHTEN_MAP_FIELDS)).  The layers travel through the device arena: large batches take the device form."""
        X = _np64(X)
        B = X.size // (4 * (N + 1))
        X = X.reshape(B, 4 * (N + 1))
        sigma = _np64(sigma).reshape(B, N + 1, 16)
        rows, cols = int(shape[0]), int(shape[1])
        flat = np.zeros((B, rows * cols), dtype=np.float32)
        tighten = np.zeros((B, TIGHTEN_MAP_FIELDS))
        _check(lib().cilqr_tighten_map(self._h, B, int(N), _p(X), _p(sigma), C.c_double(kappa), C.c_double(max_inflate), _p(flat, _fp),
                                       _p(tighten)))
        return dict(layer=flat.reshape(B, cols, rows).transpose(0, 2, 1), tighten=tighten)

    def tighten_map_device(self, stream, B, N, X, sigma, layer_out, tighten, kappa=0.0, max_inflate=1.0):
        """`cilqr_tighten_map_device`: device addresses; layer_out (B, rows*cols) float32 feeds `set_uncertainty_map_device` with
        layer_stride = rows*cols."""
        _check(lib().cilqr_tighten_map_device(self._h, _vp(stream), int(B), int(N), _vp(X), _vp(sigma), C.c_double(kappa),
                                              C.c_double(max_inflate), _vp(layer_out), _vp(tighten)))

    # ---- predicted tracks rasterised into the set uncertainty map along each plan, for a warm-started re-solve ----
    def rasterize_tracks(self, N, shape, obs_pose, obs_dim, obs_cov=None, X=None, B=None, inflate=0.2, z_max=3.0, window=2,
                         bound_min=False):
        """`cilqr_rasterize_tracks`: tracks in any shape of `obstacle_strides` (what `predict_obstacles` returns serves as it is), obs_cov
        None or 3 values per entry in the tracks' own shape; X (B, 4(N+1)) the plans, or None with B given: swept mode; shape =
        (rows, cols) of the map set on the handle.  Returns dict(layer (B, rows, cols) float32, fields (B, TRACK_MAP_FIELDS)).  The
        layers travel through the device arena: large batches take the device form."""
        if X is not None:
            X = _np64(X)
            B = X.size // (4 * (N + 1))
            X = X.reshape(B, 4 * (N + 1))
        B = int(B)
        M, obs, keep = self._obstacles(obs_pose, obs_dim, None, B, N)
        obs_cov = None if obs_cov is None else _np64(obs_cov)
        if obs_cov is not None and obs_cov.size * 4 != keep[0].size * 3:
            raise CilqrError("rasterize_tracks: obs_cov %s does not hold 3 values per entry of obs_pose %s" % (obs_cov.shape, keep[0].shape))
        rows, cols = int(shape[0]), int(shape[1])
        flat = np.zeros((B, rows * cols), dtype=np.float32)
        fields = np.zeros((B, TRACK_MAP_FIELDS))
        _check(lib().cilqr_rasterize_tracks(self._h, B, int(N), int(M), _p(X), None if obs is None else C.byref(obs), _p(obs_cov),
                                            C.c_double(inflate), C.c_double(z_max), int(window),
                                            C.c_uint32(TRACK_MAP_BOUND_MIN if bound_min else 0), _p(flat, _fp), _p(fields)))
        return dict(layer=flat.reshape(B, cols, rows).transpose(0, 2, 1), fields=fields)

    def rasterize_tracks_device(self, stream, B, N, M, X, obs_pose, obs_dim, strides, layer_out, fields, obs_cov=0, inflate=0.2,
                                z_max=3.0, window=2, flags=0):
        """`cilqr_rasterize_tracks_device`: device addresses; X 0: swept mode; strides (batch, obstacle, step, weight batch) as
        `score_batch_device`; layer_out (B, rows*cols) float32 feeds `set_uncertainty_map_device` with layer_stride = rows*cols."""
        bs, ms, ts, wbs = (int(v) for v in strides)
        obs = Obstacles(int(obs_pose) if obs_pose else None, int(obs_dim) if obs_dim else None, None, bs, ms, ts, wbs)
        _check(lib().cilqr_rasterize_tracks_device(self._h, _vp(stream), int(B), int(N), int(M), _vp(X), C.byref(obs), _vp(obs_cov),
                                                   C.c_double(inflate), C.c_double(z_max), int(window), C.c_uint32(int(flags)),
                                                   _vp(layer_out), _vp(fields)))

    def footprint_check(self, N, X, obs_pose=None, obs_dim=None, S=1, margin=0.0, min_clearance=0.0, occ_threshold=float("inf"),
                        base=None, unknown_hits=False, skip_map=False, steps=True):
        """`cilqr_footprint_check`: X (B*S, 4(N+1)) rows, row r of solve r // S; obstacles in any shape of `obstacle_strides` for the B
        solves, or None.  Returns dict(fp (B*S, FOOTPRINT_FIELDS), step_clearance (B*S, N), step_occ (B*S, N) float32 — both None
        with steps=False — and total (B*S,), None without base)."""
        X = _np64(X)
        R = X.size // (4 * (N + 1))
        X = X.reshape(R, 4 * (N + 1))
        S = int(S)
        if S < 1 or R % S:
            raise CilqrError("footprint_check: %d rows are no multiple of S = %d" % (R, S))
        B = R // S
        M, obs, keep = self._obstacles(obs_pose, obs_dim, None, B, N)
        base = None if base is None else _np64(base).reshape(R)
        fp = np.zeros((R, FOOTPRINT_FIELDS))
        step_clearance = np.zeros((R, N)) if steps else None
        step_occ = np.zeros((R, N), dtype=np.float32) if steps else None
        total = None if base is None else np.zeros(R)
        flags = (FOOTPRINT_UNKNOWN_HITS if unknown_hits else 0) | (FOOTPRINT_SKIP_MAP if skip_map else 0)
        _check(lib().cilqr_footprint_check(self._h, B, int(N), int(M), S, _p(X), None if obs is None else C.byref(obs),
                                           C.c_double(margin), C.c_double(min_clearance), C.c_double(occ_threshold),
                                           C.c_uint32(flags), _p(base), _p(fp), _p(step_clearance), _p(step_occ, _fp), _p(total)))
        return dict(fp=fp, step_clearance=step_clearance, step_occ=step_occ, total=total)

    def footprint_check_device(self, stream, B, N, M, S, X, obs_pose, obs_dim, strides, fp, margin=0.0, min_clearance=0.0,
                               occ_threshold=float("inf"), flags=0, base=0, step_clearance=0, step_occ=0, total=0):
        """`cilqr_footprint_check_device`: device addresses; strides (batch, obstacle, step, weight batch) as `score_batch_device`;
        the map is the one set by `set_uncertainty_map(_device)`."""
        bs, ms, ts, wbs = (int(v) for v in strides)
        obs = Obstacles(int(obs_pose) if obs_pose else None, int(obs_dim) if obs_dim else None, None, bs, ms, ts, wbs)
        _check(lib().cilqr_footprint_check_device(self._h, _vp(stream), int(B), int(N), int(M), int(S), _vp(X),
                                                  C.byref(obs) if M else None, C.c_double(margin), C.c_double(min_clearance),
                                                  C.c_double(occ_threshold), C.c_uint32(int(flags)), _vp(base), _vp(fp),
                                                  _vp(step_clearance), _vp(step_occ), _vp(total)))

    # ---- distance to the occupied cells of a layer: exact field, inflation, clearance of the ego rectangle ----
    @staticmethod
    def _layers(layers, geom):
        """(rows, cols) or (L, rows, cols) float32 -> (flat (L, rows*cols) column-major per layer, L)."""
        a = np.asarray(layers, dtype=np.float32)
        if a.ndim == 2:
            a = a[None]
        if a.ndim != 3 or a.shape[1:] != (geom.rows, geom.cols):
            raise CilqrError("layers %s are not (L, %d, %d)" % (a.shape, geom.rows, geom.cols))
        return np.ascontiguousarray(a.transpose(0, 2, 1)).reshape(a.shape[0], -1), int(a.shape[0])

    def map_distance(self, layers, geom, occ_threshold, unknown_seeds=False, to_free=False, L=None, want_dist=True):
        """`cilqr_map_distance`: layers (rows, cols) or (L, rows, cols) float32; one (rows, cols) layer with L given: the shared layer
        (layer_stride 0), its result written L times.  Returns dict(d2 (L, rows, cols) int32 — MAP_DISTANCE_NONE where the layer has
        no seed — and dist (L, rows, cols) float32 in metres, None with want_dist=False).  The layers travel through the device
        arena: large maps and batches take the device form."""
        flat, n = self._layers(layers, geom)
        stride = flat.shape[1]
        if L is not None:
            if n != 1:
                raise CilqrError("map_distance: L is given for ONE shared layer, not %d" % n)
            n, stride = int(L), 0
        d2 = np.zeros((n, flat.shape[1]), dtype=np.int32)
        dist = np.zeros((n, flat.shape[1]), dtype=np.float32) if want_dist else None
        flags = (MAP_DISTANCE_UNKNOWN_SEEDS if unknown_seeds else 0) | (MAP_DISTANCE_TO_FREE if to_free else 0)
        _check(lib().cilqr_map_distance(self._h, n, _p(flat, _fp), C.c_int64(stride), C.byref(geom), C.c_double(occ_threshold),
                                        C.c_uint32(flags), _p(d2, _ip), _p(dist, _fp)))
        shape = lambda a: None if a is None else a.reshape(n, geom.cols, geom.rows).transpose(0, 2, 1)
        return dict(d2=shape(d2), dist=shape(dist))

    def map_distance_device(self, stream, L, layer, layer_stride, geom, occ_threshold, d2_out, dist_out=0, flags=0):
        """`cilqr_map_distance_device`: device addresses; d2_out (L, rows*cols) int32, dist_out (L, rows*cols) float32 or 0."""
        _check(lib().cilqr_map_distance_device(self._h, _vp(stream), int(L), _vp(layer), C.c_int64(int(layer_stride)), C.byref(geom),
                                               C.c_double(occ_threshold), C.c_uint32(int(flags)), _vp(d2_out), _vp(dist_out)))

    def inflate_map(self, layers, geom, d2, inscribed, radius, peak=100.0, L=None):
        """`cilqr_inflate_map`: layers as `map_distance` takes them, d2 (L, rows, cols) int32 as it returns it.  Returns the inflated
        layers (L, rows, cols) float32."""
        flat, n = self._layers(layers, geom)
        stride = flat.shape[1]
        if L is not None:
            if n != 1:
                raise CilqrError("inflate_map: L is given for ONE shared layer, not %d" % n)
            n, stride = int(L), 0
        d2 = np.asarray(d2, dtype=np.int32)
        if d2.ndim == 2:
            d2 = d2[None]
        if d2.shape != (n, geom.rows, geom.cols):
            raise CilqrError("inflate_map: d2 %s is not (%d, %d, %d)" % (d2.shape, n, geom.rows, geom.cols))
        d2 = np.ascontiguousarray(d2.transpose(0, 2, 1)).reshape(n, -1)
        out = np.zeros((n, flat.shape[1]), dtype=np.float32)
        _check(lib().cilqr_inflate_map(self._h, n, _p(flat, _fp), C.c_int64(stride), C.byref(geom), _p(d2, _ip), C.c_double(inscribed),
                                       C.c_double(radius), C.c_double(peak), _p(out, _fp)))
        return out.reshape(n, geom.cols, geom.rows).transpose(0, 2, 1)

    def inflate_map_device(self, stream, L, layer, layer_stride, geom, d2, inscribed, radius, peak, layer_out):
        """`cilqr_inflate_map_device`: device addresses; layer_out (L, rows*cols) float32 feeds `set_uncertainty_map_device` with
        layer_stride = rows*cols."""
        _check(lib().cilqr_inflate_map_device(self._h, _vp(stream), int(L), _vp(layer), C.c_int64(int(layer_stride)), C.byref(geom),
                                              _vp(d2), C.c_double(inscribed), C.c_double(radius), C.c_double(peak), _vp(layer_out)))

    def map_obstacles(self, d2, geom, K, gap2=0, four=False, pose=None, min_cells=1, max_size=float("inf"), pad=0.0, tables=True):
        """`cilqr_map_obstacles`: d2 (rows, cols) or (L, rows, cols) int32 as `map_distance` returns it; pose None, (3,) for every
        layer or (L, 3).  Returns dict(label (L, rows, cols) int32, n (L, 4) int32 = found, of min_cells, rows written, seeds; comp
        (L, K, MAP_OBSTACLE_FIELDS); boxes (L, K, 5), pose (L, K, 4) and dim (L, K, 2), None with tables=False).  Rows at and beyond
        n[l, 2] are filler.  The arrays travel through the device arena: large maps and batches take the device form."""
        d2 = np.asarray(d2, dtype=np.int32)
        if d2.ndim == 2:
            d2 = d2[None]
        if d2.ndim != 3 or d2.shape[1:] != (geom.rows, geom.cols):
            raise CilqrError("map_obstacles: d2 %s is not (L, %d, %d)" % (d2.shape, geom.rows, geom.cols))
        n, K = int(d2.shape[0]), int(K)
        flat = np.ascontiguousarray(d2.transpose(0, 2, 1)).reshape(n, -1)
        stride = 0
        if pose is not None:
            pose = _np64(pose)
            if pose.shape not in ((3,), (n, 3)):
                raise CilqrError("map_obstacles: pose %s is neither (3,) nor (%d, 3)" % (pose.shape, n))
            stride = 3 if pose.ndim == 2 else 0
        work, label = np.zeros_like(flat), np.zeros_like(flat)
        counts = np.zeros((n, 4), dtype=np.int32)
        rows = max(K, 1)
        comp = np.zeros((n, rows, MAP_OBSTACLE_FIELDS))
        boxes, pose_out, dim_out = (np.zeros((n, rows, w)) if tables else None for w in (5, 4, 2))
        _check(lib().cilqr_map_obstacles(self._h, n, _p(flat, _ip), C.byref(geom), int(gap2), C.c_uint32(MAP_OBSTACLES_FOUR if four else 0),
                                         _p(pose), stride, K, int(min_cells), C.c_double(max_size), C.c_double(pad), _p(work, _ip),
                                         _p(label, _ip), _p(counts, _ip), _p(comp), _p(boxes), _p(pose_out), _p(dim_out)))
        return dict(label=label.reshape(n, geom.cols, geom.rows).transpose(0, 2, 1), n=counts, comp=comp, boxes=boxes, pose=pose_out,
                    dim=dim_out)

    def map_obstacles_device(self, stream, L, d2, geom, K, work, label_out, n_out, comp, boxes=0, pose_out=0, dim_out=0, gap2=0, flags=0,
                             pose=0, pose_stride=0, min_cells=1, max_size=float("inf"), pad=0.0):
        """`cilqr_map_obstacles_device`: device addresses; d2, work and label_out (L, rows*cols) int32, n_out (L, 4) int32, comp
        (L, K, MAP_OBSTACLE_FIELDS), boxes (L, K, 5), pose_out (L, K, 4) and dim_out (L, K, 2) float64 or 0; pose (L or 1, 3) or 0.
        pose_out / dim_out feed `solve_batch_obstacles_device` with strides (K, 1, 0, 0), M = K."""
        _check(lib().cilqr_map_obstacles_device(self._h, _vp(stream), int(L), _vp(d2), C.byref(geom), int(gap2), C.c_uint32(int(flags)),
                                                _vp(pose), int(pose_stride), int(K), int(min_cells), C.c_double(max_size), C.c_double(pad),
                                                _vp(work), _vp(label_out), _vp(n_out), _vp(comp), _vp(boxes), _vp(pose_out), _vp(dim_out)))

    # ---- map obstacles tracked across ticks ----
    def track_update(self, det, filt, state=None, world=None, n_det=None, reset=False, M=None):
        """`cilqr_track_update`: det (D, 5) or (W, D, 5) rows (x, y, yaw, size_x, size_y), as `map_obstacles` returns `boxes`; filt a
        `TrackFilter`; state (…, M, TRACK_STATE) and world (…, TRACK_WORLD_FIELDS) as the last call returned them, or reset=True with M
        slots for a first tick; n_det None or one count per world.  Returns dict(state, world, assign (…, D) int32, track (…, M, 6),
        dim (…, M, 2), cov (…, M, 16)): track, dim and cov are what `predict_obstacles` takes."""
        det = _np64(det)
        if det.ndim not in (2, 3) or det.shape[-1] != 5:
            raise CilqrError("track_update: det %s is not (D, 5) or (W, D, 5)" % (det.shape,))
        lead = det.shape[:-2]
        W, D = (1 if not lead else lead[0]), det.shape[-2]
        if reset:
            if M is None and state is not None:
                M = np.asarray(state).shape[-2]
            if M is None:
                raise CilqrError("track_update: reset needs the number of slots M")
            state, world = np.zeros(lead + (int(M), TRACK_STATE)), np.zeros(lead + (TRACK_WORLD_FIELDS,))
        else:
            if state is None or world is None:
                raise CilqrError("track_update: state and world are needed without reset")
            state, world = _np64(state).copy(), _np64(world).copy()
            if state.ndim != len(lead) + 2 or state.shape[-1] != TRACK_STATE or state.shape[:-2] != lead:
                raise CilqrError("track_update: state %s is not %s + (M, %d)" % (state.shape, lead, TRACK_STATE))
            if world.shape != lead + (TRACK_WORLD_FIELDS,):
                raise CilqrError("track_update: world %s is not %s" % (world.shape, lead + (TRACK_WORLD_FIELDS,)))
        M = state.shape[-2]
        counts = None
        if n_det is not None:
            counts = np.ascontiguousarray(n_det, dtype=np.int32).reshape(-1)
            if counts.size != W:
                raise CilqrError("track_update: n_det holds %d counts for %d worlds" % (counts.size, W))
        assign = np.zeros(lead + (D,), dtype=np.int32)
        track, dim, cov = np.zeros(lead + (M, 6)), np.zeros(lead + (M, 2)), np.zeros(lead + (M, 16))
        _check(lib().cilqr_track_update(self._h, int(W), int(M), int(D), _p(det) if D else None, _p(counts, _ip), C.c_int64(1),
                                        C.byref(filt), _p(state), _p(state), _p(world), C.c_uint32(TRACK_RESET if reset else 0),
                                        _p(assign, _ip) if D else None, _p(track), _p(dim), _p(cov)))
        return dict(state=state, world=world, assign=assign, track=track, dim=dim, cov=cov)

    def track_update_device(self, stream, W, M, D, det, filt, state_in, state_out, world, track_out, dim_out, cov_out, n_det=0,
                            n_det_stride=1, assign=0, flags=0):
        """`cilqr_track_update_device`: device addresses; det (W, D, 5), state (W, M, TRACK_STATE) — state_in may equal state_out —,
        world (W, TRACK_WORLD_FIELDS), track_out (W, M, 6), dim_out (W, M, 2), cov_out (W, M, 16) float64; n_det int32 read at
        n_det[w*n_det_stride] or 0; assign (W, D) int32 or 0.  With n_det = n_out + 8 bytes and n_det_stride = 4 the counts are the
        "rows written" of `map_obstacles_device`."""
        _check(lib().cilqr_track_update_device(self._h, _vp(stream), int(W), int(M), int(D), _vp(det), _vp(n_det), C.c_int64(int(n_det_stride)),
                                               C.byref(filt), _vp(state_in), _vp(state_out), _vp(world), C.c_uint32(int(flags)),
                                               _vp(assign), _vp(track_out), _vp(dim_out), _vp(cov_out)))

    # ---- static layer: the cells of tracked movers taken out of the map ----
    def clear_movers(self, layers, geom, label, comp, halo2=0, fill=0.0, assign=None, state=None, min_hits=1, v_clear=0.0, mask=None,
                     L=None, want_owner=True):
        """`cilqr_clear_movers`: layers as `map_distance` takes them (one (rows, cols) layer with L given: the shared layer); label
        (L, rows, cols) int32 and comp (L, K, MAP_OBSTACLE_FIELDS) as `map_obstacles` returns them.  The movers come in ONE of two
        forms: assign (L, K) int32 and state (L, M, TRACK_STATE) as `track_update` returns them (W = L, D = K) with min_hits and
        v_clear, or mask (L, K) int32.  Returns dict(layer (L, rows, cols) float32, owner (L, rows, cols) int32 — None with
        want_owner=False — and fields (L, CLEAR_MOVERS_FIELDS)).  The arrays travel through the device arena: large maps and
        batches take the device form."""
        flat, n = self._layers(layers, geom)
        stride = flat.shape[1]
        if L is not None:
            if n != 1:
                raise CilqrError("clear_movers: L is given for ONE shared layer, not %d" % n)
            n, stride = int(L), 0
        label = np.asarray(label, dtype=np.int32)
        if label.ndim == 2:
            label = label[None]
        if label.shape != (n, geom.rows, geom.cols):
            raise CilqrError("clear_movers: label %s is not (%d, %d, %d)" % (label.shape, n, geom.rows, geom.cols))
        label = np.ascontiguousarray(label.transpose(0, 2, 1)).reshape(n, -1)
        comp = _np64(comp)
        if comp.ndim == 2:
            comp = comp[None]
        if comp.ndim != 3 or comp.shape[0] != n or comp.shape[2] != MAP_OBSTACLE_FIELDS:
            raise CilqrError("clear_movers: comp %s is not (%d, K, %d)" % (comp.shape, n, MAP_OBSTACLE_FIELDS))
        K, M = int(comp.shape[1]), 0

        def rows_of(a, name):
            a = np.ascontiguousarray(a, dtype=np.int32)
            a = a[None] if a.ndim == 1 else a
            if a.shape != (n, K):
                raise CilqrError("clear_movers: %s %s is not (%d, %d)" % (name, a.shape, n, K))
            return a

        if assign is not None:
            assign = rows_of(assign, "assign")
        if mask is not None:
            mask = rows_of(mask, "mask")
        if state is not None:
            state = _np64(state)
            state = state[None] if state.ndim == 2 else state
            if state.ndim != 3 or state.shape[0] != n or state.shape[2] != TRACK_STATE:
                raise CilqrError("clear_movers: state %s is not (%d, M, %d)" % (state.shape, n, TRACK_STATE))
            M = int(state.shape[1])
        out = np.zeros((n, flat.shape[1]), dtype=np.float32)
        owner = np.zeros((n, flat.shape[1]), dtype=np.int32) if want_owner else None
        fields = np.zeros((n, CLEAR_MOVERS_FIELDS))
        _check(lib().cilqr_clear_movers(self._h, n, _p(flat, _fp), C.c_int64(stride), C.byref(geom), _p(label, _ip), K, _p(comp), M,
                                        _p(assign, _ip), _p(state), int(min_hits), C.c_double(v_clear), _p(mask, _ip), int(halo2),
                                        C.c_float(fill), _p(out, _fp), _p(owner, _ip), _p(fields)))
        shape = lambda a: None if a is None else a.reshape(n, geom.cols, geom.rows).transpose(0, 2, 1)
        return dict(layer=shape(out), owner=shape(owner), fields=fields)

    def clear_movers_device(self, stream, L, layer, layer_stride, geom, label, K, comp, layer_out, fields, halo2=0, fill=0.0, M=0,
                            assign=0, state=0, min_hits=1, v_clear=0.0, mask=0, owner_out=0):
        """`cilqr_clear_movers_device`: device addresses; label and owner_out (L, rows*cols) int32, comp (L, K, MAP_OBSTACLE_FIELDS),
        assign / mask (L, K) int32, state (L, M, TRACK_STATE), layer_out (L, rows*cols) float32 — it may be `layer` itself when L == 1
        or layer_stride == rows*cols —, fields (L, CLEAR_MOVERS_FIELDS) float64.  layer_out feeds `set_uncertainty_map_device`."""
        _check(lib().cilqr_clear_movers_device(self._h, _vp(stream), int(L), _vp(layer), C.c_int64(int(layer_stride)), C.byref(geom),
                                               _vp(label), int(K), _vp(comp), int(M), _vp(assign), _vp(state), int(min_hits),
                                               C.c_double(v_clear), _vp(mask), int(halo2), C.c_float(fill), _vp(layer_out),
                                               _vp(owner_out), _vp(fields)))

    def map_clearance(self, N, X, reach, S=1, margin=0.0, occ_threshold=float("inf"), min_clearance=0.0, base=None,
                      unknown_seeds=False, steps=True):
        """`cilqr_map_clearance`: X (B*S, 4(N+1)) rows, row r of solve r // S, against the map set by `set_uncertainty_map(_device)`.
        Returns dict(mc (B*S, MAP_CLEARANCE_FIELDS), step_clearance (B*S, N) — None with steps=False — and total (B*S,), None
        without base)."""
        X = _np64(X)
        R = X.size // (4 * (N + 1))
        X = X.reshape(R, 4 * (N + 1))
        S = int(S)
        if S < 1 or R % S:
            raise CilqrError("map_clearance: %d rows are no multiple of S = %d" % (R, S))
        base = None if base is None else _np64(base).reshape(R)
        mc = np.zeros((R, MAP_CLEARANCE_FIELDS))
        step_clearance = np.zeros((R, N)) if steps else None
        total = None if base is None else np.zeros(R)
        _check(lib().cilqr_map_clearance(self._h, R // S, int(N), S, _p(X), C.c_double(margin), C.c_double(occ_threshold),
                                         C.c_double(reach), C.c_double(min_clearance),
                                         C.c_uint32(MAP_CLEARANCE_UNKNOWN_SEEDS if unknown_seeds else 0), _p(base), _p(mc),
                                         _p(step_clearance), _p(total)))
        return dict(mc=mc, step_clearance=step_clearance, total=total)

    def map_clearance_device(self, stream, B, N, S, X, mc, reach, margin=0.0, occ_threshold=float("inf"), min_clearance=0.0, flags=0,
                             base=0, step_clearance=0, total=0):
        """`cilqr_map_clearance_device`: device addresses; the map is the one set by `set_uncertainty_map(_device)`."""
        _check(lib().cilqr_map_clearance_device(self._h, _vp(stream), int(B), int(N), int(S), _vp(X), C.c_double(margin),
                                                C.c_double(occ_threshold), C.c_double(reach), C.c_double(min_clearance),
                                                C.c_uint32(int(flags)), _vp(base), _vp(mc), _vp(step_clearance), _vp(total)))

    # ---- stop plans: a solved plan's path under a braking profile ----
    def stop_plans(self, N, X, U, decel, hold=1, max_deviation=float("inf"), plan_cost=None, decel_weight=0.0, allow_moving=False,
                   want_cost=True):
        """`cilqr_stop_plans`: X (B, 4(N+1)), U (B, 2N) solved plans, decel (D,) braking levels in m/s^2.  Returns dict(X (B*D, 4(N+1)),
        U (B*D, 2N), sp (B*D, STOP_FIELDS) and cost (B*D,), None with want_cost=False); row b*D + l is plan b at level l, the row
        order `footprint_check` and `map_clearance` take with S = D.  B*D must not exceed max_batch."""
        X = _np64(X)
        B = X.size // (4 * (N + 1))
        X, U = X.reshape(B, 4 * (N + 1)), _np64(U).reshape(B, 2 * N)
        decel = _np64(decel).reshape(-1)
        D = decel.size
        plan_cost = None if plan_cost is None else _np64(plan_cost).reshape(B)
        Xs, Us, sp = np.zeros((B * D, 4 * (N + 1))), np.zeros((B * D, 2 * N)), np.zeros((B * D, STOP_FIELDS))
        cost = np.zeros(B * D) if want_cost else None
        _check(lib().cilqr_stop_plans(self._h, B, int(N), int(D), _p(X), _p(U), _p(decel), int(hold), C.c_double(max_deviation),
                                      _p(plan_cost), C.c_double(decel_weight), C.c_uint32(STOP_ALLOW_MOVING if allow_moving else 0),
                                      _p(Xs), _p(Us), _p(sp), _p(cost)))
        return dict(X=Xs, U=Us, sp=sp, cost=cost)

    def stop_plans_device(self, stream, B, N, D, X, U, decel, X_stop, U_stop, sp, hold=1, max_deviation=float("inf"), plan_cost=0,
                          decel_weight=0.0, flags=0, cost=0):
        """`cilqr_stop_plans_device`: device addresses; X_stop (B*D, 4(N+1)), U_stop (B*D, 2N), sp (B*D, STOP_FIELDS), cost (B*D,) or 0."""
        _check(lib().cilqr_stop_plans_device(self._h, _vp(stream), int(B), int(N), int(D), _vp(X), _vp(U), _vp(decel), int(hold),
                                             C.c_double(max_deviation), _vp(plan_cost), C.c_double(decel_weight), C.c_uint32(int(flags)),
                                             _vp(X_stop), _vp(U_stop), _vp(sp), _vp(cost)))

    # ---- batched LocalPlanner pre-step on the device ----
    def local_plan_batch(self, path, ego):
        """path: (P, 2) shared by all candidates, or (B, P, 2) one per candidate; ego: (B, 4).
        Returns dict(poly (B,6), xplan_fl (B,2), ref_traj (B, W, 2), n (B,))."""
        ego = _np64(ego).reshape(-1, 4)
        B = ego.shape[0]
        path = _np64(path)
        if path.ndim == 3:
            if path.shape[0] != B:
                raise CilqrError("local_plan_batch: path batch dimension does not match ego")
            P, stride = path.shape[1], 2 * path.shape[1]
        else:
            path = path.reshape(-1, 2)
            P, stride = path.shape[0], 0
        W = self.params.num_of_local_wpts
        poly = np.zeros((B, POLY))
        fl = np.zeros((B, 2))
        ref = np.zeros((B, W, 2))
        n = np.zeros(B, dtype=np.int32)
        _check(lib().cilqr_local_plan_batch(self._h, B, int(P), _p(path), C.c_int64(stride), _p(ego), _p(poly), _p(fl), _p(ref),
                                            _p(n, _ip)))
        return dict(poly=poly, xplan_fl=fl, ref_traj=ref, n=n)

    def local_plan_batch_device(self, stream, B, P, path, path_stride, ego, poly, xplan_fl, ref_traj=0, n_out=0):
        _check(lib().cilqr_local_plan_batch_device(self._h, _vp(stream), int(B), int(P), _vp(path), C.c_int64(path_stride), _vp(ego),
                                                   _vp(poly), _vp(xplan_fl), _vp(ref_traj), _vp(n_out)))

    # ---- the pre-step and its surroundings in a path-aligned planning frame ----
    def local_plan_frames(self, path, ego):
        """`cilqr_local_plan_frames`: path and ego as `local_plan_batch`.  Returns dict(frames (B, 5) = (ox, oy, c, s, phi), info (B,),
        ego (B, 4) in the frame, poly (B, 6), xplan_fl (B, 2) and ref_traj (B, W, 2) in frame coordinates, n (B,), first (B,))."""
        ego = _np64(ego).reshape(-1, 4)
        B = ego.shape[0]
        path = _np64(path)
        if path.ndim == 3:
            if path.shape[0] != B:
                raise CilqrError("local_plan_frames: path batch dimension does not match ego")
            P, stride = path.shape[1], 2 * path.shape[1]
        else:
            path = path.reshape(-1, 2)
            P, stride = path.shape[0], 0
        W = self.params.num_of_local_wpts
        frames, info, ego_out = np.zeros((B, FRAME_DOUBLES)), np.zeros(B, dtype=np.int32), np.zeros((B, 4))
        poly, fl, ref = np.zeros((B, POLY)), np.zeros((B, 2)), np.zeros((B, W, 2))
        n, first = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
        _check(lib().cilqr_local_plan_frames(self._h, B, int(P), _p(path), C.c_int64(stride), _p(ego), _p(frames), _p(info, _ip),
                                             _p(ego_out), _p(poly), _p(fl), _p(ref), _p(n, _ip), _p(first, _ip)))
        return dict(frames=frames, info=info, ego=ego_out, poly=poly, xplan_fl=fl, ref_traj=ref, n=n, first=first)

    def local_plan_frames_device(self, stream, B, P, path, path_stride, ego, frames, info, ego_out, poly, xplan_fl, ref_traj=0,
                                 n_out=0, first_out=0):
        """`cilqr_local_plan_frames_device`: device addresses."""
        _check(lib().cilqr_local_plan_frames_device(self._h, _vp(stream), int(B), int(P), _vp(path), C.c_int64(path_stride), _vp(ego),
                                                    _vp(frames), _vp(info), _vp(ego_out), _vp(poly), _vp(xplan_fl), _vp(ref_traj),
                                                    _vp(n_out), _vp(first_out)))

    @staticmethod
    def _frame_stride(frames, B):
        frames = _np64(frames)
        if frames.size == FRAME_DOUBLES and frames.ndim == 1:
            return frames, 0
        if frames.shape != (B, FRAME_DOUBLES):
            raise CilqrError("frames %s are neither (%d,) nor (%d, %d)" % (frames.shape, FRAME_DOUBLES, B, FRAME_DOUBLES))
        return frames, FRAME_DOUBLES

    def frame_obstacles(self, B, N, frames, obs_pose, obs_dim, obs_cov=None, global_inflation=False):
        """`cilqr_frame_obstacles`: frames (B, 5), or (5,) one frame for the batch; obstacles in any shape of `obstacle_strides`;
        obs_cov None or (xx, xy, yy) per entry in the obstacles' own shape with 3 (or 3N) columns.  Returns dict(pose (B, M, 4N),
        dim (B, M, 2N), cov (B, M, 3N) or None): the dense table of `solve_batch` in each solve's frame."""
        frames, fs = self._frame_stride(frames, B)
        M, obs, keep = self._obstacles(obs_pose, obs_dim, None, B, N)
        obs_cov = None if obs_cov is None or M == 0 else _np64(obs_cov)
        if obs_cov is not None and obs_cov.size * 4 != keep[0].size * 3:
            raise CilqrError("frame_obstacles: obs_cov %s does not hold 3 values per entry of obs_pose %s" % (obs_cov.shape, keep[0].shape))
        pose, dim = np.zeros((B, M, 4 * N)), np.zeros((B, M, 2 * N))
        cov = None if obs_cov is None else np.zeros((B, M, 3 * N))
        _check(lib().cilqr_frame_obstacles(self._h, int(B), int(N), int(M), _p(frames), C.c_int64(fs), None if obs is None else C.byref(obs),
                                           _p(obs_cov), C.c_uint32(FRAME_GLOBAL_INFLATION if global_inflation else 0), _p(pose), _p(dim),
                                           _p(cov)))
        return dict(pose=pose, dim=dim, cov=cov)

    def frame_obstacles_device(self, stream, B, N, M, frames, frame_stride, obs_pose, obs_dim, strides, pose_out, dim_out, obs_cov=0,
                               cov_out=0, flags=0):
        """`cilqr_frame_obstacles_device`: device addresses; strides (batch, obstacle, step) in entries."""
        bs, ms, ts = (int(v) for v in tuple(strides)[:3])
        obs = Obstacles(int(obs_pose) if obs_pose else None, int(obs_dim) if obs_dim else None, None, bs, ms, ts, 0)
        _check(lib().cilqr_frame_obstacles_device(self._h, _vp(stream), int(B), int(N), int(M), _vp(frames), C.c_int64(frame_stride),
                                                  C.byref(obs) if M else None, _vp(obs_cov), C.c_uint32(int(flags)), _vp(pose_out),
                                                  _vp(dim_out), _vp(cov_out)))

    def frame_states(self, N, frames, X, direction=FRAME_FROM, S=1):
        """`cilqr_frame_states`: X (B*S, 4(N+1)) rows into (FRAME_TO) or out of (FRAME_FROM) the frame of solve row // S.  Returns the
        transformed rows."""
        X = _np64(X)
        rows = X.size // (4 * (N + 1))
        B = rows // int(S)
        X = X.reshape(rows, 4 * (N + 1))
        frames, fs = self._frame_stride(frames, B)
        out = np.zeros_like(X)
        _check(lib().cilqr_frame_states(self._h, int(B), int(S), int(N), _p(frames), C.c_int64(fs), int(direction), _p(X), _p(out)))
        return out

    def frame_states_device(self, stream, B, S, N, frames, frame_stride, direction, X_in, X_out):
        """`cilqr_frame_states_device`: device addresses; X_out may be X_in."""
        _check(lib().cilqr_frame_states_device(self._h, _vp(stream), int(B), int(S), int(N), _vp(frames), C.c_int64(frame_stride),
                                               int(direction), _vp(X_in), _vp(X_out)))

    def frame_poses(self, B, frames, poses):
        """`cilqr_frame_poses`: poses (K, 3) shared by the batch or (B, K, 3) → (B, K, 3) in each solve's frame."""
        poses = _np64(poses)
        if poses.ndim == 3:
            if poses.shape[0] != B or poses.shape[2] != 3:
                raise CilqrError("frame_poses: poses %s are not (%d, K, 3)" % (poses.shape, B))
            K, ps = poses.shape[1], 3 * poses.shape[1]
        else:
            poses = poses.reshape(-1, 3)
            K, ps = poses.shape[0], 0
        frames, fs = self._frame_stride(frames, B)
        out = np.zeros((B, K, 3))
        _check(lib().cilqr_frame_poses(self._h, int(B), int(K), _p(frames), C.c_int64(fs), _p(poses), C.c_int64(ps), _p(out)))
        return out

    def frame_poses_device(self, stream, B, K, frames, frame_stride, pose_in, pose_stride, pose_out):
        """`cilqr_frame_poses_device`: device addresses."""
        _check(lib().cilqr_frame_poses_device(self._h, _vp(stream), int(B), int(K), _vp(frames), C.c_int64(frame_stride), _vp(pose_in),
                                              C.c_int64(pose_stride), _vp(pose_out)))

    def argmin_device(self, stream, B, J, out_pair):
        _check(lib().cilqr_argmin_device(self._h, _vp(stream), int(B), _vp(J), _vp(out_pair)))

    # ---- costmap-lookup uncertainty cost (iLQR::set_uncertainty_map / clear_uncertainty_map) ----
    def set_uncertainty_map(self, layer, geom, pose=(0.0, 0.0, 0.0), probes=(3, 3)):
        """layer: (rows, cols) float32 host array (the blurred occupancy); copied into a device buffer the handle owns."""
        flat = np.ascontiguousarray(np.asfortranarray(layer, dtype=np.float32).flatten(order="F"))
        assert flat.size == geom.rows * geom.cols
        m = UncertaintyMap()
        m.layer = flat.ctypes.data
        m.geom = geom
        m.pose_x, m.pose_y, m.pose_theta = pose
        m.probes_l, m.probes_w = probes
        _check(lib().cilqr_set_uncertainty_map(self._h, C.byref(m)))

    def set_uncertainty_map_device(self, layer_ptr, geom, pose=(0.0, 0.0, 0.0), probes=(3, 3), layer_stride=0, poses_ptr=0):
        """layer_ptr / poses_ptr: device addresses that stay valid while solves run (e.g. the blur kernel's output)."""
        m = UncertaintyMap()
        m.layer = int(layer_ptr)
        m.geom = geom
        m.pose_x, m.pose_y, m.pose_theta = pose
        m.poses = int(poses_ptr) if poses_ptr else None
        m.layer_stride = int(layer_stride)
        m.probes_l, m.probes_w = probes
        _check(lib().cilqr_set_uncertainty_map_device(self._h, C.byref(m)))

    def clear_uncertainty_map(self):
        _check(lib().cilqr_clear_uncertainty_map(self._h))

    def debug_uncertainty_cost(self, states):
        states = _np64(states).reshape(-1, 4)
        n = states.shape[0]
        cost, vx, mx = np.zeros(n), np.zeros((n, 2)), np.zeros((n, 3))
        _check(lib().cilqr_debug_uncertainty_cost(self._h, n, _p(states), _p(cost), _p(vx), _p(mx)))
        return cost, vx, mx

    # ---- cross-GPU exchange step (RCCL behind the C-ABI) ----
    def comm_init_rank(self, n_ranks, rank, id_bytes):
        """id_bytes: the 128 bytes of `comm_unique_id()` made on one rank and carried to the others by the host."""
        buf = (C.c_char * COMM_ID_BYTES).from_buffer_copy(bytes(id_bytes))
        _check(lib().cilqr_comm_init_rank(self._h, int(n_ranks), int(rank), buf))

    def comm_size(self):
        return int(lib().cilqr_comm_size(self._h))

    def argmin_global_device(self, stream, B, J, index_offset, out_pair):
        _check(lib().cilqr_argmin_global_device(self._h, _vp(stream), int(B), _vp(J), C.c_int64(index_offset), _vp(out_pair)))

    def debug_select(self, triples):
        t = _np64(triples).reshape(-1, 3)
        out = np.zeros(2)
        _check(lib().cilqr_debug_select(self._h, int(t.shape[0]), _p(t), _p(out)))
        return float(out[0]), int(out[1])

    def set_diag_buffer(self, dev_ptr):
        _check(lib().cilqr_set_diag_buffer(self._h, _vp(dev_ptr)))

    def set_pass_count_buffer(self, dev_ptr):
        _check(lib().cilqr_set_pass_count_buffer(self._h, _vp(dev_ptr)))

    def solve_family(self, B, N, M):
        """`cilqr_solve_family`: lanes per solve for this shape — 64 = one wavefront per solve, less = the grouped family."""
        g = lib().cilqr_solve_family(self._h, int(B), int(N), int(M))
        if g < 0:
            _check(g)
        return g

    def solve_wavefronts(self, B, N, M):
        """`cilqr_solve_wavefronts`: wavefronts per solve of a static-obstacle batch on the one-wavefront family (1 or 2)."""
        w = lib().cilqr_solve_wavefronts(self._h, int(B), int(N), int(M))
        if w < 0:
            _check(w)
        return w

    def solve_sampled_wavefronts(self, B, N, n_obs):
        """`cilqr_solve_sampled_wavefronts`: wavefronts per solve sharing phase L of a sampled-obstacle solve (1, 2 or 4)."""
        w = lib().cilqr_solve_sampled_wavefronts(self._h, int(B), int(N), int(n_obs))
        if w < 0:
            _check(w)
        return w

    def debug_quu_inverse(self, Quu, lamb, general=True):
        Quu = _np64(Quu).reshape(-1, 4)
        lamb = _np64(lamb).reshape(-1)
        out = np.zeros_like(Quu)
        _check(lib().cilqr_debug_quu_inverse(self._h, int(Quu.shape[0]), _p(Quu), _p(lamb), _p(out), int(bool(general))))
        return out

    def debug_closest_sample(self, queries):
        """`cilqr_debug_closest_sample`: rows {poly[6], x_first, x_last, px, py} → int32 rows {search, full scan, by Newton}."""
        q = _np64(queries).reshape(-1, 10)
        out = np.zeros((q.shape[0], 3), dtype=np.int32)
        _check(lib().cilqr_debug_closest_sample(self._h, int(q.shape[0]), _p(q), out.ctypes.data_as(_ip)))
        return out

    def debug_blur_ellipse(self, abc):
        abc = _np64(abc).reshape(-1, 3)
        out = np.zeros_like(abc)
        _check(lib().cilqr_debug_blur_ellipse(self._h, int(abc.shape[0]), _p(abc), _p(out)))
        return out

    def debug_math(self, op, x):
        """`cilqr_debug_math`: the kernels' own exp_fast / sincos_fast / sincos_loop / rotate_heading on host data.  MATH_EXP (exp_full), MATH_EXP_FAST: x (n,)
        → (n,); MATH_SINCOS_FAST, MATH_SINCOS_LOOP: x (n,) → (n, 2) = (sin, cos); MATH_ROTATE: x (n, T + 1) rows of (theta0,
        delta_1..T) → (n, T, 2)."""
        op = int(op)
        if op == MATH_ROTATE:
            x = _np64(x)
            assert x.ndim == 2 and x.shape[1] >= 2
            n, T = x.shape[0], x.shape[1] - 1
            out = np.zeros((n, T, 2))
        else:
            x = _np64(x).reshape(-1)
            n, T = x.shape[0], 0
            out = np.zeros(n) if op in (MATH_EXP, MATH_EXP_FAST) else np.zeros((n, 2))
        _check(lib().cilqr_debug_math(self._h, op, int(n), int(T), _p(x), _p(out)))
        return out

    def wait(self):
        _check(lib().cilqr_wait(self._h))

    # ---- costmap warp ----
    def warp_costmap(self, src, src_geom, dst_geom, vx, vy, vtheta, bbox=None):
        """src: (rows, cols) float32 (any order; converted to column-major).  Returns (dst F-ordered, n_out_of_range)."""
        src = np.asfortranarray(src, dtype=np.float32)
        assert src.shape == (src_geom.rows, src_geom.cols)
        dst = np.zeros((dst_geom.rows, dst_geom.cols), dtype=np.float32, order="F")
        bb = None
        if bbox is not None:
            bbox = np.asfortranarray(bbox, dtype=np.float32)
            assert bbox.shape == dst.shape
            bb = bbox.ctypes.data_as(_fp)
        n = C.c_int64(0)
        _check(lib().cilqr_warp_costmap(self._h, src.ctypes.data_as(_fp), C.byref(src_geom), dst.ctypes.data_as(_fp),
                                        C.byref(dst_geom), C.c_double(vx), C.c_double(vy), C.c_double(vtheta), bb,
                                        C.byref(n)))
        return dst, int(n.value)

    def warp_costmap_device(self, stream, src, src_geom, dst, dst_geom, vx, vy, vtheta, bbox=0, n_oob=0):
        _check(lib().cilqr_warp_costmap_device(self._h, _vp(stream), _vp(src), C.byref(src_geom), _vp(dst),
                                               C.byref(dst_geom), C.c_double(vx), C.c_double(vy), C.c_double(vtheta),
                                               _vp(bbox), _vp(n_oob)))


    # ---- obstacle polygons ----
    def rasterize_polygons(self, geom, vertices, value=100.0, layer=None):
        """vertices: (n, V, 2) in the layer's frame.  layer None: a fresh layer, NaN outside the polygons (clear); otherwise the
        (rows, cols) float32 layer to accumulate into (its other cells are kept).  Returns the F-ordered layer."""
        v, n, V = _polygons(vertices)
        clear = layer is None
        out = np.zeros((geom.rows, geom.cols), dtype=np.float32, order="F") if clear else np.array(layer, dtype=np.float32, order="F")
        assert out.shape == (geom.rows, geom.cols)
        _check(lib().cilqr_rasterize_polygons(self._h, C.byref(geom), n, V, v.ctypes.data_as(_dp), C.c_float(value), int(clear),
                                              out.ctypes.data_as(_fp)))
        return out

    def rasterize_polygons_device(self, stream, geom, vertices, layer, value=100.0, clear=True):
        """layer: device address of rows*cols float32 (column-major)."""
        v, n, V = _polygons(vertices)
        _check(lib().cilqr_rasterize_polygons_device(self._h, _vp(stream), C.byref(geom), n, V, v.ctypes.data_as(_dp), C.c_float(value),
                                                     int(bool(clear)), _vp(layer)))

    def warp_costmap_polygons_device(self, stream, src, src_geom, dst, dst_geom, vx, vy, vtheta, vertices, n_oob=0):
        """`warp_costmap_device` whose override comes from the polygons ((n, V, 2), destination frame) instead of a bbox layer."""
        v, n, V = _polygons(vertices)
        _check(lib().cilqr_warp_costmap_polygons_device(self._h, _vp(stream), _vp(src), C.byref(src_geom), _vp(dst), C.byref(dst_geom),
                                                        C.c_double(vx), C.c_double(vy), C.c_double(vtheta), n, V, v.ctypes.data_as(_dp),
                                                        _vp(n_oob)))

    def costmap_frame_polygons_device(self, stream, global_layer, global_geom, vehicle_geom, vx, vy, vtheta, vertices, sigma_x, sigma_y,
                                      sigma_theta, vehicle_layer, uncertainty_layer, occupancy_out=0, n_oob=0):
        """`costmap_frame_device` with the obstacle polygons ((n, V, 2), vehicle frame) in place of the bbox layer."""
        v, n, V = _polygons(vertices)
        _check(lib().cilqr_costmap_frame_polygons_device(self._h, _vp(stream), _vp(global_layer), C.byref(global_geom),
                                                         C.byref(vehicle_geom), C.c_double(vx), C.c_double(vy), C.c_double(vtheta), n, V,
                                                         v.ctypes.data_as(_dp), C.c_double(sigma_x), C.c_double(sigma_y),
                                                         C.c_double(sigma_theta), _vp(vehicle_layer), _vp(uncertainty_layer),
                                                         _vp(occupancy_out), _vp(n_oob)))

    def warp_costmap_batch_device(self, stream, src, src_geom, dst, dst_geom, poses, bbox=0, n_oob=0):
        """poses: (K, 3) host array of (vx, vy, vtheta); dst: device address of K destination layers back to back."""
        poses = _np64(poses).reshape(-1, 3)
        _check(lib().cilqr_warp_costmap_batch_device(self._h, _vp(stream), _vp(src), C.byref(src_geom), _vp(dst), C.byref(dst_geom),
                                                     int(poses.shape[0]), _p(poses), _vp(bbox), _vp(n_oob)))

    def blur_costmap(self, src, geom, vtheta, sigma_x, sigma_y, sigma_theta, index=0):
        """src: (rows, cols) float32.  Returns (out F-ordered float32, counts (rows*cols,) int32)."""
        src = np.asfortranarray(src, dtype=np.float32)
        assert src.shape == (geom.rows, geom.cols)
        out = np.zeros((geom.rows, geom.cols), dtype=np.float32, order="F")
        cnt = np.zeros(geom.rows * geom.cols, dtype=np.int32)
        _check(lib().cilqr_blur_costmap(self._h, src.ctypes.data_as(_fp), C.byref(geom), int(index), C.c_double(vtheta),
                                        C.c_double(sigma_x), C.c_double(sigma_y), C.c_double(sigma_theta),
                                        out.ctypes.data_as(_fp), cnt.ctypes.data_as(_ip)))
        return out, cnt

    # ---- OccupancyGrid <-> layer ----
    def occupancy_to_layer(self, occ):
        occ = np.ascontiguousarray(occ, dtype=np.int8).reshape(-1)
        out = np.zeros(occ.size, dtype=np.float32)
        _check(lib().cilqr_occupancy_to_layer(self._h, occ.ctypes.data_as(C.c_void_p), C.c_int64(occ.size), _p(out, _fp)))
        return out

    def layer_to_occupancy(self, layer, data_min, data_max):
        layer = np.ascontiguousarray(layer, dtype=np.float32).reshape(-1)
        out = np.zeros(layer.size, dtype=np.int8)
        _check(lib().cilqr_layer_to_occupancy(self._h, _p(layer, _fp), C.c_int64(layer.size), C.c_float(data_min),
                                              C.c_float(data_max), out.ctypes.data_as(C.c_void_p)))
        return out

    def occupancy_to_layer_device(self, stream, occ, n_cells, layer):
        _check(lib().cilqr_occupancy_to_layer_device(self._h, _vp(stream), _vp(occ), C.c_int64(n_cells), _vp(layer)))

    def layer_to_occupancy_device(self, stream, layer, n_cells, data_min, data_max, occ):
        _check(lib().cilqr_layer_to_occupancy_device(self._h, _vp(stream), _vp(layer), C.c_int64(n_cells), C.c_float(data_min),
                                                     C.c_float(data_max), _vp(occ)))

    def costmap_frame_device(self, stream, global_layer, global_geom, vehicle_geom, vx, vy, vtheta, sigma_x, sigma_y,
                             sigma_theta, vehicle_layer, uncertainty_layer, occupancy_out=0, bbox=0, n_oob=0):
        _check(lib().cilqr_costmap_frame_device(self._h, _vp(stream), _vp(global_layer), C.byref(global_geom),
                                                C.byref(vehicle_geom), C.c_double(vx), C.c_double(vy), C.c_double(vtheta),
                                                _vp(bbox), C.c_double(sigma_x), C.c_double(sigma_y), C.c_double(sigma_theta),
                                                _vp(vehicle_layer), _vp(uncertainty_layer), _vp(occupancy_out), _vp(n_oob)))

    def blur_costmap_device(self, stream, src, geom, vtheta, sigma_x, sigma_y, sigma_theta, out, index=0, count_out=0):
        _check(lib().cilqr_blur_costmap_device(self._h, _vp(stream), _vp(src), C.byref(geom), int(index), C.c_double(vtheta),
                                               C.c_double(sigma_x), C.c_double(sigma_y), C.c_double(sigma_theta), _vp(out),
                                               _vp(count_out)))

    def blur_costmap_batch_device(self, stream, src, geom, vthetas, sigma_x, sigma_y, sigma_theta, out, index=0, count_out=0, src_stride=0):
        """vthetas: (K,) host array; src: device address of one layer (src_stride 0) or of K layers src_stride floats apart; out (and
        count_out): device addresses of K layers back to back."""
        vthetas = _np64(vthetas).reshape(-1)
        _check(lib().cilqr_blur_costmap_batch_device(self._h, _vp(stream), _vp(src), C.c_int64(src_stride), C.byref(geom), int(index),
                                                     int(vthetas.shape[0]), _p(vthetas), C.c_double(sigma_x), C.c_double(sigma_y),
                                                     C.c_double(sigma_theta), _vp(out), _vp(count_out)))

    def costmap_frame_batch_device(self, stream, global_layer, global_geom, vehicle_geom, poses, sigma_x, sigma_y, sigma_theta,
                                   vehicle_layers, uncertainty_layers, occupancy_out=0, bbox=0, n_oob=0):
        """poses: (K, 3) host array of (vx, vy, vtheta); vehicle_layers, uncertainty_layers (and occupancy_out, n_oob): device
        addresses of K layers (K counters) back to back; bbox: one device layer shared by the frames."""
        poses = _np64(poses).reshape(-1, 3)
        _check(lib().cilqr_costmap_frame_batch_device(self._h, _vp(stream), _vp(global_layer), C.byref(global_geom), C.byref(vehicle_geom),
                                                      int(poses.shape[0]), _p(poses), _vp(bbox), C.c_double(sigma_x), C.c_double(sigma_y),
                                                      C.c_double(sigma_theta), _vp(vehicle_layers), _vp(uncertainty_layers),
                                                      _vp(occupancy_out), _vp(n_oob)))
