"""ctypes binding of ``include/scpqp.h``, ``include/scpqp_noise.h``,
``include/scpqp_metrics.h``, ``include/scpqp_variants.h``, ``include/scpqp_truth.h``,
``include/scpqp_obstacles.h``, ``include/scpqp_sensing.h``, ``include/scpqp_estimator.h``,
``include/scpqp_tracker.h``, ``include/scpqp_manoeuvres.h``,
``include/scpqp_tracker_accel.h``, ``include/scpqp_imm.h``, ``include/scpqp_margin.h``,
``include/scpqp_governor.h``, ``include/scpqp_yield.h`` and ``include/scpqp_drive.h`` (the C-ABI
of the HIP library).

The shared library ``libscpqp.so`` is built in-tree (``__graft_entry__.build()``
or ``python -m scpqp.build``).  There is no CPU fallback: if the library or a
GPU is missing, loading fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libscpqp.so")

MAX_VEH = 16
MAX_OBST = 32
MAX_REFPTS = 8
MAX_HP = 64

ST_CONVERGED = 0
ST_MAX_SCP = 1
ST_INVALID = 2
ST_NUMERIC = 3
FL_POLISH_REJECTED = 0x100
FL_IPM_MAXIT = 0x200
FL_SAMPLER = 0x400
FLAG_OBST_QUIRK = 1
FLAG_COLD_QP = 2

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)


class Dims(C.Structure):
    _fields_ = [("n_veh", C.c_int32), ("hp_max", C.c_int32), ("n_obst", C.c_int32),
                ("max_batch", C.c_int32)]


class Params(C.Structure):
    _fields_ = [("dt", C.c_double), ("u_lim", C.c_double), ("dsafe_extra", C.c_double),
                ("constraint_tol", C.c_double), ("delta_tol", C.c_double),
                ("slack_weight", C.c_double), ("max_scp_iter", C.c_int32),
                ("max_ipm_iter", C.c_int32), ("polish_refine", C.c_int32), ("flags", C.c_int32),
                ("ipm_tol", C.c_double), ("polish_delta", C.c_double), ("polish_rho", C.c_double),
                ("lf", _dp), ("lr", _dp), ("q", _dp), ("q_final", _dp), ("r", _dp),
                ("dsafe_veh", _dp), ("dsafe_obs", _dp), ("ref_polyline", _dp),
                ("ref_npts", _ip), ("ref_max_pts", C.c_int32)]


class BatchIn(C.Structure):
    _fields_ = [("x0", C.c_void_p), ("u0", C.c_void_p), ("ec_noise", C.c_void_p),
                ("hp", C.c_void_p), ("obst", C.c_void_p), ("ref_points", C.c_void_p),
                ("u_warm", C.c_void_p), ("max_scp_iter", C.c_int32), ("reserved", C.c_int32),
                ("variant", C.c_void_p)]


class BatchOut(C.Structure):
    _fields_ = [("u", C.c_void_p), ("traj", C.c_void_p), ("status", C.c_void_p),
                ("n_scp", C.c_void_p), ("n_ipm", C.c_void_p), ("obj", C.c_void_p),
                ("max_violation", C.c_void_p), ("sum_violations", C.c_void_p),
                ("feasible", C.c_void_p), ("n_polish", C.c_void_p), ("n_refine", C.c_void_p),
                ("n_warm", C.c_void_p), ("trace", C.c_void_p)]


class LinOut(C.Structure):
    _fields_ = [("Ad", C.c_void_p), ("Bd", C.c_void_p), ("Ed", C.c_void_p), ("g", C.c_void_p),
                ("const_term", C.c_void_p), ("psi0", C.c_void_p), ("ref_points", C.c_void_p)]


class EvalOut(C.Structure):
    _fields_ = [("obj", C.c_void_p), ("max_violation", C.c_void_p),
                ("sum_violations", C.c_void_p), ("feasible", C.c_void_p), ("c_veh", C.c_void_p),
                ("c_obs", C.c_void_p), ("traj", C.c_void_p)]


class PlantParams(C.Structure):
    _fields_ = [("n_veh", C.c_int32), ("pad0", C.c_int32), ("lf", C.c_double * MAX_VEH),
                ("lr", C.c_double * MAX_VEH)]


class PlanInfo(C.Structure):
    """scpqp_plan_info (include/scpqp.h): the plan and kernel instantiation of a shape."""
    _fields_ = [("plan", C.c_int32), ("lean", C.c_int32), ("per_cu", C.c_int32),
                ("row_slots", C.c_int32), ("shape", C.c_int32), ("hg", C.c_int32),
                ("vg", C.c_int32), ("rm", C.c_int32), ("occ", C.c_int32), ("sh", C.c_int32),
                ("lds_bytes", C.c_int64), ("ws_doubles_per_wg", C.c_int64)]


# every symbol include/scpqp.h declares (checked by tests/test_abi.py)
EXPORTS = ("scpqp_create", "scpqp_destroy", "scpqp_last_error", "scpqp_version", "scpqp_solve",
           "scpqp_linearize", "scpqp_evaluate", "scpqp_sample_reference", "scpqp_resources",
           "scpqp_trace_layout", "scpqp_plan_query",
           "scpqp_delay_compensate", "scpqp_plant_step", "scpqp_clip_controls")


class Noise(C.Structure):
    """scpqp_noise (include/scpqp_noise.h): seed, sigma and the caller's part of the counter."""
    _fields_ = [("seed", C.c_uint64), ("sigma", C.c_double), ("epoch", C.c_uint32),
                ("b_offset", C.c_uint32)]


NOISE_SITE_DELAY, NOISE_SITE_PLANT, NOISE_SITE_LINEARIZE = 0, 1, 2

# every symbol include/scpqp_noise.h declares (checked by tests/test_noise_host.py)
NOISE_EXPORTS = ("scpqp_delay_compensate_noisy", "scpqp_plant_step_noisy", "scpqp_noise_fill")



class MetricsParams(C.Structure):
    """scpqp_metrics_params (include/scpqp_metrics.h): host pointers, copied at create."""
    _fields_ = [("n_veh", C.c_int32), ("n_obst", C.c_int32), ("ref_max_pts", C.c_int32),
                ("pad0", C.c_int32), ("tick_length", C.c_double), ("length", _dp), ("width", _dp),
                ("dsafe_veh", _dp), ("dsafe_obs", _dp), ("obstacles", _dp), ("ref_polyline", _dp),
                ("ref_npts", _ip)]


# the accumulator arrays of scpqp_metrics_acc, in the order of the structure
METRICS_ACC_FIELDS = ("min_gap_veh", "min_gap_obs", "min_margin_veh", "min_margin_obs",
                      "argmin_gap_veh", "argmin_gap_obs", "first_collision_tick",
                      "n_collision_ticks", "n_ticks_seen", "max_xtrack", "sum_sq_xtrack")


class MetricsAcc(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in METRICS_ACC_FIELDS]


class MetricsDense(C.Structure):
    _fields_ = [("gap_veh", C.c_void_p), ("gap_obs", C.c_void_p), ("xtrack", C.c_void_p)]


# every symbol include/scpqp_metrics.h declares (checked by tests/test_metrics_host.py)
METRICS_EXPORTS = ("scpqp_metrics_create", "scpqp_metrics_destroy", "scpqp_metrics_reset",
                   "scpqp_metrics_accumulate")

# every symbol include/scpqp_variants.h declares (checked by tests/test_variants_host.py)
VARIANT_EXPORTS = ("scpqp_set_variants", "scpqp_metrics_set_variants",
                   "scpqp_metrics_accumulate_variants")

TRUTH_NP = 5
TRUTH_LF, TRUTH_LR, TRUTH_TAU, TRUTH_GAIN, TRUTH_BIAS = range(TRUTH_NP)
TRUTH_FIELDS = ("lf", "lr", "tau", "gain", "bias")
TRUTH_TAU_NOMINAL = 0.1
TRUTH_FIXED, TRUTH_UNIFORM, TRUTH_NORMAL = 0, 1, 2
NOISE_SITE_TRUTH = 3


class TruthField(C.Structure):
    """scpqp_truth_field (include/scpqp_truth.h)."""
    _fields_ = [("kind", C.c_int32), ("pad0", C.c_int32), ("spread", C.c_double),
                ("lo", C.c_double), ("hi", C.c_double)]


class TruthDist(C.Structure):
    """scpqp_truth_dist (include/scpqp_truth.h)."""
    _fields_ = [("n_veh", C.c_int32), ("pad0", C.c_int32),
                ("mean", (C.c_double * MAX_VEH) * TRUTH_NP), ("field", TruthField * TRUTH_NP),
                ("seed", C.c_uint64), ("b_offset", C.c_uint32), ("pad1", C.c_uint32)]


# every symbol include/scpqp_truth.h declares (checked by tests/test_truth_host.py)
TRUTH_EXPORTS = ("scpqp_plant_step_truth", "scpqp_truth_fill_nominal", "scpqp_truth_sample")

OBST_NP = 7
(OBST_X, OBST_Y, OBST_HEADING, OBST_SPEED, OBST_LENGTH, OBST_WIDTH,
 OBST_YAW_RATE) = range(OBST_NP)
OBSTACLE_FIELDS = ("x", "y", "heading", "speed", "length", "width", "yaw_rate")
NOISE_SITE_OBSTACLE = 4


class ObstacleDist(C.Structure):
    """scpqp_obstacles_dist (include/scpqp_obstacles.h)."""
    _fields_ = [("n_obst", C.c_int32), ("pad0", C.c_int32),
                ("mean", (C.c_double * MAX_OBST) * OBST_NP), ("field", TruthField * OBST_NP),
                ("seed", C.c_uint64), ("b_offset", C.c_uint32), ("pad1", C.c_uint32)]


# every symbol include/scpqp_obstacles.h declares (checked by tests/test_obstacles_host.py)
OBSTACLE_EXPORTS = ("scpqp_obstacles_predict", "scpqp_obstacles_pose",
                    "scpqp_obstacles_fill_nominal", "scpqp_obstacles_sample",
                    "scpqp_metrics_accumulate_obstacles")

SENSE_NP = 8
(SENSE_SIG_POS, SENSE_SIG_HEADING, SENSE_SIG_SPEED, SENSE_SIG_STEER, SENSE_BIAS_HEADING,
 SENSE_SCALE_SPEED, SENSE_P_DROP, SENSE_LAG) = range(SENSE_NP)
SENSE_FIELDS = ("sig_pos", "sig_heading", "sig_speed", "sig_steer", "bias_heading", "scale_speed",
                "p_drop", "lag")
OSENSE_NP = 3
OSENSE_FIELDS = ("sig_pos", "sig_heading", "sig_speed")
NOISE_SITE_SENSE, NOISE_SITE_SENSE_DRAW, NOISE_SITE_SENSE_OBST = 5, 6, 7


class SenseStream(C.Structure):
    """scpqp_sense_stream (include/scpqp_sensing.h)."""
    _fields_ = [("seed", C.c_uint64), ("epoch", C.c_uint32), ("b_offset", C.c_uint32)]


class SenseDist(C.Structure):
    """scpqp_sense_dist (include/scpqp_sensing.h)."""
    _fields_ = [("n_veh", C.c_int32), ("pad0", C.c_int32),
                ("mean", (C.c_double * MAX_VEH) * SENSE_NP), ("field", TruthField * SENSE_NP),
                ("seed", C.c_uint64), ("b_offset", C.c_uint32), ("pad1", C.c_uint32)]


# every symbol include/scpqp_sensing.h declares (checked by tests/test_sensing_host.py)
SENSE_EXPORTS = ("scpqp_sense_measure", "scpqp_sense_fill_nominal", "scpqp_sense_sample",
                 "scpqp_obstacles_predict_sensed")

EST_NS = 5
EST_NP = 8
(EST_R_POS, EST_R_HEADING, EST_R_SPEED, EST_R_STEER, EST_Q_POS, EST_Q_HEADING, EST_Q_SPEED,
 EST_Q_STEER) = range(EST_NP)
EST_FIELDS = ("r_pos", "r_heading", "r_speed", "r_steer", "q_pos", "q_heading", "q_speed",
              "q_steer")

# every symbol include/scpqp_estimator.h declares (checked by tests/test_estimator_host.py)
EST_EXPORTS = ("scpqp_est_step",)

TRK_NS = 5
TRK_NZ = 4
TRK_NP = 9
(TRK_R_POS, TRK_R_HEADING, TRK_R_SPEED, TRK_Q_POS, TRK_Q_HEADING, TRK_Q_SPEED, TRK_Q_YAW,
 TRK_P0_YAW, TRK_W_CLAMP) = range(TRK_NP)
TRK_FIELDS = ("r_pos", "r_heading", "r_speed", "q_pos", "q_heading", "q_speed", "q_yaw",
              "p0_yaw", "w_clamp")
TRK_DSINC_SWITCH = 0.02

# every symbol include/scpqp_tracker.h declares (checked by tests/test_tracker_host.py)
TRK_EXPORTS = ("scpqp_obstacles_track",)

MAN_NSEG = 4
MAN_NF = 3
MAN_DUR, MAN_ACCEL, MAN_DYAW = range(MAN_NF)
MAN_FIELDS = ("dur", "accel", "dyaw")
MAN_PR_SWITCH = 0.1
NOISE_SITE_MANOEUVRE = 8


class ManoeuvreDist(C.Structure):
    """scpqp_manoeuvres_dist (include/scpqp_manoeuvres.h)."""
    _fields_ = [("n_obst", C.c_int32), ("pad0", C.c_int32),
                ("mean", (C.c_double * MAN_NF) * MAN_NSEG),
                ("field", (TruthField * MAN_NF) * MAN_NSEG),
                ("seed", C.c_uint64), ("b_offset", C.c_uint32), ("pad1", C.c_uint32)]


# every symbol include/scpqp_manoeuvres.h declares (checked by tests/test_manoeuvres_host.py)
MAN_EXPORTS = ("scpqp_manoeuvres_state", "scpqp_manoeuvres_pose", "scpqp_manoeuvres_sample",
               "scpqp_metrics_accumulate_posed")

TRKA_NS = 6
TRKA_NZ = 4
TRKA_NP = 14
(TRKA_R_POS, TRKA_R_HEADING, TRKA_R_SPEED, TRKA_Q_POS, TRKA_Q_HEADING, TRKA_Q_SPEED, TRKA_Q_YAW,
 TRKA_Q_ACCEL, TRKA_P0_YAW, TRKA_P0_ACCEL, TRKA_W_CLAMP, TRKA_A_CLAMP, TRKA_W_HOLD,
 TRKA_A_HOLD) = range(TRKA_NP)
TRKA_FIELDS = ("r_pos", "r_heading", "r_speed", "q_pos", "q_heading", "q_speed", "q_yaw",
               "q_accel", "p0_yaw", "p0_accel", "w_clamp", "a_clamp", "w_hold", "a_hold")
TRKA_DPR_SWITCH = 0.3

# every symbol include/scpqp_tracker_accel.h declares (checked by tests/test_tracker_accel_host.py)
TRKA_EXPORTS = ("scpqp_obstacles_track_accel",)

IMM_MAX_MODES = 4
IMM_SUM_TOL = 1e-12

# every symbol include/scpqp_imm.h declares (checked by tests/test_imm_host.py)
IMM_EXPORTS = ("scpqp_obstacles_track_imm",)

# every symbol include/scpqp_margin.h declares (checked by tests/test_margin_host.py)
MARGIN_EXPORTS = ("scpqp_obstacles_margin", "scpqp_solve_margin", "scpqp_evaluate_margin")

GOV_NP = 7
(GOV_V_REF, GOV_A_ACC, GOV_A_BRAKE, GOV_K_V, GOV_J_MAX, GOV_LOOK, GOV_BAND) = range(GOV_NP)
GOV_FIELDS = ("v_ref", "a_acc", "a_brake", "k_v", "j_max", "look", "band")

# every symbol include/scpqp_governor.h declares (checked by tests/test_governor_host.py)
GOV_EXPORTS = ("scpqp_governor_step",)

YLD_NP = 10
YLD_PRIO, YLD_A_EASE, YLD_S_STAND = 7, 8, 9
YLD_PRIO_MAX = 1 << 20
YLD_FIELDS = GOV_FIELDS + ("prio", "a_ease", "s_stand")

# every symbol include/scpqp_yield.h declares (checked by tests/test_yield_host.py)
YLD_EXPORTS = ("scpqp_yield_step",)

DRIVE_NP = 6
(DRIVE_TAU_A, DRIVE_GAIN_A, DRIVE_BIAS_A, DRIVE_A_MAX, DRIVE_B_MAX, DRIVE_HOLD) = range(DRIVE_NP)
DRIVE_FIELDS = ("tau_a", "gain_a", "bias_a", "a_max", "b_max", "hold")
NOISE_SITE_DRIVE = 9


class DriveDist(C.Structure):
    """scpqp_drive_dist (include/scpqp_drive.h)."""
    _fields_ = [("n_veh", C.c_int32), ("pad0", C.c_int32),
                ("mean", (C.c_double * MAX_VEH) * DRIVE_NP), ("field", TruthField * DRIVE_NP),
                ("seed", C.c_uint64), ("b_offset", C.c_uint32), ("pad1", C.c_uint32)]


# every symbol include/scpqp_drive.h declares (checked by tests/test_drive_host.py)
DRIVE_EXPORTS = ("scpqp_plant_step_drive", "scpqp_drive_fill_ideal", "scpqp_drive_sample")

_lib = None


def load(path=None):
    """Load the in-tree HIP library (raises OSError if it was not built).  The product
    path reads no environment variable: another build is loaded only by an explicit
    ``path`` or by ``use_build`` (benchmark and tools A/B runs)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise OSError(f"scpqp: HIP library not built ({p}); run __graft_entry__.build()")
    lib = C.CDLL(p)
    H = C.c_void_p
    lib.scpqp_create.argtypes = [C.POINTER(Dims), C.POINTER(Params), C.c_int, C.POINTER(H)]
    lib.scpqp_create.restype = C.c_int
    lib.scpqp_destroy.argtypes = [H]
    lib.scpqp_destroy.restype = C.c_int
    lib.scpqp_last_error.argtypes = []
    lib.scpqp_last_error.restype = C.c_char_p
    lib.scpqp_version.argtypes = []
    lib.scpqp_version.restype = C.c_char_p
    lib.scpqp_solve.argtypes = [H, C.c_int32, C.POINTER(BatchIn), C.POINTER(BatchOut), C.c_void_p]
    lib.scpqp_solve.restype = C.c_int
    lib.scpqp_linearize.argtypes = [H, C.c_int32, C.POINTER(BatchIn), C.POINTER(LinOut), C.c_void_p]
    lib.scpqp_linearize.restype = C.c_int
    lib.scpqp_evaluate.argtypes = [H, C.c_int32, C.POINTER(BatchIn), C.c_void_p,
                                   C.POINTER(EvalOut), C.c_void_p]
    lib.scpqp_evaluate.restype = C.c_int
    lib.scpqp_sample_reference.argtypes = [H, C.c_int32, C.POINTER(BatchIn), C.c_void_p, C.c_void_p]
    lib.scpqp_sample_reference.restype = C.c_int
    lib.scpqp_resources.argtypes = [H, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                    C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.scpqp_resources.restype = C.c_int
    lib.scpqp_trace_layout.argtypes = [H, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.scpqp_trace_layout.restype = C.c_int
    # an explicit ``path`` may name an A/B build from before the plan query
    if path is None or hasattr(lib, "scpqp_plan_query"):
        lib.scpqp_plan_query.argtypes = [C.POINTER(Dims), C.c_int32, C.POINTER(PlanInfo)]
        lib.scpqp_plan_query.restype = C.c_int
    PP = C.POINTER(PlantParams)
    V = C.c_void_p
    lib.scpqp_delay_compensate.argtypes = [PP, C.c_int32, C.c_double, C.c_int32, V, V, V, V, V,
                                           C.c_double, V]
    lib.scpqp_delay_compensate.restype = C.c_int
    lib.scpqp_plant_step.argtypes = [PP, C.c_int32, C.c_int32, C.c_double, V, V, V, V, C.c_double, V]
    lib.scpqp_plant_step.restype = C.c_int
    lib.scpqp_clip_controls.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double,
                                        V, V, V, V]
    lib.scpqp_clip_controls.restype = C.c_int
    NP = C.POINTER(Noise)
    lib.scpqp_delay_compensate_noisy.argtypes = [PP, C.c_int32, C.c_double, C.c_int32, V, V, NP, V,
                                                 V, C.c_double, V]
    lib.scpqp_delay_compensate_noisy.restype = C.c_int
    lib.scpqp_plant_step_noisy.argtypes = [PP, C.c_int32, C.c_int32, C.c_double, V, V, NP, V,
                                           C.c_double, V]
    lib.scpqp_plant_step_noisy.restype = C.c_int
    lib.scpqp_noise_fill.argtypes = [NP, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, V, V]
    lib.scpqp_noise_fill.restype = C.c_int
    MA, MD = C.POINTER(MetricsAcc), C.POINTER(MetricsDense)
    lib.scpqp_metrics_create.argtypes = [C.POINTER(MetricsParams), C.c_int, C.POINTER(H)]
    lib.scpqp_metrics_create.restype = C.c_int
    lib.scpqp_metrics_destroy.argtypes = [H]
    lib.scpqp_metrics_destroy.restype = C.c_int
    lib.scpqp_metrics_reset.argtypes = [H, C.c_int32, MA, V]
    lib.scpqp_metrics_reset.restype = C.c_int
    lib.scpqp_metrics_accumulate.argtypes = [H, C.c_int32, C.c_int32, C.c_int32, C.c_int32, V, MA,
                                             MD, V]
    lib.scpqp_metrics_accumulate.restype = C.c_int
    # an explicit ``path`` may name an A/B build from before the variants (tools/gpu.sh ab):
    # it is bound without them, and calling one there raises AttributeError
    if path is None or hasattr(lib, "scpqp_set_variants"):
        lib.scpqp_set_variants.argtypes = [H, C.c_int32, C.POINTER(Params)]
        lib.scpqp_set_variants.restype = C.c_int
        lib.scpqp_metrics_set_variants.argtypes = [H, C.c_int32, C.POINTER(MetricsParams)]
        lib.scpqp_metrics_set_variants.restype = C.c_int
        lib.scpqp_metrics_accumulate_variants.argtypes = [H, C.c_int32, C.c_int32, C.c_int32,
                                                          C.c_int32, V, MA, MD, V, V]
        lib.scpqp_metrics_accumulate_variants.restype = C.c_int
    # likewise an A/B build from before the plant truth
    if path is None or hasattr(lib, "scpqp_plant_step_truth"):
        lib.scpqp_plant_step_truth.argtypes = [PP, C.c_int32, C.c_int32, C.c_double, V, V, V, V, NP,
                                               V, C.c_double, V]
        lib.scpqp_plant_step_truth.restype = C.c_int
        lib.scpqp_truth_fill_nominal.argtypes = [PP, C.c_int32, V, V]
        lib.scpqp_truth_fill_nominal.restype = C.c_int
        lib.scpqp_truth_sample.argtypes = [C.POINTER(TruthDist), C.c_int32, V, V]
        lib.scpqp_truth_sample.restype = C.c_int
    # likewise an A/B build from before the obstacle truth
    if path is None or hasattr(lib, "scpqp_obstacles_predict"):
        D, I = C.c_double, C.c_int32
        lib.scpqp_obstacles_predict.argtypes = [I, I, I, V, D, D, D, V, V]
        lib.scpqp_obstacles_predict.restype = C.c_int
        lib.scpqp_obstacles_pose.argtypes = [I, I, V, D, I, I, V, V]
        lib.scpqp_obstacles_pose.restype = C.c_int
        lib.scpqp_obstacles_fill_nominal.argtypes = [I, _dp, I, V, V]
        lib.scpqp_obstacles_fill_nominal.restype = C.c_int
        lib.scpqp_obstacles_sample.argtypes = [C.POINTER(ObstacleDist), I, V, V]
        lib.scpqp_obstacles_sample.restype = C.c_int
        lib.scpqp_metrics_accumulate_obstacles.argtypes = [H, I, I, I, I, V, MA, MD, V, V, V]
        lib.scpqp_metrics_accumulate_obstacles.restype = C.c_int
    # likewise an A/B build from before the sensing truth
    if path is None or hasattr(lib, "scpqp_sense_measure"):
        D, I = C.c_double, C.c_int32
        SS = C.POINTER(SenseStream)
        lib.scpqp_sense_measure.argtypes = [I, I, I, I, V, V, SS, V, V, V, V]
        lib.scpqp_sense_measure.restype = C.c_int
        lib.scpqp_sense_fill_nominal.argtypes = [I, I, V, V]
        lib.scpqp_sense_fill_nominal.restype = C.c_int
        lib.scpqp_sense_sample.argtypes = [C.POINTER(SenseDist), I, V, V]
        lib.scpqp_sense_sample.restype = C.c_int
        lib.scpqp_obstacles_predict_sensed.argtypes = [I, I, I, V, V, SS, D, D, D, V, V]
        lib.scpqp_obstacles_predict_sensed.restype = C.c_int
    # likewise an A/B build from before the state estimator
    if path is None or hasattr(lib, "scpqp_est_step"):
        D, I = C.c_double, C.c_int32
        lib.scpqp_est_step.argtypes = [PP, I, I, D, D, V, V, V, V, V, V, V, V]
        lib.scpqp_est_step.restype = C.c_int
    # likewise an A/B build from before the obstacle tracker
    if path is None or hasattr(lib, "scpqp_obstacles_track"):
        D, I = C.c_double, C.c_int32
        SS = C.POINTER(SenseStream)
        lib.scpqp_obstacles_track.argtypes = [I, I, I, V, V, SS, V, D, D, D, D, V, V, V, V, V, V]
        lib.scpqp_obstacles_track.restype = C.c_int
    # likewise an A/B build from before the obstacle manoeuvres
    if path is None or hasattr(lib, "scpqp_manoeuvres_state"):
        D, I = C.c_double, C.c_int32
        lib.scpqp_manoeuvres_state.argtypes = [I, I, V, V, D, V, V]
        lib.scpqp_manoeuvres_state.restype = C.c_int
        lib.scpqp_manoeuvres_pose.argtypes = [I, I, V, V, D, I, I, V, V]
        lib.scpqp_manoeuvres_pose.restype = C.c_int
        lib.scpqp_manoeuvres_sample.argtypes = [C.POINTER(ManoeuvreDist), I, V, V]
        lib.scpqp_manoeuvres_sample.restype = C.c_int
        lib.scpqp_metrics_accumulate_posed.argtypes = [H, I, I, I, I, V, MA, MD, V, V, V, V]
        lib.scpqp_metrics_accumulate_posed.restype = C.c_int
    # likewise an A/B build from before the tracker with an acceleration state
    if path is None or hasattr(lib, "scpqp_obstacles_track_accel"):
        D, I = C.c_double, C.c_int32
        SS = C.POINTER(SenseStream)
        lib.scpqp_obstacles_track_accel.argtypes = [I, I, I, V, V, SS, V, D, D, D, D, V, V, V, V, V,
                                                    V]
        lib.scpqp_obstacles_track_accel.restype = C.c_int
    # likewise an A/B build from before the interacting-multiple-model tracker
    if path is None or hasattr(lib, "scpqp_obstacles_track_imm"):
        D, I = C.c_double, C.c_int32
        SS = C.POINTER(SenseStream)
        lib.scpqp_obstacles_track_imm.argtypes = [I, I, I, I, V, V, SS, V, V, D, D, D, D, V, V, V,
                                                  V, V, V, V, V]
        lib.scpqp_obstacles_track_imm.restype = C.c_int
    # likewise an A/B build from before the obstacle margins
    if path is None or hasattr(lib, "scpqp_obstacles_margin"):
        D, I = C.c_double, C.c_int32
        lib.scpqp_obstacles_margin.argtypes = [I, I, I, I, V, V, V, V, D, D, D, D, V, V, V]
        lib.scpqp_obstacles_margin.restype = C.c_int
        lib.scpqp_solve_margin.argtypes = [H, C.c_int32, C.POINTER(BatchIn), V,
                                           C.POINTER(BatchOut), V]
        lib.scpqp_solve_margin.restype = C.c_int
        lib.scpqp_evaluate_margin.argtypes = [H, C.c_int32, C.POINTER(BatchIn), V, V,
                                              C.POINTER(EvalOut), V]
        lib.scpqp_evaluate_margin.restype = C.c_int
    # likewise an A/B build from before the speed governor
    if path is None or hasattr(lib, "scpqp_governor_step"):
        D, I = C.c_double, C.c_int32
        lib.scpqp_governor_step.argtypes = [I, I, I, I, D, D, V, V, V, V, V, V, V, V, V, V, V, V]
        lib.scpqp_governor_step.restype = C.c_int
    # likewise an A/B build from before the right of way
    if path is None or hasattr(lib, "scpqp_yield_step"):
        D, I = C.c_double, C.c_int32
        lib.scpqp_yield_step.argtypes = [I, I, I, I, D, D] + [V] * 15
        lib.scpqp_yield_step.restype = C.c_int
    # likewise an A/B build from before the drive truth
    if path is None or hasattr(lib, "scpqp_plant_step_drive"):
        D, I = C.c_double, C.c_int32
        lib.scpqp_plant_step_drive.argtypes = [PP, I, I, D, V, V, V, V, NP, V, V, V, D, V]
        lib.scpqp_plant_step_drive.restype = C.c_int
        lib.scpqp_drive_fill_ideal.argtypes = [I, I, V, V]
        lib.scpqp_drive_fill_ideal.restype = C.c_int
        lib.scpqp_drive_sample.argtypes = [C.POINTER(DriveDist), I, V, V]
        lib.scpqp_drive_sample.restype = C.c_int
    if path is None:
        _lib = lib
    return lib


def use_build(path):
    """Tools / tests only (bench.py --lib, tools/bitwise_ab.py): make every later
    ``load()`` of this process return another build of the same C-ABI (an A/B variant or
    a diagnostic build), loaded before any solver is created."""
    global _lib
    _lib = load(os.path.abspath(path))
    return _lib


def check(rc, lib=None):
    if rc != 0:
        lib = lib or load()
        raise RuntimeError(f"scpqp error {rc}: {lib.scpqp_last_error().decode()}")
