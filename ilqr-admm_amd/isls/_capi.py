"""ctypes binding of the C ABI declared in include/isls_hip.h.

`Kernels` marshals numpy arrays or torch tensors into the argument structs of the library.  The
product instantiates it on `csrc/libisls_hip.so` (device pointers + a HIP stream); the tests
instantiate the very same class on the CPU oracle (`oracle/liboracle_isls.so`, host pointers, no
stream) so that both sides are called with identical marshaling.

There is NO fallback: if the HIP library is missing, `load_hip_library()` raises.
"""
import ctypes as C
import os

import numpy as np

try:  # torch is plumbing (device memory, streams); the binding itself works on numpy too
    import torch
except Exception:  # pragma: no cover
    torch = None

ABI_VERSION = 107            # ISLS_VERSION of include/isls_hip.h these ctypes structs mirror
OK, ERR_ARG, ERR_UNSUPPORTED, ERR_LAUNCH, ERR_COMPILE = 0, -1, -2, -3, -4
ST_NOT_PD, ST_NAN_COST, ST_LS_REJECT, ST_REG_MAX = 1, 2, 4, 8
REG_AFTER_GAIN, REG_AFTER_LS = 0, 1             # isls_reg_update_args.mode
SOLVE_CHOL, SOLVE_INV = 0, 1
MODEL_LTI, MODEL_ARM3R, MODEL_CAR, MODEL_DI, MODEL_TASSA = 0, 1, 2, 3, 4
MODEL_USER_BASE, USER_MAX_PAR = 1024, 16      # ids of user models (isls_user_model_create), parameters per model at most
USER_MAX_TAB = 16                              # words per step of a user cost's / model's table (isls_user_*_create_tab), at most
USER_MAX_FIELD, USER_MAX_FIELD_WORDS = 4, 1 << 24   # channels and samples of a user cost's 2-D field (isls_user_cost_create_field), at most
DTYPE_F64, DTYPE_F32 = 0, 1
COST_VIA, COST_PHUBER = 0, 1
COST_USER_BASE = 1024                          # ids of user costs (isls_user_cost_create)
RO_NAN_TO_1E5, RO_ACCEPT_TEST, RO_ABSOLUTE = 1, 2, 4
PROJ_NONE, PROJ_BOX, PROJ_SETS = 0, 1, 2
CTL_NOT_CAUSAL = 1

_HERE = os.path.dirname(os.path.abspath(__file__))
HIP_LIB_PATH = os.path.join(os.path.dirname(_HERE), "csrc", "libisls_hip.so")


class View(C.Structure):
    _fields_ = [("p", C.c_void_p), ("sb", C.c_int64), ("st", C.c_int64)]


class GainArgs(C.Structure):
    _fields_ = [("B", C.c_int32), ("N", C.c_int32), ("n", C.c_int32), ("m", C.c_int32),
                ("solve_mode", C.c_int32), ("_pad", C.c_int32),
                ("A", View), ("Bm", View), ("Cxx", View), ("Cuu", View), ("Cux", View),
                ("K", C.c_void_p), ("Quu", C.c_void_p), ("fac", C.c_void_p), ("Qux", C.c_void_p),
                ("status", C.c_void_p), ("active", C.c_void_p), ("rec", C.c_void_p),
                ("lin_on", C.c_int32), ("lin_model", C.c_int32), ("lin_par", C.c_void_p), ("lin_par_sb", C.c_int64)]


class RegArgs(C.Structure):
    """isls_reg_args: per-trajectory mu of the regularised gain pass"""
    _fields_ = [("mu", C.c_void_p), ("on_x", C.c_int32), ("_pad", C.c_int32)]


class RegUpdateArgs(C.Structure):
    """isls_reg_update_args: the mu / delta schedule"""
    _fields_ = [("B", C.c_int32), ("mode", C.c_int32), ("status", C.c_void_p), ("active", C.c_void_p),
                ("mu", C.c_void_p), ("delta", C.c_void_p), ("retry", C.c_void_p), ("count", C.c_void_p),
                ("factor", C.c_double), ("mu_min", C.c_double), ("mu_max", C.c_double)]


class FfSeg(C.Structure):
    """Time-parallel form of the feed-forward pass (isls_ffseg): nseg <= 1 / G NULL = sequential."""
    _fields_ = [("nseg", C.c_int32), ("seg_len", C.c_int32), ("G", C.c_void_p), ("Psi", C.c_void_p), ("v", C.c_void_p)]


class FfArgs(C.Structure):
    _fields_ = [("B", C.c_int32), ("N", C.c_int32), ("n", C.c_int32), ("m", C.c_int32),
                ("solve_mode", C.c_int32), ("_pad", C.c_int32),
                ("A", View), ("Bm", View), ("c0x", View), ("c0u", View), ("Qr", View), ("Rr", View),
                ("xhat", C.c_void_p), ("uhat", C.c_void_p),
                ("zx", C.c_void_p), ("lx", C.c_void_p), ("zu", C.c_void_p), ("lu", C.c_void_p),
                ("K", C.c_void_p), ("Quu", C.c_void_p), ("fac", C.c_void_p), ("Qux", C.c_void_p),
                ("k", C.c_void_p), ("active", C.c_void_p), ("seg", FfSeg), ("rec", C.c_void_p), ("Qr_term", C.c_void_p),
                ("lin_on", C.c_int32), ("lin_model", C.c_int32), ("lin_par", C.c_void_p), ("lin_par_sb", C.c_int64)]


class FfPrepareArgs(C.Structure):
    _fields_ = [("B", C.c_int32), ("N", C.c_int32), ("n", C.c_int32), ("m", C.c_int32),
                ("solve_mode", C.c_int32), ("_pad", C.c_int32),
                ("A", View), ("Bm", View),
                ("K", C.c_void_p), ("Quu", C.c_void_p), ("fac", C.c_void_p), ("Qux", C.c_void_p),
                ("active", C.c_void_p), ("seg", FfSeg), ("rec", C.c_void_p)]


class RolloutArgs(C.Structure):
    _fields_ = [("B", C.c_int32), ("N", C.c_int32), ("n", C.c_int32), ("m", C.c_int32), ("L", C.c_int32),
                ("model", C.c_int32), ("flags", C.c_int32), ("nvia", C.c_int32),
                ("model_par", C.c_void_p), ("model_par_sb", C.c_int64),
                ("K", C.c_void_p), ("k", C.c_void_p), ("xhat", C.c_void_p), ("uhat", C.c_void_p),
                ("x0", C.c_void_p), ("alphas", C.c_void_p),
                ("Qtab", C.c_void_p), ("Qtab_sb", C.c_int64), ("ztab", C.c_void_p), ("ztab_sb", C.c_int64),
                ("seq", C.c_void_p), ("q_nonzero", C.c_void_p), ("u_std", C.c_double),
                ("wq", View), ("wr", View),
                ("zx", C.c_void_p), ("lx", C.c_void_p), ("zu", C.c_void_p), ("lu", C.c_void_p),
                ("cost_cur", C.c_void_p), ("cost_all", C.c_void_p), ("best", C.c_void_p),
                ("cost_new", C.c_void_p), ("x_out", C.c_void_p), ("u_out", C.c_void_p),
                ("status", C.c_void_p), ("active", C.c_void_p),
                ("cost_model", C.c_int32), ("cost_par_sb", C.c_int32), ("cost_par", C.c_void_p)]


class AdmmArgs(C.Structure):
    _fields_ = [("B", C.c_int32), ("N", C.c_int32), ("n", C.c_int32), ("m", C.c_int32),
                ("proj_x", C.c_int32), ("proj_u", C.c_int32),
                ("relax", C.c_double), ("tol_abs", C.c_double), ("tol_rel", C.c_double),
                ("xx", C.c_void_p), ("xu", C.c_void_p),
                ("zx", C.c_void_p), ("lx", C.c_void_p), ("zu", C.c_void_p), ("lu", C.c_void_p),
                ("x_lo", View), ("x_hi", View), ("u_lo", View), ("u_hi", View),
                ("res", C.c_void_p), ("res_prev", C.c_void_p), ("active", C.c_void_p), ("iters", C.c_void_p),
                ("x_sets", C.c_void_p), ("u_sets", C.c_void_p), ("x_col0", C.c_int32), ("u_col0", C.c_int32),
                ("x_work", C.c_void_p), ("u_work", C.c_void_p)]


class ExpandArgs(C.Structure):
    _fields_ = [("B", C.c_int32), ("N", C.c_int32), ("n", C.c_int32), ("m", C.c_int32),
                ("nvia", C.c_int32), ("_pad", C.c_int32),
                ("Qtab", C.c_void_p), ("Qtab_sb", C.c_int64), ("ztab", C.c_void_p), ("ztab_sb", C.c_int64),
                ("seq", C.c_void_p), ("u_std", C.c_double),
                ("Qr", View), ("Rr", View),
                ("xhat", C.c_void_p), ("uhat", C.c_void_p),
                ("Cxx", C.c_void_p), ("Cuu", C.c_void_p), ("c0x", C.c_void_p), ("c0u", C.c_void_p),
                ("cost", C.c_void_p), ("active", C.c_void_p),
                ("cost_model", C.c_int32), ("cost_par_sb", C.c_int32), ("cost_par", C.c_void_p), ("q_nonzero", C.c_void_p)]


class LinearizeArgs(C.Structure):
    _fields_ = [("B", C.c_int32), ("N", C.c_int32), ("n", C.c_int32), ("m", C.c_int32),
                ("model", C.c_int32), ("_pad", C.c_int32),
                ("model_par", C.c_void_p), ("model_par_sb", C.c_int64),
                ("xhat", C.c_void_p), ("uhat", C.c_void_p), ("A", C.c_void_p), ("Bm", C.c_void_p),
                ("active", C.c_void_p)]


class AcceptArgs(C.Structure):
    _fields_ = [("B", C.c_int32), ("N", C.c_int32), ("n", C.c_int32), ("m", C.c_int32),
                ("xx", C.c_void_p), ("xu", C.c_void_p), ("cost_new", C.c_void_p),
                ("xhat", C.c_void_p), ("uhat", C.c_void_p), ("cost", C.c_void_p),
                ("cost_hist", C.c_void_p), ("hist_len", C.c_void_p),
                ("tol_cost", C.c_double), ("tol_osc", C.c_double), ("outer_active", C.c_void_p)]


class CSet(C.Structure):
    _fields_ = [("kind", C.c_int32), ("dim", C.c_int32), ("A", C.c_void_p), ("b", C.c_void_p), ("par", C.c_void_p),
                ("A_sp", C.c_int64), ("b_sp", C.c_int64), ("par_sp", C.c_int64)]


class ProjectArgs(C.Structure):
    _fields_ = [("P", C.c_int32), ("R", C.c_int32), ("d", C.c_int32), ("nsets", C.c_int32),
                ("max_iter", C.c_int32), ("algorithm", C.c_int32), ("rho", C.c_double), ("threshold", C.c_double),
                ("sets", CSet * 4),
                ("y_in", C.c_void_p), ("in_sp", C.c_int64), ("in_sr", C.c_int64),
                ("y_out", C.c_void_p), ("out_sp", C.c_int64), ("out_sr", C.c_int64),
                ("iters", C.c_void_p), ("active", C.c_void_p), ("row_mask", C.c_void_p), ("next", C.c_void_p)]


class SlsAdmmArgs(C.Structure):
    _fields_ = [("P", C.c_int32), ("R", C.c_int32), ("D", C.c_int32), ("max_iter", C.c_int32),
                ("alpha", C.c_double), ("tol", C.c_double), ("rel_tol", C.c_double),
                ("Linv", C.c_void_p), ("r_side", C.c_void_p), ("rr", C.c_void_p),
                ("proj", ProjectArgs),
                ("x_u", C.c_void_p), ("z", C.c_void_p), ("lmb", C.c_void_p), ("logs", C.c_void_p), ("iters", C.c_void_p)]


class ColumnsArgs(C.Structure):
    _fields_ = [("B", C.c_int32), ("N", C.c_int32), ("n", C.c_int32), ("m", C.c_int32), ("C", C.c_int32), ("_pad", C.c_int32),
                ("A", View), ("Bm", View), ("Cuu", View), ("c0u", View), ("Rr", View),
                ("K", C.c_void_p), ("k", C.c_void_p), ("zu", C.c_void_p), ("lu", C.c_void_p),
                ("dx", C.c_void_p), ("du", C.c_void_p), ("active", C.c_void_p)]


class DenseLoopArgs(C.Structure):
    _fields_ = [("M", C.c_int32), ("N", C.c_int32), ("n", C.c_int32), ("m", C.c_int32), ("model", C.c_int32), ("_pad", C.c_int32),
                ("model_par", C.c_void_p), ("K", C.c_void_p), ("k", C.c_void_p), ("xhat", C.c_void_p), ("uhat", C.c_void_p),
                ("x0", C.c_void_p), ("x_log", C.c_void_p), ("u_log", C.c_void_p)]


class McLoopArgs(C.Structure):
    """isls_mc_loop_args: the Monte-Carlo closed loop of a batch of controllers (isls/montecarlo.py)"""
    _fields_ = [("P", C.c_int32), ("M", C.c_int32), ("N", C.c_int32), ("n", C.c_int32), ("m", C.c_int32),
                ("model", C.c_int32), ("K_form", C.c_int32), ("_pad", C.c_int32),
                ("model_par", C.c_void_p), ("par_sb", C.c_int64),
                ("K", C.c_void_p), ("k", C.c_void_p), ("K_sb", C.c_int64), ("k_sb", C.c_int64),
                ("xhat", C.c_void_p), ("uhat", C.c_void_p), ("xhat_sb", C.c_int64), ("uhat_sb", C.c_int64),
                ("x0s", C.c_void_p), ("x0", C.c_void_p), ("x0_sb", C.c_int64), ("x0_std", C.c_void_p),
                ("w", C.c_void_p), ("noise_std", C.c_void_p), ("seed", C.c_uint64),
                ("problem0", C.c_int32), ("sample0", C.c_int32),
                ("u_lo", View), ("u_hi", View), ("x_lo", View), ("x_hi", View),
                ("viol_u", C.c_void_p), ("viol_x", C.c_void_p), ("viol_any", C.c_void_p),
                ("u_min", C.c_void_p), ("u_max", C.c_void_p), ("x_min", C.c_void_p), ("x_max", C.c_void_p),
                ("x_log", C.c_void_p), ("u_log", C.c_void_p), ("w_out", C.c_void_p), ("x0_out", C.c_void_p),
                ("work", C.c_void_p), ("work_elems", C.c_int64)]


class MpcStepArgs(C.Structure):
    """isls_mpc_step_args: one control step of a receding-horizon loop, in place (Engine.mpc_step, iSLS.mpc)"""
    _fields_ = [("B", C.c_int32), ("N", C.c_int32), ("n", C.c_int32), ("m", C.c_int32), ("model", C.c_int32), ("W", C.c_int32),
                ("model_par", C.c_void_p), ("par_sb", C.c_int64), ("plant_par", C.c_void_p), ("plant_sb", C.c_int64),
                ("xhat", C.c_void_p), ("uhat", C.c_void_p), ("K", C.c_void_p), ("zx", C.c_void_p), ("zu", C.c_void_p),
                ("tab", C.c_void_p), ("tab_sb", C.c_int64), ("tab_next", C.c_void_p), ("tab_next_sb", C.c_int64),
                ("u_lo", C.c_void_p), ("u_hi", C.c_void_p), ("w", C.c_void_p), ("noise_std", C.c_void_p), ("seed", C.c_uint64),
                ("problem0", C.c_int32), ("step", C.c_int32),
                ("x_meas_out", C.c_void_p), ("u_out", C.c_void_p), ("x_next_out", C.c_void_p),
                ("x_meas_sb", C.c_int64), ("u_out_sb", C.c_int64), ("x_next_sb", C.c_int64)]


class SampleArgs(C.Structure):
    """isls_sample_args: one sampling round about the nominal, in place (Engine.sample_round, iSLS.sample_nominal)"""
    _fields_ = [("B", C.c_int32), ("N", C.c_int32), ("n", C.c_int32), ("m", C.c_int32), ("S", C.c_int32),
                ("model", C.c_int32), ("cost_model", C.c_int32), ("nvia", C.c_int32),
                ("model_par", C.c_void_p), ("model_par_sb", C.c_int64), ("cost_par", C.c_void_p), ("cost_par_sb", C.c_int64),
                ("xhat", C.c_void_p), ("uhat", C.c_void_p),
                ("Qtab", C.c_void_p), ("Qtab_sb", C.c_int64), ("ztab", C.c_void_p), ("ztab_sb", C.c_int64),
                ("seq", C.c_void_p), ("u_std", C.c_double),
                ("sigma", C.c_void_p), ("sigma_sb", C.c_int64), ("u_lo", C.c_void_p), ("u_hi", C.c_void_p),
                ("temperature", C.c_double), ("seed", C.c_uint64), ("problem0", C.c_int32), ("phase", C.c_int32),
                ("problem_ids", C.c_void_p), ("active", C.c_void_p), ("costs", C.c_void_p),
                ("cost_before", C.c_void_p), ("cost_after", C.c_void_p), ("cost_best", C.c_void_p), ("ess", C.c_void_p),
                ("took_best", C.c_void_p), ("stat_sb", C.c_int64)]


class CovArgs(C.Structure):
    """isls_cov_args: mean and covariance of the linearised closed loop of a batch of stage-local controllers (isls/covariance.py)"""
    _fields_ = [("P", C.c_int32), ("N", C.c_int32), ("n", C.c_int32), ("m", C.c_int32),
                ("A", View), ("Bm", View),
                ("K", C.c_void_p), ("k", C.c_void_p), ("K_sb", C.c_int64), ("k_sb", C.c_int64),
                ("xhat", C.c_void_p), ("uhat", C.c_void_p), ("xhat_sb", C.c_int64), ("uhat_sb", C.c_int64),
                ("dx0", C.c_void_p), ("dx0_sb", C.c_int64), ("S0", C.c_void_p), ("S0_sb", C.c_int64),
                ("W", View), ("u_lo", View), ("u_hi", View), ("x_lo", View), ("x_hi", View),
                ("active", C.c_void_p),
                ("x_mean", C.c_void_p), ("u_mean", C.c_void_p), ("x_var", C.c_void_p), ("u_var", C.c_void_p),
                ("x_cov", C.c_void_p), ("u_cov", C.c_void_p), ("p_u", C.c_void_p), ("p_x", C.c_void_p)]


class SlsControllerArgs(C.Structure):
    _fields_ = [("B", C.c_int32), ("N", C.c_int32), ("n", C.c_int32), ("m", C.c_int32), ("A", View), ("Bm", View),
                ("PHI_U", C.c_void_p), ("du", C.c_void_p), ("K", C.c_void_p), ("k", C.c_void_p), ("flags", C.c_void_p),
                ("work", C.c_void_p)]


class ColumnsAdmmArgs(C.Structure):
    _fields_ = [("B", C.c_int32), ("N", C.c_int32), ("n", C.c_int32), ("m", C.c_int32), ("C", C.c_int32), ("phase", C.c_int32),
                ("relax", C.c_double), ("tol_abs", C.c_double), ("tol_rel", C.c_double),
                ("xx", C.c_void_p), ("xu", C.c_void_p),
                ("zx", C.c_void_p), ("lx", C.c_void_p), ("zu", C.c_void_p), ("lu", C.c_void_p),
                ("zx_prev", C.c_void_p), ("zu_prev", C.c_void_p), ("x_nom", C.c_void_p), ("u_nom", C.c_void_p),
                ("x_work", C.c_void_p), ("u_work", C.c_void_p), ("Qr", View), ("Rr", View),
                ("res", C.c_void_p), ("res_prev", C.c_void_p), ("active", C.c_void_p), ("iters", C.c_void_p)]


class OuterArgs(C.Structure):
    _fields_ = [("gain", GainArgs), ("ff", FfArgs), ("ro", RolloutArgs), ("admm", AdmmArgs),
                ("J", C.c_int32), ("skip_gain", C.c_int32), ("begin_done", C.c_int32), ("_pad", C.c_int32),
                ("log", C.c_void_p), ("outer_active", C.c_void_p), ("timing", C.c_void_p)]


class ColumnsIterationArgs(C.Structure):
    _fields_ = [("ff", FfArgs), ("cols", ColumnsArgs), ("ls", RolloutArgs), ("admm", ColumnsAdmmArgs),
                ("proj_x", C.c_void_p), ("proj_u", C.c_void_p), ("zero_x", C.c_void_p), ("zero_u", C.c_void_p), ("log", C.c_void_p),
                ("any_active", C.c_void_p)]


class ConstraintUpdateArgs(C.Structure):
    """isls_constraint_update_args (include/isls_hip.h)"""
    _fields_ = [("B", C.c_int32), ("N", C.c_int32), ("n", C.c_int32), ("m", C.c_int32), ("cost_model", C.c_int32), ("update", C.c_int32),
                ("cost_par", C.c_void_p), ("cost_par_sb", C.c_int64), ("tab", C.c_void_p), ("tab_sb", C.c_int64),
                ("xhat", C.c_void_p), ("uhat", C.c_void_p), ("viol", C.c_void_p), ("viol_prev", C.c_void_p), ("g_out", C.c_void_p),
                ("eta", C.c_double), ("phi", C.c_double), ("mu_max", C.c_double), ("active", C.c_void_p)]


class AdjointArgs(C.Structure):
    """isls_adjoint_args (include/isls_hip.h)"""
    _fields_ = [("B", C.c_int32), ("N", C.c_int32), ("n", C.c_int32), ("m", C.c_int32), ("A", View), ("Bm", View),
                ("c0x", C.c_void_p), ("c0u", C.c_void_p), ("lam", C.c_void_p), ("gu", C.c_void_p), ("gx0", C.c_void_p),
                ("active", C.c_void_p)]


class UserGradArgs(C.Structure):
    """isls_user_grad_args (include/isls_hip.h)"""
    _fields_ = [("B", C.c_int32), ("N", C.c_int32), ("n", C.c_int32), ("m", C.c_int32), ("id", C.c_int32), ("_pad", C.c_int32),
                ("par", C.c_void_p), ("par_sb", C.c_int64), ("tab", C.c_void_p), ("tab_sb", C.c_int64),
                ("xhat", C.c_void_p), ("uhat", C.c_void_p), ("lam", C.c_void_p), ("g_par", C.c_void_p), ("g_tab", C.c_void_p),
                ("active", C.c_void_p)]


class AdvanceArgs(C.Structure):
    _fields_ = [("accept", AcceptArgs), ("lin", LinearizeArgs), ("exp", ExpandArgs),
                ("admm_active", C.c_void_p), ("iters", C.c_void_p), ("lx", C.c_void_p), ("lu", C.c_void_p), ("res_prev", C.c_void_p)]


# names every build of the library must export (checked by tests/test_capi_host.py)
EXPORTED = [f"isls_{k}_{s}" for s in ("f64", "f32") for k in
            ("riccati_gain", "riccati_ff", "riccati_gain_ff", "riccati_ff_prepare", "rollout_ls", "admm_update", "project_rows", "sls_admm", "sls_closed_loop", "columns_rollout", "columns_admm", "dense_closed_loop", "mc_closed_loop", "mpc_step", "sample_nominal", "sample_nominal_fb", "cov_closed_loop", "sls_controller", "expand_quadratic", "linearize",
             "accept_step", "reduce_convergence", "reduce_convergence_table", "ilqr_admm_outer", "outer_advance", "columns_iteration",
             "user_model_step", "user_model_step_tab", "user_cost_value", "user_cost_value_tab", "user_cost_expand", "riccati_gain_reg", "reg_update",
             "user_constraint_update", "adjoint_sweep", "user_model_grad", "user_cost_grad")] + \
           ["isls_ff_segments", "isls_ff_record_elems", "isls_sls_controller_work_elems", "isls_mc_work_elems", "isls_version", "isls_dims_supported", "isls_dims_generic", "isls_error_string", "isls_timing_create",
            "isls_timing_destroy", "isls_timing_reset", "isls_timing_pause", "isls_timing_read_ms",
            "isls_gain_memo_stats", "isls_gain_memo_clear",
            "isls_user_model_create", "isls_user_model_log", "isls_user_model_code", "isls_user_model_load",
            "isls_user_cost_create", "isls_user_cost_log", "isls_user_cost_code", "isls_user_cost_load",
            "isls_user_cost_create_tab", "isls_user_cost_n_tab", "isls_user_model_create_tab", "isls_user_model_n_tab",
            "isls_user_cost_create_con", "isls_user_cost_n_con", "isls_user_model_grad_build", "isls_user_cost_grad_build",
            "isls_user_cost_create_field", "isls_user_cost_set_field", "isls_user_cost_field_dims", "isls_user_cost_field_ptr",
            "isls_user_cost_release_field"]


SET_BOX, SET_SOC_UNIT, SET_SQUARE, SET_LINEAR, SET_QUADRATIC, SET_SHELL, SET_MULTILINEAR = 1, 2, 3, 4, 5, 6, 7
SET_ROW_PAR, SET_ROW_B = 0x100, 0x200          # ISLS_SET_ROW_*: flag bits of isls_cset.kind, one par block / one b per row
ALG_ADMM, ALG_DYKSTRA, ALG_SOC = 0, 1, 2
MAX_ROW_DIM, MAX_SET_DIM, MAX_SETS = 4, 5, 4


class IslsError(RuntimeError):
    pass


def load_hip_library(path=None):
    """dlopen the HIP library and declare its functions that are not typed f64 / f32 pairs; fail loudly (no CPU fallback
    exists by design).  A handle of its own per call: library() is the process-wide one."""
    path = path or os.environ.get("ISLS_HIP_LIB") or HIP_LIB_PATH       # env override: A/B builds when tuning
    if not os.path.exists(path):
        raise IslsError(f"{path} not found: build it with `python __graft_entry__.py` "
                        f"(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    lib = C.CDLL(path)
    lib.isls_version.restype = C.c_int
    if lib.isls_version() != ABI_VERSION:                      # a stale build would read the argument blocks with another layout
        raise IslsError(f"{path} reports ABI version {lib.isls_version()}, this binding is for {ABI_VERSION}: rebuild it "
                        f"(`python __graft_entry__.py`)")
    i32 = C.c_int32
    lib.isls_error_string.restype = C.c_char_p
    lib.isls_dims_supported.restype = lib.isls_dims_generic.restype = i32
    lib.isls_dims_supported.argtypes = lib.isls_dims_generic.argtypes = [i32, i32]
    lib.isls_ff_segments.restype = i32
    lib.isls_ff_segments.argtypes = [i32, i32, C.POINTER(i32)]
    lib.isls_ff_record_elems.restype = lib.isls_sls_controller_work_elems.restype = C.c_int64
    lib.isls_ff_record_elems.argtypes = [i32, i32, i32, i32]
    lib.isls_sls_controller_work_elems.argtypes = [i32, i32, i32]
    lib.isls_mc_work_elems.restype = C.c_int64
    lib.isls_mc_work_elems.argtypes = [i32, i32, i32, i32, i32, i32]
    lib.isls_timing_create.restype = C.c_void_p
    lib.isls_timing_destroy.restype = None
    lib.isls_timing_destroy.argtypes = [C.c_void_p]
    lib.isls_timing_reset.argtypes = [C.c_void_p]
    lib.isls_timing_pause.argtypes = [C.c_void_p, C.c_int]
    lib.isls_timing_read_ms.restype = C.c_double
    lib.isls_timing_read_ms.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    src = [C.c_char_p, i32, i32, i32]                          # user models and user costs: (source, n, m, n_par)
    for noun, ids in (("model", [i32]), ("cost", [i32, i32])):   # a cost's code / load take (cost id, model id)
        for what, argtypes in (("create", src + [C.POINTER(i32)]), ("create_tab", src + [i32, C.POINTER(i32)]), ("n_tab", [i32]),
                               ("log", [i32, C.c_char_p, C.c_int64]), ("code", ids + [i32, C.c_void_p, C.POINTER(C.c_int64)]),
                               ("load", ids + [i32])):
            getattr(lib, f"isls_user_{noun}_{what}").argtypes = argtypes
        getattr(lib, f"isls_user_{noun}_log").restype = C.c_int64
    lib.isls_user_cost_create_con.argtypes = src + [i32, i32, C.POINTER(i32)]   # (.., n_tab, n_con, &id)
    lib.isls_user_cost_n_con.argtypes = [i32]
    lib.isls_user_cost_create_field.argtypes = src + [i32] * 5 + [C.POINTER(i32)]   # (.., n_tab, n_con, n_field, nx, ny, &id)
    lib.isls_user_cost_set_field.argtypes = [i32, C.c_void_p, i32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p]
    lib.isls_user_cost_field_dims.argtypes = [i32] + [C.POINTER(i32)] * 3
    lib.isls_user_cost_field_ptr.argtypes = [i32, i32, C.POINTER(C.c_void_p)]
    lib.isls_user_cost_release_field.argtypes = [i32]
    lib.isls_user_model_grad_build.argtypes = lib.isls_user_cost_grad_build.argtypes = [i32, i32]
    return lib


def gain_memo_stats(lib=None):
    """(checks, matches) of the outer driver's gain memo so far (include/isls_hip.h); synchronises: tests and tools only."""
    lib = lib or library()
    c, m = C.c_int64(0), C.c_int64(0)
    lib.isls_gain_memo_stats.argtypes = [C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    rc = lib.isls_gain_memo_stats(C.byref(c), C.byref(m))
    if rc != OK:
        raise IslsError(f"isls_gain_memo_stats -> {rc}")
    return c.value, m.value


def gain_memo_clear(lib=None):
    """Free the gain memo's entries (synchronises)."""
    lib = lib or library()
    lib.isls_gain_memo_clear.restype = None
    lib.isls_gain_memo_clear()


_LIB = None


def library():
    """The process-wide handle of the HIP library (ISLS_HIP_LIB, else csrc/libisls_hip.so), loaded on first use."""
    global _LIB
    if _LIB is None:
        _LIB = load_hip_library()
    return _LIB


def dims_supported(n, m):
    """True when the HIP library carries kernels for state dimension n and control dimension m (isls_dims_supported)."""
    return bool(library().isls_dims_supported(int(n), int(m)))


def dims_generic(n, m):
    """True when (n, m) is served at all: by the templated kernels or by the generic ones of csrc/generic.hip (n <= 16, m <= 8)."""
    return bool(library().isls_dims_generic(int(n), int(m)))


def supported_dims(n_max=16, m_max=8):
    """The (x_dim, u_dim) pairs the loaded library was built for."""
    return [(n, m) for n in range(1, n_max + 1) for m in range(1, m_max + 1) if dims_supported(n, m)]


# ------------------------------------------------------------------------------------------------
# user models and user costs: run-time compiled sources (isls_user_model_*, isls_user_cost_*)
# ------------------------------------------------------------------------------------------------
def _dtype_code(dtype):
    return DTYPE_F32 if dtype in (np.float32, "f32") or (torch is not None and dtype == torch.float32) else DTYPE_F64


class _UserKind:
    """The entry points of one kind of source (`noun`: model | cost).  A cost's code and load also take the model it is
    paired with (-1: expansion and value only); ids of the two kinds count independently from `base`."""

    def __init__(self, noun, base):
        self.noun, self.base, self.ids = noun, base, {}      # ids: (source, n, m, P) -> id, one registration per process

    def _fn(self, what):
        return getattr(library(), f"isls_user_{self.noun}_{what}")

    def _fail(self, what, rc, uid):
        return IslsError(f"isls_user_{self.noun}_{what} -> {rc}: {library().isls_error_string(rc).decode()}\n{self.log(uid)}")

    def log(self, uid):
        size = self._fn("log")(C.c_int32(uid), None, 0)
        buf = C.create_string_buffer(int(max(size, 0)) + 1)
        self._fn("log")(C.c_int32(uid), buf, len(buf))
        return buf.value.decode(errors="replace")

    def create(self, source, n, m, n_par, n_tab=0, n_con=0, field=None):
        """n_tab > 0: a source with a per-step table of that many words; the key of one without is what it was.  n_con > 0: a cost
        with that many constraints, whose n_tab counts their multipliers and mu: part of the key as well.  field = (C, nx, ny): a
        cost with a 2-D field -- a registration of its own every time, since the id owns the field's device buffers"""
        key = (str(source), int(n), int(m), int(n_par)) + ((int(n_tab),) if n_tab else ()) + ((int(n_con),) if n_con else ())
        if field is None and key in self.ids:
            return self.ids[key]
        uid = C.c_int32(-1)
        if field is not None:
            rc = self._fn("create_field")(key[0].encode(), *key[1:4], int(n_tab), int(n_con), *(int(v) for v in field), C.byref(uid))
        else:
            rc = self._fn("create_con" if n_con else "create_tab" if n_tab else "create")(key[0].encode(), *key[1:], C.byref(uid))
        if rc == ERR_COMPILE:
            raise IslsError(f"user {self.noun}: compile failed\n{self.log(uid.value) if uid.value >= self.base else ''}")
        if rc != OK:
            raise IslsError(f"isls_user_{self.noun}_create -> {rc}: {library().isls_error_string(rc).decode()}")
        if field is None:
            self.ids[key] = uid.value
        return uid.value

    def n_tab(self, uid):
        """Words per step of the source's table (0: a source without one)."""
        rc = self._fn("n_tab")(C.c_int32(uid))
        if rc < 0:
            raise IslsError(f"isls_user_{self.noun}_n_tab -> {rc}: {library().isls_error_string(rc).decode()}")
        return rc

    def code(self, uid, *model, dtype):
        args, size = [C.c_int32(v) for v in (uid,) + model] + [_dtype_code(dtype)], C.c_int64(0)
        rc = self._fn("code")(*args, None, C.byref(size))
        if rc == OK:
            buf = C.create_string_buffer(size.value)
            rc = self._fn("code")(*args, buf, C.byref(size))
        if rc != OK:
            raise self._fail("code", rc, uid)
        return buf.raw

    def load(self, uid, *model, dtype):
        rc = self._fn("load")(*[C.c_int32(v) for v in (uid,) + model], _dtype_code(dtype))
        if rc != OK:
            raise self._fail("load", rc, uid)


    def grad_build(self, uid, dtype):
        """The source's gradient program (isls_user_*_grad_build), compiled on first request; IslsError carries the log."""
        rc = self._fn("grad_build")(C.c_int32(uid), _dtype_code(dtype))
        if rc != OK:
            raise self._fail("grad_build", rc, uid)


_USER_MODEL, _USER_COST = _UserKind("model", MODEL_USER_BASE), _UserKind("cost", COST_USER_BASE)
user_model_log, user_cost_log = _USER_MODEL.log, _USER_COST.log
user_cost_n_tab = _USER_COST.n_tab


def user_model_create(source, n, m, n_par, n_tab=0):
    """Compile a user model for gfx950 (fp64 at once, fp32 on first use) and return its id; the same (source, n, m, n_par, n_tab)
    is compiled once per process.  n_tab > 0: the model reads a table of that many words per step (isls_user_model_create_tab;
    the five-argument `step`).  IslsError carries the compile log."""
    return _USER_MODEL.create(source, n, m, n_par, n_tab)


def user_model_n_tab(model_id):
    """Words per step of the model's table (0: a model without one, and every built-in model)."""
    return _USER_MODEL.n_tab(model_id) if int(model_id) >= MODEL_USER_BASE else 0


def user_model_code(model_id, dtype=np.float64):
    """The model's gfx950 code object (a bare ELF) for dtype."""
    return _USER_MODEL.code(model_id, dtype=dtype)


def user_model_load(model_id, dtype=np.float64):
    """Load the model's module onto the current device (outside any stream capture)."""
    _USER_MODEL.load(model_id, dtype=dtype)


def user_model_grad_build(model_id, dtype=np.float64):
    """Compile the model's gradient program (the parameter and table directions of iSLS.gradient) for dtype; needs no GPU."""
    _USER_MODEL.grad_build(model_id, dtype)


def user_cost_grad_build(cost_id, dtype=np.float64):
    """The same for a cost."""
    _USER_COST.grad_build(cost_id, dtype)


def user_cost_create(source, n, m, n_par, n_tab=0, n_con=0, field=None):
    """Register a user cost and compile its expansion and value for gfx950 (fp64; the line-search kernels are compiled per model
    it is used with); the same (source, n, m, n_par, n_tab, n_con) is registered once per process.  n_tab > 0: the cost reads a
    table of that many words per step (isls_user_cost_create_tab; the six-argument `stage`).  n_con > 0: `source` also defines
    `constraint` (isls_user_cost_create_con) and n_tab = W + n_con + 1: the user's W words, the multipliers and mu.  field = (C, nx, ny):
    the source may call isls::field (isls_user_cost_create_field), and every call registers a cost of its own, whose values come
    with user_cost_set_field.  IslsError carries the compile log."""
    return _USER_COST.create(source, n, m, n_par, n_tab, n_con, field)


def user_cost_set_field(cost_id, values, origin, spacing, stream=None):
    """isls_user_cost_set_field: `values` a contiguous fp64 or fp32 torch tensor [C, nx, ny] on the current device."""
    if values.dtype not in (torch.float64, torch.float32) or not values.is_contiguous():
        raise ValueError("user_cost_set_field: a contiguous fp64 or fp32 device tensor")
    org, spc = (C.c_double * 2)(*(float(v) for v in origin)), (C.c_double * 2)(*(float(v) for v in spacing))
    rc = library().isls_user_cost_set_field(C.c_int32(cost_id), C.c_void_p(values.data_ptr()), _dtype_code(values.dtype), org, spc,
                                            C.c_void_p(stream or 0))
    if rc != OK:
        raise IslsError(f"isls_user_cost_set_field -> {rc}: {library().isls_error_string(rc).decode()}")


def user_cost_field_dims(cost_id):
    """(C, nx, ny) of the cost's field, (0, 0, 0) for a cost without one (isls_user_cost_field_dims)."""
    c, nx, ny = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    rc = library().isls_user_cost_field_dims(C.c_int32(cost_id), C.byref(c), C.byref(nx), C.byref(ny))
    if rc != OK:
        raise IslsError(f"isls_user_cost_field_dims -> {rc}: {library().isls_error_string(rc).decode()}")
    return c.value, nx.value, ny.value


def user_cost_release_field(cost_id):
    """Free the field's sample buffers on every device (isls_user_cost_release_field); the next user_cost_set_field allocates again."""
    rc = library().isls_user_cost_release_field(C.c_int32(cost_id))
    if rc != OK:
        raise IslsError(f"isls_user_cost_release_field -> {rc}: {library().isls_error_string(rc).decode()}")


def user_cost_field_ptr(cost_id, dtype=np.float64):
    """The address of the field's sample buffer of dtype on the current device (None: not set there): it never moves."""
    ptr = C.c_void_p(0)
    rc = library().isls_user_cost_field_ptr(C.c_int32(cost_id), _dtype_code(dtype), C.byref(ptr))
    if rc != OK:
        raise IslsError(f"isls_user_cost_field_ptr -> {rc}: {library().isls_error_string(rc).decode()}")
    return ptr.value


def user_cost_code(cost_id, model=-1, dtype=np.float64):
    """The gfx950 code object (a bare ELF) of the cost with `model` (a model id; -1: expansion and value only) for dtype."""
    return _USER_COST.code(cost_id, model, dtype=dtype)


def user_cost_load(cost_id, model=-1, dtype=np.float64):
    """Compile (if need be) and load the module of the cost with `model` onto the current device (outside any stream capture)."""
    _USER_COST.load(cost_id, model, dtype=dtype)


def _cost_par(cost_model, cost_par, B):
    """(ptr, batch stride) of the cost parameters: a user cost's are [P] or [B, P], a built-in cost's one shared vector"""
    if int(cost_model) >= COST_USER_BASE:
        if cost_par is None:
            raise ValueError("a user cost needs its parameters (cost_par)")
        return _par(cost_par, B, "cost_par")
    return _ptr(cost_par), 0


def _cost_tab(a, cost_model, cost_tab):
    """A user cost's table [N, W] or [B, N, W] into the fields such a cost ignores otherwise (include/isls_hip.h): ztab, ztab_sb
    (0 or N W), nvia = W"""
    if cost_tab is None:
        return
    if int(cost_model) < COST_USER_BASE:
        raise ValueError("cost_tab: the per-step table of a user cost")
    if cost_tab.ndim not in (2, 3):
        raise ValueError(f"cost_tab: [N, W] or [B, N, W], got shape {tuple(cost_tab.shape)}")
    W = int(cost_tab.shape[-1])
    a.ztab, a.ztab_sb = _tab(cost_tab, a.B, (a.N, W), "cost_tab")
    a.nvia = W


# ------------------------------------------------------------------------------------------------
# array helpers (numpy or torch)
# ------------------------------------------------------------------------------------------------
def _is_torch(x):
    return torch is not None and isinstance(x, torch.Tensor)


def _ptr(x):
    if x is None:
        return None
    if _is_torch(x):
        return x.data_ptr()
    return x.ctypes.data


def _estrides(x):
    if _is_torch(x):
        return tuple(x.stride())
    return tuple(s // x.itemsize for s in x.strides)


def _sfx(x):
    dt = x.dtype
    if dt in (np.float64,) or (torch is not None and dt == torch.float64):
        return "f64"
    if dt in (np.float32,) or (torch is not None and dt == torch.float32):
        return "f32"
    raise TypeError(f"unsupported dtype {dt}")


def _sfx_int(x):
    return "i32" if x.dtype in (np.int32,) or (torch is not None and x.dtype == torch.int32) else str(x.dtype)


def _contiguous(x):
    return x.is_contiguous() if _is_torch(x) else x.flags["C_CONTIGUOUS"]


def _dense(x, shape, name):
    """Check a dense C-contiguous operand of exactly `shape`."""
    if x is None:
        return None
    if tuple(x.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(x.shape)}")
    if not _contiguous(x):
        raise ValueError(f"{name}: must be C-contiguous")
    return x


def _row_par_words(kind, dim, arr, name):
    """Words Wp of one row's parameter block of a per-row table (include/isls_hip.h ISLS_SET_ROW_PAR); SQUARE / MULTILINEAR:
    from the q of the table, which every row must share (read from the table once, when the descriptor is built: a device
    table is copied to the host for that; project_args_chain reads the numpy table before it is moved and passes the width
    on as `par_words`)."""
    fixed = {SET_BOX: 2 * dim, SET_LINEAR: 2 + dim, SET_QUADRATIC: 2, SET_SHELL: 2 + dim}
    if kind in fixed:
        return fixed[kind]
    if arr.ndim not in (2, 3):
        raise ValueError(f"{name}: with par_rows=True [Rtot, Wp] or [P, Rtot, Wp], got {tuple(arr.shape)}")
    col = arr[..., 0]
    col = np.asarray(col.cpu() if _is_torch(col) else col)
    q = int(col.flat[0])
    if np.any(col != q):
        raise ValueError(f"{name}: every row of a per-row table must carry the same q")
    if not 1 <= q <= MAX_SET_DIM:
        raise ValueError(f"{name}: q = {q} outside 1 .. {MAX_SET_DIM}")
    return 3 + q + 2 * q * q if kind == SET_SQUARE else 1 + 2 * q + q * dim


def ff_record_elems(B, N, n, m):
    """isls_ff_record_elems: elements of the packed-record buffer of the gain pass (blocked by wavefront)."""
    tpw = 64 // (n + m)
    model_words = 6 if (n, m) in ((9, 3), (4, 2)) else 0       # rec_model_words (csrc/isls_common.hpp): the arm's A[6:8, 0:3] / the car's six entries behind fac
    return -(-B // tpw) * tpw * N * ((n * n + 2 * n * m + m * m + model_words + 1) & ~1)   # record stride padded to an even word count


def sls_controller_work_elems(B, N, n):
    """isls_sls_controller_work_elems: the N(N-1)/2 blocks of Phi_x below its diagonal and xd [N, n], per problem."""
    return B * (N * (N - 1) // 2 * n * n + N * n)


def mc_work_elems(P, M, N, n, m, K_form):
    """isls_mc_work_elems: dx of every (sample, step) of a dense controller's loop, samples padded to whole workgroups."""
    return P * (-(-M // 128) * 128) * N * n if K_form == 1 else 0


def _record(rec, B, N, n, m):
    if rec is None:
        return None
    size = rec.numel() if _is_torch(rec) else rec.size
    if size < ff_record_elems(B, N, n, m) or not _contiguous(rec):
        raise ValueError(f"rec: needs a contiguous buffer of {ff_record_elems(B, N, n, m)} elements")
    return rec


def make_view(x, B, N, core, name):
    """Strided per-(b,t) operand: trailing dims == core (contiguous), leading dims broadcast to (B,N)."""
    if x is None:
        return View(None, 0, 0)
    core = tuple(core)
    nc = len(core)
    if tuple(x.shape[x.ndim - nc:]) != core:
        raise ValueError(f"{name}: trailing dims {tuple(x.shape)} != {core}")
    lead = tuple(x.shape[: x.ndim - nc])
    if len(lead) > 2:
        raise ValueError(f"{name}: at most two leading dims (batch, time)")
    st = _estrides(x)
    exp = 1
    for d, s in zip(reversed(core), reversed(st[x.ndim - nc:])):
        if d != 1 and s != exp:
            raise ValueError(f"{name}: trailing dims must be contiguous")
        exp *= d
    lead_st = st[: x.ndim - nc]
    if len(lead) == 0:
        sb = s_t = 0
    elif len(lead) == 1:            # [N, ...]: shared over the batch
        if lead[0] not in (1, N):
            raise ValueError(f"{name}: leading dim {lead[0]} is neither 1 nor N={N}")
        sb, s_t = 0, (0 if lead[0] == 1 else lead_st[0])
    else:
        if lead[0] not in (1, B) or lead[1] not in (1, N):
            raise ValueError(f"{name}: leading dims {lead} do not broadcast to ({B},{N})")
        sb = 0 if lead[0] == 1 else lead_st[0]
        s_t = 0 if lead[1] == 1 else lead_st[1]
    return View(_ptr(x), sb, s_t)


def _tab(x, B, core, name):
    """Per-batch table [core] or [B, core]: returns (ptr, batch stride in elements)."""
    core = tuple(core)
    if tuple(x.shape) == core:
        _dense(x, core, name)
        return _ptr(x), 0
    _dense(x, (B,) + core, name)
    return _ptr(x), int(np.prod(core))


def _par(par, B, name):
    """Model parameters [P] shared or [B, P] per trajectory: returns (ptr, batch stride in elements)."""
    if par.ndim not in (1, 2) or (par.ndim == 2 and par.shape[0] != B) or not _contiguous(par):
        raise ValueError(f"{name}: contiguous [P] or [B, P] with B={B}, got shape {tuple(par.shape)}")
    return _ptr(par), (int(par.shape[1]) if par.ndim == 2 else 0)


class Kernels:
    """Thin marshaling layer over one shared library exporting `<prefix><kernel>_<f64|f32>`."""

    def __init__(self, lib, prefix="isls_", with_stream=True):
        self.lib, self.prefix, self.with_stream = lib, prefix, with_stream

    # -- plumbing ---------------------------------------------------------------------------------
    def _invoke(self, name, sfx, *argv, stream=None):
        """Call <prefix><name>_<sfx>(*argv[, stream]); IslsError with the library's text for a code other than ISLS_OK."""
        sym = f"{self.prefix}{name}_{sfx}"
        fn = getattr(self.lib, sym)
        fn.restype = C.c_int
        rc = fn(*argv, C.c_void_p(stream or 0)) if self.with_stream else fn(*argv)
        if rc != OK:
            text = getattr(self.lib, "isls_error_string", None)          # the oracle has none
            if text is not None:
                text.restype = C.c_char_p
            raise IslsError(f"{sym} -> {rc}" + (f": {text(rc).decode()}" if text is not None else ""))
        return rc

    def _call(self, name, sfx, args, stream):
        return self._invoke(name, sfx, C.byref(args), stream=stream)

    # -- argument builders (also used to fill OuterArgs) --------------------------------------------
    @staticmethod
    def _set_lin(a, lin, B, dtype):
        """hint fields of isls_gain_args / isls_ff_args: lin = (model id, parameters [P] or [B, P]) or None"""
        if lin is None:
            a.lin_on, a.lin_model, a.lin_par, a.lin_par_sb = 0, 0, None, 0
            return
        model, par = lin
        if par.dtype != dtype:
            raise ValueError("lin parameters: contiguous [P] or [B, P] of the pass's dtype")
        a.lin_on, a.lin_model = 1, int(model)
        a.lin_par, a.lin_par_sb = _par(par, B, "lin parameters")

    @staticmethod
    def gain_args(A, Bm, Cxx, Cuu, K, Quu, fac, Qux, Cux=None, solve_mode=SOLVE_CHOL, status=None, active=None, rec=None, lin=None):
        """lin = (model id, parameters): A, Bm are isls_linearize's output for that model (isls_gain_args.lin_on)"""
        B, N, m, n = K.shape
        a = GainArgs(B=B, N=N, n=n, m=m, solve_mode=solve_mode)
        Kernels._set_lin(a, lin, B, K.dtype)
        a.A, a.Bm = make_view(A, B, N, (n, n), "A"), make_view(Bm, B, N, (n, m), "B")
        a.Cxx, a.Cuu = make_view(Cxx, B, N, (n, n), "Cxx"), make_view(Cuu, B, N, (m, m), "Cuu")
        a.Cux = make_view(Cux, B, N, (m, n), "Cux")
        a.K, a.Quu = _ptr(_dense(K, (B, N, m, n), "K")), _ptr(_dense(Quu, (B, N, m, m), "Quu"))
        a.fac, a.Qux = _ptr(_dense(fac, (B, N, m, m), "fac")), _ptr(_dense(Qux, (B, N, m, n), "Qux"))
        a.status, a.active = _ptr(status), _ptr(active)
        a.rec = _ptr(_record(rec, B, N, n, m))
        return a

    @staticmethod
    def ff_args(A, Bm, c0x, c0u, K, Quu, fac, Qux, k, Qr=None, Rr=None, xhat=None, uhat=None,
                zx=None, lx=None, zu=None, lu=None, solve_mode=SOLVE_CHOL, active=None, seg=None, rec=None, ncol=1, Qr_term=None,
                lin=None):
        """lin = (model id, parameters [P] or [B, P]): A, Bm are isls_linearize's output for that model (isls_ff_args.lin_on)"""
        B, N, m, n = K.shape
        cols = int(ncol) if ncol and ncol > 1 else 0            # feedback columns: zx, lx, zu, lu, k are [C,B,N,.] blocks ...
        lead = (cols, B) if cols else (B,)                      # ... read as C*B trajectories, and Quu / fac / Qux are not used
        a = FfArgs(B=B, N=N, n=n, m=m, solve_mode=solve_mode, _pad=cols)
        if lin is not None and rec is None:
            raise ValueError("lin goes with the packed records")
        Kernels._set_lin(a, lin, B, K.dtype)
        if Qr_term is not None:                                 # weight block of the last step (isls_ff_args.Qr_term): [n,n]
            if Qr is None or tuple(Qr.shape) not in ((n, n), (1, n, n), (1, 1, n, n)):
                raise ValueError("Qr_term goes with a batch-shared, time-invariant Qr block")
            a.Qr_term = _ptr(_dense(Qr_term, (n, n), "Qr_term"))
        if seg is not None:
            a.seg = seg
        a.A, a.Bm = make_view(A, B, N, (n, n), "A"), make_view(Bm, B, N, (n, m), "B")
        a.c0x, a.c0u = make_view(c0x, B, N, (n,), "c0x"), make_view(c0u, B, N, (m,), "c0u")
        a.Qr, a.Rr = make_view(Qr, B, N, (n, n), "Qr"), make_view(Rr, B, N, (m, m), "Rr")
        for W, z, l, text in ((Qr, zx, lx, "Qr given without zx/lx"), (Rr, zu, lu, "Rr given without zu/lu")):
            if W is not None and (z is None or l is None):
                raise ValueError("Qr / Rr given without z / l" if cols else text)
        a.xhat, a.uhat = _ptr(_dense(xhat, (B, N, n), "xhat")), _ptr(_dense(uhat, (B, N, m), "uhat"))
        a.zx, a.lx = _ptr(_dense(zx, lead + (N, n), "zx")), _ptr(_dense(lx, lead + (N, n), "lx"))
        a.zu, a.lu = _ptr(_dense(zu, lead + (N, m), "zu")), _ptr(_dense(lu, lead + (N, m), "lu"))
        a.k = _ptr(_dense(k, lead + (N, m), "k"))
        a.K = _ptr(_dense(K, (B, N, m, n), "K"))
        if not cols:
            a.Quu = _ptr(_dense(Quu, (B, N, m, m), "Quu"))
            a.fac, a.Qux = _ptr(_dense(fac, (B, N, m, m), "fac")), _ptr(_dense(Qux, (B, N, m, n), "Qux"))
        a.active = _ptr(active)
        a.rec = _ptr(_record(rec, B, N, n, m))
        return a

    @staticmethod
    def ff_seg(G, Psi, v, seg_len):
        """isls_ffseg over caller-owned buffers G[B,N,m,n], Psi[B,nseg,n,n], v[B,nseg,n]."""
        B, N, m, n = G.shape
        nseg = int(Psi.shape[1])
        _dense(G, (B, N, m, n), "seg.G"), _dense(Psi, (B, nseg, n, n), "seg.Psi"), _dense(v, (B, nseg, n), "seg.v")
        return FfSeg(nseg=nseg, seg_len=int(seg_len), G=_ptr(G), Psi=_ptr(Psi), v=_ptr(v))

    @staticmethod
    def ff_prepare_args(A, Bm, K, Quu, fac, Qux, seg, solve_mode=SOLVE_CHOL, active=None, rec=None):
        B, N, m, n = K.shape
        a = FfPrepareArgs(B=B, N=N, n=n, m=m, solve_mode=solve_mode, seg=seg)
        a.A, a.Bm = make_view(A, B, N, (n, n), "A"), make_view(Bm, B, N, (n, m), "B")
        a.K, a.Quu = _ptr(_dense(K, (B, N, m, n), "K")), _ptr(_dense(Quu, (B, N, m, m), "Quu"))
        a.fac, a.Qux = _ptr(_dense(fac, (B, N, m, m), "fac")), _ptr(_dense(Qux, (B, N, m, n), "Qux"))
        a.active = _ptr(active)
        a.rec = _ptr(_record(rec, B, N, n, m))
        return a

    @staticmethod
    def rollout_args(model, model_par, K, k, xhat, uhat, alphas, Qtab, ztab, seq, u_std, x_out, u_out,
                     best=None, cost_new=None, cost_all=None, x0=None, wq=None, wr=None, zx=None, lx=None,
                     zu=None, lu=None, cost_cur=None, flags=0, status=None, active=None, q_nonzero=None,
                     cost_model=COST_VIA, cost_par=None, cost_tab=None):
        B, N, m, n = K.shape
        L = int(alphas.shape[0])
        nvia = int(Qtab.shape[-3])
        a = RolloutArgs(B=B, N=N, n=n, m=m, L=L, model=model, flags=flags, nvia=nvia, u_std=float(u_std))
        a.model_par, a.model_par_sb = _par(model_par, B, "model_par")
        a.K, a.k = _ptr(_dense(K, (B, N, m, n), "K")), _ptr(_dense(k, (B, N, m), "k"))
        a.xhat, a.uhat = _ptr(_dense(xhat, (B, N, n), "xhat")), _ptr(_dense(uhat, (B, N, m), "uhat"))
        a.x0 = _ptr(_dense(x0, (B, n), "x0"))
        a.alphas = _ptr(alphas)
        a.Qtab, a.Qtab_sb = _tab(Qtab, B, (nvia, n, n), "Qtab")
        a.ztab, a.ztab_sb = _tab(ztab, B, (nvia, n), "ztab")
        if tuple(seq.shape) != (N,):
            raise ValueError("seq must be int32[N]")
        a.seq = _ptr(seq)
        if q_nonzero is not None and tuple(q_nonzero.shape) != (N,):
            raise ValueError("q_nonzero must be int32[N]")
        a.q_nonzero = _ptr(q_nonzero)
        a.wq, a.wr = make_view(wq, B, N, (n,), "wq"), make_view(wr, B, N, (m,), "wr")
        if wq is not None and (zx is None or lx is None):
            raise ValueError("wq given without zx/lx")
        if wr is not None and (zu is None or lu is None):
            raise ValueError("wr given without zu/lu")
        a.zx, a.lx = _ptr(_dense(zx, (B, N, n), "zx")), _ptr(_dense(lx, (B, N, n), "lx"))
        a.zu, a.lu = _ptr(_dense(zu, (B, N, m), "zu")), _ptr(_dense(lu, (B, N, m), "lu"))
        if (flags & RO_ACCEPT_TEST) and cost_cur is None:
            raise ValueError("ISLS_RO_ACCEPT_TEST needs cost_cur")
        a.cost_cur = _ptr(_dense(cost_cur, (B,), "cost_cur"))
        a.cost_all = _ptr(_dense(cost_all, (B, L), "cost_all"))
        a.best, a.cost_new = _ptr(best), _ptr(_dense(cost_new, (B,), "cost_new"))
        a.x_out, a.u_out = _ptr(_dense(x_out, (B, N, n), "x_out")), _ptr(_dense(u_out, (B, N, m), "u_out"))
        a.status, a.active = _ptr(status), _ptr(active)
        a.cost_model = int(cost_model)
        a.cost_par, a.cost_par_sb = _cost_par(cost_model, cost_par, B)
        _cost_tab(a, cost_model, cost_tab)
        return a

    @staticmethod
    def admm_args(xx, xu, res, zx=None, lx=None, zu=None, lu=None, x_lo=None, x_hi=None, u_lo=None, u_hi=None,
                  relax=1.0, tol_abs=0.0, tol_rel=0.0, res_prev=None, active=None, iters=None,
                  x_sets=None, x_col0=0, x_work=None, u_sets=None, u_col0=0, u_work=None):
        """x_sets / u_sets: a ProjectArgs descriptor (project_args) => ISLS_PROJ_SETS on that block, with the
        [B,N,.] scratch x_work / u_work and the first projected coordinate x_col0 / u_col0."""
        B, N, n = xx.shape
        m = xu.shape[2]
        a = AdmmArgs(B=B, N=N, n=n, m=m, relax=float(relax), tol_abs=float(tol_abs), tol_rel=float(tol_rel))
        a.proj_x = PROJ_SETS if x_sets is not None else (PROJ_BOX if x_lo is not None else PROJ_NONE)
        a.proj_u = PROJ_SETS if u_sets is not None else (PROJ_BOX if u_lo is not None else PROJ_NONE)
        if x_sets is not None:
            a.x_sets, a.x_col0, a.x_work = C.addressof(x_sets), int(x_col0), _ptr(_dense(x_work, (B, N, n), "x_work"))
        if u_sets is not None:
            a.u_sets, a.u_col0, a.u_work = C.addressof(u_sets), int(u_col0), _ptr(_dense(u_work, (B, N, m), "u_work"))
        a._keep = (x_sets, u_sets)
        a.xx, a.xu = _ptr(_dense(xx, (B, N, n), "xx")), _ptr(_dense(xu, (B, N, m), "xu"))
        a.zx, a.lx = _ptr(_dense(zx, (B, N, n), "zx")), _ptr(_dense(lx, (B, N, n), "lx"))
        a.zu, a.lu = _ptr(_dense(zu, (B, N, m), "zu")), _ptr(_dense(lu, (B, N, m), "lu"))
        a.x_lo, a.x_hi = make_view(x_lo, B, N, (n,), "x_lo"), make_view(x_hi, B, N, (n,), "x_hi")
        a.u_lo, a.u_hi = make_view(u_lo, B, N, (m,), "u_lo"), make_view(u_hi, B, N, (m,), "u_hi")
        a.res, a.res_prev = _ptr(_dense(res, (B, 2), "res")), _ptr(_dense(res_prev, (B, 2), "res_prev"))
        a.active, a.iters = _ptr(active), _ptr(iters)
        return a

    # -- kernels -------------------------------------------------------------------------------------
    def riccati_gain(self, *args, stream=None, **kw):
        a = self.gain_args(*args, **kw)
        return self._call("riccati_gain", _sfx(args[4]), a, stream)

    def riccati_ff(self, *args, stream=None, **kw):
        a = self.ff_args(*args, **kw)
        return self._call("riccati_ff", _sfx(args[4]), a, stream)

    def riccati_gain_ff(self, gain, ff, sfx, stream=None):
        """Gain pass + first feed-forward pass in one launch (argument blocks from gain_args / ff_args)."""
        self._invoke("riccati_gain_ff", sfx, C.byref(gain), C.byref(ff), stream=stream)

    def riccati_gain_reg(self, gain, ff, mu, on_x, sfx, stream=None):
        """Gain pass on Cuu + mu I (on_x: and Cxx + mu I), mu [B] per trajectory; ff: the first feed-forward pass inside (or None)."""
        if tuple(mu.shape) != (gain.B,) or _sfx(mu) != sfx or not _contiguous(mu):
            raise ValueError(f"mu: contiguous [{gain.B}] of the pass's dtype")
        reg = RegArgs(mu=_ptr(mu), on_x=int(bool(on_x)))
        self._invoke("riccati_gain_reg", sfx, C.byref(gain), C.byref(ff) if ff is not None else None, C.byref(reg), stream=stream)

    def reg_update(self, mode, status, mu, delta, factor, mu_min, mu_max, active=None, retry=None, count=None, stream=None):
        """The mu / delta schedule (isls_reg_update_*): mode REG_AFTER_GAIN or REG_AFTER_LS."""
        B = int(mu.shape[0])
        for x, name in ((mu, "mu"), (delta, "delta")):
            if tuple(x.shape) != (B,) or x.dtype != mu.dtype or not _contiguous(x):
                raise ValueError(f"{name}: contiguous [{B}]")
        a = RegUpdateArgs(B=B, mode=int(mode), status=_ptr(status), active=_ptr(active), mu=_ptr(mu), delta=_ptr(delta),
                          retry=_ptr(retry), count=_ptr(count), factor=float(factor), mu_min=float(mu_min), mu_max=float(mu_max))
        return self._call("reg_update", _sfx(mu), a, stream)

    @staticmethod
    def project_args(y_in, y_out, sets, rho=1.0, max_iter=200, threshold=1e-4, iters=None, active=None, cols=None,
                     algorithm=ALG_ADMM, row_mask=None, next_stage=None, row0=0):
        """isls_project_args for rows y[P,R,D]; `cols=(c0, d)` projects the coordinate block [c0, c0+d) of every row
        (the rest of the row is not touched).  sets: list of dicts kind, dim, A[dim,d] | [P,dim,d], b, par (arrays of
        the dtype of y; a leading P axis gives per-problem operands).  A dict with par_rows=True carries par [Rtot,Wp] or
        [P,Rtot,Wp], one parameter block per row (ISLS_SET_ROW_PAR; `par_words`, if given, is Wp as the caller read it from
        the table's q, else it is read here), with b_rows=True b [Rtot,dim] or [P,Rtot,dim]
        (ISLS_SET_ROW_B); Rtot >= row0 + R, and the call applies the rows row0 .. row0+R of those tables
        (project_args_set_row0 moves that window)."""
        P, R, D = y_in.shape
        c0, d = cols if cols is not None else (0, D)
        if not (1 <= d <= MAX_ROW_DIM) or c0 < 0 or c0 + d > D or not (1 <= len(sets) <= MAX_SETS):
            raise ValueError("project_rows: unsupported row / set dimensions")
        _dense(y_in, (P, R, D), "y_in"), _dense(y_out, (P, R, D), "y_out")
        esz = y_in.element_size() if _is_torch(y_in) else y_in.itemsize
        a = ProjectArgs(P=P, R=R, d=d, nsets=len(sets), max_iter=int(max_iter), rho=float(rho), threshold=float(threshold),
                        algorithm=int(algorithm))
        if row_mask is not None:
            if tuple(row_mask.shape) != (R,):
                raise ValueError("row_mask must be int32[R]")
            a.row_mask = _ptr(row_mask)
        a.y_in, a.y_out = _ptr(y_in) + c0 * esz, _ptr(y_out) + c0 * esz
        a.in_sp = a.out_sp = R * D
        a.in_sr = a.out_sr = D
        keep, row_ops = [], []
        direct = int(algorithm) == ALG_ADMM and len(sets) == 1 and sets[0].get("A") is None
        for i, st in enumerate(sets):
            c = a.sets[i]
            c.kind, c.dim = int(st["kind"]), int(st["dim"])
            kind = c.kind                                        # the primitive; c.kind takes the flag bits below
            if kind & ~0xff:
                raise ValueError(f"sets[{i}].kind: a SET_* primitive; per-row tables are asked for with par_rows / b_rows")
            for name, core in (("A", (c.dim, d)), ("b", (c.dim,)), ("par", None)):
                arr = st.get(name)
                if arr is None:
                    if st.get(name + "_rows"):
                        raise ValueError(f"sets[{i}].{name}_rows without sets[{i}].{name}" +
                                         (": SET_SOC_UNIT has no parameters" if name == "par" else ""))
                    continue
                if name != "A" and st.get(name + "_rows"):       # one block per row: [Rtot, W] or [P, Rtot, W]
                    if name == "par":
                        if kind == SET_SOC_UNIT:
                            raise ValueError(f"sets[{i}].par_rows: SET_SOC_UNIT has no parameters")
                        W = st.get("par_words") or _row_par_words(kind, c.dim, arr, f"sets[{i}].par")
                    else:
                        if direct or int(algorithm) == ALG_DYKSTRA:
                            raise ValueError(f"sets[{i}].b_rows: b is not used by the direct form and by ALG_DYKSTRA")
                        W = c.dim
                    if arr.ndim not in (2, 3) or arr.shape[-1] != W or (arr.ndim == 3 and arr.shape[0] != P):
                        raise ValueError(f"sets[{i}].{name}: with {name}_rows=True [Rtot, {W}] or [{P}, Rtot, {W}], got "
                                         f"{tuple(arr.shape)}")
                    if not _contiguous(arr):
                        raise ValueError(f"sets[{i}].{name}: must be C-contiguous")
                    Rtot = int(arr.shape[-2])
                    c.kind |= SET_ROW_PAR if name == "par" else SET_ROW_B
                    setattr(c, name + "_sp", Rtot * W if arr.ndim == 3 else 0)
                    row_ops.append((i, name, _ptr(arr), W * esz, Rtot))
                    keep.append(arr)
                    continue
                per = arr.ndim == (len(core) + 1 if core is not None else 2)
                if core is not None:
                    _dense(arr, ((P,) + core) if per else core, f"sets[{i}].{name}")
                elif per and arr.shape[0] != P:
                    raise ValueError(f"sets[{i}].par: leading axis must be P")
                setattr(c, name, _ptr(arr))
                setattr(c, name + "_sp", int(arr[0].numel() if _is_torch(arr) else arr[0].size) if per else 0)
                keep.append(arr)
        a.iters, a.active = _ptr(iters), _ptr(active)
        if next_stage is not None:                               # a ProjectArgs applied in place to this stage's output
            a.next = C.addressof(next_stage)
        a._keep = keep + [row_mask, next_stage]
        a._row_ops, a._next_stage, a._row0 = row_ops, next_stage, 0
        Kernels._point_rows(a, int(row0))
        a._spec = dict(sets=sets, rho=rho, max_iter=max_iter, threshold=threshold, cols=(c0, d), algorithm=int(algorithm),
                       row_mask=row_mask, next_stage=next_stage, row0=int(row0))                 # to rebuild elsewhere
        return a

    @staticmethod
    def _point_rows(a, row0):
        """the flagged operands of ONE stage -> the window of their tables that starts at row `row0`"""
        for i, name, base, stride, Rtot in a._row_ops:
            if row0 < 0 or row0 + a.R > Rtot:
                raise IslsError(f"sets[{i}].{name}: rows {row0} .. {row0 + a.R} of a per-row table of {Rtot} rows; pad the table "
                                "(repeat its last row) so that it covers the horizon at every step")
        for i, name, base, stride, Rtot in a._row_ops:
            setattr(a.sets[i], name, base + row0 * stride)
        a._row0 = row0

    @staticmethod
    def project_args_set_row0(a, row0):
        """Move the window of the per-row tables of a descriptor and of every stage behind it (`next`) to start at row `row0`:
        a host-side update of the pointers in the descriptors -- base + row0 * Wp * element size for every flagged operand --,
        which the library reads at each call.  No kernel, no copy, no synchronisation.  Returns the descriptor."""
        st = a
        while st is not None:
            Kernels._point_rows(st, int(row0))
            st = st._next_stage
        return a

    @staticmethod
    def project_args_per_row(a):
        """True if any stage of the descriptor carries a per-row table"""
        st = a
        while st is not None:
            if st._row_ops:
                return True
            st = st._next_stage
        return False

    @staticmethod
    def project_args_chain(y_in, y_out, stages, wrap=lambda a: a, iters=None, active=None):
        """Descriptor of a `projections.ConvexSets` with all its stages (`.then` chain): the stages run in order, in place on
        the first stage's output.  `wrap` moves a numpy operand to where the library expects it (device tensor / identity)."""
        R = y_in.shape[1]
        nxt = None
        for k in range(len(stages) - 1, -1, -1):
            cs = stages[k]
            if cs.cols != stages[0].cols:
                raise ValueError("the stages of a ConvexSets chain must act on the same coordinate block")
            sets = [{k_: (wrap(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v) for k_, v in st.items()} for st in cs.sets]
            for i, (st, dst) in enumerate(zip(cs.sets, sets)):    # the block width from the host's table: no read of the device
                if st.get("par_rows") and isinstance(st.get("par"), np.ndarray):
                    dst["par_words"] = _row_par_words(int(st["kind"]), int(st["dim"]), st["par"], f"sets[{i}].par")
            mask = cs.row_mask(R)
            nxt = Kernels.project_args(y_in if k == 0 else y_out, y_out, sets, rho=cs.rho, max_iter=cs.max_iter, threshold=cs.threshold,
                                       iters=iters if k == 0 else None, active=active, cols=cs.cols, algorithm=cs.algorithm,
                                       row_mask=None if mask is None else wrap(mask), next_stage=nxt, row0=stages[0].row0)
        return nxt

    def project_rows(self, y_in, y_out, sets, stream=None, **kw):
        a = self.project_args(y_in, y_out, sets, **kw)
        return self._call("project_rows", _sfx(y_in), a, stream)

    def sls_admm(self, Linv, r_side, rr, sets, x_u, stream=None, **kw):
        """isls_sls_admm: Linv [R,R], r_side [P,R,D], rr [R], sets as in project_args (A [dim,D] or [P,dim,D] ...)."""
        return self._call("sls_admm", _sfx(r_side), self.sls_admm_args(Linv, r_side, rr, sets, x_u, **kw), stream)

    @staticmethod
    def sls_admm_args(Linv, r_side, rr, sets, x_u, alpha=1.0, tol=1e-3, max_iter=50, rho=1.0, inner_max_iter=200,
                      threshold=1e-4, z=None, lmb=None, logs=None, iters=None, rel_tol=1e-2):
        """isls_sls_admm_args for the operands of sls_admm"""
        P, R, D = r_side.shape
        _dense(Linv, (R, R), "Linv"), _dense(rr, (R,), "rr"), _dense(x_u, (P, R, D), "x_u")
        pa = Kernels.project_args(x_u, x_u, sets, rho=rho, max_iter=inner_max_iter, threshold=threshold)
        a = SlsAdmmArgs(P=P, R=R, D=D, max_iter=int(max_iter), alpha=float(alpha), tol=float(tol), rel_tol=float(rel_tol),
                        proj=pa)
        a.Linv, a.r_side, a.rr = _ptr(Linv), _ptr(_dense(r_side, (P, R, D), "r_side")), _ptr(rr)
        a.x_u, a.z, a.lmb = _ptr(x_u), _ptr(_dense(z, (P, R, D), "z")), _ptr(_dense(lmb, (P, R, D), "lmb"))
        a.logs, a.iters = _ptr(_dense(logs, (P, int(max_iter), 2), "logs")), _ptr(iters)
        a._keep = pa
        return a

    def dense_closed_loop(self, model, model_par, K, k, x0, x_log, u_log, xhat=None, uhat=None, stream=None):
        """isls_dense_closed_loop: K [N m, N n], k [N m], x0 [M,n], nominal xhat [N,n] / uhat [N,m] of one problem."""
        M, N, n = x_log.shape
        m = u_log.shape[2]
        a = DenseLoopArgs(M=M, N=N, n=n, m=m, model=int(model))
        a.model_par, a.K, a.k = _ptr(model_par), _ptr(_dense(K, (N * m, N * n), "K")), _ptr(_dense(k, (N * m,), "k"))
        a.xhat, a.uhat = _ptr(_dense(xhat, (N, n), "xhat")), _ptr(_dense(uhat, (N, m), "uhat"))
        a.x0, a.x_log, a.u_log = _ptr(_dense(x0, (M, n), "x0")), _ptr(x_log), _ptr(_dense(u_log, (M, N, m), "u_log"))
        return self._call("dense_closed_loop", _sfx(x_log), a, stream)

    def sls_controller(self, A, Bm, PHI_U, du, K, k, flags, work, stream=None):
        """isls_sls_controller: PHI_U / K [B, N m, N n], du / k [B, N m], flags int32 [B], A / Bm broadcastable views
        [.,.,n,n] / [.,.,n,m], work >= sls_controller_work_elems(B, N, n) contiguous elements of the same dtype."""
        B, R, Cn = PHI_U.shape
        n = Bm.shape[-2]
        m = Bm.shape[-1]
        N = R // m
        if R != N * m or Cn != N * n:
            raise ValueError(f"PHI_U: shape {tuple(PHI_U.shape)} is not [B, N m, N n] for n={n}, m={m}")
        a = SlsControllerArgs(B=B, N=N, n=n, m=m)
        a.A, a.Bm = make_view(A, B, N, (n, n), "A"), make_view(Bm, B, N, (n, m), "B")
        a.PHI_U, a.du = _ptr(_dense(PHI_U, (B, R, Cn), "PHI_U")), _ptr(_dense(du, (B, R), "du"))
        a.K, a.k = _ptr(_dense(K, (B, R, Cn), "K")), _ptr(_dense(k, (B, R), "k"))
        a.flags = _ptr(_dense(flags, (B,), "flags"))
        size = work.numel() if _is_torch(work) else work.size
        if size < sls_controller_work_elems(B, N, n) or not _contiguous(work):
            raise ValueError(f"work: needs a contiguous buffer of {sls_controller_work_elems(B, N, n)} elements")
        a.work = _ptr(work)
        return self._call("sls_controller", _sfx(PHI_U), a, stream)

    def columns_rollout(self, *args, stream=None, **kw):
        return self._call("columns_rollout", _sfx(args[6]), self.columns_args(*args, **kw), stream)

    @staticmethod
    def columns_args(A, Bm, Cuu, c0u, K, k, dx, du, Rr=None, zu=None, lu=None, active=None):
        """isls_columns_rollout: k, dx, du column-major [C,B,N,.]; A, Bm, Cuu, c0u, Rr broadcastable views."""
        Cc, B, N, n = dx.shape
        m = du.shape[3]
        a = ColumnsArgs(B=B, N=N, n=n, m=m, C=Cc)
        a.A, a.Bm = make_view(A, B, N, (n, n), "A"), make_view(Bm, B, N, (n, m), "B")
        a.Cuu, a.c0u = make_view(Cuu, B, N, (m, m), "Cuu"), make_view(c0u, B, N, (m,), "c0u")
        a.Rr = make_view(Rr, B, N, (m, m), "Rr")
        a.K, a.k = _ptr(_dense(K, (B, N, m, n), "K")), _ptr(_dense(k, (Cc, B, N, m), "k"))
        a.zu, a.lu = _ptr(_dense(zu, (Cc, B, N, m), "zu")), _ptr(_dense(lu, (Cc, B, N, m), "lu"))
        a.dx, a.du = _ptr(_dense(dx, (Cc, B, N, n), "dx")), _ptr(_dense(du, (Cc, B, N, m), "du"))
        a.active = _ptr(active)
        return a

    def columns_admm(self, phase, dims, res, res_prev, x=None, u=None, stream=None, **kw):
        a = self.columns_admm_args(phase, dims, res, res_prev, x=x, u=u, **kw)
        return self._call("columns_admm", _sfx((x or u)["xx"]), a, stream)

    @staticmethod
    def columns_admm_args(phase, dims, res, res_prev, x=None, u=None, relax=1.0, tol_abs=0.0, tol_rel=1e-3, active=None, iters=None):
        """isls_columns_admm; dims = (B, N, n, m, C); x / u: dict(xx, z, l, z_prev, work, W, nom=None) or None."""
        B, N, n, m, Cc = dims
        a = ColumnsAdmmArgs(B=B, N=N, n=n, m=m, C=Cc, phase=int(phase), relax=float(relax), tol_abs=float(tol_abs),
                            tol_rel=float(tol_rel))
        for blk, d, names in ((x, n, ("xx", "zx", "lx", "zx_prev", "x_nom", "x_work", "Qr")),
                              (u, m, ("xu", "zu", "lu", "zu_prev", "u_nom", "u_work", "Rr"))):
            if blk is None:
                continue
            for key, name in zip(("xx", "z", "l", "z_prev"), names[:4]):
                setattr(a, name, _ptr(_dense(blk[key], (Cc, B, N, d), name)))
            setattr(a, names[4], _ptr(_dense(blk.get("nom"), (B, N, d), names[4])))
            setattr(a, names[5], _ptr(_dense(blk["work"], (B, N * d, Cc), names[5])))
            setattr(a, names[6], make_view(blk["W"], B, N, (d, d), names[6]))
        a.res, a.res_prev = _ptr(_dense(res, (B, 2), "res")), _ptr(_dense(res_prev, (B, 2), "res_prev"))
        a.active, a.iters = _ptr(active), _ptr(iters)
        return a

    @staticmethod
    def columns_iteration_args(ff, cols, ls, admm, proj_x=None, proj_u=None, zero_x=None, zero_u=None, log=None):
        """isls_columns_iteration_args from the blocks of ff_args / columns_args / rollout_args (None: no line search) /
        columns_admm_args (None: unconstrained) and the row-projection descriptors of the two blocks."""
        a = ColumnsIterationArgs(ff=ff, cols=cols)
        if ls is not None:
            a.ls = ls
        if admm is not None:
            a.admm = admm
        a.proj_x = C.addressof(proj_x) if proj_x is not None else None
        a.proj_u = C.addressof(proj_u) if proj_u is not None else None
        a.zero_x, a.zero_u, a.log = _ptr(zero_x), _ptr(zero_u), _ptr(log)
        a._keep = (ff, cols, ls, admm, proj_x, proj_u)
        return a

    def columns_iteration(self, it, sfx, stream=None):
        return self._call("columns_iteration", sfx, it, stream)

    def mc_closed_loop(self, a, sfx, stream=None):
        """isls_mc_closed_loop on a filled McLoopArgs (isls/montecarlo.py builds it)"""
        return self._call("mc_closed_loop", sfx, a, stream)

    @staticmethod
    def _out_col(t, B, d, name):
        """(ptr, batch stride) of an output of isls_mpc_step: [B, d], or a column [:, s] of a [B, T, d] log (unit stride over d)"""
        if t is None:
            return None, 0
        st = _estrides(t)
        if tuple(t.shape) != (B, d) or (d != 1 and st[1] != 1):
            raise ValueError(f"{name}: [{B}, {d}] with contiguous rows, got shape {tuple(t.shape)} strides {st}")
        return _ptr(t), int(st[0]) if B > 1 else d

    @staticmethod
    def mpc_step_args(model, model_par, xhat, uhat, K=None, zx=None, zu=None, plant_par=None, tab=None, tab_next=None,
                      u_lo=None, u_hi=None, w=None, noise_std=None, seed=0, problem0=0, step=0,
                      x_meas_out=None, u_out=None, x_next_out=None):
        """isls_mpc_step_args over the caller's arrays: xhat [B,N,n], uhat [B,N,m], K [B,N,m,n], zx, zu (in/out); tab [N,W] or
        [B,N,W] with tab_next [W] / [B,W]; the outputs [B,.] or columns of [B,T,.] logs."""
        B, N, n = xhat.shape
        m = uhat.shape[2]
        a = MpcStepArgs(B=B, N=N, n=n, m=m, model=int(model), seed=int(seed), problem0=int(problem0), step=int(step))
        a.model_par, a.par_sb = _par(model_par, B, "model_par")
        if plant_par is not None:
            a.plant_par, a.plant_sb = _par(plant_par, B, "plant_par")
        a.xhat, a.uhat = _ptr(_dense(xhat, (B, N, n), "xhat")), _ptr(_dense(uhat, (B, N, m), "uhat"))
        a.K = _ptr(_dense(K, (B, N, m, n), "K"))
        a.zx, a.zu = _ptr(_dense(zx, (B, N, n), "zx")), _ptr(_dense(zu, (B, N, m), "zu"))
        if tab is not None:
            if tab.ndim not in (2, 3):
                raise ValueError(f"tab: [N, W] or [B, N, W], got shape {tuple(tab.shape)}")
            a.W = int(tab.shape[-1])
            a.tab, a.tab_sb = _tab(tab, B, (N, a.W), "tab")
            if tab_next is not None:
                a.tab_next, a.tab_next_sb = _tab(tab_next, B, (a.W,), "tab_next")
                if (a.tab_sb == 0) != (a.tab_next_sb == 0):
                    raise ValueError("tab_next: shared with a shared table, per trajectory with a per-trajectory one")
        elif tab_next is not None:
            raise ValueError("tab_next without tab")
        a.u_lo, a.u_hi = _ptr(_dense(u_lo, (m,), "u_lo")), _ptr(_dense(u_hi, (m,), "u_hi"))
        a.w, a.noise_std = _ptr(_dense(w, (B, n), "w")), _ptr(_dense(noise_std, (n,), "noise_std"))
        a.x_meas_out, a.x_meas_sb = Kernels._out_col(x_meas_out, B, n, "x_meas_out")
        a.u_out, a.u_out_sb = Kernels._out_col(u_out, B, m, "u_out")
        a.x_next_out, a.x_next_sb = Kernels._out_col(x_next_out, B, n, "x_next_out")
        return a

    def mpc_step(self, model, model_par, xhat, uhat, stream=None, **kw):
        """isls_mpc_step: the first control through the plant, the plan moved up by one step in place, re-rolled from x+"""
        return self._call("mpc_step", _sfx(xhat), self.mpc_step_args(model, model_par, xhat, uhat, **kw), stream)

    @staticmethod
    def _stat_col(t, B, name):
        """(ptr, batch stride) of a per-problem statistic of isls_sample_nominal: [B], or a column [:, r] of a [B, rounds] log"""
        if t is None:
            return None, 0
        if tuple(t.shape) != (B,):
            raise ValueError(f"{name}: [{B}], got shape {tuple(t.shape)}")
        return _ptr(t), int(_estrides(t)[0]) if B > 1 else 1

    @staticmethod
    def sample_args(model, model_par, xhat, uhat, Qtab, ztab, seq, u_std, sigma, costs, cost_model=COST_VIA, cost_par=None,
                    cost_tab=None, u_lo=None, u_hi=None, temperature=1.0, seed=0, problem0=0, active=None, cost_before=None,
                    cost_after=None, cost_best=None, ess=None, took_best=None, problem_ids=None, phase=0):
        """isls_sample_args over the caller's arrays: xhat [B,N,n], uhat [B,N,m] (in/out), sigma [m] or [B,m], costs [B,S]; the
        statistics [B] or columns of [B, rounds] logs (one batch stride for all of them); problem_ids [B] int32: the draws'
        problem counters; phase 1 / 2: the cost launch / the update launch alone."""
        B, N, n = xhat.shape
        m = uhat.shape[2]
        nvia = int(Qtab.shape[-3])
        a = SampleArgs(B=B, N=N, n=n, m=m, S=int(costs.shape[1]), model=int(model), cost_model=int(cost_model), nvia=nvia,
                       u_std=float(u_std), temperature=float(temperature), seed=int(seed), problem0=int(problem0), phase=int(phase))
        a.problem_ids = _ptr(_dense(problem_ids, (B,), "problem_ids"))
        a.model_par, a.model_par_sb = _par(model_par, B, "model_par")
        a.cost_par, a.cost_par_sb = _cost_par(cost_model, cost_par, B)
        a.xhat, a.uhat = _ptr(_dense(xhat, (B, N, n), "xhat")), _ptr(_dense(uhat, (B, N, m), "uhat"))
        a.Qtab, a.Qtab_sb = _tab(Qtab, B, (nvia, n, n), "Qtab")
        a.ztab, a.ztab_sb = _tab(ztab, B, (nvia, n), "ztab")
        a.seq = _ptr(seq)
        _cost_tab(a, cost_model, cost_tab)
        a.sigma, a.sigma_sb = _tab(sigma, B, (m,), "sigma")
        a.u_lo, a.u_hi = _ptr(_dense(u_lo, (m,), "u_lo")), _ptr(_dense(u_hi, (m,), "u_hi"))
        a.active = _ptr(active)
        a.costs = _ptr(_dense(costs, (B, a.S), "costs"))
        strides = set()
        for name, t in (("cost_before", cost_before), ("cost_after", cost_after), ("cost_best", cost_best), ("ess", ess),
                        ("took_best", took_best)):
            ptr, sb = Kernels._stat_col(t, B, name)
            setattr(a, name, ptr)
            if t is not None:
                strides.add(sb)
        if len(strides) > 1:
            raise ValueError("the statistics of isls_sample_nominal share one batch stride")
        a.stat_sb = strides.pop() if strides else 1
        return a

    def sample_nominal(self, model, model_par, xhat, uhat, *args, stream=None, **kw):
        """isls_sample_nominal: one sampling round about (xhat, uhat), in place"""
        return self._call("sample_nominal", _sfx(xhat), self.sample_args(model, model_par, xhat, uhat, *args, **kw), stream)

    def sample_nominal_fb(self, model, model_par, xhat, uhat, *args, K, stream=None, **kw):
        """isls_sample_nominal_fb: the round in closed loop about the gains K [N,m,n] (shared) or [B,N,m,n], in place"""
        a = self.sample_args(model, model_par, xhat, uhat, *args, **kw)
        if K is None:
            raise ValueError("K: the gains [N, m, n] or [B, N, m, n]")
        if K.dtype != xhat.dtype:
            raise ValueError(f"K: dtype {xhat.dtype}, got {K.dtype}")
        ptr, sb = _tab(K, a.B, (a.N, a.m, a.n), "K")
        return self._invoke("sample_nominal_fb", _sfx(xhat), C.byref(a), C.c_void_p(ptr), C.c_int64(sb), stream=stream)

    def cov_closed_loop(self, a, sfx, stream=None):
        """isls_cov_closed_loop on a filled CovArgs (isls/covariance.py builds it)"""
        return self._call("cov_closed_loop", sfx, a, stream)

    def sls_closed_loop(self, A, Bm, K, k, x0, x_log, u_log, stream=None):
        M, N, n = x_log.shape
        m = u_log.shape[2]
        _dense(A, (n, n), "A"), _dense(Bm, (n, m), "B"), _dense(K, (N * m, N * n), "K"), _dense(k, (N * m,), "k")
        _dense(x0, (M, n), "x0"), _dense(u_log, (M, N, m), "u_log")
        return self._invoke("sls_closed_loop", _sfx(x_log), C.c_int32(M), C.c_int32(N), C.c_int32(n), C.c_int32(m),
                            *(C.c_void_p(_ptr(t)) for t in (A, Bm, K, k, x0, x_log, u_log)), stream=stream)

    def riccati_ff_prepare(self, *args, stream=None, **kw):
        a = self.ff_prepare_args(*args, **kw)
        return self._call("riccati_ff_prepare", _sfx(args[2]), a, stream)

    def ff_segments(self, N, nseg_requested):
        """(nseg, seg_len) the library uses for a horizon of N steps."""
        seg_len = C.c_int32(0)
        nseg = int(self.lib.isls_ff_segments(C.c_int32(int(N)), C.c_int32(int(nseg_requested)), C.byref(seg_len)))
        return nseg, int(seg_len.value)

    def rollout_ls(self, *args, stream=None, **kw):
        a = self.rollout_args(*args, **kw)
        return self._call("rollout_ls", _sfx(args[2]), a, stream)

    def admm_update(self, *args, stream=None, **kw):
        a = self.admm_args(*args, **kw)
        return self._call("admm_update", _sfx(args[0]), a, stream)

    def expand_quadratic(self, *args, stream=None, **kw):
        return self._call("expand_quadratic", _sfx(args[4]), self.expand_args(*args, **kw), stream)

    @staticmethod
    def expand_args(Qtab, ztab, seq, u_std, c0x, c0u, xhat=None, uhat=None, Cxx=None, Cuu=None,
                    Qr=None, Rr=None, cost=None, active=None, cost_model=COST_VIA, cost_par=None, q_nonzero=None,
                    cost_tab=None):
        B, N, n = c0x.shape
        m = c0u.shape[2]
        nvia = int(Qtab.shape[-3])
        a = ExpandArgs(B=B, N=N, n=n, m=m, nvia=nvia, u_std=float(u_std))
        a.Qtab, a.Qtab_sb = _tab(Qtab, B, (nvia, n, n), "Qtab")
        a.ztab, a.ztab_sb = _tab(ztab, B, (nvia, n), "ztab")
        a.seq = _ptr(seq)
        a.Qr, a.Rr = make_view(Qr, B, N, (n, n), "Qr"), make_view(Rr, B, N, (m, m), "Rr")
        a.xhat, a.uhat = _ptr(_dense(xhat, (B, N, n), "xhat")), _ptr(_dense(uhat, (B, N, m), "uhat"))
        a.Cxx, a.Cuu = _ptr(_dense(Cxx, (B, N, n, n), "Cxx")), _ptr(_dense(Cuu, (B, N, m, m), "Cuu"))
        a.c0x, a.c0u = _ptr(_dense(c0x, (B, N, n), "c0x")), _ptr(_dense(c0u, (B, N, m), "c0u"))
        a.cost, a.active = _ptr(_dense(cost, (B,), "cost")), _ptr(active)
        a.cost_model, a.q_nonzero = int(cost_model), _ptr(q_nonzero)
        a.cost_par, a.cost_par_sb = _cost_par(cost_model, cost_par, B)
        _cost_tab(a, cost_model, cost_tab)
        return a

    def linearize(self, *args, stream=None, **kw):
        return self._call("linearize", _sfx(args[2]), self.linearize_args(*args, **kw), stream)

    @staticmethod
    def linearize_args(model, model_par, xhat, uhat, A, Bm, active=None):
        B, N, n = xhat.shape
        m = uhat.shape[2]
        a = LinearizeArgs(B=B, N=N, n=n, m=m, model=model)
        a.model_par, a.model_par_sb = _par(model_par, B, "model_par")
        a.xhat, a.uhat = _ptr(_dense(xhat, (B, N, n), "xhat")), _ptr(_dense(uhat, (B, N, m), "uhat"))
        a.A, a.Bm = _ptr(_dense(A, (B, N, n, n), "A")), _ptr(_dense(Bm, (B, N, n, m), "B"))
        a.active = _ptr(active)
        return a

    def accept_step(self, *args, stream=None, **kw):
        return self._call("accept_step", _sfx(args[0]), self.accept_args(*args, **kw), stream)

    @staticmethod
    def accept_args(xx, xu, cost_new, xhat, uhat, cost, cost_hist=None, hist_len=None, tol_cost=-1.0,
                    tol_osc=-1.0, outer_active=None):
        B, N, n = xx.shape
        m = xu.shape[2]
        a = AcceptArgs(B=B, N=N, n=n, m=m, tol_cost=float(tol_cost), tol_osc=float(tol_osc))
        a.xx, a.xu = _ptr(_dense(xx, (B, N, n), "xx")), _ptr(_dense(xu, (B, N, m), "xu"))
        a.cost_new = _ptr(_dense(cost_new, (B,), "cost_new"))
        a.xhat, a.uhat = _ptr(_dense(xhat, (B, N, n), "xhat")), _ptr(_dense(uhat, (B, N, m), "uhat"))
        a.cost = _ptr(_dense(cost, (B,), "cost"))
        a.cost_hist, a.hist_len = _ptr(_dense(cost_hist, (B, 8), "cost_hist")), _ptr(hist_len)
        a.outer_active = _ptr(outer_active)
        return a

    @staticmethod
    def advance_args(accept, lin=None, exp=None, admm_active=None, iters=None, lx=None, lu=None, res_prev=None):
        """isls_advance_args from the blocks of accept_args / linearize_args / expand_args (lin / exp None: that stage is skipped)"""
        a = AdvanceArgs(accept=accept)
        if lin is not None:
            a.lin = lin
        if exp is not None:
            a.exp = exp
        a.admm_active, a.iters, a.lx, a.lu, a.res_prev = _ptr(admm_active), _ptr(iters), _ptr(lx), _ptr(lu), _ptr(res_prev)
        a._keep = (accept, lin, exp)
        return a

    def user_model_step(self, model_id, par, x, u, xn, stream=None):
        """isls_user_model_step: xn [R,n] = f(x [R,n], u [R,m]) with par [P] (shared) or [R,P]."""
        R, n = xn.shape
        _dense(x, (R, n), "x"), _dense(u, (R, u.shape[1]), "u")
        ptr, sb = _par(par, R, "par")
        return self._invoke("user_model_step", _sfx(xn), C.c_int32(model_id), C.c_int32(R), C.c_void_p(ptr), C.c_int64(sb),
                            C.c_void_p(_ptr(x)), C.c_void_p(_ptr(u)), C.c_void_p(_ptr(xn)), stream=stream)

    def user_model_step_tab(self, model_id, par, x, u, xn, run, N, t=None, stream=None):
        """isls_user_model_step_tab: xn [R,n] = f(x [R,n], u [R,m]; row) of a table model; the rows come in runs of `run` per
        parameter block par [P + N W] (shared) or [R / run, P + N W]; row r takes table row t[r] (int32 [R]) or r % run."""
        R, n = xn.shape
        _dense(x, (R, n), "x"), _dense(u, (R, u.shape[1]), "u")
        if t is not None:
            _dense(t, (R,), "t")
        ptr, sb = _par(par, R // int(run), "par")
        return self._invoke("user_model_step_tab", _sfx(xn), C.c_int32(model_id), C.c_int32(R), C.c_int32(int(run)), C.c_int32(int(N)),
                            C.c_void_p(ptr), C.c_int64(sb), C.c_void_p(_ptr(t)), C.c_void_p(_ptr(x)), C.c_void_p(_ptr(u)),
                            C.c_void_p(_ptr(xn)), stream=stream)

    def user_cost_value(self, cost_id, par, x, u, cost, stream=None, tab=None):
        """isls_user_cost_value: cost [R] = sum_t stage(x [R,N,n], u [R,N,m]) with par [P] (shared) or [R,P]; a cost with a table
        (isls_user_cost_value_tab): tab [N,W] (shared) or [R,N,W]."""
        R, N, n = x.shape
        _dense(u, (R, N, u.shape[2]), "u"), _dense(cost, (R,), "cost")
        ptr, sb = _par(par, R, "par")
        if tab is not None:
            tptr, tsb = _tab(tab, R, (N, int(tab.shape[-1])), "tab")
            return self._invoke("user_cost_value_tab", _sfx(cost), C.c_int32(cost_id), C.c_int32(R), C.c_int32(N), C.c_void_p(ptr),
                                C.c_int64(sb), C.c_void_p(tptr), C.c_int64(tsb), C.c_void_p(_ptr(x)), C.c_void_p(_ptr(u)),
                                C.c_void_p(_ptr(cost)), stream=stream)
        return self._invoke("user_cost_value", _sfx(cost), C.c_int32(cost_id), C.c_int32(R), C.c_int32(N), C.c_void_p(ptr), C.c_int64(sb),
                            C.c_void_p(_ptr(x)), C.c_void_p(_ptr(u)), C.c_void_p(_ptr(cost)), stream=stream)

    def user_constraint_update(self, cost_id, par, tab, xhat, uhat, viol, viol_prev, update=True, eta=0.25, phi=10.0, mu_max=1e8,
                               g_out=None, active=None, stream=None):
        """isls_user_constraint_update: the multiplier and penalty update of a cost with K constraints along xhat [B,N,n], uhat
        [B,N,m], INTO tab [B,N,W+K+1]; viol, viol_prev [B]; g_out [B,N,K] or None; update=False evaluates only."""
        B, N, n = xhat.shape
        m = int(uhat.shape[2])
        _dense(xhat, (B, N, n), "xhat"), _dense(uhat, (B, N, m), "uhat"), _dense(tab, (B, N, int(tab.shape[-1])), "tab")
        _dense(viol, (B,), "viol"), _dense(viol_prev, (B,), "viol_prev")
        for name, v in (("par", par), ("xhat", xhat), ("uhat", uhat), ("viol", viol), ("viol_prev", viol_prev), ("g_out", g_out)):
            if v is not None and v.dtype != tab.dtype:
                raise ValueError(f"{name}: dtype {v.dtype}, the table is {tab.dtype}")
        if active is not None and _sfx_int(active) != "i32":
            raise ValueError(f"active: int32, got {active.dtype}")
        a = ConstraintUpdateArgs()
        a.B, a.N, a.n, a.m, a.cost_model, a.update = B, N, n, m, int(cost_id), int(bool(update))
        a.cost_par, a.cost_par_sb = _par(par, B, "par")
        a.tab, a.tab_sb = _ptr(tab), N * int(tab.shape[-1])
        a.xhat, a.uhat, a.viol, a.viol_prev = _ptr(xhat), _ptr(uhat), _ptr(viol), _ptr(viol_prev)
        if g_out is not None:
            a.g_out = _ptr(_dense(g_out, (B, N, int(g_out.shape[-1])), "g_out"))
        a.eta, a.phi, a.mu_max = float(eta), float(phi), float(mu_max)
        if active is not None:
            a.active = _ptr(_dense(active, (B,), "active"))
        return self._call("user_constraint_update", _sfx(tab), a, stream)

    def adjoint_sweep(self, A, Bm, c0x, c0u, lam, gu, gx0=None, active=None, stream=None):
        """isls_adjoint_sweep: costate lam [B,N,n], gu [B,N,m], gx0 [B,n] from A [B|1,N,n,n] / [N,n,n] / [n,n], Bm likewise,
        c0x [B,N,n], c0u [B,N,m]."""
        B, N, n = c0x.shape
        m = int(c0u.shape[2])
        a = AdjointArgs(B=B, N=N, n=n, m=m)
        a.A, a.Bm = make_view(A, B, N, (n, n), "A"), make_view(Bm, B, N, (n, m), "B")
        a.c0x, a.c0u = _ptr(_dense(c0x, (B, N, n), "c0x")), _ptr(_dense(c0u, (B, N, m), "c0u"))
        a.lam, a.gu = _ptr(_dense(lam, (B, N, n), "lam")), _ptr(_dense(gu, (B, N, m), "gu"))
        a.gx0 = _ptr(_dense(gx0, (B, n), "gx0")) if gx0 is not None else None
        for name, v in (("A", A), ("B", Bm), ("c0u", c0u), ("lam", lam), ("gu", gu), ("gx0", gx0)):
            if v is not None and v.dtype != c0x.dtype:
                raise ValueError(f"{name}: dtype {v.dtype}, c0x is {c0x.dtype}")
        a.active = _ptr(active)
        return self._call("adjoint_sweep", _sfx(c0x), a, stream)

    def user_grad(self, noun, uid, par, xhat, uhat, lam=None, tab=None, g_par=None, g_tab=None, active=None, stream=None):
        """isls_user_{model,cost}_grad (noun: "model" | "cost"): g_par [B,P], g_tab [B,N,W] (None: not computed) along xhat, uhat;
        par: the model's block [par | rows] or the cost's parameters, [.] or [B,.]; tab: the cost's table [N,.] or [B,N,.]."""
        B, N, n = xhat.shape
        m = int(uhat.shape[2])
        a = UserGradArgs(B=B, N=N, n=n, m=m, id=int(uid))
        a.par, a.par_sb = _par(par, B, "par")
        if tab is not None:
            a.tab, a.tab_sb = _tab(tab, B, (N, int(tab.shape[-1])), "tab")
        a.xhat, a.uhat = _ptr(_dense(xhat, (B, N, n), "xhat")), _ptr(_dense(uhat, (B, N, m), "uhat"))
        a.lam = _ptr(_dense(lam, (B, N, n), "lam")) if lam is not None else None
        a.g_par = _ptr(_dense(g_par, (B, int(g_par.shape[-1])), "g_par")) if g_par is not None else None
        a.g_tab = _ptr(_dense(g_tab, (B, N, int(g_tab.shape[-1])), "g_tab")) if g_tab is not None else None
        for name, v in (("par", par), ("tab", tab), ("uhat", uhat), ("lam", lam), ("g_par", g_par), ("g_tab", g_tab)):
            if v is not None and v.dtype != xhat.dtype:
                raise ValueError(f"{name}: dtype {v.dtype}, xhat is {xhat.dtype}")
        a.active = _ptr(active)
        return self._call(f"user_{noun}_grad", _sfx(xhat), a, stream)

    def user_cost_expand(self, exp, Cux, sfx, stream=None):
        """isls_user_cost_expand: `exp` an expand_args block whose cost_model is the cost's id; Cux [B,N,m,n] or None."""
        if Cux is not None:
            _dense(Cux, (exp.B, exp.N, exp.m, exp.n), "Cux")
        return self._invoke("user_cost_expand", sfx, C.byref(exp), C.c_void_p(_ptr(Cux)), stream=stream)

    def outer_advance(self, adv, sfx, stream=None):
        return self._call("outer_advance", sfx, adv, stream)

    def _reduce(self, name, cost, res, active, status, out, *tail, stream):
        B = int(cost.shape[0]) if cost is not None else int(res.shape[0])
        return self._invoke(name, _sfx(out), C.c_int32(B), *(C.c_void_p(_ptr(t)) for t in (cost, res, active, status, out)), *tail,
                            stream=stream)

    def reduce_convergence(self, cost, res, active, status, out5, stream=None):
        return self._reduce("reduce_convergence", cost, res, active, status, out5, stream=stream)

    def reduce_convergence_table(self, cost, res, active, status, table, rank, stream=None):
        """isls_reduce_convergence_table: the shard's five numbers into row `rank` of the [W,5] table, other rows zeroed."""
        world = int(table.shape[0])
        _dense(table, (world, 5), "table")
        return self._reduce("reduce_convergence_table", cost, res, active, status, table, C.c_int32(int(rank)), C.c_int32(world),
                            stream=stream)

    def outer(self, gain, ff, ro, admm, J, sfx, skip_gain=False, log=None, outer_active=None, begin_done=False, stream=None):
        a = OuterArgs(gain=gain, ff=ff, ro=ro, admm=admm, J=int(J), skip_gain=int(bool(skip_gain)), begin_done=int(bool(begin_done)))
        a.log, a.outer_active = _ptr(log), _ptr(outer_active)
        return self._call("ilqr_admm_outer", sfx, a, stream)
