"""The C ABI of include/*.h as Python states it - the ONE place that mirrors the headers: their structures, their integer constants under the headers' own names, and
one table of every entry point with its return and argument types.  runtime.py types the libraries' functions from the table and spells every flag, status bit and
error code by these names; tests/test_abi_table.py parses the headers and holds every line below against them (names, prototypes argument by argument, struct
fields, constants, the symbols the built libraries export).  A new entry point is one line in ENTRY_POINTS; a new extension header is one more key."""
import ctypes as C


# ---- structures: field for field the typedefs of the headers ----------------------------------------------------------------------------------------------------
class PdpMat(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("bstride", C.c_int64), ("tstride", C.c_int64)]


class PdpLqrProblem(C.Structure):
    _fields_ = [("B", C.c_int), ("T", C.c_int), ("n", C.c_int), ("m", C.c_int), ("p", C.c_int)] + \
               [(k, PdpMat) for k in ("F", "G", "E", "Hxx", "Hxu", "Hxe", "Huu", "Hue", "hxx", "hxe", "X0")]


class PdpModelInfo(C.Structure):
    _fields_ = [("kind", C.c_int), ("n", C.c_int), ("m", C.c_int), ("p", C.c_int), ("nnz_path", C.c_int), ("chunk", C.c_int),
                ("name", C.c_char_p)]


class PdpOcAuxsys(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("dynF", "dynG", "dynE", "Hxx", "Hxu", "Hxe", "Hux", "Huu", "Hue", "hxx", "hxe", "dHu", "Huu_damp")]


class PdpOcSolveOpts(C.Structure):
    _fields_ = [("tol", C.c_double), ("newton_switch", C.c_double), ("max_iter", C.c_int), ("check_every", C.c_int), ("ls_trials", C.c_int),
                ("straggler_patience", C.c_int), ("print_level", C.c_int)]


class PdpOcMsOpts(C.Structure):
    _fields_ = [("tol", C.c_double), ("max_iter", C.c_int), ("flags", C.c_int), ("log_rows", C.c_int), ("dtheta_bstride", C.c_int),
                ("dtheta", C.c_void_p), ("dxdp", C.c_void_p), ("dudp", C.c_void_p), ("riccati", C.c_void_p), ("predict_record", C.c_void_p)]


class PdpOcSensOut(C.Structure):
    _fields_ = [("dxdp", C.c_void_p), ("dudp", C.c_void_p), ("riccati", C.c_void_p), ("predict_record", C.c_void_p), ("grad_x0", C.c_void_p)]


class PdpLmSchedule(C.Structure):                  # include/pdp_hip_lm.h
    _fields_ = [("up", C.c_double), ("down", C.c_double), ("lam_min", C.c_double), ("lam_max", C.c_double), ("loss_tol", C.c_double), ("max_evals", C.c_int32)]


class PdpLmState(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("theta", "trial", "lam", "current", "state", "evaluations", "rejected", "accepted", "accepted_now", "loss_trace",
                                          "lambda_trace", "parameter_trace")] + [("trace_len", C.c_int64), ("counters", C.c_void_p)]


class PdpLmPrior(C.Structure):                     # include/pdp_hip_lm_prior.h
    _fields_ = [("mean", C.c_void_p), ("precision", C.c_void_p), ("kind", C.c_int32), ("mean_kstride", C.c_int64), ("precision_kstride", C.c_int64),
                ("prior_loss", C.c_void_p)]


class PdpPolicy(C.Structure):
    _fields_ = [("kind", C.c_int), ("n_pivots", C.c_int), ("pivots", C.c_double * 16), ("n_layers", C.c_int), ("sizes", C.c_int * 16), ("n_basis", C.c_int),
                ("table", C.c_void_p)]


class PdpPolicyCot(C.Structure):                   # pdp_policy.kind | PDP_POLICY_COTANGENT: pdp_cp_step_batched reads its policy argument as this
    _fields_ = [("pol", PdpPolicy), ("x", C.c_void_p), ("grad_x", C.c_void_p), ("grad_u", C.c_void_p), ("grad_x0", C.c_void_p)]


class PdpPolicyTan(C.Structure):                   # pdp_policy.kind | PDP_POLICY_TANGENT: pdp_cp_step_batched reads its policy argument as this
    _fields_ = [("pol", PdpPolicy), ("x", C.c_void_p), ("u", C.c_void_p), ("d_theta", C.c_void_p), ("d_theta_bstride", C.c_int), ("d_x0", C.c_void_p),
                ("d_x", C.c_void_p), ("d_u", C.c_void_p)]


# ---- constants: every integer-valued #define PDP_* of include/*.h, under the header's name -------------------------------------------------------------------------
PDP_E_ARG, PDP_E_SIZE, PDP_E_LAUNCH, PDP_E_MODE = -1, -2, -3, -4                                # return codes
PDP_STATUS_NONFINITE, PDP_STATUS_PIVOT, PDP_STATUS_INDEFINITE = 1, 2, 256                       # status [B] of the LQR solve and the gradient units
PDP_KIND_OC, PDP_KIND_CP, PDP_KIND_SYSID = 0, 1, 2                                              # pdp_model_info.kind
# pdp_oc_ms_opts.flags: what the solve is asked to do
PDP_MS_WARM, PDP_MS_NO_RESTORATION, PDP_MS_FROM_CONTROLS, PDP_MS_PREDICT, PDP_MS_PREDICT_PRIMAL, PDP_MS_PREDICT_GUARD = 1, 2, 8, 16, 32, 64
PDP_MS_WITH_SOC, PDP_MS_WITH_WATCHDOG = 128, 256
# status [B] of pdp_oc_solve_ms_batched: what happened (beside PDP_STATUS_NONFINITE); the last four are informational
PDP_MS_RESTORATION, PDP_MS_MAXITER, PDP_MS_INERTIA, PDP_MS_NOGAINS, PDP_MS_INTERNAL = 4, 8, 16, 32, 64
PDP_MS_RESTORED, PDP_MS_PREDICT_REJECTED, PDP_MS_SOC, PDP_MS_WATCHDOG = 128, 512, 1024, 2048
# `flags` of the gradient units (pdp_oc_pdp_grad*_batched); the PDP_GRAD_* bits also of the SysID least-squares entry points
PDP_OC_GIVEN_TRAJ, PDP_OC_PACKED, PDP_OC_RECORD_PRIMAL, PDP_OC_COTANGENT = 1, 2, 4, 8
PDP_GRAD_GAUSS_NEWTON, PDP_GRAD_SKIP_MISSING = 16, 32
PDP_POLICY_POLY, PDP_POLICY_MLP, PDP_POLICY_TABLE = 0, 1, 2                                     # pdp_policy.kind
PDP_POLICY_COTANGENT = 256                                                                      # bit of pdp_policy.kind: the struct is the head of a pdp_policy_cot
PDP_POLICY_TANGENT = 512                                                                        # bit of pdp_policy.kind: the struct is the head of a pdp_policy_tan
PDP_LM_START, PDP_LM_ACTIVE, PDP_LM_CONVERGED, PDP_LM_STALLED, PDP_LM_BUDGET, PDP_LM_FAILED = 0, 1, 2, 3, 4, 5      # pdp_lm_state.state (include/pdp_hip_lm.h)

PDP_E = {PDP_E_ARG: "PDP_E_ARG (null pointer / bad size)", PDP_E_SIZE: "PDP_E_SIZE (dimension outside kernel limits)",
         PDP_E_LAUNCH: "PDP_E_LAUNCH (HIP launch failed)", PDP_E_MODE: "PDP_E_MODE (entry point not provided by this model kind)"}
_lm = {k: v for k, v in list(globals().items()) if k.startswith("PDP_LM_")}
LM_STATES = [k[len("PDP_LM_"):] for k in sorted(_lm, key=_lm.get)]                              # the names of pdp_lm_state.state by value: "START", "ACTIVE", ...

# ---- entry points: header -> ((library that exports them: "core" is libpdp_hip.so, "model" every libpdp_model_*.so, {name: (restype, argtypes)} in the header's
#      order), ...); include/pdp_hip.h has a section for either library, every extension header one ------------------------------------------------------------------
_V, _I, _L, _D, _P = C.c_void_p, C.c_int, C.c_int64, C.c_double, C.POINTER
_LM_UPDATE = [_I, _I, _I, _V, _I, _V, _P(PdpLmSchedule), _P(PdpLmState)]
ENTRY_POINTS = {
    "pdp_hip.h": (
        ("core", {
            "pdp_hip_version": (C.c_char_p, []),
            "pdp_lqr_workspace_bytes": (_L, [_I] * 6),
            "pdp_lqr_solve_batched": (_I, [_P(PdpLqrProblem), _V, _V, _V, _V, _V, _L, _V]),
            "pdp_cp_aux_integrate_batched": (_I, [_I] * 5 + [_V] * 8),
            "pdp_cp_grad_contract_batched": (_I, [_I] * 5 + [_V] * 7),
            "pdp_gd_update_batched": (_I, [_I, _I, _V, _V, _I, _V, _V, _V, _D, _V, _V, _V, _V, _L, _V, _V]),
            "pdp_sysid_aux_integrate_batched": (_I, [_I] * 4 + [_V] * 5),
        }),
        ("model", {
            "pdp_model_get_info": (None, [_P(PdpModelInfo)]),
            "pdp_oc_rollout_batched": (_I, [_I, _I, _V, _V, _V, _I, _V, _V, _V]),
            "pdp_oc_rollout_feedback_batched": (_I, [_I, _I, _V, _V, _V, _V, _V, _V, _I, _V, _V, _V, _V]),
            "pdp_oc_ms_residuals_batched": (_I, [_I, _I, _V, _V, _V, _V, _I, _V, _V, _V, _V, _V]),
            "pdp_oc_costate_batched": (_I, [_I, _I, _V, _V, _V, _I, _V, _V]),
            "pdp_oc_auxsys_batched": (_I, [_I, _I, _V, _V, _V, _V, _I, _P(PdpOcAuxsys), _V]),
            "pdp_oc_solve_workspace_bytes": (_L, [_I, _I, _I]),
            "pdp_oc_solve_batched": (_I, [_I, _I, _V, _V, _I, _V, _V, _V, _V, _V, _V, _V, _P(PdpOcSolveOpts), _P(C.c_int), _V, _L, _V]),
            "pdp_oc_solve_ms_workspace_bytes": (_L, [_I, _I, _I]),
            "pdp_oc_solve_ms_batched": (_I, [_I, _I, _V, _V, _I, _V, _V, _V, _V, _V, _V, _V, _V, _V, _V, _P(PdpOcMsOpts), _V, _L, _V]),
            "pdp_oc_pdp_workspace_bytes": (_L, [_I, _I]),
            "pdp_oc_pdp_grad_batched": (_I, [_I, _I, _I, _V, _V, _V, _I, _V, _V, _V, _V, _V, _V, _V, _V, _V, _V, _L, _V]),
            "pdp_oc_riccati_doubles": (_L, []),
            "pdp_oc_predict_record_floats": (_L, []),
            "pdp_oc_pdp_grad_sens_batched": (_I, [_I, _I, _I, _V, _V, _V, _I, _V, _V, _V, _V, _V, _V, _P(PdpOcSensOut), _V, _V, _L, _V]),
            "pdp_oc_predict_batched": (_I, [_I, _I, _V, _I, _V, _V, _V, _V, _V, _V, _V]),
            "pdp_oc_predict_record_batched": (_I, [_I, _I, _V, _I, _V, _V, _V, _V, _V]),
            "pdp_cp_integrate_batched": (_I, [_I, _I, _P(PdpPolicy), _I, _V, _V, _I, _V, _V, _V, _V]),
            "pdp_cp_auxsys_batched": (_I, [_I, _I, _P(PdpPolicy), _I, _V, _V, _V, _I, _V, _V, _V, _V, _V, _V, _V, _V]),
            "pdp_cp_step_workspace_bytes": (_L, [_I, _I, _P(PdpPolicy), _I]),
            "pdp_cp_step_batched": (_I, [_I, _I, _P(PdpPolicy), _I, _V, _V, _I, _V, _V, _V, _V, _V, _L, _V]),
            "pdp_sysid_integrate_batched": (_I, [_I, _I, _V, _V, _V, _I, _V, _V]),
            "pdp_sysid_auxsys_batched": (_I, [_I, _I, _V, _V, _V, _I, _V, _V, _V]),
            "pdp_sysid_step_batched": (_I, [_I, _I, _V, _V, _V, _I, _V, _V, _V]),
            "pdp_sysid_step_workspace_bytes": (_L, [_I, _I]),
            "pdp_sysid_step_ws_batched": (_I, [_I, _I, _V, _V, _V, _I, _V, _V, _V, _L, _V]),
        })),
    "pdp_hip_lm.h": (("core", {"pdp_lm_update_batched": (_I, _LM_UPDATE + [_V])}),),
    "pdp_hip_lm_prior.h": (("core", {
        "pdp_lm_update_prior_batched": (_I, _LM_UPDATE + [_P(PdpLmPrior), _V]),
        "pdp_lm_covariance_batched": (_I, [_I, _I, _V, _I, _V, _V, _V, _V, _V, _V]),
    }),),
    "pdp_hip_oc_wls.h": (("model", {
        "pdp_oc_pdp_grad_wls_batched": (_I, [_I, _I, _I, _V, _V, _V, _I, _V, _V, _V, _L, _V, _L, _D, _V, _V, _V, _V, _V, _V, _L, _V])}),),
    "pdp_hip_sysid_gn.h": (("model", {"pdp_sysid_step_gn_batched": (_I, [_I, _I, _V, _V, _V, _V, _I, _I, _V, _V, _V, _L, _V])}),),
    "pdp_hip_sysid_ini.h": (("model", {"pdp_sysid_step_gn_ini_batched": (_I, [_I, _I, _V, _V, _V, _I, _V, _I, _I, _V, _V, _V, _L, _V])}),),
    "pdp_hip_sysid_jvp.h": (("model", {
        "pdp_sysid_rollout_jvp_batched": (_I, [_I, _I, _V, _V, _V, _I, _V, _I, _V, _V, _V, _V]),
        "pdp_sysid_rollout_jvp_rows": (_I, [_I]),
    }),),
    "pdp_hip_sysid_vjp.h": (("model", {"pdp_sysid_rollout_vjp_batched": (_I, [_I, _I, _V, _V, _V, _I, _V, _V, _V, _V])}),),
    "pdp_hip_sysid_vjp_u.h": (("model", {
        "pdp_sysid_rollout_vjp_u_batched": (_I, [_I, _I, _V, _V, _V, _I, _V, _V, _V, _V, _V]),
        "pdp_sysid_rollout_vjp_u_rows": (_I, [_I]),
    }),),
    "pdp_hip_sysid_wls.h": (("model", {
        "pdp_sysid_step_wls_batched": (_I, [_I, _I, _V, _V, _V, _I, _V, _L, _D, _V, _I, _I, _V, _V, _V, _L, _V])}),),
}


def entry_points(header=None, library=None):
    """{name: (restype, argtypes)} of the entry points that `header` declares ("pdp_hip_lm.h"; None: any) and `library` exports ("core" or "model"; None: either),
    in the headers' order"""
    return {name: sig for h, sections in ENTRY_POINTS.items() if header in (None, h)
            for lib, table in sections if library in (None, lib) for name, sig in table.items()}
