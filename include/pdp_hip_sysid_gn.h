/* pdp_hip_sysid_gn.h - extension of the C-ABI of pdp_hip.h (section B, PDP_KIND_SYSID): SysID.step as a nonlinear least-squares evaluation.
 *
 * pdp_hip.h is pinned at its 33 entry points; what is added to the ABI afterwards lives in an extension header of its own that includes it.  Every model
 * library (libpdp_model_<name>.so) exports the entry point below; error codes, flags, stream and workspace conventions are those of pdp_hip.h. */
#ifndef PDP_HIP_SYSID_GN_H
#define PDP_HIP_SYSID_GN_H

#include "pdp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* SysID.step as a nonlinear least-squares evaluation: beside loss and grad the Gauss-Newton matrix G = sum_{t<=T} X_t^T X_t (X_t = dx_t/dtheta, X_0 = 0) from the
 * sensitivity tiles the kernels hold anyway.  packed [B][p + 1 + p p] is ONE ROW per trajectory, grad [p] | loss | G [p][p] row-major (the layout of
 * PDP_GRAD_GAUSS_NEWTON; G symmetric to the bit); loss [B] is written as well.  x0 [B][n] is the initial state of the rollouts (NULL: x_obs[:, 0], as in
 * pdp_sysid_step_batched); row 0 then adds |x0 - x_obs_0|^2 to the loss and nothing to grad and G.  flags: 0 or PDP_GRAD_SKIP_MISSING - a NaN in x_obs is an entry
 * that was NOT OBSERVED: its residual is dropped from the loss, its term from grad and its Jacobian row from G (selects, never products with 0; the recursion of X_t
 * itself is not masked); a trajectory with nothing observed returns exact zeros; an OBSERVED entry whose own state is not finite leaves a NaN in the loss (a diverged
 * rollout stays visible - there is no status word).  With PDP_GRAD_SKIP_MISSING the caller gives an x0 without NaN (or a fully observed x_obs[:, 0]).
 * workspace: pdp_sysid_step_workspace_bytes(B, T) bytes, as for pdp_sysid_step_ws_batched (NULL: the kernels roll out themselves, whatever the batch).
 * Null pointers (other than x0 and workspace), non-positive sizes and unknown flag bits: PDP_E_ARG before any launch; not a SysID model: PDP_E_MODE; n > 16 or
 * p > 16: PDP_E_SIZE (the caller contracts materialised sensitivities instead, as runtime.ModelLib.sysid_step does). */
int pdp_sysid_step_gn_batched(int B, int T, const double* u, const double* x_obs, const double* x0, const double* theta, int theta_bstride,
                              int flags, double* loss, double* packed, void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* PDP_HIP_SYSID_GN_H */
