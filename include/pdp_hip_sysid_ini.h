/* pdp_hip_sysid_ini.h - extension of the C-ABI of pdp_hip.h (section B, PDP_KIND_SYSID): SysID.step as a nonlinear least-squares evaluation in the parameters AND
 * the unobserved components of the initial state.
 *
 * pdp_hip.h is pinned at its 33 entry points; what is added to the ABI afterwards lives in an extension header of its own that includes it.  Every model
 * library (libpdp_model_<name>.so) exports the entry point below; error codes, flags, stream and workspace conventions are those of pdp_hip.h. */
#ifndef PDP_HIP_SYSID_INI_H
#define PDP_HIP_SYSID_INI_H

#include "pdp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The evaluation of pdp_hip_sysid_gn.h with q = popcount(ini_mask) components of the initial state as further unknowns.  ini_mask is a bit mask over the n state
 * components; its k-th set bit in ascending order, i_k, is unknown number p + k.  The evaluation point is (theta, x0): the estimated components of x0 are simply the
 * values found in x0 [B][n] (NULL: x_obs[:, 0], as in pdp_sysid_step_batched).  W = p + q.  Per trajectory
 *     X_0 [n][W] = zeros with X_0[i_k][p + k] = 1,      X_{t+1} = F_t X_t + [E_t | 0]
 *     loss  as in pdp_sysid_step_gn_batched, row 0's |x0 - x_obs_0|^2 over its observed entries included
 *     grad [W] = sum_{t<=T} d_t^T X_t,      G [W][W] = sum_{t<=T} X_t^T X_t      (d_t = x_t - x_obs_t)
 * with the masks of PDP_GRAD_SKIP_MISSING applied exactly as there (a NaN in x_obs is an entry that was NOT OBSERVED: its residual is dropped from the loss, its term
 * from grad and its Jacobian row from G - selects, never products with 0; the recursion of X_t itself is not masked; an OBSERVED entry whose own state is not finite
 * leaves a NaN in the loss).  Row 0 is no longer silent: an observed x_obs[0][i_k] adds d_0[i_k] to grad[p + k] and 1 to G[p + k][p + k].
 * packed [B][W + 1 + W W] is ONE ROW per trajectory, grad [W] | loss | G [W][W] row-major; G is symmetric to the bit (both operands of every product are the same
 * tile) and not symmetrised; loss [B] is written as well.  A trajectory with nothing observed returns exact zeros in all W + 1 + W W entries.  With
 * PDP_GRAD_SKIP_MISSING the caller gives an x0 without NaN (or a fully observed x_obs[:, 0]): an estimated component still needs a finite value to be evaluated at.
 * theta, theta_bstride, flags (0 or PDP_GRAD_SKIP_MISSING), workspace (pdp_sysid_step_workspace_bytes(B, T) bytes, or NULL): as in pdp_sysid_step_gn_batched.
 * ini_mask == 0: the call IS pdp_sysid_step_gn_batched's - the same kernels, the same row of p + 1 + p p doubles.
 * A mask bit >= n, unknown flag bits, null pointers (other than x0 and workspace), non-positive sizes: PDP_E_ARG before any launch; not a SysID model: PDP_E_MODE;
 * n > 16 or p + q > 16: PDP_E_SIZE (the caller contracts materialised sensitivities instead, as runtime.ModelLib.sysid_step does). */
int pdp_sysid_step_gn_ini_batched(int B, int T, const double* u, const double* x_obs, const double* x0, int ini_mask, const double* theta, int theta_bstride,
                                  int flags, double* loss, double* packed, void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* PDP_HIP_SYSID_INI_H */
