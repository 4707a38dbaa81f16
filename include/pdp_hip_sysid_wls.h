/* pdp_hip_sysid_wls.h - extension of the C-ABI of pdp_hip.h (section B, PDP_KIND_SYSID): SysID.step as a WEIGHTED and HUBER-ROBUST nonlinear least-squares evaluation.
 *
 * pdp_hip.h is pinned at its 33 entry points; what is added to the ABI afterwards lives in an extension header of its own that includes it.  Every model
 * library (libpdp_model_<name>.so) exports the entry point below; error codes, flags, stream and workspace conventions are those of pdp_hip.h. */
#ifndef PDP_HIP_SYSID_WLS_H
#define PDP_HIP_SYSID_WLS_H

#include "pdp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The evaluation of pdp_hip_sysid_ini.h with a weight per recorded entry and, optionally, Huber's loss on the standardised residual.
 * weights [B][T+1][n] with weights_bstride = (T+1) n, or ONE block [T+1][n] shared by the batch with weights_bstride = 0; NULL: all ones (w = 1 / sigma^2 is the
 * usual choice).  huber_delta: +inf for plain (weighted) least squares, or a threshold > 0.
 * OBSERVED: an entry is observed iff w > 0 and, under PDP_GRAD_SKIP_MISSING, x_obs is not NaN.  Anything else - w = 0 included - is NOT OBSERVED and follows
 * PDP_SYSID_GN_MISS exactly: it is selected away, never multiplied by 0; x_obs may hold anything there, NaN included; it adds nothing to the loss, grad or G.  A
 * trajectory with nothing observed returns exact zeros in all W + 1 + W W entries.  Without the flag a NaN x_obs at w > 0 shows in the loss, as it always did.
 * Per observed entry, with d = x_t - x_obs_t:
 *     e = sqrt(w) d,      psi = 1 if |e| <= delta, else delta / |e|,      rho(e) = e^2 if |e| <= delta, else 2 delta |e| - delta^2,      s = sqrt(w psi)
 * and with the sums over the observed entries, X_t the sensitivity of pdp_sysid_step_gn_ini_batched (W = p + popcount(ini_mask) columns):
 *     loss     = sum rho(e)
 *     grad [W] = sum_{t<=T} (s . d_t)^T (s . X_t)        exactly half the derivative of the loss - the scaling of the other modes
 *     G [W][W] = sum_{t<=T} (s . X_t)^T (s . X_t)        the Gauss-Newton matrix of iteratively reweighted least squares
 * (s . : the rows scaled entry by entry).  The recursion X_{t+1} = F_t X_t + [E_t | 0] itself is never scaled.  An observed entry whose own state is not finite leaves a
 * non-finite loss.  x0 [B][n] (NULL: x_obs[:, 0]), ini_mask and row 0 behave as in pdp_sysid_step_gn_ini_batched; ini_mask = 0 gives the row of p + 1 + p p doubles.
 * packed [B][W + 1 + W W] is ONE ROW per trajectory, grad [W] | loss | G [W][W] row-major; G is symmetric to the bit (both operands of every product are the same
 * scaled tile) and not symmetrised; loss [B] is written as well.
 * theta, theta_bstride, flags (0 or PDP_GRAD_SKIP_MISSING), workspace (pdp_sysid_step_workspace_bytes(B, T) bytes, or NULL): as in pdp_sysid_step_gn_batched.
 * weights = NULL and huber_delta = +inf: the results of pdp_sysid_step_gn_ini_batched within rounding (other kernels).
 * huber_delta <= 0 or NaN, a weights_bstride other than the two values above, a mask bit >= n, unknown flag bits, null pointers (other than x0, weights and
 * workspace), non-positive sizes: PDP_E_ARG before any launch; not a SysID model: PDP_E_MODE; n > 16 or W > 16: PDP_E_SIZE (the caller contracts materialised
 * sensitivities instead, as runtime.ModelLib.sysid_step does). */
int pdp_sysid_step_wls_batched(int B, int T, const double* u, const double* x_obs, const double* x0, int ini_mask, const double* weights, int64_t weights_bstride,
                               double huber_delta, const double* theta, int theta_bstride, int flags, double* loss, double* packed, void* workspace,
                               int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* PDP_HIP_SYSID_WLS_H */
