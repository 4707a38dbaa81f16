/* pdp_hip_oc_wls.h - extension of the C-ABI of pdp_hip.h (section B, PDP_KIND_OC): the fused OC / IRL gradient unit as a WEIGHTED and HUBER-ROBUST
 * nonlinear least-squares evaluation.
 *
 * pdp_hip.h is pinned at its 33 entry points; what is added to the ABI afterwards lives in an extension header of its own that includes it.  Every model
 * library (libpdp_model_<name>.so) exports the entry point below; error codes, flags, stream and workspace conventions are those of pdp_hip.h. */
#ifndef PDP_HIP_OC_WLS_H
#define PDP_HIP_OC_WLS_H

#include "pdp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The evaluation of pdp_oc_pdp_grad_batched under PDP_GRAD_GAUSS_NEWTON with a weight per demonstration entry - states AND controls - and, optionally, Huber's
 * loss on the standardised residual: the semantics of pdp_sysid_step_wls_batched (pdp_hip_sysid_wls.h), carried to states and controls.
 * weights_x [B][T+1][n] with weights_x_bstride = (T+1) n, or ONE block [T+1][n] shared by the batch with weights_x_bstride = 0; weights_u [B][T][m] with
 * weights_u_bstride = T m, or ONE block [T][m] with weights_u_bstride = 0.  Either pointer may be NULL: all ones (w = 1 / sigma^2 is the usual choice).
 * huber_delta: +inf for plain (weighted) least squares, or a threshold > 0.
 * OBSERVED: an entry is observed iff w > 0 and, under PDP_GRAD_SKIP_MISSING, its demonstration entry is not NaN.  Anything else - w = 0 included - is NOT
 * OBSERVED and follows PDP_GRAD_GAUSS_NEWTON | PDP_GRAD_SKIP_MISSING exactly: it is selected away, never multiplied by 0; the demonstration may hold anything
 * there, NaN included; it adds nothing to the loss, grad or G.  A trajectory with nothing observed returns exact zeros in all p + 1 + p p entries.  Without the
 * flag a NaN demonstration entry at w > 0 shows in the loss, as it always did.
 * Per observed entry, with d the residual (x_t - demo_x_t or u_t - demo_u_t):
 *     e = sqrt(w) d,      psi = 1 if |e| <= delta, else delta / |e|,      rho(e) = e^2 if |e| <= delta, else 2 delta |e| - delta^2,      s = sqrt(w psi)
 * and with the sums over the observed entries, X_t = dx_t/dtheta and U_t = du_t/dtheta the sensitivities of the OC solution (d^x, d^u: the residuals of the two sides):
 *     loss     = sum rho(e)
 *     grad [p] = sum_{t<=T} (s . d^x_t)^T (s . X_t) + sum_{t<T} (s . d^u_t)^T (s . U_t)      exactly half the derivative of the loss - the scaling of every other mode
 *     G [p][p] = sum_{t<=T} (s . X_t)^T (s . X_t) + sum_{t<T} (s . U_t)^T (s . U_t)          the Gauss-Newton matrix of iteratively reweighted least squares
 * (s . : the rows scaled entry by entry).  The Riccati recursion and the forward sweep themselves are never scaled.  Row 0 of the states adds rho to the loss
 * and - X_0 = 0 - nothing else.
 * packed [B][p + 1 + p p] is ONE ROW per trajectory, grad [p] | loss | G [p][p] row-major: the row of PDP_GRAD_GAUSS_NEWTON.  G is symmetric to the bit (both
 * operands of every product are the same scaled tile) and not symmetrised; loss [B] is written as well.
 * x0, u, theta, theta_bstride, demo_x, demo_u, x, lam, status, PDP_OC_GIVEN_TRAJ and the workspace (pdp_oc_pdp_workspace_bytes(B, T) bytes): as in
 * pdp_oc_pdp_grad_batched.
 * weights_x = weights_u = NULL and huber_delta = +inf: the results of PDP_GRAD_GAUSS_NEWTON (with or without PDP_GRAD_SKIP_MISSING) within rounding (other kernels).
 * PDP_E_ARG before any launch: flags other than a subset of PDP_OC_GIVEN_TRAJ | PDP_GRAD_SKIP_MISSING; huber_delta <= 0 or NaN; a weight stride other than the two
 * values above for its array; null pointers other than x0 (with a given trajectory) and the two weights; non-positive sizes; a workspace that is too small.
 * Not an OC model: PDP_E_MODE.  Outside the fused limits: PDP_E_SIZE where pdp_oc_pdp_grad_batched returns it (the limits on n, m and p before the argument checks,
 * a horizon beyond LDS behind them; this mode's pool rows are n + m words longer) - the caller contracts materialised sensitivities instead, as
 * runtime.ModelLib.oc_pdp_grad does. */
int pdp_oc_pdp_grad_wls_batched(int B, int T, int flags, const double* x0, const double* u, const double* theta, int theta_bstride,
                                const double* demo_x, const double* demo_u,
                                const double* weights_x, int64_t weights_x_bstride, const double* weights_u, int64_t weights_u_bstride, double huber_delta,
                                double* x, double* lam, double* loss, double* packed, int32_t* status,
                                void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* PDP_HIP_OC_WLS_H */
