/* pdp_hip_sysid_vjp.h - extension of the C-ABI of pdp_hip.h (section B, PDP_KIND_SYSID): the SysID rollout as a vector-Jacobian product - the gradient of ANY scalar
 * loss of a rollout with respect to the parameters and the initial state, by the adjoint (costate) sweep.
 *
 * pdp_hip.h is pinned at its 33 entry points; what is added to the ABI afterwards lives in an extension header of its own that includes it.  Every model
 * library (libpdp_model_<name>.so) exports the entry point below; error codes, stream and theta conventions are those of pdp_hip.h. */
#ifndef PDP_HIP_SYSID_VJP_H
#define PDP_HIP_SYSID_VJP_H

#include "pdp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* x [B][T+1][n] is the rollout x_{t+1} = f(x_t, u_t, theta) that pdp_sysid_integrate_batched wrote for u [B][T][m] and theta (the kernel does no rollout of its own:
 * the Jacobians are evaluated at the x it is given), grad_x [B][T+1][n] the cotangents g_t = dL/dx_t of a scalar L(x_0 .. x_T).  Per trajectory
 *     lam_T = g_T ;    t = T-1 .. 0 :   grad_theta += E_t^T lam_{t+1} ,   lam_t = g_t + F_t^T lam_{t+1} ;    grad_x0 = lam_0
 * with F_t = df/dx, E_t = df/dtheta at (x_t, u_t, theta): grad_theta [B][p] = dL/dtheta through this trajectory (a shared theta's gradient is the caller's sum over
 * the batch), grad_x0 [B][n] = dL/dx_0, grad_x[:, 0] included.  Either output may be NULL, not both.  O(T (n^2 + n p)) per trajectory, one launch, no workspace;
 * pdp_sysid_step_batched's gradient is the special case g = x - x_obs.
 * theta_bstride: 0 (one theta [p] shared by the batch) or >= p (theta [B][theta_bstride]), as elsewhere.
 * There is no masking and no status word: a NaN in a trajectory's x, u, theta or grad_x shows in that trajectory's outputs and in no other's.  With finite Jacobians a
 * zero cotangent gives exact zeros, and a cotangent that is non-zero at t = 0 only gives grad_theta = 0 and grad_x0 = g_0 to the bit.  A trajectory's output bits do
 * not depend on the batch size or on its position in the batch.
 * Left out: second order; the gradient with respect to u is pdp_sysid_rollout_vjp_u_batched's (pdp_hip_sysid_vjp_u.h).
 * NULL x, u, theta or grad_x, both outputs NULL, B <= 0, T <= 0, a theta_bstride that is neither 0 nor >= p: PDP_E_ARG before any launch; not a SysID model:
 * PDP_E_MODE; n > 64 or p > 512 (a lane owns one state component and at most eight parameters): PDP_E_SIZE. */
int pdp_sysid_rollout_vjp_batched(int B, int T, const double* x, const double* u, const double* theta, int theta_bstride, const double* grad_x, double* grad_theta,
                                  double* grad_x0, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* PDP_HIP_SYSID_VJP_H */
