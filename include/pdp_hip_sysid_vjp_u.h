/* pdp_hip_sysid_vjp_u.h - extension of the C-ABI of pdp_hip.h (section B, PDP_KIND_SYSID): the SysID rollout's vector-Jacobian product of pdp_hip_sysid_vjp.h with
 * the one argument that header leaves out - the gradient of ANY scalar loss of a rollout with respect to the inputs, from the same adjoint (costate) sweep.
 *
 * pdp_hip.h is pinned at its 33 entry points; what is added to the ABI afterwards lives in an extension header of its own that includes it.  Every model
 * library (libpdp_model_<name>.so) exports the entry points below; error codes, stream and theta conventions are those of pdp_hip.h. */
#ifndef PDP_HIP_SYSID_VJP_U_H
#define PDP_HIP_SYSID_VJP_U_H

#include "pdp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* x, u, theta, theta_bstride, grad_x, grad_theta and grad_x0 are those of pdp_sysid_rollout_vjp_batched (pdp_hip_sysid_vjp.h): x [B][T+1][n] the rollout
 * x_{t+1} = f(x_t, u_t, theta) for u [B][T][m], grad_x [B][T+1][n] the cotangents g_t = dL/dx_t of a scalar L(x_0 .. x_T).  Per trajectory
 *     lam_T = g_T ;    t = T-1 .. 0 :   grad_u[t] = G_t^T lam_{t+1} ,   grad_theta += E_t^T lam_{t+1} ,   lam_t = g_t + F_t^T lam_{t+1} ;    grad_x0 = lam_0
 * with F_t = df/dx, G_t = df/du, E_t = df/dtheta at (x_t, u_t, theta): grad_u [B][T][m] = dL/du through the dynamics.  A loss that also uses u directly adds that
 * term itself.  Every grad_u[b][t] is written exactly once and never read: the buffer need not be initialised.  One launch, no workspace.
 * Any of the three outputs may be NULL, not all of them.  With grad_u == NULL this is pdp_sysid_rollout_vjp_batched: the same kernel, the same bits.  With grad_u,
 * grad_theta and grad_x0 are the same sums of the same products in the same order.
 * Causality: lam_{t+1} collects the cotangents of the steps behind t alone.  With finite Jacobians a zero cotangent gives grad_u of exact zeros, and a cotangent that is
 * non-zero at step s only gives grad_u[t] = 0 exactly for every t >= s.  A NaN in grad_x[b][s] shows in grad_u[b][t] for t < s and leaves grad_u[b][t >= s] as it
 * was; a NaN in a trajectory's x, u, theta or grad_x shows in that trajectory's outputs and in no other's.  There is no masking and no status word.  A trajectory's
 * output bits do not depend on the batch size, on its position in the batch, or on the pool rows below.
 * Left out: second order; d/du of the least-squares rows of pdp_sysid_step_*; models without parameters.
 * NULL x, u, theta or grad_x, all three outputs NULL, B <= 0, T <= 0, a theta_bstride that is neither 0 nor >= p: PDP_E_ARG before any launch; not a SysID model:
 * PDP_E_MODE; n > 64, p + m > 512 with grad_u (a lane owns one state component and at most eight columns of [E | G]), p > 512 without it, or a pool of more than
 * 150 KB: PDP_E_SIZE. */
int pdp_sysid_rollout_vjp_u_batched(int B, int T, const double* x, const double* u, const double* theta, int theta_bstride, const double* grad_x,
                                    double* grad_theta, double* grad_x0, double* grad_u, void* stream);

/* pool rows (time steps per lane-parallel Jacobian pass) that the launch above uses with grad_u for a batch of B on this device (256 compute units assumed without
 * one): the generated chunk up to four trajectories per compute unit, beyond that what fits 2400 doubles of pool, but at least four rows.  The horizon is cut into
 * ceil(T / rows) chunks of equal length.  <= 0: the error code the launch would return (B <= 0: PDP_E_ARG). */
int pdp_sysid_rollout_vjp_u_rows(int B);

#ifdef __cplusplus
}
#endif

#endif /* PDP_HIP_SYSID_VJP_U_H */
