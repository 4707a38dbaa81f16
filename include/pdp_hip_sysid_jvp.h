/* pdp_hip_sysid_jvp.h - extension of the C-ABI of pdp_hip.h (section B, PDP_KIND_SYSID): the SysID rollout as a Jacobian-vector product - the tangent of a rollout
 * along a direction in (theta, x_0, u), by the forward (tangent) sweep.  The other half of pdp_hip_sysid_vjp.h / pdp_hip_sysid_vjp_u.h: with J v beside J' g a
 * Gauss-Newton product J' J v of any residual of the rollout is two launches whatever p is, and forward-mode differentiation works through the rollout.
 *
 * pdp_hip.h is pinned at its 33 entry points; what is added to the ABI afterwards lives in an extension header of its own that includes it.  Every model
 * library (libpdp_model_<name>.so) exports the entry points below; error codes, stream and theta conventions are those of pdp_hip.h. */
#ifndef PDP_HIP_SYSID_JVP_H
#define PDP_HIP_SYSID_JVP_H

#include "pdp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* x, u, theta and theta_bstride are those of pdp_sysid_rollout_vjp_batched (pdp_hip_sysid_vjp.h): x [B][T+1][n] the rollout x_{t+1} = f(x_t, u_t, theta) for
 * u [B][T][m] (what pdp_sysid_integrate_batched wrote: there is no rollout here).  The direction: d_theta [1 or B][p] (d_theta_bstride 0: one row shared by the batch,
 * >= p: one per trajectory), d_x0 [B][n], d_u [B][T][m].  Per trajectory
 *     d_x[0] = d_x0 ;    t = 0 .. T-1 :   d_x[t+1] = F_t d_x[t] + E_t d_theta + G_t d_u[t]
 * with F_t = df/dx, G_t = df/du, E_t = df/dtheta at (x_t, u_t, theta): d_x [B][T+1][n] = the directional derivative of the rollout.  Every d_x[b][t] is written
 * exactly once and never read: the buffer need not be initialised.  One launch, no workspace.
 * Any of the three tangents may be NULL, which means zero (d_x[b][0] is then +0.0); not all of them.  A NULL tangent and a buffer of zeros give the same bits as long
 * as d_u is NULL in both calls or in neither: with d_u another instantiation of the kernel runs (it evaluates G_t), and d_u == NULL against a d_u of zeros agrees to
 * rounding only.
 * Causality: d_x[t] collects the tangents of the steps before t alone.  With finite Jacobians zero tangents give exact zeros, and a d_u that is non-zero at step s only
 * gives d_x[t] = 0 exactly for every t <= s.  A NaN in a trajectory's x, u, theta or tangents shows in that trajectory's d_x and in no other's.  There is no masking
 * and no status word.  A trajectory's output bits do not depend on the batch size, on its position in the batch, or on the pool rows below.
 * Left out: second order; models without parameters.
 * NULL x, u, theta or d_x, all three tangents NULL, B <= 0, T <= 0, a theta_bstride or d_theta_bstride that is neither 0 nor >= p: PDP_E_ARG before any launch; not a
 * SysID model: PDP_E_MODE; n > 64, p > 512, p + m > 512 with d_u (the limits of the vjp pair: both directions always exist together), or a pool of more than
 * 150 KB: PDP_E_SIZE. */
int pdp_sysid_rollout_jvp_batched(int B, int T, const double* x, const double* u, const double* theta, int theta_bstride, const double* d_theta,
                                  int d_theta_bstride, const double* d_x0, const double* d_u, double* d_x, void* stream);

/* pool rows (time steps per lane-parallel Jacobian pass) that the launch above uses for a batch of B on this device (256 compute units assumed without one), with or
 * without d_u: the rule of pdp_sysid_rollout_vjp_batched on the same row - the generated chunk up to four trajectories per compute unit, beyond that what fits 2400
 * doubles of pool, but at least four rows.  The horizon is cut into ceil(T / rows) chunks of equal length.  <= 0: the error code the launch would return without d_u
 * (B <= 0: PDP_E_ARG). */
int pdp_sysid_rollout_jvp_rows(int B);

#ifdef __cplusplus
}
#endif

#endif /* PDP_HIP_SYSID_JVP_H */
