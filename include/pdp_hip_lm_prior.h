/* pdp_hip_lm_prior.h - extension of the C-ABI of pdp_hip_lm.h (section A, the core library libpdp_hip.so): the batched Levenberg-Marquardt update with a Gaussian prior
 * on the unknowns, and the covariance of the estimates.
 *
 * pdp_hip_lm.h stays as it is; libpdp_hip.so exports the two entry points below; error codes and the stream convention are those of pdp_hip.h. */
#ifndef PDP_HIP_LM_PRIOR_H
#define PDP_HIP_LM_PRIOR_H

#include "pdp_hip_lm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* a Gaussian prior (x - mean)' precision (x - mean) on the unknowns of every problem, in the scale of the MEAN row (a caller that minimises a sum over S samples
 * divided by S hands in its precision divided by S) */
typedef struct {
    const double* mean;        /* [K][p], or [p] with mean_kstride == 0 */
    const double* precision;   /* kind 0: the diagonal [K][p]; kind 1: full row-major [K][p][p]; shared by all problems with precision_kstride == 0 */
    int32_t kind;
    int64_t mean_kstride, precision_kstride;   /* in doubles; 0 = shared */
    double* prior_loss;        /* [K] or NULL: the prior's share of the loss at the accepted point, written on acceptance */
} pdp_lm_prior;

/* pdp_lm_update_batched with one insertion per live problem directly after its mean row is formed; x = trial[k S][.] is the point the rows were evaluated at:
 *   d_c = x_c - mean_c;  (P d)_r = sum_c P_rc d_c, summed from 0.0 in ascending c (kind 0: the single product P_rr d_r);  q = sum_r d_r (P d)_r, from 0.0 in ascending r;
 *   g_r += (P d)_r;  loss += q;  G_rc += P_rc (kind 0: the diagonal only);  the "unusable" test then covers the augmented values as well.
 * Everything downstream sees the augmented row: acceptance, current, the traces, CONVERGED against loss_tol, the damped solve; a rejected trial restores the augmented
 * row from current.  prior_loss[k] = q is written where the launch accepts the trial of problem k.  The result of a problem does not depend on K or on where it sits in
 * the batch; no floating-point atomics.
 * prior == NULL: exactly pdp_lm_update_batched.  Errors: those of pdp_lm_update_batched, in its order; a null mean or precision, a kind other than 0 / 1 or a negative
 * stride: PDP_E_ARG (with the null pointers, before the size). */
int pdp_lm_update_prior_batched(int K, int S, int p, const double* rows, int rows_bstride, const int32_t* bad, const pdp_lm_schedule* schedule, const pdp_lm_state* state,
                                const pdp_lm_prior* prior, void* stream);

/* The covariance of K estimates from their rows grad [p] | loss | G [p][p] (rows_bstride >= p + 1 + p p: the layout of pdp_lm_state.current).  Per problem A = G of
 * the row; [A | I] is reduced by the update's own elimination (partial pivoting, largest magnitude of the remaining rows, ties to the lowest row; a pivot must be
 * > 1e-300 in magnitude) and back-substituted per column; cov = scale[k] A^-1 (scale NULL: 1) as computed, not symmetrised; std_err_r = sqrt(cov_rr), NaN where that
 * is negative; pivot_ratio = smallest / largest pivot magnitude.  status 0: success; 1: a pivot failed the threshold or an entry of A or of the result is not finite -
 * then cov and std_err of that problem are NaN and its pivot_ratio is 0; the other problems are unaffected.
 * K, p <= 0, a null rows / cov / status, rows_bstride < p + 1 + p p: PDP_E_ARG; p > 16: PDP_E_SIZE (before the stride); both before any launch. */
int pdp_lm_covariance_batched(int K, int p, const double* rows, int rows_bstride, const double* scale, double* cov, double* std_err, double* pivot_ratio, int32_t* status,
                              void* stream);

#ifdef __cplusplus
}
#endif

#endif /* PDP_HIP_LM_PRIOR_H */
