/* pdp_hip_lm.h - extension of the C-ABI of pdp_hip.h (section A, the core library libpdp_hip.so): the update of MANY independent Levenberg-Marquardt problems as
 * one launch.
 *
 * pdp_hip.h is pinned at its 33 entry points; what is added to the ABI afterwards lives in an extension header of its own that includes it.  libpdp_hip.so exports
 * the entry point below; error codes and the stream convention are those of pdp_hip.h. */
#ifndef PDP_HIP_LM_H
#define PDP_HIP_LM_H

#include "pdp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the state of a problem (pdp_lm_state.state) */
#define PDP_LM_START 0      /* nothing evaluated yet: the rows of the next launch are those of the initial point, which is accepted unconditionally */
#define PDP_LM_ACTIVE 1     /* a trial point is waiting for its rows */
#define PDP_LM_CONVERGED 2  /* !(loss > loss_tol) at the accepted point */
#define PDP_LM_STALLED 3    /* lam > lam_max: no damping the schedule may try improves the loss any more (the fp64 floor of the problem) */
#define PDP_LM_BUDGET 4     /* evaluations >= max_evals */
#define PDP_LM_FAILED 5     /* the initial point could not be evaluated */

/* the schedule of irl.LMLoop, passed to the kernel by value */
typedef struct {
    double up, down;          /* lam <- lam * up after a rejected trial, lam <- max(lam / down, lam_min) after an accepted one; both > 0 */
    double lam_min, lam_max;
    double loss_tol;
    int32_t max_evals;
} pdp_lm_schedule;

/* per-problem state at fixed device addresses, allocated (and, where said, initialised) by the caller; L = trace_len */
typedef struct {
    double* theta;            /* [K][p]            the accepted point (initialised: the initial point) */
    double* trial;            /* [K S][p]          the point to evaluate next, one row per sample (initialised: the initial point of the sample's problem) */
    double* lam;              /* [K]               the damping (initialised) */
    double* current;          /* [K][p + 1 + p p]  the mean row at theta */
    int32_t* state;           /* [K]               PDP_LM_* (initialised: PDP_LM_START) */
    int32_t* evaluations;     /* [K]               (initialised: 0) */
    int32_t* rejected;        /* [K]               (initialised: 0) */
    int32_t* accepted;        /* [K]               (initialised: 0) */
    int32_t* accepted_now;    /* [K S] or NULL     written by every launch: 1 where this launch accepted the trial of the sample's problem, else 0 */
    double* loss_trace;       /* [K][L] or NULL    the loss of accepted point number i of problem k at [k][i] */
    double* lambda_trace;     /* [K][L] or NULL    the damping after that acceptance */
    double* parameter_trace;  /* [K][L][p] or NULL that point */
    int64_t trace_len;        /* L: nothing is written at or beyond it */
    int64_t* counters;        /* [2]               launches done | problems still START or ACTIVE (initialised: 0 | K; a launch subtracts the problems it finished) */
} pdp_lm_state;

/* One Levenberg-Marquardt update of K independent problems (irl.LMLoop.step on the device).  rows [K S][rows_bstride >= p + 1 + p p] holds, per sample, grad [p] |
 * loss | G [p][p] (the layout of PDP_GRAD_GAUSS_NEWTON and of pdp_sysid_step_gn_batched) evaluated at state->trial; problem k owns the S consecutive samples k S ..
 * k S + S - 1.  bad [K S] (int32, or NULL): a sample flagged != 0 makes the trial of its problem unusable.  Per problem, in irl.LMLoop's order:
 *   - a problem that is neither START nor ACTIVE is left alone, except that its trial rows are rewritten to theta (its next evaluation stays finite) and its
 *     accepted_now entries are 0;
 *   - mean row = (sum of the S rows in ascending sample order) / S; unusable if a bad flag is set or an entry of the mean row is not finite; evaluations += 1;
 *   - START: usable -> accepted (lam stays, as in LMLoop.start), else FAILED.  ACTIVE: accepted iff usable and loss_trial < loss_current (an equal loss is rejected);
 *     accepted: theta <- trial, current <- mean row, lam <- max(lam / down, lam_min), traces at the problem's accepted count, accepted += 1;
 *     rejected: rejected += 1, lam <- lam * up;
 *   - termination, in this order: !(loss_current > loss_tol) CONVERGED; evaluations >= max_evals BUDGET; lam > lam_max STALLED;
 *   - else step = solve(G + lam D, g) with D_ii = G_ii (1 where G_ii == 0: irl.lm_step's rule) by Gaussian elimination with partial pivoting (largest magnitude of
 *     the remaining rows, ties to the lowest row), trial = theta - step, written to all S trial rows, state ACTIVE;
 *   - a trial that cannot be formed (a pivot not > 1e-300 in magnitude, or a non-finite entry of the trial) still counts, as in LMLoop.step: evaluations += 1,
 *     rejected += 1, lam <- lam * up, and back to the termination test - inside the same launch.
 * Unlike the host loop there is no least-squares fallback (an exactly singular damped matrix is a rejected trial), and the solve is pivoted elimination, not a
 * Cholesky factorisation: the damped G of partially identifiable systems is not numerically definite.
 * The result of a problem does not depend on K or on where the problem sits in the batch; no floating-point atomics.  Made for many problems with few samples each
 * (a lane sums its own row over the S samples): one problem with thousands of samples stays irl.LMLoop's job.
 * K, S, p <= 0, a null rows / schedule / state or a null required pointer inside state, rows_bstride < p + 1 + p p, up <= 0 or down <= 0 (or NaN): PDP_E_ARG;
 * p > 16: PDP_E_SIZE; both before any launch. */
int pdp_lm_update_batched(int K, int S, int p, const double* rows, int rows_bstride, const int32_t* bad, const pdp_lm_schedule* schedule, const pdp_lm_state* state,
                          void* stream);

#ifdef __cplusplus
}
#endif

#endif /* PDP_HIP_LM_H */
