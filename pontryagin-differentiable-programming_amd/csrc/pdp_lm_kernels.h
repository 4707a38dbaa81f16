// pdp_lm_kernels.h - the update of K independent Levenberg-Marquardt problems as one launch (pdp_lm_update_batched, include/pdp_hip_lm.h): what irl.LMLoop.step does
// on the host - reduce the rows of the evaluation, accept or reject the trial point, move the damping, the damped solve, the next trial point, termination, traces -
// for all problems at once.  Semantics: the comment of the entry point; this header is the mapping.
//
// A problem is a 16-lane row of a wavefront, four problems per wavefront (= one 64-thread workgroup).  Lane r of a row holds row r of the augmented matrix
// [G + lam D | g] - p <= 16 doubles and the right-hand side - in registers: every index into it is a literal after unrolling (the 16 column steps test col < p, which
// is uniform; inside a step the columns >= p run through on zeros).  Lanes >= p of a row and the rows of problems >= K in the last wavefront neither load nor store; they run through the same
// instructions on values nothing reads.  Pivot search (a butterfly over the row), the broadcast of the pivot row and the row swap are width-16 shuffles (ds_bpermute:
// no LDS is allocated).  The row reduction is each lane summing its own row over the S samples in ascending order, the mean one division: no atomics on doubles, and
// no arithmetic that depends on K or on the quarter of the wavefront a problem sits in.  The only atomic is the integer subtraction of the finished problems from
// counters[1], one per wavefront that finished any.
//
// The loop "a trial that cannot be formed is a rejected trial; try the next damping" runs inside the launch and is uniform over the wavefront: while any of the four
// problems still needs a trial point, all 64 lanes run the solve (full exec mask for the shuffles) and the problems that do not need it ignore its result.  It is
// bounded by max_evals (every turn is an evaluation) and in practice by lam > lam_max.
//
// Floating-point contraction is off in the kernel: products and sums round separately, in the order written, so that the decisions (pivot choice, "pivot > 1e-300",
// strictly lower loss) are those of the same statements in numpy (tests/lm_batched_common.py).
//
// A Gaussian prior on the unknowns (pdp_lm_update_prior_batched, include/pdp_hip_lm_prior.h) is a compile-time variant of the same body: lane r loads row r of the
// precision (or its diagonal entry) and its entry of the mean, the differences d_c travel by width-16 shuffles, and the prior's share is added to the mean row before the
// vote on "unusable" - before the retry loop, so that nothing new is live across it.  The variant without a prior is pdp_lm_update_batched's kernel, instruction for
// instruction what it was before the variant existed.  lm_covariance_kernel (pdp_lm_covariance_batched) is the same mapping with [A | I] - 32 doubles - per lane.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/pdp_hip_lm_prior.h"

namespace pdp {

constexpr int LM_PMAX = 16;              // lanes of a problem's row
constexpr double LM_PIVOT_MIN = 1e-300;  // a pivot must be larger in magnitude

__device__ __forceinline__ bool lm_finite(double x) { return __builtin_fabs(x) <= 1.7976931348623157e308; }    // (false for NaN)
// values the optimiser cannot see through (a lane index, a launch constant): what is derived from them inside a loop is formed there, not hoisted out of it
__device__ __forceinline__ int lm_opaque(int v) { asm volatile("" : "+v"(v)); return v; }
__device__ __forceinline__ int lm_sopaque(int v) { asm volatile("" : "+s"(v)); return v; }
template <class T> __device__ __forceinline__ T* lm_opaque(T* q) { asm volatile("" : "+v"(q)); return q; }
// true in every lane of a 16-lane row iff `flag` is set in any of its lanes (all 64 lanes call)
__device__ __forceinline__ bool lm_row_any(bool flag, int quarter) { return ((__ballot(flag) >> (16 * quarter)) & 0xffffull) != 0; }

// the one element of the kernel's argument pack, where it has one
__device__ __forceinline__ const pdp_lm_prior& lm_only(const pdp_lm_prior& prior) { return prior; }

// Prior...: nothing - the kernel of pdp_lm_update_batched, with the kernel arguments it always had - or one pdp_lm_prior behind them
template <class... Prior>
__global__ void __launch_bounds__(64) lm_update_kernel(int K, int S, int p, const double* __restrict__ rows, int rs, const int32_t* __restrict__ bad,
                                                       pdp_lm_schedule sch, pdp_lm_state st, Prior... prior_arg) {
#pragma clang fp contract(off)
    constexpr bool PRIOR = sizeof...(Prior) != 0;
    const int lane = threadIdx.x, r = lane & 15, quarter = lane >> 4;
    const int64_t k = (int64_t)blockIdx.x * 4 + quarter;
    const bool valid = k < K, mine = valid && r < p;
    const int w = p + 1 + p * p;
    const int64_t L = st.trace_len;
    if (blockIdx.x == 0 && lane == 0) st.counters[0] += 1;

    int state = mine ? st.state[k] : PDP_LM_CONVERGED;
    const bool live = mine && (state == PDP_LM_START || state == PDP_LM_ACTIVE);
    int evals = 0, rej = 0, acc = 0;
    double lam = 0.0, theta = 0.0, loss_cur = 0.0, g = 0.0, G[LM_PMAX];
#pragma unroll
    for (int c = 0; c < LM_PMAX; ++c) G[c] = 0.0;
    bool accept = false, need = false;

    if (live) {
        evals = st.evaluations[k]; rej = st.rejected[k]; acc = st.accepted[k]; lam = st.lam[k];
        // the mean row: this lane's entry of grad, the loss, this lane's row of G
        double loss = 0.0;
        bool unusable = false;
        for (int s = 0; s < S; ++s) {
            const double* row = rows + (k * S + s) * (int64_t)rs;
            g += row[r];
            loss += row[p];
#pragma unroll
            for (int c = 0, pc = lm_sopaque(p); c < LM_PMAX; ++c) if (c < pc) G[c] += row[p + 1 + r * p + c];
            if (bad) unusable |= bad[k * S + s] != 0;
        }
        const double count = (double)S;
        g /= count; loss /= count;
        unusable |= !lm_finite(g) || !lm_finite(loss);
#pragma unroll
        for (int c = 0, pc = lm_sopaque(p); c < LM_PMAX; ++c) if (c < pc) { G[c] /= count; unusable |= !lm_finite(G[c]); }
        need = unusable;        // (for the vote below)
        loss_cur = loss;
    }
    double prior_q = 0.0;
    if constexpr (PRIOR) {
        const pdp_lm_prior& pr = lm_only(prior_arg...);
        // the prior's share (x - mean)' P (x - mean) at the point the rows were evaluated at: all 64 lanes run the shuffles, lanes that are not live carry zeros
        double d = 0.0, Prow[LM_PMAX];
#pragma unroll
        for (int c = 0; c < LM_PMAX; ++c) Prow[c] = 0.0;
        if (live) {
            d = st.trial[k * S * p + r] - pr.mean[k * pr.mean_kstride + r];
            const double* P = pr.precision + k * pr.precision_kstride;
            if (pr.kind == 0) {
                const double Prr = P[r];
#pragma unroll
                for (int c = 0; c < LM_PMAX; ++c) if (c == r) Prow[c] = Prr;
            } else {
#pragma unroll
                for (int c = 0, pc = lm_sopaque(p); c < LM_PMAX; ++c) if (c < pc) Prow[c] = P[r * p + c];
            }
        }
        double Pd = 0.0, Pdiag = 0.0;
#pragma unroll
        for (int c = 0, pc = lm_sopaque(p); c < LM_PMAX; ++c) {
            if (c < pc) Pd += Prow[c] * __shfl(d, c, 16);
            if (c == r) Pdiag = Prow[c];
        }
        if (pr.kind == 0) Pd = Pdiag * d;           // (the single product)
        const double dPd = d * Pd;
#pragma unroll
        for (int c = 0, pc = lm_sopaque(p); c < LM_PMAX; ++c) if (c < pc) prior_q += __shfl(dPd, c, 16);
        if (live) {
            g += Pd;
            loss_cur += prior_q;
            bool unusable = !lm_finite(g) || !lm_finite(loss_cur);
            if (pr.kind == 0) {
#pragma unroll
                for (int c = 0; c < LM_PMAX; ++c) if (c == r) { G[c] += Prow[c]; unusable |= !lm_finite(G[c]); }
            } else {
#pragma unroll
                for (int c = 0, pc = lm_sopaque(p); c < LM_PMAX; ++c) if (c < pc) { G[c] += Prow[c]; unusable |= !lm_finite(G[c]); }
            }
            need |= unusable;
        }
    }
    const bool unusable = lm_row_any(need, quarter);
    need = false;
    if (live) {
        evals += 1;
        double* cur = st.current + k * w;
        if (state == PDP_LM_START) accept = !unusable;
        else accept = !unusable && loss_cur < cur[p];
        if (accept) {
            theta = st.trial[k * S * p + r];
            st.theta[k * p + r] = theta;
            cur[r] = g;
            if (r == 0) cur[p] = loss_cur;
#pragma unroll
            for (int c = 0, pc = lm_sopaque(p); c < LM_PMAX; ++c) if (c < pc) cur[p + 1 + r * p + c] = G[c];
            if (state != PDP_LM_START) { const double l = lam / sch.down; lam = l > sch.lam_min ? l : sch.lam_min; }
            if (acc < L) {
                if (r == 0 && st.loss_trace) st.loss_trace[k * L + acc] = loss_cur;
                if (r == 0 && st.lambda_trace) st.lambda_trace[k * L + acc] = lam;
                if (st.parameter_trace) st.parameter_trace[(k * L + acc) * p + r] = theta;
            }
            if constexpr (PRIOR) if (r == 0 && lm_only(prior_arg...).prior_loss) lm_only(prior_arg...).prior_loss[k] = prior_q;
            acc += 1;
            need = true;
        } else if (state == PDP_LM_START) {
            state = PDP_LM_FAILED;
            theta = st.theta[k * p + r];
        } else {
            rej += 1;
            lam *= sch.up;
            theta = st.theta[k * p + r];
            g = cur[r];
            loss_cur = cur[p];
#pragma unroll
            for (int c = 0, pc = lm_sopaque(p); c < LM_PMAX; ++c) if (c < pc) G[c] = cur[p + 1 + r * p + c];
            need = true;
        }
    } else if (mine) theta = st.theta[k * p + r];

    // where this lane stores behind the loop, as per-lane addresses (and S, p) in vector registers: the kernel arguments are then dead across the loop, whose unrolled
    // column steps need the scalar registers for their lane masks (left in scalar registers, 30 words of them were parked in lanes of a vector register around the loop)
    double* const trial_out = lm_opaque(st.trial + (k * S) * p + r);
    int32_t* const now_out = lm_opaque(st.accepted_now ? st.accepted_now + k * S : (int32_t*)nullptr);
    int32_t* const state_out = lm_opaque(st.state + k);
    int32_t* const evals_out = lm_opaque(st.evaluations + k);
    int32_t* const rej_out = lm_opaque(st.rejected + k);
    int32_t* const acc_out = lm_opaque(st.accepted + k);
    double* const lam_out = lm_opaque(st.lam + k);
    long long* const active_out = lm_opaque((long long*)st.counters + 1);
    const int Sv = lm_opaque(S), pv = lm_opaque(p);
    // termination test, damped solve, next trial point - again with the next damping where the trial cannot be formed
    double trial = theta;
    for (;;) {
        if (need) {
            if (!(loss_cur > sch.loss_tol)) { state = PDP_LM_CONVERGED; need = false; }
            else if (evals >= sch.max_evals) { state = PDP_LM_BUDGET; need = false; }
            else if (lam > sch.lam_max) { state = PDP_LM_STALLED; need = false; }
        }
        if (!__any(need)) break;
        // row q of [G + lam D | g]; columns >= p are zeros nothing reads.  (q, pp: the lane's row and p through opaque copies, so that the lane masks and the
        // "col < p" tests of the 16 column steps are formed where they are used and not kept in scalar registers across the loop)
        const int q = lm_opaque(r), pp = lm_sopaque(p);
        double A[LM_PMAX], b = g;
#pragma unroll
        for (int c = 0; c < LM_PMAX; ++c) {
            A[c] = G[c];
            if (c == q) A[c] = G[c] + (G[c] == 0.0 ? lam : lam * G[c]);
        }
        bool trouble = false;
#pragma unroll
        for (int col = 0; col < LM_PMAX; ++col) {
            if (col < pp) {          // (uniform)
                // the pivot: the largest magnitude of column col among the rows col .. p - 1, ties to the lowest row (a NaN counts as the largest)
                const double a = A[col];
                double v = (q >= col && q < pp) ? (a != a ? __builtin_inf() : __builtin_fabs(a)) : -1.0;
                int at = q;
#pragma unroll
                for (int d = 1; d < 16; d <<= 1) {
                    const double vo = __shfl_xor(v, d, 16);
                    const int ao = __shfl_xor(at, d, 16);
                    if (vo > v || (vo == v && ao < at)) { v = vo; at = ao; }
                }
                // rows col and `at` change places (one shuffle per entry: every other lane reads itself), then the pivot row goes to every lane
                const int from = q == col ? at : (q == at ? col : q);
                double P[LM_PMAX];
#pragma unroll
                for (int c = col; c < LM_PMAX; ++c) {
                    A[c] = __shfl(A[c], from, 16);
                    P[c] = __shfl(A[c], col, 16);
                }
                b = __shfl(b, from, 16);
                const double Pb = __shfl(b, col, 16), piv = P[col];
                if (!(__builtin_fabs(piv) > LM_PIVOT_MIN)) trouble = true;
                const double f = q > col ? A[col] / piv : 0.0;
                if (q > col) {
#pragma unroll
                    for (int c = col + 1; c < LM_PMAX; ++c) A[c] -= f * P[c];
                    b -= f * Pb;
                }
            }
        }
        // back substitution: lane q ends with component q of the step in b
        const int q2 = lm_opaque(r);
#pragma unroll
        for (int col = LM_PMAX - 1; col >= 0; --col) {
            if (col < pp) {
                const double xc = __shfl(b / A[col], col, 16);
                if (q2 == col) b = xc; else if (q2 < col) b -= A[col] * xc;
            }
        }
        const double t = theta - b;
        const bool failed = lm_row_any(trouble || (r < p && !lm_finite(t)), quarter);
        if (need) {
            if (!failed) { trial = t; state = PDP_LM_ACTIVE; need = false; }
            else { evals += 1; rej += 1; lam *= sch.up; }
        }
    }

    if (mine) {
        for (int s = 0; s < Sv; ++s) trial_out[(int64_t)s * pv] = trial;      // (a finished problem: theta)
        if (now_out) for (int s = r; s < Sv; s += pv) now_out[s] = accept ? 1 : 0;
    }
    const bool left = live && r == 0 && state != PDP_LM_ACTIVE;
    if (live && r == 0) { *state_out = state; *evals_out = evals; *rej_out = rej; *acc_out = acc; *lam_out = lam; }
    const int gone = __popcll(__ballot(left));
    if (gone && lane == 0) atomicAdd((unsigned long long*)active_out, (unsigned long long)(-(long long)gone));
}

// cov = scale A^-1 per problem, A = the G of the problem's row: lane r holds row r of [A | I], reduced by the elimination of the update (the same pivot rule, the same
// threshold) and back-substituted per column; lane r ends with row r of A^-1 in its 16 right-hand sides.  A problem that fails (a pivot not > 1e-300, a non-finite
// entry of A or of the result) gets NaN, pivot_ratio 0 and status 1; its neighbours in the wavefront run the same instructions on their own rows.
__global__ void __launch_bounds__(64) lm_covariance_kernel(int K, int p, const double* __restrict__ rows, int rs, const double* __restrict__ scale, double* __restrict__ cov,
                                                           double* __restrict__ std_err, double* __restrict__ pivot_ratio, int32_t* __restrict__ status) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x, r = lane & 15, quarter = lane >> 4;
    const int64_t k = (int64_t)blockIdx.x * 4 + quarter;
    const bool mine = k < K && r < p;
    double A[LM_PMAX], B[LM_PMAX];
    bool trouble = false;
#pragma unroll
    for (int c = 0; c < LM_PMAX; ++c) { A[c] = 0.0; B[c] = c == r ? 1.0 : 0.0; }
    double sc = 1.0;
    if (mine) {
        const double* row = rows + k * (int64_t)rs + p + 1 + r * p;
#pragma unroll
        for (int c = 0, pc = lm_sopaque(p); c < LM_PMAX; ++c) if (c < pc) { A[c] = row[c]; trouble |= !lm_finite(A[c]); }
        if (scale) sc = scale[k];
    }
    // where this lane stores, as per-lane addresses in vector registers, and the lane's row and p through opaque copies: as in lm_update_kernel, the lane masks and the
    // "col < p" tests of the unrolled column steps are then formed where they are used and the kernel arguments are dead across them
    double* const cov_out = lm_opaque(cov + (k * p + r) * p);
    double* const std_out = lm_opaque(std_err ? std_err + k * p + r : (double*)nullptr);
    double* const ratio_out = lm_opaque(pivot_ratio ? pivot_ratio + k : (double*)nullptr);
    int32_t* const status_out = lm_opaque(status + k);
    const int pv = lm_opaque(p);
    double small = __builtin_inf(), large = 0.0;
    {
        const int q = lm_opaque(r), pp = lm_sopaque(p);
#pragma unroll
        for (int col = 0; col < LM_PMAX; ++col) {
            if (col < pp) {          // (uniform)
                const double a = A[col];
                double v = (q >= col && q < pp) ? (a != a ? __builtin_inf() : __builtin_fabs(a)) : -1.0;
                int at = q;
#pragma unroll
                for (int d = 1; d < 16; d <<= 1) {
                    const double vo = __shfl_xor(v, d, 16);
                    const int ao = __shfl_xor(at, d, 16);
                    if (vo > v || (vo == v && ao < at)) { v = vo; at = ao; }
                }
                const int from = q == col ? at : (q == at ? col : q);
                double P[LM_PMAX], PB[LM_PMAX];
#pragma unroll
                for (int c = col; c < LM_PMAX; ++c) {
                    A[c] = __shfl(A[c], from, 16);
                    P[c] = __shfl(A[c], col, 16);
                }
#pragma unroll
                for (int c = 0; c < LM_PMAX; ++c) {
                    B[c] = __shfl(B[c], from, 16);
                    PB[c] = __shfl(B[c], col, 16);
                }
                const double piv = P[col], mag = __builtin_fabs(piv);
                if (!(mag > LM_PIVOT_MIN)) trouble = true;
                if (mag < small) small = mag;
                if (mag > large) large = mag;
                const double f = q > col ? A[col] / piv : 0.0;
                if (q > col) {
#pragma unroll
                    for (int c = col + 1; c < LM_PMAX; ++c) A[c] -= f * P[c];
#pragma unroll
                    for (int c = 0; c < LM_PMAX; ++c) B[c] -= f * PB[c];
                }
            }
        }
    }
    {
        const int q = lm_opaque(r), pp = lm_sopaque(p);
#pragma unroll
        for (int col = LM_PMAX - 1; col >= 0; --col) {
            if (col < pp) {
#pragma unroll
                for (int j = 0; j < LM_PMAX; ++j) {
                    if (j < pp) {        // (uniform; the right-hand sides >= p belong to rows nothing stores)
                        const double xc = __shfl(B[j] / A[col], col, 16);
                        if (q == col) B[j] = xc; else if (q < col) B[j] -= A[col] * xc;
                    }
                }
            }
        }
    }
    const int q = lm_opaque(r);
    double diag = 0.0;
#pragma unroll
    for (int c = 0; c < LM_PMAX; ++c) {
        B[c] *= sc;
        if (c < pv) trouble |= mine && !lm_finite(B[c]);
        if (c == q) diag = B[c];
    }
    const bool failed = lm_row_any(trouble, quarter);
    if (mine) {
        const double nan = __builtin_nan("");
#pragma unroll
        for (int c = 0; c < LM_PMAX; ++c) if (c < pv) cov_out[c] = failed ? nan : B[c];
        if (std_out) *std_out = (failed || diag < 0.0) ? nan : __builtin_sqrt(diag);
        if (q == 0) {
            if (ratio_out) *ratio_out = failed ? 0.0 : small / large;
            *status_out = failed ? 1 : 0;
        }
    }
}

}  // namespace pdp
