"""Shared by tests/test_lm_prior_host.py and tests/test_gpu_lm_prior.py: the numpy restatement of ONE launch of pdp_lm_update_prior_batched and of
pdp_lm_covariance_batched (include/pdp_hip_lm_prior.h), statement by statement as the kernels are (csrc/pdp_lm_kernels.h).  It extends tests/lm_batched_common.py: the
state dict, the pivoted elimination, the damping and the schedule are that module's.

A prior is a dict(mean, precision, kind, prior_loss): mean [p] (shared) or [K, p]; kind 0: precision the diagonal, [p] or [K, p]; kind 1: the full matrix, [p, p] or
[K, p, p]; prior_loss [K] (written in place on acceptance) or None."""
import numpy as np

import lm_batched_common as lb
import sysid_gn_common as sg


def prior_of(prior, k):
    """(mean [p], precision [p] or [p, p], kind) of problem k"""
    mean, prec, kind = np.asarray(prior["mean"], dtype=float), np.asarray(prior["precision"], dtype=float), int(prior["kind"])
    assert kind in (0, 1)
    return (mean if mean.ndim == 1 else mean[k]), (prec if prec.ndim == 1 + kind else prec[k]), kind


def augment(row, p, x, mean, prec, kind):
    """the insertion after the mean row is formed: (the augmented row, the prior's share q of the loss).  Products and sums round separately, in the order written."""
    row = row.copy()
    with np.errstate(all="ignore"):
        d = x - mean
        Pd = np.zeros(p)
        for r in range(p):
            if kind == 0:
                Pd[r] = prec[r] * d[r]
            else:
                acc = 0.0
                for c in range(p):
                    acc = acc + prec[r, c] * d[c]
                Pd[r] = acc
        q = 0.0
        for r in range(p):
            q = q + d[r] * Pd[r]
        row[:p] = row[:p] + Pd
        row[p] = row[p] + q
        G = row[p + 1:p + 1 + p * p].reshape(p, p)          # (a view)
        if kind == 0:
            for r in range(p):
                G[r, r] = G[r, r] + prec[r]
        else:
            G += prec
    return row, q


def launch_prior(st, rows, bad=None, prior=None, **schedule):
    """one launch on the state dict st (in place): lb.launch with the insertion; prior None: the same statements without it"""
    sch = dict(lb.DEFAULT, **schedule)
    K, S, p, L = st["K"], st["S"], st["p"], st["L"]
    w = p + 1 + p * p
    rows = np.asarray(rows, dtype=float)
    st["counters"][0] += 1
    for k in range(K):
        st["accepted_now"][k * S:(k + 1) * S] = 0
        if st["state"][k] not in (lb.START, lb.ACTIVE):
            st["trial"][k * S:(k + 1) * S] = st["theta"][k]
            continue
        with np.errstate(all="ignore"):
            row = np.zeros(w)
            for s in range(S):
                row = row + rows[k * S + s, :w]
            row = row / float(S)
        q = None
        if prior is not None:
            row, q = augment(row, p, st["trial"][k * S], *prior_of(prior, k))
        unusable = (bad is not None and bool(np.asarray(bad)[k * S:(k + 1) * S].any())) or not np.isfinite(row).all()
        st["evaluations"][k] += 1
        first = st["state"][k] == lb.START
        accept = (not unusable) if first else (not unusable and row[p] < st["current"][k, p])
        failed = False
        if accept:
            st["theta"][k] = st["trial"][k * S]
            st["current"][k] = row
            if not first:
                st["lam"][k] = max(st["lam"][k] / sch["down"], sch["lam_min"])
            i = st["accepted"][k]
            if i < L:
                st["loss_trace"][k, i], st["lambda_trace"][k, i], st["parameter_trace"][k, i] = row[p], st["lam"][k], st["theta"][k]
            st["accepted"][k] += 1
            st["accepted_now"][k * S:(k + 1) * S] = 1
            if prior is not None and prior.get("prior_loss") is not None:
                prior["prior_loss"][k] = q
        elif first:
            failed = True
        else:
            st["rejected"][k] += 1
            st["lam"][k] = st["lam"][k] * sch["up"]
        trial = st["theta"][k].copy()
        if failed:
            st["state"][k] = lb.FAILED
        else:
            cur = st["current"][k]
            while True:
                if not cur[p] > sch["loss_tol"]:
                    st["state"][k] = lb.CONVERGED
                elif st["evaluations"][k] >= sch["max_evals"]:
                    st["state"][k] = lb.BUDGET
                elif st["lam"][k] > sch["lam_max"]:
                    st["state"][k] = lb.STALLED
                else:
                    step, ok = lb.solve_pivoted(lb.damped(cur[p + 1:].reshape(p, p), st["lam"][k]), cur[:p])
                    t = st["theta"][k] - step
                    if ok and np.isfinite(t).all():
                        trial, st["state"][k] = t, lb.ACTIVE
                    else:
                        st["evaluations"][k] += 1
                        st["rejected"][k] += 1
                        st["lam"][k] = st["lam"][k] * sch["up"]
                        continue
                break
        st["trial"][k * S:(k + 1) * S] = trial
        if st["state"][k] != lb.ACTIVE:
            st["counters"][1] -= 1
    return st


def run_prior(evaluate_rows, theta0, prior, S=1, lam0=1e-3, max_launches=None, **schedule):
    """lb.run with the prior: the lock-step loop until nothing is START or ACTIVE"""
    sch = dict(lb.DEFAULT, **schedule)
    st = lb.new_state(theta0, S, lam0, trace_len=sch["max_evals"] + 1)
    n = 0
    while st["counters"][1] > 0 and n < (max_launches or sch["max_evals"] + 1):
        rows, bad = evaluate_rows(st["trial"].copy())
        launch_prior(st, rows, bad, prior, **sch)
        n += 1
    st["launches"] = n
    return st


def inverse_pivoted(A):
    """(A^-1, ok, pivot_ratio): [A | I] reduced by lb.solve_pivoted's elimination - the same pivot rule and threshold - and back-substituted per column"""
    A = np.array(A, dtype=float)
    p = A.shape[0]
    B, ok, small, large = np.eye(p), True, np.inf, 0.0
    with np.errstate(all="ignore"):
        for c in range(p):
            mag = np.abs(A[c:, c])
            j = c + int(np.argmax(np.where(np.isnan(mag), np.inf, mag)))
            if j != c:
                A[[c, j]], B[[c, j]] = A[[j, c]], B[[j, c]]
            piv = A[c, c]
            if not abs(piv) > lb.PIVOT_MIN:
                ok = False
            if abs(piv) < small:
                small = abs(piv)
            if abs(piv) > large:
                large = abs(piv)
            for r in range(c + 1, p):
                f = A[r, c] / piv
                A[r, c + 1:] = A[r, c + 1:] - f * A[c, c + 1:]
                B[r] = B[r] - f * B[c]
        for j in range(p):
            for c in range(p - 1, -1, -1):
                B[c, j] = B[c, j] / A[c, c]
                B[:c, j] = B[:c, j] - A[:c, c] * B[c, j]
        ratio = small / large
    return B, ok, ratio


def covariance(rows, scale=None):
    """pdp_lm_covariance_batched on rows [K, >= p + 1 + p p] (p from the width of a packed row is ambiguous for a strided one: rows must be [K, p + 1 + p p]):
    dict(cov [K, p, p], std_err [K, p], pivot_ratio [K], status int32 [K])"""
    rows = np.asarray(rows, dtype=float)
    K, w = rows.shape
    p = int(round((-1 + np.sqrt(1 + 4 * (w - 1))) / 2))
    assert p + 1 + p * p == w
    cov, std, ratio, status = np.zeros((K, p, p)), np.zeros((K, p)), np.zeros(K), np.zeros(K, dtype=np.int32)
    for k in range(K):
        A = rows[k, p + 1:].reshape(p, p)
        inv, ok, pr = inverse_pivoted(A)
        with np.errstate(all="ignore"):
            C = (1.0 if scale is None else float(np.asarray(scale)[k])) * inv
            s = np.where(np.diag(C) < 0, np.nan, np.sqrt(np.abs(np.diag(C))))
        if ok and np.isfinite(A).all() and np.isfinite(C).all():
            cov[k], std[k], ratio[k] = C, s, pr
        else:
            cov[k], std[k], ratio[k], status[k] = np.nan, np.nan, 0.0, 1
    return dict(cov=cov, std_err=std, pivot_ratio=ratio, status=status)


# ---- the pendulum SysID case with a prior -----------------------------------------------------------------------------------------------------------------------------------
# With a prior the smallest loss is not 0, so no loss_tol ends these loops; started at the stored run's theta times 1, 0.9, 1.1 they take no rejected trial and reach the
# fp64 floor of the augmented loss after 6 - 9 accepted points (relative changes of 1e-15), where "strictly lower" is decided by the rounding of the solver in use.
# Hence other inputs: the starts 0.5, 1.5 and 2 times that theta, from which every problem rejects 4 - 7 trials in its first 12 evaluations, and a budget of 12
# evaluations, which ends every loop while its accepted losses still fall by more than 1e-4 relative - there two solvers that agree to rounding decide alike.
PRIOR_SCHEDULE = dict(max_evals=12, loss_tol=0.0)
PRIOR_STARTS = (0.5, 1.5, 2.0)


def prior_starts(c):
    """theta0 [K, p] of the pendulum case with a prior: problem 3 i + b starts from PRIOR_STARTS[i] times the stored run's theta"""
    theta = sg.stored(c["system"])[3]
    return np.stack([PRIOR_STARTS[(k * c["S"]) // 3] * theta for k in range(c["K"])])


def pendulum_prior(c):
    """the prior of the pendulum case: centred 5 per cent off the stored run's theta, a full precision of the size of J'J / 10 (so that neither term is negligible)"""
    p = c["theta0"].shape[1]
    rng = np.random.default_rng(4)
    M = rng.standard_normal((p, p))
    _, _, _, theta = sg.stored(c["system"])
    return 1.05 * theta, 3.0 * (M @ M.T + np.eye(p))


# ---- inputs of the covariance tests -------------------------------------------------------------------------------------------------------------------------------------------
def spd(p, seed, cond=1e3):
    rng = np.random.default_rng([seed, p])
    Q = np.linalg.qr(rng.standard_normal((p, p)))[0]
    e = np.exp(np.linspace(0.0, np.log(cond), p)) if p > 1 else np.array([2.5])
    A = (Q * e) @ Q.T
    return 0.5 * (A + A.T)


def cov_rows(mats):
    p = mats[0].shape[0]
    return np.stack([np.concatenate([np.zeros(p), [1.0], np.asarray(A, float).ravel()]) for A in mats])
