"""Shared by tests/test_lm_batched_host.py and tests/test_gpu_lm_batched.py: the numpy restatement of ONE launch of pdp_lm_update_batched (include/pdp_hip_lm.h) - many
independent Levenberg-Marquardt problems advanced in lock-step, each exactly as pdp_amd.irl.LMLoop advances one - with its own pivoted elimination (no numpy.linalg), the
inputs of the SysID cases (tests/sysid_gn_common.stored with three start scales, and the groupings), and the scripted synthetic rows of the kernel test.

The restatement works on a dict of arrays laid out as the device state (pdp_lm_state), in place; launch() is the kernel.  Arithmetic is written statement by statement as
the kernel's (products and sums round separately; the sample sum runs in ascending order from 0.0; one division by S), so that the decisions - and, where the compiler
keeps the order, the bits - agree."""
import numpy as np

import sysid_gn_common as sg

START, ACTIVE, CONVERGED, STALLED, BUDGET, FAILED = range(6)
NAMES = ["START", "ACTIVE", "CONVERGED", "STALLED", "BUDGET", "FAILED"]
PIVOT_MIN = 1e-300
DEFAULT = dict(up=10.0, down=10.0, lam_min=1e-12, lam_max=1e8, loss_tol=0.0, max_evals=50)      # irl.LMLoop's default schedule


def new_state(theta0, S, lam0=1e-3, trace_len=0):
    """the caller's initialisation of pdp_lm_state for theta0 [K, p] (lam0: a number or [K])"""
    theta0 = np.array(theta0, dtype=float)
    K, p = theta0.shape
    L = int(trace_len)
    return dict(K=K, S=int(S), p=p, L=L, theta=theta0.copy(), trial=np.repeat(theta0, S, axis=0), lam=np.broadcast_to(np.asarray(lam0, dtype=float), (K,)).copy(),
                current=np.zeros((K, p + 1 + p * p)), state=np.full(K, START, dtype=np.int32), evaluations=np.zeros(K, dtype=np.int32),
                rejected=np.zeros(K, dtype=np.int32), accepted=np.zeros(K, dtype=np.int32), accepted_now=np.zeros(K * S, dtype=np.int32),
                loss_trace=np.zeros((K, L)), lambda_trace=np.zeros((K, L)), parameter_trace=np.zeros((K, L, p)), counters=np.array([0, K], dtype=np.int64))


def solve_pivoted(A, b):
    """(x, ok): Gaussian elimination with partial pivoting on copies - the pivot of column c is the entry of largest magnitude among the rows c .., the first of equal
    ones (argmax); ok is False where a pivot is not > PIVOT_MIN in magnitude (the elimination goes on regardless, as the kernel's does)"""
    A, b = np.array(A, dtype=float), np.array(b, dtype=float)
    p, ok = len(b), True
    with np.errstate(all="ignore"):
        for c in range(p):
            mag = np.abs(A[c:, c])
            j = c + int(np.argmax(np.where(np.isnan(mag), np.inf, mag)))
            if j != c:
                A[[c, j]], b[[c, j]] = A[[j, c]], b[[j, c]]
            piv = A[c, c]
            if not abs(piv) > PIVOT_MIN:
                ok = False
            for r in range(c + 1, p):
                f = A[r, c] / piv
                A[r, c + 1:] = A[r, c + 1:] - f * A[c, c + 1:]
                b[r] = b[r] - f * b[c]
        for c in range(p - 1, -1, -1):
            b[c] = b[c] / A[c, c]
            b[:c] = b[:c] - A[:c, c] * b[c]
    return b, ok


def damped(G, lam):
    """G + lam D with D_ii = G_ii, or 1 where G_ii == 0 (irl.lm_step's rule)"""
    A = np.array(G, dtype=float)
    for i in range(A.shape[0]):
        d = A[i, i]
        A[i, i] = d + (lam if d == 0.0 else lam * d)
    return A


def launch(st, rows, bad=None, **schedule):
    """one launch on the state dict st (in place).  rows [K S, >= p + 1 + p p]: grad | loss | G per sample; bad [K S] or None"""
    sch = dict(DEFAULT, **schedule)
    K, S, p, L = st["K"], st["S"], st["p"], st["L"]
    w = p + 1 + p * p
    rows = np.asarray(rows, dtype=float)
    st["counters"][0] += 1
    for k in range(K):
        st["accepted_now"][k * S:(k + 1) * S] = 0
        if st["state"][k] not in (START, ACTIVE):
            st["trial"][k * S:(k + 1) * S] = st["theta"][k]
            continue
        with np.errstate(all="ignore"):
            row = np.zeros(w)
            for s in range(S):
                row = row + rows[k * S + s, :w]
            row = row / float(S)
        unusable = (bad is not None and bool(np.asarray(bad)[k * S:(k + 1) * S].any())) or not np.isfinite(row).all()
        st["evaluations"][k] += 1
        first = st["state"][k] == START
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
        elif first:
            failed = True
        else:
            st["rejected"][k] += 1
            st["lam"][k] = st["lam"][k] * sch["up"]
        trial = st["theta"][k].copy()
        if failed:
            st["state"][k] = FAILED
        else:
            cur = st["current"][k]
            while True:
                if not cur[p] > sch["loss_tol"]:
                    st["state"][k] = CONVERGED
                elif st["evaluations"][k] >= sch["max_evals"]:
                    st["state"][k] = BUDGET
                elif st["lam"][k] > sch["lam_max"]:
                    st["state"][k] = STALLED
                else:
                    step, ok = solve_pivoted(damped(cur[p + 1:].reshape(p, p), st["lam"][k]), cur[:p])
                    t = st["theta"][k] - step
                    if ok and np.isfinite(t).all():
                        trial, st["state"][k] = t, ACTIVE
                    else:                               # a trial that cannot be formed still counts (LMLoop.step)
                        st["evaluations"][k] += 1
                        st["rejected"][k] += 1
                        st["lam"][k] = st["lam"][k] * sch["up"]
                        continue
                break
        st["trial"][k * S:(k + 1) * S] = trial
        if st["state"][k] != ACTIVE:
            st["counters"][1] -= 1
    return st


def run(evaluate_rows, theta0, S=1, lam0=1e-3, max_launches=None, **schedule):
    """the lock-step loop: evaluate_rows(trial [K S, p]) -> (rows, bad or None); launches until nothing is START or ACTIVE.  Returns the state dict with the number of
    launches and, per problem, the launch at which it finished"""
    sch = dict(DEFAULT, **schedule)
    st = new_state(theta0, S, lam0, trace_len=sch["max_evals"] + 1)
    st["finished_at"] = np.zeros(st["K"], dtype=int)
    n = 0
    while st["counters"][1] > 0 and n < (max_launches or sch["max_evals"] + 1):
        rows, bad = evaluate_rows(st["trial"].copy())
        launch(st, rows, bad, **sch)
        n += 1
        st["finished_at"][(st["finished_at"] == 0) & ~np.isin(st["state"], (START, ACTIVE))] = n
    st["launches"] = n
    return st


# ---- the SysID cases: one problem per (start scale, trajectory) or per start scale with all trajectories -------------------------------------------------------------------
SCALES = (1.0, 0.9, 1.1)
SYSID_CASES = [("pendulum", 1), ("cartpole", 1), ("quadrotor", 1), ("pendulum", 3), ("cartpole", 3)]          # (system, S): K = 9 at S = 1, K = 3 at S = 3
SCHEDULE = dict(max_evals=30, loss_tol=1e-16)


def sysid_case(system, S):
    """dict(inputs [K S, T, m], states [K S, T+1, n], theta0 [K, p], true_parameter): problem k = (scale k // (3 / S), trajectory ...) - at S = 1 problem 3 i + b is
    trajectory b from SCALES[i] times the stored run's theta, at S = 3 problem i is all three trajectories from SCALES[i] times it"""
    inputs, states, true_parameter, theta = sg.stored(system)
    B = inputs.shape[0]
    assert B == 3 and S in (1, 3)
    K = len(SCALES) * B // S
    return dict(system=system, S=S, K=K, inputs=np.concatenate([inputs] * len(SCALES)), states=np.concatenate([states] * len(SCALES)),
                theta0=np.stack([SCALES[(k * S) // B] * theta for k in range(K)]), true_parameter=true_parameter)


def oracle_rows(c, ini_state=None, skip_missing=False):
    """evaluate_rows on the CPU reference (SysIDOracle): per-sample parameters, the packed layout"""
    sid = sg.oracle(c["system"])

    def evaluate_rows(trial):
        loss, grad, G = sg.reference_rows(sid, c["inputs"], c["states"], trial, ini_state, skip_missing)
        return np.concatenate([grad, loss[:, None], G.reshape(len(loss), -1)], axis=1), None
    return evaluate_rows


def independent_loops(c, ini_state=None, skip_missing=False, **schedule):
    """K independent irl.LMLoop runs on the CPU reference, each on its own S samples: list of results()"""
    from pdp_amd.irl import LMLoop
    sid, S, out = sg.oracle(c["system"]), c["S"], []
    sch = dict(DEFAULT, **schedule)
    for k in range(c["K"]):
        own = range(k * S, (k + 1) * S)

        def evaluate(theta, own=own):
            loss, grad, G = sg.reference_rows(sid, c["inputs"], c["states"], theta, ini_state, skip_missing, samples=own)
            with np.errstate(all="ignore"):
                return loss.mean(), grad.mean(axis=0), G.mean(axis=0)
        loop = LMLoop(evaluate, c["theta0"][k], up=sch["up"], down=sch["down"], lam_min=sch["lam_min"], lam_max=sch["lam_max"])
        out.append(loop.run(max_evals=sch["max_evals"], loss_tol=sch["loss_tol"]))
    return out


# ---- the scripted synthetic rows of the kernel test ---------------------------------------------------------------------------------------------------------------------------
# problem k plays scenario k % 10 over four launches; what each launch hands in is (loss, kind): kind "ok" a fresh well-conditioned row, "same" the rows of the launch
# before (an EQUAL loss), "nan" a NaN in the last entry of G of the last sample, "bad" a finite row whose bad flag is set
SCRIPT_SCHEDULE = dict(up=10.0, down=10.0, lam_min=1e-12, lam_max=1e8, loss_tol=1e-3, max_evals=8)
SCRIPT_TRACE_LEN = 2
SCENARIOS = [
    dict(name="accept, accept (trace full), equal loss rejected, higher loss rejected", launches=[(5.0, "ok"), (4.0, "ok"), (4.0, "same"), (4.5, "ok")]),
    dict(name="FAILED at START (NaN row)", launches=[(5.0, "nan"), (4.0, "ok"), (3.0, "ok"), (2.0, "ok")]),
    dict(name="bad flag rejected, accept, NaN row rejected", launches=[(5.0, "ok"), (4.0, "bad"), (4.0, "ok"), (3.0, "nan")]),
    dict(name="a zero diagonal entry is damped by lam itself", launches=[(5.0, "ok"), (4.0, "ok"), (3.0, "ok"), (3.5, "ok")], zero_diagonal=True),
    dict(name="exactly singular damped matrix: five trials rejected inside the launch, then BUDGET", launches=[(5.0, "ok"), (4.0, "ok"), (3.0, "ok"), (2.0, "ok")],
         singular=True, lam0=1e-20),
    dict(name="lam_min floor", launches=[(5.0, "ok"), (4.0, "ok"), (3.0, "ok"), (2.0, "ok")], lam0=5e-12),
    dict(name="STALLED", launches=[(5.0, "ok"), (6.0, "ok"), (4.0, "ok"), (3.0, "ok")], lam0=5e7),
    dict(name="CONVERGED, then left alone", launches=[(5.0, "ok"), (1e-4, "ok"), (1e-5, "ok"), (1e-6, "ok")]),
    dict(name="four acceptances into a trace of two", launches=[(5.0, "ok"), (4.0, "ok"), (3.0, "ok"), (2.0, "ok")]),
    dict(name="CONVERGED at START", launches=[(5e-4, "ok"), (4.0, "ok"), (3.0, "ok"), (2.0, "ok")]),
]


def script_lam0(K):
    return np.array([SCENARIOS[k % len(SCENARIOS)].get("lam0", 1e-3) for k in range(K)])


def script_rows(K, S, p, launch_no, seed=0):
    """(rows [K S, p + 1 + p p], bad int32 [K S]) of launch `launch_no` (0 .. 3; beyond: fresh finite rows of loss 1).  G = Q diag(e) Q' with e in [1, 1e3]; the S samples
    of a problem differ by a few per cent and their mean loss is the scripted one to rounding, except "same", which repeats the rows of the launch before bit by bit"""
    w = p + 1 + p * p
    rows, bad = np.zeros((K * S, w)), np.zeros(K * S, dtype=np.int32)
    for k in range(K):
        sc = SCENARIOS[k % len(SCENARIOS)]
        loss, kind = sc["launches"][launch_no] if launch_no < 4 else (1.0, "ok")
        src = launch_no - 1 if kind == "same" else launch_no
        rng = np.random.default_rng([seed, k, src])
        Q = np.linalg.qr(rng.standard_normal((p, p)))[0]
        G = (Q * np.exp(rng.uniform(0.0, np.log(1e3), p))) @ Q.T
        G = 0.5 * (G + G.T)
        g = rng.standard_normal(p)
        if sc.get("zero_diagonal"):
            j = p // 2
            G[j, :], G[:, j] = 0.0, 0.0
        if sc.get("singular") and p > 1:
            G, g = np.ones((p, p)), np.zeros(p)              # (g = 0: the step is exactly 0 whatever the rounding of the elimination)
        if kind == "same":
            loss = sc["launches"][src][0]
        for s in range(S):
            f = 1.0 + 0.03 * (s - (S - 1) / 2.0)                    # (the factors of a problem's samples average to 1)
            rows[k * S + s] = np.concatenate([g * f, [loss * f], (G * (1.0 if sc.get("singular") else f)).ravel()])
        if kind == "nan":
            rows[k * S + S - 1, w - 1] = np.nan
        if kind == "bad":
            bad[k * S + S - 1] = 1
    return rows, bad
