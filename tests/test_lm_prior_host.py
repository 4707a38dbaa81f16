"""CPU (no GPU needed): the Gaussian prior of the Levenberg-Marquardt loops and the covariance of their estimates (include/pdp_hip_lm_prior.h) - at the ABI (the extension
header, the two symbols, their argument errors before any launch), the numpy restatement of both kernels (tests/lm_prior_common.py), which is the yardstick of the GPU
tests, irl.LMLoop with a prior on a linear model against the closed form, the restatement against K independent irl.LMLoop runs with the same prior, the entry count of
runtime.count_observed against the oracle's residual vector, and the ValueErrors of the Python layer on the paths that need no device."""
import ctypes as C
import os

import numpy as np
import pytest

import lm_batched_common as lb
import lm_prior_common as lp
import sysid_gn_common as sg

ROOT = sg.ROOT


def _built():
    import __graft_entry__ as g
    g.build()
    from pdp_amd import codegen, runtime as rt
    return codegen, rt


def test_the_entry_points_are_declared_listed_and_exported():
    """(tests/test_abi_table.py holds the whole binding against the headers and the built libraries; what stays here is this header's own)"""
    codegen, rt = _built()
    from pdp_amd import abi
    assert list(abi.entry_points("pdp_hip_lm_prior.h", "core")) == ["pdp_lm_update_prior_batched", "pdp_lm_covariance_batched"]
    assert '#include "pdp_hip_lm.h"' in open(os.path.join(ROOT, "include", "pdp_hip_lm_prior.h")).read()
    assert [f[0] for f in rt.PdpLmPrior._fields_] == ["mean", "precision", "kind", "mean_kstride", "precision_kstride", "prior_loss"]
    assert C.sizeof(rt.PdpLmPrior) == 48                                          # (two pointers, int32 + padding, two int64, one pointer)
    assert os.path.join(codegen.CSRC, "pdp_lm_kernels.h") in codegen.source_closure(os.path.join(codegen.CSRC, "pdp_lqr.hip"))
    assert os.path.join(ROOT, "include", "pdp_hip_lm_prior.h") in [os.path.normpath(f) for f in codegen.source_closure(os.path.join(codegen.CSRC, "pdp_lqr.hip"))]


def test_argument_errors_are_returned_before_any_launch():
    """Valid (host) pointers everywhere, so that only the argument under test can be what is refused.  Nothing that passes the checks is called: no GPU is needed."""
    codegen, rt = _built()
    lib = rt.load_core()
    keep = [(C.c_double * 512)() for _ in range(20)]
    P = [C.cast(k, C.c_void_p).value for k in keep]
    K, S, p = 2, 2, 3
    w = p + 1 + p * p
    fields = [f[0] for f in rt.PdpLmState._fields_]

    def update(K=K, S=S, p=p, rows=P[0], stride=w, bad=P[1], sch=None, st=None, null_sch=False, null_st=False, prior=None):
        sch = rt.PdpLmSchedule(10.0, 10.0, 1e-12, 1e8, 0.0, 50) if sch is None else sch
        full = dict(zip(fields, P[2:14] + [4, P[14]]))
        full.update(st or {})
        stt = rt.PdpLmState(*[full[f] for f in fields])
        pr = dict(mean=P[15], precision=P[16], kind=1, mean_kstride=p, precision_kstride=p * p, prior_loss=P[17])
        pr.update(prior or {})
        prs = rt.PdpLmPrior(*[pr[f[0]] for f in rt.PdpLmPrior._fields_])
        return lib.pdp_lm_update_prior_batched(K, S, p, rows, stride, bad, None if null_sch else C.byref(sch), None if null_st else C.byref(stt), C.byref(prs), None)
    for kw in (dict(K=0), dict(K=-1), dict(S=0), dict(p=0), dict(p=-2), dict(rows=None), dict(stride=w - 1), dict(stride=0), dict(null_sch=True), dict(null_st=True),
               dict(sch=rt.PdpLmSchedule(0.0, 10.0, 1e-12, 1e8, 0.0, 50)), dict(sch=rt.PdpLmSchedule(10.0, -1.0, 1e-12, 1e8, 0.0, 50)),
               dict(sch=rt.PdpLmSchedule(float("nan"), 10.0, 1e-12, 1e8, 0.0, 50)), dict(st=dict(trace_len=-1)),
               dict(prior=dict(mean=None)), dict(prior=dict(precision=None)), dict(prior=dict(kind=2)), dict(prior=dict(kind=-1)), dict(prior=dict(mean_kstride=-1)),
               dict(prior=dict(precision_kstride=-3))) + \
            tuple(dict(st={f: None}) for f in ("theta", "trial", "lam", "current", "state", "evaluations", "rejected", "accepted", "counters")):
        assert update(**kw) == -1, kw                                             # PDP_E_ARG
    assert update(p=17, stride=17 + 1 + 17 * 17) == -2                            # PDP_E_SIZE
    assert update(p=17, stride=5) == -2 and update(p=17, rows=None) == -1 and update(p=17, prior=dict(kind=2)) == -1 and update(K=0, p=17) == -1
    # prior == NULL is pdp_lm_update_batched: its errors, in its order
    sch = rt.PdpLmSchedule(10.0, 10.0, 1e-12, 1e8, 0.0, 50)
    stt = rt.PdpLmState(*(P[2:14] + [4, P[14]]))
    assert lib.pdp_lm_update_prior_batched(0, S, p, P[0], w, None, C.byref(sch), C.byref(stt), None, None) == -1
    assert lib.pdp_lm_update_prior_batched(K, S, 17, P[0], 5, None, C.byref(sch), C.byref(stt), None, None) == -2
    assert lib.pdp_lm_update_prior_batched(K, S, p, P[0], w - 1, None, C.byref(sch), C.byref(stt), None, None) == -1

    def cov(K=K, p=p, rows=P[0], stride=w, scale=P[1], out=P[2], std=P[3], ratio=P[4], status=P[5]):
        return lib.pdp_lm_covariance_batched(K, p, rows, stride, scale, out, std, ratio, status, None)
    for kw in (dict(K=0), dict(K=-3), dict(p=0), dict(p=-1), dict(rows=None), dict(out=None), dict(status=None), dict(stride=w - 1), dict(stride=0)):
        assert cov(**kw) == -1, kw
    assert cov(p=17, stride=17 + 1 + 17 * 17) == -2 and cov(p=17, stride=5) == -2 and cov(p=17, rows=None) == -1 and cov(K=0, p=17) == -1
    assert all(v == 0.0 for k in keep for v in k)                                 # (and nothing was written by the host code)


# ---- the restatement of the update -----------------------------------------------------------------------------------------------------------------------------------------
def test_no_prior_is_the_restatement_of_the_plain_update():
    """launch_prior(prior=None) and lb.launch over the six scripted launches at K = 10, S = 2, p = 7: every array bit-equal after every launch"""
    K, S, p = 10, 2, 7
    theta0 = np.random.default_rng(1).standard_normal((K, p))
    a = lb.new_state(theta0, S, lam0=lb.script_lam0(K), trace_len=lb.SCRIPT_TRACE_LEN)
    b = lb.new_state(theta0, S, lam0=lb.script_lam0(K), trace_len=lb.SCRIPT_TRACE_LEN)
    for n in range(6):
        rows, bad = lb.script_rows(K, S, p, n, seed=p)
        lb.launch(a, rows, bad, **lb.SCRIPT_SCHEDULE)
        lp.launch_prior(b, rows, bad, None, **lb.SCRIPT_SCHEDULE)
        for key, v in a.items():
            if isinstance(v, np.ndarray):
                assert np.array_equal(v, b[key], equal_nan=True), (n, key)
    assert set(a["state"]) >= {lb.ACTIVE, lb.CONVERGED, lb.STALLED, lb.BUDGET, lb.FAILED}


def _row(g, loss, G):
    return np.concatenate([np.asarray(g, float), [loss], np.asarray(G, float).ravel()])[None]


@pytest.mark.parametrize("kind", [0, 1], ids=["diagonal", "full"])
def test_by_hand_zero_rows(kind):
    """rows all zero, P = diag(2, 4), mean = (1, -1), theta0 = 0: the augmented loss is exactly 6, g = P (theta - mean), the first trial theta - solve(P + lam diag P, g);
    then accept, reject and restore of the augmented row, prior_loss written on acceptance only"""
    P = np.diag([2.0, 4.0])
    prior = dict(mean=np.array([1.0, -1.0]), precision=np.array([2.0, 4.0]) if kind == 0 else P, kind=kind, prior_loss=np.full(1, np.nan))
    st = lb.new_state([[0.0, 0.0]], 1, lam0=1e-3, trace_len=4)
    zero = np.zeros((1, 2 + 1 + 4))
    lp.launch_prior(st, zero, None, prior)
    cur = st["current"][0]
    assert cur[2] == 6.0 and np.array_equal(cur[:2], [-2.0, 4.0]) and np.array_equal(cur[3:].reshape(2, 2), P) and prior["prior_loss"][0] == 6.0
    assert st["state"][0] == lb.ACTIVE and st["loss_trace"][0, 0] == 6.0
    trial = -np.linalg.solve(P + 1e-3 * np.diag(np.diag(P)), [-2.0, 4.0])
    assert np.abs(st["trial"][0] - trial).max() <= 1e-15
    # the trial point is nearly the prior's mean: its augmented loss is tiny, it is accepted and the augmented row is what current holds
    lp.launch_prior(st, zero, None, prior)
    t = st["theta"][0].copy()
    d = t - [1.0, -1.0]
    assert st["accepted"][0] == 2 and np.array_equal(t, st["parameter_trace"][0, 1]) and st["current"][0, 2] == prior["prior_loss"][0] == d[0] * (2.0 * d[0]) + d[1] * (4.0 * d[1])
    assert np.array_equal(st["current"][0, :2], [2.0 * d[0], 4.0 * d[1]]) and st["lam"][0] == 1e-3 / 10.0
    # a data row whose loss makes the trial worse: rejected - current, theta and prior_loss stay, lam moves, the next trial is solved from the AUGMENTED current row
    before, q = st["current"][0].copy(), prior["prior_loss"][0]
    lp.launch_prior(st, _row([1.0, 1.0], 1.0, np.eye(2)), None, prior)
    assert st["rejected"][0] == 1 and np.array_equal(st["current"][0], before) and prior["prior_loss"][0] == q and np.array_equal(st["theta"][0], t) and st["lam"][0] == 1e-3 / 10.0 * 10.0
    step, ok = lb.solve_pivoted(lb.damped(P, 1e-3 / 10.0 * 10.0), before[:2])
    assert ok and np.array_equal(st["trial"][0], t - step)
    # a NaN in the precision makes the trial unusable (the unusable test covers the augmented values)
    worse = dict(prior, precision=np.array([2.0, np.nan]) if kind == 0 else np.array([[2.0, 0.0], [0.0, np.nan]]))
    lp.launch_prior(st, zero, None, worse)
    assert st["rejected"][0] == 2 and np.array_equal(st["current"][0], before) and prior["prior_loss"][0] == q


def test_per_problem_and_shared_priors_and_the_sample_mean():
    """the prior is added to the MEAN row (after the division by S), per problem from [K, ...] arrays and shared from [p] / [p, p]"""
    K, S, p = 3, 2, 4
    rng = np.random.default_rng(2)
    theta0 = rng.standard_normal((K, p))
    rows = lb.script_rows(K, S, p, 4, seed=3)[0]                 # (launch 4: fresh finite rows for every problem)
    M = rng.standard_normal((K, p, p))
    full = M @ M.transpose(0, 2, 1)
    mean = rng.standard_normal((K, p))
    for prior in (dict(mean=mean, precision=full, kind=1), dict(mean=mean[0], precision=full[0], kind=1), dict(mean=mean, precision=np.abs(mean), kind=0),
                  dict(mean=mean[1], precision=np.abs(mean[2]), kind=0)):
        st = lb.new_state(theta0, S, trace_len=1)
        lp.launch_prior(st, rows, None, dict(prior, prior_loss=None), max_evals=5)
        for k in range(K):
            m, P, kind = lp.prior_of(prior, k)
            Pf = np.diag(P) if kind == 0 else P
            row = rows[2 * k:2 * k + 2].sum(axis=0) / 2.0
            d = theta0[k] - m
            want = np.concatenate([row[:p] + Pf @ d, [row[p] + d @ Pf @ d], (row[p + 1:].reshape(p, p) + Pf).ravel()])
            assert np.abs(st["current"][k] - want).max() <= 1e-13 * np.abs(want).max()


# ---- LMLoop with a prior --------------------------------------------------------------------------------------------------------------------------------------------------
def test_linear_model_reaches_the_closed_form_and_its_covariance():
    """r = J theta - y (20 x 4, seeded), full P: LMLoop reaches (J'J + P)^-1 (J'y + P mean) to 1e-10 relative; covariance("known") is inv(J'J + P) to the same tolerance"""
    from pdp_amd.irl import LMLoop
    rng = np.random.default_rng(11)
    J, y, mean = rng.standard_normal((20, 4)), rng.standard_normal(20), rng.standard_normal(4)
    M = rng.standard_normal((4, 4))
    P = M @ M.T

    def evaluate(theta):
        r = J @ theta - y
        return r @ r, J.T @ r, J.T @ J
    loop = LMLoop(evaluate, np.zeros(4), prior_mean=mean, prior_precision=P)
    res = loop.run(max_evals=60)
    want = np.linalg.solve(J.T @ J + P, J.T @ y + P @ mean)
    print("LMLoop with a prior on a linear model: %d evaluations, |theta - closed form| / |closed form| = %.2e" % (res["evaluations"], np.abs(loop.theta - want).max() / np.abs(want).max()))
    assert np.abs(loop.theta - want).max() <= 1e-10 * np.abs(want).max()
    d = loop.theta - mean
    assert abs(res["prior_loss"] - d @ P @ d) <= 1e-12 * (d @ P @ d) and res["loss_trace"][-1] >= res["prior_loss"]
    cov = loop.covariance("known")
    inv = np.linalg.inv(J.T @ J + P)
    assert cov["status"] == 0 and np.abs(cov["cov"] - inv).max() <= 1e-10 * np.abs(inv).max() and np.allclose(cov["std_err"], np.sqrt(np.diag(inv)), rtol=1e-10, atol=0)
    assert 0.0 < cov["pivot_ratio"] <= 1.0 and cov["sigma2"] == 1.0
    with pytest.raises(ValueError, match="prior"):
        loop.covariance("estimated", n_observed=20)
    # without a prior: the ordinary least-squares estimate, sigma^2 = |r|^2 / (N - p) and Cov = sigma^2 (J'J)^-1; N has to be given for a plain evaluate
    plain = LMLoop(evaluate, np.zeros(4))
    plain.run(max_evals=60)
    ols = np.linalg.lstsq(J, y, rcond=None)[0]
    assert np.abs(plain.theta - ols).max() <= 1e-10 * np.abs(ols).max() and "prior_loss" not in plain.results()
    with pytest.raises(NotImplementedError):
        plain.covariance("estimated")
    c = plain.covariance("estimated", n_observed=20)
    s2 = ((J @ ols - y) ** 2).sum() / 16.0
    assert abs(c["sigma2"] - s2) <= 1e-10 * s2 and np.abs(c["cov"] - s2 * np.linalg.inv(J.T @ J)).max() <= 1e-10 * s2 * np.abs(np.linalg.inv(J.T @ J)).max()
    assert np.isnan(plain.covariance("estimated", n_observed=4)["cov"]).all()      # N <= p
    diag = LMLoop(evaluate, np.zeros(4), prior_mean=mean, prior_precision=np.array([1.0, 2.0, 3.0, 4.0]))
    diag.run(max_evals=60)
    want = np.linalg.solve(J.T @ J + np.diag([1.0, 2.0, 3.0, 4.0]), J.T @ y + np.array([1.0, 2.0, 3.0, 4.0]) * mean)
    assert np.abs(diag.theta - want).max() <= 1e-10 * np.abs(want).max()


def test_restatement_with_a_prior_against_independent_lm_loops():
    """the lock-step restatement with a prior and K independent irl.LMLoop runs with the same prior take the same decisions on the oracle's rows: evaluations, rejected
    and accepted counts equal per problem; the accepted losses equal to solver rounding"""
    from pdp_amd.irl import LMLoop
    c = lb.sysid_case("pendulum", 1)
    mean, P = lp.pendulum_prior(c)
    theta0 = lp.prior_starts(c)
    st = lp.run_prior(lb.oracle_rows(c), theta0, dict(mean=mean, precision=P, kind=1, prior_loss=np.zeros(c["K"])), S=1, **lp.PRIOR_SCHEDULE)
    sid = sg.oracle("pendulum")
    worst = 0.0
    for k in range(c["K"]):
        def evaluate(theta, k=k):
            loss, grad, G = sg.reference_rows(sid, c["inputs"], c["states"], theta, samples=[k])
            return loss[0], grad[0], G[0]
        loop = LMLoop(evaluate, theta0[k], prior_mean=mean, prior_precision=P)
        r = loop.run(max_evals=lp.PRIOR_SCHEDULE["max_evals"], loss_tol=lp.PRIOR_SCHEDULE["loss_tol"])
        assert (st["evaluations"][k], st["rejected"][k], st["accepted"][k]) == (r["evaluations"], r["rejected"], r["iterations"]), (k, r["evaluations"], r["rejected"])
        a, b = st["loss_trace"][k, :st["accepted"][k]], r["loss_trace"]
        worst = max(worst, float((np.abs(a - b) / b).max()))
        assert np.abs(st["theta"][k] - loop.theta).max() <= 1e-6 * np.abs(loop.theta).max()
    print("pendulum K = 9 with a prior: evaluations %s rejected %s states %s; accepted losses differ by %.2e relative" % (list(st["evaluations"]), list(st["rejected"]),
                                                                                                                       [lb.NAMES[s] for s in st["state"]], worst))
    assert worst <= 1e-6
    assert st["rejected"].min() >= 1                # (if the inputs stop producing a rejected trial, the inputs are to be changed, not the rule)


def test_augmented_gradient_is_the_half_derivative_of_the_augmented_loss():
    """central differences (h = 1e-6) of the augmented loss of one pendulum trajectory against the augmented g of the restatement: 1e-7 of its largest entry, the tolerance
    of the central-difference tests of the SysID rows"""
    c = lb.sysid_case("pendulum", 1)
    mean, P = lp.pendulum_prior(c)
    sid, k = sg.oracle("pendulum"), 4
    x = c["theta0"][k]

    def rows_at(theta):
        loss, grad, G = sg.reference_rows(sid, c["inputs"], c["states"], theta, samples=[k])
        return np.concatenate([grad[0], loss, G[0].ravel()])

    def loss(theta):
        return lp.augment(rows_at(theta), x.size, theta, mean, P, 1)[0][x.size]
    g = lp.augment(rows_at(x), x.size, x, mean, P, 1)[0][:x.size]
    h = 1e-6
    fd = np.array([(loss(x + h * e) - loss(x - h * e)) / (2 * h) for e in np.eye(x.size)]) / 2
    err = np.abs(fd - g).max() / np.abs(g).max()
    print("augmented g vs central differences: %.2e" % err)
    assert err <= 1e-7


# ---- the restatement of the covariance ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 5, 13, 16])
def test_covariance_restatement_inverts(p):
    mats = [lp.spd(p, s) for s in range(3)]
    scale = np.array([1.0, 0.5, 3.0])
    out = lp.covariance(lp.cov_rows(mats), scale)
    assert (out["status"] == 0).all()
    for k, A in enumerate(mats):
        err = np.abs(out["cov"][k] @ A / scale[k] - np.eye(p)).max()
        assert err <= 1e-10, (p, k, err)
        assert np.array_equal(out["std_err"][k], np.sqrt(np.diag(out["cov"][k]))) and 0.0 < out["pivot_ratio"][k] <= 1.0
    assert np.array_equal(lp.covariance(lp.cov_rows(mats))["cov"][0], out["cov"][0])             # (scale None is 1)


def test_covariance_restatement_edges():
    perm = np.array([[0.0, 2.0, 0.0], [0.0, 0.0, 4.0], [5.0, 0.0, 0.0]])                         # needs a row exchange at every step
    out = lp.covariance(lp.cov_rows([perm, np.ones((3, 3)), np.array([[1.0, 0.0, 0.0], [0.0, np.nan, 0.0], [0.0, 0.0, 1.0]]), np.diag([1.0, 2.0, 4.0])]))
    assert out["status"].tolist() == [0, 1, 1, 0]
    assert np.array_equal(out["cov"][0], [[0.0, 0.0, 0.2], [0.5, 0.0, 0.0], [0.0, 0.25, 0.0]]) and out["pivot_ratio"][0] == 2.0 / 5.0
    assert np.array_equal(out["std_err"][0], [0.0, 0.0, 0.0])                                    # (a diagonal of zeros)
    for k in (1, 2):
        assert np.isnan(out["cov"][k]).all() and np.isnan(out["std_err"][k]).all() and out["pivot_ratio"][k] == 0.0
    assert np.array_equal(out["cov"][3], np.diag([1.0, 0.5, 0.25])) and out["pivot_ratio"][3] == 0.25 and np.array_equal(out["std_err"][3], [1.0, np.sqrt(0.5), 0.5])
    neg = lp.covariance(lp.cov_rows([np.diag([1.0, -4.0])]))                                        # a negative diagonal of the inverse: std_err NaN there, status still 0
    assert neg["status"][0] == 0 and neg["std_err"][0, 0] == 1.0 and np.isnan(neg["std_err"][0, 1])
    assert lp.covariance(lp.cov_rows([np.eye(2)]), np.array([np.inf]))["status"][0] == 1            # (a non-finite entry of the result)


# ---- count_observed ---------------------------------------------------------------------------------------------------------------------------------------------------------
COUNT_CASES = ["plain", "skip_missing", "zero weights", "ini_state given", "estimate_ini"]


@pytest.mark.parametrize("case", COUNT_CASES)
def test_count_observed_against_the_residual_vector(case):
    """the entries that enter the loss = the nonzero entries of the oracle's weighted residual vector on generic data (noise on the recorded states, a perturbed theta)"""
    import torch
    from pdp_amd import runtime as rt
    from pdp_amd.irl import _first_row
    sid = sg.oracle("cartpole")
    inputs, states, _, theta = sg.stored("cartpole")
    rng = np.random.default_rng(8)
    states = states + 0.01 * rng.standard_normal(states.shape)
    B, R, n = states.shape
    weights, ini, idx, skip = None, None, [], False
    if case == "skip_missing":
        states, ini, skip = sg.observe(states, every=3, components=[0, 2]), states[:, 0] + 0.1, True
        states[:, 0, 1] = 0.3                                                     # (an observed entry of row 0, next to the NaN ones)
    if case == "zero weights":
        weights = rng.uniform(0.5, 2.0, (R, n))
        weights[::2, 1], weights[5] = 0.0, 0.0
    if case == "ini_state given":
        ini = states[:, 0] + 0.1
    if case == "estimate_ini":
        idx = [1, 3]
    want = []
    for b in range(B):
        x0 = (states[b, 0] if ini is None else ini[b]).copy()
        x0[idx] += 0.05                                                           # (the estimated components at a generic point)
        d = sid.integrateDyn(x0, inputs[b], 0.9 * theta) - states[b]
        if skip:
            d = np.where(np.isnan(states[b]), 0.0, d)
        if weights is not None:
            d = np.sqrt(weights) * d
        want.append(int((d != 0.0).sum()))
    got = rt.count_observed(torch.as_tensor(states), weights, skip, _first_row(ini, idx, n))
    print(case, want, got.tolist())
    assert got.tolist() == want and got.dtype == torch.int64
    assert (want[0] < R * n) == (case != "ini_state given")                        # (every other case leaves something out: row 0 at the least)


# ---- the Python layer, on the paths that need no device --------------------------------------------------------------------------------------------------------------------
def test_keyword_validation_needs_no_device():
    from pdp_amd.irl import BatchedLMLoop, LMLoop, check_prior
    from pdp_amd import runtime as rt
    ev = lambda theta: (0.0, np.zeros(3), np.eye(3))
    ok = dict(prior_mean=np.zeros(3), prior_precision=np.eye(3))
    for bad, match in ((dict(prior_mean=None), "go together"), (dict(prior_precision=None), "go together"), (dict(prior_mean=np.zeros(2)), "prior_mean"),
                       (dict(prior_precision=np.eye(4)), "prior_precision"), (dict(prior_precision=np.array([1.0, np.nan, 1.0])), "non-finite"),
                       (dict(prior_mean=np.array([0.0, np.inf, 0.0])), "non-finite"), (dict(prior_precision=np.array([1.0, -1.0, 1.0])), "negative"),
                       (dict(prior_precision=np.diag([1.0, -2.0, 1.0])), "negative"), (dict(prior_precision=np.array([[1.0, 0.5, 0], [0.4, 1, 0], [0, 0, 1.0]])), "symmetric")):
        with pytest.raises(ValueError, match=match):
            LMLoop(ev, np.zeros(3), **dict(ok, **bad))
        with pytest.raises(ValueError, match=match):                              # (before the device is asked for)
            BatchedLMLoop(lambda trial: None, np.zeros((5, 3)), **dict(ok, **bad))
    # per-problem shapes are the batched loop's alone
    with pytest.raises(ValueError, match="prior_precision"):
        LMLoop(ev, np.zeros(3), prior_mean=np.zeros(3), prior_precision=np.ones((5, 3)))
    with pytest.raises(ValueError, match="prior_precision"):
        BatchedLMLoop(lambda trial: None, np.zeros((5, 3)), prior_mean=np.zeros(3), prior_precision=np.ones((4, 3)))
    assert check_prior("x", None, None, 3) == (None, None)
    for K, p, ms, ps, want in ((5, 3, (3,), (3,), (0, 0, 0)), (5, 3, (5, 3), (5, 3), (0, 3, 3)), (5, 3, (3,), (3, 3), (1, 0, 0)), (5, 3, (5, 3), (5, 3, 3), (1, 3, 9)),
                               (3, 3, (3,), (3, 3), (1, 0, 0))):
        assert rt.lm_prior_shapes(ms, ps, K, p) == want
    loop = LMLoop(ev, np.zeros(3))
    loop.start()
    with pytest.raises(ValueError, match="noise"):
        loop.covariance("guessed")
    c = LMLoop(lambda theta: (1.0, np.zeros(2), np.ones((2, 2))), np.zeros(2))
    c.start()
    out = c.covariance("known")
    assert out["status"] == 1 and np.isnan(out["cov"]).all() and out["pivot_ratio"] == 0.0


def test_layout_is_explicit_where_the_number_of_problems_equals_the_number_of_unknowns():
    """K == p: the shape [p, p] is a shared full matrix or one diagonal per problem - refused without prior_kind, taken as said with it; the prior of
    for_sysid(estimate_ini=, prior_ini_precision=) names its layout itself (K == W = p + q included)"""
    from pdp_amd.irl import BatchedLMLoop, check_prior, prior_layout, _prior_with_ini
    with pytest.raises(ValueError, match="prior_kind"):
        BatchedLMLoop(lambda trial: None, np.zeros((3, 3)), prior_mean=np.zeros(3), prior_precision=np.ones((3, 3)))
    with pytest.raises(ValueError, match="prior_kind"):
        check_prior("x", np.zeros(3), np.eye(3), 3, 3)
    assert prior_layout("x", (3,), (3, 3), 3, 3, "diagonal") == 0 and prior_layout("x", (3,), (3, 3), 3, 3, "full") == 1
    assert prior_layout("x", (3,), (3, 3), 3, 5) == 1 and prior_layout("x", (3,), (5, 3), 3, 5) == 0 and prior_layout("x", (3,), (3, 3), 3) == 1
    for shape, kind in (((3,), "full"), ((3, 3, 3), "diagonal"), ((5, 3), "full")):
        with pytest.raises(ValueError, match="precision"):
            prior_layout("x", (3,), shape, 3, 5 if shape == (5, 3) else 3, kind)
    with pytest.raises(ValueError, match="prior_kind"):
        prior_layout("x", (3,), (3,), 3, 3, "dense")
    # a per-problem diagonal with asymmetric rows passes as a diagonal and is refused as a full matrix
    rows = np.arange(1.0, 10.0).reshape(3, 3)
    assert check_prior("x", np.zeros(3), rows, 3, 3, "diagonal")[1].shape == (3, 3)
    with pytest.raises(ValueError, match="symmetric"):
        check_prior("x", np.zeros(3), rows, 3, 3, "full")
    # K == W = 6: p = 4, q = 2
    start = np.arange(12.0).reshape(6, 2)
    for theta_part, want in (((None, None), "diagonal"), ((np.zeros(4), np.ones(4)), "diagonal"), ((np.zeros(4), np.eye(4)), "full")):
        mean, prec, kind = _prior_with_ini("x", theta_part[0], theta_part[1], [1.0, 2.0], 4, 2, start, K=6)
        assert kind == want and mean.shape == (6, 6) and prec.shape == ((6, 6) if want == "diagonal" else (6, 6, 6))
        assert np.array_equal(mean[:, 4:], start) and check_prior("x", mean, prec, 6, 6, kind)[1] is not None
        if want == "diagonal":
            assert np.array_equal(prec[:, 4:], np.tile([1.0, 2.0], (6, 1))) and prior_layout("x", mean.shape, prec.shape, 6, 6, kind) == 0
            with pytest.raises(ValueError, match="prior_kind"):      # (what reading the shape alone would have had to guess)
                check_prior("x", mean, prec, 6, 6)


def test_host_covariance_follows_the_rules_of_the_device():
    """irl.LMLoop.covariance against the restatement of the covariance kernel: bit-equal inverse and pivot ratio on seeded matrices, and the same status on a matrix
    that is singular up to rounding (LAPACK inverts it to huge finite numbers) and on an exactly singular one"""
    from pdp_amd.irl import LMLoop, inverse_pivoted
    for p in (1, 5, 13):
        A = lp.spd(p, 3)
        loop = LMLoop(lambda theta, A=A: (2.0, np.zeros(len(A)), A), np.zeros(p))
        loop.start()
        got, ref = loop.covariance("known"), lp.covariance(lp.cov_rows([A]))
        assert got["status"] == 0 and got["pivot_ratio"] == ref["pivot_ratio"][0]
        assert np.array_equal(got["cov"], 0.5 * (ref["cov"][0] + ref["cov"][0].T))
    near = np.ones((3, 3)) + 1e-17 * np.arange(9.0).reshape(3, 3)                 # (rounds to ones((3, 3)): exactly singular in fp64)
    tiny = np.ones((3, 3)) + np.diag([0.0, 2e-16, 4e-16])                         # singular up to rounding: pivots of 1e-16
    for A in (near, tiny, np.ones((2, 2))):
        loop = LMLoop(lambda theta, A=A: (2.0, np.zeros(len(A)), A), np.zeros(len(A)))
        loop.start()
        got, ref = loop.covariance("known"), lp.covariance(lp.cov_rows([A]))
        assert got["status"] == ref["status"][0] and got["pivot_ratio"] == ref["pivot_ratio"][0], A
        assert np.array_equal(np.isnan(got["cov"]), np.isnan(ref["cov"][0]))
    inv, ok, ratio = inverse_pivoted(tiny)
    print("singular up to rounding: ok %s pivot_ratio %.1e (the diagnosis; the elimination's threshold is 1e-300, as on the device)" % (ok, ratio))
    assert ratio <= 1e-15
