"""Shared by tests/test_cp_jvp_host.py (CPU) and tests/test_gpu_cp_jvp.py (GPU): the tangent of a ControlPlanning rollout (x_0 .. x_T, u_0 .. u_{T-1}) along a
direction (d_theta, d_x0) of the policy's parameters and the initial state (cp_jvp_kernel, pdp_policy_tan, ModelLib.cp_rollout_jvp,
ControlPlanning.rollout_jvp_batch, forward mode through pdp_amd.autograd.cp_trajectory, irl.MatrixFreeLM.for_cp).

Reference - not the kernel's method: cp_vjp_common.forward_sensitivities - ControlPlanningOracle.getAuxSys at the oracle's own rollout, then its integrateAuxSys from
X_0 = [0 | I] with n zero columns appended to dUe - contracted with the direction: d_state = X [d_theta; d_x0], d_control = U [d_theta; d_x0].  `tangent_sweep`
restates the kernel's recursion in numpy on the same matrices; tests/test_cp_jvp_host.py holds it to the reference at cp_vjp_common.HOST_TOL on every case listed here.

Models, inputs and parameter blocks are those of tests/cp_edge_common.py (C16, C15, C5; B = 5; one shared theta and one per sample); the tangents are
default_rng(SEED + 1000 n + T) standard normals (d_theta [p], then d_theta_b [B, p], then d_x0 [B, n]).  Chunk edges follow ROWS, the pool rows of the sweep by the rule
of csrc/pdp_sweep_pool.h worked out by hand: stride = (PATH_NVAR + n + m) | 1 with PATH_NVAR = 28, 26, 10 variable entries of the `path` group -> 49, 45, 17 ->
2400 // stride = 48, 53, 141 -> clamped to [4, 64]."""
import functools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import cp_edge_common as ce  # noqa: E402
import cp_vjp_common as cv  # noqa: E402

ROWS = {"C16": 48, "C15": 53, "C5": 64}
ZOO_ROWS = {"cartpole": 64, "pendulum": 64, "quadrotor": 30, "robotarm": 64, "rocket": 29}      # strides 17, 7, 79, 23, 81
TOL = ce.TOL                  # 1e-10 of the largest entry of d_state and of d_control, per sample
HOST_TOL = cv.HOST_TOL        # the numpy recursion against the reference
FD_TOL = cv.FD_TOL            # the reference against central differences
SEED = 8000
BUDGET = os.path.join(ROOT, "tests", "golden", "cp_jvp_lm_budget.json")


def tuned_cases():
    """[(model, kind, key, T)] of the tuned kernel against the reference: cp_vjp_common's cases with the chunk edges by ROWS"""
    out = [(name, "poly", cv.EDGE_PIVOTS, cv.edge_T(ROWS[name], e)) for name in ce.NAMES for e in cv.EDGES]
    out += [(name, "poly", N, cv.PIVOT_T) for name, N in cv.PIVOT_CASES]
    out += [(name, "mlp", layers, T) for (name, layers) in cv.NETS for T in cv.MLP_HORIZONS]
    return out


case_id = cv.case_id


def tangents(name, kind, key, T, B=ce.B_UNIT):
    """dict(d_theta [p], d_theta_b [B, p], d_x0 [B, n])"""
    n, _ = ce.MODELS[name]
    p = ce.n_params(name, kind, key)
    rng = np.random.default_rng(SEED + 1000 * n + T)
    return dict(d_theta=rng.standard_normal(p), d_theta_b=rng.standard_normal((B, p)), d_x0=rng.standard_normal((B, n)))


def d_theta_of(tan, per_sample, b):
    return tan["d_theta_b"][b] if per_sample else tan["d_theta"]


def contract(X, U, d_theta=None, d_x0=None):
    """(d_state [T+1, n], d_control [T, m]) of the sensitivities (X [T+1, n, p + n], U [T, m, p + n]) along the direction; None = zero"""
    n = X.shape[1]
    p = X.shape[2] - n
    v = np.concatenate([np.zeros(p) if d_theta is None else np.asarray(d_theta, float), np.zeros(n) if d_x0 is None else np.asarray(d_x0, float)])
    return X @ v, U @ v


def reference_at(orc, x0, T, theta):
    """dict(x, u, X [T+1, n, p + n], U [T, m, p + n], aux) of one trajectory"""
    sol = orc.integrateSys(x0, T, theta)
    X, U, aux = cv.forward_sensitivities(orc, sol["state_traj"], sol["control_traj"], theta)
    return dict(x=np.asarray(sol["state_traj"], float), u=np.asarray(sol["control_traj"], float).reshape(T, orc.m), X=X, U=U, aux=aux)


@functools.lru_cache(maxsize=None)
def reference(name, kind, key, T, per_sample, b):
    """the sensitivities on sample b of cp_edge_common.inputs - once per process, not modified; contract() gives the tangents along any direction"""
    inp = ce.inputs(name, kind, key, T)
    return reference_at(cv.oracle_for(name, kind, key, T), inp["x0"][b], T, ce.theta_of(inp, per_sample, b))


def tangent_sweep(aux, d_theta=None, d_x0=None):
    """(d_state [T+1, n], d_control [T, m]) by the kernel's recursion on the oracle's matrices:
    dx_0 = d_x0;  du_t = (d pi/dx) dx_t + (d pi/d theta) d_theta;  dx_{t+1} = F_t dx_t + G_t du_t"""
    T = len(aux["dynF"])
    n, m = np.asarray(aux["dynG"][0]).shape
    dx = np.zeros(n) if d_x0 is None else np.array(d_x0, float)
    ds, dc = [dx], []
    for t in range(T):
        du = np.asarray(aux["dUx"][t], float).reshape(m, n) @ dx
        if d_theta is not None:
            du = du + np.asarray(aux["dUe"][t], float).reshape(m, -1) @ d_theta
        dx = np.asarray(aux["dynF"][t], float) @ dx + np.asarray(aux["dynG"][t], float).reshape(n, m) @ du
        ds.append(dx), dc.append(du)
    return np.stack(ds), np.stack(dc)


def rel(got, want):
    """max|got - want| / max|want|; a block the reference has as exact zeros must be exact zeros"""
    got, want = np.asarray(got, float), np.asarray(want, float)
    if np.abs(want).max() == 0:
        return 0.0 if np.abs(got).max() == 0 else float("inf")
    return float(np.abs(got - want).max() / np.abs(want).max())


# ---- the least-squares problem of the MatrixFreeLM.for_cp tests ------------------------------------------------------------------------------------------------
LM = dict(name="C15", pivots=6, T=12)           # p = 18: beyond any fused Gauss-Newton row


@functools.lru_cache(maxsize=None)
def lm_problem(seed=3):
    """C15 under 6 pivots, T = 12, B = 5: the targets are the oracle's rollouts at cp_edge_common.inputs' theta (reachable: the floor is rounding), the residual the
    states alone, the start theta* + 0.2 max|theta*| N(0, 1): dict(orc, x0, T, theta_true, theta0, target [B, T+1, n])"""
    name, N, T = LM["name"], LM["pivots"], LM["T"]
    orc, inp = cv.oracle_for(name, "poly", N, T), ce.inputs(name, "poly", N, T)
    th = inp["theta"]
    target = np.stack([np.asarray(orc.integrateSys(x0, T, th)["state_traj"], float) for x0 in inp["x0"]])
    theta0 = th + 0.2 * np.abs(th).max() * np.random.default_rng(seed).standard_normal(len(th))
    return dict(orc=orc, x0=inp["x0"], T=T, theta_true=th, theta0=theta0, target=target)


def lm_restatement(P, lam0=1e-3, up=10.0, down=10.0, lam_min=1e-12, lam_max=1e8, cg_tol=1e-8, cg_max=None, max_evals=30, loss_tol=1e-20):
    """MatrixFreeLM's schedule in numpy on the oracle: loss = sum r^2 / B with r = states - target, the dense J from the oracle's forward sensitivities (explicit here,
    products only in the loop under test), plain lam I, (G + lam I) s = J'r / B by conjugate gradients from 0 to a relative residual cg_tol, lam / 10 on an accepted
    step and x 10 on a rejected one, accept iff the loss is strictly lower.  The products are einsum's own loops: the counts do not depend on a BLAS.
    -> dict(loss_trace, evaluations, cg_iterations, rejected, theta)"""
    orc, x0, T, target = P["orc"], P["x0"], P["T"], P["target"]
    B, p = len(x0), orc.n_auxvar
    cg_max = 2 * p if cg_max is None else cg_max

    def evaluate(theta):
        r, J = [], []
        for b in range(B):
            ref = reference_at(orc, x0[b], T, theta)
            J.append(ref["X"][:, :, :p].reshape(-1, p))
            r.append((ref["x"] - target[b]).reshape(-1))
        r, J = np.concatenate(r), np.concatenate(J)
        return float(np.einsum("i,i->", r, r)) / B, np.einsum("ik,i->k", J, r) / B, J

    out = dict(evaluations=1, cg_iterations=0, rejected=0)
    theta, lam = P["theta0"].copy(), lam0
    loss, g, J = evaluate(theta)
    trace = [loss]
    dot = lambda a, b: float(np.einsum("i,i->", a, b))
    while out["evaluations"] < max_evals and loss > loss_tol and lam <= lam_max:
        s, r = np.zeros(p), g.copy()
        d, rr = r.copy(), dot(r, r)
        stop = cg_tol ** 2 * rr
        for _ in range(cg_max):
            if not rr > stop:
                break
            q = np.einsum("ik,i->k", J, np.einsum("ik,k->i", J, d)) / B + lam * d
            dq = dot(d, q)
            out["cg_iterations"] += 1
            if not dq > 0.0:
                break
            a = rr / dq
            s, r = s + a * d, r - a * q
            rr_new = dot(r, r)
            d, rr = r + (rr_new / rr) * d, rr_new
        trial = evaluate(theta - s)
        out["evaluations"] += 1
        if np.isfinite(trial[0]) and trial[0] < loss:
            theta, (loss, g, J), lam = theta - s, trial, max(lam / down, lam_min)
            trace.append(loss)
        else:
            out["rejected"], lam = out["rejected"] + 1, lam * up
    return dict(out, loss_trace=np.array(trace), theta=theta)


def budget():
    with open(BUDGET) as f:
        return json.load(f)
