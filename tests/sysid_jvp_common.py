"""Shared by tests/test_sysid_jvp_host.py and tests/test_gpu_sysid_jvp.py: the CPU reference of the SysID rollout's Jacobian-vector product
(pdp_sysid_rollout_jvp_batched, include/pdp_hip_sysid_jvp.h) and the cases the tests run on - those of tests/sysid_vjp_u_common.py (case, user_case) with a direction
(d_theta shared and per sample, d_x0, d_u) added.

The reference is NOT the kernel's method: the kernel sweeps ONE tangent vector forwards with the forcing term E_t d_theta + G_t d_u_t; the reference materialises the
sensitivities - X_t = dx_t/dtheta and Phi_t = dx_t/dx_0 from two integrateAuxSys runs of SysIDOracle (as sysid_vjp_common.reference does), D_{t,s} = dx_t/du_s
propagated from sympy's G_s (as sysid_vjp_u_common.reference_u does) - and contracts them with the direction:
    d_x[t] = X_t d_theta + Phi_t d_x0 + sum_{s < t} D_{t,s} d_u[s].
tangent_sweep is the kernel's recursion in numpy, kept to state how far the two methods agree on the CPU."""
import numpy as np

import sysid_vjp_common as sv
import sysid_vjp_u_common as su

ROOT, SYSTEMS, TOL, EDGE_T = su.ROOT, su.SYSTEMS, su.TOL, su.EDGE_T
rel_rows = su.rel_rows
_cases = {}


def sens(name, orc, x0, inputs, theta):
    """dict(states [B,T+1,n], X [B,T+1,n,p], Phi [B,T+1,n,n], D [B,T+1,n,T,m]) of the rollouts from x0 [B,n] under inputs [B,T,m]; theta [p] or [B,p]"""
    G = su.g_fn(name)
    inputs, theta = np.asarray(inputs, float), np.asarray(theta, float)
    B, T, m = inputs.shape
    n = orc.n
    xs_, X_, P_, D_ = [], [], [], []
    for b in range(B):
        th = theta[b] if theta.ndim == 2 else theta
        xs = np.asarray(orc.integrateDyn(x0[b], inputs[b], th), float)
        aux = orc.getAuxSys(xs, inputs[b], th)
        X = np.stack(orc.integrateAuxSys(aux["dynF"], aux["dynE"], np.zeros((n, orc.p)))["state_traj"])
        Phi = np.stack(orc.integrateAuxSys(aux["dynF"], [np.zeros((n, n))] * T, np.eye(n))["state_traj"])
        D = np.zeros((T + 1, n, T, m))
        for s in range(T):
            d = G(xs[s], inputs[b, s], th)                       # dx_{s+1}/du_s
            for t in range(s + 1, T + 1):
                D[t, :, s, :] = d
                if t < T:
                    d = aux["dynF"][t] @ d
        xs_.append(xs), X_.append(X), P_.append(Phi), D_.append(D)
    return dict(states=np.array(xs_), X=np.array(X_), Phi=np.array(P_), D=np.array(D_))


def tangent(S, d_theta=None, d_x0=None, d_u=None, T=None):
    """d_x [B,T+1,n] of the sensitivities S = sens(..) along the direction; None = zero; T: the first T steps only (the sensitivities of a prefix are a prefix)"""
    T = S["states"].shape[1] - 1 if T is None else T
    out = np.zeros(S["states"][:, :T + 1].shape)
    if d_theta is not None:
        d_theta = np.asarray(d_theta, float)
        out += np.einsum("btip,bp->bti" if d_theta.ndim == 2 else "btip,p->bti", S["X"][:, :T + 1], d_theta)
    if d_x0 is not None:
        out += np.einsum("btij,bj->bti", S["Phi"][:, :T + 1], d_x0)
    if d_u is not None:
        out += np.einsum("btisj,bsj->bti", S["D"][:, :T + 1, :, :T], np.asarray(d_u, float)[:, :T])
    return out


def tangent_sweep(name, orc, xs, inputs, theta, d_theta=None, d_x0=None, d_u=None):
    """the kernel's recursion for ONE trajectory in numpy: d_x [T+1, n]"""
    G = su.g_fn(name)
    aux = orc.getAuxSys(xs, inputs, theta)
    T = len(inputs)
    out = np.zeros((T + 1, orc.n))
    if d_x0 is not None:
        out[0] = d_x0
    for t in range(T):
        w = np.zeros(orc.n)
        if d_theta is not None:
            w = w + aux["dynE"][t] @ d_theta
        if d_u is not None:
            w = w + G(xs[t], inputs[t], theta) @ d_u[t]
        out[t + 1] = w + aux["dynF"][t] @ out[t]
    return out


def _direction(c, p, seed):
    rng = np.random.default_rng(seed)
    B, T, m = c["inputs"].shape
    n = c["x0"].shape[1]
    c["d_theta"], c["d_theta_b"] = rng.standard_normal(p), rng.standard_normal((B, p))
    c["d_x0"], c["d_u"] = rng.standard_normal((B, n)), rng.standard_normal((B, T, m))


def case(system, T=None, seed=7):
    """sysid_vjp_u_common.case with a direction (d_theta [p], d_theta_b [B,p], d_x0 [B,n], d_u [B,T,m], N(0,1)) and the sensitivities S (shared theta) and S_b
    (per-sample theta) for tangent().  Computed once and shared: do not write into it."""
    key = ("zoo", system, T, seed)
    if key not in _cases:
        c = dict(su.case(system, T, seed), name=system)
        _direction(c, c["sid"].p, seed + 100)
        c["S"] = sens(system, c["sid"], c["x0"], c["inputs"], c["theta"])
        c["S_b"] = sens(system, c["sid"], c["x0"], c["inputs"], c["theta_b"])
        assert np.abs(c["S"]["states"] - c["states"]).max() == 0.0
        _cases[key] = c
    return _cases[key]


def user_case(name, seed=5, B=3, T=10):
    """sysid_vjp_u_common.user_case with a direction and the sensitivities S of the shared theta"""
    key = ("user", name, seed, B, T)
    if key not in _cases:
        c = dict(su.user_case(name, seed=seed, B=B, T=T))
        _direction(c, c["orc"].p, seed + 100)
        c["S"] = sens(name, c["orc"], c["x0"], c["inputs"], c["theta"])
        _cases[key] = c
    return _cases[key]


def lm_problem(seed=3, B=16, T=20):
    """the least-squares problem of the MatrixFreeLM tests on linear_9_2_99: noise-free rollouts of the oracle at theta_true under inputs N(0,1) from x0 = 0.3 N(0,1),
    start theta0 = theta_true + 0.1 N(0,1): dict(orc, sid, x0, inputs, states, theta_true, theta0)"""
    key = ("lm", seed, B, T)
    if key not in _cases:
        sid, orc = sv.user_pair("linear_9_2_99")
        rng = np.random.default_rng(seed)
        theta_true = 0.5 * rng.standard_normal(orc.p)
        x0, inputs = 0.3 * rng.standard_normal((B, orc.n)), rng.standard_normal((B, T, orc.m))
        states = np.array([orc.integrateDyn(x0[b], inputs[b], theta_true) for b in range(B)], float)
        _cases[key] = dict(sid=sid, orc=orc, x0=x0, inputs=inputs, states=states, theta_true=theta_true, theta0=theta_true + 0.1 * rng.standard_normal(orc.p))
    return _cases[key]


def lm_restatement(P, lam0=1e-3, up=10.0, down=10.0, lam_min=1e-12, lam_max=1e8, cg_tol=1e-8, cg_max=None, max_evals=30, loss_tol=1e-16):
    """MatrixFreeLM's schedule in numpy on the oracle: loss = sum r^2 / B with r = rollout - recorded, J from the oracle's sensitivities X (explicit here, products only
    in the loop under test), (G + lam I) s = J'r / B by conjugate gradients from 0 to a relative residual cg_tol, accept iff the loss is strictly lower.
    -> dict(loss_trace, evaluations, cg_iterations, rejected, theta)"""
    orc, x0, u, obs = P["orc"], P["x0"], P["inputs"], P["states"]
    B, p = len(x0), orc.p
    cg_max = 2 * p if cg_max is None else cg_max

    def evaluate(theta):
        r, J = [], []
        for b in range(B):
            xs = np.asarray(orc.integrateDyn(x0[b], u[b], theta), float)
            aux = orc.getAuxSys(xs, u[b], theta)
            J.append(np.stack(orc.integrateAuxSys(aux["dynF"], aux["dynE"], np.zeros((orc.n, p)))["state_traj"]).reshape(-1, p))
            r.append((xs - obs[b]).reshape(-1))
        r, J = np.concatenate(r), np.concatenate(J)
        return float(r @ r) / B, J.T @ r / B, J

    out = dict(evaluations=1, cg_iterations=0, rejected=0)
    theta, lam = P["theta0"].copy(), lam0
    loss, g, J = evaluate(theta)
    trace = [loss]
    while out["evaluations"] < max_evals and loss > loss_tol and lam <= lam_max:
        s, r = np.zeros(p), g.copy()
        d, rr = r.copy(), float(r @ r)
        stop = cg_tol ** 2 * rr
        for _ in range(cg_max):
            if not rr > stop:
                break
            q = J.T @ (J @ d) / B + lam * d
            dq = float(d @ q)
            out["cg_iterations"] += 1
            if not dq > 0.0:
                break
            a = rr / dq
            s, r = s + a * d, r - a * q
            rr_new = float(r @ r)
            d, rr = r + (rr_new / rr) * d, rr_new
        trial = evaluate(theta - s)
        out["evaluations"] += 1
        if np.isfinite(trial[0]) and trial[0] < loss:
            theta, (loss, g, J), lam = theta - s, trial, max(lam / down, lam_min)
            trace.append(loss)
        else:
            out["rejected"], lam = out["rejected"] + 1, lam * up
    return dict(out, loss_trace=np.array(trace), theta=theta)
