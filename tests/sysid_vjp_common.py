"""Shared by tests/test_sysid_vjp_host.py and tests/test_gpu_sysid_vjp.py: the CPU reference of the SysID rollout's vector-Jacobian product
(pdp_sysid_rollout_vjp_batched, include/pdp_hip_sysid_vjp.h) and the inputs the tests run on.

The reference is NOT the kernel's method: the kernel sweeps a costate backwards, the reference propagates FORWARD sensitivities with SysIDOracle -
X_t = dx_t/dtheta from integrateAuxSys(F, E, 0) and Phi_t = dx_t/dx_0 from integrateAuxSys(F, 0, I) (a zero E of n columns) - and contracts them with the cotangents:
grad_theta = sum_t g_t' X_t, grad_x0 = sum_t g_t' Phi_t.  adjoint_sweep is the kernel's recursion in numpy, kept to state how far the two methods agree on the CPU
(<= 4e-15 relative on all five systems at the horizons of the chunk-edge tests, tests/test_sysid_vjp_host.py)."""
import numpy as np

import sysid_gn_common as sg

ROOT, SYSTEMS, TOL = sg.ROOT, sg.SYSTEMS, sg.TOL
oracle, stored, rel_rows = sg.oracle, sg.stored, sg.rel_rows
_cases = {}


def reference(sid, x0, inputs, theta, g):
    """(states [B,T+1,n], grad_theta [B,p], grad_x0 [B,n]) by forward sensitivities; theta [p] or [B,p], g [B,T+1,n] the cotangents"""
    inputs, g, theta = np.asarray(inputs, float), np.asarray(g, float), np.asarray(theta, float)
    xs_, gt, g0 = [], [], []
    for b in range(inputs.shape[0]):
        th = theta[b] if theta.ndim == 2 else theta
        xs = sid.integrateDyn(x0[b], inputs[b], th)
        aux = sid.getAuxSys(xs, inputs[b], th)
        X = np.stack(sid.integrateAuxSys(aux["dynF"], aux["dynE"], np.zeros((sid.n, sid.p)))["state_traj"])                        # [T+1, n, p]
        Phi = np.stack(sid.integrateAuxSys(aux["dynF"], [np.zeros((sid.n, sid.n))] * len(aux["dynF"]), np.eye(sid.n))["state_traj"])     # [T+1, n, n]
        xs_.append(xs)
        gt.append(np.einsum("ti,tip->p", g[b], X))
        g0.append(np.einsum("ti,tij->j", g[b], Phi))
    return np.array(xs_), np.array(gt), np.array(g0)


def adjoint_sweep(sid, xs, inputs, theta, g):
    """the kernel's recursion for ONE trajectory in numpy: (grad_theta [p], grad_x0 [n])"""
    aux = sid.getAuxSys(xs, inputs, theta)
    lam, gt = np.array(g[-1], float), np.zeros(sid.p)
    for t in range(len(inputs) - 1, -1, -1):
        gt += aux["dynE"][t].T @ lam
        lam = g[t] + aux["dynF"][t].T @ lam
    return gt, lam


def case(system, T=None, seed=7):
    """dict(sid, x0 [B,n], inputs [B,T,m], theta [p], theta_b [B,p], g [B,T+1,n], and the reference for both thetas: states, grad_theta, grad_x0, states_b,
    grad_theta_b, grad_x0_b).  T None: the stored inputs and initial states (T = 10 or 20) at the stored run's parameter; else up to 3 rollouts of horizon T under
    u = std(stored inputs) N(0,1) from the stored initial states.  Cotangents N(0,1).  Computed once and shared: do not write into it."""
    key = (system, T, seed)
    if key not in _cases:
        sid = oracle(system)
        inputs, states, _, theta = stored(system)
        rng = np.random.default_rng(seed)
        x0 = states[:, 0].copy()
        if T is not None:
            B = min(3, x0.shape[0])                              # (the rocket has two stored recordings)
            x0, inputs = x0[:B], inputs.std() * rng.standard_normal((B, T, sid.m))
        g = rng.standard_normal((inputs.shape[0], inputs.shape[1] + 1, sid.n))
        theta_b = theta * (1.0 + 0.05 * rng.standard_normal((inputs.shape[0], sid.p)))
        c = dict(sid=sid, x0=x0, inputs=inputs, theta=theta, theta_b=theta_b, g=g)
        c["states"], c["grad_theta"], c["grad_x0"] = reference(sid, x0, inputs, theta, g)
        c["states_b"], c["grad_theta_b"], c["grad_x0_b"] = reference(sid, x0, inputs, theta_b, g)
        assert np.isfinite(c["states"]).all() and np.isfinite(c["states_b"]).all(), (system, T)
        _cases[key] = c
    return _cases[key]


# the horizons of the chunk-edge tests: 2 R + 1 with R = 32 pool rows for the two small systems, R + 1 for the large ones
EDGE_T = {"pendulum": 65, "cartpole": 65, "robotarm": 33, "rocket": 33, "quadrotor": 33}


def linear_9_2_99(lib, dt=0.05):
    """x+ = x + dt (A x + B u) with theta = (vec A, vec B), row-major: (n, m, p) = (9, 2, 99) - parameters in a second 64-lane slot of the kernel"""
    n, m = 9, 2
    xs, us, a, b = sg._symbols(lib, (("x", n), ("u", m), ("a", n * n), ("b", n * m)))
    f = []
    for i in range(n):
        acc = a[i * n] * xs[0]
        for j in range(1, n):
            acc = acc + a[i * n + j] * xs[j]
        for j in range(m):
            acc = acc + b[i * m + j] * us[j]
        f.append(xs[i] + dt * acc)
    return xs, us, a + b, f


def chain_40_10_3(lib, dt=0.05):
    """the 40-state chain of tests/test_gpu_generic_sizes.py, restated: 20 masses, 10 actuators; stiffness, damping and a cubic coefficient are the unknowns"""
    nm, m = 20, 10
    qs, vs, us, ws = sg._symbols(lib, (("q", nm), ("v", nm), ("u", m), ("w", 3)))
    f = [qs[i] + dt * vs[i] for i in range(nm)]
    for i in range(nm):
        left = qs[i - 1] if i > 0 else 0.0
        right = qs[i + 1] if i + 1 < nm else 0.0
        a = ws[0] * (left - 2 * qs[i] + right) - ws[1] * vs[i] - ws[2] * qs[i] * qs[i] * qs[i]
        if i % 2 == 0:
            a = a + us[i // 2]
        f.append(vs[i] + dt * a)
    return qs + vs, us, ws, f


def user_model(builder, label):
    """(PDP.SysID, SysIDOracle) of the same equations, once in pdp_amd.sx and once in sympy"""
    import sympy as sp
    from oracle import pdp_oracle as po
    from pdp_amd import PDP
    from pdp_amd.sx import vertcat
    X, U, w, f = builder("sx")
    sid = PDP.SysID(label)
    sid.setAuxvarVariable(vertcat(*w))
    sid.setStateVariable(vertcat(*X))
    sid.setControlVariable(vertcat(*U))
    sid.setDyn(vertcat(*f))
    Xs, Us, ws, fs = builder("sympy")
    return sid, po.SysIDOracle(sp.Matrix(Xs), sp.Matrix(Us), list(ws), sp.Matrix(fs))


USER_MODELS = {"chain_40_10_3": (chain_40_10_3, "chain sysid 40"), "linear_9_2_99": (linear_9_2_99, "linear sysid 9 2 99")}


def user_case(name, seed=5, B=3, T=10):
    """the inputs of the size tests (T = 10, B = 3) for USER_MODELS[name]: dict(sid (PDP.SysID), orc, x0, inputs, theta, g, and the oracle's reference)"""
    key = ("user", name, seed)
    if key not in _cases:
        sid, orc = user_model(*USER_MODELS[name])
        rng = np.random.default_rng(seed)
        if name == "chain_40_10_3":
            theta = np.array([1.7, 0.5, 0.2])
        else:
            theta = 0.5 * rng.standard_normal(orc.p)
        x0, inputs, g = 0.3 * rng.standard_normal((B, orc.n)), rng.standard_normal((B, T, orc.m)), rng.standard_normal((B, T + 1, orc.n))
        c = dict(sid=sid, orc=orc, x0=x0, inputs=inputs, theta=theta, g=g)
        c["states"], c["grad_theta"], c["grad_x0"] = reference(orc, x0, inputs, theta, g)
        assert np.isfinite(c["states"]).all()
        _cases[key] = c
    return _cases[key]
