"""Shared by tests/test_sysid_vjp_u_host.py and tests/test_gpu_sysid_vjp_u.py: the CPU reference of the SysID rollout's gradient with respect to the inputs
(pdp_sysid_rollout_vjp_u_batched, include/pdp_hip_sysid_vjp_u.h) and the cases the tests run on - those of tests/sysid_vjp_common.py (case, user_case, prefix) with
grad_u added, and one more user model, linear_8_2_63.

The reference is NOT the kernel's method.  G_t = df/du comes from sympy, from the same expressions the oracle is built from ((X + dt f).jacobian(U) through
pdp_oracle._lamb for the zoo, the model's builder("sympy") for user models) and is propagated FORWARD: D_{t+1} = G_t, grad_u[t] = sum_{s > t} g_s' D_s,
D_{s+1} = F_s D_s.  adjoint_sweep_u is the kernel's recursion in numpy, kept to state how far the two orders of the same sums agree on the CPU."""
import numpy as np

import sysid_vjp_common as sv

ROOT, SYSTEMS, TOL, EDGE_T = sv.ROOT, sv.SYSTEMS, sv.TOL, sv.EDGE_T
rel_rows = sv.rel_rows
_gfn, _cases, _models = {}, {}, {}


def linear_8_2_63(lib, dt=0.05):
    """x+ = x + dt (A x + B u), n = 8, m = 2; theta = the first 63 entries of vec A (row-major), A[7][7] = -0.4 and B are constants: p = 63, so the two G columns are
    the columns 63 and 64 of [E | G] - the last lane of the first 64-lane slot and the first lane of the second"""
    n, m = 8, 2
    xs, us, a = sv.sg._symbols(lib, (("x", n), ("u", m), ("a", n * n - 1)))
    coef = list(a) + [-0.4]
    bmat = [[sv.LINEAR_8_B0[i], sv.LINEAR_8_B0[(i + 3) % n] * 0.5] for i in range(n)]
    f = []
    for i in range(n):
        acc = coef[i * n] * xs[0]
        for j in range(1, n):
            acc = acc + coef[i * n + j] * xs[j]
        for j in range(m):
            acc = acc + bmat[i][j] * us[j]
        f.append(xs[i] + dt * acc)
    return xs, us, a, f


U_MODELS = {"linear_8_2_63": (linear_8_2_63, "linear sysid 8 2 63")}


def builder_of(name):
    return (U_MODELS.get(name) or sv.USER_MODELS.get(name) or sv.SIZE_MODELS[name])[0]


def user_pair(name):
    """(PDP.SysID, SysIDOracle) of a user model, made once per process: sysid_vjp_common's own models are shared with its tests"""
    if name not in U_MODELS:
        return sv.user_pair(name)
    if name not in _models:
        _models[name] = sv.user_model(*U_MODELS[name])
    return _models[name]


def size_problem(name):
    from pdp_amd import PDP, codegen
    sid = user_pair(name)[0]
    return codegen.Problem(codegen.KIND_SYSID, sid.state, sid.control, sid.dyn, sid.auxvar, label=PDP._label(sid.project_name)), sid


def g_fn(name):
    """G(x, u, theta) [n, m] = d(x + dt f)/du from sympy, for a zoo system or a user model"""
    if name not in _gfn:
        import sympy as sp
        from oracle import models, pdp_oracle as po
        if name in SYSTEMS:
            st = models.SYSID_SETUP[name]
            mdl = models.REGISTRY[name](**st["kwargs"])
            X, U, w, dyn = sp.Matrix(mdl.X), sp.Matrix(mdl.U), list(mdl.dyn_auxvar), sp.Matrix(mdl.X + st["dt"] * mdl.f)
        else:
            Xs, Us, ws, fs = builder_of(name)("sympy")
            X, U, w, dyn = sp.Matrix(Xs), sp.Matrix(Us), list(ws), sp.Matrix(fs)
        fn = po._lamb([list(X), list(U), w], dyn.jacobian(U))
        n, m = len(X), len(U)
        _gfn[name] = lambda x, u, th: np.asarray(fn(x, u, np.asarray(th, float).reshape(-1)), float).reshape(n, m)
    return _gfn[name]


def reference_u(name, orc, states, inputs, theta, g):
    """grad_u [B, T, m] by forward propagation of G_t along the given rollouts `states` [B, T+1, n]; theta [p] or [B, p], g [B, T+1, n] the cotangents"""
    G = g_fn(name)
    inputs, g, theta = np.asarray(inputs, float), np.asarray(g, float), np.asarray(theta, float)
    B, T, m = inputs.shape
    out = np.zeros((B, T, m))
    for b in range(B):
        th = theta[b] if theta.ndim == 2 else theta
        F = orc.getAuxSys(states[b], inputs[b], th)["dynF"]
        for t in range(T):
            D = G(states[b, t], inputs[b, t], th)                  # dx_{t+1}/du_t
            for s in range(t + 1, T + 1):
                out[b, t] += g[b, s] @ D
                if s < T:
                    D = F[s] @ D
    return out


def adjoint_sweep_u(name, orc, xs, inputs, theta, g):
    """the kernel's recursion for ONE trajectory in numpy: grad_u [T, m]"""
    G = g_fn(name)
    F = orc.getAuxSys(xs, inputs, theta)["dynF"]
    lam, out = np.array(g[-1], float), np.zeros(np.shape(inputs))
    for t in range(len(inputs) - 1, -1, -1):
        out[t] = G(xs[t], inputs[t], theta).T @ lam
        lam = g[t] + F[t].T @ lam
    return out


def case(system, T=None, seed=7):
    """sysid_vjp_common.case with grad_u (shared theta) and grad_u_b (per-sample theta) added.  Computed once and shared: do not write into it."""
    key = ("zoo", system, T, seed)
    if key not in _cases:
        c = dict(sv.case(system, T, seed))
        c["grad_u"] = reference_u(system, c["sid"], c["states"], c["inputs"], c["theta"], c["g"])
        c["grad_u_b"] = reference_u(system, c["sid"], c["states_b"], c["inputs"], c["theta_b"], c["g"])
        _cases[key] = c
    return _cases[key]


def _base_user_case(name, seed, B, T):
    if name not in U_MODELS:
        return sv.user_case(name, seed=seed, B=B, T=T)
    sid, orc = user_pair(name)                                     # (sysid_vjp_common.user_case's recipe)
    rng = np.random.default_rng(seed)
    theta = 0.5 * rng.standard_normal(orc.p)
    x0, inputs, g = 0.3 * rng.standard_normal((B, orc.n)), rng.standard_normal((B, T, orc.m)), rng.standard_normal((B, T + 1, orc.n))
    theta_b = theta * (1.0 + 0.05 * rng.standard_normal((B, orc.p)))
    c = dict(sid=sid, orc=orc, x0=x0, inputs=inputs, theta=theta, theta_b=theta_b, g=g)
    c["states"], c["grad_theta"], c["grad_x0"] = sv.reference(orc, x0, inputs, theta, g)
    assert np.isfinite(c["states"]).all()
    return c


def user_case(name, seed=5, B=3, T=10):
    """sysid_vjp_common.user_case (the same inputs, the same reference for grad_theta and grad_x0) with grad_u for the shared theta added; `name` as well"""
    key = ("user", name, seed, B, T)
    if key not in _cases:
        c = dict(_base_user_case(name, seed, B, T), name=name)
        c["grad_u"] = reference_u(name, c["orc"], c["states"], c["inputs"], c["theta"], c["g"])
        _cases[key] = c
    return _cases[key]


def prefix(c, T):
    """the first T steps of a user_case with their own reference (the whole case when T is its horizon)"""
    if T == c["inputs"].shape[1]:
        return c
    key = ("prefix", id(c), T)
    if key not in _cases:
        d = dict(sv.prefix(c, T), name=c["name"])
        d["grad_u"] = reference_u(c["name"], c["orc"], d["states"], d["inputs"], d["theta"], d["g"])
        _cases[key] = d
    return _cases[key]
