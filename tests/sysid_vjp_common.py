"""Shared by tests/test_sysid_vjp_host.py, tests/test_gpu_sysid_vjp.py and the pair tests/test_sysid_vjp_sizes_host.py, tests/test_gpu_sysid_vjp_sizes.py (user models
with small pools, several parameter slots and n = 64: SIZE_MODELS below): the CPU reference of the SysID rollout's vector-Jacobian product
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


def _chain(lib, nm, m, dt):
    """nm masses in a row between two walls, actuators on the masses 0, 2, .., 2 (m - 1); stiffness, damping and a cubic coefficient are the unknowns"""
    qs, vs, us, ws = sg._symbols(lib, (("q", nm), ("v", nm), ("u", m), ("w", 3)))
    f = [qs[i] + dt * vs[i] for i in range(nm)]
    for i in range(nm):
        left = qs[i - 1] if i > 0 else 0.0
        right = qs[i + 1] if i + 1 < nm else 0.0
        a = ws[0] * (left - 2 * qs[i] + right) - ws[1] * vs[i] - ws[2] * qs[i] * qs[i] * qs[i]
        if i % 2 == 0 and i // 2 < m:
            a = a + us[i // 2]
        f.append(vs[i] + dt * a)
    return qs + vs, us, ws, f


def chain_40_10_3(lib, dt=0.05):
    """the 40-state chain of tests/test_gpu_generic_sizes.py, restated: 20 masses, 10 actuators"""
    return _chain(lib, 20, 10, dt)


def chain_64_4_3(lib, dt=0.05):
    """the same equations with 32 masses and 4 actuators: n = 64, every lane of the sweep owns a costate"""
    return _chain(lib, 32, 4, dt)


def chain_66(lib, dt=0.05):
    """33 masses: n = 66, two states beyond what pdp_sysid_rollout_vjp_batched takes (PDP_E_SIZE); the host test builds it, nothing launches it"""
    return _chain(lib, 33, 4, dt)


def mlp_6_2_246(lib, dt=0.05, hidden=16):
    """learned dynamics x+ = x + dt (W2 tanh(W1 [x; u] + b1) + b2), theta = (vec W1, b1, vec W2, b2) row-major: (n, m, p) = (6, 2, 246) - a dense E, four parameter slots
    with 54 live lanes in the last one, and a pool of four rows"""
    n, m = 6, 2
    xs, us, w1, b1, w2, b2 = sg._symbols(lib, (("x", n), ("u", m), ("a", hidden * (n + m)), ("b", hidden), ("c", n * hidden), ("d", n)))
    if lib == "sx":
        from pdp_amd.sx import tanh
    else:
        from sympy import tanh
    z = xs + us
    hid = []
    for k in range(hidden):
        acc = b1[k]
        for j in range(n + m):
            acc = acc + w1[k * (n + m) + j] * z[j]
        hid.append(tanh(acc))
    f = []
    for i in range(n):
        acc = b2[i]
        for k in range(hidden):
            acc = acc + w2[i * hidden + k] * hid[k]
        f.append(xs[i] + dt * acc)
    return xs, us, w1 + b1 + w2 + b2, f


LINEAR_8_B0 = (1.0, -0.5, 0.25, 0.75, -1.0, 0.5, -0.25, 1.25)


def _linear_8_1(lib, gain, dt):
    n = 8
    xs, us, a, c = sg._symbols(lib, (("x", n), ("u", 1), ("a", n * n), ("c", 1)))
    f = []
    for i in range(n):
        acc = a[i * n] * xs[0]
        for j in range(1, n):
            acc = acc + a[i * n + j] * xs[j]
        acc = acc + (LINEAR_8_B0[i] * c[0] * us[0] if gain else LINEAR_8_B0[i] * us[0])
        f.append(xs[i] + dt * acc)
    return xs, us, a + c if gain else a, f


def linear_8_1_64(lib, dt=0.05):
    """x+ = x + dt (A x + b0 u), theta = vec A row-major, b0 = LINEAR_8_B0: p = 64, one parameter slot in which every lane is live"""
    return _linear_8_1(lib, False, dt)


def linear_8_1_65(lib, dt=0.05):
    """the same with a gain on the input, x+ = x + dt (A x + theta_64 b0 u): p = 65, a second slot with one live lane"""
    return _linear_8_1(lib, True, dt)


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


# the models of tests/test_gpu_sysid_vjp_sizes.py and tests/test_sysid_vjp_sizes_host.py: small pools (CHUNK = 4, 8, 16), full and barely started parameter slots, n = 64
# (chain_66 is beyond the kernel: the host test alone builds it)
SIZE_MODELS = {"mlp_6_2_246": (mlp_6_2_246, "mlp sysid 6 2 246"), "chain_64_4_3": (chain_64_4_3, "chain sysid 64"),
               "linear_8_1_64": (linear_8_1_64, "linear sysid 8 1 64"), "linear_8_1_65": (linear_8_1_65, "linear sysid 8 1 65"), "chain_66": (chain_66, "chain sysid 66")}
_models = {}


def size_problem(name):
    """(codegen.Problem, PDP.SysID) of SIZE_MODELS[name] without building it: what codegen.generate / build_problem take"""
    from pdp_amd import PDP, codegen
    sid = user_pair(name)[0]
    return codegen.Problem(codegen.KIND_SYSID, sid.state, sid.control, sid.dyn, sid.auxvar, label=PDP._label(sid.project_name)), sid


def user_pair(name):
    """user_model of USER_MODELS / SIZE_MODELS [name], made once per process (the sympy oracle of the MLP takes seconds)"""
    if name not in _models:
        _models[name] = user_model(*(USER_MODELS.get(name) or SIZE_MODELS[name]))
    return _models[name]


def user_case(name, seed=5, B=3, T=10):
    """the inputs of the size tests for USER_MODELS / SIZE_MODELS [name]: dict(sid (PDP.SysID), orc, x0 [B,n], inputs [B,T,m], theta [p], theta_b [B,p], g [B,T+1,n], and
    the oracle's reference for the shared theta: states, grad_theta, grad_x0).  x0 = 0.3 N(0,1), inputs and cotangents N(0,1), theta = 0.5 N(0,1) (the chains: stiffness 1.7,
    damping 0.5, cubic 0.2), theta_b within 5 % of it.  Computed once and shared: do not write into it."""
    key = ("user", name, seed, B, T)
    if key not in _cases:
        sid, orc = user_pair(name)
        rng = np.random.default_rng(seed)
        if name.startswith("chain"):
            theta = np.array([1.7, 0.5, 0.2])
        else:
            theta = 0.5 * rng.standard_normal(orc.p)
        x0, inputs, g = 0.3 * rng.standard_normal((B, orc.n)), rng.standard_normal((B, T, orc.m)), rng.standard_normal((B, T + 1, orc.n))
        theta_b = theta * (1.0 + 0.05 * rng.standard_normal((B, orc.p)))
        c = dict(sid=sid, orc=orc, x0=x0, inputs=inputs, theta=theta, theta_b=theta_b, g=g)
        c["states"], c["grad_theta"], c["grad_x0"] = reference(orc, x0, inputs, theta, g)
        assert np.isfinite(c["states"]).all()
        _cases[key] = c
    return _cases[key]


def prefix(c, T, theta_key="theta"):
    """the first T steps of a user_case with their own reference (the whole case when T is its horizon and the theta is the shared one)"""
    if T == c["inputs"].shape[1] and theta_key == "theta":
        return c
    key = ("prefix", id(c), T, theta_key)
    if key not in _cases:
        d = dict(sid=c["sid"], orc=c["orc"], x0=c["x0"], inputs=c["inputs"][:, :T], theta=c[theta_key], g=c["g"][:, :T + 1])
        d["states"], d["grad_theta"], d["grad_x0"] = reference(c["orc"], d["x0"], d["inputs"], d["theta"], d["g"])
        assert np.isfinite(d["states"]).all()
        _cases[key] = d
    return _cases[key]
