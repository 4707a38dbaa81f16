"""Shared by tests/test_sysid_gn_host.py and tests/test_gpu_sysid_gn.py: the CPU reference of SysID.step as a nonlinear least-squares evaluation - loss, gradient and
Gauss-Newton matrix per trajectory from SysIDOracle.integrateDyn / getAuxSys / integrateAuxSys, masks and contractions in numpy - the data the tests run on, and the
Levenberg-Marquardt schedule (pdp_amd.irl.LMLoop, default settings) restated on that reference.

Semantics: a NaN in x_obs is an entry that was not observed (skip_missing); the rollout starts from ini_state (None: x_obs[0]); row 0 adds
|ini_state - x_obs_0|^2 over its observed entries to the loss and - X_0 = 0 - nothing to gradient and G."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SYSTEMS = ["pendulum", "cartpole", "robotarm", "rocket", "quadrotor"]
TOL = 1e-10                         # relative to the largest entry per sample
_cache = {}


def oracle(system):
    from oracle import models, pdp_oracle as po
    if system not in _cache:
        st = models.SYSID_SETUP[system]
        _cache[system] = po.make_sysid(models.REGISTRY[system](**st["kwargs"]), st["dt"])
    return _cache[system]


def stored(system):
    """(inputs [B,T,m], states [B,T+1,n], true_parameter [p], theta [p] of the reference's stored run)"""
    io = np.load(os.path.join(GOLDEN, "iodata_%s.npz" % system))
    return io["inputs"], io["states"], io["true_parameter"], np.load(os.path.join(GOLDEN, "ref_sysid_%s.npz" % system))["theta"]


def reference_rows(sid, inputs, states, theta, ini_state=None, skip_missing=False, samples=None):
    """(loss [k], grad [k,p], G [k,p,p]) of the trajectories `samples` (default: all): theta [p] or [B,p]"""
    inputs, states, theta = np.asarray(inputs, float), np.asarray(states, float), np.asarray(theta, float)
    samples = range(inputs.shape[0]) if samples is None else samples
    loss, grad, G = [], [], []
    for b in samples:
        th = theta[b] if theta.ndim == 2 else theta
        xs = sid.integrateDyn(states[b, 0] if ini_state is None else np.asarray(ini_state, float)[b], inputs[b], th)
        aux = sid.getAuxSys(xs, inputs[b], th)
        X = np.stack(sid.integrateAuxSys(aux["dynF"], aux["dynE"], np.zeros((sid.n, sid.p)))["state_traj"])          # [T+1, n, p]
        d = xs - states[b]
        if skip_missing:
            obs = ~np.isnan(states[b])
            d, X = np.where(obs, d, 0.0), np.where(obs[:, :, None], X, 0.0)
        loss.append((d * d).sum())
        grad.append(np.einsum("ti,tip->p", d, X))
        G.append(np.einsum("tip,tiq->pq", X, X))
    return np.array(loss), np.array(grad), np.array(G)


def observe(states, every, components, steps=None):
    """states with NaN everywhere but at `components` of the steps t = every, 2 every, ... (or exactly `steps`)"""
    out = np.full_like(np.asarray(states, float), np.nan)
    ts = list(range(every, states.shape[1], every)) if steps is None else list(steps)
    for t in ts:
        out[:, t, components] = states[:, t, components]
    return out


# the eight inputs of the Levenberg-Marquardt tests: (tag, system, observed entries or None = all, evaluations of the oracle schedule at loss_tol = 1e-20)
LM_INPUTS = [("pendulum", "pendulum", None, 6), ("cartpole", "cartpole", None, 4), ("robotarm", "robotarm", None, 5), ("rocket", "rocket", None, 5),
             ("quadrotor", "quadrotor", None, 8),
             ("pendulum, component 0 at t = 2, 4, .., 20", "pendulum", dict(every=2, components=[0]), 6),
             ("cartpole, components 0, 1 at t = 5, 10, 15, 20", "cartpole", dict(every=5, components=[0, 1]), 4),
             ("quadrotor, components 0, 1, 2, 6-9 at t = 5, 10", "quadrotor", dict(every=5, components=[0, 1, 2, 6, 7, 8, 9]), 8)]
LM_THETA_SYSTEMS = ("pendulum", "cartpole", "quadrotor")            # full observations: |theta - theta*| <= 1e-6 (G is singular for the robot arm and the rocket)


def lm_input(k):
    """dict(inputs, states (NaN where not observed), ini_state or None, skip_missing, theta0, true_parameter) of LM_INPUTS[k]"""
    _, system, obs, _ = LM_INPUTS[k]
    inputs, states, true_parameter, theta0 = stored(system)
    if obs is None:
        return dict(system=system, inputs=inputs, states=states, ini_state=None, skip_missing=False, theta0=theta0, true_parameter=true_parameter)
    return dict(system=system, inputs=inputs, states=observe(states, **obs), ini_state=states[:, 0].copy(), skip_missing=True, theta0=theta0, true_parameter=true_parameter)


def oracle_lm(k, loss_tol, max_evals=50):
    """the schedule of irl.LMLoop (default settings) on the CPU reference: results() of the loop"""
    from pdp_amd.irl import LMLoop
    c = lm_input(k)
    sid = oracle(c["system"])

    def evaluate(theta):
        loss, grad, G = reference_rows(sid, c["inputs"], c["states"], theta, c["ini_state"], c["skip_missing"])
        return loss.mean(), grad.mean(axis=0), G.mean(axis=0)
    return LMLoop(evaluate, c["theta0"]).run(max_evals=max_evals, loss_tol=loss_tol)


def rel_rows(a, ref):
    """per sample: largest deviation relative to the largest entry of the reference's row; the worst sample"""
    a, ref = np.asarray(a, float).reshape(len(ref), -1), np.asarray(ref, float).reshape(len(ref), -1)
    return float((np.abs(a - ref).max(axis=1) / np.maximum(np.abs(ref).max(axis=1), 1e-300)).max())


def mask_states(states):
    """the parity tests' mask: every second step (t odd), every second component; row 0 not observed (the caller gives ini_state); sample 1 with nothing observed"""
    out = np.full_like(np.asarray(states, float), np.nan)
    out[:, 1::2, 0::2] = states[:, 1::2, 0::2]
    out[1] = np.nan
    return out


def chain_16_2_16(lib, dt=0.05):
    """a linear chain of 8 masses, 2 actuators; the unknowns are the 8 stiffnesses and 8 dampings: (n, m, p) = (16, 2, 16) - the largest model of the fused kernels"""
    nm, m = 8, 2
    qs, vs, us, ks, cs = _symbols(lib, (("q", nm), ("v", nm), ("u", m), ("k", nm), ("c", nm)))
    f = [qs[i] + dt * vs[i] for i in range(nm)]
    for i in range(nm):
        left = qs[i - 1] if i > 0 else 0.0
        right = qs[i + 1] if i + 1 < nm else 0.0
        a = ks[i] * (left - 2 * qs[i] + right) - cs[i] * vs[i]
        if i % 4 == 0:
            a = a + us[i // 4]
        f.append(vs[i] + dt * a)
    return qs + vs, us, ks + cs, f


def chain_5_1_17(lib, dt=0.05):
    """a linear first-order chain of 5 cells, one input; the unknowns are the tridiagonal couplings (5 + 4 + 4) and 4 input gains: (n, m, p) = (5, 1, 17) - one parameter
    beyond the Gauss-Newton kernels' tile"""
    n = 5
    xs, us, ds, ups, los, bs = _symbols(lib, (("x", n), ("u", 1), ("d", n), ("a", n - 1), ("l", n - 1), ("b", n - 1)))
    f = []
    for i in range(n):
        a = -ds[i] * xs[i]
        if i + 1 < n:
            a = a + ups[i] * xs[i + 1] + bs[i] * us[0]
        if i > 0:
            a = a + los[i - 1] * xs[i - 1]
        f.append(xs[i] + dt * a)
    return xs, us, ds + ups + los + bs, f


def _symbols(lib, groups):
    if lib == "sx":
        from pdp_amd.sx import SX
        out = []
        for name, k in groups:
            v = SX.sym(name, k)
            out.append([v[i] for i in range(k)])
        return out
    import sympy as sp
    return [list(sp.symbols("%s0:%d" % (name, k), real=True)) for name, k in groups]
