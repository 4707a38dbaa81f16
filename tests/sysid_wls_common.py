"""Shared by tests/test_sysid_wls_host.py and tests/test_gpu_sysid_wls.py: the CPU reference of SysID.step as WEIGHTED and HUBER-ROBUST least squares - the rows
grad [W] | loss | G [W][W] per trajectory from SysIDOracle.integrateDyn / getAuxSys / integrateAuxSys (started at the selection matrix), the weights, Huber's rule and
the contractions in numpy - the corrupted data set, and the Levenberg-Marquardt schedule (pdp_amd.irl.LMLoop, default settings) restated on that reference.

Semantics (include/pdp_hip_sysid_wls.h).  An entry is OBSERVED iff w > 0 and (skip_missing) x_obs is not NaN; anything else adds nothing.  With
d = x - x_obs:  e = sqrt(w) d,  psi = 1 if |e| <= delta else delta / |e|,  rho = e^2 if |e| <= delta else 2 delta |e| - delta^2,  s = sqrt(w psi);
loss = sum rho,  grad = sum_t (s d_t)' (s X_t),  G = sum_t (s X_t)' (s X_t) over the observed entries; X_t is never scaled in its recursion."""
import numpy as np

import sysid_gn_common as sg
import sysid_ini_common as si

ROOT, TOL, SYSTEMS = sg.ROOT, sg.TOL, sg.SYSTEMS
INF = float("inf")
CORRUPTED_ENTRIES = {"pendulum": 10, "cartpole": 17, "quadrotor": 21}
HUBER_DELTA = 0.01                  # the threshold of the robust runs


def full_weights(weights, B, T, n):
    """weights broadcast to [B, T+1, n]; None: ones"""
    if weights is None:
        return np.ones((B, T + 1, n))
    return np.broadcast_to(np.asarray(weights, float), (B, T + 1, n))


def huber(e, delta):
    """(rho, psi) of the standardised residual e; the comparison is |e| <= delta (a NaN takes the second branch and stays a NaN)"""
    ae = np.abs(e)
    with np.errstate(divide="ignore", invalid="ignore"):
        quad = ae <= delta
        return np.where(quad, e * e, 2.0 * delta * ae - delta * delta), np.where(quad, 1.0, delta / ae)


def row_terms(xs, X, x_obs, w, delta, skip_missing):
    """(loss, sd [T+1, n], sX [T+1, n, W]) of one trajectory: selects, never products with 0"""
    d = xs - x_obs
    obs = (w > 0) & (~np.isnan(x_obs) if skip_missing else True)
    with np.errstate(invalid="ignore"):
        rho, psi = huber(np.sqrt(np.where(w > 0, w, 0.0)) * d, delta)
        s = np.sqrt(np.where(w > 0, w, 0.0) * psi)
        return np.where(obs, rho, 0.0).sum(), np.where(obs, s * d, 0.0), np.where(obs[:, :, None], s[:, :, None] * X, 0.0)


def reference_rows(sid, inputs, states, theta, idx=(), ini_state=None, skip_missing=False, weights=None, delta=INF, samples=None):
    """(loss [k], grad [k, W], G [k, W, W]) of the trajectories `samples` (default: all); theta [p] or [B, p]; ini_state None: states[:, 0]; weights [n], [T+1, n] or
    [B, T+1, n] or None; idx: the estimated components of x0 (W = p + len(idx))"""
    inputs, states, theta = np.asarray(inputs, float), np.asarray(states, float), np.asarray(theta, float)
    B, T, n = inputs.shape[0], inputs.shape[1], states.shape[2]
    w = full_weights(weights, B, T, n)
    samples = range(B) if samples is None else samples
    loss, grad, G = [], [], []
    for b in samples:
        th = theta[b] if theta.ndim == 2 else theta
        xs, X = si.sensitivities(sid, inputs[b], th, states[b, 0] if ini_state is None else np.asarray(ini_state, float)[b], list(idx))
        l, sd, sX = row_terms(xs, X, states[b], w[b], delta, skip_missing)
        loss.append(l)
        grad.append(np.einsum("ti,tip->p", sd, sX))
        G.append(np.einsum("tip,tiq->pq", sX, sX))
    return np.array(loss), np.array(grad), np.array(G)


def loss_only(sid, inputs_b, states_b, theta, ini, w_b, delta, skip_missing):
    """the loss of one trajectory without any sensitivity: what the central differences differentiate"""
    xs = sid.integrateDyn(ini, inputs_b, theta)
    d = xs - states_b
    obs = (w_b > 0) & (~np.isnan(states_b) if skip_missing else True)
    with np.errstate(invalid="ignore"):
        rho, _ = huber(np.sqrt(w_b) * d, delta)
    return np.where(obs, rho, 0.0).sum()


_corrupted = {}


def corrupted(system):
    """dict(inputs, states (corrupted), clean, mask (the corrupted entries), ini_state (clean states[:, 0]), trust (the trust weights), theta0, true_parameter).  5 % of the
    recorded entries (never row 0) are moved by +-(0.5 .. 1.5); the trust weights are 0 on them and 1 + i on component i elsewhere."""
    if system not in _corrupted:
        inputs, clean, true_parameter, theta0 = sg.stored(system)
        states = np.array(clean, dtype=float)
        rng = np.random.default_rng(7)
        mask = rng.random(states.shape) < 0.05
        mask[:, 0] = False
        k = int(mask.sum())
        states[mask] += rng.choice([-1., 1.], k) * (0.5 + rng.random(k))
        trust = np.where(mask, 0.0, 1.0) * (1.0 + np.arange(states.shape[2]))
        _corrupted[system] = dict(system=system, inputs=inputs, states=states, clean=np.array(clean, dtype=float), mask=mask, ini_state=np.array(clean[:, 0], dtype=float),
                                  trust=trust, theta0=theta0, true_parameter=true_parameter)
    return _corrupted[system]


# evaluations (rejected) of the oracle schedule (irl.LMLoop, default settings, loss_tol = 1e-20, at most 50 evaluations) on the corrupted data with the trust weights
TRUST_COUNTS = {"pendulum": 6, "cartpole": 5, "quadrotor": 8}
_lm = {}


def oracle_lm(system, weights=None, delta=INF, loss_tol=1e-20, max_evals=50):
    """the schedule of irl.LMLoop (default settings) on the CPU reference, one theta shared by the recordings (the mean of the rows): results() of the loop.  weights:
    None, "trust" or an array; computed once per argument set and shared between the tests"""
    from pdp_amd.irl import LMLoop
    key = (system, weights if weights is None or isinstance(weights, str) else id(weights), delta, loss_tol, max_evals)
    if key not in _lm:
        c, sid = corrupted(system), sg.oracle(system)
        w = c["trust"] if isinstance(weights, str) else weights

        def evaluate(theta):
            loss, grad, G = reference_rows(sid, c["inputs"], c["states"], theta, (), c["ini_state"], False, w, delta)
            return loss.mean(), grad.mean(axis=0), G.mean(axis=0)
        _lm[key] = LMLoop(evaluate, c["theta0"]).run(max_evals=max_evals, loss_tol=loss_tol)
    return _lm[key]


def theta_error(result, system):
    return float(np.abs(result["parameter_trace"][-1] - corrupted(system)["true_parameter"]).max())
