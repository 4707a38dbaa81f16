"""Shared by tests/test_sysid_ini_host.py and tests/test_gpu_sysid_ini.py: the CPU reference of SysID.step with estimated components of the initial state - the
augmented rows grad [W] | loss | G [W][W] per trajectory from SysIDOracle.integrateDyn / getAuxSys / integrateAuxSys started at the selection matrix, masks and
contractions in numpy - the arrow-shaped normal equations of one shared theta with one initial state per recording in numpy, the dense Jacobian they are checked
against, and the inputs of the tests.

Semantics: idx = the estimated components i_0 < i_1 < ... of x0, unknown p + k is x0[i_k], W = p + q.  X_0 [n][W] = zeros with
X_0[i_k][p + k] = 1, X_{t+1} = F_t X_t + [E_t | 0]; loss as in section 4.1d (row 0's |x0 - x_obs_0|^2 over its observed entries included); grad = sum_{t<=T} d_t' X_t,
G = sum_{t<=T} X_t' X_t with the masks of skip_missing."""
import numpy as np

import sysid_gn_common as sg
from ls_rows_common import Recorder  # noqa: F401  (the host tests take it from here)

ROOT, TOL = sg.ROOT, sg.TOL

# the parity cases: (system, estimated components).  The last one is the full tile: W = 5 + 11 = 16
PARITY = [("pendulum", [1]), ("cartpole", [2, 3]), ("cartpole", [0, 3]), ("robotarm", [2, 3]), ("rocket", [3, 4, 5, 10, 11, 12]),
          ("quadrotor", [3, 4, 5, 10, 11, 12]), ("quadrotor", list(range(2, 13)))]
PARITY_IDS = ["%s_%s" % (s, "_".join(str(i) for i in idx)) for s, idx in PARITY]


def selection(n, p, idx):
    X0 = np.zeros((n, p + len(idx)))
    for k, i in enumerate(idx):
        X0[i, p + k] = 1.0
    return X0


def sensitivities(sid, inputs_b, theta, x0, idx):
    """(x [T+1, n], X [T+1, n, W]) of one trajectory from (theta, x0)"""
    xs = sid.integrateDyn(x0, inputs_b, theta)
    aux = sid.getAuxSys(xs, inputs_b, theta)
    E = [np.concatenate([e, np.zeros((sid.n, len(idx)))], axis=1) for e in aux["dynE"]]
    return xs, np.stack(sid.integrateAuxSys(aux["dynF"], E, selection(sid.n, sid.p, idx))["state_traj"])


def reference_rows(sid, inputs, states, theta, idx, ini_state=None, skip_missing=False, samples=None):
    """(loss [k], grad [k, W], G [k, W, W]) of the trajectories `samples` (default: all); theta [p] or [B, p]; ini_state None: states[:, 0]"""
    inputs, states, theta = np.asarray(inputs, float), np.asarray(states, float), np.asarray(theta, float)
    samples = range(inputs.shape[0]) if samples is None else samples
    loss, grad, G = [], [], []
    for b in samples:
        th = theta[b] if theta.ndim == 2 else theta
        xs, X = sensitivities(sid, inputs[b], th, states[b, 0] if ini_state is None else np.asarray(ini_state, float)[b], idx)
        d = xs - states[b]
        if skip_missing:
            obs = ~np.isnan(states[b])
            d, X = np.where(obs, d, 0.0), np.where(obs[:, :, None], X, 0.0)
        loss.append((d * d).sum())
        grad.append(np.einsum("ti,tip->p", d, X))
        G.append(np.einsum("tip,tiq->pq", X, X))
    return np.array(loss), np.array(grad), np.array(G)


def packed(rows):
    loss, grad, G = rows
    return np.concatenate([grad, loss[:, None], G.reshape(len(loss), -1)], axis=1)


def unpack(row, W):
    row = np.asarray(row)
    return row[:, W], row[:, :W], row[:, W + 1:].reshape(len(row), W, W)


def arrow(loss, grad, G, p):
    """the normal equations of [theta | x0_0[idx] | ... | x0_{B-1}[idx]] with the mean over the B recordings as the loss: (loss, g [N], A [N, N])"""
    B, W = grad.shape
    q = W - p
    N = p + B * q
    g, A = np.zeros(N), np.zeros((N, N))
    for b in range(B):
        s = slice(p + b * q, p + (b + 1) * q)
        g[:p] += grad[b, :p] / B
        g[s] = grad[b, p:] / B
        A[:p, :p] += G[b, :p, :p] / B
        A[:p, s] = G[b, :p, p:] / B
        A[s, :p] = G[b, p:, :p] / B
        A[s, s] = G[b, p:, p:] / B
    return loss.sum() / B, g, A


def dense_jacobian(sid, inputs, states, theta, idx, ini_state, skip_missing):
    """(r [B (T+1) n], J [B (T+1) n, N]) of the stacked residuals with respect to [theta | x0_0[idx] | ...]; rows of entries that were not observed are zero"""
    B, p, q = inputs.shape[0], sid.p, len(idx)
    N = p + B * q
    rs, Js = [], []
    for b in range(B):
        xs, X = sensitivities(sid, inputs[b], theta, ini_state[b], idx)
        d = xs - states[b]
        if skip_missing:
            obs = ~np.isnan(states[b])
            d, X = np.where(obs, d, 0.0), np.where(obs[:, :, None], X, 0.0)
        J = np.zeros((d.size, N))
        J[:, :p] = X[:, :, :p].reshape(d.size, p)
        J[:, p + b * q:p + (b + 1) * q] = X[:, :, p:].reshape(d.size, q)
        rs.append(d.reshape(-1))
        Js.append(J)
    return np.concatenate(rs), np.concatenate(Js)


def perturbed_case(system, idx, seed):
    """masked data (sysid_gn_common.mask_states), a perturbed theta and a perturbed x0: what the central differences and the arrow matrix are checked on"""
    inputs, states, _, theta = sg.stored(system)
    rng = np.random.default_rng(seed)
    return dict(inputs=inputs, states=sg.mask_states(states), theta=theta * (1.0 + 0.05 * rng.standard_normal(theta.size)),
                ini=states[:, 0] + 0.05 * rng.standard_normal(states[:, 0].shape))


# ---- Levenberg-Marquardt: positions and attitudes observed at every step, the velocity components of x0 unknown and started at 0 -------------------------------------
LM_SYSTEMS = {"cartpole": dict(observed=[0, 1], idx=[2, 3]), "quadrotor": dict(observed=[0, 1, 2, 6, 7, 8, 9], idx=[3, 4, 5, 10, 11, 12])}
SCALES = (1.0, 0.9, 1.1)
# evaluations of the oracle schedule (irl.LMLoop, default settings) at loss_tol = 1e-20, none rejected
SHARED_COUNTS = {("cartpole", 1.0): 5, ("cartpole", 0.9): 6, ("cartpole", 1.1): 5, ("quadrotor", 1.0): 8}
# per trajectory: [scale][trajectory]
PER_TRAJECTORY_COUNTS = {"cartpole": {1.0: (5, 5, 6), 0.9: (6, 5, 6), 1.1: (6, 6, 6)}, "quadrotor": {1.0: (8, 10, 8)}}


def lm_data(system):
    """dict(inputs, states (NaN where not observed), ini_state (the estimated components 0), idx, theta_ref, x0_true)"""
    inputs, states, _, theta = sg.stored(system)
    c = LM_SYSTEMS[system]
    obs = np.full_like(states, np.nan)
    obs[:, :, c["observed"]] = states[:, :, c["observed"]]
    ini = states[:, 0].copy()
    ini[:, c["idx"]] = 0.0
    return dict(system=system, inputs=inputs, states=obs, ini_state=ini, idx=c["idx"], theta_ref=theta, x0_true=states[:, 0].copy())


def oracle_lm_shared(system, scale, loss_tol, max_evals=50):
    """irl.LMLoop (default settings) on the CPU reference: one shared theta from theta_ref * scale, one unknown x0 part per recording"""
    from pdp_amd.irl import LMLoop
    c, sid = lm_data(system), sg.oracle(system)
    B, p, idx = c["inputs"].shape[0], sid.p, c["idx"]

    def evaluate(v):
        ini = c["ini_state"].copy()
        ini[:, idx] = v[p:].reshape(B, len(idx))
        loss, grad, G = reference_rows(sid, c["inputs"], c["states"], v[:p], idx, ini, True)
        return arrow(loss, grad, G, p)
    return LMLoop(evaluate, np.concatenate([c["theta_ref"] * scale, c["ini_state"][:, idx].reshape(-1)])).run(max_evals=max_evals, loss_tol=loss_tol)


def oracle_lm_trajectory(system, b, scale, loss_tol, max_evals=50):
    """the same schedule on trajectory b alone: [theta | x0[idx]]"""
    from pdp_amd.irl import LMLoop
    c, sid = lm_data(system), sg.oracle(system)
    p, idx = sid.p, c["idx"]

    def evaluate(v):
        ini = c["ini_state"][b:b + 1].copy()
        ini[0, idx] = v[p:]
        loss, grad, G = reference_rows(sid, c["inputs"][b:b + 1], c["states"][b:b + 1], v[:p], idx, ini, True)
        return loss[0], grad[0], G[0]
    return LMLoop(evaluate, np.concatenate([c["theta_ref"] * scale, c["ini_state"][b, idx]])).run(max_evals=max_evals, loss_tol=loss_tol)
