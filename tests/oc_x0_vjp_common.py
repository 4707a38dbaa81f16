"""Shared by tests/test_oc_x0_vjp_host.py and tests/test_gpu_oc_x0_vjp.py (in-process and in its child processes): the gradient of a loss on the OC solution with
respect to the INITIAL STATE (pdp_oc_sens_out.grad_x0).

The reference is not the kernel's method: OCSysOracle.getAuxSys at (x, u, lam, theta), E / Hxe / Hue / hxe padded with n zero columns, oracle.pdp_oracle.lqr_solver
from X_0 = [0 | I] - FORWARD sensitivities by the reference's own formulas with its explicit inverses - and the last n columns contracted with the cotangents.
`adjoint_sweep` restates the kernel's recursion in numpy with gains it forms itself from the same matrices; tests/test_oc_x0_vjp_host.py holds it to the reference at
1e-11 on every case the GPU tests use, a tenth of their tolerance.  The inputs are those of oc_vjp_common.make_inputs."""
import functools

import numpy as np

import oc_vjp_common as c

ZOO = ("pendulum", "cartpole", "robotarm", "quadrotor", "rocket")
# oc_x0_vjp_rows by the rule of csrc/pdp_sweep_pool.h, worked out by hand: stride = (SOLF_NVAR + n m + n + m) | 1 with SOLF_NVAR = 3, 6, 10, 36, 42 variable
# entries of (F, G) -> 9, 15, 25, 105, 97; rows = min(64, max(4, 2400 // stride))
ROWS = {"pendulum": 64, "cartpole": 64, "robotarm": 64, "quadrotor": 22, "rocket": 24}
T_MAIN, B_MAIN = 20, 3
EDGE_SYSTEMS, B_EDGE = ("pendulum", "quadrotor"), 2
# make_inputs' seed is 7 but for the quadrotor at T = 2 R + 1 = 45: over 45 open-loop steps its sensitivities grow to 1e3 and, of seeds 1 .. 12, the reference agrees with
# ITSELF (the theta columns of the padded solve against the unpadded one, another matrix width) to 2e-11 at seed 7 and to 1e-13 at seed 3; seed 3 it is
SEEDS = {("quadrotor", 45): 3}


def inputs(system, B, T):
    return c.make_inputs(system, B, T, SEEDS.get((system, T), 7))


def edge_horizons(system):
    R = ROWS[system]
    return (1, R - 1, R, R + 1, 2 * R + 1)


def reference_cases():
    """(system, B, T, per-sample theta) of every reference the GPU tests compare with"""
    main = [(s, B_MAIN, T_MAIN, ps) for s in c.DIMS for ps in (False, True)]
    return main + [(s, B_EDGE, T, False) for s in EDGE_SYSTEMS for T in edge_horizons(s)]


@functools.lru_cache(maxsize=None)
def oracle_oc(system):
    from oracle import models, pdp_oracle as po
    st = models.IRL_SETUP[system]
    return po.make_oc(models.REGISTRY[system](**st["kwargs"]), st["dt"])


def forward_sensitivities(oc, aux, T):
    """dx_t/dx_0 [T+1, n, n] and du_t/dx_0 [T, m, n] of the auxiliary LQ system `aux` by the reference's lqr_solver: the initial state as n further parameters.  The
    first p columns are the reference's dx/dtheta, du/dtheta: asserted against the unpadded solve - the same formulas column by column, in matrix products of another
    width, so equal up to the reference's own rounding, which has to stay below 1e-12 of the largest entry: a tenth of the bound the reference is then used at."""
    from oracle import pdp_oracle as po
    n, p = oc.n, oc.p
    wide = lambda mats: [np.concatenate([M, np.zeros((M.shape[0], n))], axis=1) for M in mats]
    sol = po.lqr_solver(aux["dynF"], aux["dynG"], wide(aux["dynE"]), aux["Hxx"], aux["Huu"], aux["Hxu"], wide(aux["Hxe"]), wide(aux["Hue"]), aux["hxx"], wide(aux["hxe"]),
                        np.concatenate([np.zeros((n, p)), np.eye(n)], axis=1), T)
    X, U = np.stack(sol["state_traj_opt"]), np.stack(sol["control_traj_opt"])
    plain = po.lqr_from_aux(aux, n, p, T)
    Xp, Up = np.stack(plain["state_traj_opt"]), np.stack(plain["control_traj_opt"])
    assert np.abs(X[:, :, :p] - Xp).max() <= 1e-12 * np.abs(Xp).max() and np.abs(U[:, :, :p] - Up).max() <= 1e-12 * np.abs(Up).max()
    return X[:, :, p:], U[:, :, p:]


def reference_grad_x0(oc, x, u, lam, theta, gx, gu, aux=None):
    """dL/dx_0 [n] of one trajectory: the reference's forward sensitivities contracted with the cotangents gx [T+1, n], gu [T, m] (row 0 of gx included: X_0 = I)"""
    aux = oc.getAuxSys(x, u, lam, theta) if aux is None else aux
    Xx, Ux = forward_sensitivities(oc, aux, u.shape[0])
    return np.einsum("ti,tik->k", gx, Xx) + np.einsum("ti,tik->k", gu, Ux)


def adjoint_sweep(aux, gx, gu):
    """The kernel's recursion in numpy: mu_T = gx_T; v_t = gu_t + G_t' mu_{t+1}, mu_t = gx_t + F_t' mu_{t+1} - K_t' v_t; returns mu_0.  The gains are formed here, by
    the textbook Riccati recursion K_t = (Huu + G' P G)^-1 (Hxu' + G' P F), P_t = Hxx + F' P F - (Hxu + F' P G) K_t from P_T = hxx (u = -K x), not the reference's
    (I + P R)^-1 form."""
    T = len(aux["dynF"])
    P, mu = aux["hxx"][0], np.array(gx[T], dtype=float)
    for t in range(T - 1, -1, -1):
        F, G, Hxx, Hxu, Huu = (aux[k][t] for k in ("dynF", "dynG", "Hxx", "Hxu", "Huu"))
        K = np.linalg.solve(Huu + G.T @ P @ G, Hxu.T + G.T @ P @ F)
        v = gu[t] + G.T @ mu
        mu = gx[t] + F.T @ mu - K.T @ v
        P = Hxx + F.T @ P @ F - (Hxu + F.T @ P @ G) @ K
    return mu


@functools.lru_cache(maxsize=None)
def reference_case(system, B, T, per_sample):
    """reference and restatement of a case of reference_cases() on make_inputs' rollouts and cotangents: dict(ref [B, n], sweep [B, n]); computed once per process"""
    oc, inp = oracle_oc(system), inputs(system, B, T)
    ref, sweep = [], []
    for i in range(B):
        th = inp["theta_b"][i] if per_sample else inp["theta"]
        x = oc.rollout(inp["x0"][i], inp["u"][i], th)
        lam = oc.costate(x, inp["u"][i], th)
        aux = oc.getAuxSys(x, inp["u"][i], lam, th)
        ref.append(reference_grad_x0(oc, x, inp["u"][i], lam, th, inp["gx"][i], inp["gu"][i], aux=aux))
        sweep.append(adjoint_sweep(aux, inp["gx"][i], inp["gu"][i]))
    out = dict(ref=np.stack(ref), sweep=np.stack(sweep))
    for v in out.values():
        v.setflags(write=False)
    return out


def evaluate(mdl, inp, per_sample=False, given=False):
    """One case on the GPU: the cotangent unit without and with want_ini on the same inputs (given: on the default call's (x, lam), PDP_OC_GIVEN_TRAJ).  numpy arrays."""
    from pdp_amd import runtime as rt
    th = inp["theta_b"] if per_sample else inp["theta"]
    u, gx, gu = rt.dev(inp["u"]), rt.dev(inp["gx"]), rt.dev(inp["gu"])
    if given:
        d0 = mdl.oc_pdp_grad(u, th, rt.dev(inp["demo_x"]), rt.dev(inp["demo_u"]), x0=inp["x0"])
    traj = (lambda: dict(x=d0["x"].clone(), lam=d0["lam"].clone())) if given else (lambda: dict(x0=inp["x0"]))
    a = mdl.oc_pdp_vjp(u, th, gx, gu, **traj())
    b = mdl.oc_pdp_vjp(u, th, gx, gu, want_ini=True, **traj())
    npy = lambda t: t.detach().cpu().numpy()
    return dict(grad_x0=npy(b["grad_x0"]), grad=npy(b["grad"]), x=npy(b["x"]), lam=npy(b["lam"]), status=npy(b["status"]),
                grad_plain=npy(a["grad"]), x_plain=npy(a["x"]), lam_plain=npy(a["lam"]), status_plain=npy(a["status"]))


def wide_auxvar_oc():
    """n = 6, m = 2, p = 16 (m + p > 16: the fused kernels answer PDP_E_SIZE) - the model of tests/test_gpu_oc_vjp.py's _wide_auxvar_oc, rebuilt: same seed, same draws"""
    from pdp_amd import PDP
    from pdp_amd.sx import SX, mtimes
    rng = np.random.default_rng(12)
    n, m, dt = 6, 2, 0.1
    A, Bm = rng.standard_normal((n, n)) - np.eye(n), rng.standard_normal((n, m))
    X, U, w = SX.sym("x", n), SX.sym("u", m), SX.sym("w", 16)
    f = X + dt * (mtimes(SX(A), X) + mtimes(SX(Bm), U) + w[8:14] * X * X)
    cost = sum(w[i] * X[i] * X[i] for i in range(n)) + w[6] * U[0] * U[0] + w[7] * U[1] * U[1] + w[14] * X[0] * U[0] + w[15] * X[1] * U[1]
    oc = PDP.OCSys("wide auxvar")
    oc.setAuxvarVariable(w)
    oc.setStateVariable(X)
    oc.setControlVariable(U)
    oc.setDyn(f)
    oc.setPathCost(cost)
    oc.setFinalCost(sum(w[i] * X[i] * X[i] for i in range(n)))
    th = np.concatenate([1 + rng.random(8), 0.05 * rng.standard_normal(6), 0.1 * rng.standard_normal(2)])
    return oc, th, rng
