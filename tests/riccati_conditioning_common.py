"""Shared by tests/test_riccati_conditioning_inputs.py (CPU) and tests/test_gpu_riccati_conditioning.py (GPU, in-process and in its child processes): LQR problems
whose m x m matrix Quu = Huu + G'PG is ill-conditioned, and the two CPU evaluations they are judged by.

Recipe: the one of tests/test_gpu_lqr.py::test_lqr_matches_oracle_seeded with three changes - G_t = g_amplitude(n, m) * outer(randn(n), ones(m)) has rank 1 (m actuators pushing the
state along one direction; `near`: + 0.01 * randn(n, m)), Huu_t = s * spd(m, 0.5) (cheap controls), and Hxu, Hue are scaled by sqrt(s), s so that the stage cost stays
convex in (x, u) for every s.  Then Quu has one eigenvalue of order 1 and m - 1 of order s.

One batch holds the whole sweep s = SCALES, sample b drawn from seed + b: samples on either side of a kernel's conditioning guard share a workgroup, and B = 5 leaves the
last workgroup of the four-per-workgroup kernels ragged."""
import functools

import numpy as np

SCALES = (1.0, 1e-2, 1e-3, 1e-4, 1e-5)
T = 8
TOL = 1e-10                  # GPU vs restatement on identical inputs
REF_CAP = 1e-8               # the reference order's own fp64 error must stay below this for the comparison to mean anything
KEYS = ("F", "G", "E", "Hxx", "Huu", "Hxu", "Hxe", "Hue")

# (n, m, p) of every LQR route the GPU tests take, by kernel
STREAM_SHAPES = [(6, 4, 5), (6, 3, 5), (6, 2, 5), (13, 4, 9)]
ONE_WAVE_TWO_TILE_SHAPES = [(6, 4, 13), (6, 3, 14)]
ONE_WAVE_ONE_TILE_SHAPE = (6, 4, 5)
SMALL_SHAPES = [(4, 4, 5), (4, 3, 5), (4, 2, 5)]
GENERIC_SHAPES = [(6, 6, 5), (20, 4, 5)]
NEAR_SHAPE = (6, 4, 5)
SEED = 3
# (n, m, p, near): every distinct input of the GPU LQR tests
LQR_INPUTS = sorted({(n, m, p, False) for n, m, p in STREAM_SHAPES + ONE_WAVE_TWO_TILE_SHAPES + [ONE_WAVE_ONE_TILE_SHAPE] + SMALL_SHAPES + GENERIC_SHAPES}
                    | {NEAR_SHAPE + (True,)})


def g_amplitude(n, m):
    """0.3 (the amplitude of the well-conditioned recipe) up to n m = 8, then falling as 1 / (n m).  The large eigenvalue of Quu is about m g'Pg ~ n m amplitude^2, and
    the reference order's OWN error (it inverts I + P G Huu^-1 G') grows with it steeply: at 0.3 throughout, s = 1e-5 put the reference at 1e-8 .. 4e-7 for n m >= 12,
    above REF_CAP (tests/test_riccati_conditioning_inputs.py).  With this rule every input stays below the cap, and the guard quantity of the 4 x 4 fast path still
    falls to ~1e-6 along the sweep, far below where its error passes 1e-10 (probes/riccati_guard_sweep.py)."""
    return 0.3 * min(1.0, 8.0 / (n * m))


def lqr_problem(n, m, p, T, s, seed, near=False):
    """one trajectory: dict of F, G, E, Hxx, Huu, Hxu, Hxe, Hue [T, r, c], hxx [n, n], hxe [n, p], X0 [n, p]"""
    rng = np.random.default_rng(seed)

    def spd(k, scale):
        A = rng.standard_normal((k, k))
        return scale * (A @ A.T / k + 0.5 * np.eye(k))
    F = np.eye(n) + 0.1 * rng.standard_normal((T, n, n))
    G = g_amplitude(n, m) * rng.standard_normal((T, n))[:, :, None] * np.ones((1, 1, m))
    if near:
        G = G + 0.01 * rng.standard_normal((T, n, m))
    E = 0.1 * rng.standard_normal((T, n, p))
    Hxx = np.stack([spd(n, 1.0) for _ in range(T)])
    Huu = np.stack([spd(m, 0.5) for _ in range(T)]) * s
    Hxu = 0.05 * np.sqrt(s) * rng.standard_normal((T, n, m))
    Hxe = 0.2 * rng.standard_normal((T, n, p))
    Hue = 0.2 * s * rng.standard_normal((T, m, p))
    hxx = spd(n, 1.0)
    hxe = 0.2 * rng.standard_normal((n, p))
    X0 = rng.standard_normal((n, p))
    return dict(F=F, G=G, E=E, Hxx=Hxx, Huu=Huu, Hxu=Hxu, Hxe=Hxe, Hue=Hue, hxx=hxx, hxe=hxe, X0=X0)


def lqr_batch(n, m, p, near=False, seed=SEED, scales=SCALES, T=T):
    """the sweep as one batch: dict of [B, ...] arrays, sample b = lqr_problem(..., scales[b], seed + b)"""
    probs = [lqr_problem(n, m, p, T, s, seed + b, near) for b, s in enumerate(scales)]
    return {k: np.stack([q[k] for q in probs]) for k in probs[0]}


def sample(batch, b):
    return {k: v[b] for k, v in batch.items()}


def _args(pr):
    return [list(pr[k]) for k in KEYS] + [[pr["hxx"]], [pr["hxe"]], pr["X0"], pr["F"].shape[0]]


def solve_mp(pr):
    """(X, U, Lam): the reference's formulas (PDP.py:557-608) in 40-digit arithmetic"""
    from oracle import pdp_oracle as po
    sol = po.lqr_solver_mp(*_args(pr))
    return np.stack(sol["state_traj_opt"]), np.stack(sol["control_traj_opt"]), np.stack(sol["costate_traj_opt"])


def solve_ref(pr):
    """(X, U, Lam): the same formulas in the reference's fp64 order of operations"""
    from oracle import pdp_oracle as po
    sol = po.lqr_solver(*_args(pr))
    return np.stack(sol["state_traj_opt"]), np.stack(sol["control_traj_opt"]), np.stack(sol["costate_traj_opt"])


def rel(a, exact):
    return float(np.abs(np.asarray(a) - exact).max() / np.abs(exact).max())


@functools.lru_cache(maxsize=None)
def lqr_case(n, m, p, near=False):
    """the batch, its 40-digit solution per sample and the reference order's error per sample and quantity - computed once per process"""
    batch = lqr_batch(n, m, p, near)
    exact, ref_err = [], []
    for b in range(len(SCALES)):
        pr = sample(batch, b)
        ex = solve_mp(pr)
        exact.append(ex)
        ref_err.append(tuple(rel(r, e) for r, e in zip(solve_ref(pr), ex)))
    return batch, exact, ref_err


def bounds(ref_err):
    """per quantity: max(1e-10, the reference order's own fp64 error on the same input) - no fp64 evaluation can be asked to beat the reference's order by construction"""
    return tuple(max(TOL, e) for e in ref_err)


def check_lqr(margins, tag, ref_err, exact, got):
    """X, U, Lam of every sample of one batch against the 40-digit solution; got = (X, U, Lam or None) as [B, ...] arrays"""
    for b, s in enumerate(SCALES):
        bd = bounds(ref_err[b])
        for name, g, e, bound in zip(("X", "U", "Lam"), got, exact[b], bd):
            if g is not None:
                margins.check("ill-conditioned Quu, %s, s=%g: %s vs the 40-digit solution" % (tag, s, name), rel(g[b], e), bound)


# ---- the OC side: one linear-quadratic user model whose control weight is an auxiliary parameter -------------------------------------------------------
# x+ = x + dt (A x + b sum(u) + theta_dyn x),  c = w_u u'u + sum_i w_i x_i^2,  h = sum_i w_i x_i^2,  auxvar = [theta_dyn, w_u, w_0 .. w_{n-1}]
# G = dt b 1' has rank 1 and Huu = 2 w_u I: per-sample theta sweeps w_u = SCALES in one batch without a recompile.  n = 6: runner / evaluator kernel of the
# fused unit, multiple-shooting solver's augmented step; n = 4: the one-wave / small-system kernels.
OC_M, OC_DT = 4, 0.1
OC_SIZES = (6, 4)


def oc_constants(n):
    rng = np.random.default_rng(20 + n)
    return rng.standard_normal((n, n)) - np.eye(n), np.outer(0.3 * rng.standard_normal(n), np.ones(OC_M))


def oc_inputs(n, seed=SEED):
    """per-sample theta [B, n + 2] with w_u = SCALES, initial states, an off-optimal control trajectory, standard-normal cotangents"""
    rng = np.random.default_rng(seed + 100 * n)
    B = len(SCALES)
    theta = np.concatenate([0.1 * rng.standard_normal((B, 1)), np.asarray(SCALES)[:, None], 1 + rng.random((B, n))], axis=1)
    return dict(theta=theta, x0=0.5 * rng.standard_normal((B, n)), u=0.3 * rng.standard_normal((B, T, OC_M)),
                gx=rng.standard_normal((B, T + 1, n)), gu=rng.standard_normal((B, T, OC_M)))


def oc_model_gpu(n):
    """the model through the class surface (PDP.OCSys on the product's symbolic engine)"""
    from pdp_amd import PDP
    from pdp_amd.sx import SX, mtimes
    A, Bm = oc_constants(n)
    X, U, w = SX.sym("x", n), SX.sym("u", OC_M), SX.sym("w", n + 2)
    oc = PDP.OCSys("cheap redundant actuators n%d" % n)
    oc.setAuxvarVariable(w)
    oc.setStateVariable(X)
    oc.setControlVariable(U)
    oc.setDyn(X + OC_DT * (mtimes(SX(A), X) + mtimes(SX(Bm), U) + w[0] * X))
    oc.setPathCost(w[1] * sum(U[i] * U[i] for i in range(OC_M)) + sum(w[2 + i] * X[i] * X[i] for i in range(n)))
    oc.setFinalCost(sum(w[2 + i] * X[i] * X[i] for i in range(n)))
    return oc


@functools.lru_cache(maxsize=None)
def oc_model_oracle(n):
    """the same model on sympy (oracle.pdp_oracle.OCSysOracle): the CPU route to the same auxiliary systems"""
    import sympy as sp
    from oracle import pdp_oracle as po
    A, Bm = oc_constants(n)
    X, U, w = sp.Matrix(sp.symbols("x0:%d" % n, real=True)), sp.Matrix(sp.symbols("u0:%d" % OC_M, real=True)), sp.Matrix(sp.symbols("w0:%d" % (n + 2), real=True))
    state_cost = sum(w[2 + i] * X[i] ** 2 for i in range(n))
    return po.OCSysOracle(X, U, w, X + OC_DT * (sp.Matrix(A) * X + sp.Matrix(Bm) * U + w[0] * X), w[1] * (U.T * U)[0, 0] + state_cost, state_cost)


def oc_aux_oracle(n, b):
    """auxiliary system of sample b along its rolled-out trajectory, by the oracle"""
    oc, inp = oc_model_oracle(n), oc_inputs(n)
    xs = oc.rollout(inp["x0"][b], inp["u"][b], inp["theta"][b])
    lam = oc.costate(xs, inp["u"][b], inp["theta"][b])
    return oc.getAuxSys(xs, inp["u"][b], lam, inp["theta"][b])


def aux_problem(aux, n, p):
    """an auxiliary system (lists or [T, r, c] arrays, the keys of getAuxSys) as a problem of solve_mp / solve_ref: X0 = 0"""
    names = dict(F="dynF", G="dynG", E="dynE", Hxx="Hxx", Huu="Huu", Hxu="Hxu", Hxe="Hxe", Hue="Hue")
    pr = {k: np.stack([np.asarray(a, float) for a in aux[v]]) for k, v in names.items()}
    pr.update(hxx=np.asarray(aux["hxx"], float).reshape(n, n), hxe=np.asarray(aux["hxe"], float).reshape(n, p), X0=np.zeros((n, p)))
    return pr


def oc_lq_problem(n, b):
    """the OC problem of sample b itself: linear-quadratic, so its optimum from x0 is ONE solve of the LQR formulas with a single column X0 = x0 and no affine terms"""
    A, Bm = oc_constants(n)
    inp = oc_inputs(n)
    th = inp["theta"][b]
    rep = lambda M: np.stack(T * [M])
    W2 = 2.0 * np.diag(th[2:])
    return dict(F=rep(np.eye(n) + OC_DT * (A + th[0] * np.eye(n))), G=rep(OC_DT * Bm), E=np.zeros((T, n, 1)), Hxx=rep(W2), Huu=rep(2.0 * th[1] * np.eye(OC_M)),
                Hxu=np.zeros((T, n, OC_M)), Hxe=np.zeros((T, n, 1)), Hue=np.zeros((T, OC_M, 1)), hxx=W2, hxe=np.zeros((n, 1)), X0=inp["x0"][b][:, None])


@functools.lru_cache(maxsize=None)
def oc_lq_case(n):
    """per sample: the 40-digit optimum (X, U, Lam) and the reference order's error on the same problem"""
    exact, ref_err = [], []
    for b in range(len(SCALES)):
        pr = oc_lq_problem(n, b)
        ex = solve_mp(pr)
        exact.append(ex)
        ref_err.append(tuple(rel(r, e) for r, e in zip(solve_ref(pr), ex)))
    return exact, ref_err


def contract(gx, gu, X, U):
    """sum_t gx_t' X_t + gu_t' U_t  (X_0 = 0: gx_0 does not enter)"""
    return np.einsum("ti,tip->p", gx[1:], X[1:]) + np.einsum("ti,tip->p", gu, U)
