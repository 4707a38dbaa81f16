"""Shared by tests/test_tile_edge_inputs.py (CPU) and tests/test_gpu_tile_edge.py (GPU, in-process and in its child processes): three nonlinear OC models at the far
end of the size range the fused OC unit (pdp_oc_pdp_grad*_batched: n <= 16, m <= 4, m + p <= 16) and the multiple-shooting solver (pdp_oc_solve_ms_batched: n <= 16,
m <= 4) advertise, their inputs, and the kernels' layout rules restated from the code generator's counts.

    name   n  m   p   what it reaches
    E16   16  4  12   Ms2Layout::AUG == false (the solver's separate W recursion: n = 16 only), no padding row in any state tile, m + p = 16, M = 4
    E15   15  3  13   NA = NX + 1 = 16 (a full augmented tile), m + p = 16, M = 3, odd n
    E5     5  1  15   the smallest size past the small-system kernels (NX > 4), M = 1 under the pair kernels, m + p = 16

Each is a chain of n // 2 masses with cubic springs (states: positions q, velocities v and, for odd n, one first-order state z), actuators on the first m even
masses, dt = 0.05:
    q_i+ = q_i + dt v_i,   v_i+ = v_i + dt (k (q_{i-1} - 2 q_i + q_{i+1}) - d v_i - c q_i^3 [+ u_{i/2}]),   z+ = z + dt (-w_1 z + q_0 q_1)
    path cost = sum_i w_i q_i^2 + sum_j w_{nm+j} e_j + w_u u'u + 0.3 v'v,   final cost = sum_i w_i q_i^2
    auxvar = [k, d, c, w_0 .. w_{p-5}, w_u]
where the weights beyond one per position go to further quadratic terms e_j of the state, in this order: 0.1 v_i^2, 0.1 z^2, 0.1 x_i x_j (i < j over the whole state).
Every parameter enters the dynamics or the cost, so no column of dx/dtheta is identically zero (tests/test_tile_edge_inputs.py checks it).  The equations are written
once against a list of scalar symbols, so the product (pdp_amd.sx) and the oracle (sympy) are given the same ones.  Exactly three models: each costs about a minute
of hipcc on its first use."""
import functools

import numpy as np

MODELS = {"E16": (16, 4, 12), "E15": (15, 3, 13), "E5": (5, 1, 15)}
DT = 0.05
TOL = 1e-10                  # GPU vs restatement on identical inputs, relative to the largest entry, per sample
REF_CAP = 1e-12              # the reference order's own fp64 error (against 40-digit arithmetic) must stay below this for the comparison to mean anything
B_UNIT = 5                   # the last workgroup of the two- and four-per-workgroup layouts is ragged
SHORT_HORIZONS = (1, 7)      # and ROWS + 6, ROWS + 7 of the model (unit_horizons): two backward chunks, of equal and of unequal length


# ---- the equations ----------------------------------------------------------------------------------------------------------------------------------------
def _symbols(name, lib):
    n, m, p = MODELS[name]
    if lib == "sx":
        from pdp_amd.sx import SX
        X, U, w = SX.sym("x", n), SX.sym("u", m), SX.sym("w", p)
        return [X[i] for i in range(n)], [U[i] for i in range(m)], [w[i] for i in range(p)]
    import sympy as sp
    return tuple(list(sp.symbols("%s0:%d" % (s, k), real=True)) for s, k in (("x", n), ("u", m), ("w", p)))


def equations(name, lib, theta=None):
    """(state, control, auxvar, dynamics, path cost, final cost) as lists of scalars / scalars of the symbolic library `lib` ("sx": pdp_amd.sx, else sympy).
    theta [p] (tests/cp_edge_common.py: ControlPlanning has no auxvar): the parameters are replaced by these doubles - pdp_amd.sx.substitute / sympy's .subs on the
    finished expressions, so both libraries are given the same numbers in the same places - and the auxvar comes back as an empty list"""
    if theta is not None:
        xs, us, ws, f, path, final = equations(name, lib)
        vals = [float(v) for v in theta]
        assert len(vals) == len(ws)
        if lib == "sx":
            from pdp_amd import sx
            old, new = sx.vertcat(*ws), sx.SX(np.array(vals).reshape(-1, 1))
            sub = lambda e: sx.substitute(e, old, new)
            return xs, us, [], [sub(fi) for fi in f], sub(path), sub(final)
        import sympy as sp
        rep = dict(zip(ws, (sp.Float(v, 40) for v in vals)))              # the double itself, carried at 40 digits: products of constants are not rounded to 53 bits
        return xs, us, [], [fi.subs(rep) for fi in f], path.subs(rep), final.subs(rep)
    n, m, p = MODELS[name]
    xs, us, ws = _symbols(name, lib)
    nm, odd, nw = n // 2, n % 2 == 1, p - 4
    assert nw >= nm and nm >= 2
    q, v = xs[:nm], xs[nm:2 * nm]
    k, d, c3, wq, wu = ws[0], ws[1], ws[2], ws[3:3 + nw], ws[3 + nw]
    acc = []
    for i in range(nm):
        left = q[i - 1] if i > 0 else 0.0
        right = q[i + 1] if i + 1 < nm else 0.0
        a = k * (left - 2 * q[i] + right) - d * v[i] - c3 * q[i] * q[i] * q[i]
        if i % 2 == 0 and i // 2 < m:
            a = a + us[i // 2]
        acc.append(a)
    f = [q[i] + DT * v[i] for i in range(nm)] + [v[i] + DT * acc[i] for i in range(nm)]
    if odd:
        f.append(xs[2 * nm] + DT * (q[0] * q[1] - wq[1] * xs[2 * nm]))
    extras = [0.1 * vi * vi for vi in v] + ([0.1 * xs[2 * nm] * xs[2 * nm]] if odd else []) + [0.1 * xs[i] * xs[j] for i in range(n) for j in range(i + 1, n)]
    add = lambda terms: functools.reduce(lambda a, b: a + b, terms)
    final = add([wq[i] * q[i] * q[i] for i in range(nm)])
    path = add([wq[i] * q[i] * q[i] for i in range(nm)] + [wq[nm + j] * extras[j] for j in range(nw - nm)] + [wu * add([u * u for u in us])] + [0.3 * add([vi * vi for vi in v])])
    return xs, us, ws, f, path, final


def model_gpu(name):
    """the model through the class surface (PDP.OCSys on the product's symbolic engine); .model() generates and compiles it on first use"""
    from pdp_amd import PDP
    from pdp_amd.sx import vertcat
    xs, us, ws, f, path, final = equations(name, "sx")
    oc = PDP.OCSys("tile edge " + name)
    oc.setAuxvarVariable(vertcat(*ws))
    oc.setStateVariable(vertcat(*xs))
    oc.setControlVariable(vertcat(*us))
    oc.setDyn(vertcat(*f))
    oc.setPathCost(path)
    oc.setFinalCost(final)
    return oc


@functools.lru_cache(maxsize=None)
def model_oracle(name):
    """the same equations on sympy (oracle.pdp_oracle.OCSysOracle)"""
    import sympy as sp
    from oracle import pdp_oracle as po
    xs, us, ws, f, path, final = equations(name, "sympy")
    return po.OCSysOracle(sp.Matrix(xs), sp.Matrix(us), list(ws), sp.Matrix(f), path, final)


@functools.lru_cache(maxsize=None)
def generated_info(name):
    """what the code generator says of the model (sizes, entries and constants per matrix group) - no compiling"""
    from pdp_amd import PDP, codegen
    oc = model_gpu(name)
    pb = codegen.Problem(codegen.KIND_OC, oc.state, oc.control, oc.dyn, oc.auxvar, oc.path_cost, oc.final_cost, label=PDP._label(oc.project_name))
    return codegen.generate(pb)[1]


# ---- the kernels' layout rules, restated (csrc/pdp_fused3_kernels.h Fused3Layout / fused3_ok, csrc/pdp_ocsolve2_kernels.h Ms2Layout / ms2_ok,
#      csrc/pdp_model_kernels.h FusedLayout / fused_lds_bytes, csrc/pdp_launch.h traj_per_workgroup) ----------------------------------------------------------
RICCATI_SCRATCH = 272 + 272 + 64
SLICE = 160 * 1024 // 8 // 4


def fused3_layout(info, xw=0):
    """xw: the extra words of a forward row (Fused3Layout<Mdl, XW>: n + m scales in the weighted mode, with them dlT is n words longer); 0 in every other mode"""
    n, m, p, nv, nc = info["n"], info["m"], info["p"], info["nvar"], info["nconst"]
    npc = max(1, info["npc"])
    NA, NB = nv["patha"], max(nv["pathb"], 16)
    BSTRIDE = (NA + NB + 1 + nc["patha"] + nc["pathb"]) | 1
    FSTRIDE = (nv["fwd"] + n + m + xw + 1 + nc["fwd"]) | 1
    PAR = RICCATI_SCRATCH + 1 + nc["fin"] + nv["fin"]
    POOL = PAR + p + npc + n + (n if xw else 0) + 8
    BUF = (SLICE - POOL) // 2
    return dict(BSTRIDE=BSTRIDE, FSTRIDE=FSTRIDE, BUF=BUF, ROWS=min(64, BUF // BSTRIDE), ROWSF=min(64, BUF // FSTRIDE))


def fused3_ok(info, T, xw=0):
    L = fused3_layout(info, xw)
    return info["n"] > 4 and L["ROWS"] >= 4 and L["ROWSF"] >= 4 and (T + 1) * info["n"] + T * info["m"] <= 2 * L["BUF"]


def fused_accepts(info, T, xw=0):
    """pdp_oc_pdp_grad_batched does not answer PDP_E_SIZE: one tile per matrix, one [control | parameter] tile, the one-wave kernel's LDS within a CU's 160 KB
    (fused_lds_bytes<Mdl, XW>: xw further words per forward row and, with them, n behind dlT)"""
    n, m, p, nv, nc = info["n"], info["m"], info["p"], info["nvar"], info["nconst"]
    NC = 1 + max(nc["patha"] + nc["pathb"], nc["fwd"], nc["fin"])
    pool = max(info["chunk"] * max((nv["patha"] + nv["pathb"] + n) | 1, (nv["fwd"] + n + m + xw) | 1), nv["fin"] + 1, (T + 1) * n + T * m)
    return n <= 16 and m <= 4 and m + p <= 16 and 8 * (RICCATI_SCRATCH + NC + pool + n + (n if xw else 0) + p + max(1, info["npc"]) + 8) <= 160 * 1024


def ms2_layout(info):
    n, m, p, nv, nc = info["n"], info["m"], info["p"], info["nvar"], info["nconst"]
    npc = max(1, info["npc"])
    BSTRIDE = (nv["sol"] + 2 * n + m + 1 + nc["sol"] + 1) | 1
    FSTRIDE = (nv["solf"] + 2 * n + m + 1 + nc["solf"] + 1) | 1
    NCFIN = 1 + nc["fin"]
    PAR = RICCATI_SCRATCH + NCFIN + nv["fin"]
    CTL = (PAR + p + npc + n + 1) & ~1
    BUF = (SLICE - (CTL + 40)) // 2
    return dict(AUG=4 < n < 16, NA=n + 1 if 4 < n < 16 else n, BSTRIDE=BSTRIDE, FSTRIDE=FSTRIDE, BUF=BUF, ROWS=min(64, BUF // BSTRIDE), ROWSF=min(64, BUF // FSTRIDE),
                fits=nv["fin"] + NCFIN + PAR <= SLICE)


def ms2_ok(info):
    L = ms2_layout(info)
    return info["n"] <= 16 and info["m"] <= 4 and L["ROWS"] >= 4 and L["ROWSF"] >= 4 and L["fits"]


def traj_per_workgroup(B, cus, max_tpw=4):
    return 1 if B <= cus else (2 if (B <= 2 * cus or max_tpw == 2) else 4)


def backward_chunks(info, T):
    """lengths of the fused unit's backward chunks, last time steps first (oc_pdp_fused3_kernel: nchunk = ceil(T / ROWS) chunks of ceil(T / nchunk) steps, the one at t = 0 short)"""
    rows = fused3_layout(info)["ROWS"]
    nchunk = -(-T // rows)
    ch = -(-T // nchunk)
    return [min(ch, T - k * ch) for k in range(nchunk - 1, -1, -1)]


def unit_horizons(info):
    """T = 1, T = 7 (inside one chunk), ROWS + 6 and ROWS + 7: two backward chunks each.  ROWS is even for all three models (22, 22, 42), so ROWS + 6 splits into equal
    halves; ROWS + 7 is there for the unequal pair"""
    rows = fused3_layout(info)["ROWS"]
    return SHORT_HORIZONS + (rows + 6, rows + 7)


# ---- inputs of the fused unit -------------------------------------------------------------------------------------------------------------------------------
def theta_nominal(name, rng=None):
    """stiffness 2, damping 0.3, cubic coefficient 0.3, weights in [1, 2), control weight 0.2"""
    p = MODELS[name][2]
    rng = np.random.default_rng(100 + MODELS[name][0]) if rng is None else rng
    return np.concatenate([[2.0, 0.3, 0.3], 1.0 + rng.random(p - 4), [0.2]])


def unit_inputs(name, T, seed=None):
    """B = 5: x0 ~ 0.5 N(0, 1), controls ~ 0.3 N(0, 1), standard-normal demonstrations and cotangents, one shared and one per-sample parameter (5 % around it)"""
    n, m, p = MODELS[name]
    rng = np.random.default_rng(1000 * n + T if seed is None else seed)
    B = B_UNIT
    theta = theta_nominal(name)
    return dict(name=name, B=B, T=T, theta=theta, theta_b=theta[None, :] * (1 + 0.05 * rng.standard_normal((B, p))), x0=0.5 * rng.standard_normal((B, n)),
                u=0.3 * rng.standard_normal((B, T, m)), demo_x=rng.standard_normal((B, T + 1, n)), demo_u=rng.standard_normal((B, T, m)),
                gx=rng.standard_normal((B, T + 1, n)), gu=rng.standard_normal((B, T, m)))


def theta_of(inp, per_sample, b):
    return inp["theta_b"][b] if per_sample else inp["theta"]


@functools.lru_cache(maxsize=None)
def unit_oracle(name, T, per_sample, b):
    """oracle.pdp_oc_unit of sample b (rollout from x0): dict with state_traj, costate_traj, aux, lqr (X, U, PP, WW), loss, grad - computed once per process, not modified"""
    from oracle import pdp_oracle as po
    inp = unit_inputs(name, T)
    return po.pdp_oc_unit(model_oracle(name), inp["x0"][b], inp["u"][b], theta_of(inp, per_sample, b), inp["demo_x"][b], inp["demo_u"][b])


def unit_exact(name, T, per_sample, b):
    """(X, U) of the same auxiliary system by the reference's formulas in 40-digit arithmetic"""
    from oracle import pdp_oracle as po
    n, m, p = MODELS[name]
    aux = unit_oracle(name, T, per_sample, b)["aux"]
    ex = po.lqr_solver_mp(aux["dynF"], aux["dynG"], aux["dynE"], aux["Hxx"], aux["Huu"], aux["Hxu"], aux["Hxe"], aux["Hue"], aux["hxx"], aux["hxe"], np.zeros((n, p)), T)
    return np.stack(ex["state_traj_opt"]), np.stack(ex["control_traj_opt"])


def rel(a, b):
    """max|a - b| / max|b|"""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.abs(a - b).max() / np.abs(b).max())


# ---- inputs of the solver -----------------------------------------------------------------------------------------------------------------------------------
# (a) positive weights, far initial states: step lengths below 1 in the first iterations; (b) one position weight = -2, cheap controls: inertia corrections.
# The recipe of tests/test_gpu_edge_cases.py::test_multiple_shooting_route_for_20_states_follows_the_oracle.
REGIMES = {"a": dict(T=30, scale=5.0), "b": dict(T=25, scale=2.0)}
SOLVER_DRAWS = 6             # rows of default_rng(n).standard_normal((SOLVER_DRAWS, n)); SOLVER_ROWS picks two of them per (model, regime)
MAX_ITER_ORACLE = 25         # a draw is used only if oracle.ipopt_ms.solve converges within this many iterations, with no restoration


def solver_theta(name, regime):
    th = theta_nominal(name)
    if regime == "b":
        th[3] = -2.0         # w_0
        th[-1] = 0.02
    return th


def solver_draws(name, regime):
    n = MODELS[name][0]
    return REGIMES[regime]["scale"] * np.random.default_rng(n).standard_normal((SOLVER_DRAWS, n))


# the first two draws of each (model, regime) that meet the conditions of tests/test_tile_edge_inputs.py; a draw that is passed over is named there with what it does
# (E15 (b) draw 1 is passed over: 17 iterations, one of them a restoration)
SOLVER_ROWS = {("E16", "a"): (0, 1), ("E16", "b"): (0, 1), ("E15", "a"): (0, 1), ("E15", "b"): (0, 2), ("E5", "a"): (0, 1), ("E5", "b"): (0, 1)}


def solver_inputs(name, regime):
    """dict(T, theta, x0 [2, n]): the two initial states of this (model, regime)"""
    return dict(T=REGIMES[regime]["T"], theta=solver_theta(name, regime), x0=solver_draws(name, regime)[list(SOLVER_ROWS[name, regime])])


@functools.lru_cache(maxsize=None)
def solver_oracle(name, regime, row):
    """(result, log) of oracle.ipopt_ms.solve on draw `row` - once per process"""
    from oracle import ipopt_ms
    log = []
    ref = ipopt_ms.solve(model_oracle(name), solver_draws(name, regime)[row], REGIMES[regime]["T"], solver_theta(name, regime), tol=1e-10, log=log, max_iter=100)
    return ref, log


def judge_solve(margins, tag, got, b, ref, log, worst=None, prefix="tile edge solver"):
    """tests/test_gpu_ocsolver.py::_follows on row b of a solver result (dict of [B, ...] arrays): the oracle's iteration count and step lengths, dw to 1e-12, f / inf_pr /
    theta to 1e-9, state / control / costate to 1e-9 of the largest entry - recorded through `margins` under `prefix`, or collected in `worst` (its .add)"""
    assert bool(got["converged"][b]) and int(got["status"][b]) == 0, (tag, b, got["status"][b])
    assert int(got["iterations"][b]) == ref["iterations"] == len(log), (tag, b, int(got["iterations"][b]), ref["iterations"])
    for r, l in zip(got["log"][b], log):
        assert r[5] == l["alpha"], (tag, b, l["it"], r[5], l["alpha"])
        assert abs(r[4] - l["dw"]) <= 1e-12 * max(1.0, l["dw"]), (tag, b, l["it"], r[4], l["dw"])
        assert abs(r[1] - l["f"]) <= 1e-9 * max(1.0, abs(l["f"])), (tag, b, l["it"], r[1], l["f"])
        assert abs(r[7] - l["theta"]) <= 1e-9 * max(1.0, l["theta"]) and abs(r[2] - l["inf_pr"]) <= 1e-9 * max(1.0, l["inf_pr"]), (tag, b, l["it"], r[7], l["theta"], r[2], l["inf_pr"])
    for k, kr in (("state", "state_traj_opt"), ("control", "control_traj_opt"), ("costate", "costate_traj_opt")):
        err = rel(got[k][b], ref[kr])
        if worst is None:
            margins.check("%s %s row %d: %s vs ipopt_ms.solve (relative to the largest entry)" % (prefix, tag, b, k), err, 1e-9)
        else:
            worst.add("%s vs ipopt_ms.solve (relative to the largest entry)" % k, err, "row %d" % b)
