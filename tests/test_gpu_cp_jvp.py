"""GPU: the ControlPlanning tangent layer - cp_jvp_kernel behind pdp_cp_step_batched with a pdp_policy_tan (PDP_POLICY_TANGENT), ModelLib.cp_rollout_jvp,
ControlPlanning.rollout_jvp_batch, torch.autograd.forward_ad through pdp_amd.autograd.cp_trajectory and irl.MatrixFreeLM.for_cp.

Reference (cp_jvp_common): ControlPlanningOracle.getAuxSys at the oracle's own rollout, integrateAuxSys from X_0 = [0 | I] with n zero columns behind dUe - forward
sensitivities in the reference's order, not the kernel's sweep of one vector - contracted with the direction; tests/test_cp_jvp_host.py holds the reference's own
error on exactly these cases (the numpy recursion agrees with it to 1e-11).  Bound: 1e-10 of the largest entry of d_state and of d_control, per sample, B = 5, shared
and per-sample theta, all five samples.  The kernel is given the GPU's own rollout and controls (cp_integrate), as the layer gives them.

Cases: the three edge models of tests/cp_edge_common.py under the Lagrange policy at the sweep's chunk edges T = 1, R - 1, R, R + 1, 2 R + 1 with R = cp_jvp_rows()
read from the model; 1 and 16 pivots; the seven networks of cp_vjp_common.NETS, each at T = 1, 7, 65; statements that hold to the bit; duality with cp_vjp_kernel;
the one-column materialised route beyond the sweep's limits; forward mode through the layer; the Levenberg-Marquardt loop; the example."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import cp_edge_common as ce  # noqa: E402
import cp_jvp_common as cj  # noqa: E402
import cp_vjp_common as cv  # noqa: E402


def npy(t):
    return t.detach().cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


_models = {}


def model(name):
    """the edge model's library: compiled on first use, once per process"""
    if name not in _models:
        _models[name] = ce.model_gpu(name).model()
    return _models[name]


def policy(kind, key, T):
    from pdp_amd import runtime as rt
    return rt.make_policy("poly", pivots=np.linspace(0, T, key)) if kind == "poly" else rt.make_policy("mlp", layers=list(key))


def against_reference(margins, label, name, kind, key, T, **kw):
    """one case, shared and per-sample theta (and d_theta), all five samples: d_state and d_control against the reference, both tangents and each alone"""
    mdl = model(name)
    inp = ce.inputs(name, kind, key, T)
    pol = policy(kind, key, T)
    tan = cj.tangents(name, kind, key, T)
    n, m = ce.MODELS[name]
    worst_x = worst_u = 0.0
    for per_sample in (False, True):
        th = inp["theta_b"] if per_sample else inp["theta"]
        dth = tan["d_theta_b"] if per_sample else tan["d_theta"]
        x, u, _ = mdl.cp_integrate_T(pol, inp["p"], inp["x0"], th, T)
        for use_th, use_x0 in ((True, True), (True, False), (False, True)):
            out = mdl.cp_rollout_jvp(pol, inp["p"], x, u, th, d_theta=dth if use_th else None, d_x0=tan["d_x0"] if use_x0 else None, **kw)
            dx, du = npy(out["d_state"]), npy(out["d_control"])
            assert dx.shape == (inp["B"], T + 1, n) and du.shape == (inp["B"], T, m)
            for b in range(inp["B"]):
                r = cj.reference(name, kind, key, T, per_sample, b)
                want_x, want_u = cj.contract(r["X"], r["U"], cj.d_theta_of(tan, per_sample, b) if use_th else None, tan["d_x0"][b] if use_x0 else None)
                worst_x, worst_u = max(worst_x, cj.rel(dx[b], want_x)), max(worst_u, cj.rel(du[b], want_u))
    print("%s: d_state %.3e, d_control %.3e" % (label, worst_x, worst_u))
    margins.check("cp jvp %s vs reference: d_state (its largest entry)" % label, worst_x, cj.TOL)
    margins.check("cp jvp %s vs reference: d_control (its largest entry)" % label, worst_u, cj.TOL)


# ---- the tuned kernel against the reference ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edge", cv.EDGES)
@pytest.mark.parametrize("name", ce.NAMES)
def test_lagrange_policy_at_the_chunk_edges(margins, name, edge):
    R = model(name).cp_jvp_rows()                  # read from the model; the host test holds cj.ROWS, by which the reference's cases are listed, to the same rule
    assert R == cj.ROWS[name]
    T = cv.edge_T(R, edge)
    against_reference(margins, "%s Lagrange N = 6, T = %s = %d" % (name, edge, T), name, "poly", cv.EDGE_PIVOTS, T)


@pytest.mark.parametrize("name,pivots", cv.PIVOT_CASES)
def test_one_and_sixteen_pivots(margins, name, pivots):
    against_reference(margins, "%s Lagrange N = %d, T = %d" % (name, pivots, cv.PIVOT_T), name, "poly", pivots, cv.PIVOT_T)


@pytest.mark.parametrize("T", cv.MLP_HORIZONS)
@pytest.mark.parametrize("name,layers", list(cv.NETS), ids=["%s_%s" % (n, "x".join(map(str, l))) for n, l in cv.NETS])
def test_network_policies(margins, name, layers, T):
    n, m = ce.MODELS[name]
    assert ce.route(name, layers) != "generic", "on the tuned route"
    against_reference(margins, "%s network %s (p = %d), T = %d" % (name, list(layers), ce.mlp_params(n, layers), T), name, "mlp", layers, T)


# ---- exact statements ---------------------------------------------------------------------------------------------------------------------------------------------
EXACT = (("C5", "poly", 6, 65), ("C5", "mlp", (32, 1), 7), ("C16", "mlp", (12, 16, 4), 65))


def _setup(case):
    name, kind, key, T = case
    mdl, inp, pol = model(name), ce.inputs(name, kind, key, T), policy(kind, key, T)
    x, u, _ = mdl.cp_integrate_T(pol, inp["p"], inp["x0"], inp["theta_b"], T)
    return mdl, inp, pol, x, u, cj.tangents(name, kind, key, T)


@pytest.mark.parametrize("case", EXACT, ids=cv.case_id)
def test_zero_tangents_null_tangents_and_the_stride_of_d_theta(case):
    mdl, inp, pol, x, u, tan = _setup(case)
    p, th = inp["p"], inp["theta_b"]
    run = lambda **kw: {k: npy(v) for k, v in mdl.cp_rollout_jvp(pol, p, x, u, th, **kw).items()}
    out = run(d_theta=np.zeros_like(tan["d_theta_b"]), d_x0=np.zeros_like(tan["d_x0"]))
    assert (out["d_state"] == 0).all() and (out["d_control"] == 0).all()
    full = run(d_theta=tan["d_theta_b"], d_x0=tan["d_x0"])
    assert np.isfinite(full["d_state"]).all() and np.isfinite(full["d_control"]).all() and np.abs(full["d_control"]).max() > 0
    assert (full["d_state"][:, 0] == tan["d_x0"]).all()
    # a NULL tangent is a buffer of zeros (+0.0: np.zeros_like, not 0 * tangent, which keeps the signs)
    only_th, only_x0 = run(d_theta=tan["d_theta_b"]), run(d_x0=tan["d_x0"])
    zeros_x0, zeros_th = run(d_theta=tan["d_theta_b"], d_x0=np.zeros_like(tan["d_x0"])), run(d_theta=np.zeros_like(tan["d_theta_b"]), d_x0=tan["d_x0"])
    for k in ("d_state", "d_control"):
        assert same_bits(only_th[k], zeros_x0[k]) and same_bits(only_x0[k], zeros_th[k]), k
    assert (only_th["d_state"][:, 0] == 0).all()
    # one d_theta shared by the batch is the same row repeated with the stride p
    shared, repeated = run(d_theta=tan["d_theta"], d_x0=tan["d_x0"]), run(d_theta=np.repeat(tan["d_theta"][None], inp["B"], axis=0), d_x0=tan["d_x0"])
    for k in ("d_state", "d_control"):
        assert same_bits(shared[k], repeated[k]), k
    # without d_u the bits of d_state are the same
    no_u = mdl.cp_rollout_jvp(pol, p, x, u, th, d_theta=tan["d_theta_b"], d_x0=tan["d_x0"], want_control=False)
    assert sorted(no_u) == ["d_state"] and same_bits(npy(no_u["d_state"]), full["d_state"])


@pytest.mark.parametrize("case", EXACT, ids=cv.case_id)
def test_a_row_depends_neither_on_its_batch_nor_on_its_position_and_a_nan_stays_in_its_trajectory(case):
    mdl, inp, pol, x, u, tan = _setup(case)
    p, th = inp["p"], inp["theta_b"]
    full = {k: npy(v) for k, v in mdl.cp_rollout_jvp(pol, p, x, u, th, d_theta=tan["d_theta_b"], d_x0=tan["d_x0"]).items()}
    xn, un = npy(x), npy(u)
    for rows in ([3], [4, 2, 0], [1, 1, 1, 1, 1, 1, 1]):
        o = mdl.cp_rollout_jvp(pol, p, xn[rows], un[rows], th[rows], d_theta=tan["d_theta_b"][rows], d_x0=tan["d_x0"][rows])
        assert same_bits(npy(o["d_state"]), full["d_state"][rows]) and same_bits(npy(o["d_control"]), full["d_control"][rows]), rows
    keep = [0, 1, 3, 4]
    for bad in (dict(d_theta=tan["d_theta_b"].copy(), d_x0=tan["d_x0"]), dict(d_theta=tan["d_theta_b"], d_x0=tan["d_x0"].copy())):
        (bad["d_theta"] if bad["d_theta"] is not tan["d_theta_b"] else bad["d_x0"])[2, 0] = np.nan
        o = {k: npy(v) for k, v in mdl.cp_rollout_jvp(pol, p, x, u, th, **bad).items()}
        assert np.isnan(o["d_state"][2]).any()
        assert same_bits(o["d_state"][keep], full["d_state"][keep]) and same_bits(o["d_control"][keep], full["d_control"][keep])


def test_the_step_the_rollout_and_the_vjp_are_what_they_were_around_a_jvp_call():
    import torch
    for case in EXACT[:2]:
        name, kind, key, T = case
        cp = ce.model_gpu(name)
        cp._model = model(name)
        if kind == "poly":
            cp.setPolyControl(np.linspace(0, T, key))
        else:
            cp.setNeuralPolicy(list(key[:-1]))
        inp, tan = ce.inputs(name, kind, key, T), cj.tangents(name, kind, key, T)
        gx, gu = cv.cotangents(name, T)

        def everything():
            out = cp.step_batch(inp["x0"], T, inp["theta_b"]) + cp.integrateSys_batch(inp["x0"], T, inp["theta_b"])
            v = cp.rollout_vjp_batch(out[2], inp["theta_b"], gx, gu)
            return out + (v["grad_theta"], v["grad_x0"])
        before = everything()
        out = cp.rollout_jvp_batch(before[2], before[3], inp["theta_b"], d_auxvar=tan["d_theta_b"], d_ini_state=tan["d_x0"])
        assert tuple(out["d_state"].shape) == (inp["B"], T + 1, ce.MODELS[name][0]) and tuple(out["d_control"].shape) == (inp["B"], T, ce.MODELS[name][1])
        after = everything()
        assert all(torch.equal(a, b) for a, b in zip(before, after))


# ---- duality with the adjoint sweep -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", EXACT + (("C15", "poly", 6, 54),), ids=cv.case_id)
def test_duality_with_the_adjoint_sweep(margins, case):
    """<gx, d_state> + <gu, d_control> against <grad_theta, d_theta> + <grad_x0, d_x0> with the unchanged cp_vjp_kernel, for random cotangents and tangents: the gap
    the per-entry bound of both sides implies, 1e-10 (|g|_1 max|J v| + |v|_1 max|J' g|), per trajectory"""
    name, kind, key, T = case
    mdl, inp, pol, x, u, tan = _setup(case)
    gx, gu = cv.cotangents(name, T)
    jv = {k: npy(v) for k, v in mdl.cp_rollout_jvp(pol, inp["p"], x, u, inp["theta_b"], d_theta=tan["d_theta_b"], d_x0=tan["d_x0"]).items()}
    jtg = {k: npy(v) for k, v in mdl.cp_rollout_vjp(pol, inp["p"], x, inp["theta_b"], gx, gu).items()}
    for b in range(inp["B"]):
        g, Jv = np.concatenate([gx[b].ravel(), gu[b].ravel()]), np.concatenate([jv["d_state"][b].ravel(), jv["d_control"][b].ravel()])
        v, Jtg = np.concatenate([tan["d_theta_b"][b], tan["d_x0"][b]]), np.concatenate([jtg["grad_theta"][b], jtg["grad_x0"][b]])
        allowed = np.abs(g).sum() * np.abs(Jv).max() + np.abs(v).sum() * np.abs(Jtg).max()
        margins.check("cp jvp %s sample %d: g . (J v) against (J' g) . v" % (cv.case_id(case), b), abs(float(g @ Jv) - float(Jtg @ v)) / allowed, cj.TOL)


# ---- beyond the sweep's limits: the one-column materialised route ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,layers", cv.FALLBACK_NETS, ids=["p612", "width33"])
def test_networks_beyond_the_limits_take_the_materialised_route(margins, name, layers):
    assert ce.route(name, layers) == "generic"
    against_reference(margins, "%s network %s, T = %d, materialised" % (name, list(layers), cv.FALLBACK_T), name, "mlp", layers, cv.FALLBACK_T)


def test_the_materialised_route_on_a_table_policy_and_forced_on_a_tuned_case(margins):
    """a table policy whose table is the Lagrange basis is the Lagrange policy: the same reference; and the forced route agrees with the reference on a network"""
    from pdp_amd import runtime as rt
    name, N, T = "C5", 6, 7
    mdl, inp = model(name), ce.inputs(name, "poly", N, T)
    orc = cv.oracle_for(name, "poly", N, T)
    pol = rt.make_policy("table", table=np.stack([orc._basis(t) for t in range(T)]))
    tan = cj.tangents(name, "poly", N, T)
    x, u, _ = mdl.cp_integrate_T(pol, inp["p"], inp["x0"], inp["theta_b"], T)
    out = mdl.cp_rollout_jvp(pol, inp["p"], x, u, inp["theta_b"], d_theta=tan["d_theta_b"], d_x0=tan["d_x0"])
    worst = 0.0
    for b in range(inp["B"]):
        r = cj.reference(name, "poly", N, T, True, b)
        want_x, want_u = cj.contract(r["X"], r["U"], tan["d_theta_b"][b], tan["d_x0"][b])
        worst = max(worst, cj.rel(npy(out["d_state"])[b], want_x), cj.rel(npy(out["d_control"])[b], want_u))
    margins.check("cp jvp C5 table policy (the Lagrange basis), T = 7, materialised, vs reference: d_state and d_control", worst, cj.TOL)
    against_reference(margins, "C5 network [32, 1], T = 7, materialised by force", "C5", "mlp", (32, 1), 7, force_materialised=True)


# ---- the layer -----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("system", sorted(cv.LAYER))
def test_forward_mode_through_the_layer(margins, system):
    """torch.autograd.forward_ad through cp_trajectory on the cart-pole and the quadrotor of the zoo: dual theta ([p] and [B, p]) and a dual ini_state, together and
    each alone, give rollout_jvp_batch's bits and follow the reference; the backward pass next to it is the one it was"""
    import torch
    import torch.autograd.forward_ad as fwAD
    from pdp_amd.autograd import cp_trajectory
    cfg, inp = cv.LAYER[system], cv.layer_inputs(system)
    cp, orc = cv.zoo_cp(system, layers=cfg["layers"]), cv.zoo_oracle(system, cfg["layers"])
    B, T, p = cfg["B"], cfg["T"], orc.n_auxvar
    rng = np.random.default_rng(cj.SEED + orc.n)
    dv = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda", dtype=torch.float64)
    d_x0 = rng.standard_normal((B, orc.n))
    x0, dx0 = dv(inp["x0"]), dv(d_x0)
    for key in ("theta", "theta_b"):
        d_theta = rng.standard_normal(p if key == "theta" else (B, p))
        th, dth = dv(inp[key]), dv(d_theta)
        x, u, _ = cp.integrateSys_batch(x0, T, th)
        with fwAD.dual_level():
            state, control = cp_trajectory(cp, fwAD.make_dual(x0, dx0), T, fwAD.make_dual(th, dth))
            (xs, dxs), (us, dus) = fwAD.unpack_dual(state), fwAD.unpack_dual(control)
            direct = cp.rollout_jvp_batch(x, u, th, d_auxvar=dth, d_ini_state=dx0)
            assert same_bits(npy(xs), npy(x)) and same_bits(npy(us), npy(u))
            assert same_bits(npy(dxs), npy(direct["d_state"])) and same_bits(npy(dus), npy(direct["d_control"]))
            worst = 0.0
            for b in range(B):
                r = cj.reference_at(orc, inp["x0"][b], T, inp[key][b] if key == "theta_b" else inp[key])
                want_x, want_u = cj.contract(r["X"], r["U"], d_theta[b] if key == "theta_b" else d_theta, d_x0[b])
                worst = max(worst, cj.rel(npy(dxs)[b], want_x), cj.rel(npy(dus)[b], want_u))
            margins.check("cp layer forward mode, %s, %s: tangents of state and control (largest entry)" % (system, key), worst, cj.TOL)
            state, control = cp_trajectory(cp, x0, T, fwAD.make_dual(th, dth))
            only = cp.rollout_jvp_batch(x, u, th, d_auxvar=dth)
            assert same_bits(npy(fwAD.unpack_dual(state).tangent), npy(only["d_state"])) and same_bits(npy(fwAD.unpack_dual(control).tangent), npy(only["d_control"]))
            state, control = cp_trajectory(cp, fwAD.make_dual(x0, dx0), T, th)
            only = cp.rollout_jvp_batch(x, u, th, d_ini_state=dx0)
            assert same_bits(npy(fwAD.unpack_dual(state).tangent), npy(only["d_state"])) and same_bits(npy(fwAD.unpack_dual(control).tangent), npy(only["d_control"]))
        theta = th.clone().requires_grad_(True)
        gx, gu = dv(inp["gx"]), dv(inp["gu"])
        state, control = cp_trajectory(cp, x0, T, theta)
        ((gx * state).sum() + (gu * control).sum()).backward()
        want = cp.rollout_vjp_batch(x, th, gx, gu, want_ini=False)["grad_theta"]
        assert same_bits(npy(theta.grad), npy(want.sum(dim=0) if key == "theta" else want))


# ---- Levenberg-Marquardt -----------------------------------------------------------------------------------------------------------------------------------------------
def test_matrix_free_lm_for_cp_on_the_budget_problem():
    """MatrixFreeLM.for_cp on the problem of the host test's numpy restatement (C15, 6 pivots, p = 18, T = 12, B = 5, states-only residual, reachable targets): a loss
    below 1e-18, a strictly decreasing accepted trace, at most twice the evaluations and twice the CG iterations of the restatement
    (tests/golden/cp_jvp_lm_budget.json)"""
    import torch
    from pdp_amd.irl import MatrixFreeLM
    P, budget = cj.lm_problem(), cj.budget()
    cp = ce.model_gpu(cj.LM["name"])
    cp._model = model(cj.LM["name"])
    cp.setPolyControl(np.linspace(0, P["T"], cj.LM["pivots"]))
    target = torch.as_tensor(P["target"], device="cuda")
    loop = MatrixFreeLM.for_cp(cp, P["x0"], P["T"], P["theta0"], lambda state, control: state - target)
    r = loop.run(max_evals=2 * budget["evaluations"], loss_tol=1e-18)
    print("loss trace %s; %d evaluations (restatement %d), %d rejected, %d CG iterations (restatement %d); |theta - truth| %.2e"
          % (" ".join("%.3e" % v for v in r["loss_trace"]), r["evaluations"], budget["evaluations"], r["rejected"], r["cg_iterations"], budget["cg_iterations"],
             np.abs(r["parameter_trace"][-1] - P["theta_true"]).max()))
    assert set(r) >= {"loss_trace", "parameter_trace", "lambda_trace", "evaluations", "rejected", "stalled", "iterations", "cg_iterations"}
    assert r["loss_trace"][-1] < 1e-18 and (np.diff(r["loss_trace"]) < 0).all()
    assert r["evaluations"] <= 2 * budget["evaluations"] and r["cg_iterations"] <= 2 * budget["cg_iterations"]
    assert r["parameter_trace"].shape == (len(r["loss_trace"]), 18) and not r["stalled"]


def test_the_example_runs_at_a_reduced_size():
    """examples/cp_gauss_newton_plan.py at B = 4, T = 10, 4 pivots, 10 Adam steps: both loops run and the Levenberg-Marquardt trace decreases"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("cp_gauss_newton_plan", os.path.join(ROOT, "examples", "cp_gauss_newton_plan.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    out = ex.main(["--batch", "4", "--horizon", "10", "--pivots", "4", "--max-evals", "10", "--adam-iters", "10"])
    lm = out["lm"]
    assert len(out["adam"]) == 10 and np.isfinite(out["adam"]).all() and np.isfinite(lm["loss_trace"]).all()
    assert len(lm["loss_trace"]) >= 2 and (np.diff(lm["loss_trace"]) < 0).all() and lm["cg_iterations"] >= 1
