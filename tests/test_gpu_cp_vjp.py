"""GPU: the ControlPlanning adjoint layer - cp_vjp_kernel behind pdp_cp_step_batched with a pdp_policy_cot (PDP_POLICY_COTANGENT), ModelLib.cp_rollout_vjp,
ControlPlanning.rollout_vjp_batch and pdp_amd.autograd.cp_trajectory.

Reference (cp_vjp_common): ControlPlanningOracle.getAuxSys at the oracle's own rollout, integrateAuxSys from X_0 = [0 | I] with n zero columns behind dUe - forward
sensitivities in the reference's order, not the kernel's adjoint sweep - contracted with the cotangents; tests/test_cp_vjp_host.py holds the reference's own error on
exactly these cases (the numpy recursion agrees with it to 4.2e-15 at the worst, bound 1e-11).  Bounds: the gradient 1e-10 of the largest entry OF EACH parameter block
(cp_edge_common.blocks), grad_x0 1e-10 of its largest entry, per sample, B = 5, shared and per-sample theta.  The kernel is given the GPU's own rollout
(cp_integrate), as the layer gives it.

Cases: the three edge models of tests/cp_edge_common.py under the Lagrange policy at the sweep's chunk edges T = 1, R - 1, R, R + 1, 2 R + 1 with R = cp_vjp_rows()
read from the model; 1 and 16 pivots; networks without a hidden layer, with a layer of 20 and of 32 units, eight layers, p = 480 and p = 65, each at T = 1, 7, 65;
the cost's own gradients as cotangents against ControlPlanning.step; statements that hold to the bit; the materialised route beyond the sweep's limits; the layer."""
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
import cp_vjp_common as cv  # noqa: E402


def npy(t):
    return t.detach().cpu().numpy()


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
    """one case, shared and per-sample theta, all five samples: the worst block of the gradient and grad_x0 against the reference"""
    mdl = model(name)
    inp = ce.inputs(name, kind, key, T)
    pol = policy(kind, key, T)
    gx, gu = cv.cotangents(name, T)
    worst_g = worst_x = 0.0
    for per_sample in (False, True):
        th = inp["theta_b"] if per_sample else inp["theta"]
        x, _, _ = mdl.cp_integrate_T(pol, inp["p"], inp["x0"], th, T)
        out = mdl.cp_rollout_vjp(pol, inp["p"], x, th, gx, gu, **kw)
        g, g0 = npy(out["grad_theta"]), npy(out["grad_x0"])
        assert g.shape == (inp["B"], inp["p"]) and g0.shape == (inp["B"], ce.MODELS[name][0])
        for b in range(inp["B"]):
            r = cv.reference(name, kind, key, T, per_sample, b)
            worst_g = max(worst_g, cv.grad_rel(name, kind, key, g[b], r["grad_theta"]))
            worst_x = max(worst_x, cv.x0_rel(g0[b], r["grad_x0"]))
    print("%s: gradient %.3e, grad_x0 %.3e" % (label, worst_g, worst_x))
    margins.check("cp vjp %s vs reference: gradient (largest entry of each block)" % label, worst_g, cv.TOL)
    margins.check("cp vjp %s vs reference: grad_x0 (its largest entry)" % label, worst_x, cv.TOL)


# ---- the tuned kernel against the reference ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edge", cv.EDGES)
@pytest.mark.parametrize("name", ce.NAMES)
def test_lagrange_policy_at_the_chunk_edges(margins, name, edge):
    R = model(name).cp_vjp_rows()                  # read from the model; the host test holds cv.ROWS, by which the reference's cases are listed, to the same rule
    assert R == cv.ROWS[name]
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


# ---- against the step kernels -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cv.STEP_CASES, ids=cv.case_id)
def test_the_costs_own_gradients_as_cotangents_give_the_step_kernels_gradient(margins, case):
    """dcx, dcu of cp_auxsys and dhx as gx_T: grad_theta is ControlPlanning.step's gradient (forward sensitivities on MFMA tiles for the Lagrange policy, the register
    kernel for (12, 16, 4), cp_step_adjoint_kernel for (20, 4)), per parameter block"""
    import torch
    name, kind, key, T = case
    mdl, inp, pol = model(name), ce.inputs(name, kind, key, T), policy(kind, key, T)
    if kind == "mlp":
        assert ce.route(name, key) == ("register" if key == (12, 16, 4) else "adjoint")
    worst = 0.0
    for th in (inp["theta"], inp["theta_b"]):
        _, grad, x, u = mdl.cp_step(pol, inp["p"], inp["x0"], th, T, want_traj=True)
        aux = mdl.cp_auxsys(pol, inp["p"], x, u, th)
        gx = torch.cat([aux["dcx"], aux["dhx"][:, None]], dim=1)
        out = mdl.cp_rollout_vjp(pol, inp["p"], x, th, gx, aux["dcu"], want_ini=False)
        assert sorted(out) == ["grad_theta"]
        for b in range(inp["B"]):
            worst = max(worst, cv.grad_rel(name, kind, key, npy(out["grad_theta"])[b], npy(grad)[b]))
    print("%s: %.3e" % (cv.case_id(case), worst))
    margins.check("cp vjp %s with the cost's gradients vs step_batch: gradient (largest entry of each block)" % cv.case_id(case), worst, cv.TOL)


# ---- exact statements ---------------------------------------------------------------------------------------------------------------------------------------------
EXACT = (("C5", "poly", 6, 65), ("C5", "mlp", (32, 1), 7), ("C16", "mlp", (12, 16, 4), 65))


def _setup(case):
    name, kind, key, T = case
    mdl, inp, pol = model(name), ce.inputs(name, kind, key, T), policy(kind, key, T)
    x, _, _ = mdl.cp_integrate_T(pol, inp["p"], inp["x0"], inp["theta_b"], T)
    gx, gu = cv.cotangents(name, T)
    return mdl, inp, pol, x, gx, gu


@pytest.mark.parametrize("case", EXACT, ids=cv.case_id)
def test_zero_cotangents_give_zeros_and_gx0_alone_passes_through(case):
    mdl, inp, pol, x, gx, gu = _setup(case)
    out = mdl.cp_rollout_vjp(pol, inp["p"], x, inp["theta_b"], 0 * gx, 0 * gu)
    assert (npy(out["grad_theta"]) == 0).all() and (npy(out["grad_x0"]) == 0).all()
    g0 = 0 * gx
    g0[:, 0] = gx[:, 0]
    out = mdl.cp_rollout_vjp(pol, inp["p"], x, inp["theta_b"], g0, 0 * gu)
    assert (npy(out["grad_x0"]) == gx[:, 0]).all() and (npy(out["grad_theta"]) == 0).all()


@pytest.mark.parametrize("case", EXACT, ids=cv.case_id)
def test_a_row_depends_neither_on_its_batch_nor_on_its_position_and_the_outputs_not_on_each_other(case):
    mdl, inp, pol, x, gx, gu = _setup(case)
    th = inp["theta_b"]
    both = mdl.cp_rollout_vjp(pol, inp["p"], x, th, gx, gu)
    G, G0 = npy(both["grad_theta"]), npy(both["grad_x0"])
    assert np.isfinite(G).all() and np.isfinite(G0).all() and np.abs(G).max() > 0
    xn = npy(x)
    for rows in ([3], [4, 2, 0], [1, 1, 1, 1, 1, 1, 1]):
        o = mdl.cp_rollout_vjp(pol, inp["p"], xn[rows], th[rows], gx[rows], gu[rows])
        assert np.array_equal(npy(o["grad_theta"]), G[rows]) and np.array_equal(npy(o["grad_x0"]), G0[rows]), rows
    only_theta = mdl.cp_rollout_vjp(pol, inp["p"], x, th, gx, gu, want_ini=False)
    only_ini = mdl.cp_rollout_vjp(pol, inp["p"], x, th, gx, gu, want_theta=False)
    assert sorted(only_theta) == ["grad_theta"] and sorted(only_ini) == ["grad_x0"]
    assert np.array_equal(npy(only_theta["grad_theta"]), G) and np.array_equal(npy(only_ini["grad_x0"]), G0)
    # a non-finite input gives a non-finite row, and that row only
    bad = gx.copy()
    bad[2, 3, 0] = np.nan
    o = mdl.cp_rollout_vjp(pol, inp["p"], x, th, bad, gu)
    keep = [0, 1, 3, 4]
    assert np.isnan(npy(o["grad_x0"])[2]).any() and np.array_equal(npy(o["grad_theta"])[keep], G[keep]) and np.array_equal(npy(o["grad_x0"])[keep], G0[keep])


def test_the_step_and_the_rollout_are_what_they_were_around_a_vjp_call():
    import torch
    for case in EXACT[:2]:
        name, kind, key, T = case
        cp = ce.model_gpu(name)
        cp._model = model(name)
        if kind == "poly":
            cp.setPolyControl(np.linspace(0, T, key))
        else:
            cp.setNeuralPolicy(list(key[:-1]))
        inp = ce.inputs(name, kind, key, T)
        gx, gu = cv.cotangents(name, T)
        before = cp.step_batch(inp["x0"], T, inp["theta_b"]) + cp.integrateSys_batch(inp["x0"], T, inp["theta_b"])
        out = cp.rollout_vjp_batch(before[2], inp["theta_b"], gx, gu)
        assert tuple(out["grad_theta"].shape) == (inp["B"], inp["p"])
        after = cp.step_batch(inp["x0"], T, inp["theta_b"]) + cp.integrateSys_batch(inp["x0"], T, inp["theta_b"])
        assert all(torch.equal(a, b) for a, b in zip(before, after))


# ---- beyond the sweep's limits: the materialised route -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,layers", cv.FALLBACK_NETS, ids=["p612", "width33"])
def test_networks_beyond_the_limits_take_the_materialised_route(margins, name, layers):
    assert ce.route(name, layers) == "generic"
    against_reference(margins, "%s network %s, T = %d, materialised" % (name, list(layers), cv.FALLBACK_T), name, "mlp", layers, cv.FALLBACK_T)


def test_the_materialised_route_on_a_table_policy_and_forced_on_a_tuned_case(margins):
    """a table policy whose table is the Lagrange basis is the Lagrange policy: the same reference; and the forced route agrees with the sweep on a network"""
    from pdp_amd import runtime as rt
    name, N, T = "C5", 6, 7
    mdl, inp = model(name), ce.inputs(name, "poly", 6, 7)
    orc = cv.oracle_for(name, "poly", N, T)
    pol = rt.make_policy("table", table=np.stack([orc._basis(t) for t in range(T)]))
    gx, gu = cv.cotangents(name, T)
    x, _, _ = mdl.cp_integrate_T(pol, inp["p"], inp["x0"], inp["theta_b"], T)
    out = mdl.cp_rollout_vjp(pol, inp["p"], x, inp["theta_b"], gx, gu)
    worst = 0.0
    for b in range(inp["B"]):
        r = cv.reference(name, "poly", N, T, True, b)
        worst = max(worst, cv.grad_rel(name, "poly", N, npy(out["grad_theta"])[b], r["grad_theta"]), cv.x0_rel(npy(out["grad_x0"])[b], r["grad_x0"]))
    margins.check("cp vjp C5 table policy (the Lagrange basis), T = 7, materialised, vs reference: gradient blocks and grad_x0", worst, cv.TOL)
    against_reference(margins, "C5 network [32, 1], T = 7, materialised by force", "C5", "mlp", (32, 1), 7, force_materialised=True)


# ---- the layer -----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_sample", [False, True], ids=["shared", "per_sample"])
@pytest.mark.parametrize("system", sorted(cv.LAYER))
def test_the_layers_gradients_follow_the_reference(margins, system, per_sample):
    import torch
    from pdp_amd.autograd import cp_trajectory
    cfg, inp = cv.LAYER[system], cv.layer_inputs(system)
    cp, orc = cv.zoo_cp(system, layers=cfg["layers"]), cv.zoo_oracle(system, cfg["layers"])
    assert cp.n_auxvar == orc.n_auxvar
    B, T = cfg["B"], cfg["T"]
    f64 = dict(dtype=torch.float64, device="cuda")
    gx, gu = torch.tensor(inp["gx"], **f64), torch.tensor(inp["gu"], **f64)

    def run(ini_grad):
        theta = torch.tensor(inp["theta_b"] if per_sample else inp["theta"], requires_grad=True, **f64)
        ini = torch.tensor(inp["x0"], requires_grad=ini_grad, **f64)
        state, control = cp_trajectory(cp, ini, T, theta)
        assert tuple(state.shape) == (B, T + 1, orc.n) and tuple(control.shape) == (B, T, orc.m)
        ((gx * state).sum() + (gu * control).sum()).backward()
        return theta.grad, ini.grad
    gt, gi = run(True)
    refs = [cv.reference_at(orc, inp["x0"][b], T, inp["theta_b"][b] if per_sample else inp["theta"], inp["gx"][b], inp["gu"][b]) for b in range(B)]
    want_t = np.stack([r["grad_theta"] for r in refs]) if per_sample else sum(r["grad_theta"] for r in refs)
    want_i = np.stack([r["grad_x0"] for r in refs])
    margins.check("cp layer %s %s theta.grad vs reference (largest entry)" % (system, "per-sample" if per_sample else "shared"),
                  np.abs(npy(gt) - want_t).max() / np.abs(want_t).max(), cv.TOL)
    margins.check("cp layer %s %s ini_state.grad vs reference (largest entry)" % (system, "per-sample" if per_sample else "shared"),
                  np.abs(npy(gi) - want_i).max() / np.abs(want_i).max(), cv.TOL)
    gt2, gi2 = run(False)
    assert gi2 is None and torch.equal(gt, gt2)                      # bit-identical without the initial state's gradient
    # a missing cotangent is zeros: a loss on the controls alone, and on the states alone
    theta = torch.tensor(inp["theta"], requires_grad=True, **f64)
    state, control = cp_trajectory(cp, inp["x0"], T, theta)
    (gu * control).sum().backward()
    want_u = sum(cv.reference_at(orc, inp["x0"][b], T, inp["theta"], 0 * inp["gx"][b], inp["gu"][b])["grad_theta"] for b in range(B))
    assert np.abs(npy(theta.grad) - want_u).max() <= cv.TOL * np.abs(want_u).max()
    theta.grad = None
    state, control = cp_trajectory(cp, inp["x0"], T, theta)
    (gx * state).sum().backward()
    want_x = sum(cv.reference_at(orc, inp["x0"][b], T, inp["theta"], inp["gx"][b], 0 * inp["gu"][b])["grad_theta"] for b in range(B))
    assert np.abs(npy(theta.grad) - want_x).max() <= cv.TOL * np.abs(want_x).max()


def test_the_layers_argument_errors():
    import torch
    from pdp_amd.autograd import cp_trajectory
    cfg, inp = cv.LAYER["cartpole"], cv.layer_inputs("cartpole")
    cp = cv.zoo_cp("cartpole", layers=cfg["layers"])
    f64 = dict(dtype=torch.float64, device="cuda")
    theta = torch.tensor(inp["theta"], **f64)
    with pytest.raises(TypeError, match="CUDA fp64"):
        cp_trajectory(cp, inp["x0"], cfg["T"], theta.cpu())
    with pytest.raises(TypeError, match="CUDA fp64"):
        cp_trajectory(cp, inp["x0"], cfg["T"], theta.float())
    with pytest.raises(ValueError, match="p = %d" % cp.n_auxvar):
        cp_trajectory(cp, inp["x0"], cfg["T"], theta[:-1])
    with pytest.raises(ValueError, match="per-sample"):
        cp_trajectory(cp, inp["x0"], cfg["T"], theta[None].repeat(cfg["B"] + 1, 1))
    with pytest.raises(TypeError, match="ini_state"):
        cp_trajectory(cp, torch.tensor(inp["x0"], dtype=torch.float32, device="cuda", requires_grad=True), cfg["T"], theta)
    with pytest.raises(ValueError, match="ini_state"):
        cp_trajectory(cp, inp["x0"][:, :3], cfg["T"], theta)
    with pytest.raises(ValueError, match="horizon"):
        cp_trajectory(cp, inp["x0"], 0, theta)


def test_adam_on_the_examples_loss_goes_down():
    """examples/cp_layer_custom_loss.py at B = 4, T = 10: 20 Adam steps end strictly below the starting loss"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("cp_layer_custom_loss", os.path.join(ROOT, "examples", "cp_layer_custom_loss.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    trace = ex.main(["--iters", "20", "--batch", "4", "--horizon", "10"])
    assert len(trace) == 20 and np.isfinite(trace).all() and trace[-1] < trace[0], trace
