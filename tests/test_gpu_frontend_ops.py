"""GPU: generated models that use every operator the symbolic front-end offers (tests/frontend_ops_common.py) through the kernels that evaluate a user's model.
tests/test_frontend_ops_host.py holds the CPU half: the front-end and the emitted text against sympy at 40 digits, and the conditions on the inputs used here.

a. OPT, the operator table, at T = 1 with the batch rows as argument points: oc_rollout, oc_costate and oc_auxsys against sympy's derivatives at 40 digits, PER ENTRY
   relative to that entry's own magnitude (a 1e13 exp row cannot hide a wrong log row), structural zeros exactly zero, odd powers of negative bases finite with the
   base's sign.
b. OPS5 as OC: oc_rollout, oc_costate, oc_auxsys against the oracle at T = 1, 7 and ROWS + 7.
c. OPS5 as OC: the fused unit (loss, gradient, dx/dtheta, du/dtheta) against oracle.pdp_oc_unit and, on every sample, the 40-digit (X, U); the cotangent unit with the initial-state
   gradient against the same sensitivities contracted; one oc_solve_ms case (w7 raised: H_uu positive definite) against oracle.ipopt_ms.solve with the tolerances of
   tests/test_gpu_tile_edge.py's solver rows.
d. OPS3 (n = 3): the same on the small-system route - the model's library holds the one-wave unit and no runner / evaluator instantiation.
e. OPS5 as SysID (auxvar w0..w4) at T = 7 and R + 1 (R the sweep kernels' pool rows): sysid_integrate, sysid_auxsys, sysid_step (loss, gradient, Gauss-Newton matrix),
   sysid_rollout_vjp with the gradient with respect to the inputs (the `pathu` group, precompute_u) and sysid_rollout_jvp, against SysIDOracle's forward sensitivities and
   sympy's G = df/du propagated forward.
f. OPS5 as ControlPlanning (the parameters as numbers) at T = 7 and R + 1 of cp_vjp_rows(), under a Lagrange policy with 4 pivots and a 5-4-2 tanh network: integrateSys,
   getAuxSys, step, rollout_vjp and rollout_jvp against ControlPlanningOracle built as cp_vjp_common.oracle_for builds it.

B = 5, one shared theta and one per sample (5 % around nominal: precompute runs per trajectory).  Tolerance: TOL = 1e-10 relative to the largest entry of the compared
array, per sample, through the `margins` fixture; OPT per entry with the same 1e-10.

Measured on an MI355X, the worst figure of each part over theta modes, samples, horizons and quantities (every one against the bound 1e-10):
    a. OPT, per entry                 2.8e-14  (oc_auxsys hxx; every other quantity <= 1.8e-15)
    b. OPS5 OC model evaluation       1.2e-15  (oc_costate, T = 35)
    c. OPS5 OC fused unit             5.7e-13  (du/dtheta at T = 35, shared theta, sample 3, against the oracle's U and against the 40-digit U alike; the oracle itself
                                               is 3.1e-13 from 40 digits on that sample - H_uu is indefinite there, smallest eigenvalue -3.4; T = 1 and 7:
                                               <= 4.7e-15); solver rows 1.1e-15 of 1e-9, the oracle's 4 iterations with its step lengths
    d. OPS3 on the one-wave route     1.9e-14  (the cotangent unit, T = 1)
    e. OPS5 SysID                     2.7e-14  (sysid_step gradient, T = 33)
    f. OPS5 ControlPlanning           1.9e-15  Lagrange (rollout_vjp grad_x0, T = 49), 2.5e-15 network (rollout_vjp grad_theta, T = 49)
No entry point disagreed with its reference: the device pow at negative bases, the rewritten divisions and the hoisted values are as the host computes them.

The five model libraries are compiled on first use (about a minute of hipcc each, side by side in `built`), which is host time."""
import os
import sys
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import frontend_ops_common as c  # noqa: E402
import tile_edge_common as te  # noqa: E402

MODES = (False, True)            # shared theta, per-sample theta


def npy(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def built():
    """{(name, kind): library path}: the five model libraries, compiled side by side where they are not there yet (content-hash cache of codegen.build_problem)"""
    from pdp_amd import codegen
    res = codegen.build_many([c.problem(name, kind) for name, kind in c.LIBRARIES], workers=len(c.LIBRARIES))
    return {key: lib for key, (lib, _) in zip(c.LIBRARIES, res)}


@pytest.fixture(scope="module")
def models(built):
    """{(name, kind): (class-surface object, ModelLib)}, each library loaded once"""
    out = {}
    for name, kind in c.LIBRARIES:
        obj = c.model_gpu(name, kind)
        out[name, kind] = (obj, obj.model())
        assert out[name, kind][1].path == built[name, kind]
    return out


class _Worst(c.Worst):
    """frontend_ops_common.Worst (a NaN comes in and stays), printed and then held to the bound through `margins`"""

    def check(self, margins, tag, bound=c.TOL):
        for quantity, (value, where) in self.v.items():
            print("%s: %s %.3e at %s" % (tag, quantity, value, where))
        for quantity, (value, where) in self.v.items():
            margins.check("frontend ops %s: %s" % (tag, quantity), value, bound)


@pytest.fixture(autouse=True)
def no_kernel_by_kernel_route():
    """the fused OC unit announces the kernel-by-kernel route it takes beyond its limits with a RuntimeWarning: an error in every test of this module (the SysID and
    ControlPlanning entry points have no such announcement: their tests assert the sizes and rows that keep them on the tuned kernels)"""
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*kernel-by-kernel route.*")
        yield


# ---- a. the operator table ------------------------------------------------------------------------------------------------------------------------------------
def test_operator_table_entry_by_entry(models, margins):
    mdl = models["OPT", "oc"][1]
    n, m, p = c.MODELS["OPT"]
    P = c.opt_points()
    B = P["B"]
    xg = np.stack([P["x0"], P["x1"]], axis=1)                    # the given trajectory: matrices at (x0, u, lam), the final cost's at x1
    worst = _Worst()
    for per_sample in MODES:
        th = P["theta_b"] if per_sample else P["theta"]
        x, cost = mdl.oc_rollout(P["x0"], P["u"], th)
        lam = mdl.oc_costate(xg, P["u"], th)
        aux = {k: npy(v) for k, v in mdl.oc_auxsys(xg, P["u"], P["lam"], th).items()}
        x, cost, lam = npy(x), npy(cost), npy(lam)
        assert np.array_equal(x[:, 0], P["x0"])
        for b in range(B):
            w = th[b] if per_sample else th
            at = "%s theta, row %d" % ("per-sample" if per_sample else "shared", b)
            e0 = c.exact("OPT", "oc", P["x0"][b], P["u"][b, 0], P["lam"][b, 0], w)
            e1 = c.exact("OPT", "oc", P["x1"][b], P["u"][b, 0], P["lam"][b, 0], w, final_only=True)
            ef = c.exact("OPT", "oc", e0["dyn"][0][:, 0], P["u"][b, 0], P["lam"][b, 0], w, final_only=True)             # the final cost at the rollout's own end point
            worst.add("oc_rollout x_1 = op(x_0)", c.entry_err(x[b, 1], e0["dyn"][0][:, 0], e0["dyn"][1][:, 0]), at)
            want_cost = e0["path_cost"][0][0, 0] + ef["final_cost"][0][0, 0]
            worst.add("oc_rollout cost", abs(cost[b] - want_cost) / abs(want_cost), at)
            worst.add("oc_costate lam_1 = dh/dx(x_1)", c.entry_err(lam[b, 0], e1["dhx"][0][:, 0], e1["dhx"][1][:, 0]), at)
            for k, key in (("dynF", "F"), ("dynG", "G"), ("dynE", "E"), ("Hxx", "Hxx"), ("Hxu", "Hxu"), ("Hxe", "Hxe"), ("Huu", "Huu"), ("Hue", "Hue")):
                worst.add("oc_auxsys " + k, c.entry_err(aux[k][b, 0], *e0[key]), at)
            worst.add("oc_auxsys Hux", c.entry_err(aux["Hux"][b, 0], e0["Hxu"][0].T, e0["Hxu"][1].T), at)
            for k in ("hxx", "hxe"):
                worst.add("oc_auxsys " + k, c.entry_err(aux[k][b], *e1[k]), at)
            # odd powers at negative bases: d2/dx2 x^7 = 42 x^5 and d2/dx2 x^-3 = 12 x^-5 are the whole of H_xx[9, 9] and H_xx[10, 10] (their dynamics rows are linear in x)
            for i in (9, 10):
                h = aux["Hxx"][b, 0][i, i]
                assert np.isfinite(h) and np.sign(h) == np.sign(P["x0"][b, i]), (at, i, h, P["x0"][b, i])
    worst.check(margins, "OPT T=1, per entry")


# ---- b. - d. the OC models ------------------------------------------------------------------------------------------------------------------------------------
AUX_T = ("dynF", "dynG", "dynE", "Hxx", "Hxu", "Hxe", "Hux", "Huu", "Hue")


def _model_evaluation(mdl, name, T, worst):
    inp = c.unit_inputs(name, T)
    for per_sample in MODES:
        th = inp["theta_b"] if per_sample else inp["theta"]
        os_ = [c.unit_oracle(name, T, per_sample, b) for b in range(c.B)]
        xo, lo = np.stack([o["state_traj"] for o in os_]), np.stack([o["costate_traj"] for o in os_])
        x, cost = mdl.oc_rollout(inp["x0"], inp["u"], th)
        lam = npy(mdl.oc_costate(xo, inp["u"], th))
        aux = {k: npy(v) for k, v in mdl.oc_auxsys(xo, inp["u"], lo, th).items()}
        x, cost = npy(x), npy(cost)
        orc = c.model_oracle(name)
        for b in range(c.B):
            at = "%s theta, sample %d" % ("per-sample" if per_sample else "shared", b)
            worst.add("oc_rollout x vs OCSysOracle.rollout", c.rel(x[b], xo[b]), at)
            want = orc.cost(xo[b], inp["u"][b], c.theta_of(inp, per_sample, b))
            worst.add("oc_rollout cost vs OCSysOracle.cost (relative)", abs(cost[b] - want) / abs(want), at)
            worst.add("oc_costate vs OCSysOracle.costate", c.rel(lam[b], lo[b]), at)
            for k in AUX_T:
                worst.add("oc_auxsys %s vs getAuxSys" % k, c.rel(aux[k][b], np.stack(os_[b]["aux"][k])), at)
            for k in ("hxx", "hxe"):
                worst.add("oc_auxsys %s vs getAuxSys" % k, c.rel(aux[k][b], os_[b]["aux"][k][0]), at)


def _fused_unit(mdl, name, T, worst):
    import oc_x0_vjp_common as cx
    inp = c.unit_inputs(name, T)
    orc = c.model_oracle(name)
    for per_sample in MODES:
        th = inp["theta_b"] if per_sample else inp["theta"]
        d = mdl.oc_pdp_grad(inp["u"], th, inp["demo_x"], inp["demo_u"], x0=inp["x0"], want_sens=True)
        pl = mdl.oc_pdp_grad(inp["u"], th, inp["demo_x"], inp["demo_u"], x0=inp["x0"])
        v = mdl.oc_pdp_vjp(inp["u"], th, inp["gx"], inp["gu"], x0=inp["x0"], want_ini=True)
        d, pl, v = ({k: npy(t) for k, t in r.items()} for r in (d, pl, v))
        assert not d["status"].any() and not pl["status"].any() and not v["status"].any()
        for b in range(c.B):
            at = "%s theta, sample %d" % ("per-sample" if per_sample else "shared", b)
            o = c.unit_oracle(name, T, per_sample, b)
            X, U = np.stack(o["lqr"]["state_traj_opt"]), np.stack(o["lqr"]["control_traj_opt"])
            for r in (d, pl, v):
                worst.add("unit x vs OCSysOracle.rollout", c.rel(r["x"][b], o["state_traj"]), at)
                worst.add("unit lam vs OCSysOracle.costate", c.rel(r["lam"][b], o["costate_traj"]), at)
            for r in (d, pl):
                worst.add("loss vs irl_loss_grad (relative)", abs(r["loss"][b] - o["loss"]) / o["loss"], at)
                worst.add("gradient vs irl_loss_grad", c.rel(r["grad"][b], o["grad"]), at)
            worst.add("dxdp vs the oracle's X", c.rel(d["dxdp"][b], X), at)
            worst.add("dudp vs the oracle's U", c.rel(d["dudp"][b], U), at)
            Xe, Ue = c.unit_exact(name, T, per_sample, b)
            worst.add("dxdp vs the 40-digit X", c.rel(d["dxdp"][b], Xe), at)
            worst.add("dudp vs the 40-digit U", c.rel(d["dudp"][b], Ue), at)
            gx = inp["gx"][b].copy()
            gx[0] = 0.0                                                                                    # X_0 = 0: gx_0 does not enter the parameter gradient
            worst.add("cotangent unit vs the oracle's sensitivities contracted with the same cotangents",
                      c.rel(v["grad"][b], np.einsum("ti,tip->p", gx, X) + np.einsum("ti,tip->p", inp["gu"][b], U)), at)
            ref0 = cx.reference_grad_x0(orc, o["state_traj"], inp["u"][b], o["costate_traj"], c.theta_of(inp, per_sample, b), inp["gx"][b], inp["gu"][b], aux=o["aux"])
            worst.add("cotangent unit's grad_x0 vs the forward sensitivities from X_0 = I contracted", c.rel(v["grad_x0"][b], ref0), at)


@pytest.mark.parametrize("T", c.unit_horizons("OPS5"))
def test_ops5_model_evaluation_follows_the_oracle(models, margins, T):
    worst = _Worst()
    _model_evaluation(models["OPS5", "oc"][1], "OPS5", T, worst)
    worst.check(margins, "OPS5 OC T=%d" % T)


@pytest.mark.parametrize("T", c.unit_horizons("OPS5"))
def test_ops5_fused_unit_follows_the_oracle(models, margins, T):
    info = c.generated_info("OPS5")
    assert te.fused3_ok(info, T) and te.fused_accepts(info, T)              # the runner / evaluator kernels
    if T > 7:
        assert len(te.backward_chunks(info, T)) == 2
    worst = _Worst()
    _fused_unit(models["OPS5", "oc"][1], "OPS5", T, worst)
    worst.check(margins, "OPS5 OC unit T=%d" % T)


def test_ops5_solver_reaches_the_oracles_optimum(models, margins):
    mdl = models["OPS5", "oc"][1]
    x0 = c.solver_x0()[[0, 1, 0]]
    sol = mdl.oc_solve_ms(x0, c.solver_theta(), c.SOLVER_T, tol=1e-10, log_rows=c.MAX_ITER_ORACLE + 5)
    got = {k: npy(sol[k]) for k in ("state", "control", "costate", "iterations", "status", "converged", "log")}
    for b, row in enumerate((0, 1, 0)):
        ref, log = c.solver_oracle(row)
        te.judge_solve(margins, "OPS5 w7=%g" % c.W7_SOLVER, got, b, ref, log, prefix="frontend ops solver")          # the tolerances of tests/test_gpu_tile_edge.py's solver rows
    for k in ("state", "control", "costate", "iterations", "log"):
        assert np.array_equal(got[k][0], got[k][2]), k


@pytest.mark.parametrize("T", c.unit_horizons("OPS3"))
def test_ops3_on_the_small_system_route(models, margins, built, T):
    from pdp_amd import codegen
    info = c.generated_info("OPS3")
    assert info["n"] <= 4 and not te.fused3_ok(info, T) and te.fused_accepts(info, T)
    kernels = set(codegen.kernel_resources(built["OPS3", "oc"]))
    assert any(k.startswith("oc_pdp_fused_kernel<") for k in kernels) and not any(k.startswith("oc_pdp_fused3_kernel<") for k in kernels), sorted(kernels)
    big = set(codegen.kernel_resources(built["OPS5", "oc"]))
    assert any(k.startswith("oc_pdp_fused3_kernel<") for k in big)          # (the check can tell them apart)
    worst = _Worst()
    _model_evaluation(models["OPS3", "oc"][1], "OPS3", T, worst)
    _fused_unit(models["OPS3", "oc"][1], "OPS3", T, worst)
    worst.check(margins, "OPS3 OC T=%d" % T)


# ---- e. OPS5 as SysID -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", c.sysid_horizons())
def test_ops5_as_sysid_follows_the_oracle(models, margins, T):
    mdl = models["OPS5", "sysid"][1]
    n, m, p = mdl.n, mdl.m, mdl.p
    assert (n, m, p) == (5, 2, c.SYSID_P)
    if T > 7:
        assert T == mdl.sysid_jvp_rows(c.B) + 1 == mdl.sysid_vjp_u_rows(c.B) + 1           # one step past the pool rows: a second pass of one step
    cs = c.sysid_case(T)
    worst = _Worst()
    for per_sample in MODES:
        th = cs["theta_b"] if per_sample else cs["theta"]
        refs = [c.sysid_reference(T, per_sample, b) for b in range(c.B)]
        xo = np.stack([r["x"] for r in refs])
        x = npy(mdl.sysid_integrate(cs["x0"], cs["inputs"], th))
        F, E = (npy(a) for a in mdl.sysid_auxsys(xo, cs["inputs"], th))
        loss, grad = (npy(a) for a in mdl.sysid_step(cs["inputs"], cs["xobs"], th))
        gn = {k: npy(v) for k, v in mdl.sysid_step(cs["inputs"], cs["xobs"], th, gauss_newton=True).items()}
        vjp = {k: npy(v) for k, v in mdl.sysid_rollout_vjp(xo, cs["inputs"], th, cs["g"], want_inputs=True).items()}
        d_x = npy(mdl.sysid_rollout_jvp(xo, cs["inputs"], th, d_theta=cs["d_theta"], d_x0=cs["d_x0"], d_u=cs["d_u"]))
        for b, r in enumerate(refs):
            at = "%s theta, sample %d" % ("per-sample" if per_sample else "shared", b)
            worst.add("sysid_integrate vs integrateDyn", c.rel(x[b], r["x"]), at)
            worst.add("sysid_auxsys F vs getAuxSys", c.rel(F[b], r["F"]), at)
            worst.add("sysid_auxsys E vs getAuxSys", c.rel(E[b], r["E"]), at)
            for l, g in ((loss, grad), (gn["loss"], gn["grad"])):
                worst.add("sysid_step loss (relative)", abs(l[b] - r["loss"]) / r["loss"], at)
                worst.add("sysid_step gradient vs the forward sensitivities", c.rel(g[b], r["grad"]), at)
            worst.add("sysid_step Gauss-Newton matrix vs X'X", c.rel(gn["gn"][b], r["gn"]), at)
            worst.add("sysid_rollout_vjp grad_theta", c.rel(vjp["grad_theta"][b], r["grad_theta"]), at)
            worst.add("sysid_rollout_vjp grad_x0", c.rel(vjp["grad_x0"][b], r["grad_x0"]), at)
            worst.add("sysid_rollout_vjp grad_u vs sympy's G propagated forward", c.rel(vjp["grad_u"][b], r["grad_u"]), at)
            worst.add("sysid_rollout_jvp d_x vs the forward sensitivities contracted", c.rel(d_x[b], r["d_x"]), at)
    worst.check(margins, "OPS5 SysID T=%d" % T)


# ---- f. OPS5 as ControlPlanning -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", c.cp_horizons())
@pytest.mark.parametrize("policy", ("poly", "mlp"))
def test_ops5_as_control_planning_follows_the_oracle(models, margins, policy, T):
    cp = c.cp_model_gpu(policy, T)
    cp._model = models["OPS5", "cp"][1]                     # the library loaded once
    cs = c.cp_case(policy, T)
    assert cp.n_auxvar == cs["p"]
    if T > 7:
        assert T == cp.model().cp_vjp_rows() + 1
    worst = _Worst()
    for per_sample in MODES:
        th = cs["theta_b"] if per_sample else cs["theta"]
        refs = [c.cp_reference(policy, T, per_sample, b) for b in range(c.B)]
        xo, uo = np.stack([r["x"] for r in refs]), np.stack([r["u"] for r in refs])
        x, u, cost = (npy(a) for a in cp.integrateSys_batch(cs["x0"], T, th))
        aux = {k: npy(v) for k, v in cp.getAuxSys_batch(xo, uo, th).items()}
        loss, grad = (npy(a) for a in cp.step_batch(cs["x0"], T, th))
        vjp = {k: npy(v) for k, v in cp.rollout_vjp_batch(xo, th, cs["gx"], cs["gu"]).items()}
        jvp = {k: npy(v) for k, v in cp.rollout_jvp_batch(xo, uo, th, d_auxvar=cs["d_theta"], d_ini_state=cs["d_x0"]).items()}
        for b, r in enumerate(refs):
            at = "%s theta, sample %d" % ("per-sample" if per_sample else "shared", b)
            worst.add("integrateSys x", c.rel(x[b], r["x"]), at)
            worst.add("integrateSys u", c.rel(u[b], r["u"]), at)
            worst.add("integrateSys cost (relative)", abs(cost[b] - r["cost"]) / abs(r["cost"]), at)
            for k in ("dynF", "dynG", "dUx", "dUe"):
                want = np.stack([np.asarray(a, float) for a in r["aux"][k]])
                if np.abs(want).max() == 0:                  # d pi/dx of the Lagrange policy
                    assert not aux[k][b].any(), (k, at)
                else:
                    worst.add("getAuxSys " + k, c.rel(aux[k][b], want), at)
            for k in ("dcx", "dcu", "dhx"):
                worst.add("getAuxSys " + k, c.rel(aux[k][b], r[k]), at)
            worst.add("step loss (relative)", abs(loss[b] - r["cost"]) / abs(r["cost"]), at)
            worst.add("step gradient vs ControlPlanningOracle.step", c.rel(grad[b], r["step_grad"]), at)
            worst.add("rollout_vjp grad_theta", c.rel(vjp["grad_theta"][b], r["grad_theta"]), at)
            worst.add("rollout_vjp grad_x0", c.rel(vjp["grad_x0"][b], r["grad_x0"]), at)
            worst.add("rollout_jvp d_state", c.rel(jvp["d_state"][b], r["d_state"]), at)
            worst.add("rollout_jvp d_control", c.rel(jvp["d_control"][b], r["d_control"]), at)
    worst.check(margins, "OPS5 CP %s T=%d" % (policy, T))
