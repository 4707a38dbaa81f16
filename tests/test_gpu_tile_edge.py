"""GPU: the fused OC unit (pdp_oc_pdp_grad*_batched) and the multiple-shooting solver (pdp_oc_solve_ms_batched) at the far end of the sizes they advertise - the three
models of tests/tile_edge_common.py:  E16 (n, m, p) = (16, 4, 12): the solver's non-homogeneous form (every `if constexpr (!AUG)` branch of pdp_ocsolve2_kernels.h
exists for n = 16 only), no padding row in any state tile;  E15 (15, 3, 13): a full augmented tile, NA = 16;  E5 (5, 1, 15): the first size past the small-system
kernels, one control under the pair kernels.  All three fill the [control | parameter] tile to its last column (m + p = 16; 17 is refused).

The kernel-selecting variables are read once per process, so the kernels run in child processes that save an .npz (`_worker`):
    default    PDP_FUSED_VARIANT=3, PDP_MS_VARIANT=2: the runner / evaluator kernels, one trajectory per workgroup at these batch sizes - and the one launch of E16 at
               B = 2 CUs + 1, four per workgroup
    tpw2/tpw4  PDP_FUSED_TPW=2 / 4: B = 5 leaves the last workgroup ragged
    one_wave   PDP_FUSED_VARIANT=1, PDP_MS_VARIANT=1: the one-wave kernels
Fused unit: every model x horizon (1, 7, ROWS + 6, ROWS + 7: the last two span two backward chunks) x {shared, per-sample theta} x {rollout, given trajectory}, B = 5,
every sample against oracle.pdp_oc_unit on the same inputs.  Solver: every model x regime, B = 3, row by row against oracle.ipopt_ms.solve.
tests/test_tile_edge_inputs.py holds the conditions that make these comparisons mean something (the oracle's own rounding error is below 1e-15 here).
tests/test_gpu_tile_edge_modes.py runs the unit's masked, weighted / Huber and initial-state modes on the same models, and these calls again, at horizons on both sides of
every forward chunk (none of the four horizons here spans two forward chunks).

Tolerance: 1e-10 relative to the largest entry of the compared array, per sample, through the `margins` fixture - one line per (variant, model,
horizon, quantity) with the largest figure over theta modes, trajectory modes and samples; the loss to 1e-12 relative; the solver as
tests/test_gpu_ocsolver.py::_follows: same iteration count, same step lengths, dw to 1e-12, f / inf_pr / theta to 1e-9, state / control / costate to 1e-9 of the largest
entry.  The points predicted from the packed fp32 record are held to fp32 accuracy of the correction, as in tests/test_gpu_predict.py.

The models are compiled on first use (about a minute of hipcc each; `built` compiles the three side by side), which is host time."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import tile_edge_common as c  # noqa: E402

NAMES = sorted(c.MODELS)
UNIT_MODES = ("default", "tpw2", "tpw4", "one_wave")
ENV = {"default": dict(PDP_FUSED_VARIANT="3", PDP_MS_VARIANT="2"), "tpw2": dict(PDP_FUSED_VARIANT="3", PDP_FUSED_TPW="2"), "tpw4": dict(PDP_FUSED_VARIANT="3", PDP_FUSED_TPW="4"),
       "one_wave": dict(PDP_FUSED_VARIANT="1", PDP_MS_VARIANT="1")}
LOG_ROWS = c.MAX_ITER_ORACLE + 5
SOLVER_BATCH = (0, 1, 0)                    # rows of solver_inputs()["x0"]: two initial states and a copy of the first


def npy(t):
    return t.detach().cpu().numpy()


def _cases(info, horizons=None):
    return [(T, per_sample, given) for T in (c.unit_horizons(info) if horizons is None else horizons) for per_sample in (False, True) for given in (False, True)]


# ---- child process ------------------------------------------------------------------------------------------------------------------------------------------
def _unit(out, name, oc, horizons=None):
    """every case of one model: the default unit (plain, and with the sensitivities and the Riccati record), the cotangent unit, the Gauss-Newton unit
    (horizons: tests/test_gpu_tile_edge_modes.py runs the same calls at its own)"""
    import torch
    from pdp_amd import runtime as rt
    n, m, p = c.MODELS[name]
    for T, per_sample, given in _cases(oc._model_info, horizons):
        inp = c.unit_inputs(name, T)
        B = inp["B"]
        th = inp["theta_b"] if per_sample else inp["theta"]
        u, dx, du = rt.dev(inp["u"]), rt.dev(inp["demo_x"]), rt.dev(inp["demo_u"])
        d0 = oc.pdp_grad_batch(u, th, dx, du, ini_state=inp["x0"])
        traj = lambda: dict(state_traj=d0["x"].clone(), costate_traj=d0["lam"].clone()) if given else dict(ini_state=inp["x0"])
        pl = oc.pdp_grad_batch(u, th, dx, du, **traj()) if given else d0
        ds = oc.pdp_grad_batch(u, th, dx, du, want_sens=True, want_riccati=True, **traj())
        cot = oc.pdp_vjp_batch(u, th, inp["gx"], inp["gu"], **traj())
        rows = torch.full((B + 1, p + 1 + p * p), float("nan"), dtype=torch.float64, device="cuda")
        gn = oc.pdp_grad_batch(u, th, dx, du, want_gauss_newton=True, buffers={"packed_gn": rows[:B]}, **traj())
        assert gn["packed_gn"].data_ptr() == rows.data_ptr()
        key = "%s_%d_%d_%d_" % (name, T, per_sample, given)
        for k, v in (("x", pl["x"]), ("lam", pl["lam"]), ("loss", pl["loss"]), ("grad", pl["grad"]), ("status", pl["status"]), ("xs", ds["x"]), ("lams", ds["lam"]),
                     ("losss", ds["loss"]), ("grads", ds["grad"]), ("statuss", ds["status"]), ("dxdp", ds["dxdp"]), ("dudp", ds["dudp"]), ("ric", ds["riccati"]),
                     ("cot", cot["grad"]), ("statusc", cot["status"]), ("rows", rows), ("statusg", gn["status"]), ("lossg", gn["loss"])):
            out[key + k] = npy(v)


def _solve(out, name, oc, mode):
    import torch
    mdl = oc.model()
    for reg in sorted(c.REGIMES):
        si = c.solver_inputs(name, reg)
        x0 = si["x0"][list(SOLVER_BATCH)]
        sol = mdl.oc_solve_ms(x0, si["theta"], si["T"], tol=1e-10, log_rows=LOG_ROWS)
        for k in ("state", "control", "costate", "iterations", "status", "converged", "log"):
            out["%s_%s_%s" % (name, reg, k)] = npy(sol[k])
        if mode != "default":
            continue
        # the class surface: the same call behind OCSys.ocSolver_batch
        cs = oc.ocSolver_batch(x0, si["T"], si["theta"])
        direct = mdl.oc_solve_ms(x0, si["theta"], si["T"], tol=1e-9 * 0.1)          # (ocsolver.solve_batch's tolerance for the kernel, to the bit)
        out["%s_%s_method_ms" % (name, reg)] = npy(cs["method_ms"])
        out["%s_%s_class_equal" % (name, reg)] = np.array([bool(torch.equal(cs[k], direct[k])) for k in ("state", "control", "costate")])
        out["%s_%s_class_state" % (name, reg)] = npy(cs["state"])
        if name == "E16":       # four trajectories per workgroup: oc_solve_ms2_kernel<PdpModel, 4, false>
            cus = torch.cuda.get_device_properties(0).multi_processor_count
            Bb = 2 * cus + 1
            big = mdl.oc_solve_ms(si["x0"][np.arange(Bb) % 2], si["theta"], si["T"], tol=1e-10, log_rows=LOG_ROWS)
            for k in ("state", "control", "costate", "iterations", "status", "converged", "log"):
                out["%s_%s_big_%s" % (name, reg, k)] = npy(big[k])
            out["cus"] = np.array(cus)
    # PDP_MS_FROM_CONTROLS | PDP_MS_WARM: an entry of the runner / evaluator kernel alone (PDP_E_SIZE where ms2_ok does not hold; any PDP_MS_VARIANT)
    si = c.solver_inputs(name, "a")
    fc = mdl.oc_solve_ms(si["x0"][list(SOLVER_BATCH)], si["theta"], si["T"], tol=1e-10, log_rows=LOG_ROWS, u_init=np.zeros((len(SOLVER_BATCH), si["T"], mdl.m)))
    for k in ("state", "control", "costate", "iterations", "status", "converged", "log"):
        out["%s_fc_%s" % (name, k)] = npy(fc[k])
    if mode == "default":
        # the predicted starting point at the optimum of regime (a): from the fp64 sensitivity outputs and from the packed fp32 record
        sol = mdl.oc_solve_ms(si["x0"][list(SOLVER_BATCH)], si["theta"], si["T"], tol=1e-11)
        B, p = len(SOLVER_BATCH), mdl.p
        g = mdl.oc_pdp_grad(sol["control"], si["theta"], sol["state"], sol["control"], x=sol["state"], lam=sol["costate"], want_sens=True, want_riccati=True,
                            want_predict_record=True)
        dth = si["theta"][None] * 0.02 * np.random.default_rng(3).uniform(-1, 1, (B, p))
        pred = mdl.oc_predict(sol["state"], sol["control"], sol["costate"], dth, g["dxdp"], g["dudp"], g["riccati"])
        prec = mdl.oc_predict_from_record(sol["state"], sol["control"], sol["costate"], dth, g["predict_record"])
        out["%s_pred_dth" % name], out["%s_pred_conv" % name] = dth, npy(sol["converged"])
        for k, v in zip(("x", "u", "lam", "x64", "u64", "lam64", "x32", "u32", "lam32"), (sol["state"], sol["control"], sol["costate"]) + tuple(pred) + tuple(prec)):
            out["%s_pred_%s" % (name, k)] = npy(v)


def _worker(mode):
    """runs in a child process whose environment selects the kernels; every entry point returned 0 (runtime.check raises otherwise)"""
    out = {}
    ocs = {name: c.model_gpu(name) for name in NAMES}
    for name in NAMES:
        ocs[name].model()                   # through the class surface; compiled by now (the `built` fixture), else on this first use
        info = ocs[name]._model_info
        assert (info["n"], info["m"], info["p"]) == c.MODELS[name] and c.ms2_ok(info) and all(c.fused3_ok(info, T) and c.fused_accepts(info, T) for T in c.unit_horizons(info))
    for name in NAMES:
        _unit(out, name, ocs[name])
        print("unit %s done" % name, flush=True)
    if mode in ("default", "one_wave"):
        for name in NAMES:
            _solve(out, name, ocs[name], mode)
            print("solver %s done" % name, flush=True)
    return out


# ---- parent -------------------------------------------------------------------------------------------------------------------------------------------------
_results, _stopped = {}, []


@pytest.fixture(scope="module")
def built():
    """the three model libraries, compiled side by side where they are not there yet (content-hash cache of codegen.build_problem)"""
    from concurrent.futures import ThreadPoolExecutor
    from pdp_amd import PDP, codegen

    def build(name):
        oc = c.model_gpu(name)
        pb = codegen.Problem(codegen.KIND_OC, oc.state, oc.control, oc.dyn, oc.auxvar, oc.path_cost, oc.final_cost, label=PDP._label(oc.project_name))
        return codegen.build_problem(pb)[0]
    with ThreadPoolExecutor(max_workers=3) as ex:
        return dict(zip(NAMES, ex.map(build, NAMES)))


@pytest.fixture(scope="module")
def run(built, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("tile_edge")

    def _run(mode):
        if mode not in _results:
            # a child that died (a fault, a time limit) ends the GPU work of this module: nothing more is started on the device
            assert not _stopped, "not started: the child process of mode %r failed before" % _stopped[0]
            f = os.path.join(str(tmp), mode + ".npz")
            code = ("import sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_tile_edge as m; np.savez(%r, **m._worker(%r))" % (ROOT, HERE, f, mode))
            env = {k: v for k, v in os.environ.items() if k not in ("PDP_FUSED_VARIANT", "PDP_FUSED_TPW", "PDP_MS_VARIANT")}
            try:
                r = subprocess.run([sys.executable, "-c", code], env=dict(env, **ENV[mode]), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
            except subprocess.TimeoutExpired:
                _stopped.append(mode)
                raise
            if r.returncode != 0:
                _stopped.append(mode)
            assert r.returncode == 0, "mode %s: exit %d\n%s" % (mode, r.returncode, r.stdout[-4000:])
            _results[mode] = dict(np.load(f))
        return _results[mode]
    return _run


class _Worst:
    """the largest figure per quantity over the cases of one (variant, model, horizon), and where it occurred"""

    def __init__(self):
        self.v = {}

    def add(self, quantity, value, where):
        prev = self.v.get(quantity)
        if prev is None or (prev[0] == prev[0] and not (value <= prev[0])):      # (a NaN comes in and stays)
            self.v[quantity] = (float(value), where)

    def check(self, margins, tag, bounds):
        for quantity, (value, where) in self.v.items():
            print("%s: %s %.3e at %s" % (tag, quantity, value, where))
        for quantity, (value, where) in self.v.items():
            margins.check("tile edge %s: %s" % (tag, quantity), value, bounds.get(quantity, c.TOL))


def _judge_unit(res, name, T, per_sample, given, worst):
    """one case, every sample, against oracle.pdp_oc_unit (rollout, costates, aux system, lqrSolver, the IRL chain rule of irl_loss_grad) on the same inputs"""
    n, m, p = c.MODELS[name]
    inp = c.unit_inputs(name, T)
    B = inp["B"]
    g = lambda k: res["%s_%d_%d_%d_%s" % (name, T, per_sample, given, k)]
    where = "%s theta, %s" % ("per-sample" if per_sample else "shared", "given trajectory" if given else "rollout")
    for k in ("status", "statuss", "statusc", "statusg"):
        assert not g(k).any(), (name, T, where, k, g(k))
    rows = g("rows")
    assert rows.shape == (B + 1, p + 1 + p * p) and np.isfinite(rows[:B]).all() and np.isnan(rows[B]).all(), (name, T, where)      # every entry written, nothing behind the last row
    G = rows[:B, p + 1:].reshape(B, p, p)
    assert np.array_equal(G, np.swapaxes(G, 1, 2)), (name, T, where)                                                              # the same products in the same order
    assert np.array_equal(g("lossg"), rows[:B, p])
    assert g("ric").shape == (B, T, n * n + n * p + 1)
    for b in range(B):
        o = c.unit_oracle(name, T, per_sample, b)
        X, U = np.stack(o["lqr"]["state_traj_opt"]), np.stack(o["lqr"]["control_traj_opt"])
        PP, WW = np.stack(o["lqr"]["PP"]), np.stack(o["lqr"]["WW"])
        at = "%s, sample %d" % (where, b)
        for k in ("x", "xs"):
            worst.add("x vs OCSysOracle.rollout", c.rel(g(k)[b], o["state_traj"]), at)
        for k in ("lam", "lams"):
            worst.add("lam vs OCSysOracle.costate", c.rel(g(k)[b], o["costate_traj"]), at)
        worst.add("dxdp vs the oracle's X", c.rel(g("dxdp")[b], X), at)
        worst.add("dudp vs the oracle's U", c.rel(g("dudp")[b], U), at)
        for k in ("loss", "losss", "lossg"):
            worst.add("loss vs irl_loss_grad (relative)", abs(g(k)[b] - o["loss"]) / o["loss"], at)
        for k, arr in (("grad", g("grad")), ("grads", g("grads")), ("rows", rows[:, :p])):
            worst.add("gradient vs irl_loss_grad", c.rel(arr[b], o["grad"]), at)
        ric = g("ric")[b]
        worst.add("Riccati record vs lqr_solver PP", c.rel(ric[:, :n * n].reshape(T, n, n), PP), at)
        worst.add("Riccati record vs lqr_solver WW", c.rel(ric[:, n * n:n * n + n * p].reshape(T, n, p), WW), at)
        gx = inp["gx"][b].copy()
        gx[0] = 0.0                                                                                    # X_0 = 0: gx_0 does not enter
        worst.add("cotangent unit vs the oracle's sensitivities contracted with the same cotangents",
                  c.rel(g("cot")[b], np.einsum("ti,tip->p", gx, X) + np.einsum("ti,tip->p", inp["gu"][b], U)), at)
        worst.add("Gauss-Newton block vs X'X + U'U of the oracle", c.rel(G[b], np.einsum("tip,tiq->pq", X, X) + np.einsum("tip,tiq->pq", U, U)), at)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("mode", UNIT_MODES)
def test_fused_unit_follows_the_oracle(run, margins, mode, name):
    res = run(mode)
    info = c.generated_info(name)
    for T in c.unit_horizons(info):
        worst = _Worst()
        for per_sample in (False, True):
            for given in (False, True):
                _judge_unit(res, name, T, per_sample, given, worst)
        worst.check(margins, "%s %s T=%d" % (mode, name, T), {"loss vs irl_loss_grad (relative)": 1e-12})


@pytest.mark.parametrize("name", NAMES)
def test_trajectories_per_workgroup_layouts_agree_to_the_bit(run, name):
    """one wave pair per trajectory whatever the workgroup: 1 (the batch rule at B = 5), 2 and 4 per workgroup - every output of every case, the NaN guard row included.

    This test found that the bits of a trajectory depended on the batch it was sent in: under hipcc's default -ffp-contract=fast, oc_pdp_fused3_kernel<PdpModel, 4, *>
    of E5 fused another product of c_x than <1> and <2> did, and the costate of q_1 differed in the last bit (2.2e-16 of 0.91: one sample in five at T = 7, per-sample
    theta; one entry of 1200 at T = 48) - with -ffp-contract=off the three agreed.  A user's model is now built with -ffp-contract=on (codegen.USER_MODEL_FLAGS: the
    source decides what is fused, the same in every instantiation).  Every output that differs is listed with the size of the difference."""
    a = run("default")
    differing = []
    for mode in ("tpw2", "tpw4"):
        b = run(mode)
        keys = [k for k in a if k.startswith(name + "_") and k.split("_")[1].isdigit()]
        assert len(keys) == 18 * len(_cases(c.generated_info(name)))
        for k in keys:
            cut = -1 if k.endswith("_ric") else None                    # (the record's last word per stage is scratch)
            x, y = a[k][..., :cut], b[k][..., :cut]
            if not np.array_equal(x, y, equal_nan=True):
                d = np.abs(x - y)
                differing.append("%s %s: %d of %d entries, largest difference %.3e of the largest entry %.3e" % (mode, k, int((d > 0).sum()), d.size, np.nanmax(d), np.nanmax(np.abs(x))))
    assert not differing, "\n".join(differing)


def _judge_solve(margins, tag, got, b, ref, log, worst=None):
    """tile_edge_common.judge_solve (shared with tests/test_gpu_frontend_ops.py): tests/test_gpu_ocsolver.py::_follows on row b of a solver result"""
    c.judge_solve(margins, tag, got, b, ref, log, worst)


def _solver_result(res, prefix):
    return {k: res["%s_%s" % (prefix, k)] for k in ("state", "control", "costate", "iterations", "status", "converged", "log")}


@pytest.mark.parametrize("reg", sorted(c.REGIMES))
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("mode", ("default", "one_wave"))
def test_solver_follows_the_oracle_iteration_by_iteration(run, margins, mode, name, reg):
    got = _solver_result(run(mode), "%s_%s" % (name, reg))
    rows = c.SOLVER_ROWS[name, reg]
    for b, src in enumerate(SOLVER_BATCH):
        ref, log = c.solver_oracle(name, reg, rows[src])
        _judge_solve(margins, "%s %s (%s)" % (mode, name, reg), got, b, ref, log)
    for k in ("state", "control", "costate", "iterations", "log"):      # equal inputs in two workgroups of one launch: equal bits
        assert np.array_equal(got[k][0], got[k][2]), k


@pytest.mark.parametrize("reg", sorted(c.REGIMES))
def test_solver_non_homogeneous_form_at_four_trajectories_per_workgroup(run, margins, reg):
    """E16 at B = 2 CUs + 1: oc_solve_ms2_kernel<PdpModel, 4, false> - the n = 16 form of the Newton step in the instantiation that runs out of registers (256 VGPRs,
    124 spilled) - every row against the oracle's solve of its initial state"""
    res = run("default")
    cus = int(res["cus"])
    got = _solver_result(res, "E16_%s_big" % reg)
    B = got["state"].shape[0]
    assert B == 2 * cus + 1 and c.traj_per_workgroup(B, cus) == 4 and c.traj_per_workgroup(len(SOLVER_BATCH), cus) == 1
    rows = c.SOLVER_ROWS["E16", reg]
    worst = _Worst()
    for b in range(B):
        ref, log = c.solver_oracle("E16", reg, rows[b % 2])
        _judge_solve(margins, "default E16 (%s) B=%d" % (reg, B), got, b, ref, log, worst)
    worst.check(margins, "solver default E16 (%s) B=2 CUs+1, four per workgroup" % reg, dict.fromkeys(worst.v, 1e-9))
    small = _solver_result(res, "E16_%s" % reg)
    same = all(np.array_equal(got[k][b], small[k][b % 2]) for k in ("state", "control", "costate") for b in range(B))
    print("E16 (%s): the rows at four per workgroup %s the rows at one per workgroup to the bit" % (reg, "equal" if same else "do not equal"))


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("mode", ("default", "one_wave"))
def test_solver_from_controls_entry_runs_the_pair_kernel(run, margins, mode, name):
    """PDP_MS_FROM_CONTROLS | PDP_MS_WARM returned 0 in the child (whatever PDP_MS_VARIANT says): the runner / evaluator kernel served these sizes; from zero controls, their
    rollout and the least-squares multipliers it follows the restatement started the same way"""
    from oracle import ipopt_ms
    got = _solver_result(run(mode), "%s_fc" % name)
    si = c.solver_inputs(name, "a")
    for b, src in enumerate(SOLVER_BATCH):
        log = []
        ref = ipopt_ms.solve(c.model_oracle(name), si["x0"][src], si["T"], si["theta"], tol=1e-10, log=log, u_init=np.zeros((si["T"], c.MODELS[name][1])))
        assert ref["restorations"] == 0 and log[0]["inf_pr"] <= 1e-12
        _judge_solve(margins, "%s %s from controls" % (mode, name), got, b, ref, log)


@pytest.mark.parametrize("name", NAMES)
def test_class_surface_reports_the_multiple_shooting_method(run, name):
    res = run("default")
    for reg in sorted(c.REGIMES):
        assert res["%s_%s_method_ms" % (name, reg)].all() and res["%s_%s_class_equal" % (name, reg)].all(), (name, reg)
        assert c.rel(res["%s_%s_class_state" % (name, reg)], res["%s_%s_state" % (name, reg)]) <= 1e-9      # ... and the solve the oracle comparison above is made on


@pytest.mark.parametrize("name", NAMES)
def test_predicted_start_matches_the_oracle(run, margins, name):
    """pdp_oc_predict_batched (fp64 sensitivities and Riccati record) and pdp_oc_predict_record_batched (packed fp32 record) at the optimum of regime (a), a 2 % parameter
    step per sample, against ipopt_ms.predict_start from the same point"""
    from oracle import ipopt_ms
    res = run("default")
    g = lambda k: res["%s_pred_%s" % (name, k)]
    assert g("conv").all()
    th = c.solver_inputs(name, "a")["theta"]
    oc = c.model_oracle(name)
    for b in range(len(SOLVER_BATCH)):
        ex, eu, el = ipopt_ms.predict_start(oc, g("x")[b], g("u")[b], g("lam")[b], th, g("dth")[b])
        for lab, e, base in (("x", ex, g("x")[b]), ("u", eu, g("u")[b]), ("lam", el, g("lam")[b])):
            margins.check("tile edge %s sample %d: point predicted from the fp64 outputs vs oracle predict_start, %s" % (name, b, lab), c.rel(g(lab + "64")[b], e), c.TOL)
            margins.check("tile edge %s sample %d: point predicted from the fp32 record vs oracle, %s (relative to the size of the correction)" % (name, b, lab),
                          np.abs(g(lab + "32")[b] - e).max() / np.abs(e - base).max(), 1e-5 if lab == "lam" else 1e-6)
        assert np.array_equal(g("x64")[b][0], g("x")[b][0])                                             # x_0 is fixed: X_0 = 0


def test_code_object_of_the_16_state_model_holds_the_pair_solver(built):
    """the instantiations the solver tests above ran exist in E16's library: one, two and four trajectories per workgroup"""
    from pdp_amd import codegen
    kernels = codegen.kernel_resources(built["E16"])
    assert {"oc_solve_ms2_kernel<%d,0>" % k for k in (1, 2, 4)} <= set(kernels)
    r = kernels["oc_solve_ms2_kernel<4,0>"]
    print("E16 oc_solve_ms2_kernel<4, false>: %d VGPRs, %d spilled, %d bytes of scratch" % (r["vgpr"], r["spill"], r["scratch"]))
