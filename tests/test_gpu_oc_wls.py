"""GPU: pdp_oc_pdp_grad_wls_batched - the fused OC / IRL unit as weighted and Huber-robust least squares (include/pdp_hip_oc_wls.h; ModelLib.oc_pdp_grad(weights_x=,
weights_u=, huber_delta=), OCSys.pdp_grad_batch(weights_state=, weights_control=, huber_delta=), LMLoop.for_irl / BatchedLMLoop.for_irl with the same keywords).

Shapes (tests/oc_vjp_common.make_inputs; those of tests/test_gpu_oc_missing.py): the smallest at which each kernel path can go wrong.  Runner / evaluator kernel (n > 4):
quadrotor at T = 41 - two chunks of unequal length - and T = 7, rocket at T = 31; B = 5 at 1, 2 and 4 trajectories per workgroup (PDP_FUSED_TPW, read once per process:
one child process each).  One-wave kernel (n <= 4): cart-pole at T = 70 and T = 7, pendulum (n = 2); B = 3; its n > 4 branch in a child process.  Weights, NaN marks and
delta: tests/oc_wls_common.py (weights 0 for certain where oc_missing_common.make_masks forces a gap, NaN on half of the zero-weight entries, under the flag also on
positive-weight ones; the last sample has every weight 0, the one before it weights 1 and no NaN; delta = the median of |e| over the observed entries).  Every shape runs
twice: weights and Huber (rows_h), and the weights alone (rows_w, delta = +inf).

Reference: the default unit's own want_sens=True outputs on the zero-filled demonstrations, scaled and contracted in torch fp64 exactly as the header's three formulas
state (oc_wls_common.contract_wls).  Tolerance: 1e-10 of the largest entry of the compared array, per sample - BASELINE.md section 3's GPU-vs-restatement tolerance on
identical inputs.  The CPU oracle is compared where tests/test_gpu_oc_vjp.py documents that its own rounding error is below that: quadrotor T = 41, rocket T = 31,
cart-pole and pendulum T = 7.  The Levenberg-Marquardt budgets are twice the evaluations the same schedule needs on the CPU oracle on the same corrupted demonstrations
(tests/test_oc_wls_host.py); traces are printed, not asserted."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)
TOL = 1e-10
INF = float("inf")

# (system, B, T, per-sample theta, given trajectory, PDP_GRAD_SKIP_MISSING with NaN on positive-weight entries too)
F3_CASES = [("quadrotor", 5, 41, False, False, False), ("quadrotor", 5, 41, True, True, True), ("quadrotor", 5, 7, True, False, True),
            ("rocket", 5, 31, False, True, False), ("rocket", 5, 31, True, False, True)]
F1_CASES = [("cartpole", 3, 70, False, False, False), ("cartpole", 3, 70, True, True, True), ("cartpole", 3, 7, True, False, True),
            ("pendulum", 3, 70, False, True, True), ("pendulum", 3, 7, True, False, False)]

WORKER = r'''
import os, sys
import numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(here)r)
import oc_vjp_common as c, oc_wls_common as ow
from pdp_amd import zoo
out = {}
for k, (system, B, T, per_sample, given, skip) in enumerate(%(cases)r):
    r = ow.evaluate(zoo.get(system, "irl"), c.make_inputs(system, B, T), per_sample, given, skip)
    for key, v in r.items():
        out["%%d_%%s" %% (k, key)] = v
np.savez(sys.argv[1], **out)
'''


def npy(t):
    return t.detach().cpu().numpy()


def _tag(case):
    system, B, T, per_sample, given, skip = case
    return "%s B=%d T=%d %s theta, %s%s" % (system, B, T, "per-sample" if per_sample else "shared", "given trajectory" if given else "rollout",
                                           ", skip_missing" if skip else "")


def _split(rows, B, p):
    return rows[:B, :p], rows[:B, p], rows[:B, p + 1:].reshape(B, p, p)


def _judge(margins, tag, r):
    """checks 1 - 6 of one shape, for the Huber call (h) and the weights-only call (w)"""
    import oc_wls_common as ow
    p = r["grad_ref_h"].shape[1]
    B = r["rows_h"].shape[0] - 1
    dark, ones = ow.dark_sample(B), ow.ones_sample(B)
    seen = [i for i in range(B) if i != dark]
    assert np.isfinite(r["delta"]) and r["delta"] > 0
    for v, what in (("h", "weights and Huber (delta %.3e)" % r["delta"]), ("w", "weights alone")):
        rows = r["rows_" + v]
        grad, loss, G = _split(rows, B, p)
        # 1. the rows were NaN before the call: every entry was written and is finite, and nothing behind the last row
        assert np.isfinite(rows[:B]).all(), (tag, v)
        assert np.isnan(rows[B]).all(), (tag, v)
        # 2. against the scaled contraction of the default unit's own sensitivities
        gr, lr, Gr = r["grad_ref_" + v], r["loss_ref_" + v], r["G_ref_" + v]
        assert all(np.abs(Gr[i]).max() > 0 and np.abs(gr[i]).max() > 0 and lr[i] > 0 for i in seen), (tag, v)
        margins.check("OC wls %s, %s: gradient vs contract_wls (per sample, relative to the largest entry)" % (tag, what), max(ow.rel(grad[i], gr[i]) for i in seen), TOL)
        margins.check("OC wls %s, %s: loss vs the sum of rho" % (tag, what), max(ow.rel(loss[i], lr[i]) for i in seen), TOL)
        margins.check("OC wls %s, %s: G vs einsum of the row-scaled sensitivities" % (tag, what), max(ow.rel(G[i], Gr[i]) for i in seen), TOL)
        # 3. both operands of every product are the same scaled tile: symmetric to the bit; positive semi-definite
        assert np.array_equal(G, np.swapaxes(G, 1, 2)), (tag, v)
        for i in seen:
            ev = np.linalg.eigvalsh(G[i])
            assert ev[0] >= -1e-12 * ev[-1], (tag, v, i, ev)
        # 4. nothing observed: exact zeros
        assert not rows[dark].any(), (tag, v)
        assert lr[dark] == 0.0 and not Gr[dark].any() and not gr[dark].any()
        # 6. trajectory, costates and status are the default call's
        assert not r["status_" + v].any() and np.array_equal(r["status_" + v], r["status0"]), (tag, v)
        assert np.array_equal(r["x_" + v], r["x_def"]) and np.array_equal(r["lam_" + v], r["lam_def"]), (tag, v)
    # 5. weights 1, no NaN, delta = +inf: the Gauss-Newton call (other instantiations: within the tolerance, bit-equality only reported)
    grad, loss, G = _split(r["rows_w"], B, p)
    ng, nl, nG = _split(r["gn_rows"], B, p)
    margins.check("OC wls %s, ones-sample at delta = inf: gradient vs gauss_newton=True" % tag, ow.rel(grad[ones], ng[ones]), TOL)
    margins.check("OC wls %s, ones-sample at delta = inf: loss vs gauss_newton=True" % tag, ow.rel(loss[ones], nl[ones]), TOL)
    margins.check("OC wls %s, ones-sample at delta = inf: G vs gauss_newton=True" % tag, ow.rel(G[ones], nG[ones]), TOL)
    print("OC wls %s, ones-sample at delta = inf bit-equal to gauss_newton=True: %s" % (tag, np.array_equal(r["rows_w"][ones], r["gn_rows"][ones])))


def _oracle_oc(name, _cache={}):
    from oracle import models, pdp_oracle as po
    if name not in _cache:
        st = models.IRL_SETUP[name]
        _cache[name] = po.make_oc(models.REGISTRY[name](**st["kwargs"]), st["dt"])
    return _cache[name]


def _judge_oracle(margins, tag, inp, r, per_sample, skip=False):
    """8. against the CPU oracle: the restatement of the reference's unit on the same inputs, its trajectory and sensitivities scaled and contracted (a weighted sample
    and the ones-sample)"""
    import oc_wls_common as ow
    from oracle import pdp_oracle as po
    oc = _oracle_oc(inp["system"])
    mi = ow.weight_inputs(inp, skip)
    B, p = inp["B"], r["grad_ref_h"].shape[1]
    for i in (0, ow.ones_sample(B)):
        th = inp["theta_b"][i] if per_sample else inp["theta"]
        unit = po.pdp_oc_unit(oc, inp["x0"][i], inp["u"][i], th, mi["demo_x0"][i], mi["demo_u0"][i])
        for v, delta in (("h", float(r["delta"])), ("w", INF)):
            grad, loss, G = _split(r["rows_" + v], B, p)
            lo, go, Go = ow.contract_wls_np(np.asarray(unit["state_traj"]), inp["u"][i], mi["demo_x0"][i], mi["demo_u0"][i], mi["ox"][i], mi["ou"][i], mi["wx"][i], mi["wu"][i],
                                            delta, np.stack(unit["lqr"]["state_traj_opt"]), np.stack(unit["lqr"]["control_traj_opt"]))
            margins.check("OC wls %s (%s) sample %d: loss vs oracle.pdp_oc_unit, scaled" % (tag, v, i), ow.rel(loss[i], lo), TOL)
            margins.check("OC wls %s (%s) sample %d: gradient vs oracle.pdp_oc_unit, scaled and contracted" % (tag, v, i), ow.rel(grad[i], go), TOL)
            margins.check("OC wls %s (%s) sample %d: G vs oracle.pdp_oc_unit sensitivities, row-scaled and contracted with themselves" % (tag, v, i), ow.rel(G[i], Go), TOL)


def test_runner_evaluator_kernel_at_1_2_4_trajectories_per_workgroup(margins, tmp_path):
    import oc_vjp_common as c
    results = {}
    for tpw in (1, 2, 4):                       # (stops at the first failing child: the assert ends the test)
        path = str(tmp_path / ("tpw%d.npz" % tpw))
        env = dict(os.environ, PDP_FUSED_TPW=str(tpw))
        env.pop("PDP_FUSED_VARIANT", None)
        r = subprocess.run([sys.executable, "-c", WORKER % dict(root=ROOT, here=HERE, cases=F3_CASES), path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                           timeout=300, env=env)
        assert r.returncode == 0, "PDP_FUSED_TPW=%d: %s" % (tpw, r.stdout[-3000:])
        z = np.load(path)
        for k, case in enumerate(F3_CASES):
            res = {key.split("_", 1)[1]: z[key] for key in z.files if key.startswith("%d_" % k)}
            _judge(margins, "fused3 TPW=%d %s" % (tpw, _tag(case)), res)
            results[tpw, k] = res
    # 7. one wave pair per trajectory whatever the workgroup: the three layouts agree to the bit (NaN guard rows included)
    for k in range(len(F3_CASES)):
        for key in ("rows_h", "rows_w"):
            assert np.array_equal(results[1, k][key], results[2, k][key], equal_nan=True) and np.array_equal(results[1, k][key], results[4, k][key], equal_nan=True), \
                (_tag(F3_CASES[k]), key)
    for k in (0, 4):                            # quadrotor T = 41 shared theta, rocket T = 31 per-sample theta under the flag
        system, B, T, per_sample, given, skip = F3_CASES[k]
        _judge_oracle(margins, "fused3 TPW=4 " + _tag(F3_CASES[k]), c.make_inputs(system, B, T), results[4, k], per_sample, skip)


@pytest.mark.parametrize("case", F1_CASES, ids=[_tag(cs).replace(" ", "_").replace(",", "") for cs in F1_CASES])
def test_one_wave_kernel(margins, case):
    import oc_vjp_common as c
    import oc_wls_common as ow
    from pdp_amd import zoo
    system, B, T, per_sample, given, skip = case
    inp = c.make_inputs(system, B, T)
    r = ow.evaluate(zoo.get(system, "irl"), inp, per_sample, given, skip)
    _judge(margins, "one-wave " + _tag(case), r)
    if T == 7:
        _judge_oracle(margins, "one-wave " + _tag(case), inp, r, per_sample, skip)


def test_one_wave_kernel_beyond_four_states(margins, tmp_path):
    """the one-wave kernel's n > 4 branch in PDP_FUSED_GN_W (oc_vjp_common.run_one_wave_beyond_four_states: quadrotor T = 41 rollout, rocket T = 31 given trajectory)"""
    import oc_vjp_common as c
    c.run_one_wave_beyond_four_states(margins, tmp_path, WORKER, F3_CASES, _judge, _judge_oracle, _tag)


def test_variants_shared_blocks_one_side_only_and_huber_only(margins):
    """each at one shape (quadrotor B = 5, T = 7, the runner / evaluator kernel; cart-pole B = 3, T = 7, the one-wave kernel): ONE weight block shared by the batch
    (stride 0), only weights_x, only weights_u, only huber_delta - a NULL weights pointer is all ones"""
    import torch
    import oc_vjp_common as c
    import oc_wls_common as ow
    from pdp_amd import runtime as rt, zoo
    for system, B, T in (("quadrotor", 5, 7), ("cartpole", 3, 7)):
        mdl = zoo.get(system, "irl")
        p = mdl.p
        mi = ow.weight_inputs(c.make_inputs(system, B, T), False)
        u, x0, dx0, du0 = rt.dev(mi["u"]), mi["x0"], rt.dev(mi["demo_x0"]), rt.dev(mi["demo_u0"])
        ds = mdl.oc_pdp_grad(u, mi["theta"], dx0, du0, x0=x0, want_sens=True)
        wx1, wu1 = mi["wx"][0], mi["wu"][0]                                        # one block [T+1, n] / [T, m] for every sample
        for name, wx, wu, huber in (("shared blocks", wx1, wu1, True), ("shared component weights", wx1[T], wu1[1], False), ("only weights_x", mi["wx"], None, True),
                                    ("only weights_u", None, mi["wu"], False), ("only huber_delta", None, None, True)):
            full = lambda w, ref: None if w is None else np.broadcast_to(w, ref.shape)
            fx, fu = full(wx, mi["demo_x"]), full(wu, mi["demo_u"])
            m2 = dict(mi, wx=np.ones(mi["demo_x"].shape) if fx is None else fx, wu=np.ones(mi["demo_u"].shape) if fu is None else fu)
            m2["ox"], m2["ou"] = m2["wx"] > 0, m2["wu"] > 0
            delta = ow.median_delta(npy(ds["x"]), mi["u"], m2) if huber else INF
            ref = ow.contract_wls(ds["x"], u, dx0, du0, torch.as_tensor(m2["ox"], device="cuda"), torch.as_tensor(m2["ou"], device="cuda"), rt.dev(m2["wx"]), rt.dev(m2["wu"]),
                                  delta, ds["dxdp"], ds["dudp"])
            rows = torch.full((B + 1, p + 1 + p * p), float("nan"), dtype=torch.float64, device="cuda")
            g = mdl.oc_pdp_grad(u, mi["theta"], dx0, du0, x0=x0, weights_x=wx, weights_u=wu, huber_delta=delta if huber else None, buffers={"packed_gn": rows[:B]})
            out = npy(rows)
            assert np.isfinite(out[:B]).all() and np.isnan(out[B]).all() and int(g["status"].sum()) == 0, (system, name)
            grad, loss, G = _split(out, B, p)
            lr, gr, Gr = (npy(t) for t in ref)
            seen = [i for i in range(B) if Gr[i].any()]
            assert len(seen) >= B - 1, (system, name)
            margins.check("OC wls %s T=7, %s: gradient" % (system, name), max(ow.rel(grad[i], gr[i]) for i in seen), TOL)
            margins.check("OC wls %s T=7, %s: loss" % (system, name), max(ow.rel(loss[i], lr[i]) for i in seen), TOL)
            margins.check("OC wls %s T=7, %s: G" % (system, name), max(ow.rel(G[i], Gr[i]) for i in seen), TOL)
            assert np.array_equal(G, np.swapaxes(G, 1, 2)), (system, name)
            for i in range(B):
                if i not in seen:
                    assert not out[i].any(), (system, name, i)


def test_beyond_the_fused_limits_the_materialised_route_fills_the_same_rows(margins):
    """PDP_E_SIZE from the entry point: the kernel-by-kernel route, the sensitivities through HBM, scaled and contracted with torch.einsum into the same rows"""
    import torch
    import oc_wls_common as ow
    from pdp_amd import runtime as rt
    from test_gpu_oc_missing import _wide_auxvar_oc
    oc, th, rng = _wide_auxvar_oc()
    n, m, p, T, B = 6, 2, 16, 9, 2
    x0, u = 0.5 * rng.standard_normal((B, n)), 0.3 * rng.standard_normal((B, T, m))
    inp = dict(B=4, T=T, demo_x=np.zeros((4, T + 1, n)), demo_u=np.zeros((4, T, m)))
    inp["demo_x"][:B], inp["demo_u"][:B] = 0.1 * rng.standard_normal((B, T + 1, n)), 0.1 * rng.standard_normal((B, T, m))
    mi = {k: (v[:B] if isinstance(v, np.ndarray) else v) for k, v in ow.weight_inputs(inp, True).items()}      # (samples 0 and 1 of four: both weighted and marked)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        ref = oc.pdp_grad_batch(u, th, mi["demo_x0"], mi["demo_u0"], ini_state=x0, want_sens=True)
        delta = ow.median_delta(npy(ref["x"]), u, mi)
        out = oc.pdp_grad_batch(u, th, mi["demo_xm"], mi["demo_um"], ini_state=x0, skip_missing=True, weights_state=mi["wx"], weights_control=mi["wu"], huber_delta=delta)
    loss_ref, grad_ref, G_ref = (npy(t) for t in ow.contract_wls(ref["x"], rt.dev(u), rt.dev(mi["demo_x0"]), rt.dev(mi["demo_u0"]), torch.as_tensor(mi["ox"], device="cuda"),
                                                                 torch.as_tensor(mi["ou"], device="cuda"), rt.dev(mi["wx"]), rt.dev(mi["wu"]), delta, ref["dxdp"], ref["dudp"]))
    row = out["packed_gn"]
    assert row.shape == (B, p + 1 + p * p) and out["gn"].shape == (B, p, p) and int(out["status"].sum()) == 0 and bool(torch.isfinite(row).all())
    assert torch.equal(row[:, :p], out["grad"]) and torch.equal(row[:, p], out["loss"]) and torch.equal(row[:, p + 1:].reshape(B, p, p), out["gn"])
    margins.check("OC wls beyond the fused limits (n=6 m=2 p=16): G vs contract_wls", max(ow.rel(npy(out["gn"])[i], G_ref[i]) for i in range(B)), TOL)
    margins.check("OC wls beyond the fused limits: gradient", max(ow.rel(npy(out["grad"])[i], grad_ref[i]) for i in range(B)), TOL)
    margins.check("OC wls beyond the fused limits: loss", max(ow.rel(npy(out["loss"])[i], loss_ref[i]) for i in range(B)), TOL)
    assert torch.equal(out["x"], ref["x"]) and torch.equal(out["lam"], ref["lam"])


# ---- Levenberg-Marquardt on the corrupted demonstrations of tests/oc_wls_common.corrupted, beside the oracle schedule of tests/test_oc_wls_host.py
def _err(theta, c):
    return float(np.abs(np.asarray(theta) - c["true_parameter"]).max())


@pytest.mark.parametrize("system", ["pendulum", "cartpole"])
def test_lm_loops_with_weight_zero_on_the_corrupted_entries(system):
    """the clean problem again: at most twice the oracle's evaluations, final loss <= 1e-10 - LMLoop, BatchedLMLoop with all demonstrations as one problem, and
    BatchedLMLoop with one problem per demonstration (the oracle's counts per demonstration)"""
    import oc_wls_common as ow
    from pdp_amd import zoo
    from pdp_amd.irl import BatchedLMLoop, LMLoop
    c, mdl = ow.corrupted(system), zoo.get(system, "irl")
    B = c["demo_x"].shape[0]
    kw = dict(weights_state=c["trust_x"], weights_control=c["trust_u"])
    budget = 2 * ow.TRUST_COUNTS[system]
    r = LMLoop.for_irl(mdl, c["demo_x"], c["demo_u"], c["theta0"], **kw).run(max_evals=budget, loss_tol=1e-16)
    print("%s LMLoop, weight 0 on %s corrupted entries: losses" % (system, ow.CORRUPTED_ENTRIES[system]), r["loss_trace"], "evaluations", r["evaluations"], "rejected",
          r["rejected"], "theta error %.2e" % _err(r["parameter_trace"][-1], c))
    assert r["evaluations"] <= budget and r["loss_trace"][-1] <= 1e-10 and (np.diff(r["loss_trace"]) < 0).all()
    rb = BatchedLMLoop.for_irl(mdl, c["demo_x"], c["demo_u"], c["theta0"], samples_per_problem=B, max_evals=budget, loss_tol=1e-16, **kw).run()
    print("%s BatchedLMLoop, one problem: losses" % system, rb["loss_trace"][0], "evaluations", rb["evaluations"], "state", rb["state"], "theta error %.2e" % _err(rb["theta"][0], c))
    assert rb["evaluations"][0] <= budget and rb["loss"][0] <= 1e-10
    per = ow.TRUST_COUNTS_PER_DEMO[system]
    rk = BatchedLMLoop.for_irl(mdl, c["demo_x"], c["demo_u"], c["theta0"], samples_per_problem=1, max_evals=2 * max(per), loss_tol=1e-16, **kw).run()
    print("%s BatchedLMLoop, one problem per demonstration: final losses" % system, rk["loss"], "evaluations", rk["evaluations"], "state", rk["state"])
    assert all(rk["evaluations"][k] <= 2 * per[k] for k in range(B)) and (rk["loss"] <= 1e-10).all()


@pytest.mark.parametrize("system", ["pendulum", "cartpole"])
def test_lm_loops_with_huber_end_ten_times_closer_than_plain_least_squares(system):
    """delta = oc_wls_common.HUBER_DELTA, unit weights: at most twice the oracle's evaluations, |theta - theta*| at least the factor 10 that the host test pins below
    the plain run's (same loop, same budget rule) - LMLoop, and BatchedLMLoop with all demonstrations as one problem"""
    import oc_wls_common as ow
    from pdp_amd import zoo
    from pdp_amd.irl import BatchedLMLoop, LMLoop
    c, mdl = ow.corrupted(system), zoo.get(system, "irl")
    B = c["demo_x"].shape[0]
    bp, bh = 2 * ow.PLAIN_COUNTS[system], 2 * ow.HUBER_COUNTS[system]
    plain = LMLoop.for_irl(mdl, c["demo_x"], c["demo_u"], c["theta0"]).run(max_evals=bp)
    robust = LMLoop.for_irl(mdl, c["demo_x"], c["demo_u"], c["theta0"], huber_delta=ow.HUBER_DELTA).run(max_evals=bh)
    e0, e1 = _err(plain["parameter_trace"][-1], c), _err(robust["parameter_trace"][-1], c)
    print("%s LMLoop: plain %.3e (%d evaluations, %d rejected, stalled %s)  Huber %.3e (%d, %d, %s)" % (system, e0, plain["evaluations"], plain["rejected"], plain["stalled"],
                                                                                                  e1, robust["evaluations"], robust["rejected"], robust["stalled"]))
    print("  Huber losses", robust["loss_trace"])
    assert plain["evaluations"] <= bp and robust["evaluations"] <= bh
    assert e1 * 10 <= e0
    rb = BatchedLMLoop.for_irl(mdl, c["demo_x"], c["demo_u"], c["theta0"], samples_per_problem=B, max_evals=bh, huber_delta=ow.HUBER_DELTA).run()
    eb = _err(rb["theta"][0], c)
    print("%s BatchedLMLoop, one problem, Huber: %.3e (%d evaluations, state %s)" % (system, eb, rb["evaluations"][0], rb["state"][0]))
    assert rb["evaluations"][0] <= bh and eb * 10 <= e0


def test_example_method_lm_with_huber_on_corrupted_cartpole_demonstrations():
    """examples/irl_pdp.py --system cartpole --method lm --huber 0.01 --outliers 0.05: runs, prints its accepted points and its summary; the loss falls (its minimum is
    not zero: the outliers stay in the data)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "irl_pdp.py"), "--system", "cartpole", "--method", "lm", "--huber", "0.01", "--outliers", "0.05"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    print(r.stdout[-1500:])
    done = [ln for ln in r.stdout.splitlines() if ln.startswith("done:")]
    accepted = [float(ln.split("loss")[1].split()[0]) for ln in r.stdout.splitlines() if ln.startswith("accepted")]
    assert len(done) == 1 and len(accepted) >= 2 and (np.diff(accepted) <= 0).all() and accepted[-1] < 0.5 * accepted[0], r.stdout[-3000:]      # (seven printed digits)
    assert any("outliers" in ln for ln in r.stdout.splitlines())


# ---- the wiring of the Python evaluation: the entry points with hand-built arguments, to the bit ---------------------------------------------------------------------
@pytest.mark.parametrize("per_sample", [False, True], ids=["shared_theta", "per_sample_theta"])
@pytest.mark.parametrize("mode", ["gn", "gn_flag", "weights_both"])
def test_python_evaluation_launches_the_entry_point_with_these_arguments(mode, per_sample):
    """Cart-pole, B = 5, T = 7, one oc_solve_ms; the rows of ModelLib.oc_rows_prepared's evaluation on the solutions - what oc_pdp_grad and the IRL loops run - are
    torch.equal to the rows of a direct ctypes call of the mode's entry point on the given (x, lam) with hand-built arguments: both launch the same deterministic
    kernel.  The loss the kernel writes beside the row is the row's own."""
    import torch
    import oc_vjp_common as c
    from pdp_amd import runtime as rt, zoo
    mdl = zoo.get("cartpole", "irl")
    inp = c.make_inputs("cartpole", 5, 7)
    B, T, n, m, p = 5, 7, mdl.n, mdl.m, mdl.p
    theta = inp["theta_b"] if per_sample else inp["theta"]
    s = mdl.oc_solve_ms(inp["x0"], theta, T)
    assert bool(s["converged"].all())
    x, u, lam = s["state"], s["control"], s["costate"]
    demo_x, demo_u = inp["demo_x"].copy(), inp["demo_u"].copy()
    skip = mode == "gn_flag"
    if skip:
        demo_x[:, 1::3, 1] = np.nan
        demo_u[:, 2::3] = np.nan
    wx = wu = None
    if mode == "weights_both":
        wx = np.broadcast_to(1.0 / (0.5 + np.arange(n)) ** 2, (B, T + 1, n)).copy()
        wx[:, 1::4, 2] = 0.0
        wu = np.full((T, m), 0.25)
        wu[3] = 0.0
    rows = mdl.oc_rows_prepared(demo_x, demo_u, skip, wx, wu, 0.05 if wx is not None else None)[0]
    out = rows(u, theta, x=x, lam=lam)
    got = out["packed_gn"].clone()
    assert tuple(got.shape) == (B, p + 1 + p * p) and not bool(out["status"].any())
    th_d = rt.dev(theta).reshape(-1, p)
    tb, dx_d, du_d = (p if per_sample else 0), rt.dev(demo_x), rt.dev(demo_u)
    f64 = dict(dtype=torch.float64, device="cuda")
    packed, loss, status = torch.full((B, p + 1 + p * p), 7.0, **f64), torch.full((B,), 7.0, **f64), torch.zeros((B,), dtype=torch.int32, device="cuda")
    nbytes = int(mdl.lib.pdp_oc_pdp_workspace_bytes(B, T))
    ws = torch.empty((max(nbytes, 8) // 8,), **f64)
    P, st, flags = rt.ptr, rt.current_stream_ptr(), 1 | (32 if skip else 0)
    if wx is not None:
        wx_d, wu_d = rt.dev(wx), rt.dev(wu)
        rc = mdl.lib.pdp_oc_pdp_grad_wls_batched(B, T, flags, None, P(u), P(th_d), tb, P(dx_d), P(du_d), P(wx_d), (T + 1) * n, P(wu_d), 0, 0.05, P(x), P(lam), P(loss),
                                                 P(packed), P(status), P(ws), nbytes, st)
    else:
        rc = mdl.lib.pdp_oc_pdp_grad_batched(B, T, flags | 16, None, P(u), P(th_d), tb, P(dx_d), P(du_d), P(x), P(lam), P(loss), P(packed), None, None, P(status), P(ws),
                                             nbytes, st)
    assert rc == 0
    assert torch.isfinite(packed).all() and float(packed.abs().max()) > 0 and torch.equal(got, packed)
    assert torch.equal(loss, packed[:, p]) and torch.equal(out["loss"], packed[:, p])
