"""GPU: PDP_GRAD_SKIP_MISSING - demonstrations with gaps: a NaN in demo_x / demo_u is an entry that was not observed and is left out of the fused unit's loss, gradient and
Gauss-Newton matrix (include/pdp_hip.h; ModelLib.oc_pdp_grad(skip_missing=True), OCSys.pdp_grad_batch(skip_missing=True), LMLoop.for_irl(ini_state=, skip_missing=True),
examples/irl_pdp.py --method lm --every / --observe / --no-controls).

Shapes (tests/oc_vjp_common.make_inputs; those of tests/test_gpu_oc_gn.py): the smallest at which each kernel path can go wrong.  Runner / evaluator kernel (n > 4): quadrotor
at T = 41 - two backward chunks of unequal length - and T = 7, rocket at T = 31; B = 5 at 1, 2 and 4 trajectories per workgroup (PDP_FUSED_TPW, read once per process: one
child process each).  One-wave kernel (n <= 4): cart-pole at T = 70 = 64 + 6 and T = 7, pendulum (n = 2); B = 3.  Masks (tests/oc_missing_common.make_masks): fixed seed,
about half of all entries NaN, NaN for certain at all of demo_x[:, 0], one whole state row and one whole control row in mid-horizon, both sides of the middle chunk boundary,
demo_u at t = 0 and T - 1, half the components of demo_x[:, T]; the last sample has every entry NaN, the one before it none.

Reference: the default unit's own want_sens=True outputs on the same inputs with the NaNs replaced by zeros, contracted with the masks in torch fp64 exactly as the header's
three formulas state.  Tolerance: 1e-10 of the largest entry of the compared array, per sample - BASELINE.md section 3's GPU-vs-restatement tolerance on identical inputs.  The
CPU oracle is compared where tests/test_gpu_oc_vjp.py documents that its own rounding error is below that: quadrotor T = 41, rocket T = 31, cart-pole and pendulum T = 7.
The Levenberg-Marquardt budgets are twice the evaluations the same schedule needs on the CPU oracle on the same sparse data; traces are printed, not asserted."""
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

# (system, B, T, per-sample theta, given trajectory)
F3_CASES = [("quadrotor", 5, 41, False, False), ("quadrotor", 5, 41, True, True), ("quadrotor", 5, 7, True, False), ("rocket", 5, 31, False, True), ("rocket", 5, 31, True, False)]
F1_CASES = [("cartpole", 3, 70, False, False), ("cartpole", 3, 70, True, True), ("cartpole", 3, 7, True, False), ("pendulum", 3, 70, False, True), ("pendulum", 3, 7, True, False)]

WORKER = r'''
import os, sys
import numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(here)r)
import oc_vjp_common as c, oc_missing_common as ms
from pdp_amd import zoo
out = {}
for k, (system, B, T, per_sample, given) in enumerate(%(cases)r):
    r = ms.evaluate(zoo.get(system, "irl"), c.make_inputs(system, B, T), per_sample, given)
    for key, v in r.items():
        out["%%d_%%s" %% (k, key)] = v
np.savez(sys.argv[1], **out)
'''


def npy(t):
    return t.detach().cpu().numpy()


def _tag(case):
    system, B, T, per_sample, given = case
    return "%s B=%d T=%d %s theta, %s" % (system, B, T, "per-sample" if per_sample else "shared", "given trajectory" if given else "rollout")


def _split(rows, B, p):
    return rows[:B, :p], rows[:B, p], rows[:B, p + 1:].reshape(B, p, p)


def _judge(margins, tag, r):
    """checks 1 - 4 of one shape"""
    import oc_missing_common as ms
    p = r["grad_ref"].shape[1]
    B = r["rows"].shape[0] - 1
    dark, full = ms.all_nan_sample(B), ms.nan_free_sample(B)
    seen = [i for i in range(B) if i != dark]
    grad, loss, G = _split(r["rows"], B, p)
    # 1. with PDP_GRAD_GAUSS_NEWTON.  The rows were NaN before the call: every entry was written and is finite, and nothing behind the last row
    assert np.isfinite(r["rows"][:B]).all(), tag
    assert np.isnan(r["rows"][B]).all(), tag
    assert all(np.abs(r["G_ref"][i]).max() > 0 and np.abs(r["grad_ref"][i]).max() > 0 and r["loss_ref"][i] > 0 for i in seen), tag
    margins.check("OC missing %s: gradient vs the masked contraction of the default unit's own sensitivities (per sample, relative to the largest entry)" % tag,
                  max(ms.rel(grad[i], r["grad_ref"][i]) for i in seen), TOL)
    margins.check("OC missing %s: loss vs the masked sum of squares" % tag, max(ms.rel(loss[i], r["loss_ref"][i]) for i in seen), TOL)
    margins.check("OC missing %s: G vs einsum of the row-masked sensitivities" % tag, max(ms.rel(G[i], r["G_ref"][i]) for i in seen), TOL)
    assert np.array_equal(G, np.swapaxes(G, 1, 2)), tag                                    # both operands carry the mask: symmetric to the bit
    for i in seen:
        ev = np.linalg.eigvalsh(G[i])
        assert ev[0] >= -1e-12 * ev[-1], (tag, i, ev)
    assert not r["status"].any() and not r["status0"].any(), tag                           # a missing entry sets no status bit
    assert np.array_equal(r["x"], r["x_def"]) and np.array_equal(r["lam"], r["lam_def"]), tag
    assert np.array_equal(loss, r["loss"]), tag                                            # loss [B] is the row's loss column
    # 2. the flag alone and with PDP_OC_PACKED
    assert np.isfinite(r["plain_grad"][:B]).all() and np.isnan(r["plain_grad"][B]).all() and np.isfinite(r["packed"][:B]).all() and np.isnan(r["packed"][B]).all(), tag
    for name, g_, l_ in (("alone", r["plain_grad"][:B], r["plain_loss"]), ("packed", r["packed"][:B, :p], r["packed"][:B, p])):
        margins.check("OC missing %s, the flag %s: gradient" % (tag, name), max(ms.rel(g_[i], r["grad_ref"][i]) for i in seen), TOL)
        margins.check("OC missing %s, the flag %s: loss" % (tag, name), max(ms.rel(l_[i], r["loss_ref"][i]) for i in seen), TOL)
    assert np.array_equal(r["packed"][:B, p], r["packed_loss"]), tag
    for k in ("plain", "packed"):
        assert not r[k + "_status"].any() and np.array_equal(r[k + "_x"], r["x_def"]) and np.array_equal(r[k + "_lam"], r["lam_def"]), (tag, k)
    # 3. nothing observed: exact zeros
    assert not r["rows"][dark].any() and r["loss"][dark] == 0.0 and not r["plain_grad"][dark].any() and r["plain_loss"][dark] == 0.0 and not r["packed"][dark].any(), tag
    assert r["loss_ref"][dark] == 0.0 and not r["G_ref"][dark].any()
    # 4. nothing missing: the same call without the flag (another instantiation, compiled with its own contraction: within the tolerance, bit-equality only reported)
    ng, nl, nG = _split(r["noflag_rows"], B, p)
    margins.check("OC missing %s, NaN-free sample: gradient vs the call without the flag" % tag, ms.rel(grad[full], ng[full]), TOL)
    margins.check("OC missing %s, NaN-free sample: loss vs the call without the flag" % tag, ms.rel(loss[full], nl[full]), TOL)
    margins.check("OC missing %s, NaN-free sample: G vs the call without the flag" % tag, ms.rel(G[full], nG[full]), TOL)
    margins.check("OC missing %s, NaN-free sample, the flag alone: gradient vs the call without the flag" % tag, ms.rel(r["plain_grad"][full], r["noflag_grad"][full]), TOL)
    margins.check("OC missing %s, NaN-free sample, the flag alone: loss vs the call without the flag" % tag, ms.rel(r["plain_loss"][full], r["noflag_loss"][full]), TOL)
    print("OC missing %s, NaN-free sample bit-equal to the call without the flag: row %s, plain gradient %s, plain loss %s" % (
        tag, np.array_equal(r["rows"][full], r["noflag_rows"][full]), np.array_equal(r["plain_grad"][full], r["noflag_grad"][full]), r["plain_loss"][full] == r["noflag_loss"][full]))


def _oracle_oc(name, _cache={}):
    from oracle import models, pdp_oracle as po
    if name not in _cache:
        st = models.IRL_SETUP[name]
        _cache[name] = po.make_oc(models.REGISTRY[name](**st["kwargs"]), st["dt"])
    return _cache[name]


def _judge_oracle(margins, tag, inp, r, per_sample):
    """5. against the CPU oracle: the restatement of the reference's unit on the same inputs, its trajectory and sensitivities masked and contracted (a masked sample and the
    NaN-free one)"""
    import oc_missing_common as ms
    from oracle import pdp_oracle as po
    oc = _oracle_oc(inp["system"])
    mi = ms.mask_inputs(inp)
    B, p = inp["B"], r["grad_ref"].shape[1]
    grad, loss, G = _split(r["rows"], B, p)
    for i in (0, ms.nan_free_sample(B)):
        th = inp["theta_b"][i] if per_sample else inp["theta"]
        unit = po.pdp_oc_unit(oc, inp["x0"][i], inp["u"][i], th, mi["demo_x0"][i], mi["demo_u0"][i])
        X, U = np.stack(unit["lqr"]["state_traj_opt"]), np.stack(unit["lqr"]["control_traj_opt"])
        wx, wu = mi["wx"][i], mi["wu"][i]
        ex, eu = np.where(wx, np.asarray(unit["state_traj"]) - mi["demo_x0"][i], 0.0), np.where(wu, inp["u"][i] - mi["demo_u0"][i], 0.0)
        Xm, Um = np.where(wx[:, :, None], X, 0.0), np.where(wu[:, :, None], U, 0.0)
        lo, go = (ex ** 2).sum() + (eu ** 2).sum(), np.einsum("ti,tip->p", ex, Xm) + np.einsum("ti,tip->p", eu, Um)
        Go = np.einsum("tip,tiq->pq", Xm, Xm) + np.einsum("tip,tiq->pq", Um, Um)
        margins.check("OC missing %s sample %d: loss vs oracle.pdp_oc_unit, masked" % (tag, i), ms.rel(loss[i], lo), TOL)
        margins.check("OC missing %s sample %d: gradient vs oracle.pdp_oc_unit, masked and contracted" % (tag, i), ms.rel(grad[i], go), TOL)
        margins.check("OC missing %s sample %d: G vs oracle.pdp_oc_unit sensitivities, row-masked and contracted with themselves" % (tag, i), ms.rel(G[i], Go), TOL)


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
    # one wave pair per trajectory whatever the workgroup: the three layouts agree to the bit (NaN guard rows included)
    for k in range(len(F3_CASES)):
        for key in ("rows", "plain_grad", "plain_loss", "packed"):
            assert np.array_equal(results[1, k][key], results[2, k][key], equal_nan=True) and np.array_equal(results[1, k][key], results[4, k][key], equal_nan=True), \
                (_tag(F3_CASES[k]), key)
    for k in (0, 4):                            # quadrotor T = 41 shared theta, rocket T = 31 per-sample theta
        system, B, T, per_sample, given = F3_CASES[k]
        _judge_oracle(margins, "fused3 TPW=4 " + _tag(F3_CASES[k]), c.make_inputs(system, B, T), results[4, k], per_sample)


@pytest.mark.parametrize("case", F1_CASES, ids=[_tag(cs).replace(" ", "_") for cs in F1_CASES])
def test_one_wave_kernel(margins, case):
    import oc_vjp_common as c
    import oc_missing_common as ms
    from pdp_amd import zoo
    system, B, T, per_sample, given = case
    inp = c.make_inputs(system, B, T)
    r = ms.evaluate(zoo.get(system, "irl"), inp, per_sample, given)
    _judge(margins, "one-wave " + _tag(case), r)
    if T == 7:
        _judge_oracle(margins, "one-wave " + _tag(case), inp, r, per_sample)


def test_one_wave_kernel_beyond_four_states(margins, tmp_path):
    """the one-wave kernel's n > 4 branch in the two PDP_GRAD_SKIP_MISSING modes (the references: the default and the record-writing one) (oc_vjp_common.run_one_wave_beyond_four_states)"""
    import oc_vjp_common as c
    c.run_one_wave_beyond_four_states(margins, tmp_path, WORKER, F3_CASES, _judge, _judge_oracle, _tag)


def test_argument_errors():
    """6. PDP_GRAD_SKIP_MISSING with PDP_OC_COTANGENT or with any sensitivity output is PDP_E_ARG and launches nothing; alone and with PDP_GRAD_GAUSS_NEWTON it runs"""
    import ctypes as C
    import oc_vjp_common as c
    import oc_missing_common as ms
    import torch
    from pdp_amd import runtime as rt, zoo
    for system in ("cartpole", "quadrotor"):
        mdl = zoo.get(system, "irl")
        n, m, p = mdl.n, mdl.m, mdl.p
        B, T = 3, 7
        inp = ms.mask_inputs(c.make_inputs(system, B, T))
        f64 = dict(dtype=torch.float64, device="cuda")
        x0, u, th, dx, du = (rt.dev(inp[k]) for k in ("x0", "u", "theta", "demo_xm", "demo_um"))
        x, lam, loss, row = torch.empty((B, T + 1, n), **f64), torch.empty((B, T, n), **f64), torch.empty((B,), **f64), torch.zeros((B, p + 1 + p * p), **f64)
        dxdp, dudp = torch.empty((B, T + 1, n, p), **f64), torch.empty((B, T, m, p), **f64)
        ric = torch.empty((B, T, int(mdl.lib.pdp_oc_riccati_doubles())), **f64)
        prec = torch.empty((B, T, int(mdl.lib.pdp_oc_predict_record_floats())), dtype=torch.float32, device="cuda")
        status = torch.zeros((B,), dtype=torch.int32, device="cuda")
        nbytes = mdl.lib.pdp_oc_pdp_workspace_bytes(B, T)
        ws = torch.empty((max(nbytes, 8) // 8,), **f64)
        P = rt.ptr

        def plain(flags, dx_=None, du_=None):
            return mdl.lib.pdp_oc_pdp_grad_batched(B, T, flags, P(x0), P(u), P(th), 0, P(dx), P(du), P(x), P(lam), P(loss), P(row), P(dx_), P(du_), P(status), P(ws), nbytes,
                                                   rt.current_stream_ptr())

        def sens(flags, **kw):
            so = rt.PdpOcSensOut(*[kw[k].data_ptr() if k in kw else None for k in ("dxdp", "dudp", "riccati", "predict_record")])
            return mdl.lib.pdp_oc_pdp_grad_sens_batched(B, T, flags, P(x0), P(u), P(th), 0, P(dx), P(du), P(x), P(lam), P(loss), P(row), C.byref(so), P(status), P(ws),
                                                        nbytes, rt.current_stream_ptr())
        assert plain(32 | 8) == -1 and plain(32 | 8 | 16) == -1 and sens(32 | 8) == -1
        assert plain(32, dx_=dxdp) == -1 and plain(32, du_=dudp) == -1 and plain(32 | 16, dx_=dxdp, du_=dudp) == -1
        assert sens(32, dxdp=dxdp) == -1 and sens(32, dudp=dudp) == -1 and sens(32, riccati=ric) == -1 and sens(32, predict_record=prec) == -1
        assert sens(32 | 16, riccati=ric) == -1 and plain(32 | 16 | 2) == -1
        torch.cuda.synchronize()
        assert not bool(row.any())                                  # nothing was launched
        assert plain(32) == 0
        torch.cuda.synchronize()
        g1 = row.reshape(-1)[:B * p].clone()
        assert bool(torch.isfinite(g1).all()) and bool(g1.abs().sum() > 0) and int(status.sum()) == 0
        row.zero_()
        assert plain(32 | 16) == 0
        r1 = row.clone()
        assert sens(32 | 16) == 0
        torch.cuda.synchronize()
        assert torch.equal(row, r1) and bool(torch.isfinite(r1).all()) and bool(r1.abs().sum() > 0) and int(status.sum()) == 0
        g2 = r1[:, :p]                                              # the same gradient in both layouts (two instantiations, each with its own contraction: not to the bit)
        assert float(((g2 - g1.reshape(B, p)).abs().amax(dim=1) / g2.abs().amax(dim=1).clamp_min(1e-300)).max()) <= TOL


def _wide_auxvar_oc():
    """m + p > 16 (m = 2, p = 16): the model of tests/test_gpu_oc_vjp.py::_wide_auxvar_oc, which the fused kernels refuse (PDP_E_SIZE)"""
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


def test_beyond_the_fused_limits_the_materialised_route_fills_the_same_rows(margins):
    """7. PDP_E_SIZE from the entry point: the kernel-by-kernel route, the sensitivities through HBM, masked and contracted with torch.einsum into the same rows"""
    import oc_missing_common as ms
    import torch
    from pdp_amd import runtime as rt
    oc, th, rng = _wide_auxvar_oc()
    n, m, p, T, B = 6, 2, 16, 9, 2
    x0, u = 0.5 * rng.standard_normal((B, n)), 0.3 * rng.standard_normal((B, T, m))
    demo_x, demo_u = 0.1 * rng.standard_normal((B, T + 1, n)), 0.1 * rng.standard_normal((B, T, m))
    wx, wu = ms.make_masks(4, T, n, m)                              # (samples 0 and 1 of four: both masked)
    wx, wu = wx[:B], wu[:B]
    dxm, dum, dx0, du0 = np.where(wx, demo_x, np.nan), np.where(wu, demo_u, np.nan), np.where(wx, demo_x, 0.0), np.where(wu, demo_u, 0.0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        ref = oc.pdp_grad_batch(u, th, dx0, du0, ini_state=x0, want_sens=True)
        out = oc.pdp_grad_batch(u, th, dxm, dum, ini_state=x0, want_gauss_newton=True, skip_missing=True)
        pl = oc.pdp_grad_batch(u, th, dxm, dum, ini_state=x0, skip_missing=True)
    loss_ref, grad_ref, G_ref = (npy(t) for t in ms.contract(ref["x"], rt.dev(u), rt.dev(dx0), rt.dev(du0), torch.as_tensor(wx, device="cuda"), torch.as_tensor(wu, device="cuda"), ref["dxdp"], ref["dudp"]))
    row = out["packed_gn"]
    assert row.shape == (B, p + 1 + p * p) and out["gn"].shape == (B, p, p) and int(out["status"].sum()) == 0 and bool(torch.isfinite(row).all())
    assert torch.equal(row[:, :p], out["grad"]) and torch.equal(row[:, p], out["loss"]) and torch.equal(row[:, p + 1:].reshape(B, p, p), out["gn"])
    margins.check("OC missing beyond the fused limits (n=6 m=2 p=16): G vs the masked contraction", max(ms.rel(npy(out["gn"])[i], G_ref[i]) for i in range(B)), TOL)
    margins.check("OC missing beyond the fused limits: gradient", max(ms.rel(npy(out["grad"])[i], grad_ref[i]) for i in range(B)), TOL)
    margins.check("OC missing beyond the fused limits: loss", max(ms.rel(npy(out["loss"])[i], loss_ref[i]) for i in range(B)), TOL)
    margins.check("OC missing beyond the fused limits, the flag alone: gradient", max(ms.rel(npy(pl["grad"])[i], grad_ref[i]) for i in range(B)), TOL)
    margins.check("OC missing beyond the fused limits, the flag alone: loss", max(ms.rel(npy(pl["loss"])[i], loss_ref[i]) for i in range(B)), TOL)
    assert torch.equal(out["x"], ref["x"]) and torch.equal(out["lam"], ref["lam"]) and int(pl["status"].sum()) == 0


# ---- Levenberg-Marquardt on sparse demonstrations: the stored demonstrations, the reference's own initial parameter, every entry not named NaN (all controls included)
def _sparse(system, steps, comps):
    d = np.load(os.path.join(ROOT, "tests", "golden", "demos_%s.npz" % system))
    theta0 = np.load(os.path.join(ROOT, "tests", "golden", "irltrace_head_%s.npz" % system))["param"][0]
    demo_x, demo_u = np.full(d["state"].shape, np.nan), np.full(d["control"].shape, np.nan)
    for t in steps:
        demo_x[:, t, comps] = d["state"][:, t, comps]
    return d, theta0, demo_x, demo_u


def _run_lm(system, steps, comps, shape, budget):
    from pdp_amd import zoo
    from pdp_amd.irl import LMLoop
    d, theta0, demo_x, demo_u = _sparse(system, steps, comps)
    assert d["state"].shape == shape and np.isnan(demo_u).all() and np.isnan(demo_x[:, 0]).all()
    r = LMLoop.for_irl(zoo.get(system, "irl"), demo_x, demo_u, theta0, ini_state=d["state"][:, 0], skip_missing=True).run(max_evals=budget, loss_tol=1e-16)
    print("%s LM on %d observed entries per demonstration: losses" % (system, int((~np.isnan(demo_x[0])).sum())), r["loss_trace"], "evaluations", r["evaluations"],
          "rejected", r["rejected"], "stalled", r["stalled"])
    assert r["evaluations"] <= budget
    assert r["loss_trace"][-1] <= 1e-10
    assert (np.diff(r["loss_trace"]) < 0).all()


def test_lm_sparse_one_wave_kernel_pendulum():
    """state component 0 at t = 2, 4, ..., 20 of 5 x T = 20; the CPU restatement of the schedule needs 6 evaluations (1.9e-22), none rejected"""
    _run_lm("pendulum", range(2, 21, 2), [0], (5, 21, 2), 12)


def test_lm_sparse_one_wave_kernel_cartpole():
    """components 0, 1 at t = 10, 20, 30 of 5 x T = 30 (the data of examples/oc_layer_custom_loss.py); the restatement needs 5 evaluations (9.7e-19), none rejected"""
    _run_lm("cartpole", (10, 20, 30), [0, 1], (5, 31, 4), 10)


def test_lm_sparse_runner_evaluator_kernel_rocket():
    """position and quaternion (components 0, 1, 2, 6, 7, 8, 9) at t = 4, 8, ..., 40 of 1 x T = 40; the restatement needs 7 evaluations (6.2e-22), none rejected"""
    _run_lm("rocket", range(4, 41, 4), [0, 1, 2, 6, 7, 8, 9], (1, 41, 13), 14)


def test_example_method_lm_on_sparse_cartpole_demonstrations():
    """examples/irl_pdp.py --system cartpole --method lm --every 10 --observe 0,1 --no-controls"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "irl_pdp.py"), "--system", "cartpole", "--method", "lm", "--every", "10", "--observe", "0,1",
                        "--no-controls"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    done = [ln for ln in r.stdout.splitlines() if ln.startswith("done:")]
    assert len(done) == 1, r.stdout[-3000:]
    final = float(done[0].split("final loss")[1].split()[0])
    assert final <= 1e-10, r.stdout[-3000:]
    assert len([ln for ln in r.stdout.splitlines() if ln.startswith("accepted")]) >= 2
