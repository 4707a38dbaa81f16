"""GPU: the fused OC unit's Gauss-Newton mode (PDP_GRAD_GAUSS_NEWTON: the packed row gradient | loss | G = J'J per trajectory), its runtime / class surface
(ModelLib.oc_pdp_grad(gauss_newton=True), OCSys.pdp_grad_batch(want_gauss_newton=True)) and the Levenberg-Marquardt loop on top (pdp_amd.irl.LMLoop, examples/irl_pdp.py
--method lm).

Shapes (tests/oc_vjp_common.make_inputs): the smallest at which each kernel path can go wrong.  Runner / evaluator kernel (n > 4): quadrotor at T = 41 - two backward chunks of
unequal length - and T = 7, rocket at T = 31; B = 5 at 1, 2 and 4 trajectories per workgroup (PDP_FUSED_TPW, read once per process: one child process each), the last workgroup
ragged for 2 and 4.  One-wave kernel (n <= 4): cart-pole at T = 70 = 64 + 6 and T = 7, pendulum (n = 2); B = 3.  The CPU oracle is compared where tests/test_gpu_oc_vjp.py
documents that its own rounding error is below the tolerance: quadrotor T = 41, rocket T = 31, cart-pole and pendulum T = 7.

Tolerance: 1e-10 relative to the largest entry of the compared array, per sample - BASELINE.md section 3's GPU-vs-restatement tolerance on identical inputs.  The loop's
bounds are those of the same schedule run on the CPU oracle: twice its evaluations, loss <= 1e-10 where it reaches 1e-19 .. 1e-21.  The traces are printed, not asserted."""
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
import oc_vjp_common as c, oc_gn_common as gn
from pdp_amd import zoo
out = {}
for k, (system, B, T, per_sample, given) in enumerate(%(cases)r):
    r = gn.evaluate(zoo.get(system, "irl"), c.make_inputs(system, B, T), per_sample, given)
    for key, v in r.items():
        out["%%d_%%s" %% (k, key)] = v
np.savez(sys.argv[1], **out)
'''


def npy(t):
    return t.detach().cpu().numpy()


def _split(r):
    B = r["rows"].shape[0] - 1
    p = r["grad_def"].shape[1]
    rows = r["rows"][:B]
    return rows[:, :p], rows[:, p], rows[:, p + 1:].reshape(B, p, p)


def _judge(margins, tag, r):
    import oc_gn_common as gn
    B = r["rows"].shape[0] - 1
    grad, loss, G = _split(r)
    # the rows were NaN before the call: every entry was written, and nothing behind the last row
    assert np.isfinite(r["rows"][:B]).all(), tag
    assert np.isnan(r["rows"][B]).all(), tag
    assert np.abs(r["G_ref"]).max() > 0
    margins.check("OC GN %s: G vs einsum(dxdp, dxdp) + einsum(dudp, dudp) of the default unit's own sensitivities (per sample, relative to the largest entry)" % tag,
                  gn.rel_per_sample(G, r["G_ref"]), TOL)
    assert np.array_equal(r["status"], r["status0"]) and not r["status"].any(), tag
    assert np.array_equal(r["x"], r["x_def"]) and np.array_equal(r["lam"], r["lam_def"]), tag
    margins.check("OC GN %s: gradient columns vs the default unit's gradient (0 expected)" % tag, gn.rel_per_sample(grad, r["grad_def"]), TOL)
    margins.check("OC GN %s: loss column vs the default unit's loss (0 expected)" % tag, float(np.abs(loss - r["loss_def"]).max() / np.abs(r["loss_def"]).max()), TOL)
    assert np.array_equal(loss, r["loss"]), tag                   # loss [B] is written as before
    assert np.array_equal(G, np.swapaxes(G, 1, 2)), tag            # the same products in the same order: symmetric to the bit
    for i in range(B):
        ev = np.linalg.eigvalsh(G[i])
        assert ev[0] >= -1e-12 * ev[-1], (tag, i, ev)


def _oracle_oc(name, _cache={}):
    from oracle import models, pdp_oracle as po
    if name not in _cache:
        st = models.IRL_SETUP[name]
        _cache[name] = po.make_oc(models.REGISTRY[name](**st["kwargs"]), st["dt"])
    return _cache[name]


def _judge_oracle(margins, tag, inp, r, per_sample, samples=(0, 1)):
    """3. against the CPU oracle: the restatement of the reference's unit on the same inputs, its sensitivities contracted with themselves"""
    from oracle import pdp_oracle as po
    oc = _oracle_oc(inp["system"])
    G = _split(r)[2]
    for i in samples:
        th = inp["theta_b"][i] if per_sample else inp["theta"]
        unit = po.pdp_oc_unit(oc, inp["x0"][i], inp["u"][i], th, inp["demo_x"][i], inp["demo_u"][i])
        X, U = np.stack(unit["lqr"]["state_traj_opt"]), np.stack(unit["lqr"]["control_traj_opt"])
        Go = np.einsum("tip,tiq->pq", X, X) + np.einsum("tip,tiq->pq", U, U)
        margins.check("OC GN %s sample %d: G vs oracle.pdp_oc_unit sensitivities contracted with themselves" % (tag, i), np.abs(G[i] - Go).max() / np.abs(Go).max(), TOL)


def _tag(case):
    system, B, T, per_sample, given = case
    return "%s B=%d T=%d %s theta, %s" % (system, B, T, "per-sample" if per_sample else "shared", "given trajectory" if given else "rollout")


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
    # one wave pair per trajectory whatever the workgroup: the three layouts agree to the bit (NaN guard row included)
    for k in range(len(F3_CASES)):
        assert np.array_equal(results[1, k]["rows"], results[2, k]["rows"], equal_nan=True) and np.array_equal(results[1, k]["rows"], results[4, k]["rows"], equal_nan=True), \
            _tag(F3_CASES[k])
    for k in (0, 4):                            # quadrotor T = 41 shared theta, rocket T = 31 per-sample theta
        system, B, T, per_sample, given = F3_CASES[k]
        _judge_oracle(margins, "fused3 TPW=4 " + _tag(F3_CASES[k]), c.make_inputs(system, B, T), results[4, k], per_sample)


@pytest.mark.parametrize("case", F1_CASES, ids=[_tag(cs).replace(" ", "_") for cs in F1_CASES])
def test_one_wave_kernel(margins, case):
    import oc_vjp_common as c
    import oc_gn_common as gn
    from pdp_amd import zoo
    system, B, T, per_sample, given = case
    inp = c.make_inputs(system, B, T)
    r = gn.evaluate(zoo.get(system, "irl"), inp, per_sample, given)
    _judge(margins, "one-wave " + _tag(case), r)
    if T == 7:
        _judge_oracle(margins, "one-wave " + _tag(case), inp, r, per_sample)


def test_one_wave_kernel_beyond_four_states(margins, tmp_path):
    """the one-wave kernel's n > 4 branch in the Gauss-Newton mode (oc_vjp_common.run_one_wave_beyond_four_states)"""
    import oc_vjp_common as c
    c.run_one_wave_beyond_four_states(margins, tmp_path, WORKER, F3_CASES, _judge, _judge_oracle, _tag)


def test_argument_errors():
    """4. PDP_GRAD_GAUSS_NEWTON with PDP_OC_COTANGENT, with PDP_OC_PACKED or with any sensitivity output is PDP_E_ARG; the flag alone runs"""
    import ctypes as C
    import oc_vjp_common as c
    import torch
    from pdp_amd import runtime as rt, zoo
    for system in ("cartpole", "quadrotor"):
        mdl = zoo.get(system, "irl")
        n, m, p = mdl.n, mdl.m, mdl.p
        inp = c.make_inputs(system, 2, 7)
        B, T = 2, 7
        f64 = dict(dtype=torch.float64, device="cuda")
        x0, u, th, dx, du = (rt.dev(inp[k]) for k in ("x0", "u", "theta", "demo_x", "demo_u"))
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
        assert plain(16 | 8) == -1 and plain(16 | 2) == -1 and plain(16 | 8 | 2) == -1
        assert plain(16, dx_=dxdp) == -1 and plain(16, du_=dudp) == -1 and plain(16, dx_=dxdp, du_=dudp) == -1
        assert sens(16, dxdp=dxdp) == -1 and sens(16, dudp=dudp) == -1 and sens(16, riccati=ric) == -1 and sens(16, predict_record=prec) == -1
        torch.cuda.synchronize()
        assert not bool(row.any())                                  # nothing was launched
        assert plain(16) == 0
        r1 = row.clone()
        assert sens(16) == 0
        torch.cuda.synchronize()
        assert torch.equal(row, r1) and bool(r1.abs().sum() > 0) and int(status.sum()) == 0


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


def test_beyond_the_fused_limits_the_materialised_route_fills_the_same_row(margins):
    """5. PDP_E_SIZE from the entry point: the kernel-by-kernel route with the sensitivities through HBM, contracted by two einsums into the same row layout"""
    import oc_gn_common as gn
    import torch
    oc, th, rng = _wide_auxvar_oc()
    n, m, p, T, B = 6, 2, 16, 9, 2
    x0, u = 0.5 * rng.standard_normal((B, n)), 0.3 * rng.standard_normal((B, T, m))
    demo_x, demo_u = 0.1 * rng.standard_normal((B, T + 1, n)), 0.1 * rng.standard_normal((B, T, m))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        ref = oc.pdp_grad_batch(u, th, demo_x, demo_u, ini_state=x0, want_sens=True)
        out = oc.pdp_grad_batch(u, th, demo_x, demo_u, ini_state=x0, want_gauss_newton=True)
    G_ref = torch.einsum("btip,btiq->bpq", ref["dxdp"], ref["dxdp"]) + torch.einsum("btip,btiq->bpq", ref["dudp"], ref["dudp"])
    row = out["packed_gn"]
    assert row.shape == (B, p + 1 + p * p) and out["gn"].shape == (B, p, p) and int(out["status"].sum()) == 0
    assert torch.equal(row[:, :p], out["grad"]) and torch.equal(row[:, p], out["loss"]) and torch.equal(row[:, p + 1:].reshape(B, p, p), out["gn"])
    margins.check("OC GN beyond the fused limits (n=6 m=2 p=16): materialised route's G vs einsum(dxdp, dxdp) + einsum(dudp, dudp)", gn.rel_per_sample(npy(out["gn"]), npy(G_ref)), TOL)
    margins.check("OC GN beyond the fused limits: gradient vs the default call's", gn.rel_per_sample(npy(out["grad"]), npy(ref["grad"])), TOL)
    assert torch.equal(out["loss"], ref["loss"]) and torch.equal(out["x"], ref["x"]) and torch.equal(out["lam"], ref["lam"])


def _stored(system):
    d = np.load(os.path.join(ROOT, "tests", "golden", "demos_%s.npz" % system))
    theta0 = np.load(os.path.join(ROOT, "tests", "golden", "irltrace_head_%s.npz" % system))["param"][0]
    last = float(np.load(os.path.join(ROOT, "tests", "golden", "irltrace_%s.npz" % system))["loss_next"][-1])
    return d, theta0, last


def test_lm_loop_runner_evaluator_kernel_rocket():
    """6. the stored rocket demonstration (1 x T = 40) from the reference's own initial parameter: the CPU restatement of the schedule needs 7 evaluations (6.9e-21; two
    evaluations earlier 1.8e-4); twice as many are allowed here"""
    from pdp_amd import zoo
    from pdp_amd.irl import LMLoop
    d, theta0, last = _stored("rocket")
    assert d["state"].shape == (1, 41, 13)
    r = LMLoop.for_irl(zoo.get("rocket", "irl"), d["state"], d["control"], theta0).run(max_evals=14, loss_tol=1e-16)
    print("rocket LM: losses", r["loss_trace"], "evaluations", r["evaluations"], "rejected", r["rejected"], "stalled", r["stalled"], "stored trace's last loss", last)
    assert r["evaluations"] <= 14
    assert r["loss_trace"][-1] <= 1e-10
    assert r["loss_trace"][-1] < 1e-6 * last


def test_lm_loop_one_wave_kernel_pendulum():
    """7. the stored pendulum demonstrations (5 x T = 20): the restatement needs 6 evaluations and is within 3e-6 of the true parameter after 5, exact after 6"""
    from pdp_amd import zoo
    from pdp_amd.irl import LMLoop
    d, theta0, last = _stored("pendulum")
    assert d["state"].shape == (5, 21, 2)
    r = LMLoop.for_irl(zoo.get("pendulum", "irl"), d["state"], d["control"], theta0).run(max_evals=12, loss_tol=1e-16)
    th = r["parameter_trace"][-1]
    rel = float((np.abs(th - d["true_parameter"]) / np.abs(d["true_parameter"])).max())          # per parameter
    assert (d["true_parameter"] != 0).all()
    print("pendulum LM: losses", r["loss_trace"], "evaluations", r["evaluations"], "rejected", r["rejected"], "stalled", r["stalled"], "theta error", rel)
    assert r["evaluations"] <= 12
    assert r["loss_trace"][-1] <= 1e-10
    assert rel <= 1e-5


def test_example_method_lm_on_the_cartpole():
    """8. examples/irl_pdp.py --system cartpole --method lm: exit 0, the printed final loss below the last loss of the reference's stored gradient-descent trace"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "irl_pdp.py"), "--system", "cartpole", "--method", "lm"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    done = [ln for ln in r.stdout.splitlines() if ln.startswith("done:")]
    assert len(done) == 1, r.stdout[-3000:]
    final = float(done[0].split("final loss")[1].split()[0])
    assert final < _stored("cartpole")[2], r.stdout[-3000:]
    assert len([ln for ln in r.stdout.splitlines() if ln.startswith("accepted")]) >= 2
