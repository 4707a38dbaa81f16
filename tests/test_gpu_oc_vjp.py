"""GPU: the fused OC unit as a vector-Jacobian product (PDP_OC_COTANGENT: caller-supplied loss cotangents in place of x - x_demo, u - u_demo), its runtime / class
surface (ModelLib.oc_pdp_vjp, OCSys.pdp_vjp_batch) and the torch.autograd layer on top (pdp_amd.autograd.oc_trajectory).

Shapes: the smallest at which each kernel path can go wrong.  Runner / evaluator kernel (n > 4): quadrotor (CHUNK 33) at T = 41 - two backward chunks of unequal length -
and T = 7 - inside one chunk -, rocket (CHUNK 28) at T = 31; B = 5 at 1, 2 and 4 trajectories per workgroup (PDP_FUSED_TPW, read once per process: one child process
each), the last workgroup ragged for 2 and 4.  One-wave kernel (n <= 4): cart-pole (CHUNK 64) at T = 70 = 64 + 6 and T = 7, pendulum (n = 2); B = 3.

The CPU oracle (oracle.pdp_oc_unit: the reference's formulas in their fp64 order, two explicit inverses of I + P R per stage) is compared where its OWN rounding error,
measured against the same formulas in 40-digit arithmetic (oracle.lqr_solver_mp) on these inputs, is below the tolerance: quadrotor T = 41 (1e-11), rocket T = 31 (1e-12),
cart-pole and pendulum T = 7 (1e-15, 1e-12).  Over 70 cart-pole steps the fp64 reference order itself is off by 7e-10 .. 3e-8 on these inputs (tests/test_gpu_models.py
says the same of the stored demonstrations); that horizon is held to the written-out sensitivities of the GPU unit only.

Tolerance: 1e-10 relative to the largest entry of the compared gradient, per sample - BASELINE.md section 3's GPU-vs-restatement tolerance on identical inputs; the
finite-difference bound of the layer test is the one tests/test_gpu_configs.py uses for the same quantity through the same solver (2e-4 of the largest difference)."""
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

# (system, B, T, per-sample theta, given trajectory, gx[:, 0] = 1e30)
F3_CASES = [("quadrotor", 5, 41, False, False, False), ("quadrotor", 5, 41, True, True, True), ("quadrotor", 5, 7, True, False, False),
            ("rocket", 5, 31, False, True, False), ("rocket", 5, 31, True, False, True)]
F1_CASES = [("cartpole", 3, 70, False, False, False), ("cartpole", 3, 70, True, True, True), ("cartpole", 3, 7, True, False, False),
            ("pendulum", 3, 70, False, True, False), ("pendulum", 3, 7, True, False, True)]

WORKER = r'''
import os, sys
import numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(here)r)
import oc_vjp_common as c
from pdp_amd import zoo
out = {}
for k, (system, B, T, per_sample, given, big) in enumerate(%(cases)r):
    r = c.evaluate(zoo.get(system, "irl"), c.make_inputs(system, B, T), per_sample, given, big)
    for key, v in r.items():
        out["%%d_%%s" %% (k, key)] = v
np.savez(sys.argv[1], **out)
'''


def npy(t):
    return t.detach().cpu().numpy()


def _judge(margins, tag, r):
    import oc_vjp_common as c
    assert np.isfinite(r["g"]).all() and np.abs(r["g_ref"]).max() > 0
    # 1. against the parent's own functionality: the sensitivities written out and contracted in torch
    margins.check("OC vjp %s: cotangent unit vs einsum(g, dxdp) + einsum(g, dudp) (per sample, relative to the largest entry)" % tag, c.rel_per_sample(r["g"], r["g_ref"]), TOL)
    assert np.array_equal(r["status"], r["status0"]) and not r["status"].any(), tag
    assert np.array_equal(r["x"], r["x_def"]) and np.array_equal(r["lam"], r["lam_def"]), tag
    # 3. the default mode is the special case g = x - x_demo, u - u_demo (same operations on the same bits: 0 expected)
    margins.check("OC vjp %s: cotangent unit on the default mode's residuals vs the default unit's gradient" % tag, c.rel_per_sample(r["g_special"], r["grad_def"]), TOL)


def _oracle_oc(name, _cache={}):
    from oracle import models, pdp_oracle as po
    if name not in _cache:
        st = models.IRL_SETUP[name]
        _cache[name] = po.make_oc(models.REGISTRY[name](**st["kwargs"]), st["dt"])
    return _cache[name]


def _judge_oracle(margins, tag, inp, r, per_sample, samples=(0, 1)):
    """2. against the CPU oracle: the restatement of the reference's unit on the same inputs, its sensitivities contracted with the same cotangents"""
    from oracle import pdp_oracle as po
    oc = _oracle_oc(inp["system"])
    for i in samples:
        th = inp["theta_b"][i] if per_sample else inp["theta"]
        unit = po.pdp_oc_unit(oc, inp["x0"][i], inp["u"][i], th, inp["demo_x"][i], inp["demo_u"][i])
        X, U = np.stack(unit["lqr"]["state_traj_opt"]), np.stack(unit["lqr"]["control_traj_opt"])
        gx = inp["gx"][i].copy()
        gx[0] = 0.0
        g = np.einsum("ti,tip->p", gx, X) + np.einsum("ti,tip->p", inp["gu"][i], U)
        margins.check("OC vjp %s sample %d: cotangent unit vs oracle.pdp_oc_unit sensitivities contracted with the same cotangents" % (tag, i),
                      np.abs(r["g"][i] - g).max() / np.abs(g).max(), TOL)


def _tag(case):
    system, B, T, per_sample, given, big = case
    return "%s B=%d T=%d %s theta, %s%s" % (system, B, T, "per-sample" if per_sample else "shared", "given trajectory" if given else "rollout",
                                             ", gx[:,0]=1e30" if big else "")


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
    # one wave pair per trajectory whatever the workgroup: the three layouts agree to the bit
    for k in range(len(F3_CASES)):
        assert np.array_equal(results[1, k]["g"], results[2, k]["g"]) and np.array_equal(results[1, k]["g"], results[4, k]["g"]), _tag(F3_CASES[k])
    for k in (0, 4):                            # quadrotor T = 41 shared theta, rocket T = 31 per-sample theta
        system, B, T, per_sample, given, big = F3_CASES[k]
        _judge_oracle(margins, "fused3 TPW=4 " + _tag(F3_CASES[k]), c.make_inputs(system, B, T), results[4, k], per_sample)


@pytest.mark.parametrize("case", F1_CASES, ids=[_tag(cs).replace(" ", "_") for cs in F1_CASES])
def test_one_wave_kernel(margins, case):
    import oc_vjp_common as c
    from pdp_amd import zoo
    system, B, T, per_sample, given, big = case
    inp = c.make_inputs(system, B, T)
    r = c.evaluate(zoo.get(system, "irl"), inp, per_sample, given, big)
    _judge(margins, "one-wave " + _tag(case), r)
    if T == 7:
        _judge_oracle(margins, "one-wave " + _tag(case), inp, r, per_sample)


def test_one_wave_kernel_beyond_four_states(margins, tmp_path):
    """the one-wave kernel's n > 4 branch in the cotangent mode (oc_vjp_common.run_one_wave_beyond_four_states)"""
    import oc_vjp_common as c
    c.run_one_wave_beyond_four_states(margins, tmp_path, WORKER, F3_CASES, _judge, _judge_oracle, _tag)


def test_buffers_are_reused_and_the_class_surface_forwards(margins):
    import oc_vjp_common as c
    import torch
    from pdp_amd import PDP, zoo
    from pdp_amd.sx import vertcat
    inp = c.make_inputs("cartpole", 3, 7)
    mdl = zoo.get("cartpole", "irl")
    bufs = {}
    a = mdl.oc_pdp_vjp(inp["u"], inp["theta"], inp["gx"], inp["gu"], x0=inp["x0"], buffers=bufs)
    ga, ptrs = a["grad"].clone(), {k: v.data_ptr() for k, v in bufs.items()}
    b = mdl.oc_pdp_vjp(inp["u"], inp["theta"], 2 * inp["gx"], 2 * inp["gu"], x0=inp["x0"], buffers=bufs)
    assert ptrs == {k: v.data_ptr() for k, v in bufs.items()} and set(bufs) == {"x", "lam", "grad", "status", "ws"}
    assert torch.equal(b["grad"], 2 * ga)                        # (a power of two scales every product and sum exactly)
    env, dt = zoo.make_env("cartpole", "irl")
    oc = PDP.OCSys("cartpole")
    oc.setAuxvarVariable(vertcat(env.dyn_auxvar, env.cost_auxvar))
    oc.setControlVariable(env.U)
    oc.setStateVariable(env.X)
    oc.setDyn(env.X + dt * env.f)
    oc.setPathCost(env.path_cost)
    oc.setFinalCost(env.final_cost)
    o = oc.pdp_vjp_batch(inp["u"], inp["theta"], inp["gx"], inp["gu"], ini_state=inp["x0"])
    assert torch.equal(o["grad"], ga) and sorted(o) == ["grad", "lam", "status", "x"]
    o = oc.pdp_vjp_batch(inp["u"], torch.as_tensor(inp["theta"], device="cuda"), inp["gx"], inp["gu"], state_traj=a["x"], costate_traj=a["lam"])
    assert torch.equal(o["grad"], ga)


def test_argument_errors():
    """4. PDP_OC_COTANGENT with any sensitivity output or with PDP_OC_PACKED is PDP_E_ARG; loss = NULL is accepted under the flag only"""
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
        x0, u, th, gx, gu = (rt.dev(inp[k]) for k in ("x0", "u", "theta", "gx", "gu"))
        x, lam, loss, grad, pk = torch.empty((B, T + 1, n), **f64), torch.empty((B, T, n), **f64), torch.empty((B,), **f64), torch.empty((B, p), **f64), torch.empty((B, p + 1), **f64)
        dxdp, dudp = torch.empty((B, T + 1, n, p), **f64), torch.empty((B, T, m, p), **f64)
        ric = torch.empty((B, T, int(mdl.lib.pdp_oc_riccati_doubles())), **f64)
        prec = torch.empty((B, T, int(mdl.lib.pdp_oc_predict_record_floats())), dtype=torch.float32, device="cuda")
        status = torch.zeros((B,), dtype=torch.int32, device="cuda")
        nbytes = mdl.lib.pdp_oc_pdp_workspace_bytes(B, T)
        ws = torch.empty((max(nbytes, 8) // 8,), **f64)
        P = rt.ptr

        def plain(flags, loss_t, grad_t=grad, dx=None, du=None):
            return mdl.lib.pdp_oc_pdp_grad_batched(B, T, flags, P(x0), P(u), P(th), 0, P(gx), P(gu), P(x), P(lam), P(loss_t), P(grad_t), P(dx), P(du), P(status), P(ws), nbytes,
                                                   rt.current_stream_ptr())

        def sens(flags, **kw):
            so = rt.PdpOcSensOut(*[kw[k].data_ptr() if k in kw else None for k in ("dxdp", "dudp", "riccati", "predict_record")])
            return mdl.lib.pdp_oc_pdp_grad_sens_batched(B, T, flags, P(x0), P(u), P(th), 0, P(gx), P(gu), P(x), P(lam), P(loss), P(grad), C.byref(so), P(status), P(ws),
                                                        nbytes, rt.current_stream_ptr())
        assert plain(8, loss, dx=dxdp) == -1 and plain(8, loss, du=dudp) == -1 and plain(8, loss, dx=dxdp, du=dudp) == -1
        assert sens(8, dxdp=dxdp) == -1 and sens(8, dudp=dudp) == -1 and sens(8, riccati=ric) == -1 and sens(8, predict_record=prec) == -1
        assert plain(8 | 2, loss, grad_t=pk) == -1 and plain(8 | 2 | 1, loss, grad_t=pk) == -1
        assert plain(0, None) == -1 and plain(1, None) == -1          # the default mode still needs its loss output
        assert plain(8, None) == 0 and sens(8) == 0                    # the flag alone, without and with a loss pointer
        g1 = grad.clone()
        assert plain(8, loss) == 0
        torch.cuda.synchronize()
        assert torch.equal(grad, g1) and int(status.sum()) == 0


def _wide_auxvar_oc():
    """m + p > 16 (m = 2, p = 16): the model of tests/test_gpu_edge_cases.py that the fused kernels refuse (PDP_E_SIZE)"""
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


def test_beyond_the_fused_limits_takes_the_materialised_route(margins):
    """5. PDP_E_SIZE from the entry point: oc_pdp_vjp runs the kernel-by-kernel route with the cotangents in the contraction, and warns once per model"""
    import oc_vjp_common as c
    import torch
    oc, th, rng = _wide_auxvar_oc()
    n, m, p, T, B = 6, 2, 16, 9, 2
    x0, u = 0.5 * rng.standard_normal((B, n)), 0.3 * rng.standard_normal((B, T, m))
    gx, gu = rng.standard_normal((B, T + 1, n)), rng.standard_normal((B, T, m))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        ref = oc.pdp_grad_batch(u, th, np.zeros((B, T + 1, n)), np.zeros((B, T, m)), ini_state=x0, want_sens=True)
    g_ref = torch.einsum("bti,btip->bp", torch.as_tensor(gx, device="cuda"), ref["dxdp"]) + torch.einsum("bti,btip->bp", torch.as_tensor(gu, device="cuda"), ref["dudp"])
    gx[:, 0] = 1e30
    oc.model()._warned_materialised = False
    with pytest.warns(RuntimeWarning, match="kernel-by-kernel"):
        out = oc.pdp_vjp_batch(u, th, gx, gu, ini_state=x0)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                          # once per model: the second call is silent
        out2 = oc.pdp_vjp_batch(u, th, gx, gu, state_traj=out["x"].clone(), costate_traj=out["lam"].clone())
    assert out["grad"].shape == (B, p) and int(out["status"].sum()) == 0
    margins.check("OC vjp beyond the fused limits (n=6 m=2 p=16): materialised route vs einsum(g, dxdp) + einsum(g, dudp)", c.rel_per_sample(npy(out["grad"]), npy(g_ref)), TOL)
    margins.check("OC vjp beyond the fused limits, given trajectory", c.rel_per_sample(npy(out2["grad"]), npy(g_ref)), TOL)
    assert torch.equal(out["x"], ref["x"]) and torch.equal(out["lam"], ref["lam"])


def _irl_oc(system):
    from pdp_amd import PDP, zoo
    from pdp_amd.sx import vertcat
    env, dt = zoo.make_env(system, "irl")
    oc = PDP.OCSys(system)
    oc.setAuxvarVariable(vertcat(env.dyn_auxvar, env.cost_auxvar))
    oc.setControlVariable(env.U)
    oc.setStateVariable(env.X)
    oc.setDyn(env.X + dt * env.f)
    oc.setPathCost(env.path_cost)
    oc.setFinalCost(env.final_cost)
    return oc


@pytest.mark.parametrize("system,fd_params", [("cartpole", range(7)), ("quadrotor", (0, 4, 7))])
def test_autograd_layer(margins, system, fd_params):
    """6. loss(oc_trajectory(theta)).backward(): theta.grad against the written-out sensitivities contracted with autograd's own cotangents, and against central
    differences of the loss through re-solving at theta +- 1e-5 e_k"""
    import oc_vjp_common as c
    import torch
    from pdp_amd.autograd import oc_trajectory
    oc = _irl_oc(system)
    B, T = 4, 20
    n, m = c.DIMS[system]
    rng = np.random.default_rng(3)
    if system == "cartpole":
        x0 = np.zeros((B, n))
        x0[:, 1] = rng.uniform(-0.5, 0.5, B)
        theta0 = np.array(c.THETA[system]) * (1 + 0.05 * rng.standard_normal(7))
    else:
        x0 = np.zeros((B, n))
        x0[:, 0:3] = rng.uniform(-2, 2, (B, 3))
        x0[:, 6] = 1.0
        theta0 = np.array(c.THETA[system]) * (1 + 0.05 * rng.standard_normal(9))
    w = torch.tensor([1.0, 0.5], dtype=torch.float64, device="cuda")
    cc = torch.tensor([0.3, -0.2], dtype=torch.float64, device="cuda")

    def loss_of(state, control):
        return (w * (state[:, [T // 2, T], :2] - cc) ** 2).sum() + 0.01 * (control ** 2).sum()

    def solve_loss(th):
        s, u, info = oc_trajectory(oc, x0, T, torch.as_tensor(th, dtype=torch.float64, device="cuda"), return_info=True, tol=1e-11)
        assert bool(info["converged"].all()), (system, th)
        return float(loss_of(s, u))
    # shared theta: the gradient is the sum over the batch
    theta = torch.tensor(theta0, dtype=torch.float64, device="cuda", requires_grad=True)
    state, control, info = oc_trajectory(oc, x0, T, theta, return_info=True, tol=1e-11)
    assert bool(info["converged"].all()) and state.shape == (B, T + 1, n) and control.shape == (B, T, m)
    L = loss_of(state, control)
    gs, gc = torch.autograd.grad(L, (state, control), retain_graph=True)
    L.backward()
    sens = oc.pdp_grad_batch(info["control"], theta0, np.zeros((B, T + 1, n)), np.zeros((B, T, m)), state_traj=info["state"], costate_traj=info["costate"], want_sens=True)
    g_b = torch.einsum("bti,btip->bp", gs, sens["dxdp"]) + torch.einsum("bti,btip->bp", gc, sens["dudp"])
    g_ref = npy(g_b.sum(dim=0))
    g = npy(theta.grad)
    assert g.shape == theta0.shape
    margins.check("OC layer %s B=4 T=20 shared theta: theta.grad vs autograd cotangents contracted with dxdp / dudp" % system, np.abs(g - g_ref).max() / np.abs(g_ref).max(), TOL)
    eps = 1e-5
    fd = np.array([(solve_loss(theta0 + eps * np.eye(theta0.size)[k]) - solve_loss(theta0 - eps * np.eye(theta0.size)[k])) / (2 * eps) for k in fd_params])
    margins.check("OC layer %s B=4 T=20 shared theta: theta.grad vs central differences through re-solving (relative to the largest difference)" % system,
                  np.abs(g[list(fd_params)] - fd).max() / np.abs(fd).max(), 2e-4)
    # per-sample theta [B, p]: one row each
    theta_b = torch.tensor(np.tile(theta0, (B, 1)), dtype=torch.float64, device="cuda", requires_grad=True)
    s2, u2 = oc_trajectory(oc, x0, T, theta_b, tol=1e-11)
    loss_of(s2, u2).backward()
    assert theta_b.grad.shape == (B, theta0.size)
    margins.check("OC layer %s B=4 T=20 per-sample theta: theta.grad rows vs contracted sensitivities" % system, c.rel_per_sample(npy(theta_b.grad), npy(g_b)), TOL)
    # a loss that does not touch the controls: the missing incoming gradient is zeros
    theta_c = torch.tensor(theta0, dtype=torch.float64, device="cuda", requires_grad=True)
    s3, _ = oc_trajectory(oc, x0, T, theta_c, tol=1e-11)
    (s3[:, T, 0] ** 2).sum().backward()
    g3 = torch.einsum("b,bp->p", 2 * info["state"][:, T, 0], sens["dxdp"][:, T, 0])
    margins.check("OC layer %s: states-only loss, no control cotangent" % system, np.abs(npy(theta_c.grad) - npy(g3)).max() / np.abs(npy(g3)).max(), TOL)


def test_autograd_layer_refusals():
    import torch
    from pdp_amd.autograd import oc_trajectory
    from pdp_amd import PDP
    from pdp_amd.sx import SX, dot, vertcat
    oc = _irl_oc("cartpole")
    theta = torch.tensor([0.5, 0.5, 1.0, 1.0, 6.0, 1.0, 1.0], dtype=torch.float64, device="cuda", requires_grad=True)
    x0 = torch.zeros((2, 4), dtype=torch.float64, device="cuda", requires_grad=True)
    with pytest.raises(NotImplementedError, match="ini_state"):
        oc_trajectory(oc, x0, 10, theta)
    with pytest.raises(TypeError):
        oc_trajectory(oc, x0.detach(), 10, theta.detach().cpu())
    with pytest.raises(TypeError):
        oc_trajectory(oc, x0.detach(), 10, theta.detach().float())
    x, u, w = SX.sym("x", 2), SX.sym("u", 1), SX.sym("w", 1)
    ob = PDP.OCSys("bounded double integrator")
    ob.setAuxvarVariable(w)
    ob.setStateVariable(x)
    ob.setControlVariable(u, [-1.0], [1.0])
    ob.setDyn(x + 0.1 * vertcat(x[1], u[0]))
    ob.setPathCost(w[0] * dot(x, x) + dot(u, u))
    ob.setFinalCost(dot(x, x))
    assert ob.has_bounds()
    with pytest.raises(NotImplementedError, match="bounds"):
        oc_trajectory(ob, np.zeros((2, 2)), 10, torch.ones(1, dtype=torch.float64, device="cuda", requires_grad=True))


def test_unconverged_samples_warn_once_per_call():
    import torch
    from pdp_amd.autograd import oc_trajectory
    oc = _irl_oc("cartpole")
    theta = torch.tensor([0.5, 0.5, 1.0, 1.0, 6.0, 1.0, 1.0], dtype=torch.float64, device="cuda", requires_grad=True)
    x0 = np.zeros((3, 4))
    x0[:, 1] = [0.3, -0.4, 0.5]
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        s, u = oc_trajectory(oc, x0, 20, theta, max_iter=1, neighbor_retries=0)
    assert len([r for r in rec if issubclass(r.category, RuntimeWarning) and "did not converge" in str(r.message)]) == 1
    s.sum().backward()                                           # differentiated at the last iterate
    assert theta.grad.shape == (7,) and bool(torch.isfinite(theta.grad).all())


def test_custom_loss_example_learns():
    """7. examples/oc_layer_custom_loss.py: three optimiser steps at B = 4, the printed loss decreases"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "oc_layer_custom_loss.py"), "--iters", "3", "--batch", "4"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    losses = [float(ln.split("loss")[1].split()[0]) for ln in r.stdout.splitlines() if ln.startswith("iter")]
    assert len(losses) == 3 and losses[2] < losses[1] < losses[0], r.stdout
