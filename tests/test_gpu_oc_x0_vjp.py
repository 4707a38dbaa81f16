"""GPU: the gradient of a loss on the OC solution with respect to the INITIAL STATE - pdp_oc_sens_out.grad_x0 of pdp_oc_pdp_grad_sens_batched (the adjoint sweep
oc_x0_vjp_kernel behind the fused unit's launch), ModelLib.oc_pdp_vjp / oc_pdp_grad(want_ini=True), OCSys.pdp_vjp_batch, and oc_trajectory(..., ini_grad=True).

Reference (oc_x0_vjp_common): the oracle's auxiliary system at the oracle's own rollout, the reference's lqr_solver from X_0 = [0 | I] - forward sensitivities with
its explicit inverses, not the kernel's adjoint sweep - contracted with the cotangents; tests/test_oc_x0_vjp_host.py holds the reference's own error on exactly these
cases below 1e-11.  Tolerance: 1e-10 of the largest entry per sample (tests/test_gpu_oc_vjp.py's TOL).

Shapes: B <= 4.  T = 20 on the four zoo systems - pendulum and cart-pole run the one-wave fused kernel, quadrotor and rocket the runner / evaluator pair - and, for
the sweep's chunks, T = 1, R - 1, R, R + 1, 2 R + 1 with R = oc_x0_vjp_rows() on pendulum (R = 64) and quadrotor (R = 22)."""
import ctypes as C
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

WORKER = r'''
import sys
import numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(here)r)
import oc_x0_vjp_common as cx
from pdp_amd import zoo
r = cx.evaluate(zoo.get("quadrotor", "irl"), cx.inputs("quadrotor", cx.B_MAIN, cx.T_MAIN))
np.savez(sys.argv[1], **r)
'''


def npy(t):
    return t.detach().cpu().numpy()


def _judge(margins, tag, r, ref):
    import oc_vjp_common as c
    assert np.isfinite(r["grad_x0"]).all() and not r["status"].any(), tag
    margins.check("OC x0 vjp %s: grad_x0 vs the reference's forward sensitivities from X_0 = I contracted with the cotangents" % tag, c.rel_per_sample(r["grad_x0"], ref), TOL)
    # the same fused launch: every other output keeps its bits
    for k in ("grad", "x", "lam", "status"):
        assert np.array_equal(r[k], r[k + "_plain"]), (tag, k)


@pytest.mark.parametrize("given", [False, True], ids=["rollout", "given_trajectory"])
@pytest.mark.parametrize("per_sample", [False, True], ids=["shared_theta", "per_sample_theta"])
@pytest.mark.parametrize("system", ["pendulum", "cartpole", "quadrotor", "rocket"])
def test_each_zoo_system_in_the_cotangent_mode(margins, system, per_sample, given):
    import oc_x0_vjp_common as cx
    from pdp_amd import zoo
    r = cx.evaluate(zoo.get(system, "irl"), cx.inputs(system, cx.B_MAIN, cx.T_MAIN), per_sample, given)
    ref = cx.reference_case(system, cx.B_MAIN, cx.T_MAIN, per_sample)["ref"]
    _judge(margins, "%s B=%d T=%d %s theta, %s" % (system, cx.B_MAIN, cx.T_MAIN, "per-sample" if per_sample else "shared", "given trajectory" if given else "rollout"), r, ref)


@pytest.mark.parametrize("system,k", [(s, k) for s in ("pendulum", "quadrotor") for k in range(5)],
                         ids=["%s_%s" % (s, e) for s in ("pendulum", "quadrotor") for e in ("T1", "R-1", "R", "R+1", "2R+1")])
def test_chunk_edges(margins, system, k):
    import oc_x0_vjp_common as cx
    from pdp_amd import zoo
    mdl = zoo.get(system, "irl")
    R = mdl.oc_x0_vjp_rows()
    assert R == cx.ROWS[system]
    T = (1, R - 1, R, R + 1, 2 * R + 1)[k]
    r = cx.evaluate(mdl, cx.inputs(system, cx.B_EDGE, T))
    _judge(margins, "%s B=%d T=%d (rows %d)" % (system, cx.B_EDGE, T, R), r, cx.reference_case(system, cx.B_EDGE, T, False)["ref"])


@pytest.mark.parametrize("system", ["cartpole", "quadrotor"])
def test_exact_values(system):
    import oc_x0_vjp_common as cx
    import torch
    from pdp_amd import zoo
    mdl = zoo.get(system, "irl")
    inp = cx.inputs(system, 3, cx.T_MAIN)
    n = mdl.n
    zx, zu = np.zeros_like(inp["gx"]), np.zeros_like(inp["gu"])
    # all-zero cotangents: exact zeros
    out = mdl.oc_pdp_vjp(inp["u"], inp["theta"], zx, zu, x0=inp["x0"], want_ini=True)
    assert int(out["status"].sum()) == 0 and bool((out["grad_x0"] == 0).all())
    # only state[0]'s own cotangent: mu stays 0 down to step 0, grad_x0 = gx_0 to the bit
    cvec = np.random.default_rng(1).standard_normal((3, n))
    gx = zx.copy()
    gx[:, 0] = cvec
    out = mdl.oc_pdp_vjp(inp["u"], inp["theta"], gx, zu, x0=inp["x0"], want_ini=True)
    assert np.array_equal(npy(out["grad_x0"]), cvec)
    # a trajectory's row: the same bits alone and as the last of three
    full = mdl.oc_pdp_vjp(inp["u"], inp["theta_b"], inp["gx"], inp["gu"], x0=inp["x0"], want_ini=True)
    last = mdl.oc_pdp_vjp(inp["u"][2:], inp["theta_b"][2:], inp["gx"][2:], inp["gu"][2:], x0=inp["x0"][2:], want_ini=True)
    assert torch.equal(full["grad_x0"][2:], last["grad_x0"]) and bool(torch.isfinite(full["grad_x0"]).all())


@pytest.mark.parametrize("system", ["cartpole", "quadrotor"])
def test_default_mode(margins, system):
    """half the gradient of the demonstration loss: the cotangent-mode result for g = x - demo; alone, packed, and beside the sensitivity outputs"""
    import oc_vjp_common as c
    import oc_x0_vjp_common as cx
    import torch
    from pdp_amd import runtime as rt, zoo
    mdl = zoo.get(system, "irl")
    inp = cx.inputs(system, cx.B_MAIN, cx.T_MAIN)
    u, dx, du = rt.dev(inp["u"]), rt.dev(inp["demo_x"]), rt.dev(inp["demo_u"])
    d0 = mdl.oc_pdp_grad(u, inp["theta"], dx, du, x0=inp["x0"])
    d1 = mdl.oc_pdp_grad(u, inp["theta"], dx, du, x0=inp["x0"], want_ini=True)
    for k in ("loss", "grad", "x", "lam", "status"):
        assert torch.equal(d0[k], d1[k]), k
    v = mdl.oc_pdp_vjp(u, inp["theta"], d0["x"] - dx, u - du, x0=inp["x0"], want_ini=True)
    margins.check("OC x0 vjp %s: default mode's grad_x0 vs the cotangent mode on x - demo, u - demo" % system, c.rel_per_sample(npy(d1["grad_x0"]), npy(v["grad_x0"])), TOL)
    d2 = mdl.oc_pdp_grad(u, inp["theta"], dx, du, x0=inp["x0"], want_ini=True, packed=True)
    d3 = mdl.oc_pdp_grad(u, inp["theta"], dx, du, x=d0["x"].clone(), lam=d0["lam"].clone(), want_ini=True, want_sens=True, want_riccati=True)
    s3 = mdl.oc_pdp_grad(u, inp["theta"], dx, du, x=d0["x"].clone(), lam=d0["lam"].clone(), want_sens=True, want_riccati=True)
    assert torch.equal(d2["grad_x0"], d1["grad_x0"]) and torch.equal(d2["packed"][:, :-1], d0["grad"]) and torch.equal(d2["packed"][:, -1], d0["loss"])
    assert torch.equal(d3["grad_x0"], d1["grad_x0"])
    for k in ("loss", "grad", "dxdp", "dudp", "status"):
        assert torch.equal(d3[k], s3[k]), k
    # (P_{t+1} | W_{t+1} of every stage; the record's last word is scratch, which the runner / evaluator kernel never writes: whatever the allocation held)
    assert torch.equal(d3["riccati"][..., :-1], s3["riccati"][..., :-1])


def test_refusals_through_the_c_entry_point():
    """PDP_GRAD_GAUSS_NEWTON / PDP_GRAD_SKIP_MISSING with grad_x0: PDP_E_ARG and nothing written; the other four fields stay PDP_E_ARG under PDP_OC_COTANGENT"""
    import oc_x0_vjp_common as cx
    import torch
    from pdp_amd import runtime as rt, zoo
    for system in ("cartpole", "quadrotor"):
        mdl = zoo.get(system, "irl")
        n, m, p = mdl.n, mdl.m, mdl.p
        B, T = 2, 7
        inp = cx.inputs(system, B, T)
        f64 = dict(dtype=torch.float64, device="cuda")
        x0, u, th, gx, gu = (rt.dev(inp[k]) for k in ("x0", "u", "theta", "demo_x", "demo_u"))
        mark = -7.25
        x, lam, loss = torch.full((B, T + 1, n), mark, **f64), torch.full((B, T, n), mark, **f64), torch.full((B,), mark, **f64)
        grad, gx0 = torch.full((B, p + 1 + p * p), mark, **f64), torch.full((B, n), mark, **f64)
        dxdp = torch.empty((B, T + 1, n, p), **f64)
        status = torch.full((B,), 77, dtype=torch.int32, device="cuda")
        nbytes = mdl.lib.pdp_oc_pdp_workspace_bytes(B, T)
        ws = torch.empty((max(nbytes, 8) // 8,), **f64)
        P = rt.ptr

        def sens(flags, so, wsb=nbytes):
            return mdl.lib.pdp_oc_pdp_grad_sens_batched(B, T, flags, P(x0), P(u), P(th), 0, P(gx), P(gu), P(x), P(lam), P(loss), P(grad), C.byref(so), P(status), P(ws),
                                                        wsb, rt.current_stream_ptr())
        only = rt.PdpOcSensOut(None, None, None, None, gx0.data_ptr())
        for flags in (16, 32, 16 | 32, 16 | 1, 32 | 2):
            assert sens(flags, only) == -1, (system, flags)
        assert sens(8, rt.PdpOcSensOut(dxdp.data_ptr(), None, None, None, gx0.data_ptr())) == -1
        assert sens(0, only, wsb=nbytes - 8) == -1                   # a workspace the fused launch refuses
        torch.cuda.synchronize()
        for t in (x, lam, loss, grad, gx0):
            assert bool((t == mark).all())
        assert bool((status == 77).all())
        assert sens(16, rt.PdpOcSensOut(None, None, None, None)) == 0 and sens(8, only) == 0 and sens(0, only) == 0
        torch.cuda.synchronize()
        assert bool(torch.isfinite(gx0).all()) and int(status.sum()) == 0


def test_runner_evaluator_kernel_at_1_2_4_trajectories_per_workgroup(margins, tmp_path):
    """the gains the sweep reads are written by the runner / evaluator pair in each of its workgroup layouts (PDP_FUSED_TPW, read once per process): one child process
    per value, one after another, each under its own timeout; B = 3 leaves the last workgroup ragged at 2 and 4"""
    import oc_x0_vjp_common as cx
    ref = cx.reference_case("quadrotor", cx.B_MAIN, cx.T_MAIN, False)["ref"]
    got = {}
    for tpw in (1, 2, 4):                       # (stops at the first failing child: the assert ends the test)
        path = str(tmp_path / ("tpw%d.npz" % tpw))
        env = dict(os.environ, PDP_FUSED_TPW=str(tpw))
        env.pop("PDP_FUSED_VARIANT", None)
        r = subprocess.run([sys.executable, "-c", WORKER % dict(root=ROOT, here=HERE), path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240, env=env)
        assert r.returncode == 0, "PDP_FUSED_TPW=%d: exit %d\n%s" % (tpw, r.returncode, r.stdout[-3000:])
        z = np.load(path)
        got[tpw] = {k: z[k] for k in z.files}
        _judge(margins, "quadrotor B=3 T=20, %d trajectories per workgroup" % tpw, got[tpw], ref)
    assert np.array_equal(got[1]["grad_x0"], got[2]["grad_x0"]) and np.array_equal(got[1]["grad_x0"], got[4]["grad_x0"])


def test_beyond_the_fused_limits_takes_the_materialised_route(margins):
    """n = 6, m = 2, p = 16: PDP_E_SIZE from the entry point; want_ini through the kernel-by-kernel route (n further columns, X_0 = [0 | I]) against an LQ solve of its
    own whose only columns start at X_0 = I, contracted with the cotangents"""
    import oc_vjp_common as c
    import oc_x0_vjp_common as cx
    import torch
    from pdp_amd import runtime as rt
    oc, th, rng = cx.wide_auxvar_oc()
    n, m, p, T, B = 6, 2, 16, 9, 2
    x0, u = 0.5 * rng.standard_normal((B, n)), 0.3 * rng.standard_normal((B, T, m))
    gx, gu = rng.standard_normal((B, T + 1, n)), rng.standard_normal((B, T, m))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        plain = oc.pdp_vjp_batch(u, th, gx, gu, ini_state=x0)
        out = oc.pdp_vjp_batch(u, th, gx, gu, ini_state=x0, want_ini=True)
        dflt = oc.pdp_grad_batch(u, th, np.zeros((B, T + 1, n)), np.zeros((B, T, m)), ini_state=x0, want_ini=True)
    assert int(out["status"].sum()) == 0 and torch.equal(out["x"], plain["x"]) and torch.equal(out["lam"], plain["lam"])
    aux = oc.getAuxSys_batch(out["x"], u, out["lam"], th)
    f64 = dict(dtype=torch.float64, device="cuda")
    X, U, _, st = rt.lqr_solve(aux["dynF"], aux["dynG"], aux["Hxx"], aux["Huu"], aux["hxx"], torch.zeros((B, n, n), **f64), E=torch.zeros((B, T, n, n), **f64), Hxu=aux["Hxu"],
                               Hxe=torch.zeros((B, T, n, n), **f64), Hue=torch.zeros((B, T, m, n), **f64), X0=torch.eye(n, **f64), want_costate=False)
    gxd, gud = rt.dev(gx), rt.dev(gu)
    ref = torch.einsum("bti,btik->bk", gxd, X) + torch.einsum("bti,btik->bk", gud, U)
    assert out["grad_x0"].shape == (B, n) and int(st.sum()) == 0
    margins.check("OC x0 vjp beyond the fused limits (n=6 m=2 p=16): materialised route vs sensitivities started at X_0 = I", c.rel_per_sample(npy(out["grad_x0"]), npy(ref)), TOL)
    margins.check("OC x0 vjp beyond the fused limits: theta gradient beside grad_x0 vs the call without it", c.rel_per_sample(npy(out["grad"]), npy(plain["grad"])), TOL)
    ref0 = torch.einsum("bti,btik->bk", dflt["x"], X) + torch.einsum("bti,btik->bk", rt.dev(u), U)          # default mode, demonstration 0: g = x, u
    margins.check("OC x0 vjp beyond the fused limits, default mode", c.rel_per_sample(npy(dflt["grad_x0"]), npy(ref0)), TOL)


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


@pytest.mark.parametrize("system,fd_at", [("cartpole", ((0, 1), (1, 3), (3, 0))), ("quadrotor", ((0, 0), (2, 4), (3, 11)))])
def test_autograd_layer_with_ini_grad(margins, system, fd_at):
    """loss(oc_trajectory(ini_state, theta, ini_grad=True)).backward(): ini_state.grad against the reference at the solved trajectory contracted with autograd's own
    cotangents, and against central differences through re-solving at x0 +- 1e-5 e_k for three (sample, component) pairs; theta.grad keeps its bits"""
    import oc_vjp_common as c
    import oc_x0_vjp_common as cx
    import torch
    from pdp_amd.autograd import oc_trajectory
    oc = _irl_oc(system)
    B, T = 4, 20
    n, m = c.DIMS[system]
    rng = np.random.default_rng(3)
    x0 = np.zeros((B, n))
    if system == "cartpole":
        x0[:, 1] = rng.uniform(-0.5, 0.5, B)
    else:
        x0[:, 0:3] = rng.uniform(-2, 2, (B, 3))
        x0[:, 6] = 1.0
    theta0 = np.array(c.THETA[system]) * (1 + 0.05 * rng.standard_normal(len(c.THETA[system])))
    w = torch.tensor([1.0, 0.5], dtype=torch.float64, device="cuda")
    cc = torch.tensor([0.3, -0.2], dtype=torch.float64, device="cuda")
    f64 = dict(dtype=torch.float64, device="cuda")

    def loss_of(state, control):
        return (w * (state[:, [T // 2, T], :2] - cc) ** 2).sum() + 0.01 * (control ** 2).sum() + 0.5 * (state[:, 0] ** 2).sum()

    theta = torch.tensor(theta0, requires_grad=True, **f64)
    ini = torch.tensor(x0, requires_grad=True, **f64)
    state, control, info = oc_trajectory(oc, ini, T, theta, return_info=True, ini_grad=True, tol=1e-11)
    assert bool(info["converged"].all()) and state.shape == (B, T + 1, n)
    L = loss_of(state, control)
    gs, gc = torch.autograd.grad(L, (state, control), retain_graph=True)
    L.backward()
    assert ini.grad.shape == (B, n) and theta.grad.shape == theta0.shape
    ocr = cx.oracle_oc(system)
    xs, us, ls = npy(info["state"]), npy(info["control"]), npy(info["costate"])
    ref = np.stack([cx.reference_grad_x0(ocr, xs[i], us[i], ls[i], theta0, npy(gs)[i], npy(gc)[i]) for i in range(B)])
    margins.check("OC layer %s B=4 T=20: ini_state.grad vs the reference contracted with autograd's cotangents" % system, c.rel_per_sample(npy(ini.grad), ref), TOL)
    # theta.grad of the same backward: the bits of a backward without ini_grad
    theta2 = torch.tensor(theta0, requires_grad=True, **f64)
    s2, u2 = oc_trajectory(oc, x0, T, theta2, tol=1e-11)
    loss_of(s2, u2).backward()
    assert torch.equal(theta.grad, theta2.grad)
    # a theta that requires no gradient is allowed, and ini_state.grad is the same
    ini3 = torch.tensor(x0, requires_grad=True, **f64)
    s3, u3 = oc_trajectory(oc, ini3, T, theta.detach(), ini_grad=True, tol=1e-11)
    loss_of(s3, u3).backward()
    assert torch.equal(ini3.grad, ini.grad)

    def solve_loss(x0v):
        s, u, inf = oc_trajectory(oc, torch.tensor(x0v, **f64), T, theta.detach(), return_info=True, ini_grad=True, tol=1e-11)
        assert bool(inf["converged"].all())
        return float(loss_of(s, u))
    eps, fd, got = 1e-5, [], []
    for b, k in fd_at:
        e = np.zeros((B, n))
        e[b, k] = eps
        fd.append((solve_loss(x0 + e) - solve_loss(x0 - e)) / (2 * eps))
        got.append(float(ini.grad[b, k]))
    fd, got = np.array(fd), np.array(got)
    margins.check("OC layer %s B=4 T=20: ini_state.grad vs central differences through re-solving (relative to the largest difference)" % system,
                  np.abs(got - fd).max() / np.abs(fd).max(), 2e-4)


def test_autograd_layer_refusals_with_and_without_the_keyword():
    import torch
    from pdp_amd.autograd import oc_trajectory
    oc = _irl_oc("cartpole")
    theta = torch.tensor([0.5, 0.5, 1.0, 1.0, 6.0, 1.0, 1.0], dtype=torch.float64, device="cuda", requires_grad=True)
    x0 = torch.zeros((2, 4), dtype=torch.float64, device="cuda", requires_grad=True)
    with pytest.raises(NotImplementedError, match="ini_state"):       # without the keyword: the refusal of before
        oc_trajectory(oc, x0, 10, theta)
    with pytest.raises(TypeError, match="ini_grad"):
        oc_trajectory(oc, x0.detach().cpu(), 10, theta, ini_grad=True)
    with pytest.raises(TypeError, match="ini_grad"):
        oc_trajectory(oc, x0.detach().float(), 10, theta, ini_grad=True)
    with pytest.raises(TypeError, match="ini_grad"):
        oc_trajectory(oc, np.zeros((2, 4)), 10, theta, ini_grad=True)
    with pytest.raises(TypeError):
        oc_trajectory(oc, x0, 10, theta.detach().cpu(), ini_grad=True)
