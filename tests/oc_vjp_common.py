"""Shared by tests/test_gpu_oc_vjp.py (in-process and in its child processes): inputs of the cotangent-mode tests and the calls every shape goes through."""
import numpy as np

THETA = {"pendulum": [1.0, 1.0, 0.1, 10.0, 1.0],
         "cartpole": [0.5, 0.5, 1.0, 1.0, 6.0, 1.0, 1.0],
         "quadrotor": [1.0, 1.0, 1.0, 1.0, 0.4, 1.0, 1.0, 5.0, 1.0],
         "rocket": [0.5, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 50.0, 1.0, 1.0]}
DIMS = {"pendulum": (2, 1), "cartpole": (4, 1), "quadrotor": (13, 4), "rocket": (13, 3)}


def make_inputs(system, B, T, seed=7):
    """random controls of moderate size around rest / hover (the inputs of tests/test_gpu_fused_variants.py for the 13-state systems), standard normal cotangents,
    a demonstration for the default mode, one shared and one per-sample parameter; fixed seed"""
    n, m = DIMS[system]
    rng = np.random.default_rng(seed)
    theta = np.asarray(THETA[system], dtype=np.float64)
    if n == 13:
        x0 = np.zeros((B, n))
        x0[:, 0:3] = rng.uniform(-2, 2, (B, 3))
        x0[:, 3:6] = 0.1 * rng.standard_normal((B, 3))
        q = np.concatenate([np.ones((B, 1)), 0.1 * rng.standard_normal((B, 3))], axis=1)
        x0[:, 6:10] = q / np.linalg.norm(q, axis=1, keepdims=True)
        x0[:, 10:13] = 0.05 * rng.standard_normal((B, 3))
        if system == "quadrotor":
            u = 2.5 + 0.05 * rng.standard_normal((B, T, m))       # hover thrust per rotor
        else:
            u = 0.05 * rng.standard_normal((B, T, m))
            u[:, :, 0] += 10.0                                      # hover thrust along the body axis
    else:
        x0 = 0.1 * rng.standard_normal((B, n))
        u = 0.1 * rng.standard_normal((B, T, m))
    return dict(system=system, B=B, T=T, x0=x0, u=u, theta=theta, theta_b=theta[None, :] * (1 + 0.05 * rng.standard_normal((B, theta.size))),
                gx=rng.standard_normal((B, T + 1, n)), gu=rng.standard_normal((B, T, m)),
                demo_x=0.1 * rng.standard_normal((B, T + 1, n)), demo_u=u + 0.1 * rng.standard_normal((B, T, m)))


def evaluate(mdl, inp, per_sample=False, given=False, big_gx0=False):
    """One shape through: the default unit (plain, and with the sensitivities written), the cotangent unit on (gx, gu), and the cotangent unit on the default
    mode's own residuals.  given: the cotangent calls get the default call's (x, lam) (PDP_OC_GIVEN_TRAJ), else they roll out from x0.  big_gx0: gx[:, 0] = 1e30
    (it must not be read).  Returns numpy arrays; g_ref = einsum(gx, dxdp) + einsum(gu, dudp) in torch fp64."""
    import torch
    from pdp_amd import runtime as rt
    th = inp["theta_b"] if per_sample else inp["theta"]
    u, x0, demo_x, demo_u = rt.dev(inp["u"]), inp["x0"], rt.dev(inp["demo_x"]), rt.dev(inp["demo_u"])
    gx, gu = rt.dev(inp["gx"]).clone(), rt.dev(inp["gu"])
    d0 = mdl.oc_pdp_grad(u, th, demo_x, demo_u, x0=x0)
    ds = mdl.oc_pdp_grad(u, th, demo_x, demo_u, x0=x0, want_sens=True)
    g_ref = torch.einsum("bti,btip->bp", gx, ds["dxdp"]) + torch.einsum("bti,btip->bp", gu, ds["dudp"])
    if big_gx0:
        gx[:, 0] = 1e30
    traj = dict(x=d0["x"].clone(), lam=d0["lam"].clone()) if given else dict(x0=x0)
    v = mdl.oc_pdp_vjp(u, th, gx, gu, **traj)
    traj = dict(x=d0["x"].clone(), lam=d0["lam"].clone()) if given else dict(x0=x0)
    s = mdl.oc_pdp_vjp(u, th, d0["x"] - demo_x, u - demo_u, **traj)
    npy = lambda t: t.detach().cpu().numpy()
    return dict(g=npy(v["grad"]), g_ref=npy(g_ref), status=npy(v["status"]), status0=npy(d0["status"]), x=npy(v["x"]), x_def=npy(d0["x"]), lam=npy(v["lam"]),
                lam_def=npy(d0["lam"]), g_special=npy(s["grad"]), grad_def=npy(d0["grad"]))


def rel_per_sample(a, b):
    """max_b  max|a_b - b_b| / max|b_b|"""
    a, b = np.asarray(a), np.asarray(b)
    return max(np.abs(a[i] - b[i]).max() / np.abs(b[i]).max() for i in range(a.shape[0]))


def run_one_wave_beyond_four_states(margins, tmp_path, worker, f3_cases, judge, judge_oracle, tag):
    """The one-wave kernel's n > 4 branch (full tiles, not its small-system form): what a long horizon (quadrotor T >= 260) or PDP_FUSED_VARIANT=1 selects where the
    runner / evaluator kernel runs by default.  The switch is read once per process: one child process runs the calling file's WORKER on two of its runner / evaluator
    cases - quadrotor B = 5, T = 41, shared theta, rollout: two chunks of the one-wave kernel too, 21 + 20 steps (FusedChunk = the generated CHUNK = 33) - and rocket
    B = 5, T = 31, given trajectory (CHUNK 28: 16 + 15).  Judged by the calling file's own checks at its own tolerance (the reference is the same process's want_sens
    output); the oracle where that file compares it: the quadrotor case."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    cases = [f3_cases[0], f3_cases[3]]
    assert cases[0][:5] == ("quadrotor", 5, 41, False, False) and cases[1][:5] == ("rocket", 5, 31, False, True)
    path = str(tmp_path / "variant1.npz")
    r = subprocess.run([sys.executable, "-c", worker % dict(root=os.path.dirname(here), here=here, cases=cases), path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=300, env=dict(os.environ, PDP_FUSED_VARIANT="1"))
    assert r.returncode == 0, r.stdout[-3000:]
    z = np.load(path)
    for k, case in enumerate(cases):
        res = {key.split("_", 1)[1]: z[key] for key in z.files if key.startswith("%d_" % k)}
        judge(margins, "one-wave n > 4 " + tag(case), res)
        if k == 0:
            judge_oracle(margins, "one-wave n > 4 " + tag(case), make_inputs(*case[:3]), res, case[3])

