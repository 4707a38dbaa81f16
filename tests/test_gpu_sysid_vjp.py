"""GPU: the SysID rollout as a vector-Jacobian product (pdp_sysid_rollout_vjp_batched, sysid_vjp_kernel) and the autograd layer on it, against the forward-sensitivity
reference of tests/sysid_vjp_common.py: 1e-10 of the largest entry per sample."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import sysid_vjp_common as sv

pytestmark = pytest.mark.gpu
TOL = sv.TOL


def npy(t):
    return t.detach().cpu().numpy()


def model(system):
    from pdp_amd import zoo
    return zoo.get(system, "sysid")


def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


def run(mdl, c, theta_key="theta", g=None, **kw):
    """rollout on the GPU from the case's initial states, then the new entry point: (states, dict of numpy outputs)"""
    x = mdl.sysid_integrate(c["x0"], c["inputs"], c[theta_key])
    out = mdl.sysid_rollout_vjp(x, c["inputs"], c[theta_key], c["g"] if g is None else g, **kw)
    return x, {k: npy(v) for k, v in out.items()}


@pytest.mark.parametrize("system", sv.SYSTEMS)
def test_stored_data_against_the_reference(margins, system):
    """the stored inputs (T = 10 or 20), shared and per-sample theta; both outputs, and each one alone (the other NULL) to the bit"""
    mdl, c = model(system), sv.case(system)
    for key, sfx in (("theta", ""), ("theta_b", "_b")):
        x, out = run(mdl, c, key)
        tag = "sysid vjp %s %s theta" % (system, "per-sample" if sfx else "shared")
        margins.check(tag + ": rollout", sv.rel_rows(npy(x), c["states" + sfx]), TOL)
        margins.check(tag + ": grad_theta", sv.rel_rows(out["grad_theta"], c["grad_theta" + sfx]), TOL)
        margins.check(tag + ": grad_x0", sv.rel_rows(out["grad_x0"], c["grad_x0" + sfx]), TOL)
        _, only_theta = run(mdl, c, key, want_ini=False)
        _, only_ini = run(mdl, c, key, want_theta=False)
        assert set(only_theta) == {"grad_theta"} and set(only_ini) == {"grad_x0"}
        assert same_bits(only_theta["grad_theta"], out["grad_theta"]) and same_bits(only_ini["grad_x0"], out["grad_x0"])


@pytest.mark.parametrize("system", ["pendulum", "cartpole", "quadrotor"])
def test_chunk_edges(margins, system):
    """T = 1 (the chain never iterates), and T = R - 1, R, R + 1, 2 R + 1 around the R pool rows of the launch; the longest horizon is the shared case (pendulum and
    cart-pole 65, quadrotor 33 = R + 1), shorter ones are its prefixes with their own reference"""
    mdl, sid = model(system), sv.oracle(system)
    R = mdl.sysid_vjp_rows(3, cus())
    assert R == mdl.chunk == 32
    long = sv.case(system, sv.EDGE_T[system])
    for T in [t for t in (1, R - 1, R, R + 1, 2 * R + 1) if t <= sv.EDGE_T[system]]:
        if T == sv.EDGE_T[system]:
            c = long
        else:
            c = dict(x0=long["x0"], inputs=long["inputs"][:, :T], theta=long["theta"], g=long["g"][:, :T + 1])
            _, c["grad_theta"], c["grad_x0"] = sv.reference(sid, c["x0"], c["inputs"], c["theta"], c["g"])
        x, out = run(mdl, c)
        margins.check("sysid vjp %s T = %d: grad_theta" % (system, T), sv.rel_rows(out["grad_theta"], c["grad_theta"]), TOL)
        margins.check("sysid vjp %s T = %d: grad_x0" % (system, T), sv.rel_rows(out["grad_x0"], c["grad_x0"]), TOL)
        if T == 1:                                       # grad_theta = E_0' g_1, grad_x0 = g_0 + F_0' g_1 from the oracle's Jacobians directly
            for b in range(len(c["x0"])):
                aux = sid.getAuxSys(npy(x)[b], c["inputs"][b], c["theta"])
                margins.check("sysid vjp %s T = 1 sample %d: E_0' g_1" % (system, b), sv.rel_rows(out["grad_theta"][b:b + 1], (aux["dynE"][0].T @ c["g"][b, 1])[None]), TOL)
                margins.check("sysid vjp %s T = 1 sample %d: g_0 + F_0' g_1" % (system, b),
                              sv.rel_rows(out["grad_x0"][b:b + 1], (c["g"][b, 0] + aux["dynF"][0].T @ c["g"][b, 1])[None]), TOL)


@pytest.mark.parametrize("system", sv.SYSTEMS)
def test_the_residual_cotangent_reproduces_sysid_step(margins, system):
    """g = x - x_obs: the gradient of SysID.step_batch (forward sensitivities on MFMA tiles) from the adjoint sweep"""
    from pdp_amd import runtime as rt
    mdl = model(system)
    inputs, states, _, theta = sv.stored(system)
    _, grad = mdl.sysid_step(inputs, states, theta)
    x = mdl.sysid_integrate(states[:, 0], inputs, theta)
    out = mdl.sysid_rollout_vjp(x, inputs, theta, x - rt.dev(states), want_ini=False)
    margins.check("sysid vjp %s, g = x - x_obs, vs SysID.step_batch's gradient" % system, sv.rel_rows(npy(out["grad_theta"]), npy(grad)), TOL)


@pytest.mark.parametrize("system", ["pendulum", "quadrotor"])
def test_exact_zeros_and_single_step_cotangents(margins, system):
    mdl, c = model(system), sv.case(system)
    z = np.zeros_like(c["g"])
    _, out = run(mdl, c, g=z)
    assert not out["grad_theta"].any() and not out["grad_x0"].any()
    first = z.copy()
    first[:, 0] = c["g"][:, 0]
    _, out = run(mdl, c, g=first)
    assert not out["grad_theta"].any() and same_bits(out["grad_x0"], c["g"][:, 0])
    last = z.copy()
    last[:, -1] = c["g"][:, -1]
    _, gt, g0 = sv.reference(c["sid"], c["x0"], c["inputs"], c["theta"], last)
    _, out = run(mdl, c, g=last)
    margins.check("sysid vjp %s, cotangent at t = T only: grad_theta" % system, sv.rel_rows(out["grad_theta"], gt), TOL)
    margins.check("sysid vjp %s, cotangent at t = T only: grad_x0" % system, sv.rel_rows(out["grad_x0"], g0), TOL)


@pytest.mark.parametrize("system", ["pendulum", "quadrotor"])
def test_output_bits_do_not_depend_on_the_batch(system):
    """three trajectories sent alone (B = 1) and inside B = 2 #CU + 1 and B = 4 #CU + 1 (where the host sizes the pool for two workgroups per SIMD), first, middle and
    last position: the same bits"""
    import torch
    mdl, c = model(system), sv.case(system)
    alone = []
    for b in range(3):
        one = dict(x0=c["x0"][b:b + 1], inputs=c["inputs"][b:b + 1], theta_b=c["theta_b"][b:b + 1], g=c["g"][b:b + 1])
        alone.append(run(mdl, one, "theta_b")[1])
    for B in (2 * cus() + 1, 4 * cus() + 1):
        pos = [0, B // 2, B - 1]
        idx = np.arange(B) % c["inputs"].shape[0]
        idx[pos] = [0, 1, 2]
        big = dict(x0=c["x0"][idx], inputs=c["inputs"][idx], theta_b=c["theta_b"][idx], g=c["g"][idx])
        _, out = run(mdl, big, "theta_b")
        for k, b in enumerate(pos):
            assert same_bits(out["grad_theta"][b], alone[k]["grad_theta"][0]) and same_bits(out["grad_x0"][b], alone[k]["grad_x0"][0]), (B, b)
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", sorted(sv.USER_MODELS))
def test_sizes_beyond_the_fused_tiles(margins, name):
    """n = 40 (beyond sysid_step_kernel's tiles) and p = 99 (a second 64-lane parameter slot), through the class surface against SysIDOracle from sympy"""
    c = sv.user_case(name)
    sid = c["sid"]
    x = sid.integrateDyn_batch(c["x0"], c["inputs"], c["theta"])
    out = sid.rollout_vjp_batch(x, c["inputs"], c["theta"], c["g"])
    assert tuple(out["grad_theta"].shape) == (3, c["orc"].p) and tuple(out["grad_x0"].shape) == (3, c["orc"].n)
    margins.check("sysid vjp %s: rollout" % name, sv.rel_rows(npy(x), c["states"]), TOL)
    margins.check("sysid vjp %s: grad_theta" % name, sv.rel_rows(npy(out["grad_theta"]), c["grad_theta"]), TOL)
    margins.check("sysid vjp %s: grad_x0" % name, sv.rel_rows(npy(out["grad_x0"]), c["grad_x0"]), TOL)


def test_a_nan_stays_in_its_trajectory():
    mdl, c = model("quadrotor"), sv.case("quadrotor")
    _, clean = run(mdl, c)
    g = c["g"].copy()
    g[1, 4, 2] = np.nan
    _, out = run(mdl, c, g=g)
    assert np.isnan(out["grad_x0"][1]).any() and np.isnan(out["grad_theta"][1]).any()
    for b in (0, 2):
        assert same_bits(out["grad_theta"][b], clean["grad_theta"][b]) and same_bits(out["grad_x0"][b], clean["grad_x0"][b])


def test_the_layer_on_the_pendulum(margins):
    """B = 2, T = 5, L = sum w . state^2: theta.grad and ini_state.grad equal the reference contraction with g = 2 w . state; a shared theta's gradient is the sum of
    the per-sample rows; what the layer cannot differentiate is refused"""
    import torch
    from pdp_amd import PDP, zoo
    from pdp_amd.autograd import sysid_trajectory
    c = sv.case("pendulum")
    env, dt = zoo.make_env("pendulum", "sysid")
    sid = PDP.SysID("pendulum")                      # (the zoo's own library: same label, same equations)
    sid.setAuxvarVariable(env.dyn_auxvar)
    sid.setStateVariable(env.X)
    sid.setControlVariable(env.U)
    sid.setDyn(env.X + dt * env.f)
    B, T = 2, 5
    x0, inputs, w = c["x0"][:B], c["inputs"][:B, :T], np.abs(c["g"][:B, :T + 1])
    wd, ud = torch.as_tensor(w, device="cuda"), torch.as_tensor(inputs, device="cuda")
    rows = {}
    for key in ("theta_b", "theta"):
        th0 = c[key][:B] if key == "theta_b" else c[key]
        theta = torch.tensor(th0, device="cuda", dtype=torch.float64, requires_grad=True)
        ini = torch.tensor(x0, device="cuda", dtype=torch.float64, requires_grad=True)
        state = sysid_trajectory(sid, ini, ud, theta)
        assert tuple(state.shape) == (B, T + 1, 2)
        (wd * state ** 2).sum().backward()
        xs, gt, g0 = sv.reference(c["sid"], x0, inputs, th0, np.zeros((B, T + 1, 2)))
        _, gt, g0 = sv.reference(c["sid"], x0, inputs, th0, 2.0 * w * xs)
        rows[key] = gt
        want = gt if key == "theta_b" else gt.sum(axis=0)[None]
        margins.check("sysid layer, pendulum, %s: theta.grad" % key, sv.rel_rows(npy(theta.grad).reshape(want.shape), want), TOL)
        margins.check("sysid layer, pendulum, %s: ini_state.grad" % key, sv.rel_rows(npy(ini.grad), g0), TOL)
    # without a gradient for ini_state: an array goes in, theta.grad is the same
    theta = torch.tensor(c["theta"], device="cuda", dtype=torch.float64, requires_grad=True)
    (wd * sysid_trajectory(sid, x0, inputs, theta) ** 2).sum().backward()
    margins.check("sysid layer, pendulum, ini_state an array: theta.grad", sv.rel_rows(npy(theta.grad)[None], rows["theta"].sum(axis=0)[None]), TOL)
    with pytest.raises(NotImplementedError, match="df/du"):
        sysid_trajectory(sid, x0, ud.clone().requires_grad_(True), theta)
    with pytest.raises(TypeError, match="CUDA fp64"):
        sysid_trajectory(sid, x0, inputs, theta.detach().cpu())
    with pytest.raises(ValueError, match=r"\[p\] or \[B, p\]"):
        sysid_trajectory(sid, x0, inputs, torch.ones(4, device="cuda", dtype=torch.float64))


def test_the_example_trains_from_sin_and_cos_of_the_angle():
    """examples/sysid_layer_custom_loss.py in a fresh process: exit 0, and both the loss and the parameter error end below where they started"""
    r = subprocess.run([sys.executable, os.path.join(sv.ROOT, "examples", "sysid_layer_custom_loss.py")], cwd=sv.ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    print(r.stdout)
    ini = re.search(r"^initial: loss ([0-9.eE+-]+)\s+parameter error ([0-9.eE+-]+)", r.stdout, flags=re.M)
    fin = re.search(r"^final: +loss ([0-9.eE+-]+)\s+parameter error ([0-9.eE+-]+)", r.stdout, flags=re.M)
    assert ini and fin, r.stdout[-2000:]
    assert float(fin.group(1)) < float(ini.group(1)) and float(fin.group(2)) < float(ini.group(2))
