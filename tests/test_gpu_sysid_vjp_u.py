"""GPU: the SysID rollout's gradient with respect to the inputs (pdp_sysid_rollout_vjp_u_batched, sysid_vjp_u_kernel) and the autograd layer's input_grad=True on
it, against the reference of tests/sysid_vjp_u_common.py (G_t from sympy, propagated forward): 1e-10 of the largest entry per sample."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import sysid_vjp_common as sv
import sysid_vjp_u_common as su

pytestmark = pytest.mark.gpu
TOL = su.TOL
ALL = dict(want_inputs=True)
SUBSETS = [dict(want_inputs=True, want_ini=False), dict(want_inputs=True, want_theta=False), dict(want_inputs=True, want_ini=False, want_theta=False)]


def npy(t):
    return t.detach().cpu().numpy()


def model(system):
    from pdp_amd import zoo
    return zoo.get(system, "sysid")


def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def run(mdl, c, theta_key="theta", g=None, inputs=None, **kw):
    """rollout on the GPU from the case's initial states, then the entry point: (states, dict of numpy outputs)"""
    u = c["inputs"] if inputs is None else inputs
    x = mdl.sysid_integrate(c["x0"], u, c[theta_key])
    out = mdl.sysid_rollout_vjp(x, u, c[theta_key], c["g"] if g is None else g, **kw)
    return x, {k: npy(v) for k, v in out.items()}


def check_three(margins, tag, out, c, sfx=""):
    margins.check(tag + ": grad_u", su.rel_rows(out["grad_u"], c["grad_u" + sfx]), TOL)
    margins.check(tag + ": grad_theta", su.rel_rows(out["grad_theta"], c["grad_theta" + sfx]), TOL)
    margins.check(tag + ": grad_x0", su.rel_rows(out["grad_x0"], c["grad_x0" + sfx]), TOL)


def check_subsets(tag, mdl, c, out, theta_key="theta"):
    """grad_u has the same bits in every subset of outputs that contains it; without it the entry point is the old one to the bit; with it grad_theta and grad_x0 are
    within TOL of the old entry point's (bit-equal or not is printed)"""
    for kw in SUBSETS:
        _, part = run(mdl, c, theta_key, **kw)
        assert set(part) == {"grad_u"} | ({"grad_theta"} if kw.get("want_theta", True) else set()) | ({"grad_x0"} if kw.get("want_ini", True) else set())
        for k in part:
            assert same_bits(part[k], out[k]), (tag, kw, k)
    _, old = run(mdl, c, theta_key)
    assert set(old) == {"grad_theta", "grad_x0"}
    print("%s: grad_theta / grad_x0 with grad_u asked for %s the bits of pdp_sysid_rollout_vjp_batched" %
          (tag, "have" if same_bits(old["grad_theta"], out["grad_theta"]) and same_bits(old["grad_x0"], out["grad_x0"]) else "DO NOT have"))
    assert su.rel_rows(out["grad_theta"], old["grad_theta"]) <= TOL and su.rel_rows(out["grad_x0"], old["grad_x0"]) <= TOL


def null_grad_u_is_the_old_entry_point(mdl, c, theta_key="theta"):
    """the new entry point with grad_u = NULL against the old one: the same bits"""
    import torch
    from pdp_amd import runtime as rt
    _, old = run(mdl, c, theta_key)
    th = rt.dev(c[theta_key])
    B, T = c["inputs"].shape[:2]
    x = mdl.sysid_integrate(c["x0"], c["inputs"], c[theta_key])
    u, g = rt.dev(c["inputs"]), rt.dev(c["g"])
    gt, g0 = torch.empty((B, mdl.p), dtype=torch.float64, device="cuda"), torch.empty((B, mdl.n), dtype=torch.float64, device="cuda")
    rt.check(mdl.lib.pdp_sysid_rollout_vjp_u_batched(B, T, rt.ptr(x), rt.ptr(u), rt.ptr(th), mdl.p if th.dim() == 2 else 0, rt.ptr(g), rt.ptr(gt), rt.ptr(g0), None,
                                                     rt.current_stream_ptr()), "pdp_sysid_rollout_vjp_u_batched")
    assert same_bits(npy(gt), old["grad_theta"]) and same_bits(npy(g0), old["grad_x0"])


@pytest.mark.parametrize("system", su.SYSTEMS)
def test_stored_data_against_the_reference(margins, system):
    """the stored inputs (T = 10 or 20), shared and per-sample theta: all three gradients, and the subsets of outputs"""
    mdl, c = model(system), su.case(system)
    for key, sfx in (("theta", ""), ("theta_b", "_b")):
        x, out = run(mdl, c, key, **ALL)
        tag = "sysid vjp_u %s %s theta" % (system, "per-sample" if sfx else "shared")
        assert out["grad_u"].shape == c["inputs"].shape
        margins.check(tag + ": rollout", su.rel_rows(npy(x), c["states" + sfx]), TOL)
        check_three(margins, tag, out, c, sfx)
        check_subsets(tag, mdl, c, out, key)
        null_grad_u_is_the_old_entry_point(mdl, c, key)


@pytest.mark.parametrize("system", ["pendulum", "cartpole", "quadrotor"])
def test_chunk_edges(margins, system):
    """T = 1, R - 1, R, R + 1, 2 R + 1 around the R pool rows of the launch (the quadrotor up to R + 1 = 33); the longest horizon is the shared case, shorter ones are
    its prefixes with their own reference"""
    mdl, sid = model(system), sv.oracle(system)
    R = mdl.sysid_vjp_u_rows(3)
    assert R == mdl.chunk == 32
    long = su.case(system, su.EDGE_T[system])
    for T in [t for t in (1, R - 1, R, R + 1, 2 * R + 1) if t <= su.EDGE_T[system]]:
        if T == su.EDGE_T[system]:
            c = long
        else:
            c = dict(x0=long["x0"], inputs=long["inputs"][:, :T], theta=long["theta"], g=long["g"][:, :T + 1])
            xs, c["grad_theta"], c["grad_x0"] = sv.reference(sid, c["x0"], c["inputs"], c["theta"], c["g"])
            c["grad_u"] = su.reference_u(system, sid, xs, c["inputs"], c["theta"], c["g"])
        x, out = run(mdl, c, **ALL)
        check_three(margins, "sysid vjp_u %s T = %d" % (system, T), out, c)
        if T == 1:                                       # grad_u[0] = G_0' g_1 from sympy's G directly
            G = su.g_fn(system)
            for b in range(len(c["x0"])):
                want = G(npy(x)[b, 0], c["inputs"][b, 0], c["theta"]).T @ c["g"][b, 1]
                margins.check("sysid vjp_u %s T = 1 sample %d: G_0' g_1" % (system, b), su.rel_rows(out["grad_u"][b], want[None]), TOL)


@pytest.mark.parametrize("system", ["pendulum", "quadrotor"])
def test_causality_and_exact_zeros(margins, system):
    """a zero cotangent gives exact zeros; a cotangent at step s only (s = 0, R, T at T = R + 1) leaves grad_u[:, t >= s] exactly zero - a result stored at the wrong
    step, or a staging row read across the chunk boundary, shows here - and the earlier steps within TOL"""
    mdl = model(system)
    R = mdl.sysid_vjp_u_rows(3)
    c = su.case(system, R + 1)
    T = R + 1
    z = np.zeros_like(c["g"])
    _, out = run(mdl, c, g=z, **ALL)
    assert not out["grad_u"].any() and not out["grad_theta"].any() and not out["grad_x0"].any()
    for s in (0, R, T):
        g = z.copy()
        g[:, s] = c["g"][:, s]
        _, out = run(mdl, c, g=g, **ALL)
        assert not out["grad_u"][:, s:].any(), (system, s)
        if s > 0:
            want = su.reference_u(system, c["sid"], c["states"], c["inputs"], c["theta"], g)
            assert not want[:, s:].any() and np.abs(want[:, :s]).max(axis=(1, 2)).min() > 0
            margins.check("sysid vjp_u %s T = %d, cotangent at step %d only: grad_u" % (system, T, s), su.rel_rows(out["grad_u"], want), TOL)


@pytest.mark.parametrize("system", ["pendulum", "quadrotor"])
def test_output_bits_do_not_depend_on_the_batch(system):
    """three trajectories sent alone (B = 1) and inside B = 2 #CU + 1 and B = 4 #CU + 1 (where the host sizes the pool anew), first, middle and last position: the
    same bits in all three outputs"""
    import torch
    mdl, c = model(system), su.case(system)
    alone = []
    for b in range(3):
        one = dict(x0=c["x0"][b:b + 1], inputs=c["inputs"][b:b + 1], theta_b=c["theta_b"][b:b + 1], g=c["g"][b:b + 1])
        alone.append(run(mdl, one, "theta_b", **ALL)[1])
    for B in (2 * cus() + 1, 4 * cus() + 1):
        pos = [0, B // 2, B - 1]
        idx = np.arange(B) % c["inputs"].shape[0]
        idx[pos] = [0, 1, 2]
        big = dict(x0=c["x0"][idx], inputs=c["inputs"][idx], theta_b=c["theta_b"][idx], g=c["g"][idx])
        _, out = run(mdl, big, "theta_b", **ALL)
        for k, b in enumerate(pos):
            for name in ("grad_u", "grad_theta", "grad_x0"):
                assert same_bits(out[name][b], alone[k][name][0]), (B, b, name)
    torch.cuda.synchronize()


def test_a_nan_stays_in_its_trajectory_and_behind_its_step():
    """quadrotor, stored data.  NaN in g[1, 4, 2]: lam_t is NaN for t <= 4, so grad_u[1, t <= 3] is NaN and nothing else is: grad_u[1, t >= 4] and the trajectories 0 and
    2 have the clean run's bits.  NaN in inputs[1, 4, 0]: the trajectories 0 and 2 unchanged to the bit"""
    mdl, c = model("quadrotor"), su.case("quadrotor")
    _, clean = run(mdl, c, **ALL)
    assert np.isfinite(clean["grad_u"]).all()
    g = c["g"].copy()
    g[1, 4, 2] = np.nan
    _, out = run(mdl, c, g=g, **ALL)
    assert np.isnan(out["grad_u"][1, :4]).all() and same_bits(out["grad_u"][1, 4:], clean["grad_u"][1, 4:])
    for b in (0, 2):
        assert all(same_bits(out[k][b], clean[k][b]) for k in ("grad_u", "grad_theta", "grad_x0"))
    u = c["inputs"].copy()
    u[1, 4, 0] = np.nan
    _, out = run(mdl, c, inputs=u, **ALL)
    assert np.isnan(out["grad_u"][1]).any()
    for b in (0, 2):
        assert all(same_bits(out[k][b], clean[k][b]) for k in ("grad_u", "grad_theta", "grad_x0"))


# model -> (pool rows of a small batch, horizons): where the G columns sit among the lanes' columns c = lane + 64 q of [E | G]
COLUMNS = {"linear_8_1_64": (16, (1, 17)),                   # p = 64: the G column is lane 0 of a slot of its own
           "linear_8_1_65": (16, (1, 17)),                   # p = 65: lane 1 of slot 1, beside one parameter
           "linear_8_2_63": (32, (1, 32, 33)),               # p = 63: lane 63 of slot 0 and lane 0 of slot 1
           "linear_9_2_99": (16, (1, 17)),                   # p = 99: lanes 35 and 36 of the second slot
           "chain_40_10_3": (16, (1, 17)),                   # m = 10
           "chain_64_4_3": (8, (1, 8, 9, 17)),               # n = 64: every lane owns a costate
           "mlp_6_2_246": (4, (1, 3, 4, 5, 9, 13))}          # p = 246: lanes 54 and 55 of the last slot; a pool of four rows


@pytest.mark.parametrize("name", sorted(COLUMNS))
def test_column_mapping_of_user_models(margins, name):
    """through the class surface against the sympy oracle; the horizons are prefixes of the longest with their own reference"""
    rows, horizons = COLUMNS[name]
    sid = su.user_pair(name)[0]
    mdl = sid.model()
    assert mdl.sysid_vjp_u_rows(3) == rows == mdl.chunk, "the pool-row rule changed: the horizons above no longer sit at the chunk edges"
    long = su.user_case(name, T=max(horizons))
    for T in horizons:
        c = su.prefix(long, T)
        x = sid.integrateDyn_batch(c["x0"], c["inputs"], c["theta"])
        out = {k: npy(v) for k, v in sid.rollout_vjp_batch(x, c["inputs"], c["theta"], c["g"], want_inputs=True).items()}
        assert out["grad_u"].shape == (3, T, mdl.m)
        tag = "sysid vjp_u %s T = %d" % (name, T)
        margins.check(tag + ": rollout", su.rel_rows(npy(x), c["states"]), TOL)
        check_three(margins, tag, out, c)
        only = npy(sid.rollout_vjp_batch(x, c["inputs"], c["theta"], c["g"], want_ini=False, want_theta=False, want_inputs=True)["grad_u"])
        assert same_bits(only, out["grad_u"]), tag
        if T == 1:
            G = su.g_fn(name)
            for b in range(3):
                want = G(npy(x)[b, 0], c["inputs"][b, 0], c["theta"]).T @ c["g"][b, 1]
                margins.check("%s sample %d: G_0' g_1" % (tag, b), su.rel_rows(out["grad_u"][b], want[None]), TOL)


def test_the_layer_on_the_pendulum(margins):
    """B = 2, T = 5, input_grad=True, L = sum w . state^2 + 0.1 sum inputs^2: inputs.grad is the reference through the dynamics plus 0.2 inputs, theta.grad and
    ini_state.grad are those of tests/test_gpu_sysid_vjp.py; a theta that requires no gradient gets none and leaves inputs.grad's bits"""
    import torch
    from pdp_amd import PDP, zoo
    from pdp_amd.autograd import sysid_trajectory
    c = su.case("pendulum")
    env, dt = zoo.make_env("pendulum", "sysid")
    sid = PDP.SysID("pendulum")                      # (the zoo's own library: same label, same equations)
    sid.setAuxvarVariable(env.dyn_auxvar)
    sid.setStateVariable(env.X)
    sid.setControlVariable(env.U)
    sid.setDyn(env.X + dt * env.f)
    B, T = 2, 5
    x0, inputs, w = c["x0"][:B], c["inputs"][:B, :T], np.abs(c["g"][:B, :T + 1])
    wd = torch.as_tensor(w, device="cuda")
    grads = {}
    for key in ("theta_b", "theta"):
        th0 = c[key][:B] if key == "theta_b" else c[key]
        theta = torch.tensor(th0, device="cuda", dtype=torch.float64, requires_grad=True)
        ini = torch.tensor(x0, device="cuda", dtype=torch.float64, requires_grad=True)
        ud = torch.tensor(inputs, device="cuda", dtype=torch.float64, requires_grad=True)
        state = sysid_trajectory(sid, ini, ud, theta, input_grad=True)
        assert tuple(state.shape) == (B, T + 1, 2)
        ((wd * state ** 2).sum() + 0.1 * (ud ** 2).sum()).backward()
        xs, _, _ = sv.reference(c["sid"], x0, inputs, th0, np.zeros((B, T + 1, 2)))
        _, gt, g0 = sv.reference(c["sid"], x0, inputs, th0, 2.0 * w * xs)
        gu = su.reference_u("pendulum", c["sid"], xs, inputs, th0, 2.0 * w * xs) + 0.2 * inputs
        want = gt if key == "theta_b" else gt.sum(axis=0)[None]
        margins.check("sysid layer with input_grad, pendulum, %s: inputs.grad" % key, su.rel_rows(npy(ud.grad), gu), TOL)
        margins.check("sysid layer with input_grad, pendulum, %s: theta.grad" % key, su.rel_rows(npy(theta.grad).reshape(want.shape), want), TOL)
        margins.check("sysid layer with input_grad, pendulum, %s: ini_state.grad" % key, su.rel_rows(npy(ini.grad), g0), TOL)
        grads[key] = npy(ud.grad)
    theta = torch.tensor(c["theta"], device="cuda", dtype=torch.float64)
    ud = torch.tensor(inputs, device="cuda", dtype=torch.float64, requires_grad=True)
    ((wd * sysid_trajectory(sid, x0, ud, theta, input_grad=True) ** 2).sum() + 0.1 * (ud ** 2).sum()).backward()
    assert theta.grad is None and same_bits(npy(ud.grad), grads["theta"])
    with pytest.raises(NotImplementedError, match="df/du"):
        sysid_trajectory(sid, x0, ud, theta)
    with pytest.raises(TypeError, match="CUDA fp64"):
        sysid_trajectory(sid, x0, inputs, theta, input_grad=True)
    with pytest.raises(TypeError, match="CUDA fp64"):
        sysid_trajectory(sid, x0, ud.detach().float(), theta, input_grad=True)


def test_the_example_plans_inputs_through_the_model():
    """examples/sysid_layer_plan_inputs.py in a fresh process: exit 0, and the loss ends below where it started"""
    r = subprocess.run([sys.executable, os.path.join(su.ROOT, "examples", "sysid_layer_plan_inputs.py")], cwd=su.ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    print(r.stdout)
    ini = re.search(r"^initial: loss ([0-9.eE+-]+)", r.stdout, flags=re.M)
    fin = re.search(r"^final: +loss ([0-9.eE+-]+)", r.stdout, flags=re.M)
    assert ini and fin, r.stdout[-2000:]
    assert float(fin.group(1)) < float(ini.group(1))
