"""GPU: the SysID rollout's Jacobian-vector product (pdp_sysid_rollout_jvp_batched, sysid_jvp_kernel), forward-mode differentiation through the autograd layer and
MatrixFreeLM on it, against the reference of tests/sysid_jvp_common.py (materialised sensitivities contracted with the direction): 1e-10 of the largest entry per
sample."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import sysid_jvp_common as sj
import sysid_vjp_common as sv

pytestmark = pytest.mark.gpu
TOL = sj.TOL
ALONE = {"d_theta": ("d_theta",), "d_x0": ("d_x0",), "d_u": ("d_u",)}


def npy(t):
    return t.detach().cpu().numpy()


def model(system):
    from pdp_amd import zoo
    return zoo.get(system, "sysid")


def zoo_sid(system):
    """a PDP.SysID on the zoo's own library: same label, same equations"""
    from pdp_amd import PDP, zoo
    env, dt = zoo.make_env(system, "sysid")
    sid = PDP.SysID(system)
    sid.setAuxvarVariable(env.dyn_auxvar)
    sid.setStateVariable(env.X)
    sid.setControlVariable(env.U)
    sid.setDyn(env.X + dt * env.f)
    return sid


def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def run(mdl, c, theta_key="theta", T=None, **tangents):
    """rollout on the GPU from the case's initial states (the first T steps), then the entry point: (states, d_x as numpy)"""
    u = c["inputs"] if T is None else c["inputs"][:, :T]
    if tangents.get("d_u") is not None and T is not None:
        tangents = dict(tangents, d_u=tangents["d_u"][:, :T])
    x = mdl.sysid_integrate(c["x0"], u, c[theta_key])
    return x, npy(mdl.sysid_rollout_jvp(x, u, c[theta_key], **tangents))


def check_directions(margins, tag, mdl, c, S, theta_key="theta", dth_key="d_theta", T=None):
    """all three tangents, and each alone, within TOL of the reference"""
    full = dict(d_theta=c[dth_key], d_x0=c["d_x0"], d_u=c["d_u"])
    for label, keys in dict(ALONE, all=("d_theta", "d_x0", "d_u")).items():
        kw = {k: full[k] for k in keys}
        x, got = run(mdl, c, theta_key, T=T, **kw)
        want = sj.tangent(S, T=T, **kw)
        assert got.shape == want.shape and np.abs(want).max(axis=(1, 2)).min() > 0
        margins.check("%s, %s: d_x" % (tag, label), sj.rel_rows(got, want), TOL)
    return x


@pytest.mark.parametrize("system", sj.SYSTEMS)
def test_stored_data_against_the_reference(margins, system):
    """the stored inputs (T = 10 or 20): theta shared and per sample, d_theta shared and per sample; all three tangents, and each alone"""
    mdl, c = model(system), sj.case(system)
    for key, S in (("theta", "S"), ("theta_b", "S_b")):
        for dkey in ("d_theta", "d_theta_b"):
            tag = "sysid jvp %s, %s, %s" % (system, key, dkey)
            x = check_directions(margins, tag, mdl, c, c[S], key, dkey)
            margins.check(tag + ": rollout", sj.rel_rows(npy(x), c[S]["states"]), TOL)


@pytest.mark.parametrize("system", sj.SYSTEMS)
def test_chunk_edges(margins, system):
    """T = 1, 31, 32, 33 and EDGE_T around the R = 32 pool rows the library reports; shorter horizons are prefixes of the longest (their sensitivities are prefixes)"""
    mdl = model(system)
    R = mdl.sysid_jvp_rows(3)
    assert R == mdl.chunk == 32
    long = sj.case(system, sj.EDGE_T[system])
    for T in sorted({1, R - 1, R, R + 1, sj.EDGE_T[system]}):
        check_directions(margins, "sysid jvp %s T = %d" % (system, T), mdl, long, long["S"], T=T)


@pytest.mark.parametrize("system", ["pendulum", "quadrotor"])
def test_exact_zeros_and_causality(margins, system):
    """zero tangents give exact zeros; a d_u that is non-zero at step s only (s = 0, R, T - 1 at T = R + 1) leaves d_x[t <= s] exactly zero and the later steps within
    TOL; a d_x0 alone gives d_x[:, 0] equal to it to the bit"""
    mdl = model(system)
    R = mdl.sysid_jvp_rows(3)
    T = R + 1
    c = sj.case(system, T)
    zt, z0, zu = np.zeros_like(c["d_theta"]), np.zeros_like(c["d_x0"]), np.zeros_like(c["d_u"])
    for kw in (dict(d_theta=zt), dict(d_x0=z0), dict(d_u=zu), dict(d_theta=zt, d_x0=z0, d_u=zu), dict(d_theta=np.zeros_like(c["d_theta_b"]), d_x0=z0)):
        _, got = run(mdl, c, **kw)
        assert got.shape[1:] == (T + 1, mdl.n) and (got == 0.0).all(), sorted(kw)
    for s in (0, R, T - 1):
        du = zu.copy()
        du[:, s] = c["d_u"][:, s]
        for extra in ({}, dict(d_theta=zt, d_x0=z0)):
            _, got = run(mdl, c, d_u=du, **extra)
            assert (got[:, :s + 1] == 0.0).all(), (system, s)
            want = sj.tangent(c["S"], d_u=du)
            assert not want[:, :s + 1].any() and np.abs(want[:, s + 1:]).max(axis=(1, 2)).min() > 0
            margins.check("sysid jvp %s T = %d, d_u at step %d only: d_x" % (system, T, s), sj.rel_rows(got, want), TOL)
    for extra in ({}, dict(d_u=c["d_u"]), dict(d_theta=c["d_theta"])):
        _, got = run(mdl, c, d_x0=c["d_x0"], **extra)
        assert same_bits(got[:, 0], c["d_x0"])
    _, got = run(mdl, c, d_theta=c["d_theta"])
    assert (got[:, 0] == 0.0).all()


def test_a_nan_stays_in_its_trajectory():
    """quadrotor, stored data.  NaN in one trajectory's d_theta row, d_x0, d_u or inputs: the trajectories 0 and 2 keep the clean run's bits; with the NaN in d_u[1, 4]
    the steps up to 4 of trajectory 1 keep them too"""
    mdl, c = model("quadrotor"), sj.case("quadrotor")
    full = dict(d_theta=c["d_theta_b"], d_x0=c["d_x0"], d_u=c["d_u"])
    _, clean = run(mdl, c, **full)
    assert np.isfinite(clean).all()
    for k, at in (("d_theta", (1, 2)), ("d_x0", (1, 3)), ("d_u", (1, 4, 0))):
        bad = full[k].copy()
        bad[at] = np.nan
        _, got = run(mdl, c, **dict(full, **{k: bad}))
        assert np.isnan(got[1]).any() and same_bits(got[0], clean[0]) and same_bits(got[2], clean[2]), k
        if k == "d_u":
            assert same_bits(got[1, :5], clean[1, :5]) and np.isnan(got[1, 5:]).any()
    u = c["inputs"].copy()
    u[1, 4, 0] = np.nan
    x = mdl.sysid_integrate(c["x0"], u, c["theta"])
    got = npy(mdl.sysid_rollout_jvp(x, u, c["theta"], **full))
    assert np.isnan(got[1]).any() and same_bits(got[0], clean[0]) and same_bits(got[2], clean[2])


@pytest.mark.parametrize("system", ["pendulum", "quadrotor"])
def test_output_bits_do_not_depend_on_the_batch(system):
    """three trajectories sent alone (B = 1) and inside B = 2 #CU + 1 and B = 4 #CU + 1, first, middle and last position: the same bits, with and without d_u (the
    zoo's rows fit 2400 doubles: where the rows change with B is test_the_row_clamp_changes_the_chunks_and_no_bit)"""
    import torch
    mdl, c = model(system), sj.case(system, sj.EDGE_T[system])
    for with_u in (True, False):
        pick = lambda idx: dict(d_theta=c["d_theta_b"][idx], d_x0=c["d_x0"][idx], **(dict(d_u=c["d_u"][idx]) if with_u else {}))
        alone = []
        for b in range(3):
            one = dict(x0=c["x0"][b:b + 1], inputs=c["inputs"][b:b + 1], theta_b=c["theta_b"][b:b + 1])
            alone.append(run(mdl, one, "theta_b", **pick(slice(b, b + 1)))[1])
        for B in (2 * cus() + 1, 4 * cus() + 1):
            pos = [0, B // 2, B - 1]
            idx = np.arange(B) % c["inputs"].shape[0]
            idx[pos] = [0, 1, 2]
            big = dict(x0=c["x0"][idx], inputs=c["inputs"][idx], theta_b=c["theta_b"][idx])
            _, out = run(mdl, big, "theta_b", **pick(idx))
            for k, b in enumerate(pos):
                assert same_bits(out[b], alone[k][0]), (with_u, B, b)
    torch.cuda.synchronize()


@pytest.mark.parametrize("system", ["pendulum", "quadrotor"])
def test_a_null_tangent_is_a_buffer_of_zeros(margins, system):
    """within one instantiation (d_u NULL in both calls, or given in both) a NULL d_theta / d_x0 and zeros give the same bits; across the two instantiations
    d_u = None against a zero d_u is held to TOL, and whether the bits agree is printed"""
    mdl, c = model(system), sj.case(system, sj.EDGE_T[system])
    zt, z0, zu = np.zeros_like(c["d_theta"]), np.zeros_like(c["d_x0"]), np.zeros_like(c["d_u"])
    for extra in ({}, dict(d_u=c["d_u"])):
        _, a = run(mdl, c, d_theta=c["d_theta"], **extra)
        _, b = run(mdl, c, d_theta=c["d_theta"], d_x0=z0, **extra)
        assert same_bits(a, b)
        _, a = run(mdl, c, d_x0=c["d_x0"], **extra)
        _, b = run(mdl, c, d_x0=c["d_x0"], d_theta=zt, **extra)
        _, b2 = run(mdl, c, d_x0=c["d_x0"], d_theta=np.zeros_like(c["d_theta_b"]), **extra)
        assert same_bits(a, b) and same_bits(a, b2)
    _, a = run(mdl, c, d_theta=c["d_theta"], d_x0=c["d_x0"])
    _, b = run(mdl, c, d_theta=c["d_theta"], d_x0=c["d_x0"], d_u=zu)
    print("sysid jvp %s: d_u = None and a zero d_u %s the same bits" % (system, "give" if same_bits(a, b) else "DO NOT give"))
    margins.check("sysid jvp %s: d_u = None against a zero d_u" % system, sj.rel_rows(b, a), TOL)


@pytest.mark.parametrize("system", sj.SYSTEMS)
def test_duality_with_the_adjoint_sweep(margins, system):
    """sum g . (J v) against (J' g) . v with the unchanged vjp kernels, for random g and v = (d_theta, d_x0, d_u): the gap the per-entry bound of both sides implies,
    1e-10 (|g|_1 max|Jv| + |v|_1 max|J'g|), per trajectory"""
    mdl, c = model(system), sj.case(system, sj.EDGE_T[system])
    x, jv = run(mdl, c, "theta_b", d_theta=c["d_theta_b"], d_x0=c["d_x0"], d_u=c["d_u"])
    out = {k: npy(v) for k, v in mdl.sysid_rollout_vjp(x, c["inputs"], c["theta_b"], c["g"], want_inputs=True).items()}
    for b in range(c["inputs"].shape[0]):
        lhs = float((c["g"][b] * jv[b]).sum())
        v = np.concatenate([c["d_theta_b"][b], c["d_x0"][b], c["d_u"][b].ravel()])
        jtg = np.concatenate([out["grad_theta"][b], out["grad_x0"][b], out["grad_u"][b].ravel()])
        allowed = np.abs(c["g"][b]).sum() * np.abs(jv[b]).max() + np.abs(v).sum() * np.abs(jtg).max()
        margins.check("sysid jvp %s sample %d: g . (J v) against (J' g) . v" % (system, b), abs(lhs - float(jtg @ v)) / allowed, TOL)


@pytest.mark.parametrize("system", ["pendulum", "quadrotor"])
def test_against_the_fused_unit_and_the_materialised_sensitivities(margins, system):
    """stored data, d_x0 = 0, no d_u: J' J d_theta from jvp + vjp against SysID.step's Gauss-Newton matrix times d_theta, and J d_theta against X @ d_theta with X
    from pdp_sysid_aux_integrate_batched"""
    from pdp_amd import runtime as rt
    mdl = model(system)
    inputs, states, _, theta = sv.stored(system)
    dth = sj.case(system)["d_theta"]
    x = mdl.sysid_integrate(states[:, 0], inputs, theta)
    jv = mdl.sysid_rollout_jvp(x, inputs, theta, d_theta=dth)
    gn = npy(mdl.sysid_step(inputs, states, theta, gauss_newton=True)["gn"])
    got = npy(mdl.sysid_rollout_vjp(x, inputs, theta, jv, want_ini=False)["grad_theta"])
    margins.check("sysid jvp + vjp %s: J' J v against the fused unit's G v" % system, sj.rel_rows(got, gn @ dth), TOL)
    F, E = mdl.sysid_auxsys(x, inputs, theta)
    X = npy(rt.sysid_aux_integrate(F, E))
    margins.check("sysid jvp %s: J v against the materialised X v" % system, sj.rel_rows(npy(jv), X @ dth), TOL)


def _guarded(mdl, c, x, T, **kw):
    """through the raw entry point into a buffer with NaN rows in front and behind: d_x, and nothing is written outside [B, T+1, n]"""
    import torch
    from pdp_amd import runtime as rt
    B = c["inputs"].shape[0]
    buf = torch.full((B + 2, T + 1, mdl.n), float("nan"), dtype=torch.float64, device="cuda")
    u, th = rt.dev(c["inputs"][:, :T]), rt.dev(c["theta"])
    t = {k: (None if kw.get(k) is None else rt.dev(kw[k][:, :T] if k == "d_u" else kw[k])) for k in ("d_theta", "d_x0", "d_u")}
    opt = lambda a: None if a is None else rt.ptr(a)
    rt.check(mdl.lib.pdp_sysid_rollout_jvp_batched(B, T, rt.ptr(x), rt.ptr(u), rt.ptr(th), 0, opt(t["d_theta"]), 0, opt(t["d_x0"]), opt(t["d_u"]), rt.ptr(buf[1:]),
                                                   rt.current_stream_ptr()), "pdp_sysid_rollout_jvp_batched")
    buf = npy(buf)
    assert np.isnan(buf[0]).all() and np.isnan(buf[B + 1]).all()
    return buf[1:B + 1]


# model -> (pool rows of a small batch, horizons)
USER = {"linear_9_2_99": (16, (1, 17)), "chain_40_10_3": (16, (1, 16, 17)), "mlp_6_2_246": (4, (1, 3, 4, 5, 9, 13)), "chain_64_4_3": (8, (1, 8, 9, 17))}


@pytest.mark.parametrize("name", sorted(USER))
def test_user_models(margins, name):
    """p = 99 (d_theta read through two 64-lane slots' worth of scalar loads), m = 10, a dense E with a pool of four rows, n = 64 (every lane owns a component): all
    three tangents and each alone at the chunk edges, against the sympy oracle; the guarded raw call has the layer's bits and writes nothing outside its tensor"""
    rows, horizons = USER[name]
    sid = sj.su.user_pair(name)[0]
    mdl = sid.model()
    assert mdl.sysid_jvp_rows(3) == rows == mdl.chunk, "the pool-row rule changed: the horizons above no longer sit at the chunk edges"
    long = sj.user_case(name, T=max(horizons))
    for T in horizons:
        tag = "sysid jvp %s T = %d" % (name, T)
        x = check_directions(margins, tag, mdl, long, long["S"], T=T)
        margins.check(tag + ": rollout", sj.rel_rows(npy(x), long["S"]["states"][:, :T + 1]), TOL)
        for kw in (dict(d_theta=long["d_theta"], d_x0=long["d_x0"], d_u=long["d_u"]), dict(d_theta=long["d_theta"])):
            assert same_bits(_guarded(mdl, long, x, T, **kw), run(mdl, long, T=T, **kw)[1]), (tag, sorted(kw))
    if name == "chain_64_4_3":
        T = max(horizons)
        for comp in (63, 0):
            d0 = np.zeros_like(long["d_x0"])
            d0[:, comp] = long["d_x0"][:, comp]
            _, got = run(mdl, long, d_x0=d0)
            margins.check("sysid jvp %s T = %d, a tangent in component %d of x_0 alone" % (name, T, comp), sj.rel_rows(got, sj.tangent(long["S"], d_x0=d0)), TOL)


def test_the_row_clamp_changes_the_chunks_and_no_bit(margins):
    """linear_9_2_99 (row stride 189): 16 pool rows up to four trajectories per CU, 12 beyond.  T = 13 is one chunk in the small batch and two in the large one, T = 25
    is 13 + 12 against 9 + 9 + 7.  Three trajectories sent alone (B = 1) and at the first, middle and last position of B = 4 #CU + 1: the same bits"""
    import torch
    name = "linear_9_2_99"
    mdl = sj.su.user_pair(name)[0].model()
    B = 4 * cus() + 1
    assert mdl.sysid_jvp_rows(1) == 16 and mdl.sysid_jvp_rows(B) == 12
    long = sj.user_case(name, T=25)
    for T in (13, 25):
        sub = lambda idx: dict(x0=long["x0"][idx], inputs=long["inputs"][idx], theta=long["theta"])
        tang = lambda idx: dict(d_theta=long["d_theta"], d_x0=long["d_x0"][idx], d_u=long["d_u"][idx])
        alone = [run(mdl, sub(slice(b, b + 1)), T=T, **tang(slice(b, b + 1)))[1] for b in range(3)]
        pos = [0, B // 2, B - 1]
        idx = np.arange(B) % 3
        idx[pos] = [0, 1, 2]
        _, out = run(mdl, sub(idx), T=T, **tang(idx))
        for k, b in enumerate(pos):
            assert same_bits(out[b], alone[k][0]), (T, b)
        margins.check("sysid jvp %s T = %d, B = %d (12 pool rows): d_x" % (name, T, B),
                      sj.rel_rows(out[pos], sj.tangent(long["S"], long["d_theta"], long["d_x0"], long["d_u"], T=T)), TOL)
    torch.cuda.synchronize()


def test_forward_mode_through_the_layer(margins):
    """torch.autograd.forward_ad through sysid_trajectory on the pendulum: dual tensors for theta ([p] and [B, p]), ini_state and - with input_grad=True - inputs give
    rollout_jvp_batch's bits; without input_grad a dual `inputs` is refused; the backward pass next to it is the one it was"""
    import torch
    import torch.autograd.forward_ad as fwAD
    from pdp_amd.autograd import sysid_trajectory
    c = sj.case("pendulum")
    sid = zoo_sid("pendulum")
    dv = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda", dtype=torch.float64)
    x0, u = dv(c["x0"]), dv(c["inputs"])
    for key, dkey in (("theta", "d_theta"), ("theta_b", "d_theta_b")):
        th, dth, dx0, du = dv(c[key]), dv(c[dkey]), dv(c["d_x0"]), dv(c["d_u"])
        x = sid.integrateDyn_batch(x0, u, th)
        with fwAD.dual_level():
            out = sysid_trajectory(sid, fwAD.make_dual(x0, dx0), fwAD.make_dual(u, du), fwAD.make_dual(th, dth), input_grad=True)
            primal, tangent = fwAD.unpack_dual(out)
            assert same_bits(npy(primal), npy(x))
            assert same_bits(npy(tangent), npy(sid.rollout_jvp_batch(x, u, th, d_auxvar=dth, d_ini_state=dx0, d_inputs=du)))
            margins.check("sysid layer forward mode, pendulum, %s: tangent" % key, sj.rel_rows(npy(tangent), sj.tangent(c["S" if key == "theta" else "S_b"], c[dkey],
                                                                                                                     c["d_x0"], c["d_u"])), TOL)
            tangent = fwAD.unpack_dual(sysid_trajectory(sid, x0, u, fwAD.make_dual(th, dth))).tangent
            assert same_bits(npy(tangent), npy(sid.rollout_jvp_batch(x, u, th, d_auxvar=dth)))
            tangent = fwAD.unpack_dual(sysid_trajectory(sid, fwAD.make_dual(x0, dx0), u, th)).tangent
            assert same_bits(npy(tangent), npy(sid.rollout_jvp_batch(x, u, th, d_ini_state=dx0)))
            with pytest.raises(NotImplementedError, match="input_grad=True"):
                sysid_trajectory(sid, x0, fwAD.make_dual(u, du), th)
        theta = th.clone().requires_grad_(True)
        g = dv(c["g"])
        (sysid_trajectory(sid, x0, u, theta) * g).sum().backward()
        want = sid.rollout_vjp_batch(x, u, th, g, want_ini=False)["grad_theta"]
        assert same_bits(npy(theta.grad), npy(want.sum(dim=0) if key == "theta" else want))


def test_matrix_free_lm_on_the_wide_linear_model():
    """MatrixFreeLM.for_sysid on linear_9_2_99 (p = 99), the problem of the host test's numpy restatement: a mean loss <= 1e-16, a strictly decreasing accepted trace,
    at most twice the evaluations and twice the CG iterations of the restatement (tests/golden/sysid_jvp_lm_budget.json)"""
    from pdp_amd.irl import MatrixFreeLM
    P = sj.lm_problem()
    with open(os.path.join(sj.ROOT, "tests", "golden", "sysid_jvp_lm_budget.json")) as f:
        budget = json.load(f)
    loop = MatrixFreeLM.for_sysid(P["sid"], P["inputs"], P["states"], P["theta0"])
    r = loop.run(max_evals=2 * budget["evaluations"], loss_tol=1e-16)
    print("loss trace %s; %d evaluations (restatement %d), %d rejected, %d CG iterations (restatement %d); |theta - truth| %.2e"
          % (" ".join("%.3e" % v for v in r["loss_trace"]), r["evaluations"], budget["evaluations"], r["rejected"], r["cg_iterations"], budget["cg_iterations"],
             np.abs(r["parameter_trace"][-1] - P["theta_true"]).max()))
    assert set(r) >= {"loss_trace", "parameter_trace", "lambda_trace", "evaluations", "rejected", "stalled", "cg_iterations"}
    assert r["loss_trace"][-1] <= 1e-16 and (np.diff(r["loss_trace"]) < 0).all()
    assert r["evaluations"] <= 2 * budget["evaluations"] and r["cg_iterations"] <= 2 * budget["cg_iterations"]
    assert r["parameter_trace"].shape == (len(r["loss_trace"]), 99) and not r["stalled"]


def test_matrix_free_lm_with_a_measurement_function(margins):
    """the pendulum seen as (sin q, cos q) of the angle alone, stored inputs: each Gauss-Newton product of the loop agrees with J' J v / B formed from the oracle's
    sensitivities and the measurement's Jacobian, to TOL; the loop's final loss is printed"""
    import torch
    from pdp_amd.irl import MatrixFreeLM
    c = sj.case("pendulum")
    sid = zoo_sid("pendulum")
    inputs, states, true_parameter, theta = sv.stored("pendulum")
    B = inputs.shape[0]
    seen = torch.as_tensor(np.stack([np.sin(states[:, :, 0]), np.cos(states[:, :, 0])], axis=2), device="cuda")
    residual = lambda s: torch.stack([torch.sin(s[:, :, 0]), torch.cos(s[:, :, 0])], dim=2) - seen
    loop = MatrixFreeLM(sid, states[:, 0], inputs, theta, residual)
    loop.start()
    S = c["S"]                                           # (sj.case's shared theta is the stored run's: the same rollouts)
    q = S["states"][:, :, 0]
    Jh = np.stack([np.cos(q), -np.sin(q)], axis=2)       # d(sin q, cos q)/dq  [B, T+1, 2]
    J = Jh[:, :, :, None] * S["X"][:, :, 0, None, :]     # [B, T+1, 2, p]
    G = np.einsum("btkp,btkq->pq", J, J) / B
    rng = np.random.default_rng(11)
    for k in range(3):
        v = rng.standard_normal(3)
        got = npy(loop.gauss_newton_product(torch.as_tensor(v, device="cuda")))
        margins.check("MatrixFreeLM pendulum (sin q, cos q): Gauss-Newton product %d" % k, sj.rel_rows(got[None], (G @ v)[None]), TOL)
    r = loop.run(max_evals=30)
    print("pendulum from (sin q, cos q): loss trace %s; %d evaluations, %d CG iterations; theta %s (true %s)"
          % (" ".join("%.3e" % v for v in r["loss_trace"]), r["evaluations"], r["cg_iterations"], r["parameter_trace"][-1], true_parameter))


def test_the_example_runs():
    """examples/sysid_gauss_newton_wide.py in a fresh process: exit 0, both problems print their traces"""
    r = subprocess.run([sys.executable, os.path.join(sj.ROOT, "examples", "sysid_gauss_newton_wide.py")], cwd=sj.ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    print(r.stdout)
    assert "linear_9_2_99" in r.stdout and "pendulum" in r.stdout and r.stdout.count("loss trace") == 2
