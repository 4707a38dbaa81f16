"""CPU (no GPU needed): pdp_sysid_rollout_jvp_batched - the SysID rollout's Jacobian-vector product - at the ABI (the table, the argument errors before any launch,
the pool rows), at the Python layers against a recorder library, the kernel resources of the zoo libraries, the reference of tests/sysid_jvp_common.py against the
tangent recursion in numpy and against central differences of the oracle's rollout, and MatrixFreeLM's schedule restated in numpy.  Bounds: those of the vjp pair
(tests/test_sysid_vjp_host.py) - 1e-13 numpy against numpy, 1e-6 for central differences with h = 1e-6."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import sysid_jvp_common as sj
import sysid_vjp_common as sv
import sysid_vjp_u_common as su

NAME, ROWS = "pdp_sysid_rollout_jvp_batched", "pdp_sysid_rollout_jvp_rows"
BUDGET = os.path.join(sj.ROOT, "tests", "golden", "sysid_jvp_lm_budget.json")


def _built():
    import __graft_entry__ as g
    g.build()
    from pdp_amd import codegen, runtime as rt, zoo
    return codegen, rt, zoo


def _worst_against_sweep(name, orc, c, S, theta, T):
    worst = 0.0
    for b in range(c["inputs"].shape[0]):
        for kw in (dict(d_theta=c["d_theta"], d_x0=c["d_x0"][b], d_u=c["d_u"][b]), dict(d_theta=c["d_theta"]), dict(d_x0=c["d_x0"][b]), dict(d_u=c["d_u"][b])):
            got = sj.tangent_sweep(name, orc, S["states"][b], c["inputs"][b], theta, **kw)
            batch = {k: (v if k == "d_theta" else np.repeat(v[None], c["inputs"].shape[0], axis=0)) for k, v in kw.items()}
            want = sj.tangent(S, **batch)[b]
            worst = max(worst, np.abs(got - want).max() / np.abs(got).max())
    return worst


@pytest.mark.parametrize("system", sj.SYSTEMS)
def test_reference_agrees_with_the_tangent_recursion_in_numpy(system):
    """materialised sensitivities contracted with the direction against the forward sweep of one tangent vector, both in numpy, at the chunk-edge horizons (65 / 33),
    all three tangents and each alone: 1e-13 of the largest entry per sample, the bound of the vjp pair"""
    c = sj.case(system, sj.EDGE_T[system])
    worst = _worst_against_sweep(system, c["sid"], c, c["S"], c["theta"], sj.EDGE_T[system])
    print("%s T = %d: sensitivities . direction vs tangent sweep %.2e" % (system, sj.EDGE_T[system], worst))
    assert worst <= 1e-13


@pytest.mark.parametrize("name", ["linear_9_2_99", "chain_40_10_3"])
def test_user_model_reference_agrees_with_the_tangent_recursion_in_numpy(name):
    c = sj.user_case(name, T=17)
    worst = _worst_against_sweep(name, c["orc"], c, c["S"], c["theta"], 17)
    print("%s T = 17: sensitivities . direction vs tangent sweep %.2e" % (name, worst))
    assert worst <= 1e-13


@pytest.mark.parametrize("system", sj.SYSTEMS)
def test_reference_agrees_with_central_differences_of_the_oracle_rollout(system):
    """(x(z + h v) - x(z - h v)) / 2 h along the direction v = (d_theta, d_x0, d_u), sample 0 at the chunk-edge horizon, h = 1e-6: within 1e-6 of the largest entry"""
    c = sj.case(system, sj.EDGE_T[system])
    sid, b, h = c["sid"], 0, 1e-6
    roll = lambda s: np.asarray(sid.integrateDyn(c["x0"][b] + s * c["d_x0"][b], c["inputs"][b] + s * c["d_u"][b], c["theta"] + s * c["d_theta"]), float)
    fd = (roll(h) - roll(-h)) / (2 * h)
    want = sj.tangent(c["S"], c["d_theta"], c["d_x0"], c["d_u"])[b]
    worst = np.abs(fd - want).max() / np.abs(want).max()
    print("%s T = %d: central differences vs the reference: d_x %.2e" % (system, sj.EDGE_T[system], worst))
    assert worst <= 1e-6


def test_the_entry_points_are_listed_with_their_arguments():
    from pdp_amd import abi
    table = abi.entry_points("pdp_hip_sysid_jvp.h", "model")
    assert list(table) == [NAME, ROWS]
    assert table[NAME][0] is C.c_int and len(table[NAME][1]) == 12 and table[ROWS] == (C.c_int, [C.c_int])
    assert not abi.entry_points("pdp_hip_sysid_jvp.h", "core")
    assert len(abi.entry_points()) == 45 and len(abi.entry_points("pdp_hip.h")) == 33


def test_argument_errors_are_returned_before_any_launch():
    """valid (host) pointers everywhere, so that only the argument under test can be what is refused; nothing that passes the checks is called: no GPU here"""
    codegen, rt, zoo = _built()
    mdl = rt.load_model(codegen.build_problem(zoo.make_problem("quadrotor", "sysid"))[0])
    assert (mdl.p, mdl.m) == (5, 4)
    keep = [(C.c_double * 8)() for _ in range(7)]
    x, u, th, dth, dx0, du, dx = (C.cast(k, C.c_void_p) for k in keep)
    fn = getattr(mdl.lib, NAME)
    ok = dict(B=1, T=4, x=x, u=u, th=th, tb=0, dth=dth, dtb=0, dx0=dx0, du=du, dx=dx)

    def call(lib_fn=fn, **kw):
        a = dict(ok, **kw)
        return lib_fn(a["B"], a["T"], a["x"], a["u"], a["th"], a["tb"], a["dth"], a["dtb"], a["dx0"], a["du"], a["dx"], None)
    for kw in (dict(dth=None, dx0=None, du=None), dict(B=0), dict(B=-3), dict(T=0), dict(T=-2), dict(tb=4), dict(tb=1), dict(tb=-5), dict(dtb=4), dict(dtb=1),
               dict(dtb=-5), dict(x=None), dict(u=None), dict(th=None), dict(dx=None), dict(B=0, du=None), dict(x=None, dth=None, dx0=None), dict(tb=3, du=None)):
        assert call(**kw) == -1, kw                                               # PDP_E_ARG
    assert all(v == 0.0 for k in keep for v in k)
    for mode in ("irl", "oc"):                                                    # an OC and a CP library
        other = rt.load_model(codegen.build_problem(zoo.make_problem("cartpole", mode))[0])
        f = getattr(other.lib, NAME)
        assert call(f, tb=0, dtb=0) == -4 and call(f, du=None) == -4 and call(f, dth=None, dx0=None) == -4       # PDP_E_MODE
        assert call(f, B=0) == -1 and call(f, dth=None, dx0=None, du=None) == -1                                  # the argument check comes first
        assert getattr(other.lib, ROWS)(1) == -4 and getattr(other.lib, ROWS)(0) == -1


def test_a_66_state_model_is_refused_before_any_launch():
    """PDP_E_SIZE from chain_66 (n = 66) with valid host pointers, with and without d_u; PDP_E_ARG comes first; no buffer is touched, nothing is instantiated"""
    codegen, rt, _ = _built()
    lib, _ = codegen.build_problem(sv.size_problem("chain_66")[0])
    mdl = rt.load_model(lib)
    keep = [(C.c_double * (5 * 66))() for _ in range(7)]
    for k in keep:
        k[:] = [1.5] * len(k)
    x, u, th, dth, dx0, du, dx = (C.cast(k, C.c_void_p) for k in keep)
    fn = getattr(mdl.lib, NAME)
    assert fn(1, 4, x, u, th, 0, dth, 0, dx0, du, dx, None) == -2 and fn(1, 4, x, u, th, 0, dth, 0, None, None, dx, None) == -2        # PDP_E_SIZE
    assert fn(0, 4, x, u, th, 0, dth, 0, dx0, du, dx, None) == -1 and fn(1, 4, x, u, th, 0, None, 0, None, None, dx, None) == -1       # PDP_E_ARG first
    assert getattr(mdl.lib, ROWS)(1) == -2
    assert not [k for k in codegen.kernel_resources(lib) if k.startswith("sysid_jvp_kernel")]
    assert all(v == 1.5 for k in keep for v in k)


def test_pool_rows_of_the_zoo_models():
    """the row rule of pdp_sysid_rollout_vjp_batched on the same row (256 compute units assumed without a device)"""
    codegen, rt, zoo = _built()
    for system in sj.SYSTEMS:
        lib, info = codegen.build_problem(zoo.make_problem(system, "sysid"))
        mdl = rt.load_model(lib)
        for B in (1, 3, 1024, 1025, 5000):
            assert mdl.sysid_jvp_rows(B) == mdl.sysid_vjp_rows(B, 256), (system, B)
        assert mdl.sysid_jvp_rows(1) == mdl.chunk == info["chunk"]
        with pytest.raises(RuntimeError, match="PDP_E_ARG"):
            mdl.sysid_jvp_rows(0)


def test_zoo_kernels_do_not_spill_and_use_no_scratch():
    """the two instantiations (without / with d_u) of sysid_jvp_kernel in the five zoo libraries"""
    codegen, _, zoo = _built()
    for system in sj.SYSTEMS:
        lib, _ = codegen.build_problem(zoo.make_problem(system, "sysid"))
        k = codegen.kernel_resources(lib)
        assert {"sysid_jvp_kernel<0>", "sysid_jvp_kernel<1>"} <= set(k), sorted(k)
        for key in ("sysid_jvp_kernel<0>", "sysid_jvp_kernel<1>"):
            r = k[key]
            print("%s: %s vgpr %d sgpr %d spill %d scratch %d" % (system, key, r["vgpr"], r["sgpr"], r["spill"], r["scratch"]))
            assert r["spill"] == 0 and r["scratch"] == 0, (system, key, r)


@pytest.mark.parametrize("name", ["linear_9_2_99", "chain_40_10_3", "mlp_6_2_246", "chain_64_4_3"])
def test_kernel_resources_of_the_user_models(name):
    """printed, not bounded: near the limits the instantiations may spill as their vjp twins do (DESIGN section 4.1l records the figures)"""
    codegen, rt, _ = _built()
    lib, info = codegen.build_problem(su.size_problem(name)[0])
    k = codegen.kernel_resources(lib)
    assert rt.load_model(lib).sysid_jvp_rows(3) == info["chunk"]
    for key in ("sysid_jvp_kernel<0>", "sysid_jvp_kernel<1>", "sysid_vjp_kernel", "sysid_vjp_u_kernel"):
        r = k[key]
        print("%s: %s vgpr %d sgpr %d spill %d scratch %d B" % (name, key, r["vgpr"], r["sgpr"], r["spill"], r["scratch"]))


def _stand_ins(monkeypatch):
    import ls_rows_common as lr
    from pdp_amd import PDP, runtime
    lr.stand_in_torch(monkeypatch)
    monkeypatch.setattr(runtime, "ptr", lambda t: ("ptr", tuple(t.shape)))
    mdl = runtime.ModelLib.__new__(runtime.ModelLib)
    mdl.n, mdl.m, mdl.p, mdl.chunk, mdl.nnz_path, mdl.lib = 4, 1, 3, 32, 10, lr.Recorder()
    sid = PDP.SysID.__new__(PDP.SysID)
    sid.n_state, sid.n_control, sid.n_auxvar, sid._model = 4, 1, 3, mdl
    return mdl, sid


def test_the_layers_against_a_recorder_library(monkeypatch):
    """no GPU: the library records.  Shape errors are ValueErrors before any call; a None tangent is a NULL pointer; the stride of d_theta follows its shape"""
    mdl, sid = _stand_ins(monkeypatch)
    B, T = 3, 6
    x, u, th = np.zeros((B, T + 1, 4)), np.zeros((B, T, 1)), np.ones(3)
    good = dict(state_traj=x, inputs=u, auxvar_value=th, d_auxvar=np.ones(3), d_ini_state=np.ones((B, 4)), d_inputs=np.ones((B, T, 1)))
    bad = [dict(state_traj=x[:, :-1]), dict(state_traj=x[:2]), dict(inputs=u[0]), dict(inputs=np.zeros((B, T, 2))), dict(inputs=np.zeros((B, 0, 1))),
           dict(auxvar_value=np.ones(4)), dict(auxvar_value=np.ones((2, 3))), dict(d_auxvar=np.ones(4)), dict(d_auxvar=np.ones((2, 3))),
           dict(d_ini_state=np.ones((B, 3))), dict(d_ini_state=np.ones(4)), dict(d_inputs=np.ones((B, T + 1, 1))), dict(d_inputs=np.ones((B, T))),
           dict(d_auxvar=None, d_ini_state=None, d_inputs=None)]
    for kw in bad:
        with pytest.raises(ValueError, match="sysid_rollout_jvp"):
            sid.rollout_jvp_batch(**dict(good, **kw))
    with pytest.raises(ValueError, match="nothing to compute"):
        mdl.sysid_rollout_jvp(x, u, th)
    assert mdl.lib.calls == []
    P = lambda *shape: ("ptr", shape)
    head = (B, T, P(B, T + 1, 4), P(B, T, 1), P(3), 0)
    out = sid.rollout_jvp_batch(**good)
    assert tuple(out.shape) == (B, T + 1, 4)
    sid.rollout_jvp_batch(x, u, th, d_auxvar=np.ones((B, 3)))
    mdl.sysid_rollout_jvp(x, u, np.ones((B, 3)), d_x0=np.ones((B, 4)))
    mdl.sysid_rollout_jvp(x, u, th, d_u=np.ones((B, T, 1)))
    assert mdl.lib.calls == [(NAME, head + (P(3), 0, P(B, 4), P(B, T, 1), P(B, T + 1, 4), None)),
                             (NAME, head + (P(B, 3), 3, None, None, P(B, T + 1, 4), None)),
                             (NAME, (B, T, P(B, T + 1, 4), P(B, T, 1), P(B, 3), 3, None, 0, P(B, 4), None, P(B, T + 1, 4), None)),
                             (NAME, head + (None, 0, None, P(B, T, 1), P(B, T + 1, 4), None))]


def test_matrix_free_lm_refuses_bad_shapes_before_any_launch():
    from pdp_amd import irl

    class Sid:
        n_state, n_control, n_auxvar = 4, 1, 3
    f = lambda s: s
    for kw in (dict(inputs=np.zeros((2, 5))), dict(inputs=np.zeros((2, 5, 2))), dict(ini_state=np.zeros((3, 4))), dict(theta0=np.zeros(4)), dict(residual=None)):
        a = dict(dict(ini_state=np.zeros((2, 4)), inputs=np.zeros((2, 5, 1)), theta0=np.zeros(3), residual=f), **kw)
        with pytest.raises(ValueError, match="MatrixFreeLM"):
            irl.MatrixFreeLM(Sid(), a["ini_state"], a["inputs"], a["theta0"], a["residual"])
    with pytest.raises(ValueError, match="MatrixFreeLM.for_sysid"):
        irl.MatrixFreeLM.for_sysid(Sid(), np.zeros((2, 5, 1)), np.zeros((2, 5, 4)), np.zeros(3))
    assert "Marquardt's scaling" in irl.MatrixFreeLM.__doc__


def test_matrix_free_lm_restated_in_numpy_reaches_the_floor():
    """MatrixFreeLM's schedule on the oracle of linear_9_2_99 (B = 16, T = 20, noise-free, start 0.1 N(0,1) from the truth): a mean loss <= 1e-16 within 30
    evaluations, a strictly decreasing trace; its counts are the budget the GPU loop is held to (twice of each), recorded in tests/golden/sysid_jvp_lm_budget.json"""
    r = sj.lm_restatement(sj.lm_problem())
    print("loss trace %s; %d evaluations, %d rejected, %d CG iterations" % (" ".join("%.3e" % v for v in r["loss_trace"]), r["evaluations"], r["rejected"],
                                                                            r["cg_iterations"]))
    assert r["loss_trace"][-1] <= 1e-16 and r["evaluations"] <= 30
    assert (np.diff(r["loss_trace"]) < 0).all()
    with open(BUDGET) as f:
        budget = json.load(f)
    # the recorded counts are this restatement's: the evaluations exactly; the CG count within a tenth (the iteration at which a residual crosses 1e-8 of its start
    # moves by a few with the summation order of the BLAS underneath numpy)
    assert budget["evaluations"] == r["evaluations"] and abs(budget["cg_iterations"] - r["cg_iterations"]) <= 0.1 * budget["cg_iterations"], (budget, r)
