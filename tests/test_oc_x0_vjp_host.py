"""CPU (no GPU needed): the initial-state gradient of the OC unit - the grown struct pdp_oc_sens_out (grad_x0, last) in abi.py and in the header, the argument
refusals of the runtime and the class surface before any foreign call, the calls without want_ini as they were, the rows rule restated in ModelLib.oc_x0_vjp_rows,
and the mathematics: the adjoint sweep (oc_x0_vjp_common.adjoint_sweep, the kernel's recursion) against the reference's forward sensitivities on every case the GPU
tests use, and the reference against central differences through re-solving."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)


def test_the_struct_grew_by_one_last_field_and_no_entry_point_was_added():
    from pdp_amd import abi
    assert abi.PdpOcSensOut._fields_[-1][0] == "grad_x0" and len(abi.PdpOcSensOut._fields_) == 5
    so = abi.PdpOcSensOut(1, 2, 3, 4)                               # four positional values still construct it: the new field is NULL
    assert (so.dxdp, so.dudp, so.riccati, so.predict_record, so.grad_x0) == (1, 2, 3, 4, None)
    assert abi.PdpOcSensOut(None, None, None, None, 5).grad_x0 == 5
    assert C.sizeof(abi.PdpOcSensOut) == 5 * C.sizeof(C.c_void_p)
    assert len(abi.entry_points()) == 45


def test_the_headers_struct_has_the_field_last():
    src = open(os.path.join(ROOT, "include", "pdp_hip.h")).read()
    body = re.search(r"typedef struct pdp_oc_sens_out \{(.*?)\} pdp_oc_sens_out;", src, flags=re.S).group(1)
    fields = re.findall(r"(double|float)\s*\*\s*(\w+)\s*;", body)
    assert fields == [("double", "dxdp"), ("double", "dudp"), ("double", "riccati"), ("float", "predict_record"), ("double", "grad_x0")]
    assert "rebuil" in open(os.path.join(ROOT, "INTEGRATION.md")).read().split("`double* grad_x0`", 1)[1][:1500]       # C callers are told to rebuild against the grown struct


class _NoForeignCalls:
    def __getattr__(self, name):
        raise AssertionError("foreign call %s before the arguments were validated" % name)


def test_refused_combinations_are_value_errors_before_any_foreign_call():
    from pdp_amd import PDP, runtime
    mdl = runtime.ModelLib.__new__(runtime.ModelLib)
    mdl.n, mdl.m, mdl.p, mdl.lib = 4, 1, 7, _NoForeignCalls()
    B, T = 3, 6
    u, th, x0, dx, du = np.zeros((B, T, 1)), np.ones(7), np.zeros((B, 4)), np.zeros((B, T + 1, 4)), np.zeros((B, T, 1))
    refused = (dict(gauss_newton=True), dict(skip_missing=True), dict(gauss_newton=True, skip_missing=True), dict(weights_x=np.ones(4)), dict(weights_u=np.ones(1)),
               dict(huber_delta=1.0))
    for kw in refused:
        with pytest.raises(ValueError, match="want_ini"):
            mdl.oc_pdp_grad(u, th, dx, du, x0=x0, want_ini=True, **kw)
    oc = PDP.OCSys.__new__(PDP.OCSys)
    for kw in (dict(want_gauss_newton=True), dict(skip_missing=True), dict(weights_state=np.ones(4)), dict(weights_control=np.ones(1)), dict(huber_delta=1.0)):
        with pytest.raises(ValueError, match="want_ini"):
            oc.pdp_grad_batch(u, th, dx, du, ini_state=x0, want_ini=True, **kw)
    # the cotangent call judges its shapes first, with want_ini as without
    with pytest.raises(ValueError, match="cotangents"):
        mdl.oc_pdp_vjp(u, th, np.zeros((B, T, 4)), du, x0=x0, want_ini=True)
    with pytest.raises(ValueError, match="x0"):
        mdl.oc_pdp_vjp(u, th, dx, du, want_ini=True)


OC_LAYOUT = {"pdp_oc_pdp_grad_batched": "B T flags x0 u theta tb demo_x demo_u x lam loss grad dxdp dudp status ws nbytes stream",
             "pdp_oc_pdp_grad_sens_batched": "B T flags x0 u theta tb demo_x demo_u x lam loss grad sens status ws nbytes stream"}
SCALARS = ("B", "T", "flags", "tb", "nbytes")


def _recorded(monkeypatch, method, **kw):
    """the foreign calls of one ModelLib method on the stand-ins of ls_rows_common: [(name, scalar arguments, names of the NULL pointers, NULL fields of sens)]"""
    import ls_rows_common as lr
    lr.stand_in_torch(monkeypatch)
    mdl = lr.stand_in_model(4, 1, 7)
    B, T = 3, 6
    u, th, x0, dx, du = np.zeros((B, T, 1)), np.ones(7), np.zeros((B, 4)), np.zeros((B, T + 1, 4)), np.zeros((B, T, 1))
    out = getattr(mdl, method)(u, th, dx, du, x0=x0, **kw)
    calls = []
    for name, args in mdl.lib.calls:
        if name not in OC_LAYOUT:                                # (size queries)
            continue
        names = OC_LAYOUT[name].split()
        assert len(args) == len(names), (name, len(args))
        a = dict(zip(names, args))
        sens = a.pop("sens", None)
        null = {k for k, v in a.items() if k not in SCALARS and getattr(v, "value", v) is None}
        so = None if sens is None else tuple(k for k, _ in sens._obj._fields_ if getattr(sens._obj, k) is None)
        calls.append((name, {k: a[k] for k in SCALARS}, null, so))
    return calls, out


def test_without_want_ini_the_foreign_calls_are_todays_and_with_it_the_sens_entry_point_carries_the_field(monkeypatch):
    B, T = 3, 6
    scal = lambda flags: dict(B=B, T=T, flags=flags, tb=0, nbytes=0)
    # the cotangent call: pdp_oc_pdp_grad_batched with PDP_OC_COTANGENT, no loss and no sensitivity pointers - as before the field existed
    calls, out = _recorded(monkeypatch, "oc_pdp_vjp")
    assert calls == [("pdp_oc_pdp_grad_batched", scal(8), {"loss", "dxdp", "dudp", "stream"}, None)]
    assert sorted(out) == ["grad", "lam", "status", "x"]
    calls, out = _recorded(monkeypatch, "oc_pdp_vjp", want_ini=False)
    assert calls == [("pdp_oc_pdp_grad_batched", scal(8), {"loss", "dxdp", "dudp", "stream"}, None)]
    calls, out = _recorded(monkeypatch, "oc_pdp_vjp", want_ini=True)
    assert calls == [("pdp_oc_pdp_grad_sens_batched", scal(8), {"loss", "stream"}, ("dxdp", "dudp", "riccati", "predict_record"))]
    assert sorted(out) == ["grad", "grad_x0", "lam", "status", "x"] and tuple(out["grad_x0"].shape) == (B, 4)
    # the default unit
    calls, out = _recorded(monkeypatch, "oc_pdp_grad")
    assert calls == [("pdp_oc_pdp_grad_batched", scal(0), {"dxdp", "dudp", "stream"}, None)]
    assert sorted(out) == ["grad", "lam", "loss", "status", "x"]
    calls, out = _recorded(monkeypatch, "oc_pdp_grad", want_ini=True, packed=True)
    assert calls == [("pdp_oc_pdp_grad_sens_batched", scal(2), {"stream"}, ("dxdp", "dudp", "riccati", "predict_record"))]
    assert tuple(out["grad_x0"].shape) == (B, 4) and tuple(out["packed"].shape) == (B, 8)
    calls, out = _recorded(monkeypatch, "oc_pdp_grad", want_ini=True, want_sens=True)
    assert calls == [("pdp_oc_pdp_grad_sens_batched", scal(0), {"stream"}, ("riccati", "predict_record"))]


def test_rows_rule_of_the_five_zoo_models():
    import oc_x0_vjp_common as cx
    from pdp_amd import codegen, runtime, zoo
    for system in cx.ZOO:
        info = codegen.generate(zoo.make_problem(system, "irl"))[1]
        mdl = runtime.ModelLib.__new__(runtime.ModelLib)
        mdl.name, mdl.n, mdl.m = info["name"], info["n"], info["m"]
        assert mdl.oc_x0_vjp_rows() == cx.ROWS[system], system
    # the header of the sweep kernels' pool states the same rule
    src = open(os.path.join(codegen.CSRC, "pdp_sweep_pool.h")).read()
    assert "struct OcX0VjpPool : SweepPool<Mdl::SOLF_NVAR, Mdl::SOLF_NCONST, Mdl::NX * Mdl::NU + Mdl::NX + Mdl::NU> {" in src
    assert "static constexpr int STRIDE = (NVAR + TAIL) | 1;" in src and "constexpr int SWEEP_POOL_DOUBLES = 2400;" in src
    assert "SWEEP_POOL_DOUBLES / stride < 4 ? 4 : (SWEEP_POOL_DOUBLES / stride > 64 ? 64 : SWEEP_POOL_DOUBLES / stride)" in src
    assert runtime.SWEEP_POOL_DOUBLES == 2400


@pytest.mark.parametrize("case", __import__("oc_x0_vjp_common").reference_cases(), ids=lambda cs: "%s_B%d_T%d_%s" % (cs[0], cs[1], cs[2], "per_sample" if cs[3] else "shared"))
def test_adjoint_sweep_equals_the_references_forward_sensitivities(case):
    """the kernel's recursion (numpy, own gains) against lqr_solver from X_0 = [0 | I] contracted with the cotangents: 1e-11 of the largest entry per sample, a tenth of
    the GPU tolerance - the reference's own error on these inputs is then below what the GPU tests ask"""
    import oc_vjp_common as c
    import oc_x0_vjp_common as cx
    r = cx.reference_case(*case)
    assert np.isfinite(r["ref"]).all() and np.abs(r["ref"]).max() > 0
    err = c.rel_per_sample(r["sweep"], r["ref"])
    print("adjoint sweep vs reference, %s: %.3e" % (case, err))
    assert err <= 1e-11, (case, err)


@pytest.mark.parametrize("system", ["pendulum", "cartpole"])
def test_reference_equals_central_differences_through_re_solving(system):
    """L(x*(x0), u*(x0)) with x*, u* from OCSysOracle.solve_oc: dL/dx0 by the reference at the solved trajectory (state[0]'s own cotangent included) against central
    differences at x0 +- 1e-5 e_k; 2e-4 of the largest difference, tests/test_gpu_oc_vjp.py's bound for the same kind of check"""
    import oc_vjp_common as c
    import oc_x0_vjp_common as cx
    oc = cx.oracle_oc(system)
    n, m = c.DIMS[system]
    # a stored demonstration (an optimal trajectory of the reference at its true parameter) is the Newton solve's starting point: from zero controls it does not converge
    d = np.load(os.path.join(HERE, "golden", "demos_%s.npz" % system))
    theta, x0, T = d["true_parameter"], d["state"][0][0], d["control"].shape[1]
    w = np.arange(1, n + 1) / n

    def loss(sol):
        x, u = sol["state_traj_opt"], sol["control_traj_opt"]
        return float((w * (x[T // 2] - 0.2) ** 2).sum() + (w * (x[T] + 0.1) ** 2).sum() + 0.5 * (x[0] ** 2).sum() + 0.01 * (u ** 2).sum())
    sol = oc.solve_oc(x0, T, theta, guess=(d["state"][0], d["control"][0], d["costate"][0]))
    assert sol["kkt_residual"] < 1e-10
    x, u, lam = sol["state_traj_opt"], sol["control_traj_opt"], sol["costate_traj_opt"]
    gx = np.zeros((T + 1, n))
    gx[T // 2], gx[T], gx[0] = 2 * w * (x[T // 2] - 0.2), 2 * w * (x[T] + 0.1), x[0]
    g = cx.reference_grad_x0(oc, x, u, lam, theta, gx, 0.02 * u)
    assert np.abs(cx.adjoint_sweep(oc.getAuxSys(x, u, lam, theta), gx, 0.02 * u) - g).max() <= 1e-11 * np.abs(g).max()
    eps, guess = 1e-5, (x, u, lam)
    fd = np.array([(loss(oc.solve_oc(x0 + eps * e, T, theta, guess=guess)) - loss(oc.solve_oc(x0 - eps * e, T, theta, guess=guess))) / (2 * eps) for e in np.eye(n)])
    err = np.abs(g - fd).max() / np.abs(fd).max()
    print("reference dL/dx0 vs central differences, %s: %.3e" % (system, err))
    assert err <= 2e-4, (system, err)
