"""CPU (no GPU needed): the flag words of the C ABI as the host paths of ModelLib form them - opts.flags of pdp_oc_solve_ms_batched and the integer `flags` of the
gradient units and of the SysID least-squares entry points - characterised by what reaches the foreign call, in the manner of tests/test_ls_rows_host.py (the stand-in
library of ls_rows_common records the calls).  Every expected value is a DECIMAL integer read off include/*.h, on purpose: the test was written against the binding that
spelled these words as bare numbers and stays unchanged now that it spells them by the headers' names.  And the branches that test the return code PDP_E_SIZE (-2):
a stand-in that refuses one entry point, and the materialised route must be entered (nothing raises)."""
import ctypes
import types

import numpy as np
import pytest

import ls_rows_common as lr

n, m, p, B, T = 4, 1, 3, 3, 6


class Refusing(lr.Recorder):
    """the recorder, but one entry point answers `code` (PDP_E_SIZE = -2: outside the kernels' limits)"""

    def __init__(self, refused, code=-2):
        lr.Recorder.__init__(self)
        self.refused, self.code = refused, code

    def __getattr__(self, name):
        def f(*args):
            self.calls.append((name, args))
            return self.code if name == self.refused else 0
        return f


def last_call(mdl, name, nargs):
    got, args = mdl.lib.calls[-1]
    assert got == name and len(args) == nargs, (got, len(args))
    return args


def oc_data():
    rng = np.random.default_rng(2)
    return rng.standard_normal((B, T, m)), np.ones(p), rng.standard_normal((B, T + 1, n)), rng.standard_normal((B, T, m)), np.zeros((B, n))


def given_trajectory():
    import torch
    return dict(x=torch.zeros((B, T + 1, n), dtype=torch.float64), lam=torch.zeros((B, T, n), dtype=torch.float64))


# ---- pdp_oc_solve_ms_batched: opts.flags (PDP_MS_* of include/pdp_hip.h), read from the byref object of argument 15 -------------------------------------------------
def _warm():
    return tuple(np.zeros(s) for s in ((B, T + 1, n), (B, T, m), (B, T, n)))


def _predict(**kw):
    return dict(dict(dtheta=np.zeros(p), dxdp=np.zeros((B, T + 1, n, p)), dudp=np.zeros((B, T, m, p))), **kw)


SOLVE_MS = [
    ("cold", dict(), 0),
    ("warm", dict(warm=_warm()), 1),
    ("no_restoration", dict(restoration=False), 2),
    ("warm_no_restoration", dict(warm=_warm(), restoration=False), 3),
    ("u_init", dict(u_init=np.zeros((B, T, m))), 9),
    ("soc", dict(soc=True), 128),
    ("watchdog", dict(watchdog=True), 256),
    ("soc_watchdog_u_init_no_restoration", dict(soc=True, watchdog=True, u_init=np.zeros((B, T, m)), restoration=False), 395),
    ("predict", dict(warm=_warm(), predict=_predict()), 81),                                     # the guard is on by default
    ("predict_unguarded", dict(warm=_warm(), predict=_predict(guard=False)), 17),
    ("predict_primal", dict(warm=_warm(), predict=_predict(primal=True)), 113),
    ("predict_primal_unguarded", dict(warm=_warm(), predict=_predict(primal=True, guard=False)), 49),
]


@pytest.mark.parametrize("case", SOLVE_MS, ids=[c[0] for c in SOLVE_MS])
def test_oc_solve_ms_option_word(monkeypatch, case):
    _, kw, flags = case
    lr.stand_in_torch(monkeypatch)
    mdl = lr.stand_in_model()
    out = mdl.oc_solve_ms(np.zeros((B, n)), np.ones(p), T, **kw)
    opts = last_call(mdl, "pdp_oc_solve_ms_batched", 19)[15]._obj
    assert opts.flags == flags and opts.max_iter == 300 and opts.log_rows == 0
    assert (opts.dtheta is not None) == ("predict" in kw) and opts.predict_record is None
    assert tuple(out["status"].shape) == (B,) and tuple(out["converged"].shape) == (B,)


# ---- the gradient unit: `flags` is argument 2 of pdp_oc_pdp_grad_batched, pdp_oc_pdp_grad_sens_batched and pdp_oc_pdp_grad_wls_batched ----------------------------------
OC_GRAD = [
    ("plain", dict(), False, "pdp_oc_pdp_grad_batched", 19, 0),
    ("given_trajectory", dict(), True, "pdp_oc_pdp_grad_batched", 19, 1),
    ("packed", dict(packed=True), False, "pdp_oc_pdp_grad_batched", 19, 2),
    ("packed_given_trajectory", dict(packed=True), True, "pdp_oc_pdp_grad_batched", 19, 3),
    ("predict_record", dict(want_predict_record=True), False, "pdp_oc_pdp_grad_sens_batched", 18, 0),
    ("predict_record_primal", dict(want_predict_record="primal"), False, "pdp_oc_pdp_grad_sens_batched", 18, 4),
    ("riccati_given_trajectory", dict(want_riccati=True, want_sens=True), True, "pdp_oc_pdp_grad_sens_batched", 18, 1),
    ("skip_missing", dict(skip_missing=True), False, "pdp_oc_pdp_grad_batched", 19, 32),
    ("skip_missing_packed", dict(skip_missing=True, packed=True), False, "pdp_oc_pdp_grad_batched", 19, 34),
    ("gauss_newton", dict(gauss_newton=True), False, "pdp_oc_pdp_grad_batched", 19, 16),
    ("gauss_newton_skip_missing", dict(gauss_newton=True, skip_missing=True), False, "pdp_oc_pdp_grad_batched", 19, 48),
    ("gauss_newton_given_trajectory", dict(gauss_newton=True), True, "pdp_oc_pdp_grad_batched", 19, 17),
    ("weighted", dict(weights_x=np.ones(n)), False, "pdp_oc_pdp_grad_wls_batched", 22, 0),
    ("weighted_skip_missing_given_trajectory", dict(weights_u=np.ones(m), huber_delta=0.5, skip_missing=True), True, "pdp_oc_pdp_grad_wls_batched", 22, 33),
]


@pytest.mark.parametrize("case", OC_GRAD, ids=[c[0] for c in OC_GRAD])
def test_oc_pdp_grad_flag_word(monkeypatch, case):
    _, kw, given, name, nargs, flags = case
    lr.stand_in_torch(monkeypatch)
    mdl = lr.stand_in_model()
    u, th, dx, du, x0 = oc_data()
    mdl.oc_pdp_grad(u, th, dx, du, **(given_trajectory() if given else dict(x0=x0)), **kw)
    assert last_call(mdl, name, nargs)[2] == flags


@pytest.mark.parametrize("given, flags", [(False, 8), (True, 9)], ids=["x0", "given_trajectory"])
def test_oc_pdp_vjp_flag_word(monkeypatch, given, flags):
    lr.stand_in_torch(monkeypatch)
    mdl = lr.stand_in_model()
    u, th, _, _, x0 = oc_data()
    out = mdl.oc_pdp_vjp(u, th, np.ones((B, T + 1, n)), np.ones((B, T, m)), **(given_trajectory() if given else dict(x0=x0)))
    args = last_call(mdl, "pdp_oc_pdp_grad_batched", 19)
    assert args[2] == flags and args[11].value is None and args[12].value == out["grad"].data_ptr()          # no loss is formed; the gradient is plain [B, p]


def prepared_stand_ins(monkeypatch):
    """what oc_pdp_grad_prepared needs beyond stand_in_torch: a current stream, and a row to fill that calls itself a device tensor (the call insists on one)"""
    import torch
    lr.stand_in_torch(monkeypatch).cuda.current_stream = staticmethod(lambda: types.SimpleNamespace(cuda_stream=None))

    class OnDevice(torch.Tensor):
        is_cuda = property(lambda self: True)
    return torch.zeros((B, p + 1), dtype=torch.float64).as_subclass(OnDevice)


def test_oc_pdp_grad_prepared_flag_word(monkeypatch):
    row = prepared_stand_ins(monkeypatch)
    mdl = lr.stand_in_model()
    u, th, dx, du, x0 = oc_data()
    step, out = mdl.oc_pdp_grad_prepared(u, th, dx, du, x0, packed_out=row)
    first = last_call(mdl, "pdp_oc_pdp_grad_batched", 19)
    assert first[2] == 2 and first[12].value == out["packed"].data_ptr()
    mdl.lib.calls.clear()
    step()
    again = last_call(mdl, "pdp_oc_pdp_grad_batched", 19)
    assert again[2] == 2 and [getattr(a, "value", a) for a in again[:18]] == [getattr(a, "value", a) for a in first[:18]]


# ---- SysID.step's three Gauss-Newton routes: `flags` by position (include/pdp_hip_sysid_gn.h, pdp_hip_sysid_ini.h, pdp_hip_sysid_wls.h) --------------------------------
SYSID = [
    ("gn", dict(gauss_newton=True), "pdp_sysid_step_gn_batched", 13, 7),
    ("gn_ini", dict(gauss_newton=True, estimate_ini=[1, 3]), "pdp_sysid_step_gn_ini_batched", 14, 8),
    ("wls", dict(weights=np.ones(n)), "pdp_sysid_step_wls_batched", 17, 11),
]


@pytest.mark.parametrize("skip_missing", [False, True], ids=["all_observed", "skip_missing"])
@pytest.mark.parametrize("case", SYSID, ids=[c[0] for c in SYSID])
def test_sysid_step_flag_word(monkeypatch, case, skip_missing):
    _, kw, name, nargs, at = case
    lr.stand_in_torch(monkeypatch)
    mdl = lr.stand_in_model()
    rng = np.random.default_rng(3)
    mdl.sysid_step(rng.standard_normal((B, T, m)), rng.standard_normal((B, T + 1, n)), np.ones(p), skip_missing=skip_missing, **kw)
    assert last_call(mdl, name, nargs)[at] == (32 if skip_missing else 0)


# ---- the return code -2 (PDP_E_SIZE): the materialised route is entered and nothing raises ------------------------------------------------------------------------------
def refused_model(entry_point, code=-2):
    mdl = lr.stand_in_model()
    mdl.lib = Refusing(entry_point, code)
    return mdl


OC_FALLBACK = [
    ("plain", dict(), "_oc_pdp_grad_materialised", 0, None),
    ("packed", dict(packed=True), "_oc_pdp_grad_materialised", 2, None),
    ("want_sens", dict(want_sens=True), "_oc_pdp_grad_materialised", 0, None),
    ("skip_missing", dict(skip_missing=True), "_oc_rows_materialised", 32, "missing_data"),
    ("gauss_newton", dict(gauss_newton=True), "_oc_rows_materialised", 16, "plain"),
    ("gauss_newton_skip_missing", dict(gauss_newton=True, skip_missing=True), "_oc_rows_materialised", 48, "missing_data"),
]


@pytest.mark.parametrize("case", OC_FALLBACK, ids=[c[0] for c in OC_FALLBACK])
def test_oc_pdp_grad_beyond_the_fused_kernels_takes_the_materialised_route(monkeypatch, case):
    _, kw, route, flags, rule = case
    lr.stand_in_torch(monkeypatch)
    mdl = refused_model("pdp_oc_pdp_grad_batched")
    entered = []
    setattr(mdl, route, lambda *a, **k: entered.append(a))
    u, th, dx, du, x0 = oc_data()
    with pytest.warns(RuntimeWarning, match="kernel-by-kernel route"):
        out = mdl.oc_pdp_grad(u, th, dx, du, x0=x0, **kw)
    assert len(entered) == 1 and entered[0][7] == flags and (rule is None or entered[0][11] == rule)      # (u, th, demo_x, demo_u, x0, x, lam, flags, loss, row, status, rule)
    assert tuple(out["grad"].shape) == (B, p) and tuple(out["loss"].shape) == (B,)


def test_weighted_oc_rows_beyond_the_fused_kernels_take_the_materialised_route(monkeypatch):
    lr.stand_in_torch(monkeypatch)
    mdl = refused_model("pdp_oc_pdp_grad_wls_batched")
    entered = []
    mdl._oc_rows_materialised = lambda *a, **k: entered.append(a)
    u, th, dx, du, x0 = oc_data()
    with pytest.warns(RuntimeWarning, match="kernel-by-kernel route"):
        out = mdl.oc_pdp_grad(u, th, dx, du, x0=x0, weights_x=np.ones(n), skip_missing=True)
    assert len(entered) == 1 and entered[0][7] == 32 and entered[0][11] == "weighted" and tuple(out["packed_gn"].shape) == (B, p + 1 + p * p)


def test_prediction_records_beyond_the_fused_kernels_are_refused_by_name(monkeypatch):
    lr.stand_in_torch(monkeypatch)
    mdl = refused_model("pdp_oc_pdp_grad_sens_batched")
    u, th, dx, du, x0 = oc_data()
    with pytest.raises(RuntimeError, match="outputs of the fused kernels"):
        mdl.oc_pdp_grad(u, th, dx, du, x0=x0, want_predict_record=True)


def test_oc_pdp_vjp_beyond_the_fused_kernels_takes_the_materialised_route(monkeypatch):
    lr.stand_in_torch(monkeypatch)
    mdl = refused_model("pdp_oc_pdp_grad_batched")
    entered = []
    mdl._oc_pdp_grad_materialised = lambda *a, **k: entered.append(a)
    u, th, _, _, x0 = oc_data()
    with pytest.warns(RuntimeWarning, match="kernel-by-kernel route"):
        out = mdl.oc_pdp_vjp(u, th, np.ones((B, T + 1, n)), np.ones((B, T, m)), x0=x0)
    assert len(entered) == 1 and entered[0][7] == 8 and entered[0][8] is None and tuple(out["grad"].shape) == (B, p)


def test_another_error_code_is_an_error_by_its_name(monkeypatch):
    row = prepared_stand_ins(monkeypatch)
    u, th, dx, du, x0 = oc_data()
    for code, text in ((-1, "PDP_E_ARG"), (-3, "PDP_E_LAUNCH"), (-4, "PDP_E_MODE")):
        mdl = refused_model("pdp_oc_pdp_grad_batched", code)
        with pytest.raises(RuntimeError, match="pdp_oc_pdp_grad_batched failed: %s" % text):
            mdl.oc_pdp_grad(u, th, dx, du, x0=x0)
    mdl = refused_model("pdp_oc_pdp_grad_batched")
    with pytest.raises(RuntimeError, match=r"prepared call\): PDP_E_SIZE"):
        mdl.oc_pdp_grad_prepared(u, th, dx, du, x0, packed_out=row)


def _materialised_stages(monkeypatch, mdl):
    """the stages of ModelLib._oc_pdp_grad_materialised as stand-ins: zeros of the right shapes, a record of which ran, a Recorder for the core library"""
    import torch
    from pdp_amd import runtime
    z = lambda *s: torch.zeros(s, dtype=torch.float64)

    class Core(lr.Recorder):                                                        # (keeps a copy of the first contracted operand: it does not outlive the call)
        def __getattr__(self, name):
            def f(*args):
                self.calls.append((name, args))
                self.ex_path = np.ctypeslib.as_array((ctypes.c_double * (B * T * n)).from_address(args[5].value)).reshape(B, T, n).copy()
                return 0
            return f
    ran, core = [], Core()
    mdl.oc_rollout = lambda x0, u, theta, want_cost=True: (ran.append("rollout") or z(B, T + 1, n), None)
    mdl.oc_costate = lambda x, u, theta: ran.append("costate") or z(B, T, n)
    mdl.oc_auxsys = lambda x, u, lam, theta, only=None: ran.append("auxsys") or dict.fromkeys(("dynF", "dynG", "dynE", "Hxx", "Hxu", "Hxe", "Huu", "Hue", "hxx", "hxe"))
    monkeypatch.setattr(runtime, "lqr_solve", lambda *a, **k: (z(B, T + 1, n, p), z(B, T, m, p), None, torch.zeros(B, dtype=torch.int32)))
    monkeypatch.setattr(runtime, "load_core", lambda: core)
    return ran, core


def test_the_materialised_gradient_reads_the_given_trajectory_and_cotangent_bits(monkeypatch):
    """flags & 1 (PDP_OC_GIVEN_TRAJ): no rollout, no costates; flags & 8 (PDP_OC_COTANGENT): no loss is formed (none is there to write into) and row 0 of the
    cotangent is not read; the contraction is one call of pdp_cp_grad_contract_batched of the core library either way"""
    import torch
    lr.stand_in_torch(monkeypatch)
    mdl = lr.stand_in_model()
    ran, core = _materialised_stages(monkeypatch, mdl)
    u, th, dx, du, x0 = oc_data()
    out = mdl.oc_pdp_grad_materialised(u, th, dx, du, x0=x0)
    assert ran == ["rollout", "costate", "auxsys"] and [c[0] for c in core.calls] == ["pdp_cp_grad_contract_batched"] and len(core.calls[0][1]) == 12
    assert core.calls[0][1][:5] == (B, T, n, m, p)
    want = (torch.as_tensor(dx) ** 2).sum(dim=(1, 2)) + (torch.as_tensor(u - du) ** 2).sum(dim=(1, 2))         # the stand-in rollout is zero
    assert torch.equal(out["loss"], want)
    del ran[:], core.calls[:]
    mdl.oc_pdp_grad_materialised(u, th, dx, du, **given_trajectory())
    assert ran == ["auxsys"] and [c[0] for c in core.calls] == ["pdp_cp_grad_contract_batched"]
    del ran[:], core.calls[:]
    mdl.lib = Refusing("pdp_oc_pdp_grad_batched")
    gx = np.ones((B, T + 1, n))
    with pytest.warns(RuntimeWarning, match="kernel-by-kernel route"):
        mdl.oc_pdp_vjp(u, th, gx, np.ones((B, T, m)), x0=x0)
    assert ran == ["rollout", "costate", "auxsys"] and len(core.calls) == 1
    assert (core.ex_path[:, 0] == 0.0).all() and (core.ex_path[:, 1:] == 1.0).all() and (gx == 1.0).all()


def test_cp_integrate_beyond_the_integrator_rolls_out_with_the_step_kernel(monkeypatch):
    import torch
    from pdp_amd import runtime
    lr.stand_in_torch(monkeypatch)
    mdl = refused_model("pdp_cp_integrate_batched")
    entered = []
    z = lambda *s: torch.zeros(s, dtype=torch.float64)
    mdl.cp_step = lambda pol, p_, x0, theta, T_, want_traj=False: entered.append((p_, T_, want_traj)) or (z(B), z(B, p_), z(B, T_ + 1, n), z(B, T_, m))
    x, u, loss = mdl.cp_integrate_T(runtime.make_policy("poly", pivots=[0.0, 3.0, 6.0]), 3, np.zeros((B, n)), np.ones(3), T)
    assert entered == [(3, T, True)] and tuple(x.shape) == (B, T + 1, n) and tuple(u.shape) == (B, T, m) and tuple(loss.shape) == (B,)


def test_sysid_step_beyond_the_fused_kernels_takes_the_materialised_route(monkeypatch):
    import torch
    from pdp_amd import runtime
    lr.stand_in_torch(monkeypatch)
    rng = np.random.default_rng(4)
    u, xo, th = rng.standard_normal((B, T, m)), rng.standard_normal((B, T + 1, n)), np.ones(p)
    mdl = refused_model("pdp_sysid_step_ws_batched")
    entered = []
    monkeypatch.setattr(runtime, "sysid_aux_integrate", lambda F, E, X0=None: entered.append("aux") or torch.zeros((B, T + 1, n, p), dtype=torch.float64))
    loss, grad = mdl.sysid_step(u, xo, th)
    assert entered == ["aux"] and [c[0] for c in mdl.lib.calls][-2:] == ["pdp_sysid_integrate_batched", "pdp_sysid_auxsys_batched"]
    assert tuple(loss.shape) == (B,) and tuple(grad.shape) == (B, p)
    for _, kw, name, _, _ in SYSID:
        for skip_missing in (False, True):
            mdl = refused_model(name)
            width = p + len(kw.get("estimate_ini", ()))
            del entered[:]
            mdl._sysid_materialised = lambda u_, xobs, th_, x0, ini_index=(): entered.append(list(ini_index)) or (
                torch.zeros((B, T + 1, n), dtype=torch.float64), torch.zeros((B, T + 1, n, p + len(ini_index)), dtype=torch.float64))
            out = mdl.sysid_step(u, xo, th, skip_missing=skip_missing, **kw)
            assert entered == [list(kw.get("estimate_ini", ()))] and tuple(out["packed_gn"].shape) == (B, width + 1 + width * width)
            assert torch.equal(out["loss"], (torch.as_tensor(xo) ** 2).sum(dim=(1, 2)))                          # the stand-in rollout is zero, every weight is one
