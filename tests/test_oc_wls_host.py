"""CPU (no GPU needed): pdp_oc_pdp_grad_wls_batched - the fused OC / IRL unit as weighted and Huber-robust least squares - at the ABI (the header, the binding's lists,
the argument errors before any launch), the ValueErrors of the Python layers before any foreign call, the CPU oracle's row (oracle/ipopt_ms.solve, pdp_oracle.pdp_oc_unit,
the header's formulas in numpy: tests/oc_wls_common.py) against central differences of the loss through re-solved OC problems, and the oracle's Levenberg-Marquardt
schedule on the corrupted demonstrations that the GPU tests are held to (DESIGN.md section 4.1h holds the figures)."""
import ctypes as C
import os

import numpy as np
import pytest

import oc_wls_common as ow

ROOT = ow.ROOT
NAME = "pdp_oc_pdp_grad_wls_batched"
INF = float("inf")

PLAIN_COUNTS, HUBER_COUNTS, TRUST_COUNTS = ow.PLAIN_COUNTS, ow.HUBER_COUNTS, ow.TRUST_COUNTS          # the evaluation counts written down with the helper


def _built():
    import __graft_entry__ as g
    g.build()
    from pdp_amd import codegen, runtime as rt, zoo
    return codegen, rt, zoo


def test_the_entry_point_is_declared_listed_and_exported():
    """(tests/test_abi_table.py holds the whole binding against the headers and the built libraries; what stays here is this entry point's own line)"""
    from pdp_amd import abi
    (name, (restype, sig)), = abi.entry_points("pdp_hip_oc_wls.h", "model").items()
    assert name == NAME and restype is C.c_int
    assert len(sig) == 22 and sig[10] is C.c_int64 and sig[12] is C.c_int64 and sig[13] is C.c_double and sig[20] is C.c_int64


def test_argument_errors_are_returned_before_any_launch():
    """Valid (host) pointers everywhere, so that only the argument under test can be what is refused; the horizon is far beyond the kernels' LDS, so that a call that
    passes the argument checks returns PDP_E_SIZE and nothing is ever launched, with or without a GPU in the machine."""
    codegen, rt, zoo = _built()
    for system, n, m in (("quadrotor", 13, 4), ("cartpole", 4, 1)):
        mdl = rt.load_model(codegen.build_problem(zoo.make_problem(system, "irl"))[0])
        assert (mdl.n, mdl.m) == (n, m)
        B, T = 1, 100000
        keep = [(C.c_double * 8)() for _ in range(14)]
        x0, u, th, dx, du, wx, wu, x, lam, loss, packed, status, ws = (C.cast(k, C.c_void_p) for k in keep[:13])
        ok = dict(B=B, T=T, flags=0, x0=x0, u=u, th=th, dx=dx, du=du, wx=wx, wxs=(T + 1) * n, wu=wu, wus=T * m, delta=0.5, x=x, lam=lam, loss=loss, packed=packed,
                  status=status, ws=ws, wsb=1 << 60)

        def call(fn=getattr(mdl.lib, NAME), **kw):
            a = dict(ok, **kw)
            return fn(a["B"], a["T"], a["flags"], a["x0"], a["u"], a["th"], 0, a["dx"], a["du"], a["wx"], a["wxs"], a["wu"], a["wus"], a["delta"], a["x"], a["lam"],
                      a["loss"], a["packed"], a["status"], a["ws"], a["wsb"], None)
        for kw in (dict(flags=2), dict(flags=4), dict(flags=8), dict(flags=16), dict(flags=32 | 16), dict(flags=64), dict(flags=-1),
                   dict(delta=0.0), dict(delta=-1.0), dict(delta=-INF), dict(delta=float("nan")),
                   dict(wxs=1), dict(wxs=n), dict(wxs=T * n), dict(wxs=-(T + 1) * n), dict(wxs=T * m), dict(wx=None, wxs=7),
                   dict(wus=1), dict(wus=m), dict(wus=(T + 1) * m), dict(wus=-T * m), dict(wus=T * m + 1), dict(wu=None, wus=7),
                   dict(u=None), dict(th=None), dict(dx=None), dict(du=None), dict(x=None), dict(lam=None), dict(loss=None), dict(packed=None), dict(status=None),
                   dict(ws=None), dict(x0=None), dict(B=0), dict(B=-3), dict(T=0, wxs=0, wus=0), dict(T=-2, wxs=0, wus=0), dict(wsb=0), dict(wsb=8)):
            assert call(**kw) == -1, (system, kw)                                   # PDP_E_ARG
        for kw in (dict(), dict(delta=INF), dict(flags=1), dict(flags=32), dict(flags=33), dict(flags=1, x0=None), dict(wxs=0), dict(wus=0), dict(wxs=0, wus=0),
                   dict(wx=None, wxs=0), dict(wu=None, wus=0), dict(wx=None, wu=None, wxs=0, wus=0), dict(wx=None), dict(wu=None)):
            assert call(**kw) == -2, (system, kw)                                   # the checks pass; the horizon is beyond LDS: PDP_E_SIZE, before any launch
        assert all(v == 0.0 for k in keep for v in k)
    sid = rt.load_model(codegen.build_problem(zoo.make_problem("cartpole", "sysid"))[0])
    for flags in (0, 1, 32):
        for delta in (INF, 0.1):
            assert call(getattr(sid.lib, NAME), flags=flags, delta=delta) == -4      # PDP_E_MODE: not an OC model


def test_weights_and_delta_are_normalised_or_refused():
    import torch
    from pdp_amd.runtime import oc_wls_arguments
    B, T, n, m = 3, 6, 4, 2
    assert oc_wls_arguments(None, None, None, B, T, n, m) == (None, 0, None, 0, INF) and oc_wls_arguments(None, None, 0.5, B, T, n, m) == (None, 0, None, 0, 0.5)
    wx, wxs, wu, wus, delta = oc_wls_arguments(np.arange(4.0), np.arange(2.0), None, B, T, n, m)
    assert wx.shape == (T + 1, n) and wxs == 0 and wu.shape == (T, m) and wus == 0 and delta == INF and (wx == np.arange(4.0)).all() and (wu == np.arange(2.0)).all()
    wx, wxs, wu, wus, _ = oc_wls_arguments(np.ones((T + 1, n)), np.ones((B, T, m)), 1.0, B, T, n, m)
    assert wx.shape == (T + 1, n) and wxs == 0 and wu.shape == (B, T, m) and wus == T * m
    wx, wxs, wu, wus, _ = oc_wls_arguments(torch.ones((B, T + 1, n), dtype=torch.float64), None, 1.0, B, T, n, m)
    assert tuple(wx.shape) == (B, T + 1, n) and wxs == (T + 1) * n and wu is None and wus == 0
    wx, wxs, wu, wus, _ = oc_wls_arguments(None, torch.ones(m, dtype=torch.float64), INF, B, T, n, m)
    assert wx is None and tuple(wu.shape) == (T, m) and wus == 0
    for bad in (-np.ones(n), np.array([1.0, np.nan, 1.0, 1.0]), np.array([1.0, INF, 1.0, 1.0]), np.ones((T, n)), np.ones((B, T + 1)), np.ones((1, T + 1, n)), np.ones(()),
                np.ones((B, T, n))):
        with pytest.raises(ValueError, match="weights_x"):
            oc_wls_arguments(bad, None, None, B, T, n, m)
    for bad in (-np.ones(m), np.array([1.0, np.nan]), np.array([INF, 1.0]), np.ones((T + 1, m)), np.ones((B, T)), np.ones((1, T, m)), np.ones(()), np.ones((B, T + 1, m))):
        with pytest.raises(ValueError, match="weights_u"):
            oc_wls_arguments(None, bad, None, B, T, n, m)
    for bad in (0.0, -1.0, float("nan"), -INF):
        with pytest.raises(ValueError, match="huber_delta"):
            oc_wls_arguments(None, None, bad, B, T, n, m)


class _NoForeignCalls:
    def __getattr__(self, name):
        raise AssertionError("foreign call %s before the arguments were validated" % name)


def test_every_layer_refuses_before_any_foreign_call():
    from pdp_amd import PDP, runtime
    from pdp_amd.irl import BatchedLMLoop, LMLoop
    mdl = runtime.ModelLib.__new__(runtime.ModelLib)
    mdl.n, mdl.m, mdl.p, mdl.lib = 4, 1, 7, _NoForeignCalls()
    B, T = 3, 6
    u, th, x0, dx, du = np.zeros((B, T, 1)), np.ones(7), np.zeros((B, 4)), np.zeros((B, T + 1, 4)), np.zeros((B, T, 1))
    given = (dict(weights_x=np.ones(4)), dict(weights_u=np.ones(1)), dict(huber_delta=0.5), dict(weights_x=np.ones(4), weights_u=np.ones(1), huber_delta=0.5))
    bad = ((dict(weights_x=-np.ones(4)), "weights_x"), (dict(weights_x=np.ones((B, T, 4))), "weights_x"), (dict(weights_x=np.full(4, np.nan)), "weights_x"),
           (dict(weights_u=np.full(1, INF)), "weights_u"), (dict(weights_u=np.ones((T + 1, 1))), "weights_u"), (dict(huber_delta=0.0), "huber_delta"),
           (dict(huber_delta=-0.1), "huber_delta"), (dict(huber_delta=float("nan")), "huber_delta"))
    for w in given:
        for kw, name in ((dict(want_sens=True), "want_sens"), (dict(want_riccati=True), "want_riccati"), (dict(want_predict_record=True), "want_predict_record"),
                         (dict(want_predict_record="primal"), "want_predict_record"), (dict(packed=True), "packed")):
            with pytest.raises(ValueError, match=name):
                mdl.oc_pdp_grad(u, th, dx, du, x0=x0, **w, **kw)
    for kw, match in bad:
        with pytest.raises(ValueError, match=match):
            mdl.oc_pdp_grad(u, th, dx, du, x0=x0, **kw)
        with pytest.raises(ValueError, match=match):
            mdl.oc_pdp_grad(u, th, dx, du, x0=x0, skip_missing=True, **kw)
    oc = PDP.OCSys.__new__(PDP.OCSys)
    oc.n_state, oc.n_control = 4, 1
    rename = dict(weights_x="weights_state", weights_u="weights_control", huber_delta="huber_delta")
    for w in given:
        w = {rename[k]: v for k, v in w.items()}
        for kw, name in ((dict(want_sens=True), "want_sens"), (dict(want_riccati=True), "want_riccati"), (dict(want_predict_record=True), "want_predict_record")):
            with pytest.raises(ValueError, match=name):
                oc.pdp_grad_batch(u, th, dx, du, ini_state=x0, **w, **kw)
    for kw, match in bad:
        with pytest.raises(ValueError, match=match):
            oc.pdp_grad_batch(u, th, dx, du, ini_state=x0, **{rename[k]: v for k, v in kw.items()})
    for loop in (LMLoop, BatchedLMLoop):
        for kw, match in bad:
            with pytest.raises(ValueError, match=match):
                loop.for_irl(mdl, dx, du, np.ones(7), **{rename[k]: v for k, v in kw.items()})
    nan_x = dx.copy()
    nan_x[1, 0, 2] = np.nan
    for loop in (LMLoop, BatchedLMLoop):                                            # the NaN-start check under skip_missing stays
        with pytest.raises(ValueError, match="ini_state"):
            loop.for_irl(mdl, nan_x, du, np.ones(7), skip_missing=True, weights_state=np.ones(4), huber_delta=0.5)


@pytest.mark.parametrize("system", ["pendulum", "cartpole"])
def test_oracle_gradient_agrees_with_central_differences(system):
    """The corrupted demonstrations with every third state row and every sixth control row NaN (PDP_GRAD_SKIP_MISSING), per-component state weights and a control weight
    with zeros on observed and on missing entries, Huber at the median of |e| (entries on both branches), a perturbed theta: grad [p] is half the derivative of the
    loss with respect to theta through the RE-SOLVED OC problem (h = 1e-6): 1e-7 of its largest entry.  Seen with solves at tol = 1e-10: 1.6e-8 (pendulum), 2.8e-8
    (cart-pole) - the same at tol = 1e-13: the finite difference's own error, not the solves'."""
    c = ow.corrupted(system)
    rng = np.random.default_rng(3)
    T, n, m = c["demo_u"].shape[1], c["demo_x"].shape[2], c["demo_u"].shape[2]
    wx = np.broadcast_to(1.0 / (0.5 + np.arange(n)) ** 2, c["demo_x"].shape).copy()
    wx[:, 4::5] = 0.0
    wu = np.full(c["demo_u"].shape, 2.0)
    wu[:, 3::7] = 0.0
    dx, du = c["demo_x"].copy(), c["demo_u"].copy()
    dx[:, 2::3], du[:, 5::6] = np.nan, np.nan
    theta = c["theta0"] * (1.0 + 0.05 * rng.standard_normal(c["theta0"].size))
    one = lambda a: a[:1]
    args = (system, one(c["x0"]), theta, one(dx), one(du), one(wx), one(wu))
    sols = ow.oracle_rows(*args, INF, True)[3]
    x, u = np.asarray(sols[0][0]), np.asarray(sols[0][1]).reshape(T, m)
    ox, ou = (wx[0] > 0) & ~np.isnan(dx[0]), (wu[0] > 0) & ~np.isnan(du[0])
    e = np.concatenate([(np.sqrt(wx[0]) * np.abs(x - np.nan_to_num(dx[0])))[ox], (np.sqrt(wu[0]) * np.abs(u - np.nan_to_num(du[0])))[ou]])
    delta = float(np.median(e))
    assert 4 * (e <= delta).sum() >= e.size and 4 * (e > delta).sum() >= e.size        # both branches
    _, grad, _, sols = ow.oracle_rows(*args, delta, True)
    h = 1e-6
    loss = lambda th: ow.oracle_rows(system, one(c["x0"]), th, one(dx), one(du), one(wx), one(wu), delta, True, warm=sols)[0][0]
    fd = np.array([(loss(theta + h * e_) - loss(theta - h * e_)) / (2 * h) for e_ in np.eye(theta.size)]) / 2
    err = np.abs(fd - grad[0]).max() / np.abs(grad[0]).max()
    print("%s: central differences through re-solved problems vs the oracle's row %.2e (delta %.3e, %d of %d entries beyond it)" % (system, err, delta, (e > delta).sum(), e.size))
    assert err <= 1e-7


def test_corrupted_data_set_is_the_one_written_down():
    for system, (kx, ku) in ow.CORRUPTED_ENTRIES.items():
        c = ow.corrupted(system)
        assert int(c["cx"].sum()) == kx and int(c["cu"].sum()) == ku and not c["cx"][:, 0].any()
        for moved, hit in ((np.abs(c["demo_x"] - c["clean_x"]), c["cx"]), (np.abs(c["demo_u"] - c["clean_u"]), c["cu"])):
            assert ((moved[hit] >= 0.5) & (moved[hit] <= 1.5)).all() and not moved[~hit].any()
        assert (c["trust_x"][c["cx"]] == 0).all() and (c["trust_x"][~c["cx"]] == 1).all() and (c["trust_u"][c["cu"]] == 0).all() and (c["trust_u"][~c["cu"]] == 1).all()


@pytest.mark.parametrize("system", sorted(TRUST_COUNTS))
def test_oracle_schedule_with_weight_zero_on_the_corrupted_entries(system):
    """weight 0 on the corrupted entries: the problem is the clean one again"""
    r = ow.oracle_lm(system, "trust", loss_tol=1e-16)
    print(system, r["evaluations"], " ".join("%.3e" % v for v in r["loss_trace"]), "theta error %.2e" % ow.theta_error(r, system))
    assert r["evaluations"] == TRUST_COUNTS[system] and r["rejected"] == 0 and not r["stalled"]
    assert (np.diff(r["loss_trace"]) < 0).all() and r["loss_trace"][-1] <= 1e-16
    assert ow.theta_error(r, system) <= 1e-8
    for b_, k in enumerate(ow.TRUST_COUNTS_PER_DEMO[system]):                        # one problem per demonstration: what BatchedLMLoop's budget is taken from
        assert ow.oracle_lm(system, "trust", loss_tol=1e-16, samples=[b_])["evaluations"] == k, (system, b_)


@pytest.mark.parametrize("system", sorted(HUBER_COUNTS))
def test_oracle_schedule_with_huber_is_ten_times_closer_than_plain_least_squares(system):
    """delta = 0.01 on the corrupted demonstrations, unit weights.  Measured 117 x (pendulum: 9.0 -> 7.7e-2) and 107 x (cart-pole: 7.2e-2 -> 6.8e-4), every run ending
    stalled at the non-zero minimum of its loss; the test asks 10 x."""
    plain, robust = ow.oracle_lm(system, "plain"), ow.oracle_lm(system, "huber")
    e0, e1 = ow.theta_error(plain, system), ow.theta_error(robust, system)
    print("%s: plain %.3e (%d evaluations, %d rejected)  Huber %.3e (%d, %d)" % (system, e0, plain["evaluations"], plain["rejected"], e1, robust["evaluations"],
                                                                                robust["rejected"]))
    assert plain["evaluations"] == PLAIN_COUNTS[system] and robust["evaluations"] == HUBER_COUNTS[system]
    assert e1 * 10 <= e0


def test_example_disturbs_the_demonstrations_and_derives_the_weights():
    """examples/irl_pdp.py disturb_demos: --noise-sigma (per state component, then per control component; weights 1 / s^2) and --outliers (never row 0 of the states)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("irl_pdp_example", os.path.join(ROOT, "examples", "irl_pdp.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    rng = np.random.default_rng(0)
    dx, du = rng.standard_normal((5, 31, 4)), rng.standard_normal((5, 30, 1))
    mx, mu, wx, wu, k = ex.disturb_demos(dx, du, outliers=0.05, seed=1)
    hx, hu = mx != dx, mu != du
    assert wx is None and wu is None and k == hx.sum() + hu.sum() and 0 < k < 0.1 * (dx.size + du.size) and not hx[:, 0].any()
    moved = np.concatenate([np.abs(mx - dx)[hx], np.abs(mu - du)[hu]])
    assert ((moved >= 0.5) & (moved <= 1.5)).all()
    mx, mu, wx, wu, k = ex.disturb_demos(dx, du, noise_sigma=[1e-3, 1e-3, 1e-2, 1e-2, 0.1])
    assert k == 0 and np.allclose(wx, [1e6, 1e6, 1e4, 1e4]) and np.allclose(wu, [100.0]) and np.array_equal(mx[:, 0], dx[:, 0])
    assert 0 < np.abs(mx - dx)[:, 1:, :2].max() < 1e-2 and 0 < np.abs(mu - du).max() < 1.0
    with pytest.raises(AssertionError, match="noise-sigma"):
        ex.disturb_demos(dx, du, noise_sigma=[1e-3] * 4)
    assert np.array_equal(ex.disturb_demos(dx, du)[0], dx)
