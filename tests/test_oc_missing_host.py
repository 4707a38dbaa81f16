"""CPU (no GPU needed): PDP_GRAD_SKIP_MISSING (a NaN in demo_x / demo_u is an entry that was not observed) - its ABI constant, its argument validation at the entry points
before any launch, and the refusals of ModelLib.oc_pdp_grad, OCSys.pdp_grad_batch and LMLoop.for_irl before any foreign call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_defines_the_flag_and_keeps_its_33_entry_points_and_four_oc_defines():
    src = open(os.path.join(ROOT, "include", "pdp_hip.h")).read()
    assert re.search(r"^#define\s+PDP_GRAD_SKIP_MISSING\s+32\b", src, flags=re.M)
    assert re.search(r"^#define\s+PDP_GRAD_GAUSS_NEWTON\s+16\b", src, flags=re.M)
    flags = {k: int(v) for k, v in re.findall(r"^#define\s+(PDP_OC_[A-Z_]+)\s+(\d+)", src, flags=re.M)}
    assert flags == {"PDP_OC_GIVEN_TRAJ": 1, "PDP_OC_PACKED": 2, "PDP_OC_RECORD_PRIMAL": 4, "PDP_OC_COTANGENT": 8}      # no PDP_OC_* define was added; 32 is a new bit
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert len(set(re.findall(r"\b(pdp_[a-z0-9_]+)\s*\(", code))) == 33


def test_entry_points_accept_the_valid_and_reject_the_bad_combinations_before_any_launch():
    """Valid (host) pointers everywhere, so that only the flag combination can be what is refused; the horizon is far beyond the kernels' LDS, so that a call that passes
    the argument checks returns PDP_E_SIZE - where it is returned today - and nothing is ever launched, with or without a GPU in the machine."""
    import __graft_entry__ as g
    g.build()
    from pdp_amd import codegen, runtime as rt, zoo
    for system in ("quadrotor", "cartpole"):
        mdl = rt.load_model(codegen.build_problem(zoo.make_problem(system, "irl"))[0])
        B, T = 1, 100000
        keep = [(C.c_double * 8)() for _ in range(16)]
        x0, u, th, dx, du, x, lam, loss, grad, dxdp, dudp, ric, ws = (C.cast(k, C.c_void_p) for k in keep[:13])
        prec, status = C.cast(keep[13], C.c_void_p), C.cast(keep[14], C.c_void_p)
        big = 1 << 60

        def plain(flags, dx_=None, du_=None):
            return mdl.lib.pdp_oc_pdp_grad_batched(B, T, flags, x0, u, th, 0, dx, du, x, lam, loss, grad, dx_, du_, status, ws, big, None)

        def sens(flags, **kw):
            so = rt.PdpOcSensOut(*[kw.get(k).value if k in kw else None for k in ("dxdp", "dudp", "riccati", "predict_record")])
            return mdl.lib.pdp_oc_pdp_grad_sens_batched(B, T, flags, x0, u, th, 0, dx, du, x, lam, loss, grad, C.byref(so), status, ws, big, None)
        for flags in (32, 32 | 1, 32 | 2, 32 | 16, 32 | 16 | 1):                  # PDP_E_SIZE: the combination passed the argument checks
            assert plain(flags) == -2, (system, flags)
            assert sens(flags) == -2, (system, flags)
        assert plain(32 | 8) == -1 and plain(32 | 8 | 16) == -1 and sens(32 | 8) == -1 and sens(32 | 8 | 16) == -1
        assert plain(32, dx_=dxdp) == -1 and plain(32, du_=dudp) == -1 and plain(32, dx_=dxdp, du_=dudp) == -1
        assert sens(32, dxdp=dxdp) == -1 and sens(32, dudp=dudp) == -1 and sens(32, riccati=ric) == -1 and sens(32, predict_record=prec) == -1
        assert plain(32 | 16, dx_=dxdp) == -1 and sens(32 | 16, riccati=ric) == -1 and plain(32 | 16 | 2) == -1
        assert plain(0) == -2 and plain(16) == -2 and plain(8) == -2 and plain(0, dx_=dxdp) == -2     # without the flag: as before


class _NoForeignCalls:
    def __getattr__(self, name):
        raise AssertionError("foreign call %s before the arguments were validated" % name)


def test_runtime_and_class_surface_reject_the_combinations_before_any_foreign_call():
    from pdp_amd import PDP, runtime
    mdl = runtime.ModelLib.__new__(runtime.ModelLib)
    mdl.n, mdl.m, mdl.p, mdl.lib = 4, 1, 7, _NoForeignCalls()
    B, T = 3, 6
    u, th, x0, dx, du = np.zeros((B, T, 1)), np.ones(7), np.zeros((B, 4)), np.full((B, T + 1, 4), np.nan), np.zeros((B, T, 1))
    for kw in (dict(want_sens=True), dict(want_riccati=True), dict(want_predict_record=True), dict(want_predict_record="primal"), dict(want_sens=True, want_riccati=True),
               dict(want_sens=True, packed=True)):
        with pytest.raises(ValueError, match="skip_missing"):
            mdl.oc_pdp_grad(u, th, dx, du, x0=x0, skip_missing=True, **kw)
        with pytest.raises(ValueError, match="skip_missing"):
            mdl.oc_pdp_grad(u, th, dx, du, x0=x0, skip_missing=True, gauss_newton=True, **kw)
    with pytest.raises(TypeError):                                          # the cotangent call has no such switch: a NaN cotangent is an error, not an absence
        mdl.oc_pdp_vjp(u, th, dx, du, x0=x0, skip_missing=True)
    oc = PDP.OCSys.__new__(PDP.OCSys)
    for kw in (dict(want_sens=True), dict(want_riccati=True), dict(want_predict_record=True)):
        with pytest.raises(ValueError, match="skip_missing"):
            oc.pdp_grad_batch(u, th, dx, du, ini_state=x0, skip_missing=True, **kw)
        with pytest.raises(ValueError, match="skip_missing"):
            oc.pdp_grad_batch(u, th, dx, du, ini_state=x0, skip_missing=True, want_gauss_newton=True, **kw)
    with pytest.raises(TypeError):
        oc.pdp_vjp_batch(u, th, dx, du, ini_state=x0, skip_missing=True)


def test_for_irl_refuses_a_nan_initial_state_before_any_launch():
    from pdp_amd import runtime
    from pdp_amd.irl import LMLoop
    mdl = runtime.ModelLib.__new__(runtime.ModelLib)
    mdl.n, mdl.m, mdl.p, mdl.lib = 4, 1, 7, _NoForeignCalls()
    B, T = 2, 5
    demo_x, demo_u = np.full((B, T + 1, 4), np.nan), np.full((B, T, 1), np.nan)
    demo_x[:, 5, :2] = 0.25
    with pytest.raises(ValueError, match="ini_state"):                      # demo_x[:, 0] is all NaN and would be the initial state
        LMLoop.for_irl(mdl, demo_x, demo_u, np.ones(7), skip_missing=True)
    bad = np.zeros((B, 4))
    bad[1, 2] = np.nan
    with pytest.raises(ValueError, match="ini_state"):                      # ... and so is a NaN in the initial state that was given
        LMLoop.for_irl(mdl, demo_x, demo_u, np.ones(7), ini_state=bad, skip_missing=True)
    demo_x[:, 0] = 0.0
    demo_x[0, 0, 3] = np.nan                                                # one component is enough
    with pytest.raises(ValueError, match="ini_state"):
        LMLoop.for_irl(mdl, demo_x, demo_u, np.ones(7), skip_missing=True)


def test_example_masks_what_is_not_observed():
    """examples/irl_pdp.py mask_demos: --every K, --observe i,j, --no-controls -> NaN everywhere else (the cart-pole data of examples/oc_layer_custom_loss.py)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("irl_pdp_example", os.path.join(ROOT, "examples", "irl_pdp.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    rng = np.random.default_rng(0)
    dx, du = rng.standard_normal((5, 31, 4)), rng.standard_normal((5, 30, 1))
    mx, mu = ex.mask_demos(dx, du, every=10, observe=[0, 1], no_controls=True)
    assert np.isnan(mu).all() and (~np.isnan(mx)).sum() == 5 * 3 * 2
    for t in (10, 20, 30):
        assert np.array_equal(mx[:, t, :2], dx[:, t, :2]) and np.isnan(mx[:, t, 2:]).all()
    mx, mu = ex.mask_demos(dx, du)
    assert np.array_equal(mx, dx) and np.array_equal(mu, du)
