"""CPU (no GPU needed): pdp_sysid_rollout_vjp_batched - the SysID rollout as a vector-Jacobian product - at the ABI (the header, the binding's lists, the argument
errors before any launch), the shape errors of the class surface, and the reference of tests/sysid_vjp_common.py against central differences of the oracle's rollout and
against the kernel's own recursion restated in numpy."""
import ctypes as C
import os

import numpy as np
import pytest

import sysid_vjp_common as sv

ROOT = sv.ROOT
NAME = "pdp_sysid_rollout_vjp_batched"


def _built():
    import __graft_entry__ as g
    g.build()
    from pdp_amd import codegen, runtime as rt, zoo
    return codegen, rt, zoo


def test_the_entry_point_is_declared_listed_and_exported():
    """(tests/test_abi_table.py holds the whole binding against the headers and the built libraries; what stays here is this entry point's own line)"""
    from pdp_amd import abi
    (name, (restype, argtypes)), = abi.entry_points("pdp_hip_sysid_vjp.h", "model").items()
    assert name == NAME and restype is C.c_int and len(argtypes) == 10


def test_argument_errors_are_returned_before_any_launch():
    """valid (host) pointers everywhere, so that only the argument under test can be what is refused; nothing that passes the checks is called: no GPU here"""
    codegen, rt, zoo = _built()
    mdl = rt.load_model(codegen.build_problem(zoo.make_problem("quadrotor", "sysid"))[0])
    assert mdl.p == 5
    keep = [(C.c_double * 8)() for _ in range(6)]
    x, u, th, g, gt, g0 = (C.cast(k, C.c_void_p) for k in keep)
    fn = getattr(mdl.lib, NAME)
    ok = dict(B=1, T=4, x=x, u=u, th=th, tb=0, g=g, gt=gt, g0=g0)

    def call(lib_fn=fn, **kw):
        a = dict(ok, **kw)
        return lib_fn(a["B"], a["T"], a["x"], a["u"], a["th"], a["tb"], a["g"], a["gt"], a["g0"], None)
    for kw in (dict(B=0), dict(B=-3), dict(T=0), dict(T=-2), dict(x=None), dict(u=None), dict(th=None), dict(g=None), dict(gt=None, g0=None), dict(tb=4), dict(tb=1),
               dict(tb=-5)):
        assert call(**kw) == -1, kw                                               # PDP_E_ARG
    assert all(v == 0.0 for k in keep for v in k)
    oc = rt.load_model(codegen.build_problem(zoo.make_problem("cartpole", "irl"))[0])
    assert call(getattr(oc.lib, NAME)) == -4 and call(getattr(oc.lib, NAME), tb=oc.p) == -4 and call(getattr(oc.lib, NAME), g0=None) == -4      # PDP_E_MODE
    assert call(getattr(oc.lib, NAME), B=0) == -1                                 # the argument check comes first


def test_the_size_limit_is_a_compile_time_condition_of_the_host_routine():
    """PDP_E_SIZE for n > 64 or p > 512: a model of that size takes far longer to build than a test may, so the condition is read where it is decided"""
    src = open(os.path.join(ROOT, "pontryagin-differentiable-programming_amd", "csrc", "pdp_model.hip")).read()
    def body_of(head):
        body = src[src.index(head):]
        return body[:body.index("\n}\n")]
    # the routine: its argument check, then the plan of the sweep launches with the limit as a compile-time argument, then the launch
    body = body_of("int sysid_rollout_vjp(")
    assert "sweep_plan<Mdl, SysidVjpPool, sweep_fits_p<Mdl>>(B)" in body
    assert "template <class Mdl> constexpr bool sweep_fits_p = Mdl::NX <= 64 && Mdl::NP <= 512;" in src
    assert body.index("return PDP_E_ARG") < body.index("sweep_plan<") < body.index("if constexpr (!pl.ok) return pl.rows;") < body.index("launch(")
    # the plan: the model kind, then the limit, both compile-time conditions, then the bound on the block
    plan = body_of("auto sweep_plan(int B)")
    assert "else if constexpr (!FITS) return SweepPlan<false>{PDP_E_SIZE, 0};" in plan
    assert plan.index("PDP_E_MODE") < plan.index("if constexpr (!FITS)") < plan.index("150 * 1024") and "PDP_E_ARG" not in plan
    assert "n > 64 or p > 512" in open(os.path.join(ROOT, "include", "pdp_hip_sysid_vjp.h")).read()


def test_shape_errors_are_value_errors_before_any_launch(monkeypatch):
    """no GPU: the library is a recorder that must stay empty"""
    import sysid_ini_common as si
    from pdp_amd import PDP, runtime
    mdl = runtime.ModelLib.__new__(runtime.ModelLib)
    mdl.n, mdl.m, mdl.p, mdl.chunk, mdl.nnz_path, mdl.lib = 4, 1, 3, 32, 10, si.Recorder()
    sid = PDP.SysID.__new__(PDP.SysID)
    sid.n_state, sid.n_control, sid.n_auxvar, sid._model = 4, 1, 3, mdl
    B, T = 3, 6
    x, u, th, g = np.zeros((B, T + 1, 4)), np.zeros((B, T, 1)), np.ones(3), np.zeros((B, T + 1, 4))
    bad = [dict(state_traj=x[:, :-1]), dict(state_traj=x[:2]), dict(inputs=u[0]), dict(inputs=np.zeros((B, T, 2))), dict(inputs=np.zeros((B, 0, 1))),
           dict(grad_state=g[:, :, :3]), dict(grad_state=g[:, 1:]), dict(auxvar_value=np.ones(4)), dict(auxvar_value=np.ones((2, 3))), dict(auxvar_value=np.ones((3, 3, 1)))]
    for kw in bad:
        a = dict(dict(state_traj=x, inputs=u, auxvar_value=th, grad_state=g), **kw)
        with pytest.raises(ValueError, match="sysid_rollout_vjp"):
            sid.rollout_vjp_batch(a["state_traj"], a["inputs"], a["auxvar_value"], a["grad_state"])
    with pytest.raises(ValueError, match="nothing to compute"):
        mdl.sysid_rollout_vjp(x, u, th, g, want_ini=False, want_theta=False)
    for kw in (dict(ini_state=np.zeros((B, 3))), dict(ini_state=np.zeros(4)), dict(inputs=np.zeros((B, T))), dict(inputs=np.zeros((B, T, 3))),
               dict(auxvar_value=np.ones(2)), dict(auxvar_value=np.ones((B + 1, 3)))):
        a = dict(dict(ini_state=np.zeros((B, 4)), inputs=u, auxvar_value=th), **kw)
        with pytest.raises(ValueError, match="integrateDyn_batch"):
            sid.integrateDyn_batch(a["ini_state"], a["inputs"], a["auxvar_value"])
    assert mdl.lib.calls == []
    assert mdl.sysid_vjp_rows(1, 256) == 32 and mdl.sysid_vjp_rows(1024, 256) == 32 and mdl.sysid_vjp_rows(1025, 256) == 32       # stride 15: 160 rows would fit
    mdl.nnz_path, mdl.n = 200, 40                                                                                                # stride 241: nine rows beyond 4 per CU
    assert mdl.sysid_vjp_rows(1024, 256) == 32 and mdl.sysid_vjp_rows(1025, 256) == 9
    mdl.nnz_path = 700                                                                                                           # not even four rows: the chunk stays
    assert mdl.sysid_vjp_rows(1025, 256) == 32


def test_the_layer_refuses_what_it_cannot_differentiate():
    import torch
    from pdp_amd import autograd

    class Sid:
        n_auxvar = 3
    with pytest.raises(TypeError, match="CUDA fp64"):
        autograd.sysid_trajectory(Sid(), np.zeros((2, 4)), np.zeros((2, 5, 1)), torch.ones(3, dtype=torch.float64, requires_grad=True))
    with pytest.raises(TypeError, match="CUDA fp64"):
        autograd.sysid_trajectory(Sid(), np.zeros((2, 4)), np.zeros((2, 5, 1)), np.ones(3))
    doc = autograd.__doc__
    assert "sysid_trajectory" in doc and "Limits" in doc and "oc_trajectory: no gradient with respect to ini_state" in doc


@pytest.mark.parametrize("system", sv.SYSTEMS)
def test_reference_agrees_with_central_differences_of_the_oracle_rollout(system):
    """L = sum g . x(theta, x0) is linear in the rollout, so its derivative is the reference's contraction: central differences with h = 1e-6 (truncation h^2, rounding
    eps / h ~ 1e-10) within 1e-6 of the largest entry, stored data, sample 0, shared and perturbed parameters"""
    c = sv.case(system)
    sid, b, h = c["sid"], 0, 1e-6
    for th, gt, g0 in ((c["theta"], c["grad_theta"][b], c["grad_x0"][b]), (c["theta_b"][b], c["grad_theta_b"][b], c["grad_x0_b"][b])):
        L = lambda v: float((c["g"][b] * sid.integrateDyn(v[sid.p:], c["inputs"][b], v[:sid.p])).sum())
        v0 = np.concatenate([th, c["x0"][b]])
        fd = np.array([(L(v0 + h * e) - L(v0 - h * e)) / (2 * h) for e in np.eye(v0.size)])
        et = np.abs(fd[:sid.p] - gt).max() / np.abs(gt).max()
        e0 = np.abs(fd[sid.p:] - g0).max() / np.abs(g0).max()
        print("%s: central differences vs the reference: grad_theta %.2e  grad_x0 %.2e" % (system, et, e0))
        assert et <= 1e-6 and e0 <= 1e-6


@pytest.mark.parametrize("system", sv.SYSTEMS)
def test_reference_agrees_with_the_adjoint_recursion_in_numpy(system):
    """forward sensitivities against the costate sweep, both in numpy, at the chunk-edge horizons (65 / 33): the two orders of the same sums differ by rounding alone -
    1e-13 of the largest entry is three digits inside the GPU tests' 1e-10, and above the rounding of sums of at most 66 x 13 products of entries up to a few hundred
    times the result (the two are seen to differ by 7e-16 .. 4e-15)"""
    c = sv.case(system, sv.EDGE_T[system])
    worst = 0.0
    for b in range(c["inputs"].shape[0]):
        gt, g0 = sv.adjoint_sweep(c["sid"], c["states"][b], c["inputs"][b], c["theta"], c["g"][b])
        worst = max(worst, np.abs(gt - c["grad_theta"][b]).max() / np.abs(gt).max(), np.abs(g0 - c["grad_x0"][b]).max() / np.abs(g0).max())
    print("%s T = %d: forward sensitivities vs adjoint sweep %.2e" % (system, sv.EDGE_T[system], worst))
    assert worst <= 1e-13
