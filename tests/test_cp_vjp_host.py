"""CPU (no GPU needed): the ControlPlanning adjoint layer - the bit PDP_POLICY_COTANGENT and the struct pdp_policy_cot in abi.py and in the header, no entry point
added, the C refusals of the built model library with untouched outputs, the shape refusals of the runtime before any foreign call, the rows rule restated in
ModelLib.cp_vjp_rows, and the mathematics: the kernel's recursion in numpy (cp_vjp_common.adjoint_sweep) against the reference's forward sensitivities on every case
the GPU tests use (1e-11), and the reference against central differences through ControlPlanningOracle.integrateSys (2e-4, met with a margin of at least 10 x)."""
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


def test_the_bit_and_the_struct_mirror_the_header_and_no_entry_point_was_added():
    from pdp_amd import abi, runtime
    assert abi.PDP_POLICY_COTANGENT == 256
    assert not abi.PDP_POLICY_COTANGENT & (abi.PDP_POLICY_POLY | abi.PDP_POLICY_MLP | abi.PDP_POLICY_TABLE)
    src = open(os.path.join(ROOT, "include", "pdp_hip.h")).read()
    assert re.search(r"^#define PDP_POLICY_COTANGENT 256\b", src, flags=re.M)
    body = re.search(r"typedef struct pdp_policy_cot \{(.*?)\} pdp_policy_cot;", re.sub(r"/\*.*?\*/", "", src, flags=re.S), flags=re.S).group(1)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    assert decls == ["pdp_policy pol", "const double* x", "const double* grad_x", "const double* grad_u", "double* grad_x0"]
    assert [f[0] for f in abi.PdpPolicyCot._fields_] == ["pol", "x", "grad_x", "grad_u", "grad_x0"]
    assert abi.PdpPolicyCot._fields_[0][1] is abi.PdpPolicy                                   # by value, first: a pdp_policy_cot* is a pdp_policy*
    assert all(t is C.c_void_p for _, t in abi.PdpPolicyCot._fields_[1:])
    assert abi.PdpPolicyCot.pol.offset == 0 and C.sizeof(abi.PdpPolicyCot) == C.sizeof(abi.PdpPolicy) + 4 * C.sizeof(C.c_void_p)
    assert runtime.PdpPolicyCot is abi.PdpPolicyCot
    assert len(abi.entry_points()) == 45
    assert sorted(os.listdir(os.path.join(ROOT, "include"))) == sorted(abi.ENTRY_POINTS)        # no header added either


@pytest.fixture(scope="module")
def libs():
    import __graft_entry__ as g
    g.build()
    from pdp_amd import codegen, runtime, zoo
    load = lambda system, mode: runtime.load_model(codegen.build_problem(zoo.make_problem(system, mode))[0])
    return dict(cp=load("cartpole", "oc"), oc=load("cartpole", "irl"), sysid=load("cartpole", "sysid"))


def _cot(rt, pol, x, gx, gu, gx0, bit=True):
    cot = rt.PdpPolicyCot()
    C.memmove(C.byref(cot.pol), C.byref(pol), C.sizeof(rt.PdpPolicy))
    cot.pol.kind = pol.kind | (rt.PDP_POLICY_COTANGENT if bit else 0)
    addr = lambda a: None if a is None else a.ctypes.data
    cot.x, cot.grad_x, cot.grad_u, cot.grad_x0 = addr(x), addr(gx), addr(gu), addr(gx0)
    return cot


def test_the_c_refusals_come_before_any_launch_and_leave_the_outputs_untouched(libs):
    """host memory stands in for device memory: a refused call never reads or writes it"""
    from pdp_amd import abi, runtime as rt
    cp = libs["cp"]
    n, m, B, T = cp.n, cp.m, 3, 6
    assert (n, m) == (4, 1)
    pol = rt.make_policy("mlp", layers=[5, 1])
    p = 5 * 4 + 5 + 5 + 1
    x, gx, gu, th = np.ones((B, T + 1, n)), np.ones((B, T + 1, n)), np.ones((B, T, m)), np.ones(p)
    grad, gx0, other = np.full((B, p), 7.5), np.full((B, n), 7.5), np.full((B, T + 1, n), 7.5)
    A = lambda a: None if a is None else C.c_void_p(a.ctypes.data)

    def call(lib, cot, p=p, theta=th, loss=None, grad=grad, xo=None, uo=None, B=B, T=T):
        return lib.pdp_cp_step_batched(B, T, C.cast(C.byref(cot), C.POINTER(rt.PdpPolicy)), p, None, A(theta), 0, A(loss), A(grad), A(xo), A(uo), None, 0, None)
    ok = lambda **kw: _cot(rt, pol, **dict(dict(x=x, gx=gx, gu=gu, gx0=gx0), **kw))
    E_ARG, E_SIZE, E_MODE = abi.PDP_E_ARG, abi.PDP_E_SIZE, abi.PDP_E_MODE
    # PDP_E_ARG: loss, x, u of the call must be NULL; an output; the struct's inputs; theta; B, T
    assert call(cp.lib, ok(), loss=other) == E_ARG and call(cp.lib, ok(), xo=other) == E_ARG and call(cp.lib, ok(), uo=other) == E_ARG
    assert call(cp.lib, ok(gx0=None), grad=None) == E_ARG
    assert call(cp.lib, ok(x=None)) == E_ARG and call(cp.lib, ok(gx=None)) == E_ARG and call(cp.lib, ok(gu=None)) == E_ARG
    assert call(cp.lib, ok(), theta=None) == E_ARG and call(cp.lib, ok(), B=0) == E_ARG and call(cp.lib, ok(), T=0) == E_ARG
    assert call(cp.lib, ok(), p=p + 1) == E_ARG                                               # the parameter vector has not the network's length
    poly17 = _cot(rt, rt.make_policy("poly", pivots=np.linspace(0, T, 3)), x, gx, gu, gx0)
    assert call(cp.lib, poly17, p=4) == E_ARG                                                 # p != pivots * m
    # PDP_E_SIZE: beyond the limits of the sweep - the caller takes the materialised route
    wide = _cot(rt, rt.make_policy("mlp", layers=[33, 1]), x, gx, gu, gx0)
    assert call(cp.lib, wide, p=33 * 4 + 33 + 33 + 1) == E_SIZE
    deep = _cot(rt, rt.make_policy("mlp", layers=[2] * 8 + [1]), x, gx, gu, gx0)
    assert call(cp.lib, deep, p=2 * 4 + 2 + 7 * 6 + 3) == E_SIZE
    big = _cot(rt, rt.make_policy("mlp", layers=[32, 32, 1]), x, gx, gu, gx0)
    assert 32 * 4 + 32 + 32 * 32 + 32 + 33 > 512 and call(cp.lib, big, p=32 * 4 + 32 + 32 * 32 + 32 + 33) == E_SIZE
    table = rt.PdpPolicy()
    table.kind, table.n_basis, table.table = abi.PDP_POLICY_TABLE, 3, other.ctypes.data
    assert call(cp.lib, _cot(rt, table, x, gx, gu, gx0), p=3) == E_SIZE
    # PDP_E_MODE: not a ControlPlanning model
    assert call(libs["oc"].lib, ok()) == E_MODE and call(libs["sysid"].lib, ok()) == E_MODE
    # the other ControlPlanning entry points refuse the bit
    c = ok()
    pp = C.cast(C.byref(c), C.POINTER(rt.PdpPolicy))
    assert cp.lib.pdp_cp_integrate_batched(B, T, pp, p, A(other), A(th), 0, A(other), A(other), A(other), None) == E_ARG
    assert cp.lib.pdp_cp_auxsys_batched(B, T, pp, p, A(x), A(gu), A(th), 0, A(other), A(other), A(other), A(other), None, None, None, None) == E_ARG
    assert cp.lib.pdp_cp_step_workspace_bytes(1024, 100, pp, p) == 0
    assert libs["oc"].lib.pdp_cp_integrate_batched(B, T, pp, p, A(other), A(th), 0, A(other), A(other), A(other), None) == E_MODE
    # ... and without the bit the workspace query is the one it was
    plain = _cot(rt, rt.make_policy("mlp", layers=[4, 4, 1]), x, gx, gu, gx0, bit=False)
    assert cp.lib.pdp_cp_step_workspace_bytes(1024, 100, C.byref(plain.pol), 4 * 4 + 4 + 4 * 4 + 4 + 4 + 1) > 0
    assert (grad == 7.5).all() and (gx0 == 7.5).all() and (other == 7.5).all() and (x == 1).all() and (gx == 1).all() and (gu == 1).all()


class _NoForeignCalls:
    def __getattr__(self, name):
        raise AssertionError("foreign call %s before the arguments were validated" % name)


def test_shape_errors_are_value_errors_before_any_foreign_call():
    from pdp_amd import runtime as rt
    mdl = rt.ModelLib.__new__(rt.ModelLib)
    mdl.n, mdl.m, mdl.p, mdl.lib = 4, 1, 0, _NoForeignCalls()
    pol, p, B, T = rt.make_policy("mlp", layers=[5, 1]), 31, 3, 6
    x, gx, gu, th = np.zeros((B, T + 1, 4)), np.zeros((B, T + 1, 4)), np.zeros((B, T, 1)), np.zeros(p)
    for bad, match in ((dict(x=np.zeros((B, T + 1, 3))), "state_traj"), (dict(x=np.zeros((B, 1, 4))), "state_traj"), (dict(x=np.zeros((T + 1, 4))), "state_traj"),
                       (dict(grad_x=np.zeros((B, T, 4))), "grad_state"), (dict(grad_u=np.zeros((B, T + 1, 1))), "grad_control"),
                       (dict(grad_u=np.zeros((B, T, 2))), "grad_control"), (dict(theta=np.zeros(p + 1)), "theta"), (dict(theta=np.zeros((2, p))), "theta"),
                       (dict(want_theta=False, want_ini=False), "nothing to compute")):
        kw = dict(dict(x=x, theta=th, grad_x=gx, grad_u=gu), **bad)
        with pytest.raises(ValueError, match=match):
            mdl.cp_rollout_vjp(pol, p, **kw)


def test_rows_rule_of_the_zoo_models_and_of_the_edge_models():
    import cp_edge_common as ce
    import cp_vjp_common as cv
    from pdp_amd import codegen, runtime, zoo
    for system, rows in cv.ZOO_ROWS.items():
        info = codegen.generate(zoo.make_problem(system, "oc"))[1]
        mdl = runtime.ModelLib.__new__(runtime.ModelLib)
        mdl.name, mdl.n, mdl.m = info["name"], info["n"], info["m"]
        assert mdl.cp_vjp_rows() == rows, system
    for name in ce.NAMES:
        info = codegen.write_header(ce.problem(name))[1]
        mdl = runtime.ModelLib.__new__(runtime.ModelLib)
        mdl.name, mdl.n, mdl.m = info["name"], info["n"], info["m"]
        stride = (info["nvar"]["path"] + info["n"] + info["m"] + max(info["n"] + info["m"], 16)) | 1
        assert mdl.cp_vjp_rows() == cv.ROWS[name] == min(64, max(4, 2400 // stride)), name
    # the header of the sweep kernels' pool states the same rule, and the host launches with it
    src = open(os.path.join(codegen.CSRC, "pdp_sweep_pool.h")).read()
    assert "struct CpVjpPool : SweepPool<Mdl::PATH_NVAR, Mdl::PATH_NCONST, Mdl::NX + Mdl::NU + (Mdl::NX + Mdl::NU > 16 ? Mdl::NX + Mdl::NU : 16)> {" in src
    assert "static constexpr int STRIDE = (NVAR + TAIL) | 1;" in src and "constexpr int SWEEP_POOL_DOUBLES = 2400;" in src
    assert "constexpr int rows = oc_x0_vjp_rows_of(CpVjpPool<Mdl>::STRIDE);" in open(os.path.join(codegen.CSRC, "pdp_model.hip")).read()
    assert runtime.SWEEP_POOL_DOUBLES == 2400


@pytest.mark.parametrize("case", __import__("cp_vjp_common").all_cases(), ids=__import__("cp_vjp_common").case_id)
def test_adjoint_sweep_equals_the_references_forward_sensitivities(case):
    """the kernel's recursion (numpy) against integrateAuxSys from X_0 = [0 | I] contracted with the cotangents, per parameter block and for grad_x0: 1e-11, a tenth
    of the GPU tolerance - the reference's own error on these inputs is then below what the GPU tests ask.  Samples 0 and 4, shared and per-sample theta."""
    import cp_vjp_common as cv
    name, kind, key, T = case
    gx, gu = cv.cotangents(name, T)
    worst = 0.0
    for per_sample, b in ((False, 0), (True, 4)):
        r = cv.reference(name, kind, key, T, per_sample, b)
        assert np.isfinite(r["grad_theta"]).all() and np.abs(r["grad_theta"]).max() > 0 and np.abs(r["grad_x0"]).max() > 0
        g, mu = cv.adjoint_sweep(r["aux"], gx[b], gu[b])
        worst = max(worst, cv.grad_rel(name, kind, key, g, r["grad_theta"]), cv.x0_rel(mu, r["grad_x0"]))
    print("adjoint sweep vs reference, %s: %.3e" % (cv.case_id(case), worst))
    assert worst <= cv.HOST_TOL, (case, worst)


@pytest.mark.parametrize("kind,key", [("poly", 6), ("mlp", (6, 1))], ids=["lagrange", "mlp_6x1"])
def test_reference_equals_central_differences_through_the_oracles_rollout(kind, key):
    """L = sum gx . x + sum gu . u of ControlPlanningOracle.integrateSys at theta +- h e_k and x_0 +- h e_k (h = 1e-5) against the reference's dL/dtheta and dL/dx_0 on
    C5, T = 12: 2e-4 of the largest derivative, and met with a margin of at least 10 x"""
    import cp_edge_common as ce
    import cp_vjp_common as cv
    name, T, h = "C5", 12, 1e-5
    orc = cv.oracle_for(name, kind, key, T)
    inp = ce.inputs(name, kind, key, T)
    x0, theta = inp["x0"][1], inp["theta"]
    gx, gu = (a[1] for a in cv.cotangents(name, T))
    r = cv.reference_at(orc, x0, T, theta, gx, gu)

    def loss(x0_, th_):
        sol = orc.integrateSys(x0_, T, th_)
        return float((gx * sol["state_traj"]).sum() + (gu * sol["control_traj"]).sum())
    fd_th = np.array([(loss(x0, theta + h * e) - loss(x0, theta - h * e)) / (2 * h) for e in np.eye(len(theta))])
    fd_x0 = np.array([(loss(x0 + h * e, theta) - loss(x0 - h * e, theta)) / (2 * h) for e in np.eye(len(x0))])
    e_th, e_x0 = np.abs(fd_th - r["grad_theta"]).max() / np.abs(fd_th).max(), np.abs(fd_x0 - r["grad_x0"]).max() / np.abs(fd_x0).max()
    print("reference vs central differences, C5 %s: theta %.3e, x0 %.3e" % (kind, e_th, e_x0))
    assert max(e_th, e_x0) <= cv.FD_TOL / 10, (e_th, e_x0)
