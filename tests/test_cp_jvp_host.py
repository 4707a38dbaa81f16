"""CPU (no GPU needed): the ControlPlanning tangent layer - the bit PDP_POLICY_TANGENT and the struct pdp_policy_tan in abi.py and in the header, no entry point and
no header added, the C refusals of the built model library with untouched outputs, the shape refusals of the runtime before any foreign call, the rows rule restated in
ModelLib.cp_jvp_rows, the registers of cp_jvp_kernel, the Python layers (ModelLib.cp_rollout_jvp, ControlPlanning.rollout_jvp_batch, the autograd layer's jvp,
MatrixFreeLM.for_cp) against stand-ins, and the mathematics: the kernel's recursion in numpy (cp_jvp_common.tangent_sweep) against the reference's forward
sensitivities contracted with the direction on every case the GPU tests use (1e-11), the reference against central differences through
ControlPlanningOracle.integrateSys (2e-4), and MatrixFreeLM's schedule restated in numpy on the problem of the GPU loop."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import cp_edge_common as ce  # noqa: E402
import cp_jvp_common as cj  # noqa: E402
import cp_vjp_common as cv  # noqa: E402

TAN_FIELDS = ["pol", "x", "u", "d_theta", "d_theta_bstride", "d_x0", "d_x", "d_u"]


def test_the_bit_and_the_struct_mirror_the_header_and_no_entry_point_was_added():
    from pdp_amd import abi, runtime
    assert abi.PDP_POLICY_TANGENT == 512 == runtime.PDP_POLICY_TANGENT
    assert not abi.PDP_POLICY_TANGENT & (abi.PDP_POLICY_POLY | abi.PDP_POLICY_MLP | abi.PDP_POLICY_TABLE | abi.PDP_POLICY_COTANGENT)
    src = open(os.path.join(ROOT, "include", "pdp_hip.h")).read()
    assert re.search(r"^#define PDP_POLICY_TANGENT 512\b", src, flags=re.M)
    body = re.search(r"typedef struct pdp_policy_tan \{(.*?)\} pdp_policy_tan;", re.sub(r"/\*.*?\*/", "", src, flags=re.S), flags=re.S).group(1)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    assert decls == ["pdp_policy pol", "const double* x", "const double* u", "const double* d_theta", "int d_theta_bstride", "const double* d_x0", "double* d_x",
                     "double* d_u"]
    assert [f[0] for f in abi.PdpPolicyTan._fields_] == TAN_FIELDS
    assert abi.PdpPolicyTan._fields_[0][1] is abi.PdpPolicy                                   # by value, first: a pdp_policy_tan* is a pdp_policy*
    assert [t for _, t in abi.PdpPolicyTan._fields_[1:]] == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    assert abi.PdpPolicyTan.pol.offset == 0 and C.sizeof(abi.PdpPolicyTan) == C.sizeof(abi.PdpPolicy) + 7 * C.sizeof(C.c_void_p)      # (the int is padded to a pointer)
    assert runtime.PdpPolicyTan is abi.PdpPolicyTan
    assert len(abi.entry_points()) == 45
    assert sorted(os.listdir(os.path.join(ROOT, "include"))) == sorted(abi.ENTRY_POINTS)        # no header added either
    assert [f[0] for f in abi.PdpPolicyCot._fields_] == ["pol", "x", "grad_x", "grad_u", "grad_x0"]      # ... and the cotangent struct is the one it was


@pytest.fixture(scope="module")
def libs():
    import __graft_entry__ as g
    g.build()
    from pdp_amd import codegen, runtime, zoo
    load = lambda system, mode: runtime.load_model(codegen.build_problem(zoo.make_problem(system, mode))[0])
    return dict(cp=load("cartpole", "oc"), oc=load("cartpole", "irl"), sysid=load("cartpole", "sysid"))


def _tan(rt, pol, x, u, dth, dx0, dx, du, stride=0, bits=None):
    tan = rt.PdpPolicyTan()
    C.memmove(C.byref(tan.pol), C.byref(pol), C.sizeof(rt.PdpPolicy))
    tan.pol.kind = pol.kind | (rt.PDP_POLICY_TANGENT if bits is None else bits)
    addr = lambda a: None if a is None else a.ctypes.data
    tan.x, tan.u, tan.d_theta, tan.d_theta_bstride, tan.d_x0, tan.d_x, tan.d_u = addr(x), addr(u), addr(dth), stride, addr(dx0), addr(dx), addr(du)
    return tan


def test_the_c_refusals_come_before_any_launch_and_leave_the_outputs_untouched(libs):
    """host memory stands in for device memory: a refused call never reads or writes it"""
    from pdp_amd import abi, runtime as rt
    cp = libs["cp"]
    n, m, B, T = cp.n, cp.m, 3, 6
    assert (n, m) == (4, 1)
    pol = rt.make_policy("mlp", layers=[5, 1])
    p = 5 * 4 + 5 + 5 + 1
    x, u, th, dth, dx0 = np.ones((B, T + 1, n)), np.ones((B, T, m)), np.ones(p), np.ones(p), np.ones((B, n))
    dx, du, other = np.full((B, T + 1, n), 7.5), np.full((B, T, m), 7.5), np.full((B, max(p, (T + 1) * n)), 7.5)
    A = lambda a: None if a is None else C.c_void_p(a.ctypes.data)

    def call(lib, tan, p=p, theta=th, loss=None, grad=None, xo=None, uo=None, B=B, T=T):
        return lib.pdp_cp_step_batched(B, T, C.cast(C.byref(tan), C.POINTER(rt.PdpPolicy)), p, None, A(theta), 0, A(loss), A(grad), A(xo), A(uo), None, 0, None)
    ok = lambda pol=pol, **kw: _tan(rt, pol, **dict(dict(x=x, u=u, dth=dth, dx0=dx0, dx=dx, du=du), **kw))
    E_ARG, E_SIZE, E_MODE = abi.PDP_E_ARG, abi.PDP_E_SIZE, abi.PDP_E_MODE
    # PDP_E_ARG: loss, grad, x, u of the call must be NULL; the struct's rollout and output; no tangent at all; both bits; theta; B, T; the stride
    for kw in (dict(loss=other), dict(grad=other), dict(xo=other), dict(uo=other), dict(theta=None), dict(B=0), dict(T=0), dict(p=p + 1)):
        assert call(cp.lib, ok(), **kw) == E_ARG, kw
    for kw in (dict(x=None), dict(u=None), dict(dx=None), dict(dth=None, dx0=None), dict(dth=None, dx0=None, du=None), dict(stride=3), dict(stride=-p),
               dict(bits=abi.PDP_POLICY_TANGENT | abi.PDP_POLICY_COTANGENT)):
        assert call(cp.lib, ok(**kw)) == E_ARG, kw
    assert call(cp.lib, ok(rt.make_policy("poly", pivots=np.linspace(0, T, 3))), p=4) == E_ARG                      # p != pivots * m
    assert call(cp.lib, ok(rt.make_policy("mlp", layers=[5, 2])), p=5 * 4 + 5 + 2 * 5 + 2) == E_ARG                  # the network's output is not m wide
    # PDP_E_SIZE: beyond the limits of the sweep - the caller takes the materialised route
    assert call(cp.lib, ok(rt.make_policy("mlp", layers=[33, 1])), p=33 * 4 + 33 + 33 + 1) == E_SIZE
    assert call(cp.lib, ok(rt.make_policy("mlp", layers=[2] * 8 + [1])), p=2 * 4 + 2 + 7 * 6 + 3) == E_SIZE
    assert 32 * 4 + 32 + 32 * 32 + 32 + 33 > 512 and call(cp.lib, ok(rt.make_policy("mlp", layers=[32, 32, 1])), p=32 * 4 + 32 + 32 * 32 + 32 + 33) == E_SIZE
    table = rt.PdpPolicy()
    table.kind, table.n_basis, table.table = abi.PDP_POLICY_TABLE, 3, other.ctypes.data
    assert call(cp.lib, ok(table), p=3) == E_SIZE
    # PDP_E_MODE: not a ControlPlanning model
    assert call(libs["oc"].lib, ok()) == E_MODE and call(libs["sysid"].lib, ok()) == E_MODE
    # the other ControlPlanning entry points refuse the bit exactly as they refuse PDP_POLICY_COTANGENT
    t = ok()
    pp = C.cast(C.byref(t), C.POINTER(rt.PdpPolicy))
    assert cp.lib.pdp_cp_integrate_batched(B, T, pp, p, A(other), A(th), 0, A(other), A(other), A(other), None) == E_ARG
    assert cp.lib.pdp_cp_auxsys_batched(B, T, pp, p, A(x), A(u), A(th), 0, A(other), A(other), A(other), A(other), None, None, None, None) == E_ARG
    assert cp.lib.pdp_cp_step_workspace_bytes(1024, 100, pp, p) == 0
    assert libs["oc"].lib.pdp_cp_integrate_batched(B, T, pp, p, A(other), A(th), 0, A(other), A(other), A(other), None) == E_MODE
    # ... and without the bit the workspace query is the one it was
    plain = ok(rt.make_policy("mlp", layers=[4, 4, 1]), bits=0)
    assert cp.lib.pdp_cp_step_workspace_bytes(1024, 100, C.byref(plain.pol), 4 * 4 + 4 + 4 * 4 + 4 + 4 + 1) > 0
    assert (dx == 7.5).all() and (du == 7.5).all() and (other == 7.5).all()
    assert all((a == 1).all() for a in (x, u, th, dth, dx0))


class _NoForeignCalls:
    def __getattr__(self, name):
        raise AssertionError("foreign call %s before the arguments were validated" % name)


def test_shape_errors_are_value_errors_before_any_foreign_call():
    from pdp_amd import runtime as rt
    mdl = rt.ModelLib.__new__(rt.ModelLib)
    mdl.n, mdl.m, mdl.p, mdl.lib = 4, 1, 0, _NoForeignCalls()
    pol, p, B, T = rt.make_policy("mlp", layers=[5, 1]), 31, 3, 6
    x, u, th = np.zeros((B, T + 1, 4)), np.zeros((B, T, 1)), np.zeros(p)
    for bad, match in ((dict(x=np.zeros((B, T + 1, 3))), "state_traj"), (dict(x=np.zeros((B, 1, 4))), "state_traj"), (dict(x=np.zeros((T + 1, 4))), "state_traj"),
                       (dict(u=np.zeros((B, T + 1, 1))), "control_traj"), (dict(u=np.zeros((B, T, 2))), "control_traj"), (dict(u=np.zeros((B, T))), "control_traj"),
                       (dict(theta=np.zeros(p + 1)), "theta"), (dict(theta=np.zeros((2, p))), "theta"), (dict(d_theta=np.zeros(p + 1)), "d_theta"),
                       (dict(d_theta=np.zeros((2, p))), "d_theta"), (dict(d_x0=np.zeros((B, 3))), "d_x0"), (dict(d_x0=np.zeros(4)), "d_x0"),
                       (dict(d_theta=None, d_x0=None), "nothing to compute")):
        kw = dict(dict(x=x, u=u, theta=th, d_theta=np.zeros(p), d_x0=np.zeros((B, 4))), **bad)
        with pytest.raises(ValueError, match=match):
            mdl.cp_rollout_jvp(pol, p, **kw)


def test_rows_rule_of_the_zoo_models_and_of_the_edge_models():
    """stride = (PATH_NVAR + n + m) | 1 by hand: cart-pole 11 + 4 + 1 -> 17, pendulum 4 + 2 + 1 -> 7, quadrotor 62 + 13 + 4 -> 79, robot arm 16 + 4 + 2 -> 23,
    rocket 65 + 13 + 3 -> 81; C16 28 + 16 + 4 -> 49, C15 26 + 15 + 3 -> 45, C5 10 + 5 + 1 -> 17; rows = 2400 // stride clamped to [4, 64]"""
    from pdp_amd import codegen, runtime, zoo
    by_hand = {"cartpole": 17, "pendulum": 7, "quadrotor": 79, "robotarm": 23, "rocket": 81, "C16": 49, "C15": 45, "C5": 17}
    for name, stride in by_hand.items():
        assert min(64, max(4, 2400 // stride)) == dict(cj.ZOO_ROWS, **cj.ROWS)[name], name
    for system, rows in cj.ZOO_ROWS.items():
        info = codegen.generate(zoo.make_problem(system, "oc"))[1]
        mdl = runtime.ModelLib.__new__(runtime.ModelLib)
        mdl.name, mdl.n, mdl.m = info["name"], info["n"], info["m"]
        assert (info["nvar"]["path"] + info["n"] + info["m"]) | 1 == by_hand[system], system
        assert mdl.cp_jvp_rows() == rows, system
    for name in ce.NAMES:
        info = codegen.write_header(ce.problem(name))[1]
        mdl = runtime.ModelLib.__new__(runtime.ModelLib)
        mdl.name, mdl.n, mdl.m = info["name"], info["n"], info["m"]
        assert (info["nvar"]["path"] + info["n"] + info["m"]) | 1 == by_hand[name], name
        assert mdl.cp_jvp_rows() == cj.ROWS[name], name
    # the header of the sweep kernels' pool states the same rule, and the host launches with it
    src = open(os.path.join(codegen.CSRC, "pdp_sweep_pool.h")).read()
    assert "struct CpJvpPool : SweepPool<Mdl::PATH_NVAR, Mdl::PATH_NCONST, Mdl::NX + Mdl::NU> {" in src
    assert "static constexpr int STRIDE = (NVAR + TAIL) | 1;" in src and "constexpr int SWEEP_POOL_DOUBLES = 2400;" in src
    assert "constexpr int rows = oc_x0_vjp_rows_of(CpJvpPool<Mdl>::STRIDE);" in open(os.path.join(codegen.CSRC, "pdp_model.hip")).read()


def _resources(lib):
    from pdp_amd import codegen
    k = codegen.kernel_resources(lib)
    assert [key for key in k if key.startswith("cp_jvp_kernel")] == ["cp_jvp_kernel"], sorted(k)
    return k["cp_jvp_kernel"]


@pytest.mark.parametrize("name", ce.NAMES)
def test_registers_of_the_edge_models_kernel(libs, name):
    """printed; no spill"""
    from pdp_amd import codegen
    r = _resources(codegen.build_problem(ce.problem(name))[0])
    print("%s: cp_jvp_kernel vgpr %d sgpr %d spill %d scratch %d" % (name, r["vgpr"], r["sgpr"], r["spill"], r["scratch"]))
    assert r["spill"] == 0, (name, r)


def test_zoo_kernels_do_not_spill_and_use_no_scratch(libs):
    """one cp_jvp_kernel in each of the five ControlPlanning libraries of the zoo, none in a library of another kind"""
    from pdp_amd import codegen, zoo
    for system in sorted(cj.ZOO_ROWS):
        r = _resources(codegen.build_problem(zoo.make_problem(system, "oc"))[0])
        print("%s: cp_jvp_kernel vgpr %d sgpr %d spill %d scratch %d" % (system, r["vgpr"], r["sgpr"], r["spill"], r["scratch"]))
        assert r["spill"] == 0 and r["scratch"] == 0, (system, r)
    for mode in ("irl", "sysid"):
        assert not [k for k in codegen.kernel_resources(codegen.build_problem(zoo.make_problem("cartpole", mode))[0]) if k.startswith("cp_jvp_kernel")]


# ---- the Python layers against stand-ins --------------------------------------------------------------------------------------------------------------------------
def _stand_ins(monkeypatch):
    import ls_rows_common as lr
    from pdp_amd import PDP, runtime
    lr.stand_in_torch(monkeypatch)
    monkeypatch.setattr(runtime, "ptr", lambda t: None if t is None else ("ptr", tuple(t.shape)))
    mdl = runtime.ModelLib.__new__(runtime.ModelLib)
    mdl.n, mdl.m, mdl.p, mdl.lib = 4, 1, 0, lr.Recorder()
    cp = PDP.ControlPlanning.__new__(PDP.ControlPlanning)
    cp.n_state, cp.n_control, cp.n_auxvar, cp._model, cp._policy = 4, 1, 31, mdl, runtime.make_policy("mlp", layers=[5, 1])
    return mdl, cp


def test_the_runtime_and_the_class_against_a_recorder_library(monkeypatch):
    """no GPU: the library records.  One call of pdp_cp_step_batched per jvp, its policy argument the head of a pdp_policy_tan with the bit set and the tensors' addresses;
    a None tangent is a NULL pointer; the stride of d_theta follows its shape; want_control=False is a NULL d_u"""
    from pdp_amd import abi
    mdl, cp = _stand_ins(monkeypatch)
    B, T, p = 3, 6, 31
    x, u, th = np.zeros((B, T + 1, 4)), np.zeros((B, T, 1)), np.ones(p)
    seen = []

    class Lib:                                                       # (the struct lives as long as the call: read it there)
        def pdp_cp_step_batched(self, *args):
            tan = C.cast(args[2], C.POINTER(abi.PdpPolicyTan)).contents
            seen.append(("pdp_cp_step_batched", args[:2] + args[3:], {f: getattr(tan, f) for f in TAN_FIELDS[1:]}, tan.pol.kind, tan.pol.n_layers,
                         list(tan.pol.sizes[:2])))
            return 0
    mdl.lib = Lib()
    import torch
    keep = dict(x=torch.zeros((B, T + 1, 4), dtype=torch.float64), u=torch.zeros((B, T, 1), dtype=torch.float64), dth=torch.ones(p, dtype=torch.float64),
                dthb=torch.ones((B, p), dtype=torch.float64), dx0=torch.ones((B, 4), dtype=torch.float64))
    outs = [cp.rollout_jvp_batch(keep["x"], keep["u"], th, d_auxvar=keep["dth"], d_ini_state=keep["dx0"]),
            cp.rollout_jvp_batch(keep["x"], keep["u"], th, d_auxvar=keep["dthb"]),
            mdl.cp_rollout_jvp(cp._policy, p, keep["x"], keep["u"], np.ones((B, p)), d_x0=keep["dx0"], want_control=False)]
    assert [s[0] for s in seen] == ["pdp_cp_step_batched"] * 3
    P = lambda *shape: ("ptr", shape)
    tail = lambda theta, tb: (p, None, theta, tb, None, None, None, None, None, 0, None)       # x0, loss, grad, x, u, workspace of the call: NULL
    assert seen[0][1] == (B, T) + tail(P(1, p), 0) and seen[1][1] == (B, T) + tail(P(1, p), 0) and seen[2][1] == (B, T) + tail(P(B, p), p)
    for s in seen:
        assert s[3] == abi.PDP_POLICY_MLP | abi.PDP_POLICY_TANGENT and s[4] == 2 and s[5] == [5, 1]
        assert s[2]["x"] == keep["x"].data_ptr() and s[2]["u"] == keep["u"].data_ptr()
    a, b, c = (s[2] for s in seen)
    assert (a["d_theta"], a["d_theta_bstride"], a["d_x0"]) == (keep["dth"].data_ptr(), 0, keep["dx0"].data_ptr())
    assert (b["d_theta"], b["d_theta_bstride"], b["d_x0"]) == (keep["dthb"].data_ptr(), p, None)
    assert (c["d_theta"], c["d_theta_bstride"], c["d_x0"]) == (None, 0, keep["dx0"].data_ptr())
    assert a["d_x"] == outs[0]["d_state"].data_ptr() and a["d_u"] == outs[0]["d_control"].data_ptr()
    assert c["d_x"] == outs[2]["d_state"].data_ptr() and c["d_u"] is None and sorted(outs[2]) == ["d_state"]
    assert tuple(outs[0]["d_state"].shape) == (B, T + 1, 4) and tuple(outs[0]["d_control"].shape) == (B, T, 1)
    assert cp._policy.kind == abi.PDP_POLICY_MLP                                             # the caller's policy keeps its kind


class _LinearCP:
    """a ControlPlanning stand-in in torch on the CPU: x+ = A x + Bm u with the open-loop policy u_t = theta[t m .. t m + m) - what the layer and the loop call, recorded"""
    n_state, n_control = 3, 2

    def __init__(self, T):
        import torch
        rng = np.random.default_rng(5)
        self.T, self.n_auxvar, self._policy, self.calls = T, 2 * T, object(), []
        self.A = torch.as_tensor(np.eye(3) + 0.1 * rng.standard_normal((3, 3)))
        self.Bm = torch.as_tensor(rng.standard_normal((3, 2)))

    def _roll(self, x0, u):
        import torch
        xs = [x0]
        for t in range(self.T):
            xs.append(xs[-1] @ self.A.T + u[:, t] @ self.Bm.T)
        return torch.stack(xs, dim=1)

    def _u(self, theta, B):
        return theta.reshape(-1, self.T, 2).expand(B, self.T, 2)

    def integrateSys_batch(self, x0, T, theta):
        self.calls.append("rollout")
        u = self._u(theta, x0.shape[0]).contiguous()
        return self._roll(x0, u), u, None

    def rollout_jvp_batch(self, x, u, theta, d_auxvar=None, d_ini_state=None):
        import torch
        self.calls.append(("jvp", d_auxvar is not None, d_ini_state is not None, tuple(x.shape), tuple(u.shape)))
        B = x.shape[0]
        du = torch.zeros_like(u) if d_auxvar is None else self._u(d_auxvar, B).contiguous()
        return dict(d_state=self._roll(torch.zeros_like(x[:, 0]) if d_ini_state is None else d_ini_state, du), d_control=du)

    def rollout_vjp_batch(self, x, theta, gx, gu, want_theta=True, want_ini=True):
        import torch
        self.calls.append(("vjp", want_theta, want_ini))
        with torch.enable_grad():                        # (the dynamics are linear: the gradient does not depend on where it is taken)
            th = torch.zeros((x.shape[0], self.n_auxvar), dtype=torch.float64, requires_grad=True)
            x0 = x[:, 0].detach().clone().requires_grad_(True)
            u = self._u(th, x.shape[0])
            L = (self._roll(x0, u) * gx).sum() + (u * gu).sum()
            g = torch.autograd.grad(L, [th, x0])
        return dict(grad_theta=g[0], grad_x0=g[1])


def test_forward_mode_and_backward_of_the_layer_against_a_stand_in():
    """_CPTrajectory on CPU tensors: forward_ad reaches rollout_jvp_batch with the saved (state, control) and None where an input carries no tangent; the tangents are
    those of the stand-in; the backward pass next to it still reads the rollout and theta it saved"""
    import torch
    import torch.autograd.forward_ad as fwAD
    from pdp_amd.autograd import _CPTrajectory
    T, B = 4, 3
    cp = _LinearCP(T)
    rng = np.random.default_rng(0)
    t64 = lambda a: torch.as_tensor(a, dtype=torch.float64)
    theta, x0, dth, dx0 = t64(rng.standard_normal(2 * T)), t64(rng.standard_normal((B, 3))), t64(rng.standard_normal(2 * T)), t64(rng.standard_normal((B, 3)))
    want = cp.rollout_jvp_batch(*cp.integrateSys_batch(x0, T, theta)[:2], theta, d_auxvar=dth, d_ini_state=dx0)
    cp.calls.clear()
    with fwAD.dual_level():
        state, control = _CPTrajectory.apply(fwAD.make_dual(theta, dth), fwAD.make_dual(x0, dx0), cp, T)
        assert torch.equal(fwAD.unpack_dual(state).tangent, want["d_state"]) and torch.equal(fwAD.unpack_dual(control).tangent, want["d_control"])
        state, control = _CPTrajectory.apply(fwAD.make_dual(theta, dth), x0, cp, T)
        assert torch.equal(fwAD.unpack_dual(control).tangent, want["d_control"])
        state, control = _CPTrajectory.apply(theta, fwAD.make_dual(x0, dx0), cp, T)
        assert bool((fwAD.unpack_dual(control).tangent == 0).all()) and torch.equal(fwAD.unpack_dual(state).tangent[:, 0], dx0)
    shapes = ((B, T + 1, 3), (B, T, 2))
    assert cp.calls == ["rollout", ("jvp", True, True) + shapes, "rollout", ("jvp", True, False) + shapes, "rollout", ("jvp", False, True) + shapes]
    cp.calls.clear()
    th = theta.clone().requires_grad_(True)
    state, control = _CPTrajectory.apply(th, x0, cp, T)
    gx, gu = t64(rng.standard_normal(tuple(state.shape))), t64(rng.standard_normal(tuple(control.shape)))
    ((state * gx).sum() + (control * gu).sum()).backward()
    assert cp.calls == ["rollout", ("vjp", True, False)]
    direct = cp.rollout_vjp_batch(state.detach(), theta, gx, gu)["grad_theta"].sum(dim=0)
    assert torch.equal(th.grad, direct)
    # duality of the stand-in's pair, through the layer: <g, J v> = <J' g, v>
    lhs = float((gx * want["d_state"]).sum() + (gu * want["d_control"]).sum())
    rhs = float(th.grad @ dth) + float((cp.rollout_vjp_batch(state.detach(), theta, gx, gu)["grad_x0"] * dx0).sum())
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs)


def test_for_cp_refuses_bad_arguments_and_runs_the_loop_on_a_stand_in(monkeypatch):
    """MatrixFreeLM.for_cp: ValueErrors before any call; on the linear stand-in (a linear least-squares problem) the loop reaches the target with residual(state,
    control), each CG iteration one jvp and one vjp on the saved rollout and no rollout; MatrixFreeLM(sid, ..) keeps its own adapter"""
    import ls_rows_common as lr
    import torch
    from pdp_amd import irl
    lr.stand_in_torch(monkeypatch)
    T, B = 4, 3
    cp = _LinearCP(T)
    rng = np.random.default_rng(1)
    x0, truth = rng.standard_normal((B, 3)), rng.standard_normal(2 * T)
    f = lambda state, control: state
    for kw, match in ((dict(ini_state=np.zeros((B, 4))), "ini_state"), (dict(ini_state=np.zeros(3)), "ini_state"), (dict(horizon=0), "horizon"),
                      (dict(theta0=np.zeros(2 * T + 1)), "theta0"), (dict(residual=None), "residual")):
        a = dict(dict(ini_state=x0, horizon=T, theta0=truth, residual=f), **kw)
        with pytest.raises(ValueError, match="MatrixFreeLM.for_cp: " + match):
            irl.MatrixFreeLM.for_cp(cp, a["ini_state"], a["horizon"], a["theta0"], a["residual"])

    class NoPolicy:
        n_state, n_control, n_auxvar = 3, 2, 8
    with pytest.raises(ValueError, match="policy"):
        irl.MatrixFreeLM.for_cp(NoPolicy(), x0, T, truth, f)
    assert cp.calls == []
    target_x, target_u, _ = cp.integrateSys_batch(torch.as_tensor(x0), T, torch.as_tensor(truth))
    cp.calls.clear()
    loop = irl.MatrixFreeLM.for_cp(cp, x0, T, truth + 0.3 * rng.standard_normal(2 * T), lambda state, control: torch.cat([(state - target_x).reshape(B, -1),
                                                                                                                      0.5 * (control - target_u).reshape(B, -1)], dim=1))
    r = loop.run(max_evals=10, loss_tol=1e-24)
    assert r["loss_trace"][-1] <= 1e-24 and (np.diff(r["loss_trace"]) < 0).all() and r["rejected"] == 0
    assert set(r) >= {"loss_trace", "parameter_trace", "lambda_trace", "evaluations", "rejected", "stalled", "iterations", "cg_iterations"}
    assert np.abs(r["parameter_trace"][-1] - truth).max() <= 1e-10
    assert cp.calls.count("rollout") == r["evaluations"]
    assert sum(1 for c in cp.calls if c[0] == "jvp") == r["cg_iterations"]
    assert sum(1 for c in cp.calls if c[0] == "vjp") == r["cg_iterations"] + r["evaluations"]
    assert all(c[1:3] == (True, False) for c in cp.calls if c[0] in ("jvp", "vjp"))
    assert isinstance(loop.sweeps, irl._CPSweeps)

    class Sid:
        n_state, n_control, n_auxvar = 4, 1, 3
    plain = irl.MatrixFreeLM(Sid(), np.zeros((2, 4)), np.zeros((2, 5, 1)), np.zeros(3), lambda s: s)
    assert isinstance(plain.sweeps, irl._SysIDSweeps) and plain.sweeps.sid is plain.sid and plain.B == 2 and plain.p == 3


# ---- the mathematics ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cj.tuned_cases(), ids=cj.case_id)
def test_tangent_sweep_equals_the_references_forward_sensitivities(case):
    """the kernel's recursion (numpy) against integrateAuxSys from X_0 = [0 | I] contracted with the direction, d_state and d_control each relative to its largest
    entry: 1e-11, a tenth of the GPU tolerance - the reference's own error on these inputs is then below what the GPU tests ask.  Samples 0 and 4, shared and
    per-sample theta, both tangents and each alone."""
    name, kind, key, T = case
    tan = cj.tangents(name, kind, key, T)
    worst = 0.0
    for per_sample, b in ((False, 0), (True, 4)):
        r = cj.reference(name, kind, key, T, per_sample, b)
        dth, dx0 = cj.d_theta_of(tan, per_sample, b), tan["d_x0"][b]
        for kw in (dict(d_theta=dth, d_x0=dx0), dict(d_theta=dth), dict(d_x0=dx0)):
            want_x, want_u = cj.contract(r["X"], r["U"], **kw)
            got_x, got_u = cj.tangent_sweep(r["aux"], **kw)
            assert np.isfinite(want_x).all() and np.abs(want_x).max() > 0
            worst = max(worst, cj.rel(got_x, want_x), cj.rel(got_u, want_u))
    print("tangent sweep vs reference, %s: %.3e" % (cj.case_id(case), worst))
    assert worst <= cj.HOST_TOL, (case, worst)


@pytest.mark.parametrize("kind,key", [("poly", 6), ("mlp", (6, 1))], ids=["lagrange", "mlp_6x1"])
def test_reference_equals_central_differences_through_the_oracles_rollout(kind, key):
    """the columns of the reference's sensitivities against (rollout(theta + h e_k) - rollout(theta - h e_k)) / 2 h and the same in x_0 (h = 1e-5) of
    ControlPlanningOracle.integrateSys on C5, T = 12, and the tangent along the case's direction: 2e-4 of the largest entry"""
    name, T, h = "C5", 12, 1e-5
    orc = cv.oracle_for(name, kind, key, T)
    inp = ce.inputs(name, kind, key, T)
    x0, theta = inp["x0"][1], inp["theta"]
    r = cj.reference_at(orc, x0, T, theta)
    p, n = len(theta), len(x0)

    def roll(x0_, th_):
        sol = orc.integrateSys(x0_, T, th_)
        return np.asarray(sol["state_traj"], float), np.asarray(sol["control_traj"], float).reshape(T, orc.m)
    cols = [(roll(x0, theta + h * e), roll(x0, theta - h * e)) for e in np.eye(p)] + [(roll(x0 + h * e, theta), roll(x0 - h * e, theta)) for e in np.eye(n)]
    fd_X = np.stack([(a[0] - b[0]) / (2 * h) for a, b in cols], axis=2)
    fd_U = np.stack([(a[1] - b[1]) / (2 * h) for a, b in cols], axis=2)
    e_X, e_U = np.abs(fd_X - r["X"]).max() / np.abs(fd_X).max(), np.abs(fd_U - r["U"]).max() / np.abs(fd_U).max()
    tan = cj.tangents(name, kind, key, T)
    want_x, want_u = cj.contract(r["X"], r["U"], tan["d_theta"], tan["d_x0"][1])
    (xp, up), (xm, um) = roll(x0 + h * tan["d_x0"][1], theta + h * tan["d_theta"]), roll(x0 - h * tan["d_x0"][1], theta - h * tan["d_theta"])
    e_dx, e_du = cj.rel((xp - xm) / (2 * h), want_x), cj.rel((up - um) / (2 * h), want_u)
    print("reference vs central differences, C5 %s: X %.3e, U %.3e, d_state %.3e, d_control %.3e" % (kind, e_X, e_U, e_dx, e_du))
    assert max(e_X, e_U, e_dx, e_du) <= cj.FD_TOL, (e_X, e_U, e_dx, e_du)


def test_matrix_free_lm_restated_in_numpy_reaches_the_floor():
    """MatrixFreeLM's schedule on the oracle (cp_jvp_common.lm_problem: C15, 6 pivots, p = 18, T = 12, B = 5, reachable targets, states-only residual): a strictly
    decreasing trace to below 1e-20.  Its counts are the budget the GPU loop is held to (twice of each): tests/golden/cp_jvp_lm_budget.json, written here where it is
    missing, and the committed file must hold exactly these counts."""
    r = cj.lm_restatement(cj.lm_problem())
    print("loss trace %s; %d evaluations, %d rejected, %d CG iterations" % (" ".join("%.3e" % v for v in r["loss_trace"]), r["evaluations"], r["rejected"],
                                                                            r["cg_iterations"]))
    assert r["loss_trace"][-1] < 1e-20 and (np.diff(r["loss_trace"]) < 0).all()
    counts = {"evaluations": r["evaluations"], "rejected": r["rejected"], "cg_iterations": r["cg_iterations"]}
    if not os.path.exists(cj.BUDGET):
        with open(cj.BUDGET, "w") as f:
            json.dump(counts, f, indent=1, sort_keys=True)
            f.write("\n")
        pytest.fail("tests/golden/cp_jvp_lm_budget.json was missing: written with %s - commit it" % counts)
    assert cj.budget() == counts, (cj.budget(), counts)
