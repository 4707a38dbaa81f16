"""CPU (no GPU needed): pdp_sysid_rollout_vjp_u_batched - the SysID rollout's gradient with respect to the inputs - at the generator (the `pathu` group), at the ABI
(the table, the exported symbols, the argument errors before any launch, the pool rows), at the Python layers against a recorder library, and the reference of
tests/sysid_vjp_u_common.py against the adjoint recursion in numpy and against central differences of the oracle's rollout.  Bounds: those of
tests/test_sysid_vjp_host.py - 1e-13 numpy against numpy, 1e-6 for central differences with h = 1e-6."""
import ctypes as C

import numpy as np
import pytest

import sysid_vjp_common as sv
import sysid_vjp_u_common as su

NAME, ROWS = "pdp_sysid_rollout_vjp_u_batched", "pdp_sysid_rollout_vjp_u_rows"
SIZE_NAMES = ["chain_40_10_3", "chain_64_4_3", "linear_8_1_64", "linear_8_1_65", "linear_8_2_63", "linear_9_2_99", "mlp_6_2_246"]
# pool rows of a small batch: the generated chunk of the model (tests/test_sysid_vjp_sizes_host.py for four of them; linear_8_2_63: a path row of 135 + 8 doubles, 32 of
# which are within _pick_chunk's 34 KB)
CHUNK = {"chain_40_10_3": 16, "chain_64_4_3": 8, "linear_8_1_64": 16, "linear_8_1_65": 16, "linear_8_2_63": 32, "linear_9_2_99": 16, "mlp_6_2_246": 4}


def _built():
    import __graft_entry__ as g
    g.build()
    from pdp_amd import codegen, runtime as rt, zoo
    return codegen, rt, zoo


def _user_lib(name):
    codegen, _, _ = _built()
    return codegen.build_problem(su.size_problem(name)[0])


@pytest.mark.parametrize("system", su.SYSTEMS)
def test_reference_agrees_with_the_adjoint_recursion_in_numpy(system):
    """G_t propagated forward against the costate sweep, both in numpy, at the chunk-edge horizons (65 / 33): the two orders of the same sums differ by rounding alone
    (seen: 6.6e-16 .. 4.6e-15); 1e-13 of the largest entry per sample, as for grad_theta and grad_x0"""
    c = su.case(system, su.EDGE_T[system])
    worst = 0.0
    for b in range(c["inputs"].shape[0]):
        gu = su.adjoint_sweep_u(system, c["sid"], c["states"][b], c["inputs"][b], c["theta"], c["g"][b])
        worst = max(worst, np.abs(gu - c["grad_u"][b]).max() / np.abs(gu).max())
    print("%s T = %d: forward propagation of G vs adjoint sweep %.2e" % (system, su.EDGE_T[system], worst))
    assert worst <= 1e-13


def test_user_model_reference_agrees_with_the_adjoint_recursion_in_numpy():
    """the same for the user model this file adds (its G columns straddle two lane slots on the GPU), T = 17"""
    c = su.user_case("linear_8_2_63", T=17)
    worst = 0.0
    for b in range(3):
        gu = su.adjoint_sweep_u("linear_8_2_63", c["orc"], c["states"][b], c["inputs"][b], c["theta"], c["g"][b])
        worst = max(worst, np.abs(gu - c["grad_u"][b]).max() / np.abs(gu).max())
    print("linear_8_2_63 T = 17: forward propagation of G vs adjoint sweep %.2e" % worst)
    assert worst <= 1e-13


@pytest.mark.parametrize("system", su.SYSTEMS)
def test_reference_agrees_with_central_differences_of_the_oracle_rollout(system):
    """L = sum g . x(u) is linear in the rollout, so dL/du is the reference's contraction: sample 0 at the chunk-edge horizon, central differences with h = 1e-6 along
    every sixth step's inputs and the last step's, within 1e-6 of the largest entry of grad_u (seen: 3.0e-9 rocket .. 2.3e-7 pendulum)"""
    c = su.case(system, su.EDGE_T[system])
    sid, b, h = c["sid"], 0, 1e-6
    T, m = c["inputs"].shape[1:]
    L = lambda u: float((c["g"][b] * sid.integrateDyn(c["x0"][b], u, c["theta"])).sum())
    worst = 0.0
    for t in sorted(set(range(0, T, 6)) | {T - 1}):
        for j in range(m):
            e = np.zeros((T, m))
            e[t, j] = h
            fd = (L(c["inputs"][b] + e) - L(c["inputs"][b] - e)) / (2 * h)
            worst = max(worst, abs(fd - c["grad_u"][b, t, j]))
    worst /= np.abs(c["grad_u"][b]).max()
    print("%s T = %d: central differences vs the reference: grad_u %.2e" % (system, T, worst))
    assert worst <= 1e-6


def test_the_generator_adds_a_group_of_its_own_and_leaves_path_alone():
    from pdp_amd import codegen, zoo
    for system in su.SYSTEMS:
        src, info = codegen.generate(zoo.make_problem(system, "sysid"))
        assert set(info["nvar"]) == {"path", "pathu"} and 0 < info["nvar"]["pathu"] <= info["n"] * info["m"]
        for word in ("PATHU_NVAR", "PATHU_NCONST", "eval_pathu", "pathu_code", "pathu_const", "// ---- group 'pathu': G[%dx%d]" % (info["n"], info["m"])):
            assert word in src, (system, word)
        assert src.index("eval_path(") < src.index("eval_pathu(")                  # emitted behind `path`
        assert info["chunk"] == codegen._pick_chunk(info["nvar"]["path"], info["n"]) == 32
        # `path` as it was generated before the group existed: its packed entries (ModelLib.nnz_path restates them) and the hoisted values of precompute
        assert (info["nvar"]["path"], info["npc"]) == {"pendulum": (5, 8), "cartpole": (10, 3), "robotarm": (14, 16), "rocket": (56, 9), "quadrotor": (54, 10)}[system]
        assert "static constexpr int NPC = %d;" % info["npc"] in src and "precompute_u(" in src and "NPCU" in src
    for mode in ("irl", "oc"):
        src, info = codegen.generate(zoo.make_problem("cartpole", mode))
        assert "pathu" not in src and "PATHU" not in src and "pathu" not in info["nvar"]


def test_the_entry_points_are_listed_with_their_arguments():
    from pdp_amd import abi
    table = abi.entry_points("pdp_hip_sysid_vjp_u.h", "model")
    assert list(table) == [NAME, ROWS]
    assert table[NAME][0] is C.c_int and len(table[NAME][1]) == 11 and table[ROWS] == (C.c_int, [C.c_int])
    assert not abi.entry_points("pdp_hip_sysid_vjp_u.h", "core")


def test_argument_errors_are_returned_before_any_launch():
    """valid (host) pointers everywhere, so that only the argument under test can be what is refused; nothing that passes the checks is called: no GPU here"""
    codegen, rt, zoo = _built()
    mdl = rt.load_model(codegen.build_problem(zoo.make_problem("quadrotor", "sysid"))[0])
    assert (mdl.p, mdl.m) == (5, 4)
    keep = [(C.c_double * 8)() for _ in range(7)]
    x, u, th, g, gt, g0, gu = (C.cast(k, C.c_void_p) for k in keep)
    fn = getattr(mdl.lib, NAME)
    ok = dict(B=1, T=4, x=x, u=u, th=th, tb=0, g=g, gt=gt, g0=g0, gu=gu)

    def call(lib_fn=fn, **kw):
        a = dict(ok, **kw)
        return lib_fn(a["B"], a["T"], a["x"], a["u"], a["th"], a["tb"], a["g"], a["gt"], a["g0"], a["gu"], None)
    for kw in (dict(gt=None, g0=None, gu=None), dict(B=0), dict(B=-3), dict(T=0), dict(T=-2), dict(tb=4), dict(tb=1), dict(tb=-5), dict(x=None), dict(u=None),
               dict(th=None), dict(g=None), dict(B=0, gu=None), dict(x=None, gt=None, g0=None), dict(tb=3, gu=None)):
        assert call(**kw) == -1, kw                                               # PDP_E_ARG
    assert all(v == 0.0 for k in keep for v in k)
    oc = rt.load_model(codegen.build_problem(zoo.make_problem("cartpole", "irl"))[0])
    ocf = getattr(oc.lib, NAME)
    assert call(ocf) == -4 and call(ocf, gu=None) == -4 and call(ocf, gt=None, g0=None, tb=oc.p) == -4      # PDP_E_MODE
    assert call(ocf, B=0) == -1 and call(ocf, gt=None, g0=None, gu=None) == -1                               # the argument check comes first
    assert getattr(oc.lib, ROWS)(1) == -4 and getattr(oc.lib, ROWS)(0) == -1


def test_a_66_state_model_is_refused_before_any_launch():
    """PDP_E_SIZE from chain_66 (n = 66) with valid host pointers, with and without grad_u; PDP_E_ARG comes first; no buffer is touched"""
    codegen, rt, _ = _built()
    lib, _ = codegen.build_problem(sv.size_problem("chain_66")[0])
    mdl = rt.load_model(lib)
    assert (mdl.n, mdl.m, mdl.p) == (66, 4, 3)
    keep = [(C.c_double * (5 * 66))() for _ in range(7)]
    for k in keep:
        k[:] = [1.5] * len(k)
    x, u, th, g, gt, g0, gu = (C.cast(k, C.c_void_p) for k in keep)
    fn = getattr(mdl.lib, NAME)
    assert fn(1, 4, x, u, th, 0, g, gt, g0, gu, None) == -2 and fn(1, 4, x, u, th, 0, g, None, None, gu, None) == -2        # PDP_E_SIZE
    assert fn(1, 4, x, u, th, 3, g, gt, g0, None, None) == -2
    assert fn(0, 4, x, u, th, 0, g, gt, g0, gu, None) == -1 and fn(1, 4, x, u, th, 0, g, None, None, None, None) == -1     # PDP_E_ARG first
    assert getattr(mdl.lib, ROWS)(1) == -2
    assert "sysid_vjp_u_kernel" not in codegen.kernel_resources(lib)                 # a compile-time branch: nothing is instantiated
    assert all(v == 1.5 for k in keep for v in k)


def test_pool_rows_of_the_zoo_models():
    """a small batch gets the generated chunk; beyond four trajectories per compute unit (256 assumed without a device) the rule of sysid_vjp_rows on the longer row:
    what fits 2400 doubles, at least four rows, at most the chunk"""
    codegen, rt, zoo = _built()
    for system in su.SYSTEMS:
        lib, info = codegen.build_problem(zoo.make_problem(system, "sysid"))
        mdl = rt.load_model(lib)
        assert mdl.sysid_vjp_u_rows(1) == mdl.chunk == info["chunk"] and mdl.sysid_vjp_u_rows(1024) == mdl.chunk
        stride = (info["nvar"]["path"] + info["nvar"]["pathu"] + info["n"] + info["m"]) | 1
        fit = 2400 // stride
        assert mdl.sysid_vjp_u_rows(1025) == (min(fit, mdl.chunk) if fit >= 4 else mdl.chunk), system
        assert mdl.nnz_path == info["nvar"]["path"]
        with pytest.raises(RuntimeError, match="PDP_E_ARG"):
            mdl.sysid_vjp_u_rows(0)


def _stand_ins(monkeypatch):
    import ls_rows_common as lr
    from pdp_amd import PDP, runtime
    lr.stand_in_torch(monkeypatch)
    monkeypatch.setattr(runtime, "ptr", lambda t: ("ptr", tuple(t.shape)))
    mdl = runtime.ModelLib.__new__(runtime.ModelLib)
    mdl.n, mdl.m, mdl.p, mdl.chunk, mdl.nnz_path, mdl.lib = 4, 1, 3, 32, 10, lr.Recorder()       # (what tests/test_sysid_vjp_host.py gives its bare ModelLib: nothing more is needed)
    sid = PDP.SysID.__new__(PDP.SysID)
    sid.n_state, sid.n_control, sid.n_auxvar, sid._model = 4, 1, 3, mdl
    return mdl, sid


def test_the_layers_against_a_recorder_library(monkeypatch):
    """no GPU: the library records.  Shape errors are ValueErrors before any call; without want_inputs the old symbol gets the old ten arguments; with it the new
    symbol gets them and the grad_u buffer; all three switches off is refused"""
    mdl, sid = _stand_ins(monkeypatch)
    B, T = 3, 6
    x, u, th, g = np.zeros((B, T + 1, 4)), np.zeros((B, T, 1)), np.ones(3), np.zeros((B, T + 1, 4))
    bad = [dict(state_traj=x[:, :-1]), dict(state_traj=x[:2]), dict(inputs=u[0]), dict(inputs=np.zeros((B, T, 2))), dict(inputs=np.zeros((B, 0, 1))),
           dict(grad_state=g[:, :, :3]), dict(grad_state=g[:, 1:]), dict(auxvar_value=np.ones(4)), dict(auxvar_value=np.ones((2, 3)))]
    for kw in bad:
        a = dict(dict(state_traj=x, inputs=u, auxvar_value=th, grad_state=g), **kw)
        with pytest.raises(ValueError, match="sysid_rollout_vjp"):
            sid.rollout_vjp_batch(a["state_traj"], a["inputs"], a["auxvar_value"], a["grad_state"], want_inputs=True)
    with pytest.raises(ValueError, match="nothing to compute"):
        mdl.sysid_rollout_vjp(x, u, th, g, want_ini=False, want_theta=False)
    with pytest.raises(ValueError, match="nothing to compute"):
        sid.rollout_vjp_batch(x, u, th, g, want_ini=False, want_theta=False, want_inputs=False)
    assert mdl.lib.calls == []
    P = lambda *shape: ("ptr", shape)
    old = (B, T, P(B, T + 1, 4), P(B, T, 1), P(3), 0, P(B, T + 1, 4))
    out = sid.rollout_vjp_batch(x, u, th, g)
    assert set(out) == {"grad_theta", "grad_x0"}
    out = mdl.sysid_rollout_vjp(x, u, th, g, want_ini=False, want_inputs=False)
    assert set(out) == {"grad_theta"}
    assert mdl.lib.calls == [("pdp_sysid_rollout_vjp_batched", old + (P(B, 3), P(B, 4), None)), ("pdp_sysid_rollout_vjp_batched", old + (P(B, 3), None, None))]
    del mdl.lib.calls[:]
    out = sid.rollout_vjp_batch(x, u, th, g, want_inputs=True)
    assert set(out) == {"grad_theta", "grad_x0", "grad_u"} and tuple(out["grad_u"].shape) == (B, T, 1)
    out = sid.rollout_vjp_batch(x, u, np.ones((B, 3)), g, want_ini=False, want_theta=False, want_inputs=True)
    assert set(out) == {"grad_u"}
    per_sample = (B, T, P(B, T + 1, 4), P(B, T, 1), P(B, 3), 3, P(B, T + 1, 4))
    assert mdl.lib.calls == [(NAME, old + (P(B, 3), P(B, 4), P(B, T, 1), None)), (NAME, per_sample + (None, None, P(B, T, 1), None))]


def test_the_layer_refuses_what_it_cannot_differentiate():
    import torch
    from pdp_amd import autograd

    class Sid:
        n_auxvar = 3
    theta = torch.ones(3, dtype=torch.float64)
    with pytest.raises(TypeError, match="CUDA fp64"):                               # (theta comes first: a CPU tensor)
        autograd.sysid_trajectory(Sid(), np.zeros((2, 4)), np.zeros((2, 5, 1)), theta, input_grad=True)
    with pytest.raises(NotImplementedError, match="df/du") as err:
        autograd.sysid_trajectory(Sid(), np.zeros((2, 4)), torch.zeros((2, 5, 1), dtype=torch.float64, requires_grad=True), _cuda_like(theta))
    assert "input_grad=True" in str(err.value)
    for inputs in (torch.zeros((2, 5, 1), dtype=torch.float64, requires_grad=True), np.zeros((2, 5, 1)), _cuda_like(torch.zeros((2, 5, 1), dtype=torch.float32))):
        with pytest.raises(TypeError, match="input_grad=True the inputs must be a CUDA fp64 tensor"):
            autograd.sysid_trajectory(Sid(), np.zeros((2, 4)), inputs, _cuda_like(theta), input_grad=True)
    doc = autograd.__doc__
    assert "input_grad=True" in doc and "Limits" in doc and "oc_trajectory: no gradient with respect to ini_state" in doc


def _cuda_like(t):
    """a CPU tensor that answers is_cuda = True: the layer's type checks run without a GPU, nothing is launched behind them"""
    import torch

    class T(torch.Tensor):
        is_cuda = True
    return t.as_subclass(T)


@pytest.mark.parametrize("name", SIZE_NAMES)
def test_pool_rows_and_kernel_resources_of_the_size_models(name):
    """pool rows of a small batch = the generated chunk; the figures of sysid_vjp_u_kernel are printed, not bounded: the MLP's and the 64-state chain's instantiations
    spill, as their sysid_vjp_kernel twins do"""
    codegen, rt, _ = _built()
    lib, info = _user_lib(name)
    mdl = rt.load_model(lib)
    assert info["chunk"] == CHUNK[name] == mdl.sysid_vjp_u_rows(1) == mdl.sysid_vjp_u_rows(3)
    k = codegen.kernel_resources(lib)
    r, r0 = k["sysid_vjp_u_kernel"], k["sysid_vjp_kernel"]
    print("%s: n = %d m = %d p = %d path nvar %d pathu nvar %d CHUNK %d; sysid_vjp_u_kernel vgpr %d (agpr %d) spill %d scratch %d B; sysid_vjp_kernel vgpr %d spill %d scratch %d B"
          % (name, info["n"], info["m"], info["p"], info["nvar"]["path"], info["nvar"]["pathu"], info["chunk"], r["vgpr"], r["agpr"], r["spill"], r["scratch"],
             r0["vgpr"], r0["spill"], r0["scratch"]))


def test_zoo_kernels_use_no_scratch():
    """sysid_vjp_u_kernel of the five zoo libraries: no spills, no scratch (tests/test_abi_and_host.py reads the spills of every kernel; the scratch is held here)"""
    codegen, _, zoo = _built()
    for system in su.SYSTEMS:
        lib, _ = codegen.build_problem(zoo.make_problem(system, "sysid"))
        r = codegen.kernel_resources(lib)["sysid_vjp_u_kernel"]
        print("%s: sysid_vjp_u_kernel vgpr %d sgpr %d spill %d scratch %d" % (system, r["vgpr"], r["sgpr"], r["spill"], r["scratch"]))
        assert r["spill"] == 0 and r["scratch"] == 0, (system, r)
