"""CPU (no GPU needed): pdp_sysid_step_gn_ini_batched - SysID.step with estimated components of the initial state - at the ABI (the header, the binding's lists, the
argument errors before any launch), the normalisation of estimate_ini, the arrow-shaped normal equations of LMLoop.for_sysid(estimate_ini=) against the dense Jacobian,
the reference rows of tests/sysid_ini_common.py against central differences of the loss, and the evaluation counts of the oracle schedule that the GPU tests are held
to."""
import ctypes as C

import numpy as np
import pytest

import sysid_gn_common as sg
import sysid_ini_common as si

ROOT = sg.ROOT
NAME = "pdp_sysid_step_gn_ini_batched"


def _built():
    import __graft_entry__ as g
    g.build()
    from pdp_amd import codegen, runtime as rt, zoo
    return codegen, rt, zoo


def test_the_entry_point_is_declared_listed_and_exported():
    """(tests/test_abi_table.py holds the whole binding against the headers and the built libraries; what stays here is this entry point's own line)"""
    from pdp_amd import abi
    (name, (restype, argtypes)), = abi.entry_points("pdp_hip_sysid_ini.h", "model").items()
    assert name == NAME and restype is C.c_int and len(argtypes) == 14


def test_argument_errors_are_returned_before_any_launch():
    """valid (host) pointers everywhere, so that only the argument under test can be what is refused; nothing that passes the checks is called: no GPU here"""
    codegen, rt, zoo = _built()
    mdl = rt.load_model(codegen.build_problem(zoo.make_problem("quadrotor", "sysid"))[0])
    keep = [(C.c_double * 8)() for _ in range(7)]
    u, xo, x0, th, loss, packed, ws = (C.cast(k, C.c_void_p) for k in keep)
    fn = getattr(mdl.lib, NAME)
    ok = dict(B=1, T=4, u=u, xo=xo, x0=x0, mask=0b111000, th=th, flags=0, loss=loss, packed=packed)

    def call(lib_fn=fn, **kw):
        a = dict(ok, **kw)
        return lib_fn(a["B"], a["T"], a["u"], a["xo"], a["x0"], a["mask"], a["th"], 0, a["flags"], a["loss"], a["packed"], ws, 1 << 40, None)
    for kw in (dict(B=0), dict(T=0), dict(T=-2), dict(u=None), dict(xo=None), dict(th=None), dict(loss=None), dict(packed=None), dict(flags=1), dict(flags=16),
               dict(flags=64), dict(flags=-1), dict(mask=1 << 13), dict(mask=(1 << 13) | 8), dict(mask=1 << 20), dict(mask=-1),
               dict(mask=0, flags=64), dict(mask=0, B=0), dict(mask=0, packed=None)):
        assert call(**kw) == -1, kw                                               # PDP_E_ARG (mask 0: pdp_sysid_step_gn_batched's own checks)
    assert call(mask=0b1111111111111) == -2                                       # p + q = 5 + 13 > 16: PDP_E_SIZE, before any launch
    assert call(mask=0b0111111111111) == -2                                       # 5 + 12
    assert all(v == 0.0 for k in keep for v in k)
    oc = rt.load_model(codegen.build_problem(zoo.make_problem("cartpole", "irl"))[0])
    for flags in (0, 32):
        for mask in (0, 0b1100):
            assert call(getattr(oc.lib, NAME), flags=flags, mask=mask) == -4      # PDP_E_MODE: not a SysID model
    assert call(getattr(oc.lib, NAME), mask=1 << 4) == -1                         # the argument check comes first (cart-pole: n = 4)


def test_estimate_ini_is_normalised_or_refused():
    from pdp_amd.runtime import ini_indices
    assert ini_indices(None, 4) == ([], 0) and ini_indices([], 4) == ([], 0) and ini_indices(np.zeros(4, bool), 4) == ([], 0)
    assert ini_indices([2, 3], 4) == ([2, 3], 12) and ini_indices((0, 3), 4) == ([0, 3], 9) and ini_indices(np.array([1]), 2) == ([1], 2)
    assert ini_indices([False, False, True, True], 4) == ([2, 3], 12) and ini_indices(np.array([True, False, False, True]), 4) == ([0, 3], 9)
    assert ini_indices(range(2, 13), 13) == (list(range(2, 13)), sum(1 << i for i in range(2, 13)))
    import torch
    assert ini_indices(torch.tensor([3, 4, 5]), 13) == ([3, 4, 5], 56) and ini_indices(torch.tensor([False, True]), 2) == ([1], 2)
    for bad, n in (([2, 2], 4), ([4], 4), ([-1], 4), ([3, 2], 4), ([True, False, True], 4), ([0.5], 4), ([0, 1, 1, 3], 4)):
        with pytest.raises(ValueError, match="estimate_ini"):
            ini_indices(bad, n)


def test_sysid_step_passes_the_mask_and_returns_rows_of_width_W(monkeypatch):
    """no GPU: tensors are replaced by a stand-in, the library by a recorder.  estimate_ini goes to the new entry point with the mask as its sixth argument; without
    it, or with nothing selected, the calls are the ones they were."""
    import torch
    from pdp_amd import runtime

    class _Torch:
        float64 = torch.float64

        class cuda:
            @staticmethod
            def is_current_stream_capturing():
                return False
        empty = staticmethod(lambda shape, dtype=None, device=None: torch.zeros(shape, dtype=dtype))
        zeros = staticmethod(lambda shape, dtype=None, device=None: torch.zeros(shape, dtype=dtype))
    monkeypatch.setattr(runtime, "torch_cuda", lambda: _Torch)
    monkeypatch.setattr(runtime, "dev", lambda a: a if hasattr(a, "data_ptr") else torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=float))))
    monkeypatch.setattr(runtime, "current_stream_ptr", lambda: None)
    mdl = runtime.ModelLib.__new__(runtime.ModelLib)
    mdl.n, mdl.m, mdl.p, mdl.lib = 4, 1, 3, si.Recorder()
    B, T = 3, 6
    u, xo, th = np.zeros((B, T, 1)), np.zeros((B, T + 1, 4)), np.ones(3)
    out = mdl.sysid_step(u, xo, th, gauss_newton=True, skip_missing=True, ini_state=np.zeros((B, 4)), estimate_ini=[2, 3])
    assert [c[0] for c in mdl.lib.calls] == ["pdp_sysid_step_workspace_bytes", NAME]
    args = mdl.lib.calls[1][1]
    assert len(args) == 14 and args[:2] == (B, T) and args[5] == 12 and args[8] == 32 and args[4].value is not None
    assert set(out) == {"packed_gn", "loss", "grad", "gn", "ini_index"} and out["ini_index"] == [2, 3]
    assert tuple(out["packed_gn"].shape) == (B, 5 + 1 + 25) and tuple(out["grad"].shape) == (B, 5) and tuple(out["gn"].shape) == (B, 5, 5)
    assert out["gn"].data_ptr() == out["packed_gn"][:, 6:].data_ptr() and out["loss"].data_ptr() == out["packed_gn"][:, 5].data_ptr()
    mdl.lib.calls.clear()
    loss, grad = mdl.sysid_step(u, xo, th, estimate_ini=np.array([True, False, False, True]))
    assert mdl.lib.calls[1][0] == NAME and mdl.lib.calls[1][1][5] == 9 and mdl.lib.calls[1][1][8] == 0 and mdl.lib.calls[1][1][4].value is None
    assert tuple(loss.shape) == (B,) and tuple(grad.shape) == (B, 5)
    for kw, name in ((dict(estimate_ini=[]), "pdp_sysid_step_ws_batched"), (dict(estimate_ini=None, gauss_newton=True), "pdp_sysid_step_gn_batched"),
                     (dict(estimate_ini=[], gauss_newton=True), "pdp_sysid_step_gn_batched")):
        mdl.lib.calls.clear()
        out = mdl.sysid_step(u, xo, th, **kw)
        assert [c[0] for c in mdl.lib.calls] == ["pdp_sysid_step_workspace_bytes", name]
        if kw.get("gauss_newton"):
            assert tuple(out["gn"].shape) == (B, 3, 3) and "ini_index" not in out      # nothing selected is estimate_ini=None
    # an estimated component still needs a finite starting value
    mdl.lib.calls.clear()
    x0 = np.zeros((B, 4))
    x0[1, 2] = np.nan
    with pytest.raises(ValueError, match="ini_state"):
        mdl.sysid_step(u, xo, th, skip_missing=True, ini_state=x0, estimate_ini=[2, 3])
    with pytest.raises(ValueError, match="estimate_ini"):
        mdl.sysid_step(u, xo, th, estimate_ini=[4])
    assert mdl.lib.calls == []


@pytest.mark.parametrize("system, idx", [("pendulum", [1]), ("cartpole", [2, 3]), ("quadrotor", [3, 4, 5, 10, 11, 12])], ids=["pendulum", "cartpole", "quadrotor"])
def test_arrow_matrix_is_the_dense_jacobians_normal_matrix(system, idx):
    """irl.arrow_normal_equations (torch, here on CPU tensors) and its numpy restatement against J'J / B and J'r / B of the stacked dense Jacobian: 1e-12 relative"""
    import torch
    from pdp_amd.irl import arrow_normal_equations
    sid, c = sg.oracle(system), si.perturbed_case(system, idx, seed=7)
    B, p, q = c["inputs"].shape[0], sid.p, len(idx)
    N = p + B * q
    rows = si.reference_rows(sid, c["inputs"], c["states"], c["theta"], idx, c["ini"], True)
    r, J = si.dense_jacobian(sid, c["inputs"], c["states"], c["theta"], idx, c["ini"], True)
    loss, g, A = si.arrow(*rows, p)
    flat = arrow_normal_equations(torch.as_tensor(si.packed(rows)), p, q).numpy()
    assert flat.shape == (N + 1 + N * N,)
    for tag, (l_, g_, A_) in (("numpy", (loss, g, A)), ("torch", (flat[N], flat[:N], flat[N + 1:].reshape(N, N)))):
        ref_A, ref_g, ref_l = J.T @ J / B, J.T @ r / B, r @ r / B
        ea, eg, el = np.abs(A_ - ref_A).max() / np.abs(ref_A).max(), np.abs(g_ - ref_g).max() / np.abs(ref_g).max(), abs(l_ - ref_l) / ref_l
        print("%s %s: G %.2e  g %.2e  loss %.2e" % (system, tag, ea, eg, el))
        assert ea <= 1e-12 and eg <= 1e-12 and el <= 1e-12
        assert np.array_equal(A_, A_.T)
        for b in range(B):                          # two different recordings share no entry
            for b2 in range(b + 1, B):
                assert not A_[p + b * q:p + (b + 1) * q, p + b2 * q:p + (b2 + 1) * q].any()


@pytest.mark.parametrize("system, idx", [("pendulum", [1]), ("cartpole", [2, 3]), ("quadrotor", [3, 4, 5, 10, 11, 12])], ids=["pendulum", "cartpole", "quadrotor"])
def test_reference_gradient_agrees_with_central_differences(system, idx):
    """masked data, perturbed theta and x0: grad [W] is half the derivative of the loss with respect to [theta | x0[idx]] (h = 1e-6): 1e-7 of its largest entry"""
    sid, c = sg.oracle(system), si.perturbed_case(system, idx, seed=3)
    p, h, b = sid.p, 1e-6, 0                       # (sample 1 of the mask has nothing observed)
    grad = si.reference_rows(sid, c["inputs"], c["states"], c["theta"], idx, c["ini"], True, samples=[b])[1][0]

    def loss(v):
        ini = c["ini"][b].copy()
        ini[idx] = v[p:]
        xs = sid.integrateDyn(ini, c["inputs"][b], v[:p])
        d = xs - c["states"][b]
        return (np.where(np.isnan(c["states"][b]), 0.0, d) ** 2).sum()
    v0 = np.concatenate([c["theta"], c["ini"][b, idx]])
    fd = np.array([(loss(v0 + h * e) - loss(v0 - h * e)) / (2 * h) for e in np.eye(v0.size)]) / 2
    err = np.abs(fd - grad).max() / np.abs(grad).max()
    print("%s: central differences vs the restatement %.2e" % (system, err))
    assert err <= 1e-7


@pytest.mark.parametrize("system, scale", sorted(si.SHARED_COUNTS), ids=["%s_%.1f" % k for k in sorted(si.SHARED_COUNTS)])
def test_oracle_schedule_shared_theta_reproduces_the_evaluation_counts(system, scale):
    r = si.oracle_lm_shared(system, scale, 1e-20)
    print(system, scale, r["evaluations"], " ".join("%.3e" % v for v in r["loss_trace"]))
    assert r["evaluations"] == si.SHARED_COUNTS[(system, scale)] and r["rejected"] == 0 and not r["stalled"]
    assert (np.diff(r["loss_trace"]) < 0).all()
    if system == "cartpole":
        c = si.lm_data(system)
        th, B = r["parameter_trace"][-1], c["inputs"].shape[0]
        assert np.abs(th[:3] - sg.stored(system)[2]).max() <= 1e-8
        assert np.abs(th[3:].reshape(B, 2) - c["x0_true"][:, c["idx"]]).max() <= 1e-8


@pytest.mark.parametrize("system, scale", [(s, sc) for s in sorted(si.PER_TRAJECTORY_COUNTS) for sc in sorted(si.PER_TRAJECTORY_COUNTS[s])],
                         ids=["%s_%.1f" % (s, sc) for s in sorted(si.PER_TRAJECTORY_COUNTS) for sc in sorted(si.PER_TRAJECTORY_COUNTS[s])])
def test_oracle_schedule_per_trajectory_reproduces_the_evaluation_counts(system, scale):
    got = []
    for b in range(3):
        r = si.oracle_lm_trajectory(system, b, scale, 1e-20)
        print(system, scale, b, r["evaluations"], " ".join("%.3e" % v for v in r["loss_trace"]))
        assert r["rejected"] == 0 and not r["stalled"] and (np.diff(r["loss_trace"]) < 0).all()
        got.append(r["evaluations"])
    assert tuple(got) == si.PER_TRAJECTORY_COUNTS[system][scale]
