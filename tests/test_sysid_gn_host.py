"""CPU (no GPU needed): pdp_sysid_step_gn_batched - SysID.step with the Gauss-Newton matrix and missing observations - at the ABI (the symbol, its argument errors
before any launch), the inputs of the Levenberg-Marquardt tests pinned by the oracle schedule, and ModelLib.sysid_step's default call, which stays today's call."""
import ctypes as C

import numpy as np
import pytest

import ls_rows_common as lr
import sysid_gn_common as sg

ROOT = sg.ROOT


def _built():
    import __graft_entry__ as g
    g.build()
    from pdp_amd import codegen, runtime as rt, zoo
    return codegen, rt, zoo


def test_the_entry_point_is_declared_listed_and_exported():
    """(tests/test_abi_table.py holds the whole binding against the headers and the built libraries; what stays here is this entry point's own line)"""
    from pdp_amd import abi
    (name, (restype, argtypes)), = abi.entry_points("pdp_hip_sysid_gn.h", "model").items()
    assert name == "pdp_sysid_step_gn_batched" and restype is C.c_int and len(argtypes) == 13


def test_argument_errors_are_returned_before_any_launch():
    """Valid (host) pointers everywhere, so that only the argument under test can be what is refused.  Nothing that passes the checks is called here: this machine
    may have no GPU."""
    codegen, rt, zoo = _built()
    mdl = rt.load_model(codegen.build_problem(zoo.make_problem("quadrotor", "sysid"))[0])
    keep = [(C.c_double * 8)() for _ in range(7)]
    u, xo, x0, th, loss, packed, ws = (C.cast(k, C.c_void_p) for k in keep)
    fn = mdl.lib.pdp_sysid_step_gn_batched
    B, T, big = 1, 4, 1 << 40
    ok = dict(B=B, T=T, u=u, xo=xo, x0=x0, th=th, flags=0, loss=loss, packed=packed)

    def call(**kw):
        a = dict(ok, **kw)
        return fn(a["B"], a["T"], a["u"], a["xo"], a["x0"], a["th"], 0, a["flags"], a["loss"], a["packed"], ws, big, None)
    for kw in (dict(B=0), dict(B=-3), dict(T=0), dict(u=None), dict(xo=None), dict(th=None), dict(loss=None), dict(packed=None),
               dict(flags=1), dict(flags=16), dict(flags=32 | 16), dict(flags=64), dict(flags=-1)):
        assert call(**kw) == -1, kw                                               # PDP_E_ARG
    assert all(v == 0.0 for k in keep for v in k)                                 # (and nothing was written by the host code)
    oc = rt.load_model(codegen.build_problem(zoo.make_problem("cartpole", "irl"))[0])
    for flags in (0, 32):
        assert oc.lib.pdp_sysid_step_gn_batched(B, T, u, xo, x0, th, 0, flags, loss, packed, ws, big, None) == -4      # PDP_E_MODE: not a SysID model
    assert oc.lib.pdp_sysid_step_gn_batched(B, T, u, xo, x0, th, 0, 64, loss, packed, ws, big, None) == -1              # the argument check comes first


@pytest.mark.parametrize("k", range(len(sg.LM_INPUTS)), ids=[t[0] for t in sg.LM_INPUTS])
def test_oracle_lm_schedule_reproduces_the_evaluation_counts(k):
    """pins the eight inputs of the Levenberg-Marquardt tests (tests/test_gpu_sysid_gn.py): irl.LMLoop with default settings on the CPU reference, from the stored
    run's theta, loss_tol = 1e-20"""
    r = sg.oracle_lm(k, 1e-20)
    print(sg.LM_INPUTS[k][0], " ".join("%.3e" % v for v in r["loss_trace"]))
    assert r["evaluations"] == sg.LM_INPUTS[k][3] and r["rejected"] == 0 and not r["stalled"]
    assert r["loss_trace"][-1] <= 1e-16 and (np.diff(r["loss_trace"]) < 0).all()


def test_sysid_step_with_default_arguments_is_todays_call(monkeypatch):
    """no GPU: tensors are replaced by a stand-in, the library by a recorder.  The default call passes today's eleven arguments to pdp_sysid_step_ws_batched and never
    touches the new entry point; each of the three new arguments alone goes to pdp_sysid_step_gn_batched with the flags it asks for."""
    lr.stand_in_torch(monkeypatch)
    mdl = lr.stand_in_model()
    B, T = 3, 6
    u, xo, th = np.zeros((B, T, 1)), np.zeros((B, T + 1, 4)), np.ones(3)
    loss, grad = mdl.sysid_step(u, xo, th)
    names = [c[0] for c in mdl.lib.calls]
    assert names == ["pdp_sysid_step_workspace_bytes", "pdp_sysid_step_ws_batched"]
    args = mdl.lib.calls[1][1]
    assert len(args) == 11 and args[:2] == (B, T) and tuple(loss.shape) == (B,) and tuple(grad.shape) == (B, 3)
    for kw, flags, dict_out in ((dict(gauss_newton=True), 0, True), (dict(skip_missing=True), 32, False), (dict(ini_state=np.zeros((B, 4))), 0, False),
                                (dict(gauss_newton=True, skip_missing=True, ini_state=np.zeros((B, 4))), 32, True)):
        mdl.lib.calls.clear()
        out = mdl.sysid_step(u, xo, th, **kw)
        assert [c[0] for c in mdl.lib.calls] == ["pdp_sysid_step_workspace_bytes", "pdp_sysid_step_gn_batched"]
        args = mdl.lib.calls[1][1]
        assert len(args) == 13 and args[:2] == (B, T) and args[7] == flags and (args[4].value is None) == ("ini_state" not in kw)
        if dict_out:
            assert set(out) == {"packed_gn", "loss", "grad", "gn"} and tuple(out["packed_gn"].shape) == (B, 3 + 1 + 9) and tuple(out["gn"].shape) == (B, 3, 3)
            assert out["gn"].data_ptr() == out["packed_gn"][:, 4:].data_ptr() and out["loss"].data_ptr() == out["packed_gn"][:, 3].data_ptr()
        else:
            assert tuple(out[0].shape) == (B,) and tuple(out[1].shape) == (B, 3)
    # skip_missing: a NaN in the initial state that would be used is refused before any foreign call
    mdl.lib.calls.clear()
    bad = xo.copy()
    bad[1, 0, 2] = np.nan
    with pytest.raises(ValueError, match="ini_state"):
        mdl.sysid_step(u, bad, th, skip_missing=True)
    x0 = np.zeros((B, 4))
    x0[2, 1] = np.nan
    with pytest.raises(ValueError, match="ini_state"):
        mdl.sysid_step(u, xo, th, gauss_newton=True, skip_missing=True, ini_state=x0)
    assert mdl.lib.calls == []
    mdl.sysid_step(u, bad, th, skip_missing=True, ini_state=np.zeros((B, 4)))      # the unobserved first row is fine once ini_state is given
    assert [c[0] for c in mdl.lib.calls][-1] == "pdp_sysid_step_gn_batched"
