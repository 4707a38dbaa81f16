"""CPU (no GPU needed): the host paths of the least-squares rows - ModelLib.sysid_step, ModelLib.oc_pdp_grad and the evaluations of the Levenberg-Marquardt
constructors of irl.py - characterised by the foreign calls they make: the stand-in library records them (ls_rows_common), and for every mode the test states the call
sequence and every scalar argument of the evaluation call literally.  Written against the five separate host paths and kept unchanged when they became one routine per
unit.  And the one function that forms the packed row from materialised sensitivities, to the bit against the five expressions it replaced."""
import numpy as np
import pytest

import ls_rows_common as lr

INF = float("inf")
n, m, p, B, T = 4, 1, 3, 3, 6
IDX, MASK, W = [1, 3], 10, 5

# the positional arguments of the evaluation entry points (include/pdp_hip_sysid_gn.h, pdp_hip_sysid_ini.h, pdp_hip_sysid_wls.h, pdp_hip.h, pdp_hip_oc_wls.h)
LAYOUT = {
    "pdp_sysid_step_gn_batched": "B T u xobs x0 theta tb flags loss packed ws nbytes stream",
    "pdp_sysid_step_gn_ini_batched": "B T u xobs x0 ini_mask theta tb flags loss packed ws nbytes stream",
    "pdp_sysid_step_wls_batched": "B T u xobs x0 ini_mask w wbs delta theta tb flags loss packed ws nbytes stream",
    "pdp_oc_pdp_grad_batched": "B T flags x0 u theta tb demo_x demo_u x lam loss packed dxdp dudp status ws nbytes stream",
    "pdp_oc_pdp_grad_wls_batched": "B T flags x0 u theta tb demo_x demo_u wx wxs wu wus delta x lam loss packed status ws nbytes stream",
}
POINTERS = set("u xobs x0 theta w loss packed ws stream demo_x demo_u x lam dxdp dudp status wx wu".split())


def the_call(mdl, workspace_query):
    """the recorded calls are the workspace query and ONE evaluation; that call as dict(name, every scalar argument, null = the names of its NULL pointers, ptr = the
    addresses of the others)"""
    assert [c[0] for c in mdl.lib.calls[:-1]] == [workspace_query], [c[0] for c in mdl.lib.calls]
    name, args = mdl.lib.calls[-1]
    names = LAYOUT[name].split()
    assert len(args) == len(names), (name, len(args))
    value = lambda a: getattr(a, "value", a)
    out = dict(name=name, null={k for k, a in zip(names, args) if k in POINTERS and value(a) is None},
               ptr={k: value(a) for k, a in zip(names, args) if k in POINTERS and value(a) is not None})
    out.update({k: a for k, a in zip(names, args) if k not in POINTERS})
    mdl.lib.calls.clear()
    return out


def scalars(call):
    return {k: v for k, v in call.items() if k != "ptr"}


def sysid_data():
    rng = np.random.default_rng(0)
    return rng.standard_normal((B, T, m)), rng.standard_normal((B, T + 1, n)), np.ones(p)


SYSID_STEP = [
    ("gauss_newton", dict(gauss_newton=True),
     dict(name="pdp_sysid_step_gn_batched", B=3, T=6, tb=0, flags=0, nbytes=0, null={"x0", "ws", "stream"}), "dict", 3),
    ("skip_missing", dict(skip_missing=True),
     dict(name="pdp_sysid_step_gn_batched", B=3, T=6, tb=0, flags=32, nbytes=0, null={"x0", "ws", "stream"}), "pair", 3),
    ("ini_state", dict(ini_state=np.zeros((B, n))),
     dict(name="pdp_sysid_step_gn_batched", B=3, T=6, tb=0, flags=0, nbytes=0, null={"ws", "stream"}), "pair", 3),
    ("estimate_ini", dict(estimate_ini=[1, 3]),
     dict(name="pdp_sysid_step_gn_ini_batched", B=3, T=6, ini_mask=10, tb=0, flags=0, nbytes=0, null={"x0", "ws", "stream"}), "pair", 5),
    ("weights", dict(weights=np.ones(n)),
     dict(name="pdp_sysid_step_wls_batched", B=3, T=6, ini_mask=0, wbs=0, delta=INF, tb=0, flags=0, nbytes=0, null={"x0", "ws", "stream"}), "dict", 3),
    ("huber_delta", dict(huber_delta=0.5),
     dict(name="pdp_sysid_step_wls_batched", B=3, T=6, ini_mask=0, wbs=0, delta=0.5, tb=0, flags=0, nbytes=0, null={"x0", "w", "ws", "stream"}), "dict", 3),
    ("weights_and_estimate_ini", dict(weights=np.ones((B, T + 1, n)), estimate_ini=[1, 3], skip_missing=True, ini_state=np.zeros((B, n))),
     dict(name="pdp_sysid_step_wls_batched", B=3, T=6, ini_mask=10, wbs=28, delta=INF, tb=0, flags=32, nbytes=0, null={"ws", "stream"}), "dict+ini", 5),
]


@pytest.mark.parametrize("case", SYSID_STEP, ids=[c[0] for c in SYSID_STEP])
def test_sysid_step_makes_one_call_with_these_arguments(monkeypatch, case):
    _, kw, expected, shape, width = case
    lr.stand_in_torch(monkeypatch)
    mdl = lr.stand_in_model()
    u, xo, th = sysid_data()
    out = mdl.sysid_step(u, xo, th, **kw)
    assert scalars(the_call(mdl, "pdp_sysid_step_workspace_bytes")) == expected
    if shape == "pair":
        assert tuple(out[0].shape) == (B,) and tuple(out[1].shape) == (B, width)
    else:
        assert set(out) == {"packed_gn", "loss", "grad", "gn"} | ({"ini_index"} if shape == "dict+ini" else set())
        assert tuple(out["packed_gn"].shape) == (B, width + 1 + width * width) and tuple(out["gn"].shape) == (B, width, width)
        assert out["loss"].data_ptr() == out["packed_gn"][:, width].data_ptr() and out["gn"].data_ptr() == out["packed_gn"][:, width + 1:].data_ptr()
        assert shape == "dict" or out["ini_index"] == IDX
    per_sample = np.ones((B, p))                                                    # per-sample parameters: the row stride is p
    mdl.sysid_step(u, xo, per_sample, **kw)
    assert scalars(the_call(mdl, "pdp_sysid_step_workspace_bytes")) == dict(expected, tb=3)


def test_sysid_step_keeps_one_buffer_per_entry_point_in_a_shared_dict(monkeypatch):
    lr.stand_in_torch(monkeypatch)
    mdl = lr.stand_in_model()
    u, xo, th = sysid_data()
    bufs = {}
    for kw in (dict(gauss_newton=True), dict(estimate_ini=[1, 3]), dict(weights=np.ones(n)), dict(weights=np.ones(n), estimate_ini=[1, 3])):
        mdl.sysid_step(u, xo, th, buffers=bufs, **kw)
    assert set(bufs) == {"loss", "packed_gn", "packed_gn_ini", "packed_gn_wls"}
    assert tuple(bufs["packed_gn"].shape) == (B, 13) and tuple(bufs["packed_gn_ini"].shape) == (B, 31) and tuple(bufs["packed_gn_wls"].shape) == (B, 31)
    kept = bufs["packed_gn"].data_ptr()
    assert mdl.sysid_step(u, xo, th, gauss_newton=True, buffers=bufs)["packed_gn"].data_ptr() == kept


def oc_data():
    rng = np.random.default_rng(1)
    return rng.standard_normal((B, T, m)), np.ones(p), rng.standard_normal((B, T + 1, n)), rng.standard_normal((B, T, m)), np.zeros((B, n))


OC_GRAD = [
    ("gauss_newton", dict(gauss_newton=True), False,
     dict(name="pdp_oc_pdp_grad_batched", B=3, T=6, flags=16, tb=0, nbytes=0, null={"dxdp", "dudp", "stream"})),
    ("gauss_newton_skip_missing", dict(gauss_newton=True, skip_missing=True), False,
     dict(name="pdp_oc_pdp_grad_batched", B=3, T=6, flags=48, tb=0, nbytes=0, null={"dxdp", "dudp", "stream"})),
    ("weights_x", dict(weights_x=np.ones(n)), False,
     dict(name="pdp_oc_pdp_grad_wls_batched", B=3, T=6, flags=0, tb=0, wxs=0, wus=0, delta=INF, nbytes=0, null={"wu", "stream"})),
    ("huber_delta_given_trajectory", dict(huber_delta=0.5), True,
     dict(name="pdp_oc_pdp_grad_wls_batched", B=3, T=6, flags=1, tb=0, wxs=0, wus=0, delta=0.5, nbytes=0, null={"x0", "wx", "wu", "stream"})),
]


@pytest.mark.parametrize("case", OC_GRAD, ids=[c[0] for c in OC_GRAD])
def test_oc_pdp_grad_makes_one_call_with_these_arguments(monkeypatch, case):
    import torch
    _, kw, given, expected = case
    lr.stand_in_torch(monkeypatch)
    mdl = lr.stand_in_model()
    u, th, dx, du, x0 = oc_data()
    traj = dict(x=torch.zeros((B, T + 1, n), dtype=torch.float64), lam=torch.zeros((B, T, n), dtype=torch.float64)) if given else dict(x0=x0)
    out = mdl.oc_pdp_grad(u, th, dx, du, **traj, **kw)
    call = the_call(mdl, "pdp_oc_pdp_workspace_bytes")
    assert scalars(call) == expected
    assert set(out) == {"packed_gn", "loss", "grad", "gn", "x", "lam", "status"}
    assert tuple(out["packed_gn"].shape) == (B, 13) and tuple(out["gn"].shape) == (B, 3, 3) and out["grad"].data_ptr() == out["packed_gn"].data_ptr()
    assert call["ptr"]["packed"] == out["packed_gn"].data_ptr() and call["ptr"]["x"] == out["x"].data_ptr() and call["ptr"]["lam"] == out["lam"].data_ptr()
    if given:
        assert out["x"].data_ptr() == traj["x"].data_ptr() and out["lam"].data_ptr() == traj["lam"].data_ptr()
    mdl.oc_pdp_grad(u, np.ones((B, p)), dx, du, **traj, **kw)                         # per-sample parameters: the row stride is p
    assert scalars(the_call(mdl, "pdp_oc_pdp_workspace_bytes")) == dict(expected, tb=3)


LM_SYSID = [
    ("LMLoop", False, False, dict(name="pdp_sysid_step_gn_batched", B=3, T=6, tb=0, flags=0, nbytes=0, null={"x0", "ws", "stream"})),
    ("LMLoop_weights", False, True,
     dict(name="pdp_sysid_step_wls_batched", B=3, T=6, ini_mask=0, wbs=0, delta=INF, tb=0, flags=0, nbytes=0, null={"x0", "ws", "stream"})),
    ("LMLoop_estimate_ini", True, False,
     dict(name="pdp_sysid_step_gn_ini_batched", B=3, T=6, ini_mask=10, tb=0, flags=0, nbytes=0, null={"ws", "stream"})),
    ("LMLoop_estimate_ini_weights", True, True,
     dict(name="pdp_sysid_step_wls_batched", B=3, T=6, ini_mask=10, wbs=0, delta=INF, tb=0, flags=0, nbytes=0, null={"ws", "stream"})),
]


@pytest.mark.parametrize("case", LM_SYSID, ids=[c[0] for c in LM_SYSID])
def test_lm_loop_for_sysid_evaluates_with_one_call(monkeypatch, case):
    from pdp_amd.irl import LMLoop
    _, ini, weighted, expected = case
    lr.stand_in_torch(monkeypatch)
    mdl = lr.stand_in_model()
    u, xo, th = sysid_data()
    loop = LMLoop.for_sysid(mdl, u, xo, th, estimate_ini=IDX if ini else None, weights=np.ones(n) if weighted else None)
    assert mdl.lib.calls == []                                                      # nothing is launched before the first evaluation
    vector = np.concatenate([th, xo[:, 0][:, IDX].reshape(-1)]) if ini else th
    assert loop.theta.shape == vector.shape
    first = loop.evaluate(vector)
    a = the_call(mdl, "pdp_sysid_step_workspace_bytes")
    assert scalars(a) == expected
    assert first[0] == 0.0 and first[1].shape == vector.shape and first[2].shape == (vector.size, vector.size)      # (the recorder leaves zeros)
    loop.evaluate(vector + 1.0)
    b = the_call(mdl, "pdp_sysid_step_workspace_bytes")
    assert scalars(b) == expected
    for k in ("u", "xobs", "loss", "packed") + (("x0",) if ini else ()) + (("w",) if weighted else ()):
        assert a["ptr"][k] == b["ptr"][k], k                                        # data, weights, the initial states and the row stay where they are


BATCHED_SYSID = [
    ("BatchedLMLoop", False, False, dict(name="pdp_sysid_step_gn_batched", B=3, T=6, tb=3, flags=0, nbytes=0, null={"x0", "ws", "stream"})),
    ("BatchedLMLoop_weights", False, True,
     dict(name="pdp_sysid_step_wls_batched", B=3, T=6, ini_mask=0, wbs=0, delta=INF, tb=3, flags=0, nbytes=0, null={"x0", "ws", "stream"})),
    ("BatchedLMLoop_estimate_ini", True, False,
     dict(name="pdp_sysid_step_gn_ini_batched", B=3, T=6, ini_mask=10, tb=5, flags=0, nbytes=0, null={"ws", "stream"})),
    ("BatchedLMLoop_estimate_ini_weights", True, True,
     dict(name="pdp_sysid_step_wls_batched", B=3, T=6, ini_mask=10, wbs=0, delta=INF, tb=5, flags=0, nbytes=0, null={"ws", "stream"})),
]


@pytest.mark.parametrize("case", BATCHED_SYSID, ids=[c[0] for c in BATCHED_SYSID])
def test_batched_lm_loop_for_sysid_evaluates_with_one_call(monkeypatch, case):
    import torch
    from pdp_amd.irl import BatchedLMLoop
    _, ini, weighted, expected = case
    lr.stand_in_torch(monkeypatch)
    mdl = lr.stand_in_model()
    u, xo, th = sysid_data()
    loop = BatchedLMLoop.for_sysid(mdl, u, xo, th, estimate_ini=IDX if ini else None, weights=np.ones(n) if weighted else None)
    assert mdl.lib.calls == [] and tuple(loop.trial.shape) == (B, W if ini else p)
    rows, bad = loop.evaluate_rows(loop.trial)
    a = the_call(mdl, "pdp_sysid_step_workspace_bytes")
    assert scalars(a) == expected
    assert a["ptr"]["theta"] == loop.trial.data_ptr()                               # the parameters are read in place: from wide rows with stride W too
    width = W if ini else p
    assert tuple(rows.shape) == (B, width + 1 + width * width) and bad.dtype == torch.int32 and tuple(bad.shape) == (B,) and int(bad.sum()) == 0
    if ini:                                                                         # the estimated components travel from the trial rows into the persistent x0
        loop.trial[:, p:] = torch.arange(B * 2, dtype=torch.float64).view(B, 2) + 7.0
    loop.evaluate_rows(loop.trial)
    b = the_call(mdl, "pdp_sysid_step_workspace_bytes")
    assert scalars(b) == expected and b["ptr"] == a["ptr"]                          # every pointer stays: data, weights, x0, the row
    if ini:
        import ctypes
        x0 = np.ctypeslib.as_array((ctypes.c_double * (B * n)).from_address(b["ptr"]["x0"])).reshape(B, n)
        assert (x0[:, IDX] == np.arange(B * 2).reshape(B, 2) + 7.0).all() and (x0[:, [0, 2]] == xo[:, 0][:, [0, 2]]).all()


def _fixed_solve(mdl):
    """stands in for oc_solve_ms: fixed tensors, converged, no status bit"""
    import torch
    sol = dict(state=torch.zeros((B, T + 1, n), dtype=torch.float64), control=torch.zeros((B, T, m), dtype=torch.float64),
               costate=torch.zeros((B, T, n), dtype=torch.float64), converged_flags=torch.ones(B, dtype=torch.int32), status=torch.zeros(B, dtype=torch.int32))
    seen = []

    def solve(x0, theta, T_, **kw):
        seen.append(dict(kw, x0=x0, theta=theta, T=T_))
        return dict(sol)
    mdl.oc_solve_ms = solve
    return sol, seen


IRL = [
    ("LMLoop", "LMLoop", False, dict(name="pdp_oc_pdp_grad_batched", B=3, T=6, flags=17, tb=0, nbytes=0, null={"x0", "dxdp", "dudp", "stream"})),
    ("LMLoop_weights_state", "LMLoop", True,
     dict(name="pdp_oc_pdp_grad_wls_batched", B=3, T=6, flags=1, tb=0, wxs=0, wus=0, delta=INF, nbytes=0, null={"x0", "wu", "stream"})),
    ("BatchedLMLoop", "BatchedLMLoop", False, dict(name="pdp_oc_pdp_grad_batched", B=3, T=6, flags=17, tb=3, nbytes=0, null={"x0", "dxdp", "dudp", "stream"})),
    ("BatchedLMLoop_weights_state", "BatchedLMLoop", True,
     dict(name="pdp_oc_pdp_grad_wls_batched", B=3, T=6, flags=1, tb=3, wxs=0, wus=0, delta=INF, nbytes=0, null={"x0", "wu", "stream"})),
]


@pytest.mark.parametrize("case", IRL, ids=[c[0] for c in IRL])
def test_for_irl_evaluates_with_one_solve_and_one_call(monkeypatch, case):
    import torch
    from pdp_amd import irl
    _, cls, weighted, expected = case
    lr.stand_in_torch(monkeypatch)
    mdl = lr.stand_in_model()
    sol, seen = _fixed_solve(mdl)
    _, th, dx, du, _ = oc_data()
    loop = getattr(irl, cls).for_irl(mdl, dx, du, th, weights_state=np.ones(n) if weighted else None)
    assert mdl.lib.calls == [] and seen == []
    if cls == "LMLoop":
        loss, g, G = loop.evaluate(th)
        assert loss == 0.0 and g.shape == (p,) and G.shape == (p, p)
    else:
        rows, bad = loop.evaluate_rows(loop.trial)
        assert tuple(rows.shape) == (B, 13) and bad.dtype == torch.int32 and int(bad.sum()) == 0
    a = the_call(mdl, "pdp_oc_pdp_workspace_bytes")
    assert scalars(a) == expected
    assert len(seen) == 1 and seen[0]["T"] == T and seen[0]["warm"] is None and (np.asarray(seen[0]["x0"]) == dx[:, 0]).all()
    assert a["ptr"]["u"] == sol["control"].data_ptr() and a["ptr"]["x"] == sol["state"].data_ptr() and a["ptr"]["lam"] == sol["costate"].data_ptr()
    if cls == "BatchedLMLoop":
        assert a["ptr"]["theta"] == loop.trial.data_ptr()
        sol["status"][1] = 4                                                        # a solve status bit outside the informational ones: that sample is bad
        sol["converged_flags"][2] = 0
        assert loop.evaluate_rows(loop.trial)[1].tolist() == [0, 1, 1]
        sol["status"][:] = torch.tensor([128, 512, 1024 | 2048], dtype=torch.int32)  # informational bits alone are not
        sol["converged_flags"][2] = 1
        assert loop.evaluate_rows(loop.trial)[1].tolist() == [0, 0, 0]
    else:
        sol["status"][1] = 4
        assert loop.evaluate(th) is None
        sol["status"][1] = 128 | 512 | 1024 | 2048
        assert loop.evaluate(th) is not None
        sol["converged_flags"][0] = 0
        assert loop.evaluate(th) is None


# ---- the packed row from materialised sensitivities, to the bit ---------------------------------------------------------------------------------------------------
def _fallback_inputs():
    """seeded CPU tensors, B = 3, T = 4, n = 3, m = 2, W = 3: NaNs in the data, one NaN in a state at an OBSERVED entry, zeros among the weights, and a delta that
    leaves entries on both Huber branches"""
    import torch
    g = torch.Generator().manual_seed(11)
    Bf, Tf, nf, mf, Wf = 3, 4, 3, 2, 3
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x, u, demo_x, demo_u = r(Bf, Tf + 1, nf), r(Bf, Tf, mf), r(Bf, Tf + 1, nf), r(Bf, Tf, mf)
    X, U = r(Bf, Tf + 1, nf, Wf), r(Bf, Tf, mf, Wf)
    wx, wu = r(Bf, Tf + 1, nf).abs() + 0.1, r(Tf, mf).abs() + 0.1
    demo_x[0, 1, 2] = demo_x[2, 4, 0] = demo_x[1, 0, 1] = float("nan")
    demo_u[1, 2, 0] = demo_u[2, 3, 1] = float("nan")
    wx[0, 2, 1] = wx[1, 3, 0] = wx[0, 1, 2] = 0.0                                    # zeros on observed entries and on a missing one
    wu[1, 1] = 0.0
    x[1, 2, 2] = float("nan")                                                       # a state that is not finite where the data is observed and the weight positive
    assert not torch.isnan(demo_x[1, 2, 2]) and wx[1, 2, 2] > 0
    return Bf, Wf, x, u, demo_x, demo_u, X, U, wx, wu, 0.9


def test_packed_row_from_sensitivities_equals_the_five_expressions_to_the_bit():
    import torch
    from pdp_amd.runtime import packed_row_from_sensitivities as row_of
    Bf, Wf, x, u, demo_x, demo_u, X, U, wx, wu, delta = _fallback_inputs()
    both = (wx > 0) & ~torch.isnan(demo_x) & ~torch.isnan(x)
    e = (wx.sqrt() * (x - demo_x)).abs()[both]
    assert int((e <= delta).sum()) >= 3 and int((e > delta).sum()) >= 3                # both Huber branches occur
    new = lambda: torch.full((Bf, Wf + 1 + Wf * Wf), 7.0, dtype=torch.float64)
    same = lambda a, b: torch.equal(a.view(torch.int64), b.view(torch.int64))          # torch.equal on the bit patterns: the rows hold NaNs, on purpose

    def check(reference, sides, rule, **kw):
        want, got = new(), new()
        reference(want)
        row_of(got, sides, rule, **kw)
        assert same(want, got), (rule, kw)
        return want
    sysid = [(x, demo_x, None, X)]
    oc = lambda wxd, wud: [(x, demo_x, wxd, X), (u, demo_u, wud, U)]
    clean = torch.nan_to_num(demo_x, nan=0.25)
    check(lambda pk: lr.sysid_gn(pk, x, clean, X, Wf), [(x, clean, None, X)], "plain")
    check(lambda pk: lr.sysid_gn(pk, x, demo_x, X, Wf), sysid, "plain")                                         # (NaNs go through as they always did)
    miss = check(lambda pk: lr.sysid_gn_skip_missing(pk, x, demo_x, X, Wf), sysid, "missing_residual")
    assert torch.isnan(miss[1, Wf]) and not torch.isnan(miss[1, :Wf]).any() and not torch.isnan(miss[[0, 2]]).any()      # the NaN state shows in the loss alone
    for skip in (False, True):
        for d in (delta, INF):
            for w in (wx, wx[0], None):
                check(lambda pk: lr.sysid_weighted(pk, x, demo_x, X, Wf, w, d, skip), [(x, demo_x, w, X)], "weighted", delta=d, skip_missing=skip)
                check(lambda pk: lr.oc_weighted(pk, x, u, demo_x, demo_u, X, U, Wf, w, wu, d, skip), oc(w, wu), "weighted", delta=d, skip_missing=skip)
            check(lambda pk: lr.oc_weighted(pk, x, u, demo_x, demo_u, X, U, Wf, wx, None, d, skip), oc(wx, None), "weighted", delta=d, skip_missing=skip)
    ocm = check(lambda pk: lr.oc_gn_skip_missing(pk, x, u, demo_x, demo_u, X, U, Wf), oc(None, None), "missing_data")
    assert torch.isnan(ocm[1]).any() and not torch.isnan(ocm[[0, 2]]).any()                                      # the OC rule keeps that NaN in the gradient as well
