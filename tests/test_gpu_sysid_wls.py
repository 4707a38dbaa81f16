"""GPU: SysID.step as weighted and Huber-robust least squares (pdp_sysid_step_wls_batched; sysid_step_kernel / sysid_step2_kernel MODE 5 and 6) - the rows
grad [W] | loss | G [W][W] against the CPU reference of tests/sysid_wls_common.py (SysIDOracle + numpy) on all five systems, over every kernel the dispatch can pick at
the edges of their chunks, the size edges, the return codes, and the two Levenberg-Marquardt loops on it against the oracle's schedule.

Tolerance: TOL = 1e-10 relative to the largest entry of the reference row for every comparison with the reference and between kernels; exact
zeros where nothing is observed; G symmetric to the bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

import sysid_gn_common as sg
import sysid_ini_common as si
import sysid_wls_common as sw
from sysid_gn_common import TOL, rel_rows

pytestmark = pytest.mark.gpu
ROOT = sg.ROOT
INF = float("inf")
INI = {"pendulum": [1], "cartpole": [2, 3], "robotarm": [2, 3], "rocket": [3, 4, 5, 10, 11, 12], "quadrotor": [3, 4, 5, 10, 11, 12]}
CASES = ("weights", "zeros_nan", "flag", "huber", "ini_huber", "trivial", "shared", "nothing")
_ref = {}


def npy(t):
    return t.detach().cpu().numpy()


def model(system):
    from pdp_amd import zoo
    return zoo.get(system, "sysid")


def component_weights(n):
    return 1.0 / (0.5 + np.arange(n)) ** 2                 # w = 1 / sigma^2 with sigma = 0.5, 1.5, 2.5, ...


def median_delta(sid, inputs, states, theta, ini, w, skip_missing):
    """Huber's threshold at the median of the observed standardised residuals |e| of the first three samples (the reference is not rolled out for a whole batch): entries
    on both branches"""
    es = []
    for b in range(min(3, inputs.shape[0])):
        th = theta[b] if np.ndim(theta) == 2 else theta
        e = np.abs(np.sqrt(w[b]) * (sid.integrateDyn(ini[b], inputs[b], th) - states[b]))
        es.append(e[(w[b] > 0) & (~np.isnan(states[b]) if skip_missing else True) & (e > 0)])
    es = np.concatenate(es)
    delta = float(np.median(es))
    assert delta > 0 and (es <= delta).sum() >= 1 and (es > delta).sum() >= 1
    return delta


def build(system, name, inputs, states, theta):
    """the keywords of ModelLib.sysid_step (and of sysid_wls_common.reference_rows) of one case on the given data.  states: the recorded ones; a case writes its NaN
    into a copy."""
    sid = sg.oracle(system)
    B, T, n = inputs.shape[0], inputs.shape[1], states.shape[2]
    t_, i_ = np.meshgrid(np.arange(T + 1), np.arange(n), indexing="ij")
    wc = np.broadcast_to(component_weights(n), (B, T + 1, n)).copy()
    xo, kw = np.array(states, dtype=float), {}
    if name == "weights":                                   # (i) per-component weights only
        kw = dict(weights=component_weights(n))
    elif name == "zeros_nan":                               # (ii) weights with zeros, NaN in x_obs under the zeros, no flag
        zero = ((t_ + i_) % 3 == 0) & (t_ >= 1)
        wc[:, zero] = 0.0
        xo[:, zero] = np.nan
        kw = dict(weights=wc)
    elif name == "flag":                                    # (iii) the flag, NaN (row 0 and sample 1 not observed at all) and weights with zeros of their own
        xo = sg.mask_states(states)
        wc[:, (t_ + 2 * i_) % 5 == 0] = 0.0
        kw = dict(weights=wc, skip_missing=True, ini_state=states[:, 0].copy())
    elif name == "huber":                                   # (iv) Huber with entries on both branches, per-component weights
        kw = dict(weights=component_weights(n), huber_delta=median_delta(sid, inputs, states, theta, states[:, 0], wc, False))
    elif name == "ini_huber":                               # (v) estimate_ini with weights and Huber; the shifted start makes row 0 contribute
        ini = states[:, 0] + 0.01
        wc[:, (t_ + i_) % 4 == 3] = 0.0
        kw = dict(weights=wc, huber_delta=median_delta(sid, inputs, states, theta, ini, wc, False), ini_state=ini, estimate_ini=INI[system])
    elif name == "trivial":                                 # (vi) weights = NULL, delta off: the row of pdp_sysid_step_gn_ini_batched
        kw = dict(huber_delta=INF, ini_state=states[:, 0] + 0.01, estimate_ini=INI[system])
    elif name == "shared":                                  # (vii) one [T+1, n] block for the batch
        w2 = wc[0] * (1.0 + 0.1 * t_)
        w2[(t_ * i_) % 7 == 3] = 0.0
        kw = dict(weights=w2)
    elif name == "nothing":                                 # (viii) one sample with nothing observed (weights alone; its x_obs holds NaN and numbers)
        wc[1 % B] = 0.0
        xo[1 % B, 1::2] = np.nan
        kw = dict(weights=wc, huber_delta=0.5)
    return xo, kw


def reference(system, name, inputs, states, theta, samples=None):
    xo, kw = build(system, name, inputs, states, theta)
    return si.packed(sw.reference_rows(sg.oracle(system), inputs, xo, theta, kw.get("estimate_ini", ()), kw.get("ini_state"), kw.get("skip_missing", False),
                                       kw.get("weights"), kw.get("huber_delta", INF), samples))


def stored_reference(system, name):
    """computed once per case, shared by the tests, never written to"""
    if (system, name) not in _ref:
        inputs, states, _, theta = sg.stored(system)
        _ref[(system, name)] = reference(system, name, inputs, states, theta)
        _ref[(system, name)].setflags(write=False)
    return _ref[(system, name)]


def run(system, name, inputs, states, theta):
    xo, kw = build(system, name, inputs, states, theta)
    out = model(system).sysid_step(inputs, xo, theta, **kw)
    W = model(system).p + len(kw.get("estimate_ini", ()))
    assert tuple(out["packed_gn"].shape) == (inputs.shape[0], W + 1 + W * W) and out.get("ini_index", []) == list(kw.get("estimate_ini", []))
    return npy(out["packed_gn"]).copy()


def check_rows(margins, tag, system, name, rows, ref, samples=None):
    W = model(system).p + (len(INI[system]) if name in ("ini_huber", "trivial") else 0)
    got = rows if samples is None else rows[list(samples)]
    for part, sl in (("gradient", slice(0, W)), ("loss", slice(W, W + 1)), ("G", slice(W + 1, None))):
        margins.check("%s: %s" % (tag, part), rel_rows(got[:, sl], ref[:, sl]), TOL)
    margins.check("%s: row" % tag, rel_rows(got, ref), TOL)
    G = rows[:, W + 1:].reshape(len(rows), W, W)
    assert np.array_equal(G, np.swapaxes(G, 1, 2)), tag + ": G is not symmetric to the bit"
    assert np.isfinite(rows).all() and (np.diagonal(G, axis1=1, axis2=2) >= 0).all() and (rows[:, W] >= 0).all(), tag
    if name in ("flag", "nothing") and len(rows) > 1:
        assert not rows[1].any(), tag + ": the sample with nothing observed is not exact zeros in all W + 1 + W W entries"
        assert rows[0].any()


# ---- parity, all five systems, stored data (B = 3: the pair kernel with one trajectory per workgroup) ---------------------------------------------------------------------
@pytest.mark.parametrize("system", sg.SYSTEMS)
def test_parity_with_the_reference(margins, system):
    inputs, states, _, theta = sg.stored(system)
    mdl = model(system)
    for name in CASES:
        rows = run(system, name, inputs, states, theta)
        check_rows(margins, "SysID WLS %s, %s" % (system, name), system, name, rows, stored_reference(system, name))
    # (vi) against the entry point it extends, and with ini_mask = 0 against pdp_sysid_step_gn_batched's row
    ini = states[:, 0] + 0.01
    gn_ini = npy(mdl.sysid_step(inputs, states, theta, gauss_newton=True, ini_state=ini, estimate_ini=INI[system])["packed_gn"])
    margins.check("SysID WLS %s, trivial call vs pdp_sysid_step_gn_ini_batched" % system, rel_rows(run(system, "trivial", inputs, states, theta), gn_ini), TOL)
    for skip in (False, True):
        gn = npy(mdl.sysid_step(inputs, states, theta, gauss_newton=True, skip_missing=skip, ini_state=ini)["packed_gn"])
        got = npy(mdl.sysid_step(inputs, states, theta, huber_delta=INF, skip_missing=skip, ini_state=ini)["packed_gn"])
        margins.check("SysID WLS %s, trivial call, ini_mask = 0, skip_missing = %s vs pdp_sysid_step_gn_batched" % (system, skip), rel_rows(got, gn), TOL)
    # a NaN in x_obs at w > 0 without the flag shows in the loss, as it always did
    xo = states.copy()
    xo[0, 2, 0] = np.nan
    out = mdl.sysid_step(inputs, xo, theta, weights=component_weights(mdl.n), huber_delta=0.5)
    assert np.isnan(npy(out["loss"])[0]) and np.isfinite(npy(out["packed_gn"])[1:]).all()
    out = mdl.sysid_step(inputs, xo, theta, weights=component_weights(mdl.n), huber_delta=0.5, skip_missing=True)
    assert np.isfinite(npy(out["packed_gn"])).all()


# ---- every kernel of the dispatch at the chunk edges -----------------------------------------------------------------------------------------------------------------------
EDGE_CASES = ("flag", "ini_huber")                         # MODE 5 with the flag, NaN and zero weights; MODE 6 with Huber


def edge_data(system, B, T):
    """random inputs rolled out at the true parameter by the model's own integrator, a 5 % relative disturbance on top (so that no residual is zero), theta per sample.
    Not the stored recordings replicated: those end at T = 20 (pendulum) and T = 10 (quadrotor), short of the chunk of 32 steps whose edges the horizons sit at - the
    way tests/test_gpu_sysid_gn.py makes its edge cases.  The integrator only makes the data; what the rows are held to is the oracle's own rollout."""
    _, states, true_parameter, theta = sg.stored(system)
    rng = np.random.default_rng(100 * T + B)
    x0 = states[np.arange(B) % states.shape[0], 0] * (1.0 + 0.05 * rng.standard_normal((B, states.shape[2])))
    inputs = rng.uniform(-1.0, 1.0, (B, T, model(system).m))
    xs = npy(model(system).sysid_integrate(x0, inputs, true_parameter))
    assert np.isfinite(xs).all()
    xs[:, 1:] += 0.05 * rng.standard_normal(xs[:, 1:].shape) * (np.abs(xs[:, 1:]) + 0.1)
    return inputs, xs, theta[None] * (1.0 + 0.03 * rng.standard_normal((B, theta.size)))


def _edge_rows(system, horizons, batches):
    out = {}
    for T in horizons:
        for B in batches:
            inputs, states, theta = edge_data(system, B, T)
            for name in EDGE_CASES:
                out["%s_T%d_B%d_%s" % (system, T, B, name)] = run(system, name, inputs, states, theta)
    return out


def _check_edges(margins, tag, system, horizons, batches, rows, against=None):
    """samples 0, 1 and the last against the oracle; all samples against `against` (the same data in another process or through another kernel)"""
    for T in horizons:
        for B in batches:
            inputs, states, theta = edge_data(system, B, T)
            samples = sorted({0, 1, B - 1})
            for name in EDGE_CASES:
                key = "%s_T%d_B%d_%s" % (system, T, B, name)
                t = "%s: %s T = %d B = %d %s" % (tag, system, T, B, name)
                check_rows(margins, t + " vs oracle (samples 0, 1, last)", system, name, rows[key], reference(system, name, inputs, states, theta, samples), samples)
                if against is not None:
                    margins.check(t + " vs the pair kernel with one trajectory per workgroup (all samples)", rel_rows(rows[key], against(key, name, inputs, states, theta)), TOL)


def _sliced(system):
    """the same arrays in slices of 128 rows: the pair kernel with one trajectory per workgroup (the masks and weights are built once, for the full call, and sliced)"""
    def f(key, name, inputs, states, theta):
        xo, kw = build(system, name, inputs, states, theta)
        parts = []
        for i in range(0, inputs.shape[0], 128):
            sl = slice(i, min(i + 128, inputs.shape[0]))
            k2 = {k: (v[sl] if k in ("weights", "ini_state") and np.ndim(v) == (3 if k == "weights" else 2) else v) for k, v in kw.items()}
            parts.append(npy(model(system).sysid_step(inputs[sl], xo[sl], theta[sl], **k2)["packed_gn"]).copy())
        return np.concatenate(parts)
    return f


@pytest.mark.parametrize("system", ["pendulum", "quadrotor"])
def test_every_kernel_of_the_dispatch_at_the_chunk_edges(margins, system):
    """default dispatch: B = 3 pair kernel with one trajectory per workgroup, B = 301 pair kernel with two (the last workgroup's second slot is empty), B = 515 one-wave
    kernel; horizons of one step, one step less than a chunk, exactly a chunk, a chunk and a step; n = 2 (pendulum) and n = 13 (quadrotor)"""
    ch = model(system).chunk
    horizons, batches = (1, ch - 1, ch, ch + 1), (3, 301, 515)
    _check_edges(margins, "default dispatch", system, horizons, batches, _edge_rows(system, horizons, batches), _sliced(system))


SWITCHES = [("one-wave kernel at B = 3", dict(PDP_SYSID_VARIANT="1"), (3,)), ("pre-pass + GIVEN kernel at B = 3", dict(PDP_SYSID_PREPASS="1"), (3,)),
            ("pool of 4 rows", dict(PDP_SYSID_ROWS="4"), (3, 515))]


def _child(k, path):
    """in a subprocess (the switches are read once per process): the edge cases under SWITCHES[k] -> npz"""
    out = {}
    for system in ("pendulum", "quadrotor"):
        ch = model(system).chunk
        out.update(_edge_rows(system, (1, ch - 1, ch, ch + 1), SWITCHES[k][2]))
    np.savez(path, **out)


@pytest.mark.parametrize("k", range(len(SWITCHES)), ids=["one_wave", "prepass_given", "rows_4"])
def test_kernel_selecting_switches(margins, tmp_path, k):
    """PDP_SYSID_VARIANT=1, PDP_SYSID_PREPASS=1, PDP_SYSID_ROWS=4 - each in a fresh child process, held to the oracle (samples 0, 1, last) and to this process's default
    dispatch on the same data"""
    name, env, batches = SWITCHES[k]
    f = str(tmp_path / ("switch%d.npz" % k))
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_sysid_wls as m; m._child(%d, %r)" % (ROOT, os.path.join(ROOT, "tests"), k, f)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, "%s: %s" % (name, r.stdout[-3000:])
    res = np.load(f)
    for system in ("pendulum", "quadrotor"):
        ch = model(system).chunk
        _check_edges(margins, name, system, (1, ch - 1, ch, ch + 1), batches, res, lambda key, nm, inputs, states, theta: run(system, nm, inputs, states, theta))


# ---- size edges: user models through PDP.SysID --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder, fused", [(sg.chain_16_2_16, True), (sg.chain_5_1_17, False)], ids=["n16_m2_p16_fused", "n5_m1_p17_materialised"])
def test_size_edges_through_the_class_surface(margins, builder, fused):
    """(16, 2, 16): the largest model of the fused kernels (W = 16); (5, 1, 17): one parameter beyond them - the entry point answers PDP_E_SIZE and the same row comes
    from scaled residuals and row-scaled materialised sensitivities.  Both against SysIDOracle built from the same equations in sympy."""
    import sympy as sp
    from oracle import pdp_oracle as po
    from pdp_amd import PDP, runtime as rt
    from pdp_amd.sx import vertcat
    X, U, w, f = builder("sx")
    Xs, Us, ws_, fs = builder("sympy")
    n, m, p = len(Xs), len(Us), len(ws_)
    sid = PDP.SysID("sysid wls chain %d %d %d" % (n, m, p))
    sid.setAuxvarVariable(vertcat(*w))
    sid.setStateVariable(vertcat(*X))
    sid.setControlVariable(vertcat(*U))
    sid.setDyn(vertcat(*f))
    orc = po.SysIDOracle(sp.Matrix(Xs), sp.Matrix(Us), list(ws_), sp.Matrix(fs))
    rng = np.random.default_rng(n + p)
    B, T = 3, 9
    th_true, th = 1.0 + 0.3 * rng.uniform(-1, 1, p), 1.0 + 0.3 * rng.uniform(-1, 1, p)
    inputs, x0 = rng.uniform(-1, 1, (B, T, m)), 0.5 * rng.standard_normal((B, n))
    states = np.stack([orc.integrateDyn(x0[i], inputs[i], th_true) for i in range(B)])
    masked = sg.mask_states(states)
    wts = np.broadcast_to(component_weights(n), states.shape).copy()
    wts[:, 2::3, 1::2] = 0.0
    mdl = sid.model()
    if not fused:                                       # the entry point itself refuses the size, before any launch
        packed, loss = rt.dev(np.full((B, p + 1 + p * p), 7.0)), rt.dev(np.full((B,), 7.0))
        u_d, x_d, th_d, w_d = rt.dev(inputs), rt.dev(states), rt.dev(th), rt.dev(wts)
        rc = mdl.lib.pdp_sysid_step_wls_batched(B, T, rt.ptr(u_d), rt.ptr(x_d), None, 0, rt.ptr(w_d), (T + 1) * n, 0.5, rt.ptr(th_d), 0, 0, rt.ptr(loss), rt.ptr(packed), None, 0,
                                                rt.current_stream_ptr())
        assert rc == -2 and float(packed.min()) == 7.0 and float(loss.min()) == 7.0
    tag = "SysID WLS chain (%d, %d, %d)" % (n, m, p)
    delta = median_delta(orc, inputs, states, th, states[:, 0], wts, False)
    out = sid.step_batch(inputs, states, th, weights=wts, huber_delta=delta)
    assert tuple(out["packed_gn"].shape) == (B, p + 1 + p * p)
    margins.check(tag + " weights + Huber", rel_rows(npy(out["packed_gn"]), si.packed(sw.reference_rows(orc, inputs, states, th, (), None, False, wts, delta))), TOL)
    G = npy(out["gn"])
    assert np.array_equal(G, np.swapaxes(G, 1, 2))
    out = sid.step_batch(inputs, masked, th, skip_missing=True, ini_state=x0, weights=wts, huber_delta=delta)
    margins.check(tag + " masked, weights + Huber", rel_rows(npy(out["packed_gn"]), si.packed(sw.reference_rows(orc, inputs, masked, th, (), x0, True, wts, delta))), TOL)
    assert not npy(out["packed_gn"])[1].any()
    if not fused:                                       # and with an estimated component: W = 18
        out = sid.step_batch(inputs, states, th, ini_state=x0 + 0.01, estimate_ini=[0], weights=wts, huber_delta=delta)
        assert tuple(out["packed_gn"].shape) == (B, 18 + 1 + 18 * 18)
        margins.check(tag + " {0}, weights + Huber", rel_rows(npy(out["packed_gn"]), si.packed(sw.reference_rows(orc, inputs, states, th, [0], x0 + 0.01, False, wts, delta))), TOL)


# ---- argument errors on the GPU ------------------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_write_nothing():
    """(PDP_E_MODE of an OC library needs no GPU: tests/test_sysid_wls_host.py)"""
    from pdp_amd import runtime as rt
    import torch
    mdl = model("cartpole")
    inputs, states, _, theta = sg.stored("cartpole")
    B, T, n, W = inputs.shape[0], inputs.shape[1], mdl.n, mdl.p + 2
    u, xo, th, w = rt.dev(inputs), rt.dev(states), rt.dev(theta), rt.dev(np.ones(states.shape))
    packed, loss = rt.dev(np.full((B, W + 1 + W * W), 7.0)), rt.dev(np.full((B,), 7.0))
    P, st, full = rt.ptr, rt.current_stream_ptr(), (T + 1) * n
    fn = mdl.lib.pdp_sysid_step_wls_batched
    for a in ((B, T, P(u), P(xo), None, 12, P(w), full, 0.0), (B, T, P(u), P(xo), None, 12, P(w), full, -1.0), (B, T, P(u), P(xo), None, 12, P(w), full, float("nan")),
              (B, T, P(u), P(xo), None, 12, P(w), n, 0.5), (B, T, P(u), P(xo), None, 12, P(w), full + 1, 0.5), (B, T, P(u), P(xo), None, 12, None, 1, INF),
              (B, T, P(u), P(xo), None, 1 << 4, P(w), full, 0.5), (0, T, P(u), P(xo), None, 12, P(w), full, 0.5), (B, 0, P(u), P(xo), None, 0, P(w), full, 0.5),
              (B, T, None, P(xo), None, 12, P(w), full, 0.5), (B, T, P(u), None, None, 0, P(w), full, 0.5)):
        assert fn(*a, P(th), 0, 0, P(loss), P(packed), None, 0, st) == -1, a[5:]
    for flags in (1, 16, 64):
        assert fn(B, T, P(u), P(xo), None, 12, P(w), full, 0.5, P(th), 0, flags, P(loss), P(packed), None, 0, st) == -1
    assert fn(B, T, P(u), P(xo), None, 12, P(w), full, 0.5, None, 0, 0, P(loss), P(packed), None, 0, st) == -1
    assert fn(B, T, P(u), P(xo), None, 12, P(w), full, 0.5, P(th), 0, 0, None, P(packed), None, 0, st) == -1
    assert fn(B, T, P(u), P(xo), None, 12, P(w), full, 0.5, P(th), 0, 0, P(loss), None, None, 0, st) == -1
    torch.cuda.synchronize()
    assert float(packed.min()) == 7.0 and float(packed.max()) == 7.0 and float(loss.min()) == 7.0 and float(loss.max()) == 7.0
    assert fn(B, T, P(u), P(xo), None, 12, P(w), full, 0.5, P(th), 0, 0, P(loss), P(packed), None, 0, st) == 0       # (and the same buffers are written by a valid call)
    torch.cuda.synchronize()
    assert float((packed == 7.0).sum()) == 0.0 and torch.equal(loss, packed[:, W])
    for kw, match in ((dict(weights=-np.ones(n)), "weights"), (dict(weights=np.full(n, np.nan)), "weights"), (dict(huber_delta=0.0), "huber_delta"),
                      (dict(weights=rt.dev(-np.ones(states.shape))), "weights")):
        with pytest.raises(ValueError, match=match):
            mdl.sysid_step(inputs, states, theta, **kw)
    with pytest.raises(ValueError, match="ini_state"):
        mdl.sysid_step(inputs, sg.mask_states(states), theta, weights=np.ones(n), skip_missing=True)        # row 0 is not observed and no ini_state is given


# ---- the wiring of the Python evaluation: every mode's entry point with hand-built arguments, to the bit ---------------------------------------------------------------
WIRING = [("gn", dict()), ("gn_flag", dict(skip_missing=True)), ("ini", dict(estimate_ini=[1, 3])), ("ini_flag", dict(estimate_ini=[1, 3], skip_missing=True)),
          ("weights_delta", dict(weights=True, huber_delta=0.05)), ("weights_ini", dict(weights=True, estimate_ini=[1, 3]))]


@pytest.mark.parametrize("theta_form", ["shared", "per_sample", "wide_rows"])
@pytest.mark.parametrize("mode", WIRING, ids=[w[0] for w in WIRING])
def test_python_evaluation_launches_the_entry_point_with_these_arguments(mode, theta_form):
    """Cart-pole, B = 5 (odd: the tail of the trajectories-per-workgroup split), T = 7.  The rows of ModelLib.sysid_rows_prepared's evaluation - what sysid_step and the
    Levenberg-Marquardt loops run - are torch.equal to the rows of a direct ctypes call of the mode's entry point with hand-built arguments: both launch the same
    deterministic kernel.  theta [p] shared, [B, p] per sample, or wide rows [B, W] = theta_b | x0_b[idx] read in place with stride W (without estimated components
    W = p: the per-sample rows of a tensor that is passed as it is)."""
    import torch
    from pdp_amd import runtime as rt
    _, kw = mode
    mdl = model("cartpole")
    theta = sg.stored("cartpole")[3]
    B, T, n, p = 5, 7, mdl.n, mdl.p
    rng = np.random.default_rng(5)                                                  # (the stored recordings are three: five short ones around rest instead)
    inputs, states = 0.5 * rng.standard_normal((B, T, mdl.m)), 0.1 * rng.standard_normal((B, T + 1, n))
    skip, idx = kw.get("skip_missing", False), kw.get("estimate_ini", [])
    W, mask = p + len(idx), sum(1 << i for i in idx)
    x0 = states[:, 0] + 0.01
    if skip:
        states[:, 2::3, 1] = np.nan
    w = None
    if kw.get("weights"):
        w = np.broadcast_to(component_weights(n), (B, T + 1, n)).copy()
        w[:, 1::4, 2] = 0.0
    delta = kw.get("huber_delta")
    theta_b = theta[None] * (1.0 + 0.02 * rng.standard_normal((B, p)))
    rows, held = mdl.sysid_rows_prepared(inputs, states, skip, x0, idx, w, delta, own_x0=True)
    if theta_form == "shared":
        given, th_d, tb = theta, rt.dev(theta), 0
    elif theta_form == "per_sample":
        given = th_d = rt.dev(theta_b)
        tb = p
    else:
        given = th_d = rt.dev(np.concatenate([theta_b, x0[:, idx] + 0.02], axis=1))
        tb = W
    got = rows(given)["packed_gn"].clone()
    assert tuple(got.shape) == (B, W + 1 + W * W)
    x0_d = rt.dev(x0)
    if theta_form == "wide_rows" and idx:
        x0_d[:, idx] = th_d[:, p:]
        assert torch.equal(held["x0"], x0_d)                                          # the estimated components went from the rows into the persistent x0
    u_d, xo_d = rt.dev(inputs), rt.dev(states)
    packed, loss = torch.full((B, W + 1 + W * W), 7.0, dtype=torch.float64, device="cuda"), torch.full((B,), 7.0, dtype=torch.float64, device="cuda")
    P, st, flags = rt.ptr, rt.current_stream_ptr(), 32 if skip else 0
    if w is not None:
        w_d = rt.dev(w)
        rc = mdl.lib.pdp_sysid_step_wls_batched(B, T, P(u_d), P(xo_d), P(x0_d), mask, P(w_d), (T + 1) * n, INF if delta is None else delta, P(th_d), tb, flags, P(loss),
                                                P(packed), None, 0, st)
    elif idx:
        rc = mdl.lib.pdp_sysid_step_gn_ini_batched(B, T, P(u_d), P(xo_d), P(x0_d), mask, P(th_d), tb, flags, P(loss), P(packed), None, 0, st)
    else:
        rc = mdl.lib.pdp_sysid_step_gn_batched(B, T, P(u_d), P(xo_d), P(x0_d), P(th_d), tb, flags, P(loss), P(packed), None, 0, st)
    assert rc == 0
    assert torch.isfinite(packed).all() and float(packed.abs().max()) > 0 and torch.equal(got, packed)


# ---- Levenberg-Marquardt -----------------------------------------------------------------------------------------------------------------------------------------------
def _print(tag, orc, r):
    print("%s\n  oracle %d evaluations, %d rejected: %s\n  GPU    %d evaluations, %d rejected: %s" % (tag, orc["evaluations"], orc["rejected"], " ".join("%.3e" % v for v in orc["loss_trace"]),
                                                                                                   r["evaluations"], r["rejected"], " ".join("%.3e" % v for v in r["loss_trace"])))


@pytest.mark.parametrize("system", sorted(sw.TRUST_COUNTS))
def test_lm_loop_with_trust_weights_follows_the_oracle_schedule(system):
    from pdp_amd.irl import LMLoop
    c, orc = sw.corrupted(system), sw.oracle_lm(system, "trust", loss_tol=1e-16)
    r = LMLoop.for_sysid(model(system), c["inputs"], c["states"], c["theta0"], ini_state=c["ini_state"], weights=c["trust"]).run(max_evals=50, loss_tol=1e-16)
    _print("%s, trust weights" % system, orc, r)
    assert r["evaluations"] <= 2 * orc["evaluations"] and not r["stalled"]
    assert r["loss_trace"][-1] <= 1e-10 and (np.diff(r["loss_trace"]) < 0).all()
    assert sw.theta_error(r, system) <= 1e-6


@pytest.mark.parametrize("system", ["pendulum", "cartpole"])
def test_lm_loop_with_huber_is_ten_times_closer_than_plain_least_squares(system):
    from pdp_amd.irl import LMLoop
    c, mdl = sw.corrupted(system), model(system)
    orc = sw.oracle_lm(system, None, sw.HUBER_DELTA)
    plain = LMLoop.for_sysid(mdl, c["inputs"], c["states"], c["theta0"], ini_state=c["ini_state"]).run(max_evals=50, loss_tol=1e-20)
    r = LMLoop.for_sysid(mdl, c["inputs"], c["states"], c["theta0"], ini_state=c["ini_state"], huber_delta=sw.HUBER_DELTA).run(max_evals=50, loss_tol=1e-20)
    _print("%s, Huber delta = %g" % (system, sw.HUBER_DELTA), orc, r)
    e0, e1 = sw.theta_error(plain, system), sw.theta_error(r, system)
    print("  |theta - theta*|: plain least squares %.2e, Huber %.2e" % (e0, e1))
    assert r["evaluations"] <= 2 * orc["evaluations"]
    assert e1 * 10 <= e0


def test_lm_loop_with_estimate_ini_weights_and_huber():
    """LMLoop.for_sysid(estimate_ini=, weights=, huber_delta=) evaluates the row of the reference: its first evaluation against sysid_wls_common, and the loss decreases"""
    from pdp_amd.irl import LMLoop, arrow_normal_equations
    import torch
    system, idx = "cartpole", [2, 3]
    c, mdl, sid = sw.corrupted(system), model(system), sg.oracle(system)
    ini = c["ini_state"].copy()
    ini[:, idx] = 0.0
    loop = LMLoop.for_sysid(mdl, c["inputs"], c["states"], c["theta0"], ini_state=ini, estimate_ini=idx, weights=c["trust"], huber_delta=0.5)
    r = loop.run(max_evals=12)
    rows = sw.reference_rows(sid, c["inputs"], c["states"], c["theta0"], idx, ini, False, c["trust"], 0.5)
    flat = arrow_normal_equations(torch.as_tensor(si.packed(rows)), mdl.p, 2).numpy()
    N = mdl.p + 3 * 2
    assert abs(r["loss_trace"][0] - flat[N]) <= TOL * flat[N] and (np.diff(r["loss_trace"]) < 0).all() and len(r["loss_trace"]) >= 3
    theta, x0 = loop.split(r["parameter_trace"][-1])
    print("cartpole, estimate_ini + trust weights + Huber 0.5: %s; |theta - theta*| %.2e |x0 - x0*| %.2e" % (" ".join("%.3e" % v for v in r["loss_trace"]),
                                                                                                           np.abs(theta - c["true_parameter"]).max(), np.abs(x0 - c["ini_state"]).max()))


@pytest.mark.parametrize("system", ["pendulum", "cartpole"])
def test_batched_lm_loop_with_trust_weights_and_huber(system):
    """BatchedLMLoop.for_sysid beside the oracle schedule on the corrupted recordings, in both groupings.
    One problem of the three recordings (samples_per_problem = 3): the problem of LMLoop.for_sysid and of sysid_wls_common.oracle_lm - trust weights converge to theta*,
    Huber at delta = 0.01 ends ten times closer than plain least squares, each in at most twice the oracle's evaluations.
    One problem per recording (K = 3), each beside the oracle schedule on that recording alone: the same assertions, with one reasoned exception - a recording that holds
    no corrupted entry (the pendulum's second: sysid_wls_common.corrupted()["mask"][1] is empty) has nothing for Huber to gain, both runs converge, and there both
    parameter errors are held to 1e-6 instead of to the factor 10.  Then estimate_ini with the trust weights."""
    from pdp_amd.irl import BatchedLMLoop
    c, mdl = sw.corrupted(system), model(system)
    star = c["true_parameter"]

    def run(tol, S=1, **kw):
        return BatchedLMLoop.for_sysid(mdl, c["inputs"], c["states"], c["theta0"], samples_per_problem=S, ini_state=c["ini_state"], max_evals=50, loss_tol=tol, **kw).run()
    # ---- the three recordings as one problem
    orc_t, orc_h = sw.oracle_lm(system, "trust", loss_tol=1e-16), sw.oracle_lm(system, None, sw.HUBER_DELTA)
    trust, plain, robust = run(1e-16, 3, weights=c["trust"]), run(1e-20, 3), run(1e-20, 3, huber_delta=sw.HUBER_DELTA)
    e0, e1 = np.abs(plain["theta"][0] - star).max(), np.abs(robust["theta"][0] - star).max()
    print("%s, one problem of 3 recordings: trust weights oracle %d evaluations, GPU %d, %s, loss %.3e; Huber oracle %d (%d rejected), GPU %d (%d), %s; "
          "|theta - theta*| plain %.2e Huber %.2e" % (system, orc_t["evaluations"], trust["evaluations"][0], trust["state"][0], trust["loss"][0], orc_h["evaluations"],
                                                    orc_h["rejected"], robust["evaluations"][0], robust["rejected"][0], robust["state"][0], e0, e1))
    assert trust["state"][0] == "CONVERGED" and trust["evaluations"][0] <= 2 * orc_t["evaluations"] and trust["loss"][0] <= 1e-10
    assert np.abs(trust["theta"][0] - star).max() <= 1e-6
    assert robust["evaluations"][0] <= 2 * orc_h["evaluations"]
    assert e1 * 10 <= e0
    # ---- one problem per recording
    trust, plain, robust = run(1e-16, weights=c["trust"]), run(1e-20), run(1e-20, huber_delta=sw.HUBER_DELTA)
    for k in range(3):
        orc_t, orc_h = _oracle_trajectory(system, k, c["trust"][k:k + 1], INF, 1e-16), _oracle_trajectory(system, k, None, sw.HUBER_DELTA, 1e-20)
        e0, e1 = np.abs(plain["theta"][k] - star).max(), np.abs(robust["theta"][k] - star).max()
        print("%s, recording %d (%d corrupted entries): trust weights oracle %d evaluations, GPU %d (%d rejected) %s, loss %.3e; Huber oracle %d (%d rejected), GPU %d (%d) %s; "
              "|theta - theta*| plain %.2e Huber %.2e" % (system, k, c["mask"][k].sum(), orc_t["evaluations"], trust["evaluations"][k], trust["rejected"][k], trust["state"][k],
                                                        trust["loss"][k], orc_h["evaluations"], orc_h["rejected"], robust["evaluations"][k], robust["rejected"][k],
                                                        robust["state"][k], e0, e1))
        assert trust["state"][k] == "CONVERGED" and trust["evaluations"][k] <= 2 * orc_t["evaluations"] and trust["loss"][k] <= 1e-10, k
        assert robust["evaluations"][k] <= 2 * orc_h["evaluations"], k
        if c["mask"][k].any():
            assert e1 * 10 <= e0, k
        else:
            assert e0 <= 1e-6 and e1 <= 1e-6, k
    assert np.abs(trust["theta"] - star).max() <= 1e-6
    if system == "cartpole":
        ini = c["ini_state"].copy()
        ini[:, [2, 3]] = 0.0
        loop = BatchedLMLoop.for_sysid(mdl, c["inputs"], c["states"], c["theta0"], ini_state=ini, estimate_ini=[2, 3], weights=c["trust"], max_evals=50, loss_tol=1e-16)
        r = loop.run()
        theta, x0 = loop.split(r["theta"])
        print("estimate_ini + trust weights: %s evaluations, %s, losses %s" % (r["evaluations"], r["state"], r["loss"]))
        assert all(st == "CONVERGED" for st in r["state"]) and np.abs(theta - star).max() <= 1e-6 and np.abs(x0 - c["ini_state"]).max() <= 1e-6


def _oracle_trajectory(system, b, w, delta, loss_tol):
    from pdp_amd.irl import LMLoop
    c, sid = sw.corrupted(system), sg.oracle(system)

    def evaluate(theta):
        loss, grad, G = sw.reference_rows(sid, c["inputs"][b:b + 1], c["states"][b:b + 1], theta, (), c["ini_state"][b:b + 1], False, w, delta)
        return loss[0], grad[0], G[0]
    return LMLoop(evaluate, c["theta0"]).run(max_evals=50, loss_tol=loss_tol)


# ---- the example ---------------------------------------------------------------------------------------------------------------------------------------------------------
def test_example_with_weights_huber_and_outliers():
    args = ["--system", "cartpole", "--method", "lm", "--noise-sigma", "1e-3,1e-3,1e-2,1e-2", "--huber", "3", "--outliers", "0.05"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "sysid_pdp.py")] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    lines = r.stdout.splitlines()
    done = [ln for ln in lines if ln.startswith("done:")]
    assert len(done) == 1 and len([ln for ln in lines if ln.startswith("accepted")]) >= 2, r.stdout[-3000:]
    first, last = (float(v) for v in done[0].split("loss ")[-1].split(";")[0].split(" -> "))
    assert last < first, r.stdout[-3000:]
