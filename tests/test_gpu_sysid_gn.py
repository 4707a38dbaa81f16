"""GPU: SysID.step as a nonlinear least-squares evaluation (pdp_sysid_step_gn_batched; sysid_step_kernel / sysid_step2_kernel MODE 1 and 2) - loss, gradient and the
Gauss-Newton matrix G = sum_t X_t' X_t per trajectory, complete data and data with gaps (NaN = not observed), a given initial state - against the CPU reference of
tests/sysid_gn_common.py (SysIDOracle + numpy), over every kernel the dispatch can pick and the edges of their tiles and chunks; the Levenberg-Marquardt loop on it
(irl.LMLoop.for_sysid) against the oracle's schedule; the example driver.

Tolerance: TOL = 1e-10 relative to the largest entry per sample, for every comparison of this file - against the oracle, between kernels and
between modes (the modes and kernels order the same sums the same way, but nothing here relies on the compiler contracting them alike)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import sysid_gn_common as sg
from sysid_gn_common import TOL, rel_rows

pytestmark = pytest.mark.gpu
ROOT = sg.ROOT
SLICE = 64                      # batches of at most this many trajectories take the pair kernel with ONE trajectory per workgroup (B <= number of CUs): the "B = 3 path"


def npy(t):
    return t.detach().cpu().numpy()


def model(system):
    from pdp_amd import zoo
    return zoo.get(system, "sysid")


def chunk(system):
    from pdp_amd import codegen, zoo
    return int(codegen.generate(zoo.make_problem(system, "sysid"))[1]["chunk"])


def make_case(system, B, T, seed):
    """inputs, complete states, the masked states (tests/sysid_gn_common.mask_states), an initial state and theta [p] (B = 3) or [B, p] (per-sample perturbations).
    The stored data where (B, T) is the stored shape, else random inputs rolled out at the true parameter by the model's own integrator."""
    inputs, states, true_parameter, theta = sg.stored(system)
    rng = np.random.default_rng(seed)
    if (B, T) != inputs.shape[:2]:
        x0 = states[np.arange(B) % states.shape[0], 0] * (1.0 + 0.05 * rng.standard_normal((B, states.shape[2])))
        inputs = rng.uniform(-1.0, 1.0, (B, T, inputs.shape[2]))
        states = npy(model(system).sysid_integrate(x0, inputs, true_parameter))
        assert np.isfinite(states).all()
    if B > 3:
        theta = theta[None] * (1.0 + 0.03 * rng.standard_normal((B, theta.size)))
    return dict(system=system, inputs=inputs, states=states, masked=sg.mask_states(states), ini=states[:, 0].copy(), theta=theta)


def run(mdl, c, masked, gauss_newton=True, shifted=0.0, sl=slice(None)):
    """numpy (loss [B], grad [B,p], G [B,p,p] or None) of one call on the samples sl"""
    th = c["theta"][sl] if np.ndim(c["theta"]) == 2 else c["theta"]
    kw = dict(skip_missing=True, ini_state=c["ini"][sl]) if masked else {}
    if shifted:
        kw["ini_state"] = c["ini"][sl] + shifted
    out = mdl.sysid_step(c["inputs"][sl], (c["masked"] if masked else c["states"])[sl], th, gauss_newton=gauss_newton, **kw)
    if gauss_newton:
        return npy(out["loss"]), npy(out["grad"]), npy(out["gn"])
    return npy(out[0]), npy(out[1]), None


def reference(c, masked, samples=None, shifted=0.0):
    ini = c["ini"] + shifted if (masked or shifted) else None
    return sg.reference_rows(sg.oracle(c["system"]), c["inputs"], c["masked"] if masked else c["states"], c["theta"], ini, masked, samples)


def check_rows(margins, tag, got, ref, samples=None):
    """loss (relative), gradient and G rows within TOL of the reference rows; G symmetric to the bit; an unobserved sample exact zeros"""
    pick = (lambda a: a) if samples is None else (lambda a: a[list(samples)])
    loss, grad, G = (pick(a) for a in got)
    margins.check(tag + ": loss", rel_rows(loss[:, None], ref[0][:, None]), TOL)
    margins.check(tag + ": gradient", rel_rows(grad, ref[1]), TOL)
    margins.check(tag + ": G", rel_rows(G, ref[2]), TOL)
    assert np.array_equal(got[2], np.swapaxes(got[2], 1, 2)), tag + ": G is not symmetric to the bit"


def check_unobserved_sample(tag, got):
    assert got[0][1] == 0.0 and not got[1][1].any() and not got[2][1].any(), tag + ": the sample with nothing observed is not exact zeros"


# ---- parity, all five systems, stored data ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("system", sg.SYSTEMS)
def test_parity_with_the_reference(margins, system):
    mdl = model(system)
    c = make_case(system, *sg.stored(system)[0].shape[:2], seed=1)
    tag = "SysID GN %s" % system
    gn, ref = run(mdl, c, False), reference(c, False)
    check_rows(margins, tag + ", complete data (MODE 1)", gn, ref)
    assert np.isfinite(gn[2]).all() and (np.diagonal(gn[2], axis1=1, axis2=2) >= 0).all()
    plain = run(mdl, c, False, gauss_newton=False)                                   # today's call: pdp_sysid_step_ws_batched
    margins.check(tag + ": loss column vs the plain call", rel_rows(gn[0][:, None], plain[0][:, None]), TOL)
    margins.check(tag + ": gradient columns vs the plain call", rel_rows(gn[1], plain[1]), TOL)
    out2 = mdl.sysid_step(c["inputs"], c["states"], c["theta"], gauss_newton=True, skip_missing=True)      # MODE 2 on NaN-free data
    margins.check(tag + ": MODE 2 vs MODE 1 on NaN-free data, packed row", rel_rows(npy(out2["packed_gn"]), np.concatenate([gn[1], gn[0][:, None], gn[2].reshape(len(gn[0]), -1)], 1)), TOL)
    l2, g2 = mdl.sysid_step(c["inputs"], c["states"], c["theta"], skip_missing=True)[:2]                     # skip_missing alone: (loss, grad) of the same launch
    assert np.array_equal(npy(l2), npy(out2["loss"])) and np.array_equal(npy(g2), npy(out2["grad"]))
    # a given initial state that is not the first observed row: row 0 adds |x0 - x_obs_0|^2 to the loss, nothing to gradient and G
    sh = run(mdl, c, False, shifted=0.01)
    check_rows(margins, tag + ", complete data, ini_state = x_obs_0 + 0.01", sh, reference(c, False, shifted=0.01))
    # every second step, every second component, row 0 unobserved (ini_state given), sample 1 with nothing observed
    ms = run(mdl, c, True)
    check_rows(margins, tag + ", masked data (MODE 2)", ms, reference(c, True))
    check_unobserved_sample(tag, ms)
    lm, gm = mdl.sysid_step(c["inputs"], c["masked"], c["theta"], skip_missing=True, ini_state=c["ini"])[:2]
    assert np.array_equal(npy(lm), ms[0]) and np.array_equal(npy(gm), ms[1])


# ---- every kernel of the dispatch, tile and chunk edges -------------------------------------------------------------------------------------------------------------------
def _edge_cases(system, horizons, batches, margins=None, tag=""):
    """runs complete (MODE 1) and masked (MODE 2, ini_state) data at every (T, B); returns {key: rows}; with `margins` checks them: samples 0, 1, last against the oracle,
    and for B > SLICE all samples against the same data run in slices of SLICE (the pair kernel with one trajectory per workgroup)"""
    mdl, out = model(system), {}
    for T in horizons:
        for B in batches:
            c = make_case(system, B, T, seed=100 * T + B)
            for masked in (False, True):
                got = run(mdl, c, masked)
                out["%s_T%d_B%d_%s" % (system, T, B, "masked" if masked else "complete")] = np.concatenate([got[1], got[0][:, None], got[2].reshape(B, -1)], 1)
                if margins is None:
                    continue
                t = "%s %s T = %d B = %d %s" % (tag, system, T, B, "masked" if masked else "complete")
                samples = sorted({0, 1, B - 1})
                check_rows(margins, t + " vs oracle (samples 0, 1, last)", got, reference(c, masked, samples), samples)
                if masked:
                    check_unobserved_sample(t, got)
                if B > SLICE:
                    parts = [run(mdl, c, masked, sl=slice(i, min(i + SLICE, B))) for i in range(0, B, SLICE)]
                    small = tuple(np.concatenate([pt[k] for pt in parts]) for k in range(3))
                    check_rows(margins, t + " vs the one-trajectory-per-workgroup pair kernel (all samples)", got, small)
    return out


@pytest.mark.parametrize("system", ["pendulum", "quadrotor"])
def test_every_kernel_of_the_dispatch_at_the_chunk_edges(margins, system):
    """default dispatch: B = 3 pair kernel with one trajectory per workgroup, B = 259 pair kernel with two (the odd tail slot), B = 515 one-wave kernel; horizons of one
    step, exactly one chunk, two chunks and a step; n = 2 (pendulum) and n = 13 (quadrotor)"""
    ch = chunk(system)
    _edge_cases(system, (1, ch, 2 * ch + 1), (3, 259, 515), margins, "default dispatch")


SWITCHES = [("one-wave kernel at B = 3", dict(PDP_SYSID_VARIANT="1"), (3,)), ("pre-pass + GIVEN kernel at B = 3", dict(PDP_SYSID_PREPASS="1"), (3,)),
            ("pool of 4 rows", dict(PDP_SYSID_ROWS="4"), (3, 515))]


def _child(k, path):
    """in a subprocess (the switches are read once per process): the edge cases under SWITCHES[k] -> npz"""
    out = {}
    for system in ("pendulum", "quadrotor"):
        ch = chunk(system)
        out.update(_edge_cases(system, (1, ch, 2 * ch + 1), SWITCHES[k][2]))
    np.savez(path, **out)


def test_kernel_selecting_switches(margins, tmp_path):
    """PDP_SYSID_VARIANT=1 (one wavefront per trajectory), PDP_SYSID_PREPASS=1 (rollout beforehand from ini_state + the GIVEN kernel), PDP_SYSID_ROWS=4 (many chunks, the
    last one shorter) - each in a child process, each held to the oracle (samples 0, 1, last) and to this process's default dispatch on the same data"""
    for k, (name, env, batches) in enumerate(SWITCHES):
        f = str(tmp_path / ("switch%d.npz" % k))
        code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_sysid_gn as m; m._child(%d, %r)" % (ROOT, os.path.join(ROOT, "tests"), k, f)
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert r.returncode == 0, "%s: %s" % (name, r.stdout[-3000:])
        res = np.load(f)
        for system in ("pendulum", "quadrotor"):
            mdl, ch = model(system), chunk(system)
            p = mdl.p
            for T in (1, ch, 2 * ch + 1):
                for B in batches:
                    c = make_case(system, B, T, seed=100 * T + B)
                    for masked in (False, True):
                        row = res["%s_T%d_B%d_%s" % (system, T, B, "masked" if masked else "complete")]
                        got = (row[:, p], row[:, :p], row[:, p + 1:].reshape(B, p, p))
                        t = "%s: %s T = %d B = %d %s" % (name, system, T, B, "masked" if masked else "complete")
                        samples = sorted({0, 1, B - 1})
                        check_rows(margins, t + " vs oracle (samples 0, 1, last)", got, reference(c, masked, samples), samples)
                        if masked:
                            check_unobserved_sample(t, got)
                        check_rows(margins, t + " vs the default dispatch (all samples)", got, run(mdl, c, masked))


# ---- size edges: user models through PDP.SysID --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder, fused", [(sg.chain_16_2_16, True), (sg.chain_5_1_17, False)], ids=["n16_m2_p16_fused", "n5_m1_p17_materialised"])
def test_size_edges_through_the_class_surface(margins, builder, fused):
    """(16, 2, 16): the largest model of the fused kernels; (5, 1, 17): one parameter beyond them - the entry point answers PDP_E_SIZE and the same row is contracted
    from the materialised sensitivities.  Both against SysIDOracle built from the same equations in sympy."""
    import sympy as sp
    from oracle import pdp_oracle as po
    from pdp_amd import PDP, runtime as rt
    from pdp_amd.sx import vertcat
    X, U, w, f = builder("sx")
    Xs, Us, ws_, fs = builder("sympy")
    n, m, p = len(Xs), len(Us), len(ws_)
    sid = PDP.SysID("sysid gn chain %d %d %d" % (n, m, p))
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
    mdl = sid.model()
    if not fused:                                       # the entry point itself refuses the size, before any launch
        packed, loss = rt.dev(np.full((B, p + 1 + p * p), 7.0)), rt.dev(np.full((B,), 7.0))
        u_d, x_d, th_d = rt.dev(inputs), rt.dev(states), rt.dev(th)
        rc = mdl.lib.pdp_sysid_step_gn_batched(B, T, rt.ptr(u_d), rt.ptr(x_d), None, rt.ptr(th_d), 0, 0, rt.ptr(loss), rt.ptr(packed), None, 0, rt.current_stream_ptr())
        assert rc == -2 and float(packed.min()) == 7.0 and float(loss.min()) == 7.0
    tag = "SysID GN chain (%d, %d, %d)" % (n, m, p)
    out = sid.step_batch(inputs, states, th, want_gauss_newton=True)
    assert tuple(out["packed_gn"].shape) == (B, p + 1 + p * p)
    check_rows(margins, tag + " complete", (npy(out["loss"]), npy(out["grad"]), npy(out["gn"])), sg.reference_rows(orc, inputs, states, th))
    l0, g0 = sid.step_batch(inputs, states, th)
    margins.check(tag + ": gradient columns vs the plain call", rel_rows(npy(out["grad"]), npy(g0)), TOL)
    out = sid.step_batch(inputs, masked, th, want_gauss_newton=True, skip_missing=True, ini_state=x0)
    got = (npy(out["loss"]), npy(out["grad"]), npy(out["gn"]))
    check_rows(margins, tag + " masked", got, sg.reference_rows(orc, inputs, masked, th, x0, True))
    check_unobserved_sample(tag, got)


# ---- argument errors on the GPU ------------------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_write_nothing():
    from pdp_amd import runtime as rt
    import torch
    mdl = model("cartpole")
    inputs, states, _, theta = sg.stored("cartpole")
    B, T, p = inputs.shape[0], inputs.shape[1], mdl.p
    u, xo, th = rt.dev(inputs), rt.dev(states), rt.dev(theta)
    packed, loss = rt.dev(np.full((B, p + 1 + p * p), 7.0)), rt.dev(np.full((B,), 7.0))
    P, st = rt.ptr, rt.current_stream_ptr()
    fn = mdl.lib.pdp_sysid_step_gn_batched
    assert fn(B, T, P(u), P(xo), None, P(th), 0, 64, P(loss), P(packed), None, 0, st) == -1            # unknown flag bit
    assert fn(B, T, P(u), P(xo), None, P(th), 0, 16, P(loss), P(packed), None, 0, st) == -1            # PDP_GRAD_GAUSS_NEWTON is not a flag of this entry point
    assert fn(0, T, P(u), P(xo), None, P(th), 0, 0, P(loss), P(packed), None, 0, st) == -1
    assert fn(B, -1, P(u), P(xo), None, P(th), 0, 32, P(loss), P(packed), None, 0, st) == -1
    assert fn(B, T, None, P(xo), None, P(th), 0, 0, P(loss), P(packed), None, 0, st) == -1
    assert fn(B, T, P(u), None, None, P(th), 0, 0, P(loss), P(packed), None, 0, st) == -1
    assert fn(B, T, P(u), P(xo), None, None, 0, 0, P(loss), P(packed), None, 0, st) == -1
    assert fn(B, T, P(u), P(xo), None, P(th), 0, 0, None, P(packed), None, 0, st) == -1
    torch.cuda.synchronize()
    assert float(packed.min()) == 7.0 and float(packed.max()) == 7.0 and float(loss.min()) == 7.0 and float(loss.max()) == 7.0
    assert fn(B, T, P(u), P(xo), None, P(th), 0, 0, P(loss), P(packed), None, 0, st) == 0              # (and the same buffers are written by a valid call)
    torch.cuda.synchronize()
    assert float((packed == 7.0).sum()) == 0.0 and torch.equal(loss, packed[:, p])
    with pytest.raises(ValueError, match="ini_state"):
        mdl.sysid_step(inputs, sg.mask_states(states), theta, gauss_newton=True, skip_missing=True)     # row 0 is not observed and no ini_state is given


# ---- Levenberg-Marquardt -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(sg.LM_INPUTS)), ids=[t[0] for t in sg.LM_INPUTS])
def test_lm_loop_follows_the_oracle_schedule(k):
    from pdp_amd.irl import LMLoop
    c = sg.lm_input(k)
    orc = sg.oracle_lm(k, 1e-16)
    loop = LMLoop.for_sysid(model(c["system"]), c["inputs"], c["states"], c["theta0"], ini_state=c["ini_state"], skip_missing=c["skip_missing"])
    r = loop.run(max_evals=50, loss_tol=1e-16)
    print("%s\n  oracle %d evaluations: %s\n  GPU    %d evaluations, %d rejected: %s" % (sg.LM_INPUTS[k][0], orc["evaluations"], " ".join("%.3e" % v for v in orc["loss_trace"]),
                                                                                        r["evaluations"], r["rejected"], " ".join("%.3e" % v for v in r["loss_trace"])))
    assert r["evaluations"] <= 2 * orc["evaluations"] and not r["stalled"]
    assert r["loss_trace"][-1] <= 1e-10
    assert (np.diff(r["loss_trace"]) < 0).all()
    if c["ini_state"] is None and c["system"] in sg.LM_THETA_SYSTEMS:
        assert np.abs(r["parameter_trace"][-1] - c["true_parameter"]).max() <= 1e-6


# ---- the example ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args", [("--system", "cartpole", "--method", "lm"), ("--system", "pendulum", "--method", "lm", "--every", "2", "--observe", "0")],
                         ids=["cartpole", "pendulum_every_2_component_0"])
def test_example_with_method_lm(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "sysid_pdp.py")] + list(args), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    lines = r.stdout.splitlines()
    done = [ln for ln in lines if ln.startswith("done:")]
    assert len(done) == 1, r.stdout[-3000:]
    last = float(done[0].split("loss ")[-1].split(";")[0].split(" -> ")[1])
    assert last <= 1e-10, r.stdout[-3000:]
    assert len([ln for ln in lines if ln.startswith("accepted")]) >= 2, r.stdout[-3000:]
