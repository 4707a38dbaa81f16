"""GPU: SysID.step with estimated components of the initial state (pdp_sysid_step_gn_ini_batched; sysid_step_kernel / sysid_step2_kernel MODE 3 and 4) - the augmented
rows grad [W] | loss | G [W][W] against the CPU reference of tests/sysid_ini_common.py (SysIDOracle started at the selection matrix + numpy) over every kernel the
dispatch can pick, the per-row properties, the materialised route beyond the tile, the return codes, and the two Levenberg-Marquardt loops on it against the oracle's
schedule.

Tolerance: TOL = 1e-10 relative to the largest entry of the reference row for every comparison with the reference; "the same row" between
kernels' slots of one launch, and between ini_mask = 0 and pdp_sysid_step_gn_batched, is equality to the bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

import sysid_gn_common as sg
import sysid_ini_common as si
from sysid_gn_common import TOL, rel_rows

pytestmark = pytest.mark.gpu
ROOT = sg.ROOT
_ref = {}


def npy(t):
    return t.detach().cpu().numpy()


def model(system):
    from pdp_amd import zoo
    return zoo.get(system, "sysid")


VARIANTS = ("complete", "masked", "shifted")
SHIFT = 0.01


def case(k):
    """the stored samples at their stored T.  complete: all data, flags 0, x0 = NULL; masked: the data of sysid_gn_common.mask_states, skip_missing, ini_state given;
    shifted: all data, flags 0, ini_state = x_obs_0 + 0.01 - row 0 is observed and d_0 = 0.01 on every component, so every estimated component's grad[p + k] carries its
    row-0 term in every kernel (in `complete` d_0 is zero, in `masked` row 0 is not observed)"""
    system, idx = si.PARITY[k]
    inputs, states, _, theta = sg.stored(system)
    return dict(system=system, idx=idx, inputs=inputs, states=states, masked=sg.mask_states(states), ini=states[:, 0].copy(), theta=theta)


def reference(k, variant):
    """computed once per case, shared by the tests, never written to"""
    if (k, variant) not in _ref:
        c = case(k)
        masked = variant == "masked"
        ini = {"complete": None, "masked": c["ini"], "shifted": c["ini"] + SHIFT}[variant]
        rows = si.reference_rows(sg.oracle(c["system"]), c["inputs"], c["masked"] if masked else c["states"], c["theta"], c["idx"], ini, masked)
        _ref[(k, variant)] = si.packed(rows)
        _ref[(k, variant)].setflags(write=False)
    return _ref[(k, variant)]


def run(k, variant, tile=None):
    """packed rows [B, W + 1 + W W] of one call; tile: the batch is that many rows, row b a copy of the stored sample b % (number of stored samples)"""
    c = case(k)
    nb = c["inputs"].shape[0]
    pick = np.arange(nb if tile is None else tile) % nb
    kw = {"complete": {}, "masked": dict(skip_missing=True, ini_state=c["ini"][pick]), "shifted": dict(ini_state=c["ini"][pick] + SHIFT)}[variant]
    out = model(c["system"]).sysid_step(c["inputs"][pick], (c["masked"] if variant == "masked" else c["states"])[pick], c["theta"], gauss_newton=True, estimate_ini=c["idx"], **kw)
    assert out["ini_index"] == c["idx"]
    return npy(out["packed_gn"]).copy()


def check_rows(margins, tag, k, variant, rows):
    """the first rows (one per stored sample: 3, the rocket 2) against the reference"""
    p = model(si.PARITY[k][0]).p
    W = p + len(si.PARITY[k][1])
    ref = reference(k, variant)
    nb = len(ref)
    assert rows.shape[1] == W + 1 + W * W
    got = rows[:nb]
    for name, sl in (("gradient", slice(0, W)), ("loss", slice(W, W + 1)), ("G", slice(W + 1, None))):
        margins.check("%s: %s" % (tag, name), rel_rows(got[:, sl], ref[:, sl]), TOL)
    margins.check("%s: row" % tag, rel_rows(got, ref), TOL)
    G = rows[:, W + 1:].reshape(len(rows), W, W)
    assert np.array_equal(G, np.swapaxes(G, 1, 2)), tag + ": G is not symmetric to the bit"
    if variant == "masked":
        assert not rows[1::nb].any(), tag + ": the sample with nothing observed is not exact zeros in all W + 1 + W W entries"
    else:
        assert np.isfinite(rows).all() and (np.diagonal(G, axis1=1, axis2=2) >= 0).all()
    if variant == "shifted":                    # the reference's row-0 term is there to be missed: it is d_0[i_k] = 0.01 of grad[p + k]
        assert (np.abs(ref[:, p:W]) > 0).all()


# ---- parity: the pair kernel with one trajectory per workgroup (the default dispatch at B = 3) -------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(si.PARITY)), ids=si.PARITY_IDS)
def test_parity_pair_kernel_one_trajectory_per_workgroup(margins, k):
    for v in VARIANTS:
        check_rows(margins, "SysID INI %s, pair kernel x1, %s (MODE %d)" % (si.PARITY_IDS[k], v, 4 if v == "masked" else 3), k, v, run(k, v))


# ---- parity: the pair kernel with two trajectories per workgroup, B = 2 #CU - 1 (the last workgroup has a slot that is not `mine`) --------------------------------------
@pytest.mark.parametrize("k", range(len(si.PARITY)), ids=si.PARITY_IDS)
def test_parity_pair_kernel_two_trajectories_per_workgroup(margins, k):
    import torch
    B = 2 * torch.cuda.get_device_properties(0).multi_processor_count - 1
    assert B % 2 == 1 and B > 3
    for v in VARIANTS:
        rows = run(k, v, tile=B)
        assert rows.shape[0] == B
        check_rows(margins, "SysID INI %s, pair kernel x2 at B = %d, %s" % (si.PARITY_IDS[k], B, v), k, v, rows)
        nb = len(reference(k, v))
        for b in range(nb, B):
            assert np.array_equal(rows[b], rows[b % nb]), "row %d is not the row of the sample it copies" % b


# ---- parity: the one-wave kernel and the pre-pass + GIVEN kernel, each in a child process (the switches are read once per process) ---------------------------------------
SWITCHES = [("one-wave kernel", dict(PDP_SYSID_VARIANT="1")), ("pre-pass + GIVEN kernel", dict(PDP_SYSID_PREPASS="1"))]


def _child(path):
    out = {}
    for k in range(len(si.PARITY)):
        for v in VARIANTS:
            out["%d_%s" % (k, v)] = run(k, v)
    np.savez(path, **out)


@pytest.mark.parametrize("s", range(len(SWITCHES)), ids=["one_wave", "prepass_given"])
def test_parity_under_the_kernel_selecting_switches(margins, tmp_path, s):
    name, env = SWITCHES[s]
    f = str(tmp_path / "rows.npz")
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_sysid_ini as m; m._child(%r)" % (ROOT, os.path.join(ROOT, "tests"), f)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, "%s: %s" % (name, r.stdout[-3000:])
    res = np.load(f)
    for k in range(len(si.PARITY)):
        for v in VARIANTS:
            check_rows(margins, "SysID INI %s, %s, %s" % (si.PARITY_IDS[k], name, v), k, v, res["%d_%s" % (k, v)])


# ---- per-row properties ------------------------------------------------------------------------------------------------------------------------------------------------
def test_row_zero_is_no_longer_silent(margins):
    """an observed x_obs[0][i_k] adds d_0[i_k] to grad[p + k] and 1 to G[p + k][p + k]; an unobserved one adds nothing.  Cart-pole {2, 3}, ini_state = x_obs_0 + 0.01,
    row 0 observed in component 2 only - against the reference, and against the same data with row 0 not observed at all: the differences are exactly those terms"""
    system, idx = "cartpole", [2, 3]
    mdl, sid = model(system), sg.oracle(system)
    inputs, states, _, theta = sg.stored(system)
    p, W = mdl.p, mdl.p + 2
    ini = states[:, 0] + 0.01
    obs = sg.mask_states(states)
    obs[1, 1::2, 0::2] = states[1, 1::2, 0::2]                                         # (every sample observed here)
    first = obs.copy()
    first[:, 0, 2] = states[:, 0, 2]
    rows = {}
    for tag, xo in (("row 0 unobserved", obs), ("row 0: component 2", first)):
        out = mdl.sysid_step(inputs, xo, theta, gauss_newton=True, skip_missing=True, ini_state=ini, estimate_ini=idx)
        rows[tag] = npy(out["packed_gn"]).copy()
        margins.check("SysID INI cartpole {2, 3}, %s" % tag, rel_rows(rows[tag], si.packed(si.reference_rows(sid, inputs, xo, theta, idx, ini, True))), TOL)
    diff = rows["row 0: component 2"] - rows["row 0 unobserved"]
    l_, g_, G_ = si.unpack(diff, W)
    tol = 1e-12 * max(1.0, np.abs(rows["row 0 unobserved"]).max())                     # the two runs differ in the first term of their sums: roundings of the rest
    assert np.abs(g_[:, p] - 0.01).max() <= tol and np.abs(G_[:, p, p] - 1.0).max() <= tol and np.abs(l_ - 1e-4).max() <= tol
    g_[:, p], G_[:, p, p] = 0.0, 0.0
    assert np.abs(g_).max() <= tol and np.abs(G_).max() <= tol


@pytest.mark.parametrize("system", ["cartpole", "quadrotor"])
def test_ini_mask_zero_is_the_gauss_newton_call(system):
    from pdp_amd import runtime as rt
    import torch
    mdl = model(system)
    inputs, states, _, theta = sg.stored(system)
    B, T, p = inputs.shape[0], inputs.shape[1], mdl.p
    u, th, P, st = rt.dev(inputs), rt.dev(theta), rt.ptr, rt.current_stream_ptr()
    for flags, xo, x0 in ((0, rt.dev(states), None), (32, rt.dev(sg.mask_states(states)), rt.dev(states[:, 0].copy()))):
        out = mdl.sysid_step(u, xo, th, gauss_newton=True, skip_missing=bool(flags), ini_state=x0)
        packed, loss = rt.dev(np.full((B, p + 1 + p * p), 7.0)), rt.dev(np.full((B,), 7.0))
        assert mdl.lib.pdp_sysid_step_gn_ini_batched(B, T, P(u), P(xo), P(x0), 0, P(th), 0, flags, P(loss), P(packed), None, 0, st) == 0
        torch.cuda.synchronize()
        assert torch.equal(packed, out["packed_gn"]) and torch.equal(loss, out["loss"])
        via = mdl.sysid_step(u, xo, th, gauss_newton=True, skip_missing=bool(flags), ini_state=x0, estimate_ini=[])      # nothing selected is estimate_ini=None
        assert "ini_index" not in via and torch.equal(via["packed_gn"], out["packed_gn"])


# ---- beyond the tile: PDP_E_SIZE and the materialised route ----------------------------------------------------------------------------------------------------------------
def test_size_route_quadrotor_with_twelve_estimated_components(margins):
    from pdp_amd import runtime as rt
    system, idx = "quadrotor", list(range(1, 13))                                       # W = 5 + 12 = 17
    mdl, sid = model(system), sg.oracle(system)
    inputs, states, _, theta = sg.stored(system)
    B, T, W = inputs.shape[0], inputs.shape[1], mdl.p + 12
    u, xo, th, P = rt.dev(inputs), rt.dev(states), rt.dev(theta), rt.ptr
    packed, loss = rt.dev(np.full((B, W + 1 + W * W), 7.0)), rt.dev(np.full((B,), 7.0))
    rc = mdl.lib.pdp_sysid_step_gn_ini_batched(B, T, P(u), P(xo), None, sum(1 << i for i in idx), P(th), 0, 0, P(loss), P(packed), None, 0, rt.current_stream_ptr())
    assert rc == -2 and float(packed.min()) == 7.0 and float(loss.min()) == 7.0          # the entry point itself refuses the size, before any launch
    masked, ini = sg.mask_states(states), states[:, 0].copy()
    for tag, xs, kw, ref_kw in (("complete", states, {}, dict(ini_state=None, skip_missing=False)),
                                ("masked", masked, dict(skip_missing=True, ini_state=ini), dict(ini_state=ini, skip_missing=True))):
        out = mdl.sysid_step(inputs, xs, theta, gauss_newton=True, estimate_ini=idx, **kw)
        assert tuple(out["packed_gn"].shape) == (B, W + 1 + W * W) and tuple(out["gn"].shape) == (B, W, W)
        margins.check("SysID INI quadrotor W = 17 (materialised), %s" % tag, rel_rows(npy(out["packed_gn"]), si.packed(si.reference_rows(sid, inputs, xs, theta, idx, **ref_kw))), TOL)
        if kw:
            assert not npy(out["packed_gn"])[1].any()
        l2, g2 = mdl.sysid_step(inputs, xs, theta, estimate_ini=idx, **kw)                # without gauss_newton: (loss, grad [B, W]) of the same route
        assert np.array_equal(npy(l2), npy(out["loss"])) and np.array_equal(npy(g2), npy(out["grad"]))


def test_size_route_chain_5_1_17_through_the_class_surface(margins):
    """p = 17 alone is beyond the tile: {0} gives W = 18, through PDP.SysID.step_batch against SysIDOracle built from the same equations in sympy"""
    import sympy as sp
    from oracle import pdp_oracle as po
    from pdp_amd import PDP
    from pdp_amd.sx import vertcat
    X, U, w, f = sg.chain_5_1_17("sx")
    Xs, Us, ws_, fs = sg.chain_5_1_17("sympy")
    n, m, p = len(Xs), len(Us), len(ws_)
    sid = PDP.SysID("sysid gn chain %d %d %d" % (n, m, p))
    sid.setAuxvarVariable(vertcat(*w))
    sid.setStateVariable(vertcat(*X))
    sid.setControlVariable(vertcat(*U))
    sid.setDyn(vertcat(*f))
    orc = po.SysIDOracle(sp.Matrix(Xs), sp.Matrix(Us), list(ws_), sp.Matrix(fs))
    rng = np.random.default_rng(n + p)
    B, T, W = 3, 9, p + 1
    th_true, th = 1.0 + 0.3 * rng.uniform(-1, 1, p), 1.0 + 0.3 * rng.uniform(-1, 1, p)
    inputs, x0 = rng.uniform(-1, 1, (B, T, m)), 0.5 * rng.standard_normal((B, n))
    states = np.stack([orc.integrateDyn(x0[i], inputs[i], th_true) for i in range(B)])
    masked = sg.mask_states(states)
    out = sid.step_batch(inputs, states, th, want_gauss_newton=True, estimate_ini=[0])
    assert tuple(out["packed_gn"].shape) == (B, W + 1 + W * W)
    margins.check("SysID INI chain (5, 1, 17) {0} complete", rel_rows(npy(out["packed_gn"]), si.packed(si.reference_rows(orc, inputs, states, th, [0]))), TOL)
    out = sid.step_batch(inputs, masked, th, want_gauss_newton=True, skip_missing=True, ini_state=x0 + 0.01, estimate_ini=[0])
    margins.check("SysID INI chain (5, 1, 17) {0} masked", rel_rows(npy(out["packed_gn"]), si.packed(si.reference_rows(orc, inputs, masked, th, [0], x0 + 0.01, True))), TOL)
    assert not npy(out["packed_gn"])[1].any()


# ---- return codes through the raw call ---------------------------------------------------------------------------------------------------------------------------------
def test_return_codes_write_nothing():
    from pdp_amd import runtime as rt, zoo
    import torch
    mdl = model("cartpole")
    inputs, states, _, theta = sg.stored("cartpole")
    B, T, W = inputs.shape[0], inputs.shape[1], mdl.p + 2
    u, xo, th = rt.dev(inputs), rt.dev(states), rt.dev(theta)
    packed, loss = rt.dev(np.full((B, W + 1 + W * W), 7.0)), rt.dev(np.full((B,), 7.0))
    P, st = rt.ptr, rt.current_stream_ptr()
    fn = mdl.lib.pdp_sysid_step_gn_ini_batched
    assert fn(B, T, P(u), P(xo), None, 1 << 4, P(th), 0, 0, P(loss), P(packed), None, 0, st) == -1            # a mask bit >= n (cart-pole: n = 4): PDP_E_ARG
    assert fn(B, T, P(u), P(xo), None, 12 | (1 << 9), P(th), 0, 32, P(loss), P(packed), None, 0, st) == -1
    assert fn(B, T, P(u), P(xo), None, 12, P(th), 0, 64, P(loss), P(packed), None, 0, st) == -1               # an unknown flag bit: PDP_E_ARG
    assert fn(B, T, P(u), P(xo), None, 12, P(th), 0, 16, P(loss), P(packed), None, 0, st) == -1
    assert fn(0, T, P(u), P(xo), None, 12, P(th), 0, 0, P(loss), P(packed), None, 0, st) == -1
    assert fn(B, T, P(u), P(xo), None, 12, P(th), 0, 0, None, P(packed), None, 0, st) == -1
    oc = zoo.get("cartpole", "irl")
    for flags in (0, 32):
        assert oc.lib.pdp_sysid_step_gn_ini_batched(B, T, P(u), P(xo), None, 12, P(th), 0, flags, P(loss), P(packed), None, 0, st) == -4      # an OC library: PDP_E_MODE
    torch.cuda.synchronize()
    assert float(packed.min()) == 7.0 and float(packed.max()) == 7.0 and float(loss.min()) == 7.0 and float(loss.max()) == 7.0
    assert fn(B, T, P(u), P(xo), None, 12, P(th), 0, 0, P(loss), P(packed), None, 0, st) == 0                  # (and the same buffers are written by a valid call)
    torch.cuda.synchronize()
    assert float((packed == 7.0).sum()) == 0.0 and torch.equal(loss, packed[:, W])


# ---- Levenberg-Marquardt -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("system, scale", sorted(si.SHARED_COUNTS), ids=["%s_%.1f" % k for k in sorted(si.SHARED_COUNTS)])
def test_lm_loop_shared_theta_follows_the_oracle_schedule(system, scale):
    from pdp_amd.irl import LMLoop
    c = si.lm_data(system)
    orc = si.oracle_lm_shared(system, scale, 1e-16)
    loop = LMLoop.for_sysid(model(system), c["inputs"], c["states"], c["theta_ref"] * scale, ini_state=c["ini_state"], skip_missing=True, estimate_ini=c["idx"])
    r = loop.run(max_evals=50, loss_tol=1e-16)
    print("%s x %.1f\n  oracle %d evaluations: %s\n  GPU    %d evaluations, %d rejected: %s" % (system, scale, orc["evaluations"], " ".join("%.3e" % v for v in orc["loss_trace"]),
                                                                                              r["evaluations"], r["rejected"], " ".join("%.3e" % v for v in r["loss_trace"])))
    assert r["evaluations"] <= 2 * orc["evaluations"]
    assert r["loss_trace"][-1] <= 1e-10
    assert (np.diff(r["loss_trace"]) < 0).all()
    theta, ini = loop.split(r["parameter_trace"][-1])
    assert theta.shape == (model(system).p,) and ini.shape == c["x0_true"].shape
    if system == "cartpole":
        assert np.abs(theta - sg.stored(system)[2]).max() <= 1e-6
        assert np.abs(ini - c["x0_true"]).max() <= 1e-6


def test_batched_lm_loop_per_trajectory_cartpole():
    """K = 9: the three stored trajectories from theta_ref x {1.0, 0.9, 1.1}, each with its own theta and its own unknown velocities"""
    from pdp_amd.irl import BatchedLMLoop
    system = "cartpole"
    c, mdl = si.lm_data(system), model(system)
    pick = np.tile(np.arange(3), 3)
    theta0 = np.stack([c["theta_ref"] * s for s in si.SCALES for _ in range(3)])
    loop = BatchedLMLoop.for_sysid(mdl, c["inputs"][pick], c["states"][pick], theta0, ini_state=c["ini_state"][pick], skip_missing=True, estimate_ini=c["idx"],
                                   max_evals=50, loss_tol=1e-16)
    r = loop.run()
    theta, ini = loop.split(r["theta"])
    assert theta.shape == (9, mdl.p) and ini.shape == (9, mdl.n)
    for k in range(9):
        orc = si.oracle_lm_trajectory(system, int(pick[k]), si.SCALES[k // 3], 1e-16)
        print("trajectory %d x %.1f\n  oracle %d evaluations: %s\n  GPU    %d evaluations, %d rejected, %s: %s"
              % (pick[k], si.SCALES[k // 3], orc["evaluations"], " ".join("%.3e" % v for v in orc["loss_trace"]), r["evaluations"][k], r["rejected"][k], r["state"][k],
                 " ".join("%.3e" % v for v in r["loss_trace"][k])))
    for k in range(9):
        orc = si.oracle_lm_trajectory(system, int(pick[k]), si.SCALES[k // 3], 1e-16)
        assert r["state"][k] == "CONVERGED" and r["evaluations"][k] <= 2 * orc["evaluations"], k
    assert np.abs(theta - sg.stored(system)[2]).max() <= 1e-6
    assert np.abs(ini - c["x0_true"][pick]).max() <= 1e-6


def test_for_sysid_argument_rules():
    from pdp_amd.irl import BatchedLMLoop, LMLoop
    c, mdl = si.lm_data("quadrotor"), model("quadrotor")
    with pytest.raises(ValueError, match="samples_per_problem"):
        BatchedLMLoop.for_sysid(mdl, c["inputs"][:2], c["states"][:2], c["theta_ref"], samples_per_problem=2, ini_state=c["ini_state"][:2], skip_missing=True,
                                estimate_ini=c["idx"])
    with pytest.raises(ValueError, match="> 16"):
        BatchedLMLoop.for_sysid(mdl, c["inputs"], c["states"], c["theta_ref"], ini_state=c["ini_state"], skip_missing=True, estimate_ini=list(range(1, 13)))
    with pytest.raises(ValueError, match="BatchedLMLoop"):
        LMLoop.for_sysid(mdl, c["inputs"], c["states"], c["theta_ref"], n_total=6, ini_state=c["ini_state"], skip_missing=True, estimate_ini=c["idx"])
    big = np.arange(42) % 3                                                             # N = 5 + 42 * 6 = 257
    with pytest.raises(ValueError, match="BatchedLMLoop"):
        LMLoop.for_sysid(mdl, c["inputs"][big], c["states"][big], c["theta_ref"], ini_state=c["ini_state"][big], skip_missing=True, estimate_ini=c["idx"])
    bad = c["ini_state"].copy()
    bad[0, 3] = np.nan
    with pytest.raises(ValueError, match="ini_state"):
        LMLoop.for_sysid(mdl, c["inputs"], c["states"], c["theta_ref"], ini_state=bad, skip_missing=True, estimate_ini=c["idx"])


# ---- the example ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [(), ("--per-trajectory",)], ids=["shared", "per_trajectory"])
def test_example_with_estimate_ini(extra):
    args = ["--system", "cartpole", "--method", "lm", "--observe", "0,1", "--estimate-ini", "2,3"] + list(extra)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "sysid_pdp.py")] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    lines = r.stdout.splitlines()
    if extra:
        done = [ln for ln in lines if ln.startswith("trajectory")]
        assert len(done) == 3 and all("CONVERGED" in ln and "ini_state" in ln for ln in done), r.stdout[-3000:]
    else:
        done = [ln for ln in lines if ln.startswith("done:")]
        assert len(done) == 1 and "ini_state" in done[0], r.stdout[-3000:]
        assert float(done[0].split("loss ")[-1].split(";")[0].split(" -> ")[1]) <= 1e-10, r.stdout[-3000:]
