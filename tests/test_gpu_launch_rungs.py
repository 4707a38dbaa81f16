"""The rungs of the host-side dispatch ladders (csrc/pdp_model.hip, csrc/pdp_lqr.hip) that no other test enters, each against the same rows computed at a rung that
other tests pin to the oracle.  Which instantiation a call takes follows from the batch size, the device's CU count and the number of 16-column parameter tiles; the
rules are restated in `_pair_rung` / `_one_wave_per` below and every case asserts that it is on the rung it is meant for (so the file stays honest on another device).

ControlPlanning.step, Lagrange policy, quadrotor (m = 4) at T = 7 with 4 / 8 / 12 / 16 pivots = 1 .. 4 parameter tiles, per-sample parameters:
  cp_step_poly2_kernel<NT, TPW>   (PDP_CP_POLY_VARIANT=3)   (1, 4), (3, 4), (4, 4) at B = 2 cus + 1; (4, 2) at B = cus + 1; B = cus, the largest batch whose tiles still
                                                            spread over grid.y: (2, 1) with 3 and with 4 tiles.  [(1, 1), (1, 2), (2, 1), (2, 2), (2, 4), (3, 2):
                                                            tests/test_gpu_cp_pair.py.  (3, 1) and (4, 1) cannot be reached: three tiles per pair need B > cus, one
                                                            trajectory per workgroup B <= cus.]
  cp_step_poly_kernel<NT>         (PDP_CP_POLY_VARIANT=1)   NT = 3, 4 at B = 2 cus + 1   [NT = 1, 2: tests/test_gpu_cp_pair.py, tests/test_gpu_models.py]
  cp_step_poly_kernel<NT, GIVEN>  (PDP_CP_PREPASS=1)        NT = 3, 4 at B = cus + 1     [NT = 1, 2: tests/test_gpu_edge_cases.py, tests/test_gpu_configs_oracle.py]
Reference rows: the same trajectories in sub-batches of at most cus rows with PDP_CP_POLY_VARIANT=1 - cp_step_poly_kernel<1>, one tile per wavefront over grid.y, the
instantiation tests/test_gpu_models.py holds against the reference's own ControlPlanning.step runs.

LQR.lqrSolver, lqr_solve_stream_kernel<M, 16> (13 .. 16 lines per ring slot), M = 1 .. 4 at n = 15 [<M, 12>: test_lqr_every_kernel_instantiation] against
lqr_solve_kernel<M, 1> (PDP_LQR_VARIANT=1), which tests/test_gpu_lqr.py holds against the oracle.

pdp_cp_aux_integrate_batched, cp_aux_kernel<1> (p <= 16) against the same columns inside a wider problem, cp_aux_kernel<2> (tests/test_gpu_lqr.py holds it against numpy).

Tolerance: the project's HIP-vs-oracle tolerance, 1e-10 relative to the largest entry.  The switches are read once per process: three child
processes in all."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10
T = 7
PIVOTS = {1: 4, 2: 8, 3: 12, 4: 16}                 # parameter tiles -> pivots of the quadrotor's policy (p = 4 pivots)
LQR_SHAPES = [(15, 1, 14), (15, 2, 14), (15, 3, 13), (15, 4, 12)]          # (n, m, p): 15, 16, 16, 16 lines per slot


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _split(nt, want):                               # split_tiles (csrc/pdp_launch.h): tiles per wavefront / pair, grid.y
    gy = max(1, min(nt, want))
    per = -(-nt // gy)
    return per, -(-nt // per)


def _tpw(B, cus):
    return 1 if B <= cus else (2 if B <= 2 * cus else 4)


def _pair_rung(nt, B, cus):
    return _split(nt, 2 * cus // B)[0], _tpw(B, cus)


def _one_wave_per(nt, B, cus):
    return _split(nt, 4 * cus // B)[0]


def _cp_inputs(nt, cus):
    rng = np.random.default_rng(40 + nt)
    B, p = 2 * cus + 1, 4 * PIVOTS[nt]
    x0 = 0.3 * rng.standard_normal((B, 13))
    x0[:, 6] = 1.0
    return x0, 0.05 * rng.standard_normal((B, p)), p


def _cp(out, tag, nt, B, cus, chunk=None):
    from pdp_amd import runtime as rt, zoo
    mdl = zoo.get("quadrotor", "oc")
    x0, th, p = _cp_inputs(nt, cus)
    pol = rt.make_policy("poly", pivots=np.linspace(0, T, PIVOTS[nt]))
    parts = [mdl.cp_step(pol, p, x0[lo:min(lo + (chunk or B), B)], th[lo:min(lo + (chunk or B), B)], T) for lo in range(0, B, chunk or B)]
    out["%s_%d_%d_loss" % (tag, nt, B)] = np.concatenate([l.cpu().numpy() for l, _ in parts])
    out["%s_%d_%d_grad" % (tag, nt, B)] = np.concatenate([g.cpu().numpy() for _, g in parts])


def _lqr(out, tag):
    from pdp_amd import runtime as rt
    for n, m, p in LQR_SHAPES:
        rng = np.random.default_rng(100 * m + p)
        Tl, B = 6, 3
        spd = lambda k, s: (lambda A: s * (A @ A.T / k + 0.5 * np.eye(k)))(rng.standard_normal((k, k)))
        F = np.eye(n) + 0.1 * rng.standard_normal((B, Tl, n, n))
        G, E = 0.3 * rng.standard_normal((B, Tl, n, m)), 0.1 * rng.standard_normal((B, Tl, n, p))
        Hxx = np.stack([np.stack([spd(n, 1.0) for _ in range(Tl)]) for _ in range(B)])
        Huu = np.stack([np.stack([spd(m, 0.5) for _ in range(Tl)]) for _ in range(B)])
        Hxu, Hxe, Hue = 0.05 * rng.standard_normal((B, Tl, n, m)), 0.2 * rng.standard_normal((B, Tl, n, p)), 0.2 * rng.standard_normal((B, Tl, m, p))
        hxx, hxe, X0 = np.stack([spd(n, 1.0) for _ in range(B)]), 0.2 * rng.standard_normal((B, n, p)), rng.standard_normal((B, n, p))
        X, U, Lam, st = rt.lqr_solve(F, G, Hxx, Huu, hxx, hxe, E=E, Hxu=Hxu, Hxe=Hxe, Hue=Hue, X0=X0)
        assert int(st.sum()) == 0
        for k, v in (("X", X), ("U", U), ("Lam", Lam)):
            out["%s_%d_%s" % (tag, m, k)] = v.cpu().numpy()


def _worker(mode):
    """runs in a child process whose environment selects the kernels"""
    sys.path.insert(0, ROOT)
    cus, out = _cus(), {}
    if mode == "one_wave":                          # PDP_CP_POLY_VARIANT=1, PDP_LQR_VARIANT=1: the reference rows, and the one-wave rungs NT = 3, 4
        for nt in (1, 2, 3, 4):
            _cp(out, "ref", nt, 2 * cus + 1, cus, chunk=cus)
        for nt in (3, 4):
            _cp(out, "one_wave", nt, 2 * cus + 1, cus)
        _lqr(out, "one_wave")
    elif mode == "pair":                            # PDP_CP_POLY_VARIANT=3; the streamed lqrSolver kernel by default
        for nt, B in ((1, 2 * cus + 1), (3, 2 * cus + 1), (4, 2 * cus + 1), (4, cus + 1), (3, cus), (4, cus)):
            _cp(out, "pair", nt, B, cus)
        _lqr(out, "stream")
    else:                                           # PDP_CP_PREPASS=1: rollout pre-pass + the given-trajectory kernel
        for nt in (3, 4):
            _cp(out, "given", nt, cus + 1, cus)
    return out


ENV = {"one_wave": dict(PDP_CP_POLY_VARIANT="1", PDP_LQR_VARIANT="1", PDP_CP_PREPASS="0"), "pair": dict(PDP_CP_POLY_VARIANT="3", PDP_CP_PREPASS="0"),
       "given": dict(PDP_CP_PREPASS="1")}
_results = {}


def _run(mode, tmp):
    if mode not in _results:
        f = os.path.join(str(tmp), mode + ".npz")
        code = ("import sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_launch_rungs as m; np.savez(%r, **m._worker(%r))"
                % (ROOT, os.path.join(ROOT, "tests"), f, mode))
        env = {k: v for k, v in os.environ.items() if k not in ("PDP_CP_POLY_VARIANT", "PDP_LQR_VARIANT", "PDP_CP_PREPASS", "PDP_CP_GIVEN_WGS")}
        r = subprocess.run([sys.executable, "-c", code], env=dict(env, **ENV[mode]), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:]              # (every entry point returned status 0: runtime.check raises otherwise)
        _results[mode] = dict(np.load(f))
    return _results[mode]


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    cus = _cus()
    for nt in (1, 2, 3, 4):                         # the reference rung: every sub-batch has one tile per wavefront
        assert _one_wave_per(nt, cus, cus) == 1
    return _run("one_wave", tmp_path_factory.mktemp("rungs"))


def _agree(got, ref, what):
    assert np.isfinite(got).all(), what
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print("%-40s relative to the largest entry: %.3e" % (what, err))
    assert err <= TOL, (what, err)


def _judge_cp(res, reference, tag, nt, B):
    for k in ("loss", "grad"):
        _agree(res["%s_%d_%d_%s" % (tag, nt, B, k)], reference["ref_%d_%d_%s" % (nt, 2 * _cus() + 1, k)][:B], "%s nt=%d B=%d %s" % (tag, nt, B, k))


def test_pair_kernel_rungs(reference, tmp_path):
    cus = _cus()
    cases = [(1, 2 * cus + 1, (1, 4)), (3, 2 * cus + 1, (3, 4)), (4, 2 * cus + 1, (4, 4)), (4, cus + 1, (4, 2)), (3, cus, (2, 1)), (4, cus, (2, 1))]
    for nt, B, rung in cases:
        assert _pair_rung(nt, B, cus) == rung, (nt, B, cus)
    assert _split(3, 2 * cus // cus) == (2, 2) and _split(4, 2 * cus // (cus + 1))[1] == 1          # B = cus: the last batch with grid.y > 1
    res = _run("pair", tmp_path)
    for nt, B, _ in cases:
        _judge_cp(res, reference, "pair", nt, B)


def test_one_wave_kernel_three_and_four_tiles_per_wavefront(reference):
    cus = _cus()
    for nt in (3, 4):
        assert _one_wave_per(nt, 2 * cus + 1, cus) == nt
        _judge_cp(reference, reference, "one_wave", nt, 2 * cus + 1)


def test_given_trajectory_kernel_three_and_four_tiles(reference, tmp_path):
    cus = _cus()
    res = _run("given", tmp_path)
    for nt in (3, 4):
        _judge_cp(res, reference, "given", nt, cus + 1)


def test_streamed_lqr_kernel_sixteen_lines_per_slot(reference, tmp_path):
    res = _run("pair", tmp_path)
    for n, m, p in LQR_SHAPES:
        for k in ("X", "U", "Lam"):
            _agree(res["stream_%d_%s" % (m, k)], reference["one_wave_%d_%s" % (m, k)], "lqr n=%d m=%d p=%d %s" % (n, m, p, k))


def test_aux_integrator_one_parameter_tile():
    """a column of X, U depends on its own column of X0, Ue only: p = 11 (one tile per trajectory) equals the first 11 columns of p = 37 (two tiles per wavefront)"""
    from pdp_amd import runtime as rt
    rng = np.random.default_rng(12)
    B, Ta, n, m, p, p1 = 3, 7, 13, 4, 37, 11
    F, G, Ux = 0.3 * rng.standard_normal((B, Ta, n, n)), rng.standard_normal((B, Ta, n, m)), 0.2 * rng.standard_normal((B, Ta, m, n))
    Ue, X0 = rng.standard_normal((B, Ta, m, p)), rng.standard_normal((B, n, p))
    X, U = (a.cpu().numpy() for a in rt.cp_aux_integrate(F, G, Ux, Ue, X0))
    X1, U1 = (a.cpu().numpy() for a in rt.cp_aux_integrate(F, G, Ux, np.ascontiguousarray(Ue[..., :p1]), np.ascontiguousarray(X0[..., :p1])))
    _agree(X1, X[..., :p1], "cp_aux p=11 X")
    _agree(U1, U[..., :p1], "cp_aux p=11 U")
