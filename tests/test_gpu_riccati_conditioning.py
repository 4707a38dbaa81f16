"""GPU: the m x m solve of the backward Riccati step on ill-conditioned Quu = Huu + G'PG - cheap controls (Huu ~ s) acting on the state through a rank-1 G, so that
Quu has one eigenvalue of order 1 and m - 1 of order s - through every kernel that carries the solve: the LQR kernels (stream, one-wave at one and two parameter tiles,
small-system, size-generic), the fused OC unit with its sensitivities written out and in cotangent mode, and the Newton step of the OC solver.

Inputs: tests/riccati_conditioning_common.py.  One batch of B = 5 holds the sweep s = 1, 1e-2, 1e-3, 1e-4, 1e-5: samples on either side of a conditioning guard share
a workgroup, the last workgroup of the four-per-workgroup kernels is ragged.  T = 8.

Reference: the reference's formulas in 40-digit arithmetic (oracle.pdp_oracle.lqr_solver_mp).  Error: max |diff| / max |40-digit value|, per sample and quantity.
Bound: max(1e-10, the error of the reference's own fp64 order of operations on the same input) - 1e-10 is BASELINE.md section 3's GPU-vs-restatement tolerance, and no
fp64 evaluation can be asked to beat the reference's order by construction; tests/test_riccati_conditioning_inputs.py keeps that second term below 1e-8.  No factor
is granted on top.  Every comparison goes through the `margins` fixture (profiles/*_parity_margins.txt holds a run).

The guards of the cofactor fast paths used to be 1e-10 on |det| against the size of its terms, which sees the cancellation of the last sum only and not the one inside
the minors.  The CPU emulation of the kernels' algebra (probes/riccati_guard_sweep.py, profiles/riccati_guard_sweep.txt) puts that fast path at 1e-9 .. order 1 on the
m = 4 and m = 3 inputs of this file from s = 1e-2 / 1e-3 down, with status 0; the guards are now set from that sweep."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import riccati_conditioning_common as rc      # noqa: E402


def npy(t):
    return None if t is None else t.detach().cpu().numpy()


def _solve(batch, want_costate=True):
    from pdp_amd import runtime as rt
    X, U, Lam, st = rt.lqr_solve(batch["F"], batch["G"], batch["Hxx"], batch["Huu"], batch["hxx"], batch["hxe"], E=batch["E"], Hxu=batch["Hxu"], Hxe=batch["Hxe"],
                                 Hue=batch["Hue"], X0=batch["X0"], want_costate=want_costate)
    return npy(X), npy(U), npy(Lam), npy(st)


def _lqr_route(margins, tag, n, m, p, near=False):
    batch, exact, ref_err = rc.lqr_case(n, m, p, near)
    X, U, Lam, st = _solve(batch)
    assert not st.any(), (tag, st)
    rc.check_lqr(margins, "%s n=%d m=%d p=%d%s" % (tag, n, m, p, " near-rank-1 G" if near else ""), ref_err, exact, (X, U, Lam))
    X2, U2, L2, st2 = _solve(batch, want_costate=False)
    assert L2 is None and not st2.any(), (tag, st2)
    rc.check_lqr(margins, "%s n=%d m=%d p=%d%s, no costate output" % (tag, n, m, p, " near-rank-1 G" if near else ""), ref_err, exact, (X2, U2, None))


@pytest.mark.parametrize("n,m,p", rc.STREAM_SHAPES)
def test_lqr_stream_kernel(margins, n, m, p):
    """dense matrices, one parameter tile: the runner / streamer kernel (the default)"""
    _lqr_route(margins, "LQR stream kernel", n, m, p)


def test_lqr_stream_kernel_near_rank_one(margins):
    _lqr_route(margins, "LQR stream kernel", *rc.NEAR_SHAPE, near=True)


@pytest.mark.parametrize("n,m,p", rc.ONE_WAVE_TWO_TILE_SHAPES)
def test_lqr_one_wave_kernel_two_parameter_tiles(margins, n, m, p):
    """p > 16 - m: the gains multiply a second parameter tile (riccati_backward_extra)"""
    assert p > 16 - m
    _lqr_route(margins, "LQR one-wave kernel, two tiles", n, m, p)


@pytest.mark.parametrize("n,m,p", rc.SMALL_SHAPES)
def test_lqr_small_system_kernel(margins, n, m, p):
    """n <= 4, m + p <= 16: four trajectories per wavefront, B = 5 leaves the second wavefront with one.  M = 4 has always taken the pivoted inverse here (its
    regression test); M = 3, 2 go through inverse_small_fast"""
    assert n <= 4 and m + p <= 16
    _lqr_route(margins, "LQR small-system kernel", n, m, p)


@pytest.mark.parametrize("n,m,p", rc.GENERIC_SHAPES)
def test_lqr_size_generic_kernel(margins, n, m, p):
    assert n > 16 or m > 4
    _lqr_route(margins, "LQR size-generic kernel", n, m, p)


LQR_WORKER = r'''
import sys
import numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(here)r)
import riccati_conditioning_common as rc
from pdp_amd import runtime as rt
b = rc.lqr_batch(*%(shape)r)
out = {}
for tag, wc in (("c", True), ("n", False)):
    X, U, Lam, st = rt.lqr_solve(b["F"], b["G"], b["Hxx"], b["Huu"], b["hxx"], b["hxe"], E=b["E"], Hxu=b["Hxu"], Hxe=b["Hxe"], Hue=b["Hue"], X0=b["X0"], want_costate=wc)
    out.update({tag + "X": X.cpu().numpy(), tag + "U": U.cpu().numpy(), tag + "st": st.cpu().numpy()})
    if wc:
        out["cLam"] = Lam.cpu().numpy()
np.savez(sys.argv[1], **out)
'''


def test_lqr_one_wave_kernel_one_parameter_tile(margins, tmp_path):
    """PDP_LQR_VARIANT=1 (read once per process: a child) keeps the one-wave kernel where the stream kernel is the default"""
    n, m, p = rc.ONE_WAVE_ONE_TILE_SHAPE
    path = str(tmp_path / "one_wave.npz")
    r = subprocess.run([sys.executable, "-c", LQR_WORKER % dict(root=ROOT, here=HERE, shape=(n, m, p)), path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=300, env=dict(os.environ, PDP_LQR_VARIANT="1"))
    assert r.returncode == 0, r.stdout[-3000:]
    z = np.load(path)
    _, exact, ref_err = rc.lqr_case(n, m, p)
    assert not z["cst"].any() and not z["nst"].any()
    rc.check_lqr(margins, "LQR one-wave kernel, one tile n=%d m=%d p=%d" % (n, m, p), ref_err, exact, (z["cX"], z["cU"], z["cLam"]))
    rc.check_lqr(margins, "LQR one-wave kernel, one tile n=%d m=%d p=%d, no costate output" % (n, m, p), ref_err, exact, (z["nX"], z["nU"], None))


# ---- fused OC unit: sensitivities written out (want_sens) and cotangent mode ------------------------------------------------------------------------------
def oc_unit(n):
    """one model through: dict of numpy arrays (x, lam, dxdp, dudp, status, the cotangent unit's grad / status, the auxiliary matrices of the class surface)"""
    oc, inp = rc.oc_model_gpu(n), rc.oc_inputs(n)
    B = len(rc.SCALES)
    zx, zu = np.zeros((B, rc.T + 1, n)), np.zeros((B, rc.T, rc.OC_M))
    s = oc.pdp_grad_batch(inp["u"], inp["theta"], zx, zu, ini_state=inp["x0"], want_sens=True)
    v = oc.pdp_vjp_batch(inp["u"], inp["theta"], inp["gx"], inp["gu"], ini_state=inp["x0"])
    aux = oc.getAuxSys_batch(s["x"], inp["u"], s["lam"], inp["theta"])
    out = {k: npy(s[k]) for k in ("x", "lam", "dxdp", "dudp", "status")}
    out.update(vjp_grad=npy(v["grad"]), vjp_status=npy(v["status"]), vjp_x=npy(v["x"]))
    out.update({"aux_" + k: npy(a) for k, a in aux.items()})
    return out


OC_WORKER = r'''
import sys
import numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(here)r)
import test_gpu_riccati_conditioning as t
np.savez(sys.argv[1], **t.oc_unit(%(n)d))
'''


def _judge_oc_unit(margins, tag, n, r):
    p = n + 2
    inp = rc.oc_inputs(n)
    assert not r["status"].any() and not r["vjp_status"].any(), (tag, r["status"], r["vjp_status"])
    assert np.array_equal(r["x"], r["vjp_x"])
    for b, s in enumerate(rc.SCALES):
        aux = {k[4:]: v[b] for k, v in r.items() if k.startswith("aux_")}
        assert np.linalg.matrix_rank(aux["dynG"][0]) == 1 and np.allclose(aux["Huu"][0], 2 * s * np.eye(rc.OC_M), rtol=1e-12, atol=0)
        pr = rc.aux_problem(aux, n, p)
        ex, ref = rc.solve_mp(pr), rc.solve_ref(pr)
        ref_err = [rc.rel(a, e) for a, e in zip(ref, ex)]
        g_ex, g_ref = rc.contract(inp["gx"][b], inp["gu"][b], ex[0], ex[1]), rc.contract(inp["gx"][b], inp["gu"][b], ref[0], ref[1])
        ref_err.append(rc.rel(g_ref, g_ex))
        assert max(ref_err) < rc.REF_CAP, (tag, s, ref_err)
        bd = rc.bounds(ref_err)
        margins.check("ill-conditioned Quu, %s, w_u=%g: dxdp vs the 40-digit solution of the class surface's auxiliary system" % (tag, s), rc.rel(r["dxdp"][b], ex[0]), bd[0])
        margins.check("ill-conditioned Quu, %s, w_u=%g: dudp vs the 40-digit solution" % (tag, s), rc.rel(r["dudp"][b], ex[1]), bd[1])
        margins.check("ill-conditioned Quu, %s, w_u=%g: cotangent unit vs the 40-digit solution contracted with the same cotangents" % (tag, s),
                      rc.rel(r["vjp_grad"][b], g_ex), bd[3])


def test_fused_unit_runner_evaluator_kernel_at_1_and_4_trajectories_per_workgroup(margins, tmp_path):
    """n = 6, m = 4: the runner / evaluator kernel; PDP_FUSED_TPW is read once per process, one child each; B = 5 leaves the second workgroup ragged at 4"""
    n = 6
    rc.oc_model_gpu(n).model()                  # built once here; the children find it by its content hash
    res = {}
    for tpw in (1, 4):                          # (stops at the first failing child: the assert ends the test)
        path = str(tmp_path / ("tpw%d.npz" % tpw))
        env = dict(os.environ, PDP_FUSED_TPW=str(tpw))
        env.pop("PDP_FUSED_VARIANT", None)
        r = subprocess.run([sys.executable, "-c", OC_WORKER % dict(root=ROOT, here=HERE, n=n), path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600,
                           env=env)
        assert r.returncode == 0, "PDP_FUSED_TPW=%d: %s" % (tpw, r.stdout[-3000:])
        res[tpw] = dict(np.load(path))
        _judge_oc_unit(margins, "fused unit n=6 m=4 TPW=%d" % tpw, n, res[tpw])
    for k in ("dxdp", "dudp", "vjp_grad", "aux_Huu", "aux_dynG"):          # one wave pair per trajectory whatever the workgroup
        assert np.array_equal(res[1][k], res[4][k]), k


def test_fused_unit_one_wave_kernel(margins):
    """n = 4, m = 4: the one-wave kernel of the fused unit (small-system algebra)"""
    _judge_oc_unit(margins, "fused unit n=4 m=4 one-wave", 4, oc_unit(4))


# ---- OC solver: the Newton step's Riccati sweep ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["auto", "single"])
@pytest.mark.parametrize("n", rc.OC_SIZES)
def test_oc_solver_reaches_the_lq_optimum(margins, n, method):
    """The model is linear-quadratic: its optimum is one solve of the LQR formulas from x0 (rc.oc_lq_problem), taken in 40 digits.  ocSolver_batch from the zero guess at
    tol 1e-11, per-sample theta sweeping w_u; "auto" is the multiple-shooting kernel, "single" the single-shooting one (both Newton steps are Riccati sweeps).  The
    iteration count is recorded in the margins file, not asserted (there is no reference count for it)."""
    oc, inp = rc.oc_model_gpu(n), rc.oc_inputs(n)
    exact, ref_err = rc.oc_lq_case(n)
    sol = oc.ocSolver_batch(inp["x0"], rc.T, inp["theta"], tol=1e-11, method=method)
    conv, x, u = npy(sol["converged"]), npy(sol["state"]), npy(sol["control"])
    tag = "ocSolver_batch(method=%s) n=%d m=4" % (method, n)
    margins.check("ill-conditioned Quu, %s: %d iterations of the slowest sample (recorded, not a parity figure)" % (tag, int(sol["iterations"])), 0.0, 0.0)
    assert conv.all(), conv
    for b, s in enumerate(rc.SCALES):
        bd = rc.bounds(ref_err[b])
        margins.check("ill-conditioned Quu, %s, w_u=%g: state vs the 40-digit LQ optimum" % (tag, s), rc.rel(x[b][:, :, None], exact[b][0]), bd[0])
        margins.check("ill-conditioned Quu, %s, w_u=%g: control vs the 40-digit LQ optimum" % (tag, s), rc.rel(u[b][:, :, None], exact[b][1]), bd[1])
