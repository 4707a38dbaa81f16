"""CPU: the inputs of tests/test_gpu_riccati_conditioning.py keep the comparison meaningful - on every one of them the reference's own fp64 order of operations
(oracle.pdp_oracle.lqr_solver) stays within 1e-8 of the same formulas in 40-digit arithmetic (lqr_solver_mp), per sample and per quantity.  The GPU tests bound the
kernels by max(1e-10, that error); an input on which the reference itself has lost its digits would make that bound say nothing.  If an input breaks the cap, the
input changes, not the cap."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import riccati_conditioning_common as rc      # noqa: E402


@pytest.mark.parametrize("n,m,p,near", rc.LQR_INPUTS, ids=["n%d_m%d_p%d%s" % (n, m, p, "_near" if near else "") for n, m, p, near in rc.LQR_INPUTS])
def test_lqr_inputs_reference_order_below_cap(n, m, p, near):
    batch, exact, ref_err = rc.lqr_case(n, m, p, near)
    assert batch["G"].shape == (len(rc.SCALES), rc.T, n, m)
    for b, s in enumerate(rc.SCALES):
        print("n=%d m=%d p=%d%s s=%g: reference order vs 40 digits  X %.2e  U %.2e  Lam %.2e" % ((n, m, p, " near" if near else "", s) + ref_err[b]))
        rank = np.linalg.matrix_rank(batch["G"][b, 0])
        assert rank == (min(n, m) if near else 1)
        assert np.linalg.eigvalsh(batch["Huu"][b, 0]).min() > 0
        assert max(ref_err[b]) < rc.REF_CAP, (n, m, p, near, s, ref_err[b])


@pytest.mark.parametrize("n", rc.OC_SIZES)
def test_oc_auxiliary_systems_reference_order_below_cap(n):
    """the auxiliary systems of the fused-unit tests, built by the sympy oracle from the same model and inputs"""
    p = n + 2
    for b, s in enumerate(rc.SCALES):
        aux = rc.oc_aux_oracle(n, b)
        assert np.allclose(aux["Huu"][0], 2 * s * np.eye(rc.OC_M), rtol=1e-14, atol=0) and np.linalg.matrix_rank(aux["dynG"][0]) == 1
        pr = rc.aux_problem(aux, n, p)
        ex, ref = rc.solve_mp(pr), rc.solve_ref(pr)
        err = tuple(rc.rel(r, e) for r, e in zip(ref, ex))
        inp = rc.oc_inputs(n)
        g_ex, g_ref = rc.contract(inp["gx"][b], inp["gu"][b], ex[0], ex[1]), rc.contract(inp["gx"][b], inp["gu"][b], ref[0], ref[1])
        print("OC n=%d w_u=%g: reference order vs 40 digits  dxdp %.2e  dudp %.2e  Lam %.2e  contracted %.2e" % ((n, s) + err + (rc.rel(g_ref, g_ex),)))
        assert max(err) < rc.REF_CAP and rc.rel(g_ref, g_ex) < rc.REF_CAP, (n, s, err)


@pytest.mark.parametrize("n", rc.OC_SIZES)
def test_oc_lq_optimum_reference_order_below_cap(n):
    exact, ref_err = rc.oc_lq_case(n)
    for b, s in enumerate(rc.SCALES):
        print("OC optimum n=%d w_u=%g: reference order vs 40 digits  x %.2e  u %.2e  lam %.2e" % ((n, s) + ref_err[b]))
        assert max(ref_err[b]) < rc.REF_CAP, (n, s, ref_err[b])
