"""GPU: the hand-scheduled backward step of the fused OC unit's runner (oc_pdp_fused3_kernel; riccati_backward<.., SCHED = true>, pdp_riccati.h) keeps every
bit of what the unscheduled kernel computed.

Reference: tests/golden/fused3_sched_parent.npz, recorded on the GPU by probes/record_fused3_sched_golden.py from the build of the parent commit (hash and seed inside the
file) - not from the code under test.  Comparison: np.array_equal on loss, grad, x, lam and status (and dxdp, dudp where they are written); there is no tolerance, the
change is a re-ordering of the same instructions.

Cases (tests/fused3_sched_common.py): the quadrotor at B = 3 and T = 1, 3 (single-step loops only), 4 (one group of U = 4), 5 (a group and a single step), 18 (two backward
chunks), 26 (two forward chunks, gain look-ahead clamped at T - 1); PDP_OC_GIVEN_TRAJ at T = 5; the sensitivity outputs at T = 5 (the sign of U where it is stored); and
the cheap-control model of tests/riccati_conditioning_common.py, whose ill-conditioned Quu sends steps through the pivoted fallback of the 4 x 4 solve (the reciprocal
issued ahead of the guard's branch is dropped there) - PDP_STATUS_PIVOT as on the parent."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import fused3_sched_common as fc      # noqa: E402


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(HERE, "golden", fc.GOLDEN)) as z:
        g = {k: z[k] for k in z.files}
    assert int(g["seed"]) == fc.SEED
    return g


def _check(golden, name, got, fields=fc.FIELDS):
    for k in fields:
        want = golden["%s/%s" % (name, k)]
        assert got[k].shape == want.shape and got[k].dtype == want.dtype, (name, k, got[k].shape, got[k].dtype)
        assert np.array_equal(got[k], want), "%s: %s differs from the parent commit's bits (max |diff| %g)" % (
            name, k, float(np.abs(got[k].astype(np.float64) - want.astype(np.float64)).max()))


@pytest.mark.parametrize("T", fc.HORIZONS)
def test_quadrotor_horizon_keeps_the_parents_bits(golden, T):
    name = "T%d" % T
    got = fc.run_case(name)
    assert not got["status"].any()
    _check(golden, name, got)


def test_given_trajectory_keeps_the_parents_bits(golden):
    """PDP_OC_GIVEN_TRAJ: no rollout on the runner, no costate chain on the evaluator; x and lam handed in are the parent's"""
    got = fc.run_case("given_T5", given=(golden["T5/x"], golden["T5/lam"]))
    _check(golden, "given_T5", got)


def test_sensitivity_outputs_keep_the_parents_bits(golden):
    """dxdp, dudp written out (the RIC instantiation): U_t is stored with the sign the parent gave it"""
    got = fc.run_case("sens_T5")
    _check(golden, "sens_T5", got, fc.FIELDS + ("dxdp", "dudp"))
    assert np.abs(got["dudp"]).max() > 0.0


def test_pivoted_fallback_keeps_the_parents_bits(golden):
    """ill-conditioned Quu: the guard of the cofactor inverse sends steps to the pivoted elimination; bits and status (PDP_STATUS_PIVOT included) as on the parent"""
    got = fc.run_case("pivot")
    _check(golden, "pivot", got)
