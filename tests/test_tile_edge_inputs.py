"""CPU: the conditions under which tests/test_gpu_tile_edge.py means something, checked on the oracle and the code generator alone (no compiling, no GPU).

1. Sizes: the three models of tests/tile_edge_common.py have the (n, m, p) they are there for - E16 a full state tile and the solver's non-homogeneous form, E15 a full
   augmented tile, all three a full [control | parameter] tile - and no parameter is idle.
2. Kernel selection: the restated fused3_ok(T) / ms2_ok hold for every model at every horizon used, so the runner / evaluator kernels are the ones under test, and the
   two long horizons span two backward chunks, the second one of unequal lengths.
3. Rounding error of the reference order: oracle.pdp_oc_unit's X, U against the same formulas in 40-digit arithmetic (oracle.lqr_solver_mp) on the same auxiliary system,
   <= 1e-12 of the largest entry.  Measured: 1.3e-16 .. 4.9e-16 on every sample of every input (T = 1, 7, ROWS + 6, ROWS + 7; shared and per-sample theta).  The 40-digit
   solve costs 5 s per sample at n = 16, T = 28, so the test measures both theta modes at the short horizons and one sample at each long one.
4. Solver runs: every solver input converges in oracle.ipopt_ms.solve within 25 iterations without a restoration; over the inputs of each model at least one iteration
   corrects the inertia (dw > 0) and at least one shortens the step (alpha < 1)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import tile_edge_common as c  # noqa: E402

NAMES = sorted(c.MODELS)


@pytest.mark.parametrize("name", NAMES)
def test_sizes_and_kernel_selection(name):
    info = c.generated_info(name)
    n, m, p = c.MODELS[name]
    assert (info["n"], info["m"], info["p"]) == (n, m, p)
    assert m + p == 16                                         # the shared [control | parameter] tile is full; m + p = 17 is the first refused size
    ms2 = c.ms2_layout(info)
    if name == "E16":
        assert n == 16 and not ms2["AUG"] and ms2["NA"] == 16      # the `if constexpr (!AUG)` branches
    elif name == "E15":
        assert n + 1 == 16 and ms2["AUG"] and ms2["NA"] == 16      # a full augmented tile
    else:
        assert n == 5 and m == 1 and ms2["AUG"]                    # the first size past the small-system kernels
    assert c.ms2_ok(info)
    f3 = c.fused3_layout(info)
    hs = c.unit_horizons(info)
    assert hs == (1, 7, f3["ROWS"] + 6, f3["ROWS"] + 7)
    for T in hs:
        assert c.fused3_ok(info, T) and c.fused_accepts(info, T), (name, T)
    assert [len(c.backward_chunks(info, T)) for T in hs] == [1, 1, 2, 2]
    a, b = c.backward_chunks(info, hs[3])
    assert a != b and a + b == hs[3]
    for reg in c.REGIMES:                                      # (the solver's chunks: T = 25 / 30 is one chunk for every model - the hand-over protocol of longer horizons is
        assert c.REGIMES[reg]["T"] <= ms2["ROWS"]               #  tests/test_gpu_predict.py's subject at T = 100)
    # one more parameter is refused by the fused unit, one more state by both
    assert not c.fused_accepts(dict(info, p=p + 1), 7) and not c.fused_accepts(dict(info, n=17), 7) and not c.ms2_ok(dict(info, n=17))


@pytest.mark.parametrize("name", NAMES)
def test_every_parameter_moves_the_trajectory(name):
    """no column of dx/dtheta is identically zero at T = 7 (40-digit solution of sample 0, shared theta)"""
    Xe, Ue = c.unit_exact(name, 7, False, 0)
    assert (np.abs(Xe).max(axis=(0, 1)) > 0).all() and (np.abs(Ue).max(axis=(0, 1)) > 0).all()


@pytest.mark.parametrize("name", NAMES)
def test_reference_order_is_accurate_on_the_unit_inputs(name):
    hs = c.unit_horizons(c.generated_info(name))
    cases = [(T, ps, b) for T in hs[:2] for ps, b in ((False, 0), (True, c.B_UNIT - 1))] + [(hs[2], False, 0), (hs[3], True, c.B_UNIT - 1)]
    for T, per_sample, b in cases:
        o = c.unit_oracle(name, T, per_sample, b)
        Xe, Ue = c.unit_exact(name, T, per_sample, b)
        ex, eu = c.rel(np.stack(o["lqr"]["state_traj_opt"]), Xe), c.rel(np.stack(o["lqr"]["control_traj_opt"]), Ue)
        print("%s T=%d %s theta sample %d: reference order vs 40 digits X %.2e U %.2e" % (name, T, "per-sample" if per_sample else "shared", b, ex, eu))
        assert ex <= c.REF_CAP and eu <= c.REF_CAP, (name, T, per_sample, b, ex, eu)


@pytest.mark.parametrize("name", NAMES)
def test_solver_inputs_converge_and_exercise_the_safeguards(name):
    seen_dw = seen_alpha = False
    for reg in sorted(c.REGIMES):
        rows = c.SOLVER_ROWS[name, reg]
        assert len(rows) == 2 and len(set(rows)) == 2
        for row in rows:
            ref, log = c.solver_oracle(name, reg, row)
            print("%s (%s) draw %d: %d iterations, %d restorations, dw > 0 on %d, alpha < 1 on %d" % (name, reg, row, ref["iterations"], ref["restorations"],
                                                                                                     sum(l["dw"] > 0 for l in log), sum(l["alpha"] < 1 for l in log)))
            assert ref["iterations"] == len(log) <= c.MAX_ITER_ORACLE and ref["restorations"] == 0, (name, reg, row)
            seen_dw = seen_dw or any(l["dw"] > 0.0 for l in log)
            seen_alpha = seen_alpha or any(l["alpha"] < 1.0 for l in log)
    assert seen_dw and seen_alpha
