"""CPU (no GPU needed): pdp_lm_update_batched - the Levenberg-Marquardt update of many independent problems as one launch - at the ABI (the extension header, the
symbol, its argument errors before any launch), and its numpy restatement (tests/lm_batched_common.py), which is the yardstick of the kernel test: against K independent
irl.LMLoop runs on the oracle's rows, and on a hand-written sequence for the rules at the edges."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lm_batched_common as lb
import sysid_gn_common as sg

ROOT = sg.ROOT


def _built():
    import __graft_entry__ as g
    g.build()
    from pdp_amd import codegen, runtime as rt
    return codegen, rt


def test_the_entry_point_is_declared_listed_and_exported():
    """(tests/test_abi_table.py holds the whole binding against the headers and the built libraries; what stays here is this header's own)"""
    codegen, rt = _built()
    from pdp_amd import abi
    assert list(abi.entry_points("pdp_hip_lm.h", "core")) == ["pdp_lm_update_batched"]
    assert rt.LM_STATES == lb.NAMES
    header = open(os.path.join(ROOT, "include", "pdp_hip_lm.h")).read()
    for value, name in enumerate(lb.NAMES):
        assert re.search(r"#define PDP_LM_%s %d\b" % (name, value), header), name
    assert os.path.join(codegen.CSRC, "pdp_lm_kernels.h") in codegen.source_closure(os.path.join(codegen.CSRC, "pdp_lqr.hip"))     # (part of the build stamp)


def test_argument_errors_are_returned_before_any_launch():
    """Valid (host) pointers everywhere, so that only the argument under test can be what is refused.  Nothing that passes the checks is called here: this machine may
    have no GPU."""
    codegen, rt = _built()
    fn = rt.load_core().pdp_lm_update_batched
    keep = [(C.c_double * 512)() for _ in range(16)]
    P = [C.cast(k, C.c_void_p).value for k in keep]
    K, S, p = 2, 2, 3
    w = p + 1 + p * p
    fields = [f[0] for f in rt.PdpLmState._fields_]

    def call(K=K, S=S, p=p, rows=P[0], stride=w, bad=P[1], sch=None, st=None, null_sch=False, null_st=False):
        sch = rt.PdpLmSchedule(10.0, 10.0, 1e-12, 1e8, 0.0, 50) if sch is None else sch
        full = dict(zip(fields, P[2:14] + [4, P[14]]))
        full.update(st or {})
        stt = rt.PdpLmState(*[full[f] for f in fields])
        return fn(K, S, p, rows, stride, bad, None if null_sch else C.byref(sch), None if null_st else C.byref(stt), None)
    for kw in (dict(K=0), dict(K=-1), dict(S=0), dict(p=0), dict(p=-2), dict(rows=None), dict(stride=w - 1), dict(stride=0), dict(null_sch=True), dict(null_st=True),
               dict(sch=rt.PdpLmSchedule(0.0, 10.0, 1e-12, 1e8, 0.0, 50)), dict(sch=rt.PdpLmSchedule(10.0, -1.0, 1e-12, 1e8, 0.0, 50)),
               dict(sch=rt.PdpLmSchedule(float("nan"), 10.0, 1e-12, 1e8, 0.0, 50)), dict(st=dict(trace_len=-1))) + \
            tuple(dict(st={f: None}) for f in ("theta", "trial", "lam", "current", "state", "evaluations", "rejected", "accepted", "counters")):
        assert call(**kw) == -1, kw                                               # PDP_E_ARG
    assert call(p=17, stride=17 + 1 + 17 * 17) == -2                              # PDP_E_SIZE
    assert call(p=17, stride=5) == -2 and call(p=17, rows=None) == -1             # (the size comes before the stride that depends on it, a null pointer before both)
    assert call(K=0, p=17) == -1
    assert all(v == 0.0 for k in keep for v in k)                                 # (and nothing was written by the host code)


@pytest.mark.parametrize("system, S", lb.SYSID_CASES, ids=["%s_K%d_S%d" % (s, 9 // n, n) for s, n in lb.SYSID_CASES])
def test_restatement_against_independent_lm_loops(system, S):
    """the lock-step restatement and K independent irl.LMLoop runs take the same decisions on the oracle's rows: evaluations, rejected and accepted counts equal per
    problem, every problem CONVERGED, the accepted losses above 1e-8 equal to solver rounding (pivoted elimination against numpy.linalg.solve)"""
    c = lb.sysid_case(system, S)
    st = lb.run(lb.oracle_rows(c), c["theta0"], S=S, **lb.SCHEDULE)
    loops = lb.independent_loops(c, **lb.SCHEDULE)
    print("%s K = %d S = %d: %d launches; evaluations %s rejected %s finished at launch %s" % (system, c["K"], S, st["launches"], list(st["evaluations"]), list(st["rejected"]),
                                                                                               list(st["finished_at"])))
    worst = 0.0
    for k, r in enumerate(loops):
        assert (st["evaluations"][k], st["rejected"][k], st["accepted"][k]) == (r["evaluations"], r["rejected"], r["iterations"]), (k, r["evaluations"], r["rejected"])
        assert st["state"][k] == lb.CONVERGED and not r["stalled"] and r["loss_trace"][-1] <= lb.SCHEDULE["loss_tol"], k
        a, b = st["loss_trace"][k, :st["accepted"][k]], r["loss_trace"]
        big = b > 1e-8
        worst = max(worst, float((np.abs(a - b)[big] / b[big]).max()))
        assert (np.diff(a) < 0).all()
    print("  accepted losses above 1e-8: largest relative difference %.2e" % worst)
    assert worst <= 1e-6
    if system == "pendulum" and S == 1:
        # the inputs must exercise a rejected trial and problems that finish at different launches (if this stops holding, the inputs are to be changed)
        assert st["rejected"].max() >= 1 and len(set(st["finished_at"])) >= 2


# ---- the rules at the edges, by hand -------------------------------------------------------------------------------------------------------------------------------------
def _row(g, loss, G):
    return np.concatenate([np.asarray(g, float), [loss], np.asarray(G, float).ravel()])[None]


def test_equal_loss_is_rejected_and_lam_moves():
    G = np.array([[2.0, 0.5], [0.5, 1.0]])
    st = lb.new_state([[1.0, -1.0]], 1, lam0=1e-3, trace_len=4)
    lb.launch(st, _row([1.0, 2.0], 5.0, G))
    assert st["state"][0] == lb.ACTIVE and st["accepted"][0] == 1 and st["lam"][0] == 1e-3 and st["accepted_now"][0] == 1          # START: accepted, lam stays
    step = np.linalg.solve(G + 1e-3 * np.diag(np.diag(G)), [1.0, 2.0])
    assert np.abs(st["trial"][0] - ([1.0, -1.0] - step)).max() <= 1e-15
    trial = st["trial"][0].copy()
    lb.launch(st, _row([1.0, 2.0], 5.0, G))                                       # an equal loss is rejected
    assert (st["rejected"][0], st["accepted"][0], st["lam"][0], st["accepted_now"][0]) == (1, 1, 1e-3 * 10.0, 0) and (st["theta"][0] == [1.0, -1.0]).all()
    lb.launch(st, _row([0.5, 0.5], 4.0, G))                                       # a lower one accepted: theta <- the trial that was evaluated
    assert st["accepted"][0] == 2 and st["lam"][0] == 1e-3 * 10.0 / 10.0 and st["loss_trace"][0, 1] == 4.0 and st["lambda_trace"][0, 1] == st["lam"][0]
    assert not (st["theta"][0] == trial).all() and st["evaluations"][0] == 3 and list(st["counters"]) == [3, 1]
    assert (st["parameter_trace"][0, 1] == st["theta"][0]).all() and (st["parameter_trace"][0, 0] == [1.0, -1.0]).all()


def test_zero_diagonal_entry_is_damped_by_lam_itself():
    G = np.array([[4.0, 0.0], [0.0, 0.0]])
    st = lb.new_state([[0.0, 0.0]], 1, lam0=0.5)
    lb.launch(st, _row([2.0, 3.0], 1.0, G))
    assert st["state"][0] == lb.ACTIVE and np.array_equal(st["trial"][0], [-2.0 / (4.0 + 0.5 * 4.0), -3.0 / 0.5])


def test_exactly_singular_damped_matrix_is_rejected_inside_the_launch():
    """G = c [[1, 1], [1, 1]], lam = 1e-20: 1 + lam == 1 until lam = 1e-15 - five trials that cannot be formed, counted, inside ONE launch"""
    G = 1.0 * np.ones((2, 2))               # (c = 1: c + lam c == c exactly as long as 1 + lam == 1)
    st = lb.new_state([[1.0, 2.0]], 1, lam0=1e-20)
    lb.launch(st, _row([0.0, 0.0], 1.0, G))
    assert (st["evaluations"][0], st["rejected"][0], st["accepted"][0], st["state"][0]) == (6, 5, 1, lb.ACTIVE)
    assert abs(st["lam"][0] / 1e-15 - 1.0) < 1e-12 and 1.0 + st["lam"][0] > 1.0 and np.array_equal(st["trial"][0], [1.0, 2.0])
    # with a budget of four evaluations the same launch ends in BUDGET after three of them
    st = lb.new_state([[1.0, 2.0]], 1, lam0=1e-20)
    lb.launch(st, _row([0.0, 0.0], 1.0, G), max_evals=4)
    assert (st["evaluations"][0], st["rejected"][0], st["state"][0]) == (4, 3, lb.BUDGET) and list(st["counters"]) == [1, 0]
    x, ok = lb.solve_pivoted([[0.0, 1.0], [2.0, 0.0]], [3.0, 4.0])                # (a zero in front is pivoted away, not a failure)
    assert ok and np.array_equal(x, [2.0, 3.0])
    assert not lb.solve_pivoted(np.ones((3, 3)), [1.0, 1.0, 1.0])[1]
    A = np.array([[1.0, 2.0, 0.0], [-4.0, 1.0, 1.0], [4.0, 0.5, 3.0]])            # |-4| == |4|: the tie goes to the lower row
    x, ok = lb.solve_pivoted(A, A @ [1.0, -2.0, 3.0])
    assert ok and np.abs(x - [1.0, -2.0, 3.0]).max() <= 1e-14


def test_lam_min_floor_stalled_budget_converged_and_failed():
    G = np.eye(2)
    st = lb.new_state([[0.0, 0.0]] * 5, 1, lam0=[5e-12, 5e7, 1e-3, 1e-3, 1e-3], trace_len=1)
    rows = np.concatenate([_row([1.0, 1.0], 5.0, G)] * 5)
    rows[3, 2] = np.nan                                                           # problem 3: the initial point cannot be evaluated
    rows[4, 2] = 1e-9                                                             # problem 4: below loss_tol at START
    bad = np.zeros(5, dtype=np.int32)
    lb.launch(st, rows, bad, loss_tol=1e-6, max_evals=3)
    assert list(st["state"]) == [lb.ACTIVE, lb.ACTIVE, lb.ACTIVE, lb.FAILED, lb.CONVERGED] and list(st["counters"]) == [1, 3]
    assert np.array_equal(st["trial"][3], st["theta"][3]) and st["evaluations"][3] == 1 and st["accepted"][3] == 0
    rows = np.concatenate([_row([1.0, 1.0], v, G) for v in (4.0, 6.0, 4.0, 1.0, 1.0)])
    bad[2] = 1                                                                    # problem 2: a lower loss, but flagged
    lb.launch(st, rows, bad, loss_tol=1e-6, max_evals=3)
    assert st["lam"][0] == 1e-12 and st["state"][0] == lb.ACTIVE                  # max(5e-13, lam_min)
    assert st["lam"][1] == 5e7 * 10.0 and st["state"][1] == lb.STALLED and st["rejected"][1] == 1
    assert st["rejected"][2] == 1 and st["state"][2] == lb.ACTIVE
    assert st["evaluations"][3] == 1 and st["evaluations"][4] == 1                # finished problems are left alone
    assert st["accepted"][0] == 2 and st["loss_trace"][0, 0] == 5.0               # (a trace of one entry is full: the second acceptance is not written)
    lb.launch(st, rows, None, loss_tol=1e-6, max_evals=3)
    assert list(st["state"]) == [lb.BUDGET, lb.STALLED, lb.BUDGET, lb.FAILED, lb.CONVERGED] and list(st["counters"]) == [3, 0]
    assert np.array_equal(st["trial"], st["theta"])
