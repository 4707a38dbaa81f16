"""GPU: pdp_lm_update_batched (csrc/pdp_lm_kernels.h) - the Levenberg-Marquardt update of many independent problems as one launch - against its numpy restatement
(tests/lm_batched_common.py) on scripted synthetic rows, placement independence, and irl.BatchedLMLoop on the stored SysID and IRL data against the restatement on the
oracle and against K separate irl.LMLoop runs on the device.

Tolerances: decisions (states, counters, accepted_now) and lam exactly; theta, current and traces within 1e-14 of the buffer's largest entry (copies, ordered sums and
one division: bit equality is expected and printed); trial within 1e-10 of its largest entry (the project's HIP-vs-oracle tolerance; elimination
at cond <= 1e3 and p <= 16 predicts about 2e-12).  After each comparison the restatement continues from the KERNEL's trial points (theta is a copy of the trial point
that was evaluated), so that every launch is compared on its own."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import lm_batched_common as lb
import sysid_gn_common as sg

pytestmark = pytest.mark.gpu
ROOT = sg.ROOT
GUARD = 3                       # rows of NaN (int32: -77) behind every buffer that must stay as they are
F64 = ("theta", "trial", "lam", "current", "loss_trace", "lambda_trace", "parameter_trace")
I32 = ("state", "evaluations", "rejected", "accepted", "accepted_now")
OPTIONAL = ("accepted_now", "loss_trace", "lambda_trace", "parameter_trace")


def npy(t):
    return t.detach().cpu().numpy()


class Device:
    """the state of lb.new_state on the device, every buffer with GUARD guard rows behind it"""

    def __init__(self, st, optional=True):
        import torch
        self.full, self.view, self.optional = {}, {}, optional
        for key in F64 + I32 + ("counters",):
            a = st[key]
            if key in I32:
                full = torch.full((a.shape[0] + GUARD,) + a.shape[1:], -77, dtype=torch.int32, device="cuda")
            elif key == "counters":
                full = torch.full((2 + GUARD,), -77, dtype=torch.int64, device="cuda")
            else:
                full = torch.full((a.shape[0] + GUARD,) + a.shape[1:], float("nan"), dtype=torch.float64, device="cuda")
            full[:a.shape[0]] = torch.as_tensor(a, device="cuda")
            self.full[key], self.view[key] = full, full[:a.shape[0]]

    def update(self, rows, bad, **schedule):
        from pdp_amd import runtime as rt
        v = self.view
        opt = {k: v[k] for k in OPTIONAL} if self.optional else {}
        rt.lm_update(rows, v["theta"], v["trial"], v["lam"], v["current"], v["state"], v["evaluations"], v["rejected"], v["accepted"], v["counters"], bad=bad, **opt, **schedule)

    def host(self):
        return {k: npy(t) for k, t in self.view.items()}

    def guards_untouched(self):
        for key, full in self.full.items():
            g = npy(full[self.view[key].shape[0]:])
            assert (g == -77).all() if g.dtype.kind == "i" else np.isnan(g).all(), "guard rows of %s were written" % key


def strided(rows):
    """rows in a wider, longer buffer of NaN: (the buffer, the [K S, w] view the kernel gets)"""
    import torch
    n, w = rows.shape
    buf = torch.full((n + GUARD, w + 3), float("nan"), dtype=torch.float64, device="cuda")
    buf[:n, :w] = torch.as_tensor(rows, device="cuda")
    return buf, buf[:n, :w]


def compare(margins, tag, got, st, optional=True):
    """one launch: the device state against the restatement's; returns whether every fp64 buffer is bit-equal"""
    for key in I32 + ("counters",):
        if key in OPTIONAL and not optional:
            continue
        assert np.array_equal(got[key], st[key]), "%s: %s %s != %s" % (tag, key, got[key].tolist(), st[key].tolist())
    assert np.array_equal(got["lam"], st["lam"]), "%s: lam %s != %s" % (tag, got["lam"], st["lam"])
    bits = True
    for key in ("theta", "current", "loss_trace", "lambda_trace", "parameter_trace", "trial"):
        if key in OPTIONAL and not optional:
            continue
        a, b = got[key], st[key]
        assert np.isfinite(a).all(), "%s: %s is not finite" % (tag, key)
        bits = bits and np.array_equal(a, b)
        if a.size:
            margins.check("%s: %s" % (tag, key), np.abs(a - b).max() / max(np.abs(b).max(), 1e-300), 1e-10 if key == "trial" else 1e-14)
    return bits


SHAPES = [(1, 1, 1), (5, 1, 5), (3, 1, 13), (9, 3, 9), (4, 1, 16), (67, 2, 16)]


@pytest.mark.parametrize("K, S, p", SHAPES, ids=["K%d_S%d_p%d" % s for s in SHAPES])
def test_kernel_against_the_restatement_on_scripted_rows(margins, K, S, p):
    """four scripted launches (lb.SCENARIOS: problem k plays scenario k % 10) and two more on fresh rows, strided rows, a trace of two entries; then the same script with
    every optional pointer null.  One lane (p = 1), odd p, K not a multiple of the four problems per wavefront, the full tile, more than one workgroup."""
    import torch
    rng = np.random.default_rng(K * 100 + p)
    theta0 = rng.standard_normal((K, p))
    played = sorted({k % len(lb.SCENARIOS) for k in range(K)})
    for optional in (True, False):
        st = lb.new_state(theta0, S, lam0=lb.script_lam0(K), trace_len=lb.SCRIPT_TRACE_LEN)
        dv = Device(st, optional)
        bits, seen, before = True, set(), None
        for n in range(6):
            rows, bad = lb.script_rows(K, S, p, n, seed=p)
            if not optional:
                bad = None                      # (the "bad" launches are then ordinary ones, for kernel and restatement alike)
            buf, view = strided(rows) if optional else (None, torch.as_tensor(rows, device="cuda"))
            dv.update(view, torch.as_tensor(bad, device="cuda") if bad is not None else None, **lb.SCRIPT_SCHEDULE)
            lb.launch(st, rows, bad, **lb.SCRIPT_SCHEDULE)
            got = dv.host()
            tag = "LM kernel K=%d S=%d p=%d %s launch %d" % (K, S, p, "all outputs" if optional else "optional pointers null", n)
            bits = compare(margins, tag, got, st, optional) and bits
            dv.guards_untouched()
            if buf is not None:
                assert np.isnan(npy(buf[:, -3:])).all() and np.isnan(npy(buf[-GUARD:])).all()
            st["trial"][:] = got["trial"]       # (continue from the kernel's trial points: see the header)
            seen |= set(st["state"].tolist())
            if n == 3:                          # the script is over: what is finished now must not change any more
                before = {k: v.copy() for k, v in got.items()}
                done = ~np.isin(st["state"], (lb.START, lb.ACTIVE))
        got = dv.host()
        for key in ("theta", "lam", "current", "state", "evaluations", "rejected", "accepted", "loss_trace", "lambda_trace", "parameter_trace"):
            if key in OPTIONAL and not optional:
                continue
            assert np.array_equal(got[key][done], before[key][done], equal_nan=True), "%s of a finished problem changed in a later launch" % key
        assert np.array_equal(got["trial"].reshape(K, S, p)[done], np.repeat(got["theta"][done][:, None], S, axis=1))
        if optional:
            assert not got["accepted_now"].reshape(K, S)[done].any()
        print("K=%d S=%d p=%d %s: scenarios %s, states seen %s, fp64 buffers bit-equal to the restatement: %s"
              % (K, S, p, "all outputs" if optional else "optional pointers null", played, sorted(lb.NAMES[s] for s in seen), bits))
        if K >= len(lb.SCENARIOS) and optional:
            assert seen >= {lb.ACTIVE, lb.CONVERGED, lb.STALLED, lb.BUDGET, lb.FAILED}
            singular = 4
            assert st["evaluations"][singular] == 8 and st["rejected"][singular] >= 5 and st["state"][singular] == lb.BUDGET
            assert (st["accepted"] > lb.SCRIPT_TRACE_LEN).any()                   # a full trace was met


def test_placement_independence(margins):
    """problem computed alone (K = 1) and inside K = 9 at positions 0, 3, 4, 8 (first and last quarter of a wavefront, the next wavefront, the last problem): bit-equal"""
    import torch
    S, p, K = 2, 7, 9
    sch = dict(lb.SCRIPT_SCHEDULE, loss_tol=0.0, max_evals=50)
    rng = np.random.default_rng(5)
    theta_own, theta_other = rng.standard_normal((1, p)), rng.standard_normal((K, p))
    losses = [5.0, 4.0, 4.5, 3.0]               # accept, accept, reject, accept

    def own_rows(n):
        rows = lb.script_rows(1, S, p, 0, seed=100 + n)[0]
        rows[:, p] *= losses[n] / 5.0
        return rows

    def play(K_, pos):
        theta0 = theta_other[:K_].copy()
        theta0[pos] = theta_own[0]
        dv = Device(lb.new_state(theta0, S, lam0=1e-3, trace_len=4))
        for n in range(4):
            rows = lb.script_rows(K_, S, p, n, seed=7)[0]
            rows[pos * S:(pos + 1) * S] = own_rows(n)
            dv.update(torch.as_tensor(rows, device="cuda"), None, **sch)
        got = dv.host()
        return {k: (v.reshape(K_, -1)[pos] if k != "counters" else None) for k, v in got.items()}
    alone = play(1, 0)
    assert alone["accepted"][0] == 3 and alone["rejected"][0] == 1 and alone["state"][0] == lb.ACTIVE
    for pos in (0, 3, 4, 8):
        inside = play(K, pos)
        for key in F64 + I32:
            assert np.array_equal(alone[key], inside[key]), "position %d: %s differs from the problem computed alone" % (pos, key)


# ---- BatchedLMLoop on the stored SysID data --------------------------------------------------------------------------------------------------------------------------------
# the partial-data case: pendulum, component 0 at t = 2, 4, .., 20, a given initial state, K = 3 - the three start scales, each problem with all three trajectories
# (S = 3).  With one trajectory per problem the data of trajectory 1 alone do not pin the parameters: the oracle's schedule itself crawls there (30 evaluations, loss
# 9e-5), so "every problem CONVERGED" can only be asked of the grouping in which the restatement converges (6, 6, 7 evaluations).
SYSID = [(s, S, False) for s, S in lb.SYSID_CASES if (s, S) != ("cartpole", 3)] + [("pendulum", 3, True)]


def _case(system, S, partial):
    c = lb.sysid_case(system, S)
    if not partial:
        return c, None
    _, states, _, _ = sg.stored(system)
    c["states"] = np.concatenate([sg.observe(states, every=2, components=[0])] * len(lb.SCALES))
    return c, np.concatenate([states[:, 0]] * len(lb.SCALES))


@functools.lru_cache(maxsize=None)
def _restated(system, S, partial):
    c, ini = _case(system, S, partial)
    st = lb.run(lb.oracle_rows(c, ini, partial), c["theta0"], S=S, **lb.SCHEDULE)
    assert (st["state"] == lb.CONVERGED).all()
    return st


@pytest.mark.parametrize("system, S, partial", SYSID, ids=["%s_S%d%s" % (s, S, "_partial" if pt else "") for s, S, pt in SYSID])
def test_for_sysid(margins, system, S, partial):
    from pdp_amd import zoo
    from pdp_amd.irl import BatchedLMLoop, LMLoop
    c, ini = _case(system, S, partial)
    ref = _restated(system, S, partial)
    mdl = zoo.get(system, "sysid")
    loop = BatchedLMLoop.for_sysid(mdl, c["inputs"], c["states"], c["theta0"], samples_per_problem=S, ini_state=ini, skip_missing=partial, **lb.SCHEDULE)
    r = loop.run()
    tag = "BatchedLMLoop.for_sysid %s K=%d S=%d%s" % (system, c["K"], S, " partial data" if partial else "")
    print("%s: %d launches (restatement %d); evaluations %s (restatement %s); rejected %s; states %s" % (tag, r["launches"], ref["launches"], r["evaluations"].tolist(),
                                                                                                         ref["evaluations"].tolist(), r["rejected"].tolist(), r["state"]))
    assert r["state"] == ["CONVERGED"] * c["K"]
    assert (r["evaluations"] <= 2 * ref["evaluations"]).all() and r["launches"] <= 2 * ref["launches"]
    assert (r["loss"] <= 1e-10).all()
    for k in range(c["K"]):
        assert (np.diff(r["loss_trace"][k]) < 0).all() and r["loss_trace"][k][-1] == r["loss"][k] and len(r["loss_trace"][k]) == r["accepted"][k]
        assert np.array_equal(r["parameter_trace"][k][-1], r["theta"][k])
    if not partial and system in ("pendulum", "cartpole"):
        assert np.abs(r["theta"] - c["true_parameter"]).max() <= 1e-6
    # K separate host-driven loops on the device, each on its own slice
    worst, same = 0.0, True
    for k in range(c["K"]):
        sl = slice(k * S, (k + 1) * S)
        one = LMLoop.for_sysid(mdl, c["inputs"][sl], c["states"][sl], c["theta0"][k], ini_state=None if ini is None else ini[sl], skip_missing=partial)
        o = one.run(max_evals=lb.SCHEDULE["max_evals"], loss_tol=lb.SCHEDULE["loss_tol"])
        same = same and (o["evaluations"], o["rejected"], o["iterations"]) == (r["evaluations"][k], r["rejected"][k], r["accepted"][k])
        n = min(len(o["loss_trace"]), len(r["loss_trace"][k]))
        a, b = r["loss_trace"][k][:n], o["loss_trace"][:n]
        big = b > 1e-8
        worst = max(worst, float((np.abs(a - b)[big] / b[big]).max()))
    print("  against %d separate LMLoop.for_sysid runs: counts equal: %s; accepted losses above 1e-8 differ by %.2e relative" % (c["K"], same, worst))
    margins.check(tag + ": accepted losses above 1e-8 vs separate LMLoop runs", worst, 1e-6)


def test_for_sysid_argument_rules():
    from pdp_amd import zoo
    from pdp_amd.irl import BatchedLMLoop
    inputs, states, _, theta = sg.stored("pendulum")
    with pytest.raises(ValueError, match="ini_state"):
        BatchedLMLoop.for_sysid(zoo.get("pendulum", "sysid"), inputs, sg.observe(states, every=2, components=[0]), theta, skip_missing=True)
    loop = BatchedLMLoop.for_sysid(zoo.get("pendulum", "sysid"), inputs, states, theta, max_evals=5)               # theta0 [p] is broadcast to the K problems
    assert tuple(loop.theta.shape) == (3, theta.size) and tuple(loop.trial.shape) == (3, theta.size)
    loop.step()
    assert loop.active() == 3 and loop.results()["state"] == ["ACTIVE"] * 3 and loop.results()["evaluations"].tolist() == [1, 1, 1]


# ---- BatchedLMLoop on the stored demonstrations -----------------------------------------------------------------------------------------------------------------------------
def _demos(system):
    d = np.load(os.path.join(ROOT, "tests", "golden", "demos_%s.npz" % system))
    return d, np.load(os.path.join(ROOT, "tests", "golden", "irltrace_head_%s.npz" % system))["param"][0]


def test_for_irl_pendulum():
    """one IRL problem per stored demonstration (K = 5, S = 1): the oracle's schedule needs 6 - 7 evaluations per problem"""
    from pdp_amd import zoo
    from pdp_amd.irl import BatchedLMLoop
    d, theta0 = _demos("pendulum")
    assert d["state"].shape == (5, 21, 2)
    r = BatchedLMLoop.for_irl(zoo.get("pendulum", "irl"), d["state"], d["control"], theta0, max_evals=14, loss_tol=1e-16).run()
    print("BatchedLMLoop.for_irl pendulum: launches %d evaluations %s rejected %s states %s final losses %s" % (r["launches"], r["evaluations"].tolist(), r["rejected"].tolist(),
                                                                                                                r["state"], r["loss"]))
    assert r["state"] == ["CONVERGED"] * 5 and (r["evaluations"] <= 14).all()
    assert (r["loss"] <= 1e-10).all()
    for k in range(5):
        assert (np.diff(r["loss_trace"][k]) < 0).all()


def test_for_irl_cartpole_is_reported():
    """cart-pole demonstrations 0, 1, 3, 4 (demonstration 2 crawls for the oracle's schedule as well): run and printed, nothing asserted on the outcome"""
    from pdp_amd import zoo
    from pdp_amd.irl import BatchedLMLoop
    d, theta0 = _demos("cartpole")
    pick = [0, 1, 3, 4]
    r = BatchedLMLoop.for_irl(zoo.get("cartpole", "irl"), d["state"][pick], d["control"][pick], theta0, max_evals=18, loss_tol=1e-16).run()
    print("BatchedLMLoop.for_irl cartpole demonstrations %s: launches %d evaluations %s rejected %s states %s final losses %s"
          % (pick, r["launches"], r["evaluations"].tolist(), r["rejected"].tolist(), r["state"], r["loss"]))


def test_example_per_trajectory():
    """examples/sysid_pdp.py --method lm --per-trajectory: one line per stored trajectory with evaluations, state and final loss; every problem CONVERGED"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "sysid_pdp.py"), "--system", "pendulum", "--method", "lm", "--per-trajectory"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("problem")]
    assert len(lines) == 3 and all("CONVERGED" in ln and "evaluations" in ln for ln in lines), r.stdout[-3000:]
    assert all(float(ln.split(" -> ")[1].split()[0]) <= 1e-10 for ln in lines), r.stdout[-3000:]
    assert len([ln for ln in r.stdout.splitlines() if ln.startswith("done:")]) == 1
