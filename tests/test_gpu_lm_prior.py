"""GPU: the Gaussian prior inside the batched Levenberg-Marquardt update (pdp_lm_update_prior_batched) and the covariance kernel (pdp_lm_covariance_batched), both in
csrc/pdp_lm_kernels.h, against their numpy restatement (tests/lm_prior_common.py) - in the harness of tests/test_gpu_lm_batched.py: guard rows behind every buffer,
strided rows, the restatement continuing from the kernel's trial points - and irl.BatchedLMLoop / irl.LMLoop with a prior and with covariance() on the stored SysID and
IRL data against the restatement on the oracle.

Tolerances: decisions (states, counters, accepted_now, status) and lam exactly; theta, current, traces and prior_loss within 1e-14 of the buffer's largest entry (ordered
sums: bit equality is expected and printed); trial, cov, std_err and pivot_ratio within 1e-10 of the problem's largest entry (elimination at cond
<= 1e3 and p <= 16 predicts about 2e-12)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import lm_batched_common as lb
import lm_prior_common as lp
import sysid_gn_common as sg
import test_gpu_lm_batched as tb

pytestmark = pytest.mark.gpu
ROOT = sg.ROOT
GUARD = tb.GUARD
npy = tb.npy


def guarded(a, dtype=None):
    """(the buffer with GUARD guard rows of NaN / -77 behind it, the view the kernel gets)"""
    import torch
    a = np.asarray(a)
    if a.dtype.kind == "i":
        full = torch.full((a.shape[0] + GUARD,) + a.shape[1:], -77, dtype=torch.int32, device="cuda")
    else:
        full = torch.full((a.shape[0] + GUARD,) + a.shape[1:], float("nan"), dtype=torch.float64, device="cuda")
    full[:a.shape[0]] = torch.as_tensor(a, device="cuda")
    return full, full[:a.shape[0]]


def guard_untouched(full, n):
    g = npy(full[n:])
    return (g == -77).all() if g.dtype.kind == "i" else np.isnan(g).all()


class PriorDevice(tb.Device):
    """tb.Device whose update launches pdp_lm_update_prior_batched with the prior of a restatement dict"""

    def __init__(self, st, prior, optional=True):
        super().__init__(st, optional)
        self.prior = prior
        if prior is not None:
            self.mean, self.precision = (guarded(prior[k]) for k in ("mean", "precision"))
            self.prior_loss = guarded(prior["prior_loss"]) if prior.get("prior_loss") is not None else None

    def update(self, rows, bad, **schedule):
        from pdp_amd import runtime as rt
        v = self.view
        opt = {k: v[k] for k in tb.OPTIONAL} if self.optional else {}
        pr = {}
        if self.prior is not None:
            pr = dict(prior_mean=self.mean[1], prior_precision=self.precision[1], prior_loss=self.prior_loss[1] if self.prior_loss else None,
                      diagonal_per_problem=self.prior["kind"] == 0 and self.precision[1].dim() == 2)
        rt.lm_update_prior(rows, v["theta"], v["trial"], v["lam"], v["current"], v["state"], v["evaluations"], v["rejected"], v["accepted"], v["counters"], bad=bad, **opt,
                           **pr, **schedule)

    def guards_untouched(self):
        super().guards_untouched()
        if self.prior is not None:
            for full, view in (self.mean, self.precision) + ((self.prior_loss,) if self.prior_loss else ()):
                assert guard_untouched(full, view.shape[0])


def make_prior(K, p, theta0, variant, seed):
    """the four layouts: diagonal / full precision, shared (stride 0) / one per problem; the mean near the start points, the precision of the order of a tenth of the
    scripted G (eigenvalues in [1, 1e3]), so that neither the data nor the prior decides alone"""
    rng = np.random.default_rng([seed, K, p])
    per = variant.endswith("per problem")
    n = K if per else 1
    mean = theta0[:n] + 0.3 * rng.standard_normal((n, p))
    if variant.startswith("diagonal"):
        prec = rng.uniform(0.0, 20.0, (n, p))
        prec[:, p // 2] = 0.0                                                     # (an unknown the prior says nothing about)
    else:
        M = rng.standard_normal((n, p, p))
        prec = 10.0 * M @ M.transpose(0, 2, 1) / p
        prec = 0.5 * (prec + prec.transpose(0, 2, 1))
    return dict(mean=mean if per else mean[0], precision=prec if per else prec[0], kind=0 if variant.startswith("diagonal") else 1, prior_loss=np.full(K, np.nan))


VARIANTS = ["diagonal shared", "diagonal per problem", "full shared", "full per problem"]


@pytest.mark.parametrize("K, S, p", tb.SHAPES, ids=["K%d_S%d_p%d" % s for s in tb.SHAPES])
def test_update_kernel_with_a_prior_against_the_restatement(margins, K, S, p):
    """the six scripted launches of the update test with each of the four prior layouts (the last one also with every optional pointer null, prior_loss included)"""
    import torch
    rng = np.random.default_rng(K * 100 + p)
    theta0 = rng.standard_normal((K, p))
    for variant, optional in [(v, True) for v in VARIANTS] + [(VARIANTS[-1], False)]:
        prior = make_prior(K, p, theta0, variant, seed=7)
        if not optional:
            prior["prior_loss"] = None
        st = lb.new_state(theta0, S, lam0=lb.script_lam0(K), trace_len=lb.SCRIPT_TRACE_LEN)
        dv = PriorDevice(st, prior, optional)
        bits, seen = True, set()
        for n in range(6):
            rows, bad = lb.script_rows(K, S, p, n, seed=p)
            if not optional:
                bad = None
            buf, view = tb.strided(rows) if optional else (None, torch.as_tensor(rows, device="cuda"))
            dv.update(view, torch.as_tensor(bad, device="cuda") if bad is not None else None, **lb.SCRIPT_SCHEDULE)
            lp.launch_prior(st, rows, bad, prior, **lb.SCRIPT_SCHEDULE)
            got = dv.host()
            tag = "LM prior kernel K=%d S=%d p=%d %s%s launch %d" % (K, S, p, variant, "" if optional else ", optional pointers null", n)
            bits = tb.compare(margins, tag, got, st, optional) and bits
            if optional:
                a, b = npy(dv.prior_loss[1]), prior["prior_loss"]
                assert np.array_equal(np.isnan(a), np.isnan(b)), tag
                if (~np.isnan(b)).any():
                    bits = bits and np.array_equal(a, b, equal_nan=True)
                    margins.check(tag + ": prior_loss", np.nanmax(np.abs(a - b)) / max(np.nanmax(np.abs(b)), 1e-300), 1e-14)
            dv.guards_untouched()
            if buf is not None:
                assert np.isnan(npy(buf[:, -3:])).all() and np.isnan(npy(buf[-GUARD:])).all()
            st["trial"][:] = got["trial"]           # (continue from the kernel's trial points)
            seen |= set(st["state"].tolist())
        print("K=%d S=%d p=%d %s%s: states seen %s, accepted %s rejected %s, fp64 buffers bit-equal to the restatement: %s"
              % (K, S, p, variant, "" if optional else " (optional pointers null)", sorted(lb.NAMES[s] for s in seen), st["accepted"].tolist()[:10], st["rejected"].tolist()[:10], bits))
        if K >= len(lb.SCENARIOS) and optional:
            assert seen >= {lb.ACTIVE, lb.FAILED} and st["rejected"].max() >= 1 and st["accepted"].max() >= 2


def test_null_prior_is_the_plain_entry_point():
    """pdp_lm_update_prior_batched(prior = NULL) and pdp_lm_update_batched over the scripted six launches at K = 10, S = 2, p = 7: every buffer bit-equal"""
    import torch
    K, S, p = 10, 2, 7
    theta0 = np.random.default_rng(1).standard_normal((K, p))
    a = tb.Device(lb.new_state(theta0, S, lam0=lb.script_lam0(K), trace_len=lb.SCRIPT_TRACE_LEN))
    b = PriorDevice(lb.new_state(theta0, S, lam0=lb.script_lam0(K), trace_len=lb.SCRIPT_TRACE_LEN), None)
    for n in range(6):
        rows, bad = lb.script_rows(K, S, p, n, seed=p)
        for dv in (a, b):
            dv.update(torch.as_tensor(rows, device="cuda"), torch.as_tensor(bad, device="cuda"), **lb.SCRIPT_SCHEDULE)
        ga, gb = a.host(), b.host()
        for key in ga:
            assert np.array_equal(ga[key], gb[key], equal_nan=True), (n, key)
        b.guards_untouched()
    assert set(ga["state"].tolist()) >= {lb.ACTIVE, lb.CONVERGED, lb.STALLED, lb.BUDGET, lb.FAILED}


def test_placement_independence_with_a_prior():
    """a problem with its own prior computed alone (K = 1) and inside K = 9 at positions 0, 3, 4, 8: bit-equal, prior_loss included"""
    import torch
    S, p, K = 2, 7, 9
    sch = dict(lb.SCRIPT_SCHEDULE, loss_tol=0.0, max_evals=50)
    rng = np.random.default_rng(5)
    theta_own, theta_other = rng.standard_normal((1, p)), rng.standard_normal((K, p))
    own_prior, other_prior = make_prior(1, p, theta_own, "full per problem", 3), make_prior(K, p, theta_other, "full per problem", 4)

    def play(K_, pos):
        theta0 = theta_other[:K_].copy()
        theta0[pos] = theta_own[0]
        prior = dict(mean=other_prior["mean"][:K_].copy(), precision=other_prior["precision"][:K_].copy(), kind=1, prior_loss=np.full(K_, np.nan))
        prior["mean"][pos], prior["precision"][pos] = own_prior["mean"][0], own_prior["precision"][0]
        dv = PriorDevice(lb.new_state(theta0, S, lam0=1e-3, trace_len=4), prior)
        for n in range(4):
            rows = lb.script_rows(K_, S, p, n, seed=7)[0]
            rows[pos * S:(pos + 1) * S] = lb.script_rows(1, S, p, 0, seed=100 + n)[0]
            dv.update(torch.as_tensor(rows, device="cuda"), None, **sch)
        got = dict(dv.host(), prior_loss=npy(dv.prior_loss[1]))
        return {k: (v.reshape(K_, -1)[pos] if k != "counters" else None) for k, v in got.items()}
    alone = play(1, 0)
    assert alone["accepted"][0] >= 2 and np.isfinite(alone["prior_loss"]).all()
    for pos in (0, 3, 4, 8):
        inside = play(K, pos)
        for key in tb.F64 + tb.I32 + ("prior_loss",):
            assert np.array_equal(alone[key], inside[key]), "position %d: %s differs from the problem computed alone" % (pos, key)


# ---- the covariance kernel --------------------------------------------------------------------------------------------------------------------------------------------------
COV_SHAPES = [(1, 1), (5, 5), (3, 13), (4, 16), (67, 16)]


def cov_launch(rows, scale, p, want=("std_err", "pivot_ratio")):
    """the entry point itself on guarded buffers and strided rows: dict of host arrays"""
    import ctypes as C
    import torch
    from pdp_amd import runtime as rt
    K = rows.shape[0]
    buf, view = tb.strided(rows)
    out = {"cov": guarded(np.zeros((K, p, p))), "std_err": guarded(np.zeros((K, p))), "pivot_ratio": guarded(np.zeros(K)), "status": guarded(np.zeros(K, dtype=np.int32))}
    sc = torch.as_tensor(scale, device="cuda") if scale is not None else None
    rt.check(rt.load_core().pdp_lm_covariance_batched(K, p, rt.ptr(view), int(view.stride(0)), rt.ptr(sc), rt.ptr(out["cov"][1]),
                                                      rt.ptr(out["std_err"][1]) if "std_err" in want else None, rt.ptr(out["pivot_ratio"][1]) if "pivot_ratio" in want else None,
                                                      rt.ptr(out["status"][1]), rt.current_stream_ptr()), "pdp_lm_covariance_batched")
    torch.cuda.synchronize()
    for key, (full, v) in out.items():
        assert guard_untouched(full, K), key
    assert np.isnan(npy(buf[:, -3:])).all() and np.isnan(npy(buf[-GUARD:])).all()
    return {k: npy(v) for k, (full, v) in out.items()}


@pytest.mark.parametrize("K, p", COV_SHAPES, ids=["K%d_p%d" % s for s in COV_SHAPES])
def test_covariance_kernel_against_the_restatement(margins, K, p):
    """seeded symmetric positive definite matrices (cond 1e3) with - from K = 3 on - an exactly singular problem at 1 and one with a NaN at 2, scale null and given"""
    from pdp_amd import runtime as rt
    mats = [lp.spd(p, s) for s in range(K)]
    if K >= 3:
        mats[1] = np.ones((p, p))
        mats[2] = mats[2].copy()
        mats[2][p - 1, p // 2] = np.nan
    if K >= 5:
        P = np.eye(p)[::-1]
        mats[4] = P @ np.diag(np.arange(1.0, p + 1.0))                            # (needs a row exchange at every step but the middle one)
    rows = lp.cov_rows(mats)
    failed = [1, 2] if K >= 3 else []
    for scale in (None, np.random.default_rng(K).uniform(0.5, 2.0, K)):
        ref = lp.covariance(rows, scale)
        got = cov_launch(rows, scale, p)
        tag = "covariance kernel K=%d p=%d scale %s" % (K, p, "null" if scale is None else "given")
        assert got["status"].tolist() == ref["status"].tolist() == [1 if k in failed else 0 for k in range(K)], tag
        bits = True
        for k in range(K):
            if k in failed:
                assert np.isnan(got["cov"][k]).all() and np.isnan(got["std_err"][k]).all() and got["pivot_ratio"][k] == 0.0, (tag, k)
                continue
            big = np.abs(ref["cov"][k]).max()
            margins.check("%s problem %d: cov" % (tag, k), np.abs(got["cov"][k] - ref["cov"][k]).max() / big, 1e-10)
            margins.check("%s problem %d: std_err" % (tag, k), np.abs(got["std_err"][k] - ref["std_err"][k]).max() / max(np.abs(ref["std_err"][k]).max(), 1e-300), 1e-10)
            margins.check("%s problem %d: pivot_ratio" % (tag, k), abs(got["pivot_ratio"][k] - ref["pivot_ratio"][k]) / ref["pivot_ratio"][k], 1e-10)
            bits = bits and np.array_equal(got["cov"][k], ref["cov"][k])
            if np.isfinite(mats[k]).all():
                assert np.abs(got["cov"][k] @ mats[k] / (1.0 if scale is None else scale[k]) - np.eye(p)).max() <= 1e-10
        print("%s: cov bit-equal to the restatement: %s" % (tag, bits))
        # the optional outputs null: cov and status as before
        bare = cov_launch(rows, scale, p, want=())
        assert np.array_equal(bare["cov"], got["cov"], equal_nan=True) and np.array_equal(bare["status"], got["status"])
        assert not bare["std_err"].any() and not bare["pivot_ratio"].any()       # (left as they were)
        # the neighbours of a failed problem: bit-equal to their result alone
        if K >= 4:
            for k in (0, 3):
                alone = cov_launch(rows[k:k + 1], None if scale is None else scale[k:k + 1], p)
                for key in ("cov", "std_err", "pivot_ratio", "status"):
                    assert np.array_equal(alone[key][0], got[key][k]), (tag, k, key)
    # the Python wrapper: packed rows, its own outputs
    import torch
    out = rt.lm_covariance(torch.as_tensor(rows, device="cuda"))
    ref = lp.covariance(rows)
    assert npy(out["status"]).tolist() == ref["status"].tolist() and np.array_equal(npy(out["cov"]), cov_launch(rows, None, p)["cov"], equal_nan=True)


# ---- BatchedLMLoop with a prior and with covariance() on the stored SysID data -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 3], ids=["K9_S1", "K3_S3"])
def test_for_sysid_with_a_prior(margins, S):
    """pendulum from the starts of lp.prior_starts under lp.PRIOR_SCHEDULE (why these: tests/lm_prior_common.py), a full prior in natural units: counts equal to the
    restatement on the oracle (which gets P / S, the scale of the mean row); accepted losses within 1e-6 relative; covariance("known") against numpy on the oracle's rows
    at the returned theta: (sum of the samples' G + P)^-1, within 10 cond 1e-10 (the rows agree to 1e-10; the inverse amplifies by the condition
    number); problem 0 of S = 3 also as irl.LMLoop.for_sysid on its three trajectories with the same natural-unit prior"""
    from pdp_amd import zoo
    from pdp_amd.irl import BatchedLMLoop, LMLoop
    c = lb.sysid_case("pendulum", S)
    K, p = c["K"], c["theta0"].shape[1]
    mean, P = lp.pendulum_prior(c)
    theta0 = lp.prior_starts(c)
    ref = lp.run_prior(lb.oracle_rows(c), theta0, dict(mean=mean, precision=P / S, kind=1, prior_loss=np.full(K, np.nan)), S=S, **lp.PRIOR_SCHEDULE)
    mdl = zoo.get("pendulum", "sysid")
    kind = dict(prior_kind="full") if K == p else {}          # (S = 3: K == p == 3, where the shape [3, 3] alone is refused)
    loop = BatchedLMLoop.for_sysid(mdl, c["inputs"], c["states"], theta0, samples_per_problem=S, prior_mean=mean, prior_precision=P, **kind, **lp.PRIOR_SCHEDULE)
    r = loop.run()
    tag = "BatchedLMLoop.for_sysid pendulum K=%d S=%d with a prior" % (K, S)
    print("%s: evaluations %s (restatement %s) rejected %s (%s) accepted %s (%s) states %s" % (tag, r["evaluations"].tolist(), ref["evaluations"].tolist(), r["rejected"].tolist(),
                                                                                            ref["rejected"].tolist(), r["accepted"].tolist(), ref["accepted"].tolist(), r["state"]))
    for key in ("evaluations", "rejected", "accepted"):
        assert np.array_equal(r[key], ref[key]), key
    assert r["state"] == [lb.NAMES[s] for s in ref["state"]] and ref["rejected"].max() >= 1
    worst = max(float((np.abs(r["loss_trace"][k] - ref["loss_trace"][k, :ref["accepted"][k]]) / ref["loss_trace"][k, :ref["accepted"][k]]).max()) for k in range(K))
    margins.check(tag + ": accepted losses vs the restatement on the oracle", worst, 1e-6)
    d = r["theta"] - mean
    margins.check(tag + ": prior_loss", np.abs(r["prior_loss"] - np.einsum("ki,ij,kj->k", d, P / S, d)).max() / np.abs(r["prior_loss"]).max(), 1e-12)
    with pytest.raises(ValueError, match="prior"):
        loop.covariance("estimated")
    cov = loop.covariance("known")
    sid = sg.oracle("pendulum")
    _, _, G = sg.reference_rows(sid, c["inputs"], c["states"], np.repeat(r["theta"], S, axis=0))
    for k in range(K):
        A = G[k * S:(k + 1) * S].sum(axis=0) + P
        want = np.linalg.inv(A)
        margins.check("%s problem %d: covariance('known') vs numpy on the oracle's rows" % (tag, k), np.abs(cov["cov"][k] - want).max() / np.abs(want).max(),
                      10 * np.linalg.cond(A) * 1e-10)
        assert cov["status"][k] == 0 and np.array_equal(cov["cov"][k], cov["cov"][k].T) and np.allclose(cov["std_err"][k], np.sqrt(np.diag(want)), rtol=1e-4, atol=0)
    assert (cov["sigma2"] == 1.0).all() and ((cov["pivot_ratio"] > 0) & (cov["pivot_ratio"] <= 1)).all()
    if S == 3:
        one = LMLoop.for_sysid(mdl, c["inputs"][:3], c["states"][:3], theta0[0], prior_mean=mean, prior_precision=P)
        o = one.run(max_evals=lp.PRIOR_SCHEDULE["max_evals"], loss_tol=lp.PRIOR_SCHEDULE["loss_tol"])
        assert (o["evaluations"], o["rejected"], o["iterations"]) == (r["evaluations"][0], r["rejected"][0], r["accepted"][0])
        margins.check(tag + ": LMLoop.for_sysid on problem 0, accepted losses", float((np.abs(o["loss_trace"] - r["loss_trace"][0]) / o["loss_trace"]).max()), 1e-6)
        margins.check(tag + ": LMLoop.for_sysid on problem 0, prior_loss", abs(o["prior_loss"] - r["prior_loss"][0]) / r["prior_loss"][0], 1e-6)
        oc = one.covariance("known")
        margins.check(tag + ": LMLoop.covariance('known') vs the device's", np.abs(oc["cov"] - cov["cov"][0]).max() / np.abs(cov["cov"][0]).max(), 1e-6)
        assert one.n_observed == int(loop.n_observed[0].item()) == 3 * 20 * 2


def test_for_sysid_covariance_with_an_estimated_noise_level(margins):
    """pendulum K = 9, S = 1 on noisy states (sigma = 0.01, seeded), no prior, 12 evaluations: sigma^2 = loss / (N - p) with N = 40 (rows 1 .. 20 of two components; row 0
    is the rollout's own start) and Cov = sigma^2 G^-1 against numpy on the oracle's rows at the returned theta, within 10 cond 1e-10"""
    from pdp_amd import zoo
    from pdp_amd.irl import BatchedLMLoop
    c = lb.sysid_case("pendulum", 1)
    noisy = c["states"] + 0.01 * np.random.default_rng(6).standard_normal(c["states"].shape)
    loop = BatchedLMLoop.for_sysid(zoo.get("pendulum", "sysid"), c["inputs"], noisy, c["theta0"], max_evals=12)
    r = loop.run()
    assert npy(loop.n_observed).tolist() == [40] * 9
    cov = loop.covariance("estimated")
    loss, _, G = sg.reference_rows(sg.oracle("pendulum"), c["inputs"], noisy, r["theta"])
    p = r["theta"].shape[1]
    print("estimated noise level: sigma %s (0.01 was added), pivot_ratio %s" % (np.sqrt(cov["sigma2"]).round(5).tolist(), cov["pivot_ratio"]))
    for k in range(9):
        s2 = loss[k] / (40 - p)
        want = s2 * np.linalg.inv(G[k])
        margins.check("covariance('estimated') problem %d: sigma2" % k, abs(cov["sigma2"][k] - s2) / s2, 1e-9)
        margins.check("covariance('estimated') problem %d: cov" % k, np.abs(cov["cov"][k] - want).max() / np.abs(want).max(), 10 * np.linalg.cond(G[k]) * 1e-10)
        assert cov["status"][k] == 0
    few = loop.covariance("estimated", n_observed=np.array([40, 3, 2] + [40] * 6))
    assert np.isnan(few["cov"][1:3]).all() and np.isnan(few["sigma2"][1:3]).all() and np.array_equal(few["cov"][0], cov["cov"][0]) and np.array_equal(few["cov"][3:], cov["cov"][3:])
    with pytest.raises(ValueError, match="noise"):
        loop.covariance("guessed")


@pytest.mark.parametrize("K", [3, 5], ids=["K3", "K5_equals_W"])
def test_estimate_ini_with_a_prior_on_the_initial_state(margins, K):
    """cart-pole, components 0, 1 observed, components 2, 3 of x0 estimated from 0 with prior_ini_precision = (0.5, 2): the device loop against the restatement on the
    oracle's augmented rows with the diagonal prior [0 | prior_ini_precision] centred on [0 | the starting components]; a budget of 4 evaluations: up to there the
    accepted losses of the oracle schedule fall by more than 1e-6 relative (from the fifth accepted point of trajectory 1 on by 3e-10 and less, where rows that agree
    to 1e-10 no longer decide alike)"""
    import sysid_ini_common as si
    from pdp_amd import zoo
    from pdp_amd.irl import BatchedLMLoop
    c, sid = si.lm_data("cartpole"), sg.oracle("cartpole")
    pick = np.arange(K) % c["inputs"].shape[0]      # (K = 5: the three recordings and two of them again - as many problems as unknowns, W = p + q = 5)
    c = dict(c, **{k: c[k][pick] for k in ("inputs", "states", "ini_state", "x0_true")})
    idx, p = c["idx"], sid.p
    q = len(idx)
    assert K != 5 or K == p + q
    pi = np.array([0.5, 2.0])
    sch = dict(max_evals=4, loss_tol=0.0)

    def evaluate_rows(trial):
        ini = c["ini_state"].copy()
        ini[:, idx] = trial[:, p:]
        return si.packed(si.reference_rows(sid, c["inputs"], c["states"], trial[:, :p], idx, ini, True)), None
    theta0 = np.concatenate([np.repeat(c["theta_ref"][None], K, axis=0), c["ini_state"][:, idx]], axis=1)
    prior = dict(mean=np.concatenate([np.zeros((K, p)), c["ini_state"][:, idx]], axis=1), precision=np.tile(np.concatenate([np.zeros(p), pi]), (K, 1)), kind=0,
                 prior_loss=np.full(K, np.nan))
    ref = lp.run_prior(evaluate_rows, theta0, prior, S=1, **sch)
    loop = BatchedLMLoop.for_sysid(zoo.get("cartpole", "sysid"), c["inputs"], c["states"], c["theta_ref"], ini_state=c["ini_state"], skip_missing=True, estimate_ini=idx,
                                   prior_ini_precision=pi, **sch)
    r = loop.run()
    print("estimate_ini with a prior on x0: evaluations %s rejected %s accepted %s; x0[idx] %s (true %s)" % (r["evaluations"].tolist(), r["rejected"].tolist(), r["accepted"].tolist(),
                                                                                                       r["theta"][:, p:].round(4).tolist(), c["x0_true"][:, idx].round(4).tolist()))
    for key in ("evaluations", "rejected", "accepted"):
        assert np.array_equal(r[key], ref[key]), key
    worst = max(float((np.abs(r["loss_trace"][k] - ref["loss_trace"][k, :ref["accepted"][k]]) / ref["loss_trace"][k, :ref["accepted"][k]]).max()) for k in range(K))
    margins.check("estimate_ini with prior_ini_precision: accepted losses vs the restatement", worst, 1e-6)
    d = r["theta"][:, p:] - c["ini_state"][:, idx]
    margins.check("estimate_ini with prior_ini_precision: prior_loss", np.abs(r["prior_loss"] - (d * d * pi).sum(axis=1)).max() / np.abs(r["prior_loss"]).max(), 1e-12)
    T = c["inputs"].shape[1]
    assert npy(loop.n_observed).tolist() == [(T + 1) * 2] * K and q == 2          # rows 0 .. T of the two observed components (ini_state is given; the estimated ones are NaN in the data)
    with pytest.raises(ValueError, match="estimate_ini"):
        BatchedLMLoop.for_sysid(zoo.get("cartpole", "sysid"), c["inputs"], c["states"], c["theta_ref"], ini_state=c["ini_state"], skip_missing=True, prior_ini_precision=pi)


def test_for_irl_with_a_prior():
    """one IRL problem per stored pendulum demonstration (K = 5) with a diagonal prior: evaluations, rejected and accepted counts, and the state, against irl.LMLoop with
    the same prior on the oracle (re-solved OC problems, warm from the last accepted solution).  A budget of 4 evaluations: on the oracle the accepted losses fall by
    3e-3 relative and more up to the fourth point and by 4e-9 .. 1e-11 from the fifth on - below what solves converged to 1e-10 on two machines decide alike."""
    import oc_wls_common as ow
    from pdp_amd import zoo
    from pdp_amd.irl import BatchedLMLoop, LMLoop
    d, theta0 = tb._demos("pendulum")
    K, p, budget = 5, theta0.size, 4
    mean, prec = 1.1 * theta0, np.full(p, 0.5)
    loop = BatchedLMLoop.for_irl(zoo.get("pendulum", "irl"), d["state"], d["control"], theta0, max_evals=budget, prior_mean=mean, prior_precision=prec)
    r = loop.run()
    print("BatchedLMLoop.for_irl pendulum with a prior: evaluations %s rejected %s accepted %s states %s losses %s prior_loss %s"
          % (r["evaluations"].tolist(), r["rejected"].tolist(), r["accepted"].tolist(), r["state"], r["loss"], r["prior_loss"]))
    T, n, m = d["control"].shape[1], d["state"].shape[2], d["control"].shape[2]
    assert npy(loop.n_observed).tolist() == [T * n + T * m] * K
    for k in range(K):
        state = {"accepted": None, "trial": None}

        def evaluate(theta, k=k, state=state):
            loss, grad, G, sols = ow.oracle_rows("pendulum", d["state"][k:k + 1, 0], theta, d["state"][k:k + 1], d["control"][k:k + 1], warm=state["accepted"])
            state["trial"] = sols
            return loss[0], grad[0], G[0]
        one = LMLoop(evaluate, theta0, prior_mean=mean, prior_precision=prec)
        one.on_accept = lambda state=state: state.update(accepted=state["trial"])
        o = one.run(max_evals=budget)
        assert (o["evaluations"], o["rejected"], o["iterations"]) == (r["evaluations"][k], r["rejected"][k], r["accepted"][k]), k
        assert r["state"][k] == ("BUDGET" if o["evaluations"] >= budget else "STALLED" if o["stalled"] else "CONVERGED")
        assert abs(o["loss_trace"][-1] - r["loss"][k]) <= 1e-6 * o["loss_trace"][-1] and abs(o["prior_loss"] - r["prior_loss"][k]) <= 1e-6 * o["prior_loss"]
    cov = loop.covariance("known")
    assert (cov["status"] == 0).all() and np.isfinite(cov["std_err"]).all()


def test_example_with_a_prior_and_covariance():
    """examples/sysid_pdp.py --method lm --per-trajectory --prior-sigma 0.5 --covariance: per problem a line with theta +- std_err and the pivot ratio"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "sysid_pdp.py"), "--system", "pendulum", "--method", "lm", "--per-trajectory", "--prior-sigma", "0.5",
                        "--covariance"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("problem")]
    assert len([ln for ln in lines if "evaluations" in ln]) == 3, r.stdout[-3000:]
    err = [ln for ln in lines if "+-" in ln and "pivot_ratio" in ln]
    assert len(err) == 3, r.stdout[-3000:]
    assert len([ln for ln in r.stdout.splitlines() if ln.startswith("done:")]) == 1


def test_per_problem_diagonal_where_K_equals_p(margins):
    """pendulum K = 3, S = 3, p = 3: a diagonal precision per problem, [K, p] = [3, 3], with prior_kind="diagonal" - against the restatement on the oracle (which is told
    the kind); without prior_kind the shape is refused; read as a full matrix it is not even symmetric"""
    from pdp_amd import zoo
    from pdp_amd.irl import BatchedLMLoop
    c = lb.sysid_case("pendulum", 3)
    K, S = c["K"], 3
    assert K == c["theta0"].shape[1] == 3
    mean = lp.pendulum_prior(c)[0]
    prec = np.array([[30.0, 3.0, 0.3], [0.0, 60.0, 6.0], [9.0, 0.9, 90.0]])
    theta0 = lp.prior_starts(c)
    mdl = zoo.get("pendulum", "sysid")
    with pytest.raises(ValueError, match="prior_kind"):
        BatchedLMLoop.for_sysid(mdl, c["inputs"], c["states"], theta0, samples_per_problem=S, prior_mean=mean, prior_precision=prec)
    with pytest.raises(ValueError, match="symmetric"):
        BatchedLMLoop.for_sysid(mdl, c["inputs"], c["states"], theta0, samples_per_problem=S, prior_mean=mean, prior_precision=prec, prior_kind="full")
    ref = lp.run_prior(lb.oracle_rows(c), theta0, dict(mean=mean, precision=prec / S, kind=0, prior_loss=np.full(K, np.nan)), S=S, **lp.PRIOR_SCHEDULE)
    r = BatchedLMLoop.for_sysid(mdl, c["inputs"], c["states"], theta0, samples_per_problem=S, prior_mean=mean, prior_precision=prec, prior_kind="diagonal",
                                **lp.PRIOR_SCHEDULE).run()
    for key in ("evaluations", "rejected", "accepted"):
        assert np.array_equal(r[key], ref[key]), key
    worst = max(float((np.abs(r["loss_trace"][k] - ref["loss_trace"][k, :ref["accepted"][k]]) / ref["loss_trace"][k, :ref["accepted"][k]]).max()) for k in range(K))
    margins.check("per-problem diagonal at K == p: accepted losses vs the restatement", worst, 1e-6)
    d = r["theta"] - mean
    margins.check("per-problem diagonal at K == p: prior_loss", np.abs(r["prior_loss"] - (d * d * prec / S).sum(axis=1)).max() / np.abs(r["prior_loss"]).max(), 1e-12)


def test_a_non_finite_prior_makes_the_trial_unusable(margins):
    """the kernel's "unusable" test covers the augmented values: K = 5, p = 3, finite rows; a NaN in the precision of problem 1 and an inf in the mean of problem 3 from
    the start (FAILED at START), a NaN written into the precision of problem 2 after the first launch (its trials are rejected from then on, current stays)"""
    import torch
    K, S, p = 5, 1, 3
    rng = np.random.default_rng(12)
    theta0 = rng.standard_normal((K, p))
    for variant in ("diagonal per problem", "full per problem"):
        prior = make_prior(K, p, theta0, variant, seed=9)
        prior["precision"][1].flat[-1] = np.nan
        prior["mean"][3, 0] = np.inf
        st = lb.new_state(theta0, S, trace_len=3)
        dv = PriorDevice(st, prior)
        for n in range(3):
            rows = lb.script_rows(K, S, p, 4, seed=20 + n)[0]
            rows[:, p] = 5.0 - n                    # (finite rows with a falling loss: without the prior's trouble every trial would be accepted)
            if n == 1:
                prior["precision"][2].flat[0] = np.nan
                dv.precision[1][2].view(-1)[0] = float("nan")
            dv.update(torch.as_tensor(rows, device="cuda"), None, max_evals=10)
            lp.launch_prior(st, rows, None, prior, max_evals=10)
            got = dv.host()
            tb.compare(margins, "non-finite prior, %s, launch %d" % (variant, n), got, st)
            dv.guards_untouched()
            st["trial"][:] = got["trial"]
        assert st["state"].tolist() == [lb.ACTIVE, lb.FAILED, lb.ACTIVE, lb.FAILED, lb.ACTIVE]
        assert st["rejected"].tolist() == [0, 0, 2, 0, 0] and st["accepted"].tolist() == [3, 0, 1, 0, 3]
        assert np.isnan(npy(dv.prior_loss[1])[[1, 3]]).all() and np.isfinite(npy(dv.prior_loss[1])[[0, 2, 4]]).all()


def test_irl_example_with_a_prior_and_covariance():
    """examples/irl_pdp.py --method lm --prior-sigma 0.5 --covariance on the pendulum (irl.LMLoop.for_irl with a prior, LMLoop.covariance): one line with theta +- std_err
    and the pivot ratio, a finite final loss"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "irl_pdp.py"), "--system", "pendulum", "--method", "lm", "--iters", "6", "--prior-sigma", "0.5",
                        "--covariance"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    err = [ln for ln in r.stdout.splitlines() if ln.startswith("theta ") and "+-" in ln and "pivot_ratio" in ln]
    assert len(err) == 1 and "noise known" in err[0] and "singular" not in err[0] and "nan" not in err[0].lower(), r.stdout[-3000:]
    done = [ln for ln in r.stdout.splitlines() if ln.startswith("done:")]
    assert len(done) == 1 and np.isfinite(float(done[0].split("final loss ")[1].split()[0])), r.stdout[-3000:]
