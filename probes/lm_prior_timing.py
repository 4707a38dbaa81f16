#!/usr/bin/env python3
"""What a Gaussian prior inside the batched Levenberg-Marquardt update, and one covariance launch, cost: the workload of probes/lm_batched_timing.py - quadrotor SysID,
K = 1024 problems of S = 1 trajectory, T = 100 (bench config C5a), p = 5.

    eval               the evaluation alone: pdp_sysid_step_gn_batched with per-sample parameters, one launch
    eval+update        the evaluation and pdp_lm_update_batched - the kernel without a prior, the same code object as before the prior variant existed
                       (profiles/lm_prior_code_object_diff.txt)
    eval+update_prior  the evaluation and pdp_lm_update_prior_batched with a full-matrix prior per problem (K p p + K p doubles more to read, p shuffles per lane more)
    covariance         one launch of pdp_lm_covariance_batched on the K current rows

Estimate written down before the run: the update is launch-bound (8.1 us); the prior adds K (p p + p) 8 = 246 KB of reads and about 3 p = 15
shuffles per lane in front of a loop that already runs 832 of them - well under a microsecond, inside the run-to-run spread.  The covariance launch reads the same 254 KB
as the update, runs one elimination over [A | I] (twice the row length of the update's [A | b]) and 16 back substitutions, no retry loop, and writes K p p + K p + K
doubles: of the update's order, 6 - 12 us.

The method of probes/lm_batched_timing.py: HIP-event-bracketed windows of --launches back-to-back calls behind a warm-up, the variants alternating inside every round,
--rounds rounds; reported per iteration: median over the rounds, and their min .. max as the run-to-run spread.  The foreign calls are marshalled once.  The state is
re-armed before every window, outside it, so that every launch of the update does the full work of an active problem: reduce, (add the prior,) decide, solve.

    python probes/lm_prior_timing.py [--out profiles/lm_prior_timing.txt]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=1024)
    ap.add_argument("--horizon", type=int, default=100)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from pdp_amd import runtime as rt, zoo
    from pdp_amd.irl import lm_step
    import time
    mdl = zoo.get("quadrotor", "sysid")
    K, T, n, m, p = a.problems, a.horizon, mdl.n, mdl.m, mdl.p
    w = p + 1 + p * p
    io = np.load(os.path.join(ROOT, "tests", "golden", "iodata_quadrotor.npz"))
    rng = np.random.default_rng(0)
    f64, i32 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.int32, device="cuda")
    x0 = rt.dev(io["states"][np.arange(K) % io["states"].shape[0], 0] * (1.0 + 0.05 * rng.standard_normal((K, n))))
    u = rt.dev(rng.uniform(-1.0, 1.0, (K, T, m)))
    xobs = mdl.sysid_integrate(x0, u, io["true_parameter"])                        # the data: rolled out at the true parameter
    theta0 = rt.dev(io["true_parameter"][None] * (1.0 + 0.05 * rng.standard_normal((K, p))))          # per-problem parameters
    loss, rows = torch.empty((K,), **f64), torch.empty((K, w), **f64)
    nbytes = int(mdl.lib.pdp_sysid_step_workspace_bytes(K, T))
    ws = torch.empty((max(nbytes, 8) // 8,), **f64)
    P, stream = rt.ptr, rt.current_stream_ptr()
    a_eval = (K, T, P(u), P(xobs), None, P(theta0), p, 0, P(loss), P(rows), P(ws) if nbytes else None, nbytes, stream)
    fn_eval = mdl.lib.pdp_sysid_step_gn_batched
    # the device state of the update
    st = dict(theta=theta0.clone(), trial=theta0.clone(), lam=torch.empty((K,), **f64), current=torch.empty((K, w), **f64), state=torch.empty((K,), **i32),
              evaluations=torch.zeros((K,), **i32), rejected=torch.zeros((K,), **i32), accepted=torch.zeros((K,), **i32), accepted_now=torch.zeros((K,), **i32),
              counters=torch.zeros((2,), dtype=torch.int64, device="cuda"))
    sch = rt.PdpLmSchedule(1.0, 10.0, 1e-12, 1e8, 0.0, 1 << 30)            # up = 1: a rejected trial leaves the damping, so no problem ever stalls inside a window
    cst = rt.PdpLmState(*[st[k].data_ptr() for k in ("theta", "trial", "lam", "current", "state", "evaluations", "rejected", "accepted", "accepted_now")], None, None, None, 0,
                        st["counters"].data_ptr())
    fn_update = rt.load_core().pdp_lm_update_batched
    a_update = (K, 1, p, P(rows), w, None, C.byref(sch), C.byref(cst), stream)
    # a full-matrix prior per problem, of the size of a hundredth of G, centred 5 per cent off the start; the covariance outputs
    M = rng.standard_normal((K, p, p))
    prec, mean, prior_loss = rt.dev(M @ M.transpose(0, 2, 1)), rt.dev(theta0.cpu().numpy() * 1.05), torch.zeros((K,), **f64)
    prior = rt.PdpLmPrior(mean.data_ptr(), prec.data_ptr(), 1, p, p * p, prior_loss.data_ptr())
    fn_prior = rt.load_core().pdp_lm_update_prior_batched
    a_prior = a_update[:-1] + (C.byref(prior), stream)
    cov, std, ratio, status = torch.empty((K, p, p), **f64), torch.empty((K, p), **f64), torch.empty((K,), **f64), torch.empty((K,), **i32)
    fn_cov = rt.load_core().pdp_lm_covariance_batched
    a_cov = (K, p, P(st["current"]), w, None, P(cov), P(std), P(ratio), P(status), stream)
    rt.check(fn_eval(*a_eval), "eval")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(rows).all())
    first = rows.clone()

    def arm():
        """every problem ACTIVE at theta0 with a current row whose loss is far above the rows' (with or without the prior's share): the first launch of a window accepts, every later one meets an equal loss,
        rejects and solves again (up = 1) - each launch reduces, decides and solves for all K problems"""
        st["theta"].copy_(theta0); st["trial"].copy_(theta0); st["lam"].fill_(1e-3); st["current"].copy_(first); st["current"][:, p] *= 1e6
        st["state"].fill_(1); st["counters"].copy_(torch.tensor([0, K], device="cuda"))
        for k in ("evaluations", "rejected", "accepted"):
            st[k].zero_()
    def eval_update():
        rt.check(fn_eval(*a_eval), "eval")
        rt.check(fn_update(*a_update), "update")

    def eval_update_prior():
        rt.check(fn_eval(*a_eval), "eval")
        rt.check(fn_prior(*a_prior), "update with a prior")
    variants = (("eval", lambda: rt.check(fn_eval(*a_eval), "eval"), a.launches), ("eval+update", eval_update, a.launches), ("eval+update_prior", eval_update_prior, a.launches),
                ("covariance", lambda: rt.check(fn_cov(*a_cov), "covariance"), a.launches))
    # the update's result first: one launch on the armed state against irl.lm_step on the host
    arm()
    eval_update()
    torch.cuda.synchronize()
    c = st["current"].cpu().numpy()
    want = np.stack([theta0.cpu().numpy()[k] - lm_step(c[k, :p], c[k, p + 1:].reshape(p, p), 1e-4) for k in range(K)])
    dev = float(np.abs(st["trial"].cpu().numpy() - want).max() / np.abs(want).max())
    assert int(st["accepted"].sum()) == K and int(st["state"].sum()) == K and dev <= 1e-10, dev
    # the prior's result: one launch on the armed state against numpy; the covariance of the rows it left against numpy.linalg.inv
    arm()
    eval_update_prior()
    rt.check(fn_cov(*a_cov), "covariance")
    torch.cuda.synchronize()
    c2, th, mu, Pm = st["current"].cpu().numpy(), theta0.cpu().numpy(), mean.cpu().numpy(), prec.cpu().numpy()
    d = th - mu
    want = c[:, p] + np.einsum("ki,kij,kj->k", d, Pm, d)
    dev_prior = float(np.abs(c2[:, p] - want).max() / np.abs(want).max())
    inv = np.linalg.inv(c2[:, p + 1:].reshape(K, p, p))
    dev_cov = float((np.abs(cov.cpu().numpy() - inv).max(axis=(1, 2)) / np.abs(inv).max(axis=(1, 2))).max())
    assert int(st["accepted"].sum()) == K and dev_prior <= 1e-12 and int(status.sum()) == 0, (dev_prior, int(status.sum()))
    times = {k: [] for k, _, _ in variants}
    for r in range(a.rounds + 1):
        for k, f, count in variants:
            arm()
            for _ in range(20):                                  # warm-up of this variant: code objects, allocator, clocks under load
                f()
            arm()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(count):
                f()
            e1.record()
            e1.synchronize()
            if r > 0:                                            # round 0 is warm-up as a whole
                times[k].append(e0.elapsed_time(e1) / count)
    still = int(st["counters"][1].item())
    lines = ["Batched Levenberg-Marquardt with a prior, quadrotor SysID n = %d m = %d p = %d, K = %d problems of S = 1 trajectory, T = %d; %s, %s"
             % (n, m, p, K, T, torch.cuda.get_device_name(0), time.strftime("%Y-%m-%d")),
             "ms per iteration: HIP events around %d back-to-back iterations behind a warm-up, variants alternating, %d rounds (median, min .. max = run-to-run spread)"
             % (a.launches, a.rounds),
             "estimate before the run: the prior adds %d KB of reads and about 15 shuffles per lane to a launch-bound 8 us kernel - well under a microsecond; the covariance "
             "launch is of the update's order, 6 - 12 us" % (K * (p * p + p) * 8 // 1000),
             "augmented loss of the first launch vs numpy: largest deviation %.2e relative; covariance vs numpy.linalg.inv of the device's G (cond up to %.1e): %.2e of the "
             "largest entry; problems still active after the last window: %d of %d" % (dev_prior, float(np.linalg.cond(c2[:, p + 1:].reshape(K, p, p)).max()), dev_cov, still, K)]
    for k, _, _ in variants:
        t = np.array(times[k])
        lines.append("  %-18s median %.4f ms   min %.4f   max %.4f   spread %.1f %%" % (k, np.median(t), t.min(), t.max(), 100 * (t.max() - t.min()) / np.median(t)))
    med = {k: float(np.median(times[k])) for k, _, _ in variants}
    lines.append("  update = eval+update - eval = %.4f ms   update with a prior = eval+update_prior - eval = %.4f ms   the prior = %+.4f ms   covariance = %.4f ms"
                 % (med["eval+update"] - med["eval"], med["eval+update_prior"] - med["eval"], med["eval+update_prior"] - med["eval+update"], med["covariance"]))
    txt = "\n".join(lines) + "\n"
    print(txt, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt)


if __name__ == "__main__":
    main()
