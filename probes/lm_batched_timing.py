#!/usr/bin/env python3
"""What one iteration of MANY Levenberg-Marquardt problems costs: quadrotor SysID, K = 1024 problems of S = 1 trajectory, T = 100 (bench config C5a), p = 5.

    eval          the evaluation alone: pdp_sysid_step_gn_batched with per-sample parameters, one launch (DESIGN section 4.1d measured 0.0715 ms with a shared parameter)
    eval+update   the evaluation and pdp_lm_update_batched (csrc/pdp_lm_kernels.h): accept / reject, damping, damped solve, next trial points, termination - on the device
    eval+host     the host alternative for the same iteration: the evaluation, the K rows copied to the host, K irl.lm_step calls in numpy with the accept / reject
                  bookkeeping, the trial points copied back

Estimate written down before the run: the update reads K (p + 1 + p p) 8 = 254 KB and runs 256 short wavefronts, so eval+update - eval is launch-bound: a few
microseconds, under 15 % of eval.

The method of probes/sysid_gn_timing.py: HIP-event-bracketed windows of --launches back-to-back calls behind a warm-up, the variants alternating inside every round,
--rounds rounds; reported per iteration: median over the rounds, and their min .. max as the run-to-run spread.  The foreign calls of the first two variants are
marshalled once.  The state is re-armed (all problems ACTIVE, lam as at the start) before every window, outside it; the rows do not depend on the trial points inside a
window (the evaluation reads a fixed parameter tensor), so that every launch of the update does the full work of an active problem: reduce, decide, solve.

    python probes/lm_batched_timing.py [--out profiles/lm_batched_timing.txt]
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
    rt.check(fn_eval(*a_eval), "eval")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(rows).all())
    first = rows.clone()

    def arm():
        """every problem ACTIVE at theta0 with a current row whose loss is above the rows': the first launch of a window accepts, every later one meets an equal loss,
        rejects and solves again (up = 1) - each launch reduces, decides and solves for all K problems"""
        st["theta"].copy_(theta0); st["trial"].copy_(theta0); st["lam"].fill_(1e-3); st["current"].copy_(first); st["current"][:, p] *= 2.0
        st["state"].fill_(1); st["counters"].copy_(torch.tensor([0, K], device="cuda"))
        for k in ("evaluations", "rejected", "accepted"):
            st[k].zero_()
    host = dict(theta=theta0.cpu().numpy().copy(), lam=np.full(K, 1e-3), cur=first.cpu().numpy().copy())
    trial_dev = theta0.clone()

    def eval_host():
        rt.check(fn_eval(*a_eval), "eval")
        r = rows.cpu().numpy()                                   # (synchronises)
        trial = np.empty((K, p))
        for k in range(K):
            if np.isfinite(r[k]).all() and r[k, p] < host["cur"][k, p]:
                host["cur"][k], host["lam"][k] = r[k], max(host["lam"][k] / 10.0, 1e-12)
            else:
                host["lam"][k] = min(host["lam"][k] * 10.0, 1e8)
            c = host["cur"][k]
            trial[k] = host["theta"][k] - lm_step(c[:p], c[p + 1:].reshape(p, p), host["lam"][k])
        trial_dev.copy_(torch.as_tensor(trial), non_blocking=False)

    def eval_update():
        rt.check(fn_eval(*a_eval), "eval")
        rt.check(fn_update(*a_update), "update")
    variants = (("eval", lambda: rt.check(fn_eval(*a_eval), "eval"), a.launches), ("eval+update", eval_update, a.launches), ("eval+host", eval_host, max(1, a.launches // 10)))
    # the update's result first: one launch on the armed state against irl.lm_step on the host
    arm()
    eval_update()
    torch.cuda.synchronize()
    c = st["current"].cpu().numpy()
    want = np.stack([theta0.cpu().numpy()[k] - lm_step(c[k, :p], c[k, p + 1:].reshape(p, p), 1e-4) for k in range(K)])
    dev = float(np.abs(st["trial"].cpu().numpy() - want).max() / np.abs(want).max())
    assert int(st["accepted"].sum()) == K and int(st["state"].sum()) == K and dev <= 1e-10, dev
    times = {k: [] for k, _, _ in variants}
    for r in range(a.rounds + 1):
        for k, f, count in variants:
            arm()
            for _ in range(20 if count == a.launches else 2):    # warm-up of this variant: code objects, allocator, clocks under load
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
    lines = ["Batched Levenberg-Marquardt, quadrotor SysID n = %d m = %d p = %d, K = %d problems of S = 1 trajectory, T = %d; %s" % (n, m, p, K, T, torch.cuda.get_device_name(0)),
             "ms per iteration: HIP events around %d back-to-back iterations (eval+host: %d) behind a warm-up, variants alternating, %d rounds (median, min .. max = run-to-run "
             "spread)" % (a.launches, max(1, a.launches // 10), a.rounds),
             "estimate before the run: the update reads %d KB and runs %d short wavefronts - launch-bound, a few microseconds, under 15 %% of eval" % (K * w * 8 // 1000, (K + 3) // 4),
             "first trial points of the update vs irl.lm_step on the host: largest deviation %.2e of the largest entry; problems still active after the last window: %d of %d"
             % (dev, still, K)]
    for k, _, _ in variants:
        t = np.array(times[k])
        lines.append("  %-12s median %.4f ms   min %.4f   max %.4f   spread %.1f %%" % (k, np.median(t), t.min(), t.max(), 100 * (t.max() - t.min()) / np.median(t)))
    med = {k: float(np.median(times[k])) for k, _, _ in variants}
    lines.append("  update = eval+update - eval = %.4f ms = %.1f %% of eval   eval+host / eval+update = %.1f"
                 % (med["eval+update"] - med["eval"], 100 * (med["eval+update"] - med["eval"]) / med["eval"], med["eval+host"] / med["eval+update"]))
    txt = "\n".join(lines) + "\n"
    print(txt, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt)


if __name__ == "__main__":
    main()
