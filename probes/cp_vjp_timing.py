#!/usr/bin/env python3
"""What the ControlPlanning adjoint layer costs, B = 1024, T = 100, on the quadrotor (n = 13, m = 4): the tanh-MLP policy of the bench's C5b (hidden [13, 13],
p = 420) and a Lagrange policy (6 pivots, p = 24), same inputs for every variant:

    sweep              pdp_cp_step_batched with a pdp_policy_cot: cp_vjp_kernel on a given rollout - dL/dtheta and dL/dx_0, one launch
    rollout + sweep    pdp_cp_integrate_batched, then the sweep: what a forward + backward of pdp_amd.autograd.cp_trajectory launches
    step               pdp_cp_step_batched as ControlPlanning.step_batch calls it: the fused rollout + gradient of the one loss it serves
    rollout + mater.   the rollout, then ModelLib.cp_rollout_vjp(force_materialised=True): getAuxSys -> integrateAuxSys -> contraction through HBM - what a caller had
                       to do for another loss before the layer, and what the layer does beyond the sweep's limits (--launches / 10 calls per window: it is Python-level and slow)

HIP-event-bracketed windows of --launches back-to-back calls behind a warm-up, the variants alternating inside every round, --rounds rounds; reported per call:
median over the rounds, and their min .. max as the run-to-run spread.  The foreign calls of the first three are marshalled once.  No threshold: the figures are written
down beside the estimate made before the kernel was timed.

    python probes/cp_vjp_timing.py [--out profiles/cp_vjp_timing.txt]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ESTIMATE = ("estimate made before the first timing (DESIGN.md section 4.1o): MLP p = 420 - sweep 0.15 - 0.3 ms, rollout + sweep 0.3 - 0.5 ms = 1.5 - 2.5 x the fused step "
            "(0.21 ms), materialised 5 - 15 ms = 20 - 50 x the layer; Lagrange p = 24 - sweep 0.02 - 0.04 ms")


def measure(label, pol, p, theta_of, a, lines):
    import torch
    from pdp_amd import runtime as rt, zoo
    mdl = zoo.get("quadrotor", "oc")
    B, T, n, m = a.batch, a.horizon, mdl.n, mdl.m
    rng = np.random.default_rng(0)
    x0 = np.zeros((B, n))
    x0[:, :3] = rng.uniform(-2, 2, (B, 3))
    x0[:, 6] = 1
    f64 = dict(dtype=torch.float64, device="cuda")
    x0, th = rt.dev(x0), rt.dev(theta_of(rng))
    gx, gu = rt.dev(rng.standard_normal((B, T + 1, n))), rt.dev(rng.standard_normal((B, T, m)))
    x, u, cost = torch.empty((B, T + 1, n), **f64), torch.empty((B, T, m), **f64), torch.empty((B,), **f64)
    grad, gx0, loss, sgrad = torch.empty((B, p), **f64), torch.empty((B, n), **f64), torch.empty((B,), **f64), torch.empty((B, p), **f64)
    P, stream = rt.ptr, rt.current_stream_ptr()
    cot = rt.PdpPolicyCot()
    C.memmove(C.byref(cot.pol), C.byref(pol), C.sizeof(rt.PdpPolicy))
    cot.pol.kind = pol.kind | rt.PDP_POLICY_COTANGENT
    cot.x, cot.grad_x, cot.grad_u, cot.grad_x0 = x.data_ptr(), gx.data_ptr(), gu.data_ptr(), gx0.data_ptr()
    a_sweep = (B, T, C.cast(C.byref(cot), C.POINTER(rt.PdpPolicy)), p, None, P(th), 0, None, P(grad), None, None, None, 0, stream)
    a_roll = (B, T, C.byref(pol), p, P(x0), P(th), 0, P(x), P(u), P(cost), stream)
    nbytes = mdl.lib.pdp_cp_step_workspace_bytes(B, T, C.byref(pol), p)
    ws = torch.empty((max(nbytes, 8) // 8,), **f64)
    a_step = (B, T, C.byref(pol), p, P(x0), P(th), 0, P(loss), P(sgrad), None, None, P(ws) if nbytes else None, nbytes, stream)

    def rollout():
        rt.check(mdl.lib.pdp_cp_integrate_batched(*a_roll), "rollout")

    def sweep():
        rt.check(mdl.lib.pdp_cp_step_batched(*a_sweep), "sweep")

    def rollout_sweep():
        rollout()
        sweep()

    def step():
        rt.check(mdl.lib.pdp_cp_step_batched(*a_step), "step")

    def rollout_materialised():
        rollout()
        return mdl.cp_rollout_vjp(pol, p, x, th, gx, gu, force_materialised=True)
    variants = (("sweep", sweep, 1), ("rollout + sweep", rollout_sweep, 1), ("step", step, 1), ("rollout + mater.", rollout_materialised, 10))
    # results first: finite, and the sweep and the materialised route agree
    rollout_sweep()
    out = rollout_materialised()
    torch.cuda.synchronize()
    agree = float((out["grad_theta"] - grad).abs().max() / grad.abs().max())
    assert bool(torch.isfinite(grad).all()) and bool(torch.isfinite(gx0).all()) and agree < 1e-9, agree
    del out
    times = {k: [] for k, _, _ in variants}
    for r in range(a.rounds + 1):
        for k, f, div in variants:
            for _ in range(max(2, 20 // div)):                   # warm-up of this variant: code objects, allocator, clocks under load
                f()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(max(1, a.launches // div)):
                f()
            e1.record()
            e1.synchronize()
            if r > 0:                                            # round 0 is warm-up as a whole
                times[k].append(e0.elapsed_time(e1) / max(1, a.launches // div))
    lines.append("quadrotor n = %d m = %d, %s p = %d, B = %d, T = %d, %d pool rows in the sweep; sweep vs materialised route: %.1e of the largest entry"
                 % (n, m, label, p, B, T, mdl.cp_vjp_rows(), agree))
    for k, _, _ in variants:
        t = np.array(times[k])
        lines.append("  %-17s median %.4f ms   min %.4f   max %.4f   spread %.1f %%" % (k, np.median(t), t.min(), t.max(), 100 * (t.max() - t.min()) / np.median(t)))
    med = {k: float(np.median(times[k])) for k, _, _ in variants}
    lines.append("  rollout + sweep against the fused step: x %.2f;   the materialised route against rollout + sweep: x %.1f"
                 % (med["rollout + sweep"] / med["step"], med["rollout + mater."] / med["rollout + sweep"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--horizon", type=int, default=100)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from pdp_amd import runtime as rt
    lines = ["ControlPlanning adjoint layer: the sweep, rollout + sweep, the fused step, the materialised route; %s" % torch.cuda.get_device_name(0),
             "ms per call: HIP events around %d back-to-back calls (materialised: %d) behind a warm-up, variants alternating, %d rounds (median, min .. max = run-to-run spread)"
             % (a.launches, max(1, a.launches // 10), a.rounds), ESTIMATE]
    measure("tanh MLP [13, 13, 4] (C5b)", rt.make_policy("mlp", layers=[13, 13, 4]), 420, lambda rng: 0.1 * rng.standard_normal(420), a, lines)
    measure("Lagrange, 6 pivots", rt.make_policy("poly", pivots=np.linspace(0, a.horizon, 6)), 24, lambda rng: 2.5 + 0.05 * rng.standard_normal(24), a, lines)      # (around hover)
    txt = "\n".join(lines) + "\n"
    print(txt, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt)


if __name__ == "__main__":
    main()
