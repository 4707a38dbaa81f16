#!/usr/bin/env python3
"""Gradient and Gauss-Newton matrix G = J'J of the demonstration loss, quadrotor B = 1024, T = 50 (the benchmark shape), same inputs:

    default      the fused unit as it is (what bench.py times): loss and gradient, one launch
    gauss_newton the fused unit with PDP_GRAD_GAUSS_NEWTON: the packed row gradient | loss | G, one launch
    materialise  what a caller had to do before the flag existed: the unit with dxdp / dudp written to HBM (63.6 MB of fp64 at this shape), then two torch.einsum and an add

HIP-event-bracketed windows of --launches back-to-back calls behind a warm-up, the three variants alternating inside every round, --rounds rounds; reported per
call: median over the rounds, and their min .. max as the run-to-run spread.  Foreign calls are marshalled once (no Python wrapper inside the window).

    python probes/oc_gn_timing.py [--out profiles/oc_gn_timing.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--horizon", type=int, default=50)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from pdp_amd import runtime as rt, zoo
    mdl = zoo.get("quadrotor", "irl")
    B, T, n, m, p = a.batch, a.horizon, mdl.n, mdl.m, mdl.p
    rng = np.random.default_rng(0)
    x0 = np.zeros((B, n))
    x0[:, 0:3] = rng.uniform(-2, 2, (B, 3))
    x0[:, 6] = 1.0
    f64 = dict(dtype=torch.float64, device="cuda")
    x0, u = rt.dev(x0), rt.dev(2.5 + 0.05 * rng.standard_normal((B, T, m)))
    th = rt.dev(np.array([1.0, 1.0, 1.0, 1.0, 0.4, 1.0, 1.0, 5.0, 1.0]))
    gx, gu = rt.dev(0.1 * rng.standard_normal((B, T + 1, n))), u + 0.1 * rt.dev(rng.standard_normal((B, T, m)))      # the demonstration
    row = torch.empty((B, p + 1 + p * p), **f64)
    x, lam, loss, grad, status = torch.empty((B, T + 1, n), **f64), torch.empty((B, T, n), **f64), torch.empty((B,), **f64), torch.empty((B, p), **f64), \
        torch.empty((B,), dtype=torch.int32, device="cuda")
    dxdp, dudp = torch.empty((B, T + 1, n, p), **f64), torch.empty((B, T, m, p), **f64)
    nbytes = mdl.lib.pdp_oc_pdp_workspace_bytes(B, T)
    ws = torch.empty((max(nbytes, 8) // 8,), **f64)
    P, fn, stream = rt.ptr, mdl.lib.pdp_oc_pdp_grad_batched, rt.current_stream_ptr()

    def args(flags, grad_t, dx, du):
        return (B, T, flags, P(x0), P(u), P(th), 0, P(gx), P(gu), P(x), P(lam), P(loss), P(grad_t), P(dx), P(du), P(status), P(ws), nbytes, stream)
    a_gn, a_def, a_sens = args(16, row, None, None), args(0, grad, None, None), args(0, grad, dxdp, dudp)

    def gn():
        rt.check(fn(*a_gn), "gauss_newton")

    def default():
        rt.check(fn(*a_def), "default")
    g_alt = [None]

    def materialise():
        rt.check(fn(*a_sens), "sens")
        g_alt[0] = torch.einsum("btip,btiq->bpq", dxdp, dxdp) + torch.einsum("btip,btiq->bpq", dudp, dudp)
    variants = (("default", default), ("gauss_newton", gn), ("materialise", materialise))
    # results first: the Gauss-Newton instantiation and the materialised alternative compute the same matrix, and the same gradient as the default unit
    gn()
    G = row[:, p + 1:].reshape(B, p, p).clone()
    materialise()
    torch.cuda.synchronize()
    dev_rel = float(((G - g_alt[0]).abs().amax(dim=(1, 2)) / g_alt[0].abs().amax(dim=(1, 2))).max())
    assert int(status.sum()) == 0 and dev_rel <= 1e-10 and torch.equal(row[:, :p], grad) and torch.equal(row[:, p], loss), dev_rel
    times = {k: [] for k, _ in variants}
    for r in range(a.rounds + 1):
        for k, f in variants:
            for _ in range(20):                                  # warm-up of this variant: code objects, allocator, clocks under load
                f()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                f()
            e1.record()
            e1.synchronize()
            if r > 0:                                            # round 0 is warm-up as a whole
                times[k].append(e0.elapsed_time(e1) / a.launches)
    lines = ["OC gradient unit with the Gauss-Newton matrix, quadrotor n = %d m = %d p = %d, B = %d, T = %d; %s" % (n, m, p, B, T, torch.cuda.get_device_name(0)),
             "ms per call: HIP events around %d back-to-back calls behind 20 warm-up calls, variants alternating, %d rounds (median, min .. max = run-to-run spread)"
             % (a.launches, a.rounds),
             "largest relative deviation of G, Gauss-Newton instantiation vs materialised alternative (per sample, of the largest entry): %.2e; gradient and loss bit-equal to the default unit's" % dev_rel]
    for k, _ in variants:
        t = np.array(times[k])
        lines.append("  %-12s median %.4f ms   min %.4f   max %.4f   spread %.1f %%" % (k, np.median(t), t.min(), t.max(), 100 * (t.max() - t.min()) / np.median(t)))
    med = {k: float(np.median(times[k])) for k, _ in variants}
    lines.append("  gauss_newton / default = %.3f     materialise / gauss_newton = %.2f" % (med["gauss_newton"] / med["default"], med["materialise"] / med["gauss_newton"]))
    lines.append("  sensitivity outputs the materialised alternative writes and re-reads: %.1f MB" % ((dxdp.numel() + dudp.numel()) * 8 / 1e6))
    txt = "\n".join(lines) + "\n"
    print(txt, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt)


if __name__ == "__main__":
    main()
