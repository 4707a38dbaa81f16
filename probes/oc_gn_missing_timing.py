#!/usr/bin/env python3
"""What the mask of PDP_GRAD_SKIP_MISSING costs the fused unit, quadrotor B = 1024, T = 50 (the benchmark shape), same inputs:

    default          the fused unit as it is (what bench.py times): loss and gradient               } instantiations that exist without the flag: the yardsticks
    gauss_newton     PDP_GRAD_GAUSS_NEWTON: the packed row gradient | loss | G                      } of this run (their code objects are unchanged)
    gn_skip_full     PDP_GRAD_GAUSS_NEWTON | PDP_GRAD_SKIP_MISSING on the same, NaN-free demonstrations: the compare and the selects, nothing selected away
    gn_skip_half     the same with about half of all demonstration entries NaN (fixed seed; all of demo_x[:, 0] among them)

HIP-event-bracketed windows of --launches back-to-back calls behind a warm-up, the variants alternating inside every round, --rounds rounds; reported per call: median
over the rounds, and their min .. max as the run-to-run spread.  Foreign calls are marshalled once (no Python wrapper inside the window).

    python probes/oc_gn_missing_timing.py [--out profiles/oc_gn_missing_timing.txt]
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
    wx, wu = torch.as_tensor(rng.random((B, T + 1, n)) < 0.5, device="cuda"), torch.as_tensor(rng.random((B, T, m)) < 0.5, device="cuda")                             # True = observed
    wx[:, 0] = False
    nan = torch.full((), float("nan"), **f64)
    gxh, guh = torch.where(wx, gx, nan), torch.where(wu, gu, nan)
    row, row_s = torch.empty((B, p + 1 + p * p), **f64), torch.empty((B, p + 1 + p * p), **f64)
    x, lam, loss, grad, status = torch.empty((B, T + 1, n), **f64), torch.empty((B, T, n), **f64), torch.empty((B,), **f64), torch.empty((B, p), **f64), \
        torch.empty((B,), dtype=torch.int32, device="cuda")
    dxdp, dudp = torch.empty((B, T + 1, n, p), **f64), torch.empty((B, T, m, p), **f64)
    nbytes = mdl.lib.pdp_oc_pdp_workspace_bytes(B, T)
    ws = torch.empty((max(nbytes, 8) // 8,), **f64)
    P, fn, stream = rt.ptr, mdl.lib.pdp_oc_pdp_grad_batched, rt.current_stream_ptr()

    def args(flags, grad_t, dx, du, sx=None, su=None):
        return (B, T, flags, P(x0), P(u), P(th), 0, P(dx), P(du), P(x), P(lam), P(loss), P(grad_t), P(sx), P(su), P(status), P(ws), nbytes, stream)
    calls = {"default": args(0, grad, gx, gu), "gauss_newton": args(16, row, gx, gu), "gn_skip_full": args(16 | 32, row_s, gx, gu), "gn_skip_half": args(16 | 32, row_s, gxh, guh)}
    variants = [(k, (lambda c=c, k=k: rt.check(fn(*c), k))) for k, c in calls.items()]
    run = dict(variants)
    # results first.  NaN-free demonstrations: the masked instantiation computes what the Gauss-Newton one does; half-masked: what the masked contraction of the
    # materialised sensitivities gives
    run["gauss_newton"]()
    run["gn_skip_full"]()
    torch.cuda.synchronize()
    scale = row.abs().amax(dim=1, keepdim=True)
    dev_full = float(((row_s - row).abs() / scale).max())
    rt.check(fn(*args(0, grad, gx, gu, dxdp, dudp)), "sens")
    run["gn_skip_half"]()
    torch.cuda.synchronize()
    zero = torch.zeros((), **f64)
    ex, eu = torch.where(wx, x - gx, zero), torch.where(wu, u - gu, zero)
    Xm, Um = torch.where(wx[..., None], dxdp, zero), torch.where(wu[..., None], dudp, zero)
    ref = torch.cat([torch.einsum("bti,btip->bp", ex, Xm) + torch.einsum("bti,btip->bp", eu, Um), ((ex ** 2).sum(dim=(1, 2)) + (eu ** 2).sum(dim=(1, 2)))[:, None],
                     (torch.einsum("btip,btiq->bpq", Xm, Xm) + torch.einsum("btip,btiq->bpq", Um, Um)).reshape(B, p * p)], dim=1)
    parts = ((0, p), (p, p + 1), (p + 1, p + 1 + p * p))
    dev_half = max(float(((row_s[:, i:j] - ref[:, i:j]).abs().amax(dim=1) / ref[:, i:j].abs().amax(dim=1)).max()) for i, j in parts)
    assert int(status.sum()) == 0 and dev_full <= 1e-10 and dev_half <= 1e-10 and bool(torch.isfinite(row_s).all()), (dev_full, dev_half)
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
    lines = ["OC gradient unit with missing observations (PDP_GRAD_SKIP_MISSING), quadrotor n = %d m = %d p = %d, B = %d, T = %d; %s" % (n, m, p, B, T, torch.cuda.get_device_name(0)),
             "ms per call: HIP events around %d back-to-back calls behind 20 warm-up calls, variants alternating, %d rounds (median, min .. max = run-to-run spread)"
             % (a.launches, a.rounds),
             "largest relative deviation (per sample, of the largest entry of gradient / loss / G): masked instantiation on NaN-free demonstrations vs the Gauss-Newton "
             "instantiation %.2e; on half-masked demonstrations (%.1f %% of the entries NaN) vs the masked contraction of the materialised sensitivities %.2e"
             % (dev_full, 100.0 * (1.0 - float((wx.sum() + wu.sum()) / (wx.numel() + wu.numel()))), dev_half)]
    for k, _ in variants:
        t = np.array(times[k])
        lines.append("  %-13s median %.4f ms   min %.4f   max %.4f   spread %.1f %%" % (k, np.median(t), t.min(), t.max(), 100 * (t.max() - t.min()) / np.median(t)))
    med = {k: float(np.median(times[k])) for k, _ in variants}
    lines.append("  gauss_newton / default = %.3f     gn_skip_full / gauss_newton = %.3f     gn_skip_half / gauss_newton = %.3f"
                 % (med["gauss_newton"] / med["default"], med["gn_skip_full"] / med["gauss_newton"], med["gn_skip_half"] / med["gauss_newton"]))
    txt = "\n".join(lines) + "\n"
    print(txt, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt)


if __name__ == "__main__":
    main()
