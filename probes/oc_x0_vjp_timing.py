#!/usr/bin/env python3
"""What the gradient with respect to the initial state costs on top of the cotangent-mode call, quadrotor and cart-pole, B = 1024, T = 50, same inputs:

    plain       pdp_oc_pdp_grad_batched with PDP_OC_COTANGENT: dL/dtheta, one launch (the fused unit)
    with x0     pdp_oc_pdp_grad_sens_batched with PDP_OC_COTANGENT and pdp_oc_sens_out.grad_x0: the same launch and, behind it on the same stream, the adjoint sweep
                oc_x0_vjp_kernel - dL/dtheta and dL/dx_0

HIP-event-bracketed windows of --launches back-to-back calls behind a warm-up, the two variants alternating inside every round, --rounds rounds; reported per call:
median over the rounds, and their min .. max as the run-to-run spread.  Foreign calls are marshalled once (no Python wrapper inside the window).  No threshold: the
figures are written down beside the estimate made before the kernel existed.

    python probes/oc_x0_vjp_timing.py [--out profiles/oc_x0_vjp_timing.txt]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ESTIMATE = "estimate made beforehand, from the SysID adjoint sweep's 0.040 ms at T = 100: 0.02 - 0.03 ms on top of the launch (a guess)"


def measure(system, theta, a, lines):
    import torch
    from pdp_amd import runtime as rt, zoo
    mdl = zoo.get(system, "irl")
    B, T, n, m, p = a.batch, a.horizon, mdl.n, mdl.m, mdl.p
    rng = np.random.default_rng(0)
    x0 = np.zeros((B, n))
    if system == "quadrotor":
        x0[:, 0:3] = rng.uniform(-2, 2, (B, 3))
        x0[:, 6] = 1.0
        u = 2.5 + 0.05 * rng.standard_normal((B, T, m))
    else:
        x0 = 0.1 * rng.standard_normal((B, n))
        u = 0.1 * rng.standard_normal((B, T, m))
    f64 = dict(dtype=torch.float64, device="cuda")
    x0, u, th = rt.dev(x0), rt.dev(u), rt.dev(np.asarray(theta, dtype=float))
    gx, gu = rt.dev(rng.standard_normal((B, T + 1, n))), rt.dev(rng.standard_normal((B, T, m)))
    x, lam, grad, gx0 = torch.empty((B, T + 1, n), **f64), torch.empty((B, T, n), **f64), torch.empty((B, p), **f64), torch.empty((B, n), **f64)
    status = torch.empty((B,), dtype=torch.int32, device="cuda")
    nbytes = mdl.lib.pdp_oc_pdp_workspace_bytes(B, T)
    ws = torch.empty((max(nbytes, 8) // 8,), **f64)
    P, stream = rt.ptr, rt.current_stream_ptr()
    so = rt.PdpOcSensOut(None, None, None, None, gx0.data_ptr())
    a_plain = (B, T, 8, P(x0), P(u), P(th), 0, P(gx), P(gu), P(x), P(lam), P(None), P(grad), P(None), P(None), P(status), P(ws), nbytes, stream)
    a_x0 = (B, T, 8, P(x0), P(u), P(th), 0, P(gx), P(gu), P(x), P(lam), P(None), P(grad), C.byref(so), P(status), P(ws), nbytes, stream)

    def plain():
        rt.check(mdl.lib.pdp_oc_pdp_grad_batched(*a_plain), "plain")

    def with_x0():
        rt.check(mdl.lib.pdp_oc_pdp_grad_sens_batched(*a_x0), "with x0")
    variants = (("plain", plain), ("with x0", with_x0))
    # results first: the same theta gradient to the bit, a finite grad_x0
    plain()
    g0 = grad.clone()
    with_x0()
    torch.cuda.synchronize()
    assert torch.equal(g0, grad) and int(status.sum()) == 0 and bool(torch.isfinite(gx0).all())
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
    lines.append("%s n = %d m = %d p = %d, B = %d, T = %d, %d pool rows in the sweep" % (system, n, m, p, B, T, mdl.oc_x0_vjp_rows()))
    for k, _ in variants:
        t = np.array(times[k])
        lines.append("  %-8s median %.4f ms   min %.4f   max %.4f   spread %.1f %%" % (k, np.median(t), t.min(), t.max(), 100 * (t.max() - t.min()) / np.median(t)))
    med = {k: float(np.median(times[k])) for k, _ in variants}
    lines.append("  grad_x0 on top of the launch: %.4f ms (x %.3f)" % (med["with x0"] - med["plain"], med["with x0"] / med["plain"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--horizon", type=int, default=50)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    lines = ["OC cotangent-mode call without and with pdp_oc_sens_out.grad_x0; %s" % torch.cuda.get_device_name(0),
             "ms per call: HIP events around %d back-to-back calls behind 20 warm-up calls, variants alternating, %d rounds (median, min .. max = run-to-run spread)"
             % (a.launches, a.rounds), ESTIMATE]
    measure("quadrotor", [1.0, 1.0, 1.0, 1.0, 0.4, 1.0, 1.0, 5.0, 1.0], a, lines)
    measure("cartpole", [0.5, 0.5, 1.0, 1.0, 6.0, 1.0, 1.0], a, lines)
    txt = "\n".join(lines) + "\n"
    print(txt, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt)


if __name__ == "__main__":
    main()
