#!/usr/bin/env python3
"""What the ControlPlanning rollout's Jacobian-vector product costs, B = 1024, T = 100, on the quadrotor (n = 13, m = 4): the tanh-MLP policy of the bench's C5b (hidden
[13, 13], p = 420) and a Lagrange policy (6 pivots, p = 24), on a rollout that is already there, same inputs for every variant:

    tangent sweep      pdp_cp_step_batched with a pdp_policy_tan: cp_jvp_kernel - d_state and d_control along (d_theta, d_x0), one launch
    adjoint sweep      pdp_cp_step_batched with a pdp_policy_cot: the unchanged cp_vjp_kernel - dL/dtheta (the yardstick: the code object it was)
    gn product         one Gauss-Newton product of the states-only residual: the tangent sweep with d_theta alone and no d_control, then the adjoint sweep on its output
    one column mater.  ModelLib.cp_rollout_jvp(force_materialised=True): getAuxSys -> dUe @ d_theta -> integrateAuxSys on one column through HBM - what the layer does
                       beyond the sweep's limits (--launches / 10 calls per window: it is Python-level and slow)

HIP-event-bracketed windows of --launches back-to-back calls behind a warm-up, the variants alternating inside every round, --rounds rounds; reported per call:
median over the rounds, and their min .. max as the run-to-run spread.  The foreign calls of the first three are marshalled once.  No threshold: the figures are written
down beside the estimate made before the kernel was timed, and the ratio to the adjoint sweep of the same run whichever way it falls.

    python probes/cp_jvp_timing.py [--out profiles/cp_jvp_timing.txt]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ESTIMATE = ("estimate made before the first timing (DESIGN.md section 4.1p): MLP p = 420 - tangent sweep 0.2 - 0.3 ms = 0.45 - 0.65 of the adjoint sweep (0.476 ms), "
            "gn product 0.65 - 0.8 ms, one column materialised 1.5 - 4 ms; Lagrange p = 24 - tangent sweep 0.04 - 0.07 ms = 0.45 - 0.8 of the adjoint sweep (0.091 ms), "
            "gn product 0.13 - 0.16 ms, one column materialised 0.2 - 0.5 ms")


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
    dth, dx0 = rt.dev(rng.standard_normal(p)), rt.dev(rng.standard_normal((B, n)))
    x, u, _ = mdl.cp_integrate_T(pol, p, x0, th, T)
    dx, du, dx2, grad, grad2, zu = (torch.empty((B, T + 1, n), **f64), torch.empty((B, T, m), **f64), torch.empty((B, T + 1, n), **f64), torch.empty((B, p), **f64),
                                    torch.empty((B, p), **f64), torch.zeros((B, T, m), **f64))
    P, stream = rt.ptr, rt.current_stream_ptr()

    def tan_of(d_x0, d_x, d_u):
        tan = rt.PdpPolicyTan()
        C.memmove(C.byref(tan.pol), C.byref(pol), C.sizeof(rt.PdpPolicy))
        tan.pol.kind = pol.kind | rt.PDP_POLICY_TANGENT
        tan.x, tan.u, tan.d_theta, tan.d_theta_bstride, tan.d_x = x.data_ptr(), u.data_ptr(), dth.data_ptr(), 0, d_x.data_ptr()
        tan.d_x0, tan.d_u = (None if d_x0 is None else d_x0.data_ptr()), (None if d_u is None else d_u.data_ptr())
        return tan

    def cot_of(g_x, g_u):
        cot = rt.PdpPolicyCot()
        C.memmove(C.byref(cot.pol), C.byref(pol), C.sizeof(rt.PdpPolicy))
        cot.pol.kind = pol.kind | rt.PDP_POLICY_COTANGENT
        cot.x, cot.grad_x, cot.grad_u, cot.grad_x0 = x.data_ptr(), g_x.data_ptr(), g_u.data_ptr(), None
        return cot
    structs = [tan_of(dx0, dx, du), cot_of(gx, gu), tan_of(None, dx2, None), cot_of(dx2, zu)]
    head = lambda s: (B, T, C.cast(C.byref(s), C.POINTER(rt.PdpPolicy)), p, None, P(th), 0, None)
    a_tan, a_cot = head(structs[0]) + (None, None, None, None, 0, stream), head(structs[1]) + (P(grad), None, None, None, 0, stream)
    a_gn1, a_gn2 = head(structs[2]) + (None, None, None, None, 0, stream), head(structs[3]) + (P(grad2), None, None, None, 0, stream)

    def tangent():
        rt.check(mdl.lib.pdp_cp_step_batched(*a_tan), "tangent sweep")

    def adjoint():
        rt.check(mdl.lib.pdp_cp_step_batched(*a_cot), "adjoint sweep")

    def gn():
        rt.check(mdl.lib.pdp_cp_step_batched(*a_gn1), "tangent sweep")
        rt.check(mdl.lib.pdp_cp_step_batched(*a_gn2), "adjoint sweep")

    def materialised():
        return mdl.cp_rollout_jvp(pol, p, x, u, th, d_theta=dth, d_x0=dx0, force_materialised=True)
    variants = (("tangent sweep", tangent, 1), ("adjoint sweep", adjoint, 1), ("gn product", gn, 1), ("one column mater.", materialised, 10))
    # results first: finite, and the sweep and the materialised route agree
    tangent(), adjoint(), gn()
    out = materialised()
    torch.cuda.synchronize()
    agree = max(float((out["d_state"] - dx).abs().max() / dx.abs().max()), float((out["d_control"] - du).abs().max() / du.abs().max()))
    assert all(bool(torch.isfinite(t).all()) for t in (dx, du, dx2, grad, grad2)) and agree < 1e-9, agree
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
    lines.append("quadrotor n = %d m = %d, %s p = %d, B = %d, T = %d, pool rows: tangent sweep %d, adjoint sweep %d; sweep vs materialised route: %.1e of the largest entry"
                 % (n, m, label, p, B, T, mdl.cp_jvp_rows(), mdl.cp_vjp_rows(), agree))
    for k, _, _ in variants:
        t = np.array(times[k])
        lines.append("  %-17s median %.4f ms   min %.4f   max %.4f   spread %.1f %%" % (k, np.median(t), t.min(), t.max(), 100 * (t.max() - t.min()) / np.median(t)))
    med = {k: float(np.median(times[k])) for k, _, _ in variants}
    lines.append("  tangent sweep / adjoint sweep = %.3f;   gn product / adjoint sweep = %.2f;   one column materialised / tangent sweep = x %.1f"
                 % (med["tangent sweep"] / med["adjoint sweep"], med["gn product"] / med["adjoint sweep"], med["one column mater."] / med["tangent sweep"]))


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
    lines = ["ControlPlanning rollout: the tangent sweep (jvp) beside the adjoint sweep (vjp), a Gauss-Newton product, the one-column materialised route; %s"
             % torch.cuda.get_device_name(0),
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
