#!/usr/bin/env python3
"""What the SysID rollout's Jacobian-vector product costs: sysid_jvp_kernel (pdp_sysid_rollout_jvp_batched) beside the unchanged sysid_vjp_kernel
(pdp_sysid_rollout_vjp_batched) in the same run, B = 1024, T = 100, on a rollout that is already there:

    quadrotor (n = 13, m = 4, p = 5) and the linear model x+ = x + dt (A x + B u), theta = (vec A, vec B) (n = 9, m = 2, p = 99)
      vjp        pdp_sysid_rollout_vjp_batched: grad_theta and grad_x0 (the yardstick: the code object it was)
      jvp_theta  pdp_sysid_rollout_jvp_batched with d_theta alone (no `pathu`)
      jvp_all    pdp_sysid_rollout_jvp_batched with d_theta, d_x0 and d_u
      gn         one Gauss-Newton product of the recorded-state residual: jvp_theta, then vjp on its output (grad_theta alone)
      X@v        p = 99 only: the materialised route - pdp_sysid_auxsys_batched, pdp_sysid_aux_integrate_batched (X [B, T+1, n, p]), then X @ v in torch

No threshold is set in advance: nobody has measured this kernel.  Whatever comes out is written down beside the estimate.

The method of probes/sysid_vjp_timing.py: HIP-event-bracketed windows of --launches back-to-back calls behind a warm-up, the variants alternating inside every round,
--rounds rounds; reported per call: median over the rounds, and their min .. max as the run-to-run spread.

    python probes/sysid_jvp_timing.py [--out profiles/sysid_jvp_timing.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--horizon", type=int, default=100)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import sysid_vjp_common as sv
    from pdp_amd import runtime as rt, zoo
    B, T = a.batch, a.horizon
    f64 = dict(dtype=torch.float64, device="cuda")
    P, stream = rt.ptr, rt.current_stream_ptr()
    rng = np.random.default_rng(0)

    def rel(x, y):
        x, y = x.reshape(B, -1), y.reshape(B, -1)
        return float(((x - y).abs().amax(dim=1) / y.abs().amax(dim=1)).max())

    def setup(tag, mdl, x0, u, th_true, materialised):
        n, m, p = mdl.n, mdl.m, mdl.p
        xobs = mdl.sysid_integrate(x0, u, th_true)
        th = rt.dev(th_true * 1.05)
        x = mdl.sysid_integrate(x0, u, th)
        g = x - xobs
        dth, dx0, du = rt.dev(rng.standard_normal(p)), rt.dev(rng.standard_normal((B, n))), rt.dev(rng.standard_normal((B, T, m)))
        gt, g0, gt2 = torch.empty((B, p), **f64), torch.empty((B, n), **f64), torch.empty((B, p), **f64)
        dx1, dx2, dx3 = (torch.empty((B, T + 1, n), **f64) for _ in range(3))
        L = mdl.lib
        head = (B, T, P(x), P(u), P(th), 0)
        keep = [x, u, th, g, dth, dx0, du, gt, g0, gt2, dx1, dx2, dx3]

        def vjp():
            rt.check(L.pdp_sysid_rollout_vjp_batched(*head, P(g), P(gt), P(g0), stream), "vjp")

        def jvp_theta():
            rt.check(L.pdp_sysid_rollout_jvp_batched(*head, P(dth), 0, None, None, P(dx1), stream), "jvp")

        def jvp_all():
            rt.check(L.pdp_sysid_rollout_jvp_batched(*head, P(dth), 0, P(dx0), P(du), P(dx2), stream), "jvp")

        def gn():
            rt.check(L.pdp_sysid_rollout_jvp_batched(*head, P(dth), 0, None, None, P(dx3), stream), "jvp")
            rt.check(L.pdp_sysid_rollout_vjp_batched(*head, P(dx3), P(gt2), None, stream), "vjp")
        out = [(tag + " vjp", vjp), (tag + " jvp_theta", jvp_theta), (tag + " jvp_all", jvp_all), (tag + " gn", gn)]
        vjp(), jvp_theta(), jvp_all(), gn()
        torch.cuda.synchronize()
        note = "%s n = %d m = %d p = %d: pool rows %d" % (tag, n, m, p, mdl.sysid_jvp_rows(B))
        if materialised:
            def xv():
                F, E = mdl.sysid_auxsys(x, u, th)
                return rt.sysid_aux_integrate(F, E) @ dth
            note += "; J v of the kernel and of the materialised X @ v differ by %.2e" % rel(dx1, xv())
            out.append((tag + " X@v", xv))
        return out, note, keep

    quad = zoo.get("quadrotor", "sysid")
    io = np.load(os.path.join(ROOT, "tests", "golden", "iodata_quadrotor.npz"))
    x0 = rt.dev(io["states"][np.arange(B) % io["states"].shape[0], 0] * (1.0 + 0.05 * rng.standard_normal((B, quad.n))))
    vq, note_q, keep_q = setup("quadrotor", quad, x0, rt.dev(rng.uniform(-1.0, 1.0, (B, T, quad.m))), io["true_parameter"], False)
    big = sv.user_model(*sv.USER_MODELS["linear_9_2_99"])[0].model()
    A = -np.eye(9) + 0.3 * rng.standard_normal((9, 9))
    vl, note_l, keep_l = setup("linear_9_2_99", big, rt.dev(rng.standard_normal((B, 9))), rt.dev(rng.uniform(-1.0, 1.0, (B, T, 2))),
                               np.concatenate([A.reshape(-1), rng.standard_normal(18)]), True)
    variants = vq + vl
    times = {k: [] for k, _ in variants}
    for r in range(a.rounds + 1):
        for k, f in variants:
            for _ in range(min(20, a.launches)):                 # warm-up of this variant: code objects, clocks under load
                f()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                f()
            e1.record()
            e1.synchronize()
            if r > 0:                                            # round 0 is warm-up as a whole
                times[k].append(e0.elapsed_time(e1) / a.launches)
    lines = ["SysID rollout: tangent sweep (jvp) beside the adjoint sweep (vjp), B = %d, T = %d; %s" % (B, T, torch.cuda.get_device_name(0)),
             "ms per call: HIP events around %d back-to-back calls behind a warm-up, variants alternating, %d rounds (median, min .. max = run-to-run spread)"
             % (a.launches, a.rounds), note_q, note_l]
    for k, _ in variants:
        t = np.array(times[k])
        lines.append("  %-26s median %.4f ms   min %.4f   max %.4f   spread %.1f %%" % (k, np.median(t), t.min(), t.max(), 100 * (t.max() - t.min()) / np.median(t)))
    med = {k: float(np.median(times[k])) for k, _ in variants}
    for tag in ("quadrotor", "linear_9_2_99"):
        lines.append("  %s: jvp_theta / vjp = %.3f   jvp_all / vjp = %.3f   gn / vjp = %.3f" % (tag, med[tag + " jvp_theta"] / med[tag + " vjp"],
                                                                                               med[tag + " jvp_all"] / med[tag + " vjp"], med[tag + " gn"] / med[tag + " vjp"]))
    lines.append("  linear_9_2_99: X@v / gn = %.2f" % (med["linear_9_2_99 X@v"] / med["linear_9_2_99 gn"]))
    txt = "\n".join(lines) + "\n"
    print(txt, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt)


if __name__ == "__main__":
    main()
