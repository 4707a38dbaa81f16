#!/usr/bin/env python3
"""What the gradient with respect to the inputs costs on the SysID rollout's adjoint sweep: sysid_vjp_kernel (pdp_sysid_rollout_vjp_batched, the code object it was
before sysid_vjp_u_kernel existed) against sysid_vjp_u_kernel (pdp_sysid_rollout_vjp_u_batched) in the same run, B = 1024, T = 100, on a rollout and a cotangent that
are already there:

    quadrotor (n = 13, m = 4, p = 5: the G columns share the one lane slot with the parameters) and the linear model x+ = x + dt (A x + B u), theta = (vec A, vec B)
    (n = 9, m = 2, p = 99: the G columns are lanes 35 and 36 of the second slot)
      old        pdp_sysid_rollout_vjp_batched: grad_theta and grad_x0
      u_all      pdp_sysid_rollout_vjp_u_batched: grad_theta, grad_x0 and grad_u
      u_only     pdp_sysid_rollout_vjp_u_batched: grad_u alone

No threshold is set in advance: nobody has measured this kernel.  Whatever comes out is written down beside the estimate.

The method of probes/sysid_vjp_timing.py: HIP-event-bracketed windows of --launches back-to-back calls behind a warm-up, the variants alternating inside every round,
--rounds rounds; reported per call: median over the rounds, and their min .. max as the run-to-run spread.

    python probes/sysid_vjp_u_timing.py [--out profiles/sysid_vjp_u_timing.txt]
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
    cus = torch.cuda.get_device_properties(0).multi_processor_count

    def rel(x, y):
        x, y = x.reshape(B, -1), y.reshape(B, -1)
        return float(((x - y).abs().amax(dim=1) / y.abs().amax(dim=1)).max())

    def setup(tag, mdl, x0, u, th_true):
        n, m, p = mdl.n, mdl.m, mdl.p
        xobs = mdl.sysid_integrate(x0, u, th_true)
        th = rt.dev(th_true * 1.05)
        x = mdl.sysid_integrate(x0, u, th)
        g = x - xobs
        gt0, g00 = torch.empty((B, p), **f64), torch.empty((B, n), **f64)
        gt1, g01, gu1, gu2 = torch.empty((B, p), **f64), torch.empty((B, n), **f64), torch.empty((B, T, m), **f64), torch.empty((B, T, m), **f64)
        L = mdl.lib
        head = (B, T, P(x), P(u), P(th), 0, P(g))
        keep = (x, u, th, g, gt0, g00, gt1, g01, gu1, gu2)

        def old():
            rt.check(L.pdp_sysid_rollout_vjp_batched(*head, P(gt0), P(g00), stream), "vjp")

        def u_all():
            rt.check(L.pdp_sysid_rollout_vjp_u_batched(*head, P(gt1), P(g01), P(gu1), stream), "vjp_u")

        def u_only():
            rt.check(L.pdp_sysid_rollout_vjp_u_batched(*head, None, None, P(gu2), stream), "vjp_u")
        old(), u_all(), u_only()
        torch.cuda.synchronize()
        dev = max(rel(gt1, gt0), rel(g01, g00))
        assert dev <= 1e-10 and bool((gu1 == gu2).all()), (tag, dev)
        note = "%s n = %d m = %d p = %d: pool rows %d (old) / %d (with grad_u); grad_theta, grad_x0 of the two kernels differ by %.2e, bit-equal: %s" % (
            tag, n, m, p, mdl.sysid_vjp_rows(B, cus), mdl.sysid_vjp_u_rows(B), dev, bool((gt1 == gt0).all() and (g01 == g00).all()))
        return [(tag + " old", old), (tag + " u_all", u_all), (tag + " u_only", u_only)], note, keep

    quad = zoo.get("quadrotor", "sysid")
    io = np.load(os.path.join(ROOT, "tests", "golden", "iodata_quadrotor.npz"))
    x0 = rt.dev(io["states"][np.arange(B) % io["states"].shape[0], 0] * (1.0 + 0.05 * rng.standard_normal((B, quad.n))))
    vq, note_q, keep_q = setup("quadrotor", quad, x0, rt.dev(rng.uniform(-1.0, 1.0, (B, T, quad.m))), io["true_parameter"])
    big = sv.user_model(*sv.USER_MODELS["linear_9_2_99"])[0].model()
    A = -np.eye(9) + 0.3 * rng.standard_normal((9, 9))
    vl, note_l, keep_l = setup("linear_9_2_99", big, rt.dev(rng.standard_normal((B, 9))), rt.dev(rng.uniform(-1.0, 1.0, (B, T, 2))),
                               np.concatenate([A.reshape(-1), rng.standard_normal(18)]))
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
    lines = ["SysID adjoint sweep with and without the gradient with respect to the inputs, B = %d, T = %d, g = x - x_obs; %s" % (B, T, torch.cuda.get_device_name(0)),
             "ms per call: HIP events around %d back-to-back calls behind a warm-up, variants alternating, %d rounds (median, min .. max = run-to-run spread)"
             % (a.launches, a.rounds), note_q, note_l]
    for k, _ in variants:
        t = np.array(times[k])
        lines.append("  %-22s median %.4f ms   min %.4f   max %.4f   spread %.1f %%" % (k, np.median(t), t.min(), t.max(), 100 * (t.max() - t.min()) / np.median(t)))
    med = {k: float(np.median(times[k])) for k, _ in variants}
    for tag in ("quadrotor", "linear_9_2_99"):
        lines.append("  %s: u_all / old = %.3f   u_only / old = %.3f" % (tag, med[tag + " u_all"] / med[tag + " old"], med[tag + " u_only"] / med[tag + " old"]))
    txt = "\n".join(lines) + "\n"
    print(txt, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt)


if __name__ == "__main__":
    main()
