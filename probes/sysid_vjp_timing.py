#!/usr/bin/env python3
"""The SysID rollout's vector-Jacobian product (pdp_sysid_rollout_vjp_batched, the adjoint sweep) against the forward-sensitivity routes to the same gradient,
B = 1024, T = 100, same inputs, cotangent g = x - x_obs (the one loss the forward routes serve):

    quadrotor (n = 13, p = 5: where forward sensitivities on MFMA tiles are at their best)
      a_vjp            the new kernel alone, on a rollout and a cotangent that are already there
      a_rollout_vjp    (a) pdp_sysid_integrate_batched + the new kernel: the two launches of the layer's forward and backward
      b_step           (b) pdp_sysid_step_ws_batched, the fused SysID.step of the parent: rollout and X_{t+1} = F X_t + E in one launch
    linear model x+ = x + dt (A x + B u), theta = (vec A, vec B) (n = 9, m = 2, p = 99: beyond the fused step's 64 parameters)
      c_rollout_vjp    ModelLib.sysid_integrate + ModelLib.sysid_rollout_vjp
      c_materialised   (c) ModelLib.sysid_step: integrate, getAuxSys, integrateAuxSys with X [B, T+1, n, p] in HBM, two contractions
    (both through their Python methods, allocations included: that is how the route is reached)

No threshold is set in advance: nobody has measured this kernel.  Whatever comes out is written down.

The method of probes/sysid_gn_timing.py: HIP-event-bracketed windows of --launches back-to-back calls behind a warm-up, the variants alternating inside every round,
--rounds rounds; reported per call: median over the rounds, and their min .. max as the run-to-run spread.

    python probes/sysid_vjp_timing.py [--out profiles/sysid_vjp_timing.txt]
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
    ap.add_argument("--launches-large", type=int, default=5, help="calls per window of the p = 99 variants (the materialised route moves ~1.5 GB per call)")
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

    # ---- quadrotor
    mdl = zoo.get("quadrotor", "sysid")
    n, m, p = mdl.n, mdl.m, mdl.p
    io = np.load(os.path.join(ROOT, "tests", "golden", "iodata_quadrotor.npz"))
    x0 = rt.dev(io["states"][np.arange(B) % io["states"].shape[0], 0] * (1.0 + 0.05 * rng.standard_normal((B, n))))
    u = rt.dev(rng.uniform(-1.0, 1.0, (B, T, m)))
    xobs = mdl.sysid_integrate(x0, u, io["true_parameter"])                        # the data: rolled out at the true parameter
    xobs[:, 0] = x0
    th = rt.dev(io["true_parameter"] * 1.05)
    x = torch.empty((B, T + 1, n), **f64)
    loss, grad_b, grad_a, gx0 = torch.empty((B,), **f64), torch.empty((B, p), **f64), torch.empty((B, p), **f64), torch.empty((B, n), **f64)
    nbytes = int(mdl.lib.pdp_sysid_step_workspace_bytes(B, T))
    ws = torch.empty((max(nbytes, 8) // 8,), **f64)
    wsp = P(ws) if nbytes else None
    L = mdl.lib
    roll_args = (B, T, P(x0), P(u), P(th), 0, P(x), stream)
    rt.check(L.pdp_sysid_integrate_batched(*roll_args), "integrate")
    g = x - xobs
    vjp_args = (B, T, P(x), P(u), P(th), 0, P(g), P(grad_a), P(gx0), stream)
    step_args = (B, T, P(u), P(xobs), P(th), 0, P(loss), P(grad_b), wsp, nbytes, stream)

    def a_vjp():
        rt.check(L.pdp_sysid_rollout_vjp_batched(*vjp_args), "vjp")

    def a_rollout_vjp():
        rt.check(L.pdp_sysid_integrate_batched(*roll_args), "integrate")
        rt.check(L.pdp_sysid_rollout_vjp_batched(*vjp_args), "vjp")

    def b_step():
        rt.check(L.pdp_sysid_step_ws_batched(*step_args), "step")
    a_rollout_vjp()
    b_step()
    torch.cuda.synchronize()
    dev_quad = rel(grad_a, grad_b)

    # ---- the linear model with p = 99
    sid, _ = sv.user_model(*sv.USER_MODELS["linear_9_2_99"])
    big = sid.model()
    A = -np.eye(9) + 0.3 * rng.standard_normal((9, 9))
    th_true = np.concatenate([A.reshape(-1), rng.standard_normal(18)])
    x0c, uc = rt.dev(rng.standard_normal((B, 9))), rt.dev(rng.uniform(-1.0, 1.0, (B, T, 2)))
    xobsc = big.sysid_integrate(x0c, uc, th_true)
    thc = rt.dev(th_true * 1.05)
    out_c = {}

    def c_rollout_vjp():
        xc = big.sysid_integrate(x0c, uc, thc)
        out_c["vjp"] = big.sysid_rollout_vjp(xc, uc, thc, xc - xobsc, want_ini=False)["grad_theta"]

    def c_materialised():
        out_c["mat"] = big.sysid_step(uc, xobsc, thc)[1]
    c_rollout_vjp()
    c_materialised()
    torch.cuda.synchronize()
    dev_lin = rel(out_c["vjp"], out_c["mat"])
    assert max(dev_quad, dev_lin) <= 1e-10, (dev_quad, dev_lin)

    variants = (("a_vjp", a_vjp, a.launches), ("a_rollout_vjp", a_rollout_vjp, a.launches), ("b_step", b_step, a.launches),
                ("c_rollout_vjp", c_rollout_vjp, a.launches_large), ("c_materialised", c_materialised, a.launches_large))
    times = {k: [] for k, _, _ in variants}
    for r in range(a.rounds + 1):
        for k, f, count in variants:
            for _ in range(min(20, count)):                      # warm-up of this variant: code objects, allocator, clocks under load
                f()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(count):
                f()
            e1.record()
            e1.synchronize()
            if r > 0:                                            # round 0 is warm-up as a whole
                times[k].append(e0.elapsed_time(e1) / count)
    lines = ["SysID gradient by the adjoint sweep (pdp_sysid_rollout_vjp_batched) against the forward-sensitivity routes, B = %d, T = %d, g = x - x_obs; %s"
             % (B, T, torch.cuda.get_device_name(0)),
             "ms per call: HIP events around %d (p = 99: %d) back-to-back calls behind a warm-up, variants alternating, %d rounds (median, min .. max = run-to-run spread)"
             % (a.launches, a.launches_large, a.rounds),
             "quadrotor n = %d m = %d p = %d, pool rows %d; linear model n = 9 m = 2 p = 99, pool rows %d" % (n, m, p, mdl.sysid_vjp_rows(B, torch.cuda.get_device_properties(0).multi_processor_count),
                                                                                                    big.sysid_vjp_rows(B, torch.cuda.get_device_properties(0).multi_processor_count)),
             "largest relative deviation of the gradients (per sample, of the largest entry): quadrotor a vs b %.2e; linear model c_rollout_vjp vs c_materialised %.2e"
             % (dev_quad, dev_lin)]
    for k, _, _ in variants:
        t = np.array(times[k])
        lines.append("  %-16s median %.4f ms   min %.4f   max %.4f   spread %.1f %%" % (k, np.median(t), t.min(), t.max(), 100 * (t.max() - t.min()) / np.median(t)))
    med = {k: float(np.median(times[k])) for k, _, _ in variants}
    lines.append("  a_rollout_vjp / b_step = %.3f   a_vjp / b_step = %.3f   c_rollout_vjp / c_materialised = %.4f"
                 % (med["a_rollout_vjp"] / med["b_step"], med["a_vjp"] / med["b_step"], med["c_rollout_vjp"] / med["c_materialised"]))
    txt = "\n".join(lines) + "\n"
    print(txt, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt)


if __name__ == "__main__":
    main()
