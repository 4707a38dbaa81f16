#!/usr/bin/env python3
"""SysID.step with the Gauss-Newton matrix G = sum_t X_t' X_t, quadrotor B = 1024, T = 100 (bench config C5a), same inputs:

    plain        pdp_sysid_step_ws_batched as it is (what bench.py times): loss and gradient, one launch
    gn           pdp_sysid_step_gn_batched, flags 0 (MODE 1): the packed row gradient | loss | G, one launch
    gn_miss      the same with PDP_GRAD_SKIP_MISSING (MODE 2) on NaN-free data
    gn_miss_half MODE 2 with every second step and every second component NaN (a given initial state)
    materialise  what a caller had to do before the entry point existed (and what runtime.ModelLib.sysid_step still does beyond the fused kernels' tiles):
                 sysid_integrate, sysid_auxsys, sysid_aux_integrate to HBM, then the residual and two torch.einsum

The method of probes/oc_gn_timing.py: HIP-event-bracketed windows of --launches back-to-back calls behind a warm-up, the variants alternating inside every round,
--rounds rounds; reported per call: median over the rounds, and their min .. max as the run-to-run spread.  Foreign calls of the fused variants are marshalled once
(no Python wrapper inside the window).

    python probes/sysid_gn_timing.py [--out profiles/sysid_gn_timing.txt]
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
    ap.add_argument("--horizon", type=int, default=100)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from pdp_amd import runtime as rt, zoo
    mdl = zoo.get("quadrotor", "sysid")
    B, T, n, m, p = a.batch, a.horizon, mdl.n, mdl.m, mdl.p
    io = np.load(os.path.join(ROOT, "tests", "golden", "iodata_quadrotor.npz"))
    rng = np.random.default_rng(0)
    f64 = dict(dtype=torch.float64, device="cuda")
    x0 = rt.dev(io["states"][np.arange(B) % io["states"].shape[0], 0] * (1.0 + 0.05 * rng.standard_normal((B, n))))
    u = rt.dev(rng.uniform(-1.0, 1.0, (B, T, m)))
    xobs = mdl.sysid_integrate(x0, u, io["true_parameter"])                        # the data: rolled out at the true parameter
    th = rt.dev(io["true_parameter"] * 1.05)
    half = xobs.clone()
    half[:, 0::2, :] = float("nan")
    half[:, :, 1::2] = float("nan")
    loss, grad = torch.empty((B,), **f64), torch.empty((B, p), **f64)
    rows = {k: torch.empty((B, p + 1 + p * p), **f64) for k in ("gn", "gn_miss", "gn_miss_half")}
    nbytes = int(mdl.lib.pdp_sysid_step_workspace_bytes(B, T))
    ws = torch.empty((max(nbytes, 8) // 8,), **f64)
    P, stream = rt.ptr, rt.current_stream_ptr()
    a_plain = (B, T, P(u), P(xobs), P(th), 0, P(loss), P(grad), P(ws) if nbytes else None, nbytes, stream)

    def gn_args(obs, ini, flags, row):
        return (B, T, P(u), P(obs), P(ini) if ini is not None else None, P(th), 0, flags, P(loss), P(row), P(ws) if nbytes else None, nbytes, stream)
    a_gn, a_miss, a_half = gn_args(xobs, None, 0, rows["gn"]), gn_args(xobs, None, 32, rows["gn_miss"]), gn_args(half, x0, 32, rows["gn_miss_half"])
    fn_plain, fn_gn = mdl.lib.pdp_sysid_step_ws_batched, mdl.lib.pdp_sysid_step_gn_batched
    alt = {}

    def materialise():
        x = mdl.sysid_integrate(x0, u, th)
        F, E = mdl.sysid_auxsys(x, u, th)
        X = rt.sysid_aux_integrate(F, E)
        d = x - xobs
        alt["loss"], alt["grad"], alt["G"] = (d * d).sum(dim=(1, 2)), torch.einsum("bti,btip->bp", d, X), torch.einsum("btip,btiq->bpq", X, X)
        alt["bytes"] = 8 * (x.numel() + F.numel() + E.numel() + X.numel())
    variants = (("plain", lambda: rt.check(fn_plain(*a_plain), "plain")), ("gn", lambda: rt.check(fn_gn(*a_gn), "gn")),
                ("gn_miss", lambda: rt.check(fn_gn(*a_miss), "gn_miss")), ("gn_miss_half", lambda: rt.check(fn_gn(*a_half), "gn_miss_half")), ("materialise", materialise))
    # results first: the fused modes and the materialised alternative compute the same row
    for _, f in variants:
        f()
    torch.cuda.synchronize()
    G = rows["gn"][:, p + 1:].reshape(B, p, p)

    def rel(x, y):
        x, y = x.reshape(B, -1), y.reshape(B, -1)
        return float(((x - y).abs().amax(dim=1) / y.abs().amax(dim=1)).max())
    dev_G, dev_g, dev_plain, dev_modes = rel(G, alt["G"]), rel(rows["gn"][:, :p], alt["grad"]), rel(rows["gn"][:, :p], grad), rel(rows["gn_miss"], rows["gn"])
    assert max(dev_G, dev_g, dev_plain, dev_modes) <= 1e-10 and torch.equal(G, G.transpose(1, 2)) and bool(torch.isfinite(rows["gn_miss_half"]).all()), \
        (dev_G, dev_g, dev_plain, dev_modes)
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
    lines = ["SysID.step with the Gauss-Newton matrix, quadrotor n = %d m = %d p = %d, B = %d, T = %d; %s" % (n, m, p, B, T, torch.cuda.get_device_name(0)),
             "ms per call: HIP events around %d back-to-back calls behind 20 warm-up calls, variants alternating, %d rounds (median, min .. max = run-to-run spread)"
             % (a.launches, a.rounds),
             "largest relative deviation (per sample, of the largest entry): G fused vs materialised %.2e, gradient fused vs materialised %.2e, gradient MODE 1 vs plain kernel "
             "%.2e, packed row MODE 2 vs MODE 1 on NaN-free data %.2e; G symmetric to the bit" % (dev_G, dev_g, dev_plain, dev_modes)]
    for k, _ in variants:
        t = np.array(times[k])
        lines.append("  %-12s median %.4f ms   min %.4f   max %.4f   spread %.1f %%" % (k, np.median(t), t.min(), t.max(), 100 * (t.max() - t.min()) / np.median(t)))
    med = {k: float(np.median(times[k])) for k, _ in variants}
    lines.append("  gn / plain = %.3f   gn_miss / plain = %.3f   gn_miss_half / plain = %.3f   materialise / gn = %.2f   materialise / gn_miss = %.2f"
                 % (med["gn"] / med["plain"], med["gn_miss"] / med["plain"], med["gn_miss_half"] / med["plain"], med["materialise"] / med["gn"], med["materialise"] / med["gn_miss"]))
    lines.append("  trajectory, Jacobians and sensitivities the materialised route writes and re-reads: %.1f MB" % (alt["bytes"] / 1e6))
    txt = "\n".join(lines) + "\n"
    print(txt, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt)


if __name__ == "__main__":
    main()
