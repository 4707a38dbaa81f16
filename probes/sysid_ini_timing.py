#!/usr/bin/env python3
"""SysID.step with estimated components of the initial state against the Gauss-Newton modes it extends, quadrotor B = 1024, T = 100 (bench config C5a), same inputs,
the velocities and body rates of x0 estimated (q = 6: components 3, 4, 5, 10, 11, 12; W = 11):

    gn           pdp_sysid_step_gn_batched, flags 0 (MODE 1): the row gradient [5] | loss | G [5][5]
    ini          pdp_sysid_step_gn_ini_batched, flags 0 (MODE 3): the row gradient [11] | loss | G [11][11]
    gn_miss      MODE 2 (PDP_GRAD_SKIP_MISSING) on NaN-free data, a given x0 - THE YARDSTICK: the unchanged code object, timed in the same run
    ini_miss     MODE 4 on the same data with the same x0
    gn_miss_half / ini_miss_half   MODE 2 / MODE 4 with every second step and every second component NaN

The estimate, written down before the first run: the new modes issue the same tile operations per step (the unit columns ride in the columns of the X tile that were
zero; no MFMA, no LDS word more) and differ in the initial tile (a scan of n mask bits per lane, once) and in the row they write, 133 instead of 31 doubles per
trajectory - 1.09 MB instead of 0.25 MB per call, well under a microsecond of HBM time against a call of some 0.07 ms.  Expectation: ini / gn and ini_miss / gn_miss
within the run-to-run spread of gn_miss.  Whatever comes out is written down.

The method of probes/sysid_gn_timing.py: HIP-event-bracketed windows of --launches back-to-back calls behind a warm-up, the variants alternating inside every round,
--rounds rounds; reported per call: median over the rounds, and their min .. max as the run-to-run spread.  Foreign calls are marshalled once.

    python probes/sysid_ini_timing.py [--out profiles/sysid_ini_timing.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IDX = [3, 4, 5, 10, 11, 12]


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
    q, mask = len(IDX), sum(1 << i for i in IDX)
    W = p + q
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
    loss = torch.empty((B,), **f64)
    names = ("gn", "ini", "gn_miss", "ini_miss", "gn_miss_half", "ini_miss_half")
    rows = {k: torch.empty((B, (W if k.startswith("ini") else p) * ((W if k.startswith("ini") else p) + 1) + 1), **f64) for k in names}
    nbytes = int(mdl.lib.pdp_sysid_step_workspace_bytes(B, T))
    ws = torch.empty((max(nbytes, 8) // 8,), **f64)
    P, stream = rt.ptr, rt.current_stream_ptr()
    wsp = P(ws) if nbytes else None
    fn_gn, fn_ini = mdl.lib.pdp_sysid_step_gn_batched, mdl.lib.pdp_sysid_step_gn_ini_batched

    def gn(obs, flags, row):
        args = (B, T, P(u), P(obs), P(x0), P(th), 0, flags, P(loss), P(row), wsp, nbytes, stream)
        return lambda: rt.check(fn_gn(*args), "gn")

    def ini(obs, flags, row):
        args = (B, T, P(u), P(obs), P(x0), mask, P(th), 0, flags, P(loss), P(row), wsp, nbytes, stream)
        return lambda: rt.check(fn_ini(*args), "ini")
    variants = (("gn", gn(xobs, 0, rows["gn"])), ("ini", ini(xobs, 0, rows["ini"])), ("gn_miss", gn(xobs, 32, rows["gn_miss"])), ("ini_miss", ini(xobs, 32, rows["ini_miss"])),
                ("gn_miss_half", gn(half, 32, rows["gn_miss_half"])), ("ini_miss_half", ini(half, 32, rows["ini_miss_half"])))
    # results first: the theta block of the augmented row is the row of the mode it extends; the x0 block against the materialised sensitivities
    for _, f in variants:
        f()
    torch.cuda.synchronize()

    def blocks(row, w):
        return row[:, :w], row[:, w], row[:, w + 1:].reshape(B, w, w)

    def rel(x, y):
        x, y = x.reshape(B, -1), y.reshape(B, -1)
        return float(((x - y).abs().amax(dim=1) / y.abs().amax(dim=1)).max())
    devs = []
    for k in ("", "_miss", "_miss_half"):
        (g1, l1, G1), (g3, l3, G3) = blocks(rows["gn" + k], p), blocks(rows["ini" + k], W)
        devs.append(max(rel(g3[:, :p], g1), rel(l3[:, None], l1[:, None]), rel(G3[:, :p, :p], G1)))
        assert torch.equal(G3, G3.transpose(1, 2))
    x = mdl.sysid_integrate(x0, u, th)
    F, E = mdl.sysid_auxsys(x, u, th)
    Ew, X0 = torch.zeros((B, T, n, W), **f64), torch.zeros((B, n, W), **f64)
    Ew[..., :p] = E
    for k, i in enumerate(IDX):
        X0[:, i, p + k] = 1.0
    X = rt.sysid_aux_integrate(F, Ew, X0)
    d = x - xobs
    g3, _, G3 = blocks(rows["ini"], W)
    dev_g, dev_G = rel(g3, torch.einsum("bti,btip->bp", d, X)), rel(G3, torch.einsum("btip,btiq->bpq", X, X))
    assert max(devs + [dev_g, dev_G]) <= 1e-10 and bool(torch.isfinite(rows["ini_miss_half"]).all()), (devs, dev_g, dev_G)
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
    lines = ["SysID.step with estimated components of the initial state, quadrotor n = %d m = %d p = %d q = %d (W = %d), B = %d, T = %d; %s"
             % (n, m, p, q, W, B, T, torch.cuda.get_device_name(0)),
             "ms per call: HIP events around %d back-to-back calls behind 20 warm-up calls, variants alternating, %d rounds (median, min .. max = run-to-run spread)"
             % (a.launches, a.rounds),
             "estimate before the run: ini / gn and ini_miss / gn_miss within the run-to-run spread of gn_miss (same tile operations; the row is %d instead of %d doubles)"
             % (W + 1 + W * W, p + 1 + p * p),
             "largest relative deviation (per sample, of the largest entry): theta block of the augmented row vs the row of MODE 1 / 2 / 2 half-masked %.2e / %.2e / %.2e; "
             "augmented gradient and G vs materialised sensitivities %.2e, %.2e; G symmetric to the bit" % (devs[0], devs[1], devs[2], dev_g, dev_G)]
    for k, _ in variants:
        t = np.array(times[k])
        lines.append("  %-14s median %.4f ms   min %.4f   max %.4f   spread %.1f %%" % (k, np.median(t), t.min(), t.max(), 100 * (t.max() - t.min()) / np.median(t)))
    med = {k: float(np.median(times[k])) for k, _ in variants}
    lines.append("  ini / gn = %.3f   ini_miss / gn_miss = %.3f   ini_miss_half / gn_miss_half = %.3f"
                 % (med["ini"] / med["gn"], med["ini_miss"] / med["gn_miss"], med["ini_miss_half"] / med["gn_miss_half"]))
    txt = "\n".join(lines) + "\n"
    print(txt, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt)


if __name__ == "__main__":
    main()
