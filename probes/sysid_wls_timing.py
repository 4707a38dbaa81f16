#!/usr/bin/env python3
"""SysID.step as weighted and Huber-robust least squares against the skip-missing Gauss-Newton modes, quadrotor B = 1024, T = 100 (bench config C5a), same inputs:

    gn_miss       pdp_sysid_step_gn_batched, PDP_GRAD_SKIP_MISSING on NaN-free data, a given x0 (MODE 2) - THE YARDSTICK: the unchanged code object, timed in the same run
    wls_w         pdp_sysid_step_wls_batched (MODE 5), per-entry weights [B][T+1][n] with 5 % zeros, delta = +inf
    wls_wh        the same with Huber at the median standardised residual
    ini_miss      pdp_sysid_step_gn_ini_batched, q = 6 (components 3, 4, 5, 10, 11, 12; W = 11), the flag (MODE 4)
    wls_ini_w / wls_ini_wh   MODE 6 with the same mask: weights only / weights and Huber
    materialised  the route ModelLib.sysid_step takes beyond the tile (sysid_integrate, sysid_auxsys, sysid_aux_integrate, scaled residuals and a row-scaled X in two
                  einsums), restated here on the same inputs, weights and Huber

The estimate, written down before the first run: one wavefront per SIMD at this batch.  The sensitivity loop gains a gather of four LDS words,
four multiplies and four compare-select pairs per step where MODE 2 has four compares and eight selects (about 67 cycles per step, section 4.1d): 20 - 45 cycles more
per step, 1 - 2 us over T = 100.  The lane-parallel pass gains a division and two square roots per entry in fp64 (about 200 cycles per entry, 13 entries per lane, four
chunks of 25 lanes): about 10 000 cycles, 4 - 5 us.  Huber on or off is a run-time select around the same instructions.  Expectation: wls_w = wls_wh = 1.07 - 1.10 x
gn_miss, wls_ini_* the same against ini_miss, the materialised route tens of times slower.  Whatever comes out is written down.

The method of probes/sysid_ini_timing.py: HIP-event-bracketed windows of --launches back-to-back calls behind a warm-up, the variants alternating inside every round,
--rounds rounds; reported per call: median over the rounds, and their min .. max as the run-to-run spread.  Foreign calls are marshalled once.

    python probes/sysid_wls_timing.py [--out profiles/sysid_wls_timing.txt]
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
    wnp = np.broadcast_to(1.0 / (0.5 + np.arange(n)) ** 2, (B, T + 1, n)).copy()
    wnp[rng.random(wnp.shape) < 0.05] = 0.0
    w = rt.dev(wnp)
    x = mdl.sysid_integrate(x0, u, th)
    e = (w.sqrt() * (x - xobs)).abs()
    delta = float(e[w > 0].median())
    beyond = float((e[w > 0] > delta).double().mean())
    inf = float("inf")
    loss = torch.empty((B,), **f64)
    names = ("gn_miss", "wls_w", "wls_wh", "ini_miss", "wls_ini_w", "wls_ini_wh")
    rows = {k: torch.empty((B, (W if "ini" in k else p) * ((W if "ini" in k else p) + 1) + 1), **f64) for k in names}
    nbytes = int(mdl.lib.pdp_sysid_step_workspace_bytes(B, T))
    ws = torch.empty((max(nbytes, 8) // 8,), **f64)
    P, stream = rt.ptr, rt.current_stream_ptr()
    wsp = P(ws) if nbytes else None
    fn_gn, fn_ini, fn_wls = mdl.lib.pdp_sysid_step_gn_batched, mdl.lib.pdp_sysid_step_gn_ini_batched, mdl.lib.pdp_sysid_step_wls_batched

    def gn(row):
        args = (B, T, P(u), P(xobs), P(x0), P(th), 0, 32, P(loss), P(row), wsp, nbytes, stream)
        return lambda: rt.check(fn_gn(*args), "gn")

    def ini(row):
        args = (B, T, P(u), P(xobs), P(x0), mask, P(th), 0, 32, P(loss), P(row), wsp, nbytes, stream)
        return lambda: rt.check(fn_ini(*args), "ini")

    def wls(row, msk, dlt):
        args = (B, T, P(u), P(xobs), P(x0), msk, P(w), (T + 1) * n, dlt, P(th), 0, 32, P(loss), P(row), wsp, nbytes, stream)
        return lambda: rt.check(fn_wls(*args), "wls")

    mat = {}

    def materialised():
        xs = mdl.sysid_integrate(x0, u, th)
        F, E = mdl.sysid_auxsys(xs, u, th)
        X = rt.sysid_aux_integrate(F, E)                                           # [B, T+1, n, p]
        zero = torch.zeros((), **f64)
        d = xs - xobs
        obs = (w > 0) & (xobs == xobs)
        ee = w.sqrt() * d
        ae = ee.abs()
        quad = ae <= delta
        s = torch.where(quad, w, w * (delta / ae)).sqrt()
        mat["loss"] = torch.where(obs, torch.where(quad, ee * ee, 2.0 * delta * ae - delta * delta), zero).sum(dim=(1, 2))
        sd = torch.where(obs, s * d, zero)
        sX = torch.where((obs & (s != 0))[..., None], s[..., None] * X, zero)
        mat["grad"] = torch.einsum("bti,btip->bp", sd, sX)
        mat["G"] = torch.einsum("btip,btiq->bpq", sX, sX)
    variants = (("gn_miss", gn(rows["gn_miss"])), ("wls_w", wls(rows["wls_w"], 0, inf)), ("wls_wh", wls(rows["wls_wh"], 0, delta)), ("ini_miss", ini(rows["ini_miss"])),
                ("wls_ini_w", wls(rows["wls_ini_w"], mask, inf)), ("wls_ini_wh", wls(rows["wls_ini_wh"], mask, delta)), ("materialised", materialised))
    # results first: the fused rows against the materialised restatement, and the theta block of MODE 6 against MODE 5
    for _, f in variants:
        f()
    torch.cuda.synchronize()

    def rel(x_, y_):
        x_, y_ = x_.reshape(B, -1), y_.reshape(B, -1)
        return float(((x_ - y_).abs().amax(dim=1) / y_.abs().amax(dim=1)).max())
    r5, r6 = rows["wls_wh"], rows["wls_ini_wh"]
    dev_mat = max(rel(r5[:, :p], mat["grad"]), rel(r5[:, p:p + 1], mat["loss"][:, None]), rel(r5[:, p + 1:], mat["G"]))
    G6 = r6[:, W + 1:].reshape(B, W, W)
    dev_56 = max(rel(r6[:, :p], r5[:, :p]), rel(r6[:, W:W + 1], r5[:, p:p + 1]), rel(G6[:, :p, :p], r5[:, p + 1:]))
    assert torch.equal(G6, G6.transpose(1, 2)) and max(dev_mat, dev_56) <= 1e-10 and all(bool(torch.isfinite(v).all()) for v in rows.values()), (dev_mat, dev_56)
    times = {k: [] for k, _ in variants}
    for r in range(a.rounds + 1):
        for k, f in variants:
            nl = a.launches if k != "materialised" else max(1, a.launches // 20)
            for _ in range(20 if k != "materialised" else 2):    # warm-up of this variant: code objects, allocator, clocks under load
                f()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(nl):
                f()
            e1.record()
            e1.synchronize()
            if r > 0:                                            # round 0 is warm-up as a whole
                times[k].append(e0.elapsed_time(e1) / nl)
    lines = ["SysID.step, weighted and Huber-robust least squares, quadrotor n = %d m = %d p = %d q = %d (W = %d), B = %d, T = %d; %s"
             % (n, m, p, q, W, B, T, torch.cuda.get_device_name(0)),
             "ms per call: HIP events around %d back-to-back calls (materialised: %d) behind a warm-up, variants alternating, %d rounds (median, min .. max = run-to-run spread)"
             % (a.launches, max(1, a.launches // 20), a.rounds),
             "weights [B][T+1][n], 5 %% zeros; Huber delta = %.3e, %.1f %% of the weighted entries beyond it" % (delta, 100 * beyond),
             "estimate before the run: wls_w = wls_wh = 1.07 - 1.10 x gn_miss, wls_ini_* the same against ini_miss; the materialised route tens of times slower",
             "largest relative deviation (per sample, of the largest entry): MODE 5 row vs the materialised restatement %.2e; theta block of MODE 6 vs MODE 5 %.2e; "
             "G symmetric to the bit" % (dev_mat, dev_56)]
    for k, _ in variants:
        t = np.array(times[k])
        lines.append("  %-14s median %.4f ms   min %.4f   max %.4f   spread %.1f %%" % (k, np.median(t), t.min(), t.max(), 100 * (t.max() - t.min()) / np.median(t)))
    med = {k: float(np.median(times[k])) for k, _ in variants}
    lines.append("  wls_w / gn_miss = %.3f   wls_wh / gn_miss = %.3f   wls_ini_w / ini_miss = %.3f   wls_ini_wh / ini_miss = %.3f   materialised / wls_wh = %.1f"
                 % (med["wls_w"] / med["gn_miss"], med["wls_wh"] / med["gn_miss"], med["wls_ini_w"] / med["ini_miss"], med["wls_ini_wh"] / med["ini_miss"],
                    med["materialised"] / med["wls_wh"]))
    txt = "\n".join(lines) + "\n"
    print(txt, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt)


if __name__ == "__main__":
    main()
