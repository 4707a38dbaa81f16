#!/usr/bin/env python3
"""What weights and Huber's loss cost the fused OC unit (pdp_oc_pdp_grad_wls_batched, PDP_FUSED_GN_W), quadrotor B = 1024, T = 50 (the benchmark shape), same inputs:

    default          the fused unit as it is (what bench.py times): loss and gradient               } instantiations of the unchanged code object: default and gauss_newton
    gauss_newton     PDP_GRAD_GAUSS_NEWTON: the packed row gradient | loss | G                      } must time as on the parent, gn_skip_full is the YARDSTICK of this run
    gn_skip_full     PDP_GRAD_GAUSS_NEWTON | PDP_GRAD_SKIP_MISSING (PDP_FUSED_GN_MISS) on NaN-free demonstrations
    wls_w            weights [B][T+1][n] and [B][T][m] (5 % zeros), delta = +inf
    wls_wh           the same weights and Huber at the median standardised residual

HIP-event-bracketed windows of --launches back-to-back calls behind a warm-up, the variants alternating inside every round, --rounds rounds; reported per call: median
over the rounds, and their min .. max as the run-to-run spread.  Foreign calls are marshalled once (no Python wrapper inside the window).

    python probes/oc_wls_timing.py [--out profiles/oc_wls_timing.txt]
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
    wx = rt.dev(np.where(rng.random((B, T + 1, n)) < 0.05, 0.0, rng.uniform(0.25, 4.0, (B, T + 1, n))))
    wu = rt.dev(np.where(rng.random((B, T, m)) < 0.05, 0.0, rng.uniform(0.25, 4.0, (B, T, m))))
    w = p + 1 + p * p
    row, row_s, row_w, row_h = (torch.empty((B, w), **f64) for _ in range(4))
    x, lam, loss, grad, status = torch.empty((B, T + 1, n), **f64), torch.empty((B, T, n), **f64), torch.empty((B,), **f64), torch.empty((B, p), **f64), \
        torch.empty((B,), dtype=torch.int32, device="cuda")
    dxdp, dudp = torch.empty((B, T + 1, n, p), **f64), torch.empty((B, T, m, p), **f64)
    nbytes = mdl.lib.pdp_oc_pdp_workspace_bytes(B, T)
    ws = torch.empty((max(nbytes, 8) // 8,), **f64)
    P, fn, fw, stream = rt.ptr, mdl.lib.pdp_oc_pdp_grad_batched, mdl.lib.pdp_oc_pdp_grad_wls_batched, rt.current_stream_ptr()

    def args(flags, grad_t, sx=None, su=None):
        return (B, T, flags, P(x0), P(u), P(th), 0, P(gx), P(gu), P(x), P(lam), P(loss), P(grad_t), P(sx), P(su), P(status), P(ws), nbytes, stream)

    def wargs(out, wx_, wu_, delta):
        return (B, T, 0, P(x0), P(u), P(th), 0, P(gx), P(gu), P(wx_), (T + 1) * n if wx_ is not None else 0, P(wu_), T * m if wu_ is not None else 0, delta, P(x), P(lam),
                P(loss), P(out), P(status), P(ws), nbytes, stream)
    # the sensitivities, for the reference and for delta
    rt.check(fn(*args(0, grad, dxdp, dudp)), "sens")
    torch.cuda.synchronize()
    ex, eu = wx.sqrt() * (x - gx), wu.sqrt() * (u - gu)
    delta = float(torch.cat([ex[wx > 0].abs(), eu[wu > 0].abs()]).median())
    inf = float("inf")
    calls = {"default": (fn, args(0, grad)), "gauss_newton": (fn, args(16, row)), "gn_skip_full": (fn, args(16 | 32, row_s)), "wls_w": (fw, wargs(row_w, wx, wu, inf)),
             "wls_wh": (fw, wargs(row_h, wx, wu, delta))}
    variants = [(k, (lambda f=f, c=c, k=k: rt.check(f(*c), k))) for k, (f, c) in calls.items()]
    for _, f in variants:
        f()
    row_1 = torch.empty((B, w), **f64)
    rt.check(fw(*wargs(row_1, None, None, inf)), "wls without weights")
    torch.cuda.synchronize()
    dev_ones = float(((row_1 - row).abs().amax(dim=1) / row.abs().amax(dim=1)).max())
    zero = torch.zeros((), **f64)

    def side(v, demo, wt, S, dl):
        d, obs = v - demo, wt > 0
        e = wt.sqrt() * d
        ae = e.abs()
        quad = ae <= dl
        s = torch.where(quad, wt, wt * (dl / ae)).sqrt()
        return torch.where(obs, torch.where(quad, e * e, 2.0 * dl * ae - dl * dl), zero).sum(dim=(1, 2)), torch.where(obs, s * d, zero), \
            torch.where(obs[..., None], s[..., None] * S, zero), float((obs & ~quad).sum()) / float(obs.sum())
    devs, beyond = {}, 0.0
    for name, out, dl in (("wls_w", row_w, inf), ("wls_wh", row_h, delta)):
        lx, sdx, sX, bx = side(x, gx, wx, dxdp, dl)
        lu, sdu, sU, bu = side(u, gu, wu, dudp, dl)
        ref = torch.cat([torch.einsum("bti,btip->bp", sdx, sX) + torch.einsum("bti,btip->bp", sdu, sU), (lx + lu)[:, None],
                         (torch.einsum("btip,btiq->bpq", sX, sX) + torch.einsum("btip,btiq->bpq", sU, sU)).reshape(B, p * p)], dim=1)
        devs[name] = max(float(((out[:, i:j] - ref[:, i:j]).abs().amax(dim=1) / ref[:, i:j].abs().amax(dim=1)).max()) for i, j in ((0, p), (p, p + 1), (p + 1, w)))
        beyond = bx if dl != inf else beyond
        G = out[:, p + 1:].view(B, p, p)
        assert torch.equal(G, G.transpose(1, 2))
    assert int(status.sum()) == 0 and dev_ones <= 1e-10 and max(devs.values()) <= 1e-10, (dev_ones, devs)
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
    lines = ["OC gradient unit, weighted and Huber-robust least squares (PDP_FUSED_GN_W), quadrotor n = %d m = %d p = %d, B = %d, T = %d; %s" % (n, m, p, B, T, torch.cuda.get_device_name(0)),
             "ms per call: HIP events around %d back-to-back calls behind 20 warm-up calls, variants alternating, %d rounds (median, min .. max = run-to-run spread)"
             % (a.launches, a.rounds),
             "weights [B][T+1][n] and [B][T][m], 5 %% zeros; Huber delta = %.3e, %.1f %% of the weighted state entries beyond it" % (delta, 100.0 * beyond),
             "largest relative deviation (per sample, of the largest entry of gradient / loss / G): without weights at delta = inf vs the Gauss-Newton instantiation %.2e; "
             "weights vs the scaled contraction of the materialised sensitivities %.2e; weights and Huber %.2e; G symmetric to the bit" % (dev_ones, devs["wls_w"], devs["wls_wh"])]
    for k, _ in variants:
        t = np.array(times[k])
        lines.append("  %-13s median %.4f ms   min %.4f   max %.4f   spread %.1f %%" % (k, np.median(t), t.min(), t.max(), 100 * (t.max() - t.min()) / np.median(t)))
    med = {k: float(np.median(times[k])) for k, _ in variants}
    lines.append("  gauss_newton / default = %.3f   gn_skip_full / gauss_newton = %.3f   wls_w / gn_skip_full = %.3f   wls_wh / gn_skip_full = %.3f"
                 % (med["gauss_newton"] / med["default"], med["gn_skip_full"] / med["gauss_newton"], med["wls_w"] / med["gn_skip_full"], med["wls_wh"] / med["gn_skip_full"]))
    txt = "\n".join(lines) + "\n"
    print(txt, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt)


if __name__ == "__main__":
    main()
