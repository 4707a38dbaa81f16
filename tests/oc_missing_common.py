"""Shared by tests/test_gpu_oc_missing.py (in-process and in its child processes): masks of missing observations for the inputs of tests/oc_vjp_common.make_inputs, and
one shape of PDP_GRAD_SKIP_MISSING through every call it is compared with.

Samples of a batch: the last one has EVERY demonstration entry NaN, the one before it has none; the others are masked."""
import numpy as np


def all_nan_sample(B):
    return B - 1


def nan_free_sample(B):
    return B - 2


def make_masks(B, T, n, m, seed=11):
    """(wx [B, T+1, n], wu [B, T, m]) bool, True = observed.  About half of all entries are missing (fixed seed), and missing for certain are: all of demo_x[:, 0]; one
    whole state row (t = T // 3) and one whole control row (t = 2 T // 3) in mid-horizon; states and controls of the two steps on both sides of the boundary between two
    chunks of equal length (t = (T + 1) // 2 - 1 and (T + 1) // 2: where a horizon that needs two chunks is cut); demo_u at t = 0 and T - 1; the even components of
    demo_x[:, T] (the odd ones are observed for certain)."""
    rng = np.random.default_rng(seed)
    wx, wu = rng.random((B, T + 1, n)) < 0.5, rng.random((B, T, m)) < 0.5
    tb = (T + 1) // 2
    wx[:, 0] = False
    wx[:, T // 3] = False
    wu[:, (2 * T) // 3] = False
    wx[:, tb - 1:tb + 1] = False
    wu[:, tb - 1:tb + 1] = False
    wu[:, 0] = False
    wu[:, T - 1] = False
    wx[:, T, 0::2] = False
    wx[:, T, 1::2] = True
    wx[all_nan_sample(B)], wu[all_nan_sample(B)] = False, False
    wx[nan_free_sample(B)], wu[nan_free_sample(B)] = True, True
    return wx, wu


def mask_inputs(inp):
    """inp (oc_vjp_common.make_inputs) with wx, wu, the NaN-marked demonstrations demo_xm / demo_um and the zero-filled ones demo_x0 / demo_u0"""
    B, T = inp["B"], inp["T"]
    n, m = inp["demo_x"].shape[2], inp["demo_u"].shape[2]
    wx, wu = make_masks(B, T, n, m)
    out = dict(inp, wx=wx, wu=wu)
    out["demo_xm"], out["demo_um"] = np.where(wx, inp["demo_x"], np.nan), np.where(wu, inp["demo_u"], np.nan)
    out["demo_x0"], out["demo_u0"] = np.where(wx, inp["demo_x"], 0.0), np.where(wu, inp["demo_u"], 0.0)
    return out


def contract(x, u, demo_x0, demo_u0, wx, wu, dxdp, dudp):
    """the three formulas of PDP_GRAD_SKIP_MISSING (include/pdp_hip.h) in torch fp64: (loss [B], grad [B, p], G [B, p, p]) from the trajectory, the zero-filled
    demonstrations, the masks and the sensitivities"""
    import torch
    zero = torch.zeros((), dtype=torch.float64, device=x.device)
    ex, eu = torch.where(wx, x - demo_x0, zero), torch.where(wu, u - demo_u0, zero)
    Xm, Um = torch.where(wx[..., None], dxdp, zero), torch.where(wu[..., None], dudp, zero)
    loss = (ex ** 2).sum(dim=(1, 2)) + (eu ** 2).sum(dim=(1, 2))
    grad = torch.einsum("bti,btip->bp", ex, Xm) + torch.einsum("bti,btip->bp", eu, Um)
    G = torch.einsum("btip,btiq->bpq", Xm, Xm) + torch.einsum("btip,btiq->bpq", Um, Um)
    return loss, grad, G


def evaluate(mdl, inp, per_sample=False, given=False):
    """The default unit (plain, with the sensitivities written, and its Gauss-Newton instantiation) on the zero-filled demonstrations, and the unit with skip_missing on
    the NaN-marked ones: with gauss_newton, alone and packed.  given: the skip_missing calls get the default call's (x, lam) (PDP_OC_GIVEN_TRAJ), else they roll out from
    x0.  Output rows are pre-filled with NaN and followed by one guard row.  Returns numpy arrays; the reference is contract() on the default unit's own outputs."""
    import torch
    from pdp_amd import runtime as rt
    mi = mask_inputs(inp)
    th = mi["theta_b"] if per_sample else mi["theta"]
    u, x0 = rt.dev(mi["u"]), mi["x0"]
    dxm, dum, dx0, du0 = (rt.dev(mi[k]) for k in ("demo_xm", "demo_um", "demo_x0", "demo_u0"))
    wx, wu = torch.as_tensor(mi["wx"], device="cuda"), torch.as_tensor(mi["wu"], device="cuda")
    B, p = u.shape[0], mdl.p
    d0 = mdl.oc_pdp_grad(u, th, dx0, du0, x0=x0)
    ds = mdl.oc_pdp_grad(u, th, dx0, du0, x0=x0, want_sens=True)
    g0 = mdl.oc_pdp_grad(u, th, dx0, du0, x0=x0, gauss_newton=True)              # (the NaN-free sample: the same call without the flag)
    loss_ref, grad_ref, G_ref = contract(ds["x"], u, dx0, du0, wx, wu, ds["dxdp"], ds["dudp"])

    def traj():
        return dict(x=d0["x"].clone(), lam=d0["lam"].clone()) if given else dict(x0=x0)
    nan = float("nan")
    rows = torch.full((B + 1, p + 1 + p * p), nan, dtype=torch.float64, device="cuda")
    g = mdl.oc_pdp_grad(u, th, dxm, dum, gauss_newton=True, skip_missing=True, buffers={"packed_gn": rows[:B]}, **traj())
    assert g["packed_gn"].data_ptr() == rows.data_ptr() and g["gn"].shape == (B, p, p) and g["grad"].shape == (B, p)
    gbuf = torch.full((B + 1, p), nan, dtype=torch.float64, device="cuda")
    pl = mdl.oc_pdp_grad(u, th, dxm, dum, skip_missing=True, buffers={"grad": gbuf[:B]}, **traj())
    assert pl["grad"].data_ptr() == gbuf.data_ptr()
    pkbuf = torch.full((B + 1, p + 1), nan, dtype=torch.float64, device="cuda")
    pk = mdl.oc_pdp_grad(u, th, dxm, dum, skip_missing=True, packed=True, buffers={"packed": pkbuf[:B]}, **traj())
    assert pk["packed"].data_ptr() == pkbuf.data_ptr()
    npy = lambda t: t.detach().cpu().numpy()
    return dict(rows=npy(rows), loss=npy(g["loss"]), status=npy(g["status"]), x=npy(g["x"]), lam=npy(g["lam"]),
                plain_grad=npy(gbuf), plain_loss=npy(pl["loss"]), plain_status=npy(pl["status"]), plain_x=npy(pl["x"]), plain_lam=npy(pl["lam"]),
                packed=npy(pkbuf), packed_loss=npy(pk["loss"]), packed_status=npy(pk["status"]), packed_x=npy(pk["x"]), packed_lam=npy(pk["lam"]),
                loss_ref=npy(loss_ref), grad_ref=npy(grad_ref), G_ref=npy(G_ref), status0=npy(d0["status"]), x_def=npy(d0["x"]), lam_def=npy(d0["lam"]),
                noflag_loss=npy(d0["loss"]), noflag_grad=npy(d0["grad"]), noflag_rows=npy(g0["packed_gn"]))


def rel(a, b):
    """max|a - b| / max|b| of one sample's array (a scalar: |a - b| / |b|)"""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.abs(a - b).max() / np.abs(b).max())
