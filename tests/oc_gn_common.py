"""Shared by tests/test_gpu_oc_gn.py (in-process and in its child processes): one shape of the Gauss-Newton mode through every call it is compared with.  Inputs:
tests/oc_vjp_common.make_inputs."""
import numpy as np


def evaluate(mdl, inp, per_sample=False, given=False):
    """The default unit (plain, and with the sensitivities written) and the Gauss-Newton unit on the same inputs.  given: the Gauss-Newton call gets the default call's
    (x, lam) (PDP_OC_GIVEN_TRAJ), else it rolls out from x0.  The packed rows are pre-filled with NaN and followed by one guard row.  Returns numpy arrays;
    G_ref = einsum(dxdp, dxdp) + einsum(dudp, dudp) in torch fp64."""
    import torch
    from pdp_amd import runtime as rt
    th = inp["theta_b"] if per_sample else inp["theta"]
    u, x0, demo_x, demo_u = rt.dev(inp["u"]), inp["x0"], rt.dev(inp["demo_x"]), rt.dev(inp["demo_u"])
    B, p = u.shape[0], mdl.p
    d0 = mdl.oc_pdp_grad(u, th, demo_x, demo_u, x0=x0)
    ds = mdl.oc_pdp_grad(u, th, demo_x, demo_u, x0=x0, want_sens=True)
    G_ref = torch.einsum("btip,btiq->bpq", ds["dxdp"], ds["dxdp"]) + torch.einsum("btip,btiq->bpq", ds["dudp"], ds["dudp"])
    rows = torch.full((B + 1, p + 1 + p * p), float("nan"), dtype=torch.float64, device="cuda")
    traj = dict(x=d0["x"].clone(), lam=d0["lam"].clone()) if given else dict(x0=x0)
    g = mdl.oc_pdp_grad(u, th, demo_x, demo_u, gauss_newton=True, buffers={"packed_gn": rows[:B]}, **traj)
    assert g["packed_gn"].data_ptr() == rows.data_ptr() and g["gn"].shape == (B, p, p) and g["grad"].shape == (B, p)
    assert torch.equal(g["gn"].reshape(B, -1), rows[:B, p + 1:]) and torch.equal(g["grad"], rows[:B, :p])
    npy = lambda t: t.detach().cpu().numpy()
    return dict(rows=npy(rows), loss=npy(g["loss"]), G_ref=npy(G_ref), status=npy(g["status"]), status0=npy(d0["status"]), x=npy(g["x"]), x_def=npy(d0["x"]),
                lam=npy(g["lam"]), lam_def=npy(d0["lam"]), grad_def=npy(d0["grad"]), loss_def=npy(d0["loss"]))


def rel_per_sample(a, b):
    """max_b  max|a_b - b_b| / max|b_b|"""
    a, b = np.asarray(a), np.asarray(b)
    return max(np.abs(a[i] - b[i]).max() / np.abs(b[i]).max() for i in range(a.shape[0]))
