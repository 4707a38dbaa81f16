"""Shared by the host tests of the least-squares rows (tests/test_ls_rows_host.py, tests/test_sysid_gn_host.py, tests/sysid_ini_common.py): the stand-ins that let
ModelLib's marshalling run without a GPU - a recorder for the foreign library, torch on the CPU under the names the runtime uses - and the FROZEN restatement of the five
expressions that formed the packed row grad [W] | loss | G [W][W] from materialised sensitivities before runtime.packed_row_from_sensitivities replaced them."""
import numpy as np


class Recorder:
    """stands in for the foreign library: records every call and answers 0"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*args):
            self.calls.append((name, args))
            return 0
        return f


def stand_in_torch(monkeypatch):
    """No GPU: runtime.torch_cuda() answers torch itself with the factories' device argument dropped (and empty as zeros: what a recorder leaves behind is finite),
    runtime.dev keeps tensors and converts the rest on the CPU, the stream pointer is None.  Returns the stand-in."""
    import torch
    from pdp_amd import runtime

    def on_cpu(f):
        return lambda *a, device=None, **kw: f(*a, **kw)

    class _Cuda:
        is_current_stream_capturing = staticmethod(lambda: False)

    class _Torch:
        cuda = _Cuda

        def __getattr__(self, name):
            if name in ("empty", "zeros", "ones", "full", "tensor", "as_tensor"):
                return on_cpu(getattr(torch, "zeros" if name == "empty" else name))
            return getattr(torch, name)
    stand_in = _Torch()
    monkeypatch.setattr(runtime, "torch_cuda", lambda: stand_in)
    monkeypatch.setattr(runtime, "dev", lambda a: a if hasattr(a, "data_ptr") else torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=float))))
    monkeypatch.setattr(runtime, "current_stream_ptr", lambda: None)
    return stand_in


def stand_in_model(n=4, m=1, p=3):
    """a ModelLib without a library: its sizes and a Recorder"""
    from pdp_amd import runtime
    mdl = runtime.ModelLib.__new__(runtime.ModelLib)
    mdl.n, mdl.m, mdl.p, mdl.lib = n, m, p, Recorder()
    return mdl


# ---- the frozen reference: the five expressions as they stood in runtime.py, verbatim but for the names of their inputs (CPU tensors; zero / one: 0-dim fp64) ----------
def sysid_gn(packed, x, xobs, X, W):
    import torch
    B = x.shape[0]
    d = x - xobs
    packed[:, W] = (d * d).sum(dim=(1, 2))
    packed[:, :W] = torch.einsum("bti,btip->bp", d, X)
    packed[:, W + 1:] = torch.einsum("btip,btiq->bpq", X, X).reshape(B, W * W)


def sysid_gn_skip_missing(packed, x, xobs, X, W):
    import torch
    B = x.shape[0]
    d = x - xobs
    zero = torch.zeros((), dtype=torch.float64)
    packed[:, W] = torch.where(xobs == xobs, d * d, zero).sum(dim=(1, 2))
    obs = d == d
    d, X = torch.where(obs, d, zero), torch.where(obs[..., None], X, zero)
    packed[:, :W] = torch.einsum("bti,btip->bp", d, X)
    packed[:, W + 1:] = torch.einsum("btip,btiq->bpq", X, X).reshape(B, W * W)


def sysid_weighted(packed, x, xobs, X, W, wd, delta, skip_missing):
    import torch
    B, R, n = xobs.shape
    zero = torch.zeros((), dtype=torch.float64)
    wf = (wd if wd is not None else torch.ones((), dtype=torch.float64)).expand(B, R, n)
    d = x - xobs
    obs = (wf > 0) & (xobs == xobs) if skip_missing else wf > 0
    e = wf.sqrt() * d
    ae = e.abs()
    quad = ae <= delta
    s = torch.where(quad, wf, wf * (delta / ae)).sqrt()
    packed[:, W] = torch.where(obs, torch.where(quad, e * e, 2.0 * delta * ae - delta * delta), zero).sum(dim=(1, 2))
    sd = torch.where(obs, s * d, zero)
    sX = torch.where((obs & (s != 0))[..., None], s[..., None] * X, zero)
    packed[:, :W] = torch.einsum("bti,btip->bp", sd, sX)
    packed[:, W + 1:] = torch.einsum("btip,btiq->bpq", sX, sX).reshape(B, W * W)


def oc_gn_skip_missing(pk, x, u, demo_x, demo_u, dxdp, dudp, p):
    import torch
    B = x.shape[0]
    loss, grad = torch.empty(B, dtype=torch.float64), pk[:, :p]
    wx, wu = ~torch.isnan(demo_x), ~torch.isnan(demo_u)
    zero = torch.zeros((), dtype=torch.float64)
    ex, eu = torch.where(wx, x - demo_x, zero), torch.where(wu, u - demo_u, zero)
    loss.copy_((ex ** 2).sum(dim=(1, 2)) + (eu ** 2).sum(dim=(1, 2)))
    dxdp, dudp = torch.where(wx[..., None], dxdp, zero), torch.where(wu[..., None], dudp, zero)
    grad.copy_(torch.einsum("bti,btip->bp", ex, dxdp) + torch.einsum("bti,btip->bp", eu, dudp))
    pk[:, p].copy_(loss)
    pk[:, p + 1:].copy_((torch.einsum("btip,btiq->bpq", dxdp, dxdp) + torch.einsum("btip,btiq->bpq", dudp, dudp)).reshape(B, p * p))


def oc_weighted(pk, x, u, demo_x, demo_u, dxdp, dudp, p, wxd, wud, delta, skip_missing):
    import torch
    B = x.shape[0]
    loss = torch.empty(B, dtype=torch.float64)
    zero, one = torch.zeros((), dtype=torch.float64), torch.ones((), dtype=torch.float64)

    def side(v, demo, w, S):
        wf = (w if w is not None else one).expand(*demo.shape)
        d = v - demo
        obs = (wf > 0) & (demo == demo) if skip_missing else wf > 0
        e = wf.sqrt() * d
        ae = e.abs()
        quad = ae <= delta
        s = torch.where(quad, wf, wf * (delta / ae)).sqrt()
        rho = torch.where(obs, torch.where(quad, e * e, 2.0 * delta * ae - delta * delta), zero).sum(dim=(1, 2))
        return rho, torch.where(obs, s * d, zero), torch.where((obs & (s != 0))[..., None], s[..., None] * S, zero)
    lx, sdx, sX = side(x, demo_x, wxd, dxdp)
    lu, sdu, sU = side(u, demo_u, wud, dudp)
    loss.copy_(lx + lu)
    pk[:, p].copy_(loss)
    pk[:, :p].copy_(torch.einsum("bti,btip->bp", sdx, sX) + torch.einsum("bti,btip->bp", sdu, sU))
    pk[:, p + 1:].copy_((torch.einsum("btip,btiq->bpq", sX, sX) + torch.einsum("btip,btiq->bpq", sU, sU)).reshape(B, p * p))
