"""ctypes binding of the C-ABI in include/*.h + torch tensor plumbing (device memory, streams).  abi.py mirrors the headers (structures, constants, the table of entry
points); the structures, PDP_E and LM_STATES are re-exported here for the callers that always found them here.

PyTorch is used for HBM allocation / stream handles only; every arithmetic result of the hot path comes
from the HIP kernels in libpdp_hip.so / libpdp_model_*.so.  There is NO CPU fallback: if the shared
library is missing or the GPU is absent, calls raise (RuntimeError) instead of silently computing elsewhere.
"""
import ctypes as C
import os

import numpy as np

from .abi import (LM_STATES, PDP_E, PDP_E_SIZE, PDP_GRAD_GAUSS_NEWTON, PDP_GRAD_SKIP_MISSING, PDP_MS_FROM_CONTROLS, PDP_MS_NO_RESTORATION,  # noqa: F401
                  PDP_MS_PREDICT, PDP_MS_PREDICT_GUARD, PDP_MS_PREDICT_PRIMAL, PDP_MS_WARM, PDP_MS_WITH_SOC, PDP_MS_WITH_WATCHDOG, PDP_OC_COTANGENT, PDP_OC_GIVEN_TRAJ,
                  PDP_OC_PACKED, PDP_OC_RECORD_PRIMAL, PDP_POLICY_COTANGENT, PDP_POLICY_MLP, PDP_POLICY_POLY, PDP_POLICY_TABLE, PDP_POLICY_TANGENT, PdpLmPrior, PdpLmSchedule, PdpLmState, PdpLqrProblem, PdpMat,
                  PdpModelInfo, PdpOcAuxsys, PdpOcMsOpts, PdpOcSensOut, PdpOcSolveOpts, PdpPolicy, PdpPolicyCot, PdpPolicyTan, entry_points)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(_HERE, "lib")
CORE_LIB = os.path.join(LIB_DIR, "libpdp_hip.so")

_core = None


def _dlopen(path):
    """dlopen one of our libraries AFTER torch, so that its libamdhip64.so.7 dependency resolves to the HIP runtime
    torch already loaded (one runtime per process; loading /opt/rocm's copy first leaves torch without a device)."""
    import torch  # noqa: F401
    return C.CDLL(path)


def check(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed: %s" % (what, PDP_E.get(rc, rc)))


def load_core():
    """dlopen libpdp_hip.so (built by __graft_entry__.build()); raises if it is not there."""
    global _core
    if _core is None:
        if not os.path.exists(CORE_LIB):
            raise RuntimeError("libpdp_hip.so not built (%s): run `python -c 'import __graft_entry__ as g; g.build()'`; "
                               "there is no CPU fallback" % CORE_LIB)
        lib = _dlopen(CORE_LIB)
        for name, (res, args) in entry_points(library="core").items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _core = lib
    return _core


def gd_update(loss, grad, lr, theta, dtheta, counters, status=None, converged=None, iterations=None, loss_trace=None, parameter_trace=None):
    """theta <- theta - lr * mean gradient with traces and health counters, one launch (pdp_gd_update_batched).  loss [B], grad [B, p] (rows may be strided: a view of
    the packed [B, p + 1] output), theta / dtheta [p] fp64, counters int64 [4] = (iterations done, unconverged solves, numerical trouble, Newton iterations);
    status / converged / iterations: int32 [B] or None."""
    torch = torch_cuda()
    B, p = grad.shape
    assert loss.dtype == torch.float64 and grad.dtype == torch.float64 and grad.stride(1) == 1 and loss.is_contiguous() and counters.dtype == torch.int64 and counters.numel() >= 4
    for t in (status, converged, iterations):
        assert t is None or (t.dtype == torch.int32 and t.is_contiguous() and t.numel() == B)
    assert theta.dtype == torch.float64 and theta.numel() == p and dtheta.numel() == p and theta.is_contiguous() and dtheta.is_contiguous()
    tl = 0
    if loss_trace is not None:
        tl = loss_trace.shape[0]
        assert loss_trace.is_contiguous() and (parameter_trace is None or (parameter_trace.is_contiguous() and tuple(parameter_trace.shape) == (tl, p)))
    elif parameter_trace is not None:
        tl = parameter_trace.shape[0]
        assert parameter_trace.is_contiguous() and parameter_trace.shape[1] == p
    check(load_core().pdp_gd_update_batched(B, p, ptr(loss), ptr(grad), int(grad.stride(0)), ptr(status), ptr(converged), ptr(iterations), float(lr), ptr(theta), ptr(dtheta),
                                            ptr(loss_trace), ptr(parameter_trace), int(tl), ptr(counters), current_stream_ptr()), "pdp_gd_update_batched")


def _lm_structs(theta, trial, lam, current, state, evaluations, rejected, accepted, counters, up, down, lam_min, lam_max, loss_tol, max_evals, bad, accepted_now,
                loss_trace, lambda_trace, parameter_trace):
    """the checks of the state buffers of lm_update / lm_update_prior and the two structs of include/pdp_hip_lm.h: (PdpLmSchedule, PdpLmState)"""
    torch = torch_cuda()
    K, p = theta.shape
    assert trial.dim() == 2 and trial.shape[1] == p and trial.shape[0] % K == 0
    S, w = trial.shape[0] // K, p + 1 + p * p
    for t, shape in ((theta, (K, p)), (trial, (K * S, p)), (lam, (K,)), (current, (K, w))):
        assert t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == shape
    for t in (state, evaluations, rejected, accepted):
        assert t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == (K,)
    for t in (bad, accepted_now):
        assert t is None or (t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == (K * S,))
    assert counters.dtype == torch.int64 and counters.is_contiguous() and counters.numel() >= 2
    L = next((int(t.shape[1]) for t in (loss_trace, lambda_trace, parameter_trace) if t is not None), 0)
    for t, shape in ((loss_trace, (K, L)), (lambda_trace, (K, L)), (parameter_trace, (K, L, p))):
        assert t is None or (t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == shape)
    sch = PdpLmSchedule(float(up), float(down), float(lam_min), float(lam_max), float(loss_tol), int(max_evals))
    st = PdpLmState(*[t.data_ptr() if t is not None else None for t in (theta, trial, lam, current, state, evaluations, rejected, accepted, accepted_now, loss_trace,
                                                                         lambda_trace, parameter_trace)], L, counters.data_ptr())
    return sch, st


def lm_update(rows, theta, trial, lam, current, state, evaluations, rejected, accepted, counters, up=10.0, down=10.0, lam_min=1e-12, lam_max=1e8, loss_tol=0.0,
              max_evals=50, bad=None, accepted_now=None, loss_trace=None, lambda_trace=None, parameter_trace=None):
    """One Levenberg-Marquardt update of K independent problems, one launch (pdp_lm_update_batched, include/pdp_hip_lm.h: the semantics).  rows [K S, p + 1 + p p] =
    grad | loss | G per sample, evaluated at `trial` (rows may be strided: a view of a wider buffer); the state at fixed device addresses, initialised by the caller:
    theta [K, p], trial [K S, p], lam [K], current [K, p + 1 + p p] fp64; state, evaluations, rejected, accepted int32 [K]; counters int64 [2] = launches done |
    problems still START or ACTIVE (initialised 0 | K).  Optional: bad int32 [K S], accepted_now int32 [K S], loss_trace / lambda_trace [K, L], parameter_trace [K, L, p]."""
    torch = torch_cuda()
    sch, st = _lm_structs(theta, trial, lam, current, state, evaluations, rejected, accepted, counters, up, down, lam_min, lam_max, loss_tol, max_evals, bad, accepted_now,
                          loss_trace, lambda_trace, parameter_trace)
    K, p = theta.shape
    S, w = trial.shape[0] // K, p + 1 + p * p
    assert rows.dtype == torch.float64 and rows.dim() == 2 and tuple(rows.shape) == (K * S, w) and rows.stride(1) == 1 and rows.stride(0) >= w
    check(load_core().pdp_lm_update_batched(K, S, p, ptr(rows), int(rows.stride(0)), ptr(bad), C.byref(sch), C.byref(st), current_stream_ptr()), "pdp_lm_update_batched")


def lm_prior_shapes(prior_mean, prior_precision, K, p, diagonal_per_problem=False):
    """(kind, mean_kstride, precision_kstride) of a prior from its shapes (tuples): mean [p] or [K, p]; precision [p] (diagonal, shared), [p, p] (full, shared), [K, p]
    (diagonal, per problem) or [K, p, p] (full, per problem).  Where K == p, [p, p] is the shared full matrix unless diagonal_per_problem says otherwise.  Anything else
    is a ValueError."""
    ms, ps = tuple(int(v) for v in prior_mean), tuple(int(v) for v in prior_precision)
    if ms not in ((p,), (K, p)):
        raise ValueError("prior_mean is [p] = [%d] or [K, p] = [%d, %d], got %s" % (p, K, p, list(ms)))
    table = {(p,): (0, 0), (p, p): (1, 0), (K, p, p): (1, p * p)}
    if diagonal_per_problem:
        table[(K, p)] = (0, p)
    table.setdefault((K, p), (0, p))
    if ps not in table:
        raise ValueError("prior_precision is [p], [p, p], [K, p] or [K, p, p] with K = %d, p = %d, got %s" % (K, p, list(ps)))
    kind, pks = table[ps]
    return kind, (p if len(ms) == 2 else 0), pks


def lm_update_prior(rows, theta, trial, lam, current, state, evaluations, rejected, accepted, counters, up=10.0, down=10.0, lam_min=1e-12, lam_max=1e8, loss_tol=0.0,
                    max_evals=50, bad=None, accepted_now=None, loss_trace=None, lambda_trace=None, parameter_trace=None, prior_mean=None, prior_precision=None,
                    prior_loss=None, diagonal_per_problem=False):
    """lm_update with a Gaussian prior (x - mean)' P (x - mean) on the unknowns of every problem, added to the MEAN row inside the update launch
    (pdp_lm_update_prior_batched, include/pdp_hip_lm_prior.h: the semantics).  prior_mean [p] or [K, p]; prior_precision [p] / [K, p] (the diagonal) or [p, p] /
    [K, p, p] (full; where K == p, [p, p] is the shared full matrix unless diagonal_per_problem is set), shared by all problems or one per problem by its shape; prior_loss [K] or None: the prior's share of the loss at the accepted
    point.  All fp64, contiguous, on the device.  Without prior_mean and prior_precision the launch is pdp_lm_update_batched's, through the new entry point."""
    torch = torch_cuda()
    assert rows.dtype == torch.float64 and rows.dim() == 2 and rows.stride(1) == 1
    sch, st = _lm_structs(theta, trial, lam, current, state, evaluations, rejected, accepted, counters, up, down, lam_min, lam_max, loss_tol, max_evals, bad, accepted_now,
                          loss_trace, lambda_trace, parameter_trace)
    K, p = theta.shape
    S, w = trial.shape[0] // K, p + 1 + p * p
    assert tuple(rows.shape) == (K * S, w) and rows.stride(0) >= w
    prior = None
    if prior_mean is not None or prior_precision is not None:
        if prior_mean is None or prior_precision is None:
            raise ValueError("lm_update_prior: prior_mean and prior_precision go together")
        kind, mks, pks = lm_prior_shapes(prior_mean.shape, prior_precision.shape, K, p, diagonal_per_problem)
        for t in (prior_mean, prior_precision):
            assert t.dtype == torch.float64 and t.is_contiguous() and t.is_cuda
        assert prior_loss is None or (prior_loss.dtype == torch.float64 and prior_loss.is_contiguous() and tuple(prior_loss.shape) == (K,))
        prior = C.byref(PdpLmPrior(prior_mean.data_ptr(), prior_precision.data_ptr(), kind, mks, pks, prior_loss.data_ptr() if prior_loss is not None else None))
    else:
        assert prior_loss is None
    check(load_core().pdp_lm_update_prior_batched(K, S, p, ptr(rows), int(rows.stride(0)), ptr(bad), C.byref(sch), C.byref(st), prior, current_stream_ptr()),
          "pdp_lm_update_prior_batched")


def lm_covariance(rows, scale=None):
    """The covariance of K estimates, one launch (pdp_lm_covariance_batched): rows [K, p + 1 + p p] = grad | loss | G per problem (BatchedLMLoop.current; rows may be
    strided), scale [K] or None (1).  Returns dict(cov [K, p, p] = scale G^-1 as computed - not symmetrised, std_err [K, p], pivot_ratio [K], status int32 [K]: 0, or 1
    where G is singular to the elimination or holds a non-finite entry - cov and std_err of that problem NaN, pivot_ratio 0), device tensors."""
    torch = torch_cuda()
    assert rows.dtype == torch.float64 and rows.dim() == 2 and rows.stride(1) == 1 and rows.is_cuda
    K, w = (int(v) for v in rows.shape)
    p = int(round((-1.0 + (1.0 + 4.0 * (w - 1)) ** 0.5) / 2.0))
    assert p >= 1 and p + 1 + p * p == w and rows.stride(0) >= w, "rows is [K, p + 1 + p p]"
    assert scale is None or (scale.dtype == torch.float64 and scale.is_contiguous() and tuple(scale.shape) == (K,) and scale.is_cuda)
    cov, std = torch.empty((K, p, p), dtype=torch.float64, device="cuda"), torch.empty((K, p), dtype=torch.float64, device="cuda")
    ratio, status = torch.empty((K,), dtype=torch.float64, device="cuda"), torch.empty((K,), dtype=torch.int32, device="cuda")
    check(load_core().pdp_lm_covariance_batched(K, p, ptr(rows), int(rows.stride(0)), ptr(scale), ptr(cov), ptr(std), ptr(ratio), ptr(status), current_stream_ptr()),
          "pdp_lm_covariance_batched")
    return dict(cov=cov, std_err=std, pivot_ratio=ratio, status=status)


def count_observed(data, weights=None, skip_missing=False, first_row=True):
    """The number of entries of data [B, R, n] that enter a weighted / partially observed sum-of-squares loss, per trajectory: int64 [B] on the device of `data` (a torch
    expression: CPU tensors included).  An entry counts iff its weight is > 0 (weights None: 1; [n], [R, n] or [B, R, n]) and, under skip_missing, it is not NaN.
    first_row: True - row 0 counts like the others; False - it does not (a state row 0 that is the rollout's own initial state: its residual is identically zero); a bool
    mask [n] - row 0 counts in these components only (the estimated components of the initial state)."""
    import torch
    data = torch.as_tensor(data)
    B, R, n = (int(v) for v in data.shape)
    on = torch.ones((B, R, n), dtype=torch.bool, device=data.device)
    if weights is not None:
        on = on & (torch.as_tensor(weights, device=data.device) > 0).expand(B, R, n)
    if skip_missing:
        on = on & ~torch.isnan(data)
    if first_row is not True:
        keep = torch.zeros(n, dtype=torch.bool, device=data.device) if first_row is False else torch.as_tensor(first_row, dtype=torch.bool, device=data.device).reshape(n)
        on = torch.cat([on[:, :1] & keep, on[:, 1:]], dim=1)
    return on.sum(dim=(1, 2))


def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("no MI355X visible (torch.cuda.is_available() is False): the PDP kernels need a GPU, there is no CPU fallback")
    return torch


def current_stream_ptr():
    torch = torch_cuda()
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a, device=None):
    """numpy / list / tensor -> contiguous fp64 CUDA tensor."""
    torch = torch_cuda()
    if isinstance(a, torch.Tensor):
        return a.to(device=device or "cuda", dtype=torch.float64).contiguous()
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=np.float64)), device=device or "cuda")


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(None)


def _shape_of(a):
    return tuple(int(k) for k in (a.shape if hasattr(a, "shape") else np.shape(a)))


SWEEP_POOL_DOUBLES = 2400       # csrc/pdp_sweep_pool.h: the pool of the sweep kernels beyond four trajectories per compute unit


def _mat(t, B, time_varying):
    """tensor [B?,T?,r,c] -> PdpMat with zero strides on broadcast axes."""
    if t is None:
        return PdpMat(None, 0, 0), None
    t = dev(t)
    r, c = t.shape[-2], t.shape[-1]
    if time_varying:
        if t.dim() == 4:
            bs, ts = (t.shape[1] * r * c if t.shape[0] > 1 else 0), (r * c if t.shape[1] > 1 else 0)
        elif t.dim() == 3:
            bs, ts = 0, (r * c if t.shape[0] > 1 else 0)
        else:
            bs, ts = 0, 0
    else:
        bs, ts = (r * c if (t.dim() == 3 and t.shape[0] > 1) else 0), 0
    return PdpMat(t.data_ptr(), bs, ts), t


def lqr_solve(F, G, Hxx, Huu, hxx, hxe, E=None, Hxu=None, Hxe=None, Hue=None, X0=None, T=None, want_costate=True):
    """Batched LQR.lqrSolver.  Time-varying families are [B,T,r,c] (or [T,r,c] shared over the batch, or [r,c]
    time-invariant); terminal / initial ones [B,r,c] or [r,c].  Returns (X [B,T+1,n,p], U [B,T,m,p], Lam or None, status [B])."""
    torch = torch_cuda()
    lib = load_core()
    keep = []
    F_t = dev(F)
    n = F_t.shape[-1]
    G_t = dev(G)
    m = G_t.shape[-1]
    hxe_t = dev(hxe)
    p = hxe_t.shape[-1]
    B = 1
    for a in (F_t, G_t):
        if a.dim() == 4:
            B = max(B, a.shape[0])
    for a in (hxe_t, dev(hxx)) + ((dev(X0),) if X0 is not None else ()):
        if a.dim() == 3:
            B = max(B, a.shape[0])
    if T is None:
        T = F_t.shape[-3] if F_t.dim() >= 3 else None
    assert T is not None, "horizon T is required for time-invariant problems"
    pr = PdpLqrProblem()
    pr.B, pr.T, pr.n, pr.m, pr.p = B, int(T), n, m, p
    for name, val, tv in (("F", F_t, True), ("G", G_t, True), ("E", E, True), ("Hxx", Hxx, True), ("Hxu", Hxu, True), ("Hxe", Hxe, True),
                          ("Huu", Huu, True), ("Hue", Hue, True), ("hxx", hxx, False), ("hxe", hxe_t, False), ("X0", X0, False)):
        mat, t = _mat(val, B, tv)
        setattr(pr, name, mat)
        keep.append(t)
    # parameter columns one launch carries: 4 tiles of 16 (the first shared with the controls) in the tile kernels, 32 in the generic one
    pmax = 64 - m if (n <= 16 and m <= 4) else 32
    if p > pmax:
        # more columns than the kernel's tiles hold (a neural policy's auxvar, a wide X0): the columns of (E, Hxe, Hue, hxe, X0) -> (X, U, Lam)
        # are independent given the gains, so the problem is solved in column blocks (each launch repeats the n x n backward recursion)
        cut = lambda a, c0, c1: None if a is None else dev(a)[..., c0:c1].contiguous()
        parts = [lqr_solve(F_t, G_t, Hxx, Huu, hxx, cut(hxe_t, c0, min(p, c0 + pmax)), E=cut(E, c0, min(p, c0 + pmax)), Hxu=Hxu, Hxe=cut(Hxe, c0, min(p, c0 + pmax)),
                           Hue=cut(Hue, c0, min(p, c0 + pmax)), X0=cut(X0, c0, min(p, c0 + pmax)), T=T, want_costate=want_costate) for c0 in range(0, p, pmax)]
        status = parts[0][3]
        for q in parts[1:]:
            status = status | q[3]
        return (torch.cat([q[0] for q in parts], dim=-1), torch.cat([q[1] for q in parts], dim=-1),
                torch.cat([q[2] for q in parts], dim=-1) if want_costate else None, status)
    X = torch.empty((B, T + 1, n, p), dtype=torch.float64, device="cuda")
    U = torch.empty((B, T, m, p), dtype=torch.float64, device="cuda")
    Lam = torch.empty((B, T, n, p), dtype=torch.float64, device="cuda") if want_costate else None
    status = torch.zeros((B,), dtype=torch.int32, device="cuda")
    nbytes = lib.pdp_lqr_workspace_bytes(B, T, n, m, p, 1 if want_costate else 0)
    ws = torch.empty((max(nbytes, 8) // 8,), dtype=torch.float64, device="cuda")
    rc = lib.pdp_lqr_solve_batched(C.byref(pr), ptr(X), ptr(U), ptr(Lam), ptr(status), ptr(ws), nbytes, current_stream_ptr())
    check(rc, "pdp_lqr_solve_batched")
    return X, U, Lam, status


def cp_aux_integrate(F, G, Ux, Ue, X0=None):
    torch = torch_cuda()
    lib = load_core()
    F, G, Ux, Ue = dev(F), dev(G), dev(Ux), dev(Ue)
    B, T, n, _ = F.shape
    m, p = Ue.shape[-2], Ue.shape[-1]
    X0 = dev(X0) if X0 is not None else None
    X = torch.empty((B, T + 1, n, p), dtype=torch.float64, device="cuda")
    U = torch.empty((B, T, m, p), dtype=torch.float64, device="cuda")
    check(lib.pdp_cp_aux_integrate_batched(B, T, n, m, p, ptr(F), ptr(G), ptr(Ux), ptr(Ue), ptr(X0), ptr(X), ptr(U), current_stream_ptr()),
          "pdp_cp_aux_integrate_batched")
    return X, U


def sysid_aux_integrate(F, E, X0=None):
    torch = torch_cuda()
    lib = load_core()
    F, E = dev(F), dev(E)
    B, T, n, _ = F.shape
    p = E.shape[-1]
    X0 = dev(X0) if X0 is not None else None
    X = torch.empty((B, T + 1, n, p), dtype=torch.float64, device="cuda")
    check(lib.pdp_sysid_aux_integrate_batched(B, T, n, p, ptr(F), ptr(E), ptr(X0), ptr(X), current_stream_ptr()),
          "pdp_sysid_aux_integrate_batched")
    return X


def ini_indices(estimate_ini, n):
    """The estimated components of an initial state, normalised: estimate_ini is None, a bool mask [n] or ascending unique state indices; returns (indices as a list
    of int, the bit mask of pdp_sysid_step_gn_ini_batched).  Duplicates, indices out of range or not ascending, and a mask of another length are a ValueError."""
    if estimate_ini is None:
        return [], 0
    a = np.asarray(estimate_ini.cpu() if hasattr(estimate_ini, "cpu") else estimate_ini)
    if a.dtype == bool:
        if a.shape != (n,):
            raise ValueError("estimate_ini: a bool mask has one entry per state component (%d), got shape %s" % (n, a.shape))
        idx = [int(i) for i in np.flatnonzero(a)]
    else:
        a = a.reshape(-1)
        if a.size and not np.issubdtype(a.dtype, np.integer):
            raise ValueError("estimate_ini: state indices (integers) or a bool mask [n]")
        idx = [int(i) for i in a]
        if any(i < 0 or i >= n for i in idx):
            raise ValueError("estimate_ini: state index out of range 0 .. %d: %s" % (n - 1, idx))
        if len(set(idx)) != len(idx):
            raise ValueError("estimate_ini: duplicate state index: %s" % idx)
        if idx != sorted(idx):
            raise ValueError("estimate_ini: state indices in ascending order (unknown p + k is the k-th of them): %s" % idx)
    return idx, sum(1 << i for i in idx)


def refuse_nan_initial_state(who, data, ini_state, name):
    """skip_missing: a NaN in the initial state that would be used - ini_state, else data[:, 0] - is a ValueError before any launch, in the name of the caller `who`
    (`name`: what it calls `data`).  Judged on what the caller gave (a host array is not moved to the device first)."""
    first = ini_state if ini_state is not None else (data if hasattr(data, "data_ptr") else np.asarray(data, dtype=float))[:, 0]
    if bool(first.isnan().any()) if hasattr(first, "data_ptr") else bool(np.isnan(np.asarray(first, dtype=float)).any()):
        raise ValueError("%s: skip_missing=True and the initial state (%s) holds a NaN: give ini_state [B, n]" % (who, "%s[:, 0]" % name if ini_state is None else "ini_state"))


def _huber_threshold(huber_delta):
    """huber_delta as a float, +inf for off (None); not > 0 is a ValueError"""
    delta = float("inf") if huber_delta is None else float(huber_delta)
    if not delta > 0.0:
        raise ValueError("huber_delta: a threshold > 0 (None: plain least squares), got %r" % (huber_delta,))
    return delta


def _weight_block(w, name, B, rows, k, rows_text, letter):
    """One block of weights, checked on what the caller gave (a host array is not moved to the device first): (the weights as given but shaped [rows, k] or
    [B, rows, k], or None; their batch stride).  They broadcast from [k], [rows, k] or [B, rows, k]; a negative or non-finite weight or another shape is a ValueError
    in the name of the keyword (`rows_text` and `letter`: how the message spells rows and k)."""
    if w is None:
        return None, 0
    w = w if hasattr(w, "data_ptr") else np.asarray(w, dtype=float)
    shape = tuple(w.shape)
    if shape not in ((k,), (rows, k), (B, rows, k)):
        raise ValueError("%s: shape [%s], [%s, %s] or [B, %s, %s] = (%d,), (%d, %d) or (%d, %d, %d), got %s"
                         % (name, letter, rows_text, letter, rows_text, letter, k, rows, k, B, rows, k, shape))
    if not bool(((w >= 0) & (w < float("inf"))).all()):          # (a NaN fails the comparison)
        raise ValueError("%s: finite and >= 0 (0: the entry is not observed)" % name)
    if len(shape) == 1:
        w = w.expand(rows, k) if hasattr(w, "data_ptr") else np.broadcast_to(w, (rows, k))
    return w, (0 if len(w.shape) == 2 else rows * k)


def wls_arguments(weights, huber_delta, B, T, n):
    """The weights and Huber's threshold of pdp_sysid_step_wls_batched, normalised and checked on what the caller gave (a host array is not moved to the device first):
    returns (weights as given but shaped [T+1, n] or [B, T+1, n], or None; weights_bstride; delta as a float, +inf for off).  weights broadcast from [n], [T+1, n] or
    [B, T+1, n]; a negative or non-finite weight, another shape, or a huber_delta that is not > 0 is a ValueError before any launch.  ModelLib.sysid_rows_prepared
    calls it once for many evaluations."""
    delta = _huber_threshold(huber_delta)
    return _weight_block(weights, "weights", B, T + 1, n, "T+1", "n") + (delta,)


def oc_wls_arguments(weights_x, weights_u, huber_delta, B, T, n, m):
    """The weights and Huber's threshold of pdp_oc_pdp_grad_wls_batched, normalised and checked on what the caller gave, in the spirit of wls_arguments: returns
    (weights_x shaped [T+1, n] or [B, T+1, n], or None; its batch stride; weights_u shaped [T, m] or [B, T, m], or None; its batch stride; delta as a float, +inf for
    off).  weights_x broadcasts from [n], [T+1, n] or [B, T+1, n], weights_u from [m], [T, m] or [B, T, m]; a negative or non-finite weight, another shape, or a
    huber_delta that is not > 0 is a ValueError before any launch.  ModelLib.oc_rows_prepared calls it once for many evaluations."""
    delta = _huber_threshold(huber_delta)
    return _weight_block(weights_x, "weights_x", B, T + 1, n, "T+1", "n") + _weight_block(weights_u, "weights_u", B, T, m, "T", "m") + (delta,)


def _buffer(bufs, key, shape, dtype=None):
    """The tensor `key` of a caller's dict of buffers (outputs and workspaces reused between calls) in the asked shape and dtype (None: fp64): allocated when it is
    not there, again when the shape changed"""
    t = bufs.get(key)
    if t is None or tuple(t.shape) != tuple(shape):
        torch = torch_cuda()
        t = bufs[key] = torch.empty(shape, dtype=torch.float64 if dtype is None else dtype, device="cuda")
    return t


def packed_row_from_sensitivities(packed, sides, rule, delta=float("inf"), skip_missing=False):
    """The packed row grad [W] | loss | G [W][W] of a sum-of-squares loss from MATERIALISED sensitivities, written into packed [B, W + 1 + W W]: what the fused
    least-squares entry points write themselves within their tiles, for the problems beyond them (PDP_E_SIZE).  sides: a list of (values [B, R, k], data [B, R, k],
    weights broadcastable to [B, R, k] or None, sensitivities [B, R, k, W]) - the states for SysID.step, states and controls for the OC unit; their losses, gradients
    and matrices add up.  rule, always as selects - never a product with 0:
      "plain"             every entry counts;
      "missing_residual"  SysID's skip_missing: the loss leaves out the entries whose DATA is NaN, gradient and G those whose DIFFERENCE is NaN - an observed entry
                          with a non-finite state keeps its NaN in the loss, as in the kernels;
      "missing_data"      the OC unit's skip_missing: everything leaves out the entries whose data is NaN;
      "weighted"          weights w and Huber's threshold delta on e = sqrt(w) (values - data): an entry counts iff w > 0 and, under skip_missing, its data is not NaN;
                          the residuals and the rows of the sensitivities are scaled by sqrt(w), beyond delta by sqrt(w delta / |e|).
    Tensors of any one device (no check, no synchronisation)."""
    import torch
    B, W = packed.shape[0], sides[0][3].shape[-1]
    zero = torch.zeros((), dtype=torch.float64, device=packed.device)
    loss = grad = G = None
    for v, data, w, S in sides:
        d = v - data
        if rule == "plain":
            rho = (d * d).sum(dim=(1, 2))
        elif rule == "missing_residual":
            rho = torch.where(data == data, d * d, zero).sum(dim=(1, 2))
            obs = d == d
            d, S = torch.where(obs, d, zero), torch.where(obs[..., None], S, zero)
        elif rule == "missing_data":
            obs = ~torch.isnan(data)
            d = torch.where(obs, d, zero)
            rho = (d ** 2).sum(dim=(1, 2))
            S = torch.where(obs[..., None], S, zero)
        else:
            wf = (w if w is not None else torch.ones((), dtype=torch.float64, device=packed.device)).expand(*data.shape)
            obs = (wf > 0) & (data == data) if skip_missing else wf > 0
            e = wf.sqrt() * d
            ae = e.abs()
            quad = ae <= delta
            s = torch.where(quad, wf, wf * (delta / ae)).sqrt()
            rho = torch.where(obs, torch.where(quad, e * e, 2.0 * delta * ae - delta * delta), zero).sum(dim=(1, 2))
            d, S = torch.where(obs, s * d, zero), torch.where((obs & (s != 0))[..., None], s[..., None] * S, zero)
        g, GG = torch.einsum("bti,btip->bp", d, S), torch.einsum("btip,btiq->bpq", S, S)
        loss, grad, G = (rho, g, GG) if loss is None else (loss + rho, grad + g, G + GG)
    packed[:, W] = loss
    packed[:, :W] = grad
    packed[:, W + 1:] = G.reshape(B, W * W)


# ------------------------------------------------------------------------------------------------------
# per-model libraries (section B of include/pdp_hip.h)
# ------------------------------------------------------------------------------------------------------
_models = {}


def make_policy(kind, pivots=None, layers=None, table=None):
    """pdp_policy (include/pdp_hip.h): "poly" (Lagrange pivots, PDP.py:699-725), "mlp" (layers = hidden + [m], PDP.py:727-759) or "table" (table [T, n_basis]: the basis
    values of an open-loop policy at every step, u_t = sum_i table[t, i] theta_i - the warped / recovery-matrix variants, PDP.py:882-1141).  A table policy keeps its
    device tensor alive through the returned struct (pol._table)."""
    pol = PdpPolicy()
    if kind == "poly":
        pol.kind = PDP_POLICY_POLY
        pol.n_pivots = len(pivots)
        assert pol.n_pivots <= 16, "at most 16 Lagrange pivots"
        for i, v in enumerate(pivots):
            pol.pivots[i] = float(v)
    elif kind == "table":
        pol.kind = PDP_POLICY_TABLE
        pol._table = dev(np.ascontiguousarray(np.asarray(table, dtype=float)))
        assert pol._table.dim() == 2
        pol.n_basis = int(pol._table.shape[1])
        pol.table = pol._table.data_ptr()
    else:
        pol.kind = PDP_POLICY_MLP
        pol.n_layers = len(layers)
        assert pol.n_layers <= 16, "at most 16 weight layers"
        for i, v in enumerate(layers):
            pol.sizes[i] = int(v)
    return pol


class ModelLib:
    """One generated model library; methods mirror the C entry points on torch tensors."""

    def __init__(self, path):
        if not os.path.exists(path):
            raise RuntimeError("model library %s not built; there is no CPU fallback" % path)
        self.path = path
        self.lib = _dlopen(path)
        for name, (res, args) in entry_points(library="model").items():
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = res, args
        info = PdpModelInfo()
        self.lib.pdp_model_get_info(C.byref(info))
        self.kind, self.n, self.m, self.p = info.kind, info.n, info.m, info.p
        self.nnz_path, self.chunk, self.name = info.nnz_path, info.chunk, info.name.decode()

    # -- helpers
    def _theta(self, theta, B, p=None):
        th = dev(theta)
        p = self.p if p is None else p
        th = th.reshape(-1, p)
        assert th.shape[0] in (1, B), "theta must be [p] (shared) or [B,p]"
        return th, (p if th.shape[0] == B and B > 1 else 0)

    # -- OC
    def oc_rollout(self, x0, u, theta, want_cost=True):
        torch = torch_cuda()
        x0, u = dev(x0).reshape(-1, self.n), dev(u)
        B, T = x0.shape[0], u.shape[1]
        th, tb = self._theta(theta, B)
        x = torch.empty((B, T + 1, self.n), dtype=torch.float64, device="cuda")
        cost = torch.empty((B,), dtype=torch.float64, device="cuda") if want_cost else None
        check(self.lib.pdp_oc_rollout_batched(B, T, ptr(x0), ptr(u), ptr(th), tb, ptr(x), ptr(cost), current_stream_ptr()), "pdp_oc_rollout_batched")
        return x, cost

    def oc_rollout_feedback(self, x0, ubar, xbar, gains, alpha, theta):
        torch = torch_cuda()
        x0, ubar, xbar, gains, alpha = dev(x0).reshape(-1, self.n), dev(ubar), dev(xbar), dev(gains), dev(alpha)
        B, T = ubar.shape[0], ubar.shape[1]
        th, tb = self._theta(theta, B)
        x = torch.empty((B, T + 1, self.n), dtype=torch.float64, device="cuda")
        u = torch.empty((B, T, self.m), dtype=torch.float64, device="cuda")
        cost = torch.empty((B,), dtype=torch.float64, device="cuda")
        check(self.lib.pdp_oc_rollout_feedback_batched(B, T, ptr(x0), ptr(ubar), ptr(xbar), ptr(gains), ptr(alpha), ptr(th), tb, ptr(x), ptr(u), ptr(cost),
                                                       current_stream_ptr()), "pdp_oc_rollout_feedback_batched")
        return x, u, cost

    def oc_solve(self, x0, u_init, theta, tol=1e-9, newton_switch=1e-2, max_iter=300, check_every=2, ls_trials=10, straggler_patience=0,
                 print_level=0, want_gains=False):
        """Batched Newton solve of the OC problem (pdp_oc_solve_batched; stands where OCSys.ocSolver calls IPOPT).  u_init [B,T,m] is
        not modified.  Returns dict(state, control, costate, cost, grad_norm, converged (bool), iterations[, gains])."""
        torch = torch_cuda()
        x0, u = dev(x0).reshape(-1, self.n), dev(u_init).clone()
        B, T = u.shape[0], u.shape[1]
        th, tb = self._theta(theta, B)
        f64 = dict(dtype=torch.float64, device="cuda")
        x, lam = torch.empty((B, T + 1, self.n), **f64), torch.empty((B, T, self.n), **f64)
        cost, gnorm = torch.empty((B,), **f64), torch.empty((B,), **f64)
        conv = torch.zeros((B,), dtype=torch.int32, device="cuda")
        gains = torch.empty((B, T, self.n * self.m + self.m), **f64) if want_gains else None
        nbytes = self.lib.pdp_oc_solve_workspace_bytes(B, T, ls_trials)
        ws = torch.empty((max(nbytes, 8) // 8,), **f64)
        opts = PdpOcSolveOpts(tol, newton_switch, int(max_iter), int(check_every), int(ls_trials), int(straggler_patience), int(print_level))
        it = C.c_int(0)
        check(self.lib.pdp_oc_solve_batched(B, T, ptr(x0), ptr(th), tb, ptr(u), ptr(x), ptr(lam), ptr(cost), ptr(gnorm), ptr(conv), ptr(gains),
                                            C.byref(opts), C.byref(it), ptr(ws), nbytes, current_stream_ptr()), "pdp_oc_solve_batched")
        out = {"state": x, "control": u, "costate": lam, "cost": cost, "grad_norm": gnorm, "converged": conv != 0, "iterations": it.value}
        if want_gains:
            out["gains"] = gains
        return out

    def oc_solve_ms(self, x0, theta, T, tol=1e-10, max_iter=300, warm=None, want_gains=False, log_rows=0, restoration=True, u_init=None, consume_warm=False, predict=None,
                    soc=False, watchdog=False):
        """watchdog=True: IPOPT's watchdog in the line search (PDP_MS_WITH_WATCHDOG, include/pdp_hip.h: opt-in, not together with soc) - for cold solves that crawl.
        The reference's multiple-shooting NLP (PDP.py:131-182) solved by IPOPT's algorithm from its all-zero initial guess
        (pdp_oc_solve_ms_batched: a persistent pair of wavefronts per trajectory, all iterations in one launch).  warm = (x, u, lam) starts
        from a given point instead (x[:, 0] is replaced by x0).  restoration=False: a line search that falls below alpha_min ends the trajectory with
        PDP_MS_RESTORATION instead of entering the feasibility restoration (include/pdp_hip.h).  u_init [B, T, m] (instead of warm): start from these
        controls, their rollout and the least-squares multiplier estimate (PDP_MS_FROM_CONTROLS).  consume_warm: the warm tensors themselves become the outputs
        (no copies: for callers that built the starting point for this call, e.g. oc_predict).  predict = dict(dtheta [p] or [B, p], dxdp, dudp[, riccati]) with
        warm = the solution at the previous parameter: the kernel starts from its first-order prediction for the step dtheta (PDP_MS_PREDICT: what oc_predict computes,
        applied while the point is loaded - no extra launch; with consume_warm the previous solution's tensors are overwritten by the new one, as an IRL loop wants it).
        predict["guard"] (default True, PDP_MS_PREDICT_GUARD): the previous solution is evaluated beside its prediction and the solve starts from whichever has the smaller
        scaled KKT error (a first-order prediction across a large parameter step can be worse than no prediction: status & PDP_MS_PREDICT_REJECTED (512) marks the trajectories where it was dropped).
        soc=True (PDP_MS_WITH_SOC): IPOPT's second-order correction in the line search (status & PDP_MS_SOC (1024): a corrected step was taken; include/pdp_hip.h says why it is off by default).
        Returns dict(state, control, costate, cost,
        resid [B,2], converged (bool), iterations [B], status [B][, gains])."""
        torch = torch_cuda()
        x0 = dev(x0).reshape(-1, self.n)
        B, T = x0.shape[0], int(T)
        th, tb = self._theta(theta, B)
        f64 = dict(dtype=torch.float64, device="cuda")
        if warm is not None:
            assert u_init is None, "warm and u_init exclude each other"
            if consume_warm:        # in place: the caller's tensors ARE the outputs - a silent copy would leave an IRL loop re-solving from a stale point
                for a in warm:          # (an exception, not an assert: under `python -O` the silent copy would come back)
                    if not (torch.is_tensor(a) and a.is_cuda and a.dtype == torch.float64 and a.is_contiguous()):
                        raise TypeError("oc_solve_ms(consume_warm=True) works IN PLACE on the warm start: state, control and costate must be contiguous fp64 CUDA tensors "
                                        "(got %s); pass consume_warm=False to start from a copy of anything dev() converts" % (type(a).__name__ if not torch.is_tensor(a)
                                        else "%s %s tensor, contiguous=%s" % (a.device.type, a.dtype, a.is_contiguous())))
                x, u, lam = warm
            else:
                x, u, lam = (dev(a).clone().contiguous() for a in warm)
            assert x.shape == (B, T + 1, self.n) and u.shape == (B, T, self.m) and lam.shape == (B, T, self.n)
        elif u_init is not None:
            u = dev(u_init).clone().contiguous()
            assert u.shape == (B, T, self.m)
            x, lam = torch.zeros((B, T + 1, self.n), **f64), torch.zeros((B, T, self.n), **f64)
        else:
            x, u, lam = torch.empty((B, T + 1, self.n), **f64), torch.empty((B, T, self.m), **f64), torch.empty((B, T, self.n), **f64)
        cost, resid = torch.empty((B,), **f64), torch.empty((B, 2), **f64)
        conv, iters, status = (torch.zeros((B,), dtype=torch.int32, device="cuda") for _ in range(3))
        gains = torch.empty((B, T, self.n * self.m + self.m), **f64) if want_gains else None
        nbytes = self.lib.pdp_oc_solve_ms_workspace_bytes(B, T, int(max_iter))
        ws = torch.empty((max(nbytes, 8) // 8,), **f64)
        log = torch.zeros((B, int(log_rows), 8), **f64) if log_rows > 0 else None
        flags = (PDP_MS_WARM if warm is not None else 0) | (0 if restoration else PDP_MS_NO_RESTORATION) | (PDP_MS_WARM | PDP_MS_FROM_CONTROLS if u_init is not None else 0) | \
            (PDP_MS_WITH_SOC if soc else 0) | (PDP_MS_WITH_WATCHDOG if watchdog else 0)
        opts = PdpOcMsOpts(float(tol), int(max_iter), flags, int(log_rows))
        keep = None
        if predict is not None:
            assert warm is not None, "predict needs the previous solution as the warm point"
            dth, dtb = self._theta(predict["dtheta"], B)
            opts.flags |= PDP_MS_PREDICT
            opts.dtheta_bstride, opts.dtheta = dtb, dth.data_ptr()
            if predict.get("record") is not None:           # the packed fp32 record (oc_pdp_grad(want_predict_record=True))
                keep = (dth, predict["record"])
                assert keep[1].dtype == torch.float32 and tuple(keep[1].shape) == (B, T, int(self.lib.pdp_oc_predict_record_floats())) and keep[1].is_contiguous()
                opts.predict_record = keep[1].data_ptr()
            else:
                keep = (dth, dev(predict["dxdp"]), dev(predict["dudp"]), dev(predict["riccati"]) if predict.get("riccati") is not None else None)
                assert keep[1].shape == (B, T + 1, self.n, self.p) and keep[2].shape == (B, T, self.m, self.p)
                opts.dxdp, opts.dudp = keep[1].data_ptr(), keep[2].data_ptr()
                opts.riccati = keep[3].data_ptr() if keep[3] is not None else None
            if predict.get("primal"):                       # states and controls only (a record written with want_predict_record="primal" holds nothing else)
                opts.flags |= PDP_MS_PREDICT_PRIMAL
            if predict.get("guard", True):                  # (default) the prediction is kept only if its KKT error does not exceed the previous solution's;
                opts.flags |= PDP_MS_PREDICT_GUARD          # status bit PDP_MS_PREDICT_REJECTED says where it was not
        check(self.lib.pdp_oc_solve_ms_batched(B, T, ptr(x0), ptr(th), tb, ptr(x), ptr(u), ptr(lam), ptr(cost), ptr(resid), ptr(conv), ptr(iters),
                                               ptr(status), ptr(gains), ptr(log), C.byref(opts), ptr(ws), nbytes, current_stream_ptr()), "pdp_oc_solve_ms_batched")
        out = {"state": x, "control": u, "costate": lam, "cost": cost, "resid": resid, "converged": conv != 0, "converged_flags": conv, "iterations": iters, "status": status}
        if want_gains:
            out["gains"] = gains
        if log is not None:
            out["log"] = log            # [B, log_rows, 8]: iteration, objective, inf_pr, inf_du, dw, alpha (minus alpha: a second-order-corrected step), grad(phi)'d, theta
        return out

    def oc_costate(self, x, u, theta):
        torch = torch_cuda()
        x, u = dev(x), dev(u)
        B, T = u.shape[0], u.shape[1]
        th, tb = self._theta(theta, B)
        lam = torch.empty((B, T, self.n), dtype=torch.float64, device="cuda")
        check(self.lib.pdp_oc_costate_batched(B, T, ptr(x), ptr(u), ptr(th), tb, ptr(lam), current_stream_ptr()), "pdp_oc_costate_batched")
        return lam

    def oc_ms_residuals(self, x, u, lam, theta):
        """Residuals of ocSolver's multiple-shooting NLP at (x, u, lam) (pdp_oc_ms_residuals_batched): dict(c [B,T,n] defects, rx [B,T+1,n], ru [B,T,m] Lagrangian
        gradients, cost [B,T+1] stage costs with the final cost last)."""
        torch = torch_cuda()
        x, u, lam = dev(x), dev(u), dev(lam)
        B, T = u.shape[0], u.shape[1]
        th, tb = self._theta(theta, B)
        f64 = dict(dtype=torch.float64, device="cuda")
        out = {"c": torch.empty((B, T, self.n), **f64), "rx": torch.empty((B, T + 1, self.n), **f64), "ru": torch.empty((B, T, self.m), **f64),
               "cost": torch.empty((B, T + 1), **f64)}
        check(self.lib.pdp_oc_ms_residuals_batched(B, T, ptr(x), ptr(u), ptr(lam), ptr(th), tb, ptr(out["c"]), ptr(out["rx"]), ptr(out["ru"]), ptr(out["cost"]),
                                                   current_stream_ptr()), "pdp_oc_ms_residuals_batched")
        return out

    def oc_auxsys(self, x, u, lam, theta, only=None):
        """materialised OCSys.getAuxSys; `only` = iterable of keys to produce (others are skipped), may include 'dHu'"""
        torch = torch_cuda()
        x, u, lam = dev(x), dev(u), dev(lam)
        B, T = u.shape[0], u.shape[1]
        n, m, p = self.n, self.m, self.p
        th, tb = self._theta(theta, B)
        shp = dict(dynF=(B, T, n, n), dynG=(B, T, n, m), dynE=(B, T, n, p), Hxx=(B, T, n, n), Hxu=(B, T, n, m), Hxe=(B, T, n, p),
                   Hux=(B, T, m, n), Huu=(B, T, m, m), Hue=(B, T, m, p), hxx=(B, n, n), hxe=(B, n, p))
        if only is not None:
            shp["dHu"] = (B, T, m)
            shp = {k: v for k, v in shp.items() if k in only}
        out = {k: torch.empty(s, dtype=torch.float64, device="cuda") for k, s in shp.items()}
        o = PdpOcAuxsys(**{k: v.data_ptr() for k, v in out.items()})
        check(self.lib.pdp_oc_auxsys_batched(B, T, ptr(x), ptr(u), ptr(lam), ptr(th), tb, C.byref(o), current_stream_ptr()), "pdp_oc_auxsys_batched")
        return out

    def oc_pdp_grad(self, u, theta, demo_x, demo_u, x0=None, x=None, lam=None, want_sens=False, buffers=None, packed=False, want_riccati=False,
                    want_predict_record=False, gauss_newton=False, skip_missing=False, weights_x=None, weights_u=None, huber_delta=None, want_ini=False):
        """Fused forward + Riccati + PDP gradient.  Give (x, lam) to use an optimal trajectory (PDP_OC_GIVEN_TRAJ),
        else x0 and the kernel integrates u and the costates itself.  Returns dict(loss, grad, x, lam, status[, dxdp, dudp][, riccati]).
        packed: the kernel writes gradient and loss as one [B, p+1] tensor (PDP_OC_PACKED; out["packed"], out["grad"] is a view of it).
        want_riccati (with want_sens: everything oc_predict needs): also the Riccati matrices of the auxiliary control system,
        out["riccati"] [B, T, n n + n p + 1] = P_{t+1} | W_{t+1} | one scratch word per stage (pdp_oc_pdp_grad_sens_batched).
        want_predict_record: out["predict_record"], float32 [B, T, 2 n p + m p + n (n + 1) / 2] - the same information packed in single precision, what an IRL loop
        hands to the next oc_solve_ms(predict=dict(dtheta=..., record=...)) (2.4 times less memory traffic than the fp64 outputs).  want_predict_record="primal"
        (PDP_OC_RECORD_PRIMAL): only the X | U part of the record is written - for oc_solve_ms(predict=dict(..., primal=True)), the prediction of states and controls.
        gauss_newton (PDP_GRAD_GAUSS_NEWTON): the kernel also contracts the sensitivity tiles of its forward sweep with themselves and writes ONE row per trajectory,
        out["packed_gn"] [B, p + 1 + p p] = gradient | loss | G row-major, G = J'J = sum_t X_t' X_t + U_t' U_t the Gauss-Newton matrix of the sum-of-squares loss (no
        factor: grad = J'r and G belong together); out["grad"] and out["gn"] [B, p, p] are views of it.  Not together with want_sens, want_riccati, want_predict_record or
        packed (ValueError).  Beyond the fused kernels' limits the row is filled from the materialised sensitivities (two einsums): one layout either way.
        skip_missing (PDP_GRAD_SKIP_MISSING): a NaN in demo_x / demo_u marks an entry that was not observed - its residual is left out of the loss, its term out of the
        gradient and, with gauss_newton, its Jacobian row out of G (only NaN: an inf propagates as always).  demo_x[:, 0] may be all NaN when x0 is given.  Alone, with
        packed or with gauss_newton; with want_sens, want_riccati or want_predict_record: ValueError (and oc_pdp_vjp has no such switch: a NaN cotangent is an error).
        Beyond the fused kernels' limits the same rows come from the materialised sensitivities, masked and contracted with torch.einsum.
        weights_x [n], [T+1, n] or [B, T+1, n], weights_u [m], [T, m] or [B, T, m], huber_delta (pdp_oc_pdp_grad_wls_batched, include/pdp_hip_oc_wls.h: the semantics):
        a weight per demonstration entry (0: not observed) and Huber's loss on the standardised residual.  Any of the three implies the packed Gauss-Newton dict
        (packed_gn, grad, loss, gn as views) of the weighted / robust loss; they combine with skip_missing, x0, a given (x, lam) and buffers={"packed_gn": ...}; with
        want_sens, want_riccati, want_predict_record or packed: ValueError.  Beyond the fused kernels' limits the same row comes from scaled residuals and row-scaled
        materialised sensitivities.
        want_ini (pdp_oc_sens_out.grad_x0): also out["grad_x0"] [B, n], half the gradient of the loss with respect to the initial state through the solution (the
        convention of out["grad"]), from an adjoint sweep behind the unit's launch; every other output keeps its bits.  Alone, with packed, want_sens, want_riccati or
        want_predict_record; with gauss_newton, skip_missing or the weights: ValueError.  Beyond the fused kernels' limits: the materialised route with n further columns."""
        weighted = weights_x is not None or weights_u is not None or huber_delta is not None
        if want_ini and (weighted or gauss_newton or skip_missing):
            raise ValueError("oc_pdp_grad: want_ini=True (the gradient with respect to the initial state) goes with the plain gradient, packed and the sensitivity "
                             "outputs - not with gauss_newton, skip_missing, weights_x, weights_u or huber_delta")
        if weighted:
            for name, on in (("want_sens", want_sens), ("want_riccati", want_riccati), ("want_predict_record", want_predict_record), ("packed", packed)):
                if on:
                    raise ValueError("oc_pdp_grad: weights_x, weights_u and huber_delta give the packed Gauss-Newton row only - not together with %s" % name)
            u_shape = tuple(np.shape(u))
            if len(u_shape) != 3 or u_shape[2] != self.m:
                raise ValueError("oc_pdp_grad: u must be [B, T, %d], got %s" % (self.m, u_shape))
        if skip_missing and (want_sens or want_riccati or want_predict_record):
            raise ValueError("oc_pdp_grad: skip_missing=True goes with the gradient, packed or gauss_newton rows only - not with want_sens, want_riccati or "
                             "want_predict_record")
        if gauss_newton and (want_sens or want_riccati or want_predict_record or packed):
            raise ValueError("oc_pdp_grad: gauss_newton=True goes with the plain gradient only - not with want_sens, want_riccati, want_predict_record or packed")
        if weighted or gauss_newton:
            if x is not None and lam is None:
                raise ValueError("oc_pdp_grad: a given trajectory needs x and lam")
            if x is None and x0 is None:
                raise ValueError("oc_pdp_grad: x0 [B, %d] is needed unless (x, lam) are given" % self.n)
            return self.oc_rows_prepared(demo_x, demo_u, skip_missing, weights_x, weights_u, huber_delta, buffers)[0](u, theta, x0, x, lam)
        torch = torch_cuda()
        u, demo_x, demo_u = dev(u), dev(demo_x), dev(demo_u)
        B, T = u.shape[0], u.shape[1]
        n, m, p = self.n, self.m, self.p
        th, tb = self._theta(theta, B)
        flags = 0
        if x is not None:
            assert lam is not None
            x, lam, flags = dev(x), dev(lam), PDP_OC_GIVEN_TRAJ
            x0 = None
        else:
            x0 = dev(x0).reshape(B, n)
        bufs = buffers if buffers is not None else {}
        if x is None:
            x, lam = _buffer(bufs, "x", (B, T + 1, n)), _buffer(bufs, "lam", (B, T, n))
        loss = _buffer(bufs, "loss", (B,))
        if packed:
            pk = _buffer(bufs, "packed", (B, p + 1))
            grad, flags = pk[:, :p], flags | PDP_OC_PACKED
        else:
            pk = grad = _buffer(bufs, "grad", (B, p))
        status = _buffer(bufs, "status", (B,), torch.int32)
        dxdp = _buffer(bufs, "dxdp", (B, T + 1, n, p)) if want_sens else None
        dudp = _buffer(bufs, "dudp", (B, T, m, p)) if want_sens else None
        ric = _buffer(bufs, "riccati", (B, T, int(self.lib.pdp_oc_riccati_doubles()))) if want_riccati else None
        prec = _buffer(bufs, "predict_record", (B, T, int(self.lib.pdp_oc_predict_record_floats())), torch.float32) if want_predict_record else None
        if want_predict_record == "primal":
            flags |= PDP_OC_RECORD_PRIMAL
        if skip_missing:
            flags |= PDP_GRAD_SKIP_MISSING
        nbytes = self.lib.pdp_oc_pdp_workspace_bytes(B, T)
        ws = _buffer(bufs, "ws", (max(nbytes, 8) // 8,))
        gx0 = _buffer(bufs, "grad_x0", (B, n)) if want_ini else None
        if want_riccati or want_predict_record or want_ini:
            so = PdpOcSensOut(dxdp.data_ptr() if dxdp is not None else None, dudp.data_ptr() if dudp is not None else None,
                              ric.data_ptr() if ric is not None else None, prec.data_ptr() if prec is not None else None, *((gx0.data_ptr(),) if want_ini else ()))
            rc = self.lib.pdp_oc_pdp_grad_sens_batched(B, T, flags, ptr(x0), ptr(u), ptr(th), tb, ptr(demo_x), ptr(demo_u), ptr(x), ptr(lam), ptr(loss),
                                                       ptr(pk), C.byref(so), ptr(status), ptr(ws), nbytes, current_stream_ptr())
            if rc == PDP_E_SIZE and (want_riccati or want_predict_record):
                raise RuntimeError("pdp_oc_pdp_grad_sens_batched: the Riccati / prediction records are outputs of the fused kernels (n <= 16, m <= 4, m + p <= 16)")
        else:
            rc = self.lib.pdp_oc_pdp_grad_batched(B, T, flags, ptr(x0), ptr(u), ptr(th), tb, ptr(demo_x), ptr(demo_u), ptr(x), ptr(lam), ptr(loss),
                                                  ptr(pk), ptr(dxdp), ptr(dudp), ptr(status), ptr(ws), nbytes, current_stream_ptr())
        if rc == PDP_E_SIZE:
            # m + p > 16 (beyond the fused kernel's single parameter tile), n > 16 / m > 4 (beyond one tile per matrix: the size-generic LQR
            # kernel takes over - any n, m), or a horizon whose staging exceeds the LDS: the reference's own route, kernel by kernel
            self._warn_materialised(T)
            if skip_missing:                                    # loss and gradient of the masked row (_oc_rows: the same route, the same contraction)
                row = torch.empty((B, p + 1 + p * p), dtype=torch.float64, device="cuda")
                self._oc_rows_materialised(u, th, demo_x, demo_u, x0, x, lam, flags, loss, row, status, "missing_data")
                grad.copy_(row[:, :p])
            else:
                self._oc_pdp_grad_materialised(u, theta, demo_x, demo_u, x0, x, lam, flags, loss, grad, status, dxdp, dudp, grad_x0=gx0)
            if packed:
                pk[:, p].copy_(loss)
            rc = 0
        check(rc, "pdp_oc_pdp_grad_batched")
        out = dict(loss=loss, grad=grad, x=x, lam=lam, status=status)
        if packed:
            out["packed"] = pk
        if want_sens:
            out.update(dxdp=dxdp, dudp=dudp)
        if want_riccati:
            out["riccati"] = ric
        if want_predict_record:
            out["predict_record"] = prec
        if want_ini:
            out["grad_x0"] = gx0
        return out

    def _oc_rows_materialised(self, u, th, demo_x, demo_u, x0, x, lam, flags, loss, pk, status, rule, wxd=None, wud=None, delta=float("inf")):
        """The packed row of the OC unit beyond the fused kernels' limits, by `rule` of packed_row_from_sensitivities: the want_sens launch of the kernel-by-kernel
        route gives x, lam, status and the sensitivities.  "plain": loss and gradient are that launch's own and G is contracted here.  Else the launch runs on the
        demonstrations with their NaNs replaced by zeros and the whole row is re-formed here from masked / scaled residuals and sensitivities (selected, not
        multiplied: an inf in an absent slot cannot exist - only NaN is absent).  Fills loss [B], pk [B, p + 1 + p p] and status."""
        torch = torch_cuda()
        (B, T), n, m, p = u.shape[:2], self.n, self.m, self.p
        dxdp, dudp = torch.empty((B, T + 1, n, p), dtype=torch.float64, device="cuda"), torch.empty((B, T, m, p), dtype=torch.float64, device="cuda")
        if rule == "plain":
            self._oc_pdp_grad_materialised(u, th, demo_x, demo_u, x0, x, lam, flags, loss, pk[:, :p], status, dxdp, dudp)
            pk[:, p].copy_(loss)
            pk[:, p + 1:].copy_((torch.einsum("btip,btiq->bpq", dxdp, dxdp) + torch.einsum("btip,btiq->bpq", dudp, dudp)).reshape(B, p * p))
            return
        zero = torch.zeros((), dtype=torch.float64, device="cuda")
        self._oc_pdp_grad_materialised(u, th, torch.where(torch.isnan(demo_x), zero, demo_x), torch.where(torch.isnan(demo_u), zero, demo_u), x0, x, lam, flags, loss,
                                       pk[:, :p], status, dxdp, dudp)
        packed_row_from_sensitivities(pk, [(x, demo_x, wxd, dxdp), (u, demo_u, wud, dudp)], rule, delta, bool(flags & PDP_GRAD_SKIP_MISSING))
        loss.copy_(pk[:, p])

    def _oc_rows(self, u, th, tb, demo_x, demo_u, x0, x, lam, buffers, skip_missing=False, wls=None):
        """The fused OC unit as a least-squares evaluation on device tensors and normalised arguments, no check and no host synchronisation, ONE launch: what
        oc_pdp_grad runs with gauss_newton or weights and what every evaluation of the IRL loops of irl.py runs (oc_rows_prepared marshals for it).  th [1 or B, p]
        with row stride tb; (x, lam) given (PDP_OC_GIVEN_TRAJ) or x0 [B, n]; wls: None - pdp_oc_pdp_grad_batched with PDP_GRAD_GAUSS_NEWTON - or (weights_x
        [T+1, n] or [B, T+1, n] or None, its batch stride, weights_u [T, m] or [B, T, m] or None, its batch stride, delta as a float) from oc_wls_arguments -
        pdp_oc_pdp_grad_wls_batched.  Returns the packed Gauss-Newton dict: packed_gn [B, p + 1 + p p] and loss, grad, gn as views of it, x, lam, status."""
        torch = torch_cuda()
        B, T, n, p = u.shape[0], u.shape[1], self.n, self.p
        bufs = buffers if buffers is not None else {}
        flags = PDP_GRAD_SKIP_MISSING if skip_missing else 0
        if x is not None:
            flags |= PDP_OC_GIVEN_TRAJ
        else:
            x, lam = _buffer(bufs, "x", (B, T + 1, n)), _buffer(bufs, "lam", (B, T, n))
        loss, pk, status = _buffer(bufs, "loss", (B,)), _buffer(bufs, "packed_gn", (B, p + 1 + p * p)), _buffer(bufs, "status", (B,), torch.int32)
        nbytes = self.lib.pdp_oc_pdp_workspace_bytes(B, T)
        ws = _buffer(bufs, "ws", (max(nbytes, 8) // 8,))
        if wls is not None:
            name, (wxd, wxs, wud, wus, delta) = "pdp_oc_pdp_grad_wls_batched", wls
            rc = self.lib.pdp_oc_pdp_grad_wls_batched(B, T, flags, ptr(x0), ptr(u), ptr(th), tb, ptr(demo_x), ptr(demo_u), ptr(wxd), wxs, ptr(wud), wus, delta, ptr(x),
                                                      ptr(lam), ptr(loss), ptr(pk), ptr(status), ptr(ws), nbytes, current_stream_ptr())
        else:
            name, flags = "pdp_oc_pdp_grad_batched", flags | PDP_GRAD_GAUSS_NEWTON
            rc = self.lib.pdp_oc_pdp_grad_batched(B, T, flags, ptr(x0), ptr(u), ptr(th), tb, ptr(demo_x), ptr(demo_u), ptr(x), ptr(lam), ptr(loss), ptr(pk), ptr(None),
                                                  ptr(None), ptr(status), ptr(ws), nbytes, current_stream_ptr())
        if rc == PDP_E_SIZE:                        # beyond the fused kernels' limits: the same row from the materialised sensitivities
            self._warn_materialised(T)
            if wls is not None:
                self._oc_rows_materialised(u, th, demo_x, demo_u, x0, x, lam, flags, loss, pk, status, "weighted", wxd, wud, delta)
            else:
                self._oc_rows_materialised(u, th, demo_x, demo_u, x0, x, lam, flags, loss, pk, status, "missing_data" if skip_missing else "plain")
            rc = 0
        check(rc, name)
        return dict(packed_gn=pk, loss=pk[:, p], grad=pk[:, :p], gn=pk[:, p + 1:].view(B, p, p), x=x, lam=lam, status=status)

    def oc_rows_prepared(self, demo_x, demo_u, skip_missing=False, weights_x=None, weights_u=None, huber_delta=None, buffers=None):
        """The OC unit's least-squares evaluation as a PREPARED call: weights_x, weights_u and huber_delta are checked once (oc_wls_arguments on the shape of demo_u:
        ValueErrors before anything is moved), demonstrations and weights moved to the device once; the returned rows(u, theta, x0=None, x=None, lam=None) is then
        one launch per call (_oc_rows: pdp_oc_pdp_grad_wls_batched where one of the three keywords was given, else pdp_oc_pdp_grad_batched with
        PDP_GRAD_GAUSS_NEWTON) and returns the packed Gauss-Newton dict.  theta [p] shared or [B, p] per sample; (x, lam) a given trajectory, else x0.  Returns
        (rows, held) with held = dict(demo_x, demo_u): the device tensors the evaluations read."""
        wls = None
        if weights_x is not None or weights_u is not None or huber_delta is not None:
            B, T = (int(v) for v in np.shape(demo_u)[:2])
            wx, wxs, wu, wus, delta = oc_wls_arguments(weights_x, weights_u, huber_delta, B, T, self.n, self.m)
            wls = (dev(wx).contiguous() if wx is not None else None, wxs, dev(wu).contiguous() if wu is not None else None, wus, delta)
        demo_x, demo_u = dev(demo_x), dev(demo_u)
        bufs = buffers if buffers is not None else {}

        def rows(u, theta, x0=None, x=None, lam=None):
            u = dev(u)
            B = u.shape[0]
            th, tb = self._theta(theta, B)
            if x is not None:
                x, lam, x0 = dev(x), dev(lam), None
            else:
                x0 = dev(x0).reshape(B, self.n)
            return self._oc_rows(u, th, tb, demo_x, demo_u, x0, x, lam, bufs, skip_missing, wls)
        return rows, dict(demo_x=demo_x, demo_u=demo_u)

    def oc_pdp_vjp(self, u, theta, gx, gu, x0=None, x=None, lam=None, buffers=None, want_ini=False):
        """The fused unit as a vector-Jacobian product of the OC solution (PDP_OC_COTANGENT, include/pdp_hip.h): gx [B, T+1, n] = dL/dx and gu [B, T, m] = dL/du are the
        cotangents of a caller's scalar loss L(x, u); grad [B, p] = sum_t gx_t' X_t + gu_t' U_t is dL/dtheta through the solution, X_t, U_t never leaving the chip.
        gx[:, 0] is not read (X_0 = 0).  Trajectory arguments as in oc_pdp_grad: (x, lam) given (PDP_OC_GIVEN_TRAJ), else x0 and the kernel integrates u and the costates.
        No loss is formed.  Returns dict(grad, x, lam, status); `buffers` (a dict the caller keeps) reuses the output tensors and the workspace between calls.
        Problems beyond the fused kernels' limits take the kernel-by-kernel route, as in oc_pdp_grad.
        want_ini (pdp_oc_sens_out.grad_x0 of pdp_oc_pdp_grad_sens_batched): also grad_x0 [B, n] = dL/dx_0 through the solution - the adjoint sweep mu_T = gx_T,
        v_t = gu_t + G_t' mu_{t+1}, mu_t = gx_t + F_t' mu_{t+1} - K_t' v_t, grad_x0 = mu_0 with the unit's own gains K_t, launched behind the unit on the same stream.
        gx[:, 0] is then read by the sweep and enters grad_x0 only; grad, x, lam and status keep their bits."""
        n, m, p = self.n, self.m, self.p
        u_shape, gx_shape, gu_shape = tuple(np.shape(u)), tuple(np.shape(gx)), tuple(np.shape(gu))
        if len(u_shape) != 3 or u_shape[2] != m:                # (shapes are judged before anything is converted or launched)
            raise ValueError("oc_pdp_vjp: u must be [B, T, %d], got %s" % (m, u_shape))
        B, T = u_shape[0], u_shape[1]
        if gx_shape != (B, T + 1, n) or gu_shape != (B, T, m):
            raise ValueError("oc_pdp_vjp: cotangents must be gx [B, T+1, n] = %s and gu [B, T, m] = %s, got %s and %s"
                             % ((B, T + 1, n), (B, T, m), gx_shape, gu_shape))
        if x is not None and (lam is None or tuple(np.shape(x)) != (B, T + 1, n) or tuple(np.shape(lam)) != (B, T, n)):
            raise ValueError("oc_pdp_vjp: a given trajectory needs x %s and lam %s" % ((B, T + 1, n), (B, T, n)))
        if x is None and (x0 is None or int(np.prod(np.shape(x0))) != B * n):
            raise ValueError("oc_pdp_vjp: x0 [B, %d] is needed unless (x, lam) are given" % n)
        torch = torch_cuda()
        u, gx, gu = dev(u), dev(gx), dev(gu)
        th, tb = self._theta(theta, B)
        flags = PDP_OC_COTANGENT
        if x is not None:
            x, lam, flags = dev(x), dev(lam), flags | PDP_OC_GIVEN_TRAJ
            x0 = None
        else:
            x0 = dev(x0).reshape(B, n)
        bufs = buffers if buffers is not None else {}
        if x is None:
            x, lam = _buffer(bufs, "x", (B, T + 1, n)), _buffer(bufs, "lam", (B, T, n))
        grad = _buffer(bufs, "grad", (B, p))
        status = _buffer(bufs, "status", (B,), torch.int32)
        nbytes = self.lib.pdp_oc_pdp_workspace_bytes(B, T)
        ws = _buffer(bufs, "ws", (max(nbytes, 8) // 8,))
        gx0 = _buffer(bufs, "grad_x0", (B, n)) if want_ini else None
        if want_ini:
            so = PdpOcSensOut(None, None, None, None, gx0.data_ptr())
            rc = self.lib.pdp_oc_pdp_grad_sens_batched(B, T, flags, ptr(x0), ptr(u), ptr(th), tb, ptr(gx), ptr(gu), ptr(x), ptr(lam), ptr(None),
                                                       ptr(grad), C.byref(so), ptr(status), ptr(ws), nbytes, current_stream_ptr())
        else:
            rc = self.lib.pdp_oc_pdp_grad_batched(B, T, flags, ptr(x0), ptr(u), ptr(th), tb, ptr(gx), ptr(gu), ptr(x), ptr(lam), ptr(None),
                                                  ptr(grad), ptr(None), ptr(None), ptr(status), ptr(ws), nbytes, current_stream_ptr())
        if rc == PDP_E_SIZE:
            self._warn_materialised(T)
            self._oc_pdp_grad_materialised(u, theta, gx, gu, x0, x, lam, flags, None, grad, status, grad_x0=gx0)
            rc = 0
        check(rc, "pdp_oc_pdp_grad_batched (PDP_OC_COTANGENT)")
        out = dict(grad=grad, x=x, lam=lam, status=status)
        if want_ini:
            out["grad_x0"] = gx0
        return out

    def oc_x0_vjp_rows(self):
        """Pool rows (time steps per lane-parallel pass) of the initial-state adjoint sweep, oc_x0_vjp_kernel: csrc/pdp_sweep_pool.h's rule restated (no entry
        point reports it) - what a pool of SWEEP_POOL_DOUBLES holds of rows of SOLF_NVAR + n m + n + m doubles, made odd, at least 4 and at most 64.  SOLF_NVAR, the number of
        variable entries of (F, G), is read from the model's generated header.  The result bits do not depend on the rows: tests place their chunk edges by them."""
        import re
        from . import codegen
        src = open(os.path.join(codegen.GEN_DIR, self.name + ".h")).read()
        nvar = int(re.search(r"\bSOLF_NVAR\s*=\s*(\d+)", src).group(1))
        stride = (nvar + self.n * self.m + self.n + self.m) | 1
        return min(64, max(4, SWEEP_POOL_DOUBLES // stride))

    def _warn_materialised(self, T):
        """once per model: the problem is outside the fused kernel's limits and takes the kernel-by-kernel route"""
        if not getattr(self, "_warned_materialised", False):
            import warnings
            warnings.warn("pdp_oc_pdp_grad_batched: problem outside the fused kernel's limits (n = %d, m = %d, p = %d, T = %d): taking the "
                          "kernel-by-kernel route through HBM (several launches, roughly ten times slower)" % (self.n, self.m, self.p, T), RuntimeWarning)
            self._warned_materialised = True

    def oc_pdp_grad_prepared(self, u, theta, demo_x, demo_u, x0, packed_out=None):
        """The fused OC unit as a PREPARED call: every argument of pdp_oc_pdp_grad_batched marshalled once; the returned step() is one foreign call on the stream that is
        current when it runs (no tensor conversions, no dictionary, no allocation per step) - what a driver that calls the unit in a loop on fixed buffers should use, and what
        bench.py times: oc_pdp_grad's Python wrapper costs 25 - 60 us per call, which a busy host cannot always hide under a 97 us kernel (the driver's 0.104 - 0.109 ms per step
        against 0.097 - 0.099 ms of kernel time).  Returns (step, out) with out = dict(loss, grad, x, lam, status, packed): the tensors every step() overwrites.
        packed_out: a [B, p + 1] tensor to receive gradient | loss (PDP_OC_PACKED), e.g. the buffer a collective sends; allocated when None."""
        torch = torch_cuda()
        u, demo_x, demo_u = dev(u), dev(demo_x), dev(demo_u)
        B, T = u.shape[0], u.shape[1]
        n, p = self.n, self.p
        th, tb = self._theta(theta, B)
        x0 = dev(x0).reshape(B, n)
        f64 = dict(dtype=torch.float64, device="cuda")
        x, lam, loss = torch.empty((B, T + 1, n), **f64), torch.empty((B, T, n), **f64), torch.empty((B,), **f64)
        pk = torch.empty((B, p + 1), **f64) if packed_out is None else packed_out
        assert pk.is_cuda and pk.dtype == torch.float64 and pk.is_contiguous() and tuple(pk.shape) == (B, p + 1)
        status = torch.empty((B,), dtype=torch.int32, device="cuda")
        nbytes = self.lib.pdp_oc_pdp_workspace_bytes(B, T)
        ws = torch.empty((max(nbytes, 8) // 8,), **f64)
        keep = (u, th, demo_x, demo_u, x0, x, lam, loss, pk, status, ws)                 # (the closure owns every buffer the kernel touches)
        fn = self.lib.pdp_oc_pdp_grad_batched
        args = (B, T, PDP_OC_PACKED, ptr(x0), ptr(u), ptr(th), tb, ptr(demo_x), ptr(demo_u), ptr(x), ptr(lam), ptr(loss), ptr(pk), ptr(None), ptr(None), ptr(status), ptr(ws), nbytes)
        rc0 = fn(*args, current_stream_ptr())
        if rc0 != 0:
            raise RuntimeError("pdp_oc_pdp_grad_batched (prepared call): %s - problems outside the fused kernel's limits take oc_pdp_grad" % PDP_E.get(rc0, rc0))
        cur = torch.cuda.current_stream

        def step(_fn=fn, _args=args, _keep=keep):
            rc = _fn(*_args, C.c_void_p(cur().cuda_stream))
            if rc != 0:
                check(rc, "pdp_oc_pdp_grad_batched")
        return step, dict(loss=loss, grad=pk[:, :p], x=x, lam=lam, status=status, packed=pk)

    def oc_predict_from_record(self, x, u, lam, dtheta, record, primal=False):
        """oc_predict from the packed fp32 record (pdp_oc_predict_record_batched): new tensors (x, u, lam) + first-order change for the step dtheta
        (primal: states and controls only, lam is returned as it came)"""
        x, u, lam = dev(x).clone(), dev(u).clone(), dev(lam).clone()
        B, T = u.shape[0], u.shape[1]
        dth, dtb = self._theta(dtheta, B)
        assert record.dtype == torch_cuda().float32 and tuple(record.shape) == (B, T, int(self.lib.pdp_oc_predict_record_floats()))
        check(self.lib.pdp_oc_predict_record_batched(B, T, ptr(dth), dtb, ptr(record), ptr(x), ptr(u), None if primal else ptr(lam), current_stream_ptr()),
              "pdp_oc_predict_record_batched")
        return x, u, lam

    def oc_predict(self, x, u, lam, dtheta, dxdp, dudp, riccati=None):
        """First-order prediction of the optimal (x, u, lam) at theta + dtheta from the gradient unit's sensitivity outputs (pdp_oc_predict_batched):
        returns NEW tensors x + X dtheta, u + U dtheta and - with `riccati` - lam_t + P_{t+1} X_{t+1} dtheta + W_{t+1} dtheta (else lam unchanged).
        dtheta [p] (shared) or [B, p].  What an IRL loop hands to oc_solve_ms(warm=...) at the next parameter."""
        torch = torch_cuda()
        x, u, lam = dev(x).clone(), dev(u).clone(), dev(lam).clone()
        B, T = u.shape[0], u.shape[1]
        dth, dtb = self._theta(dtheta, B)
        dxdp, dudp = dev(dxdp), dev(dudp)
        assert dxdp.shape == (B, T + 1, self.n, self.p) and dudp.shape == (B, T, self.m, self.p)
        ric = dev(riccati) if riccati is not None else None
        check(self.lib.pdp_oc_predict_batched(B, T, ptr(dth), dtb, ptr(dxdp), ptr(dudp), ptr(ric), ptr(x), ptr(u), ptr(lam) if ric is not None else None,
                                              current_stream_ptr()), "pdp_oc_predict_batched")
        return x, u, lam

    def _oc_pdp_grad_materialised(self, u, theta, demo_x, demo_u, x0, x, lam, flags, loss, grad, status, dxdp=None, dudp=None, grad_x0=None):
        """The PDP gradient unit by the reference's own route (PDP.py:272-314, 557-608 and the chain rule of cartpole_PDP.py:63-74), one
        kernel per stage: trajectory and costates (unless given), aux matrices to HBM, lqrSolver (column blocks for any p), contraction
        with (x - x_demo, u - u_demo) - or, with flags & PDP_OC_COTANGENT, with the cotangents that demo_x / demo_u then carry (row 0 of demo_x unread; no loss).
        Fills the given output tensors.  grad_x0 [B, n]: the initial state as n further parameters of the LQ system - zero columns in E, Hxe, Hue, hxe and
        X_0 = [0 | I] - whose columns of the sensitivities are contracted with the same cotangents (row 0 of demo_x included)."""
        torch = torch_cuda()
        B, T = u.shape[0], u.shape[1]
        n, m, p = self.n, self.m, self.p
        if not (flags & PDP_OC_GIVEN_TRAJ):
            x.copy_(self.oc_rollout(x0, u, theta, want_cost=False)[0])
            lam.copy_(self.oc_costate(x, u, theta))
        aux = self.oc_auxsys(x, u, lam, theta)
        if grad_x0 is None:
            X, U, _, st = lqr_solve(aux["dynF"], aux["dynG"], aux["Hxx"], aux["Huu"], aux["hxx"], aux["hxe"], E=aux["dynE"], Hxu=aux["Hxu"], Hxe=aux["Hxe"],
                                    Hue=aux["Hue"], want_costate=False)
        else:
            wide = lambda a: torch.cat([a, a.new_zeros(a.shape[:-1] + (n,))], dim=-1)
            X0 = torch.cat([u.new_zeros((n, p)), torch.eye(n, dtype=torch.float64, device="cuda")], dim=1)
            Xw, Uw, _, st = lqr_solve(aux["dynF"], aux["dynG"], aux["Hxx"], aux["Huu"], aux["hxx"], wide(aux["hxe"]), E=wide(aux["dynE"]), Hxu=aux["Hxu"],
                                      Hxe=wide(aux["Hxe"]), Hue=wide(aux["Hue"]), X0=X0, want_costate=False)
            X, U = Xw[..., :p].contiguous(), Uw[..., :p].contiguous()
        if flags & PDP_OC_COTANGENT:
            ex, eu = demo_x.clone(), demo_u
            ex[:, 0] = 0.0
        else:
            ex, eu = x - demo_x, u - demo_u
            loss.copy_((ex ** 2).sum(dim=(1, 2)) + (eu ** 2).sum(dim=(1, 2)))
        if grad_x0 is not None:
            ex_all = demo_x if flags & PDP_OC_COTANGENT else ex
            grad_x0.copy_(torch.einsum("bti,btik->bk", ex_all, Xw[..., p:]) + torch.einsum("bti,btik->bk", eu, Uw[..., p:]))
        g = torch.empty((B, p), dtype=torch.float64, device="cuda")
        core = load_core()
        ex_path, ex_fin, eu_c = ex[:, :T].contiguous(), ex[:, T].contiguous(), eu.contiguous()      # (named: they must outlive the launch)
        check(core.pdp_cp_grad_contract_batched(B, T, n, m, p, ptr(ex_path), ptr(eu_c), ptr(ex_fin), ptr(X), ptr(U), ptr(g), current_stream_ptr()),
              "pdp_cp_grad_contract_batched")
        grad.copy_(g)
        status.copy_(st)
        if dxdp is not None:
            dxdp.copy_(X)
        if dudp is not None:
            dudp.copy_(U)

    def oc_pdp_grad_materialised(self, u, theta, demo_x, demo_u, x0=None, x=None, lam=None, want_sens=False):
        """same results as oc_pdp_grad through the materialised kernels (getAuxSys -> lqrSolver -> chain rule): the reference's data flow"""
        torch = torch_cuda()
        u, demo_x, demo_u = dev(u), dev(demo_x), dev(demo_u)
        B, T = u.shape[0], u.shape[1]
        f64 = dict(dtype=torch.float64, device="cuda")
        flags = 0
        if x is not None:
            x, lam, flags = dev(x).clone(), dev(lam).clone(), PDP_OC_GIVEN_TRAJ
        else:
            x0 = dev(x0).reshape(B, self.n)
            x, lam = torch.empty((B, T + 1, self.n), **f64), torch.empty((B, T, self.n), **f64)
        loss, grad = torch.empty((B,), **f64), torch.empty((B, self.p), **f64)
        status = torch.zeros((B,), dtype=torch.int32, device="cuda")
        dxdp = torch.empty((B, T + 1, self.n, self.p), **f64) if want_sens else None
        dudp = torch.empty((B, T, self.m, self.p), **f64) if want_sens else None
        self._oc_pdp_grad_materialised(u, theta, demo_x, demo_u, x0, x, lam, flags, loss, grad, status, dxdp, dudp)
        out = dict(loss=loss, grad=grad, x=x, lam=lam, status=status)
        if want_sens:
            out.update(dxdp=dxdp, dudp=dudp)
        return out

    # -- ControlPlanning
    def cp_integrate(self, pol, p, x0, theta):
        torch = torch_cuda()
        x0 = dev(x0).reshape(-1, self.n)
        B = x0.shape[0]
        th, tb = self._theta(theta, B, p)
        T = self._T
        x = torch.empty((B, T + 1, self.n), dtype=torch.float64, device="cuda")
        u = torch.empty((B, T, self.m), dtype=torch.float64, device="cuda")
        cost = torch.empty((B,), dtype=torch.float64, device="cuda")
        rc = self.lib.pdp_cp_integrate_batched(B, T, C.byref(pol), p, ptr(x0), ptr(th), tb, ptr(x), ptr(u), ptr(cost), current_stream_ptr())
        if rc == PDP_E_SIZE:        # a network wider than the lane-per-trajectory integrator's local arrays: the size-generic step kernel rolls out as well (its gradient is dropped)
            loss, _, x, u = self.cp_step(pol, p, x0, th, T, want_traj=True)
            return x, u, loss
        check(rc, "pdp_cp_integrate_batched")
        return x, u, cost

    def cp_integrate_T(self, pol, p, x0, theta, T):
        self._T = int(T)
        return self.cp_integrate(pol, p, x0, theta)

    def cp_auxsys(self, pol, p, x, u, theta, want_cost_grads=True):
        torch = torch_cuda()
        x, u = dev(x), dev(u)
        B, T = u.shape[0], u.shape[1]
        n, m = self.n, self.m
        th, tb = self._theta(theta, B, p)
        e = lambda *s: torch.empty(s, dtype=torch.float64, device="cuda")
        out = dict(dynF=e(B, T, n, n), dynG=e(B, T, n, m), dUx=e(B, T, m, n), dUe=e(B, T, m, p))
        if want_cost_grads:
            out.update(dcx=e(B, T, n), dcu=e(B, T, m), dhx=e(B, n))
        check(self.lib.pdp_cp_auxsys_batched(B, T, C.byref(pol), p, ptr(x), ptr(u), ptr(th), tb, ptr(out["dynF"]), ptr(out["dynG"]), ptr(out["dUx"]),
                                             ptr(out["dUe"]), ptr(out.get("dcx")), ptr(out.get("dcu")), ptr(out.get("dhx")), current_stream_ptr()),
              "pdp_cp_auxsys_batched")
        return out

    def cp_step(self, pol, p, x0, theta, T, want_traj=False):
        """ControlPlanning.step (pdp_cp_step_batched): forward-sensitivity kernels for the Lagrange policy, adjoint kernels for the MLP
        policy, the size-generic adjoint kernel for everything beyond their limits and for table policies (the workspace any of them asks for is allocated here)."""
        torch = torch_cuda()
        x0 = dev(x0).reshape(-1, self.n)
        B = x0.shape[0]
        th, tb = self._theta(theta, B, p)
        loss = torch.empty((B,), dtype=torch.float64, device="cuda")
        grad = torch.empty((B, p), dtype=torch.float64, device="cuda")
        x = torch.empty((B, T + 1, self.n), dtype=torch.float64, device="cuda") if want_traj else None
        u = torch.empty((B, T, self.m), dtype=torch.float64, device="cuda") if want_traj else None
        nbytes = self.lib.pdp_cp_step_workspace_bytes(B, int(T), C.byref(pol), p)
        ws = torch.empty((nbytes // 8,), dtype=torch.float64, device="cuda") if nbytes > 0 else None
        rc = self.lib.pdp_cp_step_batched(B, int(T), C.byref(pol), p, ptr(x0), ptr(th), tb, ptr(loss), ptr(grad), ptr(x), ptr(u), ptr(ws), nbytes,
                                          current_stream_ptr())
        check(rc, "pdp_cp_step_batched")        # (no size is refused since round 5: what the tuned kernels do not take runs on the size-generic adjoint kernel)
        return (loss, grad, x, u) if want_traj else (loss, grad)

    def cp_step_materialised(self, pol, p, x0, theta, T, want_traj=False):
        """ControlPlanning.step exactly as the reference composes it (PDP.py:850-878): integrateSys -> getAuxSys ->
        integrateAuxSys (forward sensitivities, MFMA tiles over the parameter dimension) -> chain rule; every stage materialised in HBM."""
        torch = torch_cuda()
        x0 = dev(x0).reshape(-1, self.n)
        B = x0.shape[0]
        th, tb = self._theta(theta, B, p)
        x, u, loss = self.cp_integrate_T(pol, p, x0, th, T)
        aux = self.cp_auxsys(pol, p, x, u, th)
        X, U = cp_aux_integrate(aux["dynF"], aux["dynG"], aux["dUx"], aux["dUe"])
        grad = torch.empty((B, p), dtype=torch.float64, device="cuda")
        lib = load_core()
        check(lib.pdp_cp_grad_contract_batched(B, int(T), self.n, self.m, p, ptr(aux["dcx"]), ptr(aux["dcu"]), ptr(aux["dhx"]), ptr(X), ptr(U),
                                               ptr(grad), current_stream_ptr()), "pdp_cp_grad_contract_batched")
        return (loss, grad, x, u) if want_traj else (loss, grad)

    def cp_vjp_rows(self):
        """Pool rows (time steps per lane-parallel pass) of the ControlPlanning adjoint sweep, cp_vjp_kernel: csrc/pdp_sweep_pool.h's rule restated (no entry point
        reports it) - what a pool of SWEEP_POOL_DOUBLES holds of rows of PATH_NVAR + n + m + max(n + m, 16) doubles, made odd, at least 4 and at most 64.  PATH_NVAR, the number of
        variable entries of the `path` group, is read from the model's generated header.  The result bits do not depend on the rows: tests place their chunk edges by
        them."""
        import re
        from . import codegen
        src = open(os.path.join(codegen.GEN_DIR, self.name + ".h")).read()
        nvar = int(re.search(r"\bPATH_NVAR\s*=\s*(\d+)", src).group(1))
        stride = (nvar + self.n + self.m + max(self.n + self.m, 16)) | 1
        return min(64, max(4, SWEEP_POOL_DOUBLES // stride))

    def cp_rollout_vjp(self, pol, p, x, theta, grad_x, grad_u, want_theta=True, want_ini=True, force_materialised=False):
        """The rollout under a policy as a vector-Jacobian product (pdp_cp_step_batched with a pdp_policy_cot, include/pdp_hip.h: the semantics): x [B, T+1, n] the
        rollout of cp_integrate for theta ([p] or [B, p]), grad_x [B, T+1, n] = dL/dx, grad_u [B, T, m] = dL/du of any scalar loss L -> dict(grad_theta [B, p] = dL/dtheta
        per trajectory, grad_x0 [B, n] = dL/dx_0), one launch of the adjoint sweep.  want_theta / want_ini = False: that output is not computed.  Beyond the sweep's limits
        (PDP_E_SIZE: a table policy, n > 16, m > 4, p > 512, a network of more than 8 layers or 32 units) the forward sensitivities are materialised and contracted:
        no size is refused.  force_materialised: that route whatever the size (probes, tests).  Shape errors are ValueErrors before any foreign call."""
        sx, sg, su = _shape_of(x), _shape_of(grad_x), _shape_of(grad_u)
        if len(sx) != 3 or sx[2] != self.n or sx[0] < 1 or sx[1] < 2:
            raise ValueError("cp_rollout_vjp: state_traj must be [B, T+1, %d] with B, T >= 1, got %s" % (self.n, sx))
        B, T = sx[0], sx[1] - 1
        if sg != sx:
            raise ValueError("cp_rollout_vjp: grad_state must be [B, T+1, n] = %s, got %s" % (sx, sg))
        if su != (B, T, self.m):
            raise ValueError("cp_rollout_vjp: grad_control must be [B, T, m] = %s, got %s" % ((B, T, self.m), su))
        p = int(p)
        if _shape_of(theta) not in ((p,), (1, p), (B, p)):
            raise ValueError("cp_rollout_vjp: theta must be [p] or [B, p] with p = %d, B = %d, got %s" % (p, B, _shape_of(theta)))
        if not (want_theta or want_ini):
            raise ValueError("cp_rollout_vjp: want_theta and want_ini are both False - nothing to compute")
        torch = torch_cuda()
        x, gx, gu = dev(x), dev(grad_x), dev(grad_u)
        th, tb = self._theta(theta, B, p)
        out = {}
        if want_theta:
            out["grad_theta"] = torch.empty((B, p), dtype=torch.float64, device="cuda")
        if want_ini:
            out["grad_x0"] = torch.empty((B, self.n), dtype=torch.float64, device="cuda")
        rc = PDP_E_SIZE
        if not force_materialised:
            cot = PdpPolicyCot()
            C.memmove(C.byref(cot.pol), C.byref(pol), C.sizeof(PdpPolicy))
            cot.pol.kind = pol.kind | PDP_POLICY_COTANGENT
            cot.x, cot.grad_x, cot.grad_u = x.data_ptr(), gx.data_ptr(), gu.data_ptr()
            cot.grad_x0 = out["grad_x0"].data_ptr() if want_ini else None
            rc = self.lib.pdp_cp_step_batched(B, T, C.cast(C.byref(cot), C.POINTER(PdpPolicy)), p, None, ptr(th), tb, None, ptr(out.get("grad_theta")), None, None, None, 0,
                                              current_stream_ptr())
        if rc == PDP_E_SIZE:
            self._cp_rollout_vjp_materialised(pol, p, x, th, gx, gu, out)
            rc = 0
        check(rc, "pdp_cp_step_batched (PDP_POLICY_COTANGENT)")
        return out

    def _cp_rollout_vjp_materialised(self, pol, p, x, th, gx, gu, out):
        """cp_rollout_vjp through the materialised kernels: getAuxSys -> integrateAuxSys (forward sensitivities; for dL/dx_0 n further columns, zero in dUe, from
        X_0 = [0 | I]) -> the chain rule with the cotangents in the places of c_x, c_u, h_x"""
        torch = torch_cuda()
        B, T, n = x.shape[0], x.shape[1] - 1, self.n
        u = self.cp_integrate_T(pol, p, x[:, 0].contiguous(), th, T)[1]         # u_t = pi(t, x_t, theta) along the given rollout: x is that rollout
        aux = self.cp_auxsys(pol, p, x, u, th, want_cost_grads=False)
        dUe, X0, w = aux["dUe"], None, p
        if "grad_x0" in out:
            w = p + n
            dUe = torch.cat([dUe, dUe.new_zeros((B, T, self.m, n))], dim=-1).contiguous()
            X0 = torch.cat([x.new_zeros((n, p)), torch.eye(n, dtype=torch.float64, device="cuda")], dim=1).expand(B, n, w).contiguous()
        X, U = cp_aux_integrate(aux["dynF"], aux["dynG"], aux["dUx"], dUe, X0)
        g = torch.empty((B, w), dtype=torch.float64, device="cuda")
        gx_path, gx_fin = gx[:, :T].contiguous(), gx[:, T].contiguous()          # (named: they must outlive the launch)
        check(load_core().pdp_cp_grad_contract_batched(B, T, n, self.m, w, ptr(gx_path), ptr(gu), ptr(gx_fin), ptr(X), ptr(U), ptr(g), current_stream_ptr()),
              "pdp_cp_grad_contract_batched")
        if "grad_theta" in out:
            out["grad_theta"].copy_(g[:, :p])
        if "grad_x0" in out:
            out["grad_x0"].copy_(g[:, p:])

    def cp_jvp_rows(self):
        """Pool rows (time steps per lane-parallel pass) of the ControlPlanning tangent sweep, cp_jvp_kernel: csrc/pdp_sweep_pool.h's rule restated as cp_vjp_rows does,
        on the shorter row of CpJvpPool - PATH_NVAR + n + m doubles, made odd; what a pool of SWEEP_POOL_DOUBLES holds of them, at least 4 and at most 64.  The result
        bits do not depend on the rows: tests place their chunk edges by them."""
        import re
        from . import codegen
        src = open(os.path.join(codegen.GEN_DIR, self.name + ".h")).read()
        nvar = int(re.search(r"\bPATH_NVAR\s*=\s*(\d+)", src).group(1))
        stride = (nvar + self.n + self.m) | 1
        return min(64, max(4, SWEEP_POOL_DOUBLES // stride))

    def cp_rollout_jvp(self, pol, p, x, u, theta, d_theta=None, d_x0=None, want_control=True, force_materialised=False):
        """The rollout under a policy as a Jacobian-vector product (pdp_cp_step_batched with a pdp_policy_tan, include/pdp_hip.h: the semantics): x [B, T+1, n] and
        u [B, T, m] the rollout of cp_integrate for theta ([p] or [B, p]); the direction d_theta ([p]: shared by the batch, or [B, p]) and d_x0 [B, n], each None for
        zero, not both -> dict(d_state [B, T+1, n], d_control [B, T, m]), the tangent of the rollout along it, one launch of the tangent sweep
        d_u[t] = pi_x d_x[t] + pi_theta d_theta, d_x[t+1] = F_t d_x[t] + G_t d_u[t].  want_control=False: d_control is not stored.  Beyond the sweep's limits
        (PDP_E_SIZE: those of cp_rollout_vjp) ONE column of the forward sensitivities is integrated through the materialised kernels: no size is refused.
        force_materialised: that route whatever the size (probes, tests).  Shape errors are ValueErrors before any foreign call."""
        sx, su = _shape_of(x), _shape_of(u)
        if len(sx) != 3 or sx[2] != self.n or sx[0] < 1 or sx[1] < 2:
            raise ValueError("cp_rollout_jvp: state_traj must be [B, T+1, %d] with B, T >= 1, got %s" % (self.n, sx))
        B, T = sx[0], sx[1] - 1
        if su != (B, T, self.m):
            raise ValueError("cp_rollout_jvp: control_traj must be [B, T, m] = %s, got %s" % ((B, T, self.m), su))
        p = int(p)
        if _shape_of(theta) not in ((p,), (1, p), (B, p)):
            raise ValueError("cp_rollout_jvp: theta must be [p] or [B, p] with p = %d, B = %d, got %s" % (p, B, _shape_of(theta)))
        if d_theta is None and d_x0 is None:
            raise ValueError("cp_rollout_jvp: d_theta and d_x0 are both None - nothing to compute")
        if d_theta is not None and _shape_of(d_theta) not in ((p,), (1, p), (B, p)):
            raise ValueError("cp_rollout_jvp: d_theta must be [p] or [B, p] with p = %d, B = %d, got %s" % (p, B, _shape_of(d_theta)))
        if d_x0 is not None and _shape_of(d_x0) != (B, self.n):
            raise ValueError("cp_rollout_jvp: d_x0 must be [B, n] = %s, got %s" % ((B, self.n), _shape_of(d_x0)))
        torch = torch_cuda()
        x, u = dev(x), dev(u)
        th, tb = self._theta(theta, B, p)
        dth, dtb = self._theta(d_theta, B, p) if d_theta is not None else (None, 0)
        dx0 = dev(d_x0) if d_x0 is not None else None
        out = {"d_state": torch.empty((B, T + 1, self.n), dtype=torch.float64, device="cuda")}      # (every entry is written exactly once: no need to clear them)
        if want_control:
            out["d_control"] = torch.empty((B, T, self.m), dtype=torch.float64, device="cuda")
        rc = PDP_E_SIZE
        if not force_materialised:
            tan = PdpPolicyTan()
            C.memmove(C.byref(tan.pol), C.byref(pol), C.sizeof(PdpPolicy))
            tan.pol.kind = pol.kind | PDP_POLICY_TANGENT
            tan.x, tan.u, tan.d_x = x.data_ptr(), u.data_ptr(), out["d_state"].data_ptr()
            tan.d_theta, tan.d_theta_bstride = (dth.data_ptr() if dth is not None else None), dtb
            tan.d_x0 = dx0.data_ptr() if dx0 is not None else None
            tan.d_u = out["d_control"].data_ptr() if want_control else None
            rc = self.lib.pdp_cp_step_batched(B, T, C.cast(C.byref(tan), C.POINTER(PdpPolicy)), p, None, ptr(th), tb, None, None, None, None, None, 0,
                                              current_stream_ptr())
        if rc == PDP_E_SIZE:
            self._cp_rollout_jvp_materialised(pol, p, x, u, th, dth, dx0, out)
            rc = 0
        check(rc, "pdp_cp_step_batched (PDP_POLICY_TANGENT)")
        return out

    def _cp_rollout_jvp_materialised(self, pol, p, x, u, th, dth, dx0, out):
        """cp_rollout_jvp through the materialised kernels, on ONE column: getAuxSys, then dUe @ d_theta as a [B, T, m, 1] block, then integrateAuxSys from
        X_0 = d_x0[:, :, None]"""
        torch = torch_cuda()
        B, T = x.shape[0], x.shape[1] - 1
        aux = self.cp_auxsys(pol, p, x, u, th, want_cost_grads=False)
        if dth is None:
            col = x.new_zeros((B, T, self.m, 1))
        else:
            v = dth.reshape(-1, p)
            col = (aux["dUe"] @ (v[:, None, :, None] if v.shape[0] == B else v[0][:, None])).contiguous()
        X0 = (x.new_zeros((B, self.n, 1)) if dx0 is None else dx0[:, :, None]).contiguous()
        X, U = cp_aux_integrate(aux["dynF"], aux["dynG"], aux["dUx"], col, X0)
        out["d_state"].copy_(X[..., 0])
        if "d_control" in out:
            out["d_control"].copy_(U[..., 0])

    # -- SysID
    def sysid_integrate(self, x0, u, theta):
        torch = torch_cuda()
        x0, u = dev(x0).reshape(-1, self.n), dev(u)
        B, T = u.shape[0], u.shape[1]
        th, tb = self._theta(theta, B)
        x = torch.empty((B, T + 1, self.n), dtype=torch.float64, device="cuda")
        check(self.lib.pdp_sysid_integrate_batched(B, T, ptr(x0), ptr(u), ptr(th), tb, ptr(x), current_stream_ptr()), "pdp_sysid_integrate_batched")
        return x

    def sysid_auxsys(self, x, u, theta):
        torch = torch_cuda()
        x, u = dev(x), dev(u)
        B, T = u.shape[0], u.shape[1]
        th, tb = self._theta(theta, B)
        F = torch.empty((B, T, self.n, self.n), dtype=torch.float64, device="cuda")
        E = torch.empty((B, T, self.n, self.p), dtype=torch.float64, device="cuda")
        check(self.lib.pdp_sysid_auxsys_batched(B, T, ptr(x), ptr(u), ptr(th), tb, ptr(F), ptr(E), current_stream_ptr()), "pdp_sysid_auxsys_batched")
        return F, E

    def _check_rollout_shapes(self, who, u, theta, **trajs):
        """(B, T) of the inputs u [B, T, m] of `who` (sysid_rollout_vjp / sysid_rollout_jvp), after checking them, the [B, T+1, n] arrays `trajs` (by the name the
        message gives them) and theta; a ValueError otherwise"""
        su = _shape_of(u)
        if len(su) != 3 or su[2] != self.m or su[0] < 1 or su[1] < 1:
            raise ValueError("%s: inputs must be [B, T, %d] with B, T >= 1, got %s" % (who, self.m, su))
        B, T = su[0], su[1]
        for name, a in trajs.items():
            if _shape_of(a) != (B, T + 1, self.n):
                raise ValueError("%s: %s must be [B, T+1, n] = %s, got %s" % (who, name, (B, T + 1, self.n), _shape_of(a)))
        if _shape_of(theta) not in ((self.p,), (1, self.p), (B, self.p)):
            raise ValueError("%s: theta must be [p] or [B, p] with p = %d, B = %d, got %s" % (who, self.p, B, _shape_of(theta)))
        return B, T

    def _sweep_rows(self, entry, B):
        """pool rows of a sweep launch for a batch of B on this device, as the library's entry point `entry` reports them"""
        rows = int(getattr(self.lib, entry)(int(B)))
        if rows <= 0:
            raise RuntimeError("%s failed: %s" % (entry, PDP_E.get(rows, rows)))
        return rows

    def sysid_rollout_vjp(self, x, u, theta, grad_x, want_ini=True, want_theta=True, want_inputs=False):
        """The rollout as a vector-Jacobian product (pdp_sysid_rollout_vjp_batched, include/pdp_hip_sysid_vjp.h: the semantics): x [B, T+1, n] the rollout of
        sysid_integrate for u [B, T, m] and theta ([p] or [B, p]), grad_x [B, T+1, n] = dL/dx of any scalar loss L -> dict(grad_theta [B, p] = dL/dtheta per trajectory,
        grad_x0 [B, n] = dL/dx_0), one launch of the adjoint sweep.  want_ini / want_theta = False: that output is not computed.  want_inputs=True: also grad_u [B, T, m] =
        dL/du through the dynamics, from the same launch (pdp_sysid_rollout_vjp_u_batched, include/pdp_hip_sysid_vjp_u.h); without it the call is the one it always was.
        Not all three switches off.  Shape errors are ValueErrors before any launch."""
        B, T = self._check_rollout_shapes("sysid_rollout_vjp", u, theta, state_traj=x, grad_state=grad_x)
        if not (want_ini or want_theta or want_inputs):
            raise ValueError("sysid_rollout_vjp: want_theta, want_ini and want_inputs are all False - nothing to compute")
        torch = torch_cuda()
        x, u, g, th = dev(x), dev(u), dev(grad_x), dev(theta)
        tb = self.p if (th.dim() == 2 and th.shape[0] == B and B > 1) else 0
        out = {}
        if want_theta:
            out["grad_theta"] = torch.empty((B, self.p), dtype=torch.float64, device="cuda")
        if want_ini:
            out["grad_x0"] = torch.empty((B, self.n), dtype=torch.float64, device="cuda")
        if want_inputs:
            out["grad_u"] = torch.empty((B, T, self.m), dtype=torch.float64, device="cuda")       # (written exactly once per step: no need to clear it)
            check(self.lib.pdp_sysid_rollout_vjp_u_batched(B, T, ptr(x), ptr(u), ptr(th), tb, ptr(g), ptr(out["grad_theta"]) if want_theta else None,
                                                           ptr(out["grad_x0"]) if want_ini else None, ptr(out["grad_u"]), current_stream_ptr()),
                  "pdp_sysid_rollout_vjp_u_batched")
            return out
        check(self.lib.pdp_sysid_rollout_vjp_batched(B, T, ptr(x), ptr(u), ptr(th), tb, ptr(g), ptr(out["grad_theta"]) if want_theta else None,
                                                     ptr(out["grad_x0"]) if want_ini else None, current_stream_ptr()), "pdp_sysid_rollout_vjp_batched")
        return out

    def sysid_vjp_u_rows(self, B):
        """pool rows (time steps per Jacobian pass) of sysid_rollout_vjp's kernel with want_inputs=True for a batch of B on this device, as the library itself decides
        them (pdp_sysid_rollout_vjp_u_rows): the row there also holds the entries of G = df/du and m staging doubles, so the rows beyond four trajectories per
        compute unit are fewer than sysid_vjp_rows' - the chunk edges the tests aim at"""
        return self._sweep_rows("pdp_sysid_rollout_vjp_u_rows", B)

    def sysid_vjp_rows(self, B, cus):
        """pool rows (time steps per Jacobian pass) of sysid_rollout_vjp's kernel for a batch of B on a chip of `cus` compute units: the host's rule
        (sysid_vjp_rows_of, csrc/pdp_sweep_pool.h) restated - the chunk edges the tests aim at"""
        if B <= 4 * cus:
            return self.chunk
        fit = SWEEP_POOL_DOUBLES // ((self.nnz_path + self.n) | 1)
        return min(fit, self.chunk) if fit >= 4 else self.chunk

    def sysid_rollout_jvp(self, x, u, theta, d_theta=None, d_x0=None, d_u=None):
        """The rollout as a Jacobian-vector product (pdp_sysid_rollout_jvp_batched, include/pdp_hip_sysid_jvp.h: the semantics): x [B, T+1, n] the rollout of
        sysid_integrate for u [B, T, m] and theta ([p] or [B, p]); the direction d_theta ([p]: shared by the batch, or [B, p]), d_x0 [B, n], d_u [B, T, m], each None
        for zero, not all of them -> d_x [B, T+1, n], the tangent of the rollout along it: d_x[t+1] = F_t d_x[t] + E_t d_theta + G_t d_u[t], one launch of the tangent
        sweep.  Without d_u the kernel does not evaluate G = df/du.  Shape errors are ValueErrors before any launch."""
        B, T = self._check_rollout_shapes("sysid_rollout_jvp", u, theta, state_traj=x)
        if d_theta is None and d_x0 is None and d_u is None:
            raise ValueError("sysid_rollout_jvp: d_theta, d_x0 and d_u are all None - nothing to compute")
        if d_theta is not None and _shape_of(d_theta) not in ((self.p,), (1, self.p), (B, self.p)):
            raise ValueError("sysid_rollout_jvp: d_theta must be [p] or [B, p] with p = %d, B = %d, got %s" % (self.p, B, _shape_of(d_theta)))
        if d_x0 is not None and _shape_of(d_x0) != (B, self.n):
            raise ValueError("sysid_rollout_jvp: d_x0 must be [B, n] = %s, got %s" % ((B, self.n), _shape_of(d_x0)))
        if d_u is not None and _shape_of(d_u) != (B, T, self.m):
            raise ValueError("sysid_rollout_jvp: d_u must be [B, T, m] = %s, got %s" % ((B, T, self.m), _shape_of(d_u)))
        torch = torch_cuda()
        x, u, th = dev(x), dev(u), dev(theta)
        dth, dx0, du = (None if a is None else dev(a) for a in (d_theta, d_x0, d_u))
        tb = self.p if (th.dim() == 2 and th.shape[0] == B and B > 1) else 0
        dtb = self.p if (dth is not None and dth.dim() == 2 and dth.shape[0] == B and B > 1) else 0
        d_x = torch.empty((B, T + 1, self.n), dtype=torch.float64, device="cuda")                # (every row is written exactly once: no need to clear it)
        opt = lambda t: None if t is None else ptr(t)
        check(self.lib.pdp_sysid_rollout_jvp_batched(B, T, ptr(x), ptr(u), ptr(th), tb, opt(dth), dtb, opt(dx0), opt(du), ptr(d_x), current_stream_ptr()),
              "pdp_sysid_rollout_jvp_batched")
        return d_x

    def sysid_jvp_rows(self, B):
        """pool rows (time steps per Jacobian pass) of sysid_rollout_jvp's kernel for a batch of B on this device, as the library itself decides them
        (pdp_sysid_rollout_jvp_rows): sysid_vjp_rows' rule on the same row, with or without d_u - the chunk edges the tests aim at"""
        return self._sweep_rows("pdp_sysid_rollout_jvp_rows", B)

    def _sysid_workspace(self, B, T):
        """(workspace tensor or None, its bytes) of the fused SysID.step entry points"""
        torch = torch_cuda()
        nbytes = int(self.lib.pdp_sysid_step_workspace_bytes(B, T))              # > 0: large batch, the trajectories are rolled out beforehand, one lane each
        ws = None
        if nbytes > 0:
            # kept per (B, T): an SGD loop calls this every step, and a captured hipGraph (irl.GDLoop) holds the raw pointer - a buffer that a later, larger call freed
            # would leave the graph writing through a dangling pointer (round-4 advice).  Bounded (round-5 advice: a caller with ragged batches or horizon sweeps grew
            # one buffer per shape for the lifetime of the library): the eight most recently used shapes stay, and every shape that was used DURING a graph capture
            # stays for good (its pointer is baked into the graph).
            from collections import OrderedDict
            cache = self.__dict__.setdefault("_sysid_ws", OrderedDict())
            pinned = self.__dict__.setdefault("_sysid_ws_pinned", set())
            ws = cache.get((B, T))
            if ws is None:
                ws = cache[(B, T)] = torch.empty((nbytes // 8,), dtype=torch.float64, device="cuda")
            cache.move_to_end((B, T))
            if torch.cuda.is_current_stream_capturing():
                pinned.add((B, T))
            for key in [k for k in cache if k not in pinned][:max(0, len(cache) - len(pinned) - 8)]:
                del cache[key]
        return ws, nbytes

    def sysid_step(self, u, xobs, theta, gauss_newton=False, skip_missing=False, ini_state=None, buffers=None, estimate_ini=None, weights=None, huber_delta=None):
        """SysID.step per trajectory (pdp_sysid_step_ws_batched): (loss [B], grad [B, p]).  Models beyond the fused kernels' tiles (n > 16 or p > 64) take the reference's own
        route kernel by kernel - integrateDyn -> getAuxSys -> integrateAuxSys (size-generic kernels) -> the chain rule of PDP.py:1285-1291 as two tensor contractions: no size
        is refused.
        gauss_newton: the step as a nonlinear least-squares evaluation (pdp_sysid_step_gn_batched, one launch): returns dict(packed_gn [B, p + 1 + p p] = grad | loss | G
        per trajectory, and loss [B], grad [B, p], gn [B, p, p] as VIEWS of it), G = sum_t X_t' X_t the Gauss-Newton matrix of the loss (what irl.LMLoop.for_sysid
        averages).  skip_missing: a NaN in xobs is an entry that was not observed (PDP_GRAD_SKIP_MISSING): loss, gradient and G over the observed entries; a NaN in the
        initial state the rollouts would start from is a ValueError before any launch.  ini_state [B, n]: the initial state of the rollouts instead of xobs[:, 0]; row 0 then
        adds |ini_state - xobs_0|^2 to the loss.  skip_missing or ini_state without gauss_newton return (loss, grad) from the same launch.  Beyond the fused kernels' tiles
        (n > 16 or p > 16) the same row is contracted from the materialised sensitivities.  buffers: a dict the caller keeps - the output tensors are reused between calls.
        estimate_ini: ascending unique state indices or a bool mask [n] (ini_indices) - these q components of the initial state are unknowns beside theta
        (pdp_sysid_step_gn_ini_batched, one launch): the evaluation point is (theta, ini_state or xobs[:, 0]), the sensitivity of x0[i_k] is column p + k of the same tile,
        and every p above becomes W = p + q: (loss, grad [B, W]), or with gauss_newton the same dict over W plus ini_index (the list of indices).  An estimated component
        still needs a finite starting value (the NaN check of skip_missing stays).  W > 16 or n > 16: the same row from the materialised sensitivities started at the
        selection matrix.
        weights, huber_delta: weighted and Huber-robust least squares (pdp_sysid_step_wls_batched, one launch; either keyword implies the packed dict, like
        gauss_newton=True).  weights broadcast from [n], [T+1, n] (one block shared by the batch) or [B, T+1, n], finite and >= 0: w = 1 / sigma^2 per entry, 0 = not
        observed (xobs may hold anything there).  huber_delta > 0 acts on the standardised residual e = sqrt(w) (x - xobs): rho = e^2 up to delta, 2 delta |e| - delta^2
        beyond; loss = sum rho, grad its exact half derivative, gn the Gauss-Newton matrix of iteratively reweighted least squares (include/pdp_hip_sysid_wls.h).  They
        combine with skip_missing, ini_state and estimate_ini; W > 16 or n > 16: the same row from scaled residuals and row-scaled materialised sensitivities."""
        idx, _ = ini_indices(estimate_ini, self.n)
        weighted = weights is not None or huber_delta is not None
        if weighted or idx or gauss_newton or skip_missing or ini_state is not None:      # (nothing selected is estimate_ini=None: today's calls and today's rows)
            out = self.sysid_rows_prepared(u, xobs, skip_missing, ini_state, idx, weights, huber_delta, buffers)[0](theta)
            return out if gauss_newton or weighted else (out["loss"], out["grad"])
        torch = torch_cuda()
        u, xobs = dev(u), dev(xobs)
        B, T = u.shape[0], u.shape[1]
        th, tb = self._theta(theta, B)
        loss = torch.empty((B,), dtype=torch.float64, device="cuda")
        grad = torch.empty((B, self.p), dtype=torch.float64, device="cuda")
        ws, nbytes = self._sysid_workspace(B, T)
        rc = self.lib.pdp_sysid_step_ws_batched(B, T, ptr(u), ptr(xobs), ptr(th), tb, ptr(loss), ptr(grad), ptr(ws), nbytes, current_stream_ptr())
        if rc == PDP_E_SIZE:
            x = self.sysid_integrate(xobs[:, 0].contiguous(), u, th)
            F, E = self.sysid_auxsys(x, u, th)
            X = sysid_aux_integrate(F, E)                                           # [B, T+1, n, p]
            d = x - xobs
            return (d * d).sum(dim=(1, 2)), torch.einsum("bti,btip->bp", d, X)
        check(rc, "pdp_sysid_step_ws_batched")
        return loss, grad

    def _sysid_materialised(self, u, xobs, th, x0, ini_index=()):
        """(x [B, T+1, n], X [B, T+1, n, W]) from the size-generic kernels - sysid_integrate, sysid_auxsys, sysid_aux_integrate: the rollout from x0 (None: xobs[:, 0])
        and its sensitivities with respect to theta and the components ini_index of x0 (X_0 = the selection matrix; W = p + len(ini_index)).  What the Gauss-Newton
        entry points' rows are contracted from beyond the fused kernels' tile (PDP_E_SIZE).  Device tensors; th [1 or B, >= p]."""
        torch = torch_cuda()
        B, T, n, p = u.shape[0], u.shape[1], self.n, self.p
        if th.shape[-1] != p:                       # (parameters read in place from wider rows: theta_b | x0_b[idx])
            th = th[:, :p].contiguous()
        x = self.sysid_integrate(x0 if x0 is not None else xobs[:, 0].contiguous(), u, th)
        F, E = self.sysid_auxsys(x, u, th)
        if not ini_index:
            return x, sysid_aux_integrate(F, E)
        W = p + len(ini_index)
        Ew = torch.zeros((B, T, n, W), dtype=torch.float64, device="cuda")
        Ew[..., :p] = E
        X0 = torch.zeros((B, n, W), dtype=torch.float64, device="cuda")
        for k, i in enumerate(ini_index):
            X0[:, i, p + k] = 1.0
        return x, sysid_aux_integrate(F, Ew, X0)

    def _sysid_rows(self, u, xobs, th, tb, x0, buffers, skip_missing=False, ini_index=(), ini_mask=0, wls=None):
        """SysID.step as a least-squares evaluation on device tensors and normalised arguments, no check and no host synchronisation, ONE launch: what every Gauss-Newton
        mode of sysid_step and every evaluation of the loops of irl.py runs (sysid_rows_prepared marshals for it).  th [1 or B, >= p] with row stride tb (wider rows
        are read in place); x0 [B, n] or None (xobs[:, 0]); ini_index / ini_mask: the estimated components of x0 (ini_indices), W = p + q unknowns; wls: None, or
        (weights [T+1, n] or [B, T+1, n] or None, their batch stride, delta as a float) from wls_arguments.  Weights or delta go to pdp_sysid_step_wls_batched
        (buffer packed_gn_wls), estimated components to pdp_sysid_step_gn_ini_batched (packed_gn_ini), everything else to pdp_sysid_step_gn_batched (packed_gn).
        Returns the packed dict over W: packed_gn [B, W + 1 + W W] and loss, grad, gn as views of it, ini_index where components are estimated."""
        B, T, W = u.shape[0], u.shape[1], self.p + len(ini_index)
        bufs = buffers if buffers is not None else {}
        flags = PDP_GRAD_SKIP_MISSING if skip_missing else 0
        loss = _buffer(bufs, "loss", (B,))
        packed = _buffer(bufs, "packed_gn_wls" if wls is not None else ("packed_gn_ini" if ini_mask else "packed_gn"), (B, W + 1 + W * W))
        ws, nbytes = self._sysid_workspace(B, T)
        if wls is not None:
            name, (wd, wbs, delta) = "pdp_sysid_step_wls_batched", wls
            rc = self.lib.pdp_sysid_step_wls_batched(B, T, ptr(u), ptr(xobs), ptr(x0), ini_mask, ptr(wd), wbs, delta, ptr(th), tb, flags, ptr(loss), ptr(packed), ptr(ws),
                                                     nbytes, current_stream_ptr())
        elif ini_mask:
            name = "pdp_sysid_step_gn_ini_batched"
            rc = self.lib.pdp_sysid_step_gn_ini_batched(B, T, ptr(u), ptr(xobs), ptr(x0), ini_mask, ptr(th), tb, flags, ptr(loss), ptr(packed), ptr(ws), nbytes,
                                                        current_stream_ptr())
        else:
            name = "pdp_sysid_step_gn_batched"
            rc = self.lib.pdp_sysid_step_gn_batched(B, T, ptr(u), ptr(xobs), ptr(x0), ptr(th), tb, flags, ptr(loss), ptr(packed), ptr(ws), nbytes, current_stream_ptr())
        if rc == PDP_E_SIZE:                        # beyond the fused kernels' tile: the same row from the materialised sensitivities (started at the selection matrix)
            x, X = self._sysid_materialised(u, xobs, th, x0, ini_index)             # X [B, T+1, n, W]
            if wls is not None:
                packed_row_from_sensitivities(packed, [(x, xobs, wls[0], X)], "weighted", wls[2], skip_missing)
            else:
                packed_row_from_sensitivities(packed, [(x, xobs, None, X)], "missing_residual" if skip_missing else "plain")
            rc = 0
        check(rc, name)
        out = dict(packed_gn=packed, loss=packed[:, W], grad=packed[:, :W], gn=packed[:, W + 1:].view(B, W, W))
        if ini_index:
            out["ini_index"] = list(ini_index)
        return out

    def sysid_rows_prepared(self, u, xobs, skip_missing=False, ini_state=None, estimate_ini=None, weights=None, huber_delta=None, buffers=None, own_x0=False,
                            who="sysid_step", data_name="xobs"):
        """SysID.step's least-squares evaluation as a PREPARED call: the keywords of sysid_step are checked once (ValueErrors in the name of `who`, which calls xobs
        `data_name`), data and weights moved to the device once; the returned rows(theta) is then one launch per call, no check and no host synchronisation
        (_sysid_rows), and returns sysid_step's packed dict.  theta: [p] shared, [B, p] per sample, or - with estimate_ini and own_x0 - wide rows [B, W] = theta_b |
        x0_b[idx] as a device tensor: theta is read from them in place (row stride W) and the estimated components are copied into x0, one small device copy.
        own_x0: the initial states are a tensor of this call's own at a fixed address, started from ini_state or xobs[:, 0] - what wide rows are copied into, and
        what a caller with another layout of its unknowns writes the estimated components into itself between evaluations.  Returns (rows, held) with held =
        dict(u, xobs, x0, columns): the device tensors the evaluations read; columns the estimated components as an index tensor (None without own_x0 or them)."""
        idx, mask = ini_indices(estimate_ini, self.n)
        wls = wls_arguments(weights, huber_delta, int(u.shape[0]), int(u.shape[1]), self.n) if weights is not None or huber_delta is not None else None
        if skip_missing:
            refuse_nan_initial_state(who, xobs, ini_state, data_name)
        torch = torch_cuda()
        u, xobs = dev(u), dev(xobs)
        B, p = u.shape[0], self.p
        x0 = dev(ini_state).reshape(B, self.n).contiguous() if ini_state is not None else None
        if own_x0:
            x0 = (x0 if x0 is not None else xobs[:, 0]).contiguous().clone()
        if wls is not None and wls[0] is not None:
            wls = (dev(wls[0]).contiguous(),) + wls[1:]
        cols = torch.tensor(idx, dtype=torch.int64, device="cuda") if idx and own_x0 else None
        bufs = buffers if buffers is not None else {}

        def rows(theta):
            if cols is not None and hasattr(theta, "data_ptr") and theta.dim() == 2 and theta.shape[1] == p + len(idx):
                x0.index_copy_(1, cols, theta[:, p:])
                th, tb = theta, p + len(idx)
            else:
                th, tb = self._theta(theta, B)
            return self._sysid_rows(u, xobs, th, tb, x0, bufs, skip_missing, idx, mask, wls)
        return rows, dict(u=u, xobs=xobs, x0=x0, columns=cols)


def load_model(path):
    if path not in _models:
        _models[path] = ModelLib(path)
    return _models[path]
