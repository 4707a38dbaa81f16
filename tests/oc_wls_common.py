"""Shared by tests/test_gpu_oc_wls.py (in-process and in its child processes) and tests/test_oc_wls_host.py: weights, NaN marks and Huber thresholds for the inputs of
tests/oc_vjp_common.make_inputs, the three formulas of include/pdp_hip_oc_wls.h restated in torch fp64 and in numpy, and one shape of pdp_oc_pdp_grad_wls_batched through
every call it is compared with.

Samples of a batch: the last one has EVERY weight 0, the one before it has every weight 1 and no NaN; the others are weighted and marked."""
import numpy as np


def dark_sample(B):
    return B - 1


def ones_sample(B):
    return B - 2


def forced_zero(B, T, n, m):
    """(zx [B, T+1, n], zu [B, T, m]) bool, True where the weight is 0 for certain - the places tests/oc_missing_common.make_masks forces: row 0 of the states; one whole
    state row (t = T // 3) and one whole control row (t = 2 T // 3) in mid-horizon; states and controls on both sides of the middle chunk boundary (t = (T + 1) // 2 - 1
    and (T + 1) // 2); demo_u at t = 0 and T - 1; the even components of demo_x[:, T]."""
    zx, zu = np.zeros((B, T + 1, n), dtype=bool), np.zeros((B, T, m), dtype=bool)
    tb = (T + 1) // 2
    zx[:, 0] = True
    zx[:, T // 3] = True
    zu[:, (2 * T) // 3] = True
    zx[:, tb - 1:tb + 1] = True
    zu[:, tb - 1:tb + 1] = True
    zu[:, 0] = True
    zu[:, T - 1] = True
    zx[:, T, 0::2] = True
    return zx, zu


def make_weights(B, T, n, m, seed=23):
    """weights from {0 with probability 1/4} u [0.25, 4] (fixed seed), 0 at forced_zero, positive for certain at the odd components of row T; last sample all 0, the
    one before it all 1"""
    rng = np.random.default_rng(seed)
    wx = np.where(rng.random((B, T + 1, n)) < 0.25, 0.0, rng.uniform(0.25, 4.0, (B, T + 1, n)))
    wu = np.where(rng.random((B, T, m)) < 0.25, 0.0, rng.uniform(0.25, 4.0, (B, T, m)))
    wx[:, T, 1::2] = rng.uniform(0.25, 4.0, wx[:, T, 1::2].shape)
    zx, zu = forced_zero(B, T, n, m)
    wx[zx], wu[zu] = 0.0, 0.0
    wx[dark_sample(B)], wu[dark_sample(B)] = 0.0, 0.0
    wx[ones_sample(B)], wu[ones_sample(B)] = 1.0, 1.0
    return wx, wu


def weight_inputs(inp, skip, seed=23):
    """inp (oc_vjp_common.make_inputs) with the weights wx, wu, the NaN-marked demonstrations demo_xm / demo_um (NaN on half of the zero-weight entries; skip: also on a
    tenth of the positive-weight ones - not observed under PDP_GRAD_SKIP_MISSING), the zero-filled ones demo_x0 / demo_u0 and the observed-masks ox, ou.  The ones-sample
    holds no NaN."""
    B, T = inp["B"], inp["T"]
    n, m = inp["demo_x"].shape[2], inp["demo_u"].shape[2]
    wx, wu = make_weights(B, T, n, m, seed)
    rng = np.random.default_rng(seed + 1)
    out = dict(inp, wx=wx, wu=wu, skip=bool(skip))
    for k, w, d in (("x", wx, inp["demo_x"]), ("u", wu, inp["demo_u"])):
        nan = (w == 0) & (rng.random(w.shape) < 0.5)
        if skip:
            nan |= (w > 0) & (rng.random(w.shape) < 0.1)
        nan[ones_sample(B)] = False
        out["demo_%sm" % k], out["demo_%s0" % k], out["o" + k] = np.where(nan, np.nan, d), np.where(nan, 0.0, d), (w > 0) & ~nan
    return out


def huber_terms(xp, w, d, obs, delta):
    """e, psi-scaled s and rho of the header, entry by entry (xp: numpy or torch).  Entries that are not observed: s = 0, rho = 0 (selected, never multiplied)."""
    zero = 0.0 if xp is np else xp.zeros((), dtype=xp.float64, device=d.device)
    ws = xp.where(obs, w, zero + 1.0)                          # (a readable value where nothing is observed)
    e = xp.sqrt(ws) * xp.where(obs, d, zero)
    ae = xp.abs(e)
    quad = ae <= delta
    big = xp.where(quad, zero + 1.0, ae)                        # (no 0 / 0 on the quadratic branch)
    s = xp.where(obs, xp.sqrt(xp.where(quad, ws, ws * (delta / big))), zero)
    rho = xp.where(obs, xp.where(quad, e * e, 2.0 * delta * ae - delta * delta), zero)
    return ae, quad, s, rho


def median_delta(x, u, mi):
    """delta of a case: the median of |e| = sqrt(w) |d| over the observed entries of the whole batch (numpy, from a trajectory x and the controls u)"""
    ex = (np.sqrt(mi["wx"]) * np.abs(x - mi["demo_x0"]))[mi["ox"]]
    eu = (np.sqrt(mi["wu"]) * np.abs(u - mi["demo_u0"]))[mi["ou"]]
    return float(np.median(np.concatenate([ex, eu])))


def contract_wls(x, u, demo_x0, demo_u0, ox, ou, wx, wu, delta, dxdp, dudp, cap=True):
    """the three formulas of include/pdp_hip_oc_wls.h in torch fp64: (loss [B], grad [B, p], G [B, p, p]) from the trajectory, the zero-filled demonstrations, the
    observed-masks, the weights (None: ones), delta and the sensitivities.  cap (a finite delta): each Huber branch holds at least a quarter of the observed entries."""
    import torch
    one = torch.ones((), dtype=torch.float64, device=x.device)
    zero = torch.zeros((), dtype=torch.float64, device=x.device)
    sides = []
    for v, demo, obs, w, S in ((x, demo_x0, ox, wx, dxdp), (u, demo_u0, ou, wu, dudp)):
        d = v - demo
        ae, quad, s, rho = huber_terms(torch, (w if w is not None else one).expand(*d.shape), d, obs, delta)
        sides.append((rho.sum(dim=(1, 2)), torch.where(obs, s * d, zero), torch.where(obs[..., None], s[..., None] * S, zero), int((obs & quad).sum()), int((obs & ~quad).sum())))
    if cap and np.isfinite(delta):
        nq, nl = sides[0][3] + sides[1][3], sides[0][4] + sides[1][4]
        assert 4 * nq >= nq + nl and 4 * nl >= nq + nl, ("a Huber branch holds less than a quarter of the observed entries", nq, nl)
    loss = sides[0][0] + sides[1][0]
    grad = torch.einsum("bti,btip->bp", sides[0][1], sides[0][2]) + torch.einsum("bti,btip->bp", sides[1][1], sides[1][2])
    G = torch.einsum("btip,btiq->bpq", sides[0][2], sides[0][2]) + torch.einsum("btip,btiq->bpq", sides[1][2], sides[1][2])
    return loss, grad, G


def contract_wls_np(x, u, demo_x0, demo_u0, ox, ou, wx, wu, delta, X, U):
    """the same for ONE trajectory in numpy: (loss, grad [p], G [p, p]) from x [T+1, n], u [T, m], the sensitivities X [T+1, n, p], U [T, m, p]"""
    out = []
    for v, demo, obs, w, S in ((x, demo_x0, ox, wx, X), (u, demo_u0, ou, wu, U)):
        d = v - demo
        with np.errstate(invalid="ignore"):                     # (delta = +inf: inf 0 on the branch that is not selected)
            ae, quad, s, rho = huber_terms(np, np.broadcast_to(1.0 if w is None else w, d.shape), d, obs, delta)
        out.append((rho.sum(), np.where(obs, s * d, 0.0), np.where(obs[..., None], s[..., None] * S, 0.0)))
    return (out[0][0] + out[1][0], np.einsum("ti,tip->p", out[0][1], out[0][2]) + np.einsum("ti,tip->p", out[1][1], out[1][2]),
            np.einsum("tip,tiq->pq", out[0][2], out[0][2]) + np.einsum("tip,tiq->pq", out[1][2], out[1][2]))


def evaluate(mdl, inp, per_sample=False, given=False, skip=False):
    """The default unit (plain, with the sensitivities written, and its Gauss-Newton instantiation) on the zero-filled demonstrations, and the weighted unit on the
    NaN-marked ones: with weights and Huber's loss at delta = the median of |e| (rows_h), and with the weights alone (rows_w, delta = +inf).  given: the weighted calls
    get the default call's (x, lam) (PDP_OC_GIVEN_TRAJ), else they roll out from x0.  Output rows are pre-filled with NaN and followed by one guard row.  Returns numpy
    arrays; the reference is contract_wls() on the default unit's own outputs."""
    import torch
    from pdp_amd import runtime as rt
    mi = weight_inputs(inp, skip)
    th = mi["theta_b"] if per_sample else mi["theta"]
    u, x0 = rt.dev(mi["u"]), mi["x0"]
    dxm, dum, dx0, du0, wx, wu = (rt.dev(mi[k]) for k in ("demo_xm", "demo_um", "demo_x0", "demo_u0", "wx", "wu"))
    ox, ou = torch.as_tensor(mi["ox"], device="cuda"), torch.as_tensor(mi["ou"], device="cuda")
    B, p = u.shape[0], mdl.p
    d0 = mdl.oc_pdp_grad(u, th, dx0, du0, x0=x0)
    ds = mdl.oc_pdp_grad(u, th, dx0, du0, x0=x0, want_sens=True)
    g0 = mdl.oc_pdp_grad(u, th, dx0, du0, x0=x0, gauss_newton=True)              # (the ones-sample: no NaN, no weight, the same residuals)
    npy = lambda t: t.detach().cpu().numpy()
    delta = median_delta(npy(ds["x"]), mi["u"], mi)
    inf = float("inf")
    ref_h = contract_wls(ds["x"], u, dx0, du0, ox, ou, wx, wu, delta, ds["dxdp"], ds["dudp"])
    ref_w = contract_wls(ds["x"], u, dx0, du0, ox, ou, wx, wu, inf, ds["dxdp"], ds["dudp"])

    def traj():
        return dict(x=d0["x"].clone(), lam=d0["lam"].clone()) if given else dict(x0=x0)
    out = dict(delta=np.float64(delta), status0=npy(d0["status"]), x_def=npy(d0["x"]), lam_def=npy(d0["lam"]), gn_rows=npy(g0["packed_gn"]))
    for tag, dl, ref in (("h", delta, ref_h), ("w", None, ref_w)):
        rows = torch.full((B + 1, p + 1 + p * p), float("nan"), dtype=torch.float64, device="cuda")
        g = mdl.oc_pdp_grad(u, th, dxm, dum, weights_x=wx, weights_u=wu, huber_delta=dl, skip_missing=skip, buffers={"packed_gn": rows[:B]}, **traj())
        assert g["packed_gn"].data_ptr() == rows.data_ptr() and g["gn"].shape == (B, p, p) and g["grad"].shape == (B, p) and g["loss"].shape == (B,)
        out.update({"rows_" + tag: npy(rows), "status_" + tag: npy(g["status"]), "x_" + tag: npy(g["x"]), "lam_" + tag: npy(g["lam"]),
                    "loss_ref_" + tag: npy(ref[0]), "grad_ref_" + tag: npy(ref[1]), "G_ref_" + tag: npy(ref[2])})
    return out


def rel(a, b):
    """max|a - b| / max|b| of one sample's array (a scalar: |a - b| / |b|)"""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.abs(a - b).max() / np.abs(b).max())


# ---- corrupted demonstrations for the Levenberg-Marquardt tests (host: the CPU oracle; GPU: both loops)
def corrupt(state, control, seed=5, fraction=0.05):
    """5 % of the state and control entries, never row 0 of the states, moved by +-(0.5 .. 1.5), fixed seed: (demo_x, demo_u, cx, cu) with the bool masks of the
    corrupted entries"""
    rng = np.random.default_rng(seed)
    out = []
    for a, first in ((state, 1), (control, 0)):
        hit = rng.random(a.shape) < fraction
        hit[:, :first] = False
        move = rng.choice([-1.0, 1.0], a.shape) * rng.uniform(0.5, 1.5, a.shape)
        out.append((np.where(hit, a + move, a), hit))
    return out[0][0], out[1][0], out[0][1], out[1][1]


# ---- the CPU oracle on SOLVED OC problems (oracle/ipopt_ms.solve, then pdp_oracle.pdp_oc_unit on the solution's controls, then the formulas in numpy)
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HUBER_DELTA = 0.01                                  # delta of the Levenberg-Marquardt runs on the corrupted demonstrations
# irl.LMLoop at its default schedule on the CPU oracle (oracle_lm), evaluations: all demonstrations as one problem (tests/test_oc_wls_host.py asserts these), and with
# weight 0 on the corrupted entries one problem per demonstration (loss_tol = 1e-16)
PLAIN_COUNTS = {"pendulum": 36, "cartpole": 26}            # ends stalled at the non-zero minimum of the corrupted problem
HUBER_COUNTS = {"pendulum": 34, "cartpole": 28}            # likewise, delta = HUBER_DELTA
TRUST_COUNTS = {"pendulum": 6, "cartpole": 7}              # the clean problem again, none rejected
TRUST_COUNTS_PER_DEMO = {"pendulum": (7, 7, 7, 18, 12), "cartpole": (6, 6, 23, 7, 6)}
CORRUPTED_ENTRIES = {"pendulum": (15, 9), "cartpole": (39, 8)}   # corrupt(seed=5) on examples/data/demos_<system>.npz: (state entries, control entries)


def oracle_oc(system, _cache={}):
    from oracle import models, pdp_oracle as po
    if system not in _cache:
        st = models.IRL_SETUP[system]
        _cache[system] = po.make_oc(models.REGISTRY[system](**st["kwargs"]), st["dt"])
    return _cache[system]


def corrupted(system, _cache={}):
    """the stored demonstrations of examples/data with corrupt()'s outliers, the reference's own initial parameter, and the three weightings of the LM runs"""
    if system not in _cache:
        d = np.load(os.path.join(ROOT, "examples", "data", "demos_%s.npz" % system))
        theta0 = np.load(os.path.join(ROOT, "tests", "golden", "irltrace_head_%s.npz" % system))["param"][0]
        demo_x, demo_u, cx, cu = corrupt(d["state"], d["control"])
        _cache[system] = dict(system=system, clean_x=d["state"], clean_u=d["control"], demo_x=demo_x, demo_u=demo_u, cx=cx, cu=cu, theta0=theta0,
                              true_parameter=d["true_parameter"], x0=d["state"][:, 0].copy(), trust_x=np.where(cx, 0.0, 1.0), trust_u=np.where(cu, 0.0, 1.0))
    return _cache[system]


def oracle_rows(system, x0, theta, demo_x, demo_u, wx=None, wu=None, delta=float("inf"), skip=False, warm=None, tol=1e-10):
    """(loss [B], grad [B, p], G [B, p, p], solutions) of the weighted / Huber loss on re-solved OC problems, one per demonstration; warm: the solutions to start from"""
    from oracle import ipopt_ms, pdp_oracle as po
    oc = oracle_oc(system)
    B, T = demo_u.shape[0], demo_u.shape[1]
    rows, sols = [], []
    for b in range(B):
        s = ipopt_ms.solve(oc, x0[b], T, theta, tol=tol, warm=None if warm is None else warm[b])
        unit = po.pdp_oc_unit(oc, x0[b], s["control_traj_opt"], theta, np.nan_to_num(demo_x[b]), np.nan_to_num(demo_u[b]))
        ox = np.ones(demo_x[b].shape, bool) if wx is None else np.broadcast_to(wx, demo_x.shape)[b] > 0
        ou = np.ones(demo_u[b].shape, bool) if wu is None else np.broadcast_to(wu, demo_u.shape)[b] > 0
        if skip:
            ox, ou = ox & ~np.isnan(demo_x[b]), ou & ~np.isnan(demo_u[b])
        rows.append(contract_wls_np(np.asarray(unit["state_traj"]), np.asarray(s["control_traj_opt"]).reshape(T, -1), np.where(ox, demo_x[b], 0.0), np.where(ou, demo_u[b], 0.0),
                                    ox, ou, None if wx is None else np.broadcast_to(wx, demo_x.shape)[b], None if wu is None else np.broadcast_to(wu, demo_u.shape)[b], delta,
                                    np.stack(unit["lqr"]["state_traj_opt"]), np.stack(unit["lqr"]["control_traj_opt"])))
        sols.append((s["state_traj_opt"], s["control_traj_opt"], s["costate_traj_opt"]))
    return np.array([r[0] for r in rows]), np.stack([r[1] for r in rows]), np.stack([r[2] for r in rows]), sols


def oracle_lm(system, mode, max_evals=50, loss_tol=0.0, samples=None):
    """irl.LMLoop at its default schedule on the CPU oracle, the evaluation of LMLoop.for_irl restated (warm solves from copies of the last accepted solutions, the mean
    row): mode "plain" (unit weights), "huber" (HUBER_DELTA) or "trust" (weight 0 on the corrupted entries).  samples: the demonstrations of the problem (default: all).  Returns results()."""
    from pdp_amd.irl import LMLoop
    c = corrupted(system)
    if samples is not None:
        c = dict(c, **{k: c[k][list(samples)] for k in ("x0", "demo_x", "demo_u", "trust_x", "trust_u")})
    kw = dict(plain={}, huber=dict(delta=HUBER_DELTA), trust=dict(wx=c["trust_x"], wu=c["trust_u"]))[mode]
    state = {"accepted": None, "trial": None}

    def evaluate(theta):
        loss, grad, G, sols = oracle_rows(system, c["x0"], theta, c["demo_x"], c["demo_u"], warm=state["accepted"], **kw)
        state["trial"] = sols
        return loss.mean(), grad.mean(axis=0), G.mean(axis=0)
    loop = LMLoop(evaluate, c["theta0"])
    loop.on_accept = lambda: state.update(accepted=state["trial"])
    return loop.run(max_evals=max_evals, loss_tol=loss_tol)


def theta_error(r, system):
    return float(np.abs(r["parameter_trace"][-1] - corrupted(system)["true_parameter"]).max())
