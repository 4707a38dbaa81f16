"""Shared by tests/test_tile_edge_modes_inputs.py (CPU) and tests/test_gpu_tile_edge_modes.py (GPU, in-process and in its child processes): the fused OC unit's
masked (skip_missing), weighted / Huber and initial-state (want_ini) modes on the three models of tests/tile_edge_common.py - horizons at every chunk length a mode
runs with, masks and weights placed by those chunks, and references formed from the oracle alone.

Layouts, restated from the code generator's counts (tile_edge_common.generated_info):
    pair kernels    Fused3Layout<Mdl, XW> (csrc/pdp_fused3_kernels.h) through tile_edge_common.fused3_layout(info, xw): XW = 0, and XW = n + m in the weighted mode, whose
                    forward rows hold the n + m scales (ROWSF 39 -> 28 for E16, 40 -> 30 for E15, 64 -> 64 for E5; ROWS stays 22 / 22 / 42)
    one-wave kernel FusedLayout<Mdl, XW> (csrc/pdp_model_kernels.h): backward and forward chunks both hold Mdl::CHUNK steps whatever XW (40 / 40 / 64) - XW makes the
                    forward row longer, and with it the pool, not the chunk
    x0 sweep        OcX0VjpPool<Mdl> (csrc/pdp_sweep_pool.h): rows = what 2400 doubles hold of rows of (SOLF_NVAR + n m + n + m) | 1, at least 4, at most 64
                    (25 / 32 / 64)
Every sweep cuts T steps into ceil(T / R) chunks of ceil(T / nchunk) steps, the last one short (chunk_starts).

Samples of a batch (B = 5), as in tests/oc_missing_common.py and tests/oc_wls_common.py: the last one is dark (nothing observed), the one before it is fully
observed, the others are masked.  Nothing here runs a kernel or reads a kernel's output: Huber's threshold is the median of the standardised residuals on the ORACLE's
rollout."""
import functools

import numpy as np

import oc_wls_common as wls
import oc_x0_vjp_common as cx0
import tile_edge_common as c

NAMES = sorted(c.MODELS)
B = c.B_UNIT
DARK, FULL = B - 1, B - 2
MASKED = tuple(range(B - 2))
LOSS_TOL = 1e-12
P_OBSERVED = 0.6             # of the entries no rule decides (the rules below take a quarter to a third of a long horizon away)


# ---- layouts ------------------------------------------------------------------------------------------------------------------------------------------------
def xw_of(info):
    """extra words of a forward row in the weighted mode: the n + m scales"""
    return info["n"] + info["m"]


def one_wave_layout(info, xw=0):
    """FusedLayout<Mdl, XW>: CH steps per chunk in both sweeps (FusedChunk: Mdl::CHUNK, no dependence on XW), the row strides and the pool in doubles"""
    n, m, nv = info["n"], info["m"], info["nvar"]
    bs, fs = (nv["patha"] + nv["pathb"] + n) | 1, (nv["fwd"] + n + m + xw) | 1
    return dict(CH=info["chunk"], BSTRIDE=bs, FSTRIDE=fs, POOL=max(info["chunk"] * max(bs, fs), nv["fin"] + 1))


def x0_rows(info):
    """oc_x0_vjp_rows_of(OcX0VjpPool<Mdl>::STRIDE)"""
    n, m = info["n"], info["m"]
    stride = (info["nvar"]["solf"] + n * m + n + m) | 1
    return min(64, max(4, 2400 // stride))


def chunk_starts(T, rows):
    """first steps of the chunks behind the first one: ceil(T / rows) chunks of ceil(T / nchunk) steps"""
    nchunk = -(-T // rows)
    ch = -(-T // nchunk)
    return [k * ch for k in range(1, nchunk)]


def sweep_rows(info):
    """steps per chunk of every sweep a mode of the unit runs, by what it is: the masks and scales live in the forward rows, the costates in the backward ones"""
    xw = xw_of(info)
    f0, fw = c.fused3_layout(info), c.fused3_layout(info, xw)
    return {"pair backward": f0["ROWS"], "pair backward, weighted": fw["ROWS"], "pair forward": f0["ROWSF"], "pair forward, weighted": fw["ROWSF"],
            "one-wave": one_wave_layout(info)["CH"], "one-wave, weighted": one_wave_layout(info, xw)["CH"], "x0 sweep": x0_rows(info)}


def boundaries(info, T):
    """{sweep: first steps of its chunks behind the first} at horizon T"""
    return {k: chunk_starts(T, r) for k, r in sweep_rows(info).items()}


def route(info, T, xw=0):
    """what oc_pdp_launch<Mdl, XW> does at PDP_FUSED_VARIANT=3 (csrc/pdp_model.hip): "refused" (PDP_E_SIZE: the host then contracts materialised sensitivities),
    "pair" (oc_pdp_fused3_kernel) or "one-wave" """
    if not c.fused_accepts(info, T, xw):
        return "refused"
    return "pair" if c.fused3_ok(info, T, xw) else "one-wave"


def horizons(info):
    """tile_edge_common.unit_horizons (1, 7, ROWS + 6, ROWS + 7), R - 1, R, R + 1 for R the forward chunk of the pair kernels at XW = 0 and at XW = n + m, of the
    one-wave kernel with and without the extra words, and the rows of the x0 sweep, and 2 R + 1 for the x0 sweep - without what the unit refuses or routes away from the
    pair kernels at XW = 0 (the weighted mode's route is asserted, not assumed: tests/test_tile_edge_modes_inputs.py)"""
    rows = sweep_rows(info)
    hs = set(c.unit_horizons(info))
    for k in ("pair forward", "pair forward, weighted", "one-wave", "one-wave, weighted", "x0 sweep"):
        hs |= {rows[k] - 1, rows[k], rows[k] + 1}
    hs.add(2 * rows["x0 sweep"] + 1)
    return tuple(sorted(T for T in hs if T >= 1 and route(info, T) == "pair"))


# ---- masks and weights --------------------------------------------------------------------------------------------------------------------------------------
def _rng(name, T, salt):
    return np.random.default_rng([salt, c.MODELS[name][0], T])


@functools.lru_cache(maxsize=None)
def make_masks(name, T):
    """(wx [B, T+1, n], wu [B, T, m]) bool, True = observed, on unit_inputs(name, T).  P_OBSERVED of the entries are observed (fixed seed) but for the rules, later
    ones first:  the last sample dark, the one before it fully observed;  row T of the states: even components missing, odd ones observed;  state component n - 1 missing
    at t = 0, 2, 4 .. < T and observed at t = 1 (at odd n its row T is missing too: without this the seed decides whether it is observed at all);  all controls at t = 0 and T - 1 missing;  states and controls of the two steps on either side of EVERY chunk boundary of every sweep
    (boundaries(): backward, forward, forward in the weighted mode, one-wave, x0 sweep) missing;  one whole state row (t = T // 3) and one whole control row
    (t = 2 T // 3) missing;  all of row 0 of the states missing."""
    n, m, _ = c.MODELS[name]
    rng = _rng(name, T, 11)
    wx, wu = rng.random((B, T + 1, n)) < P_OBSERVED, rng.random((B, T, m)) < P_OBSERVED
    wx[:, 0] = False
    wx[:, T // 3] = False
    wu[:, (2 * T) // 3] = False
    for t0s in boundaries(c.generated_info(name), T).values():
        for t0 in t0s:
            wx[:, t0 - 1:t0 + 1] = False
            wu[:, t0 - 1:t0 + 1] = False
    wu[:, 0] = False
    wu[:, T - 1] = False
    wx[:, 0:T:2, n - 1] = False
    wx[:, 1, n - 1] = True
    wx[:, T, 0::2] = False
    wx[:, T, 1::2] = True
    wx[DARK], wu[DARK] = False, False
    wx[FULL], wu[FULL] = True, True
    for a in (wx, wu):
        a.setflags(write=False)
    return wx, wu


@functools.lru_cache(maxsize=None)
def make_weights(name, T):
    """(Wx [B, T+1, n], Wu [B, T, m]): log-uniform in [1e-2, 1e2] (fixed seed); EXACT zeros on the missing entries of sample 0's mask and on all of the dark sample"""
    n, m, _ = c.MODELS[name]
    rng = _rng(name, T, 23)
    Wx, Wu = 10.0 ** rng.uniform(-2.0, 2.0, (B, T + 1, n)), 10.0 ** rng.uniform(-2.0, 2.0, (B, T, m))
    mx, mu = make_masks(name, T)
    Wx[0][~mx[0]], Wu[0][~mu[0]] = 0.0, 0.0
    Wx[DARK], Wu[DARK] = 0.0, 0.0
    for a in (Wx, Wu):
        a.setflags(write=False)
    return Wx, Wu


# The calls of the weighted unit, by tag: (weights on the state side, on the control side, Huber, skip_missing, where the demonstrations are NaN).
#   shapes: "B" [B, T+1, n] / [B, T, m];  "T" ONE block [T+1, n] / [T, m], sample 0's (with its zeros);  "n" [n] / [m], a row of sample 1 (all positive);  None: not given
#   NaN:    "zero" where the weight is 0 - WITHOUT skip_missing: weight 0 is not observed and the NaN must not surface;  "mask" where make_masks says missing;  None
WEIGHTED = {
    "w":   ("B", "B", False, False, "zero"),        # weights on both sides, huber_delta off
    "wh":  ("T", "T", True, False, "zero"),         # weights plus Huber
    "whs": ("B", "B", True, True, "mask"),          # weights plus Huber plus skip_missing on the NaN-marked demonstrations
    "h":   (None, None, True, False, None),         # Huber alone
    "wx":  ("n", None, False, False, None),         # weights on one side only: the states ...
    "wu":  (None, "n", True, False, None),          # ... and the controls, with Huber
}
DARK_IN = ("w", "whs")                              # the calls in which the last sample has nothing observed


def masked_demos(name, T):
    """(demo_x, demo_u) of unit_inputs(name, T) with NaN on the missing entries of make_masks"""
    inp = c.unit_inputs(name, T)
    mx, mu = make_masks(name, T)
    return np.where(mx, inp["demo_x"], np.nan), np.where(mu, inp["demo_u"], np.nan)


def weighted_case(name, T, tag):
    """dict of one call of WEIGHTED, without its threshold: weights_state / weights_control as they are passed (or None), huber, skip_missing, demo_x / demo_u as they
    are passed (NaN-marked), and for the reference Wx [B, T+1, n], Wu [B, T, m] (ones where none are given) and the observed-masks ox, ou"""
    sx, su, huber, skip, nan = WEIGHTED[tag]
    inp = c.unit_inputs(name, T)
    out = dict(huber=huber, skip_missing=skip)
    mask = dict(zip("xu", make_masks(name, T)))
    for k, shape, W, demo in (("x", sx, make_weights(name, T)[0], inp["demo_x"]), ("u", su, make_weights(name, T)[1], inp["demo_u"])):
        given = {None: None, "B": W, "T": W[0], "n": W[1][W.shape[1] // 2]}[shape]
        full = np.ones(W.shape) if given is None else np.broadcast_to(given, W.shape)
        assert shape != "n" or (given > 0).all()
        bad = {None: np.zeros(W.shape, dtype=bool), "zero": full == 0, "mask": ~mask[k]}[nan]
        out["weights_" + ("state" if k == "x" else "control")] = given
        out["W" + k], out["demo_" + k], out["o" + k] = full, np.where(bad, np.nan, demo), (full > 0) & ~(bad if skip else np.zeros_like(bad))
        assert not (np.isnan(out["demo_" + k]) & out["o" + k]).any()            # a NaN never sits on an observed entry: it must not surface
    return out


@functools.lru_cache(maxsize=None)
def oracle_rollout(name, T, per_sample):
    """[B, T+1, n]: OCSysOracle.rollout of every sample - the state_traj of unit_oracle (tests/test_tile_edge_modes_inputs.py holds them equal to the bit), without the
    unit behind it"""
    inp = c.unit_inputs(name, T)
    oc = c.model_oracle(name)
    x = np.stack([np.asarray(oc.rollout(inp["x0"][b], inp["u"][b], c.theta_of(inp, per_sample, b)), dtype=float) for b in range(B)])
    x.setflags(write=False)
    return x


def standardised(name, T, per_sample, case):
    """(|e| of the states [B, T+1, n], of the controls [B, T, m]) = sqrt(w) |residual| on the oracle's rollout, 0 where nothing is observed"""
    inp = c.unit_inputs(name, T)
    x = oracle_rollout(name, T, per_sample)
    ex = np.where(case["ox"], np.sqrt(case["Wx"]) * np.abs(x - np.where(case["ox"], case["demo_x"], 0.0)), 0.0)
    eu = np.where(case["ou"], np.sqrt(case["Wu"]) * np.abs(inp["u"] - np.where(case["ou"], case["demo_u"], 0.0)), 0.0)
    return ex, eu


def huber_delta(name, T, per_sample, tag):
    """the threshold of a call: the median of the standardised residuals over the observed entries of the batch - halfway between two neighbouring entries at the middle - from
    the ORACLE's rollout; None where Huber is off"""
    case = weighted_case(name, T, tag)
    if not case["huber"]:
        return None
    ex, eu = standardised(name, T, per_sample, case)
    e = np.sort(np.concatenate([ex[case["ox"]], eu[case["ou"]]]))
    mid = e.size // 2                       # (an odd count: between the middle entry and the next one - the median itself would BE an entry, and the rounding of a
    return float(0.5 * (e[mid - 1] + e[mid]) if e.size % 2 == 0 else 0.5 * (e[mid] + e[mid + 1]))     # kernel's rollout would decide its branch)


def all_deltas(names=NAMES):
    """{"<name>_<T>_<per_sample>_<tag>": threshold} of every call with Huber's loss - what the parent hands to the child processes, which form no reference themselves"""
    return {"%s_%d_%d_%s" % (name, T, ps, tag): huber_delta(name, T, ps, tag) for name in names for T in horizons(c.generated_info(name)) for ps in (0, 1)
            for tag in WEIGHTED if WEIGHTED[tag][2]}


# ---- references ---------------------------------------------------------------------------------------------------------------------------------------------
def sensitivities(name, T, per_sample, b):
    """(x [T+1, n], X [T+1, n, p], U [T, m, p]) of sample b from tile_edge_common.unit_oracle"""
    o = c.unit_oracle(name, T, per_sample, b)
    return np.asarray(o["state_traj"], dtype=float), np.stack(o["lqr"]["state_traj_opt"]), np.stack(o["lqr"]["control_traj_opt"])


def contract(x, u, demo_x, demo_u, ox, ou, Wx, Wu, delta, X, U):
    """(loss, half gradient [p], G [p, p]) of ONE sample by the formulas of include/pdp_hip_oc_wls.h (oc_wls_common.contract_wls_np); weights None and delta = +inf:
    the formulas of PDP_GRAD_SKIP_MISSING, include/pdp_hip.h (tests/test_tile_edge_modes_inputs.py holds this against oc_missing_common.contract)"""
    return wls.contract_wls_np(x, u, np.where(ox, demo_x, 0.0), np.where(ou, demo_u, 0.0), ox, ou, Wx, Wu, float("inf") if delta is None else delta, X, U)


def masked_reference(name, T, per_sample, b):
    """the skip_missing unit on masked_demos: (loss, grad, G) of sample b"""
    inp = c.unit_inputs(name, T)
    x, X, U = sensitivities(name, T, per_sample, b)
    mx, mu = make_masks(name, T)
    return contract(x, inp["u"][b], inp["demo_x"][b], inp["demo_u"][b], mx[b], mu[b], None, None, None, X, U)


def weighted_reference(name, T, per_sample, b, tag):
    """the weighted unit on weighted_case(tag) at huber_delta(tag): (loss, grad, G) of sample b"""
    inp = c.unit_inputs(name, T)
    case = weighted_case(name, T, tag)
    x, X, U = sensitivities(name, T, per_sample, b)
    return contract(x, inp["u"][b], case["demo_x"][b], case["demo_u"][b], case["ox"][b], case["ou"][b], case["Wx"][b], case["Wu"][b],
                    huber_delta(name, T, per_sample, tag), X, U)


@functools.lru_cache(maxsize=None)
def x0_sensitivities(name, T, per_sample, b):
    """(dx_t/dx_0 [T+1, n, n], du_t/dx_0 [T, m, n]): oc_x0_vjp_common.forward_sensitivities on the oracle's auxiliary system - what reference_grad_x0 contracts, kept so
    that the two cotangent sets of a sample share one padded solve"""
    return cx0.forward_sensitivities(c.model_oracle(name), c.unit_oracle(name, T, per_sample, b)["aux"], T)


def x0_reference(name, T, per_sample, b):
    """(grad_x0 of the cotangent unit on gx, gu;  grad_x0 of the default unit: the residuals x - demo_x, u - demo_u as cotangents, row 0 included) - each the
    contraction of oc_x0_vjp_common.reference_grad_x0"""
    inp = c.unit_inputs(name, T)
    Xx, Ux = x0_sensitivities(name, T, per_sample, b)
    x = np.asarray(c.unit_oracle(name, T, per_sample, b)["state_traj"], dtype=float)
    pair = lambda gx, gu: np.einsum("ti,tik->k", gx, Xx) + np.einsum("ti,tik->k", gu, Ux)
    return pair(inp["gx"][b], inp["gu"][b]), pair(x - inp["demo_x"][b], inp["u"][b] - inp["demo_u"][b])
