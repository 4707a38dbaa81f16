"""CPU: the conditions under which tests/test_gpu_tile_edge_modes.py means something, checked on the oracle and the code generator alone (no compiling, no GPU).

1. Horizons: each model's set as literals - a change of a layout (Fused3Layout<Mdl, XW>, FusedLayout, OcX0VjpPool, the code generator's counts) fails here and does not
   silently move the coverage.  Every horizon runs the pair kernels in BOTH layouts (XW = 0, and XW = n + m of the weighted mode) and fits the one-wave kernel; every sweep
   has a horizon of exactly one chunk and one of exactly two.
2. Masks: the certain entries are as tile_edge_modes_common.make_masks states them - the two steps at every chunk boundary of every sweep among them; every state and
   control component is both observed and missing over time in every masked sample (T >= 7: at T = 1 row 0 and both control rules leave (n // 2) / (2 n + m) of the
   entries, so there the batch as a whole is looked at); 25 % .. 75 % of a masked sample are observed (T >= 7, for the same reason).
3. Weights: log-uniform in [1e-2, 1e2], exact zeros where stated, a NaN on every zero weight of the calls without skip_missing and on no observed entry.
4. Huber: in every sample that is neither dark nor fully observed each branch holds at least 20 % of the observed entries, and no entry lies within 1e-6 (relative) of
   the threshold - the kernel's rollout differs from the oracle's by rounding, and that must not move an entry to the other branch.
5. Reference accuracy (REF_CAP = 1e-12): loss, gradient and G formed from the fp64 oracle against the same contractions of the 40-digit X, U carried out in mpmath; the
   grad_x0 reference (the reference's padded forward solve) against oc_x0_vjp_common.adjoint_sweep, another method.  At T = 7 and at the longest horizon of each model.
6. No empty comparison: no row or column of G's reference vanishes in a masked sample."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import oc_x0_vjp_common as cx0  # noqa: E402
import tile_edge_common as c  # noqa: E402
import tile_edge_modes_common as k  # noqa: E402

NAMES = k.NAMES
HORIZONS = {"E16": (1, 7, 24, 25, 26, 27, 28, 29, 38, 39, 40, 41, 51), "E15": (1, 7, 28, 29, 30, 31, 32, 33, 39, 40, 41, 65), "E5": (1, 7, 48, 49, 63, 64, 65, 129)}
ROWS = {"E16": {"pair backward": 22, "pair backward, weighted": 22, "pair forward": 39, "pair forward, weighted": 28, "one-wave": 40, "one-wave, weighted": 40, "x0 sweep": 25},
        "E15": {"pair backward": 22, "pair backward, weighted": 22, "pair forward": 40, "pair forward, weighted": 30, "one-wave": 40, "one-wave, weighted": 40, "x0 sweep": 32},
        "E5": {"pair backward": 42, "pair backward, weighted": 42, "pair forward": 64, "pair forward, weighted": 64, "one-wave": 64, "one-wave, weighted": 64, "x0 sweep": 64}}


def _cases(name):
    return [(T, ps) for T in k.horizons(c.generated_info(name)) for ps in (False, True)]


@pytest.mark.parametrize("name", NAMES)
def test_horizon_sets_and_routes(name):
    info = c.generated_info(name)
    xw = k.xw_of(info)
    assert xw == sum(c.MODELS[name][:2])
    assert k.sweep_rows(info) == ROWS[name]
    hs = k.horizons(info)
    assert hs == HORIZONS[name]
    assert set(c.unit_horizons(info)) <= set(hs)
    for T in hs:
        # the weighted mode's longer rows route no horizon away from the pair kernels (oc_pdp_launch<Mdl, XW>), and the one-wave kernel takes every one as well
        assert k.route(info, T) == "pair" and k.route(info, T, xw) == "pair", (name, T)
        assert c.fused3_ok(info, T) and c.fused3_ok(info, T, xw) and c.fused_accepts(info, T) and c.fused_accepts(info, T, xw), (name, T)
    # the one-wave kernel's pool grows with XW, its chunk does not
    assert k.one_wave_layout(info, xw)["FSTRIDE"] > k.one_wave_layout(info)["FSTRIDE"] and k.one_wave_layout(info, xw)["CH"] == k.one_wave_layout(info)["CH"] == info["chunk"]
    for sweep, R in ROWS[name].items():
        if sweep.startswith("pair backward"):
            continue                                                # (ROWS + 6 and ROWS + 7 of tile_edge_common: two backward chunks; none of the horizons is one full chunk)
        nch = {T: len(k.chunk_starts(T, R)) + 1 for T in hs}
        assert nch[R] == 1 and nch[R + 1] == 2 and R - 1 in hs, (name, sweep, nch)
    R = ROWS[name]["x0 sweep"]
    assert len(k.chunk_starts(2 * R + 1, R)) == 2                                                      # three chunks of the x0 sweep
    assert k.chunk_starts(7, 4) == [4] and k.chunk_starts(9, 4) == [3, 6] and k.chunk_starts(8, 4) == [4] and k.chunk_starts(4, 4) == []
    for T in hs:                                                    # the restated backward chunks are tile_edge_common's
        assert [T - sum(c.backward_chunks(info, T)[:i]) for i in range(1, len(c.backward_chunks(info, T)))][::-1] == k.chunk_starts(T, ROWS[name]["pair backward"])


@pytest.mark.parametrize("name", NAMES)
def test_masks_hold_the_certain_entries(name):
    n, m, _ = c.MODELS[name]
    info = c.generated_info(name)
    for T in k.horizons(info):
        wx, wu = k.make_masks(name, T)
        assert wx.shape == (k.B, T + 1, n) and wu.shape == (k.B, T, m) and wx.dtype == bool and wu.dtype == bool
        assert not wx[k.DARK].any() and not wu[k.DARK].any() and wx[k.FULL].all() and wu[k.FULL].all()
        bounds = k.boundaries(info, T)
        assert set(bounds) == set(ROWS[name])
        for b in k.MASKED:
            assert not wx[b, 0].any()
            assert not wx[b, T, 0::2].any() and wx[b, T, 1::2].all()
            assert not wx[b, 0:T:2, n - 1].any() and (wx[b, 1, n - 1] or (T == 1 and n % 2 == 1))
            assert not wx[b, T // 3].any() or T // 3 == T
            assert not wu[b, (2 * T) // 3].any() and not wu[b, 0].any() and not wu[b, T - 1].any()
            for sweep, t0s in bounds.items():
                assert len(t0s) == -(-T // ROWS[name][sweep]) - 1
                for t0 in t0s:
                    assert 1 <= t0 < T
                    assert not wx[b, t0 - 1].any() and not wu[b, t0 - 1].any() and not wu[b, t0].any(), (name, T, sweep, t0)
                    assert not wx[b, t0].any() or t0 == T
            if T >= 7:
                assert (wx[b].any(axis=0) & ~wx[b].all(axis=0)).all() and (wu[b].any(axis=0) & ~wu[b].all(axis=0)).all(), (name, T, b)
                frac = (wx[b].sum() + wu[b].sum()) / (wx[b].size + wu[b].size)
                assert 0.25 <= frac <= 0.75, (name, T, b, frac)
        assert (wx.any(axis=(0, 1)) & ~wx.all(axis=(0, 1))).all() and (wu.any(axis=(0, 1)) & ~wu.all(axis=(0, 1))).all()
        dx, du = k.masked_demos(name, T)
        assert np.array_equal(np.isnan(dx), ~wx) and np.array_equal(np.isnan(du), ~wu)


@pytest.mark.parametrize("name", NAMES)
def test_weights_and_their_calls(name):
    n, m, _ = c.MODELS[name]
    assert set(k.DARK_IN) <= set(k.WEIGHTED)
    for T in k.horizons(c.generated_info(name)):
        Wx, Wu = k.make_weights(name, T)
        mx, mu = k.make_masks(name, T)
        for W, mk in ((Wx, mx), (Wu, mu)):
            pos = W[W > 0]
            assert (W >= 0).all() and pos.min() >= 1e-2 and pos.max() <= 1e2
            assert np.array_equal(W[0] == 0, ~mk[0]) and not W[k.DARK].any() and (W[1:k.DARK] > 0).all()
        assert np.log10(Wx[Wx > 0]).std() > 0.9 or T == 1                # (log-uniform over four decades: 4 / sqrt(12) = 1.15)
        shapes = {"x": set(), "u": set()}
        for tag in k.WEIGHTED:
            case = k.weighted_case(name, T, tag)
            for side, key, full in (("x", "weights_state", (k.B, T + 1, n)), ("u", "weights_control", (k.B, T, m))):
                w = case[key]
                if w is not None:
                    assert w.shape in (full, full[1:], full[2:])
                    shapes[side].add(len(w.shape))
                    assert np.array_equal(np.broadcast_to(w, full), case["W" + side])
                else:
                    assert (case["W" + side] == 1).all()
                nan = np.isnan(case["demo_" + side])
                assert not (nan & case["o" + side]).any()
                if not case["skip_missing"]:
                    assert np.array_equal(nan, case["W" + side] == 0) or not nan.any()           # weight 0 without the flag: the NaN must not surface
                    assert np.array_equal(case["o" + side], case["W" + side] > 0)
                else:
                    assert np.array_equal(nan, ~(mx if side == "x" else mu))
                    assert np.array_equal(case["o" + side], (case["W" + side] > 0) & ~nan)
            dark = not case["ox"][k.DARK].any() and not case["ou"][k.DARK].any()
            assert dark == (tag in k.DARK_IN)
        assert shapes == {"x": {1, 2, 3}, "u": {1, 2, 3}}                                            # [n], [T+1, n], [B, T+1, n] and likewise for the controls
        w = k.weighted_case(name, T, "w")
        assert np.isnan(w["demo_x"]).sum() == (Wx == 0).sum() > 0 and np.isnan(w["demo_u"]).sum() == (Wu == 0).sum() > 0
        hs = [tag for tag in k.WEIGHTED if k.WEIGHTED[tag][2]]
        assert {k.WEIGHTED[t][:2] for t in hs} >= {("T", "T"), ("B", "B"), (None, None)} and any(k.WEIGHTED[t][3] for t in hs)


@pytest.mark.parametrize("name", NAMES)
def test_huber_thresholds_split_every_sample(name):
    """the threshold is formed from the oracle's rollout (which is unit_oracle's state_traj to the bit), never from a kernel's output"""
    worst_split, worst_gap = 1.0, np.inf
    T0 = k.horizons(c.generated_info(name))[1]
    for ps in (False, True):
        assert np.array_equal(k.oracle_rollout(name, T0, ps)[0], np.asarray(c.unit_oracle(name, T0, ps, 0)["state_traj"], dtype=float))
    for T, ps in _cases(name):
        for tag in k.WEIGHTED:
            delta = k.huber_delta(name, T, ps, tag)
            if not k.WEIGHTED[tag][2]:
                assert delta is None
                continue
            case = k.weighted_case(name, T, tag)
            ex, eu = k.standardised(name, T, ps, case)
            assert delta > 0 and np.isfinite(delta)
            for b in range(k.B):
                e = np.concatenate([ex[b][case["ox"][b]], eu[b][case["ou"][b]]])
                if e.size == 0:
                    continue
                gap = np.abs(e - delta).min() / delta
                worst_gap = min(worst_gap, gap)
                assert gap > 1e-6, (name, T, ps, tag, b, gap)
                partly = e.size < ex[b].size + eu[b].size
                if b != k.DARK and b != k.FULL and partly and T >= 7:               # (T = 1: four to eighteen observed entries a sample)
                    lo = (e <= delta).mean()
                    worst_split = min(worst_split, lo, 1 - lo)
                    assert 0.2 <= lo <= 0.8, (name, T, ps, tag, b, lo)
    print("%s: smallest Huber branch %.3f of a sample's observed entries, nearest entry %.2e (relative) from its threshold" % (name, worst_split, worst_gap))


def _mp_contract(x, u, demo_x, demo_u, ox, ou, Wx, Wu, delta, X, U):
    """tile_edge_modes_common.contract in 40-digit arithmetic (mpmath): object arrays, products and sums of mpf"""
    import mpmath as mp
    f = np.vectorize(lambda v: mp.mpf(float(v)), otypes=[object])
    loss, grad, G = mp.mpf(0), 0, 0
    for v, demo, obs, W, S in ((x, demo_x, ox, Wx, X), (u, demo_u, ou, Wu, U)):
        idx = np.argwhere(obs)
        if len(idx) == 0:
            continue
        d = f(v[obs]) - f(demo[obs])
        w = f(np.ones(v.shape)[obs] if W is None else W[obs])
        e = np.array([mp.sqrt(wi) * abs(di) for wi, di in zip(w, d)], dtype=object)
        quad = np.array([ei <= delta for ei in e]) if delta is not None else np.ones(len(e), dtype=bool)
        s2 = np.array([wi if q else wi * delta / ei for wi, q, ei in zip(w, quad, e)], dtype=object)
        loss += sum(ei * ei if q else 2 * delta * ei - delta * delta for ei, q in zip(e, quad))
        Sm = f(S[obs])                                              # [observed entries, p]
        grad = grad + (s2 * d) @ Sm
        G = G + Sm.T @ (s2[:, None] * Sm)
    return loss, grad, G


@pytest.mark.parametrize("name", NAMES)
def test_references_are_accurate(name):
    import mpmath as mp
    hs = k.horizons(c.generated_info(name))
    worst = {}

    def note(what, v):
        worst[what] = max(worst.get(what, 0.0), float(v))
        assert v <= c.REF_CAP, (name, what, v)
    old = mp.mp.dps
    mp.mp.dps = 40
    try:
        for T, ps, b in ((7, False, 0), (hs[-1], True, 1)):
            inp = c.unit_inputs(name, T)
            x, X, U = k.sensitivities(name, T, ps, b)
            Xe, Ue = c.unit_exact(name, T, ps, b)
            note("X", c.rel(X, Xe))
            note("U", c.rel(U, Ue))
            mx, mu = k.make_masks(name, T)
            calls = [("masked", k.masked_reference(name, T, ps, b), (inp["demo_x"][b], inp["demo_u"][b], mx[b], mu[b], None, None, None))]
            for tag in k.WEIGHTED:
                case = k.weighted_case(name, T, tag)
                delta = k.huber_delta(name, T, ps, tag)
                calls.append((tag, k.weighted_reference(name, T, ps, b, tag), (case["demo_x"][b], case["demo_u"][b], case["ox"][b], case["ou"][b], case["Wx"][b], case["Wu"][b],
                                                                               None if delta is None else mp.mpf(delta))))
            for tag, (loss, grad, G), args in calls:
                le, ge, Ge = _mp_contract(x, inp["u"][b], *args, Xe, Ue)
                tofl = np.vectorize(float, otypes=[float])
                note("loss (%s)" % tag, abs(loss - float(le)) / float(le))
                note("gradient (%s)" % tag, c.rel(grad, tofl(ge)))
                note("G (%s)" % tag, c.rel(G, tofl(Ge)))
            aux = c.unit_oracle(name, T, ps, b)["aux"]
            for ref, (gx, gu) in zip(k.x0_reference(name, T, ps, b), ((inp["gx"][b], inp["gu"][b]), (x - inp["demo_x"][b], inp["u"][b] - inp["demo_u"][b]))):
                note("grad_x0 vs adjoint_sweep", c.rel(ref, cx0.adjoint_sweep(aux, gx, gu)))
                assert np.array_equal(ref, cx0.reference_grad_x0(c.model_oracle(name), None, inp["u"][b], None, None, gx, gu, aux=aux))
    finally:
        mp.mp.dps = old
    for what, v in worst.items():
        print("%s: reference vs 40 digits / another method, %s %.2e" % (name, what, v))


@pytest.mark.parametrize("name", NAMES)
def test_masked_reference_is_the_formula_of_the_header_and_not_empty(name):
    """contract() with no weights and no threshold is oc_missing_common.contract (torch, on the CPU) - and in the masked samples no row or column of G's reference is zero"""
    import torch
    import oc_missing_common as cm
    n, m, p = c.MODELS[name]
    for T, ps in _cases(name):
        inp = c.unit_inputs(name, T)
        mx, mu = k.make_masks(name, T)
        for b in k.MASKED:
            loss, grad, G = k.masked_reference(name, T, ps, b)
            if T >= 7:
                assert (np.abs(G).max(axis=0) > 0).all() and np.abs(grad).min() > 0 and loss > 0, (name, T, ps, b)
            if (T, b) in ((7, 0), (k.horizons(c.generated_info(name))[-1], 1)):
                x, X, U = k.sensitivities(name, T, ps, b)
                t = lambda a: torch.as_tensor(np.array(a))[None]
                l2, g2, G2 = cm.contract(t(x), t(inp["u"][b]), t(np.where(mx[b], inp["demo_x"][b], 0.0)), t(np.where(mu[b], inp["demo_u"][b], 0.0)), t(mx[b]), t(mu[b]), t(X), t(U))
                assert abs(float(l2[0]) - loss) <= 1e-14 * loss and c.rel(g2[0].numpy(), grad) <= 1e-14 and c.rel(G2[0].numpy(), G) <= 1e-14
        for tag in k.WEIGHTED:
            for b in k.MASKED:
                loss, grad, G = k.weighted_reference(name, T, ps, b, tag)
                assert loss > 0 and (T == 1 or (np.abs(G).max(axis=0) > 0).all()), (name, T, ps, tag, b)
        for tag in k.DARK_IN:
            loss, grad, G = k.weighted_reference(name, T, ps, k.DARK, tag)
            assert loss == 0 and not grad.any() and not G.any()


@pytest.mark.parametrize("name", NAMES)
def test_one_misread_entry_at_a_chunk_boundary_would_show(name):
    """the comparison has teeth where it is aimed: at the first horizon of two forward chunks of each layout, ONE missing entry beside the boundary taken as observed - a
    mask or a zero weight read from the neighbouring row, say - moves loss, gradient and G of the reference by more than a thousand times the tolerances they are held to"""
    info = c.generated_info(name)
    for sweep in ("pair forward", "pair forward, weighted", "one-wave"):
        T = ROWS[name][sweep] + 1
        (t0,) = k.chunk_starts(T, ROWS[name][sweep])
        inp = c.unit_inputs(name, T)
        x, X, U = k.sensitivities(name, T, False, 0)
        mx, mu = k.make_masks(name, T)
        case = k.weighted_case(name, T, "w")
        for t in (t0 - 1, t0):
            for side in ("x", "u"):
                ox, ou = mx[0].copy(), mu[0].copy()
                wx, wu = case["Wx"][0].copy(), case["Wu"][0].copy()
                (ox if side == "x" else ou)[t, 0] = True
                (wx if side == "x" else wu)[t, 0] = 1.0
                ref = k.masked_reference(name, T, False, 0)
                got = k.contract(x, inp["u"][0], inp["demo_x"][0], inp["demo_u"][0], ox, ou, None, None, None, X, U)
                refw = k.weighted_reference(name, T, False, 0, "w")
                gotw = k.contract(x, inp["u"][0], inp["demo_x"][0], inp["demo_u"][0], wx > 0, wu > 0, wx, wu, None, X, U)
                for r, g in ((ref, got), (refw, gotw)):
                    assert abs(g[0] - r[0]) / r[0] > 1e3 * k.LOSS_TOL, (name, sweep, t, side)
                    assert c.rel(g[1], r[1]) > 1e3 * c.TOL and c.rel(g[2], r[2]) > 1e3 * c.TOL, (name, sweep, t, side, c.rel(g[1], r[1]), c.rel(g[2], r[2]))
