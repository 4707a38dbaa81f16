"""GPU: the fused OC unit's masked (skip_missing), weighted / Huber (pdp_oc_pdp_grad_wls_batched) and initial-state (want_ini: oc_x0_vjp_kernel behind the launch) modes
at the far end of the sizes the unit advertises - the three models of tests/tile_edge_common.py (n = 16, 15, 5; m + p = 16: the [control | parameter] tile full to its
last column), where tests/test_gpu_oc_missing.py, test_gpu_oc_wls.py and test_gpu_oc_x0_vjp.py run on the zoo (n = 2, 4, 13) and against the default unit's own
sensitivities.  Here every sample of every call is judged against references formed from the oracle alone (tests/tile_edge_modes_common.py; its conditions:
tests/test_tile_edge_modes_inputs.py).

Horizons (tile_edge_modes_common.horizons): those of tests/test_gpu_tile_edge.py and R - 1, R, R + 1 for every forward chunk length R a mode runs with - the pair
kernels' at XW = 0 and in the weighted mode's longer rows, the one-wave kernel's, the x0 sweep's rows - and 2 R + 1 of the x0 sweep.  Masks and zero weights lie on both
sides of every chunk boundary.  The calls of tests/test_gpu_tile_edge.py (plain, want_sens + want_riccati, cotangent, Gauss-Newton) run again at these horizons and are
judged by its _judge_unit: none of its own horizons spans two forward chunks.

One child process per kernel selection (test_gpu_tile_edge.ENV: default, tpw2, tpw4, one_wave), each under its own time limit; after a child that died or ran out of
time nothing more is started on the device.  A child forms no reference: Huber's thresholds come from the parent (the oracle's rollout), the child saves an .npz, the
parent judges it.  Through the class surface (OCSys.pdp_grad_batch / pdp_vjp_batch; PDP_OC_PACKED, which it does not offer, through OCSys.model().oc_pdp_grad), output
rows pre-filled with NaN and followed by one guard row.  A call that leaves the fused kernels (the materialised route warns) fails the child.

Judged, per sample: gradient, grad_x0 and G to 1e-10 of the largest entry (tile_edge_common.TOL), losses to 1e-12 relative, through `margins`:
one line per (selection, model, horizon, quantity).  Exact: status 0; G symmetric; guard rows NaN, rows finite; the dark sample all zeros; the fully observed sample
under skip_missing equal to the call without the flag; x and lam of every call equal to the plain call's; grad with want_ini equal to grad without; the packed, plain
and Gauss-Newton rows of the masked unit equal in loss and gradient - all to the bit.  tpw2 and tpw4 equal default to the bit in every output."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import test_gpu_tile_edge as te  # noqa: E402
import tile_edge_common as c  # noqa: E402
import tile_edge_modes_common as k  # noqa: E402

NAMES = k.NAMES
MODES = te.UNIT_MODES
CHILD_TIMEOUT = 300
built = te.built                 # (the fixture: the three model libraries, the ones tests/test_gpu_tile_edge.py builds)
MASKED_CALLS = ("ms", "mp", "mg")       # skip_missing alone, with PDP_OC_PACKED, with want_gauss_newton
KEYS_PER_CASE = 18 + 5 * len(MASKED_CALLS) + 5 * len(k.WEIGHTED) + 5 + 6


def _key(name, T, per_sample, given):
    return "%s_%d_%d_%d_" % (name, T, per_sample, given)


# ---- child process ------------------------------------------------------------------------------------------------------------------------------------------
def _modes(out, name, oc, deltas):
    """every case of one model: the masked unit (alone, packed, Gauss-Newton), the six calls of the weighted unit, the cotangent and the default unit with want_ini - after
    test_gpu_tile_edge._unit has run the old calls of the same case, whose (x, lam) the given-trajectory calls are handed"""
    import torch
    from pdp_amd import runtime as rt
    n, m, p = c.MODELS[name]
    B = k.B
    nan = float("nan")
    hs = k.horizons(oc._model_info)
    te._unit(out, name, oc, hs)
    for T, per_sample, given in te._cases(oc._model_info, hs):
        inp = c.unit_inputs(name, T)
        th = inp["theta_b"] if per_sample else inp["theta"]
        key = _key(name, T, per_sample, given)
        u = rt.dev(inp["u"])
        traj = lambda: dict(state_traj=rt.dev(out[key + "x"]), costate_traj=rt.dev(out[key + "lam"])) if given else dict(ini_state=inp["x0"])
        low = lambda: dict(x=rt.dev(out[key + "x"]), lam=rt.dev(out[key + "lam"])) if given else dict(x0=inp["x0"])
        guard = lambda w: torch.full((B + 1, w), nan, dtype=torch.float64, device="cuda")

        def save(tag, res, **rows):
            for kk, v in rows.items():
                out[key + tag + "_" + kk] = te.npy(v)
            for kk in ("loss", "status", "x", "lam"):
                if kk in res:
                    out[key + tag + "_" + kk] = te.npy(res[kk])
        # masked
        dxm, dum = (rt.dev(a) for a in k.masked_demos(name, T))
        g = guard(p)
        r = oc.pdp_grad_batch(u, th, dxm, dum, skip_missing=True, buffers={"grad": g[:B]}, **traj())
        assert r["grad"].data_ptr() == g.data_ptr()
        save("ms", r, rows=g)
        g = guard(p + 1)
        r = oc.model().oc_pdp_grad(u, th, dxm, dum, skip_missing=True, packed=True, buffers={"packed": g[:B]}, **low())
        assert r["packed"].data_ptr() == g.data_ptr()
        save("mp", r, rows=g)
        g = guard(p + 1 + p * p)
        r = oc.pdp_grad_batch(u, th, dxm, dum, skip_missing=True, want_gauss_newton=True, buffers={"packed_gn": g[:B]}, **traj())
        assert r["packed_gn"].data_ptr() == g.data_ptr()
        save("mg", r, rows=g)
        # weighted
        for tag in k.WEIGHTED:
            case = k.weighted_case(name, T, tag)
            delta = deltas["%s_%d_%d_%s" % (name, T, per_sample, tag)] if case["huber"] else None
            g = guard(p + 1 + p * p)
            r = oc.pdp_grad_batch(u, th, rt.dev(case["demo_x"]), rt.dev(case["demo_u"]), weights_state=case["weights_state"], weights_control=case["weights_control"],
                                  huber_delta=delta, skip_missing=case["skip_missing"], buffers={"packed_gn": g[:B]}, **traj())
            assert r["packed_gn"].data_ptr() == g.data_ptr()
            save(tag, r, rows=g)
        # initial state
        g = guard(n)
        r = oc.pdp_vjp_batch(u, th, inp["gx"], inp["gu"], want_ini=True, buffers={"grad_x0": g[:B]}, **traj())
        assert r["grad_x0"].data_ptr() == g.data_ptr()
        save("vi", r, rows=g, grad=r["grad"])
        g = guard(n)
        r = oc.pdp_grad_batch(u, th, rt.dev(inp["demo_x"]), rt.dev(inp["demo_u"]), want_ini=True, buffers={"grad_x0": g[:B]}, **traj())
        assert r["grad_x0"].data_ptr() == g.data_ptr()
        save("gi", r, rows=g, grad=r["grad"])


def _worker(mode, deltas_file):
    """runs in a child process whose environment selects the kernels; every entry point returned 0 (runtime.check raises otherwise) and none left the fused kernels"""
    import warnings
    warnings.simplefilter("error", RuntimeWarning)              # (ModelLib._warn_materialised: PDP_E_SIZE answered by the kernel-by-kernel route)
    with open(deltas_file) as f:
        deltas = json.load(f)
    out = {}
    ocs = {name: c.model_gpu(name) for name in NAMES}
    for name in NAMES:
        ocs[name].model()
        info = ocs[name]._model_info
        xw = k.xw_of(info)
        assert (info["n"], info["m"], info["p"]) == c.MODELS[name]
        assert all(k.route(info, T) == "pair" and k.route(info, T, xw) == "pair" for T in k.horizons(info))
    for name in NAMES:
        t0 = time.time()
        _modes(out, name, ocs[name], deltas)
        print("modes %s done in %.1f s" % (name, time.time() - t0), flush=True)
    return out


# ---- parent -------------------------------------------------------------------------------------------------------------------------------------------------
_results, _stopped, _wall = {}, [], {}


@pytest.fixture(scope="module")
def run(built, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("tile_edge_modes")
    deltas_file = os.path.join(str(tmp), "deltas.json")
    with open(deltas_file, "w") as f:
        json.dump(k.all_deltas(), f)

    def _run(mode):
        if mode not in _results:
            # a child that died (a fault, a time limit) ends the GPU work of this module: nothing more is started on the device
            assert not _stopped, "not started: the child process of mode %r failed before" % _stopped[0]
            f = os.path.join(str(tmp), mode + ".npz")
            code = ("import sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_tile_edge_modes as m; np.savez(%r, **m._worker(%r, %r))"
                    % (ROOT, HERE, f, mode, deltas_file))
            env = {kk: v for kk, v in os.environ.items() if kk not in ("PDP_FUSED_VARIANT", "PDP_FUSED_TPW", "PDP_MS_VARIANT")}
            t0 = time.time()
            try:
                r = subprocess.run([sys.executable, "-c", code], env=dict(env, **te.ENV[mode]), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=CHILD_TIMEOUT)
            except subprocess.TimeoutExpired:
                _stopped.append(mode)
                raise
            _wall[mode] = time.time() - t0
            print("child %s: %.1f s of wall time\n%s" % (mode, _wall[mode], r.stdout[-600:]))
            if r.returncode != 0:
                _stopped.append(mode)
            assert r.returncode == 0, "mode %s: exit %d\n%s" % (mode, r.returncode, r.stdout[-4000:])
            _results[mode] = dict(np.load(f))
        return _results[mode]
    return _run


def _split(rows, p):
    return rows[:k.B, :p], rows[:k.B, p], rows[:k.B, p + 1:].reshape(k.B, p, p)


def _judge_modes(res, name, T, per_sample, given, worst, broken):
    """one case: every call of _modes, every sample, against the references of tile_edge_modes_common; what has to hold to the bit and does not goes to `broken`"""
    n, m, p = c.MODELS[name]
    B = k.B
    key = _key(name, T, per_sample, given)
    g = lambda kk: res[key + kk]
    where = "%s theta, %s" % ("per-sample" if per_sample else "shared", "given trajectory" if given else "rollout")

    def exact(ok, what):
        if not ok:
            broken.append("%s T=%d %s: %s" % (name, T, where, what))

    def diff(a, b):
        d = np.abs(np.asarray(a, dtype=float) - np.asarray(b, dtype=float))
        return "%d of %d entries, largest difference %.3e of the largest entry %.3e" % (int((d > 0).sum()), d.size, d.max(), np.abs(np.asarray(b, dtype=float)).max())

    def same(a, b, what):
        if not np.array_equal(a, b):
            broken.append("%s T=%d %s: %s: %s" % (name, T, where, what, diff(a, b)))
    calls = MASKED_CALLS + tuple(k.WEIGHTED) + ("vi", "gi")
    width = {"ms": p, "mp": p + 1, "vi": n, "gi": n}
    for tag in calls:
        rows = g(tag + "_rows")
        assert not g(tag + "_status").any(), (name, T, where, tag, g(tag + "_status"))
        assert rows.shape == (B + 1, width.get(tag, p + 1 + p * p)), (name, T, where, tag, rows.shape)
        assert np.isfinite(rows[:B]).all() and np.isnan(rows[B]).all(), (name, T, where, tag)                  # every entry written, nothing behind the last row
        same(g(tag + "_x"), g("x"), "x of %s vs the plain call" % tag)
        same(g(tag + "_lam"), g("lam"), "lam of %s vs the plain call" % tag)
    # masked
    grad_s, loss_s = g("ms_rows")[:B], g("ms_loss")
    grad_p, loss_p = g("mp_rows")[:B, :p], g("mp_rows")[:B, p]
    grad_g, loss_g, G_g = _split(g("mg_rows"), p)
    same(g("mp_loss"), loss_p, "loss [B] of the packed masked call vs its row")
    same(g("mg_loss"), loss_g, "loss [B] of the masked Gauss-Newton call vs its row")
    same(grad_p, grad_s, "masked gradient, packed vs alone")
    same(grad_g, grad_s, "masked gradient, Gauss-Newton row vs alone")
    same(loss_p, loss_s, "masked loss, packed vs alone")
    same(loss_g, loss_s, "masked loss, Gauss-Newton row vs alone")
    assert np.array_equal(G_g, np.swapaxes(G_g, 1, 2)), (name, T, where, "masked G")
    for what, a in (("gradient alone", grad_s[k.DARK]), ("loss alone", loss_s[k.DARK]), ("packed row", g("mp_rows")[k.DARK]), ("Gauss-Newton row", g("mg_rows")[k.DARK])):
        exact(not np.any(a), "dark sample, masked %s is not all zeros" % what)
    same(grad_s[k.FULL], g("grad")[k.FULL], "fully observed sample under skip_missing vs the call without the flag: gradient")
    same(loss_s[k.FULL], g("loss")[k.FULL], "fully observed sample under skip_missing vs the call without the flag: loss")
    same(g("mp_rows")[k.FULL], np.concatenate([g("grad")[k.FULL], g("loss")[k.FULL:k.FULL + 1]]), "fully observed sample under skip_missing, packed, vs the call without the flag")
    same(g("mg_rows")[k.FULL], g("rows")[k.FULL], "fully observed sample under skip_missing, Gauss-Newton row, vs the call without the flag")
    # weighted
    W = {tag: _split(g(tag + "_rows"), p) for tag in k.WEIGHTED}
    for tag, (gw, lw, Gw) in W.items():
        assert np.array_equal(Gw, np.swapaxes(Gw, 1, 2)), (name, T, where, tag, "G")
        same(g(tag + "_loss"), lw, "loss [B] of the weighted call %s vs its row" % tag)
        if tag in k.DARK_IN:
            exact(not g(tag + "_rows")[k.DARK].any(), "dark sample, weighted call %s is not all zeros" % tag)
    # initial state
    same(g("vi_grad"), g("cot"), "grad of the cotangent unit with want_ini vs without")
    same(g("gi_grad"), g("grad"), "grad of the default unit with want_ini vs without")
    same(g("gi_loss"), g("loss"), "loss of the default unit with want_ini vs without")
    # every sample against the oracle
    for b in range(B):
        at = "%s, sample %d" % (where, b)
        loss, grad, G = k.masked_reference(name, T, per_sample, b)
        if b == k.DARK:
            assert loss == 0.0 and not grad.any() and not G.any()
        else:
            for what, a in (("alone", grad_s), ("packed", grad_p), ("Gauss-Newton", grad_g)):
                worst.add("masked gradient (%s) vs the oracle's masked contraction" % what, c.rel(a[b], grad), at)
            for what, a in (("alone", loss_s), ("packed", loss_p), ("Gauss-Newton", loss_g)):
                worst.add("masked loss (%s) vs the oracle's masked sum (relative)" % what, abs(a[b] - loss) / loss, at)
            worst.add("masked G vs X'X + U'U of the oracle's observed rows", c.rel(G_g[b], G), at)
        for tag, (gw, lw, Gw) in W.items():
            loss, grad, G = k.weighted_reference(name, T, per_sample, b, tag)
            if b == k.DARK and tag in k.DARK_IN:
                assert loss == 0.0 and not grad.any() and not G.any()
                continue
            worst.add("weighted gradient (%s) vs the oracle's scaled contraction" % tag, c.rel(gw[b], grad), at)
            worst.add("weighted loss (%s) vs the oracle's sum of rho (relative)" % tag, abs(lw[b] - loss) / loss, at)
            worst.add("weighted G (%s) vs the oracle's scaled rows" % tag, c.rel(Gw[b], G), at)
        ref_v, ref_g = k.x0_reference(name, T, per_sample, b)
        worst.add("grad_x0 of the cotangent unit vs the reference's padded forward solve", c.rel(g("vi_rows")[b], ref_v), at)
        worst.add("grad_x0 of the default unit vs the reference's padded forward solve", c.rel(g("gi_rows")[b], ref_g), at)


def _loss_bounds(worst):
    return {q: k.LOSS_TOL for q in worst.v if "loss" in q}


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("mode", MODES)
def test_modes_follow_the_oracle(run, margins, mode, name):
    res = run(mode)
    broken = []
    for T in k.horizons(c.generated_info(name)):
        worst = te._Worst()
        for per_sample in (False, True):
            for given in (False, True):
                _judge_modes(res, name, T, per_sample, given, worst, broken)
        worst.check(margins, "modes %s %s T=%d" % (mode, name, T), _loss_bounds(worst))
    assert not broken, "%d claims of bit-equality do not hold:\n%s" % (len(broken), "\n".join(broken[:60]))


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("mode", MODES)
def test_old_calls_follow_the_oracle_across_the_forward_chunks(run, margins, mode, name):
    """tests/test_gpu_tile_edge.py's calls and its judgement (_judge_unit) at the horizons of this file: ROWSF - 1, ROWSF, ROWSF + 1 and beyond"""
    res = run(mode)
    for T in k.horizons(c.generated_info(name)):
        worst = te._Worst()
        for per_sample in (False, True):
            for given in (False, True):
                te._judge_unit(res, name, T, per_sample, given, worst)
        worst.check(margins, "modes, old calls, %s %s T=%d" % (mode, name, T), {"loss vs irl_loss_grad (relative)": k.LOSS_TOL})


@pytest.mark.parametrize("name", NAMES)
def test_trajectories_per_workgroup_layouts_agree_to_the_bit(run, name):
    """one wave pair per trajectory whatever the workgroup (test_gpu_tile_edge.py's test of the same name, on the calls of this file): every output of every case at two
    and four trajectories per workgroup equals the batch rule's one per workgroup, the NaN guard rows included.  Every output that differs is listed with its size."""
    a = run("default")
    differing = []
    for mode in ("tpw2", "tpw4"):
        b = run(mode)
        keys = [kk for kk in a if kk.startswith(name + "_") and kk.split("_")[1].isdigit()]
        assert len(keys) == KEYS_PER_CASE * len(te._cases(c.generated_info(name), k.horizons(c.generated_info(name)))), len(keys)
        for kk in keys:
            cut = -1 if kk.endswith("_ric") else None                    # (the record's last word per stage is scratch)
            x, y = a[kk][..., :cut], b[kk][..., :cut]
            if not np.array_equal(x, y, equal_nan=True):
                d = np.abs(x - y)
                differing.append("%s %s: %d of %d entries, largest difference %.3e of the largest entry %.3e" % (mode, kk, int((d > 0).sum()), d.size, np.nanmax(d), np.nanmax(np.abs(x))))
    assert not differing, "%d outputs differ:\n%s" % (len(differing), "\n".join(differing[:60]))


def test_wall_time_of_the_children(run, margins):
    """each child ended within its time limit; the figures go to the margins file"""
    for mode in MODES:
        run(mode)
    for mode in MODES:
        margins.check("tile edge modes, child %s: wall time in seconds (bound: its time limit)" % mode, _wall[mode], CHILD_TIMEOUT)
