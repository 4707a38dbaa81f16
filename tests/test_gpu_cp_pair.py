"""cp_step_poly2_kernel and sysid_step2_kernel (rollout wave + sensitivity wave per trajectory, csrc/pdp_cp_pair_kernels.h) against cp_step_poly_kernel /
sysid_step_kernel (one wavefront per trajectory):
the same arithmetic in the same order - loss, trajectory and gradient must agree BIT FOR BIT - over the workgroup shapes (1 / 2 / 4 trajectories per workgroup by
batch size), one to four parameter tiles, horizons of one chunk and of several, per-sample parameters, and a batch that is not a multiple of the workgroup.  The
one-wave kernel is pinned on the reference's own ControlPlanning.step runs (ref_cp_*_poly.npz, tests/test_gpu_models.py) and on the oracle at C3 / C4 sizes
(tests/test_gpu_configs.py - which run the pair kernel by default); this file transfers the pin between the two.

SysID.step transfers it in EVERY mode of the two kernels (MODES below: plain, Gauss-Newton, skip-missing, estimated initial states, weighted / Huber), through
ModelLib.sysid_step, at the chunk edges T = 1, 32, 33 and at one and two trajectories per workgroup (B = 3, 259), shared and per-sample parameters.  Seen on the
commit before the two kernels were moved into csrc/pdp_sysid_step_kernels.h, where they were two separate texts: 292 arrays compared, 0 differ - every mode bit for
bit, so every mode is asserted bit for bit; the same on the commit that moved them."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (system, pivots, horizon, batch): p = pivots x m -> 1 .. 4 tiles of 16 parameters; batches around the 256 / 512 CU thresholds of the workgroup shape
CASES = [("quadrotor", 6, 50, 1024), ("quadrotor", 6, 50, 1027), ("quadrotor", 3, 20, 5), ("quadrotor", 10, 37, 300), ("quadrotor", 16, 64, 131), ("rocket", 6, 100, 512),
         ("rocket", 6, 100, 700), ("cartpole", 5, 70, 9), ("pendulum", 12, 33, 260), ("robotarm", 7, 35, 64), ("quadrotor", 4, 1, 3), ("quadrotor", 4, 2, 3)]


# SysID.step: (system, horizon, batch)
SYSID_CASES = [("quadrotor", 100, 1024), ("quadrotor", 40, 1025), ("rocket", 70, 300), ("cartpole", 33, 7), ("pendulum", 1, 3), ("robotarm", 2, 70), ("quadrotor", 100, 513)]


# SysID.step in every mode of the two kernels (csrc/pdp_sysid_step_kernels.h), through ModelLib.sysid_step: mode -> keywords.  "ini" / "w" stand for the case's own
# ini_state / weights; estimate_ini: MODE_INI[system].  gauss_newton beside estimate_ini selects the packed row as the result (the same launch): G is compared too
MODES = [("plain", {}), ("gn", dict(gauss_newton=True)), ("gn_miss", dict(gauss_newton=True, skip_missing=True, ini_state="ini")),
         ("ini", dict(estimate_ini=True, gauss_newton=True)), ("ini_miss", dict(estimate_ini=True, gauss_newton=True, skip_missing=True, ini_state="ini")),
         ("wls", dict(weights="w", huber_delta=0.5)), ("wls_ini", dict(weights="w", huber_delta=0.5, estimate_ini=True))]
MODE_INI = dict(pendulum=[1], quadrotor=[3, 4, 5, 10, 11, 12])
# CHUNK = 32: no chunk loop to speak of, exactly one chunk, two chunks of 17 and 16; one trajectory per workgroup, and two with an odd tail slot
MODE_SHAPES = [(system, T, B) for system in ("pendulum", "quadrotor") for T in (1, 32, 33) for B in (3, 259)]


def _run_modes(zoo, out):
    for si, (system, T, B) in enumerate(MODE_SHAPES):
        mdl = zoo.get(system, "sysid")
        rng = np.random.default_rng(900 + si)
        u = 0.3 * rng.standard_normal((B, T, mdl.m))
        xobs = 0.3 * rng.standard_normal((B, T + 1, mdl.n))
        if system == "quadrotor":
            xobs[:, :, 6] += 1.0
        ini = xobs[:, 0] * (1.0 + 0.05 * rng.standard_normal((B, mdl.n)))
        xmiss = np.where(rng.random(xobs.shape) < 0.15, np.nan, xobs)        # row 0 included: the rollouts start from ini_state
        w = rng.uniform(0.2, 3.0, xobs.shape)
        w[rng.random(xobs.shape) < 0.1] = 0.0
        th = 1.0 + 0.2 * rng.uniform(-1, 1, mdl.p)
        thb = th[None] * (1 + 0.05 * rng.standard_normal((B, mdl.p)))       # per-sample parameters
        for mode, kw in MODES:
            kw = {k: (ini if v == "ini" else w if v == "w" else MODE_INI[system] if k == "estimate_ini" else v) for k, v in kw.items()}
            for tag, theta in (("shared", th), ("per_sample", thb)):
                r = mdl.sysid_step(u, xmiss if kw.get("skip_missing") else xobs, theta, **kw)
                r = dict(packed=r["packed_gn"]) if isinstance(r, dict) else dict(loss=r[0], grad=r[1])
                for k, v in r.items():
                    out["mode_%s_%s_T%d_B%d_%s_%s" % (mode, system, T, B, tag, k)] = v.cpu().numpy()


def _run_all():
    sys.path.insert(0, ROOT)
    from pdp_amd import runtime as rt, zoo
    out = {}
    _run_modes(zoo, out)
    for ci, (system, T, B) in enumerate(SYSID_CASES):
        mdl = zoo.get(system, "sysid")
        rng = np.random.default_rng(500 + ci)
        u = 0.3 * rng.standard_normal((B, T, mdl.m))
        xobs = 0.3 * rng.standard_normal((B, T + 1, mdl.n))
        if system in ("quadrotor", "rocket"):
            xobs[:, :, 6] += 1.0
        th = 1.0 + 0.2 * rng.uniform(-1, 1, mdl.p)
        loss, grad = mdl.sysid_step(u, xobs, th)
        lossb, gradb = mdl.sysid_step(u, xobs, th[None] * (1 + 0.05 * rng.standard_normal((B, mdl.p))))
        for k, v in (("loss", loss), ("grad", grad), ("loss_b", lossb), ("grad_b", gradb)):
            out["sysid%d_%s" % (ci, k)] = v.cpu().numpy()
    for ci, (system, npiv, T, B) in enumerate(CASES):
        mdl = zoo.get(system, "oc")
        rng = np.random.default_rng(300 + ci)
        p = npiv * mdl.m
        x0 = 0.3 * rng.standard_normal((B, mdl.n))
        if system in ("quadrotor", "rocket"):
            x0[:, 6] = 1.0
        th = 0.3 * rng.standard_normal(p)
        pol = rt.make_policy("poly", pivots=np.linspace(0, T, npiv))
        loss, grad, x, u = mdl.cp_step(pol, p, x0, th, T, want_traj=True)
        thb = th[None] * (1 + 0.05 * rng.standard_normal((B, p)))            # per-sample parameters
        loss2, grad2 = mdl.cp_step(pol, p, x0, thb, T)
        for k, v in (("loss", loss), ("grad", grad), ("x", x), ("u", u), ("loss_b", loss2), ("grad_b", grad2)):
            out["%d_%s" % (ci, k)] = v.cpu().numpy()
    return out


def test_pair_kernel_equals_one_wave_kernel(tmp_path):
    """both sides in subprocesses: the kernel choice is read from the environment once per process (PDP_CP_POLY_VARIANT=3: the pair for every batch size)"""
    res = {}
    for tag, env in (("pair", dict(PDP_CP_POLY_VARIANT="3", PDP_SYSID_VARIANT="2")), ("onewave", dict(PDP_CP_POLY_VARIANT="1", PDP_SYSID_VARIANT="1"))):
        f = str(tmp_path / (tag + ".npz"))
        code = ("import sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_cp_pair as m; np.savez(%r, **m._run_all())"
                % (ROOT, os.path.join(ROOT, "tests"), f))
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-3000:]
        res[tag] = np.load(f)
    new, ref = res["pair"], res["onewave"]
    worst = {}
    for k in sorted(new.files):
        a, b = new[k], ref[k]
        assert np.isfinite(a).all(), k
        if not np.array_equal(a, b):
            worst[k] = float(np.abs(a - b).max() / max(1e-300, np.abs(b).max()))
    print("%d arrays compared, %d differ: %s" % (len(new.files), len(worst), json.dumps(worst)))
    assert not worst, "pair kernels differ from the one-wave kernels: %s" % json.dumps(worst)
