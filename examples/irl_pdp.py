#!/usr/bin/env python3
"""Inverse reinforcement learning with PDP on the GPU - the loop of the reference's Examples/IRL/<sys>/<sys>_PDP.py
(e.g. cartpole_PDP.py:32-94) with the per-demo Python loop replaced by ONE batched launch per stage:

    for k in iterations:   traj  = ocSolver(theta_k)                     (IPOPT's iteration in one GPU launch, started from the first-order PREDICTION
                                                                          traj_{k-1} + d traj / d theta (theta_k - theta_{k-1}) the previous gradient step provides)
                           loss, dp = aux system + Riccati + chain rule  (fused kernel; keeps d traj / d theta for the next prediction)
                           theta_{k+1} = theta_k - lr * mean(dp)

Demonstrations: the reference's stored demos (examples/data/demos_<sys>.npz, copies of the extracts under tests/golden), or any `<name>_demos.mat` written by the reference's
generate_demos.py (field names trajectories[i].state_traj_opt / control_traj_opt, true_parameter, dt; e.g.
Examples/IRL/cartpole/generate_demos.py:38-43) through --demos.  Results are saved with the reference's field names
(results.loss_trace / parameter_trace / learning_rate / time_passed) so its plotting scripts keep working.

    python examples/irl_pdp.py --system cartpole --iters 200 --lr 1e-4 [--demos path/to/cartpole_demos.mat]

--method lm: the same problem as nonlinear least squares (the loss is a sum of squares).  The fused kernel also returns the Gauss-Newton matrix J'J beside the gradient
(PDP_GRAD_GAUSS_NEWTON), and a Levenberg-Marquardt loop (pdp_amd.irl.LMLoop; --iters bounds its evaluations) takes a handful of steps where gradient descent takes thousands:

    python examples/irl_pdp.py --system cartpole --method lm

Demonstrations with gaps (--method lm): --every K keeps the states at t = K, 2K, ... <= T, --observe i,j,... the listed state components, --no-controls no control; every
other entry becomes NaN = not observed (PDP_GRAD_SKIP_MISSING), and the solves start from the demonstrations' own first states:

    python examples/irl_pdp.py --system cartpole --method lm --every 10 --observe 0,1 --no-controls

Noisy and corrupted demonstrations (--method lm): weighted and Huber-robust least squares (the weights_state= / weights_control= / huber_delta= keywords of the loops,
pdp_oc_pdp_grad_wls_batched).  --noise-sigma s0,s1,... (one value per state component, then one per control component) adds Gaussian noise of that standard deviation
to the demonstrations (states at t >= 1, every control) and weights every entry of a component by 1 / s_i^2; --outliers moves that fraction of the entries (states at
t >= 1, every control) by +-(0.5 .. 1.5); --huber is Huber's threshold on the standardised residual sqrt(w) d, which keeps such entries from steering the fit:

    python examples/irl_pdp.py --system cartpole --method lm --huber 0.01 --outliers 0.05

A prior and error bars (--method lm): --prior-sigma S puts a Gaussian prior of standard deviation S around the starting parameter (the prior_mean= / prior_precision=
keywords of the loops), --covariance prints theta +- std_err and the pivot ratio of the covariance solve (loop.covariance()).  Keyframes without controls leave the scale
of the cost weights unidentified: the pivot ratio shows it, the prior makes the problem well posed:

    python examples/irl_pdp.py --system cartpole --method lm --every 10 --observe 0,1 --no-controls --prior-sigma 0.5 --covariance
"""
import argparse
import os
import sys
import time

import numpy as np
import scipy.io as sio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pdp_amd import PDP, ocsolver, zoo          # noqa: E402
from pdp_amd.sx import vertcat                  # noqa: E402


def load_demos(path):
    """(state [B,T+1,n], control [B,T,m], true_parameter [p]) from the npz fixtures or from a .mat in the reference's schema"""
    if path.endswith(".npz"):
        d = np.load(path)
        return d["state"], d["control"], d["true_parameter"]
    d = sio.loadmat(path)
    tr = d["trajectories"]
    xs = np.stack([np.asarray(tr[0, i]["state_traj_opt"][0, 0], dtype=float) for i in range(tr.shape[1])])
    us = np.stack([np.asarray(tr[0, i]["control_traj_opt"][0, 0], dtype=float) for i in range(tr.shape[1])])
    return xs, us, d["true_parameter"].astype(float).flatten()


def reference_last_loss(system):
    """(steps, mean loss) where the reference's own stored gradient-descent run on the stored demonstrations ends (tests/golden/irltrace_<sys>.npz; that run starts from the
    reference's initial parameter, row 0 of irltrace_head_<sys>.npz["param"], which --init replays), or None where the trace is not at hand"""
    path = os.path.join(ROOT, "tests", "golden", "irltrace_%s.npz" % system)
    if not os.path.exists(path):
        return None
    z = np.load(path)
    return int(z["K"]), float(z["loss_next"][-1])


def mask_demos(demo_x, demo_u, every=None, observe=None, no_controls=False):
    """the demonstrations with every entry that is not observed set to NaN: states at t = every, 2 every, ... <= T (None: every step), components `observe` (None: all),
    controls all or none"""
    T, n = demo_u.shape[1], demo_x.shape[2]
    steps = np.arange(T + 1) if every is None else np.arange(every, T + 1, every)
    comps = np.arange(n) if observe is None else np.asarray(observe, dtype=int)
    mx = np.full(demo_x.shape, np.nan)
    mx[:, steps[:, None], comps[None, :]] = demo_x[:, steps[:, None], comps[None, :]]
    return mx, (np.full(demo_u.shape, np.nan) if no_controls else demo_u.copy())


def disturb_demos(demo_x, demo_u, noise_sigma=None, outliers=0.0, seed=0):
    """(demo_x, demo_u, weights_state or None, weights_control or None, number of outliers): Gaussian noise of standard deviation noise_sigma[i] on component i (n state
    components, then m control components) with the weights 1 / s_i^2, and `outliers` of the entries moved by +-(0.5 .. 1.5).  Row 0 of the states stays as recorded:
    the solves start there."""
    n, m = demo_x.shape[2], demo_u.shape[2]
    rng = np.random.default_rng(seed)
    demo_x, demo_u, wx, wu, k = demo_x.copy(), demo_u.copy(), None, None, 0
    if noise_sigma is not None:
        sig = np.asarray(noise_sigma, dtype=float)
        assert sig.shape == (n + m,) and (sig > 0).all(), "--noise-sigma: %d positive values, one per state component, then one per control component" % (n + m)
        demo_x[:, 1:] += sig[:n] * rng.standard_normal(demo_x[:, 1:].shape)
        demo_u += sig[n:] * rng.standard_normal(demo_u.shape)
        wx, wu = 1.0 / sig[:n] ** 2, 1.0 / sig[n:] ** 2
    if outliers > 0:
        for a_, first in ((demo_x, 1), (demo_u, 0)):
            hit = rng.random(a_.shape) < outliers
            hit[:, :first] = False
            a_[hit] += (rng.choice([-1.0, 1.0], a_.shape) * rng.uniform(0.5, 1.5, a_.shape))[hit]
            k += int(hit.sum())
    return demo_x, demo_u, wx, wu, k


def run_lm(a, oc, demo_x, demo_u, theta, true_parameter):
    from pdp_amd.irl import LMLoop
    t0 = time.time()
    wls = {}
    if a.noise_sigma is not None or a.outliers > 0:
        sig = None if a.noise_sigma is None else [float(v) for v in a.noise_sigma.split(",")]
        demo_x, demo_u, wx, wu, k = disturb_demos(demo_x, demo_u, sig, a.outliers, a.seed)
        if wx is not None:
            wls.update(weights_state=wx, weights_control=wu)
        if a.outliers > 0:
            print("%d of %d demonstration entries are outliers" % (k, demo_x.size + demo_u.size))
    if a.huber is not None:
        wls["huber_delta"] = a.huber
    if a.prior_sigma is not None:
        assert a.prior_sigma > 0, "--prior-sigma: a positive number"
        wls.update(prior_mean=np.array(theta, dtype=float), prior_precision=np.full(np.size(theta), 1.0 / a.prior_sigma ** 2))
    sparse = a.every is not None or a.observe is not None or a.no_controls
    if sparse:
        assert a.every is None or a.every >= 1, "--every: a positive number of steps"
        observe = None if a.observe is None else [int(v) for v in a.observe.split(",")]
        assert observe is None or all(0 <= i < demo_x.shape[2] for i in observe), "--observe: state components 0 .. %d" % (demo_x.shape[2] - 1)
        ini_state = demo_x[:, 0].copy()
        demo_x, demo_u = mask_demos(demo_x, demo_u, a.every, observe, a.no_controls)
        print("observed: %d of %d state entries, %d of %d control entries per demonstration" % (
            int((~np.isnan(demo_x[0])).sum()), demo_x[0].size, int((~np.isnan(demo_u[0])).sum()), demo_u[0].size))
        loop = LMLoop.for_irl(oc.model(), demo_x, demo_u, theta, ini_state=ini_state, skip_missing=True, **wls)
    else:
        loop = LMLoop.for_irl(oc.model(), demo_x, demo_u, theta, **wls)
    r = loop.run(max_evals=a.iters, loss_tol=a.loss_tol)
    for k, (loss, th, lam) in enumerate(zip(r["loss_trace"], r["parameter_trace"], r["lambda_trace"])):
        print("accepted %3d  loss %.6e  |theta - theta*| %.4e  next damping %.1e" % (k, loss, np.abs(th - true_parameter).max(), lam))
    if a.covariance:
        noise = "known" if (a.noise_sigma is not None or a.prior_sigma is not None) else "estimated"
        c = loop.covariance(noise)
        print("theta %s  (noise %s, sigma^2 %.3e)  pivot_ratio %.2e%s" % ("  ".join("%.5f +- %.1e" % (v, e) for v, e in zip(r["parameter_trace"][-1], c["std_err"])), noise,
                                                                           c["sigma2"], c["pivot_ratio"], "" if c["status"] == 0 else "  (singular)"))
    save = {"trail_no": 0, "loss_trace": r["loss_trace"], "parameter_trace": r["parameter_trace"], "learning_rate": 0.0, "time_passed": time.time() - t0}
    if a.out:
        sio.savemat(a.out, {"results": save})
    ref = reference_last_loss(a.system) if a.demos is None else None
    print("done: %d evaluations (%d rejected%s) x %d demos in %.2f s, final loss %.4e%s" % (
        r["evaluations"], r["rejected"], ", stalled at the damping limit" if r["stalled"] else "", demo_x.shape[0], save["time_passed"], r["loss_trace"][-1],
        "  (for comparison, another start: the reference's stored gradient-descent run on these demos, from its own initial parameter, ends at %.4e after %d steps)"
        % (ref[1], ref[0]) if ref else ""))
    return list(r["loss_trace"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--system", default="cartpole", choices=["pendulum", "cartpole", "robotarm", "quadrotor", "rocket"])
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--sigma", type=float, default=0.3, help="initial parameter = true + U(-sigma/2, sigma/2)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--init", default=None, help="initial parameter: comma-separated values or a .npy file (default: true + U(-sigma/2, sigma/2)); e.g. row 0 of a stored "
                                                 "parameter_trace to replay the reference's run")
    ap.add_argument("--out", default=None)
    ap.add_argument("--record", default="full", choices=["full", "primal"],
                    help="what the gradient unit keeps for the next solve's predicted start: states, controls and multipliers (full) or states and controls only "
                         "(primal: cheaper to write and read; enough where the multipliers move little per step, e.g. the quadrotor)")
    ap.add_argument("--graph", action="store_true",
                    help="keep the loop on the device and replay each iteration as one hipGraph (pdp_amd.irl.IRLLoop): no host work per iteration, traces written by the graph")
    ap.add_argument("--method", default="gd", choices=["gd", "lm"],
                    help="gd: the reference's gradient descent (default); lm: Levenberg-Marquardt on the Gauss-Newton matrix the fused kernel returns "
                         "(--iters = most evaluations, --lr unused)")
    ap.add_argument("--loss-tol", type=float, default=1e-16, help="--method lm: stop at this mean loss")
    ap.add_argument("--every", type=int, default=None, help="--method lm: only the states at t = K, 2K, ... <= T are observed (default: every step)")
    ap.add_argument("--observe", default=None, help="--method lm: comma-separated state components that are observed (default: all)")
    ap.add_argument("--no-controls", action="store_true", help="--method lm: no control is observed")
    ap.add_argument("--noise-sigma", default=None, help="--method lm: noise levels s0,s1,... added to the demonstrations, one per state component, then one per control "
                                                        "component; the weights are 1 / s_i^2")
    ap.add_argument("--huber", type=float, default=None, help="--method lm: Huber's threshold on the standardised residual")
    ap.add_argument("--outliers", type=float, default=0.0, help="--method lm: this fraction of the demonstration entries is moved by +-(0.5 .. 1.5)")
    ap.add_argument("--prior-sigma", type=float, default=None, help="--method lm: a Gaussian prior of this standard deviation around the starting parameter")
    ap.add_argument("--covariance", action="store_true", help="--method lm: print theta +- std_err and the pivot ratio of the covariance solve")
    ap.add_argument("--demos", default=None, help="<name>_demos.mat in the reference's schema (default: the stored demos of --system)")
    a = ap.parse_args()
    if (a.noise_sigma is not None or a.huber is not None or a.outliers > 0) and a.method != "lm":
        ap.error("--noise-sigma / --huber / --outliers need --method lm")
    if (a.prior_sigma is not None or a.covariance) and a.method != "lm":
        ap.error("--prior-sigma / --covariance need --method lm")

    env, dt = zoo.make_env(a.system, "irl")
    oc = PDP.OCSys(a.system)
    oc.setAuxvarVariable(vertcat(env.dyn_auxvar, env.cost_auxvar))
    oc.setControlVariable(env.U)
    oc.setStateVariable(env.X)
    oc.setDyn(env.X + dt * env.f)
    oc.setPathCost(env.path_cost)
    oc.setFinalCost(env.final_cost)
    oc.diffPMP()

    demo_x, demo_u, true_parameter = load_demos(a.demos or os.path.join(ROOT, "examples", "data", "demos_%s.npz" % a.system))
    T = demo_u.shape[1]
    rng = np.random.default_rng(a.seed)
    theta = true_parameter + a.sigma * rng.random(true_parameter.size) - a.sigma / 2
    if a.init is not None:
        theta = np.load(a.init).astype(float).reshape(-1) if a.init.endswith(".npy") else np.array([float(v) for v in a.init.split(",")])
        assert theta.size == true_parameter.size, "--init: %d values for %d parameters" % (theta.size, true_parameter.size)
    assert a.method == "lm" or (a.every is None and a.observe is None and not a.no_controls), "--every / --observe / --no-controls go with --method lm"
    if a.method == "lm":
        return run_lm(a, oc, demo_x, demo_u, theta, true_parameter)
    loss_trace, parameter_trace = [], []
    warm, predict, theta_prev = None, None, None
    fused = oc.model().n <= 16 and oc.model().m <= 4 and oc.model().m + oc.model().p <= 16      # the kernels that keep the sensitivities
    t0 = time.time()
    if a.graph:
        assert fused, "--graph needs the fused kernels (n <= 16, m <= 4, m + p <= 16)"
        from pdp_amd.irl import IRLLoop
        loop = IRLLoop(oc.model(), demo_x, demo_u, theta, a.lr, record=a.record, max_steps=a.iters + 8)
        loop.run(a.iters)
        r = loop.results()
        loss_trace, parameter_trace = list(r["loss_trace"][:a.iters]), list(r["parameter_trace"][:a.iters])
        if r["unconverged_solves"] or r["riccati_trouble"]:
            print("warning: %d OC solves did not converge, %d trajectories with numerical trouble in the Riccati sweep" % (r["unconverged_solves"], r["riccati_trouble"]))
        for k in range(0, a.iters, max(1, a.iters // 10)):
            print("iter %5d  loss %.6e  |theta - theta*| %.4f" % (k, loss_trace[k], np.abs(parameter_trace[k] - true_parameter).max()))
        save = {"trail_no": 0, "loss_trace": loss_trace, "parameter_trace": parameter_trace, "learning_rate": a.lr, "time_passed": time.time() - t0}
        if a.out:
            sio.savemat(a.out, {"results": save})
        print("done: %d iterations x %d demos in %.2f s, one hipGraph per iteration  (loss %.4e -> %.4e)" % (a.iters, demo_x.shape[0], save["time_passed"], loss_trace[0], loss_trace[-1]))
        return loss_trace
    for k in range(a.iters):
        # first iterate: cold, the reference's all-zero guess (PDP.py:155,166).  Afterwards the multiple-shooting solver starts from the previous solution moved
        # along its own sensitivities, (x, u, lambda)_{k-1} + (X, U, Lambda)_{k-1} (theta_k - theta_{k-1}) - the auxiliary control system the gradient step has just
        # solved IS that derivative (PDP.py:582-608) - and needs about one Newton iteration (two from the unmoved previous solution)
        if predict is not None:
            predict["dtheta"] = theta - theta_prev
        sol = ocsolver.solve_batch(oc, demo_x[:, 0], T, theta, warm_start=warm, predict=predict)
        if not bool(sol["converged"].all()):
            print("iter %5d  warning: %d of %d OC solves did not converge" % (k, int((~sol["converged"]).sum()), demo_x.shape[0]))
        warm = {key: sol[key] for key in ("state", "control", "costate")}
        out = oc.pdp_grad_batch(sol["control"], theta, demo_x, demo_u, state_traj=sol["state"], costate_traj=sol["costate"], want_predict_record=(("primal" if a.record == "primal" else True) if fused else False))
        if fused:
            predict, theta_prev = {"record": out["predict_record"], "primal": a.record == "primal"}, theta.copy()
        if int(out["status"].sum()) != 0:
            print("iter %5d  warning: Riccati sweep reported numerical trouble on %d trajectories" % (k, int((out["status"] != 0).sum())))
        loss = float(out["loss"].mean())
        dp = out["grad"].mean(dim=0).cpu().numpy()
        theta = theta - a.lr * dp
        loss_trace.append(loss)
        parameter_trace.append(theta.copy())
        if k % max(1, a.iters // 10) == 0:
            print("iter %5d  loss %.6e  |theta - theta*| %.4f" % (k, loss, np.abs(theta - true_parameter).max()))
    save = {"trail_no": 0, "loss_trace": loss_trace, "parameter_trace": parameter_trace, "learning_rate": a.lr, "time_passed": time.time() - t0}
    if a.out:
        sio.savemat(a.out, {"results": save})
    print("done: %d iterations x %d demos in %.2f s  (loss %.4e -> %.4e)" % (a.iters, demo_x.shape[0], save["time_passed"], loss_trace[0], loss_trace[-1]))
    return loss_trace


if __name__ == "__main__":
    main()
