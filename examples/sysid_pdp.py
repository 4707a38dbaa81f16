#!/usr/bin/env python3
"""System identification with PDP on the GPU - the loop of the reference's Examples/SysID/<sys>/*_PDP.py (quadrotor/uav_PDP.py:33-59)
on the reference's stored input/state data (tests/golden/iodata_<sys>.npz), or any `<stem>_iodata.mat` written by the reference's
generate_traj.py (struct <stem>_iodata with batch_inputs / batch_states / true_parameter, e.g.
Examples/SysID/quadrotor/generate_traj.py:36-42) through --data.

    python examples/sysid_pdp.py --system quadrotor --iters 2000 --lr 1e-4 [--data path/to/uav_iodata.mat]

--method lm: the same problem as nonlinear least squares (pdp_amd.irl.LMLoop.for_sysid: Levenberg-Marquardt on the Gauss-Newton matrix the fused kernel returns with the
gradient, one launch per evaluation) - a handful of evaluations instead of thousands of descent steps.  With it, partial data: --every K keeps the samples at
t = K, 2K, ... only, --observe i,j,... only those state components; every other entry becomes NaN = not observed, and the rollouts start from the recorded initial states.

    python examples/sysid_pdp.py --system pendulum --method lm --every 2 --observe 0

--method lm --per-trajectory: one problem PER stored trajectory, each with its own parameter estimate, all advanced in lock-step on the device
(pdp_amd.irl.BatchedLMLoop.for_sysid: one launch of the fused kernel per evaluation of all problems, one launch that accepts or rejects, damps, solves and terminates per
problem); prints evaluations, state and final loss per problem.

    python examples/sysid_pdp.py --system pendulum --method lm --per-trajectory

--method lm --estimate-ini i,j,...: these components of every recording's initial state are NOT known (an encoder without velocities does not give the initial velocity
either) and are estimated together with the parameters, from 0: the sensitivity with respect to them is a further column of the tile the fused kernel holds anyway.
Shared parameters with one initial state per recording (LMLoop.for_sysid(estimate_ini=)), or with --per-trajectory one parameter estimate and one initial state per
trajectory (BatchedLMLoop.for_sysid(estimate_ini=)).

    python examples/sysid_pdp.py --system cartpole --method lm --observe 0,1 --estimate-ini 2,3

--method lm --noise-sigma s0,s1,... --huber DELTA --outliers FRACTION: weighted and Huber-robust least squares (the weights= / huber_delta= keywords of the two loops; one
launch per evaluation as before).  --noise-sigma adds Gaussian noise of standard deviation s_i to component i of the recorded states (t >= 1) and weights every entry of
that component by 1 / s_i^2; --outliers moves that fraction of the recorded entries (t >= 1) by +-(0.5 .. 1.5); --huber is Huber's threshold on the standardised residual
sqrt(w) (x - x_obs).  (--sigma is the spread of the starting parameter, as it always was.)

    python examples/sysid_pdp.py --system cartpole --method lm --noise-sigma 1e-3,1e-3,1e-2,1e-2 --huber 3 --outliers 0.05

--method lm --prior-sigma S --covariance: a Gaussian prior of standard deviation S around the starting parameter (the prior_mean= / prior_precision= keywords of the two
loops: a partially identifiable problem becomes well posed) and the error bars of the estimate (loop.covariance(): theta +- std_err and the pivot ratio of the solve, the
diagnosis of a parameter the data do not pin).  The noise level is taken as known where --noise-sigma gives the weights or a prior is set, else estimated from the loss:

    python examples/sysid_pdp.py --system pendulum --method lm --per-trajectory --prior-sigma 0.5 --covariance
"""
import argparse
import os
import sys
import time

import numpy as np
import scipy.io as sio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pdp_amd import PDP, zoo          # noqa: E402


def load_iodata(path):
    """(inputs [B,T,m], states [B,T+1,n], true_parameter [p]) from the npz fixtures or from a .mat in the reference's schema"""
    if path.endswith(".npz"):
        io = np.load(path)
        return io["inputs"], io["states"], io["true_parameter"]
    d = sio.loadmat(path)
    key = [k for k in d if k.endswith("_iodata")][0]
    x = d[key][0, 0]
    return np.asarray(x["batch_inputs"], float), np.asarray(x["batch_states"], float), np.asarray(x["true_parameter"], float).flatten()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--system", default="quadrotor", choices=["pendulum", "cartpole", "robotarm", "quadrotor", "rocket"])
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--sigma", type=float, default=0.6)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--graph", action="store_true", help="keep the loop on the device (pdp_amd.irl.GDLoop: two launches per iteration, replayed as a hipGraph); equal horizons only")
    ap.add_argument("--data", default=None, help="<stem>_iodata.mat in the reference's schema (default: the stored data of --system)")
    ap.add_argument("--method", default="gd", choices=["gd", "lm"], help="gd: the reference's gradient descent; lm: Levenberg-Marquardt (at most min(--iters, 100) evaluations)")
    ap.add_argument("--every", type=int, default=1, help="--method lm: only the samples at t = K, 2K, ... are observed")
    ap.add_argument("--observe", default=None, help="--method lm: only these state components are observed (comma-separated indices)")
    ap.add_argument("--per-trajectory", action="store_true", help="--method lm: one problem per trajectory, all in lock-step on the device (irl.BatchedLMLoop)")
    ap.add_argument("--estimate-ini", default=None, help="--method lm: these components of the initial states are unknown and estimated with the parameters (comma-separated)")
    ap.add_argument("--noise-sigma", default=None, help="--method lm: per-component noise levels s0,s1,... added to the recorded states; the weights are 1 / s_i^2")
    ap.add_argument("--huber", type=float, default=None, help="--method lm: Huber's threshold on the standardised residual")
    ap.add_argument("--outliers", type=float, default=0.0, help="--method lm: this fraction of the recorded entries is moved by +-(0.5 .. 1.5)")
    ap.add_argument("--prior-sigma", type=float, default=None, help="--method lm: a Gaussian prior of this standard deviation around the starting parameter")
    ap.add_argument("--covariance", action="store_true", help="--method lm: print theta +- std_err and the pivot ratio of the covariance solve")
    a = ap.parse_args()
    partial = a.every > 1 or a.observe is not None
    if (a.prior_sigma is not None or a.covariance) and a.method != "lm":
        ap.error("--prior-sigma / --covariance need --method lm")
    if a.prior_sigma is not None and not a.prior_sigma > 0:
        ap.error("--prior-sigma: a positive number")
    if a.estimate_ini is not None and a.method != "lm":
        ap.error("--estimate-ini needs --method lm")
    if partial and a.method != "lm":
        ap.error("--every / --observe need --method lm")
    if a.per_trajectory and a.method != "lm":
        ap.error("--per-trajectory needs --method lm")
    if (a.noise_sigma is not None or a.huber is not None or a.outliers > 0) and a.method != "lm":
        ap.error("--noise-sigma / --huber / --outliers need --method lm")
    env, dt = zoo.make_env(a.system, "sysid")
    sid = PDP.SysID(a.system)
    sid.setAuxvarVariable(env.dyn_auxvar)
    sid.setStateVariable(env.X)
    sid.setControlVariable(env.U)
    sid.setDyn(env.X + dt * env.f)
    inputs, states, true_parameter = load_iodata(a.data or os.path.join(ROOT, "tests", "golden", "iodata_%s.npz" % a.system))
    batch_inputs = [inputs[i] for i in range(inputs.shape[0])]
    batch_states = [states[i] for i in range(states.shape[0])]
    rng = np.random.default_rng(a.seed)
    theta = true_parameter + a.sigma * rng.random(true_parameter.size) - a.sigma / 2
    wls = {}
    if a.noise_sigma is not None or a.outliers > 0:         # (row 0 stays as recorded: the rollouts start there)
        states = states.copy()
        if a.noise_sigma is not None:
            sig = np.array([float(c) for c in a.noise_sigma.split(",")])
            if sig.shape != (states.shape[2],) or not (sig > 0).all():
                ap.error("--noise-sigma: %d positive values, one per state component" % states.shape[2])
            states[:, 1:] += sig * rng.standard_normal(states[:, 1:].shape)
            wls["weights"] = 1.0 / sig ** 2
        if a.outliers > 0:
            hit = rng.random(states.shape) < a.outliers
            hit[:, 0] = False
            k = int(hit.sum())
            states[hit] += rng.choice([-1.0, 1.0], k) * (0.5 + rng.random(k))
            print("%d of %d recorded entries are outliers" % (k, states.size))
    if a.huber is not None:
        wls["huber_delta"] = a.huber
    if a.prior_sigma is not None:
        wls["prior_mean"], wls["prior_precision"] = theta.copy(), np.full(theta.size, 1.0 / a.prior_sigma ** 2)
        if a.estimate_ini is not None:              # the same prior on the estimated components of the initial states, around their start (0)
            wls["prior_ini_precision"] = np.full(len(a.estimate_ini.split(",")), 1.0 / a.prior_sigma ** 2)
    noise = "known" if (a.noise_sigma is not None or a.prior_sigma is not None) else "estimated"
    loss_trace, parameter_trace = [], []
    t0 = time.time()
    if a.method == "lm":
        from pdp_amd.irl import BatchedLMLoop, LMLoop
        masked = None
        if partial:
            comps = [int(c) for c in a.observe.split(",")] if a.observe is not None else list(range(states.shape[2]))
            masked = np.full_like(states, np.nan)
            for t in range(a.every, states.shape[1], a.every):
                masked[:, t, comps] = states[:, t, comps]
        if a.estimate_ini is not None:
            idx = [int(c) for c in a.estimate_ini.split(",")]
            ini = states[:, 0].copy()
            ini[:, idx] = 0.0                       # not known: the estimate starts from 0
            data = masked if partial else states.copy()
            if not partial:
                data[:, 0, idx] = np.nan            # (what is estimated was not recorded)
            make = BatchedLMLoop.for_sysid if a.per_trajectory else LMLoop.for_sysid
            loop = make(sid.model(), inputs, data, theta, ini_state=ini, skip_missing=True, estimate_ini=idx, **wls, **(dict(max_evals=min(a.iters, 100), loss_tol=1e-20)
                                                                                                                     if a.per_trajectory else {}))
            r = loop.run() if a.per_trajectory else loop.run(max_evals=min(a.iters, 100), loss_tol=1e-20)
            if a.covariance:                        # over the whole vector of unknowns: theta, then the estimated components of the initial state(s)
                c = loop.covariance(noise)
                for k in (range(inputs.shape[0]) if a.per_trajectory else [None]):
                    v, e = (r["theta"][k], c["std_err"][k]) if a.per_trajectory else (r["parameter_trace"][-1], c["std_err"])
                    print("%s [theta | ini_state%s] %s  (noise %s)  pivot_ratio %.2e" % ("problem %3d " % k if a.per_trajectory else "", idx,
                          "  ".join("%.5f +- %.1e" % (vi, ei) for vi, ei in zip(v, e)), noise, c["pivot_ratio"][k] if a.per_trajectory else c["pivot_ratio"]))
            if a.per_trajectory:
                th, x0 = loop.split(r["theta"])
                for k in range(inputs.shape[0]):
                    print("trajectory %3d  %2d evaluations  %2d rejected  %-9s  loss %.6e -> %.6e  |theta - theta*| = %.2e  |ini_state - x0*| = %.2e  theta %s"
                          % (k, r["evaluations"][k], r["rejected"][k], r["state"][k], r["loss_trace"][k][0], r["loss"][k], np.abs(th[k] - true_parameter).max(),
                             np.abs(x0[k] - states[k, 0]).max(), np.array2string(th[k], precision=4)))
                print("done: %d problems in %d launches, %.2f s; largest final loss %.4e" % (inputs.shape[0], r["launches"], time.time() - t0, np.max(r["loss"])))
                return r
            for k in range(len(r["loss_trace"])):
                print("accepted %3d  loss %.6e  lambda %.1e  theta %s" % (k, r["loss_trace"][k], r["lambda_trace"][k],
                                                                          np.array2string(loop.split(r["parameter_trace"][k])[0], precision=4)))
            print("%d evaluations, %d rejected%s" % (r["evaluations"], r["rejected"], ", stalled" if r["stalled"] else ""))
            th, x0 = loop.split(r["parameter_trace"][-1])
            print("done: %d accepted points in %.2f s; loss %.4e -> %.4e; |theta - theta*| = %.2e; |ini_state - x0*| = %.2e"
                  % (len(r["loss_trace"]), time.time() - t0, r["loss_trace"][0], r["loss_trace"][-1], np.abs(th - true_parameter).max(), np.abs(x0 - states[:, 0]).max()))
            return r
        if a.per_trajectory:
            kw = dict(ini_state=states[:, 0], skip_missing=True) if partial else {}
            loop = BatchedLMLoop.for_sysid(sid.model(), inputs, masked if partial else states, theta, max_evals=min(a.iters, 100), loss_tol=1e-20, **kw, **wls)
            r = loop.run()
            for k in range(inputs.shape[0]):
                print("problem %3d  %2d evaluations  %2d rejected  %-9s  loss %.6e -> %.6e  |theta - theta*| = %.2e  theta %s"
                      % (k, r["evaluations"][k], r["rejected"][k], r["state"][k], r["loss_trace"][k][0], r["loss"][k], np.abs(r["theta"][k] - true_parameter).max(),
                         np.array2string(r["theta"][k], precision=4)))
            if a.covariance:
                c = loop.covariance(noise)
                for k in range(inputs.shape[0]):
                    print("problem %3d  theta %s  (noise %s, sigma^2 %.3e)  pivot_ratio %.2e%s"
                          % (k, "  ".join("%.5f +- %.1e" % (v, e) for v, e in zip(r["theta"][k], c["std_err"][k])), noise, c["sigma2"][k], c["pivot_ratio"][k],
                             "" if c["status"][k] == 0 else "  (singular)"))
            print("done: %d problems in %d launches, %.2f s; largest final loss %.4e" % (inputs.shape[0], r["launches"], time.time() - t0, np.max(r["loss"])))
            return r
        if partial:
            loop = LMLoop.for_sysid(sid.model(), inputs, masked, theta, ini_state=states[:, 0], skip_missing=True, **wls)
        else:
            loop = LMLoop.for_sysid(sid.model(), inputs, states, theta, **wls)
        r = loop.run(max_evals=min(a.iters, 100), loss_tol=1e-20)
        loss_trace, parameter_trace = list(r["loss_trace"]), list(r["parameter_trace"])
        for k in range(len(loss_trace)):
            print("accepted %3d  loss %.6e  lambda %.1e  theta %s" % (k, loss_trace[k], r["lambda_trace"][k], np.array2string(parameter_trace[k], precision=4)))
        print("%d evaluations, %d rejected%s" % (r["evaluations"], r["rejected"], ", stalled" if r["stalled"] else ""))
        if a.covariance:
            c = loop.covariance(noise)
            print("theta %s  (noise %s, sigma^2 %.3e)  pivot_ratio %.2e" % ("  ".join("%.5f +- %.1e" % (v, e) for v, e in zip(parameter_trace[-1], c["std_err"])), noise,
                                                                            c["sigma2"], c["pivot_ratio"]))
        theta, a.iters = parameter_trace[-1], len(loss_trace)
    elif a.graph:
        from pdp_amd import runtime as rt
        from pdp_amd.irl import GDLoop
        mdl = sid.model()
        u_d, x_d = rt.dev(np.stack(batch_inputs)), rt.dev(np.stack(batch_states))
        loop = GDLoop(lambda th: mdl.sysid_step(u_d, x_d, th), theta, a.lr, max_steps=a.iters + 8)
        loop.run(a.iters)
        r = loop.results()
        loss_trace, parameter_trace = list(r["loss_trace"][:a.iters]), list(r["parameter_trace"][:a.iters])
        theta = parameter_trace[-1]
        for k in range(0, a.iters, max(1, a.iters // 10)):
            print("iter %5d  loss %.6e  theta %s" % (k, loss_trace[k], np.array2string(parameter_trace[k], precision=4)))
    for k in range(0 if not (a.graph or a.method == "lm") else a.iters, a.iters):
        loss, dp = sid.step(batch_inputs, batch_states, theta)
        theta = theta - a.lr * dp
        loss_trace.append(loss)
        parameter_trace.append(theta.copy())
        if k % max(1, a.iters // 10) == 0:
            print("iter %5d  loss %.6e  theta %s" % (k, loss, np.array2string(theta, precision=4)))
    save = {"trail_no": 0, "loss_trace": loss_trace, "parameter_trace": parameter_trace, "learning_rate": a.lr, "time_passed": time.time() - t0}
    if a.out:
        sio.savemat(a.out, {"results": save})
    print("done: %d iterations in %.2f s; loss %.4e -> %.4e; |theta - theta*| = %.4f" % (a.iters, save["time_passed"], loss_trace[0], loss_trace[-1],
                                                                                         np.abs(theta - true_parameter).max()))
    return loss_trace


if __name__ == "__main__":
    main()
